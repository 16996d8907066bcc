// The per-component box of K24, K26, K27 and K28: six ints (x0, x1, y0, y1, z0, z1), both ends inclusive, its voxels numbered x
// slowest, z fastest.  The host check of a caller's boxes, and the device's decoding of one.
#pragma once

#include "common.hpp"

namespace dnmf {

// K24 keeps a lane's voxels of a box in registers, at most 16 for each of 256 lanes; K27 holds the whole box in LDS.
constexpr int BOX_MAX_VOXELS = 4096;

// The n boxes of a host array lie inside the volume sz, are not empty and hold at most `limit` voxels each; a larger one is
// reported with the code `too_large`, the limit named by `limit_text`.  vmax, where given: the largest voxel count.
inline int check_boxes(const char *fn, const int *sz, const int *boxes, int n, int limit, int too_large,
                       const char *limit_text = "at most ", int *vmax = nullptr) {
    int largest = 0;
    for (int k = 0; k < n; ++k) {
        const int *b = boxes + 6 * (long)k;
        const bool inside = b[0] >= 0 && b[1] < sz[0] && b[2] >= 0 && b[3] < sz[1] && b[4] >= 0 && b[5] < sz[2];
        DNMF_REQUIRE(inside && b[0] <= b[1] && b[2] <= b[3] && b[4] <= b[5], DNMF_E_SHAPE,
                     "%s: box %d = x %d..%d, y %d..%d, z %d..%d is empty or outside the volume %dx%dx%d", fn, k, b[0], b[1], b[2], b[3],
                     b[4], b[5], sz[0], sz[1], sz[2]);
        const long nb = (long)(b[1] - b[0] + 1) * (b[3] - b[2] + 1) * (b[5] - b[4] + 1);
        DNMF_REQUIRE(nb <= limit, too_large, "%s: box %d holds %ld voxels, %s%d", fn, k, nb, limit_text, limit);
        if ((int)nb > largest) largest = (int)nb;
    }
    if (vmax) *vmax = largest;
    return DNMF_OK;
}

struct Box {
    int x0, y0, z0, ey, ez, n;
};

__device__ __forceinline__ Box load_box(const int *b) {
    Box q;
    q.x0 = b[0], q.y0 = b[2], q.z0 = b[4];
    q.ey = b[3] - b[2] + 1, q.ez = b[5] - b[4] + 1;
    q.n = (b[1] - b[0] + 1) * q.ey * q.ez;
    return q;
}

// voxel i of the box (x slowest, z fastest) -> its offset inside a frame
__device__ __forceinline__ int box_offset(const Box &q, int i, int Y, int Z) {
    const int bz = i % q.ez, r = i / q.ez, by = r % q.ey, bx = r / q.ey;
    return ((q.x0 + bx) * Y + q.y0 + by) * Z + q.z0 + bz;
}

}  // namespace dnmf
