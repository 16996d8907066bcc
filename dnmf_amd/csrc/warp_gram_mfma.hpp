// What the Gram kernels on the matrix pipe share -- K3 / K3b (warp_gram_rhs.hip) and both K3s variants
// (warp_gram_sparse.hip): a wave is one work item (a chunk of 64-voxel patches of one frame), one lane computes the
// warp of one voxel per coordinate pass and parks the record in wave-private LDS; on the host, the patch shape, the
// chunk plan and the argument checks of the entry points.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace dnmf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int GRAM_SS = 64;  // voxels per coordinate pass (one per lane)

// upper-triangle tile (bi <= bj) of an NB x NB grid of 16x16 tiles
__host__ __device__ constexpr int tile_index(int NB, int bi, int bj) { return bi * NB - bi * (bi - 1) / 2 + (bj - bi); }

// Kernel arguments every one of these kernels takes (embedded in GramParams / SparseParams behind the footprint fields)
struct GramCommon {
    Volume vol;
    const float *beta;
    int T;
    const int *times;
    int B;
    const float *frames;
    long ldf;
    const int *frame_ids;
    float *slab;       // (B, nchunks, floats of one work item); the layout of an item is the kernel's own
    int nchunks;
    long chunk_len;    // passes (patches of 64 voxels) per chunk
    // a pass is a compact patch of 2^lgx x 2^lgy x 2^lgz = 64 voxels (8x8 for Z == 1), not a run of 64 voxels: its
    // gathers touch ~80 distinct footprint rows instead of ~130, so more of them hit in L1, and fewer footprints reach
    // into it, so K3s has fewer active blocks and tiles per pass
    int lgy, lgz, npy, npz;
    long npatch;
};

// The work-item prologue and the patch walk are NOT shared: each of the four kernels keeps its own copy.  Moving them
// into a struct here (force-inlined, by reference) changed the instruction order or the register allocation of every
// compute kernel, and so did a shared coordinate pass in K3s (voxel_record below serves K3 / K3b); they stay in the kernels until a change of theirs can be timed.

// Voxel record of the coordinate pass: byte offsets of the NTAP footprint rows, their weights (0 outside the volume,
// and for a voxel of a patch that sticks out of the volume) and the frame value.  NTAP = 4 (Z == 1, bilinear) or 8
// (trilinear); tap c: dx = c&1, dy = (c>>1)&1, dz = c>>2 (ATen's corner order).  `bt` NULL: no warp.
template <int NTAP>
__device__ __forceinline__ void voxel_record(const float *bt, const Volume &vol, unsigned row_bytes,
                                             const float *__restrict__ yb, int x, int y, int z, unsigned (&rows)[NTAP],
                                             float (&w)[NTAP], float &yv) {
#pragma unroll
    for (int c = 0; c < NTAP; ++c) rows[c] = 0u, w[c] = 0.0f;
    yv = 0.0f;
    if (x < vol.X && y < vol.Y && z < vol.Z) {
        unsigned voxs[NTAP];
        if (bt) {
            const Sample sm = make_sample_t<(NTAP == 8)>(bt, vol, x, y, z);
            make_taps<NTAP>(sm, vol, w, voxs);
        } else {   // no warp (beta == NULL): the footprint row of the voxel itself, weight 1 -- exact on any lattice
            const unsigned self = (unsigned)((x * vol.Y + y) * vol.Z + z);
#pragma unroll
            for (int c = 0; c < NTAP; ++c) voxs[c] = self, w[c] = c == 0 ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < NTAP; ++c) rows[c] = voxs[c] * row_bytes;
        yv = yb[((long)x * vol.Y + y) * vol.Z + z];
    }
}

// LDS traffic of one wave is processed in order; only the compiler has to be kept from reordering
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- host: patch shape and chunk plan --------------------------------------------------------------------------
inline void patch_shape(GramCommon &c) {
    const Volume &vol = c.vol;
    c.lgz = vol.Z == 1 ? 0 : (vol.Z == 2 ? 1 : 2);
    c.lgy = vol.Z <= 2 ? 3 : 2;
    const int lgx = 6 - c.lgy - c.lgz;
    c.npz = (vol.Z + (1 << c.lgz) - 1) >> c.lgz;
    c.npy = (vol.Y + (1 << c.lgy) - 1) >> c.lgy;
    c.npatch = (long)((vol.X + (1 << lgx) - 1) >> lgx) * c.npy * c.npz;
}

constexpr int GRAM_ITEMS_DENSE = 4096;   // aim for >= 4096 wave-sized work items
constexpr int GRAM_ITEMS_SPARSE = 8192;  // passes differ a lot in cost: more, smaller work items than the dense kernel

// upper bound of the chunk count chosen at launch (which also depends on the shape): what a workspace is sized for
inline long max_chunks(int B, int target_items) {
    const long want = (target_items + B - 1) / B;
    return want < 1 ? 1 : (want > 64 ? 64 : want);
}

inline void choose_chunks(long npatch, int B, int target_items, int &nchunks, long &chunk_len) {
    long want = max_chunks(B, target_items);
    if (want > npatch) want = npatch;
    chunk_len = (npatch + want - 1) / want;  // coordinate passes per chunk
    nchunks = (int)((npatch + chunk_len - 1) / chunk_len);
}

// ---- host: entry points ----------------------------------------------------------------------------------------
// The argument checks the entry points share, in the order they have always been made, and the common block filled
// (chunk plan included).  `A` is the footprint buffer with rows of `Kp` floats (`kname`: what the entry calls Kp),
// `kp_max` the widest row the entry takes (0: checked by its dispatch); `a_vec`: A is read with 16-byte loads, one copy
// per frame `a_stride` floats apart.
inline int gram_common_args(const char *who, const char *kname, GramCommon &c, const void *A, int Kp, int kp_want,
                            int kp_max, bool a_vec, long a_stride, int K, int X, int Y, int Z,
                            const float *beta, int T, const int *times, int B, const float *frames, long ldf,
                            const int *frame_ids, const float *G, const float *r, void *workspace, int target_items) {
    DNMF_REQUIRE(A && frames && G && r && workspace, DNMF_E_NULL, "%s: NULL buffer", who);
    DNMF_REQUIRE(X > 0 && Y > 0 && Z > 0 && K > 0 && T > 0 && B > 0 && Kp == kp_want, DNMF_E_SHAPE,
                 "%s: X=%d Y=%d Z=%d K=%d %s=%d T=%d B=%d", who, X, Y, Z, K, kname, Kp, T, B);
    DNMF_REQUIRE(kp_max == 0 || Kp <= kp_max, DNMF_E_UNSUPPORTED, "%s: K=%d > %d", who, K, kp_max);
    c.vol = make_volume(X, Y, Z);
    DNMF_REQUIRE(ldf >= c.vol.P && a_stride >= 0, DNMF_E_SHAPE, "%s: ldf=%ld < P=%ld", who, ldf, c.vol.P);
    DNMF_REQUIRE(c.vol.P * Kp < (1L << 30), DNMF_E_UNSUPPORTED, "%s: P*%s=%ld %s", who, kname, c.vol.P * Kp,
                 a_vec ? "does not fit 32-bit byte offsets" : "too large");
    DNMF_REQUIRE((!a_vec || ((reinterpret_cast<size_t>(A) & 15) == 0 && (a_stride % 4) == 0)) &&
                     (reinterpret_cast<size_t>(workspace) & 15) == 0,
                 DNMF_E_SHAPE, "%s: %s workspace must be 16-byte aligned", who, a_vec ? "Apk /" : "the");
    c.beta = beta, c.T = T, c.times = times, c.B = B;
    c.frames = frames, c.ldf = ldf, c.frame_ids = frame_ids;
    c.slab = static_cast<float *>(workspace);
    patch_shape(c);
    choose_chunks(c.npatch, B, target_items, c.nchunks, c.chunk_len);
    return DNMF_OK;
}

// f(std::integral_constant<int, NB>) for the block counts the kernels are built for; false for any other NB
template <class F>
inline bool dispatch_nb(int NB, int &rc, F &&f) {
    switch (NB) {
        case 1: rc = f(std::integral_constant<int, 1>{}); return true;
        case 2: rc = f(std::integral_constant<int, 2>{}); return true;
        case 3: rc = f(std::integral_constant<int, 3>{}); return true;
        case 4: rc = f(std::integral_constant<int, 4>{}); return true;
        case 5: rc = f(std::integral_constant<int, 5>{}); return true;
        case 6: rc = f(std::integral_constant<int, 6>{}); return true;
        case 7: rc = f(std::integral_constant<int, 7>{}); return true;
        case 8: rc = f(std::integral_constant<int, 8>{}); return true;
        default: return false;
    }
}

}  // namespace dnmf
