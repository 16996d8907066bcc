// K27: cleaning the footprints -- median filter, energy (or maximum) cut, morphological closing, largest face-connected part
// (dnmf_clean_footprints).  include/dnmf_hip.h has the contract, tests/footprint_clean_restatement.py the definition.  Every output
// is an integer or a bit pattern; the kernel's only floating-point arithmetic is the sequential float64 sum of squares of the cut
// and two float64 products.
//
// Clean.  One workgroup of FC_THREADS lanes per neuron, its box (at most BOX_MAX_VOXELS voxels, x slowest) in LDS; a lane takes the
// box voxels lane, lane + FC_THREADS, ...
//   median    27 (Z == 1: 9) taps from global memory, as 32-bit keys in IEEE totalOrder, sorted in registers by an odd-even
//             transposition network of constant indices; the middle key is the median;
//   cut       'nrg': the box values as 64-bit keys, block_sort_keys, then ONE lane adds the squares from the top in float64 --
//             np.cumsum's additions, in its order -- once for the total and once up to the first index that reaches nrgthr * total.
//             Zeros add nothing, so both walks stop after the positive values.  'max': a max-reduction and one product;
//   closing   dilation and erosion read one byte mask and write another: 27 LDS reads a voxel each;
//   parts     minimum-label propagation over the face neighbours with one pointer jump, in two phases (every lane reads, a barrier,
//             every lane writes) until a block-wide flag stays clear -- at most n rounds; labels only decrease and are indices of
//             voxels of the same part, so the fixed point is the part's lowest index under any schedule.  Sizes by integer LDS
//             atomics; the largest part, a tie to the lowest index, by a max-reduction of (size, ~index).
// The result goes to a compact (K, BOX_MAX_VOXELS) buffer, the statistics to (K, 6) ints and (K, 2) doubles.
//
// Scatter.  One thread per entry of the (P, K) output, K fastest: the compact value inside the neuron's box, 0 outside, the input's
// own bits for a neuron that was refused (ok = 0).  An entry is read and written by the same thread: out may be A itself.
//
// No floating-point atomics, no scratch.
#include "block_ops.hpp"
#include "boxes.hpp"

namespace dnmf {
namespace {

constexpr int FC_THREADS = 256, FC_WAVES = FC_THREADS / 64;
constexpr int FC_PER_LANE = BOX_MAX_VOXELS / FC_THREADS;
constexpr int FC_ISTATS = 6, FC_DSTATS = 2;                        // ok, n_box, n_cut, n_closed, n_parts, n_kept; threshold, energy
constexpr int FC_NONE = 0x7fffffff;                                // the label of a voxel outside the mask

struct CleanArgs {
    const float *A;
    long lda;
    const int *boxes;
    int X, Y, Z;
    int method, median, closing, values;
    double nrgthr, maxthr;
    float *comp;            // (K, BOX_MAX_VOXELS)
    int *istats;            // (K, FC_ISTATS)
    double *dstats;         // (K, FC_DSTATS)
};

struct OpMaxKey {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

// fp32 <-> 32-bit key in IEEE totalOrder, every NaN the top key (block_ops.hpp's to_key for a float)
__device__ __forceinline__ uint32_t key32(float f) {
    if (f != f) return ~0u;
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value32(uint32_t k) {
    if (k == ~0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

// the median of the 3 x 3 x NZ neighbourhood of (x, y, z) in the volume, coordinates clamped to it
template <int NZ>
__device__ __forceinline__ float median_at(const float *col, long lda, int x, int y, int z, int X, int Y, int Z) {
    constexpr int N = 9 * NZ;
    uint32_t w[N];
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dz = 0; dz < NZ; ++dz) {
                const int xi = min(max(x + dx, 0), X - 1), yi = min(max(y + dy, 0), Y - 1);
                const int zi = NZ == 1 ? z : min(max(z + dz - 1, 0), Z - 1);
                w[((dx + 1) * 3 + dy + 1) * NZ + dz] = key32(col[((long)(xi * Y + yi) * Z + zi) * lda]);
            }
#pragma unroll
    for (int pass = 0; pass < N; ++pass)
#pragma unroll
        for (int i = pass & 1; i + 1 < N; i += 2) {
            const uint32_t a = w[i], b = w[i + 1];
            w[i] = min(a, b), w[i + 1] = max(a, b);
        }
    return value32(w[N / 2]);
}

// bit 0: a value that is not finite or is negative; bit 1: a positive value
__device__ __forceinline__ uint64_t judge(float v) {
    return (uint64_t)(!__builtin_isfinite(v) || v < 0.0f) | ((uint64_t)(v > 0.0f) << 1);
}

__global__ __launch_bounds__(FC_THREADS) void clean_footprints_kernel(CleanArgs g) {
    __shared__ float m[BOX_MAX_VOXELS];
    __shared__ uint64_t key[BOX_MAX_VOXELS];              // the sort of the cut; after it the labels and the part sizes
    __shared__ uint8_t keep[BOX_MAX_VOXELS], closed[BOX_MAX_VOXELS];
    __shared__ uint64_t red[FC_WAVES];
    __shared__ double cut[2];                            // threshold, energy
    int *lab = reinterpret_cast<int *>(key), *cnt = lab + BOX_MAX_VOXELS;
    uint8_t *dil = reinterpret_cast<uint8_t *>(cnt);

    const int tid = threadIdx.x;
    const long k = blockIdx.x;
    const int *b = g.boxes + 6 * k;
    // all three extents are needed below (the closing and the parts walk the box itself), so not boxes.hpp's Box
    const int x0 = b[0], y0 = b[2], z0 = b[4];
    const int ex = b[1] - x0 + 1, ey = b[3] - y0 + 1, ez = b[5] - z0 + 1;
    const int n = ex * ey * ez;                          // the host has checked the boxes: 1 <= n <= BOX_MAX_VOXELS, inside the volume
    const float *col = g.A + k;
    int *ist = g.istats + FC_ISTATS * k;
    double *dst = g.dstats + FC_DSTATS * k;

    // 1. the box values, and whether they can be cleaned at all
    uint64_t flags = 0;
    for (int v = tid; v < n; v += FC_THREADS) {
        const int bz = v % ez, r = v / ez, by = r % ey, bx = r / ey;
        const float a = col[((long)((x0 + bx) * g.Y + y0 + by) * g.Z + z0 + bz) * g.lda];
        m[v] = a;
        flags |= judge(a);
    }
    flags = block_reduce<FC_THREADS>(flags, OpOr(), red);
    // 2. the median, from the volume: m is written by its owner only and nobody reads it here
    if (flags == 2 && g.median) {
        flags = 0;
        for (int v = tid; v < n; v += FC_THREADS) {
            const int bz = v % ez, r = v / ez, by = r % ey, bx = r / ey;
            const int x = x0 + bx, y = y0 + by, z = z0 + bz;
            const float a = g.Z == 1 ? median_at<1>(col, g.lda, x, y, z, g.X, g.Y, g.Z) : median_at<3>(col, g.lda, x, y, z, g.X, g.Y, g.Z);
            m[v] = a;
            flags |= judge(a);
        }
        flags = block_reduce<FC_THREADS>(flags, OpOr(), red);
    }
    int n_cut = 0;
    if (flags == 2) {
        // 3. the cut
        if (g.method == 0) {
            int npos = 0;
            for (int v = tid; v < n; v += FC_THREADS) {
                key[v] = to_key((double)m[v]);
                npos += m[v] > 0.0f;
            }
            npos = block_reduce<FC_THREADS>(npos, OpSum(), red);
            block_sort_keys<FC_THREADS>(key, n);
            if (tid == 0) {
                double total = 0.0;
                for (int i = 0; i < npos; ++i) {
                    const double v = from_key(key[n - 1 - i]);
                    total += v * v;
                }
                const double target = g.nrgthr * total;
                double cum = 0.0, thr = 0.0;
                for (int i = 0; i < npos; ++i) {
                    thr = from_key(key[n - 1 - i]);
                    cum += thr * thr;
                    if (cum >= target) break;
                }
                cut[0] = thr, cut[1] = cum / total;
            }
            __syncthreads();
        } else {
            double mx = 0.0;
            for (int v = tid; v < n; v += FC_THREADS) mx = fmax(mx, (double)m[v]);
            mx = block_reduce<FC_THREADS>(mx, OpFmax(), red);
            if (tid == 0) cut[0] = g.maxthr * mx, cut[1] = quiet_nan();
            __syncthreads();
        }
        const double thr = cut[0];
        for (int v = tid; v < n; v += FC_THREADS) {
            const float a = m[v];
            const bool on = g.method == 0 ? ((double)a >= thr && a > 0.0f) : (double)a > thr;
            keep[v] = on;
            n_cut += on;
        }
        n_cut = block_reduce<FC_THREADS>(n_cut, OpSum(), red);     // its barriers: keep is visible, the sort keys are free
    }
    if (n_cut == 0) {                                    // refused, the whole workgroup alike: the scatter copies the column
        if (tid == 0) {
            ist[0] = 0, ist[1] = n, ist[2] = 0, ist[3] = 0, ist[4] = 0, ist[5] = 0;
            dst[0] = quiet_nan(), dst[1] = quiet_nan();
        }
        return;
    }

    // 4. closing: dil = or of keep over the neighbourhood inside the box, closed = and of dil over it
    if (g.closing) {
        for (int v = tid; v < n; v += FC_THREADS) {
            const int bz = v % ez, r = v / ez, by = r % ey, bx = r / ey;
            int any = 0;
            for (int xx = max(bx - 1, 0); xx <= min(bx + 1, ex - 1); ++xx)
                for (int yy = max(by - 1, 0); yy <= min(by + 1, ey - 1); ++yy)
                    for (int zz = max(bz - 1, 0); zz <= min(bz + 1, ez - 1); ++zz) any |= keep[(xx * ey + yy) * ez + zz];
            dil[v] = (uint8_t)any;
        }
        __syncthreads();
        for (int v = tid; v < n; v += FC_THREADS) {
            const int bz = v % ez, r = v / ez, by = r % ey, bx = r / ey;
            int all = 1;
            for (int xx = max(bx - 1, 0); xx <= min(bx + 1, ex - 1); ++xx)
                for (int yy = max(by - 1, 0); yy <= min(by + 1, ey - 1); ++yy)
                    for (int zz = max(bz - 1, 0); zz <= min(bz + 1, ez - 1); ++zz) all &= dil[(xx * ey + yy) * ez + zz];
            closed[v] = (uint8_t)all;
        }
    } else {
        for (int v = tid; v < n; v += FC_THREADS) closed[v] = keep[v];
    }
    __syncthreads();                                     // closed is visible, dil is free

    // 5. the parts
    int n_closed = 0;
    for (int v = tid; v < n; v += FC_THREADS) {
        lab[v] = closed[v] ? v : FC_NONE;
        cnt[v] = 0;
        n_closed += closed[v];
    }
    n_closed = block_reduce<FC_THREADS>(n_closed, OpSum(), red);
    for (int round = 0; round < n; ++round) {
        int best[FC_PER_LANE];
#pragma unroll
        for (int q = 0; q < FC_PER_LANE; ++q) {
            const int v = tid + q * FC_THREADS;
            best[q] = FC_NONE;
            if (v < n && closed[v]) {
                const int bz = v % ez, r = v / ez, by = r % ey, bx = r / ey;
                int l = lab[v];
                if (bx > 0) l = min(l, lab[v - ey * ez]);         // a neighbour outside the mask holds FC_NONE
                if (bx < ex - 1) l = min(l, lab[v + ey * ez]);
                if (by > 0) l = min(l, lab[v - ez]);
                if (by < ey - 1) l = min(l, lab[v + ez]);
                if (bz > 0) l = min(l, lab[v - 1]);
                if (bz < ez - 1) l = min(l, lab[v + 1]);
                best[q] = lab[l];                                 // l is a voxel of this part, and lab[l] <= l
            }
        }
        __syncthreads();                                 // every read of this round is done
        int changed = 0;
#pragma unroll
        for (int q = 0; q < FC_PER_LANE; ++q) {
            const int v = tid + q * FC_THREADS;
            if (v < n && best[q] < lab[v]) lab[v] = best[q], changed = 1;
        }
        if (block_reduce<FC_THREADS>(changed, OpSum(), red) == 0) break;
    }
    for (int v = tid; v < n; v += FC_THREADS)
        if (closed[v]) atomicAdd(&cnt[lab[v]], 1);
    __syncthreads();
    int n_parts = 0;
    uint64_t top = 0;
    for (int v = tid; v < n; v += FC_THREADS)
        if (closed[v] && lab[v] == v) {
            ++n_parts;
            const uint64_t cand = ((uint64_t)cnt[v] << 32) | (uint32_t)(BOX_MAX_VOXELS - v);    // larger size, then lower index
            top = cand > top ? cand : top;
        }
    n_parts = block_reduce<FC_THREADS>(n_parts, OpSum(), red);
    top = block_reduce<FC_THREADS>(top, OpMaxKey(), red);
    const int winner = BOX_MAX_VOXELS - (int)(uint32_t)top, n_kept = (int)(top >> 32);

    // 6. the values
    float *comp = g.comp + BOX_MAX_VOXELS * k;
    for (int v = tid; v < n; v += FC_THREADS) {
        float a = 0.0f;
        if (closed[v] && lab[v] == winner) {
            a = m[v];
            if (g.values == 1 && g.median) {
                const int bz = v % ez, r = v / ez, by = r % ey, bx = r / ey;
                a = col[((long)((x0 + bx) * g.Y + y0 + by) * g.Z + z0 + bz) * g.lda];
            }
        }
        comp[v] = a;
    }
    if (tid == 0) {
        ist[0] = 1, ist[1] = n, ist[2] = n_cut, ist[3] = n_closed, ist[4] = n_parts, ist[5] = n_kept;
        dst[0] = cut[0], dst[1] = cut[1];
    }
}

struct ScatterArgs {
    const float *A, *comp;
    float *out;
    long lda, ldo, P;
    const int *boxes, *istats;
    int K, Y, Z;
};

__global__ __launch_bounds__(FC_THREADS) void scatter_footprints_kernel(ScatterArgs g) {
    const long e = (long)blockIdx.x * FC_THREADS + threadIdx.x;
    if (e >= g.P * g.K) return;
    const long p = e / g.K;
    const int k = (int)(e % g.K);
    float a;
    if (g.istats[FC_ISTATS * k] == 0) {
        a = g.A[p * g.lda + k];
    } else {
        const int z = (int)(p % g.Z), r = (int)(p / g.Z), y = r % g.Y, x = r / g.Y;
        const int *b = g.boxes + 6 * k;
        const bool inside = x >= b[0] && x <= b[1] && y >= b[2] && y <= b[3] && z >= b[4] && z <= b[5];
        a = inside ? g.comp[(long)BOX_MAX_VOXELS * k + ((x - b[0]) * (b[3] - b[2] + 1) + y - b[2]) * (b[5] - b[4] + 1) + z - b[4]] : 0.0f;
    }
    g.out[p * g.ldo + k] = a;
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_clean_footprints_workspace(int K) {
    if (K < 1) {
        dnmf::fail(DNMF_E_SHAPE, "dnmf_clean_footprints_workspace: K=%d neurons", K);
        return 0;
    }
    return sizeof(float) * dnmf::BOX_MAX_VOXELS * (size_t)K;
}

int dnmf_clean_footprints(const float *A, long lda, const int *sz, const int *boxes, const int *boxes_dev, int K, int method,
                          double nrgthr, double maxthr, int median, int closing, int values, float *out, long ldo, int *istats,
                          double *dstats, void *workspace, size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_clean_footprints";
    DNMF_REQUIRE(A && sz && boxes && boxes_dev && out && istats && dstats && workspace, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(K >= 1, DNMF_E_SHAPE, "%s: K=%d neurons", fn, K);
    const int X = sz[0], Y = sz[1], Z = sz[2];
    const long P = (long)X * Y * Z;
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    DNMF_REQUIRE(lda >= K && ldo >= K, DNMF_E_SHAPE, "%s: lda=%ld or ldo=%ld below a row of K=%d", fn, lda, ldo, K);
    DNMF_REQUIRE((method == 0 || method == 1) && (median == 0 || median == 1) && (closing == 0 || closing == 1) &&
                     (values == 0 || values == 1),
                 DNMF_E_SHAPE, "%s: method=%d, median=%d, closing=%d, values=%d: each is 0 or 1", fn, method, median, closing, values);
    DNMF_REQUIRE(method == 1 || (nrgthr > 0.0 && nrgthr <= 1.0), DNMF_E_SHAPE, "%s: nrgthr=%g outside (0, 1]", fn, nrgthr);
    DNMF_REQUIRE(method == 0 || maxthr >= 0.0, DNMF_E_SHAPE, "%s: maxthr=%g, not >= 0", fn, maxthr);
    const int rb = check_boxes(fn, sz, boxes, K, BOX_MAX_VOXELS, DNMF_E_SHAPE);
    if (rb != DNMF_OK) return rb;
    const size_t need = dnmf_clean_footprints_workspace(K);
    DNMF_REQUIRE(workspace_bytes >= need, DNMF_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu", fn, workspace_bytes, need);
    DNMF_REQUIRE(((size_t)workspace & 3) == 0, DNMF_E_WORKSPACE, "%s: workspace must be 4-byte aligned", fn);
    // out is A itself (an entry is read and written by one thread) or apart from it
    const char *alo = reinterpret_cast<const char *>(A), *ahi = alo + sizeof(float) * (size_t)((P - 1) * lda + K);
    const char *olo = reinterpret_cast<const char *>(out), *ohi = olo + sizeof(float) * (size_t)((P - 1) * ldo + K);
    DNMF_REQUIRE((out == A && ldo == lda) || ohi <= alo || ahi <= olo, DNMF_E_SHAPE,
                 "%s: out overlaps A without being A itself (same pointer, same row stride)", fn);
    const long blocks = (P * K + FC_THREADS - 1) / FC_THREADS;
    DNMF_REQUIRE(blocks < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld entries to write", fn, P * K);

    CleanArgs g;
    g.A = A, g.lda = lda, g.boxes = boxes_dev, g.X = X, g.Y = Y, g.Z = Z;
    g.method = method, g.median = median, g.closing = closing, g.values = values, g.nrgthr = nrgthr, g.maxthr = maxthr;
    g.comp = static_cast<float *>(workspace), g.istats = istats, g.dstats = dstats;
    hipLaunchKernelGGL(clean_footprints_kernel, dim3((unsigned)K), dim3(FC_THREADS), 0, (hipStream_t)stream, g);
    const int rc = check_launch(fn);
    if (rc != DNMF_OK) return rc;
    ScatterArgs s;
    s.A = A, s.comp = g.comp, s.out = out, s.lda = lda, s.ldo = ldo, s.P = P, s.boxes = boxes_dev, s.istats = istats;
    s.K = K, s.Y = Y, s.Z = Z;
    hipLaunchKernelGGL(scatter_footprints_kernel, dim3((unsigned)blocks), dim3(FC_THREADS), 0, (hipStream_t)stream, s);
    return check_launch(fn);
}

}  // extern "C"
