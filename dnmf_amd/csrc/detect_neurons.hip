// K14: neuron centres of a template volume by a greedy matched-filter pursuit (tests/detect_restatement.py is the
// definition, in float64; everything here is fp32).
//
// The footprint model exp(-|x - p|^2 / sigma^2) (Demix/dNMF.py:39-40) is its own matched filter.  With g1(d) = exp(-d^2 /
// sigma^2) and r = ceil(3 sigma):
//   filter   R = g (*) (V - background), separable, truncated at r voxels per axis, zero padding: two launches -- the y pass,
//            which folds the z pass into its loads (z is the contiguous axis and usually 1 or 2 voxels long), then the x pass.
//            A block stages its tile plus the 2 r rows around it in LDS and reads each of them once (the halo is re-read by
//            the neighbouring blocks, from L2); the r + 1 taps are made by every block into LDS.  What is stored is the SCORE
//            S = R prod_axis sqrt(nmax / n(q)), n(q) = sum of the squared taps that fall inside the volume at q and nmax its
//            value in the middle of the axis: S = R wherever the window is inside the volume, and under white noise S has the
//            same variance everywhere, so a blob cut by the border competes, and is located, on equal terms (S / sqrt(nmax n)
//            peaks exactly at the centre of an isolated truncated blob; R peaks up to a voxel inside it).  n(q) comes from
//            the running sums of the squared taps.
//   table    per tile of 16 x 16 x 4 voxels the largest score and its linear index (equal scores: the lowest index).
//   pursuit  ONE workgroup of 1024 threads loops K times with no host round trip: arg-max of the table, sub-voxel refinement
//            of the peak (log-parabola per axis), the least-squares amplitude of the truncated footprint, subtraction of the
//            filter's response to that footprint through per-axis tables h_axis in LDS, exclusion (-inf) of the voxels within
//            min_distance, and the new maxima of the tiles the window touched.  The steps are separated by __syncthreads; R
//            and the table live in the caller's workspace and are only touched by this workgroup.
#include "block_ops.hpp"
#include "matched_filter.hpp"

namespace dnmf {
namespace {

constexpr int DT_R_MAX = MF_R_MAX; // taps per side: sigma <= 32
constexpr int DT_WR_MAX = 511;    // half-width of the pursuit's window: max(2 r, what min_distance reaches)
constexpr int DT_TX = 16, DT_TY = 16, DT_TZ = 4;   // a tile of the table
constexpr int DT_TILE_OUT = 1024; // outputs of a filter block
constexpr int DT_THREADS = 1024;  // the pursuit's workgroup
constexpr int DT_WAVES = DT_THREADS / 64;

struct DetectGeom {
    int X, Y, Z;
    int r, wr;
    int ntx, nty, ntz, ntiles;
    float inv_s2;     // 1 / sigma^2
    float md2;        // min_distance^2
    float threshold;
};

// One wave: the pair of tile `t` of the table, valid in lane 63.  NaN scores never win: a tile of nothing but NaN reports
// (-inf, INT_MAX), a tile of excluded voxels (-inf, its lowest voxel).
__device__ __forceinline__ void tile_argmax(const float *R, const DetectGeom &g, int t, int lane, float &bv, int &bi) {
    const int tz = t % g.ntz, ty = (t / g.ntz) % g.nty, tx = t / (g.ntz * g.nty);
    const int x0 = tx * DT_TX, y0 = ty * DT_TY, z0 = tz * DT_TZ;
    const int ex = min(DT_TX, g.X - x0), ey = min(DT_TY, g.Y - y0), ez = min(DT_TZ, g.Z - z0);
    const int n = ex * ey * ez;
    bv = -__builtin_inff(), bi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const int lz = i % ez, ly = (i / ez) % ey, lx = i / (ez * ey);
        const int idx = ((x0 + lx) * g.Y + (y0 + ly)) * g.Z + (z0 + lz);
        const float v = R[idx];
        if (better(v, idx, bv, bi)) bv = v, bi = idx;
    }
    wave_argmax_last(bv, bi);
}

// ---- filter ----------------------------------------------------------------------------------------------------------
// The volume as (A, S, B): element (a, s, b) at (a S + s) B + b; the pass runs along s.  A block makes `rows` x `bw`
// outputs of one a (rows <= ts, bw <= tbw <= 64, ts tbw <= DT_TILE_OUT) from the (rows + 2 r) x bw inputs staged in LDS,
// rows outside the volume as zeros, each times the weight sqrt(nmax / n) of its place along s.  LOADZ: B is the z axis and
// what is staged is the (weighted) z pass of (in - background), made from the global values (the whole z window of a voxel
// lies in one or two cache lines).
template <bool LOADZ>
__global__ __launch_bounds__(256) void filter_axis_kernel(const float *__restrict__ in, float *__restrict__ out, int S, int B, int ts,
                                                           int tbw, int nsb, int nbb, int r, float inv_s2, float background) {
    extern __shared__ float lds[];
    float *tap = lds;                       // r + 1
    float *c2 = lds + ((r + 4) & ~3);       // r + 1 running sums of tap^2
    float *tile = lds + 2 * ((r + 4) & ~3); // (rows + 2 r) x bw
    const int tid = threadIdx.x;
    fill_taps(tap, c2, r, inv_s2, tid, 256);
    const int bb = blockIdx.x % nbb, sb = (blockIdx.x / nbb) % nsb, a = blockIdx.x / (nbb * nsb);
    const int s0 = sb * ts, b0 = bb * tbw;
    const int rows = min(ts, S - s0), bw = min(tbw, B - b0);
    __syncthreads();
    const int nload = (rows + 2 * r) * bw;
    for (int e = tid; e < nload; e += 256) {
        const int sl = e / bw, bl = e - sl * bw;
        const int s = s0 - r + sl;
        float v = 0.0f;
        if (in_range(s, S)) {
            const long base = ((long)a * S + s) * B;
            if (LOADZ) {
                const int z = b0 + bl;
                const int zhi = min(B - 1, z + r);
                for (int zz = max(0, z - r); zz <= zhi; ++zz) v += tap[abs(zz - z)] * (in[base + zz] - background);
                v *= axis_weight(c2, r, z, B);
            } else {
                v = in[base + b0 + bl];
            }
        }
        tile[e] = v;
    }
    __syncthreads();
    const int nout = rows * bw;
    for (int e = tid; e < nout; e += 256) {
        const int sl = e / bw, bl = e - sl * bw;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * r; ++k) acc += tap[abs(k - r)] * tile[(sl + k) * bw + bl];
        out[((long)a * S + s0 + sl) * B + b0 + bl] = acc * axis_weight(c2, r, s0 + sl, S);
    }
}

// ---- table -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tile_table_kernel(const float *__restrict__ R, DetectGeom g, float *__restrict__ tmax,
                                                          int *__restrict__ tidx) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= g.ntiles) return;     // whole waves leave together
    float bv;
    int bi;
    tile_argmax(R, g, t, threadIdx.x & 63, bv, bi);
    if ((threadIdx.x & 63) == 63) tmax[t] = bv, tidx[t] = bi;
}

// ---- pursuit ---------------------------------------------------------------------------------------------------------
// R, tmax, tidx, positions are read back after this workgroup wrote them: no __restrict__, and every such hand-over has a
// __syncthreads between the stores and the loads (one workgroup, one CU: its L1 serves both).
__global__ __launch_bounds__(DT_THREADS) void pursuit_kernel(float *R, float *tmax, int *tidx, DetectGeom g, int K, float *positions,
                                                              float *amplitudes, int *count) {
    __shared__ float s_tap[DT_R_MAX + 1];
    __shared__ float s_c2[DT_R_MAX + 1];
    __shared__ float s_e[3][2 * DT_R_MAX + 1];    // g1(x - p^) over the footprint's voxels, 0 outside the volume
    __shared__ float s_h[3][2 * DT_WR_MAX + 1];   // the filter's response to it, per axis
    __shared__ float s_wv[DT_WAVES];
    __shared__ int s_wi[DT_WAVES];
    __shared__ float s_f[12];                     // 0..2 delta, 4..6 the terms of ln S^, 8..10 sum e^2
    __shared__ int s_close;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S[3] = {g.X, g.Y, g.Z};
    const int r = g.r, wr = g.wr;
    const float ninf = -__builtin_inff();
    fill_taps(s_tap, s_c2, r, g.inv_s2, tid, DT_THREADS);
    __syncthreads();
    int found = 0;
    for (int k = 0; k < K; ++k) {
        // pick
        float bv = ninf;
        int bi = 0x7fffffff;
        for (int t = tid; t < g.ntiles; t += DT_THREADS) {
            const float v = tmax[t];
            const int i = tidx[t];
            if (better(v, i, bv, bi)) bv = v, bi = i;
        }
        wave_argmax_last(bv, bi);
        if (lane == 63) s_wv[wave] = bv, s_wi[wave] = bi;
        __syncthreads();
        bv = s_wv[0], bi = s_wi[0];
#pragma unroll
        for (int w = 1; w < DT_WAVES; ++w) {
            const float v = s_wv[w];
            const int i = s_wi[w];
            if (better(v, i, bv, bi)) bv = v, bi = i;
        }
        // the same in every thread: the loop ends for the whole workgroup
        if (!(bv > g.threshold) || !(bv < __builtin_inff()) || bi == 0x7fffffff) break;
        const int p[3] = {bi / (g.Y * g.Z), (bi / g.Z) % g.Y, bi % g.Z};
        // refine: one thread per axis
        if (tid < 3) {
            const int d = tid;
            const int stride = d == 0 ? g.Y * g.Z : (d == 1 ? g.Z : 1);
            float dl = 0.0f, adj = 0.0f;
            // the parabola through ln S at p* and its two neighbours; at the first or last voxel of an axis of three or more
            // the one through p* and the two voxels inward (t counts inward there)
            const bool two = p[d] > 0 && p[d] < S[d] - 1;
            const bool one = !two && S[d] >= 3;
            if (bv > 0.0f && (two || one)) {
                const int in = p[d] == 0 ? stride : -stride;
                const float m = R[two ? bi - stride : bi + in], q = R[two ? bi + stride : bi + 2 * in];
                refine_axis(bv, m, q, two, p[d] == 0, dl, adj);
            }
            s_f[d] = dl, s_f[4 + d] = adj;
        }
        if (tid == 0) s_close = 0;
        __syncthreads();
        // a refined centre within min_distance of an earlier one is dropped (p* itself cannot be: it would be excluded)
        float ph[3] = {(float)p[0] + s_f[0], (float)p[1] + s_f[1], (float)p[2] + s_f[2]};
        for (int j = tid; j < k; j += DT_THREADS) {
            const float dx = positions[3 * j] - ph[0], dy = positions[3 * j + 1] - ph[1], dz = positions[3 * j + 2] - ph[2];
            if (dx * dx + dy * dy + dz * dz <= g.md2) s_close = 1;
        }
        __syncthreads();
        const bool keep = s_close == 0;
        float dl[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            dl[d] = keep ? s_f[d] : 0.0f;
            ph[d] = (float)p[d] + dl[d];
        }
        const float rhat = keep ? refined_score(bv, s_f[4], s_f[5], s_f[6]) : bv;
        // the footprint along each axis: x = p* + o, o in [-r, r]
        for (int i = tid; i < 3 * (2 * r + 1); i += DT_THREADS) {
            const int d = i / (2 * r + 1), o = i - d * (2 * r + 1) - r;
            s_e[d][o + r] = footprint_tap(p[d], o, dl[d], S[d], g.inv_s2);
        }
        __syncthreads();
        // h(q) = sum_x g1(x - q) e(x) over |x - q| <= r, q = p* + j, j in [-wr, wr]; and the norms sum e^2
        for (int i = tid; i < 3 * (2 * wr + 1); i += DT_THREADS) {
            const int d = i / (2 * wr + 1), j = i - d * (2 * wr + 1) - wr;
            float acc = 0.0f;
            const int ohi = min(r, j + r);
            for (int o = max(-r, j - r); o <= ohi; ++o) acc += s_tap[abs(o - j)] * s_e[d][o + r];
            s_h[d][j + wr] = in_range(p[d] + j, S[d]) ? acc * axis_weight(s_c2, r, p[d] + j, S[d]) : 0.0f;
        }
        if (tid >= DT_THREADS - 64 && tid < DT_THREADS - 61) {
            const int d = tid - (DT_THREADS - 64);
            float acc = 0.0f;
            for (int o = 0; o <= 2 * r; ++o) acc += s_e[d][o] * s_e[d][o];
            s_f[8 + d] = acc;
        }
        __syncthreads();
        // S^ = a sqrt(prod nmax) sqrt(prod sum e^2) for the footprint a e_x e_y e_z
        const float amp = footprint_amplitude(rhat, s_c2, r, S, s_f[8], s_f[9], s_f[10]);
        // subtract and exclude over the window
        int lo[3], ext[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = max(0, p[d] - wr);
            ext[d] = min(S[d] - 1, p[d] + wr) - lo[d] + 1;
        }
        const int n = ext[0] * ext[1] * ext[2];
        for (int i = tid; i < n; i += DT_THREADS) {
            const int qz = lo[2] + i % ext[2], qy = lo[1] + (i / ext[2]) % ext[1], qx = lo[0] + i / (ext[2] * ext[1]);
            const int idx = (qx * g.Y + qy) * g.Z + qz;
            const float h = (s_h[0][qx - p[0] + wr] * s_h[1][qy - p[1] + wr]) * s_h[2][qz - p[2] + wr];
            const float dx = (float)qx - ph[0], dy = (float)qy - ph[1], dz = (float)qz - ph[2];
            float v = R[idx] - amp * h;
            if (dx * dx + dy * dy + dz * dz <= g.md2) v = ninf;
            R[idx] = v;
        }
        if (tid < 3) positions[3 * k + tid] = ph[tid];
        if (tid == 3) amplitudes[k] = amp;
        __syncthreads();
        // the tiles the window touched, one wave each
        const int t0[3] = {lo[0] / DT_TX, lo[1] / DT_TY, lo[2] / DT_TZ};
        const int tn[3] = {(lo[0] + ext[0] - 1) / DT_TX - t0[0] + 1, (lo[1] + ext[1] - 1) / DT_TY - t0[1] + 1,
                           (lo[2] + ext[2] - 1) / DT_TZ - t0[2] + 1};
        const int nt = tn[0] * tn[1] * tn[2];
        for (int i = wave; i < nt; i += DT_WAVES) {
            const int t = ((t0[0] + i / (tn[2] * tn[1])) * g.nty + (t0[1] + (i / tn[2]) % tn[1])) * g.ntz + (t0[2] + i % tn[2]);
            float v;
            int ix;
            tile_argmax(R, g, t, lane, v, ix);
            if (lane == 63) tmax[t] = v, tidx[t] = ix;
        }
        __syncthreads();
        found = k + 1;
    }
    const float nan = __builtin_nanf("");
    for (int i = 3 * found + tid; i < 3 * K; i += DT_THREADS) positions[i] = nan;
    for (int i = found + tid; i < K; i += DT_THREADS) amplitudes[i] = nan;
    if (tid == 0) *count = found;
}

// 0 ok, else the error already recorded
int detect_geometry(const char *fn, const int *sz, int K, double sigma, double min_distance, DetectGeom &g) {
    DNMF_REQUIRE(sz, DNMF_E_NULL, "%s: NULL sz", fn);
    DNMF_REQUIRE(sz[0] > 0 && sz[1] > 0 && sz[2] > 0, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE((long)sz[0] * sz[1] * sz[2] < (1L << 31), DNMF_E_UNSUPPORTED, "%s: volume %dx%dx%d has 2^31 voxels or more", fn, sz[0],
                 sz[1], sz[2]);
    DNMF_REQUIRE(K >= 1, DNMF_E_SHAPE, "%s: K=%d must be at least 1", fn, K);
    DNMF_REQUIRE(sigma > 0.0 && sigma < __builtin_inf(), DNMF_E_SHAPE, "%s: sigma=%g must be positive and finite", fn, sigma);
    DNMF_REQUIRE(sigma <= DT_R_MAX / 3.0, DNMF_E_UNSUPPORTED, "%s: sigma=%g: the filter holds at most %d taps per side (sigma <= %d)", fn,
                 sigma, DT_R_MAX, DT_R_MAX / 3);
    DNMF_REQUIRE(min_distance >= 0.0 && min_distance < __builtin_inf(), DNMF_E_SHAPE, "%s: min_distance=%g must be >= 0 and finite", fn,
                 min_distance);
    g.X = sz[0], g.Y = sz[1], g.Z = sz[2];
    g.r = (int)__builtin_ceil(3.0 * sigma);
    DNMF_REQUIRE(min_distance <= DT_WR_MAX - 2, DNMF_E_UNSUPPORTED, "%s: min_distance=%g: at most %d voxels", fn, min_distance,
                 DT_WR_MAX - 2);
    // |q - p*| <= min_distance + 1/2 per axis for every excluded voxel q
    const int we = (int)__builtin_ceil(min_distance) + 1;
    g.wr = 2 * g.r > we ? 2 * g.r : we;
    g.ntx = (g.X + DT_TX - 1) / DT_TX, g.nty = (g.Y + DT_TY - 1) / DT_TY, g.ntz = (g.Z + DT_TZ - 1) / DT_TZ;
    g.ntiles = g.ntx * g.nty * g.ntz;
    g.inv_s2 = (float)(1.0 / (sigma * sigma));
    g.md2 = (float)(min_distance * min_distance);
    g.threshold = 0.0f;
    return DNMF_OK;
}

size_t detect_workspace(const DetectGeom &g) {
    const size_t P = (size_t)g.X * g.Y * g.Z;
    return 2 * align256(P * sizeof(float)) + 2 * align256((size_t)g.ntiles * sizeof(float));
}

template <bool LOADZ>
void launch_filter(const float *in, float *out, int A, int S, int B, const DetectGeom &g, float background, hipStream_t st) {
    const int tbw = B < 64 ? B : 64;
    const int ts = S < DT_TILE_OUT / tbw ? S : DT_TILE_OUT / tbw;
    const int nsb = (S + ts - 1) / ts, nbb = (B + tbw - 1) / tbw;
    const size_t lds = (2 * (size_t)((g.r + 4) & ~3) + (size_t)(ts + 2 * g.r) * tbw) * sizeof(float);
    hipLaunchKernelGGL(filter_axis_kernel<LOADZ>, dim3((unsigned)((long)A * nsb * nbb)), dim3(256), lds, st, in, out, S, B, ts, tbw, nsb,
                       nbb, g.r, g.inv_s2, background);
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_detect_neurons_workspace(const int *sz, int K, double sigma) {
    dnmf::DetectGeom g;
    if (dnmf::detect_geometry("dnmf_detect_neurons_workspace", sz, K, sigma, 0.0, g) != DNMF_OK) return 0;
    return dnmf::detect_workspace(g);
}

int dnmf_detect_neurons(const float *img, const int *sz, int K, double sigma, double min_distance, double threshold, double background,
                        float *positions, float *amplitudes, int *count, void *workspace, size_t workspace_bytes,
                        dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(img && positions && amplitudes && count && workspace, DNMF_E_NULL, "dnmf_detect_neurons: NULL argument");
    DetectGeom g;
    const int rc = detect_geometry("dnmf_detect_neurons", sz, K, sigma, min_distance, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(background > -__builtin_inf() && background < __builtin_inf(), DNMF_E_SHAPE,
                 "dnmf_detect_neurons: background=%g must be finite", background);
    DNMF_REQUIRE(threshold == threshold && threshold < __builtin_inf(), DNMF_E_SHAPE, "dnmf_detect_neurons: threshold=%g must be below +inf",
                 threshold);
    DNMF_REQUIRE(workspace_bytes >= detect_workspace(g), DNMF_E_WORKSPACE, "dnmf_detect_neurons: workspace of %zu bytes, need %zu",
                 workspace_bytes, detect_workspace(g));
    DNMF_REQUIRE(((size_t)workspace & 3) == 0, DNMF_E_WORKSPACE, "dnmf_detect_neurons: workspace must be 4-byte aligned");
    // a threshold below the fp32 range rounds to -inf, which every finite score passes
    g.threshold = (float)threshold;
    const size_t P = (size_t)g.X * g.Y * g.Z;
    char *w = static_cast<char *>(workspace);
    float *tmp = reinterpret_cast<float *>(w);
    float *R = reinterpret_cast<float *>(w + align256(P * sizeof(float)));
    float *tmax = reinterpret_cast<float *>(w + 2 * align256(P * sizeof(float)));
    int *tidx = reinterpret_cast<int *>(w + 2 * align256(P * sizeof(float)) + align256((size_t)g.ntiles * sizeof(float)));
    const hipStream_t st = (hipStream_t)stream;
    launch_filter<true>(img, tmp, g.X, g.Y, g.Z, g, (float)background, st);      // z (on load) and y
    launch_filter<false>(tmp, R, 1, g.X, g.Y * g.Z, g, 0.0f, st);                // x
    hipLaunchKernelGGL(tile_table_kernel, dim3((unsigned)((g.ntiles + 3) / 4)), dim3(256), 0, st, R, g, tmax, tidx);
    hipLaunchKernelGGL(pursuit_kernel, dim3(1), dim3(DT_THREADS), 0, st, R, tmax, tidx, g, K, positions, amplitudes, count);
    return check_launch("dnmf_detect_neurons");
}

}  // extern "C"
