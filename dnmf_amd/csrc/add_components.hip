// K28: new components from the residual -- the two kernels that turn candidate boxes into footprints and traces learned from
// the residual movie.  include/dnmf_hip.h has the contract, tests/add_restatement.py the definition in float64.
//
// K28a (dnmf_residual_boxes) gathers e[m, t, j] = frames_t(v_j) - sub_t(v_j) for the voxels v_j of candidate box m (x slowest, z
// fastest, as K24 numbers them) into a compact fp32 buffer E (M, n, vmax).  A workgroup owns one box and a run of RB_FRAMES frames;
// a lane works out its voxels' offsets once and walks the run, so the lanes of a wave read the z-rows of the box and write
// consecutive j.
//
// K28b (dnmf_rank1_nmf) fits the non-negative rank-1 factor a c^T of E[m] over the frames whose samples are all finite, by
// alternating half-steps, all iterations in one launch, one workgroup per candidate.  a lives in LDS and c in the caller's
// workspace, both in float64; the fp32 results are rounded once at the end.
//   c-step  a wave takes a frame: its lanes take the voxels lane, lane + 64, .. in that order, the wave tree (block_ops.hpp) adds
//           the lanes, lane 0 forms c_t.  Wave w takes the frames w, w + NM_WAVES, ..; lane 0 adds c_t^2 (and what else is summed
//           over frames) in that order, and block_reduce adds the waves.
//   a-step  a lane owns a voxel of a tile of 64 and walks the frames of its wave's segment (wave w: frames [w L, (w + 1) L), L =
//           ceil(n / NM_WAVES)) in their order; the NM_WAVES partial sums of a voxel meet in LDS and are added in wave order.
// Both read E[m] along j: coalesced.  Every sum has a fixed order and there are no atomics: the same input gives the same bits.
#include "block_ops.hpp"
#include "boxes.hpp"

namespace dnmf {
namespace {

constexpr int AC_MAX_BOXES = 4096;
constexpr int AC_MAX_FRAMES = 18432;

constexpr int RB_THREADS = 256;
constexpr int RB_FRAMES = 8;            // frames a workgroup gathers: the offsets of a lane's voxels are worked out once per run

struct GatherArgs {
    const float *frames, *sub;
    long ldf, lds;
    const int *frame_ids, *boxes;
    int Y, Z, B, n, vmax, t0;
    float *E;
};

__global__ __launch_bounds__(RB_THREADS) void residual_boxes_kernel(GatherArgs g) {
    const int m = blockIdx.x, f0 = blockIdx.y * RB_FRAMES, f1 = min(g.B, f0 + RB_FRAMES);
    const Box q = load_box(g.boxes + 6 * (long)m);
    float *Em = g.E + ((size_t)m * g.n + g.t0) * g.vmax;
    for (int j = threadIdx.x; j < g.vmax; j += RB_THREADS) {
        const int off = j < q.n ? box_offset(q, j, g.Y, g.Z) : -1;
        for (int f = f0; f < f1; ++f) {
            float e = 0.0f;
            if (off >= 0) {
                e = g.frames[(long)(g.frame_ids ? g.frame_ids[f] : f) * g.ldf + off];
                if (g.sub) e = e - g.sub[(long)f * g.lds + off];
            }
            Em[(size_t)f * g.vmax + j] = e;
        }
    }
}

constexpr int NM_THREADS = 512, NM_WAVES = NM_THREADS / 64;

struct NmfArgs {
    const float *E, *a0;
    const int *nvox;
    int n, vmax, iters;
    float *a, *c;
    double *stats, *cws;      // (M, 4); the workspace: (M, n) float64 traces between the steps
    int *n_valid, *ok;
};

__device__ __forceinline__ bool positive(double v) { return v > 0.0 && __builtin_isfinite(v); }

// sum of a_j^2 over the box, in every lane: a lane adds its voxels tid, tid + NM_THREADS, .. in that order, then block_reduce
__device__ __forceinline__ double norm2(const double *a, int nm, double *red) {
    double s = 0.0;
    for (int j = threadIdx.x; j < nm; j += NM_THREADS) s = fma(a[j], a[j], s);
    return block_reduce<NM_THREADS>(s, OpSum(), red);
}

// One c-step: c_t = max(<a, e_t>, 0) / saa on the valid frames, NaN on the others, to cw.  first: the frames are classified here
// (valid <=> sum_j e^2 is finite: squares of finite fp32 samples cannot overflow a float64 sum), energy = sum over the valid
// frames of sum_j e^2, nvalid their number.  Returns sum c_t^2 in every lane; cross = sum c_t <a, e_t>.
__device__ __forceinline__ double c_step(const float *Em, const double *a, double *cw, int nm, int n, int vmax, double saa, bool first,
                                         double &energy, int &nvalid, double &cross, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double scc = 0.0, sx = 0.0, sen = 0.0;
    int nv = 0;
    for (int t = wave; t < n; t += NM_WAVES) {
        const float *e = Em + (size_t)t * vmax;
        double dot = 0.0, ee = 0.0;
        for (int j = lane; j < nm; j += 64) {
            const double v = (double)e[j];
            dot = fma(a[j], v, dot);
            if (first) ee = fma(v, v, ee);
        }
        dot = wave_sum(dot);
        if (first) ee = wave_sum(ee);
        if (lane == 0) {
            const bool valid = first ? __builtin_isfinite(ee) : cw[t] == cw[t];
            double ct = quiet_nan();
            if (valid) {
                ct = fmax(dot, 0.0) / saa;
                scc = fma(ct, ct, scc);
                sx = fma(ct, dot, sx);
                if (first) sen += ee, ++nv;
            }
            cw[t] = ct;
        }
    }
    scc = block_reduce<NM_THREADS>(scc, OpSum(), red);
    cross = block_reduce<NM_THREADS>(sx, OpSum(), red);
    if (first) {
        energy = block_reduce<NM_THREADS>(sen, OpSum(), red);
        nvalid = block_reduce<NM_THREADS>(nv, OpSum(), red);
    }
    return scc;   // the reductions end with a barrier: cw is visible to the workgroup
}

// One a-step: a_j = max(sum_{t valid} c_t e_tj, 0) / scc.  part: NM_WAVES x 64 doubles of LDS.
__device__ __forceinline__ void a_step(const float *Em, double *a, const double *cw, int nm, int n, int vmax, double scc, double *part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = (n + NM_WAVES - 1) / NM_WAVES, ta = min(n, wave * L), tb = min(n, ta + L);
    for (int j0 = 0; j0 < nm; j0 += 64) {
        const int j = j0 + lane;
        double acc = 0.0;
        if (j < nm) {
#pragma unroll 4
            for (int t = ta; t < tb; ++t) {
                const double ct = cw[t], v = (double)Em[(size_t)t * vmax + j];   // both loads unconditional: they pipeline
                acc = ct == ct ? fma(ct, v, acc) : acc;
            }
        }
        part[wave * 64 + lane] = acc;
        __syncthreads();
        if (wave == 0 && j < nm) {
            double s = part[lane];
#pragma unroll
            for (int w = 1; w < NM_WAVES; ++w) s += part[w * 64 + lane];
            a[j] = fmax(s, 0.0) / scc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NM_THREADS) void rank1_nmf_kernel(NmfArgs g) {
    __shared__ double a[BOX_MAX_VOXELS];
    __shared__ double part[NM_WAVES * 64];
    __shared__ double red[NM_WAVES];
    const int tid = threadIdx.x, m = blockIdx.x;
    const int n = g.n, vmax = g.vmax;
    const int nraw = g.nvox[m];
    const int nm = min(max(nraw, 0), vmax);
    const float *Em = g.E + (size_t)m * n * vmax;
    double *cw = g.cws + (size_t)m * n;

    for (int j = tid; j < nm; j += NM_THREADS) a[j] = (double)g.a0[(size_t)m * vmax + j];
    __syncthreads();
    const double norm0 = norm2(a, nm, red);
    double saa = norm0, scc = 0.0, energy = 0.0, cross = 0.0;
    int nvalid = 0;
    bool ok = nraw >= 1 && nraw <= vmax && positive(saa);
    // every branch below is taken by the whole workgroup: ok depends on block-wide values only
    for (int it = 0; ok && it <= g.iters; ++it) {
        if (it == g.iters) {
            // the finish: a scaled to the norm of the start, then one more c-step
            const double s = sqrt(norm0 / saa);
            for (int j = tid; j < nm; j += NM_THREADS) a[j] *= s;
            __syncthreads();
            saa = norm2(a, nm, red);
            ok = positive(saa);
            if (!ok) break;
        }
        scc = c_step(Em, a, cw, nm, n, vmax, saa, it == 0, energy, nvalid, cross, red);
        ok = nvalid >= 1 && positive(scc);
        if (!ok || it == g.iters) break;
        a_step(Em, a, cw, nm, n, vmax, scc, part);
        saa = norm2(a, nm, red);
        ok = positive(saa);
    }
    if (!ok && nraw >= 1 && nraw <= vmax && nvalid == 0 && !positive(norm0)) {
        // the start itself was refused before any frame was read: the energy and the valid frames are still reported
        double unused = 0.0;
        c_step(Em, a, cw, nm, n, vmax, 1.0, true, energy, nvalid, unused, red);
    }

    const float nanf = __int_as_float(0x7fc00000);
    for (int j = tid; j < vmax; j += NM_THREADS) g.a[(size_t)m * vmax + j] = j < nm ? (ok ? (float)a[j] : nanf) : 0.0f;
    for (int t = tid; t < n; t += NM_THREADS) g.c[(size_t)m * n + t] = ok ? (float)cw[t] : nanf;
    if (tid == 0) {
        double *st = g.stats + 4 * (size_t)m;
        st[0] = energy;
        st[1] = ok ? 2.0 * cross - saa * scc : quiet_nan();
        st[2] = ok ? saa : quiet_nan();
        st[3] = ok ? scc : quiet_nan();
        g.n_valid[m] = nvalid;
        g.ok[m] = ok ? 1 : 0;
    }
}

int nmf_limits(const char *fn, int M, int n, int vmax) {
    DNMF_REQUIRE(M >= 1 && n >= 1 && vmax >= 1, DNMF_E_SHAPE, "%s: M=%d candidates, n=%d frames, vmax=%d voxels", fn, M, n, vmax);
    DNMF_REQUIRE(vmax <= BOX_MAX_VOXELS, DNMF_E_UNSUPPORTED, "%s: vmax=%d voxels a box, at most %d", fn, vmax, BOX_MAX_VOXELS);
    DNMF_REQUIRE(M <= AC_MAX_BOXES, DNMF_E_UNSUPPORTED, "%s: M=%d candidates, at most %d", fn, M, AC_MAX_BOXES);
    DNMF_REQUIRE(n <= AC_MAX_FRAMES, DNMF_E_UNSUPPORTED, "%s: n=%d frames, at most %d", fn, n, AC_MAX_FRAMES);
    return DNMF_OK;
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_residual_boxes(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const int *sz, int B,
                        const int *boxes, const int *boxes_dev, int M, float *E, int n, int vmax, int t0, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_residual_boxes";
    DNMF_REQUIRE(frames && sz && boxes && boxes_dev && E, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    const long P = (long)sz[0] * sz[1] * sz[2];
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    const int rc = nmf_limits(fn, M, n, vmax);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(B >= 1 && t0 >= 0 && (long)t0 + B <= n, DNMF_E_SHAPE, "%s: B=%d frames at t0=%d of n=%d", fn, B, t0, n);
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P), DNMF_E_SHAPE, "%s: ldf=%ld lds=%ld below a row of P=%ld", fn, ldf, lds, P);
    const int rb = check_boxes(fn, sz, boxes, M, vmax, DNMF_E_SHAPE, "vmax=");
    if (rb != DNMF_OK) return rb;
    GatherArgs a;
    a.frames = frames, a.sub = sub, a.ldf = ldf, a.lds = lds, a.frame_ids = frame_ids, a.boxes = boxes_dev;
    a.Y = sz[1], a.Z = sz[2], a.B = B, a.n = n, a.vmax = vmax, a.t0 = t0, a.E = E;
    const unsigned runs = (unsigned)((B + RB_FRAMES - 1) / RB_FRAMES);
    hipLaunchKernelGGL(residual_boxes_kernel, dim3((unsigned)M, runs), dim3(RB_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}

size_t dnmf_rank1_nmf_workspace(int M, int n) {
    using namespace dnmf;
    if (nmf_limits("dnmf_rank1_nmf_workspace", M, n, 1) != DNMF_OK) return 0;
    return align256((size_t)M * n * sizeof(double));
}

int dnmf_rank1_nmf(const float *E, int M, int n, int vmax, const int *nvox, const float *a0, int iters, float *a, float *c,
                   double *stats, int *n_valid, int *ok, void *workspace, size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_rank1_nmf";
    DNMF_REQUIRE(E && nvox && a0 && a && c && stats && n_valid && ok && workspace, DNMF_E_NULL, "%s: NULL argument", fn);
    const int rc = nmf_limits(fn, M, n, vmax);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(iters >= 1, DNMF_E_SHAPE, "%s: iters=%d", fn, iters);
    const size_t need = align256((size_t)M * n * sizeof(double));
    DNMF_REQUIRE(workspace_bytes >= need, DNMF_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu", fn, workspace_bytes, need);
    DNMF_REQUIRE(((size_t)workspace & 7) == 0, DNMF_E_WORKSPACE, "%s: workspace must be 8-byte aligned", fn);
    NmfArgs g;
    g.E = E, g.a0 = a0, g.nvox = nvox, g.n = n, g.vmax = vmax, g.iters = iters;
    g.a = a, g.c = c, g.stats = stats, g.cws = static_cast<double *>(workspace), g.n_valid = n_valid, g.ok = ok;
    hipLaunchKernelGGL(rank1_nmf_kernel, dim3((unsigned)M), dim3(NM_THREADS), 0, (hipStream_t)stream, g);
    return check_launch(fn);
}

}  // extern "C"
