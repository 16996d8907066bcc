// K31: the running-percentile baseline of a movie and what is read against it (dF/F).  include/dnmf_hip.h has the contract,
// tests/dff_restatement.py the definition.
//
// K31a (dnmf_running_quantile): per voxel and window of W frames, every S frames, the kept samples of ranks lo and hi and their
// count.  A workgroup of 256 threads owns V = 64, 32 or 16 contiguous voxels (by W: the window must fit LDS) and a run of
// consecutive windows.  The window's samples live in LDS as K30's 32-bit keys (key32.hpp), a sample that is not finite as the
// key RQ_NONE above every other; the rows form a ring, frame t in slot t mod W, so the step to the next window loads its S new
// rows over the S that left and a sample comes from HBM once per run.  L = 256 / V lanes share a voxel: lane l holds the slots
// with (slot mod 2L) / 2 = l, two adjacent slots as one 8-byte word, and the word of slot pair k of thread tid is word
// k 256 + tid of the ring -- a wave reads 64 consecutive 8-byte words per instruction (ds_read_b64: 64 banks of 4 bytes per
// half-wave, none twice).  The selection is a bisection on the key from bit 31 down, count(key < candidate) over the window summed
// over the L lanes by a butterfly inside the wave (adjacent lanes: no LDS, no barrier), then one pass for count(key <= a_lo) and
// the least key above it, which settles a_hi as in K30.  Integer counts only: the same bits for every run length, every cut of
// the movie and every launch.  The rows are written to the ring with a stride of 2L words between voxels (8-way on the 32 banks
// of a store for V = 64): a sample is stored once and read 32 W / S times, so the store is left as it is.
//
// K31b (dnmf_baseline_apply): one streaming launch; a thread owns a voxel and a chunk of consecutive frames, keeps the two knot
// values of the current interval in registers and fetches one when the interval moves on.
#include "block_ops.hpp"
#include "key32.hpp"

namespace dnmf {
namespace {

constexpr int RQ_THREADS = 256;
constexpr int RQ_MAX_WINDOW = 2048;
constexpr int RQ_UNROLL = 4;               // rows whose loads are in flight together, per thread
constexpr int RQ_TARGET_BLOCKS = 1024;     // run = 0: about this many workgroups
constexpr uint32_t RQ_NONE = 0xffffffffu;  // the key of a sample left out: no finite float has it (+max is 0xff7fffff)
constexpr int BA_CHUNK = 32;               // frames of a thread of K31b
constexpr int BA_UNROLL = 4;

// voxels of a workgroup by the rows of a window: 64 x 512 x 4 B = 128 KiB of the 160 a CU has
inline int tile_voxels(int rows) { return rows <= 512 ? 64 : rows <= 1024 ? 32 : 16; }

struct WindowPlan {
    int T, W, S, Wn;   // Wn = min(W, T): the rows of every window
    long J;
    __host__ __device__ int start(long j) const {
        const long s = j * S, last = T > W ? T - W : 0;
        return (int)(s < last ? s : last);
    }
};

int window_plan(const char *fn, long T, int W, int S, WindowPlan &p) {
    DNMF_REQUIRE(T >= 1 && T <= 2147483647L - RQ_MAX_WINDOW, DNMF_E_SHAPE, "%s: T=%ld frames", fn, T);
    DNMF_REQUIRE(W >= 1, DNMF_E_SHAPE, "%s: window=%d frames", fn, W);
    DNMF_REQUIRE(S >= 1 && S <= W, DNMF_E_SHAPE, "%s: stride=%d outside [1, window=%d]", fn, S, W);
    DNMF_REQUIRE(W <= RQ_MAX_WINDOW, DNMF_E_UNSUPPORTED, "%s: window=%d frames, at most %d (a window lives in LDS)", fn, W, RQ_MAX_WINDOW);
    p.T = (int)T, p.W = W, p.S = S, p.Wn = T < W ? (int)T : W;
    p.J = T <= W ? 1 : (T - W + S - 1) / S + 1;
    return DNMF_OK;
}

struct RQArgs {
    const float *frames;
    long ldf, P, ldk;
    const int *frame_ids;
    WindowPlan w;
    int row0;          // the frame of row 0 of the call
    long j0, j1;       // the windows of the call
    int run, nk;       // windows a workgroup; slot pairs a thread
    double q;
    float *lo, *hi;
    int *n;
};

template <int V>
__global__ __launch_bounds__(RQ_THREADS) void running_quantile_kernel(RQArgs a) {
    extern __shared__ uint32_t ring[];   // nk x 256 pairs of keys
    constexpr int L = RQ_THREADS / V;
    const int tid = threadIdx.x;
    uint2 *ring2 = reinterpret_cast<uint2 *>(ring);
    for (int k = 0; k < a.nk; ++k) ring2[k * RQ_THREADS + tid] = make_uint2(RQ_NONE, RQ_NONE);
    __syncthreads();
    // loading: thread (lr, lv) takes voxel lv of the rows lr, lr + L, ..
    const int lv = tid % V, lr = tid / V;
    const long gl = (long)blockIdx.x * V + lv;
    const bool live = gl < a.P;
    const long rl = live ? gl : a.P - 1;   // a lane past the volume reads the last voxel and keeps nothing
    // selecting: thread (sv, sl) is lane sl of voxel sv
    const int sv = tid / L, sl = tid % L;
    const long gs = (long)blockIdx.x * V + sv;
    const int Wn = a.w.Wn, nk = a.nk;
    auto word = [&](int slot) {
        const int m = slot % (2 * L);
        return (slot / (2 * L)) * (2 * RQ_THREADS) + (lv * L + (m >> 1)) * 2 + (m & 1);
    };
    auto row = [&](int t) { return a.frames + (long)(a.frame_ids ? a.frame_ids[t - a.row0] : t - a.row0) * a.ldf; };
    // count(key < cand) and count(key <= cand) of the voxel's window, in every one of its L lanes
    auto lanes_sum = [&](int c) {
#pragma unroll
        for (int o = 1; o < L; o <<= 1) c += __shfl_xor(c, o, 64);
        return c;
    };
    auto count_below = [&](uint32_t cand) {
        int c = 0;
#pragma unroll 4
        for (int k = 0; k < nk; ++k) {
            const uint2 kk = ring2[k * RQ_THREADS + tid];
            c += (kk.x < cand) + (kk.y < cand);
        }
        return lanes_sum(c);
    };
    const long ja = a.j0 + (long)blockIdx.y * a.run, jb = ja + a.run < a.j1 ? ja + a.run : a.j1;
    int loaded = a.w.start(ja);   // the frames [start(j), loaded) of window j are in the ring
    for (long j = ja; j < jb; ++j) {
        const int e = a.w.start(j) + Wn;
        for (int t0 = loaded + lr; t0 < e; t0 += L * RQ_UNROLL) {
            float y[RQ_UNROLL];
#pragma unroll
            for (int u = 0; u < RQ_UNROLL; ++u) y[u] = t0 + u * L < e ? row(t0 + u * L)[rl] : 0.0f;
#pragma unroll
            for (int u = 0; u < RQ_UNROLL; ++u)
                if (t0 + u * L < e) ring[word((t0 + u * L) % Wn)] = live && __builtin_isfinite(y[u]) ? to_key32(y[u]) : RQ_NONE;
        }
        loaded = e;
        __syncthreads();
        const int nn = count_below(RQ_NONE);
        const uint32_t rlo = nn ? (uint32_t)floor(a.q * (double)(nn - 1)) : 0u;
        uint32_t pre = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = pre | (1u << bit);
            if ((uint32_t)count_below(cand) <= rlo) pre = cand;
        }
        int cle = 0;
        uint32_t nxt = RQ_NONE;
#pragma unroll 4
        for (int k = 0; k < nk; ++k) {
            const uint2 kk = ring2[k * RQ_THREADS + tid];
            cle += (kk.x <= pre) + (kk.y <= pre);
            if (kk.x > pre && kk.x < nxt) nxt = kk.x;
            if (kk.y > pre && kk.y < nxt) nxt = kk.y;
        }
        cle = lanes_sum(cle);
#pragma unroll
        for (int o = 1; o < L; o <<= 1) nxt = min(nxt, (uint32_t)__shfl_xor((int)nxt, o, 64));
        if (sl == 0 && gs < a.P) {
            float x0 = __uint_as_float(0x7fc00000u), x1 = x0;
            if (nn) {
                const uint32_t rhi = min(rlo + 1u, (uint32_t)nn - 1u);
                x0 = from_key32(pre);
                x1 = (rhi == rlo || (uint32_t)cle >= rlo + 2u) ? x0 : from_key32(nxt);
            }
            const size_t at = (size_t)j * a.ldk + gs;
            a.lo[at] = x0, a.hi[at] = x1, a.n[at] = nn;
        }
        __syncthreads();   // the next window's rows go over slots this one read
    }
}

template <int V>
int launch_running_quantile(const char *fn, const RQArgs &a, unsigned ntiles, unsigned nruns, size_t lds, hipStream_t st) {
    if (lds > 48u * 1024u) {   // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void *)running_quantile_kernel<V>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail((int)e, "%s: %zu bytes of LDS: %s", fn, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(running_quantile_kernel<V>, dim3(ntiles, nruns), dim3(RQ_THREADS), lds, st, a);
    return check_launch(fn);
}

struct BAArgs {
    const float *frames;
    long ldf, P, ldv, ldo, row0;
    const int *frame_ids;
    const double *value, *centres;
    int B, J, mode, chunk;
    double offset;
    float *out;
};

__global__ __launch_bounds__(256) void baseline_apply_kernel(BAArgs a) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.P) return;
    const int i0 = (int)blockIdx.y * a.chunk, i1 = min(a.B, i0 + a.chunk);
    // the last knot at or before the chunk's first frame (-1: none), by bisection; it only moves forward from there
    int jj = -1;
    {
        const double t = (double)(a.row0 + i0);
        int lo = 0, hi = a.J;   // centres[< lo] <= t < centres[>= hi]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.centres[mid] <= t) lo = mid + 1;
            else hi = mid;
        }
        jj = lo - 1;
    }
    int ca = -1, cb = -1;   // the knots held in ba, bb
    double ba = 0.0, bb = 0.0;
    const float nanf32 = __uint_as_float(0x7fc00000u);
    for (int i = i0; i < i1; i += BA_UNROLL) {
        float y[BA_UNROLL];
#pragma unroll
        for (int u = 0; u < BA_UNROLL; ++u)
            y[u] = i + u < i1 ? a.frames[(long)(a.frame_ids ? a.frame_ids[i + u] : i + u) * a.ldf + v] : 0.0f;
#pragma unroll
        for (int u = 0; u < BA_UNROLL; ++u) {
            if (i + u >= i1) break;
            const double t = (double)(a.row0 + i + u);
            while (jj + 1 < a.J && a.centres[jj + 1] <= t) ++jj;
            const int ja = jj < 0 ? 0 : jj, jb = ja + 1 < a.J ? ja + 1 : a.J - 1;
            if (ja != ca) ba = ja == cb ? bb : a.value[(size_t)ja * a.ldv + v], ca = ja;
            if (jb != cb) bb = a.value[(size_t)jb * a.ldv + v], cb = jb;
            double f0 = ba;
            if (jj >= 0 && jj + 1 < a.J) {
                const double cj = a.centres[jj], w = (t - cj) / (a.centres[jj + 1] - cj);
                if (w != 0.0) {
                    const double d = bb - ba, wd = w * d;   // two roundings, as the definition writes them
                    f0 = ba + wd;
                }
            }
            const double yd = (double)y[u];
            bool ok = __builtin_isfinite(y[u]) && __builtin_isfinite(f0);
            double r = f0;
            if (a.mode != DNMF_BASELINE_F0) {
                r = yd - f0;
                if (a.mode != DNMF_BASELINE_DF) {
                    const double den = f0 + a.offset;
                    ok = ok && den > 0.0;
                    r = r / (a.mode == DNMF_BASELINE_DFF ? den : sqrt(den));
                }
            }
            a.out[(long)(i + u) * a.ldo + v] = ok ? (float)r : nanf32;
        }
    }
}

}  // namespace
}  // namespace dnmf

extern "C" {

long dnmf_running_windows(long T, int window, int stride) {
    dnmf::WindowPlan p;
    if (dnmf::window_plan("dnmf_running_windows", T, window, stride, p) != DNMF_OK) return 0;
    return p.J;
}

int dnmf_running_quantile(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, long T, int window,
                          int stride, double q, int run, float *lo, float *hi, int *n, long ldk, long *windows,
                          dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_running_quantile";
    DNMF_REQUIRE(frames && sz && lo && hi && n && windows, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    const long P = (long)sz[0] * sz[1] * sz[2];
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    WindowPlan w;
    const int rc = window_plan(fn, T, window, stride, w);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(q >= 0.0 && q <= 1.0, DNMF_E_SHAPE, "%s: q=%g outside [0, 1]", fn, q);
    DNMF_REQUIRE(B >= 1 && row0 >= 0 && row0 + B <= T, DNMF_E_SHAPE, "%s: rows %ld .. %ld of T=%ld frames", fn, row0, row0 + B, T);
    DNMF_REQUIRE(ldf >= P && ldk >= P, DNMF_E_SHAPE, "%s: ldf=%ld, ldk=%ld below a row of P=%ld", fn, ldf, ldk, P);
    DNMF_REQUIRE(run >= 0, DNMF_E_SHAPE, "%s: run=%d", fn, run);
    // the windows that lie wholly inside the rows given
    long j0 = 0;
    while (j0 < w.J && w.start(j0) < row0) ++j0;
    long j1 = j0;
    while (j1 < w.J && (long)w.start(j1) + w.Wn <= row0 + B) ++j1;
    windows[0] = j0, windows[1] = j1;
    if (j1 == j0) return DNMF_OK;
    const int V = tile_voxels(w.Wn), L = RQ_THREADS / V;
    const long ntiles = (P + V - 1) / V, nw = j1 - j0;
    long chosen = run;
    if (run == 0) {
        const long want = (RQ_TARGET_BLOCKS + ntiles - 1) / ntiles;
        chosen = (nw + want - 1) / want;
        if ((nw + chosen - 1) / chosen > 65535) chosen = (nw + 65534) / 65535;
    }
    if (chosen > nw) chosen = nw;
    const long nruns = (nw + chosen - 1) / chosen;
    DNMF_REQUIRE(nruns <= 65535, DNMF_E_UNSUPPORTED, "%s: %ld runs of %ld windows (they ride on gridDim.y: at most 65535)", fn, nruns, chosen);
    RQArgs a;
    a.frames = frames, a.ldf = ldf, a.P = P, a.ldk = ldk, a.frame_ids = frame_ids, a.w = w, a.row0 = (int)row0;
    a.j0 = j0, a.j1 = j1, a.run = (int)chosen, a.nk = (w.Wn + 2 * L - 1) / (2 * L), a.q = q, a.lo = lo, a.hi = hi, a.n = n;
    const size_t lds = (size_t)a.nk * RQ_THREADS * 2 * sizeof(uint32_t);
    const hipStream_t st = (hipStream_t)stream;
    if (V == 64) return launch_running_quantile<64>(fn, a, (unsigned)ntiles, (unsigned)nruns, lds, st);
    if (V == 32) return launch_running_quantile<32>(fn, a, (unsigned)ntiles, (unsigned)nruns, lds, st);
    return launch_running_quantile<16>(fn, a, (unsigned)ntiles, (unsigned)nruns, lds, st);
}

int dnmf_baseline_apply(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, const double *value,
                        long ldv, const double *centres, int J, int mode, double offset, float *out, long ldo,
                        dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_baseline_apply";
    DNMF_REQUIRE(frames && sz && value && centres && out, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    const long P = (long)sz[0] * sz[1] * sz[2];
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    DNMF_REQUIRE(B >= 1 && J >= 1 && row0 >= 0 && row0 <= 2147483647L - B, DNMF_E_SHAPE, "%s: B=%d rows from frame %ld, J=%d knots", fn, B,
                 row0, J);
    DNMF_REQUIRE(mode >= DNMF_BASELINE_F0 && mode <= DNMF_BASELINE_DFSQRTF, DNMF_E_SHAPE,
                 "%s: mode=%d (0 baseline, 1 df, 2 dff, 3 dfsqrtf)", fn, mode);
    DNMF_REQUIRE(offset - offset == 0.0, DNMF_E_SHAPE, "%s: offset=%g is not finite", fn, offset);
    DNMF_REQUIRE(ldf >= P && ldv >= P && ldo >= P, DNMF_E_SHAPE, "%s: ldf=%ld, ldv=%ld, ldo=%ld below a row of P=%ld", fn, ldf, ldv, ldo, P);
    // what the call is known to read of frames: every row without frame_ids, else no more than its first is certain
    const float *fend = frames + (frame_ids ? P : (long)(B - 1) * ldf + P), *oend = out + (long)(B - 1) * ldo + P;
    DNMF_REQUIRE(oend <= frames || fend <= out, DNMF_E_SHAPE, "%s: out aliases frames (a frame is read after others were written)", fn);
    BAArgs a;
    a.frames = frames, a.ldf = ldf, a.P = P, a.ldv = ldv, a.ldo = ldo, a.row0 = row0, a.frame_ids = frame_ids;
    a.value = value, a.centres = centres, a.B = B, a.J = J, a.mode = mode, a.offset = offset, a.out = out;
    a.chunk = BA_CHUNK;
    if (((long)B + a.chunk - 1) / a.chunk > 65535) a.chunk = (int)(((long)B + 65534) / 65535);
    hipLaunchKernelGGL(baseline_apply_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)((B + a.chunk - 1) / a.chunk)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return check_launch(fn);
}

}  // extern "C"
