// K21: spike deconvolution of the traces -- AR(1), non-negative.  include/dnmf_hip.h has the contract, tests/deconv_restatement.py the
// definition in float64 (D1 .. D6 below are its sections).
//
// One launch, one workgroup of DC_THREADS lanes per trace, everything in float64.  With x_t = c_t g^-t the AR(1) constraint
// c_t >= g c_{t-1} reads x_t >= x_{t-1}: a weighted isotonic regression, solved by pool-adjacent-violators (PAVA).
//   1  statistics of the trace: the valid frames, their mean, D3's two autocovariances; D2 and D4 select by bisection on the 64-bit
//      key of a value (one block-wide count per key bit, the keys in LDS), never by sorting;
//   2  solve(lam): lane i runs PAVA on its own `per` contiguous frames.  A pool's record (num, den, len, prev) sits in the slot of
//      its first frame, len = 0 marks a slot that starts no pool, prev chains the stack.  Then a stitch in log2(DC_THREADS) levels:
//      at the level of stride s the lanes i = 0, 2s, 4s, .. append the pools of the segments [i + s, i + 2s) to the stack of the
//      segments [i, i + s) one by one, merging backwards while they violate, and stop at the first pool that fits without a merge
//      (the rest of the right block is in order already).  The pairs of a level touch disjoint slots.
//   3  every lane expands the pools over its frames to c and s and adds its squared residuals in frame order; a wave reduces in a
//      fixed tree, the waves are added in their order -- no floating-point atomics, the same input gives the same bits.
// D5's search for the penalty calls 2 and 3 in a loop inside the kernel (block-uniform control flow, no host synchronisation).
// The records take 24 bytes a frame: up to DC_LDS_FRAMES frames they live in LDS, longer traces keep them in the caller's workspace
// and only the 8 T bytes of keys in LDS.  The trace itself is read from its fp32 row (L2) whenever it is needed.
// The reductions and the selection helpers are those of block_ops.hpp, which K20 uses too.
#include <cmath>
#include <cstdint>

#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int DC_THREADS = 1024;
constexpr int DC_STATIC_LDS = 16 * 1024;                           // bytes set aside for the static arrays below (they take 8.2 KiB)
constexpr int DC_DYNAMIC_LDS = 160 * 1024 - DC_STATIC_LDS;
constexpr int DC_RECORD = 24;                                      // bytes of a pool record: num, den (double), len, prev (int)
constexpr int DC_LDS_FRAMES = DC_DYNAMIC_LDS / DC_RECORD;          // 6144: the longest trace whose records fit LDS
constexpr int DC_MAX_ELEMS = DC_DYNAMIC_LDS / 8;                   // 18 432: the longest trace whose keys fit LDS (K20's limit)
constexpr size_t DC_HEADER = 256;
constexpr int DC_DOUBLINGS = 64, DC_HALVINGS = 32, DC_MIN_VALID = 4;   // tests/deconv_restatement.py: DOUBLINGS, HALVINGS, MIN_VALID
constexpr int DC_INFO = 8;                                         // doubles of info per trace

struct DcArgs {
    const float *in;
    long ldi, ldo;
    int K, T;
    const double *g, *penalty, *baseline, *noise;
    double pct;
    float *c, *s;
    double *info;
    char *records;   // workspace form: K blocks of DC_RECORD * T bytes
};

// a trace's pool records (LDS or workspace) and what solve() needs around them
struct Pools {
    double *num, *den;
    int *len, *prev;
    const float *row;
    int T, c0, c1, per;       // this lane's frames [c0, c1), `per` frames a lane
    double g, lng, b;
    int *s_top, *s_last;      // DC_THREADS ints each
    void *red;
};

__device__ __forceinline__ bool violates(const Pools &P, int p, int q) {
    const double dp = P.den[p];
    if (!(dp > 0.0)) return false;   // only a leading run of missing frames: never merged into
    const double dq = P.den[q];
    if (!(dq > 0.0)) return true;    // missing frames merge backwards
    return P.num[q] / dq < (P.num[p] / dp) * exp((double)P.len[p] * P.lng);
}

__device__ __forceinline__ void merge(const Pools &P, int p, int q) {
    const double gl = exp((double)P.len[p] * P.lng);
    P.num[p] = P.num[p] + gl * P.num[q];
    P.den[p] = P.den[p] + gl * gl * P.den[q];
    P.len[p] = P.len[p] + P.len[q];
    P.len[q] = 0;
}

// merge p backwards while it violates -> the pool it ends up in
__device__ __forceinline__ int settle(const Pools &P, int p) {
    for (;;) {
        const int pp = P.prev[p];
        if (pp < 0 || !violates(P, pp, p)) return p;
        merge(P, pp, p);
        p = pp;
    }
}

struct Solved {
    double rss;
    int positive, pools;   // frames with c > 0; pools
};

// D1 for the penalty lam.  WRITE: round c and s to the output rows.  Every lane of the workgroup must call it.
template <bool WRITE>
__device__ __forceinline__ Solved solve(const Pools &P, double lam, float *c_out, float *s_out) {
    const int tid = threadIdx.x, T = P.T;
    const double mu = 1.0 - P.g;
    // PAVA on the lane's own frames
    int top = -1;
    for (int t = P.c0; t < P.c1; ++t) {
        const double y = (double)P.row[t];
        const bool w = isfinite(y);
        P.num[t] = (w ? y - P.b : 0.0) - lam * (t < T - 1 ? mu : 1.0);
        P.den[t] = w ? 1.0 : 0.0;
        P.len[t] = 1, P.prev[t] = top;
        top = settle(P, t);
    }
    P.s_top[tid] = top;
    __syncthreads();
    // the stitch: block [tid, tid + s) of segments takes in block [tid + s, tid + 2 s)
    for (int s = 1; s < DC_THREADS; s <<= 1) {
        if ((tid & (2 * s - 1)) == 0) {
            const long first = (long)(tid + s) * P.per;
            if (first < T) {
                const int end = (int)min((long)T, (long)(tid + 2 * s) * P.per);
                int p = P.s_top[tid], q = (int)first;
                while (q < end) {
                    if (!violates(P, p, q)) {
                        P.prev[q] = p;
                        break;
                    }
                    const int nxt = q + max(P.len[q], 1);   // a pool start: len >= 1
                    merge(P, p, q);
                    p = settle(P, p);
                    q = nxt;
                }
                P.s_top[tid] = q >= end ? p : P.s_top[tid + s];
            }
        }
        __syncthreads();
    }
    // the last pool start at or before the end of every lane's frames
    int last = -1;
    for (int t = P.c0; t < P.c1; ++t)
        if (P.len[t] > 0) last = t;
    P.s_last[tid] = last;
    __syncthreads();
    Solved r;
    r.rss = 0.0, r.positive = 0, r.pools = 0;
    if (P.c0 < P.c1) {
        int cur = -1;                                   // the pool that covers frame c0 - 1
        for (int l = tid - 1; l >= 0 && cur < 0; --l) cur = P.s_last[l];
        double cv = 0.0, cprev = 0.0;                   // the pool's max(v, 0); c of the frame before
        if (cur >= 0) {
            const double d = P.den[cur];
            cv = d > 0.0 ? fmax(P.num[cur] / d, 0.0) : 0.0;
            cprev = cv * exp((double)(P.c0 - 1 - cur) * P.lng);
        }
        for (int t = P.c0; t < P.c1; ++t) {
            double c, s = 0.0;
            if (P.len[t] > 0) {
                cur = t, ++r.pools;
                const double d = P.den[t];
                cv = d > 0.0 ? fmax(P.num[t] / d, 0.0) : 0.0;
                c = cv;
                s = t == 0 ? c : fmax(c - P.g * cprev, 0.0);
            } else {
                c = cv * exp((double)(t - cur) * P.lng);
            }
            cprev = c;
            r.positive += c > 0.0;
            const double y = (double)P.row[t];
            if (isfinite(y)) {
                const double e = y - P.b - c;
                r.rss += e * e;
            }
            if (WRITE) c_out[t] = (float)c, s_out[t] = (float)s;
        }
    }
    r.rss = block_reduce<DC_THREADS>(r.rss, OpSum(), P.red);
    r.positive = block_reduce<DC_THREADS>(r.positive, OpSum(), P.red);
    if (WRITE) r.pools = block_reduce<DC_THREADS>(r.pools, OpSum(), P.red);
    return r;   // the reductions end with a barrier: the records may be written again
}

__device__ __forceinline__ bool given(const double *a, int k, double &v) {
    v = a ? a[k] : quiet_nan();
    return v == v;
}

template <bool WS>
__global__ __launch_bounds__(DC_THREADS) void deconvolve_traces_kernel(DcArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ double red[DC_THREADS / 64];
    __shared__ int s_top[DC_THREADS], s_last[DC_THREADS];
    const int k = blockIdx.x, tid = threadIdx.x, T = a.T;
    const float *row = a.in + (long)k * a.ldi;
    float *c_out = a.c + (long)k * a.ldo, *s_out = a.s + (long)k * a.ldo;
    double *info = a.info + (size_t)k * DC_INFO;

    // ---- the statistics of the trace
    int n_valid = 0, n1 = 0, n2 = 0;
    double sum = 0.0;
    for (int t = tid; t < T; t += DC_THREADS) {
        const double y = (double)row[t];
        if (isfinite(y)) {
            ++n_valid, sum += y;
            if (t + 1 < T && isfinite((double)row[t + 1])) ++n1;
            if (t + 2 < T && isfinite((double)row[t + 2])) ++n2;
        }
    }
    n_valid = block_reduce<DC_THREADS>(n_valid, OpSum(), red), n1 = block_reduce<DC_THREADS>(n1, OpSum(), red), n2 = block_reduce<DC_THREADS>(n2, OpSum(), red);
    sum = block_reduce<DC_THREADS>(sum, OpSum(), red);
    double g, lam, b, sigma;
    const bool has_g = given(a.g, k, g), has_lam = given(a.penalty, k, lam), has_b = given(a.baseline, k, b);
    const bool has_sigma = given(a.noise, k, sigma);
    bool ok = n_valid >= DC_MIN_VALID && !(((!has_lam && !has_sigma) || !has_g) && n1 < 2);
    if (ok && !has_g) {   // D3
        const double m = sum / (double)n_valid;
        double p1 = 0.0, p2 = 0.0;
        for (int t = tid; t < T; t += DC_THREADS) {
            const double y = (double)row[t];
            if (isfinite(y)) {
                const double y1 = t + 1 < T ? (double)row[t + 1] : quiet_nan(), y2 = t + 2 < T ? (double)row[t + 2] : quiet_nan();
                if (isfinite(y1)) p1 += (y - m) * (y1 - m);
                if (isfinite(y2)) p2 += (y - m) * (y2 - m);
            }
        }
        p1 = block_reduce<DC_THREADS>(p1, OpSum(), red), p2 = block_reduce<DC_THREADS>(p2, OpSum(), red);
        const double ac1 = p1 / (double)n1, ac2 = n2 > 0 ? p2 / (double)n2 : quiet_nan();
        g = ac1 > 0.0 ? ac2 / ac1 : quiet_nan();
    }
    ok = ok && g > 0.0 && g < 1.0;
    uint64_t *key = reinterpret_cast<uint64_t *>(dyn);
    if (ok && !has_b) {   // D4
        for (int t = tid; t < T; t += DC_THREADS) {
            const double y = (double)row[t];
            dyn[t] = isfinite(y) ? y : quiet_nan();
        }
        const int lowbit = to_keys<DC_THREADS>(dyn, T, red);
        double pos = (double)n_valid * a.pct / 100.0 - 0.5;
        pos = fmin(fmax(pos, 0.0), (double)(n_valid - 1));
        const double fl = floor(pos);
        double v0, v1;
        block_select_pair<DC_THREADS, false>(key, T, 0, (int)fl, n_valid, lowbit, red, v0, v1);
        b = v0 + (pos - fl) * (v1 - v0);
    }
    ok = ok && isfinite(b) && !(has_lam && lam < 0.0);
    if (ok && !has_sigma) {   // D2
        if (n1 >= 2) {
            for (int t = tid; t < T; t += DC_THREADS) {
                const double y0 = (double)row[t], y1 = t + 1 < T ? (double)row[t + 1] : quiet_nan();
                dyn[t] = isfinite(y0) && isfinite(y1) ? y1 - y0 : quiet_nan();
            }
            int lowbit = to_keys<DC_THREADS>(dyn, T, red);
            const double med = block_median<DC_THREADS>(key, T, n1, lowbit, red);
            for (int t = tid; t < T; t += DC_THREADS) {
                const double y0 = (double)row[t], y1 = t + 1 < T ? (double)row[t + 1] : quiet_nan();
                dyn[t] = isfinite(y0) && isfinite(y1) ? fabs((y1 - y0) - med) : quiet_nan();
            }
            lowbit = to_keys<DC_THREADS>(dyn, T, red);
            sigma = 1.4826 * block_median<DC_THREADS>(key, T, n1, lowbit, red) / sqrt(2.0);
        } else {
            sigma = quiet_nan();
        }
    }
    if (!ok) {   // D6 (block-uniform)
        const float nanf_ = __int_as_float(0x7fc00000);
        for (int t = tid; t < T; t += DC_THREADS) c_out[t] = nanf_, s_out[t] = nanf_;
        if (tid == 0) {
            for (int i = 0; i < 5; ++i) info[i] = quiet_nan();
            info[5] = (double)n_valid, info[6] = 0.0, info[7] = 0.0;
        }
        return;
    }

    // ---- D1 / D5
    Pools P;
    if (WS) {
        char *rec = a.records + (size_t)k * DC_RECORD * (size_t)T;
        P.num = reinterpret_cast<double *>(rec), P.den = P.num + T;
        P.len = reinterpret_cast<int *>(P.den + T), P.prev = P.len + T;
    } else {
        P.num = dyn, P.den = dyn + T;
        P.len = reinterpret_cast<int *>(dyn + 2 * (size_t)T), P.prev = P.len + T;
    }
    P.row = row, P.T = T, P.per = (T + DC_THREADS - 1) / DC_THREADS;
    P.c0 = (int)min((long)T, (long)tid * P.per), P.c1 = min(T, P.c0 + P.per);
    P.g = g, P.lng = log(g), P.b = b, P.s_top = s_top, P.s_last = s_last, P.red = red;
    __syncthreads();   // the keys are done with
    if (!has_lam) {
        const double target = sigma * sigma * (double)n_valid;
        lam = 0.0;
        if (!(solve<false>(P, 0.0, nullptr, nullptr).rss >= target)) {
            double lo = 0.0, hi = sigma;
            for (int i = 0; i < DC_DOUBLINGS; ++i) {
                const Solved r = solve<false>(P, hi, nullptr, nullptr);
                if (r.rss >= target || r.positive == 0) break;
                lo = hi, hi = 2.0 * hi;
            }
            for (int i = 0; i < DC_HALVINGS; ++i) {
                const double mid = 0.5 * (lo + hi);
                if (solve<false>(P, mid, nullptr, nullptr).rss >= target) hi = mid;
                else lo = mid;
            }
            lam = hi;
        }
    }
    const Solved r = solve<true>(P, lam, c_out, s_out);
    if (tid == 0) {
        info[0] = g, info[1] = lam, info[2] = b, info[3] = sigma, info[4] = r.rss;
        info[5] = (double)n_valid, info[6] = (double)r.pools, info[7] = 1.0;
    }
}

struct DcPlan {
    size_t bytes;
    unsigned lds;
    bool ws;
};

int dc_plan(const char *fn, int K, int T, DcPlan &p) {
    DNMF_REQUIRE(K >= 1 && T >= 1, DNMF_E_SHAPE, "%s: K=%d traces, T=%d frames", fn, K, T);
    DNMF_REQUIRE(T <= DC_MAX_ELEMS && K <= DC_MAX_ELEMS, DNMF_E_UNSUPPORTED,
                 "%s: K=%d, T=%d: at most %d traces of at most %d frames (a trace's float64 keys must fit LDS)", fn, K, T,
                 DC_MAX_ELEMS, DC_MAX_ELEMS);
    p.ws = T > DC_LDS_FRAMES;
    p.bytes = DC_HEADER + (p.ws ? align256((size_t)K * (size_t)T * DC_RECORD) : 0);
    p.lds = (unsigned)((size_t)T * (p.ws ? 8 : DC_RECORD));
    p.lds = (p.lds + 15u) & ~15u;
    return DNMF_OK;
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_deconvolve_traces_workspace(int K, int T) {
    dnmf::DcPlan p;
    if (dnmf::dc_plan("dnmf_deconvolve_traces_workspace", K, T, p) != DNMF_OK) return 0;
    return p.bytes;
}

int dnmf_deconvolve_traces(const float *traces, long ldt, int K, int T, const double *g, const double *penalty, const double *baseline,
                           const double *noise, double baseline_percentile, float *c, float *s, long ldo, double *info, void *workspace,
                           size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(traces && c && s && info && workspace, DNMF_E_NULL, "dnmf_deconvolve_traces: NULL argument");
    DcPlan p;
    const int rc = dc_plan("dnmf_deconvolve_traces", K, T, p);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldt >= T && ldo >= T, DNMF_E_SHAPE, "dnmf_deconvolve_traces: ldt=%ld ldo=%ld below a row of T=%d", ldt, ldo, T);
    DNMF_REQUIRE(baseline_percentile >= 0.0 && baseline_percentile <= 100.0, DNMF_E_SHAPE,
                 "dnmf_deconvolve_traces: baseline_percentile=%g", baseline_percentile);
    DNMF_REQUIRE(workspace_bytes >= p.bytes, DNMF_E_WORKSPACE, "dnmf_deconvolve_traces: workspace of %zu bytes, need %zu",
                 workspace_bytes, p.bytes);
    DNMF_REQUIRE(((size_t)workspace & 7) == 0, DNMF_E_WORKSPACE, "dnmf_deconvolve_traces: workspace must be 8-byte aligned");
    DcArgs a;
    a.in = traces, a.ldi = ldt, a.ldo = ldo, a.K = K, a.T = T;
    a.g = g, a.penalty = penalty, a.baseline = baseline, a.noise = noise, a.pct = baseline_percentile;
    a.c = c, a.s = s, a.info = info, a.records = static_cast<char *>(workspace) + DC_HEADER;
    const hipStream_t st = (hipStream_t)stream;
    const void *fn = p.ws ? (const void *)deconvolve_traces_kernel<true> : (const void *)deconvolve_traces_kernel<false>;
    if (p.lds > 48u * 1024u) {   // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return fail((int)e, "dnmf_deconvolve_traces: %u bytes of LDS: %s", p.lds, hipGetErrorString(e));
    }
    if (p.ws) hipLaunchKernelGGL(deconvolve_traces_kernel<true>, dim3((unsigned)K), dim3(DC_THREADS), p.lds, st, a);
    else hipLaunchKernelGGL(deconvolve_traces_kernel<false>, dim3((unsigned)K), dim3(DC_THREADS), p.lds, st, a);
    return check_launch("dnmf_deconvolve_traces");
}

}  // extern "C"
