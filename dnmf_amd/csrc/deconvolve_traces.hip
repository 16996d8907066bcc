// K21: spike deconvolution of the traces -- AR(1), non-negative.  include/dnmf_hip.h has the contract, tests/deconv_restatement.py the
// definition in float64 (D1 .. D6 below are its sections).
//
// One launch, one workgroup of DC_THREADS lanes per trace, everything in float64.  D1 is ar1_pools.hpp's pool-adjacent-violators
// solver (that header explains the scheme) with den_t = 1 on a valid frame; this file has the rest:
//   1  statistics of the trace: the valid frames, their mean, D3's two autocovariances; D2 and D4 select by bisection on the 64-bit
//      key of a value (one block-wide count per key bit, the keys in LDS), never by sorting;
//   2  solve(lam): the records of the lane's frames from the trace, then the local pools, the stitch and the expansion to c and s;
//   3  every lane adds its squared residuals in frame order; a wave reduces in a fixed tree, the waves are added in their order --
//      no floating-point atomics, the same input gives the same bits.
// D5's search for the penalty calls 2 and 3 in a loop inside the kernel (block-uniform control flow, no host synchronisation).
// Up to POOL_LDS_FRAMES frames the records live in LDS, longer traces keep them in the caller's workspace and only the 8 T bytes
// of keys in LDS.  The trace itself is read from its fp32 row (L2) whenever it is needed.
// The reductions and the selection helpers are those of block_ops.hpp, which K20 uses too.
#include <cmath>
#include <cstdint>

#include "ar1_pools.hpp"

namespace dnmf {
namespace {

constexpr int DC_THREADS = 1024;
constexpr int DC_MAX_ELEMS = POOL_DYNAMIC_LDS / 8;                 // 18 432: the longest trace whose keys fit LDS (K20's limit)
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
    char *records;   // workspace form: K blocks of POOL_RECORD * T bytes
};

// what solve() needs around a trace's pool records
struct Trace {
    Pools P;
    const float *row;
    double g, b;
    int *s_top, *s_last;      // DC_THREADS ints each
    void *red;
};

struct Solved {
    double rss;
    int positive, pools;   // frames with c > 0; pools
};

// D1 for the penalty lam.  WRITE: round c and s to the output rows.  Every lane of the workgroup must call it.
template <bool WRITE>
__device__ __forceinline__ Solved solve(const Trace &tr, double lam, float *c_out, float *s_out) {
    const Pools &P = tr.P;
    const double mu = 1.0 - tr.g;
    const int top = pools_local(P, [&](int t) {
        const double y = (double)tr.row[t];
        const bool w = isfinite(y);
        P.num[t] = (w ? y - tr.b : 0.0) - lam * (t < P.T - 1 ? mu : 1.0);
        P.den[t] = w ? 1.0 : 0.0;
    });
    pools_stitch<DC_THREADS>(P, top, tr.s_top);
    Solved r;
    r.rss = 0.0, r.positive = 0;
    r.pools = pools_expand<DC_THREADS>(P, tr.g, tr.s_last, [&](int t, double c, double s) {
        r.positive += c > 0.0;
        const double y = (double)tr.row[t];
        if (isfinite(y)) {
            const double e = y - tr.b - c;
            r.rss += e * e;
        }
        if (WRITE) c_out[t] = (float)c, s_out[t] = (float)s;
    });
    r.rss = block_reduce<DC_THREADS>(r.rss, OpSum(), tr.red);
    r.positive = block_reduce<DC_THREADS>(r.positive, OpSum(), tr.red);
    if (WRITE) r.pools = block_reduce<DC_THREADS>(r.pools, OpSum(), tr.red);
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
    Trace tr;
    tr.P = pools_over<DC_THREADS>(WS ? (void *)(a.records + (size_t)k * POOL_RECORD * (size_t)T) : (void *)dyn, T, log(g));
    tr.row = row, tr.g = g, tr.b = b, tr.s_top = s_top, tr.s_last = s_last, tr.red = red;
    __syncthreads();   // the keys are done with
    if (!has_lam) {
        const double target = sigma * sigma * (double)n_valid;
        lam = 0.0;
        if (!(solve<false>(tr, 0.0, nullptr, nullptr).rss >= target)) {
            double lo = 0.0, hi = sigma;
            for (int i = 0; i < DC_DOUBLINGS; ++i) {
                const Solved r = solve<false>(tr, hi, nullptr, nullptr);
                if (r.rss >= target || r.positive == 0) break;
                lo = hi, hi = 2.0 * hi;
            }
            for (int i = 0; i < DC_HALVINGS; ++i) {
                const double mid = 0.5 * (lo + hi);
                if (solve<false>(tr, mid, nullptr, nullptr).rss >= target) hi = mid;
                else lo = mid;
            }
            lam = hi;
        }
    }
    const Solved r = solve<true>(tr, lam, c_out, s_out);
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
    p.ws = T > POOL_LDS_FRAMES;
    p.bytes = DC_HEADER + (p.ws ? align256((size_t)K * (size_t)T * POOL_RECORD) : 0);
    p.lds = (unsigned)((size_t)T * (p.ws ? 8 : POOL_RECORD));
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
    const int rl = allow_dynamic_lds("dnmf_deconvolve_traces", fn, p.lds);
    if (rl != DNMF_OK) return rl;
    if (p.ws) hipLaunchKernelGGL(deconvolve_traces_kernel<true>, dim3((unsigned)K), dim3(DC_THREADS), p.lds, st, a);
    else hipLaunchKernelGGL(deconvolve_traces_kernel<false>, dim3((unsigned)K), dim3(DC_THREADS), p.lds, st, a);
    return check_launch("dnmf_deconvolve_traces");
}

}  // extern "C"
