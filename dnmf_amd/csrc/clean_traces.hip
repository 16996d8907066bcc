// K20: trace clean-up -- mask, outliers, bleach detrend, dF/F0, gap filling, smoothing, rescale.  include/dnmf_hip.h has the
// contract, tests/traces_restatement.py the definition in float64 (S1 .. S6 below are its steps).
//
// One workgroup of CT_THREADS lanes per trace, the working trace as float64 in LDS (8 T bytes), three launches on one stream:
//   A  per trace: S1, S2, F0 and, for modes 2 / 3, the running median and the exponential fit; mode 1 scales the trace instead.
//      The trace after S2 goes to the workspace (wx), where C picks it up.
//   B  one workgroup, modes 1 and 3 only: mode 1's frame mean over the traces, its running median and fit; mode 3's median of F0.
//   C  per trace: subtract the curve / divide by F0, S4, S5, S6, round once to fp32.
// Order statistics select by bisection on the monotone 64-bit key of a value: a window median takes one counting pass over the
// window per key bit (lane t reads key[lo + j]: neighbouring lanes, neighbouring LDS words), the percentile and the median of F0 one
// block-wide count per bit.  Bits below the lowest set bit of any value of the trace are skipped (a trace that came from fp32 has at
// least 28 of them).  Sums: a lane adds its frames t = lane, lane + CT_THREADS, ... in that order, a wave reduces in a fixed tree,
// the waves are added in their order (block_ops.hpp, which also has the key helpers) -- no floating-point atomics, the same input
// gives the same bits.
#include <cmath>
#include <cstdint>

#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int CT_THREADS = 1024;
constexpr int CT_STATIC_LDS = 16 * 1024;                   // bytes set aside for the static arrays below (they take 8.2 KiB)
constexpr int CT_MAX_ELEMS = (160 * 1024 - CT_STATIC_LDS) / 8;   // doubles of the dynamic part: 18 432
constexpr size_t CT_HEADER = 256;                          // bytes: a, b, fitted of mode 1, median F0 of mode 3
constexpr int CT_FIT_ITERS = 20, CT_FIT_HALVINGS = 10;     // tests/traces_restatement.py: FIT_ITERS, FIT_HALVINGS
constexpr double CT_FIT_SLACK = 1e-8;                      // FIT_SLACK there

// Median of key[lo..hi] (lo <= hi inside the array) without its NANKEYs; NaN when nothing is left, or, with INCLUDENAN, when one
// entry is a NANKEY.  One pass over the window per key bit from 63 down to lowbit; an even count takes the float64 mean of the two
// middle values.
template <bool INCLUDENAN>
__device__ __forceinline__ double window_median(const uint64_t *key, int lo, int hi, int lowbit) {
    int n = 0;
    for (int j = lo; j <= hi; ++j) n += key[j] != NANKEY;
    if (n == 0 || (INCLUDENAN && n != hi - lo + 1)) return quiet_nan();
    const int k = (n - 1) >> 1;
    uint64_t pre = 0;
    for (int bit = 63; bit >= lowbit; --bit) {
        const uint64_t cand = pre | (1ull << bit);
        int c = 0;
        for (int j = lo; j <= hi; ++j) c += key[j] < cand;
        if (c <= k) pre = cand;
    }
    const double m = from_key(pre);
    if (n & 1) return m;
    int cle = 0;
    uint64_t nxt = NANKEY;
    for (int j = lo; j <= hi; ++j) {
        const uint64_t kk = key[j];
        cle += kk <= pre;
        if (kk > pre && kk < nxt) nxt = kk;
    }
    return 0.5 * (m + from_key(cle >= k + 2 ? pre : nxt));
}

// out[t] = the median of the W frames around t (window [t - W/2, t - W/2 + W - 1], cut at the ends) of key[0..T)
template <bool INCLUDENAN>
__device__ __forceinline__ void running_median(const uint64_t *key, int T, int W, int lowbit, double *out) {
    const int h = W / 2;
    for (int t = threadIdx.x; t < T; t += CT_THREADS) {
        const int lo = max(0, t - h), hi = (int)min((long)T - 1, (long)t - h + W - 1);
        out[t] = hi >= lo ? window_median<INCLUDENAN>(key, lo, hi, lowbit) : quiet_nan();
    }
}

// ---- the exponential fit -------------------------------------------------------------------------------------------------------
struct FitEval {
    double a, f, db;
};

// For the decay b: a = the least-squares amplitude, f = the squared error, db = the Gauss-Newton step of b with a eliminated
// (the model's derivative a (x - c) e with e projected out).  y: LDS, NaN = no sample; x_t = t + 1.
__device__ __forceinline__ FitEval fit_eval(const double *y, int T, double b, void *red) {
    double see = 0.0, sye = 0.0, sxee = 0.0;
    for (int t = threadIdx.x; t < T; t += CT_THREADS) {
        const double v = y[t];
        if (v == v) {
            const double x = (double)(t + 1), e = exp(b * x);
            see += e * e, sye += v * e, sxee += x * e * e;
        }
    }
    see = block_reduce<CT_THREADS>(see, OpSum(), red), sye = block_reduce<CT_THREADS>(sye, OpSum(), red), sxee = block_reduce<CT_THREADS>(sxee, OpSum(), red);
    FitEval r;
    r.a = sye / see;
    const double c = sxee / see;
    double f = 0.0, num = 0.0, den = 0.0;
    for (int t = threadIdx.x; t < T; t += CT_THREADS) {
        const double v = y[t];
        if (v == v) {
            const double x = (double)(t + 1), e = exp(b * x);
            const double res = v - r.a * e, u = (x - c) * e;
            f += res * res, num += u * res, den += u * u;
        }
    }
    r.f = block_reduce<CT_THREADS>(f, OpSum(), red), num = block_reduce<CT_THREADS>(num, OpSum(), red), den = block_reduce<CT_THREADS>(den, OpSum(), red);
    const double q = num / (r.a * den);
    r.db = (r.a * den != 0.0 && isfinite(q)) ? q : 0.0;
    return r;
}

// least-squares a exp(b x) on the samples of y: the log-linear fit of the positive ones, then damped Gauss-Newton steps
__device__ __forceinline__ void fit_exp(const double *y, int T, void *red, double &a_out, double &b_out) {
    double ymax = quiet_nan();
    int npos = 0;
    double sx = 0.0;
    for (int t = threadIdx.x; t < T; t += CT_THREADS) {
        const double v = y[t];
        if (v == v) ymax = fmax(ymax, v);
        if (v > 0.0) ++npos, sx += (double)(t + 1);
    }
    ymax = block_reduce<CT_THREADS>(ymax, OpFmax(), red), npos = block_reduce<CT_THREADS>(npos, OpSum(), red), sx = block_reduce<CT_THREADS>(sx, OpSum(), red);
    double b = 0.0;
    if (npos >= 2) {
        const double lmax = log(ymax), xm = sx / (double)npos;
        double num = 0.0, den = 0.0;
        for (int t = threadIdx.x; t < T; t += CT_THREADS) {
            const double v = y[t];
            if (v > 0.0) {
                const double dx = (double)(t + 1) - xm;
                num += dx * (log(v) - lmax), den += dx * dx;
            }
        }
        num = block_reduce<CT_THREADS>(num, OpSum(), red), den = block_reduce<CT_THREADS>(den, OpSum(), red);
        if (den > 0.0) b = num / den;
    }
    FitEval cur = fit_eval(y, T, b, red);
    for (int it = 0; it < CT_FIT_ITERS; ++it) {
        double lam = 1.0;
        bool moved = false;
        for (int h = 0; h < CT_FIT_HALVINGS; ++h) {
            const double bn = b + lam * cur.db;
            const FitEval nxt = fit_eval(y, T, bn, red);
            if (nxt.f <= cur.f * (1.0 + CT_FIT_SLACK)) {   // false for a NaN
                cur = nxt, b = bn, moved = true;
                break;
            }
            lam *= 0.5;
        }
        if (!moved) break;
    }
    a_out = cur.a, b_out = b;
}

// ---- arguments -----------------------------------------------------------------------------------------------------------------
struct CtArgs {
    const float *in;
    long ldi, ldo;
    int K, T, lead, trim, mode, W, interp, smooth, sw;
    double floor_, sigma;
    float *out;
    double *scales, *offsets, *a, *b, *F0;
    int *fitted, *nout;
    double *hdr, *wx, *wy;   // workspace: header, the trace after S2 (K, T), a second row per trace (K, T)
};

// running median of x[0..T) (LDS, destroyed: left as keys) into grow (a global row), back into x; -> valid outputs
template <bool INCLUDENAN>
__device__ __forceinline__ int median_through(double *x, int T, int W, double *grow, void *red) {
    const int lowbit = to_keys<CT_THREADS>(x, T, red);
    running_median<INCLUDENAN>(reinterpret_cast<const uint64_t *>(x), T, W, lowbit, grow);
    __syncthreads();
    int nv = 0;
    for (int t = threadIdx.x; t < T; t += CT_THREADS) {   // a lane reads back what it wrote itself
        const double v = grow[t];
        x[t] = v, nv += v == v;
    }
    __syncthreads();
    return block_reduce<CT_THREADS>(nv, OpSum(), red);
}

// ---- phase A -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void clean_traces_a_kernel(CtArgs g) {
    extern __shared__ __attribute__((aligned(16))) double x[];
    __shared__ double red[CT_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, T = g.T;
    const float *row = g.in + (long)k * g.ldi;
    double *wx = g.wx + (size_t)k * T, *wy = g.wy + (size_t)k * T;
    // S1
    for (int t = tid; t < T; t += CT_THREADS) {
        double v = (double)row[t];
        if (!isfinite(v) || v <= g.floor_ || (g.trim && (t < g.lead || t == T - 1))) v = quiet_nan();
        x[t] = v;
    }
    __syncthreads();
    // S2
    int nout = 0;
    if (g.sigma > 0.0) {
        int n = 0;
        double s = 0.0;
        for (int t = tid; t < T; t += CT_THREADS) {
            const double v = x[t];
            if (v == v) ++n, s += v;
        }
        n = block_reduce<CT_THREADS>(n, OpSum(), red), s = block_reduce<CT_THREADS>(s, OpSum(), red);
        const double mean = s / (double)n;
        double q = 0.0;
        for (int t = tid; t < T; t += CT_THREADS) {
            const double v = x[t];
            if (v == v) q += (v - mean) * (v - mean);
        }
        q = block_reduce<CT_THREADS>(q, OpSum(), red);
        const double thr = g.sigma * sqrt(q / (double)(n - 1)) + mean;
        unsigned flags = 0;   // bit i: frame tid + i CT_THREADS is extreme (T <= CT_MAX_ELEMS: at most 18 frames a lane)
        int i = 0;
        for (int t = tid; t < T; t += CT_THREADS, ++i) {
            if (t >= 1 && t <= T - 2) {
                const double d0 = x[t] - x[t - 1], d1 = x[t + 1] - x[t];
                if ((d0 > thr && d1 < -thr) || (d0 < -thr && d1 > thr)) flags |= 1u << i, ++nout;
            }
        }
        __syncthreads();
        i = 0;
        for (int t = tid; t < T; t += CT_THREADS, ++i)
            if (flags >> i & 1) x[t] = quiet_nan();
        __syncthreads();
        nout = block_reduce<CT_THREADS>(nout, OpSum(), red);
        // median of three, the window cut at the ends; a NaN in it gives NaN
        for (int t = tid; t < T; t += CT_THREADS) {
            const double c = x[t];
            double m;
            if (T == 1) m = c;
            else if (t == 0) m = 0.5 * (c + x[1]);
            else if (t == T - 1) m = 0.5 * (x[T - 2] + c);
            else {
                const double l = x[t - 1], r = x[t + 1];
                m = fmax(fmin(l, c), fmin(fmax(l, c), r));
                if (l != l || c != c || r != r) m = quiet_nan();
            }
            wx[t] = m;
        }
        __syncthreads();
        for (int t = tid; t < T; t += CT_THREADS) x[t] = wx[t];
        __syncthreads();
    } else {
        for (int t = tid; t < T; t += CT_THREADS) wx[t] = x[t];
    }
    double F0 = quiet_nan(), a = quiet_nan(), b = quiet_nan(), scale = 1.0, offset = 0.0;
    int fitted = 0;
    if (g.mode > 0) {
        // F0: the 5th percentile of the entries > 0.1 (MATLAB's prctile)
        const int lowbit = to_keys<CT_THREADS>(x, T, red);
        const uint64_t *key = reinterpret_cast<const uint64_t *>(x);
        const uint64_t above = to_key(0.1);
        int n = 0;
        for (int t = tid; t < T; t += CT_THREADS) n += key[t] > above && key[t] != NANKEY;
        n = block_reduce<CT_THREADS>(n, OpSum(), red);
        if (n > 0) {
            double pos = (double)n * 5.0 / 100.0 - 0.5;
            pos = fmin(fmax(pos, 0.0), (double)(n - 1));
            const double fl = floor(pos);
            double v0, v1;
            block_select_pair<CT_THREADS>(key, T, above, (int)fl, n, lowbit, red, v0, v1);
            F0 = v0 + (pos - fl) * (v1 - v0);
        }
        if (g.mode == 1) {
            // the reference's global variant: every trace to [0, 1] first
            for (int t = tid; t < T; t += CT_THREADS) x[t] = wx[t];
            __syncthreads();
            double lo = quiet_nan(), hi = quiet_nan();
            for (int t = tid; t < T; t += CT_THREADS) lo = fmin(lo, x[t]);
            offset = block_reduce<CT_THREADS>(lo, OpFmin(), red);
            for (int t = tid; t < T; t += CT_THREADS) hi = fmax(hi, x[t] - offset);
            scale = block_reduce<CT_THREADS>(hi, OpFmax(), red);
            for (int t = tid; t < T; t += CT_THREADS) wx[t] = (x[t] - offset) / scale;
        } else {
            running_median<false>(key, T, g.W, lowbit, wy);
            __syncthreads();
            int nv = 0;
            for (int t = tid; t < T; t += CT_THREADS) {
                const double v = wy[t];
                x[t] = v, nv += v == v;
            }
            __syncthreads();
            nv = block_reduce<CT_THREADS>(nv, OpSum(), red);
            fitted = (double)nv > 0.1 * (double)T;
            if (fitted) fit_exp(x, T, red, a, b);
        }
    }
    if (tid == 0) {
        g.F0[k] = F0, g.a[k] = a, g.b[k] = b, g.fitted[k] = fitted, g.nout[k] = nout;
        g.scales[k] = scale, g.offsets[k] = offset;
    }
}

// ---- phase B -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void clean_traces_b_kernel(CtArgs g) {
    extern __shared__ __attribute__((aligned(16))) double x[];
    __shared__ double red[CT_THREADS / 64];
    const int tid = threadIdx.x, T = g.T, K = g.K;
    if (g.mode == 1) {
        for (int t = tid; t < T; t += CT_THREADS) {   // the mean over the traces, in their order
            double s = 0.0;
            int n = 0;
            for (int k = 0; k < K; ++k) {
                const double v = g.wx[(size_t)k * T + t];
                if (v == v) s += v, ++n;
            }
            x[t] = n ? s / (double)n : quiet_nan();
        }
        __syncthreads();
        const int nv = median_through<false>(x, T, g.W, g.wy, red);
        double a = quiet_nan(), b = quiet_nan();
        const int fitted = (double)nv > 0.1 * (double)T;
        if (fitted) fit_exp(x, T, red, a, b);
        if (tid == 0) g.hdr[0] = a, g.hdr[1] = b, g.hdr[2] = (double)fitted;
    } else {   // mode 3: the median of the F0 that are no NaN
        for (int k = tid; k < K; k += CT_THREADS) x[k] = g.F0[k];
        __syncthreads();
        to_keys<CT_THREADS>(x, K, red);   // its lowest bit is not used: every bit is searched
        const uint64_t *key = reinterpret_cast<const uint64_t *>(x);
        int n = 0;
        for (int k = tid; k < K; k += CT_THREADS) n += key[k] != NANKEY;
        n = block_reduce<CT_THREADS>(n, OpSum(), red);
        const double med = n > 0 ? block_median<CT_THREADS>(key, K, n, 0, red) : quiet_nan();
        if (tid == 0) g.hdr[3] = med;
    }
}

// ---- phase C -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void clean_traces_c_kernel(CtArgs g) {
    extern __shared__ __attribute__((aligned(16))) double x[];
    __shared__ double red[CT_THREADS / 64];
    __shared__ int s_first[CT_THREADS], s_last[CT_THREADS];
    const int k = blockIdx.x, tid = threadIdx.x, T = g.T;
    const double *wx = g.wx + (size_t)k * T;
    double *wy = g.wy + (size_t)k * T;
    double scale = g.scales[k], offset = g.offsets[k], doff = 0.0;
    for (int t = tid; t < T; t += CT_THREADS) x[t] = wx[t];
    // S3: subtract a decaying curve; mode 3 divides by the common F0
    if (g.mode > 0) {
        double a = g.a[k], b = g.b[k];
        int fitted = g.fitted[k];
        if (g.mode == 1) a = g.hdr[0], b = g.hdr[1], fitted = g.hdr[2] != 0.0;
        if (fitted && b < 0.0) {
            doff = a;
            for (int t = tid; t < T; t += CT_THREADS) x[t] = x[t] - a * exp(b * (double)(t + 1));
        }
        if (g.mode == 1 && tid == 0) g.a[k] = a, g.b[k] = b, g.fitted[k] = fitted;
        if (g.mode == 3) {
            const double med = g.hdr[3];
            scale = med < 1.0 ? 1.0 : med, offset = 0.0;
            for (int t = tid; t < T; t += CT_THREADS) x[t] = x[t] / scale;
            if (tid == 0) g.F0[k] = med;
        }
    }
    __syncthreads();
    // S4: NaNs between two samples lie on the line through them.  A lane owns `per` contiguous frames.
    if (g.interp) {
        const int per = (T + CT_THREADS - 1) / CT_THREADS;
        const int c0 = min(T, tid * per), c1 = min(T, c0 + per);
        int first = -1, last = -1;
        for (int t = c0; t < c1; ++t)
            if (x[t] == x[t]) {
                if (first < 0) first = t;
                last = t;
            }
        s_first[tid] = first, s_last[tid] = last;
        __syncthreads();
        int l = -1, rnext = -1;
        for (int c = tid - 1; c >= 0 && l < 0; --c) l = s_last[c];
        for (int c = tid + 1; c < CT_THREADS && rnext < 0; ++c) rnext = s_first[c];
        for (int t = c0; t < c1; ++t) {
            if (x[t] == x[t]) {
                l = t;
                continue;
            }
            int r = rnext;
            for (int u = t + 1; u < c1; ++u)   // frames ahead in the chunk are still as they were
                if (x[u] == x[u]) {
                    r = u;
                    break;
                }
            if (l >= 0 && r >= 0) {
                const double slope = (x[r] - x[l]) / (double)(r - l);
                x[t] = slope * (double)(t - l) + x[l];
            }
        }
        __syncthreads();
    }
    // S5
    if (g.smooth == 1) {
        const int h = g.sw / 2;
        for (int t = tid; t < T; t += CT_THREADS) {
            const int lo = max(0, t - h), hi = (int)min((long)T - 1, (long)t - h + g.sw - 1);
            double s = quiet_nan();
            if (hi >= lo) {
                s = x[lo];
                for (int j = lo + 1; j <= hi; ++j) s += x[j];
                s = s / (double)(hi - lo + 1);
            }
            wy[t] = s;
        }
        __syncthreads();
        for (int t = tid; t < T; t += CT_THREADS) x[t] = wy[t];
        __syncthreads();
    } else if (g.smooth == 2) {
        median_through<true>(x, T, g.sw, wy, red);
    }
    // S6
    if (g.mode < 3) {
        double lo = quiet_nan(), hi = quiet_nan();
        for (int t = tid; t < T; t += CT_THREADS) lo = fmin(lo, x[t]);
        const double noff = block_reduce<CT_THREADS>(lo, OpFmin(), red);
        for (int t = tid; t < T; t += CT_THREADS) hi = fmax(hi, x[t] - noff);
        const double nscale = block_reduce<CT_THREADS>(hi, OpFmax(), red);
        for (int t = tid; t < T; t += CT_THREADS) x[t] = (x[t] - noff) / nscale * 0.9 + 0.05;
        offset = offset + (doff + noff) * scale;
        scale = scale * nscale;
    }
    float *out = g.out + (long)k * g.ldo;
    for (int t = tid; t < T; t += CT_THREADS) out[t] = (float)x[t];
    if (tid == 0) g.scales[k] = scale, g.offsets[k] = offset;
}

struct CtPlan {
    size_t off_x, off_y, bytes;
    unsigned lds;
};

int ct_plan(const char *fn, int K, int T, CtPlan &p) {
    DNMF_REQUIRE(K >= 1 && T >= 1, DNMF_E_SHAPE, "%s: K=%d traces, T=%d frames", fn, K, T);
    DNMF_REQUIRE(T <= CT_MAX_ELEMS && K <= CT_MAX_ELEMS, DNMF_E_UNSUPPORTED,
                 "%s: K=%d, T=%d: a trace (and the F0 of all traces) must fit %d float64 in LDS", fn, K, T, CT_MAX_ELEMS);
    const size_t arr = align256((size_t)K * T * sizeof(double));
    p.off_x = CT_HEADER, p.off_y = CT_HEADER + arr, p.bytes = CT_HEADER + 2 * arr;
    p.lds = (unsigned)(sizeof(double) * (size_t)(T > K ? T : K));
    p.lds = (p.lds + 15u) & ~15u;
    return DNMF_OK;
}

long ct_round(double v) { return (long)std::floor(v + 0.5); }   // MATLAB's round for v >= 0

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_clean_traces_workspace(int K, int T) {
    dnmf::CtPlan p;
    if (dnmf::ct_plan("dnmf_clean_traces_workspace", K, T, p) != DNMF_OK) return 0;
    return p.bytes;
}

int dnmf_clean_traces(const float *traces, long ldt, int K, int T, double fps, double sigma_threshold, int detrend_mode, int interp,
                      int smooth, int smooth_window, int trim, double floor_value, float *out, long ldo, double *scales, double *offsets,
                      double *a, double *b, double *F0, int *fitted, int *n_outliers, void *workspace, size_t workspace_bytes,
                      dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(traces && out && scales && offsets && a && b && F0 && fitted && n_outliers && workspace, DNMF_E_NULL,
                 "dnmf_clean_traces: NULL argument");
    CtPlan p;
    const int rc = ct_plan("dnmf_clean_traces", K, T, p);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldt >= T && ldo >= T, DNMF_E_SHAPE, "dnmf_clean_traces: ldt=%ld ldo=%ld below a row of T=%d", ldt, ldo, T);
    DNMF_REQUIRE(fps > 0.0 && fps <= 1.0e6, DNMF_E_SHAPE, "dnmf_clean_traces: fps=%g", fps);
    DNMF_REQUIRE(sigma_threshold >= 0.0 && std::isfinite(floor_value), DNMF_E_SHAPE, "dnmf_clean_traces: sigma_threshold=%g floor=%g",
                 sigma_threshold, floor_value);
    DNMF_REQUIRE(detrend_mode >= 0 && detrend_mode <= 3, DNMF_E_SHAPE, "dnmf_clean_traces: detrend_mode=%d", detrend_mode);
    DNMF_REQUIRE(interp == 0 || interp == 1, DNMF_E_SHAPE, "dnmf_clean_traces: interp=%d (0 none, 1 linear)", interp);
    DNMF_REQUIRE(smooth >= 0 && smooth <= 2, DNMF_E_SHAPE, "dnmf_clean_traces: smooth=%d (0 none, 1 movmean, 2 movmedian)", smooth);
    DNMF_REQUIRE(smooth == 0 || smooth_window >= 1, DNMF_E_SHAPE, "dnmf_clean_traces: smooth_window=%d", smooth_window);
    const long W = ct_round(10.0 * fps);
    DNMF_REQUIRE(detrend_mode == 0 || W >= 1, DNMF_E_SHAPE, "dnmf_clean_traces: fps=%g gives a running median over %ld frames", fps, W);
    DNMF_REQUIRE(workspace_bytes >= p.bytes, DNMF_E_WORKSPACE, "dnmf_clean_traces: workspace of %zu bytes, need %zu", workspace_bytes,
                 p.bytes);
    DNMF_REQUIRE(((size_t)workspace & 7) == 0, DNMF_E_WORKSPACE, "dnmf_clean_traces: workspace must be 8-byte aligned");
    char *w = static_cast<char *>(workspace);
    CtArgs g;
    g.in = traces, g.ldi = ldt, g.ldo = ldo, g.K = K, g.T = T;
    const long lead = ct_round(fps / 2.0);
    g.lead = (int)(lead < T ? lead : T), g.trim = trim != 0, g.mode = detrend_mode, g.W = (int)W;
    g.interp = interp, g.smooth = smooth, g.sw = smooth_window, g.floor_ = floor_value, g.sigma = sigma_threshold;
    g.out = out, g.scales = scales, g.offsets = offsets, g.a = a, g.b = b, g.F0 = F0, g.fitted = fitted, g.nout = n_outliers;
    g.hdr = reinterpret_cast<double *>(w), g.wx = reinterpret_cast<double *>(w + p.off_x), g.wy = reinterpret_cast<double *>(w + p.off_y);
    const hipStream_t st = (hipStream_t)stream;
    const void *kernels[3] = {(const void *)clean_traces_a_kernel, (const void *)clean_traces_b_kernel,
                              (const void *)clean_traces_c_kernel};
    if (p.lds > 48u * 1024u)   // beyond the default limit of dynamic LDS
        for (const void *fn : kernels) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
            if (e != hipSuccess) return fail((int)e, "dnmf_clean_traces: %u bytes of LDS: %s", p.lds, hipGetErrorString(e));
        }
    hipLaunchKernelGGL(clean_traces_a_kernel, dim3((unsigned)K), dim3(CT_THREADS), p.lds, st, g);
    if (detrend_mode == 1 || detrend_mode == 3) hipLaunchKernelGGL(clean_traces_b_kernel, dim3(1), dim3(CT_THREADS), p.lds, st, g);
    hipLaunchKernelGGL(clean_traces_c_kernel, dim3((unsigned)K), dim3(CT_THREADS), p.lds, st, g);
    return check_launch("dnmf_clean_traces");
}

}  // extern "C"
