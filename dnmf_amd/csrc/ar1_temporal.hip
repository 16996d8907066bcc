// K32: the AR(1)-constrained trace update -- one row step of block coordinate descent per listed neuron.  include/dnmf_hip.h has
// the contract, tests/ar1_restatement.py the definition in float64.
//
// One launch is one colour of the overlap graph: the listed neurons share no Gram entry, so their row steps are independent.  One
// workgroup of AR_THREADS lanes per listed neuron k, everything in float64:
//   1  frame t = tid, tid + AR_THREADS, ..: the weight w_t = G_t[k,k] and the target y_t = C[k,t] + (r_t[k] - sum_l G_t[k,l] C[l,t]) / w_t,
//      the sum over the listed columns in their order (all columns without a list), one product and one addition a term.  A frame
//      whose w_t is not finite or <= 0, or whose y_t is not finite, carries no weight.  The pool record of the frame is written
//      straight from them: num = w_t (y_t - b) - lam mu_t, den = w_t (0 without weight), mu_t = 1 - g, 1 on the last frame;
//   2  lane i runs pool-adjacent-violators on its own `per` contiguous frames, then the stitch in log2(AR_THREADS) levels, then every
//      lane expands the pools over its frames -- K21's scheme (deconvolve_traces.hip, whose comment explains it) with den = w_t
//      where K21 has 1.  The device functions below restate K21's: that kernel stays as it is, bit for bit;
//   3  row k of the state becomes b + c, the row of s the spikes.
// g = 0 is the plain coordinate step max(0, y_t - b - lam / w_t) + b, a branch of its own (block-uniform) that never forms log 0.
// The records take 24 bytes a frame and live in LDS: T <= AR_LDS_FRAMES.  No floating-point atomics, no scratch, counts are
// integers: the same input gives the same bits.
#include <cmath>
#include <cstdint>

#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int AR_THREADS = 1024;
constexpr int AR_STATIC_LDS = 16 * 1024;                           // bytes set aside for the static arrays below (they take 8.2 KiB)
constexpr int AR_RECORD = 24;                                      // bytes of a pool record: num, den (double), len, prev (int)
constexpr int AR_LDS_FRAMES = (160 * 1024 - AR_STATIC_LDS) / AR_RECORD;   // 6144
constexpr int AR_MAX_K = 4096;

struct ArArgs {
    const float *G, *r;
    double *C;
    long ldc, lds;
    int K, T, n_ids, NN;
    const int *ids, *nbr;
    const double *g, *penalty, *baseline;
    double *s;
    int *counts;   // (K, 2): pools, weightless frames of row k
};

struct ArPools {
    double *num, *den;
    int *len, *prev;
    double lng;
};

__device__ __forceinline__ bool violates(const ArPools &P, int p, int q) {
    const double dp = P.den[p];
    if (!(dp > 0.0)) return false;   // only a leading run of weightless frames: never merged into
    const double dq = P.den[q];
    if (!(dq > 0.0)) return true;    // weightless frames merge backwards
    return P.num[q] / dq < (P.num[p] / dp) * exp((double)P.len[p] * P.lng);
}

__device__ __forceinline__ void merge(const ArPools &P, int p, int q) {
    const double gl = exp((double)P.len[p] * P.lng);
    P.num[p] = P.num[p] + gl * P.num[q];
    P.den[p] = P.den[p] + gl * gl * P.den[q];
    P.len[p] = P.len[p] + P.len[q];
    P.len[q] = 0;
}

// merge p backwards while it violates -> the pool it ends up in
__device__ __forceinline__ int settle(const ArPools &P, int p) {
    for (;;) {
        const int pp = P.prev[p];
        if (pp < 0 || !violates(P, pp, p)) return p;
        merge(P, pp, p);
        p = pp;
    }
}

__global__ __launch_bounds__(AR_THREADS) void ar1_temporal_kernel(ArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ int red[AR_THREADS / 64];
    __shared__ int s_top[AR_THREADS], s_last[AR_THREADS];
    const int tid = threadIdx.x, T = a.T, K = a.K;
    const int k = a.ids[blockIdx.x];
    if ((unsigned)k >= (unsigned)K) return;   // block-uniform; the wrapper lets no such id through
    const double g = a.g[k], lam = a.penalty[k], b = a.baseline[k];
    double *crow = a.C + (long)k * a.ldc, *srow = a.s + (long)k * a.lds;
    const int *list = a.nbr ? a.nbr + (long)k * a.NN : nullptr;
    const int nl = a.nbr ? a.NN : K;
    const bool plain = !(g > 0.0);

    ArPools P;
    P.num = dyn, P.den = dyn + T;
    P.len = reinterpret_cast<int *>(dyn + 2 * (size_t)T), P.prev = P.len + T;
    P.lng = plain ? 0.0 : log(g);
    const double mu = 1.0 - g;

    // ---- 1: weights, targets, records
    int weightless = 0;
    for (int t = tid; t < T; t += AR_THREADS) {
        const float *Gk = a.G + ((long)t * K + k) * K;
        const double w = (double)Gk[k];
        double acc = 0.0;
        for (int j = 0; j < nl; ++j) {
            const int l = list ? list[j] : j;
            if ((unsigned)l < (unsigned)K) acc = acc + (double)Gk[l] * a.C[(long)l * a.ldc + t];
        }
        const double y = crow[t] + ((double)a.r[(long)t * K + k] - acc) / w;
        const bool ok = isfinite(w) && w > 0.0 && isfinite(y);
        weightless += ok ? 0 : 1;
        if (plain) {
            const double x = ok ? fmax(0.0, (y - b) - lam / w) : 0.0;
            crow[t] = x + b, srow[t] = x;
        } else {
            P.num[t] = (ok ? w * (y - b) : 0.0) - lam * (t < T - 1 ? mu : 1.0);
            P.den[t] = ok ? w : 0.0;
        }
    }
    weightless = block_reduce<AR_THREADS>(weightless, OpSum(), red);   // ends with a barrier: the records are complete
    if (plain) {
        if (tid == 0) a.counts[2 * k] = T, a.counts[2 * k + 1] = weightless;
        return;
    }

    // ---- 2: PAVA on the lane's own frames, the stitch, the expansion
    const int per = (T + AR_THREADS - 1) / AR_THREADS;
    const int c0 = (int)min((long)T, (long)tid * per), c1 = min(T, c0 + per);
    int top = -1;
    for (int t = c0; t < c1; ++t) {
        P.len[t] = 1, P.prev[t] = top;
        top = settle(P, t);
    }
    s_top[tid] = top;
    __syncthreads();
    // block [tid, tid + s) of segments takes in block [tid + s, tid + 2 s)
    for (int s = 1; s < AR_THREADS; s <<= 1) {
        if ((tid & (2 * s - 1)) == 0) {
            const long first = (long)(tid + s) * per;
            if (first < T) {
                const int end = (int)min((long)T, (long)(tid + 2 * s) * per);
                int p = s_top[tid], q = (int)first;
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
                s_top[tid] = q >= end ? p : s_top[tid + s];
            }
        }
        __syncthreads();
    }
    // the last pool start at or before the end of every lane's frames
    int last = -1;
    for (int t = c0; t < c1; ++t)
        if (P.len[t] > 0) last = t;
    s_last[tid] = last;
    __syncthreads();
    int pools = 0;
    if (c0 < c1) {
        int cur = -1;                                   // the pool that covers frame c0 - 1
        for (int l = tid - 1; l >= 0 && cur < 0; --l) cur = s_last[l];
        double cv = 0.0, cprev = 0.0;                   // the pool's max(v, 0); c of the frame before
        if (cur >= 0) {
            const double d = P.den[cur];
            cv = d > 0.0 ? fmax(P.num[cur] / d, 0.0) : 0.0;
            cprev = cv * exp((double)(c0 - 1 - cur) * P.lng);
        }
        for (int t = c0; t < c1; ++t) {
            double c, s = 0.0;
            if (P.len[t] > 0) {
                cur = t, ++pools;
                const double d = P.den[t];
                cv = d > 0.0 ? fmax(P.num[t] / d, 0.0) : 0.0;
                c = cv;
                s = t == 0 ? c : fmax(c - g * cprev, 0.0);
            } else {
                c = cv * exp((double)(t - cur) * P.lng);
            }
            cprev = c;
            crow[t] = b + c, srow[t] = s;
        }
    }
    pools = block_reduce<AR_THREADS>(pools, OpSum(), red);
    if (tid == 0) a.counts[2 * k] = pools, a.counts[2 * k + 1] = weightless;
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_ar1_temporal_step(const float *G, const float *r, double *C, long ldc, int K, int T, const int *ids, int n_ids,
                           const double *g, const double *penalty, const double *baseline, const int *nbr, int NN, double *s,
                           long lds, int *counts, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(G && r && C && ids && g && penalty && baseline && s && counts, DNMF_E_NULL, "dnmf_ar1_temporal_step: NULL argument");
    DNMF_REQUIRE(K >= 1 && T >= 1 && ldc >= T && lds >= T && n_ids >= 1 && n_ids <= K && (!nbr || NN >= 1), DNMF_E_SHAPE,
                 "dnmf_ar1_temporal_step: K=%d T=%d ldc=%ld lds=%ld n_ids=%d NN=%d", K, T, ldc, lds, n_ids, NN);
    DNMF_REQUIRE(T <= AR_LDS_FRAMES && K <= AR_MAX_K, DNMF_E_UNSUPPORTED,
                 "dnmf_ar1_temporal_step: K=%d, T=%d: at most %d neurons and %d frames (a row's pool records must fit LDS)", K, T,
                 AR_MAX_K, AR_LDS_FRAMES);
    ArArgs a;
    a.G = G, a.r = r, a.C = C, a.ldc = ldc, a.lds = lds, a.K = K, a.T = T, a.n_ids = n_ids, a.NN = nbr ? NN : 0;
    a.ids = ids, a.nbr = nbr, a.g = g, a.penalty = penalty, a.baseline = baseline, a.s = s, a.counts = counts;
    const unsigned lds_bytes = ((unsigned)T * AR_RECORD + 15u) & ~15u;
    if (lds_bytes > 48u * 1024u) {   // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void *)ar1_temporal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes);
        if (e != hipSuccess) return fail((int)e, "dnmf_ar1_temporal_step: %u bytes of LDS: %s", lds_bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(ar1_temporal_kernel, dim3((unsigned)n_ids), dim3(AR_THREADS), lds_bytes, (hipStream_t)stream, a);
    return check_launch("dnmf_ar1_temporal_step");
}

}  // extern "C"
