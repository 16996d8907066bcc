// K32: the AR(1)-constrained trace update -- one row step of block coordinate descent per listed neuron.  include/dnmf_hip.h has
// the contract, tests/ar1_restatement.py the definition in float64.
//
// One launch is one colour of the overlap graph: the listed neurons share no Gram entry, so their row steps are independent.  One
// workgroup of AR_THREADS lanes per listed neuron k, everything in float64:
//   1  frame t = tid, tid + AR_THREADS, ..: the weight w_t = G_t[k,k] and the target y_t = C[k,t] + (r_t[k] - sum_l G_t[k,l] C[l,t]) / w_t,
//      the sum over the listed columns in their order (all columns without a list), one product and one addition a term.  A frame
//      whose w_t is not finite or <= 0, or whose y_t is not finite, carries no weight.  The pool record of the frame is written
//      straight from them: num = w_t (y_t - b) - lam mu_t, den = w_t (0 without weight), mu_t = 1 - g, 1 on the last frame;
//   2  the local pools of every lane's frames, the stitch, the expansion: ar1_pools.hpp's solver (that header explains the
//      scheme), which K21 (deconvolve_traces.hip) uses with den = 1 where this kernel has w_t;
//   3  row k of the state becomes b + c, the row of s the spikes.
// g = 0 is the plain coordinate step max(0, y_t - b - lam / w_t) + b, a branch of its own (block-uniform) that never forms log 0.
// The records live in LDS: T <= POOL_LDS_FRAMES.  No floating-point atomics, no scratch, counts are integers: the same input gives
// the same bits.
#include <cmath>
#include <cstdint>

#include "ar1_pools.hpp"

namespace dnmf {
namespace {

constexpr int AR_THREADS = 1024;
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

    const Pools P = pools_over<AR_THREADS>(dyn, T, plain ? 0.0 : log(g));
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

    // ---- 2, 3: the local pools (the records are complete), the stitch, the expansion into the rows
    pools_stitch<AR_THREADS>(P, pools_local(P, [](int) {}), s_top);
    int pools = pools_expand<AR_THREADS>(P, g, s_last, [&](int t, double c, double s) { crow[t] = b + c, srow[t] = s; });
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
    DNMF_REQUIRE(T <= POOL_LDS_FRAMES && K <= AR_MAX_K, DNMF_E_UNSUPPORTED,
                 "dnmf_ar1_temporal_step: K=%d, T=%d: at most %d neurons and %d frames (a row's pool records must fit LDS)", K, T,
                 AR_MAX_K, POOL_LDS_FRAMES);
    ArArgs a;
    a.G = G, a.r = r, a.C = C, a.ldc = ldc, a.lds = lds, a.K = K, a.T = T, a.n_ids = n_ids, a.NN = nbr ? NN : 0;
    a.ids = ids, a.nbr = nbr, a.g = g, a.penalty = penalty, a.baseline = baseline, a.s = s, a.counts = counts;
    const unsigned lds_bytes = ((unsigned)T * POOL_RECORD + 15u) & ~15u;
    const int rl = allow_dynamic_lds("dnmf_ar1_temporal_step", (const void *)ar1_temporal_kernel, lds_bytes);
    if (rl != DNMF_OK) return rl;
    hipLaunchKernelGGL(ar1_temporal_kernel, dim3((unsigned)n_ids), dim3(AR_THREADS), lds_bytes, (hipStream_t)stream, a);
    return check_launch("dnmf_ar1_temporal_step");
}

}  // extern "C"
