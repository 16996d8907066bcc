// K4h -- exact non-negative least-squares read-out of the traces (HALS / cyclic coordinate descent) on the hoisted
// Gram data, beside the multiplicative update K4 (mu_temporal.hip).
//
// Per call, over the frames t of the call,
//   F(C) = sum_t ( 1/2 c_t^T G_t c_t - r_t^T c_t ) + gamma/2 sum_{t<T-1} |c_{t+1} - c_t|^2 ,  C >= 0
// (the function whose gradient K4 splits).  One coordinate update of (k,t), n_t = real neighbours of frame t:
//   d = G_t[k,k] + gamma n_t ;  c_k <- d > 0 ? max(0, (r_t[k] - sum_{l != k} G_t[k,l] c_l + gamma (c_{k,t-1} + c_{k,t+1})) / d) : 0
// A sweep visits k = 0 .. K-1 ascending in every frame; with gamma != 0 the even frames first, then the odd ones
// (red-black in t: frames of one colour do not see each other, so a half sweep is one launch).
//
// The update is sequential in k, so the parallelism is across frames: ONE WAVE PER FRAME, up to four frames per
// workgroup, and no workgroup barrier anywhere (a wave only orders its own LDS traffic).  The wave keeps the gradient
// g = G c - r + gamma (n_t c - neighbours) and c in LDS, in fp64.  In residual form the update above is
//   c_k^new = max(0, c_k - g_k / d) ,   delta = c_k^new - c_k ,   g += delta * (G[:,k] + gamma n_t e_k)
// which differs from the direct formula in fp64 rounding only; a coordinate that does not move (delta == 0: every
// clamped neuron at convergence) costs two LDS reads.  G[:,k] is row k (G is symmetric):
//   NN == 0 (dense):  K/64 entries per lane straight from global memory, the next row in flight while this one is used;
//   NN in {8,16,32}:  the NN listed entries of every row staged in LDS once (from a dense G or from the K3n slot tables),
//                     NN lanes each touching one entry of g.
#include "trace_calls.hpp"

namespace dnmf {

// orders the LDS traffic of the lanes of one wave (the hardware executes a wave's LDS instructions in order; this keeps
// the compiler from moving them across and makes the wave's writes visible to its other lanes)
__device__ __forceinline__ void hals_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes of LDS one wave (one frame) needs: g, c, d as K doubles each, then K rows of NN + 1 floats (odd stride: the lanes
// that walk down a column of the staged rows hit different banks)
inline size_t hals_wave_bytes(int K, int NN) {
    const size_t rowf = NN ? (((size_t)K * (NN + 1) + 1) & ~(size_t)1) : 0;
    return 3 * (size_t)K * sizeof(double) + rowf * sizeof(float);
}

// src: G (T,K,K) dense, or (SLOTS) the slot tables of K3n, (T, nchunks, nslot) floats.
// C32 (gamma == 0: fp32 state, rounded once at the end) or C64 (fp64 state, in place); exactly one is non-NULL.
// parity < 0: wave f works on frame f; else on frame 2 f + parity.  iters == 0: nothing is written but kkt.
template <int NN, bool SLOTS>
__global__ __launch_bounds__(256) void hals_temporal_kernel(const float *__restrict__ src, const float *__restrict__ r,
                                                            int nchunks, int nslot, const int *__restrict__ pair_slot,
                                                            const int *__restrict__ nbr, float *C32, double *C64, long ldc,
                                                            int K, int T, int nframes, int iters, double gamma, int parity,
                                                            double *__restrict__ kkt, unsigned wave_bytes) {
    extern __shared__ double hals_lds[];
    constexpr int RS = NN + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * (blockDim.x >> 6) + wave;
    if (f >= nframes) return;   // partial last workgroup; no workgroup barrier below
    const int t = parity < 0 ? f : 2 * f + parity;
    double *g = (double *)((char *)hals_lds + (size_t)wave * wave_bytes);
    double *c = g + K, *dd = c + K;
    float *rows = (float *)(dd + K);
    (void)rows;

    const float *Gt = src + (SLOTS ? (long)t * nchunks * nslot : (long)t * K * K);
    auto slot_sum = [&](int slot) { return slot_chunk_sum(Gt, nchunks, nslot, slot); };   // as gram_lists_finish_kernel sums
    auto column = [&](int k, int j) {   // the j-th listed column of row k; -1 for an entry outside [0,K), which then
        const int l = nbr[k * NN + j];  // contributes nothing anywhere (the contract wants none: no read out of bounds)
        return (unsigned)l < (unsigned)K ? l : -1;
    };
    const bool left = gamma != 0.0 && t > 0, right = gamma != 0.0 && t + 1 < T;
    const double gn = gamma * (double)((left ? 1 : 0) + (right ? 1 : 0));

    // ---- stage the state, the diagonal and (lists) the rows ----
    for (int k = lane; k < K; k += 64) {
        c[k] = C64 ? C64[(long)k * ldc + t] : (double)C32[(long)k * ldc + t];
        const float gkk = SLOTS ? slot_sum(pair_slot[(long)k * K + k]) : Gt[(long)k * K + k];
        dd[k] = (double)gkk + gn;
    }
    if constexpr (NN > 0) {
        for (int e = lane; e < K * NN; e += 64) {
            const int k = e / NN, j = e % NN;
            const int l = column(k, j);
            rows[k * RS + j] = l < 0 ? 0.0f : (SLOTS ? slot_sum(pair_slot[(long)l * K + k]) : Gt[(long)k * K + l]);
        }
    }
    hals_wave_sync();
    // ---- g = G c - r + gamma (n_t c - neighbours) ----
    for (int k = lane; k < K; k += 64) {
        double dot = 0.0;
        if constexpr (NN > 0) {
            for (int j = 0; j < NN; ++j) {
                const int l = column(k, j);
                if (l >= 0) dot = fma((double)rows[k * RS + j], c[l], dot);
            }
        } else {
            for (int l = 0; l < K; ++l) dot = fma((double)Gt[(long)l * K + k], c[l], dot);
        }
        const double rk = SLOTS ? (double)slot_sum(k) : (double)r[(long)t * K + k];
        double nb = 0.0;
        if (left) nb += C64[(long)k * ldc + t - 1];
        if (right) nb += C64[(long)k * ldc + t + 1];
        g[k] = (dot - rk) + (gn * c[k] - gamma * nb);
    }
    hals_wave_sync();

    // ---- the sweeps ----
    for (int it = 0; it < iters; ++it) {
        if constexpr (NN > 0) {
            int lnext = lane < NN ? column(0, lane) : -1;
            for (int k = 0; k < K; ++k) {
                const int l = lnext;
                if (k + 1 < K) lnext = lane < NN ? column(k + 1, lane) : -1;
                const double ck = c[k], d = dd[k];
                const double cn = d > 0.0 ? fmax(0.0, ck - g[k] / d) : 0.0;
                const double delta = cn - ck;
                if (delta != 0.0) {   // wave-uniform
                    const bool diag = l == k;
                    const bool listed = __ballot(diag) != 0ull;
                    if (l >= 0) g[l] = fma(delta, diag ? d : (double)rows[k * RS + lane], g[l]);
                    if (lane == NN) {   // an idle lane: NN < 64
                        c[k] = cn;
                        if (!listed) g[k] = fma(delta, d, g[k]);   // row k does not list itself (an empty footprint)
                    }
                    hals_wave_sync();
                }
            }
        } else {
            float cur[4], nxt[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) nxt[i] = lane + 64 * i < K ? Gt[lane + 64 * i] : 0.0f;
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
                if (k + 1 < K) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) nxt[i] = lane + 64 * i < K ? Gt[(long)(k + 1) * K + lane + 64 * i] : 0.0f;
                }
                const double ck = c[k], d = dd[k];
                const double cn = d > 0.0 ? fmax(0.0, ck - g[k] / d) : 0.0;
                const double delta = cn - ck;
                if (delta != 0.0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int l = lane + 64 * i;
                        if (l < K) g[l] = fma(delta, l == k ? d : (double)cur[i], g[l]);
                    }
                    if (lane == 0) c[k] = cn;
                    hals_wave_sync();
                }
            }
        }
    }

    // ---- results ----
    if (kkt) {
        double m = 0.0;
        for (int k = lane; k < K; k += 64) {
            const double pg = c[k] > 0.0 ? g[k] : fmin(g[k], 0.0);
            m = fmax(m, fabs(pg));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
        if (lane == 0) kkt[t] = m;
    }
    if (iters > 0) {
        for (int k = lane; k < K; k += 64) {
            if (C64)
                C64[(long)k * ldc + t] = c[k];
            else
                C32[(long)k * ldc + t] = (float)c[k];
        }
    }
}

// one launch: all frames (parity < 0) or the frames of one colour
static int hals_launch(const char *what, bool slots, const float *src, const float *r, int nchunks, int nslot,
                       const int *pair_slot, const int *nbr, int NN, float *C32, double *C64, long ldc, int K, int T,
                       int iters, double gamma, int parity, double *kkt, hipStream_t st) {
    const int nframes = parity < 0 ? T : (T - parity + 1) / 2;
    if (nframes <= 0 || (iters == 0 && !kkt)) return DNMF_OK;
    const size_t wb = hals_wave_bytes(K, NN);
    const int wpb = (int)(wb * 4 <= 61440 ? 4 : (wb * 2 <= 61440 ? 2 : 1));   // <= 60 KiB of LDS per workgroup
    const dim3 grid((unsigned)((nframes + wpb - 1) / wpb)), block(64 * wpb);
    const size_t lds = wb * wpb;
    auto launch = [&](auto nn, auto sl) {
        hipLaunchKernelGGL((hals_temporal_kernel<decltype(nn)::value, decltype(sl)::value>), grid, block, lds, st, src, r, nchunks,
                           nslot, pair_slot, nbr, C32, C64, ldc, K, T, nframes, iters, gamma, parity, kkt, (unsigned)wb);
    };
    if (slots) with_list_width<false>(NN, [&](auto nn) { launch(nn, std::true_type{}); });
    else with_list_width<true>(NN, [&](auto nn) { launch(nn, std::false_type{}); });
    return check_launch(what);
}

}  // namespace dnmf

extern "C" {

int dnmf_hals_temporal(const float *G, const float *r, float *C, long ldc, int K, int T, int iters, const int *nbr, int NN,
                       double *kkt, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(G && r && C, DNMF_E_NULL, "dnmf_hals_temporal: NULL buffer");
    if (!nbr) NN = 0;
    const int rc = check_trace_call("dnmf_hals_temporal", K, T, ldc, LISTS_OR_DENSE, NN, iters >= 0, " iters=%d", iters);
    if (rc != DNMF_OK) return rc;
    return hals_launch("dnmf_hals_temporal", false, G, r, 0, 0, nullptr, nbr, NN, C, nullptr, ldc, K, T, iters, 0.0, -1, kkt,
                       (hipStream_t)stream);
}

int dnmf_hals_temporal_slots(const float *slab, int nchunks, int nslot, const int *pair_slot, float *C, long ldc, int K,
                             int T, int iters, const int *nbr, int NN, double *kkt, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(slab && pair_slot && C && nbr, DNMF_E_NULL, "dnmf_hals_temporal_slots: NULL buffer");
    const int rc = check_trace_call("dnmf_hals_temporal_slots", K, T, ldc, LISTS_ONLY, NN, iters >= 0 && nchunks > 0 && nslot > K,
                                    " iters=%d nchunks=%d nslot=%d", iters, nchunks, nslot);
    if (rc != DNMF_OK) return rc;
    return hals_launch("dnmf_hals_temporal_slots", true, slab, nullptr, nchunks, nslot, pair_slot, nbr, NN, C, nullptr, ldc, K,
                       T, iters, 0.0, -1, kkt, (hipStream_t)stream);
}

int dnmf_hals_temporal_step(const float *G, const float *r, double *C, long ldc, int K, int T, double gamma, int parity,
                            const int *nbr, int NN, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(G && r && C, DNMF_E_NULL, "dnmf_hals_temporal_step: NULL buffer");
    if (!nbr) NN = 0;
    const int rc = check_trace_call("dnmf_hals_temporal_step", K, T, ldc, LISTS_OR_DENSE, NN, parity == 0 || parity == 1,
                                    " parity=%d (0 or 1)", parity);
    if (rc != DNMF_OK) return rc;
    return hals_launch("dnmf_hals_temporal_step", false, G, r, 0, 0, nullptr, nbr, NN, nullptr, C, ldc, K, T, 1, gamma, parity,
                       nullptr, (hipStream_t)stream);
}

int dnmf_hals_temporal_kkt(const float *G, const float *r, const double *C, long ldc, int K, int T, double gamma,
                           const int *nbr, int NN, double *kkt, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(G && r && C && kkt, DNMF_E_NULL, "dnmf_hals_temporal_kkt: NULL buffer");
    if (!nbr) NN = 0;
    const int rc = check_trace_call("dnmf_hals_temporal_kkt", K, T, ldc, LISTS_OR_DENSE, NN, true, "");
    if (rc != DNMF_OK) return rc;
    // iters == 0: the kernel reads C and writes kkt only
    return hals_launch("dnmf_hals_temporal_kkt", false, G, r, 0, 0, nullptr, nbr, NN, nullptr, const_cast<double *>(C), ldc, K,
                       T, 0, gamma, -1, kkt, (hipStream_t)stream);
}

}  // extern "C"
