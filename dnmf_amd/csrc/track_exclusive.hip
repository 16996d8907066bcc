// K15x: exclusive neuron tracking (tests/track_exclusive_restatement.py is the definition, in float64; everything here is fp32).
// K15's search (track_search.hpp) with the neurons already placed in the frame taken off the region as it is staged: the
// footprints are the model's own Gaussians, a_j prod_d exp(-(x_d - p^_{j,d})^2 / sigma^2) within r of the pick p*_j, so the
// frame is never changed and the rest of the search -- passes, pick, refine -- runs as in K15.
//
// One launch, one workgroup of 256 threads per frame, which walks the K R searches of its frame one after the other (round by
// round, each in the order of `order`): a search needs the results of those before it, so a frame has no more parallelism
// than one workgroup, and the call that of T workgroups.
//   placed   p^ (3 floats), p* (3 ints), a and a valid flag per neuron, in LDS beside the search's buffers; thread 0, which
//            alone holds the amplitude, writes the entry of the neuron just searched.
//   cull     wave 0 lists the placed neighbours whose +-r box meets the region (a ballot per 64 neurons, in the order of the
//            neuron index: the list, and so the order of the subtractions, does not depend on the schedule).  A neighbour that is
//            left out contributes 0 to every voxel of the region by definition: the cull is exact.
//   tables   per listed neighbour one table per axis over the region's extent along it: g1(x - p^) inside the box, 0 outside,
//            the one of the first axis times -a.  TKX_CHUNK neighbours at a time.
//   subtract as a voxel is staged: per neighbour three LDS reads, one multiply and one FMA.  Neighbours beyond the first
//            TKX_CHUNK (rare: more than 16 boxes meeting one region) are taken off the staged region in further passes.
// Per search three barriers more than K15's six (placed list, cull, tables), two more per further chunk.  No atomics, no
// scratch, no workspace; every output element is written by thread 0 of its frame's workgroup.
#include "track_search.hpp"

namespace dnmf {
namespace {

constexpr int TKX_K_MAX = 1024;     // neurons the placed list may hold (9 words of LDS each, the cull list included)
constexpr int TKX_CHUNK = 16;       // neighbours whose tables are in LDS at once

// Offsets, in words from the start of the dynamic LDS, of what follows the search's own buffers.
struct ExclusiveGeom {
    int tab;          // TKX_CHUNK tables of tl words
    int tl;           // the largest region's extents, summed over the axes
    int placed;       // 8 K words: p^ (3 K), p* (3 K), a (K), valid (K)
    int list;         // K
    int rounds;
};

struct PlacedList {
    float *ph;        // [d * K + j]
    int *ps;          // [d * K + j]
    float *a;
    int *valid;
    int K;
};

struct StageExclusive {
    PlacedList P;
    int *list, *count;      // the neighbours that meet the region, and how many
    float *tab;
    int self, r;
    float inv_s2;
    int q0, q1, q2, c0, c1, c2, tl, ncull, nb;     // the region, as begin got it; scalars: an indexed array would go to scratch

    // the tables of the neighbours list[first], ..., at most TKX_CHUNK of them
    __device__ __forceinline__ void build(int first, int tid) {
        nb = min(TKX_CHUNK, ncull - first);
        for (int i = tid; i < nb * tl; i += TK_THREADS) {
            const int n = i / tl, off = i - n * tl;
            const int d = off < c0 ? 0 : (off < c0 + c1 ? 1 : 2);
            const int l = off - pick3(d, 0, c0, c0 + c1);
            const int j = list[first + n];
            const int x = pick3(d, q0, q1, q2) + l;
            const float t = (float)x - P.ph[d * P.K + j];
            float v = abs(x - P.ps[d * P.K + j]) <= r ? expf(-(t * t) * inv_s2) : 0.0f;
            if (d == 0) v *= -P.a[j];
            tab[i] = v;
        }
    }

    __device__ __forceinline__ void begin(int q0_, int q1_, int q2_, int c0_, int c1_, int c2_, int tid) {
        q0 = q0_, q1 = q1_, q2 = q2_, c0 = c0_, c1 = c1_, c2 = c2_;
        tl = c0 + c1 + c2;
        const int lane = tid & 63;
        __syncthreads();        // the entry thread 0 wrote after the search before; that search's reads of list and tab
        if (tid < 64) {
            int cnt = 0;
            for (int base = 0; base < P.K; base += 64) {
                const int j = base + lane;
                bool hit = j < P.K && j != self && P.valid[j] != 0;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int p = hit ? P.ps[d * P.K + j] : 0;
                    hit = hit && p + r >= pick3(d, q0, q1, q2) && p - r <= pick3(d, q0 + c0, q1 + c1, q2 + c2) - 1;
                }
                const unsigned long long m = __ballot(hit);
                if (hit) list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = j;
                cnt += __popcll(m);
            }
            if (lane == 0) *count = cnt;
        }
        __syncthreads();
        ncull = *count;
        build(0, tid);
        __syncthreads();
    }

    __device__ __forceinline__ float operator()(float v, int l0, int l1, int l2) const {
        const float *t = tab;
        for (int n = 0; n < nb; ++n, t += tl) v = fmaf(t[l0] * t[c0 + l1], t[c0 + c1 + l2], v);
        return v;
    }

    __device__ __forceinline__ void finish(float *buf, int tid) {
        const int nin = c0 * c1 * c2;
        for (int first = TKX_CHUNK; first < ncull; first += TKX_CHUNK) {      // ncull is the same in every thread
            __syncthreads();    // every thread is done with the tables of the chunk before
            build(first, tid);
            __syncthreads();
            for (int e = tid; e < nin; e += TK_THREADS) {
                const int l2 = e % c2, l1 = (e / c2) % c1, l0 = e / (c2 * c1);
                buf[e] = (*this)(buf[e], l0, l1, l2);
            }
        }
    }
};

// predict (K,3,T) or (K,3); order (K,T); positions (K,3,T) fp64, amplitudes / peaks / n_subtracted (K,T) or NULL.
template <typename TP>
__global__ __launch_bounds__(TK_THREADS) void track_exclusive_kernel(const float *__restrict__ frames, long ldf, TrackGeom g, ExclusiveGeom x,
                                                                     int T, const int *__restrict__ times, const TP *__restrict__ predict,
                                                                     int per_frame, int K, const int *__restrict__ order,
                                                                     const float *__restrict__ background, double *__restrict__ positions,
                                                                     float *__restrict__ amplitudes, float *__restrict__ peaks,
                                                                     int *__restrict__ n_subtracted) {
    extern __shared__ float lds[];
    __shared__ float s_wv[TK_WAVES];
    __shared__ int s_wi[TK_WAVES];
    __shared__ float s_e2[3];
    __shared__ int s_count;
    const TrackLds L = {lds, lds + g.rpad, lds + 2 * g.rpad, lds + 2 * g.rpad + g.nA, s_wv, s_wi, s_e2};
    float *pl = lds + x.placed;
    const PlacedList P = {pl, reinterpret_cast<int *>(pl + 3 * K), pl + 6 * K, reinterpret_cast<int *>(pl + 7 * K), K};
    StageExclusive stage;
    stage.P = P, stage.list = reinterpret_cast<int *>(lds + x.list), stage.count = &s_count, stage.tab = lds + x.tab;
    stage.r = g.r, stage.inv_s2 = g.inv_s2;
    const int tid = threadIdx.x;
    const int j = (int)blockIdx.x;
    const float *fr = frames + (long)(times ? times[j] : j) * ldf;
    const float bg = background ? background[j] : 0.0f;
    for (int i = tid; i < K; i += TK_THREADS) P.valid[i] = 0;
    fill_taps(L.tap, L.c2, g.r, g.inv_s2, tid, TK_THREADS);
    __syncthreads();
    // everything the loops branch on is the same in every thread
    for (int round = 0; round < x.rounds; ++round) {
        for (int i = 0; i < K; ++i) {
            const int k = order[(long)i * T + j];
            if ((unsigned)k >= (unsigned)K) continue;      // not a neuron: the caller's order is no permutation
            const long pin = per_frame ? (long)k * 3 * T + j : (long)k * 3;
            const long pst = per_frame ? T : 1;
            float phat[3] = {0.0f, 0.0f, 0.0f}, amp = 0.0f, peak = 0.0f;
            int pick[3] = {0, 0, 0};
            stage.self = k, stage.ncull = 0;
            const bool found = track_search_staged(fr, bg, g, (double)predict[pin], (double)predict[pin + pst], (double)predict[pin + 2 * pst],
                                                   L, tid, phat, amp, peak, pick, stage);
            if (tid == 0) {
                // no other thread reads the list between the tables of this search and the first barrier of the next
                P.valid[k] = found ? 1 : 0;
                if (found) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) P.ph[d * K + k] = phat[d], P.ps[d * K + k] = pick[d];
                    P.a[k] = amp;
                }
                if (round == x.rounds - 1) {
                    const long out = (long)k * T + j;
#pragma unroll
                    for (int d = 0; d < 3; ++d) positions[((long)k * 3 + d) * T + j] = found ? (double)phat[d] : __builtin_nan("");
                    if (amplitudes) amplitudes[out] = found ? amp : __builtin_nanf("");
                    if (peaks) peaks[out] = found ? peak : __builtin_nanf("");
                    if (n_subtracted) n_subtracted[out] = stage.ncull;
                }
            }
        }
    }
}

// 0 ok, else the error already recorded: K15's checks, then what the placed list and the tables add to its LDS.
inline int track_exclusive_geometry(const char *fn, const int *sz, int T, int K, double sigma, const int *search, int rounds, double threshold,
                                    long ldf, TrackGeom &g, ExclusiveGeom &x, size_t &lds) {
    DNMF_REQUIRE(rounds >= 1, DNMF_E_SHAPE, "%s: rounds=%d must be at least 1", fn, rounds);
    DNMF_REQUIRE(K <= TKX_K_MAX, DNMF_E_UNSUPPORTED, "%s: K=%d: the placed list holds at most %d neurons", fn, K, TKX_K_MAX);
    const int rc = track_geometry(fn, sz, T, K, sigma, search, threshold, ldf, g, lds);
    if (rc != DNMF_OK) return rc;
    long tl = 0;
    for (int d = 0; d < 3; ++d) tl += 2L * ((long)search[d] + 1 + g.r) + 1 < sz[d] ? 2L * ((long)search[d] + 1 + g.r) + 1 : sz[d];
    const size_t words = lds / sizeof(float) + (size_t)TKX_CHUNK * tl + 9 * (size_t)K;
    DNMF_REQUIRE(words * sizeof(float) <= TK_LDS_BUDGET, DNMF_E_UNSUPPORTED,
                 "%s: sigma=%g, search (%d, %d, %d), K=%d: the region (%zu bytes), %d neighbour tables of %ld words and the placed list "
                 "of %d neurons need %zu bytes, more than the %zu bytes of LDS a workgroup may take",
                 fn, sigma, search[0], search[1], search[2], K, lds, TKX_CHUNK, tl, K, words * sizeof(float), TK_LDS_BUDGET);
    x.tab = (int)(lds / sizeof(float));
    x.tl = (int)tl;
    x.placed = x.tab + TKX_CHUNK * (int)tl;
    x.list = x.placed + 8 * K;
    x.rounds = rounds;
    lds = words * sizeof(float);
    return DNMF_OK;
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_track_neurons_exclusive(const float *frames, long ldf, const int *sz, int T, const int *times, const void *predict, int predict_f64,
                                 int predict_per_frame, int K, const int *order, int rounds, double sigma, const int *search,
                                 double threshold, const float *background, double *positions, float *amplitudes, float *peaks,
                                 int *n_subtracted, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames, DNMF_E_NULL, "dnmf_track_neurons_exclusive: NULL frames");
    DNMF_REQUIRE(sz, DNMF_E_NULL, "dnmf_track_neurons_exclusive: NULL sz");
    DNMF_REQUIRE(predict, DNMF_E_NULL, "dnmf_track_neurons_exclusive: NULL predict");
    DNMF_REQUIRE(order, DNMF_E_NULL, "dnmf_track_neurons_exclusive: NULL order");
    DNMF_REQUIRE(search, DNMF_E_NULL, "dnmf_track_neurons_exclusive: NULL search");
    DNMF_REQUIRE(positions, DNMF_E_NULL, "dnmf_track_neurons_exclusive: NULL positions");
    TrackGeom g;
    ExclusiveGeom x;
    size_t lds = 0;
    const int rc = track_exclusive_geometry("dnmf_track_neurons_exclusive", sz, T, K, sigma, search, rounds, threshold, ldf, g, x, lds);
    if (rc != DNMF_OK) return rc;
    const dim3 grid((unsigned)T);
    const hipStream_t st = (hipStream_t)stream;
    if (predict_f64)
        hipLaunchKernelGGL(track_exclusive_kernel<double>, grid, dim3(TK_THREADS), lds, st, frames, ldf, g, x, T, times,
                           static_cast<const double *>(predict), predict_per_frame, K, order, background, positions, amplitudes, peaks,
                           n_subtracted);
    else
        hipLaunchKernelGGL(track_exclusive_kernel<float>, grid, dim3(TK_THREADS), lds, st, frames, ldf, g, x, T, times,
                           static_cast<const float *>(predict), predict_per_frame, K, order, background, positions, amplitudes, peaks,
                           n_subtracted);
    return check_launch("dnmf_track_neurons_exclusive");
}

}  // extern "C"
