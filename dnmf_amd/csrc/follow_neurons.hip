// K15c: chained neuron tracking (tests/follow_restatement.py is the definition, in float64).  K15's search (track_search.hpp)
// unchanged, run frame after frame: each neuron is carried from the anchor frame to the last frame by one chain and to the
// first frame by another, every search around the position the chain predicts from what it found before.
//
// One launch, one workgroup of 256 threads per (neuron, direction): 2 K workgroups, each of which walks its frames one after
// the other -- the T steps of a chain are sequential by definition, so the launch has the parallelism of 2 K workgroups and no
// more.  The state of a chain (last position, velocity, frames since the last result, misses) lives in registers and is the
// same in every thread: it is made from the result of track_search, which every thread holds, so every barrier and the exit of
// the loop are reached by the whole workgroup.  The recurrence is float64, every operation rounded once (no contraction), on
// the positions as they are stored -- fp32 widened -- so the host can repeat it bit for bit from the outputs.  Every (k, j)
// of every output is written by exactly one workgroup (the backward chain repeats the anchor search and leaves the anchor
// frame's row to the forward chain): no atomics, no initialisation, no workspace.  There is still no exclusion between
// neurons: two chains may follow the same blob.
#include "track_search.hpp"

namespace dnmf {
namespace {

// pred = last + (momentum * vel) * n and vel = (p - last) / n: one rounding per operation, in the order written
__device__ __forceinline__ double chain_predict(double last, double momentum, double vel, int n) {
#pragma clang fp contract(off)
    const double mv = momentum * vel;
    const double step = mv * (double)n;
    return last + step;
}

__device__ __forceinline__ double chain_velocity(double p, double last, int n) {
#pragma clang fp contract(off)
    const double d = p - last;
    return d / (double)n;
}

// start (K,3) fp64; positions, predicted (K,3,T) fp64; amplitudes / peaks (K,T) or NULL; lost_at (K,2).
__global__ __launch_bounds__(TK_THREADS) void follow_kernel(const float *__restrict__ frames, long ldf, TrackGeom g, int T,
                                                            const int *__restrict__ times, const double *__restrict__ start, int K,
                                                            int anchor, double momentum, int max_gap,
                                                            const float *__restrict__ background, double *__restrict__ positions,
                                                            float *__restrict__ amplitudes, float *__restrict__ peaks,
                                                            double *__restrict__ predicted, int *__restrict__ lost_at) {
    extern __shared__ float lds[];
    __shared__ float s_wv[TK_WAVES];
    __shared__ int s_wi[TK_WAVES];
    __shared__ float s_e2[3];
    const TrackLds L = {lds, lds + g.rpad, lds + 2 * g.rpad, lds + 2 * g.rpad + g.nA, s_wv, s_wi, s_e2};
    const int tid = threadIdx.x;
    const int k = (int)(blockIdx.x % (unsigned)K), dir = (int)(blockIdx.x / (unsigned)K);   // 0 forward, 1 backward
    const int step = dir ? -1 : 1;
    const int nvisit = dir ? anchor + 1 : T - anchor;
    const double nan = __builtin_nan("");
    // the taps are the same for every frame; the first barrier of the first search orders them
    fill_taps(L.tap, L.c2, g.r, g.inv_s2, tid, TK_THREADS);
    double last[3], vel[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < 3; ++d) last[d] = start[(long)k * 3 + d];
    int n = 0, miss = 0;
    // a start that is not finite: the chain is lost before its first search
    int lost = __builtin_isfinite(last[0]) && __builtin_isfinite(last[1]) && __builtin_isfinite(last[2]) ? -1 : anchor;
    int i = 0;
    // everything the loop branches on is the same in every thread
    for (; i < nvisit && lost < 0; ++i) {
        const int j = anchor + i * step;
        const bool mine = !(dir && i == 0);       // the anchor frame's outputs are the forward chain's
        const long out = (long)k * T + j;
        double pred[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) pred[d] = chain_predict(last[d], momentum, vel[d], n);
        float phat[3] = {0.0f, 0.0f, 0.0f}, amp = 0.0f, peak = 0.0f;
        const bool found = track_search(frames + (long)(times ? times[j] : j) * ldf, background ? background[j] : 0.0f, g, pred[0], pred[1],
                                        pred[2], L, tid, phat, amp, peak);
        if (mine && tid == 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                predicted[((long)k * 3 + d) * T + j] = pred[d];
                positions[((long)k * 3 + d) * T + j] = found ? (double)phat[d] : nan;
            }
            if (amplitudes) amplitudes[out] = found ? amp : __builtin_nanf("");
            if (peaks) peaks[out] = found ? peak : __builtin_nanf("");
        }
        if (found) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double p = (double)phat[d];
                if (n > 0) vel[d] = chain_velocity(p, last[d], n);
                last[d] = p;
            }
            n = 1, miss = 0;
        } else {
            ++n, ++miss;
            if (miss > max_gap) lost = j;
        }
    }
    // a lost chain: the frames it did not visit
    for (int v = i + tid; v < nvisit; v += TK_THREADS) {
        if (dir && v == 0) continue;
        const int j = anchor + v * step;
        const long out = (long)k * T + j;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            predicted[((long)k * 3 + d) * T + j] = nan;
            positions[((long)k * 3 + d) * T + j] = nan;
        }
        if (amplitudes) amplitudes[out] = __builtin_nanf("");
        if (peaks) peaks[out] = __builtin_nanf("");
    }
    if (tid == 0) lost_at[(long)k * 2 + dir] = lost;
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_follow_neurons(const float *frames, long ldf, const int *sz, int T, const int *times, const double *start, int K, double sigma,
                        const int *search, int anchor, double momentum, int max_gap, double threshold, const float *background,
                        double *positions, float *amplitudes, float *peaks, double *predicted, int *lost_at, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames, DNMF_E_NULL, "dnmf_follow_neurons: NULL frames");
    DNMF_REQUIRE(sz, DNMF_E_NULL, "dnmf_follow_neurons: NULL sz");
    DNMF_REQUIRE(start, DNMF_E_NULL, "dnmf_follow_neurons: NULL start");
    DNMF_REQUIRE(search, DNMF_E_NULL, "dnmf_follow_neurons: NULL search");
    DNMF_REQUIRE(positions, DNMF_E_NULL, "dnmf_follow_neurons: NULL positions");
    DNMF_REQUIRE(predicted, DNMF_E_NULL, "dnmf_follow_neurons: NULL predicted");
    DNMF_REQUIRE(lost_at, DNMF_E_NULL, "dnmf_follow_neurons: NULL lost_at");
    TrackGeom g;
    size_t lds = 0;
    const int rc = track_geometry("dnmf_follow_neurons", sz, T, K, sigma, search, threshold, ldf, g, lds);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(anchor >= 0 && anchor < T, DNMF_E_SHAPE, "dnmf_follow_neurons: anchor=%d outside [0, %d)", anchor, T);
    DNMF_REQUIRE(momentum >= 0.0 && momentum <= 1.0, DNMF_E_SHAPE, "dnmf_follow_neurons: momentum=%g must lie in [0, 1]", momentum);
    DNMF_REQUIRE(max_gap >= 0, DNMF_E_SHAPE, "dnmf_follow_neurons: max_gap=%d must not be negative", max_gap);
    DNMF_REQUIRE(K < (1 << 30), DNMF_E_UNSUPPORTED, "dnmf_follow_neurons: K=%d: 2 K workgroups do not fit a grid", K);
    hipLaunchKernelGGL(follow_kernel, dim3(2u * (unsigned)K), dim3(TK_THREADS), lds, (hipStream_t)stream, frames, ldf, g, T, times, start, K,
                       anchor, momentum, max_gap, background, positions, amplitudes, peaks, predicted, lost_at);
    return check_launch("dnmf_follow_neurons");
}

}  // extern "C"
