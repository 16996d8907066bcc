// K15: per-frame neuron tracking by a local matched filter (tests/track_restatement.py is the definition, in float64;
// everything here is fp32, widened where the positions are stored).
//
// For every neuron k and frame j the score volume of K14 -- S = g (*) (frame - background) prod_axis sqrt(nmax / n(q)), g the
// footprint model's own Gaussian truncated at r = ceil(3 sigma) -- is evaluated only where it is needed: on the search window
// |q - c| <= search around the rounded prediction c and the one-voxel ring around it that the refinement reads.  The K T
// searches are independent: nothing is subtracted and nothing excluded, so a neuron within about 2 sigma of a brighter one
// can be captured by it; the search window is the guard.
//
// One launch, one workgroup of 256 threads per (k, j), blocks of one frame next to one another (their regions share lines in
// L2); the search itself -- region, passes, pick, refine -- is track_search.hpp, which K15c (follow_neurons.hip) runs frame
// after frame.
#include "track_search.hpp"

namespace dnmf {
namespace {

// predict (K,3,T) or (K,3); positions (K,3,T) fp64, amplitudes / peaks (K,T) or NULL.
template <typename TP>
__global__ __launch_bounds__(TK_THREADS) void track_kernel(const float *__restrict__ frames, long ldf, TrackGeom g, int T,
                                                           const int *__restrict__ times, const TP *__restrict__ predict, int per_frame,
                                                           int K, const float *__restrict__ background, double *__restrict__ positions,
                                                           float *__restrict__ amplitudes, float *__restrict__ peaks) {
    extern __shared__ float lds[];
    __shared__ float s_wv[TK_WAVES];
    __shared__ int s_wi[TK_WAVES];
    __shared__ float s_e2[3];
    const TrackLds L = {lds, lds + g.rpad, lds + 2 * g.rpad, lds + 2 * g.rpad + g.nA, s_wv, s_wi, s_e2};
    const int tid = threadIdx.x;
    const int k = (int)(blockIdx.x % (unsigned)K), j = (int)(blockIdx.x / (unsigned)K);
    const long out = (long)k * T + j;
    const long pin = per_frame ? (long)k * 3 * T + j : (long)k * 3;
    const long pst = per_frame ? T : 1;
    fill_taps(L.tap, L.c2, g.r, g.inv_s2, tid, TK_THREADS);
    float phat[3] = {0.0f, 0.0f, 0.0f}, amp = 0.0f, peak = 0.0f;
    // `found` is the same in every thread
    const bool found = track_search(frames + (long)(times ? times[j] : j) * ldf, background ? background[j] : 0.0f, g, (double)predict[pin],
                                    (double)predict[pin + pst], (double)predict[pin + 2 * pst], L, tid, phat, amp, peak);
    if (tid == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) positions[((long)k * 3 + d) * T + j] = found ? (double)phat[d] : __builtin_nan("");
        if (amplitudes) amplitudes[out] = found ? amp : __builtin_nanf("");
        if (peaks) peaks[out] = found ? peak : __builtin_nanf("");
    }
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_track_neurons(const float *frames, long ldf, const int *sz, int T, const int *times, const void *predict, int predict_f64,
                       int predict_per_frame, int K, double sigma, const int *search, double threshold, const float *background,
                       double *positions, float *amplitudes, float *peaks, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames, DNMF_E_NULL, "dnmf_track_neurons: NULL frames");
    DNMF_REQUIRE(sz, DNMF_E_NULL, "dnmf_track_neurons: NULL sz");
    DNMF_REQUIRE(predict, DNMF_E_NULL, "dnmf_track_neurons: NULL predict");
    DNMF_REQUIRE(search, DNMF_E_NULL, "dnmf_track_neurons: NULL search");
    DNMF_REQUIRE(positions, DNMF_E_NULL, "dnmf_track_neurons: NULL positions");
    TrackGeom g;
    size_t lds = 0;
    const int rc = track_geometry("dnmf_track_neurons", sz, T, K, sigma, search, threshold, ldf, g, lds);
    if (rc != DNMF_OK) return rc;
    const dim3 grid((unsigned)((long)K * T));
    const hipStream_t st = (hipStream_t)stream;
    if (predict_f64)
        hipLaunchKernelGGL(track_kernel<double>, grid, dim3(TK_THREADS), lds, st, frames, ldf, g, T, times, static_cast<const double *>(predict),
                           predict_per_frame, K, background, positions, amplitudes, peaks);
    else
        hipLaunchKernelGGL(track_kernel<float>, grid, dim3(TK_THREADS), lds, st, frames, ldf, g, T, times, static_cast<const float *>(predict),
                           predict_per_frame, K, background, positions, amplitudes, peaks);
    return check_launch("dnmf_track_neurons");
}

}  // extern "C"
