// The search K15 (track_neurons.hip), K15c (follow_neurons.hip) and K15x (track_exclusive.hip) share: one workgroup of TK_THREADS threads looks for the
// peak of one frame's K14 score inside the window around one predicted position (tests/track_restatement.py is the
// definition, in float64; everything here is fp32), and the host-side geometry that sizes its LDS.
//
//   region   the voxels of the volume within r of the scores wanted: at most prod_axis min(S, 2 (search + 1 + r) + 1), loaded
//            with the background taken off into LDS along the contiguous axis; voxels beyond the volume are not stored -- the
//            passes clip their taps to the region, which is the zero padding.
//   passes   three separable passes from LDS to LDS, the axis with the longest region first (the host fixes the order from
//            the largest extents a region can have, so the two buffers it sizes hold every pass): each pass makes only the
//            scores of window + ring along its own axis, so the later passes work on 2 search + 3 planes instead of
//            2 (search + 1 + r) + 1, and multiplies in the weight of its axis.  Lanes run along the contiguous axis:
//            consecutive LDS words for every tap.
//   pick     arg-max over the window (equal scores: the lowest voxel index of the volume, NaN scores never win): DPP per wave,
//            four pairs through LDS.
//   refine   every thread evaluates the three log-parabolas (LDS broadcasts); waves 0..2 sum the squared footprint taps of one
//            axis each; thread 0 gets the amplitude.
// LDS: the two buffers and the taps, at most TK_LDS_BUDGET bytes, so at least three workgroups fit a CU whatever the
// arguments; at sigma = 3, search (6, 6, 1) on Z = 2 it is 13 KB and the 8 workgroups of a CU's 32 waves all fit.
#pragma once

#include "matched_filter.hpp"

namespace dnmf {
namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr size_t TK_LDS_BUDGET = 48 * 1024;   // bytes of LDS a workgroup may ask for: region + first pass + taps

struct TrackGeom {
    int X, Y, Z;
    int r;
    int sx, sy, sz;       // search
    int o0, o1, o2;       // the axes in the order of the passes
    int nA;               // floats of the first buffer
    int rpad;             // floats of one tap table
    float inv_s2, threshold;
};

__device__ __forceinline__ int pick3(int d, int a, int b, int c) { return d == 0 ? a : (d == 1 ? b : c); }

// Per axis: the window [wlo, whi] (clipped to the volume), the scores wanted [slo, shi] = window + ring, widened to the
// three voxels the one-sided parabola reads where the window touches an end of the axis, and the region [ilo, ihi] within r
// of them.  False when the prediction is not finite or the window has no voxel in the volume.
__device__ __forceinline__ bool axis_ranges(double p, int search, int r, int S, int &wlo, int &whi, int &slo, int &shi, int &ilo,
                                            int &ihi) {
    const double c = rint(p);                           // half to even
    if (!(__builtin_isfinite(c) && c + (double)search >= 0.0 && c - (double)search <= (double)(S - 1))) return false;
    wlo = (int)fmax(c - (double)search, 0.0), whi = (int)fmin(c + (double)search, (double)(S - 1));
    slo = max(0, wlo - 1), shi = min(S - 1, whi + 1);
    if (wlo == 0) shi = max(shi, min(S - 1, 2));
    if (whi == S - 1) slo = min(slo, max(0, S - 3));
    ilo = max(0, slo - r), ihi = min(S - 1, shi + r);
    return true;
}

// One pass along axis d: src holds the box of extents (c0, c1, c2) whose first voxel is (q0, q1, q2) of the volume; dst gets
// the same box with axis d cut to [lo, hi], each value the tap sum along d over the voxels of src's box within r, times the
// weight of its place.  Updates the box.
__device__ __forceinline__ void filter_pass(const float *src, float *dst, const float *tap, const float *c2, int r, int d, int lo, int hi,
                                            int S, int &c0, int &c1, int &c2e, int &q0, int &q1, int &q2, int tid) {
    const int cd = pick3(d, c0, c1, c2e), qd = pick3(d, q0, q1, q2);
    const int stride = pick3(d, c1 * c2e, c2e, 1);
    const int n0 = d == 0 ? hi - lo + 1 : c0, n1 = d == 1 ? hi - lo + 1 : c1, n2 = d == 2 ? hi - lo + 1 : c2e;
    const int nout = n0 * n1 * n2;
    for (int e = tid; e < nout; e += TK_THREADS) {
        const int l2 = e % n2, l1 = (e / n2) % n1, l0 = e / (n2 * n1);
        const int q = lo + pick3(d, l0, l1, l2);
        const int klo = max(q - r, qd), khi = min(q + r, qd + cd - 1);
        // src index of the first tap: this output's place with axis d moved to klo
        const int base = ((d == 0 ? klo - qd : l0) * c1 + (d == 1 ? klo - qd : l1)) * c2e + (d == 2 ? klo - qd : l2);
        float acc = 0.0f;
        for (int x = klo; x <= khi; ++x) acc += tap[abs(x - q)] * src[base + (x - klo) * stride];
        dst[e] = acc * axis_weight(c2, r, q, S);
    }
    c0 = n0, c1 = n1, c2e = n2;
    if (d == 0) q0 = lo;
    if (d == 1) q1 = lo;
    if (d == 2) q2 = lo;
}

// The LDS of one search, carved from the dynamic region of track_geometry's size, and the few words the waves exchange.
struct TrackLds {
    float *tap, *c2, *bufA, *bufB;
    float *wv;     // TK_WAVES
    int *wi;       // TK_WAVES
    float *e2;     // 3
};

// What a search does to the region as it stages it.  K15 and K15c stage the frame as it is; K15x (track_exclusive.hip) takes the
// placed neighbours off.  begin: the region is known -- the box of extents (c0, c1, c2) whose first voxel is (q0, q1, q2) -- and
// nothing of it is staged yet; operator(): the value to store for the voxel (l0, l1, l2) of the box, given frame - background;
// finish: every thread has stored its values in buf (voxel e = tid, tid + TK_THREADS, ...), the barrier that ends the
// staging has not been reached.  begin and finish are called by the whole workgroup and may hold barriers.
struct StageAsIs {
    __device__ __forceinline__ void begin(int, int, int, int, int, int, int) {}
    __device__ __forceinline__ float operator()(float v, int, int, int) const { return v; }
    __device__ __forceinline__ void finish(float *, int) {}
};

// One search of the frame row `fr` (background `bg` taken off) around `pred`, by the whole workgroup; every argument, and so
// the result and every branch around a barrier, is the same in every thread.  The caller has filled L.tap / L.c2 (fill_taps;
// the first barrier here orders them) and no thread may still read L of an earlier search of a kind that this one writes: the
// barriers of a search order bufA, bufB, wv and wi against the search before; e2 and c2 are read by thread 0 after the last
// barrier and written again only after the first barriers of the next search.
// True: p^ in phat (every thread), the score at the picked voxel in peak (every thread), the amplitude in amp (thread 0 only),
// p* in pick (every thread).
template <typename Stage>
__device__ __forceinline__ bool track_search_staged(const float *__restrict__ fr, float bg, const TrackGeom &g, double px, double py,
                                                    double pz, const TrackLds &L, int tid, float (&phat)[3], float &amp, float &peak,
                                                    int (&pick)[3], Stage &stage) {
    const float *tap = L.tap, *c2 = L.c2;
    float *bufA = L.bufA, *bufB = L.bufB;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = g.r;
    const int S[3] = {g.X, g.Y, g.Z};
    int wlo[3], whi[3], slo[3], shi[3], ilo[3], ihi[3];
    bool found = axis_ranges(px, g.sx, r, g.X, wlo[0], whi[0], slo[0], shi[0], ilo[0], ihi[0]);
    found = axis_ranges(py, g.sy, r, g.Y, wlo[1], whi[1], slo[1], shi[1], ilo[1], ihi[1]) && found;
    found = axis_ranges(pz, g.sz, r, g.Z, wlo[2], whi[2], slo[2], shi[2], ilo[2], ihi[2]) && found;
    if (!found) return false;
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    // region
    int c0 = ihi[0] - ilo[0] + 1, c1 = ihi[1] - ilo[1] + 1, c2e = ihi[2] - ilo[2] + 1;
    int q0 = ilo[0], q1 = ilo[1], q2 = ilo[2];
    const int nin = c0 * c1 * c2e;
    stage.begin(q0, q1, q2, c0, c1, c2e, tid);
    for (int e = tid; e < nin; e += TK_THREADS) {
        const int l2 = e % c2e, l1 = (e / c2e) % c1, l0 = e / (c2e * c1);
        bufA[e] = stage(fr[((long)(q0 + l0) * g.Y + (q1 + l1)) * g.Z + (q2 + l2)] - bg, l0, l1, l2);
    }
    stage.finish(bufA, tid);
    __syncthreads();
    filter_pass(bufA, bufB, tap, c2, r, g.o0, pick3(g.o0, slo[0], slo[1], slo[2]), pick3(g.o0, shi[0], shi[1], shi[2]),
                pick3(g.o0, g.X, g.Y, g.Z), c0, c1, c2e, q0, q1, q2, tid);
    __syncthreads();
    filter_pass(bufB, bufA, tap, c2, r, g.o1, pick3(g.o1, slo[0], slo[1], slo[2]), pick3(g.o1, shi[0], shi[1], shi[2]),
                pick3(g.o1, g.X, g.Y, g.Z), c0, c1, c2e, q0, q1, q2, tid);
    __syncthreads();
    filter_pass(bufA, bufB, tap, c2, r, g.o2, pick3(g.o2, slo[0], slo[1], slo[2]), pick3(g.o2, shi[0], shi[1], shi[2]),
                pick3(g.o2, g.X, g.Y, g.Z), c0, c1, c2e, q0, q1, q2, tid);
    __syncthreads();
    // bufB: the scores of the box (c0, c1, c2e) at (q0, q1, q2) = slo.  pick
    const int w1 = whi[1] - wlo[1] + 1, w2 = whi[2] - wlo[2] + 1;
    const int nw = (whi[0] - wlo[0] + 1) * w1 * w2;
    for (int e = tid; e < nw; e += TK_THREADS) {
        const int x = wlo[0] + e / (w2 * w1), y = wlo[1] + (e / w2) % w1, z = wlo[2] + e % w2;
        const float v = bufB[((x - q0) * c1 + (y - q1)) * c2e + (z - q2)];
        const int idx = (x * g.Y + y) * g.Z + z;
        if (better(v, idx, bv, bi)) bv = v, bi = idx;
    }
    wave_argmax_last(bv, bi);
    if (lane == 63) L.wv[wave] = bv, L.wi[wave] = bi;
    __syncthreads();
    bv = L.wv[0], bi = L.wi[0];
#pragma unroll
    for (int w = 1; w < TK_WAVES; ++w) {
        const float v = L.wv[w];
        const int i = L.wi[w];
        if (better(v, i, bv, bi)) bv = v, bi = i;
    }
    found = bv > g.threshold && bv < __builtin_inff() && bi != 0x7fffffff;
    if (!found) return false;
    // refine: the same in every thread
    const int p[3] = {bi / (g.Y * g.Z), (bi / g.Z) % g.Y, bi % g.Z};
    const int at = ((p[0] - q0) * c1 + (p[1] - q1)) * c2e + (p[2] - q2);
    const int stride[3] = {c1 * c2e, c2e, 1};
    float dl[3], adj[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        dl[d] = 0.0f, adj[d] = 0.0f;
        const bool two = p[d] > 0 && p[d] < S[d] - 1;
        const bool one = !two && S[d] >= 3;
        if (bv > 0.0f && (two || one)) {
            const int in = p[d] == 0 ? stride[d] : -stride[d];
            const float m = bufB[two ? at - stride[d] : at + in], q = bufB[two ? at + stride[d] : at + 2 * in];
            refine_axis(bv, m, q, two, p[d] == 0, dl[d], adj[d]);
        }
    }
    // sum of the squared footprint taps: wave d takes axis d
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (wave == d) {
            float acc = 0.0f;
            for (int o = lane - r; o <= r; o += 64) {
                const float e = footprint_tap(p[d], o, dl[d], S[d], g.inv_s2);
                acc += e * e;
            }
            acc = wave_sum_last(acc);
            if (lane == 63) L.e2[d] = acc;
        }
    }
    __syncthreads();
    if (tid == 0) amp = footprint_amplitude(refined_score(bv, adj[0], adj[1], adj[2]), c2, r, S, L.e2[0], L.e2[1], L.e2[2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) phat[d] = (float)p[d] + dl[d], pick[d] = p[d];
    peak = bv;
    return true;
}

// The search of K15 and K15c: the frame as it is.
__device__ __forceinline__ bool track_search(const float *__restrict__ fr, float bg, const TrackGeom &g, double px, double py, double pz,
                                             const TrackLds &L, int tid, float (&phat)[3], float &amp, float &peak) {
    StageAsIs stage;
    int pick[3];
    return track_search_staged(fr, bg, g, px, py, pz, L, tid, phat, amp, peak, pick, stage);
}

// 0 ok, else the error already recorded.  Everything that can be checked without the device.
inline int track_geometry(const char *fn, const int *sz, int T, int K, double sigma, const int *search, double threshold, long ldf,
                          TrackGeom &g, size_t &lds) {
    DNMF_REQUIRE(sz[0] > 0 && sz[1] > 0 && sz[2] > 0, DNMF_E_SHAPE, "%s: sz: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE((long)sz[0] * sz[1] * sz[2] < (1L << 31), DNMF_E_UNSUPPORTED, "%s: sz: volume %dx%dx%d has 2^31 voxels or more", fn,
                 sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(K >= 1, DNMF_E_SHAPE, "%s: K=%d must be at least 1", fn, K);
    DNMF_REQUIRE(T >= 1, DNMF_E_SHAPE, "%s: T=%d must be at least 1", fn, T);
    DNMF_REQUIRE(sigma > 0.0 && sigma < __builtin_inf(), DNMF_E_SHAPE, "%s: sigma=%g must be positive and finite", fn, sigma);
    DNMF_REQUIRE(search[0] >= 0 && search[1] >= 0 && search[2] >= 0, DNMF_E_SHAPE, "%s: search (%d, %d, %d) < 0", fn, search[0],
                 search[1], search[2]);
    DNMF_REQUIRE(threshold == threshold && threshold < __builtin_inf(), DNMF_E_SHAPE, "%s: threshold=%g must be below +inf", fn,
                 threshold);
    DNMF_REQUIRE(ldf >= (long)sz[0] * sz[1] * sz[2], DNMF_E_SHAPE, "%s: ldf=%ld for a volume of %ld voxels", fn, ldf,
                 (long)sz[0] * sz[1] * sz[2]);
    DNMF_REQUIRE(sigma <= MF_R_MAX / 3.0, DNMF_E_UNSUPPORTED, "%s: sigma=%g: the filter holds at most %d taps per side (sigma <= %d)", fn,
                 sigma, MF_R_MAX, MF_R_MAX / 3);
    DNMF_REQUIRE((long)K * T < (1L << 31), DNMF_E_UNSUPPORTED, "%s: K x T = %ld searches", fn, (long)K * T);
    g.X = sz[0], g.Y = sz[1], g.Z = sz[2];
    g.r = (int)__builtin_ceil(3.0 * sigma);
    g.sx = search[0], g.sy = search[1], g.sz = search[2];
    // the largest region and the most scores an axis can have (axis_ranges)
    long in[3], sc[3];
    for (int d = 0; d < 3; ++d) {
        in[d] = 2L * ((long)search[d] + 1 + g.r) + 1 < sz[d] ? 2L * ((long)search[d] + 1 + g.r) + 1 : sz[d];
        sc[d] = 2L * search[d] + 3 < sz[d] ? 2L * search[d] + 3 : sz[d];
    }
    int o[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2 - a; ++b)
            if (in[o[b]] < in[o[b + 1]]) {
                const int t = o[b];
                o[b] = o[b + 1], o[b + 1] = t;
            }
    g.o0 = o[0], g.o1 = o[1], g.o2 = o[2];
    g.rpad = (g.r + 4) & ~3;
    // buffer A: the region, then the second pass; buffer B: the first pass, then the scores (both smaller than what they follow)
    const long limit = (long)(TK_LDS_BUDGET / sizeof(float));
    const bool small = in[0] <= limit && in[1] <= limit && in[2] <= limit && in[0] * in[1] <= limit && in[0] * in[1] * in[2] <= limit;
    const long nA = small ? in[0] * in[1] * in[2] : 0;
    const long nB = small ? sc[o[0]] * in[o[1]] * in[o[2]] : 0;
    lds = small ? (size_t)(2 * g.rpad + nA + nB) * sizeof(float) : 0;
    DNMF_REQUIRE(small && lds <= TK_LDS_BUDGET, DNMF_E_UNSUPPORTED,
                 "%s: sigma=%g, search (%d, %d, %d): a region of %ld x %ld x %ld voxels needs more than the %zu bytes of LDS a workgroup "
                 "may take",
                 fn, sigma, search[0], search[1], search[2], in[0], in[1], in[2], TK_LDS_BUDGET);
    g.nA = (int)nA;
    g.inv_s2 = (float)(1.0 / (sigma * sigma));
    // a threshold below the fp32 range rounds to -inf, which every finite score passes
    g.threshold = (float)threshold;
    return DNMF_OK;
}

}  // namespace
}  // namespace dnmf
