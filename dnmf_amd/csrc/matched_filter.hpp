// The arithmetic K14 (detect_neurons.hip) and K15 (track_neurons.hip) share: the taps g1(d) = exp(-d^2 / sigma^2) of the
// matched filter and the running sums of their squares, the per-axis noise weight, the (value, lowest index) arg-max, the
// log-parabola refinement of a peak and the least-squares amplitude of the truncated footprint.  tests/detect_restatement.py
// is the definition in float64; everything here is fp32.
#pragma once

#include "common.hpp"

namespace dnmf {

constexpr int MF_R_MAX = 96;      // taps per side: sigma <= 32

// tap[i] = g1(i) and c2[i] = tap[0]^2 + ... + tap[i]^2 for i <= r, made by the threads tid, tid + nthreads, ...
__device__ __forceinline__ void fill_taps(float *tap, float *c2, int r, float inv_s2, int tid, int nthreads) {
    for (int i = tid; i <= r; i += nthreads) {
        tap[i] = expf(-(float)(i * i) * inv_s2);
        float acc = 0.0f;
        for (int j = 0; j <= i; ++j) {
            const float t = expf(-(float)(j * j) * inv_s2);
            acc += t * t;
        }
        c2[i] = acc;
    }
}

// sum of the squared taps inside an axis of S voxels at voxel s, from c2[k] = tap[0]^2 + ... + tap[k]^2
__device__ __forceinline__ float axis_norm(const float *c2, int r, int s, int S) { return c2[min(r, s)] + c2[min(r, S - 1 - s)] - c2[0]; }
// sqrt(nmax / n(s)): 1 where the window is inside the volume
__device__ __forceinline__ float axis_weight(const float *c2, int r, int s, int S) {
    return sqrtf(axis_norm(c2, r, (S - 1) / 2, S) / axis_norm(c2, r, s, S));
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// (largest value, lowest index among equals) over the wave, valid in lane 63: the fixed tree of wave_sum_last with the
// lanes that have no partner keeping their own pair
template <int CTRL, int RMASK>
__device__ __forceinline__ void argmax_step(float &v, int &i) {
    const int vb = __builtin_bit_cast(int, v);
    const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(vb, vb, CTRL, RMASK, 0xf, false));
    const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, RMASK, 0xf, false);
    const bool take = better(ov, oi, v, i);
    v = take ? ov : v, i = take ? oi : i;
}

__device__ __forceinline__ void wave_argmax_last(float &v, int &i) {
    argmax_step<0x111, 0xf>(v, i);  // row_shr:1
    argmax_step<0x112, 0xf>(v, i);  // row_shr:2
    argmax_step<0x114, 0xf>(v, i);  // row_shr:4
    argmax_step<0x118, 0xf>(v, i);  // row_shr:8 -> lane 15 of a row holds the row's pair
    argmax_step<0x142, 0xa>(v, i);  // row_bcast:15 into rows 1 and 3
    argmax_step<0x143, 0xc>(v, i);  // row_bcast:31 into rows 2 and 3
}

// One axis of the refinement of a peak c > 0: the parabola f(t) = ln c + b t + a2 t^2 through ln S at p* and its two
// neighbours (m, q) when `two`; else, at the first (`first`) or last voxel of an axis of three or more, the one through p*
// and the two voxels inward, m next to p* and q beyond it (t counts inward there).  Where m, q > 0 and a2 < 0: dl = the
// peak's offset from p* along the axis, clamped to +-1/2, and adj = f(t) - ln c there; else both 0.
__device__ __forceinline__ void refine_axis(float c, float m, float q, bool two, bool first, float &dl, float &adj) {
    dl = 0.0f, adj = 0.0f;
    if (m > 0.0f && q > 0.0f) {
        const float lm = logf(m), lc = logf(c), lq = logf(q);
        // f(t) = lc + b t + a2 t^2
        const float a2 = two ? 0.5f * (lm - 2.0f * lc + lq) : 0.5f * (lc - 2.0f * lm + lq);
        const float b = two ? 0.5f * (lq - lm) : (lm - lc) - a2;
        if (a2 < 0.0f) {
            const float t = fminf(0.5f, fmaxf(-0.5f, -b / (2.0f * a2)));
            adj = b * t + a2 * t * t;
            dl = two || first ? t : -t;
        }
    }
}

// S^ from S(p*) and the three adj of refine_axis
__device__ __forceinline__ float refined_score(float c, float adj0, float adj1, float adj2) { return c * expf((adj0 + adj1) + adj2); }

// g1(x - p^) at the voxel x = p* + o of an axis of S voxels (0 outside the volume), p^ = p* + dl
__device__ __forceinline__ float footprint_tap(int p, int o, float dl, int S, float inv_s2) {
    const float t = (float)o - dl;
    return in_range(p + o, S) ? expf(-(t * t) * inv_s2) : 0.0f;
}

// a = S^ / sqrt(prod_axis nmax sum e^2) for the footprint a e_x e_y e_z: e2[d] = the sum of footprint_tap^2 over |o| <= r
__device__ __forceinline__ float footprint_amplitude(float shat, const float *c2, int r, const int *S, float e2x, float e2y, float e2z) {
    return shat / sqrtf(((e2x * axis_norm(c2, r, (S[0] - 1) / 2, S[0])) * (e2y * axis_norm(c2, r, (S[1] - 1) / 2, S[1]))) *
                        (e2z * axis_norm(c2, r, (S[2] - 1) / 2, S[2])));
}

}  // namespace dnmf
