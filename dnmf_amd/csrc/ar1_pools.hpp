// The AR(1) pool-adjacent-violators solver that K21 (deconvolve_traces.hip) and K32 (ar1_temporal.hip) share.
//
// With x_t = c_t g^-t the AR(1) constraint c_t >= g c_{t-1} reads x_t >= x_{t-1}: a weighted isotonic regression, solved by
// pool-adjacent-violators (PAVA).  A frame comes with num_t and den_t (K21: den_t = 1 for a valid frame; K32: den_t = w_t; 0 marks
// a frame without weight); a pool of frames [p, p + len) has the value num / den at its first frame and decays by g a frame.  One
// workgroup of THREADS lanes per trace, everything in float64, every lane calls the three steps in their order:
//   pools_local   lane i runs PAVA on its own `per` contiguous frames [c0, c1).  A pool's record (num, den, len, prev) sits in the
//                 slot of its first frame, len = 0 marks a slot that starts no pool, prev chains the stack.  -> the lane's top pool;
//   pools_stitch  log2(THREADS) levels: at the level of stride s the lanes i = 0, 2s, 4s, .. append the pools of the segments
//                 [i + s, i + 2s) to the stack of the segments [i, i + s) one by one, merging backwards while they violate, and stop
//                 at the first pool that fits without a merge (the rest of the right block is in order already).  The pairs of a
//                 level touch disjoint slots; one barrier a level;
//   pools_expand  every lane walks its frames in order and hands (t, c_t, s_t) to the caller -> the pools that start in them.
// A leading run of frames without weight is a pool with den = 0: it is never merged into (`violates` is false for it), and frames
// without weight further on merge backwards.  The barriers stand in loops whose trip counts depend on THREADS only, never on the
// data.  No floating-point atomics, no reduction here at all: what the caller sums from pools_expand it sums in frame order.
// The records take POOL_RECORD bytes a frame, in LDS up to POOL_LDS_FRAMES frames (K32's limit; K21 moves them to a workspace
// beyond it).
#pragma once

#include <cmath>

#include "block_ops.hpp"

namespace dnmf {

constexpr int POOL_STATIC_LDS = 16 * 1024;                         // bytes set aside for the callers' static arrays (they take 8.2 KiB)
constexpr int POOL_DYNAMIC_LDS = 160 * 1024 - POOL_STATIC_LDS;
constexpr int POOL_RECORD = 24;                                    // bytes of a pool record: num, den (double), len, prev (int)
constexpr int POOL_LDS_FRAMES = POOL_DYNAMIC_LDS / POOL_RECORD;    // 6144: the longest trace whose records fit LDS

// a trace's pool records, and this lane's share of its frames
struct Pools {
    double *num, *den;
    int *len, *prev;
    double lng;          // log g
    int T, per, c0, c1;  // `per` frames a lane; this lane's are [c0, c1)
};

// the records of T frames over `base` (LDS or global memory, 8-byte aligned, POOL_RECORD * T bytes)
template <int THREADS>
__device__ __forceinline__ Pools pools_over(void *base, int T, double lng) {
    Pools P;
    P.num = static_cast<double *>(base), P.den = P.num + T;
    P.len = reinterpret_cast<int *>(P.den + T), P.prev = P.len + T;
    P.lng = lng, P.T = T, P.per = (T + THREADS - 1) / THREADS;
    P.c0 = (int)min((long)T, (long)threadIdx.x * P.per), P.c1 = min(T, P.c0 + P.per);
    return P;
}

__device__ __forceinline__ bool violates(const Pools &P, int p, int q) {
    const double dp = P.den[p];
    if (!(dp > 0.0)) return false;   // only a leading run of frames without weight: never merged into
    const double dq = P.den[q];
    if (!(dq > 0.0)) return true;    // frames without weight merge backwards
    return P.num[q] / dq < (P.num[p] / dp) * exp((double)P.len[p] * P.lng);
}

__device__ __forceinline__ void merge(const Pools &P, int p, int q) {
    const double gl = exp((double)P.len[p] * P.lng);
    P.num[p] = P.num[p] + gl * P.num[q];
    P.den[p] = P.den[p] + gl * gl * P.den[q];
    P.len[p] = P.len[p] + P.len[q];
    P.len[q] = 0;
}

// merge p backwards while it violates -> the pool it ends up in
__device__ __forceinline__ int settle(const Pools &P, int p) {
    for (;;) {
        const int pp = P.prev[p];
        if (pp < 0 || !violates(P, pp, p)) return p;
        merge(P, pp, p);
        p = pp;
    }
}

// PAVA on the lane's own frames -> its top pool (-1: no frame).  fill(t) writes num[t] and den[t] just before frame t is pushed
// (a caller whose records are complete, behind a barrier, passes a no-op).
template <typename Fill>
__device__ __forceinline__ int pools_local(const Pools &P, Fill fill) {
    int top = -1;
    for (int t = P.c0; t < P.c1; ++t) {
        fill(t);
        P.len[t] = 1, P.prev[t] = top;
        top = settle(P, t);
    }
    return top;
}

// The stitch: block [tid, tid + s) of segments takes in block [tid + s, tid + 2 s).  s_top: THREADS ints of LDS.
template <int THREADS>
__device__ __forceinline__ void pools_stitch(const Pools &P, int top, int *s_top) {
    const int tid = threadIdx.x, T = P.T;
    s_top[tid] = top;
    __syncthreads();
    for (int s = 1; s < THREADS; s <<= 1) {
        if ((tid & (2 * s - 1)) == 0) {
            const long first = (long)(tid + s) * P.per;
            if (first < T) {
                const int end = (int)min((long)T, (long)(tid + 2 * s) * P.per);
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
}

// The expansion: frame(t, c, s) for the lane's frames in order, c the solution and s = max(c_t - g c_{t-1}, 0) at a pool start
// (c_0 at t = 0), 0 inside a pool -> the pools that start in the lane's frames.  s_last: THREADS ints of LDS.  The records are
// only read; the caller's next barrier frees them.
template <int THREADS, typename Frame>
__device__ __forceinline__ int pools_expand(const Pools &P, double g, int *s_last, Frame frame) {
    const int tid = threadIdx.x;
    // the last pool start at or before the end of every lane's frames
    int last = -1;
    for (int t = P.c0; t < P.c1; ++t)
        if (P.len[t] > 0) last = t;
    s_last[tid] = last;
    __syncthreads();
    int pools = 0;
    if (P.c0 < P.c1) {
        int cur = -1;                                   // the pool that covers frame c0 - 1
        for (int l = tid - 1; l >= 0 && cur < 0; --l) cur = s_last[l];
        double cv = 0.0, cprev = 0.0;                   // the pool's max(v, 0); c of the frame before
        if (cur >= 0) {
            const double d = P.den[cur];
            cv = d > 0.0 ? fmax(P.num[cur] / d, 0.0) : 0.0;
            cprev = cv * exp((double)(P.c0 - 1 - cur) * P.lng);
        }
        for (int t = P.c0; t < P.c1; ++t) {
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
            frame(t, c, s);
        }
    }
    return pools;
}

// host: a launch with more than the default 48 KiB of dynamic LDS has to raise the kernel's limit first
inline int allow_dynamic_lds(const char *fn, const void *kernel, unsigned bytes) {
    if (bytes <= 48u * 1024u) return DNMF_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail((int)e, "%s: %u bytes of LDS: %s", fn, bytes, hipGetErrorString(e));
    return DNMF_OK;
}

}  // namespace dnmf
