// What the analysis kernels (K11 .. K13, K18 .. K27) share: wave and workgroup reductions in a fixed order, order statistics on
// the monotone 64-bit key of a float64 (one by bisection, many by a workgroup sort), and the host-side plan of a call whose frames
// go in segments.  The hot path (K2, K3*, K4*,
// K7, K16) keeps its own fp32 reductions (common.hpp: wave_sum_last).
//
// The contract of the reductions.  "The same input gives the same bits" is a promise of every kernel that includes this file, and
// it rests on the order in which the terms are added: that order is part of the interface, not a detail of the implementation.
//   wave          offsets 32, 16, .. 1 over the 64 lanes.  wave_reduce / wave_sum (shfl_down): the result is valid in lane 0 only.
//                 wave_sum_all (shfl_xor butterfly): the result is in every lane.  No barrier, no LDS.
//   block_reduce  the wave tree, lane 0 of each wave stores to red[wave], a barrier, every lane forms red[0] op red[1] op .. in wave
//                 order, a second barrier.  The result is in every lane; `red` (THREADS / 64 values of 8 bytes) is free on return.
//   block_sum0    the wave tree, red[wave], ONE barrier, thread 0 forms 0.0 + red[0] + red[1] + ..; the result is valid in thread 0
//                 only (0.0 elsewhere).  `red` (THREADS / 64 doubles) is free again after the caller's next barrier.
// Every lane of the workgroup must reach a block_* call (they hold barriers), and THREADS is the workgroup's size, a multiple of 64.
// What a lane adds up before it calls (its frames t = lane, lane + THREADS, .. in that order, say) is the caller's half of the order.
#pragma once

#include <cstdint>

#include "common.hpp"

namespace dnmf {

// bytes rounded up to the 256-byte granule of the workspace layouts
__host__ __device__ constexpr size_t align256(size_t n) { return (n + 255) / 256 * 256; }

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- reductions ----------------------------------------------------------------------------------------------------------------
struct OpSum {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpOr {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a | b; }
};
struct OpMinKey {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a < b ? a : b; }
};
struct OpFmin {   // NaN is the neutral element: nanmin
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpFmax {
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_down(v, off, 64));
    return v;
}

__device__ __forceinline__ double wave_sum(double v) { return wave_reduce(v, OpSum()); }

template <typename T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int THREADS, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, void *redv) {
    T *red = static_cast<T *>(redv);
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = red[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) s = op(s, red[w]);
    __syncthreads();
    return s;
}

template <int THREADS>
__device__ __forceinline__ double block_sum0(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) s += red[w];
    return s;
}

// ---- order statistics on 64-bit keys -------------------------------------------------------------------------------------------
constexpr uint64_t NANKEY = ~0ull;

// value -> key with key(a) < key(b) <=> a < b; every NaN -> NANKEY, above every value
__device__ __forceinline__ uint64_t to_key(double v) {
    if (v != v) return NANKEY;
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

__device__ __forceinline__ double from_key(uint64_t k) {
    if (k == NANKEY) return quiet_nan();
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// x[0..n) (doubles, NaN = none) -> keys in place; returns the lowest key bit that any value has set (63 when there is none; 0 as
// soon as one value is negative, whose key is the complement of its bits): the bits below it need no pass.
template <int THREADS>
__device__ __forceinline__ int to_keys(double *x, int n, void *red) {
    uint64_t bits = 0;
    for (int t = threadIdx.x; t < n; t += THREADS) {
        const double v = x[t];
        if (v == v) {
            const uint64_t u = (uint64_t)__double_as_longlong(v);
            bits |= (u >> 63) ? 1ull : u;
        }
        x[t] = __longlong_as_double((long long)to_key(v));
    }
    bits = block_reduce<THREADS>(bits, OpOr(), red) & ~(1ull << 63);   // ends with a barrier: the keys are visible
    return bits ? __builtin_ctzll(bits) : 63;
}

// The k-th and (k + 1)-th smallest (from 0; the k-th again when there is no further one) of the keys above `above` that are
// no NANKEY, 0 <= k < their count.  One block-wide count per key bit from 63 down to lowbit.  above = 0 takes every key: no
// double that is not a NaN has the key 0 -- the only bit pattern that would map to it is the all-ones NaN, and a NaN becomes
// NANKEY before that -- so kk > 0 holds for every key that counts.  ABOVE = false is that case without the comparison (measured
// on K21: 2 to 8 % of a call); `above` is then not read.
template <int THREADS, bool ABOVE = true>
__device__ __forceinline__ void block_select_pair(const uint64_t *key, int n, uint64_t above, int k, int count, int lowbit, void *red,
                                                  double &v0, double &v1) {
    uint64_t pre = 0;
    for (int bit = 63; bit >= lowbit; --bit) {
        const uint64_t cand = pre | (1ull << bit);
        int c = 0;
        for (int t = threadIdx.x; t < n; t += THREADS) {
            const uint64_t kk = key[t];
            c += (!ABOVE || kk > above) && kk < cand;
        }
        if (block_reduce<THREADS>(c, OpSum(), red) <= k) pre = cand;
    }
    int cle = 0;
    uint64_t nxt = NANKEY;
    for (int t = threadIdx.x; t < n; t += THREADS) {
        const uint64_t kk = key[t];
        cle += (!ABOVE || kk > above) && kk <= pre;
        if (kk > pre && kk < nxt) nxt = kk;
    }
    cle = block_reduce<THREADS>(cle, OpSum(), red);
    nxt = block_reduce<THREADS>(nxt, OpMinKey(), red);
    v0 = from_key(pre);
    v1 = (k + 1 >= count || cle >= k + 2) ? v0 : from_key(nxt);
}

// np.median of the `count` >= 1 keys that are no NANKEY
template <int THREADS>
__device__ __forceinline__ double block_median(const uint64_t *key, int n, int count, int lowbit, void *red) {
    double v0, v1;
    block_select_pair<THREADS, false>(key, n, 0, (count - 1) >> 1, count, lowbit, red, v0, v1);
    return (count & 1) ? v0 : 0.5 * (v0 + v1);
}

// The power of two at or above n >= 1: the keys that block_sort_keys needs room for.
__host__ __device__ constexpr int sort_size(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// key[0..n) -> ascending, in place, NANKEYs last; for callers that want many order statistics of one row (after the sort the k-th
// smallest is key[k]), where block_select_pair would cost 64 counting passes each.  `key` must have room for sort_size(n) keys:
// [n, sort_size(n)) is filled with NANKEY here and holds NANKEY on return.  The caller's own writes of key[0..n) need no barrier
// before the call (the fill touches other slots and a barrier follows it); the call ends with a barrier, and every lane of the
// workgroup must reach it.
// The contract of the order: a bitonic network over P = sort_size(n) slots -- for k = 2, 4, .. P and j = k / 2, k / 4, .. 1 the
// slots l < (l | j) with bit j of l clear are compared and exchanged towards ascending where bit k of l is clear, descending
// elsewhere; one barrier after each of the log2(P) (log2(P) + 1) / 2 steps, nothing but LDS.  Keys are totally ordered and equal
// keys are the same bits, so the sorted row does not depend on the network at all: the same input gives the same bits, and an
// exchange of equal keys is skipped.  Banks: for j >= 32 the 32 lanes of a half-wave read 32 consecutive keys (one 256-byte bank
// row: no conflict); for j < 32 they read 32 keys out of 64 consecutive ones, two bank rows: 2-way.
template <int THREADS>
__device__ __forceinline__ void block_sort_keys(uint64_t *key, int n) {
    const int P = sort_size(n);
    for (int t = n + (int)threadIdx.x; t < P; t += THREADS) key[t] = NANKEY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t a = key[lo], b = key[hi];
                if ((lo & k) == 0 ? a > b : a < b) key[lo] = b, key[hi] = a;
            }
            __syncthreads();
        }
}

// ---- the frame segments of a streamed call (host) ------------------------------------------------------------------------------
// A call of B frames is cut into nseg segments of seglen frames that ride on gridDim.y.  segment > 0 sets seglen; 0 asks for about
// target_blocks workgroups over the call's `units` (tiles, neurons), with segments no shorter than min_segment frames.  cap is the
// most segments a call of B frames can have: it sizes the state, and does not decrease with B.
struct SegmentPlan {
    int seglen, nseg;
    long cap;
};

inline int segment_plan(const char *fn, int B, int segment, long units, int target_blocks, int min_segment, SegmentPlan &p) {
    DNMF_REQUIRE(segment >= 0, DNMF_E_SHAPE, "%s: segment=%d", fn, segment);
    if (segment > 0) {
        p.seglen = segment;
        p.cap = ((long)B + segment - 1) / segment;
    } else {
        long want = (target_blocks + units - 1) / units;
        const long most = ((long)B + min_segment - 1) / min_segment;
        if (want > most) want = most;
        p.seglen = (int)((B + want - 1) / want);
        p.cap = want;
    }
    DNMF_REQUIRE(p.cap <= 65535, DNMF_E_UNSUPPORTED, "%s: %ld segments of %d frames (they ride on gridDim.y: at most 65535)", fn, p.cap,
                 p.seglen);
    p.nseg = (int)(((long)B + p.seglen - 1) / p.seglen);
    return DNMF_OK;
}

}  // namespace dnmf
