// K30: exact order statistics over time, per voxel -- the samples of ranks lo and hi of up to four quantiles of a movie that does
// not fit in LDS.  include/dnmf_hip.h has the contract, tests/robust_restatement.py the definition.
//
// A radix select on the monotone 32-bit key of a float (block_ops.hpp's to_key, one word shorter), 4 bits a pass from the top:
// TS_DIGITS = 8 digit passes and one pair pass, each of which streams the movie once.  A workgroup owns TS_V contiguous voxels and a
// segment of frames: a frame row is read in full 1 KiB lines, and thread i keeps the 16 counters of its voxel (per quantile) in
// its own column of LDS -- cnt[(h 16 + digit) TS_V + i], bank i mod 32 whatever the digit, no two threads share a word, no barrier
// and no atomics in the loop.  At its end a workgroup adds its non-zero counters to the state with integer atomics (integer adds
// give the same sums in any order: the same input gives the same bits, however the movie is cut).  The open kernel of the next pass
// picks the digit and the remaining rank of every voxel and quantile and clears the counters; the pair pass counts the samples
// <= a_lo and takes the least sample above it, which settles a_hi without a second selection.
#include "block_ops.hpp"
#include "key32.hpp"

namespace dnmf {
namespace {

constexpr int TS_V = 256;              // voxels of a workgroup = its threads
constexpr int TS_BINS = 16;            // 4-bit digits
constexpr int TS_DIGITS = 8;           // digit passes; pass TS_DIGITS is the pair pass
constexpr int TS_MAXQ = 4;
constexpr int TS_UNROLL = 4;           // frames whose loads are in flight together
constexpr int TS_MIN_SEGMENT = 64;     // frames: below this a workgroup's 16 Q atomic adds a voxel cost more than its frames
constexpr int TS_TARGET_BLOCKS = 2048;
constexpr long TS_MAX_ROWS = 2147483647L;   // the counters are 32 bits wide

struct SelectPlan {
    long P;
    int Q, ntiles;
    size_t off_n, off_lo, off_rank, off_prefix, off_carry, off_hist, bytes;
};

int select_plan(const char *fn, const int *sz, int nq, SelectPlan &g) {
    DNMF_REQUIRE(sz, DNMF_E_NULL, "%s: sz is NULL", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(nq >= 1 && nq <= TS_MAXQ, DNMF_E_SHAPE, "%s: %d quantiles, 1 to %d a call", fn, nq, TS_MAXQ);
    g.P = (long)sz[0] * sz[1] * sz[2], g.Q = nq;
    DNMF_REQUIRE(g.P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, g.P);
    g.ntiles = (int)((g.P + TS_V - 1) / TS_V);
    const size_t P = (size_t)g.P, word = align256(P * 4), perq = align256((size_t)nq * P * 4);
    g.off_n = 0;
    g.off_lo = g.off_n + word;
    g.off_rank = g.off_lo + perq;
    g.off_prefix = g.off_rank + perq;
    g.off_carry = g.off_prefix + perq;
    g.off_hist = g.off_carry + word;
    g.bytes = g.off_hist + align256((size_t)nq * TS_BINS * P * 4);
    return DNMF_OK;
}

struct SelectArgs {
    const float *frames, *centre, *carry;
    long ldf, P;
    const int *frame_ids;
    int B, j0, seglen;       // terms j0 .. B - 1 of the call, seglen of them a workgroup
    int nh;                  // histograms a voxel: 1 in the top pass (no prefix yet), else Q
    int Q, shift;
    uint32_t mask;           // the key bits above the digit of this pass
    const uint32_t *prefix;  // (Q, P)
    uint32_t *hist;          // (Q, 16, P); the pair pass: count(x <= a_lo) (Q, P), then min{x > a_lo} (Q, P)
};

// The samples f0 .. f1 - 1 of voxel v in the order of the rows: fn(key, kept)
template <int SRC, typename F>
__device__ __forceinline__ void for_samples(const SelectArgs &a, int f0, int f1, long v, F fn) {
    auto row = [&](int j) { return a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf; };
    const float c = SRC == DNMF_SELECT_ABSDEV ? a.centre[v] : 0.0f;
    float prev = 0.0f;
    if (SRC == DNMF_SELECT_ABSDIFF) prev = f0 == 0 ? a.carry[v] : row(f0 - 1)[v];
    auto take = [&](float y) {
        float x = y;
        if (SRC == DNMF_SELECT_ABSDEV) x = fabsf(__fsub_rn(y, c));
        if (SRC == DNMF_SELECT_ABSDIFF) x = fabsf(__fsub_rn(y, prev)), prev = y;
        fn(to_key32(x), (bool)__builtin_isfinite(x));
    };
    int f = f0;
    for (; f + TS_UNROLL <= f1; f += TS_UNROLL) {
        float y[TS_UNROLL];
#pragma unroll
        for (int k = 0; k < TS_UNROLL; ++k) y[k] = row(f + k)[v];
#pragma unroll
        for (int k = 0; k < TS_UNROLL; ++k) take(y[k]);
    }
    for (; f < f1; ++f) take(row(f)[v]);
}

template <int SRC>
__global__ __launch_bounds__(TS_V) void select_count_kernel(SelectArgs a) {
    extern __shared__ uint32_t cnt[];   // (nh, 16, TS_V): column tid belongs to this thread alone
    const int tid = threadIdx.x;
    const long v0 = (long)blockIdx.x * TS_V + tid;
    const bool live = v0 < a.P;
    const long v = live ? v0 : a.P - 1;   // a lane past the volume reads the last voxel and adds nothing
    const int f0 = a.j0 + (int)blockIdx.y * a.seglen, f1 = min(a.B, f0 + a.seglen);
    for (int i = 0; i < a.nh * TS_BINS; ++i) cnt[i * TS_V + tid] = 0;
    uint32_t pre[TS_MAXQ];
#pragma unroll
    for (int q = 0; q < TS_MAXQ; ++q) pre[q] = q < a.nh && a.mask ? a.prefix[(size_t)q * a.P + v] : 0u;
    const int shift = a.shift, nh = a.nh;
    const uint32_t mask = a.mask;
    for_samples<SRC>(a, f0, f1, v, [&](uint32_t key, bool kept) {
        const int digit = (int)((key >> shift) & (TS_BINS - 1));
#pragma unroll
        for (int q = 0; q < TS_MAXQ; ++q)
            if (q < nh && kept && ((key ^ pre[q]) & mask) == 0) cnt[(q * TS_BINS + digit) * TS_V + tid] += 1;
    });
    if (!live) return;
    for (int i = 0; i < a.nh * TS_BINS; ++i) {
        const uint32_t c = cnt[i * TS_V + tid];
        if (c) atomicAdd(a.hist + (size_t)i * a.P + v, c);
    }
}

template <int SRC>
__global__ __launch_bounds__(TS_V) void select_pair_kernel(SelectArgs a) {
    const long v0 = (long)blockIdx.x * TS_V + threadIdx.x;
    const bool live = v0 < a.P;
    const long v = live ? v0 : a.P - 1;
    const int f0 = a.j0 + (int)blockIdx.y * a.seglen, f1 = min(a.B, f0 + a.seglen);
    uint32_t klo[TS_MAXQ], cle[TS_MAXQ], nxt[TS_MAXQ];
#pragma unroll
    for (int q = 0; q < TS_MAXQ; ++q) klo[q] = q < a.Q ? a.prefix[(size_t)q * a.P + v] : 0u, cle[q] = 0u, nxt[q] = ~0u;
    for_samples<SRC>(a, f0, f1, v, [&](uint32_t key, bool kept) {
#pragma unroll
        for (int q = 0; q < TS_MAXQ; ++q) {
            cle[q] += kept && key <= klo[q];
            if (kept && key > klo[q] && key < nxt[q]) nxt[q] = key;
        }
    });
    if (!live) return;
#pragma unroll
    for (int q = 0; q < TS_MAXQ; ++q)
        if (q < a.Q) {
            if (cle[q]) atomicAdd(a.hist + (size_t)q * a.P + v, cle[q]);
            if (nxt[q] != ~0u) atomicMin(a.hist + (size_t)(a.Q + q) * a.P + v, nxt[q]);
        }
}

struct Quantiles {
    double q[TS_MAXQ];
};

// Before the first piece of pass `pass`: the digit of pass - 1 and the rank that remains, per voxel and quantile, from the
// counters of that pass; then the counters cleared for this one.  One thread a voxel; it touches that voxel's words only.
__global__ __launch_bounds__(256) void select_open_kernel(long P, int Q, int pass, Quantiles qs, int *__restrict__ n,
                                                          uint32_t *__restrict__ lo, uint32_t *__restrict__ rank,
                                                          uint32_t *__restrict__ prefix, uint32_t *__restrict__ hist) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= P) return;
    if (pass == 0) {
        for (int q = 0; q < Q; ++q) prefix[(size_t)q * P + v] = 0u, rank[(size_t)q * P + v] = 0u, lo[(size_t)q * P + v] = 0u;
        n[v] = 0;
    } else {
        const int d = pass - 1, shift = 32 - 4 * pass;
        if (d == 0) {
            uint32_t nn = 0;
            for (int b = 0; b < TS_BINS; ++b) nn += hist[(size_t)b * P + v];
            n[v] = (int)nn;
            for (int q = 0; q < Q; ++q) {
                const uint32_t l = nn ? (uint32_t)floor(qs.q[q] * (double)(nn - 1)) : 0u;
                lo[(size_t)q * P + v] = l, rank[(size_t)q * P + v] = l;
            }
        }
        for (int q = 0; q < Q; ++q) {
            const uint32_t *h = hist + (size_t)(d == 0 ? 0 : q) * TS_BINS * P + v;
            uint32_t r = rank[(size_t)q * P + v], cum = 0, pick = 0;
            bool found = false;
            for (int b = 0; b < TS_BINS; ++b) {
                const uint32_t c = h[(size_t)b * P];
                if (!found && r - cum < c) pick = (uint32_t)b, r -= cum, found = true;
                if (!found) cum += c;
            }
            prefix[(size_t)q * P + v] |= pick << shift;
            rank[(size_t)q * P + v] = found ? r : 0u;
        }
    }
    if (pass < TS_DIGITS) {
        for (int i = 0; i < Q * TS_BINS; ++i) hist[(size_t)i * P + v] = 0u;
    } else {
        for (int q = 0; q < Q; ++q) hist[(size_t)q * P + v] = 0u, hist[(size_t)(Q + q) * P + v] = ~0u;
    }
}

__global__ __launch_bounds__(256) void select_carry_kernel(const float *__restrict__ frames, long ldf, const int *__restrict__ frame_ids,
                                                           int B, long P, float *__restrict__ carry) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < P) carry[v] = frames[(long)(frame_ids ? frame_ids[B - 1] : B - 1) * ldf + v];
}

__global__ __launch_bounds__(256) void select_finish_kernel(long P, int Q, const int *__restrict__ n, const uint32_t *__restrict__ lo,
                                                            const uint32_t *__restrict__ prefix, const uint32_t *__restrict__ hist,
                                                            float *__restrict__ a_lo, float *__restrict__ a_hi, int *__restrict__ n_out) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= P) return;
    const uint32_t nn = (uint32_t)n[v];
    n_out[v] = (int)nn;
    for (int q = 0; q < Q; ++q) {
        float x0 = __uint_as_float(0x7fc00000u), x1 = x0;
        if (nn) {
            const uint32_t l = lo[(size_t)q * P + v], hi = min(l + 1u, nn - 1u);
            const uint32_t cle = hist[(size_t)q * P + v], nxt = hist[(size_t)(Q + q) * P + v];
            x0 = from_key32(prefix[(size_t)q * P + v]);
            x1 = (hi == l || cle >= l + 2u) ? x0 : from_key32(nxt);
        }
        a_lo[(size_t)q * P + v] = x0, a_hi[(size_t)q * P + v] = x1;
    }
}

template <int SRC>
void launch_pass(const SelectArgs &a, bool pair, int ntiles, int nseg, hipStream_t st) {
    if (pair)
        hipLaunchKernelGGL((select_pair_kernel<SRC>), dim3((unsigned)ntiles, (unsigned)nseg), dim3(TS_V), 0, st, a);
    else
        hipLaunchKernelGGL((select_count_kernel<SRC>), dim3((unsigned)ntiles, (unsigned)nseg), dim3(TS_V),
                           (size_t)a.nh * TS_BINS * TS_V * sizeof(uint32_t), st, a);
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_temporal_select_passes(void) { return dnmf::TS_DIGITS + 1; }

size_t dnmf_temporal_select_workspace(const int *sz, int nq) {
    dnmf::SelectPlan g;
    if (dnmf::select_plan("dnmf_temporal_select_workspace", sz, nq, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_temporal_select_pass(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, int source,
                              const float *centre, const double *q, int nq, int pass, long rows_before, int segment, void *state,
                              size_t state_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_temporal_select_pass";
    DNMF_REQUIRE(frames && state && q, DNMF_E_NULL, "%s: NULL argument", fn);
    SelectPlan g;
    const int rc = select_plan(fn, sz, nq, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(B >= 1, DNMF_E_SHAPE, "%s: B=%d frames", fn, B);
    DNMF_REQUIRE(source == DNMF_SELECT_VALUE || source == DNMF_SELECT_ABSDEV || source == DNMF_SELECT_ABSDIFF, DNMF_E_SHAPE,
                 "%s: source=%d (0 value, 1 absdev, 2 absdiff)", fn, source);
    DNMF_REQUIRE(centre || source != DNMF_SELECT_ABSDEV, DNMF_E_NULL, "%s: source absdev needs a centre image", fn);
    DNMF_REQUIRE(pass >= 0 && pass <= TS_DIGITS, DNMF_E_SHAPE, "%s: pass=%d of %d", fn, pass, TS_DIGITS + 1);
    DNMF_REQUIRE(ldf >= g.P, DNMF_E_SHAPE, "%s: ldf=%ld below a row of P=%ld", fn, ldf, g.P);
    DNMF_REQUIRE(rows_before >= 0 && rows_before <= TS_MAX_ROWS - B, DNMF_E_UNSUPPORTED,
                 "%s: %ld + %d rows, at most %ld (32-bit counters)", fn, rows_before, B, TS_MAX_ROWS);
    Quantiles qs = {};
    for (int i = 0; i < nq; ++i) {
        DNMF_REQUIRE(q[i] >= 0.0 && q[i] <= 1.0, DNMF_E_SHAPE, "%s: q[%d]=%g outside [0, 1]", fn, i, q[i]);
        qs.q[i] = q[i];
    }
    DNMF_REQUIRE(state_bytes >= g.bytes, DNMF_E_WORKSPACE, "%s: state of %zu bytes, need %zu", fn, state_bytes, g.bytes);
    DNMF_REQUIRE(((size_t)state & 3) == 0, DNMF_E_WORKSPACE, "%s: state must be 4-byte aligned", fn);
    // the terms of the call: the first row of a movie has no difference to its predecessor
    const int j0 = source == DNMF_SELECT_ABSDIFF && rows_before == 0 ? 1 : 0;
    SegmentPlan sp = {};
    if (B > j0) {
        const int src = segment_plan(fn, B - j0, segment, g.ntiles, TS_TARGET_BLOCKS, TS_MIN_SEGMENT, sp);
        if (src != DNMF_OK) return src;
    }
    char *w = static_cast<char *>(state);
    int *n = reinterpret_cast<int *>(w + g.off_n);
    uint32_t *lo = reinterpret_cast<uint32_t *>(w + g.off_lo), *rank = reinterpret_cast<uint32_t *>(w + g.off_rank);
    uint32_t *prefix = reinterpret_cast<uint32_t *>(w + g.off_prefix), *hist = reinterpret_cast<uint32_t *>(w + g.off_hist);
    float *carry = reinterpret_cast<float *>(w + g.off_carry);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned vblocks = (unsigned)((g.P + 255) / 256);
    if (rows_before == 0) hipLaunchKernelGGL(select_open_kernel, dim3(vblocks), dim3(256), 0, st, g.P, nq, pass, qs, n, lo, rank, prefix, hist);
    if (B > j0) {
        SelectArgs a;
        a.frames = frames, a.centre = centre, a.carry = carry, a.ldf = ldf, a.P = g.P, a.frame_ids = frame_ids;
        a.B = B, a.j0 = j0, a.seglen = sp.seglen;
        a.nh = pass == 0 ? 1 : nq, a.Q = nq, a.shift = pass < TS_DIGITS ? 28 - 4 * pass : 0;
        a.mask = pass == 0 ? 0u : (0xffffffffu << (32 - 4 * pass));
        a.prefix = prefix, a.hist = hist;
        const bool pair = pass == TS_DIGITS;
        if (source == DNMF_SELECT_VALUE) launch_pass<DNMF_SELECT_VALUE>(a, pair, g.ntiles, sp.nseg, st);
        else if (source == DNMF_SELECT_ABSDEV) launch_pass<DNMF_SELECT_ABSDEV>(a, pair, g.ntiles, sp.nseg, st);
        else launch_pass<DNMF_SELECT_ABSDIFF>(a, pair, g.ntiles, sp.nseg, st);
    }
    if (source == DNMF_SELECT_ABSDIFF) {
        // the last row of the piece, for the first term of the next one: after the pass kernel, which read the old one
        hipLaunchKernelGGL(select_carry_kernel, dim3(vblocks), dim3(256), 0, st, frames, ldf, frame_ids, B, g.P, carry);
    }
    return check_launch(fn);
}

int dnmf_temporal_select_finish(const int *sz, int nq, const void *state, size_t state_bytes, float *lo, float *hi, int *n,
                                dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_temporal_select_finish";
    DNMF_REQUIRE(state && lo && hi && n, DNMF_E_NULL, "%s: NULL argument", fn);
    SelectPlan g;
    const int rc = select_plan(fn, sz, nq, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(state_bytes >= g.bytes, DNMF_E_WORKSPACE, "%s: state of %zu bytes, need %zu", fn, state_bytes, g.bytes);
    const char *w = static_cast<const char *>(state);
    hipLaunchKernelGGL(select_finish_kernel, dim3((unsigned)((g.P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g.P, nq,
                       reinterpret_cast<const int *>(w + g.off_n), reinterpret_cast<const uint32_t *>(w + g.off_lo),
                       reinterpret_cast<const uint32_t *>(w + g.off_prefix), reinterpret_cast<const uint32_t *>(w + g.off_hist), lo, hi, n);
    return check_launch(fn);
}

}  // extern "C"
