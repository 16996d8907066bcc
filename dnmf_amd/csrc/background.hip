// K19: a rank-1 background b (x) f fitted on the residual r = frames - sub by alternating exact coordinate steps (rank-1
// HALS), and its subtraction.  include/dnmf_hip.h has the contracts, tests/background_restatement.py the definition in float64.
//
// Both half-steps are one pass over the movie that subtracts as it reads (8 B per voxel and frame with sub, 4 B without; the
// residual is never written), in float64: r = (double)y - (double)m is exact, the products and sums are float64.
//   dots    f_j = max(0, sum_p b_p r_jp) / sum_p b_p^2: a workgroup owns a frame and a segment of contiguous voxels, every lane
//           keeps float64 sums, the wave and then the workgroup reduce them in a fixed tree, a second launch adds a frame's
//           segments in their order.  The workgroups of the call's first frame also sum b^2 over their segment.
//   accum   b_p = max(0, sum_t f_t r_tp) / sum_t f_t^2: a workgroup owns a tile of BG_TILE contiguous voxels (four per lane) and a
//           segment of frames; the sums live in registers, f_t is a uniform load.  A second launch adds the segments to the
//           caller's state in their order, a third writes b.
// No floating-point atomics: the same input at the same addresses gives the same bits.
//
// K23: the same two passes for R images and R time courses (2 <= R <= 8) with R sums where K19 has one, the R x R Gram matrix of the
// factor held fixed from a launch of its own, and a per-frame (per-voxel) non-negative solve by coordinate sweeps in the finishing
// launch; tests/background_rank_restatement.py is its definition.
//
// One skeleton, two policies.  What walks the movie is written once: the workgroup prologues, the head / 16-byte body / tail walk of
// a dots segment (segment_walk), the accumulate kernel (K19 runs its R = 1 instantiation), the reduction of the accumulate partials,
// and the tile prologue, clamp, NaN row and store of the subtraction.  What the families do with a residual stays their own, because
// it decides the bits: K19's dots keep four float64 sums a lane (head, body x y z w, tail) and sum b^2 beside them, K23's one sum per
// component; K19 subtracts with one fp32 fmaf, K23 with float64 products added c ascending; K19 finishes in closed form, K23 by sweeps.
#include <cstdint>

#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int BG_THREADS = 256, BG_WAVES = BG_THREADS / 64;
constexpr int BG_TILE = 4 * BG_THREADS;          // voxels of a workgroup of accum and subtract: one float4 a lane
constexpr long BG_DOTS_MIN_SEG = BG_TILE;        // voxels: a segment of dots is a multiple of this
constexpr int BG_DOTS_TARGET_BLOCKS = 4096;
constexpr int BG_ACC_MIN_SEGMENT = 16;           // frames: below this the partial sums cost more traffic than the frames
constexpr int BG_ACC_TARGET_BLOCKS = 2048;
constexpr size_t BG_HEADER = 256;                // bytes: sum f^2

__device__ __forceinline__ unsigned word_phase(const void *p) { return (unsigned)(((uintptr_t)p >> 2) & 3); }

// ---- dots ----------------------------------------------------------------------------------------------------------------------
struct DotsPlan {
    long seglen;
    int nseg;
    size_t off_bb, bytes;   // part (B, nseg) float64, then the nseg sums of b^2
};

int dots_plan(const char *fn, long P, int B, DotsPlan &g) {
    DNMF_REQUIRE(P >= 1 && B >= 1, DNMF_E_SHAPE, "%s: P=%ld voxels, B=%d frames", fn, P, B);
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    long want = (BG_DOTS_TARGET_BLOCKS + (long)B - 1) / B;
    const long most = (P + BG_DOTS_MIN_SEG - 1) / BG_DOTS_MIN_SEG;
    if (want > most) want = most;
    const long len = (P + want - 1) / want;
    g.seglen = (len + BG_DOTS_MIN_SEG - 1) / BG_DOTS_MIN_SEG * BG_DOTS_MIN_SEG;
    g.nseg = (int)((P + g.seglen - 1) / g.seglen);
    DNMF_REQUIRE((long)B * g.nseg < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld workgroups", fn, (long)B * g.nseg);
    g.off_bb = align256((size_t)B * g.nseg * sizeof(double));
    g.bytes = g.off_bb + align256((size_t)g.nseg * sizeof(double));
    return DNMF_OK;
}

struct DotsArgs {
    const float *frames, *sub, *b;
    long ldf, lds, ldb, P, seglen;   // ldb: between the R images of K23
    const int *frame_ids;
    int nseg;
    double *part, *bbpart;           // bbpart: K19
};

// The work of a dots workgroup: frame j of the call, segment s of n voxels; y, m (NULL without SUB) and b at its first voxel.
struct Segment {
    int j, s;
    long n;
    const float *y, *m, *b;
};

template <bool SUB>
__device__ __forceinline__ Segment dots_segment(const DotsArgs &a) {
    const long bid = blockIdx.x;
    Segment g;
    g.j = (int)(bid / a.nseg), g.s = (int)(bid - (long)g.j * a.nseg);
    const long p0 = (long)g.s * a.seglen;
    g.n = (a.P - p0 < a.seglen ? a.P - p0 : a.seglen);
    g.y = a.frames + (long)(a.frame_ids ? a.frame_ids[g.j] : g.j) * a.ldf + p0;
    g.m = SUB ? a.sub + (long)g.j * a.lds + p0 : nullptr;
    g.b = a.b + p0;
    return g;
}

template <bool SUB>
__device__ __forceinline__ double residual(float y, float m) { return SUB ? (double)y - (double)m : (double)y; }

// The walk of a segment, the residuals r = y - m handed on in float64.  16-byte loads from the first voxel at which y, m and the R
// rows of b (ldb floats apart) are all aligned; rows whose starts differ in phase (P % 4 != 0 against the aligned b) are read one
// float at a time.  one(i, r, slot): voxel i of the segment, slot 0 before the 16-byte body and 1 behind it.  four(head, i, r0 .. r3):
// the voxels head + 4 i .. head + 4 i + 3, for the caller's own 16-byte load of float4 i of every (b row + head).
template <bool SUB, int R, typename One, typename Four>
__device__ __forceinline__ void segment_walk(const Segment &g, long ldb, One &&one, Four &&four) {
    const int tid = threadIdx.x;
    const float *__restrict__ y = g.y, *__restrict__ m = g.m;
    const unsigned ph = word_phase(y);
    bool vec = !SUB || word_phase(m) == ph;
#pragma unroll
    for (int c = 0; c < R; ++c) vec = vec && word_phase(g.b + (long)c * ldb) == ph;
    long head = vec ? (long)((4 - ph) & 3) : g.n;
    if (head > g.n) head = g.n;
    const long n4 = (g.n - head) >> 2;
    for (long i = tid; i < head; i += BG_THREADS) one(i, residual<SUB>(y[i], SUB ? m[i] : 0.0f), 0);
    const float4 *y4 = reinterpret_cast<const float4 *>(y + head);
    const float4 *m4 = SUB ? reinterpret_cast<const float4 *>(m + head) : nullptr;
#pragma unroll 2
    for (long i = tid; i < n4; i += BG_THREADS) {
        const float4 yv = y4[i];
        const float4 mv = SUB ? m4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        four(head, i, residual<SUB>(yv.x, mv.x), residual<SUB>(yv.y, mv.y), residual<SUB>(yv.z, mv.z), residual<SUB>(yv.w, mv.w));
    }
    for (long i = head + 4 * n4 + tid; i < g.n; i += BG_THREADS) one(i, residual<SUB>(y[i], SUB ? m[i] : 0.0f), 1);
}

// K19: four float64 sums a lane -- the head in slot 0, the body in slots x y z w, the tail in slot 1 -- as (a0 + a1) + (a2 + a3);
// WITH_BB: b^2 beside them in the same way.
template <bool SUB, bool WITH_BB>
__device__ __forceinline__ void dots_sums(const Segment &g, double &sum, double &sumq) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    auto term = [&](float b, double r, int k) {
        const double bd = (double)b;
        acc[k] = fma(bd, r, acc[k]);
        if (WITH_BB) q[k] = fma(bd, bd, q[k]);
    };
    segment_walk<SUB, 1>(
        g, 0, [&](long i, double r, int slot) { term(g.b[i], r, slot); },
        [&](long head, long i, double r0, double r1, double r2, double r3) {
            const float4 bv = reinterpret_cast<const float4 *>(g.b + head)[i];
            term(bv.x, r0, 0), term(bv.y, r1, 1), term(bv.z, r2, 2), term(bv.w, r3, 3);
        });
    sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    sumq = (q[0] + q[1]) + (q[2] + q[3]);
}

template <bool SUB>
__global__ __launch_bounds__(BG_THREADS) void background_dots_kernel(DotsArgs a) {
    __shared__ double red[2 * BG_WAVES];
    const Segment g = dots_segment<SUB>(a);
    double sum, sumq;
    if (g.j == 0) {   // the first frame's workgroups also sum b^2 over their segment
        dots_sums<SUB, true>(g, sum, sumq);
        const double tq = block_sum0<BG_THREADS>(sumq, red + BG_WAVES);
        if (threadIdx.x == 0) a.bbpart[g.s] = tq;
    } else {
        dots_sums<SUB, false>(g, sum, sumq);
    }
    const double t = block_sum0<BG_THREADS>(sum, red);
    if (threadIdx.x == 0) a.part[blockIdx.x] = t;
}

// num_j = the segments of frame j in their order; bb = the segments of b^2 in their order (every thread the same sum)
__global__ __launch_bounds__(BG_THREADS) void background_dots_finish_kernel(const double *__restrict__ part, const double *__restrict__ bbpart,
                                                                            int nseg, int B, double *__restrict__ num, double *__restrict__ bb,
                                                                            float *__restrict__ f) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    double q = 0.0;
    for (int s = 0; s < nseg; ++s) q += bbpart[s];
    double acc = 0.0;
    for (int s = 0; s < nseg; ++s) acc += part[(long)j * nseg + s];
    if (num) num[j] = acc;
    f[j] = q > 0.0 ? (float)(fmax(0.0, acc) / q) : 0.0f;
    if (j == 0 && bb) *bb = q;
}

// ---- accum ---------------------------------------------------------------------------------------------------------------------
struct AccumPlan : SegmentPlan {
    long ntiles;
    size_t stride;   // doubles of one (P,) array
    size_t off_sums, off_part, bytes;
};

int accum_plan(const char *fn, long P, int B, int segment, AccumPlan &g) {
    DNMF_REQUIRE(P >= 1 && B >= 1, DNMF_E_SHAPE, "%s: P=%ld voxels, B=%d frames", fn, P, B);
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    g.ntiles = (P + BG_TILE - 1) / BG_TILE;
    const int rc = segment_plan(fn, B, segment, g.ntiles, BG_ACC_TARGET_BLOCKS, BG_ACC_MIN_SEGMENT, g);
    if (rc != DNMF_OK) return rc;
    const size_t arr = align256((size_t)P * sizeof(double));
    g.stride = arr / sizeof(double);
    g.off_sums = BG_HEADER;
    g.off_part = g.off_sums + arr;
    g.bytes = g.off_part + (size_t)g.cap * arr;
    return DNMF_OK;
}

// The `live` (1..4) floats at row + p, p a multiple of 4, zeros beyond: one 16-byte load where the row start allows it.
__device__ __forceinline__ float4 load4(const float *__restrict__ row, long p, int live) {
    if (live == 4 && word_phase(row) == 0) return *reinterpret_cast<const float4 *>(row + p);
    float4 v;
    v.x = row[p];
    v.y = live > 1 ? row[p + 1] : 0.0f;
    v.z = live > 2 ? row[p + 2] : 0.0f;
    v.w = live > 3 ? row[p + 3] : 0.0f;
    return v;
}

struct AccumRankArgs {
    const float *frames, *sub, *f;
    long ldf, lds, ldf_t, P;   // ldf_t: between the R time courses
    const int *frame_ids;
    int B, seglen;
    double *part;
    size_t stride;
};

// part[segment][c][p] = sum over the segment's frames of f_c[t] (y - m): four voxels a lane, 4 R float64 sums in registers.  Both
// families: K19 is R = 1.
template <int R, bool SUB>
__global__ __launch_bounds__(BG_THREADS) void background_accum_rank_kernel(AccumRankArgs a) {
    const long p = (long)blockIdx.x * BG_TILE + 4 * (long)threadIdx.x;
    if (p >= a.P) return;
    const int live = a.P - p >= 4 ? 4 : (int)(a.P - p);
    const int seg = blockIdx.y;
    const int f0 = seg * a.seglen, f1 = min(a.B, f0 + a.seglen);
    double s[R][4];
#pragma unroll
    for (int c = 0; c < R; ++c) s[c][0] = s[c][1] = s[c][2] = s[c][3] = 0.0;
#pragma unroll 2
    for (int j = f0; j < f1; ++j) {
        const float4 y = load4(a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf, p, live);
        double r0 = (double)y.x, r1 = (double)y.y, r2 = (double)y.z, r3 = (double)y.w;
        if (SUB) {
            const float4 m = load4(a.sub + (long)j * a.lds, p, live);
            r0 -= (double)m.x, r1 -= (double)m.y, r2 -= (double)m.z, r3 -= (double)m.w;
        }
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const double fc = (double)a.f[(long)c * a.ldf_t + j];
            s[c][0] = fma(fc, r0, s[c][0]);
            s[c][1] = fma(fc, r1, s[c][1]);
            s[c][2] = fma(fc, r2, s[c][2]);
            s[c][3] = fma(fc, r3, s[c][3]);
        }
    }
#pragma unroll
    for (int c = 0; c < R; ++c) {
        double *out = a.part + ((size_t)seg * R + c) * a.stride + p;
        out[0] = s[c][0];
        if (live > 1) out[1] = s[c][1];
        if (live > 2) out[2] = s[c][2];
        if (live > 3) out[3] = s[c][3];
    }
}

// sums[c][p] = (first ? 0 : sums[c][p]) + the segments in their order; c rides on gridDim.y.  With f (K19, R = 1) workgroup 0 also
// leaves ff = (first ? 0 : ff) + sum f^2 of the call (fixed tree); K23 passes NULL and has its Gram launch.
__global__ __launch_bounds__(BG_THREADS) void background_accum_reduce_kernel(const double *__restrict__ part, size_t stride, int nseg, int R,
                                                                             long P, int first, double *__restrict__ sums,
                                                                             const float *__restrict__ f, int B, double *__restrict__ ff) {
    __shared__ double red[BG_WAVES];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (i < P) {
        double acc = first ? 0.0 : sums[(size_t)c * stride + i];
        for (int s = 0; s < nseg; ++s) acc += part[((size_t)s * R + c) * stride + i];
        sums[(size_t)c * stride + i] = acc;
    }
    if (f && blockIdx.x == 0) {
        double q = 0.0;
        for (int j = threadIdx.x; j < B; j += BG_THREADS) {
            const double v = (double)f[j];
            q = fma(v, v, q);
        }
        const double t = block_sum0<BG_THREADS>(q, red);
        if (threadIdx.x == 0) *ff = (first ? 0.0 : *ff) + t;
    }
}

__global__ __launch_bounds__(BG_THREADS) void background_accum_finish_kernel(const double *__restrict__ sums, const double *__restrict__ ff,
                                                                             long P, float *__restrict__ b, double *__restrict__ num,
                                                                             double *__restrict__ ff_out) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double q = *ff, v = sums[p];
    if (num) num[p] = v;
    b[p] = q > 0.0 ? (float)(fmax(0.0, v) / q) : 0.0f;
    if (p == 0 && ff_out) *ff_out = q;
}

// ---- subtract ------------------------------------------------------------------------------------------------------------------
struct SubtractArgs {
    const float *frames, *b, *f;
    long ldf, ldo, ldb, ldf_t, P, ntiles;
    const int *frame_ids, *times;
    int nf, clamp, R;
    float *out;
};

// `live` (1..4) floats to o + p, p a multiple of 4: one 16-byte store where the row start allows it.
__device__ __forceinline__ void store4(float *__restrict__ o, long p, int live, float4 r) {
    if (live == 4 && word_phase(o) == 0) {
        *reinterpret_cast<float4 *>(o + p) = r;
        return;
    }
    o[p] = r.x;
    if (live > 1) o[p + 1] = r.y;
    if (live > 2) o[p + 2] = r.z;
    if (live > 3) o[p + 3] = r.w;
}

// K19 (RANK false): out = fmaf(-b, f[t], y), one fp32 fused multiply-add.  K23: out = (float)((double)y - sum_c (double)b_c (double)f_c[t]),
// the products added one by one, c ascending.
template <bool RANK>
__global__ __launch_bounds__(BG_THREADS) void background_subtract_kernel(SubtractArgs a) {
    const long bid = blockIdx.x;
    const int j = (int)(bid / a.ntiles);
    const long p = (bid - (long)j * a.ntiles) * BG_TILE + 4 * (long)threadIdx.x;
    if (p >= a.P) return;
    const int live = a.P - p >= 4 ? 4 : (int)(a.P - p);
    const int t = a.times ? a.times[j] : j;
    const bool known = t >= 0 && t < a.nf;
    const float4 y = load4(a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf, p, live);
    float4 r;
    if (RANK) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (known)
            for (int c = 0; c < a.R; ++c) {
                const double fc = (double)a.f[(long)c * a.ldf_t + t];
                const float4 b = load4(a.b + (long)c * a.ldb, p, live);
                s0 = s0 + (double)b.x * fc, s1 = s1 + (double)b.y * fc, s2 = s2 + (double)b.z * fc, s3 = s3 + (double)b.w * fc;
            }
        r.x = (float)((double)y.x - s0), r.y = (float)((double)y.y - s1), r.z = (float)((double)y.z - s2), r.w = (float)((double)y.w - s3);
    } else {
        const float fj = known ? a.f[t] : 0.0f;
        const float4 b = load4(a.b, p, live);
        r.x = fmaf(-b.x, fj, y.x), r.y = fmaf(-b.y, fj, y.y), r.z = fmaf(-b.z, fj, y.z), r.w = fmaf(-b.w, fj, y.w);
    }
    if (a.clamp) r.x = fmaxf(r.x, 0.0f), r.y = fmaxf(r.y, 0.0f), r.z = fmaxf(r.z, 0.0f), r.w = fmaxf(r.w, 0.0f);
    // a time f has no entry for: the row becomes NaN instead of reading beyond f (after the clamp: fmaxf drops a NaN)
    if (!known) r.x = r.y = r.z = r.w = __builtin_nanf("");
    store4(a.out + (long)j * a.ldo, p, live, r);
}

// ---- K23: rank R ---------------------------------------------------------------------------------------------------------------
// R images b_c (rows of ldb floats) and R time courses f_c (rows of ldf_t floats), 2 <= R <= 8, R a template parameter so that the
// R sums of a lane are registers.  A half-step is still one pass over the movie: the pass leaves R sums per frame (per voxel), a
// small launch leaves the R x R Gram matrix of the factor held fixed, and the last launch solves every frame's (voxel's) R-variable
// non-negative problem by `inner` cyclic coordinate sweeps in float64 from its current value, the Gram matrix in LDS.
constexpr int BGR_MIN = 2, BGR_MAX = 8;
constexpr long BG_GRAM_CHUNK = 4096;             // elements of a workgroup of the Gram launch
constexpr size_t BGR_HEADER = 512;               // bytes: the R x R Gram matrix, float64, row-major

__host__ __device__ constexpr int tri_at(int j, int i) { return j * (j + 1) / 2 + i; }   // (j, i), i <= j, in the packed triangle

// x_j <- max(0, (N_j - sum_{i != j} G_ji x_i) / G_jj), 0 where G_jj == 0, j = 0 .. R-1, `inner` times; the products and
// differences one by one, i ascending (tests/background_rank_restatement.py: sweep does the same operations in the same order)
template <int R>
__device__ __forceinline__ void bg_sweep(const double *G, const double (&N)[R], double (&x)[R], int inner) {
    for (int it = 0; it < inner; ++it) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            double s = N[j];
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (i != j) s = s - G[j * R + i] * x[i];
            const double d = G[j * R + j];
            x[j] = d != 0.0 ? fmax(0.0, s / d) : 0.0;
        }
    }
}

// The packed lower triangle of X X^T over a chunk of the n columns of the R rows x (ld floats apart): one partial per workgroup.
template <int R>
__global__ __launch_bounds__(BG_THREADS) void background_gram_kernel(const float *__restrict__ x, long ld, long n, double *__restrict__ part) {
    constexpr int NT = R * (R + 1) / 2;
    __shared__ double red[BG_WAVES][NT];
    const long i0 = (long)blockIdx.x * BG_GRAM_CHUNK;
    const long i1 = n - i0 < BG_GRAM_CHUNK ? n : i0 + BG_GRAM_CHUNK;
    double acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += BG_THREADS) {
        double v[R];
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = (double)x[(long)j * ld + i];
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int c = 0; c <= j; ++c) acc[tri_at(j, c)] = fma(v[j], v[c], acc[tri_at(j, c)]);
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const double s = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NT) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < BG_WAVES; ++w) s += red[w][threadIdx.x];
        part[(long)blockIdx.x * NT + threadIdx.x] = s;
    }
}

// G (R x R, both triangles) = (first ? 0 : G) + the chunks in their order
template <int R>
__global__ __launch_bounds__(64) void background_gram_reduce_kernel(const double *__restrict__ part, long nchunks, int first, double *G) {
    constexpr int NT = R * (R + 1) / 2;
    const int k = threadIdx.x;
    if (k >= R * R) return;
    const int j = k / R, i = k - j * R;
    const int t = j >= i ? tri_at(j, i) : tri_at(i, j);
    double s = first ? 0.0 : G[k];
    for (long c = 0; c < nchunks; ++c) s += part[c * NT + t];
    G[k] = s;
}

// part[(frame, segment)][c] = sum over the segment's voxels of b_c (y - m): one float64 sum per component and lane
template <int R, bool SUB>
__global__ __launch_bounds__(BG_THREADS) void background_dots_rank_kernel(DotsArgs a) {
    __shared__ double red[BG_WAVES][R];
    const int tid = threadIdx.x;
    const Segment g = dots_segment<SUB>(a);
    double acc[R];
#pragma unroll
    for (int c = 0; c < R; ++c) acc[c] = 0.0;
    segment_walk<SUB, R>(
        g, a.ldb,
        [&](long i, double r, int) {
#pragma unroll
            for (int c = 0; c < R; ++c) acc[c] = fma((double)g.b[(long)c * a.ldb + i], r, acc[c]);
        },
        [&](long head, long i, double r0, double r1, double r2, double r3) {
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const float4 bv = reinterpret_cast<const float4 *>(g.b + (long)c * a.ldb + head)[i];
                acc[c] = fma((double)bv.x, r0, acc[c]);
                acc[c] = fma((double)bv.y, r1, acc[c]);
                acc[c] = fma((double)bv.z, r2, acc[c]);
                acc[c] = fma((double)bv.w, r3, acc[c]);
            }
        });
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const double v = wave_sum(acc[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = v;
    }
    __syncthreads();
    if (tid < R) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < BG_WAVES; ++w) t += red[w][tid];
        a.part[(long)blockIdx.x * R + tid] = t;
    }
}

// Per frame: N_c = the segments in their order, then the sweeps from the frame's current f; num is (R, B), q_out the Gram matrix
template <int R>
__global__ __launch_bounds__(BG_THREADS) void background_dots_rank_finish_kernel(const double *__restrict__ part, const double *__restrict__ Q,
                                                                                 int nseg, int B, int inner, float *f, long ldf_t,
                                                                                 double *__restrict__ num, double *__restrict__ q_out) {
    __shared__ double G[R * R];
    if (threadIdx.x < R * R) G[threadIdx.x] = Q[threadIdx.x];
    __syncthreads();
    if (blockIdx.x == 0 && q_out && threadIdx.x < R * R) q_out[threadIdx.x] = G[threadIdx.x];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    double N[R], x[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        double acc = 0.0;
        for (int s = 0; s < nseg; ++s) acc += part[((long)t * nseg + s) * R + c];
        N[c] = acc;
        x[c] = (double)f[(long)c * ldf_t + t];
        if (num) num[(long)c * B + t] = acc;
    }
    bg_sweep<R>(G, N, x, inner);
#pragma unroll
    for (int c = 0; c < R; ++c) f[(long)c * ldf_t + t] = (float)x[c];
}

// Per voxel: the sweeps from the voxel's current b with W in LDS; num is (R, P), w_out the Gram matrix
template <int R>
__global__ __launch_bounds__(BG_THREADS) void background_accum_rank_finish_kernel(const double *__restrict__ sums, size_t stride,
                                                                                  const double *__restrict__ W, long P, int inner, float *b,
                                                                                  long ldb, double *__restrict__ num, double *__restrict__ w_out) {
    __shared__ double G[R * R];
    if (threadIdx.x < R * R) G[threadIdx.x] = W[threadIdx.x];
    __syncthreads();
    if (blockIdx.x == 0 && w_out && threadIdx.x < R * R) w_out[threadIdx.x] = G[threadIdx.x];
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double N[R], x[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        N[c] = sums[(size_t)c * stride + p];
        x[c] = (double)b[(long)c * ldb + p];
        if (num) num[(long)c * P + p] = N[c];
    }
    bg_sweep<R>(G, N, x, inner);
#pragma unroll
    for (int c = 0; c < R; ++c) b[(long)c * ldb + p] = (float)x[c];
}

// ---- what the entries share ----------------------------------------------------------------------------------------------------
unsigned lane_blocks(long n) { return (unsigned)((n + BG_THREADS - 1) / BG_THREADS); }   // workgroups of a launch with one element a lane

// `what`: "workspace" or "state", as the entry's texts call it
int check_workspace(const char *fn, const char *what, const void *ws, size_t bytes, size_t need) {
    DNMF_REQUIRE(bytes >= need, DNMF_E_WORKSPACE, "%s: %s of %zu bytes, need %zu", fn, what, bytes, need);
    DNMF_REQUIRE(((size_t)ws & 7) == 0, DNMF_E_WORKSPACE, "%s: %s must be 8-byte aligned", fn, what);
    return DNMF_OK;
}

int rank_check(const char *fn, int R, int inner) {
    DNMF_REQUIRE(R >= BGR_MIN && R <= BGR_MAX, DNMF_E_UNSUPPORTED, "%s: R=%d components (%d .. %d; one component is K19's entry)", fn, R, BGR_MIN,
                 BGR_MAX);
    DNMF_REQUIRE(inner >= 1, DNMF_E_SHAPE, "%s: inner=%d sweeps", fn, inner);
    return DNMF_OK;
}

// Both subtractions: K19 is R = 1 with the one fmaf (RANK false: no rows of b or f in its texts), K23 checks its R first.
template <bool RANK>
int subtract(const char *fn, const float *frames, long ldf, const int *frame_ids, const float *b, long ldb, const float *f, long ldf_t, int R, int nf,
             const int *times, long P, int B, float *out, long ldo, int clamp, dnmf_stream_t stream) {
    DNMF_REQUIRE(frames && b && f && out, DNMF_E_NULL, "%s: NULL argument", fn);
    if (RANK) {
        const int rc = rank_check(fn, R, 1);
        if (rc != DNMF_OK) return rc;
    }
    DNMF_REQUIRE(P >= 1 && B >= 1 && nf >= 1, DNMF_E_SHAPE, "%s: P=%ld voxels, B=%d frames, nf=%d", fn, P, B, nf);
    if (RANK) {
        DNMF_REQUIRE(ldf >= P && ldo >= P && ldb >= P, DNMF_E_SHAPE, "%s: ldf=%ld ldo=%ld ldb=%ld below a row of P=%ld", fn, ldf, ldo, ldb, P);
        DNMF_REQUIRE(ldf_t >= nf, DNMF_E_SHAPE, "%s: ldf_t=%ld below a row of nf=%d", fn, ldf_t, nf);
    } else {
        DNMF_REQUIRE(ldf >= P && ldo >= P, DNMF_E_SHAPE, "%s: ldf=%ld ldo=%ld below a row of P=%ld", fn, ldf, ldo, P);
    }
    DNMF_REQUIRE(times || B <= nf, DNMF_E_SHAPE, "%s: B=%d frames but f has %d values and times is NULL", fn, B, nf);
    DNMF_REQUIRE(out != frames || (!frame_ids && ldo == ldf), DNMF_E_SHAPE, "%s: in place (out == frames) needs frame_ids NULL and ldo == ldf", fn);
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    SubtractArgs a;
    a.frames = frames, a.b = b, a.f = f, a.ldf = ldf, a.ldo = ldo, a.ldb = ldb, a.ldf_t = ldf_t, a.P = P, a.ntiles = (P + BG_TILE - 1) / BG_TILE;
    a.frame_ids = frame_ids, a.times = times, a.nf = nf, a.clamp = clamp != 0, a.R = R, a.out = out;
    DNMF_REQUIRE(a.ntiles * B < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld workgroups (split the call)", fn, a.ntiles * B);
    hipLaunchKernelGGL(background_subtract_kernel<RANK>, dim3((unsigned)(a.ntiles * B)), dim3(BG_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}

// ---- K23: the plans and the launches by R --------------------------------------------------------------------------------------
size_t gram_bytes(long n, int R) { return align256((size_t)((n + BG_GRAM_CHUNK - 1) / BG_GRAM_CHUNK) * (R * (R + 1) / 2) * sizeof(double)); }

struct DotsRankPlan {
    DotsPlan d;
    size_t off_gram, off_part, bytes;   // Q at 0, the chunks of the Gram launch, part (B, nseg, R) float64
};

int dots_rank_plan(const char *fn, long P, int B, int R, DotsRankPlan &g) {
    int rc = rank_check(fn, R, 1);
    if (rc != DNMF_OK) return rc;
    rc = dots_plan(fn, P, B, g.d);
    if (rc != DNMF_OK) return rc;
    g.off_gram = BGR_HEADER;
    g.off_part = g.off_gram + gram_bytes(P, R);
    g.bytes = g.off_part + align256((size_t)B * g.d.nseg * R * sizeof(double));
    return DNMF_OK;
}

struct AccumRankPlan {
    AccumPlan a;
    size_t off_sums, off_part, off_gram, bytes;   // W at 0 and sums (R, stride) persist between the calls; part and the chunks do not
};

int accum_rank_plan(const char *fn, long P, int B, int R, int segment, AccumRankPlan &g) {
    int rc = rank_check(fn, R, 1);
    if (rc != DNMF_OK) return rc;
    rc = accum_plan(fn, P, B, segment, g.a);
    if (rc != DNMF_OK) return rc;
    const size_t arr = g.a.stride * sizeof(double);
    g.off_sums = BGR_HEADER;
    g.off_part = g.off_sums + (size_t)R * arr;
    g.off_gram = g.off_part + (size_t)g.a.cap * R * arr;
    g.bytes = g.off_gram + gram_bytes(B, R);
    return DNMF_OK;
}

template <int R>
void launch_gram(const float *x, long ld, long n, double *part, int first, double *G, hipStream_t st) {
    const long nchunks = (n + BG_GRAM_CHUNK - 1) / BG_GRAM_CHUNK;
    hipLaunchKernelGGL(background_gram_kernel<R>, dim3((unsigned)nchunks), dim3(BG_THREADS), 0, st, x, ld, n, part);
    hipLaunchKernelGGL(background_gram_reduce_kernel<R>, dim3(1), dim3(64), 0, st, part, nchunks, first, G);
}

template <int R>
void launch_dots_rank(const DotsArgs &a, int B, int inner, float *f, long ldf_t, double *num, double *q, double *Q, double *gram,
                      hipStream_t st) {
    launch_gram<R>(a.b, a.ldb, a.P, gram, 1, Q, st);
    const dim3 grid((unsigned)((long)B * a.nseg));
    if (a.sub) hipLaunchKernelGGL((background_dots_rank_kernel<R, true>), grid, dim3(BG_THREADS), 0, st, a);
    else hipLaunchKernelGGL((background_dots_rank_kernel<R, false>), grid, dim3(BG_THREADS), 0, st, a);
    hipLaunchKernelGGL(background_dots_rank_finish_kernel<R>, dim3(lane_blocks(B)), dim3(BG_THREADS), 0, st, a.part, Q, a.nseg, B, inner, f, ldf_t, num, q);
}

// The accumulate pass and the reduction of its partials, the first two launches of both b half-steps.  ff: K19's sum f^2, which
// the reduction then keeps (NULL: K23).
template <int R>
void launch_accum(const AccumRankArgs &a, const AccumPlan &g, int first, double *sums, double *ff, hipStream_t st) {
    const dim3 grid((unsigned)g.ntiles, (unsigned)g.nseg);
    if (a.sub) hipLaunchKernelGGL((background_accum_rank_kernel<R, true>), grid, dim3(BG_THREADS), 0, st, a);
    else hipLaunchKernelGGL((background_accum_rank_kernel<R, false>), grid, dim3(BG_THREADS), 0, st, a);
    hipLaunchKernelGGL(background_accum_reduce_kernel, dim3(lane_blocks(a.P), (unsigned)R), dim3(BG_THREADS), 0, st, a.part, a.stride, g.nseg, R,
                       a.P, first, sums, ff ? a.f : nullptr, a.B, ff);
}

template <int R>
void launch_accum_rank(const AccumRankArgs &a, const AccumRankPlan &g, int first, int finish, int inner, double *W, double *sums, double *gram,
                       float *b, long ldb, double *num, double *w, hipStream_t st) {
    launch_accum<R>(a, g.a, first, sums, nullptr, st);
    launch_gram<R>(a.f, a.ldf_t, (long)a.B, gram, first, W, st);
    if (finish)
        hipLaunchKernelGGL(background_accum_rank_finish_kernel<R>, dim3(lane_blocks(a.P)), dim3(BG_THREADS), 0, st, sums, a.stride, W, a.P, inner,
                           b, ldb, num, w);
}

// R is a template parameter of the kernels: one case per supported value
#define DNMF_BG_BY_RANK(R, CALL) \
    switch (R) {                 \
        case 2: CALL(2); break;  \
        case 3: CALL(3); break;  \
        case 4: CALL(4); break;  \
        case 5: CALL(5); break;  \
        case 6: CALL(6); break;  \
        case 7: CALL(7); break;  \
        default: CALL(8); break; \
    }

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_background_dots_workspace(long P, int B) {
    dnmf::DotsPlan g;
    if (dnmf::dots_plan("dnmf_background_dots_workspace", P, B, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_background_dots(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *b, long P, int B,
                         double *num, double *bb, float *f, void *workspace, size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_background_dots";
    DNMF_REQUIRE(frames && b && f && workspace, DNMF_E_NULL, "%s: NULL argument", fn);
    DotsPlan g;
    int rc = dots_plan(fn, P, B, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P), DNMF_E_SHAPE, "%s: ldf=%ld lds=%ld below a row of P=%ld", fn, ldf, lds, P);
    rc = check_workspace(fn, "workspace", workspace, workspace_bytes, g.bytes);
    if (rc != DNMF_OK) return rc;
    char *w = static_cast<char *>(workspace);
    DotsArgs a;
    a.frames = frames, a.sub = sub, a.b = b, a.ldf = ldf, a.lds = lds, a.ldb = P, a.P = P, a.seglen = g.seglen, a.frame_ids = frame_ids;
    a.nseg = g.nseg, a.part = reinterpret_cast<double *>(w), a.bbpart = reinterpret_cast<double *>(w + g.off_bb);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)B * g.nseg));
    if (sub) hipLaunchKernelGGL(background_dots_kernel<true>, grid, dim3(BG_THREADS), 0, st, a);
    else hipLaunchKernelGGL(background_dots_kernel<false>, grid, dim3(BG_THREADS), 0, st, a);
    hipLaunchKernelGGL(background_dots_finish_kernel, dim3(lane_blocks(B)), dim3(BG_THREADS), 0, st, a.part, a.bbpart, g.nseg, B, num, bb, f);
    return check_launch(fn);
}

size_t dnmf_background_accum_workspace(long P, int B, int segment) {
    dnmf::AccumPlan g;
    if (dnmf::accum_plan("dnmf_background_accum_workspace", P, B, segment, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_background_accum(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *f, long P, int B,
                          int first, int finish, int segment, void *state, size_t state_bytes, float *b, double *num, double *ff,
                          dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_background_accum";
    DNMF_REQUIRE(frames && f && state, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(b || !finish, DNMF_E_NULL, "%s: b is NULL with finish", fn);
    AccumPlan g;
    int rc = accum_plan(fn, P, B, segment, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P), DNMF_E_SHAPE, "%s: ldf=%ld lds=%ld below a row of P=%ld", fn, ldf, lds, P);
    rc = check_workspace(fn, "state", state, state_bytes, g.bytes);
    if (rc != DNMF_OK) return rc;
    char *w = static_cast<char *>(state);
    double *hdr = reinterpret_cast<double *>(w), *sums = reinterpret_cast<double *>(w + g.off_sums);
    AccumRankArgs a;
    a.frames = frames, a.sub = sub, a.f = f, a.ldf = ldf, a.lds = lds, a.ldf_t = B, a.P = P, a.frame_ids = frame_ids, a.B = B;
    a.seglen = g.seglen, a.part = reinterpret_cast<double *>(w + g.off_part), a.stride = g.stride;
    const hipStream_t st = (hipStream_t)stream;
    launch_accum<1>(a, g, first != 0, sums, hdr, st);
    if (finish) hipLaunchKernelGGL(background_accum_finish_kernel, dim3(lane_blocks(P)), dim3(BG_THREADS), 0, st, sums, hdr, P, b, num, ff);
    return check_launch(fn);
}

int dnmf_background_subtract(const float *frames, long ldf, const int *frame_ids, const float *b, const float *f, int nf, const int *times,
                             long P, int B, float *out, long ldo, int clamp, dnmf_stream_t stream) {
    return dnmf::subtract<false>("dnmf_background_subtract", frames, ldf, frame_ids, b, P, f, nf, 1, nf, times, P, B, out, ldo, clamp, stream);
}

size_t dnmf_background_dots_rank_workspace(long P, int B, int R) {
    dnmf::DotsRankPlan g;
    if (dnmf::dots_rank_plan("dnmf_background_dots_rank_workspace", P, B, R, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_background_dots_rank(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *b, long ldb, int R,
                              long P, int B, int inner, float *f, long ldf_t, double *num, double *q, void *workspace, size_t workspace_bytes,
                              dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_background_dots_rank";
    DNMF_REQUIRE(frames && b && f && workspace, DNMF_E_NULL, "%s: NULL argument", fn);
    int rc = rank_check(fn, R, inner);
    if (rc != DNMF_OK) return rc;
    DotsRankPlan g;
    rc = dots_rank_plan(fn, P, B, R, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P) && ldb >= P, DNMF_E_SHAPE, "%s: ldf=%ld lds=%ld ldb=%ld below a row of P=%ld", fn, ldf, lds, ldb, P);
    DNMF_REQUIRE(ldf_t >= B, DNMF_E_SHAPE, "%s: ldf_t=%ld below a row of B=%d", fn, ldf_t, B);
    rc = check_workspace(fn, "workspace", workspace, workspace_bytes, g.bytes);
    if (rc != DNMF_OK) return rc;
    char *w = static_cast<char *>(workspace);
    DotsArgs a;
    a.frames = frames, a.sub = sub, a.b = b, a.ldf = ldf, a.lds = lds, a.ldb = ldb, a.P = P, a.seglen = g.d.seglen, a.frame_ids = frame_ids;
    a.nseg = g.d.nseg, a.part = reinterpret_cast<double *>(w + g.off_part), a.bbpart = nullptr;
    double *Q = reinterpret_cast<double *>(w), *gram = reinterpret_cast<double *>(w + g.off_gram);
    const hipStream_t st = (hipStream_t)stream;
#define DNMF_BG_CALL(N) launch_dots_rank<N>(a, B, inner, f, ldf_t, num, q, Q, gram, st)
    DNMF_BG_BY_RANK(R, DNMF_BG_CALL)
#undef DNMF_BG_CALL
    return check_launch(fn);
}

size_t dnmf_background_accum_rank_workspace(long P, int B, int R, int segment) {
    dnmf::AccumRankPlan g;
    if (dnmf::accum_rank_plan("dnmf_background_accum_rank_workspace", P, B, R, segment, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_background_accum_rank(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *f, long ldf_t, int R,
                               long P, int B, int first, int finish, int segment, int inner, void *state, size_t state_bytes, float *b, long ldb,
                               double *num, double *w_out, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_background_accum_rank";
    DNMF_REQUIRE(frames && f && state, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(b || !finish, DNMF_E_NULL, "%s: b is NULL with finish", fn);
    int rc = rank_check(fn, R, inner);
    if (rc != DNMF_OK) return rc;
    AccumRankPlan g;
    rc = accum_rank_plan(fn, P, B, R, segment, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P) && (!finish || ldb >= P), DNMF_E_SHAPE, "%s: ldf=%ld lds=%ld ldb=%ld below a row of P=%ld", fn, ldf,
                 lds, ldb, P);
    DNMF_REQUIRE(ldf_t >= B, DNMF_E_SHAPE, "%s: ldf_t=%ld below a row of B=%d", fn, ldf_t, B);
    rc = check_workspace(fn, "state", state, state_bytes, g.bytes);
    if (rc != DNMF_OK) return rc;
    char *w = static_cast<char *>(state);
    double *W = reinterpret_cast<double *>(w), *sums = reinterpret_cast<double *>(w + g.off_sums);
    double *gram = reinterpret_cast<double *>(w + g.off_gram);
    AccumRankArgs a;
    a.frames = frames, a.sub = sub, a.f = f, a.ldf = ldf, a.lds = lds, a.ldf_t = ldf_t, a.P = P, a.frame_ids = frame_ids, a.B = B;
    a.seglen = g.a.seglen, a.part = reinterpret_cast<double *>(w + g.off_part), a.stride = g.a.stride;
    const hipStream_t st = (hipStream_t)stream;
#define DNMF_BG_CALL(N) launch_accum_rank<N>(a, g, first != 0, finish != 0, inner, W, sums, gram, b, ldb, num, w_out, st)
    DNMF_BG_BY_RANK(R, DNMF_BG_CALL)
#undef DNMF_BG_CALL
    return check_launch(fn);
}

int dnmf_background_subtract_rank(const float *frames, long ldf, const int *frame_ids, const float *b, long ldb, const float *f, long ldf_t, int R,
                                  int nf, const int *times, long P, int B, float *out, long ldo, int clamp, dnmf_stream_t stream) {
    return dnmf::subtract<true>("dnmf_background_subtract_rank", frames, ldf, frame_ids, b, ldb, f, ldf_t, R, nf, times, P, B, out, ldo, clamp,
                                stream);
}

}  // extern "C"
