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
#include <cstdint>

#include "common.hpp"

namespace dnmf {
namespace {

constexpr int BG_THREADS = 256, BG_WAVES = BG_THREADS / 64;
constexpr int BG_TILE = 4 * BG_THREADS;          // voxels of a workgroup of accum and subtract: one float4 a lane
constexpr long BG_DOTS_MIN_SEG = BG_TILE;        // voxels: a segment of dots is a multiple of this
constexpr int BG_DOTS_TARGET_BLOCKS = 4096;
constexpr int BG_ACC_MIN_SEGMENT = 16;           // frames: below this the partial sums cost more traffic than the frames
constexpr int BG_ACC_TARGET_BLOCKS = 2048;
constexpr size_t BG_HEADER = 256;                // bytes: sum f^2

__host__ __device__ constexpr size_t bg_align(size_t n) { return (n + 255) / 256 * 256; }

// sum over the 64 lanes, valid in lane 0 (a fixed tree)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sum over the workgroup, valid in thread 0: the waves in their order.  `red` holds BG_WAVES doubles and is free again after
// the next barrier.
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
#pragma unroll
        for (int w = 0; w < BG_WAVES; ++w) s += red[w];
    return s;
}

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
    g.off_bb = bg_align((size_t)B * g.nseg * sizeof(double));
    g.bytes = g.off_bb + bg_align((size_t)g.nseg * sizeof(double));
    return DNMF_OK;
}

struct DotsArgs {
    const float *frames, *sub, *b;
    long ldf, lds, P, seglen;
    const int *frame_ids;
    int nseg;
    double *part, *bbpart;
};

// One term b (y - m) added to `acc`; WITH_BB: b^2 to `q`.
template <bool SUB, bool WITH_BB>
__device__ __forceinline__ void dots_term(float y, float m, float b, double &acc, double &q) {
    const double bd = (double)b;
    const double r = SUB ? (double)y - (double)m : (double)y;
    acc = fma(bd, r, acc);
    if (WITH_BB) q = fma(bd, bd, q);
}

template <bool SUB, bool WITH_BB>
__device__ __forceinline__ void dots_segment(const float *__restrict__ y, const float *__restrict__ m, const float *__restrict__ b,
                                             long n, double &sum, double &sumq) {
    const int tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    // 16-byte loads from the first voxel at which y, m and b are all aligned; rows whose starts differ in phase (P % 4 != 0
    // against the aligned b) are read one float at a time
    const unsigned ph = word_phase(y);
    const bool vec = word_phase(b) == ph && (!SUB || word_phase(m) == ph);
    long head = vec ? (long)((4 - ph) & 3) : n;
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    for (long i = tid; i < head; i += BG_THREADS) dots_term<SUB, WITH_BB>(y[i], SUB ? m[i] : 0.0f, b[i], acc[0], q[0]);
    const float4 *y4 = reinterpret_cast<const float4 *>(y + head), *b4 = reinterpret_cast<const float4 *>(b + head);
    const float4 *m4 = SUB ? reinterpret_cast<const float4 *>(m + head) : nullptr;
#pragma unroll 2
    for (long i = tid; i < n4; i += BG_THREADS) {
        const float4 yv = y4[i], bv = b4[i];
        const float4 mv = SUB ? m4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        dots_term<SUB, WITH_BB>(yv.x, mv.x, bv.x, acc[0], q[0]);
        dots_term<SUB, WITH_BB>(yv.y, mv.y, bv.y, acc[1], q[1]);
        dots_term<SUB, WITH_BB>(yv.z, mv.z, bv.z, acc[2], q[2]);
        dots_term<SUB, WITH_BB>(yv.w, mv.w, bv.w, acc[3], q[3]);
    }
    for (long i = head + 4 * n4 + tid; i < n; i += BG_THREADS) dots_term<SUB, WITH_BB>(y[i], SUB ? m[i] : 0.0f, b[i], acc[1], q[1]);
    sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    sumq = (q[0] + q[1]) + (q[2] + q[3]);
}

template <bool SUB>
__global__ __launch_bounds__(BG_THREADS) void background_dots_kernel(DotsArgs a) {
    __shared__ double red[2 * BG_WAVES];
    const long bid = blockIdx.x;
    const int j = (int)(bid / a.nseg), s = (int)(bid - (long)j * a.nseg);
    const long p0 = (long)s * a.seglen;
    const long n = (a.P - p0 < a.seglen ? a.P - p0 : a.seglen);
    const float *y = a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf + p0;
    const float *m = SUB ? a.sub + (long)j * a.lds + p0 : nullptr;
    const float *b = a.b + p0;
    double sum, sumq;
    if (j == 0) {   // the first frame's workgroups also sum b^2 over their segment
        dots_segment<SUB, true>(y, m, b, n, sum, sumq);
        const double tq = block_sum(sumq, red + BG_WAVES);
        if (threadIdx.x == 0) a.bbpart[s] = tq;
    } else {
        dots_segment<SUB, false>(y, m, b, n, sum, sumq);
    }
    const double t = block_sum(sum, red);
    if (threadIdx.x == 0) a.part[bid] = t;
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
struct AccumPlan {
    long ntiles;
    int seglen, nseg;
    size_t stride;   // doubles of one (P,) array
    size_t off_sums, off_part, bytes;
};

int accum_plan(const char *fn, long P, int B, int segment, AccumPlan &g) {
    DNMF_REQUIRE(P >= 1 && B >= 1, DNMF_E_SHAPE, "%s: P=%ld voxels, B=%d frames", fn, P, B);
    DNMF_REQUIRE(segment >= 0, DNMF_E_SHAPE, "%s: segment=%d", fn, segment);
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    g.ntiles = (P + BG_TILE - 1) / BG_TILE;
    long cap;   // the most segments a call of B frames can have: it sizes the state, and does not decrease with B
    if (segment > 0) {
        g.seglen = segment;
        cap = ((long)B + segment - 1) / segment;
    } else {
        long want = (BG_ACC_TARGET_BLOCKS + g.ntiles - 1) / g.ntiles;
        const long most = ((long)B + BG_ACC_MIN_SEGMENT - 1) / BG_ACC_MIN_SEGMENT;
        if (want > most) want = most;
        g.seglen = (int)((B + want - 1) / want);
        cap = want;
    }
    DNMF_REQUIRE(cap <= 65535, DNMF_E_UNSUPPORTED, "%s: %ld segments of %d frames (they ride on gridDim.y: at most 65535)", fn, cap,
                 g.seglen);
    g.nseg = (int)(((long)B + g.seglen - 1) / g.seglen);
    const size_t arr = bg_align((size_t)P * sizeof(double));
    g.stride = arr / sizeof(double);
    g.off_sums = BG_HEADER;
    g.off_part = g.off_sums + arr;
    g.bytes = g.off_part + (size_t)cap * arr;
    return DNMF_OK;
}

struct AccumArgs {
    const float *frames, *sub, *f;
    long ldf, lds, P;
    const int *frame_ids;
    int B, seglen;
    double *part;
    size_t stride;
};

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

template <bool SUB>
__global__ __launch_bounds__(BG_THREADS) void background_accum_kernel(AccumArgs a) {
    const long p = (long)blockIdx.x * BG_TILE + 4 * (long)threadIdx.x;
    if (p >= a.P) return;
    const int live = a.P - p >= 4 ? 4 : (int)(a.P - p);
    const int seg = blockIdx.y;
    const int f0 = seg * a.seglen, f1 = min(a.B, f0 + a.seglen);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 2
    for (int j = f0; j < f1; ++j) {
        const float4 y = load4(a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf, p, live);
        const double fj = (double)a.f[j];
        if (SUB) {
            const float4 m = load4(a.sub + (long)j * a.lds, p, live);
            s0 = fma(fj, (double)y.x - (double)m.x, s0);
            s1 = fma(fj, (double)y.y - (double)m.y, s1);
            s2 = fma(fj, (double)y.z - (double)m.z, s2);
            s3 = fma(fj, (double)y.w - (double)m.w, s3);
        } else {
            s0 = fma(fj, (double)y.x, s0);
            s1 = fma(fj, (double)y.y, s1);
            s2 = fma(fj, (double)y.z, s2);
            s3 = fma(fj, (double)y.w, s3);
        }
    }
    double *out = a.part + (size_t)seg * a.stride + p;
    out[0] = s0;
    if (live > 1) out[1] = s1;
    if (live > 2) out[2] = s2;
    if (live > 3) out[3] = s3;
}

// sums = (first ? 0 : sums) + the segments in their order; ff = (first ? 0 : ff) + sum f^2 of the call (workgroup 0, fixed tree)
__global__ __launch_bounds__(BG_THREADS) void background_accum_reduce_kernel(const double *__restrict__ part, size_t stride, int nseg, long P,
                                                                             int first, const float *__restrict__ f, int B,
                                                                             double *__restrict__ sums, double *__restrict__ ff) {
    __shared__ double red[BG_WAVES];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) {
        double acc = first ? 0.0 : sums[i];
        for (int s = 0; s < nseg; ++s) acc += part[(size_t)s * stride + i];
        sums[i] = acc;
    }
    if (blockIdx.x == 0) {
        double q = 0.0;
        for (int j = threadIdx.x; j < B; j += BG_THREADS) {
            const double v = (double)f[j];
            q = fma(v, v, q);
        }
        const double t = block_sum(q, red);
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
    long ldf, ldo, P, ntiles;
    const int *frame_ids, *times;
    int nf, clamp;
    float *out;
};

__global__ __launch_bounds__(BG_THREADS) void background_subtract_kernel(SubtractArgs a) {
    const long bid = blockIdx.x;
    const int j = (int)(bid / a.ntiles);
    const long p = (bid - (long)j * a.ntiles) * BG_TILE + 4 * (long)threadIdx.x;
    if (p >= a.P) return;
    const int live = a.P - p >= 4 ? 4 : (int)(a.P - p);
    const int t = a.times ? a.times[j] : j;
    // a time f has no entry for: the row becomes NaN instead of reading beyond f
    const float fj = (t >= 0 && t < a.nf) ? a.f[t] : __builtin_nanf("");
    const float4 y = load4(a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf, p, live);
    const float4 b = load4(a.b, p, live);
    float4 r;
    r.x = fmaf(-b.x, fj, y.x), r.y = fmaf(-b.y, fj, y.y), r.z = fmaf(-b.z, fj, y.z), r.w = fmaf(-b.w, fj, y.w);
    if (a.clamp) r.x = fmaxf(r.x, 0.0f), r.y = fmaxf(r.y, 0.0f), r.z = fmaxf(r.z, 0.0f), r.w = fmaxf(r.w, 0.0f);
    if (t < 0 || t >= a.nf) r.x = r.y = r.z = r.w = fj;   // fmaxf drops a NaN
    float *o = a.out + (long)j * a.ldo;
    if (live == 4 && word_phase(o) == 0) {
        *reinterpret_cast<float4 *>(o + p) = r;
        return;
    }
    o[p] = r.x;
    if (live > 1) o[p + 1] = r.y;
    if (live > 2) o[p + 2] = r.z;
    if (live > 3) o[p + 3] = r.w;
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
    DNMF_REQUIRE(frames && b && f && workspace, DNMF_E_NULL, "dnmf_background_dots: NULL argument");
    DotsPlan g;
    const int rc = dots_plan("dnmf_background_dots", P, B, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P), DNMF_E_SHAPE, "dnmf_background_dots: ldf=%ld lds=%ld below a row of P=%ld", ldf, lds, P);
    DNMF_REQUIRE(workspace_bytes >= g.bytes, DNMF_E_WORKSPACE, "dnmf_background_dots: workspace of %zu bytes, need %zu", workspace_bytes,
                 g.bytes);
    DNMF_REQUIRE(((size_t)workspace & 7) == 0, DNMF_E_WORKSPACE, "dnmf_background_dots: workspace must be 8-byte aligned");
    char *w = static_cast<char *>(workspace);
    DotsArgs a;
    a.frames = frames, a.sub = sub, a.b = b, a.ldf = ldf, a.lds = lds, a.P = P, a.seglen = g.seglen, a.frame_ids = frame_ids;
    a.nseg = g.nseg;
    a.part = reinterpret_cast<double *>(w), a.bbpart = reinterpret_cast<double *>(w + g.off_bb);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)B * g.nseg));
    if (sub) hipLaunchKernelGGL(background_dots_kernel<true>, grid, dim3(BG_THREADS), 0, st, a);
    else hipLaunchKernelGGL(background_dots_kernel<false>, grid, dim3(BG_THREADS), 0, st, a);
    hipLaunchKernelGGL(background_dots_finish_kernel, dim3((unsigned)((B + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0, st, a.part,
                       a.bbpart, g.nseg, B, num, bb, f);
    return check_launch("dnmf_background_dots");
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
    DNMF_REQUIRE(frames && f && state, DNMF_E_NULL, "dnmf_background_accum: NULL argument");
    DNMF_REQUIRE(b || !finish, DNMF_E_NULL, "dnmf_background_accum: b is NULL with finish");
    AccumPlan g;
    const int rc = accum_plan("dnmf_background_accum", P, B, segment, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= P && (!sub || lds >= P), DNMF_E_SHAPE, "dnmf_background_accum: ldf=%ld lds=%ld below a row of P=%ld", ldf, lds, P);
    DNMF_REQUIRE(state_bytes >= g.bytes, DNMF_E_WORKSPACE, "dnmf_background_accum: state of %zu bytes, need %zu", state_bytes, g.bytes);
    DNMF_REQUIRE(((size_t)state & 7) == 0, DNMF_E_WORKSPACE, "dnmf_background_accum: state must be 8-byte aligned");
    char *w = static_cast<char *>(state);
    double *hdr = reinterpret_cast<double *>(w), *sums = reinterpret_cast<double *>(w + g.off_sums);
    AccumArgs a;
    a.frames = frames, a.sub = sub, a.f = f, a.ldf = ldf, a.lds = lds, a.P = P, a.frame_ids = frame_ids, a.B = B, a.seglen = g.seglen;
    a.part = reinterpret_cast<double *>(w + g.off_part), a.stride = g.stride;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.ntiles, (unsigned)g.nseg);
    if (sub) hipLaunchKernelGGL(background_accum_kernel<true>, grid, dim3(BG_THREADS), 0, st, a);
    else hipLaunchKernelGGL(background_accum_kernel<false>, grid, dim3(BG_THREADS), 0, st, a);
    const unsigned pblocks = (unsigned)((P + BG_THREADS - 1) / BG_THREADS);
    hipLaunchKernelGGL(background_accum_reduce_kernel, dim3(pblocks), dim3(BG_THREADS), 0, st, a.part, g.stride, g.nseg, P, first != 0, f, B,
                       sums, hdr);
    if (finish) hipLaunchKernelGGL(background_accum_finish_kernel, dim3(pblocks), dim3(BG_THREADS), 0, st, sums, hdr, P, b, num, ff);
    return check_launch("dnmf_background_accum");
}

int dnmf_background_subtract(const float *frames, long ldf, const int *frame_ids, const float *b, const float *f, int nf, const int *times,
                             long P, int B, float *out, long ldo, int clamp, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames && b && f && out, DNMF_E_NULL, "dnmf_background_subtract: NULL argument");
    DNMF_REQUIRE(P >= 1 && B >= 1 && nf >= 1, DNMF_E_SHAPE, "dnmf_background_subtract: P=%ld voxels, B=%d frames, nf=%d", P, B, nf);
    DNMF_REQUIRE(ldf >= P && ldo >= P, DNMF_E_SHAPE, "dnmf_background_subtract: ldf=%ld ldo=%ld below a row of P=%ld", ldf, ldo, P);
    DNMF_REQUIRE(times || B <= nf, DNMF_E_SHAPE, "dnmf_background_subtract: B=%d frames but f has %d values and times is NULL", B, nf);
    DNMF_REQUIRE(out != frames || (!frame_ids && ldo == ldf), DNMF_E_SHAPE,
                 "dnmf_background_subtract: in place (out == frames) needs frame_ids NULL and ldo == ldf");
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_background_subtract: %ld voxels (32-bit offsets)", P);
    SubtractArgs a;
    a.frames = frames, a.b = b, a.f = f, a.ldf = ldf, a.ldo = ldo, a.P = P, a.ntiles = (P + BG_TILE - 1) / BG_TILE;
    a.frame_ids = frame_ids, a.times = times, a.nf = nf, a.clamp = clamp != 0, a.out = out;
    DNMF_REQUIRE(a.ntiles * B < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_background_subtract: %ld workgroups (split the call)", a.ntiles * B);
    hipLaunchKernelGGL(background_subtract_kernel, dim3((unsigned)(a.ntiles * B)), dim3(BG_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("dnmf_background_subtract");
}

}  // extern "C"
