// K26: merging duplicate components -- the statistics of listed pairs of components (dnmf_component_pairs) and the merged model
// from a table of groups and their coefficients (dnmf_merge_apply).  include/dnmf_hip.h has the contract,
// tests/merge_restatement.py the definition in float64.
//
// Pairs.  One workgroup of MC_THREADS lanes per listed pair (i, j).  A lane takes the voxels of the intersection of the two boxes
// (x slowest, z fastest) at lane, lane + MC_THREADS, .. and adds a_i a_j in float64; the workgroup finds the first frame where
// both traces are finite by a min-reduction on the frame index; a lane then takes the frames at lane, lane + MC_THREADS, .. and
// adds the count, the five sums of the traces shifted by their values at that first frame, and the raw product.  Eight
// block_sum0 reductions (block_ops.hpp: a fixed order), thread 0 writes.  No atomics, no scratch, no workspace.
//
// Apply.  One launch, one thread per entry of the new model: A_out[v, g] = sum over the members k of group g of u_k A[v, k] and
// C_out[g, t] = sum_k w_k C[k, t], in member order, in float64, rounded once.
#include "block_ops.hpp"
#include "boxes.hpp"

namespace dnmf {
namespace {

constexpr int MC_THREADS = 256, MC_WAVES = MC_THREADS / 64;
constexpr int MC_SUMS = 8;              // saa, n, si, sj, sii, sjj, sij, scc

struct PairArgs {
    const float *A, *C;
    long lda, ldc;
    const int *boxes, *pairs;
    int Y, Z, T;
    double *out;            // (N, MC_SUMS)
};

__global__ __launch_bounds__(MC_THREADS) void component_pairs_kernel(PairArgs g) {
    __shared__ double red[MC_SUMS][MC_WAVES];
    __shared__ uint64_t redk[MC_WAVES];
    const int tid = threadIdx.x;
    const long p = blockIdx.x;
    const int i = g.pairs[2 * p], j = g.pairs[2 * p + 1];
    const int *bi = g.boxes + 6 * (long)i, *bj = g.boxes + 6 * (long)j;
    const int x0 = max(bi[0], bj[0]), x1 = min(bi[1], bj[1]);
    const int y0 = max(bi[2], bj[2]), y1 = min(bi[3], bj[3]);
    const int z0 = max(bi[4], bj[4]), z1 = min(bi[5], bj[5]);
    const int ey = y1 - y0 + 1, ez = z1 - z0 + 1;
    const int n = (x1 >= x0 && ey > 0 && ez > 0) ? (x1 - x0 + 1) * ey * ez : 0;   // inside both boxes: at most BOX_MAX_VOXELS
    const Box q = {x0, y0, z0, ey, ez, n};
    const float *Ai = g.A + (long)i * g.lda, *Aj = g.A + (long)j * g.lda;
    double saa = 0.0;
    for (int v = tid; v < n; v += MC_THREADS) {
        const int off = box_offset(q, v, g.Y, g.Z);
        saa = fma((double)Ai[off], (double)Aj[off], saa);
    }

    const float *Ci = g.C + (long)i * g.ldc, *Cj = g.C + (long)j * g.ldc;
    uint64_t first = (uint64_t)g.T;
    for (int t = tid; t < g.T; t += MC_THREADS)
        if (__builtin_isfinite(Ci[t]) && __builtin_isfinite(Cj[t])) {
            first = (uint64_t)t;      // a lane's frames ascend: its first hit is its lowest
            break;
        }
    const int t0 = (int)block_reduce<MC_THREADS>(first, OpMinKey(), redk);
    double cnt = 0.0, si = 0.0, sj = 0.0, sii = 0.0, sjj = 0.0, sij = 0.0, scc = 0.0;
    if (t0 < g.T) {
        const double ci0 = (double)Ci[t0], cj0 = (double)Cj[t0];
        for (int t = tid; t < g.T; t += MC_THREADS) {
            const float fi = Ci[t], fj = Cj[t];
            if (__builtin_isfinite(fi) && __builtin_isfinite(fj)) {
                const double ci = (double)fi, cj = (double)fj, di = ci - ci0, dj = cj - cj0;
                cnt += 1.0;
                si += di, sj += dj;
                sii = fma(di, di, sii), sjj = fma(dj, dj, sjj), sij = fma(di, dj, sij);
                scc = fma(ci, cj, scc);
            }
        }
    }
    // one row of red per value: no barrier is needed between the reductions
    const double v[MC_SUMS] = {saa, cnt, si, sj, sii, sjj, sij, scc};
    double s[MC_SUMS];
#pragma unroll
    for (int q = 0; q < MC_SUMS; ++q) s[q] = block_sum0<MC_THREADS>(v[q], red[q]);
    if (tid == 0) {
        double *out = g.out + MC_SUMS * p;
#pragma unroll
        for (int q = 0; q < MC_SUMS; ++q) out[q] = s[q];
    }
}

struct ApplyArgs {
    const float *A, *C;
    long lda, ldc, ldao, ldco, P;
    int T, Kout;
    const int *offsets, *members;
    const double *u, *w;
    float *A_out, *C_out;
};

__global__ __launch_bounds__(MC_THREADS) void merge_apply_kernel(ApplyArgs g) {
    const long e = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    const long nA = g.P * g.Kout, nC = (long)g.Kout * g.T;
    if (e < nA) {
        const long v = e / g.Kout;
        const int q = (int)(e % g.Kout);
        const float *row = g.A + v * g.lda;
        double acc = 0.0;
        bool any = false;
        for (int m = g.offsets[q]; m < g.offsets[q + 1]; ++m) {
            const double term = g.u[m] * (double)row[g.members[m]];
            acc = any ? acc + term : term;      // the first term as it is: a singleton with u = 1 keeps -0.0 and every NaN payload
            any = true;
        }
        g.A_out[v * g.ldao + q] = (float)acc;
    } else if (e < nA + nC) {
        const long f = e - nA;
        const int q = (int)(f / g.T), t = (int)(f % g.T);
        double acc = 0.0;
        bool any = false;
        for (int m = g.offsets[q]; m < g.offsets[q + 1]; ++m) {
            const double term = g.w[m] * (double)g.C[(long)g.members[m] * g.ldc + t];
            acc = any ? acc + term : term;
            any = true;
        }
        g.C_out[(long)q * g.ldco + t] = (float)acc;
    }
}

// [p, p + the bytes of `rows` rows of `row` floats at stride ld)
struct Span {
    const char *lo, *hi;
};
Span span_of(const float *p, long rows, long ld, long row) {
    const char *lo = reinterpret_cast<const char *>(p);
    return {lo, lo + sizeof(float) * (size_t)((rows - 1) * ld + row)};
}
bool overlaps(const Span &a, const Span &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_component_pairs(const float *A, long lda, const int *sz, const int *boxes, const int *boxes_dev, int K, const float *C,
                         long ldc, int T, const int *pairs, const int *pairs_dev, int N, double *out, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_component_pairs";
    DNMF_REQUIRE(A && sz && boxes && boxes_dev && C && pairs && pairs_dev && out, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(K >= 1 && T >= 1 && N >= 1, DNMF_E_SHAPE, "%s: K=%d neurons, T=%d frames, N=%d pairs", fn, K, T, N);
    const int X = sz[0], Y = sz[1], Z = sz[2];
    const long P = (long)X * Y * Z;
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, P);
    DNMF_REQUIRE(lda >= P, DNMF_E_SHAPE, "%s: lda=%ld below a row of P=%ld", fn, lda, P);
    DNMF_REQUIRE(ldc >= T, DNMF_E_SHAPE, "%s: ldc=%ld below a row of T=%d", fn, ldc, T);
    const int rb = check_boxes(fn, sz, boxes, K, BOX_MAX_VOXELS, DNMF_E_SHAPE);
    if (rb != DNMF_OK) return rb;
    for (long p = 0; p < N; ++p)
        DNMF_REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < K && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < K, DNMF_E_SHAPE,
                     "%s: pair %ld = (%d, %d) outside [0, %d)", fn, p, pairs[2 * p], pairs[2 * p + 1], K);
    PairArgs g;
    g.A = A, g.C = C, g.lda = lda, g.ldc = ldc, g.boxes = boxes_dev, g.pairs = pairs_dev, g.Y = Y, g.Z = Z, g.T = T, g.out = out;
    hipLaunchKernelGGL(component_pairs_kernel, dim3((unsigned)N), dim3(MC_THREADS), 0, (hipStream_t)stream, g);
    return check_launch(fn);
}

int dnmf_merge_apply(const float *A, long lda, long P, int K, const float *C, long ldc, int T, const int *offsets, const int *members,
                     const int *offsets_dev, const int *members_dev, int Kout, const double *u, const double *w, float *A_out, long ldao,
                     float *C_out, long ldco, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_merge_apply";
    DNMF_REQUIRE(A && C && offsets && members && offsets_dev && members_dev && u && w && A_out && C_out, DNMF_E_NULL,
                 "%s: NULL argument", fn);
    DNMF_REQUIRE(P >= 1 && K >= 1 && T >= 1 && Kout >= 1, DNMF_E_SHAPE, "%s: P=%ld voxels, K=%d neurons, T=%d frames, %d groups", fn, P,
                 K, T, Kout);
    DNMF_REQUIRE(Kout <= K, DNMF_E_SHAPE, "%s: %d groups of K=%d neurons", fn, Kout, K);
    DNMF_REQUIRE(lda >= K && ldao >= Kout, DNMF_E_SHAPE, "%s: lda=%ld below K=%d or ldao=%ld below the %d groups", fn, lda, K, ldao, Kout);
    DNMF_REQUIRE(ldc >= T && ldco >= T, DNMF_E_SHAPE, "%s: ldc=%ld ldco=%ld below a row of T=%d", fn, ldc, ldco, T);
    DNMF_REQUIRE(offsets[0] == 0, DNMF_E_SHAPE, "%s: offsets[0]=%d, not 0", fn, offsets[0]);
    for (int q = 0; q < Kout; ++q)
        DNMF_REQUIRE(offsets[q + 1] > offsets[q] && offsets[q + 1] <= K, DNMF_E_SHAPE,
                     "%s: group %d = members [%d, %d): empty, or more members than the K=%d neurons", fn, q, offsets[q], offsets[q + 1], K);
    for (int m = 0; m < offsets[Kout]; ++m)
        DNMF_REQUIRE(members[m] >= 0 && members[m] < K, DNMF_E_SHAPE, "%s: member %d = %d outside [0, %d)", fn, m, members[m], K);
    const Span sa = span_of(A, P, lda, K), sc = span_of(C, K, ldc, T), oa = span_of(A_out, P, ldao, Kout), oc = span_of(C_out, Kout, ldco, T);
    DNMF_REQUIRE(!overlaps(oa, sa) && !overlaps(oa, sc) && !overlaps(oc, sa) && !overlaps(oc, sc) && !overlaps(oa, oc), DNMF_E_SHAPE,
                 "%s: A_out or C_out overlaps an input or the other output (a group reads entries that another has written)", fn);
    ApplyArgs g;
    g.A = A, g.C = C, g.lda = lda, g.ldc = ldc, g.ldao = ldao, g.ldco = ldco, g.P = P, g.T = T, g.Kout = Kout;
    g.offsets = offsets_dev, g.members = members_dev, g.u = u, g.w = w, g.A_out = A_out, g.C_out = C_out;
    const long total = P * Kout + (long)Kout * T, blocks = (total + MC_THREADS - 1) / MC_THREADS;
    DNMF_REQUIRE(blocks < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld entries to write", fn, total);
    hipLaunchKernelGGL(merge_apply_kernel, dim3((unsigned)blocks), dim3(MC_THREADS), 0, (hipStream_t)stream, g);
    return check_launch(fn);
}

}  // extern "C"
