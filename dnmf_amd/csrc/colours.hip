// K29: the channel colours of a multi-channel model.  With A_t the uncoloured warped footprints of frame t, G_t = A_t^T A_t and
// r_t^c = A_t^T y_t^c, the squared error of channel c is a quadratic in x = colours[c, :]:
//   M[k, l] = sum_t G_t[k, l] C[k, t] C[l, t]        b[c, k] = sum_t r_t^c[k] C[k, t]        x <- argmin_{x >= 0} 1/2 x^T M x - b_c^T x
// include/dnmf_hip.h has the contract, tests/colours_restatement.py the definition in float64.
//
// K29a (dnmf_colour_normal_eqs) is one streaming read of G.  A workgroup of CN_THREADS lanes owns a tile of CN_TK x CN_TL entries
// (k, l) and one segment of CN_SEG frames; wave w holds the rows k0 + 4 w .. k0 + 4 w + 3 and lane i the column l0 + i, so a wave
// reads 256 consecutive bytes of G[t, k, :].  The C[k, t] and C[l, t] of the tile and the segment are staged in LDS once.  A term is
// (double)G * ((double)C[k, t] * (double)C[l, t]) -- the inner product is exact and symmetric in (k, l), so a symmetric G gives a
// symmetric M bit for bit -- and a lane adds its terms in the order of t, starting from 0.0.  Further workgroups form the segment's
// part of b the same way, one lane per (c, k).
// The segments are cut on the count of frames SINCE THE STATE WAS RESET, not on the frames of a call: the state keeps that count, the
// sum of the closed segments and the part of the open one, and a call's first workgroup of an entry goes on from the open part.  So
// the additions are the same whatever pieces the movie comes in, and the result has the same bits.  A second launch adds the closed
// segments of the call to the state in their order (no floating-point atomics), a third steps the count.
//
// K29b (dnmf_colour_solve): cyclic coordinate descent, one workgroup per channel.  x, the diagonal and b_c are in LDS and the
// running h = M x in the registers of the lane that owns an entry, all float64.  A step k needs h[k] and x[k] in every lane: the
// owner of the NEXT coordinate leaves both in one of two LDS slots before the step's single barrier.  Row k of M (= column k: M is
// symmetric) comes from LDS where 8 K^2 bytes fit beside the vectors (K <= CS_LDS_MAX_K), else from global memory with the next row
// in flight while this one is used.
#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int CN_THREADS = 256;
constexpr int CN_SEG = 32;              // frames of a segment
constexpr int CN_TK = 16, CN_TL = 64;   // the tile of (k, l)
constexpr int CN_ROWS = CN_TK / (CN_THREADS / 64);
constexpr int COLOUR_MAX_K = 4096, COLOUR_MAX_NC = 16;
constexpr size_t CN_HEADER = 256;       // bytes: the count of frames since the reset

struct ColourPlan {
    int K, NC, B, ntl, ntiles, nbt, units;
    long cap;             // the most segments a call of B frames can touch
    size_t E, slab;       // entries (M then b), doubles between two slabs
    size_t bytes;         // header | sum of the closed segments | open segment | cap partial slabs
};

int colour_plan(const char *fn, int K, int NC, int B, ColourPlan &g) {
    DNMF_REQUIRE(K >= 1 && NC >= 1 && B >= 1, DNMF_E_SHAPE, "%s: K=%d neurons, NC=%d channels, B=%d frames", fn, K, NC, B);
    DNMF_REQUIRE(K <= COLOUR_MAX_K && NC <= COLOUR_MAX_NC, DNMF_E_UNSUPPORTED, "%s: K=%d (<= %d), NC=%d (<= %d)", fn, K, COLOUR_MAX_K, NC,
                 COLOUR_MAX_NC);
    g.K = K, g.NC = NC, g.B = B;
    g.ntl = (K + CN_TL - 1) / CN_TL;
    g.ntiles = ((K + CN_TK - 1) / CN_TK) * g.ntl;
    g.nbt = (K + CN_THREADS - 1) / CN_THREADS;
    g.units = g.ntiles + NC * g.nbt;
    g.cap = ((long)B + CN_SEG - 1) / CN_SEG + 1;
    DNMF_REQUIRE(g.cap <= 65535, DNMF_E_UNSUPPORTED, "%s: %ld segments of %d frames (they ride on gridDim.y: at most 65535)", fn, g.cap,
                 CN_SEG);
    g.E = (size_t)K * K + (size_t)NC * K;
    g.slab = align256(g.E * sizeof(double)) / sizeof(double);
    g.bytes = CN_HEADER + (2 + (size_t)g.cap) * g.slab * sizeof(double);
    return DNMF_OK;
}

struct NormalArgs {
    const float *G, *r, *C;
    long ldc;
    int K, NC, B, ntl, ntiles, nbt, first, finish;
    const long *done;     // the header
    double *acc, *open, *part;
    size_t slab, E;
    double *M, *b;
};

// the frames [j0, j1) of the call that fall into segment `seg`, counted from the `off` frames the open segment already holds
__device__ __forceinline__ void segment_frames(int seg, int off, int B, int &j0, int &j1) {
    j0 = max(0, seg * CN_SEG - off);
    j1 = min(B, (seg + 1) * CN_SEG - off);
}

__global__ __launch_bounds__(CN_THREADS) void colour_accumulate_kernel(NormalArgs g) {
    __shared__ float ck[CN_SEG][CN_TK], cl[CN_SEG][CN_TL];
    const int tid = threadIdx.x, unit = blockIdx.x, seg = blockIdx.y;
    const int off = g.first ? 0 : (int)(g.done[0] % CN_SEG);
    int j0, j1;
    segment_frames(seg, off, g.B, j0, j1);
    if (j0 >= j1) return;                          // the whole workgroup: no barrier yet
    const bool carry = seg == 0 && off > 0;        // goes on from the open segment of the earlier calls
    const int K = g.K, nfr = j1 - j0;
    double *part = g.part + (size_t)seg * g.slab;
    if (unit >= g.ntiles) {                        // b: one lane per (c, k)
        const int c = (unit - g.ntiles) / g.nbt, k = ((unit - g.ntiles) % g.nbt) * CN_THREADS + tid;
        if (k >= K) return;
        const size_t e = (size_t)K * K + (size_t)c * K + k;
        const float *rc = g.r + ((size_t)c * g.B + j0) * K + k, *Ck = g.C + (long)k * g.ldc + j0;
        double s = carry ? g.open[e] : 0.0;
        for (int j = 0; j < nfr; ++j) s += (double)rc[(size_t)j * K] * (double)Ck[j];
        part[e] = s;
        return;
    }
    const int k0 = (unit / g.ntl) * CN_TK, l0 = (unit % g.ntl) * CN_TL;
    for (int i = tid; i < (CN_TK + CN_TL) * nfr; i += CN_THREADS) {
        const int row = i / nfr, tt = i % nfr;     // consecutive lanes read consecutive frames of one trace
        const int n = row < CN_TK ? k0 + row : l0 + row - CN_TK;
        const float v = n < K ? g.C[(long)n * g.ldc + j0 + tt] : 0.0f;
        if (row < CN_TK) ck[tt][row] = v;
        else cl[tt][row - CN_TK] = v;
    }
    __syncthreads();
    const int lane = tid & 63, kw = k0 + (tid >> 6) * CN_ROWS, l = l0 + lane;
    if (l >= K || kw >= K) return;
    const int rows = min(CN_ROWS, K - kw);
    double s[CN_ROWS];
#pragma unroll
    for (int i = 0; i < CN_ROWS; ++i) s[i] = (carry && i < rows) ? g.open[(size_t)(kw + i) * K + l] : 0.0;
    const float *Gp = g.G + ((size_t)j0 * K + kw) * K + l;
    const size_t frame = (size_t)K * K;
#pragma unroll 4
    for (int tt = 0; tt < nfr; ++tt) {
        const double cc = (double)cl[tt][lane];
#pragma unroll
        for (int i = 0; i < CN_ROWS; ++i) {
            const float gv = i < rows ? Gp[(size_t)tt * frame + (size_t)i * K] : 0.0f;
            s[i] += (double)gv * ((double)ck[tt][(tid >> 6) * CN_ROWS + i] * cc);
        }
    }
#pragma unroll
    for (int i = 0; i < CN_ROWS; ++i)
        if (i < rows) part[(size_t)(kw + i) * K + l] = s[i];
}

// One lane per entry: state = (first ? 0 : state) + the segments this call has closed, in their order; the segment that stays open
// is kept beside it; with finish M and b = the two added.
__global__ __launch_bounds__(CN_THREADS) void colour_finish_kernel(NormalArgs g) {
    const size_t e = (size_t)blockIdx.x * CN_THREADS + threadIdx.x;
    if (e >= g.E) return;
    const int off = g.first ? 0 : (int)(g.done[0] % CN_SEG);
    const long total = (long)off + g.B;
    const int nclosed = (int)(total / CN_SEG);
    double acc = g.first ? 0.0 : g.acc[e];
    for (int s = 0; s < nclosed; ++s) acc += g.part[(size_t)s * g.slab + e];
    g.acc[e] = acc;
    double out = acc;
    if (total % CN_SEG) {
        const double op = g.part[(size_t)nclosed * g.slab + e];
        g.open[e] = op;
        out = acc + op;
    }
    if (g.finish) {
        const size_t KK = (size_t)g.K * g.K;
        if (e < KK) g.M[e] = out;
        else g.b[e - KK] = out;
    }
}

__global__ void colour_count_kernel(long *done, int first, int B) { done[0] = (first ? 0 : done[0]) + B; }

// ---- K29b ---------------------------------------------------------------------------------------------------------------------------
constexpr int CS_THREADS = 256;
constexpr int CS_LDS_MAX_K = 128;       // 8 K^2 = 128 KiB of the CU's 160 beside 3 K doubles and the slots

struct SolveArgs {
    const double *M, *b;
    const float *colours;
    int K, sweeps;
    float *out;
    double *kkt;
    int *ok;
};

inline size_t solve_lds(int K) {
    const size_t vec = (3 * (size_t)K + 8) * sizeof(double);
    return vec + (K <= CS_LDS_MAX_K ? (size_t)K * K * sizeof(double) : 0);
}

template <int SLOTS, bool LDSM>
__global__ __launch_bounds__(CS_THREADS) void colour_solve_kernel(SolveArgs a) {
    extern __shared__ double cs_lds[];
    const int tid = threadIdx.x, c = blockIdx.x, K = a.K;
    double *x = cs_lds, *bb = x + K, *dg = bb + K, *slot = dg + K, *red = slot + 4, *Ml = red + 4;
    const double *Mrows = LDSM ? Ml : a.M;
    const float *col = a.colours + (size_t)c * K;

    int bad = 0;
    for (size_t e = tid; e < (size_t)K * K; e += CS_THREADS) {
        const double v = a.M[e];
        bad |= !__builtin_isfinite(v);
        if (LDSM) Ml[e] = v;
    }
    for (int k = tid; k < K; k += CS_THREADS) {
        const double v = a.b[(size_t)c * K + k];
        bad |= !__builtin_isfinite(v);
        bb[k] = v, dg[k] = a.M[(size_t)k * K + k], x[k] = (double)col[k];
    }
    bad = block_reduce<CS_THREADS>(bad, OpSum(), red);     // ends with a barrier: the staged values are visible
    if (bad) {                                             // the channel keeps its row
        if (a.out)
            for (int k = tid; k < K; k += CS_THREADS) a.out[(size_t)c * K + k] = col[k];
        if (tid == 0) a.kkt[c] = quiet_nan(), a.ok[c] = 0;
        return;
    }
    // h = M x, the terms of an entry added in the order of k
    double h[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) h[s] = 0.0;
    for (int k = 0; k < K; ++k) {
        const double xk = x[k];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int l = tid + s * CS_THREADS;
            if (l < K) h[s] += Mrows[(size_t)k * K + l] * xk;
        }
    }
    if (tid == 0) slot[0] = h[0], slot[1] = x[0];
    __syncthreads();

    double cur[SLOTS], nxt[SLOTS];
    auto fetch = [&](int k) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int l = tid + s * CS_THREADS;
            nxt[s] = l < K ? Mrows[(size_t)k * K + l] : 0.0;
        }
    };
    const long steps = (long)a.sweeps * K;
    if (steps > 0) fetch(0);
    int k = 0;
    for (long n = 0; n < steps; ++n) {
        const int p = (int)(n & 1), kn = k + 1 < K ? k + 1 : 0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) cur[s] = nxt[s];
        if (n + 1 < steps) fetch(kn);                      // in flight while this row is used
        const double hk = slot[2 * p], xk = slot[2 * p + 1], d = dg[k];
        double xn = xk;
        if (d > 0.0 && __builtin_isfinite(d)) xn = fmax(0.0, xk + (bb[k] - hk) / d);
        const double delta = xn - xk;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int l = tid + s * CS_THREADS;
            if (delta != 0.0 && l < K) h[s] += delta * cur[s];
            if (l == k) x[k] = xn;
            if (l == kn) slot[2 * (1 - p)] = h[s], slot[2 * (1 - p) + 1] = (kn == k) ? xn : x[kn];
        }
        __syncthreads();
        k = kn;
    }
    // the projected gradient, and the colours rounded once
    double m = 0.0;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int l = tid + s * CS_THREADS;
        if (l < K) {
            const double gl = h[s] - bb[l], xl = x[l];
            m = fmax(m, fabs(xl > 0.0 ? gl : fmin(gl, 0.0)));
            if (a.sweeps > 0) a.out[(size_t)c * K + l] = (float)xl;
        }
    }
    m = block_reduce<CS_THREADS>(m, OpFmax(), red);
    if (tid == 0) a.kkt[c] = m, a.ok[c] = 1;
}

template <int SLOTS, bool LDSM>
int solve_launch(const char *fn, const SolveArgs &a, int NC, hipStream_t st) {
    const size_t lds = solve_lds(a.K);
    if (lds > 48u * 1024u) {   // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void *)colour_solve_kernel<SLOTS, LDSM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return fail((int)e, "%s: %zu bytes of LDS: %s", fn, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL((colour_solve_kernel<SLOTS, LDSM>), dim3((unsigned)NC), dim3(CS_THREADS), lds, st, a);
    return check_launch(fn);
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_colour_normal_eqs_workspace(int K, int NC, int B) {
    dnmf::ColourPlan g;
    if (dnmf::colour_plan("dnmf_colour_normal_eqs_workspace", K, NC, B, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_colour_normal_eqs(const float *G, const float *r, const float *C, long ldc, int K, int NC, int B, int first, int finish,
                           void *state, size_t state_bytes, double *M, double *b, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_colour_normal_eqs";
    DNMF_REQUIRE(G && r && C && state, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE((M && b) || !finish, DNMF_E_NULL, "%s: M or b is NULL with finish", fn);
    ColourPlan g;
    const int rc = colour_plan(fn, K, NC, B, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldc >= B, DNMF_E_SHAPE, "%s: ldc=%ld below a row of B=%d", fn, ldc, B);
    DNMF_REQUIRE(state_bytes >= g.bytes, DNMF_E_WORKSPACE, "%s: state of %zu bytes, need %zu", fn, state_bytes, g.bytes);
    DNMF_REQUIRE(((size_t)state & 7) == 0, DNMF_E_WORKSPACE, "%s: state must be 8-byte aligned", fn);
    char *ws = static_cast<char *>(state);
    NormalArgs a;
    a.G = G, a.r = r, a.C = C, a.ldc = ldc;
    a.K = K, a.NC = NC, a.B = B, a.ntl = g.ntl, a.ntiles = g.ntiles, a.nbt = g.nbt, a.first = first != 0, a.finish = finish != 0;
    a.done = reinterpret_cast<const long *>(ws);
    a.acc = reinterpret_cast<double *>(ws + CN_HEADER), a.open = a.acc + g.slab, a.part = a.open + g.slab;
    a.slab = g.slab, a.E = g.E;
    a.M = M, a.b = b;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(colour_accumulate_kernel, dim3((unsigned)g.units, (unsigned)g.cap), dim3(CN_THREADS), 0, st, a);
    hipLaunchKernelGGL(colour_finish_kernel, dim3((unsigned)((g.E + CN_THREADS - 1) / CN_THREADS)), dim3(CN_THREADS), 0, st, a);
    hipLaunchKernelGGL(colour_count_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<long *>(ws), a.first, B);
    return check_launch(fn);
}

int dnmf_colour_solve(const double *M, const double *b, const float *colours, int K, int NC, int sweeps, float *out, double *kkt,
                      int *ok, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_colour_solve";
    DNMF_REQUIRE(M && b && colours && kkt && ok, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(K >= 1 && NC >= 1 && sweeps >= 0, DNMF_E_SHAPE, "%s: K=%d neurons, NC=%d channels, sweeps=%d", fn, K, NC, sweeps);
    DNMF_REQUIRE(out || sweeps == 0, DNMF_E_NULL, "%s: out is NULL with sweeps=%d", fn, sweeps);
    DNMF_REQUIRE(K <= COLOUR_MAX_K && NC <= COLOUR_MAX_NC, DNMF_E_UNSUPPORTED, "%s: K=%d (<= %d), NC=%d (<= %d)", fn, K, COLOUR_MAX_K, NC,
                 COLOUR_MAX_NC);
    SolveArgs a;
    a.M = M, a.b = b, a.colours = colours, a.K = K, a.sweeps = sweeps, a.out = out, a.kkt = kkt, a.ok = ok;
    const hipStream_t st = (hipStream_t)stream;
    if (K <= CS_LDS_MAX_K) return solve_launch<1, true>(fn, a, NC, st);
    const int per_lane = (K + CS_THREADS - 1) / CS_THREADS;
    if (per_lane <= 1) return solve_launch<1, false>(fn, a, NC, st);
    if (per_lane <= 2) return solve_launch<2, false>(fn, a, NC, st);
    if (per_lane <= 4) return solve_launch<4, false>(fn, a, NC, st);
    if (per_lane <= 8) return solve_launch<8, false>(fn, a, NC, st);
    return solve_launch<16, false>(fn, a, NC, st);
}

}  // extern "C"
