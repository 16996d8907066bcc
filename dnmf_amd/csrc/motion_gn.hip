// K16 -- the per-frame normal equations of the motion fit, and the Levenberg-Marquardt step that uses them.
//
// The motion loss sum_t sum_v (A_tC(v) - y_t(v))^2 is a sum over frames, and frame t only sees beta[:, :, t]: 30 unknowns
// (12 at Z = 1) against P residuals.  With r(v) = A_tC(v) - y(v), g_d(v) = d A_tC / d q_d (v) -- both exactly K2's, same
// warp, same normalise / un-normalise round trip, same taps from the halo layout -- and the CENTRED quadratic basis
//   phi(v) = quadratic_basis(u(v)),   u_d = 2 x_d / (S_d - 1) - 1   (u_d = 0 on an axis of one voxel)
// the Jacobian row of voxel v is J(v)[a,d] = phi_a(v) g_d(v), and per frame
//   H = sum_v J^T J (30,30),   g = sum_v J^T r (30),   sse = sum_v r^2,        parameter index a*3 + d.
// Centred coordinates keep every monomial in [-1, 1]: in voxel monomials H has entries up to 511^4 beside entries of
// order 1 and is useless in fp32.  tests/gn_restatement.py is the definition in float64.
//
// Kernel shape: K2's work layout (warp_taps.hpp) -- a lane owns one position of the (y,z) plane (both slices of it at
// Z == 2) and walks down PLANE_ROWS consecutive x.  u_y and u_z are constant along the walk, so a thread only accumulates moments over x:
// sum g_d g_e u_x^m (m = 0..4) and sum r g_d u_x^m (m = 0..2): 15 + 6 + 1 sums at Z = 1, 30 + 9 + 1 per slice at Z > 1.
// phi_a phi_b is a monomial of degree <= 4 in u, so the DISTINCT sums behind H are (monomials of degree <= 4) x (pairs
// d <= e): 15 x 3 = 45 at Z = 1, 35 x 6 = 210 at Z > 1; behind g (degree <= 2) x d: 12 / 30.  A thread expands its moments
// into those (a product with powers of its u_y, u_z), the block reduces them (DPP tree per wave, four waves through
// LDS) and writes one row of partial sums; the finish kernel adds the rows of a frame in float64 and only there
// spreads them into the full symmetric matrix.
#include "warp_taps.hpp"

namespace dnmf {

// monomials u_x^i u_y^j u_z^k of degree <= DEG in NDIM variables, numbered i outermost, k innermost
template <int NDIM, int DEG>
__host__ __device__ constexpr int mono_count() {
    int n = 0;
    for (int i = 0; i <= DEG; ++i)
        for (int j = 0; j <= DEG - i; ++j)
            for (int k = 0; k <= (NDIM == 3 ? DEG - i - j : 0); ++k) ++n;
    return n;
}
template <int NDIM, int DEG>
__host__ __device__ constexpr int mono_index(int ei, int ej, int ek) {
    int n = 0;
    for (int i = 0; i <= DEG; ++i)
        for (int j = 0; j <= DEG - i; ++j)
            for (int k = 0; k <= (NDIM == 3 ? DEG - i - j : 0); ++k) {
                if (i == ei && j == ej && k == ek) return n;
                ++n;
            }
    return -1;
}

// layout of one row of sums: [pair (d <= e)][monomial of degree <= 4], then [d][monomial of degree <= 2], then sse
template <int NDIM>
struct GnSums {
    static constexpr int ND = NDIM;
    static constexpr int NP = NDIM * (NDIM + 1) / 2;
    static constexpr int NM4 = mono_count<NDIM, 4>();
    static constexpr int NM2 = mono_count<NDIM, 2>();
    static constexpr int G0 = NP * NM4;
    static constexpr int SSE = G0 + NDIM * NM2;
    static constexpr int NS = SSE + 1;
    __host__ __device__ static constexpr int pair(int d, int e) { return d * NDIM - d * (d - 1) / 2 + (e - d); }   // d <= e
};
static_assert(GnSums<2>::NS == 45 + 12 + 1 && GnSums<3>::NS == 210 + 30 + 1, "the sums a block reduces");
static_assert(GnSums<3>::NS <= PLANE_COLS, "one thread per sum writes the block's row");

// u = coordinate * s + o per axis: s = 2 / (S - 1), o = -1 (s = o = 0 on an axis of one voxel)
struct Centre {
    float s[3], o[3];
};

// (x, x*x, u_x, u_x^2) for every x of the volume (scalar loads in the main kernel)
__global__ void k16_xtab_kernel(float4 *__restrict__ xtab, int X) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < X) {
        const float xf = (float)x;
        const float u = X > 1 ? (float)(2.0 * (double)x / (double)(X - 1) - 1.0) : 0.0f;
        xtab[x] = make_float4(xf, __fmul_rn(xf, xf), u, u * u);
    }
}

// ZM = 1: Z == 1 (two coordinates, four taps, the z terms left out); 2: Z == 2 (a lane owns both slices, their z-pairs
// are one 16-byte gather per x-corner); 3: Z > 2.  The sample and its derivative are the code K2 calls (warp_taps.hpp), with
// the wave-uniform choice of the division shortcut and the integer tap offsets.
template <int ZM>
__global__ __launch_bounds__(256) void warp_normal_eqs_kernel(const float *__restrict__ S, long lds, const int *__restrict__ s_ids,
                                                              const float *__restrict__ frames, long ldf,
                                                              const int *__restrict__ frame_ids, Volume vol, HaloLayout hl,
                                                              Centre cen, const float *__restrict__ beta, int T,
                                                              const int *__restrict__ times, float *__restrict__ partial,
                                                              const float4 *__restrict__ xtab, int nub) {
    constexpr bool HASZ = ZM > 1;
    constexpr bool ZPAIR = ZM == 2;
    constexpr int NV = ZPAIR ? 2 : 1;
    using L = GnSums<HASZ ? 3 : 2>;
    constexpr int ND = L::ND, NP = L::NP;
    const int b = blockIdx.y;
    float *__restrict__ prow = partial + ((long)b * gridDim.x + blockIdx.x) * L::NS;
    float bt[30];
    load_beta(beta, T, times[b], bt);
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 30; ++i) finite = finite && bt[i] - bt[i] == 0.0f;   // false for NaN and +-inf
    if (!finite) {   // block-uniform: nothing is gathered; H and g get zeros, sse a NaN
        if ((int)threadIdx.x < L::NS) prow[threadIdx.x] = (int)threadIdx.x == L::SSE ? __builtin_nanf("") : 0.0f;
        return;
    }
    const char *__restrict__ s = reinterpret_cast<const char *>(S + (long)(s_ids ? s_ids[b] : b) * lds);
    const float *__restrict__ y = frames + (long)(frame_ids ? frame_ids[b] : b) * ldf;

    float hm[NV][NP][5], gm[NV][ND][3];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int m = 0; m < 5; ++m) hm[v][p][m] = 0.0f;
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int m = 0; m < 3; ++m) gm[v][d][m] = 0.0f;
    }
    float sq = 0.0f;
    const int YZ = vol.Y * vol.Z;
    const int plane = ZPAIR ? vol.Y : YZ;
    const int bu = blockIdx.x % nub, bx = blockIdx.x / nub;
    const int u = bu * PLANE_COLS + threadIdx.x;        // position in the (y,z) plane; Z == 2: y
    const int yy = ZM == 3 ? div_small(u, vol.Z, vol.rcp_z) : u;
    const int z = ZM == 3 ? u - yy * vol.Z : 0;
    const float yf = (float)yy, zf = (float)z;

    if (u < plane) {
        float b2[30];
        double_beta(bt, b2);
        Monomials<true> mono[NV];   // y, z, y^2, z^2, yz of the lane's voxels: fixed along the rows
#pragma unroll
        for (int v = 0; v < NV; ++v) mono[v] = monomials<true>(0.0f, yf, ZPAIR ? (float)v : zf);
        const int x_first = bx * PLANE_ROWS;
        const int nrow = min(PLANE_ROWS, vol.X - x_first);
        const unsigned u4 = (unsigned)u * (4u * NV);
        for (int i = 0; i < nrow; ++i) {
            const float4 xt = xtab[x_first + i];
            const float ux = xt.z, ux2 = xt.w, ux3 = ux2 * ux, ux4 = ux2 * ux2;
            const float xy = __fmul_rn(xt.x, yf);
            const char *op = reinterpret_cast<const char *>(y + (long)(x_first + i) * YZ) + u4;
            float other[NV];
            if constexpr (ZPAIR) {
                const float2 o2 = *reinterpret_cast<const float2 *>(op);   // (x, y, 0), (x, y, 1)
                other[0] = o2.x, other[NV - 1] = o2.y;
            } else {
                other[0] = *reinterpret_cast<const float *>(op);
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                WarpTaps<HASZ> q;
                const unsigned olo = warp_taps_front<ZM, -1, false>(b2, mono[v], xt.x, xt.y, xy, vol, hl, q);
                gather_tap_row<ZM>(s, olo, hl, q.t[0]);
                gather_tap_row<ZM>(s, olo + (unsigned)hl.row4, hl, q.t[1]);
                float rec, g[3];
                blend_taps<HASZ>(q, rec, g);
                const float resid = rec - other[v];
                sq = fmaf(resid, resid, sq);
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const float rg = resid * g[d];
                    gm[v][d][0] += rg;
                    gm[v][d][1] = fmaf(ux, rg, gm[v][d][1]);
                    gm[v][d][2] = fmaf(ux2, rg, gm[v][d][2]);
#pragma unroll
                    for (int e = d; e < ND; ++e) {
                        const float gg = g[d] * g[e];
                        float(&h)[5] = hm[v][L::pair(d, e)];
                        h[0] += gg;
                        h[1] = fmaf(ux, gg, h[1]);
                        h[2] = fmaf(ux2, gg, h[2]);
                        h[3] = fmaf(ux3, gg, h[3]);
                        h[4] = fmaf(ux4, gg, h[4]);
                    }
                }
            }
        }
    }

    // a thread's share of every distinct sum: its x-moments times powers of its u_y, u_z; then the block reduction
    // (wave_sum_last: a DPP tree, total in lane 63; the four waves' totals through LDS)
    __shared__ float red[4][L::NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float py[5], pz[NV][5];
    {
        const float uy = fmaf(yf, cen.s[1], cen.o[1]);
        py[0] = 1.0f;
#pragma unroll
        for (int j = 1; j < 5; ++j) py[j] = py[j - 1] * uy;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float uz = HASZ ? fmaf(ZPAIR ? (float)v : zf, cen.s[2], cen.o[2]) : 0.0f;
            pz[v][0] = 1.0f;
#pragma unroll
            for (int k = 1; k < 5; ++k) pz[v][k] = pz[v][k - 1] * uz;
        }
    }
    {
        int n = 0;
#pragma unroll
        for (int i = 0; i <= 4; ++i)
#pragma unroll
            for (int j = 0; j <= 4 - i; ++j)
#pragma unroll
                for (int k = 0; k <= (HASZ ? 4 - i - j : 0); ++k) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        float val = 0.0f;
#pragma unroll
                        for (int v = 0; v < NV; ++v) val = fmaf(py[j] * pz[v][k], hm[v][p][i], val);
                        val = wave_sum_last(val);
                        if (lane == 63) red[wave][p * L::NM4 + n] = val;
                    }
                    ++n;
                }
        n = 0;
#pragma unroll
        for (int i = 0; i <= 2; ++i)
#pragma unroll
            for (int j = 0; j <= 2 - i; ++j)
#pragma unroll
                for (int k = 0; k <= (HASZ ? 2 - i - j : 0); ++k) {
#pragma unroll
                    for (int d = 0; d < ND; ++d) {
                        float val = 0.0f;
#pragma unroll
                        for (int v = 0; v < NV; ++v) val = fmaf(py[j] * pz[v][k], gm[v][d][i], val);
                        val = wave_sum_last(val);
                        if (lane == 63) red[wave][L::G0 + d * L::NM2 + n] = val;
                    }
                    ++n;
                }
        const float v = wave_sum_last(sq);
        if (lane == 63) red[wave][L::SSE] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < L::NS)
        prow[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// exponents of the quadratic basis [1, x, y, z, x^2, y^2, z^2, xy, xz, yz]
__device__ constexpr int GN_EX[10] = {0, 1, 0, 0, 2, 0, 0, 1, 1, 0};
__device__ constexpr int GN_EY[10] = {0, 0, 1, 0, 0, 2, 0, 1, 0, 1};
__device__ constexpr int GN_EZ[10] = {0, 0, 0, 1, 0, 0, 2, 0, 1, 1};

// One block per frame: the block rows of the frame added in float64 (fixed order), then spread into H (30,30), g (30), sse.
// NDIM = 2 (Z == 1): entries of an unknown with z in its basis term or d == 2 are exact zeros.
template <int NDIM>
__global__ __launch_bounds__(256) void warp_normal_eqs_finish_kernel(const float *__restrict__ partial, int nblk,
                                                                     double *__restrict__ H, double *__restrict__ g,
                                                                     double *__restrict__ sse, int accumulate) {
    using L = GnSums<NDIM>;
    __shared__ double tot[L::NS];
    const int b = blockIdx.x, j = threadIdx.x;
    if (j < L::NS) {
        const float *src = partial + (long)b * nblk * L::NS + j;
        double s0 = 0.0;
        for (int k = 0; k < nblk; ++k) s0 += (double)src[(long)k * L::NS];
        tot[j] = s0;
    }
    __syncthreads();
    auto active = [](int a, int d) { return NDIM == 3 || (GN_EZ[a] == 0 && d < 2); };
    for (int idx = j; idx < 900; idx += 256) {
        const int r = idx / 30, c = idx - r * 30;
        const int a = r / 3, d = r - a * 3, a2 = c / 3, e = c - a2 * 3;
        double val = 0.0;
        if (active(a, d) && active(a2, e)) {
            const int m = mono_index<NDIM, 4>(GN_EX[a] + GN_EX[a2], GN_EY[a] + GN_EY[a2], GN_EZ[a] + GN_EZ[a2]);
            val = tot[L::pair(d < e ? d : e, d < e ? e : d) * L::NM4 + m];
        }
        double *dst = H + (long)b * 900 + idx;
        *dst = accumulate ? *dst + val : val;
    }
    if (j < 30) {
        const int a = j / 3, d = j - a * 3;
        const double val = active(a, d) ? tot[L::G0 + d * L::NM2 + mono_index<NDIM, 2>(GN_EX[a], GN_EY[a], GN_EZ[a])] : 0.0;
        g[(long)b * 30 + j] = accumulate ? g[(long)b * 30 + j] + val : val;
    }
    if (j == 32) sse[b] = accumulate ? sse[b] + tot[L::SSE] : tot[L::SSE];
}

// ---- the Levenberg-Marquardt step ----------------------------------------------------------------------------------
// active unknowns: all 30, or at Z == 1 the 12 without z: lm_act(nfull, i) = parameter index of the i-th.  Both lists go up
// by the degree of the basis term, so the unknowns of a warp order (K16o) are the first lm_order_count of them.
__device__ __forceinline__ int lm_act(int nfull, int i) {
    if (nfull == 30) return i;
    constexpr int AZ[6] = {0, 1, 2, 4, 5, 7};
    return AZ[i >> 1] * 3 + (i & 1);
}

// The damped solve the step kernels end with, by the one wave of the block (all 64 threads call it, after a barrier that
// follows the last write of Ha / ga / bacc):  (H' + l diag(H') + tiny I) delta = -g' on the first nact of the nfull (30 or 12)
// active unknowns, scaled to a unit diagonal, float64 Cholesky, two triangular solves, d beta = M delta, beta[:, :, t] =
// fp32(bacc + d beta).  H' = Ha, g' = ga; with PRIOR, H' = Ha + hadd I and g' = ga + gadd (gadd: 30 doubles in LDS by parameter
// index) on those unknowns.  Ha, ga and bacc are the state the calling kernel has just written: plain pointers, nothing here
// may be read as invariant.
template <bool PRIOR>
__device__ void lm_damped_solve(const double *Ha, const double *ga, double l, int nact, int nfull, const double *__restrict__ M,
                                const float *bacc, float *beta, int T, int t, double hadd, const double *gadd) {
    __shared__ double A[30][31];
    __shared__ double rhs[30], sc[30], dl[30];
    __shared__ int okflag;
    const int j = threadIdx.x;
    auto act = [nfull](int i) { return lm_act(nfull, i); };
    auto diag = [&](int i) {
        if constexpr (PRIOR) return Ha[act(i) * 31] + hadd;
        else return Ha[act(i) * 31];
    };
    if (j == 0) okflag = 1;
    double hmax = 0.0;
    for (int i = 0; i < nact; ++i) hmax = fmax(hmax, diag(i));
    const double tiny = 1e-12 * hmax + 1e-30;
    // (H + lam diag(H) + tiny I) delta = -g, scaled to a unit diagonal: sc = 1 / sqrt(diagonal)
    if (j < nact) {
        const double dd = diag(j) * (1.0 + l) + tiny;
        sc[j] = 1.0 / sqrt(dd);
    }
    __syncthreads();
    if (j < nact) {
        for (int c = 0; c < nact; ++c) {
            double v = Ha[act(j) * 30 + act(c)];
            if constexpr (PRIOR)
                if (c == j) v += hadd;
            if (c == j) v = v * (1.0 + l) + tiny;
            A[j][c] = v * sc[j] * sc[c];
        }
        if constexpr (PRIOR) rhs[j] = -(ga[act(j)] + gadd[act(j)]) * sc[j];
        else rhs[j] = -ga[act(j)] * sc[j];
    }
    __syncthreads();
    // Cholesky A = L L^T in place (lower triangle), row j owned by thread j
    for (int k = 0; k < nact; ++k) {
        if (j == 0) {
            const double piv = A[k][k];
            if (!(piv > 0.0) || !(piv - piv == 0.0)) okflag = 0;
            A[k][k] = sqrt(piv);
        }
        __syncthreads();
        if (!okflag) break;
        if (j > k && j < nact) A[j][k] /= A[k][k];
        __syncthreads();
        if (j > k && j < nact)
            for (int c = k + 1; c <= j; ++c) A[j][c] -= A[j][k] * A[c][k];
        __syncthreads();
    }
    if (j == 0) {
        if (okflag) {
            for (int i = 0; i < nact; ++i) {       // L w = rhs
                double v = rhs[i];
                for (int c = 0; c < i; ++c) v -= A[i][c] * rhs[c];
                rhs[i] = v / A[i][i];
            }
            for (int i = nact - 1; i >= 0; --i) {  // L^T y = w
                double v = rhs[i];
                for (int c = i + 1; c < nact; ++c) v -= A[c][i] * rhs[c];
                rhs[i] = v / A[i][i];
            }
        }
        for (int i = 0; i < 30; ++i) dl[i] = 0.0;
        if (okflag)
            for (int i = 0; i < nact; ++i) dl[act(i)] = rhs[i] * sc[i];
    }
    __syncthreads();
    if (j < 30) {   // delta (centred basis) -> d beta = M delta, per coordinate d
        const int a = j / 3, d = j - a * 3;
        double db = 0.0;
        for (int c = 0; c < 10; ++c) db += M[a * 10 + c] * dl[c * 3 + d];
        beta[(long)j * T + t] = (float)((double)bacc[j] + db);
    }
}

// One wave per frame, float64, everything on the device.  State of frame b: the accepted coefficients beta_acc (30 floats,
// [a*3+d]), their H / g / sse, the damping lam, sse0 (the first evaluation) and counts = (accepted, rejected, initialised).
// The trial coefficients live in beta (10,3,T) at column times[b], where K16 reads them.
__global__ __launch_bounds__(64) void lm_step_kernel(const double *__restrict__ H, const double *__restrict__ g,
                                                     const double *__restrict__ sse, int nact, const double *__restrict__ M,
                                                     float *__restrict__ beta, int T, const int *__restrict__ times,
                                                     double *__restrict__ Hacc, double *__restrict__ gacc,
                                                     double *__restrict__ sse_acc, double *__restrict__ sse0,
                                                     double *__restrict__ lam, float *__restrict__ beta_acc,
                                                     int *__restrict__ counts, double nu, double lam0, double lam_min,
                                                     double lam_max, int accept_only) {
    const int b = blockIdx.x, j = threadIdx.x, t = times[b];
    const bool first = counts[b * 3 + 2] == 0;
    const double st = sse[b], sa = sse_acc[b];
    const bool accept = first || (st - st == 0.0 && st < sa);   // finite and below
    double l = first ? lam0 : lam[b];
    if (!first) l = accept ? fmax(l / nu, lam_min) : fmin(l * nu, lam_max);
    __syncthreads();   // every thread has read the state before it changes
    if (accept) {
        for (int i = j; i < 900; i += 64) Hacc[(long)b * 900 + i] = H[(long)b * 900 + i];
        if (j < 30) {
            gacc[b * 30 + j] = g[b * 30 + j];
            beta_acc[b * 30 + j] = beta[(long)j * T + t];
        }
    }
    if (j == 0) {
        lam[b] = l;
        if (accept) sse_acc[b] = st;
        if (first) sse0[b] = st, counts[b * 3 + 2] = 1;
        else counts[b * 3 + (accept ? 0 : 1)] += 1;
    }
    __syncthreads();
    if (accept_only) {
        if (j < 30) beta[(long)j * T + t] = beta_acc[b * 30 + j];
        return;
    }
    lm_damped_solve<false>(Hacc + (long)b * 900, gacc + b * 30, l, nact, nact, M, beta_acc + b * 30, beta, T, t, 0.0, nullptr);
}

// K16s: the step with the temporal prior m sum_{s in N_t} |theta_t - theta_s|^2, theta = Minv beta per coordinate on the active
// unknowns, N_t = the frames t +- 1 inside [0, T) whose column of beta_ref (every frame's ACCEPTED coefficients) is finite.
// Both sides of the accept test carry their prior against the CURRENT beta_ref; on accept the trial's column goes to beta_ref.
// A neighbour's theta is 10 x 10 x (2 or 3) FMAs from its fp32 column: computed here, kept in LDS, never stored.  The frames of
// a launch are pairwise non-adjacent (the caller's contract): no block reads a column another block writes.
__global__ __launch_bounds__(64) void lm_step_smooth_kernel(const double *__restrict__ H, const double *__restrict__ g,
                                                            const double *__restrict__ sse, int nact,
                                                            const double *__restrict__ M, const double *__restrict__ Minv,
                                                            float *__restrict__ beta, int T, const int *__restrict__ times,
                                                            double *__restrict__ Hacc, double *__restrict__ gacc,
                                                            double *__restrict__ sse_acc, double *__restrict__ sse0,
                                                            double *__restrict__ lam, float *__restrict__ beta_acc,
                                                            int *__restrict__ counts, double nu, double lam0, double lam_min,
                                                            double lam_max, int accept_only, float *beta_ref, double m,
                                                            double *__restrict__ prior) {
    __shared__ double thn[2][30];       // theta of the neighbours in use
    __shared__ double sq[2][30];        // squared distances to them: [0] of the trial, [1] of the accepted point
    __shared__ double gadd[30];
    const int b = blockIdx.x, j = threadIdx.x, t = times[b];
    const int a = j / 3, d = j - a * 3;
    const bool unknown = j < 30 && (nact == 30 || (GN_EZ[a] == 0 && d < 2));
    const bool first = counts[b * 3 + 2] == 0;
    // theta of a column held with stride ld between its 30 entries; exact zero on an inactive unknown
    auto theta = [&](const float *col, long ld) {
        double v = 0.0;
        if (unknown)
            for (int c = 0; c < 10; ++c) v = fma(Minv[a * 10 + c], (double)col[(long)(c * 3 + d) * ld], v);
        return v;
    };
    int nn = 0;                         // block-uniform
    if (m != 0.0) {
        for (int side = -1; side <= 1; side += 2) {
            const int s = t + side;
            if (s < 0 || s >= T) continue;
            const float v = j < 30 ? beta_ref[(long)j * T + s] : 0.0f;
            if (!__all(v - v == 0.0f)) continue;    // a column with a NaN or an inf is no neighbour
            if (j < 30) thn[nn][j] = theta(beta_ref + s, T);
            ++nn;
        }
    }
    const double th_trial = theta(beta + t, T);
    const double th_old = first ? 0.0 : theta(beta_acc + b * 30, 1);
    __syncthreads();
    if (j < 30) {
        double qt = 0.0, qa = 0.0;
        for (int i = 0; i < nn; ++i) {
            const double dt = th_trial - thn[i][j], da = th_old - thn[i][j];
            qt += dt * dt, qa += da * da;
        }
        sq[0][j] = qt, sq[1][j] = qa;
    }
    __syncthreads();
    double p_trial = 0.0, p_acc = 0.0;
    if (nn > 0) {                       // every thread adds the 30 terms in the same order: one value in the whole wave
        for (int i = 0; i < 30; ++i) p_trial += sq[0][i], p_acc += sq[1][i];
        p_trial *= m, p_acc *= m;
    }
    const double st = sse[b], sa = sse_acc[b];
    const double ft = st + p_trial, fa = sa + p_acc;
    const bool accept = first || (ft - ft == 0.0 && ft < fa);   // finite and below
    double l = first ? lam0 : lam[b];
    if (!first) l = accept ? fmax(l / nu, lam_min) : fmin(l * nu, lam_max);
    __syncthreads();   // every thread has read the state before it changes
    if (accept) {
        for (int i = j; i < 900; i += 64) Hacc[(long)b * 900 + i] = H[(long)b * 900 + i];
        if (j < 30) {
            const float bt = beta[(long)j * T + t];
            gacc[b * 30 + j] = g[b * 30 + j];
            beta_acc[b * 30 + j] = bt;
            beta_ref[(long)j * T + t] = bt;
        }
    }
    if (j < 30) {
        const double th = accept ? th_trial : th_old;
        double ga = 0.0;
        for (int i = 0; i < nn; ++i) ga += th - thn[i][j];
        gadd[j] = m * ga;
    }
    if (j == 0) {
        lam[b] = l;
        prior[b] = accept ? p_trial : p_acc;
        if (accept) sse_acc[b] = st;
        if (first) sse0[b] = st, counts[b * 3 + 2] = 1;
        else counts[b * 3 + (accept ? 0 : 1)] += 1;
    }
    __syncthreads();
    if (accept_only) {
        if (j < 30) beta[(long)j * T + t] = beta_acc[b * 30 + j];
        return;
    }
    lm_damped_solve<true>(Hacc + (long)b * 900, gacc + b * 30, l, nact, nact, M, beta_acc + b * 30, beta, T, t, m * (double)nn,
                          gadd);
}

// K16o: the step on the unknowns of one warp order -- the rows of the centred basis of degree <= order (0: row 0, 1: rows
// 0 .. 3, 2: all ten) without the z rows and the z component at Z == 1.  lm_order_count of the nfull active unknowns.
__device__ __forceinline__ int lm_order_count(int nfull, int order) {
    const int rows = nfull == 30 ? (order == 0 ? 1 : order == 1 ? 4 : 10) : (order == 0 ? 1 : order == 1 ? 3 : 6);
    return rows * (nfull == 30 ? 3 : 2);
}

// lm_step_smooth_kernel over that set: K16's H and g are taken whole and restricted here, so the damped system, its diagonal
// scaling and tiny, the prior (theta, both sides of the accept test, hadd and gadd) all see the selected unknowns only, and the
// bookkeeping is the same.  M takes centred terms of a degree to raw rows of that degree or lower, so d beta is an exact zero
// on the rows above the order; they are put back from beta_acc all the same, which makes "untouched" a matter of bits (-0.0,
// a NaN's payload) and not of arithmetic.  m == 0: no prior, Minv / beta_ref / prior are not read (they may be NULL) and the
// solve is lm_step_kernel's instantiation; order == 2 is then lm_step_kernel, and with m != 0 lm_step_smooth_kernel, step for step.
__global__ __launch_bounds__(64) void lm_step_order_kernel(const double *__restrict__ H, const double *__restrict__ g,
                                                           const double *__restrict__ sse, int nfull, int order,
                                                           const double *__restrict__ M, const double *__restrict__ Minv,
                                                           float *__restrict__ beta, int T, const int *__restrict__ times,
                                                           double *__restrict__ Hacc, double *__restrict__ gacc,
                                                           double *__restrict__ sse_acc, double *__restrict__ sse0,
                                                           double *__restrict__ lam, float *__restrict__ beta_acc,
                                                           int *__restrict__ counts, double nu, double lam0, double lam_min,
                                                           double lam_max, int accept_only, float *beta_ref, double m,
                                                           double *__restrict__ prior) {
    __shared__ double thn[2][30];       // theta of the neighbours in use
    __shared__ double sq[2][30];        // squared distances to them: [0] of the trial, [1] of the accepted point
    __shared__ double gadd[30];
    const int b = blockIdx.x, j = threadIdx.x, t = times[b];
    const int a = j / 3, d = j - a * 3;
    const int nact = lm_order_count(nfull, order);
    const bool unknown = j < 30 && GN_EX[a] + GN_EY[a] + GN_EZ[a] <= order && (nfull == 30 || (GN_EZ[a] == 0 && d < 2));
    const bool first = counts[b * 3 + 2] == 0;
    // theta of a column held with stride ld between its 30 entries; exact zero outside the selected unknowns
    auto theta = [&](const float *col, long ld) {
        double v = 0.0;
        if (unknown)
            for (int c = 0; c < 10; ++c) v = fma(Minv[a * 10 + c], (double)col[(long)(c * 3 + d) * ld], v);
        return v;
    };
    int nn = 0;                         // block-uniform
    double th_trial = 0.0, th_old = 0.0, p_trial = 0.0, p_acc = 0.0;
    if (m != 0.0) {
        for (int side = -1; side <= 1; side += 2) {
            const int s = t + side;
            if (s < 0 || s >= T) continue;
            const float v = j < 30 ? beta_ref[(long)j * T + s] : 0.0f;
            if (!__all(v - v == 0.0f)) continue;    // a column with a NaN or an inf is no neighbour
            if (j < 30) thn[nn][j] = theta(beta_ref + s, T);
            ++nn;
        }
        th_trial = theta(beta + t, T);
        th_old = first ? 0.0 : theta(beta_acc + b * 30, 1);
        __syncthreads();
        if (j < 30) {
            double qt = 0.0, qa = 0.0;
            for (int i = 0; i < nn; ++i) {
                const double dt = th_trial - thn[i][j], da = th_old - thn[i][j];
                qt += dt * dt, qa += da * da;
            }
            sq[0][j] = qt, sq[1][j] = qa;
        }
        __syncthreads();
        if (nn > 0) {                   // every thread adds the 30 terms in the same order: one value in the whole wave
            for (int i = 0; i < 30; ++i) p_trial += sq[0][i], p_acc += sq[1][i];
            p_trial *= m, p_acc *= m;
        }
    }
    const double st = sse[b], sa = sse_acc[b];
    const double ft = st + p_trial, fa = sa + p_acc;
    const bool accept = first || (ft - ft == 0.0 && ft < fa);   // finite and below
    double l = first ? lam0 : lam[b];
    if (!first) l = accept ? fmax(l / nu, lam_min) : fmin(l * nu, lam_max);
    __syncthreads();   // every thread has read the state before it changes
    if (accept) {
        for (int i = j; i < 900; i += 64) Hacc[(long)b * 900 + i] = H[(long)b * 900 + i];
        if (j < 30) {
            const float bt = beta[(long)j * T + t];
            gacc[b * 30 + j] = g[b * 30 + j];
            beta_acc[b * 30 + j] = bt;
            if (m != 0.0) beta_ref[(long)j * T + t] = bt;
        }
    }
    if (m != 0.0 && j < 30) {
        const double th = accept ? th_trial : th_old;
        double ga = 0.0;
        for (int i = 0; i < nn; ++i) ga += th - thn[i][j];
        gadd[j] = m * ga;
    }
    if (j == 0) {
        lam[b] = l;
        if (m != 0.0) prior[b] = accept ? p_trial : p_acc;
        if (accept) sse_acc[b] = st;
        if (first) sse0[b] = st, counts[b * 3 + 2] = 1;
        else counts[b * 3 + (accept ? 0 : 1)] += 1;
    }
    __syncthreads();
    if (accept_only) {
        if (j < 30) beta[(long)j * T + t] = beta_acc[b * 30 + j];
        return;
    }
    if (m != 0.0)
        lm_damped_solve<true>(Hacc + (long)b * 900, gacc + b * 30, l, nact, nfull, M, beta_acc + b * 30, beta, T, t, m * (double)nn,
                              gadd);
    else
        lm_damped_solve<false>(Hacc + (long)b * 900, gacc + b * 30, l, nact, nfull, M, beta_acc + b * 30, beta, T, t, 0.0, nullptr);
    // thread j wrote entry j a moment ago: its own store, in program order
    if (j < 30 && GN_EX[a] + GN_EY[a] + GN_EZ[a] > order) beta[(long)j * T + t] = beta_acc[b * 30 + j];
}

// K16j: the volume-preserving prior.  The map of a frame in centred coordinates is q_d(u) = sum_a basis_a(u) theta[a,d]; its
// Jacobian in voxel coordinates is Jx[d][e] = (sum_a d basis_a / d u_e theta[a,d]) / h_e with h_e = (S_e - 1) / 2, the TRUE
// Jacobian of the model's map (csrc/tracks.hip's, not the reference's log_det_jac with its xz / yz rows swapped).  At the sample
// points -- the corners u in {-1, +1}^n, first axis slowest, then the centre u = 0: 9 points, 5 at Z == 1 -- the residual is
// rho_p = log det Jx(u_p): 0 for the identity, a rigid motion or a shear, +inf where det Jx <= 0 or is not finite.
struct JacHalf {
    double h[3];    // (S_e - 1) / 2; 1 on the z axis at Z == 1 (it is not used there)
};

__device__ __forceinline__ int lm_jac_points(int nfull) { return nfull == 30 ? 9 : 5; }

// sample point p of lm_jac_points(nfull)
__device__ __forceinline__ void lm_jac_point(int nfull, int p, double (&u)[3]) {
    const int nc = nfull == 30 ? 8 : 4;
    u[0] = u[1] = u[2] = 0.0;
    if (p < nc) {
        if (nfull == 30) u[0] = p & 4 ? 1.0 : -1.0, u[1] = p & 2 ? 1.0 : -1.0, u[2] = p & 1 ? 1.0 : -1.0;
        else u[0] = p & 2 ? 1.0 : -1.0, u[1] = p & 1 ? 1.0 : -1.0;
    }
}

// d basis_a / d u_e at u, basis = [1, u0, u1, u2, u0^2, u1^2, u2^2, u0 u1, u0 u2, u1 u2]
__device__ __forceinline__ double lm_jac_dbasis(int a, int e, const double (&u)[3]) {
    const double u0 = u[0], u1 = u[1], u2 = u[2];
    if (e == 0) return a == 1 ? 1.0 : a == 4 ? 2.0 * u0 : a == 7 ? u1 : a == 8 ? u2 : 0.0;
    if (e == 1) return a == 2 ? 1.0 : a == 5 ? 2.0 * u1 : a == 7 ? u0 : a == 9 ? u2 : 0.0;
    return a == 3 ? 1.0 : a == 6 ? 2.0 * u2 : a == 8 ? u0 : a == 9 ? u1 : 0.0;
}

// lm_step_order_kernel with the prior J = mj / NP sum_p rho_p^2 on top (mj == 0: without it): the accept test compares
// sse + temporal prior + J on both sides, so a trial that folds at a sample point (J = +inf) is never accepted after the first call
// and an accepted point that folds is beaten by any admissible trial.  The step adds the exact Gauss-Newton terms
// mj / NP sum_p jrho_p jrho_p^T to H' and mj / NP sum_p rho_p jrho_p to g' at the point kept, jrho_p[a*3+d] = sum_e (Jx^-1)[e][d]
// (d basis_a / d u_e)(u_p) / h_e on the selected unknowns (the value of rho sees the whole map); a point whose rho is not finite
// adds nothing.  The accepted column's rho is recomputed from beta_acc in every call: no state beyond lm_step_order_kernel's.
// The dense H' and g' are staged in LDS and the damped solve is lm_step_kernel's instantiation on them.  Sums over p run in
// the order of p in every thread: no atomics, the same bits on every run.  jac (B): J of the point kept; min_det (B): its smallest
// det Jx over the sample points.
__global__ __launch_bounds__(64) void lm_step_jac_kernel(const double *__restrict__ H, const double *__restrict__ g,
                                                         const double *__restrict__ sse, int nfull, int order,
                                                         const double *__restrict__ M, const double *__restrict__ Minv,
                                                         float *__restrict__ beta, int T, const int *__restrict__ times,
                                                         double *__restrict__ Hacc, double *__restrict__ gacc,
                                                         double *__restrict__ sse_acc, double *__restrict__ sse0,
                                                         double *__restrict__ lam, float *__restrict__ beta_acc,
                                                         int *__restrict__ counts, double nu, double lam0, double lam_min,
                                                         double lam_max, int accept_only, float *beta_ref, double m,
                                                         double *__restrict__ prior, double mj, JacHalf half,
                                                         double *__restrict__ jac, double *__restrict__ min_det) {
    __shared__ double thn[2][30];       // theta of the neighbours in use
    __shared__ double sq[2][30];        // squared distances to them: [0] of the trial, [1] of the accepted point
    __shared__ double thf[2][30];       // theta on every active unknown: [0] the trial, [1] the accepted point
    __shared__ double rho[2][9], dets[2][9], inv[2][9][9];
    __shared__ double jr[9][30];        // jrho_p of the point kept
    __shared__ double Hs[900], gs[30];  // H' and g'
    const int b = blockIdx.x, j = threadIdx.x, t = times[b];
    const int a = j / 3, d = j - a * 3;
    const int nact = lm_order_count(nfull, order);
    const int npts = lm_jac_points(nfull);
    auto selected = [&](int i) {        // parameter index i is an unknown of the order
        const int ai = i / 3, di = i - ai * 3;
        return GN_EX[ai] + GN_EY[ai] + GN_EZ[ai] <= order && (nfull == 30 || (GN_EZ[ai] == 0 && di < 2));
    };
    const bool active = j < 30 && (nfull == 30 || (GN_EZ[a] == 0 && d < 2));
    const bool unknown = j < 30 && selected(j);
    const bool first = counts[b * 3 + 2] == 0;
    // theta of a column held with stride ld between its 30 entries, on every active unknown
    auto theta = [&](const float *col, long ld) {
        double v = 0.0;
        if (active)
            for (int c = 0; c < 10; ++c) v = fma(Minv[a * 10 + c], (double)col[(long)(c * 3 + d) * ld], v);
        return v;
    };
    int nn = 0;                         // block-uniform
    double p_trial = 0.0, p_acc = 0.0;
    const double tf_trial = theta(beta + t, T);
    const double tf_old = first ? 0.0 : theta(beta_acc + b * 30, 1);
    const double th_trial = unknown ? tf_trial : 0.0, th_old = unknown ? tf_old : 0.0;
    if (j < 30) thf[0][j] = tf_trial, thf[1][j] = tf_old;
    if (m != 0.0) {
        for (int side = -1; side <= 1; side += 2) {
            const int s = t + side;
            if (s < 0 || s >= T) continue;
            const float v = j < 30 ? beta_ref[(long)j * T + s] : 0.0f;
            if (!__all(v - v == 0.0f)) continue;    // a column with a NaN or an inf is no neighbour
            if (j < 30) thn[nn][j] = unknown ? theta(beta_ref + s, T) : 0.0;
            ++nn;
        }
    }
    __syncthreads();
    if (m != 0.0 && j < 30) {
        double qt = 0.0, qa = 0.0;
        for (int i = 0; i < nn; ++i) {
            const double dt = th_trial - thn[i][j], da = th_old - thn[i][j];
            qt += dt * dt, qa += da * da;
        }
        sq[0][j] = qt, sq[1][j] = qa;
    }
    // lanes 0 .. npts-1: the trial at point p; lanes 16 .. 16+npts-1: the accepted point
    {
        const int col = j >> 4, p = j & 15;
        if (col < 2 && p < npts) {
            double u[3], J[3][3];
            lm_jac_point(nfull, p, u);
#pragma unroll
            for (int dd = 0; dd < 3; ++dd)
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    double v = 0.0;
#pragma unroll
                    for (int aa = 1; aa < 10; ++aa) v += lm_jac_dbasis(aa, e, u) * thf[col][aa * 3 + dd];
                    J[dd][e] = v / half.h[e];
                }
            if (nfull != 30) J[2][2] = 1.0;     // x and y only: the 2 x 2 determinant and inverse
            const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                         c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
            const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
            const bool ok = det > 0.0 && det - det == 0.0;
            const double r = 1.0 / det;
            double *iv = inv[col][p];           // Jx^-1 [e][d] at e*3+d: the adjugate over the determinant
            iv[0] = c00 * r, iv[3] = c01 * r, iv[6] = c02 * r;
            iv[1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r;
            iv[4] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r;
            iv[7] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r;
            iv[2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r;
            iv[5] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r;
            iv[8] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r;
            dets[col][p] = det;
            rho[col][p] = ok ? log(det) : __builtin_inf();
        }
    }
    __syncthreads();
    if (m != 0.0 && nn > 0) {           // every thread adds the 30 terms in the same order: one value in the whole wave
        for (int i = 0; i < 30; ++i) p_trial += sq[0][i], p_acc += sq[1][i];
        p_trial *= m, p_acc *= m;
    }
    const double wj = mj / (double)npts;
    double j_trial = 0.0, j_acc = 0.0;
    if (mj != 0.0) {
        for (int p = 0; p < npts; ++p) j_trial += rho[0][p] * rho[0][p], j_acc += rho[1][p] * rho[1][p];
        j_trial *= wj, j_acc *= wj;
    }
    const double st = sse[b], sa = sse_acc[b];
    const double ft = (st + p_trial) + j_trial, fa = (sa + p_acc) + j_acc;
    const bool accept = first || (ft - ft == 0.0 && ft < fa);   // finite and below
    const int kept = accept ? 0 : 1;
    double l = first ? lam0 : lam[b];
    if (!first) l = accept ? fmax(l / nu, lam_min) : fmin(l * nu, lam_max);
    double dmin = dets[kept][0];
    for (int p = 1; p < npts; ++p) dmin = dets[kept][p] < dmin || dets[kept][p] != dets[kept][p] ? dets[kept][p] : dmin;
    __syncthreads();   // every thread has read the state before it changes
    if (accept && j < 30) {
        const float bt = beta[(long)j * T + t];
        beta_acc[b * 30 + j] = bt;
        if (m != 0.0) beta_ref[(long)j * T + t] = bt;
    }
    if (j < 30) {       // the rows jrho_p of the point kept and g'
        double gj = 0.0;
        for (int p = 0; p < npts; ++p) {
            const double r = rho[kept][p];
            double v = 0.0;
            if (unknown && r - r == 0.0) {
                double u[3];
                lm_jac_point(nfull, p, u);
#pragma unroll
                for (int e = 0; e < 3; ++e) v += inv[kept][p][e * 3 + d] * (lm_jac_dbasis(a, e, u) / half.h[e]);
                gj += r * v;
            }
            jr[p][j] = v;
        }
        double gv = accept ? g[b * 30 + j] : gacc[b * 30 + j];
        if (accept) gacc[b * 30 + j] = gv;
        if (m != 0.0) {
            const double th = accept ? th_trial : th_old;
            double ga = 0.0;
            for (int i = 0; i < nn; ++i) ga += th - thn[i][j];
            gv += m * ga;
        }
        if (mj != 0.0) gv += wj * gj;
        gs[j] = gv;
    }
    __syncthreads();
    const double hadd = m * (double)nn;
    for (int i = j; i < 900; i += 64) {
        const int r = i / 30, c = i - r * 30;
        double v = accept ? H[(long)b * 900 + i] : Hacc[(long)b * 900 + i];
        if (accept) Hacc[(long)b * 900 + i] = v;
        if (m != 0.0 && r == c && selected(r)) v += hadd;
        if (mj != 0.0) {
            double s = 0.0;
            for (int p = 0; p < npts; ++p) s += jr[p][r] * jr[p][c];
            v += wj * s;
        }
        Hs[i] = v;
    }
    if (j == 0) {
        lam[b] = l;
        if (m != 0.0) prior[b] = accept ? p_trial : p_acc;
        jac[b] = accept ? j_trial : j_acc;
        min_det[b] = dmin;
        if (accept) sse_acc[b] = st;
        if (first) sse0[b] = st, counts[b * 3 + 2] = 1;
        else counts[b * 3 + (accept ? 0 : 1)] += 1;
    }
    __syncthreads();
    if (accept_only) {
        if (j < 30) beta[(long)j * T + t] = beta_acc[b * 30 + j];
        return;
    }
    lm_damped_solve<false>(Hs, gs, l, nact, nfull, M, beta_acc + b * 30, beta, T, t, 0.0, nullptr);
    // thread j wrote entry j a moment ago: its own store, in program order
    if (j < 30 && GN_EX[a] + GN_EY[a] + GN_EZ[a] > order) beta[(long)j * T + t] = beta_acc[b * 30 + j];
}

}  // namespace dnmf

extern "C" {

static int k16_sums(int Z) { return Z > 1 ? dnmf::GnSums<3>::NS : dnmf::GnSums<2>::NS; }

size_t dnmf_warp_normal_eqs_workspace(int X, int Y, int Z, int B) {
    if (X <= 0 || Y <= 0 || Z <= 0 || B <= 0) return 0;
    return dnmf::plane_walk_xtab_bytes<float4>(X) + (size_t)B * dnmf::plane_walk_blocks(X, Y, Z, nullptr) * k16_sums(Z) * sizeof(float);
}

int dnmf_warp_normal_eqs(const float *S, long lds, const int *s_ids, const float *frames, long ldf, const int *frame_ids,
                         int X, int Y, int Z, const float *beta, int T, const int *times, int B, double *H, double *g,
                         double *sse, int accumulate, void *workspace, size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(S && frames && beta && times && H && g && sse && workspace, DNMF_E_NULL, "dnmf_warp_normal_eqs: NULL buffer");
    DNMF_REQUIRE(X > 0 && Y > 0 && Z > 0 && T > 0 && B > 0 && B <= 65535, DNMF_E_SHAPE,
                 "dnmf_warp_normal_eqs: X=%d Y=%d Z=%d T=%d B=%d", X, Y, Z, T, B);
    Volume vol;
    HaloLayout hl;
    int nblk = 0, nub = 0;
    const int rc = plane_walk_geometry("dnmf_warp_normal_eqs", X, Y, Z, vol, hl, nblk, nub);
    if (rc != 0) return rc;
    DNMF_REQUIRE(lds >= hl.Pp && ldf >= vol.P, DNMF_E_SHAPE, "dnmf_warp_normal_eqs: lds=%ld < %ld (halo layout) or ldf=%ld < P=%ld",
                 lds, hl.Pp, ldf, vol.P);
    DNMF_REQUIRE(workspace_bytes >= dnmf_warp_normal_eqs_workspace(X, Y, Z, B), DNMF_E_WORKSPACE,
                 "dnmf_warp_normal_eqs: workspace %zu < %zu bytes", workspace_bytes, dnmf_warp_normal_eqs_workspace(X, Y, Z, B));
    Centre cen;
    const int dims[3] = {X, Y, Z};
    for (int d = 0; d < 3; ++d) {
        cen.s[d] = dims[d] > 1 ? (float)(2.0 / (double)(dims[d] - 1)) : 0.0f;
        cen.o[d] = dims[d] > 1 ? -1.0f : 0.0f;
    }
    float4 *xtab = static_cast<float4 *>(workspace);
    float *partial = reinterpret_cast<float *>(static_cast<char *>(workspace) + plane_walk_xtab_bytes<float4>(X));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k16_xtab_kernel, dim3((unsigned)((X + 255) / 256)), dim3(256), 0, st, xtab, X);
    const dim3 grid((unsigned)nblk, (unsigned)B);
#define DNMF_K16_LAUNCH(ZM)                                                                                                   \
    hipLaunchKernelGGL((warp_normal_eqs_kernel<ZM>), grid, dim3(256), 0, st, S, lds, s_ids, frames, ldf, frame_ids, vol, hl, cen, \
                       beta, T, times, partial, xtab, nub)
    if (Z > 2) DNMF_K16_LAUNCH(3);
    else if (Z == 2) DNMF_K16_LAUNCH(2);
    else DNMF_K16_LAUNCH(1);
#undef DNMF_K16_LAUNCH
    if (Z > 1)
        hipLaunchKernelGGL((warp_normal_eqs_finish_kernel<3>), dim3((unsigned)B), dim3(256), 0, st, partial, nblk, H, g, sse,
                           accumulate);
    else
        hipLaunchKernelGGL((warp_normal_eqs_finish_kernel<2>), dim3((unsigned)B), dim3(256), 0, st, partial, nblk, H, g, sse,
                           accumulate);
    return check_launch("dnmf_warp_normal_eqs");
}

int dnmf_lm_step(const double *H, const double *g, const double *sse, int B, int Z, const double *M, float *beta, int T,
                 const int *times, double *H_acc, double *g_acc, double *sse_acc, double *sse0, double *lam, float *beta_acc,
                 int *counts, double nu, double lam0, double lam_min, double lam_max, int accept_only, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(H && g && sse && M && beta && times && H_acc && g_acc && sse_acc && sse0 && lam && beta_acc && counts,
                 DNMF_E_NULL, "dnmf_lm_step: NULL buffer");
    DNMF_REQUIRE(B > 0 && Z > 0 && T > 0, DNMF_E_SHAPE, "dnmf_lm_step: B=%d Z=%d T=%d", B, Z, T);
    DNMF_REQUIRE(nu > 1.0 && lam0 > 0.0 && lam_min > 0.0 && lam_max >= lam_min, DNMF_E_SHAPE,
                 "dnmf_lm_step: nu=%g lam0=%g lam_min=%g lam_max=%g (want nu > 1, 0 < lam_min <= lam_max, lam0 > 0)", nu, lam0,
                 lam_min, lam_max);
    hipLaunchKernelGGL(lm_step_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, H, g, sse, Z > 1 ? 30 : 12, M, beta, T,
                       times, H_acc, g_acc, sse_acc, sse0, lam, beta_acc, counts, nu, lam0, lam_min, lam_max, accept_only);
    return check_launch("dnmf_lm_step");
}

int dnmf_lm_step_smooth(const double *H, const double *g, const double *sse, int B, int Z, const double *M, const double *Minv,
                        float *beta, int T, const int *times, double *H_acc, double *g_acc, double *sse_acc, double *sse0,
                        double *lam, float *beta_acc, int *counts, double nu, double lam0, double lam_min, double lam_max,
                        int accept_only, float *beta_ref, double m, double *prior, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(H && g && sse && M && Minv && beta && times && H_acc && g_acc && sse_acc && sse0 && lam && beta_acc && counts &&
                     beta_ref && prior,
                 DNMF_E_NULL, "dnmf_lm_step_smooth: NULL buffer");
    DNMF_REQUIRE(B > 0 && Z > 0 && T > 0, DNMF_E_SHAPE, "dnmf_lm_step_smooth: B=%d Z=%d T=%d", B, Z, T);
    DNMF_REQUIRE(nu > 1.0 && lam0 > 0.0 && lam_min > 0.0 && lam_max >= lam_min, DNMF_E_SHAPE,
                 "dnmf_lm_step_smooth: nu=%g lam0=%g lam_min=%g lam_max=%g (want nu > 1, 0 < lam_min <= lam_max, lam0 > 0)", nu,
                 lam0, lam_min, lam_max);
    DNMF_REQUIRE(m >= 0.0 && m - m == 0.0, DNMF_E_SHAPE, "dnmf_lm_step_smooth: m=%g (want a finite weight >= 0)", m);
    DNMF_REQUIRE(beta_ref != beta, DNMF_E_SHAPE, "dnmf_lm_step_smooth: beta_ref must not be beta (it holds accepted points only)");
    hipLaunchKernelGGL(lm_step_smooth_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, H, g, sse, Z > 1 ? 30 : 12, M,
                       Minv, beta, T, times, H_acc, g_acc, sse_acc, sse0, lam, beta_acc, counts, nu, lam0, lam_min, lam_max,
                       accept_only, beta_ref, m, prior);
    return check_launch("dnmf_lm_step_smooth");
}

int dnmf_lm_step_order(const double *H, const double *g, const double *sse, int B, int Z, int order, const double *M,
                       const double *Minv, float *beta, int T, const int *times, double *H_acc, double *g_acc, double *sse_acc,
                       double *sse0, double *lam, float *beta_acc, int *counts, double nu, double lam0, double lam_min,
                       double lam_max, int accept_only, float *beta_ref, double m, double *prior, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(H && g && sse && M && beta && times && H_acc && g_acc && sse_acc && sse0 && lam && beta_acc && counts, DNMF_E_NULL,
                 "dnmf_lm_step_order: NULL buffer");
    DNMF_REQUIRE(B > 0 && Z > 0 && T > 0, DNMF_E_SHAPE, "dnmf_lm_step_order: B=%d Z=%d T=%d", B, Z, T);
    DNMF_REQUIRE(order >= 0 && order <= 2, DNMF_E_SHAPE, "dnmf_lm_step_order: order=%d (0 translation, 1 affine, 2 quadratic)", order);
    DNMF_REQUIRE(nu > 1.0 && lam0 > 0.0 && lam_min > 0.0 && lam_max >= lam_min, DNMF_E_SHAPE,
                 "dnmf_lm_step_order: nu=%g lam0=%g lam_min=%g lam_max=%g (want nu > 1, 0 < lam_min <= lam_max, lam0 > 0)", nu,
                 lam0, lam_min, lam_max);
    DNMF_REQUIRE(m >= 0.0 && m - m == 0.0, DNMF_E_SHAPE, "dnmf_lm_step_order: m=%g (want a finite weight >= 0)", m);
    DNMF_REQUIRE(m == 0.0 || (Minv && beta_ref && prior), DNMF_E_NULL, "dnmf_lm_step_order: NULL Minv, beta_ref or prior with m != 0");
    DNMF_REQUIRE(m == 0.0 || beta_ref != beta, DNMF_E_SHAPE,
                 "dnmf_lm_step_order: beta_ref must not be beta (it holds accepted points only)");
    hipLaunchKernelGGL(lm_step_order_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, H, g, sse, Z > 1 ? 30 : 12, order,
                       M, Minv, beta, T, times, H_acc, g_acc, sse_acc, sse0, lam, beta_acc, counts, nu, lam0, lam_min, lam_max,
                       accept_only, beta_ref, m, prior);
    return check_launch("dnmf_lm_step_order");
}

int dnmf_lm_step_jac(const double *H, const double *g, const double *sse, int B, int X, int Y, int Z, int order, const double *M,
                     const double *Minv, float *beta, int T, const int *times, double *H_acc, double *g_acc, double *sse_acc,
                     double *sse0, double *lam, float *beta_acc, int *counts, double nu, double lam0, double lam_min,
                     double lam_max, int accept_only, float *beta_ref, double m, double *prior, double mj, double *jac,
                     double *min_det, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(H && g && sse && M && Minv && beta && times && H_acc && g_acc && sse_acc && sse0 && lam && beta_acc && counts &&
                     jac && min_det,
                 DNMF_E_NULL, "dnmf_lm_step_jac: NULL buffer");
    DNMF_REQUIRE(B > 0 && X > 1 && Y > 1 && Z > 0 && T > 0, DNMF_E_SHAPE,
                 "dnmf_lm_step_jac: B=%d X=%d Y=%d Z=%d T=%d (the x and y axes need two voxels at least)", B, X, Y, Z, T);
    DNMF_REQUIRE(order >= 0 && order <= 2, DNMF_E_SHAPE, "dnmf_lm_step_jac: order=%d (0 translation, 1 affine, 2 quadratic)", order);
    DNMF_REQUIRE(nu > 1.0 && lam0 > 0.0 && lam_min > 0.0 && lam_max >= lam_min, DNMF_E_SHAPE,
                 "dnmf_lm_step_jac: nu=%g lam0=%g lam_min=%g lam_max=%g (want nu > 1, 0 < lam_min <= lam_max, lam0 > 0)", nu, lam0,
                 lam_min, lam_max);
    DNMF_REQUIRE(m >= 0.0 && m - m == 0.0 && mj >= 0.0 && mj - mj == 0.0, DNMF_E_SHAPE,
                 "dnmf_lm_step_jac: m=%g mj=%g (want finite weights >= 0)", m, mj);
    DNMF_REQUIRE(m == 0.0 || (beta_ref && prior), DNMF_E_NULL, "dnmf_lm_step_jac: NULL beta_ref or prior with m != 0");
    DNMF_REQUIRE(m == 0.0 || beta_ref != beta, DNMF_E_SHAPE,
                 "dnmf_lm_step_jac: beta_ref must not be beta (it holds accepted points only)");
    JacHalf half;
    half.h[0] = 0.5 * (double)(X - 1), half.h[1] = 0.5 * (double)(Y - 1), half.h[2] = Z > 1 ? 0.5 * (double)(Z - 1) : 1.0;
    hipLaunchKernelGGL(lm_step_jac_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, H, g, sse, Z > 1 ? 30 : 12, order, M,
                       Minv, beta, T, times, H_acc, g_acc, sse_acc, sse0, lam, beta_acc, counts, nu, lam0, lam_min, lam_max,
                       accept_only, beta_ref, m, prior, mj, half, jac, min_det);
    return check_launch("dnmf_lm_step_jac");
}

}  // extern "C"
