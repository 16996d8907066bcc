// K17: the trilinear registered movie under the fitted warp.  For every lattice point u of the footprint volume and every
// frame t: the x with q_t(x) = u (Newton from x = u) and the frame sampled trilinearly there, zero padding -- the model's own
// forward (grid_sample, zeros, align_corners=True) read backwards.  tests/pullback_restatement.py is the definition in float64.
//
// Conventions are those of tracks.hip: q_t(x) = basis(x) . beta[:, :, t] in voxel indices, basis = [1, x, y, z, x^2, y^2, z^2,
// xy, xz, yz], the true Jacobian (row 8 = xz, row 9 = yz).  Unlike K7 (image_iwarp.hip) nothing here carries the reference's
// sz-for-(sz - 1) scaling: this is an extension, not a parity path.
//
// Arithmetic is fp32 on the DISPLACEMENT d = x - u, not on x.  q is quadratic, so with e0 = q(u) - u and J0 = J(u)
//     q(u + d) - u = e0 + J0 d + Q(d),   Q_k(d) = b4k dx^2 + b5k dy^2 + b6k dz^2 + b7k dx dy + b8k dx dz + b9k dy dz
// exactly, and J(u + d) = J0 + dQ/dd.  e0 is formed with the identity taken off inside an FMA (fma(b, u, -u) rounds (b - 1) u
// once), so every rounding is at the size of the displacement, not of the position: about ten roundings of half an ulp of |d|
// (|d| = 77 voxels, 0.15 of 512: 4e-5 in all) plus the one of x = u + d (3e-5 at 512) against the 1e-3 voxel of the contract.
// At the identity e0 = 0, at an integer translation e0 is that integer and J = I: d is exact and the weights are 1 and 0.
//
// A step below 1e-6, the definition's tolerance, is under the rounding floor of fp32; the kernel stops at a step below
// PB_TOL (relative to |d| beyond 32 voxels): Newton converges quadratically, so the error left after such a step is far below
// the step itself.
#include "common.hpp"

namespace dnmf {
namespace {

constexpr int PB_NEWTON_CAP = 32;   // Newton steps at most (K12's cap)
constexpr float PB_TOL = 1e-4f;     // a step below this in every coordinate ends the iteration
constexpr int PB_ROWS = 8;          // consecutive x a lane walks: the terms in (y, z) are paid once per PB_ROWS points
constexpr int PB_COLS = 256;        // positions of the (y, z) plane per block

struct PullbackArgs {
    const float *frames;
    long ldf, ldc_in;
    int nchan;
    const int *frame_ids;
    int X, Y, Z;
    const float *beta;
    int T;
    const int *times;
    float *out;
    long ldo, ldc_out;
    int fill_mode;
    float fill;
    float *coords;
    unsigned long long *bad;
    unsigned ident_mask;   // bit a*3 + k: coefficient (a, k) is the identity's (a row or a column of an axis of extent 1)
    int nxc;               // chunks of PB_ROWS rows along x
};

// one axis of the sample: clamped tap indices i0, i1 (always inside [0, S)), their weights (0 for a tap outside the volume)
__device__ __forceinline__ void axis_taps(float x, int S, int &i0, int &i1, float &w0, float &w1, bool &v0, bool &v1) {
    const bool near = x > -1.0f && x < (float)S;   // false for NaN; only then does (int)floor(x) mean anything
    const float f = floorf(x);
    const int i = near ? (int)f : -2;
    w1 = x - f, w0 = 1.0f - w1;
    v0 = near && i >= 0;
    v1 = near && i + 1 <= S - 1;
    i0 = max(i, 0), i1 = min(max(i + 1, 0), S - 1);
}

template <bool HASZ>
__global__ __launch_bounds__(PB_COLS) void warp_pullback_kernel(const PullbackArgs a) {
    constexpr int ND = HASZ ? 3 : 2;
    const int b = blockIdx.y;
    const int t_in = a.times ? a.times[b] : b;
    const bool t_ok = t_in >= 0 && t_in < a.T;   // a frame index outside beta: NaN coefficients, every point bad
    const int t = t_ok ? t_in : 0;
    const long row = a.frame_ids ? a.frame_ids[b] : b;
    // beta_t: 30 wave-uniform values (scalar loads); rows and columns of an axis of extent 1 are the identity's
    float bt[30];
#pragma unroll
    for (int i = 0; i < 30; ++i) {
        const float id = (i == 3 || i == 7 || i == 11) ? 1.0f : 0.0f;
        bt[i] = ((a.ident_mask >> i) & 1u) ? id : (t_ok ? a.beta[(long)i * a.T + t] : __builtin_nanf(""));
    }
#define BT(r, k) bt[(r) * 3 + (k)]
    const int tile = blockIdx.x / a.nxc, xc = blockIdx.x - tile * a.nxc;
    const int c = tile * PB_COLS + threadIdx.x;
    const int plane = a.Y * a.Z;
    const bool live = c < plane;
    const int iy = HASZ ? c / a.Z : c, iz = HASZ ? c - iy * a.Z : 0;
    const float y = (float)iy, z = (float)iz;

    // the terms of e0 = q(u) - u and of J0 = J(u) that do not depend on x:  e0_k = A_k + x (B_k + b4k x)
    float A[ND], Bx[ND], H[ND][ND], b4x2[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        float s = k == 1 ? fmaf(BT(2, k), y, -y) : BT(2, k) * y;
        if (HASZ) s = k == 2 ? s + fmaf(BT(3, k), z, -z) : fmaf(BT(3, k), z, s);
        s = fmaf(BT(5, k), y * y, s);
        if (HASZ) s = fmaf(BT(6, k), z * z, s), s = fmaf(BT(9, k), y * z, s);
        A[k] = s + BT(0, k);
        float r = fmaf(BT(7, k), y, k == 0 ? BT(1, k) - 1.0f : BT(1, k));
        if (HASZ) r = fmaf(BT(8, k), z, r);
        Bx[k] = r;
        b4x2[k] = BT(4, k) + BT(4, k);
        float h0 = fmaf(BT(7, k), y, BT(1, k)), h1 = fmaf(BT(5, k) + BT(5, k), y, BT(2, k));
        if (HASZ) h0 = fmaf(BT(8, k), z, h0), h1 = fmaf(BT(9, k), z, h1);
        H[k][0] = h0, H[k][1] = h1;
        if constexpr (HASZ) H[k][2] = fmaf(BT(6, k) + BT(6, k), z, fmaf(BT(9, k), y, BT(3, k)));
    }

    const float *fr = a.frames + row * a.ldf;
    float *orow = a.out + (long)b * a.ldo;
    const float nanv = __builtin_nanf("");
    unsigned nbad = 0;
    const int x_end = min(a.X, (xc + 1) * PB_ROWS);
    for (int ix = xc * PB_ROWS; ix < x_end; ++ix) {
        const float x = (float)ix;
        float e0[ND], J0[ND][ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            e0[k] = fmaf(x, fmaf(BT(4, k), x, Bx[k]), A[k]);
            J0[k][0] = fmaf(b4x2[k], x, H[k][0]);
            J0[k][1] = fmaf(BT(7, k), x, H[k][1]);
            if constexpr (HASZ) J0[k][2] = fmaf(BT(8, k), x, H[k][2]);
        }
        // Newton on d, from d = 0.  A fixed trip count with a per-lane flag; the wave leaves together once every lane has
        // finished (a wave-uniform branch).
        float d[3] = {0.0f, 0.0f, 0.0f};
        bool done = false, bad = false;
        for (int it = 0; it < PB_NEWTON_CAP; ++it) {
            if (!(done || bad || !live)) {
                float r[ND], J[ND][ND];
#pragma unroll
                for (int k = 0; k < ND; ++k) {
                    float s = fmaf(J0[k][0], d[0], e0[k]);
                    s = fmaf(J0[k][1], d[1], s);
                    s = fmaf(BT(4, k), d[0] * d[0], s);
                    s = fmaf(BT(5, k), d[1] * d[1], s);
                    s = fmaf(BT(7, k), d[0] * d[1], s);
                    J[k][0] = fmaf(BT(7, k), d[1], fmaf(b4x2[k], d[0], J0[k][0]));
                    J[k][1] = fmaf(BT(5, k) + BT(5, k), d[1], fmaf(BT(7, k), d[0], J0[k][1]));
                    if constexpr (HASZ) {
                        s = fmaf(J0[k][2], d[2], s);
                        s = fmaf(BT(6, k), d[2] * d[2], s);
                        s = fmaf(BT(8, k), d[0] * d[2], s);
                        s = fmaf(BT(9, k), d[1] * d[2], s);
                        J[k][0] = fmaf(BT(8, k), d[2], J[k][0]);
                        J[k][1] = fmaf(BT(9, k), d[2], J[k][1]);
                        J[k][2] = fmaf(BT(6, k) + BT(6, k), d[2], fmaf(BT(9, k), d[1], fmaf(BT(8, k), d[0], J0[k][2])));
                    }
                    r[k] = s;
                }
                float det, s[3] = {0.0f, 0.0f, 0.0f};
                if constexpr (HASZ) {   // the step J^-1 r by the adjugate, as K12
                    const float c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
                    const float c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
                    const float c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
                    det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
                    s[0] = c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2];
                    s[1] = c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2];
                    s[2] = c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2];
                } else {
                    det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
                    s[0] = J[1][1] * r[0] - J[0][1] * r[1];
                    s[1] = J[0][0] * r[1] - J[1][0] * r[0];
                }
                if (!(fabsf(det) >= 1e-12f)) {
                    bad = true;
                } else {
                    const float inv = 1.0f / det;
                    float big = 0.0f, far = 0.0f;
#pragma unroll
                    for (int k = 0; k < ND; ++k) {
                        s[k] *= inv;
                        d[k] -= s[k];
                        big = fmaxf(big, fabsf(s[k]));
                        far = fmaxf(far, fabsf(d[k]));
                    }
                    // NaN or inf in d: far is inf, or a NaN step leaves big < tol false for ever -- test d itself
                    bool finite = __builtin_isfinite(d[0]) && __builtin_isfinite(d[1]);
                    if (HASZ) finite = finite && __builtin_isfinite(d[2]);
                    if (!finite) bad = true;
                    else done = big < PB_TOL * fmaxf(1.0f, far * (1.0f / 32.0f));
                }
            }
            if (__all(done || bad || !live)) break;
        }
        if (!live) continue;
        bad = bad || !done;
        nbad += bad ? 1u : 0u;

        const float px = x + d[0], py = y + d[1], pz = HASZ ? z + d[2] : 0.0f;
        int x0, x1, y0, y1, z0 = 0, z1 = 0;
        float wx0, wx1, wy0, wy1, wz0 = 1.0f, wz1 = 0.0f;
        bool vx0, vx1, vy0, vy1, vz0 = true, vz1 = false;
        axis_taps(px, a.X, x0, x1, wx0, wx1, vx0, vx1);
        axis_taps(py, a.Y, y0, y1, wy0, wy1, vy0, vy1);
        if constexpr (HASZ) axis_taps(pz, a.Z, z0, z1, wz0, wz1, vz0, vz1);
        bool outside = !(px >= 0.0f && px <= (float)(a.X - 1) && py >= 0.0f && py <= (float)(a.Y - 1));
        if (HASZ) outside = outside || !(pz >= 0.0f && pz <= (float)(a.Z - 1));
        const bool filled = a.fill_mode ? (bad || outside) : false;
        // tap offsets inside a frame (every index is clamped into the volume) and weights
        int off[HASZ ? 8 : 4];
        float w[HASZ ? 8 : 4];
        bool v[HASZ ? 8 : 4];
        {
            const int ox[2] = {x0 * plane, x1 * plane}, oy[2] = {y0 * a.Z, y1 * a.Z}, oz[2] = {z0, z1};
            const float ax[2] = {wx0, wx1}, ay[2] = {wy0, wy1}, az[2] = {wz0, wz1};
            const bool bx[2] = {vx0, vx1}, by[2] = {vy0, vy1}, bz[2] = {vz0, vz1};
            int n = 0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int l = 0; l < (HASZ ? 2 : 1); ++l, ++n) {
                        off[n] = ox[i] + oy[j] + oz[l];
                        w[n] = HASZ ? ax[i] * ay[j] * az[l] : ax[i] * ay[j];
                        v[n] = bx[i] && by[j] && bz[l];
                    }
        }
        const int p = ix * plane + c;
        for (int ch = 0; ch < a.nchan; ++ch) {
            const float *src = fr + (long)ch * a.ldc_in;
            float acc = 0.0f;
#pragma unroll
            for (int n = 0; n < (HASZ ? 8 : 4); ++n) {
                const float val = src[off[n]];          // inside the volume whatever v[n] says
                acc = fmaf(w[n], v[n] ? val : 0.0f, acc);   // a tap outside the volume contributes 0, not 0 * val
            }
            orow[(long)ch * a.ldc_out + p] = filled ? a.fill : (bad ? 0.0f : acc);
        }
        if (a.coords) {
            float *cp = a.coords + ((long)b * a.X * plane + p) * 3;
            cp[0] = bad ? nanv : px, cp[1] = bad ? nanv : py, cp[2] = bad ? nanv : pz;
        }
    }
#undef BT
    if (a.bad) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o);
        if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(a.bad, (unsigned long long)nbad);
    }
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_warp_pullback(const float *frames, long ldf, long ldc_in, int nchan, const int *frame_ids, int X, int Y, int Z,
                       const float *beta, int T, const int *times, int B, float *out, long ldo, long ldc_out, int fill_mode,
                       float fill_value, float *coords, long long *bad_count, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames && beta && out, DNMF_E_NULL, "dnmf_warp_pullback: NULL argument");
    DNMF_REQUIRE(X > 0 && Y > 0 && Z > 0 && T > 0 && B >= 0, DNMF_E_SHAPE, "dnmf_warp_pullback: volume %dx%dx%d T=%d B=%d", X, Y, Z, T, B);
    DNMF_REQUIRE(times || B <= T, DNMF_E_SHAPE, "dnmf_warp_pullback: B=%d frames without times, T=%d", B, T);
    DNMF_REQUIRE(nchan >= 1, DNMF_E_SHAPE, "dnmf_warp_pullback: nchan=%d", nchan);
    DNMF_REQUIRE(fill_mode == 0 || fill_mode == 1, DNMF_E_SHAPE, "dnmf_warp_pullback: fill_mode=%d (0 zero padding, 1 fill_value)",
                 fill_mode);
    const long P = (long)X * Y * Z;
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_warp_pullback: %ld voxels (32-bit tap offsets)", P);
    if (nchan == 1) ldc_in = ldc_out = P;   // unused with one channel
    DNMF_REQUIRE(ldc_in >= P && ldc_out >= P && ldf >= (nchan - 1) * ldc_in + P && ldo >= (nchan - 1) * ldc_out + P, DNMF_E_SHAPE,
                 "dnmf_warp_pullback: strides ldf=%ld ldc_in=%ld ldo=%ld ldc_out=%ld too short for %d channels of P=%ld", ldf, ldc_in,
                 ldo, ldc_out, nchan, P);
    DNMF_REQUIRE(B <= 65535, DNMF_E_UNSUPPORTED, "dnmf_warp_pullback: B=%d frames in one call (they ride on gridDim.y: at most 65535)", B);
    const long plane = (long)Y * Z;
    const long tiles = (plane + PB_COLS - 1) / PB_COLS;
    const int nxc = (X + PB_ROWS - 1) / PB_ROWS;
    DNMF_REQUIRE(tiles * nxc < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_warp_pullback: %ld blocks per frame", tiles * nxc);
    if (B == 0) return DNMF_OK;
    // rows of the basis that use axis d: x 1 4 7 8, y 2 5 7 9, z 3 6 8 9 (tracks.hip); an axis of extent 1 is inactive: those rows
    // and its output column are the identity's, which leaves its coordinate at 0 and the solve to the other axes
    static const int uses[3][4] = {{1, 4, 7, 8}, {2, 5, 7, 9}, {3, 6, 8, 9}};
    const int S[3] = {X, Y, Z};
    unsigned mask = 0;
    for (int d = 0; d < 3; ++d) {
        if (S[d] > 1) continue;
        for (int r = 0; r < 10; ++r) mask |= 1u << (r * 3 + d);
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 3; ++k) mask |= 1u << (uses[d][j] * 3 + k);
    }
    PullbackArgs a;
    a.frames = frames, a.ldf = ldf, a.ldc_in = ldc_in, a.nchan = nchan, a.frame_ids = frame_ids;
    a.X = X, a.Y = Y, a.Z = Z, a.beta = beta, a.T = T, a.times = times;
    a.out = out, a.ldo = ldo, a.ldc_out = ldc_out, a.fill_mode = fill_mode, a.fill = fill_value;
    a.coords = coords, a.bad = reinterpret_cast<unsigned long long *>(bad_count), a.ident_mask = mask, a.nxc = nxc;
    const dim3 grid((unsigned)(tiles * nxc), (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
    if (Z > 1)
        hipLaunchKernelGGL(warp_pullback_kernel<true>, grid, dim3(PB_COLS), 0, st, a);
    else
        hipLaunchKernelGGL(warp_pullback_kernel<false>, grid, dim3(PB_COLS), 0, st, a);
    return check_launch("dnmf_warp_pullback");
}

}  // extern "C"
