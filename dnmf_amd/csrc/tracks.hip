// K11 / K12 / K13: the bridge between per-frame neuron positions ("tracks", (K,3,T)) and the quadratic warp beta, and the
// box-mean trace read-out on tracked positions (reference WUtils/Simulator.py:230-240 get_roi_signals, Utils.py:14-52).
//
// Conventions (Demix/dNMF.py:53-58): q_t(x) = basis(x) . beta[:, :, t], basis = [1, x, y, z, x^2, y^2, z^2, xy, xz, yz],
// maps a voxel x of frame t to the point of the footprint volume sampled there.  A neuron whose footprint is centred at r
// is seen in frame t at the x* with q_t(x*) = r.  Coordinates are voxel indices.  The Jacobian is the true one of that
// basis (row 8 = xz, row 9 = yz), not the swapped convention ExponentialFP.log_det_jac keeps from the reference.
//
// None of the three is bound by bandwidth: K T small independent problems on data that is already on the device.  All
// arithmetic is float64 (fp32 only where a value is stored: beta, the frames).
#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int TR_MAX_BOX = 4096;   // voxels of the largest K13 box
constexpr int TR_NEWTON_CAP = 32;  // K12: Newton steps at most

struct Geometry {
    double a[3];   // u = a p + c per axis: 2 / (S - 1), -1; an axis of extent 1 has a = c = 0 (u = 0)
    double c[3];
    double h[3];   // (S - 1) / 2: the identity map in normalised inputs is p = h u + h
    int active[3];
};

inline Geometry make_geometry(int X, int Y, int Z) {
    Geometry g;
    const int S[3] = {X, Y, Z};
    for (int d = 0; d < 3; ++d) {
        g.active[d] = S[d] > 1;
        g.a[d] = S[d] > 1 ? 2.0 / (double)(S[d] - 1) : 0.0;
        g.c[d] = S[d] > 1 ? -1.0 : 0.0;
        g.h[d] = 0.5 * (double)(S[d] - 1);
    }
    return g;
}

__device__ __forceinline__ void basis10(double x, double y, double z, double *f) {
    f[0] = 1.0, f[1] = x, f[2] = y, f[3] = z;
    f[4] = x * x, f[5] = y * y, f[6] = z * z;
    f[7] = x * y, f[8] = x * z, f[9] = y * z;
}

// ---- K11 ---------------------------------------------------------------------------------------------------------
// One wave per frame.  Lanes stride over the neurons and keep the 55 sums of the upper triangle of Phi^T Phi and the 30
// of Phi^T (R - p) in registers (float64); a butterfly leaves every total in every lane.  The 10 x 10 system -- rows
// that are not free replaced by unit rows -- is then solved in registers: lane j < 10 holds column j, lanes 10..12 the
// three right-hand sides, every row operation is one instruction for all 13 columns and the pivot column travels by
// shuffles with compile-time lane numbers.  Partial pivoting; a pivot at or below 1e-12 of the largest diagonal entry
// marks the frame singular.
//
// free_mask: bit i set = row i of B' is free.  beta (10,3,T) fp32, ok (T).
template <typename TP>
__global__ __launch_bounds__(64) void fit_warp_kernel(const TP *__restrict__ tracks, int K, int T, const double *__restrict__ targets,
                                                       Geometry g, unsigned free_mask, int nfree, double ridge,
                                                       float *__restrict__ beta, unsigned char *__restrict__ ok) {
    const int t = blockIdx.x;
    const int lane = threadIdx.x;
    double N[55], r[30];
#pragma unroll
    for (int i = 0; i < 55; ++i) N[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 30; ++i) r[i] = 0.0;
    double count = 0.0;
    for (int k = lane; k < K; k += 64) {
        const double px = (double)tracks[((long)k * 3 + 0) * T + t];
        const double py = (double)tracks[((long)k * 3 + 1) * T + t];
        const double pz = (double)tracks[((long)k * 3 + 2) * T + t];
        if (!(__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz))) continue;   // not tracked here
        const double u[3] = {g.a[0] * px + g.c[0], g.a[1] * py + g.c[1], g.a[2] * pz + g.c[2]};
        double f[10];
        basis10(u[0], u[1], u[2], f);
        // residual of the identity map: R - (h u + h) (= R - p up to rounding)
        double e[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) e[d] = targets[3 * k + d] - (g.h[d] * u[d] + g.h[d]);
        int n = 0;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
#pragma unroll
            for (int j = i; j < 10; ++j) N[n++] += f[i] * f[j];
#pragma unroll
            for (int d = 0; d < 3; ++d) r[3 * i + d] += f[i] * e[d];
        }
        count += 1.0;
    }
#pragma unroll
    for (int i = 0; i < 55; ++i) N[i] = wave_sum_all(N[i]);
#pragma unroll
    for (int i = 0; i < 30; ++i) r[i] = wave_sum_all(r[i]);
    count = wave_sum_all(count);

    // this lane's column of the augmented system [Phi^T Phi + ridge I | Phi^T e]; axes of extent 1 get no right-hand side
    double col[10];
    double scale = 0.0;
    {
        int n = 0;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const bool fi = (free_mask >> i) & 1u;
#pragma unroll
            for (int j = i; j < 10; ++j, ++n) {
                const bool fj = (free_mask >> j) & 1u;
                double v = (fi && fj) ? N[n] : 0.0;
                if (i == j) {
                    v = fi ? v + ridge : 1.0;
                    if (fi) scale = fmax(scale, v);
                }
                if (lane == j) col[i] = v;
                if (lane == i && i != j) col[j] = v;
            }
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (lane == 10 + d) col[i] = (fi && g.active[d]) ? r[3 * i + d] : 0.0;
        }
        if (lane > 12) {
#pragma unroll
            for (int i = 0; i < 10; ++i) col[i] = 0.0;
        }
    }
    bool good = !(ridge == 0.0 && count < (double)nfree) && scale > 0.0 && scale < __builtin_inf();
    const double tiny = 1e-12 * scale;
#pragma unroll
    for (int p = 0; p < 10; ++p) {
        // column p below the diagonal, from lane p; the largest entry is the pivot (the first of equal ones)
        double v[10];
        int piv = p;
#pragma unroll
        for (int i = p; i < 10; ++i) v[i] = __shfl(col[i], p);
        double best = fabs(v[p]);
#pragma unroll
        for (int i = p + 1; i < 10; ++i) {
            if (fabs(v[i]) > best) best = fabs(v[i]), piv = i;
        }
        // swap rows p and piv (piv is the same in every lane)
        double vp = v[p];
#pragma unroll
        for (int i = p + 1; i < 10; ++i) {
            if (i == piv) {
                const double s = col[p];
                col[p] = col[i], col[i] = s;
                vp = v[i], v[i] = v[p];
            }
        }
        if (((free_mask >> p) & 1u) && !(fabs(vp) > tiny)) good = false;
        const double inv = 1.0 / vp;
#pragma unroll
        for (int i = p + 1; i < 10; ++i) col[i] -= (v[i] * inv) * col[p];
    }
    // back substitution in the lanes of the right-hand sides
#pragma unroll
    for (int i = 9; i >= 0; --i) {
        double s = col[i];
#pragma unroll
        for (int j = i + 1; j < 10; ++j) s -= __shfl(col[i], j) * col[j];
        const double x = s / __shfl(col[i], i);
        if (lane >= 10) col[i] = x;
    }
    // lanes 10..12: B' = B'_id + D, back to voxel inputs, one rounding to fp32
    bool finite = true;
    double b[10];
    const int d = lane >= 10 && lane <= 12 ? lane - 10 : 0;
    {
        double B[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) B[i] = col[i];
        B[0] += g.h[d];
        B[1 + d] += g.h[d];
        const double *a = g.a, *c = g.c;
        b[0] = B[0] + c[0] * B[1] + c[1] * B[2] + c[2] * B[3] + c[0] * c[0] * B[4] + c[1] * c[1] * B[5] + c[2] * c[2] * B[6] +
               c[0] * c[1] * B[7] + c[0] * c[2] * B[8] + c[1] * c[2] * B[9];
        b[1] = a[0] * (B[1] + 2.0 * c[0] * B[4] + c[1] * B[7] + c[2] * B[8]);
        b[2] = a[1] * (B[2] + 2.0 * c[1] * B[5] + c[0] * B[7] + c[2] * B[9]);
        b[3] = a[2] * (B[3] + 2.0 * c[2] * B[6] + c[0] * B[8] + c[1] * B[9]);
        b[4] = a[0] * a[0] * B[4], b[5] = a[1] * a[1] * B[5], b[6] = a[2] * a[2] * B[6];
        b[7] = a[0] * a[1] * B[7], b[8] = a[0] * a[2] * B[8], b[9] = a[1] * a[2] * B[9];
#pragma unroll
        for (int i = 0; i < 10; ++i) finite = finite && __builtin_isfinite(b[i]) && fabs(b[i]) < 3.0e38;
    }
    const bool mine = lane >= 10 && lane <= 12;
    // every column must be finite (the vote is over the whole wave: other lanes hold zeros)
    good = good && __all(mine ? finite : true);
    if (mine) {
        const bool ident = !good || !g.active[d];
#pragma unroll
        for (int i = 0; i < 10; ++i) beta[((long)i * 3 + d) * T + t] = ident ? (i == 1 + d ? 1.0f : 0.0f) : (float)b[i];
    }
    if (lane == 0) ok[t] = good ? 1 : 0;
}

// ---- K12 ---------------------------------------------------------------------------------------------------------
// One thread per (neuron, frame), frames fastest.  Newton on q_t(x) = target in float64 with the analytic Jacobian, a
// fixed trip count.  out (K,3,B).
__global__ __launch_bounds__(256) void invert_warp_kernel(const float *__restrict__ beta, int T, const int *__restrict__ times, int B,
                                                           const double *__restrict__ targets, int K, const double *__restrict__ start,
                                                           double tol, double *__restrict__ out) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)K * B) return;
    const int k = (int)(id / B), j = (int)(id - (long)k * B);
    const int t = times ? times[j] : j;
    double b[30];
#pragma unroll
    for (int i = 0; i < 30; ++i) b[i] = (double)beta[(long)i * T + t];
    const double r[3] = {targets[3 * k], targets[3 * k + 1], targets[3 * k + 2]};
    double x[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = start ? start[((long)k * 3 + d) * B + j] : r[d];
    bool done = false, bad = false;
    for (int it = 0; it < TR_NEWTON_CAP; ++it) {
        if (done || bad) continue;
        double f[10];
        basis10(x[0], x[1], x[2], f);
        double e[3], J[3][3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < 10; ++i) q += f[i] * b[3 * i + d];
            e[d] = q - r[d];
            J[d][0] = b[3 + d] + 2.0 * b[12 + d] * x[0] + b[21 + d] * x[1] + b[24 + d] * x[2];
            J[d][1] = b[6 + d] + 2.0 * b[15 + d] * x[1] + b[21 + d] * x[0] + b[27 + d] * x[2];
            J[d][2] = b[9 + d] + 2.0 * b[18 + d] * x[2] + b[24 + d] * x[0] + b[27 + d] * x[1];
        }
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        if (!(fabs(det) >= 1e-12)) {
            bad = true;
            continue;
        }
        const double inv = 1.0 / det;
        // step = J^-1 e by the adjugate
        const double s0 = (c00 * e[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * e[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * e[2]) * inv;
        const double s1 = (c01 * e[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * e[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * e[2]) * inv;
        const double s2 = (c02 * e[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * e[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * e[2]) * inv;
        x[0] -= s0, x[1] -= s1, x[2] -= s2;
        if (!(__builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]))) {
            bad = true;
            continue;
        }
        done = fabs(s0) < tol && fabs(s1) < tol && fabs(s2) < tol;
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int d = 0; d < 3; ++d) out[((long)k * 3 + d) * B + j] = (done && !bad) ? x[d] : nan;
}

// ---- K13 ---------------------------------------------------------------------------------------------------------
// One wave per (neuron, frame), four per block.  The box of (2w + 1) voxels per axis around the position rounded half to
// even; voxels of the box outside the volume are zeros that count in the mean (np.pad 'constant', Utils.py:44-50), NaN
// voxels are left out (nanmean).  float64 sum, a fixed butterfly: the result does not depend on the launch.
template <typename TP>
__global__ __launch_bounds__(256) void roi_signals_kernel(const float *__restrict__ frames, long ldf, int X, int Y, int Z,
                                                           const TP *__restrict__ tracks, int K, int T, int wx, int wy, int wz,
                                                           double *__restrict__ out) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)K * T) return;     // whole waves leave together
    const int lane = threadIdx.x & 63;
    const int k = (int)(item / T), t = (int)(item - (long)k * T);
    const double p[3] = {(double)tracks[((long)k * 3 + 0) * T + t], (double)tracks[((long)k * 3 + 1) * T + t],
                         (double)tracks[((long)k * 3 + 2) * T + t]};
    const int S[3] = {X, Y, Z};
    int c[3];
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double q = rint(p[d]);                       // half to even, like torch.round
        inside = inside && q >= 0.0 && q <= (double)(S[d] - 1);   // false for NaN
        c[d] = inside ? (int)q : 0;
    }
    if (!inside) {
        if (lane == 0) out[item] = __builtin_nan("");
        return;
    }
    const int ny = 2 * wy + 1, nz = 2 * wz + 1;
    const int nbox = (2 * wx + 1) * ny * nz;
    const float *fr = frames + (long)t * ldf;
    double sum = 0.0;
    int n = 0;
    for (int i = lane; i < nbox; i += 64) {
        const int ix = i / (ny * nz), rem = i - ix * ny * nz;
        const int iy = rem / nz, iz = rem - iy * nz;
        const int x = c[0] - wx + ix, y = c[1] - wy + iy, z = c[2] - wz + iz;
        if (in_range(x, X) && in_range(y, Y) && in_range(z, Z)) {
            const float v = fr[((long)x * Y + y) * Z + z];
            if (v == v) sum += (double)v, ++n;
        } else {
            ++n;                                           // a padded zero
        }
    }
    sum = wave_sum_all(sum), n = wave_sum_all(n);
    if (lane == 0) out[item] = n > 0 ? sum / (double)n : __builtin_nan("");
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_fit_quadratic_warp(const void *tracks, int tracks_f64, int K, int T, const double *targets, int X, int Y, int Z, int order,
                            double ridge, float *beta, unsigned char *ok, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(tracks && targets && beta && ok, DNMF_E_NULL, "dnmf_fit_quadratic_warp: NULL argument");
    DNMF_REQUIRE(K > 0 && T > 0 && X > 0 && Y > 0 && Z > 0, DNMF_E_SHAPE, "dnmf_fit_quadratic_warp: K=%d T=%d volume %dx%dx%d", K, T,
                 X, Y, Z);
    DNMF_REQUIRE(ridge >= 0.0 && ridge < __builtin_inf(), DNMF_E_SHAPE, "dnmf_fit_quadratic_warp: ridge=%g must be >= 0 and finite",
                 ridge);
    DNMF_REQUIRE(order >= 0 && order <= 2, DNMF_E_UNSUPPORTED,
                 "dnmf_fit_quadratic_warp: order=%d (0 translation, 1 affine, 2 quadratic)", order);
    const Geometry g = make_geometry(X, Y, Z);
    // rows of the basis that use axis d: x 1 4 7 8, y 2 5 7 9, z 3 6 8 9
    static const unsigned uses[3] = {(1u << 1) | (1u << 4) | (1u << 7) | (1u << 8), (1u << 2) | (1u << 5) | (1u << 7) | (1u << 9),
                                     (1u << 3) | (1u << 6) | (1u << 8) | (1u << 9)};
    unsigned mask = order == 0 ? 0x1u : (order == 1 ? 0xfu : 0x3ffu);
    for (int d = 0; d < 3; ++d)
        if (!g.active[d]) mask &= ~uses[d];
    const int nfree = __builtin_popcount(mask);
    const hipStream_t st = (hipStream_t)stream;
    if (tracks_f64)
        hipLaunchKernelGGL(fit_warp_kernel<double>, dim3((unsigned)T), dim3(64), 0, st, static_cast<const double *>(tracks), K, T, targets,
                           g, mask, nfree, ridge, beta, ok);
    else
        hipLaunchKernelGGL(fit_warp_kernel<float>, dim3((unsigned)T), dim3(64), 0, st, static_cast<const float *>(tracks), K, T, targets,
                           g, mask, nfree, ridge, beta, ok);
    return check_launch("dnmf_fit_quadratic_warp");
}

int dnmf_invert_quadratic_warp(const float *beta, int T, const int *times, int B, const double *targets, int K, const double *start,
                               double tol, double *out, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(beta && targets && out, DNMF_E_NULL, "dnmf_invert_quadratic_warp: NULL argument");
    DNMF_REQUIRE(K > 0 && T > 0 && B >= 0 && (times || B <= T), DNMF_E_SHAPE, "dnmf_invert_quadratic_warp: K=%d T=%d B=%d", K, T, B);
    DNMF_REQUIRE(tol > 0.0 && tol < __builtin_inf(), DNMF_E_SHAPE, "dnmf_invert_quadratic_warp: tol=%g must be positive", tol);
    if (B == 0) return DNMF_OK;
    const long n = (long)K * B;
    DNMF_REQUIRE((n + 255) / 256 < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_invert_quadratic_warp: K x B = %ld problems", n);
    hipLaunchKernelGGL(invert_warp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, beta, T, times, B,
                       targets, K, start, tol, out);
    return check_launch("dnmf_invert_quadratic_warp");
}

int dnmf_roi_signals(const float *frames, long ldf, int X, int Y, int Z, const void *tracks, int tracks_f64, int K, int T,
                     const int *window, double *out, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames && tracks && window && out, DNMF_E_NULL, "dnmf_roi_signals: NULL argument");
    DNMF_REQUIRE(K > 0 && T > 0 && X > 0 && Y > 0 && Z > 0 && ldf >= (long)X * Y * Z, DNMF_E_SHAPE,
                 "dnmf_roi_signals: K=%d T=%d volume %dx%dx%d ldf=%ld", K, T, X, Y, Z, ldf);
    DNMF_REQUIRE(window[0] >= 0 && window[1] >= 0 && window[2] >= 0, DNMF_E_SHAPE, "dnmf_roi_signals: window (%d, %d, %d) < 0",
                 window[0], window[1], window[2]);
    long box = 1;
    for (int d = 0; d < 3; ++d) {
        // each factor is checked before it is multiplied in: the product cannot overflow
        DNMF_REQUIRE(window[d] <= TR_MAX_BOX / 2 && box * (2L * window[d] + 1) <= TR_MAX_BOX, DNMF_E_UNSUPPORTED,
                     "dnmf_roi_signals: the box of window (%d, %d, %d) has more than %d voxels", window[0], window[1], window[2],
                     TR_MAX_BOX);
        box *= 2L * window[d] + 1;
    }
    const long n = (long)K * T;
    DNMF_REQUIRE((n + 3) / 4 < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_roi_signals: K x T = %ld traces values", n);
    const dim3 grid((unsigned)((n + 3) / 4));
    const hipStream_t st = (hipStream_t)stream;
    if (tracks_f64)
        hipLaunchKernelGGL(roi_signals_kernel<double>, grid, dim3(256), 0, st, frames, ldf, X, Y, Z, static_cast<const double *>(tracks),
                           K, T, window[0], window[1], window[2], out);
    else
        hipLaunchKernelGGL(roi_signals_kernel<float>, grid, dim3(256), 0, st, frames, ldf, X, Y, Z, static_cast<const float *>(tracks), K,
                           T, window[0], window[1], window[2], out);
    return check_launch("dnmf_roi_signals");
}

}  // extern "C"
