// K9: the piecewise-rigid corrected movie.  Reference: Demix/MotionCorrect.py, tile_and_correct_3d
// :1639-1654 with shifts_opencv=True -- the per-patch shifts resized to a full-size field (skimage resize, order 1,
// mode 'reflect' = scipy's 'mirror'), added to the voxel grid, and the frame warped with skimage's warp (order 3,
// mode 'constant', cval 0 = scipy map_coordinates with the cubic B-spline prefilter), clipped to the frame's range.
//
// Three steps per chunk of frames, all fp32:
//   1. pw_fir_x_kernel: frame + add_to_movie, filtered along x with the truncated cubic B-spline prefilter (below), into
//      the coefficient buffer; the frame's min / max (of frame + add) on the side, for the clip.
//   2. pw_fir_kernel: the same filter along y, then along z (an axis of one voxel is left alone).
//   3. pw_eval_kernel: per output voxel, the shift field interpolated from the (NP,3) patch shifts, the sample position,
//      the 4 x 4 x 4 tap spline (4 x 4 for Z == 1) on the coefficients, the cut rule and the clip.
// The shift field is never written out: NP x 3 floats per frame are interpolated per voxel.
//
// The prefilter.  scipy's spline_filter (order 3) gives the coefficients of the mirror-extended data: the infinite
// filter h[k] = sqrt(3) z1^|k|, z1 = sqrt(3) - 2, applied to the signal mirrored about its end samples.  |z1|^13 < 4e-8,
// so h is cut at |k| <= 12 (a relative error of 1e-7) and the indices fold back into the axis (period 2n - 2), which
// serves short axes (n = 2 .. 12) the same way as long ones.
#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int PW_R = 12;    // FIR radius
constexpr int PW_SX = 8;    // x outputs per thread of the x pass (a window of PW_SX + 2 PW_R loads)

__constant__ float kPwH[PW_R + 1] = {1.732050808e+00f, -4.641016151e-01f, 1.243556530e-01f, -3.332099679e-02f,
                                     8.928334181e-03f, -2.392339934e-03f, 6.410255532e-04f, -1.717622793e-04f,
                                     4.602356403e-05f, -1.233197682e-05f, 3.304343229e-06f, -8.853960997e-07f,
                                     2.372411699e-07f};

// index j of the mirror-extended axis of n samples (..., 2, 1, 0, 1, 2, ..., n-1, n-2, ...) -> [0, n-1]
__device__ __forceinline__ int pw_fold(int j, int n) {
    if ((unsigned)j < (unsigned)n) return j;      // inside: no division
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = j % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// float <-> unsigned with the order of the floats (atomicMin / atomicMax on the frame's range)
__device__ __forceinline__ unsigned pw_ord(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pw_unord(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// lo = the largest, hi = the smallest value of the order-preserving encoding
__global__ void pw_range_init_kernel(unsigned *lohi, int nf) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nf) lohi[2 * f] = 0xffffffffu, lohi[2 * f + 1] = 0u;
}

// Step 1.  grid (ceil(YZ / 256), ceil(X / PW_SX), nf): thread = one (y,z) column, PW_SX consecutive x.
__global__ __launch_bounds__(256) void pw_fir_x_kernel(const float *frames, long ldf, const int *frame_ids, int f0, float add,
                                                       int X, long YZ, float *coef, long P, unsigned *lohi) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.z;
    const int x0 = blockIdx.y * PW_SX;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (c < YZ) {
        const long row = frame_ids ? frame_ids[f0 + f] : (long)(f0 + f);
        const float *src = frames + row * ldf + c;
        float win[PW_SX + 2 * PW_R];
        if (x0 >= PW_R && x0 + PW_SX + PW_R <= X) {   // away from the ends: no folding
#pragma unroll
            for (int j = 0; j < PW_SX + 2 * PW_R; ++j) win[j] = __fadd_rn(src[(long)(x0 - PW_R + j) * YZ], add);
        } else {
#pragma unroll
            for (int j = 0; j < PW_SX + 2 * PW_R; ++j) win[j] = __fadd_rn(src[(long)pw_fold(x0 - PW_R + j, X) * YZ], add);
        }
        float *dst = coef + (long)f * P + c;
#pragma unroll
        for (int i = 0; i < PW_SX; ++i) {
            if (x0 + i >= X) break;
            const float v = win[i + PW_R];
            float acc = kPwH[0] * v;
#pragma unroll
            for (int k = 1; k <= PW_R; ++k) acc = fmaf(kPwH[k], __fadd_rn(win[i + PW_R - k], win[i + PW_R + k]), acc);
            dst[(long)(x0 + i) * YZ] = X == 1 ? v : acc;
            lo = fminf(lo, v), hi = fmaxf(hi, v);
        }
    }
    // one atomic pair per wave
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(lohi + 2 * f, pw_ord(lo));
        atomicMax(lohi + 2 * f + 1, pw_ord(hi));
    }
}

// Step 2, one axis of n samples between `inner` (stride) and the rest.  grid (ceil(P / 256), nf): thread = one voxel; the
// 25 taps of neighbouring threads overlap, and are served by the cache.
__global__ __launch_bounds__(256) void pw_fir_kernel(const float *in, float *out, unsigned P, int n, unsigned inner) {
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P) return;
    const long off = (long)blockIdx.y * P;
    const int i = (int)((g / inner) % (unsigned)n);
    const float *src = in + off + (g - (unsigned)i * inner);
    float acc = kPwH[0] * src[(unsigned)i * inner];
    if (i >= PW_R && i + PW_R < n) {   // away from the ends: no folding
#pragma unroll
        for (int k = 1; k <= PW_R; ++k) acc = fmaf(kPwH[k], __fadd_rn(src[(unsigned)(i - k) * inner], src[(unsigned)(i + k) * inner]), acc);
    } else {
#pragma unroll
        for (int k = 1; k <= PW_R; ++k)
            acc = fmaf(kPwH[k], __fadd_rn(src[(unsigned)pw_fold(i - k, n) * inner], src[(unsigned)pw_fold(i + k, n) * inner]), acc);
    }
    out[off + g] = acc;
}

// Linear interpolation (order 1, mode 'mirror') of a grid of m values to n outputs at output index o: skimage's resize
// samples c = (m / n) (o + 0.5) - 0.5.  Corner i0 (and i0 + 1 when m > 1) with weight 1 - w, w.
struct PwLin {
    int i0, i1;
    double w;
};
__device__ __forceinline__ PwLin pw_lin(int o, int m, int n) {
    PwLin r;
    if (m == 1) {
        r.i0 = r.i1 = 0, r.w = 0.0;
        return r;
    }
    double c = (double)m / (double)n * ((double)o + 0.5) - 0.5;
    if (c < 0.0) c = -c;
    if (c > (double)(m - 1)) c = 2.0 * (double)(m - 1) - c;
    int i = (int)floor(c);
    i = i < 0 ? 0 : (i > m - 2 ? m - 2 : i);
    r.i0 = i, r.i1 = i + 1, r.w = c - (double)i;
    return r;
}

// Cubic B-spline taps of one axis of n samples at coordinate c (0 <= c <= n-1): folded indices and weights.
__device__ __forceinline__ void pw_taps(float c, int n, int idx[4], float w[4]) {
    if (n == 1) {
        idx[0] = idx[1] = idx[2] = idx[3] = 0;
        w[0] = w[2] = w[3] = 0.0f, w[1] = 1.0f;
        return;
    }
    const float fl = floorf(c);
    const float t = c - fl, s = 1.0f - t;
    const int i = (int)fl;
    const float t2 = t * t, t3 = t2 * t;
    w[0] = s * s * s * (1.0f / 6.0f);
    w[1] = 0.5f * t3 - t2 + 2.0f / 3.0f;
    w[2] = 0.5f * (t + t2 - t3) + 1.0f / 6.0f;
    w[3] = t3 * (1.0f / 6.0f);
#pragma unroll
    for (int a = 0; a < 4; ++a) idx[a] = pw_fold(i - 1 + a, n);
}

// Step 3.  grid (ceil(P / 256), frame groups): thread = one voxel, frames blockIdx.y, + gridDim.y, ...  The per-voxel sums
// of the finite values go to tsum / tcount directly with one frame group, else to part / partc (one row of P per group;
// pw_sum_kernel adds them up in group order): no atomics, the same sums on every run.
template <bool HASZ>
__global__ __launch_bounds__(256) void pw_eval_kernel(const float *coef, int nf, int X, int Y, int Z, int d0, int d1, int d2,
                                                      const float *shifts, int NP, const unsigned *lohi, float add, float *out,
                                                      long ldo, float *tsum, int *tcount, float *part, int *partc) {
    const unsigned P = (unsigned)X * Y * Z;
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P) return;
    const unsigned yz = g / (unsigned)Z;
    const int z = (int)(g - yz * (unsigned)Z), x = (int)(yz / (unsigned)Y), y = (int)(yz - (unsigned)x * Y);
    const PwLin lx = pw_lin(x, d0, X), ly = pw_lin(y, d1, Y), lz = pw_lin(z, d2, Z);
    int q[8];
    double wq[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int ix = (a & 4) ? lx.i1 : lx.i0, iy = (a & 2) ? ly.i1 : ly.i0, iz = (a & 1) ? lz.i1 : lz.i0;
        q[a] = 3 * ((ix * d1 + iy) * d2 + iz);
        wq[a] = ((a & 4) ? lx.w : 1.0 - lx.w) * ((a & 2) ? ly.w : 1.0 - ly.w) * ((a & 1) ? lz.w : 1.0 - lz.w);
    }
    float acc = 0.0f;
    int cnt = 0;
    for (int f = blockIdx.y; f < nf; f += gridDim.y) {
        const float *s = shifts + (long)f * NP * 3;
        double fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll
        for (int a = 0; a < 8; ++a) fx += wq[a] * s[q[a]], fy += wq[a] * s[q[a] + 1], fz += wq[a] * s[q[a] + 2];
        // the stored shifts are (-x, -y, +z): the field that moves the image is (+x, +y, +z)
        const float cx = __fadd_rn((float)x, (float)-fx), cy = __fadd_rn((float)y, (float)-fy), cz = __fadd_rn((float)z, (float)fz);
        float v = 0.0f;
        // any coordinate outside [0, n-1] (or not finite) is cval = 0
        if (cx >= 0.0f && cx <= (float)(X - 1) && cy >= 0.0f && cy <= (float)(Y - 1) && cz >= 0.0f && cz <= (float)(Z - 1)) {
            int ix[4], iy[4], iz[4];
            float wx[4], wy[4], wz[4];
            pw_taps(cx, X, ix, wx);
            pw_taps(cy, Y, iy, wy);
            const float *cf = coef + (long)f * P;
            if (HASZ) {
                pw_taps(cz, Z, iz, wz);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float sa = 0.0f;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float *r = cf + ((long)ix[a] * Y + iy[b]) * Z;
                        float sb = 0.0f;
#pragma unroll
                        for (int c = 0; c < 4; ++c) sb = fmaf(wz[c], r[iz[c]], sb);
                        sa = fmaf(wy[b], sb, sa);
                    }
                    v = fmaf(wx[a], sa, v);
                }
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float sa = 0.0f;
#pragma unroll
                    for (int b = 0; b < 4; ++b) sa = fmaf(wy[b], cf[(long)ix[a] * Y + iy[b]], sa);
                    v = fmaf(wx[a], sa, v);
                }
            }
            // skimage's _clip_warp_output: an exact cval stays, the rest is clipped to the frame's range
            if (v != 0.0f) v = fminf(fmaxf(v, pw_unord(lohi[2 * f])), pw_unord(lohi[2 * f + 1]));
        }
        const float o = __fsub_rn(v, add);
        out[(long)f * ldo + g] = o;
        if (o == o) acc += o, ++cnt;
    }
    if (part) part[(long)blockIdx.y * P + g] = acc, partc[(long)blockIdx.y * P + g] = cnt;
    else if (tsum) tsum[g] += acc, tcount[g] += cnt;
}

__global__ __launch_bounds__(256) void pw_sum_kernel(const float *part, const int *partc, int groups, unsigned P, float *tsum,
                                                     int *tcount) {
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P) return;
    float acc = 0.0f;
    int cnt = 0;
    for (int k = 0; k < groups; ++k) acc += part[(long)k * P + g], cnt += partc[(long)k * P + g];
    tsum[g] += acc, tcount[g] += cnt;
}

// frames per chunk: two coefficient buffers of at most 512 MiB together
int pw_chunk(long P, int B) {
    long c = (512L << 20) / (8 * P);
    if (c > 65535) c = 65535;
    if (c < 1) c = 1;
    if (c > B) c = B;
    return (int)c;
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_apply_pwrigid_workspace(int X, int Y, int Z, const int *strides, const int *overlaps, int B) {
    using namespace dnmf;
    if (X <= 0 || Y <= 0 || Z <= 0 || B <= 0) return 0;
    if (dnmf_register_patches_grid(X, Y, Z, strides, overlaps, nullptr, nullptr) <= 0) return 0;
    const long P = (long)X * Y * Z;
    const int Bc = pw_chunk(P, B);
    return 2 * align256((size_t)Bc * P * sizeof(float)) + align256((size_t)Bc * 2 * sizeof(unsigned));
}

int dnmf_apply_pwrigid(const float *frames, long ldf, const int *frame_ids, int B, int X, int Y, int Z, const int *strides,
                       const int *overlaps, const float *patch_shifts, float add_to_movie, float *out, long ldo, float *tsum,
                       int *tcount, void *workspace, size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames && strides && overlaps && patch_shifts && out && workspace, DNMF_E_NULL, "dnmf_apply_pwrigid: NULL argument");
    DNMF_REQUIRE((tsum == nullptr) == (tcount == nullptr), DNMF_E_NULL, "dnmf_apply_pwrigid: tsum and tcount go together");
    const long P = (long)X * Y * Z;
    DNMF_REQUIRE(X > 0 && Y > 0 && Z > 0 && B > 0 && ldf >= P && ldo >= P && P < (1L << 31), DNMF_E_SHAPE,
                 "dnmf_apply_pwrigid: X=%d Y=%d Z=%d B=%d ldf=%ld ldo=%ld", X, Y, Z, B, ldf, ldo);
    int dims[3];
    const int NP = dnmf_register_patches_grid(X, Y, Z, strides, overlaps, dims, nullptr);
    DNMF_REQUIRE(NP > 0, DNMF_E_SHAPE, "dnmf_apply_pwrigid: strides + overlaps must fit the volume");
    const size_t need = dnmf_apply_pwrigid_workspace(X, Y, Z, strides, overlaps, B);
    DNMF_REQUIRE(workspace_bytes >= need, DNMF_E_WORKSPACE, "dnmf_apply_pwrigid: workspace %zu < %zu bytes", workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    const int Bc = pw_chunk(P, B);
    char *ws = static_cast<char *>(workspace);
    float *bufA = reinterpret_cast<float *>(ws);
    float *bufB = reinterpret_cast<float *>(ws + align256((size_t)Bc * P * sizeof(float)));
    unsigned *lohi = reinterpret_cast<unsigned *>(ws + 2 * align256((size_t)Bc * P * sizeof(float)));
    const long YZ = (long)Y * Z;
    const unsigned bP = (unsigned)((P + 255) / 256);
    for (int f0 = 0; f0 < B; f0 += Bc) {
        const int nf = B - f0 < Bc ? B - f0 : Bc;
        hipLaunchKernelGGL(pw_range_init_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, lohi, nf);
        hipLaunchKernelGGL(pw_fir_x_kernel, dim3((unsigned)((YZ + 255) / 256), (unsigned)((X + PW_SX - 1) / PW_SX), (unsigned)nf),
                           dim3(256), 0, st, frames, ldf, frame_ids, f0, add_to_movie, X, YZ, bufA, P, lohi);
        float *cur = bufA, *nxt = bufB;
        if (Y > 1) {
            hipLaunchKernelGGL(pw_fir_kernel, dim3(bP, (unsigned)nf), dim3(256), 0, st, cur, nxt, (unsigned)P, Y, (unsigned)Z);
            float *t = cur;
            cur = nxt, nxt = t;
        }
        if (Z > 1) {
            hipLaunchKernelGGL(pw_fir_kernel, dim3(bP, (unsigned)nf), dim3(256), 0, st, cur, nxt, (unsigned)P, Z, 1u);
            float *t = cur;
            cur = nxt, nxt = t;
        }
        // with tsum: up to 32 frame groups, their partial sums (floats, then ints) in the free coefficient buffer
        int groups = nf;
        if (tsum) groups = nf < 32 ? nf : 32, groups = groups < Bc / 2 ? groups : Bc / 2, groups = groups < 1 ? 1 : groups;
        float *part = tsum && groups > 1 ? nxt : nullptr;
        int *partc = part ? reinterpret_cast<int *>(nxt + (long)groups * P) : nullptr;
        const float *sh = patch_shifts + (long)f0 * NP * 3;
        float *o = out + (long)f0 * ldo;
        if (Z > 1)
            hipLaunchKernelGGL(pw_eval_kernel<true>, dim3(bP, (unsigned)groups), dim3(256), 0, st, cur, nf, X, Y, Z, dims[0], dims[1], dims[2], sh,
                               NP, lohi, add_to_movie, o, ldo, tsum, tcount, part, partc);
        else
            hipLaunchKernelGGL(pw_eval_kernel<false>, dim3(bP, (unsigned)groups), dim3(256), 0, st, cur, nf, X, Y, Z, dims[0], dims[1], dims[2], sh,
                               NP, lohi, add_to_movie, o, ldo, tsum, tcount, part, partc);
        if (part) hipLaunchKernelGGL(pw_sum_kernel, dim3(bP), dim3(256), 0, st, part, partc, groups, (unsigned)P, tsum, tcount);
    }
    return check_launch("dnmf_apply_pwrigid");
}

}  // extern "C"
