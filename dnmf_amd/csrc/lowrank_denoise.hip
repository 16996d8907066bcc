// K34: local low-rank denoising of a registered movie -- per patch a truncated SVD by subspace iteration, the patches blended
// by tent weights.  include/dnmf_hip.h has the contract, tests/denoise_restatement.py the definition.
//
// The patches of a plan all have the same shape (a patch larger than an axis is the axis, the last one is clamped to the
// volume), so a patch is its index p = (ix cy + iy) cz + iz and the per-axis triple (count, stride, len): no table of boxes goes
// to the device.  D[v, t] = (y[v, t] - centre[v]) / scale[v] in float64, v the voxel's index in the patch (z fastest).
//
// K34a / K34c (lowrank_pass_kernel): one workgroup of 256 threads per patch.  U (n x R float64) sits in LDS for the whole call;
// the frames go through in tiles of F = 32 (16 above 256 voxels, 8 above 512: the tile of D is F (n + 1) doubles, one double
// of padding a row so that the lanes of a wave that read one voxel of 8 frames hit 8 banks).  Per tile: every thread loads its
// up to 4 voxels of every frame and stores D; lane (f, j) forms q[f, j] = sum_v D[v, f] U[v, j] over v = 0 .. n - 1 in that
// order; then (K34a) the thread that owns entry (v, j) of W adds D[v, f] q[f, j] for f in frame order, W read and written once
// a tile, or (K34c) q goes to Q and sum_v D^2 to the energy table.  The order of every sum is fixed by v and by the frame, not
// by the tile or the call: the same bits however the movie is cut.  A sample, centre or scale that is not usable clears ok[p];
// a patch with ok = 0 is skipped from then on.
// K34b (lowrank_mgs_kernel): modified Gram-Schmidt of W in LDS, block_reduce sums (block_ops.hpp: a fixed tree).
// K34d (lowrank_ritz_kernel): B = Q^T Q by four waves over four quarters of the frames, cyclic Jacobi by thread 0 in LDS, the
// order of the eigenvalues, kept, explained, and the rotation of the rows of U and Q, a row a thread.
// K34e (lowrank_blend_kernel): a thread owns a voxel and 8 consecutive frames, walks the patches that cover the voxel in
// ascending p and holds the 8 partial sums in registers; U is read once per patch and column for the 8 frames.
// No kernel indexes a register array by a run-time value (R is a guard inside unrolled loops of 8): no scratch.
#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_MAX_VOXELS = 1024;
constexpr int LR_MAX_RANK = 8;
constexpr int LR_SLOTS = LR_MAX_VOXELS / LR_THREADS;   // voxels of a thread
constexpr int LR_BLEND_FRAMES = 8;                     // frames of a thread of K34e

struct LRAxis {
    int count, stride, len, last;   // last = extent - len, the start of the clamped patch
    __host__ __device__ int start(int i) const {
        const long s = (long)i * stride;
        return (int)(s < last ? s : last);
    }
};

struct LRPlan {
    LRAxis ax[3];
    int X, Y, Z, n;
    long NP, P;
};

inline int tile_frames(int n) { return n <= 256 ? 32 : n <= 512 ? 16 : 8; }

// plan: per axis (count, stride, len), 9 ints on the host
int make_plan(const char *fn, const int *sz, const int *plan, LRPlan &p) {
    DNMF_REQUIRE(sz && plan, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    p.X = sz[0], p.Y = sz[1], p.Z = sz[2];
    p.P = (long)sz[0] * sz[1] * sz[2];
    DNMF_REQUIRE(p.P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, p.P);
    long n = 1, np = 1;
    for (int a = 0; a < 3; ++a) {
        const int count = plan[3 * a], stride = plan[3 * a + 1], len = plan[3 * a + 2];
        DNMF_REQUIRE(count >= 1 && stride >= 1 && len >= 1 && len <= sz[a], DNMF_E_SHAPE,
                     "%s: axis %d: %d patches of %d every %d on an extent of %d", fn, a, count, len, stride, sz[a]);
        const int last = sz[a] - len;
        // the patches reach the end, each starts where the one before it has not ended, and none repeats the clamped one
        DNMF_REQUIRE((long)(count - 1) * stride >= last && (count == 1 || (long)(count - 2) * stride < last) && (count == 1 || stride <= len),
                     DNMF_E_SHAPE, "%s: axis %d: %d patches of %d every %d do not tile an extent of %d", fn, a, count, len, stride, sz[a]);
        p.ax[a].count = count, p.ax[a].stride = stride, p.ax[a].len = len, p.ax[a].last = last;
        n *= len, np *= count;
    }
    DNMF_REQUIRE(n <= LR_MAX_VOXELS, DNMF_E_UNSUPPORTED, "%s: a patch of %ld voxels, at most %d (a patch is never cut)", fn, n, LR_MAX_VOXELS);
    DNMF_REQUIRE(np < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld patches", fn, np);
    p.n = (int)n, p.NP = np;
    return DNMF_OK;
}

struct PatchOrigin {
    int x0, y0, z0;
};

__device__ __forceinline__ PatchOrigin patch_origin(const LRPlan &pl, long p) {
    const int cy = pl.ax[1].count, cz = pl.ax[2].count;
    PatchOrigin o;
    o.z0 = pl.ax[2].start((int)(p % cz));
    o.y0 = pl.ax[1].start((int)((p / cz) % cy));
    o.x0 = pl.ax[0].start((int)(p / ((long)cz * cy)));
    return o;
}

struct PassArgs {
    const float *frames;
    long ldf;
    const int *frame_ids;
    int B;
    long row0, T;   // K34c: the rows are the frames row0 .. of the T of Q and energy
    LRPlan pl;
    int R, F;
    const double *centre, *scale, *U;
    double *W, *Q, *energy;
    int *ok;
};

template <bool PROJECT>
__global__ __launch_bounds__(LR_THREADS) void lowrank_pass_kernel(PassArgs a) {
    extern __shared__ double lr_lds[];
    const long p = blockIdx.x;
    if (a.ok[p] == 0) return;   // the whole workgroup: nobody else writes ok[p]
    const int tid = threadIdx.x, n = a.pl.n, R = a.R, F = a.F, ldd = n + 1;
    double *Us = lr_lds, *Dt = Us + (size_t)n * R, *qs = Dt + (size_t)F * ldd;
    const PatchOrigin o = patch_origin(a.pl, p);
    const int ny = a.pl.ax[1].len, nz = a.pl.ax[2].len;
    long off[LR_SLOTS];
    double c[LR_SLOTS], s[LR_SLOTS];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < LR_SLOTS; ++k) {
        const int i = tid + k * LR_THREADS;
        off[k] = 0, c[k] = 0.0, s[k] = 1.0;
        if (i < n) {
            const int lz = i % nz, ly = (i / nz) % ny, lx = i / (nz * ny);
            off[k] = ((long)(o.x0 + lx) * a.pl.Y + (o.y0 + ly)) * a.pl.Z + (o.z0 + lz);
            c[k] = a.centre[off[k]];
            if (a.scale) s[k] = a.scale[off[k]];
            bad = bad || !__builtin_isfinite(c[k]) || !(s[k] > 0.0) || !__builtin_isfinite(s[k]);
        }
    }
    const size_t base = (size_t)p * n * R;
    for (int e = tid; e < n * R; e += LR_THREADS) Us[e] = a.U[base + e];
    for (int b0 = 0; b0 < a.B; b0 += F) {
        const int Fc = a.B - b0 < F ? a.B - b0 : F;
        __syncthreads();   // the tile before this one has been read (and, the first time, U is in LDS)
        for (int f = 0; f < Fc; ++f) {
            const float *row = a.frames + (long)(a.frame_ids ? a.frame_ids[b0 + f] : b0 + f) * a.ldf;
            float y[LR_SLOTS];
#pragma unroll
            for (int k = 0; k < LR_SLOTS; ++k) y[k] = tid + k * LR_THREADS < n ? row[off[k]] : 0.0f;
#pragma unroll
            for (int k = 0; k < LR_SLOTS; ++k)
                if (tid + k * LR_THREADS < n) {
                    bad = bad || !__builtin_isfinite(y[k]);
                    Dt[f * ldd + tid + k * LR_THREADS] = ((double)y[k] - c[k]) / s[k];
                }
        }
        __syncthreads();
        if (tid < Fc * R) {
            const int f = tid / R, j = tid % R;
            const double *d = Dt + f * ldd;
            double q = 0.0, en = 0.0;
            for (int v = 0; v < n; ++v) {
                const double dv = d[v];
                q = fma(dv, Us[v * R + j], q);
                if (PROJECT) en = fma(dv, dv, en);
            }
            if (PROJECT) {
                const size_t t = (size_t)p * a.T + (size_t)(a.row0 + b0 + f);
                a.Q[t * R + j] = q;
                if (j == 0) a.energy[t] = en;
            } else {
                qs[f * LR_MAX_RANK + j] = q;
            }
        }
        if (!PROJECT) {
            __syncthreads();
            for (int e = tid; e < n * R; e += LR_THREADS) {
                const int v = e / R, j = e % R;
                double acc = a.W[base + e];
                for (int f = 0; f < Fc; ++f) acc = fma(Dt[f * ldd + v], qs[f * LR_MAX_RANK + j], acc);
                a.W[base + e] = acc;
            }
        }
    }
    if (bad) a.ok[p] = 0;
}

__global__ __launch_bounds__(LR_THREADS) void lowrank_mgs_kernel(int n, int R, double *U, double *W, const int *ok) {
    extern __shared__ double lr_lds[];
    __shared__ double red[LR_THREADS / 64];
    double *Ws = lr_lds;
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * n * R;
    const bool live = ok[blockIdx.x] != 0;
    for (int e = tid; e < n * R; e += LR_THREADS) Ws[e] = live ? W[base + e] : 0.0;
    __syncthreads();
    auto dot = [&](int i, int j) {
        double s = 0.0;
        for (int v = tid; v < n; v += LR_THREADS) s = fma(Ws[v * R + i], Ws[v * R + j], s);
        return block_reduce<LR_THREADS>(s, OpSum(), red);
    };
    for (int j = 0; j < R; ++j) {
        const double before = sqrt(dot(j, j));
        for (int i = 0; i < j; ++i) {
            const double d = dot(i, j);
            for (int v = tid; v < n; v += LR_THREADS) Ws[v * R + j] = fma(-d, Ws[v * R + i], Ws[v * R + j]);
            __syncthreads();
        }
        const double after = sqrt(dot(j, j));
        const bool zero = after <= 1e-12 * before;
        for (int v = tid; v < n; v += LR_THREADS) Ws[v * R + j] = zero ? 0.0 : Ws[v * R + j] / after;
        __syncthreads();
    }
    for (int e = tid; e < n * R; e += LR_THREADS) U[base + e] = Ws[e], W[base + e] = 0.0;
}

struct RitzArgs {
    int n, R, keep, sweeps;
    long T;
    double edge;
    double *U, *Q;
    const double *energy;
    const int *ok;
    double *lam, *explained;
    int *kept;
};

// the rows r = tid, tid + 256, .. of M (rows x R) times the R x R matrix Vr (LDS, leading dimension 8), in place
__device__ __forceinline__ void rotate_rows(double *M, long rows, int R, const double *Vr) {
    for (long r = threadIdx.x; r < rows; r += LR_THREADS) {
        double old[LR_MAX_RANK];
#pragma unroll
        for (int i = 0; i < LR_MAX_RANK; ++i) old[i] = i < R ? M[r * R + i] : 0.0;
#pragma unroll
        for (int j = 0; j < LR_MAX_RANK; ++j) {
            if (j >= R) continue;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < LR_MAX_RANK; ++i)
                if (i < R) s = fma(old[i], Vr[i * LR_MAX_RANK + j], s);
            M[r * R + j] = s;
        }
    }
}

__global__ __launch_bounds__(LR_THREADS) void lowrank_ritz_kernel(RitzArgs a) {
    __shared__ double part[LR_THREADS], Bs[64], Vs[64], Vr[64], red[LR_THREADS / 64], lams[LR_MAX_RANK];
    __shared__ int ord[LR_MAX_RANK];
    const long p = blockIdx.x;
    const int tid = threadIdx.x, R = a.R;
    if (a.ok[p] == 0) {
        if (tid < R) a.lam[p * R + tid] = 0.0;
        if (tid == 0) a.kept[p] = 0, a.explained[p] = 0.0;
        return;
    }
    double *Q = a.Q + (size_t)p * a.T * R, *U = a.U + (size_t)p * a.n * R;
    // B = Q^T Q: wave w adds the frames of quarter w in order, then the four quarters in order
    {
        const int w = tid >> 6, e = tid & 63, i = e >> 3, j = e & 7;
        const long t0 = a.T * w / 4, t1 = a.T * (w + 1) / 4;
        double s = 0.0;
        if (i < R && j < R)
            for (long t = t0; t < t1; ++t) s = fma(Q[t * R + i], Q[t * R + j], s);
        part[tid] = s;
    }
    double en = 0.0;
    for (long t = tid; t < a.T; t += LR_THREADS) en += a.energy[(size_t)p * a.T + t];
    en = block_reduce<LR_THREADS>(en, OpSum(), red);   // its barriers publish part[]
    if (tid < 64) {
        Bs[tid] = ((part[tid] + part[64 + tid]) + part[128 + tid]) + part[192 + tid];
        Vs[tid] = (tid >> 3) == (tid & 7) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        for (int sweep = 0; sweep < a.sweeps; ++sweep)
            for (int x = 0; x < R - 1; ++x)
                for (int y = x + 1; y < R; ++y) {
                    const double bxy = Bs[x * 8 + y];
                    if (bxy == 0.0) continue;
                    const double tau = (Bs[y * 8 + y] - Bs[x * 8 + x]) / (2.0 * bxy);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                    for (int k = 0; k < R; ++k) {
                        const double u = Bs[k * 8 + x], v = Bs[k * 8 + y];
                        Bs[k * 8 + x] = c * u - s * v, Bs[k * 8 + y] = s * u + c * v;
                    }
                    for (int k = 0; k < R; ++k) {
                        const double u = Bs[x * 8 + k], v = Bs[y * 8 + k];
                        Bs[x * 8 + k] = c * u - s * v, Bs[y * 8 + k] = s * u + c * v;
                    }
                    for (int k = 0; k < R; ++k) {
                        const double u = Vs[k * 8 + x], v = Vs[k * 8 + y];
                        Vs[k * 8 + x] = c * u - s * v, Vs[k * 8 + y] = s * u + c * v;
                    }
                }
        // descending, ties by index
        for (int j = 0; j < R; ++j) {
            const double lj = Bs[j * 8 + j];
            int rank = 0;
            for (int i = 0; i < R; ++i) {
                const double li = Bs[i * 8 + i];
                rank += li > lj || (li == lj && i < j);
            }
            ord[rank] = j, lams[rank] = lj;
        }
        int kept = 0;
        if (a.keep < 0) {
            for (int j = 0; j < R; ++j) kept += lams[j] > a.edge;
        } else {
            for (int j = 0; j < R && j < a.keep; ++j) kept += lams[j] > 0.0;
        }
        double sum = 0.0;
        for (int j = 0; j < kept; ++j) sum += lams[j];
        a.kept[p] = kept;
        a.explained[p] = en > 0.0 ? sum / en : 0.0;
        for (int j = 0; j < R; ++j) a.lam[p * R + j] = lams[j];
    }
    __syncthreads();
    if (tid < 64) Vr[tid] = (tid & 7) < R ? Vs[(tid >> 3) * 8 + ord[tid & 7]] : 0.0;
    __syncthreads();
    rotate_rows(U, a.n, R, Vr);
    rotate_rows(Q, a.T, R, Vr);
}

struct BlendArgs {
    const float *frames;
    long ldf, ldo;
    const int *frame_ids;
    int B;
    long row0, T;
    LRPlan pl;
    int R;
    const double *centre, *scale, *U, *Q;
    const int *kept, *ok;
    float *out;
};

// the patches i0 .. i1 of an axis that hold the coordinate x
__device__ __forceinline__ void covering(const LRAxis &ax, int x, int &i0, int &i1) {
    i1 = x >= ax.last ? ax.count - 1 : x / ax.stride;
    const int need = x - ax.len + 1;   // the least start that still reaches x
    i0 = need <= 0 ? 0 : (need + ax.stride - 1) / ax.stride;
    if (i0 > ax.count - 1) i0 = ax.count - 1;
}

__global__ __launch_bounds__(LR_THREADS) void lowrank_blend_kernel(BlendArgs a) {
    const long v = (long)blockIdx.x * LR_THREADS + threadIdx.x;
    if (v >= a.pl.P) return;
    const int b0 = (int)blockIdx.y * LR_BLEND_FRAMES, R = a.R, n = a.pl.n;
    const int z = (int)(v % a.pl.Z), y = (int)((v / a.pl.Z) % a.pl.Y), x = (int)(v / ((long)a.pl.Z * a.pl.Y));
    const int ny = a.pl.ax[1].len, nz = a.pl.ax[2].len, cy = a.pl.ax[1].count, cz = a.pl.ax[2].count;
    int ix0, ix1, iy0, iy1, iz0, iz1;
    covering(a.pl.ax[0], x, ix0, ix1);
    covering(a.pl.ax[1], y, iy0, iy1);
    covering(a.pl.ax[2], z, iz0, iz1);
    const double c = a.centre[v], s = a.scale ? a.scale[v] : 1.0;
    double num[LR_BLEND_FRAMES];
#pragma unroll
    for (int f = 0; f < LR_BLEND_FRAMES; ++f) num[f] = 0.0;
    double den = 0.0;
    for (int ix = ix0; ix <= ix1; ++ix) {
        const int lx = x - a.pl.ax[0].start(ix);
        if (lx < 0 || lx >= a.pl.ax[0].len) continue;
        for (int iy = iy0; iy <= iy1; ++iy) {
            const int ly = y - a.pl.ax[1].start(iy);
            if (ly < 0 || ly >= ny) continue;
            for (int iz = iz0; iz <= iz1; ++iz) {
                const int lz = z - a.pl.ax[2].start(iz);
                if (lz < 0 || lz >= nz) continue;
                const long p = ((long)ix * cy + iy) * cz + iz;
                if (a.ok[p] == 0) continue;
                const int wx = min(lx + 1, a.pl.ax[0].len - lx), wy = min(ly + 1, ny - ly), wz = min(lz + 1, nz - lz);
                const double w = (double)(wx * wy * wz);
                const double *Up = a.U + ((size_t)p * n + (size_t)((lx * ny + ly) * nz + lz)) * R;
                const double *Qp = a.Q + (size_t)p * a.T * R;
                const int k = a.kept[p];
                double val[LR_BLEND_FRAMES];
#pragma unroll
                for (int f = 0; f < LR_BLEND_FRAMES; ++f) val[f] = 0.0;
                for (int j = 0; j < k; ++j) {
                    const double u = Up[j];
#pragma unroll
                    for (int f = 0; f < LR_BLEND_FRAMES; ++f) {
                        const int b = b0 + f < a.B ? b0 + f : a.B - 1;   // a frame past the call repeats the last one and is dropped
                        val[f] = fma(u, Qp[(size_t)(a.row0 + b) * R + j], val[f]);
                    }
                }
#pragma unroll
                for (int f = 0; f < LR_BLEND_FRAMES; ++f) num[f] += w * (c + s * val[f]);
                den += w;
            }
        }
    }
#pragma unroll
    for (int f = 0; f < LR_BLEND_FRAMES; ++f) {
        const int b = b0 + f;
        if (b >= a.B) break;
        float r;
        if (den > 0.0) r = (float)(num[f] / den);
        else r = a.frames[(long)(a.frame_ids ? a.frame_ids[b] : b) * a.ldf + v];
        a.out[(long)b * a.ldo + v] = r;
    }
}

int check_rank(const char *fn, int rank) {
    DNMF_REQUIRE(rank >= 1 && rank <= LR_MAX_RANK, DNMF_E_SHAPE, "%s: rank=%d outside [1, %d]", fn, rank, LR_MAX_RANK);
    return DNMF_OK;
}

int check_rows(const char *fn, const LRPlan &pl, long ldf, int B, long row0, long T) {
    DNMF_REQUIRE(B >= 1 && row0 >= 0 && T >= 1 && row0 + B <= T && T <= 2147483647L, DNMF_E_SHAPE, "%s: rows %ld .. %ld of T=%ld frames", fn,
                 row0, row0 + B, T);
    DNMF_REQUIRE(ldf >= pl.P, DNMF_E_SHAPE, "%s: ldf=%ld below a row of P=%ld", fn, ldf, pl.P);
    return DNMF_OK;
}

template <bool PROJECT>
int launch_pass(const char *fn, const PassArgs &a, hipStream_t st) {
    const size_t lds = ((size_t)a.pl.n * a.R + (size_t)a.F * (a.pl.n + 1) + (size_t)a.F * LR_MAX_RANK) * sizeof(double);
    if (lds > 48u * 1024u) {   // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void *)lowrank_pass_kernel<PROJECT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail((int)e, "%s: %zu bytes of LDS: %s", fn, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lowrank_pass_kernel<PROJECT>, dim3((unsigned)a.pl.NP), dim3(LR_THREADS), lds, st, a);
    return check_launch(fn);
}

}  // namespace
}  // namespace dnmf

extern "C" {

long dnmf_lowrank_patches(const int *sz, const int *plan) {
    dnmf::LRPlan p;
    if (dnmf::make_plan("dnmf_lowrank_patches", sz, plan, p) != DNMF_OK) return 0;
    return p.NP;
}

int dnmf_lowrank_tile_frames(int n) { return n >= 1 && n <= dnmf::LR_MAX_VOXELS ? dnmf::tile_frames(n) : 0; }

int dnmf_lowrank_accumulate(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, const int *plan, int rank,
                            const double *centre, const double *scale, const double *U, double *W, int *ok, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_lowrank_accumulate";
    DNMF_REQUIRE(frames && centre && U && W && ok, DNMF_E_NULL, "%s: NULL argument", fn);
    PassArgs a;
    int rc = make_plan(fn, sz, plan, a.pl);
    if (rc == DNMF_OK) rc = check_rank(fn, rank);
    if (rc == DNMF_OK) rc = check_rows(fn, a.pl, ldf, B, 0, B);
    if (rc != DNMF_OK) return rc;
    a.frames = frames, a.ldf = ldf, a.frame_ids = frame_ids, a.B = B, a.row0 = 0, a.T = B, a.R = rank, a.F = tile_frames(a.pl.n);
    a.centre = centre, a.scale = scale, a.U = U, a.W = W, a.Q = nullptr, a.energy = nullptr, a.ok = ok;
    return launch_pass<false>(fn, a, (hipStream_t)stream);
}

int dnmf_lowrank_orthonormalise(long NP, int n, int rank, double *U, double *W, const int *ok, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_lowrank_orthonormalise";
    DNMF_REQUIRE(U && W && ok, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(NP >= 1 && NP < (1L << 31) && n >= 1, DNMF_E_SHAPE, "%s: %ld patches of %d voxels", fn, NP, n);
    DNMF_REQUIRE(n <= LR_MAX_VOXELS, DNMF_E_UNSUPPORTED, "%s: a patch of %d voxels, at most %d", fn, n, LR_MAX_VOXELS);
    const int rc = check_rank(fn, rank);
    if (rc != DNMF_OK) return rc;
    const size_t lds = (size_t)n * rank * sizeof(double);
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute((const void *)lowrank_mgs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail((int)e, "%s: %zu bytes of LDS: %s", fn, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lowrank_mgs_kernel, dim3((unsigned)NP), dim3(LR_THREADS), lds, (hipStream_t)stream, n, rank, U, W, ok);
    return check_launch(fn);
}

int dnmf_lowrank_project(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, long T, const int *plan,
                         int rank, const double *centre, const double *scale, const double *U, double *Q, double *energy, int *ok,
                         dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_lowrank_project";
    DNMF_REQUIRE(frames && centre && U && Q && energy && ok, DNMF_E_NULL, "%s: NULL argument", fn);
    PassArgs a;
    int rc = make_plan(fn, sz, plan, a.pl);
    if (rc == DNMF_OK) rc = check_rank(fn, rank);
    if (rc == DNMF_OK) rc = check_rows(fn, a.pl, ldf, B, row0, T);
    if (rc != DNMF_OK) return rc;
    a.frames = frames, a.ldf = ldf, a.frame_ids = frame_ids, a.B = B, a.row0 = row0, a.T = T, a.R = rank, a.F = tile_frames(a.pl.n);
    a.centre = centre, a.scale = scale, a.U = U, a.W = nullptr, a.Q = Q, a.energy = energy, a.ok = ok;
    return launch_pass<true>(fn, a, (hipStream_t)stream);
}

int dnmf_lowrank_ritz(long NP, int n, long T, int rank, int keep, double edge, int sweeps, double *U, double *Q, const double *energy,
                      const int *ok, double *lam, int *kept, double *explained, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_lowrank_ritz";
    DNMF_REQUIRE(U && Q && energy && ok && lam && kept && explained, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(NP >= 1 && NP < (1L << 31) && n >= 1 && n <= LR_MAX_VOXELS && T >= 1, DNMF_E_SHAPE, "%s: %ld patches of %d voxels, T=%ld", fn, NP,
                 n, T);
    const int rc = check_rank(fn, rank);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(sweeps >= 0 && sweeps <= 64, DNMF_E_SHAPE, "%s: sweeps=%d outside [0, 64]", fn, sweeps);
    DNMF_REQUIRE(keep >= 0 || edge >= 0.0, DNMF_E_SHAPE, "%s: keep < 0 (by the noise edge) needs an edge >= 0, got %g", fn, edge);
    RitzArgs a;
    a.n = n, a.R = rank, a.keep = keep, a.sweeps = sweeps, a.T = T, a.edge = edge, a.U = U, a.Q = Q, a.energy = energy, a.ok = ok;
    a.lam = lam, a.explained = explained, a.kept = kept;
    hipLaunchKernelGGL(lowrank_ritz_kernel, dim3((unsigned)NP), dim3(LR_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}

int dnmf_lowrank_reconstruct(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, long T, const int *plan,
                             int rank, const double *centre, const double *scale, const double *U, const double *Q, const int *kept,
                             const int *ok, float *out, long ldo, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_lowrank_reconstruct";
    DNMF_REQUIRE(frames && centre && U && Q && kept && ok && out, DNMF_E_NULL, "%s: NULL argument", fn);
    BlendArgs a;
    int rc = make_plan(fn, sz, plan, a.pl);
    if (rc == DNMF_OK) rc = check_rank(fn, rank);
    if (rc == DNMF_OK) rc = check_rows(fn, a.pl, ldf, B, row0, T);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldo >= a.pl.P, DNMF_E_SHAPE, "%s: ldo=%ld below a row of P=%ld", fn, ldo, a.pl.P);
    const long chunks = ((long)B + LR_BLEND_FRAMES - 1) / LR_BLEND_FRAMES;
    DNMF_REQUIRE(chunks <= 65535, DNMF_E_UNSUPPORTED, "%s: B=%d rows (groups of %d ride on gridDim.y: at most 65535)", fn, B, LR_BLEND_FRAMES);
    a.frames = frames, a.ldf = ldf, a.ldo = ldo, a.frame_ids = frame_ids, a.B = B, a.row0 = row0, a.T = T, a.R = rank;
    a.centre = centre, a.scale = scale, a.U = U, a.Q = Q, a.kept = kept, a.ok = ok, a.out = out;
    hipLaunchKernelGGL(lowrank_blend_kernel, dim3((unsigned)((a.pl.P + LR_THREADS - 1) / LR_THREADS), (unsigned)chunks), dim3(LR_THREADS), 0,
                       (hipStream_t)stream, a);
    return check_launch(fn);
}

}  // extern "C"
