// K18: summary images of a video -- per voxel mean, std (population), max over time and the local correlation image (the
// mean Pearson correlation with the 6 / 26 neighbours).  include/dnmf_hip.h has the contract, tests/summary_restatement.py
// the definition in float64.
//
// One pass over the movie.  A workgroup owns a tile of SI_TX x SI_TC voxels of the (x, c = y Z + z) plane and a segment of
// frames; per frame it stages the tile plus a halo of one x row and Z + 1 columns in LDS (double buffered: one barrier a
// frame, the next frame's loads are in flight while this one is summed), and every thread keeps the float64 sums of its
// voxel in registers: sum d, sum d^2 and sum d_p d_q for the half-set of directions (13 / 3; 4 / 2 at Z == 1), d = x - x0
// with x0 the voxel's value in the first frame after the reset.  The differences are exact in float64, so a constant voxel
// has a variance of exactly 0.  The partial sums of a segment go to the workspace; a second kernel adds the segments to the
// state in a fixed order (no floating-point atomics: the same input gives the same bits), a third writes the images.
#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int SI_TX = 16, SI_TC = 64, SI_THREADS = SI_TX * SI_TC;
constexpr int SI_SLOTS = 2;          // staged values a thread keeps in registers (enough for Z <= 23)
constexpr int SI_MIN_SEGMENT = 16;   // frames: below this the partial sums cost more traffic than the frames
constexpr int SI_TARGET_BLOCKS = 1024;
constexpr int SI_MAX_Z = 137;        // two staged tiles within 48 KiB of LDS
constexpr size_t SI_HEADER = 256;    // bytes: the frame count

// The half-set of the 26 directions in lexicographic order, m = 0..12: (0,0,1) (0,1,-1) (0,1,0) (0,1,1) (1,-1,-1) ... (1,1,1).
__host__ __device__ constexpr int dir_dx(int m) { return m >= 4 ? 1 : 0; }
__host__ __device__ constexpr int dir_dy(int m) { return m == 0 ? 0 : (m <= 3 ? 1 : (m - 4) / 3 - 1); }
__host__ __device__ constexpr int dir_dz(int m) { return m == 0 ? 1 : (m <= 3 ? m - 2 : (m - 4) % 3 - 1); }
// direction k of a neighbourhood -> m.  full: all 13, without z the four with dz == 0; face: z, y, x.
__host__ __device__ constexpr int dir_of(bool full, bool hasz, int k) {
    return full ? (hasz ? k : 2 + 3 * k) : (hasz ? (k == 0 ? 0 : (k == 1 ? 2 : 8)) : (k == 0 ? 2 : 8));
}
__host__ __device__ constexpr int dir_count(bool full, bool hasz) { return full ? (hasz ? 13 : 4) : (hasz ? 3 : 2); }

struct SummaryPlan : SegmentPlan {
    int X, Y, Z, full, nd;
    long P, plane;
    int ntx, ntc;
    size_t off_sums, off_max, off_pivot, off_part, off_pmax, bytes;   // sums: (2 + nd, P) float64
};

// Everything the two entries agree on; validates what both take.
int summary_plan(const char *fn, const int *sz, int neighbours, int B, int segment, SummaryPlan &g) {
    DNMF_REQUIRE(sz, DNMF_E_NULL, "%s: sz is NULL", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(B >= 1, DNMF_E_SHAPE, "%s: B=%d frames", fn, B);
    DNMF_REQUIRE(neighbours == DNMF_NEIGHBOURS_FACE || neighbours == DNMF_NEIGHBOURS_FULL, DNMF_E_SHAPE,
                 "%s: neighbours=%d (0 face, 1 full)", fn, neighbours);
    g.X = sz[0], g.Y = sz[1], g.Z = sz[2], g.full = neighbours == DNMF_NEIGHBOURS_FULL;
    g.P = (long)g.X * g.Y * g.Z, g.plane = (long)g.Y * g.Z;
    DNMF_REQUIRE(g.P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, g.P);
    DNMF_REQUIRE(g.Z <= SI_MAX_Z, DNMF_E_UNSUPPORTED, "%s: Z=%d, at most %d (the halo of a tile is Z + 1 columns)", fn, g.Z, SI_MAX_Z);
    g.nd = dir_count(g.full, g.Z > 1);
    g.ntx = (g.X + SI_TX - 1) / SI_TX, g.ntc = (int)((g.plane + SI_TC - 1) / SI_TC);
    const int rc = segment_plan(fn, B, segment, (long)g.ntx * g.ntc, SI_TARGET_BLOCKS, SI_MIN_SEGMENT, g);
    if (rc != DNMF_OK) return rc;
    const size_t P = (size_t)g.P, sums = align256((size_t)(2 + g.nd) * P * sizeof(double)), fl = align256(P * sizeof(float));
    g.off_sums = SI_HEADER;
    g.off_max = g.off_sums + sums;
    g.off_pivot = g.off_max + fl;
    g.off_part = g.off_pivot + fl;
    g.off_pmax = g.off_part + (size_t)g.cap * sums;
    g.bytes = g.off_pmax + (size_t)g.cap * fl;
    return DNMF_OK;
}

struct SummaryArgs {
    const float *frames, *sub;
    long ldf, lds;
    const int *frame_ids;
    int X, Z, B, seglen, first;
    int plane, ntc;
    const float *pivot_in;   // the state's pivot (first == 0)
    float *pivot_out;        // the state's pivot (first != 0: segment 0 writes it)
    double *part;            // (nseg, 2 + ND, P)
    float *pmax;             // (nseg, P)
    size_t part_stride;      // doubles between two segments
    size_t pmax_stride;      // floats between two segments
    long P;
};

// One staged value: entry i of the (SI_TX + 2) x W tile -> its offset inside a frame, -1 outside the volume.
__device__ __forceinline__ int slot_offset(int i, int W, int gx0, int gc0, int X, int plane) {
    const int r = i / W, j = i - r * W;
    const int gx = gx0 + r, gc = gc0 + j;
    return (gx >= 0 && gx < X && gc >= 0 && gc < plane) ? gx * plane + gc : -1;
}

__device__ __forceinline__ float sample(const float *fr, const float *sb, int off) {
    if (off < 0) return 0.0f;
    return sb ? __fsub_rn(fr[off], sb[off]) : fr[off];
}

template <bool FULL, bool HASZ>
__global__ __launch_bounds__(SI_THREADS) void summary_accumulate_kernel(SummaryArgs a) {
    constexpr int ND = dir_count(FULL, HASZ);
    extern __shared__ float tile[];
    const int H = a.Z + 1, W = SI_TC + 2 * H, n = (SI_TX + 2) * W;
    const int tid = threadIdx.x, lx = tid / SI_TC, lc = tid - lx * SI_TC;
    const int tx = blockIdx.x / a.ntc, tc = blockIdx.x - tx * a.ntc;
    const int gx0 = tx * SI_TX - 1, gc0 = tc * SI_TC - H;
    const int seg = blockIdx.y;
    const int f0 = seg * a.seglen, f1 = min(a.B, f0 + a.seglen);

    int off[SI_SLOTS];
#pragma unroll
    for (int k = 0; k < SI_SLOTS; ++k) {
        const int i = tid + k * SI_THREADS;
        off[k] = i < n ? slot_offset(i, W, gx0, gc0, a.X, a.plane) : -2;   // -2: no such entry
    }
    auto row = [&](int j) { return a.frames + (long)(a.frame_ids ? a.frame_ids[j] : j) * a.ldf; };
    auto subrow = [&](int j) { return a.sub ? a.sub + (long)j * a.lds : nullptr; };
    // entries beyond the register slots (Z > 23) go straight to LDS
    auto stage_rest = [&](float *buf, const float *fr, const float *sb) {
        for (int i = tid + SI_SLOTS * SI_THREADS; i < n; i += SI_THREADS) buf[i] = sample(fr, sb, slot_offset(i, W, gx0, gc0, a.X, a.plane));
    };

    const int gx = gx0 + 1 + lx, gc = gc0 + H + lc;
    const bool live = gx < a.X && gc < a.plane;
    const int own = (lx + 1) * W + H + lc;
    int nb[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        constexpr bool f = FULL, h = HASZ;
        const int m = dir_of(f, h, k);
        nb[k] = own + dir_dx(m) * W + dir_dy(m) * a.Z + dir_dz(m);
    }

    // the pivots of the voxel and of its ND neighbours, through the second buffer
    float x0, p0[ND];
    {
        float *buf = tile + n;
        const float *fr = a.first ? row(0) : a.pivot_in, *sb = a.first ? subrow(0) : nullptr;
#pragma unroll
        for (int k = 0; k < SI_SLOTS; ++k)
            if (off[k] != -2) buf[tid + k * SI_THREADS] = sample(fr, sb, off[k]);
        stage_rest(buf, fr, sb);
        __syncthreads();
        x0 = buf[own];
#pragma unroll
        for (int k = 0; k < ND; ++k) p0[k] = buf[nb[k]];
        if (a.first && seg == 0 && live) a.pivot_out[(long)gx * a.plane + gc] = x0;
    }

    double s1 = 0.0, s2 = 0.0, cr[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) cr[k] = 0.0;
    float mx = -__builtin_inff();
    bool bad = false;
    const double x0d = (double)x0;

    float v[SI_SLOTS];
    {
        const float *fr = row(f0), *sb = subrow(f0);
#pragma unroll
        for (int k = 0; k < SI_SLOTS; ++k) v[k] = off[k] != -2 ? sample(fr, sb, off[k]) : 0.0f;
    }
    for (int f = f0; f < f1; ++f) {
        float *buf = tile + ((f - f0) & 1) * n;
#pragma unroll
        for (int k = 0; k < SI_SLOTS; ++k)
            if (off[k] != -2) buf[tid + k * SI_THREADS] = v[k];
        if (n > SI_SLOTS * SI_THREADS) stage_rest(buf, row(f), subrow(f));
        __syncthreads();
        if (f + 1 < f1) {
            const float *fr = row(f + 1), *sb = subrow(f + 1);
#pragma unroll
            for (int k = 0; k < SI_SLOTS; ++k) v[k] = off[k] != -2 ? sample(fr, sb, off[k]) : 0.0f;
        }
        const float xv = buf[own];
        const double d = (double)xv - x0d;
        s1 += d;
        s2 = fma(d, d, s2);
#pragma unroll
        for (int k = 0; k < ND; ++k) cr[k] = fma(d, (double)buf[nb[k]] - (double)p0[k], cr[k]);
        mx = fmaxf(mx, xv);
        bad = bad || !__builtin_isfinite(xv);
    }
    if (!live) return;
    const long p = (long)gx * a.plane + gc;
    double *out = a.part + (size_t)seg * a.part_stride + p;
    // a voxel with a sample that is not finite is marked by a NaN sum
    out[0] = bad ? __builtin_nan("") : s1;
    out[a.P] = s2;
#pragma unroll
    for (int k = 0; k < ND; ++k) out[(long)(2 + k) * a.P] = cr[k];
    a.pmax[(size_t)seg * a.pmax_stride + p] = mx;
}

// state = (first ? 0 : state) + the segments in their order; the frame count
__global__ __launch_bounds__(256) void summary_reduce_kernel(const double *__restrict__ part, const float *__restrict__ pmax,
                                                             size_t part_stride, size_t pmax_stride, int nseg, int rows, long P, int first,
                                                             int B, double *__restrict__ sums, float *__restrict__ smax,
                                                             long long *__restrict__ count) {
    const long total = (long)rows * P;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *count = first ? (long long)B : *count + B;
    if (i < total) {
        double acc = first ? 0.0 : sums[i];
        for (int s = 0; s < nseg; ++s) acc += part[(size_t)s * part_stride + i];
        sums[i] = acc;
    }
    if (i < P) {
        float m = first ? -__builtin_inff() : smax[i];
        for (int s = 0; s < nseg; ++s) m = fmaxf(m, pmax[(size_t)s * pmax_stride + i]);
        smax[i] = m;
    }
}

struct VoxelStat {
    double s1, var;
    bool ok;   // every sample finite
};

__device__ __forceinline__ VoxelStat voxel_stat(const double *sums, long P, long p, double T) {
    VoxelStat v;
    v.s1 = sums[p];
    const double s2 = sums[P + p];
    v.ok = __builtin_isfinite(v.s1) && __builtin_isfinite(s2);
    v.var = fmax(0.0, (s2 - v.s1 * v.s1 / T) / T);
    return v;
}

// images (4, P): mean, std, max, corr
__global__ __launch_bounds__(256) void summary_finish_kernel(const double *__restrict__ sums, const float *__restrict__ smax,
                                                             const float *__restrict__ pivot, const long long *__restrict__ count, int X,
                                                             int Y, int Z, int full, double *__restrict__ images) {
    const long P = (long)X * Y * Z;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double T = (double)*count, nan = __builtin_nan("");
    const int z = (int)(p % Z), y = (int)((p / Z) % Y), x = (int)(p / ((long)Y * Z));
    const VoxelStat me = voxel_stat(sums, P, p, T);
    if (!me.ok) {
        images[p] = images[P + p] = images[2 * P + p] = images[3 * P + p] = nan;
        return;
    }
    images[p] = (double)pivot[p] + me.s1 / T;
    images[P + p] = sqrt(me.var);
    images[2 * P + p] = (double)smax[p];
    const bool hasz = Z > 1;
    const int nd = dir_count(full != 0, hasz);
    const double sdp = sqrt(me.var);
    double acc = 0.0;
    int pairs = 0;
    for (int k = 0; k < nd; ++k) {
        const int m = dir_of(full != 0, hasz, k);
        const int dx = dir_dx(m), dy = dir_dy(m), dz = dir_dz(m);
        const long step = ((long)dx * Y + dy) * Z + dz;
        for (int sgn = 1; sgn >= -1; sgn -= 2) {
            const int qx = x + sgn * dx, qy = y + sgn * dy, qz = z + sgn * dz;
            if (qx < 0 || qx >= X || qy < 0 || qy >= Y || qz < 0 || qz >= Z) continue;
            const long q = p + sgn * step;
            const VoxelStat nbr = voxel_stat(sums, P, q, T);
            if (!nbr.ok || !(nbr.var > 0.0) || !(me.var > 0.0)) continue;
            // the product of the pair sits with the voxel the direction starts from
            const double spq = sums[(long)(2 + k) * P + (sgn > 0 ? p : q)];
            const double cov = (spq - me.s1 * nbr.s1 / T) / T;
            acc += cov / (sdp * sqrt(nbr.var));
            ++pairs;
        }
    }
    images[3 * P + p] = pairs ? acc / (double)pairs : nan;
}

template <bool FULL, bool HASZ>
void launch_accumulate(const SummaryPlan &g, const SummaryArgs &a, hipStream_t st) {
    const size_t lds = 2 * (size_t)(SI_TX + 2) * (SI_TC + 2 * (g.Z + 1)) * sizeof(float);
    hipLaunchKernelGGL((summary_accumulate_kernel<FULL, HASZ>), dim3((unsigned)(g.ntx * g.ntc), (unsigned)g.nseg), dim3(SI_THREADS), lds, st, a);
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_summary_images_workspace(const int *sz, int neighbours, int B, int segment) {
    dnmf::SummaryPlan g;
    if (dnmf::summary_plan("dnmf_summary_images_workspace", sz, neighbours, B, segment, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_summary_images(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const int *sz, int B,
                        int neighbours, int first, int finish, int segment, void *state, size_t state_bytes, double *images,
                        dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(frames && state && sz, DNMF_E_NULL, "dnmf_summary_images: NULL argument");
    DNMF_REQUIRE(images || !finish, DNMF_E_NULL, "dnmf_summary_images: images is NULL with finish");
    SummaryPlan g;
    const int rc = summary_plan("dnmf_summary_images", sz, neighbours, B, segment, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= g.P && (!sub || lds >= g.P), DNMF_E_SHAPE, "dnmf_summary_images: ldf=%ld lds=%ld below a row of P=%ld", ldf, lds, g.P);
    DNMF_REQUIRE((long)g.ntx * g.ntc < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_summary_images: %ld tiles", (long)g.ntx * g.ntc);
    DNMF_REQUIRE(state_bytes >= g.bytes, DNMF_E_WORKSPACE, "dnmf_summary_images: state of %zu bytes, need %zu", state_bytes, g.bytes);
    DNMF_REQUIRE(((size_t)state & 7) == 0, DNMF_E_WORKSPACE, "dnmf_summary_images: state must be 8-byte aligned");
    char *w = static_cast<char *>(state);
    long long *count = reinterpret_cast<long long *>(w);
    double *sums = reinterpret_cast<double *>(w + g.off_sums);
    float *smax = reinterpret_cast<float *>(w + g.off_max);
    float *pivot = reinterpret_cast<float *>(w + g.off_pivot);
    const size_t sums_bytes = g.off_max - g.off_sums, fl_bytes = g.off_pivot - g.off_max;
    SummaryArgs a;
    a.frames = frames, a.sub = sub, a.ldf = ldf, a.lds = lds, a.frame_ids = frame_ids;
    a.X = g.X, a.Z = g.Z, a.B = B, a.seglen = g.seglen, a.first = first != 0;
    a.plane = (int)g.plane, a.ntc = g.ntc;
    a.pivot_in = pivot, a.pivot_out = pivot;
    a.part = reinterpret_cast<double *>(w + g.off_part), a.pmax = reinterpret_cast<float *>(w + g.off_pmax);
    a.part_stride = sums_bytes / sizeof(double), a.pmax_stride = fl_bytes / sizeof(float);
    a.P = g.P;
    const hipStream_t st = (hipStream_t)stream;
    const bool hasz = g.Z > 1;
    if (g.full && hasz) launch_accumulate<true, true>(g, a, st);
    else if (g.full) launch_accumulate<true, false>(g, a, st);
    else if (hasz) launch_accumulate<false, true>(g, a, st);
    else launch_accumulate<false, false>(g, a, st);
    const long total = (long)(2 + g.nd) * g.P;
    hipLaunchKernelGGL(summary_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.part, a.pmax, a.part_stride,
                       a.pmax_stride, g.nseg, 2 + g.nd, g.P, a.first, B, sums, smax, count);
    if (finish)
        hipLaunchKernelGGL(summary_finish_kernel, dim3((unsigned)((g.P + 255) / 256)), dim3(256), 0, st, sums, smax, pivot, count, g.X, g.Y,
                           g.Z, g.full, images);
    return check_launch("dnmf_summary_images");
}

}  // extern "C"
