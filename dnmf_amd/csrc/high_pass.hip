// K22: spatial high-pass of every frame -- the filter MotionCorrect's gSig_filt registers on (high_pass_filter_space,
// reference MotionCorrect.py:1262-1270: cv2.filter2D with a zero-sum Gaussian disc, BORDER_REFLECT, slice by slice).
// include/dnmf_hip.h has the contract, tests/high_pass_restatement.py the definition in float64.
//
// A workgroup owns a tile of HP_TX x HP_TC voxels of the (x, c) plane and walks the frames of its share of the batch.  c is
// the contiguous axis: c = y Z + z with every slice interleaved (Zt = Z; a step in y is Z columns of the tile) while the tile
// plus its halo of h = n / 2 rows and h Z columns fits the LDS budget, else one slice per workgroup (Zt = 1, blockIdx.z = z;
// the loads then stride by Z floats).  Reflection is resolved once per workgroup into two offset tables (rows, columns);
// staging a frame is tile[r][j] = frame[rowoff[r] + coloff[j]], contiguous along c wherever nothing reflects, and the
// inner loop has no index arithmetic.  A lane owns HP_R outputs down x in one column: for tap column j it walks the rows of
// that column's run of non-zero taps (a disc: about 0.75 n^2 taps, never the full square) and every value read from LDS
// feeds up to HP_R fused multiply-adds, the taps sliding through a register window (they are wave-uniform: scalar loads).
// Output r sums its taps in the order j ascending, i ascending: fp32 FMAs in a fixed order, no atomics, the same bits on
// every run.  Taps that are zero are not applied (a NaN spreads over the support only); a column whose zeros lie between
// non-zero taps (no disc has one) sends the whole workgroup down the tested path for every tap.
#include "common.hpp"

namespace dnmf {
namespace {

constexpr int HP_R = 8, HP_LX = 4, HP_TX = HP_R * HP_LX, HP_TC = 64, HP_THREADS = HP_LX * HP_TC;
constexpr int HP_MAX_N = 31;
constexpr int HP_TABLE = 32;                  // entries of the run tables (>= HP_MAX_N)
constexpr size_t HP_LDS_BUDGET = 64 * 1024;   // bytes of dynamic LDS a workgroup may ask for

struct HighPassArgs {
    const float *frames;
    const int *frame_ids;
    const float *taps;
    float *out;
    long ldf, ldo;
    int X, Y, Z, B, n;
    int Zt;       // slices interleaved in a tile row: Z, or 1 (one slice per workgroup)
    int cs;       // floats between two columns of the tile in a frame: Z / Zt
    int ncols;    // columns of the plane the tiles cover: Y Zt
    int ntc;      // tiles along c
    int rows, W;  // the staged tile: HP_TX + 2 h rows of HP_TC + 2 h Zt floats
    int plane;    // Y Z
};

__host__ __device__ inline size_t hp_lds_bytes(int rows, int W) {
    return sizeof(float) * ((size_t)rows * W + rows + W + 3 * HP_TABLE);
}

// BORDER_REFLECT of any index: reflection with period 2 N (fedcba|abcdefgh|hgfedcb, as often as it takes)
__device__ __forceinline__ int reflect(int p, int N) {
    int m = p % (2 * N);
    if (m < 0) m += 2 * N;
    return m < N ? m : 2 * N - 1 - m;
}

__global__ __launch_bounds__(HP_THREADS) void high_pass_kernel(HighPassArgs a) {
    extern __shared__ float smem[];
    float *tile = smem;
    int *rowoff = reinterpret_cast<int *>(tile + (size_t)a.rows * a.W);
    int *coloff = rowoff + a.rows;
    int *runlo = coloff + a.W, *runhi = runlo + HP_TABLE, *runhole = runhi + HP_TABLE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lx = tid / HP_TC, lc = tid - lx * HP_TC;
    const int n = a.n, h = n >> 1, W = a.W;
    const int tx = blockIdx.x / a.ntc, tc = blockIdx.x - tx * a.ntc;
    const int x0 = tx * HP_TX, c0 = tc * HP_TC, z0 = blockIdx.z;

    for (int r = tid; r < a.rows; r += HP_THREADS) rowoff[r] = reflect(x0 - h + r, a.X) * a.plane;
    for (int j = tid; j < W; j += HP_THREADS) {
        const int gc = c0 - h * a.Zt + j;
        int y = gc / a.Zt;
        if (y * a.Zt > gc) --y;                      // floor for the negative columns of the halo
        coloff[j] = reflect(y, a.Y) * a.Z + (gc - y * a.Zt) + z0;
    }
    // per tap column j: the first and the last non-zero tap, and whether a zero lies between them
    if (tid < HP_TABLE) {
        int lo = n, hi = -1, zeros = 0, hole = 0;
        if (tid < n)
            for (int i = 0; i < n; ++i) {
                if (a.taps[i * n + tid] != 0.0f) {
                    if (hi >= 0 && zeros) hole = 1;
                    if (hi < 0) lo = i;
                    hi = i, zeros = 0;
                } else {
                    ++zeros;
                }
            }
        runlo[tid] = lo, runhi[tid] = hi, runhole[tid] = hole;
    }
    __syncthreads();
    int anyhole = 0;
    for (int j = 0; j < n; ++j) anyhole |= runhole[j];
    const bool holes = __builtin_amdgcn_readfirstlane(anyhole) != 0;

    const int gc = c0 + lc;
    const bool live = gc < a.ncols;
    const int ocol = gc * a.cs + z0;
    const float *base = tile + (lx * HP_R) * W + lc;

    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const float *fr = a.frames + (long)(a.frame_ids ? a.frame_ids[b] : b) * a.ldf;
        __syncthreads();   // the tables are written; the last frame's reads are done
        for (int r = wave; r < a.rows; r += HP_THREADS / 64) {
            const float *src = fr + rowoff[r];
            float *dst = tile + r * W;
            for (int j = lane; j < W; j += 64) dst[j] = src[coloff[j]];
        }
        __syncthreads();

        float acc[HP_R];
#pragma unroll
        for (int r = 0; r < HP_R; ++r) acc[r] = 0.0f;
        for (int j = 0; j < n; ++j) {
            const int i0 = __builtin_amdgcn_readfirstlane(runlo[j]), i1 = __builtin_amdgcn_readfirstlane(runhi[j]);
            if (i0 > i1) continue;
            const float *col = base + j * a.Zt;
            // tw[r] = taps[k - r][j], the tap output r applies to tile row k; 0 outside the run
            float tw[HP_R];
#pragma unroll
            for (int r = 0; r < HP_R; ++r) tw[r] = 0.0f;
            for (int k = i0; k <= i1 + HP_R - 1; ++k) {
#pragma unroll
                for (int r = HP_R - 1; r > 0; --r) tw[r] = tw[r - 1];
                tw[0] = k <= i1 ? a.taps[k * n + j] : 0.0f;
                const float v = col[k * W];
                if (!holes && k >= i0 + HP_R - 1 && k <= i1) {
#pragma unroll
                    for (int r = 0; r < HP_R; ++r) acc[r] = fmaf(tw[r], v, acc[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < HP_R; ++r)
                        if (tw[r] != 0.0f) acc[r] = fmaf(tw[r], v, acc[r]);
                }
            }
        }
        if (live) {
            float *o = a.out + (long)b * a.ldo + ocol;
#pragma unroll
            for (int r = 0; r < HP_R; ++r) {
                const int x = x0 + lx * HP_R + r;
                if (x < a.X) o[(long)x * a.plane] = acc[r];
            }
        }
    }
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_high_pass_frames(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, const float *taps, int n,
                          float *out, long ldo, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(sz, DNMF_E_NULL, "dnmf_high_pass_frames: sz is NULL");
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "dnmf_high_pass_frames: volume %dx%dx%d", sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(B >= 1, DNMF_E_SHAPE, "dnmf_high_pass_frames: B=%d frames", B);
    DNMF_REQUIRE(n >= 1 && (n & 1), DNMF_E_SHAPE, "dnmf_high_pass_frames: n=%d taps a side (odd, >= 1)", n);
    DNMF_REQUIRE(n <= HP_MAX_N, DNMF_E_UNSUPPORTED, "dnmf_high_pass_frames: n=%d taps a side, at most %d (gSig <= 10)", n, HP_MAX_N);
    DNMF_REQUIRE(frames && taps && out, DNMF_E_NULL, "dnmf_high_pass_frames: NULL argument");
    const long P = (long)sz[0] * sz[1] * sz[2];
    DNMF_REQUIRE(P < (1L << 31), DNMF_E_UNSUPPORTED, "dnmf_high_pass_frames: %ld voxels (32-bit offsets)", P);
    DNMF_REQUIRE(ldf >= P && ldo >= P, DNMF_E_SHAPE, "dnmf_high_pass_frames: ldf=%ld ldo=%ld below a row of P=%ld", ldf, ldo, P);
    HighPassArgs a;
    a.frames = frames, a.frame_ids = frame_ids, a.taps = taps, a.out = out, a.ldf = ldf, a.ldo = ldo;
    a.X = sz[0], a.Y = sz[1], a.Z = sz[2], a.B = B, a.n = n;
    a.plane = a.Y * a.Z;
    const int h = n / 2;
    a.rows = HP_TX + 2 * h;
    // every slice in one tile while it fits, else a workgroup per slice
    const long Wall = HP_TC + 2L * h * a.Z;
    a.Zt = (Wall < (1L << 20) && hp_lds_bytes(a.rows, (int)Wall) <= HP_LDS_BUDGET) ? a.Z : 1;
    a.cs = a.Z / a.Zt;
    a.ncols = a.Y * a.Zt;
    a.W = HP_TC + 2 * h * a.Zt;
    a.ntc = (a.ncols + HP_TC - 1) / HP_TC;
    const long tiles = (long)((a.X + HP_TX - 1) / HP_TX) * a.ntc;
    const int slices = a.Zt == a.Z ? 1 : a.Z;
    DNMF_REQUIRE(tiles < (1L << 31) && slices <= 65535, DNMF_E_UNSUPPORTED, "dnmf_high_pass_frames: %ld tiles, %d slices", tiles, slices);
    const dim3 grid((unsigned)tiles, (unsigned)(B < 65535 ? B : 65535), (unsigned)slices);
    hipLaunchKernelGGL(high_pass_kernel, grid, dim3(HP_THREADS), hp_lds_bytes(a.rows, a.W), (hipStream_t)stream, a);
    return check_launch("dnmf_high_pass_frames");
}

}  // extern "C"
