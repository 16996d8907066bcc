// K10: exact nearest-point search for an arbitrary point cloud per frame (ExponentialFP.image_iwarp on any flow,
// Demix/dNMF.py:95-103: scipy's NearestNDInterpolator, a cKDTree query in float64).
//
// Contract: for every frame f and query q, the point i of the smallest (d2, i) in lexicographic order, d2 the float64
// squared distance ((qx - px)^2 + (qy - py)^2) + (qz - pz)^2 of the coordinates as stored (fp32 points are widened
// exactly).  Exact ties go to the lowest index, the rule of K7.  Nothing depends on the order of the atomics below.
//
// Per chunk of frames:
//   1. np_bbox_kernel      the frame's bounding box of the finite coordinates (order-preserving uint64 atomics);
//   2. np_grid_kernel      a uniform cell grid over the box, about one point per cell, at most N cells; an axis of
//                          zero extent gets one cell;
//   3. np_count_kernel     each point's cell and its rank inside the cell (an atomic counter per cell);
//   4. np_scan_*           exclusive scan of the counts -> the start of every cell (counts of N + 1 cells per frame,
//                          tiles of 1024, a scan of the tile sums, the tiles again with their offsets);
//   5. np_scatter_kernel   one record {x, y, z, index} per point in cell order (16 B for fp32, 32 B for fp64);
//   6. np_query_kernel     one thread per query: Chebyshev shells of cells around the query's cell, nearest first,
//                          until the distance to every unsearched cell exceeds the best d2 (see np_query_kernel).
// Every cell coordinate is clamped to its axis, so non-finite or far-away coordinates cannot leave the arrays; they
// only cost time.
#include "common.hpp"

namespace dnmf {
namespace {

constexpr int NP_TILE = 1024;     // counts per scan tile (256 threads x 4)
constexpr long NP_HEAD = 256;     // per-frame header: Grid (128 B) + the box (6 uint64)

struct Grid {
    double lo[3];     // box corner
    double inv[3];    // cells per unit length (0 on an axis of one cell)
    double h[3];      // cell size (extent / cells)
    double s[3];      // slack of every cell face (rounding of the cell assignment), > 0
    int n[3];         // cells per axis
    int pad;
};
static_assert(sizeof(Grid) <= 128, "Grid must fit its header slot");

template <typename T> struct Rec;
template <> struct Rec<float> { float x, y, z; int i; };
template <> struct Rec<double> { double x, y, z; long i; };

// double <-> uint64 with the order of the doubles
__device__ __forceinline__ unsigned long long np_ord(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double np_unord(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// The per-frame layout of the workspace: header, records (32 B per point), (cell, rank) per point, N + 1 counts, tile sums.
struct Layout {
    long rec, pc, cnt, tiles, stride;
};
__host__ __device__ inline long np_tiles(int N) { return ((long)N + 1 + NP_TILE - 1) / NP_TILE; }
__host__ __device__ inline Layout np_layout(int N) {
    Layout l;
    l.rec = NP_HEAD;
    l.pc = l.rec + 32L * N;
    l.cnt = l.pc + 8L * N;
    l.tiles = l.cnt + 4L * (N + 1);
    const long end = l.tiles + 4L * np_tiles(N);
    l.stride = (end + 255) & ~255L;
    return l;
}

// Cell of coordinate v along axis d (clamped: NaN -> 0, +-inf and far outliers -> the end cells).
__device__ __forceinline__ int np_cell(const Grid &g, int d, double v) {
    const double t = (v - g.lo[d]) * g.inv[d];
    return (int)fmin(fmax(t, 0.0), (double)(g.n[d] - 1));
}

// Squared distance from q to the box [a, b] (0 inside); a NaN face gives a NaN, which never prunes.
__device__ __forceinline__ double np_gap2(double q, double a, double b) {
    const double g = fmax(fmax(a - q, q - b), 0.0);
    return g * g;
}

__global__ void np_init_kernel(char *ws, long stride, int nf) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    unsigned long long *box = reinterpret_cast<unsigned long long *>(ws + f * stride + 128);
    for (int d = 0; d < 3; ++d) box[d] = ~0ull, box[3 + d] = 0ull;
}

// zero the N + 1 counts of every frame of the chunk: grid (ceil((N + 1) / 256), nf)
__global__ void np_zero_kernel(char *ws, long stride, long cnt_off, int L) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < L) reinterpret_cast<int *>(ws + blockIdx.y * stride + cnt_off)[c] = 0;
}

// 1.  grid (gx, nf), 256 threads: box of the finite coordinates
template <typename T>
__global__ __launch_bounds__(256) void np_bbox_kernel(const T *points, long ldp, int N, int f0, char *ws, long stride) {
    const int f = blockIdx.y;
    const T *p = points + (long)(f0 + f) * ldp;
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()};
    double hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        for (int d = 0; d < 3; ++d) {
            const double v = (double)p[3 * i + d];
            if (__builtin_isfinite(v)) lo[d] = fmin(lo[d], v), hi[d] = fmax(hi[d], v);
        }
    }
    __shared__ double red[4][6];
    for (int d = 0; d < 3; ++d) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], o));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], o));
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int d = 0; d < 3; ++d) red[w][d] = lo[d], red[w][3 + d] = hi[d];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        double v = red[0][k];
        for (int j = 1; j < 4; ++j) v = k < 3 ? fmin(v, red[j][k]) : fmax(v, red[j][k]);
        unsigned long long *box = reinterpret_cast<unsigned long long *>(ws + f * stride + 128);
        if (k < 3) {
            if (v != __builtin_inf()) atomicMin(box + k, np_ord(v));
        } else {
            if (v != -__builtin_inf()) atomicMax(box + k, np_ord(v));
        }
    }
}

// 2.  one thread per frame: the cell grid.  Cells of size h = (volume of the active axes / N)^(1/k) (k axes of non-zero
// extent), floor(extent / h) cells per active axis, at least 1; the product stays <= N.
__global__ void np_grid_kernel(char *ws, long stride, int nf, int N) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const unsigned long long *box = reinterpret_cast<const unsigned long long *>(ws + f * stride + 128);
    Grid g;
    double lo[3], ext[3], vol = 1.0;
    int k = 0;
    for (int d = 0; d < 3; ++d) {
        double a = np_unord(box[d]), b = np_unord(box[3 + d]);
        if (!(a <= b)) a = b = 0.0;                        // no finite coordinate on this axis
        lo[d] = a, ext[d] = b - a;
        if (ext[d] > 0.0 && ext[d] < __builtin_inf()) vol *= ext[d], ++k;
        g.s[d] = 1e-12 * (fabs(a) + fabs(b)) + 1e-300;
    }
    const double hc = k ? pow(vol / (double)N, 1.0 / k) : 0.0;
    double cells = 1.0;   // a double: three axes of up to N cells each would overflow a long
    for (int d = 0; d < 3; ++d) {
        int n = 1;
        if (ext[d] > 0.0 && ext[d] < __builtin_inf() && hc > 0.0) n = (int)fmin(fmax(floor(ext[d] / hc), 1.0), (double)N);
        g.n[d] = n;
        cells *= n;
    }
    while (cells > N) {                                    // rounding of pow: halve the longest axis until it fits
        int m = 0;
        for (int d = 1; d < 3; ++d) m = g.n[d] > g.n[m] ? d : m;
        cells = cells / g.n[m] * (double)((g.n[m] + 1) / 2);
        g.n[m] = (g.n[m] + 1) / 2;
    }
    for (int d = 0; d < 3; ++d) {
        g.lo[d] = lo[d];
        g.inv[d] = g.n[d] > 1 ? (double)g.n[d] / ext[d] : 0.0;
        g.h[d] = g.n[d] > 1 ? ext[d] / (double)g.n[d] : ext[d];
        g.s[d] += 1e-12 * ext[d];
    }
    g.pad = 0;
    *reinterpret_cast<Grid *>(ws + f * stride) = g;
}

// 3.  grid (ceil(N / 256), nf): cell and rank inside the cell of every point
template <typename T>
__global__ __launch_bounds__(256) void np_count_kernel(const T *points, long ldp, int N, int f0, char *ws, long stride, Layout l) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    char *fw = ws + blockIdx.y * stride;
    const Grid g = *reinterpret_cast<const Grid *>(fw);
    const T *p = points + (long)(f0 + blockIdx.y) * ldp + 3L * i;
    const int c = (np_cell(g, 0, (double)p[0]) * g.n[1] + np_cell(g, 1, (double)p[1])) * g.n[2] + np_cell(g, 2, (double)p[2]);
    const int r = atomicAdd(reinterpret_cast<int *>(fw + l.cnt) + c, 1);
    reinterpret_cast<int2 *>(fw + l.pc)[i] = make_int2(c, r);
}

// block-wide inclusive scan of one value per thread (256 threads); returns the block's total through *total
__device__ __forceinline__ int np_block_scan(int v, int *total) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == 63) part[w] = v;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < w; ++j) before += part[j];
    *total = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    return v + before;
}

// 4a.  grid (tiles, nf): sum of each tile of counts
__global__ __launch_bounds__(256) void np_scan_tiles_kernel(char *ws, long stride, Layout l, int L) {
    char *fw = ws + blockIdx.y * stride;
    const int *cnt = reinterpret_cast<const int *>(fw + l.cnt);
    const long base = (long)blockIdx.x * NP_TILE + 4L * threadIdx.x;
    int v = 0;
    for (int k = 0; k < 4; ++k) v += base + k < L ? cnt[base + k] : 0;
    int total;
    np_block_scan(v, &total);
    if (threadIdx.x == 0) reinterpret_cast<int *>(fw + l.tiles)[blockIdx.x] = total;
}

// 4b.  grid (nf): exclusive scan of the tile sums of a frame, in place
__global__ __launch_bounds__(256) void np_scan_tops_kernel(char *ws, long stride, Layout l, int nt) {
    int *t = reinterpret_cast<int *>(ws + blockIdx.x * stride + l.tiles);
    int carry = 0;
    for (int b = 0; b < nt; b += 256) {
        const int j = b + threadIdx.x;
        const int v = j < nt ? t[j] : 0;
        int total;
        const int inc = np_block_scan(v, &total);
        if (j < nt) t[j] = carry + inc - v;
        carry += total;
    }
}

// 4c.  grid (tiles, nf): counts -> exclusive starts, in place
__global__ __launch_bounds__(256) void np_scan_apply_kernel(char *ws, long stride, Layout l, int L) {
    char *fw = ws + blockIdx.y * stride;
    int *cnt = reinterpret_cast<int *>(fw + l.cnt);
    const long base = (long)blockIdx.x * NP_TILE + 4L * threadIdx.x;
    int v[4], s = 0;
    for (int k = 0; k < 4; ++k) v[k] = base + k < L ? cnt[base + k] : 0, s += v[k];
    int total;
    int run = np_block_scan(s, &total) - s + reinterpret_cast<const int *>(fw + l.tiles)[blockIdx.x];
    for (int k = 0; k < 4; ++k) {
        if (base + k < L) cnt[base + k] = run;
        run += v[k];
    }
}

// 5.  grid (ceil(N / 256), nf): the records in cell order
template <typename T>
__global__ __launch_bounds__(256) void np_scatter_kernel(const T *points, long ldp, int N, int f0, char *ws, long stride, Layout l) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    char *fw = ws + blockIdx.y * stride;
    const int2 cr = reinterpret_cast<const int2 *>(fw + l.pc)[i];
    const int pos = reinterpret_cast<const int *>(fw + l.cnt)[cr.x] + cr.y;
    const T *p = points + (long)(f0 + blockIdx.y) * ldp + 3L * i;
    Rec<T> r;
    r.x = p[0], r.y = p[1], r.z = p[2], r.i = i;
    reinterpret_cast<Rec<T> *>(fw + l.rec)[pos] = r;
}

// lexicographic (d2, index) update; a NaN distance never wins
__device__ __forceinline__ void np_take(double d2, int i, double &best, int &bi) {
    if (d2 < best || (d2 == best && i < bi)) best = d2, bi = i;
}

// 6.  grid (ceil(Q / 256), nf): one thread per query.
//
// Cell c along axis d holds points whose coordinate lies in [lo + c h - s, lo + (c + 1) h + s]: the assignment
// t = (v - lo) * inv rounds twice (relative 2^-53 each) and lo + c h once, all far inside the slack s = 1e-12 (|lo| +
// |hi| + extent).  After the shells 0..r, the points not yet seen lie in the slabs beyond the searched box of cells: for
// each axis and side where cells remain, the frame's box with that axis cut to the slab.  The search stops when the
// squared distance to the nearest such slab, shrunk by 1e-12 for its own rounding, is above the best d2: every unseen
// point then has a larger computed d2, so neither the distance nor the index rule can prefer it.  The same test skips
// single cells of a shell.  The shells end at the edge of the grid in every direction at the latest.
template <typename T>
__global__ __launch_bounds__(256) void np_query_kernel(const double *queries, long ldq, int Q, int f0, const char *ws, long stride,
                                                       Layout l, const float *values, long ldv, int *index_out, long ldi,
                                                       float *value_out, long ldo) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int f = blockIdx.y;
    const char *fw = ws + f * stride;
    const Grid g = *reinterpret_cast<const Grid *>(fw);
    const int *start = reinterpret_cast<const int *>(fw + l.cnt);
    const Rec<T> *rec = reinterpret_cast<const Rec<T> *>(fw + l.rec);
    const double *qp = queries + (long)(f0 + f) * ldq + 3L * q;
    const double qv[3] = {qp[0], qp[1], qp[2]};
    int cq[3], rmax = 0;
    double blo[3], bhi[3], bg[3];
    for (int d = 0; d < 3; ++d) {
        cq[d] = np_cell(g, d, qv[d]);
        const int e = cq[d] > g.n[d] - 1 - cq[d] ? cq[d] : g.n[d] - 1 - cq[d];
        rmax = e > rmax ? e : rmax;
        blo[d] = g.lo[d] - g.s[d];
        bhi[d] = g.lo[d] + g.n[d] * g.h[d] + g.s[d];
        bg[d] = np_gap2(qv[d], blo[d], bhi[d]);
    }
    double best = __builtin_inf();
    int bi = 0x7fffffff;
    for (int r = 0;; ++r) {
        const int x0 = cq[0] - r > 0 ? cq[0] - r : 0, x1 = cq[0] + r < g.n[0] - 1 ? cq[0] + r : g.n[0] - 1;
        const int y0 = cq[1] - r > 0 ? cq[1] - r : 0, y1 = cq[1] + r < g.n[1] - 1 ? cq[1] + r : g.n[1] - 1;
        const int z0 = cq[2] - r > 0 ? cq[2] - r : 0, z1 = cq[2] + r < g.n[2] - 1 ? cq[2] + r : g.n[2] - 1;
        for (int cx = x0; cx <= x1; ++cx) {
            const double gx = np_gap2(qv[0], g.lo[0] + cx * g.h[0] - g.s[0], g.lo[0] + (cx + 1) * g.h[0] + g.s[0]);
            for (int cy = y0; cy <= y1; ++cy) {
                const double gxy = gx + np_gap2(qv[1], g.lo[1] + cy * g.h[1] - g.s[1], g.lo[1] + (cy + 1) * g.h[1] + g.s[1]);
                const bool rim = cx == cq[0] - r || cx == cq[0] + r || cy == cq[1] - r || cy == cq[1] + r;
                // on the rim of x / y every z of the range; inside it (r >= 1) only the two z faces of the shell
                for (int cz = rim ? z0 : cq[2] - r; cz <= (rim ? z1 : cq[2] + r); cz += rim ? 1 : 2 * r) {
                    if (cz < 0 || cz >= g.n[2]) continue;
                    const double b2 = gxy + np_gap2(qv[2], g.lo[2] + cz * g.h[2] - g.s[2], g.lo[2] + (cz + 1) * g.h[2] + g.s[2]);
                    if (b2 * (1.0 - 1e-12) > best) continue;
                    const int c = (cx * g.n[1] + cy) * g.n[2] + cz;
                    const int e = start[c + 1];
                    for (int k = start[c]; k < e; ++k) {
                        const Rec<T> p = rec[k];
                        const double dx = qv[0] - (double)p.x, dy = qv[1] - (double)p.y, dz = qv[2] - (double)p.z;
                        np_take(dx * dx + dy * dy + dz * dz, (int)p.i, best, bi);
                    }
                }
            }
        }
        if (r >= rmax) break;
        // distance to the unsearched slabs
        double lb = __builtin_inf();
        for (int d = 0; d < 3; ++d) {
            const double rest = bg[0] + bg[1] + bg[2] - bg[d];
            if (cq[d] + r + 1 <= g.n[d] - 1)
                lb = fmin(lb, rest + np_gap2(qv[d], g.lo[d] + (cq[d] + r + 1) * g.h[d] - g.s[d], bhi[d]));
            if (cq[d] - r - 1 >= 0)
                lb = fmin(lb, rest + np_gap2(qv[d], blo[d], g.lo[d] + (cq[d] - r) * g.h[d] + g.s[d]));
        }
        if (lb * (1.0 - 1e-12) > best) break;
    }
    if (bi == 0x7fffffff) bi = 0;          // only when every distance is NaN (non-finite input): stay inside the rows
    index_out[(long)(f0 + f) * ldi + q] = bi;
    if (value_out) value_out[(long)(f0 + f) * ldo + q] = values[(long)(f0 + f) * ldv + bi];
}

int np_chunk(int N, int B) {
    const long s = np_layout(N).stride;
    long c = (512L << 20) / s;
    if (c > 65535) c = 65535;
    if (c < 1) c = 1;
    if (c > B) c = B;
    return (int)c;
}

template <typename T>
void np_run(const T *points, long ldp, int N, const double *queries, long ldq, int Q, int B, const float *values, long ldv,
            int *index_out, long ldi, float *value_out, long ldo, char *ws, int Bc, hipStream_t st) {
    // the chunk's frames (at most Bc) share one launch of every step
    const Layout l = np_layout(N);
    const int L = N + 1;
    const unsigned nt = (unsigned)np_tiles(N);
    const unsigned gN = (unsigned)((N + 255) / 256), gL = (unsigned)((L + 255) / 256), gQ = (unsigned)((Q + 255) / 256);
    for (int f0 = 0; f0 < B; f0 += Bc) {
        const int nf = B - f0 < Bc ? B - f0 : Bc;
        const unsigned gf = (unsigned)((nf + 63) / 64);
        const unsigned gb = gN < 64 ? gN : 64;
        hipLaunchKernelGGL(np_init_kernel, dim3(gf), dim3(64), 0, st, ws, l.stride, nf);
        hipLaunchKernelGGL(np_zero_kernel, dim3(gL, (unsigned)nf), dim3(256), 0, st, ws, l.stride, l.cnt, L);
        hipLaunchKernelGGL(np_bbox_kernel<T>, dim3(gb, (unsigned)nf), dim3(256), 0, st, points, ldp, N, f0, ws, l.stride);
        hipLaunchKernelGGL(np_grid_kernel, dim3(gf), dim3(64), 0, st, ws, l.stride, nf, N);
        hipLaunchKernelGGL(np_count_kernel<T>, dim3(gN, (unsigned)nf), dim3(256), 0, st, points, ldp, N, f0, ws, l.stride, l);
        hipLaunchKernelGGL(np_scan_tiles_kernel, dim3(nt, (unsigned)nf), dim3(256), 0, st, ws, l.stride, l, L);
        hipLaunchKernelGGL(np_scan_tops_kernel, dim3((unsigned)nf), dim3(256), 0, st, ws, l.stride, l, (int)nt);
        hipLaunchKernelGGL(np_scan_apply_kernel, dim3(nt, (unsigned)nf), dim3(256), 0, st, ws, l.stride, l, L);
        hipLaunchKernelGGL(np_scatter_kernel<T>, dim3(gN, (unsigned)nf), dim3(256), 0, st, points, ldp, N, f0, ws, l.stride, l);
        hipLaunchKernelGGL(np_query_kernel<T>, dim3(gQ, (unsigned)nf), dim3(256), 0, st, queries, ldq, Q, f0, ws, l.stride, l,
                           values, ldv, index_out, ldi, value_out, ldo);
    }
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_nearest_points_workspace(int N, int B) {
    using namespace dnmf;
    if (N <= 0 || B <= 0) return 0;
    return (size_t)np_chunk(N, B) * (size_t)np_layout(N).stride;
}

int dnmf_nearest_points(const void *points, int points_f64, long ldp, int N, const double *queries, long ldq, int Q, int B,
                        const float *values, long ldv, int *index_out, long ldi, float *value_out, long ldo, void *workspace,
                        size_t workspace_bytes, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(points && queries && index_out && workspace, DNMF_E_NULL, "dnmf_nearest_points: NULL argument");
    DNMF_REQUIRE((values == nullptr) == (value_out == nullptr), DNMF_E_NULL,
                 "dnmf_nearest_points: values and value_out go together");
    DNMF_REQUIRE(N > 0 && Q >= 0 && B >= 0, DNMF_E_SHAPE, "dnmf_nearest_points: N=%d Q=%d B=%d", N, Q, B);
    DNMF_REQUIRE(N < (1 << 30), DNMF_E_UNSUPPORTED, "dnmf_nearest_points: N=%d >= 2^30 points", N);
    DNMF_REQUIRE(ldp >= 3L * N && (ldq == 0 || ldq >= 3L * Q) && ldi >= Q && (!values || (ldv >= N && ldo >= Q)), DNMF_E_SHAPE,
                 "dnmf_nearest_points: strides ldp=%ld ldq=%ld ldv=%ld ldi=%ld ldo=%ld below a row (N=%d Q=%d)", ldp, ldq, ldv,
                 ldi, ldo, N, Q);
    if (B == 0 || Q == 0) return DNMF_OK;
    const size_t one = dnmf_nearest_points_workspace(N, 1);
    DNMF_REQUIRE(workspace_bytes >= one, DNMF_E_WORKSPACE, "dnmf_nearest_points: workspace %zu < %zu bytes (one frame)",
                 workspace_bytes, one);
    DNMF_REQUIRE(((size_t)workspace & 255) == 0, DNMF_E_WORKSPACE, "dnmf_nearest_points: workspace not 256-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    // frames per chunk: what the workspace holds, at most the 512 MiB chunk of dnmf_nearest_points_workspace(N, B)
    const size_t fit = workspace_bytes / one;
    const int Bc = fit < (size_t)np_chunk(N, B) ? (int)fit : np_chunk(N, B);
    if (points_f64)
        np_run(static_cast<const double *>(points), ldp, N, queries, ldq, Q, B, values, ldv, index_out, ldi, value_out, ldo, ws, Bc, st);
    else
        np_run(static_cast<const float *>(points), ldp, N, queries, ldq, Q, B, values, ldv, index_out, ldi, value_out, ldo, ws, Bc, st);
    return check_launch("dnmf_nearest_points");
}

}  // extern "C"
