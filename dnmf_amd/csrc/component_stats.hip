// K24: per-component statistics of a fitted model on the registered movie -- for every neuron k, on its box of n voxels, per
// frame the three sums of e_t = frames_t - sub_t + a C[k, t] (sum e, sum e^2, sum a e), from them the Pearson correlation of
// the footprint a with e_t and the raw trace, and the weighted mean image of e_t over the frames with its correlation with
// a.  include/dnmf_hip.h has the contract, tests/components_restatement.py the definition in float64.
//
// One pass over the boxes of the movie.  A workgroup of CS_THREADS lanes owns one neuron and a segment of frames; every
// lane keeps its voxels of the box (at most 16: a box holds at most 4096) in registers -- the offset inside a frame, the
// footprint value, and the float64 image sum.  Per frame a lane forms e on its voxels (the next frame's loads are already
// in flight), the three partial sums go down the wave by shuffles and across the four waves through LDS, both in a fixed
// order, with one barrier a frame (two buffers); the total of sum e says whether the box held a sample that is not finite,
// and only then does the frame's w e enter the image sums.  A segment's image sums go to the state; a second launch adds
// the segments of a neuron in their order (no floating-point atomics: the same input gives the same bits) and forms the
// per-frame and per-neuron figures.
#include "block_ops.hpp"
#include "boxes.hpp"

namespace dnmf {
namespace {

constexpr int CS_THREADS = 256, CS_WAVES = CS_THREADS / 64;
constexpr int CS_MIN_SEGMENT = 16;      // frames: below this the partial image sums cost more traffic than the frames
constexpr int CS_TARGET_BLOCKS = 2048;

struct ComponentPlan : SegmentPlan {
    int X, Y, Z, K, vmax, slots;
    long P;
    size_t vstride;                                              // doubles between the image sums of two (neuron, segment)s
    size_t off_w, off_img, off_pw, off_pimg, bytes;
};

// Everything the two entries agree on; validates what both take.  boxes is a host array.
int component_plan(const char *fn, const int *sz, const int *boxes, int K, int B, int segment, ComponentPlan &g) {
    DNMF_REQUIRE(sz && boxes, DNMF_E_NULL, "%s: sz or boxes is NULL", fn);
    DNMF_REQUIRE(sz[0] >= 1 && sz[1] >= 1 && sz[2] >= 1, DNMF_E_SHAPE, "%s: volume %dx%dx%d", fn, sz[0], sz[1], sz[2]);
    DNMF_REQUIRE(K >= 1 && B >= 1, DNMF_E_SHAPE, "%s: K=%d neurons, B=%d frames", fn, K, B);
    g.X = sz[0], g.Y = sz[1], g.Z = sz[2], g.K = K;
    g.P = (long)g.X * g.Y * g.Z;
    DNMF_REQUIRE(g.P < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld voxels (32-bit offsets)", fn, g.P);
    DNMF_REQUIRE(K <= (1 << 20), DNMF_E_UNSUPPORTED, "%s: K=%d neurons", fn, K);
    const int rb = check_boxes(fn, sz, boxes, K, BOX_MAX_VOXELS, DNMF_E_UNSUPPORTED, "at most ", &g.vmax);
    if (rb != DNMF_OK) return rb;
    const int per_lane = (g.vmax + CS_THREADS - 1) / CS_THREADS;
    g.slots = 1;
    while (g.slots < per_lane) g.slots *= 2;
    const int rc = segment_plan(fn, B, segment, K, CS_TARGET_BLOCKS, CS_MIN_SEGMENT, g);
    if (rc != DNMF_OK) return rc;
    g.vstride = align256((size_t)g.vmax * sizeof(double)) / sizeof(double);
    const size_t Ks = (size_t)K, cap = (size_t)g.cap;
    g.off_w = 0;
    g.off_img = g.off_w + align256(Ks * sizeof(double));
    g.off_pw = g.off_img + Ks * g.vstride * sizeof(double);
    g.off_pimg = g.off_pw + align256(Ks * cap * sizeof(double));
    g.bytes = g.off_pimg + Ks * cap * g.vstride * sizeof(double);
    return DNMF_OK;
}

struct ComponentArgs {
    const float *frames, *sub, *A, *C, *w;
    long ldf, lds, lda, ldc, ldw;
    const int *frame_ids, *boxes;
    int Y, Z, B, seglen;
    double *sums;          // (K, B, 3)
    double *part_img;      // (K, cap, vstride)
    double *part_w;        // (K, cap)
    size_t cap, vstride;
};

// The sums of three values over the workgroup behind one barrier, in every lane, in block_reduce's order (block_ops.hpp).  red:
// CS_WAVES x 3 doubles of LDS that no lane still reads.
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum(a), b = wave_sum(b), c = wave_sum(c);
    if (lane == 0) red[wave * 3] = a, red[wave * 3 + 1] = b, red[wave * 3 + 2] = c;
    __syncthreads();
    a = red[0], b = red[1], c = red[2];
#pragma unroll
    for (int v = 1; v < CS_WAVES; ++v) a += red[v * 3], b += red[v * 3 + 1], c += red[v * 3 + 2];
}

template <int SLOTS>
__global__ __launch_bounds__(CS_THREADS) void component_accumulate_kernel(ComponentArgs g) {
    __shared__ double red[2][CS_WAVES * 3];
    const int tid = threadIdx.x, k = blockIdx.x, seg = blockIdx.y;
    const int f0 = seg * g.seglen, f1 = min(g.B, f0 + g.seglen);
    const Box q = load_box(g.boxes + 6 * (long)k);
    const float *Ak = g.A + (long)k * g.lda;
    const float *Ck = g.C + (long)k * g.ldc, *wk = g.w + (long)k * g.ldw;

    int off[SLOTS];
    float a[SLOTS];
    double img[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int i = tid + s * CS_THREADS;
        off[s] = i < q.n ? box_offset(q, i, g.Y, g.Z) : -1;
        a[s] = off[s] >= 0 ? Ak[off[s]] : 0.0f;
        img[s] = 0.0;
    }
    auto row = [&](int j) { return g.frames + (long)(g.frame_ids ? g.frame_ids[j] : j) * g.ldf; };
    auto subrow = [&](int j) { return g.sub ? g.sub + (long)j * g.lds : nullptr; };

    float vf[SLOTS], vs[SLOTS];
    auto fetch = [&](int j) {
        const float *fr = row(j), *sb = subrow(j);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            vf[s] = off[s] >= 0 ? fr[off[s]] : 0.0f;
            vs[s] = (sb && off[s] >= 0) ? sb[off[s]] : 0.0f;
        }
    };
    if (f0 < f1) fetch(f0);
    double wacc = 0.0;
    for (int j = f0; j < f1; ++j) {
        const double c = (double)Ck[j], wj = (double)wk[j];
        double e[SLOTS], se = 0.0, see = 0.0, sae = 0.0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            // the residual with the neuron's own contribution put back; both steps exact but the last addition
            e[s] = off[s] >= 0 ? ((double)vf[s] - (double)vs[s]) + (double)a[s] * c : 0.0;
            se += e[s];
            see = fma(e[s], e[s], see);
            sae = fma((double)a[s], e[s], sae);
        }
        if (j + 1 < f1) fetch(j + 1);
        block_sum3(se, see, sae, red[(j - f0) & 1]);
        // a sample that is not finite makes sum e not finite (finite fp32 terms cannot overflow a float64 sum)
        const bool valid = __builtin_isfinite(se);
        if (valid && wj != 0.0) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) img[s] = fma(wj, e[s], img[s]);
            wacc += wj;
        }
        if (tid == 0) {
            const double nan = __builtin_nan("");
            double *out = g.sums + ((size_t)k * g.B + j) * 3;
            out[0] = valid ? se : nan, out[1] = valid ? see : nan, out[2] = valid ? sae : nan;
        }
    }
    double *pimg = g.part_img + ((size_t)k * g.cap + seg) * g.vstride;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
        if (off[s] >= 0) pimg[tid + s * CS_THREADS] = img[s];
    if (tid == 0) g.part_w[(size_t)k * g.cap + seg] = wacc;
}

struct FinishArgs {
    const float *A;
    long lda;
    const int *boxes;
    int Y, Z, B, nseg, first, finish;
    const double *sums, *part_img, *part_w;
    size_t cap, vstride;
    double *wsum, *img;                                  // the state: (K), (K, vstride)
    double *foot, *frame_corr, *raw, *image, *r_values;  // (K, 3), (K, B), (K, B), (K, ldi), (K)
    long ldi;
};

// Pearson of two samples from their sums; NaN where a variance is not positive
__device__ __forceinline__ double pearson(double n, double sa, double saa, double sb, double sbb, double sab) {
    const double va = n * saa - sa * sa, vb = n * sbb - sb * sb;
    if (!(va > 0.0) || !(vb > 0.0)) return __builtin_nan("");
    return (n * sab - sa * sb) / sqrt(va * vb);
}

// One workgroup a neuron: state = (first ? 0 : state) + the segments in their order; foot, frame_corr and raw of this call's
// frames; with finish the mean image and its correlation with the footprint.
__global__ __launch_bounds__(CS_THREADS) void component_finish_kernel(FinishArgs g) {
    __shared__ double red[2][CS_WAVES * 3];
    const int tid = threadIdx.x, k = blockIdx.x;
    const Box q = load_box(g.boxes + 6 * (long)k);
    const float *Ak = g.A + (long)k * g.lda;
    const double nan = __builtin_nan("");

    double wtot = g.first ? 0.0 : g.wsum[k];
    for (int s = 0; s < g.nseg; ++s) wtot += g.part_w[(size_t)k * g.cap + s];

    double *img = g.img + (size_t)k * g.vstride;
    double sa = 0.0, saa = 0.0, unused = 0.0;
    double sm = 0.0, smm = 0.0, sam = 0.0;
    for (int i = tid; i < q.n; i += CS_THREADS) {
        double acc = g.first ? 0.0 : img[i];
        const double *p = g.part_img + (size_t)k * g.cap * g.vstride + i;
        for (int s = 0; s < g.nseg; ++s) acc += p[(size_t)s * g.vstride];
        img[i] = acc;
        const double av = (double)Ak[box_offset(q, i, g.Y, g.Z)];
        sa += av;
        saa = fma(av, av, saa);
        if (g.finish) {
            const double m = acc / wtot;     // 0 / 0 = NaN without a weight
            g.image[(long)k * g.ldi + i] = m;
            sm += m;
            smm = fma(m, m, smm);
            sam = fma(av, m, sam);
        }
    }
    if (g.finish)
        for (long i = q.n + tid; i < g.ldi; i += CS_THREADS) g.image[(long)k * g.ldi + i] = nan;
    block_sum3(sa, saa, unused, red[0]);
    const double n = (double)q.n;
    if (g.finish) {
        block_sum3(sm, smm, sam, red[1]);
        if (tid == 0) g.r_values[k] = wtot > 0.0 ? pearson(n, sa, saa, sm, smm, sam) : nan;
    }
    // every lane has read the old weight sum before the second reduction's barrier, or holds it in wtot already
    __syncthreads();
    if (tid == 0) {
        g.wsum[k] = wtot;
        g.foot[3 * (long)k] = n, g.foot[3 * (long)k + 1] = sa, g.foot[3 * (long)k + 2] = saa;
    }
    const double va = n * saa - sa * sa;
    for (int j = tid; j < g.B; j += CS_THREADS) {
        const double *s = g.sums + ((size_t)k * g.B + j) * 3;
        const double se = s[0], see = s[1], sae = s[2];
        const bool ok = __builtin_isfinite(se);
        g.frame_corr[(size_t)k * g.B + j] = ok ? pearson(n, sa, saa, se, see, sae) : nan;
        g.raw[(size_t)k * g.B + j] = (ok && va > 0.0) ? (n * sae - sa * se) / va : nan;
    }
}

template <int SLOTS>
void launch_accumulate(const ComponentPlan &g, const ComponentArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((component_accumulate_kernel<SLOTS>), dim3((unsigned)g.K, (unsigned)g.nseg), dim3(CS_THREADS), 0, st, a);
}

}  // namespace
}  // namespace dnmf

extern "C" {

size_t dnmf_component_stats_workspace(const int *sz, const int *boxes, int K, int B, int segment) {
    dnmf::ComponentPlan g;
    if (dnmf::component_plan("dnmf_component_stats_workspace", sz, boxes, K, B, segment, g) != DNMF_OK) return 0;
    return g.bytes;
}

int dnmf_component_stats(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const int *sz, int B,
                         const float *A, long lda, const int *boxes, const int *boxes_dev, int K, const float *C, long ldc,
                         const float *w, long ldw, int first, int finish, int segment, void *state, size_t state_bytes,
                         double *sums, double *foot, double *frame_corr, double *raw, double *image, long ldi, double *r_values,
                         dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_component_stats";
    DNMF_REQUIRE(frames && sz && A && boxes && boxes_dev && C && w && state, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(sums && foot && frame_corr && raw, DNMF_E_NULL, "%s: a per-frame output is NULL", fn);
    DNMF_REQUIRE((image && r_values) || !finish, DNMF_E_NULL, "%s: image or r_values is NULL with finish", fn);
    ComponentPlan g;
    const int rc = component_plan(fn, sz, boxes, K, B, segment, g);
    if (rc != DNMF_OK) return rc;
    DNMF_REQUIRE(ldf >= g.P && (!sub || lds >= g.P) && lda >= g.P, DNMF_E_SHAPE, "%s: ldf=%ld lds=%ld lda=%ld below a row of P=%ld", fn,
                 ldf, lds, lda, g.P);
    DNMF_REQUIRE(ldc >= B && ldw >= B, DNMF_E_SHAPE, "%s: ldc=%ld ldw=%ld below a row of B=%d", fn, ldc, ldw, B);
    DNMF_REQUIRE(!finish || ldi >= g.vmax, DNMF_E_SHAPE, "%s: ldi=%ld below the largest box of %d voxels", fn, ldi, g.vmax);
    DNMF_REQUIRE(state_bytes >= g.bytes, DNMF_E_WORKSPACE, "%s: state of %zu bytes, need %zu", fn, state_bytes, g.bytes);
    DNMF_REQUIRE(((size_t)state & 7) == 0, DNMF_E_WORKSPACE, "%s: state must be 8-byte aligned", fn);
    char *ws = static_cast<char *>(state);
    ComponentArgs a;
    a.frames = frames, a.sub = sub, a.A = A, a.C = C, a.w = w;
    a.ldf = ldf, a.lds = lds, a.lda = lda, a.ldc = ldc, a.ldw = ldw;
    a.frame_ids = frame_ids, a.boxes = boxes_dev;
    a.Y = g.Y, a.Z = g.Z, a.B = B, a.seglen = g.seglen;
    a.sums = sums;
    a.part_img = reinterpret_cast<double *>(ws + g.off_pimg), a.part_w = reinterpret_cast<double *>(ws + g.off_pw);
    a.cap = g.cap, a.vstride = g.vstride;
    const hipStream_t st = (hipStream_t)stream;
    switch (g.slots) {
        case 1: launch_accumulate<1>(g, a, st); break;
        case 2: launch_accumulate<2>(g, a, st); break;
        case 4: launch_accumulate<4>(g, a, st); break;
        case 8: launch_accumulate<8>(g, a, st); break;
        default: launch_accumulate<16>(g, a, st); break;
    }
    FinishArgs f;
    f.A = A, f.lda = lda, f.boxes = boxes_dev;
    f.Y = g.Y, f.Z = g.Z, f.B = B, f.nseg = g.nseg, f.first = first != 0, f.finish = finish != 0;
    f.sums = sums, f.part_img = a.part_img, f.part_w = a.part_w;
    f.cap = g.cap, f.vstride = g.vstride;
    f.wsum = reinterpret_cast<double *>(ws + g.off_w), f.img = reinterpret_cast<double *>(ws + g.off_img);
    f.foot = foot, f.frame_corr = frame_corr, f.raw = raw, f.image = image, f.r_values = r_values, f.ldi = ldi;
    hipLaunchKernelGGL(component_finish_kernel, dim3((unsigned)g.K), dim3(CS_THREADS), 0, st, f);
    return check_launch(fn);
}

}  // extern "C"
