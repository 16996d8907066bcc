// K25: histogram_match -- the affine map that carries the quantiles of a moving trace onto those of a reference trace.
// include/dnmf_hip.h has the contract, tests/histmatch_restatement.py the definition in float64 (H1 .. H5 below are its sections).
//
// One launch, one workgroup per row, everything in float64.
//   1  H1 / H2 for a: the row's samples go to LDS as 64-bit keys, every sample that is not finite as NANKEY; block_sort_keys
//      (block_ops.hpp: a bitonic network in LDS) sorts them, the valid ones first; quantile j then is two reads at the integer index
//      j (na - 1) / (nbins - 1) and one interpolation, into the table qa in LDS.  The same key buffer serves b, giving qb.
//   2  H3 / H5: lane i adds the bins i, i + THREADS, .. in that order, block_reduce (block_ops.hpp) adds the lanes in a fixed tree:
//      the means, then the centred and the raw second moments in one pass, the residuals of the two boundary solutions when the
//      non-negative fit needs them, the residual of the solution taken.  Every lane holds every sum, so the branches are uniform.
//   3  H4: the row of a is read again (L2), out_t = a_t beta0 + beta1 is rounded once to fp32 and stored.
// No floating-point atomics, no workspace: the same input gives the same bits.
// LDS: 8 sort_size(max(Ta, Tb)) bytes of keys and 16 nbins bytes of tables, sized per call -- 9.6 KiB for 1000 frames and 100 bins,
// 144 KiB at the limits (16 384 frames: 128 KiB; 1024 bins: 16 KiB) of the CU's 160.  Rows of up to HM_SMALL_ELEMS samples run in
// workgroups of 256 lanes: a step of the network is then at most two exchanges a lane, a barrier joins 4 waves instead of 16 and up
// to 8 rows share a CU; longer rows take 1024 lanes (8 exchanges a lane and step at the limit).
#include <cmath>
#include <cstdint>

#include "block_ops.hpp"

namespace dnmf {
namespace {

constexpr int HM_MAX_ELEMS = 16384;     // samples of a row: a power of two whose keys (128 KiB) fit LDS beside both tables
constexpr int HM_MAX_BINS = 1024;
constexpr int HM_MAX_ROWS = 18432;      // what K20 and K21 accept
constexpr int HM_SMALL_ELEMS = 1024;    // rows up to here: HM_SMALL_THREADS lanes
constexpr int HM_SMALL_THREADS = 256, HM_THREADS = 1024;

struct HmArgs {
    const float *a, *b;
    long lda, ldb, ldo;   // ldb = 0: one row of b for every row of a
    int Ta, Tb, nbins, nonneg, P;   // P = sort_size(max(Ta, Tb))
    float *out;
    double *beta, *distance, *qa, *qb;
    int *info;
};

// H1 and H2 of one row: its T samples -> sorted keys in key[0 .. sort_size(T)) and the nbins quantiles in q (NaN without a valid
// sample); returns the number of valid samples.  Ends with a barrier: q is visible and the keys may be overwritten.
template <int THREADS>
__device__ __forceinline__ int sorted_quantiles(const float *row, int T, uint64_t *key, double *q, int nbins, void *red) {
    int c = 0;
    for (int t = threadIdx.x; t < T; t += THREADS) {
        const double v = (double)row[t];
        const bool fin = isfinite(v);
        c += fin;
        key[t] = fin ? to_key(v) : NANKEY;
    }
    block_sort_keys<THREADS>(key, T);
    const int n = block_reduce<THREADS>(c, OpSum(), red);
    for (int j = threadIdx.x; j < nbins; j += THREADS) {
        double v = quiet_nan();
        if (n > 0) {
            const int num = j * (n - 1), lo = num / (nbins - 1), hi = min(lo + 1, n - 1);   // j (n - 1) < 2^24
            const double x0 = from_key(key[lo]), x1 = from_key(key[hi]);
            v = x0 + (x1 - x0) * ((double)(num - lo * (nbins - 1)) / (double)(nbins - 1));
        }
        q[j] = v;
    }
    __syncthreads();
    return n;
}

// sum over the bins of (b0 qa + b1 - qb)^2, in every lane
template <int THREADS>
__device__ __forceinline__ double residual(const double *qa, const double *qb, int nbins, double b0, double b1, void *red) {
    double s = 0.0;
    for (int j = threadIdx.x; j < nbins; j += THREADS) {
        const double r = b0 * qa[j] + b1 - qb[j];
        s += r * r;
    }
    return block_reduce<THREADS>(s, OpSum(), red);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void histogram_match_kernel(HmArgs g) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ double red[THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, nbins = g.nbins, Ta = g.Ta;
    uint64_t *key = reinterpret_cast<uint64_t *>(dyn);
    double *qa = dyn + g.P, *qb = qa + nbins;
    const float *arow = g.a + (long)k * g.lda;
    float *orow = g.out + (long)k * g.ldo;

    const int na = sorted_quantiles<THREADS>(arow, Ta, key, qa, nbins, red);
    const int nb = sorted_quantiles<THREADS>(g.b + (long)k * g.ldb, g.Tb, key, qb, nbins, red);
    if (g.qa)
        for (int j = tid; j < nbins; j += THREADS) g.qa[(size_t)k * nbins + j] = qa[j];
    if (g.qb)
        for (int j = tid; j < nbins; j += THREADS) g.qb[(size_t)k * nbins + j] = qb[j];
    const bool ok = na > 0 && nb > 0;
    if (tid == 0) g.info[3 * k] = na, g.info[3 * k + 1] = nb, g.info[3 * k + 2] = ok;
    if (!ok) {   // H1 (block-uniform)
        const float nanf_ = __int_as_float(0x7fc00000);
        for (int t = tid; t < Ta; t += THREADS) orow[t] = nanf_;
        if (tid == 0) g.beta[2 * k] = quiet_nan(), g.beta[2 * k + 1] = quiet_nan(), g.distance[k] = quiet_nan();
        return;
    }

    // ---- H3
    double sa = 0.0, sb = 0.0;
    for (int j = tid; j < nbins; j += THREADS) sa += qa[j], sb += qb[j];
    sa = block_reduce<THREADS>(sa, OpSum(), red), sb = block_reduce<THREADS>(sb, OpSum(), red);
    const double am = sa / (double)nbins, bm = sb / (double)nbins;
    double Saa = 0.0, Sab = 0.0, Paa = 0.0, Pab = 0.0;
    for (int j = tid; j < nbins; j += THREADS) {
        const double x = qa[j], y = qb[j];
        Saa += (x - am) * (x - am), Sab += (x - am) * (y - bm);
        Paa += x * x, Pab += x * y;
    }
    Saa = block_reduce<THREADS>(Saa, OpSum(), red), Sab = block_reduce<THREADS>(Sab, OpSum(), red);
    Paa = block_reduce<THREADS>(Paa, OpSum(), red), Pab = block_reduce<THREADS>(Pab, OpSum(), red);
    if (qa[0] == qa[nbins - 1]) Saa = 0.0, Sab = 0.0;   // a constant moving trace, whatever the rounding of am leaves
    double b0, b1;
    if (Saa == 0.0) {
        b0 = 0.0, b1 = g.nonneg ? fmax(bm, 0.0) : bm;
    } else {
        b0 = Sab / Saa, b1 = bm - b0 * am;
        if (g.nonneg && !(b0 >= 0.0 && b1 >= 0.0)) {
            const double f1 = fmax(bm, 0.0), s0 = Paa != 0.0 ? fmax(Pab / Paa, 0.0) : 0.0;
            const double r1 = residual<THREADS>(qa, qb, nbins, 0.0, f1, red), r2 = residual<THREADS>(qa, qb, nbins, s0, 0.0, red);
            if (r2 < r1) b0 = s0, b1 = 0.0;
            else b0 = 0.0, b1 = f1;
        }
    }
    // ---- H5
    const double rss = residual<THREADS>(qa, qb, nbins, b0, b1, red);
    if (tid == 0) g.beta[2 * k] = b0, g.beta[2 * k + 1] = b1, g.distance[k] = sqrt(rss / (double)nbins);
    // ---- H4
    for (int t = tid; t < Ta; t += THREADS) {
        const double v = (double)arow[t];
        orow[t] = isfinite(v) ? (float)(v * b0 + b1) : __int_as_float(0x7fc00000);
    }
}

template <int THREADS>
int hm_launch(const HmArgs &g, int K, unsigned lds, hipStream_t st) {
    if (lds > 48u * 1024u) {   // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void *)histogram_match_kernel<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail((int)e, "dnmf_histogram_match: %u bytes of LDS: %s", lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(histogram_match_kernel<THREADS>, dim3((unsigned)K), dim3(THREADS), lds, st, g);
    return check_launch("dnmf_histogram_match");
}

}  // namespace
}  // namespace dnmf

extern "C" {

int dnmf_histogram_match(const float *a, long lda, int Ta, const float *b, long ldb, int Tb, int K, int nbins, int nonneg, float *out,
                         long ldo, double *beta, double *distance, int *info, double *qa, double *qb, dnmf_stream_t stream) {
    using namespace dnmf;
    const char *fn = "dnmf_histogram_match";
    DNMF_REQUIRE(a && b && out && beta && distance && info, DNMF_E_NULL, "%s: NULL argument", fn);
    DNMF_REQUIRE(K >= 1 && Ta >= 1 && Tb >= 1, DNMF_E_SHAPE, "%s: K=%d rows, Ta=%d, Tb=%d samples", fn, K, Ta, Tb);
    DNMF_REQUIRE(nbins >= 2, DNMF_E_SHAPE, "%s: nbins=%d: at least 2", fn, nbins);
    DNMF_REQUIRE(nonneg == 0 || nonneg == 1, DNMF_E_SHAPE, "%s: nonneg=%d: 0 (regular) or 1 (non-negative)", fn, nonneg);
    DNMF_REQUIRE(lda >= Ta && ldo >= Ta, DNMF_E_SHAPE, "%s: lda=%ld ldo=%ld below a row of Ta=%d", fn, lda, ldo, Ta);
    DNMF_REQUIRE(ldb == 0 || ldb >= Tb, DNMF_E_SHAPE, "%s: ldb=%ld: 0 (one row for all) or at least Tb=%d", fn, ldb, Tb);
    DNMF_REQUIRE(Ta <= HM_MAX_ELEMS && Tb <= HM_MAX_ELEMS && nbins <= HM_MAX_BINS && K <= HM_MAX_ROWS, DNMF_E_UNSUPPORTED,
                 "%s: K=%d, Ta=%d, Tb=%d, nbins=%d: at most %d rows of at most %d samples (a row's float64 keys must fit LDS), at most "
                 "%d bins", fn, K, Ta, Tb, nbins, HM_MAX_ROWS, HM_MAX_ELEMS, HM_MAX_BINS);
    HmArgs g;
    g.a = a, g.b = b, g.lda = lda, g.ldb = ldb, g.ldo = ldo, g.Ta = Ta, g.Tb = Tb, g.nbins = nbins, g.nonneg = nonneg;
    g.P = sort_size(Ta > Tb ? Ta : Tb);
    g.out = out, g.beta = beta, g.distance = distance, g.qa = qa, g.qb = qb, g.info = info;
    const unsigned lds = (unsigned)(8 * (size_t)g.P + 16 * (size_t)nbins);
    const hipStream_t st = (hipStream_t)stream;
    return g.P <= HM_SMALL_ELEMS ? hm_launch<HM_SMALL_THREADS>(g, K, lds, st) : hm_launch<HM_THREADS>(g, K, lds, st);
}

}  // extern "C"
