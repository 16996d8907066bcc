// K3n -- fused warp + per-frame Gram matrix + right-hand side for COMPACT footprints, neuron by neuron.
//
// Reference: the two contractions of DeformableNMF.update_temporal (Demix/dNMF.py:141-142) on the warped
// footprints of spatial_pushforward (dNMF.py:69-87), as K3 / K3s.
//
// Why another kernel.  The reference's Gaussians underflow to an exact zero ~30 px from their centre, so at
// 512x512, K=100 a voxel sees 1.1 non-zero footprints on average and A_t^T A_t has ~2.6 GFLOP of non-zero products
// per 4000 frames, not 11.6 TFLOP.  K3s skips whole 16-neuron blocks but still evaluates 16x16 products per active
// block pair on the matrix pipe and spends most of its time on block bookkeeping.  Here nothing is padded to
// blocks: a wave walks over tiles of 256 voxels, looks up which neurons can reach the tile at all and evaluates
// only those, on the vector ALU -- no MFMA: there is no dense operand left to feed it.
//
// Exactness.  A product is skipped only when one factor is an exact zero, so every sum equals the dense kernel's
// up to the order of fp32 additions:
//   - bbox[k] is the bounding box of the non-zeros of footprint k (dnmf_pack_footprints_lists);
//   - a tile's neuron list (lists_tilemask_kernel, one bit per neuron) is every k whose bbox meets a box that
//     CONTAINS all taps of the tile's voxels: the range of the warped coordinate over the tile by interval
//     arithmetic on the ten monomials, widened by a margin far above the fp32 rounding of either evaluation.  A
//     neuron listed without need contributes exact zeros (its footprint is zero outside its bbox);
//   - G[k,l] can be non-zero for some warp only if a 2x2(x2) tap cell meets both bboxes, i.e. if per axis
//     k_lo - 1 <= l_hi and l_lo - 1 <= k_hi: a static pattern, independent of the warp (both footprints move
//     under the same map).  Pairs outside the pattern are never accumulated and come out as 0.
//
// Data flow.  Lane = voxel: 32 lanes along y for Z == 1 (a wave reads whole 128-byte lines of the frame; 16 for 3-D
// volumes), four voxels per lane along x; tiles (8 x 32 x 1, 8 x 16 x 2 or 4 x 16 x 4 voxels) are walked along x, so a
// lane's (y,z) and the monomials without x change only at the end of a tile row.  At is in the halo layout of common.hpp:
// a tap outside the volume reads a zero, no masks or clamps along x and y.  Per listed neuron the warped values a_k of
// the lane's voxels are NTAP FMAs on NTAP gathered taps.  Gathered straight from global memory those are 2 x NTAP/2
// eight-byte loads per voxel with addresses that differ from lane to lane: ~16 cycles of a CU's texture path per
// wave-instruction whatever its width (tools/gather_probe.hip), eight per neuron and tile, which kept that path 96 %
// busy and set the kernel's time.  For Z <= 2 the taps of a tile lie in a region of 12 rows x 40 floats of the footprint
// image (lists_tilemask_kernel: the tile's tap box, first column aligned to 16 bytes): the wave copies that region of
// each listed neuron straight into LDS with two sixteen-byte requests per lane (global_load_lds) and gathers from LDS
// (2.5 cycles per instruction); tiles whose taps do not fit (a warp that scales a tile by more than ~10 %) and volumes
// with Z > 2 keep the direct gathers.  Then r_k += a_k.y and G_kl += a_k.a_l for the listed l >= k as per-lane partial sums.  While consecutive tiles have the same list the partial sums stay in registers;
// when the list changes: a fixed DPP tree over the 64 lanes and one LDS add by the last lane into the wave's private
// table of pattern slots.  LDS operations of one wave retire in order, so the sum is deterministic.  The table
// goes to a slab per (frame, chunk); the finish kernel adds the chunks in order and scatters the slots into dense
// G (K,K), r (K).
//
// Files.  warp_gram_lists.hpp: the parameters, the kernel template and its launchers.  This file: the pack, mask, pairs and
// finish kernels, the host side, the entry points and the Z == 1 instantiations.  warp_gram_lists_z.hip: the Z >= 2
// instantiations -- apart only so that the two compile side by side (about 23 s and 50 s), with the same flags.

#include "warp_gram_lists.hpp"

namespace dnmf {

__global__ __launch_bounds__(256) void lists_axis_masks_kernel(const int *__restrict__ bbox, int K, Volume vol, int NW,
                                                               unsigned long long *__restrict__ masks) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= axis_masks_entries(vol)) return;
    const int S[3] = {vol.X, vol.Y, vol.Z};
    long o = e;
    int d = 0;
    while (o >= 2L * (S[d] + 2)) o -= 2L * (S[d] + 2), ++d;
    const bool hi_table = o >= S[d] + 2;
    const int i = hi_table ? (int)(o - (S[d] + 2)) : (int)o - 1;
    for (int w = 0; w < NW; ++w) {
        unsigned long long m = 0;
        for (int j = 0; j < 64; ++j) {
            const int k = 64 * w + j;
            if (k >= K) break;
            const int lo = bbox[k * 6 + 2 * d], hi = bbox[k * 6 + 2 * d + 1];
            const bool in = lo <= hi && (hi_table ? hi >= i : lo <= i);
            m |= (unsigned long long)in << j;
        }
        masks[e * NW + w] = m;
    }
}

// One thread per (frame, tile): the tile's neuron list as NW 64-bit words.
template <int NW>
__global__ __launch_bounds__(256) void lists_tilemask_kernel(ListParams p) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long)p.B * p.ntiles) return;
    const int b = (int)(id / p.ntiles), q = (int)(id - (long)b * p.ntiles);
    const Volume vol = p.vol;
    const int t = p.times ? p.times[b] : b;
    float bt[30];
    load_beta(p.beta, p.T, t, bt);
    const int qx = q % p.ntx, rest = q / p.ntx, qz = rest % p.ntz, qy = rest / p.ntz;
    const int tx = LISTS_VPL << p.lgx, ty = 1 << p.lgy, tz = 1 << p.lgz;
    const int S[3] = {vol.X, vol.Y, vol.Z};
    const int first[3] = {qx * tx, qy * ty, qz * tz}, size[3] = {tx, ty, tz};
    float lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) lo[d] = (float)first[d], hi[d] = (float)min(first[d] + size[d] - 1, S[d] - 1);
    const bool hasz = vol.Z > 1;
    unsigned long long m[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) m[w] = ~0ull;
    int ta[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
    bool finite = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        int a = 0, c = 0;  // tap range along d; Z == 1: the taps sit in slice 0
        if ((d < 2 || hasz) && !tap_range(bt, vol, d, lo, hi, hasz, a, c)) {
            // NaN coordinates: every tap of the tile is pulled into the halo and reads zeros
#pragma unroll
            for (int w = 0; w < NW; ++w) m[w] = 0;
            finite = false;
            continue;
        }
        ta[d] = a, tc[d] = c;
        const unsigned long long *LO = p.axis_masks + (axis_masks_offset(vol, d, 0) + (min(c, S[d]) + 1 < 0 ? 0 : min(c, S[d]) + 1)) * NW;
        const unsigned long long *HI = p.axis_masks + (axis_masks_offset(vol, d, 1) + min(max(a, 0), S[d] + 1)) * NW;
#pragma unroll
        for (int w = 0; w < NW; ++w) m[w] &= LO[w] & HI[w];
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) p.tile_masks[id * NW + w] = m[w];
    // the region of a footprint image that holds every tap of the tile (the gathers clamp their base corner into
    // [-HALO, S], the second corner is one further), origin pulled back so that the region stays inside the image
    // (Z == 2: a halo row interleaves the two slices, column y of the volume is floats 2 (y + HALO), 2 (y + HALO) + 1, and
    // the region holds both slices of its columns, so the z range of the taps does not matter)
    int2 reg = make_int2(-1, 0);
    if (vol.Z <= 2 && finite && p.hl.Xp >= LISTS_RR && p.hl.rowf >= LISTS_RC && p.hl.Xp < 32768 && p.hl.rowf < 65536) {
        const int ax = max(ta[0], -HALO), cx = min(tc[0], vol.X + 1), ay = max(ta[1], -HALO), cy = min(tc[1], vol.Y + 1);
        const int r0 = min(ax + HALO, p.hl.Xp - LISTS_RR), c0 = min(((ay + HALO) * vol.Z) & ~3, p.hl.rowf - LISTS_RC);
        if (cx >= ax && cy >= ay && cx + HALO - r0 < LISTS_RR && (cy + HALO) * vol.Z + vol.Z - 1 - c0 < LISTS_RC)
            reg = make_int2(r0, c0);
    }
    int nlist = 0;
    unsigned ids = 0xffffffffu;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        unsigned long long rem = m[w];
        while (rem) {
            if (nlist < 4) ids = (ids & ~(0xffu << (8 * nlist))) | ((unsigned)(64 * w + __builtin_ctzll(rem)) << (8 * nlist));
            ++nlist, rem &= rem - 1;
        }
    }
    // w: the tile's place, qx | (qy * ntz + qz) << 16 when both fit 16 bits (else -1: the kernel divides)
    const int place = (qx < 65536 && rest < 32768) ? (qx | rest << 16) : -1;
    p.tile_desc[id] = make_int4(reg.x < 0 ? -1 : (reg.x << 16 | reg.y), (int)ids, nlist, place);
}

// G[b] (K,K), r[b] (K) <- ordered sum of the chunk tables of frame b
__global__ __launch_bounds__(256) void gram_lists_finish_kernel(const float *__restrict__ slab, int nchunks, int nslot,
                                                                const int *__restrict__ pair_slot, int K,
                                                                float *__restrict__ G, float *__restrict__ r) {
    const int b = blockIdx.x;
    const float *src = slab + (long)b * nchunks * nslot;
    for (int e = threadIdx.x; e < K * K + K; e += blockDim.x) {
        const int slot = e < K * K ? pair_slot[e] : e - K * K;
        const float s = slot_chunk_sum(src, nchunks, nslot, slot);
        if (e < K * K)
            G[(long)b * K * K + e] = s;
        else
            r[(long)b * K + (e - K * K)] = s;
    }
}

// ---- layout ----------------------------------------------------------------------------------------------
__global__ void lists_init_kernel(int *bbox, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < K * 6) bbox[i] = (i & 1) ? -1 : 0x7fffffff;
}

// At[k][halo(p)] = A[p][k] through a 32x32 LDS tile (the border of At is zeroed beforehand); bbox[k] grows over the
// non-zeros
__global__ __launch_bounds__(256) void lists_transpose_kernel(const float *__restrict__ A, long P, int K, Volume vol,
                                                              HaloLayout hl, float *__restrict__ At,
                                                              int *__restrict__ bbox) {
    __shared__ float tile[32][33];
    const long p0 = (long)blockIdx.x * 32;
    const int k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const long pp = p0 + i;
        const int k = k0 + tx;
        tile[i][tx] = (pp < P && k < K) ? A[pp * K + k] : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i;
        const long pp = p0 + tx;
        const bool in = k < K && pp < P;
        const float v = in ? tile[tx][i] : 0.0f;
        int x = 0, y = 0, z = 0;
        if (in) {
            voxel_xyz(pp, vol, x, y, z);
            At[(long)k * hl.Pp + (long)(x + HALO) * hl.rowf + (long)(y + HALO) * vol.Z + z] = v;
        }
        // the box grows by what the 32 lanes that hold neuron k found, one set of atomics per half wave with a non-zero
        // (one per non-zero voxel kept this kernel at 2.9 ms per call at 512x512, K=100: 76 GB/s)
        const bool nz = v != 0.0f;
        const unsigned long long any = __ballot(nz);
        if (any == 0) continue;   // wave-uniform
        int lo[3] = {nz ? x : 0x7fffffff, nz ? y : 0x7fffffff, nz ? z : 0x7fffffff};
        int hi[3] = {nz ? x : -1, nz ? y : -1, nz ? z : -1};
#pragma unroll
        for (int off = 16; off > 0; off >>= 1)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = min(lo[d], __shfl_xor(lo[d], off, 32));
                hi[d] = max(hi[d], __shfl_xor(hi[d], off, 32));
            }
        if (tx == 0 && hi[0] >= 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) atomicMin(&bbox[k * 6 + 2 * d], lo[d]), atomicMax(&bbox[k * 6 + 2 * d + 1], hi[d]);
        }
    }
}

// pattern of G and its slots: one block, thread k owns row k.  Slots: [0,K) rhs, then (k,k), then (k,l>k) in order.
__global__ __launch_bounds__(256) void lists_pairs_kernel(const int *__restrict__ bbox, int K, int *__restrict__ pair_slot,
                                                          int *__restrict__ nslot_out) {
    __shared__ int cnt[256];
    __shared__ int base[257];
    const int k = threadIdx.x;
    auto meets = [&](int a, int c) {
        bool ok = true;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int alo = bbox[a * 6 + 2 * d], ahi = bbox[a * 6 + 2 * d + 1];
            const int clo = bbox[c * 6 + 2 * d], chi = bbox[c * 6 + 2 * d + 1];
            ok = ok && alo <= ahi && clo <= chi && alo - 1 <= chi && clo - 1 <= ahi;
        }
        return ok;
    };
    int n = 0;
    if (k < K) {
        n = 1;  // (k,k)
        for (int l = k + 1; l < K; ++l) n += meets(k, l) ? 1 : 0;
    }
    cnt[k] = n;
    __syncthreads();
    if (k == 0) {
        int s = K;
        for (int i = 0; i < 256; ++i) base[i] = s, s += cnt[i];
        base[256] = s;  // trash slot
        *nslot_out = s + 1;
    }
    __syncthreads();
    if (k < K) {
        const int trash = base[256];
        int s = base[k];
        pair_slot[k * K + k] = s++;
        for (int l = k + 1; l < K; ++l) {
            const int v = meets(k, l) ? s++ : trash;
            pair_slot[k * K + l] = v;
            pair_slot[l * K + k] = v;
        }
    }
}

static void lists_tile_shape(const Volume &vol, int &lgx, int &lgy, int &lgz, int &ntx, int &nty, int &ntz, int &ntiles) {
    lgz = vol.Z == 1 ? 0 : (vol.Z == 2 ? 1 : 2);
    lgy = vol.Z == 1 ? 5 : 4;
    lgx = 6 - lgy - lgz;
    const int tx = LISTS_VPL << lgx, ty = 1 << lgy, tz = 1 << lgz;
    ntx = (vol.X + tx - 1) / tx;
    ntz = (vol.Z + tz - 1) / tz;
    nty = (vol.Y + ty - 1) / ty;
    ntiles = ntx * nty * ntz;
}

// chunks per frame that the workspace is sized for: LISTS_ITEMS wave-sized work items per launch (several rounds of four
// waves per SIMD), 1 .. 64 per frame
static long lists_max_chunks(int B) {
    const long want = (LISTS_ITEMS + B - 1) / B;
    return want < 1 ? 1 : (want > 64 ? 64 : want);
}

// chunks = n (1 .. 64) asks for n chunks per frame instead of the library's choice (0): the parity tests use it to give a
// wave of a small problem the long runs of tiles (and of equal lists) it has at the bench size.
static void lists_choose_chunks(int ntiles, int B, int chunks, int &nchunks, int &chunk_len) {
    long want = lists_max_chunks(B);
    if (chunks >= 1 && chunks <= want) want = chunks;   // never more tables than the workspace was sized for
    if (want > ntiles) want = ntiles;
    chunk_len = (int)((ntiles + want - 1) / want);
    nchunks = (ntiles + chunk_len - 1) / chunk_len;
}

static int lists_words(int K) { return K <= 64 ? 1 : (K <= 128 ? 2 : 4); }

// One kernel or two?  A second launch has its fixed cost per wave (table, slab, the scan for its tiles): it pays when a
// wave has a long run of tiles -- 512x512, K=100: 205 tiles per wave at 4000 frames (3.6 ms against 3.7), 25 at 400
// frames (0.89 ms against 0.51 in one kernel); 256x256x1000, K=50: 16 tiles per wave, 0.92 against 0.58.  The density
// of the footprints does not decide it: 512x512x4000 with K=200 (45 % of the tiles list more than four neurons) takes
// 9.1 ms in two launches and 12.2 in one.
// passes = 1 | 2 overrides the choice (0) (the parity tests run both forms on small problems).
static int lists_passes(int chunk_len, int passes) { return passes ? passes : (chunk_len < 100 ? 1 : 2); }

// the launch forms a caller may ask for: passes 0 | 1 | 2, chunks 0 .. 64, 0 the library's choice
static bool lists_form_ok(int passes, int chunks) { return passes >= 0 && passes <= 2 && chunks >= 0 && chunks <= 64; }

// tiles, chunks and tables of a launch on p.vol with p.B frames in the form (passes, chunks)
static void lists_plan(ListParams &p, int passes, int chunks) {
    lists_tile_shape(p.vol, p.lgx, p.lgy, p.lgz, p.ntx, p.nty, p.ntz, p.ntiles);
    lists_choose_chunks(p.ntiles, p.B, chunks, p.nchunks, p.chunk_len);
    p.tables = p.nchunks * lists_passes(p.chunk_len, passes);
}

template <int NW>
static void launch_tilemask(const ListParams &p, hipStream_t st) {
    const long nthreads = (long)p.B * p.ntiles;
    hipLaunchKernelGGL((lists_tilemask_kernel<NW>), dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, p);
}

SideStream &side_stream() {
    static SideStream per_device[64];
    static std::mutex create;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    SideStream &ss = per_device[dev];
    std::lock_guard<std::mutex> hold(create);
    if (!ss.stream) {
        hipStream_t s = nullptr;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&a, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&b, hipEventDisableTiming) == hipSuccess)
            ss.stream = s, ss.fork = a, ss.join = b;
    }
    return ss;
}

}  // namespace dnmf

extern "C" {

size_t dnmf_lists_axis_masks_bytes(int X, int Y, int Z, int K) {
    if (X <= 0 || Y <= 0 || Z <= 0 || K <= 0 || K > 64 * dnmf::LISTS_MAXW) return 0;
    return (size_t)dnmf::axis_masks_entries(dnmf::make_volume(X, Y, Z)) * dnmf::lists_words(K) * sizeof(unsigned long long);
}

int dnmf_pack_footprints_lists(const float *A, int X, int Y, int Z, int K, float *At, int *bbox, int *pair_slot,
                               int *nslot, void *axis_masks, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(A && At && bbox && pair_slot && nslot && axis_masks, DNMF_E_NULL, "dnmf_pack_footprints_lists: NULL buffer");
    DNMF_REQUIRE(X > 0 && Y > 0 && Z > 0 && K > 0, DNMF_E_SHAPE, "dnmf_pack_footprints_lists: X=%d Y=%d Z=%d K=%d", X, Y, Z,
                 K);
    DNMF_REQUIRE(K <= 64 * LISTS_MAXW, DNMF_E_UNSUPPORTED, "dnmf_pack_footprints_lists: K=%d > %d", K, 64 * LISTS_MAXW);
    const Volume vol = make_volume(X, Y, Z);
    const HaloLayout hl = make_halo_layout(X, Y, Z);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(At, 0, (size_t)K * hl.Pp * sizeof(float), st);
    DNMF_REQUIRE(e == hipSuccess, (int)e, "dnmf_pack_footprints_lists: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(lists_init_kernel, dim3((K * 6 + 255) / 256), dim3(256), 0, st, bbox, K);
    hipLaunchKernelGGL(lists_transpose_kernel, dim3((unsigned)((vol.P + 31) / 32), (unsigned)((K + 31) / 32)), dim3(256), 0,
                       st, A, vol.P, K, vol, hl, At, bbox);
    hipLaunchKernelGGL(lists_pairs_kernel, dim3(1), dim3(256), 0, st, bbox, K, pair_slot, nslot);
    hipLaunchKernelGGL(lists_axis_masks_kernel, dim3((unsigned)((axis_masks_entries(vol) + 255) / 256)), dim3(256), 0, st, bbox,
                       K, vol, lists_words(K), static_cast<unsigned long long *>(axis_masks));
    return check_launch("dnmf_pack_footprints_lists");
}

// workspace = slot tables (B, nchunks, nslot) floats, then the tile lists (B, ntiles, NW) 64-bit words
static size_t lists_slab_bytes(int nslot, int B) {
    const size_t tables = 2 * (size_t)dnmf::lists_max_chunks(B);   // up to two tables per chunk
    return ((size_t)B * tables * (size_t)nslot * sizeof(float) + 255) / 256 * 256;
}

// the tiles' list words, rounded up so that the 16-byte descriptors behind them are aligned
static size_t lists_masks_bytes(int K, int B, int ntiles) {
    return ((size_t)B * ntiles * dnmf::lists_words(K) * sizeof(unsigned long long) + 15) / 16 * 16;
}

size_t dnmf_warp_gram_rhs_lists_workspace(int nslot, int K, int X, int Y, int Z, int B) {
    using namespace dnmf;
    if (nslot <= 0 || B <= 0 || K <= 0 || K > 64 * LISTS_MAXW || X <= 0 || Y <= 0 || Z <= 0) return 0;
    int lgx, lgy, lgz, ntx, nty, ntz, ntiles;
    lists_tile_shape(make_volume(X, Y, Z), lgx, lgy, lgz, ntx, nty, ntz, ntiles);
    return lists_slab_bytes(nslot, B) + lists_masks_bytes(K, B, ntiles) + (size_t)B * ntiles * sizeof(int4);
}

int dnmf_warp_gram_rhs_lists(const float *At, const int *bbox, const int *pair_slot, const void *axis_masks, int nslot, int K,
                             int X, int Y, int Z, const float *beta, int T, const int *times, int B, const float *frames,
                             long ldf, const int *frame_ids, float *G, float *r, void *workspace, size_t workspace_bytes,
                             unsigned long long *counters, int passes, int chunks, dnmf_stream_t stream) {
    using namespace dnmf;
    DNMF_REQUIRE(At && bbox && pair_slot && axis_masks && beta && frames && workspace && (!G == !r), DNMF_E_NULL,
                 "dnmf_warp_gram_rhs_lists: NULL buffer");
    DNMF_REQUIRE(lists_form_ok(passes, chunks), DNMF_E_SHAPE, "dnmf_warp_gram_rhs_lists: passes=%d chunks=%d", passes, chunks);
    DNMF_REQUIRE(X > 0 && Y > 0 && Z > 0 && K > 0 && T > 0 && B > 0 && nslot > K, DNMF_E_SHAPE,
                 "dnmf_warp_gram_rhs_lists: X=%d Y=%d Z=%d K=%d T=%d B=%d nslot=%d", X, Y, Z, K, T, B, nslot);
    DNMF_REQUIRE(K <= 64 * LISTS_MAXW, DNMF_E_UNSUPPORTED, "dnmf_warp_gram_rhs_lists: K=%d > %d", K, 64 * LISTS_MAXW);
    DNMF_REQUIRE(nslot <= LISTS_MAX_SLOTS, DNMF_E_UNSUPPORTED,
                 "dnmf_warp_gram_rhs_lists: %d pattern slots > %d (footprints overlap too much for this kernel)", nslot,
                 LISTS_MAX_SLOTS);
    ListParams p;
    p.vol = make_volume(X, Y, Z);
    p.hl = make_halo_layout(X, Y, Z);
    DNMF_REQUIRE(ldf >= p.vol.P, DNMF_E_SHAPE, "dnmf_warp_gram_rhs_lists: ldf=%ld < P=%ld", ldf, p.vol.P);
    DNMF_REQUIRE(p.hl.Pp < (1L << 29) && p.hl.row4 < (1 << 23) && p.hl.Xp < (1 << 23), DNMF_E_UNSUPPORTED,
                 "dnmf_warp_gram_rhs_lists: volume %dx%dx%d too large for 32-bit tap offsets", X, Y, Z);
    p.At = At, p.bbox = bbox, p.pair_slot = pair_slot, p.nslot = nslot, p.K = K;
    p.axis_masks = static_cast<const unsigned long long *>(axis_masks);
    p.beta = beta, p.T = T, p.times = times, p.B = B;
    p.frames = frames, p.ldf = ldf, p.frame_ids = frame_ids;
    p.slab = static_cast<float *>(workspace);
    p.tile_masks = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + lists_slab_bytes(nslot, B));
    p.counters = counters;
    lists_plan(p, passes, chunks);
    DNMF_REQUIRE(workspace_bytes >= dnmf_warp_gram_rhs_lists_workspace(nslot, K, X, Y, Z, B), DNMF_E_WORKSPACE,
                 "dnmf_warp_gram_rhs_lists: workspace %zu < %zu bytes", workspace_bytes,
                 dnmf_warp_gram_rhs_lists_workspace(nslot, K, X, Y, Z, B));
    hipStream_t st = (hipStream_t)stream;
    const long nitems = (long)p.nchunks * B;
    const unsigned nwg = (unsigned)((nitems + 3) / 4);
    const int nw = lists_words(K);
    p.tile_desc = reinterpret_cast<int4 *>(reinterpret_cast<char *>(p.tile_masks) + lists_masks_bytes(K, B, p.ntiles));
    // four slot tables (padded to 16 bytes), then for Z <= 2 the four waves' staging regions
    const size_t lds = (((size_t)4 * nslot + 3) & ~(size_t)3) * sizeof(float) +
                       (Z <= 2 ? (size_t)4 * LISTS_NG * LISTS_REGION * sizeof(float) : 0);
    if (nw == 1) launch_tilemask<1>(p, st);
    else if (nw == 2) launch_tilemask<2>(p, st);
    else launch_tilemask<4>(p, st);
    if (Z > 1) {
        launch_lists_z(p, nwg, lds, st, nw);
    } else {
        if (nw == 1) launch_lists_t<1, 1>(p, nwg, lds, st);
        else if (nw == 2) launch_lists_t<1, 2>(p, nwg, lds, st);
        else launch_lists_t<1, 4>(p, nwg, lds, st);
    }
    if (G)
        hipLaunchKernelGGL(gram_lists_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, p.slab, p.tables, nslot,
                           pair_slot, K, G, r);
    return check_launch("dnmf_warp_gram_rhs_lists");
}

int dnmf_warp_gram_rhs_lists_chunks(int X, int Y, int Z, int B, int passes, int chunks) {
    using namespace dnmf;
    if (X <= 0 || Y <= 0 || Z <= 0 || B <= 0 || !lists_form_ok(passes, chunks)) return 0;
    ListParams p{};
    p.vol = make_volume(X, Y, Z), p.B = B;
    lists_plan(p, passes, chunks);
    return p.tables;
}

}  // extern "C"
