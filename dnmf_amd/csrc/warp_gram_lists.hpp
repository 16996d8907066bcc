// K3n -- the kernel template, its parameters and its launchers: what both translation units of K3n need
// (warp_gram_lists.hip has the description, the other kernels and the entry points).
#pragma once
#include <mutex>
#include <type_traits>

#include "warp_taps.hpp"

namespace dnmf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The coordinates of a voxel's taps are the reference's fp32 sequence -- the ten-term FMA chain, n = 2q/(S-1) - 1,
// u = ((n+1)/2)(S-1) -- which is what decides floor() at lattice coincidences and what K2, K1 and the dense kernels
// evaluate (has the measured alternative and why it is not taken).

// Waves per SIMD the kernels are compiled for:
constexpr int LISTS_WAVES = 4;      // Z == 1 (128 registers)
constexpr int LISTS_WAVES_Z2 = 4;   // the same for Z == 2
constexpr int LISTS_WAVES_Z2L = 3;  // its long-list pass (two groups of four neurons' values in registers)
constexpr int LISTS_WAVES_Z3 = 3;   // and for Z > 2 (direct gathers only)

constexpr int LISTS_NG = 4;      // neurons evaluated together (register slots); longer lists are cut into groups
constexpr int LISTS_LGV = 2;      // log2 of the voxels per lane (consecutive x positions, interleaved by lane)
constexpr int LISTS_VPL = 1 << LISTS_LGV;
constexpr int LISTS_MAXW = 4;    // 64-neuron words of a tile's list: K <= 256
constexpr long LISTS_ITEMS = 16384;  // target number of wave-sized work items per launch
constexpr int LISTS_MAX_SLOTS = 3800;  // 4 waves x 3800 words of LDS per workgroup
// Staged gathers (Z <= 2): the taps of an 8 x 32 tile lie in a region of RR rows x RC floats of a footprint image; a wave
// copies that region of each listed neuron from global memory straight into LDS (global_load_lds, sixteen bytes per lane
// and request, through no registers) and gathers from there (see the kernel).
constexpr int LISTS_RR = 12, LISTS_RC = 40;                 // 9 tap rows + slack; 33 tap columns + alignment of the first + slack
constexpr int LISTS_REGION = LISTS_RR * LISTS_RC;            // floats per neuron: 1,920 bytes, 120 sixteen-byte pieces
static_assert(LISTS_RC % 4 == 0 && LISTS_REGION / 4 <= 128 && LISTS_REGION / 4 > 64, "stage_dma moves two pieces per lane");

struct ListParams {
    const float *At;       // (K, halo layout)
    const int *bbox;       // (K,6) xlo,xhi,ylo,yhi,zlo,zhi; lo > hi for an all-zero footprint
    const int *pair_slot;  // (K,K) symmetric; pairs outside the pattern point at the trash slot nslot-1
    const unsigned long long *axis_masks;  // per axis and bound the neurons whose box starts / ends there (see below)
    int nslot;             // K rhs slots, then the pattern pairs, then one trash slot
    int K;
    Volume vol;
    HaloLayout hl;
    const float *beta;
    int T;
    const int *times;
    int B;
    const float *frames;
    long ldf;
    const int *frame_ids;
    float *slab;  // (B, tables, nslot): table c of a frame from chunk c; with two launches table nchunks + c from the second
    unsigned long long *tile_masks;  // (B, ntiles, NW): the neuron list of every tile of every frame
    int4 *tile_desc;       // (B, ntiles): x = the tile's tap region packed as first halo row << 16 | first float of a halo row,
                           // -1: the taps do not fit LISTS_RR x LISTS_RC (or Z > 1): direct gathers; y = the list's first
                           // four neurons, one per byte in ascending order (0xff past the end); z = its length
    int nchunks, chunk_len;
    int tables;            // nchunks, or 2 nchunks when the long-list tiles go in a launch of their own
    int lgx, lgy, lgz;  // tile = (LISTS_VPL << lgx) x (1 << lgy) x (1 << lgz) voxels, lgx + lgy + lgz = 6: 8 x 32 x 1 for
                        // Z == 1 (a wave reads whole 128-byte lines of a frame: with 16 voxels along y every line was
                        // fetched twice, by tiles 32 apart in the walk), 8 x 16 x 2, 4 x 16 x 4
    int ntx, nty, ntz, ntiles;     // tile q = (qy * ntz + qz) * ntx + qx: walked along x
    unsigned long long *counters;  // optional: [0] += (tile, neuron) evaluations, [1] += (tile, pair) sums
};

// ---- neuron lists of the tiles ---------------------------------------------------------------------------
// axis_masks: for axis d (0,1,2) two tables of S_d + 2 entries of NW 64-bit words:
//   LO_d[i + 1] = { k : bbox_lo_d[k] <= i },  i = -1 .. S_d   (entry 0 is the empty set)
//   HI_d[i]     = { k : bbox_hi_d[k] >= i },  i =  0 .. S_d+1 (the last two are empty)
// so the neurons whose box meets [a, b] along d are LO_d[min(b, S_d) + 1] & HI_d[max(a, 0)]: the list of a tile is the
// AND of three such pairs.  Built by lists_axis_masks_kernel from bbox.
__host__ __device__ inline long axis_masks_offset(const Volume &vol, int d, int hi_table) {
    const int S[3] = {vol.X, vol.Y, vol.Z};
    long o = 0;
    for (int e = 0; e < d; ++e) o += 2L * (S[e] + 2);
    return o + (hi_table ? S[d] + 2 : 0);
}
__host__ __device__ inline long axis_masks_entries(const Volume &vol) { return 2L * (vol.X + vol.Y + vol.Z + 6); }

// ---- reading the slot tables -----------------------------------------------------------------------------
// The value of `slot` in a frame whose nchunks tables of nslot floats start at `tables`: the sum over the chunks in their order.
// This is what gram_lists_finish_kernel writes to G and r, and what the slot forms of K4 and K4h read in its place (trace_calls.hpp),
// so the three agree bit for bit.  The trash slot nslot - 1 stands for an exact zero.  The unsigned comparison also makes a zero
// of a negative slot or of one >= nslot instead of reading out of bounds; the layout produces neither (an rhs slot is a neuron
// index below K <= nslot - 1, pair_slot holds pattern slots and the trash slot only).
__device__ __forceinline__ float slot_chunk_sum(const float *__restrict__ tables, int nchunks, int nslot, int slot) {
    float s = 0.0f;
    if ((unsigned)slot < (unsigned)(nslot - 1))
        for (int c = 0; c < nchunks; ++c) s += tables[(long)c * nslot + slot];
    return s;
}

// PASS 1: the tiles with at most LISTS_NG neurons; PASS 2: the other tiles, into tables of their own (the consumers sum
// a frame's tables in order), launched on a side stream so that the two run side by side: pass 2 alone is a chain of
// memory round trips per tile with nothing to hide them behind.  Two kernels because the compiler allocates registers for the union
// of all paths of one: with the staged long-list code inside, the short-list loop spilled.  PASS 0 is the one-kernel
// form (every tile, long lists by direct gathers) for launches whose waves have only a short run of tiles each, where the
// second launch costs more than it saves; the host picks (lists_passes).
//
// ZM = 1: Z == 1 (four taps).  ZM = 2: Z == 2 -- the two z-taps of a corner are the adjacent floats of a halo row, fetched
// as the pair (slice 0, slice 1) whose members take the weight of the tap they stand for (warp_recon_grad.hip has the
// derivation), from the staged region like Z == 1 (a region is 12 rows x 20 columns x 2 slices) or, for tiles without a
// region, as two sixteen-byte gathers per voxel and neuron.  ZM = 3: Z > 2, four eight-byte gathers (z-pair of a corner).
// For Z >= 2 the blend is hierarchical (z, then y, then x: s0 + w1 (s1 - s0) along x and y, whose weights add up to 1
// exactly) from four weights per voxel; eight pre-multiplied weights per voxel cost 16 more registers.
template <int ZM, int NW, int FAST, bool F32OFF, int PASS>
__global__ __launch_bounds__(256, (ZM == 1 ? LISTS_WAVES : (ZM == 2 ? (PASS == 2 ? LISTS_WAVES_Z2L : LISTS_WAVES_Z2) : LISTS_WAVES_Z3))) void warp_gram_lists_kernel(ListParams p) {
    constexpr bool LONGPASS = PASS == 2;
    extern __shared__ float s_tab[];
    constexpr bool HASZ = ZM > 1;
    constexpr int NPAIR = LISTS_NG * (LISTS_NG + 1) / 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long item = (long)blockIdx.x * 4 + wave;  // chunk-major: neighbouring waves work on the same part of At
    if (item >= (long)p.nchunks * p.B) return;      // whole wave leaves; no workgroup barrier below
    const int chunk = (int)(item / p.B);
    const int b = (int)(item - (long)chunk * p.B);
    const int t = p.times ? p.times[b] : b;
    const float *__restrict__ yb = p.frames + (long)(p.frame_ids ? p.frame_ids[b] : b) * p.ldf;
    const Volume vol = p.vol;
    const HaloLayout hl = p.hl;
    const int K = p.K;
    const size_t plane = (size_t)hl.Pp * 4u;  // bytes of one neuron's footprint image

    float bt[30];
    load_beta(p.beta, p.T, t, bt);

    float *tab = s_tab + (size_t)wave * p.nslot;
    for (int i = lane; i < p.nslot; i += 64) tab[i] = 0.0f;
    const unsigned tab_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float *)tab;  // LDS byte address
    // this wave's LISTS_NG staging regions (Z <= 2 only; 16-byte aligned: the tables before them are padded)
    char *stage_lds = reinterpret_cast<char *>(s_tab + (((size_t)4 * p.nslot + 3) & ~(size_t)3)) +
                      (size_t)wave * (LISTS_NG * LISTS_REGION * 4);
    // piece e = lane + 64 j (j = 0, 1) of a region is row e / (RC/4), floats 4 (e % (RC/4)) .. +3
    constexpr int PPR = LISTS_RC / 4;
    const int piece_row[2] = {lane / PPR, (lane + 64) / PPR};
    const int piece_c4[2] = {lane - piece_row[0] * PPR, lane + 64 - piece_row[1] * PPR};
    const int4 *__restrict__ descs = p.tile_desc + (long)b * p.ntiles;

    const int lgx = p.lgx, lgz = p.lgz;
    const int lgy = p.lgy;
    const int lz = lane & ((1 << lgz) - 1), ly = (lane >> lgz) & ((1 << lgy) - 1), lx = lane >> (lgz + lgy);
    const int q_begin = chunk * p.chunk_len;
    const int q_end = min(q_begin + p.chunk_len, p.ntiles);
    const unsigned long long *__restrict__ masks = p.tile_masks + (long)b * p.ntiles * NW;
    unsigned long long n_eval = 0, n_pair = 0;  // wave-uniform
#ifdef DNMF_K3N_STAMPS
    // diagnostic build only (tools/k3n_stamps.py): wave cycles per section of the tile loop into counters[2..8] (section 3
    // is no longer there: its slot stays zero), then the number of non-empty tiles, of long-list tiles and of flushed runs
    unsigned long long st_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, st_last = __builtin_amdgcn_s_memtime();
#define DNMF_STAMP(i)                                                     \
    {                                                                     \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();      \
        st_acc[i] += now_ - st_last, st_last = now_;                      \
    }
#else
#define DNMF_STAMP(i)
#endif

    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // one lane, one LDS add (an atomic builtin here is rewritten into a cross-lane reduction loop)
    auto add_slot = [&](int slot, float total_in_last_lane) {
        const unsigned addr = tab_lds + 4u * (unsigned)slot;
        if (lane == 63) asm volatile("ds_add_f32 %0, %1" : : "v"(addr), "v"(total_in_last_lane) : "memory");
    };
    // slot of a pair: a scalar load issued before the arithmetic that precedes its use
    auto pair_slot_of = [&](int k, int l) {
        return __builtin_amdgcn_readfirstlane(p.pair_slot[max(k, 0) * K + max(l, 0)]);
    };
    // the lowest LISTS_NG set bits of a list (-1 past its end); `rem` loses them
    auto take_ids = [&](unsigned long long (&rem)[NW], int (&ks)[LISTS_NG]) {
#pragma unroll
        for (int i = 0; i < LISTS_NG; ++i) {
            int k = -1;
            bool found = false;
#pragma unroll
            for (int wd = 0; wd < NW; ++wd) {
                const bool take = !found && rem[wd] != 0;
                k = take ? 64 * wd + __builtin_ctzll(rem[wd]) : k;
                rem[wd] = take ? rem[wd] & (rem[wd] - 1) : rem[wd];
                found = found || take;
            }
            ks[i] = k;
        }
    };

    // partial sums of the current run of tiles with one and the same list of at most LISTS_NG neurons
    float acc_r[LISTS_NG], acc_p[NPAIR];
    int run_k[LISTS_NG];
    int run_n = 0;  // 0: nothing pending
    auto flush = [&]() {
        if (run_n == 0) return;
        auto go = [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            int sl[N][N];
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int j = i; j < N; ++j) sl[i][j] = pair_slot_of(run_k[i], run_k[j]);
            float sr[N], sp[N][N];
            int e = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                sr[i] = wave_sum_last(acc_r[i]);
#pragma unroll
                for (int j = i; j < N; ++j) sp[i][j] = wave_sum_last(acc_p[e++]);
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                add_slot(run_k[i], sr[i]);
#pragma unroll
                for (int j = i; j < N; ++j) add_slot(sl[i][j], sp[i][j]);
            }
        };
        using std::integral_constant;
        switch (run_n) {
            case 1: go(integral_constant<int, 1>{}); break;
            case 2: go(integral_constant<int, 2>{}); break;
            case 3: go(integral_constant<int, 3>{}); break;
            default: go(integral_constant<int, 4>{}); break;
        }
        static_assert(LISTS_NG == 4, "the dispatch above lists the group sizes");
        run_n = 0;
    };

    float b2[30];
    double_beta(bt, b2);
    Monomials<HASZ> mono = monomials<HASZ>(0.0f, 0.0f, 0.0f);
    int row_of_c = -1;  // the tile row (qy, qz) `mono` belongs to
    unsigned long long prev[NW];
#pragma unroll
    for (int wd = 0; wd < NW; ++wd) prev[wd] = 0;
    int prev_ids = -1;   // PASS 1: the previous tile's list (a list of one to four neurons is never -1: neuron 255 in all
                         // four bytes would need four equal entries)

    // The lists and regions of 64 tiles at a time, one tile per lane (a per-tile load of these wave-uniform words would
    // put a full memory round trip in front of every tile); a tile then takes its words from that lane.
    for (int q0 = q_begin; q0 < q_end; q0 += 64) {
      unsigned my_lo[NW], my_hi[NW];
      int my_reg = -1;   // region origin packed as row << 16 | column (both below 65536: checked on the host), -1: none
      int my_ids = -1, my_n = 0;   // PASS 1: the list itself (at most four neurons: one per byte) and its length
      int my_place = -1;           // qx | tile row << 16 (-1: not packed)
      {
          const int ql = min(q0 + lane, q_end - 1);
          if (PASS != 1) {   // the short-list pass needs no masks: its lists fit the descriptor
#pragma unroll
              for (int wd = 0; wd < NW; ++wd) {
                  const unsigned long long m = masks[(long)ql * NW + wd];
                  my_lo[wd] = (unsigned)m, my_hi[wd] = (unsigned)(m >> 32);
              }
          }
          const int4 dsc = descs[ql];
          my_reg = ZM == 3 ? -1 : dsc.x, my_ids = dsc.y, my_n = dsc.z, my_place = dsc.w;
      }
      if (LONGPASS) {   // nothing for this pass among these 64 tiles?
          int myn = 0;
#pragma unroll
          for (int wd = 0; wd < NW; ++wd) myn += __builtin_popcount(my_lo[wd]) + __builtin_popcount(my_hi[wd]);
          if (__ballot(myn > LISTS_NG) == 0) continue;
      }
      const int q1 = min(q0 + 64, q_end);
      for (int q = q0; q < q1; ++q) {
        const int jl = q - q0;
        unsigned long long msk[NW];
        int n = 0;  // wave-uniform
        bool same = true;
        int ids = -1;
        if (PASS == 1) {
            n = __builtin_amdgcn_readlane(my_n, jl);
            if (n == 0 || n > LISTS_NG) continue;
            ids = __builtin_amdgcn_readlane(my_ids, jl);
            same = ids == prev_ids;
            prev_ids = ids;
        } else {
#pragma unroll
            for (int wd = 0; wd < NW; ++wd) {
                msk[wd] = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)my_hi[wd], jl) << 32) |
                          (unsigned)__builtin_amdgcn_readlane((int)my_lo[wd], jl);
                n += __builtin_popcountll(msk[wd]);
                same = same && msk[wd] == prev[wd];
            }
        }
        if (n == 0 || (PASS == 1 && n > LISTS_NG) || (PASS == 2 && n <= LISTS_NG)) continue;
        DNMF_STAMP(0)   // tile bookkeeping
#ifdef DNMF_K3N_STAMPS
        st_acc[7] += 1, st_acc[8] += n > LISTS_NG, st_acc[9] += (!same || n > LISTS_NG) && run_n != 0;   // tiles, long lists, flushes
#endif
        if (!same || n > LISTS_NG) flush();
        DNMF_STAMP(1)   // reductions of a finished run
        if (PASS != 1) {
#pragma unroll
            for (int wd = 0; wd < NW; ++wd) prev[wd] = n > LISTS_NG ? 0 : msk[wd];
        }

        // the tile's column and row in the walk: from its descriptor (integer divisions by run-time values cost the
        // scalar unit ~20 instructions each)
        const int place = __builtin_amdgcn_readlane(my_place, jl);
        const int qx = place >= 0 ? (place & 0xffff) : q % p.ntx, rest = place >= 0 ? (place >> 16) : q / p.ntx;
        if (rest != row_of_c) {
            const int qz = HASZ ? rest % p.ntz : 0, qy = HASZ ? rest / p.ntz : rest;
            mono = monomials<HASZ>(0.0f, (float)((qy << lgy) + ly), (float)((qz << lgz) + lz));
            row_of_c = rest;
        }
        const int qz = HASZ ? rest % p.ntz : 0, qy = HASZ ? rest / p.ntz : rest;
        const int y = (qy << lgy) + ly, z = (qz << lgz) + lz;
        const bool yz_in = y < vol.Y && z < vol.Z;
        // staged gathers for this tile?  (wave-uniform)
        int reg_r0 = -1, reg_c0 = 0;
        if (ZM != 3) {
            const int rg = __builtin_amdgcn_readlane(my_reg, jl);
            reg_r0 = rg < 0 ? -1 : rg >> 16, reg_c0 = rg & 0xffff;
        }
        // lists of more than two groups keep the direct gathers (and their offsets)
        const bool staged = ZM != 3 && reg_r0 >= 0 && n <= (PASS == 2 ? 2 : 1) * LISTS_NG;
        // byte offset of volume voxel (0,0,0) inside a staged region, and of the region inside a footprint image
        const float lds_origin = 4.0f * (float)((HALO - reg_r0) * LISTS_RC + HALO * (ZM == 2 ? 2 : 1) - reg_c0);
        const unsigned reg_goff = (unsigned)(reg_r0 * hl.row4 + reg_c0 * 4);

        // staged through registers instead: the region of neuron k as two sixteen-byte pieces per lane, then into staging slot i
        // (only the never-taken branch of the short-list path below uses these two)
        auto stage_load = [&](int k, f32x4 (&piece)[2]) {
            const char *__restrict__ Ak = reinterpret_cast<const char *>(p.At) + (size_t)k * plane + reg_goff;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned o = (unsigned)(piece_row[j] * hl.row4 + piece_c4[j] * 16);
                asm("" : "+v"(o));
                piece[j] = (j == 0 || lane + 64 < LISTS_REGION / 4) ? *reinterpret_cast<const f32x4 *>(Ak + o)
                                                                   : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        auto stage_store = [&](int i, const f32x4 (&piece)[2]) {
            char *dst = stage_lds + i * (LISTS_REGION * 4);
            *reinterpret_cast<f32x4 *>(dst + lane * 16) = piece[0];
            if (lane + 64 < LISTS_REGION / 4) *reinterpret_cast<f32x4 *>(dst + (lane + 64) * 16) = piece[1];
        };
        // the short list (PASS 1: it came with the tile's descriptor; the one-kernel form reads it off the mask words)
        int ks[LISTS_NG];
#pragma unroll
        for (int i = 0; i < LISTS_NG; ++i) ks[i] = -1;
        if (PASS == 1) {
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i) ks[i] = i < n ? (int)(((unsigned)ids >> (8 * i)) & 0xffu) : -1;
        } else if (PASS == 0 && n <= LISTS_NG) {
            unsigned long long rem[NW];
#pragma unroll
            for (int wd = 0; wd < NW; ++wd) rem[wd] = msk[wd];
            take_ids(rem, ks);
        }
        // The regions of the list go from global memory straight into LDS, through no registers.  LDS-DMA: neuron k's region
        // into staging slot i, two sixteen-byte pieces per lane, 120 in all (piece e = lane + 64 j lands at
        // byte 16 e of the slot: the DMA writes lane l's 16 bytes at base + 16 l)
        auto stage_dma = [&](int k, int i) {
            const char *__restrict__ Ak = reinterpret_cast<const char *>(p.At) + (size_t)k * plane + reg_goff;
            auto dst = (__attribute__((address_space(3))) char *)(stage_lds + i * (LISTS_REGION * 4));
            __builtin_amdgcn_global_load_lds(Ak + (unsigned)(piece_row[0] * hl.row4 + piece_c4[0] * 16), dst, 16, 0, 0);
            if (lane + 64 < LISTS_REGION / 4)
                __builtin_amdgcn_global_load_lds(Ak + (unsigned)(piece_row[1] * hl.row4 + piece_c4[1] * 16), dst + 1024, 16, 0, 0);
        };
        // a short list's regions are all requested here, ahead of the tile's coordinate arithmetic, which hides their latency
        if (PASS != 2 && staged && n <= LISTS_NG) {
            // (the last tile's reads of the slots have long returned: their values went into its sums)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i)
                if (i < n) stage_dma(ks[i], i);
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- taps of this lane's four voxels: byte offsets of the two x-columns of the tap cell, weights ------------
        // Z == 1: off[.][dx] = byte offset of the (y, y+1) pair of x-column dx, w[.][dy + 2 dx] the four weights.
        // Z >= 2: off[.][0] = byte offset of the base corner's z-pair, w[.] = {weight of x-corner 1, of y-corner 1,
        // of the z-pair's members}.  A staged tile keeps the LDS byte offset of the base corner inside a region in off[.][0].
        unsigned off[LISTS_VPL][HASZ ? 1 : 2];
        float w[LISTS_VPL][4];
        float yv[LISTS_VPL];
        const int xt = qx << (lgx + LISTS_LGV);  // first x of the tile
        const float x0f = (float)(xt + lx);
        const bool full = xt + (LISTS_VPL << lgx) <= vol.X && (qy << lgy) + (1 << lgy) <= vol.Y && (qz << lgz) + (1 << lgz) <= vol.Z;
        // frame values: (scalar base + 32-bit lane offset) loads; the voxels of a lane are (1 << lgx) rows apart
        const unsigned yo0 = (unsigned)(((xt + lx) * vol.Y + min(y, vol.Y - 1)) * vol.Z + min(z, vol.Z - 1)) * 4u;
        const unsigned ystep = (unsigned)((vol.Y * vol.Z) << lgx) * 4u;
        auto taps = [&](auto full_tile) {
            constexpr bool FULL = decltype(full_tile)::value;
#pragma unroll
            for (int v = 0; v < LISTS_VPL; ++v) {
                const int x = xt + (v << lgx) + lx;
                float fx, fy, wx[2], wy[2];
                Monomials<HASZ> m = mono;
                m.x = x0f + (float)(v << lgx), m.xx = __fmul_rn(m.x, m.x), m.xy = __fmul_rn(m.x, m.y);
                if (HASZ) m.xz = __fmul_rn(m.x, m.z);
                axis_taps_halo(unnormalise(normalise_axis<FAST>(poly_a<HASZ>(b2, 0, m), vol, 0), vol.hx1), hl.xhi, fx, wx[0],
                               wx[1]);
                axis_taps_halo(unnormalise(normalise_axis<FAST>(poly_a<HASZ>(b2, 1, m), vol, 1), vol.hy1), hl.yhi, fy, wy[0],
                               wy[1]);
                const float uz = HASZ ? unnormalise(normalise_axis<FAST>(poly_a<HASZ>(b2, 2, m), vol, 2), vol.hz1) : 0.0f;
                const unsigned o0 = halo_offset<F32OFF>(fx, fy, hl, hl.origin4, hl.origin4f);
                const bool in = FULL || (yz_in && x < vol.X);   // a voxel beyond the volume: weights 0, frame value 0
                if constexpr (HASZ) {
                    float wzm[2];
                    const unsigned zo = z_pair_members<ZM, false>(uz, vol, wzm, nullptr);   // no derivatives here
                    // (a voxel beyond the volume is not covered by the tile's region: it reads the region's first floats,
                    // times zero)
                    off[v][0] = staged ? (in ? (unsigned)fmaf(fx, (float)(4 * LISTS_RC), fmaf(fy, 8.0f, lds_origin)) : 0u) : o0 + zo;
                    w[v][0] = wx[1], w[v][1] = wy[1], w[v][2] = in ? wzm[0] : 0.0f, w[v][3] = in ? wzm[1] : 0.0f;
                } else {
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        off[v][dx] = o0 + (dx ? (unsigned)hl.row4 : 0u);
                        if (staged && dx == 0)
                            off[v][0] = in ? (unsigned)fmaf(fx, (float)(4 * LISTS_RC), fmaf(fy, 4.0f, lds_origin)) : 0u;
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy) w[v][dy + 2 * dx] = in ? __fmul_rn(wx[dx], wy[dy]) : 0.0f;
                    }
                }
                unsigned yo = in ? yo0 + (unsigned)v * ystep : 0u;
                asm("" : "+v"(yo));
                const float val = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(yb) + yo);
                yv[v] = in ? val : 0.0f;
            }
        };
        if (full)
            taps(std::true_type{});
        else
            taps(std::false_type{});
        DNMF_STAMP(2)   // coordinates, weights, frame loads issued

        // z-pair members -> y -> x for Z >= 2: quad = the (y, z0), (y, z1), (y + 1, z0), (y + 1, z1) values of x-corner 0 / 1
        auto blend8 = [&](const float (&q0)[4], const float (&q1)[4], const float (&wv)[4]) {
            const float t00 = fmaf(wv[3], q0[1], wv[2] * q0[0]), t01 = fmaf(wv[3], q0[3], wv[2] * q0[2]);
            const float t10 = fmaf(wv[3], q1[1], wv[2] * q1[0]), t11 = fmaf(wv[3], q1[3], wv[2] * q1[2]);
            const float a0 = fmaf(wv[1], t01 - t00, t00), a1 = fmaf(wv[1], t11 - t10, t10);
            return fmaf(wv[0], a1 - a0, a0);
        };
        auto eval = [&](int k, float (&a)[LISTS_VPL]) {
            const char *__restrict__ Ak = reinterpret_cast<const char *>(p.At) + (size_t)k * plane;
#pragma unroll
            for (int v = 0; v < LISTS_VPL; ++v) {
                if constexpr (HASZ) {
                    float q[2][4];
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx)
                        gather_tap_row<ZM>(Ak, off[v][0] + (dx ? (unsigned)hl.row4 : 0u), hl, q[dx]);
                    a[v] = blend8(q[0], q[1], w[v]);
                } else {
                    float s = 0.0f;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        // the offsets are re-materialised as 32-bit values here so that the loads take the
                        // (scalar base + 32-bit vector offset) form; hoisted out of the neuron loop they become 64-bit pairs
                        unsigned o = off[v][e];
                        asm("" : "+v"(o));
                        const char *src = Ak + o;
                        const float s0 = *reinterpret_cast<const float *>(src);
                        const float s1 = *reinterpret_cast<const float *>(src + 4);
                        s = fmaf(s0, w[v][2 * e], s);
                        s = fmaf(s1, w[v][2 * e + 1], s);
                    }
                    a[v] = s;
                }
            }
        };
        // the warped values of the lane's voxels from staging slot i
        auto eval_staged = [&](int i, float (&a)[LISTS_VPL]) {
            const char *src0 = stage_lds + i * (LISTS_REGION * 4);
#pragma unroll
            for (int v = 0; v < LISTS_VPL; ++v) {
                const char *src = src0 + off[v][0];
                if constexpr (HASZ) {   // Z == 2: four eight-byte reads (the z-pairs of the corners)
                    float q[2][4];
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const float2 t0 = *reinterpret_cast<const float2 *>(src + dx * (4 * LISTS_RC));
                        const float2 t1 = *reinterpret_cast<const float2 *>(src + dx * (4 * LISTS_RC) + 8);
                        q[dx][0] = t0.x, q[dx][1] = t0.y, q[dx][2] = t1.x, q[dx][3] = t1.y;
                    }
                    a[v] = blend8(q[0], q[1], w[v]);
                } else {
                    float s = 0.0f;
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const float s0 = *reinterpret_cast<const float *>(src + dx * (4 * LISTS_RC));
                        const float s1 = *reinterpret_cast<const float *>(src + dx * (4 * LISTS_RC) + 4);
                        s = fmaf(s0, w[v][2 * dx], s);
                        s = fmaf(s1, w[v][2 * dx + 1], s);
                    }
                    a[v] = s;
                }
            }
        };
        auto dot4 = [&](const float (&a)[LISTS_VPL], const float (&cc)[LISTS_VPL], float init) {
            float s = init;
#pragma unroll
            for (int v = 0; v < LISTS_VPL; ++v) s = fmaf(a[v], cc[v], s);
            return s;
        };

        n_eval += n, n_pair += n * (n + 1) / 2;
        if (PASS != 2 && n <= LISTS_NG) {
            // the usual case: the whole list in registers; sums join the pending run (same list) or start one
            const bool fresh = run_n == 0;
            auto go = [&](auto nn) {
                constexpr int N = decltype(nn)::value;
                float a[N][LISTS_VPL];
                if (staged) {
                    // The regions have landed: they were requested BEFORE the tile's LISTS_VPL frame values (one load each, issued
                    // by taps() of a full tile, none in between: sched_barrier after the requests, this statement a compiler
                    // barrier), and vector memory returns in order -- "at most LISTS_VPL outstanding" = every region is in LDS,
                    // while the frame values (from HBM, the longest latency of the tile) may still be on their way: they are not
                    // needed until the sums after the taps, where the compiler places its own wait.  (2.98 -> 2.92 ms per 4000
                    // frames of 512x512, K = 100; nothing at Z = 2.)
                    if (full)
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LISTS_VPL) : "memory");
                    else
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        eval_staged(i, a[i]);
                        // Z >= 2: a neuron's taps are 32 values per lane; all four neurons' reads hoisted together spill
                        if (HASZ) __builtin_amdgcn_sched_barrier(0);
                    }
                } else if (staged) {
                    // Never taken: a staged tile took the branch above.  This is the earlier staging through registers, two
                    // neurons at a time.  It stays for now because the compiler orders and allocates the short-list kernels
                    // differently without it (same instruction count, other registers and schedule): removing it is a change
                    // to measure on its own.
#pragma unroll
                    for (int i0 = 0; i0 < N; i0 += 2) {
                        f32x4 piece[2][2];
#pragma unroll
                        for (int i = i0; i < N && i < i0 + 2; ++i) stage_load(ks[i], piece[i - i0]);
#pragma unroll
                        for (int i = i0; i < N && i < i0 + 2; ++i) stage_store(i, piece[i - i0]);
                    }
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        eval_staged(i, a[i]);
                        if (HASZ) __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < N; ++i) {   // Z == 1: the rows of all N neurons are requested together
                        eval(ks[i], a[i]);
                        if (HASZ) __builtin_amdgcn_sched_barrier(0);   // (32 values per neuron and lane)
                    }
                }
                int e = 0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    acc_r[i] = dot4(a[i], yv, fresh ? 0.0f : acc_r[i]);
#pragma unroll
                    for (int j = i; j < N; ++j, ++e) acc_p[e] = dot4(a[i], a[j], fresh ? 0.0f : acc_p[e]);
                }
            };
            using std::integral_constant;
            switch (n) {
                case 1: go(integral_constant<int, 1>{}); break;
                case 2: go(integral_constant<int, 2>{}); break;
                case 3: go(integral_constant<int, 3>{}); break;
                default: go(integral_constant<int, 4>{}); break;
            }
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i) run_k[i] = ks[i];
            run_n = n;
#ifdef DNMF_K3N_STAMPS
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            asm volatile("" ::"v"(acc_r[0]), "v"(acc_p[0]));
#endif
            DNMF_STAMP(4)   // taps from LDS (or direct gathers), per-lane sums
            continue;
        }
        if constexpr (PASS != 1) {
        if (PASS == 2 && staged) {
            // Five to eight neurons on a staged tile: two groups A (four) and B through the same staging slots.  A's
            // values stay in registers while its own sums are reduced like a finished run; then B's regions replace
            // A's in LDS and every B neuron is summed against A, the frame and the B neurons before it.  (With direct
            // gathers, every neuron of B evaluated twice and a table lookup in front of every group of sums these
            // tiles -- 4.8 % of all at 512x512, K=100 -- took 17.6 % of the kernel's time.)
            unsigned long long rem[NW];
#pragma unroll
            for (int wd = 0; wd < NW; ++wd) rem[wd] = msk[wd];
            int kA[LISTS_NG], kB[LISTS_NG];
            take_ids(rem, kA);
            take_ids(rem, kB);
            const int nB = n - LISTS_NG;
            float aA[LISTS_NG][LISTS_VPL], aB[LISTS_NG][LISTS_VPL];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the last tile's reads of the slots have returned
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i) stage_dma(kA[i], i);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i) {
                eval_staged(i, aA[i]);
                if (HASZ) __builtin_amdgcn_sched_barrier(0);
            }
            {
                int e = 0;
#pragma unroll
                for (int i = 0; i < LISTS_NG; ++i) {
                    acc_r[i] = dot4(aA[i], yv, 0.0f);
#pragma unroll
                    for (int j = i; j < LISTS_NG; ++j, ++e) acc_p[e] = dot4(aA[i], aA[j], 0.0f);
                    run_k[i] = kA[i];
                }
                run_n = LISTS_NG;
                flush();
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // group A's values are in registers
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i)
                if (i < nB) stage_dma(kB[i], i);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = 0; j < LISTS_NG; ++j) {
                if (j >= nB) break;   // wave-uniform
                eval_staged(j, aB[j]);
                int sc[LISTS_NG], sb[LISTS_NG];
#pragma unroll
                for (int i = 0; i < LISTS_NG; ++i) sc[i] = pair_slot_of(kA[i], kB[j]);
#pragma unroll
                for (int i = 0; i <= j; ++i) sb[i] = pair_slot_of(kB[i], kB[j]);
                float tc[LISTS_NG], tb[LISTS_NG];
#pragma unroll
                for (int i = 0; i < LISTS_NG; ++i) tc[i] = wave_sum_last(dot4(aA[i], aB[j], 0.0f));
#pragma unroll
                for (int i = 0; i <= j; ++i) tb[i] = wave_sum_last(dot4(aB[i], aB[j], 0.0f));
                const float tr = wave_sum_last(dot4(aB[j], yv, 0.0f));
#pragma unroll
                for (int i = 0; i < LISTS_NG; ++i) add_slot(sc[i], tc[i]);
#pragma unroll
                for (int i = 0; i <= j; ++i) add_slot(sb[i], tb[i]);
                add_slot(kB[j], tr);
            }
            DNMF_STAMP(6)   // a long-list tile, after its coordinates
            continue;
        }
        // longer lists, 3-D volumes, tiles without a region: groups of LISTS_NG neurons with direct gathers, every group
        // against itself and against every later group; reduced and added tile by tile
        unsigned long long rem1[NW];
#pragma unroll
        for (int wd = 0; wd < NW; ++wd) rem1[wd] = msk[wd];
        for (int g1 = 0; g1 < n; g1 += LISTS_NG) {
            int kA[LISTS_NG];
            float aA[LISTS_NG][LISTS_VPL];
            take_ids(rem1, kA);
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i)
                if (kA[i] >= 0) {
                    eval(kA[i], aA[i]);
                } else {
#pragma unroll
                    for (int v = 0; v < LISTS_VPL; ++v) aA[i][v] = 0.0f;
                }
#pragma unroll
            for (int i = 0; i < LISTS_NG; ++i) {
                if (kA[i] < 0) continue;
                add_slot(kA[i], wave_sum_last(dot4(aA[i], yv, 0.0f)));
#pragma unroll
                for (int j = i; j < LISTS_NG; ++j)
                    if (kA[j] >= 0) add_slot(pair_slot_of(kA[i], kA[j]), wave_sum_last(dot4(aA[i], aA[j], 0.0f)));
            }
            unsigned long long rem2[NW];
#pragma unroll
            for (int wd = 0; wd < NW; ++wd) rem2[wd] = rem1[wd];
            for (int g2 = g1 + LISTS_NG; g2 < n; g2 += LISTS_NG) {
                int kB[LISTS_NG];
                take_ids(rem2, kB);
#pragma unroll
                for (int j = 0; j < LISTS_NG; ++j) {
                    if (kB[j] < 0) continue;
                    float aB[LISTS_VPL];
                    eval(kB[j], aB);
                    int sl[LISTS_NG];
#pragma unroll
                    for (int i = 0; i < LISTS_NG; ++i) sl[i] = pair_slot_of(kA[i], kB[j]);
                    float sp[LISTS_NG];
#pragma unroll
                    for (int i = 0; i < LISTS_NG; ++i) sp[i] = wave_sum_last(dot4(aA[i], aB, 0.0f));
#pragma unroll
                    for (int i = 0; i < LISTS_NG; ++i)
                        if (kA[i] >= 0) add_slot(sl[i], sp[i]);
                }
            }
        }
        DNMF_STAMP(6)   // a long-list tile, after its coordinates
        }
      }
    }
    flush();

    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float *out = p.slab + ((long)b * p.tables + (LONGPASS ? p.nchunks : 0) + chunk) * p.nslot;
    for (int i = lane; i < p.nslot; i += 64) out[i] = tab[i];
    if (p.counters && lane == 0) {
        atomicAdd(&p.counters[0], n_eval);
        atomicAdd(&p.counters[1], n_pair);
#ifdef DNMF_K3N_STAMPS
        DNMF_STAMP(5)
        for (int i = 0; i < 10; ++i) atomicAdd(&p.counters[2 + i], st_acc[i]);
#endif
    }
}
#undef DNMF_STAMP

// The stream the second pass runs on and the two events of its fork / join, one set per device, made on first use and
// kept (the only state K3n holds; warp_gram_lists.hip defines it), with the mutex that serialises the fork / join of one device -- shared by every
// instantiation and both translation units: the events are shared, and a wait takes whatever was last recorded on its
// event when it is enqueued.
struct SideStream {
    std::mutex lock;
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
SideStream &side_stream();   // locks nothing; callers hold .lock around the fork / join

template <int ZM, int NW, int FAST, bool F32OFF>
void launch_lists_passes(const ListParams &p, unsigned nwg, size_t lds, hipStream_t st) {
    if (p.tables == p.nchunks) {
        hipLaunchKernelGGL((warp_gram_lists_kernel<ZM, NW, FAST, F32OFF, 0>), dim3(nwg), dim3(256), lds, st, p);
        return;
    }
    // fork: the second pass on the side stream behind the lists, join before anything that follows on `st`
    // (one host thread at a time through the fork / join of a device)
    SideStream &ss = side_stream();
    std::lock_guard<std::mutex> hold(ss.lock);
    const bool forked = ss.stream && hipEventRecord(ss.fork, st) == hipSuccess &&
                        hipStreamWaitEvent(ss.stream, ss.fork, 0) == hipSuccess;
    if (forked) {
        hipLaunchKernelGGL((warp_gram_lists_kernel<ZM, NW, FAST, F32OFF, 2>), dim3(nwg), dim3(256), lds, ss.stream, p);
        const bool recorded = hipEventRecord(ss.join, ss.stream) == hipSuccess;
        hipLaunchKernelGGL((warp_gram_lists_kernel<ZM, NW, FAST, F32OFF, 1>), dim3(nwg), dim3(256), lds, st, p);
        if (!recorded || hipStreamWaitEvent(st, ss.join, 0) != hipSuccess)
            (void)hipStreamSynchronize(ss.stream);   // the join could not be enqueued: wait for the side stream here
    } else {   // no side stream to be had: one after the other
        hipLaunchKernelGGL((warp_gram_lists_kernel<ZM, NW, FAST, F32OFF, 1>), dim3(nwg), dim3(256), lds, st, p);
        hipLaunchKernelGGL((warp_gram_lists_kernel<ZM, NW, FAST, F32OFF, 2>), dim3(nwg), dim3(256), lds, st, p);
    }
}

// the passes of one (Z form, list width), behind lists_tilemask_kernel on `st`
template <int ZM, int NW>
void launch_lists_t(const ListParams &p, unsigned nwg, size_t lds, hipStream_t st) {
    if (p.vol.fastdiv && p.hl.f32off)
        launch_lists_passes<ZM, NW, 1, true>(p, nwg, lds, st);
    else if (p.vol.fastdiv)
        launch_lists_passes<ZM, NW, 1, false>(p, nwg, lds, st);
    else
        launch_lists_passes<ZM, NW, 0, false>(p, nwg, lds, st);
}

// The Z >= 2 instantiations are compiled in warp_gram_lists_z.hip, the Z == 1 ones in warp_gram_lists.hip, with the same
// flags: two translation units only so that they compile side by side (about 50 s and 23 s; one unit would take their sum).
void launch_lists_z(const ListParams &p, unsigned nwg, size_t lds, hipStream_t st, int nw);

}  // namespace dnmf
