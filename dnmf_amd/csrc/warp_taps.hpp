// The warped sample from a halo-layout image, as K2 (warp_recon_grad.hip), K16 (motion_gn.hip) and K3n
// (warp_gram_lists.hpp) take it: the z-pair members, the tap-row gather, the value and gradient blend, the per-voxel
// front end of the kernels that walk along x -- and the host plan of that walk.  Compiled under each including file's
// own flags.
#pragma once
#include "common.hpp"

namespace dnmf {

typedef float f32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));   // four floats at an 8-byte aligned address
typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// ZM names the three forms of a sample: 1: Z == 1 (two coordinates, four taps); 2: Z == 2; 3: Z > 2.
//
// Z >= 2.  The two z-taps of a corner are adjacent floats of a halo row ((y + HALO) Z + z): they are fetched as ONE pair
// (izc, izc + 1) with izc = the base slice clamped into [0, Z - 2], i.e. the pair inside the volume that holds every
// in-range z-tap of the sample; a tap outside [0, Z) has no partner in the pair and its weight is dropped -- what
// grid_sample's per-corner bounds test does -- by giving each member of the pair the weight of the tap it stands for
// (or 0).  For Z == 2 the pair is always (0, 1) and the pairs of the corners y and y + 1 are 16 contiguous bytes: a voxel
// is TWO sixteen-byte gathers (one per x-corner; eight four-byte ones took 8.1 ms per 4000 frames at 512x512x2); for
// Z > 2 four eight-byte ones.
//
// z_pair_members: the weights wzm[2] of the pair's members for source coordinate uz and, with DERIV, vz[2] = d weight /
// d u_z of the tap a member stands for (vz may be null without DERIV).  Returns the byte offset of the pair in its halo row.
template <int ZM, bool DERIV>
__device__ __forceinline__ unsigned z_pair_members(float uz, const Volume &vol, float *wzm, float *vz) {
    static_assert(ZM == 2 || ZM == 3, "Z == 1 has no z-taps");
    if (ZM == 2) {
        // the pair is (0, 1): weights of its members by common.hpp: z_pair_weights.  d weight / d u of
        // member 0 is +1 for f = floor(u) = -1 and -1 for f = 0, of member 1 +1 for f = 0 and -1 for f = 1,
        // else 0: with c = 2 f + 1 (c - 2) that is -c where |c| = 1.
        const float uc = z_pair_weights(uz, wzm[0], wzm[1]);
        if constexpr (DERIV) {
            const float c0 = fmaf(2.0f, floorf(uc), 1.0f), c1 = c0 - 2.0f;
            vz[0] = fabsf(c0) == 1.0f ? -c0 : 0.0f;
            vz[1] = fabsf(c1) == 1.0f ? -c1 : 0.0f;
        }
        return 0u;
    }
    int iz;
    float wz[2];
    axis_weights(uz, iz, wz[0], wz[1]);
    // member 0 / 1 of the pair (izc, izc + 1) stands for tap iz / iz + 1 when iz == izc, member 0 for tap
    // iz + 1 when iz == izc - 1 (tap iz = -1 is outside), member 1 for tap iz when iz == izc + 1 (tap
    // iz + 1 = Z is outside)
    const int izc = clamp_index(iz, vol.Z - 1);
    const bool same = iz == izc;
    wzm[0] = same ? wz[0] : (iz + 1 == izc ? wz[1] : 0.0f);
    wzm[1] = same ? wz[1] : (iz == izc + 1 ? wz[0] : 0.0f);
    if constexpr (DERIV) {
        const bool below = iz + 1 == izc, above = iz == izc + 1;
        vz[0] = same ? -1.0f : (below ? 1.0f : 0.0f);
        vz[1] = same ? 1.0f : (above ? -1.0f : 0.0f);
    }
    return (unsigned)izc * 4u;
}

// One x-corner row of taps at byte offset o of the image at `base`: v[2 dy + dz] (Z == 1: v[dy]).
template <int ZM>
__device__ __forceinline__ void gather_tap_row(const char *__restrict__ base, unsigned o, const HaloLayout &hl,
                                               float (&v)[ZM > 1 ? 4 : 2]) {
    asm("" : "+v"(o));
    const char *t = base + o;   // (scalar base + 32-bit offset) loads
    if constexpr (ZM == 2) {          // (y, z0), (y, z1), (y + 1, z0), (y + 1, z1): one load, 8-byte aligned
        const f32x4_a8 r = *reinterpret_cast<const f32x4_a8 *>(t);
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
    } else if constexpr (ZM == 3) {   // the z-pair of corner y, then of corner y + 1
        const f32x2_a4 r0 = *reinterpret_cast<const f32x2_a4 *>(t);
        const f32x2_a4 r1 = *reinterpret_cast<const f32x2_a4 *>(t + hl.col4);
        v[0] = r0.x, v[1] = r0.y, v[2] = r1.x, v[3] = r1.y;
    } else {
        v[0] = *reinterpret_cast<const float *>(t);
        v[1] = *reinterpret_cast<const float *>(t + 4);
    }
}

// A voxel's sample with its derivatives: the two tap rows as gather_tap_row leaves them, the weight of corner 1 along x
// and y (corner 0 has 1 - that, exactly), and the z-pair members
template <bool HASZ>
struct WarpTaps {
    float t[2][HASZ ? 4 : 2];   // [dx][2 dy + dz]
    float wx1, wy1, wzm[2], vz[2];
};

// rec = A_tC at the voxel, g[d] = d rec / d u_d (source coordinates, voxel units)
template <bool HASZ>
__device__ __forceinline__ void blend_taps(const WarpTaps<HASZ> &q, float &rec, float (&g)[3]) {
    rec = 0.0f, g[0] = 0.0f, g[1] = 0.0f, g[2] = 0.0f;
#pragma unroll
    for (int dz = 0; dz < (HASZ ? 2 : 1); ++dz) {
        const float s00 = q.t[0][dz], s01 = q.t[1][dz];                              // s[dy][dx] of this z-slice
        const float s10 = q.t[0][(HASZ ? 2 : 1) + dz], s11 = q.t[1][(HASZ ? 2 : 1) + dz];
        // x- and y-blends as s0 + w1 (s1 - s0): the weights of an axis add up to exactly 1 (u - f and
        // (f + 1) - u are exact), the differences are the gradient's anyway -- one operation less per blend
        // than w0 s0 + w1 s1
        const float d0 = s01 - s00;                          // x-differences of the rows
        const float d1 = s11 - s10;
        const float a0 = fmaf(q.wx1, d0, s00);               // x-interpolated rows y0, y1
        const float a1 = fmaf(q.wx1, d1, s10);
        const float gy2 = a1 - a0;
        const float r2 = fmaf(q.wy1, gy2, a0);               // value of this z-slice
        const float gx2 = fmaf(q.wy1, d1 - d0, d0);
        if (HASZ) {
            rec = fmaf(q.wzm[dz], r2, rec);
            g[0] = fmaf(q.wzm[dz], gx2, g[0]);
            g[1] = fmaf(q.wzm[dz], gy2, g[1]);
            g[2] = fmaf(q.vz[dz], r2, g[2]);
        } else {
            rec = r2, g[0] = gx2, g[1] = gy2;
        }
    }
}

// The front end of a voxel for a thread that walks along x with (y, z) fixed: coordinates (the reference's FMA chain,
// common.hpp: poly_a, and its normalise / un-normalise round trip), x and y weights and the z-pair members into q;
// returns the byte offset of the tap row dx = 0 (the row dx = 1 is hl.row4 further).  `mono` holds the monomials without
// x, (x, xx, xy) those with it.
// ZC: the voxel's slice when it is known at compile time (Z == 2: 0 or 1), else -1.  z == 0: the four terms with z
// add an exact zero each (the Z == 1 chain); z == 1: their monomials are 1, 1, x, y.
template <int ZM, int FAST, bool F32OFF, int ZC = -1>
__device__ __forceinline__ unsigned warp_taps_front(const float *b2, const Monomials<true> &mono, float x, float xx, float xy,
                                                    const Volume &vol, const HaloLayout &hl, WarpTaps<(ZM > 1)> &q) {
    constexpr bool HASZ = ZM > 1;
    constexpr int ND = HASZ ? 3 : 2;
    float a[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (ZC == 0) {
        Monomials<false> m;
        m.x = x, m.y = mono.y, m.z = 0.0f, m.xx = xx, m.yy = mono.yy, m.zz = 0.0f, m.xy = xy, m.xz = 0.0f, m.yz = 0.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) a[d] = poly_a<false>(b2, d, m);
    } else {
        Monomials<true> m = mono;
        m.x = x, m.xx = xx, m.xy = xy;
        if constexpr (ZC == 1) {
            m.z = 1.0f, m.zz = 1.0f, m.xz = x, m.yz = mono.y;
        } else if (HASZ) {
            m.xz = __fmul_rn(x, mono.z);
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) a[d] = HASZ ? poly_a<true>(b2, d, m) : poly_a<false>(b2, d, Monomials<false>{m.x, m.y, 0.0f, m.xx, m.yy, 0.0f, m.xy, 0.0f, 0.0f});
    }
    float fx, fy, w0;
    axis_taps_halo(unnormalise(normalise_axis<FAST>(a[0], vol, 0), vol.hx1), hl.xhi, fx, w0, q.wx1);
    axis_taps_halo(unnormalise(normalise_axis<FAST>(a[1], vol, 1), vol.hy1), hl.yhi, fy, w0, q.wy1);
    const unsigned o0 = halo_offset<F32OFF>(fx, fy, hl, hl.origin4, hl.origin4f);   // base corner, slice 0
    unsigned zo = 0u;
    if constexpr (HASZ) zo = z_pair_members<ZM, true>(unnormalise(normalise_axis<FAST>(a[2], vol, 2), vol.hz1), vol, q.wzm, q.vz);
    return o0 + (ZM == 3 ? zo : 0u);
}

// ---- the host plan of the walk ---------------------------------------------------------------------------------------
// A block owns PLANE_ROWS x-rows by PLANE_COLS consecutive positions of the (y,z) plane; a lane owns one position (both
// slices of it at Z == 2) and walks down the rows.
constexpr int PLANE_ROWS = 32;    // voxels per lane: consecutive x (the block reduction is paid once per PLANE_ROWS voxels)
constexpr int PLANE_COLS = 256;   // positions of the (y,z) plane per block: 64 lanes x 4 waves

// blocks per frame; nub_out: blocks across the plane
inline long plane_walk_blocks(int X, int Y, int Z, int *nub_out) {
    const long nub = ((long)Y * (Z == 2 ? 1 : Z) + PLANE_COLS - 1) / PLANE_COLS;   // Z == 2: a lane owns both slices
    if (nub_out) *nub_out = (int)nub;
    return nub * ((X + PLANE_ROWS - 1) / PLANE_ROWS);
}

// bytes of the per-x table the walk reads with scalar loads (Entry per x), rounded up to 256
template <class Entry>
inline size_t plane_walk_xtab_bytes(int X) { return ((size_t)X * sizeof(Entry) + 255) / 256 * 256; }

// the limits of the walk, checked for entry point `who`; fills vol / hl / nblk / nub
inline int plane_walk_geometry(const char *who, int X, int Y, int Z, Volume &vol, HaloLayout &hl, int &nblk, int &nub) {
    vol = make_volume(X, Y, Z);
    hl = make_halo_layout(X, Y, Z);
    // 32-bit byte offsets into an image; 24-bit multiplies for the tap offsets
    DNMF_REQUIRE(hl.Pp < (1L << 29) && hl.row4 < (1 << 23) && hl.Xp < (1 << 23), DNMF_E_UNSUPPORTED,
                 "%s: volume %dx%dx%d too large for 32-bit tap offsets", who, X, Y, Z);
    const long nblk_l = plane_walk_blocks(X, Y, Z, &nub);
    DNMF_REQUIRE(nblk_l < (1L << 31), DNMF_E_UNSUPPORTED, "%s: %ld blocks per frame", who, nblk_l);
    nblk = (int)nblk_l;
    return DNMF_OK;
}

}  // namespace dnmf
