/*
 * dnmf_hip.h -- C ABI of libdnmf_hip.so: the MI355X (gfx950) kernels of the deformable-NMF hot path.
 *
 * The reference (mathdiane/dNMF) has no FFI or plugin interface: its hot path is stock torch / numpy
 * calls inside Demix/dNMF.py.  Each entry point below therefore replaces a group of those calls and
 * cites them (paths relative to the reference root).  The Python mirror of the reference classes
 * (dnmf_amd/Demix/dNMF.py) is the only caller; INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add to call the same functions from the original file.
 *
 * Conventions
 *   - plain C, no torch types; every pointer is a DEVICE pointer unless it says "host";
 *   - the caller owns every buffer (torch allocates them); the library keeps no state between calls
 *     other than the thread-local text behind dnmf_last_error();
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on it and returns -- no host synchronisation, no allocation;
 *   - return value: 0 = ok, negative = argument error (DNMF_E_*), positive = hipError_t;
 *   - layouts are the reference's: a volume is (X,Y,Z) row-major with voxel index
 *     p = (x*Y + y)*Z + z, P = X*Y*Z; footprints A are (P,K) (= torch (X,Y,Z,K) contiguous,
 *     Demix/dNMF.py:39-40); beta is (10,3,T) contiguous (Demix/dNMF.py:24-27); traces C are (K,T)
 *     with row stride ldc (Demix/dNMF.py:130); a frame is P floats;
 *   - Z == 1 means "z pinned to slice 0" (the reference divides 0/0 there; see oracle/dnmf_oracle.py);
 *   - HALO LAYOUT: the two single-channel images the hot kernels gather from -- the reconstruction images S
 *     (read by K2) and the neuron-major footprints At (read by K3n) -- carry a zero border of DNMF_HALO voxels
 *     around x and y: voxel (x,y,z) lives at (x + DNMF_HALO)*row + (y + DNMF_HALO)*Z + z with
 *     row = dnmf_halo_row(Y,Z) = (Y + 2*DNMF_HALO)*Z rounded up to a multiple of 32 floats (rows start on 128-byte
 *     lines), and an image has dnmf_halo_voxels(X,Y,Z) = (X + 2*DNMF_HALO)*row floats.  A trilinear tap outside the
 *     volume then reads a zero, which is what grid_sample's zero padding (Demix/dNMF.py:57) contributes, without
 *     per-corner bounds tests.  The kernels that WRITE such images (dnmf_recon_image*, dnmf_pack_footprints_lists)
 *     write the border (and the alignment excess of every row) too.
 */
#ifndef DNMF_HIP_H
#define DNMF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNMF_ABI_VERSION 7

#define DNMF_OK 0
#define DNMF_E_NULL (-1)      /* required pointer is NULL */
#define DNMF_E_SHAPE (-2)     /* non-positive or inconsistent size */
#define DNMF_E_UNSUPPORTED (-3) /* valid request outside what this build handles (e.g. K too large) */
#define DNMF_E_WORKSPACE (-4) /* workspace too small */

typedef void *dnmf_stream_t;

#define DNMF_HALO 2
/* Floats of one row / of one whole halo-layout image of an X x Y x Z volume (0 on bad sizes). */
int dnmf_halo_row(int Y, int Z);
long dnmf_halo_voxels(int X, int Y, int Z);

/* ABI version of the loaded library (DNMF_ABI_VERSION). */
int dnmf_version(void);
/* Text of the last error raised on the calling thread ("" if none). */
const char *dnmf_last_error(void);
/* "file:hash;file:hash;..." of the sources this library was compiled from (dnmf_amd/build.py computes the hashes and
 * passes them at compile time; "" for a build made without it).  bench.py reports counter data from profiles/ only when
 * the hashes recorded with them equal these. */
const char *dnmf_build_stamp(void);

/* ---- packed footprints ---------------------------------------------------------------------
 * The Gram kernel reads footprints from a zero-padded copy with row length Kp = 16*ceil((K+1)/16)
 * floats (16-byte aligned rows; one spare column carries the frame so that A_t^T y falls out of the
 * same matrix product).  dnmf_padded_k returns Kp (0 if K < 1). */
int dnmf_padded_k(int K);
/* Apk (P,Kp) <- A (P,K), pad columns zeroed.  Replaces nothing in the reference (layout change). */
int dnmf_pack_footprints(const float *A, long P, int K, float *Apk, int Kp, dnmf_stream_t stream);

/* ---- K1: materialised warp ---------------------------------------------------------------------
 * ExponentialFP.forward up to A_t (Demix/dNMF.py:54-57): q = basis.beta_t, n = 2q/(S-1)-1, zero-padded
 * trilinear gather of all K channels (torch grid_sample, align_corners=True).
 *   times  (B) int32 frame indices into beta's last axis
 *   A_t    (B,K,X,Y,Z) or NULL;  grid (X,Y,Z,3,B) normalised coordinates or NULL */
int dnmf_warp_gather(const float *A, int X, int Y, int Z, int K, const float *beta, int T,
                     const int *times, int B, float *A_t, float *grid, dnmf_stream_t stream);

/* ---- reconstruction image ------------------------------------------------------------------------
 * S[b,p] = sum_k C[k,times[b]] * A[p,k]  (fp32 MFMA).  Because the trilinear gather is linear in the
 * footprints, A_tC of Demix/dNMF.py:58 equals the gather of this single image; K2 consumes it.
 *   Apk (P,Kp) packed footprints, P = X*Y*Z; C (K,T) row stride ldc;
 *   S (B, halo layout) row stride lds >= dnmf_halo_voxels(X,Y,Z) floats, border written as zeros */
int dnmf_recon_image(const float *Apk, int X, int Y, int Z, int K, int Kp, const float *C, long ldc, const int *times,
                     int B, float *S, long lds, dnmf_stream_t stream);

/* ---- K2: fused warp + reconstruction + loss + d loss / d beta --------------------------------------
 * One mini-batch of update_motion (Demix/dNMF.py:186-190): forward (dNMF.py:54-58), F.mse_loss
 * (dNMF.py:188, mean over B*P) and its autograd gradient w.r.t. beta[:,:,times]; also reg of
 * dNMF.py:60-61 (gradient-free in the reference).
 *   S       recon images in the halo layout (zero border), frame b at S + s_ids[b]*lds (s_ids NULL -> b)
 *   frames  video frames, frame b at frames + frame_ids[b]*ldf (frame_ids NULL -> b).  Z == 2: ldf must be even (the two
 *           slices of a column are read as one aligned pair of floats; an odd ldf is DNMF_E_SHAPE)
 *   gout    NULL, or (B,P) upstream gradient d L / d A_tC of an arbitrary loss: then grad receives
 *           its chain through the warp unscaled, `frames` may be NULL and loss / frame_loss are
 *           meaningless (this is the backward of the autograd node the Python surface exposes)
 *   recon   (B,P) A_tC or NULL
 *   grad    (10,3,T): columns times[b] are INCREMENTED by the gradient (autograd .grad semantics);
 *           times must not contain duplicates
 *   norm_frames  number of frames the mean of the loss runs over (0 -> B): lets one launch evaluate many
 *           mini-batches of norm_frames frames each
 *   loss    (1) sum over b of frame_loss;  frame_loss (B) per-frame sum of squares / (norm_frames*P) or NULL
 *   reg     (B) or NULL
 *   workspace: dnmf_warp_recon_grad_workspace(X,Y,Z,B) bytes */
size_t dnmf_warp_recon_grad_workspace(int X, int Y, int Z, int B);
int dnmf_warp_recon_grad(const float *S, long lds, const int *s_ids, const float *frames, long ldf,
                         const int *frame_ids, const float *gout, int X, int Y, int Z, const float *beta,
                         int T, const int *times, int B, int norm_frames, float *recon, float *grad, float *loss,
                         float *frame_loss, float *reg, void *workspace, size_t workspace_bytes,
                         dnmf_stream_t stream);

/* ---- K3: fused warp + per-frame Gram + rhs ---------------------------------------------------------
 * The two large contractions of update_temporal (Demix/dNMF.py:141-142) on the warped footprints of
 * spatial_pushforward (dNMF.py:69-87) without materialising A_t:
 *   G[b] = A_t^T A_t (K,K),  r[b] = A_t^T y_b (K),  A_t = warp of A by beta[:,:,times[b]].
 * fp32 MFMA (v_mfma_f32_16x16x4_f32), upper triangle only, symmetric fill.
 *   Apk      packed footprints; a_frame_stride 0 = one A for all frames, else floats between the
 *            per-frame packed A of consecutive b (static update_temporal on an explicit A_t)
 *   beta     NULL = no warp: every voxel takes its own footprint row with weight 1 (the static update_temporal of
 *            Demix/dNMF.py:139-149 on an explicit A_t; a trilinear re-sampling at the identity is not exact in fp32)
 *   times    (B) or NULL (-> 0..B-1); frames / ldf / frame_ids as in K2
 *   G (B,K,K), r (B,K); workspace: dnmf_warp_gram_rhs_workspace(P,K,B) bytes */
size_t dnmf_warp_gram_rhs_workspace(long P, int K, int B);
int dnmf_warp_gram_rhs(const float *Apk, int Kp, int K, long a_frame_stride, int X, int Y, int Z,
                       const float *beta, int T, const int *times, int B, const float *frames, long ldf,
                       const int *frame_ids, float *G, float *r, void *workspace, size_t workspace_bytes,
                       dnmf_stream_t stream);

/* K3b: the same contraction on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16): warped footprints and frame are
 * evaluated in fp32 as above, rounded to bf16 (nearest even) and accumulated in fp32.  Reduced precision that the
 * reference does not have (it contracts in float64); offered for BASELINE config 5.  Same arguments, workspace and
 * results layout as dnmf_warp_gram_rhs. */
int dnmf_warp_gram_rhs_bf16(const float *Apk, int Kp, int K, long a_frame_stride, int X, int Y, int Z,
                            const float *beta, int T, const int *times, int B, const float *frames, long ldf,
                            const int *frame_ids, float *G, float *r, void *workspace, size_t workspace_bytes,
                            dnmf_stream_t stream);

/* ---- K3s: the same contraction with exact-zero block skipping ---------------------------------------------
 * For footprints that are exactly zero over most of the volume (the reference's Gaussians underflow to 0 in
 * fp32 beyond ~30 px; multiplicative updates keep zeros).  Neurons are taken in the order `order` (K ints, sorted
 * channel -> neuron; the caller sorts them along a space-filling curve) and cut into blocks of 16; a product in
 * which either factor is an exact zero is not evaluated, which changes no sum.
 * dnmf_pack_footprints_sparse: Aps (P,Ks) <- A[:, order], Ks = dnmf_sparse_k(K) = 16*ceil(K/16), zero padded;
 *   row_mask[p] bit b = row p has a non-zero among channels 16b..16b+15.  K <= 128.
 * dnmf_warp_gram_rhs_sparse: arguments as dnmf_warp_gram_rhs; G, r come out in the ORIGINAL neuron order.
 *   counters: NULL, or 2 x uint64 that are INCREMENTED by the MFMA instructions issued and by the (block, k-step)
 *   gathers executed (the work that was not skipped; bench.py's roofline uses them). */
int dnmf_sparse_k(int K);
int dnmf_pack_footprints_sparse(const float *A, long P, int K, const int *order, float *Aps, int Ks,
                                unsigned char *row_mask, dnmf_stream_t stream);
size_t dnmf_warp_gram_rhs_sparse_workspace(long P, int K, int B);
int dnmf_warp_gram_rhs_sparse(const float *Aps, int Ks, int K, const int *order, const unsigned char *row_mask,
                              int X, int Y, int Z, const float *beta, int T, const int *times, int B,
                              const float *frames, long ldf, const int *frame_ids, float *G, float *r,
                              void *workspace, size_t workspace_bytes, unsigned long long *counters,
                              dnmf_stream_t stream);

/* The same with a local block table: a wave keeps accumulators only for the (at most four) blocks it is working
 * with and adds finished tiles into its slab, so four waves fit on a SIMD.  Same arguments and results. */
size_t dnmf_warp_gram_rhs_sparse_lt_workspace(long P, int K, int B);
int dnmf_warp_gram_rhs_sparse_lt(const float *Aps, int Ks, int K, const int *order, const unsigned char *row_mask,
                                 int X, int Y, int Z, const float *beta, int T, const int *times, int B,
                                 const float *frames, long ldf, const int *frame_ids, float *G, float *r,
                                 void *workspace, size_t workspace_bytes, unsigned long long *counters,
                                 dnmf_stream_t stream);

/* ---- K3n: the same contraction neuron by neuron, for compact footprints ---------------------------------------
 * When every footprint is non-zero only inside a small box (the reference's Gaussians: ~61 px wide), almost all of
 * A_t^T A_t is a sum of products with an exact zero.  This kernel evaluates, per tile of 256 voxels, only the neurons
 * whose box the tile's taps can reach, on the vector ALU; sums are those of dnmf_warp_gram_rhs up to the order of
 * fp32 additions and are deterministic.  K <= 256.
 * dnmf_pack_footprints_lists: At (K, halo layout) <- A (P,K) transposed, border zeroed; bbox (K,6) int32 =
 *   xlo,xhi,ylo,yhi,zlo,zhi of the non-zeros of each footprint; pair_slot (K,K) int32 and *nslot (one int32, DEVICE) =
 *   the static pattern of G: slots [0,K) hold r, the following ones the pairs (k,l) whose boxes can meet under one tap
 *   cell, the last one (nslot-1) collects everything else; axis_masks (dnmf_lists_axis_masks_bytes(X,Y,Z,K) bytes) =
 *   per axis and coordinate the set of neurons whose box starts at or before / ends at or after it, from which the
 *   neuron list of a tile is three pairs of lookups.  The caller reads *nslot back once to size the workspace.
 * dnmf_warp_gram_rhs_lists: other arguments and results as dnmf_warp_gram_rhs (G dense (B,K,K), r (B,K); both NULL:
 *   the slot tables are left at the start of the workspace for dnmf_mu_temporal_slots);
 *   nslot <= 3800 (DNMF_E_UNSUPPORTED beyond: the footprints overlap too much, use K3 / K3s);
 *   workspace: dnmf_warp_gram_rhs_lists_workspace(nslot,K,X,Y,Z,B) bytes (slot tables, then the tile lists);
 *   counters: NULL, or 2 x uint64 INCREMENTED by the (tile, neuron) evaluations and the (tile, pair) sums done.
 *   Long videos: the tiles with more than four neurons are evaluated by a second launch on a side stream the library
 *   keeps (forked from `stream` behind the lists, joined back to it before the call's last kernel): ordering on
 *   `stream` is as if everything ran there.
 *   passes, chunks: the launch form, 0 = the library's choice (what every product caller passes).  passes 1 | 2: one
 *   launch, or the second one above, instead of the choice by tiles per wave; chunks 1 .. 64: that many chunks per frame
 *   (clipped to the number of tiles; a request above what the workspace is sized for falls back to the library's choice).
 *   Other values are refused (DNMF_E_SHAPE) before anything is launched.  Results differ between forms only in the order of
 *   fp32 additions.
 * dnmf_warp_gram_rhs_lists_chunks: slot tables per frame that a launch in the form (passes, chunks) writes; 0 for a
 *   bad shape or a refused form. */
size_t dnmf_lists_axis_masks_bytes(int X, int Y, int Z, int K);
int dnmf_pack_footprints_lists(const float *A, int X, int Y, int Z, int K, float *At, int *bbox, int *pair_slot,
                               int *nslot, void *axis_masks, dnmf_stream_t stream);
size_t dnmf_warp_gram_rhs_lists_workspace(int nslot, int K, int X, int Y, int Z, int B);
int dnmf_warp_gram_rhs_lists_chunks(int X, int Y, int Z, int B, int passes, int chunks);
int dnmf_warp_gram_rhs_lists(const float *At, const int *bbox, const int *pair_slot, const void *axis_masks, int nslot,
                             int K, int X, int Y, int Z, const float *beta, int T, const int *times, int B,
                             const float *frames, long ldf, const int *frame_ids, float *G, float *r, void *workspace,
                             size_t workspace_bytes, unsigned long long *counters, int passes, int chunks,
                             dnmf_stream_t stream);

/* Reconstruction image from the K3n layout: S (halo layout) as dnmf_recon_image, summing per tile of 4 x 64 voxels only the neurons
 * whose box meets the tile (static lists); bound by writing S.  K <= 256.  At and S 16-byte aligned, lds a multiple of 4
 * floats (dnmf_halo_voxels is a multiple of 32). */
int dnmf_recon_image_lists(const float *At, const int *bbox, int K, int X, int Y, int Z, const float *C, long ldc,
                           const int *times, int B, float *S, long lds, dnmf_stream_t stream);
/* The same with skip_empty != 0: tiles no neuron's box meets are left alone instead of being zeroed -- for a caller that
 * keeps S between calls and knows those tiles hold zeros already (an earlier call with skip_empty == 0 and the same bbox on
 * the same rows of S wrote them). */
int dnmf_recon_image_lists_ex(const float *At, const int *bbox, int K, int X, int Y, int Z, const float *C, long ldc,
                              const int *times, int B, float *S, long lds, int skip_empty, dnmf_stream_t stream);

/* One group of mini-batches of the fused motion epoch with the reconstruction images kept in the last-level cache:
 * dnmf_recon_image_lists and dnmf_warp_recon_grad (its frames / frame_ids / times / norm_frames / grad / frame_loss / reg
 * arguments, no upstream gradient, A_tC not returned) alternate over pieces of `chunk` frames that share ONE buffer of
 * `chunk` images, so S_t = A.C_t never makes the round trip through HBM (Demix/dNMF.py:58 + 186-190 for B frames).
 * Same kernels and sums as the two calls on all B frames (K2's finish kernel runs once at the end).  norm_frames > 0 is
 * required; B may exceed 65535; Z == 2: ldf even, as K2 asks; workspace: dnmf_motion_grad_lists_workspace(X,Y,Z,chunk,B) bytes. */
size_t dnmf_motion_grad_lists_workspace(int X, int Y, int Z, int chunk, int B);
int dnmf_motion_grad_lists(const float *At, const int *bbox, int K, const float *C, long ldc, const float *frames, long ldf,
                           const int *frame_ids, int X, int Y, int Z, const float *beta, int T, const int *times, int B,
                           int norm_frames, float *grad, float *frame_loss, float *reg, int chunk, void *workspace,
                           size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K4: multiplicative update of the traces --------------------------------------------------------
 * C <- C * (r + gamma*nbr) / (G C + 2 gamma C + 1e-32)  (Demix/dNMF.py:143-148, looped at dNMF.py:172-173)
 * on the hoisted G, r.  Arithmetic in fp64 like the reference's numpy code.
 *   G (T,K,K) symmetric, r (T,K)
 *
 * dnmf_mu_temporal: `iters` rounds without the neighbour term (gamma None or 0: frames independent, the
 *   whole loop runs in registers); C (K,T) fp32 row stride ldc, in/out, rounded to fp32 once at the end
 *   as dNMF.py:177 does.
 * dnmf_mu_temporal_step: ONE round with the neighbour term on an fp64 state, Cin -> Cout (both (K,T),
 *   row stride ldc, distinct buffers).  Neighbours of the first / last frame are replicated
 *   (dNMF.py:145) unless c_left / c_right (K doubles: the adjacent frame owned by the neighbouring
 *   T-shard) are given. */
int dnmf_mu_temporal(const float *G, const float *r, float *C, long ldc, int K, int T, int iters,
                     dnmf_stream_t stream);
/* dnmf_mu_temporal when G has a known pattern (the static pattern of K3n): nbr (K,NN) int32 lists for every row the
 * columns that can be non-zero in ascending order, padded with columns that cannot; NN in {8,16,32}.  Bit-identical
 * results (the skipped terms are exact zeros), NN instead of K terms per row and round. */
int dnmf_mu_temporal_nbr(const float *G, const float *r, float *C, long ldc, int K, int T, int iters, const int *nbr,
                         int NN, dnmf_stream_t stream);
/* The same straight from the slot tables of K3n: call dnmf_warp_gram_rhs_lists with G = r = NULL (the tables then stay
 * in its workspace as (T, nchunks, nslot) floats, nchunks = dnmf_warp_gram_rhs_lists_chunks(X,Y,Z,T,passes,chunks) of the
 * same form) and hand the workspace in as `slab`.  Bit-identical to finishing into a dense G first; saves writing and re-reading (T,K,K). */
int dnmf_mu_temporal_slots(const float *slab, int nchunks, int nslot, const int *pair_slot, float *C, long ldc, int K,
                           int T, int iters, const int *nbr, int NN, dnmf_stream_t stream);
int dnmf_mu_temporal_step(const float *G, const float *r, const double *Cin, double *Cout, long ldc, int K,
                          int T, double gamma, const double *c_left, const double *c_right,
                          dnmf_stream_t stream);

/* ---- K4h: exact non-negative least-squares traces (HALS / cyclic coordinate descent) -------------------
 * A second consumer of the G, r that K4 reads.  Per call it descends on
 *   F(C) = sum_t ( 1/2 c_t^T G_t c_t - r_t^T c_t ) + gamma/2 sum_{t=0..T-2} |c_{t+1} - c_t|^2 ,  C >= 0
 * (the function whose gradient K4 splits, replicated edges included) one coordinate at a time.  With n_t the number of
 * real neighbours of frame t (2 inside, 1 at an end, 0 when T = 1) the update of (k,t) is
 *   d = G_t[k,k] + gamma n_t
 *   c_k <- d > 0 ? max(0, (r_t[k] - sum_{l != k} G_t[k,l] c_l + gamma (c_{k,t-1} + c_{k,t+1}, real neighbours only)) / d) : 0
 * No 1e-32 enters; d == 0 (a footprint that is zero everywhere under this warp, gamma = 0) gives 0.  Arithmetic in fp64;
 * the kernel carries the gradient and applies c_k - grad_k / d, which differs from the formula in fp64 rounding only.
 * Sweep order (part of the contract: results are deterministic): k = 0 .. K-1 ascending in every frame; with gamma != 0
 * all even frames first, then all odd frames (red-black in t), each half sweep one launch.
 *   G (T,K,K) fp32 symmetric, r (T,K) fp32, K <= 256 (DNMF_E_UNSUPPORTED beyond).
 *   nbr: NULL, or (K,NN) int32, NN in {8,16,32}: per row the columns that can be non-zero, distinct, in [0,K), padded
 *     with columns that cannot (the lists of K3n's pattern): only those entries of G are read; same result, since a
 *     column outside the pattern holds an exact zero.  An entry outside [0,K) is skipped (it breaks the contract; nothing is
 *     read out of bounds for it).  NN is ignored when nbr is NULL.
 *   kkt: NULL, or (T) fp64: after the last sweep kkt[t] = max_k |pg_k| on the fp64 state, pg_k = grad_k if c_k > 0 else
 *     min(grad_k, 0), grad = G c - r + gamma (n_t c - neighbours): zero exactly at a solution.  On the fp32 forms this is
 *     the state BEFORE its rounding to fp32: it says how far the sweeps got (down to ~1e-15 of the gradient's terms), while
 *     the stored fp32 traces sit at their rounding floor (~1e-7 of them); dnmf_hals_temporal_kkt on the stored traces
 *     gives that figure.
 *
 * dnmf_hals_temporal: gamma = 0, `iters` sweeps in one launch (frames are independent); C (K,T) fp32, row stride ldc,
 *   in/out, rounded to fp32 once at the end like dnmf_mu_temporal.  iters = 0 leaves C alone and still fills kkt.
 * dnmf_hals_temporal_slots: the same straight from the slot tables of K3n (arguments as dnmf_mu_temporal_slots): entry
 *   (k,l) is the ordered sum over the chunks of slot pair_slot[k][l], r[k] that of slot k, the slot nslot-1 a zero.
 * dnmf_hals_temporal_step: ONE half sweep with the neighbour term on an fp64 state C (K,T), row stride ldc, in place:
 *   the frames t = parity, parity + 2, ... are updated from their neighbours of the other colour; parity in {0,1}.  A full
 *   sweep is parity 0, then parity 1.  The frames of the call are the whole time axis (no shard edges).
 * dnmf_hals_temporal_kkt: kkt (T) as above for an fp64 state C and any gamma (also 0); C is only read. */
int dnmf_hals_temporal(const float *G, const float *r, float *C, long ldc, int K, int T, int iters, const int *nbr, int NN,
                       double *kkt, dnmf_stream_t stream);
int dnmf_hals_temporal_slots(const float *slab, int nchunks, int nslot, const int *pair_slot, float *C, long ldc, int K,
                             int T, int iters, const int *nbr, int NN, double *kkt, dnmf_stream_t stream);
int dnmf_hals_temporal_step(const float *G, const float *r, double *C, long ldc, int K, int T, double gamma, int parity,
                            const int *nbr, int NN, dnmf_stream_t stream);
int dnmf_hals_temporal_kkt(const float *G, const float *r, const double *C, long ldc, int K, int T, double gamma,
                           const int *nbr, int NN, double *kkt, dnmf_stream_t stream);

/* ---- K5 / K6: multiplicative update of the footprints -----------------------------------------------
 * DeformableNMF.update_spatial (Demix/dNMF.py:151-160).
 * dnmf_spatial_accum: A1[p,k] = sum_t Y[t,p] C[k,t] (fp32 MFMA, dNMF.py:154) and Cs = C C^T (dNMF.py:153) over
 *   the T frames given: frame t at Y + frame_ids[t]*ldy (NULL -> t), trace column times[t] (NULL -> t);
 *   Ct: NULL, or the same traces frame-major, Ct[c*ldct + k] = C[k*ldc + c] for every column c the call touches: the
 *   matrix operands are then read in 64-byte runs instead of 16 rows x 16 bytes per instruction (the kernel's limit);
 *   accumulate != 0 adds to A1 / Cs instead of overwriting (frame chunks).  With the T axis sharded the caller
 *   sums A1 (P,K) and Cs (K,K) over ranks (RCCL all-reduce) before dnmf_mu_spatial.
 * dnmf_mu_spatial: A <- A * A1 / (A Cs + gamma D + 1e-32) in place (dNMF.py:155-159); D (P,K) or NULL. */
int dnmf_spatial_accum(const float *Y, long ldy, const int *frame_ids, const float *C, long ldc, const float *Ct,
                       long ldct, const int *times, int T, long P, int K, float *A1, float *Cs, int accumulate,
                       dnmf_stream_t stream);
int dnmf_mu_spatial(float *A, const float *A1, const float *Cs, const float *D, double gamma, long P, int K,
                    dnmf_stream_t stream);

/* ---- C1: frame-summed accumulators across the GPUs of a node -----------------------------------------
 * With the T axis sharded over ranks the two sums over frames of update_spatial (A1 = Y_i C^T, dNMF.py:154, and
 * Cs = C C^T, dNMF.py:153) are completed by ONE RCCL all-reduce each per update; nothing else on the path
 * communicates.  The communicator is the only state the library ever holds, behind an opaque handle the caller owns.
 * RCCL is bound at run time (dlopen of the librccl already in the process -- torch's -- else the system one), so
 * the library loads on hosts without it and these calls then return DNMF_E_UNSUPPORTED.
 *   dnmf_comm_unique_id: rank 0 fills `id` (HOST, DNMF_COMM_ID_BYTES) and hands it to the other ranks out of band
 *     (the host mirror broadcasts it over the caller's torch.distributed group);
 *   dnmf_comm_init: collective over the nranks processes, each with its own current HIP device;
 *   dnmf_allreduce_sum_f32: buf (count floats, device) <- sum over ranks, in place, enqueued on `stream`;
 *   dnmf_comm_destroy: releases the communicator (NULL is accepted).
 * Positive return values of these four are ncclResult_t codes (text in dnmf_last_error). */
#define DNMF_COMM_ID_BYTES 128
typedef void *dnmf_comm_t;
int dnmf_comm_unique_id(void *id_host);
int dnmf_comm_init(dnmf_comm_t *comm, const void *id_host, int nranks, int rank);
int dnmf_allreduce_sum_f32(dnmf_comm_t comm, float *buf, size_t count, dnmf_stream_t stream);
int dnmf_comm_destroy(dnmf_comm_t comm);

/* ---- K7: registered video ---------------------------------------------------------------------------
 * ExponentialFP.image_iwarp over the frames of spatial_pushforward (Demix/dNMF.py:81-83, 89-91, 95-103): every
 * lattice point takes the value of the voxel whose warped position ((n+1)/2 * sz, the reference's scaling
 * there) is nearest (float64 distances on the fp32 positions, ties to the lowest voxel index).  The search runs in
 * a window around the back-mapped lattice point whose radius follows from a lower bound of the warp's stretch, so
 * it returns what an exhaustive search returns; lattice points whose window would be too large (a folding or
 * violent warp, points far outside the warped image) are searched exhaustively.
 *   out (B,P) row stride ldo;  workspace: dnmf_image_iwarp_workspace(X,Y,Z,B) bytes (one flag per lattice point, sixteen constants of the
 *   frame's warp and one counter of marked points per frame), 8-byte aligned;
 *   exhaustive != 0: every lattice point by the exhaustive search (the checker of the window search);
 *   fallback_count: NULL, or one uint64 INCREMENTED by the lattice points that took the exhaustive search. */
size_t dnmf_image_iwarp_workspace(int X, int Y, int Z, int B);
int dnmf_image_iwarp(const float *frames, long ldf, const int *frame_ids, int X, int Y, int Z, const float *beta,
                     int T, const int *times, int B, float *out, long ldo, void *workspace, size_t workspace_bytes,
                     int exhaustive, unsigned long long *fallback_count, dnmf_stream_t stream);
/* dnmf_image_iwarp over colour channels that share the warp: frame row b holds `nchan` channels, channel c at
 * frames[row + c ldc_in]; the search runs once per lattice point and channel c of out row b (at c ldc_out) gathers from channel c
 * of the frame.  Otherwise as dnmf_image_iwarp (the same workspace; the fallback count is per lattice point, not per channel):
 * nchan >= 1; for nchan > 1 ldc_in, ldc_out >= P, ldf >= (nchan-1) ldc_in + P, ldo >= (nchan-1) ldc_out + P.  Channel by channel
 * the result equals dnmf_image_iwarp's on that channel. */
int dnmf_image_iwarp_channels(const float *frames, long ldf, long ldc_in, int nchan, const int *frame_ids, int X, int Y, int Z,
                              const float *beta, int T, const int *times, int B, float *out, long ldo, long ldc_out, void *workspace,
                              size_t workspace_bytes, int exhaustive, unsigned long long *fallback_count, dnmf_stream_t stream);

/* ---- Adam on beta for one epoch of mini-batches ------------------------------------------------------
 * update_motion steps the caller's torch.optim.Adam once per mini-batch on the whole (10,3,T) tensor
 * (Demix/dNMF.py:186-191; optimiser built at demo.py:42): columns outside the mini-batch get a zero gradient
 * but still move once they have moment history.  Columns are independent, so an epoch of `nsteps` steps in
 * which frame t belongs to mini-batch frame_step[t] (0-based, <0 = none) is evaluated per column:
 *   phase 0: the frame_step[t] zero-gradient steps before its mini-batch (then run K2 on all frames),
 *   phase 1: the step with grad[:, :, t] and the zero-gradient steps after it.
 * beta, exp_avg, exp_avg_sq (10,3,T) are the optimiser's own tensors, updated in place; step0 = steps taken
 * before this epoch.  torch.optim.Adam with amsgrad off, weight_decay 0, maximize off: the step with a gradient is
 * torch's fp32 arithmetic literally; a run of zero-gradient steps is evaluated in closed form (m b1^i, v b2^i, the
 * increments of p summed in double, ending when m underflows), within 1e-6 of the displacement of the step-by-step
 * fp32 evaluation.
 *   order  NULL, or (T) a permutation of the frames sorted by frame_step: thread r of the launch takes frame
 *          order[r], so the lanes of a wave walk through the same window of steps (speed only).
 *   workspace: dnmf_adam_epoch_workspace(nsteps) bytes (the step-dependent scalars of the epoch, rebuilt by each call) */
size_t dnmf_adam_epoch_workspace(int nsteps);
int dnmf_adam_epoch(float *beta, const float *grad, float *exp_avg, float *exp_avg_sq, int T, long step0,
                    const int *frame_step, const int *order, int nsteps, double lr, double beta1, double beta2,
                    double eps, int phase, void *workspace, size_t workspace_bytes, dnmf_stream_t stream);

/* ---- synthetic input: the render loop of the simulator ------------------------------------------------
 * WUtils/Simulator.py:66-73 (generate_video) with simulate_cell (:197-212): frame t0+t receives, neuron by
 * neuron in index order, fp32(traces[k,t] * exp(-|v - positions[k,:,t]|^2 / (2 shape_std))) added in fp32.
 *   positions (K,3,T_total) fp32, traces (K,T_total) fp64, out (T,P) fp32 row stride ldo (frames t0..t0+T-1)
 *   amp_max >= max(traces): bounds the window outside which a term is exactly 0 after the fp32 cast */
int dnmf_render_frames(const float *positions, const double *traces, int K, int T_total, int t0, int T, int X,
                       int Y, int Z, double shape_std, double amp_max, float *out, long ldo,
                       dnmf_stream_t stream);

/* ---- K5 / K6, list form (compact footprints) ---------------------------------------------------------------------
 * Reference: DeformableNMF.update_spatial, Demix/dNMF.py:151-160 -- A1 = Y_i C^T is only ever used multiplied by A, which is
 * an exact zero outside footprint k's non-zero box and stays zero under the update.  Tiles of 4 x-rows x 64 positions of the
 * (y,z) plane list the neurons whose box (bbox of dnmf_pack_footprints_lists) meets them; the sums exist only for (tile,
 * listed neuron) pairs, in a compact buffer A1c of `total` floats (1 KiB per pair) -- also what the ranks all-reduce.
 * tables: int[2 ntiles + 2 + 32 ntiles], ntiles = dnmf_spatial_lists_tiles: list lengths, entry offsets (tables[2 ntiles] =
 * total, -1 when a tile lists more than 32 neurons: use the dense kernels), an overflow counter, the lists.
 * dnmf_spatial_accum_lists: A1c and Cs = C C^T (float64 sums) over the T frames given (rows frame_ids[b] or b of Y, trace
 * columns times[b] or b).  dnmf_mu_spatial_lists: A1c in = the (all-reduced) sums, out = the new footprint values; A (P,K) is
 * updated in place at the listed entries (every other entry is and stays zero); At = the neuron-major halo copy of A. */
long dnmf_spatial_lists_tiles(int X, int Y, int Z);
int dnmf_spatial_lists_setup(const int *bbox, int K, int X, int Y, int Z, int *tables, dnmf_stream_t stream);
size_t dnmf_spatial_accum_lists_workspace(int X, int Y, int Z, long total, int T);
int dnmf_spatial_accum_lists(const float *Y, long ldy, const int *frame_ids, const float *C, long ldc, const int *times, int T, int X,
                             int Yd, int Z, int K, const int *tables, long total, float *A1c, float *Cs, void *workspace,
                             size_t workspace_bytes, dnmf_stream_t stream);
/* dnmf_spatial_accum_lists over colour channels that share the traces: row b of Y holds `nchan` channels ldyc floats apart and
 *   A1c[(tile, listed k)] = sum_c colours[c,k] sum_t Y^c_t[v] C[k,t],   Cs = C C^T as above;
 * colours (nchan, K) fp32 on the device, not NULL for nchan > 1 (NULL with nchan = 1: dnmf_spatial_accum_lists; colour 1
 * gives the same bits);
 * ldyc >= P and ldy >= (nchan-1) ldyc + P for nchan > 1.  Same tables, workspace and dnmf_mu_spatial_lists (with Cs multiplied
 * entry by entry by colours^T colours) as the single-channel form. */
int dnmf_spatial_accum_lists_channels(const float *Y, long ldy, long ldyc, int nchan, const float *colours, const int *frame_ids,
                                      const float *C, long ldc, const int *times, int T, int X, int Yd, int Z, int K, const int *tables,
                                      long total, float *A1c, float *Cs, void *workspace, size_t workspace_bytes,
                                      dnmf_stream_t stream);
int dnmf_mu_spatial_lists(float *A, const float *At, float *A1c, const float *Cs, const float *D, double gamma, int X, int Y, int Z,
                          int K, const int *tables, dnmf_stream_t stream);

/* ---- K6h: exact NNLS footprint update (HALS / cyclic coordinate descent), beside the multiplicative update K6 ---------
 * Not in the reference.  On the sums of K5 the footprint problem separates by voxel:
 *   min 1/2 a^T Cs a - A1[p]^T a + gamma D[p]^T a ,  a >= 0 ,  over the neurons whose box holds voxel p
 * (summed over p: 1/2 |Y_i - A C|^2 + gamma sum D o A up to a constant).  One sweep, k ascending over those neurons:
 *   g = sum_l a_l Cs[l,k] - A1[p,k] + gamma D[p,k]  (l over the same neurons, ascending, current values)
 *   a_k <- max(0, a_k - g / Cs[k,k])                (Cs[k,k] <= 0 or not finite: a_k stays)
 * A box is (xlo, xhi, ylo, yhi, zlo, zhi), inclusive (the bbox of dnmf_pack_footprints_lists, possibly dilated); a value
 * outside its neuron's box is zero and stays zero.  State and g are float64, `sweeps` >= 1 sweeps run in one launch and
 * the state is rounded to fp32 once; no floating-point atomics, the same bits on every run, and the two forms give the
 * same bits on the same sums.  kkt (K) float64 or NULL: per neuron the largest |pg| over its box, pg = g where a > 0,
 * else min(g, 0), of the float64 state after the last sweep (zero exactly at the solution).
 * dnmf_hals_spatial: A, A1, D (or NULL) as (P,K), in place; boxes (K,6) or NULL (every voxel free; X, Y, Z then unused,
 *   else X Y Z = P); values outside the boxes are written as 0.
 * dnmf_hals_spatial_kkt: kkt of a stored fp32 A for the given sums; A is only read.
 * dnmf_hals_spatial_lists: the arguments of dnmf_mu_spatial_lists plus bbox (K,6), the boxes the tables were made from;
 *   A1c in = the sums, out = the new values.  With kkt a workspace of dnmf_hals_spatial_lists_workspace bytes holds the
 *   per-(tile, slot) maxima a second launch reduces per neuron. */
int dnmf_hals_spatial(float *A, const float *A1, const float *Cs, const float *D, double gamma, long P, int K, int sweeps,
                      const int *boxes, int X, int Y, int Z, double *kkt, dnmf_stream_t stream);
int dnmf_hals_spatial_kkt(const float *A, const float *A1, const float *Cs, const float *D, double gamma, long P, int K,
                          const int *boxes, int X, int Y, int Z, double *kkt, dnmf_stream_t stream);
size_t dnmf_hals_spatial_lists_workspace(int X, int Y, int Z);
int dnmf_hals_spatial_lists(float *A, const float *At, float *A1c, const float *Cs, const float *D, double gamma, int X, int Y, int Z,
                            int K, const int *tables, const int *bbox, int sweeps, double *kkt, void *workspace,
                            size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K8: position initialiser ----------------------------------------------------------------------
 * Reference: Demix/MotionCorrect.py -- MotionCorrect.motion_correct_pwrigid :260-328 -> tile_and_correct_3d :1518-1608
 * (per frame: rigid shift, then one shift per patch inside rigid +- max_deviation_rigid; register_translation_3d :648-797 with
 * the matrix-multiply upsampled DFT :498-614) and MotionCorrect.apply_shifts_points :351-371.  The module is an orphan of
 * the reference tree, cannot be imported in the build container and has no fixtures: parity is pinned only against the
 * restatement oracle/motion_oracle.py ("parity unpinned").
 *
 * dnmf_register_patches_grid: the patch grid of sliding_window_3d :1190-1221 (windows of strides + overlaps every `strides`,
 * the last one flush with the end).  Returns the number of patches NP (0: the windows do not fit), dims[3] = patches per
 * axis, starts (NP,3) = first voxel of each patch in the reference's order (x outermost); dims / starts may be NULL (host
 * pointers).
 * dnmf_register_patches: frames (>= B rows of ldf floats, voxel p = (x Y + y) Z + z; row frame_ids[b] or b), tmpl (X Y Z)
 * -> rigid_shifts (B,3) as register_translation_3d returns them, patch_shifts (B,NP,3) with the signs of
 * tile_and_correct_3d's total_shifts (-x, -y, +z), i.e. what the class stores in x/y/z_shifts_els.  strides, overlaps,
 * max_shifts: 3 host ints each.  All device buffers fp32.  A search window holds at most 32 shifts per axis: max_shifts = 0
 * searches the whole axis, as numpy's empty slice cc[0:-0] does in the reference, and is refused (DNMF_E_UNSUPPORTED) on
 * an axis longer than 32 voxels.  upsample_factor = 1 returns the integer peak of the window, as the reference does.
 * valu (here and in dnmf_rigid_correct): 0 runs the axis transforms as f32 MFMAs, 1 on the vector ALU (the kernel kept as the
 * checker of the MFMA one); any other value is refused (DNMF_E_SHAPE). */
int dnmf_register_patches_grid(int X, int Y, int Z, const int *strides, const int *overlaps, int *dims, int *starts);
size_t dnmf_register_patches_workspace(int X, int Y, int Z, const int *strides, const int *overlaps, int B);
int dnmf_register_patches(const float *frames, long ldf, const int *frame_ids, int B, const float *tmpl, int X, int Y, int Z,
                          const int *strides, const int *overlaps, const int *max_shifts, int max_deviation_rigid,
                          int upsample_factor, float add_to_movie, float *rigid_shifts, float *patch_shifts, void *workspace,
                          size_t workspace_bytes, int valu, dnmf_stream_t stream);
/* Rigid correction of the frames against a template (tile_and_correct_3d :1518-1574 with max_deviation_rigid == 0, the
 * pass motion_correct_batch_rigid :1770-1877 makes to build the template a piecewise-rigid pass starts from):
 * rigid_shifts (B,3) as register_translation_3d returns them (the reference's shifts_rig holds their negatives, :1574);
 * corrected (NULL or B rows of ldc floats): every frame moved by its shift through the phases of its spectrum
 * (apply_shifts_dft :1028-1157, 3-D branch), minus add_to_movie; border_nan: what goes where the shift brought in voxels
 * from the other side -- 0 nothing (False of the reference), 1 NaN (True), 2 the frame's smallest value ('min'), 3 the
 * nearest row / column / slice inside ('copy'); tsum / tcount (both NULL, or P
 * floats / ints): += the finite corrected values and their number per voxel -- the nanmean of
 * tile_and_correct_wrapper :2057 is tsum / tcount. */
size_t dnmf_rigid_correct_workspace(int X, int Y, int Z, int B);
int dnmf_rigid_correct(const float *frames, long ldf, const int *frame_ids, int B, const float *tmpl, int X, int Y, int Z,
                       const int *max_shifts, int upsample_factor, float add_to_movie, int border_nan, float *rigid_shifts,
                       float *corrected, long ldc, float *tsum, int *tcount, void *workspace, size_t workspace_bytes,
                       int valu, dnmf_stream_t stream);
/* apply_shifts_points :351-371: points (K,3), patch_shifts (T,NP,3) as above, centers (NP,3) = patch start + strides / 2 ->
 * out (K,3,T): out[k,0/1,t] = p - (s[t] - s[0]), out[k,2,t] = p + (s[t] - s[0]) with s the shifts of the patch whose
 * centre is nearest to point k. */
int dnmf_apply_shifts_points(const float *points, int K, const float *patch_shifts, int T, int NP, const float *centers, float *out,
                             dnmf_stream_t stream);

/* ---- K9: the piecewise-rigid corrected movie ---------------------------------------------------------
 * Reference: Demix/MotionCorrect.py, tile_and_correct_3d :1639-1654 (shifts_opencv=True, the class default), the chunk
 * template of tile_and_correct_wrapper :2057-2058.  Per frame img (+ add_to_movie):
 *   field  the patch shifts on the grid of dnmf_register_patches_grid (dims, x outermost), moving the image by (+x, +y, +z)
 *          = (-s0, -s1, +s2) of patch_shifts, resized to (X, Y, Z) as skimage's resize (order 1, mode 'reflect') does:
 *          linear interpolation at c_d = (dims_d / N_d) (o + 0.5) - 0.5 with the edge mirrored;
 *   warp   skimage's warp (order 3, mode 'constant', cval 0) at (x + fx, y + fy, z + fz), fp32 sums: the cubic B-spline of
 *          the mirror-extended frame; a sample with any coordinate < 0 or > n - 1 is 0;
 *   clip   _clip_warp_output: 0 stays 0, the rest is clipped to [min, max] of img + add_to_movie;
 *   out    warp - add_to_movie (samples from outside the volume come out as -add_to_movie).
 * frames: >= B rows of ldf floats (voxel p = (x Y + y) Z + z; row frame_ids[b] or b), patch_shifts (B,NP,3) with the signs of
 * x/y/z_shifts_els (-x, -y, +z) as dnmf_register_patches returns them, strides / overlaps 3 host ints each, out B rows of ldo
 * floats.  tsum / tcount (both NULL, or P floats / ints): += the finite corrected values and their number per voxel (the
 * chunk template is tsum / tcount).  The workspace (dnmf_apply_pwrigid_workspace) holds the prefiltered frames of a chunk
 * of frames, at most 512 MiB; the call walks the frames in such chunks. */
size_t dnmf_apply_pwrigid_workspace(int X, int Y, int Z, const int *strides, const int *overlaps, int B);
int dnmf_apply_pwrigid(const float *frames, long ldf, const int *frame_ids, int B, int X, int Y, int Z, const int *strides,
                       const int *overlaps, const float *patch_shifts, float add_to_movie, float *out, long ldo, float *tsum,
                       int *tcount, void *workspace, size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K10: nearest point of an arbitrary point cloud ---------------------------------------------------------------------
 * ExponentialFP.image_iwarp on any flow (Demix/dNMF.py:95-103: scipy's NearestNDInterpolator, a cKDTree query in float64).
 * Per frame b < B: N points (x, y, z) at points + b ldp (fp32, or fp64 with points_f64 != 0; element stride 3), Q queries
 * (x, y, z) fp64 at queries + b ldq (ldq == 0: one query set for every frame).  For every query, the index i of the
 * smallest (d2, i) in lexicographic order, d2 = ((qx - px)^2 + (qy - py)^2) + (qz - pz)^2 in float64 on the coordinates as
 * stored: exact, ties to the lowest index, independent of the launch shape and of the order of atomics.
 *   index_out (B,Q) int32, row stride ldi >= Q;  values: NULL (indices only), or (B,N) fp32 with row stride ldv >= N,
 *   and then value_out (B,Q) fp32, row stride ldo >= Q, gets values[b][index] in the same pass (both NULL or both set);
 *   strides in elements: ldp >= 3N, ldq == 0 or >= 3Q;
 *   workspace: 256-byte aligned, at least dnmf_nearest_points_workspace(N, 1) bytes (one frame); the call walks the frames in
 *   chunks of what the workspace holds, at most dnmf_nearest_points_workspace(N, B) bytes (<= 512 MiB, or one frame);
 *   Q == 0 or B == 0: nothing to do (DNMF_OK);  N <= 0, Q < 0, B < 0 or a stride below a row: DNMF_E_SHAPE;  N >= 2^30:
 *   DNMF_E_UNSUPPORTED;  a short or misaligned workspace: DNMF_E_WORKSPACE.
 * Non-finite coordinates keep every access in bounds but give unspecified indices (dnmf_amd.ops refuses them).  A cloud
 * whose points crowd into few cells (duplicates, a line, one far outlier) costs up to O(N) per query. */
size_t dnmf_nearest_points_workspace(int N, int B);
int dnmf_nearest_points(const void *points, int points_f64, long ldp, int N, const double *queries, long ldq, int Q, int B,
                        const float *values, long ldv, int *index_out, long ldi, float *value_out, long ldo, void *workspace,
                        size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K11 / K12 / K13: tracks <-> warp, and the ROI trace read-out ------------------------------------------------------
 * q_t(x) = basis(x) . beta[:, :, t], basis = [1, x, y, z, x^2, y^2, z^2, xy, xz, yz] (Demix/dNMF.py:46-58), maps a voxel of
 * frame t to the point of the footprint volume sampled there; a neuron whose footprint is centred at r is seen in frame t at
 * the x* with q_t(x*) = r.  Coordinates are voxel indices.  Tracks are (K,3,T) contiguous, fp32 or fp64 (tracks_f64 != 0).
 *
 * K11 dnmf_fit_quadratic_warp: per frame t the beta_t that sends the tracked positions to `targets` (K,3) fp64 in the least-
 * squares sense.  A position with a non-finite coordinate is "not tracked in this frame" and skipped.  With u = 2 p / (S - 1)
 * - 1 per axis (u = 0 on an axis of extent 1), phi = basis(u) restricted to the free rows -- order 0 (translation): {0},
 * 1 (affine): {0..3}, 2 (quadratic): {0..9}, minus every row that involves an axis of extent 1 -- it minimises
 *     sum_k |phi(P[k,:,t]) B' - R[k]|^2 + ridge |B' - B'_id|_F^2
 * over the free rows of B' (B'_id: the identity map in the same coordinates; the other rows, and the output column of an
 * axis of extent 1, stay at the identity), in float64: normal equations, Gaussian elimination with partial pivoting.  beta is
 * B' converted back to voxel inputs in float64 and rounded once to fp32: beta (10,3,T), all T columns are written.  ok (T)
 * bytes: 0 where the system is singular to working precision (a pivot <= 1e-12 of the largest diagonal entry, or fewer
 * tracked neurons than free rows with ridge == 0); such a frame gets the exact identity.  No NaN is ever written to beta.
 *
 * K12 dnmf_invert_quadratic_warp: for every neuron k < K and frame j < B (column times[j] of beta, or j when times is NULL)
 * the x* with q_t(x*) = targets[k] by Newton's method in float64 on the analytic Jacobian, from start (K,3,B) fp64 (NULL:
 * the target itself, the solution at the identity), until a step is below tol in every coordinate; 32 steps at most.  out
 * (K,3,B) fp64; NaN where it did not converge, met |det J| < 1e-12 or left the finite numbers.
 *
 * K13 dnmf_roi_signals: WUtils/Simulator.py:230-240 get_roi_signals on frames that live on the device: >= T rows of ldf >=
 * X Y Z floats, row t = frame t.  out (K,T) fp64 = the mean of the box of 2 window[d] + 1 voxels per axis (window: 3 host
 * ints >= 0) around the position rounded half to even; voxels of the box outside the volume count as zeros (Utils.py:44-50),
 * NaN voxels are left out; NaN when the rounded position is outside the volume, not finite, or every voxel is NaN.  A box of
 * more than 4096 voxels: DNMF_E_UNSUPPORTED. */
int dnmf_fit_quadratic_warp(const void *tracks, int tracks_f64, int K, int T, const double *targets, int X, int Y, int Z, int order,
                            double ridge, float *beta, unsigned char *ok, dnmf_stream_t stream);
int dnmf_invert_quadratic_warp(const float *beta, int T, const int *times, int B, const double *targets, int K, const double *start,
                               double tol, double *out, dnmf_stream_t stream);
int dnmf_roi_signals(const float *frames, long ldf, int X, int Y, int Z, const void *tracks, int tracks_f64, int K, int T,
                     const int *window, double *out, dnmf_stream_t stream);

/* ---- K14: neuron centres of a template volume ----------------------------------------------------------------------------
 * A greedy matched-filter pursuit with the footprint model's own Gaussian (Demix/dNMF.py:39-40), g1(d) = exp(-d^2 / sigma^2)
 * truncated at r = ceil(3 sigma) voxels per axis; the reference has no counterpart (its real data ships with annotated
 * positions).  tests/detect_restatement.py is the definition in float64; all arithmetic here is fp32.
 *   filter   R = g (*) (img - background), separable, zero padding;
 *   score    S(q) = R(q) prod_axis sqrt(nmax / n(q)), n(q) = the sum of the squared taps that fall inside the volume at q, nmax
 *            its value in the middle of the axis: S = R wherever the window is inside the volume, the same noise level
 *            everywhere, and the peak of a blob cut by the border stays on its centre;
 *   pursuit  up to K times: p* = arg-max S (equal scores: the lowest voxel index; NaN scores never win), stop when S(p*) <=
 *            threshold or is not finite; per axis the peak of the parabola through ln S at p* and its two neighbours (at the
 *            first / last voxel of an axis of >= 3: p* and the two voxels inward), where those scores are > 0 and the parabola
 *            is concave, clamped to +-1/2 voxel: between two neighbours delta = (ln m - ln q) / (2 (ln m - 2 ln c + ln q)),
 *            ln S^ = ln c - sum (ln m - ln q) delta / 4; centre p^ = p* + delta (p^ = p*, S^ = S(p*) when p^ would lie within
 *            min_distance of an earlier centre); amplitude a = S^ / sqrt(prod_axis nmax sum_x g1(x - p^)^2) over the voxels of
 *            the volume within r of p*: the least-squares amplitude of the truncated footprint; S(q) -= a prod_axis sqrt(nmax /
 *            n(q)) sum_x g1(x - q) g1(x - p^) (same x, |x - q| <= r: the score of that footprint); S = -inf where
 *            |q - p^|_2 <= min_distance.
 * img: X Y Z floats, voxel p = (x Y + y) Z + z; sz: 3 host ints.  positions (K,3), amplitudes (K) fp32 and count (one int) on
 * the device; rows from count on are NaN.  One call is four launches (two filter passes, the table of tile maxima, one
 * workgroup that runs the whole pursuit) and no host synchronisation.  workspace: 4-byte aligned,
 * dnmf_detect_neurons_workspace(sz, K, sigma) bytes (0 on bad arguments) = two volumes and the table.
 * DNMF_E_SHAPE: sigma <= 0 or not finite, K < 1, a size < 1, min_distance < 0 or not finite, background not finite, threshold
 * NaN or +inf;  DNMF_E_UNSUPPORTED: sigma > 32, min_distance > 509, 2^31 voxels or more;  DNMF_E_WORKSPACE: a short or
 * misaligned workspace (nothing is launched). */
size_t dnmf_detect_neurons_workspace(const int *sz, int K, double sigma);
int dnmf_detect_neurons(const float *img, const int *sz, int K, double sigma, double min_distance, double threshold, double background,
                        float *positions, float *amplitudes, int *count, void *workspace, size_t workspace_bytes,
                        dnmf_stream_t stream);

/* ---- K15: per-frame neuron tracking by a local matched filter ------------------------------------------------------------
 * For every neuron k < K and frame j < T the peak of K14's score volume of that frame inside a search window around a
 * predicted position.  tests/track_restatement.py is the definition in float64; all arithmetic here is fp32 and the positions
 * are widened where they are stored.
 *   score    S_j = K14's score of frame j: taps g1(d) = exp(-d^2 / sigma^2) truncated at r = ceil(3 sigma), zero padding,
 *            background[j] taken off first, per-axis weight sqrt(nmax / n(q));
 *   window   c = predict[k, :, j] rounded half to even; the voxels q of the volume with |q_d - c_d| <= search[d] on every axis;
 *   pick     p* = arg-max of S_j over the window (equal scores: the lowest voxel index (x Y + y) Z + z; NaN scores never win);
 *   refine   K14's rule unchanged: per axis the log-parabola through S_j at p* and its two neighbours (at the first / last voxel
 *            of an axis of >= 3: p* and the two voxels inward), where those scores are > 0 and the parabola is concave, clamped
 *            to +-1/2 voxel; the neighbours are voxels of the volume and may lie outside the window; p^ = p* + delta;
 *   amplitude a = S^ / sqrt(prod_axis nmax sum_x g1(x - p^)^2) over the voxels of the volume within r of p*, as K14.
 * A row is NaN when the prediction is not finite, the window has no voxel inside the volume, S_j(p*) is not finite or
 * S_j(p*) <= threshold.  Nothing is subtracted and nothing excluded: the K T searches are independent, so a neuron within about
 * 2 sigma of a brighter one can be captured by it -- the search window is the guard.  Frame j does not depend on frame j - 1:
 * predict carries any prior.
 * frames: >= max row + 1 rows of ldf >= X Y Z floats, voxel p = (x Y + y) Z + z; sz, search: 3 host ints; times: T device row
 * indices (NULL: 0..T-1); predict: (K,3,T) when predict_per_frame, else (K,3) used for every frame, fp64 when predict_f64 else
 * fp32; background: T device floats (NULL: 0).  positions (K,3,T) fp64, the layout K11 / K12 / K13 read; amplitudes and peaks
 * (= S_j(p*)) (K,T) fp32, either may be NULL.  One launch, one workgroup per (k, j), which stages the region of at most
 * prod_axis min(S, 2 (search + 1 + r) + 1) voxels in LDS; no host synchronisation, no workspace.
 * DNMF_E_NULL: frames, sz, predict, search or positions NULL;  DNMF_E_SHAPE: sigma <= 0 or not finite, K or T < 1, a size < 1, a
 * negative search entry, threshold NaN or +inf, ldf < X Y Z;  DNMF_E_UNSUPPORTED: sigma > 32, 2^31 voxels or K T searches or
 * more, a region that needs more than 48 KiB of LDS (the message names its size).  Nothing is launched on an error. */
int dnmf_track_neurons(const float *frames, long ldf, const int *sz, int T, const int *times, const void *predict, int predict_f64,
                       int predict_per_frame, int K, double sigma, const int *search, double threshold, const float *background,
                       double *positions, float *amplitudes, float *peaks, dnmf_stream_t stream);

/* ---- K15c: chained neuron tracking -- K15's search, frame after frame ----------------------------------------------------
 * Every neuron k < K is carried from the anchor frame through the T frames by two independent chains: the forward one visits
 * the frames anchor, anchor + 1, ..., T - 1, the backward one anchor, anchor - 1, ..., 0 (it repeats the anchor search and
 * writes nothing for the anchor frame).  tests/follow_restatement.py is the definition in float64.  A chain starts with
 * last = start[k], vel = 0, n = 0, miss = 0 and does, per visited frame j:
 *   predict  pred = last + (momentum * vel) * n, float64, every operation rounded once in the order written (no fused
 *            multiply-add); predicted[k, :, j] = pred;
 *   search   K15's search of frame j around pred, unchanged: window, pick, refinement, amplitude and NaN rules;
 *   found    if n > 0: vel = (p^ - last) / n;  last = p^ (as stored: fp32 widened), n = 1, miss = 0; the row is written;
 *   missed   the row is NaN; n += 1, miss += 1; if miss > max_gap the chain is lost: lost_at[k, direction] = j, and every later
 *            frame of the chain gets NaN rows and a NaN predicted.
 * A start row that is not finite loses both chains before their first search: lost_at = anchor and every frame is NaN, predicted
 * included.  momentum = 0 searches around the last position found; momentum = 1 extrapolates the last step, which follows a
 * neuron that moves further per frame than the window is wide.  There is still no exclusion between neurons: a neuron within
 * about 2 sigma of a brighter one can be captured by it, and two chains may then follow the same blob.
 * frames, ldf, sz, times (T device row indices, NULL: 0..T-1; anchor counts slots of times), search, threshold, background: as
 * K15's.  start (K,3) fp64 on the device.  positions, predicted (K,3,T) fp64; amplitudes, peaks (K,T) fp32, either may be NULL;
 * lost_at (K,2) int, forward then backward, -1 for a chain that was never lost.  One launch of 2 K workgroups, one per (neuron,
 * direction), each of which walks its frames one after the other with its state in registers: the T steps of a chain are
 * sequential, so the call has the parallelism of 2 K workgroups only.  Every output element is written by exactly one
 * workgroup; no atomics, no host synchronisation, no workspace.  LDS as K15's.
 * DNMF_E_NULL: frames, sz, start, search, positions, predicted or lost_at NULL;  DNMF_E_SHAPE: K15's, anchor outside [0, T),
 * momentum outside [0, 1] or not finite, max_gap < 0;  DNMF_E_UNSUPPORTED: K15's.  Nothing is launched on an error. */
int dnmf_follow_neurons(const float *frames, long ldf, const int *sz, int T, const int *times, const double *start, int K, double sigma,
                        const int *search, int anchor, double momentum, int max_gap, double threshold, const float *background,
                        double *positions, float *amplitudes, float *peaks, double *predicted, int *lost_at, dnmf_stream_t stream);

/* ---- K15x: exclusive neuron tracking -- K15's search with the placed neighbours taken off -------------------------------------
 * K15 with exclusion between the neurons of a frame.  tests/track_exclusive_restatement.py is the definition in float64; all
 * arithmetic here is fp32.  Every frame j < T on its own; order[:, j] ((K,T) device ints, a permutation of 0..K-1 per frame) is
 * the sequence of its searches.  A placed neuron i is its latest result (p*_i, p^_i, a_i); its footprint is
 * a_i prod_d exp(-(x_d - p^_{i,d})^2 / sigma^2) at the voxels of the volume with |x_d - p*_{i,d}| <= r on every axis, 0 elsewhere.
 *   round 1   for k in order[:, j]: K15's search of (k, j) -- window around predict, pick, refinement, amplitude, threshold and
 *             NaN rules unchanged -- on frame_j - background_j - the footprints of the neurons placed so far in this frame.  A
 *             search with a result places k; one without leaves it unplaced, and it is never subtracted;
 *   rounds    2 .. rounds, the same order: k is searched again with all other placed neurons at their latest result taken off;
 *             the new result replaces the old one; without a result k's row becomes NaN and k is unplaced.
 * The outputs are those of the last round.  n_subtracted[k, j]: how many placed neighbours' +-r boxes met the region that (k, j)'s
 * last search staged (0 without a window).  A frame's K rounds searches depend on one another and run in sequence.  Chaining
 * on the frame before (K15c) with exclusion would need all K chains in lock-step per frame: not provided.
 * frames, ldf, sz, times, predict, predict_f64, predict_per_frame, sigma, search, threshold, background, positions, amplitudes,
 * peaks: as K15's.  order is not verified (it is device data): an entry outside [0, K) is skipped, and the rows of a neuron that
 * a frame's order leaves out are not written.  n_subtracted (K,T) int or NULL.  One launch of T workgroups, one per frame; the
 * placed list (9 words per neuron) and 16 neighbour tables lie in LDS beside K15's region: K <= 1024, and all of it within
 * 48 KiB.  The same input gives the same bits; no atomics, no host synchronisation, no workspace.
 * DNMF_E_NULL: frames, sz, predict, order, search or positions NULL;  DNMF_E_SHAPE: K15's, rounds < 1;  DNMF_E_UNSUPPORTED: K15's,
 * K > 1024, LDS over 48 KiB (the message names the parts).  Nothing is launched on an error. */
int dnmf_track_neurons_exclusive(const float *frames, long ldf, const int *sz, int T, const int *times, const void *predict, int predict_f64,
                                 int predict_per_frame, int K, const int *order, int rounds, double sigma, const int *search,
                                 double threshold, const float *background, double *positions, float *amplitudes, float *peaks,
                                 int *n_subtracted, dnmf_stream_t stream);

/* ---- K16: per-frame normal equations of the motion fit, and the Levenberg-Marquardt step -----------------------------------
 * The motion loss is a sum over frames and frame t only sees beta[:, :, t]: 30 unknowns (12 at Z == 1) against P residuals.
 * With r(v) = A_tC(v) - y(v) and g_d(v) = d A_tC / d q_d (v) exactly as K2 forms them (same warp, same taps, out-of-bounds
 * corners add zeros) and the CENTRED basis phi(v) = quadratic_basis(u(v)), u_d = 2 x_d / (S_d - 1) - 1 (0 on an axis of one
 * voxel), the Jacobian row of voxel v is J(v)[a,d] = phi_a(v) g_d(v) and, per frame b, with the parameter index a*3 + d:
 *   H (B,30,30) = sum_v J^T J    float64, symmetric, both triangles written
 *   g (B,30)    = sum_v J^T r    float64
 *   sse (B)     = sum_v r^2      float64
 * Sums run in fp32 inside a block and in float64 across the blocks of a frame.  At Z == 1 the unknowns with z in their basis
 * term or d == 2 get exact zeros.  accumulate != 0 adds to H, g, sse instead of overwriting them (colour channels are extra
 * voxels that share beta).  A frame whose beta has a non-finite entry is skipped: H and g get 0, sse NaN, nothing is gathered.
 * tests/gn_restatement.py is the definition in float64.
 *   S, lds, s_ids, frames, ldf, frame_ids, beta, T, times: as K2's (times must not contain duplicates; B <= 65535)
 *   workspace: dnmf_warp_normal_eqs_workspace(X,Y,Z,B) bytes
 * DNMF_E_NULL: a NULL buffer;  DNMF_E_SHAPE: a size, T or B < 1, B > 65535, lds or ldf below a row;  DNMF_E_UNSUPPORTED: a
 * volume beyond K2's 32-bit tap offsets;  DNMF_E_WORKSPACE: a short workspace. */
size_t dnmf_warp_normal_eqs_workspace(int X, int Y, int Z, int B);
int dnmf_warp_normal_eqs(const float *S, long lds, const int *s_ids, const float *frames, long ldf, const int *frame_ids,
                         int X, int Y, int Z, const float *beta, int T, const int *times, int B, double *H, double *g,
                         double *sse, int accumulate, void *workspace, size_t workspace_bytes, dnmf_stream_t stream);

/* One damped Gauss-Newton step per frame from K16's output at the trial coefficients, one wave per frame, float64, no host
 * synchronisation.  The trial coefficients of frame b are column times[b] of beta (10,3,T); the state of frame b is H_acc
 * (B,30,30), g_acc (B,30), sse_acc (B): the normal equations at the accepted coefficients beta_acc (B,30) ([a*3+d], fp32), the
 * damping lam (B), sse0 (B) (the first evaluation) and counts (B,3) = accepted steps, rejected steps, initialised; counts must
 * be zero before the first call, nothing else needs initialising.
 *   first call of a frame (counts[b,2] == 0): the trial is accepted unconditionally, lam = lam0, sse0 = sse;
 *   later: sse finite and < sse_acc -> accept (trial becomes the accepted state, lam = max(lam / nu, lam_min)),
 *          else reject (lam = min(lam nu, lam_max));
 *   then  (H_acc + lam diag(H_acc) + tiny I) delta = -g_acc on the active unknowns (all 30, at Z == 1 the 12 without z) with
 *          tiny = 1e-12 max_i H_ii + 1e-30, by a Cholesky factorisation of the system scaled to a unit diagonal (a pivot that is
 *          not positive and finite: delta = 0);  d beta[a,d] = sum_c M[a,c] delta[c,d] with M (10,10) row-major float64, the
 *          change of basis basis(u(v)) . gamma = basis(v) . (M gamma);  beta[:, :, times[b]] = fp32(beta_acc + d beta).
 *   accept_only != 0: the accept / reject bookkeeping, then beta[:, :, times[b]] = beta_acc (the best accepted coefficients).
 * H == 0 gives delta = 0; a NaN frame stays NaN and touches nothing else.
 * DNMF_E_NULL: a NULL buffer;  DNMF_E_SHAPE: B, Z or T < 1, nu <= 1, lam0 or lam_min <= 0, lam_max < lam_min. */
int dnmf_lm_step(const double *H, const double *g, const double *sse, int B, int Z, const double *M, float *beta, int T,
                 const int *times, double *H_acc, double *g_acc, double *sse_acc, double *sse0, double *lam, float *beta_acc,
                 int *counts, double nu, double lam0, double lam_min, double lam_max, int accept_only, dnmf_stream_t stream);

/* K16s: dnmf_lm_step with a temporal smoothness prior.  theta_t (30, [a*3+d]) are frame t's coefficients in the centred basis on
 * the active unknowns (beta[:, :, t] = M theta_t per coordinate; theta = Minv beta, Minv (10,10) row-major float64 = the inverse
 * of M on the active monomials, zeros on the others), and frame t minimises
 *   f_t(theta) = sse_t(theta) + m sum_{s in N_t} |theta - theta_s|^2,
 * N_t = the frames t - 1, t + 1 inside [0, T) whose column of beta_ref is finite.  beta_ref (10,3,T) fp32 holds every frame's
 * ACCEPTED coefficients; it is read at t +- 1, written at t on accept, and must not be beta (which holds untested trials).
 *   accept   first call: always.  Later: f_t(trial) finite and < f_t(accepted), both priors against the current beta_ref.
 *            On accept the trial's column is also written to beta_ref.  lam, sse0 and counts as dnmf_lm_step.
 *   step     H' = H_acc + m |N_t| I, g' = g_acc + m sum_s (theta_acc - theta_s) on the active unknowns, then dnmf_lm_step's
 *            damped solve of (H' + lam diag H' + tiny I) delta = -g' (the same device function) and d beta = M delta.
 *            H_acc == 0 gives a damped step to the neighbours' mean, not delta = 0.
 *   prior    (B) float64 out: m sum_s |theta_acc - theta_s|^2 of the accepted point after this call.  sse_acc and sse0 stay
 *            the data term alone.
 * m == 0, or a frame without a neighbour, is dnmf_lm_step exactly.  tests/gn_smooth_restatement.py is the definition.
 * CONTRACT: the frames of one launch are pairwise non-adjacent (|times[i] - times[j]| != 1; all of one parity is enough): a
 * block reads beta_ref[t +- 1] while the block of another frame may write its own column.  Nothing checks this on the device.
 * One wave per frame, float64, no host synchronisation, no workspace.
 * DNMF_E_NULL: a NULL buffer;  DNMF_E_SHAPE: as dnmf_lm_step, or m < 0 or not finite, or beta_ref == beta. */
int dnmf_lm_step_smooth(const double *H, const double *g, const double *sse, int B, int Z, const double *M, const double *Minv,
                        float *beta, int T, const int *times, double *H_acc, double *g_acc, double *sse_acc, double *sse0,
                        double *lam, float *beta_acc, int *counts, double nu, double lam0, double lam_min, double lam_max,
                        int accept_only, float *beta_ref, double m, double *prior, dnmf_stream_t stream);

/* K16o: the step for one warp order (csrc/motion_gn.hip, lm_step_order_kernel).  dnmf_lm_step's arguments, order after Z, and
 * dnmf_lm_step_smooth's Minv, beta_ref, m and prior.  The unknowns are the rows of the centred basis of degree <= order:
 *   order 0 (translation): row 0;  1 (affine): rows 0 .. 3;  2 (quadratic): all ten
 * -- 3, 12 or 30 unknowns; at Z == 1, where the z rows and the z component stay out, 2, 6 or 12.  H, g and sse are K16's, whole:
 * the restriction happens here, so one set of normal equations serves every order.  Over the selected unknowns everything is
 * as the two steps above have it over all of them: the damped system (its diagonal scaling and tiny from the restricted
 * block's own diagonal), accept / reject, the damping bounds, accept_only, a pivot that is not positive and finite, H == 0, a
 * NaN frame; and with m != 0 the prior, theta = Minv beta taken on the selected unknowns only in the accept test, in prior (B)
 * and in H' and g'.  M takes a centred term to raw rows of its degree or lower, so the rows of beta[:, :, times[b]] above the
 * order (1 .. 9 under order 0, 4 .. 9 under order 1) keep their bits.
 * m == 0: no prior; Minv, beta_ref and prior are not read and may be NULL, the frames need not be non-adjacent.  m != 0:
 * dnmf_lm_step_smooth's CONTRACT holds.  order == 2 takes dnmf_lm_step's steps (m == 0) or dnmf_lm_step_smooth's (m != 0), bit for
 * bit; those two stay the entries of the default path.  tests/gn_order_restatement.py is the definition.
 * DNMF_E_NULL: a NULL buffer (Minv, beta_ref, prior: only with m != 0);  DNMF_E_SHAPE: as dnmf_lm_step_smooth, or order outside
 * 0 .. 2. */
int dnmf_lm_step_order(const double *H, const double *g, const double *sse, int B, int Z, int order, const double *M,
                       const double *Minv, float *beta, int T, const int *times, double *H_acc, double *g_acc, double *sse_acc,
                       double *sse0, double *lam, float *beta_acc, int *counts, double nu, double lam0, double lam_min,
                       double lam_max, int accept_only, float *beta_ref, double m, double *prior, dnmf_stream_t stream);

/* K16j: the step with a volume-preserving prior (csrc/motion_gn.hip, lm_step_jac_kernel).  dnmf_lm_step_order's arguments, the
 * volume's X, Y, Z in place of Z, and mj, jac, min_det.  With theta a frame's coefficients in the centred basis on the active
 * unknowns, the frame's map is q_d(u) = sum_a basis_a(u) theta[a,d], basis(u) = [1, u0, u1, u2, u0^2, u1^2, u2^2, u0 u1, u0 u2,
 * u1 u2], and its Jacobian in voxel coordinates Jx[d][e] = (d q_d / d u_e) / h_e, h_e = (S_e - 1) / 2 -- 3 x 3, or 2 x 2 over (x, y)
 * at Z == 1.  This is the TRUE Jacobian of the model's map (K11 / K12's), not the reference's log_det_jac, which swaps the xz and
 * yz rows.  Sample points: the corners u in {-1, +1}^n in the order of counting with the first axis slowest, then the centre
 * u = 0: NP = 9, or 5 at Z == 1.
 *   rho_p    log det Jx(u_p): 0 for the identity, a rigid motion in voxel coordinates or a shear; +inf where det Jx(u_p) <= 0
 *            or is not finite.
 *   J        mj / NP sum_p rho_p^2, the frame's prior; +inf for a map that folds at a sample point.
 *   accept   first call: always.  Later: sse + temporal prior + J of the trial finite and below that of the accepted point
 *            (recomputed from beta_acc).  A trial that folds at a sample point is therefore never accepted after the first call,
 *            and an accepted point that folds is beaten by any admissible trial.
 *   step     H' gains mj / NP sum_p jrho_p jrho_p^T and g' gains mj / NP sum_p rho_p jrho_p at the point kept, on the unknowns
 *            of the order, jrho_p[a*3+d] = sum_e (Jx^-1)[e][d] (d basis_a / d u_e)(u_p) / h_e: the exact Gauss-Newton terms of
 *            the sum of squares J.  A point whose rho is not finite adds nothing.  rho itself sees the whole map, not the
 *            order's unknowns alone.  Then dnmf_lm_step's damped solve on the dense H' (the same device function).
 *   jac      (B) float64 out: J of the point kept.   min_det (B) float64 out: its smallest det Jx over the sample points.
 * det Jx is a cubic polynomial in u: positive at the sample points does not prove positive everywhere.
 * mj == 0: no such prior (jac = 0; min_det is still written), the steps of dnmf_lm_step_order up to the rounding of its sums.
 * m != 0: dnmf_lm_step_smooth's CONTRACT holds; m == 0: beta_ref and prior may be NULL.  Minv is always read.
 * Sums over p run in a fixed order, no atomics: the same input gives the same bits.  One wave per frame, float64, no host
 * synchronisation, no workspace.  tests/gn_jac_restatement.py is the definition.
 * DNMF_E_NULL: a NULL buffer (beta_ref, prior: only with m != 0);  DNMF_E_SHAPE: as dnmf_lm_step_order, X or Y < 2, mj < 0 or not
 * finite. */
int dnmf_lm_step_jac(const double *H, const double *g, const double *sse, int B, int X, int Y, int Z, int order, const double *M,
                     const double *Minv, float *beta, int T, const int *times, double *H_acc, double *g_acc, double *sse_acc,
                     double *sse0, double *lam, float *beta_acc, int *counts, double nu, double lam0, double lam_min,
                     double lam_max, int accept_only, float *beta_ref, double m, double *prior, double mj, double *jac,
                     double *min_det, dnmf_stream_t stream);

/* ---- K17: the trilinear registered movie under the fitted warp ----------------------------------------------------------------
 * For every frame j < B (column t = times[j] of beta, or j when times is NULL; row frame_ids[j] of frames, or j) and every lattice
 * point u = (i, j, k) of the footprint volume: the x with q_t(x) = u, and the frame sampled trilinearly at x.  Conventions as K11 /
 * K12: q_t(x) = basis(x) . beta[:, :, t] in voxel indices, the true Jacobian.  tests/pullback_restatement.py is the definition in
 * float64.  An EXTENSION, not a parity path: true voxel coordinates throughout, none of the sz-for-(sz - 1) scaling K7 keeps from
 * the reference's spatial_pushforward.
 *   solve    Newton from x = u; an axis of extent 1 is inactive (its coordinate stays 0, its equation is dropped: K2's Z == 1).
 *            The definition stops at a step below 1e-6 in every coordinate, 32 steps at most; the kernel iterates in fp32 on the
 *            displacement x - u and stops at a step below 1e-4 (relative to |x - u| beyond 32 voxels).  Contract: x is within 1e-3
 *            voxel of the definition's wherever that converges with |det J| >= 0.5, at extents up to 512.  A point is BAD when
 *            |det J| < 1e-12, an iterate is not finite or the steps run out; so is every point of a frame whose t is outside [0, T).
 *   sample   sum over the 8 taps (4 at Z == 1) of w Y[tap], weights from floor(x) and x - floor(x); a tap outside the volume
 *            contributes 0 (grid_sample, zeros, align_corners=True: the model's own forward), NaN voxels propagate as IEEE gives
 *            them.  At the identity and at an integer translation inside the volume the output equals the input bit for bit.
 *   fill     fill_mode 0: the zero padding above, bad points 0;  1: fill_value (NaN, say) at every point whose x lies outside
 *            [0, S_d - 1] on an active axis, and at bad points.
 * Frame row b holds nchan channels that share the warp, channel c at frames[row + c ldc_in] and at out[b ldo + c ldc_out]: one
 * solve per lattice point serves them all (nchan == 1: ldc_in, ldc_out unused).  coords: NULL or (B,P,3) fp32, the x of every
 * point (NaN where bad).  bad_count: NULL or one int64 INCREMENTED by the bad points of the call (per lattice point, not per
 * channel).  One launch, no workspace, no host synchronisation.
 * DNMF_E_NULL: frames, beta or out NULL;  DNMF_E_SHAPE: a size or T < 1, B < 0, B > T without times, nchan < 1, fill_mode not 0 / 1,
 * ldc_in or ldc_out < P, ldf < (nchan-1) ldc_in + P, ldo < (nchan-1) ldc_out + P;  DNMF_E_UNSUPPORTED: 2^31 voxels or more, B > 65535
 * (frames ride on gridDim.y: split the call). */
int dnmf_warp_pullback(const float *frames, long ldf, long ldc_in, int nchan, const int *frame_ids, int X, int Y, int Z,
                       const float *beta, int T, const int *times, int B, float *out, long ldo, long ldc_out, int fill_mode,
                       float fill_value, float *coords, long long *bad_count, dnmf_stream_t stream);

/* ---- K18: summary images of a video: mean, std, max over time and the local correlation image -----------------------------
 * For B frames x[t, p] of a volume (X, Y, Z) (rows of ldf >= P floats, voxel p = (x Y + y) Z + z; row frame_ids[j] of frames, or j,
 * for the j-th frame of the call) and, with sub, x = frames - sub rounded to fp32 (row j of sub, lds >= P floats: the result equals,
 * bit for bit, the call on explicitly subtracted rows).  tests/summary_restatement.py is the definition in float64.  Per voxel,
 * over every frame since the state was reset:
 *   mean, std (population, ddof = 0), max;
 *   corr     the mean, over the valid neighbours q of p, of the Pearson correlation of the two time series.  DNMF_NEIGHBOURS_FACE:
 *            the voxels that differ by 1 on one axis (6; 4 at Z == 1), DNMF_NEIGHBOURS_FULL: by at most 1 on every axis (26; 8).
 *            No padding and no wrap: a neighbour outside the volume does not exist, an axis of one voxel has none.  A pair is valid
 *            when both voxels are finite in every frame and both variances are > 0; a voxel without a valid pair gets NaN.
 *   A voxel with a sample that is not finite is NaN in all four images and is nobody's neighbour.
 * One pass in float64 on d = x - x0, x0 the voxel's value in the first frame after the reset (exact in float64, so a constant voxel
 * has a variance of exactly 0): sum d, sum d^2 and sum d_p d_q for the half-set of directions (13 full, 3 face; 4 and 2 at Z == 1);
 * var = max(0, (sum d^2 - (sum d)^2 / T) / T).  A workgroup owns a tile of voxels (staged with a one-voxel halo in LDS) and a
 * segment of frames (segment > 0: that many frames each; 0: the kernel's choice, enough segments to fill the machine); a second
 * launch adds the segments to the state in a fixed order -- no floating-point atomics, the same input gives the same bits.
 *   state    caller-owned, 8-byte aligned, dnmf_summary_images_workspace(sz, neighbours, B, segment) bytes (0 on bad arguments; it
 *            does not decrease with B, so the size for the largest call serves every call): the frame count, the sums, the max, the
 *            pivot x0, and the partial sums of the segments of one call.  first != 0 resets it; a movie larger than one buffer is
 *            fed in several calls with the same sz and neighbours.
 *   finish   != 0: a third launch writes images (4, P) float64: mean, std, max, corr.
 * No host synchronisation: the frame count lives in the state.
 * DNMF_E_NULL: frames, sz or state NULL, images NULL with finish;  DNMF_E_SHAPE: a size or B < 1, an unknown neighbourhood,
 * segment < 0, ldf or lds < P;  DNMF_E_UNSUPPORTED: 2^31 voxels or more, Z > 137 (LDS), more than 65535 segments;
 * DNMF_E_WORKSPACE: a short or misaligned state.  Nothing is launched on an error. */
#define DNMF_NEIGHBOURS_FACE 0
#define DNMF_NEIGHBOURS_FULL 1
size_t dnmf_summary_images_workspace(const int *sz, int neighbours, int B, int segment);
int dnmf_summary_images(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const int *sz, int B,
                        int neighbours, int first, int finish, int segment, void *state, size_t state_bytes, double *images,
                        dnmf_stream_t stream);

/* ---- K19: a rank-1 background b (x) f on the residual, fitted by alternating exact coordinate steps, and its subtraction --------
 * Model: frames[t, p] ~ sub[t, p] + b[p] f[t] with b >= 0 an image over the P voxels and f >= 0 one value per frame; sub is what the
 * model already predicts (NULL: nothing).  r = (double)frames - (double)sub is exact and is never written: the two half-steps read
 * the movie once each (8 B per voxel and frame with sub, 4 B without), in float64, without floating-point atomics -- the same input
 * at the same addresses gives the same bits.  tests/background_restatement.py is the definition in float64.  Rows as in K18: ldf >= P
 * floats, row frame_ids[j] of frames (or j) for the j-th frame of the call, row j of sub (lds >= P).  Rows whose start is 16-byte
 * aligned are read 16 bytes at a time, others (P % 4 != 0) float by float.  Frames, sub, b and f must be finite: a value that is not
 * poisons the sums it enters, nothing detects it.  No host synchronisation; nothing is launched on an error.
 *
 * dnmf_background_dots: num[j] = sum_p b[p] r[j, p] (float64, B values, may be NULL), *bb = sum_p b[p]^2 (float64, once per call,
 *   may be NULL) and f[j] = (float)(max(0, num[j]) / bb), 0 when bb == 0 (B values).  One workgroup per (frame, segment of voxels),
 *   float64 sums per lane reduced in a fixed tree, one partial per workgroup in the workspace; a second launch adds a frame's
 *   partials in their order.  workspace: caller-owned, 8-byte aligned, dnmf_background_dots_workspace(P, B) bytes (0 on bad arguments).
 *   DNMF_E_NULL: frames, b, f or workspace NULL;  DNMF_E_SHAPE: P or B < 1, ldf or lds < P;  DNMF_E_UNSUPPORTED: 2^31 voxels or more;
 *   DNMF_E_WORKSPACE: a short or misaligned workspace.
 *
 * dnmf_background_accum: per voxel num[p] = sum_t f[t] r[t, p] over every frame since the state was reset (f[j] belongs to the j-th
 *   frame of the call), ff = sum_t f[t]^2, and with finish != 0 a last launch writes b[p] = (float)(max(0, num[p]) / ff), 0 when
 *   ff == 0 (P values), num (P float64, may be NULL) and *ff (may be NULL).  One workgroup per (tile of 1024 contiguous voxels, segment
 *   of frames; segment > 0: that many frames each, 0: the kernel's choice, enough segments to fill the machine), float64 sums in
 *   registers, the partial sums of a segment in the state; a second launch adds the segments to the state in their order.
 *   state: caller-owned, 8-byte aligned, dnmf_background_accum_workspace(P, B, segment) bytes (0 on bad arguments; it does not
 *   decrease with B, so the size for the largest call serves every call).  first != 0 resets it; a movie larger than one buffer is fed
 *   in several calls and gives the result of one call up to the order of the sums.
 *   DNMF_E_NULL: frames, f or state NULL, b NULL with finish;  DNMF_E_SHAPE: P or B < 1, segment < 0, ldf or lds < P;
 *   DNMF_E_UNSUPPORTED: 2^31 voxels or more, more than 65535 segments;  DNMF_E_WORKSPACE: a short or misaligned state.
 *
 * dnmf_background_subtract: out[j, p] = fmaf(-b[p], f[t], frames[row, p]) in fp32 (one rounding), max(., 0) when clamp != 0;
 *   t = times[j] or j, f has nf values (a t outside [0, nf) makes row j NaN).  out: B rows of ldo >= P floats; out == frames (in
 *   place) is allowed with frame_ids NULL and ldo == ldf, any other overlap is not.  One launch, no workspace.
 *   DNMF_E_NULL: frames, b, f or out NULL;  DNMF_E_SHAPE: P, B or nf < 1, ldf or ldo < P, B > nf without times, out == frames with
 *   frame_ids or ldo != ldf;  DNMF_E_UNSUPPORTED: 2^31 voxels or more, 2^31 workgroups or more (split the call). */
size_t dnmf_background_dots_workspace(long P, int B);
int dnmf_background_dots(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *b, long P, int B,
                         double *num, double *bb, float *f, void *workspace, size_t workspace_bytes, dnmf_stream_t stream);
size_t dnmf_background_accum_workspace(long P, int B, int segment);
int dnmf_background_accum(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *f, long P, int B,
                          int first, int finish, int segment, void *state, size_t state_bytes, float *b, double *num, double *ff,
                          dnmf_stream_t stream);
int dnmf_background_subtract(const float *frames, long ldf, const int *frame_ids, const float *b, const float *f, int nf, const int *times,
                             long P, int B, float *out, long ldo, int clamp, dnmf_stream_t stream);

/* ---- K23: a rank-R background sum_c b_c (x) f_c on the residual, 2 <= R <= 8 ---------------------------------------------------------
 * Model: frames[t, p] ~ sub[t, p] + sum_{c < R} b_c[p] f_c[t], b_c >= 0, f_c >= 0; r, rows, frame_ids, sub, the alignment rule, the
 * finiteness rule and the error codes as in K19.  b: R rows of ldb >= P floats; f: R rows of ldf_t floats (>= B, the frames of the
 * call; >= nf for subtract).  tests/background_rank_restatement.py is the definition in float64.  A half-step is one pass over the
 * movie whatever R is (8 B per voxel and frame with sub, 4 B without): the pass leaves R float64 sums per frame (per voxel), a small
 * launch the R x R Gram matrix of the factor held fixed, and the last launch solves every frame's (voxel's) non-negative problem
 *     min over x >= 0 of x^T G x - 2 N^T x      by `inner` >= 1 cyclic sweeps  x_j <- max(0, (N_j - sum_{i != j} G_ji x_i) / G_jj),
 * j = 0 .. R-1, 0 where G_jj == 0, in float64 from the current value (the f or b passed in), rounded once to fp32.  `inner` is a
 * parameter of the algorithm, not a tolerance.  R is a template parameter of the kernels (the R, or 4 R, sums of a lane are registers).
 * Float64 sums in a fixed order, no floating-point atomics: the same input at the same addresses gives the same bits.  No host
 * synchronisation; nothing is launched on an error.
 *
 * dnmf_background_dots_rank: num[c * B + j] = sum_p b_c[p] r[j, p] ((R, B) float64, may be NULL), q = B^T B ((R, R) float64, may be
 *   NULL), and f[c * ldf_t + j] is read as the start of frame j's solve and overwritten with its result.  One workgroup per (frame,
 *   segment of voxels) as in K19 with R sums a lane (the rows of b are read again for every frame, from cache); the Gram launch has
 *   one workgroup per 4096 voxels.  workspace: caller-owned, 8-byte aligned, dnmf_background_dots_rank_workspace(P, B, R) bytes.
 *
 * dnmf_background_accum_rank: per voxel num[c * P + p] = sum_t f_c[t] r[t, p] over every frame since the state was reset, W = F F^T
 *   over the same frames, and with finish != 0 b[c * ldb + p] is read as the start of voxel p's solve and overwritten with its result;
 *   num ((R, P) float64) and w ((R, R) float64) may be NULL.  Tiles, segments, first / finish / segment and the state as in K19, with
 *   4 R sums a lane; state: dnmf_background_accum_rank_workspace(P, B, R, segment) bytes (it does not decrease with B); every call on
 *   one state has the same P and R.
 *
 * dnmf_background_subtract_rank: out[j, p] = (float)((double)frames[row, p] - sum_c (double)b_c[p] (double)f_c[t]), the products
 *   added one by one with c ascending, max(., 0) when clamp != 0; t, nf, the NaN row, in-place use and the codes as in K19.
 *
 * DNMF_E_UNSUPPORTED: R outside 2 .. 8 (one component is K19's entry), and K19's cases;  DNMF_E_SHAPE: inner < 1, ldb < P, ldf_t < B
 * (subtract: < nf), and K19's cases;  DNMF_E_NULL, DNMF_E_WORKSPACE as in K19. */
size_t dnmf_background_dots_rank_workspace(long P, int B, int R);
int dnmf_background_dots_rank(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *b, long ldb, int R,
                              long P, int B, int inner, float *f, long ldf_t, double *num, double *q, void *workspace, size_t workspace_bytes,
                              dnmf_stream_t stream);
size_t dnmf_background_accum_rank_workspace(long P, int B, int R, int segment);
int dnmf_background_accum_rank(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const float *f, long ldf_t, int R,
                               long P, int B, int first, int finish, int segment, int inner, void *state, size_t state_bytes, float *b, long ldb,
                               double *num, double *w, dnmf_stream_t stream);
int dnmf_background_subtract_rank(const float *frames, long ldf, const int *frame_ids, const float *b, long ldb, const float *f, long ldf_t, int R,
                                  int nf, const int *times, long P, int B, float *out, long ldo, int clamp, dnmf_stream_t stream);

/* ---- K20: trace clean-up: mask, single-frame outliers, bleach detrend, dF/F0, gap filling, smoothing, rescale ---------------------
 * tests/traces_restatement.py (clean_traces) is the definition, step by step (S1 .. S6), in float64; this entry computes it for K
 * traces of T frames: traces = K rows of ldt >= T floats, out = K rows of ldo >= T floats (the input is only read; out may not
 * overlap it).  One workgroup per trace with the working trace as float64 in LDS, every output rounded once to fp32; three launches
 * on the stream (per trace; one workgroup for what couples the traces, modes 1 and 3 only; per trace), no host synchronisation,
 * nothing launched on an error.  Sums are taken in a fixed order without floating-point atomics: the same input gives the same bits.
 * Medians and the percentile select by bisection on the 64-bit key of a value (one counting pass per key bit), never by sorting.
 *   fps               frames per second (> 0): S1 masks the first floor(fps / 2 + 0.5) frames and the last one when trim != 0; the
 *                     running median of S3 spans W = floor(10 fps + 0.5) frames
 *   sigma_threshold   S2 (outliers and the median of three) runs when > 0
 *   detrend_mode      0 none, 1 one curve for all traces, 2 one per trace, 3 one per trace and the division by max(median F0, 1)
 *   interp            0 none, 1 linear (S4);  smooth: 0 none, 1 movmean, 2 movmedian over smooth_window >= 1 frames (S5)
 *   floor_value       S1 masks values <= floor_value (and every value that is not finite)
 * Outputs, K values each: scales, offsets (out = 0.9 (x - offset) / scale + 0.05 of the detrended x for modes 0 .. 2; mode 3:
 * scale = max(median F0, 1), offset 0), a, b (the fitted curve a exp(b (t + 1)); NaN where none was fitted; mode 1: the common one),
 * F0 (NaN for mode 0; mode 3: the common median), fitted (0 / 1), n_outliers (frames S2 removed).
 * workspace: caller-owned, 8-byte aligned, dnmf_clean_traces_workspace(K, T) bytes (0 on bad arguments): the trace after S2 and its
 * running median, float64.  T and K are limited by the LDS: at most 18 432 each; larger ones are refused, nothing is truncated.
 * DNMF_E_NULL: any pointer NULL;  DNMF_E_SHAPE: K or T < 1, ldt or ldo < T, fps <= 0 or W < 1 with detrend_mode > 0,
 * sigma_threshold < 0, a floor_value that is not finite, detrend_mode, interp or smooth outside their values, smooth_window < 1 with
 * smooth;  DNMF_E_UNSUPPORTED: T or K above 18 432;  DNMF_E_WORKSPACE: a short or misaligned workspace. */
size_t dnmf_clean_traces_workspace(int K, int T);
int dnmf_clean_traces(const float *traces, long ldt, int K, int T, double fps, double sigma_threshold, int detrend_mode, int interp,
                      int smooth, int smooth_window, int trim, double floor_value, float *out, long ldo, double *scales, double *offsets,
                      double *a, double *b, double *F0, int *fitted, int *n_outliers, void *workspace, size_t workspace_bytes,
                      dnmf_stream_t stream);

/* ---- K21: spike deconvolution of the traces: AR(1), non-negative ---------------------------------------------------------------------
 * tests/deconv_restatement.py (deconvolve_traces) is the definition (D1 .. D6), in float64; this entry computes it for K traces of T
 * frames: traces = K rows of ldt >= T floats, c and s = K rows of ldo >= T floats each (the input is only read; the outputs may
 * not overlap it).  Per trace y, with w_t = 1 where y_t is finite and 0 elsewhere, c >= 0 minimises
 *     1/2 sum_t w_t (y_t - b - c_t)^2 + lam sum_t s_t,   s_0 = c_0,  s_t = c_t - g c_{t-1} >= 0:
 * c is the denoised calcium trace, s the spikes.  With x_t = c_t g^-t this is a weighted isotonic regression; it is solved exactly
 * by pool-adjacent-violators, every lane on a segment of its own, then a stitch of the segments.  One launch, one workgroup per
 * trace, float64 inside, c and s rounded once to fp32, no host synchronisation, nothing launched on an error.  Sums are taken in a
 * fixed order without floating-point atomics: the same input gives the same bits.
 *   g, penalty, baseline, noise   K doubles each on the device, or NULL; NULL or a NaN entry means "estimate" for that trace:
 *                     g = ac(2) / ac(1) of the autocovariances over the valid pairs (D3); baseline = the baseline_percentile-th
 *                     percentile (hazen) of the valid frames (D4); noise = 1.4826 MAD / sqrt(2) of the differences of adjacent valid
 *                     frames (D2); penalty = the lam at which the residual sum of squares reaches noise^2 n_valid, bracketed by at most
 *                     64 doublings from noise and 32 halvings, inside the kernel (D5)
 *   info              K rows of 8 doubles: g, penalty, baseline, noise, RSS, n_valid, number of pools, ok (1 / 0)
 * A trace is refused (ok = 0, its rows of c and s and the first five entries of info NaN) with fewer than 4 valid frames, with fewer
 * than 2 adjacent valid pairs when the noise or g must be estimated, with ac(1) <= 0 or g outside (0, 1), with a given penalty < 0 or
 * a given baseline that is not finite (D6).
 * workspace: caller-owned, 8-byte aligned, dnmf_deconvolve_traces_workspace(K, T) bytes (0 on bad arguments): the pool records of
 * traces of more than 6144 frames (24 bytes a frame; shorter traces keep them in LDS).  T and K: at most 18 432 each (what
 * dnmf_clean_traces accepts); larger ones are refused, nothing is truncated.
 * DNMF_E_NULL: traces, c, s, info or workspace NULL;  DNMF_E_SHAPE: K or T < 1, ldt or ldo < T, baseline_percentile outside
 * [0, 100];  DNMF_E_UNSUPPORTED: T or K above 18 432;  DNMF_E_WORKSPACE: a short or misaligned workspace. */
size_t dnmf_deconvolve_traces_workspace(int K, int T);
int dnmf_deconvolve_traces(const float *traces, long ldt, int K, int T, const double *g, const double *penalty, const double *baseline,
                           const double *noise, double baseline_percentile, float *c, float *s, long ldo, double *info, void *workspace,
                           size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K32: AR(1)-constrained trace update: one row step of block coordinate descent per listed neuron ------------------------------------
 * tests/ar1_restatement.py (row_terms, row_step) is the definition, in float64.  On the Gram data G (T,K,K), r (T,K) of T consecutive
 * frames in time order and the float64 state C (K rows of ldc >= T doubles), for every listed neuron k = ids[i], i < n_ids, row k is
 * replaced by the exact minimiser over that row, the other rows fixed, of
 *     F(C) = sum_t (1/2 c_t^T G_t c_t - r_t^T c_t) + sum_k penalty_k sum_t s_kt,   x = C[k,:] - baseline_k,
 *     s_k0 = x_0 >= 0,  s_kt = x_t - g_k x_{t-1} >= 0:
 * with w_t = G_t[k,k] and y_t = C[k,t] + (r_t[k] - sum_l G_t[k,l] C[l,t]) / w_t (the sum over the columns nbr lists for row k, in
 * the order of the list, entries outside [0, K) skipped; without nbr over all columns ascending) the row becomes baseline_k plus the
 * minimiser of 1/2 sum_t w_t (y_t - baseline_k - x_t)^2 + penalty_k sum_t s_t -- K21's problem with the weight w_t where K21 has 1,
 * solved the same way (per-lane pool-adjacent-violators, a stitch, the expansion).  A frame whose w_t is not finite or <= 0, or
 * whose y_t is not finite, carries no weight: the trace decays through it.  g_k = 0: the plain coordinate step
 * max(0, y_t - baseline_k - penalty_k / w_t) + baseline_k, 0 + baseline_k on a frame without weight.
 * The listed neurons must share no Gram entry (one colour of the overlap graph): their steps then do not see each other and one
 * launch runs them side by side, one workgroup each.  A list must name row k itself where G_t[k,k] != 0.
 *   g, penalty, baseline   K doubles each on the device: g in [0, 1), penalty >= 0, baseline finite (the caller's to ensure)
 *   s                      K rows of lds >= T doubles: row k receives the spikes s_kt of the new row
 *   counts                 K rows of 2 ints: row k receives the number of pools (T with g_k = 0) and of frames without weight
 * Rows that are not listed are only read.  Float64 inside, sums in a fixed order without floating-point atomics: the same input
 * gives the same bits.  One launch, no host synchronisation, nothing launched on an error.
 * DNMF_E_NULL: any pointer but nbr NULL;  DNMF_E_SHAPE: K, T or n_ids < 1, n_ids > K, ldc or lds < T, NN < 1 with nbr;
 * DNMF_E_UNSUPPORTED: T above 6144 (24 bytes of pool record a frame, in LDS) or K above 4096: refused, nothing is truncated. */
int dnmf_ar1_temporal_step(const float *G, const float *r, double *C, long ldc, int K, int T, const int *ids, int n_ids,
                           const double *g, const double *penalty, const double *baseline, const int *nbr, int NN, double *s,
                           long lds, int *counts, dnmf_stream_t stream);

/* ---- K22: spatial high-pass of every frame (the filter MotionCorrect's gSig_filt registers on) -----------------------------------------
 * For B frames of a volume (X, Y, Z) (rows of ldf >= P floats, voxel p = (x Y + y) Z + z; row frame_ids[b] of frames, or b) and an
 * (n, n) array of fp32 taps on the device, n odd, h = n / 2:
 *     out[b, x, y, z] = sum over i, j with taps[i, j] != 0 of taps[i, j] * in[b, r_X(x + i - h), r_Y(y + j - h), z],
 * r_N the reflection with period 2 N (m = p mod 2 N; m if m < N, else 2 N - 1 - m): cv2.filter2D with BORDER_REFLECT, slice by slice,
 * as high_pass_filter_space (reference MotionCorrect.py:1262-1270) applies it.  An extent shorter than h (several bounces) and an
 * extent of 1 are valid.  Taps that are zero are not applied, so a NaN spreads over the support of the taps only.
 * tests/high_pass_restatement.py is the definition in float64.  fp32 fused multiply-adds in a fixed order (j ascending, then i
 * ascending), no atomics: the same input gives the same bits.  One launch, no workspace, no host synchronisation.
 *   out      B rows of ldo >= P floats (floats beyond P are left alone); it may not overlap the rows read.
 * DNMF_E_NULL: frames, sz, taps or out NULL;  DNMF_E_SHAPE: a size, B or n < 1, an even n, ldf or ldo < P;  DNMF_E_UNSUPPORTED: n > 31
 * (gSig > 10), 2^31 voxels or more.  Nothing is launched on an error. */
int dnmf_high_pass_frames(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, const float *taps, int n,
                          float *out, long ldo, dnmf_stream_t stream);

/* ---- K24: per-component statistics on the registered movie: does a fitted component explain anything? --------------------------------
 * For K neurons and B frames of a volume (X, Y, Z) (rows of ldf >= P floats, voxel p = (x Y + y) Z + z; row frame_ids[j] of frames, or
 * j, for the j-th frame of the call; row j of sub, lds >= P floats, or NULL: nothing is subtracted), everything in the coordinates of
 * the footprints.  Neuron k has a box boxes[k] = (x0, x1, y0, y1, z0, z1), inclusive (the layout of dnmf_pack_footprints_lists' bbox),
 * of n voxels u in the order x slowest, z fastest, and the footprint values a(u) = A[k lda + u] (K rows of lda >= P floats).  With
 *     e_t(u) = ((double)frames_t(u) - (double)sub_t(u)) + (double)a(u) (double)C[k ldc + j]
 * -- the residual with the neuron's own contribution put back; C (K rows of ldc >= B floats) in the call's frame order:
 *   sums        (K, B, 3) float64: sum e, sum e^2, sum a e over the box;
 *   foot        (K, 3) float64: n, sum a, sum a^2;
 *   frame_corr  (K, B) float64: Pearson of a and e_t on the box, (n sum ae - sum a sum e) / sqrt((n sum a^2 - (sum a)^2)(n sum e^2 -
 *               (sum e)^2));
 *   raw         (K, B) float64: (n sum ae - sum a sum e) / (n sum a^2 - (sum a)^2), the least-squares amplitude of a in e_t with a free
 *               offset -- the neuron's raw trace;  both NaN where a variance is not positive;
 *   image       (K, ldi >= the largest n) float64: sum_t w[k, t] e_t(u) / sum_t w[k, t] over every frame since the state was reset, w (K
 *               rows of ldw >= B floats) >= 0 and finite; NaN past a box's n and where the weights sum to 0;
 *   r_values    (K) float64: Pearson of a and image[k] on the box; NaN where the weights sum to 0 or a variance is not positive.
 * tests/components_restatement.py is the definition in float64.  An (k, t) whose box holds a sample that is not finite is invalid: its
 * three sums, frame_corr and raw are NaN and it takes no part in image[k], as if its weight were 0.  The test is on e_t: a C[k, t] or
 * a footprint value on the box that is not finite makes the (k, t) invalid in the same way.  w is the caller's to keep >= 0 and
 * finite: it is not checked, and a weight that is not finite makes image[k] and r_values[k] NaN or meaningless.
 * One workgroup per (neuron, segment of frames) -- segment > 0: that many frames each; 0: the kernel's choice, enough segments to fill
 * the machine; a lane keeps its voxels' footprint values and float64 image sums in registers for the whole segment.  The per-frame
 * sums are reduced across the lanes in a fixed order; a second launch adds the segments of a neuron in their order and forms foot,
 * frame_corr, raw and, with finish, image and r_values.  No floating-point atomics: the same input gives the same bits.
 *   boxes      (K, 6) int32 on the HOST: checked before anything is launched, and the size of the largest box sizes the state;
 *   boxes_dev  the same (K, 6) int32 on the device: what the kernels read;
 *   state      caller-owned, 8-byte aligned, dnmf_component_stats_workspace(sz, boxes, K, B, segment) bytes (0 on bad arguments; it
 *              does not decrease with B): the weight sums, the image sums and the partial sums of the segments of one call.  first != 0
 *              resets it; a movie larger than one buffer is fed in several calls with the same sz, boxes and A.  The per-frame outputs
 *              (sums, frame_corr, raw) belong to the call; foot is written by every call.
 *   finish     != 0: the second launch also writes image and r_values.
 * No host synchronisation.
 * DNMF_E_NULL: a NULL buffer (sub and frame_ids may be; image and r_values without finish);  DNMF_E_SHAPE: a size, K or B < 1,
 * segment < 0, a box that is empty or reaches outside the volume, ldf, lds or lda < P, ldc or ldw < B, ldi below the largest box;
 * DNMF_E_UNSUPPORTED: a box of more than 4096 voxels (K13's limit: 16 voxels a lane), 2^31 voxels or more, more than 65535 segments;
 * DNMF_E_WORKSPACE: a short or misaligned state.  Nothing is launched on an error. */
size_t dnmf_component_stats_workspace(const int *sz, const int *boxes, int K, int B, int segment);
int dnmf_component_stats(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const int *sz, int B,
                         const float *A, long lda, const int *boxes, const int *boxes_dev, int K, const float *C, long ldc,
                         const float *w, long ldw, int first, int finish, int segment, void *state, size_t state_bytes,
                         double *sums, double *foot, double *frame_corr, double *raw, double *image, long ldi, double *r_values,
                         dnmf_stream_t stream);

/* ---- K25: histogram_match: the affine map that carries a moving trace's quantiles onto a reference trace's ---------------------------
 * tests/histmatch_restatement.py (histogram_match) is the definition (H1 .. H5), in float64; this entry computes it for K rows:
 * a = K rows of lda >= Ta floats (the moving traces), b = K rows of ldb >= Tb floats, or ONE row shared by every row of a when
 * ldb = 0 (the reference traces), out = K rows of ldo >= Ta floats (the inputs are only read; out may not overlap them).  Per row:
 *   H1  the valid samples of a, and separately of b, are the finite ones (na, nb of them); a and b need no frame-to-frame
 *       correspondence: lengths and masks may differ;
 *   H2  nbins quantiles of each, qa and qb, at the exact rational indices j (n - 1) / (nbins - 1) of the sorted valid samples, linearly
 *       interpolated -- np.quantile(x, np.linspace(0, 1, nbins)) with the two samples picked by integer arithmetic;
 *   H3  beta = the least-squares fit of qb on [qa, 1], centred (a constant moving trace: beta0 = 0, beta1 = mean qb); with nonneg = 1
 *       the exact minimiser under beta0 >= 0 and beta1 >= 0 (what nnls on that design returns): the free solution where it is
 *       feasible, else the better of the two boundary solutions;
 *   H4  out_t = a_t beta0 + beta1, NaN where a_t is not finite;
 *   H5  distance = sqrt(mean_j (beta0 qa_j + beta1 - qb_j)^2), the RMS mismatch of the matched quantiles.
 * Two deviations from the reference's Demix/Traces.py::histogram_match, both stated in the restatement: H1 drops +-inf as well as
 * NaN (one infinite sample would make every fit NaN), and H5 computes the distance the reference declares but returns as NaN.
 * One launch, one workgroup per row, float64 inside, out rounded once to fp32, no workspace, no host synchronisation, nothing launched
 * on an error.  A row's samples are sorted as 64-bit keys in LDS (a bitonic network, csrc/block_ops.hpp: block_sort_keys), after
 * which every quantile is two reads; sums are taken in a fixed order without floating-point atomics: the same input gives the same
 * bits.
 *   nonneg     0: 'regular', 1: 'non-negative'
 *   beta       (K, 2) doubles: beta0 (scale), beta1 (offset);  distance: K doubles
 *   info       (K, 3) int32: na, nb, ok.  A row with na = 0 or nb = 0 is refused: ok = 0, beta, distance and its row of out NaN
 *   qa, qb     (K, nbins) doubles each, or NULL: the quantiles (NaN for a side without a valid sample)
 * Limits, set by the LDS (8 bytes a key up to the next power of two, 16 bytes a bin: 144 of the CU's 160 KiB at the limits): Ta and Tb
 * at most 16 384, nbins at most 1024, K at most 18 432; larger ones are refused, nothing is truncated.
 * DNMF_E_NULL: a, b, out, beta, distance or info NULL;  DNMF_E_SHAPE: K, Ta or Tb < 1, nbins < 2, nonneg outside {0, 1}, lda or ldo
 * < Ta, ldb neither 0 nor >= Tb;  DNMF_E_UNSUPPORTED: above the limits. */
int dnmf_histogram_match(const float *a, long lda, int Ta, const float *b, long ldb, int Tb, int K, int nbins, int nonneg, float *out,
                         long ldo, double *beta, double *distance, int *info, double *qa, double *qb, dnmf_stream_t stream);

/* ---- K26: merging duplicate components: the statistics of pairs of components, and the merged model (csrc/merge_components.hip) ------
 * tests/merge_restatement.py is the definition in float64.  Two components that sit on one cell overlap in space and are correlated
 * in time; dnmf_component_pairs measures both for N listed pairs, the host decides the groups and their coefficients (ops.merge_plan:
 * K is small), and dnmf_merge_apply writes the merged model.
 *
 * dnmf_component_pairs.  A = K rows of lda >= P floats, the footprints as rows (voxel p = (x Y + y) Z + z), boxes (K, 6) int32 =
 * (x0, x1, y0, y1, z0, z1) inclusive, as in K24; C = K rows of ldc >= T floats, the traces, NaN or inf allowed; pairs (N, 2) int32,
 * (i, j) in any order, i == j allowed.  Per pair, out[p] = 8 doubles:
 *   saa                     sum a_i a_j over the intersection of the two boxes, 0 where it is empty ((k, k): sum a_k^2 on the box);
 *   n                       the frames where both traces are finite; t0 the first of them;
 *   si, sj, sii, sjj, sij   sum d_i, d_j, d_i^2, d_j^2, d_i d_j over those frames, d = c - c[t0] (K18's shift: a constant trace has a
 *                           variance of exactly 0);
 *   scc                     sum c_i c_j over those frames, not shifted.
 * One workgroup of 256 lanes per pair: a lane takes the voxels of the intersection (x slowest, z fastest), then the frames, at lane,
 * lane + 256, .. in that order; t0 comes from a min-reduction on the frame index; the sums are reduced by block_sum0
 * (csrc/block_ops.hpp) in its fixed order.  float64, no atomics, no workspace: the same input gives the same bits.  One launch, no host
 * synchronisation.
 *   boxes, pairs          on the HOST: checked before anything is launched;
 *   boxes_dev, pairs_dev  the same arrays on the device: what the kernel reads.
 * DNMF_E_NULL: a NULL argument;  DNMF_E_SHAPE: a size, K, T or N < 1, lda < P, ldc < T, a pair index outside [0, K), a box that is
 * empty or reaches outside the volume or holds more than 4096 voxels (K24's limit);  DNMF_E_UNSUPPORTED: 2^31 voxels or more.
 *
 * dnmf_merge_apply.  The groups as a CSR table: group g has the members members[offsets[g] .. offsets[g + 1]), indices into the K old
 * components; u and w hold one double per entry of members.  A = P rows of lda >= K floats (the (P, K) layout of the model's
 * footprints, K fastest), C = K rows of ldc >= T floats:
 *   A_out[v ldao + g] = (float) sum_m u[m] (double)A[v lda + members[m]]        P rows of ldao >= Kout floats
 *   C_out[g ldco + t] = (float) sum_m w[m] (double)C[members[m] ldc + t]        Kout rows of ldco >= T floats
 * the sums over a group's members in their order, in float64, rounded once; floats beyond a row's extent are left alone.  The first
 * term is taken as it is, so a group of one member with u = w = 1 comes out bit for bit.  One launch, one thread per entry written.
 *   offsets, members          on the HOST (Kout + 1 and offsets[Kout] ints): checked before anything is launched;
 *   offsets_dev, members_dev  the same on the device;  u, w: device doubles.
 * DNMF_E_NULL: a NULL argument;  DNMF_E_SHAPE: P, K, T or Kout < 1, Kout > K, lda < K, ldao < Kout, ldc or ldco < T, offsets that do
 * not start at 0 or do not increase or pass K, a member outside [0, K), A_out or C_out overlapping A, C or each other;
 * DNMF_E_UNSUPPORTED: 2^39 entries or more.  Nothing is launched on an error. */
int dnmf_component_pairs(const float *A, long lda, const int *sz, const int *boxes, const int *boxes_dev, int K, const float *C,
                         long ldc, int T, const int *pairs, const int *pairs_dev, int N, double *out, dnmf_stream_t stream);
int dnmf_merge_apply(const float *A, long lda, long P, int K, const float *C, long ldc, int T, const int *offsets, const int *members,
                     const int *offsets_dev, const int *members_dev, int Kout, const double *u, const double *w, float *A_out, long ldao,
                     float *C_out, long ldco, dnmf_stream_t stream);

/* ---- K27: cleaning the footprints: median, energy cut, closing, largest part (csrc/footprint_clean.hip) -----------------------------
 * tests/footprint_clean_restatement.py is the definition; every output is an integer or a bit pattern, and an implementation has
 * exactly these bits.  A = P rows of lda >= K floats (the (P, K) layout of the model's footprints, K fastest; voxel p = (x Y + y) Z +
 * z), boxes (K, 6) int32 = (x0, x1, y0, y1, z0, z1) inclusive, as in K24.  Per neuron k, on its box (n voxels):
 *   1  refused (ok = 0, the column of out = the column of A bit for bit) when a box value is not finite or is negative, when none is
 *      positive, when a median of step 2 is such a value (possible only through taps outside the box), or when step 3 keeps nothing;
 *   2  median = 1: m = the median of the 3 x 3 x 3 (Z == 1: 3 x 3 x 1) neighbourhood in the VOLUME, coordinates clamped to it
 *      (scipy.ndimage.median_filter(mode='nearest')), the values ordered as IEEE totalOrder; median = 0: m = a;
 *   3  method 0 ('nrg'): v = the box values of m, descending, cum[j] = the float64 sum of (double)v[i]^2 for i <= j added in that order,
 *      j* = the first j with cum[j] >= nrgthr cum[n - 1], threshold = v[j*], keep = m >= threshold and m > 0 (every tie kept), energy =
 *      cum[j*] / cum[n - 1];  method 1 ('max'): threshold = maxthr (double)max m, keep = (double)m > threshold, energy = NaN;
 *   4  closing = 1: dilation by the full 3 x 3 x 3 element with 0 outside the box, then erosion with 1 outside the box;
 *   5  the largest face-connected (6 neighbours) part by voxel count, a tie to the part that holds the lowest linear index;
 *   6  out = m (values 0, 'filtered') or a (values 1, 'original') on that part, 0 on the rest of the column.
 *   istats  (K, 6) int32: ok, n_box, n_cut, n_closed, n_parts, n_kept (the last four 0 with ok = 0)
 *   dstats  (K, 2) doubles: threshold, energy (both NaN with ok = 0)
 * Two launches, no host synchronisation: one workgroup of 256 lanes per neuron with the box in LDS (56 KiB) writes a compact (K, 4096)
 * buffer in the workspace and the statistics; one thread per entry of out then writes the (P, K) result, K fastest.  The cumulative
 * sum is formed by one lane in the order above (np.cumsum's additions); the parts by minimum-label propagation with a pointer jump,
 * at most n rounds, whose fixed point does not depend on the schedule; sizes by integer LDS atomics.  No floating-point atomics: the
 * same input gives the same bits.  out may be A itself (same pointer and row stride), and may not overlap it otherwise.
 *   boxes      on the HOST: checked before anything is launched;  boxes_dev: the same array on the device
 *   workspace  dnmf_clean_footprints_workspace(K) bytes (0: K < 1), 4-byte aligned
 * DNMF_E_NULL: a NULL argument;  DNMF_E_SHAPE: a size or K < 1, lda or ldo < K, a switch outside {0, 1}, nrgthr outside (0, 1] (method
 * 0), maxthr < 0 (method 1), a box that is empty or reaches outside the volume or holds more than 4096 voxels, out overlapping A;
 * DNMF_E_WORKSPACE: a short or misaligned workspace;  DNMF_E_UNSUPPORTED: 2^31 voxels or 2^39 entries or more.  Nothing is launched on
 * an error. */
size_t dnmf_clean_footprints_workspace(int K);
int dnmf_clean_footprints(const float *A, long lda, const int *sz, const int *boxes, const int *boxes_dev, int K, int method,
                          double nrgthr, double maxthr, int median, int closing, int values, float *out, long ldo, int *istats,
                          double *dstats, void *workspace, size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K28: new components from the residual: the residual on candidate boxes and its rank-1 factor (csrc/add_components.hip) ---------
 * tests/add_restatement.py is the definition in float64.  M candidates, each a box boxes[m] = (x0, x1, y0, y1, z0, z1) inclusive, as in
 * K24, of n_m voxels v_j in the order x slowest, z fastest; a movie of n frames in footprint coordinates.
 *
 * dnmf_residual_boxes (K28a).  For the B frames of the call (rows of ldf >= P floats; row frame_ids[f] of frames, or f; row f of sub,
 * lds >= P floats, or NULL: nothing is subtracted) and every box
 *     E[(m n + t0 + f) vmax + j] = frames_f(v_j) - sub_f(v_j)        one fp32 subtraction; frames_f(v_j) itself without sub
 * for j < n_m, and 0 for n_m <= j < vmax: E is a compact (M, n, vmax) fp32 buffer of which this call writes the frames t0 .. t0 + B - 1,
 * so a movie larger than one buffer goes through in pieces.  A sample that is not finite is copied as it is.  One launch, one workgroup
 * per (box, run of 8 frames); the lanes read the z-rows of the box and write consecutive j.
 *   boxes      (M, 6) int32 on the HOST: checked before anything is launched;  boxes_dev: the same on the device
 * DNMF_E_NULL: frames, sz, boxes, boxes_dev or E NULL;  DNMF_E_SHAPE: a size, M, n, vmax or B < 1, t0 < 0 or t0 + B > n, ldf or lds <
 * P, a box that is empty, reaches outside the volume or holds more than vmax voxels;  DNMF_E_UNSUPPORTED: vmax > 4096, M > 4096, n >
 * 18 432, 2^31 voxels or more.
 *
 * dnmf_rank1_nmf (K28b).  Per candidate the non-negative rank-1 factor a c^T of E[m] (n rows of vmax floats, of which the first
 * nvox[m] = n_m count), from the start a0 (M rows of vmax floats).  The valid frames V are those whose n_m samples are all finite.
 *     repeat iters times:   c_t = max(sum_j a_j e_tj, 0) / sum_j a_j^2  (t in V);   a_j = max(sum_{t in V} c_t e_tj, 0) / sum_{t in V} c_t^2
 *     finish:               a *= sqrt(sum a0^2 / sum a^2), then the c-step once more
 *   a        (M, vmax) fp32: the footprint on the box, 0 for j >= n_m
 *   c        (M, n) fp32: the trace, NaN on the frames outside V
 *   stats    (M, 4) float64: energy = sum_{V, j} e^2;  explained = 2 sum_{t in V} c_t <a, e_t> - |a|^2 |c|^2 (what a c^T takes off the
 *            energy);  |a|^2;  |c|^2 -- of the float64 a and c before they are rounded
 *   n_valid  (M) int32: the frames in V;   ok (M) int32
 * A candidate whose sum a^2 or sum c^2 is not a positive finite number at any step, or whose V is empty, is refused: ok = 0, its a
 * (j < n_m) and c are NaN, explained and the two norms NaN; energy and n_valid are still those of its frames.  So is one whose
 * nvox[m] is outside [1, vmax] (energy 0, n_valid 0).  Nothing is raised.
 * Products of the fp32 samples are taken in float64 and summed in float64 in a fixed order (csrc/add_components.hip states it); a
 * and c stay in float64 between the steps -- a in LDS, c in the workspace -- and are rounded to fp32 once.  One launch runs every
 * iteration, one workgroup of 512 lanes per candidate; no atomics: the same input gives the same bits.  No host synchronisation.
 *   workspace  dnmf_rank1_nmf_workspace(M, n) bytes (0 on bad arguments), 8-byte aligned
 * DNMF_E_NULL: a NULL argument;  DNMF_E_SHAPE: M, n, vmax or iters < 1;  DNMF_E_UNSUPPORTED: vmax > 4096, M > 4096, n > 18 432;
 * DNMF_E_WORKSPACE: a short or misaligned workspace.  Nothing is launched on an error. */
int dnmf_residual_boxes(const float *frames, long ldf, const float *sub, long lds, const int *frame_ids, const int *sz, int B,
                        const int *boxes, const int *boxes_dev, int M, float *E, int n, int vmax, int t0, dnmf_stream_t stream);
size_t dnmf_rank1_nmf_workspace(int M, int n);
int dnmf_rank1_nmf(const float *E, int M, int n, int vmax, const int *nvox, const float *a0, int iters, float *a, float *c,
                   double *stats, int *n_valid, int *ok, void *workspace, size_t workspace_bytes, dnmf_stream_t stream);

/* ---- K29: the channel colours of a multi-channel model: normal equations and their non-negative solve (csrc/colours.hip) -----------
 * tests/colours_restatement.py is the definition in float64.  Channel c of a frame is modelled as sum_k colours[c, k] A_k(q_t) C[k, t];
 * with A_t the UNCOLOURED warped footprints of frame t, G_t = A_t^T A_t and r_t^c = A_t^T y_t^c, the squared error of channel c is the
 * quadratic 1/2 x^T M x - b_c^T x (+ a constant) in x = colours[c, :], with
 *     M[k, l] = sum_t G_t[k, l] C[k, t] C[l, t]   (K, K), the same for every channel       b[c, k] = sum_t r_t^c[k] C[k, t]   (NC, K)
 *
 * dnmf_colour_normal_eqs (K29a).  G (B, K, K) and r (NC, B, K) fp32, contiguous, of the B frames of the call; C = K rows of ldc >= B
 * floats, the traces of those frames.  A term is (double)G ((double)C[k, t] (double)C[l, t]) -- the inner product is exact, so a
 * symmetric G gives a symmetric M bit for bit -- and (double)r (double)C[k, t]; the terms of an entry are added in float64 in the order
 * of t within a segment of 32 frames, from 0.0, and the segments in their order, from 0.0.  The segments are cut on the count of
 * frames since the state was reset, which the state keeps with the sum of the closed segments and the open one: a movie fed in pieces
 * of ANY sizes (first = 1 resets the state, the last call has finish = 1 and writes M and b; both may be NULL without it) gives the
 * bits of one call.  One streaming read of G: a workgroup owns 16 x 64 entries (k, l), a lane 4 of them with consecutive lanes on
 * consecutive l, and one segment, whose traces it stages in LDS once.  Three launches, no floating-point atomics, no host
 * synchronisation; nothing is launched on an error.
 *   state   dnmf_colour_normal_eqs_workspace(K, NC, B) bytes (0 on bad arguments), 8-byte aligned; it grows with B, so the state of the
 *           largest call serves every call
 * DNMF_E_NULL: G, r, C or state NULL, M or b NULL with finish;  DNMF_E_SHAPE: K, NC or B < 1, ldc < B;  DNMF_E_UNSUPPORTED: K > 4096,
 * NC > 16, more than 65534 segments;  DNMF_E_WORKSPACE: a short or misaligned state.
 *
 * dnmf_colour_solve (K29b).  Per channel c, from x = (double)colours[c, :] and h = M x (the terms of h[l] added in the order of k),
 * `sweeps` sweeps of k = 0 .. K - 1:
 *     d = M[k, k];  d > 0 and finite:  x_k' = fmax(0, x_k + (b[c, k] - h[k]) / d),  h += (x_k' - x_k) M[k, :]  (skipped when nothing moves)
 * and a coordinate with any other d is left alone.  M[k, :] stands for column k: M is taken as symmetric.  Then
 *   out    (NC, K) fp32: x rounded once (not written with sweeps = 0, and may then be NULL)
 *   kkt    (NC) float64: max_k |pg_k|, pg_k = (h - b_c)[k] where x_k > 0, else min((h - b_c)[k], 0): zero exactly at the solution
 *   ok     (NC) int32: 0 for a channel whose b, or the shared M, holds an entry that is not finite; its row of out = its row of
 *          colours bit for bit and its kkt is NaN
 * One launch, one workgroup of 256 lanes per channel, float64 throughout.  M is held in LDS where K <= 128 (8 K^2 = 128 KiB of the CU's
 * 160) and read from global memory, a row ahead, beyond that.  The same input gives the same bits.
 * DNMF_E_NULL: M, b, colours, kkt or ok NULL, out NULL with sweeps > 0;  DNMF_E_SHAPE: K or NC < 1, sweeps < 0;  DNMF_E_UNSUPPORTED:
 * K > 4096, NC > 16.  Nothing is launched on an error. */
size_t dnmf_colour_normal_eqs_workspace(int K, int NC, int B);
int dnmf_colour_normal_eqs(const float *G, const float *r, const float *C, long ldc, int K, int NC, int B, int first, int finish,
                           void *state, size_t state_bytes, double *M, double *b, dnmf_stream_t stream);
int dnmf_colour_solve(const double *M, const double *b, const float *colours, int K, int NC, int sweeps, float *out, double *kkt,
                      int *ok, dnmf_stream_t stream);

/* ---- K30: exact order statistics over time, per voxel: the samples behind the median, noise and percentile images ------------------
 * (csrc/robust_images.hip; tests/robust_restatement.py is the definition.)  For the rows y[t, p] of a movie of a volume (X, Y, Z) (rows
 * of ldf >= P floats, voxel p = (x Y + y) Z + z; row frame_ids[j] of frames, or j, for the j-th row of the call) the sequence of a
 * voxel is, by source,
 *   DNMF_SELECT_VALUE    x_t = y_t;
 *   DNMF_SELECT_ABSDEV   x_t = |y_t - centre[p]|, centre a (P) fp32 image: one fp32 subtraction rounded to nearest, then the sign off;
 *   DNMF_SELECT_ABSDIFF  x_t = |y_{t+1} - y_t| in the order the rows are given, the same arithmetic: one term fewer than the movie has
 *                        rows.  The last row of a piece is kept in the state, so a cut between two pieces loses no term.
 * Samples that are not finite are left out; n[p] counts the others.  For each of the nq <= 4 quantiles q[i] in [0, 1] (a HOST array)
 * h = q (n - 1) in float64, lo = floor(h), hi = min(lo + 1, n - 1), and the results are the kept samples of ranks lo and hi in
 * ascending order (from 0; -0 and +0 are one value, returned as +0): input samples, comparable for equality.  Where n = 0 both are NaN.
 * The interpolation between the two is the caller's, in float64.
 * A radix select on the order-preserving 32-bit key of a float, 4 bits a pass: dnmf_temporal_select_passes() = 9 passes (8 digits from
 * the top, then one that counts the samples <= a_lo and takes the least sample above it, which settles a_hi).  EVERY pass streams the
 * whole movie once, in any number of calls (pieces) of any sizes, the same rows in the same order in every pass:
 *   for pass in 0 .. 8:  for every piece:  dnmf_temporal_select_pass(piece, .., pass, rows_before = rows of the earlier pieces, ..)
 *   dnmf_temporal_select_finish(..)
 * rows_before == 0 opens the pass: a launch picks, per voxel and quantile, the digit of the pass before from its counters, and clears
 * them.  The library does not know how many rows a pass had; feeding every pass the same rows is the caller's duty (ops.py keeps count
 * and refuses).  A workgroup owns 256 contiguous voxels (every row is read in full lines) and a segment of frames (segment > 0: that
 * many frames each; 0: the kernel's choice); a thread keeps its voxel's 16 counters per quantile in a column of LDS of its own and
 * adds them to the state with integer atomics at the end -- integer sums do not depend on the order, no floating-point atomics: the
 * same input gives the same bits on every run and however the movie is cut.  4 B per voxel and frame are read in each pass.
 *   state    caller-owned, 4-byte aligned, dnmf_temporal_select_workspace(sz, nq) bytes (0 on bad arguments; it does not depend on
 *            the number of frames): per voxel n and the carried row, per voxel and quantile lo, the remaining rank and the key prefix
 *            (4 B each), and the 16 counters: (8 + 76 nq) B a voxel -- 80 MiB for 512 x 512 x 2 with 2 quantiles.
 *   finish   writes lo (nq, P) fp32, hi (nq, P) fp32 and n (P) int32; valid after pass 8.
 * No host synchronisation.  DNMF_E_NULL: frames, sz, q, state or an output NULL, centre NULL with DNMF_SELECT_ABSDEV;  DNMF_E_SHAPE: a
 * size or B < 1, nq outside 1 .. 4, a q outside [0, 1] (NaN included), an unknown source, pass outside 0 .. 8, segment < 0, ldf < P;
 * DNMF_E_UNSUPPORTED: 2^31 voxels or more, rows_before + B > 2^31 - 1 (the counters are 32 bits wide; nothing is ever truncated), more
 * than 65535 segments;  DNMF_E_WORKSPACE: a short or misaligned state.  Nothing is launched on an error. */
#define DNMF_SELECT_VALUE 0
#define DNMF_SELECT_ABSDEV 1
#define DNMF_SELECT_ABSDIFF 2
int dnmf_temporal_select_passes(void);
size_t dnmf_temporal_select_workspace(const int *sz, int nq);
int dnmf_temporal_select_pass(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, int source,
                              const float *centre, const double *q, int nq, int pass, long rows_before, int segment, void *state,
                              size_t state_bytes, dnmf_stream_t stream);
int dnmf_temporal_select_finish(const int *sz, int nq, const void *state, size_t state_bytes, float *lo, float *hi, int *n,
                                dnmf_stream_t stream);

/* ---- K31: the running-percentile baseline of a movie, and the movie read against it (dF/F) ----------------------------------------
 * (csrc/running_baseline.hip; tests/dff_restatement.py is the definition.)  A movie of T frames is covered by J windows of
 * `window` = W frames, one every `stride` = S frames (1 <= S <= W <= 2048): J = 1 if T <= W, else ceil((T - W) / S) + 1
 * (dnmf_running_windows; 0 on bad arguments); window j holds the frames [s_j, e_j), s_j = min(j S, max(T - W, 0)),
 * e_j = min(s_j + W, T) -- the last window ends at T and is full-length whenever T >= W -- and its knot sits at c_j = (s_j + e_j - 1) / 2.
 *
 * K31a, dnmf_running_quantile.  frames: B rows of ldf >= P floats (row frame_ids[i] of frames, or i, for the i-th row of the call), the
 * frames row0 .. row0 + B - 1 of the movie in time order.  Computed are exactly the windows that lie wholly inside these rows, j0 .. j1 - 1,
 * and windows[0] = j0, windows[1] = j1 (windows: a HOST array of two longs, written before the call returns; j0 == j1: nothing is
 * launched).  Per voxel p and window j, of the samples of the window that are finite (NaN and +-inf are left out, as in K30):
 *   n[j ldk + p]    int32, their count;
 *   lo, hi[j ldk + p]  fp32, those of ranks floor(h) and min(floor(h) + 1, n - 1) in ascending order, h = q (n - 1) in float64: input
 *                   samples, bit for bit (-0 and +0 are one value, returned as +0); NaN where n = 0.
 * Rows outside j0 .. j1 - 1 of the three tables are not touched; the interpolation between lo and hi is the caller's, in float64.
 * A workgroup owns 64 contiguous voxels (32 for W > 512, 16 for W > 1024) and `run` consecutive windows (0: the kernel's choice --
 * about 1024 workgroups, so that a movie of few voxels, a matrix of traces, still fills the machine).  It holds the window in LDS
 * as K30's 32-bit keys in a ring of W rows, so that the step to the next window reads S new rows: within a run every sample is
 * read from memory once, (W + (run - 1) S) rows per run.  Selection by bisection on the key, integer counts only: no floating-point
 * atomics, no scratch, no workspace, and the same bits for every run, for every cut of the movie into calls and on every launch.
 *
 * K31b, dnmf_baseline_apply.  value (J, ldv >= P) float64: the knot values b_j per voxel; centres (J) float64 DEVICE, strictly
 * increasing: their abscissae.  For row i of the call, frame t = row0 + i:  F0 = b_0 for t <= c_0, b_{J-1} for t >= c_{J-1}, else with
 * c_j <= t < c_{j+1} and w = (t - c_j) / (c_{j+1} - c_j):  F0 = b_j if w == 0, else b_j + w (b_{j+1} - b_j), each operation rounded
 * once in float64 (a NaN knot spreads through this arithmetic and nowhere else).  out[i ldo + p], from the fp32 sample y and F0 in
 * float64, rounded once to fp32, by mode:
 *   DNMF_BASELINE_F0  F0;   DNMF_BASELINE_DF  y - F0;   DNMF_BASELINE_DFF  (y - F0) / (F0 + offset);
 *   DNMF_BASELINE_DFSQRTF  (y - F0) / sqrt(F0 + offset);
 * NaN where y or F0 is not finite and, in the last two modes, where F0 + offset <= 0.  One streaming launch: 4 B read and 4 B written
 * per voxel and frame, a thread keeps the two knot values of its interval in registers over 32 consecutive frames.  out may not
 * overlap frames.
 * No host synchronisation.  DNMF_E_NULL: a required pointer NULL;  DNMF_E_SHAPE: a size, B, J, T or window < 1, stride outside
 * [1, window], q outside [0, 1] (NaN included), rows outside the movie, run < 0, an unknown mode, an offset that is not finite, a
 * leading dimension below P, out overlapping frames;  DNMF_E_UNSUPPORTED: window > 2048, 2^31 voxels or more, more than 65535 runs.
 * Nothing is launched on an error. */
#define DNMF_BASELINE_F0 0
#define DNMF_BASELINE_DF 1
#define DNMF_BASELINE_DFF 2
#define DNMF_BASELINE_DFSQRTF 3
long dnmf_running_windows(long T, int window, int stride);
int dnmf_running_quantile(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, long T, int window,
                          int stride, double q, int run, float *lo, float *hi, int *n, long ldk, long *windows,
                          dnmf_stream_t stream);
int dnmf_baseline_apply(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, const double *value,
                        long ldv, const double *centres, int J, int mode, double offset, float *out, long ldo,
                        dnmf_stream_t stream);

/* ---- K34: local low-rank denoising of a registered movie: patch-wise truncated SVD, blended ----------------------------------------
 * (csrc/lowrank_denoise.hip; tests/denoise_restatement.py is the definition.)  The volume is covered by patches of one shape:
 * `plan` is a HOST array of 9 ints, per axis (count, stride, len) -- patch i of an axis starts at min(i stride, extent - len) and holds
 * len <= extent voxels; the last one ends at the extent (count - 1) stride >= extent - len, no patch repeats it, stride <= len.  Patch
 * p = (ix cy + iy) cz + iz; a voxel's index v in its patch runs z fastest; n = lenx leny lenz <= 1024 (dnmf_lowrank_patches: the
 * number of patches NP, 0 on a bad plan; dnmf_lowrank_tile_frames(n): the frames K34a stages at once, 32, 16 above 256 voxels, 8
 * above 512; 0 for n outside [1, 1024]).  All state is float64 on the device: U, W (NP, n, R), Q (NP, T, R), energy (NP, T), lam
 * (NP, R), explained (NP); kept, ok (NP) int32.  1 <= R = rank <= 8.  centre, scale: (P) float64 images, scale NULL = ones;
 * D[v, t] = (y[v, t] - centre[v]) / scale[v].  frames: B rows of ldf >= P floats, row frame_ids[i] (or i) the i-th of the call.
 *
 * K34a, dnmf_lowrank_accumulate.  W[p] += D_p (D_p^T U[p]) over the rows of the call: per frame q = D_t^T U (the voxels in order),
 * then W[v, :] += D[v, t] q, the frames in order -- the same bits however the movie is cut into calls.  A sample or centre that is not
 * finite, or a scale that is not finite or <= 0, sets ok[p] = 0 (the caller starts it at 1); a patch with ok = 0 is skipped.
 * K34b, dnmf_lowrank_orthonormalise.  U[p] = MGS(W[p]) in column order -- a column whose norm after the projections is <= 1e-12 x
 * its norm before becomes zero -- and W[p] = 0; U[p] = 0 where ok[p] = 0.
 * K34c, dnmf_lowrank_project.  Q[p, row0 + i, :] = D_t^T U[p] and energy[p, row0 + i] = sum_v D[v, t]^2 for the rows of the call.
 * K34d, dnmf_lowrank_ritz.  B = Q^T Q, `sweeps` sweeps of cyclic Jacobi (a parameter of the algorithm, not a tolerance), lam =
 * the eigenvalues in descending order (ties by index), U and Q rotated to match; kept[p] = the number of lam > edge (keep < 0), or of
 * lam > 0 among the first keep; explained[p] = sum of the kept lam / sum_t energy[p, t] (0 where that is 0).  ok[p] = 0: lam = 0,
 * kept = 0, explained = 0.
 * K34e, dnmf_lowrank_reconstruct.  out[i ldo + v] = fp32( sum_p w_p (centre + scale sum_{j < kept[p]} U[p, v, j] Q[p, row0 + i, j])
 * / sum_p w_p ) over the patches p with ok[p] = 1 that hold v, ascending, w_p = prod_axes min(i + 1, len - i) for the in-patch
 * coordinates i; frames[..] itself, bit for bit, where no such patch holds v (frames is read nowhere else).
 * One workgroup per patch (a-d), one thread per voxel and 8 frames (e).  No floating-point atomics, no scratch, no workspace, no host
 * synchronisation.  DNMF_E_NULL: a required pointer NULL;  DNMF_E_SHAPE: a size < 1, a plan that does not tile the volume, rank
 * outside [1, 8], rows outside the movie, a leading dimension below P, sweeps outside [0, 64];  DNMF_E_UNSUPPORTED: n > 1024, 2^31
 * voxels or patches or more, B > 8 x 65535 (K34e).  Nothing is launched on an error. */
long dnmf_lowrank_patches(const int *sz, const int *plan);
int dnmf_lowrank_tile_frames(int n);
int dnmf_lowrank_accumulate(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, const int *plan, int rank,
                            const double *centre, const double *scale, const double *U, double *W, int *ok, dnmf_stream_t stream);
int dnmf_lowrank_orthonormalise(long NP, int n, int rank, double *U, double *W, const int *ok, dnmf_stream_t stream);
int dnmf_lowrank_project(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, long T, const int *plan,
                         int rank, const double *centre, const double *scale, const double *U, double *Q, double *energy, int *ok,
                         dnmf_stream_t stream);
int dnmf_lowrank_ritz(long NP, int n, long T, int rank, int keep, double edge, int sweeps, double *U, double *Q, const double *energy,
                      const int *ok, double *lam, int *kept, double *explained, dnmf_stream_t stream);
int dnmf_lowrank_reconstruct(const float *frames, long ldf, const int *frame_ids, const int *sz, int B, long row0, long T, const int *plan,
                             int rank, const double *centre, const double *scale, const double *U, const double *Q, const int *kept,
                             const int *ok, float *out, long ldo, dnmf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_HIP_H */
