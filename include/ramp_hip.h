/*
 * ramp_hip.h -- C ABI of libramp_hip.so, the MI355X (gfx950) implementation of
 * the RAMP-VO tracking hot path.
 *
 * Every entry point replaces one native entry point (or one fused group of
 * ATen calls) of the reference; the reference interface it stands in for is
 * cited as file:line (paths relative to the upstream repository).  The
 * reference binds its natives through pybind11/torch::Tensor; this boundary is
 * plain C: device pointers, sizes, a hipStream_t (passed as void*), int status.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host
 *   - index arrays are int64 (torch.long), like the reference
 *   - return value: RAMP_OK (0) or a negative RAMP_E* code; kernels are
 *     enqueued on `stream` and NOT synchronised
 *   - no entry point allocates device memory: scratch is supplied by the
 *     caller (`ws`, sized by the matching *_workspace_bytes query)
 *   - poses are [tx ty tz qx qy qz qw] float32 (lietorch SE3 embedding)
 *   - feature maps come in two layouts: RAMP_NCHW (the reference's) and
 *     RAMP_NHWC (channels-last, this library's native layout: one pixel's
 *     channels are contiguous so a wavefront reads whole 512 B rows)
 *   - the Python binding (rampvo_amd/_lib.py) keeps no copy of the numbers or
 *     signatures below: it reads this file when it is imported.  So a value
 *     macro is `#define RAMP_<NAME> <integer or float literal>`, a scalar
 *     parameter is an int, long, size_t, float, double or <stdint.h> type, and
 *     everything with a `*` is passed as a void pointer.  The structs are still
 *     mirrored by hand there (a test holds them to the C compiler's layout)
 */
#ifndef RAMP_HIP_H
#define RAMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAMP_OK 0
#define RAMP_EINVAL -1      /* bad argument (null pointer, unsupported size) */
#define RAMP_ELAUNCH -2     /* HIP reported a launch/runtime error            */
#define RAMP_EWORKSPACE -3  /* workspace too small                            */
#define RAMP_EUNSUPPORTED -4

#define RAMP_F32 0
#define RAMP_F16 1

/* ramp_corr_fwd*, fp32 + RAMP_NHWC only: OR into `dtype` to use the fp32 MFMA kernel (2.1x faster; results
 * within 1e-5 of the default kernel, which keeps the reference's channel-ordered fmaf accumulation)      */
#define RAMP_CORR_MFMA32 0x40
/* fp32 features as split fp16 pairs, "x2" (round 6): every value x = xh + xl 2^-11 (xh = fp16(x), xl = fp16((x - xh) 2^11): 22
 * significant bits), a dot product = three v_mfma_f32_16x16x32_f16 products (ah bh; ah bl + al bh) into two fp32 accumulators:
 * fp32-class accuracy (<= 1e-5 of the default kernel like RAMP_CORR_MFMA32, whose fp32 MFMAs cost >= 240 us per launch at
 * 41k factors) at the fp16 kernel's speed for twice the window bytes.  OR into `dtype` (RAMP_F32) of
 *   ramp_pyramid_pack: the planes are written as [H][4][2][W][32] fp16 (per row and 32-channel step a [W][32] plane of high
 *     parts, then one of low parts; 512 bytes per pixel like the fp32 planes) -- level 4 is pooled in fp32, then split;
 *   ramp_corr_fwd* with RAMP_NHWC32: the target maps are such planes (fmap1 stays fp32 RAMP_NHWC rows, split while loading;
 *     the output stays fp32).  Any other layout / dtype with this bit: RAMP_EINVAL.                                      */
#define RAMP_CORR_X2 0x80

#define RAMP_NCHW 0
#define RAMP_NHWC 1
#define RAMP_NHWC32 2  /* [H][C/32][W][32] (fp16) / [H][C/16][W][16] (fp32: with RAMP_CORR_MFMA32 only) / [H][4][2][W][32] fp16
                          parts (fp32 with RAMP_CORR_X2): correlation target maps (ramp_pyramid_pack); 64 bytes per pixel and
                          plane = one 16-byte load of every lane quarter */

/* library / build identification: returns a static string */
const char *ramp_version(void);

/* ------------------------------------------------------------------ altcorr */

/* cuda_corr.patchify_forward + the bilinear blend of altcorr.patchify
 * (ramp/altcorr/correlation.cpp:47-50, correlation_kernel.cu:16-47,288-307,
 *  ramp/altcorr/correlation.py:51-68).
 *   net    [n][C][H][W] (NCHW) or [n][H][W][C] (NHWC), dtype
 *   coords [n][M][2] float32 (x, y)
 *   out    bilinear=1: [n][M][C][2R+1][2R+1]   (altcorr.patchify, fused)
 *          bilinear=0: [n][M][C][2R+2][2R+2]   (raw cuda_corr.patchify_forward)
 *   out_layout RAMP_NCHW: as above;  RAMP_NHWC: [n][M][d][d][C]                */
int ramp_patchify_fwd(const void *net, const float *coords, void *out, int n, int C, int H,
                      int W, int M, int radius, int bilinear, int dtype, int layout,
                      int out_layout, void *stream);

/* All per-frame gathers at the M patch centres in one launch (ramp/net.py:167-203: gmap = 3x3 patches of fmap, imap =
 * 1x1 of the context map, the 3x3 (x, y, disparity=1) patches of the coordinate grid, the colours of the full-resolution
 * image at 4*(coords+0.5); Ramp_vo.py:353-354: uint8 BGR colours).  Bit-identical to the four ramp_patchify_fwd calls.
 *   fmap [h][w][CF], imap [h][w][CI] (NHWC, dtype RAMP_F32 / RAMP_F16); image [3][H][W] fp32; coords [M][2] fp32
 *   -> gmap [M][3][3][CF], imap_p [M][CI] (dtype), patches [M][3][3][3] fp32 (channel-major), clr [M][3] fp32,
 *      colors [M][3] uint8 (BGR)                                                                                  */
int ramp_frame_gather(const void *fmap, const void *imap, const float *image, const float *coords, void *gmap,
                      void *imap_p, float *patches, float *clr, unsigned char *colors, int M, int h, int w, int H,
                      int W, int CF, int CI, int dtype, void *stream);

/* cuda_corr.forward (ramp/altcorr/correlation.cpp:28-35,
 * correlation_kernel.cu:82-136 + host blend/permute 193-233), fused over the
 * levels of the feature pyramid and with the torch.stack(..., -1) of
 * ramp/Ramp_vo.py:175-182 folded into the store.
 *   fmap1   patch features: NCHW [N1][C][P][P] or NHWC [N1][P][P][C]
 *   level l target features: NCHW [N2][C][H2_l][W2_l] or NHWC [N2][H2_l][W2_l][C]
 *   coords  [E][2][P][P] float32, divided by coord_div_l inside the kernel
 *   ii[E]   index into fmap1,  jj[E] index into the level's fmap
 *   out     [E][2R+1 (x off)][2R+1 (y off)][P][P][nlevels], dtype
 * nlevels==1 reproduces cuda_corr.forward's (permuted, contiguous) result.   */
typedef struct {
  const void *fmap;
  int H2, W2;
  float coord_div;
} ramp_corr_level;

int ramp_corr_fwd(const void *fmap1, const ramp_corr_level *levels_host, int nlevels,
                  const float *coords, const int64_t *ii, const int64_t *jj, void *out, int E,
                  int N1, int N2, int C, int P, int radius, int dtype, int layout,
                  void *stream);

/* Same result as ramp_corr_fwd (every edge is computed independently, so the
 * schedule cannot change a value).  order[E] (int32, device; NULL = identity)
 * is the order in which edges are handed to workgroups: consecutive positions
 * run on the same XCD, so a target-frame-major order keeps each frame's
 * feature plane in one L2.  The tracker passes the (jj, ii) pair grouping of
 * its graph plan.  out_row_elems (0 = dense, 441 * nlevels): elements per edge
 * row of `out`; the tail of a longer row is zero filled -- 896 instead of 882
 * makes the rows 16-byte aligned for the first Linear layer of the update
 * operator (library GEMM: 49 instead of 88 us at E = 40k).  mod_ii / mod_jj
 * > 0: ii[e] % mod_ii and jj[e] % mod_jj are used (the `kk % (M*mem)`,
 * `jj % mem` ring-buffer slots of ramp/Ramp_vo.py:178-179).                 */
int ramp_corr_fwd_ordered(const void *fmap1, const ramp_corr_level *levels_host, int nlevels,
                          const float *coords, const int64_t *ii, const int64_t *jj,
                          const int32_t *order, void *out, int out_row_elems, long mod_ii, long mod_jj, int E,
                          int N1, int N2, int C, int P, int radius, int dtype, int layout, void *stream);

/* Ramp_vo.__call__'s pyramid store (ramp/Ramp_vo.py:378-381: fmap1_[slot] =
 * fmap, fmap2_[slot] = avg_pool2d(fmap, 4, 4)) for fp16 channels-last features:
 * fmap [H][W][C] -> level1 [H][C/32][W][32] (same values) and level4
 * [H/4][C/32][W/4][32] (4x4 mean, fp32 sum, one rounding).  These are the
 * RAMP_NHWC32 target maps of ramp_corr_fwd (fmap1 stays RAMP_NHWC).  fp32 features
 * (dtype RAMP_F32): planes of 16 channels, [H][8][W][16] and [H/4][8][W/4][16]; the
 * mean is the window summed in (ky, kx) order times 1/16 = torch's avg_pool2d.
 * dtype RAMP_F32 | RAMP_CORR_X2: the same fp32 input, planes of split fp16 pairs (see RAMP_CORR_X2; same byte counts).
 * C == 128, W % 16 == 0, H % 4 == 0, else RAMP_EUNSUPPORTED.                 */
int ramp_pyramid_pack(const void *fmap, void *level1, void *level4, int H, int W, int C, int dtype,
                      void *stream);
/* channels per plane of the RAMP_NHWC32 layout this library packs and reads ([H][C/k][W][k]): 32.  Libraries of rounds
 * 2-3 packed planes of 8; the caller sizes and converts its ring buffers with this value, and a binding written for
 * another width must refuse to run (rampvo_amd/_lib.py checks it when the library loads).                           */
int ramp_corr_kplane(void);

/* Event list -> int8 bin stack, the encoder's event input (reference utils/transformers.py:128-161,
 * EventToStack_Numpy; upstream a host-side np.add.at).  Event i goes to bin
 * int32(float32(bins * i) / N); polarities p[i] (+-1) are accumulated per (bin, y, x) and the sum is cast to
 * int8 (wraps).  Integer pixel coordinates only (the reference's uint16 path; its sub-pixel bilinear path is
 * ramp_event_warp with RAMP_WARP_IDENTITY).  out_i8 and/or out_f32 [bins][H][W]; ws: ramp_event_stack_workspace_bytes.          */
size_t ramp_event_stack_workspace_bytes(int bins, int H, int W);
int ramp_event_stack(const int32_t *x, const int32_t *y, const int8_t *p, int N, int bins, int H, int W,
                     int8_t *out_i8, float *out_f32, void *ws, size_t ws_bytes, void *stream);

/* Depth initialisation of a new frame (ramp/Ramp_vo.py:370-371): the lower median (torch.median) of the
 * inverse depths of the last F frames' patches -- patches_src = &patches_[n-F], [F][M][3][P][P] -- written
 * into channel 2 of the M new patches patches_dst [M][3][P][P].  F*M*P*P <= 4096.                   */
int ramp_depth_median_fill(const float *patches_src, int F, int M, int P, float *patches_dst, void *stream);
/* the same median into device memory (*out), for a caller that computes it ahead of ramp_frame_commit (median_dev) */
int ramp_depth_median(const float *patches_src, int F, int M, int P, float *out, void *stream);
/* the same over rows n - F .. n - 1 of patches_base [rows][M][3][P][P] with n = *n_dev read on the device (a caller that
 * does not know the row count: the device-resident tracker).  Fewer than F rows: the rows there are; none: *out = 0.  */
int ramp_depth_median_rows(const float *patches_base, const int32_t *n_dev, int F, int M, int P, float *out, void *stream);

/* Event-biased patch-centre selection: get_coords_from_topk_events + nms_image
 * (ramp/utils.py:186-226, 157-183; upstream ~20 ATen launches) for one frame.
 *   events [bins][H][W] float32 (W % 4 == 0); score = mean over bins of the 4x4 average of |events|,
 *   laid out [W/4][H/4]; local maxima of an nms_kernel_size^2 window kept (0 = no NMS);
 *   the k largest cells in descending order, equal cells by lowest flat index first.  The order is exact for any
 *   number of ties, zeros included (event stacks are small integers: most cells of a quiet scene are equal):
 *   the cells above the k-th largest value T are all taken, then the cells equal to T in index order until
 *   there are k; the same input gives the same bits on every call
 *   coords [k][2] float32 = (flat_index / (H/4) as a TRUE division -- x carries y/h, as upstream --,
 *   flat_index % (H/4));  indices [k] int64 flat indices (optional, may be NULL)
 *   ws: ramp_event_topk_workspace_bytes(H, W);  k <= 512                                          */
size_t ramp_event_topk_workspace_bytes(int H, int W);
int ramp_event_topk(const float *events, int bins, int H, int W, int k, int nms_kernel_size, float *coords,
                    int64_t *indices, void *ws, size_t ws_bytes, void *stream);

/* ----------------------------------------------------------------- lietorch */
/* lietorch_backends.{expm,logm,inv,mul,act4,adj,adjT} for group_id 3 (SE3),
 * float32, forward only (ramp/lietorch/src/lietorch.cpp:286-316; math from
 * ramp/lietorch/include/se3.h:30-142, so3.h:31-208).  n = batch elements.   */
int ramp_se3_exp(const float *a, float *X, int n, void *stream);
int ramp_se3_log(const float *X, float *a, int n, void *stream);
int ramp_se3_inv(const float *X, float *Y, int n, void *stream);
int ramp_se3_mul(const float *X, const float *Y, float *Z, int n, void *stream);
int ramp_se3_act4(const float *X, const float *p, float *q, int n, void *stream);
int ramp_se3_adj(const float *X, const float *a, float *b, int n, void *stream);
int ramp_se3_adjT(const float *X, const float *a, float *b, int n, void *stream);

/* ---------------------------------------------------------- projective ops */
/* pops.transform(SE3(poses), patches, intrinsics, ii, jj, kk[, tonly])
 * followed by .permute(0,1,4,2,3).contiguous(), i.e. Ramp_vo.reproject
 * (ramp/projective_ops.py:16-101 jacobian=False path, ramp/Ramp_vo.py:184-192;
 * ~10 torch kernels + 3 lietorch launches upstream).
 *   poses [Np][7], patches [Nk][3][P][P], intrinsics [Np][4] (per frame)
 *   out   [E][2][P][P]                                                        */
int ramp_transform(const float *poses, const float *patches, const float *intrinsics,
                   const int64_t *ii, const int64_t *jj, const int64_t *kk, float *out, int E,
                   int P, int tonly, void *stream);

/* cuda_ba.reproject (ramp/fastba/ba.cpp:48-56, ba_cuda.cu:379-429,585-617):
 * frame-0 intrinsics, no depth clamp.  out [E][2][P][P]                      */
int ramp_reproject(const float *poses, const float *patches, const float *intrinsics,
                   const int64_t *ii, const int64_t *jj, const int64_t *kk, float *out, int E,
                   int P, void *stream);

/* pops.point_cloud (ramp/projective_ops.py:103-105) reduced to what
 * Ramp_vo.update keeps (ramp/Ramp_vo.py:308-310): the 3-D point of each patch
 * centre.  ix[m] = source frame of patch m.  out [m][3]                      */
int ramp_point_cloud(const float *poses, const float *patches, const float *intrinsics,
                     const int64_t *ix, float *out, int m, int P, void *stream);

/* Ramp_vo.motionmag(i, j) and motionmag(j, i) in one launch (ramp/Ramp_vo.py:227-243 over
 * pops.flow_mag, projective_ops.py:108-118, beta-weighted full / translation-only flow).  The
 * edges of each direction are located through the (ii, jj) grouping of ramp_group_by[_small]
 * (order / seg / sorted unique keys / ngroups); key_ij, key_ji are the two pair keys in that
 * grouping's key space.  out2[0] = mean flow i->j, out2[1] = j->i (NaN when a direction has no edge). */
int ramp_motionmag(const float *poses, const float *patches, const float *intrinsics,
                   const int64_t *ii, const int64_t *jj, const int64_t *kk, const int32_t *order,
                   const int32_t *seg, const int64_t *ukeys, const int32_t *ngroups, int64_t key_ij,
                   int64_t key_ji, float beta, float *out2, int P, void *stream);

/* DAMPED_LINEAR motion model (ramp/Ramp_vo.py:356-363; 5 lietorch launches upstream):
 * poses[n] = Exp(damping * Log(poses[n-1] * poses[n-2]^-1)) * poses[n-1]                      */
int ramp_motion_model(float *poses, int n, float damping, void *stream);

/* The per-frame bookkeeping of Ramp_vo.__call__ (ramp/Ramp_vo.py:345-363: tstamps_[n], index_map_[n+1],
 * intrinsics_[n], motion-model pose) as one launch.  motion: 0 = none, 1 = DAMPED_LINEAR (as above),
 * 2 = poses[n] = poses[n-1]; copy_k: intrinsics[n] = intrinsics[n-1] (the caller writes the row itself when
 * the intrinsics changed); tstamps / index_map may be NULL.                                       */
int ramp_frame_begin(float *poses, int n, int motion, float damping, int64_t *tstamps, int64_t counter,
                     int64_t *index_map, int64_t index_val, float *intrinsics, int copy_k, void *stream);

/* ramp_frame_begin + ramp_depth_median_fill + ramp_multi_copy of a steady-state Ramp_vo.__call__ as ONE launch
 * (ramp/Ramp_vo.py:345-381; three dependent tiny launches on the frame's critical path otherwise):
 *   frame_begin's arguments as above; patches_state [N][M][3][P][P] fp32: the depth channel of patches_new
 *   [M][3][P][P] becomes the median of rows n - median_frames .. n - 1 (median_frames = 0: left as is) and
 *   patches_new is stored as row n; then dst[b] = src[b] for n_copy <= 6 further buffers (16-byte aligned,
 *   16-byte multiples: colours, imap, gmap, fmap1, fmap2 rows).                                          */
int ramp_frame_commit(float *poses, int n, int motion, float damping, int64_t *tstamps, int64_t counter,
                      int64_t *index_map, int64_t index_val, float *intrinsics, int copy_k, float *patches_state,
                      int median_frames, int M, int P, float *patches_new, int n_copy, const void *const *src_host,
                      void *const *dst_host, const long *bytes_host, const float *median_dev, void *stream);

/* Tracker bookkeeping helpers (host-side pointer arrays, <= 10 buffers per call).
 * ramp_multi_copy: dst[b][0:bytes[b]) = src[b][...] -- the per-frame stores of imap/gmap/fmap1/fmap2/
 *   patches/colors into the state buffers (ramp/Ramp_vo.py:345-381) in one launch.
 * ramp_shift_rows: rows k+1..nrows-1 of every buffer move down by one -- the keyframe-removal loop of
 *   ramp/Ramp_vo.py:258-268; mod[b] > 0 marks a ring buffer (row r lives at slot r % mod[b]).        */
int ramp_multi_copy(const void *const *src_host, void *const *dst_host, const long *bytes_host, int n,
                    void *stream);
int ramp_shift_rows(void *const *base_host, const long *row_bytes_host, const int *mod_host, int n, int k,
                    int nrows, void *stream);

/* ------------------------------------------------------------------- graph */
/* group the E edges by an int64 key (device-side replacement of the
 * torch.unique / torch::_unique / std::stable_sort host round trips at
 * ramp/blocks.py:43, ramp/fastba/ba_cuda.cu:447, ramp/fastba/ba.cpp:59-97).
 *   keys      : 0 <= key < 2^63 (the sort ignores bit 63: a negative key is a contract violation, and so is a
 *               key at or above a given key_bound)
 *   key_bound : exclusive upper bound of the keys (0 = unknown: full 63 bits)
 *   order[E]      edge indices sorted by (key, edge index)  (stable)
 *   gid[E]        dense rank of the edge's key among the sorted unique keys
 *                 (== the `inverse` of torch.unique(sorted=True))
 *   seg_start[E+1] first sorted position of every group, seg_start[G] = E
 *   ukeys[E]      the sorted unique keys (first G entries valid), may be NULL
 *   ngroups       device int: G                                              */
size_t ramp_group_by_workspace_bytes(int E);
int ramp_group_by(const int64_t *keys, int E, int64_t key_bound, int32_t *order, int32_t *gid,
                  int32_t *seg_start, int64_t *ukeys, int32_t *ngroups, void *ws,
                  size_t ws_bytes, void *stream);

/* cuda_ba.neighbors(kk, jj) (ramp/fastba/ba.cpp:59-97): previous / next edge
 * of the same kk ordered by jj (stable), -1 at either end.  Entirely on the
 * device (the reference copies to the host, sorts, copies back).
 * kk_bound / jj_bound: exclusive upper bounds (0 = unknown).                 */
size_t ramp_neighbors_workspace_bytes(int E);
int ramp_neighbors(const int64_t *kk, const int64_t *jj, int64_t *ix, int64_t *jx, int E,
                   int64_t kk_bound, int64_t jj_bound, void *ws, size_t ws_bytes,
                   void *stream);

/* SoftAgg core (ramp/blocks.py:44-45; torch_scatter.scatter_softmax +
 * scatter_sum): y[g][c] = sum_{e in g} softmax_e(gx[e][c]) * fx[e][c]
 * with the groups given by ramp_group_by's (order, seg_start, ngroups).
 *   fx, gx [E][C] dtype;  y [>=G][C] dtype (rows >= G untouched)             */
int ramp_segment_softmax_sum(const void *fx, const void *gx, const int32_t *order,
                             const int32_t *seg_start, const int32_t *ngroups, void *y, int E,
                             int C, int max_groups, int dtype, void *stream);

/* ------------------------------------------------------------------ fastba */
/* cuda_ba.forward (ramp/fastba/ba.cpp:32-45, ba_cuda.cu:433-582): `iterations`
 * damped Gauss-Newton steps on the reprojection error of the patch centres,
 * poses t0..t1-1 free.  poses [n_poses][7] and patches [n_patches][3][P][P]
 * are updated IN PLACE (rows t0..t1-1 / depth channel of the patches that
 * appear in kk), exactly as the reference mutates its arguments.
 *   target, weight [E][2]; lmbda [1]; intrinsics [>=1][4] (row 0 is used,
 *   ba_cuda.cu:253-258)
 *   info: optional device int (bit mask, zeroed by the call): bit 0 = the Cholesky factorisation hit a
 *         non-positive pivot or produced a step that is not finite (the reference discards cholesky_ex's info and
 *         returns NaN poses; here the pose step of that iteration is dropped); bit 1 = more than 1024 pose-pair records touch one pose (> 512 frames
 *         connected to one frame): the normal equations are incomplete, the result must be discarded
 * Deterministic: all reductions are ordered segment sums, no float atomics.  */
size_t ramp_ba_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1);
int ramp_ba_forward(float *poses, float *patches, const float *intrinsics, const float *target,
                    const float *weight, const float *lmbda, const int64_t *ii,
                    const int64_t *jj, const int64_t *kk, int E, int P, int n_poses,
                    int n_patches, int t0, int t1, int iterations, void *ws, size_t ws_bytes,
                    int32_t *info, void *stream);

/* ramp_ba_forward with the two edge groupings supplied by the caller (the tracker builds them once
 * per graph change and shares them with the update operator's SoftAgg): by patch kk
 * (order_k / seg_k / ngroups_k / ukeys_k = sorted unique kk) and by pose pair (ii, jj) in
 * lexicographic order (order_p / seg_p / ngroups_p), as produced by ramp_group_by[_small].
 * max_patches / max_pairs: upper bounds of the group counts (grid sizes, workspace).          */
size_t ramp_ba_planned_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1,
                                       int max_patches, int max_pairs);
int ramp_ba_forward_planned(float *poses, float *patches, const float *intrinsics, const float *target,
                            const float *weight, const float *lmbda, const int64_t *ii,
                            const int64_t *jj, const int64_t *kk, int E, int P, int n_poses,
                            int n_patches, int t0, int t1, int iterations, const int32_t *order_k,
                            const int32_t *seg_k, const int32_t *ngroups_k, const int64_t *ukeys_k,
                            int max_patches, const int32_t *order_p, const int32_t *seg_p,
                            const int32_t *ngroups_p, int max_pairs, void *ws, size_t ws_bytes,
                            int32_t *info, void *stream);

/* Uncertainty of the window: the marginal covariance of the free poses and the marginal variance of every patch depth, from
 * the system ramp_ba_forward builds in ONE iteration, linearised at the state passed in.  No step is taken: poses and
 * patches are only read.  With the per-factor terms, the validity gate and the fixed poses exactly as in ramp_ba_forward,
 *   Q = 1 / (C + lambda),  S = B - E Q E',  S_dd += 1e-4 S_dd + 1   (the solver's own diagonal damping: the covariance is
 *                                                                   that of the system the step is actually solved with)
 *   cov [6N][6N]        = S^-1, N = t1 - t0, symmetric bit for bit, both triangles written.  Tangent order as the step's:
 *                         translation 3, rotation 3 per pose; the perturbation is the left one of the retraction
 *                         T <- Exp(xi) T on the world-to-camera poses
 *   depth_var [n_patches]: entry kk = Q_k + Q_k^2 |L^-1 e_k|^2 (S = L L'; never below Q_k) for every patch with at least
 *                         one factor; the other entries are left as the caller filled them
 *   stats [8] words     : [0] chi2 = sum over valid factors of w0 rx^2 + w1 ry^2 (float, summed in a fixed order), then as
 *                         int32 bit patterns [1] valid factors, [2] Mu (patches with a factor), [3] N, [4] t0,
 *                         [5] 1 when the factorisation failed; [6], [7] zero
 * t1 == t0 (no free pose): cov is not touched, depth_var = Q_k.  E >= 1.
 *   info: optional device int, zeroed by the call; bit 0 = the factorisation hit a non-positive pivot or the inverse is not
 *         finite: cov and the depth_var entries the call writes are then NaN (never a plausible number); bit 1 as
 *         ramp_ba_forward.  The return value stays RAMP_OK: it is an arithmetic outcome.
 * Deterministic: ordered sums and fma chains only, the same bits from call to call.                                    */
size_t ramp_ba_covariance_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1);
int ramp_ba_covariance(const float *poses, const float *patches, const float *intrinsics, const float *target,
                       const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                       const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1, float *cov,
                       float *depth_var, float *stats, void *ws, size_t ws_bytes, int32_t *info, void *stream);

/* ramp_ba_covariance with the caller's two edge groupings, as ramp_ba_forward_planned takes them                  */
size_t ramp_ba_covariance_planned_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1, int max_patches,
                                                  int max_pairs);
int ramp_ba_covariance_planned(const float *poses, const float *patches, const float *intrinsics, const float *target,
                               const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                               const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1,
                               float *cov, float *depth_var, float *stats, const int32_t *order_k,
                               const int32_t *seg_k, const int32_t *ngroups_k, const int64_t *ukeys_k, int max_patches,
                               const int32_t *order_p, const int32_t *seg_p, const int32_t *ngroups_p, int max_pairs,
                               void *ws, size_t ws_bytes, int32_t *info, void *stream);

/* The map with its uncertainty: ramp_ba_covariance plus, for every patch with at least one factor, its world point, the 3 x 3
 * covariance of that point, the pose-depth cross term it is formed with and its valid-factor count.  cov, depth_var, stats and
 * info are those of ramp_ba_covariance, the same bits (the map stage runs behind the covariance's and only reads them).
 * From the joint inverse of the damped system, with e_k patch k's E row:  cov(xi, z_k) = -Q_k S^-1 e_k.  The point of patch k
 * is ramp_point_cloud's: source frame i = the ii of the patch's factors, world-to-camera pose T_i = (t, R), ray
 * r = ((x - cx) / fx, (y - cy) / fy, 1) at the centre pixel (row 1, column 1: the pixel whose depth the system solves for),
 * inverse depth d, X_w = R' (r / d - t).  Intrinsics: ROW 0, as the system the covariance comes from uses -- where every row is
 * equal X_w is ramp_point_cloud's output bit for bit.  Perturbations as the step's: the LEFT one T <- Exp(xi) T with
 * xi = (translation 3, rotation 3), and d <- d + z:
 *   J_p = R' [ -I | [r / d]x ]  (3 x 6),   J_d = -R' r / d^2  (3 x 1)
 *   point_cov = J_p cov_ii J_p' + depth_var_k J_d J_d' + (J_p c) J_d' + J_d (J_p c)',   c = the rows of cov(xi, z_k) of frame i
 * Outputs, indexed by patch id kk like depth_var; entries of patches without a factor are left as the caller filled them:
 *   point [n_patches][3]
 *   point_cov [n_patches][6]      : xx, xy, xz, yy, yz, zz (symmetric by construction: one value per off-diagonal pair)
 *   pose_depth_cov [n_patches][6] : c; zeros where the source frame is not a free pose (i < t0 or i >= t1, or t1 == t0) --
 *                                   point_cov is then depth_var_k J_d J_d' (rank one)
 *   n_obs [n_patches] int32       : the patch's factors that pass the validity gate
 * Info bit 0 (failed factorisation, as ramp_ba_covariance): point_cov and pose_depth_cov entries the call writes are NaN;
 * point and n_obs are written as usual (point stays finite).  All four outputs are required.  Deterministic: fma chains and
 * fixed reduction trees, no atomics.  The workspace may exceed ramp_ba_covariance's.                                      */
size_t ramp_ba_map_covariance_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1);
int ramp_ba_map_covariance(const float *poses, const float *patches, const float *intrinsics, const float *target,
                           const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                           const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1, float *cov,
                           float *depth_var, float *stats, float *point, float *point_cov, float *pose_depth_cov,
                           int32_t *n_obs, void *ws, size_t ws_bytes, int32_t *info, void *stream);
/* ... with the caller's two edge groupings, as ramp_ba_covariance_planned takes them                                */
size_t ramp_ba_map_covariance_planned_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1, int max_patches,
                                                      int max_pairs);
int ramp_ba_map_covariance_planned(const float *poses, const float *patches, const float *intrinsics, const float *target,
                                   const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                                   const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1,
                                   float *cov, float *depth_var, float *stats, float *point, float *point_cov,
                                   float *pose_depth_cov, int32_t *n_obs, const int32_t *order_k, const int32_t *seg_k,
                                   const int32_t *ngroups_k, const int64_t *ukeys_k, int max_patches,
                                   const int32_t *order_p, const int32_t *seg_p, const int32_t *ngroups_p, int max_pairs,
                                   void *ws, size_t ws_bytes, int32_t *info, void *stream);

/* Stable stream compaction of the map: index [<= n] receives, ASCENDING, the ids i < n of the points with
 *   all six point_cov entries finite,  sqrt(xx + yy + zz) <= max_sigma,  sqrt(depth_var_i) / d_i <= max_rel_depth_sigma
 *   (d_i: the inverse depth of patch i, patches [n][3][P][P] at the centre pixel)  and  n_obs_i >= min_obs,
 * and *count (device int32) their number; index entries behind *count are not written.  A criterion is switched off by
 * passing +inf (the two sigmas) or 0 (min_obs); a NaN or a zero depth never passes a criterion that is on.  The order is the
 * patch order whatever the launch geometry (ballot + ordered prefix, one workgroup).  dyn_rows != NULL: n is clipped to
 * *dyn_rows * per_row on the device (e.g. &dyn[RAMP_DYN_NROW] and M for a device-resident tracker; n is then the capacity). */
int ramp_map_select(const float *point_cov, const float *depth_var, const float *patches, const int32_t *n_obs, int n, int P,
                    const int32_t *dyn_rows, int per_row, float max_sigma, float max_rel_depth_sigma, int min_obs,
                    int32_t *index, int32_t *count, void *stream);

/* group-by for a SMALL key range known to the caller: key = a[e]*mul + (b ? b[e] : 0) - sub must lie
 * in [0, K).  Histogram + one-workgroup scan + scatter + per-segment rank sort (5 short kernels vs a
 * radix sort); same outputs and the same (stable) ordering as ramp_group_by.  ukeys = key + sub.
 * max_groups is an upper bound on G (fewer is a contract violation), and 0 means min(K, E).
 * A key outside [0, K) makes the call yield the empty grouping: *ngroups == 0 and seg_start[0] == 0, so every
 * consumer launches over no group; the other outputs then hold anything, inside their extents.  */
size_t ramp_group_by_small_workspace_bytes(int E, int K);
int ramp_group_by_small(const int64_t *a, const int64_t *b, int64_t mul, int64_t sub, int K, int E,
                        int32_t *order, int32_t *gid, int32_t *seg_start, int64_t *ukeys,
                        int32_t *ngroups, int max_groups, void *ws, size_t ws_bytes, void *stream);

/* cuda_ba.neighbors derived from the per-kk groups (no second sort): every group's edges are
 * ranked by (jj, edge index), whatever the group's length.  max_groups: an upper bound on *ngroups.
 * kj_order (optional, int32 [E]): the factors in that (kk, jj) order -- a factor's temporal neighbours are its
 * neighbours in this list.                                                                          */
int ramp_neighbors_from_groups(const int32_t *order, const int32_t *seg_start, const int32_t *ngroups,
                               const int64_t *jj, int64_t *ix, int64_t *jx, int32_t *kj_order, int E,
                               int max_groups, void *stream);

/* ------------------------------------------------------------------ encoder */
/* flags[0] = any(a != 0), flags[1] = any(b != 0): the "events / image present" tests of
 * ramp/extractor.py:253-254, kept on the device (the reference syncs the host on each).       */
int ramp_any_nonzero(const float *a, long na, const float *b, long nb, int32_t *flags, void *stream);
/* the same test with one result per workgroup and no memset in front: blockflags [2][1024] int32 (row 0: a, row 1: b);
 * returns the number of workgroups nblk (> 0) whose results are valid, or an error code (< 0).  The consumer
 * (ramp_lstm_superstate_blocks) ORs blockflags[r][0 .. nblk).                                                       */
int ramp_any_nonzero_blocks(const float *a, long na, const float *b, long nb, int32_t *blockflags, void *stream);
/* the same launch also zeroes `clear` [clear_bytes] (16-byte aligned, a multiple of 16): the InstanceNorm accumulators of
 * the frame's tower pass (ramp_conv job acc_out / acc_in) without a memset launch in front of the front end          */
int ramp_any_nonzero_blocks_clear(const float *a, long na, const float *b, long nb, int32_t *blockflags, void *clear,
                                  long clear_bytes, void *stream);

/* The two per-pixel LSTM cells and the super-state 1x1 convolution of the SingleScale encoder,
 * fused (ramp/extractor.py:239-259: nn.LSTM x2 on [H*W,1,C] sequences + Conv2d(30->15) x2), on the
 * matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 products): the three matrix-vector products per
 * pixel are batched over 16-pixel tiles.
 *   ev [5][HW], im [3][HW] planar float32
 *   h_ev,c_ev,h_im,c_im [ceil(HW/16)][16 px][4 q][4 t] tile-major recurrent state, unit = 4 t + q (in/out, unit 15 = 0):
 *   a lane's four K-step operands / outputs are one 16-byte access
 *   ss [HW][16] channels-last super-state (in/out, channel 15 = 0)
 *   wfrag: per-lane MFMA fragments of the weights, rampvo_amd/conv_hip.py::pack_lstm_mfma
 *   flags[2]: events / image present (ramp_any_nonzero)
 *   has_state / has_ss: 0 on the first call after reinit_hidden (zero initial state)            */
int ramp_lstm_superstate_tiled(const float *ev, const float *im, float *h_ev, float *c_ev, float *h_im,
                               float *c_im, float *ss, const float *wfrag, const int32_t *flags, int HW,
                               int has_state, int has_ss, void *stream);
/* ramp_lstm_superstate_tiled with the presence flags as ramp_any_nonzero_blocks leaves them (nblk > 0) */
int ramp_lstm_superstate_blocks(const float *ev, const float *im, float *h_ev, float *c_ev, float *h_im,
                                float *c_im, float *ss, const float *wfrag, const int32_t *blockflags, int nblk, int HW,
                                int has_state, int has_ss, void *stream);

/* One scale (1, 2 or 4) of the MultiScale encoder's recurrent front end for one time step
 * (ramp/extractor.py:540-566 with LSTMEncoder :376-385 and SuperStateEncoder :432-463): strided
 * conv_1 on events / image, a per-pixel LSTM step from the zero state (hidden size D = 16*scale),
 * then s <- mix_ev([s ; h_ev]) and, if use_im (the frame's mask), s <- mix_im([s ; h_im]).
 *   ev [5][H][W], im [3][H][W] float32;  state [Hs*Ws][D] channels-last super-state, in/out
 *   weights_host: 12 device pointers (a host array): conv_1 ev W [5][5][K][K], b; conv_1 im W
 *   [3][3][K][K], b; LSTM ev W_ih [4D][5], b_ih+b_hh [4D]; LSTM im W_ih [4D][3], b [4D]; mix ev W^T
 *   [2D][D], b [D]; mix im W^T [2D][D], b [D]    (packed by rampvo_amd/conv_hip.py::pack_ms_scale)
 *   has_state: 0 on the first call after reinit_hidden (zero super-state)                        */
int ramp_ms_lstm_superstate(const float *ev, const float *im, const float *const *weights_host,
                            float *state, int H, int W, int scale, int has_state, int use_im,
                            void *stream);

/* The same step with every matrix-vector product batched over 16 pixels on v_mfma_f32_16x16x4_f32 (exact fp32 products; the
 * summation order differs from the VALU kernel's): wfrag = per-lane A fragments [nfrag][64], wsmall = conv_1 weights /
 * biases and the gate / mix biases (both packed by rampvo_amd/conv_hip.py::pack_ms_scale_mfma; layouts in csrc/conv.hip).
 * state16: optional [Hs*Ws][D] fp16 copy of the new super-state (the conv towers' second / third input).           */
int ramp_ms_lstm_superstate_mfma(const float *ev, const float *im, const float *wfrag, const float *wsmall, float *state,
                                 void *state16, int H, int W, int scale, int has_state, int use_im, void *stream);

/* nn.Conv2d (+ fused neighbours) of the encoder towers as an implicit GEMM on MFMA
 * (ramp/extractor.py:8-57, 60-130; reference: cuDNN).  NHWC activations, padding = K/2.
 *   x [H][W][Cin] (Cin % 16 == 0), y [OH][OW][Cout] (Cout % 32 == 0)
 *   wpk: weights in MFMA fragment order (rampvo_amd/conv_hip.py::pack_conv_weight)
 *   pre_scale/pre_shift [Cin] (optional): x <- relu(x*scale + shift) while loading, i.e. the
 *       producer's InstanceNorm + ReLU fused into this conv
 *   y = [relu]( conv + bias );  if res: y = relu(y + res);  y *= out_scale
 *   stats (optional) [Cout][2][ramp_conv2d_stats_blocks(...)]: per-block partial sum / sum of
 *       squares of (conv + bias), reduced by ramp_in_stats_finalize                                     */
int ramp_conv2d_nhwc(const void *x, const void *wpk, const float *bias, const float *pre_scale,
                     const float *pre_shift, const void *res, void *y, float *stats, int H, int W,
                     int Cin, int Cout, int KH, int KW, int stride, int relu, float out_scale,
                     int dtype, void *stream);

/* One layer of up to TWO independent conv problems of the same shape (the fmap and imap towers read the same input
 * through the same layer shapes and differ in weights, norm and the last layer's Cout) as ONE launch of the
 * LDS-tiled fp16 kernel; fields as the arguments of ramp_conv2d_nhwc (stats: reduce with ramp_in_stats_finalize).
 * RAMP_EUNSUPPORTED for layer shapes the tiled kernel does not cover (use ramp_conv2d_nhwc).                     */
typedef struct ramp_conv_job {
  const void *x, *wpk;
  const float *bias, *pre_scale, *pre_shift;
  const void *res;
  void *y;
  float *stats;
  int32_t Cout, relu;
  float out_scale;
  float act_scale, w_scale;   /* RAMP_CONV_FP8 only: x * act_scale and w * w_scale (wpk packed as e4m3 bytes) are the
                                 MFMA operands, saturating at +-448; the accumulator is divided by their product */
  /* accumulator mode of the InstanceNorm statistics (no ramp_in_stats_finalize launch between two layers): the layer
   * ADDS its per-workgroup partial sums, as exact 2^-20 fixed-point integers, to acc_out [RAMP_IN_ACC_R][Cout][2] uint64
   * (ZERO before the layer; order independent, so reproducible), and takes its input's normalisation from acc_in
   * [RAMP_IN_ACC_R][Cin][2] (+ the pixel count and eps of that InstanceNorm) instead of pre_scale / pre_shift: every
   * consumer workgroup sums the replicas and forms scale = rsqrt(var + eps), shift = -mean * scale itself (Cin <= 128) */
  void *acc_out;
  const void *acc_in;
  float in_count, in_eps;
  /* two-source input (half in): channels [c0, Cin) come from x2 [H][W][Cin - c0], x is [H][W][c0] -- the MultiScale
   * towers' torch.cat((x, x_down2), dim=1) (ramp/extractor.py:300, 306) without the copy; c0 and Cin - c0 multiples of
   * 8, no input normalisation.  x2 = NULL: one source                                                              */
  const void *x2;
  int32_t c0;
  /* fused residual-block tail (half in, accumulator mode; ramp/extractor.py:49-57): with `skip` [H][W][Cin] the input
   * pixel is relu(relu(x * scale + shift) + skip') -- x normalised through acc_in, skip' = skip, or skip normalised through
   * acc_skip (+ skip_count, skip_eps), or the fp16-rounded relu of that (skip_relu) -- rounded to fp16 once: what
   * ramp_norm_add_relu_f16_acc writes, without the launch.  `mat` [H][W][Cin] (stride-1 layers): the pixels are also
   * written out, each by the workgroup that owns it, for the block that takes them as its skip.  NULL: a plain input  */
  const void *skip;
  const void *acc_skip;
  float skip_count, skip_eps;
  int32_t skip_relu;
  void *mat;
} ramp_conv_job;
#define RAMP_IN_ACC_R 8
int ramp_conv2d_nhwc_multi(const ramp_conv_job *jobs, int njobs, int H, int W, int Cin, int KH, int stride,
                           int dtype, void *stream);

/* dtype of ramp_conv2d_nhwc: RAMP_F32 (fp32 in/out, exact fp32 MFMA), RAMP_F16 (half in/out, fp16
 * MFMA, fp32 accumulation / bias / statistics; Cin % 32 == 0) or RAMP_F16|RAMP_IN_F32 (fp32 in,
 * half out: the first layer of the mixed-precision tower, Cin == 16)                            */
#define RAMP_IN_F32 0x10
/* fp16 only: use the direct (one global round trip per tap) kernel instead of the LDS-tiled one;
 * both give identical results (kept for the A/B test)                                          */
#define RAMP_CONV_DIRECT 0x20
/* ramp_conv2d_nhwc_multi only, with RAMP_F16 (half in / out): the layer's products run on the fp8 MFMA
 * (v_mfma_f32_16x16x32_fp8_fp8, OCP e4m3 operands, fp32 accumulate) -- BASELINE configs[4]'s "fp16 encoder on fp8
 * MFMA"; weights packed as e4m3 fragments (rampvo_amd/conv_hip.py::pack_conv_weight mode "f8")                    */
#define RAMP_CONV_FP8 0x40

/* ramp_conv2d_nhwc only, as RAMP_F32 | RAMP_CONV_X3: fp32 in / out at fp32 accuracy on the f16 matrix cores (every operand split
 * into two fp16 numbers, three MFMA products into one fp32 accumulator: csrc/conv.hip::conv_x3_kernel); weights packed by
 * rampvo_amd/conv_hip.py::pack_conv_weight mode "x3"; layer shapes: 3x3 stride 1 (32|64 -> 32|64), 3x3 stride 2 (32 -> 64),
 * 7x7 stride 2 (16 -> 32), else RAMP_EUNSUPPORTED (ramp_conv2d_stats_blocks says so first)                                   */
#define RAMP_CONV_X3 0x80

/* number of per-block partials ramp_conv2d_nhwc writes to `stats` for this layer shape / dtype   */
int ramp_conv2d_stats_blocks(int H, int W, int Cin, int Cout, int KH, int stride, int dtype);
/* 1 where ramp_conv2d_nhwc runs this layer shape / dtype on the LDS-tiled fp16 kernel (the shapes ramp_conv2d_nhwc_multi
 * covers; its partials are per 8 x 16 output tile), 0 where on the direct one                                         */
int ramp_conv2d_tiled(int Cin, int Cout, int KH, int stride, int dtype);
/* The instances of the LDS-tiled fp16 kernel, as its one table lists them (csrc/conv.hip::CONV_TILE_ROWS; for tests that
 * take the table as their parameter list).  ramp_conv2d_tile_rows: the number of rows.  ramp_conv2d_tile_row: row i
 * (0 <= i < rows, else RAMP_EINVAL) -- filter size K, stride S, in_f32 (1: the fp32-input first layer), input channels
 * Cin, NT (16-channel tiles per workgroup: NT = 4 rows want every Cout % 64 == 0), tile height TH (8 or 16 output rows
 * of 16 pixels) and `variants`, the RAMP_TILE_* bits: the instances the row has beside its plain one and the entry
 * points that may select it.  The first row that fits a launch wins.                                                  */
#define RAMP_TILE_FP8 1      /* an fp8 instance (RAMP_CONV_FP8)                              */
#define RAMP_TILE_TAIL 2     /* a fused-block-tail instance (ramp_conv_job.skip)             */
#define RAMP_TILE_SINGLE 4   /* ramp_conv2d_nhwc may select the row                          */
#define RAMP_TILE_PAIRED 8   /* ramp_conv2d_nhwc_multi may select the row                    */
int ramp_conv2d_tile_rows(void);
int ramp_conv2d_tile_row(int i, int *K, int *S, int *in_f32, int *Cin, int *NT, int *TH, int *variants);
/* the row ramp_conv2d_nhwc_multi would launch for these arguments, without launching (the same validation and the same
 * selection, tile height included: the code the launch itself runs): its index >= 0; -1 - row where the two towers' 7x7
 * first layer goes to the dual kernel instead of that row (row 0, so -1: the same number as RAMP_EINVAL -- the launch's
 * own return code tells the two apart); or the launch's error code (RAMP_EINVAL, RAMP_EUNSUPPORTED).  The instance of
 * the row is the fp8 one with RAMP_CONV_FP8, the tail one where a job has `skip`, else the plain one.                  */
int ramp_conv2d_multi_row(const ramp_conv_job *jobs, int njobs, int H, int W, int Cin, int KH, int stride, int dtype);

/* InstanceNorm2d statistics (affine=False, biased variance): scale = rsqrt(var+eps),
 * shift = -mean*scale, from the per-block partials of ramp_conv2d_nhwc                         */
int ramp_in_stats_finalize(const float *partial, int nblk, int C, float count, float eps, float *scale,
                           float *shift, void *stream);

/* accumulator-mode counterparts: ramp_norm_add_relu_f16 with y's (and a normalised skip's) statistics taken from their
 * accumulators, and the (scale, shift) arrays of an accumulator for a consumer without that path                      */
int ramp_norm_add_relu_f16_acc(const void *y, const void *acc_y, float count_y, float eps_y, const void *skip,
                               const void *acc_skip, float count_skip, float eps_skip, void *out, long n, int C,
                               int skip_relu, void *stream);
int ramp_in_acc_finalize(const void *acc, int C, float count, float eps, float *scale, float *shift, void *stream);

/* out = relu(x*s + h)   (InstanceNorm + ReLU materialised where a skip connection needs it)    */
int ramp_affine_relu(const float *x, const float *s, const float *h, float *out, long n, int C,
                     void *stream);

/* half-storage variants (x, y, skip, out are half; scale/shift stay fp32) */
int ramp_affine_relu_f16(const void *x, const float *s, const float *h, void *out, long n, int C,
                         void *stream);
/* skip_relu: the skip operand is relu(skip*ss + hs) (an InstanceNorm + ReLU that was never materialised) */
int ramp_norm_add_relu_f16(const void *y, const float *sy, const float *hy, const void *skip,
                           const float *ss, const float *hs, void *out, long n, int C, int skip_relu,
                           void *stream);

/* residual-block tail: out = relu( skip' + relu(y*sy + hy) ), skip' = skip*ss + hs if ss else skip
 * (ramp/extractor.py:49-57 with the norms folded in)                                           */
int ramp_norm_add_relu(const float *y, const float *sy, const float *hy, const float *skip,
                       const float *ss, const float *hs, float *out, long n, int C, void *stream);

/* ---------------------------------------------------------- update operator */
/* Row-fused glue of the update operator (ramp/net.py:69-90, ramp/blocks.py:15-50); rows are
 * [E][384].  `dtype` is the GEMM I/O dtype T (RAMP_F16 under MIXED_PRECISION); the hidden state
 * is fp32 as under the reference's autocast.
 *
 * ramp_upd_row_fuse: t = A[rowA(e)] + B[rowB(e)] + C[rowC(e)]; optional LayerNorm(ln_w, ln_b, eps)
 *   (nn.LayerNorm(384, eps=1e-3), net.py:45,49-52,60) and ReLU; written as fp32 (out_f32) and/or
 *   T (out_t).  rowB(e) = idxB[e] (int64) or idxB32[e] or e, taken modulo modB when modB > 0
 *   (the `kk % (M*mem)` ring-buffer gather of Ramp_vo.py:282); rowC likewise.  rowA(e) = idxA[e] or e;
 *   idxA[e] < 0 reads a zero row: the tracker keeps the hidden state of the PREVIOUS graph and maps
 *   the current edges into it (removed edges drop out, new edges start at zero: Ramp_vo.py:204-205,
 *   268-270) instead of compacting / growing the [E,384] state every frame.  A fp32, B/C of T. */
int ramp_upd_row_fuse(const float *A, const int64_t *idxA, const void *B, const void *C, const int64_t *idxB,
                      const int32_t *idxB32, long modB, const int64_t *idxC, const int32_t *idxC32,
                      const float *ln_w, const float *ln_b, float eps, int relu, float *out_f32,
                      void *out_t, int E, int dtype, void *stream);
/* out[e] = idx[e] >= 0 ? X[idx[e]] : 0  -- `mask_ix * net[:, ix]` of net.py:78-82 (X fp32, out T) */
int ramp_upd_gather_mask(const float *X, const int64_t *idx, void *out, int E, int dtype, void *stream);
/* GatedResidual tail (blocks.py:30-31): t = X + sigmoid(G) * R, optional LayerNorm; written as
 * fp32, T and ReLU(T) (each optional) */
int ramp_upd_gated(const float *X, const void *G, const void *R, const float *ln_w, const float *ln_b,
                   float eps, float *out_f32, void *out_t, void *out_relu_t, int E, int dtype,
                   void *stream);
/* heads + Ramp_vo.update's target / filter_features (net.py:64-67, Ramp_vo.py:288-294,
 * utils.py:557-570): hw [E][4] = (delta_x, delta_y, w_x, w_y) pre-sigmoid, coords [E][2][P][P];
 * target = centre + delta, weight = sigmoid(w) zeroed outside [0,wd]x[0,ht]; delta optional    */
int ramp_upd_heads(const void *hw, const float *coords, float *target, float *weight, float *delta,
                   int E, int P, float wd, float ht, int dtype, void *stream);
/* SoftAgg core over the stacked [f | g] GEMM output fg [E][768] (single-pass online softmax):
 * y[g] = sum_{e in g} softmax_e(g[e]) * f[e]  (blocks.py:44-45)                                */
int ramp_upd_segment_softmax(const void *fg, const int32_t *order, const int32_t *seg_start,
                             const int32_t *ngroups, void *y, int max_groups, int dtype, void *stream);

/* HOST helper (pointers are host memory, nothing is launched): the factor-graph edit of
 * Ramp_vo.keyframe() (ramp/Ramp_vo.py:247-274 + remove_factors :203-208) for one outcome of the motion
 * test, one pass over the host mirror.  k_remove < 0: no keyframe is dropped.  out [4][cap] int64 =
 * (ii, jj, kk, hidden-state row) of the factors kept; rows_in NULL = identity.  Returns their number.  */
int ramp_graph_edit_host(const int64_t *ii, const int64_t *jj, const int64_t *kk, const int64_t *rows_in, int E,
                         int M, int k_remove, int n_after, int removal_window, int64_t *out, int cap,
                         int64_t *ranges /* optional [4]: min/max kk, min/max frame index of the kept factors */);

/* ------------------------------------------------ fused update-operator GEMM chains (fp16) */
/* gru[1..3] of the update operator (ramp/net.py:49-54; GatedResidual: ramp/blocks.py:15-31) as ONE
 * launch: x -> x + sigmoid(Wg x) * W2 relu(W1 x) -> LayerNorm -> the same again, 6 Linear layers with the
 * 64-row activation tile resident in LDS, fp16 MFMA / fp32 accumulate.
 *   x32 [E][384] fp32 (output of gru[0], the caller's LayerNorm);  out32 [E][384] fp32;
 *   relu_t [E][384] fp16 = relu(out32), the heads' input
 *   wp_host[6]: fp16 weights of (g1.gate, g1.res[0], g1.res[2], g2.gate, g2.res[0], g2.res[2]) packed in
 *   MFMA fragment order [K/32][N/16][64 lanes][8] (lane (q, j): W[16 nt + j][32 ks + 8 q ..]);
 *   bias_host[6]: fp32 [384] each (host arrays of device pointers); ln_w, ln_b, eps: gru[2].
 *   add_t != NULL: the kernel first forms x = LayerNorm(x32 + add_t[add_idx[e]]; pre_w, pre_b, pre_eps) itself
 *   -- the expand-and-add of the second SoftAgg (ramp/net.py:85) and gru[0] -- add_t [groups][384] fp16,
 *   add_idx [E] int32; NULL: x32 is already the output of gru[0].                                       */
int ramp_upd_gru(const float *x32, const void *add_t, const int32_t *add_idx, const float *pre_w, const float *pre_b,
                 float pre_eps, const void *const *wp_host, const float *const *bias_host, const float *ln_w,
                 const float *ln_b, float eps, float *out32, void *relu_t, int E, void *stream);
/* ramp_upd_gru with the two heads and target / weight formed from the result tile in the same launch
 * (ramp/net.py:87-90 `d`, `w`; ramp/Ramp_vo.py:291-297: target = centre + delta, weight = sigmoid, zero outside the
 * image): heads_w [4][384] fp16 (d.weight rows 0..1, w.weight rows 0..1), heads_b [4], coords [E][2][P][P],
 * target / weight [E][2] fp32.  The heads' fp16 input relu(out32) is not written.  Same arithmetic as
 * ramp_upd_heads_linear up to the order of the 384-term sums.                                              */
int ramp_upd_gru_heads(const float *x32, const void *add_t, const int32_t *add_idx, const float *pre_w, const float *pre_b,
                       float pre_eps, const void *const *wp_host, const float *const *bias_host, const float *ln_w,
                       const float *ln_b, float eps, float *out32, const void *heads_w, const float *heads_b,
                       const float *coords, float *target, float *weight, int E, int P, float wd, float ht, void *stream);
/* Rows per workgroup (64 or 80) of the gru launch for E factors, the rule the launch itself applies: the tile that needs fewer
 * rounds of one workgroup per CU (ties: 64; CU count of the current device, 256 without one).  E_hint: the caller's estimate
 * of the live count where E is only a launch bound (the device-resident step) -- it replaces E when 0 < E_hint < E.  The
 * frame pipeline asks this to place the next frame's front end around the launch (rampvo_amd/frame_pipeline.py).         */
int ramp_upd_gru_tile_rows(int E, int E_hint);
size_t ramp_upd_mlp_lds_bytes(void);

/* net_out[e] = net_in[e] + Lb(relu(La(idx[e] >= 0 ? net_in[idx[e]] : 0)))  -- the temporal-neighbour MLPs
 * c1 / c2 (ramp/net.py:43-46, 77-82) with the gather, both Linear layers and the residual add in one
 * launch.  net_in != net_out (other workgroups gather from net_in); out_t: optional fp16 copy of
 * net_out.  wa / wb packed like ramp_upd_gru's weights, ba / bb fp32 [384].                          */
int ramp_upd_nbr(const float *net_in, const int64_t *idx, const void *wa, const float *ba, const void *wb,
                 const float *bb, float *net_out, void *out_t, int E, void *stream);

/* The whole correlation MLP and Update.norm in one launch (ramp/net.py:57-62, 71-74):
 *   c = Linear3(relu(LayerNorm(Linear2(relu(Linear1(corr))))));  net_out = LayerNorm_norm((net[net_map] + inp[inp_idx % inp_mod]) + c)
 * corr [E][corr_k] fp16 (corr_k a multiple of 32: 896 = 882 + zero padding); w1 packed [corr_k/32][24][64][8] from the
 * zero-padded weight, w2 / w3 packed like ramp_upd_gru's weights, biases fp32 [384] (fp16-rounded values); net [*][384] fp32 or
 * NULL (zeros), net_map [E] (-1: zero row) or NULL (identity); inp [*][384] fp16, inp_idx NULL = identity.  Linear outputs
 * are rounded to fp16 where the reference's autocast makes them half tensors.                                             */
int ramp_upd_corr_mlp(const void *corr, int corr_k, const void *w1, const float *b1, const void *w2, const float *b2,
                      const void *w3, const float *b3, const float *ln_w, const float *ln_b, float ln_eps,
                      const float *net, const int64_t *net_map, const void *inp, const int64_t *inp_idx, long inp_mod,
                      const float *norm_w, const float *norm_b, float norm_eps, float *net_out, int E, void *stream);

/* fp16 path: the two heads' Linear layers (ramp/net.py:64-66) + ramp_upd_heads's epilogue in one launch:
 * hw = relu_t [E][384] @ heads_w [4][384]^T + heads_b (rounded to fp16 like the GEMM's output), then target = patch
 * centre of coords + hw[:2], weight = sigmoid(hw[2:]) zeroed where target is outside [0,wd]x[0,ht].     */
int ramp_upd_heads_linear(const void *relu_t, const void *heads_w, const float *heads_b, const float *coords,
                          float *target, float *weight, int E, int P, float wd, float ht, void *stream);

/* SoftAgg front half (ramp/blocks.py:42-46) in one launch: x = x32[e] (+ add_t[add_idx[e]], written to x32_out
 * when given; x32_out may be x32);  fg[e] = [ f(x) | g(x) ]  fp16 [E][768].  wf / wg packed like ramp_upd_gru's
 * weights, bf / bg fp32 [384].                                                                        */
int ramp_upd_fg(const float *x32, const void *add_t, const int32_t *add_idx, float *x32_out, const void *wf,
                const float *bf, const void *wg, const float *bg, void *fg, int E, void *stream);

/* nn.Linear(384, 384) on a small fp16 table: y[r] = fp16(x[r] W^T + b) -- SoftAgg's `h` layer on the group table
 * (ramp/blocks.py:46-47), the one GEMM of the fused update operator that used to be a library call.  w_packed like
 * ramp_upd_gru's weights, bias fp32 [384]; rows_dev (optional, device int32): only rows < *rows_dev are computed.   */
int ramp_upd_linear(const void *x, const void *w_packed, const float *bias, void *y, int rows, const int32_t *rows_dev,
                    void *stream);

/* SoftAgg (ramp/blocks.py:33-50: y = scatter_sum(f(x) * scatter_softmax(g(x))), h(y)) of the fp16 path WITHOUT the
 * [E, 768] rows of [f | g] going through memory: ramp_upd_softagg walks the grouping's sorted factor list (`order`,
 * groups = contiguous runs; `gid`: factor -> group), 80 positions per workgroup, forms g and f on the same tile and leaves
 * one fragment (running maximum, sum, weighted sum)[384] per run of a group inside a 20-position block in
 * frag[group + position / 20] (ramp_upd_softagg_frag_rows(E, max_groups) rows of 3 x 384 floats); ramp_upd_softagg_finish
 * merges a group's fragments in slot order (seg_start = the grouping's segment starts), y = a / z, and applies h:
 * hy [max_groups][384] fp16 (rows >= *ngroups are zero).  x = x32 (+ add_t[add_idx]); weights as ramp_upd_fg /
 * ramp_upd_linear.  Replaces ramp_upd_fg + ramp_upd_segment_softmax + ramp_upd_linear (same values up to the order of
 * the fp32 additions).                                                                                             */
size_t ramp_upd_softagg_frag_rows(int E, int max_groups);
int ramp_upd_softagg(const float *x32, const void *add_t, const int32_t *add_idx, const int32_t *order,
                     const int32_t *gid, const void *wf, const float *bf, const void *wg, const float *bg, float *frag,
                     int E, void *stream);
int ramp_upd_softagg_finish(const float *frag, const int32_t *seg_start, const int32_t *ngroups, const void *wh,
                            const float *bh, void *hy, int max_groups, void *stream);

/* ---------------------------------------------------------------- the update operator at fp32 accuracy (MIXED_PRECISION off)
 *
 * The same chains for fp32 features (ramp/net.py:69-90 without autocast): every Linear layer is formed on the f16 matrix
 * cores from split operands (x = xh + xl, three f16 products into one fp32 accumulator: csrc/update_x3.hip), nothing
 * between layers is rounded to fp16; biases, LayerNorm, gate, residual stream, the SoftAgg tables and the heads are fp32.
 * Agreement with an fp32 GEMM chain: ~1e-6 of the output scale (22-bit operands, fp32 accumulation).  All tables and
 * rows are float; weights `*w*` are "x3 packs" of an nn.Linear weight W [384][K] (K a multiple of 32):
 *     [K/32][24][2][64 lanes][8] fp16 -- plane 0 = fp16(W 2^s), plane 1 = fp16(W 2^s - plane 0), s the power of two that
 *     puts max |W| into [2^12, 2^13); lane (q, j) of fragment (ks, nt) holds W[16 nt + j][32 ks + 8 q .. + 8];
 *     followed by one float, 2^-s   (rampvo_amd/update_fused.py::pack_linear_x3).
 * Linear inputs must stay below 65504 in magnitude (as on the MIXED_PRECISION path).  Arguments otherwise as the
 * ramp_upd_* function of the same name.                                                                              */
int ramp_x3_corr_mlp(const float *corr, int corr_k, const void *w1, const float *b1, const void *w2, const float *b2,
                     const void *w3, const float *b3, const float *ln_w, const float *ln_b, float ln_eps, const float *net,
                     const int64_t *net_map, const float *inp, const int64_t *inp_idx, long inp_mod, const float *norm_w,
                     const float *norm_b, float norm_eps, float *net_out, int E, void *stream);
int ramp_x3_nbr(const float *net_in, const int64_t *idx, const void *wa, const float *ba, const void *wb, const float *bb,
                float *net_out, int E, void *stream);
/* fg [E][768] fp32 = [f(x) | g(x)], x = x32 (+ add_t[add_idx], fp32 table; written to x32_out when given)              */
int ramp_x3_fg(const float *x32, const float *add_t, const int32_t *add_idx, float *x32_out, const void *wf, const float *bf,
               const void *wg, const float *bg, float *fg, int E, void *stream);
/* y [max_groups][384] fp32: the softmax-weighted segment sums of ramp_x3_fg's rows (ramp/blocks.py:46-48; 8 row lanes per
 * group, merged in lane order); rows >= *ngroups are zero                                                            */
int ramp_x3_segment_softmax(const float *fg, const int32_t *order, const int32_t *seg_start, const int32_t *ngroups, float *y,
                            int max_groups, void *stream);
/* y[r] = x[r] W^T + b on a table of rows (SoftAgg's `h`); rows_dev (optional, device int32): only rows < *rows_dev      */
int ramp_x3_linear(const float *x, const void *w_packed, const float *bias, float *y, int rows, const int32_t *rows_dev,
                   void *stream);
/* gru (LayerNorm, GatedResidual, LayerNorm, GatedResidual) with x = LayerNorm_pre((x32 (+ add0_t[add0_idx])) + add_t[add_idx])
 * when add_t is given; relu32 (optional) = relu(out32); heads_w [4][384] / heads_b [4] fp32 (optional): the d / w heads and
 * target / weight as ramp_upd_gru_heads, in fp32                                                                      */
int ramp_x3_gru(const float *x32, const float *add0_t, const int32_t *add0_idx, const float *add_t, const int32_t *add_idx,
                const float *pre_w, const float *pre_b, float pre_eps, const void *const *wp_host, const float *const *bias_host,
                const float *ln_w, const float *ln_b, float eps, float *out32, float *relu32, int E, const float *heads_w,
                const float *heads_b, const float *coords, float *target, float *weight, int P, float wd, float ht, void *stream);

/* ---------------------------------------------------------------- device-resident tracking step
 *
 * Ramp_vo.__call__ in steady state (ramp/Ramp_vo.py:327-410): the frame's state stores, update() (:276-310:
 * reproject, corr, the update operator, two BA iterations, point cloud) and keyframe() (:237-274: the motion test, the
 * removal of a keyframe and of old factors) followed by the NEXT frame's append_factors (:194-201, :312-325) -- as ONE
 * host call that never reads the device.  The reference decides keyframe() on the host (`.item()`), so every frame
 * waits for the GPU to drain; here the decision is taken by a kernel and everything that depends on it -- the row a
 * frame is stored to, the factor count, the optimisation window -- is read by the kernels from a block of int32 words
 * in device memory (`dyn`), their launch sizes being capacity bounds.  The host mirrors the state lazily (dyn_host).
 */
#define RAMP_DYN_WORDS 32
#define RAMP_DYN_N 0        /* keyframes incl. the newest frame: Ramp_vo.n during update() / keyframe(), BA's t1   */
#define RAMP_DYN_NROW 1     /* row the NEXT frame is stored to (Ramp_vo.n before its `n += 1`)                    */
#define RAMP_DYN_E 2        /* factors in the current graph (incl. the ones the newest frame added)               */
#define RAMP_DYN_KLO 3      /* lower bound of kk (offset of the counting group-by)                                */
#define RAMP_DYN_FLO 4      /* lowest frame index in ii / jj                                                      */
#define RAMP_DYN_W 5        /* pair keys are jj * W + ii                                                          */
#define RAMP_DYN_REMOVED 6  /* outcome of the last keyframe test: 1 = keyframe K was dropped                      */
#define RAMP_DYN_K 7        /* the keyframe that test looked at (n - KEYFRAME_INDEX)                              */
#define RAMP_DYN_NPREV 8    /* Ramp_vo.n when the test ran                                                        */
#define RAMP_DYN_EPREV 9    /* factors before the edit                                                            */
#define RAMP_DYN_EKEPT 10   /* factors the edit kept (next graph = kept ++ new)                                   */
#define RAMP_DYN_STATUS 11  /* sticky bits, RAMP_STATUS_* below                                                   */
#define RAMP_DYN_NLOG 12    /* entries written to the delta log                                                   */
#define RAMP_DYN_FRAME 13   /* `counter` of the last frame stepped (tags the host's lazy copy)                    */
#define RAMP_DYN_MEDOK 14   /* 1: ramp_track.median holds the depth median of the three newest frames (set beside the
                             * motion test, cleared by an update-only step; 0 when the host hands the state over)     */
#define RAMP_DYN_FRAME2 31  /* = RAMP_DYN_FRAME, in the other half of the block: the two differ in a torn host copy         */
#define RAMP_TRACK_LOG 12   /* floats per delta-log entry: t1, t0 (as int32 bit patterns), dP[7], pad             */
/* the bits of the RAMP_DYN_STATUS word: set by the kernel that meets the condition, never cleared by a step */
#define RAMP_STATUS_BA_STEP_DROPPED 1    /* BA dropped a pose step (ramp_ba_forward's info bit 0)                    */
#define RAMP_STATUS_BA_PAIR_OVERFLOW 2   /* BA's pair list overflowed (ramp_ba_forward's info bit 1)                 */
#define RAMP_STATUS_FACTORS_FULL 4       /* factor capacity exceeded                                                 */
#define RAMP_STATUS_KEY_RANGE 8          /* group-by key out of range                                                */
#define RAMP_STATUS_LOG_FULL 16          /* delta log full                                                           */
#define RAMP_STATUS_E_BOUND 32           /* a step's E_bound was below the live factor count                         */
#define RAMP_STATUS_FRAMES_FULL 64       /* frame buffers full (n_rows)                                              */
#define RAMP_STATUS_GATE_TIMEOUT 128     /* a gate wait (ramp_stream_wait_flag) timed out: the front end ran unordered */

/* A pose record (ramp_track_publish): 32 words = two 64-byte halves, written to slot `counter % ring_cap` of a ring in pinned
 * host memory, one record per accepted frame.  The frame tag sits in both halves (as in `dyn`): the first half is stored,
 * then a system-scope fence, then the second half -- a host copy whose two tags differ is torn.  Integer words are int32,
 * POSE / INV are float bit patterns, TSTAMP is a double split into its low and high word.                               */
#define RAMP_POSE_WORDS 32
#define RAMP_POSE_FRAME 0       /* `counter` of the frame (the record's tag)                                          */
#define RAMP_POSE_N 1           /* Ramp_vo.n when the frame's update() ran                                            */
#define RAMP_POSE_E 2           /* live factors behind the frame's graph edit (Ramp_vo.peek()'s E)                    */
#define RAMP_POSE_STATUS 3      /* the sticky status word (RAMP_DYN_STATUS) as the frame left it                      */
#define RAMP_POSE_DROPPED 4     /* 1: this frame's keyframe test dropped a keyframe                                   */
#define RAMP_POSE_T1 5          /* the delta entry that test wrote: the dropped frame ...                             */
#define RAMP_POSE_T0 6          /* ... and the frame its pose is chained to (both -1 when DROPPED is 0)               */
#define RAMP_POSE_KF_TSTAMP 7   /* `counter` of the frame whose pose row is published (the newest keyframe)           */
#define RAMP_POSE_TSTAMP 8      /* [2] the caller's time stamp of the frame (Ramp_vo.tlist), a double: low, high word  */
#define RAMP_POSE_POSE 16       /* [7] the newest frame's pose as stored: world -> camera (tx ty tz qx qy qz qw)       */
#define RAMP_POSE_INV 23        /* [7] its inverse, camera -> world: the convention of Ramp_vo.terminate()            */
#define RAMP_POSE_FRAME2 31     /* = RAMP_POSE_FRAME, in the other half                                               */
#define RAMP_TRAJ_UNRESOLVED 1  /* ramp_trajectory_resolve's status bit: a frame is neither a keyframe nor reachable
                                   through the delta logs (its row is the identity)                                      */

#define RAMP_TRACK_COMMIT 1    /* store the front end's outputs as frame NROW first                               */
#define RAMP_TRACK_UPDATE 2    /* Ramp_vo.update()                                                                */
#define RAMP_TRACK_KEYFRAME 4  /* Ramp_vo.keyframe() + the next frame's append_factors + its plan                 */
#define RAMP_TRACK_MM_GIVEN 8  /* (tests) keyframe(): take the two flow magnitudes from t->mm instead of computing */
#define RAMP_TRACK_WRAP_COORDS 16 /* (measurement) move every reprojection into the target plane by whole plane sizes
                                     before the correlation launch: bench.py's roofline leg with every factor live    */
#define RAMP_TRACK_UPDATE_PRE 64   /* the part of update() in front of the update operator: reprojection + correlation        */
#define RAMP_TRACK_UPDATE_POST 128 /* the part behind it: two BA iterations + point cloud, from t->target / t->weight.  With
                                      PRE and POST as two calls the caller runs the operator in between on t->coords / t->corr
                                      and leaves the new hidden state in t->net[0], target / weight in their buffers -- the
                                      fp32 path (MIXED_PRECISION off), whose Linear layers are library GEMMs; it still never
                                      reads the device (launch sizes = E_bound)                                          */
#define RAMP_TRACK_COMPACT_COORDS 32 /* (measurement) the same, and every patch with unit pixel spacing around its centre (a
                                     converged tracker's factors: one 10 x 10 union window per level)                  */

/* The weights of the update operator in the formats its fused chains read: fp16 features -- Linear weights as fp16 MFMA
 * fragments (ramp_upd_gru), their biases fp32 [384] holding fp16-rounded values, heads_w [4][384] fp16; fp32 features -- "x3
 * packs" (ramp_x3_*) with fp32 biases, heads_w [4][384] fp32.  corr_w1 is packed from the weight zero-padded to 896 columns;
 * LayerNorm parameters are fp32 in both.  rampvo_amd/update_fused.py::FusedUpdate.record() fills it once per set of weights. */
typedef struct ramp_track_weights {
  const void *corr_w1, *corr_w2, *corr_w3;
  const float *corr_b1, *corr_b2, *corr_b3, *corr_ln_w, *corr_ln_b, *norm_w, *norm_b;
  const void *c1_wa, *c1_wb, *c2_wa, *c2_wb;
  const float *c1_ba, *c1_bb, *c2_ba, *c2_bb;
  const void *kk_wf, *kk_wg, *kk_wh, *ij_wf, *ij_wg, *ij_wh;
  const float *kk_bf, *kk_bg, *kk_bh, *ij_bf, *ij_bg, *ij_bh;
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
  const void *gru_w[6];
  const float *gru_b[6];
  const void *heads_w;
  const float *heads_b;
  float corr_ln_eps, norm_eps, ln1_eps, ln2_eps;
} ramp_track_weights;

/* One call of the whole update operator (ramp/net.py:69-90): the launch sequence the device-resident step makes, for a
 * caller that knows its row count.  fp32 = 0: fp16 features, the ramp_upd_* chains -- corr_mlp, nbr (c1), nbr (c2), softagg +
 * softagg_finish over the patch groups, the same over the pair groups with hkk[kk_gid] added on the way, gru;  fp32 = 1: the
 * ramp_x3_* chains, each SoftAgg as fg + segment_softmax + linear.  T is half / float accordingly.
 *   corr [E][896] T (882 + zero tail);  net_prev [*][384] fp32 or NULL (zeros), row net_map[e] of it per factor (-1: zero
 *   row; NULL: row e);  inp [*][384] T, row inp_idx[e] % inp_mod (inp_idx NULL: row e);
 *   state[2]: [E][384] fp32 scratch, distinct, state[0] != net_prev;  net_out [E][384] fp32 (may be state[1] or net_prev);
 *   relu_out [E][384] T = relu(net_out), the input of the heads -- or, with coords [E][2][P][P] given, target / weight
 *   [E][2] formed by the gru launch (image size wd x ht) and relu_out optional;
 *   kk_* / ij_*: the factors grouped by patch / by pose pair (ramp_group_by: order [E], gid [E], seg [groups + 1], ngroups
 *   [1] on the device, cap >= *ngroups);  ix / jx [E]: the temporal neighbours (-1: none);
 *   hkk [kk_cap][384], hij [ij_cap][384] T: the SoftAgg tables;  sagg_frag (fp16 features):
 *   [ramp_upd_softagg_frag_rows(E, max(kk_cap, ij_cap))][3][384];  fg [E][768], ykk [kk_cap][384], yij [ij_cap][384] (fp32
 *   features; hkk / hij rows >= *ngroups are left alone there);
 *   E_hint: ramp_track.E_hint's meaning (0: none).
 * RAMP_EINVAL, before anything is launched, unless every pointer the precision needs is there; E = 0 launches nothing. */
typedef struct ramp_update_args {
  const ramp_track_weights *w;
  const void *corr;
  const float *net_prev;
  const int64_t *net_map;
  const void *inp;
  const int64_t *inp_idx;
  long inp_mod;
  float *state[2];
  float *net_out;
  void *relu_out;
  const float *coords;
  float *target, *weight;
  const int32_t *kk_order, *kk_gid, *kk_seg, *kk_ngroups, *ij_order, *ij_gid, *ij_seg, *ij_ngroups;
  const int64_t *ix, *jx;
  float *sagg_frag, *fg, *ykk, *yij;
  void *hkk, *hij;
  int kk_cap, ij_cap, E, E_hint, P, fp32;
  float wd, ht;
} ramp_update_args;
int ramp_update_forward(const ramp_update_args *args, void *stream);

typedef struct ramp_track {
  /* configuration (cfg: PATCHES_PER_FRAME, PATCH_LIFETIME, REMOVAL_WINDOW, OPTIMIZATION_WINDOW, KEYFRAME_INDEX,
   * KEYFRAME_THRESH, MOTION_MODEL (1 DAMPED_LINEAR, 2 copy), MOTION_DAMPING) */
  int M, P, mem, n_rows, patch_lifetime, removal_window, opt_window, keyframe_index, motion_model;
  int feat_h, feat_w;                 /* level-1 feature plane (level 4 is feat_h/4 x feat_w/4)                  */
  int E_cap, kk_cap, ij_cap, kkey_cap, pkey_cap, log_cap, m_cap;
  float motion_damping, pad0;
  double keyframe_thresh;
  /* tracker state (ramp/Ramp_vo.py:54-100), layouts as in rampvo_amd/Ramp_vo.py */
  int32_t *dyn;                       /* [RAMP_DYN_WORDS] */
  float *poses, *patches, *intrinsics, *points;
  int64_t *tstamps, *index_map;
  const int64_t *ixm;                 /* [n_rows * M]: patch -> source frame                                     */
  void *colors, *imap, *gmap, *fmap1, *fmap2;
  const float *lmbda;
  /* the front end's outputs of the frame being committed */
  const void *fe_colors, *fe_imap, *fe_gmap, *fe_fmap1, *fe_fmap2;
  float *fe_patches;
  /* factor graph, double buffered: [4][E_cap] int64 rows (ii, jj, kk, hidden-state row) */
  int64_t *graph[2];
  /* graph plan */
  int32_t *kk_order, *kk_gid, *kk_seg, *kk_ngroups, *ij_order, *ij_gid, *ij_seg, *ij_ngroups;
  int64_t *kk_ukeys, *ij_ukeys, *ix, *jx;
  int32_t *kj;                        /* [E_cap] factors in (kk, jj) order (a by-product of the neighbour search)  */
  void *plan_ws;                      /* ZERO before the first plan (each plan leaves its histograms cleared)      */
  size_t plan_ws_bytes;
  /* update operator */
  ramp_track_weights w;
  float *coords;                      /* [E_cap][2][P][P] */
  void *corr;                         /* [E_cap][896] fp16 */
  float *net[3];                      /* [E_cap][384] fp32: [0] the hidden state (in: previous, out: new), [1], [2] scratch */
  void *fg, *ykk, *hkk, *yij, *hij;   /* the SoftAgg tables of ramp_update_args; fg / ykk / yij are read and written by
                                       * fp32-feature steps only (fp16 steps need hkk / hij and sagg_frag)             */
  float *sagg_frag;                   /* fp16 features: [ramp_upd_softagg_frag_rows(E_cap, max(kk_cap, ij_cap))][3][384], the
                                       * two SoftAggs run as ramp_upd_softagg + _finish                                   */
  float *target, *weight;             /* [E_cap][2] */
  /* bundle adjustment */
  void *ba_ws;
  size_t ba_ws_bytes;
  /* keyframe() */
  float *mm;                          /* [2] flow magnitudes of the motion test */
  float *median;                      /* optional [1]: depth initialisation of the next frame (ramp/Ramp_vo.py:370-371), computed in
                                       * the motion test's launch instead of at the head of the next step (KEYFRAME_INDEX >= 4:
                                       * the three newest frames are the same whether or not the test drops a keyframe)       */
  float *dlog;                        /* [log_cap][RAMP_TRACK_LOG] */
  int32_t *edit_ws;                   /* [3 * ceil(E_cap / 256) + 8]  */
  int32_t *dyn_host;                  /* optional pinned host copy of dyn, refreshed asynchronously after each step */
  int32_t *dyn_host_dev;              /* optional: device address of dyn_host (ramp_host_device_pointer, resolved once):
                                       * the plan's last launch then writes the copy itself                          */
  /* optional hipEvent_t handles recorded on `stream` by ramp_track_step (measurement only: bench.py's roofline legs):
   * [0] before / [1] after the correlation kernel, [2] after the update operator's last chain (gru), [3] before /
   * [4] after bundle adjustment                                                                                  */
  void *probe[5];
  int32_t E_hint;                     /* optional (> 0): the caller's estimate of the live factor count (E_bound is an upper
                                       * bound): picks the gru launch's tile (64 / 80 rows per workgroup)                    */
  uint32_t gate_seq;                  /* with gate_flag: the value stored into it where the next frame's front end may start:
                                       * by the first SoftAgg launch (fp16 features), by a one-thread launch in front of the
                                       * correlation launch (fp32 features)                                               */
  int32_t feat_fp32;                  /* 0: fp16 features (imap / gmap / fmap rows of 2-byte elements, chunked [h][C/32][w][32] pyramid
                                       * planes, corr [E_cap][896] fp16); 2: fp32 features, chunked planes of split fp16 pairs
                                       * (RAMP_CORR_X2: corr_mfma_kernel<CorrX2>; feat_plain must be 0), everything else as 1;
                                       * 1: fp32 features, planes chunked as [h][C/16][w][16]
                                       * (feat_plain = 0) or plain NHWC, corr [E_cap][896] fp32 by corr_mfma_kernel<float>
                                       * or corr_kernel<float> (corr_f32_mfma), operator csrc/update_x3.hip               */
  int32_t feat_plain;                 /* 1: the pyramid planes are plain NHWC [h][w][128] rows instead of the
                                       * chunked [h][C/32][w][32] layout -- feature planes whose width is no multiple of 16 or
                                       * whose height is no multiple of 4 (ramp_pyramid_pack's shapes): corr_mfma_kernel<half, false>  */
  uint32_t *gate_flag;                /* optional signal word (ramp_signal_alloc): "the next frame's front end may start"  *
                                       * without a packet on this stream -- the other stream waits with                    *
                                       * ramp_stream_wait_flag (a hipEventRecord costs ~5 us between two kernels of the   *
                                       * recording stream, tools/mb/stream_signal.hip); takes the place of gate_event     */
  int32_t *fmap1_slot;                /* optional [mem] int32, a permutation of 0 .. mem - 1 (identity at hand-over): ring row r of
                                       * the level-0 correlation planes lives in physical slot fmap1_slot[r] of `fmap1`.  A
                                       * dropped keyframe then rotates table entries instead of moving three 4.9 MB planes
                                       * (ramp/Ramp_vo.py:259-271 shifts them); every reader of `fmap1` rows (correlation, frame
                                       * commit, warm-up) goes through the table; the caller undoes the permutation when it takes
                                       * the buffers back.  NULL: rows are slots                                           */
  int32_t corr_f32_mfma;              /* feat_fp32 == 1: the correlation kernel -- 1 corr_mfma_kernel<float> (the fp32 matrix
                                       * cores), 0 corr_kernel<float> (the reference kernel's summation order, plain planes
                                       * only).  The caller sets it from the mode its features were packed in
                                       * (rampvo_amd: Patchifier.pack_f32, RAMP_CORR_F32_MFMA)                          */
} ramp_track;

/* cache warm-up for the next step's correlation kernel: reads the planes of the window's frames and the patch features
 * once (no effect on any value; `sink` [1] is never written in practice).  Meant for the front-end stream, in the slack
 * behind the front end.                                                                                            */
int ramp_track_warm(const ramp_track *t, int32_t *sink, void *stream);
/* holds `stream` back for about `microseconds` with one sleeping wave (frame pipelining: the next frame's encoder
 * should reach the chip a little behind the gru launch)                                         */
int ramp_stream_delay(int microseconds, void *stream);

/* Cross-stream "go" through a 32-bit word instead of an event: the producer is a KERNEL that stores a sequence number
 * (no packet between its stream's launches); the consumer stream waits with ONE sleeping wave that looks at the word
 * every ~3 us and ends when it is >= value, or after timeout_us (a producer that never comes must not hang the stream;
 * a time-out is an ERROR for whoever relied on the order: it is recorded in *status);
 * it then sleeps then_delay_us more.  (A hipStreamWaitValue32 in its place slows the other streams' launches down for
 * as long as it is pending, and so does a wave that polls without pauses: DESIGN.md section 8.0.)  The word lives in
 * signal memory (hipExtMallocWithFlags(hipMallocSignalMemory)), zero-initialised.                                    */
int ramp_signal_alloc(uint32_t **flag);
int ramp_signal_free(uint32_t *flag);
int ramp_stream_wait_flag(void *stream, const uint32_t *flag, uint32_t value, int timeout_us, int then_delay_us,
                          int32_t *status /* optional: bit 128 is ORed in when the wait times out */);
/* the producer side as a launch of its own (one thread storing `value`), for producers that are not this library's kernels */
int ramp_stream_signal(void *stream, uint32_t *flag, uint32_t value);
/* device address of a pinned (mapped) host allocation */
int ramp_host_device_pointer(void *host, void **dev);

size_t ramp_track_sizeof(void);      /* sizeof(ramp_track): lets a binding check its mirror of the struct */
size_t ramp_track_plan_workspace_bytes(int E_cap, int kkey_cap, int pkey_cap);
size_t ramp_track_ba_workspace_bytes(int E_cap, int n_rows, int M, int opt_window, int kk_cap, int ij_cap);

/* plan (groupings + temporal neighbours) of graph[cur] with the sizes in dyn: needed once, when the host hands a graph
 * over; afterwards every step builds the next one                                                                  */
int ramp_track_plan(const ramp_track *t, int cur, void *stream);

/* One tracked frame (flags = COMMIT | UPDATE | KEYFRAME), a bare update() (flags = UPDATE), ...; `cur` = which half of
 * graph[] holds the current graph (KEYFRAME writes the next one to 1 - cur).  k_new: optional device [4] intrinsics at
 * feature resolution when they differ from the previous frame's.  gate_event: optional hipEvent_t recorded before the
 * last kernel of the update operator (where the next frame's front end may start on another stream).  E_bound: the
 * caller's upper bound of the current factor count (from its lazy copy of dyn; 0 = E_cap) -- sizes the per-factor
 * launches; a bound below the live count raises status bit 32 instead of truncating silently.                      */
int ramp_track_step(const ramp_track *t, int cur, int64_t counter, int flags, int E_bound, const float *k_new,
                    void *gate_event, void *stream);

/* ramp_ba_covariance for a device-resident tracker BETWEEN two frames, as one call that never reads the device: the window
 * [max(n - opt_window, 1), n) with n = dyn[RAMP_DYN_NROW] keyframes, the factors the last graph edit kept (the first
 * dyn[RAMP_DYN_EKEPT] of graph[cur]; the next frame's factors behind them point at a frame that is not stored yet and take
 * no part), the last update's t->target / t->weight read through the kept factors' hidden-state rows (their index in the
 * graph that update ran on), at the poses and patches as they are now.  The kept factors are grouped for this call (the
 * tracker's plan covers the next frame's factors too) into `ws`, with t->plan_ws as scratch; the system is built in
 * t->ba_ws.  Nothing of the tracker's state is written: not dyn, not its status word, not the plan.
 *   cov [6 opt_window][6 opt_window] (the leading 6N x 6N block is the window's; a shorter window leaves identity blocks
 *   behind it), depth_var [n_rows * M] (entries without a kept factor untouched), stats [8] as ramp_ba_covariance: N and
 *   t0 are read from there.  cur: the half of graph[] that holds the current graph (as ramp_track_step's next call).     */
size_t ramp_track_uncertainty_workspace_bytes(const ramp_track *t);
int ramp_track_uncertainty(const ramp_track *t, int cur, float *cov, float *depth_var, float *stats, void *ws,
                           size_t ws_bytes, void *stream);

/* ramp_ba_map_covariance for a device-resident tracker between two frames: ramp_track_uncertainty (same window, same kept
 * factors, same cov / depth_var / stats bits) plus the map's four outputs, capacity sized: point [n_rows * M][3],
 * point_cov [n_rows * M][6], pose_depth_cov [n_rows * M][6], n_obs [n_rows * M] (entries without a kept factor untouched).
 * The sizes are read on the device; nothing of the tracker's state is written.                                         */
size_t ramp_track_map_workspace_bytes(const ramp_track *t);
int ramp_track_map(const ramp_track *t, int cur, float *cov, float *depth_var, float *stats, float *point, float *point_cov,
                   float *pose_depth_cov, int32_t *n_obs, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- live poses (csrc/publish.hip)
 *
 * ramp_track_publish: one wave that writes the pose record of frame `counter` (layout: RAMP_POSE_*) into slot
 * counter % ring_cap of `ring_dev`, the DEVICE address (ramp_host_device_pointer) of a ring of ring_cap records in pinned
 * host memory.  Enqueued on the frame's stream BEHIND the frame's ramp_track_step: the keyframe test's outcome is part of
 * the record, so the launch follows the graph edit and reads the newest pose from the row the edit left it in
 * (dyn[RAMP_DYN_NROW] - 1) -- the same seven floats bundle adjustment wrote, a row shift only moves them.
 *   t != NULL : a device-resident frame; n, the row, the factor count, the status word, the test's outcome and its delta
 *               entry are read from t->dyn / t->dlog, poses and time stamps from t->poses / t->tstamps; the _imm arguments
 *               are ignored.
 *   t == NULL : a host-driven frame; the caller passes the same values as immediates (row_imm: the row of `poses` that
 *               holds the newest frame's pose, 0 <= row_imm < n_rows; t1_imm / t0_imm: -1 without a delta entry).
 * tstamp: the caller's time stamp of the frame.                                                                        */
int ramp_track_publish(const ramp_track *t, int64_t counter, double tstamp, float *ring_dev, int ring_cap,
                       const float *poses, const int64_t *tstamps, int n_rows, int n_imm, int row_imm, int E_imm,
                       int status_imm, int dropped_imm, int t1_imm, int t0_imm, void *stream);

/* ramp_trajectory_resolve: what Ramp_vo.terminate() computes (ramp/Ramp_vo.py:113-133), as one launch of one workgroup.
 * out[t] for t in [0, T): inv(kf_poses[i]) where kf_tstamps[i] == t for a keyframe i < n; otherwise
 * inv(dP_t * (dP_t0 * ( ... * kf_pose))) along the delta chain (t -> t0 -> ...), entries taken from extra_log [n_extra]
 * and dlog [nlog], both in the RAMP_TRACK_LOG layout (a frame found in both: the dlog entry; a frame that is a keyframe
 * and has an entry: the keyframe).  Products are formed innermost first, in rounds of increasing chain depth, with the
 * device functions of ramp_se3_mul / ramp_se3_inv: the rows equal the host recursion's bit for bit.
 * dyn != NULL: n = dyn[RAMP_DYN_NROW] and nlog = dyn[RAMP_DYN_NLOG] (a device-resident tracker; the arguments n / nlog are
 * then the CAPACITIES of kf_poses and dlog, the device values are clamped to them).  ws: int32 [3 * T] scratch.
 * *status (device int32, written by the launch): 0, or RAMP_TRAJ_UNRESOLVED.                                          */
int ramp_trajectory_resolve(const float *kf_poses, const int64_t *kf_tstamps, int n, const int32_t *dyn, const float *dlog,
                            int nlog, const float *extra_log, int n_extra, int T, float *out, int32_t *ws, int32_t *status,
                            void *stream);

/* ---------------------------------------------------------------- poses at any time (csrc/interp.hip)
 *
 * ramp_se3_interp: the SE(3) geodesic through the knots of a trajectory, evaluated at Q time stamps, as two launches (one
 * lane per segment, then one lane per query).
 *   knots [T][7] (t, q) as ramp_se3_*; times [T] float64, non-decreasing; query [Q] float64.  Per query t:
 *     s     = the largest index with times[s] <= t, clamped to [0, T - 2]
 *     alpha = (t - times[s]) / (times[s + 1] - times[s]), formed in float64 and rounded to fp32 once; a clamped segment of
 *             zero length: alpha = 0 for t < times[s], else 1
 *     xi_s  = Log(knots[s + 1] * knots[s]^-1)   (the left increment, tangent order translation 3, rotation 3)
 *     out   = Exp(alpha * xi_s) * knots[s]      (the arithmetic of ramp_se3_log / _exp / _mul / _inv)
 *     twist = xi_s / (times[s + 1] - times[s]) [Q][6], optional (NULL): the segment's constant left twist; zero for a segment
 *             of zero length and for T == 1
 *   Outside [times[0], times[T - 1]]: alpha is clamped to [0, 1], or with RAMP_INTERP_EXTRAPOLATE the end segment's screw
 *   motion is continued.  T == 1: every query returns the knot.
 *   flags: RAMP_INTERP_EXTRAPOLATE; RAMP_INTERP_ROW_STORES (every lane stores its own 28- / 24-byte row instead of the tile
 *   leaving through LDS as contiguous full-width stores: the same bits, kept for tools/pose_query_cost.py).
 *   seg_ws: ramp_se3_interp_workspace_bytes(T) bytes, 16-byte aligned (the segments' increments, twists and lengths).
 *   status: device int32 [4], written by the call: [0] bits (RAMP_INTERP_BAD_TIMES: a time stamp of `times` decreases or is
 *   not finite), [1] queries below times[0], [2] queries above times[T - 1], [3] NaN queries.
 * Failures follow the convention of ramp_ba_covariance (NaN, never a plausible number; the return value stays RAMP_OK, it is
 * an outcome of the data): RAMP_INTERP_BAD_TIMES makes every row of out and twist NaN; a NaN query makes its own row NaN and
 * is counted.  T < 1 or Q < 0: RAMP_EINVAL.  Q == 0: RAMP_OK, nothing is launched and nothing written, status included.
 * A row is a function of its own query alone: its bits depend neither on Q, nor on its position, nor on the queries' order.
 * ramp_se3_interp_lds_knots(): the largest T whose knot times the query launch stages in LDS; above it the search reads
 * global memory.                                                                                                       */
#define RAMP_INTERP_EXTRAPOLATE 1
#define RAMP_INTERP_ROW_STORES 2
#define RAMP_INTERP_BAD_TIMES 1 /* status[0] bit 0 */
size_t ramp_se3_interp_workspace_bytes(int T);
int ramp_se3_interp_lds_knots(void);
int ramp_se3_interp(const float *knots, const double *times, int T, const double *query, int Q, int flags, float *out,
                    float *twist, void *seg_ws, size_t seg_ws_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------- motion-compensated events (csrc/warp.hip)
 *
 * ramp_event_warp: every event is warped from the camera pose at its own time stamp to the pose at t_ref, and the warped
 * events are splat bilinearly into an image of warped events and / or a bin stack.  One pass over the events: segment
 * search, interpolation, warp and scatter; the per-event pose is never written.
 *   events: x, y [N] fp32 pixel coordinates (fractions allowed), t [N] float64, p [N] int8 polarity (+-1; 0 is read as -1).
 *   knots [T][7], times [T] float64: a CAMERA-TO-WORLD trajectory, as ramp_trajectory_resolve writes it; C(t) is the geodesic
 *   of ramp_se3_interp through it (the same s, the same alpha formed in float64, the same segment table), held outside the
 *   knots' range or continued with RAMP_INTERP_EXTRAPOLATE.  t_ref: float64, finite.  intrinsics: device (fx, fy, cx, cy).
 *   invdepth: device pointer; RAMP_WARP_DEPTH_SCALAR: one float; RAMP_WARP_DEPTH_MAP: [H][W] floats, sampled at the event's
 *   rounded pixel (rint: halves to even), clamped to the image.  Inverse depth 0 compensates the rotation alone.
 *     G  = C(t_ref)^-1 * C(t)                 (C(t_ref)^-1 is formed once, in the segment launch)
 *     X' = R_G * ((x - cx) / fx, (y - cy) / fy, 1) + t_G * d
 *     x' = fx * (X' / Z') + cx,   y' = fy * (Y' / Z') + cy
 *   G is composed so that an event whose C(t) equals C(t_ref) in every bit (T == 1; t == t_ref) gets the exact identity.
 *   An event is INVALID when x, y or t is not finite, when Z' <= RAMP_WARP_MIN_Z (or Z' is NaN), or when x' or y' is not
 *   finite: it contributes nothing and its row of xy_out is NaN.  RAMP_WARP_MIN_Z = 0.2 takes the role of
 *   projective_ops.MIN_DEPTH, in the same units: Z' is the depth at t_ref relative to the depth at t (d scales the
 *   translation), so the test drops events whose point comes closer than a fifth of its depth or passes behind the camera.
 *   Scatter: the neighbours floor(x'), floor(x') + 1 with weights 1 - wx, wx (wx = x' - floor(x'), fp32), the same in y;
 *   neighbours outside the image are dropped.  A neighbour contributes c = llrint(ldexp(wx_i * wy_j, 24)) (one fp32 product,
 *   no FMA), added with 64-bit INTEGER atomics: the sums do not depend on the events' order and a call repeats its bits.
 *   |sum| < 2^63 holds up to 2^39 events on one pixel.
 *   Outputs, each optional (NULL), converted by a finishing launch (float(sum) * 2^-24 rounds once):
 *     xy_out [N][2] fp32      the warped coordinates
 *     iwe [2][H][W] fp32      plane 0 the polarity-signed sum, plane 1 the unsigned count
 *     stack_f32, stack_i8 [bins][H][W]   event i goes to bin int32(float32(bins) * float32(i) / float32(N)) as in
 *                             ramp_event_stack (capped at bins - 1); int8: the fixed-point sum divided by 2^24 toward zero,
 *                             then modulo 256.  (stack_f32 is the sum itself, not the value of the wrapped int8.)
 *   RAMP_WARP_IDENTITY: no trajectory -- x' = x, y' = y; t, knots, times, intrinsics and invdepth are not read (NULL).  This
 *   is the sub-pixel bilinear path of the event stack.
 *   status: device int32 [8], written by the call: [0] bits (RAMP_INTERP_BAD_TIMES), [1] / [2] events below / above the
 *   knots' range, [3] events with a coordinate or time stamp that is not finite ([1], [2] count the others only), [4] events
 *   rejected by the Z' test or whose projection is not finite, [5] valid events whose four neighbours all lie outside the
 *   image, [6] events with a neighbour inside it, [7] 0.  [3] + [4] + [5] + [6] = N.  RAMP_INTERP_BAD_TIMES makes every
 *   output NaN (0 for int8) and [4] - [6] zero; [1] - [3] are still counted.  These are outcomes of the data: RAMP_OK.
 *   ws: ramp_event_warp_workspace_bytes(T, bins, H, W) bytes, 16-byte aligned (segment table, C(t_ref)^-1, counters, int64
 *   accumulators); xy_out 8-byte aligned (else RAMP_EINVAL).  Launches: at most three kernels behind one
 *   hipMemsetAsync, all on `stream`, nothing synchronised.
 *   N == 0: RAMP_OK, nothing is launched and nothing written.  T < 1, H, W or bins < 1, no output requested, a t_ref that is
 *   not finite: RAMP_EINVAL (bins is 1 for a caller without a stack).
 * ramp_event_warp_grid_events(): the number of events one trip of the full event grid covers; above it the workgroups take
 * a second trip.                                                                                                       */
#define RAMP_WARP_DEPTH_SCALAR 0
#define RAMP_WARP_DEPTH_MAP 4
#define RAMP_WARP_IDENTITY 8
#define RAMP_WARP_MIN_Z 0.2f
size_t ramp_event_warp_workspace_bytes(int T, int bins, int H, int W);
long ramp_event_warp_grid_events(void);
int ramp_event_warp(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                    const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth, int flags,
                    int bins, int H, int W, float *xy_out, float *iwe, float *stack_f32, int8_t *stack_i8, void *ws,
                    size_t ws_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------- event multi-view stereo (csrc/emvs.hip)
 *
 * ramp_event_dsi: depth from a plane sweep of the events (the space-sweep "disparity space image" of EMVS, Rebecq et al., IJCV
 * 2018).  Every event is back-projected from the camera pose at its own time stamp and swept through D planes of constant
 * inverse depth of the camera at t_ref; each plane takes the bilinear splat of ramp_event_warp.  Votes pile up where the
 * scene's edges are: per pixel, the plane with the most votes, refined by a parabola, is a semi-dense inverse depth.
 *   events: x, y [N] fp32, t [N] float64 (the polarity takes no part); knots, times, t_ref, intrinsics and
 *   RAMP_INTERP_EXTRAPOLATE (the only flag) as ramp_event_warp.  range: device float [2] = (d_lo, d_hi), inverse depths in the
 *   unit of the knots' translations; the host never reads it.  The planes are uniform in inverse depth:
 *     step = (double(d_hi) - double(d_lo)) / (D - 1)   (0 for D == 1),     d_k = float32(double(d_lo) + k * step)
 * Vote.  The statements of ramp_event_warp up to R = R_G ((x - cx) / fx, (y - cy) / fy, 1) and t_G (the same segment table,
 *   alpha, C(t), G), once per event; then per plane X'_k = R + t_G * d_k and the projection of ramp_event_warp.  A plane whose
 *   Z' <= RAMP_WARP_MIN_Z (or NaN) or whose projection is not finite gets NO VOTE from this event; every other plane gets the
 *   splat of ramp_event_warp at (x'_k, y'_k): the neighbours floor and floor + 1, c = llrint(ldexp(wx_i * wy_j, 24)), neighbours
 *   outside the image dropped (a vote may so add nothing), added with 64-bit INTEGER atomics into
 *     dsi int64 [D][H][W]       caller-owned, 8-byte aligned, zeroed by the call
 *   The sums do not depend on the events' order and a call repeats its bits.
 *     coords fp32 [N][D][2]     optional (NULL), 8-byte aligned: (x'_k, y'_k), NaN where the plane got no vote.  For tests and
 *                               small calls: it is N * D * 8 bytes.
 * Detect, per pixel, in integers:  best = max_k dsi[k],  plane = the LOWEST k that attains it.  The pixel is detected when
 *     best >= min_fixed   and, with adaptive_radius r > 0,   best >= (box // n_in) + offset_fixed
 *   box: the int64 sum of `best` over the (2r + 1)^2 window clipped to the image, n_in: the pixels of that window inside the
 *   image, //: floor division; min_fixed = llrint(min_votes * 2^24), offset_fixed = llrint(adaptive_offset * 2^24) (it may be
 *   negative).  Refinement, in float64 without FMA: with (a, b, c) = dsi[plane - 1, plane, plane + 1],
 *     delta = (a - c) / (2 den)  for 0 < plane < D - 1 and den = a - 2 b + c != 0 (integers),  else 0
 *     invdepth = float32(double(d_lo) + (plane + delta) * step)
 * Outputs, each optional (NULL): invdepth [H][W] fp32; confidence [H][W] fp32 = float(best) * 2^-24, detected or not; plane
 *   [H][W] int32, -1 where not detected.  A pixel that is not detected gets *fill (a device float) in invdepth, NaN when fill is
 *   NULL.
 * status: device int32 [8], written by the call: [0] bits (bit 0 RAMP_INTERP_BAD_TIMES; RAMP_DSI_BAD_RANGE: a word of range is
 *   not finite, d_lo < 0, or d_hi <= d_lo with D > 1), [1] / [2] events below / above the knots' range ([3] not among them), [3]
 *   events with a coordinate or time stamp that is not finite, [4] finite events that voted in no plane, [5] events that voted in
 *   at least one plane, [6] detected pixels, [7] 0.  [3] + [4] + [5] = N.
 * Failures, never a plausible number: either bit makes invdepth, confidence and coords NaN, plane -1, dsi zero and [5], [6]
 *   zero (the finite events are then counted in [4]).  Outcomes of the data: RAMP_OK.
 * ws: ramp_event_dsi_ws_bytes(T, H, W) bytes, 16-byte aligned (segment table, C(t_ref)^-1, counters, per pixel the best
 *   votes, plane and refined inverse depth).  Launches: one hipMemsetAsync (the DSI) and four kernels (segment table and
 *   C(t_ref)^-1, vote, detect, threshold and status), all on `stream`, nothing read back, nothing synchronised, no
 *   floating-point atomics.  N == 0 runs them all: the DSI is zero, nothing is detected, invdepth is the fill everywhere.
 * RAMP_EINVAL: NULL events with N > 0, N < 0, T < 1, H, W or D < 1, adaptive_radius outside [0, 15], unknown flags, a t_ref,
 *   min_votes or adaptive_offset that is not finite, a NULL knots / times / intrinsics / range / dsi / ws / status, a dsi or
 *   coords that is not 8-byte aligned.  RAMP_EUNSUPPORTED: D * H * W >= 2^31, or N * D >= 2^38 (below it every box sum stays
 *   below 2^62).  RAMP_EWORKSPACE: a workspace too small.  A refused call touches nothing.
 * ramp_event_dsi_grid_events(): the number of events one trip of the full event grid covers.                            */
#define RAMP_DSI_BAD_RANGE 2 /* status[0] bit 1 */
size_t ramp_event_dsi_ws_bytes(int T, int H, int W);
long ramp_event_dsi_grid_events(void);
int ramp_event_dsi(const float *x, const float *y, const double *t, int N, const float *knots, const double *times, int T,
                   double t_ref, const float *intrinsics, const float *range, int flags, int D, int H, int W, double min_votes,
                   int adaptive_radius, double adaptive_offset, const float *fill, int64_t *dsi, float *coords,
                   float *invdepth, float *confidence, int32_t *plane, void *ws, size_t ws_bytes, int32_t *status,
                   void *stream);

/* ---------------------------------------------------------------- event map (csrc/evmap.hip)
 *
 * What EMVS does behind its detection: the semi-dense inverse depths of one reference view (ramp_event_dsi's invdepth / plane /
 * confidence, or any map) are median-filtered over the detected pixels, isolated detections are dropped, the rest is lifted to
 * world points (ramp_depth_points); the clouds of successive views are merged in a voxel hash table (ramp_point_map_*).
 *
 * ramp_depth_points.  invdepth [H][W] fp32; plane [H][W] int32, optional: a pixel is DETECTED when plane >= 0, with plane ==
 *   NULL when invdepth is finite and > 0; confidence [H][W] fp32, optional (NULL: 1); cam: device float [7], CAMERA-TO-WORLD
 *   (t, q as stored, not normalised: a row of the trajectory / of ramp_se3_interp); intrinsics: device (fx, fy, cx, cy) at the
 *   image's resolution; median_radius r in 0 .. 3; min_support s >= 1; min_invdepth >= 0, finite.
 * Filter, per detected pixel: the inverse depths of the detected pixels of the (2r + 1)^2 window clipped to the image, the
 *   pixel itself among them, n in number.  n < s: the pixel is ISOLATED.  Else the filtered value is the LOWER median, the
 *   element of index (n - 1) / 2 in ascending order -- the order of the project's median (csrc/median.h): that of the floats'
 *   bits mapped to unsigned words, -0 below +0, a NaN with a clear sign bit above +inf.  r = 0: the pixel's own value.
 * Lift, fp32 without FMA, (u, v) the integer pixel coordinates:   z = 1.0f / d,
 *     Xc = (((u - cx) / fx) * z, ((v - cy) / fy) * z, z),    Xw = q Xc q^-1 + t   (lt_qrot of csrc/ramp_device.h)
 *   DEPTH REJECTED: d not finite, d <= 0, d < min_invdepth, or a world point that is not finite.
 * Outputs, compacted in ascending pixel index (a scan gives the positions: no atomics): points [K][3] fp32, conf [K] fp32,
 *   pixel [K] int32 (v * W + u), each with room for H * W rows; count: device int32 = K; invdepth_filtered [H][W] fp32,
 *   optional (NULL): the filtered value of a lifted pixel, NaN elsewhere.
 * status: device int32 [8], written by the call: [0] bits (bit 0 RAMP_DEPTH_POINTS_BAD_CAMERA: a word of cam or intrinsics is
 *   not finite, or fx / fy is 0: nothing is detected, count = 0, invdepth_filtered NaN everywhere, [1] .. [4] zero), [1]
 *   detected, [2] isolated, [3] depth rejected, [4] lifted = count, [5] .. [7] 0.  [2] + [3] + [4] = [1].
 * ws: ramp_depth_points_ws_bytes(H, W) bytes, 256-byte aligned.  One hipMemsetAsync (status), two kernels and one hipcub
 *   scan, all on `stream`, nothing read back, nothing synchronised, no floating-point atomics; a call repeats its bits.
 * RAMP_EINVAL: H or W < 1, r outside [0, 3], s < 1, a min_invdepth that is negative or not finite, a NULL invdepth / cam /
 *   intrinsics / points / conf / pixel / count / ws / status, a ws that is not 256-byte aligned.  RAMP_EUNSUPPORTED: H * W >=
 *   2^31.  RAMP_EWORKSPACE: a workspace too small.  A refused call touches nothing.
 *
 * The voxel hash.  map: a caller-owned device buffer of ramp_point_map_bytes(capacity) bytes, 64-byte aligned; capacity: a
 *   power of two, 2^3 .. 2^30 (else the size is 0 and every call RAMP_EINVAL).  A 64-byte header (word 0: the occupied slots,
 *   int64) and one 64-byte slot per voxel: key int64 (-1: empty; no voxel's key has bit 63 set), n int64, sq[3] int64, sc int64,
 *   views uint64, one spare word.  ramp_point_map_clear: one launch; a buffer has to be cleared before its first insert.
 * ramp_point_map_insert.  points [n_points][3] fp32, conf [n_points] fp32 (NULL: 1); count: optional device int32, the live
 *   rows are then min(max(*count, 0), n_points), and n_points is the launch bound; voxel: the edge, a double, finite, > 0;
 *   view >= 0: the id of the reference view.  One lane per point, float64 without FMA, per axis a:
 *     g = double(p[a]) / voxel,  i = floor(g),  q = llrint((g - i) * 2^20) in 0 .. 2^20;   |i| >= 2^20: OUT OF RANGE
 *     key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20),      c = llrint(min(double(conf), 2^20) * 2^16)
 *   A coordinate or confidence that is not finite, or a confidence below 0: NOT FINITE.  Both kinds are counted and dropped.
 *   Slot: the finaliser of splitmix64 on the key (z ^= z >> 30, z *= 0xbf58476d1ce4e5b9, z ^= z >> 27, z *= 0x94d049bb133111eb,
 *   z ^= z >> 31) masked to the capacity, then linear probing with a 64-bit atomicCAS on the key word.  On a claim or a match:
 *   n += 1, sq[a] += q[a], sc += c (atomicAdd), views |= 1 << (view & 63) (atomicOr): VIEW IDS WRAP AT 64.  The probe loop is
 *   bounded by `capacity` iterations; a point that ends it without a slot is DROPPED-FULL.  No lane waits for another lane.
 *   status: device int32 [8], written by the call: [0] 0, [1] seen (the live rows), [2] not finite, [3] out of range, [4]
 *   dropped-full, [5] accumulated, [6] occupied slots after the call, [7] 0.  [2] + [3] + [4] + [5] = [1].  All sums are
 *   integers: while nothing is dropped-full the table does not depend on the points' order or on how they are split over calls.
 *   One hipMemsetAsync (status) and two kernels (one with n_points == 0).
 * ramp_point_map_export.  The occupied slots with n >= min_points and popcount(views) >= min_views, sorted by key ascending
 *   (hipcub radix sort over the whole table), the first max_out of them, K in number:
 *     points [K][3] fp32: float32((double(i_a) + (double(sq_a) / double(n)) * 2^-20) * voxel)     (voxel: as at the inserts)
 *     n [K] int32 (saturating), conf [K] fp32 = float32(double(sc) * 2^-16), n_views [K] int32, key [K] int64, count: device
 *     int32 = K.  Each array has room for min(max_out, capacity) rows.
 *   status: device int32 [8]: [0] 0, [1] slots that pass, [2] of those, cut off by max_out (the highest keys), [3] occupied
 *   slots, [4] .. [7] 0.  ws: ramp_point_map_export_ws_bytes(capacity) bytes (24 bytes per slot and hipcub's own),
 *   256-byte aligned.  One hipMemsetAsync (status), two kernels around the sort.  The map is not written.
 * All on `stream`, nothing read back, nothing synchronised, no floating-point atomics.  RAMP_EINVAL: a NULL or misaligned map,
 *   a capacity that is not a power of two in 2^3 .. 2^30, a voxel that is not finite or not > 0, n_points < 0, NULL points with
 *   n_points > 0, view < 0, min_points / min_views / max_out < 0, a NULL output with max_out > 0, a NULL count / ws / status, a
 *   misaligned ws or key.  RAMP_EWORKSPACE: a workspace too small.  A refused call touches nothing.                        */
#define RAMP_DEPTH_POINTS_BAD_CAMERA 1 /* status[0] bit 0 */
size_t ramp_depth_points_ws_bytes(int H, int W);
int ramp_depth_points(const float *invdepth, const int32_t *plane, const float *confidence, const float *cam,
                      const float *intrinsics, int H, int W, int median_radius, int min_support, float min_invdepth,
                      float *points, float *conf, int32_t *pixel, float *invdepth_filtered, int32_t *count, void *ws,
                      size_t ws_bytes, int32_t *status, void *stream);
size_t ramp_point_map_bytes(long capacity);
int ramp_point_map_clear(void *map, long capacity, void *stream);
int ramp_point_map_insert(void *map, long capacity, const float *points, const float *conf, int n_points, const int32_t *count,
                          double voxel, int view, int32_t *status, void *stream);
size_t ramp_point_map_export_ws_bytes(long capacity);
int ramp_point_map_export(const void *map, long capacity, double voxel, long min_points, int min_views, int max_out,
                          float *points, int32_t *n, float *conf, int32_t *n_views, int64_t *key, int32_t *count, void *ws,
                          size_t ws_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------- event map rendering (csrc/maprender.hip)
 *
 * ramp_point_map_render: the voxel hash seen from any camera -- a z-buffered [H][W] map of inverse depth, the map
 * ramp_event_warp samples with RAMP_WARP_DEPTH_MAP.  map, capacity, voxel: as at the inserts; the map is not written.
 * Which slots take part.  One lane per slot reads the table where it is (no sort, no export).  A slot takes part when key !=
 *   -1, n >= min_points and popcount(views) >= min_views: the export's conditions.  Every other occupied slot is FILTERED.
 * World point.  The export's mean point, fp32: float32((double(i_a) + (double(sq_a) / double(n)) * 2^-20) * voxel) (one device
 *   function, csrc/evmap_device.h, which the export calls as well).
 * Camera.  cam: device float [7], CAMERA-TO-WORLD (t, q as stored, not normalised: a row of the trajectory / of
 *   ramp_se3_interp, as in ramp_depth_points); intrinsics: device (fx, fy, cx, cy) at the image's resolution.
 * Projection, fp32 without FMA:   Xc = q^-1 (Xw - t) q   (lt_qrot of csrc/ramp_device.h with (-qx, -qy, -qz, qw)),
 *     z = Xc.z,   d' = 1.0f / z,   u = fx * (Xc.x * d') + cx,   v = fy * (Xc.y * d') + cy
 *   REJECTED: z <= RAMP_WARP_MIN_Z (or NaN), a word of Xc that is not finite, or u or v not finite.
 * Footprint.  The centre pixel is (rintf(u), rintf(v)) -- half to even, the rounding with which ramp_event_warp samples an
 *   [H][W] map, so a rendered map and its consumer agree on what a pixel is.  footprint == 0: r_p = radius.  Else r_p is half
 *   the voxel's projected edge, float64 without FMA:
 *     rho = ((0.5 * voxel) * double(max(|fx|, |fy|))) * double(d'),    r_p = min(radius, max(0, (int)ceil(rho - 0.5)))
 *   (the comparison with radius is made on the double: a huge rho never reaches an integer).  The slot covers the square
 *   [px - r_p, px + r_p] x [py - r_p, py + r_p] clipped to the image.  A square without a pixel inside the image: the slot is
 *   OUTSIDE (tested in floating point before any conversion to an integer: a huge u does not overflow).  Else it is RENDERED.
 * Visibility.  Per pixel the winner is the covering slot with the largest d' -- the floats' bits compared as unsigned words,
 *   d' > 0 -- and among equal bits the one with the LOWEST key (keys are unique): the image depends neither on the order of
 *   the slots nor on the order of the inserts that built the table.
 * Outputs.  invdepth [H][W] fp32: the winner's d'; a pixel no slot covers gets *fill (fill: optional device float word, as in
 *   ramp_event_dsi) or NaN with fill == NULL.  key [H][W] int64, optional: the winner's key, -1 where nothing rendered.  n [H][W]
 *   int32, optional: the winner's n, saturating as the export's, 0 where nothing rendered.  conf [H][W] fp32, optional: the
 *   winner's float32(double(sc) * 2^-16), 0 where nothing rendered.  records [capacity][4] fp32, optional: (u, v, d',
 *   float(r_p)) of every slot that is rendered or outside, a NaN row for every other slot.
 * status: device int32 [8], written by the call: [0] bits (bit 0 RAMP_MAP_RENDER_BAD_CAMERA, raised exactly as
 *   RAMP_DEPTH_POINTS_BAD_CAMERA: a word of cam or intrinsics is not finite, or fx / fy is 0: invdepth and conf are NaN
 *   everywhere, fill or not, key -1, n 0, records NaN, [1] .. [6] zero -- never a plausible number), [1] occupied slots, [2]
 *   filtered, [3] rejected, [4] outside, [5] rendered (covers at least one pixel, whether or not it wins one), [6] pixels with
 *   a winner, [7] 0.  [2] + [3] + [4] + [5] = [1].
 * ws: ramp_point_map_render_ws_bytes(H, W) bytes (12 bytes per pixel), 256-byte aligned.  One hipMemsetAsync (status) and FOUR
 *   launches on `stream`: the clear of the workspace; per slot a return-less 32-bit atomicMax of the bits of d'; per slot a
 *   return-less 64-bit atomicMin of the key where the slot's bits are the pixel's; per pixel, one writer, the outputs, the
 *   winner's slot found by a read-only probe of the hash bounded by `capacity`.  The table is read twice.  Nothing is read
 *   back, nothing synchronised, no floating-point atomics, no lane waits for another one; a call repeats its bits.
 * RAMP_EINVAL: H or W < 1, radius outside 0 .. 7, a capacity that is not a power of two in 2^3 .. 2^30, a voxel that is not
 *   finite or not > 0, min_points or min_views < 0, a NULL map / cam / intrinsics / invdepth / ws / status, a map that is not
 *   64-byte, a ws that is not 256-byte or a key that is not 8-byte aligned.  RAMP_EUNSUPPORTED: H * W >= 2^31.
 *   RAMP_EWORKSPACE: a workspace too small.  A refused call touches nothing.                                            */
#define RAMP_MAP_RENDER_BAD_CAMERA 1 /* status[0] bit 0 */
size_t ramp_point_map_render_ws_bytes(int H, int W);
int ramp_point_map_render(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam,
                          const float *intrinsics, int H, int W, int radius, int footprint, const float *fill, float *invdepth,
                          int64_t *key, int32_t *n, float *conf, float *records, void *ws, size_t ws_bytes, int32_t *status,
                          void *stream);

/* ---------------------------------------------------------------- time surface (csrc/timesurface.hip)
 *
 * ramp_time_surface: per pixel the newest time stamp at or before t_ref, decayed and smoothed -- negated, the distance-like
 * field ramp_point_map_localize samples: near 0 where events fired just before t_ref, 1 where none did.
 * Last time stamps.  x, y: device fp32 [N]; t: device float64 [N], in any order.  The pixel of an event is (rintf(x),
 *   rintf(y)) -- half to even, the rounding with which ramp_event_warp samples a map.  Per pixel the largest finite t <= t_ref
 *   over the events and, if given, last_t_in (device float64 [H][W], ramp_event_filter's convention: NaN means no event yet; a
 *   word that is not finite or lies behind t_ref counts as none).  One return-less 64-bit atomicMax per used event on the
 *   double's bits mapped to an unsigned word of the same order (the word 0: no event), behind a relaxed load that skips an
 *   atomic which cannot change the word.  The integer max does not depend on the events' order: a call repeats its bits.
 * Surface, fp32.  raw(u) = expf(float32((last(u) - t_ref) / tau)), the quotient formed in float64; raw(u) = 0 where there is no
 *   time stamp.  With RAMP_TIME_SURFACE_NEGATE raw becomes 1.0f - raw.
 * Smoothing.  `smooth` passes (0 .. 8) of the separable 5-tap binomial (1, 4, 6, 4, 1) / 16, rows then columns, edges
 *   replicated, fp32 without FMA: ((((1 a + 4 b) + 6 c) + 4 d) + 1 e) * 0.0625f.  Tiles go through LDS; the passes ping-pong
 *   between `surface` and the workspace.  An fp32 emulator reproduces `surface` bit for bit from `raw`.
 * Outputs.  surface [H][W] fp32.  raw [H][W] fp32, optional: the surface in front of the smoothing.  last_t_out [H][W] float64,
 *   optional: the time stamps, NaN where there is none -- last_t_in of a later call.
 * status: device int32 [8], written by the call: [0] bits (bit 0 RAMP_TIME_SURFACE_BAD_ARGS: t_ref or tau is not finite or tau
 *   <= 0: surface and raw are NaN everywhere, last_t_out is still written), [1] events seen, [2] not finite (x, y or t), [3]
 *   outside the image, [4] later than t_ref, [5] used, [6] pixels with a time stamp, [7] 0.  [2] + [3] + [4] + [5] = [1] = N.
 * ws: ramp_time_surface_ws_bytes(H, W) bytes (12 bytes per pixel), 256-byte aligned.  One hipMemsetAsync (status) and 3 + 2 *
 *   smooth launches on `stream` (2 + 2 * smooth with N == 0, which is valid: the surface of last_t_in, or all "no event").
 *   Nothing is read back, nothing synchronised, no floating-point atomics, no lane waits for another one.
 * RAMP_EINVAL: N < 0, H or W < 1, smooth outside 0 .. 8, an unknown flag, a NULL surface / status / ws, NULL events with N > 0,
 *   a ws that is not 256-byte, a float64 buffer that is not 8-byte or another one that is not 4-byte aligned.
 *   RAMP_EUNSUPPORTED: H * W >= 2^31.  RAMP_EWORKSPACE: a workspace too small.  A refused call touches nothing.        */
#define RAMP_TIME_SURFACE_BAD_ARGS 1 /* status[0] bit 0 */
#define RAMP_TIME_SURFACE_NEGATE 1   /* flags */
size_t ramp_time_surface_ws_bytes(int H, int W);
int ramp_time_surface(const float *x, const float *y, const double *t, long N, const double *last_t_in, double t_ref, double tau,
                      int H, int W, int smooth, int flags, float *surface, float *raw, double *last_t_out, void *ws,
                      size_t ws_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------- event map localisation (csrc/maplocalize.hip)
 *
 * ramp_point_map_localize_eval: one evaluation of the alignment of the voxel hash with a time surface at a camera pose.
 * map, capacity, voxel, min_points, min_views, cam (CAMERA-TO-WORLD), intrinsics: as in ramp_point_map_render; which slots take
 * part (the export's conditions), their mean point and their projection (Xc, u, v, REJECTED) are the renderer's, one device
 * function (csrc/evmap_device.h): both entries give a voxel the same u, v in every bit.  The map is not written.
 * surface: device fp32 [H][W] (ramp_time_surface with RAMP_TIME_SURFACE_NEGATE).
 * Reach.  (u, v) is IN REACH when its four bilinear neighbours lie inside the image: 0 <= floorf(u) < W - 1 and 0 <= floorf(v) <
 *   H - 1, tested in floating point before any conversion.
 * Residual, fp32 without FMA, x0 = floorf(u), y0 = floorf(v), ax = u - x0, ay = v - y0, bx = 1.0f - ax, by = 1.0f - ay, s00 =
 *   surface[y0][x0], s10 = surface[y0][x0 + 1], s01 = surface[y0 + 1][x0], s11 = surface[y0 + 1][x0 + 1]:
 *     r  = by * (bx * s00 + ax * s10) + ay * (bx * s01 + ax * s11)
 *     gu = by * (s10 - s00) + ay * (s11 - s01),    gv = bx * (s01 - s00) + ax * (s11 - s10)     (the interpolant's own derivative)
 * Row, float64 without FMA from those fp32 words, (X, Y, z) = Xc, gx = double(gu) * double(fx), gy = double(gv) * double(fy):
 *     J0 = gx / z,  J1 = gy / z,  J2 = -(gx * X + gy * Y) / (z * z),  J3 = Y * J2 - z * J1,  J4 = z * J0 - X * J2,  J5 = X * J1 - Y * J0
 *   the derivative of r for the LEFT perturbation T <- Exp(xi) T of the world-to-camera pose T = cam^-1, xi = (translation 3,
 *   rotation 3).  Huber threshold k = huber (<= 0: off): |r| <= k: w = 1, rho = r * r; else w = k / |r|, rho = (2 k) |r| - k k.
 *   A slot that takes part but is REJECTED or out of reach contributes rho of r = 1, the surface's "no event" value, and no J:
 *   the cost is a sum over the same slots at every pose, and a step cannot lower it by pushing points out of the image.
 * sums: device float64 [32]: [0..20] sum (w J_p) J_q over p <= q, row-major; [21..26] sum (w J_p) r; [27] sum rho, the cost;
 *   [28] the slots in reach; [29] the slots that take part; [30], [31] 0.  Per lane over its slots in ascending order (a
 *   grid-stride loop, the grid capped: ramp_point_map_localize_grid_slots() slots per trip), then a fixed butterfly per wave,
 *   the waves in wave order, the workgroups' rows in index order by one workgroup: no floating-point atomics, and for a given
 *   table and arguments a call repeats its bits.  (Another insert order can move a slot, and with it the sums' rounding.)
 * records [capacity][8] fp32, optional: (u, v, r, gu, gv, Xc.x, Xc.y, Xc.z); a slot that does not take part gets a NaN row, a
 *   rejected one NaN in u .. gv, one out of reach NaN in r .. gv.
 * status: device int32 [8], written by the call: [0] bits (bit 0 RAMP_MAP_LOCALIZE_BAD_CAMERA, raised exactly as
 *   RAMP_MAP_RENDER_BAD_CAMERA: sums and records are then NaN, [1] .. [5] zero), [1] occupied slots, [2] filtered, [3] rejected,
 *   [4] out of reach, [5] in reach, [6], [7] 0.  [2] + [3] + [4] + [5] = [1].  A surface pixel that is NaN makes r and the cost NaN.
 * ws: ramp_point_map_localize_ws_bytes(capacity, iters) bytes, 256-byte aligned: ONE size for every valid capacity and iters
 *   (the workgroups' rows under the grid's cap and the loop's state; the arguments are only checked, 0 for an invalid one), so
 *   a caller queries it once.  One hipMemsetAsync (status), two launches.
 * RAMP_EINVAL: the renderer's list with H or W < 2, a NULL surface or sums, a NaN huber, sums not 8-byte aligned.
 *   RAMP_EUNSUPPORTED: H * W >= 2^31.  RAMP_EWORKSPACE.  A refused call touches nothing.
 *
 * ramp_point_map_localize: Levenberg-Marquardt over those evaluations, on the device: one call enqueues the whole solve, nothing
 * is read back.  A state machine, one step (a one-wave launch) behind every evaluation; all state float64, only + - * / and
 * sqrt in the order written, no FMA: a float64 restatement gives the same bits.
 *   state: C = (c[3], q[4]) camera-to-world (cam0 widened), lambda = lambda0, f, (H, b) = (sums[0..20], sums[21..26]) kept
 *   e == 0:     f = f0 = cost, keep (H, b);  in reach < 6 ? FEW : iters == 0 ? ITERS : propose
 *   cost < f:   C = trial, f = cost, keep (H, b), history[n_accepted++] = f, lambda = max(lambda / 10, 1e-12), rejects = 0;
 *               n_accepted == iters ? ITERS : in reach < 6 ? FEW : propose
 *   otherwise:  lambda = lambda * 10, rejects += 1;  rejects == RAMP_LOCALIZE_REJECTS ? STALLED : propose      (a NaN cost lands here)
 *   propose:    A = H, A_jj = H_jj + lambda * H_jj;  A = L L' by columns j = 0 .. 5, every sum started from A's word and reduced
 *               term by term in ascending k; a pivot that is not > 0 and finite: SINGULAR.  L y = -b forward, L' delta = y
 *               backward (terms in ascending k).  sqrt(sum delta_i^2) < min_step ? CONVERGED : trial = retract(C, delta); the
 *               next evaluation reads float32(trial).  The last evaluation enqueued ends a machine still running: BUDGET.
 *   retract:    delta = (v, w);  s = sqrt(1 + (w.w) / 4);  conj(dq) = (-(w / 2) / s, 1 / s)      (the Cayley map: Exp to first
 *               order, rational);  q' = q * conj(dq) (Hamilton, xyzw), divided by its norm;  c' = c - rot(q', v)    (lt_qrot's
 *               statements in float64): C' = C D^-1 for T' = D T, D = (R(dq), v).
 *   iters accepted steps at most (0 .. RAMP_LOCALIZE_MAX_ITERS); max_evals <= 0: 1 + 9 * iters evaluations, else the smaller of
 *   the two.  lambda0, the factors 10, the 8 rejections and min_step are values nobody has tuned.
 * Outputs (device).  pose_out float64 [7]: C; pose_f32 fp32 [7]: the bits the evaluation at C read; result float64 [4]: cost,
 *   cost0, lambda, the slots in reach at C; hessian float64 [36], gradient float64 [6]: the kept H (full, symmetric) and b;
 *   history float64 [iters]: the accepted costs, NaN behind them; status int32 [8]: the words of the evaluation at C; info int32
 *   [8]: reason (RAMP_LOCALIZE_*), n_accepted, n_evals, rejects, the OR of every evaluation's status[0], 0, 0, 0.  After FEW or
 *   SINGULAR with nothing accepted, or with the bad-camera bit in info[4], pose_out and pose_f32 are NaN in every word: never a
 *   plausible number.
 * RAMP_EINVAL as the evaluation, and: iters outside its range, lambda0 or min_step negative or not finite, a NULL output (history
 *   with iters > 0), a float64 output that is not 8-byte aligned.  3 launches per evaluation enqueued, behind one hipMemsetAsync
 *   and one copy of cam0; the launches behind a stop return at their first statement.                                    */
#define RAMP_MAP_LOCALIZE_BAD_CAMERA 1 /* status[0] bit 0 */
#define RAMP_LOCALIZE_ITERS 1
#define RAMP_LOCALIZE_CONVERGED 2
#define RAMP_LOCALIZE_STALLED 3
#define RAMP_LOCALIZE_SINGULAR 4
#define RAMP_LOCALIZE_FEW 5
#define RAMP_LOCALIZE_BUDGET 6
#define RAMP_LOCALIZE_MAX_ITERS 4096
#define RAMP_LOCALIZE_REJECTS 8 /* a step is given up after this many rejections in a row */
size_t ramp_point_map_localize_ws_bytes(long capacity, int iters);
long ramp_point_map_localize_grid_slots(void);
int ramp_point_map_localize_eval(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam,
                                 const float *intrinsics, const float *surface, int H, int W, double huber, double *sums,
                                 float *records, void *ws, size_t ws_bytes, int32_t *status, void *stream);
int ramp_point_map_localize(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam0,
                            const float *intrinsics, const float *surface, int H, int W, double huber, double lambda0,
                            double min_step, int iters, int max_evals, double *pose_out, float *pose_f32, double *result,
                            double *hessian, double *gradient, double *history, int32_t *status, int32_t *info, void *ws,
                            size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- inverse-depth map (csrc/depthmap.hip)
 *
 * ramp_invdepth_map: the selected patches of the window are projected into one camera pose and regressed to a dense map of
 * inverse depth -- the [H][W] map ramp_event_warp samples with RAMP_WARP_DEPTH_MAP.
 *   poses [ceil(n / M)][7] world-to-camera (the tracker's poses); patches [n][3][P][P] (x, y, inverse depth; the centre
 *   pixel (P / 2, P / 2) is read), patch k belongs to frame k / M; intrinsics: device (fx, fy, cx, cy) at patch resolution;
 *   scale > 0: image pixel = scale * patch coordinate (the image intrinsics are scale * intrinsics); cam: device float [7], a
 *   CAMERA-TO-WORLD pose, a row of ramp_trajectory_resolve / ramp_se3_interp.
 *   Selection: index != NULL: the patch ids index[0 .. *count) as ramp_map_select writes them (K: the capacity of index;
 *   count == NULL: all K; *count is clamped to [0, K]); index == NULL: all patches below the clipped n, or with
 *   last_rows > 0 the newest last_rows * per_row of them.  dyn_rows != NULL: n is clipped to *dyn_rows * per_row on the
 *   device, exactly as ramp_map_select does (n is then the capacity).  An id outside [0, clipped n) is rejected as a patch
 *   without a depth.  The record capacity Kc is K with an index, else n, or min(n, last_rows * per_row).
 *   conf [n] (NULL: c = 1): the confidence of patch k, or with RAMP_DEPTHMAP_CONF_IS_VARIANCE its variance, c = 1 / conf[k].
 *   prior: device float (NULL allowed when prior_weight == 0), pw = prior_weight, or with RAMP_DEPTHMAP_PRIOR_RELATIVE
 *   pw = prior_weight / prior^2 formed on the device (a prior of relative sigma prior_weight^-1/2, to be weighed against
 *   1 / variance confidences).  prior_weight == 0: pw = 0 and the prior is not read.  radius R > 0: the support, image pixels.
 * Stage 1, per selected patch with r = ((x - cx) / fx, (y - cy) / fy, 1) and inverse depth d (fp32, the arithmetic of
 * ramp_se3_inv / ramp_se3_mul):
 *     G = cam^-1 * T_i^-1,   X' = R_G r + t_G d,   u = scale * (fx X'/Z' + cx),  v likewise,   d' = d / Z'
 *   gives the record (u, v, d', c).  A rejected patch is counted in exactly one status word, tested in this order:
 *     [2] d or c is not finite or <= 0 (an infinite variance included; an id outside the patches)
 *     [3] Z' <= RAMP_WARP_MIN_Z or NaN, or u, v or d' not finite
 *     [4] out of reach: u < -R, u > W - 1 + R, or the same in v
 *   and its record carries weight exactly 0: (NaN, NaN, NaN, 0) for [2] and [3], (u, v, d', 0) for [4].
 * Stage 2, per integer pixel (x, y), in fp32 without FMA, the sums running over the records in selection order:
 *     s_k = 1 - ((x - u_k)^2 + (y - v_k)^2) * (1 / R^2),   w_k = c_k * max(s_k, 0)^2        (biweight: compact support)
 *     S0 = sum w_k,  S1 = sum w_k d'_k,   invdepth = (pw * prior + S1) / (pw + S0),   weight = S0
 *   A pixel with S0 == 0 gets the prior's own bits when pw > 0 and NaN when pw == 0 -- never a plausible number;
 *   ramp_event_warp rejects and counts an event that samples NaN.  A pw that is not finite (a relative prior of 0) makes
 *   every pixel NaN.  A record that is culled for a tile would have contributed w = 0 exactly and all terms are >= 0: a pixel's
 *   bits do not depend on tiling or culling, and a call repeats its bits (no atomics in the sums).
 * Outputs, each optional (NULL): invdepth [H][W], weight [H][W], records [Kc][4] (rows behind the live count are zero).
 * status: device int32 [8], written by the call: [0] bits (RAMP_DEPTHMAP_BAD_CAM: an entry of cam is not finite), [1] patches
 *   considered, [2] / [3] / [4] rejected as above, [5] contributing, [6] pixels with S0 == 0 (0 when neither map is
 *   requested), [7] 0.  [2] + [3] + [4] + [5] = [1].  RAMP_DEPTHMAP_BAD_CAM makes every output NaN (the live records
 *   included); the patches that pass the test of [2] are then counted in [3].  Outcomes of the data: RAMP_OK.
 * ws: ramp_invdepth_map_workspace_bytes(Kc) bytes, 16-byte aligned (the live count and the records).  Launches: one 32-byte
 *   hipMemsetAsync (the status words are the counters) and two kernels -- one when only records are requested -- all on
 *   `stream`, nothing synchronised.  n == 0, an empty selection and a NULL selection on zero capacity are legal and run the
 *   launches (the sizes live on the device): the prior everywhere, or NaN and weight 0 with pw == 0.
 * RAMP_EINVAL: H, W < 1; R or scale not finite or <= 0; prior_weight negative or not finite; no output requested; M, P < 1;
 *   unknown flags; count without index; last_rows > 0 with per_row < 1; a NULL prior with prior_weight > 0.
 * ramp_invdepth_map_stage_records(): the number of records one LDS chunk of the regression holds.                       */
#define RAMP_DEPTHMAP_CONF_IS_VARIANCE 1
#define RAMP_DEPTHMAP_PRIOR_RELATIVE 2
#define RAMP_DEPTHMAP_BAD_CAM 1 /* status[0] bit 0 */
size_t ramp_invdepth_map_workspace_bytes(int K);
int ramp_invdepth_map_stage_records(void);
int ramp_invdepth_map(const float *poses, const float *patches, const float *intrinsics, const float *cam, int n, int M, int P,
                      float scale, const int32_t *index, const int32_t *count, int K, const int32_t *dyn_rows, int per_row,
                      int last_rows, const float *conf, const float *prior, float prior_weight, float radius, int flags, int H,
                      int W, float *invdepth, float *weight, float *records, void *ws, size_t ws_bytes, int32_t *status,
                      void *stream);

/* ---------------------------------------------------------------- event contrast and its gradient (csrc/contrast.hip)
 *
 * ramp_event_contrast: the variance of the image of warped events (contrast maximisation's objective) and its gradient with
 * respect to a small correction theta = (v[3], w[3], lam) of the warp: translation 3, rotation 3, a log depth scale.
 * Everything up to X' is ramp_event_warp's, statement for statement: segment search, alpha in float64, C(t),
 * G = C(t_ref)^-1 C(t), the depth sampled at the event's own rounded pixel, P = ((x - cx) / fx, (y - cy) / fy, 1).  The
 * arguments are ramp_event_warp's without the stack; RAMP_WARP_IDENTITY is not accepted.  The correction acts in the reference
 * camera frame, to first order, by definition:
 *     tau = float32(t - t_ref)            (the difference formed in float64; the unit of the time stamps)
 *     ds  = d * expf(lam)
 *     X1  = R_G P + t_G ds
 *     X2  = X1 + tau * (v * ds + w x X1)
 *     x'  = fx X2.x / X2.z + cx ,  y' = fy X2.y / X2.z + cy
 *           invalid exactly as ramp_event_warp, with X2.z in the place of Z'
 *   correction: device float [7], or NULL for zero (the correction is then not evaluated at all).  A correction of zeros and
 *   NULL give the accumulators, the image and the status words of ramp_event_warp bit for bit.
 *   I(u) = sum_k s_k b(u - x'_k) is the bilinear splat of ramp_event_warp (the same fixed point, neighbours outside the image
 *   dropped); s_k = p_k, or 1 with RAMP_CONTRAST_UNSIGNED (the count plane).  With P_n = H W, mu = mean(I) and
 *   f = (1 / P_n) sum_u (I(u) - mu)^2 (the population variance), per event over the in-image neighbours (jx, jy) in {0,1}^2:
 *     df/dx'_k = (2 / P_n) s_k sum (I(ix + jx, iy + jy) - mu) * (jx ? +1 : -1) * wy[jy]
 *     df/dy'_k = (2 / P_n) s_k sum (I(ix + jx, iy + jy) - mu) * (jy ? +1 : -1) * wx[jx]
 *   (the mu term cancels only for events with all four neighbours inside, so it stays) and, for r any 3-vector:
 *     dx'/dX2 = (fx / Z, 0, -fx X / Z^2)         dy'/dX2 = (0, fy / Z, -fy Y / Z^2)
 *     dX2/dv  = tau ds I_3
 *     dX2/dw . r = tau (r x X1)                  i.e. the matrix -tau [X1]_x
 *     dX2/dlam = t_G ds + tau (v ds + w x (t_G ds))
 *   The correction is linear, so these derivatives are exact at any theta.
 *   Outputs:
 *     iwe [2][H][W] fp32 (optional, NULL)   as ramp_event_warp: plane 0 the polarity-signed sum, plane 1 the count
 *     sums  int64 [2]      the exact sums of the signed and of the count accumulators (units of 2^-24)
 *     stats float64 [8]    [0] the variance f, [1] the mean mu, [2] sum_u I(u)^2, [3] P_n, the rest 0 -- of the signed image,
 *                          or of the count image with RAMP_CONTRAST_UNSIGNED
 *     grad  float64 [7] (optional, NULL)    df/dtheta in the order (v, w, lam)
 *     status int32 [8]     ramp_event_warp's words; bit 1 of word 0: RAMP_CONTRAST_BAD_CORRECTION
 *   Determinism: the accumulators and the two sums are integer sums, the squares are centred with mu before they are summed
 *   over the pixels in a fixed order: stats, sums and iwe do not depend on the order of the events.  grad is a sum of doubles
 *   in an order fixed by the arguments: it repeats its bits from call to call; another order of the events moves it by the
 *   rounding of a float64 sum.  No floating-point atomics anywhere.
 *   Failures, never a plausible number (RAMP_OK: outcomes of the data): RAMP_INTERP_BAD_TIMES, or a correction with an entry
 *   that is not finite (RAMP_CONTRAST_BAD_CORRECTION), make stats[0 .. 2], grad and iwe NaN and sums 0; status [4] - [6] are
 *   then zero.  An event that is not finite or rejected is counted and contributes nothing.  No contributing event: variance
 *   0 and gradient 0, the true values.
 *   ws: ramp_event_contrast_workspace_bytes(T, H, W) bytes, 16-byte aligned; sums, stats and grad 8-byte aligned.  Launches:
 *   at most five kernels (four without grad) behind one hipMemsetAsync, all on `stream`, nothing synchronised.
 *   N == 0: RAMP_OK, nothing is launched and nothing written.  N < 0, T < 1, H or W < 1, unknown flags, a t_ref that is not
 *   finite, a NULL sums / stats / status: RAMP_EINVAL; a short workspace: RAMP_EWORKSPACE.                                */
#define RAMP_CONTRAST_UNSIGNED 16
#define RAMP_CONTRAST_BAD_CORRECTION 2 /* status[0] bit 1 */
size_t ramp_event_contrast_workspace_bytes(int T, int H, int W);
int ramp_event_contrast(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                        const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth,
                        const float *correction, int flags, int H, int W, float *iwe, int64_t *sums, double *stats, double *grad,
                        void *ws, size_t ws_bytes, int32_t *status, void *stream);

/* ramp_event_align: contrast maximisation on the device.  Normalised gradient ascent with backtracking over the evaluations of
 * ramp_event_contrast (variance and gradient at a correction), the line search itself run by a one-wave kernel behind every
 * evaluation: one call enqueues the whole alignment, nothing is read back, nothing synchronised.  The arguments up to
 * `flags, H, W` are ramp_event_contrast's; `correction` is the start (device float [7], or NULL for zero).
 *   free_mask  bit i frees component i of theta = (v[3], w[3], lam): mask[i] = 1.0 or 0.0
 *   step       the first step length, in the units of theta;  iters: the accepted steps asked for
 *   max_evals  the evaluations enqueued (clamped to 1 + 9 * iters, at which the budget can never bind)
 * The definition is a state machine with one step per evaluation.  All state is float64 unless noted:
 *     theta[7], f, g[7], f0, length, gm[7], norm, trial[7];  int32 n_accepted, n_evals, halvings, reason, seen;
 *     history[iters];  the status[8] words of the evaluation at theta
 *   Set-up: theta = the start, length = step, reason = 0; the evaluation reads float32(theta).
 *   After evaluation e with its stats[0], grad[7], status[8]:
 *     reason != 0: nothing.  Otherwise n_evals += 1, seen |= status[0], and
 *     e == 0:                    f = f0 = stats[0], g = grad, keep status;  iters == 0 ? reason = ITERS : propose(new direction)
 *     e > 0, ft = stats[0] > f:  theta = trial, f = ft, g = grad, keep status, history[n_accepted++] = f, length *= 2,
 *                                halvings = 0;  n_accepted == iters ? reason = ITERS : propose(new direction)
 *     e > 0 otherwise (a NaN ft among them):  length *= 0.5, halvings += 1;
 *                                halvings == 9 ? reason = STALLED : propose(same direction): gm and norm as they are
 *   propose(new direction): gm[i] = g[i] * mask[i];  norm = sqrt(((((((0.0 + gm0^2) + gm1^2) + ...) + gm6^2), the products
 *     and sums rounded one by one in this order, sqrt correctly rounded;  not (norm > 0 && norm < inf): reason = FLAT, stop.
 *   Both proposals: trial[i] = theta[i] + (length * gm[i]) / norm; the next evaluation reads float32(trial[i]), rounded to
 *     nearest even, overflow to infinity allowed (RAMP_CONTRAST_BAD_CORRECTION then answers NaN: a rejected trial).
 *   After the last evaluation a reason still 0 becomes BUDGET: theta is the last accepted point, a valid ascent result.
 * Evaluations behind the one that set `reason` are enqueued all the same and return at their first statement (a device word
 * the step kernel sets): empty launches.  The segment launch runs once, in front of evaluation 0, whose word 0 carries its
 * RAMP_INTERP_BAD_TIMES bit.  That evaluation is then NaN, and NaN stops the machine at once (ITERS with iters == 0, FLAT
 * otherwise: gm is NaN under any mask), so no later evaluation, whose memset would have cleared the bit, ever runs: `seen`
 * and `status` carry it to the outputs whatever max_evals is.
 *   Outputs, all on the device, all written by the step kernel of the last evaluation:
 *     correction     float64 [7]     theta
 *     correction_f32 float [7]       the bits the evaluation at theta read: ready for ramp_event_contrast
 *     result         float64 [4]     f, f0, the final length, 0
 *     grad           float64 [7]     g, the gradient at theta
 *     history        float64 [iters] the accepted variances, NaN behind n_accepted (may be NULL when iters == 0)
 *     status         int32 [8]       the words of the evaluation at theta
 *     info           int32 [8]       [0] reason [1] n_accepted [2] n_evals [3] halvings [4] seen, the rest 0
 *   The result is the bits of the same loop run on the host over ramp_event_contrast: the statistics are integer sums, grad
 *   repeats its bits for equal arguments, and the loop's own arithmetic is the float64 operations written above.
 *   N == 0: no contrast launches; the step kernel alone answers for the all-zero statistics (FLAT, n_evals = 1, variance 0,
 *   the start).  ws: ramp_event_align_workspace_bytes(T, H, W) bytes, 16-byte aligned, at least
 *   ramp_event_contrast_workspace_bytes; the float64 outputs 8-byte, the others 4-byte aligned.  Launches: the segment launch,
 *   then per evaluation one hipMemsetAsync and five kernels, all on `stream`.
 *   NULL or misaligned pointers, iters < 0 or > 65536, max_evals < 1, free_mask outside 7 bits, a step or t_ref that is not
 *   finite, and what ramp_event_contrast refuses: RAMP_EINVAL; a short workspace: RAMP_EWORKSPACE.                        */
#define RAMP_ALIGN_ITERS 1
#define RAMP_ALIGN_STALLED 2
#define RAMP_ALIGN_FLAT 3
#define RAMP_ALIGN_BUDGET 4
#define RAMP_ALIGN_MAX_ITERS 65536
#define RAMP_ALIGN_TRIALS 9 /* the first trial of a direction and up to 8 halvings */
size_t ramp_event_align_workspace_bytes(int T, int H, int W);
int ramp_event_align(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                     const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth,
                     const float *correction, int flags, int H, int W, int free_mask, double step, int iters, int max_evals,
                     double *correction_out, float *correction_f32, double *result, double *grad, double *history,
                     int32_t *status, int32_t *info, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- event voxel grids (csrc/voxel.hip)
 *
 * ramp_event_voxel: the reference's "voxels" event representation (utils/transformers.py:21-125,
 * EventSequenceToVoxelGrid_Pytorch) for S slices of one event list in one call: every event votes into the two time bins next
 * to its normalised time stamp with linear weights, and the grid of a slice is standardised over its non-zero cells.
 *   events: x, y [N] fp32 pixel coordinates, t [N] float64, p [N] int8 polarity (0 is read as -1), as ramp_event_warp.
 *   offsets: DEVICE int64 [S + 1], never read by the host: slice s is the events [offsets[s], offsets[s + 1]); NULL with
 *   S == 1: one slice [0, N).  An empty slice gives an all-zero grid and a stats row of zeros.
 *   Votes, per slice (float64 up to ti, fp32 behind it, no FMA):
 *     t_first, t_last = the time stamps of the slice's first and last event BY POSITION (not min / max)
 *     deltaT = t_last - t_first, and 1.0 when that is 0
 *     tn  = ((bins - 1) * (t - t_first)) / deltaT              in this order
 *     ti  = floor(tn),   dts = float32(tn - ti)
 *     pol * (1.0f - dts) -> bin ti       when 0 <= ti < bins
 *     pol * dts          -> bin ti + 1   when 0 <= ti and ti + 1 < bins          (bins == 1: pol into bin 0)
 *   Pixels: the coordinate truncated toward zero (the reference's .long()); unlike the reference, which does not check, an
 *   event whose pixel lies outside the image is dropped and counted.  RAMP_VOXEL_SUBPIXEL: the two neighbours per axis of
 *   ramp_event_warp's scatter (floor, weights 1 - w and w, neighbours outside the image dropped); a neighbour's share of a
 *   vote v is (wx * wy) * v, two fp32 products in this order.  A NaN coordinate row -- what ramp_event_warp writes to xy_out
 *   for an invalid event -- is skipped and counted.  Integer-valued coordinates give the default mode's bits and words (a
 *   neighbour of weight zero does not make a pixel).
 *   Accumulation: FIXED POINT, llrint(ldexp(value, 24)) added with 64-bit INTEGER atomics into int64 accumulators
 *   [slices][bins][H][W]: the sums do not depend on the events' order, a call repeats its bits.  No float atomics.
 *   grid [S][bins][H][W] fp32: float(sum) * 2^-24 (rounds once), or with RAMP_VOXEL_NORMALIZE, over the n cells with sum != 0:
 *     mean = (the exact integer sum of those sums) / (n * 2^24)                        float64
 *     var  = sum((acc * 2^-24 - mean)^2) / (n - 1)     float64, per-workgroup partials in an order fixed by (bins, H, W)
 *     cell = float32((acc * 2^-24 - mean) / std) where std = sqrt(var) > 0, float32(acc * 2^-24 - mean) otherwise -- n == 1
 *     included, whose unbiased std is NaN, as in torch.  Cells with sum == 0 stay 0; n == 0 leaves the grid as it is.
 *   stats float64 [S][4], in every mode: n, mean, std, the sum of the non-zero cells (n == 0: zeros; n == 1: std NaN).
 *   status: device int32 [8], written by the call, summed over all slices: [0] bits (RAMP_VOXEL_BAD_OFFSETS: an offset is
 *   negative, exceeds N or decreases; RAMP_VOXEL_BAD_TIMES: the first or last time stamp of a non-empty slice is not
 *   finite), [1] events seen (those of the slices), [2] events with a coordinate or time stamp that is not finite, [3] finite
 *   events whose pixel lies outside the image, [4] events inside it without a vote (ti outside [0, bins), every event of a
 *   slice that fails its time check), [5] events that voted, [6], [7] 0.  [2] + [3] + [4] + [5] = [1].
 *   Failures, never a plausible number (RAMP_OK: outcomes of the data): RAMP_VOXEL_BAD_OFFSETS makes every grid and stats
 *   value NaN and no event is read ([1] - [5] are 0); RAMP_VOXEL_BAD_TIMES makes the grid and the stats row of that slice NaN.
 *   ws: 16-byte aligned.  ramp_event_voxel_workspace_bytes(s, bins, H, W) holds s slices at once; the entry works through the
 *   slices in chunks of as many as ws_bytes holds (at most 32768) and the result does not depend on the chunking; less than
 *   one slice's worth: RAMP_EWORKSPACE.  Launches per chunk: one hipMemsetAsync and four kernels (vote, count, spread, finish;
 *   no vote with N == 0), and once per call the check of the offsets; all on `stream`, nothing synchronised.
 *   N < 0, S, bins, H or W < 1, unknown flags, NULL offsets with S != 1, a NULL grid / stats / status / ws, NULL events with
 *   N > 0, stats or offsets not 8-byte aligned: RAMP_EINVAL.  bins * H * W >= 2^31: RAMP_EUNSUPPORTED.
 * ramp_event_voxel_grid_events(): the number of events one trip of the full vote grid covers; above it the workgroups take a
 * second trip.  ramp_event_voxel_lds_offsets(): the number of offsets of a chunk the vote launch stages in LDS; a chunk with
 * more searches them in global memory.                                                                                */
#define RAMP_VOXEL_NORMALIZE 1
#define RAMP_VOXEL_SUBPIXEL 2
#define RAMP_VOXEL_BAD_OFFSETS 1 /* status[0] bit 0 */
#define RAMP_VOXEL_BAD_TIMES 2   /* status[0] bit 1 */
size_t ramp_event_voxel_workspace_bytes(int slices, int bins, int H, int W);
long ramp_event_voxel_grid_events(void);
int ramp_event_voxel_lds_offsets(void);
int ramp_event_voxel(const float *x, const float *y, const double *t, const int8_t *p, long N, const int64_t *offsets, int S,
                     int bins, int H, int W, int flags, float *grid, double *stats, int32_t *status, void *ws, size_t ws_bytes,
                     void *stream);

/* ---------------------------------------------------------------- lens distortion (csrc/rectify.hip)
 *
 * The event kernels above model the camera as a pinhole (fx, fy, cx, cy).  These two entries stand between a real sensor and
 * them: ramp_event_rectify takes raw events to sub-pixel coordinates of a rectified pinhole camera (the xy format
 * ramp_event_voxel's RAMP_VOXEL_SUBPIXEL and ramp_event_warp accept, NaN rows included), ramp_image_rectify resamples a raw
 * frame into the same camera.
 *   camera: DEVICE float [RAMP_CAMERA_WORDS], never read by the host, 4-byte aligned:
 *     [RAMP_CAMERA_RAW .. +3]        the raw intrinsics fx, fy, cx, cy
 *     [RAMP_CAMERA_MODEL]            RAMP_CAM_PINHOLE, RAMP_CAM_RADTAN or RAMP_CAM_EQUIDISTANT, as a float
 *     [RAMP_CAMERA_COEFFS .. +4]     radtan: k1, k2, p1, p2, k3 (OpenCV's order); equidistant: k1 .. k4, 0; pinhole: not used
 *     [RAMP_CAMERA_ROTATION .. +8]   R [3][3] row-major, raw camera -> rectified camera; a caller without one writes the identity
 *     [RAMP_CAMERA_NEW .. +3]        the rectified intrinsics fx', fy', cx', cy'
 *     every other word 0.
 *   Models, (x, y) the normalised raw ray, all arithmetic fp32 without FMA:
 *     RAMP_CAM_PINHOLE       (xd, yd) = (x, y)
 *     RAMP_CAM_RADTAN        r2 = x^2 + y^2,  rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
 *                            xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),   yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y
 *     RAMP_CAM_EQUIDISTANT   (Kalibr "equidistant", OpenCV fisheye)  r = sqrt(x^2 + y^2),  th = atan(r),
 *                            thd = th (1 + th^2 (k1 + th^2 (k2 + th^2 (k3 + th^2 k4)))),  (xd, yd) = (thd / r)(x, y); r == 0: (x, y)
 * ramp_event_rectify: x, y [N] fp32 pixels of the raw sensor, or int32 with RAMP_RECTIFY_XY_I32 (converted to fp32; integer-
 *   valued floats give the same bits).  Per event, one lane:
 *     (xd, yd) = ((x - cx) / fx, (y - cy) / fy)
 *     the model is inverted with exactly RAMP_RECTIFY_ITERS Newton steps -- no data-dependent trip count:
 *       radtan: 2-D Newton with the analytic Jacobian J (symmetric), from (xd, yd): p <- p - J^-1 (distort(p) - (xd, yd))
 *       equidistant: thd = sqrt(xd^2 + yd^2); 1-D Newton on th from thd; (x, y) = (tan th / thd)(xd, yd), thd == 0: (xd, yd)
 *     the solution is ACCEPTED only when every iterate is finite, det J (d thd / d th) > 0 at the start and at every iterate
 *     (a hop across the fold of a strongly distorting polynomial is rejected, never returned), the final residual
 *     |distort(p) - (xd, yd)| in raw pixels (the components times fx, fy; equidistant: |thd(th) - thd| max(fx, fy)) is
 *     <= RAMP_RECTIFY_TOL, and for the equidistant model 0 <= th < pi / 2
 *     X = R (x, y, 1);   x' = fx' X / Z + cx',  y' = fy' Y / Z + cy'
 *   xy_out [N][2] fp32, 8-byte aligned; valid_out [N] uint8 (optional, NULL).  An event that is not valid gets a NaN row and 0.
 *   status: device int32 [8], written by the call: [0] bits (RAMP_RECTIFY_BAD_CAMERA: a word of the record is not finite, the
 *   model is unknown, or fx, fy, fx' or fy' is <= 0), [1] events, [2] x or y not finite, [3] not invertible, [4] behind
 *   (Z <= 0 or NaN, or a projection that is not finite), [5] valid but outside [0, W - 1] x [0, H - 1] -- the coordinates are
 *   still written -- [6] valid and inside, [7] 0.  [2] + [3] + [4] + [5] + [6] = [1].  RAMP_RECTIFY_BAD_CAMERA makes every row
 *   NaN; the finite events are then counted in [3].  Outcomes of the data: RAMP_OK.
 *   A row is a function of its own event and the record alone: its bits depend neither on N, nor on its position, nor on the
 *   order of the events, and a call repeats its bits.  One kernel behind one 32-byte hipMemsetAsync on `stream`, nothing
 *   synchronised.  N == 0: RAMP_OK, nothing is launched and nothing written.  N < 0, H or W < 1, unknown flags, a NULL x / y /
 *   camera / xy_out / status, xy_out not 8-byte aligned: RAMP_EINVAL.
 *   ramp_event_rectify_grid_events(): the number of events one trip of the full grid covers; above it the workgroups take a
 *   second trip.
 * ramp_image_rectify: the forward direction, closed form.  src [C][Hs][Ws] fp32, or uint8 with RAMP_RECTIFY_SRC_U8; out
 *   [C][H][W] fp32, the rectified camera's image.  Per output pixel (u, v), one lane for all channels:
 *     ray = R^T ((u - cx') / fx', (v - cy') / fy', 1);  (x, y) = (X / Z, Y / Z);  (xd, yd) = distort(x, y)
 *     xs = fx xd + cx,  ys = fy yd + cy
 *   The pixel is SAMPLED when Z > 0, det J (d thd / d th) > 0 at the ray, xs and ys are finite, and 0 <= xs <= Ws - 1,
 *   0 <= ys <= Hs - 1; with x0 = floor(xs), wx = xs - x0 (y likewise) and a, b, c, d the source at (x0, y0), (x0 + 1, y0),
 *   (x0, y0 + 1), (x0 + 1, y0 + 1) -- an index past the last row or column is clamped, its weight is then exactly 0:
 *     top = (1 - wx) a + wx b,  bot = (1 - wx) c + wx d,  val = (1 - wy) top + wy bot       fp32, every product and sum rounded
 *   norm: RAMP_RECTIFY_NORM_NONE val; _HALF 2 (val / 255) - 0.5; _UNIT 2 (val / 255) - 1 (the two branches of the reference's
 *   normalize_image, ramp/utils.py:573-583; a correctly rounded fp32 division).  Any other pixel gets `fill` in every channel.
 *   map_out [H][W][2] fp32 (optional, 8-byte aligned): (xs, ys), NaN where the pixel is not sampled; mask_out [H][W] uint8
 *   (optional): 1 where sampled.
 *   status: device int32 [8]: [0] bits (RAMP_RECTIFY_BAD_CAMERA: every pixel is `fill` and counted in [2]), [1] pixels, [2] not
 *   sampled by the fold, a ray behind the camera or coordinates that are not finite, [3] outside the source, [4] sampled,
 *   [5] - [7] 0.  [2] + [3] + [4] = [1].  One kernel behind one 32-byte hipMemsetAsync on `stream`, nothing synchronised; a
 *   pixel's bits depend on its own coordinates, the record and the source alone.
 *   C, Hs, Ws, H or W < 1, unknown flags or norm, a NULL src / camera / out / status, a misaligned map_out: RAMP_EINVAL; H W or
 *   Hs Ws >= 2^31: RAMP_EUNSUPPORTED.                                                                                  */
#define RAMP_CAMERA_WORDS 32
#define RAMP_CAMERA_RAW 0
#define RAMP_CAMERA_MODEL 4
#define RAMP_CAMERA_COEFFS 5
#define RAMP_CAMERA_ROTATION 12
#define RAMP_CAMERA_NEW 24
#define RAMP_CAM_PINHOLE 0
#define RAMP_CAM_RADTAN 1
#define RAMP_CAM_EQUIDISTANT 2
#define RAMP_RECTIFY_ITERS 8
#define RAMP_RECTIFY_TOL 0.015625f /* 2^-6 raw pixels */
#define RAMP_RECTIFY_XY_I32 1
#define RAMP_RECTIFY_SRC_U8 2
#define RAMP_RECTIFY_NORM_NONE 0
#define RAMP_RECTIFY_NORM_HALF 1
#define RAMP_RECTIFY_NORM_UNIT 2
#define RAMP_RECTIFY_BAD_CAMERA 1 /* status[0] bit 0 */
long ramp_event_rectify_grid_events(void);
int ramp_event_rectify(const void *x, const void *y, long N, const float *camera, int flags, int H, int W, float *xy_out,
                       uint8_t *valid_out, int32_t *status, void *stream);
int ramp_image_rectify(const void *src, int C, int Hs, int Ws, const float *camera, int flags, int norm, float fill, int H, int W,
                       float *out, float *map_out, uint8_t *mask_out, int32_t *status, void *stream);

/* ---------------------------------------------------------------- event denoising (csrc/filter.hip)
 *
 * ramp_event_filter: the first step behind a real sensor -- a hot-pixel mask, a refractory period and the 8-neighbour
 * background-activity filter over one event list, order-independent and bit-exact.  The xy it writes is the format
 * ramp_event_rectify (fp32 path), RAMP_VOXEL_SUBPIXEL, ramp_event_warp and ramp_event_contrast take: a NaN row for every event
 * that is not kept, which they skip and count.
 *   events: x, y [N] fp32, or int32 with RAMP_FILTER_XY_I32 (converted to fp32; integer-valued floats give the same bits);
 *   t [N] float64.  The pixel is the coordinate truncated toward zero, as in ramp_event_voxel.  Polarity takes no part.
 *   Candidates: an event whose x, y or t is not finite is class [2]; a finite event whose pixel is outside the sensor is
 *   class [3]; the rest are CANDIDATES.
 *   Order: within a pixel the order of the indices; the time stamps of every pixel's candidates must not decrease in that
 *   order (a time-sorted stream satisfies this).  Across pixels e' PRECEDES e when (t', index') < (t, index)
 *   lexicographically -- on a globally time-sorted stream the order of the indices.
 *   Hot pixels: c[q] = the number of candidates at pixel q, n = the number of pixels with c >= 1, S1 = sum c, S2 = sum c^2
 *   (exact int64).  In float64, in this order, without FMA:
 *     mean = S1 / n,   var = max(S2 / n - mean * mean, 0),   thr = mean + hot_sigma * sqrt(var)
 *   q is hot when hot_count > 0 and c[q] > hot_count, or hot_sigma > 0 and c[q] > thr, or hot_in[q] != 0 (hot_in: optional
 *   uint8 [H][W]).  Every candidate at a hot pixel is class [4]; it gives no support and does not touch the state.
 *   State: last_t_in, optional float64 [H][W]: per non-hot pixel the time stamp of the last candidate seen there in earlier
 *   calls, NaN for none; it acts as one virtual event that precedes every event of the call at that pixel.  NULL: all NaN.
 *   Refractory period (refractory > 0): t_own = the time stamp of the IMMEDIATE predecessor at the candidate's own pixel --
 *   the previous candidate there, kept or not, else the state; class [5] when t - t_own < refractory (a float64 subtraction).
 *   History-free on purpose: an event's outcome is a function of the raw stream (the chained variant is not built).
 *   Background activity (support_dt >= 0; negative: off): for each of the 8 neighbour pixels -- the own pixel excluded, a
 *   neighbour outside the sensor or hot skipped -- t_nb = the time stamp of the neighbour's last candidate that precedes the
 *   event, else the neighbour's state; the event has SUPPORT when some neighbour has t - t_nb <= support_dt.  A candidate
 *   without support is class [6].  An event dropped by the refractory test still supports its neighbours.
 *   Every other candidate is KEPT, class [7].  The first class that applies, [2] to [7], is the one counted.
 *   On a globally time-sorted stream this is, event for event, the textbook sequential filter over a last-time-stamp map
 *   (test the own entry, test the eight neighbours' entries, write the own entry).
 *   Outputs (optional ones NULL; keep_out and status are required):
 *     keep_out [N] uint8: 1 for class [7], else 0.  xy_out [N][2] fp32, 8-byte aligned: the input coordinates for kept events,
 *     a NaN row for every other.  index_out [N] int32: the K kept indices in ascending order, then -1.  count_out: K as a
 *     device int64.  hot_out [H][W] uint8: the final mask, hot_in included.  stats_out float64 [4]: n, mean, std, thr (thr NaN
 *     when hot_sigma <= 0; n == 0: 0 and three NaN).  last_t_out [H][W] float64: per non-hot pixel its last candidate's time
 *     stamp, else last_t_in's value; written by a launch of its own behind the filter launch, so last_t_out == last_t_in is
 *     allowed.
 *   status: device int32 [8], written by the call: [0] bits (RAMP_FILTER_BAD_ORDER: a pixel's candidates decrease in time in
 *   index order, or a pixel's first candidate lies before its state -- hot pixels included), [1] events, [2] - [7] the class
 *   counts; [2] + ... + [7] = [1].
 *   RAMP_FILTER_BAD_ORDER is an outcome of the data (RAMP_OK), never a plausible number: every keep is 0, xy_out NaN, count 0,
 *   index_out -1, last_t_out and stats_out NaN, [4] - [7] 0 ([1] - [3] are still counted; hot_out is the mask of the counts,
 *   which do not depend on the order).
 *   Launches, all on `stream`, nothing synchronised, no floating-point atomics, every loop a binary search or of fixed length:
 *   one memset; the key kernel; a STABLE radix sort of (pixel, index) over ceil(log2(H W + 1)) bits (hipcub); the segment
 *   kernel (per-pixel offsets by binary search: counts are differences, not atomics); the hot stage (integer sums and the order
 *   check, then threshold and mask); the filter kernel, one lane per sorted position (the own predecessor at position - 1,
 *   eight binary searches over the neighbours' segments); with index_out a scan (hipcub) and the compaction; the state and
 *   status launch.  The result is a function of the input alone: a call repeats its bits.
 *   N == 0: RAMP_OK, nothing is launched and nothing written except a copy last_t_in -> last_t_out when both are given and
 *   differ.  N < 0, H or W < 1, unknown flags, a NULL keep_out / status (N > 0: x / y / t / ws), xy_out, last_t_in, last_t_out,
 *   stats_out or count_out not 8-byte aligned, ws not 16-byte aligned, refractory < 0, refractory or support_dt not finite:
 *   RAMP_EINVAL.  N >= 2^31 or H W >= 2^31 - 1: RAMP_EUNSUPPORTED.  ws_bytes below
 *   ramp_event_filter_workspace_bytes(N, H, W): RAMP_EWORKSPACE.
 * ramp_event_filter_grid_events(): the number of events one trip of the full grid covers; above it the workgroups take a
 * second trip.                                                                                                        */
#define RAMP_FILTER_XY_I32 1
#define RAMP_FILTER_BAD_ORDER 1 /* status[0] bit 0 */
size_t ramp_event_filter_workspace_bytes(long N, int H, int W);
long ramp_event_filter_grid_events(void);
int ramp_event_filter(const void *x, const void *y, const double *t, long N, int H, int W, int flags, double support_dt,
                      double refractory, int hot_count, double hot_sigma, const uint8_t *hot_in, const double *last_t_in,
                      double *last_t_out, uint8_t *keep_out, float *xy_out, int32_t *index_out, int64_t *count_out,
                      uint8_t *hot_out, double *stats_out, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- event optical flow (csrc/flow.hip)
 *
 * ramp_event_flow: how the image moves at each event, without a trajectory and without a depth -- per event a plane fitted to
 * the surface of active events around it at its own time (Benosman et al., "Event-based visual flow", TNNLS 2014).  The result
 * is the NORMAL flow.  Order-independent and bit-exact: every rounding below is fixed.
 *   Events: x, y [N] fp32, or int32 with RAMP_FLOW_XY_I32; t [N] float64; p [N] int8, optional (NULL).  The pixel is the
 *   coordinate truncated toward zero, and the finiteness and range tests are ramp_event_filter's: class [2] is an event that is
 *   not finite, class [3] an event outside the sensor, the rest are CANDIDATES.
 *   Surfaces: without p one; with p two (p > 0 is plane 1, else plane 0), and an event sees only its own plane.  With S the
 *   number of planes a CELL is (plane, pixel), its key plane * H * W + pixel.
 *   Order: within a cell the order of the indices; every cell's time stamps must not decrease in that order.  Across cells e'
 *   PRECEDES e when (t', i') < (t, i) lexicographically (ramp_event_filter's rule).
 *   State: last_t_in, optional float64 [S][H][W], NaN meaning none: one virtual event per cell that precedes the call's.
 *   last_t_out: per cell the last candidate's time stamp, else the input's value; written by a launch of its own, so
 *   last_t_out == last_t_in is allowed.  With S = 1 it is the array of ramp_event_filter's and ramp_time_surface's last_t.
 *   Points: for a candidate at (qx, qy) with (t, i), every offset j = (dy + r) * (2r + 1) + (dx + r), dx, dy in -r .. r, r in
 *   1 .. 3, in ascending j.  The centre is always a point with s = 0 (the event overwrites its own surface entry: its own
 *   predecessor takes no part).  A neighbour outside the sensor is skipped.  Otherwise t_nb = the time stamp of the last
 *   candidate of cell (own plane, neighbour pixel) that precedes the event, else that cell's state, else none; with
 *   delta = t - t_nb (one float64 subtraction) the neighbour is a point with s = -delta when delta <= window_dt (a NaN
 *   compares false).
 *   Fit: n, Sx, Sy, Sxx, Sxy, Syy are exact integers over the points; Sxs = sum (double)dx * s, Sys = sum (double)dy * s,
 *   Ss = sum s in float64, without FMA, added in ascending j from +0 (a skipped offset adds nothing).  The int64 cofactors
 *     C00 = Syy n - Sy Sy    C01 = Sx Sy - Sxy n    C02 = Sxy Sy - Syy Sx
 *     C11 = Sxx n - Sx Sx    C12 = Sxy Sx - Sxx Sy   C22 = Sxx Syy - Sxy Sxy        D = Sxx C00 + Sxy C01 + Sx C02
 *   Class [4] when n < min_points, class [5] when D == 0.  Otherwise, each integer converted exactly,
 *     a = ((C00 Sxs + C01 Sys) + C02 Ss) / D    b = ((C01 Sxs + C11 Sys) + C12 Ss) / D    c = ((C02 Sxs + C12 Sys) + C22 Ss) / D
 *   Refinement (refine in 0 .. 2 passes): a non-centre point is dropped when fabs(s - ((a * dx + b * dy) + c)) > outlier_dt,
 *   all points tested against the same fit.  Nothing dropped: the passes end.  Otherwise the sums and the fit are recomputed
 *   over the remaining points, with the same two class tests.
 *   Flow: g2 = a * a + b * b, vx = a / g2, vy = b / g2.  Class [6] ("flat") when g2 is not positive, when vx or vy is not
 *   finite, or when vx * vx + vy * vy > max_speed * max_speed (max_speed = +inf is allowed).  Everything else is valid, class
 *   [7].  The first class that applies, [2] to [7], is the one counted.
 *   Outputs (optional ones NULL; flow and status are required):
 *     flow [N][2] fp32, 8-byte aligned: (float)vx, (float)vy in pixels per unit of t; every row that is not class [7] is NaN.
 *     cls [N] uint8: the class.  n_used [N] uint8: the final n, 0 for classes [2] and [3].  fit [N][3] float64: a, b, c, NaN
 *     where the final fit was not formed (classes [2] to [5]).
 *     flow_map [2][H][W] fp32 and map_index [H][W] int32 (both or neither): per pixel the flow and the index of the valid event
 *     with the LARGEST INDEX at that pixel, over both planes; NaN and -1 without one.  An int32 atomicMax of the index, then a
 *     resolve pass with one writer per pixel.
 *     last_t_out.  status: device int32 [8]: [0] bit 0 RAMP_FLOW_BAD_ORDER, [1] events, [2] .. [7] the class counts;
 *     [2] + ... + [7] = [1].
 *   RAMP_FLOW_BAD_ORDER (a cell's candidates decrease in time in index order, or its first candidate lies before its state) is
 *   an outcome of the data (RAMP_OK), never a plausible number: flow, fit, flow_map and last_t_out are NaN, map_index is -1,
 *   every cls and n_used is 0, [4] .. [7] are 0 ([1] .. [3] are still counted).
 *   Launches, all on `stream`, nothing synchronised, no floating-point atomics, every loop a binary search or of fixed length:
 *   memsets; the key kernel; a STABLE radix sort of (cell, index) over ceil(log2(S H W + 1)) bits (hipcub); the segment kernel;
 *   the time-stamp gather with the order check; the fit kernel, one lane per sorted position, templated on r ((2r + 1)^2 - 1
 *   binary searches, the points' s in an LDS slab [j][lane], the used set a 64-bit mask; 256 lanes per workgroup, 128 at
 *   r = 3); the state, map and status launch.  The result is a function of the input alone: a call repeats its bits.
 *   N == 0: RAMP_OK, no kernel is launched: status is zeroed, flow_map is NaN and map_index -1, last_t_in is copied to
 *   last_t_out when both are given and differ -- S planes, S = 2 when p is not NULL -- (last_t_out without last_t_in is left
 *   as it is).
 *   RAMP_EINVAL: r outside 1 .. 3, min_points outside 3 .. (2r + 1)^2, refine outside 0 .. 2, window_dt or outlier_dt negative
 *   or NaN, max_speed NaN or <= 0, N < 0, H or W < 1, unknown flags, a NULL status (N > 0: flow / x / y / t / ws), one of
 *   flow_map / map_index without the other, flow, fit, last_t_in or last_t_out not 8-byte aligned, status, flow_map or map_index
 *   not 4-byte aligned, ws not 16-byte aligned.  RAMP_EUNSUPPORTED: N >= 2^31 or 2 H W >= 2^31 - 1.  RAMP_EWORKSPACE: ws_bytes
 *   below ramp_event_flow_ws_bytes(N, H, W, planes) (planes: 1 without p, 2 with; 0 for sizes that are refused).  A refused call
 *   touches nothing.
 * ramp_event_flow_grid_events(): the number of events one trip of the full grid covers at r <= 2 (half of it at r = 3); above
 * it the workgroups take a second trip.                                                                                 */
#define RAMP_FLOW_XY_I32 1
#define RAMP_FLOW_BAD_ORDER 1 /* status[0] bit 0: the value of RAMP_FILTER_BAD_ORDER */
size_t ramp_event_flow_ws_bytes(long N, int H, int W, int planes);
long ramp_event_flow_grid_events(void);
int ramp_event_flow(const void *x, const void *y, const double *t, const int8_t *p, long N, int H, int W, int flags, int r,
                    double window_dt, int min_points, int refine, double outlier_dt, double max_speed, const double *last_t_in,
                    double *last_t_out, float *flow, uint8_t *cls, uint8_t *n_used, double *fit, float *flow_map,
                    int32_t *map_index, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- event corner detection (csrc/corner.hip)
 *
 * ramp_event_corners: which events are corners -- FAST-style arcs of newest events on the surface of active events around each
 * event at its own time (Mueggler, Bartolozzi and Scaramuzza, "Fast Event-based Corner Detection", BMVC 2017; with
 * RAMP_CORNER_WIDE the Arc* acceptance of Alzugaray and Chli, RA-L 2018).  Order-independent and bit-exact: time stamps are
 * only compared, there is no floating-point arithmetic and no tolerance anywhere.
 *   Shared with ramp_event_flow, word for word: events (x, y [N] fp32, or int32 with RAMP_CORNER_XY_I32; t [N] float64; p [N]
 *   int8, optional), pixels (the coordinate truncated toward zero), candidates, class [2] (not finite) and class [3] (outside
 *   the sensor); the planes S (1 without p, 2 with; p > 0 is plane 1) and the rule that an event sees only its own plane; cells
 *   (plane, pixel), the order within a cell (the indices; time stamps must not decrease) and across cells (e' PRECEDES e when
 *   (t', i') < (t, i) lexicographically); the state last_t_in / last_t_out (float64 [S][H][W], NaN = none, one virtual event per
 *   cell that precedes the call's, in place allowed), and RAMP_CORNER_BAD_ORDER with its emptying behaviour.  With S = 1 the
 *   state is the very array of ramp_event_filter, ramp_time_surface and ramp_event_flow.
 *   Circles: the order of each list is part of the definition; k ascends along each list, each entry is (dx, dy).
 *     inner, n = 16: (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3)
 *     outer, n = 20: (0,4) (1,4) (2,3) (3,2) (4,1) (4,0) (4,-1) (3,-2) (2,-3) (1,-4) (0,-4) (-1,-4) (-2,-3) (-3,-2) (-4,-1)
 *                    (-4,0) (-4,1) (-3,2) (-2,3) (-1,4)
 *   Class [4], border: a candidate with qx < 4, qy < 4, qx > W - 5 or qy > H - 5 (its outer circle is not wholly on the sensor).
 *   A sensor with H < 9 or W < 9 has only border pixels: valid, not refused.
 *   Per circle: v[k] = the time stamp of the last candidate of cell (own plane, circle pixel k) that precedes the event (t, i),
 *   else that cell's state, else NaN, which counts as below every number.  The event's own pixel and its own predecessor take
 *   no part.  An ARC (start, L) is the cyclic run k = start, start + 1, .., start + L - 1 (mod n).  It PASSES when every v on it
 *   is strictly greater than every v off it: equal values across the boundary fail, an arc that holds a NaN fails.  The lengths
 *   allowed are lo .. hi (the published values: inner 3 .. 6, outer 4 .. 8; parameters, 1 <= lo <= hi <= n - 1); with
 *   RAMP_CORNER_WIDE an arc also passes when n - L is in lo .. hi (the complement of a wide arc of oldest events).  Several
 *   lengths can pass (the sets above a threshold are nested): the arc REPORTED is the one with the smallest L; its start is the
 *   one index whose predecessor is off the arc.  L = n cannot pass.  Equivalently: for an element e with a number let
 *   m_e = {k : v[k] >= v[e]}; the circle passes exactly when some m_e is a cyclic run of an allowed size.
 *   Classes: [5] the inner circle has no passing arc; [6] the inner circle passes, the outer does not; [7] both pass: a corner.
 *   The first class that applies, [2] to [7], is the one counted.
 *   Outputs (optional ones NULL; cls and status are required):
 *     cls [N] uint8: the class.  arc [N][4] uint8, 4-byte aligned: inner start, inner L, outer start, outer L; zeros for a
 *     circle that was not evaluated or did not pass.
 *     index [N] int32 and count [1] int32 (both or neither): the corner events' indices ascending, -1 beyond the count.
 *     corner_count [H][W] int32: corner events per pixel over both planes (int32 atomic adds).
 *     last_t_out.  status: device int32 [8]: [0] bit 0 RAMP_CORNER_BAD_ORDER, [1] events, [2] .. [7] the class counts;
 *     [2] + ... + [7] = [1].
 *   RAMP_CORNER_BAD_ORDER (a cell's candidates decrease in time in index order, or its first candidate lies before its state)
 *   is an outcome of the data (RAMP_OK), never a plausible answer: every cls and arc is 0, index is -1, count 0, corner_count 0,
 *   last_t_out NaN, [4] .. [7] are 0 ([1] .. [3] are still counted).
 *   Launches, all on `stream`, nothing synchronised, no floating-point atomics, every loop a binary search or of fixed length:
 *   memsets; the key kernel; a STABLE radix sort of (cell, index) over ceil(log2(S H W + 1)) bits (hipcub); the segment kernel;
 *   the time-stamp gather with the order check; the corner kernel, one lane per sorted position (16 binary searches into
 *   registers and the inner test; for the lanes that passed 20 more and the outer test); with index, a running count of the
 *   corner flags (hipcub); the state, index and status launch.  The result is a function of the input alone: a call repeats
 *   its bits.
 *   N == 0: RAMP_OK, no kernel is launched: status, count and corner_count are zeroed, last_t_in is copied to last_t_out when
 *   both are given and differ -- S planes, S = 2 when p is not NULL -- (last_t_out without last_t_in is left as it is).
 *   RAMP_EINVAL: an arc range outside 1 <= lo <= hi <= n - 1, N < 0, H or W < 1, unknown flags, a NULL status (N > 0: cls / x /
 *   y / t / ws), one of index / count without the other, last_t_in or last_t_out not 8-byte aligned, status, arc, index, count
 *   or corner_count not 4-byte aligned, ws not 16-byte aligned.  RAMP_EUNSUPPORTED: N >= 2^31 or 2 H W >= 2^31 - 1.
 *   RAMP_EWORKSPACE: ws_bytes below ramp_event_corners_ws_bytes(N, H, W, planes) (planes: 1 without p, 2 with; 0 for sizes that
 *   are refused).  A refused call touches nothing.
 * ramp_event_corners_grid_events(): the number of events one trip of the full grid covers; above it the workgroups take a
 * second trip.                                                                                                           */
#define RAMP_CORNER_XY_I32 1
#define RAMP_CORNER_WIDE 2
#define RAMP_CORNER_BAD_ORDER 1 /* status[0] bit 0: the value of RAMP_FILTER_BAD_ORDER */
size_t ramp_event_corners_ws_bytes(long N, int H, int W, int planes);
long ramp_event_corners_grid_events(void);
int ramp_event_corners(const void *x, const void *y, const double *t, const int8_t *p, long N, int H, int W, int flags,
                       int inner_lo, int inner_hi, int outer_lo, int outer_hi, const double *last_t_in, double *last_t_out,
                       uint8_t *cls, uint8_t *arc, int32_t *index, int32_t *count, int32_t *corner_count, int32_t *status,
                       void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- event corner tracks (csrc/cornertrack.hip)
 *
 * ramp_event_corner_tracks: links corner events in space and time into feature tracks -- each with an identity, a birth and a
 * length -- and gives the full two-component image velocity at each of them, the mean since the track's birth.  Every
 * CANDIDATE is linked to the newest candidate around it that precedes it by at most max_dt; without one a track is born.
 * Order-independent and bit-exact: time stamps are compared, subtracted once and divided once, every rounding below is fixed.
 *   Shared with ramp_event_corners, word for word: events (x, y [N] fp32, or int32 with RAMP_CORNER_TRACK_XY_I32; t [N]
 *   float64; p [N] int8, optional), pixels (the coordinate truncated toward zero), class [2] (not finite) and class [3]
 *   (outside the sensor); the planes S (1 without p, 2 with; p > 0 is plane 1) and the rule that an event sees only its own
 *   plane; cells (plane, pixel), the order within a cell (the indices; time stamps must not decrease) and across cells (e'
 *   PRECEDES e when (t', i') < (t, i) lexicographically), and RAMP_CORNER_TRACK_BAD_ORDER with its emptying behaviour.
 *   Candidates: corner, uint8 [N], nonzero = the event is a candidate (ramp_event_corners' cls == 7, or any mask); NULL: every
 *   valid event is one.  A valid event that is not a candidate is class [4]: it takes no part and leaves the state alone.
 *   State: state_in, optional int64 [S][H][W][4], one record per cell: word 0 the bits of t (NaN = none), word 1 the track
 *   id, word 2 the bits of t0, word 3 the birth pixel index y0 * W + x0 in the low 32 bits and the length in the high 32 bits.
 *   A record with a number in word 0 is one virtual candidate of its cell that precedes the call's.  next_id_in, a device
 *   int64 word, goes with it (both or neither; neither: empty state, ids from 0).  The state is also the live-track map: a
 *   cell with t >= now - max_dt holds a live track's newest corner.  Nothing is pruned by age.
 *   Parent of a candidate e at pixel (qx, qy) with (t, i): walk the (2 rho + 1)^2 window clipped to the sensor, the own pixel
 *   included, in ascending j = (dy + rho) * (2 rho + 1) + (dx + rho).  In each cell take the last candidate of e's own plane
 *   that precedes e; if there is none, the cell's state record.  The cell is ELIGIBLE when that time stamp t' is a number
 *   (not NaN) and t - t' <= max_dt (one float64 subtraction, no FMA).  The parent is the eligible cell with the greatest t';
 *   ties go to the smallest dx^2 + dy^2, then to the lowest j.  No index takes part in the choice: a state record and an event
 *   of this call compete on equal terms.
 *   Classes: [5] no eligible cell, a track is born; [6] the parent is a state record; [7] the parent is an event of this
 *   call.  The first class that applies, [2] to [7], is the one counted.
 *   Tracks: a parent strictly precedes its child, so the parent relation is a forest.  A ROOT is an event of class [5] or [6].
 *   A root of class [5] with index r: track = next_id_in + r, birth = (t_r, qx_r, qy_r), length = 1.  A root of class [6]:
 *   track and birth are the record's, length = the record's + 1.  Every other event takes track and birth from its root and
 *   length = length(parent) + 1.  length saturates at 2^31 - 1.  next_id_out = next_id_in + N: ids are global event numbers,
 *   so a stream fed in pieces gets the ids of the stream fed whole.
 *   velocity = ((float)((qx - x0) / (t - t0)), (float)((qy - y0) / (t - t0))): exact integer differences converted to
 *   float64, one float64 subtraction, one float64 division each, no FMA; NaN when t == t0, which includes every birth.  It is
 *   the MEAN velocity since birth; parent lets a consumer walk back for anything more local.
 *   state_out: per cell the record (t, track, t0, birth pixel | length << 32) of its last candidate in this call, else the
 *   record of state_in (else NaN, 0, 0, 0); the state is read by the link launch alone and written by the last one, so
 *   state_out == state_in and next_id_out == next_id_in are allowed.
 *   Outputs (optional ones NULL; cls, status and, with N > 0, state_out and next_id_out are required):
 *     cls [N] uint8: the class.  parent [N] int32: the parent's event index, -1 for a birth or a non-candidate, -2 for a state
 *     record.  track [N] int64: -1 for non-candidates.  length [N] int32: 0 for non-candidates.  birth [N][3] float64: t0, x0,
 *     y0, NaN for non-candidates.  velocity [N][2] fp32, NaN for non-candidates.
 *     status: device int32 [8]: [0] bit 0 RAMP_CORNER_TRACK_BAD_ORDER, [1] events, [2] .. [7] the class counts;
 *     [2] + ... + [7] = [1].
 *   RAMP_CORNER_TRACK_BAD_ORDER (a cell's candidates decrease in time in index order, or its first candidate lies before its
 *   state's t) is an outcome of the data (RAMP_OK), never a plausible answer: every cls and length is 0, parent and track are
 *   -1, birth and velocity NaN, every cell of state_out has word 0 = NaN and the rest 0, next_id_out = next_id_in + N,
 *   [4] .. [7] are 0 ([1] .. [3] are still counted).
 *   Launches, all on `stream`, nothing synchronised, no LDS, no atomics on results, no floating-point atomics, every loop a
 *   binary search or of fixed length: a memset; the key kernel (a non-candidate takes the sentinel key, as an invalid event
 *   does); a STABLE radix sort of (cell, index) over ceil(log2(S H W + 1)) bits (hipcub); the segment kernel; the time-stamp
 *   gather with the order check; the link kernel, one lane per sorted position ((2 rho + 1)^2 binary searches, the running
 *   best (t', d^2) and its source -- a sorted position or a state cell -- in registers); ceil(log2(max(N, 2))) rounds of
 *   pointer jumping over sorted positions between two buffers of (ancestor, links to it), launched unconditionally -- the
 *   host never learns the candidate count -- and never in place; the resolve launch (track, birth, length, velocity and parent
 *   from the roots, the state, next_id_out, the status words).  The result is a function of the input alone: a call repeats
 *   its bits.
 *   N == 0: RAMP_OK, no kernel is launched: status is zeroed, state_in is copied to state_out and next_id_in to next_id_out
 *   where both are given and differ -- S planes, S = 2 when p is not NULL -- (an output without its input is left as it is).
 *   RAMP_EINVAL: rho outside 0 .. 5, max_dt NaN or negative (+inf is allowed), N < 0, H or W < 1, unknown flags, a NULL
 *   status (N > 0: cls / state_out / next_id_out / x / y / t / ws), one of state_in / next_id_in without the other, state_in,
 *   state_out, next_id_in, next_id_out, track or birth not 8-byte aligned, status, parent, length or velocity not 4-byte
 *   aligned, ws not 16-byte aligned.  RAMP_EUNSUPPORTED: N >= 2^31 or 2 H W >= 2^31 - 1.  RAMP_EWORKSPACE: ws_bytes below
 *   ramp_event_corner_tracks_ws_bytes(N, H, W, planes) (planes: 1 without p, 2 with; 0 for sizes that are refused).  A
 *   refused call touches nothing.
 * ramp_event_corner_tracks_grid_events(): the number of events one trip of the full grid covers; above it the workgroups take
 * a second trip.                                                                                                         */
#define RAMP_CORNER_TRACK_XY_I32 1
#define RAMP_CORNER_TRACK_BAD_ORDER 1 /* status[0] bit 0: the value of RAMP_FILTER_BAD_ORDER */
size_t ramp_event_corner_tracks_ws_bytes(long N, int H, int W, int planes);
long ramp_event_corner_tracks_grid_events(void);
int ramp_event_corner_tracks(const void *x, const void *y, const double *t, const int8_t *p, const uint8_t *corner, long N, int H,
                             int W, int flags, int rho, double max_dt, const int64_t *state_in, const int64_t *next_id_in,
                             int64_t *state_out, int64_t *next_id_out, uint8_t *cls, int32_t *parent, int64_t *track,
                             int32_t *length, double *birth, float *velocity, int32_t *status, void *ws, size_t ws_bytes,
                             void *stream);

/* ---------------------------------------------------------------- event landmarks (csrc/landmark.hip)
 *
 * ramp_event_landmarks: one corner track, seen from the camera poses at its own events' time stamps, is one 3-D point.  Every
 * track of ramp_event_corner_tracks is triangulated along the trajectory: a midpoint solve, a fixed number of Gauss-Newton steps
 * on the reprojection error, a covariance in the convention of ramp_ba_map_covariance and a class that says why a landmark is
 * not valid.
 *   Inputs: x, y [N] fp32 pixel coordinates of the pinhole camera `intrinsics` (device fx, fy, cx, cy) -- what ramp_event_warp
 *   takes; raw pixels are rectified first.  t [N] float64.  track [N] int64: ramp_event_corner_tracks' output, negative = the
 *   event observes nothing.  knots [T][7], times [T]: a CAMERA-TO-WORLD trajectory as for ramp_event_warp.  flags:
 *   RAMP_INTERP_EXTRAPOLATE alone.
 *   An event is an OBSERVATION when track >= 0, x, y and t are finite, and times[0] <= t <= times[T - 1] (with
 *   RAMP_INTERP_EXTRAPOLATE: any finite t).  The first test that fails counts the event: no track [1], not finite [2], outside
 *   the knots' range [3].  Its pose C_i = (c_i, q_i) is ramp_se3_interp's at t_i (the same s, the same alpha formed in float64
 *   and rounded once, the same statements: the same bits).  The camera ray is f_i = ((x - cx) / fx, (y - cy) / fy, 1) in fp32,
 *   its world direction d_i = q_i f_i (the rotation of ramp_event_warp, fp32), and ev_ray[i] = (c_i, d_i), six fp32 words: the
 *   call's own record.  EVERYTHING BEHIND THIS POINT IS FLOAT64 computed from fp32 words -- c_i, d_i, q_i, x_i, y_i, the
 *   intrinsics -- each converted exactly: u_i = d_i / |d_i|, R_i the rotation of q_i / |q_i|.
 *   Landmarks: the set of observations with one id, numbered in ascending id; lm_track[l] is the id.  Within a landmark the
 *   observations are ordered by (t, index) (-0.0 is 0.0).  count[0] = min(tracks seen, max_landmarks): the highest ids are cut
 *   off and counted, as ramp_point_map_export cuts at max_out; rows from count[0] on are not written.  ev_landmark[i]: the
 *   landmark number of observation i, -1 for an event that is no observation and for an observation whose landmark was cut
 *   off.
 *   Per landmark with n observations, c0 the centre of its first:
 *     1. A = sum (I - u_i u_i^T), b = sum (I - u_i u_i^T)(c_i - c0), X = c0 + A^-1 b by a 3x3 Cholesky (l00 = sqrt(a00),
 *        l10 = a01 / l00, l20 = a02 / l00, p1 = a11 - l10^2, l11 = sqrt(p1), l21 = (a12 - l20 l10) / l11, p2 = (a22 - l20^2) -
 *        l21^2, l22 = sqrt(p2); forward, then back substitution).  It FAILS when a pivot a00, p1, p2 is <= 0 or not finite.
 *     2. exactly `refine` (0 .. 4) Gauss-Newton steps, no trip count depends on the data: Y_i = R_i^T (X - c_i),
 *        r_i = (fx (Y.x / Y.z) + cx - x_i, fy (Y.y / Y.z) + cy - y_i), J_i = dr_i / dX, H = sum J^T J, g = sum J^T r,
 *        X <- X - H^-1 g (the same Cholesky).  A step whose factorisation fails or whose result is not finite keeps X.
 *     3. a last pass at the final X: H, rms = sqrt(sum |r_i|^2 / n), ev_residual[i] = r_i, cov = sigma_px^2 H^-1 stored xx, xy,
 *        xz, yy, yz, zz (the order of ramp_ba_map_covariance's point_cov).
 *     4. parallax = max_i acos(clamp((u_i.x u_1.x + u_i.y u_1.y) + u_i.z u_1.z, -1, 1)) in radians, u_1 the first observation's.
 *     5. span = (t_first, t_last).
 *   cls is the first that applies: 1 n < min_obs; 2 parallax < min_parallax; 3 the Cholesky of step 1 failed; 4 some Y_i.z <=
 *   RAMP_WARP_MIN_Z (or NaN) at the final X; 5 rms > max_rms; 6 a word of point or cov, as stored, is not finite; 7 valid.
 *   point [.][3] and cov [.][6] fp32 are NaN unless cls is 7 -- never a plausible number, so ramp_point_map_insert(point, count)
 *   drops every landmark that is not valid by itself.  n_obs int32, parallax fp32 and span [.][2] float64 are written for every
 *   landmark; rms fp32 and the landmark's rows of ev_residual are NaN when step 1 failed, else what step 3 gives whatever the
 *   class.  ev_residual [N][2] is NaN for every event that is not an observation of a landmark kept, ev_ray [N][6] for every
 *   event that is not an observation.  ev_landmark, ev_residual, ev_ray: optional, NULL.
 *   status: device int32 [8]: [0] bit 0 RAMP_INTERP_BAD_TIMES (the knots' time stamps decrease or are not finite), [1] events
 *   without a track, [2] not finite, [3] outside the knots' range, [4] observations, [5] tracks seen, [6] tracks cut off,
 *   [7] valid landmarks; [1] + [2] + [3] + [4] = N.  RAMP_INTERP_BAD_TIMES is an outcome of the data (RAMP_OK), never a
 *   plausible answer: count = 0, every ev_landmark is -1, ev_residual and ev_ray are NaN, [4] .. [7] are 0 ([1] .. [3] are
 *   still counted by the tests above, so the sum is then short of N).
 *   Launches, all on `stream`, nothing synchronised; the host never learns the observation count or the landmark count, every
 *   loop is a bounded search, of fixed length or strided over a device count: a memset; the key kernel ((ordered bits of t,
 *   index) and the segment table of ramp_se3_interp; an event that is no observation takes the all-ones key); a STABLE 64-bit
 *   radix sort by time (hipcub); the id gather; a stable 64-bit radix sort by id; head flags; one exclusive sum (landmark
 *   numbers, the landmarks' first positions, count); the ray kernel, one lane per SORTED position (segment search over the
 *   knot times, in LDS up to 4096 knots, else in global memory; the pose; (c, d, q, x, y) written contiguously per landmark);
 *   the solve kernel, one wave per landmark striding over count, lanes striding over the landmark's observations, every sum
 *   through a fixed butterfly, refine + 2 passes over the rays.  No floating-point atomics anywhere.  A call repeats its bits,
 *   and its landmarks -- every per-landmark output -- do not depend on the order of the events as long as no track holds two
 *   equal time stamps (the index then decides their order, and with it the order of the sums and which observation is first).
 *   Only the observations of this call are triangulated; nothing is carried from call to call.
 *   N == 0: RAMP_OK, no kernel is launched: count and status are zeroed.
 *   RAMP_EINVAL, touching nothing: N < 0, T < 1, unknown flags, min_obs < 2, refine outside 0 .. 4, min_parallax, max_rms or
 *   sigma_px negative or not finite, max_landmarks < 1, a NULL lm_track, point, cov, n_obs, cls, rms, parallax, span, count or
 *   status (N > 0: x, y, t, track, knots, times, intrinsics, ws), lm_track, span, t, track or times not 8-byte aligned, any
 *   other array not 4-byte aligned, ws not 16-byte aligned.  RAMP_EUNSUPPORTED: N >= 2^31.  RAMP_EWORKSPACE: ws_bytes below
 *   ramp_event_landmarks_ws_bytes(N, T, max_landmarks) (0 for sizes that are refused).
 * ramp_event_landmarks_grid_events(): the number of events one trip of the full grid covers; above it the workgroups take a
 * second trip.                                                                                                            */
size_t ramp_event_landmarks_ws_bytes(long N, int T, long max_landmarks);
long ramp_event_landmarks_grid_events(void);
int ramp_event_landmarks(const float *x, const float *y, const double *t, const int64_t *track, long N, const float *knots,
                         const double *times, int T, const float *intrinsics, int flags, int min_obs, int refine,
                         float min_parallax, float max_rms, float sigma_px, long max_landmarks, int64_t *lm_track, float *point,
                         float *cov, int32_t *n_obs, uint8_t *cls, float *rms, float *parallax, double *span, int32_t *count,
                         int32_t *ev_landmark, float *ev_residual, float *ev_ray, int32_t *status, void *ws, size_t ws_bytes,
                         void *stream);

/* ---------------------------------------------------------------- IMU: preintegration and alignment (csrc/imu.hip)
 *
 * A monocular trajectory has an arbitrary unit and no notion of down.  These entries take raw IMU samples and the trajectory as
 * it is (a ramp_trajectory_resolve / ramp_se3_interp row per knot) and return the gyro bias, the metric scale, gravity in the
 * tracker's world frame and a velocity per knot.  The tracker's step, its bundle adjustment and every other kernel are untouched.
 *   Inputs.  tau [N] float64 sample times; gyro, accel [N][3] float, or float64 with RAMP_IMU_F64 (rad/s, m/s^2: the
 *   accelerometer measures R^T (a - g)).  knots [T][7] fp32 camera-to-world (tx ty tz qx qy qz qw); the quaternion is taken to
 *   float64 and normalised there.  times [T] float64, in the unit of tau.  stride >= 1: the knots used are 0, stride,
 *   2 stride, ..., K = (T - 1) / stride + 1 of them.  extrinsics: HOST float64 [12], R_bc [3][3] row-major then p_bc [3], the
 *   camera in the IMU (body) frame; NULL: identity.  R_bc has to be a rotation -- every word of R R^T - I within
 *   RAMP_IMU_ROTATION_TOL and det R > 0, else RAMP_EINVAL, never a plausible answer from a matrix that is none -- and is
 *   converted to a unit quaternion on the host.  bias_g, bias_a: HOST float64 [3] or NULL for zero.  max_gap: seconds, > 0, infinity allowed.  gravity_norm: 0 = free, else the known norm G.
 *   One interval [T_k, T_k+1] of consecutive used knots.  Its breakpoints u_0 .. u_m are T_k, the samples with
 *   T_k < tau_i < T_k+1, then T_k+1: a sample equal to an end is not repeated, duplicated tau give sub-intervals of length 0,
 *   which are identities.  The measurement is piecewise linear between samples (at a sample's own time: that sample).  On a
 *   sub-interval of length dt, w = 1/2 (gyro(u_j) + gyro(u_j+1)) - bias_g, a likewise with bias_a, and its element is
 *     e = (E, dv, dp, dt, J) = (Exp(w dt), a dt, (a dt)(dt / 2), dt, -Jr(w dt) dt)
 *   with Exp as a unit quaternion and Jr = I - b [phi]x + c [phi]x^2, b = (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2,
 *   c = (th - sin th) / th^3; below th^2 = 1e-4 all four coefficients are their Taylor series to th^8 (no cancellation, no
 *   sin / cos call).  Elements compose in order with the associative law
 *     (R1,v1,p1,t1,J1) o (R2,v2,p2,t2,J2) = (R1 R2,  v1 + R1 v2,  (p1 + v1 t2) + R1 p2,  t1 + t2,  R2^T J1 + J2)
 *   and the product over the interval is (dR, dv, dp, dt, J_Rg): Forster's on-manifold preintegral with d dR / d bias_g.  All
 *   of it is float64 without FMA contraction.  The quaternion product is not renormalised on the way; the record's is
 *   normalised once and given qw >= 0.
 *   preint [K - 1][RAMP_IMU_PREINT_WORDS] float64: [0] dt (the composed sum), [1] the sub-interval count m, [2..5] dR as
 *   qx qy qz qw, [6..8] dv, [9..11] dp, [12..20] J_Rg row-major, [21..23] 0.
 *   Covered.  An interval is covered when tau_0 <= T_k and T_k+1 <= tau_N-1, every sample it touches (from the last one at or
 *   before T_k to the first one at or after T_k+1) is finite, no two consecutive touched samples are further apart than
 *   max_gap, and T_k+1 > T_k.  Anything else is counted and its record is NaN in all 24 words.
 *   Kernel.  One wave per interval: two binary searches in tau, then the sub-intervals in chunks of 64, one per lane; a chunk is
 *   reduced by an ORDERED shuffle tree (offsets 1, 2, 4, ...: lane i takes own o lane(i + off); lanes beyond the tail hold the
 *   identity, which is neutral to the bit on either side) and chunks chain left to right in lane 0.  A record's bits are a
 *   function of its own interval's samples and the biases alone -- not of K, stride or its position -- and a call repeats its
 *   bits.  An interval with 10^6 samples costs one wave's walk: accepted, a VO interval holds tens of samples.
 *   status: device int32 [8]: [0] bits, [1] samples, [2] intervals, [3] intervals not covered (range, gap, not finite),
 *   [4] intervals with T_k+1 <= T_k, [5] intervals in the (first) gyro step, [6] triples used, [7] 0.  [3] + [4] + covered = [2].
 *   RAMP_IMU_BAD_ORDER: tau or times (all T) decrease or are not finite; no interval is walked, all count in [3], every output
 *   is NaN.  A gyro bias that is not finite -- what a failed gyro step leaves -- is treated alike: the integration behind it
 *   walks nothing, every interval counts in [3] and every record is NaN, so [6] is 0 and the scale stage ends in
 *   RAMP_IMU_FEW_TRIPLES.
 * ramp_imu_preintegrate: one 32-byte hipMemsetAsync of status, the check kernel, the integration.  [5], [6] stay 0.
 * ramp_imu_align: with R_wb = R_wc R_bc^T, c_k = R_wc,k (-R_bc^T p_bc), pbar the knots' translations, p_wb = s pbar + c:
 *   Gyro bias, gyro_steps (1 .. RAMP_IMU_MAX_GYRO_STEPS) Gauss-Newton steps, re-integrating in front of each: over the covered
 *     intervals r_k = Log(dR_k^T R_wb,k^T R_wb,k+1), H = sum J^T J, b = sum J^T r, delta = H^-1 b (3 x 3 Cholesky),
 *     bias_g += delta.  Fewer than one covered interval, a pivot that is not positive and finite or a result that is not
 *     finite: RAMP_IMU_GYRO_FAILED, the bias NaN (and with it everything behind).
 *   Scale and gravity: the integration is run AGAIN with the corrected bias -- the records carry no Jacobians of dv and dp with
 *     respect to the biases, a deliberate simplification: the integration is cheap here.  Every pair of consecutive covered
 *     intervals 1 = (k, k+1), 2 = (k+1, k+2) gives three rows in x = (s, g), the velocities eliminated:
 *       s [(p3 - p2) / dt2 - (p2 - p1) / dt1] - 1/2 (dt1 + dt2) g
 *           = (((R2 dp2 / dt2 - R1 dp1 / dt1) + R1 dv1) - (c3 - c2) / dt2) + (c2 - c1) / dt1          (p = pbar, R = R_wb)
 *     N = sum A^T A [4][4], y = sum A^T rhs [4]: per-workgroup partials of 256 triples (wave butterflies, the four waves in
 *     order), then one wave over the partials in index order: an order fixed by K alone.  One lane solves by Cholesky.
 *     RAMP_IMU_SCALE_FAILED with RAMP_IMU_FEW_TRIPLES (fewer than two triples), RAMP_IMU_SINGULAR (a pivot that is not positive
 *     and finite, sums or a solution that are not finite) or RAMP_IMU_BAD_SCALE (s <= 0); bias_g1 stays valid.
 *   Known norm G > 0: exactly four tangent refinements from N and y alone, no second pass over the data: with gh = g / |g|,
 *     b1 = normalise(gh x e), e the axis of the smallest |gh| component (the first on ties), b2 = gh x b1, x0 = (0, G gh),
 *     P = [e_s, (0, b1), (0, b2)]:  (P^T N P) z = P^T (y - N x0),  g = G gh + z1 b1 + z2 b2,  gh = g / |g|,  x = (z0, G gh).
 *   Velocities [K][3]: v_k = (((p_k+1 - p_k) - 1/2 g dt^2) - R_k dp) / dt with p = s pbar + c; the last knot takes
 *     v + g dt + R dv of the last interval; NaN beside an interval that is not covered.
 *   residual [K - 2]: |A x - rhs| per triple (NaN for a triple not used);  rms = sqrt(sum residual^2 / triples).
 *   The accelerometer bias is an input and is not estimated.
 *   Outputs, all on the device:  result float64 [16]: [0] s, [1..3] g, [4..6] bias_g1, [7] rms, [8] the largest over the
 *   smallest pivot d_j = L_jj^2 of the 4 x 4 factorisation (a cheap estimate of the condition number), [9..15] 0;
 *   normal float64 [32]: N [16], y [4], the last gyro step's H [9], b [3];  velocity, residual;  preint (optional, NULL): the
 *   records of the final integration;  status.  With RAMP_IMU_SCALE_FAILED s, g, rms, [8], velocity and residual are NaN.
 *   Launches, all on `stream`, nothing read back, nothing synchronised, no floating-point atomics: one hipMemsetAsync, the check,
 *   (integrate, gyro partials, gyro final) x gyro_steps, integrate, scale partials (K > 2), scale final, and one workgroup for
 *   velocities, residuals, rms and the status words.  ws: ramp_imu_workspace_bytes(N, K) bytes, 16-byte aligned.
 *   Outcomes of the data return RAMP_OK.  NULL inputs or outputs (residual may be NULL with K == 2), N < 1 or >= 2^31, T < 2,
 *   stride < 1 or K < 2, unknown flags, max_gap not > 0, gravity_norm negative or not finite, a bias or extrinsic that is not
 *   finite, an R_bc that is no rotation, gyro_steps outside its range, float64 arrays not 8-byte (fp32 samples: 4-byte) aligned, ws not 16-byte aligned:
 *   RAMP_EINVAL; a short workspace: RAMP_EWORKSPACE.                                                                   */
#define RAMP_IMU_F64 1
#define RAMP_IMU_PREINT_WORDS 24
#define RAMP_IMU_MAX_GYRO_STEPS 16
#define RAMP_IMU_ROTATION_TOL 1e-6
#define RAMP_IMU_BAD_ORDER 1    /* status[0] bit 0 */
#define RAMP_IMU_GYRO_FAILED 2  /* bit 1 */
#define RAMP_IMU_SCALE_FAILED 4 /* bit 2, with one of the three below */
#define RAMP_IMU_FEW_TRIPLES 8
#define RAMP_IMU_SINGULAR 16
#define RAMP_IMU_BAD_SCALE 32
size_t ramp_imu_workspace_bytes(long N, int K);
int ramp_imu_preintegrate(const double *tau, const void *gyro, const void *accel, long N, const double *times, int T, int stride,
                          const double *bias_g, const double *bias_a, double max_gap, int flags, double *preint,
                          int32_t *status, void *stream);
int ramp_imu_align(const double *tau, const void *gyro, const void *accel, long N, const float *knots, const double *times, int T,
                   int stride, const double *extrinsics, const double *bias_g, const double *bias_a, double max_gap,
                   double gravity_norm, int gyro_steps, int flags, double *result, double *normal, double *velocity,
                   double *residual, double *preint, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- IMU propagation (csrc/imu_propagate.hip)
 *
 * Poses at the sample rate ahead of a knot: from an anchor -- a knot's pose and what ramp_imu_align found for it -- forward
 * through every sample behind it, one row per sample.  Nothing of the entries above changes.
 *   Inputs.  tau, gyro, accel, N, flags (RAMP_IMU_F64), extrinsics (HOST [12], NULL: identity; the rotation test), bias_a (HOST
 *   [3] or NULL) and max_gap as in ramp_imu_align.  horizon: seconds, > 0, infinity allowed.  anchor: DEVICE float64
 *   [RAMP_IMU_ANCHOR_WORDS]; the host never reads it:  [0] t0;  [1..3] pbar0, the knot's translation in the tracker's unit;
 *   [4..7] the knot's quaternion xyzw, camera to world, normalised here in float64;  [8..10] v0, metric, world frame (the
 *   knot's row of `velocity`);  [11] s;  [12..14] g;  [15..17] bias_g;  [18..23] 0.
 *   Definition, float64 without FMA contraction, the element and the law of the section above word for word (J is not carried:
 *   11 words).  u_i = max(tau_i, t0).  The measurement is piecewise linear between samples; at t0 it is interpolated between
 *   the last sample at or before t0 and the next, exactly as an interval's first sub-interval is formed above (a sample on t0
 *   is used as it is).  e_i (i >= 1) is the element on [u_i-1, u_i] with w = 1/2 (gyro(u_i-1) + gyro(u_i)) - bias_g, a likewise
 *   with bias_a; a sub-interval of length 0 is the identity.  P_0 is the identity, P_i = e_1 o ... o e_i = (dR, dv, dp, dt).
 *   With R0 = R_wc0 R_bc^T and p0 = s pbar0 - R0 p_bc, row i is
 *     R_wb = R0 dR        v = (v0 + g dt) + R0 dv        p_wb = ((p0 + v0 dt) + 1/2 g dt^2) + R0 dp
 *   Outputs, all on the device; times_out and state may be NULL.
 *   state [N][16] float64: [0] dt, [1..4] q_wb (normalised once, its sign as it comes), [5..7] v, [8..10] p_wb, [11..15] 0.
 *   poses [N][7] fp32, camera to world in the tracker's unit, a ramp_trajectory_resolve row in every respect: translation
 *   (p_wb + R_wb p_bc) / s, rotation q_wb (x) q_bc normalised in float64, each rounded to fp32 once.
 *   times_out [N] = u_i: with poses the `knots, times` of ramp_se3_interp / ramp_event_warp.  Rows at or before the anchor hold
 *   the anchor's pose at time t0; equal time stamps do not decrease, which those entries accept.
 *   status: device int32 [8]: [0] bits, [1] samples, [2] rows held (tau_i <= t0), [3] rows propagated, [4] rows cut off,
 *   [5] rows beyond the horizon, [6], [7] 0;  [2] + [3] + [4] + [5] = [1] whenever no bit is set.
 *   Bits: RAMP_IMU_BAD_ORDER (tau decreases or is not finite), RAMP_IMU_BAD_ANCHOR (a word of anchor[0..17] is not finite, or
 *   s <= 0), RAMP_IMU_NO_START (tau[0] > t0).  Any bit: every word of poses, state and times_out is NaN, nothing is walked.
 *   Dead reckoning does not bridge a break: with b the first index with u_b > t0 at which sample b or sample b - 1 is not finite
 *   or tau_b - tau_b-1 > max_gap, every row >= b is NaN in poses and state and counts in [4]; its times_out stays u_i.  Samples
 *   that are not finite strictly before the last one at or before t0 are never touched.  A row with dt > horizon is NaN and
 *   counts in [5] (behind [4]).  These are outcomes of the data and return RAMP_OK.
 *   Kernel: a three-level ORDERED scan of the non-commutative product, aligned to sample 0.  A chunk is 64 samples, one per
 *   lane: lane i takes lane(i - off) o own for off = 1, 2, 4, ..., 32, the lanes before the head supplying the identity, which
 *   is neutral to the bit.  A tile is 64 chunks (4,096 samples, one workgroup); its chunk totals are scanned the same way.  The
 *   tile totals chain left to right in one wave.  Row i = (chain[tile - 1] o chunks of its tile before its own) o its chunk's
 *   scan: its bits are a function of samples 0 .. i and the arguments -- not of N, the grid or the samples behind it -- and a
 *   call repeats its bits.  The elements are recomputed in the output pass, not stored.  No floating-point atomics: b is an
 *   integer atomicMin, the counters are ballots.  One 64-byte hipMemsetAsync and five launches (check, tiles, chain, rows,
 *   status) on `stream`; nothing read back, nothing synchronised.  ws: ramp_imu_propagate_workspace_bytes(N) bytes (64 and 11
 *   doubles per chunk and per tile; 0 for N < 1), 16-byte aligned.
 *   NULL tau, gyro, accel, anchor, poses, status or ws, N < 1 or >= 2^31, unknown flags, max_gap or horizon not > 0, a bias or
 *   extrinsic that is not finite, an R_bc that is no rotation, misaligned arrays: RAMP_EINVAL; a short workspace:
 *   RAMP_EWORKSPACE.  A refusal touches nothing.                                                                          */
#define RAMP_IMU_ANCHOR_WORDS 24
#define RAMP_IMU_BAD_ANCHOR 64  /* status[0] bit 6 */
#define RAMP_IMU_NO_START 128   /* bit 7 */
size_t ramp_imu_propagate_workspace_bytes(long N);
int ramp_imu_propagate(const double *tau, const void *gyro, const void *accel, long N, const double *anchor,
                       const double *extrinsics, const double *bias_a, double max_gap, double horizon, int flags, float *poses,
                       double *times_out, double *state, int32_t *status, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RAMP_HIP_H */
