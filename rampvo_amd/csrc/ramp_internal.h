// internal (non-exported) helpers shared between translation units
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/ramp_hip.h"
#include "update_params.h"
#include "workspace.h"

size_t ramp_internal_group_by_ws(int E);
int ramp_internal_group_by(const int64_t *keys, int E, int64_t key_bound, int32_t *order,
                           int32_t *gid, int32_t *seg_start, int64_t *ukeys, int32_t *ngroups,
                           void *ws, size_t ws_bytes, hipStream_t st);

// ---- launchers with device-side sizes (the RAMP_DYN_* block of include/ramp_hip.h), used by csrc/track.hip: the
// integer size argument is the launch bound, the live count is read by the kernel from `dyn`
int ramp_i_transform_dyn(const float *poses, const float *patches, const float *intrinsics, const int64_t *ii,
                         const int64_t *jj, const int64_t *kk, float *out, int E_cap, const int32_t *dyn,
                         hipStream_t st);
int ramp_i_point_cloud_dyn(const float *poses, const float *patches, const float *intrinsics, const int64_t *ix,
                           float *out, int m_cap, const int32_t *dyn, int M, hipStream_t st);
int ramp_i_motionmag_point_cloud_dyn(const float *poses, const float *patches, const float *intrinsics, const int64_t *ii,
                                     const int64_t *jj, const int64_t *kk, const int32_t *order, const int32_t *seg,
                                     const int64_t *ukeys, const int32_t *ngroups, float beta, float *out2,
                                     int32_t *dyn, int keyframe_index, const int64_t *ix, float *points, int m_cap,
                                     int M, float *median, hipStream_t st);
int ramp_i_motionmag_dyn(const float *poses, const float *patches, const float *intrinsics, const int64_t *ii,
                         const int64_t *jj, const int64_t *kk, const int32_t *order, const int32_t *seg,
                         const int64_t *ukeys, const int32_t *ngroups, float beta, float *out2, const int32_t *dyn,
                         int keyframe_index, hipStream_t st);
int ramp_i_frame_commit_dyn(float *poses, int motion, float damping, int64_t *tstamps, int64_t counter,
                            int64_t *index_map, float *intrinsics, const float *k_new, float *patches_state,
                            int median_frames, int M, int P, float *patches_new, int n_copy, const void *const *src,
                            void *const *base, const long *bytes, const int *mod, const int32_t *dyn,
                            const float *median_ahead, int32_t *status, int E_bound, int n_rows, hipStream_t st,
                            const int32_t *slot_tab = nullptr, int slot_buf = 0, uint32_t *signal = nullptr,
                            uint32_t signal_val = 0);
size_t ramp_i_plan_dyn_ws(int E_cap, int kkey_cap, int pkey_cap);
int ramp_i_plan_dyn(const int64_t *g4, int E_cap, int E_grid, const int32_t *dyn, int32_t *status, int M, int kkey_cap,
                    int pkey_cap, int kk_cap, int ij_cap, int32_t *kk_order, int32_t *kk_gid, int32_t *kk_seg,
                    int32_t *kk_ngroups, int64_t *kk_ukeys, int32_t *ij_order, int32_t *ij_gid, int32_t *ij_seg,
                    int32_t *ij_ngroups, int64_t *ij_ukeys, int64_t *ix, int64_t *jx, int32_t *kj, void *ws,
                    size_t ws_bytes, int32_t *mirror, hipStream_t st);
// the segment launch of the event warp (csrc/warp.hip), shared with the event contrast (csrc/contrast.hip): the segment table
// into seg, C(t_ref)^-1 into ref (WARP_REF_WORDS floats), RAMP_INTERP_BAD_TIMES into ctr[0]
int ramp_i_warp_segments(const float *knots, const double *times, int T, double t_ref, int extrapolate, float *seg, float *ref,
                         int32_t *ctr, hipStream_t st);
// bundle adjustment (csrc/ba.hip): the state and the graph of one problem
struct BaProblem {
  float *poses, *patches;                                  // [n_poses][7], [n_patches][3][P][P]
  const float *intrinsics, *target, *weight, *lmbda;       // target / weight [E][2]
  const int64_t *ii, *jj, *kk;                             // [E]
  int E, P, n_poses, n_patches;
  int t0, t1;                                              // the free poses [t0, t1)
  const int32_t *dyn;                                      // device-side sizes (nullptr: none), the window is then the
  int opt_window;                                          // last opt_window poses and t0 / t1 are ramp_i_ba_*dyn's to set
};
// its factors grouped by patch (kk) and by pose pair (jj * n_poses + ii), and the caller's bounds on the group counts
struct BaGroups {
  const int32_t *order_k, *seg_k, *ngroups_k;
  const int64_t *ukeys_k;
  const int32_t *order_p, *seg_p, *ngroups_p;
  int max_patches, max_pairs;
};
size_t ramp_i_ba_dyn_ws(int E_cap, int n_poses, int n_patches, int opt_window, int max_patches, int max_pairs);
int ramp_i_ba_dyn(const BaProblem &p, const BaGroups &g, int iterations, void *ws, size_t ws_bytes, int32_t *info,
                  hipStream_t st);
// the map's outputs of a covariance call (include/ramp_hip.h ramp_ba_map_covariance), indexed by patch id; all four or none
struct BaMapOut {
  float *point, *point_cov, *pose_depth_cov;               // [n_patches][3], [n_patches][6], [n_patches][6]
  int32_t *n_obs;                                          // [n_patches]
};
size_t ramp_i_ba_cov_dyn_ws(int opt_window, int max_patches);
// map: nullptr = the covariance alone
int ramp_i_ba_cov_dyn(const BaProblem &p, const BaGroups &g, void *ba_ws, size_t ba_ws_bytes, void *cov_ws,
                      size_t cov_ws_bytes, int32_t *info, float *cov, float *depth_var, float *stats, hipStream_t st,
                      const BaMapOut *map = nullptr);
// one call of the update operator (csrc/update_op.hip): ramp_update_args plus what only the device-resident step has
struct UpdOp {
  ramp_update_args a;
  const int32_t *dyn;          // device-side sizes (nullptr: a.E rows are live), a.E is then the launch bound
  void *gate_event;            // fp16 features: "the next frame's front end may start", in front of the first SoftAgg -- an
  uint32_t *gate_flag;         // event recorded there, or (gate_flag) the word gate_seq that launch's first workgroup stores
  uint32_t gate_seq;
};
int ramp_i_update_check(const UpdOp &op);                      // RAMP_EINVAL unless every pointer the precision needs is there
int ramp_i_update_operator(const UpdOp &op, hipStream_t st);   // (a checked op)
// its stages (csrc/update_mlp.hip, csrc/update_x3.hip): one operand record each (update_params.h), which the launcher
// validates -- RAMP_EINVAL for E < 0, RAMP_OK for E = 0 before any pointer is looked at.  E_hint: ramp_track.E_hint
int ramp_i_upd_corr_mlp(const CorrTailParams &p, hipStream_t st);
int ramp_i_upd_nbr(const NbrParams &p, hipStream_t st);
int ramp_i_upd_softagg(const SoftAggParams &p, hipStream_t st);
int ramp_i_upd_gru(const GruParams &p, int E_hint, hipStream_t st);
int ramp_i_x3_corr_mlp(const X3CorrMlpParams &p, hipStream_t st);
int ramp_i_x3_nbr(const X3NbrParams &p, hipStream_t st);
int ramp_i_x3_fg(const X3FgParams &p, hipStream_t st);
int ramp_i_x3_gru(const X3GruParams &p, hipStream_t st);
extern "C" {
int ramp_i_corr_fwd(const void *fmap1, const ramp_corr_level *levels, int nlevels, const float *coords,
                    const int64_t *ii, const int64_t *jj, const int32_t *order, void *out, int out_row_elems,
                    long mod_ii, long mod_jj, int E, int N1, int N2, int C, int P, int radius, int dtype, int layout,
                    const int32_t *dyn, void *stream, const float *tf_poses = nullptr, const float *tf_patches = nullptr,
                    const float *tf_intr = nullptr, const int64_t *tf_src = nullptr, const int32_t *slot0 = nullptr);
}
