// Live poses without leaving the device-resident step (include/ramp_hip.h, "live poses").
//
//   * trk_publish_kernel: one wave per accepted frame writes a 128-byte pose record -- frame tag, time stamp, the newest
//     frame's pose and its inverse, the sizes, the keyframe test's outcome -- into a ring in pinned host memory.  The host
//     reads the ring without a HIP call (track_dev.PoseRing); nothing is handed back, nothing synchronises.
//   * traj_resolve_kernel: Ramp_vo.terminate()'s interpolation of the dropped frames' poses (the recursion of get_pose
//     along the delta chain, one ramp_se3_mul launch per link on the host) as ONE launch, reading the device-side delta log
//     and keyframe rows where they are.
#include "ramp_device.h"
#include "ramp_internal.h"

// One lane per word of the record: lanes 0 .. 15 store the first 64-byte half (tag, sizes, time stamp), then a system-scope
// fence, then lanes 16 .. 31 store the second half (pose, inverse, the tag again) -- two full 64-byte writes, in order.
// Every lane loads the seven pose floats (one broadcast load each) and forms the inverse itself; 32 copies of ~40 flops
// are cheaper than a cross-lane exchange.
__global__ void __launch_bounds__(64) trk_publish_kernel(const int32_t *__restrict__ dyn, const float *__restrict__ poses,
                                                         const int64_t *__restrict__ tstamps, const float *__restrict__ dlog,
                                                         int log_cap, int n_rows, int counter, double tstamp, int n, int row,
                                                         int E, int status, int dropped, int t1, int t0,
                                                         volatile int32_t *__restrict__ slot) {
  const int w = threadIdx.x;
  if (w >= RAMP_POSE_WORDS) return;
  if (dyn) {
    n = dyn[RAMP_DYN_NPREV];
    row = dyn[RAMP_DYN_NROW] - 1;
    E = dyn[RAMP_DYN_EKEPT];
    status = dyn[RAMP_DYN_STATUS];
    dropped = dyn[RAMP_DYN_REMOVED] != 0;
    t1 = t0 = -1;
    const int nlog = dyn[RAMP_DYN_NLOG];
    // (status bit 16: the log was full and this test's entry was not written -- the last entry is an older one)
    if (dropped && !(status & 16) && nlog >= 1 && nlog <= log_cap) {
      const float *e = dlog + (size_t)(nlog - 1) * RAMP_TRACK_LOG;
      t1 = __float_as_int(e[0]);
      t0 = __float_as_int(e[1]);
    }
  }
  row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);
  float P[7], Pi[7];
#pragma unroll
  for (int q = 0; q < 7; q++) P[q] = poses[7 * (size_t)row + q];
  lt_inv(P, Pi);
  int32_t v = 0;
  switch (w) {
    case RAMP_POSE_FRAME: case RAMP_POSE_FRAME2: v = counter; break;
    case RAMP_POSE_N: v = n; break;
    case RAMP_POSE_E: v = E; break;
    case RAMP_POSE_STATUS: v = status; break;
    case RAMP_POSE_DROPPED: v = dropped ? 1 : 0; break;
    case RAMP_POSE_T1: v = t1; break;
    case RAMP_POSE_T0: v = t0; break;
    case RAMP_POSE_KF_TSTAMP: v = (int32_t)tstamps[row]; break;
    case RAMP_POSE_TSTAMP: v = __double2loint(tstamp); break;
    case RAMP_POSE_TSTAMP + 1: v = __double2hiint(tstamp); break;
    default: break;
  }
#pragma unroll
  for (int q = 0; q < 7; q++) {
    if (w == RAMP_POSE_POSE + q) v = __float_as_int(P[q]);
    if (w == RAMP_POSE_INV + q) v = __float_as_int(Pi[q]);
  }
  if (w < RAMP_POSE_WORDS / 2) slot[w] = v;
  __threadfence_system();
  if (w >= RAMP_POSE_WORDS / 2) slot[w] = v;
}

// ---------------------------------------------------------------------------------------------- trajectory
// One workgroup.  ws: link [T] (the log entry that names frame t as its t1, -1: none), kf [T] (the keyframe row whose time
// stamp is t, -1: none), done [T] (0: open, r: resolved in round r).  `out` holds the frames' world -> camera poses while
// the chains are resolved and is inverted in place at the end.
// Association order: get_pose(t) = dP_t * get_pose(t0), so a frame is resolved from its FINISHED t0 -- one lt_mul per link,
// innermost product first.  Round r resolves the frames whose t0 was resolved in a round before r (the barrier between two
// rounds orders the rows); chains of depth d take d rounds.  No pointer jumping: (dP_t * dP_t0) * X rounds differently.
#define TRAJ_THREADS 256
__device__ __forceinline__ const float *traj_entry(const float *extra, int n_extra, const float *dlog, int e) {
  return e < n_extra ? extra + (size_t)e * RAMP_TRACK_LOG : dlog + (size_t)(e - n_extra) * RAMP_TRACK_LOG;
}
__global__ void __launch_bounds__(TRAJ_THREADS)
    traj_resolve_kernel(const float *__restrict__ kf_poses, const int64_t *__restrict__ kf_tstamps, int n,
                        const int32_t *__restrict__ dyn, const float *__restrict__ dlog, int nlog,
                        const float *__restrict__ extra, int n_extra, int T, float *out, int32_t *ws, int32_t *status) {
  const int tid = threadIdx.x;
  int32_t *link = ws, *kf = ws + T, *done = ws + 2 * (size_t)T;
  if (dyn) {                                     // (the arguments are the capacities)
    const int nd = dyn[RAMP_DYN_NROW], ld = dyn[RAMP_DYN_NLOG];
    n = nd < 0 ? 0 : (nd < n ? nd : n);
    nlog = ld < 0 ? 0 : (ld < nlog ? ld : nlog);
  }
  if (tid == 0) *status = 0;
  for (int t = tid; t < T; t += TRAJ_THREADS) { link[t] = -1; kf[t] = -1; done[t] = 0; }
  __syncthreads();
  // (a frame named twice: the later entry / the higher row, as the host's dict assignments)
  for (int e = tid; e < n_extra + nlog; e += TRAJ_THREADS) {
    const int t1 = __float_as_int(traj_entry(extra, n_extra, dlog, e)[0]);
    if (t1 >= 0 && t1 < T) atomicMax(link + t1, e);
  }
  for (int i = tid; i < n; i += TRAJ_THREADS) {
    const int64_t ts = kf_tstamps[i];
    if (ts >= 0 && ts < T) atomicMax(kf + ts, i);
  }
  __syncthreads();
  for (int t = tid; t < T; t += TRAJ_THREADS) {
    const int i = kf[t];
    if (i < 0) continue;
#pragma unroll
    for (int q = 0; q < 7; q++) out[7 * (size_t)t + q] = kf_poses[7 * (size_t)i + q];
    done[t] = 1;
  }
  for (int round = 2; round <= T + 1; round++) {
    __syncthreads();
    int progress = 0;
    for (int t = tid; t < T; t += TRAJ_THREADS) {
      if (done[t] || link[t] < 0) continue;
      const float *e = traj_entry(extra, n_extra, dlog, link[t]);
      const int t0 = __float_as_int(e[1]);
      if (t0 < 0 || t0 >= T || t0 == t) continue;
      const int d0 = done[t0];
      if (d0 == 0 || d0 >= round) continue;        // (not before this round's barrier: its row may be half written)
      float dP[7], X[7], Z[7];
#pragma unroll
      for (int q = 0; q < 7; q++) { dP[q] = e[2 + q]; X[q] = out[7 * (size_t)t0 + q]; }
      lt_mul(dP, X, Z);
#pragma unroll
      for (int q = 0; q < 7; q++) out[7 * (size_t)t + q] = Z[q];
      done[t] = round;
      progress = 1;
    }
    if (!__syncthreads_or(progress)) break;
  }
  __syncthreads();
  int bad = 0;
  for (int t = tid; t < T; t += TRAJ_THREADS) {
    float X[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Y[7];
    if (done[t]) {
#pragma unroll
      for (int q = 0; q < 7; q++) X[q] = out[7 * (size_t)t + q];
      lt_inv(X, Y);
    } else {
      bad = 1;
#pragma unroll
      for (int q = 0; q < 7; q++) Y[q] = X[q];
    }
#pragma unroll
    for (int q = 0; q < 7; q++) out[7 * (size_t)t + q] = Y[q];
  }
  if (bad) atomicOr(status, RAMP_TRAJ_UNRESOLVED);
}

extern "C" {

int ramp_track_publish(const ramp_track *t, int64_t counter, double tstamp, float *ring_dev, int ring_cap,
                       const float *poses, const int64_t *tstamps, int n_rows, int n_imm, int row_imm, int E_imm,
                       int status_imm, int dropped_imm, int t1_imm, int t0_imm, void *stream) {
  if (!ring_dev || ring_cap <= 0 || counter < 0 || counter > 0x7fffffffLL) return RAMP_EINVAL;
  const int32_t *dyn = nullptr;
  const float *dlog = nullptr;
  int log_cap = 0;
  if (t) {
    if (!t->dyn || !t->poses || !t->tstamps || !t->dlog || t->n_rows <= 0) return RAMP_EINVAL;
    dyn = t->dyn; dlog = t->dlog; log_cap = t->log_cap; poses = t->poses; tstamps = t->tstamps; n_rows = t->n_rows;
  } else if (!poses || !tstamps || n_rows <= 0 || row_imm < 0 || row_imm >= n_rows) {
    return RAMP_EINVAL;
  }
  int32_t *slot = reinterpret_cast<int32_t *>(ring_dev) + (size_t)(counter % ring_cap) * RAMP_POSE_WORDS;
  hipLaunchKernelGGL(trk_publish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dyn, poses, tstamps, dlog, log_cap,
                     n_rows, (int)counter, tstamp, n_imm, row_imm, E_imm, status_imm, dropped_imm, t1_imm, t0_imm, slot);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

int ramp_trajectory_resolve(const float *kf_poses, const int64_t *kf_tstamps, int n, const int32_t *dyn, const float *dlog,
                            int nlog, const float *extra_log, int n_extra, int T, float *out, int32_t *ws, int32_t *status,
                            void *stream) {
  if (T < 0 || n < 0 || nlog < 0 || n_extra < 0) return RAMP_EINVAL;
  if (T == 0) return RAMP_OK;
  if (!out || !ws || !status || (n > 0 && (!kf_poses || !kf_tstamps)) || (nlog > 0 && !dlog) || (n_extra > 0 && !extra_log))
    return RAMP_EINVAL;
  if ((long)n_extra + nlog > 0x7fffffffL) return RAMP_EINVAL;
  hipLaunchKernelGGL(traj_resolve_kernel, dim3(1), dim3(TRAJ_THREADS), 0, (hipStream_t)stream, kf_poses, kf_tstamps, n, dyn,
                     dlog, nlog, extra_log, n_extra, T, out, ws, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

}  // extern "C"
