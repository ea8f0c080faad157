// Localisation against the event map (include/ramp_hip.h: ramp_point_map_localize_eval, ramp_point_map_localize): the voxels of
// evmap.hip's hash, projected with a pose estimate, sample a negative time surface (timesurface.hip); a Levenberg-Marquardt loop
// over the six pose parameters drives the samples down, entirely on the device.
//
// One evaluation is two launches:
//   loc_eval_kernel    one lane per SLOT in a grid-stride loop over the table where it lies (the grid is capped at
//                      LOC_MAX_GROUPS workgroups): the export's conditions and mean point and the renderer's projection
//                      (evmap_device.h: the same u, v in every bit), the bilinear sample and the interpolant's own derivative in
//                      fp32, the row of the Jacobian, the Huber weight and the 30 sums in float64; per lane, then the fixed
//                      butterfly ramp_wave_sum, then the waves in wave order: one row of 32 doubles per workgroup
//   loc_final_kernel   one wave: the rows in index order
// No floating-point atomics; for a given table and arguments a call repeats its bits.
// The loop (ramp_point_map_localize) puts localize_step_kernel, one wave, behind every evaluation: the state machine of the
// header, float64, + - * / and sqrt in a fixed order (every translation unit is compiled with -ffp-contract=off: nothing is
// fused).  A machine that has stopped sets the `done` word, and the launches behind it return at their first statement.
#include "evmap_device.h"

#define LOC_MAX_GROUPS 256                 // the grid's cap: the final kernel adds at most this many rows
#define LOC_WAVES (EVM_THREADS / RAMP_WAVE)
#define LOC_ROW 32                         // doubles per row: 21 + 6 + cost, in reach, participating, two spare
#define LOC_H 0
#define LOC_B 21
#define LOC_COST 27
#define LOC_REACH 28
#define LOC_PART 29

enum { LOC_ABSENT = 0, LOC_FILTERED, LOC_REJECTED, LOC_OUT, LOC_IN };

struct LocEval {
  const EvmSlot *slots;
  long capacity;
  double voxel;
  long long min_points;
  int min_views;
  const float *cam, *intrinsics, *surface;
  int H, W;
  double huber;
  float *records;
  double *rows;
  int32_t *status;
  const int32_t *done;
};

// rho and w of a residual r under the Huber threshold k (k <= 0: off); a NaN r gives a NaN rho and w = 1
static __device__ __forceinline__ void loc_huber(double r, double k, double *rho, double *w) {
  const double ar = fabs(r);
  if (k > 0.0 && ar > k) {
    *w = k / ar;
    *rho = (2.0 * k) * ar - k * k;
  } else {
    *w = 1.0;
    *rho = r * r;
  }
}

__global__ void __launch_bounds__(EVM_THREADS) loc_eval_kernel(const LocEval a) {
  __shared__ double s_red[LOC_WAVES * LOC_ROW];
  if (a.done && *a.done) return;                       // (uniform: a loop that has stopped)
  const int tid = threadIdx.x;
  float c[11];
  const bool failed = evm_load_camera(a.cam, a.intrinsics, c);
  if (blockIdx.x == 0 && tid == 0 && failed) a.status[0] = RAMP_MAP_LOCALIZE_BAD_CAMERA;
  const float nan = __int_as_float(0x7fc00000);
  double acc[LOC_PART + 1];
#pragma unroll
  for (int k = 0; k <= LOC_PART; k++) acc[k] = 0.0;
  int n_occ = 0, n_filt = 0, n_rej = 0, n_out = 0, n_in = 0;
  const double fx = (double)c[7], fy = (double)c[8];
  for (long base = (long)blockIdx.x * EVM_THREADS; base < a.capacity; base += (long)gridDim.x * EVM_THREADS) {
    const long i = base + tid;
    int kind = LOC_ABSENT;
    float u = nan, v = nan, r = nan, gu = nan, gv = nan, Xc[3] = {nan, nan, nan};
    if (i < a.capacity && !failed) {
      const EvmSlot *s = a.slots + i;
      const long long key = s->key, n = s->n;
      if (key != EVM_EMPTY) {
        if (!evm_slot_passes(key, n, s->views, a.min_points, a.min_views)) kind = LOC_FILTERED;
        else {
          float d;
          if (!evm_project(key, s->sq, n, c, a.voxel, Xc, &d, &u, &v)) {
            kind = LOC_REJECTED;
            u = v = nan;
          } else {
            // in reach: the four bilinear neighbours inside the image, tested in floating point before any conversion
            const float x0 = floorf(u), y0 = floorf(v);
            if (!((double)x0 >= 0.0 && (double)x0 < (double)(a.W - 1) && (double)y0 >= 0.0 && (double)y0 < (double)(a.H - 1))) kind = LOC_OUT;
            else {
              kind = LOC_IN;
              const float ax = u - x0, ay = v - y0;
              const float *p = a.surface + ((size_t)(long)y0 * a.W + (long)x0);
              const float s00 = p[0], s10 = p[1], s01 = p[a.W], s11 = p[a.W + 1];
              const float bx = 1.0f - ax, by = 1.0f - ay;
              r = by * (bx * s00 + ax * s10) + ay * (bx * s01 + ax * s11);
              gu = by * (s10 - s00) + ay * (s11 - s01);
              gv = bx * (s01 - s00) + ax * (s11 - s10);
            }
          }
        }
      }
      if (kind == LOC_IN) {
        const double X = (double)Xc[0], Y = (double)Xc[1], z = (double)Xc[2], rd = (double)r;
        const double gx = (double)gu * fx, gy = (double)gv * fy;
        double J[6], rho, w;
        J[0] = gx / z;
        J[1] = gy / z;
        J[2] = -(gx * X + gy * Y) / (z * z);
        J[3] = Y * J[2] - z * J[1];
        J[4] = z * J[0] - X * J[2];
        J[5] = X * J[1] - Y * J[0];
        loc_huber(rd, a.huber, &rho, &w);
        int at = 0;
#pragma unroll
        for (int p = 0; p < 6; p++) {
          const double wj = w * J[p];
#pragma unroll
          for (int q = p; q < 6; q++) acc[LOC_H + at++] += wj * J[q];
          acc[LOC_B + p] += wj * rd;
        }
        acc[LOC_COST] += rho;
        acc[LOC_REACH] += 1.0;
        acc[LOC_PART] += 1.0;
      } else if (kind == LOC_REJECTED || kind == LOC_OUT) {   // the surface's "no event" value, no derivative
        double rho, w;
        loc_huber(1.0, a.huber, &rho, &w);
        acc[LOC_COST] += rho;
        acc[LOC_PART] += 1.0;
      }
    }
    if (i < a.capacity && a.records) {
      float *rec = a.records + 8 * (size_t)i;
      const bool part = kind >= LOC_REJECTED;
      rec[0] = u; rec[1] = v; rec[2] = r; rec[3] = gu; rec[4] = gv;
      rec[5] = part ? Xc[0] : nan; rec[6] = part ? Xc[1] : nan; rec[7] = part ? Xc[2] : nan;
    }
    // the trip count aside, every lane of the wave is here
    n_occ += ramp_wave_count(kind != LOC_ABSENT);
    n_filt += ramp_wave_count(kind == LOC_FILTERED);
    n_rej += ramp_wave_count(kind == LOC_REJECTED);
    n_out += ramp_wave_count(kind == LOC_OUT);
    n_in += ramp_wave_count(kind == LOC_IN);
  }
  ramp_wave_flush(a.status + 1, tid, n_occ, n_filt, n_rej, n_out, n_in);
  // per wave by a fixed butterfly, then the waves in wave order
#pragma unroll
  for (int k = 0; k <= LOC_PART; k++) {
    const double v = ramp_wave_sum(acc[k]);
    if ((tid & (RAMP_WAVE - 1)) == 0) s_red[(tid / RAMP_WAVE) * LOC_ROW + k] = v;
  }
  __syncthreads();
  if (tid < LOC_ROW) {
    double v = 0.0;
    if (tid <= LOC_PART)
      for (int w = 0; w < LOC_WAVES; w++) v += s_red[w * LOC_ROW + tid];
    a.rows[(size_t)blockIdx.x * LOC_ROW + tid] = v;
  }
}

// one wave: the rows in index order
__global__ void __launch_bounds__(RAMP_WAVE)
    loc_final_kernel(const double *__restrict__ rows, int n_rows, const int32_t *__restrict__ status, double *__restrict__ sums,
                     const int32_t *__restrict__ done) {
  if (done && *done) return;
  const int tid = threadIdx.x;
  if (tid >= LOC_ROW) return;
  double v = 0.0;
  for (int r = 0; r < n_rows; r++) v += rows[(size_t)r * LOC_ROW + tid];
  const bool failed = (status[0] & RAMP_MAP_LOCALIZE_BAD_CAMERA) != 0;
  sums[tid] = failed ? __longlong_as_double(0x7ff8000000000000ll) : v;
}

static int loc_groups(long capacity) {
  const long n = (capacity + EVM_THREADS - 1) / EVM_THREADS;
  return (int)(n < LOC_MAX_GROUPS ? n : LOC_MAX_GROUPS);
}

// the two launches (the status words are zero when the first one runs)
static int loc_evaluate(const LocEval &a, double *sums, hipStream_t st) {
  const int grid = loc_groups(a.capacity);
  hipLaunchKernelGGL(loc_eval_kernel, dim3(grid), dim3(EVM_THREADS), 0, st, a);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(loc_final_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, a.rows, grid, a.status, sums, a.done);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

// ---------------------------------------------------------------------------------------------------- the loop
struct LocState {
  double C[7], lambda, f, f0, reach, H[21], b[6], trial[7];
  int32_t n_accepted, n_evals, rejects, reason, seen, spare[3];
  int32_t status[8];                       // the words of the evaluation at C
  int32_t done[4];                         // [0]: reason != 0, the word the evaluation's launches read
  float cam[8];                            // the pose the next evaluation reads: float32(C), then float32(trial)
  float cam_C[8];                          // the bits the evaluation at C read
  double e_sums[LOC_ROW];                  // what one evaluation writes
  int32_t e_status[8];
};

struct LocOut {
  double *pose;
  float *pose_f32;
  double *result, *hessian, *gradient, *history;
  int32_t *status, *info;
};

struct LocWs {
  double *rows;
  LocState *state;
};
static size_t loc_carve(void *ws, LocWs *w) {
  WsCarver c(ws);
  w->rows = c.take<double>((size_t)LOC_MAX_GROUPS * LOC_ROW, 256);
  w->state = c.take<LocState>(1, 256);
  return c.bytes();
}

static __device__ __forceinline__ int loc_tri(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }   // i <= j

// One wave.  Every lane loads the whole state and takes every decision itself (uniform loads, no shuffles, no LDS): the
// arithmetic below is the header's, in its order, once per lane; low lanes then store.  e: the index of the evaluation in front.
__global__ void __launch_bounds__(RAMP_WAVE)
    localize_step_kernel(LocState *__restrict__ s, int e, int last, int iters, double lambda0, double min_step, const LocOut out) {
  const int lane = threadIdx.x;
  int reason = s->reason;
  if (reason != 0 && !last) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  double C[7], trial[7], Hk[21], b[6];
#pragma unroll
  for (int i = 0; i < 7; i++) { C[i] = s->C[i]; trial[i] = s->trial[i]; }
#pragma unroll
  for (int i = 0; i < 21; i++) Hk[i] = s->H[i];
#pragma unroll
  for (int i = 0; i < 6; i++) b[i] = s->b[i];
  double lambda = s->lambda, f = s->f, f0 = s->f0, reach = s->reach;
  int n_accepted = s->n_accepted, n_evals = s->n_evals, rejects = s->rejects, seen = s->seen;
  if (reason == 0) {
    const double cost = s->e_sums[LOC_COST], reach_e = s->e_sums[LOC_REACH];
    n_evals += 1;
    seen |= s->e_status[0];
    bool take;
    if (e == 0) {
#pragma unroll
      for (int i = 0; i < 7; i++) C[i] = (double)s->cam[i];
      lambda = lambda0;
      f = f0 = cost;
      take = true;
      for (int i = lane; i < iters; i += RAMP_WAVE) out.history[i] = qnan;
      if (reach_e < 6.0) reason = RAMP_LOCALIZE_FEW;
      else if (iters == 0) reason = RAMP_LOCALIZE_ITERS;
    } else if (cost < f) {                               // (a NaN cost is not smaller)
#pragma unroll
      for (int i = 0; i < 7; i++) C[i] = trial[i];
      f = cost;
      take = true;
      if (lane == 0) out.history[n_accepted] = f;
      n_accepted += 1;
      lambda = lambda / 10.0;
      if (!(lambda > 1e-12)) lambda = 1e-12;
      rejects = 0;
      if (n_accepted == iters) reason = RAMP_LOCALIZE_ITERS;
      else if (reach_e < 6.0) reason = RAMP_LOCALIZE_FEW;
    } else {
      take = false;
      lambda = lambda * 10.0;
      rejects += 1;
      if (rejects == RAMP_LOCALIZE_REJECTS) reason = RAMP_LOCALIZE_STALLED;
    }
    if (take) {
#pragma unroll
      for (int i = 0; i < 21; i++) Hk[i] = s->e_sums[LOC_H + i];
#pragma unroll
      for (int i = 0; i < 6; i++) b[i] = s->e_sums[LOC_B + i];
      reach = reach_e;
      if (lane < 8) {
        s->status[lane] = s->e_status[lane];
        s->cam_C[lane] = s->cam[lane];
      }
    }
    if (reason == 0) {                                   // propose
      double L[6][6], y[6], delta[6];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        double sum = Hk[loc_tri(j, j)] + lambda * Hk[loc_tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) sum = sum - L[j][k] * L[j][k];
        if (!(sum > 0.0 && sum < inf)) reason = RAMP_LOCALIZE_SINGULAR;
        L[j][j] = sqrt(sum);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
          double t = Hk[loc_tri(j, i)];
#pragma unroll
          for (int k = 0; k < j; k++) t = t - L[i][k] * L[j][k];
          L[i][j] = t / L[j][j];
        }
      }
      if (reason == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
          double t = -b[i];
#pragma unroll
          for (int k = 0; k < i; k++) t = t - L[i][k] * y[k];
          y[i] = t / L[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; i--) {
          double t = y[i];
#pragma unroll
          for (int k = i + 1; k < 6; k++) t = t - L[k][i] * delta[k];
          delta[i] = t / L[i][i];
        }
        double dd = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) dd = dd + delta[i] * delta[i];
        if (sqrt(dd) < min_step) reason = RAMP_LOCALIZE_CONVERGED;
        else {                                           // trial = retract(C, delta): C' = C D^-1, D = (R(dq), v), dq the Cayley map
          const double w0 = delta[3], w1 = delta[4], w2 = delta[5];
          const double ww = (w0 * w0 + w1 * w1) + w2 * w2;
          const double sc = sqrt(1.0 + ww / 4.0);
          const double bx = -((w0 / 2.0) / sc), by = -((w1 / 2.0) / sc), bz = -((w2 / 2.0) / sc), bw = 1.0 / sc;   // conj(dq)
          const double ax = C[3], ay = C[4], az = C[5], aw = C[6];
          double qx = ((aw * bx + ax * bw) + ay * bz) - az * by;
          double qy = ((aw * by - ax * bz) + ay * bw) + az * bx;
          double qz = ((aw * bz + ax * by) - ay * bx) + az * bw;
          double qw = ((aw * bw - ax * bx) - ay * by) - az * bz;
          const double nq = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
          qx = qx / nq; qy = qy / nq; qz = qz / nq; qw = qw / nq;
          const double v0 = delta[0], v1 = delta[1], v2 = delta[2];
          double u0 = qy * v2 - qz * v1, u1 = qz * v0 - qx * v2, u2 = qx * v1 - qy * v0;      // lt_qrot, in float64
          u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
          trial[0] = C[0] - ((v0 + qw * u0) + (qy * u2 - qz * u1));
          trial[1] = C[1] - ((v1 + qw * u1) + (qz * u0 - qx * u2));
          trial[2] = C[2] - ((v2 + qw * u2) + (qx * u1 - qy * u0));
          trial[3] = qx; trial[4] = qy; trial[5] = qz; trial[6] = qw;
        }
      }
    }
    if (last && reason == 0) reason = RAMP_LOCALIZE_BUDGET;
#pragma unroll
    for (int i = 0; i < 7; i++)
      if (lane == i) {
        s->C[i] = C[i]; s->trial[i] = trial[i];
        if (reason == 0) s->cam[i] = (float)trial[i];    // round to nearest even; a pose that is not finite is the evaluation's to answer
      }
    if (lane < 21) s->H[lane] = Hk[lane];
    if (lane < 6) s->b[lane] = b[lane];
    if (lane < 8) s->e_status[lane] = 0;                 // the next evaluation's counters start at zero
    if (lane == 0) {
      s->lambda = lambda; s->f = f; s->f0 = f0; s->reach = reach;
      s->n_accepted = n_accepted; s->n_evals = n_evals; s->rejects = rejects; s->reason = reason; s->seen = seen;
      s->done[0] = reason != 0;
    }
  }
  if (!last) return;
  // never a plausible pose: FEW at the start, SINGULAR with nothing accepted, a camera that was not finite
  const bool no_pose = (n_accepted == 0 && (reason == RAMP_LOCALIZE_FEW || reason == RAMP_LOCALIZE_SINGULAR)) ||
                       (seen & RAMP_MAP_LOCALIZE_BAD_CAMERA) != 0;
  if (lane < 7) {
    out.pose[lane] = no_pose ? qnan : C[lane];
    out.pose_f32[lane] = no_pose ? __int_as_float(0x7fc00000) : s->cam_C[lane];
  }
  if (lane < 36) {
    const int i = lane / 6, j = lane - 6 * i;
    out.hessian[lane] = Hk[i <= j ? loc_tri(i, j) : loc_tri(j, i)];
  }
  if (lane < 6) out.gradient[lane] = b[lane];
  if (lane < 8) {
    out.status[lane] = s->status[lane];                  // (this lane's own stores above, or an earlier launch's)
    out.info[lane] = lane == 0 ? reason : lane == 1 ? n_accepted : lane == 2 ? n_evals : lane == 3 ? rejects : lane == 4 ? seen : 0;
  }
  if (lane < 4) out.result[lane] = lane == 0 ? f : lane == 1 ? f0 : lane == 2 ? lambda : reach;
}

static int loc_check(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam,
                     const float *intrinsics, const float *surface, int H, int W, const void *ws, const int32_t *status) {
  if (H < 2 || W < 2 || !evm_capacity_ok(capacity)) return RAMP_EINVAL;
  if (!(voxel > 0.0) || !(voxel <= 1.7976931348623157e308) || min_points < 0 || min_views < 0) return RAMP_EINVAL;
  if (!map || !cam || !intrinsics || !surface || !ws || !status) return RAMP_EINVAL;
  if (((uintptr_t)map & 63) != 0 || ((uintptr_t)ws & 255) != 0) return RAMP_EINVAL;
  if ((((uintptr_t)cam | (uintptr_t)intrinsics | (uintptr_t)surface | (uintptr_t)status) & 3) != 0) return RAMP_EINVAL;
  if ((double)H * (double)W >= 2147483648.0) return RAMP_EUNSUPPORTED;
  return RAMP_OK;
}

extern "C" {
size_t ramp_point_map_localize_ws_bytes(long capacity, int iters) {
  if (!evm_capacity_ok(capacity) || iters < 0 || iters > RAMP_LOCALIZE_MAX_ITERS) return 0;
  LocWs w;
  return loc_carve(nullptr, &w);
}

long ramp_point_map_localize_grid_slots(void) { return (long)LOC_MAX_GROUPS * EVM_THREADS; }

int ramp_point_map_localize_eval(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam,
                                 const float *intrinsics, const float *surface, int H, int W, double huber, double *sums,
                                 float *records, void *ws, size_t ws_bytes, int32_t *status, void *stream) {
  const int rc = loc_check(map, capacity, voxel, min_points, min_views, cam, intrinsics, surface, H, W, ws, status);
  if (rc != RAMP_OK) return rc;
  if (!sums || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)records & 3) != 0 || huber != huber) return RAMP_EINVAL;
  LocWs w;
  if (ws_bytes < loc_carve(ws, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const LocEval a = {evm_slots(const_cast<void *>(map)), capacity, voxel, (long long)min_points, min_views, cam, intrinsics, surface,
                     H, W, huber, records, w.rows, status, nullptr};
  return loc_evaluate(a, sums, st);
}

int ramp_point_map_localize(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam0,
                            const float *intrinsics, const float *surface, int H, int W, double huber, double lambda0,
                            double min_step, int iters, int max_evals, double *pose_out, float *pose_f32, double *result,
                            double *hessian, double *gradient, double *history, int32_t *status, int32_t *info, void *ws,
                            size_t ws_bytes, void *stream) {
  const int rc = loc_check(map, capacity, voxel, min_points, min_views, cam0, intrinsics, surface, H, W, ws, status);
  if (rc != RAMP_OK) return rc;
  if (iters < 0 || iters > RAMP_LOCALIZE_MAX_ITERS || huber != huber) return RAMP_EINVAL;
  if (!(lambda0 >= 0.0) || !(lambda0 <= 1.7976931348623157e308) || !(min_step >= 0.0) || !(min_step <= 1.7976931348623157e308)) return RAMP_EINVAL;
  if (!pose_out || !pose_f32 || !result || !hessian || !gradient || (!history && iters > 0) || !info) return RAMP_EINVAL;
  if ((((uintptr_t)pose_out | (uintptr_t)result | (uintptr_t)hessian | (uintptr_t)gradient | (uintptr_t)history) & 7) != 0 ||
      (((uintptr_t)pose_f32 | (uintptr_t)info) & 3) != 0)
    return RAMP_EINVAL;
  LocWs w;
  if (ws_bytes < loc_carve(ws, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int need = 1 + (RAMP_LOCALIZE_REJECTS + 1) * iters;
  const int evals = max_evals <= 0 ? need : (max_evals < need ? max_evals : need);
  LocState *s = w.state;
  // the invariant front: the state zeroed (reason 0, the done word 0, the counters 0), the start where evaluation 0 reads it
  if (hipMemsetAsync(s, 0, sizeof(LocState), st) != hipSuccess) return RAMP_ELAUNCH;
  if (hipMemcpyAsync(s->cam, cam0, 7 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return RAMP_ELAUNCH;
  const LocEval a = {evm_slots(const_cast<void *>(map)), capacity, voxel, (long long)min_points, min_views, s->cam, intrinsics, surface,
                     H, W, huber, nullptr, w.rows, s->e_status, s->done};
  const LocOut out = {pose_out, pose_f32, result, hessian, gradient, history, status, info};
  for (int e = 0; e < evals; e++) {
    const int erc = loc_evaluate(a, s->e_sums, st);
    if (erc != RAMP_OK) return erc;
    hipLaunchKernelGGL(localize_step_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, s, e, e == evals - 1 ? 1 : 0, iters, lambda0, min_step, out);
    RAMP_CHECK_LAUNCH();
  }
  return RAMP_OK;
}
}  // extern "C"
