// IMU on the device (include/ramp_hip.h: ramp_imu_preintegrate, ramp_imu_align): on-manifold preintegration of raw gyro and
// accelerometer samples between the frames' time stamps, and the alignment of the vision trajectory to those preintegrals --
// gyro bias, metric scale, gravity, velocities.  All arithmetic is float64 without FMA contraction; nothing is read back.
//
//   imu_check_kernel      the order of tau and of the knot times -> RAMP_IMU_BAD_ORDER; the sample count; the start bias
//   imu_integrate_kernel  ONE WAVE PER INTERVAL: two binary searches in tau give its samples; the sub-intervals are walked in
//                         chunks of 64, one per lane; a chunk is reduced by an ORDERED shuffle tree (offsets 1, 2, 4, ...: lane
//                         i takes own o lane(i + off), lanes beyond the tail hold the identity, which is neutral to the bit on
//                         either side); chunks chain left to right in lane 0.  A record's bits are a function of its own
//                         interval's samples and the biases alone.  An interval with 10^6 samples costs one wave's walk.
//   imu_gyro_part_kernel  per interval r = Log(dR^T R_wb,k^T R_wb,k+1), J^T J and J^T r; per-workgroup partials, fixed order
//   imu_gyro_final_kernel one wave: the partials in index order, a 3 x 3 Cholesky solve in lane 0, bias += delta
//   imu_scale_part_kernel per triple of knots the three rows in (s, g); per-workgroup partials of N and y
//   imu_scale_final_kernel one wave: the partials, a 4 x 4 Cholesky solve, with a gravity norm four tangent refinements
//   imu_velocity_kernel   one workgroup: velocities per knot, the row residual per triple, its rms, the status words
//
// ramp_imu_align enqueues: one memset, check, (integrate, gyro part, gyro final) x gyro_steps, integrate, scale part, scale
// final, velocity.  The alignment RE-INTEGRATES with the corrected bias; it carries no bias Jacobians of dv and dp.
// No floating-point atomics anywhere: the counters are integers, the sums are partials summed in an order fixed by K.
#include "imu_device.h"

#define IMU_THREADS 256
#define IMU_WAVES (IMU_THREADS / RAMP_WAVE)
#define IMU_MAX_GROUPS 2048
#define IMU_CTR_WORDS 16                   // int32: the 8 status words, 8 spare
#define IMU_STATE_WORDS 16                 // float64: [0..2] the gyro bias as it stands, [4..7] x = (s, g), the rest spare
#define IMU_PART_WORDS 16                  // float64 per workgroup partial: 9 sums, the rest spare
#define IMU_REC RAMP_IMU_PREINT_WORDS

static __device__ __forceinline__ void imu_shfl_down(const ImuElem &e, int off, bool have, ImuElem &o) {
  const double *src = reinterpret_cast<const double *>(&e);
  double *dst = reinterpret_cast<double *>(&o);
  ImuElem id;
  imu_identity(id);
  const double *idw = reinterpret_cast<const double *>(&id);
#pragma unroll
  for (int c = 0; c < 20; c++) {
    const double v = __shfl_down(src[c], off);
    dst[c] = have ? v : idw[c];
  }
}

// the number of tau <= t (UPPER) or < t
template <bool UPPER>
static __device__ __forceinline__ long imu_bound(const double *__restrict__ tau, long N, double t) {
  long lo = 0, hi = N;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (UPPER ? tau[mid] <= t : tau[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct ImuArgs {
  const double *tau;
  const void *gyro, *accel;                 // [N][3] float or double
  const double *times;
  const double *bias_dev;                   // the gyro bias on the device, or nullptr: bias_g
  double *preint;                           // [K - 1][24]
  int32_t *ctr;
  double bias_g[3], bias_a[3], max_gap;
  long N;
  int K, stride, count;                     // count: add this integration's intervals to ctr[2..4]
};

template <typename S>
__global__ void __launch_bounds__(IMU_THREADS) imu_integrate_kernel(const ImuArgs a) {
  const int tid = threadIdx.x, lane = tid & (RAMP_WAVE - 1);
  const long k = ((long)blockIdx.x * IMU_THREADS + tid) / RAMP_WAVE;        // wave-uniform
  if (k >= a.K - 1) return;
  const double *__restrict__ tau = a.tau;
  const S *__restrict__ gy = reinterpret_cast<const S *>(a.gyro);
  const S *__restrict__ ac = reinterpret_cast<const S *>(a.accel);
  const long N = a.N;
  const double T0 = a.times[(size_t)k * a.stride], T1 = a.times[(size_t)(k + 1) * a.stride];
  double bg[3], ba[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { bg[c] = a.bias_dev ? a.bias_dev[c] : a.bias_g[c]; ba[c] = a.bias_a[c]; }
  int why = 0;                              // 1 not covered (range, gap, not finite), 2 dt <= 0
  long lo = 0, hi = 0;
  bool bias_ok = true;                      // (a failed gyro step leaves NaN: nothing is integrated with it)
#pragma unroll
  for (int c = 0; c < 3; c++) bias_ok = bias_ok && interp_finite(bg[c]);
  if ((a.ctr[0] & RAMP_IMU_BAD_ORDER) || !bias_ok) why = 1;
  else if (!(T1 > T0)) why = 2;
  else if (!(tau[0] <= T0 && T1 <= tau[N - 1])) why = 1;
  else {
    lo = imu_bound<true>(tau, N, T0);       // the samples strictly inside are [lo, hi)
    hi = imu_bound<false>(tau, N, T1);
    if (lo < 1 || hi > N - 1 || hi < lo) why = 1;      // (cannot happen for ordered tau)
  }
  ImuElem acc;
  imu_identity(acc);
  const long m = hi - lo + 1;               // sub-intervals
  bool bad = false;
  if (why == 0) {
    for (long c0 = 0; c0 < m; c0 += RAMP_WAVE) {
      const long j = c0 + lane;
      ImuElem e;
      imu_identity(e);
      if (j < m) {
        // both ends of sub-interval j lie between the samples i0 and i0 + 1
        const long i0 = lo + j - 1;
        const double t0 = tau[i0], t1 = tau[i0 + 1];
        double g0[3], g1[3], f0[3], f1[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          g0[c] = (double)gy[3 * (size_t)i0 + c]; g1[c] = (double)gy[3 * (size_t)i0 + 3 + c];
          f0[c] = (double)ac[3 * (size_t)i0 + c]; f1[c] = (double)ac[3 * (size_t)i0 + 3 + c];
          bad = bad || !interp_finite(g0[c]) || !interp_finite(g1[c]) || !interp_finite(f0[c]) || !interp_finite(f1[c]);
        }
        bad = bad || (t1 - t0) > a.max_gap;
        double u0 = t0, u1 = t1;
        if (j == 0) {
          u0 = T0;
          if (T0 != t0) {
            const double al = (T0 - t0) / (t1 - t0);
#pragma unroll
            for (int c = 0; c < 3; c++) { g0[c] = g0[c] + al * (g1[c] - g0[c]); f0[c] = f0[c] + al * (f1[c] - f0[c]); }
          }
        }
        if (j == m - 1) {
          u1 = T1;
          if (T1 != t1) {
            // (g0, f0 may be the interpolated start when m == 1: the sample's own values are read again)
            const double al = (T1 - t0) / (t1 - t0);
#pragma unroll
            for (int c = 0; c < 3; c++) {
              const double gs = (double)gy[3 * (size_t)i0 + c], fs = (double)ac[3 * (size_t)i0 + c];
              g1[c] = gs + al * (g1[c] - gs);
              f1[c] = fs + al * (f1[c] - fs);
            }
          }
        }
        const double dt = u1 - u0;
        double w[3], f[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { w[c] = 0.5 * (g0[c] + g1[c]) - bg[c]; f[c] = 0.5 * (f0[c] + f1[c]) - ba[c]; }
        imu_element(w, f, dt, e);
      }
      // the ordered tree: after the last level lane 0 holds e_0 o e_1 o ... o e_63
#pragma unroll 1
      for (int off = 1; off < RAMP_WAVE; off <<= 1) {
        ImuElem o;
        imu_shfl_down(e, off, lane + off < RAMP_WAVE, o);
        imu_compose(e, o);
      }
      if (c0 == 0) acc = e; else imu_compose(acc, e);      // (lane 0's is the one that counts)
    }
    if (__ballot(bad) != 0) why = 1;
  }
  if (lane == 0) {
    double *rec = a.preint + IMU_REC * (size_t)k;
    if (why) {
      for (int c = 0; c < IMU_REC; c++) rec[c] = imu_nan();
    } else {
      imu_qnorm(acc.q);
      if (acc.q[3] < 0.0) { acc.q[0] = -acc.q[0]; acc.q[1] = -acc.q[1]; acc.q[2] = -acc.q[2]; acc.q[3] = -acc.q[3]; }
      rec[0] = acc.t;
      rec[1] = (double)m;
#pragma unroll
      for (int c = 0; c < 4; c++) rec[2 + c] = acc.q[c];
#pragma unroll
      for (int c = 0; c < 3; c++) { rec[6 + c] = acc.v[c]; rec[9 + c] = acc.p[c]; rec[21 + c] = 0.0; }
#pragma unroll
      for (int c = 0; c < 9; c++) rec[12 + c] = acc.J[c];
    }
  }
  if (a.count) ramp_wave_flush(a.ctr + 2, tid, 1, why == 1 ? 1 : 0, why == 2 ? 1 : 0);
}

// tau and the knot times: finite and not decreasing, or RAMP_IMU_BAD_ORDER; the samples counted; the start bias into `state`
__global__ void __launch_bounds__(IMU_THREADS)
    imu_check_kernel(const double *__restrict__ tau, long N, const double *__restrict__ times, int T, int32_t *__restrict__ ctr,
                     double *__restrict__ state, double b0, double b1, double b2) {
  const int tid = threadIdx.x;
  const long n = N > T ? N : (long)T;
  int n_seen = 0, n_bad = 0;                                       // wave-uniform: sums of ballots
  for (long base = (long)blockIdx.x * IMU_THREADS; base < n; base += (long)gridDim.x * IMU_THREADS) {
    const long i = base + tid;
    bool bad = false;
    if (i < N) bad = !interp_finite(tau[i]) || (i + 1 < N && tau[i + 1] < tau[i]);
    if (i < T) bad = bad || !interp_finite(times[i]) || (i + 1 < T && times[i + 1] < times[i]);
    n_seen += ramp_wave_count(i < N);
    n_bad += ramp_wave_count(bad);
  }
  ramp_wave_flush(ctr + 1, tid, n_seen);
  if (n_bad && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(ctr, RAMP_IMU_BAD_ORDER);
  if (state && blockIdx.x == 0 && tid == 0) { state[0] = b0; state[1] = b1; state[2] = b2; }
}

// ---------------------------------------------------------------------------------------------- alignment
struct ImuAlign {
  const float *knots;                       // [T][7] camera to world
  const double *preint;
  double *state, *part;
  int32_t *ctr;
  double *result, *normal, *velocity, *residual;
  int32_t *status;
  double q_bc[4], lever[3];                 // R_bc as a unit quaternion;  -R_bc^T p_bc
  double gravity_norm;
  int K, stride, first;                     // first: the first gyro step counts its intervals into ctr[5]
};

// knot k of the K used: R_wb as a unit quaternion, pbar, c = R_wc (-R_bc^T p_bc)
static __device__ __forceinline__ void imu_body(const ImuAlign &a, int k, double *qwb, double *pbar, double *c) {
  const float *row = a.knots + 7 * (size_t)k * a.stride;
  double q[4] = {(double)row[3], (double)row[4], (double)row[5], (double)row[6]};
  imu_qnorm(q);
  const double qi[4] = {-a.q_bc[0], -a.q_bc[1], -a.q_bc[2], a.q_bc[3]};
  imu_qmul(q, qi, qwb);
  pbar[0] = (double)row[0]; pbar[1] = (double)row[1]; pbar[2] = (double)row[2];
  imu_qrot(q, 1.0, a.lever, c);
}

static __device__ __forceinline__ bool imu_covered(const double *rec) { return rec[0] == rec[0]; }

// sums v[0..n) over the workgroup in a fixed order -> part row of this workgroup (thread 0)
template <int n>
static __device__ __forceinline__ void imu_group_sum(double *v, double *s_red, double *row) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < n; c++) {
    v[c] = ramp_wave_sum(v[c]);
    if ((tid & (RAMP_WAVE - 1)) == 0) s_red[(tid / RAMP_WAVE) * IMU_PART_WORDS + c] = v[c];
  }
  __syncthreads();
  if (tid < n) {
    double s = 0.0;
    for (int w = 0; w < IMU_WAVES; w++) s += s_red[w * IMU_PART_WORDS + tid];
    row[tid] = s;
  }
}

// one wave: the partials of P workgroups, lane q takes q, q + 64, ..., then the butterfly -> every lane holds the sums
template <int n>
static __device__ __forceinline__ void imu_final_sum(const double *part, int P, double *v) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int c = 0; c < n; c++) {
    double s = 0.0;
    for (int q = lane; q < P; q += RAMP_WAVE) s += part[(size_t)q * IMU_PART_WORDS + c];
    v[c] = ramp_wave_sum(s);
  }
}

// x = A^-1 b for a symmetric positive definite A [n][n] by Cholesky; false when a pivot is not positive and finite
template <int n>
static __device__ __forceinline__ bool imu_chol_solve(const double *A, const double *b, double *x, double *pmin, double *pmax) {
  double L[n * n];
  bool ok = true;
  double lo = 0.0, hi = 0.0;
#pragma unroll
  for (int j = 0; j < n; j++) {
    double d = A[j * n + j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= L[j * n + k] * L[j * n + k];
    ok = ok && d > 0.0 && interp_finite(d);
    lo = j == 0 ? d : fmin(lo, d);
    hi = j == 0 ? d : fmax(hi, d);
    const double l = sqrt(d);
    L[j * n + j] = l;
#pragma unroll
    for (int i = j + 1; i < n; i++) {
      double s = A[i * n + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
      L[i * n + j] = s / l;
    }
  }
  double z[n];
#pragma unroll
  for (int i = 0; i < n; i++) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i * n + k] * z[k];
    z[i] = s / L[i * n + i];
  }
#pragma unroll
  for (int i = n - 1; i >= 0; i--) {
    double s = z[i];
#pragma unroll
    for (int k = i + 1; k < n; k++) s -= L[k * n + i] * x[k];
    x[i] = s / L[i * n + i];
  }
  *pmin = lo;
  *pmax = hi;
  return ok;
}

__global__ void __launch_bounds__(IMU_THREADS) imu_gyro_part_kernel(const ImuAlign a) {
  __shared__ double s_red[IMU_WAVES * IMU_PART_WORDS];
  const int tid = threadIdx.x;
  const long k = (long)blockIdx.x * IMU_THREADS + tid;
  double v[9];
#pragma unroll
  for (int c = 0; c < 9; c++) v[c] = 0.0;
  bool used = false;
  if (k < a.K - 1) {
    const double *rec = a.preint + IMU_REC * (size_t)k;
    if (imu_covered(rec)) {
      used = true;
      double q0[4], q1[4], pb[3], cc[3], t[4], rel[4], r[3];
      imu_body(a, (int)k, q0, pb, cc);
      imu_body(a, (int)k + 1, q1, pb, cc);
      const double dqi[4] = {-rec[2], -rec[3], -rec[4], rec[5]}, q0i[4] = {-q0[0], -q0[1], -q0[2], q0[3]};
      imu_qmul(q0i, q1, t);
      imu_qmul(dqi, t, rel);
      imu_qnorm(rel);
      imu_qlog(rel, r);
      const double *J = rec + 12;
      // H = J^T J (upper triangle: 00 01 02 11 12 22), b = J^T r
      int at = 0;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) v[at++] = (J[i] * J[j] + J[3 + i] * J[3 + j]) + J[6 + i] * J[6 + j];
#pragma unroll
      for (int i = 0; i < 3; i++) v[6 + i] = (J[i] * r[0] + J[3 + i] * r[1]) + J[6 + i] * r[2];
    }
  }
  const int n_used = ramp_wave_count(used);
  if (a.first) ramp_wave_flush(a.ctr + 5, tid, n_used);
  imu_group_sum<9>(v, s_red, a.part + (size_t)blockIdx.x * IMU_PART_WORDS);
}

__global__ void __launch_bounds__(RAMP_WAVE) imu_gyro_final_kernel(const ImuAlign a, int P) {
  double v[9];
  imu_final_sum<9>(a.part, P, v);
  if (threadIdx.x != 0) return;
  const double H[9] = {v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]}, b[3] = {v[6], v[7], v[8]};
  double d[3], lo, hi;
  bool ok = a.ctr[5] >= 1 && !(a.ctr[0] & RAMP_IMU_GYRO_FAILED);
#pragma unroll
  for (int c = 0; c < 9; c++) ok = ok && interp_finite(v[c]);
  ok = imu_chol_solve<3>(H, b, d, &lo, &hi) && ok;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double nb = ok ? a.state[c] + d[c] : imu_nan();
    ok = ok && interp_finite(nb);
    a.state[c] = nb;
  }
  if (!ok) {
    a.state[0] = a.state[1] = a.state[2] = imu_nan();
    atomicOr(a.ctr, RAMP_IMU_GYRO_FAILED);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) a.result[4 + c] = a.state[c];
#pragma unroll
  for (int c = 0; c < 9; c++) a.normal[20 + c] = H[c];
#pragma unroll
  for (int c = 0; c < 3; c++) a.normal[29 + c] = b[c];
}

// the rows of the triple of knots j, j + 1, j + 2:  s d - h g = rhs;  false when one of its two intervals is not covered
static __device__ __forceinline__ bool imu_triple(const ImuAlign &a, long j, double *d, double *h, double *rhs) {
  const double *r1 = a.preint + IMU_REC * (size_t)j, *r2 = r1 + IMU_REC;
  if (!(imu_covered(r1) && imu_covered(r2))) return false;
  double q1[4], q2[4], q3[4], p1[3], p2[3], p3[3], c1[3], c2[3], c3[3], x1[3], x2[3], xv[3];
  imu_body(a, (int)j, q1, p1, c1);
  imu_body(a, (int)j + 1, q2, p2, c2);
  imu_body(a, (int)j + 2, q3, p3, c3);
  const double t1 = r1[0], t2 = r2[0];
  imu_qrot(q1, 1.0, r1 + 9, x1);             // R1 dp1
  imu_qrot(q2, 1.0, r2 + 9, x2);             // R2 dp2
  imu_qrot(q1, 1.0, r1 + 6, xv);             // R1 dv1
#pragma unroll
  for (int c = 0; c < 3; c++) {
    d[c] = (p3[c] - p2[c]) / t2 - (p2[c] - p1[c]) / t1;
    rhs[c] = (((x2[c] / t2 - x1[c] / t1) + xv[c]) - (c3[c] - c2[c]) / t2) + (c2[c] - c1[c]) / t1;
  }
  *h = 0.5 * (t1 + t2);
  return true;
}

__global__ void __launch_bounds__(IMU_THREADS) imu_scale_part_kernel(const ImuAlign a) {
  __shared__ double s_red[IMU_WAVES * IMU_PART_WORDS];
  const int tid = threadIdx.x;
  const long j = (long)blockIdx.x * IMU_THREADS + tid;
  double v[9];
#pragma unroll
  for (int c = 0; c < 9; c++) v[c] = 0.0;
  bool used = false;
  double d[3], h, rhs[3];
  if (j < a.K - 2 && imu_triple(a, j, d, &h, rhs)) {
    used = true;
    // A = [d | -h I]:  N00 = d.d, N0i = -h d_i, Nii = h^2 (the other words of A^T A are zero);  y0 = d.rhs, yi = -h rhs_i
    v[0] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    v[4] = h * h;
    v[5] = (d[0] * rhs[0] + d[1] * rhs[1]) + d[2] * rhs[2];
#pragma unroll
    for (int c = 0; c < 3; c++) { v[1 + c] = -h * d[c]; v[6 + c] = -h * rhs[c]; }
  }
  ramp_wave_flush(a.ctr + 6, tid, ramp_wave_count(used));
  imu_group_sum<9>(v, s_red, a.part + (size_t)blockIdx.x * IMU_PART_WORDS);
}

__global__ void __launch_bounds__(RAMP_WAVE) imu_scale_final_kernel(const ImuAlign a, int P) {
  double v[9];
  imu_final_sum<9>(a.part, P, v);
  if (threadIdx.x != 0) return;
  const double N[16] = {v[0], v[1], v[2], v[3], v[1], v[4], 0.0, 0.0, v[2], 0.0, v[4], 0.0, v[3], 0.0, 0.0, v[4]};
  const double y[4] = {v[5], v[6], v[7], v[8]};
  double x[4], lo = 0.0, hi = 0.0;
  int bits = 0;
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 9; c++) finite = finite && interp_finite(v[c]);
  if (a.ctr[6] < 2) bits = RAMP_IMU_SCALE_FAILED | RAMP_IMU_FEW_TRIPLES;
  else if (!finite || !imu_chol_solve<4>(N, y, x, &lo, &hi)) bits = RAMP_IMU_SCALE_FAILED | RAMP_IMU_SINGULAR;
  const double G = a.gravity_norm;
  if (!bits && G > 0.0) {
    double gn = sqrt((x[1] * x[1] + x[2] * x[2]) + x[3] * x[3]);
    double gh[3] = {x[1] / gn, x[2] / gn, x[3] / gn};
#pragma unroll 1
    for (int it = 0; it < 4 && !bits; it++) {
      // b1 = normalise(gh x e), e the axis of the smallest |gh| component (the first on ties); b2 = gh x b1
      const double ax = fabs(gh[0]), ay = fabs(gh[1]), az = fabs(gh[2]);
      const int ei = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
      const double e[3] = {ei == 0 ? 1.0 : 0.0, ei == 1 ? 1.0 : 0.0, ei == 2 ? 1.0 : 0.0};
      double b1[3] = {gh[1] * e[2] - gh[2] * e[1], gh[2] * e[0] - gh[0] * e[2], gh[0] * e[1] - gh[1] * e[0]};
      const double n1 = sqrt((b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2]);
      b1[0] /= n1; b1[1] /= n1; b1[2] /= n1;
      const double b2[3] = {gh[1] * b1[2] - gh[2] * b1[1], gh[2] * b1[0] - gh[0] * b1[2], gh[0] * b1[1] - gh[1] * b1[0]};
      // P = [e_s, (0, b1), (0, b2)], x0 = (0, G gh):  (P^T N P) z = P^T (y - N x0)
      const double P4[12] = {1.0, 0.0, 0.0, 0.0, b1[0], b2[0], 0.0, b1[1], b2[1], 0.0, b1[2], b2[2]};
      const double x0[4] = {0.0, G * gh[0], G * gh[1], G * gh[2]};
      double res[4], NP[12], M[9], r[3], z[3], l3, h3;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) s += N[4 * i + k] * x0[k];
        res[i] = y[i] - s;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          double t = 0.0;
#pragma unroll
          for (int k = 0; k < 4; k++) t += N[4 * i + k] * P4[3 * k + c];
          NP[3 * i + c] = t;
        }
      }
#pragma unroll
      for (int i = 0; i < 3; i++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) s += P4[3 * k + i] * res[k];
        r[i] = s;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          double t = 0.0;
#pragma unroll
          for (int k = 0; k < 4; k++) t += P4[3 * k + i] * NP[3 * k + c];
          M[3 * i + c] = t;
        }
      }
      if (!imu_chol_solve<3>(M, r, z, &l3, &h3)) { bits = RAMP_IMU_SCALE_FAILED | RAMP_IMU_SINGULAR; break; }
      double g[3];
#pragma unroll
      for (int c = 0; c < 3; c++) g[c] = (G * gh[c] + z[1] * b1[c]) + z[2] * b2[c];
      gn = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
      for (int c = 0; c < 3; c++) { gh[c] = g[c] / gn; x[1 + c] = G * gh[c]; }
      x[0] = z[0];
    }
  }
  if (!bits) {
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 4; c++) fin = fin && interp_finite(x[c]);
    if (!fin) bits = RAMP_IMU_SCALE_FAILED | RAMP_IMU_SINGULAR;
    else if (!(x[0] > 0.0)) bits = RAMP_IMU_SCALE_FAILED | RAMP_IMU_BAD_SCALE;
  }
  if (bits) atomicOr(a.ctr, bits);
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double xc = bits ? imu_nan() : x[c];
    a.result[c] = xc;
    a.state[4 + c] = xc;
  }
  a.result[8] = bits ? imu_nan() : hi / lo;
  for (int c = 9; c < 16; c++) a.result[c] = 0.0;
#pragma unroll
  for (int c = 0; c < 16; c++) a.normal[c] = N[c];
#pragma unroll
  for (int c = 0; c < 4; c++) a.normal[16 + c] = y[c];
}

// v_k = (p_k+1 - p_k - 1/2 g dt^2 - R_k dp) / dt with p = s pbar + c;  false (NaN) beside an interval that is not covered
static __device__ __forceinline__ bool imu_velocity(const ImuAlign &a, int k, const double *x, double *v) {
  const double *rec = a.preint + IMU_REC * (size_t)k;
  const bool ok = imu_covered(rec);
  double q0[4], q1[4], p0[3], p1[3], c0[3], c1[3], rp[3];
  imu_body(a, k, q0, p0, c0);
  imu_body(a, k + 1, q1, p1, c1);
  imu_qrot(q0, 1.0, rec + 9, rp);
  const double t = rec[0];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double pa = x[0] * p0[c] + c0[c], pb = x[0] * p1[c] + c1[c];
    v[c] = ok ? (((pb - pa) - 0.5 * x[1 + c] * (t * t)) - rp[c]) / t : imu_nan();
  }
  return ok;
}

__global__ void __launch_bounds__(IMU_THREADS) imu_velocity_kernel(const ImuAlign a) {
  __shared__ double s_red[IMU_WAVES];
  const int tid = threadIdx.x, K = a.K;
  const bool failed = (a.ctr[0] & RAMP_IMU_SCALE_FAILED) != 0;
  double x[4];
#pragma unroll
  for (int c = 0; c < 4; c++) x[c] = a.state[4 + c];
  for (int k = tid; k < K; k += IMU_THREADS) {
    double v[3] = {imu_nan(), imu_nan(), imu_nan()};
    if (!failed) {
      if (k < K - 1) {
        imu_velocity(a, k, x, v);
      } else if (imu_velocity(a, K - 2, x, v)) {            // the last knot: v + g dt + R dv of the last interval
        const double *rec = a.preint + IMU_REC * (size_t)(K - 2);
        double q0[4], p0[3], c0[3], rv[3];
        imu_body(a, K - 2, q0, p0, c0);
        imu_qrot(q0, 1.0, rec + 6, rv);
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = (v[c] + x[1 + c] * rec[0]) + rv[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) a.velocity[3 * (size_t)k + c] = v[c];
  }
  double sum = 0.0;
  for (int j = tid; j < K - 2; j += IMU_THREADS) {
    double d[3], h, rhs[3], res = imu_nan();
    if (!failed && imu_triple(a, j, d, &h, rhs)) {
      double e2 = 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double e = (x[0] * d[c] - h * x[1 + c]) - rhs[c];
        e2 += e * e;
      }
      res = sqrt(e2);
      sum += e2;
    }
    a.residual[j] = res;
  }
  sum = ramp_wave_sum(sum);
  if ((tid & (RAMP_WAVE - 1)) == 0) s_red[tid / RAMP_WAVE] = sum;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < IMU_WAVES; w++) s += s_red[w];
    a.result[7] = failed ? imu_nan() : sqrt(s / (double)a.ctr[6]);
  }
  if (tid < 8) a.status[tid] = tid < 7 ? a.ctr[tid] : 0;
}

// ---------------------------------------------------------------------------------------------- host
static int imu_groups(long n) { return ramp_cdiv(n > 0 ? n : 1, IMU_THREADS); }

static void imu_launch_integrate(const ImuArgs &a, bool f64, hipStream_t st) {
  const dim3 grid(ramp_cdiv((long)(a.K - 1), IMU_WAVES));
  if (f64) hipLaunchKernelGGL(imu_integrate_kernel<double>, grid, dim3(IMU_THREADS), 0, st, a);
  else hipLaunchKernelGGL(imu_integrate_kernel<float>, grid, dim3(IMU_THREADS), 0, st, a);
}

static int imu_check_grid(long N, int T) {
  const int g = imu_groups(N > T ? N : (long)T);
  return g < IMU_MAX_GROUPS ? g : IMU_MAX_GROUPS;
}

// what both entries refuse; K on success
static int imu_arguments(const double *tau, const void *gyro, const void *accel, long N, const double *times, int T, int stride,
                         const double *bias_g, const double *bias_a, double max_gap, int flags, int *K) {
  if (!tau || !gyro || !accel || !times) return RAMP_EINVAL;
  if (N < 1 || N > 2147483647l || T < 2 || stride < 1 || (flags & ~RAMP_IMU_F64)) return RAMP_EINVAL;
  if (!(max_gap > 0.0)) return RAMP_EINVAL;
  if ((((uintptr_t)tau | (uintptr_t)times) & 7) != 0) return RAMP_EINVAL;
  if ((((uintptr_t)gyro | (uintptr_t)accel) & ((flags & RAMP_IMU_F64) ? 7 : 3)) != 0) return RAMP_EINVAL;
  for (int c = 0; c < 3; c++)
    if ((bias_g && !imu_host_finite(bias_g[c])) || (bias_a && !imu_host_finite(bias_a[c]))) return RAMP_EINVAL;
  *K = (T - 1) / stride + 1;
  return *K < 2 ? RAMP_EINVAL : RAMP_OK;
}

static ImuArgs imu_args(const double *tau, const void *gyro, const void *accel, long N, const double *times, int K, int stride,
                        const double *bias_g, const double *bias_a, double max_gap) {
  ImuArgs a;
  a.tau = tau; a.gyro = gyro; a.accel = accel; a.times = times; a.bias_dev = nullptr; a.preint = nullptr; a.ctr = nullptr;
  for (int c = 0; c < 3; c++) { a.bias_g[c] = bias_g ? bias_g[c] : 0.0; a.bias_a[c] = bias_a ? bias_a[c] : 0.0; }
  a.max_gap = max_gap; a.N = N; a.K = K; a.stride = stride; a.count = 1;
  return a;
}

// ramp_imu_align's workspace for K knots, packed: ctr | state | part | records.  The counters and the state are adjacent because
// one memset clears them.
struct ImuWs {
  int32_t *ctr;
  double *state, *part, *records;
};
static size_t imu_carve(void *ws, int K, ImuWs *w) {
  WsCarver c(ws);
  w->ctr = c.take<int32_t>(IMU_CTR_WORDS, 1);
  w->state = c.take<double>(IMU_STATE_WORDS, 1);
  w->part = c.take<double>((size_t)imu_groups(K - 1) * IMU_PART_WORDS, 1);
  w->records = c.take<double>((size_t)(K - 1) * IMU_REC, 1);
  return c.bytes();
}

extern "C" {
size_t ramp_imu_workspace_bytes(long N, int K) {
  if (N < 1 || K < 2) return 0;
  ImuWs w;
  return imu_carve(nullptr, K, &w);
}

int ramp_imu_preintegrate(const double *tau, const void *gyro, const void *accel, long N, const double *times, int T, int stride,
                          const double *bias_g, const double *bias_a, double max_gap, int flags, double *preint,
                          int32_t *status, void *stream) {
  int K = 0;
  const int rc = imu_arguments(tau, gyro, accel, N, times, T, stride, bias_g, bias_a, max_gap, flags, &K);
  if (rc != RAMP_OK) return rc;
  if (!preint || !status || ((uintptr_t)preint & 7) != 0) return RAMP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  hipLaunchKernelGGL(imu_check_kernel, dim3(imu_check_grid(N, T)), dim3(IMU_THREADS), 0, st, tau, N, times, T, status,
                     (double *)nullptr, 0.0, 0.0, 0.0);
  RAMP_CHECK_LAUNCH();
  ImuArgs a = imu_args(tau, gyro, accel, N, times, K, stride, bias_g, bias_a, max_gap);
  a.preint = preint;
  a.ctr = status;
  imu_launch_integrate(a, (flags & RAMP_IMU_F64) != 0, st);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

int ramp_imu_align(const double *tau, const void *gyro, const void *accel, long N, const float *knots, const double *times, int T,
                   int stride, const double *extrinsics, const double *bias_g, const double *bias_a, double max_gap,
                   double gravity_norm, int gyro_steps, int flags, double *result, double *normal, double *velocity,
                   double *residual, double *preint, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
  int K = 0;
  const int rc = imu_arguments(tau, gyro, accel, N, times, T, stride, bias_g, bias_a, max_gap, flags, &K);
  if (rc != RAMP_OK) return rc;
  if (!knots || !result || !normal || !velocity || !status || !ws || (K > 2 && !residual)) return RAMP_EINVAL;
  if (gyro_steps < 1 || gyro_steps > RAMP_IMU_MAX_GYRO_STEPS || !(gravity_norm >= 0.0) || !imu_host_finite(gravity_norm))
    return RAMP_EINVAL;
  if ((((uintptr_t)result | (uintptr_t)normal | (uintptr_t)velocity | (uintptr_t)residual | (uintptr_t)preint) & 7) != 0 ||
      ((uintptr_t)ws & 15) != 0)
    return RAMP_EINVAL;
  ImuAlign al;
  if (!imu_extrinsics(extrinsics, al.q_bc, al.lever, nullptr)) return RAMP_EINVAL;
  ImuWs w;
  if (ws_bytes < imu_carve(ws, K, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t *ctr = w.ctr;
  double *state = w.state, *part = w.part;
  double *records = preint ? preint : w.records;
  const bool f64 = (flags & RAMP_IMU_F64) != 0;

  ImuArgs ia = imu_args(tau, gyro, accel, N, times, K, stride, bias_g, bias_a, max_gap);
  ia.preint = records;
  ia.ctr = ctr;
  ia.bias_dev = state;
  al.knots = knots; al.preint = records; al.state = state; al.part = part; al.ctr = ctr; al.result = result; al.normal = normal;
  al.velocity = velocity; al.residual = residual; al.status = status; al.gravity_norm = gravity_norm; al.K = K;
  al.stride = stride; al.first = 1;

  // the one memset: the counters and the state
  if (hipMemsetAsync(ctr, 0, ws_span(ctr, part), st) != hipSuccess) return RAMP_ELAUNCH;
  hipLaunchKernelGGL(imu_check_kernel, dim3(imu_check_grid(N, T)), dim3(IMU_THREADS), 0, st, tau, N, times, T, ctr, state,
                     ia.bias_g[0], ia.bias_g[1], ia.bias_g[2]);
  RAMP_CHECK_LAUNCH();
  const int Pg = imu_groups(K - 1), Pt = K > 2 ? imu_groups(K - 2) : 0;
  for (int step = 0; step < gyro_steps; step++) {
    ia.count = 0;
    imu_launch_integrate(ia, f64, st);
    RAMP_CHECK_LAUNCH();
    al.first = step == 0;
    hipLaunchKernelGGL(imu_gyro_part_kernel, dim3(Pg), dim3(IMU_THREADS), 0, st, al);
    RAMP_CHECK_LAUNCH();
    hipLaunchKernelGGL(imu_gyro_final_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, al, Pg);
    RAMP_CHECK_LAUNCH();
  }
  ia.count = 1;
  imu_launch_integrate(ia, f64, st);
  RAMP_CHECK_LAUNCH();
  if (Pt > 0) {
    hipLaunchKernelGGL(imu_scale_part_kernel, dim3(Pt), dim3(IMU_THREADS), 0, st, al);
    RAMP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(imu_scale_final_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, al, Pt);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(imu_velocity_kernel, dim3(1), dim3(IMU_THREADS), 0, st, al);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
