// Event landmarks (include/ramp_hip.h: ramp_event_landmarks): every corner track is triangulated from the camera poses at its
// own events' time stamps -- a midpoint solve, `refine` Gauss-Newton steps on the reprojection error, the covariance and a class.
// The definition is in the header.  The rays are fp32 (the pose of ramp_se3_interp, the rotation of ramp_event_warp); everything
// behind them is float64.
//
//   lm_key_kernel       one lane per event and segment: the classes [1] .. [4], the key (ordered bits of t, all ones for an event
//                       that is no observation) and the segment table of interp_device.h with its check of `times`
//   hipcub SortPairs    stable, 64 bits: (time key, event index)
//   lm_id_kernel        per sorted position the track id as the second key (all ones: no observation, or a failed check)
//   hipcub SortPairs    stable, 64 bits: (id, event index) -- the observations of a track are adjacent, in (t, index) order
//   lm_head_kernel      1 where a track starts
//   hipcub ExclusiveSum landmark numbers
//   lm_ray_kernel       one lane per SORTED position: segment search (knot times in LDS up to INTERP_LDS_KNOTS), pose, ray; the
//                       record (c, d, q, x, y) at the sorted position, so a landmark's records are contiguous; the per-event
//                       outputs; per head the landmark's first position and id; the last position writes count and the status
//   lm_solve_kernel     one wave per landmark, striding over the device count; lanes stride over the landmark's records; the sums
//                       go through ramp_wave_sum and the 3x3 algebra is redundant in every lane; refine + 2 passes over records
//                       that stay in L2
// No floating-point atomics; the integer atomics are the counters'.  Every loop is a bounded search, of fixed length or strided
// over a device count.
#include "workspace_cub.h"
#include "ramp_internal.h"
#include "interp_device.h"

#define LM_CTR_WORDS 16                  // int32: [0] bits, [1] .. [4] the event classes, [8] the landmarks kept
#define LM_RAY_WORDS 12                  // fp32 per sorted position: c[3], d[3], q[4], x, y
#define LM_NONE 0xffffffffffffffffull

#define LM_MAX_GROUPS 2048               // workgroups per launch; each walks the tiles of its launch with this stride
#define LM_FLT_MAX 3.4028234663852886e38f

typedef unsigned long long lm_u64;

static inline int lm_grid(long lanes) {
  const long tiles = (lanes + INTERP_THREADS - 1) / INTERP_THREADS;
  return (int)(tiles < 1 ? 1 : (tiles < LM_MAX_GROUPS ? tiles : LM_MAX_GROUPS));
}

static __device__ __forceinline__ double lm_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

static __device__ __forceinline__ bool lm_finite32(float v) { return fabsf(v) <= LM_FLT_MAX; }

// the bits of a finite t as an unsigned key that rises with t (-0.0 is 0.0); never all ones
static __device__ __forceinline__ lm_u64 lm_time_key(double t) {
  const lm_u64 b = (lm_u64)__double_as_longlong(t == 0.0 ? 0.0 : t);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(INTERP_THREADS)
    lm_key_kernel(const float *__restrict__ x, const float *__restrict__ y, const double *__restrict__ t,
                  const int64_t *__restrict__ track, long N, const float *__restrict__ knots, const double *__restrict__ times,
                  int T, int extrapolate, float *__restrict__ seg, lm_u64 *__restrict__ key, int32_t *__restrict__ iota,
                  int32_t *__restrict__ ctr) {
  const int tid = threadIdx.x;
  const long S = T > 1 ? T - 1 : 1;
  const long lanes = N > S ? N : S;
  const long tiles = (lanes + INTERP_THREADS - 1) / INTERP_THREADS;
  const double t_lo = times[0], t_hi = times[T - 1];
  int n1 = 0, n2 = 0, n3 = 0, n4 = 0;                      // wave-uniform: sums of ballots
  bool bad = false;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    if (i < S && interp_segment_row(knots, times, T, (int)i, seg + (size_t)i * INTERP_SEG_WORDS)) bad = true;
    int c = 0;
    if (i < N) {
      const double ti = t[i];
      if (track[i] < 0) c = 1;
      else if (!(lm_finite32(x[i]) && lm_finite32(y[i]) && interp_finite(ti))) c = 2;
      else if (!extrapolate && !(ti >= t_lo && ti <= t_hi)) c = 3;
      else c = 4;
      key[i] = c == 4 ? lm_time_key(ti) : LM_NONE;
      iota[i] = (int32_t)i;
    }
    n1 += ramp_wave_count(c == 1);
    n2 += ramp_wave_count(c == 2);
    n3 += ramp_wave_count(c == 3);
    n4 += ramp_wave_count(c == 4);
  }
  if (__ballot(bad) != 0 && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(&ctr[0], RAMP_INTERP_BAD_TIMES);
  ramp_wave_flush(ctr + 1, tid, n1, n2, n3, n4);
}

__global__ void __launch_bounds__(INTERP_THREADS)
    lm_id_kernel(const lm_u64 *__restrict__ skey, const int32_t *__restrict__ sidx, const int64_t *__restrict__ track, int N,
                 const int32_t *__restrict__ ctr, lm_u64 *__restrict__ key2) {
  const bool failed = (ctr[0] & RAMP_INTERP_BAD_TIMES) != 0;
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + threadIdx.x;
    if (pos >= (long)N) continue;
    key2[pos] = (failed || skey[pos] == LM_NONE) ? LM_NONE : (lm_u64)track[sidx[pos]];
  }
}

__global__ void __launch_bounds__(INTERP_THREADS) lm_head_kernel(const lm_u64 *__restrict__ skey, int N, int32_t *__restrict__ head) {
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + threadIdx.x;
    if (pos >= (long)N) continue;
    const lm_u64 k = skey[pos];
    head[pos] = (k != LM_NONE && (pos == 0 || skey[pos - 1] != k)) ? 1 : 0;
  }
}

struct LmRayArgs {
  const float *x, *y;
  const double *t;
  const float *knots;
  const double *times;
  const float *seg, *intrinsics;
  const lm_u64 *skey;
  const int32_t *sidx, *head, *ex;
  float *ray;
  int32_t *seg_start;
  int64_t *lm_track;
  int32_t *count, *ev_landmark;
  float *ev_residual, *ev_ray;
  int32_t *status, *ctr;
  long max_landmarks;
  int N, T, extrapolate;
};

template <bool LDS_TIMES>
__global__ void __launch_bounds__(INTERP_THREADS) lm_ray_kernel(const LmRayArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_smem[];
  double *s_times = reinterpret_cast<double *>(lm_smem);
  const int tid = threadIdx.x;
  const int N = a.N, T = a.T;
  if (LDS_TIMES) {
    for (int i = tid; i < T; i += INTERP_THREADS) s_times[i] = a.times[i];
    __syncthreads();
  }
  const bool failed = (a.ctr[0] & RAMP_INTERP_BAD_TIMES) != 0;
  const float fx = a.intrinsics[0], fy = a.intrinsics[1], cx = a.intrinsics[2], cy = a.intrinsics[3];
  const int s_max = T > 1 ? T - 2 : 0;
  const float qnan = __int_as_float(0x7fc00000);
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + tid;
    if (pos >= (long)N) continue;
    const lm_u64 k = a.skey[pos];
    const size_t i = (size_t)a.sidx[pos];
    const int hd = a.head[pos];
    const int l = a.ex[pos] + hd - 1;
    int32_t evl = -1;
    float r6[6] = {qnan, qnan, qnan, qnan, qnan, qnan};
    if (k != LM_NONE) {
      const float xe = a.x[i], ye = a.y[i];
      const double te = a.t[i];
      int s;
      double ts;
      if (LDS_TIMES) {
        s = min(max(interp_upper_bound(s_times, T, te) - 1, 0), s_max);
        ts = s_times[s];
      } else {
        s = min(max(interp_upper_bound(a.times, T, te) - 1, 0), s_max);
        ts = a.times[s];
      }
      const float4 *row4 = reinterpret_cast<const float4 *>(a.seg + (size_t)s * INTERP_SEG_WORDS);
      const float4 r0 = row4[0], r1 = row4[1];      // xi[0..3]; xi[4], xi[5], the length
      const float xi[6] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y};
      const double dt = __hiloint2double(__float_as_int(r1.w), __float_as_int(r1.z));
      const float alpha = interp_alpha(te, ts, dt, a.extrapolate);
      float X[7], C[7], d[3];
#pragma unroll
      for (int c = 0; c < 7; c++) X[c] = a.knots[7 * (size_t)s + c];
      interp_pose(X, xi, alpha, C);
      const float f[3] = {(xe - cx) / fx, (ye - cy) / fy, 1.0f};
      lt_qrot(C + 3, f, d);
      float *rec = a.ray + (size_t)pos * LM_RAY_WORDS;
      rec[0] = C[0]; rec[1] = C[1]; rec[2] = C[2];
      rec[3] = d[0]; rec[4] = d[1]; rec[5] = d[2];
      rec[6] = C[3]; rec[7] = C[4]; rec[8] = C[5]; rec[9] = C[6];
      rec[10] = xe; rec[11] = ye;
#pragma unroll
      for (int c = 0; c < 3; c++) { r6[c] = C[c]; r6[3 + c] = d[c]; }
      if (hd) {
        a.seg_start[l] = (int32_t)pos;
        if ((long)l < a.max_landmarks) a.lm_track[l] = (int64_t)k;
      }
      if ((long)l < a.max_landmarks) evl = l;
    }
    if (a.ev_landmark) a.ev_landmark[i] = evl;
    if (a.ev_residual) { a.ev_residual[2 * i] = qnan; a.ev_residual[2 * i + 1] = qnan; }
    if (a.ev_ray) {
#pragma unroll
      for (int c = 0; c < 6; c++) a.ev_ray[6 * i + c] = r6[c];
    }
    if (pos == (long)N - 1) {                            // the sorted list's end: the observations are the positions in front
      const int total = a.ex[pos] + hd;
      const int n_obs = failed ? 0 : a.ctr[4];
      const int kept = (long)total < a.max_landmarks ? total : (int)a.max_landmarks;
      a.seg_start[total] = n_obs;
      a.ctr[8] = kept;
      a.count[0] = kept;
      a.status[0] = a.ctr[0];
      a.status[1] = a.ctr[1];
      a.status[2] = a.ctr[2];
      a.status[3] = a.ctr[3];
      a.status[4] = n_obs;
      a.status[5] = total;
      a.status[6] = total - kept;
      a.status[7] = 0;                                   // (the solve launch adds the valid landmarks)
    }
  }
}

// ---- float64 from here on
struct LmChol {
  double l00, l10, l11, l20, l21, l22;
  bool ok;
};

static __device__ __forceinline__ bool lm_pivot_ok(double p) { return p > 0.0 && interp_finite(p); }

// a = (xx, xy, xz, yy, yz, zz)
static __device__ __forceinline__ LmChol lm_chol(const double *a) {
  LmChol c;
  c.ok = lm_pivot_ok(a[0]);
  c.l00 = sqrt(a[0]);
  c.l10 = a[1] / c.l00;
  c.l20 = a[2] / c.l00;
  const double p1 = a[3] - c.l10 * c.l10;
  c.ok = c.ok && lm_pivot_ok(p1);
  c.l11 = sqrt(p1);
  c.l21 = (a[4] - c.l20 * c.l10) / c.l11;
  const double p2 = (a[5] - c.l20 * c.l20) - c.l21 * c.l21;
  c.ok = c.ok && lm_pivot_ok(p2);
  c.l22 = sqrt(p2);
  return c;
}

static __device__ __forceinline__ void lm_chol_solve(const LmChol &c, const double *b, double *x) {
  const double y0 = b[0] / c.l00;
  const double y1 = (b[1] - c.l10 * y0) / c.l11;
  const double y2 = ((b[2] - c.l20 * y0) - c.l21 * y1) / c.l22;
  x[2] = y2 / c.l22;
  x[1] = (y1 - c.l21 * x[2]) / c.l11;
  x[0] = ((y0 - c.l10 * x[1]) - c.l20 * x[2]) / c.l00;
}

// lt_qrot's statements in float64: uv = 2 q x p, (p + w uv) + q x uv
static __device__ __forceinline__ void lm_qrot(const double *q, const double *p, double *o) {
  double uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  uv[0] = 2.0 * uv[0];
  uv[1] = 2.0 * uv[1];
  uv[2] = 2.0 * uv[2];
  o[0] = (p[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
  o[1] = (p[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
  o[2] = (p[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}

static __device__ __forceinline__ void lm_unit(const float *d, double *u) {
  const double x = (double)d[0], y = (double)d[1], z = (double)d[2];
  const double n = sqrt((x * x + y * y) + z * z);
  u[0] = x / n;
  u[1] = y / n;
  u[2] = z / n;
}

static __device__ __forceinline__ double lm_wave_max(double v) {
#pragma unroll
  for (int off = RAMP_WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

static __device__ __forceinline__ bool lm_finite3(const double *v) { return interp_finite(v[0]) && interp_finite(v[1]) && interp_finite(v[2]); }

struct LmSolveArgs {
  const float *ray;
  const int32_t *seg_start, *sidx;
  const double *t;
  const float *intrinsics;
  const int32_t *ctr;
  float *point, *cov, *rms, *parallax, *ev_residual;
  double *span;
  int32_t *n_obs, *status;
  uint8_t *cls;
  int min_obs, refine;
  float min_parallax, max_rms, sigma_px;
};

__global__ void __launch_bounds__(INTERP_THREADS) lm_solve_kernel(const LmSolveArgs a) {
  const int lane = threadIdx.x & (RAMP_WAVE - 1);
  const int wave = (int)((blockIdx.x * (unsigned)INTERP_THREADS + threadIdx.x) / RAMP_WAVE);
  const int waves = (int)(gridDim.x * (unsigned)INTERP_THREADS / RAMP_WAVE);
  const int count = a.ctr[8];
  const double fx = (double)a.intrinsics[0], fy = (double)a.intrinsics[1], cx = (double)a.intrinsics[2], cy = (double)a.intrinsics[3];
  const double nan = lm_nan();
  const float qnan = __int_as_float(0x7fc00000);
  int n_valid = 0;                                         // wave-uniform
  for (int l = wave; l < count; l += waves) {
    const int p0 = a.seg_start[l], p1 = a.seg_start[l + 1], n = p1 - p0;
    const float *first = a.ray + (size_t)p0 * LM_RAY_WORDS;
    const double c0[3] = {(double)first[0], (double)first[1], (double)first[2]};
    double u1[3];
    lm_unit(first + 3, u1);
    // 1. the midpoint system and the parallax
    double S[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double par = 0.0;
    for (int j = p0 + lane; j < p1; j += RAMP_WAVE) {
      const float *r = a.ray + (size_t)j * LM_RAY_WORDS;
      double u[3];
      lm_unit(r + 3, u);
      const double v[3] = {(double)r[0] - c0[0], (double)r[1] - c0[1], (double)r[2] - c0[2]};
      const double m00 = 1.0 - u[0] * u[0], m01 = -(u[0] * u[1]), m02 = -(u[0] * u[2]);
      const double m11 = 1.0 - u[1] * u[1], m12 = -(u[1] * u[2]), m22 = 1.0 - u[2] * u[2];
      S[0] += m00; S[1] += m01; S[2] += m02; S[3] += m11; S[4] += m12; S[5] += m22;
      S[6] += (m00 * v[0] + m01 * v[1]) + m02 * v[2];
      S[7] += (m01 * v[0] + m11 * v[1]) + m12 * v[2];
      S[8] += (m02 * v[0] + m12 * v[1]) + m22 * v[2];
      const double dot = (u[0] * u1[0] + u[1] * u1[1]) + u[2] * u1[2];
      par = fmax(par, acos(fmin(fmax(dot, -1.0), 1.0)));
    }
#pragma unroll
    for (int c = 0; c < 9; c++) S[c] = ramp_wave_sum(S[c]);
    par = lm_wave_max(par);
    const LmChol lin = lm_chol(S);
    double X[3] = {nan, nan, nan}, cov[6] = {nan, nan, nan, nan, nan, nan}, rms = nan;
    bool zbad = false;
    if (lin.ok) {                                          // (wave-uniform: every lane holds the same sums)
      double sol[3];
      lm_chol_solve(lin, S + 6, sol);
      X[0] = c0[0] + sol[0]; X[1] = c0[1] + sol[1]; X[2] = c0[2] + sol[2];
      // 2., 3. `refine` steps, then the last pass at the final X
      for (int pass = 0; pass <= a.refine; pass++) {
        const bool last = pass == a.refine;
#pragma unroll
        for (int c = 0; c < 10; c++) S[c] = 0.0;
        bool zb = false;
        for (int j = p0 + lane; j < p1; j += RAMP_WAVE) {
          const float *r = a.ray + (size_t)j * LM_RAY_WORDS;
          const double q0 = (double)r[6], q1 = (double)r[7], q2 = (double)r[8], q3 = (double)r[9];
          const double qn = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
          const double q[4] = {q0 / qn, q1 / qn, q2 / qn, q3 / qn}, qc[4] = {-q[0], -q[1], -q[2], q[3]};
          const double v[3] = {X[0] - (double)r[0], X[1] - (double)r[1], X[2] - (double)r[2]};
          double Y[3], j0[3], j1[3];
          lm_qrot(qc, v, Y);
          const double xn = Y[0] / Y[2], yn = Y[1] / Y[2];
          const double rx = (fx * xn + cx) - (double)r[10], ry = (fy * yn + cy) - (double)r[11];
          const double a0[3] = {fx / Y[2], 0.0, -(fx * xn) / Y[2]}, a1[3] = {0.0, fy / Y[2], -(fy * yn) / Y[2]};
          lm_qrot(q, a0, j0);
          lm_qrot(q, a1, j1);
          S[0] += j0[0] * j0[0] + j1[0] * j1[0];
          S[1] += j0[0] * j0[1] + j1[0] * j1[1];
          S[2] += j0[0] * j0[2] + j1[0] * j1[2];
          S[3] += j0[1] * j0[1] + j1[1] * j1[1];
          S[4] += j0[1] * j0[2] + j1[1] * j1[2];
          S[5] += j0[2] * j0[2] + j1[2] * j1[2];
          S[6] += j0[0] * rx + j1[0] * ry;
          S[7] += j0[1] * rx + j1[1] * ry;
          S[8] += j0[2] * rx + j1[2] * ry;
          S[9] += rx * rx + ry * ry;
          zb = zb || !(Y[2] > (double)RAMP_WARP_MIN_Z);
          if (last && a.ev_residual) {
            const size_t i = (size_t)a.sidx[j];
            a.ev_residual[2 * i] = (float)rx;
            a.ev_residual[2 * i + 1] = (float)ry;
          }
        }
#pragma unroll
        for (int c = 0; c < 10; c++) S[c] = ramp_wave_sum(S[c]);
        const LmChol ch = lm_chol(S);
        if (!last) {
          double step[3];
          lm_chol_solve(ch, S + 6, step);
          const double Xn[3] = {X[0] - step[0], X[1] - step[1], X[2] - step[2]};
          if (ch.ok && lm_finite3(Xn)) { X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2]; }
        } else {
          zbad = __ballot(zb) != 0;
          rms = sqrt(S[9] / (double)n);
          const double s2 = (double)a.sigma_px * (double)a.sigma_px;
          double col[3];
          const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
          if (ch.ok) {
            lm_chol_solve(ch, e0, col);
            cov[0] = s2 * col[0];
            lm_chol_solve(ch, e1, col);
            cov[1] = s2 * col[0]; cov[3] = s2 * col[1];
            lm_chol_solve(ch, e2, col);
            cov[2] = s2 * col[0]; cov[4] = s2 * col[1]; cov[5] = s2 * col[2];
          }
        }
      }
    }
    const float parf = (float)par, rmsf = (float)rms;
    float pf[3] = {(float)X[0], (float)X[1], (float)X[2]}, cf[6];
    bool fin = lm_finite32(pf[0]) && lm_finite32(pf[1]) && lm_finite32(pf[2]);
#pragma unroll
    for (int c = 0; c < 6; c++) { cf[c] = (float)cov[c]; fin = fin && lm_finite32(cf[c]); }
    int cls;
    if (n < a.min_obs) cls = 1;
    else if (par < (double)a.min_parallax) cls = 2;
    else if (!lin.ok) cls = 3;
    else if (zbad) cls = 4;
    else if (rms > (double)a.max_rms) cls = 5;
    else if (!fin) cls = 6;
    else cls = 7;
    n_valid += cls == 7;
    if (lane == 0) {
      const size_t L = (size_t)l;
#pragma unroll
      for (int c = 0; c < 3; c++) a.point[3 * L + c] = cls == 7 ? pf[c] : qnan;
#pragma unroll
      for (int c = 0; c < 6; c++) a.cov[6 * L + c] = cls == 7 ? cf[c] : qnan;
      a.n_obs[L] = n;
      a.cls[L] = (uint8_t)cls;
      a.rms[L] = rmsf;
      a.parallax[L] = parf;
      a.span[2 * L] = a.t[a.sidx[p0]];
      a.span[2 * L + 1] = a.t[a.sidx[p1 - 1]];
    }
  }
  if (lane == 0 && n_valid) atomicAdd(&a.status[7], n_valid);
}

// the workspace: the segment table (the head, as the warp's), the counters, the two key and the two index arrays, the head
// flags, their sum, the landmarks' first positions, the records, the library's own
struct LmWs {
  float *seg, *ray;
  int32_t *ctr, *idx_a, *idx_b, *head, *ex, *seg_start;
  lm_u64 *key_a, *key_b;
  void *cub;
  size_t cub_bytes;
};

static size_t lm_cub_bytes(int n) {
  size_t b = 0;
  int32_t *v = nullptr;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, v, v, n, (hipStream_t)0);
  const size_t a = ws_cub_bytes<lm_u64>(n, 64);
  b = round_up(b + 256, 256);
  return a > b ? a : b;
}

static size_t lm_carve(void *ws, long N, int T, LmWs *w) {
  WsCarver c(ws, interp_carve(ws, T, &w->seg));
  const size_t n = (size_t)(N > 0 ? N : 1);
  (void)c.take<char>(0, 256);
  w->ctr = c.take<int32_t>(LM_CTR_WORDS, 256);
  w->key_a = c.take<lm_u64>(n, 256);
  w->key_b = c.take<lm_u64>(n, 256);
  w->idx_a = c.take<int32_t>(n, 256);
  w->idx_b = c.take<int32_t>(n, 256);
  w->head = c.take<int32_t>(n, 256);
  w->ex = c.take<int32_t>(n, 256);
  w->seg_start = c.take<int32_t>(n + 1, 256);
  w->ray = c.take<float>(n * LM_RAY_WORDS, 256);
  w->cub_bytes = lm_cub_bytes((int)n);
  w->cub = c.take<char>(w->cub_bytes, 256);
  return c.bytes();
}

static bool lm_param_ok(float v) { return v >= 0.0f && v <= 3.4028234663852886e38f; }

extern "C" {
size_t ramp_event_landmarks_ws_bytes(long N, int T, long max_landmarks) {
  if (N < 0 || N > 2147483647L || T < 1 || max_landmarks < 1) return 0;
  LmWs w;
  return lm_carve(nullptr, N, T, &w);
}

long ramp_event_landmarks_grid_events(void) { return (long)LM_MAX_GROUPS * INTERP_THREADS; }

int ramp_event_landmarks(const float *x, const float *y, const double *t, const int64_t *track, long N, const float *knots,
                         const double *times, int T, const float *intrinsics, int flags, int min_obs, int refine,
                         float min_parallax, float max_rms, float sigma_px, long max_landmarks, int64_t *lm_track, float *point,
                         float *cov, int32_t *n_obs, uint8_t *cls, float *rms, float *parallax, double *span, int32_t *count,
                         int32_t *ev_landmark, float *ev_residual, float *ev_ray, int32_t *status, void *ws, size_t ws_bytes,
                         void *stream) {
  if (N < 0 || T < 1 || (flags & ~RAMP_INTERP_EXTRAPOLATE)) return RAMP_EINVAL;
  if (min_obs < 2 || refine < 0 || refine > 4 || max_landmarks < 1) return RAMP_EINVAL;
  if (!lm_param_ok(min_parallax) || !lm_param_ok(max_rms) || !lm_param_ok(sigma_px)) return RAMP_EINVAL;
  if (!lm_track || !point || !cov || !n_obs || !cls || !rms || !parallax || !span || !count || !status) return RAMP_EINVAL;
  if (N > 0 && (!x || !y || !t || !track || !knots || !times || !intrinsics || !ws)) return RAMP_EINVAL;
  if ((((uintptr_t)lm_track | (uintptr_t)span | (uintptr_t)t | (uintptr_t)track | (uintptr_t)times) & 7) != 0 ||
      (((uintptr_t)x | (uintptr_t)y | (uintptr_t)knots | (uintptr_t)intrinsics | (uintptr_t)point | (uintptr_t)cov |
        (uintptr_t)n_obs | (uintptr_t)rms | (uintptr_t)parallax | (uintptr_t)count | (uintptr_t)ev_landmark |
        (uintptr_t)ev_residual | (uintptr_t)ev_ray | (uintptr_t)status) & 3) != 0 ||
      ((uintptr_t)ws & 15) != 0)
    return RAMP_EINVAL;
  if (N > 2147483647L) return RAMP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {                                            // no launch: two memsets
    if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    return RAMP_OK;
  }
  LmWs w;
  if (ws_bytes < lm_carve(ws, N, T, &w)) return RAMP_EWORKSPACE;
  const int n = (int)N;
  const int ex = (flags & RAMP_INTERP_EXTRAPOLATE) ? 1 : 0;
  const long S = T > 1 ? T - 1 : 1;
  if (hipMemsetAsync(w.ctr, 0, LM_CTR_WORDS * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  hipLaunchKernelGGL(lm_key_kernel, dim3(lm_grid(N > S ? N : S)), dim3(INTERP_THREADS), 0, st, x, y, t, track, N, knots, times, T,
                     ex, w.seg, w.key_a, w.idx_a, w.ctr);
  RAMP_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.key_a, w.key_b, w.idx_a, w.idx_b, n, 0, 64, st) != hipSuccess) return RAMP_ELAUNCH;
  hipLaunchKernelGGL(lm_id_kernel, dim3(lm_grid(N)), dim3(INTERP_THREADS), 0, st, w.key_b, w.idx_b, track, n, w.ctr, w.key_a);
  RAMP_CHECK_LAUNCH();
  cb = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.key_a, w.key_b, w.idx_b, w.idx_a, n, 0, 64, st) != hipSuccess) return RAMP_ELAUNCH;
  hipLaunchKernelGGL(lm_head_kernel, dim3(lm_grid(N)), dim3(INTERP_THREADS), 0, st, w.key_b, n, w.head);
  RAMP_CHECK_LAUNCH();
  cb = w.cub_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(w.cub, cb, w.head, w.ex, n, st) != hipSuccess) return RAMP_ELAUNCH;
  LmRayArgs r;
  r.x = x; r.y = y; r.t = t; r.knots = knots; r.times = times; r.seg = w.seg; r.intrinsics = intrinsics; r.skey = w.key_b;
  r.sidx = w.idx_a; r.head = w.head; r.ex = w.ex; r.ray = w.ray; r.seg_start = w.seg_start; r.lm_track = lm_track;
  r.count = count; r.ev_landmark = ev_landmark; r.ev_residual = ev_residual; r.ev_ray = ev_ray; r.status = status; r.ctr = w.ctr;
  r.max_landmarks = max_landmarks; r.N = n; r.T = T; r.extrapolate = ex;
  static_assert((size_t)INTERP_LDS_KNOTS * sizeof(double) <= 64 * 1024, "LDS within the default limit: the launch needs no hipFuncSetAttribute");
  if (T <= INTERP_LDS_KNOTS)
    hipLaunchKernelGGL((lm_ray_kernel<true>), dim3(lm_grid(N)), dim3(INTERP_THREADS), (size_t)T * sizeof(double), st, r);
  else
    hipLaunchKernelGGL((lm_ray_kernel<false>), dim3(lm_grid(N)), dim3(INTERP_THREADS), 0, st, r);
  RAMP_CHECK_LAUNCH();
  LmSolveArgs s;
  s.ray = w.ray; s.seg_start = w.seg_start; s.sidx = w.idx_a; s.t = t; s.intrinsics = intrinsics; s.ctr = w.ctr; s.point = point;
  s.cov = cov; s.rms = rms; s.parallax = parallax; s.ev_residual = ev_residual; s.span = span; s.n_obs = n_obs; s.status = status;
  s.cls = cls; s.min_obs = min_obs; s.refine = refine; s.min_parallax = min_parallax; s.max_rms = max_rms; s.sigma_px = sigma_px;
  const long bound = N < max_landmarks ? N : max_landmarks;               // the landmarks' bound: one wave each
  hipLaunchKernelGGL(lm_solve_kernel, dim3(lm_grid(bound * RAMP_WAVE)), dim3(INTERP_THREADS), 0, st, s);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
