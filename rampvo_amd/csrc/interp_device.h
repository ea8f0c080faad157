// What the pose query (interp.hip) and the event warp (warp.hip) share: the segment table of a trajectory and the place of
// a time stamp on it.  One definition, so that both evaluate the same geodesic with the same bits:
//
//   s     = largest index with times[s] <= t, clamped to [0, T - 2]
//   alpha = (t - times[s]) / (times[s + 1] - times[s])           float64, rounded to fp32 once
//   xi_s  = Log(X[s + 1] * X[s]^-1)                               the left increment, (translation 3, rotation 3)
//   X(t)  = Exp(alpha * xi_s) * X[s]
#pragma once
#include "ramp_device.h"
#include "workspace.h"

#define INTERP_THREADS 256
#define INTERP_LDS_KNOTS 4096      // knot times staged in LDS up to here (32 KiB of float64); longer: search in global memory
#define INTERP_MAX_GROUPS 2048     // workgroups per launch; each walks the query tiles with this stride
#define INTERP_SEG_WORDS 16        // per segment: xi[6], float64 length (words 6, 7), twist[6], 2 spare = one 64-byte row

// the segment table of T knots (one row for a single knot): ramp_se3_interp's whole workspace, the head of the warp's
static inline size_t interp_carve(void *ws, int T, float **seg) {
  WsCarver c(ws);
  *seg = c.take<float>((size_t)(T > 1 ? T - 1 : 1) * INTERP_SEG_WORDS, 1);
  return c.bytes();
}

static __device__ __forceinline__ bool interp_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// segment s of the table: its increment, twist and length; true when its time stamps fail the check
static __device__ __forceinline__ bool interp_segment_values(const float *__restrict__ knots, const double *__restrict__ times,
                                                             int T, int s, float *xi, float *tw, double *length) {
  const double t0 = times[s];
  bool bad = !interp_finite(t0);
  double dt = 0.0;
#pragma unroll
  for (int c = 0; c < 6; c++) { xi[c] = 0.0f; tw[c] = 0.0f; }
  if (T > 1) {
    const double t1 = times[s + 1];
    bad = bad || !interp_finite(t1) || t1 < t0;
    dt = t1 - t0;
    float X0[7], X1[7], X0i[7], D[7];
#pragma unroll
    for (int c = 0; c < 7; c++) { X0[c] = knots[7 * (size_t)s + c]; X1[c] = knots[7 * (size_t)(s + 1) + c]; }
    lt_inv(X0, X0i);
    lt_mul(X1, X0i, D);
    lt_log(D, xi);
    if (dt > 0.0) {
#pragma unroll
      for (int c = 0; c < 6; c++) tw[c] = (float)((double)xi[c] / dt);
    }
  }
  *length = dt;
  return bad;
}

// the same into the segment's 64-byte row of the table
static __device__ __forceinline__ bool interp_segment_row(const float *__restrict__ knots, const double *__restrict__ times,
                                                          int T, int s, float *__restrict__ row) {
  float xi[6], tw[6];
  double dt;
  const bool bad = interp_segment_values(knots, times, T, s, xi, tw, &dt);
#pragma unroll
  for (int c = 0; c < 6; c++) { row[c] = xi[c]; row[8 + c] = tw[c]; }
  *reinterpret_cast<double *>(row + 6) = dt;        // (rows are 64 bytes, the workspace 16-byte aligned: an aligned float64)
  row[14] = 0.0f;
  row[15] = 0.0f;
  return bad;
}

// upper bound: the number of knot times <= t (0 for a NaN)
template <typename P>
static __device__ __forceinline__ int interp_upper_bound(P tt, int T, double t) {
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tt[mid] <= t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the place of t on a segment that starts at ts and is dt long
static __device__ __forceinline__ float interp_alpha(double t, double ts, double dt, int extrapolate) {
  double a;
  if (dt > 0.0) {
    a = (t - ts) / dt;
    if (!extrapolate) a = fmin(fmax(a, 0.0), 1.0);
  } else {
    a = t < ts ? 0.0 : 1.0;                         // a segment of zero length (or a failed check of `times`)
  }
  return (float)a;
}

// Exp(alpha * xi) * X
static __device__ __forceinline__ void interp_pose(const float *X, const float *xi, float alpha, float *o) {
  float axi[6], E[7];
#pragma unroll
  for (int c = 0; c < 6; c++) axi[c] = alpha * xi[c];
  lt_exp(axi, E);
  lt_mul(E, X, o);
}
