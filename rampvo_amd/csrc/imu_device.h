// What the IMU kernels share (imu.hip: preintegration and alignment; imu_propagate.hip: the forward pass): float64 quaternions,
// the preintegration element and its associative law, and the host's tests of the extrinsics.  ONE text of the arithmetic for
// both element types: ImuElem carries d dR / d bias_g (20 words), ImuProp does not (11 words).  No FMA contraction.
#ifndef RAMP_IMU_DEVICE_H
#define RAMP_IMU_DEVICE_H
#include "ramp_internal.h"
#include "interp_device.h"

#define IMU_SMALL 1e-4                     // theta^2 below which Exp and Jr use their series: no cancellation, no sin / cos

static __device__ __forceinline__ double imu_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---------------------------------------------------------------------------------------------- quaternions xyzw, float64
static __device__ __forceinline__ void imu_qmul(const double *a, const double *b, double *o) {
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
// q p q^-1; sgn = -1: the inverse rotation
static __device__ __forceinline__ void imu_qrot(const double *q, double sgn, const double *p, double *o) {
  const double x = sgn * q[0], y = sgn * q[1], z = sgn * q[2];
  double uv[3] = {y * p[2] - z * p[1], z * p[0] - x * p[2], x * p[1] - y * p[0]};
  uv[0] += uv[0];
  uv[1] += uv[1];
  uv[2] += uv[2];
  o[0] = p[0] + q[3] * uv[0] + (y * uv[2] - z * uv[1]);
  o[1] = p[1] + q[3] * uv[1] + (z * uv[0] - x * uv[2]);
  o[2] = p[2] + q[3] * uv[2] + (x * uv[1] - y * uv[0]);
}
static __device__ __forceinline__ void imu_qnorm(double *q) {
  const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
static __device__ __forceinline__ void imu_qlog(const double *q, double *phi) {
  const double sg = q[3] < 0.0 ? -1.0 : 1.0;
  const double x = sg * q[0], y = sg * q[1], z = sg * q[2], w = sg * q[3];
  const double n = sqrt(x * x + y * y + z * z);
  const double k = n > 0.0 ? 2.0 * atan2(n, w) / n : 2.0 / w;
  phi[0] = k * x; phi[1] = k * y; phi[2] = k * z;
}

// ---------------------------------------------------------------------------------------------- elements
struct ImuElem {
  static constexpr bool HAS_J = true;
  double q[4], v[3], p[3], t, J[9];
};
struct ImuProp {                           // the element of the forward pass: J is not carried
  static constexpr bool HAS_J = false;
  double q[4], v[3], p[3], t;
};
#define IMU_PROP_WORDS 11

template <typename E>
static __device__ __forceinline__ void imu_identity(E &e) {
  e.q[0] = e.q[1] = e.q[2] = 0.0; e.q[3] = 1.0;
#pragma unroll
  for (int c = 0; c < 3; c++) { e.v[c] = 0.0; e.p[c] = 0.0; }
  e.t = 0.0;
  if constexpr (E::HAS_J) {
#pragma unroll
    for (int c = 0; c < 9; c++) e.J[c] = 0.0;
  }
}

// (Exp(w dt), a dt, 1/2 a dt^2, dt, -Jr(w dt) dt)
template <typename E>
static __device__ __forceinline__ void imu_element(const double *w, const double *a, double dt, E &e) {
  const double phi[3] = {w[0] * dt, w[1] * dt, w[2] * dt};
  const double x = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  double imag, real, b = 0.0, c = 0.0;
  if (x < IMU_SMALL) {
    imag = 0.5 * (1.0 - x / 24.0 * (1.0 - x / 80.0 * (1.0 - x / 168.0 * (1.0 - x / 288.0))));
    real = 1.0 - x / 8.0 * (1.0 - x / 48.0 * (1.0 - x / 120.0 * (1.0 - x / 224.0)));
    if constexpr (E::HAS_J) {
      b = 0.5 * (1.0 - x / 12.0 * (1.0 - x / 30.0 * (1.0 - x / 56.0 * (1.0 - x / 90.0))));
      c = (1.0 - x / 20.0 * (1.0 - x / 42.0 * (1.0 - x / 72.0 * (1.0 - x / 110.0)))) / 6.0;
    }
  } else {
    const double th = sqrt(x), h = sin(0.5 * th);
    imag = h / th;
    real = cos(0.5 * th);
    if constexpr (E::HAS_J) {
      b = 2.0 * h * h / x;
      c = (th - sin(th)) / (x * th);
    }
  }
  e.q[0] = imag * phi[0]; e.q[1] = imag * phi[1]; e.q[2] = imag * phi[2]; e.q[3] = real;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    e.v[i] = a[i] * dt;
    e.p[i] = e.v[i] * (dt / 2.0);
  }
  e.t = dt;
  if constexpr (E::HAS_J) {
    // Jr = I - b [phi]x + c [phi]x^2,  [phi]x^2 = phi phi^T - |phi|^2 I
    const double K[9] = {0.0, -phi[2], phi[1], phi[2], 0.0, -phi[0], -phi[1], phi[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double k2 = phi[i] * phi[j] - (i == j ? x : 0.0);
        e.J[3 * i + j] = -(((i == j ? 1.0 : 0.0) - b * K[3 * i + j]) + c * k2) * dt;
      }
  }
}

// A o B = (R1 R2, v1 + R1 v2, p1 + v1 t2 + R1 p2, t1 + t2, R2^T J1 + J2) into A
template <typename E>
static __device__ __forceinline__ void imu_compose(E &A, const E &B) {
  double q[4], r[3], s[3];
  imu_qmul(A.q, B.q, q);
  imu_qrot(A.q, 1.0, B.v, r);
  imu_qrot(A.q, 1.0, B.p, s);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    A.p[c] = (A.p[c] + A.v[c] * B.t) + s[c];
    A.v[c] = A.v[c] + r[c];
  }
  if constexpr (E::HAS_J) {
#pragma unroll
    for (int c = 0; c < 3; c++) {                          // the columns of J1
      const double col[3] = {A.J[c], A.J[3 + c], A.J[6 + c]};
      double o[3];
      imu_qrot(B.q, -1.0, col, o);
      A.J[c] = o[0] + B.J[c];
      A.J[3 + c] = o[1] + B.J[3 + c];
      A.J[6 + c] = o[2] + B.J[6 + c];
    }
  }
  A.t = A.t + B.t;
#pragma unroll
  for (int c = 0; c < 4; c++) A.q[c] = q[c];
}

// ---------------------------------------------------------------------------------------------- host: the extrinsics
static inline bool imu_host_finite(double v) { return v == v && v - v == 0.0; }

// R [3][3] row-major -> unit quaternion xyzw (Shepperd: the largest of the four squares is the pivot)
static inline void imu_quat_from_R(const double *R, double *q) {
  const double t[4] = {R[0], R[4], R[8], R[0] + R[4] + R[8]};
  int i = 0;
  for (int c = 1; c < 4; c++)
    if (t[c] > t[i]) i = c;
  if (i == 3) {
    const double w = sqrt(1.0 + t[3]) / 2.0;
    q[0] = (R[7] - R[5]) / (4.0 * w); q[1] = (R[2] - R[6]) / (4.0 * w); q[2] = (R[3] - R[1]) / (4.0 * w); q[3] = w;
  } else {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    const double x = sqrt(1.0 + 2.0 * t[i] - t[3]) / 2.0;
    q[i] = x;
    q[j] = (R[3 * j + i] + R[3 * i + j]) / (4.0 * x);
    q[k] = (R[3 * k + i] + R[3 * i + k]) / (4.0 * x);
    q[3] = (R[3 * k + j] - R[3 * j + k]) / (4.0 * x);
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; c++) q[c] /= n;
}

// R [3][3] row-major is a rotation: every word of R R^T - I within RAMP_IMU_ROTATION_TOL and det R > 0
static inline bool imu_is_rotation(const double *R) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
      if (!(d <= RAMP_IMU_ROTATION_TOL && d >= -RAMP_IMU_ROTATION_TOL)) return false;
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  return det > 0.0;
}

// the host extrinsics [12] (NULL: identity) as the kernels take them: q_bc, and lever = -R_bc^T p_bc; false: refused
static inline bool imu_extrinsics(const double *extrinsics, double *q_bc, double *lever, double *p_bc) {
  static const double eye[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (extrinsics) {
    for (int c = 0; c < 12; c++)
      if (!imu_host_finite(extrinsics[c])) return false;
    if (!imu_is_rotation(extrinsics)) return false;
  }
  const double *X = extrinsics ? extrinsics : eye;
  imu_quat_from_R(X, q_bc);
  for (int c = 0; c < 3; c++) {
    lever[c] = -(X[c] * X[9] + X[3 + c] * X[10] + X[6 + c] * X[11]);
    if (p_bc) p_bc[c] = X[9 + c];
  }
  return true;
}
#endif
