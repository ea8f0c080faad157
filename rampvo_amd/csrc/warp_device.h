// What the event warp (warp.hip) and the event contrast (contrast.hip) share: the layout of the workspace's head, the relative
// pose G = C(t_ref)^-1 C(t), the per-event geometry from the staged event up to X' with its validity test, and one axis of
// the bilinear splat.  One definition, so that both warp an event with the same bits:
//
//   C(t)  = Exp(alpha * xi_s) * knots[s]                  the geodesic of ramp_se3_interp (interp_device.h), camera-to-world
//   G     = C(t_ref)^-1 * C(t)
//   X'    = R_G * ((x - cx) / fx, (y - cy) / fy, 1) + t_G * d         d: inverse depth (one float, or a map)
//   x'    = fx * (X' / Z') + cx,   y' = fy * (Y' / Z') + cy           invalid: Z' <= RAMP_WARP_MIN_Z, anything not finite
#pragma once
#include "interp_device.h"

#define WARP_TILE (INTERP_THREADS * 4)   // events per workgroup trip: a 16-byte load of x and y per lane
#define WARP_MAX_GROUPS 1024             // workgroups of the event launch; each walks the tiles with this stride
#define WARP_FIX_BITS 24
#define WARP_REF_WORDS 16                // C(t_ref)^-1: translation 3, quaternion 4, 9 spare = one 64-byte row
#define WARP_CTR_WORDS 16                // int32: the 8 status words, 8 spare
#define WARP_UNI_WORDS 12                // per workgroup in LDS: C(t_ref)^-1 (7), the intrinsics (4), the scalar inverse depth

typedef unsigned long long warp_u64;

// The warp's workspace, packed: seg, ref | ctr | acc_iwe | acc_stack | end.  The counters and the accumulators are adjacent
// because one memset clears them (from ctr up to the next block the call does not clear).  n_iwe, n_stack: the int64 words of
// the two accumulators; a call that leaves one out carves it with 0 words and the other moves up.  The contrast extends the
// layout at `end` (contrast.hip).
struct WarpWs {
  float *seg, *ref;
  int32_t *ctr;
  long long *acc_iwe, *acc_stack;
  char *end;
};
static inline size_t warp_carve(void *ws, int T, size_t n_iwe, size_t n_stack, WarpWs *w) {
  WsCarver c(ws, interp_carve(ws, T, &w->seg));
  w->ref = c.take<float>(WARP_REF_WORDS, 1);
  w->ctr = c.take<int32_t>(WARP_CTR_WORDS, 1);
  w->acc_iwe = c.take<long long>(n_iwe, 1);
  w->acc_stack = c.take<long long>(n_stack, 1);
  w->end = c.take<char>(0, 1);
  return c.bytes();
}

// G = Cref^-1 * C from ref = (-(qr^-1 . tr), qr^-1) and C = (t, q), without renormalising either factor:
//   q_G = normalise(qr^-1 * q),  t_G = qr^-1 . t - qr^-1 . tr
// Both rotations of a translation are the same function of their inputs, so C == Cref in every bit gives t_G = 0 exactly, and
// the quaternion product of q with its own conjugate has exactly zero imaginary parts: G is then the exact identity.
static __device__ __forceinline__ void warp_relative(const float *ref, const float *C, float *tG, float *qG) {
  float q[4], r[3];
  lt_qmul(ref + 3, C + 3, q);
  lt_qnorm(q, qG);
  lt_qrot(ref + 3, C, r);
  tG[0] = ref[0] + r[0];
  tG[1] = ref[1] + r[1];
  tG[2] = ref[2] + r[2];
}

// ref (WARP_REF_WORDS floats) = C(t_ref)^-1 as (-(qr^-1 . tr), qr^-1), zero padded: one lane forms C(t_ref) from its own copy of
// that segment's row (the same function as the table's, the same bits)
static __device__ __forceinline__ void warp_reference_row(const float *__restrict__ knots, const double *__restrict__ times, int T,
                                                          double t_ref, int extrapolate, float *__restrict__ ref) {
  const int s = min(max(interp_upper_bound(times, T, t_ref) - 1, 0), T > 1 ? T - 2 : 0);
  float xi[6], tw[6], X[7], C[7], r[3];
  double dt;
  interp_segment_values(knots, times, T, s, xi, tw, &dt);
#pragma unroll
  for (int c = 0; c < 7; c++) X[c] = knots[7 * (size_t)s + c];
  interp_pose(X, xi, interp_alpha(t_ref, times[s], dt, extrapolate), C);
  const float qi[4] = {-C[3], -C[4], -C[5], C[6]};
  lt_qrot(qi, C, r);
  ref[0] = -r[0]; ref[1] = -r[1]; ref[2] = -r[2];
  ref[3] = qi[0]; ref[4] = qi[1]; ref[5] = qi[2]; ref[6] = qi[3];
#pragma unroll
  for (int c = 7; c < WARP_REF_WORDS; c++) ref[c] = 0.0f;
}

// one axis of the splat: the two neighbours floor(v) and floor(v) + 1, their weights 1 - w and w with w = v - floor(v), and
// whether each lies in [0, n).  The range test is made in float, so a huge coordinate never reaches an integer conversion.
static __device__ __forceinline__ void warp_axis(float v, int n, int *i0, float *w0, float *w1, bool *in0, bool *in1) {
  const float fl = floorf(v);
  const float w = v - fl;
  *w0 = 1.0f - w;
  *w1 = w;
  *in0 = fl >= 0.0f && fl <= (float)(n - 1);
  *in1 = fl >= -1.0f && fl <= (float)(n - 2);
  *i0 = (*in0 || *in1) ? (int)fl : 0;
}

static __device__ __forceinline__ bool warp_event_finite(float x, float y, double t) {
  return fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && interp_finite(t);
}

// what the geometry of an event reads besides the event itself
struct WarpScene {
  const float *knots;
  const double *times;
  const float *seg, *invdepth;
  int T, H, W, extrapolate, depth_map;
};

// The geometry of one finite event (x, y, t), up to the two terms of X' = R + t_G * d: segment search, alpha in float64,
// C(t), G = C(t_ref)^-1 C(t), the depth sampled at the event's own rounded pixel, R = R_G ((x - cx) / fx, (y - cy) / fy, 1).
// s_times: the knot times (LDS with LDS_TIMES, else global); s_uni: WARP_UNI_WORDS floats; s_range: times[0], times[T - 1].
template <bool LDS_TIMES>
static __device__ __forceinline__ void warp_event_geometry(const WarpScene &a, float x, float y, double t, const double *s_times,
                                                           const float *s_uni, const double *s_range, bool *below, bool *above,
                                                           float *R, float *tG, float *depth) {
  const int T = a.T, H = a.H, W = a.W;
  const int s_max = T > 1 ? T - 2 : 0;
  *below = t < s_range[0];
  *above = t > s_range[1];
  int s;
  double ts;
  if (LDS_TIMES) {
    s = min(max(interp_upper_bound(s_times, T, t) - 1, 0), s_max);
    ts = s_times[s];
  } else {
    s = min(max(interp_upper_bound(a.times, T, t) - 1, 0), s_max);
    ts = a.times[s];
  }
  const float4 *row4 = reinterpret_cast<const float4 *>(a.seg + (size_t)s * INTERP_SEG_WORDS);
  const float4 r0 = row4[0], r1 = row4[1];      // xi[0..3]; xi[4], xi[5], the length
  const float xi[6] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y};
  const double dt = __hiloint2double(__float_as_int(r1.w), __float_as_int(r1.z));
  const float alpha = interp_alpha(t, ts, dt, a.extrapolate);
  float X[7], C[7], qG[4], ref[7];
  const float fx = s_uni[7], fy = s_uni[8], cx = s_uni[9], cy = s_uni[10];
#pragma unroll
  for (int c = 0; c < 7; c++) ref[c] = s_uni[c];
#pragma unroll
  for (int c = 0; c < 7; c++) X[c] = a.knots[7 * (size_t)s + c];
  interp_pose(X, xi, alpha, C);
  warp_relative(ref, C, tG, qG);
  float d = s_uni[11];
  if (a.depth_map) {                             // the event's rounded pixel (half to even), clamped to the image
    const int px = (int)fminf(fmaxf(rintf(x), 0.0f), (float)(W - 1));
    const int py = (int)fminf(fmaxf(rintf(y), 0.0f), (float)(H - 1));
    d = a.invdepth[(size_t)py * W + px];
  }
  *depth = d;
  const float P[3] = {(x - cx) / fx, (y - cy) / fy, 1.0f};
  lt_qrot(qG, P, R);
}

// x' = fx * (X' / Z') + cx, y' = fy * (Y' / Z') + cy and the validity test (a NaN Z' fails the comparison: rejected, like a
// NaN projection)
static __device__ __forceinline__ bool warp_project(float Xp, float Yp, float Zp, const float *s_uni, float *xp, float *yp) {
  const float fx = s_uni[7], fy = s_uni[8], cx = s_uni[9], cy = s_uni[10];
  *xp = fx * (Xp / Zp) + cx;
  *yp = fy * (Yp / Zp) + cy;
  return Zp > RAMP_WARP_MIN_Z && fabsf(*xp) <= 3.4028234663852886e38f && fabsf(*yp) <= 3.4028234663852886e38f;
}

// the contribution of one neighbour: its fp32 weight product in fixed point
static __device__ __forceinline__ long long warp_fixed_weight(float wx, float wy) {
  return __float2ll_rn(ldexpf(__fmul_rn(wx, wy), WARP_FIX_BITS));
}
