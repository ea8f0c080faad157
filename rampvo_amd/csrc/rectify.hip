// Lens distortion (include/ramp_hip.h: ramp_event_rectify, ramp_image_rectify): raw sensor events and frames to the pinhole
// camera every other event kernel models.  The camera record is RAMP_CAMERA_WORDS device floats (layout in the header).
//
//   forward (distort), (x, y) the normalised raw ray:
//     radtan        r2 = x^2 + y^2,  rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
//                   xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),   yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y
//     equidistant   r = sqrt(x^2 + y^2),  th = atan(r),  thd = th (1 + th^2 (k1 + th^2 (k2 + th^2 (k3 + th^2 k4))))
//                   (xd, yd) = (thd / r) (x, y),  r == 0: the identity
//   inverse (undistort), RAMP_RECTIFY_ITERS Newton steps, never fewer and never more:
//     radtan        2-D Newton with the analytic (symmetric) Jacobian, from (xd, yd)
//     equidistant   1-D Newton on th from thd = sqrt(xd^2 + yd^2), then (x, y) = (tan th / thd) (xd, yd)
//
// rect_event_kernel   one lane per event and trip: normalise, invert, rotate, project; the rows of a tile leave through LDS as
//                     full-width stores; integer counters by ballots, one atomic per wave and counter
// rect_image_kernel   one lane per output pixel and trip, all channels: ray, R^T, distort, bilinear sample in fp32 without FMA
//
// Every row (pixel) is a function of its own event (pixel) and the record alone: no reduction, no floating-point atomics, a
// fixed trip count.  Its bits depend neither on N, nor on its position, nor on the order of the events, nor on the launch shape.
#include "ramp_internal.h"
#include "interp_device.h"

#define RECT_MAX_GROUPS 2048             // workgroups per launch; each walks the tiles of INTERP_THREADS with this stride
#define RECT_FLT_MAX 3.4028234663852886e38f

static __device__ __forceinline__ bool rect_finite(float v) { return fabsf(v) <= RECT_FLT_MAX; }

// the camera record in registers (the loads are wave-uniform) and whether it can be used at all
struct RectCam {
  float fx, fy, cx, cy, k[5], R[9], nfx, nfy, ncx, ncy;
  int model;
  bool bad;
};

static __device__ __forceinline__ RectCam rect_load_camera(const float *__restrict__ cam) {
  RectCam c;
  bool fin = true;
#pragma unroll
  for (int i = 0; i < RAMP_CAMERA_WORDS; i++) fin = fin && rect_finite(cam[i]);
  c.fx = cam[RAMP_CAMERA_RAW + 0]; c.fy = cam[RAMP_CAMERA_RAW + 1]; c.cx = cam[RAMP_CAMERA_RAW + 2]; c.cy = cam[RAMP_CAMERA_RAW + 3];
#pragma unroll
  for (int i = 0; i < 5; i++) c.k[i] = cam[RAMP_CAMERA_COEFFS + i];
#pragma unroll
  for (int i = 0; i < 9; i++) c.R[i] = cam[RAMP_CAMERA_ROTATION + i];
  c.nfx = cam[RAMP_CAMERA_NEW + 0]; c.nfy = cam[RAMP_CAMERA_NEW + 1]; c.ncx = cam[RAMP_CAMERA_NEW + 2]; c.ncy = cam[RAMP_CAMERA_NEW + 3];
  const float m = cam[RAMP_CAMERA_MODEL];
  const bool known = m == (float)RAMP_CAM_PINHOLE || m == (float)RAMP_CAM_RADTAN || m == (float)RAMP_CAM_EQUIDISTANT;
  c.model = known ? (int)m : RAMP_CAM_PINHOLE;
  c.bad = !(fin && known && c.fx > 0.0f && c.fy > 0.0f && c.nfx > 0.0f && c.nfy > 0.0f);
  return c;
}

// radtan at (x, y): the distorted point and the Jacobian (J12 == J21)
static __device__ __forceinline__ void rect_radtan(const float *k, float x, float y, float *xd, float *yd, float *J11, float *J12,
                                                   float *J22) {
  const float k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  const float xx = x * x, yy = y * y, xy = x * y;
  const float r2 = xx + yy;
  const float rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
  const float drad = k1 + r2 * (2.0f * k2 + r2 * (3.0f * k3));           // d rad / d r2
  *xd = x * rad + 2.0f * p1 * xy + p2 * (r2 + 2.0f * xx);
  *yd = y * rad + p1 * (r2 + 2.0f * yy) + 2.0f * p2 * xy;
  *J11 = rad + 2.0f * xx * drad + 2.0f * p1 * y + 6.0f * p2 * x;
  *J12 = 2.0f * xy * drad + 2.0f * p1 * x + 2.0f * p2 * y;
  *J22 = rad + 2.0f * yy * drad + 6.0f * p1 * y + 2.0f * p2 * x;
}

// equidistant at the angle th: thd and d thd / d th
static __device__ __forceinline__ void rect_equi(const float *k, float th, float *thd, float *dthd) {
  const float t2 = th * th;
  *thd = th * (1.0f + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
  *dthd = 1.0f + t2 * (3.0f * k[0] + t2 * (5.0f * k[1] + t2 * (7.0f * k[2] + t2 * (9.0f * k[3]))));
}

// (xd, yd) -> (x, y); false: not invertible (an iterate that is not finite, a determinant that is not positive, a residual
// above RAMP_RECTIFY_TOL raw pixels)
static __device__ __forceinline__ bool rect_undistort(const RectCam &c, float xd, float yd, float *xo, float *yo) {
  if (c.model == RAMP_CAM_RADTAN) {
    float x = xd, y = yd, fx, fy, J11, J12, J22;
    bool ok = true;
#pragma unroll 1
    for (int it = 0; it < RAMP_RECTIFY_ITERS; it++) {
      rect_radtan(c.k, x, y, &fx, &fy, &J11, &J12, &J22);
      const float det = J11 * J22 - J12 * J12;
      const float ex = fx - xd, ey = fy - yd;
      ok = ok && det > 0.0f;
      x = x - (J22 * ex - J12 * ey) / det;
      y = y - (J11 * ey - J12 * ex) / det;
      ok = ok && rect_finite(x) && rect_finite(y);
    }
    rect_radtan(c.k, x, y, &fx, &fy, &J11, &J12, &J22);
    const float det = J11 * J22 - J12 * J12;
    const float ex = (fx - xd) * c.fx, ey = (fy - yd) * c.fy;
    ok = ok && det > 0.0f && ex * ex + ey * ey <= RAMP_RECTIFY_TOL * RAMP_RECTIFY_TOL;
    *xo = x;
    *yo = y;
    return ok;
  }
  if (c.model == RAMP_CAM_EQUIDISTANT) {
    const float thd = sqrtf(xd * xd + yd * yd);
    float th = thd, f, df;
    bool ok = true;
#pragma unroll 1
    for (int it = 0; it < RAMP_RECTIFY_ITERS; it++) {
      rect_equi(c.k, th, &f, &df);
      ok = ok && df > 0.0f;
      th = th - (f - thd) / df;
      ok = ok && rect_finite(th);
    }
    rect_equi(c.k, th, &f, &df);
    const float e = fabsf(f - thd) * fmaxf(c.fx, c.fy);
    ok = ok && df > 0.0f && e <= RAMP_RECTIFY_TOL && th >= 0.0f && th < 1.57079632679489662f;
    const float s = thd > 0.0f ? tanf(ok ? th : 0.0f) / thd : 1.0f;
    *xo = s * xd;
    *yo = s * yd;
    return ok;
  }
  *xo = xd;
  *yo = yd;
  return true;
}

// (x, y) -> (xd, yd); false: the model's Jacobian determinant at the ray is not positive
static __device__ __forceinline__ bool rect_distort(const RectCam &c, float x, float y, float *xd, float *yd) {
  if (c.model == RAMP_CAM_RADTAN) {
    float J11, J12, J22;
    rect_radtan(c.k, x, y, xd, yd, &J11, &J12, &J22);
    return J11 * J22 - J12 * J12 > 0.0f;
  }
  if (c.model == RAMP_CAM_EQUIDISTANT) {
    const float r = sqrtf(x * x + y * y);
    float thd, df;
    rect_equi(c.k, atanf(r), &thd, &df);
    const float s = r > 0.0f ? thd / r : 1.0f;
    *xd = s * x;
    *yd = s * y;
    return df > 0.0f;
  }
  *xd = x;
  *yd = y;
  return true;
}

// I32: x, y are int32 pixels.  VEC: xy_out is 16-byte aligned, a full tile leaves as one 16-byte store per lane of its first half
template <bool I32, bool VEC>
__global__ void __launch_bounds__(INTERP_THREADS)
    rect_event_kernel(const void *__restrict__ xv, const void *__restrict__ yv, long N, const float *__restrict__ cam, int H, int W,
                      float *__restrict__ xy_out, unsigned char *__restrict__ valid_out, int32_t *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) float s_rows[INTERP_THREADS * 2];
  const int tid = threadIdx.x;
  const RectCam c = rect_load_camera(cam);
  const float qnan = __int_as_float(0x7fc00000);
  const long tiles = (N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n_seen = 0, n_nan = 0, n_inv = 0, n_behind = 0, n_out = 0, n_in = 0;          // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long base = tile * INTERP_THREADS;
    const long i = base + tid;
    const bool have = i < N;
    bool not_finite = false, not_inv = false, behind = false, outside = false, inside = false;
    float ox = qnan, oy = qnan;
    if (have) {
      float x, y;
      if (I32) {
        x = (float)static_cast<const int32_t *>(xv)[i];
        y = (float)static_cast<const int32_t *>(yv)[i];
      } else {
        x = static_cast<const float *>(xv)[i];
        y = static_cast<const float *>(yv)[i];
      }
      if (!(rect_finite(x) && rect_finite(y))) {
        not_finite = true;
      } else if (c.bad) {
        not_inv = true;                              // (no usable camera: nothing can be inverted)
      } else {
        const float xd = (x - c.cx) / c.fx, yd = (y - c.cy) / c.fy;
        float ux, uy;
        if (!rect_undistort(c, xd, yd, &ux, &uy)) {
          not_inv = true;
        } else {
          const float X = c.R[0] * ux + c.R[1] * uy + c.R[2];
          const float Y = c.R[3] * ux + c.R[4] * uy + c.R[5];
          const float Z = c.R[6] * ux + c.R[7] * uy + c.R[8];
          const float px = c.nfx * (X / Z) + c.ncx, py = c.nfy * (Y / Z) + c.ncy;
          if (!(Z > 0.0f) || !rect_finite(px) || !rect_finite(py)) {
            behind = true;
          } else {
            ox = px;
            oy = py;
            inside = px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1);
            outside = !inside;
          }
        }
      }
      if (valid_out) valid_out[i] = (inside || outside) ? 1 : 0;
    }
    const int live = (int)min((long)INTERP_THREADS, N - base);             // rows of this tile, >= 1
    if (tid < live) {
      s_rows[2 * tid] = ox;
      s_rows[2 * tid + 1] = oy;
    }
    __syncthreads();
    float *og = xy_out + (size_t)base * 2;
    if (VEC && live == INTERP_THREADS) {
      if (tid < INTERP_THREADS / 2) reinterpret_cast<float4 *>(og)[tid] = reinterpret_cast<const float4 *>(s_rows)[tid];
    } else {
      for (int j = tid; j < live * 2; j += INTERP_THREADS) og[j] = s_rows[j];
    }
    __syncthreads();                                 // (the next tile overwrites the staging rows)
    n_seen += ramp_wave_count(have);
    n_nan += ramp_wave_count(not_finite);
    n_inv += ramp_wave_count(not_inv);
    n_behind += ramp_wave_count(behind);
    n_out += ramp_wave_count(outside);
    n_in += ramp_wave_count(inside);
  }
  ramp_wave_flush(status + 1, tid, n_seen, n_nan, n_inv, n_behind, n_out, n_in);
  if (c.bad && blockIdx.x == 0 && tid == 0) atomicOr(&status[0], RAMP_RECTIFY_BAD_CAMERA);
}

// U8: the source is uint8, else fp32
template <bool U8>
__global__ void __launch_bounds__(INTERP_THREADS)
    rect_image_kernel(const void *__restrict__ srcv, int C, int Hs, int Ws, const float *__restrict__ cam, int H, int W, int norm,
                      float fill, float *__restrict__ out, float *__restrict__ map_out, unsigned char *__restrict__ mask_out,
                      int32_t *__restrict__ status) {
  const int tid = threadIdx.x;
  const RectCam c = rect_load_camera(cam);
  const float qnan = __int_as_float(0x7fc00000);
  const long P = (long)H * W, Ps = (long)Hs * Ws;
  const long tiles = (P + INTERP_THREADS - 1) / INTERP_THREADS;
  int n_seen = 0, n_fold = 0, n_out = 0, n_in = 0;   // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    const bool have = i < P;
    bool fold = false, outside = false, sampled = false;
    if (have) {
      const int v = (int)(i / W), u = (int)(i - (long)v * W);
      float xs = qnan, ys = qnan;
      if (c.bad) {
        fold = true;
      } else {
        // the ray of the rectified pixel in the raw camera: R^T ((u - cx') / fx', (v - cy') / fy', 1)
        const float rx = ((float)u - c.ncx) / c.nfx, ry = ((float)v - c.ncy) / c.nfy;
        const float X = c.R[0] * rx + c.R[3] * ry + c.R[6];
        const float Y = c.R[1] * rx + c.R[4] * ry + c.R[7];
        const float Z = c.R[2] * rx + c.R[5] * ry + c.R[8];
        const float x = X / Z, y = Y / Z;
        float xd, yd;
        const bool det_ok = rect_distort(c, x, y, &xd, &yd);
        xs = c.fx * xd + c.cx;
        ys = c.fy * yd + c.cy;
        if (!(Z > 0.0f) || !det_ok || !rect_finite(xs) || !rect_finite(ys)) fold = true;
        else if (!(xs >= 0.0f && xs <= (float)(Ws - 1) && ys >= 0.0f && ys <= (float)(Hs - 1))) outside = true;
        else sampled = true;
      }
      if (map_out) reinterpret_cast<float2 *>(map_out)[i] = sampled ? make_float2(xs, ys) : make_float2(qnan, qnan);
      if (mask_out) mask_out[i] = sampled ? 1 : 0;
      if (!sampled) {
        for (int ch = 0; ch < C; ch++) out[(size_t)ch * P + i] = fill;
      } else {
        // 0 <= xs <= Ws - 1: x0 is a column; a neighbour past the last column is clamped and its weight is exactly 0
        const float x0 = floorf(xs), y0 = floorf(ys);
        const float wx = xs - x0, wy = ys - y0;
        const float vx = 1.0f - wx, vy = 1.0f - wy;
        const int ix0 = (int)x0, iy0 = (int)y0;
        const int ix1 = min(ix0 + 1, Ws - 1), iy1 = min(iy0 + 1, Hs - 1);
        const size_t a00 = (size_t)iy0 * Ws + ix0, a01 = (size_t)iy0 * Ws + ix1, a10 = (size_t)iy1 * Ws + ix0,
                     a11 = (size_t)iy1 * Ws + ix1;
        for (int ch = 0; ch < C; ch++) {
          float a, b, cc, d;
          if (U8) {
            const unsigned char *s = static_cast<const unsigned char *>(srcv) + (size_t)ch * Ps;
            a = (float)s[a00]; b = (float)s[a01]; cc = (float)s[a10]; d = (float)s[a11];
          } else {
            const float *s = static_cast<const float *>(srcv) + (size_t)ch * Ps;
            a = s[a00]; b = s[a01]; cc = s[a10]; d = s[a11];
          }
          const float top = __fadd_rn(__fmul_rn(vx, a), __fmul_rn(wx, b));
          const float bot = __fadd_rn(__fmul_rn(vx, cc), __fmul_rn(wx, d));
          float val = __fadd_rn(__fmul_rn(vy, top), __fmul_rn(wy, bot));
          if (norm == RAMP_RECTIFY_NORM_HALF) val = __fsub_rn(__fmul_rn(2.0f, __fdiv_rn(val, 255.0f)), 0.5f);
          else if (norm == RAMP_RECTIFY_NORM_UNIT) val = __fsub_rn(__fmul_rn(2.0f, __fdiv_rn(val, 255.0f)), 1.0f);
          out[(size_t)ch * P + i] = val;
        }
      }
    }
    n_seen += ramp_wave_count(have);
    n_fold += ramp_wave_count(fold);
    n_out += ramp_wave_count(outside);
    n_in += ramp_wave_count(sampled);
  }
  ramp_wave_flush(status + 1, tid, n_seen, n_fold, n_out, n_in);
  if (c.bad && blockIdx.x == 0 && tid == 0) atomicOr(&status[0], RAMP_RECTIFY_BAD_CAMERA);
}

template <bool I32>
static void rect_launch_events(bool vec, int grid, hipStream_t st, const void *x, const void *y, long N, const float *cam, int H,
                               int W, float *xy_out, unsigned char *valid_out, int32_t *status) {
  if (vec) hipLaunchKernelGGL((rect_event_kernel<I32, true>), dim3(grid), dim3(INTERP_THREADS), 0, st, x, y, N, cam, H, W, xy_out,
                              valid_out, status);
  else hipLaunchKernelGGL((rect_event_kernel<I32, false>), dim3(grid), dim3(INTERP_THREADS), 0, st, x, y, N, cam, H, W, xy_out,
                          valid_out, status);
}

extern "C" {
long ramp_event_rectify_grid_events(void) { return (long)RECT_MAX_GROUPS * INTERP_THREADS; }

int ramp_event_rectify(const void *x, const void *y, long N, const float *camera, int flags, int H, int W, float *xy_out,
                       uint8_t *valid_out, int32_t *status, void *stream) {
  if (N < 0 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~RAMP_RECTIFY_XY_I32) return RAMP_EINVAL;
  if (N == 0) return RAMP_OK;
  if (!x || !y || !camera || !xy_out || !status) return RAMP_EINVAL;
  if (((uintptr_t)xy_out & 7) != 0 || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)camera | (uintptr_t)status) & 3) != 0)
    return RAMP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const long tiles = (N + INTERP_THREADS - 1) / INTERP_THREADS;
  const int grid = (int)(tiles < RECT_MAX_GROUPS ? tiles : RECT_MAX_GROUPS);
  const bool vec = ((uintptr_t)xy_out & 15) == 0;
  if (flags & RAMP_RECTIFY_XY_I32) rect_launch_events<true>(vec, grid, st, x, y, N, camera, H, W, xy_out, valid_out, status);
  else rect_launch_events<false>(vec, grid, st, x, y, N, camera, H, W, xy_out, valid_out, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

int ramp_image_rectify(const void *src, int C, int Hs, int Ws, const float *camera, int flags, int norm, float fill, int H, int W,
                       float *out, float *map_out, uint8_t *mask_out, int32_t *status, void *stream) {
  if (C < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~RAMP_RECTIFY_SRC_U8) return RAMP_EINVAL;
  if (norm != RAMP_RECTIFY_NORM_NONE && norm != RAMP_RECTIFY_NORM_HALF && norm != RAMP_RECTIFY_NORM_UNIT) return RAMP_EINVAL;
  if (!src || !camera || !out || !status) return RAMP_EINVAL;
  if (((uintptr_t)map_out & 7) != 0 || (((uintptr_t)out | (uintptr_t)camera | (uintptr_t)status) & 3) != 0) return RAMP_EINVAL;
  if (!(flags & RAMP_RECTIFY_SRC_U8) && ((uintptr_t)src & 3) != 0) return RAMP_EINVAL;
  if ((double)H * (double)W > 2147483647.0 || (double)Hs * (double)Ws > 2147483647.0) return RAMP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const long tiles = ((long)H * W + INTERP_THREADS - 1) / INTERP_THREADS;
  const int grid = (int)(tiles < RECT_MAX_GROUPS ? tiles : RECT_MAX_GROUPS);
  if (flags & RAMP_RECTIFY_SRC_U8)
    hipLaunchKernelGGL((rect_image_kernel<true>), dim3(grid), dim3(INTERP_THREADS), 0, st, src, C, Hs, Ws, camera, H, W, norm, fill,
                       out, map_out, mask_out, status);
  else
    hipLaunchKernelGGL((rect_image_kernel<false>), dim3(grid), dim3(INTERP_THREADS), 0, st, src, C, Hs, Ws, camera, H, W, norm, fill,
                       out, map_out, mask_out, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
