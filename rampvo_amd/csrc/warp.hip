// Motion-compensated events (include/ramp_hip.h: ramp_event_warp): every event is taken from the camera pose at its own time
// stamp to the pose at one reference time, and the warped events are splat bilinearly into an image of warped events and / or
// the encoder's bin stack.  One pass over the events; the per-event pose lives in registers only.
//
//   C(t)  = Exp(alpha * xi_s) * knots[s]                  the geodesic of ramp_se3_interp (interp_device.h), camera-to-world
//   G     = C(t_ref)^-1 * C(t)
//   X'    = R_G * ((x - cx) / fx, (y - cy) / fy, 1) + t_G * d         d: inverse depth (one float, or a map)
//   x'    = fx * (X' / Z') + cx,   y' = fy * (Y' / Z') + cy           invalid: Z' <= RAMP_WARP_MIN_Z, anything not finite
//
// Three launches behind one memset of the counters and accumulators:
//   warp_segment_kernel  the segment table of ramp_se3_interp (the same rows) and, in one extra workgroup, C(t_ref)^-1
//   warp_event_kernel    tiles of WARP_TILE events staged in LDS with 16-byte loads, one event per lane and trip: search,
//                        interpolation, warp, then up to four integer atomics per requested accumulator plane
//   warp_finish_kernel   accumulators -> fp32 / int8, counters -> status
//
// The splat is FIXED POINT: a neighbour's weight is the fp32 product of its two axis weights, its contribution
// llrint(weight * 2^24), added with 64-bit integer atomics.  Integer addition commutes, so the sums -- and every output --
// do not depend on the order in which events arrive, and a call repeats its bits.  |sum| < 2^63 holds up to 2^39 events on
// one pixel.  G is composed so that C(t) == C(t_ref) bit for bit gives the exact identity (see warp_relative).
#include "ramp_internal.h"
#include "warp_device.h"

__global__ void __launch_bounds__(INTERP_THREADS)
    warp_segment_kernel(const float *__restrict__ knots, const double *__restrict__ times, int T, double t_ref,
                        int extrapolate, float *__restrict__ seg, float *__restrict__ ref, int32_t *__restrict__ ctr) {
  const int S = T > 1 ? T - 1 : 1;
  if (blockIdx.x + 1 < gridDim.x) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && interp_segment_row(knots, times, T, s, seg + (size_t)s * INTERP_SEG_WORDS)) atomicOr(ctr, RAMP_INTERP_BAD_TIMES);
    return;
  }
  // the last workgroup: one lane forms C(t_ref)^-1 (warp_reference_row)
  if (threadIdx.x) return;
  warp_reference_row(knots, times, T, t_ref, extrapolate, ref);
}

struct WarpArgs {
  const float *x, *y;
  const double *t;
  const int8_t *p;
  const float *knots;
  const double *times;
  const float *seg, *ref, *intrinsics, *invdepth;
  float *xy_out;
  long long *acc_iwe, *acc_stack;
  int32_t *ctr;
  int N, T, bins, H, W, extrapolate, depth_map;
};

// IDENTITY: no trajectory, x' = x and y' = y (the bilinear path of the event stack).  LDS_TIMES, VEC: the knot times are
// staged in LDS; full tiles are loaded with 16-byte loads (every event array 16-byte aligned).
template <bool IDENTITY, bool LDS_TIMES, bool VEC>
__global__ void __launch_bounds__(INTERP_THREADS) warp_event_kernel(const WarpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char warp_smem[];
  __shared__ __attribute__((aligned(16))) double s_t[IDENTITY ? 2 : WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_x[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_y[WARP_TILE];
  __shared__ __attribute__((aligned(16))) int8_t s_p[WARP_TILE];
  __shared__ float s_uni[WARP_UNI_WORDS];
  __shared__ double s_range[2];
  double *s_times = reinterpret_cast<double *>(warp_smem);
  const int tid = threadIdx.x;
  const int N = a.N, T = a.T, H = a.H, W = a.W;
  if (!IDENTITY && LDS_TIMES)
    for (int i = tid; i < T; i += INTERP_THREADS) s_times[i] = a.times[i];
  const bool failed = !IDENTITY && (a.ctr[0] & RAMP_INTERP_BAD_TIMES) != 0;   // (raised by the segment launch in front)
  if (!IDENTITY) {
    if (tid == 12) { s_range[0] = a.times[0]; s_range[1] = a.times[T - 1]; }
    // C(t_ref)^-1 (7), the intrinsics (4) and the scalar inverse depth: read from LDS per event, not held in scalar registers
    if (tid < 7) s_uni[tid] = a.ref[tid];
    else if (tid < 11) s_uni[tid] = a.intrinsics[tid - 7];
    else if (tid == 11) s_uni[tid] = a.depth_map ? 0.0f : a.invdepth[0];
  }
  const float qnan = __int_as_float(0x7fc00000);
  const size_t HW = (size_t)H * W;
  const long tiles = ((long)N + WARP_TILE - 1) / WARP_TILE;
  int n_below = 0, n_above = 0, n_bad = 0, n_z = 0, n_out = 0, n_in = 0;    // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long base = tile * WARP_TILE;
    const int live = (int)min((long)WARP_TILE, (long)N - base);
    __syncthreads();                                 // (the staged knot times; the previous tile has been read)
    if (VEC && live == WARP_TILE) {
      reinterpret_cast<float4 *>(s_x)[tid] = reinterpret_cast<const float4 *>(a.x + base)[tid];
      reinterpret_cast<float4 *>(s_y)[tid] = reinterpret_cast<const float4 *>(a.y + base)[tid];
      reinterpret_cast<int *>(s_p)[tid] = reinterpret_cast<const int *>(a.p + base)[tid];
      if (!IDENTITY) {
        reinterpret_cast<double2 *>(s_t)[tid] = reinterpret_cast<const double2 *>(a.t + base)[tid];
        reinterpret_cast<double2 *>(s_t)[tid + INTERP_THREADS] = reinterpret_cast<const double2 *>(a.t + base)[tid + INTERP_THREADS];
      }
    } else {
      for (int i = tid; i < live; i += INTERP_THREADS) {
        s_x[i] = a.x[base + i];
        s_y[i] = a.y[base + i];
        s_p[i] = a.p[base + i];
        if (!IDENTITY) s_t[i] = a.t[base + i];
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < WARP_TILE / INTERP_THREADS; k++) {
      const int e = k * INTERP_THREADS + tid;
      const bool have = e < live;
      bool below = false, above = false, bad = false, zrej = false, outside = false, inside = false;
      if (have) {
        const long i = base + e;
        const float x = s_x[e], y = s_y[e];
        const double t = IDENTITY ? 0.0 : s_t[e];
        float xw = qnan, yw = qnan;
        bool valid = false;
        if (!warp_event_finite(x, y, t)) {
          bad = true;
        } else if (IDENTITY) {
          xw = x;
          yw = y;
          valid = true;
        } else {
          float R[3], tG[3], d;
          const WarpScene sc = {a.knots, a.times, a.seg, a.invdepth, T, H, W, a.extrapolate, a.depth_map};
          warp_event_geometry<LDS_TIMES>(sc, x, y, t, s_times, s_uni, s_range, &below, &above, R, tG, &d);
          const float Xp = R[0] + tG[0] * d, Yp = R[1] + tG[1] * d, Zp = R[2] + tG[2] * d;
          float xp, yp;
          valid = warp_project(Xp, Yp, Zp, s_uni, &xp, &yp);
          zrej = !valid;                                 // (a NaN Z' fails the comparison: rejected, like a NaN projection)
          if (valid) { xw = xp; yw = yp; }
        }
        if (failed) { valid = false; zrej = false; xw = qnan; yw = qnan; }
        if (a.xy_out) reinterpret_cast<float2 *>(a.xy_out)[i] = make_float2(xw, yw);
        if (valid) {
          int ix, iy;
          float wx[2], wy[2];
          bool inx[2], iny[2];
          warp_axis(xw, W, &ix, &wx[0], &wx[1], &inx[0], &inx[1]);
          warp_axis(yw, H, &iy, &wy[0], &wy[1], &iny[0], &iny[1]);
          inside = (inx[0] || inx[1]) && (iny[0] || iny[1]);
          outside = !inside;
          if (inside) {
            const long long pol = s_p[e] == 0 ? -1ll : (long long)s_p[e];    // (0 is read as -1, like ops.event_stack)
            int b = 0;
            if (a.acc_stack) b = min((int)(((float)a.bins * (float)i) / (float)N), a.bins - 1);
#pragma unroll
            for (int jy = 0; jy < 2; jy++)
#pragma unroll
              for (int jx = 0; jx < 2; jx++)
                if (inx[jx] && iny[jy]) {
                  const long long c = warp_fixed_weight(wx[jx], wy[jy]);
                  if (c != 0) {
                    const size_t at = (size_t)(iy + jy) * W + (size_t)(ix + jx);
                    if (a.acc_iwe) {
                      atomicAdd(reinterpret_cast<warp_u64 *>(a.acc_iwe + at), (warp_u64)(pol * c));
                      atomicAdd(reinterpret_cast<warp_u64 *>(a.acc_iwe + HW + at), (warp_u64)c);
                    }
                    if (a.acc_stack) atomicAdd(reinterpret_cast<warp_u64 *>(a.acc_stack + (size_t)b * HW + at), (warp_u64)(pol * c));
                  }
                }
          }
        }
      }
      // the trip count and `have` aside, every lane of the wave is here
      n_below += ramp_wave_count(below);
      n_above += ramp_wave_count(above);
      n_bad += ramp_wave_count(bad);
      n_z += ramp_wave_count(zrej);
      n_out += ramp_wave_count(outside);
      n_in += ramp_wave_count(inside);
    }
  }
  ramp_wave_flush(a.ctr + 1, tid, n_below, n_above, n_bad, n_z, n_out, n_in);
}

__global__ void __launch_bounds__(256)
    warp_finish_kernel(const long long *__restrict__ acc_iwe, const long long *__restrict__ acc_stack, const int32_t *__restrict__ ctr,
                       float *__restrict__ iwe, float *__restrict__ stack_f32, int8_t *__restrict__ stack_i8, long n_iwe,
                       long n_stack, int32_t *__restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool failed = (ctr[0] & RAMP_INTERP_BAD_TIMES) != 0;
  const float qnan = __int_as_float(0x7fc00000), scale = 1.0f / (float)(1 << WARP_FIX_BITS);
  if (i < 8) status[i] = i < 7 ? ctr[i] : 0;
  if (i < n_iwe) {
    iwe[i] = failed ? qnan : (float)acc_iwe[i] * scale;      // int64 -> fp32 rounds once; the power of two is exact
  } else if (i - n_iwe < n_stack) {
    const long j = i - n_iwe;
    const long long v = acc_stack[j];
    if (stack_f32) stack_f32[j] = failed ? qnan : (float)v * scale;
    if (stack_i8) stack_i8[j] = failed ? (int8_t)0 : (int8_t)(v / (1ll << WARP_FIX_BITS));   // toward zero, then modulo 256
  }
}

template <bool IDENTITY>
static int warp_launch_events(const WarpArgs &a, bool lds_times, bool vec, int grid, hipStream_t st) {
  const size_t lds = (!IDENTITY && lds_times) ? (size_t)a.T * sizeof(double) : 0;
  static_assert((size_t)INTERP_LDS_KNOTS * sizeof(double) + WARP_TILE * 17 <= 64 * 1024,
                "LDS within the default limit: the launch needs no hipFuncSetAttribute");
  if (!IDENTITY && lds_times) {
    if (vec) hipLaunchKernelGGL((warp_event_kernel<IDENTITY, !IDENTITY, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((warp_event_kernel<IDENTITY, !IDENTITY, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((warp_event_kernel<IDENTITY, false, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((warp_event_kernel<IDENTITY, false, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  }
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

int ramp_i_warp_segments(const float *knots, const double *times, int T, double t_ref, int extrapolate, float *seg, float *ref,
                         int32_t *ctr, hipStream_t st) {
  const int S = T > 1 ? T - 1 : 1;
  hipLaunchKernelGGL(warp_segment_kernel, dim3(ramp_cdiv(S, INTERP_THREADS) + 1), dim3(INTERP_THREADS), 0, st, knots, times,
                     T, t_ref, extrapolate, seg, ref, ctr);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

extern "C" {
size_t ramp_event_warp_workspace_bytes(int T, int bins, int H, int W) {
  if (H < 1 || W < 1) return 0;
  WarpWs w;                              // (room for both accumulators, whichever a call uses)
  return warp_carve(nullptr, T, (size_t)2 * H * W, (size_t)(bins > 0 ? bins : 0) * H * W, &w);
}
long ramp_event_warp_grid_events(void) { return (long)WARP_MAX_GROUPS * WARP_TILE; }

int ramp_event_warp(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                    const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth, int flags,
                    int bins, int H, int W, float *xy_out, float *iwe, float *stack_f32, int8_t *stack_i8, void *ws,
                    size_t ws_bytes, int32_t *status, void *stream) {
  const bool identity = (flags & RAMP_WARP_IDENTITY) != 0;
  if (identity) T = 1;
  if (N < 0 || T < 1 || H < 1 || W < 1 || bins < 1) return RAMP_EINVAL;
  if (!xy_out && !iwe && !stack_f32 && !stack_i8) return RAMP_EINVAL;
  if (flags & ~(RAMP_INTERP_EXTRAPOLATE | RAMP_WARP_DEPTH_MAP | RAMP_WARP_IDENTITY)) return RAMP_EINVAL;
  if (N == 0) return RAMP_OK;
  if (!x || !y || !p || !ws || !status) return RAMP_EINVAL;
  if (!identity && (!t || !knots || !times || !intrinsics || !invdepth || !(fabs(t_ref) <= 1.7976931348623157e308)))
    return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)xy_out & 7) != 0) return RAMP_EINVAL;    // (xy_out rows are stored as float2)
  if (ws_bytes < ramp_event_warp_workspace_bytes(T, bins, H, W)) return RAMP_EWORKSPACE;    // (never less than this call's own carve)
  hipStream_t st = (hipStream_t)stream;
  const size_t HW = (size_t)H * W;
  const bool stack = stack_f32 || stack_i8;
  const long n_iwe = iwe ? (long)(2 * HW) : 0, n_stack = stack ? (long)((size_t)bins * HW) : 0;
  WarpWs w;
  warp_carve(ws, T, (size_t)n_iwe, (size_t)n_stack, &w);
  float *seg = w.seg, *ref = w.ref;
  int32_t *ctr = w.ctr;
  long long *acc_iwe = iwe ? w.acc_iwe : nullptr, *acc_stack = stack ? w.acc_stack : nullptr;
  // the one memset: the counters and, behind them, the accumulators this call uses
  if (hipMemsetAsync(ctr, 0, ws_span(ctr, w.end), st) != hipSuccess) return RAMP_ELAUNCH;
  const int ex = (flags & RAMP_INTERP_EXTRAPOLATE) ? 1 : 0;
  if (!identity) {
    const int rc = ramp_i_warp_segments(knots, times, T, t_ref, ex, seg, ref, ctr, st);
    if (rc != RAMP_OK) return rc;
  }
  WarpArgs a;
  a.x = x; a.y = y; a.t = t; a.p = p; a.knots = knots; a.times = times; a.seg = seg; a.ref = ref;
  a.intrinsics = intrinsics; a.invdepth = invdepth; a.xy_out = xy_out; a.acc_iwe = acc_iwe; a.acc_stack = acc_stack;
  a.ctr = ctr; a.N = N; a.T = T; a.bins = bins; a.H = H; a.W = W; a.extrapolate = ex;
  a.depth_map = (flags & RAMP_WARP_DEPTH_MAP) ? 1 : 0;
  const long tiles = ((long)N + WARP_TILE - 1) / WARP_TILE;
  const int grid = (int)(tiles < WARP_MAX_GROUPS ? tiles : WARP_MAX_GROUPS);
  const bool vec = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)p | (identity ? 0 : (uintptr_t)t)) & 15) == 0;
  const int rc = identity ? warp_launch_events<true>(a, false, vec, grid, st)
                          : warp_launch_events<false>(a, T <= INTERP_LDS_KNOTS, vec, grid, st);
  if (rc != RAMP_OK) return rc;
  const long n = n_iwe + n_stack > 8 ? n_iwe + n_stack : 8;
  hipLaunchKernelGGL(warp_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc_iwe, acc_stack, ctr, iwe,
                     stack_f32, stack_i8, n_iwe, n_stack, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
