// Event contrast and its gradient (include/ramp_hip.h: ramp_event_contrast): the variance of the image of warped events,
// and its derivative with respect to a small correction theta = (v[3], w[3], lam) of the warp.  Everything up to X' is
// ramp_event_warp's, statement for statement (warp_device.h); the correction acts in the reference camera frame, to first
// order, by definition:
//
//   tau = float32(t - t_ref)            (the difference formed in float64; the unit of the time stamps)
//   ds  = d * expf(lam)
//   X1  = R_G P + t_G ds
//   X2  = X1 + tau * (v * ds + w x X1)
//   x'  = fx X2.x / X2.z + cx ,  y' = fy X2.y / X2.z + cy          invalid exactly as the warp, with X2.z in the place of Z'
//
// I(u) = sum_k s_k b(u - x'_k), s_k = p_k or 1 (RAMP_CONTRAST_UNSIGNED); f = (1 / P_n) sum_u (I(u) - mu)^2, P_n = H W.
//
//   df/dx'_k = (2 / P_n) s_k sum (I(ix + jx, iy + jy) - mu) * (jx ? +1 : -1) * wy[jy]       over the in-image neighbours
//   df/dy'_k = (2 / P_n) s_k sum (I(ix + jx, iy + jy) - mu) * (jy ? +1 : -1) * wx[jx]
//   dx'/dX2 = (fx / Z, 0, -fx X / Z^2)        dy'/dX2 = (0, fy / Z, -fy Y / Z^2)
//   dX2/dv  = tau ds I_3         dX2/dw . r = tau (r x X1)         dX2/dlam = t_G ds + tau (v ds + w x (t_G ds))
//
// ramp_event_align runs the line search over these evaluations on the device: align_step_kernel behind each of them (below).
//
// At most five launches behind one memset of the counters and accumulators:
//   the segment launch   of the event warp (ramp_i_warp_segments)
//   contrast_event_kernel<false>  the warp's splat with the correction: the same fixed point, the same staging and counters;
//                        every wave also adds its events' contributions to two 64-bit integer sums S1 (signed, count)
//   contrast_finish_kernel        accumulators -> iwe; with mu = S1 / P_n known exactly up to one rounding, per-workgroup
//                        partials of sum I^2 and sum (I - mu)^2 in double, (double)acc * 2^-24 being exact
//   contrast_event_kernel<true>   per event, one lane each: warp again, gather the four accumulators, seven terms in double
//                        from the fp32 geometry; per lane, then per wave by a fixed butterfly, then the waves in wave order:
//                        one row of 8 doubles per workgroup
//   contrast_final_kernel         one workgroup: partials and rows summed in index order -> stats, grad, sums, status
//
// The accumulators and S1 are integer sums: stats, sums and iwe do not depend on the order of the events.  The squares are
// centred BEFORE they are summed (that is why S1 is formed by the splat and not by the finish launch), so the variance of a
// nearly uniform image does not cancel.  grad is a sum of doubles in a fixed order for given arguments: it repeats its bits
// from call to call; another order of the events moves it by rounding.  No floating-point atomics.
#include "ramp_internal.h"
#include "warp_device.h"

#define CON_FIN_MAX_GROUPS 256           // workgroups of the finish launch; each walks the pixels with this stride
#define CON_ROW_WORDS 8                  // doubles per workgroup of the gradient launch: 7 terms, 1 spare
#define CON_WAVES (INTERP_THREADS / RAMP_WAVE)
#define CON_S1_WORD 8                    // the two int64 sums live in the spare counter words 8 .. 11

struct ConArgs {
  const float *x, *y;
  const double *t;
  const int8_t *p;
  const float *knots;
  const double *times;
  const float *seg, *ref, *intrinsics, *invdepth, *correction;
  long long *acc;                        // [2][H][W]
  int32_t *ctr;
  double *rows;                          // [grid][CON_ROW_WORDS]
  double t_ref;
  int N, T, H, W, extrapolate, depth_map, plane;
  const int32_t *done;                   // optional: a device word; not zero: every launch of the evaluation returns at once
};

// GRAD = false: the splat.  GRAD = true: the gradient's gather.  LDS_TIMES, VEC: as warp_event_kernel.
template <bool GRAD, bool LDS_TIMES, bool VEC>
__global__ void __launch_bounds__(INTERP_THREADS) contrast_event_kernel(const ConArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char con_smem[];
  __shared__ __attribute__((aligned(16))) double s_t[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_x[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_y[WARP_TILE];
  __shared__ __attribute__((aligned(16))) int8_t s_p[WARP_TILE];
  __shared__ float s_uni[WARP_UNI_WORDS];
  __shared__ float s_cor[8];
  __shared__ double s_range[2];
  __shared__ double s_red[GRAD ? CON_WAVES * CON_ROW_WORDS : 1];
  if (a.done && *a.done) return;                     // (wave-uniform: an alignment that has stopped)
  double *s_times = reinterpret_cast<double *>(con_smem);
  const int tid = threadIdx.x;
  const int N = a.N, T = a.T, H = a.H, W = a.W;
  if (LDS_TIMES)
    for (int i = tid; i < T; i += INTERP_THREADS) s_times[i] = a.times[i];
  if (tid == 12) { s_range[0] = a.times[0]; s_range[1] = a.times[T - 1]; }
  if (tid < 7) s_uni[tid] = a.ref[tid];
  else if (tid < 11) s_uni[tid] = a.intrinsics[tid - 7];
  else if (tid == 11) s_uni[tid] = a.depth_map ? 0.0f : a.invdepth[0];
  const bool has_cor = a.correction != nullptr;
  if (tid >= 16 && tid < 24) s_cor[tid - 16] = (has_cor && tid < 23) ? a.correction[tid - 16] : 0.0f;
  __syncthreads();
  bool cor_bad = false;
#pragma unroll
  for (int c = 0; c < 7; c++) cor_bad = cor_bad || !(fabsf(s_cor[c]) <= 3.4028234663852886e38f);
  if (!GRAD && cor_bad && blockIdx.x == 0 && tid == 0) atomicOr(a.ctr, RAMP_CONTRAST_BAD_CORRECTION);
  const bool failed = cor_bad || (a.ctr[0] & RAMP_INTERP_BAD_TIMES) != 0;      // (raised by the segment launch in front)
  const float v0 = s_cor[0], v1 = s_cor[1], v2 = s_cor[2], w0 = s_cor[3], w1 = s_cor[4], w2 = s_cor[5];
  const float el = has_cor ? expf(s_cor[6]) : 1.0f;
  const WarpScene sc = {a.knots, a.times, a.seg, a.invdepth, T, H, W, a.extrapolate, a.depth_map};
  const size_t HW = (size_t)H * W;
  const double fix = 1.0 / (double)(1 << WARP_FIX_BITS);
  double mu = 0.0;
  if (GRAD) {
    const long long S1 = reinterpret_cast<const long long *>(a.ctr + CON_S1_WORD)[a.plane];
    mu = ((double)S1 * fix) / (double)HW;
  }
  const long long *plane = a.acc + (size_t)a.plane * HW;
  const long tiles = ((long)N + WARP_TILE - 1) / WARP_TILE;
  int n_below = 0, n_above = 0, n_bad = 0, n_z = 0, n_out = 0, n_in = 0;    // wave-uniform: sums of ballots
  long long sum_signed = 0, sum_count = 0;                                  // per lane (the splat)
  double g[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                       // per lane (the gradient)
  for (long tile = blockIdx.x; tile < tiles && !(GRAD && failed); tile += gridDim.x) {
    const long base = tile * WARP_TILE;
    const int live = (int)min((long)WARP_TILE, (long)N - base);
    __syncthreads();                                 // (the previous tile has been read)
    if (VEC && live == WARP_TILE) {
      reinterpret_cast<float4 *>(s_x)[tid] = reinterpret_cast<const float4 *>(a.x + base)[tid];
      reinterpret_cast<float4 *>(s_y)[tid] = reinterpret_cast<const float4 *>(a.y + base)[tid];
      reinterpret_cast<int *>(s_p)[tid] = reinterpret_cast<const int *>(a.p + base)[tid];
      reinterpret_cast<double2 *>(s_t)[tid] = reinterpret_cast<const double2 *>(a.t + base)[tid];
      reinterpret_cast<double2 *>(s_t)[tid + INTERP_THREADS] = reinterpret_cast<const double2 *>(a.t + base)[tid + INTERP_THREADS];
    } else {
      for (int i = tid; i < live; i += INTERP_THREADS) {
        s_x[i] = a.x[base + i];
        s_y[i] = a.y[base + i];
        s_p[i] = a.p[base + i];
        s_t[i] = a.t[base + i];
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < WARP_TILE / INTERP_THREADS; k++) {
      const int e = k * INTERP_THREADS + tid;
      const bool have = e < live;
      bool below = false, above = false, bad = false, zrej = false, outside = false, inside = false;
      if (have) {
        const float x = s_x[e], y = s_y[e];
        const double t = s_t[e];
        float xw = 0.0f, yw = 0.0f, tau = 0.0f, ds = 0.0f;
        float X1[3] = {0.0f, 0.0f, 0.0f}, X2[3] = {0.0f, 0.0f, 0.0f}, tG[3] = {0.0f, 0.0f, 0.0f};
        bool valid = false;
        if (!warp_event_finite(x, y, t)) {
          bad = true;
        } else {
          float R[3], d;
          warp_event_geometry<LDS_TIMES>(sc, x, y, t, s_times, s_uni, s_range, &below, &above, R, tG, &d);
          ds = has_cor ? d * el : d;
          X1[0] = R[0] + tG[0] * ds; X1[1] = R[1] + tG[1] * ds; X1[2] = R[2] + tG[2] * ds;
          X2[0] = X1[0]; X2[1] = X1[1]; X2[2] = X1[2];
          if (GRAD || has_cor) tau = (float)(t - a.t_ref);
          if (has_cor) {
            X2[0] = X1[0] + tau * (v0 * ds + (w1 * X1[2] - w2 * X1[1]));
            X2[1] = X1[1] + tau * (v1 * ds + (w2 * X1[0] - w0 * X1[2]));
            X2[2] = X1[2] + tau * (v2 * ds + (w0 * X1[1] - w1 * X1[0]));
          }
          valid = warp_project(X2[0], X2[1], X2[2], s_uni, &xw, &yw);
          zrej = !valid;
        }
        if (failed) { valid = false; zrej = false; }
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
            double gx = 0.0, gy = 0.0;
#pragma unroll
            for (int jy = 0; jy < 2; jy++)
#pragma unroll
              for (int jx = 0; jx < 2; jx++)
                if (inx[jx] && iny[jy]) {
                  const size_t at = (size_t)(iy + jy) * W + (size_t)(ix + jx);
                  if (GRAD) {
                    const double dI = (double)plane[at] * fix - mu;
                    gx += dI * (jx ? (double)wy[jy] : -(double)wy[jy]);
                    gy += dI * (jy ? (double)wx[jx] : -(double)wx[jx]);
                  } else {
                    const long long c = warp_fixed_weight(wx[jx], wy[jy]);
                    if (c != 0) {
                      atomicAdd(reinterpret_cast<warp_u64 *>(a.acc + at), (warp_u64)(pol * c));
                      atomicAdd(reinterpret_cast<warp_u64 *>(a.acc + HW + at), (warp_u64)c);
                      sum_signed += pol * c;
                      sum_count += c;
                    }
                  }
                }
            if (GRAD) {
              const double sk = a.plane == 0 ? (double)pol : 1.0;
              const double fx = (double)s_uni[7], fy = (double)s_uni[8];
              const double X = (double)X2[0], Y = (double)X2[1], Z = (double)X2[2];
              const double ga = sk * gx * fx / Z, gb = sk * gy * fy / Z;          // df/dX2, without the factor 2 / P_n
              const double gc = -(sk * gx * fx * X + sk * gy * fy * Y) / (Z * Z);
              const double dtau = (double)tau, dds = (double)ds;
              const double A[3] = {(double)X1[0], (double)X1[1], (double)X1[2]};
              const double B[3] = {(double)tG[0] * dds, (double)tG[1] * dds, (double)tG[2] * dds};
              g[0] += dtau * dds * ga;
              g[1] += dtau * dds * gb;
              g[2] += dtau * dds * gc;
              g[3] += dtau * (A[1] * gc - A[2] * gb);                              // tau (X1 x df/dX2)
              g[4] += dtau * (A[2] * ga - A[0] * gc);
              g[5] += dtau * (A[0] * gb - A[1] * ga);
              const double L0 = B[0] + dtau * ((double)v0 * dds + ((double)w1 * B[2] - (double)w2 * B[1]));
              const double L1 = B[1] + dtau * ((double)v1 * dds + ((double)w2 * B[0] - (double)w0 * B[2]));
              const double L2 = B[2] + dtau * ((double)v2 * dds + ((double)w0 * B[1] - (double)w1 * B[0]));
              g[6] += ga * L0 + gb * L1 + gc * L2;
            }
          }
        }
      }
      if (!GRAD) {
        // the trip count and `have` aside, every lane of the wave is here
        n_below += ramp_wave_count(below);
        n_above += ramp_wave_count(above);
        n_bad += ramp_wave_count(bad);
        n_z += ramp_wave_count(zrej);
        n_out += ramp_wave_count(outside);
        n_in += ramp_wave_count(inside);
      }
    }
  }
  if (!GRAD) {
    sum_signed = ramp_wave_sum(sum_signed);
    sum_count = ramp_wave_sum(sum_count);
    ramp_wave_flush(a.ctr + 1, tid, n_below, n_above, n_bad, n_z, n_out, n_in);
    if ((tid & (RAMP_WAVE - 1)) == 0) {
      warp_u64 *S1 = reinterpret_cast<warp_u64 *>(a.ctr + CON_S1_WORD);
      if (sum_signed) atomicAdd(&S1[0], (warp_u64)sum_signed);
      if (sum_count) atomicAdd(&S1[1], (warp_u64)sum_count);
    }
  } else {
    // per wave by a fixed butterfly, then the waves in wave order
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 7; c++) {
      const double v = ramp_wave_sum(g[c]);
      if ((tid & (RAMP_WAVE - 1)) == 0) s_red[(tid / RAMP_WAVE) * CON_ROW_WORDS + c] = v;
    }
    __syncthreads();
    if (tid < CON_ROW_WORDS) {
      double v = 0.0;
      if (tid < 7)
        for (int w = 0; w < CON_WAVES; w++) v += s_red[w * CON_ROW_WORDS + tid];
      a.rows[(size_t)blockIdx.x * CON_ROW_WORDS + tid] = v;
    }
  }
}

// accumulators -> iwe, and per workgroup the partial sums of I^2 and (I - mu)^2 over the plane the statistics are taken from
__global__ void __launch_bounds__(256)
    contrast_finish_kernel(const long long *__restrict__ acc, const int32_t *__restrict__ ctr, float *__restrict__ iwe, long HW,
                           int plane, double *__restrict__ fin, const int32_t *__restrict__ done) {
  __shared__ double s_red[2 * CON_WAVES];
  if (done && *done) return;
  const int tid = threadIdx.x;
  const bool failed = (ctr[0] & (RAMP_INTERP_BAD_TIMES | RAMP_CONTRAST_BAD_CORRECTION)) != 0;
  const float qnan = __int_as_float(0x7fc00000), scale = 1.0f / (float)(1 << WARP_FIX_BITS);
  const double fix = 1.0 / (double)(1 << WARP_FIX_BITS);
  const double mu = ((double)reinterpret_cast<const long long *>(ctr + CON_S1_WORD)[plane] * fix) / (double)HW;
  double s2 = 0.0, c2 = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + tid; i < HW; i += (long)gridDim.x * blockDim.x) {
    const long long a0 = acc[i], a1 = acc[HW + i];
    if (iwe) {
      iwe[i] = failed ? qnan : (float)a0 * scale;      // int64 -> fp32 rounds once; the power of two is exact
      iwe[HW + i] = failed ? qnan : (float)a1 * scale;
    }
    const double v = (double)(plane ? a1 : a0) * fix;
    s2 += v * v;
    c2 += (v - mu) * (v - mu);
  }
  s2 = ramp_wave_sum(s2);
  c2 = ramp_wave_sum(c2);
  if ((tid & (RAMP_WAVE - 1)) == 0) { s_red[2 * (tid / RAMP_WAVE)] = s2; s_red[2 * (tid / RAMP_WAVE) + 1] = c2; }
  __syncthreads();
  if (tid < 2) {
    double v = 0.0;
    for (int w = 0; w < CON_WAVES; w++) v += s_red[2 * w + tid];
    fin[2 * (size_t)blockIdx.x + tid] = v;
  }
}

// one workgroup: the partials and the rows in index order
__global__ void __launch_bounds__(RAMP_WAVE)
    contrast_final_kernel(const int32_t *__restrict__ ctr, const double *__restrict__ fin, int n_fin, const double *__restrict__ rows,
                          int n_rows, long HW, int plane, long long *__restrict__ sums, double *__restrict__ stats,
                          double *__restrict__ grad, int32_t *__restrict__ status, const int32_t *__restrict__ done) {
  if (done && *done) return;
  const int tid = threadIdx.x;
  const int32_t word = ctr[0];
  const bool failed = (word & (RAMP_INTERP_BAD_TIMES | RAMP_CONTRAST_BAD_CORRECTION)) != 0;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double fix = 1.0 / (double)(1 << WARP_FIX_BITS), Pn = (double)HW;
  const long long *S1 = reinterpret_cast<const long long *>(ctr + CON_S1_WORD);
  if (tid < 8) status[tid] = tid < 7 ? ctr[tid] : 0;
  if (tid < 2) sums[tid] = S1[tid];
  if (tid < 7 && grad) {
    double v = 0.0;
    for (int r = 0; r < n_rows; r++) v += rows[(size_t)r * CON_ROW_WORDS + tid];
    grad[tid] = failed ? qnan : v * (2.0 / Pn);
  } else if (tid >= 8 && tid < 10) {
    double v = 0.0;
    for (int r = 0; r < n_fin; r++) v += fin[2 * (size_t)r + (tid - 8)];
    if (tid == 8) stats[2] = failed ? qnan : v;                  // sum of I^2
    else stats[0] = failed ? qnan : v / Pn;                      // the population variance
  } else if (tid == 10) {
    stats[1] = failed ? qnan : ((double)S1[plane] * fix) / Pn;   // the mean: the bits the other launches centred with
    stats[3] = Pn;
  } else if (tid >= 12 && tid < 16) {
    stats[tid - 8] = 0.0;
  }
}

static int con_fin_groups(long HW) {
  const long n = (HW + 255) / 256;
  return (int)(n < CON_FIN_MAX_GROUPS ? n : CON_FIN_MAX_GROUPS);
}

template <bool GRAD>
static int con_launch_events(const ConArgs &a, bool lds_times, bool vec, int grid, hipStream_t st) {
  const size_t lds = lds_times ? (size_t)a.T * sizeof(double) : 0;
  static_assert((size_t)INTERP_LDS_KNOTS * sizeof(double) + WARP_TILE * 17 + 512 <= 64 * 1024,
                "LDS within the default limit: the launch needs no hipFuncSetAttribute");
  if (lds_times) {
    if (vec) hipLaunchKernelGGL((contrast_event_kernel<GRAD, true, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((contrast_event_kernel<GRAD, true, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((contrast_event_kernel<GRAD, false, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((contrast_event_kernel<GRAD, false, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  }
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

// one evaluation: the memset of the counters (the two sums among them) and, behind them, the accumulators; the segment launch
// when `segments`; the splat, the finish, the gradient when `grad`, the final kernel
static int con_evaluate(const ConArgs &a, double *fin, bool segments, float *iwe, long long *sums, double *stats, double *grad,
                        int32_t *status, hipStream_t st) {
  const size_t HW = (size_t)a.H * a.W;
  if (hipMemsetAsync(a.ctr, 0, ws_span(a.ctr, fin), st) != hipSuccess) return RAMP_ELAUNCH;      // (fin: the block behind acc)
  int rc = RAMP_OK;
  if (segments) {
    rc = ramp_i_warp_segments(a.knots, a.times, a.T, a.t_ref, a.extrapolate, const_cast<float *>(a.seg), const_cast<float *>(a.ref),
                              a.ctr, st);
    if (rc != RAMP_OK) return rc;
  }
  const long tiles = ((long)a.N + WARP_TILE - 1) / WARP_TILE;
  const int grid = (int)(tiles < WARP_MAX_GROUPS ? tiles : WARP_MAX_GROUPS);
  const bool vec = (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.p | (uintptr_t)a.t) & 15) == 0;
  const bool lds_times = a.T <= INTERP_LDS_KNOTS;
  rc = con_launch_events<false>(a, lds_times, vec, grid, st);
  if (rc != RAMP_OK) return rc;
  const int n_fin = con_fin_groups((long)HW);
  hipLaunchKernelGGL(contrast_finish_kernel, dim3(n_fin), dim3(256), 0, st, a.acc, a.ctr, iwe, (long)HW, a.plane, fin, a.done);
  RAMP_CHECK_LAUNCH();
  if (grad) {
    rc = con_launch_events<true>(a, lds_times, vec, grid, st);
    if (rc != RAMP_OK) return rc;
  }
  hipLaunchKernelGGL(contrast_final_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, a.ctr, fin, n_fin, a.rows, grad ? grid : 0, (long)HW,
                     a.plane, sums, stats, grad, status, a.done);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

// the contrast's workspace: the warp's with the image accumulator alone (seg, ref | ctr | acc), then, packed, fin | rows
struct ConWs {
  WarpWs warp;
  double *fin, *rows;
};
static size_t con_carve(void *ws, int T, int H, int W, ConWs *w) {
  WsCarver c(ws, warp_carve(ws, T, (size_t)2 * H * W, 0, &w->warp));
  w->fin = c.take<double>((size_t)CON_FIN_MAX_GROUPS * 2, 1);
  w->rows = c.take<double>((size_t)WARP_MAX_GROUPS * CON_ROW_WORDS, 1);
  return c.bytes();
}

// the arguments both entries share -> ConArgs over the carved workspace
static ConArgs con_arguments(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                             const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth,
                             const float *correction, int flags, int H, int W, const ConWs &w) {
  ConArgs a;
  a.x = x; a.y = y; a.t = t; a.p = p; a.knots = knots; a.times = times; a.seg = w.warp.seg; a.ref = w.warp.ref;
  a.intrinsics = intrinsics; a.invdepth = invdepth; a.correction = correction; a.acc = w.warp.acc_iwe; a.ctr = w.warp.ctr;
  a.rows = w.rows;
  a.t_ref = t_ref; a.N = N; a.T = T; a.H = H; a.W = W; a.extrapolate = (flags & RAMP_INTERP_EXTRAPOLATE) ? 1 : 0;
  a.depth_map = (flags & RAMP_WARP_DEPTH_MAP) ? 1 : 0;
  a.plane = (flags & RAMP_CONTRAST_UNSIGNED) ? 1 : 0;
  a.done = nullptr;
  return a;
}

// ---------------------------------------------------------------------------------------------------- the line search
// The state machine of include/ramp_hip.h (ramp_event_align), one step behind every evaluation.  The block lives behind the
// contrast's own workspace; the front of the entry zeroes it and copies the start into `cor`.
struct AlignState {
  double theta[7], f, g[7], f0, length, gm[7], norm, trial[7];
  int32_t n_accepted, n_evals, halvings, reason, seen, spare[3];
  int32_t status[8];                     // the words of the evaluation at theta
  int32_t done[4];                       // [0]: reason != 0, the word the contrast launches read
  float cor[8];                          // the correction the next evaluation reads: float32(theta), then float32(trial)
  float cor_theta[8];                    // the bits the evaluation at theta read
  double e_stats[8], e_grad[8];          // what one evaluation writes
  long long e_sums[2];
  int32_t e_status[8];
};

struct AlignOut {
  double *correction;
  float *correction_f32;
  double *result, *grad, *history;
  int32_t *status, *info;
};

// One wave.  Every lane loads the whole state and takes every decision itself (uniform loads, no shuffles, no LDS): the
// arithmetic below is the definition's, in its order, once per lane; lane i < 7 then stores component i, lanes < 8 the status
// words, lane 0 the scalars.  e: the index of the evaluation in front; empty: N == 0, the all-zero statistics.
__global__ void __launch_bounds__(RAMP_WAVE)
    align_step_kernel(AlignState *__restrict__ s, int e, int last, int iters, int free_mask, double step, int empty,
                      const AlignOut out) {
  const int lane = threadIdx.x;
  int reason = s->reason;
  if (reason != 0 && !last) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double theta[7], g[7], gm[7], trial[7];
#pragma unroll
  for (int i = 0; i < 7; i++) { theta[i] = s->theta[i]; g[i] = s->g[i]; gm[i] = s->gm[i]; trial[i] = s->trial[i]; }
  double f = s->f, f0 = s->f0, length = s->length, norm = s->norm;
  int n_accepted = s->n_accepted, n_evals = s->n_evals, halvings = s->halvings, seen = s->seen;
  if (reason == 0) {
    const double ft = empty ? 0.0 : s->e_stats[0];
    const int word0 = empty ? 0 : s->e_status[0];
    n_evals += 1;
    seen |= word0;
    bool take;
    if (e == 0) {
#pragma unroll
      for (int i = 0; i < 7; i++) theta[i] = (double)s->cor[i];
      length = step;
      f = f0 = ft;
      take = true;
      for (int i = lane; i < iters; i += RAMP_WAVE) out.history[i] = qnan;
      if (iters == 0) reason = RAMP_ALIGN_ITERS;
    } else if (ft > f) {                               // (a NaN ft is not greater)
#pragma unroll
      for (int i = 0; i < 7; i++) theta[i] = trial[i];
      f = ft;
      take = true;
      if (lane == 0) out.history[n_accepted] = f;
      n_accepted += 1;
      length *= 2.0;
      halvings = 0;
      if (n_accepted == iters) reason = RAMP_ALIGN_ITERS;
    } else {
      take = false;
      length *= 0.5;
      halvings += 1;
      if (halvings == RAMP_ALIGN_TRIALS) reason = RAMP_ALIGN_STALLED;
    }
    if (take) {
#pragma unroll
      for (int i = 0; i < 7; i++) g[i] = empty ? 0.0 : s->e_grad[i];
      if (lane < 8) {
        s->status[lane] = empty ? 0 : s->e_status[lane];
        s->cor_theta[lane] = s->cor[lane];
      }
      if (reason == 0) {                               // propose(new direction)
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < 7; i++) {
          gm[i] = g[i] * ((free_mask >> i) & 1 ? 1.0 : 0.0);
          sum = sum + gm[i] * gm[i];
        }
        norm = sqrt(sum);
        if (!(norm > 0.0 && norm < __longlong_as_double(0x7ff0000000000000ll))) reason = RAMP_ALIGN_FLAT;
      }
    }
    if (reason == 0) {
#pragma unroll
      for (int i = 0; i < 7; i++) trial[i] = theta[i] + (length * gm[i]) / norm;
    }
    if (last && reason == 0) reason = RAMP_ALIGN_BUDGET;
#pragma unroll
    for (int i = 0; i < 7; i++)
      if (lane == i) {
        s->theta[i] = theta[i]; s->g[i] = g[i]; s->gm[i] = gm[i]; s->trial[i] = trial[i];
        if (reason == 0) s->cor[i] = (float)trial[i];  // round to nearest even; overflow to infinity is the contrast's to answer
      }
    if (lane == 0) {
      s->f = f; s->f0 = f0; s->length = length; s->norm = norm;
      s->n_accepted = n_accepted; s->n_evals = n_evals; s->halvings = halvings; s->reason = reason; s->seen = seen;
      s->done[0] = reason != 0;
    }
  }
  if (!last) return;
#pragma unroll
  for (int i = 0; i < 7; i++)
    if (lane == i) { out.correction[i] = theta[i]; out.grad[i] = g[i]; out.correction_f32[i] = s->cor_theta[i]; }
  if (lane < 8) {
    out.status[lane] = s->status[lane];                // (this lane's own stores above, or an earlier launch's)
    out.info[lane] = lane == 0 ? reason : lane == 1 ? n_accepted : lane == 2 ? n_evals : lane == 3 ? halvings : lane == 4 ? seen : 0;
  }
  if (lane < 4) out.result[lane] = lane == 0 ? f : lane == 1 ? f0 : lane == 2 ? length : 0.0;
}

// the alignment's workspace: the contrast's, then the state on the next multiple of 16
struct AlignWs {
  ConWs con;
  AlignState *state;
};
static size_t align_carve(void *ws, int T, int H, int W, AlignWs *w) {
  WsCarver c(ws, round_up(con_carve(ws, T, H, W, &w->con), 16));
  w->state = c.take<AlignState>(1, 1);
  return c.bytes();
}

extern "C" {
size_t ramp_event_contrast_workspace_bytes(int T, int H, int W) {
  if (H < 1 || W < 1) return 0;
  ConWs w;
  return con_carve(nullptr, T, H, W, &w);
}

int ramp_event_contrast(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                        const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth,
                        const float *correction, int flags, int H, int W, float *iwe, int64_t *sums, double *stats, double *grad,
                        void *ws, size_t ws_bytes, int32_t *status, void *stream) {
  if (N < 0 || T < 1 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~(RAMP_INTERP_EXTRAPOLATE | RAMP_WARP_DEPTH_MAP | RAMP_CONTRAST_UNSIGNED)) return RAMP_EINVAL;
  if (!(fabs(t_ref) <= 1.7976931348623157e308)) return RAMP_EINVAL;
  if (N == 0) return RAMP_OK;
  if (!x || !y || !t || !p || !knots || !times || !intrinsics || !invdepth || !sums || !stats || !ws || !status) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)stats & 7) != 0 || ((uintptr_t)grad & 7) != 0)
    return RAMP_EINVAL;
  ConWs w;
  if (ws_bytes < con_carve(ws, T, H, W, &w)) return RAMP_EWORKSPACE;
  const ConArgs a = con_arguments(x, y, t, p, N, knots, times, T, t_ref, intrinsics, invdepth, correction, flags, H, W, w);
  return con_evaluate(a, w.fin, true, iwe, (long long *)sums, stats, grad, status, (hipStream_t)stream);
}

size_t ramp_event_align_workspace_bytes(int T, int H, int W) {
  if (T < 1 || H < 1 || W < 1) return 0;
  AlignWs w;
  return align_carve(nullptr, T, H, W, &w);
}

int ramp_event_align(const float *x, const float *y, const double *t, const int8_t *p, int N, const float *knots,
                     const double *times, int T, double t_ref, const float *intrinsics, const float *invdepth,
                     const float *correction, int flags, int H, int W, int free_mask, double step, int iters, int max_evals,
                     double *correction_out, float *correction_f32, double *result, double *grad, double *history,
                     int32_t *status, int32_t *info, void *ws, size_t ws_bytes, void *stream) {
  if (N < 0 || T < 1 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~(RAMP_INTERP_EXTRAPOLATE | RAMP_WARP_DEPTH_MAP | RAMP_CONTRAST_UNSIGNED)) return RAMP_EINVAL;
  if (!(fabs(t_ref) <= 1.7976931348623157e308) || !(fabs(step) <= 1.7976931348623157e308)) return RAMP_EINVAL;
  if (iters < 0 || iters > RAMP_ALIGN_MAX_ITERS || max_evals < 1 || (free_mask & ~127) != 0) return RAMP_EINVAL;
  if (N > 0 && (!x || !y || !t || !p || !knots || !times || !intrinsics || !invdepth)) return RAMP_EINVAL;
  if (!correction_out || !correction_f32 || !result || !grad || (!history && iters > 0) || !status || !info || !ws) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || (((uintptr_t)correction_out | (uintptr_t)result | (uintptr_t)grad | (uintptr_t)history) & 7) != 0 ||
      (((uintptr_t)correction | (uintptr_t)correction_f32 | (uintptr_t)status | (uintptr_t)info) & 3) != 0)
    return RAMP_EINVAL;
  AlignWs w;
  if (ws_bytes < align_carve(ws, T, H, W, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int need = 1 + RAMP_ALIGN_TRIALS * iters;
  const int evals = N == 0 ? 1 : (max_evals < need ? max_evals : need);
  AlignState *s = w.state;
  // the invariant front: the state zeroed (reason 0, the done word 0), the start in the buffer evaluation 0 reads
  if (hipMemsetAsync(s, 0, sizeof(AlignState), st) != hipSuccess) return RAMP_ELAUNCH;
  if (correction && hipMemcpyAsync(s->cor, correction, 7 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return RAMP_ELAUNCH;
  ConArgs a = con_arguments(x, y, t, p, N, knots, times, T, t_ref, intrinsics, invdepth, s->cor, flags, H, W, w.con);
  a.done = s->done;
  const AlignOut out = {correction_out, correction_f32, result, grad, history, status, info};
  for (int e = 0; e < evals; e++) {
    if (N > 0) {
      const int rc = con_evaluate(a, w.con.fin, e == 0, nullptr, s->e_sums, s->e_stats, s->e_grad, s->e_status, st);
      if (rc != RAMP_OK) return rc;
    }
    hipLaunchKernelGGL(align_step_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, s, e, e == evals - 1 ? 1 : 0, iters, free_mask, step,
                       N == 0 ? 1 : 0, out);
    RAMP_CHECK_LAUNCH();
  }
  return RAMP_OK;
}
}  // extern "C"
