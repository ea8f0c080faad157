// Event multi-view stereo (include/ramp_hip.h: ramp_event_dsi): every event is back-projected as a ray from the camera pose at
// its own time stamp and swept through D planes of constant inverse depth of the camera at t_ref; each plane takes the warp's
// bilinear splat of the event (the "disparity space image" of EMVS, Rebecq et al., IJCV 2018).  Where the scene's edges are the
// votes pile up in one plane: the plane with the most votes of a pixel, refined by a parabola, is its inverse depth.
//
//   d_k   = float32(double(d_lo) + k * step),  step = (double(d_hi) - double(d_lo)) / (D - 1)         (read on the device)
//   X'_k  = R + t_G * d_k                       R, t_G: warp_event_geometry (warp_device.h), once per event
//   x'_k  = warp_project(X'_k)                  no vote: Z' <= RAMP_WARP_MIN_Z, anything not finite
//   vote  = the splat of ramp_event_warp: warp_axis, warp_fixed_weight, 64-bit integer atomics into dsi[k]
//
// Four launches behind one memset of the DSI:
//   dsi_segment_kernel    the segment table of ramp_se3_interp (the same rows), one flag per workgroup for its time stamps and,
//                         in one extra workgroup, C(t_ref)^-1 and the zeroed counters
//   dsi_vote_kernel       tiles of WARP_TILE events staged in LDS as the warp stages them; one event per lane and trip: geometry
//                         once, then the planes in order -- a workgroup's 256 events are in the same plane at the same time,
//                         and the workgroups start together, so the planes being written are few and stay in L2
//   dsi_detect_kernel     per pixel: the best plane (the lowest on a tie), its votes, the refined inverse depth
//   dsi_threshold_kernel  per DSI_TW x DSI_TH pixels: the box sum of the best votes through LDS (rows, then columns: integers,
//                         exact), the detection, the outputs and the detected count
//
// No word of the workspace is cleared by a memset: the counters are zeroed by the segment launch's extra workgroup, the bits
// of status word 0 are formed without atomics (the per-workgroup flags, the range itself), and the words every pixel owns are
// written by the pixel's lane.  Votes are integers: the sums do not depend on the events' order and a call repeats its bits.
#include "ramp_internal.h"
#include "warp_device.h"

#define DSI_TW 32
#define DSI_TH 8
#define DSI_RMAX 15                       // the largest adaptive_radius: the halo of a threshold tile in LDS
#define DSI_MAX_VOTES (1ll << 38)         // N * D below this: every box sum stays below 2^62
static_assert(DSI_TW * DSI_TH == INTERP_THREADS, "one pixel per lane");

static __device__ __forceinline__ bool dsi_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

// a word of `range` is not finite, d_lo < 0, or d_hi <= d_lo with more than one plane
static __device__ __forceinline__ bool dsi_bad_range(float lo, float hi, int D) {
  return !dsi_finite(lo) || !dsi_finite(hi) || lo < 0.0f || (D > 1 && hi <= lo);
}
static __device__ __forceinline__ double dsi_step(float lo, float hi, int D) {
  return D > 1 ? ((double)hi - (double)lo) / (double)(D - 1) : 0.0;
}

__global__ void __launch_bounds__(INTERP_THREADS)
    dsi_segment_kernel(const float *__restrict__ knots, const double *__restrict__ times, int T, double t_ref, int extrapolate,
                       float *__restrict__ seg, float *__restrict__ ref, int32_t *__restrict__ flags, int32_t *__restrict__ ctr) {
  const int S = T > 1 ? T - 1 : 1;
  if (blockIdx.x + 1 < gridDim.x) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int bad = s < S && interp_segment_row(knots, times, T, s, seg + (size_t)s * INTERP_SEG_WORDS);
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) flags[blockIdx.x] = any;
    return;
  }
  // the last workgroup: the counters, and C(t_ref)^-1 as warp_segment_kernel forms it
  if (threadIdx.x >= 1 && threadIdx.x <= WARP_CTR_WORDS) ctr[threadIdx.x - 1] = 0;
  if (threadIdx.x) return;
  warp_reference_row(knots, times, T, t_ref, extrapolate, ref);
}

struct DsiVote {
  const float *x, *y;
  const double *t;
  const float *knots;
  const double *times;
  const float *seg, *ref, *intrinsics, *range;
  const int32_t *flags;
  float *coords;
  long long *dsi;
  int32_t *ctr;
  int N, T, H, W, D, extrapolate, n_flags;
};

template <bool LDS_TIMES, bool VEC>
__global__ void __launch_bounds__(INTERP_THREADS) dsi_vote_kernel(const DsiVote a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsi_smem[];
  __shared__ __attribute__((aligned(16))) double s_t[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_x[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_y[WARP_TILE];
  __shared__ float s_uni[WARP_UNI_WORDS];
  __shared__ double s_range[2];
  double *s_times = reinterpret_cast<double *>(dsi_smem);
  const int tid = threadIdx.x;
  const int N = a.N, T = a.T, H = a.H, W = a.W, D = a.D;
  if (LDS_TIMES)
    for (int i = tid; i < T; i += INTERP_THREADS) s_times[i] = a.times[i];
  if (tid == 12) { s_range[0] = a.times[0]; s_range[1] = a.times[T - 1]; }
  if (tid < 7) s_uni[tid] = a.ref[tid];
  else if (tid < 11) s_uni[tid] = a.intrinsics[tid - 7];
  else if (tid == 11) s_uni[tid] = 0.0f;                // (the warp's scalar depth: not used, the planes take its place)
  // the bits of status word 0: the segment launch's flags and the range, the same in every workgroup
  int bad_times = 0;
  for (int i = tid; i < a.n_flags; i += INTERP_THREADS) bad_times |= a.flags[i];
  bad_times = __syncthreads_or(bad_times);              // (also the barrier behind the staged knot times and s_uni)
  const float d_lo = a.range[0], d_hi = a.range[1];
  const bool bad_range = dsi_bad_range(d_lo, d_hi, D);
  const bool failed = bad_times != 0 || bad_range;
  if (blockIdx.x == 0 && tid == 0) a.ctr[0] = (bad_times ? RAMP_INTERP_BAD_TIMES : 0) | (bad_range ? RAMP_DSI_BAD_RANGE : 0);
  const double lo = (double)d_lo, step = dsi_step(d_lo, d_hi, D);
  const float qnan = __int_as_float(0x7fc00000);
  const size_t HW = (size_t)H * W;
  const long tiles = ((long)N + WARP_TILE - 1) / WARP_TILE;
  int n_below = 0, n_above = 0, n_bad = 0, n_none = 0, n_voted = 0;    // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long base = tile * WARP_TILE;
    const int live = (int)min((long)WARP_TILE, (long)N - base);
    __syncthreads();                                   // the previous tile has been read
    if (VEC && live == WARP_TILE) {
      reinterpret_cast<float4 *>(s_x)[tid] = reinterpret_cast<const float4 *>(a.x + base)[tid];
      reinterpret_cast<float4 *>(s_y)[tid] = reinterpret_cast<const float4 *>(a.y + base)[tid];
      reinterpret_cast<double2 *>(s_t)[tid] = reinterpret_cast<const double2 *>(a.t + base)[tid];
      reinterpret_cast<double2 *>(s_t)[tid + INTERP_THREADS] = reinterpret_cast<const double2 *>(a.t + base)[tid + INTERP_THREADS];
    } else {
      for (int i = tid; i < live; i += INTERP_THREADS) {
        s_x[i] = a.x[base + i];
        s_y[i] = a.y[base + i];
        s_t[i] = a.t[base + i];
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int trip = 0; trip < WARP_TILE / INTERP_THREADS; trip++) {
      const int e = trip * INTERP_THREADS + tid;
      const bool have = e < live;
      bool below = false, above = false, bad = false, voted = false;
      if (have) {
        const size_t i = (size_t)(base + e);
        const float x = s_x[e], y = s_y[e];
        const double t = s_t[e];
        bad = !warp_event_finite(x, y, t);
        float R[3] = {0.0f, 0.0f, 0.0f}, tG[3] = {0.0f, 0.0f, 0.0f}, d;
        if (!bad) {
          const WarpScene sc = {a.knots, a.times, a.seg, nullptr, T, H, W, a.extrapolate, 0};
          warp_event_geometry<LDS_TIMES>(sc, x, y, t, s_times, s_uni, s_range, &below, &above, R, tG, &d);
        }
        const bool sweep = !bad && !failed;
        float2 *row = a.coords ? reinterpret_cast<float2 *>(a.coords) + i * (size_t)D : nullptr;
#pragma unroll 1
        for (int k = 0; k < D; k++) {
          float xw = qnan, yw = qnan;
          bool valid = false;
          if (sweep) {
            const float dk = (float)(lo + (double)k * step);
            const float Xp = R[0] + tG[0] * dk, Yp = R[1] + tG[1] * dk, Zp = R[2] + tG[2] * dk;
            float xp, yp;
            valid = warp_project(Xp, Yp, Zp, s_uni, &xp, &yp);
            if (valid) { xw = xp; yw = yp; }
          }
          if (row) row[k] = make_float2(xw, yw);
          if (valid) {
            voted = true;
            int ix, iy;
            float wx[2], wy[2];
            bool inx[2], iny[2];
            warp_axis(xw, W, &ix, &wx[0], &wx[1], &inx[0], &inx[1]);
            warp_axis(yw, H, &iy, &wy[0], &wy[1], &iny[0], &iny[1]);
            long long *plane = a.dsi + (size_t)k * HW;
#pragma unroll
            for (int jy = 0; jy < 2; jy++)
#pragma unroll
              for (int jx = 0; jx < 2; jx++)
                if (inx[jx] && iny[jy]) {
                  const long long c = warp_fixed_weight(wx[jx], wy[jy]);
                  if (c != 0) atomicAdd(reinterpret_cast<warp_u64 *>(plane + (size_t)(iy + jy) * W + (size_t)(ix + jx)), (warp_u64)c);
                }
          }
        }
      }
      // the trip count and `have` aside, every lane of the wave is here
      n_below += ramp_wave_count(below);
      n_above += ramp_wave_count(above);
      n_bad += ramp_wave_count(bad);
      n_none += ramp_wave_count(have && !bad && !voted);
      n_voted += ramp_wave_count(voted);
    }
  }
  ramp_wave_flush(a.ctr + 1, tid, n_below, n_above, n_bad, n_none, n_voted);
}

// per pixel: best = max_k dsi[k], the lowest k that attains it, and the inverse depth of the parabola through its neighbours
__global__ void __launch_bounds__(INTERP_THREADS)
    dsi_detect_kernel(const long long *__restrict__ dsi, const float *__restrict__ range, const int32_t *__restrict__ ctr, int D,
                      long HW, long long *__restrict__ best_out, float *__restrict__ inv_out, int32_t *__restrict__ plane_out,
                      int32_t *__restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 8) status[i] = i < 6 ? ctr[i] : 0;             // (the vote launch is complete; word 6 is counted by the next launch)
  if (i >= HW) return;
  long long best = dsi[i];
  int plane = 0;
  for (int k = 1; k < D; k++) {
    const long long v = dsi[(size_t)k * HW + i];
    if (v > best) { best = v; plane = k; }
  }
  double delta = 0.0;
  if (plane > 0 && plane < D - 1) {
    const long long va = dsi[(size_t)(plane - 1) * HW + i], vc = dsi[(size_t)(plane + 1) * HW + i];
    const long long den = va - 2 * best + vc;
    if (den != 0) delta = (double)(va - vc) / (2.0 * (double)den);
  }
  const float d_lo = range[0], d_hi = range[1];
  const double step = dsi_step(d_lo, d_hi, D);
  best_out[i] = best;
  plane_out[i] = plane;
  inv_out[i] = (float)((double)d_lo + ((double)plane + delta) * step);
}

__global__ void __launch_bounds__(INTERP_THREADS)
    dsi_threshold_kernel(const long long *__restrict__ best, const float *__restrict__ inv, const int32_t *__restrict__ plane_ws,
                         const int32_t *__restrict__ ctr, const float *__restrict__ fill, long long min_fixed,
                         long long offset_fixed, int r, int H, int W, float *__restrict__ invdepth,
                         float *__restrict__ confidence, int32_t *__restrict__ plane, int32_t *status) {
  __shared__ long long s_best[DSI_TH + 2 * DSI_RMAX][DSI_TW + 2 * DSI_RMAX];
  __shared__ long long s_row[DSI_TH + 2 * DSI_RMAX][DSI_TW];
  const int tid = threadIdx.x;
  const int tiles_x = (W + DSI_TW - 1) / DSI_TW;
  const int x0 = (int)(blockIdx.x % tiles_x) * DSI_TW, y0 = (int)(blockIdx.x / tiles_x) * DSI_TH;
  const bool failed = ctr[0] != 0;
  if (r > 0) {                                           // (r is the same in every lane: the barriers are uniform)
    const int rows = DSI_TH + 2 * r, cols = DSI_TW + 2 * r;
    for (int i = tid; i < rows * cols; i += INTERP_THREADS) {
      const int ly = i / cols, lx = i % cols, gy = y0 - r + ly, gx = x0 - r + lx;
      s_best[ly][lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? best[(size_t)gy * W + gx] : 0ll;
    }
    __syncthreads();
    for (int i = tid; i < rows * DSI_TW; i += INTERP_THREADS) {
      const int ly = i / DSI_TW, lx = i % DSI_TW;
      long long s = 0;
      for (int j = 0; j <= 2 * r; j++) s += s_best[ly][lx + j];
      s_row[ly][lx] = s;
    }
    __syncthreads();
  }
  const int lx = tid % DSI_TW, ly = tid / DSI_TW, px = x0 + lx, py = y0 + ly;
  bool det = false;
  if (px < W && py < H) {
    const size_t at = (size_t)py * W + px;
    const long long b = best[at];
    det = !failed && b >= min_fixed;
    if (r > 0) {
      long long box = 0;
      for (int j = 0; j <= 2 * r; j++) box += s_row[ly + j][lx];
      const long long n_in = (long long)(min(px + r, W - 1) - max(px - r, 0) + 1) * (min(py + r, H - 1) - max(py - r, 0) + 1);
      det = det && b >= box / n_in + offset_fixed;       // (box >= 0 and n_in > 0: the quotient is the floor)
    }
    const float qnan = __int_as_float(0x7fc00000);
    if (invdepth) invdepth[at] = failed ? qnan : det ? inv[at] : (fill ? fill[0] : qnan);
    if (confidence) confidence[at] = failed ? qnan : (float)b * (1.0f / (float)(1 << WARP_FIX_BITS));
    if (plane) plane[at] = det ? plane_ws[at] : -1;
  }
  // every lane of the wave is here
  const int n_det = ramp_wave_count(det);
  ramp_wave_flush(status + 6, tid, n_det);
}

// the workspace, packed: seg, ref | ctr | flags | best | inv | plane.  Nothing of it is cleared by a memset.
struct DsiWs {
  float *seg, *ref;
  int32_t *ctr, *flags;
  long long *best;
  float *inv;
  int32_t *plane;
};
static int dsi_flag_words(int T) { return ramp_cdiv(T > 1 ? T - 1 : 1, INTERP_THREADS); }
static size_t dsi_carve(void *ws, int T, size_t HW, DsiWs *w) {
  WsCarver c(ws, interp_carve(ws, T, &w->seg));
  w->ref = c.take<float>(WARP_REF_WORDS, 1);
  w->ctr = c.take<int32_t>(WARP_CTR_WORDS, 1);
  w->flags = c.take<int32_t>((size_t)dsi_flag_words(T), 16);
  w->best = c.take<long long>(HW, 1);
  w->inv = c.take<float>(HW, 1);
  w->plane = c.take<int32_t>(HW, 16);
  return c.bytes();
}

static bool dsi_fixed(double v, long long *out) {      // llrint(v * 2^24), refused when it is not finite or leaves 2^62
  const double s = v * (double)(1 << WARP_FIX_BITS);
  if (!(fabs(s) < 4611686018427387904.0)) return false;
  *out = llrint(s);
  return true;
}

extern "C" {
size_t ramp_event_dsi_ws_bytes(int T, int H, int W) {
  if (T < 1 || H < 1 || W < 1) return 0;
  DsiWs w;
  return dsi_carve(nullptr, T, (size_t)H * W, &w);
}
long ramp_event_dsi_grid_events(void) { return (long)WARP_MAX_GROUPS * WARP_TILE; }

int ramp_event_dsi(const float *x, const float *y, const double *t, int N, const float *knots, const double *times, int T,
                   double t_ref, const float *intrinsics, const float *range, int flags, int D, int H, int W, double min_votes,
                   int adaptive_radius, double adaptive_offset, const float *fill, int64_t *dsi, float *coords,
                   float *invdepth, float *confidence, int32_t *plane, void *ws, size_t ws_bytes, int32_t *status,
                   void *stream) {
  if (N < 0 || T < 1 || H < 1 || W < 1 || D < 1) return RAMP_EINVAL;
  if (adaptive_radius < 0 || adaptive_radius > DSI_RMAX) return RAMP_EINVAL;
  if (flags & ~RAMP_INTERP_EXTRAPOLATE) return RAMP_EINVAL;
  if (N > 0 && (!x || !y || !t)) return RAMP_EINVAL;
  if (!knots || !times || !intrinsics || !range || !dsi || !ws || !status) return RAMP_EINVAL;
  if (!(fabs(t_ref) <= 1.7976931348623157e308)) return RAMP_EINVAL;
  long long min_fixed, offset_fixed;
  if (!dsi_fixed(min_votes, &min_fixed) || !dsi_fixed(adaptive_offset, &offset_fixed)) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)dsi & 7) != 0 || ((uintptr_t)coords & 7) != 0) return RAMP_EINVAL;
  const size_t HW = (size_t)H * W;
  if ((double)D * (double)H * (double)W >= 2147483648.0 || (long long)N * D >= DSI_MAX_VOTES) return RAMP_EUNSUPPORTED;
  DsiWs w;
  if (ws_bytes < dsi_carve(ws, T, HW, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // the one memset: the DSI
  if (hipMemsetAsync(dsi, 0, (size_t)D * HW * sizeof(int64_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const int ex = (flags & RAMP_INTERP_EXTRAPOLATE) ? 1 : 0;
  const int n_flags = dsi_flag_words(T);
  hipLaunchKernelGGL(dsi_segment_kernel, dim3(n_flags + 1), dim3(INTERP_THREADS), 0, st, knots, times, T, t_ref, ex, w.seg, w.ref,
                     w.flags, w.ctr);
  RAMP_CHECK_LAUNCH();
  DsiVote a;
  a.x = x; a.y = y; a.t = t; a.knots = knots; a.times = times; a.seg = w.seg; a.ref = w.ref; a.intrinsics = intrinsics;
  a.range = range; a.flags = w.flags; a.coords = coords; a.dsi = reinterpret_cast<long long *>(dsi); a.ctr = w.ctr;
  a.N = N; a.T = T; a.H = H; a.W = W; a.D = D; a.extrapolate = ex; a.n_flags = n_flags;
  const long tiles = ((long)N + WARP_TILE - 1) / WARP_TILE;
  // (no event still launches one workgroup: the bits of status word 0 are formed there)
  const int grid = (int)(tiles < 1 ? 1 : tiles < WARP_MAX_GROUPS ? tiles : WARP_MAX_GROUPS);
  const bool lds_times = T <= INTERP_LDS_KNOTS;
  const bool vec = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)t) & 15) == 0;
  const size_t lds = lds_times ? (size_t)T * sizeof(double) : 0;
  static_assert((size_t)INTERP_LDS_KNOTS * sizeof(double) + WARP_TILE * 16 <= 64 * 1024,
                "LDS within the default limit: the launch needs no hipFuncSetAttribute");
  if (lds_times) {
    if (vec) hipLaunchKernelGGL((dsi_vote_kernel<true, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((dsi_vote_kernel<true, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((dsi_vote_kernel<false, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((dsi_vote_kernel<false, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  }
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(dsi_detect_kernel, dim3((unsigned)((HW + INTERP_THREADS - 1) / INTERP_THREADS)), dim3(INTERP_THREADS), 0, st,
                     a.dsi, range, w.ctr, D, (long)HW, w.best, w.inv, w.plane, status);
  RAMP_CHECK_LAUNCH();
  const unsigned tiles_xy = (unsigned)ramp_cdiv(W, DSI_TW) * (unsigned)ramp_cdiv(H, DSI_TH);
  hipLaunchKernelGGL(dsi_threshold_kernel, dim3(tiles_xy), dim3(INTERP_THREADS), 0, st, w.best, w.inv, w.plane, w.ctr, fill,
                     min_fixed, offset_fixed, adaptive_radius, H, W, invdepth, confidence, plane, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
