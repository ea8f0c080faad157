// Per-event optical flow (include/ramp_hip.h: ramp_event_flow): a local plane fit on the surface of active events at each
// event's own time (Benosman et al., "Event-based visual flow", TNNLS 2014), order-independent and bit-exact.  The definition
// is in the header.  The surface at an event's time is the filter's quantity -- per neighbour cell the last candidate that
// precedes the event, else the state -- over a (2r + 1)^2 window; the order stage is the filter's (order_device.h).
//
//   flow_key_kernel       one lane per event and trip: classes [2], [3]; the key is plane * H W + pixel, S H W otherwise
//   hipcub SortPairs      stable radix sort of (key, event index) over ceil(log2(S H W + 1)) bits
//   ord_segment_kernel    one lane per cell: the segment's start
//   flow_ts_kernel        per sorted position the time stamp (gathered once into ts[]) and the order check
//   flow_fit_kernel<R>    one lane per SORTED POSITION: (2r + 1)^2 - 1 bounded binary searches, the points' s values in a
//                         per-lane LDS slab [j][lane] with the used set as a 64-bit mask, the fit in exact integers and float64
//                         without FMA in ascending j, up to two refinement passes, the flow; everything written through the
//                         event index; class counts by ballots; the map's index by an int32 atomicMax
//   flow_finish_kernel    last_t_out per cell (a launch of its own: in place is allowed), flow_map per pixel from the winning
//                         index (one writer), the status words
//
// No floating-point atomics; every loop is a binary search or has a fixed trip count.
#include "workspace_cub.h"
#include "ramp_internal.h"
#include "order_device.h"

#define FLOW_CTR_WORDS 16                // int32: the 8 status words, 8 spare

// the workgroup of an instance: the slab is (2r + 1)^2 float64 per lane.  r = 1: 18 KiB, r = 2: 50 KiB at 256 lanes; r = 3 would
// be 98 KiB of the CU's 160 KiB -- one workgroup, four waves per CU -- so it runs 128 lanes at 49 KiB: three workgroups, six waves
template <int R> struct FlowShape {
  static constexpr int D = 2 * R + 1, P = D * D, THREADS = R == 3 ? 128 : 256;
};

template <bool I32>
__global__ void __launch_bounds__(INTERP_THREADS)
    flow_key_kernel(const void *__restrict__ xv, const void *__restrict__ yv, const double *__restrict__ t,
                    const int8_t *__restrict__ p, long N, int H, int W, uint32_t cells, uint32_t *__restrict__ key,
                    int32_t *__restrict__ iota, int32_t *__restrict__ ctr) {
  const int tid = threadIdx.x;
  const uint32_t HW = (uint32_t)H * (uint32_t)W;
  const long tiles = (N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n_seen = 0, n_bad = 0, n_out = 0;                  // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    const bool have = i < N;
    int c = 0;
    if (have) {
      uint32_t k = 0;
      c = ord_pixel(ord_coord<I32>(xv, i), ord_coord<I32>(yv, i), t[i], H, W, &k);
      if (c != 0) k = cells;
      else if (p && p[i] > 0) k += HW;
      key[i] = k;
      iota[i] = (int32_t)i;
    }
    n_seen += ramp_wave_count(have);
    n_bad += ramp_wave_count(c == 2);
    n_out += ramp_wave_count(c == 3);
  }
  ramp_wave_flush(ctr + 1, tid, n_seen, n_bad, n_out);
}

// ts[] and the order check: the neighbour in the segment, the segment's first entry against the state
__global__ void __launch_bounds__(INTERP_THREADS)
    flow_ts_kernel(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sidx, const double *__restrict__ t, int N,
                   uint32_t cells, const double *__restrict__ last_in, double *__restrict__ ts, int32_t *__restrict__ ctr) {
  const int tid = threadIdx.x;
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  bool bad = false;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    if (i >= (long)N) continue;
    const uint32_t k = skey[i];
    const double ti = t[sidx[i]];
    ts[i] = ti;
    if (k < cells) {
      double before = ord_nan();                           // (NaN: nothing in front, the comparison is false)
      if (i > 0 && skey[i - 1] == k) before = t[sidx[i - 1]];
      else if (last_in) before = last_in[k];
      bad = bad || ti < before;
    }
  }
  if (__ballot(bad) != 0 && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(&ctr[0], RAMP_FLOW_BAD_ORDER);
}

struct FlowArgs {
  const void *x, *y;
  const double *t;
  const uint32_t *skey;
  const int32_t *sidx, *start;
  const double *ts, *last_in;
  float *flow;
  uint8_t *cls_out, *n_used;
  double *fit;
  int32_t *map_index, *ctr;
  double window_dt, outlier_dt, max_speed;
  int N, H, W, planes, min_points, refine, i32;
};

template <int R>
__global__ void __launch_bounds__(FlowShape<R>::THREADS) flow_fit_kernel(const FlowArgs a) {
  constexpr int D = FlowShape<R>::D, P = FlowShape<R>::P, THREADS = FlowShape<R>::THREADS, CENTRE = R * D + R;
  __shared__ double s_slab[P][THREADS];                    // [j][lane]: a lane's points are THREADS apart, a wave's adjacent
  const int tid = threadIdx.x;
  const int N = a.N, H = a.H, W = a.W;
  const uint32_t HW = (uint32_t)H * (uint32_t)W, cells = HW * (uint32_t)a.planes;
  const bool failed = (a.ctr[0] & RAMP_FLOW_BAD_ORDER) != 0;
  const float qnan = __int_as_float(0x7fc00000);
  const long tiles = ((long)N + THREADS - 1) / THREADS;
  int n4 = 0, n5 = 0, n6 = 0, n7 = 0;                      // classes [4] .. [7], wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * THREADS + tid;
    int cls = 0;
    if (pos < (long)N) {
      const uint32_t k = a.skey[pos];
      const int32_t i = a.sidx[pos];
      int n = 0;
      double fa = ord_nan(), fb = ord_nan(), fc = ord_nan();
      float2 row = make_float2(qnan, qnan);
      if (failed) {
        cls = 0;
      } else if (k >= cells) {                             // counted by the key kernel: the class is found again for cls_out
        uint32_t unused;
        cls = a.i32 ? ord_pixel(ord_coord<true>(a.x, i), ord_coord<true>(a.y, i), a.t[i], H, W, &unused)
                    : ord_pixel(ord_coord<false>(a.x, i), ord_coord<false>(a.y, i), a.t[i], H, W, &unused);
      } else {
        const double ti = a.ts[pos];
        const uint32_t plane0 = k >= HW ? HW : 0u, pix = k - plane0;
        const int qy = (int)(pix / (uint32_t)W), qx = (int)(pix - (uint32_t)qy * (uint32_t)W);
        // the points: one bounded binary search per neighbour that lies on the sensor
        unsigned long long mask = 1ull << CENTRE;
#pragma unroll 1
        for (int j = 0; j < P; j++) {
          const int ny = qy + j / D - R, nx = qx + j % D - R;
          double s = 0.0;
          if (j != CENTRE) {
            if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            const uint32_t nb = plane0 + (uint32_t)ny * (uint32_t)W + (uint32_t)nx;
            const double delta = ti - ord_last_before(a.ts, a.sidx, a.start, a.last_in, nb, ti, i);
            if (!(delta <= a.window_dt)) continue;
            s = -delta;
            mask |= 1ull << j;
          }
          s_slab[j][tid] = s;
        }
        // the fit, and up to `refine` passes that drop outliers and fit again
        double vx = 0.0, vy = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 3; pass++) {
          int Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
          double Sxs = 0.0, Sys = 0.0, Ss = 0.0;
          n = 0;
#pragma unroll 1
          for (int row = 0; row < D; row++) {              // (a row of the window per trip: a few lane masks live, not (2r + 1)^2)
            const int dy = row - R;
#pragma unroll
            for (int col = 0; col < D; col++) {
              const int dx = col - R, j = row * D + col;
              if ((mask >> j) & 1ull) {
                const double s = s_slab[j][tid];
                n += 1; Sx += dx; Sy += dy; Sxx += dx * dx; Sxy += dx * dy; Syy += dy * dy;
                Sxs = Sxs + (double)dx * s;
                Sys = Sys + (double)dy * s;
                Ss = Ss + s;
              }
            }
          }
          if (n < a.min_points) { cls = 4; break; }
          const long long C00 = (long long)Syy * n - (long long)Sy * Sy, C01 = (long long)Sx * Sy - (long long)Sxy * n,
                          C02 = (long long)Sxy * Sy - (long long)Syy * Sx, C11 = (long long)Sxx * n - (long long)Sx * Sx,
                          C12 = (long long)Sxy * Sx - (long long)Sxx * Sy, C22 = (long long)Sxx * Syy - (long long)Sxy * Sxy;
          const long long Det = Sxx * C00 + Sxy * C01 + Sx * C02;
          if (Det == 0) { cls = 5; break; }
          const double dd = (double)Det;
          fa = (((double)C00 * Sxs + (double)C01 * Sys) + (double)C02 * Ss) / dd;
          fb = (((double)C01 * Sxs + (double)C11 * Sys) + (double)C12 * Ss) / dd;
          fc = (((double)C02 * Sxs + (double)C12 * Sys) + (double)C22 * Ss) / dd;
          cls = 7;
          if (pass == a.refine) break;
          unsigned long long kept = mask;
#pragma unroll 1
          for (int row = 0; row < D; row++) {
            const int dy = row - R;
#pragma unroll
            for (int col = 0; col < D; col++) {
              const int dx = col - R, j = row * D + col;
              if (j != CENTRE && ((mask >> j) & 1ull)) {
                const double res = s_slab[j][tid] - ((fa * (double)dx + fb * (double)dy) + fc);
                if (fabs(res) > a.outlier_dt) kept &= ~(1ull << j);
              }
            }
          }
          if (kept == mask) break;
          mask = kept;
        }
        if (cls == 7) {
          const double g2 = fa * fa + fb * fb;
          vx = fa / g2;
          vy = fb / g2;
          if (!(g2 > 0.0) || !interp_finite(vx) || !interp_finite(vy) || vx * vx + vy * vy > a.max_speed * a.max_speed) cls = 6;
          else row = make_float2((float)vx, (float)vy);
        } else {
          fa = fb = fc = ord_nan();
        }
        if (cls == 7 && a.map_index) atomicMax(&a.map_index[pix], i);
      }
      reinterpret_cast<float2 *>(a.flow)[i] = row;
      if (a.cls_out) a.cls_out[i] = (uint8_t)cls;
      if (a.n_used) a.n_used[i] = (uint8_t)n;
      if (a.fit) { a.fit[3 * (size_t)i] = fa; a.fit[3 * (size_t)i + 1] = fb; a.fit[3 * (size_t)i + 2] = fc; }
    }
    n4 += ramp_wave_count(cls == 4);
    n5 += ramp_wave_count(cls == 5);
    n6 += ramp_wave_count(cls == 6);
    n7 += ramp_wave_count(cls == 7);
  }
  ramp_wave_flush(a.ctr + 4, tid, n4, n5, n6, n7);
}

// lanes [0, cells): last_t_out; lanes [0, H W): flow_map from the winning index; the status words
__global__ void __launch_bounds__(INTERP_THREADS)
    flow_finish_kernel(const int32_t *__restrict__ start, const double *__restrict__ ts, uint32_t cells, uint32_t HW,
                       const double *last_in, double *last_out, const float *__restrict__ flow,
                       const int32_t *__restrict__ map_index, float *__restrict__ flow_map, const int32_t *__restrict__ ctr,
                       int32_t *__restrict__ status) {
  const bool failed = (ctr[0] & RAMP_FLOW_BAD_ORDER) != 0;
  const float qnan = __int_as_float(0x7fc00000);
  const long tiles = ((long)cells + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long q = tile * INTERP_THREADS + threadIdx.x;
    if (last_out && q < (long)cells) {
      const int s0 = start[q], s1 = start[q + 1];
      double v = last_in ? last_in[q] : ord_nan();         // (in place: a lane reads and writes its own cell alone)
      if (s1 > s0) v = ts[s1 - 1];
      last_out[q] = failed ? ord_nan() : v;
    }
    if (flow_map && q < (long)HW) {
      const int32_t w = map_index[q];
      flow_map[q] = w >= 0 ? flow[2 * (size_t)w] : qnan;
      flow_map[(size_t)HW + q] = w >= 0 ? flow[2 * (size_t)w + 1] : qnan;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const int w = threadIdx.x;
    status[w] = (failed && w >= 4) ? 0 : ctr[w];
  }
}

// the workspace: the counters; the two key and the two index arrays, ts, start, the library's own
struct FlowWs {
  int32_t *ctr;
  uint32_t *key, *skey;
  int32_t *iota, *sidx, *start;
  double *ts;
  void *cub;
  size_t cub_bytes;
};

static size_t flow_carve(void *ws, long N, long cells, FlowWs *w) {
  WsCarver c(ws);
  const size_t n = (size_t)(N > 0 ? N : 1);
  w->ctr = c.take<int32_t>(FLOW_CTR_WORDS, 256);
  w->key = c.take<uint32_t>(n, 256);
  w->skey = c.take<uint32_t>(n, 256);
  w->iota = c.take<int32_t>(n, 256);
  w->sidx = c.take<int32_t>(n, 256);
  w->ts = c.take<double>(n, 256);
  w->start = c.take<int32_t>((size_t)cells + 2, 256);
  w->cub_bytes = ws_cub_bytes<uint32_t>((int)n, 32);
  w->cub = c.take<char>(w->cub_bytes, 256);
  return c.bytes();
}

template <int R> static void flow_launch(const FlowArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((flow_fit_kernel<R>), dim3(ord_grid(a.N, FlowShape<R>::THREADS)), dim3(FlowShape<R>::THREADS), 0, st, a);
}

static bool flow_size_ok(long N, int H, int W, int planes) {
  return N >= 0 && N <= 2147483647L && H >= 1 && W >= 1 && (planes == 1 || planes == 2) &&
         2.0 * (double)H * (double)W < 2147483647.0;
}

extern "C" {
size_t ramp_event_flow_ws_bytes(long N, int H, int W, int planes) {
  if (!flow_size_ok(N, H, W, planes)) return 0;
  FlowWs w;
  return flow_carve(nullptr, N, (long)planes * H * W, &w);
}

long ramp_event_flow_grid_events(void) { return (long)ORD_MAX_GROUPS * INTERP_THREADS; }

int ramp_event_flow(const void *x, const void *y, const double *t, const int8_t *p, long N, int H, int W, int flags, int r,
                    double window_dt, int min_points, int refine, double outlier_dt, double max_speed, const double *last_t_in,
                    double *last_t_out, float *flow, uint8_t *cls, uint8_t *n_used, double *fit, float *flow_map,
                    int32_t *map_index, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
  if (N < 0 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~RAMP_FLOW_XY_I32) return RAMP_EINVAL;
  if (r < 1 || r > 3 || min_points < 3 || min_points > (2 * r + 1) * (2 * r + 1) || refine < 0 || refine > 2) return RAMP_EINVAL;
  if (!(window_dt >= 0.0) || !(outlier_dt >= 0.0) || !(max_speed > 0.0)) return RAMP_EINVAL;
  if (!status || (N > 0 && !flow) || (flow_map == nullptr) != (map_index == nullptr)) return RAMP_EINVAL;
  if ((((uintptr_t)flow | (uintptr_t)last_t_in | (uintptr_t)last_t_out | (uintptr_t)fit) & 7) != 0 ||
      (((uintptr_t)status | (uintptr_t)flow_map | (uintptr_t)map_index) & 3) != 0)
    return RAMP_EINVAL;
  if (N > 2147483647L || 2.0 * (double)H * (double)W >= 2147483647.0) return RAMP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int planes = p ? 2 : 1;
  const long HWl = (long)H * W, cellsl = HWl * planes;
  if (N == 0) {                                            // no launch: memsets and a copy
    if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    if (flow_map && (hipMemsetD32Async((hipDeviceptr_t)flow_map, 0x7fc00000, (size_t)(2 * HWl), st) != hipSuccess ||
                     hipMemsetAsync(map_index, 0xff, (size_t)HWl * sizeof(int32_t), st) != hipSuccess))
      return RAMP_ELAUNCH;
    if (last_t_in && last_t_out && last_t_in != last_t_out &&
        hipMemcpyAsync(last_t_out, last_t_in, (size_t)cellsl * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return RAMP_ELAUNCH;
    return RAMP_OK;
  }
  if (!x || !y || !t || !ws) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)t & 7) != 0 || (((uintptr_t)x | (uintptr_t)y) & 3) != 0) return RAMP_EINVAL;
  FlowWs w;
  if (ws_bytes < flow_carve(ws, N, cellsl, &w)) return RAMP_EWORKSPACE;
  const uint32_t HW = (uint32_t)HWl, cells = (uint32_t)cellsl;
  const int n = (int)N;
  const bool i32 = (flags & RAMP_FLOW_XY_I32) != 0;
  if (hipMemsetAsync(w.ctr, 0, FLOW_CTR_WORDS * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  if (map_index && hipMemsetAsync(map_index, 0xff, (size_t)HWl * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;   // -1
  if (i32) hipLaunchKernelGGL((flow_key_kernel<true>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, p, N, H, W, cells, w.key, w.iota, w.ctr);
  else hipLaunchKernelGGL((flow_key_kernel<false>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, p, N, H, W, cells, w.key, w.iota, w.ctr);
  RAMP_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.key, w.skey, w.iota, w.sidx, n, 0, ord_sort_bits(cells), st) != hipSuccess)
    return RAMP_ELAUNCH;
  hipLaunchKernelGGL(ord_segment_kernel, dim3(ord_grid(cellsl + 2)), dim3(INTERP_THREADS), 0, st, w.skey, n, cells, w.start);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(flow_ts_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, w.skey, w.sidx, t, n, cells, last_t_in, w.ts, w.ctr);
  RAMP_CHECK_LAUNCH();
  FlowArgs a;
  a.x = x; a.y = y; a.t = t; a.skey = w.skey; a.sidx = w.sidx; a.start = w.start; a.ts = w.ts; a.last_in = last_t_in;
  a.flow = flow; a.cls_out = cls; a.n_used = n_used; a.fit = fit; a.map_index = map_index; a.ctr = w.ctr;
  a.window_dt = window_dt; a.outlier_dt = outlier_dt; a.max_speed = max_speed;
  a.N = n; a.H = H; a.W = W; a.planes = planes; a.min_points = min_points; a.refine = refine; a.i32 = i32 ? 1 : 0;
  if (r == 1) flow_launch<1>(a, st);
  else if (r == 2) flow_launch<2>(a, st);
  else flow_launch<3>(a, st);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(flow_finish_kernel, dim3(ord_grid(last_t_out || flow_map ? cellsl : 1)), dim3(INTERP_THREADS), 0, st, w.start,
                     w.ts, cells, HW, last_t_in, last_t_out, flow, map_index, flow_map, w.ctr, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
