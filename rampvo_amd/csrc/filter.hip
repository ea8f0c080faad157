// Event denoising (include/ramp_hip.h: ramp_event_filter): a hot-pixel mask, a refractory period and the 8-neighbour
// background-activity filter over one event list, order-independent and bit-exact.  The definition is in the header; on a
// globally time-sorted stream it is, event for event, the textbook sequential filter over a last-time-stamp map.
//
// The pipeline is fixed, so that the result is a pure function of the input:
//   flt_key_kernel        one lane per event and trip: classes [2], [3]; the key is the pixel index of a candidate, H W otherwise
//   hipcub SortPairs      stable radix sort of (key, event index) over ceil(log2(H W + 1)) bits: every pixel's candidates become
//                         one segment, in index order
//   ord_segment_kernel    one lane per pixel: the segment's start, a binary search over the sorted keys (counts are differences)
//   flt_hot_sums_kernel   per sorted position the time stamp (gathered once into ts[]) and the order check -- the neighbour in
//                         the segment, the segment's first entry against the state --; per pixel n and S2 as integer sums
//   flt_hot_mask_kernel   the threshold in float64 (no FMA), the mask, the stats row
//   flt_filter_kernel     one lane per SORTED POSITION: a wave's lanes sit on the same and adjacent pixels and share the neighbour
//                         segments they search; the own predecessor at position - 1, eight bounded binary searches, the class
//                         written through the event index; class counts by ballots, one LDS reduction per workgroup in front of
//                         the int32 atomics
//   hipcub InclusiveSum   over the keep flags, and flt_compact_kernel: index_out (only when it is asked for)
//   flt_finish_kernel     last_t_out (a launch of its own behind the filter: in place is allowed), the status words, count_out
//
// No floating-point atomics; every loop is a binary search or has a fixed trip count.  Within a segment the index rises and the
// time stamp does not fall (the order check), so (t, index) rises lexicographically and "the last entry that precedes the
// event" is a partition point.
#include "workspace_cub.h"
#include "ramp_internal.h"
#include "order_device.h"                // the order stage shared with flow.hip: candidate test, segments, the search

#define FLT_WAVES (INTERP_THREADS / RAMP_WAVE)
#define FLT_CTR_WORDS 16                 // int32: the 8 status words, 8 spare; behind them two int64: n, S2

template <bool I32>
__global__ void __launch_bounds__(INTERP_THREADS)
    flt_key_kernel(const void *__restrict__ xv, const void *__restrict__ yv, const double *__restrict__ t, long N, int H, int W,
                   uint32_t *__restrict__ key, int32_t *__restrict__ iota, int32_t *__restrict__ ctr) {
  const int tid = threadIdx.x;
  const uint32_t HW = (uint32_t)H * (uint32_t)W;
  const long tiles = (N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n_seen = 0, n_bad = 0, n_out = 0;                  // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    const bool have = i < N;
    bool bad = false, outside = false;
    if (have) {
      const float x = ord_coord<I32>(xv, i), y = ord_coord<I32>(yv, i);
      uint32_t k = HW;
      const int c = ord_pixel(x, y, t[i], H, W, &k);
      bad = c == 2;
      outside = c == 3;
      key[i] = k;
      iota[i] = (int32_t)i;
    }
    n_seen += ramp_wave_count(have);
    n_bad += ramp_wave_count(bad);
    n_out += ramp_wave_count(outside);
  }
  ramp_wave_flush(ctr + 1, tid, n_seen, n_bad, n_out);
}

// lanes [0, N): sorted positions -- ts[] and the order check; lanes [0, H W): pixels -- n and S2
__global__ void __launch_bounds__(INTERP_THREADS)
    flt_hot_sums_kernel(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sidx, const double *__restrict__ t, int N,
                        uint32_t HW, const int32_t *__restrict__ start, const double *__restrict__ last_in,
                        double *__restrict__ ts, int32_t *__restrict__ ctr, unsigned long long *__restrict__ sums) {
  const int tid = threadIdx.x;
  const long lanes = (long)N > (long)HW ? (long)N : (long)HW;
  const long tiles = (lanes + INTERP_THREADS - 1) / INTERP_THREADS;
  unsigned long long n = 0, s2 = 0;
  bool bad = false;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    if (i < (long)N) {
      const uint32_t k = skey[i];
      const double ti = t[sidx[i]];
      ts[i] = ti;
      if (k < HW) {
        double before = ord_nan();                         // (NaN: nothing in front, the comparison is false)
        if (i > 0 && skey[i - 1] == k) before = t[sidx[i - 1]];
        else if (last_in) before = last_in[k];
        bad = bad || ti < before;
      }
    }
    if (i < (long)HW) {
      const unsigned long long c = (unsigned long long)(start[i + 1] - start[i]);
      n += c != 0;
      s2 += c * c;
    }
  }
#pragma unroll
  for (int off = RAMP_WAVE / 2; off > 0; off >>= 1) {    // (two sums in one butterfly: ramp_wave_sum, interleaved)
    n += __shfl_xor(n, off);
    s2 += __shfl_xor(s2, off);
  }
  if ((tid & (RAMP_WAVE - 1)) == 0) {
    if (n) atomicAdd(&sums[0], n);
    if (s2) atomicAdd(&sums[1], s2);
  }
  if (__ballot(bad) != 0 && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(&ctr[0], RAMP_FILTER_BAD_ORDER);
}

__global__ void __launch_bounds__(INTERP_THREADS)
    flt_hot_mask_kernel(const int32_t *__restrict__ start, uint32_t HW, const unsigned long long *__restrict__ sums,
                        const int32_t *__restrict__ ctr, int hot_count, double hot_sigma, const uint8_t *__restrict__ hot_in,
                        uint8_t *__restrict__ hot, uint8_t *__restrict__ hot_out, double *__restrict__ stats_out) {
  const long long n = (long long)sums[0], S2 = (long long)sums[1], S1 = (long long)start[HW];
  const bool sigma = hot_sigma > 0.0;
  double mean = ord_nan(), sd = ord_nan(), thr = ord_nan();
  if (n > 0) {                                             // float64, in this order, no FMA (the unit is built without contraction)
    mean = (double)S1 / (double)n;
    const double v = (double)S2 / (double)n - mean * mean;
    sd = sqrt(v > 0.0 ? v : 0.0);
    if (sigma) thr = mean + hot_sigma * sd;
  }
  const long tiles = ((long)HW + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long q = tile * INTERP_THREADS + threadIdx.x;
    if (q >= (long)HW) continue;
    const int c = start[q + 1] - start[q];
    const bool h = (hot_count > 0 && c > hot_count) || (sigma && (double)c > thr) || (hot_in && hot_in[q] != 0);
    hot[q] = h ? 1 : 0;
    if (hot_out) hot_out[q] = h ? 1 : 0;
  }
  if (stats_out && blockIdx.x == 0 && threadIdx.x == 0) {
    const bool failed = (ctr[0] & RAMP_FILTER_BAD_ORDER) != 0;
    stats_out[0] = failed ? ord_nan() : (double)n;
    stats_out[1] = failed ? ord_nan() : mean;
    stats_out[2] = failed ? ord_nan() : sd;
    stats_out[3] = failed ? ord_nan() : thr;
  }
}

struct FltArgs {
  const void *x, *y;
  const uint32_t *skey;
  const int32_t *sidx, *start;
  const double *ts, *last_in;
  const uint8_t *hot;
  uint8_t *keep_out;
  float *xy_out;
  int32_t *keep32, *ctr;
  double support_dt, refractory;
  int N, H, W;
};

template <bool I32>
__global__ void __launch_bounds__(INTERP_THREADS) flt_filter_kernel(const FltArgs a) {
  __shared__ int s_cnt[FLT_WAVES][4];
  const int tid = threadIdx.x;
  const int N = a.N, H = a.H, W = a.W;
  const uint32_t HW = (uint32_t)H * (uint32_t)W;
  const bool failed = (a.ctr[0] & RAMP_FILTER_BAD_ORDER) != 0;
  const bool activity = a.support_dt >= 0.0, refr = a.refractory > 0.0;
  const float qnan = __int_as_float(0x7fc00000);
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n_cls[4] = {0, 0, 0, 0};                             // classes [4] .. [7], wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + tid;
    int cls = 0;
    if (pos < (long)N) {
      const uint32_t k = a.skey[pos];
      const int32_t i = a.sidx[pos];
      if (k < HW && !failed) {
        const double ti = a.ts[pos];
        if (a.hot[k]) {
          cls = 4;
        } else {
          const double t_own = pos > (long)a.start[k] ? a.ts[pos - 1] : (a.last_in ? a.last_in[k] : ord_nan());
          if (refr && ti - t_own < a.refractory) {
            cls = 5;
          } else if (activity) {
            const int qy = (int)(k / (uint32_t)W), qx = (int)(k - (uint32_t)qy * (uint32_t)W);
            bool sup = false;
#pragma unroll 1
            for (int j = 0; j < 9; j++) {
              const int ny = qy + j / 3 - 1, nx = qx + j % 3 - 1;
              if (j == 4 || sup || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
              const uint32_t nb = (uint32_t)ny * (uint32_t)W + (uint32_t)nx;
              if (a.hot[nb]) continue;
              const double t_nb = ord_last_before(a.ts, a.sidx, a.start, a.last_in, nb, ti, i);
              sup = ti - t_nb <= a.support_dt;
            }
            cls = sup ? 7 : 6;
          } else {
            cls = 7;
          }
        }
      }
      const bool keep = cls == 7;
      a.keep_out[i] = keep ? 1 : 0;
      if (a.keep32) a.keep32[i] = keep ? 1 : 0;
      if (a.xy_out) {
        const float2 row = keep ? make_float2(ord_coord<I32>(a.x, i), ord_coord<I32>(a.y, i)) : make_float2(qnan, qnan);
        reinterpret_cast<float2 *>(a.xy_out)[i] = row;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) n_cls[c] += ramp_wave_count(cls == 4 + c);
  }
  if ((tid & (RAMP_WAVE - 1)) == 0) {
#pragma unroll
    for (int c = 0; c < 4; c++) s_cnt[tid / RAMP_WAVE][c] = n_cls[c];
  }
  __syncthreads();
  if (tid < 4) {                                           // one integer atomic per workgroup and counter that is not zero
    int v = 0;
#pragma unroll
    for (int w = 0; w < FLT_WAVES; w++) v += s_cnt[w][tid];
    if (v) atomicAdd(&a.ctr[4 + tid], v);
  }
}

// incl: the inclusive sums of keep32.  The kept events' indices in ascending order, -1 behind them
__global__ void __launch_bounds__(INTERP_THREADS)
    flt_compact_kernel(const int32_t *__restrict__ keep32, const int32_t *__restrict__ incl, int N, int32_t *__restrict__ index_out) {
  const int K = incl[N - 1];
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + threadIdx.x;
    if (i >= (long)N) continue;
    if (keep32[i]) index_out[incl[i] - 1] = (int32_t)i;    // (incl[i] - 1 < K: disjoint from the lanes that write -1)
    if (i >= (long)K) index_out[i] = -1;
  }
}

// per non-hot pixel its last candidate's time stamp, else the state; the status words; count_out
__global__ void __launch_bounds__(INTERP_THREADS)
    flt_finish_kernel(const int32_t *__restrict__ start, const double *__restrict__ ts, const uint8_t *__restrict__ hot,
                      uint32_t HW, const double *last_in, double *last_out, const int32_t *__restrict__ ctr,
                      int64_t *__restrict__ count_out, int32_t *__restrict__ status) {
  const bool failed = (ctr[0] & RAMP_FILTER_BAD_ORDER) != 0;
  if (last_out) {
    const long tiles = ((long)HW + INTERP_THREADS - 1) / INTERP_THREADS;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      const long q = tile * INTERP_THREADS + threadIdx.x;
      if (q >= (long)HW) continue;
      const int s0 = start[q], s1 = start[q + 1];
      double v = last_in ? last_in[q] : ord_nan();         // (in place: a lane reads and writes its own pixel alone)
      if (s1 > s0 && !hot[q]) v = ts[s1 - 1];
      last_out[q] = failed ? ord_nan() : v;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const int w = threadIdx.x;
    status[w] = (failed && w >= 4) ? 0 : ctr[w];
  }
  if (count_out && blockIdx.x == 0 && threadIdx.x == 0) *count_out = failed ? 0 : (int64_t)ctr[7];
}

// the workspace: counters and, adjacent, the two sums (one memset clears both); the two key and the two index arrays, ts, start,
// hot, the library's own
struct FltWs {
  int32_t *ctr;
  unsigned long long *sums;
  uint32_t *key, *skey;
  int32_t *iota, *sidx, *start;
  double *ts;
  uint8_t *hot;
  void *cub;
  size_t cub_bytes;
};

static size_t flt_carve(void *ws, long N, long HW, FltWs *w) {
  WsCarver c(ws);
  const size_t n = (size_t)(N > 0 ? N : 1);
  w->ctr = c.take<int32_t>(FLT_CTR_WORDS, 1);
  w->sums = c.take<unsigned long long>(2, 256);
  w->key = c.take<uint32_t>(n, 256);
  w->skey = c.take<uint32_t>(n, 256);
  w->iota = c.take<int32_t>(n, 256);
  w->sidx = c.take<int32_t>(n, 256);
  w->ts = c.take<double>(n, 256);
  w->start = c.take<int32_t>((size_t)HW + 2, 256);
  w->hot = c.take<uint8_t>((size_t)HW, 256);
  w->cub_bytes = ws_cub_bytes<uint32_t>((int)n, 32);
  w->cub = c.take<char>(w->cub_bytes, 256);
  return c.bytes();
}

extern "C" {
size_t ramp_event_filter_workspace_bytes(long N, int H, int W) {
  if (N < 0 || N > 2147483647L || H < 1 || W < 1 || (double)H * (double)W >= 2147483647.0) return 0;
  FltWs w;
  return flt_carve(nullptr, N, (long)H * W, &w);
}

long ramp_event_filter_grid_events(void) { return (long)ORD_MAX_GROUPS * INTERP_THREADS; }

int ramp_event_filter(const void *x, const void *y, const double *t, long N, int H, int W, int flags, double support_dt,
                      double refractory, int hot_count, double hot_sigma, const uint8_t *hot_in, const double *last_t_in,
                      double *last_t_out, uint8_t *keep_out, float *xy_out, int32_t *index_out, int64_t *count_out,
                      uint8_t *hot_out, double *stats_out, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
  if (N < 0 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~RAMP_FILTER_XY_I32) return RAMP_EINVAL;
  if (!(refractory >= 0.0) || !(fabs(refractory) <= 1.7976931348623157e308) || !(fabs(support_dt) <= 1.7976931348623157e308))
    return RAMP_EINVAL;
  if (!keep_out || !status) return RAMP_EINVAL;
  if ((((uintptr_t)xy_out | (uintptr_t)last_t_in | (uintptr_t)last_t_out | (uintptr_t)stats_out | (uintptr_t)count_out) & 7) != 0 ||
      (((uintptr_t)status | (uintptr_t)index_out) & 3) != 0)
    return RAMP_EINVAL;
  if (N > 2147483647L || (double)H * (double)W >= 2147483647.0) return RAMP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long HWl = (long)H * W;
  if (N == 0) {
    if (last_t_in && last_t_out && last_t_in != last_t_out &&
        hipMemcpyAsync(last_t_out, last_t_in, (size_t)HWl * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return RAMP_ELAUNCH;
    return RAMP_OK;
  }
  if (!x || !y || !t || !ws) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)t & 7) != 0 || (((uintptr_t)x | (uintptr_t)y) & 3) != 0) return RAMP_EINVAL;
  FltWs w;
  if (ws_bytes < flt_carve(ws, N, HWl, &w)) return RAMP_EWORKSPACE;
  const uint32_t HW = (uint32_t)HWl;
  const int n = (int)N;
  const bool i32 = (flags & RAMP_FILTER_XY_I32) != 0;
  if (hipMemsetAsync(w.ctr, 0, ws_span(w.ctr, w.sums + 2), st) != hipSuccess) return RAMP_ELAUNCH;
  if (i32) hipLaunchKernelGGL((flt_key_kernel<true>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, N, H, W, w.key, w.iota, w.ctr);
  else hipLaunchKernelGGL((flt_key_kernel<false>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, N, H, W, w.key, w.iota, w.ctr);
  RAMP_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.key, w.skey, w.iota, w.sidx, n, 0, ord_sort_bits(HW), st) != hipSuccess)
    return RAMP_ELAUNCH;
  hipLaunchKernelGGL(ord_segment_kernel, dim3(ord_grid(HWl + 2)), dim3(INTERP_THREADS), 0, st, w.skey, n, HW, w.start);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(flt_hot_sums_kernel, dim3(ord_grid(N > HWl ? N : HWl)), dim3(INTERP_THREADS), 0, st, w.skey, w.sidx, t, n, HW,
                     w.start, last_t_in, w.ts, w.ctr, w.sums);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(flt_hot_mask_kernel, dim3(ord_grid(HWl)), dim3(INTERP_THREADS), 0, st, w.start, HW, w.sums, w.ctr, hot_count,
                     hot_sigma, hot_in, w.hot, hot_out, stats_out);
  RAMP_CHECK_LAUNCH();
  // the sort's inputs are dead behind it: the keep flags and their sums take their place
  int32_t *keep32 = index_out ? (int32_t *)w.key : nullptr, *incl = w.iota;
  FltArgs a;
  a.x = x; a.y = y; a.skey = w.skey; a.sidx = w.sidx; a.start = w.start; a.ts = w.ts; a.last_in = last_t_in; a.hot = w.hot;
  a.keep_out = keep_out; a.xy_out = xy_out; a.keep32 = keep32; a.ctr = w.ctr; a.support_dt = support_dt;
  a.refractory = refractory; a.N = n; a.H = H; a.W = W;
  if (i32) hipLaunchKernelGGL((flt_filter_kernel<true>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, a);
  else hipLaunchKernelGGL((flt_filter_kernel<false>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, a);
  RAMP_CHECK_LAUNCH();
  if (index_out) {
    cb = w.cub_bytes;
    if (hipcub::DeviceScan::InclusiveSum(w.cub, cb, keep32, incl, n, st) != hipSuccess) return RAMP_ELAUNCH;
    hipLaunchKernelGGL(flt_compact_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, keep32, incl, n, index_out);
    RAMP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(flt_finish_kernel, dim3(last_t_out ? ord_grid(HWl) : 1), dim3(INTERP_THREADS), 0, st, w.start, w.ts, w.hot, HW,
                     last_t_in, last_t_out, w.ctr, count_out, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
