// Event corner detection (include/ramp_hip.h: ramp_event_corners): FAST-style arcs of newest events on the surface of active
// events at each event's own time (Mueggler et al., "Fast Event-based Corner Detection", BMVC 2017; Arc*: Alzugaray and Chli,
// RA-L 2018), order-independent and bit-exact.  The definition is in the header.  The surface at an event's time is the filter's
// and the flow's quantity -- per circle cell the last candidate that precedes the event, else the state -- and the order stage
// is theirs (order_device.h).  No floating-point arithmetic at all: time stamps are only compared.
//
//   crn_key_kernel        one lane per event and trip: classes [2], [3]; the key is plane * H W + pixel, S H W otherwise
//   hipcub SortPairs      stable radix sort of (key, event index) over ceil(log2(S H W + 1)) bits
//   ord_segment_kernel    one lane per cell: the segment's start
//   crn_ts_kernel         per sorted position the time stamp (gathered once into ts[]) and the order check
//   crn_corner_kernel     one lane per SORTED POSITION: class [4]; 16 bounded binary searches into registers and the inner arc
//                         test; for the lanes whose inner circle passed 20 more and the outer test; everything written through
//                         the event index; class counts by ballots; corner_count by an int32 atomicAdd
//   hipcub InclusiveSum   only with `index`: the running count of corners in index order
//   crn_finish_kernel     last_t_out per cell (a launch of its own: in place is allowed), index from the running counts, count,
//                         the status words
// (crn_key_kernel and crn_ts_kernel are flow.hip's statements, kept as a copy: flow.hip, filter.hip and order_device.h are
// untouched.)  No floating-point atomics; every loop is a binary search or has a fixed trip count.
#include "workspace_cub.h"
#include "ramp_internal.h"
#include "order_device.h"

#define CRN_CTR_WORDS 16                 // int32: the 8 status words, 8 spare
#define CRN_INNER 16
#define CRN_OUTER 20

// the circles, index ascending along each list (the header's order)
__device__ static constexpr int8_t CRN_INNER_DX[CRN_INNER] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__device__ static constexpr int8_t CRN_INNER_DY[CRN_INNER] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
__device__ static constexpr int8_t CRN_OUTER_DX[CRN_OUTER] = {0, 1, 2, 3, 4, 4, 4, 3, 2, 1, 0, -1, -2, -3, -4, -4, -4, -3, -2, -1};
__device__ static constexpr int8_t CRN_OUTER_DY[CRN_OUTER] = {4, 4, 3, 2, 1, 0, -1, -2, -3, -4, -4, -4, -3, -2, -1, 0, 1, 2, 3, 4};

template <bool I32>
__global__ void __launch_bounds__(INTERP_THREADS)
    crn_key_kernel(const void *__restrict__ xv, const void *__restrict__ yv, const double *__restrict__ t,
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
    crn_ts_kernel(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sidx, const double *__restrict__ t, int N,
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
  if (__ballot(bad) != 0 && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(&ctr[0], RAMP_CORNER_BAD_ORDER);
}

// The arc test of one circle of NP values held in registers -> start | L << 8 of the reported arc, 0 when none passes.  For
// every element e with a number, m_e = {k : v[k] >= v[e]} (a NaN is in no set and gives the empty set); an arc passes exactly
// when it is some m_e, so: m_e is one cyclic run (one bit whose predecessor is clear) of an allowed length; the sets are
// nested, so the shortest is the one of the smallest popcount, and its start is that one bit.
template <int NP>
static __device__ __forceinline__ uint32_t crn_arc(const double (&v)[NP], int lo, int hi, bool wide) {
  constexpr uint32_t FULL = (1u << NP) - 1u;
  int best_l = NP;
  uint32_t best_first = 0;
#pragma unroll
  for (int e = 0; e < NP; e++) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < NP; k++) m |= v[k] >= v[e] ? 1u << k : 0u;
    const uint32_t first = m & ~(((m << 1) | (m >> (NP - 1))) & FULL);
    const int l = __popc(m);
    const bool allowed = (l >= lo && l <= hi) || (wide && NP - l >= lo && NP - l <= hi);
    if (allowed && __popc(first) == 1 && l < best_l) { best_l = l; best_first = first; }
  }
  return best_first ? (uint32_t)(__ffs((int)best_first) - 1) | (uint32_t)best_l << 8 : 0u;
}

struct CrnArgs {
  const void *x, *y;
  const double *t;
  const uint32_t *skey;
  const int32_t *sidx, *start;
  const double *ts, *last_in;
  uint8_t *cls_out;
  uint32_t *arc;                                           // [N] words: inner start, inner L, outer start, outer L from the low byte
  int32_t *flag32, *corner_count, *ctr;
  int N, H, W, planes, inner_lo, inner_hi, outer_lo, outer_hi, wide, i32;
};

__global__ void __launch_bounds__(INTERP_THREADS) crn_corner_kernel(const CrnArgs a) {
  const int tid = threadIdx.x;
  const int N = a.N, H = a.H, W = a.W;
  const uint32_t HW = (uint32_t)H * (uint32_t)W, cells = HW * (uint32_t)a.planes;
  const bool failed = (a.ctr[0] & RAMP_CORNER_BAD_ORDER) != 0, wide = a.wide != 0;
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n4 = 0, n5 = 0, n6 = 0, n7 = 0;                      // classes [4] .. [7], wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + tid;
    int cls = 0;
    if (pos < (long)N) {
      const uint32_t k = a.skey[pos];
      const int32_t i = a.sidx[pos];
      uint32_t arc = 0;
      if (failed) {
        cls = 0;
      } else if (k >= cells) {                             // counted by the key kernel: the class is found again for cls_out
        uint32_t unused;
        cls = a.i32 ? ord_pixel(ord_coord<true>(a.x, i), ord_coord<true>(a.y, i), a.t[i], H, W, &unused)
                    : ord_pixel(ord_coord<false>(a.x, i), ord_coord<false>(a.y, i), a.t[i], H, W, &unused);
      } else {
        const uint32_t plane0 = k >= HW ? HW : 0u, pix = k - plane0;
        const int qy = (int)(pix / (uint32_t)W), qx = (int)(pix - (uint32_t)qy * (uint32_t)W);
        if (qx < 4 || qy < 4 || qx > W - 5 || qy > H - 5) {
          cls = 4;                                         // the outer circle leaves the sensor: below, every circle pixel is on it
        } else {
          const double ti = a.ts[pos];
          double v[CRN_INNER];
#pragma unroll
          for (int j = 0; j < CRN_INNER; j++)
            v[j] = ord_last_before(a.ts, a.sidx, a.start, a.last_in, (uint32_t)((int)k + CRN_INNER_DY[j] * W + CRN_INNER_DX[j]), ti, i);
          arc = crn_arc<CRN_INNER>(v, a.inner_lo, a.inner_hi, wide);
          cls = 5;
          if (arc) {
            double u[CRN_OUTER];
#pragma unroll
            for (int j = 0; j < CRN_OUTER; j++)
              u[j] = ord_last_before(a.ts, a.sidx, a.start, a.last_in, (uint32_t)((int)k + CRN_OUTER_DY[j] * W + CRN_OUTER_DX[j]), ti, i);
            const uint32_t outer = crn_arc<CRN_OUTER>(u, a.outer_lo, a.outer_hi, wide);
            arc |= outer << 16;
            cls = outer ? 7 : 6;
          }
          if (cls == 7 && a.corner_count) atomicAdd(&a.corner_count[pix], 1);
        }
      }
      a.cls_out[i] = (uint8_t)cls;
      if (a.arc) a.arc[i] = arc;
      if (a.flag32) a.flag32[i] = cls == 7 ? 1 : 0;
    }
    n4 += ramp_wave_count(cls == 4);
    n5 += ramp_wave_count(cls == 5);
    n6 += ramp_wave_count(cls == 6);
    n7 += ramp_wave_count(cls == 7);
  }
  ramp_wave_flush(a.ctr + 4, tid, n4, n5, n6, n7);
}

// lanes [0, cells): last_t_out; lanes [0, N): index from the running counts of the corner flags, -1 behind them; count; the
// status words
__global__ void __launch_bounds__(INTERP_THREADS)
    crn_finish_kernel(const int32_t *__restrict__ start, const double *__restrict__ ts, uint32_t cells, const double *last_in,
                      double *last_out, const int32_t *__restrict__ flag32, const int32_t *__restrict__ incl, int N,
                      int32_t *__restrict__ index, int32_t *__restrict__ count, const int32_t *__restrict__ ctr,
                      int32_t *__restrict__ status) {
  const bool failed = (ctr[0] & RAMP_CORNER_BAD_ORDER) != 0;
  const long n_cells = last_out ? (long)cells : 0, n_events = index ? (long)N : 0, lanes = n_cells > n_events ? n_cells : n_events;
  const long tiles = (lanes + INTERP_THREADS - 1) / INTERP_THREADS;
  const int K = index ? incl[N - 1] : 0;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long q = tile * INTERP_THREADS + threadIdx.x;
    if (last_out && q < (long)cells) {
      const int s0 = start[q], s1 = start[q + 1];
      double v = last_in ? last_in[q] : ord_nan();         // (in place: a lane reads and writes its own cell alone)
      if (s1 > s0) v = ts[s1 - 1];
      last_out[q] = failed ? ord_nan() : v;
    }
    if (index && q < (long)N) {
      if (flag32[q]) index[incl[q] - 1] = (int32_t)q;      // (incl[q] - 1 < K: disjoint from the lanes that write -1)
      if (q >= (long)K) index[q] = -1;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const int w = threadIdx.x;
    status[w] = (failed && w >= 4) ? 0 : ctr[w];
  }
  if (count && blockIdx.x == 0 && threadIdx.x == 0) *count = failed ? 0 : ctr[7];
}

// the workspace: the counters; the two key and the two index arrays, ts, start, the library's own
struct CrnWs {
  int32_t *ctr;
  uint32_t *key, *skey;
  int32_t *iota, *sidx, *start;
  double *ts;
  void *cub;
  size_t cub_bytes;
};

static size_t crn_carve(void *ws, long N, long cells, CrnWs *w) {
  WsCarver c(ws);
  const size_t n = (size_t)(N > 0 ? N : 1);
  w->ctr = c.take<int32_t>(CRN_CTR_WORDS, 256);
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

static bool crn_size_ok(long N, int H, int W, int planes) {
  return N >= 0 && N <= 2147483647L && H >= 1 && W >= 1 && (planes == 1 || planes == 2) &&
         2.0 * (double)H * (double)W < 2147483647.0;
}

extern "C" {
size_t ramp_event_corners_ws_bytes(long N, int H, int W, int planes) {
  if (!crn_size_ok(N, H, W, planes)) return 0;
  CrnWs w;
  return crn_carve(nullptr, N, (long)planes * H * W, &w);
}

long ramp_event_corners_grid_events(void) { return (long)ORD_MAX_GROUPS * INTERP_THREADS; }

int ramp_event_corners(const void *x, const void *y, const double *t, const int8_t *p, long N, int H, int W, int flags,
                       int inner_lo, int inner_hi, int outer_lo, int outer_hi, const double *last_t_in, double *last_t_out,
                       uint8_t *cls, uint8_t *arc, int32_t *index, int32_t *count, int32_t *corner_count, int32_t *status,
                       void *ws, size_t ws_bytes, void *stream) {
  if (N < 0 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~(RAMP_CORNER_XY_I32 | RAMP_CORNER_WIDE)) return RAMP_EINVAL;
  if (inner_lo < 1 || inner_lo > inner_hi || inner_hi > CRN_INNER - 1 || outer_lo < 1 || outer_lo > outer_hi || outer_hi > CRN_OUTER - 1)
    return RAMP_EINVAL;
  if (!status || (N > 0 && !cls) || (index == nullptr) != (count == nullptr)) return RAMP_EINVAL;
  if ((((uintptr_t)last_t_in | (uintptr_t)last_t_out) & 7) != 0 ||
      (((uintptr_t)status | (uintptr_t)arc | (uintptr_t)index | (uintptr_t)count | (uintptr_t)corner_count) & 3) != 0)
    return RAMP_EINVAL;
  if (N > 2147483647L || 2.0 * (double)H * (double)W >= 2147483647.0) return RAMP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int planes = p ? 2 : 1;
  const long HWl = (long)H * W, cellsl = HWl * planes;
  if (N == 0) {                                            // no launch: memsets and a copy
    if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    if (count && hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    if (corner_count && hipMemsetAsync(corner_count, 0, (size_t)HWl * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    if (last_t_in && last_t_out && last_t_in != last_t_out &&
        hipMemcpyAsync(last_t_out, last_t_in, (size_t)cellsl * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return RAMP_ELAUNCH;
    return RAMP_OK;
  }
  if (!x || !y || !t || !ws) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)t & 7) != 0 || (((uintptr_t)x | (uintptr_t)y) & 3) != 0) return RAMP_EINVAL;
  CrnWs w;
  if (ws_bytes < crn_carve(ws, N, cellsl, &w)) return RAMP_EWORKSPACE;
  const uint32_t cells = (uint32_t)cellsl;
  const int n = (int)N;
  const bool i32 = (flags & RAMP_CORNER_XY_I32) != 0;
  if (hipMemsetAsync(w.ctr, 0, CRN_CTR_WORDS * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  if (corner_count && hipMemsetAsync(corner_count, 0, (size_t)HWl * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  if (i32) hipLaunchKernelGGL((crn_key_kernel<true>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, p, N, H, W, cells, w.key, w.iota, w.ctr);
  else hipLaunchKernelGGL((crn_key_kernel<false>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, p, N, H, W, cells, w.key, w.iota, w.ctr);
  RAMP_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.key, w.skey, w.iota, w.sidx, n, 0, ord_sort_bits(cells), st) != hipSuccess)
    return RAMP_ELAUNCH;
  hipLaunchKernelGGL(ord_segment_kernel, dim3(ord_grid(cellsl + 2)), dim3(INTERP_THREADS), 0, st, w.skey, n, cells, w.start);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(crn_ts_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, w.skey, w.sidx, t, n, cells, last_t_in, w.ts, w.ctr);
  RAMP_CHECK_LAUNCH();
  // the sort's inputs are dead behind it: the corner flags and their running counts take their place
  int32_t *flag32 = index ? (int32_t *)w.key : nullptr, *incl = w.iota;
  CrnArgs a;
  a.x = x; a.y = y; a.t = t; a.skey = w.skey; a.sidx = w.sidx; a.start = w.start; a.ts = w.ts; a.last_in = last_t_in;
  a.cls_out = cls; a.arc = (uint32_t *)arc; a.flag32 = flag32; a.corner_count = corner_count; a.ctr = w.ctr;
  a.N = n; a.H = H; a.W = W; a.planes = planes; a.inner_lo = inner_lo; a.inner_hi = inner_hi; a.outer_lo = outer_lo;
  a.outer_hi = outer_hi; a.wide = (flags & RAMP_CORNER_WIDE) ? 1 : 0; a.i32 = i32 ? 1 : 0;
  hipLaunchKernelGGL(crn_corner_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, a);
  RAMP_CHECK_LAUNCH();
  if (index) {
    cb = w.cub_bytes;
    if (hipcub::DeviceScan::InclusiveSum(w.cub, cb, flag32, incl, n, st) != hipSuccess) return RAMP_ELAUNCH;
  }
  const long n_cells = last_t_out ? cellsl : 1, n_events = index ? N : 1, lanes = n_cells > n_events ? n_cells : n_events;
  hipLaunchKernelGGL(crn_finish_kernel, dim3(ord_grid(lanes)), dim3(INTERP_THREADS), 0, st, w.start, w.ts, cells, last_t_in,
                     last_t_out, flag32, incl, n, index, count, w.ctr, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
