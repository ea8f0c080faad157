// Event corner tracks (include/ramp_hip.h: ramp_event_corner_tracks): every candidate event is linked to the newest candidate
// in a window around it that precedes it by at most max_dt, else to the carried state of that window, else a track is born.
// The parent relation is a forest; a track is a tree's root, and every event takes its id and birth from its root and its
// length from its depth.  Order-independent and bit-exact; the definition is in the header.  The order stage is the filter's,
// the flow's and the corners' (order_device.h), over candidates only.
//
//   trk_key_kernel        one lane per event and trip: classes [2], [3], [4]; the key is plane * H W + pixel, S H W otherwise
//   hipcub SortPairs      stable radix sort of (key, event index) over ceil(log2(S H W + 1)) bits
//   ord_segment_kernel    one lane per cell: the segment's start
//   trk_ts_kernel         per sorted position the time stamp (gathered once into ts[]) and the order check against word 0 of
//                         the state
//   trk_link_kernel       one lane per SORTED POSITION: (2 rho + 1)^2 bounded binary searches, the running best (t', d^2, j)
//                         and its source in registers; classes [5] .. [7] by ballots; per position the parent, the first jump
//                         (ancestor, links to it) and, for a root, its record (id, t0, birth pixel | length)
//   trk_jump_kernel       ceil(log2(max(N, 2))) launches, unconditionally: (ancestor, links) doubled from one buffer into the
//                         other, never in place
//   trk_resolve_kernel    per sorted position track, birth, length, velocity and parent through the event index; per cell the
//                         state (a launch of its own: in place is allowed, the state is read by the link kernel alone);
//                         next_id_out and the status words
// (trk_key_kernel and trk_ts_kernel are corner.hip's statements with the candidate mask and the state's stride, kept as a copy:
// corner.hip, flow.hip, filter.hip and order_device.h are untouched.)  No LDS, no atomics on results, no floating-point
// atomics; every loop is a binary search or has a fixed trip count.
#include "workspace_cub.h"
#include "ramp_internal.h"
#include "order_device.h"

#define TRK_CTR_WORDS 16                 // int32: the 8 status words, 8 spare
#define TRK_STATE_WORDS 4                // int64 per cell: t, id, t0, birth pixel | length << 32
#define TRK_ROOT_WORDS 3                 // int64 per root: id, t0, birth pixel | length << 32
#define TRK_LEN_MAX 2147483647

static __device__ __forceinline__ int32_t trk_len_add(int32_t len, int32_t links) {      // saturating, links >= 0
  const long s = (long)len + (long)links;
  return s > (long)TRK_LEN_MAX ? TRK_LEN_MAX : (int32_t)s;
}

// the class of an event ahead of the linking: ord_pixel's, then [4] for a valid event that is not a candidate
template <bool I32>
static __device__ __forceinline__ int trk_class(const void *__restrict__ xv, const void *__restrict__ yv, const double *__restrict__ t,
                                                const uint8_t *__restrict__ corner, long i, int H, int W, uint32_t *pixel) {
  const int c = ord_pixel(ord_coord<I32>(xv, i), ord_coord<I32>(yv, i), t[i], H, W, pixel);
  return (c == 0 && corner && corner[i] == 0) ? 4 : c;
}

template <bool I32>
__global__ void __launch_bounds__(INTERP_THREADS)
    trk_key_kernel(const void *__restrict__ xv, const void *__restrict__ yv, const double *__restrict__ t,
                   const int8_t *__restrict__ p, const uint8_t *__restrict__ corner, long N, int H, int W, uint32_t cells,
                   uint32_t *__restrict__ key, int32_t *__restrict__ iota, int32_t *__restrict__ ctr) {
  const int tid = threadIdx.x;
  const uint32_t HW = (uint32_t)H * (uint32_t)W;
  const long tiles = (N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n_seen = 0, n_bad = 0, n_out = 0, n_not = 0;       // wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * INTERP_THREADS + tid;
    const bool have = i < N;
    int c = 0;
    if (have) {
      uint32_t k = 0;
      c = trk_class<I32>(xv, yv, t, corner, i, H, W, &k);
      if (c != 0) k = cells;
      else if (p && p[i] > 0) k += HW;
      key[i] = k;
      iota[i] = (int32_t)i;
    }
    n_seen += ramp_wave_count(have);
    n_bad += ramp_wave_count(c == 2);
    n_out += ramp_wave_count(c == 3);
    n_not += ramp_wave_count(c == 4);
  }
  ramp_wave_flush(ctr + 1, tid, n_seen, n_bad, n_out, n_not);
}

// ts[] and the order check: the neighbour in the segment, the segment's first entry against the state's t
__global__ void __launch_bounds__(INTERP_THREADS)
    trk_ts_kernel(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sidx, const double *__restrict__ t, int N,
                  uint32_t cells, const int64_t *__restrict__ state_in, double *__restrict__ ts, int32_t *__restrict__ ctr) {
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
      else if (state_in) before = __longlong_as_double(state_in[(size_t)k * TRK_STATE_WORDS]);
      bad = bad || ti < before;
    }
  }
  if (__ballot(bad) != 0 && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(&ctr[0], RAMP_CORNER_TRACK_BAD_ORDER);
}

struct TrkArgs {
  const void *x, *y;
  const double *t;
  const uint8_t *corner;
  const uint32_t *skey;
  const int32_t *sidx, *start;
  const double *ts;
  const int64_t *state_in, *next_id_in;
  uint8_t *cls_out;
  int32_t *par;                                            // per position: the parent's position, -1 a birth, -2 - cell a state entry
  int64_t *root;                                           // per position [TRK_ROOT_WORDS], written for roots alone
  int2 *jump;                                              // per position (ancestor, links to it)
  int32_t *ctr;
  double max_dt;
  int N, H, W, planes, rho, i32;
};

__global__ void __launch_bounds__(INTERP_THREADS) trk_link_kernel(const TrkArgs a) {
  const int tid = threadIdx.x;
  const int N = a.N, H = a.H, W = a.W, rho = a.rho;
  const uint32_t HW = (uint32_t)H * (uint32_t)W, cells = HW * (uint32_t)a.planes;
  const bool failed = (a.ctr[0] & RAMP_CORNER_TRACK_BAD_ORDER) != 0;
  const int64_t next_id = a.next_id_in ? *a.next_id_in : 0;
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  int n5 = 0, n6 = 0, n7 = 0;                              // classes [5] .. [7], wave-uniform: sums of ballots
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + tid;
    int cls = 0;
    if (pos < (long)N) {
      const uint32_t k = a.skey[pos];
      const int32_t i = a.sidx[pos];
      int32_t par = -1;
      int2 jump = make_int2((int)pos, 0);
      if (failed) {
        cls = 0;
      } else if (k >= cells) {                             // counted by the key kernel: the class is found again for cls_out
        uint32_t unused;
        cls = a.i32 ? trk_class<true>(a.x, a.y, a.t, a.corner, i, H, W, &unused) : trk_class<false>(a.x, a.y, a.t, a.corner, i, H, W, &unused);
      } else {
        const uint32_t plane0 = k >= HW ? HW : 0u, pix = k - plane0;
        const int qy = (int)(pix / (uint32_t)W), qx = (int)(pix - (uint32_t)qy * (uint32_t)W);
        const double ti = a.ts[pos];
        bool any = false;
        double best_t = 0.0;
        int best_d2 = 0;
        int32_t best_src = -1;
        for (int dy = -rho; dy <= rho; dy++) {             // ascending j: a later cell wins only when it is strictly better
          const int ny = qy + dy;
          if (ny < 0 || ny >= H) continue;
          for (int dx = -rho; dx <= rho; dx++) {
            const int nx = qx + dx;
            if (nx < 0 || nx >= W) continue;
            const uint32_t cell = plane0 + (uint32_t)ny * (uint32_t)W + (uint32_t)nx;
            const int lo = a.start[cell];
            const int p0 = ord_first_not_before(a.ts, a.sidx, lo, a.start[cell + 1], ti, i);
            double tp;
            int32_t src;
            if (p0 > lo) { tp = a.ts[p0 - 1]; src = p0 - 1; }
            else { tp = a.state_in ? __longlong_as_double(a.state_in[(size_t)cell * TRK_STATE_WORDS]) : ord_nan(); src = -2 - (int32_t)cell; }
            const double gap = ti - tp;
            const int d2 = dx * dx + dy * dy;
            const bool eligible = tp == tp && gap <= a.max_dt;
            if (eligible && (!any || tp > best_t || (tp == best_t && d2 < best_d2))) { any = true; best_t = tp; best_d2 = d2; best_src = src; }
          }
        }
        int64_t *root = a.root + (size_t)pos * TRK_ROOT_WORDS;
        if (!any) {
          cls = 5;
          root[0] = next_id + (int64_t)i;
          root[1] = __double_as_longlong(ti);
          root[2] = (int64_t)(((uint64_t)1 << 32) | (uint64_t)pix);
        } else if (best_src < 0) {
          cls = 6;
          par = best_src;
          const int64_t *s = a.state_in + (size_t)(uint32_t)(-2 - best_src) * TRK_STATE_WORDS;
          const uint64_t w3 = (uint64_t)s[3];
          const int32_t len = trk_len_add((int32_t)(w3 >> 32), 1);
          root[0] = s[1];
          root[1] = s[2];
          root[2] = (int64_t)(((uint64_t)(uint32_t)len << 32) | (w3 & 0xffffffffull));
        } else {
          cls = 7;
          par = best_src;
          jump = make_int2(best_src, 1);
        }
      }
      a.cls_out[i] = (uint8_t)cls;
      a.par[pos] = par;
      a.jump[pos] = jump;
    }
    n5 += ramp_wave_count(cls == 5);
    n6 += ramp_wave_count(cls == 6);
    n7 += ramp_wave_count(cls == 7);
  }
  ramp_wave_flush(a.ctr + 5, tid, n5, n6, n7);
}

// one round of pointer jumping, from `in` into `out`: the ancestor's ancestor, the links to it summed.  A root is its own
// ancestor at 0 links, so a lane that has arrived stays.
__global__ void __launch_bounds__(INTERP_THREADS) trk_jump_kernel(const int2 *__restrict__ in, int2 *__restrict__ out, int N) {
  const long tiles = ((long)N + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long pos = tile * INTERP_THREADS + threadIdx.x;
    if (pos >= (long)N) continue;
    const int2 mine = in[pos], up = in[mine.x];
    out[pos] = make_int2(up.x, mine.y + up.y);
  }
}

struct TrkRecord {
  int64_t id, t0_bits;
  uint32_t pix;
  int32_t length;
};

// the record of the candidate at sorted position `pos`: id, birth and length from its root, the depth added
static __device__ __forceinline__ TrkRecord trk_record(const int2 *__restrict__ jump, const int64_t *__restrict__ root, long pos) {
  const int2 j = jump[pos];
  const int64_t *r = root + (size_t)j.x * TRK_ROOT_WORDS;
  const uint64_t w = (uint64_t)r[2];
  TrkRecord rec;
  rec.id = r[0];
  rec.t0_bits = r[1];
  rec.pix = (uint32_t)w;
  rec.length = trk_len_add((int32_t)(w >> 32), j.y);
  return rec;
}

struct TrkOut {
  const uint32_t *skey;
  const int32_t *sidx, *start, *par;
  const double *ts;
  const int2 *jump;
  const int64_t *root, *state_in, *next_id_in;
  int64_t *state_out, *next_id_out, *track;
  int32_t *parent, *length, *status;
  double *birth;
  float *velocity;
  const int32_t *ctr;
  int N, H, W, planes;
};

__global__ void __launch_bounds__(INTERP_THREADS) trk_resolve_kernel(const TrkOut a) {
  const int N = a.N, W = a.W;
  const uint32_t HW = (uint32_t)a.H * (uint32_t)W, cells = HW * (uint32_t)a.planes;
  const bool failed = (a.ctr[0] & RAMP_CORNER_TRACK_BAD_ORDER) != 0;
  const long lanes = (long)cells > (long)N ? (long)cells : (long)N;
  const long tiles = (lanes + INTERP_THREADS - 1) / INTERP_THREADS;
  const double nan = ord_nan();
  const float nanf = __int_as_float(0x7fc00000);
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long q = tile * INTERP_THREADS + threadIdx.x;
    if (q < (long)cells) {                                 // (in place: a lane reads and writes its own cell alone)
      int64_t w[TRK_STATE_WORDS] = {__double_as_longlong(nan), 0, 0, 0};
      const int s0 = a.start[q], s1 = a.start[q + 1];
      if (failed) {                                        // emptied: t = NaN, the rest 0
      } else if (s1 > s0) {
        const TrkRecord rec = trk_record(a.jump, a.root, s1 - 1);
        w[0] = __double_as_longlong(a.ts[s1 - 1]);
        w[1] = rec.id;
        w[2] = rec.t0_bits;
        w[3] = (int64_t)(((uint64_t)(uint32_t)rec.length << 32) | (uint64_t)rec.pix);
      } else if (a.state_in) {
#pragma unroll
        for (int c = 0; c < TRK_STATE_WORDS; c++) w[c] = a.state_in[(size_t)q * TRK_STATE_WORDS + c];
      }
#pragma unroll
      for (int c = 0; c < TRK_STATE_WORDS; c++) a.state_out[(size_t)q * TRK_STATE_WORDS + c] = w[c];
    }
    if (q < (long)N) {
      const uint32_t k = a.skey[q];
      const size_t i = (size_t)a.sidx[q];
      int32_t parent = -1, length = 0;
      int64_t track = -1;
      double b0 = nan, b1 = nan, b2 = nan;
      float vx = nanf, vy = nanf;
      if (!failed && k < cells) {
        const TrkRecord rec = trk_record(a.jump, a.root, q);
        const uint32_t pix = k >= HW ? k - HW : k;
        const long qy = (long)(pix / (uint32_t)W), qx = (long)(pix - (uint32_t)qy * (uint32_t)W);
        const long y0 = (long)(rec.pix / (uint32_t)W), x0 = (long)(rec.pix - (uint32_t)y0 * (uint32_t)W);
        const double ti = a.ts[q], t0 = __longlong_as_double(rec.t0_bits);
        const int32_t par = a.par[q];
        parent = par >= 0 ? a.sidx[par] : (par == -1 ? -1 : -2);
        track = rec.id;
        length = rec.length;
        b0 = t0; b1 = (double)x0; b2 = (double)y0;
        if (!(ti == t0)) {                                 // (a NaN t0 gives NaN through the division)
          const double dt = ti - t0;
          vx = (float)((double)(qx - x0) / dt);
          vy = (float)((double)(qy - y0) / dt);
        }
      }
      if (a.parent) a.parent[i] = parent;
      if (a.track) a.track[i] = track;
      if (a.length) a.length[i] = length;
      if (a.birth) { a.birth[3 * i] = b0; a.birth[3 * i + 1] = b1; a.birth[3 * i + 2] = b2; }
      if (a.velocity) { a.velocity[2 * i] = vx; a.velocity[2 * i + 1] = vy; }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const int w = threadIdx.x;
    a.status[w] = (failed && w >= 4) ? 0 : a.ctr[w];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.next_id_out = (a.next_id_in ? *a.next_id_in : 0) + (int64_t)N;
}

// the workspace: the counters; the two key and the two index arrays, ts, start, the parents, the roots' records, the two jump
// buffers, the library's own
struct TrkWs {
  int32_t *ctr;
  uint32_t *key, *skey;
  int32_t *iota, *sidx, *start, *par;
  double *ts;
  int64_t *root;
  int2 *jump_a, *jump_b;
  void *cub;
  size_t cub_bytes;
};

static size_t trk_carve(void *ws, long N, long cells, TrkWs *w) {
  WsCarver c(ws);
  const size_t n = (size_t)(N > 0 ? N : 1);
  w->ctr = c.take<int32_t>(TRK_CTR_WORDS, 256);
  w->key = c.take<uint32_t>(n, 256);
  w->skey = c.take<uint32_t>(n, 256);
  w->iota = c.take<int32_t>(n, 256);
  w->sidx = c.take<int32_t>(n, 256);
  w->ts = c.take<double>(n, 256);
  w->start = c.take<int32_t>((size_t)cells + 2, 256);
  w->par = c.take<int32_t>(n, 256);
  w->root = c.take<int64_t>(n * TRK_ROOT_WORDS, 256);
  w->jump_a = c.take<int2>(n, 256);
  w->jump_b = c.take<int2>(n, 256);
  w->cub_bytes = ws_cub_bytes<uint32_t>((int)n, 32);
  w->cub = c.take<char>(w->cub_bytes, 256);
  return c.bytes();
}

static bool trk_size_ok(long N, int H, int W, int planes) {
  return N >= 0 && N <= 2147483647L && H >= 1 && W >= 1 && (planes == 1 || planes == 2) &&
         2.0 * (double)H * (double)W < 2147483647.0;
}

static int trk_rounds(long N) {                            // ceil(log2(max(N, 2))): a chain of N events has N - 1 links
  int r = 1;
  while (((long)1 << r) < N) r++;
  return r;
}

extern "C" {
size_t ramp_event_corner_tracks_ws_bytes(long N, int H, int W, int planes) {
  if (!trk_size_ok(N, H, W, planes)) return 0;
  TrkWs w;
  return trk_carve(nullptr, N, (long)planes * H * W, &w);
}

long ramp_event_corner_tracks_grid_events(void) { return (long)ORD_MAX_GROUPS * INTERP_THREADS; }

int ramp_event_corner_tracks(const void *x, const void *y, const double *t, const int8_t *p, const uint8_t *corner, long N, int H,
                             int W, int flags, int rho, double max_dt, const int64_t *state_in, const int64_t *next_id_in,
                             int64_t *state_out, int64_t *next_id_out, uint8_t *cls, int32_t *parent, int64_t *track,
                             int32_t *length, double *birth, float *velocity, int32_t *status, void *ws, size_t ws_bytes,
                             void *stream) {
  if (N < 0 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~RAMP_CORNER_TRACK_XY_I32) return RAMP_EINVAL;
  if (rho < 0 || rho > 5 || !(max_dt >= 0.0)) return RAMP_EINVAL;
  if (!status || (N > 0 && (!cls || !state_out || !next_id_out)) || (state_in == nullptr) != (next_id_in == nullptr)) return RAMP_EINVAL;
  if ((((uintptr_t)state_in | (uintptr_t)state_out | (uintptr_t)next_id_in | (uintptr_t)next_id_out | (uintptr_t)track |
        (uintptr_t)birth) & 7) != 0 ||
      (((uintptr_t)status | (uintptr_t)parent | (uintptr_t)length | (uintptr_t)velocity) & 3) != 0)
    return RAMP_EINVAL;
  if (N > 2147483647L || 2.0 * (double)H * (double)W >= 2147483647.0) return RAMP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int planes = p ? 2 : 1;
  const long HWl = (long)H * W, cellsl = HWl * planes;
  if (N == 0) {                                            // no launch: a memset and two copies
    if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
    if (state_in && state_out && state_in != state_out &&
        hipMemcpyAsync(state_out, state_in, (size_t)cellsl * TRK_STATE_WORDS * sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return RAMP_ELAUNCH;
    if (next_id_in && next_id_out && next_id_in != next_id_out &&
        hipMemcpyAsync(next_id_out, next_id_in, sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return RAMP_ELAUNCH;
    return RAMP_OK;
  }
  if (!x || !y || !t || !ws) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)t & 7) != 0 || (((uintptr_t)x | (uintptr_t)y) & 3) != 0) return RAMP_EINVAL;
  TrkWs w;
  if (ws_bytes < trk_carve(ws, N, cellsl, &w)) return RAMP_EWORKSPACE;
  const uint32_t cells = (uint32_t)cellsl;
  const int n = (int)N;
  const bool i32 = (flags & RAMP_CORNER_TRACK_XY_I32) != 0;
  if (hipMemsetAsync(w.ctr, 0, TRK_CTR_WORDS * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  if (i32) hipLaunchKernelGGL((trk_key_kernel<true>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, p, corner, N, H, W, cells, w.key, w.iota, w.ctr);
  else hipLaunchKernelGGL((trk_key_kernel<false>), dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, x, y, t, p, corner, N, H, W, cells, w.key, w.iota, w.ctr);
  RAMP_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.key, w.skey, w.iota, w.sidx, n, 0, ord_sort_bits(cells), st) != hipSuccess)
    return RAMP_ELAUNCH;
  hipLaunchKernelGGL(ord_segment_kernel, dim3(ord_grid(cellsl + 2)), dim3(INTERP_THREADS), 0, st, w.skey, n, cells, w.start);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(trk_ts_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, w.skey, w.sidx, t, n, cells, state_in, w.ts, w.ctr);
  RAMP_CHECK_LAUNCH();
  TrkArgs a;
  a.x = x; a.y = y; a.t = t; a.corner = corner; a.skey = w.skey; a.sidx = w.sidx; a.start = w.start; a.ts = w.ts;
  a.state_in = state_in; a.next_id_in = next_id_in; a.cls_out = cls; a.par = w.par; a.root = w.root; a.jump = w.jump_a;
  a.ctr = w.ctr; a.max_dt = max_dt; a.N = n; a.H = H; a.W = W; a.planes = planes; a.rho = rho; a.i32 = i32 ? 1 : 0;
  hipLaunchKernelGGL(trk_link_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, a);
  RAMP_CHECK_LAUNCH();
  int2 *from = w.jump_a, *to = w.jump_b;
  for (int r = 0, rounds = trk_rounds(N); r < rounds; r++) {
    hipLaunchKernelGGL(trk_jump_kernel, dim3(ord_grid(N)), dim3(INTERP_THREADS), 0, st, from, to, n);
    RAMP_CHECK_LAUNCH();
    int2 *swap = from; from = to; to = swap;
  }
  TrkOut o;
  o.skey = w.skey; o.sidx = w.sidx; o.start = w.start; o.par = w.par; o.ts = w.ts; o.jump = from; o.root = w.root;
  o.state_in = state_in; o.next_id_in = next_id_in; o.state_out = state_out; o.next_id_out = next_id_out; o.track = track;
  o.parent = parent; o.length = length; o.status = status; o.birth = birth; o.velocity = velocity; o.ctr = w.ctr;
  o.N = n; o.H = H; o.W = W; o.planes = planes;
  hipLaunchKernelGGL(trk_resolve_kernel, dim3(ord_grid(cellsl > N ? cellsl : N)), dim3(INTERP_THREADS), 0, st, o);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
