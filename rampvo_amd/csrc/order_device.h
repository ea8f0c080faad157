// What the event filter (filter.hip) and the event flow (flow.hip) share: the order stage that makes "the last event of a cell
// that precedes this one" an order-independent, bit-exact quantity.  A CELL is a pixel (the filter) or (plane, pixel) (the
// flow); the events are stably sorted by cell, so every cell's candidates form one segment in index order, and within a segment
// (t, index) rises lexicographically once the order check has passed.  One definition of the candidate test, the segment
// table and the partition-point search, so that both entries answer the same question with the same statements.
#pragma once
#include "interp_device.h"

#define ORD_MAX_GROUPS 2048              // workgroups per launch; each walks the tiles of its launch with this stride
#define ORD_FLT_MAX 3.4028234663852886e38f

static __device__ __forceinline__ double ord_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

template <bool I32>
static __device__ __forceinline__ float ord_coord(const void *__restrict__ v, long i) {
  return I32 ? (float)static_cast<const int32_t *>(v)[i] : static_cast<const float *>(v)[i];
}

// the class of an event ahead of every other test: 0 a candidate (*pixel = its pixel index), 2 not finite, 3 outside the sensor
static __device__ __forceinline__ int ord_pixel(float x, float y, double t, int H, int W, uint32_t *pixel) {
  if (!(fabsf(x) <= ORD_FLT_MAX && fabsf(y) <= ORD_FLT_MAX && interp_finite(t))) return 2;
  const float xt = truncf(x), yt = truncf(y);            // (the range test is made in float, as ramp_event_voxel makes it)
  if (xt >= 0.0f && xt <= (float)(W - 1) && yt >= 0.0f && yt <= (float)(H - 1)) {
    *pixel = (uint32_t)(int)yt * (uint32_t)W + (uint32_t)(int)xt;
    return 0;
  }
  return 3;
}

// the first entry of [p0, p1) that does not precede (ti, i): entries are ordered by (ts, sidx)
static __device__ __forceinline__ int ord_first_not_before(const double *__restrict__ ts, const int32_t *__restrict__ sidx, int p0,
                                                           int p1, double ti, int32_t i) {
  while (p0 < p1) {
    const int mid = p0 + ((p1 - p0) >> 1);
    const double tm = ts[mid];
    const bool less = tm < ti || (tm == ti && sidx[mid] < i);
    if (less) p0 = mid + 1; else p1 = mid;
  }
  return p0;
}

// the time stamp of the last candidate of `cell` that precedes (ti, i), else the cell's state, else NaN
static __device__ __forceinline__ double ord_last_before(const double *__restrict__ ts, const int32_t *__restrict__ sidx,
                                                         const int32_t *__restrict__ start, const double *__restrict__ last_in,
                                                         uint32_t cell, double ti, int32_t i) {
  const int lo = start[cell];
  const int p0 = ord_first_not_before(ts, sidx, lo, start[cell + 1], ti, i);
  return p0 > lo ? ts[p0 - 1] : (last_in ? last_in[cell] : ord_nan());
}

// start[q] = the number of sorted keys below q, for q in [0, cells + 1]: the segment of cell q is [start[q], start[q + 1])
static __global__ void __launch_bounds__(INTERP_THREADS)
    ord_segment_kernel(const uint32_t *__restrict__ skey, int N, uint32_t cells, int32_t *__restrict__ start) {
  const long tiles = ((long)cells + 2 + INTERP_THREADS - 1) / INTERP_THREADS;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long q = tile * INTERP_THREADS + threadIdx.x;
    if (q > (long)cells + 1) continue;
    int lo = 0, hi = N;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((long)skey[mid] < q) lo = mid + 1; else hi = mid;
    }
    start[q] = lo;
  }
}

static inline int ord_sort_bits(uint32_t cells) {        // ceil(log2(cells + 1)): the keys are 0 .. cells
  int bits = 0;
  while (bits < 32 && (cells >> bits) != 0) bits++;
  return bits;
}

static inline int ord_grid(long lanes, int threads = INTERP_THREADS) {
  const long tiles = (lanes + threads - 1) / threads;
  return (int)(tiles < 1 ? 1 : (tiles < ORD_MAX_GROUPS ? tiles : ORD_MAX_GROUPS));
}
