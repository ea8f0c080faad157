// The time surface of an event list (include/ramp_hip.h: ramp_time_surface): per pixel the newest time stamp at or before
// t_ref, decayed with exp((last - t_ref) / tau) and smoothed -- negated, the distance-like field the event map's localiser
// (maplocalize.hip) samples.  One hipMemsetAsync (the status words) and 3 + 2 * smooth launches:
//   ts_seed_kernel     per pixel: the word of last_t_in (0: no event)
//   ts_event_kernel    per event, grid-stride: the counters (one ballot per counter and wave); per used event one return-less
//                      64-bit atomicMax of the time stamp's order-preserving word, behind a relaxed load of the word: a lane
//                      that cannot raise it issues nothing (the words only grow, so a stale load costs an atomic, never a result)
//   ts_surface_kernel  per pixel, one writer: the word back as a double, raw, the optional outputs
//   ts_blur_kernel     rows, then columns, per pass: a tile and its halo through LDS, edges replicated
// The integer max does not depend on the order of its operands: the surface depends neither on the events' order nor on the
// launch's schedule, and a call repeats its bits.  No lane waits for another one.
#include "ramp_internal.h"
#include "ramp_device.h"

#define TS_THREADS 256
#define TS_MAX_GROUPS 1024
#define TS_TX 32                           // the blur's tile: 32 x 8 outputs, two more on either side along the pass
#define TS_TY 8
#define TS_MAX_SMOOTH 8
typedef unsigned long long ts_u64;

struct TsWs {
  ts_u64 *word;                            // [H * W] the largest time stamp's word
  float *tmp;                              // [H * W] the other side of the blur's ping-pong
};
static size_t ts_carve(void *ws, size_t HW, TsWs *w) {
  WsCarver c(ws);
  w->word = c.take<ts_u64>(HW, 256);
  w->tmp = c.take<float>(HW, 256);
  return c.bytes();
}

// median.h's map of a float to an unsigned word whose order is the floats', widened; no finite double maps to 0
static __device__ __forceinline__ ts_u64 ts_word(double t) {
  const ts_u64 b = (ts_u64)__double_as_longlong(t);
  return b ^ ((b >> 63) ? ~(ts_u64)0 : ((ts_u64)1 << 63));
}
static __device__ __forceinline__ double ts_time(ts_u64 w) {
  return __longlong_as_double((long long)(w ^ ((w >> 63) ? ((ts_u64)1 << 63) : ~(ts_u64)0)));
}
static __device__ __forceinline__ bool ts_finite(double t) { return fabs(t) <= 1.7976931348623157e308; }

__global__ void __launch_bounds__(TS_THREADS) ts_seed_kernel(const double *__restrict__ last_in, double t_ref, ts_u64 *__restrict__ word, long HW) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  ts_u64 w = 0;
  if (last_in) {
    const double t = last_in[i];
    if (ts_finite(t) && t <= t_ref) w = ts_word(t);
  }
  word[i] = w;
}

__global__ void __launch_bounds__(TS_THREADS)
    ts_event_kernel(const float *__restrict__ x, const float *__restrict__ y, const double *__restrict__ t, long N, double t_ref, int H,
                    int W, ts_u64 *word, int32_t *status) {
  const int tid = threadIdx.x;
  int n_seen = 0, n_bad = 0, n_out = 0, n_late = 0, n_used = 0;
  for (long base = (long)blockIdx.x * TS_THREADS; base < N; base += (long)gridDim.x * TS_THREADS) {
    const long i = base + tid;
    const bool have = i < N;
    bool bad = false, outside = false, late = false, used = false;
    if (have) {
      const float xe = x[i], ye = y[i];
      const double te = t[i];
      const float px = rintf(xe), py = rintf(ye);     // the pixel, as the warp samples a map
      if (!(fabsf(xe) <= 3.4028234663852886e38f) || !(fabsf(ye) <= 3.4028234663852886e38f) || !ts_finite(te)) bad = true;
      else if (!((double)px >= 0.0 && (double)px <= (double)(W - 1) && (double)py >= 0.0 && (double)py <= (double)(H - 1)))
        outside = true;                                // (in floating point, before any conversion to an integer)
      else if (!(te <= t_ref)) late = true;
      else {
        used = true;
        ts_u64 *at = word + ((size_t)(long)py * W + (long)px);
        const ts_u64 mine = ts_word(te);
        if (__atomic_load_n(at, __ATOMIC_RELAXED) < mine) atomicMax(at, mine);
      }
    }
    // the trip count and `have` aside, every lane of the wave is here
    n_seen += ramp_wave_count(have);
    n_bad += ramp_wave_count(bad);
    n_out += ramp_wave_count(outside);
    n_late += ramp_wave_count(late);
    n_used += ramp_wave_count(used);
  }
  ramp_wave_flush(status + 1, tid, n_seen, n_bad, n_out, n_late, n_used);
}

__global__ void __launch_bounds__(TS_THREADS)
    ts_surface_kernel(const ts_u64 *__restrict__ word, double t_ref, double tau, int negate, long HW, float *__restrict__ surface,
                      float *__restrict__ raw_out, double *__restrict__ last_out, int32_t *status) {
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * blockDim.x + tid;
  const bool failed = !ts_finite(t_ref) || !ts_finite(tau) || !(tau > 0.0);
  if (blockIdx.x == 0 && tid == 0 && failed) status[0] = RAMP_TIME_SURFACE_BAD_ARGS;
  bool stamped = false;
  if (i < HW) {
    const ts_u64 w = word[i];
    stamped = w != 0;
    const double last = stamped ? ts_time(w) : __longlong_as_double(0x7ff8000000000000ll);
    float raw = 0.0f;
    if (stamped) raw = expf((float)((last - t_ref) / tau));
    if (negate) raw = 1.0f - raw;
    if (failed) raw = __int_as_float(0x7fc00000);
    surface[i] = raw;
    if (raw_out) raw_out[i] = raw;
    if (last_out) last_out[i] = last;
  }
  // every lane of the wave is here
  const int n_stamped = ramp_wave_count(stamped);
  ramp_wave_flush(status + 6, tid, n_stamped);
}

// one half of a pass of the 5-tap binomial (1, 4, 6, 4, 1) / 16: along x (ROWS) or along y; fp32 without FMA, the five products
// summed left to right, the sum times 0.0625f; a coordinate outside the image reads the nearest pixel inside
template <bool ROWS>
__global__ void __launch_bounds__(TS_TX * TS_TY) ts_blur_kernel(const float *__restrict__ src, float *__restrict__ dst, int H, int W, long tiles_x) {
  constexpr int LX = TS_TX + (ROWS ? 4 : 0), LY = TS_TY + (ROWS ? 0 : 4);
  __shared__ float tile[LY][LX];
  const long tile_y = (long)blockIdx.x / tiles_x, tile_x = (long)blockIdx.x - tile_y * tiles_x;
  const long x0 = tile_x * TS_TX - (ROWS ? 2 : 0), y0 = tile_y * TS_TY - (ROWS ? 0 : 2);
  for (int k = threadIdx.x; k < LX * LY; k += TS_TX * TS_TY) {
    const int ly = k / LX, lx = k - ly * LX;
    const long gx = min(max(x0 + lx, 0l), (long)W - 1), gy = min(max(y0 + ly, 0l), (long)H - 1);
    tile[ly][lx] = src[(size_t)gy * W + gx];
  }
  __syncthreads();
  const int lx = threadIdx.x % TS_TX, ly = threadIdx.x / TS_TX;
  const long gx = tile_x * TS_TX + lx, gy = tile_y * TS_TY + ly;
  if (gx >= W || gy >= H) return;
  float a, b, c, d, e;
  if (ROWS) { a = tile[ly][lx]; b = tile[ly][lx + 1]; c = tile[ly][lx + 2]; d = tile[ly][lx + 3]; e = tile[ly][lx + 4]; }
  else { a = tile[ly][lx]; b = tile[ly + 1][lx]; c = tile[ly + 2][lx]; d = tile[ly + 3][lx]; e = tile[ly + 4][lx]; }
  dst[(size_t)gy * W + gx] = ((((1.0f * a + 4.0f * b) + 6.0f * c) + 4.0f * d) + 1.0f * e) * 0.0625f;
}

extern "C" {
size_t ramp_time_surface_ws_bytes(int H, int W) {
  if (H < 1 || W < 1 || (double)H * (double)W >= 2147483648.0) return 0;
  TsWs w;
  return ts_carve(nullptr, (size_t)H * W, &w);
}

int ramp_time_surface(const float *x, const float *y, const double *t, long N, const double *last_t_in, double t_ref, double tau,
                      int H, int W, int smooth, int flags, float *surface, float *raw, double *last_t_out, void *ws,
                      size_t ws_bytes, int32_t *status, void *stream) {
  if (N < 0 || H < 1 || W < 1 || smooth < 0 || smooth > TS_MAX_SMOOTH || (flags & ~RAMP_TIME_SURFACE_NEGATE)) return RAMP_EINVAL;
  if (!surface || !status || !ws || (N > 0 && (!x || !y || !t))) return RAMP_EINVAL;
  if (((uintptr_t)ws & 255) != 0 || (((uintptr_t)t | (uintptr_t)last_t_in | (uintptr_t)last_t_out) & 7) != 0 ||
      (((uintptr_t)x | (uintptr_t)y | (uintptr_t)surface | (uintptr_t)raw | (uintptr_t)status) & 3) != 0)
    return RAMP_EINVAL;
  if ((double)H * (double)W >= 2147483648.0) return RAMP_EUNSUPPORTED;
  const size_t HW = (size_t)H * W;
  TsWs w;
  if (ws_bytes < ts_carve(ws, HW, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const dim3 per_pixel((unsigned)((HW + TS_THREADS - 1) / TS_THREADS));
  hipLaunchKernelGGL(ts_seed_kernel, per_pixel, dim3(TS_THREADS), 0, st, last_t_in, t_ref, w.word, (long)HW);
  RAMP_CHECK_LAUNCH();
  if (N > 0) {
    const long groups = (N + TS_THREADS - 1) / TS_THREADS;
    hipLaunchKernelGGL(ts_event_kernel, dim3((unsigned)(groups < TS_MAX_GROUPS ? groups : TS_MAX_GROUPS)), dim3(TS_THREADS), 0, st, x, y,
                       t, N, t_ref, H, W, w.word, status);
    RAMP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ts_surface_kernel, per_pixel, dim3(TS_THREADS), 0, st, w.word, t_ref, tau, (flags & RAMP_TIME_SURFACE_NEGATE) ? 1 : 0,
                     (long)HW, surface, raw, last_t_out, status);
  RAMP_CHECK_LAUNCH();
  const long tiles_x = ((long)W + TS_TX - 1) / TS_TX, tiles_y = ((long)H + TS_TY - 1) / TS_TY;
  for (int pass = 0; pass < smooth; pass++) {
    hipLaunchKernelGGL((ts_blur_kernel<true>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TS_TX * TS_TY), 0, st, surface, w.tmp, H, W, tiles_x);
    RAMP_CHECK_LAUNCH();
    hipLaunchKernelGGL((ts_blur_kernel<false>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TS_TX * TS_TY), 0, st, w.tmp, surface, H, W, tiles_x);
    RAMP_CHECK_LAUNCH();
  }
  return RAMP_OK;
}
}  // extern "C"
