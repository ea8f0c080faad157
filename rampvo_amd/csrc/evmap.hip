// Event map (include/ramp_hip.h: ramp_depth_points, ramp_point_map_*): what EMVS (Rebecq et al., IJCV 2018) does behind the
// detection of ramp_event_dsi -- the detected inverse depths of one reference view are median-filtered over the detected
// pixels of a window, isolated detections are dropped, the rest is lifted to world points, and the clouds of successive
// reference views are merged in a voxel hash table.
//
// ramp_depth_points: one memset (the status words), two launches around one hipcub scan
//   evm_filter_kernel    per EVM_TW x EVM_TH pixels: the keys (median.h's order-preserving map of a float's bits) and the
//                        detection flags of the tile and its halo in LDS; per detected pixel the count n of detected pixels in
//                        its window, the element of rank (n - 1) / 2 by counting (no array in registers: no scratch), the
//                        lift, the counters (one ballot per counter and wave)
//   hipcub InclusiveSum  over the kept flags: the positions, ascending in the pixel index -- no atomics for them
//   evm_compact_kernel   per kept pixel: the lift again (the same statements, the same bits) into its row
//
// The voxel hash: one 64-byte slot per voxel -- key, n, sq[3], sc, views, one spare word -- behind a 64-byte header (the
// occupied count).  A point's slot is the splitmix64 finaliser of its key, masked, then linear probing: a relaxed load, a
// 64-bit atomicCAS on the key word where the load saw the empty marker, at most `capacity` probes.  No lane waits for
// another one: a probe either claims, matches or moves on.  All sums are 64-bit integers (atomicAdd, atomicOr): the table's
// sums do not depend on the points' order.  The export sorts (key, slot) pairs with hipcub's radix sort: slots that do not
// pass get the key ~0, which no voxel has (bit 63 of a voxel's key is clear), and sort behind the rest.
#include <hipcub/hipcub.hpp>

#include "evmap_device.h"

#define EVM_TW 32
#define EVM_TH 8
#define EVM_RMAX 3                         // the largest median_radius: the halo of a tile in LDS
static_assert(EVM_TW * EVM_TH == EVM_THREADS, "one pixel per lane");

// median.h's order-preserving map of a float's bits to an unsigned word, and back
static __device__ __forceinline__ unsigned evm_key(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
static __device__ __forceinline__ float evm_unkey(unsigned b) {
  return __uint_as_float(b ^ ((b >> 31) ? 0x80000000u : 0xffffffffu));
}

// the lift of pixel (u, v) with inverse depth d; false: rejected by its depth or a world point that is not finite
static __device__ __forceinline__ bool evm_lift(const float *c, int u, int v, float d, float min_invdepth, float *Xw) {
  if (!evm_finite(d) || !(d > 0.0f) || d < min_invdepth) return false;
  const float z = 1.0f / d;
  const float Xc[3] = {(((float)u - c[9]) / c[7]) * z, (((float)v - c[10]) / c[8]) * z, z};
  float r[3];
  lt_qrot(c + 3, Xc, r);
  Xw[0] = r[0] + c[0];
  Xw[1] = r[1] + c[1];
  Xw[2] = r[2] + c[2];
  return evm_finite(Xw[0]) && evm_finite(Xw[1]) && evm_finite(Xw[2]);
}

__global__ void __launch_bounds__(EVM_THREADS)
    evm_filter_kernel(const float *__restrict__ invdepth, const int32_t *__restrict__ plane, const float *__restrict__ cam,
                      const float *__restrict__ intrinsics, int H, int W, int r, int min_support, float min_invdepth,
                      float *__restrict__ filt, int32_t *__restrict__ keep, float *__restrict__ filtered_out,
                      int32_t *__restrict__ status) {
  __shared__ unsigned s_key[EVM_TH + 2 * EVM_RMAX][EVM_TW + 2 * EVM_RMAX];
  __shared__ unsigned char s_det[EVM_TH + 2 * EVM_RMAX][EVM_TW + 2 * EVM_RMAX];
  const int tid = threadIdx.x;
  const int tiles_x = (W + EVM_TW - 1) / EVM_TW;
  const int x0 = (int)(blockIdx.x % tiles_x) * EVM_TW, y0 = (int)(blockIdx.x / tiles_x) * EVM_TH;
  float c[11];
  const bool failed = evm_load_camera(cam, intrinsics, c);
  if (blockIdx.x == 0 && tid == 0) status[0] = failed ? RAMP_DEPTH_POINTS_BAD_CAMERA : 0;
  const int rows = EVM_TH + 2 * r, cols = EVM_TW + 2 * r;
  for (int i = tid; i < rows * cols; i += EVM_THREADS) {
    const int ly = i / cols, lx = i % cols, gy = y0 - r + ly, gx = x0 - r + lx;
    unsigned key = 0;
    bool det = false;
    if (!failed && gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t at = (size_t)gy * W + gx;
      const float d = invdepth[at];
      det = plane ? plane[at] >= 0 : (evm_finite(d) && d > 0.0f);
      key = evm_key(d);
    }
    s_key[ly][lx] = key;
    s_det[ly][lx] = det ? 1 : 0;
  }
  __syncthreads();
  const int lx = tid % EVM_TW, ly = tid / EVM_TW, px = x0 + lx, py = y0 + ly;
  const bool inside = px < W && py < H;
  bool det = false, isolated = false, lifted = false;
  float d = __int_as_float(0x7fc00000);
  if (inside && s_det[ly + r][lx + r]) {
    det = true;
    const int side = 2 * r + 1;
    int n = 0;
    for (int j = 0; j < side * side; j++) n += s_det[ly + j / side][lx + j % side];
    if (n < min_support) {
      isolated = true;
    } else {
      // the element of rank m in ascending order: the key with `less` <= m < `less or equal`
      const int m = (n - 1) / 2;
      unsigned found = s_key[ly + r][lx + r];
      bool have = false;
      for (int j = 0; j < side * side && !have; j++) {
        const int jy = ly + j / side, jx = lx + j % side;
        if (!s_det[jy][jx]) continue;
        const unsigned kj = s_key[jy][jx];
        int less = 0, le = 0;
        for (int i = 0; i < side * side; i++) {
          const int iy = ly + i / side, ix = lx + i % side;
          if (s_det[iy][ix]) {
            const unsigned ki = s_key[iy][ix];
            less += ki < kj;
            le += ki <= kj;
          }
        }
        if (less <= m && m < le) { found = kj; have = true; }
      }
      const float dm = evm_unkey(found);
      float Xw[3];
      lifted = evm_lift(c, px, py, dm, min_invdepth, Xw);
      if (lifted) d = dm;
    }
  }
  if (inside) {
    const size_t at = (size_t)py * W + px;
    filt[at] = d;
    keep[at] = lifted ? 1 : 0;
    if (filtered_out) filtered_out[at] = d;
  }
  // every lane of the wave is here
  const int n_det = ramp_wave_count(det), n_iso = ramp_wave_count(isolated), n_rej = ramp_wave_count(det && !isolated && !lifted),
            n_lift = ramp_wave_count(lifted);
  ramp_wave_flush(status + 1, tid, n_det, n_iso, n_rej, n_lift);
}

__global__ void __launch_bounds__(EVM_THREADS)
    evm_compact_kernel(const float *__restrict__ filt, const int32_t *__restrict__ keep, const int32_t *__restrict__ incl,
                       const float *__restrict__ confidence, const float *__restrict__ cam, const float *__restrict__ intrinsics,
                       int W, long HW, float min_invdepth, float *__restrict__ points, float *__restrict__ conf,
                       int32_t *__restrict__ pixel, int32_t *__restrict__ count) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  if (i == HW - 1) count[0] = incl[i];
  if (!keep[i]) return;
  float c[11], Xw[3];
  evm_load_camera(cam, intrinsics, c);
  evm_lift(c, (int)(i % W), (int)(i / W), filt[i], min_invdepth, Xw);
  const size_t at = (size_t)(incl[i] - 1);
  points[3 * at] = Xw[0];
  points[3 * at + 1] = Xw[1];
  points[3 * at + 2] = Xw[2];
  conf[at] = confidence ? confidence[i] : 1.0f;
  pixel[at] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------------------- the voxel hash
__global__ void __launch_bounds__(EVM_THREADS) evm_clear_kernel(EvmSlot *__restrict__ slots, evm_u64 *__restrict__ header,
                                                                long capacity) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < EVM_HEADER / 8) header[i] = 0;
  if (i >= capacity) return;
  EvmSlot s;
  s.key = EVM_EMPTY;
  s.n = s.sq[0] = s.sq[1] = s.sq[2] = s.sc = s.spare = 0;
  s.views = 0;
  slots[i] = s;
}

__global__ void __launch_bounds__(EVM_THREADS)
    evm_insert_kernel(EvmSlot *slots, evm_u64 *header, long capacity, const float *__restrict__ points,
                      const float *__restrict__ conf, int n_points, const int32_t *__restrict__ count, double voxel, int view,
                      int32_t *status) {
  const int tid = threadIdx.x;
  const int live = count ? min(max(count[0], 0), n_points) : n_points;
  const long i = (long)blockIdx.x * blockDim.x + tid;
  const bool have = i < live;
  bool bad = false, outside = false, full = false, done = false, claimed = false;
  if (have) {
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float cf = conf ? conf[i] : 1.0f;
    bad = !evm_finite(p[0]) || !evm_finite(p[1]) || !evm_finite(p[2]) || !evm_finite(cf) || cf < 0.0f;
    long long idx[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    if (!bad) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double g = (double)p[a] / voxel, fl = floor(g);
        if (!(fabs(fl) < (double)EVM_AXIS)) {
          outside = true;
        } else {
          idx[a] = (long long)fl;
          q[a] = llrint((g - fl) * (double)EVM_AXIS);
        }
      }
    }
    if (!bad && !outside) {
      const long long key = ((idx[0] + EVM_AXIS) << 42) | ((idx[1] + EVM_AXIS) << 21) | (idx[2] + EVM_AXIS);
      const long long cfix = llrint(fmin((double)cf, (double)EVM_AXIS) * (double)(1 << EVM_CONF_BITS));
      const evm_u64 mask = (evm_u64)capacity - 1;
      evm_u64 at = evm_hash((evm_u64)key) & mask;
      // at most `capacity` probes: each one claims, matches or moves on; nothing is waited for
      for (long probe = 0; probe < capacity && !done; probe++) {
        EvmSlot *s = slots + at;
        long long k = __atomic_load_n(&s->key, __ATOMIC_RELAXED);
        if (k == EVM_EMPTY) {
          k = (long long)atomicCAS(reinterpret_cast<evm_u64 *>(&s->key), (evm_u64)EVM_EMPTY, (evm_u64)key);
          if (k == EVM_EMPTY) { claimed = true; k = key; }
        }
        if (k == key) {
          atomicAdd(reinterpret_cast<evm_u64 *>(&s->n), (evm_u64)1);
#pragma unroll
          for (int a = 0; a < 3; a++) atomicAdd(reinterpret_cast<evm_u64 *>(&s->sq[a]), (evm_u64)q[a]);
          atomicAdd(reinterpret_cast<evm_u64 *>(&s->sc), (evm_u64)cfix);
          atomicOr(&s->views, (evm_u64)1 << (view & 63));
          done = true;
        }
        at = (at + 1) & mask;
      }
      full = !done;
    }
  }
  // every lane of the wave is here
  const int n_seen = ramp_wave_count(have), n_bad = ramp_wave_count(bad), n_out = ramp_wave_count(outside),
            n_full = ramp_wave_count(full), n_done = ramp_wave_count(done), n_claimed = ramp_wave_count(claimed);
  ramp_wave_flush(status + 1, tid, n_seen, n_bad, n_out, n_full, n_done);
  if ((tid & (RAMP_WAVE - 1)) == 0 && n_claimed) atomicAdd(header, (evm_u64)n_claimed);
}

__global__ void evm_occupied_kernel(const evm_u64 *__restrict__ header, int32_t *__restrict__ word) { word[0] = (int32_t)header[0]; }

__global__ void __launch_bounds__(EVM_THREADS)
    evm_flag_kernel(const EvmSlot *__restrict__ slots, long capacity, long long min_points, int min_views,
                    evm_u64 *__restrict__ keys, int32_t *__restrict__ vals, int32_t *status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool pass = false;
  if (i < capacity) {
    const EvmSlot *s = slots + i;
    const long long key = s->key;
    pass = key != EVM_EMPTY && s->n >= min_points && __popcll(s->views) >= min_views;      // (evm_slot_passes, loads on demand)
    keys[i] = pass ? (evm_u64)key : ~(evm_u64)0;
    vals[i] = (int32_t)i;
  }
  // every lane of the wave is here
  const int n_pass = ramp_wave_count(pass);
  ramp_wave_flush(status + 1, threadIdx.x, n_pass);
}

__global__ void __launch_bounds__(EVM_THREADS)
    evm_gather_kernel(const EvmSlot *__restrict__ slots, const evm_u64 *__restrict__ header, const int32_t *__restrict__ order,
                      double voxel, int max_out, float *__restrict__ points, int32_t *__restrict__ n_out,
                      float *__restrict__ conf, int32_t *__restrict__ n_views, int64_t *__restrict__ key_out,
                      int32_t *__restrict__ count, int32_t *status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int passing = status[1];                         // (the flag launch is complete)
  const int K = min(passing, max_out);
  if (i == 0) {
    count[0] = K;
    status[2] = passing - K;
    status[3] = (int32_t)header[0];
  }
  if (i >= K) return;
  const EvmSlot *s = slots + order[i];
  const long long key = s->key, n = s->n;
#pragma unroll
  for (int a = 0; a < 3; a++) points[3 * i + a] = evm_mean_axis(key, s->sq[a], n, a, voxel);
  n_out[i] = evm_count_word(n);
  conf[i] = evm_conf_word(s->sc);
  n_views[i] = __popcll(s->views);
  key_out[i] = key;
}

// ------------------------------------------------------------------------------------------------------------ workspaces
struct EvmPointsWs {
  float *filt;
  int32_t *keep, *incl;
  void *cub;
  size_t cub_bytes;
};
static size_t evm_points_carve(void *ws, size_t HW, EvmPointsWs *w) {
  size_t scan = 0;
  int32_t *v = nullptr;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, scan, v, v, (int)HW, (hipStream_t)0);
  WsCarver c(ws);
  w->filt = c.take<float>(HW, 256);
  w->keep = c.take<int32_t>(HW, 256);
  w->incl = c.take<int32_t>(HW, 256);
  w->cub_bytes = round_up(scan + 256, 256);
  w->cub = c.take<char>(w->cub_bytes, 256);
  return c.bytes();
}

struct EvmExportWs {
  evm_u64 *keys_in, *keys_out;
  int32_t *vals_in, *vals_out;
  void *cub;
  size_t cub_bytes;
};
static size_t evm_export_carve(void *ws, size_t capacity, EvmExportWs *w) {
  size_t sort = 0;
  evm_u64 *k = nullptr;
  int32_t *v = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort, k, k, v, v, (int)capacity, 0, 64, (hipStream_t)0);
  WsCarver c(ws);
  w->keys_in = c.take<evm_u64>(capacity, 256);
  w->keys_out = c.take<evm_u64>(capacity, 256);
  w->vals_in = c.take<int32_t>(capacity, 256);
  w->vals_out = c.take<int32_t>(capacity, 256);
  w->cub_bytes = round_up(sort + 256, 256);
  w->cub = c.take<char>(w->cub_bytes, 256);
  return c.bytes();
}

extern "C" {
size_t ramp_depth_points_ws_bytes(int H, int W) {
  if (H < 1 || W < 1 || (double)H * (double)W >= 2147483648.0) return 0;
  EvmPointsWs w;
  return evm_points_carve(nullptr, (size_t)H * W, &w);
}

int ramp_depth_points(const float *invdepth, const int32_t *plane, const float *confidence, const float *cam,
                      const float *intrinsics, int H, int W, int median_radius, int min_support, float min_invdepth,
                      float *points, float *conf, int32_t *pixel, float *invdepth_filtered, int32_t *count, void *ws,
                      size_t ws_bytes, int32_t *status, void *stream) {
  if (H < 1 || W < 1 || median_radius < 0 || median_radius > EVM_RMAX || min_support < 1) return RAMP_EINVAL;
  if (!(min_invdepth >= 0.0f) || !(min_invdepth <= 3.4028234663852886e38f)) return RAMP_EINVAL;
  if (!invdepth || !cam || !intrinsics || !points || !conf || !pixel || !count || !ws || !status) return RAMP_EINVAL;
  if (((uintptr_t)ws & 255) != 0) return RAMP_EINVAL;
  if ((double)H * (double)W >= 2147483648.0) return RAMP_EUNSUPPORTED;
  const size_t HW = (size_t)H * W;
  EvmPointsWs w;
  if (ws_bytes < evm_points_carve(ws, HW, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const unsigned tiles = (unsigned)ramp_cdiv(W, EVM_TW) * (unsigned)ramp_cdiv(H, EVM_TH);
  hipLaunchKernelGGL(evm_filter_kernel, dim3(tiles), dim3(EVM_THREADS), 0, st, invdepth, plane, cam, intrinsics, H, W,
                     median_radius, min_support, min_invdepth, w.filt, w.keep, invdepth_filtered, status);
  RAMP_CHECK_LAUNCH();
  size_t cub_bytes = w.cub_bytes;
  if (hipcub::DeviceScan::InclusiveSum(w.cub, cub_bytes, w.keep, w.incl, (int)HW, st) != hipSuccess) return RAMP_ELAUNCH;
  hipLaunchKernelGGL(evm_compact_kernel, dim3((unsigned)((HW + EVM_THREADS - 1) / EVM_THREADS)), dim3(EVM_THREADS), 0, st, w.filt,
                     w.keep, w.incl, confidence, cam, intrinsics, W, (long)HW, min_invdepth, points, conf, pixel, count);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

size_t ramp_point_map_bytes(long capacity) {
  return evm_capacity_ok(capacity) ? (size_t)EVM_HEADER + (size_t)capacity * sizeof(EvmSlot) : 0;
}

int ramp_point_map_clear(void *map, long capacity, void *stream) {
  if (!map || !evm_capacity_ok(capacity) || ((uintptr_t)map & 63) != 0) return RAMP_EINVAL;
  hipLaunchKernelGGL(evm_clear_kernel, dim3((unsigned)((capacity + EVM_THREADS - 1) / EVM_THREADS)), dim3(EVM_THREADS), 0,
                     (hipStream_t)stream, evm_slots(map), reinterpret_cast<evm_u64 *>(map), capacity);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

int ramp_point_map_insert(void *map, long capacity, const float *points, const float *conf, int n_points, const int32_t *count,
                          double voxel, int view, int32_t *status, void *stream) {
  if (!map || !evm_capacity_ok(capacity) || ((uintptr_t)map & 63) != 0 || !status) return RAMP_EINVAL;
  if (n_points < 0 || (n_points > 0 && !points) || view < 0) return RAMP_EINVAL;
  if (!(voxel > 0.0) || !(voxel <= 1.7976931348623157e308)) return RAMP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  evm_u64 *header = reinterpret_cast<evm_u64 *>(map);
  if (n_points > 0) {
    hipLaunchKernelGGL(evm_insert_kernel, dim3((unsigned)ramp_cdiv(n_points, EVM_THREADS)), dim3(EVM_THREADS), 0, st, evm_slots(map),
                       header, capacity, points, conf, n_points, count, voxel, view, status);
    RAMP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(evm_occupied_kernel, dim3(1), dim3(1), 0, st, header, status + 6);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

size_t ramp_point_map_export_ws_bytes(long capacity) {
  if (!evm_capacity_ok(capacity)) return 0;
  EvmExportWs w;
  return evm_export_carve(nullptr, (size_t)capacity, &w);
}

int ramp_point_map_export(const void *map, long capacity, double voxel, long min_points, int min_views, int max_out,
                          float *points, int32_t *n, float *conf, int32_t *n_views, int64_t *key, int32_t *count, void *ws,
                          size_t ws_bytes, int32_t *status, void *stream) {
  if (!map || !evm_capacity_ok(capacity) || ((uintptr_t)map & 63) != 0 || !status || !count || !ws) return RAMP_EINVAL;
  if (min_points < 0 || min_views < 0 || max_out < 0) return RAMP_EINVAL;
  if (max_out > 0 && (!points || !n || !conf || !n_views || !key)) return RAMP_EINVAL;
  if (!(voxel > 0.0) || !(voxel <= 1.7976931348623157e308)) return RAMP_EINVAL;
  if (((uintptr_t)ws & 255) != 0 || ((uintptr_t)key & 7) != 0) return RAMP_EINVAL;
  EvmExportWs w;
  if (ws_bytes < evm_export_carve(ws, (size_t)capacity, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const EvmSlot *slots = evm_slots(const_cast<void *>(map));
  const evm_u64 *header = reinterpret_cast<const evm_u64 *>(map);
  hipLaunchKernelGGL(evm_flag_kernel, dim3((unsigned)((capacity + EVM_THREADS - 1) / EVM_THREADS)), dim3(EVM_THREADS), 0, st, slots,
                     capacity, (long long)min_points, min_views, w.keys_in, w.vals_in, status);
  RAMP_CHECK_LAUNCH();
  size_t cub_bytes = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.keys_in, w.keys_out, w.vals_in, w.vals_out, (int)capacity, 0, 64,
                                         st) != hipSuccess)
    return RAMP_ELAUNCH;
  const long bound = capacity < (long)max_out ? capacity : (long)max_out;
  hipLaunchKernelGGL(evm_gather_kernel, dim3((unsigned)((bound < 1 ? 1 : bound) + EVM_THREADS - 1) / EVM_THREADS), dim3(EVM_THREADS), 0,
                     st, slots, header, w.vals_out, voxel, max_out, points, n, conf, n_views, key, count, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
