// Event map rendering (include/ramp_hip.h: ramp_point_map_render): the voxel hash of evmap.hip seen from any camera as a
// z-buffered [H][W] map of inverse depth -- the map the event warp samples with RAMP_WARP_DEPTH_MAP.
//
// One lane per SLOT reads the table where it is (no sort, no export); one hipMemsetAsync (the status words) and four launches:
//   mrd_clear_kernel    per pixel: the depth word 0 (no float > 0 has these bits), the key word ~0 (above every voxel's key)
//   mrd_depth_kernel    per slot: the export's conditions, the export's mean point (evmap_device.h), the projection, the
//                       footprint, the counters (one ballot per counter and wave), the optional record; per covered pixel a
//                       32-bit atomicMax of the bits of d' (d' > 0: the order of the bits is the order of the floats)
//   mrd_key_kernel      per slot: the same statements again (the same bits); per covered pixel whose depth word holds this
//                       slot's bits a 64-bit atomicMin of the key: among equal depths the lowest key wins
//   mrd_resolve_kernel  per pixel, one writer: the depth word back as a float, the winning key looked up in the hash by a
//                       read-only probe bounded by `capacity`, n and conf as the export forms them
// Both atomics are return-less and sit behind a relaxed load of the word: a lane whose value cannot change the word issues
// nothing (the words only grow / only shrink, so a stale load costs an atomic, never a result).  Integer max and min do not
// depend on the order of their operands: the image depends neither on the slots' order nor on the launch's schedule.  No lane
// waits for another one.
#include "evmap_device.h"

#define MRD_RMAX 7                         // the largest radius: a footprint of at most 15 x 15 pixels
#define MRD_NONE (~(evm_u64)0)             // the key word of a pixel without a winner: -1 as the int64 the caller sees

struct MrdWs {
  unsigned *depth;                         // [H * W] the bits of the largest d'
  evm_u64 *key;                            // [H * W] the lowest key among the slots with those bits
};
static size_t mrd_carve(void *ws, size_t HW, MrdWs *w) {
  WsCarver c(ws);
  w->depth = c.take<unsigned>(HW, 256);
  w->key = c.take<evm_u64>(HW, 256);
  return c.bytes();
}

// what a slot is to the image
enum { MRD_ABSENT = 0, MRD_FILTERED, MRD_REJECTED, MRD_OUTSIDE, MRD_RENDERED };
struct MrdSplat {
  int kind;
  long long key;
  float u, v, d;
  int r;                                   // r_p
  int x0, x1, y0, y1;                      // the square clipped to the image (MRD_RENDERED)
};

// The statements of the header, for one slot: both slot kernels call this, so both see the same bits.
static __device__ __forceinline__ MrdSplat mrd_splat(const EvmSlot *__restrict__ s, const float *c, double voxel, long long min_points,
                                                     int min_views, int H, int W, int radius, int footprint) {
  MrdSplat o;
  o.kind = MRD_ABSENT;
  o.u = o.v = o.d = __int_as_float(0x7fc00000);
  o.r = o.x0 = o.x1 = o.y0 = o.y1 = 0;
  const long long key = s->key;
  o.key = key;
  if (key == EVM_EMPTY) return o;
  const long long n = s->n;
  if (!evm_slot_passes(key, n, s->views, min_points, min_views)) { o.kind = MRD_FILTERED; return o; }
  float Xc[3], d, u, v;
  if (!evm_project(key, s->sq, n, c, voxel, Xc, &d, &u, &v)) {
    o.kind = MRD_REJECTED;
    return o;
  }
  int r = radius;
  if (footprint) {                          // half the voxel's projected edge, float64
    const double rho = 0.5 * voxel * (double)fmaxf(fabsf(c[7]), fabsf(c[8])) * (double)d;
    const double e = ceil(rho - 0.5);
    r = !(e < (double)radius) ? radius : (e > 0.0 ? (int)e : 0);
  }
  o.u = u; o.v = v; o.d = d; o.r = r;
  // the centre pixel and the test of the square against the image, before any conversion to an integer
  const double px = (double)rintf(u), py = (double)rintf(v);
  if (!(px + (double)r >= 0.0 && px - (double)r <= (double)(W - 1) && py + (double)r >= 0.0 && py - (double)r <= (double)(H - 1))) {
    o.kind = MRD_OUTSIDE;
    return o;
  }
  const long ix = (long)px, iy = (long)py;  // within MRD_RMAX of the image: far inside a long
  o.x0 = (int)max(ix - r, 0l); o.x1 = (int)min(ix + r, (long)W - 1);
  o.y0 = (int)max(iy - r, 0l); o.y1 = (int)min(iy + r, (long)H - 1);
  o.kind = MRD_RENDERED;
  return o;
}

__global__ void __launch_bounds__(EVM_THREADS) mrd_clear_kernel(unsigned *__restrict__ depth, evm_u64 *__restrict__ key, long HW) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  depth[i] = 0u;
  key[i] = MRD_NONE;
}

__global__ void __launch_bounds__(EVM_THREADS)
    mrd_depth_kernel(const EvmSlot *__restrict__ slots, long capacity, double voxel, long long min_points, int min_views,
                     const float *__restrict__ cam, const float *__restrict__ intrinsics, int H, int W, int radius, int footprint,
                     unsigned *depth, float *__restrict__ records, int32_t *status) {
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * blockDim.x + tid;
  float c[11];
  const bool failed = evm_load_camera(cam, intrinsics, c);
  if (blockIdx.x == 0 && tid == 0 && failed) status[0] = RAMP_MAP_RENDER_BAD_CAMERA;
  MrdSplat o;
  o.kind = MRD_ABSENT;
  o.u = o.v = o.d = __int_as_float(0x7fc00000);
  o.r = 0;
  if (i < capacity && !failed) o = mrd_splat(slots + i, c, voxel, min_points, min_views, H, W, radius, footprint);
  if (i < capacity && records) {
    const bool row = o.kind == MRD_OUTSIDE || o.kind == MRD_RENDERED;
    const float nan = __int_as_float(0x7fc00000);
    float *rec = records + 4 * (size_t)i;
    rec[0] = row ? o.u : nan;
    rec[1] = row ? o.v : nan;
    rec[2] = row ? o.d : nan;
    rec[3] = row ? (float)o.r : nan;
  }
  if (o.kind == MRD_RENDERED) {
    const unsigned bits = __float_as_uint(o.d);
    for (int y = o.y0; y <= o.y1; y++)
      for (int x = o.x0; x <= o.x1; x++) {
        unsigned *word = depth + ((size_t)y * W + x);
        if (__atomic_load_n(word, __ATOMIC_RELAXED) < bits) atomicMax(word, bits);
      }
  }
  // every lane of the wave is here
  const int n_occ = ramp_wave_count(o.kind != MRD_ABSENT), n_filt = ramp_wave_count(o.kind == MRD_FILTERED),
            n_rej = ramp_wave_count(o.kind == MRD_REJECTED), n_out = ramp_wave_count(o.kind == MRD_OUTSIDE),
            n_ren = ramp_wave_count(o.kind == MRD_RENDERED);
  ramp_wave_flush(status + 1, tid, n_occ, n_filt, n_rej, n_out, n_ren);
}

__global__ void __launch_bounds__(EVM_THREADS)
    mrd_key_kernel(const EvmSlot *__restrict__ slots, long capacity, double voxel, long long min_points, int min_views,
                   const float *__restrict__ cam, const float *__restrict__ intrinsics, int H, int W, int radius, int footprint,
                   const unsigned *__restrict__ depth, evm_u64 *key) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= capacity) return;
  float c[11];
  if (evm_load_camera(cam, intrinsics, c)) return;
  const MrdSplat o = mrd_splat(slots + i, c, voxel, min_points, min_views, H, W, radius, footprint);
  if (o.kind != MRD_RENDERED) return;
  const unsigned bits = __float_as_uint(o.d);
  const evm_u64 mine = (evm_u64)o.key;
  for (int y = o.y0; y <= o.y1; y++)
    for (int x = o.x0; x <= o.x1; x++) {
      const size_t at = (size_t)y * W + x;
      if (depth[at] == bits && __atomic_load_n(key + at, __ATOMIC_RELAXED) > mine) atomicMin(key + at, mine);
    }
}

__global__ void __launch_bounds__(EVM_THREADS)
    mrd_resolve_kernel(const EvmSlot *__restrict__ slots, long capacity, const float *__restrict__ cam,
                       const float *__restrict__ intrinsics, long HW, const unsigned *__restrict__ depth,
                       const evm_u64 *__restrict__ key, const float *__restrict__ fill, float *__restrict__ invdepth,
                       int64_t *__restrict__ key_out, int32_t *__restrict__ n_out, float *__restrict__ conf_out, int32_t *status) {
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * blockDim.x + tid;
  float c[11];
  const bool failed = evm_load_camera(cam, intrinsics, c);
  const float nan = __int_as_float(0x7fc00000);
  bool won = false;
  if (i < HW) {
    const evm_u64 k = key[i];
    won = !failed && k != MRD_NONE;
    float d = failed ? nan : (fill ? fill[0] : nan), cf = failed ? nan : 0.0f;
    int32_t n = 0;
    if (won) {
      d = __uint_as_float(depth[i]);
      // the winner's slot: the insert's probe sequence, read only, at most `capacity` probes
      const evm_u64 mask = (evm_u64)capacity - 1;
      evm_u64 at = evm_hash(k) & mask;
      cf = nan;
      for (long probe = 0; probe < capacity; probe++) {
        const EvmSlot *s = slots + at;
        const long long have = s->key;
        if (have == (long long)k) {
          n = evm_count_word(s->n);
          cf = evm_conf_word(s->sc);
          break;
        }
        if (have == EVM_EMPTY) break;
        at = (at + 1) & mask;
      }
    }
    invdepth[i] = d;
    if (key_out) key_out[i] = won ? (int64_t)k : (int64_t)-1;
    if (n_out) n_out[i] = n;
    if (conf_out) conf_out[i] = cf;
  }
  // every lane of the wave is here
  const int n_won = ramp_wave_count(won);
  ramp_wave_flush(status + 6, tid, n_won);
}

extern "C" {
size_t ramp_point_map_render_ws_bytes(int H, int W) {
  if (H < 1 || W < 1 || (double)H * (double)W >= 2147483648.0) return 0;
  MrdWs w;
  return mrd_carve(nullptr, (size_t)H * W, &w);
}

int ramp_point_map_render(const void *map, long capacity, double voxel, long min_points, int min_views, const float *cam,
                          const float *intrinsics, int H, int W, int radius, int footprint, const float *fill, float *invdepth,
                          int64_t *key, int32_t *n, float *conf, float *records, void *ws, size_t ws_bytes, int32_t *status,
                          void *stream) {
  if (H < 1 || W < 1 || radius < 0 || radius > MRD_RMAX || !evm_capacity_ok(capacity)) return RAMP_EINVAL;
  if (!(voxel > 0.0) || !(voxel <= 1.7976931348623157e308) || min_points < 0 || min_views < 0) return RAMP_EINVAL;
  if (!map || !cam || !intrinsics || !invdepth || !ws || !status) return RAMP_EINVAL;
  if (((uintptr_t)map & 63) != 0 || ((uintptr_t)ws & 255) != 0 || ((uintptr_t)key & 7) != 0) return RAMP_EINVAL;
  if ((double)H * (double)W >= 2147483648.0) return RAMP_EUNSUPPORTED;
  const size_t HW = (size_t)H * W;
  MrdWs w;
  if (ws_bytes < mrd_carve(ws, HW, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const EvmSlot *slots = evm_slots(const_cast<void *>(map));
  const dim3 per_pixel((unsigned)((HW + EVM_THREADS - 1) / EVM_THREADS)), per_slot((unsigned)((capacity + EVM_THREADS - 1) / EVM_THREADS));
  hipLaunchKernelGGL(mrd_clear_kernel, per_pixel, dim3(EVM_THREADS), 0, st, w.depth, w.key, (long)HW);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(mrd_depth_kernel, per_slot, dim3(EVM_THREADS), 0, st, slots, capacity, voxel, (long long)min_points, min_views, cam,
                     intrinsics, H, W, radius, footprint, w.depth, records, status);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(mrd_key_kernel, per_slot, dim3(EVM_THREADS), 0, st, slots, capacity, voxel, (long long)min_points, min_views, cam,
                     intrinsics, H, W, radius, footprint, w.depth, w.key);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(mrd_resolve_kernel, per_pixel, dim3(EVM_THREADS), 0, st, slots, capacity, cam, intrinsics, (long)HW, w.depth,
                     w.key, fill, invdepth, key, n, conf, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
