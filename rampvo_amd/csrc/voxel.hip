// Event voxel grids (include/ramp_hip.h: ramp_event_voxel): the reference's second event representation
// (utils/transformers.py, EventSequenceToVoxelGrid_Pytorch) for many slices of one event list in one call.  Every event
// votes into the two time bins next to its normalised time stamp with linear weights; the grid of a slice is then
// standardised over its non-zero cells.
//
//   t_first, t_last = the time stamps of the slice's first and last event BY POSITION;  deltaT = t_last - t_first, 1 when 0
//   tn  = ((bins - 1) * (t - t_first)) / deltaT          float64, in this order
//   ti  = floor(tn),  dts = float32(tn - ti),  pol = p (0 is read as -1)
//   pol * (1 - dts) -> bin ti      when 0 <= ti < bins
//   pol * dts       -> bin ti + 1  when 0 <= ti and ti + 1 < bins
//
// The pixel is the coordinate truncated toward zero, or with RAMP_VOXEL_SUBPIXEL the bilinear neighbours of warp_axis
// (warp_device.h), a neighbour's share being (wx * wy) * value in fp32.  An event outside the image is dropped and counted.
//
// Per chunk of slices that fits the workspace, four launches behind one memset of the accumulators:
//   vox_vote_kernel    tiles of WARP_TILE events staged in LDS with 16-byte loads, one event per lane and trip: the slice by
//                      a binary search over the chunk's offsets (LDS up to VOX_LDS_OFFSETS), up to eight 64-bit integer
//                      atomics per event into the int64 accumulators [slices][bins][H][W]
//   vox_count_kernel   per slice the number n of non-zero cells and their sum: integer wave reductions, integer atomics
//   vox_spread_kernel  with mean = sum / (n 2^24) known, per-workgroup partials of sum (acc 2^-24 - mean)^2 in float64
//   vox_finish_kernel  the partials of the slice in index order -> std; accumulators -> fp32 grid, stats, status
// and, once per call, vox_offsets_kernel in front of the first vote: the check of the offsets.
//
// The votes are FIXED POINT as in the event warp: llrint(value * 2^24) added with 64-bit integer atomics.  Integer addition
// commutes, so the accumulators, n, sum and mean do not depend on the order of the events or on the chunking, and a call
// repeats its bits; the squares are summed in an order fixed by (bins, H, W) alone.  No floating-point atomics.
#include "ramp_internal.h"
#include "warp_device.h"

#define VOX_LDS_OFFSETS 1024             // offsets of a chunk staged in LDS up to here (8 KiB); more: search in global memory
#define VOX_MAX_CHUNK 32768              // slices per chunk at most
#define VOX_STAT_GROUPS 256              // workgroups per slice of the count, spread and finish launches at most
#define VOX_CTR_WORDS 16                 // int32: the 8 status words, 8 spare
#define VOX_WAVES (INTERP_THREADS / RAMP_WAVE)
#define VOX_BAD_OFFSETS RAMP_VOXEL_BAD_OFFSETS
#define VOX_BAD_TIMES RAMP_VOXEL_BAD_TIMES

struct VoxArgs {
  const float *x, *y;
  const double *t;
  const int8_t *p;
  const long long *offsets;              // the chunk's sc + 1 offsets, or nullptr: one slice [0, N)
  long long *acc;                        // [sc][bins][H][W]
  int32_t *ctr;
  long N;
  int sc, bins, H, W;
};

// the number of offsets <= i among n
template <typename P>
static __device__ __forceinline__ int vox_upper_bound(P off, int n, long long i) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid + 1; else hi = mid;
  }
  return lo;
}

static __device__ __forceinline__ void vox_bounds(const long long *off, int s, long N, long long *lo, long long *hi) {
  *lo = off ? off[s] : 0;
  *hi = off ? off[s + 1] : (long long)N;
}

// the first time stamp and the span of the non-empty slice [lo, hi); false when its first or last stamp is not finite
static __device__ __forceinline__ bool vox_slice_times(const double *__restrict__ t, long long lo, long long hi, double *t0,
                                                       double *dT) {
  const double a = t[lo], b = t[hi - 1];
  const double d = b - a;
  *t0 = a;
  *dT = d == 0.0 ? 1.0 : d;
  return interp_finite(a) && interp_finite(b);
}

static __device__ __forceinline__ long long vox_fixed(float v) { return __float2ll_rn(ldexpf(v, WARP_FIX_BITS)); }

static __device__ __forceinline__ void vox_add(long long *cell, long long c) {
  if (c != 0) atomicAdd(reinterpret_cast<warp_u64 *>(cell), (warp_u64)c);
}

// offsets that are negative, exceed N or decrease: bit 0 of the status word, raised in front of the first vote
__global__ void __launch_bounds__(INTERP_THREADS)
    vox_offsets_kernel(const long long *__restrict__ off, int S, long N, int32_t *__restrict__ ctr) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > S) return;
  const long long v = off[i];
  bool bad = v < 0 || v > (long long)N;
  if (i < S) bad = bad || off[i + 1] < v;
  if (bad) atomicOr(ctr, VOX_BAD_OFFSETS);
}

// OFFS: 0 one slice [0, N); 1 the chunk's offsets staged in LDS; 2 searched in global memory.  SUB: bilinear pixels.  VEC: full
// tiles are loaded with 16-byte loads (every event array 16-byte aligned).
template <int OFFS, bool SUB, bool VEC>
__global__ void __launch_bounds__(INTERP_THREADS) vox_vote_kernel(const VoxArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vox_smem[];
  __shared__ __attribute__((aligned(16))) double s_t[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_x[WARP_TILE];
  __shared__ __attribute__((aligned(16))) float s_y[WARP_TILE];
  __shared__ __attribute__((aligned(16))) int8_t s_p[WARP_TILE];
  long long *s_off = reinterpret_cast<long long *>(vox_smem);
  const int tid = threadIdx.x;
  const long N = a.N;
  const int sc = a.sc, bins = a.bins, H = a.H, W = a.W;
  if (a.ctr[0] & VOX_BAD_OFFSETS) return;            // (raised by the check in front: no offset is trusted, nothing is read)
  long long e0 = 0, e1 = (long long)N;
  if (OFFS) { e0 = a.offsets[0]; e1 = a.offsets[sc]; }
  if (e1 <= e0) return;
  if (OFFS == 1)
    for (int i = tid; i <= sc; i += INTERP_THREADS) s_off[i] = a.offsets[i];
  const size_t HW = (size_t)H * W;
  // tiles are aligned to the event arrays, not to the chunk: the chunk's first and last tile are masked
  const long tile0 = (long)(e0 / WARP_TILE), tile1 = (long)((e1 - 1) / WARP_TILE) + 1;
  int n_seen = 0, n_bad = 0, n_out = 0, n_time = 0, n_in = 0;               // wave-uniform: sums of ballots
  for (long tile = tile0 + blockIdx.x; tile < tile1; tile += gridDim.x) {
    const long base = tile * WARP_TILE;
    const int live = (int)min((long)WARP_TILE, N - base);
    __syncthreads();                                 // (the staged offsets; the previous tile has been read)
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
      const long long i = (long long)base + e;
      const bool have = e < live && i >= e0 && i < e1;
      bool bad = false, outside = false, no_bin = false, inside = false;
      if (have) {
        const float x = s_x[e], y = s_y[e];
        const double t = s_t[e];
        int s = 0;
        long long lo = e0, hi = e1;
        if (OFFS == 1) {
          s = vox_upper_bound(s_off, sc + 1, i) - 1;
          lo = s_off[s];
          hi = s_off[s + 1];
        } else if (OFFS == 2) {
          s = vox_upper_bound(a.offsets, sc + 1, i) - 1;
          lo = a.offsets[s];
          hi = a.offsets[s + 1];
        }
        int ix = 0, iy = 0;
        float wx[2] = {1.0f, 0.0f}, wy[2] = {1.0f, 0.0f};
        bool inx[2] = {false, false}, iny[2] = {false, false};
        if (!warp_event_finite(x, y, t)) {
          bad = true;
        } else if (SUB) {
          warp_axis(x, W, &ix, &wx[0], &wx[1], &inx[0], &inx[1]);
          warp_axis(y, H, &iy, &wy[0], &wy[1], &iny[0], &iny[1]);
          // a neighbour of weight zero does not make a pixel: integer coordinates count as the truncated pixel does
          outside = !(((inx[0] && wx[0] != 0.0f) || (inx[1] && wx[1] != 0.0f)) &&
                      ((iny[0] && wy[0] != 0.0f) || (iny[1] && wy[1] != 0.0f)));
        } else {
          const float xt = truncf(x), yt = truncf(y);  // (the range test is made in float, as warp_axis makes it)
          inx[0] = xt >= 0.0f && xt <= (float)(W - 1);
          iny[0] = yt >= 0.0f && yt <= (float)(H - 1);
          outside = !(inx[0] && iny[0]);
          if (!outside) { ix = (int)xt; iy = (int)yt; }
        }
        if (!bad && !outside) {
          double t0, dT;
          const bool ok = vox_slice_times(a.t, lo, hi, &t0, &dT);
          const double tn = ((double)(bins - 1) * (t - t0)) / dT;
          const double ti = floor(tn);
          if (!ok || !(ti >= 0.0 && ti < (double)bins)) {
            no_bin = true;
          } else {
            inside = true;
            const int b = (int)ti;
            const float dts = (float)(tn - ti);
            const float pol = s_p[e] == 0 ? -1.0f : (float)s_p[e];         // (0 is read as -1, like ops.event_stack)
            const float vl = pol * (1.0f - dts), vr = pol * dts;
            const bool right = b + 1 < bins;
            long long *plane = a.acc + ((size_t)s * bins + b) * HW;
            if (!SUB) {
              const size_t at = (size_t)iy * W + (size_t)ix;
              vox_add(plane + at, vox_fixed(vl));
              if (right) vox_add(plane + HW + at, vox_fixed(vr));
            } else {
#pragma unroll
              for (int jy = 0; jy < 2; jy++)
#pragma unroll
                for (int jx = 0; jx < 2; jx++)
                  if (inx[jx] && iny[jy]) {
                    const float w = __fmul_rn(wx[jx], wy[jy]);
                    const size_t at = (size_t)(iy + jy) * W + (size_t)(ix + jx);
                    vox_add(plane + at, vox_fixed(__fmul_rn(w, vl)));
                    if (right) vox_add(plane + HW + at, vox_fixed(__fmul_rn(w, vr)));
                  }
            }
          }
        }
      }
      // the trip count and `have` aside, every lane of the wave is here
      n_seen += ramp_wave_count(have);
      n_bad += ramp_wave_count(bad);
      n_out += ramp_wave_count(outside);
      n_time += ramp_wave_count(no_bin);
      n_in += ramp_wave_count(inside);
    }
  }
  ramp_wave_flush(a.ctr + 1, tid, n_seen, n_bad, n_out, n_time, n_in);
}

// workgroup r of the P that share slice s: the number of non-zero cells and their sum, both integers
__global__ void __launch_bounds__(INTERP_THREADS)
    vox_count_kernel(const long long *__restrict__ acc, const long long *__restrict__ off, const double *__restrict__ t, long N,
                     long C, int P, long long *__restrict__ sums, int32_t *__restrict__ ctr) {
  if (ctr[0] & VOX_BAD_OFFSETS) return;
  const int tid = threadIdx.x, s = blockIdx.x / P, r = blockIdx.x % P;
  const long long *cell = acc + (size_t)s * C;
  long long n = 0, sum = 0;
  for (long i = (long)r * INTERP_THREADS + tid; i < C; i += (long)P * INTERP_THREADS) {
    const long long v = cell[i];
    n += v != 0;
    sum += v;
  }
  n = ramp_wave_sum(n);
  sum = ramp_wave_sum(sum);
  if ((tid & (RAMP_WAVE - 1)) == 0) {
    if (n) atomicAdd(reinterpret_cast<warp_u64 *>(sums + 2 * (size_t)s), (warp_u64)n);
    if (sum) atomicAdd(reinterpret_cast<warp_u64 *>(sums + 2 * (size_t)s + 1), (warp_u64)sum);
  }
  if (r == 0 && tid == 0) {
    long long lo, hi;
    double t0, dT;
    vox_bounds(off, s, N, &lo, &hi);
    if (hi > lo && !vox_slice_times(t, lo, hi, &t0, &dT)) atomicOr(ctr, VOX_BAD_TIMES);
  }
}

static __device__ __forceinline__ double vox_mean(long long n, long long sum) {
  return n ? (double)sum / ((double)n * (double)(1 << WARP_FIX_BITS)) : 0.0;
}

// the same workgroups: the centred squares of the slice's non-zero cells, one partial per workgroup
__global__ void __launch_bounds__(INTERP_THREADS)
    vox_spread_kernel(const long long *__restrict__ acc, long C, int P, const long long *__restrict__ sums,
                      const int32_t *__restrict__ ctr, double *__restrict__ part) {
  __shared__ double s_red[VOX_WAVES];
  if (ctr[0] & VOX_BAD_OFFSETS) return;
  const int tid = threadIdx.x, s = blockIdx.x / P, r = blockIdx.x % P;
  const long long *cell = acc + (size_t)s * C;
  const double fix = 1.0 / (double)(1 << WARP_FIX_BITS);
  const double mean = vox_mean(sums[2 * (size_t)s], sums[2 * (size_t)s + 1]);
  double c2 = 0.0;
  for (long i = (long)r * INTERP_THREADS + tid; i < C; i += (long)P * INTERP_THREADS) {
    const long long v = cell[i];
    if (v != 0) {
      const double d = (double)v * fix - mean;
      c2 += d * d;
    }
  }
  c2 = ramp_wave_sum(c2);
  if ((tid & (RAMP_WAVE - 1)) == 0) s_red[tid / RAMP_WAVE] = c2;
  __syncthreads();
  if (tid == 0) {
    double v = 0.0;
    for (int w = 0; w < VOX_WAVES; w++) v += s_red[w];
    part[(size_t)s * P + r] = v;
  }
}

// the same workgroups: the slice's partials in index order -> std; the accumulators -> the fp32 grid; workgroup 0 of a slice
// writes its stats row, workgroup 0 of the call's last chunk the status words
__global__ void __launch_bounds__(INTERP_THREADS)
    vox_finish_kernel(const long long *__restrict__ acc, const long long *__restrict__ off, const double *__restrict__ t, long N,
                      long C, int P, const long long *__restrict__ sums, const double *__restrict__ part,
                      const int32_t *__restrict__ ctr, int normalize, int last, float *__restrict__ grid,
                      double *__restrict__ stats, int32_t *__restrict__ status) {
  __shared__ double s_var;
  const int tid = threadIdx.x, s = blockIdx.x / P, r = blockIdx.x % P;
  bool failed = (ctr[0] & VOX_BAD_OFFSETS) != 0;
  if (!failed) {
    long long lo, hi;
    double t0, dT;
    vox_bounds(off, s, N, &lo, &hi);
    failed = hi > lo && !vox_slice_times(t, lo, hi, &t0, &dT);
  }
  if (tid < RAMP_WAVE) {                                // one wave: lane q takes the partials q, q + 64, ..., then a butterfly
    double v = 0.0;
    if (!failed)
      for (int q = tid; q < P; q += RAMP_WAVE) v += part[(size_t)s * P + q];
    v = ramp_wave_sum(v);
    if (tid == 0) s_var = v;
  }
  __syncthreads();
  const float qnan = __int_as_float(0x7fc00000), scale = 1.0f / (float)(1 << WARP_FIX_BITS);
  const double dnan = __longlong_as_double(0x7ff8000000000000ll);
  const double fix = 1.0 / (double)(1 << WARP_FIX_BITS);
  const long long n = failed ? 0 : sums[2 * (size_t)s], sum = failed ? 0 : sums[2 * (size_t)s + 1];
  const double mean = vox_mean(n, sum);
  const double sd = n ? sqrt(s_var / (double)(n - 1)) : 0.0;     // (n == 1: 0 / 0, the unbiased std of one value is NaN)
  const long long *cell = acc + (size_t)s * C;
  float *out = grid + (size_t)s * C;
  for (long i = (long)r * INTERP_THREADS + tid; i < C; i += (long)P * INTERP_THREADS) {
    const long long v = cell[i];
    float g;
    if (failed) {
      g = qnan;
    } else if (!normalize) {
      g = (float)v * scale;                              // int64 -> fp32 rounds once; the power of two is exact
    } else if (v == 0) {
      g = 0.0f;
    } else {
      const double d = (double)v * fix - mean;
      g = sd > 0.0 ? (float)(d / sd) : (float)d;
    }
    out[i] = g;
  }
  if (r == 0 && tid == 0) {
    double *row = stats + 4 * (size_t)s;
    row[0] = failed ? dnan : (double)n;
    row[1] = failed ? dnan : mean;
    row[2] = failed ? dnan : sd;
    row[3] = failed ? dnan : (double)sum * fix;
  }
  if (last && blockIdx.x == 0 && tid < 8) status[tid] = tid < 6 ? ctr[tid] : 0;
}

template <int OFFS, bool SUB>
static void vox_launch_vote(const VoxArgs &a, bool vec, int grid, size_t lds, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((vox_vote_kernel<OFFS, SUB, true>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
  else hipLaunchKernelGGL((vox_vote_kernel<OFFS, SUB, false>), dim3(grid), dim3(INTERP_THREADS), lds, st, a);
}

static int vox_stat_groups(long C) {
  const long n = (C + INTERP_THREADS - 1) / INTERP_THREADS;
  return (int)(n < VOX_STAT_GROUPS ? n : VOX_STAT_GROUPS);
}

// The workspace of a chunk of sc slices of C cells, packed: ctr | sums (n and sum per slice) | acc | part (the partials).  The
// counters, the sums and the accumulators are adjacent because one memset clears them.  Every block behind the counters is
// linear in sc: vox_carve(sc) - vox_carve(0) is sc times the bytes of one slice.
struct VoxWs {
  int32_t *ctr;
  long long *sums, *acc;
  double *part;
};
static size_t vox_carve(void *ws, int sc, long C, VoxWs *w) {
  WsCarver c(ws);
  w->ctr = c.take<int32_t>(VOX_CTR_WORDS, 1);
  w->sums = c.take<long long>(2 * (size_t)sc, 1);
  w->acc = c.take<long long>((size_t)sc * C, 1);
  w->part = c.take<double>((size_t)sc * vox_stat_groups(C), 1);
  return c.bytes();
}

extern "C" {
size_t ramp_event_voxel_workspace_bytes(int slices, int bins, int H, int W) {
  if (slices < 1 || bins < 1 || H < 1 || W < 1) return 0;
  VoxWs w;
  return vox_carve(nullptr, slices, (long)bins * H * W, &w);
}
long ramp_event_voxel_grid_events(void) { return (long)WARP_MAX_GROUPS * WARP_TILE; }
int ramp_event_voxel_lds_offsets(void) { return VOX_LDS_OFFSETS; }

int ramp_event_voxel(const float *x, const float *y, const double *t, const int8_t *p, long N, const int64_t *offsets, int S,
                     int bins, int H, int W, int flags, float *grid, double *stats, int32_t *status, void *ws, size_t ws_bytes,
                     void *stream) {
  if (N < 0 || S < 1 || bins < 1 || H < 1 || W < 1) return RAMP_EINVAL;
  if (flags & ~(RAMP_VOXEL_NORMALIZE | RAMP_VOXEL_SUBPIXEL)) return RAMP_EINVAL;
  if (!offsets && S != 1) return RAMP_EINVAL;
  if (!grid || !stats || !status || !ws) return RAMP_EINVAL;
  if (N > 0 && (!x || !y || !t || !p)) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)stats & 7) != 0 || ((uintptr_t)offsets & 7) != 0) return RAMP_EINVAL;
  if ((double)bins * (double)H * (double)W > 2147483647.0) return RAMP_EUNSUPPORTED;
  const long C = (long)bins * H * W;
  const int P = vox_stat_groups(C);
  VoxWs w;
  const size_t head = vox_carve(nullptr, 0, C, &w), one = vox_carve(nullptr, 1, C, &w);
  if (ws_bytes < one) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  size_t fit = (ws_bytes - head) / (one - head);
  if (fit > VOX_MAX_CHUNK) fit = VOX_MAX_CHUNK;
  const int chunk = (int)(fit < (size_t)S ? fit : (size_t)S);
  const long tiles = (N + WARP_TILE - 1) / WARP_TILE;
  const int vote_grid = (int)(tiles < WARP_MAX_GROUPS ? tiles : WARP_MAX_GROUPS);
  const bool vec = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)p | (uintptr_t)t) & 15) == 0;
  const bool sub = (flags & RAMP_VOXEL_SUBPIXEL) != 0;
  for (int c0 = 0; c0 < S; c0 += chunk) {
    const int sc = S - c0 < chunk ? S - c0 : chunk;
    vox_carve(ws, sc, C, &w);
    int32_t *ctr = w.ctr;
    long long *sums = w.sums, *acc = w.acc;
    double *part = w.part;
    const long long *off = offsets ? (const long long *)offsets + c0 : nullptr;
    // the one memset of the chunk: n and sum and the accumulators; in front of the first chunk the counters as well
    void *first = c0 ? (void *)sums : (void *)ctr;
    if (hipMemsetAsync(first, 0, ws_span(first, part), st) != hipSuccess) return RAMP_ELAUNCH;
    if (c0 == 0 && offsets) {
      hipLaunchKernelGGL(vox_offsets_kernel, dim3(ramp_cdiv((long)S + 1, INTERP_THREADS)), dim3(INTERP_THREADS), 0, st,
                         (const long long *)offsets, S, N, ctr);
      RAMP_CHECK_LAUNCH();
    }
    if (N > 0) {
      VoxArgs a;
      a.x = x; a.y = y; a.t = t; a.p = p; a.offsets = off; a.acc = acc; a.ctr = ctr; a.N = N; a.sc = sc; a.bins = bins;
      a.H = H; a.W = W;
      const int mode = !off ? 0 : (sc + 1 <= VOX_LDS_OFFSETS ? 1 : 2);
      const size_t lds = mode == 1 ? (size_t)(sc + 1) * sizeof(long long) : 0;
      static_assert((size_t)VOX_LDS_OFFSETS * sizeof(long long) + WARP_TILE * 17 <= 64 * 1024,
                    "LDS within the default limit: the launch needs no hipFuncSetAttribute");
      if (mode == 0) { if (sub) vox_launch_vote<0, true>(a, vec, vote_grid, lds, st); else vox_launch_vote<0, false>(a, vec, vote_grid, lds, st); }
      else if (mode == 1) { if (sub) vox_launch_vote<1, true>(a, vec, vote_grid, lds, st); else vox_launch_vote<1, false>(a, vec, vote_grid, lds, st); }
      else { if (sub) vox_launch_vote<2, true>(a, vec, vote_grid, lds, st); else vox_launch_vote<2, false>(a, vec, vote_grid, lds, st); }
      RAMP_CHECK_LAUNCH();
    }
    const dim3 groups((unsigned)sc * (unsigned)P);
    hipLaunchKernelGGL(vox_count_kernel, groups, dim3(INTERP_THREADS), 0, st, acc, off, t, N, C, P, sums, ctr);
    RAMP_CHECK_LAUNCH();
    hipLaunchKernelGGL(vox_spread_kernel, groups, dim3(INTERP_THREADS), 0, st, acc, C, P, sums, ctr, part);
    RAMP_CHECK_LAUNCH();
    hipLaunchKernelGGL(vox_finish_kernel, groups, dim3(INTERP_THREADS), 0, st, acc, off, t, N, C, P, sums, part, ctr,
                       (flags & RAMP_VOXEL_NORMALIZE) ? 1 : 0, c0 + sc >= S ? 1 : 0, grid + (size_t)c0 * C,
                       stats + 4 * (size_t)c0, status);
    RAMP_CHECK_LAUNCH();
  }
  return RAMP_OK;
}
}  // extern "C"
