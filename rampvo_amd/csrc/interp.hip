// Continuous-time pose queries: the SE(3) geodesic between the knots of a trajectory, at any time stamp
// (include/ramp_hip.h: ramp_se3_interp).
//
//   s     = largest index with times[s] <= t, clamped to [0, T - 2]
//   alpha = (t - times[s]) / (times[s + 1] - times[s])           float64, rounded to fp32 once
//   xi_s  = Log(X[s + 1] * X[s]^-1)                               the left increment, (translation 3, rotation 3)
//   X(t)  = Exp(alpha * xi_s) * X[s]
//
// Two launches: interp_segment_kernel (one lane per segment: xi_s, the segment's twist and length, the check of `times`)
// and interp_query_kernel (one lane per query, the hot path: search, one fp64 subtraction and division, lt_exp, lt_mul, a
// 28-byte row and an optional 24-byte twist).  Every row is a function of its own query alone -- the lt_* device functions
// of ramp_se3_exp / ramp_se3_mul in program order, no reduction over queries -- and the counters are integers, so a row's
// bits depend neither on Q, nor on the row's position, nor on the order of the queries, nor on the launch shape.
#include "interp_device.h"

__global__ void __launch_bounds__(INTERP_THREADS)
    interp_segment_kernel(const float *__restrict__ knots, const double *__restrict__ times, int T, float *__restrict__ seg,
                          int32_t *status) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int S = T > 1 ? T - 1 : 1;                 // (T == 1: one segment of zero length and zero motion)
  if (s >= S) return;
  if (interp_segment_row(knots, times, T, s, seg + (size_t)s * INTERP_SEG_WORDS)) atomicOr(status, RAMP_INTERP_BAD_TIMES);
}

// LDS_TIMES: the knot times are staged in LDS once per workgroup (T <= INTERP_LDS_KNOTS), else every search step is a global
// load.  LDS_ROWS: a tile's rows go through LDS and leave as full-width contiguous stores instead of one 28-byte (24-byte)
// strided row per lane.
template <bool LDS_TIMES, bool LDS_ROWS>
__global__ void __launch_bounds__(INTERP_THREADS)
    interp_query_kernel(const float *__restrict__ knots, const double *__restrict__ times, int T,
                        const double *__restrict__ query, int Q, int extrapolate, const float *__restrict__ seg,
                        float *__restrict__ out, float *__restrict__ twist, int32_t *status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char interp_smem[];
  __shared__ int s_cnt[3];
  double *s_times = reinterpret_cast<double *>(interp_smem);
  float *s_rows = reinterpret_cast<float *>(interp_smem + (LDS_TIMES ? (size_t)T * sizeof(double) : 0));
  float *s_twist = s_rows + INTERP_THREADS * 7;
  const int tid = threadIdx.x;
  if (LDS_TIMES)
    for (int i = tid; i < T; i += INTERP_THREADS) s_times[i] = times[i];
  if (tid < 3) s_cnt[tid] = 0;
  __syncthreads();
  const bool failed = (status[0] & RAMP_INTERP_BAD_TIMES) != 0;    // (raised by the segment launch in front of this one)
  const double t_first = times[0], t_last = times[T - 1];
  const int s_max = T > 1 ? T - 2 : 0;
  const float qnan = __int_as_float(0x7fc00000);
  const int tiles = (int)(((long)Q + INTERP_THREADS - 1) / INTERP_THREADS);
  int n_below = 0, n_above = 0, n_nan = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long base = (long)tile * INTERP_THREADS;
    const long qi = base + tid;
    float o[7] = {0, 0, 0, 0, 0, 0, 0}, tw[6] = {0, 0, 0, 0, 0, 0};
    if (qi < Q) {
      const double t = query[qi];
      if (t != t) {
        n_nan++;
#pragma unroll
        for (int c = 0; c < 7; c++) o[c] = qnan;
#pragma unroll
        for (int c = 0; c < 6; c++) tw[c] = qnan;
      } else {
        n_below += t < t_first;
        n_above += t > t_last;
        int s;
        double ts;
        if (LDS_TIMES) {
          s = min(max(interp_upper_bound(s_times, T, t) - 1, 0), s_max);
          ts = s_times[s];
        } else {
          s = min(max(interp_upper_bound(times, T, t) - 1, 0), s_max);
          ts = times[s];
        }
        const float4 *row4 = reinterpret_cast<const float4 *>(seg + (size_t)s * INTERP_SEG_WORDS);
        const float4 r0 = row4[0], r1 = row4[1];      // xi[0..3]; xi[4], xi[5], the length
        const float xi[6] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y};
        const double dt = __hiloint2double(__float_as_int(r1.w), __float_as_int(r1.z));
        const float alpha = interp_alpha(t, ts, dt, extrapolate);
        float X[7], axi[6], E[7];
#pragma unroll
        for (int c = 0; c < 7; c++) X[c] = knots[7 * (size_t)s + c];
#pragma unroll
        for (int c = 0; c < 6; c++) axi[c] = alpha * xi[c];
        if (twist) {
          const float4 r2 = row4[2], r3 = row4[3];
          tw[0] = r2.x; tw[1] = r2.y; tw[2] = r2.z; tw[3] = r2.w; tw[4] = r3.x; tw[5] = r3.y;
        }
        lt_exp(axi, E);
        lt_mul(E, X, o);
        if (failed) {
#pragma unroll
          for (int c = 0; c < 7; c++) o[c] = qnan;
#pragma unroll
          for (int c = 0; c < 6; c++) tw[c] = qnan;
        }
      }
    }
    if (LDS_ROWS) {
      const int live = (int)min((long)INTERP_THREADS, (long)Q - base);   // rows of this tile, >= 1
      if (tid < live) {
#pragma unroll
        for (int c = 0; c < 7; c++) s_rows[tid * 7 + c] = o[c];
        if (twist) {
#pragma unroll
          for (int c = 0; c < 6; c++) s_twist[tid * 6 + c] = tw[c];
        }
      }
      __syncthreads();
      float *og = out + (size_t)base * 7;
      for (int i = tid; i < live * 7; i += INTERP_THREADS) og[i] = s_rows[i];
      if (twist) {
        float *tg = twist + (size_t)base * 6;
        for (int i = tid; i < live * 6; i += INTERP_THREADS) tg[i] = s_twist[i];
      }
      __syncthreads();                               // (the next tile overwrites the staging rows)
    } else if (qi < Q) {
#pragma unroll
      for (int c = 0; c < 7; c++) out[(size_t)qi * 7 + c] = o[c];
      if (twist) {
#pragma unroll
        for (int c = 0; c < 6; c++) twist[(size_t)qi * 6 + c] = tw[c];
      }
    }
  }
  // counters: per lane over its tiles, per workgroup in LDS, then one integer atomic per workgroup and counter
  if (n_below) atomicAdd(&s_cnt[0], n_below);
  if (n_above) atomicAdd(&s_cnt[1], n_above);
  if (n_nan) atomicAdd(&s_cnt[2], n_nan);
  __syncthreads();
  if (tid < 3 && s_cnt[tid]) atomicAdd(&status[1 + tid], s_cnt[tid]);
}

template <bool LDS_TIMES, bool LDS_ROWS>
static int interp_launch_query(const float *knots, const double *times, int T, const double *query, int Q, int extrapolate,
                               const float *seg, float *out, float *twist, int32_t *status, hipStream_t st) {
  const int tiles = ramp_cdiv(Q, INTERP_THREADS);
  const int grid = tiles < INTERP_MAX_GROUPS ? tiles : INTERP_MAX_GROUPS;
  const size_t lds = (LDS_TIMES ? (size_t)T * sizeof(double) : 0) + (LDS_ROWS ? (size_t)INTERP_THREADS * 13 * sizeof(float) : 0);
  static_assert((size_t)INTERP_LDS_KNOTS * sizeof(double) + INTERP_THREADS * 13 * sizeof(float) <= 64 * 1024,
                "dynamic LDS within the default limit: the launch needs no hipFuncSetAttribute");
  hipLaunchKernelGGL((interp_query_kernel<LDS_TIMES, LDS_ROWS>), dim3(grid), dim3(INTERP_THREADS), lds, st, knots, times, T,
                     query, Q, extrapolate, seg, out, twist, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

extern "C" {
size_t ramp_se3_interp_workspace_bytes(int T) {
  float *seg;
  return interp_carve(nullptr, T, &seg);
}
int ramp_se3_interp_lds_knots(void) { return INTERP_LDS_KNOTS; }

int ramp_se3_interp(const float *knots, const double *times, int T, const double *query, int Q, int flags, float *out,
                    float *twist, void *seg_ws, size_t seg_ws_bytes, int32_t *status, void *stream) {
  if (T < 1 || Q < 0) return RAMP_EINVAL;
  if (Q == 0) return RAMP_OK;
  if (!knots || !times || !query || !out || !seg_ws || !status) return RAMP_EINVAL;
  if (flags & ~(RAMP_INTERP_EXTRAPOLATE | RAMP_INTERP_ROW_STORES)) return RAMP_EINVAL;
  if (((uintptr_t)seg_ws & 15) != 0) return RAMP_EINVAL;
  float *seg;
  if (seg_ws_bytes < interp_carve(seg_ws, T, &seg)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  const int S = T > 1 ? T - 1 : 1;
  hipLaunchKernelGGL(interp_segment_kernel, dim3(ramp_cdiv(S, INTERP_THREADS)), dim3(INTERP_THREADS), 0, st, knots, times,
                     T, seg, status);
  RAMP_CHECK_LAUNCH();
  const int ex = (flags & RAMP_INTERP_EXTRAPOLATE) ? 1 : 0;
  const bool lds_times = T <= INTERP_LDS_KNOTS, lds_rows = !(flags & RAMP_INTERP_ROW_STORES);
  if (lds_times)
    return lds_rows ? interp_launch_query<true, true>(knots, times, T, query, Q, ex, seg, out, twist, status, st)
                    : interp_launch_query<true, false>(knots, times, T, query, Q, ex, seg, out, twist, status, st);
  return lds_rows ? interp_launch_query<false, true>(knots, times, T, query, Q, ex, seg, out, twist, status, st)
                  : interp_launch_query<false, false>(knots, times, T, query, Q, ex, seg, out, twist, status, st);
}
}  // extern "C"
