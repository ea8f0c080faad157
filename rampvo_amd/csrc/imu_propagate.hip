// IMU propagation (include/ramp_hip.h: ramp_imu_propagate): from an anchor -- a knot's pose, its metric velocity, the
// alignment's s, g and gyro bias, all on the device -- forward through every IMU sample behind it: a pose, a velocity and a
// position per sample.  Row i needs P_i = e_1 o ... o e_i, the PREFIX products of the preintegration elements (imu_device.h: the
// arithmetic of imu.hip word for word, float64, no FMA contraction, J not carried: 11 words), so the hot path is a device-wide
// ORDERED scan over a non-commutative product.
//
// Levels, all aligned to sample 0 of the call:
//   chunk   64 samples, one per lane: an ordered inclusive scan by shuffles, off = 1, 2, 4, ..., 32: lane i takes
//           lane(i - off) o own; lanes before the head supply the identity, which is neutral to the bit
//   tile    64 chunks = 4,096 samples = one workgroup of 256 threads (4 waves, 16 chunks each): the 64 chunk totals are scanned
//           the same way by wave 0
//   chain   the tile totals, left to right: one wave loads 64 totals at a time, composes them in index order and stores the
//           inclusive products in place (2^20 samples: 256 compositions)
// so row i is  (chain[tile - 1] o scan(chunk totals of its tile)[chunk - 1]) o scan(elements of its chunk)[lane]: a function of
// samples 0 .. i and the arguments -- never of N, the grid or what lies behind -- and a call repeats its bits.
//
//   prop_check_kernel   order of tau -> RAMP_IMU_BAD_ORDER; the anchor -> RAMP_IMU_BAD_ANCHOR; tau[0] > t0 -> RAMP_IMU_NO_START;
//                       the sample count; the break index b (first row behind the anchor that a sample which is not finite or a
//                       gap above max_gap cuts off) by an integer atomicMin on a workspace word
//   prop_tile_kernel    per tile: the elements, the chunk scans, the chunk totals -> workspace; their scan, the tile total ->
//                       workspace
//   prop_chain_kernel   one wave: the tile totals -> their inclusive products, in place
//   prop_rows_kernel    per tile: the chunk prefixes into LDS, the elements AGAIN (recomputed, not stored), the chunk scans, the
//                       rows: state, poses, times_out; the four row counters (ramp_wave_count / ramp_wave_flush)
//   prop_status_kernel  the 8 status words
// ramp_imu_propagate enqueues one hipMemsetAsync (64 bytes of counters) and these five launches.  No floating-point atomics, no
// read back, no synchronisation.  The workspace holds the counters and 11 doubles per chunk and per tile.
#include "imu_device.h"

#define PROP_THREADS 256
#define PROP_WAVES (PROP_THREADS / RAMP_WAVE)
#define PROP_CHUNK RAMP_WAVE                       // samples per chunk
#define PROP_TILE_CHUNKS 64                        // chunks per tile
#define PROP_TILE (PROP_CHUNK * PROP_TILE_CHUNKS)  // samples per tile
#define PROP_CTR_WORDS 16                          // int32: [0..5] the status words, [8] the break index minus INT_MAX
#define PROP_BREAK 8
#define PROP_MAX_GROUPS 2048
#define PROP_W IMU_PROP_WORDS
#define PROP_NONE 2147483647

struct PropArgs {
  const double *tau;
  const void *gyro, *accel;                        // [N][3] float or double
  const double *anchor;                            // [24] on the device
  double *chunk_tot, *tile_tot;                    // workspace: [chunks][11], [tiles][11]
  int32_t *ctr;
  float *poses;
  double *times_out, *state;
  double q_bc[4], lever[3], p_bc[3], bias_a[3], max_gap, horizon;
  long N;
};

static __device__ __forceinline__ void prop_load(const double *src, ImuProp &e) {
  double *w = reinterpret_cast<double *>(&e);
#pragma unroll
  for (int c = 0; c < PROP_W; c++) w[c] = src[c];
}
static __device__ __forceinline__ void prop_store(double *dst, const ImuProp &e) {
  const double *w = reinterpret_cast<const double *>(&e);
#pragma unroll
  for (int c = 0; c < PROP_W; c++) dst[c] = w[c];
}

// lane `lane - off`'s element, or the identity in the lanes before the head
static __device__ __forceinline__ void prop_shfl_up(const ImuProp &e, int off, bool have, ImuProp &o) {
  const double *src = reinterpret_cast<const double *>(&e);
  double *dst = reinterpret_cast<double *>(&o);
  ImuProp id;
  imu_identity(id);
  const double *idw = reinterpret_cast<const double *>(&id);
#pragma unroll
  for (int c = 0; c < PROP_W; c++) {
    const double v = __shfl_up(src[c], off);
    dst[c] = have ? v : idw[c];
  }
}

// the ordered inclusive scan of a wave: afterwards lane i holds e_0 o e_1 o ... o e_i
static __device__ __forceinline__ void prop_wave_scan(ImuProp &e, int lane) {
#pragma unroll 1
  for (int off = 1; off < RAMP_WAVE; off <<= 1) {
    ImuProp o;
    prop_shfl_up(e, off, lane >= off, o);
    imu_compose(o, e);
    e = o;
  }
}

// e_i, the element on [u_i-1, u_i] with u = max(tau, t0): the identity for i == 0, for a row at or before the anchor and for a
// sub-interval of length 0; the measurement at t0 is interpolated between the two samples around it, as an interval's first
// sub-interval is in imu_integrate_kernel
template <typename S>
static __device__ __forceinline__ void prop_element(const PropArgs &a, long i, double t0, const double *bg, ImuProp &e) {
  imu_identity(e);
  if (i < 1 || i >= a.N) return;
  const double ta = a.tau[i - 1], tb = a.tau[i];
  if (!(tb > t0)) return;
  const S *__restrict__ gy = reinterpret_cast<const S *>(a.gyro);
  const S *__restrict__ ac = reinterpret_cast<const S *>(a.accel);
  const size_t i0 = (size_t)(i - 1);
  double g0[3], g1[3], f0[3], f1[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    g0[c] = (double)gy[3 * i0 + c]; g1[c] = (double)gy[3 * i0 + 3 + c];
    f0[c] = (double)ac[3 * i0 + c]; f1[c] = (double)ac[3 * i0 + 3 + c];
  }
  double u0 = ta;
  if (ta < t0) {
    u0 = t0;
    const double al = (t0 - ta) / (tb - ta);
#pragma unroll
    for (int c = 0; c < 3; c++) { g0[c] = g0[c] + al * (g1[c] - g0[c]); f0[c] = f0[c] + al * (f1[c] - f0[c]); }
  }
  const double dt = tb - u0;
  if (!(dt > 0.0)) return;
  double w[3], f[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { w[c] = 0.5 * (g0[c] + g1[c]) - bg[c]; f[c] = 0.5 * (f0[c] + f1[c]) - a.bias_a[c]; }
  imu_element(w, f, dt, e);
}

template <typename S>
static __device__ __forceinline__ bool prop_sample_finite(const PropArgs &a, long i) {
  const S *gy = reinterpret_cast<const S *>(a.gyro) + 3 * (size_t)i, *ac = reinterpret_cast<const S *>(a.accel) + 3 * (size_t)i;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) ok = ok && interp_finite((double)gy[c]) && interp_finite((double)ac[c]);
  return ok;
}

template <typename S>
__global__ void __launch_bounds__(PROP_THREADS) prop_check_kernel(const PropArgs a) {
  const int tid = threadIdx.x;
  const double *__restrict__ tau = a.tau;
  const long N = a.N;
  const double t0 = a.anchor[0];
  int n_seen = 0, n_bad = 0;                                       // wave-uniform: sums of ballots
  long b = PROP_NONE;
  for (long base = (long)blockIdx.x * PROP_THREADS; base < N; base += (long)gridDim.x * PROP_THREADS) {
    const long i = base + tid;
    bool bad = false;
    if (i < N) {
      const double t = tau[i];
      bad = !interp_finite(t) || (i + 1 < N && tau[i + 1] < t);
      if (i >= 1 && t > t0 && b == PROP_NONE &&
          (!prop_sample_finite<S>(a, i) || !prop_sample_finite<S>(a, i - 1) || (t - tau[i - 1]) > a.max_gap))
        b = i;
    }
    n_seen += ramp_wave_count(i < N);
    n_bad += ramp_wave_count(bad);
  }
  ramp_wave_flush(a.ctr + 1, tid, n_seen);
  if (n_bad && (tid & (RAMP_WAVE - 1)) == 0) atomicOr(a.ctr, RAMP_IMU_BAD_ORDER);
  if (b != PROP_NONE) atomicMin(a.ctr + PROP_BREAK, (int)(b - PROP_NONE));
  if (blockIdx.x == 0 && tid == 0) {
    bool ok = true;
    for (int c = 0; c < 18; c++) ok = ok && interp_finite(a.anchor[c]);
    int bits = 0;
    if (!ok || !(a.anchor[11] > 0.0)) bits |= RAMP_IMU_BAD_ANCHOR;
    if (tau[0] > t0) bits |= RAMP_IMU_NO_START;
    if (bits) atomicOr(a.ctr, bits);
  }
}

// the scan of the tile's 64 chunk totals by wave 0 (lane l: chunk l of the tile, the identity beyond the last chunk)
static __device__ __forceinline__ void prop_tile_scan(const double *tot, long first_chunk, long n_chunks, int lane, ImuProp &e) {
  imu_identity(e);
  if (first_chunk + lane < n_chunks) prop_load(tot + PROP_W * (size_t)(first_chunk + lane), e);
  prop_wave_scan(e, lane);
}

template <typename S>
__global__ void __launch_bounds__(PROP_THREADS) prop_tile_kernel(const PropArgs a) {
  if (a.ctr[0] != 0) return;                                       // a bit is set: nothing is walked
  const int tid = threadIdx.x, lane = tid & (RAMP_WAVE - 1), wave = tid / RAMP_WAVE;
  const long tile = blockIdx.x, n_chunks = (a.N + PROP_CHUNK - 1) / PROP_CHUNK;
  const double t0 = a.anchor[0];
  const double bg[3] = {a.anchor[15], a.anchor[16], a.anchor[17]};
#pragma unroll 1
  for (int k = wave; k < PROP_TILE_CHUNKS; k += PROP_WAVES) {
    const long chunk = tile * PROP_TILE_CHUNKS + k;                // wave-uniform
    if (chunk >= n_chunks) break;
    ImuProp e;
    prop_element<S>(a, chunk * PROP_CHUNK + lane, t0, bg, e);
    prop_wave_scan(e, lane);
    if (lane == RAMP_WAVE - 1) prop_store(a.chunk_tot + PROP_W * (size_t)chunk, e);
  }
  __threadfence_block();
  __syncthreads();
  if (wave == 0) {
    ImuProp e;
    prop_tile_scan(a.chunk_tot, tile * PROP_TILE_CHUNKS, n_chunks, lane, e);
    if (lane == RAMP_WAVE - 1) prop_store(a.tile_tot + PROP_W * (size_t)tile, e);
  }
}

// tile_tot[t] <- tile_tot[0] o ... o tile_tot[t], left to right: 64 totals are loaded at a time, one per lane, and every lane
// composes them in index order (the same words in every lane); lane k keeps the product that ends with its own
__global__ void __launch_bounds__(RAMP_WAVE) prop_chain_kernel(const PropArgs a, long n_tiles) {
  if (a.ctr[0] != 0) return;
  const int lane = threadIdx.x;
  ImuProp carry;
  imu_identity(carry);
  for (long base = 0; base < n_tiles; base += RAMP_WAVE) {
    ImuProp own, mine;
    imu_identity(own);
    if (base + lane < n_tiles) prop_load(a.tile_tot + PROP_W * (size_t)(base + lane), own);
    mine = own;
    const double *src = reinterpret_cast<const double *>(&own);
    const int n = n_tiles - base < RAMP_WAVE ? (int)(n_tiles - base) : RAMP_WAVE;
#pragma unroll 1
    for (int k = 0; k < n; k++) {
      ImuProp o;
      double *dst = reinterpret_cast<double *>(&o);
#pragma unroll
      for (int c = 0; c < PROP_W; c++) dst[c] = __shfl(src[c], k);
      imu_compose(carry, o);
      if (lane == k) mine = carry;
    }
    if (base + lane < n_tiles) prop_store(a.tile_tot + PROP_W * (size_t)(base + lane), mine);
  }
}

template <typename S>
__global__ void __launch_bounds__(PROP_THREADS) prop_rows_kernel(const PropArgs a) {
  __shared__ double s_pre[PROP_TILE_CHUNKS * PROP_W];              // the product in front of each chunk of the tile
  const int tid = threadIdx.x, lane = tid & (RAMP_WAVE - 1), wave = tid / RAMP_WAVE;
  const long tile = blockIdx.x, N = a.N, n_chunks = (N + PROP_CHUNK - 1) / PROP_CHUNK;
  const bool failed = a.ctr[0] != 0;
  const long brk = (long)a.ctr[PROP_BREAK] + PROP_NONE;
  const double t0 = a.anchor[0];
  const double nan = imu_nan();
  if (!failed && wave == 0) {
    ImuProp e, pre, left;
    prop_tile_scan(a.chunk_tot, tile * PROP_TILE_CHUNKS, n_chunks, lane, e);
    prop_shfl_up(e, 1, lane >= 1, left);                           // the chunks of this tile in front of chunk `lane`
    imu_identity(pre);
    if (tile > 0) prop_load(a.tile_tot + PROP_W * (size_t)(tile - 1), pre);
    imu_compose(pre, left);
    prop_store(s_pre + PROP_W * lane, pre);
  }
  __syncthreads();
  // the anchor: R0 = R_wc0 R_bc^T, p0 = s pbar0 - R0 p_bc (= s pbar0 + R_wc0 (-R_bc^T p_bc)), as imu.hip forms a knot's body
  double q0[4], p0[3], v0[3], g[3], bg[3];
  const double s = a.anchor[11];
  {
    double q[4] = {a.anchor[4], a.anchor[5], a.anchor[6], a.anchor[7]}, c0[3];
    imu_qnorm(q);
    const double qi[4] = {-a.q_bc[0], -a.q_bc[1], -a.q_bc[2], a.q_bc[3]};
    imu_qmul(q, qi, q0);
    imu_qrot(q, 1.0, a.lever, c0);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      p0[c] = s * a.anchor[1 + c] + c0[c];
      v0[c] = a.anchor[8 + c]; g[c] = a.anchor[12 + c]; bg[c] = a.anchor[15 + c];
    }
  }
  int n_held = 0, n_ok = 0, n_cut = 0, n_far = 0;                  // wave-uniform
#pragma unroll 1
  for (int k = wave; k < PROP_TILE_CHUNKS; k += PROP_WAVES) {
    const long chunk = tile * PROP_TILE_CHUNKS + k;
    if (chunk >= n_chunks) break;
    const long i = chunk * PROP_CHUNK + lane;
    const bool have = i < N;
    if (failed) {
      if (have) {
        for (int c = 0; c < 7; c++) a.poses[7 * (size_t)i + c] = __double2float_rn(nan);
        if (a.times_out) a.times_out[i] = nan;
        if (a.state)
          for (int c = 0; c < 16; c++) a.state[16 * (size_t)i + c] = nan;
      }
      continue;
    }
    ImuProp e, P;
    prop_element<S>(a, i, t0, bg, e);
    prop_wave_scan(e, lane);
    prop_load(s_pre + PROP_W * k, P);
    imu_compose(P, e);
    const double ti = have ? a.tau[i] : 0.0;
    const bool held = have && !(ti > t0), cut = have && !held && i >= brk;
    const bool far = have && !held && !cut && P.t > a.horizon;
    n_held += ramp_wave_count(held);
    n_cut += ramp_wave_count(cut);
    n_far += ramp_wave_count(far);
    n_ok += ramp_wave_count(have && !held && !cut && !far);
    if (!have) continue;
    // R_wb = R0 dR,  v = (v0 + g dt) + R0 dv,  p_wb = ((p0 + v0 dt) + 1/2 g dt^2) + R0 dp
    double qwb[4], rv[3], rp[3], v[3], p[3], pc[3], qwc[4], lv[3];
    const double dt = P.t;
    imu_qmul(q0, P.q, qwb);
    imu_qnorm(qwb);
    imu_qrot(q0, 1.0, P.v, rv);
    imu_qrot(q0, 1.0, P.p, rp);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      v[c] = (v0[c] + g[c] * dt) + rv[c];
      p[c] = ((p0[c] + v0[c] * dt) + 0.5 * g[c] * (dt * dt)) + rp[c];
    }
    // the camera: translation (p_wb + R_wb p_bc) / s, rotation q_wb (x) q_bc normalised, each rounded to fp32 once
    imu_qrot(qwb, 1.0, a.p_bc, lv);
#pragma unroll
    for (int c = 0; c < 3; c++) pc[c] = (p[c] + lv[c]) / s;
    imu_qmul(qwb, a.q_bc, qwc);
    imu_qnorm(qwc);
    const bool dead = cut || far;
    float *row = a.poses + 7 * (size_t)i;
#pragma unroll
    for (int c = 0; c < 3; c++) row[c] = __double2float_rn(dead ? nan : pc[c]);
#pragma unroll
    for (int c = 0; c < 4; c++) row[3 + c] = __double2float_rn(dead ? nan : qwc[c]);
    if (a.times_out) a.times_out[i] = held ? t0 : ti;
    if (a.state) {
      double *st = a.state + 16 * (size_t)i;
      st[0] = dead ? nan : dt;
#pragma unroll
      for (int c = 0; c < 4; c++) st[1 + c] = dead ? nan : qwb[c];
#pragma unroll
      for (int c = 0; c < 3; c++) { st[5 + c] = dead ? nan : v[c]; st[8 + c] = dead ? nan : p[c]; }
#pragma unroll
      for (int c = 11; c < 16; c++) st[c] = dead ? nan : 0.0;
    }
  }
  ramp_wave_flush(a.ctr + 2, tid, n_held, n_ok, n_cut, n_far);
}

__global__ void __launch_bounds__(RAMP_WAVE) prop_status_kernel(const int32_t *__restrict__ ctr, int32_t *__restrict__ status) {
  const int tid = threadIdx.x;
  if (tid < 8) status[tid] = tid < 6 ? ctr[tid] : 0;
}

// the workspace for N samples, packed: ctr | chunk_tot | tile_tot; `tiles` is also the grid of the tile launches
struct PropWs {
  int32_t *ctr;
  double *chunk_tot, *tile_tot;
  long tiles;
};
static size_t prop_carve(void *ws, long N, PropWs *w) {
  const long chunks = (N + PROP_CHUNK - 1) / PROP_CHUNK;
  w->tiles = (N + PROP_TILE - 1) / PROP_TILE;
  WsCarver c(ws);
  w->ctr = c.take<int32_t>(PROP_CTR_WORDS, 1);
  w->chunk_tot = c.take<double>((size_t)chunks * PROP_W, 1);
  w->tile_tot = c.take<double>((size_t)w->tiles * PROP_W, 1);
  return c.bytes();
}

extern "C" {
size_t ramp_imu_propagate_workspace_bytes(long N) {
  if (N < 1) return 0;
  PropWs w;
  return prop_carve(nullptr, N, &w);
}

int ramp_imu_propagate(const double *tau, const void *gyro, const void *accel, long N, const double *anchor,
                       const double *extrinsics, const double *bias_a, double max_gap, double horizon, int flags, float *poses,
                       double *times_out, double *state, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
  if (!tau || !gyro || !accel || !anchor || !poses || !status || !ws) return RAMP_EINVAL;
  if (N < 1 || N > 2147483647l || (flags & ~RAMP_IMU_F64)) return RAMP_EINVAL;
  if (!(max_gap > 0.0) || !(horizon > 0.0)) return RAMP_EINVAL;
  if ((((uintptr_t)tau | (uintptr_t)anchor | (uintptr_t)times_out | (uintptr_t)state) & 7) != 0) return RAMP_EINVAL;
  if ((((uintptr_t)gyro | (uintptr_t)accel) & ((flags & RAMP_IMU_F64) ? 7 : 3)) != 0) return RAMP_EINVAL;
  if ((((uintptr_t)poses | (uintptr_t)status) & 3) != 0 || ((uintptr_t)ws & 15) != 0) return RAMP_EINVAL;
  for (int c = 0; c < 3; c++)
    if (bias_a && !imu_host_finite(bias_a[c])) return RAMP_EINVAL;
  PropArgs a;
  if (!imu_extrinsics(extrinsics, a.q_bc, a.lever, a.p_bc)) return RAMP_EINVAL;
  PropWs w;
  if (ws_bytes < prop_carve(ws, N, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long tiles = w.tiles;
  a.tau = tau; a.gyro = gyro; a.accel = accel; a.anchor = anchor;
  a.ctr = w.ctr; a.chunk_tot = w.chunk_tot; a.tile_tot = w.tile_tot;
  a.poses = poses; a.times_out = times_out; a.state = state;
  for (int c = 0; c < 3; c++) a.bias_a[c] = bias_a ? bias_a[c] : 0.0;
  a.max_gap = max_gap; a.horizon = horizon; a.N = N;
  const bool f64 = (flags & RAMP_IMU_F64) != 0;
  const int check_grid = ramp_cdiv(N, PROP_THREADS) < PROP_MAX_GROUPS ? ramp_cdiv(N, PROP_THREADS) : PROP_MAX_GROUPS;
  const dim3 grid((unsigned)tiles), block(PROP_THREADS);

  // the one memset: the counters (the break word reads "none" at zero)
  if (hipMemsetAsync(a.ctr, 0, ws_span(a.ctr, a.chunk_tot), st) != hipSuccess) return RAMP_ELAUNCH;
  if (f64) hipLaunchKernelGGL(prop_check_kernel<double>, dim3(check_grid), block, 0, st, a);
  else hipLaunchKernelGGL(prop_check_kernel<float>, dim3(check_grid), block, 0, st, a);
  RAMP_CHECK_LAUNCH();
  if (f64) hipLaunchKernelGGL(prop_tile_kernel<double>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(prop_tile_kernel<float>, grid, block, 0, st, a);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(prop_chain_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, a, tiles);
  RAMP_CHECK_LAUNCH();
  if (f64) hipLaunchKernelGGL(prop_rows_kernel<double>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(prop_rows_kernel<float>, grid, block, 0, st, a);
  RAMP_CHECK_LAUNCH();
  hipLaunchKernelGGL(prop_status_kernel, dim3(1), dim3(RAMP_WAVE), 0, st, (const int32_t *)a.ctr, status);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}
}  // extern "C"
