// Inverse-depth map from the window's patches (include/ramp_hip.h: ramp_invdepth_map): the selected patches are projected into
// one camera pose and regressed to a dense [H][W] map of inverse depth with a compactly supported kernel.
//
//   project  one lane per slot of the selection: G = cam^-1 * T_i^-1, X' = R_G r + t_G d, the record (u, v, d', c); a
//            rejected patch leaves a record of weight exactly 0 and is counted once
//   regress  one workgroup per DM_TILE_W x DM_TILE_H pixels, DM_PIX pixels per lane (the same column, DM_TILE_H / DM_PIX rows
//            apart: dx is shared).  The records pass through LDS in chunks of DM_STAGE: every wave culls its quarter of the
//            chunk against the tile's box grown by the radius (ballot + ordered prefix, so the survivors keep the selection's
//            order) and all lanes then read the survivors as 16-byte broadcasts.
//
// Two launches behind one 32-byte memset of the status words, which are also the counters.  No float atomics: a pixel's two
// sums are formed by one lane, over the records in selection order, in plain fp32 without FMA.  A culled record would have
// contributed w = 0 exactly (see dm_cull_margin) and every term is >= 0, so leaving it out changes no bit: a pixel's value
// depends neither on the tile shape nor on the chunking, and a call repeats its bits.
#include "ramp_device.h"
#include "workspace.h"

#define DM_THREADS 256
#define DM_TILE_W 32
#define DM_TILE_H 16
#define DM_PIX 2                          // pixels per lane
#define DM_WAVES (DM_THREADS / RAMP_WAVE)
#define DM_STAGE 1024                     // records per LDS chunk: 16 KiB
#define DM_WAVE_STAGE (DM_STAGE / DM_WAVES)
#define DM_HDR_WORDS 4                    // workspace header: [0] the live record count, 3 spare = 16 bytes
static_assert(DM_TILE_W * DM_TILE_H == DM_THREADS * DM_PIX && DM_TILE_H % DM_PIX == 0, "tile = lanes x pixels per lane");
static_assert(DM_WAVE_STAGE % RAMP_WAVE == 0, "a wave stages whole steps");

static __device__ __forceinline__ bool dm_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

// The cull keeps a record when its centre lies within the tile's pixel box grown by R + margin.  A record outside has
// |x - u| (or |y - v|) >= R + margin for every pixel of the tile, and the margin covers the rounding of the box test itself
// (|coordinates| <= W + H + 2R, each rounded to 2^-24 relative) and of s = 1 - r2 * (1 / R^2) (a handful of 2^-24 relative
// steps) a thousand times over: such a record's s is <= 0 in fp32, max(s, 0) = 0 and w = c * 0 = 0 for a finite c.
static __device__ __forceinline__ float dm_cull_margin(float R, int H, int W) { return 0.001f * (R + (float)(H + W)); }

struct DmProject {
  const float *poses, *patches, *intrinsics, *cam, *conf;
  const int32_t *index, *count, *dyn_rows;
  float4 *rec;                            // the workspace's records [K]
  int32_t *hdr, *status;
  float *records;                         // the caller's copy [K][4], or NULL
  float scale, R;
  int n, K, M, PP, ctr, per_row, last_rows, conf_is_variance, H, W;
};

__global__ void __launch_bounds__(DM_THREADS) dm_project_kernel(const DmProject a) {
  const int tid = threadIdx.x;
  const int j = blockIdx.x * DM_THREADS + tid;
  // the sizes that live on the device: the same few scalar loads in every lane
  int n_eff = a.n;
  if (a.dyn_rows) n_eff = (int)min((long long)a.n, (long long)max(*a.dyn_rows, 0) * a.per_row);
  int lo = 0, m;
  if (a.index) {
    m = a.count ? min(max(*a.count, 0), a.K) : a.K;
  } else {
    if (a.last_rows > 0) lo = (int)max((long long)n_eff - (long long)a.last_rows * a.per_row, 0ll);
    m = n_eff - lo;                       // (<= K: K is n, or min(n, last_rows * per_row))
  }
  float cam[7];
  bool bad_cam = false;
#pragma unroll
  for (int c = 0; c < 7; c++) {
    cam[c] = a.cam[c];
    bad_cam = bad_cam || !dm_finite(cam[c]);
  }
  if (j == 0) {
    a.hdr[0] = m;
    if (bad_cam) atomicOr(a.status, RAMP_DEPTHMAP_BAD_CAM);
  }
  const float qnan = __int_as_float(0x7fc00000);
  bool r_depth = false, r_z = false, r_reach = false, r_in = false;
  const bool live = j < m;
  if (j < a.K) {
    float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);          // (slots behind the live count: zero rows)
    if (live) {
      const int k = a.index ? a.index[j] : lo + j;
      float d = qnan, c = 1.0f;
      const bool id_ok = k >= 0 && k < n_eff;                   // (an id outside the patches has no depth)
      if (id_ok) {
        d = a.patches[((size_t)k * 3 + 2) * a.PP + a.ctr];
        if (a.conf) c = a.conf_is_variance ? 1.0f / a.conf[k] : a.conf[k];
      }
      rec = make_float4(qnan, qnan, qnan, 0.0f);
      if (!(id_ok && dm_finite(d) && d > 0.0f && dm_finite(c) && c > 0.0f)) {
        r_depth = true;
      } else {
        const float fx = a.intrinsics[0], fy = a.intrinsics[1], cx = a.intrinsics[2], cy = a.intrinsics[3];
        const float x = a.patches[((size_t)k * 3 + 0) * a.PP + a.ctr], y = a.patches[((size_t)k * 3 + 1) * a.PP + a.ctr];
        float Ti[7], Tinv[7], Cinv[7], G[7], Rr[3];
        const float *Tp = a.poses + 7 * (size_t)(k / a.M);
#pragma unroll
        for (int e = 0; e < 7; e++) Ti[e] = Tp[e];
        lt_inv(Ti, Tinv);
        lt_inv(cam, Cinv);
        lt_mul(Cinv, Tinv, G);                                  // G = cam^-1 * T_i^-1
        const float r[3] = {(x - cx) / fx, (y - cy) / fy, 1.0f};
        lt_qrot(G + 3, r, Rr);
        const float Xp = Rr[0] + G[0] * d, Yp = Rr[1] + G[1] * d, Zp = Rr[2] + G[2] * d;
        const float u = a.scale * (fx * (Xp / Zp) + cx), v = a.scale * (fy * (Yp / Zp) + cy);
        const float dp = d / Zp;
        if (bad_cam || !(Zp > RAMP_WARP_MIN_Z) || !dm_finite(u) || !dm_finite(v) || !dm_finite(dp)) {
          r_z = true;                                           // (a NaN Z' fails the comparison)
        } else if (u < -a.R || u > (float)(a.W - 1) + a.R || v < -a.R || v > (float)(a.H - 1) + a.R) {
          r_reach = true;
          rec = make_float4(u, v, dp, 0.0f);
        } else {
          r_in = true;
          rec = make_float4(u, v, dp, c);
        }
      }
      if (bad_cam) rec = make_float4(qnan, qnan, qnan, qnan);
    }
    a.rec[j] = rec;
    if (a.records) {
      float *o = a.records + 4 * (size_t)j;
      o[0] = rec.x; o[1] = rec.y; o[2] = rec.z; o[3] = rec.w;
    }
  }
  // every lane of the wave is here: one ballot per counter
  const int n_live = ramp_wave_count(live), n_depth = ramp_wave_count(r_depth), n_z = ramp_wave_count(r_z);
  const int n_reach = ramp_wave_count(r_reach), n_in = ramp_wave_count(r_in);
  ramp_wave_flush(a.status + 1, tid, n_live, n_depth, n_z, n_reach, n_in);
}

__global__ void __launch_bounds__(DM_THREADS)
    dm_regress_kernel(const float4 *__restrict__ rec, const int32_t *__restrict__ hdr, const float *__restrict__ prior,
                      float prior_weight, int prior_relative, float R, int H, int W, float *__restrict__ invdepth,
                      float *__restrict__ weight, int32_t *status) {
  __shared__ __attribute__((aligned(16))) float4 s_rec[DM_WAVES][DM_WAVE_STAGE];
  __shared__ int s_cnt[DM_WAVES];
  const int tid = threadIdx.x, lane = tid & (RAMP_WAVE - 1), wave = tid / RAMP_WAVE;
  const bool bad = (status[0] & RAMP_DEPTHMAP_BAD_CAM) != 0;   // (raised by the project launch in front)
  const int m = bad ? 0 : hdr[0];
  const int x0 = blockIdx.x * DM_TILE_W, y0 = blockIdx.y * DM_TILE_H;
  const int ix = x0 + (tid % DM_TILE_W), iy = y0 + tid / DM_TILE_W;
  const float px = (float)ix;
  float py[DM_PIX], S0[DM_PIX], S1[DM_PIX];
#pragma unroll
  for (int p = 0; p < DM_PIX; p++) {
    py[p] = (float)(iy + p * (DM_TILE_H / DM_PIX));
    S0[p] = 0.0f;
    S1[p] = 0.0f;
  }
  const float grow = R + dm_cull_margin(R, H, W);
  const float bx0 = (float)x0 - grow, bx1 = (float)(x0 + DM_TILE_W - 1) + grow;
  const float by0 = (float)y0 - grow, by1 = (float)(y0 + DM_TILE_H - 1) + grow;
  const float inv_r2 = 1.0f / (R * R);
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int base = 0; base < m; base += DM_STAGE) {             // (m is the same in every lane: the barriers are uniform)
    __syncthreads();                                           // the previous chunk has been read
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < DM_WAVE_STAGE / RAMP_WAVE; s++) {
      const int j = base + wave * DM_WAVE_STAGE + s * RAMP_WAVE + lane;
      const float4 r = j < m ? rec[j] : zero;
      const bool keep = r.w > 0.0f && r.x >= bx0 && r.x <= bx1 && r.y >= by0 && r.y <= by1;
      const unsigned long long mk = __ballot(keep);
      if (keep) s_rec[wave][cnt + __popcll(mk & ((1ull << lane) - 1ull))] = r;
      cnt += __popcll(mk);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    for (int w = 0; w < DM_WAVES; w++) {
      const int c = s_cnt[w];
      for (int i = 0; i < c; i++) {
        const float4 r = s_rec[w][i];                          // one 16-byte broadcast
        const float dx = px - r.x;
        const float dx2 = dx * dx;
#pragma unroll
        for (int p = 0; p < DM_PIX; p++) {
          const float dy = py[p] - r.y;
          const float r2 = dx2 + dy * dy;
          const float t = fmaxf(1.0f - r2 * inv_r2, 0.0f);
          const float wk = r.w * (t * t);
          S0[p] += wk;
          S1[p] += wk * r.z;
        }
      }
    }
  }
  const float qnan = __int_as_float(0x7fc00000);
  float pr = 0.0f, pw = 0.0f;
  if (prior_weight != 0.0f) {
    pr = prior[0];
    pw = prior_relative ? prior_weight / (pr * pr) : prior_weight;
  }
  const bool pw_ok = pw > 0.0f && dm_finite(pw);
  int empty = 0;
#pragma unroll
  for (int p = 0; p < DM_PIX; p++) {
    const int y = iy + p * (DM_TILE_H / DM_PIX);
    if (ix < W && y < H) {
      // no data: the prior itself (not pw * prior / pw, which may round), or NaN without one
      float v = S0[p] == 0.0f ? (pw_ok ? pr : qnan) : (pw * pr + S1[p]) / (pw + S0[p]);
      if (pw != 0.0f && !pw_ok) v = qnan;                      // (a prior weight that is not finite: never a plausible number)
      const size_t at = (size_t)y * W + ix;
      if (invdepth) invdepth[at] = bad ? qnan : v;
      if (weight) weight[at] = bad ? qnan : S0[p];
      empty += S0[p] == 0.0f ? 1 : 0;
    }
  }
  empty = ramp_wave_sum(empty);
  if (lane == 0 && empty) atomicAdd(&status[6], empty);
}

static int dm_record_capacity(int n, int K, bool has_index, int per_row, int last_rows) {
  if (has_index) return K;
  if (last_rows > 0) return (int)((long long)last_rows * per_row < (long long)n ? (long long)last_rows * per_row : (long long)n);
  return n;
}

// the workspace for K records, packed: the header words | the records
struct DmWs {
  int32_t *hdr;
  float4 *rec;
};
static size_t dm_carve(void *ws, int K, DmWs *w) {
  WsCarver c(ws);
  w->hdr = c.take<int32_t>(DM_HDR_WORDS, 1);
  w->rec = c.take<float4>((size_t)(K > 0 ? K : 0), 1);
  return c.bytes();
}

extern "C" {
int ramp_invdepth_map_stage_records(void) { return DM_STAGE; }

size_t ramp_invdepth_map_workspace_bytes(int K) {
  DmWs w;
  return dm_carve(nullptr, K, &w);
}

int ramp_invdepth_map(const float *poses, const float *patches, const float *intrinsics, const float *cam, int n, int M, int P,
                      float scale, const int32_t *index, const int32_t *count, int K, const int32_t *dyn_rows, int per_row,
                      int last_rows, const float *conf, const float *prior, float prior_weight, float radius, int flags, int H,
                      int W, float *invdepth, float *weight, float *records, void *ws, size_t ws_bytes, int32_t *status,
                      void *stream) {
  if (H < 1 || W < 1 || n < 0 || M < 1 || P < 1 || per_row < 0 || last_rows < 0) return RAMP_EINVAL;
  if (!(radius > 0.0f) || !(radius <= 3.4028234663852886e38f)) return RAMP_EINVAL;
  if (!(prior_weight >= 0.0f) || !(prior_weight <= 3.4028234663852886e38f)) return RAMP_EINVAL;
  if (!(scale > 0.0f) || !(scale <= 3.4028234663852886e38f)) return RAMP_EINVAL;
  if (!invdepth && !weight && !records) return RAMP_EINVAL;
  if (flags & ~(RAMP_DEPTHMAP_CONF_IS_VARIANCE | RAMP_DEPTHMAP_PRIOR_RELATIVE)) return RAMP_EINVAL;
  if (!intrinsics || !cam || !ws || !status || (n > 0 && (!poses || !patches))) return RAMP_EINVAL;
  if ((index && K < 0) || (!index && count) || (!index && last_rows > 0 && per_row < 1)) return RAMP_EINVAL;
  if (prior_weight > 0.0f && !prior) return RAMP_EINVAL;
  if (((uintptr_t)ws & 15) != 0) return RAMP_EINVAL;
  if (ramp_cdiv(H, DM_TILE_H) > 65535) return RAMP_EUNSUPPORTED;           // (the tile rows are the grid's y)
  const int Kc = dm_record_capacity(n, K, index != nullptr, per_row, last_rows);
  DmWs w;
  if (ws_bytes < dm_carve(ws, Kc, &w)) return RAMP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // the one memset: the status words are the counters
  if (hipMemsetAsync(status, 0, 8 * sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  DmProject a;
  a.poses = poses; a.patches = patches; a.intrinsics = intrinsics; a.cam = cam; a.conf = conf;
  a.index = index; a.count = count; a.dyn_rows = dyn_rows;
  a.hdr = w.hdr; a.rec = w.rec; a.status = status; a.records = records;
  a.scale = scale; a.R = radius; a.n = n; a.K = Kc; a.M = M; a.PP = P * P; a.ctr = (P / 2) * P + P / 2;
  a.per_row = per_row; a.last_rows = last_rows; a.conf_is_variance = (flags & RAMP_DEPTHMAP_CONF_IS_VARIANCE) ? 1 : 0;
  a.H = H; a.W = W;
  // (a capacity of zero still launches: the live count and the flag word are written on the device)
  hipLaunchKernelGGL(dm_project_kernel, dim3(Kc > 0 ? ramp_cdiv(Kc, DM_THREADS) : 1), dim3(DM_THREADS), 0, st, a);
  RAMP_CHECK_LAUNCH();
  if (invdepth || weight) {
    const int gx = ramp_cdiv(W, DM_TILE_W), gy = ramp_cdiv(H, DM_TILE_H);
    hipLaunchKernelGGL(dm_regress_kernel, dim3(gx, gy), dim3(DM_THREADS), 0, st, a.rec, a.hdr, prior, prior_weight,
                       (flags & RAMP_DEPTHMAP_PRIOR_RELATIVE) ? 1 : 0, radius, H, W, invdepth, weight, status);
    RAMP_CHECK_LAUNCH();
  }
  return RAMP_OK;
}
}  // extern "C"
