// fastba.BA on gfx950: Gauss-Newton bundle adjustment of the sliding window.
//
// The reference accumulates the normal equations with ~340 float atomics per
// edge into a 60x60 matrix and then runs ~25 ATen launches per iteration.  Here
// every reduction is an ORDERED SEGMENT SUM (deterministic, no float atomics):
//
//   prep   group the edges by patch (kk) and by pose pair (ii,jj)  [graph.hip]
//   K1     per-edge record: residual, validity, Jacobians (32 floats).  With free poses K2 / K3 recompute it
//          in registers and nothing is launched; without one ba_edge_kernel writes it to memory
//   K2     patch role: one workgroup per patch walks its edge segment and
//          emits the dense E row [6N], C, u, Q = 1/(C+lambda)
//   K3     pair role: one workgroup per (i,j) segment emits the 6x6 blocks
//          w*Ji*Ji', w*Jj*Jj', -w*Ji*Jj', -w*Jj*Ji' and the gradient parts
//          (K2 and K3 are ONE launch, ba_patch_pair_kernel; without a free pose ba_patch_kernel alone)
//   K4     split-K SYRK: partial  E' diag(Q) E  and  E' diag(Q) u  (ba_schur1_kernel for a system of one tile
//          whose chunk fits the LDS, otherwise ba_schur_kernel)
//   K5     assemble  S = B - sum(partials),  y = v - ..., damping  (ba_assemble2_kernel up to 16 poses,
//          ba_assemble_kernel above)
//   K6     ba_cholb_kernel: single-workgroup LDS Cholesky + triangular solves -> dX
//   K7     ba_retract_kernel: dZ = Q (u - E dX), depth retraction, SE3 pose retraction
// K1 .. K5 are ba_build_system(); an iteration of the solver is ba_build_system(), K6, K7 (K4 .. K6 only with free poses).
//
// ramp_ba_covariance (the window's uncertainty) runs ba_build_system() once at the state passed in, then
//   C1     ba_cholinv_kernel: K6's factorisation (ba_chol_factor, without the rhs row) + in-place triangular inverse -> L^-1
//   C2     ba_cov_expand_kernel: cov = L^-T L^-1 (tiles), depth_var = Q + Q^2 |L^-1 e_k|^2 and the chi2 partials (one
//          wave per patch)
//   C3     ba_cov_stats_kernel: chi2 / valid count from the partials, in group order
//   C4     ba_map_kernel (ramp_ba_map_covariance only): the pose-depth cross term -Q_k (L^-T L^-1 e_k) of the patch's source
//          frame, the patch's world point and its 3 x 3 covariance (one wave per patch)
// and never K7: poses and patches are only read.  ramp_map_select (map_select_kernel) compacts the points that pass the
// caller's thresholds, in patch order.
//
// Math restates ramp/fastba/ba_cuda.cu:232-376 (kernel), 433-582 (host loop),
// 178-229 (retractions).  Everything is fp32 like the reference (mtype=float).
#include "ramp_device.h"
#include <stdlib.h>
#include "ramp_internal.h"

#define BA_REC 32     // floats per edge record
#define BA_PAIR 160   // floats per pair record (156 used)
#define BA_TS 64      // SYRK tile
#define BA_KB 8       // SYRK k batch


// ------------------------------------------------------------------ K1
// The per-edge record: residual, validity, Jacobians (32 floats).  ba_edge_kernel writes it to memory (the path without
// free poses); the patch / pair roles of a regular iteration recompute it in registers from the edge's 116 bytes of
// inputs while they stage their segment -- the record never goes through HBM (it was written once and read twice per
// iteration) and the launch is gone.  Same expressions either way: identical results.
struct BaEdgeIn {
  const float *poses, *patches, *intr, *target, *weight;
  const int64_t *ii, *jj, *kk;
  int PP, c11, t0, N;
};
// (gate: the validity mask on its own, 1 / 0 -- the record only carries it multiplied into the weights)
__device__ __forceinline__ void ba_edge_compute_gate(const BaEdgeIn &in, int n, float (&r)[BA_REC], float &gate) {
  const float fx = in.intr[0], fy = in.intr[1], cx = in.intr[2], cy = in.intr[3];
  int ix = (int)in.ii[n], jx = (int)in.jj[n];
  const long kx = in.kk[n];
  float pi[7], pj[7];
#pragma unroll
  for (int c = 0; c < 7; c++) { pi[c] = in.poses[7 * (size_t)ix + c]; pj[c] = in.poses[7 * (size_t)jx + c]; }
  float Xi[4], Xj[4];
  Xi[0] = (in.patches[((size_t)kx * 3 + 0) * in.PP + in.c11] - cx) / fx;
  Xi[1] = (in.patches[((size_t)kx * 3 + 1) * in.PP + in.c11] - cy) / fy;
  Xi[2] = 1.0f;
  Xi[3] = in.patches[((size_t)kx * 3 + 2) * in.PP + in.c11];
  float tij[3], qij[4];
  fb_relSE3(pi, pi + 3, pj, pj + 3, tij, qij);
  fb_actSE3(tij, qij, Xi, Xj);
  const float X = Xj[0], Y = Xj[1], Z = Xj[2], W = Xj[3];
  const float d = (Z >= 0.2f) ? 1.0f / Z : 0.0f;
  const float d2 = d * d;
  const float x1 = fx * (X / Z) + cx;
  const float y1 = fy * (Y / Z) + cy;
  const float tx_ = in.target[2 * (size_t)n + 0], ty_ = in.target[2 * (size_t)n + 1];
  const float rx = tx_ - x1, ry = ty_ - y1;
  const bool in_bounds = (sqrtf(rx * rx + ry * ry) < 128) && (Z > 0.2f) && (x1 > -64) &&
                         (y1 > -64) && (x1 < 2 * cx + 64) && (y1 < 2 * cy + 64);
  const float mask = in_bounds ? 1.0f : 0.0f;
  ix -= in.t0;
  jx -= in.t0;
  if (ix >= in.N) ix = -1;  // poses >= t1 are not free (out of B in the reference)
  if (jx >= in.N) jx = -1;
  if (ix < 0) ix = -1;
  if (jx < 0) jx = -1;
  float Jj0[6] = {fx * W * d, 0, fx * -X * W * d2, fx * -X * Y * d2, fx * (1 + X * X * d2),
                  fx * -Y * d};
  float Jj1[6] = {0, fy * W * d, fy * -Y * W * d2, fy * (-1 - Y * Y * d2), fy * (X * Y * d2),
                  fy * X * d};
  float Ji0[6], Ji1[6];
  fb_adjSE3(tij, qij, Jj0, Ji0);
  fb_adjSE3(tij, qij, Jj1, Ji1);
  const float Jz0 = fx * (tij[0] * d - tij[2] * (X * d2));
  const float Jz1 = fy * (tij[1] * d - tij[2] * (Y * d2));
#pragma unroll
  for (int c = 0; c < 6; c++) { r[c] = Ji0[c]; r[6 + c] = Ji1[c]; r[12 + c] = Jj0[c]; r[18 + c] = Jj1[c]; }
  r[24] = mask * in.weight[2 * (size_t)n + 0];
  r[25] = mask * in.weight[2 * (size_t)n + 1];
  r[26] = rx; r[27] = ry; r[28] = Jz0; r[29] = Jz1;
  r[30] = __int_as_float(ix); r[31] = __int_as_float(jx);
  gate = mask;
}
__device__ __forceinline__ void ba_edge_compute(const BaEdgeIn &in, int n, float (&r)[BA_REC]) {
  float gate;
  ba_edge_compute_gate(in, n, r, gate);
}
// window from the device-side sizes (csrc/track.hip): [max(n - opt_window, 1), n)
__device__ __forceinline__ void ba_dyn_window(const int32_t *dyn, int opt_window, int &t0, int &N) {
  if (!dyn) return;
  const int t1 = dyn[RAMP_DYN_N];
  t0 = max(t1 - opt_window, 1);
  N = min(N, t1 - t0);
}
__global__ void __launch_bounds__(256)
    ba_edge_kernel(BaEdgeIn in, float *__restrict__ rec, int E, const int32_t *__restrict__ dyn, int opt_window) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (dyn) E = dyn[RAMP_DYN_E];              // device-side sizes: E is the launch bound, the window ends at n
  ba_dyn_window(dyn, opt_window, in.t0, in.N);
  if (n >= E) return;
  float r[BA_REC];
  ba_edge_compute(in, n, r);
  float4 *r4 = reinterpret_cast<float4 *>(rec + (size_t)n * BA_REC);
#pragma unroll
  for (int c = 0; c < 8; c++) r4[c] = make_float4(r[4 * c], r[4 * c + 1], r[4 * c + 2], r[4 * c + 3]);
}
// record field offsets
#define R_JI0 0
#define R_JI1 6
#define R_JJ0 12
#define R_JJ1 18
#define R_W0 24
#define R_W1 25
#define R_R0 26
#define R_R1 27
#define R_JZ0 28
#define R_JZ1 29
#define R_I 30
#define R_J 31

// ------------------------------------------------------------------ K2
// One workgroup per patch (group of edges with the same kk).  The group's records are staged in LDS
// with all loads in flight at once (walking them from memory is one dependent round trip per edge);
// the sums run over the staged records in segment order.
#define BA_PCHUNK 32
constexpr int BA_PBATCH = 48;   // (128 / 224 measured on MI355X: 126 / 139 us per BA call against 124 -- the pair role is not the long one)
// FUSED: one thread per edge of the chunk recomputes its record (ein); otherwise the records are read from rec
template <bool FUSED>
__device__ __forceinline__ void
    ba_patch_body(int g, const float *__restrict__ rec, const int32_t *__restrict__ order,
                  const int32_t *__restrict__ seg, const int32_t *__restrict__ ngroups,
                  const float *__restrict__ lmbda, float *__restrict__ Erow,
                  float *__restrict__ Cv, float *__restrict__ uv, float *__restrict__ Qv,
                  int n6, const BaEdgeIn &ein, float *__restrict__ s_buf) {
  float (*s_rec)[BA_REC + 1] = reinterpret_cast<float (*)[BA_REC + 1]>(s_buf);      // [BA_PCHUNK][BA_REC + 1]
  if (g >= *ngroups) return;
  // The merged launch's workgroups are sized for the pair role (156 sums); a patch needs n6 + 2 threads.  Waves without a
  // column leave at once (the barrier counts live waves only): a CU holds 32 waves, and 2,100 patch workgroups of four
  // live waves each were a second round of workgroups behind 2,048 places -- with one live wave they are all resident.
  // (whole waves leave in front of the barriers below: s_barrier on gfx9 / CDNA counts the waves that are still alive, so the
  // remaining ones synchronise among themselves.  This library is built for gfx950 only; a target whose barrier counts
  // launched waves would hang here -- hence the check)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "ba_patch_body retires whole waves before __syncthreads(): valid on gfx9 / CDNA barriers only"
#endif
  const int nthr = min((int)blockDim.x, ((n6 + 2 + 63) / 64) * 64);
  if ((int)threadIdx.x >= nthr) return;
  const int tid = threadIdx.x;
  const int s0 = seg[g], s1 = seg[g + 1];
  const int a = tid / 6, c = tid - a * 6;
  float acc = 0.0f;
  for (int b0 = s0; b0 < s1; b0 += BA_PCHUNK) {
    const int nb = min(BA_PCHUNK, s1 - b0);
    __syncthreads();
    if (FUSED) {
      if (tid < nb) {
        float r[BA_REC];
        ba_edge_compute(ein, order[b0 + tid], r);
#pragma unroll
        for (int k = 0; k < BA_REC; k++) s_rec[tid][k] = r[k];
      }
    } else {
      for (int e = tid; e < nb * BA_REC; e += nthr) {
        const int l = e / BA_REC, k = e - l * BA_REC;
        s_rec[l][k] = rec[(size_t)order[b0 + l] * BA_REC + k];
      }
    }
    __syncthreads();
    if (tid < n6) {
      for (int l = 0; l < nb; l++) {
        const float *r = s_rec[l];
        const int i = __float_as_int(r[R_I]), j = __float_as_int(r[R_J]);
        if (i == a) acc += (-r[R_W0] * r[R_JZ0]) * r[R_JI0 + c];
        if (j == a) acc += (r[R_W0] * r[R_JZ0]) * r[R_JJ0 + c];
        if (i == a) acc += (-r[R_W1] * r[R_JZ1]) * r[R_JI1 + c];
        if (j == a) acc += (r[R_W1] * r[R_JZ1]) * r[R_JJ1 + c];
      }
    } else if (tid == n6) {
      for (int l = 0; l < nb; l++) {
        const float *r = s_rec[l];
        acc += (r[R_W0] * r[R_JZ0]) * r[R_JZ0];
        acc += (r[R_W1] * r[R_JZ1]) * r[R_JZ1];
      }
    } else if (tid == n6 + 1) {
      for (int l = 0; l < nb; l++) {
        const float *r = s_rec[l];
        acc += (r[R_W0] * r[R_R0]) * r[R_JZ0];
        acc += (r[R_W1] * r[R_R1]) * r[R_JZ1];
      }
    }
  }
  if (tid < n6) {
    Erow[(size_t)g * n6 + tid] = acc;
  } else if (tid == n6) {
    Cv[g] = acc;
    Qv[g] = 1.0f / (acc + lmbda[0]);
  } else if (tid == n6 + 1) {
    uv[g] = acc;
  }
}

__global__ void __launch_bounds__(256)
    ba_patch_kernel(const float *__restrict__ rec, const int32_t *__restrict__ order,
                    const int32_t *__restrict__ seg, const int32_t *__restrict__ ngroups,
                    const float *__restrict__ lmbda, float *__restrict__ Erow,
                    float *__restrict__ Cv, float *__restrict__ uv, float *__restrict__ Qv,
                    int n6) {
  __shared__ __attribute__((aligned(16))) float s_buf[BA_PCHUNK * (BA_REC + 1)];
  ba_patch_body<false>(blockIdx.x, rec, order, seg, ngroups, lmbda, Erow, Cv, uv, Qv, n6, BaEdgeIn(), s_buf);
}

// ------------------------------------------------------------------ K3
// pair record: [0,36) w Ji Ji', [36,72) w Jj Jj', [72,108) -w Ji Jj',
// [108,144) -w Jj Ji', [144,150) -w r Ji, [150,156) w r Jj.  Threads >= 156 only take part in the barriers.
__device__ __forceinline__ void
    ba_pair_body(int g, const int32_t *__restrict__ order, const int32_t *__restrict__ seg,
                 const int32_t *__restrict__ ngroups, float *__restrict__ pairs, int32_t *__restrict__ pair_ij,
                 const BaEdgeIn &ein, float *__restrict__ s_rec) {
  // BA_PBATCH records per batch (any batch size sums the records in the same order: identical values)
  if (g >= *ngroups) return;
  const int tid = threadIdx.x;
  const int s0 = seg[g], s1 = seg[g + 1];
  int blk = 0, x = 0, y = 0, oa = 0, ob = 0;
  float sgn = 1.0f;
  if (tid < 144) {
    blk = tid / 36;
    const int q = tid - blk * 36;
    x = q / 6; y = q - x * 6;
    oa = (blk == 0 || blk == 2) ? R_JI0 : R_JJ0;  // left factor
    ob = (blk == 0 || blk == 3) ? R_JI0 : R_JJ0;  // right factor
    sgn = (blk >= 2) ? -1.0f : 1.0f;
  } else if (tid < 156) {
    const int q = tid - 144;
    const bool isj = q >= 6;
    x = isj ? q - 6 : q;
    oa = isj ? R_JJ0 : R_JI0;
    sgn = isj ? 1.0f : -1.0f;
  }
  float acc = 0.0f;
  for (int b0 = s0; b0 < s1; b0 += BA_PBATCH) {
    const int nb = min(BA_PBATCH, s1 - b0);
    __syncthreads();
    if (tid < nb) {                             // one thread per edge of the batch recomputes its record
      float r[BA_REC];
      ba_edge_compute(ein, order[b0 + tid], r);
#pragma unroll
      for (int c = 0; c < BA_REC / 4; c++)
        reinterpret_cast<float4 *>(s_rec)[tid * (BA_REC / 4) + c] = make_float4(r[4 * c], r[4 * c + 1], r[4 * c + 2], r[4 * c + 3]);
    }
    __syncthreads();
    if (tid < 144) {
      for (int p = 0; p < nb; p++) {
        const float *r = s_rec + p * BA_REC;
        acc += ((sgn * r[R_W0]) * r[oa + x]) * r[ob + y];
        acc += ((sgn * r[R_W1]) * r[oa + 6 + x]) * r[ob + 6 + y];
      }
    } else if (tid < 156) {
      for (int p = 0; p < nb; p++) {
        const float *r = s_rec + p * BA_REC;
        acc += ((sgn * r[R_W0]) * r[R_R0]) * r[oa + x];
        acc += ((sgn * r[R_W1]) * r[R_R1]) * r[oa + 6 + x];
      }
    }
    if (b0 == s0 && tid == 0) {
      pair_ij[2 * g + 0] = __float_as_int(s_rec[R_I]);
      pair_ij[2 * g + 1] = __float_as_int(s_rec[R_J]);
    }
  }
  if (tid < 156) pairs[(size_t)g * BA_PAIR + tid] = acc;
}

// K2 and K3 need the same per-edge records and do not depend on each other: one launch, the first n_patch
// workgroups take the patch role, the rest the pair role
__global__ void __launch_bounds__(256)
    ba_patch_pair_kernel(int n_patch, const int32_t *__restrict__ order_k,
                         const int32_t *__restrict__ seg_k, const int32_t *__restrict__ nk,
                         const float *__restrict__ lmbda, float *__restrict__ Erow, float *__restrict__ Cv,
                         float *__restrict__ uv, float *__restrict__ Qv, int n6,
                         const int32_t *__restrict__ order_p, const int32_t *__restrict__ seg_p,
                         const int32_t *__restrict__ np, float *__restrict__ pairs, int32_t *__restrict__ pair_ij,
                         BaEdgeIn ein, const int32_t *__restrict__ dyn, int opt_window) {
  ba_dyn_window(dyn, opt_window, ein.t0, ein.N);
  __shared__ __attribute__((aligned(16))) float s_buf[BA_PBATCH * BA_REC];     // one array for both roles (6 KB)
  static_assert(BA_PBATCH * BA_REC >= BA_PCHUNK * (BA_REC + 1) && BA_PBATCH <= 256, "role buffers / one thread per record");
  if ((int)blockIdx.x < n_patch)
    ba_patch_body<true>(blockIdx.x, nullptr, order_k, seg_k, nk, lmbda, Erow, Cv, uv, Qv, n6, ein, s_buf);
  else
    ba_pair_body(blockIdx.x - n_patch, order_p, seg_p, np, pairs, pair_ij, ein, s_buf);
}

// ------------------------------------------------------------------ K4
// S_part[z] = sum_{k in chunk z} Q_k E_k E_k' (64x64 tile per block),
// y_part[z] = sum Q_k u_k E_k
__global__ void __launch_bounds__(256)
    ba_schur_kernel(const float *__restrict__ Erow, const float *__restrict__ Qv,
                    const float *__restrict__ uv, const int32_t *__restrict__ ngroups,
                    float *__restrict__ S_part, float *__restrict__ y_part, int n6, int KS) {
  __shared__ float Ea[BA_KB][BA_TS];  // scaled by Q
  __shared__ float Eb[BA_KB][BA_TS];
  __shared__ float us[BA_KB];
  const int nk = *ngroups;
  const int z = blockIdx.z;
  const int per = (nk + KS - 1) / KS;
  const int k0 = z * per, k1 = min(nk, k0 + per);
  const int r0 = blockIdx.x * BA_TS, c0 = blockIdx.y * BA_TS;
  const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
  float acc[4][4];
  float yacc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0.0f;
  for (int kb = k0; kb < k1; kb += BA_KB) {
    __syncthreads();
    for (int q = tid; q < BA_KB * BA_TS; q += 256) {
      const int kq = q / BA_TS, col = q - kq * BA_TS;
      const int k = kb + kq;
      float va = 0.0f, vb = 0.0f;
      if (k < k1) {
        if (r0 + col < n6) va = Erow[(size_t)k * n6 + r0 + col] * Qv[k];
        if (c0 + col < n6) vb = Erow[(size_t)k * n6 + c0 + col];
      }
      Ea[kq][col] = va;
      Eb[kq][col] = vb;
    }
    if (tid < BA_KB) us[tid] = (kb + tid < k1) ? uv[kb + tid] : 0.0f;
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < BA_KB; kq++) {
      float a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; q++) { a[q] = Ea[kq][ty * 4 + q]; b[q] = Eb[kq][tx * 4 + q]; }
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = __builtin_fmaf(a[x], b[y], acc[x][y]);
      if (blockIdx.y == 0 && tx == 0) {
        const float u = us[kq];
#pragma unroll
        for (int x = 0; x < 4; x++) yacc[x] = __builtin_fmaf(a[x], u, yacc[x]);
      }
    }
  }
#pragma unroll
  for (int x = 0; x < 4; x++) {
    const int r = r0 + ty * 4 + x;
    if (r >= n6) continue;
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int c = c0 + tx * 4 + y;
      if (c < n6) S_part[((size_t)z * n6 + r) * n6 + c] = acc[x][y];
    }
    if (blockIdx.y == 0 && tx == 0) y_part[(size_t)z * n6 + r] = yacc[x];
  }
}

// K4 for systems of one tile (6N <= 64) whose split-K chunk fits the LDS: the chunk's E rows, Q and u are staged ONCE (every
// load of the workgroup in flight together -- ba_schur_kernel walks the chunk in batches of 8 rows, one dependent memory round
// trip per batch), then the products run from LDS.  Same fma chain per entry in the same k order: identical partials.
#define BA_S1_ROWS 160
__global__ void __launch_bounds__(256)
    ba_schur1_kernel(const float *__restrict__ Erow, const float *__restrict__ Qv, const float *__restrict__ uv,
                     const int32_t *__restrict__ ngroups, float *__restrict__ S_part, float *__restrict__ y_part, int n6, int KS) {
  __shared__ float Es[BA_S1_ROWS][BA_TS];
  __shared__ float Qs[BA_S1_ROWS], us[BA_S1_ROWS];
  const int nk = *ngroups;
  const int z = blockIdx.z;
  const int per = (nk + KS - 1) / KS;
  const int k0 = z * per, k1 = min(nk, k0 + per);
  const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
  const int rows = max(k1 - k0, 0);
  for (int q0 = 0; q0 < rows * BA_TS; q0 += 12 * 256) {      // 12 loads per thread in flight (48 rows: one round trip)
    float ev[12];
#pragma unroll
    for (int u = 0; u < 12; u++) {
      const int q = q0 + u * 256 + tid;
      const int kq = q / BA_TS, col = q - kq * BA_TS;
      ev[u] = (q < rows * BA_TS && col < n6) ? Erow[(size_t)(k0 + kq) * n6 + col] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 12; u++) {
      const int q = q0 + u * 256 + tid;
      if (q < rows * BA_TS) Es[q / BA_TS][q % BA_TS] = ev[u];
    }
  }
  for (int q = tid; q < rows; q += 256) { Qs[q] = Qv[k0 + q]; us[q] = uv[k0 + q]; }
  __syncthreads();
  float acc[4][4];
  float yacc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0.0f;
  // (ba_schur_kernel pads its last batch of 8 with zero rows: fma(0, 0, acc) leaves acc as it is, nothing to reproduce)
  for (int kq = 0; kq < rows; kq++) {
    float a[4], b[4];
    const float qk = Qs[kq];
#pragma unroll
    for (int q = 0; q < 4; q++) { a[q] = Es[kq][ty * 4 + q] * qk; b[q] = Es[kq][tx * 4 + q]; }
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
      for (int y = 0; y < 4; y++) acc[x][y] = __builtin_fmaf(a[x], b[y], acc[x][y]);
    if (tx == 0) {
      const float u = us[kq];
#pragma unroll
      for (int x = 0; x < 4; x++) yacc[x] = __builtin_fmaf(a[x], u, yacc[x]);
    }
  }
#pragma unroll
  for (int x = 0; x < 4; x++) {
    const int r = ty * 4 + x;
    if (r >= n6) continue;
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int c = tx * 4 + y;
      if (c < n6) S_part[((size_t)z * n6 + r) * n6 + c] = acc[x][y];
    }
    if (tx == 0) y_part[(size_t)z * n6 + r] = yacc[x];
  }
}

// ------------------------------------------------------------------ K5
// One workgroup per free pose a (block row of S).  The pair records that touch pose a are first
// compacted IN ORDER into LDS (ballot prefix), then every thread sums its entries of the 6 x 6N
// row block over that short list -- fixed order, no atomics.
#define BA_MAXLIST 1024
#define BA_CHUNK 48
__global__ void __launch_bounds__(256)
    ba_assemble_kernel(const float *__restrict__ pairs, const int32_t *__restrict__ pair_ij,
                       const int32_t *__restrict__ npairs, const float *__restrict__ S_part,
                       const float *__restrict__ y_part, float *__restrict__ S,
                       float *__restrict__ yv, int n6, int KS, int32_t *__restrict__ info) {
  __shared__ int s_list[BA_MAXLIST];
  __shared__ int s_wcnt[4];
  __shared__ int s_base;
  const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np = *npairs;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int g0 = 0; g0 < np; g0 += 256) {
    const int g = g0 + tid;
    const bool hit = g < np && (pair_ij[2 * g] == a || pair_ij[2 * g + 1] == a);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; w++) off += s_wcnt[w];
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (hit && off < BA_MAXLIST) s_list[off] = g;
    __syncthreads();
    if (tid == 0) s_base += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    __syncthreads();
  }
  const int nl = min(s_base, BA_MAXLIST);
  // more pair records on one pose than the list holds (> 512 frames connected to one): the result would silently lose
  // terms -- flagged in *info (bit 1), never truncated quietly
  if (s_base > BA_MAXLIST && tid == 0 && info) atomicOr(info, 2);
  // The listed pair records are staged through LDS in chunks (coalesced, all loads in flight at
  // once) -- walking them straight from memory costs one dependent global round trip per record.
  __shared__ __attribute__((aligned(16))) float s_pr[BA_CHUNK][BA_PAIR];
  __shared__ int s_i[BA_CHUNK], s_j[BA_CHUNK];
  // the 6 x 6N row block is split over gridDim.y workgroups
  const int epb = (6 * n6 + (int)gridDim.y - 1) / (int)gridDim.y;
  const int q_lo = blockIdx.y * epb, q_hi = min(6 * n6, q_lo + epb);
  constexpr int QMAX = 5;                    // entries per thread (epb <= 1280)
  float bsum[QMAX], vsum[QMAX];
#pragma unroll
  for (int t = 0; t < QMAX; t++) { bsum[t] = 0.0f; vsum[t] = 0.0f; }
  for (int l0 = 0; l0 < nl; l0 += BA_CHUNK) {
    const int cnt = min(BA_CHUNK, nl - l0);
    __syncthreads();
    constexpr int V4 = BA_PAIR / 4;            // float4 pieces per record
    for (int e0 = 0; e0 < cnt * V4; e0 += 4 * 256) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {              // 4 independent 16-byte loads per thread in flight
        const int e = e0 + u * 256 + tid;
        const int l = min(e / V4, cnt - 1), k = e % V4;
        v[u] = reinterpret_cast<const float4 *>(pairs + (size_t)s_list[l0 + l] * BA_PAIR)[k];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int e = e0 + u * 256 + tid;
        if (e < cnt * V4) reinterpret_cast<float4 *>(&s_pr[e / V4][0])[e % V4] = v[u];
      }
    }
    if (tid < cnt) {
      const int g = s_list[l0 + tid];
      s_i[tid] = pair_ij[2 * g];
      s_j[tid] = pair_ij[2 * g + 1];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < QMAX; t++) {
      const int q = q_lo + tid + t * 256;
      if (q >= q_hi) break;
      const int x = q / n6, c = q - x * n6;
      const int b = c / 6, y = c - b * 6;
      for (int l = 0; l < cnt; l++) {          // ascending list order: the fixed summation order
        const int i = s_i[l], j = s_j[l];
        const float *pr = s_pr[l];
        if (i == a && i == b) bsum[t] += pr[x * 6 + y];
        if (j == a && j == b) bsum[t] += pr[36 + x * 6 + y];
        if (i == a && j == b) bsum[t] += pr[72 + x * 6 + y];
        if (j == a && i == b) bsum[t] += pr[108 + x * 6 + y];
        if (c == 0) {
          if (i == a) vsum[t] += pr[144 + x];
          if (j == a) vsum[t] += pr[150 + x];
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < QMAX; t++) {
    const int q = q_lo + tid + t * 256;
    if (q >= q_hi) break;
    const int x = q / n6, c = q - x * n6;
    const int r = 6 * a + x;
    // split-K partials in z order, all KS <= 64 loads in flight (branch-free: clamped index, masked add)
    float sp = 0.0f;
    {
      float v[64];
#pragma unroll
      for (int u = 0; u < 64; u++) v[u] = S_part[((size_t)(u < KS ? u : KS - 1) * n6 + r) * n6 + c];
#pragma unroll
      for (int u = 0; u < 64; u++) sp += u < KS ? v[u] : 0.0f;
    }
    float s = bsum[t] - sp;
    if (r == c) s += (1e-4f * s + 1.0f);
    S[(size_t)r * n6 + c] = s;
    if (c == 0) {
      float yp = 0.0f;
      {
        float v[64];
#pragma unroll
        for (int u = 0; u < 64; u++) v[u] = y_part[(size_t)(u < KS ? u : KS - 1) * n6 + r];
#pragma unroll
        for (int u = 0; u < 64; u++) yp += u < KS ? v[u] : 0.0f;
      }
      yv[r] = vsum[t] - yp;
    }
  }
}

// ------------------------------------------------------------------ K5, one workgroup per 6 x 6 block
// S[6a.., 6b..] = B block - sum of the split-K partials (+ damping on the diagonal), y likewise (by the diagonal workgroup).
// An off-diagonal block (a, b) takes the <= 2 pair records (i, j) = (a, b) / (b, a); the diagonal block (a, a) every record
// with i == a or j == a (~2 x the window): 7 lanes per entry sum every 7th listed record in ascending order and the seven
// partial sums are added in lane order -- fixed order, no atomics, 20-odd independent loads per thread instead of a chain
// of chunks staged through LDS behind barriers (ba_assemble_kernel: one workgroup per POSE, 19 us of a 139 us call).
// (A single lane per entry -- ascending record order, ba_assemble_kernel's -- was slower than that kernel: 151 vs 138 us per
// call.  The interleaved order moves the 180 x 180 solve of the precise.yaml window by 6e-4 of the step against the oracle --
// fp32 rounding through its conditioning -- so windows above 16 poses keep ba_assemble_kernel.)
#define BA_AP 7
__global__ void __launch_bounds__(256)
    ba_assemble2_kernel(const float *__restrict__ pairs, const int32_t *__restrict__ pair_ij,
                        const int32_t *__restrict__ npairs, const float *__restrict__ S_part,
                        const float *__restrict__ y_part, float *__restrict__ S, float *__restrict__ yv, int n6, int KS,
                        int32_t *__restrict__ info) {
  __shared__ int s_list[BA_MAXLIST], s_i[BA_MAXLIST], s_j[BA_MAXLIST];
  __shared__ int s_wcnt[4];
  __shared__ int s_base;
  __shared__ float s_part[BA_AP][48];
  const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np = *npairs;
  const bool diag = a == b;
  // the split-K partials of this thread's entry do not depend on the pair lists: their loads go out first and are in flight
  // while the list is built (one dependent memory round trip less on a launch that is nothing but round trips)
  float spv[64];
  if (tid < 36) {
    const int r = 6 * a + tid / 6, c = 6 * b + tid % 6;
#pragma unroll
    for (int u = 0; u < 64; u++) spv[u] = S_part[((size_t)(u < KS ? u : KS - 1) * n6 + r) * n6 + c];
  } else if (tid < 42 && diag) {
    const int r = 6 * a + tid - 36;
#pragma unroll
    for (int u = 0; u < 64; u++) spv[u] = y_part[(size_t)(u < KS ? u : KS - 1) * n6 + r];
  }
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int g0 = 0; g0 < np; g0 += 256) {
    const int g = g0 + tid;
    int pi = -2, pj = -2;
    if (g < np) { pi = pair_ij[2 * g]; pj = pair_ij[2 * g + 1]; }
    const bool hit = diag ? (pi == a || pj == a) : ((pi == a && pj == b) || (pi == b && pj == a));
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; w++) off += s_wcnt[w];
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (hit && off < BA_MAXLIST) { s_list[off] = g; s_i[off] = pi; s_j[off] = pj; }
    __syncthreads();
    if (tid == 0) s_base += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    __syncthreads();
  }
  const int nl = min(s_base, BA_MAXLIST);
  if (s_base > BA_MAXLIST && tid == 0 && info) atomicOr(info, 2);       // (never a silent truncation)
  // threads [0, 36 AP): entry e = tid / AP (x = e / 6, y = e % 6), partial lane pl = tid % AP; [36 AP, 42 AP): gradient x
  const int e = tid / BA_AP, pl = tid - e * BA_AP;
  float acc = 0.f;
  if (e < 36) {
    const int x = e / 6, y = e - x * 6;
    for (int l = pl; l < nl; l += BA_AP) {
      const int i = s_i[l], j = s_j[l];
      const float *pr = pairs + (size_t)s_list[l] * BA_PAIR + x * 6 + y;
      // (the four conditions and their order are ba_assemble_kernel's)
      const float v0 = (i == a && i == b) ? pr[0] : 0.f, v1 = (j == a && j == b) ? pr[36] : 0.f;
      const float v2 = (i == a && j == b) ? pr[72] : 0.f, v3 = (j == a && i == b) ? pr[108] : 0.f;
      if (i == a && i == b) acc += v0;
      if (j == a && j == b) acc += v1;
      if (i == a && j == b) acc += v2;
      if (j == a && i == b) acc += v3;
    }
    s_part[pl][e] = acc;
  }
  if (diag && tid < 6 * BA_AP) {                     // the gradient's six entries, the same way (threads 0 .. 41 again)
    const int x = tid / BA_AP, p2 = tid - x * BA_AP;
    float g = 0.f;
    for (int l = p2; l < nl; l += BA_AP) {
      const float *pr = pairs + (size_t)s_list[l] * BA_PAIR;
      if (s_i[l] == a) g += pr[144 + x];
      if (s_j[l] == a) g += pr[150 + x];
    }
    s_part[p2][36 + x] = g;
  }
  __syncthreads();
  if (tid < 36) {
    const int x = tid / 6, y = tid - x * 6;
    float bs = 0.f;
#pragma unroll
    for (int q = 0; q < BA_AP; q++) bs += s_part[q][tid];
    const int r = 6 * a + x, c = 6 * b + y;
    float sp = 0.0f;
#pragma unroll
    for (int u = 0; u < 64; u++) sp += u < KS ? spv[u] : 0.0f;
    float sv = bs - sp;
    if (r == c) sv += (1e-4f * sv + 1.0f);
    S[(size_t)r * n6 + c] = sv;
  } else if (tid < 42 && diag) {
    const int x = tid - 36, r = 6 * a + x;
    float vs = 0.f;
#pragma unroll
    for (int q = 0; q < BA_AP; q++) vs += s_part[q][tid];
    float yp = 0.0f;
#pragma unroll
    for (int u = 0; u < 64; u++) yp += u < KS ? spv[u] : 0.0f;
    yv[r] = vs - yp;
  }
}

// ------------------------------------------------------------------ K6
// Single workgroup, matrix in LDS, blocked Cholesky (block width 6 = one pose).  Per block column every thread factors the 6 x 6 diagonal block in
// REGISTERS (21 broadcast LDS reads, then no LDS traffic inside the dependency chain: with the block left in LDS the
// loads cannot move above the stores and every one of them is an exposed round trip), the row threads solve their
// panel row against it, and the whole workgroup applies the rank-6 update to the trailing matrix on a BA_TG x BA_TG thread
// grid -- two barriers per pose instead of one per column.  In the solver the right-hand side rides along as row n6
// (z = L^-1 y falls out of the panel solves) and the back substitution is blocked the same way; the covariance factors
// the same matrix without that row and inverts L in place.
#define BA_TG 32      // the workgroup is BA_TG x BA_TG = 1024 threads

// S ([n6][n6] in memory) into LDS rows of stride ld; every thread of the workgroup calls it
__device__ __forceinline__ void ba_stage_S(float *__restrict__ A, const float *__restrict__ S, int n6, int ld) {
  const int tid = threadIdx.x, nt = BA_TG * BA_TG;
  int r = tid / n6, c = tid - r * n6;          // one division, then stepping
  const int dr = nt / n6, dc = nt - dr * n6;
  for (int q = tid; q < n6 * n6; q += nt) {
    A[r * ld + c] = S[q];
    r += dr; c += dc;
    if (c >= n6) { c -= n6; r++; }
  }
}

// S = L L' in place on a matrix that is already in LDS (A: (n6 + RHS) x ld, lower triangle; with RHS the right-hand side
// is row n6 and leaves as z = L^-1 y).  Lk [n6 / 6][28] takes the factored diagonal blocks (21 lower entries + 6 inverse
// pivots), *s_bad is set where a pivot is not positive.  Every thread of the workgroup calls it; it ends on a barrier.
template <int RHS>
__device__ __forceinline__ void ba_chol_factor(float *__restrict__ A, float *__restrict__ Lk, int *s_bad, int n6) {
  const int ld = n6 + 1;
  const int tid = threadIdx.x, nt = BA_TG * BA_TG;
  const int ty = tid / BA_TG, tx = tid % BA_TG;
  if (tid == 0) *s_bad = 0;
  __syncthreads();
  const int nb = n6 / 6;
  for (int kb = 0; kb < nb; kb++) {
    const int c0 = 6 * kb;
    const int r0 = c0 + 6, m = n6 - r0;        // m trailing columns, m + RHS rows
    // only the waves that own a panel row factor the block (and the wave of tid 0, which writes Lk)
    if ((tid & ~63) < max(m + RHS, 1)) {
      float l[6][6], li[6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) l[i][j] = A[(c0 + i) * ld + c0 + j];
      bool bad = false;
#pragma unroll
      for (int j = 0; j < 6; j++) {
        float d = l[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d = __builtin_fmaf(-l[j][k], l[j][k], d);
        bad |= !(d > 0.0f);
        li[j] = __builtin_amdgcn_rsqf(d);          // v_rsq_f32, 1 ulp; d is O(1..1e6) here, no denormal range
        l[j][j] = d * li[j];
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
          float t = l[i][j];
#pragma unroll
          for (int k = 0; k < j; k++) t = __builtin_fmaf(-l[i][k], l[j][k], t);
          l[i][j] = t * li[j];
        }
      }
      if (tid == 0) {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j <= i; j++) Lk[kb * 28 + q++] = l[i][j];
#pragma unroll
        for (int j = 0; j < 6; j++) Lk[kb * 28 + 21 + j] = li[j];
        if (bad) *s_bad = 1;
      }
      // panel: rows below the block (the rhs row among them): X L_kk' = A_ik  ->  forward substitution along the row
      for (int i = r0 + tid; i < n6 + RHS; i += nt) {
        float x[6];
#pragma unroll
        for (int j = 0; j < 6; j++) x[j] = A[i * ld + c0 + j];
#pragma unroll
        for (int j = 0; j < 6; j++) {
#pragma unroll
          for (int k = 0; k < j; k++) x[j] = __builtin_fmaf(-x[k], l[j][k], x[j]);
          x[j] *= li[j];
        }
#pragma unroll
        for (int j = 0; j < 6; j++) A[i * ld + c0 + j] = x[j];
      }
    }
    __syncthreads();
    // trailing update: A[i][j] -= sum_k L[i][c0+k] L[j][c0+k],  r0 <= j <= i < n6 + RHS,  j < n6
    for (int ii = ty; ii < m + RHS; ii += BA_TG) {
      float ri[6];
#pragma unroll
      for (int k = 0; k < 6; k++) ri[k] = A[(r0 + ii) * ld + c0 + k];
      const int jmax = RHS ? min(ii, m - 1) : ii;    // (the rhs row stops in front of its own column)
      for (int jj = tx; jj <= jmax; jj += BA_TG) {
        const float *rj = A + (r0 + jj) * ld + c0;
        float t = A[(r0 + ii) * ld + r0 + jj];
#pragma unroll
        for (int k = 0; k < 6; k++) t = __builtin_fmaf(-ri[k], rj[k], t);
        A[(r0 + ii) * ld + r0 + jj] = t;
      }
    }
    __syncthreads();
  }
}

// the solve on a matrix that is already in LDS (A: (n6 + 1) x ld, lower triangle + the rhs as row n6; every thread of the
// workgroup calls it)
__device__ __forceinline__ void ba_cholb_body(float *__restrict__ A, float *__restrict__ xv, float *__restrict__ Lk,
                                              float *__restrict__ dX, int32_t *__restrict__ info, int n6) {
  const int ld = n6 + 1;
  __shared__ int s_bad;
  const int tid = threadIdx.x, nt = BA_TG * BA_TG;
  const int nb = n6 / 6;
  ba_chol_factor<1>(A, Lk, &s_bad, n6);
  const bool bad = s_bad != 0;
  if (bad && tid == 0 && info) atomicOr(info, 1);
  // L' x = z (z = row n6), block by block from the bottom
  if (n6 <= 64) {
    // one wave, no barriers: lane i keeps z_i; a block's six unknowns are solved by every lane (uniform work on broadcast
    // values), then lane i < c0 takes them out of its z_i -- per z_i the fma chain of the blocked loop below
    if (tid < 64) {
      float z = tid < n6 ? A[n6 * ld + tid] : 0.0f;
      for (int kb = nb - 1; kb >= 0; kb--) {
        const int c0 = 6 * kb;
        float lk[27], x[6];
#pragma unroll
        for (int q = 0; q < 27; q++) lk[q] = Lk[kb * 28 + q];
#pragma unroll
        for (int j = 0; j < 6; j++) x[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), c0 + j));
#pragma unroll
        for (int j = 5; j >= 0; j--) {
#pragma unroll
          for (int k = j + 1; k < 6; k++) x[j] = __builtin_fmaf(-lk[k * (k + 1) / 2 + j], x[k], x[j]);
          x[j] *= lk[21 + j];
        }
        if (tid == 0) {
#pragma unroll
          for (int j = 0; j < 6; j++) xv[c0 + j] = x[j];
        }
        if (tid < c0) {
#pragma unroll
          for (int k = 0; k < 6; k++) z = __builtin_fmaf(-A[(c0 + k) * ld + tid], x[k], z);
        }
      }
    }
    __syncthreads();
  } else
  for (int kb = nb - 1; kb >= 0; kb--) {
    const int c0 = 6 * kb;
    if (tid < 64) {                            // wave 0 (uniform work, lane 0 writes)
      float lk[27], x[6];
#pragma unroll
      for (int q = 0; q < 27; q++) lk[q] = Lk[kb * 28 + q];
#pragma unroll
      for (int j = 0; j < 6; j++) x[j] = A[n6 * ld + c0 + j];
#pragma unroll
      for (int j = 5; j >= 0; j--) {
#pragma unroll
        for (int k = j + 1; k < 6; k++) x[j] = __builtin_fmaf(-lk[k * (k + 1) / 2 + j], x[k], x[j]);
        x[j] *= lk[21 + j];
      }
      if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 6; j++) xv[c0 + j] = x[j];
      }
    }
    __syncthreads();
    for (int i = tid; i < c0; i += nt) {       // z_i -= sum_k L[c0+k][i] x[c0+k]
      float t = A[n6 * ld + i];
#pragma unroll
      for (int k = 0; k < 6; k++) t = __builtin_fmaf(-A[(c0 + k) * ld + i], xv[c0 + k], t);
      A[n6 * ld + i] = t;
    }
    __syncthreads();
  }
  // a failed factorisation -- or a step that is not finite: a vanishing pivot passes the sign test -- drops the pose
  // step (dX = 0: the reference's torch.linalg.cholesky would throw inside its try, Ramp_vo.py:302-306); bit 0 of *info either way
  __shared__ int s_nf;
  if (tid == 0) s_nf = 0;
  __syncthreads();
  for (int q = tid; q < n6; q += nt)
    if (!(fabsf(xv[q]) <= 3.0e38f)) s_nf = 1;
  __syncthreads();
  const bool drop = bad || s_nf != 0;
  if (!bad && s_nf != 0 && tid == 0 && info) atomicOr(info, 1);
  for (int q = tid; q < n6; q += nt) dX[q] = drop ? 0.0f : xv[q];
}
__global__ void __launch_bounds__(BA_TG * BA_TG)
    ba_cholb_kernel(const float *__restrict__ S, const float *__restrict__ yv,
                    float *__restrict__ dX, int32_t *__restrict__ info, int n6) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int ld = n6 + 1;                       // odd for every 6N: conflict-free column walks
  float *A = sm;                               // (n6 + 1) x ld: rows 0..n6-1 = S (lower triangle), row n6 = y
  float *xv = sm + (n6 + 1) * ld;              // n6: solution
  float *Lk = xv + n6;                         // nb x 28: the factored diagonal blocks (21 lower entries + 6 inverses)
  ba_stage_S(A, S, n6, ld);
  for (int q = threadIdx.x; q < n6; q += BA_TG * BA_TG) A[n6 * ld + q] = yv[q];
  ba_cholb_body(A, xv, Lk, dX, info, n6);
}

// ------------------------------------------------------------------ K7
__global__ void __launch_bounds__(256)
    ba_retract_kernel(float *__restrict__ poses, float *__restrict__ patches,
                      const float *__restrict__ Erow, const float *__restrict__ Qv,
                      const float *__restrict__ uv, const float *__restrict__ dX,
                      const int64_t *__restrict__ kx, const int32_t *__restrict__ ngroups,
                      int n6, int PP, int t0, int N, int depth_blocks, const int32_t *__restrict__ dyn,
                      int opt_window) {
  ba_dyn_window(dyn, opt_window, t0, N);
  if ((int)blockIdx.x >= depth_blocks) {
    // pose retraction (ba_cuda.cu:178-206)
    const int i = (blockIdx.x - depth_blocks) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float *p = poses + 7 * (size_t)(t0 + i);
    float xi[6], to[3] = {p[0], p[1], p[2]}, qo[4] = {p[3], p[4], p[5], p[6]}, tn[3], qn[4];
#pragma unroll
    for (int c = 0; c < 6; c++) xi[c] = dX[6 * i + c];
    fb_retrSE3(xi, to, qo, tn, qn);
    p[0] = tn[0]; p[1] = tn[1]; p[2] = tn[2];
    p[3] = qn[0]; p[4] = qn[1]; p[5] = qn[2]; p[6] = qn[3];
    return;
  }
  // depth retraction (ba_cuda.cu:209-229), one wavefront per patch
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int g = blockIdx.x * (blockDim.x / 64) + wave;
  if (g >= *ngroups) return;
  float s = 0.0f;
  for (int a = lane; a < n6; a += 64) s += Erow[(size_t)g * n6 + a] * dX[a];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  s = __shfl(s, 0, 64);
  const float dz = Qv[g] * (uv[g] - s);
  float *pt = patches + ((size_t)kx[g] * 3 + 2) * PP;
  float dd = pt[0];
  dd = dd + dz;
  dd = (dd > 20) ? 1.0f : dd;
  dd = fmaxf(dd, 1e-4f);
  // every lane has read pt[0] (same address) before any lane stores
  if (lane < PP) pt[lane] = dd;
}

// ------------------------------------------------------------------ uncertainty of the window (ramp_ba_covariance)
// cov = S^-1 and depth_var_k = Q_k + Q_k^2 |L^-1 e_k|^2 from the system K1 .. K5 assemble (S = L L', damping included: the
// system the step is solved with).  Two kernels of their own:
//   C1  one workgroup: S in LDS (ld = n6 + 1), K6's factorisation (ba_chol_factor without the right-hand side row: the
//       same function, so the same L), then L^-1 IN PLACE, block row by block row from the top: row block I of L^-1 is
//       -L_II^-1 (L_I,<I  X_<I) with X_<I the rows already inverted above it -- one thread per column keeps the six sums in
//       registers (the L row block is read as LDS broadcasts, the X column walk is conflict-free with the odd ld), a barrier,
//       then the rows are overwritten.  n6 (n6 + 1) + 28 n6 / 6 floats: 148 KB at n6 = 192, inside the 160 KB of a CU.
//   C2  many workgroups: cov = L^-T L^-1 on 16 x 16 tiles of the lower triangle (both triangles written from ONE value: the
//       matrix is symmetric bit for bit), one wave per patch for v = L^-1 e_k (coalesced rows of the transposed copy) and
//       the patch's chi2 / valid-factor partial over its edge segment, summed in segment order
//   C3  one workgroup: chi2 and the valid count from the per-patch partials, in group order
// No float atomics; every sum is an fma chain or an ordered sum: the outputs are the same bits from call to call.
__global__ void __launch_bounds__(BA_TG * BA_TG)
    ba_cholinv_kernel(const float *__restrict__ S, float *__restrict__ Linv, float *__restrict__ LinvT,
                      int32_t *__restrict__ flag, int32_t *__restrict__ info, int n6) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int ld = n6 + 1;                       // odd for every 6N: conflict-free column walks
  float *A = sm;                               // n6 x ld
  float *Lk = sm + n6 * ld;                    // nb x 28: the factored diagonal blocks (21 lower entries + 6 inverses)
  __shared__ int s_bad, s_nf;
  const int tid = threadIdx.x, nt = BA_TG * BA_TG;
  const int nb = n6 / 6;
  ba_stage_S(A, S, n6, ld);
  if (tid == 0) s_nf = 0;
  ba_chol_factor<0>(A, Lk, &s_bad, n6);
  // ---- X = L^-1 in place, block row by block row
  for (int kb = 0; kb < nb; kb++) {
    const int c0 = 6 * kb;
    float xd[6][6], x[6];
    const bool work = (tid & ~63) < c0 + 6;      // whole waves: columns [0, c0) and the diagonal block's writer (tid < 6)
    if (work) {
      float lk[21], li[6];
#pragma unroll
      for (int q = 0; q < 21; q++) lk[q] = Lk[kb * 28 + q];
#pragma unroll
      for (int q = 0; q < 6; q++) li[q] = Lk[kb * 28 + 21 + q];
      // the 6 x 6 inverse of the diagonal block (every thread: uniform work on broadcast values)
#pragma unroll
      for (int c = 0; c < 6; c++) {
#pragma unroll
        for (int r = 0; r < 6; r++) {
          if (r < c) { xd[r][c] = 0.0f; continue; }
          if (r == c) { xd[r][c] = li[r]; continue; }
          float t = 0.0f;
#pragma unroll
          for (int q = c; q < r; q++) t = __builtin_fmaf(lk[r * (r + 1) / 2 + q], xd[q][c], t);
          xd[r][c] = -t * li[r];
        }
      }
      if (tid < c0) {
        float t[6] = {0, 0, 0, 0, 0, 0};
        for (int k = tid & ~63; k < c0; k++) {       // (wave-uniform bounds: the L row block is read as broadcasts)
          const float xk = k >= tid ? A[k * ld + tid] : 0.0f;
#pragma unroll
          for (int r = 0; r < 6; r++) t[r] = __builtin_fmaf(A[(c0 + r) * ld + k], xk, t[r]);
        }
#pragma unroll
        for (int r = 0; r < 6; r++) {
          float a = 0.0f;
#pragma unroll
          for (int q = 0; q <= r; q++) a = __builtin_fmaf(xd[r][q], t[q], a);
          x[r] = -a;
        }
      }
    }
    __syncthreads();
    if (work) {
      if (tid < c0) {
#pragma unroll
        for (int r = 0; r < 6; r++) A[(c0 + r) * ld + tid] = x[r];
      }
      if (tid < 6) {
#pragma unroll
        for (int r = 0; r < 6; r++) {
          float v = 0.0f;
#pragma unroll
          for (int c = 0; c < 6; c++) v = (c == tid) ? xd[r][c] : v;
          A[(c0 + r) * ld + c0 + tid] = v;
        }
      }
    }
    __syncthreads();
  }
  // ---- out: L^-1 and its transpose, zeros above / below the diagonal; a failed factorisation or an inverse that is not
  // finite raises the flag (C2 then writes NaN, never a plausible number) and bit 0 of *info, as the solver does
  for (int q = tid; q < n6 * n6; q += nt) {
    const int r = q / n6, c = q - r * n6;
    const float v = c <= r ? A[r * ld + c] : 0.0f;
    if (!(fabsf(v) <= 3.0e38f)) s_nf = 1;
    Linv[q] = v;
    LinvT[(size_t)c * n6 + r] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const int bad = (s_bad | s_nf) != 0;
    *flag = bad;
    if (bad && info) atomicOr(info, 1);
  }
}

#define BA_CT 16      // cov tile
__global__ void __launch_bounds__(256)
    ba_cov_expand_kernel(const float *__restrict__ Linv, const float *__restrict__ LinvT, const int32_t *__restrict__ flag,
                         const float *__restrict__ Erow, const float *__restrict__ Qv, const int64_t *__restrict__ kx,
                         const int32_t *__restrict__ order_k, const int32_t *__restrict__ seg_k,
                         const int32_t *__restrict__ ngroups, BaEdgeIn ein, float *__restrict__ cov,
                         float *__restrict__ depth_var, float *__restrict__ cpart, int32_t *__restrict__ npart, int n6,
                         int tiles, int max_groups, const int32_t *__restrict__ dyn, int opt_window) {
  const int tid = threadIdx.x;
  const bool bad = *flag != 0;
  const float qnan = __int_as_float(0x7fc00000);
  if ((int)blockIdx.x < tiles * tiles) {
    const int bi = blockIdx.x / tiles, bj = blockIdx.x - bi * tiles;
    if (bj > bi) return;
    const int i = bi * BA_CT + tid / BA_CT, j = bj * BA_CT + tid % BA_CT;
    if (i >= n6 || j > i) return;
    float c = 0.0f;
    for (int k = i; k < n6; k++) c = __builtin_fmaf(Linv[(size_t)k * n6 + i], Linv[(size_t)k * n6 + j], c);
    if (bad) c = qnan;
    cov[(size_t)i * n6 + j] = c;
    cov[(size_t)j * n6 + i] = c;
    return;
  }
  ba_dyn_window(dyn, opt_window, ein.t0, ein.N);
  const int wave = tid / 64, lane = tid % 64;
  const int g = (blockIdx.x - tiles * tiles) * 4 + wave;
  if (g >= min(*ngroups, max_groups)) return;    // (max_groups: the rows of Erow / cpart the caller's bound gave room for)
  // v = L^-1 e_k: lane i keeps rows i, i + 64, i + 128 (n6 <= 192); column a of L^-1 is row a of the transposed copy
  float v[3] = {0, 0, 0};
  for (int a = 0; a < n6; a++) {
    const float ea = Erow[(size_t)g * n6 + a];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int i = lane + 64 * q;
      if (i < n6) v[q] = __builtin_fmaf(ea, LinvT[(size_t)a * n6 + i], v[q]);
    }
  }
  float s = v[0] * v[0];
  s = __builtin_fmaf(v[1], v[1], s);
  s = __builtin_fmaf(v[2], v[2], s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  s = __shfl(s, 0, 64);
  // the patch's part of chi2 = sum_valid (w0 rx^2 + w1 ry^2) and of the valid count, in segment order
  const int s0 = seg_k[g], s1 = seg_k[g + 1];
  float chi = 0.0f;
  int cnt = 0;
  for (int b0 = s0; b0 < s1; b0 += 64) {
    const int nb = min(64, s1 - b0);
    float term = 0.0f, gate = 0.0f;
    if (lane < nb) {
      float r[BA_REC];
      ba_edge_compute_gate(ein, order_k[b0 + lane], r, gate);
      const float tx_ = (r[R_W0] * r[R_R0]) * r[R_R0], ty_ = (r[R_W1] * r[R_R1]) * r[R_R1];
      term = gate != 0.0f ? tx_ + ty_ : 0.0f;        // (a gated factor's residual may be inf / NaN)
    }
    cnt += __popcll(__ballot(gate != 0.0f));
    for (int l = 0; l < nb; l++) chi += __shfl(term, l, 64);
  }
  if (lane == 0) {
    const float q = Qv[g];
    cpart[g] = chi;
    npart[g] = cnt;
    depth_var[kx[g]] = bad ? qnan : __builtin_fmaf(q * q, s, q);     // Q + Q^2 |L^-1 e|^2: cannot go below Q
  }
}

// stats words: [0] chi2 (float), [1] valid factors, [2] Mu, [3] N (free poses), [4] t0, [5] 1 = factorisation failed -- [1] ..
// [5] int32 bit patterns -- [6], [7] zero
__global__ void __launch_bounds__(256)
    ba_cov_stats_kernel(const float *__restrict__ cpart, const int32_t *__restrict__ npart,
                        const int32_t *__restrict__ ngroups, const int32_t *__restrict__ flag, float *__restrict__ stats,
                        int t0, int N, int max_groups, const int32_t *__restrict__ dyn, int opt_window) {
  __shared__ float s_c[256];
  __shared__ int s_n[256];
  ba_dyn_window(dyn, opt_window, t0, N);
  const int tid = threadIdx.x, nk = min(*ngroups, max_groups);
  const int per = (nk + 255) / 256;
  float c = 0.0f;
  int n = 0;
  for (int g = tid * per; g < min(nk, (tid + 1) * per); g++) { c += cpart[g]; n += npart[g]; }
  s_c[tid] = c; s_n[tid] = n;
  __syncthreads();
  if (tid == 0) {
    float ct = 0.0f;
    int nt = 0;
    for (int q = 0; q < 256; q++) { ct += s_c[q]; nt += s_n[q]; }
    stats[0] = ct;
    stats[1] = __int_as_float(nt);
    stats[2] = __int_as_float(nk);
    stats[3] = __int_as_float(N > 0 ? N : 0);
    stats[4] = __int_as_float(t0);
    stats[5] = __int_as_float(*flag != 0 ? 1 : 0);
    stats[6] = 0.0f; stats[7] = 0.0f;
  }
}

// ------------------------------------------------------------------ C4: the map (ramp_ba_map_covariance)
// One wave per patch group, behind C2 / C3 (it reads what they wrote: cov, depth_var, npart -- their outputs are the same bits
// with or without this stage).  For patch k with source frame i (the ii of its factors), a = i - t0:
//   v = L^-1 e_k as C2 forms it; w = (L^-T v)[6a .. 6a+5] from six rows of the transposed copy (lane-strided fma chains, then
//   the wave's fixed shuffle tree); c = cov(xi_i, z_k) = -Q_k w
//   the point X_w = R' (r / d - t): csrc/lie.hip::point_cloud_block's expressions with the intrinsics of row 0 (the row the
//   system is built with), so the same bits wherever every row is equal
//   J_p = R' [-I | [r / d]x],  J_d = -R' r / d^2  (left perturbation T <- Exp(xi) T, xi = (translation, rotation); d <- d + z)
//   Sigma = J_p cov_aa J_p' + var(z_k) J_d J_d' + (J_p c) J_d' + J_d (J_p c)'   -- six entries, each from ONE value
// A source frame outside [t0, t1) is fixed: c = 0 and Sigma = var(z_k) J_d J_d'.  No atomics; fma chains and fixed trees only.
__global__ void __launch_bounds__(256)
    ba_map_kernel(const float *__restrict__ LinvT, const int32_t *__restrict__ flag, const float *__restrict__ Erow,
                  const float *__restrict__ Qv, const int64_t *__restrict__ kx, const int32_t *__restrict__ order_k,
                  const int32_t *__restrict__ seg_k, const int32_t *__restrict__ ngroups, BaEdgeIn ein,
                  const float *__restrict__ cov, const float *__restrict__ depth_var, const int32_t *__restrict__ npart,
                  BaMapOut out, int n6, int max_groups, const int32_t *__restrict__ dyn, int opt_window) {
  ba_dyn_window(dyn, opt_window, ein.t0, ein.N);
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int g = blockIdx.x * 4 + wave;
  if (g >= min(*ngroups, max_groups)) return;
  const bool bad = *flag != 0;
  const float qnan = __int_as_float(0x7fc00000);
  const long k = kx[g];
  const int src = (int)ein.ii[order_k[seg_k[g]]];
  const int a = src - ein.t0;
  const bool is_free = a >= 0 && a < ein.N && 6 * a + 6 <= n6;      // (wave-uniform)
  float w6[6] = {0, 0, 0, 0, 0, 0};
  if (is_free) {
    float v[3] = {0, 0, 0};
    for (int b = 0; b < n6; b++) {
      const float eb = Erow[(size_t)g * n6 + b];
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int i = lane + 64 * q;
        if (i < n6) v[q] = __builtin_fmaf(eb, LinvT[(size_t)b * n6 + i], v[q]);
      }
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
      const float *row = LinvT + (size_t)(6 * a + r) * n6;          // column 6a + r of L^-1 (zero above the diagonal)
      float s = 0.0f;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int i = lane + 64 * q;
        if (i < n6) s = __builtin_fmaf(row[i], v[q], s);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      w6[r] = __shfl(s, 0, 64);
    }
  }
  if (lane != 0) return;
  // ---- the point (point_cloud_block's statements)
  float T[7], Tinv[7], t[3], q[4];
#pragma unroll
  for (int c = 0; c < 7; c++) T[c] = ein.poses[7 * (size_t)src + c];
  lt_inv(T, Tinv);
  lt_load(Tinv, t, q);
  const float *pt = ein.patches + (size_t)k * 3 * ein.PP;
  float X0[4], X1[4];
  X0[0] = (pt[ein.c11] - ein.intr[2]) / ein.intr[0];
  X0[1] = (pt[ein.PP + ein.c11] - ein.intr[3]) / ein.intr[1];
  X0[2] = 1.0f;
  X0[3] = pt[2 * ein.PP + ein.c11];
  lt_act4_tq(t, q, X0, X1);
  out.point[3 * (size_t)k + 0] = X1[0] / X1[3];
  out.point[3 * (size_t)k + 1] = X1[1] / X1[3];
  out.point[3 * (size_t)k + 2] = X1[2] / X1[3];
  out.n_obs[k] = npart[g];
  // ---- Jacobians: Rt = R' (the rotation of the inverse pose), pc = r / d
  float Rt[9];
  lt_q2R(q, Rt);
  const float id = 1.0f / X0[3];
  const float pc[3] = {X0[0] * id, X0[1] * id, id};
  float Jp[3][6], Jd[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float r0 = Rt[3 * i], r1 = Rt[3 * i + 1], r2 = Rt[3 * i + 2];
    Jp[i][0] = -r0; Jp[i][1] = -r1; Jp[i][2] = -r2;
    Jp[i][3] = __builtin_fmaf(r1, pc[2], -(r2 * pc[1]));
    Jp[i][4] = __builtin_fmaf(r2, pc[0], -(r0 * pc[2]));
    Jp[i][5] = __builtin_fmaf(r0, pc[1], -(r1 * pc[0]));
    const float rr = __builtin_fmaf(r1, X0[1], __builtin_fmaf(r0, X0[0], r2));      // (R' r)_i with r_z = 1
    Jd[i] = -rr * (id * id);
  }
  const float var = depth_var[k];
  float P6[6] = {0, 0, 0, 0, 0, 0}, m[3] = {0, 0, 0}, c[6] = {0, 0, 0, 0, 0, 0};
  if (is_free) {
    const float qk = Qv[g];
#pragma unroll
    for (int r = 0; r < 6; r++) c[r] = -qk * w6[r];
    float A[3][6];
#pragma unroll
    for (int y = 0; y < 6; y++) {
      float col[6];
#pragma unroll
      for (int x = 0; x < 6; x++) col[x] = cov[(size_t)(6 * a + x) * n6 + 6 * a + y];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        float s = 0.0f;
#pragma unroll
        for (int x = 0; x < 6; x++) s = __builtin_fmaf(Jp[i][x], col[x], s);
        A[i][y] = s;
      }
    }
    int e = 0;
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
      for (int y = x; y < 3; y++) {
        float s = 0.0f;
#pragma unroll
        for (int z = 0; z < 6; z++) s = __builtin_fmaf(A[x][z], Jp[y][z], s);
        P6[e++] = s;
      }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      float s = 0.0f;
#pragma unroll
      for (int z = 0; z < 6; z++) s = __builtin_fmaf(Jp[i][z], c[z], s);
      m[i] = s;
    }
  }
  int e = 0;
#pragma unroll
  for (int x = 0; x < 3; x++)
#pragma unroll
    for (int y = x; y < 3; y++) {
      float s = var * (Jd[x] * Jd[y]);
      s = __builtin_fmaf(m[x], Jd[y], s);
      s = __builtin_fmaf(Jd[x], m[y], s);
      s += P6[e];
      out.point_cov[6 * (size_t)k + e] = bad ? qnan : s;
      e++;
    }
#pragma unroll
  for (int r = 0; r < 6; r++) out.pose_depth_cov[6 * (size_t)k + r] = bad ? qnan : c[r];
}

// ramp_map_select: stable stream compaction of the points that pass the thresholds -- ONE workgroup walks the patches in
// chunks of its size; per chunk a ballot per wave, the waves' counts in wave order, the running base: the indices come out
// ascending whatever the launch geometry, and the count lands in a device word.
#define BA_SEL_THREADS 1024
__global__ void __launch_bounds__(BA_SEL_THREADS)
    map_select_kernel(const float *__restrict__ point_cov, const float *__restrict__ depth_var,
                      const float *__restrict__ patches, const int32_t *__restrict__ n_obs, int n, int PP, int ctr,
                      const int32_t *__restrict__ dyn_rows, int per_row, float max_sigma, float max_rel, int min_obs,
                      int32_t *__restrict__ index, int32_t *__restrict__ count) {
  __shared__ int s_wcnt[BA_SEL_THREADS / 64];
  __shared__ int s_base;
  if (dyn_rows) n = min(n, max(*dyn_rows, 0) * per_row);        // device-side size: the argument is the capacity
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inf = __int_as_float(0x7f800000);
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += BA_SEL_THREADS) {
    const int i = i0 + tid;
    bool hit = false;
    if (i < n) {
      const float *pc = point_cov + 6 * (size_t)i;
      bool fin = true;
#pragma unroll
      for (int e = 0; e < 6; e++) fin = fin && (fabsf(pc[e]) < inf);
      const float sig = sqrtf((pc[0] + pc[3]) + pc[5]);
      const float rel = sqrtf(depth_var[i]) / patches[((size_t)i * 3 + 2) * PP + ctr];
      hit = fin && (max_sigma == inf || sig <= max_sigma) && (max_rel == inf || rel <= max_rel) &&
            (min_obs <= 0 || n_obs[i] >= min_obs);
    }
    const unsigned long long mk = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(mk);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; w++) off += s_wcnt[w];
    off += __popcll(mk & ((1ull << lane) - 1ull));
    if (hit) index[off] = i;
    __syncthreads();
    if (tid == 0) {
      int t = s_base;
      for (int w = 0; w < BA_SEL_THREADS / 64; w++) t += s_wcnt[w];
      s_base = t;
    }
    __syncthreads();
  }
  if (tid == 0) *count = s_base;
}

__global__ void ba_pairkey_kernel(const int64_t *__restrict__ ii, const int64_t *__restrict__ jj,
                                  int64_t *__restrict__ keys, int E, long long np) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < E) keys[n] = jj[n] * np + ii[n];   // target-frame-major, as the tracker's graph plan
}

// ------------------------------------------------------------- host driver
struct BaWs {
  void *gb; size_t gb_bytes;
  int64_t *pkeys, *kx, *pukeys;
  int32_t *order_k, *seg_k, *order_p, *seg_p, *pair_ij, *counters;
  float *rec, *Erow, *Cv, *uv, *Qv, *pairs, *S_part, *y_part, *S, *yv, *dX;
  int Mu_b, Gp_b, KS, tiles;
};
// own_groups: carve room for this call's own group-by (ramp_ba_forward); otherwise the groups
// come from the caller's plan (ramp_ba_forward_planned) and Mu_b / Gp_b are the caller's bounds.
static size_t ba_carve(void *ws, int E, int n_poses, int n_patches, int N, int own_groups,
                       int max_patches, int max_pairs, BaWs *w) {
  const size_t e = (size_t)(E > 0 ? E : 1);
  const int n6 = 6 * N;
  WsCarver c(ws);
  w->Mu_b = (int)((size_t)n_patches < e ? (size_t)n_patches : e);
  if (max_patches > 0 && max_patches < w->Mu_b) w->Mu_b = max_patches;
  if (w->Mu_b < 1) w->Mu_b = 1;
  const size_t pp = (size_t)n_poses * (size_t)n_poses;
  w->Gp_b = (int)(pp < e ? pp : e);
  if (max_pairs > 0 && max_pairs < w->Gp_b) w->Gp_b = max_pairs;
  if (w->Gp_b < 1) w->Gp_b = 1;
  w->tiles = (n6 + BA_TS - 1) / BA_TS;
  if (w->tiles < 1) w->tiles = 1;
  int ks = 256 / (w->tiles * w->tiles);
  w->KS = ks < 4 ? 4 : (ks > 64 ? 64 : ks);   // split-K partials, summed in fixed order by K5
  w->gb = nullptr; w->gb_bytes = 0;
  w->pkeys = w->kx = w->pukeys = nullptr;
  w->order_k = w->seg_k = w->order_p = w->seg_p = nullptr;
  if (own_groups) {
    w->gb_bytes = ramp_internal_group_by_ws(E);
    w->gb = c.take<char>(w->gb_bytes, 256);
    w->pkeys = c.take<int64_t>(e, 256);
    w->kx = c.take<int64_t>(e, 256);
    w->pukeys = c.take<int64_t>(e, 256);
    w->order_k = c.take<int32_t>(e, 256);
    w->seg_k = c.take<int32_t>(e + 1, 256);
    w->order_p = c.take<int32_t>(e, 256);
    w->seg_p = c.take<int32_t>(e + 1, 256);
  }
  w->pair_ij = c.take<int32_t>((size_t)w->Gp_b * 2, 256);
  w->counters = c.take<int32_t>(16, 256);
  w->rec = c.take<float>(e * BA_REC, 256);
  w->Erow = c.take<float>((size_t)w->Mu_b * (n6 > 0 ? n6 : 1), 256);
  w->Cv = c.take<float>((size_t)w->Mu_b, 256);
  w->uv = c.take<float>((size_t)w->Mu_b, 256);
  w->Qv = c.take<float>((size_t)w->Mu_b, 256);
  w->pairs = c.take<float>((size_t)w->Gp_b * BA_PAIR, 256);
  w->S_part = c.take<float>((size_t)w->KS * (n6 * n6 + 1), 256);
  w->y_part = c.take<float>((size_t)w->KS * (n6 + 1), 256);
  w->S = c.take<float>((size_t)(n6 * n6 + 1), 256);
  w->yv = c.take<float>((size_t)(n6 + 1), 256);
  w->dX = c.take<float>((size_t)(n6 + 1), 256);
  return c.bytes();
}

static BaEdgeIn ba_edge_in(const BaProblem &p) {
  BaEdgeIn e;
  e.poses = p.poses; e.patches = p.patches; e.intr = p.intrinsics; e.target = p.target; e.weight = p.weight;
  e.ii = p.ii; e.jj = p.jj; e.kk = p.kk; e.PP = p.P * p.P; e.c11 = 1 * p.P + 1; e.t0 = p.t0; e.N = p.t1 - p.t0;
  return e;
}

// the single-workgroup kernels keep their matrix in LDS (ramp_launch_lds); a window whose matrix exceeds a CU's 160 KB is refused
constexpr size_t BA_LDS_MAX = 160 * 1024;

// K1 .. K5: the system at the state p.  E row, C, u, Q per patch; with free poses also the pair records, the split-K
// partials and S, y (w.S, w.yv).  The solver runs it once per iteration, the covariance once.
static int ba_build_system(const BaProblem &p, const BaGroups &g, BaWs &w, int32_t *info, hipStream_t st) {
  const int N = p.t1 - p.t0, n6 = 6 * N;
  const int pthreads = ((n6 + 2 + 63) / 64) * 64;      // a patch's workgroup: one thread per column of its E row, C and u
  if (pthreads > 256) return RAMP_EUNSUPPORTED;
  const BaEdgeIn ein = ba_edge_in(p);
  if (N <= 0) {
    // no free pose: only K2 has anything to do, on records that go through memory
    hipLaunchKernelGGL(ba_edge_kernel, dim3(ramp_cdiv(p.E, 256)), dim3(256), 0, st, ein, w.rec, p.E, p.dyn, p.opt_window);
    hipLaunchKernelGGL(ba_patch_kernel, dim3(w.Mu_b), dim3(pthreads), 0, st, w.rec, g.order_k, g.seg_k, g.ngroups_k,
                       p.lmbda, w.Erow, w.Cv, w.uv, w.Qv, n6);
    return RAMP_OK;
  }
  hipLaunchKernelGGL(ba_patch_pair_kernel, dim3(w.Mu_b + w.Gp_b), dim3(256), 0, st, w.Mu_b, g.order_k, g.seg_k,
                     g.ngroups_k, p.lmbda, w.Erow, w.Cv, w.uv, w.Qv, n6, g.order_p, g.seg_p, g.ngroups_p, w.pairs,
                     w.pair_ij, ein, p.dyn, p.opt_window);
  // (one workgroup per split-K slice where the system is a single tile; N x N assembly workgroups up to 16 poses, one per
  // pose above -- the interleaved order of the former moves a 180 x 180 solve by 6e-4 of the step)
  if (w.tiles == 1 && ramp_cdiv(w.Mu_b, w.KS) <= BA_S1_ROWS)
    hipLaunchKernelGGL(ba_schur1_kernel, dim3(1, 1, w.KS), dim3(256), 0, st, w.Erow, w.Qv, w.uv, g.ngroups_k, w.S_part,
                       w.y_part, n6, w.KS);
  else
    hipLaunchKernelGGL(ba_schur_kernel, dim3(w.tiles, w.tiles, w.KS), dim3(256), 0, st, w.Erow, w.Qv, w.uv, g.ngroups_k,
                       w.S_part, w.y_part, n6, w.KS);
  if (N <= 16)
    hipLaunchKernelGGL(ba_assemble2_kernel, dim3(N, N), dim3(256), 0, st, w.pairs, w.pair_ij, g.ngroups_p, w.S_part,
                       w.y_part, w.S, w.yv, n6, w.KS, info);
  else
    hipLaunchKernelGGL(ba_assemble_kernel, dim3(N, ramp_cdiv(6 * n6, 192)), dim3(256), 0, st, w.pairs, w.pair_ij,
                       g.ngroups_p, w.S_part, w.y_part, w.S, w.yv, n6, w.KS, info);
  return RAMP_OK;
}

// the GN iterations, given the two groupings
static int ba_iterate(const BaProblem &p, const BaGroups &g, int iterations, BaWs &w, int32_t *info, hipStream_t st) {
  const int N = p.t1 - p.t0, n6 = 6 * N;
  const size_t lds = (size_t)((n6 + 1) * (n6 + 1) + 6 * n6) * sizeof(float);
  if (lds > BA_LDS_MAX) return RAMP_EUNSUPPORTED;
  int rc;
  const int depth_blocks = ramp_cdiv(w.Mu_b, 4);
  const int pose_blocks = N > 0 ? ramp_cdiv(N, 256) : 0;
  for (int itr = 0; itr < iterations; itr++) {
    if ((rc = ba_build_system(p, g, w, info, st)) != RAMP_OK) return rc;
    if (N > 0 && (rc = ramp_launch_lds(ba_cholb_kernel, dim3(1), dim3(BA_TG * BA_TG), lds, st, w.S, w.yv, w.dX, info, n6)) != RAMP_OK)
      return rc;
    hipLaunchKernelGGL(ba_retract_kernel, dim3(depth_blocks + pose_blocks), dim3(256), 0, st, p.poses, p.patches, w.Erow,
                       w.Qv, w.uv, w.dX, g.ukeys_k, g.ngroups_k, n6, p.P * p.P, p.t0, N, depth_blocks, p.dyn, p.opt_window);
    RAMP_CHECK_LAUNCH();
  }
  return RAMP_OK;
}

// ---- uncertainty: the system of ONE iteration at the state passed in, no step taken (nothing retracts)
struct BaCovWs { float *Linv, *LinvT, *cpart; int32_t *npart, *flag; };
// what a covariance call writes; ws: its own workspace (the dyn form), or nullptr: the buffers follow BA's in the call's
// map.point != nullptr: the map stage C4 runs behind C3
struct BaCovOut { float *cov, *depth_var, *stats; void *ws; size_t ws_bytes; BaMapOut map; };
// at: where the blocks start in ws -- 0 in a workspace of their own, BA's bytes behind BA's; returns where they end
static size_t ba_cov_carve(void *ws, size_t at, int n6, int Mu_b, BaCovWs *w) {
  WsCarver c(ws, at);
  w->Linv = c.take<float>((size_t)(n6 * n6 + 1), 256);
  w->LinvT = c.take<float>((size_t)(n6 * n6 + 1), 256);
  w->cpart = c.take<float>((size_t)Mu_b, 256);
  w->npart = c.take<int32_t>((size_t)Mu_b, 256);
  w->flag = c.take<int32_t>(16, 256);
  return c.bytes();
}
static int ba_cov_run(const BaProblem &p, const BaGroups &g, BaWs &w, BaCovWs &c, const BaCovOut &out, int32_t *info,
                      hipStream_t st) {
  const int N = p.t1 - p.t0, n6 = 6 * N;
  const size_t lds = (size_t)(n6 * (n6 + 1) + (n6 / 6) * 28) * sizeof(float);
  if (lds > BA_LDS_MAX) return RAMP_EUNSUPPORTED;
  int rc;
  if (hipMemsetAsync(c.flag, 0, sizeof(int32_t), st) != hipSuccess) return RAMP_ELAUNCH;
  if ((rc = ba_build_system(p, g, w, info, st)) != RAMP_OK) return rc;
  if (N > 0 &&
      (rc = ramp_launch_lds(ba_cholinv_kernel, dim3(1), dim3(BA_TG * BA_TG), lds, st, w.S, c.Linv, c.LinvT, c.flag, info, n6)) != RAMP_OK)
    return rc;
  const int tiles = ramp_cdiv(n6, BA_CT);
  hipLaunchKernelGGL(ba_cov_expand_kernel, dim3(tiles * tiles + ramp_cdiv(w.Mu_b, 4)), dim3(256), 0, st, c.Linv, c.LinvT,
                     c.flag, w.Erow, w.Qv, g.ukeys_k, g.order_k, g.seg_k, g.ngroups_k, ba_edge_in(p), out.cov,
                     out.depth_var, c.cpart, c.npart, n6, tiles, w.Mu_b, p.dyn, p.opt_window);
  hipLaunchKernelGGL(ba_cov_stats_kernel, dim3(1), dim3(256), 0, st, c.cpart, c.npart, g.ngroups_k, c.flag, out.stats,
                     p.t0, N, w.Mu_b, p.dyn, p.opt_window);
  if (out.map.point)
    hipLaunchKernelGGL(ba_map_kernel, dim3(ramp_cdiv(w.Mu_b, 4)), dim3(256), 0, st, c.LinvT, c.flag, w.Erow, w.Qv, g.ukeys_k,
                       g.order_k, g.seg_k, g.ngroups_k, ba_edge_in(p), out.cov, out.depth_var, c.npart, out.map, n6, w.Mu_b,
                       p.dyn, p.opt_window);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

// ---- what the entry points share.  plan == nullptr: the call groups its own factors (room for that is carved);
// otherwise the groups are the caller's and its bounds size Mu_b / Gp_b.  out == nullptr: solve; otherwise the
// uncertainty (one system, `iterations` is 1).
// todo = false with RAMP_OK: a valid call that has nothing to do
static int ba_check(const BaProblem &p, const BaGroups *plan, int iterations, const BaCovOut *out, const void *ws,
                    int32_t *info, hipStream_t st, bool &todo) {
  todo = false;
  if (p.dyn && (p.E <= 0 || p.opt_window <= 0 || !ws || (out && !out->ws))) return RAMP_EINVAL;
  if (p.E < 0 || p.P < 2 || p.n_poses <= 0 || p.n_patches <= 0 || iterations < 0) return RAMP_EINVAL;
  if (p.t0 < 0 || p.t1 < p.t0 || p.t1 > p.n_poses) return RAMP_EINVAL;
  const int n6 = 6 * (p.t1 - p.t0);
  if ((size_t)((n6 + 1) * (n6 + 1) + 2 * n6) * sizeof(float) > 160 * 1024) return RAMP_EUNSUPPORTED;  // > 32 free poses
  if (out && p.E == 0) return RAMP_EINVAL;
  if (info && !p.dyn) (void)hipMemsetAsync(info, 0, sizeof(int32_t), st);     // (the dyn forms accumulate their status bits)
  if (p.E == 0 || iterations == 0) return RAMP_OK;
  if (!p.poses || !p.patches || !p.intrinsics || !p.target || !p.weight || !p.lmbda || !p.ii || !p.jj || !p.kk || !ws)
    return RAMP_EINVAL;
  if (plan && (!plan->order_k || !plan->seg_k || !plan->ngroups_k || !plan->ukeys_k || !plan->order_p || !plan->seg_p ||
               !plan->ngroups_p || plan->max_patches <= 0 || plan->max_pairs <= 0))
    return RAMP_EINVAL;
  if (out && (!out->depth_var || !out->stats || (p.t1 > p.t0 && !out->cov))) return RAMP_EINVAL;
  const BaMapOut *m = out ? &out->map : nullptr;                  // the map's four outputs: all or none
  if (m && (m->point || m->point_cov || m->pose_depth_cov || m->n_obs) &&
      !(m->point && m->point_cov && m->pose_depth_cov && m->n_obs))
    return RAMP_EINVAL;
  todo = true;
  return RAMP_OK;
}

// `ws` carved for the call (the covariance's buffers behind BA's unless the call brings a workspace for them) and checked
static int ba_carve_checked(void *ws, size_t ws_bytes, const BaProblem &p, const BaGroups *plan, const BaCovOut *out,
                            BaWs &w, BaCovWs &c) {
  const int N = p.t1 - p.t0;
  size_t a = ba_carve(ws, p.E, p.n_poses, p.n_patches, N, !plan, plan ? plan->max_patches : 0, plan ? plan->max_pairs : 0, &w);
  if (out && out->ws) {
    if (ba_cov_carve(out->ws, 0, 6 * N, w.Mu_b, &c) > out->ws_bytes) return RAMP_EWORKSPACE;
  } else if (out) {
    a = ba_cov_carve(ws, a, 6 * N, w.Mu_b, &c);
  }
  return a > ws_bytes ? RAMP_EWORKSPACE : RAMP_OK;
}

// prep of a call without a plan: group by patch, group by pose pair (the pairs only matter with a free pose)
static int ba_own_groups(const BaProblem &p, const BaWs &w, BaGroups &g, hipStream_t st) {
  int32_t *nk = w.counters, *np = w.counters + 1;
  g = BaGroups{w.order_k, w.seg_k, nk, w.kx, w.order_p, w.seg_p, np, 0, 0};
  int rc = ramp_internal_group_by(p.kk, p.E, p.n_patches, w.order_k, nullptr, w.seg_k, w.kx, nk, w.gb, w.gb_bytes, st);
  if (rc != RAMP_OK || p.t1 <= p.t0) return rc;
  hipLaunchKernelGGL(ba_pairkey_kernel, dim3(ramp_cdiv(p.E, 256)), dim3(256), 0, st, p.ii, p.jj, w.pkeys, p.E,
                     (long long)p.n_poses);
  return ramp_internal_group_by(w.pkeys, p.E, (int64_t)p.n_poses * p.n_poses, w.order_p, nullptr, w.seg_p, w.pukeys, np,
                                w.gb, w.gb_bytes, st);
}

static int ba_run(const BaProblem &p, const BaGroups *plan, int iterations, const BaCovOut *out, void *ws,
                  size_t ws_bytes, int32_t *info, hipStream_t st) {
  bool todo;
  int rc = ba_check(p, plan, iterations, out, ws, info, st, todo);
  if (rc != RAMP_OK || !todo) return rc;
  BaWs w;
  BaCovWs c;
  BaGroups own;
  if ((rc = ba_carve_checked(ws, ws_bytes, p, plan, out, w, c)) != RAMP_OK) return rc;
  if (!plan && (rc = ba_own_groups(p, w, own, st)) != RAMP_OK) return rc;
  const BaGroups &g = plan ? *plan : own;
  return out ? ba_cov_run(p, g, w, c, *out, info, st) : ba_iterate(p, g, iterations, w, info, st);
}
static size_t ba_ws_bytes(int E, int n_poses, int n_patches, int N, int own_groups, int max_patches, int max_pairs, bool cov) {
  BaWs w;
  BaCovWs c;
  if (N < 0) N = 0;
  const size_t a = ba_carve(nullptr, E, n_poses, n_patches, N, own_groups, max_patches, max_pairs, &w);
  return cov ? ba_cov_carve(nullptr, a, 6 * N, w.Mu_b, &c) : a;
}

// ---- device-side sizes (csrc/track.hip): the window [max(n - opt_window, 1), n) with n = dyn[RAMP_DYN_N] and the
// factor count dyn[RAMP_DYN_E] are read by the kernels; p.E bounds the launches, the system has opt_window poses (a
// shorter window leaves identity blocks behind it; cov is [6 opt_window]^2).  Status bits accumulate in *info (not
// cleared here).  p.t0 / p.t1 are set here.
static BaProblem ba_dyn_problem(BaProblem p) {
  p.t0 = 1; p.t1 = 1 + p.opt_window;
  return p;
}
size_t ramp_i_ba_dyn_ws(int E_cap, int n_poses, int n_patches, int opt_window, int max_patches, int max_pairs) {
  return ba_ws_bytes(E_cap, n_poses, n_patches, opt_window, 0, max_patches, max_pairs, false);
}
int ramp_i_ba_dyn(const BaProblem &p, const BaGroups &g, int iterations, void *ws, size_t ws_bytes, int32_t *info,
                  hipStream_t st) {
  if (!p.dyn) return RAMP_EINVAL;
  return ba_run(ba_dyn_problem(p), &g, iterations, nullptr, ws, ws_bytes, info, st);
}
size_t ramp_i_ba_cov_dyn_ws(int opt_window, int max_patches) {
  BaCovWs c;
  return ba_cov_carve(nullptr, 0, 6 * opt_window, max_patches > 0 ? max_patches : 1, &c);
}
// ba_ws: ramp_i_ba_dyn's
int ramp_i_ba_cov_dyn(const BaProblem &p, const BaGroups &g, void *ba_ws, size_t ba_ws_bytes, void *cov_ws,
                      size_t cov_ws_bytes, int32_t *info, float *cov, float *depth_var, float *stats, hipStream_t st,
                      const BaMapOut *map) {
  if (!p.dyn || !cov_ws) return RAMP_EINVAL;
  const BaCovOut out = {cov, depth_var, stats, cov_ws, cov_ws_bytes, map ? *map : BaMapOut{}};
  return ba_run(ba_dyn_problem(p), &g, 1, &out, ba_ws, ba_ws_bytes, info, st);
}

extern "C" {

size_t ramp_ba_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1) {
  return ba_ws_bytes(E, n_poses, n_patches, t1 - t0, 1, 0, 0, false);
}

int ramp_ba_forward(float *poses, float *patches, const float *intrinsics, const float *target, const float *weight,
                    const float *lmbda, const int64_t *ii, const int64_t *jj, const int64_t *kk, int E, int P, int n_poses,
                    int n_patches, int t0, int t1, int iterations, void *ws, size_t ws_bytes, int32_t *info, void *stream) {
  const BaProblem p = {poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, E, P, n_poses, n_patches, t0, t1,
                       nullptr, 0};
  return ba_run(p, nullptr, iterations, nullptr, ws, ws_bytes, info, (hipStream_t)stream);
}

size_t ramp_ba_planned_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1, int max_patches, int max_pairs) {
  return ba_ws_bytes(E, n_poses, n_patches, t1 - t0, 0, max_patches, max_pairs, false);
}

int ramp_ba_forward_planned(float *poses, float *patches, const float *intrinsics, const float *target, const float *weight,
                            const float *lmbda, const int64_t *ii, const int64_t *jj, const int64_t *kk, int E, int P,
                            int n_poses, int n_patches, int t0, int t1, int iterations, const int32_t *order_k,
                            const int32_t *seg_k, const int32_t *ngroups_k, const int64_t *ukeys_k, int max_patches,
                            const int32_t *order_p, const int32_t *seg_p, const int32_t *ngroups_p, int max_pairs,
                            void *ws, size_t ws_bytes, int32_t *info, void *stream) {
  const BaProblem p = {poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, E, P, n_poses, n_patches, t0, t1,
                       nullptr, 0};
  const BaGroups g = {order_k, seg_k, ngroups_k, ukeys_k, order_p, seg_p, ngroups_p, max_patches, max_pairs};
  return ba_run(p, &g, iterations, nullptr, ws, ws_bytes, info, (hipStream_t)stream);
}

size_t ramp_ba_covariance_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1) {
  return ba_ws_bytes(E, n_poses, n_patches, t1 - t0, 1, 0, 0, true);
}

// (poses and patches are only read: no retraction runs)
int ramp_ba_covariance(const float *poses, const float *patches, const float *intrinsics, const float *target,
                       const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                       const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1, float *cov,
                       float *depth_var, float *stats, void *ws, size_t ws_bytes, int32_t *info, void *stream) {
  const BaProblem p = {const_cast<float *>(poses), const_cast<float *>(patches), intrinsics, target, weight, lmbda, ii, jj,
                       kk, E, P, n_poses, n_patches, t0, t1, nullptr, 0};
  const BaCovOut out = {cov, depth_var, stats, nullptr, 0, BaMapOut{}};
  return ba_run(p, nullptr, 1, &out, ws, ws_bytes, info, (hipStream_t)stream);
}

size_t ramp_ba_covariance_planned_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1, int max_patches,
                                                  int max_pairs) {
  return ba_ws_bytes(E, n_poses, n_patches, t1 - t0, 0, max_patches, max_pairs, true);
}

int ramp_ba_covariance_planned(const float *poses, const float *patches, const float *intrinsics, const float *target,
                               const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                               const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1,
                               float *cov, float *depth_var, float *stats, const int32_t *order_k,
                               const int32_t *seg_k, const int32_t *ngroups_k, const int64_t *ukeys_k, int max_patches,
                               const int32_t *order_p, const int32_t *seg_p, const int32_t *ngroups_p, int max_pairs,
                               void *ws, size_t ws_bytes, int32_t *info, void *stream) {
  const BaProblem p = {const_cast<float *>(poses), const_cast<float *>(patches), intrinsics, target, weight, lmbda, ii, jj,
                       kk, E, P, n_poses, n_patches, t0, t1, nullptr, 0};
  const BaGroups g = {order_k, seg_k, ngroups_k, ukeys_k, order_p, seg_p, ngroups_p, max_patches, max_pairs};
  const BaCovOut out = {cov, depth_var, stats, nullptr, 0, BaMapOut{}};
  return ba_run(p, &g, 1, &out, ws, ws_bytes, info, (hipStream_t)stream);
}

size_t ramp_ba_map_covariance_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1) {
  return ba_ws_bytes(E, n_poses, n_patches, t1 - t0, 1, 0, 0, true);       // (the map stage reads the covariance's buffers)
}

int ramp_ba_map_covariance(const float *poses, const float *patches, const float *intrinsics, const float *target,
                           const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                           const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1, float *cov,
                           float *depth_var, float *stats, float *point, float *point_cov, float *pose_depth_cov,
                           int32_t *n_obs, void *ws, size_t ws_bytes, int32_t *info, void *stream) {
  if (!point || !point_cov || !pose_depth_cov || !n_obs) return RAMP_EINVAL;
  const BaProblem p = {const_cast<float *>(poses), const_cast<float *>(patches), intrinsics, target, weight, lmbda, ii, jj,
                       kk, E, P, n_poses, n_patches, t0, t1, nullptr, 0};
  const BaCovOut out = {cov, depth_var, stats, nullptr, 0, BaMapOut{point, point_cov, pose_depth_cov, n_obs}};
  return ba_run(p, nullptr, 1, &out, ws, ws_bytes, info, (hipStream_t)stream);
}

size_t ramp_ba_map_covariance_planned_workspace_bytes(int E, int n_poses, int n_patches, int t0, int t1, int max_patches,
                                                      int max_pairs) {
  return ba_ws_bytes(E, n_poses, n_patches, t1 - t0, 0, max_patches, max_pairs, true);
}

int ramp_ba_map_covariance_planned(const float *poses, const float *patches, const float *intrinsics, const float *target,
                                   const float *weight, const float *lmbda, const int64_t *ii, const int64_t *jj,
                                   const int64_t *kk, int E, int P, int n_poses, int n_patches, int t0, int t1,
                                   float *cov, float *depth_var, float *stats, float *point, float *point_cov,
                                   float *pose_depth_cov, int32_t *n_obs, const int32_t *order_k, const int32_t *seg_k,
                                   const int32_t *ngroups_k, const int64_t *ukeys_k, int max_patches,
                                   const int32_t *order_p, const int32_t *seg_p, const int32_t *ngroups_p, int max_pairs,
                                   void *ws, size_t ws_bytes, int32_t *info, void *stream) {
  if (!point || !point_cov || !pose_depth_cov || !n_obs) return RAMP_EINVAL;
  const BaProblem p = {const_cast<float *>(poses), const_cast<float *>(patches), intrinsics, target, weight, lmbda, ii, jj,
                       kk, E, P, n_poses, n_patches, t0, t1, nullptr, 0};
  const BaGroups g = {order_k, seg_k, ngroups_k, ukeys_k, order_p, seg_p, ngroups_p, max_patches, max_pairs};
  const BaCovOut out = {cov, depth_var, stats, nullptr, 0, BaMapOut{point, point_cov, pose_depth_cov, n_obs}};
  return ba_run(p, &g, 1, &out, ws, ws_bytes, info, (hipStream_t)stream);
}

int ramp_map_select(const float *point_cov, const float *depth_var, const float *patches, const int32_t *n_obs, int n, int P,
                    const int32_t *dyn_rows, int per_row, float max_sigma, float max_rel_depth_sigma, int min_obs,
                    int32_t *index, int32_t *count, void *stream) {
  if (n < 0 || P < 2 || !count || (dyn_rows && per_row <= 0)) return RAMP_EINVAL;
  if (n > 0 && (!point_cov || !depth_var || !patches || !n_obs || !index)) return RAMP_EINVAL;
  hipLaunchKernelGGL(map_select_kernel, dim3(1), dim3(BA_SEL_THREADS), 0, (hipStream_t)stream, point_cov, depth_var, patches,
                     n_obs, n, P * P, 1 * P + 1, dyn_rows, per_row, max_sigma, max_rel_depth_sigma, min_obs, index, count);
  RAMP_CHECK_LAUNCH();
  return RAMP_OK;
}

}  // extern "C"
