// What the event map (evmap.hip), its renderer (maprender.hip) and the localiser (maplocalize.hip) share: the voxel hash's slot
// and constants, its hash, the voxel indices of a key, the mean point of a slot -- one definition, so that the export and the
// renderer give a voxel the same point in every bit --, the projection of that point -- one definition again, so that the
// renderer and the localiser give a voxel the same u, v in every bit -- and the camera words with their test
// (RAMP_DEPTH_POINTS_BAD_CAMERA, RAMP_MAP_RENDER_BAD_CAMERA, RAMP_MAP_LOCALIZE_BAD_CAMERA).
#pragma once
#include "ramp_internal.h"
#include "ramp_device.h"

#define EVM_THREADS 256
#define EVM_AXIS (1ll << 20)               // voxel indices lie in (-2^20, 2^20); the fractions are in units of 2^-20 voxel
#define EVM_CONF_BITS 16
#define EVM_EMPTY (-1ll)                   // no voxel's key: bit 63 of a key is clear
#define EVM_HEADER 64                      // bytes in front of the slots

struct __attribute__((aligned(64))) EvmSlot {
  long long key, n, sq[3], sc;
  unsigned long long views;
  long long spare;
};
static_assert(sizeof(EvmSlot) == 64, "one slot, one 64-byte line");
typedef unsigned long long evm_u64;

static __device__ __forceinline__ bool evm_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

// c[0..6] = cam, c[7..10] = (fx, fy, cx, cy); true: a word is not finite or fx / fy is 0
static __device__ __forceinline__ bool evm_load_camera(const float *cam, const float *intrinsics, float *c) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 11; k++) {
    c[k] = k < 7 ? cam[k] : intrinsics[k - 7];
    bad = bad || !evm_finite(c[k]);
  }
  return bad || c[7] == 0.0f || c[8] == 0.0f;
}

static __device__ __forceinline__ evm_u64 evm_hash(evm_u64 z) {          // the finaliser of splitmix64
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the voxel index of a key along axis a (0: x, bits 42 .. 62; 1: y, bits 21 .. 41; 2: z, bits 0 .. 20)
static __device__ __forceinline__ long long evm_key_index(long long key, int a) {
  return ((key >> (42 - 21 * a)) & (2 * EVM_AXIS - 1)) - EVM_AXIS;
}

// the mean point of a slot along axis a: float32((double(i_a) + (double(sq_a) / double(n)) * 2^-20) * voxel)
static __device__ __forceinline__ float evm_mean_axis(long long key, long long sq, long long n, int a, double voxel) {
  return (float)(((double)evm_key_index(key, a) + ((double)sq / (double)n) * (1.0 / (double)EVM_AXIS)) * voxel);
}
// The projection of a slot's mean point into the camera c (evm_load_camera's words; cam is CAMERA-TO-WORLD), fp32 without FMA --
// one definition, so that the renderer (maprender.hip) and the localiser (maplocalize.hip) give a voxel the same u, v in every
// bit.  False: REJECTED (z <= RAMP_WARP_MIN_Z or NaN, a word of Xc, u or v not finite); the outputs are then not to be used.
static __device__ __forceinline__ bool evm_project(long long key, const long long *sq, long long n, const float *c, double voxel,
                                                   float *Xc, float *d_out, float *u_out, float *v_out) {
  float dX[3];
#pragma unroll
  for (int a = 0; a < 3; a++) dX[a] = evm_mean_axis(key, sq[a], n, a, voxel) - c[a];
  const float qi[4] = {-c[3], -c[4], -c[5], c[6]};
  lt_qrot(qi, dX, Xc);
  const float z = Xc[2];
  const float d = 1.0f / z;
  const float u = c[7] * (Xc[0] * d) + c[9], v = c[8] * (Xc[1] * d) + c[10];
  *d_out = d; *u_out = u; *v_out = v;
  return !(!(z > RAMP_WARP_MIN_Z) || !evm_finite(Xc[0]) || !evm_finite(Xc[1]) || !evm_finite(z) || !evm_finite(u) || !evm_finite(v));
}
// what the export writes beside the point: n saturating, the summed confidence
static __device__ __forceinline__ int32_t evm_count_word(long long n) { return (int32_t)(n < 2147483647ll ? n : 2147483647ll); }
static __device__ __forceinline__ float evm_conf_word(long long sc) {
  return (float)((double)sc * (1.0 / (double)(1 << EVM_CONF_BITS)));
}
// the export's conditions on a slot
static __device__ __forceinline__ bool evm_slot_passes(long long key, long long n, evm_u64 views, long long min_points,
                                                       int min_views) {
  return key != EVM_EMPTY && n >= min_points && __popcll(views) >= min_views;
}

static inline bool evm_capacity_ok(long capacity) {
  return capacity >= 8 && capacity <= (1l << 30) && (capacity & (capacity - 1)) == 0;
}
static inline EvmSlot *evm_slots(void *map) { return reinterpret_cast<EvmSlot *>((char *)map + EVM_HEADER); }
