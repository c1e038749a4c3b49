// The row arithmetic of the feature bank, ONE copy: F.normalize(p=2, dim=channel, eps=1e-12) of a feature row in fp32 and in bf16
// (local_attention.py:277-279) and the bf16 hi / lo split of an fp32 unit row (the operands of the two-pass kernels' matrix pass).
// Called by the contiguous kernels (exact_f32.hip l2norm_rows_f32_kernel, labelprop2.hip split_rows_bf16x2_kernel, labelprop.hip
// l2norm_rows_kernel) and by the table-driven ingest (bank_ingest.hip), which therefore writes their bits.
//
// What belongs to the bits besides these bodies is the ownership of a row, and the callers share it: one wave per row; in fp32 lane l
// owns the float4 groups l, l + 64, ... and runs ONE ascending fmaf chain over them; in bf16 lane l owns the 8-channel groups l,
// l + 64, ...; the lanes' sums meet in the butterfly below.
#pragma once
#include "vfs_common.h"

// sum over the 64 lanes of a wave, the result in every lane (xor butterfly, 32 first)
__device__ __forceinline__ float rows_wave_sum(float ss) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) ss = ss + __shfl_xor(ss, d);
  return ss;
}

// ---- fp32: every step a single correctly rounded operation (the contract of exact_f32.hip, whatever the including file sets) ----
__device__ __forceinline__ float rows_f32_sumsq(f32x4 v, float ss) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
  return ss;
}
__device__ __forceinline__ float rows_f32_norm(float ss) {
  const float nrm = sqrtf(ss);
  return nrm > 1e-12f ? nrm : 1e-12f;
}
__device__ __forceinline__ f32x4 rows_f32_unit(f32x4 v, float nrm) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] / nrm;
  return v;
}
// split of 8 consecutive channels v of a unit row, x = hi + lo: hi = bf16(x), lo = bf16(x - hi) (the difference is exact in fp32);
// layout of a split row [C/16][hi k0..7 | hi k8..15 | lo k0..7 | lo k8..15]: the hi half of 8-channel group c8 starts at
// rows_split_at(c8), its lo half 16 elements further
__device__ __forceinline__ u32x4 rows_split_hi(const float* v) { return pack8(v); }
__device__ __forceinline__ u32x4 rows_split_lo(const float* v) {
#pragma clang fp contract(off)
  float lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) lo[j] = v[j] - round_bf(v[j]);
  return pack8(lo);
}
__device__ __forceinline__ int rows_split_at(int c8) { return (c8 >> 1) * 32 + (c8 & 1) * 8; }

// ---- bf16: 8 channels per 16-byte vector, sums in fp32; a square and its addition are two roundings (what the compiler made of
// the contiguous kernel before this header existed; pinned, so that every caller gets the same bits) ----
__device__ __forceinline__ float rows_bf16_sumsq(u32x4 v, float ss) {
#pragma clang fp contract(off)
  float f[8];
  unpack8(v, f);
#pragma unroll
  for (int i = 0; i < 8; ++i) ss += f[i] * f[i];
  return ss;
}
__device__ __forceinline__ float rows_bf16_inv(float ss) { return 1.0f / fmaxf(sqrtf(ss), 1e-12f); }
__device__ __forceinline__ u32x4 rows_bf16_unit(u32x4 v, float inv) {
  float f[8];
  unpack8(v, f);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] *= inv;
  return pack8(f);
}
