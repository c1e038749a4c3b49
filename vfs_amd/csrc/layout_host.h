// Host side of the layout entry points (vfs_nhwc_bf16_to_nchw_f32 / vfs_nchw_f32_to_nhwc_bf16 / vfs_nchw_f32_add_nhwc_bf16 /
// vfs_bf16_add, csrc/layout.hip): the argument checks, the grid arithmetic, and the three maps stated element by element.  Plain
// C++ without any HIP, so that a stand-alone host program (tools/layout_check.cpp) can run it under the sanitizers; the emulator
// build compiles the same text.
//
// The maps, for n < N, hw < HW, c < C:
//   to_nchw :  dst[(n*C + c)*HW + hw] = float(src[(n*HW + hw)*C + c])                      (bf16 -> fp32 is exact)
//   to_nhwc :  dst[(n*HW + hw)*C + c] = bf16_rne(src[(n*C + c)*HW + hw])
//   join    :  dst[(n*HW + hw)*C + c] = bf16_rne(float(acc[(n*HW + hw)*C + c]) + src[(n*C + c)*HW + hw])      ONE rounding
//   add     :  dst[i] = bf16_rne(float(a[i]) + float(b[i]))
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define VFS_LAYOUT_TILE 64      // pixels (and channels) of one workgroup's tile

static inline float vfs_layout_bf16_to_f32(uint16_t v) {
  const uint32_t u = (uint32_t)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// round to nearest, ties to even; Inf stays Inf, a finite value beyond the largest bf16 rounds to Inf, NaN -> the quiet NaN
static inline uint16_t vfs_layout_f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static inline void vfs_layout_to_nchw_host(const uint16_t* src, float* dst, int N, int HW, int C) {
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int hw = 0; hw < HW; ++hw) dst[((size_t)n * C + c) * HW + hw] = vfs_layout_bf16_to_f32(src[((size_t)n * HW + hw) * C + c]);
}
// acc == nullptr: the plain conversion; else the join (dst may be acc)
static inline void vfs_layout_to_nhwc_host(const float* src, const uint16_t* acc, uint16_t* dst, int N, int HW, int C) {
  for (int n = 0; n < N; ++n)
    for (int hw = 0; hw < HW; ++hw)
      for (int c = 0; c < C; ++c) {
        const size_t o = ((size_t)n * HW + hw) * C + c;
        const float s = src[((size_t)n * C + c) * HW + hw];
        dst[o] = vfs_layout_f32_to_bf16(acc ? vfs_layout_bf16_to_f32(acc[o]) + s : s);
      }
}
static inline void vfs_layout_add_host(const uint16_t* a, const uint16_t* b, uint16_t* dst, long long n) {
  for (long long i = 0; i < n; ++i) dst[i] = vfs_layout_f32_to_bf16(vfs_layout_bf16_to_f32(a[i]) + vfs_layout_bf16_to_f32(b[i]));
}

// ---- argument checks: nullptr when the call may launch (then *tiles = workgroups), else what is wrong ----
// One workgroup per (image, 64-pixel strip, 64-channel slab); offsets inside the kernels are 64-bit, so the limit is the grid's:
// fewer than 2^31 workgroups.
static inline const char* vfs_layout_check(const void* src, const void* acc, const void* dst, int need_acc, int N, int HW, int C,
                                           long long* tiles) {
  if (!src || !dst || (need_acc && !acc)) return "null buffer";
  if (N <= 0 || HW <= 0 || C <= 0) return "N, HW and C must be positive";
  if (C % 64) return "C must be a multiple of 64";
  const long long strips = ((long long)HW + VFS_LAYOUT_TILE - 1) / VFS_LAYOUT_TILE;
  const long long slabs = C / 64;
  if (strips > 0x7fffffffLL / slabs || (long long)N > 0x7fffffffLL / (strips * slabs)) return "2^31 tiles or more";
  *tiles = (long long)N * strips * slabs;
  return nullptr;
}
static inline const char* vfs_layout_add_check(const void* a, const void* b, const void* dst, long long n, long long* blocks) {
  if (!a || !b || !dst) return "null buffer";
  if (n <= 0) return "n must be positive";
  if (n % 8) return "n must be a multiple of 8";
  if (n > (1LL << 40)) return "more than 2^40 elements";
  *blocks = (n / 8 + 255) / 256;
  return nullptr;
}
