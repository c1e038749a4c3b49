// The boundary between a caller's fp32 NCHW tensors and the engine's bf16 NHWC buffers (the module-level autograd entry points):
// stage outputs out, cotangents in, and the gradient join where a stage's own cotangent meets the gradient arriving from later
// stages.  LDS-tiled transposes (HBM bound).
//
// One workgroup (256 threads) moves a tile of 64 pixels x 64 channels of one image through LDS as fp32:
//   NCHW side : a wave owns a channel, its 64 lanes 64 consecutive pixels - 256 contiguous bytes per wave access;
//   NHWC side : a lane owns 8 consecutive channels of a pixel (16 bytes of bf16), 8 lanes a pixel's 64-channel slab (128 bytes).
// LDS tile: element (c, p) at c * 64 + (c >> 3) * 4 + p dwords - rows of 64 pixels, 4 dwords of padding after every 8 rows.
// Every LDS access is a 4-byte one (banks = dword address mod 32, conflicts within a 32-lane half):
//   NCHW-side accesses: fixed c, p = lane .. lane + 31          -> 32 consecutive dwords, 32 banks;
//   NHWC-side accesses: c = 8 cg + j (j fixed), the half's lanes are cg = 0..7 x 4 consecutive pixels p0 .. p0 + 3 (4 | p0)
//                       -> bank = (4 cg + p) mod 32: the padding moves each channel group by 4 banks, 32 distinct banks.
// HW need not be a multiple of 64 (the lanes of pixels past the end do nothing in either phase); C is a multiple of 64.
// HW == 1 (the heads' [N, C] tensors): the two layouts are the same array, so the maps are plain casts - 8 elements per lane, no LDS
// (layout_flat_kernel; taken when the fp32 side is 16-byte aligned, else the tiles above serve).
#include "vfs_ops.h"
#include "layout_host.h"

#define LAYOUT_LDS (64 * 64 + 8 * 4)
__device__ __forceinline__ int layout_lds_index(int c, int p) { return c * 64 + (c >> 3) * 4 + p; }

struct LayoutTile {
  size_t n;
  int hw0, c0;
};
__device__ __forceinline__ LayoutTile layout_tile(int HW, int C) {
  const unsigned slabs = (unsigned)C >> 6, strips = ((unsigned)HW + 63u) >> 6;
  unsigned b = blockIdx.x;
  LayoutTile t;
  t.c0 = (int)(b % slabs) << 6;
  b /= slabs;
  t.hw0 = (int)(b % strips) << 6;
  t.n = b / strips;
  return t;
}

// dst[n][c][hw] fp32 = src[n][hw][c] bf16
__global__ __launch_bounds__(256) void nhwc_bf16_to_nchw_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int HW, int C) {
  __shared__ float tile[LAYOUT_LDS];
  const LayoutTile tl = layout_tile(HW, C);
  const int t = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int q = t + 256 * r, cg = q & 7, p = q >> 3;
    if (tl.hw0 + p < HW) {
      float f[8];
      unpack8(ld16(src + (tl.n * HW + tl.hw0 + p) * C + tl.c0 + cg * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[layout_lds_index(cg * 8 + j, p)] = f[j];
    }
  }
  __syncthreads();
  const int p = t & 63, w = t >> 6;
  if (tl.hw0 + p < HW) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = w + 4 * i;
      dst[(tl.n * C + tl.c0 + c) * HW + tl.hw0 + p] = tile[layout_lds_index(c, p)];
    }
  }
}

// dst[n][hw][c] bf16 = rne(src[n][c][hw])   or, ADD,   rne(float(acc[n][hw][c]) + src[n][c][hw]).  dst may be acc: a lane reads
// the 16 bytes it writes and nobody else's (no __restrict__ on the two).
template <bool ADD>
__global__ __launch_bounds__(256) void nchw_f32_to_nhwc_bf16_kernel(const float* __restrict__ src, const bf16_t* acc, bf16_t* dst, int HW, int C) {
  __shared__ float tile[LAYOUT_LDS];
  const LayoutTile tl = layout_tile(HW, C);
  const int t = threadIdx.x;
  {
    const int p = t & 63, w = t >> 6;
    if (tl.hw0 + p < HW) {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = src[(tl.n * C + tl.c0 + w + 4 * i) * HW + tl.hw0 + p];
#pragma unroll
      for (int i = 0; i < 16; ++i) tile[layout_lds_index(w + 4 * i, p)] = v[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int q = t + 256 * r, cg = q & 7, p = q >> 3;
    if (tl.hw0 + p < HW) {
      const size_t o = (tl.n * HW + tl.hw0 + p) * C + tl.c0 + cg * 8;
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = tile[layout_lds_index(cg * 8 + j, p)];
      if (ADD) {
        float a[8];
        unpack8(ld16(acc + o), a);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = a[j] + f[j];
      }
      st16(dst + o, pack8(f));
    }
  }
}

// dst = rne(float(a) + float(b)), 8 elements per lane; dst may be a or b
__global__ __launch_bounds__(256) void bf16_add_kernel(const bf16_t* a, const bf16_t* b, bf16_t* dst, long long n8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float x[8], y[8];
  unpack8(ld16(a + i * 8), x);
  unpack8(ld16(b + i * 8), y);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] += y[j];
  st16(dst + i * 8, pack8(x));
}

// HW == 1: dst[i] = float(src[i]) (TO_F32), or bf16_rne([float(acc[i]) +] src[i]); 8 consecutive elements per lane
template <bool TO_F32, bool ADD>
__global__ __launch_bounds__(256) void layout_flat_kernel(const void* src, const bf16_t* acc, void* dst, long long n8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float f[8];
  if (TO_F32) {
    unpack8(ld16(reinterpret_cast<const bf16_t*>(src) + i * 8), f);
    float* o = reinterpret_cast<float*>(dst) + i * 8;
    *reinterpret_cast<f32x4*>(o) = (f32x4){f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(o + 4) = (f32x4){f[4], f[5], f[6], f[7]};
  } else {
    const float* in = reinterpret_cast<const float*>(src) + i * 8;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(in), hi = *reinterpret_cast<const f32x4*>(in + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = lo[j], f[4 + j] = hi[j];
    if (ADD) {
      float a[8];
      unpack8(ld16(acc + i * 8), a);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = a[j] + f[j];
    }
    st16(reinterpret_cast<bf16_t*>(dst) + i * 8, pack8(f));
  }
}
template <bool TO_F32, bool ADD>
static int layout_flat_launch(const char* who, const void* src, const bf16_t* acc, void* dst, int N, int C, hipStream_t s) {
  const long long n8 = (long long)N * C / 8;      // C % 64 == 0; N * C / 64 tiles < 2^31, so the grid fits
  hipLaunchKernelGGL((layout_flat_kernel<TO_F32, ADD>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, src, acc, dst, n8);
  return vfs_check_launch(who);
}

static int layout_refuse(const char* who, const char* what) { return vfs_fail(VFS_ERR_SHAPE, who, what); }
static bool misaligned16(const void* p) { return ((size_t)p & 15) != 0; }

int vfs_nhwc_bf16_to_nchw_f32_launch(const bf16_t* src, float* dst, int N, int HW, int C, hipStream_t s) {
  const char* who = "nhwc_bf16_to_nchw_f32";
  long long tiles = 0;
  if (const char* e = vfs_layout_check(src, nullptr, dst, 0, N, HW, C, &tiles)) return layout_refuse(who, e);
  if (misaligned16(src)) return vfs_fail(VFS_ERR_ARG, who, "the NHWC buffer must be 16-byte aligned");
  if (HW == 1 && !misaligned16(dst)) return layout_flat_launch<true, false>(who, src, nullptr, dst, N, C, s);
  hipLaunchKernelGGL(nhwc_bf16_to_nchw_f32_kernel, dim3((unsigned)tiles), dim3(256), 0, s, src, dst, HW, C);
  return vfs_check_launch(who);
}
int vfs_nchw_f32_to_nhwc_bf16_launch(const float* src, bf16_t* dst, int N, int HW, int C, hipStream_t s) {
  const char* who = "nchw_f32_to_nhwc_bf16";
  long long tiles = 0;
  if (const char* e = vfs_layout_check(src, nullptr, dst, 0, N, HW, C, &tiles)) return layout_refuse(who, e);
  if (misaligned16(dst)) return vfs_fail(VFS_ERR_ARG, who, "the NHWC buffer must be 16-byte aligned");
  if (HW == 1 && !misaligned16(src)) return layout_flat_launch<false, false>(who, src, nullptr, dst, N, C, s);
  hipLaunchKernelGGL(nchw_f32_to_nhwc_bf16_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, s, src, (const bf16_t*)nullptr, dst, HW, C);
  return vfs_check_launch(who);
}
int vfs_nchw_f32_add_nhwc_bf16_launch(const float* src, const bf16_t* acc, bf16_t* dst, int N, int HW, int C, hipStream_t s) {
  const char* who = "nchw_f32_add_nhwc_bf16";
  long long tiles = 0;
  if (const char* e = vfs_layout_check(src, acc, dst, 1, N, HW, C, &tiles)) return layout_refuse(who, e);
  if (misaligned16(acc) || misaligned16(dst)) return vfs_fail(VFS_ERR_ARG, who, "the NHWC buffers must be 16-byte aligned");
  if (HW == 1 && !misaligned16(src)) return layout_flat_launch<false, true>(who, src, acc, dst, N, C, s);
  hipLaunchKernelGGL(nchw_f32_to_nhwc_bf16_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, s, src, acc, dst, HW, C);
  return vfs_check_launch(who);
}
int vfs_bf16_add_launch(const bf16_t* a, const bf16_t* b, bf16_t* dst, long long n, hipStream_t s) {
  const char* who = "bf16_add";
  long long blocks = 0;
  if (const char* e = vfs_layout_add_check(a, b, dst, n, &blocks)) return layout_refuse(who, e);
  if (misaligned16(a) || misaligned16(b) || misaligned16(dst)) return vfs_fail(VFS_ERR_ARG, who, "the buffers must be 16-byte aligned");
  hipLaunchKernelGGL(bf16_add_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, b, dst, n / 8);
  return vfs_check_launch(who);
}
