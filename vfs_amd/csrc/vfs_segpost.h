// Post-processing of a propagated frame (vanilla_tracker.py:162-181), ONE text for both precisions:
//   up = F.interpolate(seg[HW][CO] -> [Ho][Wo], bilinear, align_corners=False)
//   per class: (up - min) / (max - min + 1e-12) where max > 0
//   label = argmax over classes (first maximum) -> uint8
// labelprop.hip (bf16 precision) and exact_f32.hip include this file and wrap the bodies in their kernels.  The arithmetic of a
// precision is the including file's floating-point mode AT THE INCLUDE: exact_f32.hip switches contraction off BEFORE it (and refuses
// to compile if this file came in earlier), so there every operation below is a single correctly rounded fp32 operation (oracle:
// xo_bilerp / xo_seg_postprocess); labelprop.hip leaves the compiler's default, which fuses the multiply-adds.  Everything here is
// `static`: the two translation units hold two different compilations of the same names.
// min / max are written as comparisons, the oracle's form: (v < m ? v : m) keeps m on a tie and on a NaN v, so the exact kernels
// keep the oracle's bits down to the sign of a zero.  fminf / fmaxf (labelprop.hip's earlier form) agree on every non-NaN input but
// may return the other zero of (+0, -0); that sign changes neither (v - min) / (max - min + 1e-12) > best nor max > 0.
#pragma once
#define VFS_SEGPOST_H
#include "vfs_lpb.h"

static __device__ __forceinline__ float seg_min(float v, float m) { return v < m ? v : m; }
static __device__ __forceinline__ float seg_max(float v, float m) { return v > m ? v : m; }

// the four taps of output pixel (oy, ox) and their weights; sy = H / Ho, sx = W / Wo
struct SegTaps {
  int y0, y1, x0, x1;
  float ly, lx, hy, hx;
};
static __device__ __forceinline__ SegTaps seg_taps(int H, int W, int oy, int ox, float sy, float sx) {
  float fy = sy * ((float)oy + 0.5f) - 0.5f, fx = sx * ((float)ox + 0.5f) - 0.5f;
  fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
  SegTaps t;
  t.y0 = (int)fy; t.x0 = (int)fx;
  t.y1 = t.y0 + (t.y0 < H - 1 ? 1 : 0); t.x1 = t.x0 + (t.x0 < W - 1 ? 1 : 0);
  t.ly = fy - (float)t.y0; t.lx = fx - (float)t.x0;
  t.hy = 1.f - t.ly; t.hx = 1.f - t.lx;
  return t;
}
static __device__ __forceinline__ float seg_blend(const SegTaps& t, float v00, float v01, float v10, float v11) {
  return t.hy * (t.hx * v00 + t.lx * v01) + t.ly * (t.hx * v10 + t.lx * v11);
}
static __device__ __forceinline__ float seg_bilerp(const float* __restrict__ seg, int H, int W, int CO, int c, int oy, int ox, float sy,
                                                   float sx) {
  const SegTaps t = seg_taps(H, W, oy, ox, sy, sx);
  return seg_blend(t, seg[((size_t)t.y0 * W + t.x0) * CO + c], seg[((size_t)t.y0 * W + t.x1) * CO + c],
                   seg[((size_t)t.y1 * W + t.x0) * CO + c], seg[((size_t)t.y1 * W + t.x1) * CO + c]);
}

// pass 1, grid (LP_POST_BLOCKS, classes): per-class min / max of the upsampled map, one class and one partial per workgroup (the 64
// workgroups of the first version walked the classes one after the other - a quarter of the CUs, 37 us per 480 x 854 frame with
// four classes).  min / max do not depend on the order: same bits.
static __device__ __forceinline__ void seg_minmax_body(const float* __restrict__ seg, float* __restrict__ partial, int H, int W, int CO,
                                                       int Ho, int Wo) {
  __shared__ float smn[256], smx[256];
  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
  const int total = Ho * Wo, c = blockIdx.y;
  const int stride = gridDim.x * 256, dy = stride / Wo, dx = stride - dy * Wo;
  float mn = INFINITY, mx = -INFINITY;
  int p = blockIdx.x * 256 + threadIdx.x, oy = p / Wo, ox = p - oy * Wo;
  for (; p < total; p += stride) {
    const float v = seg_bilerp(seg, H, W, CO, c, oy, ox, sy, sx);
    mn = seg_min(v, mn); mx = seg_max(v, mx);
    oy += dy; ox += dx;
    if (ox >= Wo) { ox -= Wo; ++oy; }
  }
  smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const float o1 = smn[threadIdx.x + s], o2 = smx[threadIdx.x + s];
      smn[threadIdx.x] = seg_min(o1, smn[threadIdx.x]);
      smx[threadIdx.x] = seg_max(o2, smx[threadIdx.x]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[((size_t)blockIdx.x * CO + c) * 2] = smn[0];
    partial[((size_t)blockIdx.x * CO + c) * 2 + 1] = smx[0];
  }
}

// pass 2: the nblk partials of pass 1 in their fixed order, then normalise and take the argmax
static __device__ __forceinline__ void seg_argmax_body(const float* __restrict__ seg, const float* __restrict__ partial, int nblk,
                                                       uint8_t* __restrict__ label, int H, int W, int CO, int Ho, int Wo) {
  __shared__ float smn[LP_MAX_CLASSES], smx[LP_MAX_CLASSES];
  if ((int)threadIdx.x < CO) {
    float mn = INFINITY, mx = -INFINITY;
    for (int b = 0; b < nblk; ++b) {
      const float p0 = partial[((size_t)b * CO + threadIdx.x) * 2], p1 = partial[((size_t)b * CO + threadIdx.x) * 2 + 1];
      mn = seg_min(p0, mn); mx = seg_max(p1, mx);
    }
    smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
  }
  __syncthreads();
  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
  const int total = Ho * Wo;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
    const int oy = p / Wo, ox = p % Wo;
    float best = -INFINITY;
    int bc = 0;
    for (int c = 0; c < CO; ++c) {
      float v = seg_bilerp(seg, H, W, CO, c, oy, ox, sy, sx);
      if (smx[c] > 0.f) v = (v - smn[c]) / (smx[c] - smn[c] + 1e-12f);
      if (v > best) { best = v; bc = c; }
    }
    label[p] = (uint8_t)bc;
  }
}

// the batch kernels: slot blockIdx.z post-processes ITS propagated frame with its own class count into the row's map position of
// its label maps (seg_post_slot: vfs_lpb.h); the class dimension of the min / max grid is sized for COcap
static __device__ __forceinline__ void seg_minmax_batch_body(const SegPostBatchArgs& b) {
  const float* seg; float* partial; uint8_t* label; int CO;
  if (!seg_post_slot(b, seg, partial, label, CO) || (int)blockIdx.y >= CO) return;
  seg_minmax_body(seg, partial, b.H, b.W, CO, b.Ho, b.Wo);
}
static __device__ __forceinline__ void seg_argmax_batch_body(const SegPostBatchArgs& b) {
  const float* seg; float* partial; uint8_t* label; int CO;
  if (!seg_post_slot(b, seg, partial, label, CO)) return;
  seg_argmax_body(seg, partial, LP_POST_BLOCKS, label, b.H, b.W, CO, b.Ho, b.Wo);
}

// The two launches of one step, for one video (classes = its CO, nslots = 1) or a lock-step batch (classes = COcap).  who /
// minmax_name / argmax_name: the entry point and its kernels in the error texts; minmax(grid) / argmax(grid) launch the form's kernels.
template <class LaunchMinmax, class LaunchArgmax>
static int seg_post_launch(const char* who, const char* minmax_name, const char* argmax_name, int classes, int nslots, int Ho, int Wo,
                           LaunchMinmax minmax, LaunchArgmax argmax) {
  if (classes < 1 || classes > LP_MAX_CLASSES) return vfs_fail(VFS_ERR_SHAPE, who, "1 <= classes <= 256");
  minmax(dim3(LP_POST_BLOCKS, classes, nslots));
  int rc = vfs_check_launch(minmax_name);
  if (rc) return rc;
  int blocks = (Ho * Wo + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  argmax(dim3(blocks, 1, nslots));
  return vfs_check_launch(argmax_name);
}
