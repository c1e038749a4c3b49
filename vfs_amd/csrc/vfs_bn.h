// The BatchNorm arithmetic, ONE copy (device helpers only): statistics -> coefficients and running statistics (forward), masked
// gradient, S1 / S2 accumulation and the dx coefficients (backward).  Every kernel that finalises statistics or takes part in a
// BatchNorm backward calls these - csrc/bn.hip, the fused Linear + BatchNorm1d launch of csrc/conv_pw.hip, the dgrad epilogues
// (vfs_conv.h bnfuse_accum) and the stem (vfs_stem.h) - because the variants must produce the same bits: the fused and the
// two-launch paths are interchangeable per layer (tests/test_emu_bn.py::test_bn_chunked_single_launch_reduction).
// The casts and the expression shapes below are part of that contract.
#pragma once
#include "vfs_common.h"

// running = (1 - momentum) * running + momentum * statistic (unbiased variance).  A NaN statistic - the poison a failed SyncBN
// window exchange writes into its sums (vfs_p2p.h) - must not reach the running statistics: they outlive the step (checkpoints).
// (written with explicit fmaf: the compiler contracted `a * b + c * d` differently in different kernels)
__device__ __forceinline__ void bn_running_update(float& rm, float& rv, float momentum, double mean, double unbiased) {
  if (mean != mean || unbiased != unbiased) return;
  const float keep = 1.f - momentum;
  rm = __builtin_fmaf(momentum, (float)mean, keep * rm);
  rv = __builtin_fmaf(momentum, (float)unbiased, keep * rv);
}

// one channel of one group: what the apply passes read (the four rows of bnp) and what the running statistics take
struct BnCoef {
  float scale, shift, invstd;   // scale = gamma * invstd, shift = beta - mean * scale
  double mean, unbiased;
};
__device__ __forceinline__ BnCoef bn_finalize_channel(double sum, double sumsq, double count, float eps, float gamma, float beta) {
  BnCoef k;
  k.mean = sum / count;
  double var = sumsq / count - k.mean * k.mean;
  if (var < 0.0) var = 0.0;
  k.invstd = (float)(1.0 / sqrt(var + (double)eps));
  k.scale = gamma * k.invstd;
  k.shift = beta - (float)k.mean * k.scale;
  k.unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
  return k;
}
// bnp[g][4][C] = {scale, shift, mean, invstd}
__device__ __forceinline__ void bn_store_params(float* bnp, int g, int C, int c, const BnCoef& k) {
  float* o = bnp + (size_t)g * 4 * C;
  o[c] = k.scale;
  o[C + c] = k.shift;
  o[2 * C + c] = (float)k.mean;
  o[3 * C + c] = k.invstd;
}

// gradient of eight channels behind the unit's ReLU: the mask is given (has_y: bit i of ymask <-> activation i is positive), or
// recomputed from x * scale + shift > 0 (relu, a plain conv->BN->ReLU unit: saves a read), or there is none
// (on a local copy, as the kernels had it inline: selecting through the caller's pointer costs bn_bwd_apply_kernel three VGPRs
// and with them a wave of occupancy)
__device__ __forceinline__ void bn_mask_grad(float* gio, const float* x, unsigned ymask, bool has_y, int relu, const float* sc,
                                             const float* sh) {
  float g[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) g[i] = gio[i];
  if (has_y) {
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = ((ymask >> i) & 1u) ? g[i] : 0.f;
  } else if (relu) {
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = (x[i] * sc[i] + sh[i] > 0.f) ? g[i] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) gio[i] = g[i];
}
__device__ __forceinline__ float bn_xhat(float x, float mean, float inv) { return (x - mean) * inv; }
// S1 += g, S2 += g * xhat
__device__ __forceinline__ void bn_bwd_accum(float* s1, float* s2, const float* g, const float* x, const float* mean, const float* inv) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s1[i] += g[i];
    s2[i] += g[i] * bn_xhat(x[i], mean[i], inv[i]);
  }
}
// dx = scale * (g - S1/count - xhat * S2/count) = scale * g + B * x + D;  rc = 1 / count
__device__ __forceinline__ void bn_bwd_coefs(float scale, float mean, float inv, double s1, double s2, float rc, float& B, float& D) {
  const float m1 = (float)s1 * rc, m2 = (float)s2 * rc;
  B = -scale * inv * m2;
  D = scale * (mean * inv * m2 - m1);
}
