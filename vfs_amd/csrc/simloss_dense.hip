// DenseSimSiamHead's loss on the head's own output: CosineSimLoss(with_norm=True, pairwise=False) per spatial position of
// bf16 NHWC maps, for all temporal rolls of the step at once (sim_loss.py:43-62 inside sim_siam_head.py:277-284 and the roll
// loop of sim_siam_base_tracker.py:39-55).  HBM bound: every operand row (the C channels of one position) is read with
// 16-byte loads by the `lpp` consecutive lanes that own the position, once per (row, roll).
//
// Grid: x = image i, y = roll k (forward) / view (backward), z = slice of the positions.  A wave holds 64 / lpp positions at a
// time (lpp = the power of two >= C / 8, at most 64; above 512 channels a lane owns up to DSL_MAX_CHUNKS 16-byte chunks), a
// workgroup of 4 waves one "unit" of 4 * 64 / lpp positions; workgroup z takes the units z, z + Z, ...
// No atomics: the forward writes one (sum cos1, sum cos2) pair per workgroup, summed in z order by the finish kernel; the
// backward's positions are independent, its sum over the rolls runs in roll order in registers.
#include "vfs_ops.h"

__device__ __forceinline__ float dsl_group_sum(float v, int lpp) {      // over the lpp consecutive lanes of a position; every lane gets it
  for (int d = lpp >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

struct DslLane {      // what a lane owns of the workgroup's current unit
  int s;              // position (>= S: none)
  int sub;            // lane within the position's group: it owns the chunks sub, sub + lpp, ...
};
__device__ __forceinline__ DslLane dsl_lane(const DenseLossArgs& a, int unit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gpw = 64 / a.lpp;
  DslLane l;
  l.sub = lane & (a.lpp - 1);
  l.s = (unit * 4 + wave) * gpw + lane / a.lpp;
  return l;
}

// partial[((k * N + i) * Z + z) * 2 + {0, 1}] = sum over the workgroup's positions of cos(p1[i], z2[j]) / cos(p2[j], z1[i]), j = roll_k(i)
template <int NCH>
__global__ __launch_bounds__(256) void dense_cosine_loss_fwd_kernel(DenseLossArgs a) {
  __shared__ float sh[4][2];
  const int i = blockIdx.x, k = blockIdx.y;
  const int j = roll_src(i, a.T, k);
  const int nch = a.C >> 3, upw = 4 * (64 / a.lpp);
  const int nunits = (a.S + upw - 1) / upw;
  const float eps = 1e-12f;
  float m1 = 0.f, m2 = 0.f;
  for (int unit = blockIdx.z; unit < nunits; unit += gridDim.z) {      // (uniform trip count: the shuffles below see whole waves)
    const DslLane l = dsl_lane(a, unit);
    float d1 = 0.f, d2 = 0.f, np1 = 0.f, nz2 = 0.f, np2 = 0.f, nz1 = 0.f;
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const int ch = l.sub + q * a.lpp;
      if (l.s < a.S && ch < nch) {
        const size_t oi = ((size_t)i * a.S + l.s) * a.C + ch * 8, oj = ((size_t)j * a.S + l.s) * a.C + ch * 8;
        float p1[8], z1[8], p2[8], z2[8];
        unpack8(ld16(a.p1 + oi), p1); unpack8(ld16(a.z1 + oi), z1);
        unpack8(ld16(a.p2 + oj), p2); unpack8(ld16(a.z2 + oj), z2);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          d1 += p1[e] * z2[e]; d2 += p2[e] * z1[e];
          np1 += p1[e] * p1[e]; nz2 += z2[e] * z2[e]; np2 += p2[e] * p2[e]; nz1 += z1[e] * z1[e];
        }
      }
    }
    d1 = dsl_group_sum(d1, a.lpp); d2 = dsl_group_sum(d2, a.lpp);
    np1 = dsl_group_sum(np1, a.lpp); nz2 = dsl_group_sum(nz2, a.lpp);
    np2 = dsl_group_sum(np2, a.lpp); nz1 = dsl_group_sum(nz1, a.lpp);
    if (l.s < a.S) {
      m1 += d1 / (fmaxf(sqrtf(np1), eps) * fmaxf(sqrtf(nz2), eps));
      m2 += d2 / (fmaxf(sqrtf(np2), eps) * fmaxf(sqrtf(nz1), eps));
    }
  }
  for (int d = a.lpp; d < 64; d <<= 1) {      // the lanes of a group hold the same value: sum over the wave's groups
    m1 += __shfl_xor(m1, d); m2 += __shfl_xor(m2, d);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[wave][0] = m1; sh[wave][1] = m2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = a.partial + (((size_t)k * a.N + i) * gridDim.z + blockIdx.z) * 2;
    out[0] = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
    out[1] = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
  }
}
// loss[k][i] = weight * (0.5 * L(m1) + 0.5 * L(m2)),  m = (sum of the Z partials, in z order) / S,  L(m) = negative ? -m : 2 - 2 m
__global__ __launch_bounds__(256) void dense_cosine_loss_finish_kernel(DenseLossArgs a, int Z) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.K * a.N) return;
  const float* part = a.partial + (size_t)e * Z * 2;
  float m1 = 0.f, m2 = 0.f;
  for (int z = 0; z < Z; ++z) { m1 += part[2 * z]; m2 += part[2 * z + 1]; }
  const float inv = 1.0f / (float)a.S;
  m1 *= inv; m2 *= inv;
  const float l1 = a.negative ? -m1 : 2.f - 2.f * m1, l2 = a.negative ? -m2 : 2.f - 2.f * m2;
  a.loss[e] = (0.5f * l1 + 0.5f * l2) * a.weight;
}

// gradient wrt p (z is detached in the reference), per position s:
//   view 0: dp1[i][s] = sum_k gloss[k][i]        * w / (2 S) * dL/da (a = p1[i][s], b = z2[roll_k(i)][s])
//   view 1: dp2[j][s] = sum_k gloss[k][inv_k(j)] * w / (2 S) * dL/da (a = p2[j][s], b = z1[inv_k(j)][s])
//   dL/da = coef * (bhat - cos * ahat) / max(|a|, eps),  coef = -2 (or -1 when negative)
// Register plan of a lane: its NCH <= DSL_MAX_CHUNKS chunks of a, of the current b and of the accumulated gradient, 8 fp32 each.
template <int NCH>
__global__ __launch_bounds__(256) void dense_cosine_loss_bwd_kernel(DenseLossArgs a) {
  const int i = blockIdx.x, view = blockIdx.y;
  const bf16_t* A = view == 0 ? a.p1 : a.p2;
  const bf16_t* Bz = view == 0 ? a.z2 : a.z1;
  bf16_t* out = view == 0 ? a.dp1 : a.dp2;
  const int nch = a.C >> 3, upw = 4 * (64 / a.lpp);
  const int nunits = (a.S + upw - 1) / upw;
  const float eps = 1e-12f, scale = a.weight * 0.5f * (a.negative ? -1.f : -2.f) / (float)a.S;
  const int bvid = i / a.T, t = i - bvid * a.T;
  for (int unit = blockIdx.z; unit < nunits; unit += gridDim.z) {
    const DslLane l = dsl_lane(a, unit);
    const bool live = l.s < a.S;
    float av[NCH][8], acc[NCH][8];
    float na = 0.f;
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const int ch = l.sub + q * a.lpp;
#pragma unroll
      for (int e = 0; e < 8; ++e) { av[q][e] = 0.f; acc[q][e] = 0.f; }
      if (live && ch < nch) unpack8(ld16(A + ((size_t)i * a.S + l.s) * a.C + ch * 8), av[q]);
#pragma unroll
      for (int e = 0; e < 8; ++e) na += av[q][e] * av[q][e];
    }
    na = fmaxf(sqrtf(dsl_group_sum(na, a.lpp)), eps);
    for (int k = 0; k < a.K; ++k) {
      int u, gi;
      if (view == 0) { u = t - k; if (u < 0) u += a.T; gi = i; }            // partner = roll_k(i), loss index i
      else { u = t + k; if (u >= a.T) u -= a.T; gi = bvid * a.T + u; }      // p2[i] is paired with loss index inv_k(i)
      const int j = bvid * a.T + u;
      float bv[NCH][8];
      float nb = 0.f, dot = 0.f;
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
        const int ch = l.sub + q * a.lpp;
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[q][e] = 0.f;
        if (live && ch < nch) unpack8(ld16(Bz + ((size_t)j * a.S + l.s) * a.C + ch * 8), bv[q]);
#pragma unroll
        for (int e = 0; e < 8; ++e) { nb += bv[q][e] * bv[q][e]; dot += av[q][e] * bv[q][e]; }
      }
      nb = fmaxf(sqrtf(dsl_group_sum(nb, a.lpp)), eps);
      const float cs = dsl_group_sum(dot, a.lpp) / (na * nb);
      const float gs = a.gloss[(size_t)k * a.N + gi] * scale / na;
      const float cb = gs / nb, ca = gs * cs / na;      // per (position, roll): the element loop below has no division
#pragma unroll
      for (int q = 0; q < NCH; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[q][e] += cb * bv[q][e] - ca * av[q][e];
    }
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const int ch = l.sub + q * a.lpp;
      if (live && ch < nch) st16(out + ((size_t)i * a.S + l.s) * a.C + ch * 8, pack8(acc[q]));
    }
  }
}

// ------------------------------------------------------------------ host side
// lanes per position and 16-byte chunks per lane for C channels (C % 8 == 0, C <= VFS_DENSE_LOSS_MAX_C)
static void dsl_plan(int C, int* lpp, int* nchl) {
  const int nch = C >> 3;
  int l = 1;
  while (l < nch && l < 64) l <<= 1;
  *lpp = l;
  *nchl = (nch + l - 1) / l;
}
// workgroups along z: a function of the row geometry alone (never of N or K), so equal inputs are summed in the same order
int vfs_dense_loss_split(int S, int C) {
  int lpp, nchl;
  dsl_plan(C, &lpp, &nchl);
  const int upw = 4 * (64 / lpp);
  const int nunits = (S + upw - 1) / upw;
  return nunits < DSL_MAX_SPLIT ? nunits : DSL_MAX_SPLIT;
}
int vfs_dense_cosine_loss_fwd_launch(const DenseLossArgs& a_in, hipStream_t s) {
  DenseLossArgs a = a_in;
  int nchl;
  dsl_plan(a.C, &a.lpp, &nchl);
  const int Z = vfs_dense_loss_split(a.S, a.C);
  const dim3 grid(a.N, a.K, Z);
  if (nchl == 1) hipLaunchKernelGGL(dense_cosine_loss_fwd_kernel<1>, grid, dim3(256), 0, s, a);
  else if (nchl == 2) hipLaunchKernelGGL(dense_cosine_loss_fwd_kernel<2>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(dense_cosine_loss_fwd_kernel<DSL_MAX_CHUNKS>, grid, dim3(256), 0, s, a);
  if (int rc = vfs_check_launch("dense_cosine_loss_fwd")) return rc;
  hipLaunchKernelGGL(dense_cosine_loss_finish_kernel, dim3((a.K * a.N + 255) / 256), dim3(256), 0, s, a, Z);
  return vfs_check_launch("dense_cosine_loss_finish");
}
int vfs_dense_cosine_loss_bwd_launch(const DenseLossArgs& a_in, hipStream_t s) {
  DenseLossArgs a = a_in;
  int nchl;
  dsl_plan(a.C, &a.lpp, &nchl);
  const dim3 grid(a.N, 2, vfs_dense_loss_split(a.S, a.C));
  if (nchl == 1) hipLaunchKernelGGL(dense_cosine_loss_bwd_kernel<1>, grid, dim3(256), 0, s, a);
  else if (nchl == 2) hipLaunchKernelGGL(dense_cosine_loss_bwd_kernel<2>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(dense_cosine_loss_bwd_kernel<DSL_MAX_CHUNKS>, grid, dim3(256), 0, s, a);
  return vfs_check_launch("dense_cosine_loss_bwd");
}
