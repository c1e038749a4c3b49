// Layout conversion, weight packing, pooling, cosine loss and SGD kernels (HBM / latency bound).
#include "vfs_ops.h"

// ------------------------------------------------------------------ input frames
// reference layout: imgs[b][v][c][t][h][w] fp32 (pipelines/formating.py:248-258), view v is
// video2images(imgs[:, v]) = frames ordered (b, t)  (common/utils.py:45-53)
__global__ __launch_bounds__(256) void imgs_to_nhwc4_kernel(const float* __restrict__ imgs, bf16_t* __restrict__ out,
                                                            int B, int V, int T, int H, int W, int Wp) {
  const long long total = (long long)V * B * T * H * Wp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    long long p = i;
    const int w = (int)(p % Wp); p /= Wp;
    const int h = (int)(p % H); p /= H;
    const int t = (int)(p % T); p /= T;
    const int b = (int)(p % B);
    const int v = (int)(p / B);
    u32x2 pk = {0u, 0u};
    if (w < W) {
      const size_t plane = (size_t)T * H * W;
      const size_t base = (((size_t)b * V + v) * 3) * plane + ((size_t)t * H + h) * W + w;
      pk.x = pack2bf(imgs[base], imgs[base + plane]);
      pk.y = pack2bf(imgs[base + 2 * plane], 0.f);
    }
    st8(out + (size_t)i * 4, pk);
  }
}
int vfs_imgs_to_nhwc4_launch(const float* imgs, bf16_t* out, int B, int V, int T, int H, int W, int Wp, hipStream_t s) {
  long long total = (long long)V * B * T * H * Wp;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(imgs_to_nhwc4_kernel, dim3((int)blocks), dim3(256), 0, s, imgs, out, B, V, T, H, W, Wp);
  return vfs_check_launch("imgs_to_nhwc4");
}

// ------------------------------------------------------------------ weight packing
// fp32 master weights [Cout][Cin][T] (T = KH*KW) -> bf16 wf [Cout][T][Cin] (forward operand) and
// wd [Cin][T][Cout] (dgrad operand), every step after the optimizer.  A workgroup transposes one
// TC x TC (cout x cin) tile through LDS: whole contiguous row segments in (coalesced), 2 packed
// elements (4 bytes) per lane out along cin for wf and along cout for wd.  T is 1 or 9 for every
// layer but the stem (kind 1: [64][3][7][7] -> [64][8][8][4], a few thousand elements).
#define PACK_TC 32
template <int T>
__device__ __forceinline__ void pack_tile(const PackDesc& d, int tile, bf16_t* sT, int KT) {
  constexpr int TC = PACK_TC;
  const int Tn = T > 0 ? T : KT;                  // taps (compile-time for the common cases)
  const int pitch = TC * Tn + 2;                  // bf16 elements per staged cout row (odd dword count)
  const int t = threadIdx.x;
  const int tiles_ci = (d.Cin + TC - 1) / TC;
  const int co0 = (tile / tiles_ci) * TC, ci0 = (tile - (tile / tiles_ci) * tiles_ci) * TC;
  const int ncout = min(TC, d.Cout - co0), ncin = min(TC, d.Cin - ci0);
  const int rowlen = ncin * Tn;
  // in: thread (row r = t / 32 + 8 i, k = t % 32 + 32 j) over the contiguous segment of each cout row
  for (int r = t >> 5; r < ncout; r += 8) {
    const float* src = d.w + ((size_t)(co0 + r) * d.Cin + ci0) * Tn;
    for (int k = t & 31; k < rowlen; k += 32) sT[r * pitch + k] = f2bf(src[k]);
  }
  __syncthreads();
  // wf[cout][tap][cin]: lane pair index = cin pair
  const int hp = (ncin + 1) >> 1;
  for (int q = t / 16; q < ncout * Tn; q += 16) {
    const int r = q / Tn, tap = q - r * Tn;
    const int cp = t & 15;
    if (cp < hp) {
      const int c = cp * 2;
      const bf16_t lo = sT[r * pitch + c * Tn + tap];
      bf16_t* dst = d.wf + ((size_t)(co0 + r) * Tn + tap) * d.Cin + ci0 + c;
      if (c + 1 < ncin && ((d.Cin | ci0) & 1) == 0) {
        const bf16_t hi = sT[r * pitch + (c + 1) * Tn + tap];
        *reinterpret_cast<uint32_t*>(dst) = (uint32_t)lo | ((uint32_t)hi << 16);
      } else {
        dst[0] = lo;
        if (c + 1 < ncin) dst[1] = sT[r * pitch + (c + 1) * Tn + tap];
      }
    }
  }
  if (d.wd) {   // wd[cin][tap][cout]: lane pair index = cout pair
    const int hq = (ncout + 1) >> 1;
    for (int q = t / 16; q < ncin * Tn; q += 16) {
      const int ci = q / Tn, tap = q - ci * Tn;
      const int rp = t & 15;
      if (rp < hq) {
        const int r = rp * 2;
        const bf16_t lo = sT[r * pitch + ci * Tn + tap];
        bf16_t* dst = d.wd + ((size_t)(ci0 + ci) * Tn + tap) * d.Cout + co0 + r;
        if (r + 1 < ncout && ((d.Cout | co0) & 1) == 0) {
          const bf16_t hi = sT[(r + 1) * pitch + ci * Tn + tap];
          *reinterpret_cast<uint32_t*>(dst) = (uint32_t)lo | ((uint32_t)hi << 16);
        } else {
          dst[0] = lo;
          if (r + 1 < ncout) dst[1] = sT[(r + 1) * pitch + ci * Tn + tap];
        }
      }
    }
  }
}


// Round 5: the two shapes that hold all but a few thousand of a ResNet's weights, with 16-byte global accesses and whole tiles in
// flight (the generic tile below moves 4 bytes per lane in two dependent phases: 1.9 TB/s over 305 MB, 164 us at the start of
// every ResNet-50 step).  T = 1, 64 | Cout, 64 | Cin: a 64 x 64 tile - wf is the converted row itself (8 bytes per lane straight
// from the registers), wd the transpose through LDS (a lane gathers 8 couts of one cin: 16-byte stores, 128-byte row segments).
// T = 9, 32 | Cout, 64 | Cin: a 32 x 64 x 9 tile - rows of 576 contiguous floats in, wf [cout][tap][64 cin] and wd [cin][tap][32 cout]
// gathered from the staged tile with 16-byte stores.
typedef __attribute__((ext_vector_type(2))) uint32_t pk_u32x2;
__device__ __forceinline__ void pack_tile_1x1_64(const PackDesc& d, int tile, bf16_t* sT) {
  constexpr int P = 66;                             // bf16 per staged row: 33 dwords (odd)
  const int t = threadIdx.x;
  const int tiles_ci = d.Cin >> 6;
  const int co0 = (tile / tiles_ci) << 6, ci0 = (tile % tiles_ci) << 6;
  const int r0 = t >> 4, c4 = (t & 15) << 2;
  f32x4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(d.w + (size_t)(co0 + r0 + 16 * i) * d.Cin + ci0 + c4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + 16 * i;
    const uint32_t lo = pack2bf(v[i][0], v[i][1]), hi = pack2bf(v[i][2], v[i][3]);
    *reinterpret_cast<pk_u32x2*>(d.wf + (size_t)(co0 + r) * d.Cin + ci0 + c4) = (pk_u32x2){lo, hi};
    *reinterpret_cast<uint32_t*>(&sT[r * P + c4]) = lo;
    *reinterpret_cast<uint32_t*>(&sT[r * P + c4 + 2]) = hi;
  }
  if (!d.wd) return;
  __syncthreads();
  const int co8 = (t & 7) << 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ci = (t >> 3) + 32 * i;
    uint32_t w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w4[j] = (uint32_t)sT[(co8 + 2 * j) * P + ci] | ((uint32_t)sT[(co8 + 2 * j + 1) * P + ci] << 16);
    *reinterpret_cast<u32x4*>(d.wd + (size_t)(ci0 + ci) * d.Cout + co0 + co8) = (u32x4){w4[0], w4[1], w4[2], w4[3]};
  }
}
__device__ __forceinline__ void pack_tile_3x3_32x64(const PackDesc& d, int tile, bf16_t* sT) {
  constexpr int RL = 64 * 9, P = RL + 2;            // staged row: 576 elements + pad (289 dwords, odd)
  const int t = threadIdx.x;
  const int tiles_ci = d.Cin >> 6;
  const int co0 = (tile / tiles_ci) << 5, ci0 = (tile % tiles_ci) << 6;
  // in: 32 rows x 144 float4; lane task q = t + 256 i -> row q / 144, float4 q % 144
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x4 v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int q = t + 256 * (9 * half + i), r = q / 144, k4 = q - r * 144;
      v[i] = *reinterpret_cast<const f32x4*>(d.w + ((size_t)(co0 + r) * d.Cin + ci0) * 9 + 4 * k4);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int q = t + 256 * (9 * half + i), r = q / 144, k4 = q - r * 144;
      *reinterpret_cast<uint32_t*>(&sT[r * P + 4 * k4]) = pack2bf(v[i][0], v[i][1]);
      *reinterpret_cast<uint32_t*>(&sT[r * P + 4 * k4 + 2]) = pack2bf(v[i][2], v[i][3]);
    }
  }
  __syncthreads();
  // wf[cout][tap][cin]: 288 (cout, tap) rows of 64 cin = 8 lanes x 8 cin
  for (int q = t; q < 288 * 8; q += 256) {
    const int row = q >> 3, c8 = (q & 7) << 3, r = row / 9, tap = row - r * 9;
    const bf16_t* src = sT + r * P + c8 * 9 + tap;
    uint32_t w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w4[j] = (uint32_t)src[(2 * j) * 9] | ((uint32_t)src[(2 * j + 1) * 9] << 16);
    *reinterpret_cast<u32x4*>(d.wf + ((size_t)(co0 + r) * 9 + tap) * d.Cin + ci0 + c8) = (u32x4){w4[0], w4[1], w4[2], w4[3]};
  }
  if (!d.wd) return;
  // wd[cin][tap][cout]: 576 (cin, tap) rows of 32 cout = 4 lanes x 8 cout
  for (int q = t; q < 576 * 4; q += 256) {
    const int row = q >> 2, co8 = (q & 3) << 3;       // row = ci * 9 + tap = the staged column
    const bf16_t* src = sT + co8 * P + row;
    uint32_t w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w4[j] = (uint32_t)src[(2 * j) * P] | ((uint32_t)src[(2 * j + 1) * P] << 16);
    const int ci = row / 9, tap = row - ci * 9;
    *reinterpret_cast<u32x4*>(d.wd + ((size_t)(ci0 + ci) * 9 + tap) * d.Cout + co0 + co8) = (u32x4){w4[0], w4[1], w4[2], w4[3]};
  }
}

#define PACK_MAX_T 25
__global__ __launch_bounds__(256) void pack_weights_kernel(const PackDesc* __restrict__ table, int n) {
  __shared__ __attribute__((aligned(16))) bf16_t sT[PACK_TC * (PACK_TC * PACK_MAX_T + 2)];
  // uniform: which tensor does this workgroup's tile belong to
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].tile_start <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const PackDesc d = table[lo];
  const int tile = (int)blockIdx.x - d.tile_start;
  if (d.kind == 1) {   // stem, 256 elements per workgroup
    const long long total = (long long)d.Cout * d.Cin * d.KH * d.KW;
    long long e = (long long)tile * 256 + threadIdx.x;
    if (e < total) {
      const bf16_t v = f2bf(d.w[e]);
      const int s = (int)(e % d.KW); e /= d.KW;
      const int r = (int)(e % d.KH); e /= d.KH;
      const int cin = (int)(e % d.Cin);
      const int cout = (int)(e / d.Cin);
      d.wf[(((size_t)cout * 8 + r) * 8 + (s + 1)) * 4 + cin] = v;
    }
    return;
  }
  const int KT = d.KH * d.KW;
  if (d.kind == 2) { pack_tile_1x1_64(d, tile, sT); return; }
  if (d.kind == 3) { pack_tile_3x3_32x64(d, tile, sT); return; }
  if (KT == 1) pack_tile<1>(d, tile, sT, 1);
  else if (KT == 9) pack_tile<9>(d, tile, sT, 9);
  else pack_tile<0>(d, tile, sT, KT);
}
int vfs_pack_weights_launch(const PackDesc* table, int ntensors, long long total_tiles, hipStream_t s) {
  if (total_tiles <= 0 || ntensors <= 0) return VFS_OK;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)total_tiles), dim3(256), 0, s, table, ntensors);
  return vfs_check_launch("pack_weights");
}

// ------------------------------------------------------------------ global average pool
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int N, int HW,
                                                          int C) {
  const int cv = C >> 3;
  const int total = N * cv;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < total; v += gridDim.x * 256) {
    const int n = v / cv, c = (v - n * cv) * 8;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll 8
    for (int p = 0; p < HW; ++p) {       // eight independent loads in flight (the rolled loop waited for each pixel in turn)
      float f[8];
      unpack8(ld16(x + ((size_t)n * HW + p) * C + c), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += f[i];
    }
    const float inv = 1.0f / (float)HW;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= inv;
    st16(y + (size_t)n * C + c, pack8(acc));
  }
}
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const bf16_t* __restrict__ g, bf16_t* __restrict__ gx, int N, int HW,
                                                          int C) {
  const int cv = C >> 3;
  const long long total = (long long)N * HW * cv;
  const float inv = 1.0f / (float)HW;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const long long p = v / cv;
    const int c = (int)(v - p * cv) * 8;
    const int n = (int)(p / HW);
    float f[8];
    unpack8(ld16(g + (size_t)n * C + c), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] *= inv;
    st16(gx + (size_t)p * C + c, pack8(f));
  }
}
int vfs_avgpool_fwd_launch(const bf16_t* x, bf16_t* y, int N, int HW, int C, hipStream_t s) {
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3((N * (C >> 3) + 255) / 256), dim3(256), 0, s, x, y, N, HW, C);
  return vfs_check_launch("avgpool_fwd");
}
int vfs_avgpool_bwd_launch(const bf16_t* g, bf16_t* gx, int N, int HW, int C, hipStream_t s) {
  long long b = ((long long)N * HW * (C >> 3) + 255) / 256;
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3((int)(b > 4096 ? 4096 : b)), dim3(256), 0, s, g, gx, N, HW, C);
  return vfs_check_launch("avgpool_bwd");
}

// db[c] += sum_m dy[m][c]   (64 channels x 4 row-slices per workgroup, fixed-order combine)
__global__ __launch_bounds__(256) void bias_grad_kernel(const bf16_t* __restrict__ dy, float* __restrict__ db, int M, int C) {
  __shared__ float sh[4][64];
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float s = 0.f;
  if (c < C)
    for (int m = sl; m < M; m += 4) s += bf2f(dy[(size_t)m * C + c]);
  sh[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && c < C) db[c] += (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]);
}
int vfs_bias_grad_launch(const bf16_t* dy, float* db, int M, int C, hipStream_t s) {
  hipLaunchKernelGGL(bias_grad_kernel, dim3((C + 63) / 64), dim3(256), 0, s, dy, db, M, C);
  return vfs_check_launch("bias_grad");
}

// ------------------------------------------------------------------ cosine loss
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
// one wave per (k, i):  loss[k][i] = w * (0.5*L(p1[i], z2[j]) + 0.5*L(p2[j], z1[i])),  j = roll_k(i)
__global__ __launch_bounds__(64) void cosine_loss_fwd_kernel(LossArgs a) {
  const int i = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  const int j = roll_src(i, a.T, k);
  float d1 = 0.f, d2 = 0.f, np1 = 0.f, nz2 = 0.f, np2 = 0.f, nz1 = 0.f;
#pragma unroll 8
  for (int c = lane; c < a.C; c += 64) {
    const float p1 = bf2f(a.p1[(size_t)i * a.C + c]), z1 = bf2f(a.z1[(size_t)i * a.C + c]);
    const float p2 = bf2f(a.p2[(size_t)j * a.C + c]), z2 = bf2f(a.z2[(size_t)j * a.C + c]);
    d1 += p1 * z2; d2 += p2 * z1;
    np1 += p1 * p1; nz2 += z2 * z2; np2 += p2 * p2; nz1 += z1 * z1;
  }
  d1 = wave_sum(d1); d2 = wave_sum(d2);
  np1 = wave_sum(np1); nz2 = wave_sum(nz2); np2 = wave_sum(np2); nz1 = wave_sum(nz1);
  if (lane == 0) {
    const float eps = 1e-12f;
    const float c1 = d1 / (fmaxf(sqrtf(np1), eps) * fmaxf(sqrtf(nz2), eps));
    const float c2 = d2 / (fmaxf(sqrtf(np2), eps) * fmaxf(sqrtf(nz1), eps));
    const float l1 = a.negative ? -c1 : 2.f - 2.f * c1;
    const float l2 = a.negative ? -c2 : 2.f - 2.f * c2;
    a.loss[(size_t)k * a.N + i] = (0.5f * l1 + 0.5f * l2) * a.weight;
  }
}
// one wave per (view, i): gradient wrt p (z is detached in the reference)
//   view 0: dp1[i] = sum_k gloss[k][i]      * w/2 * dL/da (a = p1[i], b = z2[roll_k(i)])
//   view 1: dp2[j] = sum_k gloss[k][inv_k(j)] * w/2 * dL/da (a = p2[j], b = z1[inv_k(j)])
//   dL/da = coef * (bhat - cos * ahat) / max(|a|, eps),  coef = -2 (or -1 when negative)
__global__ __launch_bounds__(64) void cosine_loss_bwd_kernel(LossArgs a) {
  const int i = blockIdx.x, view = blockIdx.y, lane = threadIdx.x;
  const bf16_t* A = view == 0 ? a.p1 : a.p2;
  const bf16_t* Bz = view == 0 ? a.z2 : a.z1;
  bf16_t* out = view == 0 ? a.dp1 : a.dp2;
  const float eps = 1e-12f, coef = a.negative ? -1.f : -2.f;
  float na = 0.f;
#pragma unroll 8
  for (int c = lane; c < a.C; c += 64) { const float v = bf2f(A[(size_t)i * a.C + c]); na += v * v; }
  na = fmaxf(sqrtf(wave_sum(na)), eps);
  const int bvid = i / a.T, t = i - bvid * a.T;
  constexpr int MAXC = 32;  // supports C <= 2048
  float acc[MAXC];
#pragma unroll
  for (int q = 0; q < MAXC; ++q) acc[q] = 0.f;
  for (int k = 0; k < a.K; ++k) {
    int u, gi;
    if (view == 0) { u = t - k; if (u < 0) u += a.T; gi = i; }        // partner = roll_k(i), loss index i
    else { u = t + k; if (u >= a.T) u -= a.T; gi = bvid * a.T + u; }  // p2[i] is paired with loss index inv_k(i)
    const int j = bvid * a.T + u;
    float nb = 0.f, dot = 0.f;
#pragma unroll 8
    for (int c = lane; c < a.C; c += 64) {
      const float av = bf2f(A[(size_t)i * a.C + c]), bv = bf2f(Bz[(size_t)j * a.C + c]);
      nb += bv * bv; dot += av * bv;
    }
    nb = fmaxf(sqrtf(wave_sum(nb)), eps);
    const float cs = wave_sum(dot) / (na * nb);
    const float gs = a.gloss[(size_t)k * a.N + gi] * a.weight * 0.5f * coef / na;
#pragma unroll
    for (int q = 0; q < MAXC; ++q) {       // loads without a per-lane condition (index clamped, the update is masked): they batch
      const int c = lane + q * 64, cc = c < a.C ? c : lane;
      const float av = bf2f(A[(size_t)i * a.C + cc]), bv = bf2f(Bz[(size_t)j * a.C + cc]);
      const float upd = gs * (bv / nb - cs * av / na);
      acc[q] += c < a.C ? upd : 0.f;
    }
  }
#pragma unroll
  for (int q = 0; q < MAXC; ++q) {
    const int c = lane + q * 64;
    if (c < a.C) out[(size_t)i * a.C + c] = f2bf(acc[q]);
  }
}
// _parse_losses (trackers/base.py:76-110) for the K unreduced loss rows of one step: means[k] = mean_i loss[k][i],
// means[K] = their sum ('loss').  One wave, fixed summation order, double accumulation.
__global__ __launch_bounds__(64) void loss_means_kernel(const float* __restrict__ loss, float* __restrict__ means, int K, int N) {
  const int lane = threadIdx.x;
  double total = 0.0;
  for (int k = 0; k < K; ++k) {
    double acc = 0.0;
    for (int i = lane; i < N; i += 64) acc += (double)loss[(size_t)k * N + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    const float m = (float)(acc / (double)N);
    if (lane == 0) means[k] = m;
    total += (double)m;
  }
  if (lane == 0) means[K] = (float)total;
}
int vfs_loss_means_launch(const float* loss, float* means, int K, int N, hipStream_t s) {
  if (K <= 0 || N <= 0) return vfs_set_error(VFS_ERR_SHAPE, "loss_means: empty");
  hipLaunchKernelGGL(loss_means_kernel, dim3(1), dim3(64), 0, s, loss, means, K, N);
  return vfs_check_launch("loss_means");
}
int vfs_cosine_loss_fwd_launch(const LossArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(cosine_loss_fwd_kernel, dim3(a.N, a.K), dim3(64), 0, s, a);
  return vfs_check_launch("cosine_loss_fwd");
}
int vfs_cosine_loss_bwd_launch(const LossArgs& a, hipStream_t s) {
  if (a.C > 2048) return vfs_set_error(VFS_ERR_SHAPE, "cosine_loss_bwd: C > 2048");
  hipLaunchKernelGGL(cosine_loss_bwd_kernel, dim3(a.N, 2), dim3(64), 0, s, a);
  return vfs_check_launch("cosine_loss_bwd");
}

// ------------------------------------------------------------------ SGD
// torch.optim.SGD (configs/*:134): g += wd*p ; buf = momentum*buf + g ; p -= lr*buf
// (a zero-initialised buf reproduces torch's "buf = g" on the first step)
// CLIP: the gradient is g * (*clip) first - torch.nn.utils.clip_grad_norm_'s in-place scaling (mmcv OptimizerHook.clip_grads,
// apis/train.py:85-93) folded into the update; the stored gradients stay as they are.  The product is handed on through an empty
// asm: it is rounded on its own, and the compiler sees the rest of the update exactly as it sees the unclipped one (a value it knows
// nothing about in place of a loaded one), so its contraction choices are the same and a coefficient of 1.0 gives the unclipped bits.
template <bool CLIP>
__device__ __forceinline__ float sgd_grad(float g, float c) {
  if (!CLIP) return g;
  float gs = g * c;
#ifndef VFS_EMU
  asm("" : "+v"(gs));
#endif
  return gs;
}
template <bool CLIP>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  long long n, float lr, float momentum, float wd, const float* __restrict__ clip,
                                                  const unsigned long long* __restrict__ skip) {
  if (skip && *skip) return;      // a poisoned step (failed SyncBN exchange, vfs_p2p.h) leaves weights and momentum alone
  const float c = CLIP ? *clip : 1.0f;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 bv = reinterpret_cast<f32x4*>(buf)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float gg = sgd_grad<CLIP>(gv[q], c) + wd * pv[q];
      bv[q] = momentum * bv[q] + gg;
      pv[q] -= lr * bv[q];
    }
    reinterpret_cast<f32x4*>(buf)[i] = bv;
    reinterpret_cast<f32x4*>(p)[i] = pv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    const float gg = sgd_grad<CLIP>(g[i], c) + wd * p[i];
    buf[i] = momentum * buf[i] + gg;
    p[i] -= lr * buf[i];
  }
}
int vfs_sgd_launch(float* p, const float* g, float* buf, long long n, float lr, float momentum, float wd, const float* clip,
                   const unsigned long long* skip, hipStream_t s) {
  long long b = ((n >> 2) + 255) / 256;
  const dim3 grid((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)));
  if (clip) hipLaunchKernelGGL(sgd_kernel<true>, grid, dim3(256), 0, s, p, g, buf, n, lr, momentum, wd, clip, skip);
  else hipLaunchKernelGGL(sgd_kernel<false>, grid, dim3(256), 0, s, p, g, buf, n, lr, momentum, wd, clip, skip);
  return vfs_check_launch("sgd");
}

// ------------------------------------------------------------------ table-driven optimizer step (vfs_opt_step_table)
// mmcv's build_optimizer with paramwise_cfg (configs/r*_*.py:134-136, apis/train.py:72) gives every parameter a param group of its
// own; torch then updates tensor by tensor.  Here one update launch sweeps the whole arena: the segment map (opt_table.h) says
// which 16-byte vectors are trainable and which group they belong to.  The groups' hyperparameter rows are kernel arguments of the
// update itself while they fit (VFS_OPT_WRITE_GROUPS groups); more groups go through a small device table that
// opt_table_write_kernel fills on the launch stream right before, again from kernel arguments.  Either way there is no host copy to
// wait for, and a changed lr is in force at the next step.  Words outside every segment - frozen parameters, the padding between
// parameters - are neither read nor written.
// A workgroup pass covers one VFS_OPT_CHUNK_WORDS chunk.  The chunk's entry index and the segment it names are uniform loads; when
// that segment holds the whole chunk (all but the chunks with a parameter edge in them: ~350 of the 37 315 of a ResNet-50), the
// group and its row are uniform too and the lanes go straight to their streaming loads.  Only a chunk with an edge in it walks
// the map per lane - from the entry index past the segments of this chunk at the most.
// SGD:   g' = clip g + wd p;  buf = momentum buf + g';  p -= lr (nesterov ? g' + momentum buf : buf)      (sgd_kernel's expressions)
// Adam:  g' = clip g + wd p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// AdamW: p *= 1 - lr wd first, g' = clip g                                                                  (adam_kernel's expressions)
struct OptHyperChunk { float v[VFS_OPT_WRITE_GROUPS * VFS_OPT_HYPER]; };
__global__ __launch_bounds__(256) void opt_table_write_kernel(OptHyperChunk c, float* __restrict__ table, int count) {
  for (int i = threadIdx.x; i < count; i += 256) table[i] = c.v[i];
}
template <int KIND, bool NEST, bool CLIP>
__device__ __forceinline__ void opt_update(float& p, float g, float& a, float& b, const float* h, float c) {
  const float lr = h[0], wd = h[1];
  if (KIND == VFS_OPT_SGD) {
    const float momentum = h[2];
    const float gg = sgd_grad<CLIP>(g, c) + wd * p;
    a = momentum * a + gg;
    if (NEST) p -= lr * (gg + momentum * a);
    else p -= lr * a;
  } else {
    const float b1 = h[2], b2 = h[3], eps = h[4], bc1 = h[5], bc2s = h[6];
    float gi = sgd_grad<CLIP>(g, c);
    if (KIND == VFS_OPT_ADAMW) p *= 1.f - lr * wd;
    else if (wd != 0.f) gi += wd * p;
    a = b1 * a + (1.f - b1) * gi;
    b = b2 * b + (1.f - b2) * gi * gi;
    p -= (lr / bc1) * (a / (sqrtf(b) / bc2s + eps));
  }
}
// vector i of a segment {.., end4, group, tail}: a whole vector, or the segment's last, partial one (its `tail` words one by one)
template <int KIND, bool NEST, bool CLIP>
__device__ __forceinline__ void opt_vector(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2,
                                           long long i, int end4, int tail, const float* __restrict__ row, float c) {
  float h[7];
#pragma unroll
  for (int q = 0; q < (KIND == VFS_OPT_SGD ? 3 : 7); ++q) h[q] = row[q];
  if (i < end4) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 av = reinterpret_cast<f32x4*>(s1)[i];
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (KIND != VFS_OPT_SGD) bv = reinterpret_cast<f32x4*>(s2)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float pq = pv[q], aq = av[q], bq = bv[q];
      opt_update<KIND, NEST, CLIP>(pq, gv[q], aq, bq, h, c);
      pv[q] = pq; av[q] = aq; bv[q] = bq;
    }
    reinterpret_cast<f32x4*>(s1)[i] = av;
    if (KIND != VFS_OPT_SGD) reinterpret_cast<f32x4*>(s2)[i] = bv;
    reinterpret_cast<f32x4*>(p)[i] = pv;
  } else {
    for (int q = 0; q < tail; ++q) {
      const long long w = (i << 2) + q;
      float bw = KIND != VFS_OPT_SGD ? s2[w] : 0.f;
      opt_update<KIND, NEST, CLIP>(p[w], g[w], s1[w], bw, h, c);
      if (KIND != VFS_OPT_SGD) s2[w] = bw;
    }
  }
}
// table: the device table, or nullptr when the rows are `rows` itself (ngroups <= VFS_OPT_WRITE_GROUPS).  With a table `rows` is
// dead: it still travels (one instantiation per kind, and only the rows that are indexed are ever loaded from the argument block).
template <int KIND, bool NEST, bool CLIP>
__global__ __launch_bounds__(256) void opt_table_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                        float* __restrict__ s2, long long nvec, const int* __restrict__ map, int nseg,
                                                        const float* __restrict__ table, const float* __restrict__ clip,
                                                        const unsigned long long* __restrict__ skip, OptHyperChunk rows) {
  if (skip && *skip) return;      // as sgd_kernel: a poisoned step leaves weights and state alone
  const float c = CLIP ? *clip : 1.0f;
  const float* hyper = table ? table : rows.v;
  const int* first = map + 4 * (long long)nseg;
  for (long long base = (long long)blockIdx.x * 256; base < nvec; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    const int s0 = first[base >> 8];
    if (s0 == nseg) continue;                   // nothing trainable from here to the end of the arena
    int begin4 = map[4 * s0], end4 = map[4 * s0 + 1], group = map[4 * s0 + 2], tail = map[4 * s0 + 3];
    if (begin4 <= base && base + 256 <= end4) {      // the whole chunk inside one segment: everything above is uniform
      opt_vector<KIND, NEST, CLIP>(p, g, s1, s2, i, end4, 0, hyper + group * VFS_OPT_HYPER, c);
      continue;
    }
    if (i >= nvec) continue;
    int s = s0;
    while ((long long)end4 + (tail != 0) <= i) {      // a chunk with a parameter edge in it: the lane's own walk
      if (++s == nseg) break;
      begin4 = map[4 * s]; end4 = map[4 * s + 1]; group = map[4 * s + 2]; tail = map[4 * s + 3];
    }
    if (s == nseg || begin4 > i) continue;      // frozen or padding
    opt_vector<KIND, NEST, CLIP>(p, g, s1, s2, i, end4, tail, hyper + group * VFS_OPT_HYPER, c);
  }
}
template <int KIND, bool NEST>
static void opt_table_launch_kind(dim3 grid, hipStream_t s, float* p, const float* g, float* s1, float* s2, long long nvec, const int* map,
                                  int nseg, const float* table, const float* clip, const unsigned long long* skip, const OptHyperChunk& rows) {
  if (clip) hipLaunchKernelGGL((opt_table_kernel<KIND, NEST, true>), grid, dim3(256), 0, s, p, g, s1, s2, nvec, map, nseg, table, clip, skip, rows);
  else hipLaunchKernelGGL((opt_table_kernel<KIND, NEST, false>), grid, dim3(256), 0, s, p, g, s1, s2, nvec, map, nseg, table, clip, skip, rows);
}
// hyper: HOST memory, ngroups x VFS_OPT_HYPER floats {lr, wd, momentum} or {lr, wd, beta1, beta2, eps}; the bias corrections of
// `step` are worked out here (as vfs_adam_launch does) and travel in slots 5 and 6
int vfs_opt_table_launch(int kind, float* p, const float* g, float* s1, float* s2, long long n, const int* map, int nseg,
                         const float* hyper, int ngroups, float* table, int nesterov, int step, const float* clip,
                         const unsigned long long* skip, hipStream_t s) {
  const bool by_value = ngroups <= VFS_OPT_WRITE_GROUPS;      // the rows ride with the update launch: nothing in front of it
  OptHyperChunk ch;
  for (int g0 = 0; g0 < ngroups; g0 += VFS_OPT_WRITE_GROUPS) {
    const int ng = ngroups - g0 < VFS_OPT_WRITE_GROUPS ? ngroups - g0 : VFS_OPT_WRITE_GROUPS;
    for (int k = 0; k < ng; ++k) {
      const float* src = hyper + (size_t)(g0 + k) * VFS_OPT_HYPER;
      float* dst = ch.v + k * VFS_OPT_HYPER;
      for (int q = 0; q < VFS_OPT_HYPER; ++q) dst[q] = q < 5 ? src[q] : 0.f;
      if (kind != VFS_OPT_SGD) {
        dst[5] = 1.f - powf(src[2], (float)step);
        dst[6] = sqrtf(1.f - powf(src[3], (float)step));
      }
    }
    for (int k = ng * VFS_OPT_HYPER; k < VFS_OPT_WRITE_GROUPS * VFS_OPT_HYPER; ++k) ch.v[k] = 0.f;
    if (!by_value)
      hipLaunchKernelGGL(opt_table_write_kernel, dim3(1), dim3(256), 0, s, ch, table + (size_t)g0 * VFS_OPT_HYPER, ng * VFS_OPT_HYPER);
  }
  if (int rc = vfs_check_launch("opt_step_table")) return rc;
  const float* dev_rows = by_value ? nullptr : table;
  const long long nvec = (n + 3) >> 2;
  long long b = (nvec + 255) / 256;
  const dim3 grid((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)));
  if (kind == VFS_OPT_SGD) {
    if (nesterov) opt_table_launch_kind<VFS_OPT_SGD, true>(grid, s, p, g, s1, s2, nvec, map, nseg, dev_rows, clip, skip, ch);
    else opt_table_launch_kind<VFS_OPT_SGD, false>(grid, s, p, g, s1, s2, nvec, map, nseg, dev_rows, clip, skip, ch);
  } else if (kind == VFS_OPT_ADAM) opt_table_launch_kind<VFS_OPT_ADAM, false>(grid, s, p, g, s1, s2, nvec, map, nseg, dev_rows, clip, skip, ch);
  else opt_table_launch_kind<VFS_OPT_ADAMW, false>(grid, s, p, g, s1, s2, nvec, map, nseg, dev_rows, clip, skip, ch);
  return vfs_check_launch("opt_step_table");
}
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ p, long long n, float scale) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] *= scale;
}
int vfs_scale_launch(float* p, long long n, float scale, hipStream_t s) {
  long long b = (n + 255) / 256;
  hipLaunchKernelGGL(scale_kernel, dim3((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b))), dim3(256), 0, s, p, n, scale);
  return vfs_check_launch("scale");
}
// x *= *coef, the scalar read from device memory when the kernel runs (vfs_amd.clip_grad_norm_: the coefficient never visits the host)
__global__ __launch_bounds__(256) void scale_by_kernel(float* __restrict__ p, long long n, const float* __restrict__ coef) {
  const float c = *coef;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] *= c;
    reinterpret_cast<f32x4*>(p)[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) p[(n4 << 2) + threadIdx.x] *= c;
}
int vfs_scale_by_launch(float* p, long long n, const float* coef, hipStream_t s) {
  long long b = ((n >> 2) + 255) / 256;
  hipLaunchKernelGGL(scale_by_kernel, dim3((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b))), dim3(256), 0, s, p, n, coef);
  return vfs_check_launch("scale_by");
}

// ------------------------------------------------------------------ gradient norm (torch.nn.utils.clip_grad_norm_)
// One streaming pass over a contiguous fp32 range: VFS_GRAD_NORM_ROWS workgroups (four per CU, every lane with up to four 16-byte
// loads in flight - the grid is sized to the chip, a range of any length is swept by its stride loop), squares accumulated in
// double, one double per workgroup written to ITS row of `rows`.  No floating-point atomics anywhere: a row's value depends on
// the range alone, so the norm is the same bits on every run.  accumulate != 0 combines with what the row holds (the trainable
// ranges of a model with frozen parameters in the middle are several segments: first launch overwrites, the others add).
// INF: maximum of |g| instead; nan_max hands a NaN on from either side, as torch's max does.
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }
template <bool INF>
__device__ __forceinline__ double norm_combine(double a, double b) { return INF ? nan_max(a, b) : a + b; }
// workgroup total of 256 threads, fixed order (xor butterfly per wave, then the four waves in index order); valid in thread 0
template <bool INF>
__device__ __forceinline__ double norm_block_total(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = norm_combine<INF>(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return norm_combine<INF>(norm_combine<INF>(norm_combine<INF>(sh[0], sh[1]), sh[2]), sh[3]);
}
template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long long n, double* __restrict__ rows,
                                                                int accumulate) {
  __shared__ double sh[4];
  const long long n4 = n >> 2;
  double acc = 0.0;
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = INF ? nan_max(acc, (double)fabsf(v[q])) : acc + (double)v[q] * (double)v[q];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = g[(n4 << 2) + threadIdx.x];
    acc = INF ? nan_max(acc, (double)fabsf(v)) : acc + (double)v * (double)v;
  }
  const double total = norm_block_total<INF>(acc, sh);
  if (threadIdx.x == 0) rows[blockIdx.x] = accumulate ? norm_combine<INF>(rows[blockIdx.x], total) : total;
}
int vfs_grad_norm_partial_launch(const float* g, long long n, int inf_norm, double* rows, int accumulate, hipStream_t s) {
  if (inf_norm) hipLaunchKernelGGL(grad_norm_partial_kernel<true>, dim3(VFS_GRAD_NORM_ROWS), dim3(256), 0, s, g, n, rows, accumulate);
  else hipLaunchKernelGGL(grad_norm_partial_kernel<false>, dim3(VFS_GRAD_NORM_ROWS), dim3(256), 0, s, g, n, rows, accumulate);
  return vfs_check_launch("grad_norm_partial");
}
// One workgroup: thread t combines rows 4t .. 4t+3 in index order, then the fixed tree above.  out[0] = the norm,
// out[1] = torch's clip_coef_clamped = min(1, max_norm / (norm + 1e-6)); a NaN norm gives a NaN coefficient (NaN > 1 is false).
// A launch of its own rather than the last-arriving workgroup of the reduction: with several segments only the last launch
// could finish, and the second launch (a dependent boundary, under 2 us) needs no ticket word and no agent-scope hand-off.
template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ rows, double max_norm, float* __restrict__ out) {
  static_assert(VFS_GRAD_NORM_ROWS == 4 * 256, "four rows per thread");
  __shared__ double sh[4];
  const int t = threadIdx.x;
  double acc = rows[4 * t];
#pragma unroll
  for (int q = 1; q < 4; ++q) acc = norm_combine<INF>(acc, rows[4 * t + q]);
  const double total = norm_block_total<INF>(acc, sh);
  if (t == 0) {
    const double norm = INF ? total : sqrt(total);
    double c = max_norm / (norm + 1e-6);
    if (c > 1.0) c = 1.0;
    out[0] = (float)norm;
    out[1] = (float)c;
  }
}
int vfs_grad_norm_finish_launch(const double* rows, int inf_norm, double max_norm, float* out, hipStream_t s) {
  if (inf_norm) hipLaunchKernelGGL(grad_norm_finish_kernel<true>, dim3(1), dim3(256), 0, s, rows, max_norm, out);
  else hipLaunchKernelGGL(grad_norm_finish_kernel<false>, dim3(1), dim3(256), 0, s, rows, max_norm, out);
  return vfs_check_launch("grad_norm_finish");
}

// bf16 gradient buckets for the data-parallel all-reduce (opt-in: halves the xGMI traffic of the 152.8 MB ResNet-50 gradient;
// the reference's DDP reduces fp32): dst = bf16(src * scale) before the collective, dst = float(src) after it
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long long n, float scale) {
  const long long n8 = n >> 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + i * 8), b = *reinterpret_cast<const f32x4*>(src + i * 8 + 4);
    const float f[8] = {a[0] * scale, a[1] * scale, a[2] * scale, a[3] * scale, b[0] * scale, b[1] * scale, b[2] * scale, b[3] * scale};
    st16(dst + i * 8, pack8(f));
  }
  if (blockIdx.x == 0)
    for (long long i = n8 * 8 + threadIdx.x; i < n; i += 256) dst[i] = f2bf(src[i] * scale);
}
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, long long n) {
  const long long n8 = n >> 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    float f[8];
    unpack8(ld16(src + i * 8), f);
    *reinterpret_cast<f32x4*>(dst + i * 8) = (f32x4){f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(dst + i * 8 + 4) = (f32x4){f[4], f[5], f[6], f[7]};
  }
  if (blockIdx.x == 0)
    for (long long i = n8 * 8 + threadIdx.x; i < n; i += 256) dst[i] = bf2f(src[i]);
}
int vfs_f32_to_bf16_launch(const float* src, bf16_t* dst, long long n, float scale, hipStream_t s) {
  if (((size_t)src & 15) || ((size_t)dst & 15)) return vfs_set_error(VFS_ERR_ARG, "f32_to_bf16: 16-byte aligned buffers");
  long long b = ((n >> 3) + 255) / 256;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b))), dim3(256), 0, s, src, dst, n, scale);
  return vfs_check_launch("f32_to_bf16");
}
int vfs_bf16_to_f32_launch(const bf16_t* src, float* dst, long long n, hipStream_t s) {
  if (((size_t)src & 15) || ((size_t)dst & 15)) return vfs_set_error(VFS_ERR_ARG, "bf16_to_f32: 16-byte aligned buffers");
  long long b = ((n >> 3) + 255) / 256;
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b))), dim3(256), 0, s, src, dst, n);
  return vfs_check_launch("bf16_to_f32");
}
