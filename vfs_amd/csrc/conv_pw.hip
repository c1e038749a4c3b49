// Pointwise (1x1, stride 1) convolution forward / dgrad as a PERSISTENT, producer/consumer-split GEMM for gfx950:
//
//   out[pixel][chan] = sum_k Wt[chan][k] * X[pixel][k]    (+ the epilogues of vfs_igemm_epi.h)
//
// Replaces the 1x1 torch conv2d calls of the reference's Bottleneck (mmaction/models/backbones/resnet.py:163-230: conv1, conv3,
// downsample through mmcv ConvModule) and their autograd dgrads - 28 % of the ResNet-50 train step's kernel time.
//
// Why a second kernel next to conv_igemm.hip (round 5; numbers in MEASUREMENTS.md): the one-tile-per-workgroup kernels pay, per
// 128 x 128 tile, a launch-to-first-load prologue, a pipeline fill, and a store tail during which the workgroup holds its LDS and
// registers but moves nothing - 2-3x the HBM / L2 roof on every 1x1 layer.  Here
//   * ONE workgroup per CU lives for the whole launch and walks a contiguous range of (pixel block, channel tile) tiles
//     (XCD-aware: the ranges of one XCD are neighbours, the channel tiles of a pixel block meet in one L2);
//   * waves 4-7 are LOADERS: they only issue LDS-DMA pieces (buffer_load ... lds, 1 KB each) of the flat (tile, K-step) sequence
//     into a ring of RING stages [W tile BC x 64 | X tile 128 x 64], as far ahead as the ring allows - across tile boundaries, so
//     the operands of tile i + 1 land while tile i's epilogue runs; their vmcnt holds DMA pieces only, so "step s has landed" is
//     an exact count;
//   * waves 0-3 are CONSUMERS: MFMA K-steps out of the ring, then the shared epilogue (own LDS stage, so it does not touch the
//     ring); their output stores are never waited for - they drain under the next tile's K-steps.
// Every wave of the workgroup executes the SAME number of s_barrier: one per K-step (B: stage landed / previous stage free), one
// after a tile's last K-step (T: the last stage is free) and the epilogue's own (the loaders mirror them).
#include "vfs_igemm_epi.h"
#include "vfs_ops.h"
#include "vfs_bn.h"


template <int BC, bool FBN>
constexpr int pw_ring_stages() {
  constexpr int stage = (BC + 128) * 64 * 2, fixed = igemm_stage_elems<BC, FBN>() * 2 + 2 * BC * 2 * 4 + 512;
  constexpr int n = (160 * 1024 - fixed) / stage;
  return n > 5 ? 5 : n;
}

template <int BC, int MODE, bool FBN>
__global__ __launch_bounds__(512) void conv_pw_kernel(ConvArgs a) {
  constexpr int BP = 128, WC = BC / 2, TM = WC / 16, TN = 4;
  constexpr int STAGE = (BC + BP) * 64;                 // bf16 elements of one ring stage: [W tile | X tile]
  constexpr int RING = pw_ring_stages<BC, FBN>();
  static_assert(RING >= 3, "ring too short");
  constexpr int XQ = 4, WQ = BC / 32, LPW = XQ + WQ;    // DMA pieces per loader wave and K-step
  constexpr bool HAS_STATS = (MODE == GATHER_FWD);
  __shared__ __attribute__((aligned(16))) bf16_t ring[RING * STAGE];
  __shared__ __attribute__((aligned(16))) bf16_t stage[igemm_stage_elems<BC, FBN>()];
  __shared__ float sRed[2][BC][2];

  const ConvGeom g = a.g;
  const int lane = threadIdx.x & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Mc = g.M;
  const int npb = (Mc + BP - 1) / BP, ncb = (a.Cout + BC - 1) / BC, nk = g.Ktot >> 6;
  // this workgroup's tiles: a contiguous range of the (pixel block, channel tile) sequence, channel tile fastest; hardware
  // workgroup b runs on XCD b % 8 (observed, a speed matter only): the ranges of one XCD are neighbours
  int lw = blockIdx.x;
  {
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = lw & 7;
    if (a.xcd_swizzle) lw = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lw >> 3);
  }
  const long long T = (long long)npb * ncb;
  const int tile_begin = (int)(T * lw / gridDim.x), tile_end = (int)(T * (lw + 1) / gridDim.x);
  const int S = (tile_end - tile_begin) * nk;           // K-steps of this workgroup
  const int nsync = ((FBN && a.bn.partial != nullptr) ? 1 : 0) + ((HAS_STATS && a.stats != nullptr) ? 1 : 0);   // barriers inside igemm_epilogue

  if (wave_u >= 4) {
    // ------------------------------------------------ loaders
    const int lwv = wave_u - 4;
    const unsigned cbytes = (unsigned)g.C * 2u, kbytes = (unsigned)g.Ktot * 2u;
    unsigned xrow[XQ], xoff[XQ], xc16[XQ], wrow[WQ], woff[WQ], wc16[WQ];
#pragma unroll
    for (int q = 0; q < XQ; ++q) {      // lane l of a piece lands at piece_base + 16 l: it FETCHES the (row, chunk) whose swizzled slot that is
      const int slot = (lwv * XQ + q) * 64 + lane, row = slot >> 3, chunk = (slot & 7) ^ ((row >> 1) & 7);
      xrow[q] = row; xc16[q] = chunk * 16; xoff[q] = row * cbytes + chunk * 16;
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int slot = (lwv * WQ + q) * 64 + lane, row = slot >> 3, chunk = (slot & 7) ^ ((row >> 1) & 7);
      wrow[q] = row; wc16[q] = chunk * 16; woff[q] = row * kbytes + chunk * 16;
    }
    const vfs_rsrc_words xrw = vfs_make_rsrc_words(a.src, (unsigned)((size_t)g.N * g.H * g.W * g.C * 2));
    const vfs_rsrc_words wrw = vfs_make_rsrc_words(a.wgt, (unsigned)((size_t)a.Cout * g.Ktot * 2));
    int ipb = tile_begin / ncb, icb = tile_begin - ipb * ncb, ikt = 0, ist = 0, issued = 0;   // the NEXT step to issue
    auto issue = [&]() {
      const int m0 = ipb * BP, c0 = icb * BC;
      bf16_t* sW = ring + ist * STAGE;
      bf16_t* sX = sW + BC * 64;
      const unsigned sx = (unsigned)m0 * cbytes + (unsigned)ikt * 128u, sw = (unsigned)c0 * kbytes + (unsigned)ikt * 128u;
#pragma unroll
      for (int q = 0; q < XQ; ++q)      // rows past the ragged end re-fetch row 0 of the tile (their outputs are masked by the epilogue)
        vfs_dma16_async(xrw, sX + (lwv * XQ + q) * 512, m0 + (int)xrow[q] < Mc ? xoff[q] : xc16[q], sx);
#pragma unroll
      for (int q = 0; q < WQ; ++q)
        vfs_dma16_async(wrw, sW + (lwv * WQ + q) * 512, c0 + (int)wrow[q] < a.Cout ? woff[q] : wc16[q], sw);
      ++issued;
      ist = ist + 1 == RING ? 0 : ist + 1;
      if (++ikt == nk) {
        ikt = 0;
        if (++icb == ncb) { icb = 0; ++ipb; }
      }
    };
#pragma unroll 1
    for (int d = 0; d < RING; ++d)
      if (issued < S) issue();
    int kt = 0;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      // this wave's pieces of step s have landed: only the pieces of the `ahead` later steps already issued may be in flight
      const int ahead = issued - 1 - s;
      if (ahead >= 4) vfs_dma_wait<4 * LPW>();
      else if (ahead == 3) vfs_dma_wait<3 * LPW>();
      else if (ahead == 2) vfs_dma_wait<2 * LPW>();
      else if (ahead == 1) vfs_dma_wait<LPW>();
      else vfs_dma_wait<0>();
      __syncthreads();                        // B(s): everybody's pieces of step s have landed; the consumers are done with step s - 1
      if (kt > 0 && issued < S) issue();      // ... whose stage takes step s - 1 + RING (after a tile's last step: issued behind T below)
      if (++kt == nk) {
        kt = 0;
        __syncthreads();                      // T: the consumers are done with step s
        if (issued < S) issue();
        for (int e = 0; e < nsync; ++e) __syncthreads();   // the epilogue's barriers
      }
    }
    return;
  }

  // -------------------------------------------------- consumers
  const int wc = wave_u >> 1, wp = wave_u & 1;
  int pb = tile_begin / ncb, cb = tile_begin - pb * ncb, st = 0;
#pragma unroll 1
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    f32x4 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();                        // B(s)
      const bf16_t* sW = ring + st * STAGE;
      __builtin_amdgcn_sched_barrier(0);
      mma_kstep<TM, TN, false>(sW, sW + BC * 64, wc * WC, wp * 64, lane, acc);
      __builtin_amdgcn_sched_barrier(0);
      st = st + 1 == RING ? 0 : st + 1;
    }
    __syncthreads();                          // T
    igemm_epilogue<BC, MODE, FBN, true>(a, pb * BP, cb * BC, pb, Mc, 0, 0, g.Ho, g.Wo, acc, stage, sRed);
    if (++cb == ncb) { cb = 0; ++pb; }
  }
}

// ------------------------------------------------------------------ host side
static int pw_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
    else n = 256;
  }
  return n;
}

template <int BC, int MODE, bool FBN>
static int launch_pw(const ConvArgs& a, hipStream_t stream) {
  const long long T = (long long)((a.g.M + 127) / 128) * ((a.Cout + BC - 1) / BC);
  const int G = (int)(T < pw_cus() ? T : pw_cus());
  hipLaunchKernelGGL((conv_pw_kernel<BC, MODE, FBN>), dim3(G), dim3(512), 0, stream, a);
  return vfs_check_launch("conv_pw");
}

// a pure-GEMM problem (checked by the caller: 1x1, stride 1, no padding, K % 64 == 0, no split-K, tensors < 4 GiB): does the
// persistent kernel take it?
bool vfs_conv_pw_eligible(const ConvArgs& a, int mode) {
  if (!vfs_option_igemm_pw || (mode != GATHER_FWD && mode != GATHER_DGRAD)) return false;
  if (a.g.KH * a.g.KW != 1 || a.g.stride != 1 || a.g.pad != 0 || a.g.H != a.g.Ho || a.g.W != a.g.Wo || a.ksplit > 1) return false;
  if (a.bn.partial && mode != GATHER_DGRAD) return false;
  if (a.coarse_log2 > 0) return false;      // (the loaders mirror a fixed number of epilogue barriers)
  if (vfs_option_igemm_pw >= 2) return true;
  const int bc = a.Cout % 128 == 0 ? 128 : 64;
  const long long T = (long long)((a.g.M + 127) / 128) * ((a.Cout + bc - 1) / bc);
  return T >= vfs_option_igemm_pw_min_tiles;
}

int vfs_conv_pw_dispatch(const ConvArgs& a, int mode, hipStream_t stream) {
  const bool wide = a.Cout % 128 == 0;
  if (mode == GATHER_FWD) return wide ? launch_pw<128, GATHER_FWD, false>(a, stream) : launch_pw<64, GATHER_FWD, false>(a, stream);
  if (a.bn.partial) return wide ? launch_pw<128, GATHER_DGRAD, true>(a, stream) : launch_pw<64, GATHER_DGRAD, true>(a, stream);
  return wide ? launch_pw<128, GATHER_DGRAD, false>(a, stream) : launch_pw<64, GATHER_DGRAD, false>(a, stream);
}

// ------------------------------------------------------------------ skinny GEMM (the SimSiam head's Linear layers)
//   out[m][c] = sum_k X[m][k] * Wt[c][k]   (+bias[c]) (+add[m][c])      for M <= 128 rows
// Replaces nn.Linear forward / dgrad of the reference's SimSiamHead (mmaction/models/heads/sim_siam_head.py:78-111: projection
// and predictor MLPs on the pooled [B*T, 2048] features).  With 64 rows the implicit-GEMM tiling (128 pixels x 64 channels) has
// 32 workgroups on 256 CUs, each walking 32 dependent K-steps: 17-21 us for 8 MB of weights (1.4 us at the HBM roof).  Here a
// workgroup owns 16 output channels x 32 rows, its four waves each take a QUARTER of K with fragments loaded straight from global
// memory into MFMA operand registers (a lane's 16 bytes = 8 consecutive k of one row: exactly the 16x16x32 fragment) - no LDS
// stage, no barrier in the loop, many independent loads in flight - and meet once in LDS.  Cout / 16 x ceil(M / 32) workgroups.

__global__ __launch_bounds__(256) void conv_skinny_kernel(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float sAcc[4][2][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int M = a.g.M, K = a.g.Ktot, C = a.Cout;
  const int ncb = C >> 4;
  const int cb = blockIdx.x % ncb, mb = blockIdx.x / ncb;
  const int c0 = cb * 16, m0 = mb * 32;
  const int kq = K >> 2;                                  // K % 128 == 0: whole 32-deep steps per wave
  const bf16_t* wrow = a.wgt + (size_t)(c0 + lr) * K + wave * kq + lq * 8;
  const int r0 = m0 + lr < M ? m0 + lr : M - 1, r1 = m0 + 16 + lr < M ? m0 + 16 + lr : M - 1;   // rows past M: clamped, masked at the store
  const bf16_t* x0 = a.src + (size_t)r0 * K + wave * kq + lq * 8;
  const bf16_t* x1 = a.src + (size_t)r1 * K + wave * kq + lq * 8;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int steps = kq >> 5;
#pragma unroll 4
  for (int s = 0; s < steps; ++s) {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(wrow + s * 32);
    const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(x0 + s * 32);
    const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(x1 + s * 32);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b1, acc1, 0, 0, 0);
  }
  *reinterpret_cast<f32x4*>(&sAcc[wave][0][lane][0]) = acc0;
  *reinterpret_cast<f32x4*>(&sAcc[wave][1][lane][0]) = acc1;
  __syncthreads();
  if (wave < 2) {      // wave w finishes row tile w: lane = (channel quad lq, row lr); the K quarters add up in wave order
    f32x4 v = *reinterpret_cast<const f32x4*>(&sAcc[0][wave][lane][0]);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f32x4*>(&sAcc[w][wave][lane][0]);
    const int m = m0 + wave * 16 + lr, c = c0 + lq * 4;
    if (m < M) {
      if (a.bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += a.bias[c + r];
      }
      if (a.add) {
        const u32x2 ad = ld8(a.add + (size_t)m * C + c);
        v[0] += bflo(ad.x); v[1] += bfhi(ad.x); v[2] += bflo(ad.y); v[3] += bfhi(ad.y);
      }
      u32x2 pk;
      pk.x = pack2bf(v[0], v[1]);
      pk.y = pack2bf(v[2], v[3]);
      st8(a.out + (size_t)m * C + c, pk);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Round 6: nn.Linear + BatchNorm1d (training statistics) + ReLU of the SimSiam head in ONE launch (sim_siam_head.py:78-111: the
// projector's Linear -> BN -> ReLU units and the predictor's first one) for the single-GPU step.  The head works on M = G x mpg <= 64
// rows (two views of 32 videos on the ResNet-50 config): conv_skinny + bn_stats_raw + bn_act were three dependent launches of 4-6 us
// each for a few KB.  A workgroup owns 16 output channels x ALL rows, so the batch statistics of its channels are local to it: the
// GEMM as in conv_skinny_kernel (four waves = four K quarters, fragments straight from global memory, four 16-row tiles per wave),
// then the statistics over the STORED (bf16) values in bn_stats_raw_kernel's summation order (eight row lanes in double, added in
// lane order - the same bits), scale / shift, running statistics group after group, and y = relu(q * scale + shift) exactly as
// bn_act_kernel computes it.  Outputs: raw (the backward needs it), act, bnp, sums, running statistics.
#define LINBN_MAXG 4
// NT = 16-row tiles per workgroup (4: <= 64 rows, the ResNet-50 config; 8 / 16: <= 128 / 256 rows, the ResNet-18 config's 2 x 128)
template <int NT>
__global__ __launch_bounds__(256) void linear_bn_act_kernel(LinBnArgs a) {
  __shared__ __attribute__((aligned(16))) float sAcc[4][NT][64][4];
  __shared__ float sRaw[NT * 16][16];
  __shared__ double sh[8][2][16];
  __shared__ float sCoef[LINBN_MAXG][2][16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int M = a.M, K = a.K, C = a.C;
  const int c0 = blockIdx.x * 16;
  const int kq = K >> 2;                                  // K % 128 == 0: whole 32-deep steps per wave
  const bf16_t* wrow = a.w + (size_t)(c0 + lr) * K + wave * kq + lq * 8;
  const bf16_t* xr[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) xr[i] = a.x + (size_t)min(16 * i + lr, M - 1) * K + wave * kq + lq * 8;      // rows past M: clamped, never stored
  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int steps = kq >> 5;
#pragma unroll 2
  for (int s = 0; s < steps; ++s) {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(wrow + s * 32);
    bf16x8 b[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) b[i] = *reinterpret_cast<const bf16x8*>(xr[i] + s * 32);
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b[i], acc[i], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) *reinterpret_cast<f32x4*>(&sAcc[wave][i][lane][0]) = acc[i];
  __syncthreads();
  // wave w finishes row tiles w, w + 4, ...: lane = (channel quad lq, row lr); the K quarters add up in wave order (as conv_skinny_kernel)
  const int cq = lq * 4;
#pragma unroll
  for (int ti = 0; ti < NT / 4; ++ti) {
    const int tile = wave + 4 * ti, m = 16 * tile + lr;
    f32x4 v = *reinterpret_cast<const f32x4*>(&sAcc[0][tile][lane][0]);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f32x4*>(&sAcc[w][tile][lane][0]);
    if (m < M) {
      if (a.bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += a.bias[c0 + cq + r];
      }
      u32x2 pk;
      pk.x = pack2bf(v[0], v[1]);
      pk.y = pack2bf(v[2], v[3]);
      st8(a.raw + (size_t)m * C + c0 + cq, pk);
      sRaw[m][cq] = bflo(pk.x); sRaw[m][cq + 1] = bfhi(pk.x); sRaw[m][cq + 2] = bflo(pk.y); sRaw[m][cq + 3] = bfhi(pk.y);
    }
  }
  __syncthreads();
  // statistics of the stored values, group after group (bn_stats_raw_kernel: eight row lanes, double, lane order)
  const int cl = t & 15, sl = (t >> 4) & 7;
  const bool stat_thread = t < 128;
  const int c = c0 + cl;
  float rm = 0.f, rv = 0.f;
  if (stat_thread && sl == 0) { rm = a.rm ? a.rm[c] : 0.f; rv = a.rv ? a.rv[c] : 0.f; }
  for (int gi = 0; gi < a.G; ++gi) {
    double a0 = 0.0, a1 = 0.0;
    if (stat_thread) {
      for (int b = sl; b < a.mpg; b += 8) {
        const double v = (double)sRaw[gi * a.mpg + b][cl];
        a0 += v;
        a1 += v * v;
      }
    }
    __syncthreads();
    if (stat_thread) { sh[sl][0][cl] = a0; sh[sl][1][cl] = a1; }
    __syncthreads();
    if (stat_thread && sl == 0) {
      double r0 = 0.0, r1 = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) { r0 += sh[k][0][cl]; r1 += sh[k][1][cl]; }
      a.sums[((size_t)gi * 2 + 0) * C + c] = r0;
      a.sums[((size_t)gi * 2 + 1) * C + c] = r1;
      const BnCoef k = bn_finalize_channel(r0, r1, a.count, a.eps, a.gamma[c], a.beta[c]);
      bn_store_params(a.bnp, gi, C, c, k);
      sCoef[gi][0][cl] = k.scale;
      sCoef[gi][1][cl] = k.shift;
      bn_running_update(rm, rv, a.momentum, k.mean, k.unbiased);
    }
  }
  if (stat_thread && sl == 0) {
    if (a.rm) a.rm[c] = rm;
    if (a.rv) a.rv[c] = rv;
  }
  __syncthreads();
#pragma unroll
  for (int ti = 0; ti < NT / 4; ++ti) {      // y = [relu](q * scale + shift) on the stored values, as bn_act_kernel
    const int m = 16 * (wave + 4 * ti) + lr;
    if (m >= M) continue;
    const int gi = m / a.mpg;
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      y[r] = sRaw[m][cq + r] * sCoef[gi][0][cq + r] + sCoef[gi][1][cq + r];
      if (a.relu) y[r] = fmaxf(y[r], 0.f);
    }
    u32x2 pk;
    pk.x = pack2bf(y[0], y[1]);
    pk.y = pack2bf(y[2], y[3]);
    st8(a.act + (size_t)m * C + c0 + cq, pk);
  }
}
int vfs_linear_bn_act_launch(const LinBnArgs& a, hipStream_t stream) {
  if (a.M < 1 || a.M > 256 || a.G < 1 || a.G > LINBN_MAXG || a.mpg * a.G != a.M || a.K % 128 || a.C % 16)
    return vfs_set_error(VFS_ERR_SHAPE, "linear_bn_act: M = G * mpg <= 256 rows, G <= 4, K % 128 == 0, C % 16 == 0");
  if (a.M <= 64) hipLaunchKernelGGL(linear_bn_act_kernel<4>, dim3(a.C / 16), dim3(256), 0, stream, a);
  else if (a.M <= 128) hipLaunchKernelGGL(linear_bn_act_kernel<8>, dim3(a.C / 16), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(linear_bn_act_kernel<16>, dim3(a.C / 16), dim3(256), 0, stream, a);
  return vfs_check_launch("linear_bn_act");
}

bool vfs_conv_skinny_eligible(const ConvArgs& a, int mode) {
  if (!vfs_option_igemm_skinny || (mode != GATHER_FWD && mode != GATHER_DGRAD)) return false;
  if (a.g.KH * a.g.KW != 1 || a.g.stride != 1 || a.g.pad != 0 || a.g.H != a.g.Ho || a.g.W != a.g.Wo || a.ksplit > 1) return false;
  // Linear layers only (1 x 1 "maps"): a backbone convolution on a tiny map keeps ONE kernel whatever its epilogue operands are -
  // the step's A/B switches (bit-packed mask on / off, ...) must not move a layer between kernels with different summation orders
  return a.g.H == 1 && a.g.W == 1 && a.g.M <= 128 && a.g.Ktot % 128 == 0 && a.Cout % 16 == 0 && !a.stats && !a.bn.partial && !a.add_mask &&
         a.g.C == a.g.Ktot;
}

int vfs_conv_skinny_dispatch(const ConvArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(conv_skinny_kernel, dim3((a.Cout / 16) * ((a.g.M + 31) / 32)), dim3(256), 0, stream, a);
  return vfs_check_launch("conv_skinny");
}
