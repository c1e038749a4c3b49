// Backward of the dilated convolutions for gfx950: input gradient and weight gradient of
//
//   y = conv(x, w, stride, padding = pad, dilation = dil)
//
// (torch autograd of mmcv ConvModule(padding=dilation, dilation=dilation), mmaction/models/backbones/resnet.py:51-58,172-179:
// the 3x3 convs of a ResNet built with dilations != 1 - the SiamFC probe's backbone with frozen_stages < 4,
// projects/siamfc-pytorch/siamfc/siamfc_tracker_base.py:131-144).
//
// Both are kernels of their own: the tuned dil == 1 kernels (conv_igemm.hip, conv_halo.hip, conv_wgrad.hip) are not touched, and
// their instantiations carry no dilation.  Shared with them: the LDS tile layout and MFMA K-step (vfs_conv.h), the epilogue of the
// implicit-GEMM kernels (vfs_igemm_epi.h: residual add, mask-gated add, bf16 rounding, whole NHWC rows) and the split-K reduction
// (vfs_wgrad_reduce_launch / vfs_wgrad_reduce_table).
//
// dgrad:  dx[n][h][w][ci] = sum_{r,s,co} dy[n][(h + pad - r dil) / stride][(w + pad - s dil) / stride][co] * wd[ci][r][s][co]
//   128 pixels x BC input channels per workgroup, K-steps of 64 output channels of one tap, register double buffer as the
//   PIPE 0 path of conv_igemm.hip.  stride 1: a pixel row's byte offset is base(row) + delta(tap, chunk) with delta uniform per
//   workgroup (delta carries the dilation: no per-load work that the undilated kernel does not do).  stride > 1: the offset is
//   derived per load and taps that fall between the samples of dy are sent out of range - the MFMAs multiply those zeros.
// wgrad:  dW[co][r][s][ci] = sum_{n,ho,wo} dy[n][ho][wo][co] * x[n][ho stride - pad + r dil][wo stride - pad + s dil][ci]
//   the generic kernel of conv_wgrad.hip (pixel-major LDS tiles, transposing LDS reads, 32x32x16 MFMA, split-K over linear pixel
//   ranges) with the tap offset of a lane's k-columns - constant over the whole pixel loop - scaled by the dilation.
#include "../../include/vfs_hip.h"
#include "vfs_igemm_epi.h"
#include "vfs_ops.h"

#define DIL_OOB 0xFFFFFFF0u   // >= any num_records: the buffer load returns zeros

template <int BC, bool S1>
__global__ __launch_bounds__(256, 2) void conv_dgrad_dil_kernel(ConvArgs a) {
  constexpr int BP = 128;
  constexpr int WC = BC / 2, TM = WC / 16, TN = 4, WLD = BC / 32;
  constexpr int OPER = 2 * (BC * 64 + BP * 64);
  constexpr int STAGE = igemm_stage_elems<BC, false>();
  constexpr int SMEM = OPER > STAGE ? OPER : STAGE;
  __shared__ __attribute__((aligned(16))) bf16_t smem[SMEM];
  __shared__ float sRed[2][BC][2];      // (forward statistics of the shared epilogue: unused by a dgrad)
  bf16_t (*sW)[BC * 64] = reinterpret_cast<bf16_t (*)[BC * 64]>(smem);
  bf16_t (*sX)[BP * 64] = reinterpret_cast<bf16_t (*)[BP * 64]>(smem + 2 * BC * 64);

  // g: N, H x W = the dy grid (gather source, C = forward Cout); Ho x Wo = the dx grid; a.Cout = forward Cin
  const ConvGeom g = a.g;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wc = wave >> 1, wp = wave & 1;
  const int ncb = a.Cout / BC;
  const int bx = blockIdx.x;
  const int pb = bx / ncb, cb = bx - pb * ncb;
  const int m0 = pb * BP, c0 = cb * BC;
  const int j = t & 7, row0 = t >> 3;
  const int cpt = g.C >> 6, ntap = g.KH * g.KW, nk = ntap * cpt;

  // ---- the four pixel rows this thread fetches
  unsigned xbase[4], xmask[4];      // stride 1: byte offset of (h + pad, w + pad) (mod 2^32), validity bit per tap
  int pnH[4], phb[4], pwb[4];       // stride > 1: n * H, h + pad, w + pad (rows past M: far negative)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + row0 + 32 * i;
    xbase[i] = 0u; xmask[i] = 0u;
    pnH[i] = 0; phb[i] = -(1 << 24); pwb[i] = -(1 << 24);
    if (m < g.M) {
      const int hw = g.Ho * g.Wo;
      const int n = m / hw;
      const int rem = m - n * hw;
      const int h = rem / g.Wo, w = rem - h * g.Wo;
      const int hb = h + g.pad, wb = w + g.pad;
      pnH[i] = n * g.H; phb[i] = hb; pwb[i] = wb;
      if (S1) {
        const long long base = ((long long)(n * g.H + hb) * g.W + wb) * g.C + j * 8;
        xbase[i] = (unsigned)(base * 2);
        unsigned mask = 0;
        for (int r = 0; r < g.KH; ++r)
          for (int s = 0; s < g.KW; ++s) {
            const int hi = hb - r * g.dil, wi = wb - s * g.dil;
            if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W) mask |= 1u << (r * g.KW + s);
          }
        xmask[i] = mask;
      }
    }
  }
  unsigned wbase[WLD];
#pragma unroll
  for (int i = 0; i < WLD; ++i) wbase[i] = (unsigned)(((size_t)(c0 + row0 + 32 * i) * g.Ktot + j * 8) * 2);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.src, 0, (unsigned)((size_t)g.N * g.H * g.W * g.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.wgt, 0, (unsigned)((size_t)a.Cout * g.Ktot * 2), 0x00020000);

  u32x4 xr[4], wr[WLD];
  int l_cc = 0, l_r = 0, l_s = 0;   // K-step counters of the NEXT load (uniform, no divisions)
  auto load_tiles = [&]() {         // called once per K-step, in order
    const int r = l_r, s = l_s, cc = l_cc << 6, ti = r * g.KW + s;
    if (++l_cc == cpt) {
      l_cc = 0;
      if (++l_s == g.KW) { l_s = 0; ++l_r; }
    }
    const int dh = r * g.dil, dw = s * g.dil;
    if (S1) {
      const int delta = (-(dh * g.W + dw) * g.C + cc) * 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned off = ((xmask[i] >> ti) & 1u) ? xbase[i] + (unsigned)delta : DIL_OOB;
        xr[i] = __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int th = phb[i] - dh, tw = pwb[i] - dw;
        const int hi = th / g.stride, wi = tw / g.stride;
        const bool ok = th >= 0 && tw >= 0 && hi * g.stride == th && wi * g.stride == tw && hi < g.H && wi < g.W;
        const unsigned off = ok ? (unsigned)((((size_t)(pnH[i] + hi) * g.W + wi) * g.C + cc + j * 8) * 2) : DIL_OOB;
        xr[i] = __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0);
      }
    }
    const unsigned wcol = (unsigned)((ti * g.C + cc) * 2);
#pragma unroll
    for (int i = 0; i < WLD; ++i) wr[i] = __builtin_amdgcn_raw_buffer_load_b128(wrs, wbase[i] + wcol, 0, 0);
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) st16(&sX[buf][lds_off(row0 + 32 * i, j)], xr[i]);
#pragma unroll
    for (int i = 0; i < WLD; ++i) st16(&sW[buf][lds_off(row0 + 32 * i, j)], wr[i]);
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};

  load_tiles();
  store_tiles(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load_tiles();
    __builtin_amdgcn_sched_barrier(0);          // keep the loads ahead of the MFMAs
    mma_kstep<TM, TN, false>(sW[cur], sX[cur], wc * WC, wp * 64, lane, acc);
    __builtin_amdgcn_sched_barrier(0);
    if (more) store_tiles(cur ^ 1);
    __syncthreads();
  }
  // The K loop ended with a barrier: the arena becomes the output stage of the shared epilogue (+ add, gated by add_mask).
  static_assert(SMEM >= igemm_stage_elems<BC, false>(), "stage does not fit the arena");
  igemm_epilogue<BC, GATHER_DGRAD, false>(a, m0, c0, pb, g.M, 0, 0, g.Ho, g.Wo, acc, smem, sRed);
}

template <int BC>
static int launch_dgrad_dil(const ConvArgs& a, hipStream_t stream) {
  const int npb = (a.g.M + 127) / 128, ncb = a.Cout / BC;
  if (a.g.stride == 1) hipLaunchKernelGGL((conv_dgrad_dil_kernel<BC, true>), dim3(npb * ncb), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((conv_dgrad_dil_kernel<BC, false>), dim3(npb * ncb), dim3(256), 0, stream, a);
  return vfs_check_launch("conv_dgrad_dilated");
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
#define DWG_RS 72   // LDS row pitch of a [pixel][64 channels] tile (as conv_wgrad.hip)

template <int BCW>
__global__ __launch_bounds__(256) void conv_wgrad_dil_kernel(WgradArgs a) {
  constexpr int BKC = 128;        // k-columns per workgroup (two forward K-steps)
  constexpr int TILE = 64 * DWG_RS, DT = BCW / 64;
  __shared__ __attribute__((aligned(16))) bf16_t sA[2][2 * TILE];
  __shared__ __attribute__((aligned(16))) bf16_t sD[2][DT * TILE];

  const ConvGeom g = a.g;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nkb = (g.Ktot + BKC - 1) / BKC;
  const int ncb = a.Cout / BCW;
  int b = blockIdx.x;
  if (a.xcd_swizzle) {            // XCD-aware block order (conv_wgrad.hip): the tiles of one pixel split share an L2
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = b & 7;
    b = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int kb = b % nkb; b /= nkb;
  const int cb = b % ncb; b /= ncb;
  const int split = b;
  const int nk = g.Ktot >> 6;

  // loader roles: A tile = 16 chunks x 16 pixel groups of the gathered input, D tile = dY
  const int a_cj = t & 15, a_pg = t >> 4;
  const int a_kt = kb * 2 + (a_cj >> 3), a_j = a_cj & 7;
  const bool a_ok = a_kt < nk;
  const KStep a_ks = kstep_decode<GATHER_FWD>(g, a_ok ? a_kt : 0);
  const int a_dh = a_ks.r * g.dil - g.pad, a_dw = a_ks.s * g.dil - g.pad;      // the lane's tap: constant over the pixel loop
  constexpr int DCH = BCW / 8;
  const int d_cj = t % DCH, d_pg = (t / DCH) & 15;
  const bool d_active = t < DCH * 16;

  const int pix_begin = split * a.pix_per_split;
  const int iters = a.pix_per_split >> 6;

  // the 4 pixels a thread gathers advance by 64 per iteration; (n, ho, wo) kept incrementally
  const int hw = g.Ho * g.Wo;
  const int dn = 64 / hw, dr = 64 - dn * hw, dh = dr / g.Wo, dw = dr - dh * g.Wo;
  int pn[4], ph[4], pw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = pix_begin + a_pg * 4 + i;
    pn[i] = m / hw;
    const int rem = m - pn[i] * hw;
    ph[i] = rem / g.Wo;
    pw[i] = rem - ph[i] * g.Wo;
  }
  u32x4 av[4], dv[4];
  auto load_tiles = [&](int it) {   // called with it = 0, 1, 2, ... in order
    const int p0 = pix_begin + it * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      av[i] = zero16();
      if (a_ok && pn[i] < g.N) {      // pixels past M (n >= N) contribute zero
        const int hi = ph[i] * g.stride + a_dh, wi = pw[i] * g.stride + a_dw;
        if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W)
          av[i] = ld16(a.x + ((size_t)(pn[i] * g.H + hi) * g.W + wi) * g.C + a_ks.c0 + a_j * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pw[i] += dw;
      if (pw[i] >= g.Wo) { pw[i] -= g.Wo; ph[i] += 1; }
      ph[i] += dh;
      if (ph[i] >= g.Ho) { ph[i] -= g.Ho; pn[i] += 1; }
      pn[i] += dn;
    }
    if (d_active) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = p0 + d_pg * 4 + i;
        dv[i] = (m < g.M) ? ld16(a.dy + (size_t)m * a.Cout + cb * BCW + d_cj * 8) : zero16();
      }
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) st16(&sA[buf][(a_cj >> 3) * TILE + (a_pg * 4 + i) * DWG_RS + a_j * 8], av[i]);
    if (d_active) {
#pragma unroll
      for (int i = 0; i < 4; ++i) st16(&sD[buf][(d_cj >> 3) * TILE + (d_pg * 4 + i) * DWG_RS + (d_cj & 7) * 8], dv[i]);
    }
  };
  // fragment geometry of conv_wgrad.hip: a k-step is 16 pixels; MFMA row = lane % 32 = channel, lane / 32 = k half
  const int l16 = lane & 15, h2 = lane >> 5;
  const int pl = 8 * h2 + (l16 >> 2), chq = ((lane >> 4) & 1) * 16 + (l16 & 3) * 4;
  const int a_base = wm * TILE + pl * DWG_RS + chq;
  const int d_base = (BCW == 128 ? wn * TILE : wn * 32) + pl * DWG_RS + chq;
  constexpr int QM = 2, QN = BCW / 64;

  vfs_f32x16 acc[QM][QN];
#pragma unroll
  for (int tm = 0; tm < QM; ++tm)
#pragma unroll
    for (int tn = 0; tn < QN; ++tn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;

  load_tiles(0);
  store_tiles(0);
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const int cur = it & 1;
    const bool more = it + 1 < iters;
    if (more) load_tiles(it + 1);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      bf16x8 af[QM], bfr[QN];
#pragma unroll
      for (int tm = 0; tm < QM; ++tm)
        af[tm] = tile_tr_frag(sA[cur] + a_base, (16 * st) * DWG_RS + tm * 32, (16 * st + 4) * DWG_RS + tm * 32);
#pragma unroll
      for (int tn = 0; tn < QN; ++tn)
        bfr[tn] = tile_tr_frag(sD[cur] + d_base, (16 * st) * DWG_RS + tn * 32, (16 * st + 4) * DWG_RS + tn * 32);
#pragma unroll
      for (int tm = 0; tm < QM; ++tm)
#pragma unroll
        for (int tn = 0; tn < QN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm], bfr[tn], acc[tm][tn], 0, 0, 0);
    }
    if (more) store_tiles(cur ^ 1);
    __syncthreads();
  }

  // D[k-column][cout] (32 x 32 tiles): register 4 q + r of lane l = k-column 8 q + 4 (l / 32) + r, cout l % 32 -> 16-byte stores
#pragma unroll
  for (int tn = 0; tn < QN; ++tn) {
    const int cout = cb * BCW + wn * (BCW / 2) + tn * 32 + (lane & 31);
#pragma unroll
    for (int tm = 0; tm < QM; ++tm)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int kc = kb * BKC + wm * 64 + tm * 32 + 8 * q + 4 * h2;
        if (kc < g.Ktot)
          *reinterpret_cast<f32x4*>(a.partial + ((size_t)split * a.Cout + cout) * g.Ktot + kc) =
              (f32x4){acc[tm][tn][4 * q], acc[tm][tn][4 * q + 1], acc[tm][tn][4 * q + 2], acc[tm][tn][4 * q + 3]};
      }
  }
}

template <int BCW>
static int launch_wgrad_dil(const WgradArgs& a0, hipStream_t stream) {
  WgradArgs a = a0;
  const int nkb = (a.g.Ktot + 127) / 128, ncb = a.Cout / BCW;
  a.xcd_swizzle = vfs_option_wgrad_xcd && nkb * ncb > 1 && nkb * ncb * a.nsplit >= 16;
  hipLaunchKernelGGL((conv_wgrad_dil_kernel<BCW>), dim3(nkb * ncb * a.nsplit), dim3(256), 0, stream, a);
  return vfs_check_launch("conv_wgrad_dilated");
}

// ---------------------------------------------------------------------------------------------------------------- C ABI
static int dil_fail(int code, const char* who, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  return vfs_set_error(code, buf);
}
// the checks both entry points share (all geometry arguments are those of the FORWARD convolution)
static int dil_check(const char* who, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                     int dilation) {
  if (dilation < 1) return dil_fail(VFS_ERR_ARG, who, "dilation >= 1");
  if (N < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0) return dil_fail(VFS_ERR_ARG, who, "N, H, W, KH, KW, stride >= 1 and pad >= 0");
  if (Ho != (H + 2 * pad - dilation * (KH - 1) - 1) / stride + 1 || Wo != (W + 2 * pad - dilation * (KW - 1) - 1) / stride + 1 || Ho < 1 || Wo < 1)
    return dil_fail(VFS_ERR_SHAPE, who, "output size does not match (H + 2 pad - dilation (K - 1) - 1) / stride + 1");
  if (Cin % 64 != 0 || Cout % 64 != 0 || Cin < 64 || Cout < 64) return dil_fail(VFS_ERR_SHAPE, who, "Cin % 64 == 0 and Cout % 64 == 0");
  if (KH * KW > 32) return dil_fail(VFS_ERR_SHAPE, who, "more than 32 taps");
  const size_t lim = 0xFFFFFFF0ull;
  if ((size_t)N * H * W * Cin * 2 >= lim || (size_t)N * Ho * Wo * Cout * 2 >= lim || (size_t)Cout * KH * KW * Cin * 2 >= lim)
    return dil_fail(VFS_ERR_SHAPE, who, "tensor >= 4 GiB (split the batch)");
  return VFS_OK;
}

extern "C" int vfs_conv_dgrad_dilated(const vfs_bf16* dy, const vfs_bf16* wd, vfs_bf16* dx, const vfs_bf16* add, const uint8_t* add_mask,
                                      int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                                      int dilation, vfs_stream_t stream) {
  static const char* who = "conv_dgrad_dilated";
  if (!dy || !wd || !dx) return dil_fail(VFS_ERR_ARG, who, "null dy, wd or dx");
  if (add_mask && !add) return dil_fail(VFS_ERR_ARG, who, "add_mask needs an add operand");
  if (int rc = dil_check(who, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, dilation)) return rc;
  ConvArgs a{};
  ConvGeom& g = a.g;      // gather source = dy [N,Ho,Wo,Cout]; destination grid = dx [N,H,W,Cin]
  g.N = N; g.H = Ho; g.W = Wo; g.C = Cout; g.Ho = H; g.Wo = W;
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad; g.Ktot = KH * KW * Cout; g.M = N * H * W; g.dil = dilation;
  a.src = dy; a.wgt = wd; a.out = dx; a.add = add; a.Cout = Cin;
  if (add_mask) { a.add_mask = add_mask; a.add_rows = (long long)N * H * W; }
  // 128-channel tiles unless that leaves the chip under-filled (the rule of conv_igemm.hip)
  const long long tiles128 = (long long)((g.M + 127) / 128) * ((Cin + 127) / 128);
  const bool wide = Cin % 128 == 0 && vfs_option_igemm_bc != 64 && tiles128 >= vfs_option_igemm_narrow_below;
  return wide ? launch_dgrad_dil<128>(a, (hipStream_t)stream) : launch_dgrad_dil<64>(a, (hipStream_t)stream);
}

extern "C" int vfs_conv_wgrad_dilated(const vfs_bf16* dy, const vfs_bf16* x, float* partial, float* grad, int N, int H, int W, int Cin,
                                      int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int dilation, int nsplit,
                                      int pix_per_split, vfs_stream_t stream) {
  static const char* who = "conv_wgrad_dilated";
  if (!dy || !x || !partial) return dil_fail(VFS_ERR_ARG, who, "null dy, x or partial");
  if (int rc = dil_check(who, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, dilation)) return rc;
  if (nsplit < 1 || pix_per_split < 64 || pix_per_split % 64 != 0) return dil_fail(VFS_ERR_SHAPE, who, "nsplit >= 1 and pix_per_split a positive multiple of 64");
  if ((long long)pix_per_split * nsplit < (long long)N * Ho * Wo) return dil_fail(VFS_ERR_SHAPE, who, "splits do not cover N * Ho * Wo");
  WgradArgs a{};
  ConvGeom& g = a.g;      // geometry of the forward conv (gather source = forward input)
  g.N = N; g.H = H; g.W = W; g.C = Cin; g.Ho = Ho; g.Wo = Wo;
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad; g.Ktot = KH * KW * Cin; g.M = N * Ho * Wo; g.dil = dilation;
  a.dy = dy; a.x = x; a.partial = partial; a.Cout = Cout; a.pix_per_split = pix_per_split; a.nsplit = nsplit;
  const int rc = Cout % 128 == 0 ? launch_wgrad_dil<128>(a, (hipStream_t)stream) : launch_wgrad_dil<64>(a, (hipStream_t)stream);
  if (rc || !grad) return rc;      // grad == NULL: the caller reduces the partials (vfs_wgrad_reduce_table)
  return vfs_wgrad_reduce_launch(partial, grad, nsplit, Cout, g.Ktot, Cin, KH, KW, 0, (hipStream_t)stream);
}
