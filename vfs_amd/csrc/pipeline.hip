// Training input pipeline on the GPU: RandomResizedCrop -> Resize(224, bilinear) -> Flip
// -> Normalize -> FormatShape('NCTHW') of the reference's train_pipeline (configs/r*_*.py:48-91;
// pipelines/augmentations.py:171-334 crop, :487-596 resize, :600-707 flip, :711-794 normalize;
// pipelines/formating.py:222-309) fused into ONE pass over the decoded uint8 frames: every output pixel
// reads its (at most) four source pixels inside the frame's crop box and writes the normalised value
// straight into the fp32 [B][V][3][T][H][W] tensor train_step takes and / or the bf16 NHWC4 frame buffer
// the stem kernel reads.  The random decisions (crop boxes, flips) are drawn on the host with the
// reference's rules and arrive as small per-frame arrays.
//
// The image arithmetic of the reference lives in mmcv -> OpenCV (absent here): restated from the
// published implementation - cv2.resize INTER_LINEAR on 8-bit data is FIXED POINT (11-bit coefficients,
// two passes, the vertical pass on (value >> 4) with a 2-bit rounding), cv2.flip, and mmcv.imnormalize_
// = cv2.subtract / cv2.multiply of a float32 image with float64 scalars (computed in double, stored as
// float32 after each step).  Byte work, HBM-bound; parity with oracle/pipeline_oracle.py is bit-exact.
#include "vfs_common.h"
#include "vfs_ops.h"

// cv2 resize (resize.cpp, INTER_LINEAR, 8-bit): source index and 11-bit weights of destination index d for an
// axis of n samples scaled to m.  Columns (XAXIS): an index outside [0, n-1) is clamped AND its fraction
// zeroed; rows: the two row indices are clamped when they are fetched, the weights stay.
template <bool XAXIS>
__device__ __forceinline__ void cv_linear_coef(int d, int n, int m, int& s0, int& s1, int& w0, int& w1) {
  const double scale = 1.0 / ((double)m / (double)n);     // cv::resize: scale = 1 / inv_scale
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (XAXIS) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
  }
  s0 = min(max(s, 0), n - 1);
  s1 = min(max(s + 1, 0), n - 1);
  w0 = (int)rintf((1.f - f) * 2048.f);     // saturate_cast<short>: round half to even
  w1 = (int)rintf(f * 2048.f);
}

// Where the pixels of frame f lie.  The uniform entry points take one dense [F][Hs][Ws][3] tensor; the ragged ones
// (vfs_crop_resize_flip_norm_ragged) a byte buffer and a descriptor row per SAMPLE, int32 {offset low, offset high, Hs, Ws}:
// the reference crops and resizes sample by sample, each at its own img_shape (augmentations.py:171-334,487-596), and
// DecordDecode returns every Kinetics video at its own size.  A row that would let a frame reach outside
// [src, src + src_bytes) makes the whole sample invalid (img == nullptr): it reads nothing and its outputs are zeros.
struct FrameSrc {
  const uint8_t* img;    // [Hs][Ws][3]
  int Hs, Ws;
};

template <bool RAGGED>
__device__ __forceinline__ FrameSrc frame_src(const PipelineArgs& a, int f) {
  if (!RAGGED) return FrameSrc{a.src + (size_t)f * a.Hs * a.Ws * 3, a.Hs, a.Ws};
  const int per = a.V * a.T;
  const int* d = a.srcdesc + 4 * (f / per);
  const long long off = (long long)(((unsigned long long)(uint32_t)d[1] << 32) | (unsigned long long)(uint32_t)d[0]);
  const int Hs = d[2], Ws = d[3];
  if (Hs <= 0 || Ws <= 0 || off < 0 || off > a.src_bytes) return FrameSrc{nullptr, 0, 0};
  const unsigned long long frame = (unsigned long long)Hs * (unsigned long long)Ws * 3ull;     // < 3 * 2^62
  unsigned long long need;
  if (__builtin_umulll_overflow(frame, (unsigned long long)per, &need) || need > (unsigned long long)(a.src_bytes - off))
    return FrameSrc{nullptr, 0, 0};
  return FrameSrc{a.src + off + (size_t)(f % per) * frame, Hs, Ws};
}

// crop + resize + flip of one output pixel (cv2.resize's two fixed-point passes, per channel, before the uint8 saturation)
__device__ __forceinline__ void resize_pixel(const PipelineArgs& a, const FrameSrc& s, int f, int x, int y, int u[3]) {
  // boxes come from the host: clamp them to the frame so a bad box can never read outside it
  const int left = min(max(a.boxes[4 * f], 0), s.Ws - 1), top = min(max(a.boxes[4 * f + 1], 0), s.Hs - 1);
  const int right = min(max(a.boxes[4 * f + 2], left + 1), s.Ws), bottom = min(max(a.boxes[4 * f + 3], top + 1), s.Hs);
  const int cw = right - left, ch = bottom - top;
  const int xr = a.flips[f] ? a.Wo - 1 - x : x;  // cv2.flip(img, 1) AFTER the resize
  int sx, sx1, ax0, ax1, sy, sy1, by0, by1;
  cv_linear_coef<true>(xr, cw, a.Wo, sx, sx1, ax0, ax1);
  cv_linear_coef<false>(y, ch, a.Ho, sy, sy1, by0, by1);
  const uint8_t* p00 = s.img + ((size_t)(top + sy) * s.Ws + left + sx) * 3;
  const uint8_t* p01 = s.img + ((size_t)(top + sy) * s.Ws + left + sx1) * 3;
  const uint8_t* p10 = s.img + ((size_t)(top + sy1) * s.Ws + left + sx) * 3;
  const uint8_t* p11 = s.img + ((size_t)(top + sy1) * s.Ws + left + sx1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = p00[c] * ax0 + p01[c] * ax1;          // horizontal pass, 8 + 11 bits
    const int h1 = p10[c] * ax0 + p11[c] * ax1;
    u[c] = (((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2;   // vertical pass
  }
}

// mmcv.imnormalize_ of one channel value
__device__ __forceinline__ float normalized(const PipelineArgs& a, int c, int u) {
  const float d = (float)((double)u - a.mean[c]);       // cv2.subtract(float32 image, float64 scalar)
  return (float)((double)d * a.stdinv[c]);              // cv2.multiply(..., 1/std)
}

// FormatShape: one pixel of frame f (pipeline order (b, v, t)) into both output layouts
__device__ __forceinline__ void store_pixel(const PipelineArgs& a, int f, int x, int y, const float o[3]) {
  const int t = f % a.T, v = (f / a.T) % a.V, b = f / (a.T * a.V);
  if (a.imgs) {
    const size_t plane = (size_t)a.T * a.Ho * a.Wo;
    float* q = a.imgs + (((size_t)b * a.V + v) * 3) * plane + ((size_t)t * a.Ho + y) * a.Wo + x;
    q[0] = o[0]; q[plane] = o[1]; q[2 * plane] = o[2];
  }
  if (a.x4) {   // frame order of the backbone batch: (view, b, t), as vfs_imgs_to_nhwc4
    const size_t fr = ((size_t)v * a.B + b) * a.T + t;
    u32x2 pk;
    pk.x = pack2bf(o[0], o[1]);
    pk.y = pack2bf(o[2], 0.f);
    st8(a.x4 + ((fr * a.Ho + y) * a.Wp + x) * 4, pk);
    if (a.Wp > a.Wo && x == a.Wo - 1) st8(a.x4 + ((fr * a.Ho + y) * a.Wp + a.Wo) * 4, (u32x2){0u, 0u});
  }
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void crop_resize_flip_norm_kernel(PipelineArgs a) {
  const long long total = (long long)a.B * a.V * a.T * a.Ho * a.Wo;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % a.Wo);
    long long r = i / a.Wo;
    const int y = (int)(r % a.Ho); r /= a.Ho;
    const int f = (int)r;                          // frame index in pipeline order: (b, v, t)
    const FrameSrc s = frame_src<RAGGED>(a, f);
    float o[3] = {0.f, 0.f, 0.f};                  // what a sample with a bad descriptor row gets
    if (!RAGGED || s.img) {
      int u[3];
      resize_pixel(a, s, f, x, y, u);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = normalized(a, c, u[c]);
    }
    store_pixel(a, f, x, y, o);
  }
}

int vfs_crop_resize_flip_norm_launch(const PipelineArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.V <= 0 || a.T <= 0 || a.Ho <= 0 || a.Wo <= 0) return vfs_set_error(VFS_ERR_SHAPE, "pipeline: empty batch");
  const long long total = (long long)a.B * a.V * a.T * a.Ho * a.Wo;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (a.ragged) hipLaunchKernelGGL(crop_resize_flip_norm_kernel<true>, dim3((int)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(crop_resize_flip_norm_kernel<false>, dim3((int)blocks), dim3(256), 0, s, a);
  return vfs_check_launch("crop_resize_flip_norm");
}

// ---- photometric steps: ColorJitter / RandomGrayScale / RandomGaussianBlur (augmentations.py:1224-1320) between Flip
// and Normalize, for the object-level configs (r18_sgd_cos_100e_r2_1xNx8_k400.py, r50_sgd_cos_100e_r5_1xNx2_k400.py).
// They act on the uint8 224x224 frame after the resize, through PIL (torchvision 0.7 ColorJitter: ImageEnhance blend,
// HSV round trip), mmcv.rgb2gray (cv2.cvtColor) and PIL's GaussianBlur (extended box blur, three passes per axis).
// Two launches: A = crop + resize + flip + the jitter ops that precede contrast in the frame's shuffled order, uint8
// RGBX into the workspace, plus the frame's sum of PIL luma when contrast follows (contrast blends towards the mean of
// the frame AS IT STANDS then); B = one 64x16 tile + 3-pixel halo in LDS: contrast, the remaining jitter ops, grey,
// the six box-blur passes, normalise, store.  Integer sums: bit-identical whatever the order of the atomics.
// A launch whose rows may carry a box radius of 1..3 (vfs_crop_resize_flip_photo_norm_blur) runs launch B as
// photo_finish_wide_kernel: the same tile with a halo of 3 * (r + 1) pixels.

#define PHOTO_TW 64
#define PHOTO_TH 16
#define PHOTO_HALO 3
#define PHOTO_LW (PHOTO_TW + 2 * PHOTO_HALO)
#define PHOTO_LH (PHOTO_TH + 2 * PHOTO_HALO)
// photo_finish_wide_kernel<R>: every pass needs its input valid r + 1 pixels further out, six passes, three per axis: a halo of
// 3 * (R + 1) for the launch-wide bound R; a frame of radius r < R fills and sweeps only its own 3 * (r + 1) of it.
// LDS per block = 2 buffers * 4 bytes * (64 + 2 halo) * (16 + 2 halo):
//   R = 1: halo  6, 76 x 28 -> 17,024 bytes     R = 2: halo  9, 82 x 34 -> 22,304 bytes     R = 3: halo 12, 88 x 40 -> 28,160 bytes
// (the radius-0 kernel: 70 x 22 -> 12,320 bytes); the 160 KiB of a CU hold 9 / 7 / 5 such blocks of 4 waves: LDS does not limit
// R = 1 (8 blocks fill the CU's 32 wave slots) and leaves 28 / 20 of the 32 waves for R = 2 / 3.
#define PHOTO_MAX_RADIUS 3
#define PHOTO_WIDE_HALO(R) (3 * ((R) + 1))
#define PHOTO_WIDE_LW(R) (PHOTO_TW + 2 * PHOTO_WIDE_HALO(R))
#define PHOTO_WIDE_LH(R) (PHOTO_TH + 2 * PHOTO_WIDE_HALO(R))

enum { PH_BRIGHT = 1, PH_CONTRAST = 2, PH_SAT = 3, PH_HUE = 4 };

struct PhotoFrame {
  int ops[4];          // jitter ops in application order (0 = none)
  int split;           // index of contrast in ops (4 if absent): ops[0, split) run in launch A, ops(split, 4) in launch B
  float fac[4];        // blend factors by op code - 1 (brightness, contrast, saturation)
  int hue, gray;
  uint32_t ww, fw;     // box-blur weights, ww == 0: no blur
  int rad;             // integer box radius, at most the launch's bound
};

// max_radius: the largest box radius the launch runs (0 for the entry points that know none: they ignore bits 8.. of word [4])
__device__ __forceinline__ PhotoFrame load_photo(const int* p, int max_radius) {
  PhotoFrame r;
  const uint32_t code = (uint32_t)p[0];
  r.split = 4;
  for (int k = 0; k < 4; ++k) {
    const int op = (int)((code >> (4 * k)) & 15u);
    r.ops[k] = op <= PH_HUE ? op : 0;        // unknown codes are no-ops
    if (r.ops[k] == PH_CONTRAST && r.split == 4) r.split = k;
  }
  r.fac[0] = __builtin_bit_cast(float, p[1]); r.fac[1] = __builtin_bit_cast(float, p[2]); r.fac[2] = __builtin_bit_cast(float, p[3]); r.fac[3] = 0.f;
  r.hue = p[4] & 255;
  r.gray = p[5] != 0;
  // host values are clamped so that no row reaches outside the tile (rad <= max_radius) and the window sum
  // 255 * ((2 rad + 1) ww + 2 fw) + 2^23 stays below 2^32 ((2 rad + 1) ww + 2 fw <= 2^24)
  r.rad = min((int)(((uint32_t)p[4] >> 8) & 255u), max_radius);
  const uint32_t taps = 2u * (uint32_t)r.rad + 1u;
  r.ww = min((uint32_t)p[6], (1u << 24) / taps);
  r.fw = min((uint32_t)p[7], ((1u << 24) - taps * r.ww) / 2);
  return r;
}

__device__ __forceinline__ int pil_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// ImagingBlend(degenerate, image, alpha): temp = d + alpha*(x - d) in fp32 with the multiply and the add rounded apart
__device__ __forceinline__ int pil_blend(int x, int d, float alpha) {
#pragma clang fp contract(off)
  const float t = (float)d + alpha * (float)(x - d);
  if (!(t > 0.f)) return 0;
  if (t >= 255.f) return 255;
  return (int)t;
}

// Pillow Convert.c rgb2hsv_row + hue shift + hsv2rgb (the HSV round trip of torchvision 0.7 adjust_hue)
__device__ __forceinline__ void pil_hue(int& r, int& g, int& b, int shift) {
#pragma clang fp contract(off)
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
  }
  const int hh = (uh + shift) & 255, v = maxc;
  if (us == 0) { r = g = b = v; return; }
  const double hf = (double)(float)hh * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const float f = (float)(hf - (double)(float)i);
  const float fs = (float)((double)(float)us / 255.0);
  const float fsf = fs * f;                                   // fp32 product in Pillow's q
  const int p = min(max((int)round((double)v * (1.0 - (double)fs)), 0), 255);
  const int q = min(max((int)round((double)v * (1.0 - (double)fsf)), 0), 255);
  const int t = min(max((int)round((double)v * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

__device__ __forceinline__ void jitter_op(int op, const PhotoFrame& ph, int cmean, int& r, int& g, int& b) {
  if (op == PH_BRIGHT) {
    r = pil_blend(r, 0, ph.fac[0]); g = pil_blend(g, 0, ph.fac[0]); b = pil_blend(b, 0, ph.fac[0]);
  } else if (op == PH_CONTRAST) {
    r = pil_blend(r, cmean, ph.fac[1]); g = pil_blend(g, cmean, ph.fac[1]); b = pil_blend(b, cmean, ph.fac[1]);
  } else if (op == PH_SAT) {
    const int l = pil_luma(r, g, b);
    r = pil_blend(r, l, ph.fac[2]); g = pil_blend(g, l, ph.fac[2]); b = pil_blend(b, l, ph.fac[2]);
  } else if (op == PH_HUE) {
    pil_hue(r, g, b, ph.hue);
  }
}

__device__ __forceinline__ uint32_t pack_rgb(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }

// mmcv.imnormalize_ + FormatShape of one uint8 pixel
__device__ __forceinline__ void store_normalized(const PipelineArgs& a, int f, int x, int y, uint32_t px) {
  float o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = normalized(a, c, (int)((px >> (8 * c)) & 255u));
  store_pixel(a, f, x, y, o);
}

// launch A: grid (pixel blocks, frames)
template <bool RAGGED>
__global__ __launch_bounds__(256) void photo_resize_kernel(PhotoArgs pa) {
  const PipelineArgs& a = pa.p;
  const int f = blockIdx.y;
  const FrameSrc fs = frame_src<RAGGED>(a, f);
  if (RAGGED && !fs.img) return;     // block-uniform: a bad descriptor row, launch B writes the frame's zeros
  const PhotoFrame ph = load_photo(pa.photo + 8 * f, 0);      // the blur words are launch B's
  const long long hw = (long long)a.Ho * a.Wo;
  uint32_t* out = pa.pix + (size_t)f * hw;
  uint32_t lsum = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % a.Wo), y = (int)(i / a.Wo);
    int u[3];
    resize_pixel(a, fs, f, x, y, u);
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = min(u[c], 255);     // cv2.resize's saturate_cast<uchar>
    for (int k = 0; k < ph.split; ++k) jitter_op(ph.ops[k], ph, 0, u[0], u[1], u[2]);
    out[i] = pack_rgb(u[0], u[1], u[2]);
    lsum += (uint32_t)pil_luma(u[0], u[1], u[2]);
  }
  if (ph.split < 4) {      // block-uniform: contrast follows, its mean needs the frame's luma sum
    __shared__ uint32_t red[256];
    red[threadIdx.x] = lsum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(pa.sums + f, (unsigned long long)red[0]);
  }
}

__device__ __forceinline__ uint32_t box_pass(uint32_t c, uint32_t lo, uint32_t hi, uint32_t ww, uint32_t fw) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t x = (c >> (8 * k)) & 255u, l = (lo >> (8 * k)) & 255u, h = (hi >> (8 * k)) & 255u;
    o |= ((x * ww + (l + h) * fw + (1u << 23)) >> 24) << (8 * k);
  }
  return o;
}

// the per-pixel tail of launch B: contrast and the jitter ops after it, then grey
__device__ __forceinline__ uint32_t photo_post(uint32_t px, const PhotoFrame& ph, int cmean) {
  int r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
  for (int k = ph.split; k < 4; ++k) jitter_op(ph.ops[k], ph, cmean, r, g, b);
  if (ph.gray) r = g = b = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;     // cv2 RGB2GRAY, 8-bit fixed point
  return pack_rgb(r, g, b);
}

// launch B: grid (column tiles, row tiles, frames)
template <bool RAGGED>
__global__ __launch_bounds__(256) void photo_finish_kernel(PhotoArgs pa) {
  const PipelineArgs& a = pa.p;
  const int f = blockIdx.z, x0 = blockIdx.x * PHOTO_TW, y0 = blockIdx.y * PHOTO_TH;
  if (RAGGED && !frame_src<RAGGED>(a, f).img) {     // block-uniform: a bad descriptor row, launch A wrote nothing for the frame
    const float zero[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < PHOTO_TW * PHOTO_TH; i += 256) {
      const int x = x0 + i % PHOTO_TW, y = y0 + i / PHOTO_TW;
      if (x < a.Wo && y < a.Ho) store_pixel(a, f, x, y, zero);
    }
    return;
  }
  const PhotoFrame ph = load_photo(pa.photo + 8 * f, 0);
  const uint32_t* in = pa.pix + (size_t)f * a.Ho * a.Wo;
  int cmean = 0;
  if (ph.split < 4) cmean = (int)((double)pa.sums[f] / ((double)a.Ho * (double)a.Wo) + 0.5);     // ImageStat mean, int(m + 0.5)
  if (ph.ww == 0) {     // no blur: pixel by pixel
    for (int i = threadIdx.x; i < PHOTO_TW * PHOTO_TH; i += 256) {
      const int x = x0 + i % PHOTO_TW, y = y0 + i / PHOTO_TW;
      if (x < a.Wo && y < a.Ho) store_normalized(a, f, x, y, photo_post(in[(size_t)y * a.Wo + x], ph, cmean));
    }
    return;
  }
  // blur: PIL's three horizontal then three vertical box passes, uint8 after each, edge pixels of the FRAME replicated
  __shared__ uint32_t buf[2][PHOTO_LH * PHOTO_LW];
  const int gx0 = x0 - PHOTO_HALO, gy0 = y0 - PHOTO_HALO;
  for (int i = threadIdx.x; i < PHOTO_LH * PHOTO_LW; i += 256) {
    const int gx = gx0 + i % PHOTO_LW, gy = gy0 + i / PHOTO_LW;
    if (gx >= 0 && gx < a.Wo && gy >= 0 && gy < a.Ho) buf[0][i] = photo_post(in[(size_t)gy * a.Wo + gx], ph, cmean);
  }
  __syncthreads();
  int cur = 0;
  for (int k = 1; k <= 3; ++k) {       // pass k is valid on local columns [k, LW - k): its neighbours were valid in pass k-1
    const int w = PHOTO_LW - 2 * k;
    for (int i = threadIdx.x; i < PHOTO_LH * w; i += 256) {
      const int lx = k + i % w, ly = i / w;
      const int gx = gx0 + lx, gy = gy0 + ly;
      if (gx < 0 || gx >= a.Wo || gy < 0 || gy >= a.Ho) continue;
      const int xl = max(gx - 1, 0) - gx0, xh = min(gx + 1, a.Wo - 1) - gx0;
      const uint32_t* s = buf[cur] + ly * PHOTO_LW;
      buf[cur ^ 1][ly * PHOTO_LW + lx] = box_pass(s[lx], s[xl], s[xh], ph.ww, ph.fw);
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int k = 1; k <= 3; ++k) {       // rows [k, LH - k) of the columns [3, LW - 3) the tile keeps
    const int h = PHOTO_LH - 2 * k;
    for (int i = threadIdx.x; i < h * PHOTO_TW; i += 256) {
      const int lx = PHOTO_HALO + i % PHOTO_TW, ly = k + i / PHOTO_TW;
      const int gx = gx0 + lx, gy = gy0 + ly;
      if (gx >= a.Wo || gy < 0 || gy >= a.Ho) continue;
      const int yl = max(gy - 1, 0) - gy0, yh = min(gy + 1, a.Ho - 1) - gy0;
      const uint32_t* s = buf[cur];
      buf[cur ^ 1][ly * PHOTO_LW + lx] = box_pass(s[ly * PHOTO_LW + lx], s[yl * PHOTO_LW + lx], s[yh * PHOTO_LW + lx], ph.ww, ph.fw);
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int i = threadIdx.x; i < PHOTO_TW * PHOTO_TH; i += 256) {
    const int x = x0 + i % PHOTO_TW, y = y0 + i / PHOTO_TW;
    if (x < a.Wo && y < a.Ho) store_normalized(a, f, x, y, buf[cur][(i / PHOTO_TW + PHOTO_HALO) * PHOTO_LW + i % PHOTO_TW + PHOTO_HALO]);
  }
}

// one pass of PIL's extended box blur at integer radius rad on one pixel: s = the line (row: stride 1, column: stride LW) in LDS,
// g = the pixel's frame coordinate on that axis, n = the frame's extent, g0 = the frame coordinate of s[0].  Neighbours are taken
// at clamped frame coordinates (ImagingLineBoxBlur8's three edge regimes in one form).  R+B and G are summed in 16-bit lanes:
// 7 taps of 255 fit 11 bits.
__device__ __forceinline__ uint32_t box_pass_wide(const uint32_t* s, int stride, int g, int g0, int n, int rad, uint32_t ww, uint32_t fw) {
  uint32_t rb = 0, gg = 0;
  for (int d = -rad; d <= rad; ++d) {
    const uint32_t p = s[(min(max(g + d, 0), n - 1) - g0) * stride];
    rb += p & 0x00FF00FFu;
    gg += (p >> 8) & 255u;
  }
  const uint32_t lo = s[(max(g - rad - 1, 0) - g0) * stride], hi = s[(min(g + rad + 1, n - 1) - g0) * stride];
  const uint32_t erb = (lo & 0x00FF00FFu) + (hi & 0x00FF00FFu), eg = ((lo >> 8) & 255u) + ((hi >> 8) & 255u);
  const uint32_t r = ((rb & 0xFFFFu) * ww + (erb & 0xFFFFu) * fw + (1u << 23)) >> 24;
  const uint32_t gr = (gg * ww + eg * fw + (1u << 23)) >> 24;
  const uint32_t b = ((rb >> 16) * ww + (erb >> 16) * fw + (1u << 23)) >> 24;
  return r | (gr << 8) | (b << 16);
}

// launch B for rows of box radius up to R (1..3): grid (column tiles, row tiles, frames).  The frame's radius is uniform in the
// block, so every loop bound and barrier below is.
template <int R, bool RAGGED>
__global__ __launch_bounds__(256) void photo_finish_wide_kernel(PhotoArgs pa) {
  constexpr int LW = PHOTO_WIDE_LW(R), LH = PHOTO_WIDE_LH(R);
  const PipelineArgs& a = pa.p;
  const int f = blockIdx.z, x0 = blockIdx.x * PHOTO_TW, y0 = blockIdx.y * PHOTO_TH;
  if (RAGGED && !frame_src<RAGGED>(a, f).img) {     // block-uniform: a bad descriptor row, launch A wrote nothing for the frame
    const float zero[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < PHOTO_TW * PHOTO_TH; i += 256) {
      const int x = x0 + i % PHOTO_TW, y = y0 + i / PHOTO_TW;
      if (x < a.Wo && y < a.Ho) store_pixel(a, f, x, y, zero);
    }
    return;
  }
  const PhotoFrame ph = load_photo(pa.photo + 8 * f, R);
  const uint32_t* in = pa.pix + (size_t)f * a.Ho * a.Wo;
  int cmean = 0;
  if (ph.split < 4) cmean = (int)((double)pa.sums[f] / ((double)a.Ho * (double)a.Wo) + 0.5);     // ImageStat mean, int(m + 0.5)
  if (ph.ww == 0) {     // no blur: pixel by pixel
    for (int i = threadIdx.x; i < PHOTO_TW * PHOTO_TH; i += 256) {
      const int x = x0 + i % PHOTO_TW, y = y0 + i / PHOTO_TW;
      if (x < a.Wo && y < a.Ho) store_normalized(a, f, x, y, photo_post(in[(size_t)y * a.Wo + x], ph, cmean));
    }
    return;
  }
  __shared__ uint32_t buf[2][LH * LW];
  const int step = ph.rad + 1, halo = 3 * step;      // <= PHOTO_WIDE_HALO(R): load_photo clamped rad to R
  const int lw = PHOTO_TW + 2 * halo, lh = PHOTO_TH + 2 * halo;      // the part of the LW x LH tile this frame uses
  const int gx0 = x0 - halo, gy0 = y0 - halo;
  for (int i = threadIdx.x; i < lh * lw; i += 256) {
    const int lx = i % lw, ly = i / lw;
    const int gx = gx0 + lx, gy = gy0 + ly;
    if (gx >= 0 && gx < a.Wo && gy >= 0 && gy < a.Ho) buf[0][ly * LW + lx] = photo_post(in[(size_t)gy * a.Wo + gx], ph, cmean);
  }
  __syncthreads();
  int cur = 0;
  for (int k = 1; k <= 3; ++k) {       // pass k is valid on local columns [k step, lw - k step): pass k-1 was valid step further out
    const int w = lw - 2 * k * step;
    for (int i = threadIdx.x; i < lh * w; i += 256) {
      const int lx = k * step + i % w, ly = i / w;
      const int gx = gx0 + lx, gy = gy0 + ly;
      if (gx < 0 || gx >= a.Wo || gy < 0 || gy >= a.Ho) continue;
      buf[cur ^ 1][ly * LW + lx] = box_pass_wide(buf[cur] + ly * LW, 1, gx, gx0, a.Wo, ph.rad, ph.ww, ph.fw);
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int k = 1; k <= 3; ++k) {       // rows [k step, lh - k step) of the columns [halo, halo + TW) the tile keeps
    const int h = lh - 2 * k * step;
    for (int i = threadIdx.x; i < h * PHOTO_TW; i += 256) {
      const int lx = halo + i % PHOTO_TW, ly = k * step + i / PHOTO_TW;
      const int gx = gx0 + lx, gy = gy0 + ly;
      if (gx >= a.Wo || gy < 0 || gy >= a.Ho) continue;
      buf[cur ^ 1][ly * LW + lx] = box_pass_wide(buf[cur] + lx, LW, gy, gy0, a.Ho, ph.rad, ph.ww, ph.fw);
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int i = threadIdx.x; i < PHOTO_TW * PHOTO_TH; i += 256) {
    const int x = x0 + i % PHOTO_TW, y = y0 + i / PHOTO_TW;
    if (x < a.Wo && y < a.Ho) store_normalized(a, f, x, y, buf[cur][(i / PHOTO_TW + halo) * LW + i % PHOTO_TW + halo]);
  }
}

template <int R>
static void photo_finish_wide_launch(const PhotoArgs& pa, dim3 grid, hipStream_t s) {
  if (pa.p.ragged) hipLaunchKernelGGL((photo_finish_wide_kernel<R, true>), grid, dim3(256), 0, s, pa);
  else hipLaunchKernelGGL((photo_finish_wide_kernel<R, false>), grid, dim3(256), 0, s, pa);
}

long long vfs_photo_workspace_bytes(int F, int Ho, int Wo) {
  return (long long)F * 8 + (long long)F * Ho * Wo * 4;
}

int vfs_crop_resize_flip_photo_norm_launch(const PhotoArgs& pa, hipStream_t s) {
  const PipelineArgs& a = pa.p;
  if (a.B <= 0 || a.V <= 0 || a.T <= 0 || a.Ho <= 0 || a.Wo <= 0) return vfs_set_error(VFS_ERR_SHAPE, "photo pipeline: empty batch");
  const long long F = (long long)a.B * a.V * a.T;
  if (F > 65535) return vfs_set_error(VFS_ERR_SHAPE, "photo pipeline: at most 65535 frames per launch");
  if (pa.max_blur_radius < 0 || pa.max_blur_radius > PHOTO_MAX_RADIUS) return vfs_set_error(VFS_ERR_SHAPE, "photo pipeline: max_blur_radius outside 0..3");
  if (hipMemsetAsync(pa.sums, 0, (size_t)F * 8, s) != hipSuccess) return vfs_set_error(VFS_ERR_LAUNCH, "photo pipeline: memset");
  const long long hw = (long long)a.Ho * a.Wo;
  long long bx = (hw + 255) / 256;
  if (bx > 4096) bx = 4096;
  if (a.ragged) hipLaunchKernelGGL(photo_resize_kernel<true>, dim3((int)bx, (int)F), dim3(256), 0, s, pa);
  else hipLaunchKernelGGL(photo_resize_kernel<false>, dim3((int)bx, (int)F), dim3(256), 0, s, pa);
  int rc = vfs_check_launch("photo_resize");
  if (rc != VFS_OK) return rc;
  const int tx = (a.Wo + PHOTO_TW - 1) / PHOTO_TW, ty = (a.Ho + PHOTO_TH - 1) / PHOTO_TH;
  if (ty > 65535) return vfs_set_error(VFS_ERR_SHAPE, "photo pipeline: output too tall");
  const dim3 grid(tx, ty, (int)F);
  if (pa.max_blur_radius == 1) photo_finish_wide_launch<1>(pa, grid, s);
  else if (pa.max_blur_radius == 2) photo_finish_wide_launch<2>(pa, grid, s);
  else if (pa.max_blur_radius == 3) photo_finish_wide_launch<3>(pa, grid, s);
  else if (a.ragged) hipLaunchKernelGGL(photo_finish_kernel<true>, grid, dim3(256), 0, s, pa);
  else hipLaunchKernelGGL(photo_finish_kernel<false>, grid, dim3(256), 0, s, pa);
  return vfs_check_launch("photo_finish");
}
