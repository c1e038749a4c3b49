// The per-frame work of the SiamFC probe's tracking loop (projects/siamfc-pytorch/siamfc/siamfc_tracker_base.py:222-297 `update`)
// around the backbone and the cross-correlation: the multi-scale search crops before them, the cubic up-sampling of the
// responses and the peak search after them.  vfs_amd/siamfc.py holds the host (numpy) versions of the same arithmetic -
// `crop_and_resize`, `resize_cubic` and the tail of `SiamFCProbe.update` - and these kernels restate them operation by
// operation: integer arithmetic in the crops, one rounded fp32 product per tap and left-to-right sums in the up-sampling,
// the host's fp32 / fp64 split in the peak search.  Every sum has a fixed order: two runs give identical bits.
//
// All three are small and memory / latency bound (3 x 255 x 255 crop pixels, 3 x 272 x 272 response values): one thread per
// output element, coalesced stores, the 17 x 17 response of a scale in LDS, wave64 shuffle reductions finished through LDS.
#include <math.h>
#include <stdio.h>

#include "vfs_common.h"
#include "vfs_ops.h"

// The host sums rounded products; a fused multiply-add would keep the product exact and change the last bit.
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// vfs_siamfc_crops: crop_and_resize for S boxes of one frame.  The box geometry (rounding, clipping, padding) is computed
// by the host in float64 exactly as crop_and_resize does and arrives as integers; the kernel evaluates the 8-bit bilinear
// resize of `_resize_linear_u8` per output pixel - its per-column / per-row (i0, i1, c1) from the same float64 expressions -
// and the average-colour padding around it.
struct LinTap {
  int i0, i1, c1;
};
__device__ __forceinline__ LinTap lin_tap(int o, int n_in, double scale) {      // `coeffs` of _resize_linear_u8 for one output index
  const double f = ((double)o + 0.5) * scale - 0.5;
  const double fl = floor(f);
  double fr = f - fl;
  int i0 = (int)fl;
  if (i0 < 0) { fr = 0.0; i0 = 0; }
  if (i0 >= n_in - 1) fr = 0.0;
  LinTap t;
  t.i0 = min(i0, n_in - 1);
  t.i1 = min(t.i0 + 1, n_in - 1);
  t.c1 = (int)rint(fr * 2048.0);      // round half to even, as np.rint
  return t;
}

// one output pixel (x, y) of a crop with geometry c of the frame [.][W][3]: v stays as it is where the crop is zeros
__device__ __forceinline__ void crop_pixel(const uint8_t* __restrict__ frame, int W, const SiamCropScale& c, int x, int y, int v[3]) {
  if (!c.valid) return;
  const int ox = x - c.padx, oy = y - c.pady;
  if (ox >= 0 && ox < c.ow && oy >= 0 && oy < c.oh) {
    const LinTap tx = lin_tap(ox, c.iw, c.sx), ty = lin_tap(oy, c.ih, c.sy);
    const int a0 = 2048 - tx.c1, a1 = tx.c1, b0 = 2048 - ty.c1, b1 = ty.c1;
    const uint8_t* r0 = frame + ((size_t)(c.py0 + ty.i0) * W + c.px0) * 3;
    const uint8_t* r1 = frame + ((size_t)(c.py0 + ty.i1) * W + c.px0) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int h0 = r0[tx.i0 * 3 + ch] * a0 + r0[tx.i1 * 3 + ch] * a1;      // horizontal pass, scaled by 2^11
      const int h1 = r1[tx.i0 * 3 + ch] * a0 + r1[tx.i1 * 3 + ch] * a1;
      const int o = ((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16);
      v[ch] = min(max((o + 2) >> 2, 0), 255);
    }
  } else {
    v[0] = c.fill[0]; v[1] = c.fill[1]; v[2] = c.fill[2];
  }
}

__global__ __launch_bounds__(256) void siamfc_crops_kernel(SiamCropArgs a) {
  const int s = blockIdx.y;
  const int n = a.out_size * a.out_size;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int y = e / a.out_size, x = e - y * a.out_size;
  int v[3] = {0, 0, 0};
  crop_pixel(a.frame, a.W, a.sc[s], x, y, v);
  float* o = a.out + (size_t)s * 3 * n + e;
  o[0] = (float)v[0];
  o[n] = (float)v[1];
  o[2 * (size_t)n] = (float)v[2];
}

int vfs_siamfc_crops_launch(const SiamCropArgs& a, hipStream_t s) {
  if (a.S < 1 || a.S > VFS_SIAMFC_MAX_SCALES) return vfs_set_error(VFS_ERR_SHAPE, "siamfc_crops: 1 <= S <= 8");
  if (a.H < 1 || a.W < 1 || a.out_size < 1 || a.out_size > 4096) return vfs_set_error(VFS_ERR_SHAPE, "siamfc_crops: H, W >= 1, 1 <= out_size <= 4096");
  for (int i = 0; i < a.S; ++i) {      // every source read and every patch pixel inside its array
    const SiamCropScale& c = a.sc[i];
    if (!c.valid) continue;
    if (!vfs_siamfc_source_inside(c, a.H, a.W))
      return vfs_set_error(VFS_ERR_ARG, "siamfc_crops: source patch outside the frame");
    if (!vfs_siamfc_target_inside(c, a.out_size))
      return vfs_set_error(VFS_ERR_ARG, "siamfc_crops: resized patch outside the crop");
  }
  const int n = a.out_size * a.out_size;
  hipLaunchKernelGGL(siamfc_crops_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)a.S), dim3(256), 0, s, a);
  return vfs_check_launch("siamfc_crops");
}

// ---------------------------------------------------------------------------------------------
// vfs_siamfc_upsample: resize_cubic of S response maps [r][r] -> [up][up] (Keys kernel, A = -0.75; the tap indices and fp32
// weights are the host's, one table for both axes), times the scale penalty, plus the maximum of every penalised map.
// Horizontal pass then vertical pass, each value ((p0 + p1) + p2) + p3 of four rounded fp32 products - the order of numpy's
// `.sum` over four elements.  A horizontal value is recomputed by the threads that need it (same operations, same bits): the
// whole op is 8 MFLOP on 289 LDS-resident floats per scale, an intermediate image would only add a barrier and a round trip.
//
// The maximum travels as a 64-bit key: the float mapped to an unsigned integer of the same order in the high half, ~index in
// the low half - the largest key is the largest value at its lowest flat index (np.argmax's tie rule), and an integer maximum
// does not depend on the order of its operands, so the one atomic per workgroup keeps the result reproducible.
__device__ __forceinline__ unsigned long long peak_key(float v, unsigned idx) {
  if (v == 0.f) v = 0.f;      // -0 == +0 for argmax
  unsigned u = __builtin_bit_cast(unsigned, v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (0xffffffffu - idx);
}
__device__ __forceinline__ float peak_key_value(unsigned long long k) {
  unsigned u = (unsigned)(k >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __builtin_bit_cast(float, u);
}

__global__ __launch_bounds__(256) void siamfc_upsample_kernel(const float* __restrict__ resp, const int* __restrict__ tap_idx,
                                                              const float* __restrict__ tap_w, const float* __restrict__ penalty,
                                                              float* __restrict__ up_out, unsigned long long* scale_max, int r, int up) {
  __shared__ float sa[VFS_SIAMFC_MAX_RESP];
  __shared__ unsigned long long red[4];
  const int s = blockIdx.y, slot = blockIdx.z, t = threadIdx.x;      // map [s][slot] of [S][N]: the single-sequence call is N = 1
  const size_t m = (size_t)s * gridDim.z + slot;
  for (int i = t; i < r * r; i += 256) sa[i] = resp[m * r * r + i];
  __syncthreads();
  const int n = up * up;
  const int e = blockIdx.x * 256 + t;
  unsigned long long key = 0;      // below the key of every number
  if (e < n) {
    const int y = e / up, x = e - y * up;
    const u32x4 xv = ld16(tap_idx + 4 * x), yv = ld16(tap_idx + 4 * y);
    const f32x4 xw = *reinterpret_cast<const f32x4*>(tap_w + 4 * x), yw = *reinterpret_cast<const f32x4*>(tap_w + 4 * y);
    int xi[4], yi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // a table entry outside the map must not become an LDS address
      xi[k] = min(max((int)xv[k], 0), r - 1);
      yi[k] = min(max((int)yv[k], 0), r - 1);
    }
    float rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* ar = sa + yi[k] * r;
      const float p0 = ar[xi[0]] * xw[0], p1 = ar[xi[1]] * xw[1], p2 = ar[xi[2]] * xw[2], p3 = ar[xi[3]] * xw[3];
      rows[k] = ((p0 + p1) + p2) + p3;
    }
    const float q0 = rows[0] * yw[0], q1 = rows[1] * yw[1], q2 = rows[2] * yw[2], q3 = rows[3] * yw[3];
    const float v = (((q0 + q1) + q2) + q3) * penalty[s];
    up_out[m * n + e] = v;
    key = peak_key(v, (unsigned)e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) red[t >> 6] = key;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) key = red[w] > key ? red[w] : key;
    __hip_atomic_fetch_max(scale_max + (size_t)slot * gridDim.y + s, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

int vfs_siamfc_upsample_launch(const float* resp, const int* tap_idx, const float* tap_w, const float* penalty, float* up_out,
                               unsigned long long* scale_max, int S, int r, int up, hipStream_t s) {
  if (S < 1 || S > VFS_SIAMFC_MAX_SCALES) return vfs_set_error(VFS_ERR_SHAPE, "siamfc_upsample: 1 <= S <= 8");
  if (r < 1 || r * r > VFS_SIAMFC_MAX_RESP || up < 1 || up > 4096)
    return vfs_set_error(VFS_ERR_SHAPE, "siamfc_upsample: r * r <= 1024, 1 <= up <= 4096");
  if (hipMemsetAsync(scale_max, 0, (size_t)S * sizeof(unsigned long long), s) != hipSuccess)
    return vfs_set_error(VFS_ERR_LAUNCH, "siamfc_upsample: clearing the per-scale maxima failed");
  const int n = up * up;
  hipLaunchKernelGGL(siamfc_upsample_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)S), dim3(256), 0, s, resp, tap_idx, tap_w, penalty,
                     up_out, scale_max, r, up);
  return vfs_check_launch("siamfc_upsample");
}

// ---------------------------------------------------------------------------------------------
// vfs_siamfc_peak: the tail of `update` on the penalised maps, ONE workgroup (74 k values, three passes out of the L2):
//   scale_id = argmax of the per-scale maxima (first one on ties);  x = map[scale_id]
//   x -= min(x)                       fp32, the minimum is exact
//   x /= sum(x) + 1e-16               the sum accumulated in fp64 and rounded to fp32; the division in fp32
//   b = (1 - wi) * x  +  wi * hann    the first product in fp32 (an fp32 array times a scalar), the rest in fp64
//   (row, col) = argmax b             lowest flat index on ties
// Each thread walks its indices in ascending order, the wave reduces by shuffles, thread 0 finishes over the 16 waves in
// order: no atomics, a fixed order.
#define PEAK_THREADS 1024
#define PEAK_WAVES (PEAK_THREADS / 64)
// The search on the S maps maps[s * map_stride ..] with their maxima scale_max[s]: thread 0 returns with the scale and the flat
// index of the peak, the other threads with partial results.
__device__ __forceinline__ void peak_search(const float* __restrict__ maps, size_t map_stride, const unsigned long long* __restrict__ scale_max,
                                            const double* __restrict__ hann, int S, int up, float one_minus_wi, double wi, int& sid, int& bi) {
  __shared__ float red_min[PEAK_WAVES];
  __shared__ double red_sum[PEAK_WAVES];
  __shared__ double red_val[PEAK_WAVES];
  __shared__ int red_idx[PEAK_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = up * up;
  sid = 0;
  float best = peak_key_value(scale_max[0]);
  for (int s = 1; s < S; ++s) {
    const float v = peak_key_value(scale_max[s]);
    if (v > best) { best = v; sid = s; }
  }
  const float* x = maps + (size_t)sid * map_stride;

  float mn = INFINITY;
  for (int i = t; i < n; i += PEAK_THREADS) mn = fminf(mn, x[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if (lane == 0) red_min[wave] = mn;
  __syncthreads();
  mn = red_min[0];
  for (int w = 1; w < PEAK_WAVES; ++w) mn = fminf(mn, red_min[w]);

  double sum = 0.0;
  for (int i = t; i < n; i += PEAK_THREADS) sum += (double)(x[i] - mn);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) red_sum[wave] = sum;
  __syncthreads();
  sum = red_sum[0];
  for (int w = 1; w < PEAK_WAVES; ++w) sum += red_sum[w];
  const float den = (float)sum + 1e-16f;

  double bv = -INFINITY;
  bi = 0x7fffffff;
  for (int i = t; i < n; i += PEAK_THREADS) {
    const float q = (x[i] - mn) / den;
    const float p = one_minus_wi * q;
    const double h = wi * hann[i];
    const double b = (double)p + h;
    if (b > bv) { bv = b; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { red_val[wave] = bv; red_idx[wave] = bi; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < PEAK_WAVES; ++w)
      if (red_val[w] > bv || (red_val[w] == bv && red_idx[w] < bi)) { bv = red_val[w]; bi = red_idx[w]; }
    if (bi >= n) bi = 0;      // a map without a single comparable value (all NaN): np.argmax answers 0
  }
}

__global__ __launch_bounds__(PEAK_THREADS) void siamfc_peak_kernel(const float* __restrict__ up_in, const unsigned long long* __restrict__ scale_max,
                                                                   const double* __restrict__ hann, int* __restrict__ record, int S, int up,
                                                                   float one_minus_wi, double wi) {
  int sid, bi;
  peak_search(up_in, (size_t)up * up, scale_max, hann, S, up, one_minus_wi, wi, sid, bi);
  if (threadIdx.x == 0) {
    const u32x4 rec = {(unsigned)sid, (unsigned)(bi / up), (unsigned)(bi % up), 0u};
    st16(record, rec);
  }
}

int vfs_siamfc_peak_launch(const float* up_in, const unsigned long long* scale_max, const double* hann, int* record, int S, int up,
                           float one_minus_wi, double wi, hipStream_t s) {
  if (S < 1 || S > VFS_SIAMFC_MAX_SCALES) return vfs_set_error(VFS_ERR_SHAPE, "siamfc_peak: 1 <= S <= 8");
  if (up < 1 || up > 4096) return vfs_set_error(VFS_ERR_SHAPE, "siamfc_peak: 1 <= up <= 4096");
  if ((size_t)record & 15) return vfs_set_error(VFS_ERR_ARG, "siamfc_peak: the record must be 16-byte aligned");
  hipLaunchKernelGGL(siamfc_peak_kernel, dim3(1), dim3(PEAK_THREADS), 0, s, up_in, scale_max, hann, record, S, up, one_minus_wi, wi);
  return vfs_check_launch("siamfc_peak");
}

// ---------------------------------------------------------------------------------------------
// The batched loop: N <= 64 slots (one sequence each) advance in lock-step, and the tracker state lives on the device
// (layout in include/vfs_hip.h: state fp64 [N][8], meta int32 [N][8], frame_off int64 [N]).  The three kernels are the ones
// above with a slot dimension - crop_pixel / lin_tap, the up-sampling kernel itself, peak_search - plus what the host loop does
// between them, restated in the types numpy really uses there (NEP 50 promotion, vfs_amd/siamfc.py):
//   center, target_sz   float32 ARRAYS updated in place from float64 operands:  center = f32(f64(center) + disp_in_image),
//                       target_sz = f32(f64(target_sz) * scale).  The state holds them widened (exact).
//   z_sz, x_sz          float32 scalars after init(), float64 from the first _apply_peak on (f32 scalar * f64 scalar -> f64).
//                       A double holds both exactly.
//   x_sz * factors[s] and every quantity of crop_params: float64; np.round / np.rint round half to even (rint here).
//   the returned box    [center[1] + 1 - (target_sz[1] - 1) / 2, ...]: float32 scalars with weak Python constants - float32
//                       arithmetic; widened to float64 only when the boxes are stacked.
// `#pragma clang fp contract(off)` above covers all of it: no product feeds an addition unrounded.
//
// The geometry comes from device memory, so no address is formed from it before it is checked: vfs_siamfc_crop_geometry
// (siamfc_batch.h) refuses a state that is not finite or not below 2^30 before any conversion to int and re-checks the two
// rectangle conditions of vfs_siamfc_crops_launch; a slot that fails has zero crops and a status bit.
__global__ __launch_bounds__(256) void siamfc_batch_crops_kernel(SiamBatchCropArgs a) {
  const int s = blockIdx.y, slot = blockIdx.z;
  const int n = a.out_size * a.out_size;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int y = e / a.out_size, x = e - y * a.out_size;
  int* meta = a.meta + (size_t)slot * VFS_SIAMFC_META_WORDS;
  int v[3] = {0, 0, 0};
  if (meta[0] != 0) {      // an inactive slot: zeros, and nothing else of the slot is read
    const double* st = a.state + (size_t)slot * VFS_SIAMFC_STATE_WORDS;
    const int H = meta[1], W = meta[2];
    const double size = a.use_z ? st[4] : st[5] * a.factors[s];
    const long long off = a.frame_off[slot];
    SiamCropScale c;
    int status = vfs_siamfc_crop_geometry(H, W, st[0], st[1], size, a.out_size, c);
    if (off < 0) { status |= VFS_SIAMFC_STATUS_STATE; c.valid = 0; }
    if (status && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(meta + 7, status);
    if (e < n) {
      c.fill[0] = meta[3]; c.fill[1] = meta[4]; c.fill[2] = meta[5];
      crop_pixel(a.frames + off * (c.valid != 0), W, c, x, y, v);
    }
  }
  if (e >= n) return;
  float* o = a.out + ((size_t)s * a.N + slot) * 3 * n + e;
  o[0] = (float)v[0];
  o[n] = (float)v[1];
  o[2 * (size_t)n] = (float)v[2];
}

static int batch_refuse(const char* entry, const char* what, int shape) {
  static thread_local char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", entry, what);
  return vfs_set_error(shape ? VFS_ERR_SHAPE : VFS_ERR_ARG, msg);
}

int vfs_siamfc_batch_crops_launch(const SiamBatchCropArgs& a, hipStream_t s) {
  int shape;
  SiamBatchGrid g;
  if (const char* e = vfs_siamfc_batch_crops_check(a.frames, a.frame_off, a.state, a.meta, a.factors, a.out, a.N, a.S, a.out_size, a.use_z, &shape, &g))
    return batch_refuse("siamfc_batch_crops", e, shape);
  hipLaunchKernelGGL(siamfc_batch_crops_kernel, dim3(g.x, g.y, g.z), dim3(g.threads), 0, s, a);
  return vfs_check_launch("siamfc_batch_crops");
}

int vfs_siamfc_batch_upsample_launch(const float* resp, const int* tap_idx, const float* tap_w, const float* penalty, float* up_out,
                                     unsigned long long* scale_max, int N, int S, int r, int up, hipStream_t s) {
  int shape;
  SiamBatchGrid g;
  if (const char* e = vfs_siamfc_batch_upsample_check(resp, tap_idx, tap_w, penalty, up_out, scale_max, N, S, r, up, &shape, &g))
    return batch_refuse("siamfc_batch_upsample", e, shape);
  if (hipMemsetAsync(scale_max, 0, (size_t)N * S * sizeof(unsigned long long), s) != hipSuccess)
    return vfs_set_error(VFS_ERR_LAUNCH, "siamfc_batch_upsample: clearing the per-scale maxima failed");
  hipLaunchKernelGGL(siamfc_upsample_kernel, dim3(g.x, g.y, g.z), dim3(g.threads), 0, s, resp, tap_idx, tap_w, penalty, up_out, scale_max, r, up);
  return vfs_check_launch("siamfc_batch_upsample");
}

// One workgroup per slot: peak_search on the slot's S maps, then one lane applies SiamFCProbe._apply_peak to the slot's state and
// writes the frame's box and triple to row meta.row.  An inactive slot is left untouched in every word; so is one whose row
// lies outside [0, rows_cap), except for its status bit.
__global__ __launch_bounds__(PEAK_THREADS) void siamfc_batch_peak_kernel(SiamBatchPeakArgs a) {
  const int slot = blockIdx.x;
  int* meta = a.meta + (size_t)slot * VFS_SIAMFC_META_WORDS;
  if (meta[0] == 0) return;      // the same for every thread of the workgroup: no barrier is skipped by some
  const int row = meta[6];
  if (row < 0 || row >= a.rows_cap) {
    if (threadIdx.x == 0) atomicOr(meta + 7, VFS_SIAMFC_STATUS_ROWS);
    return;
  }
  const size_t n = (size_t)a.up * a.up;
  int sid, bi;
  peak_search(a.up_in + (size_t)slot * n, (size_t)a.N * n, a.scale_max + (size_t)slot * a.S, a.hann, a.S, a.up, a.one_minus_wi, a.wi, sid, bi);
  if (threadIdx.x != 0) return;
  const int prow = bi / a.up, pcol = bi % a.up;
  double* st = a.state + (size_t)slot * VFS_SIAMFC_STATE_WORDS;
  const double sf = a.factors[sid], x_sz = st[5];
  const double half = (double)(a.up - 1) / 2;
  const double loc[2] = {(double)prow, (double)pcol};
  float center[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double disp_in_response = loc[k] - half;
    const double disp_in_instance = disp_in_response * a.total_stride / a.response_up;
    const double disp_in_image = disp_in_instance * x_sz * sf / a.instance_sz;
    center[k] = (float)(st[k] + disp_in_image);
  }
  const double scale = (1 - a.scale_lr) * 1.0 + a.scale_lr * sf;
  const float th = (float)(st[2] * scale), tw = (float)(st[3] * scale);
  st[0] = (double)center[0];
  st[1] = (double)center[1];
  st[2] = (double)th;
  st[3] = (double)tw;
  st[4] = st[4] * scale;
  st[5] = x_sz * scale;
  double* box = a.boxes + (size_t)row * 4;
  box[0] = (double)(center[1] + 1.f - (tw - 1.f) / 2.f);
  box[1] = (double)(center[0] + 1.f - (th - 1.f) / 2.f);
  box[2] = (double)tw;
  box[3] = (double)th;
  const u32x4 rec = {(unsigned)sid, (unsigned)prow, (unsigned)pcol, 0u};
  st16(a.records + (size_t)row * 4, rec);
  meta[6] = row + 1;
}

int vfs_siamfc_batch_peak_launch(const SiamBatchPeakArgs& a, hipStream_t s) {
  int shape;
  SiamBatchGrid g;
  if (const char* e = vfs_siamfc_batch_peak_check(a.up_in, a.scale_max, a.hann, a.factors, a.state, a.meta, a.boxes, a.records, a.rows_cap, a.N, a.S,
                                                  a.up, &shape, &g))
    return batch_refuse("siamfc_batch_peak", e, shape);
  hipLaunchKernelGGL(siamfc_batch_peak_kernel, dim3(g.x, g.y, g.z), dim3(g.threads), 0, s, a);
  return vfs_check_launch("siamfc_batch_peak");
}
