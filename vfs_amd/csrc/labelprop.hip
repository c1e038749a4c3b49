// DAVIS label propagation for gfx950: local-window affinity on MFMA + streaming top-k + softmax
// + value gather in ONE kernel, and the kernels of the bilinear-upsample / min-max / argmax post-processing (their text: vfs_segpost.h).
//
// Replaces masked_attention_efficient (mmaction/models/common/local_attention.py:237-348) with
// the circular spatial_neighbor mask (common/affinity_utils.py:144-156), as called per frame by
// VanillaTracker.forward_test (trackers/vanilla_tracker.py:132-181).  The reference materialises
// the dense [T*HW, HW] affinity in chunks of 32 queries and a [HW,HW] boolean mask; here
//   * one workgroup owns an 8x8 tile of queries and walks only the key window that can be inside
//     the circle ((8+2(r-1))^2 keys per key frame), 128 keys per step, channels in K-steps of 64
//     through the same swizzled-LDS / v_mfma_f32_16x16x32_bf16 pipeline as the convolutions
//     (rows = keys, cols = queries: a lane owns 4 keys of ONE query per 16x16 tile)
//   * the mask is the integer test dy^2+dx^2 < r^2, scores are scaled by 1/temperature and fed
//     to a per-lane sorted top-10 list (registers); the 4 lanes that share a query merge through
//     LDS at the end, then softmax over the 10 and the weighted sum of the value logits
//   * features are L2-normalised ONCE per frame when they enter the bank (l2norm kernel), not per
//     propagation step.
#include "vfs_conv.h"
#include "vfs_lpb.h"
#include "vfs_ops.h"
#include "vfs_rows.h"
#include "vfs_segpost.h"

#define LP_TOPK 10

__global__ __launch_bounds__(256) void l2norm_rows_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long long P,
                                                          int C) {
  // one wave per pixel row of C channels (F.normalize(p=2, dim=channel, eps=1e-12)); the row arithmetic is vfs_rows.h's
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  const bf16_t* src = x + (size_t)row * C;
  float ss = 0.f;
  for (int c = lane * 8; c < C; c += 512) ss = rows_bf16_sumsq(ld16(src + c), ss);
  const float inv = rows_bf16_inv(rows_wave_sum(ss));
  for (int c = lane * 8; c < C; c += 512) st16(y + (size_t)row * C + c, rows_bf16_unit(ld16(src + c), inv));
}

int vfs_l2norm_rows_launch(const bf16_t* x, bf16_t* y, long long P, int C, hipStream_t s) {
  if (C % 8) return vfs_set_error(VFS_ERR_SHAPE, "l2norm: C%8");
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, x, y, P, C);
  return vfs_check_launch("l2norm_rows");
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void topk_insert(float (&tv)[LP_TOPK], int (&ti)[LP_TOPK], float s, int id) {
  if (s > tv[LP_TOPK - 1]) { tv[LP_TOPK - 1] = s; ti[LP_TOPK - 1] = id; }
#pragma unroll
  for (int j = LP_TOPK - 1; j > 0; --j) {
    const bool sw = tv[j] > tv[j - 1];
    const float a = tv[j - 1], b = tv[j];
    const int ia = ti[j - 1], ib = ti[j];
    tv[j - 1] = sw ? b : a; tv[j] = sw ? a : b;
    ti[j - 1] = sw ? ib : ia; ti[j] = sw ? ia : ib;
  }
}

// one video (A = LabelPropArgs) or one slot of a lock-step batch (A = LabelPropSlotArgs); nsplit = the key-frame splits of THIS video
// (one video: gridDim.y), blockIdx.y < nsplit
template <class A>
__device__ __forceinline__ void labelprop_body(const A& a, int nsplit) {
  constexpr int BQ = 64, BK = 128, TM = 8;
  __shared__ __attribute__((aligned(16))) bf16_t sK[2][BK * 64];
  __shared__ __attribute__((aligned(16))) bf16_t sQ[2][BQ * 64];
  __shared__ int sKC[BK];   // packed (ky << 16 | kx) of the key rows, -1 = outside the window
  // the merge area aliases sK after the main loop
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int H = a.H, W = a.W, C = a.C, HW = H * W;
  const int tiles_x = (W + 7) >> 3;
  const int qy0 = (blockIdx.x / tiles_x) * 8, qx0 = (blockIdx.x % tiles_x) * 8;
  const int nkt = C >> 6;
  const int j = t & 7, row0 = t >> 3;

  // this lane's query (column lane&15 of the wave's 16-query tile: rows 2*wave, 2*wave+1 of the 8x8 tile)
  const int ql = wave * 16 + lr;
  const int qy = qy0 + (ql >> 3), qx = qx0 + (ql & 7);

  // loader: query rows (fixed for the whole kernel)
  size_t qoff[2];
  bool qok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rr = row0 + 32 * i;
    const int y = qy0 + (rr >> 3), x = qx0 + (rr & 7);
    qok[i] = (y < H) && (x < W);
    qoff[i] = ((size_t)a.qframe * HW + (size_t)(qok[i] ? y * W + x : 0)) * C;
  }

  float tv[LP_TOPK];
  int ti[LP_TOPK];
#pragma unroll
  for (int i = 0; i < LP_TOPK; ++i) { tv[i] = -INFINITY; ti[i] = -1; }

  // key frames are split over blockIdx.y (a DAVIS frame has only 8x14 query tiles: one workgroup
  // per tile would leave most of the 256 CUs idle); every split emits a partial top-k per query
  const int fpb = (a.nkeys + nsplit - 1) / nsplit;
  const int f_begin = (int)blockIdx.y * fpb, f_end = min(a.nkeys, f_begin + fpb);
  for (int f = f_begin; f < f_end; ++f) {
    const int slot = a.kslot[f];
    // the first non_mask_len key frames are not masked (local_attention.py:303-309: with_first_neighbor=False)
    const int r = f < a.non_mask_len ? 0 : a.radius;
    int wy0 = 0, wy1 = H - 1, wx0 = 0, wx1 = W - 1;
    if (r > 0) {
      wy0 = max(0, qy0 - (r - 1)); wy1 = min(H - 1, qy0 + 7 + (r - 1));
      wx0 = max(0, qx0 - (r - 1)); wx1 = min(W - 1, qx0 + 7 + (r - 1));
    }
    const int ww = wx1 - wx0 + 1, nwin = (wy1 - wy0 + 1) * ww;
    const int nkb = (nwin + BK - 1) / BK;
    for (int kb = 0; kb < nkb; ++kb) {
      // key rows of this block
      size_t koff[4];
      bool kok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = kb * BK + row0 + 32 * i;
        kok[i] = kk < nwin;
        const int ky = wy0 + (kok[i] ? kk / ww : 0), kx = wx0 + (kok[i] ? kk % ww : 0);
        koff[i] = ((size_t)slot * HW + (size_t)(ky * W + kx)) * C;
        if (j == 0) sKC[row0 + 32 * i] = kok[i] ? ((ky << 16) | kx) : -1;
      }
      u32x4 kr[4], qr[2];
      auto load_tiles = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) kr[i] = kok[i] ? ld16(a.fbank + koff[i] + kt * 64 + j * 8) : zero16();
#pragma unroll
        for (int i = 0; i < 2; ++i) qr[i] = qok[i] ? ld16(a.fbank + qoff[i] + kt * 64 + j * 8) : zero16();
      };
      auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st16(&sK[buf][lds_off(row0 + 32 * i, j)], kr[i]);
#pragma unroll
        for (int i = 0; i < 2; ++i) st16(&sQ[buf][lds_off(row0 + 32 * i, j)], qr[i]);
      };
      f32x4 acc[TM][1];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) acc[tm][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
      load_tiles(0);
      store_tiles(0);
      __syncthreads();
      for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        if (more) load_tiles(kt + 1);
        mma_kstep<TM, 1, false>(sK[cur], sQ[cur], 0, wave * 16, lane, acc);
        if (more) store_tiles(cur ^ 1);
        __syncthreads();
      }
      // scores -> mask -> streaming top-k (lane: keys tm*16 + 4*lq + reg, query lane&15)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const u32x4 kc = *reinterpret_cast<const u32x4*>(&sKC[tm * 16 + lq * 4]);
        float sc[4];
        int id[4];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int pk = (int)kc[rg];
          const int ky = pk >> 16, kx = pk & 0xffff;
          bool ok = pk >= 0;
          if (r > 0) {
            const int dy = ky - qy, dx = kx - qx;
            ok = ok && (dy * dy + dx * dx < r * r);
          }
          sc[rg] = ok ? acc[tm][0][rg] * a.inv_temp : -INFINITY;
          id[rg] = f * HW + ky * W + kx;
        }
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          if (__any(sc[rg] > tv[LP_TOPK - 1])) topk_insert(tv, ti, sc[rg], id[rg]);
        }
      }
      __syncthreads();   // sKC / tiles are rewritten by the next key block
    }
  }

  // merge the 4 partial lists of every query through LDS (aliases sK), then softmax + value gather
  float* mv = reinterpret_cast<float*>(&sK[0][0]);            // [64 queries][4*TOPK]
  int* mi = reinterpret_cast<int*>(mv + BQ * 4 * LP_TOPK);
#pragma unroll
  for (int i = 0; i < LP_TOPK; ++i) {
    mv[(ql * 4 + lq) * LP_TOPK + i] = tv[i];
    mi[(ql * 4 + lq) * LP_TOPK + i] = ti[i];
  }
  __syncthreads();
  if (t < BQ) {
    const int y = qy0 + (t >> 3), x = qx0 + (t & 7);
    if (y < H && x < W) {
      float* cv = mv + t * 4 * LP_TOPK;
      int* ci = mi + t * 4 * LP_TOPK;
      // top-k of this split's 4 x 10 candidates -> partial list [split][query][LP_TOPK]
      float* pv = a.pval + ((size_t)blockIdx.y * HW + (y * W + x)) * LP_TOPK;
      int* pi = a.pidx + ((size_t)blockIdx.y * HW + (y * W + x)) * LP_TOPK;
      for (int k = 0; k < LP_TOPK; ++k) {
        int best = 0;
        float bvv = cv[0];
        for (int c = 1; c < 4 * LP_TOPK; ++c)
          if (cv[c] > bvv) { bvv = cv[c]; best = c; }
        pv[k] = bvv; pi[k] = ci[best];
        cv[best] = -INFINITY; ci[best] = -1;     // an exhausted list ends in (-inf, -1), not in the id of an entry already taken
      }
    }
  }
}

// merge the per-split partial lists, softmax over the top-k, weighted sum of the value logits
template <class A>
__device__ __forceinline__ void labelprop_merge_body(const A& a, int nsplit) {
  const int HW = a.H * a.W;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= HW) return;
  const int K = a.topk < LP_TOPK ? a.topk : LP_TOPK;
  float bv[LP_TOPK];
  int bi[LP_TOPK];
#pragma unroll
  for (int k = 0; k < LP_TOPK; ++k) { bv[k] = -INFINITY; bi[k] = -1; }
  for (int sp = 0; sp < nsplit; ++sp) {
    const float* pv = a.pval + ((size_t)sp * HW + q) * LP_TOPK;
    const int* pi = a.pidx + ((size_t)sp * HW + q) * LP_TOPK;
    for (int c = 0; c < LP_TOPK; ++c) {
      const float v = pv[c];
      if (v > bv[LP_TOPK - 1]) topk_insert(bv, bi, v, pi[c]);
    }
  }
  const float m = bv[0];
  float wgt[LP_TOPK], z = 0.f;
#pragma unroll
  for (int k = 0; k < LP_TOPK; ++k) {
    wgt[k] = (k < K && bi[k] >= 0 && bv[k] > -INFINITY) ? expf(bv[k] - m) : 0.f;
    z += wgt[k];
  }
  const float iz = 1.0f / z;
  float* o = a.out + (size_t)q * a.CO;
  for (int c = 0; c < a.CO; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LP_TOPK; ++k) {
      if (wgt[k] > 0.f) {
        const int fr = bi[k] / HW, px = bi[k] - fr * HW;
        s += (wgt[k] * iz) * a.sbank[((size_t)a.kslot[fr] * HW + px) * a.CO + c];
      }
    }
    o[c] = s;
  }
}

// ---- the kernels: one video, or slot blockIdx.z of a lock-step batch (arguments built from the slot's descriptor row, as exact_f32.hip)
struct LabelPropSlotArgs {      // LabelPropArgs of one slot; the key list stays in the table
  const bf16_t* fbank; const float* sbank; float* out; float* pval; int* pidx;
  int qframe, nkeys;
  const int* kslot;
  int H, W, C, CO, radius, non_mask_len, topk;
  float inv_temp;
};
// false: the slot sits this step out.  nsplit: the key-frame splits the single-video launch chooses for the slot's nkeys - the top-k
// keeps the first of equal scores, so the order the candidates arrive in (the split) is part of the result
__device__ __forceinline__ bool lp_slot_args(const LpBatchArgs& b, LabelPropSlotArgs& a, int& nsplit) {
  const int n = blockIdx.z;
  LpbRow r;
  if (!lpb_row(b.desc, n, b.Tcap, b.max_nkeys, b.COcap, b.radius, r)) return false;
  const size_t HW = (size_t)b.H * b.W, frames = (size_t)n * b.Tcap * HW;
  a.fbank = b.fbank16 + frames * b.C;
  float* sb = b.sbank + frames * b.COcap;
  a.sbank = sb;
  a.out = sb + (size_t)r.qframe * HW * r.CO;
  a.pval = reinterpret_cast<float*>(b.ws + (size_t)n * b.ws_stride);
  a.pidx = reinterpret_cast<int*>(a.pval + (size_t)LP_MAX_SPLIT * HW * LP_TOPK);
  a.qframe = r.qframe; a.nkeys = r.nkeys; a.kslot = r.kslot;
  a.H = b.H; a.W = b.W; a.C = b.C; a.CO = r.CO; a.radius = b.radius; a.non_mask_len = r.non_mask_len; a.topk = b.topk;
  a.inv_temp = b.inv_temp;
  nsplit = lp_splits_for(r.nkeys, ((b.H + 7) >> 3) * ((b.W + 7) >> 3));
  return true;
}
__global__ __launch_bounds__(256) void labelprop_kernel(LabelPropArgs a) { labelprop_body(a, (int)gridDim.y); }
__global__ __launch_bounds__(256) void labelprop_merge_kernel(LabelPropArgs a, int nsplit) { labelprop_merge_body(a, nsplit); }
__global__ __launch_bounds__(256) void labelprop_batch_kernel(LpBatchArgs b) {
  LabelPropSlotArgs a;
  int nsplit;
  if (!lp_slot_args(b, a, nsplit) || (int)blockIdx.y >= nsplit) return;      // the grid is sized for the slot with the most splits
  labelprop_body(a, nsplit);
}
__global__ __launch_bounds__(256) void labelprop_merge_batch_kernel(LpBatchArgs b) {
  LabelPropSlotArgs a;
  int nsplit;
  if (lp_slot_args(b, a, nsplit)) labelprop_merge_body(a, nsplit);
}

// the checks of both launchers below; who: the entry point in the error text, nkeys: the most key frames a video of the launch has
static int labelprop_check(const char* who, int C, int nkeys, int topk, int H, int W) {
  if (C % 64) return vfs_fail(VFS_ERR_SHAPE, who, "C%64");
  if (nkeys < 1 || nkeys > LP_MAX_KEYS) return vfs_fail(VFS_ERR_SHAPE, who, "1 <= nkeys <= 64");
  if (topk < 1 || topk > LP_TOPK) return vfs_fail(VFS_ERR_SHAPE, who, "1 <= topk <= 10");
  if (H >= 65536 || W >= 65536) return vfs_fail(VFS_ERR_SHAPE, who, "H,W < 65536");
  return VFS_OK;
}

int vfs_labelprop_launch(const LabelPropArgs& a, hipStream_t s) {
  if (int rc = labelprop_check("labelprop", a.C, a.nkeys, a.topk, a.H, a.W)) return rc;
  const int tiles = ((a.H + 7) / 8) * ((a.W + 7) / 8);
  if (a.pval == nullptr || a.pidx == nullptr) return vfs_set_error(VFS_ERR_ARG, "labelprop: partial workspace missing");
  const int nsplit = lp_splits_for(a.nkeys, tiles);
  hipLaunchKernelGGL(labelprop_kernel, dim3(tiles, nsplit), dim3(256), 0, s, a);
  int rc = vfs_check_launch("labelprop");
  if (rc) return rc;
  hipLaunchKernelGGL(labelprop_merge_kernel, dim3((a.H * a.W + 255) / 256), dim3(256), 0, s, a, nsplit);
  return vfs_check_launch("labelprop_merge");
}

// every slot of one lock-step: the two launches of one video, each slot with the key-frame split of its own nkeys
int vfs_labelprop_batch_launch(const LpBatchArgs& b, hipStream_t s) {
  if (int rc = labelprop_check("labelprop_batch", b.C, b.max_nkeys, b.topk, b.H, b.W)) return rc;
  const int tiles = ((b.H + 7) / 8) * ((b.W + 7) / 8);
  int most = 1;
  for (int nk = 1; nk <= b.max_nkeys; ++nk) most = max(most, lp_splits_for(nk, tiles));
  hipLaunchKernelGGL(labelprop_batch_kernel, dim3(tiles, most, b.nslots), dim3(256), 0, s, b);
  int rc = vfs_check_launch("labelprop_batch");
  if (rc) return rc;
  hipLaunchKernelGGL(labelprop_merge_batch_kernel, dim3((b.H * b.W + 255) / 256, 1, b.nslots), dim3(256), 0, s, b);
  return vfs_check_launch("labelprop_merge_batch");
}

// ---------------------------------------------------------------------------------------------
// post-processing of one propagated frame (vanilla_tracker.py:162-181): the bodies and the launcher are vfs_segpost.h's, compiled here
// with the compiler's default contraction (exact_f32.hip compiles the same text without)
__global__ __launch_bounds__(256) void seg_minmax_kernel(const float* __restrict__ seg, float* __restrict__ partial, int H, int W,
                                                         int CO, int Ho, int Wo) {
  seg_minmax_body(seg, partial, H, W, CO, Ho, Wo);
}
__global__ __launch_bounds__(256) void seg_argmax_kernel(const float* __restrict__ seg, const float* __restrict__ partial,
                                                         int nblk, uint8_t* __restrict__ label, int H, int W, int CO, int Ho,
                                                         int Wo) {
  seg_argmax_body(seg, partial, nblk, label, H, W, CO, Ho, Wo);
}
__global__ __launch_bounds__(256) void seg_minmax_batch_kernel(SegPostBatchArgs b) { seg_minmax_batch_body(b); }
__global__ __launch_bounds__(256) void seg_argmax_batch_kernel(SegPostBatchArgs b) { seg_argmax_batch_body(b); }
int vfs_seg_postprocess_batch_launch(const float* sbank, float* partial, uint8_t* preds, const int* desc, int nslots, int Tcap, int Tmaps, int H,
                                     int W, int COcap, int Ho, int Wo, hipStream_t s) {
  const SegPostBatchArgs b{sbank, partial, preds, desc, Tcap, Tmaps, COcap, H, W, Ho, Wo};
  return seg_post_launch("seg_postprocess_batch", "seg_minmax_batch", "seg_argmax_batch", COcap, nslots, Ho, Wo,
                         [&](dim3 g) { hipLaunchKernelGGL(seg_minmax_batch_kernel, g, dim3(256), 0, s, b); },
                         [&](dim3 g) { hipLaunchKernelGGL(seg_argmax_batch_kernel, g, dim3(256), 0, s, b); });
}
int vfs_seg_postprocess_launch(const float* seg, float* partial, uint8_t* label, int H, int W, int CO, int Ho, int Wo,
                               hipStream_t s) {
  return seg_post_launch("seg_postprocess", "seg_minmax", "seg_argmax", CO, 1, Ho, Wo,
                         [&](dim3 g) { hipLaunchKernelGGL(seg_minmax_kernel, g, dim3(256), 0, s, seg, partial, H, W, CO, Ho, Wo); },
                         [&](dim3 g) { hipLaunchKernelGGL(seg_argmax_kernel, g, dim3(256), 0, s, seg, partial, LP_POST_BLOCKS, label, H, W, CO, Ho, Wo); });
}

// one-hot of a uint8 label map into the fp32 seg bank (vanilla_tracker.py:96-100)
__global__ __launch_bounds__(256) void onehot_kernel(const uint8_t* __restrict__ lab, float* __restrict__ out, int P, int CO) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P * CO) return;
  out[i] = (lab[i / CO] == (i % CO)) ? 1.f : 0.f;
}
int vfs_onehot_launch(const uint8_t* lab, float* out, int P, int CO, hipStream_t s) {
  hipLaunchKernelGGL(onehot_kernel, dim3((P * CO + 255) / 256), dim3(256), 0, s, lab, out, P, CO);
  return vfs_check_launch("onehot");
}
