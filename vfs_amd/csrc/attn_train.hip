// Differentiable masked_attention (mmaction/models/common/local_attention.py:161-234 with mask = spatial_neighbor(...,
// mode='circle'), affinity_utils.py:144-156): the local top-k attention of the correspondence losses, forward and backward wrt
// query, key and value.  fp32 NCHW operands, as the grad-mode ResNet.forward returns them:
//     query [N][C][HW]     key [N][C][T*HW]     value [N][CO][T*HW]     out [N][CO][HW]
// score(i, j) = <k^_i, q^_j> / temperature over the in-window keys i of query j (k^, q^: F.normalize(dim=1, eps 1e-12) when
// `normalize`), the k largest in the total order of vfs_lpx.h (larger score first, equal scores: lower flat key index first),
// softmax over those k, out_j = sum_a w_a v_{i_a}.  The window - (y - y')^2 + (x - x')^2 < (neighbor_range / 2)^2, the same for
// every key frame - is a test in the kernel; no mask and no [T*HW][HW] affinity exists anywhere.
//
// Positions are the CONTIGUOUS axis of these tensors, so a lane owns a POSITION (a query in the forward, the score gradient and
// dq; a key in dk / dv) and walks channels: every load of a wave is one coalesced row segment, or a broadcast.  The scores stay
// on the VALU: at the 4 x 4 .. 32 x 32 maps of a loss a query's window is a few dozen to a few hundred keys - a 32 x 32 MFMA tile
// of (key, query) pairs would be mostly out-of-window pairs that the selection then has to throw away, and the lane-per-query
// form needs no cross-lane step at all: the running top-k of a query lives in its lane's registers.
//
// Determinism: no atomics.  Every output element is written by exactly one lane, which adds its terms in a fixed order (channels
// ascending; selected keys in list order; for dk / dv the queries that can reach the key in ascending flat index).  The top-k
// lists of a query's four key slices are merged under a TOTAL order, so the merged list does not depend on the slicing.
#include "vfs_lpx.h"

#define AT_QT 64       // queries (forward) / positions (backward) per wave
#define AT_KS 4        // key slices of a query tile = waves of a forward workgroup
#define AT_EB 8        // candidate keys whose scores a lane accumulates side by side (one query load feeds AT_EB fmaf)
#define AT_CB 16       // channels a wave of the dq / dk / dv kernels accumulates per position

struct AttnArgs {
  const float *q, *k, *v, *dout, *invq, *invk, *w, *ds;
  const int* idx;
  float *out, *wout, *dsout, *dst;
  int* idxout;
  int N, C, T, H, W, CO, rad, K;      // rad = neighbor_range / 2, 0 = no window; K = topk
  float temp;
};

// half width of the window row dy: the largest dx >= 0 with dx^2 + dy^2 < rad^2, clipped to the map (-1: the row is empty)
__device__ __forceinline__ int attn_row_half_width(int dy, int rad, int W) {
  int hw = min(rad - 1, W - 1);
  while (hw >= 0 && hw * hw + dy * dy >= rad * rad) --hw;
  return hw;
}

// ---- forward: one workgroup = one sample x AT_QT queries; wave wv scores the window rows (frame, dy) wv, wv + 4, ... (without a
// window: the key chunks wv, wv + 4, ...) and keeps a sorted top-10 per query; wave 0 merges the four lists, applies the softmax
// and saves the K indices (-1: the zero-weight fill of a query with fewer than K in-window keys) and weights, [N][K][HW]; then
// the four waves split the output channels.
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs p) {
  __shared__ float ms[AT_KS][LPX_TOPK][AT_QT];
  __shared__ int mi[AT_KS][LPX_TOPK][AT_QT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = blockIdx.y;
  const int HW = p.H * p.W, THW = p.T * HW;
  const int j = blockIdx.x * AT_QT + lane;
  const bool vq = j < HW;
  const int jc = vq ? j : HW - 1;
  const int y = jc / p.W, x = jc - y * p.W;
  const float* qb = p.q + (size_t)n * p.C * HW + jc;
  const float* kb = p.k + (size_t)n * p.C * THW;
  const float iq = p.invq ? p.invq[(size_t)n * HW + jc] : 1.0f;
  const float* ikb = p.invk ? p.invk + (size_t)n * THW : nullptr;
  float tv[LPX_TOPK];
  int ti[LPX_TOPK];
#pragma unroll
  for (int a = 0; a < LPX_TOPK; ++a) { tv[a] = -INFINITY; ti[a] = LPX_NONE; }

  // one chunk: scores of AT_EB candidate keys (id[u], valid ok[u]) of this lane's query
  auto score_chunk = [&](const int (&id)[AT_EB], const bool (&ok)[AT_EB]) {
    float acc[AT_EB];
#pragma unroll
    for (int u = 0; u < AT_EB; ++u) acc[u] = 0.0f;
    for (int c = 0; c < p.C; ++c) {
      const float qv = qb[(size_t)c * HW] * iq;
      const float* kc = kb + (size_t)c * THW;
#pragma unroll
      for (int u = 0; u < AT_EB; ++u) acc[u] = __builtin_fmaf(qv, kc[id[u]], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < AT_EB; ++u)
      if (ok[u] && vq) lpx_insert(tv, ti, (ikb ? acc[u] * ikb[id[u]] : acc[u]) / p.temp, id[u]);
  };

  if (p.rad > 0) {
    const int DY = min(p.rad - 1, p.H - 1), rows = 2 * DY + 1;
    for (int rr = wv; rr < p.T * rows; rr += AT_KS) {
      const int t = rr / rows, dy = rr - t * rows - DY;
      const int hw = attn_row_half_width(dy, p.rad, p.W);
      const int yy = y + dy;
      const bool vy = yy >= 0 && yy < p.H;
      for (int dx0 = -hw; dx0 <= hw; dx0 += AT_EB) {
        int id[AT_EB];
        bool ok[AT_EB];
#pragma unroll
        for (int u = 0; u < AT_EB; ++u) {
          const int xx = x + dx0 + u;
          ok[u] = vy && dx0 + u <= hw && xx >= 0 && xx < p.W;
          id[u] = ok[u] ? t * HW + yy * p.W + xx : 0;
        }
        score_chunk(id, ok);
      }
    }
  } else {
    for (int e0 = wv * AT_EB; e0 < THW; e0 += AT_KS * AT_EB) {
      int id[AT_EB];
      bool ok[AT_EB];
#pragma unroll
      for (int u = 0; u < AT_EB; ++u) {
        ok[u] = e0 + u < THW;
        id[u] = ok[u] ? e0 + u : 0;
      }
      score_chunk(id, ok);
    }
  }
#pragma unroll
  for (int a = 0; a < LPX_TOPK; ++a) { ms[wv][a][lane] = tv[a]; mi[wv][a][lane] = ti[a]; }
  __syncthreads();
  if (wv == 0) {
    for (int s = 1; s < AT_KS; ++s)
#pragma unroll
      for (int a = 0; a < LPX_TOPK; ++a)
        if (mi[s][a][lane] != LPX_NONE) lpx_insert(tv, ti, ms[s][a][lane], mi[s][a][lane]);
    // softmax over the first K entries (tv is sorted: tv[0] is the maximum; the query itself is always in its window)
    float e[LPX_TOPK], sum = 0.0f;
#pragma unroll
    for (int a = 0; a < LPX_TOPK; ++a) {
      e[a] = (a < p.K && ti[a] != LPX_NONE) ? vexp(tv[a] - tv[0]) : 0.0f;
      sum += e[a];
    }
#pragma unroll
    for (int a = 0; a < LPX_TOPK; ++a) {
      const bool sel = a < p.K && ti[a] != LPX_NONE;
      const float wa = sel ? e[a] / sum : 0.0f;
      const int ia = sel ? ti[a] : -1;
      ms[0][a][lane] = wa;
      mi[0][a][lane] = ia;
      if (a < p.K && vq) {
        p.wout[((size_t)n * p.K + a) * HW + j] = wa;
        p.idxout[((size_t)n * p.K + a) * HW + j] = ia;
      }
    }
  }
  __syncthreads();
  if (!vq) return;
  const float* vb = p.v + (size_t)n * p.CO * THW;
  for (int co = wv; co < p.CO; co += AT_KS) {
    float acc = 0.0f;
#pragma unroll
    for (int a = 0; a < LPX_TOPK; ++a) {
      const int ia = mi[0][a][lane];
      if (ia >= 0) acc = __builtin_fmaf(ms[0][a][lane], vb[(size_t)co * THW + ia], acc);
    }
    p.out[((size_t)n * p.CO + co) * HW + j] = acc;
  }
}

// ---- backward 1: the score gradients.  g_a = <v_{i_a}, dout_j>, ds_a = w_a (g_a - sum_b w_b g_b) / temperature; [N][K][HW].
// One lane = one query; the fill (index -1, weight 0) gives ds = 0.
__global__ __launch_bounds__(256) void attn_ds_kernel(AttnArgs p) {
  const int HW = p.H * p.W, THW = p.T * HW, n = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= HW) return;
  int ia[LPX_TOPK];
  float wa[LPX_TOPK], g[LPX_TOPK];
#pragma unroll
  for (int a = 0; a < LPX_TOPK; ++a) {
    ia[a] = a < p.K ? p.idx[((size_t)n * p.K + a) * HW + j] : -1;
    if (ia[a] >= THW) ia[a] = -1;      // not an index the forward wrote: never dereferenced
    wa[a] = ia[a] >= 0 ? p.w[((size_t)n * p.K + a) * HW + j] : 0.0f;
    g[a] = 0.0f;
  }
  const float* vb = p.v + (size_t)n * p.CO * THW;
  const float* db = p.dout + (size_t)n * p.CO * HW + j;
  for (int co = 0; co < p.CO; ++co) {
    const float d = db[(size_t)co * HW];
#pragma unroll
    for (int a = 0; a < LPX_TOPK; ++a)
      if (ia[a] >= 0) g[a] = __builtin_fmaf(vb[(size_t)co * THW + ia[a]], d, g[a]);
  }
  float bar = 0.0f;
#pragma unroll
  for (int a = 0; a < LPX_TOPK; ++a) bar = __builtin_fmaf(wa[a], g[a], bar);
#pragma unroll
  for (int a = 0; a < LPX_TOPK; ++a)
    if (a < p.K) p.dsout[((size_t)n * p.K + a) * HW + j] = wa[a] * (g[a] - bar) / p.temp;
}

// ---- backward 2: dq^[c][j] = sum_a ds_a k^[c][i_a] (the gradient wrt the NORMALISED query; the normalisation's backward is
// vfs_simloss_norm_bwd_launch).  One workgroup = AT_QT queries x 4 waves x AT_CB channels.
__global__ __launch_bounds__(256) void attn_dq_kernel(AttnArgs p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = blockIdx.z;
  const int HW = p.H * p.W, THW = p.T * HW;
  const int j = blockIdx.x * AT_QT + lane;
  const int c0 = (blockIdx.y * 4 + wv) * AT_CB;
  if (j >= HW || c0 >= p.C) return;
  int ia[LPX_TOPK];
  float cf[LPX_TOPK];
#pragma unroll
  for (int a = 0; a < LPX_TOPK; ++a) {
    ia[a] = a < p.K ? p.idx[((size_t)n * p.K + a) * HW + j] : -1;
    if (ia[a] >= THW) ia[a] = -1;
    cf[a] = 0.0f;
    if (ia[a] >= 0) cf[a] = p.ds[((size_t)n * p.K + a) * HW + j] * (p.invk ? p.invk[(size_t)n * THW + ia[a]] : 1.0f);
  }
  const float* kb = p.k + (size_t)n * p.C * THW;
  for (int c = c0; c < c0 + AT_CB && c < p.C; ++c) {
    float acc = 0.0f;
#pragma unroll
    for (int a = 0; a < LPX_TOPK; ++a)
      if (ia[a] >= 0) acc = __builtin_fmaf(cf[a], kb[(size_t)c * THW + ia[a]], acc);
    p.dst[((size_t)n * p.C + c) * HW + j] = acc;
  }
}

// ---- backward 3: the sums over the inverted relation, dk^ and dv.  dst[ch][i] = sum over the (j, a) with i_a(j) = i of
// coef[a][j] * src[ch][j] * scale[j]   (dk^: coef = ds, src = query, scale = invq;  dv: coef = w, src = dout, no scale).
// One lane = one key i; it scans the queries that can reach it - its own window (the window is symmetric), every query without
// one - in ASCENDING flat index and looks i up in their saved lists (a key is in a list at most once); nothing is scattered,
// so there is nothing to make atomic.  One workgroup = AT_QT keys x 4 waves x AT_CB channels.
__global__ __launch_bounds__(256) void attn_inv_kernel(const float* __restrict__ coef, const float* __restrict__ src,
                                                       const float* __restrict__ scale, float* __restrict__ dst, const int* __restrict__ idx,
                                                       int CH, int T, int H, int W, int rad, int K) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = blockIdx.z;
  const int HW = H * W, THW = T * HW;
  const int i = blockIdx.x * AT_QT + lane;
  const int c0 = (blockIdx.y * 4 + wv) * AT_CB;
  if (i >= THW || c0 >= CH) return;
  const int pos = i % HW, y = pos / W, x = pos - y * W;
  const int* ib = idx + (size_t)n * K * HW;
  const float* cb = coef + (size_t)n * K * HW;
  const float* sb = src + (size_t)n * CH * HW;
  float acc[AT_CB];
#pragma unroll
  for (int cc = 0; cc < AT_CB; ++cc) acc[cc] = 0.0f;

  auto visit = [&](int j) {
    float cf = 0.0f;
    bool hit = false;
    for (int a = 0; a < K; ++a)
      if (ib[(size_t)a * HW + j] == i) { cf = cb[(size_t)a * HW + j]; hit = true; }
    if (hit) {
      if (scale) cf *= scale[(size_t)n * HW + j];
#pragma unroll
      for (int cc = 0; cc < AT_CB; ++cc)
        if (c0 + cc < CH) acc[cc] = __builtin_fmaf(cf, sb[(size_t)(c0 + cc) * HW + j], acc[cc]);
    }
  };

  if (rad > 0) {
    const int DY = min(rad - 1, H - 1);
    for (int dy = -DY; dy <= DY; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      const int hw = attn_row_half_width(dy, rad, W);
      for (int dx = -hw; dx <= hw; ++dx) {
        const int xx = x + dx;
        if (xx >= 0 && xx < W) visit(yy * W + xx);
      }
    }
  } else {
    for (int j = 0; j < HW; ++j) visit(j);
  }
#pragma unroll
  for (int cc = 0; cc < AT_CB; ++cc)
    if (c0 + cc < CH) dst[((size_t)n * CH + c0 + cc) * THW + i] = acc[cc];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static AttnArgs attn_args(const AttnShape& s) {
  AttnArgs p{};
  p.N = s.N; p.C = s.C; p.T = s.T; p.H = s.H; p.W = s.W; p.CO = s.CO; p.K = s.topk; p.temp = s.temperature;
  p.rad = s.neighbor_range > 0 ? s.neighbor_range / 2 : 0;
  return p;
}

long long vfs_attn_bwd_workspace_floats(const AttnShape& s, bool need_q, bool need_k) {
  const long long HW = (long long)s.H * s.W, THW = HW * s.T;
  long long n = (long long)s.N * s.topk * HW;                       // ds
  if (s.normalize && need_q) n += (long long)s.N * s.C * HW;        // dq^
  if (s.normalize && need_k) n += (long long)s.N * s.C * THW;       // dk^
  return n;
}

int vfs_attn_fwd_launch(const AttnShape& s, const float* q, const float* k, const float* v, float* out, int* idx, float* w, float* invq,
                        float* invk, hipStream_t st) {
  const int HW = s.H * s.W, THW = s.T * HW;
  int rc;
  if (s.normalize) {
    if ((rc = vfs_simloss_colnorm_launch(q, invq, s.N, s.C, HW, st))) return rc;
    if ((rc = vfs_simloss_colnorm_launch(k, invk, s.N, s.C, THW, st))) return rc;
  }
  AttnArgs p = attn_args(s);
  p.q = q; p.k = k; p.v = v; p.out = out; p.idxout = idx; p.wout = w;
  p.invq = s.normalize ? invq : nullptr;
  p.invk = s.normalize ? invk : nullptr;
  hipLaunchKernelGGL(attn_fwd_kernel, dim3((HW + AT_QT - 1) / AT_QT, s.N), dim3(256), 0, st, p);
  return vfs_check_launch("masked_attention_fwd");
}

int vfs_attn_bwd_launch(const AttnShape& s, const float* q, const float* k, const float* v, const float* dout, const int* idx, const float* w,
                        const float* invq, const float* invk, float* dq, float* dk, float* dv, float* ws, hipStream_t st) {
  const int HW = s.H * s.W, THW = s.T * HW;
  int rc;
  AttnArgs p = attn_args(s);
  p.q = q; p.k = k; p.v = v; p.dout = dout; p.idx = idx; p.w = w;
  p.invq = s.normalize ? invq : nullptr;
  p.invk = s.normalize ? invk : nullptr;
  float* ds = ws;
  float* gq = ds + (size_t)s.N * s.topk * HW;
  float* gk = gq + ((s.normalize && dq) ? (size_t)s.N * s.C * HW : 0);
  const int cblocks = (s.C + 4 * AT_CB - 1) / (4 * AT_CB);
  if (dq || dk) {
    p.dsout = ds;
    hipLaunchKernelGGL(attn_ds_kernel, dim3((HW + 255) / 256, s.N), dim3(256), 0, st, p);
    if ((rc = vfs_check_launch("masked_attention_bwd: score gradients"))) return rc;
    p.ds = ds;
  }
  if (dq) {
    p.dst = s.normalize ? gq : dq;
    hipLaunchKernelGGL(attn_dq_kernel, dim3((HW + AT_QT - 1) / AT_QT, cblocks, s.N), dim3(256), 0, st, p);
    if ((rc = vfs_check_launch("masked_attention_bwd: dq"))) return rc;
    if (s.normalize && (rc = vfs_simloss_norm_bwd_launch(q, invq, gq, dq, s.N, s.C, HW, st))) return rc;
  }
  if (dk) {
    hipLaunchKernelGGL(attn_inv_kernel, dim3((THW + AT_QT - 1) / AT_QT, cblocks, s.N), dim3(256), 0, st, (const float*)ds, q,
                       p.invq, s.normalize ? gk : dk, idx, s.C, s.T, s.H, s.W, p.rad, s.topk);
    if ((rc = vfs_check_launch("masked_attention_bwd: dk"))) return rc;
    if (s.normalize && (rc = vfs_simloss_norm_bwd_launch(k, invk, gk, dk, s.N, s.C, THW, st))) return rc;
  }
  if (dv) {
    hipLaunchKernelGGL(attn_inv_kernel, dim3((THW + AT_QT - 1) / AT_QT, (s.CO + 4 * AT_CB - 1) / (4 * AT_CB), s.N), dim3(256), 0, st, w, dout,
                       (const float*)nullptr, dv, idx, s.CO, s.T, s.H, s.W, p.rad, s.topk);
    if ((rc = vfs_check_launch("masked_attention_bwd: dv"))) return rc;
  }
  return VFS_OK;
}
