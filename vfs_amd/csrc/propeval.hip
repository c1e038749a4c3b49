// Output side of the label-propagation evaluation on JHMDB (pose, PCK) and VIP (human parts, mIoU):
// the three device passes around VanillaTracker.forward_test that are not DAVIS.
//
// Reference call sites:
//   vfs_heatmap_topk   JHMDBDataset.img2coord (datasets/jhmdb_dataset.py:118-136): np.argsort over every
//                      full-resolution key-point map, of which only the last `topk` entries are used
//   vfs_label_counts   intersect_and_union (core/evaluation/iou.py:5-63): three np.histogram calls per frame
//   vfs_pose_heatmaps  RawFrameDecode's pose_coord branch + draw_label_map (pipelines/loading.py:1055-1101)
// tests/prop_eval_oracle.py restates the three contracts in numpy; the kernels are tested bit for bit against it.
//
// All three are streaming passes (one read or one write of every element), no MFMA.
#include <math.h>

#include "vfs_common.h"
#include "vfs_ops.h"

// ---------------------------------------------------------------------------------------------------------
// top-k of every map.  Order: larger value ranks higher, among equal values the LOWER flat index ranks higher
// (np.argsort leaves ties open; this is the project's rule).  -0.0 == 0.0 as in every float comparison.
#define TOPK_THREADS 256
#define TOPK_WAVES (TOPK_THREADS / VFS_WAVE)
#define TOPK_NONE 0x7fffffff      // index of an empty slot: ranks below every real element of the same value

__device__ __forceinline__ bool topk_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// (value, index) arg-max over the 64 lanes of a wave, result in every lane
__device__ __forceinline__ void topk_wave_best(float& v, int& i) {
#pragma unroll
  for (int m = 1; m < VFS_WAVE; m <<= 1) {
    const float ov = __shfl_xor(v, m);
    const int oi = __shfl_xor(i, m);
    if (topk_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

template <int K>
struct TopkList {      // sorted, v[0] ranks highest; fully unrolled, lives in registers
  float v[K];
  int i[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) { v[j] = -INFINITY; i[j] = TOPK_NONE; }
  }
  // elements arrive in ascending index order, so an equal value never displaces a held one: one strict compare
  // against the current smallest is the whole fast path
  __device__ __forceinline__ void push(float x, int idx) {
    if (x > v[K - 1]) {
      v[K - 1] = x; i[K - 1] = idx;
#pragma unroll
      for (int j = K - 1; j > 0; --j) {
        if (v[j] > v[j - 1]) {
          const float tv = v[j]; v[j] = v[j - 1]; v[j - 1] = tv;
          const int ti = i[j]; i[j] = i[j - 1]; i[j - 1] = ti;
        }
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
    v[K - 1] = -INFINITY; i[K - 1] = TOPK_NONE;
  }
};

struct TopkLaneState {
  float mn;
  unsigned nonzero, nan;
};

template <int K>
__device__ __forceinline__ void topk_take(TopkList<K>& L, TopkLaneState& s, float x, int idx) {
  L.push(x, idx);
  s.mn = fminf(s.mn, x);
  s.nonzero |= (x != 0.f) ? 1u : 0u;      // true for a NaN as well
  s.nan |= (x != x) ? 1u : 0u;
}

template <int K>
__global__ __launch_bounds__(TOPK_THREADS) void heatmap_topk_kernel(HeatmapTopkArgs a) {
  __shared__ float s_v[TOPK_WAVES * K];
  __shared__ int s_i[TOPK_WAVES * K];
  __shared__ float s_mn[TOPK_WAVES];
  __shared__ unsigned s_fl[TOPK_WAVES];
  const int t = threadIdx.x, lane = t & (VFS_WAVE - 1), wave = t / VFS_WAVE;
  const long long map = blockIdx.x;
  const int HW = a.HW;
  const float* M = a.maps + map * HW;

  TopkList<K> L;
  L.clear();
  TopkLaneState st = {INFINITY, 0u, 0u};

  // scalar head up to the first 16-byte boundary (lowest indices: thread 0..2 see them before anything else)
  int head = (int)(((16u - (unsigned)((uintptr_t)M & 15u)) & 15u) >> 2);
  if (head > HW) head = HW;
  if (t < head) topk_take<K>(L, st, M[t], t);
  // 16-byte body, four independent loads in flight per lane; a lane's indices only grow
  const int nvec = (HW - head) >> 2;
  // (buffer loads: the compiler cannot split them into dwords; every step of both loops is in range, q < nvec)
  const __amdgpu_buffer_rsrc_t V = __builtin_amdgcn_make_buffer_rsrc((void*)(M + head), 0, (unsigned)nvec * 16u, 0x00020000);
  int q = t;
  for (; q + 3 * TOPK_THREADS < nvec; q += 4 * TOPK_THREADS) {
    u32x4 w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = __builtin_amdgcn_raw_buffer_load_b128(V, (unsigned)(q + u * TOPK_THREADS) * 16u, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int base = head + 4 * (q + u * TOPK_THREADS);
      const f32x4 f = __builtin_bit_cast(f32x4, w[u]);
      topk_take<K>(L, st, f[0], base);
      topk_take<K>(L, st, f[1], base + 1);
      topk_take<K>(L, st, f[2], base + 2);
      topk_take<K>(L, st, f[3], base + 3);
    }
  }
  for (; q < nvec; q += TOPK_THREADS) {
    const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(V, (unsigned)q * 16u, 0, 0));
    const int base = head + 4 * q;
    topk_take<K>(L, st, f[0], base);
    topk_take<K>(L, st, f[1], base + 1);
    topk_take<K>(L, st, f[2], base + 2);
    topk_take<K>(L, st, f[3], base + 3);
  }
  // scalar tail (highest indices: after everything else a thread has seen)
  const int tail0 = head + 4 * nvec;
  if (tail0 + t < HW) topk_take<K>(L, st, M[tail0 + t], tail0 + t);

  // inside the wave: K rounds of arg-max over the lanes' current best; the owner drops it
#pragma unroll
  for (int r = 0; r < K; ++r) {
    float bv = L.v[0];
    int bi = L.i[0];
    topk_wave_best(bv, bi);
    if (bi == L.i[0] && bi != TOPK_NONE) L.pop();
    if (lane == 0) { s_v[wave * K + r] = bv; s_i[wave * K + r] = bi; }
  }
  float mn = st.mn;
  unsigned fl = st.nonzero | (st.nan << 1);
#pragma unroll
  for (int m = 1; m < VFS_WAVE; m <<= 1) {
    mn = fminf(mn, __shfl_xor(mn, m));
    fl |= __shfl_xor(fl, m);
  }
  if (lane == 0) { s_mn[wave] = mn; s_fl[wave] = fl; }
  __syncthreads();
  if (wave != 0) return;

  // across the waves: the TOPK_WAVES * K candidates, one per lane of wave 0
  float cv = -INFINITY;
  int ci = TOPK_NONE;
  if (lane < TOPK_WAVES * K) { cv = s_v[lane]; ci = s_i[lane]; }
#pragma unroll
  for (int r = 0; r < K; ++r) {
    float bv = cv;
    int bi = ci;
    topk_wave_best(bv, bi);
    if (bi == ci) { cv = -INFINITY; ci = TOPK_NONE; }
    if (lane == 0) {      // ascending value order, as argsort(...)[-topk:]
      a.vals[map * K + (K - 1 - r)] = bv;
      a.idx[map * K + (K - 1 - r)] = bi;
    }
  }
  if (lane == 0) {
    float m2 = s_mn[0];
    unsigned f2 = s_fl[0];
#pragma unroll
    for (int w = 1; w < TOPK_WAVES; ++w) { m2 = fminf(m2, s_mn[w]); f2 |= s_fl[w]; }
    a.minv[map] = m2;
    // an element equal to -inf never enters a list (the empty slots hold -inf and admission is a strict compare): flagged
    a.flags[map] = (int)(((f2 & 1u) ? 0u : VFS_TOPK_ALL_ZERO) | ((f2 & 2u) ? VFS_TOPK_NAN : 0u) |
                         (m2 == -INFINITY ? VFS_TOPK_NEG_INF : 0u));
  }
}

template <int K>
static void topk_launch_k(const HeatmapTopkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(heatmap_topk_kernel<K>, dim3((unsigned)a.N), dim3(TOPK_THREADS), 0, s, a);
}

int vfs_heatmap_topk_launch(const HeatmapTopkArgs& a, hipStream_t s) {
  if (a.topk < 1 || a.topk > 8) return vfs_set_error(VFS_ERR_SHAPE, "heatmap_topk: topk 1..8");
  if (a.N < 0 || a.N > 0x7fffffffLL) return vfs_set_error(VFS_ERR_SHAPE, "heatmap_topk: 0..2^31-1 maps");
  if (a.HW < a.topk) return vfs_set_error(VFS_ERR_SHAPE, "heatmap_topk: a map has fewer than topk elements");
  if (a.HW > (1 << 28)) return vfs_set_error(VFS_ERR_SHAPE, "heatmap_topk: H*W <= 2^28");
  if (a.N == 0) return VFS_OK;
  switch (a.topk) {
    case 1: topk_launch_k<1>(a, s); break;
    case 2: topk_launch_k<2>(a, s); break;
    case 3: topk_launch_k<3>(a, s); break;
    case 4: topk_launch_k<4>(a, s); break;
    case 5: topk_launch_k<5>(a, s); break;
    case 6: topk_launch_k<6>(a, s); break;
    case 7: topk_launch_k<7>(a, s); break;
    default: topk_launch_k<8>(a, s); break;
  }
  return vfs_check_launch("heatmap_topk");
}

// ---------------------------------------------------------------------------------------------------------
// np.histogram(x, bins=np.arange(num_classes + 1)): the last bin is closed, so the value num_classes lands in
// class num_classes - 1; larger values are dropped.  -1 = dropped.
__device__ __forceinline__ int label_class(unsigned v, int nc) {
  return v < (unsigned)nc ? (int)v : (v == (unsigned)nc ? nc - 1 : -1);
}

#define LC_THREADS 256

struct LabelRun {      // run of identical (pred, gt) pairs seen by one thread: neighbouring pixels mostly agree
  unsigned key, len;
};

__device__ __forceinline__ void label_flush(const LabelRun& r, unsigned (*hist)[3], int nc, int ignore) {
  if (!r.len) return;
  const unsigned p = r.key & 0xffu, g = r.key >> 8;
  if ((int)g == ignore) return;
  const int pc = label_class(p, nc), gc = label_class(g, nc);
  if (pc >= 0) atomicAdd(&hist[pc][1], r.len);
  if (gc >= 0) atomicAdd(&hist[gc][2], r.len);
  if (p == g && pc >= 0) atomicAdd(&hist[pc][0], r.len);
}
__device__ __forceinline__ void label_take(LabelRun& r, unsigned p, unsigned g, unsigned (*hist)[3], int nc, int ignore) {
  const unsigned key = p | (g << 8);
  if (key == r.key) { ++r.len; return; }
  label_flush(r, hist, nc, ignore);
  r.key = key; r.len = 1;
}

__global__ __launch_bounds__(LC_THREADS) void label_counts_kernel(LabelCountsArgs a) {
  __shared__ unsigned hist[256][3];
  const int t = threadIdx.x;
  for (int i = t; i < 3 * a.num_classes; i += LC_THREADS) (&hist[0][0])[i] = 0u;
  __syncthreads();
  LabelRun run = {0u, 0u};
  const long long stride = (long long)gridDim.x * LC_THREADS;
  const long long first = (long long)blockIdx.x * LC_THREADS + t;
  for (long long q = first; q < a.nvec; q += stride) {      // 16 pixels of both maps per step
    const u32x4 pw = ld16(a.pred + 16 * q), gw = ld16(a.gt + 16 * q);
    const unsigned pa[4] = {pw.x, pw.y, pw.z, pw.w}, ga[4] = {gw.x, gw.y, gw.z, gw.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int b = 0; b < 4; ++b) label_take(run, (pa[w] >> (8 * b)) & 0xffu, (ga[w] >> (8 * b)) & 0xffu, hist, a.num_classes, a.ignore_index);
  }
  for (long long i = 16 * a.nvec + first; i < a.n; i += stride)      // tail (everything when a map is not 16-byte aligned)
    label_take(run, a.pred[i], a.gt[i], hist, a.num_classes, a.ignore_index);
  label_flush(run, hist, a.num_classes, a.ignore_index);
  __syncthreads();
  for (int i = t; i < 3 * a.num_classes; i += LC_THREADS) {
    const unsigned c = (&hist[0][0])[i];
    if (c) atomicAdd(&a.counts[i], (unsigned long long)c);
  }
}

int vfs_label_counts_launch(const LabelCountsArgs& a0, hipStream_t s) {
  LabelCountsArgs a = a0;
  if (a.num_classes < 1 || a.num_classes > 256) return vfs_set_error(VFS_ERR_SHAPE, "label_counts: 1..256 classes");
  if (a.ignore_index < -1 || a.ignore_index > 255) return vfs_set_error(VFS_ERR_SHAPE, "label_counts: ignore_index 0..255 or -1");
  if (a.n < 0 || a.n > (1LL << 40)) return vfs_set_error(VFS_ERR_SHAPE, "label_counts: 0..2^40 pixels");
  if (a.n == 0) return VFS_OK;
  const bool aligned = (((uintptr_t)a.pred | (uintptr_t)a.gt) & 15u) == 0;
  a.nvec = aligned ? a.n / 16 : 0;
  // Two workgroups per CU at most: every workgroup ends with up to 3 * num_classes 64-bit atomics on the SAME few addresses,
  // which serialise at the L2 (8 frames of 720 x 1280: 0.043 ms with one 16-pixel step per lane, 0.022 ms so).  A workgroup
  // counts in 32-bit LDS words: at most 2^40 / 512 = 2^31 pixels each.
  const long long work = a.nvec + (a.n - 16 * a.nvec);
  long long bx = (work + LC_THREADS - 1) / LC_THREADS;
  if (bx > 512) bx = 512;
  hipLaunchKernelGGL(label_counts_kernel, dim3((unsigned)bx), dim3(LC_THREADS), 0, s, a);
  return vfs_check_launch("label_counts");
}

// ---------------------------------------------------------------------------------------------------------
// key-point heat maps: out[k] = 0 everywhere, the host-computed Gaussian patch pasted with its upper-left corner at
// ul (draw_label_map's slices: image rows max(0, ul_y) .. min(br_y, H), patch row = image row - ul_y).
__global__ __launch_bounds__(256) void pose_heatmaps_kernel(PoseHeatmapArgs a) {
  const int k = blockIdx.y;
  const int* kp = a.kp + 5 * k;
  const int ulx = kp[0], uly = kp[1], inside = kp[4];
  const int x1 = min(kp[2], a.W), y1 = min(kp[3], a.H);
  float* O = a.out + (size_t)k * a.H * a.W;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.H * a.W; i += gridDim.x * 256) {
    const int y = i / a.W, x = i - y * a.W;
    float v = 0.f;
    if (inside && x >= ulx && x < x1 && y >= uly && y < y1) {
      const int gx = x - ulx, gy = y - uly;      // x >= ulx: never negative
      if (gx < a.P && gy < a.P) v = a.patch[gy * a.P + gx];
    }
    O[i] = v;
  }
}

int vfs_pose_heatmaps_launch(const PoseHeatmapArgs& a, hipStream_t s) {
  if (a.K < 0 || a.K > 65535) return vfs_set_error(VFS_ERR_SHAPE, "pose_heatmaps: 0..65535 key points");
  if (a.H < 1 || a.W < 1 || (long long)a.H * a.W > (1LL << 30)) return vfs_set_error(VFS_ERR_SHAPE, "pose_heatmaps: 1 <= H*W <= 2^30");
  if (a.P < 1 || a.P > 1024) return vfs_set_error(VFS_ERR_SHAPE, "pose_heatmaps: patch side 1..1024");
  if (a.K == 0) return VFS_OK;
  int bx = (a.H * a.W + 255) / 256;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(pose_heatmaps_kernel, dim3(bx, a.K), dim3(256), 0, s, a);
  return vfs_check_launch("pose_heatmaps");
}
