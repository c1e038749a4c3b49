// Table-driven ingest of the label propagation's feature bank for gfx950: the feature maps of n images, as the backbone leaves
// them, enter n positions of a bank in ONE launch.
//
// For query frame f the reference reads frame 0 and frames max(0, f - precede_frames) .. f - 1 only (mmaction/models/trackers/
// vanilla_tracker.py:132-149), so a bank needs precede_frames + 2 positions per video, reused as a ring (vfs_amd/labelprop.py), and
// a frame can enter it when it arrives.  With one new frame per video and step - a stream, or every slot of a lock-step batch - the
// contiguous kernels (vfs_l2norm_rows_f32 + vfs_split_rows_bf16x2, vfs_l2norm_rows) would be launched per video, and the split would
// read every unit row back.  Here the grid carries the image (blockIdx.y), a small device table says where each image goes, and one
// wave handles one row: the row is read ONCE into registers (16 bytes per lane and load), normalised, written to the bank and - fp32
// two-pass banks - split into its hi / lo copy from the same registers.
//
// The arithmetic and the ownership of a row are vfs_rows.h's, shared with the contiguous kernels: same bits.  The split is laid out
// in 8-channel groups while a lane owns float4 groups, so neighbouring lanes exchange their groups (lane ^ 1, a DPP move) and the
// even lane writes the hi half, the odd lane the lo half of the pair's 8 channels: 16 bytes per lane, 64 contiguous bytes per
// four lanes.
#include "vfs_ops.h"
#include "vfs_rows.h"

__device__ __forceinline__ f32x4 ingest_ldf4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void ingest_stf4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// first destination rows of this workgroup's image, false: they do not lie inside the banks (nothing of the image is written)
__device__ __forceinline__ bool ingest_rows(const BankIngestArgs& a, long long* frow, long long* hrow) {
  const long long* t = a.table + 2 * (size_t)blockIdx.y;
  *frow = t[0];
  *hrow = t[1];
  const long long last = a.bank_rows - a.P;
  return *frow >= 0 && *frow <= last && (!a.hl || (*hrow >= 0 && *hrow <= last));
}

// NG float4 groups per lane: C <= 256 NG
template <int NG>
__global__ __launch_bounds__(256) void bank_ingest_f32_kernel(BankIngestArgs a) {
  const int lane = threadIdx.x & 63, C = a.C;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  long long frow, hrow;
  if (row >= a.P || !ingest_rows(a, &frow, &hrow)) return;      // (whole waves leave: the exchanges below are wave-wide)
  const float* src = (const float*)a.x + ((size_t)blockIdx.y * a.P + row) * C;
  f32x4 v[NG];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int g = lane + 64 * i;
    v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (g * 4 < C) {
      v[i] = ingest_ldf4(src + g * 4);
      ss = rows_f32_sumsq(v[i], ss);
    }
  }
  if (a.unit) {
    const float nrm = rows_f32_norm(rows_wave_sum(ss));
#pragma unroll
    for (int i = 0; i < NG; ++i) v[i] = rows_f32_unit(v[i], nrm);
  }
  float* dst = (float*)a.fbank + (size_t)(frow + row) * C;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int g = lane + 64 * i;
    if (g * 4 < C) ingest_stf4(dst + g * 4, v[i]);
  }
  if (!a.hl) return;
  bf16_t* hl = a.hl + (size_t)(hrow + row) * 2 * C;
  const bool odd = lane & 1;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int g = lane + 64 * i;      // C % 16 == 0: groups g and g ^ 1 are inside the row together
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = dpp_mov<0xB1>(v[i][e]);      // quad_perm [1,0,3,2]: lane ^ 1, on the vector ALU
    const f32x4 c0 = odd ? o : v[i], c1 = odd ? v[i] : o;
    const float w[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    const u32x4 half = odd ? rows_split_lo(w) : rows_split_hi(w);
    if (g * 4 < C) st16(hl + rows_split_at(g >> 1) + (odd ? 16 : 0), half);
  }
}

// NG 8-channel groups per lane: C <= 512 NG
template <int NG>
__global__ __launch_bounds__(256) void bank_ingest_bf16_kernel(BankIngestArgs a) {
  const int lane = threadIdx.x & 63, C = a.C;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  long long frow, hrow;
  if (row >= a.P || !ingest_rows(a, &frow, &hrow)) return;
  const bf16_t* src = (const bf16_t*)a.x + ((size_t)blockIdx.y * a.P + row) * C;
  u32x4 v[NG];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int c = lane * 8 + 512 * i;
    v[i] = zero16();
    if (c < C) {
      v[i] = ld16(src + c);
      ss = rows_bf16_sumsq(v[i], ss);
    }
  }
  if (a.unit) {
    const float inv = rows_bf16_inv(rows_wave_sum(ss));
#pragma unroll
    for (int i = 0; i < NG; ++i) v[i] = rows_bf16_unit(v[i], inv);
  }
  bf16_t* dst = (bf16_t*)a.fbank + (size_t)(frow + row) * C;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int c = lane * 8 + 512 * i;
    if (c < C) st16(dst + c, v[i]);
  }
}

static dim3 ingest_grid(const BankIngestArgs& a) { return dim3((unsigned)((a.P + 3) / 4), (unsigned)a.n); }

int vfs_bank_ingest_f32_launch(const BankIngestArgs& a, hipStream_t s) {
  if (a.C % 4 || a.C > BANK_INGEST_MAX_C) return vfs_set_error(VFS_ERR_SHAPE, "bank_ingest_f32: C % 4, C <= 2048");
  if (a.hl && a.C % 16) return vfs_set_error(VFS_ERR_SHAPE, "bank_ingest_f32: C % 16 for the split copy");
  if (a.C <= 256) hipLaunchKernelGGL(bank_ingest_f32_kernel<1>, ingest_grid(a), dim3(256), 0, s, a);
  else if (a.C <= 512) hipLaunchKernelGGL(bank_ingest_f32_kernel<2>, ingest_grid(a), dim3(256), 0, s, a);
  else if (a.C <= 1024) hipLaunchKernelGGL(bank_ingest_f32_kernel<4>, ingest_grid(a), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(bank_ingest_f32_kernel<8>, ingest_grid(a), dim3(256), 0, s, a);
  return vfs_check_launch("bank_ingest_f32");
}

int vfs_bank_ingest_bf16_launch(const BankIngestArgs& a, hipStream_t s) {
  if (a.C % 8 || a.C > BANK_INGEST_MAX_C) return vfs_set_error(VFS_ERR_SHAPE, "bank_ingest_bf16: C % 8, C <= 2048");
  if (a.C <= 512) hipLaunchKernelGGL(bank_ingest_bf16_kernel<1>, ingest_grid(a), dim3(256), 0, s, a);
  else if (a.C <= 1024) hipLaunchKernelGGL(bank_ingest_bf16_kernel<2>, ingest_grid(a), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(bank_ingest_bf16_kernel<4>, ingest_grid(a), dim3(256), 0, s, a);
  return vfs_check_launch("bank_ingest_bf16");
}
