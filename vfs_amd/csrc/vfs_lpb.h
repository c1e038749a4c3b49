// Descriptor rows of the batched (lock-step) label propagation: what a workgroup of slot blockIdx.z reads before it runs the
// single-video kernel body on its slot (LpBatchArgs: vfs_ops.h; row layout: include/vfs_hip.h).
#pragma once
#include "vfs_ops.h"

struct LpbRow {
  int qframe, nkeys, non_mask_len, CO;
  const int* kslot;      // the row's key list, left in the table
};
// the row of `slot`; false: the slot sits this step out (inactive, or a row outside the ranges the host entry point checks for a
// single video - it must not index the banks).  Every wave decides for itself from one load of the key list: no barrier.
__device__ __forceinline__ bool lpb_row(const int* __restrict__ desc, int slot, int Tcap, int max_nkeys, int COcap, int radius, LpbRow& r) {
  const int* row = desc + (size_t)slot * LPB_DESC_INTS;
  if (row[0] == 0) return false;
  r.qframe = row[1]; r.nkeys = row[2]; r.non_mask_len = row[3]; r.CO = row[4];
  r.kslot = row + 8;
  if (r.qframe < 0 || r.qframe >= Tcap || r.nkeys < 1 || r.nkeys > max_nkeys || r.nkeys > LP_MAX_KEYS || r.CO < 1 || r.CO > COcap) return false;
  if (r.non_mask_len < 0 || r.non_mask_len >= r.nkeys + (radius <= 0 ? 1 : 0)) return false;
  const int lane = threadIdx.x & 63;
  const bool bad = lane < r.nkeys && (unsigned)r.kslot[lane] >= (unsigned)Tcap;
  return !__any(bad);
}
// post-processing: the slot's propagated frame (a position of its label rows), the position of its maps that the step writes and its
// class count.  The map position is column [5], which lpb_row above does not read.
__device__ __forceinline__ bool lpb_row_post(const int* __restrict__ desc, int slot, int Tcap, int Tmaps, int COcap, int& qframe, int& mpos, int& CO) {
  const int* row = desc + (size_t)slot * LPB_DESC_INTS;
  if (row[0] == 0) return false;
  qframe = row[1]; CO = row[4]; mpos = row[5];
  return qframe >= 0 && qframe < Tcap && mpos >= 0 && mpos < Tmaps && CO >= 1 && CO <= COcap;
}
// label maps of a step (exact_f32.hip, labelprop.hip): what slot blockIdx.z reads and writes
struct SegPostBatchArgs {
  const float* sbank;      // [nslots][Tcap][H*W][COcap]
  float* partial;          // [nslots][LP_POST_BLOCKS][COcap][2]
  uint8_t* preds;          // [nslots][Tmaps][Ho*Wo]
  const int* desc;
  int Tcap, Tmaps, COcap, H, W, Ho, Wo;
};
__device__ __forceinline__ bool seg_post_slot(const SegPostBatchArgs& b, const float*& seg, float*& partial, uint8_t*& label, int& CO) {
  const int n = blockIdx.z;
  int qframe, mpos;
  if (!lpb_row_post(b.desc, n, b.Tcap, b.Tmaps, b.COcap, qframe, mpos, CO)) return false;
  const size_t HW = (size_t)b.H * b.W;
  seg = b.sbank + (size_t)n * b.Tcap * HW * b.COcap + (size_t)qframe * HW * CO;
  partial = b.partial + (size_t)n * LP_POST_BLOCKS * b.COcap * 2;
  label = b.preds + ((size_t)n * b.Tmaps + mpos) * b.Ho * b.Wo;
  return true;
}
