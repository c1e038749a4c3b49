// Host side of the batched SiamFC tracking entry points (vfs_siamfc_batch_crops / _upsample / _peak, csrc/siamfc_track.hip): the
// argument checks, the grid arithmetic, and the float64 crop geometry that the crop kernel evaluates per slot (the same function
// compiles for the device).  Plain C++ without any HIP, so that a stand-alone host program (tools/siamfc_batch_check.cpp) can run
// it under the sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(VFS_EMU)
#define VFS_SIAMFC_HD __host__ __device__
#else
#define VFS_SIAMFC_HD
#endif

#define VFS_SIAMFC_MAX_SCALES 8
#define VFS_SIAMFC_MAX_RESP 1024      // r * r floats of one response map in LDS
#define VFS_SIAMFC_MAX_SLOTS 64
#define VFS_SIAMFC_MAX_SIZE 4096      // out_size, up
#define VFS_SIAMFC_STATE_WORDS 8      // fp64 per slot: center_y, center_x, target_h, target_w, z_sz, x_sz, 0, 0
#define VFS_SIAMFC_META_WORDS 8       // int32 per slot: active, H, W, fill_r, fill_g, fill_b, row, status
#define VFS_SIAMFC_STATE_LIMIT 1073741824.0      // 2^30: a centre or size at or above it (or not finite) is never converted to int
#define VFS_SIAMFC_MAX_FRAME_SIDE 32768          // H, W of a slot's frame: H * W * 3 stays far below 2^63, every index below 2^31
// status bits (meta[7]): the kernels only ever OR into the word
#define VFS_SIAMFC_STATUS_STATE 1         // crops: centre / size not finite or >= 2^30 in magnitude, or the frame size outside 1..32768
#define VFS_SIAMFC_STATUS_GEOMETRY 2      // crops: a computed rectangle left its array (the host launcher's two refusals)
#define VFS_SIAMFC_STATUS_ROWS 4          // peak: meta.row outside [0, rows_cap): the frame's box had no row to go to

struct SiamCropScale {
  int valid;           // 0: the crop is all zeros (empty in-image patch, negative pad)
  int px0, py0;        // origin of the in-image patch in the frame
  int iw, ih;          // its size
  int ow, oh;          // its size after the resize
  int padx, pady;      // where it lands in the crop; the rest is `fill`
  int fill[3];
  double sx, sy;       // iw / ow, ih / oh (float64 division, as the host's)
};

// The two rectangle conditions of vfs_siamfc_crops_launch: every source read inside the frame, every patch pixel inside the crop.
VFS_SIAMFC_HD static inline bool vfs_siamfc_source_inside(const SiamCropScale& c, int H, int W) {
  return c.iw >= 1 && c.ih >= 1 && c.px0 >= 0 && c.py0 >= 0 && c.px0 <= W - c.iw && c.py0 <= H - c.ih;
}
VFS_SIAMFC_HD static inline bool vfs_siamfc_target_inside(const SiamCropScale& c, int out_size) {
  return c.ow >= 1 && c.oh >= 1 && c.padx >= 0 && c.pady >= 0 && c.padx <= out_size - c.ow && c.pady <= out_size - c.oh;
}

// crop_params of vfs_amd/siamfc.py (the geometry of crop_and_resize) for a frame [H][W], a centre (yc, xc) and a box `size`, in
// the host's types: every quotient float64 of two integers, np.round / np.rint = rint (half to even), the pad truncated toward
// zero by the assignment to an int array.  -> status bits (0: c is filled in, c.valid says whether the crop is zeros).
// Nothing is converted to an integer before it is known to be finite and below 2^30; a computed rectangle that leaves its array
// (it cannot, from a checked state) clears c.valid and reports VFS_SIAMFC_STATUS_GEOMETRY.
VFS_SIAMFC_HD static inline int vfs_siamfc_crop_geometry(int H, int W, double yc, double xc, double size, int out_size, SiamCropScale& c) {
  c.valid = 0;
  c.px0 = c.py0 = c.iw = c.ih = c.ow = c.oh = c.padx = c.pady = 0;
  c.sx = c.sy = 1.0;
  if (H < 1 || W < 1 || H > VFS_SIAMFC_MAX_FRAME_SIDE || W > VFS_SIAMFC_MAX_FRAME_SIDE) return VFS_SIAMFC_STATUS_STATE;
  if (!(fabs(yc) < VFS_SIAMFC_STATE_LIMIT) || !(fabs(xc) < VFS_SIAMFC_STATE_LIMIT) || !(fabs(size) < VFS_SIAMFC_STATE_LIMIT))
    return VFS_SIAMFC_STATUS_STATE;      // NaN fails every comparison
  if (!(size > 2.0)) size = 2.0;         // max(2, size)
  const double half = size / 2;
  const long long x0 = (long long)rint(xc - half), y0 = (long long)rint(yc - half);
  const long long x1 = (long long)rint(xc + half), y1 = (long long)rint(yc + half);
  const long long bw = x1 - x0, bh = y1 - y0;
  if (bw < 1 || bh < 1) return VFS_SIAMFC_STATUS_GEOMETRY;      // size >= 2: cannot happen
  // img[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)].  A stop <= 0 never yields a crop: 0 is an empty slice, and a negative
  // stop (which numpy counts from the end) comes with a pad beyond out_size, which crop_and_resize answers with zeros.
  if (x1 <= 0 || y1 <= 0) return 0;
  const long long cx0 = x0 > 0 ? x0 : 0, cy0 = y0 > 0 ? y0 : 0;
  const long long cx1 = x1 < W ? x1 : W, cy1 = y1 < H ? y1 : H;
  if (cx0 >= cx1 || cy0 >= cy1) return 0;      // empty patch
  const long long iw = cx1 - cx0, ih = cy1 - cy0;
  const long long ow_r = (long long)rint((double)((long long)out_size * iw) / (double)bw);
  const long long oh_r = (long long)rint((double)((long long)out_size * ih) / (double)bh);
  const long long ow = ow_r > 1 ? ow_r : 1, oh = oh_r > 1 ? oh_r : 1;
  double px = (double)(-x0 * (long long)out_size) / (double)bw, py = (double)(-y0 * (long long)out_size) / (double)bh;
  if (!(px > 0.0)) px = 0.0;      // np.maximum(0, .)
  if (!(py > 0.0)) py = 0.0;
  const long long padx = (long long)px, pady = (long long)py;      // |x0| < 2^31, out_size <= 4096, bw >= 1: below 2^43
  if (out_size - (padx + ow) < 0 || out_size - (pady + oh) < 0) return 0;      // negative pad: zeros
  c.px0 = (int)cx0; c.py0 = (int)cy0; c.iw = (int)iw; c.ih = (int)ih;
  c.ow = (int)ow; c.oh = (int)oh; c.padx = (int)padx; c.pady = (int)pady;
  if (!vfs_siamfc_source_inside(c, H, W) || !vfs_siamfc_target_inside(c, out_size)) return VFS_SIAMFC_STATUS_GEOMETRY;
  c.sx = (double)c.iw / (double)c.ow;
  c.sy = (double)c.ih / (double)c.oh;
  c.valid = 1;
  return 0;
}

// ---- argument checks: nullptr when the call may launch, else what is wrong; *shape = 1 for a size, 0 for a pointer / alignment ----
struct SiamBatchGrid {
  unsigned x, y, z, threads;
};

static inline const char* vfs_siamfc_batch_dims_check(int N, int S, int* shape) {
  *shape = 1;
  if (N < 1 || N > VFS_SIAMFC_MAX_SLOTS) return "1 <= N <= 64";
  if (S < 1 || S > VFS_SIAMFC_MAX_SCALES) return "1 <= S <= 8";
  return nullptr;
}

static inline const char* vfs_siamfc_batch_crops_check(const void* frames, const void* frame_off, const void* state, const void* meta,
                                                       const void* factors, const void* out, int N, int S, int out_size, int use_z,
                                                       int* shape, SiamBatchGrid* grid) {
  *shape = 0;
  if (!frames || !frame_off || !state || !meta || !factors || !out) return "null buffer";
  if (((size_t)frame_off | (size_t)state | (size_t)factors) & 7) return "frame_off, state and factors must be 8-byte aligned";
  if ((size_t)meta & 3) return "meta must be 4-byte aligned";
  if (const char* e = vfs_siamfc_batch_dims_check(N, S, shape)) return e;
  if (out_size < 1 || out_size > VFS_SIAMFC_MAX_SIZE) return "1 <= out_size <= 4096";
  if (use_z != 0 && use_z != 1) return "use_z is 0 or 1";
  if (use_z && S != 1) return "use_z needs S == 1";
  grid->x = (unsigned)((out_size * out_size + 255) / 256);
  grid->y = (unsigned)S;
  grid->z = (unsigned)N;
  grid->threads = 256;
  return nullptr;
}

static inline const char* vfs_siamfc_batch_upsample_check(const void* responses, const void* tap_idx, const void* tap_w, const void* penalty,
                                                          const void* up_out, const void* scale_max, int N, int S, int r, int up, int* shape,
                                                          SiamBatchGrid* grid) {
  *shape = 0;
  if (!responses || !tap_idx || !tap_w || !penalty || !up_out || !scale_max) return "null buffer";
  if (((size_t)tap_idx | (size_t)tap_w) & 15) return "the tap tables must be 16-byte aligned";
  if ((size_t)scale_max & 7) return "scale_max must be 8-byte aligned";
  if (const char* e = vfs_siamfc_batch_dims_check(N, S, shape)) return e;
  if (r < 1 || r > VFS_SIAMFC_MAX_RESP || r * r > VFS_SIAMFC_MAX_RESP) return "r * r <= 1024";
  if (up < 1 || up > VFS_SIAMFC_MAX_SIZE) return "1 <= up <= 4096";
  grid->x = (unsigned)((up * up + 255) / 256);
  grid->y = (unsigned)S;
  grid->z = (unsigned)N;
  grid->threads = 256;
  return nullptr;
}

static inline const char* vfs_siamfc_batch_peak_check(const void* up_in, const void* scale_max, const void* hann, const void* factors,
                                                      const void* state, const void* meta, const void* boxes, const void* records,
                                                      long long rows_cap, int N, int S, int up, int* shape, SiamBatchGrid* grid) {
  *shape = 0;
  if (!up_in || !scale_max || !hann || !factors || !state || !meta || !boxes || !records) return "null buffer";
  if (((size_t)scale_max | (size_t)hann | (size_t)factors | (size_t)state | (size_t)boxes) & 7)
    return "scale_max, hann, factors, state and boxes must be 8-byte aligned";
  if ((size_t)meta & 3) return "meta must be 4-byte aligned";
  if ((size_t)records & 15) return "records must be 16-byte aligned";
  if (const char* e = vfs_siamfc_batch_dims_check(N, S, shape)) return e;
  if (up < 1 || up > VFS_SIAMFC_MAX_SIZE) return "1 <= up <= 4096";
  if (rows_cap < 1 || rows_cap > 0x7fffffffLL) return "1 <= rows_cap < 2^31";
  grid->x = (unsigned)N;
  grid->y = grid->z = 1;
  grid->threads = 1024;
  return nullptr;
}
