// Stand-alone host check of the batched SiamFC tracking entry points' host side (vfs_amd/csrc/siamfc_batch.h): the argument
// checks, the grid arithmetic and the float64 crop geometry that the crop kernel evaluates per slot, to be run under the
// sanitizers.  No HIP, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/siamfc_batch_check.cpp -o siamfc_batch_check
//   ./siamfc_batch_check            -> "siamfc_batch_check: ok", exit status 0
// The geometry is walked over states far outside every frame, huge, infinite and NaN: a conversion of an unchecked double to an
// integer, or an integer overflow in the pad arithmetic, is a UBSan report; every rectangle it accepts is then read in a heap
// frame of exactly H * W * 3 bytes and written to a crop of exactly out_size^2 bytes, so a rectangle that leaves its array is an
// ASan report.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../vfs_amd/csrc/siamfc_batch.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static bool refused(const char* got, const char* want) { return got && !std::strcmp(got, want); }

// touch what the kernel touches for geometry c: the four corners of the source patch and of the target rectangle
static void touch(const SiamCropScale& c, int H, int W, int out_size) {
  std::vector<unsigned char> frame((size_t)H * W * 3, 1), crop((size_t)out_size * out_size, 0);
  unsigned sum = 0;
  for (int y : {c.py0, c.py0 + c.ih - 1})
    for (int x : {c.px0, c.px0 + c.iw - 1}) sum += frame[((size_t)y * W + x) * 3 + 2];
  for (int y : {c.pady, c.pady + c.oh - 1})
    for (int x : {c.padx, c.padx + c.ow - 1}) crop[(size_t)y * out_size + x] = 1;
  EXPECT(sum == 4);
}

static void geometry(int H, int W, double yc, double xc, double size, int out_size, int want_status) {
  SiamCropScale c;
  const int status = vfs_siamfc_crop_geometry(H, W, yc, xc, size, out_size, c);
  EXPECT(status == want_status);
  EXPECT(!(status && c.valid));
  if (c.valid) {
    EXPECT(vfs_siamfc_source_inside(c, H, W) && vfs_siamfc_target_inside(c, out_size));
    EXPECT(c.sx == (double)c.iw / c.ow && c.sy == (double)c.ih / c.oh);
    touch(c, H, W, out_size);
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int S = VFS_SIAMFC_STATUS_STATE;
  // a box inside the frame, across borders, outside, larger than the frame, below the minimum size
  geometry(96, 128, 48, 64, 40, 63, 0);
  geometry(72, 80, 5.5, 4.25, 50.3, 31, 0);
  geometry(120, 64, 300, -200, 30, 63, 0);
  geometry(120, 64, 60, 32, 5000, 255, 0);
  geometry(48, 64, 0.2, 0.4, 0.5, 120, 0);
  geometry(1, 1, 0, 0, 2, 1, 0);
  geometry(32768, 32768, 32767, 32767, 3, 4096, 0);
  // the guard: nothing of these is converted to an integer
  geometry(96, 128, nan, 64, 40, 63, S);
  geometry(96, 128, 48, nan, 40, 63, S);
  geometry(96, 128, 48, 64, nan, 63, S);
  geometry(96, 128, inf, 64, 40, 63, S);
  geometry(96, 128, 48, -inf, 40, 63, S);
  geometry(96, 128, 48, 64, 1e300, 63, S);
  geometry(96, 128, 48, 64, VFS_SIAMFC_STATE_LIMIT, 63, S);
  geometry(96, 128, -VFS_SIAMFC_STATE_LIMIT, 64, 40, 63, S);
  geometry(0, 128, 48, 64, 40, 63, S);
  geometry(96, -5, 48, 64, 40, 63, S);
  geometry(96, 1 << 20, 48, 64, 40, 63, S);
  // just inside the guard, at both ends: the pad arithmetic stays within 64 bits, the crop is zeros
  const double edge = std::nextafter(VFS_SIAMFC_STATE_LIMIT, 0.0);
  for (double yc : {-edge, edge})
    for (double xc : {-edge, edge})
      for (double size : {2.0, 1000.0, edge}) geometry(480, 640, yc, xc, size, 4096, 0);
  geometry(480, 640, 240, 320, edge, 4096, 0);      // a one-pixel patch in a 4096 x 4096 crop: the largest pad
  // random states around and far from random frames
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> u(-1.0, 2.0), sz(0.0, 3.0);
  for (int trial = 0; trial < 20000; ++trial) {
    const int H = 1 + (int)(rng() % 300), W = 1 + (int)(rng() % 300), out_size = 1 + (int)(rng() % 255);
    const double mag = (trial % 8 == 0) ? 1e5 : 1.0;      // at most 1.8e8: inside the guard
    geometry(H, W, u(rng) * H * mag, u(rng) * W * mag, sz(rng) * (H + W) * mag, out_size, 0);
  }

  // the argument checks; P: any 16-byte aligned address (never dereferenced by the checks)
  alignas(16) static double P[4];
  const void *U8 = (const char*)P + 8, *U4 = (const char*)P + 4, *U2 = (const char*)P + 2;
  int shape = -1;
  SiamBatchGrid g{};
  EXPECT(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 64, 8, 4096, 0, &shape, &g) == nullptr);
  EXPECT(g.x == 65536 && g.y == 8 && g.z == 64 && g.threads == 256);      // 4096^2 / 256
  EXPECT(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 1, 1, 1, 1, &shape, &g) == nullptr && g.x == 1 && g.y == 1 && g.z == 1);
  EXPECT(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 16, 3, 255, 0, &shape, &g) == nullptr && g.x == 255 && g.y == 3 && g.z == 16);
  EXPECT(vfs_siamfc_batch_crops_check(U2, U8, U8, U4, U8, U4, 16, 3, 255, 0, &shape, &g) == nullptr);
  for (int k = 0; k < 6; ++k) {
    const void* a[6] = {P, P, P, P, P, P};
    a[k] = nullptr;
    EXPECT(refused(vfs_siamfc_batch_crops_check(a[0], a[1], a[2], a[3], a[4], a[5], 2, 3, 31, 0, &shape, &g), "null buffer") && shape == 0);
  }
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, U4, P, P, P, P, 2, 3, 31, 0, &shape, &g), "frame_off, state and factors must be 8-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, U4, P, P, P, 2, 3, 31, 0, &shape, &g), "frame_off, state and factors must be 8-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, U4, P, 2, 3, 31, 0, &shape, &g), "frame_off, state and factors must be 8-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, U2, P, P, 2, 3, 31, 0, &shape, &g), "meta must be 4-byte aligned") && shape == 0);
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 0, 3, 31, 0, &shape, &g), "1 <= N <= 64") && shape == 1);
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 65, 3, 31, 0, &shape, &g), "1 <= N <= 64"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 0, 31, 0, &shape, &g), "1 <= S <= 8"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 9, 31, 0, &shape, &g), "1 <= S <= 8"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 3, 0, 0, &shape, &g), "1 <= out_size <= 4096"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 3, 4097, 0, &shape, &g), "1 <= out_size <= 4096"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 3, 0x7fffffff, 0, &shape, &g), "1 <= out_size <= 4096"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 3, 31, 2, &shape, &g), "use_z is 0 or 1"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 3, 31, -1, &shape, &g), "use_z is 0 or 1"));
  EXPECT(refused(vfs_siamfc_batch_crops_check(P, P, P, P, P, P, 2, 3, 31, 1, &shape, &g), "use_z needs S == 1"));

  EXPECT(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 64, 8, 32, 4096, &shape, &g) == nullptr && g.x == 65536 && g.y == 8 && g.z == 64);
  EXPECT(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 16, 3, 17, 272, &shape, &g) == nullptr && g.x == 289 && g.threads == 256);
  EXPECT(vfs_siamfc_batch_upsample_check(U4, P, P, U4, U4, U8, 16, 3, 17, 272, &shape, &g) == nullptr);
  for (int k = 0; k < 6; ++k) {
    const void* a[6] = {P, P, P, P, P, P};
    a[k] = nullptr;
    EXPECT(refused(vfs_siamfc_batch_upsample_check(a[0], a[1], a[2], a[3], a[4], a[5], 2, 3, 5, 80, &shape, &g), "null buffer"));
  }
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, U8, P, P, P, P, 2, 3, 5, 80, &shape, &g), "the tap tables must be 16-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, U8, P, P, P, 2, 3, 5, 80, &shape, &g), "the tap tables must be 16-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, U4, 2, 3, 5, 80, &shape, &g), "scale_max must be 8-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 0, 3, 5, 80, &shape, &g), "1 <= N <= 64"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 65, 3, 5, 80, &shape, &g), "1 <= N <= 64"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 0, 5, 80, &shape, &g), "1 <= S <= 8"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 9, 5, 80, &shape, &g), "1 <= S <= 8"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 3, 0, 80, &shape, &g), "r * r <= 1024"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 3, 33, 80, &shape, &g), "r * r <= 1024"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 3, 0x7fffffff, 80, &shape, &g), "r * r <= 1024"));      // r * r is never formed
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 3, 5, 0, &shape, &g), "1 <= up <= 4096"));
  EXPECT(refused(vfs_siamfc_batch_upsample_check(P, P, P, P, P, P, 2, 3, 5, 4097, &shape, &g), "1 <= up <= 4096"));

  EXPECT(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 0x7fffffffLL, 64, 8, 4096, &shape, &g) == nullptr && g.x == 64 && g.y == 1 && g.z == 1 &&
         g.threads == 1024);
  EXPECT(vfs_siamfc_batch_peak_check(U4, U8, U8, U8, U8, U4, U8, P, 1, 1, 1, 1, &shape, &g) == nullptr && g.x == 1);
  for (int k = 0; k < 8; ++k) {
    const void* a[8] = {P, P, P, P, P, P, P, P};
    a[k] = nullptr;
    EXPECT(refused(vfs_siamfc_batch_peak_check(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 8, 2, 3, 80, &shape, &g), "null buffer"));
  }
  for (int k : {1, 2, 3, 4, 6}) {
    const void* a[8] = {P, P, P, P, P, P, P, P};
    a[k] = U4;
    EXPECT(refused(vfs_siamfc_batch_peak_check(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 8, 2, 3, 80, &shape, &g),
                   "scale_max, hann, factors, state and boxes must be 8-byte aligned"));
  }
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, U2, P, P, 8, 2, 3, 80, &shape, &g), "meta must be 4-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, U8, 8, 2, 3, 80, &shape, &g), "records must be 16-byte aligned"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 8, 0, 3, 80, &shape, &g), "1 <= N <= 64"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 8, 65, 3, 80, &shape, &g), "1 <= N <= 64"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 8, 2, 0, 80, &shape, &g), "1 <= S <= 8"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 8, 2, 9, 80, &shape, &g), "1 <= S <= 8"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 8, 2, 3, 0, &shape, &g), "1 <= up <= 4096"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 8, 2, 3, 4097, &shape, &g), "1 <= up <= 4096"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 0, 2, 3, 80, &shape, &g), "1 <= rows_cap < 2^31"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, 1LL << 31, 2, 3, 80, &shape, &g), "1 <= rows_cap < 2^31"));
  EXPECT(refused(vfs_siamfc_batch_peak_check(P, P, P, P, P, P, P, P, -1, 2, 3, 80, &shape, &g), "1 <= rows_cap < 2^31"));

  std::printf(failures ? "siamfc_batch_check: %d FAILED\n" : "siamfc_batch_check: ok\n", failures);
  return failures ? 1 : 0;
}
