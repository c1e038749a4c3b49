// Stand-alone host check of the layout entry points' host side (vfs_amd/csrc/layout_host.h): the rounding, the three maps stated
// element by element and the argument checks, to be run under the sanitizers.  No HIP, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/layout_check.cpp -o layout_check
//   ./layout_check            -> "layout_check: ok", exit status 0
// The buffers are heap blocks of exactly N * HW * C elements, so an index past the end is an ASan report.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../vfs_amd/csrc/layout_host.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static float f32_of(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static bool refused(const char* got, const char* want) { return got && !std::strcmp(got, want); }

int main() {
  // rounding: ties to even on both parities, one step either side, overflow, Inf, NaN, signed zeros
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x3F808000u)) == 0x3F80);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x3F818000u)) == 0x3F82);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x3F807FFFu)) == 0x3F80);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x3F808001u)) == 0x3F81);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x7F7F0000u)) == 0x7F7F);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x7F7F8000u)) == 0x7F80);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0xFF800000u)) == 0xFF80);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x7F800001u)) == 0x7FC0);
  EXPECT(vfs_layout_f32_to_bf16(f32_of(0x80000000u)) == 0x8000 && vfs_layout_f32_to_bf16(0.f) == 0);
  for (uint32_t v = 0; v < 0x10000u; ++v) {
    const float f = vfs_layout_bf16_to_f32((uint16_t)v);
    if (!std::isnan(f)) EXPECT(vfs_layout_f32_to_bf16(f) == v);
  }
  // the maps: to_nhwc(to_nchw(x)) == x, the join rounds once, in place
  const int shapes[][3] = {{1, 1, 64}, {3, 35, 64}, {2, 65, 128}};
  for (const auto& s : shapes) {
    const int N = s[0], HW = s[1], C = s[2];
    const size_t n = (size_t)N * HW * C;
    std::vector<uint16_t> x(n), back(n), acc(n);
    std::vector<float> t(n);
    for (size_t i = 0; i < n; ++i) x[i] = (uint16_t)((i * 2654435761u) >> 13 & 0x7F7F);      // finite patterns
    vfs_layout_to_nchw_host(x.data(), t.data(), N, HW, C);
    EXPECT(t[(size_t)(C - 1) * HW] == vfs_layout_bf16_to_f32(x[C - 1]));
    vfs_layout_to_nhwc_host(t.data(), nullptr, back.data(), N, HW, C);
    EXPECT(back == x);
    for (size_t i = 0; i < n; ++i) acc[i] = 0x3F80;      // 1.0
    for (size_t i = 0; i < n; ++i) t[i] = 0.00390625f + 7.62939453125e-06f;      // 2^-8 + 2^-17: one rounding goes up, two stay
    vfs_layout_to_nhwc_host(t.data(), acc.data(), acc.data(), N, HW, C);
    EXPECT(acc[0] == 0x3F81 && acc[n - 1] == 0x3F81);
    vfs_layout_add_host(x.data(), x.data(), back.data(), (long long)n);
    EXPECT(vfs_layout_bf16_to_f32(back[5]) == 2.f * vfs_layout_bf16_to_f32(x[5]));
  }
  // the argument checks
  long long tiles = -1;
  int one = 0;
  EXPECT(vfs_layout_check(&one, nullptr, &one, 0, 2, 65, 128, &tiles) == nullptr && tiles == 2 * 2 * 2);
  EXPECT(refused(vfs_layout_check(nullptr, nullptr, &one, 0, 2, 65, 128, &tiles), "null buffer"));
  EXPECT(refused(vfs_layout_check(&one, nullptr, &one, 1, 2, 65, 128, &tiles), "null buffer"));
  EXPECT(refused(vfs_layout_check(&one, &one, &one, 1, 0, 65, 128, &tiles), "N, HW and C must be positive"));
  EXPECT(refused(vfs_layout_check(&one, &one, &one, 1, 2, 65, 96, &tiles), "C must be a multiple of 64"));
  EXPECT(refused(vfs_layout_check(&one, &one, &one, 1, 1 << 30, 1 << 30, 1 << 30, &tiles), "2^31 tiles or more"));
  EXPECT(vfs_layout_check(&one, &one, &one, 1, 0x7fffffff, 64, 64, &tiles) == nullptr && tiles == 0x7fffffffLL);
  EXPECT(refused(vfs_layout_check(&one, &one, &one, 1, 0x7fffffff, 65, 64, &tiles), "2^31 tiles or more"));
  long long blocks = -1;
  EXPECT(vfs_layout_add_check(&one, &one, &one, 8 * 257, &blocks) == nullptr && blocks == 2);
  EXPECT(refused(vfs_layout_add_check(&one, &one, &one, 12, &blocks), "n must be a multiple of 8"));
  EXPECT(refused(vfs_layout_add_check(&one, &one, &one, 0, &blocks), "n must be positive"));
  std::printf(failures ? "layout_check: %d failure(s)\n" : "layout_check: ok\n", failures);
  return failures != 0;
}
