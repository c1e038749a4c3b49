// Stand-alone host check of the table-driven optimizer step's host side (vfs_amd/csrc/opt_table.h): the segment-map builder and the
// argument checks, to be run under the sanitizers.  No HIP, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/opt_table_check.cpp -o opt_table_check
//   ./opt_table_check            -> "opt_table_check: ok", exit status 0
// The map buffers are heap blocks of exactly the size vfs_opt_map_words_of() names, so a write past the end is an ASan report.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../vfs_amd/csrc/opt_table.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static bool refused(const char* got, const char* want) { return got && !std::strcmp(got, want); }

// what the kernel does with the map: the segment of vector i, or -1
static int lookup(const std::vector<int>& map, int nseg, long long i) {
  int s = map[4 * (size_t)nseg + (size_t)(i >> 8)];
  for (; s < nseg; ++s)
    if ((long long)map[4 * s + 1] + (map[4 * s + 3] != 0) > i) break;
  return (s == nseg || map[4 * s] > i) ? -1 : s;
}

static void check_layout(const std::vector<long long>& segs, long long n, int ngroups) {
  const int nseg = (int)(segs.size() / 3);
  const long long words = vfs_opt_map_words_of(n, nseg);
  std::vector<int> map((size_t)words + 1);      // as large as asked for; one int of slack only keeps data() non-null at 0 words
  static const long long none[3] = {0, 0, 0};
  EXPECT(vfs_opt_map_build(nseg ? segs.data() : none, nseg, n, ngroups, map.data(), words) == nullptr);
  map.pop_back();
  map.shrink_to_fit();                          // exactly `words` ints from here on: the look-ups below may not read past them
  // every vector of the arena against a direct search of the segment list
  for (long long i = 0; i < (n + 3) / 4; ++i) {
    int want = -1;
    for (int s = 0; s < nseg; ++s)
      if (segs[3 * s] <= 4 * i && 4 * i < segs[3 * s + 1]) want = s;
    const int got = lookup(map, nseg, i);
    EXPECT(got == want);
    if (got >= 0) {
      EXPECT(map[4 * got + 2] == (int)segs[3 * got + 2]);
      const long long covered = i < map[4 * got + 1] ? 4 : map[4 * got + 3];      // words of this vector the kernel touches
      EXPECT(4 * i + covered <= segs[3 * got + 1] && covered > 0);
    }
  }
}

int main() {
  // the hand-made layout of tests/test_optim_table.py: edges before, on and behind a 1024-word chunk edge
  check_layout({4, 5, 0, 8, 11, 1, 12, 16, 2, 16, 21, 0, 1024, 2048, 1, 2048, 3069, 2, 3072, 4099, 0}, 4112, 3);
  check_layout({}, 0, 1);
  check_layout({}, 5000, 1);
  check_layout({0, 1, 0}, 1, 1);
  check_layout({0, 4101, 0}, 4101, 1);
  // random layouts: parameters of 1 .. 3000 words padded to 4, some frozen, up to 448 groups
  std::mt19937 rng(7);
  for (int trial = 0; trial < 200; ++trial) {
    std::vector<long long> segs;
    long long o = 0;
    const int nparams = 1 + (int)(rng() % 60), ngroups = 1 + (int)(rng() % VFS_OPT_MAX_GROUPS);
    for (int k = 0; k < nparams; ++k) {
      const long long numel = 1 + (long long)(rng() % (rng() % 4 ? 40 : 3000));
      if (rng() % 4) segs.insert(segs.end(), {o, o + numel, (long long)(rng() % ngroups)});
      o += (numel + 3) / 4 * 4;
    }
    check_layout(segs, o, ngroups);
  }

  // the builder's refusals
  std::vector<int> map(64);
  const long long one[] = {0, 4, 0}, outside[] = {0, 65, 0}, negative[] = {-4, 4, 0}, empty[] = {8, 8, 0}, odd[] = {2, 8, 0};
  const long long unsorted[] = {8, 12, 0, 0, 4, 1}, shared[] = {0, 9, 0, 8, 12, 1}, group[] = {0, 4, 2};
  EXPECT(refused(vfs_opt_map_build(nullptr, 1, 64, 2, map.data(), 64), "null buffer"));
  EXPECT(refused(vfs_opt_map_build(one, 1, 64, 2, nullptr, 64), "null buffer"));
  EXPECT(refused(vfs_opt_map_build(one, 1, -1, 2, map.data(), 64), "n < 0"));
  EXPECT(refused(vfs_opt_map_build(one, 1, 1LL << 33, 2, map.data(), 64), "n < 2^33"));
  EXPECT(refused(vfs_opt_map_build(one, -1, 64, 2, map.data(), 64), "nseg < 0"));
  EXPECT(refused(vfs_opt_map_build(one, 1, 64, 0, map.data(), 64), "1 <= ngroups <= 448"));
  EXPECT(refused(vfs_opt_map_build(one, 1, 64, 449, map.data(), 64), "1 <= ngroups <= 448"));
  EXPECT(refused(vfs_opt_map_build(one, 1, 64, 2, map.data(), 4), "map smaller than vfs_opt_segment_map_words(n, nseg)"));
  EXPECT(refused(vfs_opt_map_build(outside, 1, 64, 2, map.data(), 64), "segments must be non-empty and inside [0, n)"));
  EXPECT(refused(vfs_opt_map_build(negative, 1, 64, 2, map.data(), 64), "segments must be non-empty and inside [0, n)"));
  EXPECT(refused(vfs_opt_map_build(empty, 1, 64, 2, map.data(), 64), "segments must be non-empty and inside [0, n)"));
  EXPECT(refused(vfs_opt_map_build(odd, 1, 64, 2, map.data(), 64), "segments must begin on a multiple of 4 words"));
  EXPECT(refused(vfs_opt_map_build(unsorted, 2, 64, 2, map.data(), 64), "segments must be sorted and must not share a 16-byte vector"));
  EXPECT(refused(vfs_opt_map_build(shared, 2, 64, 2, map.data(), 64), "segments must be sorted and must not share a 16-byte vector"));
  EXPECT(refused(vfs_opt_map_build(group, 1, 64, 2, map.data(), 64), "segment group outside [0, ngroups)"));

  // the step's refusals; P: any 16-byte aligned address (never dereferenced by the checks), H: a real host table
  alignas(16) static float P[16];
  std::vector<float> H(VFS_OPT_HYPER * 3, 0.f), H9(VFS_OPT_HYPER * 3, 0.9f);
  const void* U1 = (const char*)P + 4;
  EXPECT(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, nullptr, 16, P, 1, H.data(), 3, P, 0, 0) == nullptr);
  EXPECT(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, nullptr, 16, P, 1, H9.data(), 3, P, 1, 0) == nullptr);
  EXPECT(vfs_opt_step_check(VFS_OPT_ADAMW, P, P, P, P, 16, P, 1, H.data(), 3, P, 0, 1) == nullptr);
  EXPECT(refused(vfs_opt_step_check(3, P, P, P, P, 16, P, 1, H.data(), 3, P, 0, 1), "kind must be 0 (SGD), 1 (Adam) or 2 (AdamW)"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, nullptr, P, P, P, 16, P, 1, H.data(), 3, P, 0, 1), "null buffer"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_ADAM, P, P, P, nullptr, 16, P, 1, H.data(), 3, P, 0, 1), "null buffer"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, P, 16, P, 1, nullptr, 3, P, 0, 1), "null buffer"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, U1, P, P, P, 16, P, 1, H.data(), 3, P, 0, 1), "16-byte aligned buffers"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, P, 16, U1, 1, H.data(), 3, P, 0, 1), "16-byte aligned buffers"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, P, -1, P, 1, H.data(), 3, P, 0, 1), "n < 0"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, P, 16, P, -1, H.data(), 3, P, 0, 1), "nseg < 0"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, P, 16, P, 1, H.data(), 449, P, 0, 1), "1 <= ngroups <= 448"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_ADAM, P, P, P, P, 16, P, 1, H.data(), 3, P, 0, 0), "step >= 1"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_ADAM, P, P, P, P, 16, P, 1, H.data(), 3, P, 1, 1), "nesterov is SGD's"));
  EXPECT(refused(vfs_opt_step_check(VFS_OPT_SGD, P, P, P, P, 16, P, 1, H.data(), 3, P, 1, 1), "nesterov needs momentum > 0"));

  std::printf(failures ? "opt_table_check: %d FAILED\n" : "opt_table_check: ok\n", failures);
  return failures ? 1 : 0;
}
