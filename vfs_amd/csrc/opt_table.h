// Host side of the table-driven optimizer step (vfs_opt_step_table): the segment map of the parameter arena and the argument
// checks.  Plain C++ without any HIP, so that a stand-alone host program (tools/opt_table_check.cpp) can run it under the sanitizers.
//
// Segment map, `vfs_opt_map_words(n, nseg)` ints:
//   nseg entries {begin4, end4, group, tail}: the trainable words [4 begin4, 4 end4 + tail) of the arena belong to param group
//     `group`; the 16-byte vectors begin4 .. end4-1 are whole, vector end4 holds `tail` (0..3) words of the segment.  A segment
//     begins on a vector and the next one begins on a later vector (parameters are padded to 4 words), so a vector belongs to at
//     most one segment and the words of a last, partial vector beyond `tail` are nobody's: they are neither read nor written.
//   one entry per chunk of VFS_OPT_CHUNK_WORDS words: the index of the first segment that ends behind the chunk's first vector.
//     A workgroup pass covers exactly one chunk, reads this one index and walks on from there - past the segments of its own
//     chunk at the most, never over the table.
#pragma once

#define VFS_OPT_SGD 0
#define VFS_OPT_ADAM 1
#define VFS_OPT_ADAMW 2
#define VFS_OPT_CHUNK_WORDS 1024      // 256 lanes x one 16-byte vector
#define VFS_OPT_HYPER 8               // floats per param group in the hyperparameter table
#define VFS_OPT_WRITE_GROUPS 224      // param groups that travel by value with one launch (7168 bytes of kernel arguments): a
                                      // ResNet-50 with its head, one group per parameter (177), rides with the update launch
#define VFS_OPT_MAX_GROUPS 448        // two table-write launches

static inline long long vfs_opt_map_words_of(long long n, int nseg) {
  return 4LL * nseg + (n + VFS_OPT_CHUNK_WORDS - 1) / VFS_OPT_CHUNK_WORDS;
}

// segments: nseg x {begin, end, group} in words, host memory.  nullptr when the map was written, else what is wrong.
static inline const char* vfs_opt_map_build(const long long* segments, int nseg, long long n, int ngroups, int* map, long long words) {
  if (!segments || !map) return "null buffer";
  if (n < 0) return "n < 0";
  if (n >= (1LL << 33)) return "n < 2^33";
  if (nseg < 0) return "nseg < 0";
  if (ngroups < 1 || ngroups > VFS_OPT_MAX_GROUPS) return "1 <= ngroups <= 448";
  if (words < vfs_opt_map_words_of(n, nseg)) return "map smaller than vfs_opt_segment_map_words(n, nseg)";
  long long prev_end = 0;
  for (int s = 0; s < nseg; ++s) {
    const long long b = segments[3 * s], e = segments[3 * s + 1], grp = segments[3 * s + 2];
    if (b < 0 || e > n || b >= e) return "segments must be non-empty and inside [0, n)";
    if (b & 3) return "segments must begin on a multiple of 4 words";
    if (b < (prev_end + 3) / 4 * 4) return "segments must be sorted and must not share a 16-byte vector";
    if (grp < 0 || grp >= ngroups) return "segment group outside [0, ngroups)";
    prev_end = e;
  }
  for (int s = 0; s < nseg; ++s) {
    const long long b = segments[3 * s], e = segments[3 * s + 1];
    map[4 * s] = (int)(b >> 2);
    map[4 * s + 1] = (int)(e >> 2);
    map[4 * s + 2] = (int)segments[3 * s + 2];
    map[4 * s + 3] = (int)(e & 3);
  }
  int* first = map + 4LL * nseg;
  const long long nchunks = (n + VFS_OPT_CHUNK_WORDS - 1) / VFS_OPT_CHUNK_WORDS;
  int s = 0;
  for (long long c = 0; c < nchunks; ++c) {
    while (s < nseg && segments[3 * s + 1] <= c * VFS_OPT_CHUNK_WORDS) ++s;      // ends at or before the chunk's first word
    first[c] = s;
  }
  return nullptr;
}

// the checks of vfs_opt_step_table that need no device: nullptr, or what is wrong
static inline const char* vfs_opt_step_check(int kind, const void* params, const void* grads, const void* state1, const void* state2,
                                             long long n, const void* map, int nseg, const float* hyper, int ngroups, const void* table,
                                             int nesterov, int step) {
  if (kind != VFS_OPT_SGD && kind != VFS_OPT_ADAM && kind != VFS_OPT_ADAMW) return "kind must be 0 (SGD), 1 (Adam) or 2 (AdamW)";
  if (!params || !grads || !state1 || !map || !hyper || !table || (kind != VFS_OPT_SGD && !state2)) return "null buffer";
  if (((unsigned long long)params | (unsigned long long)grads | (unsigned long long)state1 | (unsigned long long)state2 |
       (unsigned long long)map | (unsigned long long)table) & 15)
    return "16-byte aligned buffers";
  if (n < 0) return "n < 0";
  if (n >= (1LL << 33)) return "n < 2^33";
  if (nseg < 0) return "nseg < 0";
  if (ngroups < 1 || ngroups > VFS_OPT_MAX_GROUPS) return "1 <= ngroups <= 448";
  if (kind != VFS_OPT_SGD && step < 1) return "step >= 1";
  if (kind != VFS_OPT_SGD && nesterov) return "nesterov is SGD's";
  if (kind == VFS_OPT_SGD && nesterov)
    for (int g = 0; g < ngroups; ++g)
      if (!(hyper[g * VFS_OPT_HYPER + 2] > 0.f)) return "nesterov needs momentum > 0";
  return nullptr;
}
