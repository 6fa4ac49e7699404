// The plan of one bucket-pipeline MSM call (msm.hip): the geometry that follows from (n, window bits, windows, columns) and the
// sort mode, and where every array of the call lives in the context's scratch slots 0, 1 and 2.  Plain host C++ with no HIP in it:
// tests/native/msm_plan_check.cpp checks the regions against each other and against the slot sizes on the CPU, before any kernel
// is handed a pointer made from them.
#pragma once
#include <cstddef>
#include <cstdlib>

namespace zk {

constexpr int TASK_E_MAX = 64;          // longest accumulation task (entries)
constexpr unsigned TASK_BINS = 65;      // slice lengths 0..64
constexpr int MERGE_LIGHT = 8;          // partials merged by a single thread; more -> eight lanes or one wave per bucket
constexpr unsigned MERGE_MEDIUM = 128;  // up to this many partials: eight lanes per bucket; beyond: one wave per bucket
constexpr int FINE_BITS_MAX = 8;        // F = 256 buckets per coarse bin: enough workgroups in k_msm_fine on a basis of 2^15 points
constexpr size_t MSM_POINT_BYTES = 128; // sizeof(G1X): buckets, partials, marginals

// ZKFHE_SORT: "1" the one-pass sort for every basis; "2" the two-level sort from 2048 buckets on (by default from 16384: K = 8192
// measured equal either way, at K = 32768 the two-level sort halves the sorting time); "2:<bits>" also caps the fine bits (tests:
// the geometry of n = 2^19 on a short basis).
struct MsmSortMode { bool one_pass; unsigned two_level_min_k; int fine_bits_cap; };
inline MsmSortMode msm_sort_mode(const char *env) {
  const bool two = env && env[0] == '2';
  const int bits = two && env[1] == ':' ? atoi(env + 2) : 0;
  return {env && env[0] == '1', two ? 2048u : 16384u, bits >= 6 && bits < FINE_BITS_MAX ? bits : FINE_BITS_MAX};
}

// ~3 tasks per bucket of a full-width column (profiles/r1_task_len.md): with the length-sorted task list every wave runs equal
// chains whatever E is, so E only trades the number of partials the merge has to add against the number of tasks available to
// fill the chip; 16 at k = 13 (40 entries per bucket) measured best end to end.
inline unsigned msm_task_len(size_t col_entries, unsigned K) {
  const size_t load = col_entries / K;
  // narrow windows on a long basis (the prover's c = 10 tables for columns of small values): the nominal load says 64, but those
  // columns fill a few buckets with thousands of entries and leave the rest nearly empty -- 16 keeps the chains of the full
  // buckets short (measured: 117 proofs/s against 115 at 32 and 114 at 64)
  if (K <= 1024 && load > 128) return 16;
  unsigned e = 8;
  while (e < (unsigned)TASK_E_MAX && (size_t)e * 3 < load) e <<= 1;
  return e;
}

// n points and n_cols columns; c window bits, W signed windows; K buckets per column, K1 = K + 1; col_entries = n * W, the most
// sorted entries a column can have; TASK_E entries per accumulation task, max_tasks the bound on their number, heavy_cap the bound on
// the buckets with more than MERGE_LIGHT partials; two_level: the two-level sort (k_msm_chist .. k_msm_fine), with L fine bits of
// the bucket id (they travel in the entry word above the log2(W n) index bits) and NB = K >> L coarse bins (0 with the one-pass
// sort); stage_stride = col_entries rounded up to four entries: k_msm_fine reads the staged entries in 16-byte loads.
struct MsmGeometry {
  size_t n, n_cols, col_entries, max_tasks, heavy_cap, stage_stride;
  int c, W, L;
  unsigned K, K1, TASK_E, NB;
  bool two_level;
};

inline MsmGeometry msm_geometry(size_t n, int c, int windows, size_t n_cols, const MsmSortMode &mode) {
  MsmGeometry g{};
  g.n = n, g.n_cols = n_cols, g.c = c, g.W = windows;
  g.K = 1u << (c - 1), g.K1 = g.K + 1;
  g.col_entries = n * (size_t)windows;
  g.TASK_E = msm_task_len(g.col_entries, g.K);
  g.max_tasks = (n_cols * g.col_entries) / g.TASK_E + (size_t)g.K * n_cols;
  g.heavy_cap = (n_cols * g.col_entries) / ((size_t)g.TASK_E * MERGE_LIGHT) + 1;
  int idx_bits = 1;
  while (((size_t)1 << idx_bits) < g.col_entries) ++idx_bits;
  g.L = 31 - idx_bits < mode.fine_bits_cap ? 31 - idx_bits : mode.fine_bits_cap;
  g.two_level = g.K >= mode.two_level_min_k && g.L >= 6 && !mode.one_pass;
  g.NB = g.two_level ? g.K >> g.L : 0;
  g.stage_stride = (g.col_entries + 3) & ~(size_t)3;
  return g;
}

// The arrays of a call.  Slot 1 holds the sort's counters and the task list (4-byte words but for the tasks: uint2, on an 8-byte
// boundary), slot 2 the sorted entries (padded by 64 bytes: k_msm_accumulate reads them in 16-byte loads that run past a slice's
// end), slot 0 the buckets and the accumulation partials.
// The last five are aliases.  The two-level sort's counters live inside regions of the one-pass sort, which it does not use (CHIST
// in HIST, COFF and CCURSOR in CURSOR); its staging array lies over slot 0 and is dead before buckets and partials are written; the
// marginals of the bucket reduction take the place of the partials once the buckets are merged.
enum MsmArray {
  HIST, OFF, CURSOR, BUCKET_POS_A, BUCKET_POS_B, COL_HIST, COL_BASE, N_TASKS, HEAVY_COUNT, MEDIUM_LIST, LARGE_LIST, TASKS,   // slot 1
  ENTRIES,                                                                                                                  // slot 2
  BUCKETS, PARTIALS,                                                                                                        // slot 0
  CHIST, COFF, CCURSOR, STAGE, MARG,                                                                                        // aliases
  MSM_ARRAYS
};
struct MsmRegion {
  int slot;            // of the context's scratch slots
  size_t off, bytes;   // inside the slot
  size_t end() const { return off + bytes; }
};
struct MsmLayout {
  size_t slot_bytes[3];
  MsmRegion at[MSM_ARRAYS];
};

inline MsmLayout msm_layout(const MsmGeometry &g) {
  MsmLayout l{};
  const size_t cols = g.n_cols, K = g.K;
  size_t next = 0;
  auto words = [&](MsmArray a, size_t w) {
    l.at[a] = {1, next, w * 4};
    next += w * 4;
  };
  words(HIST, cols * g.K1), words(OFF, cols * g.K1), words(CURSOR, cols * g.K1);
  words(BUCKET_POS_A, K * cols), words(BUCKET_POS_B, K * cols);
  words(COL_HIST, cols * TASK_BINS), words(COL_BASE, cols * TASK_BINS);
  words(N_TASKS, 4), words(HEAVY_COUNT, 4);
  words(MEDIUM_LIST, g.heavy_cap), words(LARGE_LIST, g.heavy_cap);
  next = (next + 7) & ~(size_t)7;
  words(TASKS, 2 * g.max_tasks);
  l.slot_bytes[1] = (3 * cols * g.K1 + 2 * K * cols + 2 * cols * TASK_BINS + 16 + 2 * g.heavy_cap + 2 * g.max_tasks) * 4;
  l.at[CHIST] = {1, l.at[HIST].off, cols * g.NB * 4};
  l.at[COFF] = {1, l.at[CURSOR].off, cols * (g.NB + 1) * 4};
  l.at[CCURSOR] = {1, l.at[COFF].end(), cols * g.NB * 4};
  l.at[ENTRIES] = {2, 0, cols * g.col_entries * 4};
  l.slot_bytes[2] = l.at[ENTRIES].bytes + 64;
  l.at[BUCKETS] = {0, 0, cols * K * MSM_POINT_BYTES};
  l.at[PARTIALS] = {0, l.at[BUCKETS].end(), g.max_tasks * MSM_POINT_BYTES};
  l.at[MARG] = {0, l.at[PARTIALS].off, cols * (K / 64 + 64) * MSM_POINT_BYTES};
  l.at[STAGE] = {0, 0, g.two_level ? cols * g.stage_stride * 4 : 0};
  l.slot_bytes[0] = l.at[PARTIALS].end() > l.at[STAGE].bytes ? l.at[PARTIALS].end() : l.at[STAGE].bytes;
  return l;
}

}  // namespace zk
