// CPU check of csrc/msm_plan.hpp: for a list of call geometries, every array of a bucket-pipeline MSM call lies inside its scratch
// slot, arrays that are live together do not overlap, the declared aliases lie inside what they alias, the alignments the kernels
// rely on hold, and the geometry and the three slot sizes equal the formulas of the dispatcher this header replaced, written out
// below on their own.  Built and run by tests/test_msm_plan_host.py (with the address and undefined-behaviour sanitizers).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "msm_plan.hpp"

using namespace zk;

static int failures = 0;
static const char *cur = "";
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      ++failures;                                                       \
      printf("case %s: %s fails (line %d)\n", cur, #cond, __LINE__);    \
    }                                                                   \
  } while (0)

static const char *const NAMES[MSM_ARRAYS] = {"hist", "off", "cursor", "bucket_posA", "bucket_posB", "col_hist", "col_base", "n_tasks", "heavy_count", "medium_list",
                                              "large_list", "tasks", "entries", "buckets", "partials", "chist", "coff", "ccursor", "stage", "marg"};
constexpr int OWN_ARRAYS = CHIST;   // the arrays before it own their bytes; CHIST and after are the aliases

static bool inside(const MsmRegion &in, const MsmRegion &out) { return in.slot == out.slot && in.off >= out.off && in.end() <= out.end(); }
static bool disjoint(const MsmRegion &a, const MsmRegion &b) { return a.slot != b.slot || a.end() <= b.off || b.end() <= a.off || !a.bytes || !b.bytes; }

// the formulas of the dispatcher before the plan existed, for (n, c, W, n_cols) and the value of ZKFHE_SORT
struct Expected {
  unsigned K, K1, TASK_E, NB;
  size_t col_entries, max_tasks, heavy_cap, stage_stride, bytes0, bytes1, bytes2;
  int L;
  bool two_level;
};
static Expected expected(size_t n, int c, int W, size_t n_cols, const char *sort_env) {
  Expected x;
  const unsigned K = 1u << (c - 1), K1 = K + 1;
  const size_t col_entries = n * (size_t)W;
  unsigned TASK_E;
  {
    const size_t load = col_entries / K;
    if (K <= 1024 && load > 128) {
      TASK_E = 16;
    } else {
      unsigned e = 8;
      while (e < 64u && (size_t)e * 3 < load) e <<= 1;
      TASK_E = e;
    }
  }
  const size_t max_tasks = (n_cols * col_entries) / TASK_E + (size_t)K * n_cols;
  const size_t heavy_cap = (n_cols * col_entries) / ((size_t)TASK_E * 8) + 1;
  const size_t words = 3 * n_cols * K1 + 2 * (size_t)K * n_cols + 2 * n_cols * 65 + 16 + 2 * heavy_cap + 2 * max_tasks;
  x.bytes1 = words * sizeof(unsigned);
  x.bytes2 = n_cols * col_entries * sizeof(unsigned) + 64;
  int idx_bits = 1;
  while (((size_t)1 << idx_bits) < col_entries) ++idx_bits;
  int L = 31 - idx_bits;
  if (L > 8) L = 8;
  if (sort_env && sort_env[0] == '2' && sort_env[1] == ':' && atoi(sort_env + 2) >= 6 && atoi(sort_env + 2) < L) L = atoi(sort_env + 2);
  const unsigned min_k = sort_env && sort_env[0] == '2' ? 2048u : 16384u;
  const bool two_level = K >= min_k && L >= 6 && !(sort_env && sort_env[0] == '1');
  const unsigned NB = two_level ? K >> L : 0;
  size_t s0 = (n_cols * (size_t)K + max_tasks) * 128;
  const size_t stage_stride = (col_entries + 3) & ~(size_t)3;
  if (two_level && s0 < n_cols * stage_stride * sizeof(unsigned)) s0 = n_cols * stage_stride * sizeof(unsigned);
  x.bytes0 = s0;
  x.K = K, x.K1 = K1, x.TASK_E = TASK_E, x.NB = NB, x.col_entries = col_entries, x.max_tasks = max_tasks, x.heavy_cap = heavy_cap;
  x.stage_stride = stage_stride, x.L = L, x.two_level = two_level;
  return x;
}

struct Case {
  const char *name;
  size_t n;
  int c;
  size_t n_cols;
  const char *sort_env;
  int two_level, L;   // what the sort rule must give, where the case is about it (-1: only compared with `expected`)
};

static void check(const Case &k) {
  cur = k.name;
  const int W = (254 + k.c - 1) / k.c;   // zk_basis_create_scaled
  const MsmGeometry g = msm_geometry(k.n, k.c, W, k.n_cols, msm_sort_mode(k.sort_env));
  const MsmLayout l = msm_layout(g);
  const size_t cols = k.n_cols;

  // 4, 5: geometry, sort rule and slot sizes as before
  const Expected x = expected(k.n, k.c, W, cols, k.sort_env);
  CHECK(g.n == k.n && g.n_cols == cols && g.c == k.c && g.W == W);
  CHECK(g.K == x.K && g.K1 == x.K1 && g.col_entries == x.col_entries && g.TASK_E == x.TASK_E);
  CHECK(g.max_tasks == x.max_tasks && g.heavy_cap == x.heavy_cap && g.stage_stride == x.stage_stride);
  CHECK(g.two_level == x.two_level && g.L == x.L && g.NB == x.NB);
  CHECK(l.slot_bytes[0] == x.bytes0 && l.slot_bytes[1] == x.bytes1 && l.slot_bytes[2] == x.bytes2);
  if (k.two_level >= 0) CHECK((int)g.two_level == k.two_level);
  if (k.L >= 0) CHECK(g.L == k.L && g.NB == (g.K >> k.L));
  if (!g.two_level) CHECK(g.NB == 0);

  // 1: every region inside its slot; regions that are live together apart from each other
  const MsmRegion *r = l.at;
  for (int i = 0; i < MSM_ARRAYS; ++i)
    if (!(r[i].slot >= 0 && r[i].slot < 3 && r[i].end() <= l.slot_bytes[r[i].slot] && r[i].off % 4 == 0)) {
      ++failures;
      printf("case %s: %s [%zu, %zu) leaves slot %d of %zu bytes\n", cur, NAMES[i], r[i].off, r[i].end(), r[i].slot, l.slot_bytes[r[i].slot]);
    }
  for (int i = 0; i < OWN_ARRAYS; ++i)
    for (int j = i + 1; j < OWN_ARRAYS; ++j)
      if (!disjoint(r[i], r[j])) {
        ++failures;
        printf("case %s: %s and %s overlap\n", cur, NAMES[i], NAMES[j]);
      }
  CHECK(r[ENTRIES].slot == 2 && r[BUCKETS].slot == 0 && r[PARTIALS].slot == 0);
  for (int i = HIST; i <= TASKS; ++i) CHECK(r[i].slot == 1);
  // the sizes the kernels write: k_msm_clear zeroes heavy_count[0..3], k_msm_task_fill caps each list at heavy_cap, one uint2 per task
  CHECK(r[HIST].bytes == cols * g.K1 * 4 && r[OFF].bytes == r[HIST].bytes && r[CURSOR].bytes == r[HIST].bytes);
  CHECK(r[BUCKET_POS_A].bytes == cols * g.K * 4 && r[BUCKET_POS_B].bytes == r[BUCKET_POS_A].bytes);
  CHECK(r[COL_HIST].bytes == cols * 65 * 4 && r[COL_BASE].bytes == r[COL_HIST].bytes);
  CHECK(r[N_TASKS].bytes >= 4 && r[HEAVY_COUNT].bytes >= 16);
  CHECK(r[MEDIUM_LIST].bytes == g.heavy_cap * 4 && r[LARGE_LIST].bytes == g.heavy_cap * 4);
  CHECK(r[TASKS].bytes == g.max_tasks * 8 && r[ENTRIES].bytes == cols * g.col_entries * 4);
  CHECK(r[BUCKETS].bytes == cols * g.K * 128 && r[PARTIALS].bytes == g.max_tasks * 128);
  CHECK(r[ENTRIES].end() + 32 <= l.slot_bytes[2]);   // 16-byte loads up to eight entries past a slice

  // 2: the aliases
  if (g.two_level) {
    CHECK(inside(r[CHIST], r[HIST]) && inside(r[COFF], r[CURSOR]) && inside(r[CCURSOR], r[CURSOR]));
    CHECK(disjoint(r[COFF], r[CCURSOR]));
    CHECK(r[CHIST].bytes == cols * g.NB * 4 && r[COFF].bytes == cols * (g.NB + 1) * 4 && r[CCURSOR].bytes == cols * g.NB * 4);
    CHECK(cols * (g.NB + 1) + cols * g.NB <= cols * g.K1);
    CHECK(r[STAGE].slot == 0 && r[STAGE].off == 0 && r[STAGE].bytes == cols * g.stage_stride * 4);
    CHECK((g.K >> g.L) << g.L == g.K && g.L >= 6 && g.L <= 8 && g.col_entries <= ((size_t)1 << (31 - g.L)));   // fine bits above the index bits
  }
  if (g.K >= 64) CHECK(inside(r[MARG], r[PARTIALS]) && r[MARG].bytes == cols * (g.K / 64 + 64) * 128);

  // 3: alignments
  CHECK(r[TASKS].off % 8 == 0);
  CHECK(g.stage_stride % 4 == 0 && g.stage_stride >= g.col_entries && g.stage_stride < g.col_entries + 4);
}

int main() {
  const Case cases[] = {
      {"a", 48, 5, 3, nullptr, 0, -1},             // K < 64
      {"b", 1000, 7, 20, nullptr, 0, -1},
      {"c", 8192, 13, 1, nullptr, 0, -1},
      {"d", 8192, 13, 40, nullptr, 0, -1},
      {"e", 8192, 16, 5, nullptr, 1, 8},           // K = 32768: two-level, L = 8
      {"f", 8192, 16, 5, "1", 0, -1},              // forced one-pass
      {"g", 4096, 13, 4, "2:6", 1, 6},
      {"h", 4096, 14, 4, "2:7", 1, 7},
      {"i", 5000, 14, 3, "2", 1, 8},               // odd length: the stride rounds up
      {"j", 64, 5, 4096, nullptr, 0, -1},          // the column limit
      {"k", (size_t)1 << 19, 16, 32, nullptr, 1, -1},   // arithmetic only: gigabyte slots
      {"l", (size_t)1 << 15, 14, 136, nullptr, 0, -1},
  };
  for (const Case &k : cases) check(k);
  {   // the sort mode on its own
    cur = "sort mode";
    const MsmSortMode d = msm_sort_mode(nullptr), one = msm_sort_mode("1"), two = msm_sort_mode("2"), cap = msm_sort_mode("2:6"), wide = msm_sort_mode("2:9"),
                      low = msm_sort_mode("2:5");
    CHECK(!d.one_pass && d.two_level_min_k == 16384 && d.fine_bits_cap == 8);
    CHECK(one.one_pass && one.two_level_min_k == 16384);
    CHECK(!two.one_pass && two.two_level_min_k == 2048 && two.fine_bits_cap == 8);
    CHECK(cap.two_level_min_k == 2048 && cap.fine_bits_cap == 6);
    CHECK(wide.fine_bits_cap == 8 && low.fine_bits_cap == 8);
  }
  if (failures) {
    printf("msm plan check: %d failure(s)\n", failures);
    return 1;
  }
  printf("msm plan check: ok\n");
  return 0;
}
