// Batched multi-scalar multiplication over BN254 G1 for gfx950 (the KZG commit of the prover).
//
// Replaces halo2_proofs `arithmetic::best_multiexp(&[Fr], &[G1Affine]) -> G1` as called by
// `ParamsKZG::{commit, commit_lagrange}` (third-party; reached from reference examples/bfv.rs:311).
// The result is a group element, so any exact algorithm gives identical bytes once normalised to
// affine; parity is checked against oracle/oracle.c orc_msm.
//
// Two algorithms.  (1) The bucket pipeline -- Pippenger with ONE bucket set per MSM and per-window precomputed bases (wide calls
// at n >= 2^15, every call at n >= 2^18):
//   * The SRS is fixed, HBM is 288 GB: zkfhe_basis_create stores T[w][i] = 2^(c*w) * P_i for every
//     signed window w (n*W*64 bytes; 10 MiB at n = 2^13, c = 13).  Digit d of scalar i in window w then
//     contributes sign(d) * T[w][i] to bucket |d| -- all windows share the same 2^(c-1) buckets, so
//     there is one bucket reduction per MSM and no window-combining doublings at all.
//   * Scalars are taken out of Montgomery form and folded to sign-magnitude (s > r/2 -> r - s with the
//     point negated), so the "negative small" witness values (r - x) cost as little as small ones,
//     and zero digits are skipped.
//   * entries (bucket, table index, sign) are counting-sorted per MSM (LDS-privatised histogram per 2048-scalar chunk,
//     exclusive scan, scatter).  Every bucket is cut into equal slices of <= E entries (E ~ bucket load / 3); the task
//     list is counting-sorted by slice length, so the 64 lanes of a wave sum slices of the same length with XYZZ mixed
//     additions and the dependent chain is bounded however skewed a column is (witness columns hold thousands of 0/1
//     cells).  A bucket's partials are merged by a thread (<= 8), by eight lanes (<= 128) or by a wave.
//   * bucket reduction sum_b b*B_b for K <= 32768 buckets: idx = 64 a + b; row and column marginal sums, then per MSM a
//     lane-parallel double-and-add over the marginals and a shuffle tree; the result is normalised to affine in the
//     same kernel (k_msm_marginals, k_msm_weighted; k_msm_small for fewer than 64 buckets).
// All MSMs of a batch (columns sharing the basis) run through each stage in ONE launch.
//
// Field arithmetic of every kernel between the tables and the final normalisation: radix 2^29, nine limbs, Montgomery
// constant 2^261 (fq29.hip.hpp: 162 carry-free multiply-adds per product instead of 128 multiply-add + carry pairs, lazy
// reduction in the point formulas).  The tables, partials, buckets and marginals hold packed 256-bit words in that
// form; k_msm_weighted / k_msm_table_fold convert the one result per MSM back before normalising it.
//
// (2) When the digit-multiple table of a basis fits its HBM budget (zkfhe_basis_create: 43 GB per SRS half at n = 2^13, 13-bit
// digits) the whole pipeline above is replaced by k_msm_table: T[i][w][j] = j * 2^(13 w) * P_i is resident, so an MSM is a
// plain sum of <= 20 n table points per column -- no sort, no buckets, no weights, one launch (+ a fold) instead of
// thirteen.  Same additions as the bucket pipeline's accumulation, none of the rest: 0.9x the VALU instructions on full-width
// columns, 0.75x on witness columns, and 0.2 ms instead of 0.54 for a lone column (profiles/r2b_msm_table.md).  The bucket
// pipeline stays for bases whose table would not fit (n >= 2^18) or would force so many more windows that it loses.
//
// This file is the host path: the table budget, basis create / destroy, the dispatcher with one function per stage of the bucket
// pipeline, and the C ABI.  A bucket-pipeline call's geometry and scratch layout are decided in msm_plan.hpp (host-only, checked on
// the CPU by tests/native/msm_plan_check.cpp); the kernels live in msm_sort.hip.hpp (digits, both sorts), msm_bucket.hip.hpp (tasks,
// accumulate, merge, reductions) and msm_table.hip.hpp (basis tables, k_msm_table, fold, sparse).  One translation unit.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "msm_plan.hpp"
// the kernels
#include "msm_sort.hip.hpp"
#include "msm_bucket.hip.hpp"
#include "msm_table.hip.hpp"

using namespace zk;

namespace {

constexpr size_t MSM_MAX_COLS = 4096;   // columns per call (ticket counters of the table path)

__global__ void __launch_bounds__(256) k_g1_add(const G1Affine *__restrict__ a, const G1Affine *__restrict__ b,
                                                G1Affine *__restrict__ out, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1X acc = g1x_from_affine(a[i]);
  g1x_add_affine(acc, b[i], false);
  out[i] = g1x_to_affine(acc);
}

__global__ void __launch_bounds__(256) k_g1_mul(const G1Affine *__restrict__ p, const Fr *__restrict__ k,
                                                G1Affine *__restrict__ out, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr s = fp_from_mont<FrP>(k[i]);
  const G1Affine base = p[i];
  G1X acc = G1X::identity();
  for (int bit = 255; bit >= 0; --bit) {
    acc = g1x_dbl(acc);
    if ((s.l[bit >> 5] >> (bit & 31)) & 1) g1x_add_affine(acc, base, false);
  }
  out[i] = g1x_to_affine(acc);
}

// Window width of the digit-multiple table: the widest (<= 15 bits) whose table fits the per-basis budget.
//   * ZKFHE_TABLE_GB unset (the library default): 48 GB, and never more than a quarter of the memory that is free on the device when
//     the basis is made -- n = 2^13: 13-bit digits for the Lagrange half of an SRS (43 GB), 11 for the monomial half, which gets
//     0.3 of the budget (srs.hip; 13 GB): 56 GB per SRS.  A library that is one tenant of the device among others (a second key, another process, a
//     k = 16 key next to a k = 13 one) must not take two thirds of it by default.
//   * ZKFHE_TABLE_GB=<GB>: an explicit budget -- the SERVICE profile of a prover that owns the GPU is 160 (bench.py sets it): 15-bit
//     digits at n = 2^13, 17 windows x 16 384 multiples x 64 B per base point, 146 GB + 43 GB (13 bits) = 189 GB per SRS; the wide
//     commitment calls then need 21.4 M additions per proof against 24.9 M with 13 bits (profiles/r5_table_budget.md: rate against
//     resident GB and build time).  A table may hold more than 2^31 entries: k_msm_table addresses it relative to the chunk it sums.
// Longer bases get narrower digits from the same budget (2^16: 11 bits, 2^19: 8 bits for the Lagrange half alone); their wide calls
// take the bucket pipeline and the table serves the calls of a few columns.  ZKFHE_TABLE_BITS forces a width (0 = no table).
// Whatever the budget says, zk_basis_create_scaled narrows the table until it fits beside a reserve for proving keys and workspaces
// (table_reserve_bytes) and reports what it built (zkfhe_basis_table_bits / _bytes; one line on stderr with ZKFHE_VERBOSE).
int table_bits(size_t n, double budget_scale) {
  // read per basis (creation is rare): tests switch widths inside one process
  const char *e = getenv("ZKFHE_TABLE_BITS");
  const int forced = e ? atoi(e) : -1;
  const char *g = getenv("ZKFHE_TABLE_GB");
  double gb = g ? atof(g) : 48.0;
  if (!g) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b / 4.0 < gb * 1073741824.0) gb = (double)free_b / 4.0 / 1073741824.0;
  }
  const double budget = gb * 1073741824.0 * budget_scale;
  auto fits = [&](int c) {
    const double entries = (double)n * (double)((255 + c - 1) / c) * (double)(1u << (c - 1));
    return c >= 8 && c <= 15 && entries * sizeof(G1Affine) <= budget;
  };
  if (forced >= 0) return forced > 0 && fits(forced) ? forced : 0;
  for (int c = 15; c >= 8; --c)
    if (fits(c)) return c;
  return 0;
}

// What stays free on the device after a table is allocated: room for proving keys (k = 13: 0.34 GB, k = 19: 11 GB) and prover
// workspaces (0.5 GB per stream at k = 13, 16 - 20 streams; several GB each at k = 19) -- an eighth of the device, at least 24 GB
// (ZKFHE_TABLE_RESERVE_GB overrides).
size_t table_reserve_bytes(size_t total_b) {
  if (const char *r = getenv("ZKFHE_TABLE_RESERVE_GB")) return (size_t)(atof(r) * 1073741824.0);
  const size_t eighth = total_b / 8, floor_b = (size_t)24 << 30;
  return eighth > floor_b ? eighth : floor_b;
}

BiasArg table_bias(int c, int W) {
  BiasArg B;
  memset(&B, 0, sizeof(B));
  for (int w = 0; w < W; ++w) {
    const int bit = c * w + c - 1;
    B.l[bit >> 5] |= 1u << (bit & 31);
  }
  return B;
}

// k_msm_table with the digit width as a literal for the widths a 2^13 basis gets -- 15 and 13 under the service profile (Lagrange
// and monomial half), 13 and 11 under the library's default budget, 9 under the 4 GB of the test suite -- and with the width as an
// argument for the rest.  ZKFHE_TABLE_GENERIC=1 (read per call: a test runs one basis through both) takes the latter for every width.
using TableKernel = decltype(&k_msm_table<false, 0>);
template <bool TREE>
TableKernel table_kernel(int c) {
  const char *g = getenv("ZKFHE_TABLE_GENERIC");
  if (!g || g[0] != '1') switch (c) {
      case 9: return k_msm_table<TREE, 9>;
      case 11: return k_msm_table<TREE, 11>;
      case 13: return k_msm_table<TREE, 13>;
      case 15: return k_msm_table<TREE, 15>;
    }
  return k_msm_table<TREE, 0>;
}

int msm_table(zkfhe_ctx *ctx, const zkfhe_basis *basis, const Fr *scalars, size_t col_stride, size_t n_cols, void *out, bool xyzz) {
  const size_t n = basis->n;
  const int c = basis->mc, W = basis->mw;
  // n_part | col_next | adds
  const size_t words = 2 * MSM_MAX_COLS + 4;
  if (!ctx->tickets) {
    ZK_HIP(ctx, hipMalloc((void **)&ctx->tickets, words * sizeof(unsigned)));
    ZK_HIP(ctx, zk_memset_async(ctx, ctx->tickets, 0, words * sizeof(unsigned), ctx->stream));
  }
  unsigned *n_part = ctx->tickets, *col_next = ctx->tickets + MSM_MAX_COLS;
  unsigned long long *adds = (unsigned long long *)(ctx->tickets + 2 * MSM_MAX_COLS);
  const size_t grid_max = (size_t)ctx->num_cu * 3;
  // chunk: 256 points when the call fills the chip that way, else 128 (a lone column of 2^13: 64 workgroups, 11 additions
  // per thread and a 9-addition butterfly each -- a smaller chunk shortens the chain and multiplies the butterflies).  Under the
  // throughput profile (ctx.hpp) the chunk stays at 256: the workgroups the call leaves idle belong to other proofs, and every visit
  // of the <true> kernel that is not made saves its block_sum_256.  -DZK_MSM_THROUGHPUT_P=128 builds the old choice for an A/B run:
  // 16 streams, gate 4, 768 timed proofs, four runs each, 285.7 against 279.2 proofs/s (+2.3 %; profiles/throughput_profile.md).
#ifndef ZK_MSM_THROUGHPUT_P
#define ZK_MSM_THROUGHPUT_P 256
#endif
  size_t P = 256;
  const size_t P_min = ctx->throughput ? ZK_MSM_THROUGHPUT_P : 128;
  while (P > P_min && n_cols * ((n + P - 1) / P) < grid_max) P >>= 1;
  const size_t cpc = (n + P - 1) / P, n_items = n_cols * cpc;
  const size_t grid = n_items < grid_max ? n_items : grid_max;
  const size_t max_part = cpc < grid ? cpc : grid;   // visits to one column
  const bool tree = n_cols <= 16;
  const unsigned L = tree ? 1 : 256;
  void *p0, *p1;
  ZK_CK(zk_scratch(ctx, 0, n_cols * max_part * L * sizeof(G1X), &p0));
  ZK_CK(zk_scratch(ctx, 1, grid * P * (size_t)W * 4, &p1));
  const int slot = n_cols * n > ((size_t)1 << 16) ? 0 : 2;   // profiling slot: a wide call or one of a few columns
  if (ctx->prof_on) ZK_HIP(ctx, zk_memset_async(ctx, adds, 0, 8, ctx->stream));
  zk_prof_begin(ctx);
  (tree ? table_kernel<true>(c) : table_kernel<false>(c))<<<(unsigned)grid, 256, 0, ctx->stream>>>(scalars, col_stride, n, basis->mult, c, W, table_bias(c, W), (unsigned)P, (unsigned)cpc,
                                                                                           (unsigned)n_cols, (unsigned)max_part, (G1X *)p0, n_part, col_next, (unsigned *)p1,
                                                                                           ctx->prof_on ? adds : nullptr);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, slot, 96.0 * (double)n * (double)n_cols);
  (xyzz ? k_msm_table_fold<true> : k_msm_table_fold<false>)<<<(unsigned)n_cols, 512, 0, ctx->stream>>>((const G1X *)p0, (unsigned)max_part, L, n_part, col_next, out);
  ZK_LAUNCH_CHECK(ctx);
  if (ctx->prof_on) {
    unsigned long long h = 0;
    ZK_HIP(ctx, hipMemcpy(&h, adds, 8, hipMemcpyDeviceToHost));
    ctx->prof_ops[slot] += (double)h;
    if (getenv("ZKFHE_VERBOSE")) fprintf(stderr, "[zkfhe] msm_table: %zu columns of %zu, %d-bit digits: %llu additions\n", n_cols, n, c, h);
  }
  return ZKFHE_OK;
}

int default_window_bits(size_t n) {
  if (n <= 64) return 5;
  if (n <= 1024) return 8;
  if (n <= 4096) return 11;
  if (n <= 16384) return 13;
  if (n <= 131072) return 14;
  return 16;
}

// The table path takes the calls of many columns when its windows are at most two more than the bucket pipeline's (whose sort and
// bucket reduction cost about that much).  ZKFHE_TABLE_WIDE=1 / 0 forces the choice; read once per process.
bool table_wide(const zkfhe_basis *b) {
  static const char *env = getenv("ZKFHE_TABLE_WIDE");
  return env ? env[0] == '1' : b->mw <= b->windows + 2;
}

// ---- the bucket pipeline, stage by stage -----------------------------------------------------------------------------------
// msm_plan.hpp decides the geometry of a call and where its arrays lie; MsmScratch is that layout as device pointers, made in
// msm_scratch and nowhere else: a.at(HIST) is the array HIST of the plan.
static_assert(sizeof(G1X) == MSM_POINT_BYTES, "msm_plan.hpp sizes buckets, partials and marginals as G1X");
struct MsmScratch {
  char *p[MSM_ARRAYS];
  template <class T = unsigned>
  T *at(MsmArray a) const { return (T *)p[a]; }
};

int msm_scratch(zkfhe_ctx *ctx, const MsmGeometry &g, MsmScratch &a) {
  const MsmLayout l = msm_layout(g);
  void *slot[3];
  for (int s : {1, 2, 0}) ZK_CK(zk_scratch(ctx, s, l.slot_bytes[s], &slot[s]));
  for (int i = 0; i < MSM_ARRAYS; ++i) a.p[i] = (char *)slot[l.at[i].slot] + l.at[i].off;
  return ZKFHE_OK;
}

int sort_one_pass(zkfhe_ctx *ctx, const MsmGeometry &g, const MsmScratch &a, const Fr *scalars, size_t col_stride) {
  const unsigned gc = std::min(zk_blocks(g.n_cols * g.K1, 256), (unsigned)ctx->num_cu * 8);
  k_msm_clear<<<gc, 256, 0, ctx->stream>>>(a.at(HIST), g.n_cols * g.K1, a.at(HEAVY_COUNT));
  ZK_LAUNCH_CHECK(ctx);
  const unsigned chunks_per_col = (unsigned)((g.n + SORT_CHUNK - 1) / SORT_CHUNK);
  const unsigned grid = (unsigned)(g.n_cols * chunks_per_col);
  const size_t sort_lds = (size_t)g.K1 * sizeof(unsigned);
  if (sort_lds > 48 * 1024) {
    ZK_CK(zk_func_max_lds(ctx, (const void *)k_msm_hist, 160 * 1024));
    ZK_CK(zk_func_max_lds(ctx, (const void *)k_msm_scatter, 160 * 1024));
  }
  k_msm_hist<<<grid, SORT_THREADS, sort_lds, ctx->stream>>>(scalars, col_stride, g.n, chunks_per_col, g.c, g.W, a.at(HIST), g.K1);
  ZK_LAUNCH_CHECK(ctx);
  k_msm_scan<<<(unsigned)g.n_cols, 256, 0, ctx->stream>>>(a.at(HIST), a.at(OFF), a.at(CURSOR), g.K1);
  ZK_LAUNCH_CHECK(ctx);
  k_msm_scatter<<<grid, SORT_THREADS, sort_lds, ctx->stream>>>(scalars, col_stride, g.n, chunks_per_col, g.c, g.W, a.at(CURSOR), g.K1, a.at(ENTRIES), g.col_entries);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

// see k_msm_chist (msm_sort.hip.hpp)
int sort_two_level(zkfhe_ctx *ctx, const MsmGeometry &g, const MsmScratch &a, const Fr *scalars, size_t col_stride) {
  k_msm_clear<<<zk_blocks(g.n_cols * g.NB, 256), 256, 0, ctx->stream>>>(a.at(CHIST), g.n_cols * g.NB, a.at(HEAVY_COUNT));
  ZK_LAUNCH_CHECK(ctx);
  const unsigned ch_chunks = (unsigned)((g.n + CH_SCALARS - 1) / CH_SCALARS), cs_chunks = (unsigned)((g.n + CS_SCALARS - 1) / CS_SCALARS);
  k_msm_chist<<<(unsigned)(g.n_cols * ch_chunks), CS_THREADS, g.NB * sizeof(unsigned), ctx->stream>>>(scalars, col_stride, g.n, ch_chunks, g.c, g.W, g.L, g.NB, a.at(CHIST));
  ZK_LAUNCH_CHECK(ctx);
  k_msm_cscan<<<zk_blocks(g.n_cols, 64), 64, 0, ctx->stream>>>(a.at(CHIST), g.NB, g.n_cols, a.at(COFF), a.at(CCURSOR));
  ZK_LAUNCH_CHECK(ctx);
  const size_t cs_lds = ((size_t)3 * g.NB + (size_t)CS_SCALARS * g.W) * sizeof(unsigned);
  if (cs_lds > 48 * 1024) ZK_CK(zk_func_max_lds(ctx, (const void *)k_msm_cscatter, 64 * 1024));
  k_msm_cscatter<<<(unsigned)(g.n_cols * cs_chunks), CS_THREADS, cs_lds, ctx->stream>>>(scalars, col_stride, g.n, cs_chunks, g.c, g.W, g.L, g.NB, a.at(CCURSOR), a.at(STAGE),
                                                                                         g.stage_stride);
  ZK_LAUNCH_CHECK(ctx);
  ZK_CK(zk_func_max_lds(ctx, (const void *)k_msm_fine, (int)(FINE_TILE * sizeof(unsigned))));
  k_msm_fine<<<(unsigned)(g.n_cols * g.NB), FINE_THREADS, FINE_TILE * sizeof(unsigned), ctx->stream>>>(a.at(COFF), g.NB, g.L, a.at(STAGE), g.stage_stride, g.col_entries, g.K1,
                                                                                                        a.at(OFF), a.at(ENTRIES));
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

int task_list(zkfhe_ctx *ctx, const MsmGeometry &g, const MsmScratch &a) {
  k_msm_task_count<<<(unsigned)g.n_cols, 256, 0, ctx->stream>>>(a.at(OFF), g.K, g.TASK_E, a.at(COL_HIST));
  ZK_LAUNCH_CHECK(ctx);
  k_msm_task_colscan<<<1, 128, 0, ctx->stream>>>(a.at(COL_HIST), (unsigned)g.n_cols, a.at(COL_BASE), a.at(N_TASKS));
  ZK_LAUNCH_CHECK(ctx);
  k_msm_task_fill<<<(unsigned)g.n_cols, 256, 0, ctx->stream>>>(a.at(OFF), g.K, g.TASK_E, a.at(COL_BASE), a.at(BUCKET_POS_A), a.at(BUCKET_POS_B), a.at<uint2>(TASKS),
                                                               a.at(HEAVY_COUNT), a.at(MEDIUM_LIST), a.at(LARGE_LIST), (unsigned)g.heavy_cap);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

int accumulate_and_merge(zkfhe_ctx *ctx, const MsmGeometry &g, const MsmScratch &a, const G1Affine *table) {
  const unsigned K = g.K, cap = (unsigned)ctx->num_cu * 32;
  const unsigned gridt = std::min(zk_blocks(g.max_tasks, 256), cap);
  zk_prof_begin(ctx);
  k_msm_accumulate<<<gridt, 256, 0, ctx->stream>>>(a.at<uint2>(TASKS), a.at(N_TASKS), a.at(OFF), a.at(ENTRIES), g.col_entries, table, K, g.TASK_E, a.at<G1X>(PARTIALS));
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, 0, 96.0 * (double)g.n * (double)g.n_cols);
  if (ctx->prof_on) {  // mixed additions of this launch = sorted entries = off[col][K] summed over the columns
    std::vector<unsigned> tot(g.n_cols);
    ZK_HIP(ctx, hipMemcpy2D(tot.data(), sizeof(unsigned), a.at(OFF) + K, (size_t)g.K1 * sizeof(unsigned), sizeof(unsigned), g.n_cols, hipMemcpyDeviceToHost));
    for (unsigned t : tot) ctx->prof_ops[0] += (double)t;
  }
  // light buckets: one thread each; medium: a wave per eight buckets; large: a wave per bucket -- three block ranges of one launch
  const unsigned gridb = std::min(zk_blocks((size_t)K * g.n_cols, 256), cap);
  const unsigned gridm = (unsigned)std::min<size_t>((g.heavy_cap / 8 + 3) / 4, 512), gridl = (unsigned)std::min<size_t>((g.heavy_cap + 3) / 4, 512);
  k_msm_merge<<<gridl + gridm + gridb, 256, 0, ctx->stream>>>(a.at(OFF), a.at(BUCKET_POS_A), a.at(BUCKET_POS_B), a.at<G1X>(PARTIALS), K, g.TASK_E, g.n_cols,
                                                              a.at<G1X>(BUCKETS), a.at(HEAVY_COUNT), a.at(MEDIUM_LIST), a.at(LARGE_LIST), (unsigned)g.heavy_cap, gridl, gridm);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

int reduce_buckets(zkfhe_ctx *ctx, const MsmGeometry &g, const MsmScratch &a, void *out, bool xyzz) {
  const unsigned K = g.K, A = K >> 6;
  const size_t n_cols = g.n_cols;
  if (K > 32768) return zk_fail_msg(ctx, ZKFHE_EINVAL, "MSM basis with more than 32768 buckets (window_bits > 16) is not supported");
  if (K < 64) {
    (xyzz ? k_msm_small<true> : k_msm_small<false>)<<<(unsigned)n_cols, 64, 0, ctx->stream>>>(a.at<G1X>(BUCKETS), K, out);
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  }
  // outputs w0 .. w0 + cnt - 1 of every column, L lanes per sum
  auto marginals = [&](unsigned L, unsigned w0, unsigned cnt) {
    const size_t waves = (n_cols * cnt + 64 / L - 1) / (64 / L);
    k_msm_marginals<<<zk_blocks(waves * 64, 256), 256, 0, ctx->stream>>>(a.at<G1X>(BUCKETS), K, n_cols, L, w0, cnt, a.at<G1X>(MARG));
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  };
  // row sums (64 buckets each) and column sums (A buckets each).  Few columns: whole-wave butterflies (shortest chain);
  // many: 8 lanes per sum (1.4 lane-additions per bucket) -- except column sums over more than 64 rows, whose serial
  // part would be A / 8 additions deep
  const unsigned Lr = n_cols <= 16 ? 64 : 8;
  const unsigned Lc = (n_cols <= 16 || A > 64) ? 64 : 8;
  if (Lr == Lc) {   // rows and columns side by side in one launch
    ZK_CK(marginals(Lr, 0, A + 64));
  } else {
    ZK_CK(marginals(Lr, 0, A));
    ZK_CK(marginals(Lc, A, 64));
  }
  (xyzz ? k_msm_weighted<true> : k_msm_weighted<false>)<<<(unsigned)n_cols, 64 * ((A + 63) / 64 + 1), 0, ctx->stream>>>(a.at<G1X>(MARG), K, out);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

// a basis' device tables and the basis itself; hipFree waits for the device
void basis_free(zkfhe_basis *b) {
  if (!b) return;
  (void)hipFree(b->table), (void)hipFree(b->mult);
  delete b;
}

// with_table: also a digit-multiple table, as wide as budget and device allow
int basis_fill(zkfhe_ctx *ctx, const zkfhe_g1_affine *bases_host, bool with_table, double table_budget_scale, zkfhe_basis *b) {
  const size_t n = b->n;
  hipError_t e = hipMalloc((void **)&b->table, (size_t)b->windows * n * sizeof(G1Affine));
  if (e != hipSuccess) return zk_fail(ctx, e == hipErrorOutOfMemory ? ZKFHE_ENOMEM : ZKFHE_EHIP, "hipMalloc(basis table)", e, __FILE__, __LINE__);
  void *tmp;
  ZK_CK(zk_scratch(ctx, 0, n * sizeof(G1Affine), &tmp));
  ZK_HIP(ctx, zk_memcpy_async(ctx, tmp, bases_host, n * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
  k_basis_table<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>((const G1Affine *)tmp, n, b->c, b->windows, b->table);
  ZK_LAUNCH_CHECK(ctx);
  int mc = with_table && n >= 256 ? table_bits(n, table_budget_scale) : 0;
  // a digit-multiple table (k_msm_table): every call against this basis becomes a plain sum of table points.  It is an
  // accelerator, not a requirement: on a device that does not have the room (other tenants, many SRS alive) the width drops
  // until it fits, and without any table the calls take the bucket pipeline
  const int mc_budget = mc;
  bool narrowed = false;
  for (; mc >= 8; --mc) {
    const int mw = (255 + mc - 1) / mc;
    const size_t bytes = (n * (size_t)mw << (mc - 1)) * sizeof(G1Affine);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + table_reserve_bytes(total_b)) {
      narrowed = true;   // the device does not have the room right now (other keys, other tenants): the next narrower width
      continue;
    }
    e = hipMalloc((void **)&b->mult, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      b->mult = nullptr;
      narrowed = true;
      continue;
    }
    b->mc = mc, b->mw = mw, b->mult_bytes = bytes;
    k_basis_multiples<<<zk_blocks(n * (size_t)mw, 64), 64, 0, ctx->stream>>>((const G1Affine *)tmp, n, mc, mw, b->mult);
    ZK_LAUNCH_CHECK(ctx);
    break;
  }
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  b->narrowed = narrowed && b->mc < mc_budget;
  if (getenv("ZKFHE_VERBOSE"))
    fprintf(stderr, "[zkfhe] basis n = %zu: digit-multiple table %d bits, %.1f GB resident%s\n", n, b->mc, (double)b->mult_bytes / 1073741824.0,
            b->narrowed ? " (narrower than the budget allows: the device did not have the room)" : (b->mc ? "" : " (none: bucket pipeline)"));
  return ZKFHE_OK;
}

int msm_sparse_form(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_sparse_term *terms_dev, size_t n_terms, size_t n_slots, void *out_dev, bool xyzz) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, basis != nullptr && basis->mult != nullptr && terms_dev != nullptr && out_dev != nullptr && n_slots > 0 && n_slots <= 65535 && n_terms <= 4096);
  (xyzz ? k_msm_sparse<true> : k_msm_sparse<false>)<<<(unsigned)n_slots, 64, 0, ctx->stream>>>(terms_dev, (unsigned)n_terms, basis->mult, basis->mc, basis->mw,
                                                                                          table_bias(basis->mc, basis->mw), out_dev);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

}  // namespace

// table_budget_scale: share of the per-basis table budget this basis may use (srs.hip: the monomial half of an SRS gets half)
int zk_basis_create_scaled(zkfhe_ctx *ctx, const zkfhe_g1_affine *bases_host, size_t n, int window_bits, double table_budget_scale, zkfhe_basis **out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, out != nullptr && bases_host != nullptr && n > 0);
  ZK_ARG(ctx, window_bits == 0 || (window_bits >= 2 && window_bits <= 16));
  const int c = window_bits ? window_bits : default_window_bits(n);
  const int windows = (254 + c - 1) / c;
  ZK_ARG(ctx, (size_t)windows * n < ((size_t)1 << 31));
  zkfhe_basis *b = new zkfhe_basis();
  b->n = n, b->c = c, b->windows = windows;
  const int rc = basis_fill(ctx, bases_host, window_bits == 0, table_budget_scale, b);
  if (rc) {
    basis_free(b);
    return rc;
  }
  *out = b;
  return ZKFHE_OK;
}

// Column c of the call holds its basis->n scalars at scalars_dev + c * col_stride: col_stride > n selects a row range of longer
// columns (the point-range shard of one rank, comm.hip) without copying it out.
int zk_msm_batch_strided(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_fr *scalars_dev, size_t col_stride, size_t n_cols, zkfhe_g1_affine *out_dev) {
  return zk_msm_batch_strided_form(ctx, basis, scalars_dev, col_stride, n_cols, out_dev, false);
}

// out_dev: n_cols affine points (64 B each) or, with xyzz, n_cols accumulator-form sums (zkfhe_g1_xyzz, 128 B each)
int zk_msm_batch_strided_form(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_fr *scalars_dev, size_t col_stride, size_t n_cols, void *out_dev, bool xyzz) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, basis != nullptr);
  if (!n_cols) return ZKFHE_OK;
  ZK_ARG(ctx, scalars_dev != nullptr && out_dev != nullptr && col_stride >= basis->n);
  ZK_ARG(ctx, n_cols <= MSM_MAX_COLS);
  const Fr *scalars = (const Fr *)scalars_dev;
  // the table path for wide calls by table_wide's rule, and always for calls of a few columns, where the pipeline's thirteen
  // dependent launches are the cost
  if (basis->mult && (table_wide(basis) || n_cols <= 8)) return msm_table(ctx, basis, scalars, col_stride, n_cols, out_dev, xyzz);
  // ZKFHE_SORT is read per call: tests switch the sort inside one process
  const MsmGeometry g = msm_geometry(basis->n, basis->c, basis->windows, n_cols, msm_sort_mode(getenv("ZKFHE_SORT")));
  MsmScratch a;
  ZK_CK(msm_scratch(ctx, g, a));
  ZK_CK(g.two_level ? sort_two_level(ctx, g, a, scalars, col_stride) : sort_one_pass(ctx, g, a, scalars, col_stride));
  ZK_CK(task_list(ctx, g, a));
  ZK_CK(accumulate_and_merge(ctx, g, a, basis->table));
  return reduce_buckets(ctx, g, a, out_dev, xyzz);
}

extern "C" {

int zkfhe_basis_create(zkfhe_ctx *ctx, const zkfhe_g1_affine *bases_host, size_t n, int window_bits, zkfhe_basis **out) {
  return zk_basis_create_scaled(ctx, bases_host, n, window_bits, 1.0, out);
}

int zkfhe_basis_destroy(zkfhe_ctx *ctx, zkfhe_basis *basis) {
  ZK_ENTER(ctx);
  if (!basis) return ZKFHE_OK;
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  basis_free(basis);
  return ZKFHE_OK;
}

size_t zkfhe_basis_len(const zkfhe_basis *basis) { return basis ? basis->n : 0; }

int zkfhe_msm_batch(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_fr *scalars_dev, size_t n_cols, zkfhe_g1_affine *out_dev) {
  return zk_msm_batch_strided(ctx, basis, scalars_dev, basis ? basis->n : 0, n_cols, out_dev);
}

// The same sums left in the accumulator form (XYZZ, 128 B each, x = X / ZZ, y = Y / ZZZ, identity ZZ = 0): the last kernel of the
// call skips its field inversion -- one lane, 40 us, at the end of every call -- and the caller normalises the points of a whole
// Fiat-Shamir round with ONE inversion (zkfhe_g1_xyzz_to_affine, host).  halo2 does the same one level up: `commit_lagrange`
// returns projective points and create_proof batch-normalises a round's commitments.
int zkfhe_msm_batch_xyzz(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_fr *scalars_dev, size_t n_cols, zkfhe_g1_xyzz *out_dev) {
  return zk_msm_batch_strided_form(ctx, basis, scalars_dev, basis ? basis->n : 0, n_cols, out_dev, true);
}

int zkfhe_msm_sparse(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_sparse_term *terms_dev, size_t n_terms, size_t n_slots, zkfhe_g1_affine *out_dev) {
  return msm_sparse_form(ctx, basis, terms_dev, n_terms, n_slots, out_dev, false);
}
int zkfhe_msm_sparse_xyzz(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_sparse_term *terms_dev, size_t n_terms, size_t n_slots, zkfhe_g1_xyzz *out_dev) {
  return msm_sparse_form(ctx, basis, terms_dev, n_terms, n_slots, out_dev, true);
}

// Accumulator-form sums -> affine points, on the host: Montgomery's trick over the ZZZ of the whole array (3 products per point and
// ONE Bernstein-Yang inversion), then x = X (ZZ / ZZZ)^2, y = Y / ZZZ; ZZ = 0 -> the identity (0, 0).  In and out are raw Montgomery
// coordinates (what the kernels store and zkfhe_msm_batch returns).  in == out element-wise aliasing is not supported.
int zkfhe_g1_xyzz_to_affine(const zkfhe_g1_xyzz *in, size_t n, zkfhe_g1_affine *out) {
  if ((!in || !out) && n) return ZKFHE_EINVAL;
  g1x_normalize_batch((const G1X *)in, n, (G1Affine *)out);
  return ZKFHE_OK;
}

int zkfhe_basis_has_multiples(const zkfhe_basis *basis) { return basis && basis->mult ? 1 : 0; }

int zkfhe_basis_table_bits(const zkfhe_basis *basis, int *wide_calls) {
  if (wide_calls) *wide_calls = basis && basis->mult && table_wide(basis) ? 1 : 0;
  return basis && basis->mult ? basis->mc : 0;
}

// bytes of the basis' digit-multiple table resident in HBM; *narrowed (optional) = 1 when the table is narrower than the budget
// would have allowed because the device did not have the room when the basis was made
size_t zkfhe_basis_table_bytes(const zkfhe_basis *basis, int *narrowed) {
  if (narrowed) *narrowed = basis && basis->narrowed ? 1 : 0;
  return basis ? basis->mult_bytes : 0;
}

int zkfhe_g1_add(zkfhe_ctx *ctx, const zkfhe_g1_affine *a, const zkfhe_g1_affine *b, zkfhe_g1_affine *out, size_t n) {
  ZK_ENTER(ctx);
  if (!n) return ZKFHE_OK;
  k_g1_add<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>((const G1Affine *)a, (const G1Affine *)b, (G1Affine *)out, n);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

int zkfhe_g1_mul(zkfhe_ctx *ctx, const zkfhe_g1_affine *p, const zkfhe_fr *k, zkfhe_g1_affine *out, size_t n) {
  ZK_ENTER(ctx);
  if (!n) return ZKFHE_OK;
  k_g1_mul<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>((const G1Affine *)p, (const Fr *)k, (G1Affine *)out, n);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

}  // extern "C"
