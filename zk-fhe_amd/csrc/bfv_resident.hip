// Resident ciphertext batches (zkfhe.h "Resident ciphertext batches", INTEGRATION.md "Chaining calls on the device"): n BFV
// ciphertexts kept on the device between calls, and the evaluation calls on them.  A batch is one device allocation of its own,
// two planes c0[n][N] | c1[n][N] of uint64_t in CircuitInput order.
//
// The invariant: every word of a batch is a residue below Q from creation to destruction.  alloc writes zeros; upload and store
// check on the device (k_cts_check) before a word becomes part of a batch; every evaluation call writes what a kernel of the
// host-array call computed mod Q from residues below Q; select, sum and box_tally copy or add residues mod Q.  So no call on a batch
// runs a range pass over ciphertexts: only the host arrays of a call (plaintexts, keys, indices, groups) are checked, on the host.
//
// An evaluation call here is its argument checks and one call of the runner of the host-array call (bfv_host.hpp:
// zk_bfv_add_run, zk_bfv_plain_run, zk_bfv_mul_run, zk_bfv_galois_run, zk_bfv_dot_core, zk_bfv_plan_run_dev, zk_bfv_monomial_run,
// zk_bfv_pack_run) on the batch's planes:
// one chunk loop per operation, so the chunk rule, the kernels, their order and their profiling slots are those of that call.  A
// runner reads a chunk from the batch (or from a contiguous copy in the work arena where a kernel wants one), writes its result to
// the work arena, and copies it into dst afterwards on the same stream: a chunk is read completely before it is written, and dst may
// be a source.  No call allocates or frees device memory apart from alloc, upload and destroy.
// The calls that take a resident key set (bfv_evk.hip: mul_evk, apply_galois_evk, slot_sum, dot; dot_plain takes none) hand the
// runner the set's transformed keys in place of host rows: no key is checked, uploaded or transformed, and a chunk of at most
// zk_bfv_wide_max ciphertexts takes the digit-parallel key switch, whose partials come from the work arena.
// This file's own kernels are three plain passes over memory, 16 bytes per lane, a capped grid with a grid stride:
//   k_cts_check      any word >= Q raises one flag word
//   k_cts_gather     dst[j] = src[idx[j]], both planes (select; idx == null: j itself, the box's [group][2][N] layout to two planes)
//   k_cts_group_sum  dst[g] = the sum mod Q of the members of group g, each thread walking its group's list for two coefficients
#include <cstring>
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
constexpr int CTS_THREADS = 256;
constexpr unsigned CTS_MAX_BLOCKS = 2048;   // the grid of a pass; the rest is the grid stride
constexpr size_t MAX_GROUPS = 4096;

// pairs 16-byte units of w: flag |= 1 if any of the 2 pairs words is >= q
__global__ __launch_bounds__(CTS_THREADS) void k_cts_check(const ulonglong2 *__restrict__ w, size_t pairs, uint64_t q, int *flag) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * CTS_THREADS + threadIdx.x; i < pairs; i += (size_t)gridDim.x * CTS_THREADS) {
    const ulonglong2 v = w[i];
    bad |= v.x >= q || v.y >= q;
  }
  if (bad) atomicOr(flag, 1);
}

// One 16-byte unit per thread and step: unit u = (plane p, ciphertext j < count, unit k < N / 2) of dst ([2][count][N]) takes
// unit k of plane p of source ciphertext idx[j] (idx == null: j), which lies at src + idx[j] ct_stride + p plane_stride words.
__global__ __launch_bounds__(CTS_THREADS) void k_cts_gather(const uint64_t *__restrict__ src, size_t ct_stride, size_t plane_stride,
                                                            const uint64_t *__restrict__ idx, size_t count, int log_n,
                                                            ulonglong2 *__restrict__ dst) {
  const int lh = log_n - 1;   // log2 of the units of a polynomial
  const size_t per_plane = count << lh, total = 2 * per_plane;
  for (size_t u = (size_t)blockIdx.x * CTS_THREADS + threadIdx.x; u < total; u += (size_t)gridDim.x * CTS_THREADS) {
    const size_t p = u >= per_plane, r = u - p * per_plane, j = r >> lh, k = r & (((size_t)1 << lh) - 1);
    const size_t from = idx ? idx[j] : j;
    dst[u] = ((const ulonglong2 *)(src + from * ct_stride + p * plane_stride))[k];
  }
}

// One 16-byte unit per thread and step: unit u = (plane p, group g < n_groups, unit k < N / 2) of dst ([2][n_groups][N]) is the sum
// mod q of unit k of plane p of the ciphertexts members[off[g]] ... members[off[g + 1] - 1] of src ([2][count][N]); an empty group
// gives zeros.  Consecutive threads read consecutive units of the same member.
__global__ __launch_bounds__(CTS_THREADS) void k_cts_group_sum(const ulonglong2 *__restrict__ src, size_t count, const unsigned *__restrict__ off,
                                                               const unsigned *__restrict__ members, size_t n_groups, int log_n, uint64_t q,
                                                               ulonglong2 *__restrict__ dst) {
  const int lh = log_n - 1;
  const size_t per_plane = n_groups << lh, total = 2 * per_plane;
  for (size_t u = (size_t)blockIdx.x * CTS_THREADS + threadIdx.x; u < total; u += (size_t)gridDim.x * CTS_THREADS) {
    const size_t p = u >= per_plane, r = u - p * per_plane, g = r >> lh, k = r & (((size_t)1 << lh) - 1);
    const ulonglong2 *s = src + ((p * count) << lh) + k;
    const unsigned lo = off[g], hi = off[g + 1];
    ulonglong2 v = make_ulonglong2(0, 0);
#pragma unroll 4
    for (unsigned i = lo; i < hi; ++i) {
      const ulonglong2 x = s[(size_t)members[i] << lh];
      v.x = add_q(v.x, x.x, q), v.y = add_q(v.y, x.y, q);
    }
    dst[u] = v;
  }
}

unsigned pass_blocks(size_t units) { return std::min<unsigned>(CTS_MAX_BLOCKS, std::max<unsigned>(1, zk_blocks(units, CTS_THREADS))); }

}  // namespace

struct zkfhe_bfv_cts {
  zkfhe_bfv_params params{};
  int device = 0;      // of the context that made it
  size_t n = 0;        // ciphertexts
  uint64_t *w = nullptr;   // the allocation: c0[n][N], then c1[n][N]
  uint64_t *plane(int comp) const { return w + comp * n * params.n; }
  Planes planes() const { return device_planes(plane(0), plane(1)); }   // what the runners of the evaluation calls take
};

namespace {

bool same_params(const zkfhe_bfv_params &a, const zkfhe_bfv_params &b) { return a.n == b.n && a.q == b.q && a.t == b.t && a.b == b.b; }

// every batch of a call lives on the context's device
int on_device(zkfhe_ctx *ctx, const char *fn, std::initializer_list<const zkfhe_bfv_cts *> batches) {
  for (const zkfhe_bfv_cts *b : batches)
    if (ctx->device != b->device)
      return refuse(ctx, fn, "the batch lives on device " + std::to_string(b->device) + " and the context on device " + std::to_string(ctx->device));
  return ZKFHE_OK;
}

// the sources and the destination of a call share their parameters
int alike(zkfhe_ctx *ctx, const char *fn, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b) {
  if (!same_params(a->params, b->params)) return refuse(ctx, fn, "the batches have different parameters");
  return ZKFHE_OK;
}

int same_count(zkfhe_ctx *ctx, const char *fn, size_t have, size_t want, const char *what) {
  if (have != want) return refuse(ctx, fn, std::string(what) + " holds " + std::to_string(have) + " ciphertexts and the call needs " + std::to_string(want));
  return ZKFHE_OK;
}

void cts_free(zkfhe_bfv_cts *b) {
  if (!b) return;
  (void)hipFree(b->w);   // waits for the device
  delete b;
}

// a batch of n ciphertexts with its allocation, the words not yet written
int cts_new(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const char *fn, zkfhe_bfv_cts **out) {
  ZK_CK(check_params(ctx, params));
  if (n >> 31) return refuse(ctx, fn, "more than 2^31 ciphertexts");
  zkfhe_bfv_cts *b = new zkfhe_bfv_cts;
  b->params = *params, b->device = ctx->device, b->n = n;
  const hipError_t e = hipMalloc(&b->w, 2 * n * params->n * 8);   // < 2^31 2^15 2^4
  if (e != hipSuccess) {
    delete b;
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return zk_fail_msg(ctx, ZKFHE_ENOMEM, std::string(fn) + ": out of device memory");
    }
    ZK_HIP(ctx, e);
  }
  *out = b;
  return ZKFHE_OK;
}

// k_cts_check over words words at w (16-byte aligned, an even count) into flag
int launch_check(zkfhe_ctx *ctx, const uint64_t *w, size_t words, uint64_t q, int *flag) {
  zk_prof_begin(ctx);
  k_cts_check<<<pass_blocks(words / 2), CTS_THREADS, 0, ctx->stream>>>((const ulonglong2 *)w, words / 2, q, flag);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_RESIDENT, (double)words * 8);
  return ZKFHE_OK;
}

int launch_gather(zkfhe_ctx *ctx, const uint64_t *src, size_t ct_stride, size_t plane_stride, const uint64_t *idx_d, size_t count, int log_n,
                  uint64_t *dst) {
  const size_t units = count << log_n;   // 2 planes of count N / 2 units
  zk_prof_begin(ctx);
  k_cts_gather<<<pass_blocks(units), CTS_THREADS, 0, ctx->stream>>>(src, ct_stride, plane_stride, idx_d, count, log_n, (ulonglong2 *)dst);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_RESIDENT, (double)units * 32);
  return ZKFHE_OK;
}

// count ciphertexts of two host planes into two device planes, in chunks
int upload_planes(zkfhe_ctx *ctx, uint64_t n, size_t count, const uint64_t *c0, const uint64_t *c1, uint64_t *d0, uint64_t *d1) {
  const size_t chunk = std::min<size_t>(count, chunk_polys(n));
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t bytes = std::min(chunk, count - lo) * n * 8;
    ZK_CK(zkfhe_upload(ctx, d0 + lo * n, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, d1 + lo * n, c1 + lo * n, bytes));
  }
  return ZKFHE_OK;
}

int read_flag(zkfhe_ctx *ctx, const int *flag, int *bad) { return zkfhe_download(ctx, bad, flag, 4); }

// the checked upload behind upload: the planes into the new batch, one pass over its words, the flag read once
int upload_fill(zkfhe_ctx *ctx, zkfhe_bfv_cts *b, const uint64_t *c0, const uint64_t *c1, const char *fn) {
  const uint64_t n = b->params.n;
  int *flag;
  ZK_CK(Arena().add(flag, 1).carve(ctx));
  ZK_HIP(ctx, zk_memset_async(ctx, flag, 0, 4, ctx->stream));
  ZK_CK(upload_planes(ctx, n, b->n, c0, c1, b->plane(0), b->plane(1)));
  ZK_CK(launch_check(ctx, b->w, 2 * b->n * n, b->params.q, flag));
  int bad = 0;
  ZK_CK(read_flag(ctx, flag, &bad));
  if (bad) return refuse(ctx, fn, "a ciphertext coefficient >= Q");
  return ZKFHE_OK;
}

// what every evaluation call starts with: its name, the context's device selected, the batches on it
#define CTS_CALL(name)                 \
  ZK_ENTER(ctx);                       \
  const char *fn = "bfv_cts_" name

int null_arg(zkfhe_ctx *ctx, const char *fn) { return refuse(ctx, fn, "a NULL argument or a zero count"); }

// add_plain and mul_plain: the plaintext rules of the host-array calls
int plain_args(zkfhe_ctx *ctx, const char *fn, const zkfhe_bfv_cts *a, size_t m_count, const uint64_t *m, const zkfhe_bfv_cts *dst) {
  if (!(ctx && a && m && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, dst}));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  if (m_count != 1 && m_count != a->n) return refuse(ctx, fn, "m_count must be 1 or the ciphertext count");
  return check_plain(ctx, m, m_count * a->params.n, a->params.q, a->params.t, fn);
}

// a call that takes a key set: the set on the context's device, with the batch's parameters
int evk_args(zkfhe_ctx *ctx, const char *fn, const zkfhe_bfv_evk *evk, const zkfhe_bfv_cts *a, EvkView *view) {
  zk_bfv_evk_view(evk, view);
  if (ctx->device != view->device)
    return refuse(ctx, fn, "the key set lives on device " + std::to_string(view->device) + " and the context on device " + std::to_string(ctx->device));
  if (!same_params(view->params, a->params)) return refuse(ctx, fn, "the key set and the batch have different parameters");
  return ZKFHE_OK;
}

int need_relin(zkfhe_ctx *ctx, const char *fn, const EvkView &view) {
  if (!view.rlk_hat) return refuse(ctx, fn, "the key set has no relinearization key");
  return ZKFHE_OK;
}

int need_galois(zkfhe_ctx *ctx, const char *fn, const zkfhe_bfv_evk *evk, uint64_t g, const uint32_t **key_hat) {
  *key_hat = zk_bfv_evk_galois(evk, g);
  if (!*key_hat) return refuse(ctx, fn, "the key set has no key for the Galois element " + std::to_string(g));
  return ZKFHE_OK;
}

// dot and dot_plain on batches: the shapes, then the core on the planes
int dot_args(zkfhe_ctx *ctx, const char *fn, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, size_t n_terms, const zkfhe_bfv_cts *dst) {
  const size_t want = n_terms >> 31 ? ~(size_t)0 : dst->n * n_terms;   // counts are below 2^31: the product fits
  ZK_CK(same_count(ctx, fn, a->n, want, "a"));
  if (b && b->n != n_terms) ZK_CK(same_count(ctx, fn, b->n, want, "b"));
  if (dst == a || dst == b) return refuse(ctx, fn, "dst must not be a source");
  return ZKFHE_OK;
}

}  // namespace

extern "C" {

int zkfhe_bfv_cts_alloc(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, zkfhe_bfv_cts **out) {
  CTS_CALL("alloc");
  if (out) *out = nullptr;
  if (!(ctx && params && out && n > 0)) return null_arg(ctx, fn);
  zkfhe_bfv_cts *b = nullptr;
  ZK_CK(cts_new(ctx, params, n, fn, &b));
  hipError_t e = zk_memset_async(ctx, b->w, 0, 2 * n * params->n * 8, ctx->stream);
  if (e == hipSuccess) e = zk_wait(ctx);
  if (e != hipSuccess) {
    cts_free(b);
    ZK_HIP(ctx, e);
  }
  *out = b;
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_upload(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, zkfhe_bfv_cts **out) {
  CTS_CALL("upload");
  if (out) *out = nullptr;
  if (!(ctx && params && c0 && c1 && out && n > 0)) return null_arg(ctx, fn);
  zkfhe_bfv_cts *b = nullptr;
  ZK_CK(cts_new(ctx, params, n, fn, &b));
  const int rc = upload_fill(ctx, b, c0, c1, fn);
  if (rc) {
    cts_free(b);
    return rc;
  }
  *out = b;
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_store(zkfhe_ctx *ctx, zkfhe_bfv_cts *cts, size_t first, size_t count, const uint64_t *c0, const uint64_t *c1) {
  CTS_CALL("store");
  if (!(ctx && cts && c0 && c1 && count > 0)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {cts}));
  if (first > cts->n || count > cts->n - first) return refuse(ctx, fn, "the range is not inside the batch");
  // Stage and check every chunk before the batch is touched; the flag is read once.  A single chunk is then copied from its stage,
  // more chunks are uploaded again, straight into the batch.
  const uint64_t n = cts->params.n;
  const size_t chunk = std::min<size_t>(count, chunk_polys(n)), cw = chunk * n;
  int *flag;
  uint64_t *stage;
  ZK_CK(Arena().add(flag, 1).add(stage, 2 * cw).carve(ctx));
  ZK_HIP(ctx, zk_memset_async(ctx, flag, 0, 4, ctx->stream));
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t c = std::min(chunk, count - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, stage, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, stage + c * n, c1 + lo * n, bytes));
    ZK_CK(launch_check(ctx, stage, 2 * c * n, cts->params.q, flag));
  }
  int bad = 0;
  ZK_CK(read_flag(ctx, flag, &bad));
  if (bad) return refuse(ctx, fn, "a ciphertext coefficient >= Q");
  if (count == chunk) {
    ZK_CK(zk_copy_d2d(ctx, cts->plane(0) + first * n, stage, cw * 8));
    ZK_CK(zk_copy_d2d(ctx, cts->plane(1) + first * n, stage + cw, cw * 8));
  } else {
    ZK_CK(upload_planes(ctx, n, count, c0, c1, cts->plane(0) + first * n, cts->plane(1) + first * n));
  }
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_download(zkfhe_ctx *ctx, const zkfhe_bfv_cts *cts, size_t first, size_t count, uint64_t *out0, uint64_t *out1) {
  CTS_CALL("download");
  if (!(ctx && cts && out0 && out1 && count > 0)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {cts}));
  if (first > cts->n || count > cts->n - first) return refuse(ctx, fn, "the range is not inside the batch");
  const uint64_t n = cts->params.n;
  const size_t chunk = std::min<size_t>(count, chunk_polys(n));
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t bytes = std::min(chunk, count - lo) * n * 8;
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, cts->plane(0) + (first + lo) * n, bytes));
    ZK_CK(zkfhe_download(ctx, out1 + lo * n, cts->plane(1) + (first + lo) * n, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_info(const zkfhe_bfv_cts *cts, zkfhe_bfv_params *params, size_t *n, uint64_t *device_bytes) {
  if (!cts) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_cts_info: cts is NULL");
  if (params) *params = cts->params;
  if (n) *n = cts->n;
  if (device_bytes) *device_bytes = (uint64_t)16 * cts->n * cts->params.n;
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_destroy(zkfhe_ctx *ctx, zkfhe_bfv_cts *cts) {
  ZK_ENTER(ctx);
  if (!cts) return ZKFHE_OK;
  if (ctx) ZK_HIP(ctx, zk_wait(ctx));   // what this context has queued against the batch
  cts_free(cts);
  return ZKFHE_OK;
}

int zkfhe_bfv_box_tally_cts(zkfhe_ctx *ctx, const zkfhe_bfv_box *box, zkfhe_bfv_cts *dst, uint64_t *counted) {
  CTS_CALL("box_tally");
  if (!(ctx && box && dst && counted)) return null_arg(ctx, fn);
  zkfhe_bfv_params prm;
  size_t n_groups;
  const uint64_t *acc;
  const unsigned long long *counts;
  ZK_CK(zk_bfv_box_view(ctx, box, &prm, &n_groups, &acc, &counts));
  ZK_CK(on_device(ctx, fn, {dst}));
  if (!same_params(prm, dst->params)) return refuse(ctx, fn, "the box and the batch have different parameters");
  ZK_CK(same_count(ctx, fn, dst->n, n_groups, "dst"));
  const uint64_t n = prm.n;
  // group g of the accumulator: c0 at (2 g) N, c1 at (2 g + 1) N
  ZK_CK(launch_gather(ctx, acc, 2 * n, n, nullptr, n_groups, bit_log2(n), dst->w));
  return zkfhe_download(ctx, counted, counts, n_groups * 8);
}

int zkfhe_bfv_cts_add(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, int subtract, zkfhe_bfv_cts *dst) {
  CTS_CALL("add");
  if (!(ctx && a && b && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, b, dst}));
  ZK_CK(alike(ctx, fn, a, b));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, b->n, a->n, "b"));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  return zk_bfv_add_run(ctx, &a->params, a->n, a->planes(), b->planes(), subtract, dst->planes());
}

int zkfhe_bfv_cts_add_plain(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t m_count, const uint64_t *m, zkfhe_bfv_cts *dst) {
  CTS_CALL("add_plain");
  ZK_CK(plain_args(ctx, fn, a, m_count, m, dst));
  return zk_bfv_plain_run(ctx, &a->params, false, a->n, a->planes(), m_count, m, dst->planes());
}

int zkfhe_bfv_cts_mul_plain(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t m_count, const uint64_t *m, zkfhe_bfv_cts *dst) {
  CTS_CALL("mul_plain");
  ZK_CK(plain_args(ctx, fn, a, m_count, m, dst));
  return zk_bfv_plain_run(ctx, &a->params, true, a->n, a->planes(), m_count, m, dst->planes());
}

int zkfhe_bfv_cts_mul(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, const uint64_t *rlk0, const uint64_t *rlk1, int base_bits,
                      zkfhe_bfv_cts *dst) {
  CTS_CALL("mul");
  if (!(ctx && a && b && rlk0 && rlk1 && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, b, dst}));
  ZK_CK(alike(ctx, fn, a, b));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, b->n, a->n, "b"));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  int l = 0;
  ZK_CK(relin_rows(ctx, &a->params, base_bits, fn, &l));
  ZK_CK(check_below_q(ctx, rlk0, (size_t)l * a->params.n, a->params.q, fn, "a relinearization-key", rlk1));
  return zk_bfv_mul_run(ctx, &a->params, a->n, a->planes(), b->planes(), host_keys(rlk0, rlk1), l, base_bits, dst->planes());
}

int zkfhe_bfv_cts_apply_galois(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, uint64_t g, const uint64_t *gk0, const uint64_t *gk1, int base_bits,
                               zkfhe_bfv_cts *dst) {
  CTS_CALL("apply_galois");
  if (!(ctx && a && gk0 && gk1 && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, dst}));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  const uint64_t n = a->params.n, q = a->params.q;
  ZK_CK(check_g(ctx, n, g, fn));
  int l = 0;
  ZK_CK(relin_rows(ctx, &a->params, base_bits, fn, &l));
  ZK_CK(check_below_q(ctx, gk0, (size_t)l * n, q, fn, "a Galois-key", gk1));
  return zk_bfv_galois_run(ctx, &a->params, a->n, a->planes(), 1, &g, host_keys(gk0, gk1), l, base_bits, false, dst->planes());
}

int zkfhe_bfv_cts_plan_apply(zkfhe_ctx *ctx, const zkfhe_bfv_plan *plan, const zkfhe_bfv_cts *a, zkfhe_bfv_cts *dst) {
  CTS_CALL("plan_apply");
  if (!(ctx && plan && a && dst)) return null_arg(ctx, fn);
  zkfhe_bfv_params prm;
  int device;
  zk_bfv_plan_view(plan, &prm, &device);
  if (ctx->device != device)
    return refuse(ctx, fn, "the plan lives on device " + std::to_string(device) + " and the context on device " + std::to_string(ctx->device));
  ZK_CK(on_device(ctx, fn, {a, dst}));
  if (!same_params(prm, a->params)) return refuse(ctx, fn, "the plan and the batch have different parameters");
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  ZK_CK(zk_bfv_plan_run_dev(ctx, plan, a->n, a->plane(0), a->plane(1), dst->plane(0), dst->plane(1)));
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_select(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t n_idx, const uint64_t *idx, zkfhe_bfv_cts *dst) {
  CTS_CALL("select");
  if (!(ctx && a && idx && dst && n_idx > 0)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, dst}));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, n_idx, "dst"));
  if (dst == a) return refuse(ctx, fn, "dst must not be the source");
  for (size_t j = 0; j < n_idx; ++j)
    if (idx[j] >= a->n) return refuse(ctx, fn, "an index is not below the source's count");
  const uint64_t n = a->params.n;
  uint64_t *idx_d;
  ZK_CK(Arena().add(idx_d, n_idx).carve(ctx));
  ZK_CK(zkfhe_upload(ctx, idx_d, idx, n_idx * 8));
  ZK_CK(launch_gather(ctx, a->w, n, a->n * n, idx_d, n_idx, bit_log2(n), dst->w));
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

int zkfhe_bfv_cts_sum(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const int32_t *group, size_t n_groups, zkfhe_bfv_cts *dst) {
  CTS_CALL("sum");
  if (!(ctx && a && dst)) return null_arg(ctx, fn);
  if (n_groups < 1 || n_groups > MAX_GROUPS) return refuse(ctx, fn, "n_groups must be in [1, 4096]");
  ZK_CK(on_device(ctx, fn, {a, dst}));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, n_groups, "dst"));
  if (dst == a) return refuse(ctx, fn, "dst must not be the source");
  // the member lists: off[g] ... off[g + 1] - 1 index the members of group g, in the order of the batch
  std::vector<unsigned> off(n_groups + 1, 0), members;
  for (size_t j = 0; j < a->n; ++j) {
    const int64_t g = group ? group[j] : 0;
    if (g >= (int64_t)n_groups) return refuse(ctx, fn, "a group is not below n_groups");
    if (g >= 0) ++off[g + 1];
  }
  for (size_t g = 0; g < n_groups; ++g) off[g + 1] += off[g];
  members.resize(std::max<size_t>(1, off[n_groups]));
  std::vector<unsigned> at(off.begin(), off.end() - 1);
  for (size_t j = 0; j < a->n; ++j) {
    const int64_t g = group ? group[j] : 0;
    if (g >= 0) members[at[g]++] = (unsigned)j;
  }
  const uint64_t n = a->params.n;
  const int log_n = bit_log2(n);
  unsigned *off_d, *members_d;
  ZK_CK(Arena().add(off_d, off.size()).add(members_d, members.size()).carve(ctx));
  ZK_CK(zkfhe_upload(ctx, off_d, off.data(), off.size() * 4));
  ZK_CK(zkfhe_upload(ctx, members_d, members.data(), members.size() * 4));
  const size_t units = n_groups << log_n;   // 2 planes of n_groups N / 2 units
  zk_prof_begin(ctx);
  k_cts_group_sum<<<pass_blocks(units), CTS_THREADS, 0, ctx->stream>>>((const ulonglong2 *)a->w, a->n, off_d, members_d, n_groups, log_n, a->params.q,
                                                                     (ulonglong2 *)dst->w);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_RESIDENT, (double)(off[n_groups] + n_groups) * 2 * n * 8);
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

// ---- the calls that take a resident key set (bfv_evk.hip): no key is checked, uploaded or transformed here

int zkfhe_bfv_cts_mul_evk(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst) {
  CTS_CALL("mul_evk");
  if (!(ctx && a && b && evk && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, b, dst}));
  EvkView view;
  ZK_CK(evk_args(ctx, fn, evk, a, &view));
  ZK_CK(alike(ctx, fn, a, b));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, b->n, a->n, "b"));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  ZK_CK(need_relin(ctx, fn, view));
  return zk_bfv_mul_run(ctx, &a->params, a->n, a->planes(), b->planes(), resident_keys(&view.rlk_hat, 1, view.special), view.l, view.base_bits, dst->planes());
}

int zkfhe_bfv_cts_apply_galois_evk(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, uint64_t g, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst) {
  CTS_CALL("apply_galois_evk");
  if (!(ctx && a && evk && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, dst}));
  EvkView view;
  ZK_CK(evk_args(ctx, fn, evk, a, &view));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  ZK_CK(check_g(ctx, a->params.n, g, fn));
  const uint32_t *key;
  ZK_CK(need_galois(ctx, fn, evk, g, &key));
  return zk_bfv_galois_run(ctx, &a->params, a->n, a->planes(), 1, &g, resident_keys(&key, 1, view.special), view.l, view.base_bits, false, dst->planes());
}

int zkfhe_bfv_cts_slot_sum(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst) {
  CTS_CALL("slot_sum");
  if (!(ctx && a && evk && dst)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, dst}));
  EvkView view;
  ZK_CK(evk_args(ctx, fn, evk, a, &view));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  size_t steps = 0;
  ZK_CK(zkfhe_bfv_slot_sum_elements(&a->params, nullptr, &steps));
  std::vector<uint64_t> gs(steps);
  ZK_CK(zkfhe_bfv_slot_sum_elements(&a->params, gs.data(), &steps));
  std::vector<const uint32_t *> keys(steps);
  for (size_t k = 0; k < steps; ++k) ZK_CK(need_galois(ctx, fn, evk, gs[k], &keys[k]));
  return zk_bfv_galois_run(ctx, &a->params, a->n, a->planes(), steps, gs.data(), resident_keys(keys.data(), steps, view.special), view.l, view.base_bits, true,
                           dst->planes());
}

int zkfhe_bfv_cts_dot(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, size_t n_terms, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst) {
  CTS_CALL("dot");
  if (!(ctx && a && b && evk && dst && n_terms > 0)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, b, dst}));
  EvkView view;
  ZK_CK(evk_args(ctx, fn, evk, a, &view));
  ZK_CK(alike(ctx, fn, a, b));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(dot_args(ctx, fn, a, b, n_terms, dst));
  ZK_CK(need_relin(ctx, fn, view));
  ZK_CK(check_dot_terms(ctx, &a->params, false, n_terms, fn));
  const DotIo io{a->planes(), b->planes(), dst->planes(), resident_keys(&view.rlk_hat, 1, view.special)};
  return zk_bfv_dot_core(ctx, &a->params, false, dst->n, n_terms, b->n / n_terms, io, view.l, view.base_bits);
}

// ---- ring packing (bfv_pack.hip): the runners of zkfhe_bfv_mul_monomial and zkfhe_bfv_pack on the batches' planes

int zkfhe_bfv_cts_mul_monomial(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t k_count, const uint64_t *k, zkfhe_bfv_cts *dst) {
  CTS_CALL("mul_monomial");
  if (!(ctx && a && k && dst)) return null_arg(ctx, fn);
  ZK_CK(check_monomial(ctx, &a->params, a->n, k_count, k, fn));
  ZK_CK(on_device(ctx, fn, {a, dst}));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, dst->n, a->n, "dst"));
  return zk_bfv_monomial_run(ctx, &a->params, a->n, a->planes(), k_count, k, dst->planes());
}

int zkfhe_bfv_cts_pack(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t n, const uint64_t *pos, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst) {
  CTS_CALL("pack");
  if (!(ctx && a && evk && dst && n > 0)) return null_arg(ctx, fn);
  ZK_CK(check_pack(ctx, &a->params, nullptr, nullptr, dst->n, n, pos, fn));
  ZK_CK(on_device(ctx, fn, {a, dst}));
  EvkView view;
  ZK_CK(evk_args(ctx, fn, evk, a, &view));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(same_count(ctx, fn, a->n, dst->n * n, "a"));   // n <= N and counts are below 2^31: the product fits
  if (dst == a) return refuse(ctx, fn, "dst must not be a source");
  std::vector<uint64_t> gs((size_t)bit_log2(a->params.n));
  pack_elements(a->params.n, gs.data());
  std::vector<const uint32_t *> keys(gs.size());
  for (size_t i = 0; i < gs.size(); ++i) ZK_CK(need_galois(ctx, fn, evk, gs[i], &keys[i]));
  return zk_bfv_pack_run(ctx, &a->params, dst->n, n, a->planes(), pos, resident_keys(keys.data(), keys.size(), view.special), view.l, view.base_bits, dst->planes());
}

int zkfhe_bfv_cts_dot_plain(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t n_terms, size_t m_groups, const uint64_t *m, zkfhe_bfv_cts *dst) {
  CTS_CALL("dot_plain");
  if (!(ctx && a && m && dst && n_terms > 0)) return null_arg(ctx, fn);
  ZK_CK(on_device(ctx, fn, {a, dst}));
  ZK_CK(alike(ctx, fn, a, dst));
  ZK_CK(dot_args(ctx, fn, a, nullptr, n_terms, dst));
  if (m_groups != 1 && m_groups != dst->n) return refuse(ctx, fn, "m_groups must be 1 or n_groups");
  ZK_CK(check_dot_terms(ctx, &a->params, true, n_terms, fn));
  const uint64_t n = a->params.n;
  ZK_CK(check_plain(ctx, m, m_groups * n_terms * n, a->params.q, a->params.t, fn));
  const DotIo io{a->planes(), host_planes(m, nullptr), dst->planes(), KeySource{}};   // the plaintexts are the call's one host operand
  return zk_bfv_dot_core(ctx, &a->params, true, dst->n, n_terms, m_groups, io, 0, 0);
}

}  // extern "C"
