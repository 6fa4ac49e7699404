// The ballot box (zkfhe.h, INTEGRATION.md "From verified proofs to a tally"): sums of BFV ciphertexts taken straight from the public
// inputs of their proofs, and the device-resident box that verifies the proofs first and holds the tally across calls.
// A proof's instances are 5 N + 1 canonical 32-byte scalars pk0 | pk1 | c0 | c1 | cyclo (host/bfv_circuit.hpp); position p of a
// polynomial is word p of the evaluator's arrays (CircuitInput order), so nothing is reordered.
//
// Per chunk of candidate items (those whose count, cyclotomic tail and, in the box, key and proof the host has accepted):
//   1. the c0 | c1 span of every candidate (2 N scalars, 64 N bytes) is packed and uploaded: raw[count][2 N] scalars;
//   2. k_ballot_unpack: one thread per scalar writes its low word to words[2][count][N] and raises flags[item] unless limbs 1 to 3
//      are zero and limb 0 is below Q;
//   3. the host reads the flags, drops what the box has counted before, and counting-sorts the kept items by group: order[] (indices
//      into the chunk), seg_off[] and gid[] per group present, the shape of zkfhe_msm_segmented;
//   4. k_ballot_sum: one thread per (group present, component, coefficient) adds its group's items to acc[n_groups][2][N]; the
//      thread of coefficient 0 of c0 adds the group's item count to counts[n_groups].
// The accumulator and the counts belong to the caller of the kernels: the work arena for zkfhe_bfv_sum_instances, allocations of the
// box's own for zkfhe_bfv_box_add.  Streaming kernels: no LDS, no scratch, every sum an add_q.
#include <cstring>
#include <set>
#include <string>

#include "../host/transcript.hpp"
#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int BALLOT_THREADS = 256;
constexpr size_t BALLOT_CHUNK = 512;     // items per chunk at most: bounds order[], seg_off[] and gid[]
constexpr size_t MAX_GROUPS = 4096;

// One thread per scalar of raw ([count][2 N] scalars of 32 bytes, total = count 2 N): lane i reads the 32 bytes at 32 i as two
// 16-byte loads and stores the low word at words[comp][item][p] (consecutive lanes, consecutive 8-byte words).
__global__ __launch_bounds__(BALLOT_THREADS) void k_ballot_unpack(const uint4 *__restrict__ raw, size_t count, int log_n, uint64_t q,
                                                                  uint64_t *__restrict__ words, unsigned *__restrict__ flags) {
  const size_t g = (size_t)blockIdx.x * BALLOT_THREADS + threadIdx.x;
  if (g >= count << (log_n + 1)) return;
  const size_t n = (size_t)1 << log_n, item = g >> (log_n + 1), comp = (g >> log_n) & 1, p = g & (n - 1);
  const uint4 lo = raw[2 * g], hi = raw[2 * g + 1];
  const uint64_t w = (uint64_t)lo.x | (uint64_t)lo.y << 32;
  words[(comp * count + item) * n + p] = w;
  if ((lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0 || w >= q) atomicOr(flags + item, 1u);
}

// One thread per (group present s < n_present, component, coefficient): the items order[seg_off[s]] ... order[seg_off[s + 1] - 1] of
// words ([2][count][N]) added to acc[gid[s]][comp][p]; counts[gid[s]] grows by the length of the list.
__global__ __launch_bounds__(BALLOT_THREADS) void k_ballot_sum(const uint64_t *__restrict__ words, size_t count, const unsigned *__restrict__ order,
                                                               const unsigned *__restrict__ seg_off, const unsigned *__restrict__ gid,
                                                               size_t n_present, int log_n, uint64_t q, uint64_t *__restrict__ acc,
                                                               unsigned long long *__restrict__ counts) {
  const size_t g = (size_t)blockIdx.x * BALLOT_THREADS + threadIdx.x;
  if (g >= n_present << (log_n + 1)) return;
  const size_t n = (size_t)1 << log_n, s = g >> (log_n + 1), comp = (g >> log_n) & 1, p = g & (n - 1);
  const unsigned lo = seg_off[s], hi = seg_off[s + 1];
  const uint64_t *src = words + comp * count * n + p;
  uint64_t *dst = acc + (((size_t)gid[s] * 2 + comp) << log_n) + p;
  uint64_t v = *dst;
#pragma unroll 4
  for (unsigned k = lo; k < hi; ++k) v = add_q(v, src[(size_t)order[k] * n], q);
  *dst = v;
  if (comp == 0 && p == 0) counts[gid[s]] += hi - lo;
}

// totals[s] += inc[s] for the ZKFHE_BALLOT_STATUSES statuses of the box
__global__ void k_ballot_totals(const unsigned long long *__restrict__ inc, unsigned long long *__restrict__ totals) {
  if (threadIdx.x < ZKFHE_BALLOT_STATUSES) totals[threadIdx.x] += inc[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------ host side

// the N + 1 scalars 1, 0, ..., 0, 1 of x^N + 1
std::vector<uint8_t> cyclo_tail(uint64_t n) {
  std::vector<uint8_t> t((n + 1) * 32, 0);
  t[0] = 1, t[n * 32] = 1;
  return t;
}

// the count and the tail: everything of "is a ciphertext" that the host decides
bool shaped(const uint8_t *inst, size_t n_inst, uint64_t n, const std::vector<uint8_t> &tail) {
  return n_inst == 5 * n + 1 && memcmp(inst + 4 * n * 32, tail.data(), tail.size()) == 0;
}

// Blake2b-256 of the low words of the 2 N scalars of a c0 | c1 span
std::array<uint8_t, 32> span_digest(const uint8_t *span, uint64_t n) {
  zkhost::Blake2b h(32, nullptr);
  uint8_t buf[128];
  for (size_t i = 0; i < 2 * n; i += 16) {   // N >= 8: 2 N is a multiple of 16
    for (int k = 0; k < 16; ++k) memcpy(buf + 8 * k, span + (i + k) * 32, 8);
    h.update(buf, 128);
  }
  std::array<uint8_t, 32> d;
  h.digest(d.data());
  return d;
}

struct Cand {
  size_t j;              // the item
  const uint8_t *span;   // its c0 | c1 scalars
  uint32_t group;        // in [0, n_groups)
};

size_t ballot_chunk(uint64_t n) { return std::min(BALLOT_CHUNK, std::max<size_t>(1, chunk_polys(n) / 2)); }

// the work buffers of one chunk
struct BallotWork {
  unsigned *flags, *order, *seg_off, *gid;
  uint64_t *raw, *words;
};
void add_ballot_work(Arena &a, uint64_t n, size_t n_cands, BallotWork &w) {
  const size_t cap = std::min(ballot_chunk(n), std::max<size_t>(1, n_cands));
  a.add(w.flags, cap).add(w.order, cap).add(w.seg_off, cap + 1).add(w.gid, cap).add(w.raw, cap * 2 * n * 4).add(w.words, cap * 2 * n);
}

// The candidates through the two kernels, chunk by chunk, into acc and counts (device, the caller's).  For every candidate in order:
// status[j] = ZKFHE_BALLOT_NOT_A_CIPHERTEXT if the device flags it, else keep(cand) decides between a status of its own (not summed)
// and ZKFHE_BALLOT_COUNTED.
template <class Keep>
int ballot_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, const std::vector<Cand> &cands, size_t n_groups, const BallotWork &w, uint64_t *acc,
               unsigned long long *counts, int32_t *status, Keep keep) {
  const uint64_t n = prm->n, q = prm->q;
  const int log_n = bit_log2(n);
  const size_t cap = ballot_chunk(n), span_bytes = 2 * n * 32;
  std::vector<uint8_t> hin;
  constexpr unsigned NO_SLOT = ~0u;
  std::vector<unsigned> flags, order, seg_off, gid, at, kept, per(n_groups, 0), slot(n_groups, NO_SLOT);   // per, slot: by group
  for (size_t c0 = 0; c0 < cands.size(); c0 += cap) {
    const size_t count = std::min(cap, cands.size() - c0);
    hin.resize(count * span_bytes);
    for (size_t i = 0; i < count; ++i) memcpy(&hin[i * span_bytes], cands[c0 + i].span, span_bytes);
    ZK_CK(zkfhe_upload(ctx, w.raw, hin.data(), hin.size()));
    ZK_HIP(ctx, zk_memset_async(ctx, w.flags, 0, count * 4, ctx->stream));
    zk_prof_begin(ctx);
    k_ballot_unpack<<<zk_blocks(count * 2 * n, BALLOT_THREADS), BALLOT_THREADS, 0, ctx->stream>>>((const uint4 *)w.raw, count, log_n, q, w.words, w.flags);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_BALLOT, (double)count * 2 * n * (32 + 8));
    flags.resize(count);
    ZK_CK(zkfhe_download(ctx, flags.data(), w.flags, count * 4));
    // the kept items of the chunk, counting-sorted by group
    kept.clear();
    for (size_t i = 0; i < count; ++i) {
      const Cand &c = cands[c0 + i];
      status[c.j] = flags[i] ? ZKFHE_BALLOT_NOT_A_CIPHERTEXT : keep(c);
      if (status[c.j] == ZKFHE_BALLOT_COUNTED) kept.push_back((unsigned)i), ++per[c.group];
    }
    if (kept.empty()) continue;
    gid.clear(), seg_off.assign(1, 0);
    for (unsigned i : kept) {   // a list per group present, in the order of first appearance
      const uint32_t g = cands[c0 + i].group;
      if (slot[g] != NO_SLOT) continue;
      slot[g] = (unsigned)gid.size();
      gid.push_back(g);
      seg_off.push_back(seg_off.back() + per[g]);
    }
    order.resize(kept.size());
    at.assign(seg_off.begin(), seg_off.end() - 1);
    for (unsigned i : kept) order[at[slot[cands[c0 + i].group]]++] = i;
    for (uint32_t g : gid) per[g] = 0, slot[g] = NO_SLOT;
    const size_t n_present = gid.size();
    ZK_CK(zkfhe_upload(ctx, w.order, order.data(), order.size() * 4));
    ZK_CK(zkfhe_upload(ctx, w.seg_off, seg_off.data(), seg_off.size() * 4));
    ZK_CK(zkfhe_upload(ctx, w.gid, gid.data(), n_present * 4));
    zk_prof_begin(ctx);
    k_ballot_sum<<<zk_blocks(n_present * 2 * n, BALLOT_THREADS), BALLOT_THREADS, 0, ctx->stream>>>(w.words, count, w.order, w.seg_off, w.gid, n_present,
                                                                                                  log_n, q, acc, counts);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_BALLOT, (double)(kept.size() + 2 * n_present) * 2 * n * 8);
  }
  return ZKFHE_OK;
}

// acc ([n_groups][2][N]) and counts to the host arrays out0, out1 ([n_groups][N]) and counted, through a bounded host buffer
int ballot_download(zkfhe_ctx *ctx, uint64_t n, size_t n_groups, const uint64_t *acc, const unsigned long long *counts, uint64_t *out0,
                    uint64_t *out1, uint64_t *counted) {
  const size_t step = std::max<size_t>(1, chunk_polys(n) / 2);   // groups per download
  std::vector<uint64_t> tmp(std::min(step, n_groups) * 2 * n);
  for (size_t g0 = 0; g0 < n_groups; g0 += step) {
    const size_t gc = std::min(step, n_groups - g0);
    ZK_CK(zkfhe_download(ctx, tmp.data(), acc + g0 * 2 * n, gc * 2 * n * 8));
    for (size_t g = 0; g < gc; ++g) {
      memcpy(out0 + (g0 + g) * n, &tmp[g * 2 * n], n * 8);
      memcpy(out1 + (g0 + g) * n, &tmp[g * 2 * n + n], n * 8);
    }
  }
  return zkfhe_download(ctx, counted, counts, n_groups * 8);
}

int bad(zkfhe_ctx *ctx, const char *fn, const std::string &what) { return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": " + what); }

}  // namespace

struct zkfhe_bfv_box {
  int device = 0;
  zkfhe_bfv_params params{};
  size_t n_groups = 0;
  std::vector<uint8_t> vk, seed, g2, key;   // key: the 2 N scalars pk0 | pk1; g2: g2 | s_g2 (256 bytes) or empty
  bool has_seed = false;
  std::set<std::array<uint8_t, 32>> seen;   // digests of the ballots counted
  bool broken = false;                      // a device error interrupted the summing of an add
  // device, the box's own: acc[n_groups][2][N], counts[n_groups], totals[ZKFHE_BALLOT_STATUSES]
  uint64_t *acc = nullptr;
  unsigned long long *counts = nullptr, *totals = nullptr;
  uint64_t totals_host[ZKFHE_BALLOT_STATUSES] = {};   // the totals after the last completed add: what zkfhe_bfv_box_info reports
};

namespace {

void box_free(zkfhe_bfv_box *b) {
  if (!b) return;
  (void)hipFree(b->acc), (void)hipFree(b->counts);   // totals: the tail of counts
  delete b;
}

int box_usable(zkfhe_ctx *ctx, const zkfhe_bfv_box *box) {
  if (ctx->device != box->device)
    return bad(ctx, "bfv_box", "the box lives on device " + std::to_string(box->device) + " and the context on device " + std::to_string(ctx->device));
  if (box->broken) return bad(ctx, "bfv_box", "a device error interrupted an earlier add: the tally may be half-applied and the box is closed");
  return ZKFHE_OK;
}

int box_alloc(zkfhe_ctx *ctx, zkfhe_bfv_box *b) {
  const size_t acc_bytes = b->n_groups * 2 * b->params.n * 8, cnt_bytes = (b->n_groups + ZKFHE_BALLOT_STATUSES) * 8;
  hipError_t e = hipMalloc(&b->acc, acc_bytes);
  if (e == hipSuccess) e = hipMalloc(&b->counts, cnt_bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return zk_fail_msg(ctx, ZKFHE_ENOMEM, "bfv_box: out of device memory");
  }
  ZK_HIP(ctx, e);
  b->totals = b->counts + b->n_groups;
  ZK_HIP(ctx, zk_memset_async(ctx, b->acc, 0, acc_bytes, ctx->stream));
  ZK_HIP(ctx, zk_memset_async(ctx, b->counts, 0, cnt_bytes, ctx->stream));
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

// The summing half of an add, on work buffers carved already: the accepted proofs through the kernels, then the totals.  From its
// first command on the box's device state may be half-applied: the caller closes the box if this fails.
int box_sum(zkfhe_ctx *ctx, zkfhe_bfv_box *box, const std::vector<Cand> &cands, size_t n_proofs, const BallotWork &w, unsigned long long *inc,
            int32_t *status) {
  const uint64_t n = box->params.n;
  // A digest enters `seen` when its ballot is kept, before the chunk's k_ballot_sum has run: `seen` and the accumulator agree only
  // if every chunk completes, which is what closing the box on a failure stands for.
  ZK_CK(ballot_run(ctx, &box->params, cands, box->n_groups, w, box->acc, box->counts, status, [&](const Cand &c) {
    return box->seen.insert(span_digest(c.span, n)).second ? ZKFHE_BALLOT_COUNTED : ZKFHE_BALLOT_REPEATED;
  }));
  unsigned long long hist[ZKFHE_BALLOT_STATUSES] = {};
  for (size_t j = 0; j < n_proofs; ++j) ++hist[status[j]];
  ZK_CK(zkfhe_upload(ctx, inc, hist, sizeof(hist)));
  zk_prof_begin(ctx);
  k_ballot_totals<<<1, 64, 0, ctx->stream>>>(inc, box->totals);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_BALLOT, 3.0 * sizeof(hist));
  ZK_HIP(ctx, zk_wait(ctx));
  for (int s = 0; s < ZKFHE_BALLOT_STATUSES; ++s) box->totals_host[s] += hist[s];   // the add is complete
  return ZKFHE_OK;
}

}  // namespace

namespace zkrns {

int zk_bfv_box_view(zkfhe_ctx *ctx, const zkfhe_bfv_box *box, zkfhe_bfv_params *params, size_t *n_groups, const uint64_t **acc,
                    const unsigned long long **counts) {
  ZK_CK(box_usable(ctx, box));
  *params = box->params, *n_groups = box->n_groups, *acc = box->acc, *counts = box->counts;
  return ZKFHE_OK;
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_instances_unpack(const zkfhe_bfv_params *params, const uint8_t *instances, size_t n_instances, uint64_t *pk0, uint64_t *pk1,
                               uint64_t *c0, uint64_t *c1, int32_t *status) {
  const char *fn = "bfv_instances_unpack";
  if (!params || !instances) return bad(nullptr, fn, "a NULL argument");
  ZK_CK(check_params(nullptr, params));
  const uint64_t n = params->n, q = params->q;
  bool ok = shaped(instances, n_instances, n, cyclo_tail(n));
  if (ok) {
    uint64_t high = 0;
    bool big = false;
    for (size_t i = 0; i < 4 * n; ++i) {
      uint64_t l[4];
      memcpy(l, instances + i * 32, 32);
      high |= l[1] | l[2] | l[3];
      big |= l[0] >= q;
    }
    ok = !high && !big;
  }
  if (!ok) {
    if (!status) return bad(nullptr, fn, "the item is not a ciphertext");
    *status = ZKFHE_BALLOT_NOT_A_CIPHERTEXT;
    return ZKFHE_OK;
  }
  uint64_t *out[4] = {pk0, pk1, c0, c1};
  for (int k = 0; k < 4; ++k)
    if (out[k])
      for (size_t p = 0; p < n; ++p) memcpy(out[k] + p, instances + (k * n + p) * 32, 8);
  if (status) *status = ZKFHE_BALLOT_COUNTED;
  return ZKFHE_OK;
}

int zkfhe_bfv_sum_instances(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_items, const uint8_t *const *instances,
                            const size_t *n_instances, const int32_t *group, size_t n_groups, uint64_t *out0, uint64_t *out1,
                            uint64_t *counted, int32_t *status) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_sum_instances";
  if (!(params && instances && n_instances && out0 && out1 && counted && status && n_items > 0)) return bad(ctx, fn, "a NULL argument or a zero count");
  for (size_t j = 0; j < n_items; ++j)
    if (!instances[j] && n_instances[j]) return bad(ctx, fn, "a NULL argument or a zero count");
  if (n_groups < 1 || n_groups > MAX_GROUPS) return bad(ctx, fn, "n_groups must be in [1, 4096]");
  ZK_CK(check_params(ctx, params));
  if (!ctx) return bad(ctx, fn, "ctx is NULL");
  const uint64_t n = params->n;
  const std::vector<uint8_t> tail = cyclo_tail(n);
  std::vector<Cand> cands;
  for (size_t j = 0; j < n_items; ++j) {
    const int64_t g = group ? group[j] : 0;
    if (g < 0)
      status[j] = ZKFHE_BALLOT_SKIPPED;
    else if ((uint64_t)g >= n_groups)
      status[j] = ZKFHE_BALLOT_BAD_GROUP;
    else if (!shaped(instances[j], n_instances[j], n, tail))
      status[j] = ZKFHE_BALLOT_NOT_A_CIPHERTEXT;
    else
      cands.push_back({j, instances[j] + 2 * n * 32, (uint32_t)g});
  }
  BallotWork w;
  uint64_t *acc;
  unsigned long long *counts;
  Arena a;
  add_ballot_work(a, n, cands.size(), w);
  ZK_CK(a.add(acc, n_groups * 2 * n).add(counts, n_groups).carve(ctx));
  ZK_HIP(ctx, zk_memset_async(ctx, acc, 0, n_groups * 2 * n * 8, ctx->stream));
  ZK_HIP(ctx, zk_memset_async(ctx, counts, 0, n_groups * 8, ctx->stream));
  ZK_CK(ballot_run(ctx, params, cands, n_groups, w, acc, counts, status, [](const Cand &) { return ZKFHE_BALLOT_COUNTED; }));
  return ballot_download(ctx, n, n_groups, acc, counts, out0, out1, counted);
}

int zkfhe_bfv_box_create(zkfhe_ctx *ctx, const uint8_t *vk_bytes, size_t vk_len, const zkfhe_bfv_params *params, const uint64_t *pk0,
                         const uint64_t *pk1, size_t n_groups, const uint8_t *srs_seed, size_t seed_len, const uint8_t *g2,
                         const uint8_t *s_g2, zkfhe_bfv_box **out) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_box";
  if (out) *out = nullptr;
  if (!(vk_bytes && vk_len && params && pk0 && pk1 && out)) return bad(ctx, fn, "a NULL argument or a zero count");
  if (n_groups < 1 || n_groups > MAX_GROUPS) return bad(ctx, fn, "n_groups must be in [1, 4096]");
  ZK_CK(check_params(ctx, params));
  if (!g2 != !s_g2 || (!g2 && !srs_seed && seed_len)) return bad(ctx, fn, "give srs_seed, or both g2 and s_g2");
  if (!ctx) return bad(ctx, fn, "ctx is NULL");
  const uint64_t n = params->n;
  ZK_CK(check_below_q(ctx, pk0, n, params->q, fn, "a public-key", pk1));
  zkfhe_bfv_box *b = new zkfhe_bfv_box;
  b->device = ctx->device;
  b->params = *params;
  b->n_groups = n_groups;
  b->vk.assign(vk_bytes, vk_bytes + vk_len);
  if (g2) {
    b->g2.assign(g2, g2 + 128);
    b->g2.insert(b->g2.end(), s_g2, s_g2 + 128);
  } else if (srs_seed) {
    b->seed.assign(srs_seed, srs_seed + seed_len);
    b->has_seed = true;
  }
  b->key.assign(2 * n * 32, 0);
  for (size_t p = 0; p < n; ++p) memcpy(&b->key[p * 32], pk0 + p, 8), memcpy(&b->key[(n + p) * 32], pk1 + p, 8);
  const int rc = box_alloc(ctx, b);
  if (rc) {
    box_free(b);
    return rc;
  }
  *out = b;
  return ZKFHE_OK;
}

int zkfhe_bfv_box_add(zkfhe_ctx *ctx, zkfhe_bfv_box *box, size_t n_proofs, const uint8_t *const *instances, const size_t *n_instances,
                      const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *group, int32_t *status, char *errs,
                      size_t err_stride) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_box";
  if (!(ctx && box && instances && n_instances && proofs && proof_lens && status && n_proofs > 0)) return bad(ctx, fn, "a NULL argument or a zero count");
  for (size_t j = 0; j < n_proofs; ++j)
    if ((!instances[j] && n_instances[j]) || (!proofs[j] && proof_lens[j])) return bad(ctx, fn, "a NULL argument or a zero count");
  ZK_CK(box_usable(ctx, box));
  const uint64_t n = box->params.n;
  const std::vector<uint8_t> tail = cyclo_tail(n);
  if (errs && err_stride)
    for (size_t j = 0; j < n_proofs; ++j) errs[j * err_stride] = 0;
  // 1 to 3 on the host; what is left goes to the verifier
  std::vector<size_t> sent;
  for (size_t j = 0; j < n_proofs; ++j) {
    const int64_t g = group ? group[j] : 0;
    if (g < 0 || (uint64_t)g >= box->n_groups)
      status[j] = ZKFHE_BALLOT_BAD_GROUP;
    else if (!shaped(instances[j], n_instances[j], n, tail))
      status[j] = ZKFHE_BALLOT_NOT_A_CIPHERTEXT;
    else if (memcmp(instances[j], box->key.data(), box->key.size()) != 0)
      status[j] = ZKFHE_BALLOT_WRONG_KEY;
    else
      sent.push_back(j);
  }
  std::vector<Cand> cands;
  if (!sent.empty()) {
    const size_t k = sent.size(), stride = errs && err_stride ? err_stride : 0;
    std::vector<const uint8_t *> v_inst(k), v_proof(k);
    std::vector<size_t> v_n(k), v_len(k);
    std::vector<int> ok(k);
    std::vector<char> v_errs(k * stride + 1);
    for (size_t i = 0; i < k; ++i) v_inst[i] = instances[sent[i]], v_n[i] = n_instances[sent[i]], v_proof[i] = proofs[sent[i]], v_len[i] = proof_lens[sent[i]];
    const int rc = zkfhe_bfv_verify_batch(ctx, box->vk.data(), box->vk.size(), k, v_inst.data(), v_n.data(), v_proof.data(), v_len.data(),
                                          box->has_seed ? box->seed.data() : nullptr, box->seed.size(), box->g2.empty() ? nullptr : box->g2.data(),
                                          box->g2.empty() ? nullptr : box->g2.data() + 128, ok.data(), stride ? v_errs.data() : nullptr, stride);
    // the box is untouched so far; a HIP error has its message already
    if (rc) return rc == ZKFHE_EHIP ? rc : zk_fail_msg(ctx, rc, std::string(fn) + ": zkfhe_bfv_verify_batch failed");
    for (size_t i = 0; i < k; ++i) {
      const size_t j = sent[i];
      if (ok[i]) {
        cands.push_back({j, instances[j] + 2 * n * 32, (uint32_t)(group ? group[j] : 0)});
      } else {
        status[j] = ZKFHE_BALLOT_REJECTED;
        if (stride) memcpy(errs + j * stride, &v_errs[i * stride], stride);
      }
    }
  }
  // 5 to 7: the device check, the digests, the sums; then the totals.  A failed carve leaves the box as it was.
  BallotWork w;
  unsigned long long *inc;
  Arena a;
  add_ballot_work(a, n, cands.size(), w);
  ZK_CK(a.add(inc, ZKFHE_BALLOT_STATUSES).carve(ctx));
  const int rc = box_sum(ctx, box, cands, n_proofs, w, inc, status);
  if (rc) box->broken = true;
  return rc;
}

int zkfhe_bfv_box_tally(zkfhe_ctx *ctx, const zkfhe_bfv_box *box, uint64_t *out0, uint64_t *out1, uint64_t *counted) {
  ZK_ENTER(ctx);
  if (!(ctx && box && out0 && out1 && counted)) return bad(ctx, "bfv_box", "a NULL argument or a zero count");
  ZK_CK(box_usable(ctx, box));
  return ballot_download(ctx, box->params.n, box->n_groups, box->acc, box->counts, out0, out1, counted);
}

int zkfhe_bfv_box_info(const zkfhe_bfv_box *box, zkfhe_bfv_params *params, size_t *n_groups, uint64_t totals[ZKFHE_BALLOT_STATUSES]) {
  if (!box) return bad(nullptr, "bfv_box", "box is NULL");
  if (params) *params = box->params;
  if (n_groups) *n_groups = box->n_groups;
  if (totals)   // the host mirror of the device totals: no device is touched and the thread's current device stays
    for (int s = 0; s < ZKFHE_BALLOT_STATUSES; ++s) totals[s] = box->totals_host[s];
  return ZKFHE_OK;
}

int zkfhe_bfv_box_destroy(zkfhe_ctx *ctx, zkfhe_bfv_box *box) {
  ZK_ENTER(ctx);
  if (!box) return ZKFHE_OK;
  if (ctx) ZK_HIP(ctx, zk_wait(ctx));   // what this context has queued against the box
  box_free(box);
  return ZKFHE_OK;
}

}  // extern "C"
