// zkfhe_bfv_verify_batch behind its argument checks: randomisers, public-key prefix groups, then per chunk of BATCH_CHUNK proofs
// one device pass (decompress the words, replay on host threads, segment lists, two segmented MSMs), and one pairing for the
// whole batch.  The only verifier unit that calls the device (csrc/verify.hip).
#include "verify_batch.hpp"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <thread>

#include "shplonk.hpp"

namespace zkhost {
namespace {
using zk::Fr;

// CPUs this process may run on: its affinity mask, capped by OMP_NUM_THREADS when set (never the machine's count)
unsigned usable_cpus() {
  unsigned n = 1;
  cpu_set_t cs;
  CPU_ZERO(&cs);
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) n = (unsigned)CPU_COUNT(&cs);
  if (const char *e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0 && (unsigned)v < n) n = (unsigned)v;
  }
  return n;
}
// f(i) for i < n on up to usable_cpus() threads; f must not throw
template <class F>
void parallel_for(size_t n, const F &f) {
  const size_t T = std::min<size_t>(usable_cpus(), n);
  if (T <= 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (size_t t = 0; t < T; ++t)
    th.emplace_back([&] {
      for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    });
  for (auto &x : th) x.join();
}
// Public-key prefix of the BFV instance column: pk0 | pk1, the first 2 N of its 5 N + 1 values (prefix_cache.hpp); 0 otherwise
size_t bfv_key_prefix(size_t n_inst) { return n_inst > 1 && (n_inst - 1) % 5 == 0 ? 2 * ((n_inst - 1) / 5) : 0; }

void put_u64(Blake2b &h, uint64_t v) { h.update(&v, 8); }
// device buffer of one chunk, freed on every path
struct DevBuf {
  zkfhe_ctx *ctx;
  void *p = nullptr;
  explicit DevBuf(zkfhe_ctx *c) : ctx(c) {}
  ~DevBuf() { if (p) zkfhe_dev_free(ctx, p); }
};

#define VB_CK(x) do { const int rc__ = (x); if (rc__) return rc__; } while (0)
const size_t BATCH_CHUNK = 256;   // proofs per device pass: ~30 MB of device memory at k = 13

struct Batch {  // what crosses a step of verify_batch
  zkfhe_ctx *ctx;
  const Vk &vk;
  const SrsG2 &srs;
  std::vector<BatchItem> &items;
  size_t P = 0;                             // instances in the shared public-key prefix
  std::vector<Transcript::State> states;    // per prefix group
  std::vector<zk::G1Affine> vkpts;          // device points [0, NV]: the vk's commitments, then the generator at NV
  size_t NV = 0, PB = 0;                    // PB = NV + 1: first proof word
  zk::G1X A = zk::G1X::identity(), B = zk::G1X::identity();   // sum r_j F_j, sum r_j W_j
  std::vector<size_t> cand;                 // proofs that reach the pairing
};
struct Chunk {  // one device pass over items [c0, c1)
  size_t c0, c1, W = 0;                     // W: words to decompress
  DevBuf buf, tb;                           // [points | compressed words | statuses], [scalars | A,B | indices | offsets]
  std::vector<zk::G1Affine> hpts;
  std::vector<int32_t> hst;
  std::vector<uint32_t> idx, off{0};
  std::vector<Fr> sc;
  std::vector<size_t> seg;                  // surviving proofs, one segment each
  Chunk(zkfhe_ctx *ctx, size_t a, size_t b) : c0(a), c1(b), buf(ctx), tb(ctx) {}
};
// Randomisers: bound to the vk and to every (instances, proof) of the batch, in order
void draw_randomisers(Batch &b) {
  uint8_t D[64];
  Blake2b hd(64, "zkfhe-batch-D");
  for (const BatchItem &it : b.items) {
    put_u64(hd, it.inst.size());
    for (const U256 &v : it.inst) hd.update(v.l, 32);
    put_u64(hd, it.len);
    hd.update(it.proof, it.len);
  }
  hd.digest(D);
  for (size_t j = 0; j < b.items.size(); ++j) {
    Blake2b h(64, "zkfhe-batch-r");
    h.update(b.vk.digest.l, 32);
    h.update(D, 64);
    put_u64(h, j);
    uint8_t d[64];
    h.digest(d);
    U256 r = fe::zero();
    memcpy(r.l, d, 16);   // 128 bits: below r, so already reduced
    if (r.is_zero()) r.l[0] = 1;
    b.items[j].r = mont(r);
  }
}
// Shared public keys: the transcript state after digest | pk0 | pk1, once per key with two proofs or more
void group_public_keys(Batch &b) {
  std::vector<BatchItem> &items = b.items;
  const size_t P = b.P = items.empty() ? 0 : bfv_key_prefix(items[0].inst.size());
  if (!P) return;
  std::map<std::string, int> key;
  std::vector<int> members;
  std::vector<size_t> leader;
  for (size_t j = 0; j < items.size(); ++j) {
    BatchItem &it = items[j];
    if (!it.live || it.inst.size() < P || it.inst.size() > b.vk.cfg.u()) continue;
    std::string k((const char *)it.inst.data(), P * 32);
    auto f = key.find(k);
    if (f == key.end()) {
      f = key.emplace(std::move(k), (int)members.size()).first;
      members.push_back(0);
      leader.push_back(j);
    }
    it.group = f->second;
    members[f->second]++;
  }
  b.states.resize(members.size());
  std::vector<char> ok(members.size(), 0);
  parallel_for(members.size(), [&](size_t g) {
    if (members[g] < 2) return;
    try {
      Transcript t(b.vk.cfg.transcript);
      t.common_scalar(b.vk.digest);
      for (size_t i = 0; i < P; ++i) t.common_scalar(items[leader[g]].inst[i]);
      b.states[g] = t.snapshot();
      ok[g] = 1;
    } catch (...) {
    }
  });
  for (BatchItem &it : items)
    if (it.group >= 0 && !ok[it.group]) it.group = -1;
}
// The vk's commitments and the generator, Montgomery, shared by every segment
void shared_points(Batch &b) {
  for (const AffinePoint &a : b.vk.fixed_commit) b.vkpts.push_back(point_mont(a));
  for (const AffinePoint &a : b.vk.sigma_commit) b.vkpts.push_back(point_mont(a));
  b.vkpts.push_back(point_mont(g1_generator()));
  b.NV = b.vkpts.size() - 1;
  b.PB = b.NV + 1;
}
// Lay the chunk's proof words out behind the shared points and decompress them on the device
int decompress_words(Batch &b, Chunk &ch) {
  const size_t cap_words = proof_words(b.vk.cfg), PB = b.PB;
  for (size_t j = ch.c0; j < ch.c1; ++j) {
    BatchItem &it = b.items[j];
    it.words = it.live ? std::min(it.len / 32, cap_words) : 0;
    it.base = ch.W;
    ch.W += it.words;
  }
  const size_t W = ch.W, n_pts = PB + W + (ch.c1 - ch.c0);   // + one F per proof
  VB_CK(zkfhe_dev_alloc(b.ctx, n_pts * 64 + W * 32 + W * 4 + 64, &ch.buf.p));
  uint8_t *d_pts = (uint8_t *)ch.buf.p, *d_in = d_pts + n_pts * 64, *d_st = d_in + W * 32;
  VB_CK(zkfhe_upload(b.ctx, d_pts, b.vkpts.data(), b.vkpts.size() * 64));
  ch.hpts.resize(W);
  ch.hst.resize(W);
  if (!W) return ZKFHE_OK;
  std::vector<uint8_t> hin(W * 32);
  for (size_t j = ch.c0; j < ch.c1; ++j)
    if (b.items[j].words) memcpy(&hin[b.items[j].base * 32], b.items[j].proof, b.items[j].words * 32);
  VB_CK(zkfhe_upload(b.ctx, d_in, hin.data(), hin.size()));
  VB_CK(zkfhe_g1_decompress(b.ctx, d_in, W, (zkfhe_g1_affine *)(d_pts + PB * 64), (int32_t *)d_st));
  VB_CK(zkfhe_download(b.ctx, ch.hpts.data(), d_pts + PB * 64, W * 64));
  return zkfhe_download(b.ctx, ch.hst.data(), d_st, W * 4);
}
// Transcript replays on host threads, from the decompressed points
void replay(Batch &b, Chunk &ch) {
  parallel_for(ch.c1 - ch.c0, [&](size_t i) {
    BatchItem &it = b.items[ch.c0 + i];
    if (!it.live) return;
    try {
      const Decoded dec{ch.hpts.data() + it.base, ch.hst.data() + it.base, it.words};
      it.op = open_proof(b.vk, it.inst, it.proof, it.len, it.group >= 0 ? &b.states[it.group] : nullptr, b.P, &dec);
      for (const Pt &q : it.op.pts)
        if (q.ref >= (int32_t)it.words) throw std::logic_error("batch verifier: a point outside the decompressed words");
    } catch (const std::exception &e) {
      it.live = false;
      it.why = e.what();
    }
  });
}
// Segments: one per surviving proof (F_j of segment k goes to point FB + k), then sum r_j F_j and sum r_j W_j
void build_segments(Batch &b, Chunk &ch) {
  const size_t PB = b.PB, FB = PB + ch.W;
  for (size_t j = ch.c0; j < ch.c1; ++j) {
    BatchItem &it = b.items[j];
    if (!it.live) continue;
    for (size_t t = 0; t < it.op.pts.size(); ++t) {
      const int32_t ref = it.op.pts[t].ref;
      ch.idx.push_back((uint32_t)(ref >= 0 ? PB + it.base + ref : ref == REF_GEN ? b.NV : REF_VK - ref));
      ch.sc.push_back(it.op.scal[t]);
    }
    ch.off.push_back((uint32_t)ch.idx.size());
    ch.seg.push_back(j);
    it.op.scal.clear();
  }
  const size_t K = ch.seg.size(), T0 = ch.off.back();
  if (!K) return;
  for (size_t k = 0; k < K; ++k) {
    ch.idx.push_back((uint32_t)(FB + k));
    ch.sc.push_back(b.items[ch.seg[k]].r);
  }
  for (size_t k = 0; k < K; ++k) {
    const BatchItem &it = b.items[ch.seg[k]];
    ch.idx.push_back((uint32_t)(PB + it.base + it.op.w.ref));
    ch.sc.push_back(it.r);
  }
  ch.off.push_back((uint32_t)(T0 + K));
  ch.off.push_back((uint32_t)ch.idx.size());
}
// F_j: segments [0, K) over the shared points; then the two weighted sums over the F_j and the proofs' h2 words, added to A, B
int sum_on_device(Batch &b, Chunk &ch) {
  zkfhe_ctx *ctx = b.ctx;
  const size_t K = ch.seg.size(), T = ch.idx.size(), T0 = T - 2 * K, FB = b.PB + ch.W;
  VB_CK(zkfhe_dev_alloc(ctx, T * 4 + T * 32 + ch.off.size() * 4 + 2 * 64 + 256, &ch.tb.p));
  uint8_t *d_pts = (uint8_t *)ch.buf.p, *d_sc = (uint8_t *)ch.tb.p, *d_ab = d_sc + T * 32, *d_idx = d_ab + 128, *d_off = d_idx + ((T * 4 + 63) & ~(size_t)63);
  VB_CK(zkfhe_upload(ctx, d_sc, ch.sc.data(), T * 32));
  VB_CK(zkfhe_upload(ctx, d_idx, ch.idx.data(), T * 4));
  VB_CK(zkfhe_upload(ctx, d_off, ch.off.data(), ch.off.size() * 4));
  VB_CK(zkfhe_msm_segmented(ctx, (const zkfhe_g1_affine *)d_pts, FB, (const uint32_t *)d_idx, (const zkfhe_fr *)d_sc, T0, (const uint32_t *)d_off, K,
                            (zkfhe_g1_affine *)(d_pts + FB * 64)));
  VB_CK(zkfhe_msm_segmented(ctx, (const zkfhe_g1_affine *)d_pts, FB + K, (const uint32_t *)d_idx, (const zkfhe_fr *)d_sc, T, (const uint32_t *)d_off + K, 2,
                            (zkfhe_g1_affine *)d_ab));
  std::vector<zk::G1Affine> F(K), AB(2);
  VB_CK(zkfhe_download(ctx, F.data(), d_pts + FB * 64, K * 64));
  VB_CK(zkfhe_download(ctx, AB.data(), d_ab, 128));
  zk::g1x_add_affine(b.A, AB[0], false);
  zk::g1x_add_affine(b.B, AB[1], false);
  for (size_t k = 0; k < K; ++k) {
    BatchItem &it = b.items[ch.seg[k]];
    it.F = point_canon(F[k]);
    it.W = it.op.w.p;
    it.op = Opening();
    b.cand.push_back(ch.seg[k]);
  }
  return ZKFHE_OK;
}
// One pairing for the whole batch; if it fails, each proof's own check from its F_j, W_j
void final_pairing(Batch &b) {
  if (b.cand.empty()) return;
  if (final_check(point_canon(zk::g1x_to_affine(b.A)), point_canon(zk::g1x_to_affine(b.B)), b.srs)) return;   // every candidate holds
  std::vector<char> ok(b.cand.size(), 0);
  parallel_for(b.cand.size(), [&](size_t i) { ok[i] = final_check(b.items[b.cand[i]].F, b.items[b.cand[i]].W, b.srs) ? 1 : 0; });
  for (size_t i = 0; i < b.cand.size(); ++i) b.items[b.cand[i]].live = ok[i] != 0;
}

}  // namespace

int verify_batch(zkfhe_ctx *ctx, const Vk &vk, const SrsG2 &srs, std::vector<BatchItem> &items) {
  Batch b{ctx, vk, srs, items};
  draw_randomisers(b);
  group_public_keys(b);
  shared_points(b);
  for (size_t c0 = 0; c0 < items.size(); c0 += BATCH_CHUNK) {
    Chunk ch(ctx, c0, std::min(items.size(), c0 + BATCH_CHUNK));
    VB_CK(decompress_words(b, ch));
    replay(b, ch);
    build_segments(b, ch);
    if (!ch.seg.empty()) VB_CK(sum_on_device(b, ch));
  }
  final_pairing(b);
  return ZKFHE_OK;
}

}  // namespace zkhost
