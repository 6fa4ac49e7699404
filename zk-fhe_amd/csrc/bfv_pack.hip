// Ring packing on the GPU (zkfhe.h "Ring packing", INTEGRATION.md "Opening chosen coefficients: ring packing"): one chosen
// coefficient of each of n ciphertexts moved into one ciphertext, everything else erased, with Galois key switches, additions and
// products by a monomial only.  Conventions of bfv_galois.hip: N residues in [0, Q) per polynomial, CircuitInput order (position
// N - 1 - d holds degree d).
//
// Degree d of x^k v is degree j = d - k mod 2N of v if j < N, else minus degree j - N (mono_coeff): a gather whose addresses depend on
// k (public) only.  v nu with nu = N^-1 mod Q is log2(N) exact halvings mod the odd Q (v even: v / 2, else (v + Q) / 2), each the
// canonical residue of v 2^-1, so the result is the canonical residue of v nu.
//   k_pack_prepare   one launch: w_(group, i) = nu x^(2N - pos) a_(group, i) for the leaves of the launch, zeros for the padding
//   k_key_switch     the key switch of bfv_key_switch.hip on the digits of sigma_g(e1 - x^s o1), read straight from the two operands
//                    (SrcPack; no odd operand: sigma_g(e1), a trace level); digit-parallel (k_key_switch_digit, k_key_switch_fold)
//                    where the key is resident and the level has at most zk_bfv_wide_max pairs
//   k_pack_finish    Garner over the five primes, x mod Q, as k_eval_epilogue EV_GALOIS; the same thread adds (e0 + x^s o0) +
//                    sigma_g(e0 - x^s o0) on component 0 and e1 + x^s o1 on component 1.  Out of place: a level reads sigma-permuted
//                    positions of its operands, so levels go back and forth between two work arrays.  With the keys of a hybrid
//                    set k_pack_finish<true> puts floor((2 x + P) / 2P) mod Q where x mod Q stands.
// Every sum is a sum mod Q of canonical residues, so the order of the additions of a level does not matter: a level is bit for bit
// (w_i + t) + zkfhe_bfv_apply_galois(w_i - t, g) with t = x^s w_(i+h).
// zk_bfv_pack_run serves the host-array call and the batch call.  Work arrays hold at most chunk_polys(N) ciphertexts.  Groups whose
// n' leaves fit go through the levels together, as many groups as fit.  A group of more leaves is reduced subtree by subtree: the
// leaves with equal index mod R = n' / C (C = chunk_polys(N)) form a subtree whose levels 1 ... log2 C use the s and g of the global
// levels; the subtrees are visited in bit-reversed order of that index, so the roots that meet at the next level arrive one after
// the other and a stack of at most log2 R pending roots suffices.  No kernel uses scratch; none branches on or addresses by a
// coefficient's value.
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;

// One thread per coefficient of out ([2][groups m][N]): leaf j < m of group grp is input leaf0 + j leaf_stride of that group, read
// at polynomial grp src_gstride + src_off + j src_jstride of src[comp]; an input past n is padding.  pos: [groups][n] or null.
__global__ __launch_bounds__(256) void k_pack_prepare(const uint64_t *__restrict__ src0, const uint64_t *__restrict__ src1, size_t src_gstride,
                                                      size_t src_off, size_t src_jstride, const uint64_t *__restrict__ pos, size_t n_in,
                                                      size_t leaf0, size_t leaf_stride, size_t m, size_t total, int log_n, uint64_t q,
                                                      uint64_t *__restrict__ out0, uint64_t *__restrict__ out1) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * total) return;
  const unsigned n = 1u << log_n;
  const size_t comp = g >= total, r = g - comp * total, poly = r >> log_n, grp = poly / m, j = poly % m, leaf = leaf0 + j * leaf_stride;
  const unsigned d = (unsigned)(r & (n - 1));
  uint64_t v = 0;
  if (leaf < n_in) {
    const unsigned k = (2 * n - (unsigned)(pos ? pos[grp * n_in + leaf] : 0)) & (2 * n - 1);
    v = mono_coeff((comp ? src1 : src0) + (grp * src_gstride + src_off + j * src_jstride) * n, d, k, n, q);
    for (int i = 0; i < log_n; ++i) v = (v >> 1) + ((v & 1) ? (q >> 1) + 1 : 0);   // v / 2 mod the odd q: (v + q) / 2 for an odd v
  }
  (comp ? out1 : out0)[poly * n + (n - 1 - d)] = v;
}

// One thread per coefficient of res ([2][c][NP][N], total = 2 c N): pair k of component comp goes to polynomial k of out[comp].
// HYB: the key switch of a hybrid key set, divided by its special modulus sp
template <bool HYB>
__global__ __launch_bounds__(256) void k_pack_finish(const uint32_t *__restrict__ res, PackOps op, unsigned s, size_t c, size_t total, int log_n,
                                                     uint64_t q, Crt5 cc, unsigned ginv, uint64_t *__restrict__ out0, uint64_t *__restrict__ out1,
                                                     uint64_t sp) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const unsigned n = 1u << log_n, d = (unsigned)(g & (n - 1));
  const size_t poly = g >> log_n, comp = poly >= c, k = poly - comp * c, at = op.at(k);
  uint64_t m[3];
  bool neg;
  crt5(res + poly * NP * n + d, n, cc, m, neg);
  uint64_t v = HYB ? crt5_div_p_mod_q(m, neg, sp, q) : crt5_mod_q(m, neg, q);   // the key switch mod Q
  const uint64_t *e = op.e[comp] + at * n, *o = op.o[comp] ? op.o[comp] + at * n : nullptr;
  uint64_t sum = e[n - 1 - d];
  if (o) sum = add_q(sum, mono_coeff(o, d, s, n, q), q);
  v = add_q(v, sum, q);
  if (!comp) v = add_q(v, pack_src(e, o, d, ginv, s, n, q), q);
  (comp ? out1 : out0)[k * n + (n - 1 - d)] = v;
}

// One thread per coefficient of out ([c][N]): out = x^k a with k = ks[0] (shared) or ks[polynomial]
__global__ __launch_bounds__(256) void k_pack_monomial(const uint64_t *__restrict__ a, const uint64_t *__restrict__ ks, int shared, size_t total,
                                                       int log_n, uint64_t q, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const unsigned n = 1u << log_n, d = (unsigned)(g & (n - 1));
  const size_t poly = g >> log_n;
  const unsigned k = (unsigned)ks[shared ? 0 : poly] & (2 * n - 1);
  out[poly * n + (n - 1 - d)] = mono_coeff(a + poly * n, d, k, n, q);
}

// ------------------------------------------------------------------------------------------------------------------ host side

unsigned bitrev(unsigned k, int bits) {
  unsigned r = 0;
  for (int i = 0; i < bits; ++i) r |= ((k >> i) & 1) << (bits - 1 - i);
  return r;
}

// what a level needs beside its operands
struct PackCtx {
  KeySwitch ks;
  const KeySource *key;
  uint32_t *acc;
};

// level lv (pack: op.o set; trace: null) over c pairs into out0, out1 ([c][N] each)
int pack_level(zkfhe_ctx *ctx, const PackCtx &pc, int lv, const PackOps &op, size_t c, uint64_t *out0, uint64_t *out1) {
  const int log_n = pc.ks.log_n;
  const uint64_t n = (uint64_t)1 << log_n;
  const unsigned s = (unsigned)(n >> lv), ginv = (unsigned)pow_mod(((uint64_t)1 << lv) + 1, n - 1, 2 * n);   // the units mod 2N have order N
  const SrcPack sp{op, s, ginv};
  const double src = sp.bytes();
  ZK_CK(zk_bfv_key_switch(ctx, pc.ks, sp, pc.key->hat(lv - 1), c, pc.acc));
  const size_t total = 2 * c * n;
  zk_prof_begin(ctx);
  const uint64_t special = pc.key->special;
  if (special != 1)
    k_pack_finish<true><<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(pc.acc, op, s, c, total, log_n, pc.ks.q, crt5_const(), ginv, out0, out1, special);
  else
    k_pack_finish<false><<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(pc.acc, op, s, c, total, log_n, pc.ks.q, crt5_const(), ginv, out0, out1, special);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_PACK, (double)total * (NP * 4 + 8 + src) + (double)c * n * src);
  return ZKFHE_OK;
}

// two work arrays of cap ciphertexts each, [c0 | c1] with the planes cap N words apart
struct PingPong {
  uint64_t *buf[2];
  size_t plane;
  int cur = 0;
  uint64_t *in(int comp) const { return buf[cur] + comp * plane; }
  uint64_t *out(int comp) const { return buf[cur ^ 1] + comp * plane; }
};

}  // namespace

namespace zkrns {

int zk_bfv_monomial_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, size_t k_count, const uint64_t *k,
                        const Planes &out) {
  const uint64_t n = prm->n, q = prm->q;
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(count, chunk_polys(n)), cw = chunk * n;
  const bool shared = k_count == 1;
  uint64_t *a_d = nullptr, *k_d, *o_d;
  Arena ar;
  a.stage(ar, a_d, cw);
  ZK_CK(ar.add(k_d, shared ? 1 : chunk).add(o_d, cw).carve(ctx));
  if (shared) ZK_CK(zkfhe_upload(ctx, k_d, k, 8));
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t c = std::min(chunk, count - lo);
    if (!shared) ZK_CK(zkfhe_upload(ctx, k_d, k + lo, c * 8));
    for (int comp = 0; comp < 2; ++comp) {
      const uint64_t *x;
      ZK_CK(a.at(ctx, comp, lo, c, n, a_d, &x));
      zk_prof_begin(ctx);
      k_pack_monomial<<<zk_blocks(c * n, 256), 256, 0, ctx->stream>>>(x, k_d, shared, c * n, log_n, q, o_d);
      ZK_LAUNCH_CHECK(ctx);
      zk_prof_end(ctx, ZKFHE_PROF_BFV_PACK, (double)c * n * 16);
      ZK_CK(out.out(ctx, comp, lo, c, n, o_d));
    }
  }
  return out.done(ctx);
}

int zk_bfv_pack_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t n_groups, size_t n, const Planes &a, const uint64_t *pos, KeySource key,
                    int l, int base_bits, const Planes &out) {
  const uint64_t N = prm->n, q = prm->q;
  const int log_n = bit_log2(N);
  size_t np = 1;   // n', the leaves of a group
  while (np < n) np <<= 1;
  const int L = bit_log2(np);
  const size_t cap = chunk_polys(N);   // a power of two
  const bool split = np > cap;         // a group's leaves do not fit the work arrays: subtrees of cap leaves
  const size_t C = split ? cap : np, gb = split ? 1 : std::min(n_groups, cap / np);
  const int log_c = bit_log2(C), depth = L - log_c;   // R = 2^depth subtrees per group
  const size_t held = gb * C, pairs = std::max(held / 2, gb), plane = held * N;
  const size_t stage_polys = split ? C : gb * n;
  PackCtx pc{{log_n, l, base_bits, q}, &key, nullptr};
  int *flag = nullptr;
  uint64_t *stage = nullptr, *pos_d = nullptr, *stack = nullptr;
  PingPong w;
  w.plane = plane;
  Arena ar;
  if (!key.resident()) ar.add(flag, 1);   // of the key transform
  key.add(ar, N, l);
  if (!a.dev) ar.add(stage, 2 * stage_polys * N);
  if (pos) ar.add(pos_d, gb * n);
  ar.add(w.buf[0], 2 * plane).add(w.buf[1], 2 * plane).add(pc.acc, 2 * pairs * NP * N);
  pc.ks.add(ar, ctx, key, pairs, true);   // the levels halve: each decides for itself
  if (split) ar.add(stack, (size_t)(depth + 2) * 2 * N);
  ZK_CK(ar.carve(ctx));
  ZK_CK(stage_keys<NP>(ctx, key, N, q, l, flag));

  // k_pack_prepare for gc groups from group g0 on: m leaves each, leaf j the input leaf0 + j leaf_stride, into w.out
  auto prepare = [&](size_t g0, size_t gc, size_t m, size_t leaf0, size_t leaf_stride) -> int {
    const uint64_t *s0, *s1;
    size_t gstride, off, jstride;
    if (a.dev) {
      s0 = a.p[0] + g0 * n * N, s1 = a.p[1] + g0 * n * N, gstride = n, off = leaf0, jstride = leaf_stride;
    } else if (!split) {   // the groups' inputs, contiguous
      for (int comp = 0; comp < 2; ++comp) ZK_CK(a.in(ctx, comp, g0 * n, gc * n, N, stage + comp * stage_polys * N));
      s0 = stage, s1 = stage + stage_polys * N, gstride = n, off = 0, jstride = 1;
    } else {   // one subtree's inputs, leaf by leaf
      for (size_t j = 0; j < m && leaf0 + j * leaf_stride < n; ++j)
        for (int comp = 0; comp < 2; ++comp) ZK_CK(a.in(ctx, comp, g0 * n + leaf0 + j * leaf_stride, 1, N, stage + (comp * stage_polys + j) * N));
      s0 = stage, s1 = stage + stage_polys * N, gstride = 0, off = 0, jstride = 1;
    }
    const size_t total = gc * m * N;
    zk_prof_begin(ctx);
    k_pack_prepare<<<zk_blocks(2 * total, 256), 256, 0, ctx->stream>>>(s0, s1, gstride, off, jstride, pos_d, n, leaf0, leaf_stride, m, total, log_n, q,
                                                                      w.out(0), w.out(1));
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_PACK, (double)total * 32);
    w.cur ^= 1;
    return ZKFHE_OK;
  };
  // pack level lv of gc groups of 2 h entries each in w.in, into dst (null: w.out, which then becomes w.in)
  auto level = [&](int lv, size_t gc, size_t h, uint64_t *dst) -> int {
    const PackOps op{{w.in(0), w.in(1)}, {w.in(0) + h * N, w.in(1) + h * N}, h, 2 * h};
    ZK_CK(pack_level(ctx, pc, lv, op, gc * h, dst ? dst : w.out(0), dst ? dst + N : w.out(1)));
    if (!dst) w.cur ^= 1;
    return ZKFHE_OK;
  };

  for (size_t g0 = 0; g0 < n_groups; g0 += gb) {
    const size_t gc = std::min(gb, n_groups - g0);
    if (pos) ZK_CK(zkfhe_upload(ctx, pos_d, pos + g0 * n, gc * n * 8));
    if (!split) {
      ZK_CK(prepare(g0, gc, np, 0, 1));
      for (int lv = 1; lv <= L; ++lv) ZK_CK(level(lv, gc, np >> lv, nullptr));
      for (int lv = L + 1; lv <= log_n; ++lv) {   // the trace on the gc roots
        const PackOps op{{w.in(0), w.in(1)}, {nullptr, nullptr}, 1, 1};
        ZK_CK(pack_level(ctx, pc, lv, op, gc, w.out(0), w.out(1)));
        w.cur ^= 1;
      }
      ZK_CK(out.out(ctx, 0, g0, gc, N, w.in(0)));
      ZK_CK(out.out(ctx, 1, g0, gc, N, w.in(1)));
      continue;
    }
    // one group, subtree by subtree: slot i of the stack is [c0 | c1] at stack + i 2 N; `pending` holds (slot, rank) of the roots
    // that wait for their partner, rank k a root of level log_c + k
    std::vector<int> free_slots;
    for (int i = depth + 1; i >= 0; --i) free_slots.push_back(i);
    std::vector<std::pair<int, int>> pending;
    auto slot = [&](int i) { return stack + (size_t)i * 2 * N; };
    for (unsigned t = 0; t < (1u << depth); ++t) {
      ZK_CK(prepare(g0, 1, C, bitrev(t, depth), (size_t)1 << depth));
      int top = free_slots.back();
      free_slots.pop_back();
      for (int lv = 1; lv <= log_c; ++lv) ZK_CK(level(lv, 1, C >> lv, lv == log_c ? slot(top) : nullptr));
      pending.push_back({top, 0});
      while (pending.size() >= 2 && pending[pending.size() - 2].second == pending.back().second) {
        const std::pair<int, int> o = pending.back(), e = pending[pending.size() - 2];   // the earlier root has the lower index
        const int dst = free_slots.back();
        free_slots.pop_back();
        const PackOps op{{slot(e.first), slot(e.first) + N}, {slot(o.first), slot(o.first) + N}, 1, 1};
        ZK_CK(pack_level(ctx, pc, log_c + e.second + 1, op, 1, slot(dst), slot(dst) + N));
        pending.pop_back(), pending.pop_back();
        free_slots.push_back(e.first), free_slots.push_back(o.first);
        pending.push_back({dst, e.second + 1});
      }
    }
    int root = pending.back().first;   // the one root of level L
    for (int lv = L + 1; lv <= log_n; ++lv) {
      const int dst = free_slots.back();
      const PackOps op{{slot(root), slot(root) + N}, {nullptr, nullptr}, 1, 1};
      ZK_CK(pack_level(ctx, pc, lv, op, 1, slot(dst), slot(dst) + N));
      free_slots.back() = root;
      root = dst;
    }
    ZK_CK(out.out(ctx, 0, g0, 1, N, slot(root)));
    ZK_CK(out.out(ctx, 1, g0, 1, N, slot(root) + N));
  }
  return out.done(ctx);
}

void pack_elements(uint64_t n, uint64_t *g) {
  for (int lv = 1; lv <= bit_log2(n); ++lv) g[lv - 1] = ((uint64_t)1 << lv) + 1;
}

int check_pack(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, const int *base_bits, int *l, size_t n_groups, size_t n, const uint64_t *pos,
               const char *fn) {
  if (!(prm->q & 1)) return refuse(ctx, fn, "Q must be odd");
  if (base_bits) ZK_CK(relin_rows(ctx, prm, *base_bits, fn, l));
  if (n > prm->n) return refuse(ctx, fn, "n = " + std::to_string(n) + " is above N");
  bool bad = false;
  for (size_t i = 0; pos && i < n_groups * n; ++i) bad |= pos[i] >= prm->n;
  if (bad) return refuse(ctx, fn, "a position is not below N");
  return ZKFHE_OK;
}

int check_monomial(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, size_t k_count, const uint64_t *k, const char *fn) {
  if (k_count != 1 && k_count != count) return refuse(ctx, fn, "k_count must be 1 or the ciphertext count");
  bool bad = false;
  for (size_t i = 0; i < k_count; ++i) bad |= k[i] >= 2 * prm->n;
  if (bad) return refuse(ctx, fn, "an exponent k is not below 2N");
  return ZKFHE_OK;
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_pack_elements(const zkfhe_bfv_params *params, uint64_t *g, size_t *count) {
  if (!count) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_pack_elements: count is NULL");
  ZK_CK(check_params(nullptr, params));
  *count = (size_t)bit_log2(params->n);
  if (g) pack_elements(params->n, g);
  return ZKFHE_OK;
}

int zkfhe_bfv_mul_monomial(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, size_t k_count,
                           const uint64_t *k, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_mul_monomial";
  if (!(ctx && params && c0 && c1 && k && out0 && out1 && n > 0)) return refuse(ctx, fn, "a NULL argument or a zero count");
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_monomial(ctx, params, n, k_count, k, fn));
  ZK_CK(check_below_q(ctx, c0, n * params->n, params->q, fn, "a ciphertext", c1));
  return zk_bfv_monomial_run(ctx, params, n, host_planes(c0, c1), k_count, k, host_planes(out0, out1));
}

int zkfhe_bfv_pack(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n, const uint64_t *c0, const uint64_t *c1,
                   const uint64_t *pos, const uint64_t *gk0, const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_pack";
  if (!(ctx && params && c0 && c1 && gk0 && gk1 && out0 && out1 && n_groups > 0 && n > 0)) return refuse(ctx, fn, "a NULL argument or a zero count");
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(check_pack(ctx, params, &base_bits, &l, n_groups, n, pos, fn));
  const uint64_t N = params->n, q = params->q;
  const size_t keys = (size_t)bit_log2(N);
  ZK_CK(check_below_q(ctx, c0, n_groups * n * N, q, fn, "a ciphertext", c1));
  ZK_CK(check_below_q(ctx, gk0, keys * l * N, q, fn, "a Galois-key", gk1));
  return zk_bfv_pack_run(ctx, params, n_groups, n, host_planes(c0, c1), pos, host_keys(gk0, gk1, keys), l, base_bits, host_planes(out0, out1));
}

}  // extern "C"
