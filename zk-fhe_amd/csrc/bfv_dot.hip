// Fused BFV inner products on the GPU (zkfhe.h, INTEGRATION.md "Inner products and weighted tallies"): sum_i a_i b_i of relinearized
// ciphertext products with one rescale and one relinearization per sum, and sum_i c_i m_i with public plaintexts m_i.
// Conventions of bfv_enc.hip: host arrays, N residues in [0, Q) per polynomial, CircuitInput order.
//
// Only the forward transforms depend on the term.  The tensor sum_i (a_i (x) b_i) is accumulated pointwise in the transform domain
// over the five primes and leaves it once:
//   1. k_rns_ntt: forward transforms of the a0, a1, b0, b1 of one pass of terms (centred), as bfv_mul lays out its `hat`;
//   2. k_bfv_dot_acc: per (group, prime, index) x0 += a0 b0, x1 += a0 b1 + a1 b0, x2 += a1 b1 over the terms of the pass (PLAIN:
//      x0 += c0 m, x1 += c1 m); the terms of a pass are split into slices over the grid, and k_bfv_dot_fold adds the slices'
//      partial planes and the sum carried from earlier passes into acc[comp][group][prime][N];
//   3. after the last pass k_rns_intt (bfv_linear.hip) once per component, group and prime, then k_eval_epilogue (EV_ROUND), the key
//      switch of bfv_mul on c^2 and k_eval_epilogue (EV_ADD); bfv_dot_plain ends with k_eval_epilogue (EV_MODQ) instead.
// Sizes: |x1| <= n_terms 2 N floor(Q/2)^2 (PLAIN: n_terms N floor(Q/2) floor(T/2)), which zkfhe_bfv_dot_max_terms keeps at or below
// half of the primes' product; the call refuses more terms.  Every value is a residue below p < 2^31, every product a mont_mul and
// every sum an add_p; no step branches on or addresses by a coefficient's value.  No kernel uses scratch.
// Each entry point is a wrapper (the host checks) around zk_bfv_dot_core, the chunk loops on operands that are each host arrays or
// device planes and a key that is host rows or resident (DotIo of Planes and a KeySource, bfv_host.hpp); bfv_resident.hip calls
// the same core on resident batches, with a key set or, for dot_plain, host plaintexts beside the device planes.
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
constexpr int DOT_THREADS = 256;

__device__ __forceinline__ void quad(const uint32_t *__restrict__ p, uint32_t v[4]) {
  const uint4 u = *reinterpret_cast<const uint4 *>(p);   // 16 bytes: planes are N 4 bytes with N >= 8, offsets multiples of 4 words
  v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
}
__device__ __forceinline__ void put_quad(uint32_t *__restrict__ p, const uint32_t v[4]) {
  *reinterpret_cast<uint4 *>(p) = make_uint4(v[0], v[1], v[2], v[3]);
}

// One thread owns 4 consecutive indices of one (group, prime, slice of terms): blockIdx.x = (group * slices + slice) * tiles + tile,
// tiles = ceil(N / 4 / DOT_THREADS), blockIdx.y = prime.  ah0, ah1: the transforms of a0, a1 (PLAIN: c0, c1), [groups][c][NP][N]; bh0, bh1:
// those of b0, b1 (PLAIN: bh0 = m, bh1 unused), [b groups][c][NP][N] with b_stride words between groups (0: one b for every group).
// Slice s sums the terms [s per, min(c, (s + 1) per)) and stores component k of its group at
// out + s slice_stride + (k comp_stride + group) NP N; with carry it adds what is stored there (slices = 1: out is the accumulator).
template <bool PLAIN>
__global__ __launch_bounds__(DOT_THREADS) void k_bfv_dot_acc(const uint32_t *__restrict__ ah0, const uint32_t *__restrict__ ah1,
                                                              const uint32_t *__restrict__ bh0, const uint32_t *__restrict__ bh1, size_t c,
                                                              size_t b_stride, unsigned per, unsigned slices, int log_n, RnsConst<NP> rc,
                                                              int carry, uint32_t *__restrict__ out, size_t comp_stride, size_t slice_stride) {
  constexpr int NC = PLAIN ? 2 : 3;
  const unsigned n = 1u << log_n, quads = n >> 2, tiles = (quads + DOT_THREADS - 1) / DOT_THREADS;
  const unsigned i4 = (blockIdx.x % tiles) * DOT_THREADS + threadIdx.x, j = blockIdx.y;
  if (i4 >= quads) return;   // N = 8: two threads per plane
  const size_t gs = blockIdx.x / tiles, g = gs / slices;
  const unsigned slice = (unsigned)(gs % slices);
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n, at = (size_t)j * n + 4 * (size_t)i4;
  const size_t lo = (size_t)slice * per, hi = lo + per < c ? lo + per : c;
  const uint32_t *A0 = ah0 + (g * c + lo) * plane + at, *A1 = ah1 + (g * c + lo) * plane + at;
  const uint32_t *B0 = bh0 + g * b_stride + lo * plane + at, *B1 = PLAIN ? B0 : bh1 + g * b_stride + lo * plane + at;
  uint32_t x[NC][4];
#pragma unroll
  for (int k = 0; k < NC; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) x[k][e] = 0;
  for (size_t k = lo; k < hi; ++k, A0 += plane, A1 += plane, B0 += plane, B1 += plane) {
    uint32_t a0[4], a1[4], b0[4], b1[4] = {0, 0, 0, 0};
    quad(A0, a0), quad(A1, a1), quad(B0, b0);
    if (!PLAIN) quad(B1, b1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (PLAIN) {
        x[0][e] = add_p(x[0][e], mont_mul(a0[e], b0[e], p, pinv), p);
        x[1][e] = add_p(x[1][e], mont_mul(a1[e], b0[e], p, pinv), p);
      } else {
        x[0][e] = add_p(x[0][e], mont_mul(a0[e], b0[e], p, pinv), p);
        x[1][e] = add_p(x[1][e], add_p(mont_mul(a0[e], b1[e], p, pinv), mont_mul(a1[e], b0[e], p, pinv), p), p);
        x[NC - 1][e] = add_p(x[NC - 1][e], mont_mul(a1[e], b1[e], p, pinv), p);
      }
    }
  }
  uint32_t *o = out + (size_t)slice * slice_stride + g * plane + at;
#pragma unroll
  for (int k = 0; k < NC; ++k, o += comp_stride * plane) {
    if (carry) {
      uint32_t v[4];
      quad(o, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[k][e] = add_p(x[k][e], v[e], p);
    }
    put_quad(o, x[k]);
  }
}

// One thread per 4 consecutive words of the n_comp * groups planes of one prime (blockIdx.y) of a launch of k_bfv_dot_acc with
// slices > 1: acc[(k comp_stride + group) NP N + ...] = (carry ? itself : 0) + the sum over the slices of part
// ([slices][n_comp][groups][NP][N]).
__global__ __launch_bounds__(DOT_THREADS) void k_bfv_dot_fold(const uint32_t *__restrict__ part, unsigned slices, size_t groups, int n_comp,
                                                               int log_n, RnsConst<NP> rc, int carry, uint32_t *__restrict__ acc,
                                                               size_t comp_stride) {
  const unsigned n = 1u << log_n, log_q = log_n - 2, j = blockIdx.y;
  const size_t polys = (size_t)n_comp * groups, f = (size_t)blockIdx.x * DOT_THREADS + threadIdx.x;
  if (f >= polys << log_q) return;
  const size_t poly = f >> log_q, at = (size_t)j * n + 4 * (f & (((size_t)1 << log_q) - 1)), plane = (size_t)NP * n;
  const size_t k = poly / groups, g = poly % groups;
  const uint32_t p = rc.p[j];
  uint32_t *o = acc + (k * comp_stride + g) * plane + at;
  uint32_t x[4] = {0, 0, 0, 0};
  if (carry) quad(o, x);
  const uint32_t *s = part + poly * plane + at;
  for (unsigned i = 0; i < slices; ++i, s += polys * plane) {
    uint32_t v[4];
    quad(s, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = add_p(x[e], v[e], p);
  }
  put_quad(o, x);
}

// ------------------------------------------------------------------------------------------------------------------ host side

typedef unsigned __int128 u128;

// whether n d <= h for d and h of three little-endian limbs
bool fits(uint64_t n, const uint64_t d[3], const uint64_t h[3]) {
  uint64_t r[4];
  u128 a = (u128)n * d[0];
  r[0] = (uint64_t)a;
  a = (u128)n * d[1] + (uint64_t)(a >> 64);
  r[1] = (uint64_t)a;
  a = (u128)n * d[2] + (uint64_t)(a >> 64);
  r[2] = (uint64_t)a, r[3] = (uint64_t)(a >> 64);
  if (r[3]) return false;
  for (int i = 2; i >= 0; --i)
    if (r[i] != h[i]) return r[i] < h[i];
  return true;
}

// the largest n with n * d <= floor(P / 2), saturating at 2^64 - 1; d = 2 N floor(Q/2)^2 or N floor(Q/2) floor(T/2), below 2^141
uint64_t max_terms(const zkfhe_bfv_params *prm, bool plain) {
  const uint64_t hq = prm->q / 2, ht = prm->t / 2;                       // below 2^62
  const u128 m = plain ? (u128)hq * ht : (u128)hq * hq;                  // below 2^124
  const uint64_t f = plain ? prm->n : 2 * prm->n;                        // at most 2^16
  uint64_t d[3];
  u128 a = (u128)(uint64_t)m * f;
  d[0] = (uint64_t)a;
  a = (u128)(uint64_t)(m >> 64) * f + (uint64_t)(a >> 64);
  d[1] = (uint64_t)a, d[2] = (uint64_t)(a >> 64);
  const Crt5 cc = crt5_const();
  uint64_t n = 0;
  for (int bit = 63; bit >= 0; --bit)
    if (fits(n | ((uint64_t)1 << bit), d, cc.H)) n |= (uint64_t)1 << bit;
  return n;
}

// How one call walks its [n_groups][n_terms] operands: passes of c terms; within a pass, sub-chunks of `sub` groups whose c terms
// hold at most chunk_polys(N) polynomials per operand; `gc` groups keep their accumulators on the device at a time.  The terms of a
// launch go in `slices` slices, so that the grid has about two workgroups per CU when the pass has the terms for it.
struct DotPlan {
  size_t c, sub, gc;
  unsigned slices;
};
DotPlan dot_plan(const zkfhe_ctx *ctx, uint64_t n, size_t n_groups, size_t n_terms) {
  DotPlan pl;
  const size_t cp = chunk_polys(n);
  pl.c = std::min(n_terms, cp);
  pl.sub = std::min(n_groups, std::max<size_t>(1, cp / pl.c));
  pl.gc = std::min(n_groups, cp);
  const size_t wg = (size_t)zk_blocks(n / 4, DOT_THREADS) * NP * pl.sub, want = 2 * (size_t)std::max(ctx->num_cu, 1);
  pl.slices = (unsigned)std::min<size_t>(pl.c, std::max<size_t>(1, (want + wg - 1) / wg));
  return pl;
}

// the terms [0, c) of sg groups, accumulated into acc ([n_comp][gc][NP][N]) at groups [s0, s0 + sg)
template <bool PLAIN>
int launch_dot(zkfhe_ctx *ctx, const uint32_t *ah0, const uint32_t *ah1, const uint32_t *bh0, const uint32_t *bh1, size_t c, size_t b_stride,
               size_t sg, unsigned max_slices, int log_n, bool first, uint32_t *part, uint32_t *acc, size_t gc, size_t s0) {
  constexpr int NC = PLAIN ? 2 : 3;
  const size_t n = (size_t)1 << log_n, plane = (size_t)NP * n;
  const unsigned per = (unsigned)((c + max_slices - 1) / max_slices), slices = (unsigned)((c + per - 1) / per);   // no empty slice
  const unsigned tiles = zk_blocks(n / 4, DOT_THREADS);
  const dim3 grid((unsigned)(sg * slices * tiles), NP);
  const RnsConst<NP> rc = rns_const<NP>(log_n);
  uint32_t *dst = acc + s0 * plane;
  const double words = (double)plane * sg;   // one polynomial of every group at every prime
  zk_prof_begin(ctx);
  if (slices == 1)
    k_bfv_dot_acc<PLAIN><<<grid, DOT_THREADS, 0, ctx->stream>>>(ah0, ah1, bh0, bh1, c, b_stride, per, 1, log_n, rc, !first, dst, gc, 0);
  else
    k_bfv_dot_acc<PLAIN><<<grid, DOT_THREADS, 0, ctx->stream>>>(ah0, ah1, bh0, bh1, c, b_stride, per, slices, log_n, rc, 0, part, sg, NC * sg * plane);
  ZK_LAUNCH_CHECK(ctx);
  // read: every operand word of every term (a shared b once per group all the same); written: the sums of every slice
  zk_prof_end(ctx, ZKFHE_PROF_BFV_DOT, 4.0 * words * ((PLAIN ? 3.0 : 4.0) * c + (double)NC * slices + (slices == 1 && !first ? NC : 0)));
  if (slices > 1) {
    zk_prof_begin(ctx);
    k_bfv_dot_fold<<<dim3(zk_blocks(NC * sg * n / 4, DOT_THREADS), NP), DOT_THREADS, 0, ctx->stream>>>(part, slices, sg, NC, log_n, rc, !first, dst, gc);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_DOT, 4.0 * words * NC * (slices + 1.0 + (first ? 0 : 1)));
  }
  return ZKFHE_OK;
}

// both calls behind their checks: PLAIN is bfv_dot_plain (a = c, b0 = m, b1 unused)
template <bool PLAIN>
int dot_core(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n_terms, size_t b_groups, const DotIo &io, int l, int base_bits) {
  constexpr int NC = PLAIN ? 2 : 3, NB = PLAIN ? 1 : 2;   // components of the sum, polynomials of a b operand
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n);
  const size_t plane = (size_t)NP * n;
  const bool shared = b_groups == 1 && n_groups > 1;
  const DotPlan pl = dot_plan(ctx, n, n_groups, n_terms);
  const size_t c_max = pl.c, sub = pl.sub, gc_max = pl.gc;
  const size_t a_polys = 2 * sub * c_max, b_polys = NB * (shared ? 1 : sub) * c_max;
  KeySource key = io.key;
  KeySwitch ks{log_n, l, base_bits, q};
  int *flag;
  uint64_t *in_d, *chat, *o_d;
  uint32_t *hat, *part, *acc;
  Arena ar;
  ar.add(flag, 1);
  if (!PLAIN) key.add(ar, n, l);
  ar.add(in_d, (a_polys + b_polys) * n).add(hat, (a_polys + b_polys) * plane).add(part, pl.slices > 1 ? pl.slices * NC * sub * plane : 0)
      .add(acc, NC * gc_max * plane).add(chat, PLAIN ? 0 : 3 * gc_max * n).add(o_d, 2 * gc_max * n);
  if (!PLAIN) ks.add(ar, ctx, key, gc_max);
  ZK_CK(ar.carve(ctx));
  if (!PLAIN) ZK_CK(stage_keys<NP>(ctx, key, n, q, l, flag));
  for (size_t g0 = 0; g0 < n_groups; g0 += gc_max) {
    const size_t gc = std::min(gc_max, n_groups - g0);
    for (size_t lo = 0; lo < n_terms; lo += c_max) {
      const size_t c = std::min(c_max, n_terms - lo);
      if (shared) {   // one b for every group: fetched and transformed once per pass, behind the a region
        uint64_t *b_d = in_d + a_polys * n;
        ZK_CK(io.b.in(ctx, 0, lo, c, n, b_d));
        if (!PLAIN) ZK_CK(io.b.in(ctx, 1, lo, c, n, b_d + c * n));
        ZK_CK(launch_rns_ntt<NP>(ctx, false, b_d, LOAD_CENTRED, q, NB * c, log_n, nullptr, 0, hat + a_polys * plane, flag));
      }
      for (size_t s0 = 0; s0 < gc; s0 += sub) {
        // sg groups of c terms: one block per operand (sg > 1 only where c = n_terms)
        const size_t sg = std::min(sub, gc - s0), w = sg * c * n, from = (g0 + s0) * n_terms + lo;   // sg c polynomials from `from` on
        const size_t b_at = shared ? a_polys : 2 * sg * c;   // the b region, in polynomials: [a0 | a1 | b0 | b1] when every group has its b
        ZK_CK(io.a.in(ctx, 0, from, sg * c, n, in_d));
        ZK_CK(io.a.in(ctx, 1, from, sg * c, n, in_d + w));
        if (!shared) {   // b_groups = n_groups
          ZK_CK(io.b.in(ctx, 0, from, sg * c, n, in_d + 2 * w));
          if (!PLAIN) ZK_CK(io.b.in(ctx, 1, from, sg * c, n, in_d + 3 * w));
        }
        ZK_CK(launch_rns_ntt<NP>(ctx, false, in_d, LOAD_CENTRED, q, (shared ? 2 : 2 + NB) * sg * c, log_n, nullptr, 0, hat, flag));
        const uint32_t *bh = hat + b_at * plane;
        ZK_CK(launch_dot<PLAIN>(ctx, hat, hat + sg * c * plane, bh, bh + (shared ? 1 : sg) * c * plane, c, shared ? 0 : c * plane, sg, pl.slices,
                                log_n, lo == 0, part, acc, gc, s0));
      }
    }
    ZK_CK(zk_rns_intt(ctx, acc, NC * gc, log_n, rns_const<NP>(log_n)));
    if (PLAIN) {
      ZK_CK(zk_bfv_eval_epilogue(ctx, acc, 2 * gc, log_n, q, EvEpi{}, o_d));
    } else {
      ZK_CK(zk_bfv_eval_epilogue(ctx, acc, 3 * gc, log_n, q, EvEpi{.mode = EV_ROUND, .t = params->t}, chat));
      ZK_CK(zk_bfv_key_switch(ctx, ks, SrcPlain{chat + 2 * gc * n}, key.hat(0), gc, acc));
      ZK_CK(zk_bfv_eval_epilogue(ctx, acc, 2 * gc, log_n, q, EvEpi{.mode = EV_ADD, .add = chat, .p = key.special}, o_d));
    }
    ZK_CK(io.out.out(ctx, 0, g0, gc, n, o_d));
    ZK_CK(io.out.out(ctx, 1, g0, gc, n, o_d + gc * n));
  }
  return io.out.done(ctx);
}

// the host checks of both calls, then the core on the host arrays
template <bool PLAIN>
int dot_call(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n_terms, const uint64_t *a0, const uint64_t *a1,
             size_t b_groups, const uint64_t *b0, const uint64_t *b1, const uint64_t *rlk0, const uint64_t *rlk1, int base_bits, uint64_t *out0,
             uint64_t *out1, const char *fn) {
  ZK_CK(check_params(ctx, params));
  int l = 0;
  if (!PLAIN) ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  if (b_groups != 1 && b_groups != n_groups)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + (PLAIN ? ": m_groups must be 1 or n_groups" : ": b_groups must be 1 or n_groups"));
  ZK_CK(check_dot_terms(ctx, params, PLAIN, n_terms, fn));   // before any O(n) pass and any device work
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, a0, n_groups * n_terms * n, q, fn, "a ciphertext", a1));
  if (PLAIN) {
    ZK_CK(check_plain(ctx, b0, b_groups * n_terms * n, q, params->t, fn));
  } else {
    ZK_CK(check_below_q(ctx, b0, b_groups * n_terms * n, q, fn, "a ciphertext", b1));
    ZK_CK(check_below_q(ctx, rlk0, (size_t)l * n, q, fn, "a relinearization-key", rlk1));
  }
  const DotIo io{host_planes(a0, a1), host_planes(b0, b1), host_planes(out0, out1), host_keys(rlk0, rlk1)};
  return dot_core<PLAIN>(ctx, params, n_groups, n_terms, b_groups, io, l, base_bits);
}

}  // namespace

namespace zkrns {

int check_dot_terms(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, bool plain, size_t n_terms, const char *fn) {
  const uint64_t limit = max_terms(prm, plain);
  if (n_terms > limit)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": n_terms " + std::to_string(n_terms) + " is above the limit " +
                                              std::to_string(limit) + " of zkfhe_bfv_dot_max_terms: split the sum and add the parts");
  return ZKFHE_OK;
}

int zk_bfv_dot_core(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, bool plain, size_t n_groups, size_t n_terms, size_t b_groups, const DotIo &io,
                    int l, int base_bits) {
  return plain ? dot_core<true>(ctx, params, n_groups, n_terms, b_groups, io, 0, 0)
               : dot_core<false>(ctx, params, n_groups, n_terms, b_groups, io, l, base_bits);
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_dot_max_terms(const zkfhe_bfv_params *params, int plain, size_t *max_terms_out) {
  if (!max_terms_out) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_dot_max_terms: max_terms is NULL");
  ZK_CK(check_params(nullptr, params));
  *max_terms_out = (size_t)max_terms(params, plain != 0);
  return ZKFHE_OK;
}

int zkfhe_bfv_dot(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n_terms, const uint64_t *a0, const uint64_t *a1,
                  size_t b_groups, const uint64_t *b0, const uint64_t *b1, const uint64_t *rlk0, const uint64_t *rlk1, int base_bits,
                  uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  if (!(ctx && a0 && a1 && b0 && b1 && rlk0 && rlk1 && out0 && out1 && n_groups > 0 && n_terms > 0))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_dot: a NULL argument or a zero count");
  return dot_call<false>(ctx, params, n_groups, n_terms, a0, a1, b_groups, b0, b1, rlk0, rlk1, base_bits, out0, out1, "bfv_dot");
}

int zkfhe_bfv_dot_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n_terms, const uint64_t *c0, const uint64_t *c1,
                        size_t m_groups, const uint64_t *m, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  if (!(ctx && c0 && c1 && m && out0 && out1 && n_groups > 0 && n_terms > 0))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_dot_plain: a NULL argument or a zero count");
  return dot_call<true>(ctx, params, n_groups, n_terms, c0, c1, m_groups, m, nullptr, nullptr, nullptr, 0, out0, out1, "bfv_dot_plain");
}

}  // extern "C"
