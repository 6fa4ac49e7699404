// The BFV key switch, for every caller: the relinearization of mul and dot (bfv_eval.hip, bfv_dot.hip), the Galois chain
// (bfv_galois.hip) and the levels of ring packing (bfv_pack.hip).  A polynomial v (what a digit source of key_switch_src.hip.hpp
// yields) is decomposed into l digits d_i = (v >> i w) & (2^w - 1); each is transformed with the five primes, multiplied by the
// transforms of key0_i and key1_i (key_hat: [2 l][5][N], the key0_i then the key1_i), the products are summed over the digits and
// transformed back, one polynomial per component (sum < l N 2^w Q < 2^116), into acc ([2][c][5][N], what the CRT epilogues read).
// The rows of a hybrid key set are the residues of integers below Q P (bfv_evk.hip): the same kernels, and a sum of at most
// l N (2^w - 1) (Q P - 1) <= P5 / 2 (zkfhe_bfv_hybrid_max_p), which the hybrid epilogues divide by P.
//   k_key_switch<Src>        the digit-serial body: one workgroup per (polynomial, prime) walks the l digits and accumulates in acc
//   k_key_switch_digit<Src>  the digit-parallel body: one workgroup per (digit, polynomial, prime) writes the two products to
//                            part[digit][comp][k][prime][N]
//   k_key_switch_fold        one workgroup per (comp, polynomial, prime): the l partials summed mod p, the inverse transform
// 5 workgroups per polynomial fill little of the device for a handful of polynomials; 5 l do better up to zk_bfv_wide_max.
// The two bodies share the digit load and the key product (load_digit, KeyRows), and all three end in inverse_scale.  mont_mul and
// add_p return canonical residues of canonical operands, and a sum of canonical residues taken mod p by add_p does not depend on
// the order of its terms, so both ways leave the same words in acc.  No kernel uses scratch; none branches on or addresses by a
// coefficient's value.
#include <cstdlib>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;

// the digit at `shift` of every coefficient of a source polynomial (at: d -> coefficient), as residues mod p in LDS
template <class At>
__device__ __forceinline__ void load_digit(uint32_t *lds, At at, int shift, uint64_t mask, unsigned n, uint32_t p) {
  for (unsigned d = threadIdx.x; d < n; d += NTT_THREADS) lds[d] = (uint32_t)(((at(d) >> shift) & mask) % p);
}

// the words of prime j of the transformed key0_i and key1_i in key_hat ([2 l][NP][N]), and a transformed digit word times both
struct KeyRows {
  const uint32_t *r0, *r1;
  __device__ __forceinline__ KeyRows(const uint32_t *key_hat, int l, size_t i, unsigned j, unsigned n)
      : r0(key_hat + i * ((size_t)NP * n) + (size_t)j * n), r1(key_hat + ((size_t)l + i) * ((size_t)NP * n) + (size_t)j * n) {}
  __device__ __forceinline__ void mul(uint32_t x, unsigned d, uint32_t p, uint32_t pinv, uint32_t &u0, uint32_t &u1) const {
    u0 = mont_mul(x, r0[d], p, pinv), u1 = mont_mul(x, r1[d], p, pinv);
  }
};

// the tail of every body: the sum of prime j in LDS (behind a barrier) transformed back and scaled into o.  n and rc come in as the
// kernel holds them: with 1 << log_n formed here, or the scale read ahead of the transform, the compiler emits other code for the
// kernels (profiles/bfv_key_switch_one.md)
__device__ __forceinline__ void inverse_scale(uint32_t *lds, const uint32_t *iv, int log_n, unsigned n, uint32_t p, uint32_t pinv,
                                              const RnsConst<NP> &rc, unsigned j, uint32_t *o) {
  rns_inverse(lds, iv, log_n, p, pinv);
  for (unsigned d = threadIdx.x; d < n; d += NTT_THREADS) o[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
}

// blockIdx.x = k * NP + prime.  The products are summed in acc[0][k][prime] and acc[1][k][prime] (each thread owns its positions),
// which are then transformed back in place.
template <class Src>
__global__ __launch_bounds__(NTT_THREADS) void k_key_switch(Src src, int l, int w, const uint32_t *__restrict__ key_hat, size_t c, int log_n,
                                                            const uint32_t *__restrict__ tw, RnsConst<NP> rc, uint32_t *__restrict__ acc, uint64_t q) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t k = blockIdx.x / NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n;
  const uint32_t *fw = tw + (size_t)j * 2 * NMAX, *iv = fw + NMAX;
  uint32_t *acc0 = acc + k * plane + (size_t)j * n, *acc1 = acc0 + c * plane;
  const auto at = src.at(k, n, q);
  const uint64_t mask = ((uint64_t)1 << w) - 1;
  for (int i = 0; i < l; ++i) {
    load_digit(lds, at, i * w, mask, n, p);   // i w < bitlen(Q - 1) <= 63
    __syncthreads();
    rns_forward(lds, fw, log_n, p, pinv);
    const KeyRows key(key_hat, l, (size_t)i, j, n);
    for (unsigned d = tid; d < n; d += NTT_THREADS) {
      uint32_t u0, u1;
      key.mul(lds[d], d, p, pinv, u0, u1);
      acc0[d] = i ? add_p(acc0[d], u0, p) : u0;
      acc1[d] = i ? add_p(acc1[d], u1, p) : u1;
    }
    __syncthreads();
  }
  for (int comp = 0; comp < 2; ++comp) {
    uint32_t *a = comp ? acc1 : acc0;
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = a[d];
    __syncthreads();
    inverse_scale(lds, iv, log_n, n, p, pinv, rc, j, a);
    __syncthreads();
  }
}

// blockIdx.x = (digit * c + k) * NP + prime; part: [l][2][c][NP][N]
template <class Src>
__global__ __launch_bounds__(NTT_THREADS) void k_key_switch_digit(Src src, int l, int w, const uint32_t *__restrict__ key_hat, size_t c, int log_n,
                                                                  const uint32_t *__restrict__ tw, RnsConst<NP> rc, uint32_t *__restrict__ part,
                                                                  uint64_t q) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t ik = blockIdx.x / NP, i = ik / c, k = ik % c;
  const unsigned n = 1u << log_n;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n;
  const auto at = src.at(k, n, q);
  load_digit(lds, at, (int)i * w, ((uint64_t)1 << w) - 1, n, p);   // i w < bitlen(Q - 1) <= 63
  __syncthreads();
  rns_forward(lds, tw + (size_t)j * 2 * NMAX, log_n, p, pinv);
  uint32_t *o0 = part + ((i * 2) * c + k) * plane + (size_t)j * n, *o1 = o0 + c * plane;
  const KeyRows key(key_hat, l, i, j, n);
  for (unsigned d = threadIdx.x; d < n; d += NTT_THREADS) key.mul(lds[d], d, p, pinv, o0[d], o1[d]);
}

// blockIdx.x = (comp * c + k) * NP + prime, which is also the polynomial of acc ([2][c][NP][N]) that the workgroup writes
__global__ __launch_bounds__(NTT_THREADS) void k_key_switch_fold(const uint32_t *__restrict__ part, int l, size_t c, int log_n,
                                                                 const uint32_t *__restrict__ tw, RnsConst<NP> rc, uint32_t *__restrict__ acc) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t digit_stride = 2 * c * NP * (size_t)n;
  const uint32_t *s = part + (size_t)blockIdx.x * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    uint32_t v = s[d];
    for (int i = 1; i < l; ++i) v = add_p(v, s[i * digit_stride + d], p);
    lds[d] = v;
  }
  __syncthreads();
  inverse_scale(lds, tw + (size_t)j * 2 * NMAX + NMAX, log_n, n, p, pinv, rc, j, acc + (size_t)blockIdx.x * n);
}

// Where the digit-parallel path stops: the grid of k_key_switch_digit, c 5 l workgroups, is at most WIDE_GRID_NUM / WIDE_GRID_DEN
// workgroups per CU of the device.  Measured on the MI355X (profiles/bfv_evk.md): up to 5/4 of the CU count the two kernels'
// slowest repeat lay below k_key_switch's fastest at every N, w and kind of key switch measured; past it not at every one.
constexpr size_t WIDE_GRID_NUM = 5, WIDE_GRID_DEN = 4;

}  // namespace

namespace zkrns {

size_t zk_bfv_wide_max(const zkfhe_ctx *ctx, uint64_t n, int l) {
  if (l < 2) return 0;
  // the partials ([l][2][c][5][N]) stay within the accumulators of a full chunk ([2][chunk_polys][5][N])
  const size_t room = chunk_polys(n) / (size_t)l;
  static const char *forced = getenv("ZKFHE_EVK_WIDE_MAX");   // measurements only: the bound itself, still within the arena's room
  if (forced) return std::min<size_t>(room, strtoull(forced, nullptr, 10));
  const size_t by_grid = (size_t)std::max(ctx->num_cu, 1) * WIDE_GRID_NUM / (WIDE_GRID_DEN * NP * (size_t)l);
  return std::min(room, by_grid);
}

void KeySwitch::add(Arena &a, const zkfhe_ctx *ctx, const KeySource &key, size_t c_max, bool per_level) {
  const uint64_t n = (uint64_t)1 << log_n;
  wide_max = key.resident() ? zk_bfv_wide_max(ctx, n, l) : 0;
  if (!per_level && c_max > wide_max) wide_max = 0;
  if (wide_max) a.add(part, (size_t)l * 2 * std::min(wide_max, c_max) * NP * n);
}

template <class Src>
int zk_bfv_key_switch(zkfhe_ctx *ctx, const KeySwitch &ks, const Src &src, const uint32_t *key_hat, size_t c, uint32_t *acc) {
  const int log_n = ks.log_n, l = ks.l;
  const bool wide = ks.part && c <= ks.wide_max;
  const void *body = wide ? (const void *)k_key_switch_digit<Src> : (const void *)k_key_switch<Src>;
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds;
  ZK_CK(ntt_lds(ctx, body, log_n, &lds));
  const RnsConst<NP> rc = rns_const<NP>(log_n);
  const double words = (double)c * NP * ((size_t)1 << log_n);
  zk_prof_begin(ctx);
  if (wide)
    k_key_switch_digit<Src><<<(unsigned)(c * NP * l), NTT_THREADS, lds, ctx->stream>>>(src, l, ks.w, key_hat, c, log_n, tw, rc, ks.part, ks.q);
  else
    k_key_switch<Src><<<(unsigned)(c * NP), NTT_THREADS, lds, ctx->stream>>>(src, l, ks.w, key_hat, c, log_n, tw, rc, acc, ks.q);
  ZK_LAUNCH_CHECK(ctx);
  // per digit: its source, two key rows, and two partials out or two accumulators in and out; serial: the inverse transforms' 16
  if (!wide) {
    zk_prof_end(ctx, Src::serial_slot, words * (l * (src.bytes() + 8.0 + 16.0) + 16.0));
    return ZKFHE_OK;
  }
  zk_prof_end(ctx, Src::digit_slot, words * l * (src.bytes() + 8.0 + 8.0));
  ZK_CK(ntt_lds(ctx, (const void *)k_key_switch_fold, log_n, &lds));
  zk_prof_begin(ctx);
  k_key_switch_fold<<<(unsigned)(2 * c * NP), NTT_THREADS, lds, ctx->stream>>>(ks.part, l, c, log_n, tw, rc, acc);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_KEY_SWITCH_WIDE, words * 2 * (4.0 * l + 4.0));
  return ZKFHE_OK;
}

template int zk_bfv_key_switch<SrcPlain>(zkfhe_ctx *, const KeySwitch &, const SrcPlain &, const uint32_t *, size_t, uint32_t *);
template int zk_bfv_key_switch<SrcGalois>(zkfhe_ctx *, const KeySwitch &, const SrcGalois &, const uint32_t *, size_t, uint32_t *);
template int zk_bfv_key_switch<SrcPack>(zkfhe_ctx *, const KeySwitch &, const SrcPack &, const uint32_t *, size_t, uint32_t *);

}  // namespace zkrns
