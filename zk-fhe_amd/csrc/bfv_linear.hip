// Hoisted BFV rotations and slot-wise linear transforms on the GPU (zkfhe.h, INTEGRATION.md "Encrypted matrix-vector products").
// Conventions of bfv_enc.hip: host arrays, N residues in [0, Q) per polynomial, CircuitInput order.
//
// out = sum_k diag_k * rot_k(x) for K Galois elements g_k.  The digits D_i = (c1 >> i w) & (2^w - 1) of c1 do not depend on g, so
// they are decomposed and transformed once per ciphertext, and sigma_g is applied to the transforms: rns_forward leaves the
// evaluation at psi^(2 br(k) + 1) at index k, so the transform of sigma_g(d) at index k is the transform of d at the index k' with
// 2 br(k') + 1 = (2 br(k) + 1) g mod 2N (galois_index).  The address depends on g (public) and never on a value.
//   k_hoist        per (ciphertext, row, prime): row 0 is c0 read centred, row 1 + i the digit D_i of c1; one forward transform
//                  each, kept as hst[ct][1 + l][5][N] (row 0 times R^-1, the factor a Montgomery product with a key word carries)
//   k_linear_acc   pointwise, per (prime, index) and CT ciphertexts per thread: for every element k,
//                  t_0 = c0^[k'] + sum_i D^_i[k'] gk0^_{k,i}[index], t_1 = sum_i D^_i[k'] gk1^_{k,i}[index] (g = 1: t_1 = sum_i
//                  D^_i 2^(i w), the transform of c1 itself, and no key is read).  apply_galois_many stores t_j per element;
//                  linear_transform accumulates acc_j += p^_k[index] t_j over the elements and stores acc_j.  Every key and
//                  diagonal word is read once per CT ciphertexts, coalesced; the digit reads are gathers that stay inside aligned
//                  blocks of 64 words of one polynomial (neighbouring indices differ in the top bits of br, which g moves only
//                  within the top bits).
//   k_rns_intt     one inverse transform per output polynomial and prime, in place
//   k_eval_epilogue (bfv_eval.hip) EV_MODQ: Garner over the five primes, x mod Q.  sigma_g(c0) is already inside the sum.
// linear_transform_bsgs is the same at two levels, out = sum_i rot_{G_i}(sum_j diag_{i,j} * rot_{b_j}(x)): k_hoist and
// k_linear_acc<ACC_MANY> leave the baby rotations in the transform domain, k_bsgs_inner multiplies them by the diagonals (a small
// matrix product per point), k_rns_intt and the epilogue reduce the inner sums mod Q (the definition takes their digits), k_hoist
// transforms those, and k_linear_acc<ACC_GIANT> rotates inner ciphertext i by giant element i and accumulates (bsgs_call).
// Sizes: |r| < Q + l N (2^w - 1) Q < 2^116 for a rotation; the transform's sum is below n_elems N floor(T/2) times that, which the
// call bounds by 2^150 (check_range) under the half of the primes' product 2^151.2.  No kernel uses scratch.
// Every call is a prepare half (the checks of elements, keys and diagonals; the element table, the keys and the diagonals uploaded
// and transformed: struct zkfhe_bfv_plan) and a run half (the ciphertext check and the chunk loop, from that struct alone).  The
// host-array calls prepare into the context's work arena and run; zkfhe_bfv_plan_create* prepare into allocations of the plan's own,
// and zkfhe_bfv_plan_apply is the run half.  The run half takes its ciphertexts from host arrays or, for the resident batches of
// bfv_resident.hip, from device planes (zk_bfv_plan_run_dev): only the copies around a chunk differ (Planes, bfv_host.hpp).
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
constexpr int ACC_THREADS = 256;
constexpr int CT = 4;                   // ciphertexts per thread of k_linear_acc: each key word serves CT of them
constexpr uint32_t NO_KEY = 0xffffffffu;   // the key slot of g = 1

// per-prime constants of k_linear_acc: 2^w R mod p (a Montgomery product by it multiplies by 2^w)
struct GadgetStep {
  uint32_t step[NP];
};

// One workgroup per (ciphertext, row, prime), blockIdx.x = (ct (1 + l) + row) NP + prime; x = [c0 | c1] ([2 c][N]).
__global__ __launch_bounds__(NTT_THREADS) void k_hoist(const uint64_t *__restrict__ x, size_t c, int l, int w, uint64_t q, int log_n,
                                                        const uint32_t *__restrict__ tw, RnsConst<NP> rc, uint32_t *__restrict__ hst) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP, rows = (unsigned)l + 1, row = (blockIdx.x / NP) % rows;
  const size_t ct = blockIdx.x / NP / rows;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  if (row == 0) {
    const uint64_t *s = x + ct * n;
    bool bad = false;
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = rns_load(s[n - 1 - d], LOAD_CENTRED, q, p, bad);
  } else {
    const uint64_t *s = x + (c + ct) * n, mask = ((uint64_t)1 << w) - 1;
    const int shift = (int)(row - 1) * w;   // < bitlen(Q - 1) <= 63
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = (uint32_t)(((s[n - 1 - d] >> shift) & mask) % p);
  }
  __syncthreads();
  rns_forward(lds, tw + (size_t)j * 2 * NMAX, log_n, p, pinv);
  uint32_t *o = hst + (size_t)blockIdx.x * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) o[d] = row ? lds[d] : mont_mul(lds[d], 1u, p, pinv);
}

// the index k' with 2 br(k') + 1 = (2 br(k) + 1) g mod 2N (br: bit reversal on log_n bits, 3 <= log_n <= 15)
__device__ __forceinline__ unsigned galois_index(unsigned k, unsigned g, int log_n) {
  const unsigned e = ((2 * (__brev(k) >> (32 - log_n)) + 1) * g) & ((2u << log_n) - 1);   // < 2^16 2^16
  return __brev(e >> 1) >> (32 - log_n);
}

// One thread per (index, prime, group of CT ciphertexts): blockIdx.x tiles the N indices, blockIdx.y is the prime, blockIdx.z the
// group.  hst: [c][1 + l][NP][N] (k_hoist); elem: [n_elems][2] = (g, key slot or NO_KEY); key_hat: [slot][2 l][NP][N], the gk0 rows
// then the gk1 rows; diag_hat: [n_elems][NP][N].
// ACC_MANY: out[k][comp][ct][prime][index] = t_comp of element k.  ACC_LINEAR: out[comp][ct][prime][index] = sum_k p^_k t_comp.
// ACC_GIANT (the outer sum of linear_transform_bsgs): element k reads the hoisted rows of ciphertext k c + ct (hst: [n_elems][c][1 + l]
// [NP][N], the inner ciphertexts of giant step k) and out[comp][ct][prime][index] += sum_k t_comp: no diagonal, and the sum starts
// from what out holds, so that groups of giant steps add up (the host zeroes out before the first group).
// Every value is a residue below p < 2^31, every product a mont_mul and every sum an add_p: nothing is carried unreduced.
enum AccMode { ACC_MANY = 0, ACC_LINEAR = 1, ACC_GIANT = 2 };
template <int MODE>
__global__ __launch_bounds__(ACC_THREADS) void k_linear_acc(const uint32_t *__restrict__ hst, const uint32_t *__restrict__ elem, int n_elems,
                                                             const uint32_t *__restrict__ key_hat, const uint32_t *__restrict__ diag_hat,
                                                             int l, size_t c, int log_n, RnsConst<NP> rc, GadgetStep gs,
                                                             uint32_t *__restrict__ out) {
  const unsigned n = 1u << log_n, idx = blockIdx.x * ACC_THREADS + threadIdx.x, j = blockIdx.y;
  if (idx >= n) return;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n, ct0 = (size_t)blockIdx.z * CT;
  const uint32_t *h[CT];   // the hoisted rows of this thread's ciphertexts at this prime (past the last one: the last one again)
#pragma unroll
  for (int t = 0; t < CT; ++t) h[t] = hst + std::min(ct0 + t, c - 1) * (size_t)(l + 1) * plane + (size_t)j * n;
  uint32_t acc0[CT], acc1[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    acc0[t] = acc1[t] = 0;
    if (MODE == ACC_GIANT && ct0 + t < c) acc0[t] = out[(ct0 + t) * plane + (size_t)j * n + idx], acc1[t] = out[(c + ct0 + t) * plane + (size_t)j * n + idx];
  }
  for (int k = 0; k < n_elems; ++k) {
    const uint32_t g = elem[2 * k], slot = elem[2 * k + 1];   // uniform over the grid
    const unsigned kp = galois_index(idx, g, log_n);
    if (MODE == ACC_GIANT && k) {
#pragma unroll
      for (int t = 0; t < CT; ++t) h[t] += c * (size_t)(l + 1) * plane;   // the inner ciphertexts of the next giant step
    }
    uint32_t t0[CT], t1[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) t0[t] = h[t][kp], t1[t] = 0;
    if (slot != NO_KEY) {
      const uint32_t *k0 = key_hat + (size_t)slot * 2 * l * plane + (size_t)j * n + idx, *k1 = k0 + (size_t)l * plane;
      for (int i = 0; i < l; ++i) {
        const uint32_t a0 = k0[(size_t)i * plane], a1 = k1[(size_t)i * plane];
#pragma unroll
        for (int t = 0; t < CT; ++t) {
          const uint32_t d = h[t][(size_t)(i + 1) * plane + kp];
          t0[t] = add_p(t0[t], mont_mul(d, a0, p, pinv), p);
          t1[t] = add_p(t1[t], mont_mul(d, a1, p, pinv), p);
        }
      }
    } else {   // g = 1: (c0, c1) itself, c1 = sum_i D_i 2^(i w)
      uint32_t pw = 1;
      for (int i = 0; i < l; ++i) {
#pragma unroll
        for (int t = 0; t < CT; ++t) t1[t] = add_p(t1[t], mont_mul(h[t][(size_t)(i + 1) * plane + kp], pw, p, pinv), p);
        pw = mont_mul(pw, gs.step[j], p, pinv);
      }
    }
    if (MODE == ACC_LINEAR) {
      const uint32_t ph = diag_hat[((size_t)k * NP + j) * n + idx];
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        acc0[t] = add_p(acc0[t], mont_mul(t0[t], ph, p, pinv), p);
        acc1[t] = add_p(acc1[t], mont_mul(t1[t], ph, p, pinv), p);
      }
    } else if (MODE == ACC_GIANT) {
#pragma unroll
      for (int t = 0; t < CT; ++t) acc0[t] = add_p(acc0[t], t0[t], p), acc1[t] = add_p(acc1[t], t1[t], p);
    } else {
      uint32_t *o = out + (size_t)k * 2 * c * plane + (size_t)j * n + idx;
#pragma unroll
      for (int t = 0; t < CT; ++t)
        if (ct0 + t < c) o[(ct0 + t) * plane] = t0[t], o[(c + ct0 + t) * plane] = t1[t];
    }
  }
  if (MODE != ACC_MANY) {
    uint32_t *o = out + (size_t)j * n + idx;
#pragma unroll
    for (int t = 0; t < CT; ++t)
      if (ct0 + t < c) o[(ct0 + t) * plane] = acc0[t], o[(c + ct0 + t) * plane] = acc1[t];
  }
}

// The inner sums of linear_transform_bsgs: per (index, prime) the small matrix product acc[i][comp][ct] = sum_b p^_{i,b} t_b[comp][ct]
// of the diagonals ([n_giant][n_baby]) with the baby rotations ([n_baby][2 c]).  One thread per (index, prime, tile of GT giant steps
// x CTI ciphertexts x 2 components): blockIdx.x tiles the N indices, blockIdx.y is the prime, blockIdx.z = giant tile * ciphertext
// groups + ciphertext group.  baby: [n_baby][2][c][NP][N] (the output of k_linear_acc<ACC_MANY>); diag_hat: [n_giant][n_baby][NP][N]
// (the rows of this launch's n_giant steps); out: [2][n_giant][c][NP][N], so that after the inverse transform and the reduction mod Q
// the n_giant c inner ciphertexts are the [c0 | c1] input of k_hoist.  Every diagonal word is read once per ciphertext group and
// every baby word once per giant tile, coalesced along the index; a tile past the last giant step or ciphertext reads the last one
// again and stores nothing.  Residues below p, mont_mul and add_p only, as in k_linear_acc.
template <int GT, int CTI>
__global__ __launch_bounds__(ACC_THREADS) void k_bsgs_inner(const uint32_t *__restrict__ baby, const uint32_t *__restrict__ diag_hat,
                                                             int n_baby, int n_giant, size_t c, int log_n, RnsConst<NP> rc,
                                                             uint32_t *__restrict__ out) {
  const unsigned n = 1u << log_n, idx = blockIdx.x * ACC_THREADS + threadIdx.x, j = blockIdx.y;
  if (idx >= n) return;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n, groups = (c + CTI - 1) / CTI, at = (size_t)j * n + idx;
  const size_t ct0 = (size_t)(blockIdx.z % groups) * CTI;
  const int i0 = (int)(blockIdx.z / groups) * GT;
  const uint32_t *d[GT], *t[CTI];
#pragma unroll
  for (int a = 0; a < GT; ++a) d[a] = diag_hat + (size_t)std::min(i0 + a, n_giant - 1) * n_baby * plane + at;
#pragma unroll
  for (int b = 0; b < CTI; ++b) t[b] = baby + std::min(ct0 + b, c - 1) * plane + at;
  uint32_t acc[GT][CTI][2];
#pragma unroll
  for (int a = 0; a < GT; ++a)
#pragma unroll
    for (int b = 0; b < CTI; ++b) acc[a][b][0] = acc[a][b][1] = 0;
  for (int k = 0; k < n_baby; ++k) {
    uint32_t ph[GT], t0[CTI], t1[CTI];
#pragma unroll
    for (int a = 0; a < GT; ++a) ph[a] = d[a][(size_t)k * plane];
#pragma unroll
    for (int b = 0; b < CTI; ++b) t0[b] = t[b][(size_t)k * 2 * c * plane], t1[b] = t[b][((size_t)k * 2 + 1) * c * plane];
#pragma unroll
    for (int a = 0; a < GT; ++a)
#pragma unroll
      for (int b = 0; b < CTI; ++b) {
        acc[a][b][0] = add_p(acc[a][b][0], mont_mul(t0[b], ph[a], p, pinv), p);
        acc[a][b][1] = add_p(acc[a][b][1], mont_mul(t1[b], ph[a], p, pinv), p);
      }
  }
#pragma unroll
  for (int a = 0; a < GT; ++a)
#pragma unroll
    for (int b = 0; b < CTI; ++b)
      if (i0 + a < n_giant && ct0 + b < c) {
        uint32_t *o = out + ((size_t)(i0 + a) * c + ct0 + b) * plane + at;
        o[0] = acc[a][b][0], o[(size_t)n_giant * c * plane] = acc[a][b][1];
      }
}

// One workgroup per (polynomial, prime) of res ([polys][NP][N]): the inverse transform in place, times scale[prime].  Launched through
// zk_rns_intt (bfv_host.hpp), which bfv_dot.hip calls too.
__global__ __launch_bounds__(NTT_THREADS) void k_rns_intt(uint32_t *__restrict__ res, int log_n, const uint32_t *__restrict__ tw, RnsConst<NP> rc) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP, n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  uint32_t *a = res + (size_t)blockIdx.x * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = a[d];
  __syncthreads();
  rns_inverse(lds, tw + (size_t)j * 2 * NMAX + NMAX, log_n, p, pinv);
  for (unsigned d = tid; d < n; d += NTT_THREADS) a[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
}

// ------------------------------------------------------------------------------------------------------------------ host side

int bitlen(unsigned __int128 v) {
  int b = 0;
  for (; v; v >>= 1) ++b;
  return b;
}

// The sum of linear_transform is carried in the five primes without a reduction: |out| < n_elems N floor(T/2) Q (1 + l N (2^w - 1)),
// which must stay below half of their product (2^151.2): refused when the bit lengths add up to more than 150.
int check_range(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t n_elems, int l, int w, const char *fn) {
  const unsigned __int128 ks = 1 + (unsigned __int128)l * prm->n * (((uint64_t)1 << w) - 1);
  const int bits = bitlen(n_elems) + bitlen(prm->n) + bitlen(prm->t / 2) + bitlen(prm->q - 1) + bitlen(ks);
  if (bits > 150)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": the sum over the elements needs " + std::to_string(bits) +
                                              " bits and the five-prime product carries 150: narrow base_bits, or split the element list and add the parts");
  return ZKFHE_OK;
}

// rc with scale = N^-1 R^(1 + products) mod p: the inverse transform's scale when every value carries R^-products
RnsConst<NP> intt_const(int log_n, int products) {
  RnsConst<NP> rc = rns_const<NP>(log_n);
  for (int j = 0; j < NP; ++j) {
    const uint64_t p = PRIMES[j], R = ((uint64_t)1 << 32) % p;
    uint64_t s = pow_mod((uint64_t)1 << log_n, p - 2, p) * R % p;
    for (int i = 0; i < products; ++i) s = s * R % p;
    rc.scale[j] = (uint32_t)s;
  }
  return rc;
}

// ciphertexts per chunk: the hoisted rows (and, per element, the outputs of apply_galois_many) of a chunk hold chunk_polys(N)
// polynomials of five primes
size_t chunk_cts(uint64_t n, size_t n_cts, size_t rows) { return std::min(n_cts, std::max<size_t>(1, chunk_polys(n) / rows)); }

// The chunk rule of linear_transform_bsgs.  A ciphertext holds max(1 + l, 2 n_baby) polynomials of hoisted rows or baby rotations
// and (1 + l) hoisted rows per giant step; cts ciphertexts with all their giant steps fit the budget of chunk_polys(N).  Where one
// ciphertext's giant rows alone exceed it (cts = 1), the giant steps go in groups of giants and the groups add up in the transform
// domain.  A chunk that is not the whole batch is a multiple of the kernels' tile of CT ciphertexts.
void bsgs_chunks(uint64_t n, size_t n_cts, size_t n_baby, size_t n_giant, size_t rows, size_t *cts, size_t *giants) {
  *cts = chunk_cts(n, n_cts, std::max(rows, 2 * n_baby) + n_giant * rows);
  if (*cts > CT && *cts < n_cts) *cts -= *cts % CT;   // whole ciphertext tiles, unless the chunk is the batch
  *giants = std::min(n_giant, std::max<size_t>(1, chunk_polys(n) / (*cts * rows)));
}

// the words of a plan's three buffers: elem_d, key_hat, diag_hat (zkfhe_bfv_plan_bytes is four times their sum)
unsigned __int128 plan_words(uint64_t n, int l, size_t n_elems, size_t slots, size_t n_diag, int which) {
  typedef unsigned __int128 u128;
  return which == 0 ? (u128)2 * n_elems : which == 1 ? (u128)2 * slots * l * n * NP : (u128)n_diag * n * NP;
}

}  // namespace

// What a linear transform holds before it sees a ciphertext: the element table, the transformed keys and the transformed diagonals,
// with the counts that their layout depends on.  The host-array calls fill one on the stack whose buffers are carved from the
// context's work arena (prepare_*), and run from it (linear_run, bsgs_run); a zkfhe_bfv_plan owns its three buffers, and
// zkfhe_bfv_plan_apply runs from it.  Nothing is written to it after prepare_device, and a run reads nothing else that outlives the
// call, so keys of other calls can be kept resident the same way: a struct of transformed buffers and counts beside this one.
struct zkfhe_bfv_plan {
  zkfhe_bfv_params params{};
  int base_bits = 0, l = 0, log_n = 0;
  int device = 0;                   // of the context that prepared it
  bool bsgs = false;                // two-level: n_baby baby elements, then n_giant giant ones; flat: n_baby elements, n_giant = 0
  size_t n_baby = 0, n_giant = 0;
  size_t slots = 0;                 // key slots: the elements with g != 1
  size_t n_diag = 0;                // diagonals: n_baby (flat), n_giant n_baby (two-level), 0 (apply_galois_many)
  std::vector<uint32_t> elem;       // the host copy of elem_d: [n_baby + n_giant][2] = (g, key slot or NO_KEY)
  uint32_t *elem_d = nullptr, *key_hat = nullptr, *diag_hat = nullptr;
  bool owned = false;               // the three buffers are this plan's own allocations (plan_free), not a carve of the arena
  uint64_t device_bytes = 0;        // owned: the sum of the three requested sizes
};

namespace {

// The elements and keys of a call: list a (all elements of a flat call, the baby elements of a two-level one), then list b (the
// giant elements; empty for a flat call).  Element k of the joint list has its key rows at block k of its own list.
struct KeyLists {
  size_t n_a, n_b;
  const uint64_t *g_a, *a0, *a1, *g_b, *b0, *b1;
  size_t count() const { return n_a + n_b; }
  uint64_t g(size_t k) const { return k < n_a ? g_a[k] : g_b[k - n_a]; }
  const uint64_t *k0(size_t k, size_t lw) const { return k < n_a ? a0 + k * lw : b0 + (k - n_a) * lw; }
  const uint64_t *k1(size_t k, size_t lw) const { return k < n_a ? a1 + k * lw : b1 + (k - n_a) * lw; }
};

// The prepare half comes in three steps, so that a host-array call keeps the order of its refusals (a ciphertext coefficient is
// checked after the range rule and before the keys) and carves its one arena between the checks and the device work.
// Step 1, no pass over an input array and no device work: the parameters, base_bits, the counts, every g, the range rule of the
// sum over n_a elements (has_diag; the inner sum of a two-level call); fills the counts and the element table of p.
int prepare_head(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const KeyLists &ks, int base_bits, bool bsgs, bool has_diag, const char *fn,
                 zkfhe_bfv_plan *p) {
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  const uint64_t n = params->n;
  if ((ks.n_a >> 20) || (ks.n_b >> 20)) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": more than 2^20 Galois elements");
  const size_t n_elems = ks.count();
  for (size_t k = 0; k < n_elems; ++k)
    if (!(ks.g(k) & 1) || ks.g(k) >= 2 * n) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": every Galois element g must be odd and below 2N");
  if (has_diag) ZK_CK(check_range(ctx, params, ks.n_a, l, base_bits, fn));   // before any O(n) pass and any device work
  p->params = *params;
  p->base_bits = base_bits, p->l = l, p->log_n = bit_log2(n), p->device = ctx->device;
  p->bsgs = bsgs, p->n_baby = ks.n_a, p->n_giant = ks.n_b, p->n_diag = !has_diag ? 0 : bsgs ? ks.n_b * ks.n_a : ks.n_a;
  p->elem.resize(2 * n_elems);
  p->slots = 0;
  for (size_t k = 0; k < n_elems; ++k) {   // g = 1 takes no key slot
    p->elem[2 * k] = (uint32_t)ks.g(k);
    p->elem[2 * k + 1] = ks.g(k) == 1 ? NO_KEY : (uint32_t)p->slots++;
  }
  return ZKFHE_OK;
}

// Step 2, the passes over the keys and the diagonals: a key coefficient >= Q, then a diagonal out of plaintext range.
int prepare_check(zkfhe_ctx *ctx, const zkfhe_bfv_plan &p, const KeyLists &ks, const uint64_t *diag, const char *fn) {
  const uint64_t n = p.params.n, q = p.params.q;
  const size_t lw = (size_t)p.l * n;
  for (size_t k = 0; k < ks.count(); ++k)   // the key rows of g = 1 are neither read nor checked
    if (ks.g(k) != 1) ZK_CK(check_below_q(ctx, ks.k0(k, lw), lw, q, fn, "a Galois-key", ks.k1(k, lw)));
  if (p.n_diag) ZK_CK(check_plain(ctx, diag, p.n_diag * n, q, p.params.t, fn, "a diagonal"));
  return ZKFHE_OK;
}

// Step 3, the device work: the element table, the keys and the diagonals uploaded and transformed into p.elem_d, p.key_hat and
// p.diag_hat, which the caller has pointed at plan_words() words each.  key_d (2 slots l N words) and diag_d (n_diag N words) are
// the staging copies and flag the transform's flag word: work buffers of the call, not kept.
int prepare_device(zkfhe_ctx *ctx, const zkfhe_bfv_plan &p, const KeyLists &ks, const uint64_t *diag, uint64_t *key_d, uint64_t *diag_d, int *flag) {
  const uint64_t n = p.params.n, q = p.params.q;
  const size_t lw = (size_t)p.l * n;
  ZK_CK(zkfhe_upload(ctx, p.elem_d, p.elem.data(), p.elem.size() * 4));
  for (size_t k = 0; k < ks.count(); ++k) {   // key slot s: its gk0 rows, then its gk1 rows
    if (p.elem[2 * k + 1] == NO_KEY) continue;
    ZK_CK(upload_key_pair(ctx, key_d + (size_t)p.elem[2 * k + 1] * 2 * lw, ks.k0(k, lw), ks.k1(k, lw), lw));
  }
  if (p.slots) ZK_CK(launch_rns_ntt<NP>(ctx, false, key_d, LOAD_RESIDUE, q, 2 * p.slots * p.l, p.log_n, nullptr, 0, p.key_hat, flag));
  if (p.n_diag) {
    ZK_CK(zkfhe_upload(ctx, diag_d, diag, p.n_diag * n * 8));
    ZK_CK(launch_rns_ntt<NP>(ctx, false, diag_d, LOAD_CENTRED, q, p.n_diag, p.log_n, nullptr, 0, p.diag_hat, flag));
  }
  return ZKFHE_OK;
}

// the prepared buffers and the staging copies as arena entries, in the order the host-array calls have always carved them
void add_prepared(Arena &a, zkfhe_bfv_plan &p, int *&flag, uint64_t *&key_d, uint64_t *&diag_d) {
  const uint64_t n = p.params.n;
  const size_t n_elems = p.n_baby + p.n_giant;
  a.add(flag, 1).add(p.elem_d, (size_t)plan_words(n, p.l, n_elems, p.slots, p.n_diag, 0)).add(key_d, 2 * p.slots * p.l * n)
      .add(p.key_hat, (size_t)plan_words(n, p.l, n_elems, p.slots, p.n_diag, 1)).add(diag_d, p.n_diag * n)
      .add(p.diag_hat, (size_t)plan_words(n, p.l, n_elems, p.slots, p.n_diag, 2));
}

// the run half's first step: a ciphertext coefficient >= Q
int check_cts(zkfhe_ctx *ctx, const zkfhe_bfv_plan &p, size_t n_cts, const uint64_t *c0, const uint64_t *c1, const char *fn) {
  return check_below_q(ctx, c0, n_cts * p.params.n, p.params.q, fn, "a ciphertext", c1);
}

// the work buffers of linear_run for n_cts ciphertexts
struct LinearWork {
  size_t chunk;
  uint64_t *x_d, *o_d;
  uint32_t *hst, *res;
};
void add_linear_work(Arena &a, const zkfhe_bfv_plan &p, size_t n_cts, LinearWork &w) {
  const uint64_t n = p.params.n;
  const size_t rows = (size_t)p.l + 1, per_ct = p.n_diag ? 2 : 2 * p.n_baby;   // output polynomials per ciphertext
  w.chunk = chunk_cts(n, n_cts, std::max(rows, per_ct));
  const size_t cw = w.chunk * n;
  a.add(w.x_d, 2 * cw).add(w.hst, rows * cw * NP).add(w.res, per_ct * cw * NP).add(w.o_d, per_ct * cw);
}

// The run half of the flat calls: the chunk loop over the ciphertexts x (host arrays or device planes, as out), from the prepared
// buffers of p.  p.n_diag == 0 is apply_galois_many.
int linear_run(zkfhe_ctx *ctx, const zkfhe_bfv_plan &p, size_t n_cts, const Planes &x, const Planes &out, const LinearWork &w) {
  const uint64_t n = p.params.n, q = p.params.q;
  const int l = p.l, log_n = p.log_n, base_bits = p.base_bits;
  const bool diag = p.n_diag != 0;
  const size_t n_elems = p.n_baby, slots = p.slots, rows = (size_t)l + 1, per_ct = diag ? 2 : 2 * n_elems, chunk = w.chunk;
  uint64_t *x_d = w.x_d, *o_d = w.o_d;
  uint32_t *hst = w.hst, *res = w.res;
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds_h;
  ZK_CK(ntt_lds(ctx, (const void *)k_hoist, log_n, &lds_h));
  const RnsConst<NP> rc = rns_const<NP>(log_n), rc_inv = intt_const(log_n, diag ? 2 : 1);
  GadgetStep gs;
  for (int j = 0; j < NP; ++j) gs.step[j] = (uint32_t)((((uint64_t)1 << base_bits) % PRIMES[j]) * (((uint64_t)1 << 32) % PRIMES[j]) % PRIMES[j]);
  const double words = (double)NP * n;   // one polynomial at every prime
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), polys = per_ct * c;
    ZK_CK(x.in(ctx, 0, lo, c, n, x_d));
    ZK_CK(x.in(ctx, 1, lo, c, n, x_d + c * n));
    zk_prof_begin(ctx);
    k_hoist<<<(unsigned)(c * rows * NP), NTT_THREADS, lds_h, ctx->stream>>>(x_d, c, l, base_bits, q, log_n, tw, rc, hst);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_HOIST, (double)c * rows * words * (8.0 + 4.0));
    const dim3 grid(zk_blocks(n, ACC_THREADS), NP, zk_blocks(c, CT));
    zk_prof_begin(ctx);
    if (diag)
      k_linear_acc<ACC_LINEAR><<<grid, ACC_THREADS, 0, ctx->stream>>>(hst, p.elem_d, (int)n_elems, p.key_hat, p.diag_hat, l, c, log_n, rc, gs, res);
    else
      k_linear_acc<ACC_MANY><<<grid, ACC_THREADS, 0, ctx->stream>>>(hst, p.elem_d, (int)n_elems, p.key_hat, nullptr, l, c, log_n, rc, gs, res);
    ZK_LAUNCH_CHECK(ctx);
    // read: every hoisted row per element, every key word once per CT ciphertexts, the diagonals likewise; written: the outputs
    zk_prof_end(ctx, ZKFHE_PROF_BFV_LINEAR, 4.0 * words * ((double)n_elems * c * rows + (double)zk_blocks(c, CT) * (2.0 * slots * l + (diag ? n_elems : 0)) + polys));
    ZK_CK(zk_rns_intt(ctx, res, polys, log_n, rc_inv));
    ZK_CK(zk_bfv_eval_epilogue(ctx, res, polys, log_n, q, EvEpi{}, o_d));
    for (size_t k = 0; k < (diag ? 1 : n_elems); ++k) {   // o_d: [element][component][c][N]
      ZK_CK(out.out(ctx, 0, k * n_cts + lo, c, n, o_d + 2 * k * c * n));
      ZK_CK(out.out(ctx, 1, k * n_cts + lo, c, n, o_d + (2 * k + 1) * c * n));
    }
  }
  return ZKFHE_OK;
}

// both flat calls: diag == nullptr is apply_galois_many
int linear_call(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, size_t n_elems,
                const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, int base_bits, const uint64_t *diag, uint64_t *out0,
                uint64_t *out1, const char *fn) {
  const KeyLists ks{n_elems, 0, g, gk0, gk1, nullptr, nullptr, nullptr};
  zkfhe_bfv_plan p;
  ZK_CK(prepare_head(ctx, params, ks, base_bits, false, diag != nullptr, fn, &p));
  ZK_CK(check_cts(ctx, p, n_cts, c0, c1, fn));
  ZK_CK(prepare_check(ctx, p, ks, diag, fn));
  int *flag;
  uint64_t *key_d, *diag_d;
  LinearWork w;
  Arena a;
  add_prepared(a, p, flag, key_d, diag_d);
  add_linear_work(a, p, n_cts, w);
  ZK_CK(a.carve(ctx));
  ZK_CK(prepare_device(ctx, p, ks, diag, key_d, diag_d, flag));
  return linear_run(ctx, p, n_cts, host_planes(c0, c1), host_planes(out0, out1), w);
}

template <int GT, int CTI>
void launch_bsgs_inner(zkfhe_ctx *ctx, const uint32_t *baby, const uint32_t *diag_hat, size_t n_baby, size_t n_giant, size_t c, int log_n,
                       const RnsConst<NP> &rc, uint32_t *out) {
  const dim3 grid(zk_blocks((size_t)1 << log_n, ACC_THREADS), NP, (unsigned)(zk_blocks(n_giant, GT) * zk_blocks(c, CTI)));
  k_bsgs_inner<GT, CTI><<<grid, ACC_THREADS, 0, ctx->stream>>>(baby, diag_hat, (int)n_baby, (int)n_giant, c, log_n, rc, out);
}

// the work buffers of bsgs_run for n_cts ciphertexts
struct BsgsWork {
  size_t chunk, group;
  uint64_t *x_d, *inner_q, *o_d;
  uint32_t *hst, *baby, *inner, *hst_in, *res;
};
void add_bsgs_work(Arena &a, const zkfhe_bfv_plan &p, size_t n_cts, BsgsWork &w) {
  const uint64_t n = p.params.n;
  const size_t rows = (size_t)p.l + 1;
  bsgs_chunks(n, n_cts, p.n_baby, p.n_giant, rows, &w.chunk, &w.group);
  const size_t cw = w.chunk * n, group = w.group;
  a.add(w.x_d, 2 * cw).add(w.hst, rows * cw * NP).add(w.baby, 2 * p.n_baby * cw * NP).add(w.inner, 2 * group * cw * NP)
      .add(w.inner_q, 2 * group * cw).add(w.hst_in, group * rows * cw * NP).add(w.res, 2 * cw * NP).add(w.o_d, 2 * cw);
}

// The run half of linear_transform_bsgs: the chunk loop over the ciphertexts and, inside it, the groups of giant steps.
int bsgs_run(zkfhe_ctx *ctx, const zkfhe_bfv_plan &p, size_t n_cts, const Planes &x, const Planes &out, const BsgsWork &w) {
  const uint64_t n = p.params.n, q = p.params.q;
  const int l = p.l, log_n = p.log_n, base_bits = p.base_bits;
  const size_t n_baby = p.n_baby, n_giant = p.n_giant, rows = (size_t)l + 1, chunk = w.chunk, group = w.group;
  const std::vector<uint32_t> &elem = p.elem;
  const uint32_t *elem_d = p.elem_d, *key_hat = p.key_hat, *diag_hat = p.diag_hat;
  uint64_t *x_d = w.x_d, *inner_q = w.inner_q, *o_d = w.o_d;
  uint32_t *hst = w.hst, *baby = w.baby, *inner = w.inner, *hst_in = w.hst_in, *res = w.res;
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds_h;
  ZK_CK(ntt_lds(ctx, (const void *)k_hoist, log_n, &lds_h));
  // Montgomery factors: a rotation carries R^-1 (one product with a key word), the inner sum one more product with a diagonal
  const RnsConst<NP> rc = rns_const<NP>(log_n), rc_inner = intt_const(log_n, 2), rc_outer = intt_const(log_n, 1);
  GadgetStep gs;
  for (int j = 0; j < NP; ++j) gs.step[j] = (uint32_t)((((uint64_t)1 << base_bits) % PRIMES[j]) * (((uint64_t)1 << 32) % PRIMES[j]) % PRIMES[j]);
  size_t baby_slots = 0;
  for (size_t k = 0; k < n_baby; ++k) baby_slots += elem[2 * k + 1] != NO_KEY;
  const double words = (double)NP * n;   // one polynomial at every prime
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo);
    ZK_CK(x.in(ctx, 0, lo, c, n, x_d));
    ZK_CK(x.in(ctx, 1, lo, c, n, x_d + c * n));
    zk_prof_begin(ctx);
    k_hoist<<<(unsigned)(c * rows * NP), NTT_THREADS, lds_h, ctx->stream>>>(x_d, c, l, base_bits, q, log_n, tw, rc, hst);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_HOIST, (double)c * rows * words * (8.0 + 4.0));
    const dim3 grid(zk_blocks(n, ACC_THREADS), NP, zk_blocks(c, CT));
    zk_prof_begin(ctx);   // the baby rotations stay in the transform domain
    k_linear_acc<ACC_MANY><<<grid, ACC_THREADS, 0, ctx->stream>>>(hst, elem_d, (int)n_baby, key_hat, nullptr, l, c, log_n, rc, gs, baby);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_LINEAR, 4.0 * words * ((double)n_baby * c * rows + (double)zk_blocks(c, CT) * 2.0 * baby_slots * l + 2.0 * n_baby * c));
    ZK_HIP(ctx, hipMemsetAsync(res, 0, 2 * c * n * NP * 4, ctx->stream));
    for (size_t g0 = 0; g0 < n_giant; g0 += group) {
      const size_t gg = std::min(group, n_giant - g0), inner_cts = gg * c;
      const uint32_t *dh = diag_hat + g0 * n_baby * NP * n;
      const int cti = c == 1 ? 1 : c == 2 ? 2 : 4;   // a single ciphertext (the tally) does not pay for a padded ciphertext tile
      zk_prof_begin(ctx);
      if (cti == 1)
        launch_bsgs_inner<8, 1>(ctx, baby, dh, n_baby, gg, c, log_n, rc, inner);
      else if (cti == 2)
        launch_bsgs_inner<4, 2>(ctx, baby, dh, n_baby, gg, c, log_n, rc, inner);
      else
        launch_bsgs_inner<4, 4>(ctx, baby, dh, n_baby, gg, c, log_n, rc, inner);
      ZK_LAUNCH_CHECK(ctx);
      // read: every baby word once per giant tile, every diagonal word once per ciphertext group; written: the inner sums
      zk_prof_end(ctx, ZKFHE_PROF_BFV_BSGS_INNER, 4.0 * words * ((double)zk_blocks(gg, cti == 1 ? 8 : 4) * 2.0 * n_baby * c + (double)zk_blocks(c, cti) * gg * n_baby + 2.0 * inner_cts));
      ZK_CK(zk_rns_intt(ctx, inner, 2 * inner_cts, log_n, rc_inner));
      ZK_CK(zk_bfv_eval_epilogue(ctx, inner, 2 * inner_cts, log_n, q, EvEpi{}, inner_q));   // [c0 | c1] of the gg c inner ciphertexts
      zk_prof_begin(ctx);
      k_hoist<<<(unsigned)(inner_cts * rows * NP), NTT_THREADS, lds_h, ctx->stream>>>(inner_q, inner_cts, l, base_bits, q, log_n, tw, rc, hst_in);
      ZK_LAUNCH_CHECK(ctx);
      zk_prof_end(ctx, ZKFHE_PROF_BFV_HOIST, (double)inner_cts * rows * words * (8.0 + 4.0));
      size_t giant_slots = 0;
      for (size_t k = 0; k < gg; ++k) giant_slots += elem[2 * (n_baby + g0 + k) + 1] != NO_KEY;
      zk_prof_begin(ctx);
      k_linear_acc<ACC_GIANT><<<grid, ACC_THREADS, 0, ctx->stream>>>(hst_in, elem_d + 2 * (n_baby + g0), (int)gg, key_hat, nullptr, l, c, log_n, rc, gs, res);
      ZK_LAUNCH_CHECK(ctx);
      // read: the hoisted rows of every inner ciphertext, every key word once per CT ciphertexts, the sum so far; written: the sum
      zk_prof_end(ctx, ZKFHE_PROF_BFV_BSGS_GIANT, 4.0 * words * ((double)inner_cts * rows + (double)zk_blocks(c, CT) * 2.0 * giant_slots * l + 4.0 * c));
    }
    ZK_CK(zk_rns_intt(ctx, res, 2 * c, log_n, rc_outer));
    ZK_CK(zk_bfv_eval_epilogue(ctx, res, 2 * c, log_n, q, EvEpi{}, o_d));
    ZK_CK(out.out(ctx, 0, lo, c, n, o_d));
    ZK_CK(out.out(ctx, 1, lo, c, n, o_d + c * n));
  }
  return ZKFHE_OK;
}

int bsgs_call(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, size_t n_baby,
              const uint64_t *g_baby, const uint64_t *bk0, const uint64_t *bk1, size_t n_giant, const uint64_t *g_giant, const uint64_t *hk0,
              const uint64_t *hk1, int base_bits, const uint64_t *diag, uint64_t *out0, uint64_t *out1) {
  const char *fn = "bfv_linear_transform_bsgs";
  const KeyLists ks{n_baby, n_giant, g_baby, bk0, bk1, g_giant, hk0, hk1};   // the baby elements, then the giant ones
  zkfhe_bfv_plan p;
  ZK_CK(prepare_head(ctx, params, ks, base_bits, true, true, fn, &p));
  ZK_CK(check_cts(ctx, p, n_cts, c0, c1, fn));
  ZK_CK(prepare_check(ctx, p, ks, diag, fn));
  int *flag;
  uint64_t *key_d, *diag_d;
  BsgsWork w;
  Arena a;
  add_prepared(a, p, flag, key_d, diag_d);
  add_bsgs_work(a, p, n_cts, w);
  ZK_CK(a.carve(ctx));
  ZK_CK(prepare_device(ctx, p, ks, diag, key_d, diag_d, flag));
  return bsgs_run(ctx, p, n_cts, host_planes(c0, c1), host_planes(out0, out1), w);
}

// the run half of a plan: its work buffers carved, then the chunk loop on host arrays or device planes
int plan_run(zkfhe_ctx *ctx, const zkfhe_bfv_plan &plan, size_t n_cts, const Planes &x, const Planes &out) {
  Arena a;
  if (plan.bsgs) {
    BsgsWork w;
    add_bsgs_work(a, plan, n_cts, w);
    ZK_CK(a.carve(ctx));
    return bsgs_run(ctx, plan, n_cts, x, out, w);
  }
  LinearWork w;
  add_linear_work(a, plan, n_cts, w);
  ZK_CK(a.carve(ctx));
  return linear_run(ctx, plan, n_cts, x, out, w);
}

// a plan's own buffers and the plan itself; hipFree waits for the device
void plan_free(zkfhe_bfv_plan *p) {
  if (!p) return;
  if (p->owned) (void)hipFree(p->elem_d), (void)hipFree(p->key_hat), (void)hipFree(p->diag_hat);
  delete p;
}

// words uint32_t of the plan's own (nullptr for none)
int plan_alloc(zkfhe_ctx *ctx, uint32_t **out, unsigned __int128 words, const char *fn) {
  if (!words) return ZKFHE_OK;
  if (words >> 60) return zk_fail_msg(ctx, ZKFHE_ENOMEM, std::string(fn) + ": out of device memory");
  const hipError_t e = hipMalloc(out, (size_t)words * 4);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return zk_fail_msg(ctx, ZKFHE_ENOMEM, std::string(fn) + ": out of device memory");
  }
  ZK_HIP(ctx, e);
  return ZKFHE_OK;
}

// The prepare half into allocations of the plan's own: the staging copies alone come from the arena.  The plan is complete, and
// readable from any stream of the device, when this returns.
int plan_fill(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const KeyLists &ks, int base_bits, bool bsgs, const uint64_t *diag, const char *fn,
              zkfhe_bfv_plan *p) {
  ZK_CK(prepare_head(ctx, params, ks, base_bits, bsgs, true, fn, p));
  ZK_CK(prepare_check(ctx, *p, ks, diag, fn));
  const uint64_t n = params->n;
  const size_t n_diag = p->n_diag;
  p->owned = true;
  unsigned __int128 total = 0;
  uint32_t **bufs[3] = {&p->elem_d, &p->key_hat, &p->diag_hat};
  for (int i = 0; i < 3; ++i) {
    const unsigned __int128 words = plan_words(n, p->l, ks.count(), p->slots, n_diag, i);
    ZK_CK(plan_alloc(ctx, bufs[i], words, fn));
    total += 4 * words;
  }
  p->device_bytes = (uint64_t)total;
  int *flag;
  uint64_t *key_d, *diag_d;
  ZK_CK(Arena().add(flag, 1).add(key_d, 2 * p->slots * p->l * n).add(diag_d, n_diag * n).carve(ctx));
  ZK_CK(prepare_device(ctx, *p, ks, diag, key_d, diag_d, flag));
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

int plan_create(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const KeyLists &ks, int base_bits, bool bsgs, const uint64_t *diag, const char *fn,
                zkfhe_bfv_plan **out) {
  zkfhe_bfv_plan *p = new zkfhe_bfv_plan;
  const int rc = plan_fill(ctx, params, ks, base_bits, bsgs, diag, fn, p);
  if (rc) {
    plan_free(p);
    return rc;
  }
  *out = p;
  return ZKFHE_OK;
}

}  // namespace

namespace zkrns {

void zk_bfv_plan_view(const zkfhe_bfv_plan *plan, zkfhe_bfv_params *params, int *device) {
  *params = plan->params;
  *device = plan->device;
}

int zk_bfv_plan_run_dev(zkfhe_ctx *ctx, const zkfhe_bfv_plan *plan, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                        uint64_t *out1) {
  return plan_run(ctx, *plan, n_cts, device_planes(c0, c1), device_planes(out0, out1));
}

int zk_rns_intt(zkfhe_ctx *ctx, uint32_t *res, size_t n_polys, int log_n, const RnsConst<NP_MAX> &rc) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds;
  ZK_CK(ntt_lds(ctx, (const void *)k_rns_intt, log_n, &lds));
  zk_prof_begin(ctx);
  k_rns_intt<<<(unsigned)(n_polys * NP), NTT_THREADS, lds, ctx->stream>>>(res, log_n, tw, rc);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_RNS_NTT, (double)n_polys * NP * 8.0 * ((size_t)1 << log_n));
  return ZKFHE_OK;
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_apply_galois_many(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1,
                                size_t n_elems, const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, int base_bits, uint64_t *out0,
                                uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && g && gk0 && gk1 && out0 && out1 && n_cts > 0 && n_elems > 0);
  return linear_call(ctx, params, n_cts, c0, c1, n_elems, g, gk0, gk1, base_bits, nullptr, out0, out1, "bfv_apply_galois_many");
}

int zkfhe_bfv_linear_transform(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1,
                               size_t n_elems, const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, int base_bits,
                               const uint64_t *diag, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && g && gk0 && gk1 && diag && out0 && out1 && n_cts > 0 && n_elems > 0);
  return linear_call(ctx, params, n_cts, c0, c1, n_elems, g, gk0, gk1, base_bits, diag, out0, out1, "bfv_linear_transform");
}

int zkfhe_bfv_linear_transform_bsgs(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1,
                                    size_t n_baby, const uint64_t *g_baby, const uint64_t *bk0, const uint64_t *bk1, size_t n_giant,
                                    const uint64_t *g_giant, const uint64_t *hk0, const uint64_t *hk1, int base_bits, const uint64_t *diag,
                                    uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && g_baby && bk0 && bk1 && g_giant && hk0 && hk1 && diag && out0 && out1 && n_cts > 0 && n_baby > 0 && n_giant > 0);
  return bsgs_call(ctx, params, n_cts, c0, c1, n_baby, g_baby, bk0, bk1, n_giant, g_giant, hk0, hk1, base_bits, diag, out0, out1);
}

int zkfhe_bfv_plan_create(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_elems, const uint64_t *g, const uint64_t *gk0,
                          const uint64_t *gk1, int base_bits, const uint64_t *diag, zkfhe_bfv_plan **out) {
  ZK_ENTER(ctx);
  if (out) *out = nullptr;
  if (!(ctx && g && gk0 && gk1 && diag && out && n_elems > 0))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_plan_create: a NULL argument or a zero count");
  const KeyLists ks{n_elems, 0, g, gk0, gk1, nullptr, nullptr, nullptr};
  return plan_create(ctx, params, ks, base_bits, false, diag, "bfv_plan_create", out);
}

int zkfhe_bfv_plan_create_bsgs(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_baby, const uint64_t *g_baby, const uint64_t *bk0,
                               const uint64_t *bk1, size_t n_giant, const uint64_t *g_giant, const uint64_t *hk0, const uint64_t *hk1,
                               int base_bits, const uint64_t *diag, zkfhe_bfv_plan **out) {
  ZK_ENTER(ctx);
  if (out) *out = nullptr;
  if (!(ctx && g_baby && bk0 && bk1 && g_giant && hk0 && hk1 && diag && out && n_baby > 0 && n_giant > 0))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_plan_create_bsgs: a NULL argument or a zero count");
  const KeyLists ks{n_baby, n_giant, g_baby, bk0, bk1, g_giant, hk0, hk1};
  return plan_create(ctx, params, ks, base_bits, true, diag, "bfv_plan_create_bsgs", out);
}

int zkfhe_bfv_plan_apply(zkfhe_ctx *ctx, const zkfhe_bfv_plan *plan, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                         uint64_t *out1) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_plan_apply";
  if (!(ctx && plan && c0 && c1 && out0 && out1 && n_cts > 0)) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a NULL argument or a zero count");
  if (ctx->device != plan->device)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": the plan lives on device " + std::to_string(plan->device) + " and the context on device " +
                                              std::to_string(ctx->device));
  ZK_CK(check_cts(ctx, *plan, n_cts, c0, c1, fn));
  return plan_run(ctx, *plan, n_cts, host_planes(c0, c1), host_planes(out0, out1));
}

int zkfhe_bfv_plan_info(const zkfhe_bfv_plan *plan, zkfhe_bfv_params *params, int *base_bits, size_t counts[3], uint64_t *device_bytes) {
  if (!plan) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_plan_info: plan is NULL");
  if (params) *params = plan->params;
  if (base_bits) *base_bits = plan->base_bits;
  if (counts) counts[0] = plan->n_baby, counts[1] = plan->n_giant, counts[2] = plan->slots;
  if (device_bytes) *device_bytes = plan->device_bytes;
  return ZKFHE_OK;
}

int zkfhe_bfv_plan_bytes(const zkfhe_bfv_params *params, int base_bits, size_t n_elems_total, size_t n_key_slots, size_t n_diagonals,
                         uint64_t *bytes) {
  if (!bytes) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_plan_bytes: bytes is NULL");
  ZK_CK(check_params(nullptr, params));
  int l = 0;
  ZK_CK(relin_rows(nullptr, params, base_bits, "bfv_plan_bytes", &l));
  // every term is below 2^64 2^6 2^15 2^4: the sum fits 128 bits
  unsigned __int128 total = 0;
  for (int i = 0; i < 3; ++i) total += 4 * plan_words(params->n, l, n_elems_total, n_key_slots, n_diagonals, i);
  if (total >> 64) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_plan_bytes: the size does not fit 64 bits");
  *bytes = (uint64_t)total;
  return ZKFHE_OK;
}

int zkfhe_bfv_plan_destroy(zkfhe_ctx *ctx, zkfhe_bfv_plan *plan) {
  ZK_ENTER(ctx);
  if (!plan) return ZKFHE_OK;
  if (ctx) ZK_HIP(ctx, zk_wait(ctx));   // what this context has queued against the plan
  plan_free(plan);
  return ZKFHE_OK;
}

}  // extern "C"
