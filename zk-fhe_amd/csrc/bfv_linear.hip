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
// Sizes: |r| < Q + l N (2^w - 1) Q < 2^116 for a rotation; the transform's sum is below n_elems N floor(T/2) times that, which the
// call bounds by 2^150 (check_range) under the half of the primes' product 2^151.2.  No kernel uses scratch.
#include <string>

#include "rns_ntt.hip.hpp"

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
// LINEAR = false: out[k][comp][ct][prime][index] = t_comp of element k.  LINEAR = true: out[comp][ct][prime][index] = sum_k p^_k t_comp.
// Every value is a residue below p < 2^31, every product a mont_mul and every sum an add_p: nothing is carried unreduced.
template <bool LINEAR>
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
  for (int t = 0; t < CT; ++t) acc0[t] = acc1[t] = 0;
  for (int k = 0; k < n_elems; ++k) {
    const uint32_t g = elem[2 * k], slot = elem[2 * k + 1];   // uniform over the grid
    const unsigned kp = galois_index(idx, g, log_n);
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
    if (LINEAR) {
      const uint32_t ph = diag_hat[((size_t)k * NP + j) * n + idx];
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        acc0[t] = add_p(acc0[t], mont_mul(t0[t], ph, p, pinv), p);
        acc1[t] = add_p(acc1[t], mont_mul(t1[t], ph, p, pinv), p);
      }
    } else {
      uint32_t *o = out + (size_t)k * 2 * c * plane + (size_t)j * n + idx;
#pragma unroll
      for (int t = 0; t < CT; ++t)
        if (ct0 + t < c) o[(ct0 + t) * plane] = t0[t], o[(c + ct0 + t) * plane] = t1[t];
    }
  }
  if (LINEAR) {
    uint32_t *o = out + (size_t)j * n + idx;
#pragma unroll
    for (int t = 0; t < CT; ++t)
      if (ct0 + t < c) o[(ct0 + t) * plane] = acc0[t], o[(c + ct0 + t) * plane] = acc1[t];
  }
}

// One workgroup per (polynomial, prime) of res ([polys][NP][N]): the inverse transform in place, times scale[prime]
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

// both calls: diag == nullptr is apply_galois_many
int linear_call(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, size_t n_elems,
                const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, int base_bits, const uint64_t *diag, uint64_t *out0,
                uint64_t *out1, const char *fn) {
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  const uint64_t n = params->n, q = params->q;
  if (n_elems >> 20) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": more than 2^20 Galois elements");
  for (size_t k = 0; k < n_elems; ++k)
    if (!(g[k] & 1) || g[k] >= 2 * n) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": every Galois element g must be odd and below 2N");
  if (diag) ZK_CK(check_range(ctx, params, n_elems, l, base_bits, fn));   // before any O(n) pass and any device work
  const int log_n = bit_log2(n);
  const size_t lw = (size_t)l * n;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, fn, "a ciphertext", c1));
  std::vector<uint32_t> elem(2 * n_elems);
  size_t slots = 0;
  for (size_t k = 0; k < n_elems; ++k) {   // the key rows of g = 1 are neither read nor checked
    elem[2 * k] = (uint32_t)g[k];
    elem[2 * k + 1] = g[k] == 1 ? NO_KEY : (uint32_t)slots++;
    if (g[k] != 1) ZK_CK(check_below_q(ctx, gk0 + k * lw, lw, q, fn, "a Galois-key", gk1 + k * lw));
  }
  if (diag) ZK_CK(check_plain(ctx, diag, n_elems * n, q, params->t, fn, "a diagonal"));

  const size_t rows = (size_t)l + 1, per_ct = diag ? 2 : 2 * n_elems;   // output polynomials per ciphertext
  const size_t chunk = chunk_cts(n, n_cts, std::max(rows, per_ct)), cw = chunk * n;
  int *flag;
  uint64_t *key_d, *diag_d, *x_d, *o_d;
  uint32_t *key_hat, *diag_hat, *elem_d, *hst, *res;
  ZK_CK(Arena().add(flag, 1).add(elem_d, 2 * n_elems).add(key_d, 2 * slots * lw).add(key_hat, 2 * slots * lw * NP)
            .add(diag_d, diag ? n_elems * n : 0).add(diag_hat, diag ? n_elems * n * NP : 0).add(x_d, 2 * cw).add(hst, rows * cw * NP)
            .add(res, per_ct * cw * NP).add(o_d, per_ct * cw).carve(ctx));
  ZK_CK(zkfhe_upload(ctx, elem_d, elem.data(), elem.size() * 4));
  for (size_t k = 0; k < n_elems; ++k) {   // key slot s: its gk0 rows, then its gk1 rows
    if (elem[2 * k + 1] == NO_KEY) continue;
    ZK_CK(zkfhe_upload(ctx, key_d + (size_t)elem[2 * k + 1] * 2 * lw, gk0 + k * lw, lw * 8));
    ZK_CK(zkfhe_upload(ctx, key_d + ((size_t)elem[2 * k + 1] * 2 + 1) * lw, gk1 + k * lw, lw * 8));
  }
  if (slots) ZK_CK(launch_rns_ntt<NP>(ctx, false, key_d, LOAD_RESIDUE, q, 2 * slots * l, log_n, nullptr, 0, key_hat, flag));
  if (diag) {
    ZK_CK(zkfhe_upload(ctx, diag_d, diag, n_elems * n * 8));
    ZK_CK(launch_rns_ntt<NP>(ctx, false, diag_d, LOAD_CENTRED, q, n_elems, log_n, nullptr, 0, diag_hat, flag));
  }
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds_h, lds_i;
  ZK_CK(ntt_lds(ctx, (const void *)k_hoist, log_n, &lds_h));
  ZK_CK(ntt_lds(ctx, (const void *)k_rns_intt, log_n, &lds_i));
  const RnsConst<NP> rc = rns_const<NP>(log_n), rc_inv = intt_const(log_n, diag ? 2 : 1);
  GadgetStep gs;
  for (int j = 0; j < NP; ++j) gs.step[j] = (uint32_t)((((uint64_t)1 << base_bits) % PRIMES[j]) * (((uint64_t)1 << 32) % PRIMES[j]) % PRIMES[j]);
  const double words = (double)NP * n;   // one polynomial at every prime
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8, polys = per_ct * c;
    ZK_CK(zkfhe_upload(ctx, x_d, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, x_d + c * n, c1 + lo * n, bytes));
    zk_prof_begin(ctx);
    k_hoist<<<(unsigned)(c * rows * NP), NTT_THREADS, lds_h, ctx->stream>>>(x_d, c, l, base_bits, q, log_n, tw, rc, hst);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_HOIST, (double)c * rows * words * (8.0 + 4.0));
    const dim3 grid(zk_blocks(n, ACC_THREADS), NP, zk_blocks(c, CT));
    zk_prof_begin(ctx);
    if (diag)
      k_linear_acc<true><<<grid, ACC_THREADS, 0, ctx->stream>>>(hst, elem_d, (int)n_elems, key_hat, diag_hat, l, c, log_n, rc, gs, res);
    else
      k_linear_acc<false><<<grid, ACC_THREADS, 0, ctx->stream>>>(hst, elem_d, (int)n_elems, key_hat, nullptr, l, c, log_n, rc, gs, res);
    ZK_LAUNCH_CHECK(ctx);
    // read: every hoisted row per element, every key word once per CT ciphertexts, the diagonals likewise; written: the outputs
    zk_prof_end(ctx, ZKFHE_PROF_BFV_LINEAR, 4.0 * words * ((double)n_elems * c * rows + (double)zk_blocks(c, CT) * (2.0 * slots * l + (diag ? n_elems : 0)) + polys));
    zk_prof_begin(ctx);
    k_rns_intt<<<(unsigned)(polys * NP), NTT_THREADS, lds_i, ctx->stream>>>(res, log_n, tw, rc_inv);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_RNS_NTT, (double)polys * words * 8.0);
    ZK_CK(zk_bfv_eval_epilogue(ctx, res, polys, log_n, q, EvEpi{}, o_d));
    for (size_t k = 0; k < (diag ? 1 : n_elems); ++k) {   // o_d: [element][component][c][N]
      ZK_CK(zkfhe_download(ctx, out0 + (k * n_cts + lo) * n, o_d + 2 * k * c * n, bytes));
      ZK_CK(zkfhe_download(ctx, out1 + (k * n_cts + lo) * n, o_d + (2 * k + 1) * c * n, bytes));
    }
  }
  return ZKFHE_OK;
}

}  // namespace

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

}  // extern "C"
