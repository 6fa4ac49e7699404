// BFV slot batching and Galois automorphisms on the GPU (zkfhe.h, INTEGRATION.md "Slots and rotations").  Conventions of bfv_enc.hip:
// host arrays, N residues in [0, Q) per polynomial, CircuitInput order (position N - 1 - d holds degree d).
//
// sigma_g(m)(x) = m(x^g) mod (x^N + 1) for odd g < 2N moves degree i to i g mod 2N, negated and placed at i g - N past N.  Read
// backwards, degree d of sigma_g(v) is degree j = d g^-1 mod 2N of v if j < N, else minus degree j - N (auto_coeff): a gather whose
// addresses depend on g (public) and never on a coefficient's value.
//   k_gal_switch    k_bfv_relin (bfv_eval.hip) whose digit load reads sigma_g(c1): per (ciphertext, prime), every digit
//                   d_i = (sigma_g(c1) >> i w) & (2^w - 1) is transformed with the five primes, multiplied by the transformed
//                   gk0_i and gk1_i and accumulated; one inverse transform per component (sum < l N 2^w Q < 2^116)
//   k_gal_epilogue  Garner over the five primes, x mod Q, + sigma_g(c0) on component 0, + x_in when set (slot_sum's
//                   x <- x + apply_galois(x), fused: the same sums mod Q as zkfhe_bfv_add)
// The Galois key is transformed once per call; slot_sum transforms all log2(N) keys once and runs every step on device buffers.
// Galois keys (and their threshold shares) are products a_j s with a ternary s: the three-prime k_rns_ntt against the transform of
// s, then k_gal_key_epilogue: 2^(j w) sigma_g(s) - a_j s - e_j mod Q.
//
// Slots (T prime below 2^31, 2N | T - 1): k_slot_ntt is one LDS NTT mod T per polynomial with rns_forward / rns_inverse and the
// Montgomery helpers of rns_ntt.hip.hpp, on a table for T built on the host and cached in the context per (T, N): psi = zeta =
// r^((T - 1) / 2N) (r the smallest primitive root mod T), so NTT index k holds m(zeta^(2 br(k) + 1)), and the slot of that
// exponent (slot p = row N/2 + j is the evaluation at zeta^((-1)^row 5^j)).  No kernel uses scratch.
#include <string>

#include "rns_ntt.hip.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;   // the key switch: five primes, as k_bfv_relin
constexpr int NP3 = 3;       // the keys: a ternary factor, three primes
constexpr int K_UNIFORM = 1, K_ERROR = 2;   // zk_bfv_sample kinds
constexpr uint32_t DOM_GK_A = 14, DOM_GK_E = 15;   // ChaCha20 domains of a_j and e_j, index g 64 + j

__device__ __forceinline__ uint64_t sub_q(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }

// degree d of sigma_g(v), v one polynomial in CircuitInput order, ginv = g^-1 mod 2N
__device__ __forceinline__ uint64_t auto_coeff(const uint64_t *__restrict__ v, unsigned d, unsigned ginv, unsigned n, uint64_t q) {
  const unsigned j = (d * ginv) & (2 * n - 1);   // d ginv < 2^15 2^16
  const uint64_t x = v[n - 1 - (j & (n - 1))];
  return j >= n && x ? q - x : x;
}

// One workgroup per (ciphertext, prime), blockIdx.x = k * NP + prime: k_bfv_relin with the digits of sigma_g(c1).  c1: [c][N];
// key_hat: [2 l][NP][N] (the gk0_i, then the gk1_i); acc[0][k][prime] and acc[1][k][prime] receive the two sums, transformed back.
__global__ __launch_bounds__(NTT_THREADS) void k_gal_switch(const uint64_t *__restrict__ c1, unsigned ginv, uint64_t q, int l, int w,
                                                            const uint32_t *__restrict__ key_hat, size_t c, int log_n,
                                                            const uint32_t *__restrict__ tw, RnsConst<NP> rc, uint32_t *__restrict__ acc) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t k = blockIdx.x / NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n;
  const uint32_t *fw = tw + (size_t)j * 2 * NMAX, *iv = fw + NMAX;
  uint32_t *acc0 = acc + k * plane + (size_t)j * n, *acc1 = acc0 + c * plane;
  const uint64_t *s = c1 + k * n, mask = ((uint64_t)1 << w) - 1;
  for (int i = 0; i < l; ++i) {
    const int shift = i * w;   // < bitlen(Q - 1) <= 63
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = (uint32_t)(((auto_coeff(s, d, ginv, n, q) >> shift) & mask) % p);
    __syncthreads();
    rns_forward(lds, fw, log_n, p, pinv);
    const uint32_t *r0 = key_hat + (size_t)i * plane + (size_t)j * n, *r1 = key_hat + (size_t)(l + i) * plane + (size_t)j * n;
    for (unsigned d = tid; d < n; d += NTT_THREADS) {
      const uint32_t x = lds[d], u0 = mont_mul(x, r0[d], p, pinv), u1 = mont_mul(x, r1[d], p, pinv);
      acc0[d] = i ? add_p(acc0[d], u0, p) : u0;
      acc1[d] = i ? add_p(acc1[d], u1, p) : u1;
    }
    __syncthreads();
  }
  for (int comp = 0; comp < 2; ++comp) {
    uint32_t *a = comp ? acc1 : acc0;
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = a[d];
    __syncthreads();
    rns_inverse(lds, iv, log_n, p, pinv);
    for (unsigned d = tid; d < n; d += NTT_THREADS) a[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
    __syncthreads();
  }
}

// One thread per output coefficient of res ([2 c][NP][N]: the sums of k_gal_switch, component 0 of the c ciphertexts, then
// component 1): x mod Q, + sigma_g(c0) for component 0 (c0: [c][N]), + x_in[pos] if x_in is set.  x_in, out: [2 c][N].
__global__ __launch_bounds__(256) void k_gal_epilogue(const uint32_t *__restrict__ res, size_t c, int log_n, uint64_t q, Crt5 cc,
                                                      const uint64_t *__restrict__ c0, unsigned ginv, const uint64_t *__restrict__ x_in,
                                                      uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (2 * c) << log_n) return;
  const size_t n = (size_t)1 << log_n, poly = g >> log_n, d = g & (n - 1), pos = poly * n + (n - 1 - d);
  uint64_t m[3];
  bool neg;
  crt5(res + poly * NP * n + d, n, cc, m, neg);
  const uint64_t rm = mod128(mod128(m[2], m[1], q), m[0], q);
  uint64_t v = neg && rm ? q - rm : rm;
  if (poly < c) v = add_q(v, auto_coeff(c0 + poly * n, (unsigned)d, ginv, (unsigned)n, q), q);
  if (x_in) v = add_q(v, x_in[pos], q);
  out[pos] = v;
}

// One thread per coefficient of l key rows (res: [l][3][N], the products a_j s): out_j = 2^(j w) sigma_g(s) - (a_j s + e_j) mod Q.
// s in {0, 1, Q - 1} selects 0, 2^(j w) or Q - 2^(j w) without a branch (as THR_GADGET of bfv_threshold.hip).
__global__ __launch_bounds__(256) void k_gal_key_epilogue(const uint32_t *__restrict__ res, size_t total, int log_n, uint64_t q, CrtConst cc,
                                                          const uint64_t *__restrict__ e, const uint64_t *__restrict__ s, unsigned ginv, int w,
                                                          uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t n = (size_t)1 << log_n, row = g >> log_n, d = g & (n - 1), pos = row * n + (n - 1 - d);
  const uint64_t v = crt3_mod_q(res + row * NP3 * n + d, n, q, cc);
  const uint64_t pw = (uint64_t)1 << (row * w), sv = auto_coeff(s, (unsigned)d, ginv, (unsigned)n, q);   // j w < bitlen(Q - 1)
  const uint64_t gs = sv == 1 ? pw : (sv == q - 1 ? q - pw : 0);
  out[pos] = sub_q(gs, add_q(v, e[pos], q), q);
}

// One workgroup per polynomial (see the top of the file).  tab: [fwd | inv | slot of NTT index][N] of T.
// decode = 0: in holds slot values in [0, T); NTT index k takes the value of its slot, the inverse transform and the scale by N^-1
//   give the coefficients mod T, written centred (x > T/2: Q - (T - x)) at out[N - 1 - d].
// decode = 1: in holds plaintexts in [0, T/2] or [Q - T/2, Q - 1], read as residues mod T; the forward transform gives the value
//   of every slot, written to out[slot].
__global__ __launch_bounds__(NTT_THREADS) void k_slot_ntt(const uint64_t *__restrict__ in, int decode, int log_n, uint64_t q, uint32_t t,
                                                          uint32_t pinv, uint32_t n_inv, const uint32_t *__restrict__ tab,
                                                          uint64_t *__restrict__ out) {
  extern __shared__ uint32_t lds[];
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint64_t *src = in + (size_t)blockIdx.x * n;
  uint64_t *dst = out + (size_t)blockIdx.x * n;
  const uint32_t *fw = tab, *iv = tab + n, *slot = tab + 2 * n;
  if (!decode) {
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = (uint32_t)src[slot[d]];
    __syncthreads();
    rns_inverse(lds, iv, log_n, t, pinv);
    for (unsigned d = tid; d < n; d += NTT_THREADS) {
      const uint32_t x = mont_mul(lds[d], n_inv, t, pinv);
      dst[n - 1 - d] = x > t / 2 ? q - (t - x) : x;
    }
    return;
  }
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    const uint64_t v = src[n - 1 - d];
    lds[d] = (uint32_t)(v > t / 2 ? t - (q - v) : v);   // q - v <= T/2
  }
  __syncthreads();
  rns_forward(lds, fw, log_n, t, pinv);
  for (unsigned d = tid; d < n; d += NTT_THREADS) dst[slot[d]] = lds[d];
}

// ------------------------------------------------------------------------------------------------------------------ host side

bool is_prime(uint64_t t) {
  if (t < 2) return false;
  for (uint64_t f = 2; f * f <= t; ++f)
    if (t % f == 0) return false;
  return true;
}

bool batching(uint64_t t, uint64_t n) { return t < ((uint64_t)1 << 31) && (t - 1) % (2 * n) == 0 && is_prime(t); }

int check_batching(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const char *fn) {
  if (!batching(params->t, params->n))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": T must be a prime below 2^31 with 2N | T - 1 (a batching modulus)");
  return ZKFHE_OK;
}

int check_g(zkfhe_ctx *ctx, uint64_t n, uint64_t g, const char *fn) {
  if (!(g & 1) || g >= 2 * n) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": the Galois element g must be odd and below 2N");
  return ZKFHE_OK;
}

int check_base_bits(zkfhe_ctx *ctx, int base_bits, const char *fn) {
  if (base_bits < 1 || base_bits > 32) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": base_bits must be in [1, 32]");
  return ZKFHE_OK;
}

int check_below_q(zkfhe_ctx *ctx, const uint64_t *v, size_t count, uint64_t q, const char *fn, const char *what) {
  for (size_t i = 0; i < count; ++i)
    if (v[i] >= q) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": " + what + " coefficient is not below Q");
  return ZKFHE_OK;
}

// g^-1 mod 2N: the units mod 2N form a group of order N
unsigned galois_inv(uint64_t g, uint64_t n) { return (unsigned)pow_mod(g, n - 1, 2 * n); }

// 5^k mod 2N for k >= 0 (k < N/2 suffices: 5 has order N/2)
uint64_t pow5(uint64_t k, uint64_t n) { return pow_mod(5, k, 2 * n); }

unsigned bitrev(unsigned k, int bits) {
  unsigned r = 0;
  for (int i = 0; i < bits; ++i) r |= ((k >> i) & 1) << (bits - 1 - i);
  return r;
}

// the slot tables of (T, N), built on first use (T a batching modulus)
int slot_tables(zkfhe_ctx *ctx, uint64_t t, uint64_t n, const zkfhe_ctx::SlotTables **out) {
  auto it = ctx->slot_tw.find({t, n});
  if (it == ctx->slot_tw.end()) {
    std::vector<uint64_t> factors;   // the distinct primes of T - 1
    uint64_t rest = t - 1;
    for (uint64_t f = 2; f * f <= rest; ++f)
      if (rest % f == 0) {
        factors.push_back(f);
        while (rest % f == 0) rest /= f;
      }
    if (rest > 1) factors.push_back(rest);
    uint64_t r = 2;
    for (;; ++r) {
      bool prim = true;
      for (uint64_t f : factors) prim = prim && pow_mod(r, (t - 1) / f, t) != 1;
      if (prim) break;
    }
    const int log_n = bit_log2(n);
    const uint64_t zeta = pow_mod(r, (t - 1) / (2 * n), t), zinv = pow_mod(zeta, t - 2, t), R = ((uint64_t)1 << 32) % t;
    std::vector<uint32_t> slot_of(2 * n, 0), h(3 * n);
    for (uint64_t j = 0, e = 1; j < n / 2; ++j, e = e * 5 % (2 * n)) slot_of[e] = (uint32_t)j, slot_of[2 * n - e] = (uint32_t)(n / 2 + j);
    for (unsigned k = 0; k < n; ++k) {
      const unsigned br = bitrev(k, log_n);
      h[k] = (uint32_t)(pow_mod(zeta, br, t) * R % t);
      h[n + k] = (uint32_t)(pow_mod(zinv, br, t) * R % t);
      h[2 * n + k] = slot_of[2 * br + 1];
    }
    zkfhe_ctx::SlotTables st;
    uint32_t inv = 1;   // t^-1 mod 2^32 by Newton
    for (int i = 0; i < 5; ++i) inv *= 2 - (uint32_t)t * inv;
    st.pinv = 0u - inv;
    st.n_inv = (uint32_t)(pow_mod(n, t - 2, t) * R % t);
    void *d;
    ZK_HIP(ctx, hipMalloc(&d, h.size() * 4));
    const hipError_t e = hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return zk_fail(ctx, ZKFHE_EHIP, "hipMemcpy", e, __FILE__, __LINE__);
    }
    st.dev = (uint32_t *)d;
    it = ctx->slot_tw.emplace(std::make_pair(t, n), st).first;   // freed with the context
  }
  *out = &it->second;
  return ZKFHE_OK;
}

// encode (decode = 0) or decode n_polys polynomials of N words
int slot_transform(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_polys, const uint64_t *in, int decode, uint64_t *out) {
  const uint64_t n = params->n, q = params->q, t = params->t;
  const int log_n = bit_log2(n);
  const zkfhe_ctx::SlotTables *st;
  ZK_CK(slot_tables(ctx, t, n, &st));
  const size_t chunk = std::min<size_t>(n_polys, chunk_polys(n)), cvec = align256(chunk * n * 8);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 2 * cvec, &w));
  uint64_t *in_d = (uint64_t *)w, *o_d = (uint64_t *)(w + cvec);
  const int lds = 4 << log_n;
  if (lds > 64 * 1024) ZK_CK(zk_func_max_lds(ctx, (const void *)k_slot_ntt, 4 << LOG_NMAX));
  for (size_t lo = 0; lo < n_polys; lo += chunk) {
    const size_t c = std::min(chunk, n_polys - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, in_d, in + lo * n, bytes));
    zk_prof_begin(ctx);
    k_slot_ntt<<<(unsigned)c, NTT_THREADS, lds, ctx->stream>>>(in_d, decode, log_n, q, (uint32_t)t, st->pinv, st->n_inv, st->dev, o_d);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_SLOT_NTT, (double)c * n * (8.0 + 4.0 + 8.0));
    ZK_CK(zkfhe_download(ctx, out + lo * n, o_d, bytes));
  }
  return ZKFHE_OK;
}

// one key switch of c ciphertexts: x_d = [c0 | c1] ([2 c][N]), key_hat: [2 l][NP][N]; out_d = [sigma_g(c0) + ks0 | ks1] (+ x_d)
int launch_galois(zkfhe_ctx *ctx, const uint64_t *x_d, size_t c, int log_n, uint64_t q, uint64_t g, int l, int w, const uint32_t *key_hat,
                  bool accumulate, uint32_t *acc, uint64_t *out_d) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  const uint64_t n = (uint64_t)1 << log_n;
  const unsigned ginv = galois_inv(g, n);
  const int lds = 4 << log_n;
  if (lds > 64 * 1024) ZK_CK(zk_func_max_lds(ctx, (const void *)k_gal_switch, 4 << LOG_NMAX));
  zk_prof_begin(ctx);
  k_gal_switch<<<(unsigned)(c * NP), NTT_THREADS, lds, ctx->stream>>>(x_d + c * n, ginv, q, l, w, key_hat, c, log_n, tw, rns_const<NP>(log_n), acc);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_GALOIS, (double)c * NP * (l * (8.0 + 8.0 + 16.0) + 16.0) * n);
  const size_t total = 2 * c * n;
  zk_prof_begin(ctx);
  k_gal_epilogue<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(acc, c, log_n, q, crt5_const(), x_d, ginv, accumulate ? x_d : nullptr, out_d);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_GALOIS, (double)total * (NP * 4 + 8 + (accumulate ? 8 : 0)) + (double)c * n * 8);
  return ZKFHE_OK;
}

// r_j = 2^(j w) sigma_g(s) - (a_j s + e_j) mod Q, j < l: a_j uniform from (crs_seed, 14, g 64 + j), e_j an error sample from
// (party_seed, 15, g 64 + j)
int galois_key(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t crs_seed[32], const uint8_t party_seed[32],
               uint64_t g, int base_bits, uint64_t *r_out, uint64_t *a_out, const char *fn) {
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_g(ctx, params->n, g, fn));
  ZK_CK(check_base_bits(ctx, base_bits, fn));
  size_t rows = 0;
  ZK_CK(zkfhe_bfv_relin_digits(params, base_bits, &rows));
  const int l = (int)rows;
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  zk_bfv_error_cdt(params->b, cdt.data());
  const size_t vec = align256(n * 8), lvec = align256((size_t)l * n * 8), plane = align256((size_t)NP3 * n * 4);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + vec + 3 * lvec + align256(n_cdt * 8) + plane + align256((size_t)l * NP3 * n * 4), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *s_d = (uint64_t *)take(vec), *a_d = (uint64_t *)take(lvec), *e_d = (uint64_t *)take(lvec), *r_d = (uint64_t *)take(lvec);
  uint64_t *cdt_d = (uint64_t *)take(align256(n_cdt * 8));
  uint32_t *hat = (uint32_t *)take(plane), *res = (uint32_t *)take(align256((size_t)l * NP3 * n * 4));
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, s_d, sk, n * 8));
  ZK_CK(launch_rns_ntt<NP3>(ctx, false, s_d, LOAD_TERNARY, q, 1, log_n, nullptr, 0, hat, flag));
  int bad = 0;
  ZK_CK(zkfhe_download(ctx, &bad, flag, 4));
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a secret-key coefficient is not in {0, 1, Q - 1}");
  ZK_CK(zkfhe_upload(ctx, cdt_d, cdt.data(), n_cdt * 8));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, DOM_GK_A, g * 64, K_UNIFORM, l, log_n, q, nullptr, 0, a_d));
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_GK_E, g * 64, K_ERROR, l, log_n, q, cdt_d, n_cdt, e_d));
  ZK_CK(launch_rns_ntt<NP3>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat, 0, res, flag));
  const size_t total = (size_t)l * n;
  zk_prof_begin(ctx);
  k_gal_key_epilogue<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(res, total, log_n, q, crt3_const(), e_d, s_d, galois_inv(g, n), base_bits, r_d);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_RNS_EPILOGUE, (double)total * (12 + 8 + 8 + 8));
  ZK_CK(zkfhe_download(ctx, r_out, r_d, total * 8));
  ZK_CK(zkfhe_download(ctx, a_out, a_d, total * 8));
  return ZKFHE_OK;
}

}  // namespace

extern "C" {

int zkfhe_bfv_slot_count(const zkfhe_bfv_params *params, size_t *slots) {
  if (!slots) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_slot_count: slots is NULL");
  ZK_CK(zk_bfv_check_params(nullptr, params));
  ZK_CK(check_batching(nullptr, params, "bfv_slot_count"));
  *slots = (size_t)params->n;
  return ZKFHE_OK;
}

int zkfhe_bfv_galois_element(const zkfhe_bfv_params *params, int64_t steps, int swap_rows, uint64_t *g) {
  if (!g) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_galois_element: g is NULL");
  ZK_CK(zk_bfv_check_params(nullptr, params));
  const uint64_t n = params->n;
  const int64_t half = (int64_t)(n / 2), k = ((steps % half) + half) % half;
  const uint64_t r = pow5((uint64_t)k, n);
  *g = swap_rows ? r * (2 * n - 1) % (2 * n) : r;
  return ZKFHE_OK;
}

int zkfhe_bfv_slot_sum_elements(const zkfhe_bfv_params *params, uint64_t *g, size_t *count) {
  if (!count) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_slot_sum_elements: count is NULL");
  ZK_CK(zk_bfv_check_params(nullptr, params));
  const uint64_t n = params->n;
  const int log_n = bit_log2(n);
  *count = (size_t)log_n;
  if (g) {
    for (int k = 0; k + 1 < log_n; ++k) g[k] = pow5((uint64_t)1 << k, n);
    g[log_n - 1] = 2 * n - 1;
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_encode_slots(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_polys, const uint64_t *values, uint64_t *m_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && values && m_out && n_polys > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_batching(ctx, params, "bfv_encode_slots"));
  bool bad = false;
  for (size_t i = 0; i < n_polys * params->n; ++i) bad |= values[i] >= params->t;
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_encode_slots: a slot value is not below T");
  return slot_transform(ctx, params, n_polys, values, 0, m_out);
}

int zkfhe_bfv_decode_slots(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_polys, const uint64_t *m, uint64_t *values_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && m && values_out && n_polys > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_batching(ctx, params, "bfv_decode_slots"));
  const uint64_t q = params->q, half = params->t / 2;
  bool bad = false;   // without a branch per word: plaintext signs are random
  for (size_t i = 0; i < n_polys * params->n; ++i) bad |= (m[i] > half) & ((m[i] >= q) | (m[i] < q - half));
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_decode_slots: a plaintext coefficient is outside [0, T/2] and [Q - T/2, Q - 1]");
  return slot_transform(ctx, params, n_polys, m, 1, values_out);
}

int zkfhe_bfv_galois_keygen(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t seed[32], uint64_t g,
                            int base_bits, uint64_t *gk0_out, uint64_t *gk1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && seed && gk0_out && gk1_out);
  return galois_key(ctx, params, sk, seed, seed, g, base_bits, gk0_out, gk1_out, "bfv_galois_keygen");
}

int zkfhe_bfv_galois_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t crs_seed[32],
                           const uint8_t party_seed[32], uint64_t g, int base_bits, uint64_t *r_out, uint64_t *a_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && crs_seed && party_seed && r_out && a_out);
  return galois_key(ctx, params, sk_i, crs_seed, party_seed, g, base_bits, r_out, a_out, "bfv_galois_share");
}

int zkfhe_bfv_apply_galois(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t g,
                           const uint64_t *gk0, const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && gk0 && gk1 && out0 && out1 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_g(ctx, params->n, g, "bfv_apply_galois"));
  ZK_CK(check_base_bits(ctx, base_bits, "bfv_apply_galois"));
  const uint64_t n = params->n, q = params->q;
  size_t rows = 0;
  ZK_CK(zkfhe_bfv_relin_digits(params, base_bits, &rows));
  const int log_n = bit_log2(n), l = (int)rows;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_apply_galois", "a ciphertext"));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_apply_galois", "a ciphertext"));
  ZK_CK(check_below_q(ctx, gk0, (size_t)l * n, q, "bfv_apply_galois", "a Galois-key"));
  ZK_CK(check_below_q(ctx, gk1, (size_t)l * n, q, "bfv_apply_galois", "a Galois-key"));
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + align256(2 * l * n * 8) + align256(2 * l * plane) + 2 * align256(2 * chunk * n * 8) + align256(2 * chunk * plane), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += align256(bytes); return r; };
  uint64_t *key_d = (uint64_t *)take(2 * l * n * 8);
  uint32_t *key_hat = (uint32_t *)take(2 * l * plane);
  uint64_t *x_d = (uint64_t *)take(2 * chunk * n * 8), *o_d = (uint64_t *)take(2 * chunk * n * 8);
  uint32_t *acc = (uint32_t *)take(2 * chunk * plane);
  ZK_CK(zkfhe_upload(ctx, key_d, gk0, (size_t)l * n * 8));
  ZK_CK(zkfhe_upload(ctx, key_d + (size_t)l * n, gk1, (size_t)l * n * 8));
  ZK_CK(launch_rns_ntt<NP>(ctx, false, key_d, LOAD_RESIDUE, q, 2 * l, log_n, nullptr, 0, key_hat, flag));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, x_d, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, x_d + c * n, c1 + lo * n, bytes));
    ZK_CK(launch_galois(ctx, x_d, c, log_n, q, g, l, base_bits, key_hat, false, acc, o_d));
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, o_d, bytes));
    ZK_CK(zkfhe_download(ctx, out1 + lo * n, o_d + c * n, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_slot_sum(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, const uint64_t *gk0,
                       const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && gk0 && gk1 && out0 && out1 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_base_bits(ctx, base_bits, "bfv_slot_sum"));
  const uint64_t n = params->n, q = params->q;
  size_t rows = 0, steps = 0;
  ZK_CK(zkfhe_bfv_relin_digits(params, base_bits, &rows));
  ZK_CK(zkfhe_bfv_slot_sum_elements(params, nullptr, &steps));
  std::vector<uint64_t> gs(steps);
  ZK_CK(zkfhe_bfv_slot_sum_elements(params, gs.data(), &steps));
  const int log_n = bit_log2(n), l = (int)rows;
  const size_t kw = (size_t)l * n;   // words of one key half
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_slot_sum", "a ciphertext"));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_slot_sum", "a ciphertext"));
  ZK_CK(check_below_q(ctx, gk0, steps * kw, q, "bfv_slot_sum", "a Galois-key"));
  ZK_CK(check_below_q(ctx, gk1, steps * kw, q, "bfv_slot_sum", "a Galois-key"));
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + align256(2 * steps * kw * 8) + align256(2 * steps * l * plane) + 2 * align256(2 * chunk * n * 8) +
                                   align256(2 * chunk * plane), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += align256(bytes); return r; };
  uint64_t *key_d = (uint64_t *)take(2 * steps * kw * 8);
  uint32_t *key_hat = (uint32_t *)take(2 * steps * l * plane);
  uint64_t *x_d = (uint64_t *)take(2 * chunk * n * 8), *y_d = (uint64_t *)take(2 * chunk * n * 8);
  uint32_t *acc = (uint32_t *)take(2 * chunk * plane);
  for (size_t k = 0; k < steps; ++k) {   // key k: its gk0 rows, then its gk1 rows
    ZK_CK(zkfhe_upload(ctx, key_d + 2 * k * kw, gk0 + k * kw, kw * 8));
    ZK_CK(zkfhe_upload(ctx, key_d + (2 * k + 1) * kw, gk1 + k * kw, kw * 8));
  }
  ZK_CK(launch_rns_ntt<NP>(ctx, false, key_d, LOAD_RESIDUE, q, 2 * steps * l, log_n, nullptr, 0, key_hat, flag));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    uint64_t *x = x_d, *y = y_d;
    ZK_CK(zkfhe_upload(ctx, x, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, x + c * n, c1 + lo * n, bytes));
    for (size_t k = 0; k < steps; ++k) {   // x <- x + apply_galois(x, g_k), on the device
      ZK_CK(launch_galois(ctx, x, c, log_n, q, gs[k], l, base_bits, key_hat + 2 * k * l * (plane / 4), true, acc, y));
      std::swap(x, y);
    }
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, x, bytes));
    ZK_CK(zkfhe_download(ctx, out1 + lo * n, x + c * n, bytes));
  }
  return ZKFHE_OK;
}

}  // extern "C"
