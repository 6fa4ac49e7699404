// BFV slot batching and Galois automorphisms on the GPU (zkfhe.h, INTEGRATION.md "Slots and rotations").  Conventions of bfv_enc.hip:
// host arrays, N residues in [0, Q) per polynomial, CircuitInput order (position N - 1 - d holds degree d).
//
// sigma_g(m)(x) = m(x^g) mod (x^N + 1) for odd g < 2N moves degree i to i g mod 2N, negated and placed at i g - N past N.  Read
// backwards, degree d of sigma_g(v) is degree j = d g^-1 mod 2N of v if j < N, else minus degree j - N (auto_coeff): a gather whose
// addresses depend on g (public) and never on a coefficient's value.  The key switch is the relinearization's (bfv_key_switch.hip):
//   k_key_switch (SrcGalois)   every digit d_i = (sigma_g(c1) >> i w) & (2^w - 1) is transformed with the five primes, multiplied
//                              by the transformed gk0_i and gk1_i and summed; one inverse transform per component
//                              (sum < l N 2^w Q < 2^116; a hybrid key set: sum <= l N (2^w - 1) (Q P - 1) <= P5 / 2)
//   k_eval_epilogue EV_GALOIS  Garner over the five primes, x mod Q, + sigma_g(c0) on component 0, + x_in when set (slot_sum's
//                              x <- x + apply_galois(x), fused: the same sums mod Q as zkfhe_bfv_add); with the keys of a hybrid
//                              set floor((2 x + P) / 2P) mod Q stands for x mod Q (k_eval_epilogue<true>)
// apply_galois and slot_sum are one chunk loop, zk_bfv_galois_run: `steps` key switches per chunk on device buffers, each added to
// its input or not.  Host keys are transformed once per call, all of them in one launch (stage_keys); the batch calls of
// bfv_resident.hip call the same runner on device planes, with host keys or the keys of a resident key set.
// Galois keys (and their threshold shares) are products a_j s with a ternary s: the three-prime k_rns_ntt against the transform of
// s, then k_rns_epilogue (bfv_enc.hip) in EPI_GADGET mode: 2^(j w) sigma_g(s) - a_j s - e_j mod Q.
//
// Slots (T prime below 2^31, 2N | T - 1): k_slot_ntt is one LDS NTT mod T per polynomial with rns_forward / rns_inverse and the
// Montgomery helpers of rns_ntt.hip.hpp, on a table for T built on the host and cached in the context per (T, N): psi = zeta =
// r^((T - 1) / 2N) (r the smallest primitive root mod T), so NTT index k holds m(zeta^(2 br(k) + 1)), and the slot of that
// exponent (slot p = row N/2 + j is the evaluation at zeta^((-1)^row 5^j)).  No kernel uses scratch.
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;   // the key switch: five primes, as the relinearization
constexpr int NP3 = 3;       // the keys: a ternary factor, three primes

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
  const size_t chunk = std::min<size_t>(n_polys, chunk_polys(n));
  uint64_t *in_d, *o_d;
  ZK_CK(Arena().add(in_d, chunk * n).add(o_d, chunk * n).carve(ctx));
  int lds;
  ZK_CK(ntt_lds(ctx, (const void *)k_slot_ntt, log_n, &lds));
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

// r_j = 2^(j w) sigma_g(s) - (a_j s + e_j) mod Q, j < l: a_j uniform from (crs_seed, 14, g 64 + j), e_j an error sample from
// (party_seed, 15, g 64 + j)
int galois_key(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t crs_seed[32], const uint8_t party_seed[32],
               uint64_t g, int base_bits, uint64_t *r_out, uint64_t *a_out, const char *fn) {
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_g(ctx, params->n, g, fn));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  const size_t lw = (size_t)l * n;
  int *flag;
  uint64_t *s_d, *a_d, *e_d, *r_d, *cdt_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(a_d, lw).add(e_d, lw).add(r_d, lw).add(cdt_d, n_cdt).add(hat, NP3 * n).add(res, lw * NP3)
            .carve(ctx));
  ZK_CK(secret_hat<NP3>(ctx, sk, n, q, s_d, hat, flag, fn));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, DOM_GK_A, g * 64, S_UNIFORM, l, log_n, q, nullptr, 0, a_d));
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_GK_E, g * 64, S_ERROR, l, log_n, q, cdt_d, n_cdt, e_d));
  ZK_CK(launch_rns_ntt<NP3>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat, 0, res, flag));
  const Epi epi{.mode = EPI_GADGET, .e = e_d, .s = s_d, .ginv = galois_inv(g, n), .w = base_bits, .neg_e = 1};
  ZK_CK(zk_bfv_epilogue(ctx, res, l, log_n, q, epi, r_d));
  ZK_CK(zkfhe_download(ctx, r_out, r_d, lw * 8));
  ZK_CK(zkfhe_download(ctx, a_out, a_d, lw * 8));
  return ZKFHE_OK;
}

// one key switch of c ciphertexts: x_d = [c0 | c1] ([2 c][N]), key_hat: [2 l][5][N] (special: its special modulus, 1: none); out_d = [sigma_g(c0) + ks0 | ks1] (+ x_d)
int galois_core(zkfhe_ctx *ctx, const uint64_t *x_d, size_t c, const KeySwitch &ks, uint64_t g, const uint32_t *key_hat, uint64_t special,
                bool accumulate, uint32_t *acc, uint64_t *out_d) {
  const unsigned ginv = galois_inv(g, (uint64_t)1 << ks.log_n);
  ZK_CK(zk_bfv_key_switch(ctx, ks, SrcGalois{x_d + (c << ks.log_n), ginv}, key_hat, c, acc));
  const EvEpi epi{.mode = EV_GALOIS, .add = accumulate ? x_d : nullptr, .poly = x_d, .ginv = ginv, .c = c, .p = special};
  return zk_bfv_eval_epilogue(ctx, acc, 2 * c, ks.log_n, ks.q, epi, out_d);
}

}  // namespace

namespace zkrns {

int check_g(zkfhe_ctx *ctx, uint64_t n, uint64_t g, const char *fn) {
  if (!(g & 1) || g >= 2 * n) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": the Galois element g must be odd and below 2N");
  return ZKFHE_OK;
}

int zk_bfv_galois_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, size_t steps, const uint64_t *gs, KeySource key,
                      int l, int base_bits, bool accumulate, const Planes &out) {
  const uint64_t n = prm->n, q = prm->q;
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(count, chunk_polys(n)), cw = chunk * n;
  KeySwitch ks{log_n, l, base_bits, q};
  int *flag = nullptr;
  uint64_t *x_d, *y_d;
  uint32_t *acc;
  Arena ar;
  if (!key.resident()) ar.add(flag, 1);   // of the key transform
  key.add(ar, n, l);
  ar.add(x_d, 2 * cw).add(y_d, 2 * cw).add(acc, 2 * cw * NP);
  ks.add(ar, ctx, key, chunk);
  ZK_CK(ar.carve(ctx));
  ZK_CK(stage_keys<NP>(ctx, key, n, q, l, flag));
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t c = std::min(chunk, count - lo);
    uint64_t *x = x_d, *y = y_d;
    ZK_CK(a.in(ctx, 0, lo, c, n, x));   // a key switch reads [c0 | c1] of the chunk
    ZK_CK(a.in(ctx, 1, lo, c, n, x + c * n));
    for (size_t k = 0; k < steps; ++k) {   // y = apply_galois(x, g_k) (+ x), then the two change places
      ZK_CK(galois_core(ctx, x, c, ks, gs[k], key.hat(k), key.special, accumulate, acc, y));
      std::swap(x, y);
    }
    ZK_CK(out.out(ctx, 0, lo, c, n, x));
    ZK_CK(out.out(ctx, 1, lo, c, n, x + c * n));
  }
  return out.done(ctx);
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_slot_count(const zkfhe_bfv_params *params, size_t *slots) {
  if (!slots) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_slot_count: slots is NULL");
  ZK_CK(check_params(nullptr, params));
  ZK_CK(check_batching(nullptr, params, "bfv_slot_count"));
  *slots = (size_t)params->n;
  return ZKFHE_OK;
}

int zkfhe_bfv_galois_element(const zkfhe_bfv_params *params, int64_t steps, int swap_rows, uint64_t *g) {
  if (!g) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_galois_element: g is NULL");
  ZK_CK(check_params(nullptr, params));
  const uint64_t n = params->n;
  const int64_t half = (int64_t)(n / 2), k = ((steps % half) + half) % half;
  const uint64_t r = pow5((uint64_t)k, n);
  *g = swap_rows ? r * (2 * n - 1) % (2 * n) : r;
  return ZKFHE_OK;
}

int zkfhe_bfv_slot_sum_elements(const zkfhe_bfv_params *params, uint64_t *g, size_t *count) {
  if (!count) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_slot_sum_elements: count is NULL");
  ZK_CK(check_params(nullptr, params));
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
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_batching(ctx, params, "bfv_encode_slots"));
  bool bad = false;
  for (size_t i = 0; i < n_polys * params->n; ++i) bad |= values[i] >= params->t;
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_encode_slots: a slot value is not below T");
  return slot_transform(ctx, params, n_polys, values, 0, m_out);
}

int zkfhe_bfv_decode_slots(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_polys, const uint64_t *m, uint64_t *values_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && m && values_out && n_polys > 0);
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_batching(ctx, params, "bfv_decode_slots"));
  ZK_CK(check_plain(ctx, m, n_polys * params->n, params->q, params->t, "bfv_decode_slots"));
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
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_g(ctx, params->n, g, "bfv_apply_galois"));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_apply_galois", &l));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_apply_galois", "a ciphertext", c1));
  ZK_CK(check_below_q(ctx, gk0, (size_t)l * n, q, "bfv_apply_galois", "a Galois-key", gk1));
  return zk_bfv_galois_run(ctx, params, n_cts, host_planes(c0, c1), 1, &g, host_keys(gk0, gk1), l, base_bits, false, host_planes(out0, out1));
}

int zkfhe_bfv_slot_sum(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, const uint64_t *gk0,
                       const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && gk0 && gk1 && out0 && out1 && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_slot_sum", &l));
  const uint64_t n = params->n, q = params->q;
  size_t steps = 0;
  ZK_CK(zkfhe_bfv_slot_sum_elements(params, nullptr, &steps));
  std::vector<uint64_t> gs(steps);
  ZK_CK(zkfhe_bfv_slot_sum_elements(params, gs.data(), &steps));
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_slot_sum", "a ciphertext", c1));
  ZK_CK(check_below_q(ctx, gk0, steps * l * n, q, "bfv_slot_sum", "a Galois-key", gk1));
  return zk_bfv_galois_run(ctx, params, n_cts, host_planes(c0, c1), steps, gs.data(), host_keys(gk0, gk1, steps), l, base_bits, true,
                           host_planes(out0, out1));
}

}  // extern "C"
