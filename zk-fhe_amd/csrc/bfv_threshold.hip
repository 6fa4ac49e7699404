// Threshold BFV on the GPU: the multiparty BFV of Mouchet et al. (collective public key, collective relinearization key, decryption
// by shares with smudging noise), so that a committee that holds the secret jointly opens the tally and nobody opens one input
// (zkfhe.h, INTEGRATION.md "Threshold decryption of the tally").  Conventions of bfv_enc.hip: host arrays, N residues in [0, Q)
// per polynomial, CircuitInput order.  Party i holds a ternary s_i; the collective s = sum_i s_i is never formed here.
//
// Every product has a ternary factor (a s_i, u_i a_j, s_i h0, s_i h1, u_i h1), so the three-prime path of rns_ntt.hip.hpp carries it
// exactly (|c| < N 2^63 <= 2^78).  The ternary operand of a call is transformed once (its load flags a non-ternary coefficient),
// one batched k_rns_ntt multiplies the rows of the other operand by it, and k_thr_epilogue rebuilds c mod Q by Garner's CRT
// (crt3_mod_q, as k_rns_epilogue) and applies the call's additions, one thread per coefficient:
//   THR_ADD      x [+ a - b] [+ e]                 h1 = s_i a_j + e1; round 2 = u_i h1 + (s_i h0 - s_i h1) + e2
//   THR_NEG_ADD  -(x + e)                           pk0_i = -(a s_i + e_i)
//   THR_SHARE    x + r - E, r uniform in [0, 2E]    d = c1 s_i + e
//   THR_GADGET   -x + e + 2^(j w) s_i for row j      h0 = -u_i a_j + 2^(j w) s_i + e0
// k_bfv_share_sum adds P coalesced planes mod Q; k_bfv_decrypt_combine forms c0 + sum_p d_p mod Q and rounds it as zkfhe_bfv_decrypt
// does (decrypt_round), in one pass.  No step branches on or addresses memory by a secret value; no kernel uses scratch.
//
// Randomness: the ChaCha20 streams and samplers of bfv_enc.hip.  Domains: 4 s_i, 5 a (CRS), 6 e_i, 7 a_j (CRS, index j),
// 9 smudging noise (index first_index + ciphertext), 10 u_i, 11 / 12 / 13 e0 / e1 / e2 of row j (index j).
#include <string>

#include "rns_ntt.hip.hpp"

using namespace zkrns;

namespace {

constexpr int NP = 3;   // the first three primes of rns_ntt.hip.hpp: product 2^89.2
constexpr int K_TERNARY = 0, K_UNIFORM = 1, K_ERROR = 2;   // zk_bfv_sample kinds

enum ThrMode { THR_ADD = 0, THR_NEG_ADD = 1, THR_SHARE = 2, THR_GADGET = 3 };
struct ThrEpi {
  int mode;
  const uint64_t *e;        // + e[pos]; THR_ADD: may be null; THR_SHARE: the uniform sample r in [0, 2E]
  const uint64_t *a, *b;    // THR_ADD: + a[pos] - b[pos] (both null or both set)
  const uint64_t *s;        // THR_GADGET: s_i, one polynomial
  uint64_t bound;           // THR_SHARE: E
  int w;                    // THR_GADGET: the digit width; row j gets 2^(j w) s_i
};

__device__ __forceinline__ uint64_t sub_q(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }

// One thread per output coefficient of res ([poly][prime][degree], total = n_polys N): x = the product mod Q, then the mode's
// additions (see the top of the file); out and every addend in CircuitInput order, read and written at pos.
__global__ __launch_bounds__(256) void k_thr_epilogue(const uint32_t *__restrict__ res, size_t total, int log_n, uint64_t q, CrtConst cc,
                                                      ThrEpi epi, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t n = (size_t)1 << log_n, poly = g >> log_n, d = g & (n - 1), pos = poly * n + (n - 1 - d);
  uint64_t v = crt3_mod_q(res + poly * NP * n + d, n, q, cc);
  if (epi.mode == THR_ADD) {
    if (epi.a) v = sub_q(add_q(v, epi.a[pos], q), epi.b[pos], q);
    if (epi.e) v = add_q(v, epi.e[pos], q);
  } else if (epi.mode == THR_NEG_ADD) {
    v = add_q(v, epi.e[pos], q);
    v = v ? q - v : 0;
  } else if (epi.mode == THR_SHARE) {
    v = sub_q(add_q(v, epi.e[pos], q), epi.bound, q);   // r <= 2E < Q
  } else {
    // j w <= (l - 1) w < bitlen(Q - 1): 2^(j w) < Q.  s_i in {0, 1, Q - 1} selects 0, 2^(j w) or Q - 2^(j w) without a branch.
    const uint64_t pw = (uint64_t)1 << (poly * epi.w), sv = epi.s[pos - poly * n];
    const uint64_t gs = sv == 1 ? pw : (sv == q - 1 ? q - pw : 0);
    v = add_q(add_q(v ? q - v : 0, epi.e[pos], q), gs, q);
  }
  out[pos] = v;
}

// One thread per word of a chunk: out[g] = sum_p src[p][g] mod Q; src: [n_parties][words], consecutive threads read consecutive words
// of every plane.
__global__ __launch_bounds__(256) void k_bfv_share_sum(const uint64_t *__restrict__ src, size_t n_parties, size_t words, uint64_t q,
                                                       uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= words) return;
  uint64_t v = 0;
#pragma unroll 4
  for (size_t p = 0; p < n_parties; ++p) v = add_q(v, src[p * words + g], q);
  out[g] = v;
}

// One thread per coefficient of a chunk of ciphertexts: m = decrypt_round([c0 + sum_p d_p]_Q), the rounding of zkfhe_bfv_decrypt.
// d: [n_parties][words].
__global__ __launch_bounds__(256) void k_bfv_decrypt_combine(const uint64_t *__restrict__ c0, const uint64_t *__restrict__ d, size_t n_parties,
                                                             size_t words, uint64_t q, uint64_t t, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= words) return;
  uint64_t v = c0[g];
#pragma unroll 4
  for (size_t p = 0; p < n_parties; ++p) v = add_q(v, d[p * words + g], q);
  out[g] = decrypt_round(v, q, t);
}

// ------------------------------------------------------------------------------------------------------------------ host side

int launch_thr_epilogue(zkfhe_ctx *ctx, const uint32_t *res, size_t n_polys, int log_n, uint64_t q, const ThrEpi &epi, uint64_t *out) {
  const size_t total = n_polys << log_n;
  zk_prof_begin(ctx);
  k_thr_epilogue<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(res, total, log_n, q, crt3_const(), epi, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_RNS_EPILOGUE, (double)total * (12 + 8 + (epi.e ? 8 : 0) + (epi.a ? 16 : 0) + (epi.s ? 8 : 0)));
  return ZKFHE_OK;
}

int launch_ntt(zkfhe_ctx *ctx, bool mul, const uint64_t *src, bool ternary, uint64_t q, size_t n_polys, int log_n, const uint32_t *hat,
               uint32_t *out, int *flag) {
  return launch_rns_ntt<NP>(ctx, mul, src, ternary ? LOAD_TERNARY : LOAD_RESIDUE, q, n_polys, log_n, hat, 0, out, flag);
}

int check_below_q(zkfhe_ctx *ctx, const uint64_t *v, size_t count, uint64_t q, const char *fn, const char *what) {
  for (size_t i = 0; i < count; ++i)
    if (v[i] >= q) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": " + what + " coefficient is not below Q");
  return ZKFHE_OK;
}

// the party's secret s_i uploaded to sk_d and transformed into hat (three planes); refuses a non-ternary key
int secret_hat(zkfhe_ctx *ctx, const uint64_t *sk, uint64_t n, uint64_t q, uint64_t *sk_d, uint32_t *hat, int *flag, const char *fn) {
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, sk_d, sk, n * 8));
  ZK_CK(launch_ntt(ctx, false, sk_d, true, q, 1, bit_log2(n), nullptr, hat, flag));
  int bad = 0;
  ZK_CK(zkfhe_download(ctx, &bad, flag, 4));
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a secret-key coefficient is not in {0, 1, Q - 1}");
  return ZKFHE_OK;
}

// u_i of the relinearization rounds (party_seed, domain 10, index 0) to u_d, and its transform to hat
int party_u_hat(zkfhe_ctx *ctx, const uint8_t party_seed[32], uint64_t n, uint64_t q, uint64_t *u_d, uint32_t *hat, int *flag) {
  const int log_n = bit_log2(n);
  ZK_CK(zk_bfv_sample(ctx, party_seed, 10, 0, K_TERNARY, 1, log_n, q, nullptr, 0, u_d));
  return launch_ntt(ctx, false, u_d, true, q, 1, log_n, nullptr, hat, flag);
}

int relin_rows(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, const char *fn, int *l) {
  if (base_bits < 1 || base_bits > 32) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": base_bits must be in [1, 32]");
  size_t rows = 0;
  ZK_CK(zkfhe_bfv_relin_digits(params, base_bits, &rows));
  *l = (int)rows;
  return ZKFHE_OK;
}

// polynomials per chunk when n_planes planes of the chunk are resident at once: the budget of chunk_polys per four planes
size_t plane_chunk(uint64_t n, size_t n_planes, size_t count) {
  return std::min(count, std::max<size_t>(1, chunk_polys(n) * 4 / n_planes));
}

}  // namespace

extern "C" {

int zkfhe_bfv_keygen_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint8_t crs_seed[32], const uint8_t party_seed[32],
                           uint64_t *sk_out, uint64_t *pk0_share_out, uint64_t *pk1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && crs_seed && party_seed && sk_out && pk0_share_out && pk1_out);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  zk_bfv_error_cdt(params->b, cdt.data());
  const size_t vec = align256(n * 8), plane = align256((size_t)NP * n * 4);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + 4 * vec + align256(n_cdt * 8) + 2 * plane, &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *s = (uint64_t *)take(vec), *a = (uint64_t *)take(vec), *e = (uint64_t *)take(vec), *pk0 = (uint64_t *)take(vec);
  uint64_t *cdt_d = (uint64_t *)take(align256(n_cdt * 8));
  uint32_t *hat = (uint32_t *)take(plane), *res = (uint32_t *)take(plane);
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, cdt_d, cdt.data(), n_cdt * 8));
  ZK_CK(zk_bfv_sample(ctx, party_seed, 4, 0, K_TERNARY, 1, log_n, q, nullptr, 0, s));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, 5, 0, K_UNIFORM, 1, log_n, q, nullptr, 0, a));
  ZK_CK(zk_bfv_sample(ctx, party_seed, 6, 0, K_ERROR, 1, log_n, q, cdt_d, n_cdt, e));
  ZK_CK(launch_ntt(ctx, false, a, false, q, 1, log_n, nullptr, hat, flag));
  ZK_CK(launch_ntt(ctx, true, s, true, q, 1, log_n, hat, res, flag));
  ZK_CK(launch_thr_epilogue(ctx, res, 1, log_n, q, ThrEpi{THR_NEG_ADD, e, nullptr, nullptr, nullptr, 0, 0}, pk0));
  ZK_CK(zkfhe_download(ctx, sk_out, s, n * 8));
  ZK_CK(zkfhe_download(ctx, pk1_out, a, n * 8));
  ZK_CK(zkfhe_download(ctx, pk0_share_out, pk0, n * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_share_aggregate(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_polys, const uint64_t *shares,
                              uint64_t *out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && shares && out && n_parties > 0 && n_polys > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const size_t stride = n_polys * n;   // words of one party
  ZK_CK(check_below_q(ctx, shares, n_parties * stride, q, "bfv_share_aggregate", "a share"));
  const size_t chunk = plane_chunk(n, n_parties, n_polys);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, align256(n_parties * chunk * n * 8) + align256(chunk * n * 8), &w));
  uint64_t *src = (uint64_t *)w, *o_d = (uint64_t *)(w + align256(n_parties * chunk * n * 8));
  for (size_t lo = 0; lo < n_polys; lo += chunk) {
    const size_t c = std::min(chunk, n_polys - lo), words = c * n;
    for (size_t p = 0; p < n_parties; ++p) ZK_CK(zkfhe_upload(ctx, src + p * words, shares + p * stride + lo * n, words * 8));
    zk_prof_begin(ctx);
    k_bfv_share_sum<<<zk_blocks(words, 256), 256, 0, ctx->stream>>>(src, n_parties, words, q, o_d);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_SHARE_SUM, (double)(n_parties + 1) * words * 8);
    ZK_CK(zkfhe_download(ctx, out + lo * n, o_d, words * 8));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_relin_share1(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t crs_seed[32],
                           const uint8_t party_seed[32], int base_bits, uint64_t *h0_out, uint64_t *h1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && crs_seed && party_seed && h0_out && h1_out);
  ZK_CK(zk_bfv_check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_relin_share1", &l));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  zk_bfv_error_cdt(params->b, cdt.data());
  const size_t vec = align256(n * 8), lvec = align256((size_t)l * n * 8), plane = align256((size_t)NP * n * 4);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + 2 * vec + 5 * lvec + align256(n_cdt * 8) + 2 * plane + align256((size_t)l * NP * n * 4), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *s_d = (uint64_t *)take(vec), *u_d = (uint64_t *)take(vec), *a_d = (uint64_t *)take(lvec), *e0_d = (uint64_t *)take(lvec);
  uint64_t *e1_d = (uint64_t *)take(lvec), *h0_d = (uint64_t *)take(lvec), *h1_d = (uint64_t *)take(lvec);
  uint64_t *cdt_d = (uint64_t *)take(align256(n_cdt * 8));
  uint32_t *hat_s = (uint32_t *)take(plane), *hat_u = (uint32_t *)take(plane), *res = (uint32_t *)take(align256((size_t)l * NP * n * 4));
  ZK_CK(secret_hat(ctx, sk_i, n, q, s_d, hat_s, flag, "bfv_relin_share1"));
  ZK_CK(zkfhe_upload(ctx, cdt_d, cdt.data(), n_cdt * 8));
  ZK_CK(party_u_hat(ctx, party_seed, n, q, u_d, hat_u, flag));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, 7, 0, K_UNIFORM, l, log_n, q, nullptr, 0, a_d));             // a_j: CRS, domain 7, index j
  ZK_CK(zk_bfv_sample(ctx, party_seed, 11, 0, K_ERROR, l, log_n, q, cdt_d, n_cdt, e0_d));       // e0_j: domain 11
  ZK_CK(zk_bfv_sample(ctx, party_seed, 12, 0, K_ERROR, l, log_n, q, cdt_d, n_cdt, e1_d));       // e1_j: domain 12
  ZK_CK(launch_ntt(ctx, true, a_d, false, q, l, log_n, hat_u, res, flag));
  ZK_CK(launch_thr_epilogue(ctx, res, l, log_n, q, ThrEpi{THR_GADGET, e0_d, nullptr, nullptr, s_d, 0, base_bits}, h0_d));
  ZK_CK(launch_ntt(ctx, true, a_d, false, q, l, log_n, hat_s, res, flag));
  ZK_CK(launch_thr_epilogue(ctx, res, l, log_n, q, ThrEpi{THR_ADD, e1_d, nullptr, nullptr, nullptr, 0, 0}, h1_d));
  ZK_CK(zkfhe_download(ctx, h0_out, h0_d, (size_t)l * n * 8));
  ZK_CK(zkfhe_download(ctx, h1_out, h1_d, (size_t)l * n * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_relin_share2(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t party_seed[32], int base_bits,
                           const uint64_t *h0, const uint64_t *h1, uint64_t *r_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && party_seed && h0 && h1 && r_out);
  ZK_CK(zk_bfv_check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_relin_share2", &l));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, h0, (size_t)l * n, q, "bfv_relin_share2", "an h0"));
  ZK_CK(check_below_q(ctx, h1, (size_t)l * n, q, "bfv_relin_share2", "an h1"));
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  zk_bfv_error_cdt(params->b, cdt.data());
  const size_t vec = align256(n * 8), lw = (size_t)l * n, lvec = align256(lw * 8), plane = align256((size_t)NP * n * 4);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + 2 * vec + 6 * lvec + align256(n_cdt * 8) + 2 * plane + align256(2 * lw * NP * 4), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *s_d = (uint64_t *)take(vec), *u_d = (uint64_t *)take(vec), *hh = (uint64_t *)take(2 * lvec), *sh = (uint64_t *)take(2 * lvec);
  uint64_t *e2_d = (uint64_t *)take(lvec), *r_d = (uint64_t *)take(lvec), *cdt_d = (uint64_t *)take(align256(n_cdt * 8));
  uint32_t *hat_s = (uint32_t *)take(plane), *hat_u = (uint32_t *)take(plane), *res = (uint32_t *)take(align256(2 * lw * NP * 4));
  ZK_CK(secret_hat(ctx, sk_i, n, q, s_d, hat_s, flag, "bfv_relin_share2"));
  ZK_CK(zkfhe_upload(ctx, cdt_d, cdt.data(), n_cdt * 8));
  ZK_CK(party_u_hat(ctx, party_seed, n, q, u_d, hat_u, flag));
  ZK_CK(zkfhe_upload(ctx, hh, h0, lw * 8));
  ZK_CK(zkfhe_upload(ctx, hh + lw, h1, lw * 8));
  ZK_CK(zk_bfv_sample(ctx, party_seed, 13, 0, K_ERROR, l, log_n, q, cdt_d, n_cdt, e2_d));   // e2_j: domain 13, index j
  // s_i h0 | s_i h1 mod Q, then r = u_i h1 + s_i h0 - s_i h1 + e2 = s_i h0 + (u_i - s_i) h1 + e2
  ZK_CK(launch_ntt(ctx, true, hh, false, q, 2 * l, log_n, hat_s, res, flag));
  ZK_CK(launch_thr_epilogue(ctx, res, 2 * l, log_n, q, ThrEpi{THR_ADD, nullptr, nullptr, nullptr, nullptr, 0, 0}, sh));
  ZK_CK(launch_ntt(ctx, true, hh + lw, false, q, l, log_n, hat_u, res, flag));
  ZK_CK(launch_thr_epilogue(ctx, res, l, log_n, q, ThrEpi{THR_ADD, e2_d, sh, sh + lw, nullptr, 0, 0}, r_d));
  ZK_CK(zkfhe_download(ctx, r_out, r_d, lw * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_decrypt_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, size_t n_cts, const uint64_t *c1,
                            const uint8_t seed[32], uint64_t first_index, uint64_t smudge_bound, uint64_t *d_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && c1 && seed && d_out && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q, delta = q / params->t;
  if (smudge_bound > (delta - 1) / 2)   // 2E + 1 > floor(Q/T), without overflow
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_decrypt_share: 2 smudge_bound + 1 must not exceed floor(Q/T)");
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_decrypt_share", "a ciphertext"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), vec = align256(n * 8), cvec = align256(chunk * n * 8);
  const size_t plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + vec + align256(plane) + 3 * cvec + align256(chunk * plane), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *s_d = (uint64_t *)take(vec);
  uint32_t *hat = (uint32_t *)take(align256(plane));
  uint64_t *c1_d = (uint64_t *)take(cvec), *r_d = (uint64_t *)take(cvec), *d_d = (uint64_t *)take(cvec);
  uint32_t *res = (uint32_t *)take(align256(chunk * plane));
  ZK_CK(secret_hat(ctx, sk_i, n, q, s_d, hat, flag, "bfv_decrypt_share"));
  const ThrEpi epi{THR_SHARE, r_d, nullptr, nullptr, nullptr, smudge_bound, 0};
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, c1_d, c1 + lo * n, bytes));
    // smudging noise: the uniform sampler mod 2E + 1, domain 9, index first_index + j
    ZK_CK(zk_bfv_sample(ctx, seed, 9, first_index + lo, K_UNIFORM, c, log_n, 2 * smudge_bound + 1, nullptr, 0, r_d));
    ZK_CK(launch_ntt(ctx, true, c1_d, false, q, c, log_n, hat, res, flag));
    ZK_CK(launch_thr_epilogue(ctx, res, c, log_n, q, epi, d_d));
    ZK_CK(zkfhe_download(ctx, d_out + lo * n, d_d, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_decrypt_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint64_t *c0,
                              const uint64_t *d, uint64_t *m_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && d && m_out && n_parties > 0 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const size_t stride = n_cts * n;   // words of one party's shares
  ZK_CK(check_below_q(ctx, c0, stride, q, "bfv_decrypt_combine", "a ciphertext"));
  ZK_CK(check_below_q(ctx, d, n_parties * stride, q, "bfv_decrypt_combine", "a decryption-share"));
  const size_t chunk = plane_chunk(n, n_parties + 1, n_cts), cvec = align256(chunk * n * 8);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 2 * cvec + align256(n_parties * chunk * n * 8), &w));
  uint64_t *c0_d = (uint64_t *)w, *m_d = (uint64_t *)(w + cvec), *d_d = (uint64_t *)(w + 2 * cvec);
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), words = c * n;
    ZK_CK(zkfhe_upload(ctx, c0_d, c0 + lo * n, words * 8));
    for (size_t p = 0; p < n_parties; ++p) ZK_CK(zkfhe_upload(ctx, d_d + p * words, d + p * stride + lo * n, words * 8));
    zk_prof_begin(ctx);
    k_bfv_decrypt_combine<<<zk_blocks(words, 256), 256, 0, ctx->stream>>>(c0_d, d_d, n_parties, words, q, params->t, m_d);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_DECRYPT_COMBINE, (double)(n_parties + 2) * words * 8);
    ZK_CK(zkfhe_download(ctx, m_out + lo * n, m_d, words * 8));
  }
  return ZKFHE_OK;
}

}  // extern "C"
