// Threshold BFV on the GPU: the multiparty BFV of Mouchet et al. (collective public key, collective relinearization key, decryption
// by shares with smudging noise), so that a committee that holds the secret jointly opens the tally and nobody opens one input
// (zkfhe.h, INTEGRATION.md "Threshold decryption of the tally").  Conventions of bfv_enc.hip: host arrays, N residues in [0, Q)
// per polynomial, CircuitInput order.  Party i holds a ternary s_i; the collective s = sum_i s_i is never formed here.
//
// Every product has a ternary factor (a s_i, u_i a_j, s_i h0, s_i h1, u_i h1), so the three-prime path of rns_ntt.hip.hpp carries it
// exactly (|c| < N 2^63 <= 2^78).  The ternary operand of a call is transformed once (its load flags a non-ternary coefficient),
// one batched k_rns_ntt multiplies the rows of the other operand by it, and k_rns_epilogue (bfv_enc.hip) rebuilds c mod Q by
// Garner's CRT and applies the call's additions, one thread per coefficient:
//   EPI_ADD      x [+ a - b] [+ e]                 h1 = s_i a_j + e1; round 2 = u_i h1 + (s_i h0 - s_i h1) + e2
//   EPI_NEG_ADD  -(x + e)                           pk0_i = -(a s_i + e_i)
//   EPI_SHARE    x + r - E, r uniform in [0, 2E]    d = c1 s_i + e
//   EPI_GADGET   -x + e + 2^(j w) s_i for row j      h0 = -u_i a_j + 2^(j w) s_i + e0
// k_bfv_share_sum adds P coalesced planes mod Q; k_bfv_decrypt_combine forms c0 + sum_p d_p mod Q and rounds it as zkfhe_bfv_decrypt
// does (decrypt_round), in one pass.  No step branches on or addresses memory by a secret value; no kernel uses scratch.
//
// Randomness: the ChaCha20 streams and samplers of bfv_enc.hip, with the domains of zkfhe.h (Domain of rns_ntt.hip.hpp).
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = 3;   // the first three primes of rns_ntt.hip.hpp: product 2^89.2

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

// u_i of the relinearization rounds (party_seed, domain 10, index 0) to u_d, and its transform to hat
int party_u_hat(zkfhe_ctx *ctx, const uint8_t party_seed[32], uint64_t n, uint64_t q, uint64_t *u_d, uint32_t *hat, int *flag) {
  const int log_n = bit_log2(n);
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_THR_U, 0, S_TERNARY, 1, log_n, q, nullptr, 0, u_d));
  return launch_rns_ntt<NP>(ctx, false, u_d, LOAD_TERNARY, q, 1, log_n, nullptr, 0, hat, flag);
}

}  // namespace

extern "C" {

int zkfhe_bfv_keygen_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint8_t crs_seed[32], const uint8_t party_seed[32],
                           uint64_t *sk_out, uint64_t *pk0_share_out, uint64_t *pk1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && crs_seed && party_seed && sk_out && pk0_share_out && pk1_out);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  int *flag;
  uint64_t *s, *a, *e, *pk0, *cdt_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(s, n).add(a, n).add(e, n).add(pk0, n).add(cdt_d, n_cdt).add(hat, NP * n).add(res, NP * n).carve(ctx));
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_KEY_S, 0, S_TERNARY, 1, log_n, q, nullptr, 0, s));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, DOM_KEY_A, 0, S_UNIFORM, 1, log_n, q, nullptr, 0, a));
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_KEY_E, 0, S_ERROR, 1, log_n, q, cdt_d, n_cdt, e));
  ZK_CK(launch_rns_ntt<NP>(ctx, false, a, LOAD_RESIDUE, q, 1, log_n, nullptr, 0, hat, flag));
  ZK_CK(launch_rns_ntt<NP>(ctx, true, s, LOAD_TERNARY, q, 1, log_n, hat, 0, res, flag));
  ZK_CK(zk_bfv_epilogue(ctx, res, 1, log_n, q, Epi{.mode = EPI_NEG_ADD, .e = e}, pk0));
  ZK_CK(zkfhe_download(ctx, sk_out, s, n * 8));
  ZK_CK(zkfhe_download(ctx, pk1_out, a, n * 8));
  ZK_CK(zkfhe_download(ctx, pk0_share_out, pk0, n * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_share_aggregate(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_polys, const uint64_t *shares,
                              uint64_t *out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && shares && out && n_parties > 0 && n_polys > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const size_t stride = n_polys * n;   // words of one party
  ZK_CK(check_below_q(ctx, shares, n_parties * stride, q, "bfv_share_aggregate", "a share"));
  const size_t chunk = plane_chunk(n, n_parties, n_polys);
  uint64_t *src, *o_d;
  ZK_CK(Arena().add(src, n_parties * chunk * n).add(o_d, chunk * n).carve(ctx));
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
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_relin_share1", &l));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  const size_t lw = (size_t)l * n;
  int *flag;
  uint64_t *s_d, *u_d, *a_d, *e0_d, *e1_d, *h0_d, *h1_d, *cdt_d;
  uint32_t *hat_s, *hat_u, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(u_d, n).add(a_d, lw).add(e0_d, lw).add(e1_d, lw).add(h0_d, lw).add(h1_d, lw).add(cdt_d, n_cdt)
            .add(hat_s, NP * n).add(hat_u, NP * n).add(res, lw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk_i, n, q, s_d, hat_s, flag, "bfv_relin_share1"));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  ZK_CK(party_u_hat(ctx, party_seed, n, q, u_d, hat_u, flag));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, DOM_RLK_A, 0, S_UNIFORM, l, log_n, q, nullptr, 0, a_d));          // a_j: CRS, index j
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_THR_E0, 0, S_ERROR, l, log_n, q, cdt_d, n_cdt, e0_d));
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_THR_E1, 0, S_ERROR, l, log_n, q, cdt_d, n_cdt, e1_d));
  ZK_CK(launch_rns_ntt<NP>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat_u, 0, res, flag));
  ZK_CK(zk_bfv_epilogue(ctx, res, l, log_n, q, Epi{.mode = EPI_GADGET, .e = e0_d, .s = s_d, .w = base_bits}, h0_d));
  ZK_CK(launch_rns_ntt<NP>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat_s, 0, res, flag));
  ZK_CK(zk_bfv_epilogue(ctx, res, l, log_n, q, Epi{.mode = EPI_ADD, .e = e1_d}, h1_d));
  ZK_CK(zkfhe_download(ctx, h0_out, h0_d, lw * 8));
  ZK_CK(zkfhe_download(ctx, h1_out, h1_d, lw * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_relin_share2(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t party_seed[32], int base_bits,
                           const uint64_t *h0, const uint64_t *h1, uint64_t *r_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && party_seed && h0 && h1 && r_out);
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_relin_share2", &l));
  const uint64_t n = params->n, q = params->q;
  const size_t lw = (size_t)l * n;
  ZK_CK(check_below_q(ctx, h0, lw, q, "bfv_relin_share2", "an h0"));
  ZK_CK(check_below_q(ctx, h1, lw, q, "bfv_relin_share2", "an h1"));
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  int *flag;
  uint64_t *s_d, *u_d, *hh, *sh, *e2_d, *r_d, *cdt_d;
  uint32_t *hat_s, *hat_u, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(u_d, n).add(hh, 2 * lw).add(sh, 2 * lw).add(e2_d, lw).add(r_d, lw).add(cdt_d, n_cdt)
            .add(hat_s, NP * n).add(hat_u, NP * n).add(res, 2 * lw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk_i, n, q, s_d, hat_s, flag, "bfv_relin_share2"));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  ZK_CK(party_u_hat(ctx, party_seed, n, q, u_d, hat_u, flag));
  ZK_CK(zkfhe_upload(ctx, hh, h0, lw * 8));
  ZK_CK(zkfhe_upload(ctx, hh + lw, h1, lw * 8));
  ZK_CK(zk_bfv_sample(ctx, party_seed, DOM_THR_E2, 0, S_ERROR, l, log_n, q, cdt_d, n_cdt, e2_d));   // e2_j: index j
  // s_i h0 | s_i h1 mod Q, then r = u_i h1 + s_i h0 - s_i h1 + e2 = s_i h0 + (u_i - s_i) h1 + e2
  ZK_CK(launch_rns_ntt<NP>(ctx, true, hh, LOAD_RESIDUE, q, 2 * l, log_n, hat_s, 0, res, flag));
  ZK_CK(zk_bfv_epilogue(ctx, res, 2 * l, log_n, q, Epi{.mode = EPI_ADD}, sh));
  ZK_CK(launch_rns_ntt<NP>(ctx, true, hh + lw, LOAD_RESIDUE, q, l, log_n, hat_u, 0, res, flag));
  ZK_CK(zk_bfv_epilogue(ctx, res, l, log_n, q, Epi{.mode = EPI_ADD, .e = e2_d, .a = sh, .b = sh + lw}, r_d));
  ZK_CK(zkfhe_download(ctx, r_out, r_d, lw * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_decrypt_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, size_t n_cts, const uint64_t *c1,
                            const uint8_t seed[32], uint64_t first_index, uint64_t smudge_bound, uint64_t *d_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && c1 && seed && d_out && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q, delta = q / params->t;
  if (smudge_bound > (delta - 1) / 2)   // 2E + 1 > floor(Q/T), without overflow
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_decrypt_share: 2 smudge_bound + 1 must not exceed floor(Q/T)");
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_decrypt_share", "a ciphertext"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), cw = chunk * n;
  int *flag;
  uint64_t *s_d, *c1_d, *r_d, *d_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(hat, NP * n).add(c1_d, cw).add(r_d, cw).add(d_d, cw).add(res, cw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk_i, n, q, s_d, hat, flag, "bfv_decrypt_share"));
  const Epi epi{.mode = EPI_SHARE, .e = r_d, .bound = smudge_bound};
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, c1_d, c1 + lo * n, bytes));
    // smudging noise: the uniform sampler mod 2E + 1, index first_index + j
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_SMUDGE, first_index + lo, S_UNIFORM, c, log_n, 2 * smudge_bound + 1, nullptr, 0, r_d));
    ZK_CK(launch_rns_ntt<NP>(ctx, true, c1_d, LOAD_RESIDUE, q, c, log_n, hat, 0, res, flag));
    ZK_CK(zk_bfv_epilogue(ctx, res, c, log_n, q, epi, d_d));
    ZK_CK(zkfhe_download(ctx, d_out + lo * n, d_d, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_decrypt_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint64_t *c0,
                              const uint64_t *d, uint64_t *m_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && d && m_out && n_parties > 0 && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const size_t stride = n_cts * n;   // words of one party's shares
  ZK_CK(check_below_q(ctx, c0, stride, q, "bfv_decrypt_combine", "a ciphertext"));
  ZK_CK(check_below_q(ctx, d, n_parties * stride, q, "bfv_decrypt_combine", "a decryption-share"));
  const size_t chunk = plane_chunk(n, n_parties + 1, n_cts);
  uint64_t *c0_d, *m_d, *d_d;
  ZK_CK(Arena().add(c0_d, chunk * n).add(m_d, chunk * n).add(d_d, n_parties * chunk * n).carve(ctx));
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
