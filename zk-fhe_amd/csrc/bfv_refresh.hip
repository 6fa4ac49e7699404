// Collective refresh and public collective key switching (PCKS) of threshold BFV on the GPU, after Mouchet et al. (zkfhe.h
// "Collective refresh and key switching", INTEGRATION.md "Refreshing and handing over a ciphertext").  Refresh re-encrypts a worn
// ciphertext into a nearly noiseless one under the same collective key, so a committee can go on multiplying; PCKS re-encrypts a
// ciphertext from the collective secret to any public key.  Nobody sees the plaintext in either.  Conventions of bfv_threshold.hip:
// host arrays, N residues in [0, Q) per polynomial, CircuitInput order; party i holds a ternary s_i.
//
// Shares.  Every product has a ternary factor (s_i c1_j, s_i a_j, u_ij pk0', u_ij pk1'), so the three-prime path of
// rns_ntt.hip.hpp carries it exactly.  s_i (and pk0' | pk1') are transformed once per call; per chunk, the rows that share a
// transformed operand go through one k_rns_ntt launch, and one k_rns_epilogue (bfv_enc.hip) per output applies the additions:
//   refresh   c1_j | a_j (2c rows) against s_i^;  EPI_MASK  h0 = x - delta M + r - E,  h1 = -x + delta M + e1
//   PCKS      c1_j against s_i^ (EPI_PLAIN);  u_ij against pk0'^  EPI_SHARE_ADD  h0 = x + s_i c1_j + r - E;
//             u_ij against pk1'^  EPI_ADD  h1 = x + e1
// Combines.  One thread per coefficient, P coalesced planes per sum: k_bfv_pcks_combine forms c0 + sum h0_i and sum h1_i in one
// pass; k_bfv_refresh_combine forms v = c0 + sum h0_i, rounds it to mu in [0, T) (the rounding of decrypt_round before centring),
// and writes delta mu + sum h1_i in the same pass.  out1 of a refresh is the CRS stream itself (k_bfv_sample).
//
// Ciphertexts per chunk: plane_chunk(N, planes, n_cts) = chunk_polys(N) * 4 / planes (at least one), with the 64-bit planes of one
// ciphertext that are resident at once: 10 for a refresh share (c1 | a, M, r, e1, h0, h1 and the six 32-bit residue rows), 9 for a
// PCKS share (c1, u, r, e1, s_i c1, h0, h1 and three residue rows), and 2 P + 3 for either combine (c0, the 2 P share planes and
// the two outputs).
// No step branches on or addresses memory by a secret value; no kernel uses scratch.
//
// Randomness: the ChaCha20 streams and samplers of bfv_enc.hip, with domains 16 to 22 of zkfhe.h (Domain of rns_ntt.hip.hpp).
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = 3;   // the first three primes of rns_ntt.hip.hpp: product 2^89.2

// One thread per word of a chunk: out0 = c0 + sum_p h0[p], out1 = sum_p h1[p] mod Q.  h0, h1: [n_parties][words].
__global__ __launch_bounds__(256) void k_bfv_pcks_combine(const uint64_t *__restrict__ c0, const uint64_t *__restrict__ h0,
                                                          const uint64_t *__restrict__ h1, size_t n_parties, size_t words, uint64_t q,
                                                          uint64_t *__restrict__ out0, uint64_t *__restrict__ out1) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= words) return;
  uint64_t v = c0[g], w = 0;
#pragma unroll 4
  for (size_t p = 0; p < n_parties; ++p) {
    v = add_q(v, h0[p * words + g], q);
    w = add_q(w, h1[p * words + g], q);
  }
  out0[g] = v;
  out1[g] = w;
}

// One thread per coefficient of a chunk: v = [c0 + sum_p h0[p]]_Q, mu = floor((2 T v + Q) / 2Q) mod T, out0 = delta mu + sum_p h1[p]
// mod Q.  h0, h1: [n_parties][words].
__global__ __launch_bounds__(256) void k_bfv_refresh_combine(const uint64_t *__restrict__ c0, const uint64_t *__restrict__ h0,
                                                             const uint64_t *__restrict__ h1, size_t n_parties, size_t words, uint64_t q,
                                                             uint64_t t, uint64_t *__restrict__ out0) {
  typedef unsigned __int128 u128;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= words) return;
  uint64_t v = c0[g];
#pragma unroll 4
  for (size_t p = 0; p < n_parties; ++p) v = add_q(v, h0[p * words + g], q);
  const u128 num = (u128)(2 * t) * v + q;   // 2 T < 2^64; the quotient is in [0, T]
  uint64_t mu = div128((uint64_t)(num >> 64), (uint64_t)num, 2 * q);
  mu = mu == t ? 0 : mu;
  uint64_t w = (q / t) * mu;   // delta mu <= Q - delta < Q
#pragma unroll 4
  for (size_t p = 0; p < n_parties; ++p) w = add_q(w, h1[p * words + g], q);
  out0[g] = w;
}

// ------------------------------------------------------------------------------------------------------------------ host side

// refusal 2 of the share calls: 2 E + 1 > floor(Q/T), without overflow
int check_smudge(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t bound, const char *fn) {
  if (bound > (params->q / params->t - 1) / 2)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": 2 smudge_bound + 1 must not exceed floor(Q/T)");
  return ZKFHE_OK;
}

int null_or_zero(zkfhe_ctx *ctx, const char *fn) { return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a NULL argument or a zero count"); }

// the parties' planes of one chunk, party-major in host memory with `stride` words per party, to dst ([n_parties][words])
int upload_planes(zkfhe_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t n_parties, size_t stride, size_t offset, size_t words) {
  for (size_t p = 0; p < n_parties; ++p) ZK_CK(zkfhe_upload(ctx, dst + p * words, src + p * stride + offset, words * 8));
  return ZKFHE_OK;
}

}  // namespace

extern "C" {

int zkfhe_bfv_pcks_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint64_t *pk0_to, const uint64_t *pk1_to,
                         size_t n_cts, const uint64_t *c1, const uint8_t seed[32], uint64_t first_index, uint64_t smudge_bound,
                         uint64_t *h0_out, uint64_t *h1_out) {
  ZK_ENTER(ctx);
  if (!(ctx && sk_i && pk0_to && pk1_to && c1 && seed && h0_out && h1_out && n_cts > 0)) return null_or_zero(ctx, "bfv_pcks_share");
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_smudge(ctx, params, smudge_bound, "bfv_pcks_share"));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, pk0_to, n, q, "bfv_pcks_share", "a public-key", pk1_to));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_pcks_share", "a ciphertext"));
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  const size_t chunk = plane_chunk(n, 9, n_cts), cw = chunk * n;
  int *flag;
  uint64_t *s_d, *pk_d, *cdt_d, *c1_d, *u_d, *r_d, *e1_d, *sc_d, *h0_d, *h1_d;
  uint32_t *hat_s, *hat_pk, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(pk_d, 2 * n).add(cdt_d, n_cdt).add(hat_s, NP * n).add(hat_pk, 2 * NP * n).add(c1_d, cw).add(u_d, cw)
            .add(r_d, cw).add(e1_d, cw).add(sc_d, cw).add(h0_d, cw).add(h1_d, cw).add(res, cw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk_i, n, q, s_d, hat_s, flag, "bfv_pcks_share"));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  ZK_CK(zkfhe_upload(ctx, pk_d, pk0_to, n * 8));
  ZK_CK(zkfhe_upload(ctx, pk_d + n, pk1_to, n * 8));
  ZK_CK(launch_rns_ntt<NP>(ctx, false, pk_d, LOAD_RESIDUE, q, 2, log_n, nullptr, 0, hat_pk, flag));   // pk0'^ | pk1'^
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    const uint64_t index0 = first_index + lo;
    ZK_CK(zkfhe_upload(ctx, c1_d, c1 + lo * n, bytes));
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_PCKS_U, index0, S_TERNARY, c, log_n, q, nullptr, 0, u_d));
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_PCKS_E0, index0, S_UNIFORM, c, log_n, 2 * smudge_bound + 1, nullptr, 0, r_d));
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_PCKS_E1, index0, S_ERROR, c, log_n, q, cdt_d, n_cdt, e1_d));
    ZK_CK(launch_rns_ntt<NP>(ctx, true, c1_d, LOAD_RESIDUE, q, c, log_n, hat_s, 0, res, flag));
    ZK_CK(zk_bfv_epilogue(ctx, res, c, log_n, q, Epi{}, sc_d));   // s_i c1_j
    ZK_CK(launch_rns_ntt<NP>(ctx, true, u_d, LOAD_TERNARY, q, c, log_n, hat_pk, 0, res, flag));
    ZK_CK(zk_bfv_epilogue(ctx, res, c, log_n, q, Epi{.mode = EPI_SHARE_ADD, .e = r_d, .a = sc_d, .bound = smudge_bound}, h0_d));
    ZK_CK(launch_rns_ntt<NP>(ctx, true, u_d, LOAD_TERNARY, q, c, log_n, hat_pk + NP * n, 0, res, flag));
    ZK_CK(zk_bfv_epilogue(ctx, res, c, log_n, q, Epi{.mode = EPI_ADD, .e = e1_d}, h1_d));
    ZK_CK(zkfhe_download(ctx, h0_out + lo * n, h0_d, bytes));
    ZK_CK(zkfhe_download(ctx, h1_out + lo * n, h1_d, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_pcks_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint64_t *c0,
                           const uint64_t *h0, const uint64_t *h1, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  if (!(ctx && c0 && h0 && h1 && out0 && out1 && n_parties > 0 && n_cts > 0)) return null_or_zero(ctx, "bfv_pcks_combine");
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const size_t stride = n_cts * n;   // words of one party's shares
  ZK_CK(check_below_q(ctx, c0, stride, q, "bfv_pcks_combine", "a ciphertext"));
  ZK_CK(check_below_q(ctx, h0, n_parties * stride, q, "bfv_pcks_combine", "a share", h1));
  const size_t chunk = plane_chunk(n, 2 * n_parties + 3, n_cts), cw = chunk * n;
  uint64_t *c0_d, *h0_d, *h1_d, *o0_d, *o1_d;
  ZK_CK(Arena().add(c0_d, cw).add(h0_d, n_parties * cw).add(h1_d, n_parties * cw).add(o0_d, cw).add(o1_d, cw).carve(ctx));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), words = c * n;
    ZK_CK(zkfhe_upload(ctx, c0_d, c0 + lo * n, words * 8));
    ZK_CK(upload_planes(ctx, h0_d, h0, n_parties, stride, lo * n, words));
    ZK_CK(upload_planes(ctx, h1_d, h1, n_parties, stride, lo * n, words));
    zk_prof_begin(ctx);
    k_bfv_pcks_combine<<<zk_blocks(words, 256), 256, 0, ctx->stream>>>(c0_d, h0_d, h1_d, n_parties, words, q, o0_d, o1_d);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_PCKS_COMBINE, (double)(2 * n_parties + 3) * words * 8);
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, o0_d, words * 8));
    ZK_CK(zkfhe_download(ctx, out1 + lo * n, o1_d, words * 8));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_refresh_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t crs_seed[32], size_t n_cts,
                            const uint64_t *c1, const uint8_t seed[32], uint64_t first_index, uint64_t smudge_bound, uint64_t *h0_out,
                            uint64_t *h1_out) {
  ZK_ENTER(ctx);
  if (!(ctx && sk_i && crs_seed && c1 && seed && h0_out && h1_out && n_cts > 0)) return null_or_zero(ctx, "bfv_refresh_share");
  ZK_CK(check_params(ctx, params));
  ZK_CK(check_smudge(ctx, params, smudge_bound, "bfv_refresh_share"));
  const uint64_t n = params->n, q = params->q, t = params->t, delta = q / t;
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_refresh_share", "a ciphertext"));
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  const size_t chunk = plane_chunk(n, 10, n_cts), cw = chunk * n;
  int *flag;
  uint64_t *s_d, *cdt_d, *src, *m_d, *r_d, *e1_d, *h0_d, *h1_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(cdt_d, n_cdt).add(hat, NP * n).add(src, 2 * cw).add(m_d, cw).add(r_d, cw).add(e1_d, cw)
            .add(h0_d, cw).add(h1_d, cw).add(res, 2 * cw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk_i, n, q, s_d, hat, flag, "bfv_refresh_share"));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), words = c * n;
    const uint64_t index0 = first_index + lo;
    ZK_CK(zkfhe_upload(ctx, src, c1 + lo * n, words * 8));   // c1_j | a_j: 2c rows against s_i^
    ZK_CK(zk_bfv_sample(ctx, crs_seed, DOM_RFR_A, index0, S_UNIFORM, c, log_n, q, nullptr, 0, src + words));
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_RFR_M, index0, S_UNIFORM, c, log_n, t, nullptr, 0, m_d));
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_RFR_E0, index0, S_UNIFORM, c, log_n, 2 * smudge_bound + 1, nullptr, 0, r_d));
    ZK_CK(zk_bfv_sample(ctx, seed, DOM_RFR_E1, index0, S_ERROR, c, log_n, q, cdt_d, n_cdt, e1_d));
    ZK_CK(launch_rns_ntt<NP>(ctx, true, src, LOAD_RESIDUE, q, 2 * c, log_n, hat, 0, res, flag));
    ZK_CK(zk_bfv_epilogue(ctx, res, c, log_n, q, Epi{.mode = EPI_MASK, .m = m_d, .e = r_d, .delta = delta, .bound = smudge_bound}, h0_d));
    ZK_CK(zk_bfv_epilogue(ctx, res + words * NP, c, log_n, q, Epi{.mode = EPI_MASK, .m = m_d, .e = e1_d, .delta = delta, .neg_x = 1}, h1_d));
    ZK_CK(zkfhe_download(ctx, h0_out + lo * n, h0_d, words * 8));
    ZK_CK(zkfhe_download(ctx, h1_out + lo * n, h1_d, words * 8));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_refresh_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint8_t crs_seed[32],
                              uint64_t first_index, const uint64_t *c0, const uint64_t *h0, const uint64_t *h1, uint64_t *out0,
                              uint64_t *out1) {
  ZK_ENTER(ctx);
  if (!(ctx && crs_seed && c0 && h0 && h1 && out0 && out1 && n_parties > 0 && n_cts > 0)) return null_or_zero(ctx, "bfv_refresh_combine");
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const size_t stride = n_cts * n;   // words of one party's shares
  ZK_CK(check_below_q(ctx, c0, stride, q, "bfv_refresh_combine", "a ciphertext"));
  ZK_CK(check_below_q(ctx, h0, n_parties * stride, q, "bfv_refresh_combine", "a share", h1));
  const int log_n = bit_log2(n);
  const size_t chunk = plane_chunk(n, 2 * n_parties + 3, n_cts), cw = chunk * n;
  uint64_t *c0_d, *h0_d, *h1_d, *o0_d, *a_d;
  ZK_CK(Arena().add(c0_d, cw).add(h0_d, n_parties * cw).add(h1_d, n_parties * cw).add(o0_d, cw).add(a_d, cw).carve(ctx));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), words = c * n;
    ZK_CK(zkfhe_upload(ctx, c0_d, c0 + lo * n, words * 8));
    ZK_CK(upload_planes(ctx, h0_d, h0, n_parties, stride, lo * n, words));
    ZK_CK(upload_planes(ctx, h1_d, h1, n_parties, stride, lo * n, words));
    ZK_CK(zk_bfv_sample(ctx, crs_seed, DOM_RFR_A, first_index + lo, S_UNIFORM, c, log_n, q, nullptr, 0, a_d));   // out1 = a_j
    zk_prof_begin(ctx);
    k_bfv_refresh_combine<<<zk_blocks(words, 256), 256, 0, ctx->stream>>>(c0_d, h0_d, h1_d, n_parties, words, q, params->t, o0_d);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_REFRESH_COMBINE, (double)(2 * n_parties + 2) * words * 8);
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, o0_d, words * 8));
    ZK_CK(zkfhe_download(ctx, out1 + lo * n, a_d, words * 8));
  }
  return ZKFHE_OK;
}

}  // extern "C"
