// Hybrid evaluation keys on the GPU (zkfhe.h "Evaluation keys modulo Q P: hybrid key switching"): a key row is an integer polynomial
// K below Q P, P the special modulus, handed out as its q-plane K mod Q and its p-plane K mod P.  Conventions of bfv_enc.hip.
//   q-plane  K0_i = -(aQ_i s + e_i) + (P mod Q) 2^(i w) G mod Q, K1_i = aQ_i: the ordinary key with its gadget scaled by P
//   p-plane  K0_i = -(aP_i s + e_i) mod P,                        K1_i = aP_i: the gadget is a multiple of P
// G is s^2 (relinearization) or sigma_g(s) (Galois); aQ_i and e_i are the streams of the ordinary keys, aP_i a stream of its own.
// Both planes are the five-prime product a_i s of k_rns_ntt against the transform of s, then k_eval_epilogue in EV_RLK mode with the
// plane's modulus and the plane's gadget: k_hybrid_plane writes (P mod Q) sigma_g(G) for the q-plane, and moves the error, sampled
// once as residues mod Q, to residues mod P; the p-plane's gadget is zero.  The kernel uses no scratch and neither branches on nor
// addresses by a coefficient's value.
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
typedef unsigned __int128 u128;

// One thread per coefficient of out (total words, polynomials of N): the centred integer of sigma_g(v) mod Q (ginv = g^-1 mod 2N;
// 1: v itself) times scale, as a residue mod m (scale < m < 2^63)
__global__ __launch_bounds__(256) void k_hybrid_plane(const uint64_t *__restrict__ v, unsigned ginv, size_t total, int log_n, uint64_t q,
                                                      uint64_t scale, uint64_t m, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const unsigned n = 1u << log_n, d = (unsigned)(g & (n - 1));
  const size_t poly = g >> log_n;
  const uint64_t x = auto_coeff(v + poly * n, d, ginv, n, q);
  const bool neg = x > q / 2;
  const u128 prod = (u128)((neg ? q - x : x) % m) * scale;
  const uint64_t r = mod128((uint64_t)(prod >> 64), (uint64_t)prod, m);
  out[poly * n + (n - 1 - d)] = neg && r ? m - r : r;
}

int hybrid_plane(zkfhe_ctx *ctx, const uint64_t *v, unsigned ginv, size_t n_polys, int log_n, uint64_t q, uint64_t scale, uint64_t m,
                 uint64_t *out) {
  const size_t total = n_polys << log_n;
  zk_prof_begin(ctx);
  k_hybrid_plane<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(v, ginv, total, log_n, q, scale, m, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_ELEMENTWISE, (double)total * 16);
  return ZKFHE_OK;
}

// The four planes of one hybrid key: relin (G = s^2; domains 7, 8, 23, index i) or the Galois key of g (G = sigma_g(s); domains 14,
// 15, 24, index g 64 + i).  The a_i come from crs_seed, the e_i from party_seed.
int hybrid_key(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk, const uint8_t crs_seed[32],
               const uint8_t party_seed[32], bool relin, uint64_t g, int base_bits, uint64_t *r_q, uint64_t *a_q, uint64_t *r_p, uint64_t *a_p,
               const char *fn) {
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  ZK_CK(check_special(ctx, params, l, base_bits, p, fn));
  if (!relin) ZK_CK(check_g(ctx, params->n, g, fn));
  const uint64_t n = params->n, q = params->q;
  // the error is sampled as a residue mod Q and read back as the centred integer
  if (2 * params->b >= q) return refuse(ctx, fn, "B must be below Q / 2");
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  const size_t lw = (size_t)l * n;
  const Domain dom_a = relin ? DOM_RLK_A : DOM_GK_A, dom_e = relin ? DOM_RLK_E : DOM_GK_E, dom_ap = relin ? DOM_HYB_RLK_A : DOM_HYB_GK_A;
  const uint64_t index0 = relin ? 0 : g * 64;
  int *flag;
  uint64_t *s_d, *s2_d, *gad_d, *a_d, *e_d, *ep_d, *r_d, *cdt_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(s2_d, n).add(gad_d, n).add(a_d, lw).add(e_d, lw).add(ep_d, lw).add(r_d, lw).add(cdt_d, n_cdt)
            .add(hat, NP * n).add(res, lw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk, n, q, s_d, hat, flag, fn));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  const uint64_t *gadget = s_d;
  if (relin) {   // s^2 mod Q: the product of s (read as ternary) with its own transform
    ZK_CK(launch_rns_ntt<NP>(ctx, true, s_d, LOAD_TERNARY, q, 1, log_n, hat, 0, res, flag));
    ZK_CK(zk_bfv_eval_epilogue(ctx, res, 1, log_n, q, EvEpi{}, s2_d));
    gadget = s2_d;
  }
  const unsigned ginv = relin ? 1u : (unsigned)pow_mod(g, n - 1, 2 * n);   // the units mod 2N have order N
  // the q-plane: the gadget (P mod Q) G
  ZK_CK(hybrid_plane(ctx, gadget, ginv, 1, log_n, q, p % q, q, gad_d));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, dom_a, index0, S_UNIFORM, l, log_n, q, nullptr, 0, a_d));
  ZK_CK(zk_bfv_sample(ctx, party_seed, dom_e, index0, S_ERROR, l, log_n, q, cdt_d, n_cdt, e_d));
  ZK_CK(launch_rns_ntt<NP>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat, 0, res, flag));
  ZK_CK(zk_bfv_eval_epilogue(ctx, res, l, log_n, q, EvEpi{.mode = EV_RLK, .add = e_d, .poly = gad_d, .w = base_bits}, r_d));
  ZK_CK(zkfhe_download(ctx, r_q, r_d, lw * 8));
  ZK_CK(zkfhe_download(ctx, a_q, a_d, lw * 8));
  // the p-plane: the same e_i mod P, no gadget; every residue below P, the epilogue reduces mod P
  ZK_CK(hybrid_plane(ctx, e_d, 1, l, log_n, q, 1, p, ep_d));
  ZK_HIP(ctx, hipMemsetAsync(gad_d, 0, n * 8, ctx->stream));
  ZK_CK(zk_bfv_sample(ctx, crs_seed, dom_ap, index0, S_UNIFORM, l, log_n, p, nullptr, 0, a_d));
  ZK_CK(launch_rns_ntt<NP>(ctx, true, a_d, LOAD_RESIDUE, p, l, log_n, hat, 0, res, flag));
  ZK_CK(zk_bfv_eval_epilogue(ctx, res, l, log_n, p, EvEpi{.mode = EV_RLK, .add = ep_d, .poly = gad_d, .w = base_bits}, r_d));
  ZK_CK(zkfhe_download(ctx, r_p, r_d, lw * 8));
  ZK_CK(zkfhe_download(ctx, a_p, a_d, lw * 8));
  return ZKFHE_OK;
}

}  // namespace

extern "C" {

int zkfhe_bfv_relin_keygen_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk, const uint8_t seed[32],
                                  int base_bits, uint64_t *rlk0_q, uint64_t *rlk1_q, uint64_t *rlk0_p, uint64_t *rlk1_p) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && seed && rlk0_q && rlk1_q && rlk0_p && rlk1_p);
  return hybrid_key(ctx, params, p, sk, seed, seed, true, 1, base_bits, rlk0_q, rlk1_q, rlk0_p, rlk1_p, "bfv_relin_keygen_hybrid");
}

int zkfhe_bfv_galois_keygen_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk, const uint8_t seed[32],
                                   uint64_t g, int base_bits, uint64_t *gk0_q, uint64_t *gk1_q, uint64_t *gk0_p, uint64_t *gk1_p) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && seed && gk0_q && gk1_q && gk0_p && gk1_p);
  return hybrid_key(ctx, params, p, sk, seed, seed, false, g, base_bits, gk0_q, gk1_q, gk0_p, gk1_p, "bfv_galois_keygen_hybrid");
}

int zkfhe_bfv_galois_share_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk_i, const uint8_t crs_seed[32],
                                  const uint8_t party_seed[32], uint64_t g, int base_bits, uint64_t *r_q, uint64_t *a_q, uint64_t *r_p,
                                  uint64_t *a_p) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk_i && crs_seed && party_seed && r_q && a_q && r_p && a_p);
  return hybrid_key(ctx, params, p, sk_i, crs_seed, party_seed, false, g, base_bits, r_q, a_q, r_p, a_p, "bfv_galois_share_hybrid");
}

}  // extern "C"
