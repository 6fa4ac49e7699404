// Resident evaluation keys (zkfhe.h "Evaluation keys that stay on the device", INTEGRATION.md "Keys that stay on the device"): one
// relinearization key and any number of Galois keys, checked, uploaded and transformed once.
//
// A key set is one device allocation of its own: for the relinearization key (if any) and then for each Galois key in the order of
// `g`, the [2 l][5][N] uint32_t transform that the key switch (bfv_key_switch.hip) reads (the l rows of key0, then the l rows of
// key1).  Creation stages the keys through the work arena (upload_key_pair, as stage_keys of bfv_host.hpp does for a host-array
// call) and runs k_rns_ntt (LOAD_RESIDUE, five primes) straight into the set, so the stored words are exactly the key_hat that a
// host-array call computes per call.  The set is read-only afterwards and complete when creation returns: any context of the device
// may read it from its own stream.  A call that takes the set hands its keys to the operation's runner as a resident KeySource,
// which stages nothing, and whose key switches of a handful of ciphertexts go the digit-parallel way (KeySwitch, bfv_host.hpp).
//
// A hybrid set (zkfhe.h "Evaluation keys modulo Q P: hybrid key switching") has the same layout.  Its rows are integers K below Q P
// for a special modulus P, given as the planes K mod Q and K mod P; k_hybrid_key_ntt forms K mod p_j for the five primes by Garner
// (t = (kp - kq) Q^-1 mod P, K = kq + Q t) and runs the forward transform of k_rns_ntt, whose instantiations stay as they are.  The
// key switch reads such a set as any other; the set carries P to the epilogues, which divide the sum by it.
#include <numeric>
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
typedef unsigned __int128 u128;

// One workgroup per (row, prime), blockIdx.x = row * NP + prime, as k_rns_ntt<NP, false>: coefficient K = kq + Q t of the row with
// t = (kp - kq) q_inv mod P (q_inv = Q^-1 mod P) is loaded as K mod p = (kq + (Q mod p)(t mod p)) mod p, then the forward transform
// into out[row][prime][N].  kq, kp: [rows][N] in CircuitInput order, words below Q and below P.
__global__ __launch_bounds__(NTT_THREADS) void k_hybrid_key_ntt(const uint64_t *__restrict__ kq, const uint64_t *__restrict__ kp, uint64_t q,
                                                                 uint64_t sp, uint64_t q_inv, int log_n, const uint32_t *__restrict__ tw,
                                                                 RnsConst<NP> rc, uint32_t *__restrict__ out) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t row = blockIdx.x / NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const uint64_t q_p = q % p;
  const uint64_t *rq = kq + row * n, *rp = kp + row * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    const uint64_t a = rq[n - 1 - d];
    const u128 prod = (u128)sub_q(rp[n - 1 - d], a % sp, sp) * q_inv;   // < P^2 < 2^126
    const uint64_t t = mod128((uint64_t)(prod >> 64), (uint64_t)prod, sp);
    lds[d] = (uint32_t)((a % p + q_p * (t % p)) % p);   // < 2^31 + 2^62
  }
  __syncthreads();
  rns_forward(lds, tw + (size_t)j * 2 * NMAX, log_n, p, pinv);
  uint32_t *o = out + (row * NP + j) * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) o[d] = lds[d];
}

// a^-1 mod m for coprime a, m (m >= 2)
uint64_t inv_mod(uint64_t a, uint64_t m) {
  __int128 r0 = m, r1 = a % m, t0 = 0, t1 = 1;
  while (r1) {
    const __int128 k = r0 / r1, r2 = r0 - k * r1, t2 = t0 - k * t1;
    r0 = r1, r1 = r2, t0 = t1, t1 = t2;
  }
  return (uint64_t)(t0 < 0 ? t0 + m : t0);
}

// x ([3] little-endian limbs) divided by d in place
void div_limbs(uint64_t x[3], uint64_t d) {
  u128 r = 0;
  for (int i = 2; i >= 0; --i) {
    const u128 cur = (r << 64) | x[i];
    x[i] = (uint64_t)(cur / d), r = cur % d;
  }
}

}  // namespace

struct zkfhe_bfv_evk {
  zkfhe_bfv_params params{};
  int device = 0;   // of the context that made it
  int base_bits = 0, l = 0;
  bool has_relin = false;
  uint64_t special = 1;       // the special modulus P of a hybrid set; 1: an ordinary set
  std::vector<uint64_t> g;    // the Galois elements, in the order of their keys
  uint32_t *hat = nullptr;    // the allocation: [has_relin + g.size()][2 l][NP][N]
  uint64_t device_bytes = 0;
  size_t key_words() const { return (size_t)2 * l * NP * params.n; }
};

namespace {

// the bytes of a set, or "does not fit"
int evk_size(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int l, size_t keys, const char *fn, uint64_t *bytes) {
  // keys < 2^64, 2 l NP N 4 < 2^7 2^3 2^15 2^2: the product fits 128 bits
  const unsigned __int128 total = (unsigned __int128)keys * 2 * l * NP * params->n * 4;
  if (total >> 64) return refuse(ctx, fn, "the size does not fit 64 bits");
  *bytes = (uint64_t)total;
  return ZKFHE_OK;
}

void evk_free(zkfhe_bfv_evk *e) {
  if (!e) return;
  (void)hipFree(e->hat);   // waits for the device
  delete e;
}

// "fn: what p-plane coefficient is not below P" if any v[i] or v2[i] >= P
int check_below_p(zkfhe_ctx *ctx, const uint64_t *v, const uint64_t *v2, size_t count, uint64_t p, const char *fn, const char *what) {
  bool bad = false;
  for (size_t i = 0; i < count; ++i) bad |= (v[i] >= p) | (v2[i] >= p);
  if (bad) return refuse(ctx, fn, std::string(what) + " p-plane coefficient is not below P");
  return ZKFHE_OK;
}

// The special modulus and the p-planes of a hybrid set, in the shapes of the q-planes rlk0, rlk1, gk0, gk1 (an ordinary set: none)
struct PPlanes {
  bool hybrid = false;
  uint64_t p = 1;
  const uint64_t *rlk0 = nullptr, *rlk1 = nullptr, *gk0 = nullptr, *gk1 = nullptr;
};

int evk_fill(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, const uint64_t *rlk0, const uint64_t *rlk1, size_t n_galois,
             const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, const PPlanes &pp, const char *fn, zkfhe_bfv_evk *e) {
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  const bool hybrid = pp.hybrid;
  if (hybrid) ZK_CK(check_special(ctx, params, l, base_bits, pp.p, fn));
  const uint64_t n = params->n, q = params->q;
  const size_t lw = (size_t)l * n;
  for (size_t i = 0; i < n_galois; ++i) ZK_CK(check_g(ctx, n, g[i], fn));
  std::vector<uint64_t> sorted(g, g + n_galois);
  std::sort(sorted.begin(), sorted.end());
  const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
  if (twice != sorted.end()) return refuse(ctx, fn, "the Galois element " + std::to_string(*twice) + " is repeated");
  if (rlk0) ZK_CK(check_below_q(ctx, rlk0, lw, q, fn, "a relinearization-key", rlk1));
  if (n_galois) {
    if ((n_galois * lw) / lw != n_galois) return refuse(ctx, fn, "the size does not fit 64 bits");
    ZK_CK(check_below_q(ctx, gk0, n_galois * lw, q, fn, "a Galois-key", gk1));
  }
  if (hybrid && rlk0) ZK_CK(check_below_p(ctx, pp.rlk0, pp.rlk1, lw, pp.p, fn, "a relinearization-key"));
  if (hybrid && n_galois) ZK_CK(check_below_p(ctx, pp.gk0, pp.gk1, n_galois * lw, pp.p, fn, "a Galois-key"));
  e->special = pp.p;
  e->params = *params, e->device = ctx->device, e->base_bits = base_bits, e->l = l, e->has_relin = rlk0 != nullptr;
  e->g.assign(g, g + n_galois);
  const size_t keys = (size_t)e->has_relin + n_galois;
  ZK_CK(evk_size(ctx, params, l, keys, fn, &e->device_bytes));
  const hipError_t err = hipMalloc(&e->hat, e->device_bytes);
  if (err == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    e->hat = nullptr;
    return zk_fail_msg(ctx, ZKFHE_ENOMEM, std::string(fn) + ": out of device memory");
  }
  ZK_HIP(ctx, err);
  // as many whole keys per chunk as the chunk rule allows, at least one: staged in the arena, transformed straight into the set
  const size_t per = std::min(keys, std::max<size_t>(1, chunk_polys(n) / (2 * (size_t)l)));
  int *flag;
  uint64_t *key_d, *keyp_d = nullptr;
  Arena ar;
  ar.add(flag, 1).add(key_d, per * 2 * lw);
  if (hybrid) ar.add(keyp_d, per * 2 * lw);
  ZK_CK(ar.carve(ctx));
  const int log_n = bit_log2(n);
  const uint64_t q_inv = hybrid ? inv_mod(q, pp.p) : 0;
  for (size_t lo = 0; lo < keys; lo += per) {
    const size_t c = std::min(per, keys - lo);
    for (size_t i = 0; i < c; ++i) {   // key lo + i: its key0 rows, then its key1 rows
      const size_t at = lo + i;
      const bool relin = e->has_relin && at == 0;
      const size_t gi = at - (e->has_relin ? 1 : 0);
      ZK_CK(upload_key_pair(ctx, key_d + 2 * i * lw, relin ? rlk0 : gk0 + gi * lw, relin ? rlk1 : gk1 + gi * lw, lw));
      if (hybrid) ZK_CK(upload_key_pair(ctx, keyp_d + 2 * i * lw, relin ? pp.rlk0 : pp.gk0 + gi * lw, relin ? pp.rlk1 : pp.gk1 + gi * lw, lw));
    }
    uint32_t *hat = e->hat + lo * e->key_words();
    if (!hybrid) {
      ZK_CK(launch_rns_ntt<NP>(ctx, false, key_d, LOAD_RESIDUE, q, 2 * c * l, log_n, nullptr, 0, hat, flag));
      continue;
    }
    const uint32_t *tw;
    ZK_CK(zk_rns_tables(ctx, &tw));
    int lds;
    ZK_CK(ntt_lds(ctx, (const void *)k_hybrid_key_ntt, log_n, &lds));
    zk_prof_begin(ctx);
    k_hybrid_key_ntt<<<(unsigned)(2 * c * l * NP), NTT_THREADS, lds, ctx->stream>>>(key_d, keyp_d, q, pp.p, q_inv, log_n, tw, rns_const<NP>(log_n), hat);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_RNS_NTT, (double)(2 * c * l) * NP * (16.0 + 4.0) * n);
  }
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

}  // namespace

namespace zkrns {

void zk_bfv_evk_view(const zkfhe_bfv_evk *evk, EvkView *view) {
  view->params = evk->params, view->device = evk->device, view->base_bits = evk->base_bits, view->l = evk->l;
  view->rlk_hat = evk->has_relin ? evk->hat : nullptr;
  view->special = evk->special;
}

const uint32_t *zk_bfv_evk_galois(const zkfhe_bfv_evk *evk, uint64_t g) {
  for (size_t i = 0; i < evk->g.size(); ++i)
    if (evk->g[i] == g) return evk->hat + (i + (evk->has_relin ? 1 : 0)) * evk->key_words();
  return nullptr;
}

uint64_t hybrid_max_p(const zkfhe_bfv_params *prm, int l, int base_bits) {
  // Q P <= floor(H / (l N (2^w - 1))) + 1 with H = floor(P5 / 2); l N (2^w - 1) < 2^6 2^15 2^32
  const Crt5 cc = crt5_const();
  uint64_t x[3] = {cc.H[0], cc.H[1], cc.H[2]};
  div_limbs(x, (uint64_t)l * prm->n * (((uint64_t)1 << base_bits) - 1));
  for (int i = 0; i < 3 && ++x[i] == 0; ++i) {}
  div_limbs(x, prm->q);
  const uint64_t top = ((uint64_t)1 << 63) - 1;
  return x[2] || x[1] || x[0] > top ? top : x[0];
}

int check_special(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, int l, int base_bits, uint64_t p, const char *fn) {
  if (p < 2 || (p >> 63)) return refuse(ctx, fn, "P must satisfy 2 <= P < 2^63");
  if (std::gcd(p, prm->q) != 1) return refuse(ctx, fn, "P and Q must be coprime");
  const uint64_t limit = hybrid_max_p(prm, l, base_bits);
  if (p > limit) return refuse(ctx, fn, "P is above the limit " + std::to_string(limit) + " of zkfhe_bfv_hybrid_max_p");
  return ZKFHE_OK;
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_evk_create(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, const uint64_t *rlk0, const uint64_t *rlk1, size_t n_galois,
                         const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, zkfhe_bfv_evk **out) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_evk_create";
  if (out) *out = nullptr;
  if (!(ctx && params && out) || !rlk0 != !rlk1 || (n_galois > 0 && !(g && gk0 && gk1))) return refuse(ctx, fn, "a NULL argument or a zero count");
  if (!rlk0 && n_galois == 0) return refuse(ctx, fn, "neither a relinearization key nor a Galois key");
  zkfhe_bfv_evk *e = new zkfhe_bfv_evk;
  const int rc = evk_fill(ctx, params, base_bits, rlk0, rlk1, n_galois, g, gk0, gk1, PPlanes{}, fn, e);
  if (rc) {
    evk_free(e);
    return rc;
  }
  *out = e;
  return ZKFHE_OK;
}

int zkfhe_bfv_evk_create_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, int base_bits, const uint64_t *rlk0_q,
                                const uint64_t *rlk1_q, const uint64_t *rlk0_p, const uint64_t *rlk1_p, size_t n_galois, const uint64_t *g,
                                const uint64_t *gk0_q, const uint64_t *gk1_q, const uint64_t *gk0_p, const uint64_t *gk1_p, zkfhe_bfv_evk **out) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_evk_create_hybrid";
  if (out) *out = nullptr;
  const bool relin = rlk0_q != nullptr;
  if (!(ctx && params && out) || relin != (rlk1_q != nullptr) || relin != (rlk0_p != nullptr) || relin != (rlk1_p != nullptr) ||
      (n_galois > 0 && !(g && gk0_q && gk1_q && gk0_p && gk1_p)))
    return refuse(ctx, fn, "a NULL argument or a zero count");
  if (!relin && n_galois == 0) return refuse(ctx, fn, "neither a relinearization key nor a Galois key");
  zkfhe_bfv_evk *e = new zkfhe_bfv_evk;
  const int rc = evk_fill(ctx, params, base_bits, rlk0_q, rlk1_q, n_galois, g, gk0_q, gk1_q, PPlanes{true, p, rlk0_p, rlk1_p, gk0_p, gk1_p}, fn, e);
  if (rc) {
    evk_free(e);
    return rc;
  }
  *out = e;
  return ZKFHE_OK;
}

int zkfhe_bfv_evk_special_modulus(const zkfhe_bfv_evk *evk, uint64_t *p) {
  if (!(evk && p)) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_evk_special_modulus: a NULL argument");
  *p = evk->special;
  return ZKFHE_OK;
}

int zkfhe_bfv_hybrid_max_p(const zkfhe_bfv_params *params, int base_bits, uint64_t *p_max) {
  if (!p_max) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_hybrid_max_p: p_max is NULL");
  ZK_CK(check_params(nullptr, params));
  int l = 0;
  ZK_CK(relin_rows(nullptr, params, base_bits, "bfv_hybrid_max_p", &l));
  *p_max = hybrid_max_p(params, l, base_bits);
  return ZKFHE_OK;
}

int zkfhe_bfv_evk_bytes(const zkfhe_bfv_params *params, int base_bits, int has_relin, size_t n_galois, uint64_t *bytes) {
  if (!bytes) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_evk_bytes: bytes is NULL");
  ZK_CK(check_params(nullptr, params));
  int l = 0;
  ZK_CK(relin_rows(nullptr, params, base_bits, "bfv_evk_bytes", &l));
  const unsigned __int128 keys = (unsigned __int128)n_galois + (has_relin ? 1 : 0);
  if (keys >> 64) return refuse(nullptr, "bfv_evk_bytes", "the size does not fit 64 bits");
  return evk_size(nullptr, params, l, (size_t)keys, "bfv_evk_bytes", bytes);
}

int zkfhe_bfv_evk_info(const zkfhe_bfv_evk *evk, zkfhe_bfv_params *params, int *base_bits, int *has_relin, size_t *n_galois, uint64_t *g_out,
                       uint64_t *device_bytes) {
  if (!evk) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_evk_info: evk is NULL");
  if (params) *params = evk->params;
  if (base_bits) *base_bits = evk->base_bits;
  if (has_relin) *has_relin = evk->has_relin;
  if (n_galois) *n_galois = evk->g.size();
  if (g_out) std::copy(evk->g.begin(), evk->g.end(), g_out);
  if (device_bytes) *device_bytes = evk->device_bytes;
  return ZKFHE_OK;
}

int zkfhe_bfv_evk_destroy(zkfhe_ctx *ctx, zkfhe_bfv_evk *evk) {
  ZK_ENTER(ctx);
  if (!evk) return ZKFHE_OK;
  if (ctx) ZK_HIP(ctx, zk_wait(ctx));   // what this context has queued against the set
  evk_free(evk);
  return ZKFHE_OK;
}

int zkfhe_bfv_evk_wide_max(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, size_t *c_max) {
  ZK_ENTER(ctx);
  const char *fn = "bfv_evk_wide_max";
  if (!(ctx && c_max)) return refuse(ctx, fn, "a NULL argument or a zero count");
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
  *c_max = zk_bfv_wide_max(ctx, params->n, l);
  return ZKFHE_OK;
}

}  // extern "C"
