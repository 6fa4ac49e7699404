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
#include <string>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;

}  // namespace

struct zkfhe_bfv_evk {
  zkfhe_bfv_params params{};
  int device = 0;   // of the context that made it
  int base_bits = 0, l = 0;
  bool has_relin = false;
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

int evk_fill(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, const uint64_t *rlk0, const uint64_t *rlk1, size_t n_galois,
             const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, const char *fn, zkfhe_bfv_evk *e) {
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, fn, &l));
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
  uint64_t *key_d;
  ZK_CK(Arena().add(flag, 1).add(key_d, per * 2 * lw).carve(ctx));
  const int log_n = bit_log2(n);
  for (size_t lo = 0; lo < keys; lo += per) {
    const size_t c = std::min(per, keys - lo);
    for (size_t i = 0; i < c; ++i) {   // key lo + i: its key0 rows, then its key1 rows
      const size_t at = lo + i;
      const bool relin = e->has_relin && at == 0;
      const size_t gi = at - (e->has_relin ? 1 : 0);
      ZK_CK(upload_key_pair(ctx, key_d + 2 * i * lw, relin ? rlk0 : gk0 + gi * lw, relin ? rlk1 : gk1 + gi * lw, lw));
    }
    ZK_CK(launch_rns_ntt<NP>(ctx, false, key_d, LOAD_RESIDUE, q, 2 * c * l, log_n, nullptr, 0, e->hat + lo * e->key_words(), flag));
  }
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}

}  // namespace

namespace zkrns {

void zk_bfv_evk_view(const zkfhe_bfv_evk *evk, EvkView *view) {
  view->params = evk->params, view->device = evk->device, view->base_bits = evk->base_bits, view->l = evk->l;
  view->rlk_hat = evk->has_relin ? evk->hat : nullptr;
}

const uint32_t *zk_bfv_evk_galois(const zkfhe_bfv_evk *evk, uint64_t g) {
  for (size_t i = 0; i < evk->g.size(); ++i)
    if (evk->g[i] == g) return evk->hat + (i + (evk->has_relin ? 1 : 0)) * evk->key_words();
  return nullptr;
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
  const int rc = evk_fill(ctx, params, base_bits, rlk0, rlk1, n_galois, g, gk0, gk1, fn, e);
  if (rc) {
    evk_free(e);
    return rc;
  }
  *out = e;
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
