// Resident evaluation keys (zkfhe.h "Evaluation keys that stay on the device", INTEGRATION.md "Keys that stay on the device"): one
// relinearization key and any number of Galois keys, checked, uploaded and transformed once, and the digit-parallel key switch that
// the batch calls on a key set (bfv_resident.hip: zkfhe_bfv_cts_*_evk, slot_sum, dot) use for a handful of ciphertexts.
//
// A key set is one device allocation of its own: for the relinearization key (if any) and then for each Galois key in the order of
// `g`, the [2 l][5][N] uint32_t transform that k_key_switch reads (the l rows of key0, then the l rows of key1).  Creation stages the
// keys through the work arena (upload_key_pair, as stage_keys of rns_ntt.hip.hpp does for a host-array call) and runs k_rns_ntt
// (LOAD_RESIDUE, five primes) straight into the set, so the stored words are exactly the key_hat that a host-array call computes per
// call.  The set is read-only afterwards and complete when creation returns: any context of the device may read it from its own
// stream.  A call that takes the set hands its keys to the operation's runner as a resident KeySource, which stages nothing.
//
// The digit-parallel key switch.  k_key_switch (bfv_eval.hip) runs one workgroup per (ciphertext, prime) that walks the l digits
// one after the other: 5 workgroups for one ciphertext.  Here the l digit transforms run side by side:
//   k_key_switch_digit<GALOIS>  one workgroup per (digit, ciphertext, prime): the digit is loaded as k_key_switch loads it (auto_coeff
//                               for GALOIS), transformed in LDS, multiplied by the two key rows of the digit and written to
//                               part[digit][comp][k][prime][N]
//   k_key_switch_fold           one workgroup per (comp, ciphertext, prime): the l partials summed mod p into LDS, one inverse
//                               transform, the scale rc.scale, into the acc layout that k_eval_epilogue reads
// Bit for bit k_key_switch: mont_mul reduces its r < 2 p once and add_p its s < 2 p once, so both return the canonical residue in
// [0, p) of canonical operands; rns_forward maps canonical residues to canonical residues (add_p, sub_p, mont_mul); the key rows are
// outputs of rns_forward.  So every partial is the canonical residue of x_i key_i R^-1 mod p, a sum of canonical residues taken
// mod p by add_p is the canonical residue of the integer sum in any order, and the fold hands rns_inverse the very word that
// k_key_switch holds in acc after its last digit.  No kernel uses scratch; neither branches on or addresses by a coefficient's value.
#include <cstdlib>
#include <string>

#include "rns_ntt.hip.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;

// blockIdx.x = (digit * c + k) * NP + prime.  src: [c][N] in CircuitInput order; key_hat: [2 l][NP][N]; part: [l][2][c][NP][N].
template <bool GALOIS>
__global__ __launch_bounds__(NTT_THREADS) void k_key_switch_digit(const uint64_t *__restrict__ src, int l, int w, const uint32_t *__restrict__ key_hat,
                                                                  size_t c, int log_n, const uint32_t *__restrict__ tw, RnsConst<NP> rc,
                                                                  uint32_t *__restrict__ part, unsigned ginv, uint64_t q) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t ik = blockIdx.x / NP, i = ik / c, k = ik % c;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n;
  const uint64_t *s = src + k * n, mask = ((uint64_t)1 << w) - 1;
  const int shift = (int)i * w;   // < bitlen(Q - 1) <= 63
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    const uint64_t v = GALOIS ? auto_coeff(s, d, ginv, n, q) : s[n - 1 - d];
    lds[d] = (uint32_t)(((v >> shift) & mask) % p);
  }
  __syncthreads();
  rns_forward(lds, tw + (size_t)j * 2 * NMAX, log_n, p, pinv);
  const uint32_t *r0 = key_hat + i * plane + (size_t)j * n, *r1 = key_hat + ((size_t)l + i) * plane + (size_t)j * n;
  uint32_t *o0 = part + ((i * 2) * c + k) * plane + (size_t)j * n, *o1 = o0 + c * plane;
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    const uint32_t x = lds[d];
    o0[d] = mont_mul(x, r0[d], p, pinv);
    o1[d] = mont_mul(x, r1[d], p, pinv);
  }
}

// blockIdx.x = (comp * c + k) * NP + prime, which is also the polynomial of acc ([2][c][NP][N]) that the workgroup writes
__global__ __launch_bounds__(NTT_THREADS) void k_key_switch_fold(const uint32_t *__restrict__ part, int l, size_t c, int log_n,
                                                                 const uint32_t *__restrict__ tw, RnsConst<NP> rc, uint32_t *__restrict__ acc) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t digit_stride = 2 * c * NP * (size_t)n;
  const uint32_t *s = part + (size_t)blockIdx.x * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    uint32_t v = s[d];
    for (int i = 1; i < l; ++i) v = add_p(v, s[i * digit_stride + d], p);
    lds[d] = v;
  }
  __syncthreads();
  rns_inverse(lds, tw + (size_t)j * 2 * NMAX + NMAX, log_n, p, pinv);
  uint32_t *o = acc + (size_t)blockIdx.x * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) o[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
}

// Where the digit-parallel path stops: the grid of k_key_switch_digit, c 5 l workgroups, is at most WIDE_GRID_NUM / WIDE_GRID_DEN
// workgroups per CU of the device.  Measured on the MI355X (profiles/bfv_evk.md): up to 5/4 of the CU count the two kernels'
// slowest repeat lay below k_key_switch's fastest at every N, w and kind of key switch measured; past it not at every one.
constexpr size_t WIDE_GRID_NUM = 5, WIDE_GRID_DEN = 4;

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

int refuse(zkfhe_ctx *ctx, const char *fn, const std::string &what) { return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": " + what); }

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

size_t zk_bfv_wide_max(const zkfhe_ctx *ctx, uint64_t n, int l) {
  if (l < 2) return 0;
  // the partials ([l][2][c][5][N]) stay within the accumulators of a full chunk ([2][chunk_polys][5][N])
  const size_t room = chunk_polys(n) / (size_t)l;
  static const char *forced = getenv("ZKFHE_EVK_WIDE_MAX");   // measurements only: the bound itself, still within the arena's room
  if (forced) return std::min<size_t>(room, strtoull(forced, nullptr, 10));
  const size_t by_grid = (size_t)std::max(ctx->num_cu, 1) * WIDE_GRID_NUM / (WIDE_GRID_DEN * NP * (size_t)l);
  return std::min(room, by_grid);
}

int zk_bfv_key_switch_wide(zkfhe_ctx *ctx, const uint64_t *src, unsigned ginv, uint64_t q, int l, int w, const uint32_t *key_hat, size_t c,
                           int log_n, uint32_t *part, uint32_t *acc) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds;
  ZK_CK(ntt_lds(ctx, ginv ? (const void *)k_key_switch_digit<true> : (const void *)k_key_switch_digit<false>, log_n, &lds));
  const RnsConst<NP> rc = rns_const<NP>(log_n);
  const double words = (double)c * NP * ((size_t)1 << log_n);
  zk_prof_begin(ctx);
  if (ginv)
    k_key_switch_digit<true><<<(unsigned)(c * NP * l), NTT_THREADS, lds, ctx->stream>>>(src, l, w, key_hat, c, log_n, tw, rc, part, ginv, q);
  else
    k_key_switch_digit<false><<<(unsigned)(c * NP * l), NTT_THREADS, lds, ctx->stream>>>(src, l, w, key_hat, c, log_n, tw, rc, part, 0, q);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_KEY_SWITCH_WIDE, words * l * (8.0 + 8.0 + 8.0));   // the digit's source, two key rows, two partials
  return zk_bfv_key_switch_fold(ctx, part, l, c, log_n, acc);
}

int zk_bfv_key_switch_fold(zkfhe_ctx *ctx, const uint32_t *part, int l, size_t c, int log_n, uint32_t *acc) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds;
  ZK_CK(ntt_lds(ctx, (const void *)k_key_switch_fold, log_n, &lds));
  const double words = (double)c * NP * ((size_t)1 << log_n);
  zk_prof_begin(ctx);
  k_key_switch_fold<<<(unsigned)(2 * c * NP), NTT_THREADS, lds, ctx->stream>>>(part, l, c, log_n, tw, rns_const<NP>(log_n), acc);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_KEY_SWITCH_WIDE, words * 2 * (4.0 * l + 4.0));
  return ZKFHE_OK;
}

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
