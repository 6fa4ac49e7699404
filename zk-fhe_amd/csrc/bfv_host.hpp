// The host vocabulary of the BFV units (bfv_*.hip): the work-arena layout, where a call's ciphertexts and keys live, and the index
// of what each unit defines for the others: the host checks, the two CRT epilogues, the key switch, the in-place inverse transform
// and the runners.  The device arithmetic and k_rns_ntt are rns_ntt.hip.hpp's.
#pragma once
#include <string>

#include "key_switch_src.hip.hpp"
#include "rns_ntt.hip.hpp"

namespace zkrns {

// "fn: what" as ZKFHE_EINVAL
inline int refuse(zkfhe_ctx *ctx, const char *fn, const std::string &what) { return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": " + what); }

// ---- defined in bfv_enc.hip (zk_rns_tables: rns_ntt.hip.hpp)
// n_polys samples of ChaCha20 stream (seed, domain, index0 + j) (cdt_dev: the n_cdt thresholds of S_ERROR)
int zk_bfv_sample(zkfhe_ctx *ctx, const uint8_t seed[32], Domain domain, uint64_t index0, SampleKind kind, size_t n_polys, int log_n,
                  uint64_t q, const uint64_t *cdt_dev, int n_cdt, uint64_t *out);
// k_rns_epilogue over res ([n_polys][3][N]) into out (CircuitInput order), in profiling slot ZKFHE_PROF_RNS_EPILOGUE
int zk_bfv_epilogue(zkfhe_ctx *ctx, const uint32_t *res, size_t n_polys, int log_n, uint64_t q, const Epi &epi, uint64_t *out);
// the parameter check of every BFV call (zkfhe.h)
int check_params(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm);
// "fn: what coefficient is not below Q" if any v[i] (or v2[i]: a second array of the same kind, checked in the same pass) >= Q
int check_below_q(zkfhe_ctx *ctx, const uint64_t *v, size_t count, uint64_t q, const char *fn, const char *what,
                  const uint64_t *v2 = nullptr);
// "fn: what coefficient is outside [0, T/2] and [Q - T/2, Q - 1]" if any m[i] is (the circuit's range check)
int check_plain(zkfhe_ctx *ctx, const uint64_t *m, size_t count, uint64_t q, uint64_t t, const char *fn, const char *what = "a plaintext");
// the rows l = ceil(bitlen(Q - 1) / w) of a key of digit width w = base_bits; refuses base_bits outside [1, 32]
int relin_rows(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, int base_bits, const char *fn, int *l);
// the 2 B thresholds of the error sampler
void error_cdt(uint64_t b, uint64_t *t);
// error_cdt of prm->b uploaded to cdt_d (2 B words)
int upload_error_cdt(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, uint64_t *cdt_d);
// the context's grow-only BFV work arena
int work_arena(zkfhe_ctx *ctx, size_t bytes, char **out);

// ---- defined in bfv_eval.hip
// k_eval_epilogue over res ([n_polys][5][N]) into out, in profiling slot ZKFHE_PROF_BFV_EVAL_EPILOGUE (EV_GALOIS: ZKFHE_PROF_BFV_GALOIS)
int zk_bfv_eval_epilogue(zkfhe_ctx *ctx, const uint32_t *res, size_t n_polys, int log_n, uint64_t q, const EvEpi &epi, uint64_t *out);

// ---- defined in bfv_linear.hip
// k_rns_intt over res ([n_polys][5][N]): one inverse transform per polynomial and prime in place, times rc.scale, in profiling slot
// ZKFHE_PROF_RNS_NTT
int zk_rns_intt(zkfhe_ctx *ctx, uint32_t *res, size_t n_polys, int log_n, const RnsConst<NP_MAX> &rc);

// The work buffers of one call, each named once: add() them in order (each 256-byte aligned, so an int flag added first stays in
// the first 256 bytes), then carve() sizes the work arena from the same list and points every buffer into it.
class Arena {
 public:
  template <class T>
  Arena &add(T *&ptr, size_t count) {
    bufs_.push_back({&ptr, align256(count * sizeof(T)), [](void *p, char *at) { *(T **)p = (T *)at; }});
    return *this;
  }
  int carve(zkfhe_ctx *ctx) {
    size_t total = 0;
    for (const Buf &b : bufs_) total += b.bytes;
    char *at;
    ZK_CK(work_arena(ctx, total, &at));
    for (const Buf &b : bufs_) b.set(b.ptr, at), at += b.bytes;
    return ZKFHE_OK;
  }

 private:
  struct Buf {
    void *ptr;
    size_t bytes;
    void (*set)(void *ptr, char *at);
  };
  std::vector<Buf> bufs_;
};

// ---- The runners of the evaluation calls: one chunk loop per operation, on operands that are host arrays or device planes (a
// resident batch) and a key that is host rows or a resident key set.  Every extern "C" entry point, host-array (bfv_eval.hip,
// bfv_galois.hip, bfv_dot.hip) or batch (bfv_resident.hip), is its argument checks and one call of a runner, so a batch call runs
// the kernels of the host-array call, in its order and its profiling slots.  No runner checks a range: its caller has.

// Where the ciphertexts of a call live: two planes c0, c1 ([count][N] each) of host memory or of device memory.  A chunk comes in
// with `in` or `at` and leaves with `out`; a runner reads a chunk completely into the work arena before it writes the chunk's
// result, so a device destination may be a source.  A source is only read.
struct Planes {
  uint64_t *p[2] = {nullptr, nullptr};
  bool dev = false;
  // c polynomials of plane comp from polynomial lo on into the device buffer dst_d: an upload or a copy on the device
  int in(zkfhe_ctx *ctx, int comp, size_t lo, size_t c, uint64_t n, uint64_t *dst_d) const {
    return dev ? zk_copy_d2d(ctx, dst_d, p[comp] + lo * n, c * n * 8) : zkfhe_upload(ctx, dst_d, p[comp] + lo * n, c * n * 8);
  }
  // the same polynomials where a kernel may read them: in the plane itself on the device, else uploaded to stage_d
  int at(zkfhe_ctx *ctx, int comp, size_t lo, size_t c, uint64_t n, uint64_t *stage_d, const uint64_t **x) const {
    *x = dev ? p[comp] + lo * n : stage_d;
    return dev ? ZKFHE_OK : zkfhe_upload(ctx, stage_d, p[comp] + lo * n, c * n * 8);
  }
  // the stage_d that `at` wants, in the caller's arena only where there is something to upload
  void stage(Arena &a, uint64_t *&stage_d, size_t words) const {
    if (!dev) a.add(stage_d, words);
  }
  // c polynomials at src_d into plane comp from polynomial lo on: a download (which waits) or a copy on the device
  int out(zkfhe_ctx *ctx, int comp, size_t lo, size_t c, uint64_t n, const uint64_t *src_d) const {
    return dev ? zk_copy_d2d(ctx, p[comp] + lo * n, src_d, c * n * 8) : zkfhe_download(ctx, p[comp] + lo * n, src_d, c * n * 8);
  }
  // the end of a call that wrote these planes: device planes are complete when the call returns
  int done(zkfhe_ctx *ctx) const {
    if (dev) ZK_HIP(ctx, zk_wait(ctx));
    return ZKFHE_OK;
  }
};
inline Planes host_planes(const uint64_t *c0, const uint64_t *c1) { return Planes{{(uint64_t *)c0, (uint64_t *)c1}, false}; }
inline Planes device_planes(const uint64_t *c0, const uint64_t *c1) { return Planes{{(uint64_t *)c0, (uint64_t *)c1}, true}; }

// the key0 rows, then the key1 rows of one key (lw = l N words each) into dst_d ([2 l][N]): what k_rns_ntt transforms into the
// [2 l][5][N] that the key switch reads
inline int upload_key_pair(zkfhe_ctx *ctx, uint64_t *dst_d, const uint64_t *k0, const uint64_t *k1, size_t lw) {
  ZK_CK(zkfhe_upload(ctx, dst_d, k0, lw * 8));
  return zkfhe_upload(ctx, dst_d + lw, k1, lw * 8);
}

// Where the `count` key-switch keys of a call come from: host rows still to be staged (key k: k0 + k l N and k1 + k l N, checked by
// the caller), or keys of a key set, transformed and on the device already (hat_d[k]: [2 l][5][N]).  add() puts the staging
// buffers into the caller's arena only where there is something to stage; stage_keys fills them; hat(k) is key k either way.
// special: the special modulus P of a hybrid key set (zkfhe.h), whose key switch the runner's epilogue divides by P; 1: ordinary
// keys, which host rows always are.
struct KeySource {
  const uint64_t *k0 = nullptr, *k1 = nullptr;
  const uint32_t *const *hat_d = nullptr;
  size_t count = 1;
  uint64_t special = 1;
  bool resident() const { return hat_d != nullptr; }
  void add(Arena &a, uint64_t n, int l) {
    words_ = (size_t)2 * l * n;
    if (!resident()) a.add(key_d_, count * words_).add(key_hat_, count * words_ * NP_MAX);
  }
  const uint32_t *hat(size_t k) const { return resident() ? hat_d[k] : key_hat_ + k * words_ * NP_MAX; }

  size_t words_ = 0;   // of one key before its transform
  uint64_t *key_d_ = nullptr;
  uint32_t *key_hat_ = nullptr;
};
inline KeySource host_keys(const uint64_t *k0, const uint64_t *k1, size_t count = 1) { return KeySource{k0, k1, nullptr, count}; }
inline KeySource resident_keys(const uint32_t *const *hat_d, size_t count = 1, uint64_t special = 1) {
  return KeySource{nullptr, nullptr, hat_d, count, special};
}

// The staging of host keys, once per call: every key's pair uploaded, one k_rns_ntt (LOAD_RESIDUE, five primes) over all of them.
// A resident key stages nothing and launches nothing.  A template for the sake of its kernel, which each unit launches as its own.
template <int NP>
int stage_keys(zkfhe_ctx *ctx, const KeySource &key, uint64_t n, uint64_t q, int l, int *flag) {
  if (key.resident()) return ZKFHE_OK;
  const size_t lw = (size_t)l * n;
  for (size_t k = 0; k < key.count; ++k) ZK_CK(upload_key_pair(ctx, key.key_d_ + k * 2 * lw, key.k0 + k * lw, key.k1 + k * lw, lw));
  return launch_rns_ntt<NP>(ctx, false, key.key_d_, LOAD_RESIDUE, q, 2 * key.count * l, bit_log2(n), nullptr, 0, key.key_hat_, flag);
}

// ---- defined in bfv_key_switch.hip
// the largest count of polynomials whose key switch goes the digit-parallel way on this device (0: never)
size_t zk_bfv_wide_max(const zkfhe_ctx *ctx, uint64_t n, int l);
// The key switches of one call: l digits of w bits, and how many polynomials at once may go the digit-parallel way.  add() reserves
// the partials ([l][2][c][5][N]) in the caller's arena where some key switch of the call takes them: never with host rows; with a
// resident key where c_max, the most polynomials of one key switch, is at most zk_bfv_wide_max (then a shorter last chunk goes the
// same way), or, per_level, where zk_bfv_wide_max is not 0 (the key switches of a call differ in size: each decides for itself).
struct KeySwitch {
  int log_n, l, w;
  uint64_t q;
  uint32_t *part = nullptr;
  size_t wide_max = 0;
  void add(Arena &a, const zkfhe_ctx *ctx, const KeySource &key, size_t c_max, bool per_level = false);
};
// The key switch of the c polynomials of src (SrcPlain, SrcGalois or SrcPack of key_switch_src.hip.hpp) against key_hat
// ([2 l][5][N]) into acc ([2][c][5][N]).  Digit-parallel (k_key_switch_digit over c 5 l workgroups into ks.part, then
// k_key_switch_fold over 2 c 5) iff ks.part is set and c <= ks.wide_max, else k_key_switch over c 5 workgroups.  Profiling slots:
// k_key_switch ZKFHE_PROF_BFV_RELIN (SrcPlain) or ZKFHE_PROF_BFV_GALOIS (SrcGalois), k_key_switch_digit of both and every fold
// ZKFHE_PROF_BFV_KEY_SWITCH_WIDE; both kernels of SrcPack ZKFHE_PROF_BFV_PACK
template <class Src>
int zk_bfv_key_switch(zkfhe_ctx *ctx, const KeySwitch &ks, const Src &src, const uint32_t *key_hat, size_t c, uint32_t *acc);

// ---- defined in bfv_eval.hip
// out = a +/- b, coefficient-wise mod Q
int zk_bfv_add_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, const Planes &b, int subtract, const Planes &out);
// out = a + delta m (mul: a m mod (x^N + 1, Q)) with m_count = 1 plaintext for every ciphertext or one per ciphertext (m: a host array)
int zk_bfv_plain_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, bool mul, size_t count, const Planes &a, size_t m_count, const uint64_t *m,
                     const Planes &out);
// out = a b relinearized with the one key of `key` (l rows of digit width base_bits).  A resident key takes the digit-parallel key
// switch where the chunk is at most zk_bfv_wide_max; host rows never do
int zk_bfv_mul_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, const Planes &b, KeySource key, int l, int base_bits,
                   const Planes &out);
// ---- defined in bfv_galois.hip
// "fn: ..." unless g is odd and below 2N
int check_g(zkfhe_ctx *ctx, uint64_t n, uint64_t g, const char *fn);
// The Galois chain: `steps` key switches per chunk, step k by gs[k] with key k of `key`.  accumulate: x <- x + apply_galois(x, gs[k])
// (slot_sum); else steps = 1 and out = apply_galois(a, gs[0]).  The digit-parallel key switch as in zk_bfv_mul_run
int zk_bfv_galois_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, size_t steps, const uint64_t *gs, KeySource key,
                      int l, int base_bits, bool accumulate, const Planes &out);
// ---- defined in bfv_dot.hip
// The chunk loops of bfv_dot (plain: bfv_dot_plain, b.p[0] the plaintexts and no key) behind the checks: a ([n_groups n_terms][N]),
// b ([b_groups n_terms][N]) and out ([n_groups][N]) each host arrays or device planes; with a resident key a pass of at most
// zk_bfv_wide_max groups takes the digit-parallel key switch
struct DotIo {
  Planes a, b, out;
  KeySource key;
};
int zk_bfv_dot_core(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, bool plain, size_t n_groups, size_t n_terms, size_t b_groups, const DotIo &io,
                    int l, int base_bits);
// "fn: n_terms ... is above the limit ..." unless n_terms is at most zkfhe_bfv_dot_max_terms
int check_dot_terms(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, bool plain, size_t n_terms, const char *fn);
// ---- defined in bfv_evk.hip
// a key set as its callers see it: the transformed relinearization key (null: none) and the transformed key of g (null: none);
// special: the special modulus of a hybrid set, 1 for an ordinary one
struct EvkView {
  zkfhe_bfv_params params;
  int device, base_bits, l;
  const uint32_t *rlk_hat;
  uint64_t special;
};
void zk_bfv_evk_view(const zkfhe_bfv_evk *evk, EvkView *view);
const uint32_t *zk_bfv_evk_galois(const zkfhe_bfv_evk *evk, uint64_t g);
// the largest P below 2^63 with l N (2^w - 1) (Q P - 1) <= floor(P5 / 2) (zkfhe_bfv_hybrid_max_p)
uint64_t hybrid_max_p(const zkfhe_bfv_params *prm, int l, int base_bits);
// the refusals of a special modulus in their order: "fn: P must satisfy 2 <= P < 2^63", "fn: P and Q must be coprime", "fn: P is
// above the limit ..." (hybrid_max_p)
int check_special(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, int l, int base_bits, uint64_t p, const char *fn);
// ---- defined in bfv_pack.hip
// out = x^k a mod (x^N + 1, Q) with k_count = 1 exponent for every ciphertext or one per ciphertext (k: a host array, every k < 2N)
int zk_bfv_monomial_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, size_t k_count, const uint64_t *k,
                        const Planes &out);
// Ring packing (zkfhe.h "Ring packing"): a holds n_groups n ciphertexts in [group][input] order, pos (a host array, [n_groups][n],
// or null: all 0) the coefficient of each that is kept, `key` the log2(N) keys of the pack elements in order; out takes n_groups
// ciphertexts.  A level's key switch goes the digit-parallel way where the key is resident and the level has at most
// zk_bfv_wide_max pairs
int zk_bfv_pack_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t n_groups, size_t n, const Planes &a, const uint64_t *pos, KeySource key,
                    int l, int base_bits, const Planes &out);
// the log2(N) pack elements 2^l + 1, l = 1 ... log2(N)
void pack_elements(uint64_t n, uint64_t *g);
// the refusals of a pack in their order: "fn: Q must be odd", base_bits outside [1, 32] (base_bits set: relin_rows into *l), "fn: n =
// ... is above N", "fn: a position is not below N" (pos: [n_groups][n] or null)
int check_pack(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, const int *base_bits, int *l, size_t n_groups, size_t n, const uint64_t *pos,
               const char *fn);
// "fn: ..." unless k_count is 1 or count and every k is below 2N
int check_monomial(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, size_t k_count, const uint64_t *k, const char *fn);
// ---- defined in bfv_linear.hip
// the parameters and the device of a plan
void zk_bfv_plan_view(const zkfhe_bfv_plan *plan, zkfhe_bfv_params *params, int *device);
// the run half of zkfhe_bfv_plan_apply on device arrays: c0, c1, out0, out1 are [n_cts][N] each on the plan's device.  A chunk is
// copied into the work arena before its kernels run and its result copied out after them, so out may be c0, c1
int zk_bfv_plan_run_dev(zkfhe_ctx *ctx, const zkfhe_bfv_plan *plan, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                        uint64_t *out1);
// ---- defined in bfv_ballot.hip
// the box's refusals (another device, a box closed by an interrupted add), then its parameters, its groups, its accumulator
// ([n_groups][2][N]) and its counts ([n_groups]) on the device
int zk_bfv_box_view(zkfhe_ctx *ctx, const zkfhe_bfv_box *box, zkfhe_bfv_params *params, size_t *n_groups, const uint64_t **acc,
                    const unsigned long long **counts);

}  // namespace zkrns
