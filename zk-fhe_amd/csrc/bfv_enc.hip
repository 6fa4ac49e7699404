// BFV key generation, encryption and decryption on the GPU: the step that produces what zkfhe_bfv_prove proves (the ciphertext
// and its witness u, e0, e1), for the scheme of the reference's input generator (README.md:25; zk-fhe_amd/inputs.py):
//     sk s ternary, pk = (-(a s + e), a);   c0 = pk0 u + floor(Q/T) m + e0,  c1 = pk1 u + e1   in Z_Q[x]/(x^N + 1).
//
// Every product has a ternary factor, so the centred integer product c of a (coefficients below 2^64) and s in {-1, 0, 1}^N has
// |c| < N 2^64 <= 2^79.  Three NTT primes below 2^31 (product 2^89.2 > 2 |c|) carry it exactly: per (polynomial, prime) one
// workgroup runs the whole negacyclic transform in LDS (k_rns_ntt of rns_ntt.hip.hpp: N <= 2^15 words = 128 KiB), the shared
// operand of a batch (pk0, pk1, a, or sk) is transformed once, and one fused epilogue (k_rns_epilogue) rebuilds c by Garner's CRT,
// reduces it mod Q, adds delta m + e (or rounds to T for decryption) and writes each output coefficient once.  Q itself need not
// be NTT-friendly.
//
// Randomness (zkfhe.h): ChaCha20 keyed by the caller's 32-byte seed, state words 12..15 = {block, domain, index_lo, index_hi},
// word w of a stream = the w-th little-endian u64 of its keystream, array position p reads word p (uniform: words 2p, 2p + 1).
// The samplers are branch-free and address nothing by a secret value (k_bfv_sample).
#include <cmath>
#include <mutex>

#include "rns_ntt.hip.hpp"

using namespace zkrns;

namespace {

constexpr int NP = 3;   // the first three primes of rns_ntt.hip.hpp: product 2^89.2
constexpr int MAX_CDT = 2046;   // 2 B thresholds, B < 1024
enum EpiMode { EPI_PLAIN = 0, EPI_ADD = 1, EPI_NEG_ADD = 2, EPI_DECRYPT = 3 };
struct Epi {
  int mode;
  const uint64_t *m;    // EPI_ADD: delta m (may be null)
  const uint64_t *e;    // EPI_ADD / EPI_NEG_ADD: + e
  const uint64_t *c0;   // EPI_DECRYPT: + c0 before rounding
  uint64_t delta, t;
};

struct ChaKey {
  uint32_t k[8];
};

// One thread per output coefficient: CRT of the three residues to the centred integer, mod Q, then the mode's additions; writes
// out[poly][N-1-d] (CircuitInput order).  m, e, c0 are read at the same position.
__global__ __launch_bounds__(256) void k_rns_epilogue(const uint32_t *__restrict__ res, size_t total, int log_n, uint64_t q, CrtConst cc,
                                                      Epi epi, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t n = (size_t)1 << log_n, poly = g >> log_n, d = g & (n - 1), pos = poly * n + (n - 1 - d);
  uint64_t v = crt3_mod_q(res + poly * NP * n + d, n, q, cc);   // c mod Q
  if (epi.mode == EPI_ADD) {
    if (epi.m) {   // m in [0, T/2] or [Q - T/2, Q): delta |m| <= Q / 2, no reduction needed
      const uint64_t mv = epi.m[pos];
      const bool mneg = mv > q / 2;
      const uint64_t dm = epi.delta * (mneg ? q - mv : mv);
      v = add_q(v, mneg && dm ? q - dm : dm, q);
    }
    v = add_q(v, epi.e[pos], q);
  } else if (epi.mode == EPI_NEG_ADD) {
    v = add_q(v, epi.e[pos], q);
    v = v ? q - v : 0;
  } else if (epi.mode == EPI_DECRYPT) {
    v = decrypt_round(add_q(v, epi.c0[pos], q), q, epi.t);   // round(T x / Q) mod T, x = [c0 + c1 s]_Q centred
  }
  out[pos] = v;
}

__device__ __forceinline__ uint32_t rotl32(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }
__device__ __forceinline__ void chacha20(const ChaKey &key, uint32_t w12, uint32_t w13, uint32_t w14, uint32_t w15, uint32_t o[16]) {
  uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                    key.k[4],    key.k[5],    key.k[6],    key.k[7],    w12,      w13,      w14,      w15};
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = s[i];
#define ZK_QR(a, b, c, d)                                    \
  o[a] += o[b], o[d] = rotl32(o[d] ^ o[a], 16);              \
  o[c] += o[d], o[b] = rotl32(o[b] ^ o[c], 12);              \
  o[a] += o[b], o[d] = rotl32(o[d] ^ o[a], 8);               \
  o[c] += o[d], o[b] = rotl32(o[b] ^ o[c], 7);
#pragma unroll 1
  for (int r = 0; r < 10; ++r) {
    ZK_QR(0, 4, 8, 12) ZK_QR(1, 5, 9, 13) ZK_QR(2, 6, 10, 14) ZK_QR(3, 7, 11, 15)
    ZK_QR(0, 5, 10, 15) ZK_QR(1, 6, 11, 12) ZK_QR(2, 7, 8, 13) ZK_QR(3, 4, 9, 14)
  }
#undef ZK_QR
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] += s[i];
}

enum SampleKind { S_TERNARY = 0, S_UNIFORM = 1, S_ERROR = 2 };

// One thread per ChaCha20 block of one polynomial (8 words: 8 ternary / error samples, or 4 uniform ones).  Polynomial j of the
// launch uses index0 + j.  Branch-free samplers: ternary ((w * 3) >> 64) - 1; uniform (x * Q) >> 128 of x = w[2p] + 2^64 w[2p+1];
// error -B + #{i : w >= T_i} over every threshold of the table (in LDS: every lane reads the same address).
__global__ __launch_bounds__(256) void k_bfv_sample(ChaKey key, uint32_t domain, uint64_t index0, int kind, size_t n_polys, int log_n,
                                                    uint64_t q, const uint64_t *__restrict__ cdt, int n_cdt, uint64_t *__restrict__ out) {
  __shared__ uint64_t tab[MAX_CDT];
  if (kind == S_ERROR) {
    for (int i = threadIdx.x; i < n_cdt; i += blockDim.x) tab[i] = cdt[i];
    __syncthreads();
  }
  const size_t n = (size_t)1 << log_n, per_poly = kind == S_UNIFORM ? n / 4 : n / 8;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_polys * per_poly) return;
  const size_t poly = g / per_poly, blk = g % per_poly;
  const uint64_t index = index0 + poly;
  uint32_t o[16];
  chacha20(key, (uint32_t)blk, domain, (uint32_t)index, (uint32_t)(index >> 32), o);
  uint64_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = (uint64_t)o[2 * i] | (uint64_t)o[2 * i + 1] << 32;
  uint64_t *dst = out + poly * n;
  if (kind == S_TERNARY) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t t = __umul64hi(w[i], 3);   // 0, 1, 2
      const uint64_t r = t + q - 1;
      dst[blk * 8 + i] = r >= q ? r - q : r;
    }
  } else if (kind == S_UNIFORM) {
    typedef unsigned __int128 u128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u128 acc = (u128)w[2 * i + 1] * q + __umul64hi(w[2 * i], q);
      dst[blk * 4 + i] = (uint64_t)(acc >> 64);
    }
  } else {
    const int64_t b = n_cdt / 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int64_t c = 0;
      for (int k = 0; k < n_cdt; ++k) c += w[i] >= tab[k];
      const int64_t x = c - b;
      dst[blk * 8 + i] = x < 0 ? q - (uint64_t)(-x) : (uint64_t)x;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host side

int work_arena(zkfhe_ctx *ctx, size_t bytes, char **out) {
  if (ctx->bfv_work_sz < bytes) {
    if (ctx->bfv_work) {
      ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
      ZK_HIP(ctx, hipFree(ctx->bfv_work));
      ctx->bfv_work = nullptr;
      ctx->bfv_work_sz = 0;
    }
    ZK_HIP(ctx, hipMalloc(&ctx->bfv_work, bytes));
    ctx->bfv_work_sz = bytes;
  }
  *out = (char *)ctx->bfv_work;
  return ZKFHE_OK;
}

int launch_ntt(zkfhe_ctx *ctx, bool mul, const uint64_t *src, bool ternary, uint64_t q, size_t n_polys, int log_n, const uint32_t *hat,
               size_t hat_stride, uint32_t *out, int *flag) {
  return launch_rns_ntt<NP>(ctx, mul, src, ternary ? LOAD_TERNARY : LOAD_RESIDUE, q, n_polys, log_n, hat, hat_stride, out, flag);
}

int launch_epilogue(zkfhe_ctx *ctx, const uint32_t *res, size_t n_polys, int log_n, uint64_t q, const Epi &epi, uint64_t *out) {
  const size_t total = n_polys << log_n;
  zk_prof_begin(ctx);
  k_rns_epilogue<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(res, total, log_n, q, crt3_const(), epi, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_RNS_EPILOGUE, (double)total * (12 + 8 + (epi.m ? 8 : 0) + (epi.e || epi.c0 ? 8 : 0)));
  return ZKFHE_OK;
}

int launch_sample(zkfhe_ctx *ctx, const ChaKey &key, uint32_t domain, uint64_t index0, int kind, size_t n_polys, int log_n, uint64_t q,
                  const uint64_t *cdt_dev, int n_cdt, uint64_t *out) {
  const size_t n = (size_t)1 << log_n, threads = n_polys * (kind == S_UNIFORM ? n / 4 : n / 8);
  zk_prof_begin(ctx);
  k_bfv_sample<<<zk_blocks(threads, 256), 256, 0, ctx->stream>>>(key, domain, index0, kind, n_polys, log_n, q, cdt_dev, n_cdt, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_SAMPLE, (double)n_polys * n * 8);
  return ZKFHE_OK;
}

bool ring_ok(uint64_t n, uint64_t q) { return n >= 8 && n <= NMAX && !(n & (n - 1)) && q >= 2 && !(q >> 63); }

int check_params(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm) {
  if (!prm) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv params: NULL");
  if (prm->n < 8 || prm->n > NMAX || (prm->n & (prm->n - 1)))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv params: N must be a power of two with 8 <= N <= 32768");
  if (prm->q < 2 || (prm->q >> 63)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv params: Q must satisfy 2 <= Q < 2^63");
  if (prm->t < 2 || prm->t >= prm->q) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv params: T must satisfy 2 <= T < Q");
  if (prm->b < 1 || prm->b >= prm->q || prm->b >= 1024) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv params: B must satisfy 1 <= B < min(Q, 1024)");
  return ZKFHE_OK;
}

// the thresholds T_i = round(2^64 P(X <= -B + i)), i < 2 B, of the discrete Gaussian (sigma 3.2) restricted to [-B, B]
void error_cdt(uint64_t b, uint64_t *t) {
  const long double two_s2 = 2.0L * 3.2L * 3.2L;
  std::vector<long double> w(2 * b + 1);
  long double z = 0;
  for (uint64_t i = 0; i <= 2 * b; ++i) {
    const long double x = (long double)((int64_t)i - (int64_t)b);
    w[i] = expl(-x * x / two_s2);
    z += w[i];
  }
  long double acc = 0;
  for (uint64_t i = 0; i < 2 * b; ++i) {
    acc += w[i];
    const long double v = floorl(ldexpl(acc / z, 64) + 0.5L);
    t[i] = v >= 18446744073709551616.0L ? ~(uint64_t)0 : (uint64_t)v;   // 2^64 itself: the top threshold 2^64 - 1 (2^-64 off)
  }
}

ChaKey cha_key(const uint8_t seed[32]) {
  ChaKey k;
  for (int i = 0; i < 8; ++i)
    k.k[i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 | (uint32_t)seed[4 * i + 3] << 24;
  return k;
}

}  // namespace

// [prime][fwd | inv][NMAX] for all NP_MAX primes (the three-prime kernels read the first three): psi^br15(k) and psi^-br15(k) in
// Montgomery form, psi of order 2 NMAX.  The first N entries are the tables of every N <= NMAX (bit reversal in 15 bits of k < N =
// bit reversal in log N bits times NMAX / N).
int zk_rns_tables(zkfhe_ctx *ctx, const uint32_t **out) {
  if (!ctx->bfv_tw) {
    std::vector<uint32_t> h((size_t)NP_MAX * 2 * NMAX);
    for (int j = 0; j < NP_MAX; ++j) {
      const uint64_t p = PRIMES[j];
      uint64_t psi = 0;
      for (uint64_t g = 2; !psi; ++g) {
        const uint64_t c = pow_mod(g, (p - 1) / (2 * NMAX), p);
        if (pow_mod(c, NMAX, p) == p - 1) psi = c;
      }
      const uint64_t psi_inv = pow_mod(psi, p - 2, p), R = ((uint64_t)1 << 32) % p;
      uint64_t f = 1, b = 1;
      std::vector<uint64_t> pf(NMAX), pb(NMAX);
      for (size_t e = 0; e < NMAX; ++e) pf[e] = f, pb[e] = b, f = f * psi % p, b = b * psi_inv % p;
      for (size_t k = 0; k < NMAX; ++k) {
        size_t r = 0;
        for (int i = 0; i < LOG_NMAX; ++i) r |= ((k >> i) & 1) << (LOG_NMAX - 1 - i);
        h[(size_t)j * 2 * NMAX + k] = (uint32_t)(pf[r] * R % p);
        h[(size_t)j * 2 * NMAX + NMAX + k] = (uint32_t)(pb[r] * R % p);
      }
    }
    void *d;
    ZK_HIP(ctx, hipMalloc(&d, h.size() * 4));
    ZK_HIP(ctx, hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    ctx->bfv_tw = (uint32_t *)d;
  }
  *out = ctx->bfv_tw;
  return ZKFHE_OK;
}

int zk_bfv_check_params(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm) { return check_params(ctx, prm); }
int zk_bfv_work_arena(zkfhe_ctx *ctx, size_t bytes, char **out) { return work_arena(ctx, bytes, out); }
void zk_bfv_error_cdt(uint64_t b, uint64_t *t) { error_cdt(b, t); }
int zk_bfv_sample(zkfhe_ctx *ctx, const uint8_t seed[32], uint32_t domain, uint64_t index0, int kind, size_t n_polys, int log_n, uint64_t q,
                  const uint64_t *cdt_dev, int n_cdt, uint64_t *out) {
  return launch_sample(ctx, cha_key(seed), domain, index0, kind, n_polys, log_n, q, cdt_dev, n_cdt, out);
}

extern "C" {

int zkfhe_poly_mul_ternary_negacyclic(zkfhe_ctx *ctx, const uint64_t *a_dev, size_t a_count, const uint64_t *s_dev, size_t n_polys,
                                      uint64_t n, uint64_t q, uint64_t *out_dev, int *not_ternary) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && a_dev && s_dev && out_dev && not_ternary && n_polys > 0 && (a_count == 1 || a_count == n_polys));
  if (!ring_ok(n, q)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "poly_mul_ternary: N must be a power of two in [8, 32768] and 2 <= Q < 2^63");
  *not_ternary = 0;
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_polys, chunk_polys(n)), plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(work_arena(ctx, 256 + align256(chunk * plane) * 2, &w));
  int *flag = (int *)w;
  uint32_t *hat = (uint32_t *)(w + 256), *res = (uint32_t *)(w + 256 + align256(chunk * plane));
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  const bool shared = a_count == 1;
  if (shared) ZK_CK(launch_ntt(ctx, false, a_dev, false, q, 1, log_n, nullptr, 0, hat, flag));
  Epi epi{EPI_PLAIN, nullptr, nullptr, nullptr, 0, 0};
  for (size_t lo = 0; lo < n_polys; lo += chunk) {
    const size_t c = std::min(chunk, n_polys - lo);
    if (!shared) ZK_CK(launch_ntt(ctx, false, a_dev + lo * n, false, q, c, log_n, nullptr, 0, hat, flag));
    ZK_CK(launch_ntt(ctx, true, s_dev + lo * n, true, q, c, log_n, hat, shared ? 0 : (size_t)NP * n, res, flag));
    ZK_CK(launch_epilogue(ctx, res, c, log_n, q, epi, out_dev + lo * n));
  }
  int bad = 0;
  ZK_CK(zkfhe_download(ctx, &bad, flag, 4));
  if (bad) {
    *not_ternary = 1;
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "poly_mul_ternary: an s coefficient is not in {0, 1, Q - 1}");
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_error_cdt(const zkfhe_bfv_params *params, uint64_t *thresholds, size_t *count) {
  if (!count) return ZKFHE_EINVAL;
  if (int rc = check_params(nullptr, params)) return rc;
  *count = 2 * params->b;
  if (thresholds) error_cdt(params->b, thresholds);
  return ZKFHE_OK;
}

int zkfhe_bfv_fhe_keypair(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint8_t seed[32], uint64_t *sk_out, uint64_t *pk0_out,
                          uint64_t *pk1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && seed && sk_out && pk0_out && pk1_out);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  error_cdt(params->b, cdt.data());
  const size_t vec = align256(n * 8);
  char *w;
  ZK_CK(work_arena(ctx, 256 + 4 * vec + align256(n_cdt * 8) + 2 * align256((size_t)NP * n * 4), &w));
  int *flag = (int *)w;
  uint64_t *s = (uint64_t *)(w + 256), *a = (uint64_t *)((char *)s + vec), *e = (uint64_t *)((char *)a + vec), *pk0 = (uint64_t *)((char *)e + vec);
  uint64_t *cdt_dev = (uint64_t *)((char *)pk0 + vec);
  uint32_t *hat = (uint32_t *)((char *)cdt_dev + align256(n_cdt * 8)), *res = (uint32_t *)((char *)hat + align256((size_t)NP * n * 4));
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, cdt_dev, cdt.data(), n_cdt * 8));
  const ChaKey key = cha_key(seed);
  ZK_CK(launch_sample(ctx, key, 4, 0, S_TERNARY, 1, log_n, q, nullptr, 0, s));
  ZK_CK(launch_sample(ctx, key, 5, 0, S_UNIFORM, 1, log_n, q, nullptr, 0, a));
  ZK_CK(launch_sample(ctx, key, 6, 0, S_ERROR, 1, log_n, q, cdt_dev, n_cdt, e));
  ZK_CK(launch_ntt(ctx, false, a, false, q, 1, log_n, nullptr, 0, hat, flag));
  ZK_CK(launch_ntt(ctx, true, s, true, q, 1, log_n, hat, 0, res, flag));
  Epi epi{EPI_NEG_ADD, nullptr, e, nullptr, 0, 0};
  ZK_CK(launch_epilogue(ctx, res, 1, log_n, q, epi, pk0));
  ZK_CK(zkfhe_download(ctx, sk_out, s, n * 8));
  ZK_CK(zkfhe_download(ctx, pk1_out, a, n * 8));
  ZK_CK(zkfhe_download(ctx, pk0_out, pk0, n * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_encrypt(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *pk0, const uint64_t *pk1, size_t n_msgs, const uint64_t *m,
                      const uint8_t seed[32], uint64_t first_index, uint64_t *u_out, uint64_t *e0_out, uint64_t *e1_out, uint64_t *c0_out,
                      uint64_t *c1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && pk0 && pk1 && m && seed && u_out && e0_out && e1_out && c0_out && c1_out && n_msgs > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q, t = params->t;
  for (uint64_t i = 0; i < n; ++i)
    if (pk0[i] >= q || pk1[i] >= q) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_encrypt: a public-key coefficient is not below Q");
  for (size_t i = 0; i < n_msgs * n; ++i)
    if (m[i] > t / 2 && (m[i] >= q || m[i] < q - t / 2))
      return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_encrypt: a message coefficient is outside [0, T/2] and [Q - T/2, Q - 1]");
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  error_cdt(params->b, cdt.data());
  const size_t chunk = std::min<size_t>(n_msgs, chunk_polys(n)), vec = align256(n * 8), cvec = align256(chunk * n * 8), plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(work_arena(ctx, 256 + 2 * vec + align256(n_cdt * 8) + 2 * align256(plane) + 6 * cvec + align256(chunk * plane), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *pk0_d = (uint64_t *)take(vec), *pk1_d = (uint64_t *)take(vec), *cdt_dev = (uint64_t *)take(align256(n_cdt * 8));
  uint32_t *hat0 = (uint32_t *)take(align256(plane)), *hat1 = (uint32_t *)take(align256(plane));
  uint64_t *m_d = (uint64_t *)take(cvec), *u_d = (uint64_t *)take(cvec), *e0_d = (uint64_t *)take(cvec), *e1_d = (uint64_t *)take(cvec);
  uint64_t *c0_d = (uint64_t *)take(cvec), *c1_d = (uint64_t *)take(cvec);
  uint32_t *res = (uint32_t *)take(align256(chunk * plane));
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, cdt_dev, cdt.data(), n_cdt * 8));
  ZK_CK(zkfhe_upload(ctx, pk0_d, pk0, n * 8));
  ZK_CK(zkfhe_upload(ctx, pk1_d, pk1, n * 8));
  ZK_CK(launch_ntt(ctx, false, pk0_d, false, q, 1, log_n, nullptr, 0, hat0, flag));
  ZK_CK(launch_ntt(ctx, false, pk1_d, false, q, 1, log_n, nullptr, 0, hat1, flag));
  const ChaKey key = cha_key(seed);
  const uint64_t delta = q / t;
  for (size_t lo = 0; lo < n_msgs; lo += chunk) {
    const size_t c = std::min(chunk, n_msgs - lo), bytes = c * n * 8;
    const uint64_t index0 = first_index + lo;
    ZK_CK(zkfhe_upload(ctx, m_d, m + lo * n, bytes));
    ZK_CK(launch_sample(ctx, key, 1, index0, S_TERNARY, c, log_n, q, nullptr, 0, u_d));
    ZK_CK(launch_sample(ctx, key, 2, index0, S_ERROR, c, log_n, q, cdt_dev, n_cdt, e0_d));
    ZK_CK(launch_sample(ctx, key, 3, index0, S_ERROR, c, log_n, q, cdt_dev, n_cdt, e1_d));
    ZK_CK(launch_ntt(ctx, true, u_d, true, q, c, log_n, hat0, 0, res, flag));
    ZK_CK(launch_epilogue(ctx, res, c, log_n, q, Epi{EPI_ADD, m_d, e0_d, nullptr, delta, t}, c0_d));
    ZK_CK(launch_ntt(ctx, true, u_d, true, q, c, log_n, hat1, 0, res, flag));
    ZK_CK(launch_epilogue(ctx, res, c, log_n, q, Epi{EPI_ADD, nullptr, e1_d, nullptr, delta, t}, c1_d));
    ZK_CK(zkfhe_download(ctx, u_out + lo * n, u_d, bytes));
    ZK_CK(zkfhe_download(ctx, e0_out + lo * n, e0_d, bytes));
    ZK_CK(zkfhe_download(ctx, e1_out + lo * n, e1_d, bytes));
    ZK_CK(zkfhe_download(ctx, c0_out + lo * n, c0_d, bytes));
    ZK_CK(zkfhe_download(ctx, c1_out + lo * n, c1_d, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_decrypt(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, size_t n_msgs, const uint64_t *c0, const uint64_t *c1,
                      uint64_t *m_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && c0 && c1 && m_out && n_msgs > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  for (size_t i = 0; i < n_msgs * n; ++i)
    if (c0[i] >= q || c1[i] >= q) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_decrypt: a ciphertext coefficient is not below Q");
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_msgs, chunk_polys(n)), vec = align256(n * 8), cvec = align256(chunk * n * 8), plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(work_arena(ctx, 256 + vec + align256(plane) + 3 * cvec + align256(chunk * plane), &w));
  int *flag = (int *)w;
  uint64_t *sk_d = (uint64_t *)(w + 256);
  uint32_t *hat = (uint32_t *)((char *)sk_d + vec);
  uint64_t *c0_d = (uint64_t *)((char *)hat + align256(plane)), *c1_d = (uint64_t *)((char *)c0_d + cvec), *m_d = (uint64_t *)((char *)c1_d + cvec);
  uint32_t *res = (uint32_t *)((char *)m_d + cvec);
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, sk_d, sk, n * 8));
  ZK_CK(launch_ntt(ctx, false, sk_d, true, q, 1, log_n, nullptr, 0, hat, flag));
  int bad = 0;
  ZK_CK(zkfhe_download(ctx, &bad, flag, 4));
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_decrypt: a secret-key coefficient is not in {0, 1, Q - 1}");
  for (size_t lo = 0; lo < n_msgs; lo += chunk) {
    const size_t c = std::min(chunk, n_msgs - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, c0_d, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, c1_d, c1 + lo * n, bytes));
    ZK_CK(launch_ntt(ctx, true, c1_d, false, q, c, log_n, hat, 0, res, flag));
    ZK_CK(launch_epilogue(ctx, res, c, log_n, q, Epi{EPI_DECRYPT, nullptr, nullptr, c0_d, 0, params->t}, m_d));
    ZK_CK(zkfhe_download(ctx, m_out + lo * n, m_d, bytes));
  }
  return ZKFHE_OK;
}

}  // extern "C"
