// The exact negacyclic product behind the BFV kernels (bfv_enc.hip, bfv_eval.hip, bfv_threshold.hip, bfv_refresh.hip, bfv_galois.hip): an RNS NTT
// over NP primes below 2^31, one workgroup per (polynomial, prime), the whole transform of N <= 2^15 words in LDS (128 KiB at
// N = 2^15), with 32-bit Montgomery arithmetic.  Templated on the prime count: encryption and the threshold calls use the first
// three primes (product 2^89.2: a ternary factor keeps the product below N 2^64), the evaluator all five (product 2^151.2: a
// product of two centred residues below 2^63 stays below 2^140).
// Headroom at p < 2^31: a b + m p < 2^62 + 2^63 < 2^64 in mont_mul, and a + b < 2^32 in add_p.
// Also the device helpers every BFV file shares, the constants and modes of the two CRT epilogues, and the launch of k_rns_ntt.  The
// host vocabulary of the BFV units (work arena, operands, keys, what each unit defines for the others) is bfv_host.hpp.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "ctx.hpp"

namespace zkrns {

constexpr int NP_MAX = 5;
// 15 2^27 + 1, 7 2^26 + 1, 45 2^24 + 1, 32766 2^16 + 1, 32760 2^16 + 1: every one has 2^16 | p - 1 (order-2N roots up to N = 2^15)
constexpr uint32_t PRIMES[NP_MAX] = {2013265921u, 469762049u, 754974721u, 2147352577u, 2146959361u};
constexpr int LOG_NMAX = 15;
constexpr size_t NMAX = (size_t)1 << LOG_NMAX;
constexpr int NTT_THREADS = 1024;

// per-call constants of the primes: p, -p^-1 mod 2^32, and N^-1 R^2 mod p (R = 2^32: the inverse transform's scale, which also
// undoes the R^-1 of the Montgomery pointwise product)
template <int NP>
struct RnsConst {
  uint32_t p[NP], pinv[NP], scale[NP];
};

// how k_rns_ntt reads a coefficient v (below 2^64) of its source: as the integer v; as a ternary {0, 1, Q-1} -> {0, 1, -1} (anything
// else is flagged and read as 0); or centred, v - Q if v > floor(Q/2)
enum LoadMode { LOAD_RESIDUE = 0, LOAD_TERNARY = 1, LOAD_CENTRED = 2 };

// the samplers of k_bfv_sample (zk_bfv_sample)
enum SampleKind { S_TERNARY = 0, S_UNIFORM = 1, S_ERROR = 2 };

// the ChaCha20 domains of the BFV samplers, word 13 of the state (the table of zkfhe.h)
enum Domain : uint32_t {
  DOM_ENC_U = 1, DOM_ENC_E0 = 2, DOM_ENC_E1 = 3,   // encryption, index first_index + message
  DOM_KEY_S = 4, DOM_KEY_A = 5, DOM_KEY_E = 6,     // (shared) public key, index 0: s and e from the party seed, a from the CRS
  DOM_RLK_A = 7, DOM_RLK_E = 8,                    // relinearization key row i (a_i also the CRS of the threshold rows)
  DOM_SMUDGE = 9,                                  // decryption-share noise, index first_index + ciphertext
  DOM_THR_U = 10, DOM_THR_E0 = 11, DOM_THR_E1 = 12, DOM_THR_E2 = 13,   // threshold relinearization rounds, row j
  DOM_GK_A = 14, DOM_GK_E = 15,                    // Galois key row j, index g 64 + j
  DOM_PCKS_U = 16, DOM_PCKS_E0 = 17, DOM_PCKS_E1 = 18,   // public collective key switch, index first_index + ciphertext
  DOM_RFR_A = 19,                                        // refresh: CRS a_j, index first_index + ciphertext
  DOM_RFR_M = 20, DOM_RFR_E0 = 21, DOM_RFR_E1 = 22,      // refresh: mask M_ij (uniform mod T), e0_ij (smudging), e1_ij
  DOM_HYB_RLK_A = 23, DOM_HYB_GK_A = 24,                 // hybrid keys: the p-plane's a_i (uniform mod P), indices as domains 7 and 14
};

__device__ __forceinline__ uint32_t mont_mul(uint32_t a, uint32_t b, uint32_t p, uint32_t pinv) {
  const uint64_t x = (uint64_t)a * b;   // < p^2 < 2^62
  const uint32_t m = (uint32_t)x * pinv;
  const uint32_t r = (uint32_t)((x + (uint64_t)m * p) >> 32);   // < 2 p
  return r >= p ? r - p : r;
}
__device__ __forceinline__ uint32_t add_p(uint32_t a, uint32_t b, uint32_t p) {
  const uint32_t s = a + b;   // < 2^32: p < 2^31
  return s >= p ? s - p : s;
}
__device__ __forceinline__ uint32_t sub_p(uint32_t a, uint32_t b, uint32_t p) { return a >= b ? a - b : a + p - b; }

__device__ __forceinline__ uint64_t add_q(uint64_t a, uint64_t b, uint64_t q) {
  const uint64_t s = a + b;   // < 2^64: q < 2^63
  return s >= q ? s - q : s;
}
__device__ __forceinline__ uint64_t sub_q(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }

// v + delta m mod Q for a plaintext m in [0, T/2] or [Q - T/2, Q): delta |m| <= Q / 2, no reduction needed
__device__ __forceinline__ uint64_t add_delta_m(uint64_t v, uint64_t m, uint64_t delta, uint64_t q) {
  const bool mneg = m > q / 2;
  const uint64_t dm = delta * (mneg ? q - m : m);
  return add_q(v, mneg && dm ? q - dm : dm, q);
}

// the gadget term of a ternary s in {0, 1, Q - 1}: 0, pw or Q - pw without a branch (pw = 2^(j w) < Q)
__device__ __forceinline__ uint64_t gadget_select(uint64_t s, uint64_t pw, uint64_t q) { return s == 1 ? pw : (s == q - 1 ? q - pw : 0); }

// degree d of sigma_g(v), v one polynomial in CircuitInput order, ginv = g^-1 mod 2N (zkfhe.h): degree j = d ginv mod 2N of v if
// j < N, else minus degree j - N.  ginv = 1 reads v[N - 1 - d].
__device__ __forceinline__ uint64_t auto_coeff(const uint64_t *__restrict__ v, unsigned d, unsigned ginv, unsigned n, uint64_t q) {
  const unsigned j = (d * ginv) & (2 * n - 1);   // d ginv < 2^15 2^16
  const uint64_t x = v[n - 1 - (j & (n - 1))];
  return j >= n && x ? q - x : x;
}

// (hi 2^64 + lo) mod q, q < 2^63: bit by bit, no data-dependent branch
__device__ __forceinline__ uint64_t mod128(uint64_t hi, uint64_t lo, uint64_t q) {
  uint64_t r = hi % q;
#pragma unroll 8
  for (int i = 63; i >= 0; --i) {
    r = (r << 1) | ((lo >> i) & 1);   // < 2 q < 2^64
    r -= r >= q ? q : 0;
  }
  return r;
}
// floor((hi 2^64 + lo) / d) for a quotient below 2^64 (hi < d), any d < 2^64
__device__ __forceinline__ uint64_t div128(uint64_t hi, uint64_t lo, uint64_t d) {
  uint64_t r = hi, quo = 0;
#pragma unroll 8
  for (int i = 63; i >= 0; --i) {
    const uint64_t carry = r >> 63;
    r = (r << 1) | ((lo >> i) & 1);
    const bool take = carry || r >= d;
    r -= take ? d : 0;
    quo |= (uint64_t)take << i;
  }
  return quo;
}

// Garner over the first three primes (product 2^89.2): y1 = (r1 - r0) p0^-1 mod p1, y2 = (r2 - r0 - p0 y1) (p0 p1)^-1 mod p2,
// x = r0 + p0 y1 + p0 p1 y2
struct CrtConst {
  uint64_t inv01, inv012, p0_mod_p2, p01;
  uint64_t P_lo, P_hi;   // p0 p1 p2
};

// the centred integer of the three residues r[0], r[n], r[2 n], reduced mod q
__device__ __forceinline__ uint64_t crt3_mod_q(const uint32_t *__restrict__ r, size_t n, uint64_t q, const CrtConst &cc) {
  const uint64_t p0 = PRIMES[0], p1 = PRIMES[1], p2 = PRIMES[2];
  const uint64_t r0 = r[0], r1 = r[n], r2 = r[2 * n];
  const uint64_t y1 = (r1 + p1 - r0 % p1) % p1 * cc.inv01 % p1;
  const uint64_t x01 = (r0 % p2 + cc.p0_mod_p2 * y1) % p2;
  const uint64_t y2 = (r2 + p2 - x01) % p2 * cc.inv012 % p2;
  typedef unsigned __int128 u128;
  const u128 x = (u128)r0 + (u128)p0 * y1 + (u128)cc.p01 * y2;   // < P
  const u128 P = ((u128)cc.P_hi << 64) | cc.P_lo;
  const bool neg = x > (P >> 1);
  const u128 mag = neg ? P - x : x;
  const uint64_t rm = mod128((uint64_t)(mag >> 64), (uint64_t)mag, q);
  return neg && rm ? q - rm : rm;
}

// Garner over the five primes: y_k = (((r_k - y_0) p_0^-1 - y_1) p_1^-1 - ...) mod p_k, x = y_0 + p_0 (y_1 + p_1 (y_2 + ...))
struct Crt5 {
  uint32_t inv[NP_MAX][NP_MAX];   // inv[j][k] = p_j^-1 mod p_k for j < k
  uint64_t P[3], H[3];            // p_0 ... p_4 and floor of its half, little-endian limbs
};

// the centred integer of the residues r[k n], k < NP_MAX: magnitude m (three limbs) and sign
__device__ __forceinline__ void crt5(const uint32_t *__restrict__ r, size_t n, const Crt5 &cc, uint64_t m[3], bool &neg) {
  typedef unsigned __int128 u128;
  uint64_t y[NP_MAX];
#pragma unroll
  for (int k = 0; k < NP_MAX; ++k) {
    const uint64_t pk = PRIMES[k];
    uint64_t t = r[k * n];
#pragma unroll
    for (int j = 0; j < k; ++j) t = (t + pk - y[j] % pk) * cc.inv[j][k] % pk;   // < 2^32 * 2^31
    y[k] = t;
  }
  uint64_t x0 = y[NP_MAX - 1], x1 = 0, x2 = 0;
#pragma unroll
  for (int k = NP_MAX - 2; k >= 0; --k) {
    const u128 a = (u128)x0 * PRIMES[k] + y[k];
    const u128 b = (u128)x1 * PRIMES[k] + (uint64_t)(a >> 64);
    x0 = (uint64_t)a, x1 = (uint64_t)b, x2 = x2 * PRIMES[k] + (uint64_t)(b >> 64);
  }
  neg = x2 > cc.H[2] || (x2 == cc.H[2] && (x1 > cc.H[1] || (x1 == cc.H[1] && x0 > cc.H[0])));
  const uint64_t d0 = cc.P[0] - x0, b0 = cc.P[0] < x0;
  const uint64_t d1 = cc.P[1] - x1 - b0, b1 = cc.P[1] < x1 || (cc.P[1] - x1) < b0;
  const uint64_t d2 = cc.P[2] - x2 - b1;
  m[0] = neg ? d0 : x0, m[1] = neg ? d1 : x1, m[2] = neg ? d2 : x2;
}
// the integer of crt5 (magnitude m, sign neg) mod q
__device__ __forceinline__ uint64_t crt5_mod_q(const uint64_t m[3], bool neg, uint64_t q) {
  const uint64_t rm = mod128(mod128(m[2], m[1], q), m[0], q);
  return neg && rm ? q - rm : rm;
}
// floor((2 x + P) / 2P) mod q for the integer x of crt5 (|x| < 2^151) and 2 <= P < 2^63: x / P rounded to nearest, ties upward
// (the hybrid key switch, zkfhe.h).  For x < 0 that is -floor((2 |x| + P - 1) / 2P).  Long division by 2P, one limb at a time
// (the remainder carried in is below 2P, so div128's hi < d holds), as EV_ROUND divides by 2Q
__device__ __forceinline__ uint64_t crt5_div_p_mod_q(const uint64_t m[3], bool neg, uint64_t sp, uint64_t q) {
  typedef unsigned __int128 u128;
  const uint64_t dp = 2 * sp;
  u128 a = ((u128)m[0] << 1) + (neg ? sp - 1 : sp);
  const uint64_t n0 = (uint64_t)a;
  a = ((u128)m[1] << 1) + (uint64_t)(a >> 64);
  const uint64_t n1 = (uint64_t)a, n2 = (m[2] << 1) + (uint64_t)(a >> 64);   // m[2] < 2^23
  const uint64_t q2 = div128(0, n2, dp), r2 = n2 - q2 * dp;
  const uint64_t q1 = div128(r2, n1, dp), r1 = n1 - q1 * dp;
  const uint64_t q0 = div128(r1, n0, dp);
  const uint64_t r = mod128(mod128(q2, q1, q), q0, q);
  return neg && r ? q - r : r;
}

// the decryption of the residue v = [c0 + c1 s]_Q: round(T x / Q) mod T with x = v centred, as a residue mod Q.  For the residue v
// the quotient floor((2 T v + Q) / 2Q) differs by T at most, which the reduction mod T removes (inputs.decrypt)
__device__ __forceinline__ uint64_t decrypt_round(uint64_t v, uint64_t q, uint64_t t) {
  typedef unsigned __int128 u128;
  const u128 num = (u128)(2 * t) * v + q;   // 2 T < 2^64
  uint64_t m = div128((uint64_t)(num >> 64), (uint64_t)num, 2 * q);   // in [0, T]
  m = m == t ? 0 : m;
  return m > t / 2 ? q - (t - m) : m;
}

// v read in `mode` as a residue mod p; `bad` collects non-ternary coefficients of LOAD_TERNARY
__device__ __forceinline__ uint32_t rns_load(uint64_t v, int mode, uint64_t q, uint32_t p, bool &bad) {
  if (mode == LOAD_TERNARY) {
    const bool one = v == 1, minus = v == q - 1;
    bad |= !(one || minus || v == 0);
    return one ? 1u : (minus ? p - 1 : 0u);
  }
  if (mode == LOAD_CENTRED) {
    const bool neg = v > q / 2;
    const uint32_t r = (uint32_t)((neg ? q - v : v) % p);
    return neg && r ? p - r : r;
  }
  return (uint32_t)(v % p);
}

// merged-twist negacyclic forward transform of lds[0, n) in place (Cooley-Tukey, bit-reversed output); fw = psi^br(k) in Montgomery
// form.  Ends with a barrier.
__device__ __forceinline__ void rns_forward(uint32_t *lds, const uint32_t *__restrict__ fw, int log_n, uint32_t p, uint32_t pinv) {
  const unsigned half = (1u << log_n) >> 1, tid = threadIdx.x;
  for (int lm = 0; lm < log_n; ++lm) {   // m = 2^lm groups, t = n / 2m
    const int lt = log_n - 1 - lm;
    const unsigned t = 1u << lt;
    for (unsigned b = tid; b < half; b += NTT_THREADS) {
      const unsigned i = b >> lt, x = (i << (lt + 1)) + (b & (t - 1));
      const uint32_t w = fw[(1u << lm) + i];
      const uint32_t U = lds[x], V = mont_mul(lds[x + t], w, p, pinv);
      lds[x] = add_p(U, V, p);
      lds[x + t] = sub_p(U, V, p);
    }
    __syncthreads();
  }
}

// the inverse (Gentleman-Sande) of rns_forward without the final scale; iv = psi^-br(k) in Montgomery form.  Ends with a barrier.
__device__ __forceinline__ void rns_inverse(uint32_t *lds, const uint32_t *__restrict__ iv, int log_n, uint32_t p, uint32_t pinv) {
  const unsigned half = (1u << log_n) >> 1, tid = threadIdx.x;
  for (int lh = log_n - 1; lh >= 0; --lh) {   // h = 2^lh groups, t = n / 2h
    const int lt = log_n - 1 - lh;
    const unsigned t = 1u << lt;
    for (unsigned b = tid; b < half; b += NTT_THREADS) {
      const unsigned i = b >> lt, x = (i << (lt + 1)) + (b & (t - 1));
      const uint32_t w = iv[(1u << lh) + i];
      const uint32_t U = lds[x], V = lds[x + t];
      lds[x] = add_p(U, V, p);
      lds[x + t] = mont_mul(sub_p(U, V, p), w, p, pinv);
    }
    __syncthreads();
  }
}

// One workgroup per (polynomial, prime), blockIdx.x = poly * NP + prime.  Loads N coefficients (src is in CircuitInput order:
// position N-1-d holds degree d) into LDS in `mode` and runs the forward transform.  MUL = false: the transform is stored to `out`
// (hat[poly][prime][N]).  MUL = true: it is multiplied by hat + poly * hat_stride, transformed back, scaled, and the residues of the
// product are stored to out[poly][prime][degree].  tw: [prime][fwd | inv][NMAX] (zk_rns_tables).
template <int NP, bool MUL>
__global__ __launch_bounds__(NTT_THREADS) void k_rns_ntt(const uint64_t *__restrict__ src, int mode, uint64_t q, int log_n,
                                                          const uint32_t *__restrict__ tw, RnsConst<NP> rc, const uint32_t *__restrict__ hat,
                                                          size_t hat_stride, uint32_t *__restrict__ out, int *flag) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t poly = blockIdx.x / NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const uint64_t *s = src + poly * n;
  bool bad = false;
  for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = rns_load(s[n - 1 - d], mode, q, p, bad);
  if (bad) atomicOr(flag, 1);
  __syncthreads();
  const uint32_t *fw = tw + (size_t)j * 2 * NMAX, *iv = fw + NMAX;   // prefixes serve every N
  rns_forward(lds, fw, log_n, p, pinv);
  uint32_t *o = out + (poly * NP + j) * n;
  if (!MUL) {
    for (unsigned d = tid; d < n; d += NTT_THREADS) o[d] = lds[d];
    return;
  }
  const uint32_t *h = hat + poly * hat_stride + (size_t)j * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = mont_mul(lds[d], h[d], p, pinv);
  __syncthreads();
  rns_inverse(lds, iv, log_n, p, pinv);
  for (unsigned d = tid; d < n; d += NTT_THREADS) o[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
}

// ---------------------------------------------------------------------------------------------------------------- host side

inline uint64_t pow_mod(uint64_t a, uint64_t e, uint64_t p) {
  uint64_t r = 1;
  for (a %= p; e; e >>= 1, a = a * a % p)
    if (e & 1) r = r * a % p;
  return r;
}

inline int bit_log2(uint64_t n) {
  int l = 0;
  while (((uint64_t)1 << l) < n) ++l;
  return l;
}

template <int NP>
RnsConst<NP> rns_const(int log_n) {
  RnsConst<NP> c;
  for (int j = 0; j < NP; ++j) {
    const uint64_t p = PRIMES[j];
    uint32_t inv = 1;   // p^-1 mod 2^32 by Newton
    for (int i = 0; i < 5; ++i) inv *= 2 - (uint32_t)p * inv;
    c.p[j] = (uint32_t)p;
    c.pinv[j] = (uint32_t)(0u - inv);
    const uint64_t n_inv = pow_mod((uint64_t)1 << log_n, p - 2, p), R2 = pow_mod(2, 64, p);
    c.scale[j] = (uint32_t)(n_inv * R2 % p);
  }
  return c;
}

inline CrtConst crt3_const() {
  const uint64_t p0 = PRIMES[0], p1 = PRIMES[1], p2 = PRIMES[2];
  CrtConst c;
  c.inv01 = pow_mod(p0 % p1, p1 - 2, p1);
  c.p01 = p0 * p1;
  c.inv012 = pow_mod(c.p01 % p2, p2 - 2, p2);
  c.p0_mod_p2 = p0 % p2;
  const unsigned __int128 P = (unsigned __int128)c.p01 * p2;
  c.P_lo = (uint64_t)P, c.P_hi = (uint64_t)(P >> 64);
  return c;
}

inline Crt5 crt5_const() {
  typedef unsigned __int128 u128;
  Crt5 c{};
  for (int j = 0; j < NP_MAX; ++j)
    for (int k = j + 1; k < NP_MAX; ++k) c.inv[j][k] = (uint32_t)pow_mod(PRIMES[j] % PRIMES[k], PRIMES[k] - 2, PRIMES[k]);
  uint64_t P[3] = {1, 0, 0};
  for (int k = 0; k < NP_MAX; ++k) {
    u128 a = (u128)P[0] * PRIMES[k];
    P[0] = (uint64_t)a;
    a = (u128)P[1] * PRIMES[k] + (uint64_t)(a >> 64);
    P[1] = (uint64_t)a;
    P[2] = P[2] * PRIMES[k] + (uint64_t)(a >> 64);
  }
  for (int i = 0; i < 3; ++i) c.P[i] = P[i];
  c.H[0] = P[0] >> 1 | P[1] << 63, c.H[1] = P[1] >> 1 | P[2] << 63, c.H[2] = P[2] >> 1;
  return c;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// polynomials per chunk of a batch: 2^21 coefficients, at least 8 polynomials
inline size_t chunk_polys(uint64_t n) { return std::max<size_t>(8, ((size_t)1 << 21) / n); }
// polynomials per chunk when n_planes planes of the chunk are resident at once: the budget of chunk_polys per four planes
inline size_t plane_chunk(uint64_t n, size_t n_planes, size_t count) {
  return std::min(count, std::max<size_t>(1, chunk_polys(n) * 4 / n_planes));
}

// The modes of the three-prime CRT epilogue (k_rns_epilogue, bfv_enc.hip): x = the product mod Q, then
//   EPI_PLAIN    x
//   EPI_ADD      x [+ delta m] [+ a - b] [+ e]
//   EPI_NEG_ADD  -(x + e)
//   EPI_DECRYPT  decrypt_round(x + c0)
//   EPI_SHARE    x + r - E, r = e uniform in [0, 2E]
//   EPI_GADGET   -x + e + 2^(j w) sigma_g(s) for row j, or -x - e + ... with neg_e
//   EPI_MASK     x - delta M + e - E, or -x + delta M + e - E with neg_x; M = m in [0, T)   (the refresh shares)
//   EPI_SHARE_ADD  x + a + r - E, r = e uniform in [0, 2E]                                  (the key-switch share h0)
enum EpiMode { EPI_PLAIN = 0, EPI_ADD = 1, EPI_NEG_ADD = 2, EPI_DECRYPT = 3, EPI_SHARE = 4, EPI_GADGET = 5, EPI_MASK = 6, EPI_SHARE_ADD = 7 };
struct Epi {
  int mode = EPI_PLAIN;
  const uint64_t *m = nullptr;                 // EPI_ADD: + delta m (may be null); EPI_MASK: M
  const uint64_t *e = nullptr;                 // the error (EPI_ADD: may be null); EPI_SHARE, EPI_SHARE_ADD: r; EPI_MASK: e or r
  const uint64_t *c0 = nullptr;                // EPI_DECRYPT
  const uint64_t *a = nullptr, *b = nullptr;   // EPI_ADD: + a - b (both null or both set); EPI_SHARE_ADD: + a
  const uint64_t *s = nullptr;                 // EPI_GADGET: s, one polynomial
  uint64_t delta = 0, t = 0, bound = 0;        // EPI_ADD, EPI_MASK: delta; EPI_DECRYPT: T; EPI_SHARE, EPI_SHARE_ADD, EPI_MASK: E
  unsigned ginv = 1;                           // EPI_GADGET: g^-1 mod 2N
  int w = 0;                                   // EPI_GADGET: the digit width
  int neg_e = 0;                               // EPI_GADGET: - e
  int neg_x = 0;                               // EPI_MASK: -x + delta M
};

// The modes of the five-prime CRT epilogue (k_eval_epilogue, bfv_eval.hip) on the centred integer x:
//   EV_MODQ    x mod Q
//   EV_ROUND   floor((2 T x + Q) / 2Q) mod Q
//   EV_ADD     x + add mod Q
//   EV_RLK     2^(i w) s^2 - x - e mod Q for polynomial i
//   EV_NOISE   |[c0 + x - delta m]_Q| with m = the decryption of [c0 + x]_Q, maximised per polynomial
//   EV_GALOIS  x mod Q, + sigma_g(c0) on the first c polynomials, + add when set
// With a special modulus p != 1 (a hybrid key set: EV_ADD and EV_GALOIS only) floor((2 x + p) / 2p) mod Q stands where x mod Q does.
enum EvMode { EV_MODQ = 0, EV_ROUND = 1, EV_ADD = 2, EV_RLK = 3, EV_NOISE = 4, EV_GALOIS = 5 };
struct EvEpi {
  int mode = EV_MODQ;
  const uint64_t *add = nullptr;    // EV_ADD: + add[pos]; EV_RLK: - e[pos]; EV_NOISE: + c0[pos]; EV_GALOIS: + x_in[pos] (may be null)
  const uint64_t *poly = nullptr;   // EV_RLK: s^2, one polynomial; EV_GALOIS: the c0 of the c ciphertexts ([c][N])
  uint64_t t = 0, delta = 0;
  int w = 0;                             // EV_RLK: the digit width; polynomial i gets 2^(i w) s^2
  unsigned long long *noise = nullptr;   // EV_NOISE: the maximum per polynomial (zeroed before the launch)
  unsigned ginv = 1;                     // EV_GALOIS: g^-1 mod 2N
  size_t c = 0;                          // EV_GALOIS
  uint64_t p = 1;                        // EV_ADD, EV_GALOIS: the special modulus of a hybrid key set (1: none)
};

// ---- defined in bfv_enc.hip
// the twiddle tables of every prime: [prime][fwd | inv][NMAX], psi^br15(k) and psi^-br15(k) in Montgomery form (built on first use)
int zk_rns_tables(zkfhe_ctx *ctx, const uint32_t **out);

// the dynamic LDS of a kernel that holds N = 2^log_n words, opted in above 64 KiB
inline int ntt_lds(zkfhe_ctx *ctx, const void *kernel, int log_n, int *lds) {
  *lds = 4 << log_n;
  if (*lds > 64 * 1024) ZK_CK(zk_func_max_lds(ctx, kernel, 4 << LOG_NMAX));
  return ZKFHE_OK;
}

// k_rns_ntt over n_polys polynomials with the first NP primes; mul: the MUL = true instance against hat
template <int NP>
int launch_rns_ntt(zkfhe_ctx *ctx, bool mul, const uint64_t *src, int mode, uint64_t q, size_t n_polys, int log_n, const uint32_t *hat,
                   size_t hat_stride, uint32_t *out, int *flag) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds;
  ZK_CK(ntt_lds(ctx, mul ? (const void *)k_rns_ntt<NP, true> : (const void *)k_rns_ntt<NP, false>, log_n, &lds));
  zk_prof_begin(ctx);
  if (mul)
    k_rns_ntt<NP, true><<<(unsigned)(n_polys * NP), NTT_THREADS, lds, ctx->stream>>>(src, mode, q, log_n, tw, rns_const<NP>(log_n), hat, hat_stride, out, flag);
  else
    k_rns_ntt<NP, false><<<(unsigned)(n_polys * NP), NTT_THREADS, lds, ctx->stream>>>(src, mode, q, log_n, tw, rns_const<NP>(log_n), nullptr, 0, out, flag);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_RNS_NTT, (double)n_polys * NP * (8.0 + (mul ? 8.0 : 4.0)) * ((size_t)1 << log_n));
  return ZKFHE_OK;
}

// the secret key uploaded to sk_d and transformed with the first NP primes into hat; refuses a non-ternary key (zeroes flag first)
template <int NP>
int secret_hat(zkfhe_ctx *ctx, const uint64_t *sk, uint64_t n, uint64_t q, uint64_t *sk_d, uint32_t *hat, int *flag, const char *fn) {
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, sk_d, sk, n * 8));
  ZK_CK(launch_rns_ntt<NP>(ctx, false, sk_d, LOAD_TERNARY, q, 1, bit_log2(n), nullptr, 0, hat, flag));
  int bad = 0;
  ZK_CK(zkfhe_download(ctx, &bad, flag, 4));
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a secret-key coefficient is not in {0, 1, Q - 1}");
  return ZKFHE_OK;
}

}  // namespace zkrns
