// BFV evaluation on the GPU: what an aggregator computes on ciphertexts whose proofs it has checked (zkfhe.h, INTEGRATION.md
// "Computing on verified ciphertexts").  Polynomials are in the conventions of bfv_enc.hip: N residues in [0, Q), CircuitInput order.
//
// add / subtract / sum / add_plain are coefficient-wise mod Q.  mul_plain and mul need exact products of two polynomials with
// coefficients up to Q / 2 in size: |x1| = |a0 b1 + a1 b0| < 2 N (Q / 2)^2 < 2^140 at N = 2^15, Q < 2^63, so the RNS NTT of
// rns_ntt.hip.hpp runs with all five primes (product 2^151.2) on centred inputs.  mul:
//   1. k_rns_ntt: forward transforms of a0, a1, b0, b1 (centred), one workgroup per (polynomial, prime);
//   2. k_bfv_tensor: x0 = a0 b0, x1 = a0 b1 + a1 b0, x2 = a1 b1 pointwise, one inverse transform each;
//   3. k_eval_epilogue (EV_ROUND): Garner into three u64 limbs, centre, c^_j = floor((2 T x_j + Q) / 2Q) mod Q;
//   4. k_bfv_relin: per (pair, prime), every digit d_i = (c^2 >> i w) & (2^w - 1) is loaded, transformed, multiplied by the
//      transformed rlk0_i and rlk1_i and accumulated pointwise; one inverse transform per component (sum < l N 2^w Q < 2^114);
//   5. k_eval_epilogue (EV_ADD): out_j = c^_j + sum mod Q.
// The relinearization key is transformed once per call.  No step branches on or addresses by a coefficient's value.
#include <cstring>

#include "rns_ntt.hip.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
typedef unsigned __int128 u128;

enum EvMode { EV_MODQ = 0, EV_ROUND = 1, EV_ADD = 2, EV_RLK = 3, EV_NOISE = 4 };
struct EvEpi {
  int mode;
  const uint64_t *add;   // EV_ADD: + add[pos]; EV_RLK: - e[pos]; EV_NOISE: + c0[pos]
  const uint64_t *s2;    // EV_RLK: s^2, one polynomial
  uint64_t t, delta;
  int w;                 // EV_RLK: the digit width; polynomial i gets 2^(i w) s^2
  unsigned long long *noise;   // EV_NOISE: the maximum per polynomial (zeroed before the launch)
};

__device__ __forceinline__ uint64_t sub_q(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }

// One thread per output coefficient of res ([poly][prime][degree], total = n_polys N): the centred integer x of its residues, then
// EV_MODQ x mod Q; EV_ROUND floor((2 T x + Q) / 2Q) mod Q; EV_ADD x + add mod Q; EV_RLK 2^(i w) s^2 - x - e mod Q for polynomial i;
// EV_NOISE |[c0 + x - delta m]_Q| with m = the decryption of [c0 + x]_Q, maximised per polynomial.  out: CircuitInput order.
__global__ __launch_bounds__(256) void k_eval_epilogue(const uint32_t *__restrict__ res, size_t total, int log_n, uint64_t q, Crt5 cc,
                                                       EvEpi epi, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t n = (size_t)1 << log_n, poly = g >> log_n, d = g & (n - 1), pos = poly * n + (n - 1 - d);
  uint64_t m[3];
  bool neg;
  crt5(res + poly * NP * n + d, n, cc, m, neg);
  if (epi.mode == EV_ROUND) {
    // num = |x| 2T + (x < 0 ? Q - 1 : Q) in four limbs: floor((2 T x + Q) / 2Q) = -floor((2 T |x| + Q - 1) / 2Q) for x < 0
    const uint64_t t2 = 2 * epi.t, dq = 2 * q;   // both < 2^64
    u128 a = (u128)m[0] * t2 + (neg ? q - 1 : q);
    const uint64_t n0 = (uint64_t)a;
    a = (u128)m[1] * t2 + (uint64_t)(a >> 64);
    const uint64_t n1 = (uint64_t)a;
    a = (u128)m[2] * t2 + (uint64_t)(a >> 64);
    const uint64_t n2 = (uint64_t)a, n3 = (uint64_t)(a >> 64);
    // long division by 2Q, one limb at a time (the remainder carried in is below 2Q, so div128's hi < d holds)
    const uint64_t q3 = div128(0, n3, dq), r3 = n3 - q3 * dq;
    const uint64_t q2 = div128(r3, n2, dq), r2 = n2 - q2 * dq;
    const uint64_t q1 = div128(r2, n1, dq), r1 = n1 - q1 * dq;
    const uint64_t q0 = div128(r1, n0, dq);
    const uint64_t r = mod128(mod128(mod128(q3 % q, q2, q), q1, q), q0, q);
    out[pos] = neg && r ? q - r : r;
    return;
  }
  const uint64_t rm = mod128(mod128(m[2], m[1], q), m[0], q);
  uint64_t v = neg && rm ? q - rm : rm;   // x mod Q
  if (epi.mode == EV_ADD) {
    v = add_q(v, epi.add[pos], q);
  } else if (epi.mode == EV_RLK) {
    const u128 k = (u128)epi.s2[n - 1 - d] << (poly * epi.w);   // i w <= 62, s^2 < 2^63
    v = sub_q(mod128((uint64_t)(k >> 64), (uint64_t)k, q), add_q(v, epi.add[pos], q), q);
  } else if (epi.mode == EV_NOISE) {
    v = add_q(v, epi.add[pos], q);   // [c0 + c1 s]_Q
    const u128 num = (u128)(2 * epi.t) * v + q;
    uint64_t dm = div128((uint64_t)(num >> 64), (uint64_t)num, 2 * q);   // as EPI_DECRYPT of bfv_enc.hip: in [0, T]
    dm = dm == epi.t ? 0 : dm;
    dm = dm > epi.t / 2 ? q - (epi.t - dm) : dm;   // m as a residue
    const u128 prod = (u128)epi.delta * dm;
    const uint64_t x = sub_q(v, mod128((uint64_t)(prod >> 64), (uint64_t)prod, q), q);
    atomicMax(epi.noise + poly, (unsigned long long)(x > q / 2 ? q - x : x));
    return;
  }
  out[pos] = v;
}

// One workgroup per (component, pair, prime), blockIdx.x = (comp * c + k) * NP + prime.  hat holds the transforms of a0, a1, b0, b1
// of c pairs ([4 c][NP][N]); x0 = a0 b0, x1 = a0 b1 + a1 b0, x2 = a1 b1 are formed pointwise, transformed back and scaled into
// out[comp][k][prime][degree].
__global__ __launch_bounds__(NTT_THREADS) void k_bfv_tensor(const uint32_t *__restrict__ hat, size_t c, int log_n, const uint32_t *__restrict__ tw,
                                                            RnsConst<NP> rc, uint32_t *__restrict__ out) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t kc = blockIdx.x / NP, comp = kc / c, k = kc % c;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n;
  const uint32_t *A0 = hat + k * plane + (size_t)j * n, *A1 = A0 + c * plane, *B0 = A1 + c * plane, *B1 = B0 + c * plane;
  for (unsigned d = tid; d < n; d += NTT_THREADS) {
    uint32_t v;
    if (comp == 0)
      v = mont_mul(A0[d], B0[d], p, pinv);
    else if (comp == 1)
      v = add_p(mont_mul(A0[d], B1[d], p, pinv), mont_mul(A1[d], B0[d], p, pinv), p);
    else
      v = mont_mul(A1[d], B1[d], p, pinv);
    lds[d] = v;
  }
  __syncthreads();
  rns_inverse(lds, tw + (size_t)j * 2 * NMAX + NMAX, log_n, p, pinv);
  uint32_t *o = out + (size_t)blockIdx.x * n;
  for (unsigned d = tid; d < n; d += NTT_THREADS) o[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
}

// One workgroup per (pair, prime), blockIdx.x = k * NP + prime.  For every digit i < l, d_i = (c2 >> i w) & (2^w - 1) of pair k
// (c2: [c][N], CircuitInput order) is loaded, transformed and multiplied by the transforms of rlk0_i and rlk1_i (rlk_hat: [2 l][NP][N],
// the rlk0_i then the rlk1_i); the products are summed in acc[0][k][prime] and acc[1][k][prime] (each thread owns its positions),
// which are then transformed back in place.
__global__ __launch_bounds__(NTT_THREADS) void k_bfv_relin(const uint64_t *__restrict__ c2, int l, int w, const uint32_t *__restrict__ rlk_hat,
                                                           size_t c, int log_n, const uint32_t *__restrict__ tw, RnsConst<NP> rc,
                                                           uint32_t *__restrict__ acc) {
  extern __shared__ uint32_t lds[];
  const unsigned j = blockIdx.x % NP;
  const size_t k = blockIdx.x / NP;
  const unsigned n = 1u << log_n, tid = threadIdx.x;
  const uint32_t p = rc.p[j], pinv = rc.pinv[j];
  const size_t plane = (size_t)NP * n;
  const uint32_t *fw = tw + (size_t)j * 2 * NMAX, *iv = fw + NMAX;
  uint32_t *acc0 = acc + k * plane + (size_t)j * n, *acc1 = acc0 + c * plane;
  const uint64_t *s = c2 + k * n, mask = ((uint64_t)1 << w) - 1;
  for (int i = 0; i < l; ++i) {
    const int shift = i * w;   // < bitlen(Q - 1) <= 63
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = (uint32_t)(((s[n - 1 - d] >> shift) & mask) % p);
    __syncthreads();
    rns_forward(lds, fw, log_n, p, pinv);
    const uint32_t *r0 = rlk_hat + (size_t)i * plane + (size_t)j * n, *r1 = rlk_hat + (size_t)(l + i) * plane + (size_t)j * n;
    for (unsigned d = tid; d < n; d += NTT_THREADS) {
      const uint32_t x = lds[d], u0 = mont_mul(x, r0[d], p, pinv), u1 = mont_mul(x, r1[d], p, pinv);
      acc0[d] = i ? add_p(acc0[d], u0, p) : u0;
      acc1[d] = i ? add_p(acc1[d], u1, p) : u1;
    }
    __syncthreads();
  }
  for (int comp = 0; comp < 2; ++comp) {
    uint32_t *a = comp ? acc1 : acc0;
    for (unsigned d = tid; d < n; d += NTT_THREADS) lds[d] = a[d];
    __syncthreads();
    rns_inverse(lds, iv, log_n, p, pinv);
    for (unsigned d = tid; d < n; d += NTT_THREADS) a[d] = mont_mul(lds[d], rc.scale[j], p, pinv);
    __syncthreads();
  }
}

// One thread per coefficient of [c0 | c1] (2 N threads): acc[comp][i] (+)= sum over the count ciphertexts of src[comp][k][i] mod Q.
// src: [2][count][N]; consecutive threads read consecutive words of each ciphertext.
__global__ __launch_bounds__(256) void k_bfv_sum(const uint64_t *__restrict__ src, size_t count, int log_n, uint64_t q, int first,
                                                 uint64_t *__restrict__ acc) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)1 << log_n;
  if (g >= 2 * n) return;
  const size_t comp = g >> log_n, i = g & (n - 1);
  const uint64_t *s = src + comp * count * n + i;
  uint64_t v = first ? 0 : acc[g];
#pragma unroll 8
  for (size_t k = 0; k < count; ++k) v = add_q(v, s[k * n], q);
  acc[g] = v;
}

// add / subtract (b != null) or add delta m (m != null; m_shared: one plaintext of N for every polynomial): one thread per coefficient
__global__ __launch_bounds__(256) void k_bfv_add(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, int subtract,
                                                 const uint64_t *__restrict__ m, int m_shared, uint64_t delta, size_t total, int log_n,
                                                 uint64_t q, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t v = a[g];
  if (b) {
    out[g] = subtract ? sub_q(v, b[g], q) : add_q(v, b[g], q);
    return;
  }
  // m in [0, T/2] or [Q - T/2, Q): delta |m| <= Q / 2, no reduction needed (EPI_ADD of bfv_enc.hip)
  const uint64_t mv = m[m_shared ? (g & (((size_t)1 << log_n) - 1)) : g];
  const bool mneg = mv > q / 2;
  const uint64_t dm = delta * (mneg ? q - mv : mv);
  out[g] = add_q(v, mneg && dm ? q - dm : dm, q);
}

// ------------------------------------------------------------------------------------------------------------------ host side

int launch_eval_epilogue(zkfhe_ctx *ctx, const uint32_t *res, size_t n_polys, int log_n, uint64_t q, const EvEpi &epi, uint64_t *out) {
  const size_t total = n_polys << log_n;
  zk_prof_begin(ctx);
  k_eval_epilogue<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(res, total, log_n, q, crt5_const(), epi, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_EVAL_EPILOGUE, (double)total * (NP * 4 + 8 + (epi.add ? 8 : 0)));
  return ZKFHE_OK;
}

int launch_tensor(zkfhe_ctx *ctx, const uint32_t *hat, size_t c, int log_n, uint32_t *out) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  const int lds = 4 << log_n;
  if (lds > 64 * 1024) ZK_CK(zk_func_max_lds(ctx, (const void *)k_bfv_tensor, 4 << LOG_NMAX));
  zk_prof_begin(ctx);
  k_bfv_tensor<<<(unsigned)(3 * c * NP), NTT_THREADS, lds, ctx->stream>>>(hat, c, log_n, tw, rns_const<NP>(log_n), out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_TENSOR, (double)c * NP * (16.0 + 12.0) * ((size_t)1 << log_n));
  return ZKFHE_OK;
}

int launch_relin(zkfhe_ctx *ctx, const uint64_t *c2, int l, int w, const uint32_t *rlk_hat, size_t c, int log_n, uint32_t *acc) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  const int lds = 4 << log_n;
  if (lds > 64 * 1024) ZK_CK(zk_func_max_lds(ctx, (const void *)k_bfv_relin, 4 << LOG_NMAX));
  zk_prof_begin(ctx);
  k_bfv_relin<<<(unsigned)(c * NP), NTT_THREADS, lds, ctx->stream>>>(c2, l, w, rlk_hat, c, log_n, tw, rns_const<NP>(log_n), acc);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_RELIN, (double)c * NP * (l * (8.0 + 8.0 + 16.0) + 16.0) * ((size_t)1 << log_n));
  return ZKFHE_OK;
}

int launch_add(zkfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, int subtract, const uint64_t *m, int m_shared, uint64_t delta,
               size_t total, int log_n, uint64_t q, uint64_t *out) {
  zk_prof_begin(ctx);
  k_bfv_add<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(a, b, subtract, m, m_shared, delta, total, log_n, q, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_ELEMENTWISE, (double)total * 24);
  return ZKFHE_OK;
}

int relin_digits(uint64_t q, int w) {
  int bits = 0;
  while (bits < 64 && ((q - 1) >> bits)) ++bits;   // bitlen(Q - 1)
  return (bits + w - 1) / w;
}

int check_below_q(zkfhe_ctx *ctx, const uint64_t *v, size_t count, uint64_t q, const char *what) {
  for (size_t i = 0; i < count; ++i)
    if (v[i] >= q) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(what) + " coefficient is not below Q");
  return ZKFHE_OK;
}

int check_plain(zkfhe_ctx *ctx, const uint64_t *m, size_t count, uint64_t q, uint64_t t, const char *fn) {
  for (size_t i = 0; i < count; ++i)
    if (m[i] > t / 2 && (m[i] >= q || m[i] < q - t / 2))
      return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a plaintext coefficient is outside [0, T/2] and [Q - T/2, Q - 1]");
  return ZKFHE_OK;
}

// the secret key, transformed with the five primes into hat (NP planes); refuses a non-ternary key
int secret_hat(zkfhe_ctx *ctx, const uint64_t *sk, uint64_t n, uint64_t q, uint64_t *sk_d, uint32_t *hat, int *flag, const char *fn) {
  ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  ZK_CK(zkfhe_upload(ctx, sk_d, sk, n * 8));
  ZK_CK(launch_rns_ntt<NP>(ctx, false, sk_d, LOAD_TERNARY, q, 1, bit_log2(n), nullptr, 0, hat, flag));
  int bad = 0;
  ZK_CK(zkfhe_download(ctx, &bad, flag, 4));
  if (bad) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": a secret-key coefficient is not in {0, 1, Q - 1}");
  return ZKFHE_OK;
}

int check_base_bits(zkfhe_ctx *ctx, int base_bits, const char *fn) {
  if (base_bits < 1 || base_bits > 32) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(fn) + ": base_bits must be in [1, 32]");
  return ZKFHE_OK;
}

}  // namespace

extern "C" {

int zkfhe_bfv_add(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                  const uint64_t *b1, int subtract, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && a0 && a1 && b0 && b1 && out0 && out1 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  for (const uint64_t *v : {a0, a1, b0, b1}) ZK_CK(check_below_q(ctx, v, n_cts * n, q, "bfv_add: a ciphertext"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), cvec = align256(chunk * n * 8);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 3 * cvec, &w));
  uint64_t *a_d = (uint64_t *)w, *b_d = (uint64_t *)(w + cvec), *o_d = (uint64_t *)(w + 2 * cvec);
  for (int comp = 0; comp < 2; ++comp) {
    const uint64_t *a = comp ? a1 : a0, *b = comp ? b1 : b0;
    uint64_t *out = comp ? out1 : out0;
    for (size_t lo = 0; lo < n_cts; lo += chunk) {
      const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
      ZK_CK(zkfhe_upload(ctx, a_d, a + lo * n, bytes));
      ZK_CK(zkfhe_upload(ctx, b_d, b + lo * n, bytes));
      ZK_CK(launch_add(ctx, a_d, b_d, subtract, nullptr, 0, 0, c * n, log_n, q, o_d));
      ZK_CK(zkfhe_download(ctx, out + lo * n, o_d, bytes));
    }
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_sum(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                  uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && out0 && out1 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_sum: a ciphertext"));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_sum: a ciphertext"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), cvec = align256(chunk * n * 8);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, align256(2 * n * 8) + 2 * cvec, &w));
  uint64_t *acc = (uint64_t *)w, *src = (uint64_t *)(w + align256(2 * n * 8));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, src, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, src + c * n, c1 + lo * n, bytes));
    zk_prof_begin(ctx);
    k_bfv_sum<<<zk_blocks(2 * n, 256), 256, 0, ctx->stream>>>(src, c, log_n, q, lo == 0, acc);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_BFV_ELEMENTWISE, (double)(2 * c + 4) * n * 8);
  }
  ZK_CK(zkfhe_download(ctx, out0, acc, n * 8));
  ZK_CK(zkfhe_download(ctx, out1, acc + n, n * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_add_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, size_t m_count,
                        const uint64_t *m, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && m && out0 && out1 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  if (m_count != 1 && m_count != n_cts) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_add_plain: m_count must be 1 or the ciphertext count");
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_add_plain: a ciphertext"));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_add_plain: a ciphertext"));
  ZK_CK(check_plain(ctx, m, m_count * n, q, params->t, "bfv_add_plain"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), cvec = align256(chunk * n * 8);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 3 * cvec, &w));
  uint64_t *c_d = (uint64_t *)w, *m_d = (uint64_t *)(w + cvec), *o_d = (uint64_t *)(w + 2 * cvec);
  const bool shared = m_count == 1;
  if (shared) ZK_CK(zkfhe_upload(ctx, m_d, m, n * 8));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, c_d, c0 + lo * n, bytes));
    if (!shared) ZK_CK(zkfhe_upload(ctx, m_d, m + lo * n, bytes));
    ZK_CK(launch_add(ctx, c_d, nullptr, 0, m_d, shared, q / params->t, c * n, log_n, q, o_d));
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, o_d, bytes));
  }
  if (out1 != c1) memcpy(out1, c1, n_cts * n * 8);
  return ZKFHE_OK;
}

int zkfhe_bfv_mul_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, size_t m_count,
                        const uint64_t *m, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && m && out0 && out1 && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  if (m_count != 1 && m_count != n_cts) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_mul_plain: m_count must be 1 or the ciphertext count");
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_mul_plain: a ciphertext"));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_mul_plain: a ciphertext"));
  ZK_CK(check_plain(ctx, m, m_count * n, q, params->t, "bfv_mul_plain"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), cvec = align256(chunk * n * 8), cplane = align256(chunk * NP * n * 4);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + 3 * cvec + 2 * cplane, &w));
  int *flag = (int *)w;
  uint64_t *c_d = (uint64_t *)(w + 256), *m_d = (uint64_t *)((char *)c_d + cvec), *o_d = (uint64_t *)((char *)m_d + cvec);
  uint32_t *hat = (uint32_t *)((char *)o_d + cvec), *res = (uint32_t *)((char *)hat + cplane);
  const bool shared = m_count == 1;
  if (shared) {
    ZK_CK(zkfhe_upload(ctx, m_d, m, n * 8));
    ZK_CK(launch_rns_ntt<NP>(ctx, false, m_d, LOAD_CENTRED, q, 1, log_n, nullptr, 0, hat, flag));
  }
  const EvEpi epi{EV_MODQ, nullptr, nullptr, 0, 0, 0, nullptr};
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    if (!shared) {
      ZK_CK(zkfhe_upload(ctx, m_d, m + lo * n, bytes));
      ZK_CK(launch_rns_ntt<NP>(ctx, false, m_d, LOAD_CENTRED, q, c, log_n, nullptr, 0, hat, flag));
    }
    for (int comp = 0; comp < 2; ++comp) {
      ZK_CK(zkfhe_upload(ctx, c_d, (comp ? c1 : c0) + lo * n, bytes));
      ZK_CK(launch_rns_ntt<NP>(ctx, true, c_d, LOAD_CENTRED, q, c, log_n, hat, shared ? 0 : (size_t)NP * n, res, flag));
      ZK_CK(launch_eval_epilogue(ctx, res, c, log_n, q, epi, o_d));
      ZK_CK(zkfhe_download(ctx, (comp ? out1 : out0) + lo * n, o_d, bytes));
    }
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_relin_digits(const zkfhe_bfv_params *params, int base_bits, size_t *l) {
  if (!l) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_relin_digits: l is NULL");
  ZK_CK(zk_bfv_check_params(nullptr, params));
  ZK_CK(check_base_bits(nullptr, base_bits, "bfv_relin_digits"));
  *l = (size_t)relin_digits(params->q, base_bits);
  return ZKFHE_OK;
}

int zkfhe_bfv_relin_keygen(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t seed[32], int base_bits,
                           uint64_t *rlk0_out, uint64_t *rlk1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && seed && rlk0_out && rlk1_out);
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_base_bits(ctx, base_bits, "bfv_relin_keygen"));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), l = relin_digits(q, base_bits), n_cdt = (int)(2 * params->b);
  std::vector<uint64_t> cdt(n_cdt);
  zk_bfv_error_cdt(params->b, cdt.data());
  const size_t vec = align256(n * 8), lvec = align256(l * n * 8), plane = align256((size_t)NP * n * 4);
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + 2 * vec + 3 * lvec + align256(n_cdt * 8) + plane + align256((size_t)l * NP * n * 4), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += bytes; return r; };
  uint64_t *s_d = (uint64_t *)take(vec), *s2_d = (uint64_t *)take(vec), *a_d = (uint64_t *)take(lvec), *e_d = (uint64_t *)take(lvec);
  uint64_t *r0_d = (uint64_t *)take(lvec), *cdt_d = (uint64_t *)take(align256(n_cdt * 8));
  uint32_t *hat = (uint32_t *)take(plane), *res = (uint32_t *)take(align256((size_t)l * NP * n * 4));
  ZK_CK(secret_hat(ctx, sk, n, q, s_d, hat, flag, "bfv_relin_keygen"));
  ZK_CK(zkfhe_upload(ctx, cdt_d, cdt.data(), n_cdt * 8));
  // s^2 mod Q: the product of s (read as ternary) with its own transform
  ZK_CK(launch_rns_ntt<NP>(ctx, true, s_d, LOAD_TERNARY, q, 1, log_n, hat, 0, res, flag));
  ZK_CK(launch_eval_epilogue(ctx, res, 1, log_n, q, EvEpi{EV_MODQ, nullptr, nullptr, 0, 0, 0, nullptr}, s2_d));
  ZK_CK(zk_bfv_sample(ctx, seed, 7, 0, 1, l, log_n, q, nullptr, 0, a_d));         // a_i: uniform, domain 7, index i
  ZK_CK(zk_bfv_sample(ctx, seed, 8, 0, 2, l, log_n, q, cdt_d, n_cdt, e_d));      // e_i: error, domain 8, index i
  ZK_CK(launch_rns_ntt<NP>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat, 0, res, flag));
  ZK_CK(launch_eval_epilogue(ctx, res, l, log_n, q, EvEpi{EV_RLK, e_d, s2_d, 0, 0, base_bits, nullptr}, r0_d));
  ZK_CK(zkfhe_download(ctx, rlk0_out, r0_d, (size_t)l * n * 8));
  ZK_CK(zkfhe_download(ctx, rlk1_out, a_d, (size_t)l * n * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_mul(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_pairs, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                  const uint64_t *b1, const uint64_t *rlk0, const uint64_t *rlk1, int base_bits, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && a0 && a1 && b0 && b1 && rlk0 && rlk1 && out0 && out1 && n_pairs > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  ZK_CK(check_base_bits(ctx, base_bits, "bfv_mul"));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), l = relin_digits(q, base_bits);
  for (const uint64_t *v : {a0, a1, b0, b1}) ZK_CK(check_below_q(ctx, v, n_pairs * n, q, "bfv_mul: a ciphertext"));
  ZK_CK(check_below_q(ctx, rlk0, (size_t)l * n, q, "bfv_mul: a relinearization-key"));
  ZK_CK(check_below_q(ctx, rlk1, (size_t)l * n, q, "bfv_mul: a relinearization-key"));
  const size_t chunk = std::min<size_t>(n_pairs, chunk_polys(n)), plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + align256(2 * l * n * 8) + align256(2 * l * plane) + align256(4 * chunk * n * 8) + align256(4 * chunk * plane) +
                                   align256(3 * chunk * plane) + align256(3 * chunk * n * 8) + align256(2 * chunk * n * 8), &w));
  int *flag = (int *)w;
  char *at = w + 256;
  auto take = [&](size_t bytes) { char *r = at; at += align256(bytes); return r; };
  uint64_t *rlk_d = (uint64_t *)take(2 * l * n * 8);
  uint32_t *rlk_hat = (uint32_t *)take(2 * l * plane);
  uint64_t *in_d = (uint64_t *)take(4 * chunk * n * 8);
  uint32_t *hat = (uint32_t *)take(4 * chunk * plane), *res = (uint32_t *)take(3 * chunk * plane);
  uint64_t *chat = (uint64_t *)take(3 * chunk * n * 8), *o_d = (uint64_t *)take(2 * chunk * n * 8);
  ZK_CK(zkfhe_upload(ctx, rlk_d, rlk0, (size_t)l * n * 8));
  ZK_CK(zkfhe_upload(ctx, rlk_d + (size_t)l * n, rlk1, (size_t)l * n * 8));
  ZK_CK(launch_rns_ntt<NP>(ctx, false, rlk_d, LOAD_RESIDUE, q, 2 * l, log_n, nullptr, 0, rlk_hat, flag));
  const uint64_t *src[4] = {a0, a1, b0, b1};
  for (size_t lo = 0; lo < n_pairs; lo += chunk) {
    const size_t c = std::min(chunk, n_pairs - lo), bytes = c * n * 8;
    for (int i = 0; i < 4; ++i) ZK_CK(zkfhe_upload(ctx, in_d + i * c * n, src[i] + lo * n, bytes));
    ZK_CK(launch_rns_ntt<NP>(ctx, false, in_d, LOAD_CENTRED, q, 4 * c, log_n, nullptr, 0, hat, flag));
    ZK_CK(launch_tensor(ctx, hat, c, log_n, res));
    ZK_CK(launch_eval_epilogue(ctx, res, 3 * c, log_n, q, EvEpi{EV_ROUND, nullptr, nullptr, params->t, 0, 0, nullptr}, chat));
    ZK_CK(launch_relin(ctx, chat + 2 * c * n, l, base_bits, rlk_hat, c, log_n, res));
    ZK_CK(launch_eval_epilogue(ctx, res, 2 * c, log_n, q, EvEpi{EV_ADD, chat, nullptr, 0, 0, 0, nullptr}, o_d));
    ZK_CK(zkfhe_download(ctx, out0 + lo * n, o_d, bytes));
    ZK_CK(zkfhe_download(ctx, out1 + lo * n, o_d + c * n, bytes));
  }
  return ZKFHE_OK;
}

int zkfhe_bfv_noise(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, size_t n_cts, const uint64_t *c0, const uint64_t *c1,
                    uint64_t *noise_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && c0 && c1 && noise_out && n_cts > 0);
  ZK_CK(zk_bfv_check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_noise: a ciphertext"));
  ZK_CK(check_below_q(ctx, c1, n_cts * n, q, "bfv_noise: a ciphertext"));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), vec = align256(n * 8), cvec = align256(chunk * n * 8);
  const size_t plane = (size_t)NP * n * 4;
  char *w;
  ZK_CK(zk_bfv_work_arena(ctx, 256 + vec + align256(plane) + 2 * cvec + align256(chunk * 8) + align256(chunk * plane), &w));
  int *flag = (int *)w;
  uint64_t *sk_d = (uint64_t *)(w + 256);
  uint32_t *hat = (uint32_t *)((char *)sk_d + vec);
  uint64_t *c0_d = (uint64_t *)((char *)hat + align256(plane)), *c1_d = (uint64_t *)((char *)c0_d + cvec);
  uint64_t *nz_d = (uint64_t *)((char *)c1_d + cvec);
  uint32_t *res = (uint32_t *)((char *)nz_d + align256(chunk * 8));
  ZK_CK(secret_hat(ctx, sk, n, q, sk_d, hat, flag, "bfv_noise"));
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, c0_d, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, c1_d, c1 + lo * n, bytes));
    ZK_HIP(ctx, hipMemsetAsync(nz_d, 0, c * 8, ctx->stream));
    ZK_CK(launch_rns_ntt<NP>(ctx, true, c1_d, LOAD_RESIDUE, q, c, log_n, hat, 0, res, flag));
    const EvEpi epi{EV_NOISE, c0_d, nullptr, params->t, q / params->t, 0, (unsigned long long *)nz_d};
    ZK_CK(launch_eval_epilogue(ctx, res, c, log_n, q, epi, nullptr));
    ZK_CK(zkfhe_download(ctx, noise_out + lo, nz_d, c * 8));
  }
  return ZKFHE_OK;
}

}  // extern "C"
