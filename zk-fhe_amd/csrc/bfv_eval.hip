// BFV evaluation on the GPU: what an aggregator computes on ciphertexts whose proofs it has checked (zkfhe.h, INTEGRATION.md
// "Computing on verified ciphertexts").  Polynomials are in the conventions of bfv_enc.hip: N residues in [0, Q), CircuitInput order.
//
// add / subtract / sum / add_plain are coefficient-wise mod Q.  mul_plain and mul need exact products of two polynomials with
// coefficients up to Q / 2 in size: |x1| = |a0 b1 + a1 b0| < 2 N (Q / 2)^2 < 2^140 at N = 2^15, Q < 2^63, so the RNS NTT of
// rns_ntt.hip.hpp runs with all five primes (product 2^151.2) on centred inputs.  mul:
//   1. k_rns_ntt: forward transforms of a0, a1, b0, b1 (centred), one workgroup per (polynomial, prime);
//   2. k_bfv_tensor: x0 = a0 b0, x1 = a0 b1 + a1 b0, x2 = a1 b1 pointwise, one inverse transform each;
//   3. k_eval_epilogue (EV_ROUND): Garner into three u64 limbs, centre, c^_j = floor((2 T x_j + Q) / 2Q) mod Q;
//   4. the key switch of bfv_key_switch.hip on c^2 itself (SrcPlain: the relinearization): every digit d_i = (c^2 >> i w) & (2^w - 1)
//      is transformed, multiplied by the transformed rlk0_i and rlk1_i and summed; one inverse transform per component
//      (sum < l N 2^w Q < 2^114; with the keys of a hybrid set, integers below Q P, sum <= l N (2^w - 1) (Q P - 1) <= P5 / 2);
//   5. k_eval_epilogue (EV_ADD): out_j = c^_j + sum mod Q (a hybrid set: the sum divided by P with rounding, k_eval_epilogue<true>).
// The relinearization key is transformed once per call.  No step branches on or addresses by a coefficient's value.
// k_eval_epilogue also serves the Galois key switch of bfv_galois.hip (EV_GALOIS).
// add / subtract, add_plain / mul_plain and mul each have one runner (zk_bfv_add_run, zk_bfv_plain_run, zk_bfv_mul_run: the chunk
// loop, on operands that are host arrays or device planes and a key that is host rows or resident, bfv_host.hpp).  An entry point
// here is its host checks and one call of a runner on host arrays; the batch calls of bfv_resident.hip call the same runners.
#include <cstring>

#include "bfv_host.hpp"

using namespace zkrns;

namespace {

constexpr int NP = NP_MAX;
typedef unsigned __int128 u128;

// One thread per output coefficient of res ([poly][prime][degree], total = n_polys N): the centred integer x of its residues, then
// the mode's result (EvMode).  out: CircuitInput order.  HYB: the epilogue of a hybrid key switch (EV_ADD, EV_GALOIS), which puts
// floor((2 x + P) / 2P) mod Q where the ordinary one puts x mod Q; the ordinary instance keeps its code.
template <bool HYB>
__global__ __launch_bounds__(256) void k_eval_epilogue(const uint32_t *__restrict__ res, size_t total, int log_n, uint64_t q, Crt5 cc,
                                                       EvEpi epi, uint64_t *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t n = (size_t)1 << log_n, poly = g >> log_n, d = g & (n - 1), pos = poly * n + (n - 1 - d);
  uint64_t m[3];
  bool neg;
  crt5(res + poly * NP * n + d, n, cc, m, neg);
  if (!HYB && epi.mode == EV_ROUND) {
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
  uint64_t v = HYB ? crt5_div_p_mod_q(m, neg, epi.p, q) : crt5_mod_q(m, neg, q);   // x mod Q
  if (epi.mode == EV_ADD) {
    v = add_q(v, epi.add[pos], q);
  } else if (!HYB && epi.mode == EV_RLK) {
    const u128 k = (u128)epi.poly[n - 1 - d] << (poly * epi.w);   // i w <= 62, s^2 < 2^63
    v = sub_q(mod128((uint64_t)(k >> 64), (uint64_t)k, q), add_q(v, epi.add[pos], q), q);
  } else if (!HYB && epi.mode == EV_NOISE) {
    v = add_q(v, epi.add[pos], q);   // [c0 + c1 s]_Q
    const u128 prod = (u128)epi.delta * decrypt_round(v, q, epi.t);   // delta m, m as a residue
    const uint64_t x = sub_q(v, mod128((uint64_t)(prod >> 64), (uint64_t)prod, q), q);
    atomicMax(epi.noise + poly, (unsigned long long)(x > q / 2 ? q - x : x));
    return;
  } else if (epi.mode == EV_GALOIS) {
    if (poly < epi.c) v = add_q(v, auto_coeff(epi.poly + poly * n, (unsigned)d, epi.ginv, (unsigned)n, q), q);
    if (epi.add) v = add_q(v, epi.add[pos], q);
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
  out[g] = add_delta_m(v, m[m_shared ? (g & (((size_t)1 << log_n) - 1)) : g], delta, q);
}

// ------------------------------------------------------------------------------------------------------------------ host side

int launch_tensor(zkfhe_ctx *ctx, const uint32_t *hat, size_t c, int log_n, uint32_t *out) {
  const uint32_t *tw;
  ZK_CK(zk_rns_tables(ctx, &tw));
  int lds;
  ZK_CK(ntt_lds(ctx, (const void *)k_bfv_tensor, log_n, &lds));
  zk_prof_begin(ctx);
  k_bfv_tensor<<<(unsigned)(3 * c * NP), NTT_THREADS, lds, ctx->stream>>>(hat, c, log_n, tw, rns_const<NP>(log_n), out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_TENSOR, (double)c * NP * (16.0 + 12.0) * ((size_t)1 << log_n));
  return ZKFHE_OK;
}

}  // namespace

namespace zkrns {

int zk_bfv_eval_epilogue(zkfhe_ctx *ctx, const uint32_t *res, size_t n_polys, int log_n, uint64_t q, const EvEpi &epi, uint64_t *out) {
  const size_t total = n_polys << log_n;
  zk_prof_begin(ctx);
  if (epi.p != 1)
    k_eval_epilogue<true><<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(res, total, log_n, q, crt5_const(), epi, out);
  else
    k_eval_epilogue<false><<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(res, total, log_n, q, crt5_const(), epi, out);
  ZK_LAUNCH_CHECK(ctx);
  double bytes = (double)total * (NP * 4 + 8 + (epi.add ? 8 : 0));
  if (epi.mode == EV_GALOIS) bytes += (double)(epi.c << log_n) * 8;   // sigma_g(c0)
  zk_prof_end(ctx, epi.mode == EV_GALOIS ? ZKFHE_PROF_BFV_GALOIS : ZKFHE_PROF_BFV_EVAL_EPILOGUE, bytes);
  return ZKFHE_OK;
}

namespace {

// k_bfv_add over total words: out = a +/- b (b set) or a + delta m (m set; m_shared: one plaintext of N words for every polynomial)
int add_core(zkfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, int subtract, const uint64_t *m, int m_shared, uint64_t delta, size_t total,
             int log_n, uint64_t q, uint64_t *out) {
  zk_prof_begin(ctx);
  k_bfv_add<<<zk_blocks(total, 256), 256, 0, ctx->stream>>>(a, b, subtract, m, m_shared, delta, total, log_n, q, out);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_BFV_ELEMENTWISE, (double)total * 24);
  return ZKFHE_OK;
}

// rows centred polynomials of src ([rows][N]) transformed with the five primes into hat ([rows][5][N])
int centred_hat(zkfhe_ctx *ctx, const uint64_t *src, uint64_t q, size_t rows, int log_n, uint32_t *hat, int *flag) {
  return launch_rns_ntt<NP>(ctx, false, src, LOAD_CENTRED, q, rows, log_n, nullptr, 0, hat, flag);
}

// one component of mul_plain: out = x m mod (x^N + 1, Q) for the c polynomials of x against m_hat (hat_stride 0: one plaintext)
int mul_plain_core(zkfhe_ctx *ctx, const uint64_t *x, size_t c, int log_n, uint64_t q, const uint32_t *m_hat, size_t hat_stride, uint32_t *res,
                   int *flag, uint64_t *out) {
  ZK_CK(launch_rns_ntt<NP>(ctx, true, x, LOAD_CENTRED, q, c, log_n, m_hat, hat_stride, res, flag));
  return zk_bfv_eval_epilogue(ctx, res, c, log_n, q, EvEpi{}, out);
}

// the work buffers of mul behind its key
struct MulWork {
  int *flag;
  uint64_t *in_d, *chat, *o_d;
  uint32_t *hat, *res;
  const uint32_t *key;   // the transformed key ([2 l][5][N])
  uint64_t special;      // its special modulus (1: none)
};

// steps 1 to 5 of the top of the file for c pairs: w.in_d = [a0 | a1 | b0 | b1] ([4 c][N]); w.o_d = [out0 | out1]
int mul_core(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t c, const KeySwitch &ks, const MulWork &w) {
  const uint64_t n = prm->n, q = prm->q;
  const int log_n = bit_log2(n);
  ZK_CK(centred_hat(ctx, w.in_d, q, 4 * c, log_n, w.hat, w.flag));
  ZK_CK(launch_tensor(ctx, w.hat, c, log_n, w.res));
  ZK_CK(zk_bfv_eval_epilogue(ctx, w.res, 3 * c, log_n, q, EvEpi{.mode = EV_ROUND, .t = prm->t}, w.chat));
  ZK_CK(zk_bfv_key_switch(ctx, ks, SrcPlain{w.chat + 2 * c * n}, w.key, c, w.res));
  return zk_bfv_eval_epilogue(ctx, w.res, 2 * c, log_n, q, EvEpi{.mode = EV_ADD, .add = w.chat, .p = w.special}, w.o_d);
}

}  // namespace

int zk_bfv_add_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, const Planes &b, int subtract, const Planes &out) {
  const uint64_t n = prm->n, q = prm->q;
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(count, chunk_polys(n)), cw = chunk * n;
  uint64_t *a_d = nullptr, *b_d = nullptr, *o_d;
  Arena ar;
  a.stage(ar, a_d, cw), b.stage(ar, b_d, cw);
  ZK_CK(ar.add(o_d, cw).carve(ctx));
  for (int comp = 0; comp < 2; ++comp)
    for (size_t lo = 0; lo < count; lo += chunk) {
      const size_t c = std::min(chunk, count - lo);
      const uint64_t *x, *y;
      ZK_CK(a.at(ctx, comp, lo, c, n, a_d, &x));
      ZK_CK(b.at(ctx, comp, lo, c, n, b_d, &y));
      ZK_CK(add_core(ctx, x, y, subtract, nullptr, 0, 0, c * n, log_n, q, o_d));
      ZK_CK(out.out(ctx, comp, lo, c, n, o_d));
    }
  return out.done(ctx);
}

int zk_bfv_plain_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, bool mul, size_t count, const Planes &a, size_t m_count, const uint64_t *m,
                     const Planes &out) {
  const uint64_t n = prm->n, q = prm->q;
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(count, chunk_polys(n)), cw = chunk * n;
  int *flag = nullptr;
  uint64_t *c_d = nullptr, *m_d, *o_d;
  uint32_t *hat = nullptr, *res = nullptr;
  Arena ar;
  if (mul) ar.add(flag, 1);
  a.stage(ar, c_d, cw);
  ar.add(m_d, cw).add(o_d, cw);
  if (mul) ar.add(hat, cw * NP).add(res, cw * NP);
  ZK_CK(ar.carve(ctx));
  const bool shared = m_count == 1;
  if (shared) {
    ZK_CK(zkfhe_upload(ctx, m_d, m, n * 8));
    if (mul) ZK_CK(centred_hat(ctx, m_d, q, 1, log_n, hat, flag));
  }
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t c = std::min(chunk, count - lo);
    if (!shared) {
      ZK_CK(zkfhe_upload(ctx, m_d, m + lo * n, c * n * 8));
      if (mul) ZK_CK(centred_hat(ctx, m_d, q, c, log_n, hat, flag));
    }
    for (int comp = 0; comp < (mul ? 2 : 1); ++comp) {
      const uint64_t *x;
      ZK_CK(a.at(ctx, comp, lo, c, n, c_d, &x));
      if (mul)
        ZK_CK(mul_plain_core(ctx, x, c, log_n, q, hat, shared ? 0 : (size_t)NP * n, res, flag, o_d));
      else
        ZK_CK(add_core(ctx, x, nullptr, 0, m_d, shared, q / prm->t, c * n, log_n, q, o_d));
      ZK_CK(out.out(ctx, comp, lo, c, n, o_d));
    }
  }
  if (!mul && out.p[1] != a.p[1]) {   // add_plain leaves c1 as it is: copied where the data lives, not at all in place
    if (out.dev)
      ZK_CK(a.in(ctx, 1, 0, count, n, out.p[1]));
    else if (a.dev)
      ZK_CK(out.out(ctx, 1, 0, count, n, a.p[1]));
    else
      memcpy(out.p[1], a.p[1], count * n * 8);
  }
  return out.done(ctx);
}

int zk_bfv_mul_run(zkfhe_ctx *ctx, const zkfhe_bfv_params *prm, size_t count, const Planes &a, const Planes &b, KeySource key, int l, int base_bits,
                   const Planes &out) {
  const uint64_t n = prm->n;
  const size_t chunk = std::min<size_t>(count, chunk_polys(n)), cw = chunk * n;
  KeySwitch ks{bit_log2(n), l, base_bits, prm->q};
  MulWork w;
  Arena ar;
  ar.add(w.flag, 1);
  key.add(ar, n, l);
  ar.add(w.in_d, 4 * cw).add(w.hat, 4 * cw * NP).add(w.res, 3 * cw * NP).add(w.chat, 3 * cw).add(w.o_d, 2 * cw);
  ks.add(ar, ctx, key, chunk);
  ZK_CK(ar.carve(ctx));
  ZK_CK(stage_keys<NP>(ctx, key, n, prm->q, l, w.flag));
  w.key = key.hat(0), w.special = key.special;
  const Planes *src[2] = {&a, &b};
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t c = std::min(chunk, count - lo);
    for (int i = 0; i < 4; ++i) ZK_CK(src[i / 2]->in(ctx, i % 2, lo, c, n, w.in_d + i * c * n));   // the 4 c transforms want them contiguous
    ZK_CK(mul_core(ctx, prm, c, ks, w));
    ZK_CK(out.out(ctx, 0, lo, c, n, w.o_d));
    ZK_CK(out.out(ctx, 1, lo, c, n, w.o_d + c * n));
  }
  return out.done(ctx);
}

}  // namespace zkrns

extern "C" {

int zkfhe_bfv_add(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                  const uint64_t *b1, int subtract, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && a0 && a1 && b0 && b1 && out0 && out1 && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, a0, n_cts * n, q, "bfv_add", "a ciphertext", a1));
  ZK_CK(check_below_q(ctx, b0, n_cts * n, q, "bfv_add", "a ciphertext", b1));
  return zk_bfv_add_run(ctx, params, n_cts, host_planes(a0, a1), host_planes(b0, b1), subtract, host_planes(out0, out1));
}

int zkfhe_bfv_sum(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                  uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && out0 && out1 && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_sum", "a ciphertext", c1));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n));
  uint64_t *acc, *src;
  ZK_CK(Arena().add(acc, 2 * n).add(src, 2 * chunk * n).carve(ctx));
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
  ZK_CK(check_params(ctx, params));
  if (m_count != 1 && m_count != n_cts) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_add_plain: m_count must be 1 or the ciphertext count");
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_add_plain", "a ciphertext", c1));
  ZK_CK(check_plain(ctx, m, m_count * n, q, params->t, "bfv_add_plain"));
  return zk_bfv_plain_run(ctx, params, false, n_cts, host_planes(c0, c1), m_count, m, host_planes(out0, out1));
}

int zkfhe_bfv_mul_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, size_t m_count,
                        const uint64_t *m, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && c0 && c1 && m && out0 && out1 && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  if (m_count != 1 && m_count != n_cts) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bfv_mul_plain: m_count must be 1 or the ciphertext count");
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_mul_plain", "a ciphertext", c1));
  ZK_CK(check_plain(ctx, m, m_count * n, q, params->t, "bfv_mul_plain"));
  return zk_bfv_plain_run(ctx, params, true, n_cts, host_planes(c0, c1), m_count, m, host_planes(out0, out1));
}

int zkfhe_bfv_relin_digits(const zkfhe_bfv_params *params, int base_bits, size_t *l) {
  if (!l) return zk_fail_msg(nullptr, ZKFHE_EINVAL, "bfv_relin_digits: l is NULL");
  ZK_CK(check_params(nullptr, params));
  int rows = 0;
  ZK_CK(relin_rows(nullptr, params, base_bits, "bfv_relin_digits", &rows));
  *l = (size_t)rows;
  return ZKFHE_OK;
}

int zkfhe_bfv_relin_keygen(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t seed[32], int base_bits,
                           uint64_t *rlk0_out, uint64_t *rlk1_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && seed && rlk0_out && rlk1_out);
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_relin_keygen", &l));
  const uint64_t n = params->n, q = params->q;
  const int log_n = bit_log2(n), n_cdt = (int)(2 * params->b);
  const size_t lw = (size_t)l * n;
  int *flag;
  uint64_t *s_d, *s2_d, *a_d, *e_d, *r0_d, *cdt_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(s_d, n).add(s2_d, n).add(a_d, lw).add(e_d, lw).add(r0_d, lw).add(cdt_d, n_cdt).add(hat, NP * n)
            .add(res, lw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk, n, q, s_d, hat, flag, "bfv_relin_keygen"));
  ZK_CK(upload_error_cdt(ctx, params, cdt_d));
  // s^2 mod Q: the product of s (read as ternary) with its own transform
  ZK_CK(launch_rns_ntt<NP>(ctx, true, s_d, LOAD_TERNARY, q, 1, log_n, hat, 0, res, flag));
  ZK_CK(zk_bfv_eval_epilogue(ctx, res, 1, log_n, q, EvEpi{}, s2_d));
  ZK_CK(zk_bfv_sample(ctx, seed, DOM_RLK_A, 0, S_UNIFORM, l, log_n, q, nullptr, 0, a_d));    // a_i, index i
  ZK_CK(zk_bfv_sample(ctx, seed, DOM_RLK_E, 0, S_ERROR, l, log_n, q, cdt_d, n_cdt, e_d));   // e_i, index i
  ZK_CK(launch_rns_ntt<NP>(ctx, true, a_d, LOAD_RESIDUE, q, l, log_n, hat, 0, res, flag));
  ZK_CK(zk_bfv_eval_epilogue(ctx, res, l, log_n, q, EvEpi{.mode = EV_RLK, .add = e_d, .poly = s2_d, .w = base_bits}, r0_d));
  ZK_CK(zkfhe_download(ctx, rlk0_out, r0_d, lw * 8));
  ZK_CK(zkfhe_download(ctx, rlk1_out, a_d, lw * 8));
  return ZKFHE_OK;
}

int zkfhe_bfv_mul(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_pairs, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                  const uint64_t *b1, const uint64_t *rlk0, const uint64_t *rlk1, int base_bits, uint64_t *out0, uint64_t *out1) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && a0 && a1 && b0 && b1 && rlk0 && rlk1 && out0 && out1 && n_pairs > 0);
  ZK_CK(check_params(ctx, params));
  int l = 0;
  ZK_CK(relin_rows(ctx, params, base_bits, "bfv_mul", &l));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, a0, n_pairs * n, q, "bfv_mul", "a ciphertext", a1));
  ZK_CK(check_below_q(ctx, b0, n_pairs * n, q, "bfv_mul", "a ciphertext", b1));
  ZK_CK(check_below_q(ctx, rlk0, (size_t)l * n, q, "bfv_mul", "a relinearization-key", rlk1));
  return zk_bfv_mul_run(ctx, params, n_pairs, host_planes(a0, a1), host_planes(b0, b1), host_keys(rlk0, rlk1), l, base_bits, host_planes(out0, out1));
}

int zkfhe_bfv_noise(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, size_t n_cts, const uint64_t *c0, const uint64_t *c1,
                    uint64_t *noise_out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && sk && c0 && c1 && noise_out && n_cts > 0);
  ZK_CK(check_params(ctx, params));
  const uint64_t n = params->n, q = params->q;
  ZK_CK(check_below_q(ctx, c0, n_cts * n, q, "bfv_noise", "a ciphertext", c1));
  const int log_n = bit_log2(n);
  const size_t chunk = std::min<size_t>(n_cts, chunk_polys(n)), cw = chunk * n;
  int *flag;
  uint64_t *sk_d, *c0_d, *c1_d;
  unsigned long long *nz_d;
  uint32_t *hat, *res;
  ZK_CK(Arena().add(flag, 1).add(sk_d, n).add(hat, NP * n).add(c0_d, cw).add(c1_d, cw).add(nz_d, chunk).add(res, cw * NP).carve(ctx));
  ZK_CK(secret_hat<NP>(ctx, sk, n, q, sk_d, hat, flag, "bfv_noise"));
  const EvEpi epi{.mode = EV_NOISE, .add = c0_d, .t = params->t, .delta = q / params->t, .noise = nz_d};
  for (size_t lo = 0; lo < n_cts; lo += chunk) {
    const size_t c = std::min(chunk, n_cts - lo), bytes = c * n * 8;
    ZK_CK(zkfhe_upload(ctx, c0_d, c0 + lo * n, bytes));
    ZK_CK(zkfhe_upload(ctx, c1_d, c1 + lo * n, bytes));
    ZK_HIP(ctx, hipMemsetAsync(nz_d, 0, c * 8, ctx->stream));
    ZK_CK(launch_rns_ntt<NP>(ctx, true, c1_d, LOAD_RESIDUE, q, c, log_n, hat, 0, res, flag));
    ZK_CK(zk_bfv_eval_epilogue(ctx, res, c, log_n, q, epi, nullptr));
    ZK_CK(zkfhe_download(ctx, noise_out + lo, nz_d, c * 8));
  }
  return ZKFHE_OK;
}

}  // extern "C"
