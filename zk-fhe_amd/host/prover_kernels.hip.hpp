// Device kernels of the prover steps P1, P4-P10: everything between the column NTT/MSM
// primitives of csrc/ and the host-side transcript.  All polynomials stay resident in HBM; the
// extended (quotient) domain is kept COSET-MAJOR ([k1][k2], see zkfhe_coset_ntt_batch), so a rotation by
// omega is an index shift inside a row and X^n - 1 is constant per row.
#pragma once
#include "../csrc/ctx.hpp"
#include "../csrc/fr9.hip.hpp"
#include "chain_jobs.hpp"

namespace zkp {

using zk::Fr;

// ------------------------------------------------------------------------------------------- small utilities
// Kernel bodies that more than one launch runs are __device__ functions of (blk, nblk): the index of the workgroup among the nblk
// workgroups that share the body's rows.  A kernel of its own passes (blockIdx.x, gridDim.x); a launch that runs several bodies side
// by side gives every body a range of its workgroups (the "side by side" kernels below).  No body waits for another workgroup.
// out[i] = start * base^i
__device__ __forceinline__ void powers_body(Fr start, Fr base, Fr *__restrict__ out, size_t n, unsigned blk, unsigned nblk) {
  for (size_t i = blk * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)nblk * blockDim.x) {
    Fr r = start, b = base;
    for (size_t e = i; e; e >>= 1) {
      if (e & 1) r = r * b;
      b = zk::fp_sqr<zk::FrP>(b);
    }
    out[i] = r;
  }
}
static __global__ void __launch_bounds__(256) k_powers(Fr start, Fr base, Fr *__restrict__ out, size_t n) { powers_body(start, base, out, n, blockIdx.x, gridDim.x); }

// SRS: den[i] = n (s - w^i)   (inverted by the caller);  then li[i] = w^i (s^n - 1) * inv[i]
// ---- the blinding stream on the device ------------------------------------------------------------------------------
// draw(i) = Blake2b-512(person "zkfhe-rng", seed[32] || i as u64 LE) reduced mod r (transcript.hpp `Rng`, oracle/halo2_ref.py
// `Rng`): counter based, so every blinding row / random coefficient of a proof is a pure function of (seed, index) and is
// written where it is needed -- no host hashing (it was 50 k hashes = 12 ms of host CPU per k = 13 proof) and no upload.
__device__ __forceinline__ unsigned long long rotr64(unsigned long long x, int n) { return (x >> n) | (x << (64 - n)); }
__device__ __forceinline__ Fr rng_draw(const unsigned long long seed[4], unsigned long long ctr) {
  typedef unsigned long long u64;
  const u64 IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                     0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  const unsigned char S[12][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
  u64 h[8], m[16], v[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV[i];
  h[0] ^= 0x01010040ULL;                 // digest length 64, no key, fanout = depth = 1
  h[6] ^= 0x6e722d6568666b7aULL;         // personalisation "zkfhe-rn"
  h[7] ^= 0x0000000000000067ULL;         //                 "g" + zero padding
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = 0;
  m[0] = seed[0], m[1] = seed[1], m[2] = seed[2], m[3] = seed[3], m[4] = ctr;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = h[i];
    v[i + 8] = IV[i];
  }
  v[12] ^= 40;        // 40 message bytes
  v[14] = ~v[14];     // last block
#define ZK_B2G(a, b, c, d, x, y)          \
  v[a] = v[a] + v[b] + (x);               \
  v[d] = rotr64(v[d] ^ v[a], 32);         \
  v[c] = v[c] + v[d];                     \
  v[b] = rotr64(v[b] ^ v[c], 24);         \
  v[a] = v[a] + v[b] + (y);               \
  v[d] = rotr64(v[d] ^ v[a], 16);         \
  v[c] = v[c] + v[d];                     \
  v[b] = rotr64(v[b] ^ v[c], 63);
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    ZK_B2G(0, 4, 8, 12, m[S[r][0]], m[S[r][1]])
    ZK_B2G(1, 5, 9, 13, m[S[r][2]], m[S[r][3]])
    ZK_B2G(2, 6, 10, 14, m[S[r][4]], m[S[r][5]])
    ZK_B2G(3, 7, 11, 15, m[S[r][6]], m[S[r][7]])
    ZK_B2G(0, 5, 10, 15, m[S[r][8]], m[S[r][9]])
    ZK_B2G(1, 6, 11, 12, m[S[r][10]], m[S[r][11]])
    ZK_B2G(2, 7, 8, 13, m[S[r][12]], m[S[r][13]])
    ZK_B2G(3, 4, 9, 14, m[S[r][14]], m[S[r][15]])
  }
#undef ZK_B2G
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
  // from_bytes_wide: lo + hi * 2^256 mod r, as a Montgomery value
  Fr lo, hi;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo.l[2 * i] = (zk::u32)h[i];
    lo.l[2 * i + 1] = (zk::u32)(h[i] >> 32);
    hi.l[2 * i] = (zk::u32)h[4 + i];
    hi.l[2 * i + 1] = (zk::u32)(h[4 + i] >> 32);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {   // 2^256 < 6 r
    zk::fp_reduce_once<zk::FrP>(lo.l);
    zk::fp_reduce_once<zk::FrP>(hi.l);
  }
  // lo, hi canonical integers: (lo + hi 2^256) 2^256 = lo * R2 / R ... as Montgomery values: mont(lo) + mont(hi) * mont(2^256)
  const Fr r2 = Fr::r2();
  const Fr lom = zk::fp_mul<zk::FrP>(lo, r2);                        // lo in Montgomery form
  const Fr him = zk::fp_mul<zk::FrP>(zk::fp_mul<zk::FrP>(hi, r2), r2);   // (hi * 2^256) in Montgomery form
  return zk::fp_add<zk::FrP>(lom, him);
}
struct RngSeed {
  unsigned long long w[4];
};
// Blinding rows drawn by the kernel that writes the rest of the column (no launch of their own): row u + j of column c takes
// draw(ctr0 + c * ctr_col_stride + j) -- k_rng_fill's counter layout, so every value is the one k_rng_fill would store.
// on = 0: the kernel treats those rows as it does without blinding.
struct RngRows {
  RngSeed seed;
  unsigned long long ctr0, ctr_col_stride;
  int on;
};
__device__ __forceinline__ Fr rng_row(const RngRows &b, size_t col, size_t j) { return rng_draw(b.seed.w, b.ctr0 + col * b.ctr_col_stride + j); }
// A draw is one long dependent chain (about 8 us): a kernel whose threads own runs of rows must not draw a column's rows one after
// the other in the lane that owns them.  Such a kernel is launched with a few workgroups more -- [first_block, gridDim.x) -- which
// do what k_rng_fill does, one draw per thread, beside the workgroups that move the data:
// dst[c * col_stride + j] = draw of row j of column c, j < per_col.
__device__ __forceinline__ void rng_tail_blocks(const RngRows &b, unsigned first_block, Fr *__restrict__ dst, size_t per_col, size_t col_stride, size_t n_cols) {
  const size_t total = per_col * n_cols, T = (size_t)(gridDim.x - first_block) * blockDim.x;
  for (size_t g = (size_t)(blockIdx.x - first_block) * blockDim.x + threadIdx.x; g < total; g += T) {
    const size_t c = g / per_col, j = g - c * per_col;
    dst[c * col_stride + j] = rng_row(b, c, j);
  }
}
static inline unsigned rng_tail_grid(const RngRows &b, size_t draws, unsigned threads) { return b.on ? (unsigned)((draws + threads - 1) / threads) : 0u; }
// dst[c * col_stride + j] = draw(ctr0 + c * ctr_col_stride + j)   (Montgomery), j < per_col, c < n_cols
static __global__ void __launch_bounds__(256) k_rng_fill(RngSeed seed, unsigned long long ctr0, unsigned long long ctr_col_stride, Fr *__restrict__ dst,
                                                  size_t per_col, size_t col_stride, size_t n_cols) {
  const size_t total = per_col * n_cols;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t c = g / per_col, j = g - c * per_col;
    dst[c * col_stride + j] = rng_draw(seed.w, ctr0 + c * ctr_col_stride + j);
  }
}

// Canonical values of a column-contiguous table (pinned host memory mapped into the device, or device memory) -> Montgomery
// columns, rows >= u drawn from the blinding stream in the same pass: the upload of a witness phase in one launch.
static __global__ void __launch_bounds__(256) k_to_mont_blind(const Fr *__restrict__ src, Fr *__restrict__ dst, size_t n, unsigned u, size_t n_cols, RngRows blind) {
  const size_t total = n_cols * n;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t c = g / n, r = g - c * n;
    dst[g] = r >= u ? rng_row(blind, c, r - u) : zk::fr29_to_mont(src[g]);
  }
}
// The proof's staging ring (pinned, mapped) -> its device mirror, by a kernel: 16-byte units [0, n16) of src go to dst.  Every unit
// is read once, coalesced.  The same launch carries the public inputs into the instance column: inst_n canonical values (read from
// the ring) -> Montgomery, and inst_zero rows behind them back to zero (a shorter instance than the previous proof's).
static __global__ void __launch_bounds__(256) k_ring_flush(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16, const Fr *__restrict__ inst_src,
                                                    Fr *__restrict__ inst_dst, size_t inst_n, size_t inst_zero) {
  const size_t total = n16 + inst_n + inst_zero;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    if (g < n16) dst[g] = src[g];
    else if (g < n16 + inst_n) inst_dst[g - n16] = zk::fr29_to_mont(inst_src[g - n16]);
    else inst_dst[g - n16] = Fr::zero();
  }
}

static __global__ void __launch_bounds__(256) k_srs_den(const Fr *__restrict__ wpow, Fr s, Fr nn, Fr *__restrict__ out, size_t n) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = (s - wpow[i]) * nn;
}
static __global__ void __launch_bounds__(256) k_srs_li(const Fr *__restrict__ wpow, Fr snm1, Fr *__restrict__ inv_inout, size_t n) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) inv_inout[i] = wpow[i] * snm1 * inv_inout[i];
}
static __global__ void __launch_bounds__(256) k_fill_point(zk::G1Affine p, zk::G1Affine *__restrict__ out, size_t n) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = p;
}

// sigma_l[cell] = delta^(col of target) * omega^(row of target)
static __global__ void __launch_bounds__(256) k_sigma_values(const uint32_t *__restrict__ target, const Fr *__restrict__ dpow,
                                                      const Fr *__restrict__ wpow, Fr *__restrict__ out, size_t cells, int log_n) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= cells) return;
  const uint32_t t = target[i];
  out[i] = dpow[t >> log_n] * wpow[t & ((1u << log_n) - 1)];
}

// ------------------------------------------------------------------------------------------- grand products
struct PermArgs {
  const Fr *adv;      // [n_advice][n] Lagrange
  const Fr *constcol; // [n]
  const Fr *inst;     // [n]
  const Fr *sigma;    // [n_perm][n]
  const Fr *wpow;     // omega^i
  const Fr *beta_delta;  // [n_perm] beta * delta^c
  Fr beta, gamma;
  unsigned n_advice, n_perm, chunk, n_chunks;
  size_t n;
};
__device__ __forceinline__ const Fr *perm_col(const PermArgs &a, unsigned c) {
  return c < a.n_advice ? a.adv + (size_t)c * a.n : (c == a.n_advice ? a.constcol : a.inst);
}
// num[j][i] = prod_c (v_c + beta delta^c w^i + gamma), den[j][i] = prod_c (v_c + beta sigma_c + gamma)
static __global__ void __launch_bounds__(256) k_perm_num_den(PermArgs a, Fr *__restrict__ num, Fr *__restrict__ den) {
  const size_t total = (size_t)a.n_chunks * a.n;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const unsigned j = (unsigned)(g / a.n);
    const size_t i = g - (size_t)j * a.n;
    Fr nu = Fr::one(), de = Fr::one();
    const Fr w = a.wpow[i];
    for (unsigned c = j * a.chunk; c < (j + 1) * a.chunk && c < a.n_perm; ++c) {
      const Fr v = perm_col(a, c)[i];
      nu = nu * (v + a.beta_delta[c] * w + a.gamma);
      de = de * (v + a.beta * a.sigma[(size_t)c * a.n + i] + a.gamma);
    }
    num[g] = nu;
    den[g] = de;
  }
}
// lookup: num = (a + beta)(s + gamma), den = (a' + beta)(s' + gamma)
__device__ __forceinline__ void lookup_num_den_body(const Fr *__restrict__ a_cols, const Fr *__restrict__ table, const Fr *__restrict__ la, const Fr *__restrict__ ls,
                                                    const Fr &beta, const Fr &gamma, unsigned n_lookup, size_t n, Fr *__restrict__ num, Fr *__restrict__ den, unsigned blk,
                                                    unsigned nblk) {
  const size_t total = (size_t)n_lookup * n;
  const zk::Fr9S beta9 = zk::fr9_load(beta);
  const zk::Fr9C gamma9 = zk::fr9_load32(gamma);
  for (size_t g = blk * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)nblk * blockDim.x) {
    const size_t i = g % n;
    num[g] = zk::fr9_store(zk::fr9_lookup_term(zk::fr9_load(a_cols[g]), beta9, zk::fr9_lookup_sum(zk::fr9_load32(table[i]), gamma9)));
    den[g] = zk::fr9_store(zk::fr9_lookup_term(zk::fr9_load(la[g]), beta9, zk::fr9_lookup_sum(zk::fr9_load32(ls[g]), gamma9)));
  }
}
static __global__ void __launch_bounds__(256) k_lookup_num_den(const Fr *__restrict__ a_cols, const Fr *__restrict__ table, const Fr *__restrict__ la,
                                                        const Fr *__restrict__ ls, Fr beta, Fr gamma, unsigned n_lookup, size_t n,
                                                        Fr *__restrict__ num, Fr *__restrict__ den) {
  lookup_num_den_body(a_cols, table, la, ls, beta, gamma, n_lookup, n, num, den, blockIdx.x, gridDim.x);
}
// Side by side: the lookup ratios' two factors and, in the last workgroup, pout[i] = pstart * pbase^i (beta * delta^c: the
// permutation argument's constants).  Neither reads what the other writes; both start from the round's beta and gamma.  Grid: the
// workgroups of k_lookup_num_den (none when n_lookup == 0) + 1.
static __global__ void __launch_bounds__(256) k_lookup_num_den_powers(const Fr *__restrict__ a_cols, const Fr *__restrict__ table, const Fr *__restrict__ la,
                                                               const Fr *__restrict__ ls, Fr beta, Fr gamma, unsigned n_lookup, size_t n, Fr *__restrict__ num,
                                                               Fr *__restrict__ den, Fr pstart, Fr pbase, Fr *__restrict__ pout, size_t pn) {
  if (blockIdx.x + 1 == gridDim.x) powers_body(pstart, pbase, pout, pn, 0, 1);
  else lookup_num_den_body(a_cols, table, la, ls, beta, gamma, n_lookup, n, num, den, blockIdx.x, gridDim.x - 1);
}

// Exclusive running product per column: z[0] = 1, z[i+1] = z[i] * r[i] for i < u; z has u+1 defined entries.
// One workgroup of 1024 threads per column; thread t owns rows [t*per, (t+1)*per).  `total[col]` = z[u].  blind.on: the rows
// u + 1 .. n - 1 of the columns are their blinding rows, drawn by the workgroups behind the n_cols of the columns (rng_tail_blocks).
static __global__ void __launch_bounds__(1024) k_prefix_product(const Fr *__restrict__ ratio, Fr *__restrict__ z, Fr *__restrict__ total, size_t n,
                                                         unsigned u, unsigned n_cols, RngRows blind) {
  __shared__ Fr sh[1024];
  if (blockIdx.x >= n_cols) {
    rng_tail_blocks(blind, n_cols, z + u + 1, n - u - 1, n, n_cols);
    return;
  }
  const size_t col = blockIdx.x;
  const Fr *r = ratio + col * n;
  Fr *o = z + col * n;
  const unsigned per = (unsigned)((n + 1023) / 1024);
  const unsigned lo = threadIdx.x * per;
  // the runs and the scan on nine-limb values (csrc/fr9.hip.hpp): the running product S, every ratio read in the C form; the LDS
  // keeps packed canonical words
  zk::Lz<0, 1, 2> local = zk::lz_widen<0, 1, 2>(zk::fr9_one());
  for (unsigned k = 0; k < per; ++k) {
    const unsigned i = lo + k;
    if (i < u) local = zk::fr9_mul(local, zk::fr9_load32(r[i]));
  }
  sh[threadIdx.x] = zk::fr9_store(local);
  __syncthreads();
  // inclusive Hillis-Steele scan of the 1024 partial products
  for (unsigned d = 1; d < 1024; d <<= 1) {
    if (threadIdx.x >= d) local = zk::fr9_mul(local, zk::fr9_load32(sh[threadIdx.x - d]));
    __syncthreads();
    if (threadIdx.x >= d) sh[threadIdx.x] = zk::fr9_store(local);
    __syncthreads();
  }
  zk::Lz<0, 1, 2> acc = zk::lz_widen<0, 1, 2>(threadIdx.x ? zk::fr9_load(sh[threadIdx.x - 1]) : zk::fr9_one());  // product of everything before this thread's rows
  for (unsigned k = 0; k < per; ++k) {
    const unsigned i = lo + k;
    if (i <= u) o[i] = zk::fr9_store(acc);
    if (i < u) acc = zk::fr9_mul(acc, zk::fr9_load32(r[i]));
  }
  if (threadIdx.x == 1023) total[col] = sh[1023];
}
// Long columns (k >= 17): the column is cut into `segs` segments of `seg_len` rows, one workgroup each, so that a call fills the chip
// (at k = 19 one workgroup per column meant 100 workgroups walking 512 rows per thread twice: 3.2 ms per call).  Three launches:
// k_prefix_seg_totals (product of every segment), k_prefix_seg_scan (per column: exclusive scan of the segment products, `total[col]`),
// k_prefix_seg_apply (the running product inside a segment, started from its carry).  Same values as k_prefix_product: field
// multiplication is associative and the results are canonical.
static __global__ void __launch_bounds__(1024) k_prefix_seg_totals(const Fr *__restrict__ ratio, Fr *__restrict__ seg_total, size_t n, unsigned u, unsigned seg_len) {
  __shared__ Fr sh[1024];
  const size_t col = blockIdx.y;
  const unsigned seg = blockIdx.x, base = seg * seg_len;
  const Fr *r = ratio + col * n;
  const unsigned per = (seg_len + 1023) / 1024, lo = base + threadIdx.x * per;
  Fr local = Fr::one();
  for (unsigned k = 0; k < per; ++k) {
    const unsigned i = lo + k;
    if (i < u && i < base + seg_len) local = local * r[i];
  }
  sh[threadIdx.x] = local;
  __syncthreads();
  for (unsigned d = 512; d > 0; d >>= 1) {   // product reduction (order is irrelevant: commutative)
    if (threadIdx.x < d) sh[threadIdx.x] = sh[threadIdx.x] * sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) seg_total[col * gridDim.x + seg] = sh[0];
}
static __global__ void __launch_bounds__(64) k_prefix_seg_scan(Fr *__restrict__ seg_total, unsigned segs, unsigned n_cols, Fr *__restrict__ total) {
  const unsigned col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  Fr acc = Fr::one();
  for (unsigned s = 0; s < segs; ++s) {
    const Fr t = seg_total[(size_t)col * segs + s];
    seg_total[(size_t)col * segs + s] = acc;   // carry into segment s
    acc = acc * t;
  }
  total[col] = acc;
}
static __global__ void __launch_bounds__(1024) k_prefix_seg_apply(const Fr *__restrict__ ratio, const Fr *__restrict__ seg_carry, Fr *__restrict__ z, size_t n, unsigned u,
                                                            unsigned seg_len) {
  __shared__ Fr sh[1024];
  const size_t col = blockIdx.y;
  const unsigned seg = blockIdx.x, base = seg * seg_len, end = base + seg_len;
  const Fr *r = ratio + col * n;
  Fr *o = z + col * n;
  const unsigned per = (seg_len + 1023) / 1024, lo = base + threadIdx.x * per;
  Fr local = Fr::one();
  for (unsigned k = 0; k < per; ++k) {
    const unsigned i = lo + k;
    if (i < u && i < end) local = local * r[i];
  }
  sh[threadIdx.x] = local;
  __syncthreads();
  for (unsigned d = 1; d < 1024; d <<= 1) {
    Fr v = sh[threadIdx.x];
    Fr other = threadIdx.x >= d ? sh[threadIdx.x - d] : Fr::one();
    __syncthreads();
    if (threadIdx.x >= d) sh[threadIdx.x] = other * v;
    __syncthreads();
  }
  Fr acc = seg_carry[col * gridDim.x + seg];
  if (threadIdx.x) acc = acc * sh[threadIdx.x - 1];
  for (unsigned k = 0; k < per; ++k) {
    const unsigned i = lo + k;
    if (i >= end) break;
    if (i <= u) o[i] = acc;
    if (i < u) acc = acc * r[i];
  }
}
// Chunk carries of the permutation argument on the device (was: download the totals, multiply on the host, upload):
// carry[j] = prod_{i < j} total[i] in place, *closes = (the product of all of them == 1).  With check_ones every total itself
// has to be one (the lookup products) and the array is left alone.  One workgroup of 1024 threads; count <= 4096.
__device__ __forceinline__ void chunk_carry_body(Fr *__restrict__ total, unsigned count, int check_ones, int *__restrict__ closes) {
  __shared__ Fr sh[1024];
  __shared__ int bad;
  const unsigned t = threadIdx.x;
  if (t == 0) bad = 0;
  __syncthreads();
  const unsigned per = (count + 1023) / 1024, lo = t * per;
  if (check_ones) {
    const Fr one = Fr::one();
    for (unsigned k = 0; k < per; ++k)
      if (lo + k < count && !(total[lo + k] == one)) bad = 1;
    __syncthreads();
    if (t == 0) *closes = bad ? 0 : 1;
    return;
  }
  Fr vals[4];
  Fr local = Fr::one();
#pragma unroll
  for (unsigned k = 0; k < 4; ++k) {   // per <= 4; unrolled so that vals stays in registers
    vals[k] = k < per && lo + k < count ? total[lo + k] : Fr::one();
    local = local * vals[k];
  }
  sh[t] = local;
  __syncthreads();
  const unsigned active = (count + per - 1) / per;   // threads that hold totals: the scan stops once it spans them (66 chunks: 7 steps, not 10)
  for (unsigned d = 1; d < active; d <<= 1) {
    const Fr v = sh[t];
    const Fr other = t >= d ? sh[t - d] : Fr::one();
    __syncthreads();
    if (t >= d) sh[t] = other * v;
    __syncthreads();
  }
  Fr acc = t ? sh[t - 1] : Fr::one();
#pragma unroll
  for (unsigned k = 0; k < 4; ++k) {
    if (k < per && lo + k < count) total[lo + k] = acc;
    acc = acc * vals[k];
  }
  if (active == 0 ? t == 0 : t == active - 1) *closes = (active == 0 || sh[t] == Fr::one()) ? 1 : 0;   // the threads past it hold ones: sh[active - 1] is the product of all
}
static __global__ void __launch_bounds__(1024) k_chunk_carry(Fr *__restrict__ total, unsigned count, int check_ones, int *__restrict__ closes) {
  chunk_carry_body(total, count, check_ones, closes);
}
// Side by side, one workgroup each: the carries of total[0, n_carry) with closes[0], and the all-ones check of
// total[n_carry, n_carry + n_ones) with closes[1] (grid 2; grid 1 when there are no lookups)
static __global__ void __launch_bounds__(1024) k_chunk_carry_both(Fr *__restrict__ total, unsigned n_carry, unsigned n_ones, int *__restrict__ closes) {
  if (blockIdx.x == 0) chunk_carry_body(total, n_carry, 0, closes);
  else chunk_carry_body(total + n_carry, n_ones, 1, closes + 1);
}
// z[col][0..u] *= carry[col]
static __global__ void __launch_bounds__(256) k_scale_rows(Fr *__restrict__ z, const Fr *__restrict__ carry, size_t n, unsigned rows, unsigned n_cols) {
  const size_t total = (size_t)n_cols * rows;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const unsigned col = (unsigned)(g / rows);
    const unsigned i = (unsigned)(g - (size_t)col * rows);
    Fr *p = z + (size_t)col * n + i;
    *p = *p * carry[col];
  }
}

// ------------------------------------------------------------------------------------------- quotient
enum { QG_GATE = 0, QG_RLC = 1, QG_PERM_HEAD = 2, QG_PERM_C = 3, QG_PERM_D = 4, QG_LOOKUP = 5, QG_PERM_FIRST = 6, QG_PERM_LAST = 7 };
struct QGroup {
  int type, first, count, pad;
};
struct QArgs {
  const Fr *adv, *fix, *sig, *pz, *lz, *la, *ls, *inst, *lext, *xs;  // extended (coset-major) evaluations
  const Fr *beta_delta;                                               // [n_perm]
  const QGroup *groups;
  Fr *partials;  // [n_groups][4n]
  Fr y, beta, gamma, gamma_rlc;
  unsigned log_n, u, n_gate, n_rlc, adv_rlc0, fix_qrlc0, fix_const, fix_table, adv_lookup0, n_lookup, n_advice, n_perm, chunk, n_chunks;
  unsigned rows;  // cosets evaluated (3 or 4) = rows per column of every extended array (column stride rows * n)
  // the points of this launch: [pt0, pt0 + pt_count) of the rows * n (everything, or one coset row at a time when the rows'
  // shares are gathered across ranks while the next row is evaluated)
  size_t pt0, pt_count;
};

static __global__ void __launch_bounds__(256) k_quotient_partials(QArgs a) {
  const size_t n = (size_t)1 << a.log_n, ne = n * a.rows;
  const size_t p = a.pt0 + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (p >= a.pt0 + a.pt_count || p >= ne) return;
  const QGroup g = a.groups[blockIdx.y];
  const size_t row0 = p & ~(n - 1);           // k1 * n
  const size_t k2 = p & (n - 1);
  auto at = [&](const Fr *base, unsigned col, unsigned rot) -> Fr { return base[(size_t)col * ne + row0 + ((k2 + rot) & (n - 1))]; };
  // Nine-limb values throughout (csrc/fr9.hip.hpp): of every product one operand is read in the standard form (S: ld) and one in the
  // 2^261 form (C: ld32, the same word five bits up), the result is S; acc and the running products never leave limb form.
  auto ld = [&](const Fr *base, unsigned col, unsigned rot) { return zk::fr9_load(at(base, col, rot)); };
  auto ld32 = [&](const Fr *base, unsigned col, unsigned rot) { return zk::fr9_load32(at(base, col, rot)); };
  const zk::Fr9C y = zk::fr9_load32(a.y);
  zk::Lz<0, 1, 3> acc = zk::lz_widen<0, 1, 3>(zk::lz_zero());
  // acc * y + u * v with one Montgomery reduction (fr9_mul2): the Horner step of every expression; u is C, v is S
  auto horner = [&](const zk::Fr9C &u, const auto &v) { acc = zk::lz_widen<0, 1, 3>(zk::fr9_mul2(acc, y, u, v)); };
  switch (g.type) {
    case QG_GATE:
      for (int j = g.first; j < g.first + g.count; ++j) {
        const Fr q = at(a.fix, j, 0);
        if (!q.is_zero())
          horner(zk::fr9_load32(q), zk::fr9_norm(zk::lz_sub(zk::lz_add(ld(a.adv, j, 0), zk::fr9_mul(ld(a.adv, j, 1), ld32(a.adv, j, 2))), ld(a.adv, j, 3))));
        else acc = zk::lz_widen<0, 1, 3>(zk::fr9_mul(acc, y));
      }
      break;
    case QG_RLC: {
      const zk::Fr9C gamma_rlc = zk::fr9_load32(a.gamma_rlc);
      for (int j = g.first; j < g.first + g.count; ++j) {
        const unsigned col = a.adv_rlc0 + j;
        horner(ld32(a.fix, a.fix_qrlc0 + j, 0), zk::fr9_norm(zk::lz_sub(zk::lz_add(zk::fr9_mul(ld(a.adv, col, 0), gamma_rlc), ld(a.adv, col, 1)), ld(a.adv, col, 2))));
      }
      break;
    }
    case QG_PERM_HEAD: {
      const Fr zm = at(a.pz, a.n_chunks - 1, 0);
      acc = zk::lz_widen<0, 1, 3>(zk::fr9_mul(zk::fr9_load32(a.lext[p]), zk::lz_sub(zk::fr9_one(), ld(a.pz, 0, 0))));
      horner(zk::fr9_load32(a.lext[ne + p]), zk::lz_sub(zk::fr9_mul(zk::fr9_load(zm), zk::fr9_load32(zm)), zk::fr9_load(zm)));
      break;
    }
    case QG_PERM_FIRST:   // the two expressions of QG_PERM_HEAD as groups of their own (they belong to different ranks when the
      acc = zk::lz_widen<0, 1, 3>(zk::fr9_mul(zk::fr9_load32(a.lext[p]), zk::lz_sub(zk::fr9_one(), ld(a.pz, 0, 0))));   // quotient is sharded by column)
      break;
    case QG_PERM_LAST: {
      const Fr zm = at(a.pz, a.n_chunks - 1, 0);
      acc = zk::lz_widen<0, 1, 3>(zk::fr9_mul(zk::fr9_load32(a.lext[ne + p]), zk::lz_sub(zk::fr9_mul(zk::fr9_load(zm), zk::fr9_load32(zm)), zk::fr9_load(zm))));
      break;
    }
    case QG_PERM_C: {
      const zk::Fr9C l0 = zk::fr9_load32(a.lext[p]);
      for (int j = g.first; j < g.first + g.count; ++j) horner(l0, zk::lz_sub(ld(a.pz, j, 0), ld(a.pz, j - 1, a.u)));
      break;
    }
    case QG_PERM_D: {
      // a factor v + beta sigma + gamma is built in the C form (v, gamma read five bits up; beta and the thread's x turned to the
      // 2^266 form once, so that their products with the S values sigma and beta_delta[c] come out C): the running products stay S
      const zk::Fr9C lact = zk::fr9_load32(a.lext[2 * ne + p]), gamma = zk::fr9_load32(a.gamma);
      const zk::Lz<0, 1, 2> beta = zk::fr9_cc(zk::fr9_load32(a.beta)), x = zk::fr9_cc(zk::fr9_load32(a.xs[p]));
      for (int j = g.first; j < g.first + g.count; ++j) {
        zk::Lz<0, 1, 3> left = zk::lz_widen<0, 1, 3>(ld(a.pz, j, 1)), right = zk::lz_widen<0, 1, 3>(ld(a.pz, j, 0));
        for (unsigned c = j * a.chunk; c < (j + 1) * a.chunk && c < a.n_perm; ++c) {
          const zk::Fr9C v = zk::fr9_load32(c < a.n_advice ? at(a.adv, c, 0) : (c == a.n_advice ? at(a.fix, a.fix_const, 0) : a.inst[p]));
          left = zk::fr9_perm_step(left, zk::fr9_perm_factor(v, zk::fr9_mul(ld(a.sig, c, 0), beta), gamma));
          right = zk::fr9_perm_step(right, zk::fr9_perm_factor(v, zk::fr9_mul(zk::fr9_load(a.beta_delta[c]), x), gamma));
        }
        horner(lact, zk::lz_sub(left, right));
      }
      break;
    }
    case QG_LOOKUP: {
      const zk::Fr9C l0 = zk::fr9_load32(a.lext[p]), ll = zk::fr9_load32(a.lext[ne + p]), lact = zk::fr9_load32(a.lext[2 * ne + p]);
      const zk::Fr9C gamma = zk::fr9_load32(a.gamma);
      const zk::Fr9S beta = zk::fr9_load(a.beta), one = zk::fr9_one();
      const zk::Lz<0, 1, 64> s_gamma = zk::fr9_lookup_sum(ld32(a.fix, a.fix_table, 0), gamma);
      for (int i = g.first; i < g.first + g.count; ++i) {
        const Fr z0 = at(a.lz, i, 0), ap = at(a.la, i, 0), sp = at(a.ls, i, 0);
        const auto d = zk::lz_sub(zk::fr9_load(ap), zk::fr9_load(sp));   // ap - sp
        horner(l0, zk::lz_sub(one, zk::fr9_load(z0)));
        horner(ll, zk::lz_sub(zk::fr9_mul(zk::fr9_load(z0), zk::fr9_load32(z0)), zk::fr9_load(z0)));
        horner(lact, zk::fr9_mul2(ld32(a.lz, i, 1), zk::fr9_lookup_term(zk::fr9_load(ap), beta, zk::fr9_lookup_sum(zk::fr9_load32(sp), gamma)), zk::fr9_load32(z0),
                                  zk::lz_neg(zk::fr9_lookup_term(ld(a.adv, a.adv_lookup0 + i, 0), beta, s_gamma))));
        horner(l0, d);
        horner(lact, zk::fr9_mul(zk::lz_sub(zk::fr9_load32(ap), ld32(a.la, i, (unsigned)(n - 1))), d));
      }
      break;
    }
  }
  a.partials[(size_t)blockIdx.y * ne + p] = zk::fr9_store(acc);
}

// h_ext[p] = (sum_g ypow[g] * partials[g][p]) * zinv[k1]
static __global__ void __launch_bounds__(256) k_quotient_combine(const Fr *__restrict__ partials, const Fr *__restrict__ ypow, unsigned n_groups,
                                                          const Fr *__restrict__ zinv, unsigned log_n, unsigned rows, size_t pt0, size_t pt_count, Fr *__restrict__ h_ext) {
  const size_t n = (size_t)1 << log_n, ne = n * rows;
  const size_t p = pt0 + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (p >= pt0 + pt_count || p >= ne) return;
  // ypow and zinv come in the 2^261 form (constants of the call): nine-limb products, two groups per reduction, a lazy sum
  zk::F29 acc;
#pragma unroll
  for (int l = 0; l < 9; ++l) acc.l[l] = 0;
  unsigned g = 0;
  for (; g + 1 < n_groups; g += 2)
    acc = zk::fr29_weak_reduce(zk::f29_add(acc, zk::fr29_mul2(zk::fr29_unpack(partials[(size_t)g * ne + p]), zk::fr29_unpack(ypow[g]),
                                                             zk::fr29_unpack(partials[(size_t)(g + 1) * ne + p]), zk::fr29_unpack(ypow[g + 1]))));
  if (g < n_groups) acc = zk::fr29_weak_reduce(zk::f29_add(acc, zk::fr29_mul(zk::fr29_unpack(partials[(size_t)g * ne + p]), zk::fr29_unpack(ypow[g]))));
  h_ext[p] = zk::fr29_pack(zk::fr29_canonical(zk::fr29_mul(acc, zk::fr29_unpack(zinv[p >> log_n]))));
}

// Quotient from three cosets.  rows3[k1][i] = i-th coefficient (already scaled by 1/n) of h restricted to the coset
// g_k1 <w>, i.e. g_k1^i * sum_m h_m[i] c_k1^m with c_k1 = g_k1^n; pw[k1][i] = g_k1^-i; vinv = inverse of the 3x3
// Vandermonde matrix (c_k1^m).  h_c[m * n + i] = sum_k1 vinv[m][k1] * rows3[k1][i] * pw[k1][i]; the fourth piece is zero.
struct Mat3 {
  Fr v[9];
};
static __global__ void __launch_bounds__(256) k_ext3_combine(const Fr *__restrict__ rows3, const Fr *__restrict__ pw, Mat3 vinv, size_t n, Fr *__restrict__ h_c) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr t[3];
#pragma unroll
  for (int k1 = 0; k1 < 3; ++k1) t[k1] = rows3[(size_t)k1 * n + i] * pw[(size_t)k1 * n + i];
#pragma unroll
  for (int m = 0; m < 3; ++m) h_c[(size_t)m * n + i] = vinv.v[3 * m] * t[0] + vinv.v[3 * m + 1] * t[1] + vinv.v[3 * m + 2] * t[2];
  h_c[3 * n + i] = Fr::zero();
}

// ------------------------------------------------------------------------------------------- evaluations
// barycentric weights: d[r][i] = z_r - w^i (inverted by the caller), then b[r][i] = c * w^i * inv
__device__ __forceinline__ void bary_den_body(const Fr *__restrict__ wpow, const Fr *__restrict__ pts, unsigned n_pts, size_t n, Fr *__restrict__ out, unsigned blk,
                                              unsigned nblk) {
  const size_t total = (size_t)n_pts * n;
  for (size_t g = blk * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)nblk * blockDim.x)
    out[g] = pts[g / n] - wpow[g % n];
}
static __global__ void __launch_bounds__(256) k_bary_den(const Fr *__restrict__ wpow, const Fr *__restrict__ pts, unsigned n_pts, size_t n,
                                                  Fr *__restrict__ out) {
  bary_den_body(wpow, pts, n_pts, n, out, blockIdx.x, gridDim.x);
}
static __global__ void __launch_bounds__(256) k_bary_weights(const Fr *__restrict__ wpow, Fr c, size_t total, size_t n, Fr *__restrict__ inout) {
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x)
    inout[g] = inout[g] * wpow[g % n] * c;
}
// one workgroup per job: out[job][r] = sum_i col[i] * bw[rot_index[r]][i], up to 4 rotations per job
struct EvalJob {
  const Fr *col;
  int n_rot;
  int rot[4];  // indices into the weight table
};
// gridDim.y row slices (long columns): slice y sums rows [y n / Y, (y + 1) n / Y) into out[(y * jobs + job) * 4 + r]
static __global__ void __launch_bounds__(256) k_eval_jobs(const EvalJob *__restrict__ jobs, const Fr *__restrict__ bw /* 2^261 form: k_bary_weights with c * 32 */,
                                                          size_t n, Fr *__restrict__ out) {
  __shared__ Fr sh[256];
  const EvalJob job = jobs[blockIdx.x];
  // Nine-limb products (csrc/fr29.hip.hpp): the weights are the constant operand, stored in the 2^261 form, and two rows share one
  // Montgomery reduction (fr29_mul2); the accumulators stay below 2 r in limb form.  r < n_rot is tested inside fully unrolled
  // loops: with a loop bound read from the job the four accumulators were indexed dynamically and lived in scratch memory (144
  // bytes per lane; 5.4 ms of a k = 19 proof, 3.8 ms without the scratch, with the 8 x 32-bit product).
  zk::F29 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int l = 0; l < 9; ++l) acc[r].l[l] = 0;
  const size_t lo = (n / gridDim.y) * blockIdx.y, hi = blockIdx.y + 1 == gridDim.y ? n : lo + n / gridDim.y;
  size_t i = lo + threadIdx.x;
  for (; i + 256 < hi; i += 512) {
    const zk::F29 v0 = zk::fr29_unpack(job.col[i]), v1 = zk::fr29_unpack(job.col[i + 256]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < job.n_rot) {
        const Fr *w = bw + (size_t)job.rot[r] * n + i;
        acc[r] = zk::fr29_weak_reduce(zk::f29_add(acc[r], zk::fr29_mul2(v0, zk::fr29_unpack(w[0]), v1, zk::fr29_unpack(w[256]))));
      }
  }
  if (i < hi) {
    const zk::F29 v0 = zk::fr29_unpack(job.col[i]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < job.n_rot) acc[r] = zk::fr29_weak_reduce(zk::f29_add(acc[r], zk::fr29_mul(v0, zk::fr29_unpack(bw[(size_t)job.rot[r] * n + i]))));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r >= job.n_rot) break;
    sh[threadIdx.x] = zk::fr29_pack(zk::fr29_canonical(acc[r]));
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + r] = sh[0];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------- SHPLONK
// out[i] = sum_m s[m] * ptr[m][i].  The scalars are constants of the call, uploaded in the 2^261 form (zk_fr_to_29): nine-limb
// products, two columns per Montgomery reduction (fr29_mul2), the sum kept below 2 r in limb form (csrc/fr29.hip.hpp) -- these
// sums were 6 % of the summed kernel time of the k = 13 wave with the 8 x 32-bit product and an addition mod r per term.
static __device__ __forceinline__ Fr lincomb29(const Fr *const *__restrict__ ptrs, const Fr *__restrict__ s29, unsigned k0, unsigned k1, size_t i) {
  zk::F29 acc;
#pragma unroll
  for (int l = 0; l < 9; ++l) acc.l[l] = 0;
  unsigned k = k0;
  for (; k + 1 < k1; k += 2)
    acc = zk::fr29_weak_reduce(zk::f29_add(acc, zk::fr29_mul2(zk::fr29_unpack(ptrs[k][i]), zk::fr29_unpack(s29[k]), zk::fr29_unpack(ptrs[k + 1][i]), zk::fr29_unpack(s29[k + 1]))));
  if (k < k1) acc = zk::fr29_weak_reduce(zk::f29_add(acc, zk::fr29_mul(zk::fr29_unpack(ptrs[k][i]), zk::fr29_unpack(s29[k]))));
  return zk::fr29_pack(zk::fr29_canonical(acc));
}
// out[i] = the sum over the members [k0, k1) of the lists: the body of the plain kernel, of a chunk of the chunked one and of a job
__device__ __forceinline__ void lincomb_body(const Fr *const *__restrict__ ptrs, const Fr *__restrict__ s29, unsigned k0, unsigned k1, size_t n, Fr *__restrict__ out,
                                             unsigned blk, unsigned nblk) {
  for (size_t i = blk * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)nblk * blockDim.x) out[i] = lincomb29(ptrs, s29, k0, k1, i);
}
static __global__ void __launch_bounds__(256) k_lincomb_ptrs(const Fr *const *__restrict__ ptrs, const Fr *__restrict__ s29, unsigned m, size_t n,
                                                      Fr *__restrict__ out) {
  lincomb_body(ptrs, s29, 0, m, n, out, blockIdx.x, gridDim.x);
}
// the same sum split over blockIdx.y chunks of `per` pointers: partial[chunk][i]; k_sum_rows adds the chunks up.  One thread
// looping over ~600 columns is a 0.7 ms dependent chain; 13 chunks of 48 run side by side.
static __global__ void __launch_bounds__(256) k_lincomb_ptrs_chunked(const Fr *const *__restrict__ ptrs, const Fr *__restrict__ s29, unsigned m, unsigned per, size_t n,
                                                              Fr *__restrict__ partial) {
  const unsigned k0 = blockIdx.y * per, k1 = min(k0 + per, m);
  lincomb_body(ptrs, s29, k0, k1, n, partial + (size_t)blockIdx.y * n, blockIdx.x, gridDim.x);
}
__device__ __forceinline__ void sum_rows_body(const Fr *__restrict__ partial, unsigned rows, size_t n, Fr *__restrict__ out, unsigned blk, unsigned nblk) {
  for (size_t i = blk * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)nblk * blockDim.x) {
    Fr acc = partial[i];
    for (unsigned r = 1; r < rows; ++r) acc = acc + partial[(size_t)r * n + i];
    out[i] = acc;
  }
}
static __global__ void __launch_bounds__(256) k_sum_rows(const Fr *__restrict__ partial, unsigned rows, size_t n, Fr *__restrict__ out) {
  sum_rows_body(partial, rows, n, out, blockIdx.x, gridDim.x);
}
struct ShSet {
  Fr rc[4];    // r_j coefficients (ascending), unused ones zero
  Fr pts[4];   // points of S_j
  Fr vj;       // v^j
  Fr coef;     // v^j * Z_{T\S_j}(u)
  Fr r_u;      // r_j(u)
  int n_pts, pad[3];
};
// zs[j][i] = prod_{p in S_j} (w^i - p)
__device__ __forceinline__ void sh_zs_body(const ShSet *__restrict__ sets, unsigned n_sets, const Fr *__restrict__ wpow, size_t n, Fr *__restrict__ zs, unsigned blk,
                                           unsigned nblk) {
  const size_t total = (size_t)n_sets * n;
  for (size_t g = blk * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)nblk * blockDim.x) {
    const ShSet &s = sets[g / n];
    const Fr w = wpow[g % n];
    Fr acc = Fr::one();
    for (int t = 0; t < s.n_pts; ++t) acc = acc * (w - s.pts[t]);
    zs[g] = acc;
  }
}
static __global__ void __launch_bounds__(256) k_sh_zs(const ShSet *__restrict__ sets, unsigned n_sets, const Fr *__restrict__ wpow, size_t n,
                                               Fr *__restrict__ zs) {
  sh_zs_body(sets, n_sets, wpow, n, zs, blockIdx.x, gridDim.x);
}
// Side by side: every linear combination of a round in one launch.  blockIdx.y < n_jobs picks a job of the list that chain_jobs.hpp
// cuts (one per chunk of at most 48 members of a set): the k_lincomb_ptrs body over the members [first, first + m) of the round's
// pointer and scalar lists, into row `set` of `direct` (a set of one chunk) or into slot `slot` of `partial` (k_chain_sums adds a
// set's slots up).  The rows blockIdx.y >= n_jobs run, TAIL_ZS: the k_sh_zs body, TAIL_BARY: the k_bary_den body -- neither reads
// what a job writes.  `tab`: the ShSet records / the evaluation points, `count` of them.  TAIL_NONE: jobs only (gridDim.y == n_jobs).
// The launch takes the larger register count of its bodies: TAIL_ZS has 66 VGPRs, 7 waves per SIMD, where the jobs alone have 60 and
// 8 -- the prover uses it while the whole launch stays below 7 waves per SIMD, and TAIL_NONE with k_sh_zs behind it otherwise.
enum { TAIL_ZS = 0, TAIL_BARY = 1, TAIL_NONE = 2 };
template <int TAIL>
static __global__ void __launch_bounds__(256) k_chain_jobs(const chain::Job *__restrict__ jobs, unsigned n_jobs, const Fr *const *__restrict__ ptrs, const Fr *__restrict__ s29,
                                                    size_t n, Fr *__restrict__ direct, Fr *__restrict__ partial, const void *__restrict__ tab, unsigned count,
                                                    const Fr *__restrict__ wpow, Fr *__restrict__ tail_out) {
  if (blockIdx.y < n_jobs) {
    const chain::Job j = jobs[blockIdx.y];
    lincomb_body(ptrs, s29, j.first, j.first + j.m, n, j.slot < 0 ? direct + (size_t)j.set * n : partial + (size_t)j.slot * n, blockIdx.x, gridDim.x);
    return;
  }
  const unsigned blk = (blockIdx.y - n_jobs) * gridDim.x + blockIdx.x, nblk = (gridDim.y - n_jobs) * gridDim.x;
  if (TAIL == TAIL_ZS) sh_zs_body((const ShSet *)tab, count, wpow, n, tail_out, blk, nblk);
  else if (TAIL == TAIL_BARY) bary_den_body(wpow, (const Fr *)tab, count, n, tail_out, blk, nblk);
}
// direct[set] = the sum of the `chunks` slots of `partial` from `slot0` on, for the set blockIdx.y picks: k_sum_rows per chunked set
static __global__ void __launch_bounds__(256) k_chain_sums(const chain::Sum *__restrict__ sums, const Fr *__restrict__ partial, size_t n, Fr *__restrict__ direct) {
  const chain::Sum s = sums[blockIdx.y];
  sum_rows_body(partial + (size_t)s.slot0 * n, s.chunks, n, direct + (size_t)s.set * n, blockIdx.x, gridDim.x);
}
// hq[i] = sum_j v^j (F_j[i] - r_j(w^i)) * zs_inv[j][i]
static __global__ void __launch_bounds__(256) k_sh_h(const ShSet *__restrict__ sets, unsigned n_sets, const Fr *__restrict__ F, const Fr *__restrict__ zs_inv,
                                              const Fr *__restrict__ wpow, size_t n, Fr *__restrict__ hq) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const Fr w = wpow[i];
    Fr acc = Fr::zero();
    for (unsigned j = 0; j < n_sets; ++j) {
      const ShSet &s = sets[j];
      Fr r = s.rc[3];
      r = r * w + s.rc[2];
      r = r * w + s.rc[1];
      r = r * w + s.rc[0];
      acc = acc + s.vj * (F[(size_t)j * n + i] - r) * zs_inv[(size_t)j * n + i];
    }
    hq[i] = acc;
  }
}
// den[i] = w^i - u (inverted by the caller);  W[i] = (sum_j coef_j (F_j[i] - r_j(u)) - ztu * hq[i]) * inv[i]
static __global__ void __launch_bounds__(256) k_sh_den(const Fr *__restrict__ wpow, Fr u, size_t n, Fr *__restrict__ out) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = wpow[i] - u;
}
// the per-set constants of k_sh_w, by kernel argument (they depend on the last challenge: no table to send for them)
struct ShW {
  Fr coef[8], r_u[8];   // v^j * Z_{T\S_j}(u) and r_j(u), at most 8 rotation sets
};
static __global__ void __launch_bounds__(256) k_sh_w(ShW sets, unsigned n_sets, const Fr *__restrict__ F, const Fr *__restrict__ hq,
                                              Fr ztu, const Fr *__restrict__ inv, size_t n, Fr *__restrict__ W) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Fr acc = Fr::zero();
#pragma unroll
    for (unsigned j = 0; j < 8; ++j)   // unrolled: a run-time index into a kernel argument would put the struct into scratch memory
      if (j < n_sets) acc = acc + sets.coef[j] * (F[(size_t)j * n + i] - sets.r_u[j]);
    W[i] = (acc - ztu * hq[i]) * inv[i];
  }
}

}  // namespace zkp
