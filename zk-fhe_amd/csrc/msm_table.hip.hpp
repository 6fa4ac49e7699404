// The digit-multiple table path of the MSM (included by msm.hip alone, after msm_sort.hip.hpp and msm_bucket.hip.hpp): biased
// digits, the basis tables, k_msm_table and its fold, and the sparse sum.
#pragma once
#include "ctx.hpp"
#include "fr29.hip.hpp"
#include "g1x29_wave.hip.hpp"

namespace {
using namespace zk;

// ---- digit-multiple table path ---------------------------------------------------------------------------------------
// With T[(i*W + w)*J + j-1] = j * 2^(c*w) * P_i  (j = 1..J = 2^(c-1), W = ceil(255/c) signed windows) resident in HBM an MSM is
// a plain sum of at most n*W table points: no sort, no buckets, no weights, no doublings.  At n = 2^13, c = 12 the table is
// 23.6 GB of the 288 -- the SRS is fixed for the life of the prover, HBM is what this chip has most of.
struct BiasArg {
  u32 l[9];   // sum_w 2^(c*w + c-1): with it, window w of (s + bias) minus 2^(c-1) is a signed digit in [-J, J-1] and the digits
};            // sum to s without a carry chain; the zero windows of a short scalar stay zero digits

__device__ __forceinline__ u32 bits_at(const u32 (&l)[9], int bit, int c) {
  const int limb = bit >> 5, sh = bit & 31;
  u32 lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {   // selects, not indexed loads: the limbs stay in registers
    if (k == limb) lo = l[k];
    if (k == limb + 1) hi = l[k];
  }
  return (u32)((((u64)hi << 32) | lo) >> sh) & ((1u << c) - 1);
}

// W of a literal width (0: the width is an argument); windows a magnitude below 2^32 reaches, bias carry included
constexpr int table_windows(int c) { return c ? (255 + c - 1) / c : 0; }
constexpr int table_short_windows(int c) { return c ? (32 / c + 2 < table_windows(c) ? 32 / c + 2 : table_windows(c)) : 0; }

// the digit of window w when the width is a literal: after unrolling, limb index and shift are literals too -- a shift pair or a bit
// field extract and a mask, where bits_at selects among the nine limbs
template <int C>
__device__ __forceinline__ u32 digit_at(const u32 (&l)[9], int w) {
  const int bit = w * C, k = bit >> 5, sh = bit & 31;
  u32 v = l[k] >> sh;
  if (sh + C > 32) v |= l[k + 1] << (32 - sh);
  return v & ((1u << C) - 1);
}

// the scalar out of its Montgomery form, split into sign and magnitude (|s| < 2^253); returns the sign.  The nine-limb reduction gives
// s in [0, r] without a final subtraction (fr29.hip.hpp); (r - 1) / 2 - s borrows exactly when s is above the half, and r - r = 0.
__device__ __forceinline__ bool scalar_magnitude(const Fr &mont, Fr &s) {
  const u32 H[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};   // fr_gt_half's
  s = fr29_from_mont_weak(mont);
  u32 br = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) (void)zk_subc(H[k], s.l[k], br, &br);
  const bool neg = br != 0;
  if (neg) {
    br = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s.l[k] = zk_subc(FrP::MOD[k], s.l[k], br, &br);
  }
  return neg;
}

// |s| + bias; returns the sign, and in `bits` the bit length of |s|: windows above bits / c + 1 hold zero digits (a negative digit
// carries one into the next window, not further), that is the bias alone.  `high`: whether |s| has more than 32 bits.
__device__ __forceinline__ bool biased_scalar(const Fr &mont, const BiasArg &B, u32 (&out)[9], int &bits, bool &high) {
  Fr s;
  const bool neg = scalar_magnitude(mont, s);
  bits = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (s.l[k]) bits = 32 * k + 32 - __clz(s.l[k]);
  high = (s.l[1] | s.l[2] | s.l[3] | s.l[4] | s.l[5] | s.l[6] | s.l[7]) != 0;
  u32 carry = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const u64 v = (u64)s.l[k] + B.l[k] + carry;
    out[k] = (u32)v;
    carry = (u32)(v >> 32);
  }
  out[8] = B.l[8] + carry;
  return neg;
}

// One thread per (point, window) row: j * B for j = 1..J, each normalised on its own (a 40 us inversion per entry and lane;
// 369 M entries at n = 2^13, c = 12 -- a quarter of a second per basis, once).
__global__ void __launch_bounds__(64) k_basis_multiples(const G1Affine *__restrict__ bases, size_t n, int c, int W, G1Affine *__restrict__ T) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n * (size_t)W) return;
  const size_t i = t / (size_t)W;
  const int w = (int)(t % (size_t)W);
  const size_t J = (size_t)1 << (c - 1);
  G1Affine *row = T + t * J;
  G1Affine b = bases[i];
  if (!b.is_identity() && w) b = g1x_to_affine(g1x_mul_pow2(g1x_from_affine(b), c * w));
  if (b.is_identity()) {
    for (size_t j = 0; j < J; ++j) row[j] = b;
    return;
  }
  row[0] = g1_affine_to_29(b);   // stored in the 2^261 Montgomery form of the MSM kernels
  if (J == 1) return;
  G1X acc = g1x_from_affine_dbl(b);
  row[1] = g1_affine_to_29(g1x_to_affine(acc));
  for (size_t j = 2; j < J; ++j) {
    g1x_add_affine(acc, b, false);
    row[j] = g1_affine_to_29(g1x_to_affine(acc));
  }
}

// Work item = chunk of P <= 256 consecutive points of one column.  Every column has a chunk counter; a grid of persistent
// workgroups (three per CU) is spread over the columns, each draws chunks of its column until the counter runs out and then
// moves on to the next column that has chunks left -- a workgroup on a full-width column draws few chunks, one on a column of
// 0/1 cells many, and the accumulators live as long as the workgroup stays with a column (witness columns mix 0/1 cells,
// 8-bit range cells and full-width values: 0.5 to 22 additions per scalar).  Per chunk: the non-zero digits of the P
// scalars are compacted into an LDS list of table offsets (digit mask per thread, prefix sum over the workgroup), then
// the 256 threads take the list entries round-robin: every lane has the same number of mixed additions (+-1).
// Leaving a column, the workgroup appends to that column's partial list: with TREE one butterfly and one partial (calls of a
// few columns: thousands of short visits per column, the fold must stay short); without, every thread stores its accumulator
// as it is -- 256 partials per visit and no butterfly (eight dependent point additions with most lanes idle cost as much as
// eleven useful ones), and no point-addition code besides the loop's in the kernel: 168 VGPRs (three waves per SIMD; rocprof
// shows the arch / accumulation halves of the unified file), no scratch.  k_msm_table_fold sums the lists.
// C: the digit width as a literal for the widths msm.hip's table_kernel() names -- the window loop unrolled, every digit at a
// literal limb and shift, one extraction pass; the same entries in the same order as the run-time width C = 0 writes
// (profiles/msm_scalar_prep.md: the 136-column call of a k = 13 proof issues 4.2 % fewer VALU instructions, the 266-column call 12 %).
template <bool TREE, int C /* the table's digit width as a literal, 0: whatever c_arg says */>
__global__ void __launch_bounds__(256, TREE ? 1 : 3) k_msm_table(const Fr *__restrict__ scalars, size_t col_stride, size_t n, const G1Affine *__restrict__ T, int c_arg, int W_arg, BiasArg B,
                                                   unsigned P, unsigned cpc /* chunks per column */, unsigned n_cols, unsigned max_part,
                                                   G1X *__restrict__ partials /* [n_cols][max_part][TREE ? 1 : 256] */,
                                                   unsigned *__restrict__ n_part /* [n_cols] visits recorded, zero on entry */,
                                                   unsigned *__restrict__ col_next /* [n_cols] next chunk, zero on entry */,
                                                   unsigned *__restrict__ lists /* [gridDim.x][P * W] */, unsigned long long *__restrict__ adds) {
  const int c = C ? C : c_arg, W = C ? table_windows(C) : W_arg;
  // the entry list of the chunk in flight: in global memory (written and read by this workgroup only: it stays in this CU's
  // L1 / this XCD's L2), not in LDS -- with no LDS to its name the kernel shares a CU with the NTT tile kernel (147 KB of the
  // 160), whose waves wait on LDS while these issue multiply-adds
  unsigned *__restrict__ lst = lists + (size_t)blockIdx.x * P * (unsigned)W;
  __shared__ G1X sh[TREE ? 128 : 1];
  __shared__ unsigned wave_cnt[4], item_sh;
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = 1 << (c - 1);
  G1X29 acc = G1X29::identity();
  unsigned col = (unsigned)(((unsigned long long)blockIdx.x * n_cols) / gridDim.x), done = 0, total = 0;
  for (;;) {
    __syncthreads();   // the previous chunk's list is consumed
    if (threadIdx.x == 0) item_sh = atomicAdd(&col_next[col], 1u);
    __syncthreads();
    const unsigned chunk = item_sh;
    if (chunk >= cpc) {
      // this column has no chunks left: hand over what was summed, then look for the next column that has some
      if (done) {
        if (TREE) acc = block_sum_256(acc, sh);
        __syncthreads();
        if (threadIdx.x == 0) item_sh = atomicAdd(&n_part[col], 1u);
        __syncthreads();
        const size_t slot = (size_t)col * max_part + item_sh;
        if (TREE) {
          if (threadIdx.x == 0) partials[slot] = g1x29_store(acc);
        } else {
          partials[slot * 256 + threadIdx.x] = g1x29_store(acc);
        }
        acc = G1X29::identity();
        done = 0;
      }
      // next: the column with the most chunks left (not the neighbour: the workgroups would pile up on it for a chunk each,
      // and every visit costs the fold 256 additions)
      __syncthreads();
      if (threadIdx.x == 0) item_sh = 0;
      __syncthreads();
      // A column is joined only while it has at least MIN_JOIN chunks left (or has not been started): the last chunks of a
      // column stay with the workgroups that are on it.  Without the floor every idle workgroup of the call's tail jumped onto
      // the last busy columns for ONE chunk each -- up to 32 visits on a column of 32 chunks, and the fold's duration is that
      // of its longest column (measured: visits per column 6 on average, 30 at the maximum; 320 - 360 us per wide fold).
      // ... and among the columns that qualify every workgroup has its own order of preference (a hash of column and
      // workgroup): choosing "the column with the most chunks left" sent all workgroups that went idle at the same moment to the
      // same column.
      const unsigned MIN_JOIN = cpc < 4u ? cpc : 4u;
      unsigned best = 0;   // (preference << 12) | column, n_cols <= 4096
      for (unsigned j = threadIdx.x; j < n_cols; j += 256) {
        const unsigned nx = __hip_atomic_load(&col_next[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nx < cpc && (nx == 0 || cpc - nx >= MIN_JOIN)) {
          const unsigned h = ((j * 2654435761u) ^ (blockIdx.x * 40503u + 12345u) * 2246822519u) >> 13;   // 19 bits, never zero with the +1 below
          best = max(best, (((h & 0x7ffffu) + 1u) << 12) | j);
        }
      }
      if (best) atomicMax(&item_sh, best);
      __syncthreads();
      const unsigned found = item_sh;
      if (!found) break;
      col = found & 4095u;
      continue;
    }
    ++done;
    {
      const size_t i = (size_t)chunk * P + threadIdx.x;
      const bool valid = threadIdx.x < P && i < n;
      u32 sb[9];
      bool neg = false, high = false;
      int bits = 0;
      if (valid) neg = biased_scalar(scalars[(size_t)col * col_stride + i], B, sb, bits, high);
      // the windows with a non-zero digit, one bit each (W <= 32: c >= 8).  C != 0: one unrolled pass, every digit at a literal
      // position, and the same unrolled loop writes the entries after the prefix sum, predicated on the mask bit -- the digit is
      // derived again from its literal position (two instructions; holding seventeen of them would cost registers).  A window above
      // a short scalar holds the bias alone and tests as zero, so the bound of the run-time loop is not needed per lane; the wave
      // as a whole skips the windows that no magnitude below 2^32 reaches when none of its lanes has a longer one (two thirds of
      // a proof's scalars are 0/1 and range cells).
      constexpr int WS = table_short_windows(C), WC = table_windows(C);
      u32 mask = 0;
      bool wide = false;
      if constexpr (C != 0) {
        wide = __any(high) != 0;
        if (valid) {
#pragma unroll
          for (int w = 0; w < WS; ++w)
            if ((int)digit_at<C>(sb, w) != half) mask |= 1u << w;
          if (wide) {
#pragma unroll
            for (int w = WS; w < WC; ++w)
              if ((int)digit_at<C>(sb, w) != half) mask |= 1u << w;
          }
        }
      } else if (valid) {
        const int wtop = min(W, bits / c + 2);
        for (int w = 0; w < wtop; ++w)
          if ((int)bits_at(sb, w * c, c) != half) mask |= 1u << w;
      }
      const unsigned mine = (unsigned)__popc(mask);
      unsigned incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if ((int)lane >= d) incl += t;
      }
      if (lane == 63) wave_cnt[wv] = incl;
      __syncthreads();
      unsigned off = incl - mine;
      for (unsigned v = 0; v < wv; ++v) off += wave_cnt[v];
      // table offsets relative to the chunk's first point (31 bits + sign: P * W * 2^(c-1) <= 256 * 32 * 2^14; the whole table of a
      // 15-bit Lagrange half has more than 2^31 entries), in ascending order of the window within a thread
      const unsigned row0 = threadIdx.x * (unsigned)W;
      if constexpr (C != 0) {
        unsigned base = (row0 << (C - 1)) - 1u;   // |d| >= 1 comes on top
        // opaque, or base + (w << (C - 1)) is hoisted out of the chunk loop for every w: seventeen registers held across the
        // addition loop, 40 bytes of them in scratch
        asm volatile("" : "+v"(base));
        const u32 flip = neg ? 0x80000000u : 0u;
        auto entry = [&](int w) {
          if ((mask >> w) & 1u) {
            const int d = (int)digit_at<C>(sb, w) - half;
            lst[off++] = (base + ((unsigned)w << (C - 1)) + (unsigned)(d < 0 ? -d : d)) | (((u32)d ^ flip) & 0x80000000u);
          }
        };
#pragma unroll
        for (int w = 0; w < WS; ++w) entry(w);
        if (wide) {
#pragma unroll
          for (int w = WS; w < WC; ++w) entry(w);
        }
      } else {
        while (mask) {
          const int w = __builtin_ctz(mask);
          mask &= mask - 1;
          const int d = (int)bits_at(sb, w * c, c) - half;
          lst[off++] = (((row0 + (unsigned)w) << (c - 1)) + (unsigned)(d < 0 ? -d : d) - 1u) | ((neg != (d < 0)) ? 0x80000000u : 0u);
        }
      }
    }
    __syncthreads();
    const unsigned M = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    total += M;
    // software pipeline: the entry two steps ahead and the table point one step ahead are in flight during an addition
    const G1Affine *__restrict__ Tc = T + (((size_t)chunk * P * (size_t)W) << (c - 1));   // this chunk's rows of the table
    unsigned e = threadIdx.x, en = 0, en2 = 0;
    G1Affine p;
    if (e < M) {
      en = lst[e];
      p = Tc[en & 0x7fffffffu];
    }
    if (e + 256 < M) en2 = lst[e + 256];
    while (e < M) {
      const unsigned e2 = e + 256;
      unsigned en3 = 0;
      G1Affine p2;
      if (e2 < M) p2 = Tc[en2 & 0x7fffffffu];
      if (e2 + 256 < M) en3 = lst[e2 + 256];
      g1x29_add_affine(acc, g1a29_load(p), (en >> 31) != 0);
      e = e2;
      en = en2;
      en2 = en3;
      p = p2;
    }
  }
  if (adds && threadIdx.x == 0 && total) atomicAdd(adds, (unsigned long long)total);
}

// out[col] = sum of the column's partial list (n_part[col] * L entries), normalised; the counters go back to zero.
// 512 threads: with L = 256 (one accumulator per thread and visit) the two halves of the workgroup take the even and the odd
// visits -- a column of the wide calls collects 25 to 30 visits (every workgroup that drew a chunk of it), and the visits are
// the sequential part of this kernel: visits / 2 + 9 dependent point additions instead of visits + 8.  The next partial is in
// flight during an addition.
template <bool XYZZ>
__global__ void __launch_bounds__(512) k_msm_table_fold(const G1X *__restrict__ partials, unsigned max_part, unsigned L, unsigned *__restrict__ n_part,
                                                        unsigned *__restrict__ col_next, void *__restrict__ out) {
  __shared__ G1X sh[256];
  const unsigned col = blockIdx.x, t = threadIdx.x & 255u, q = threadIdx.x >> 8;
  const unsigned np = n_part[col] * L;
  const G1X *mine = partials + (size_t)col * max_part * L;
  G1X29 f = G1X29::identity();
  {
    // L = 256: entry v * 256 + t, v = q, q + 2, ...; L = 1: entries threadIdx.x, threadIdx.x + 512, ...
    const unsigned first = L == 256 ? q * 256u + t : threadIdx.x, step = 512u;
    unsigned b = first;
    G1X cur;
    if (b < np) cur = mine[b];
    while (b < np) {
      const unsigned nb = b + step;
      G1X nxt;
      if (nb < np) nxt = mine[nb];
      g1x29_add(f, g1x29_load(cur));
      cur = nxt;
      b = nb;
    }
  }
  // 512 -> 256 -> 128 -> 64 through LDS, then a butterfly in the first wave
  if (q == 1) sh[t] = g1x29_store(f);
  __syncthreads();
  if (q == 0) g1x29_add(f, g1x29_load(sh[t]));
  __syncthreads();
  if (q == 0 && t >= 128) sh[t - 128] = g1x29_store(f);
  __syncthreads();
  if (q == 0 && t < 128) g1x29_add(f, g1x29_load(sh[t]));
  __syncthreads();
  if (q == 0 && t >= 64 && t < 128) sh[t - 64] = g1x29_store(f);
  __syncthreads();
  if (threadIdx.x < 64) {
    g1x29_add(f, g1x29_load(sh[t]));
    for (int m = 1; m < 64; m <<= 1) {
      const G1X29 other = g1x_shfl_xor(f, m);
      g1x29_add(f, other);
    }
    if (threadIdx.x == 0) {
      if (XYZZ) ((G1X *)out)[col] = g1x29_to_std(f);   // normalised by the caller, a round's points at a time
      else ((G1Affine *)out)[col] = g1x_to_affine(g1x29_to_std(f));
      n_part[col] = 0;
      col_next[col] = 0;
    }
  }
}

// table[w][i] = 2^(c*w) * P_i
__global__ void __launch_bounds__(256) k_basis_table(const G1Affine *__restrict__ bases, size_t n, int c, int windows,
                                                     G1Affine *__restrict__ table) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p = bases[i];
  table[i] = g1_affine_to_29(p);   // the tables hold the 2^261 Montgomery form of the MSM kernels (fq29.hip.hpp)
  G1X cur = g1x_from_affine(p);
  for (int w = 1; w < windows; ++w) {
    cur = g1x_mul_pow2(cur, c);
    G1Affine a = g1x_to_affine(cur);
    table[(size_t)w * n + i] = g1_affine_to_29(a);
    cur = g1x_from_affine(a);
  }
}

// A handful of non-zero scalars against a basis with a digit-multiple table: out[slot] = sum over the cells of that slot of
// scalar * P_row.  One wave per slot, lanes over the windows, a butterfly, one normalisation.  (The prover's early
// phase-1 commitment: the 16 challenge-dependent gate cells of the constrain_mul gates, as corrections to <= 4 columns.)
template <bool XYZZ>
__global__ void __launch_bounds__(64) k_msm_sparse(const zkfhe_sparse_term *__restrict__ terms, unsigned n_terms, const G1Affine *__restrict__ T, int c, int W,
                                                   BiasArg B, void *__restrict__ out) {
  const unsigned slot = blockIdx.x, lane = threadIdx.x;
  const int half = 1 << (c - 1);
  G1X29 acc = G1X29::identity();
  for (unsigned t = 0; t < n_terms; ++t) {
    if (terms[t].slot != slot) continue;
    Fr s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.l[2 * i] = (u32)terms[t].scalar.l[i];
      s.l[2 * i + 1] = (u32)(terms[t].scalar.l[i] >> 32);
    }
    u32 sb[9];
    int bits;
    bool high;
    const bool neg = biased_scalar(s, B, sb, bits, high);
    const int d = (int)lane < W ? (int)bits_at(sb, (int)lane * c, c) - half : 0;   // window = lane (W <= 64)
    if (d) {
      const G1Affine p = T[(((size_t)terms[t].row * W + lane) << (c - 1)) + (size_t)(d < 0 ? -d : d) - 1];
      g1x29_add_affine(acc, g1a29_load(p), neg != (d < 0));
    }
  }
  for (int m = 1; m < 64; m <<= 1) {
    const G1X29 other = g1x_shfl_xor(acc, m);
    g1x29_add(acc, other);
  }
  if (lane == 0) {
    if (XYZZ) ((G1X *)out)[slot] = g1x29_to_std(acc);
    else ((G1Affine *)out)[slot] = g1x_to_affine(g1x29_to_std(acc));
  }
}

}  // namespace
