// MSM bucket pipeline, stages 2 to 4 (included by msm.hip alone): the task list, accumulation, merge and the bucket reductions.
#pragma once
#include "ctx.hpp"
#include "g1x29_wave.hip.hpp"
#include "msm_plan.hpp"

namespace {
using namespace zk;

// ---- bounded-length accumulation tasks -------------------------------------------------------------
// A bucket with cnt entries is cut into ceil(cnt / TASK_E) tasks; one thread sums one task (<= TASK_E mixed
// additions), so the longest dependent chain in the kernel no longer depends on how skewed a column is
// (witness columns hold thousands of 0/1 cells).  k_msm_task_count: tasks per column; k_msm_task_fill:
// the task list (bucket id, slice); k_msm_accumulate: one thread per task -> partial sum;
// k_msm_merge: one thread per bucket adds its partials (few), buckets with many partials go to a wave each.
// The task length is chosen per basis geometry (msm_task_len, msm_plan.hpp): ~1/5 of the bucket load of a full-width column.

// Slices of a bucket with cnt entries: nt = ceil(cnt / E) slices, the first r = cnt % nt of length a + 1, the others of
// length a = cnt / nt.  The task list is ordered by slice length, longest first (counting sort over the E length
// classes): the 64 lanes of a wave then run chains of the SAME length -- with the bucket-ordered list a wave mixed
// lengths between E/2 and E and idled behind its longest lane (measured: 54 % of the modmul peak at E = 32 against
// 85 % at E = 8, where slices are nearly equal but every bucket costs five partials in the merge).
struct Slices {
  unsigned nt, a, r;
};
__device__ __forceinline__ Slices slices_of(unsigned cnt, unsigned TASK_E) {
  Slices s;
  s.nt = (cnt + TASK_E - 1) / TASK_E;
  s.a = s.nt ? cnt / s.nt : 0;
  s.r = s.nt ? cnt - s.a * s.nt : 0;
  return s;
}
// position of partial j of a bucket in the task / partial arrays
__device__ __forceinline__ unsigned partial_pos(const Slices &s, unsigned posA, unsigned posB, unsigned j) { return j < s.r ? posA + j : posB + (j - s.r); }

// zero the bucket histogram and the heavy-bucket counter of a call (one launch instead of two runtime fills)
__global__ void __launch_bounds__(256) k_msm_clear(unsigned *__restrict__ hist, size_t words, unsigned *__restrict__ heavy_count) {
  const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i0 < 4) heavy_count[i0] = 0;
  for (size_t i = i0; i < words; i += (size_t)gridDim.x * blockDim.x) hist[i] = 0;
}

// per column: number of slices of every length
__global__ void __launch_bounds__(256) k_msm_task_count(const unsigned *__restrict__ off, unsigned K, unsigned TASK_E, unsigned *__restrict__ col_hist /* [n_cols][TASK_BINS] */) {
  __shared__ unsigned h[TASK_BINS];
  for (unsigned i = threadIdx.x; i < TASK_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const unsigned *o = off + (size_t)blockIdx.x * (K + 1);
  for (unsigned b = threadIdx.x; b < K; b += 256) {
    const Slices s = slices_of(o[b + 1] - o[b], TASK_E);
    if (!s.nt) continue;
    if (s.r) atomicAdd(&h[s.a + 1], s.r);
    atomicAdd(&h[s.a], s.nt - s.r);
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < TASK_BINS; i += 256) col_hist[(size_t)blockIdx.x * TASK_BINS + i] = h[i];
}
// first task of every (length, column): lengths descending, columns ascending inside a length.  One block of 128 threads.
__global__ void __launch_bounds__(128) k_msm_task_colscan(const unsigned *__restrict__ col_hist, unsigned n_cols, unsigned *__restrict__ col_base /* [n_cols][TASK_BINS] */,
                                                          unsigned *__restrict__ n_tasks) {
  __shared__ unsigned bin_total[TASK_BINS], bin_base[TASK_BINS];
  const unsigned L = threadIdx.x;
  if (L < TASK_BINS) {
    unsigned s = 0;
    for (unsigned c = 0; c < n_cols; ++c) s += col_hist[(size_t)c * TASK_BINS + L];
    bin_total[L] = s;
  }
  __syncthreads();
  if (L == 0) {
    unsigned acc = 0;
    for (int l = (int)TASK_BINS - 1; l >= 0; --l) {
      bin_base[l] = acc;
      acc += bin_total[l];
    }
    *n_tasks = acc;
  }
  __syncthreads();
  if (L < TASK_BINS) {
    unsigned acc = bin_base[L];
    for (unsigned c = 0; c < n_cols; ++c) {
      col_base[(size_t)c * TASK_BINS + L] = acc;
      acc += col_hist[(size_t)c * TASK_BINS + L];
    }
  }
}
// per column: hand out the positions (LDS cursors per length class) and write the task list
__global__ void __launch_bounds__(256) k_msm_task_fill(const unsigned *__restrict__ off, unsigned K, unsigned TASK_E, const unsigned *__restrict__ col_base,
                                                       unsigned *__restrict__ bucket_posA, unsigned *__restrict__ bucket_posB /* [n_cols][K] each */,
                                                       uint2 *__restrict__ tasks, unsigned *__restrict__ heavy_count /* [0] medium, [1] large */,
                                                       unsigned *__restrict__ medium_list, unsigned *__restrict__ large_list, unsigned heavy_cap) {
  __shared__ unsigned cur[TASK_BINS];
  const size_t col = blockIdx.x;
  for (unsigned i = threadIdx.x; i < TASK_BINS; i += 256) cur[i] = col_base[col * TASK_BINS + i];
  __syncthreads();
  const unsigned *o = off + col * (K + 1);
  for (unsigned b = threadIdx.x; b < K; b += 256) {
    const Slices s = slices_of(o[b + 1] - o[b], TASK_E);
    if (!s.nt) continue;
    const unsigned g = (unsigned)(col * K + b);
    const unsigned posA = s.r ? atomicAdd(&cur[s.a + 1], s.r) : 0u;
    const unsigned posB = atomicAdd(&cur[s.a], s.nt - s.r);
    bucket_posA[g] = posA;
    bucket_posB[g] = posB;
    if (s.nt > (unsigned)MERGE_LIGHT) {   // the merge kernel's block ranges for buckets with many partials
      const bool large = s.nt > MERGE_MEDIUM;
      const unsigned slot = atomicAdd(&heavy_count[large ? 1 : 0], 1u);
      if (slot < heavy_cap) (large ? large_list : medium_list)[slot] = g;
    }
    for (unsigned j = 0; j < s.r; ++j) tasks[posA + j] = make_uint2(g, j);
    for (unsigned j = s.r; j < s.nt; ++j) tasks[posB + (j - s.r)] = make_uint2(g, j);
  }
}

// 16-byte load of four consecutive entry words at a 4-byte aligned address (the entry array is padded by 32 bytes)
__device__ __forceinline__ uint4 ld_entries(const unsigned *p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

__global__ void __launch_bounds__(256) k_msm_accumulate(const uint2 *__restrict__ tasks, const unsigned *__restrict__ n_tasks_ptr,
                                                        const unsigned *__restrict__ off, const unsigned *__restrict__ entries,
                                                        size_t col_entries, const G1Affine *__restrict__ table, unsigned K, unsigned TASK_E,
                                                        G1X *__restrict__ partials) {
  const unsigned n_tasks = *n_tasks_ptr;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n_tasks; t += (size_t)gridDim.x * blockDim.x) {
    const uint2 tk = tasks[t];
    const size_t col = tk.x / K;
    const unsigned b = tk.x - (unsigned)col * K;
    const unsigned *o = off + col * (K + 1);
    const Slices s = slices_of(o[b + 1] - o[b], TASK_E);
    const unsigned lo = o[b] + (tk.y < s.r ? tk.y * (s.a + 1) : tk.y * s.a + s.r);
    const unsigned hi = lo + s.a + (tk.y < s.r ? 1u : 0u);
    const unsigned *e = entries + col * col_entries;
    // software pipeline: the table gather of entry k+1 is in flight while entry k is added (PMC showed 40 % of the wave
    // cycles of the plain loop waiting on this dependent load chain).  The entry indices themselves come in 16-byte
    // loads into an 8-entry shift window: with one 4-byte load per entry and lanes 4*E bytes apart, every lane pulled
    // its own cache line through L1 once per entry.
    G1X29 acc = G1X29::identity();
    const unsigned *ep = e + lo;
    uint4 w0 = ld_entries(ep), w1 = ld_entries(ep + 4);
    unsigned valid = 8;
    G1Affine p = table[w0.x & 0x7fffffffu];
    const unsigned cnt_e = hi - lo;
    for (unsigned i = 0; i < cnt_e; ++i) {
      const unsigned en = w0.x, en1 = w0.y;
      G1Affine pn = p;
      if (i + 1 < cnt_e) pn = table[en1 & 0x7fffffffu];
      g1x29_add_affine(acc, g1a29_load(p), (en >> 31) != 0);
      p = pn;
      w0.x = w0.y, w0.y = w0.z, w0.z = w0.w, w0.w = w1.x;
      w1.x = w1.y, w1.y = w1.z, w1.z = w1.w;
      if (--valid == 4) {
        w1 = ld_entries(ep + i + 5);   // entries i+5 .. i+8 of the slice (window now starts at i+1)
        valid = 8;
      }
    }
    partials[t] = g1x29_store(acc);
  }
}

// bucket sum = sum of its partials, ONE launch with three block ranges that run side by side (they used to be two
// kernels and two loops, one after the other: 650 us of dependent chains per call):
//   large_blocks: skewed witness columns (thousands of 0/1 cells in one bucket): one wave per bucket, 6-step tree;
//   medium_blocks: buckets with <= MERGE_MEDIUM partials -- every column has ~2^(254 mod c) of them, the narrow top
//     window piles its digits onto them -- eight lanes per bucket, lanes stride over the partials, 3-step butterfly;
//   the rest: one thread per bucket with <= MERGE_LIGHT partials (every bucket of a full-width column).
// The medium / large lists are written by k_msm_task_fill.
__global__ void __launch_bounds__(256) k_msm_merge(const unsigned *__restrict__ off, const unsigned *__restrict__ bucket_posA, const unsigned *__restrict__ bucket_posB,
                                                   const G1X *__restrict__ partials, unsigned K, unsigned TASK_E, size_t n_cols, G1X *__restrict__ buckets,
                                                   const unsigned *__restrict__ heavy_count, const unsigned *__restrict__ medium_list,
                                                   const unsigned *__restrict__ large_list, unsigned heavy_cap, unsigned large_blocks, unsigned medium_blocks) {
  // block order = dispatch order: the long chains (large, then medium) go first, the light range fills the chip behind them
  const unsigned lane = threadIdx.x & 63;
  if (blockIdx.x < large_blocks) {
    unsigned cnt = heavy_count[1];
    if (cnt > heavy_cap) cnt = heavy_cap;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned n_waves = (large_blocks * blockDim.x) >> 6;
    for (unsigned h = wave; h < cnt; h += n_waves) {
      const size_t g = large_list[h];
      const size_t col = g / K;
      const unsigned b = (unsigned)(g - col * K);
      const unsigned *o = off + col * (K + 1);
      const Slices s = slices_of(o[b + 1] - o[b], TASK_E);
      const unsigned nt = s.nt;
      const unsigned pa = bucket_posA[g], pb = bucket_posB[g];
      G1X29 acc = G1X29::identity();
      for (unsigned j = lane; j < nt; j += 64) g1x29_add(acc, g1x29_load(partials[partial_pos(s, pa, pb, j)]));
      for (int d = 32; d > 0; d >>= 1) {
        const G1X29 other = g1x_shfl_down(acc, d);
        if ((int)lane < d) g1x29_add(acc, other);
      }
      if (lane == 0) buckets[g] = g1x29_store(acc);
    }
    return;
  }
  if (blockIdx.x < large_blocks + medium_blocks) {
    unsigned cnt = heavy_count[0];
    if (cnt > heavy_cap) cnt = heavy_cap;
    const unsigned wave = ((blockIdx.x - large_blocks) * blockDim.x + threadIdx.x) >> 6;
    const unsigned n_waves = (medium_blocks * blockDim.x) >> 6;
    for (unsigned base = wave * 8; base < cnt; base += n_waves * 8) {
      const unsigned h = base + (lane >> 3), sub = lane & 7;
      size_t g = 0;
      unsigned nt = 0, pa = 0, pb = 0;
      Slices s = {0, 0, 0};
      if (h < cnt) {
        g = medium_list[h];
        const size_t col = g / K;
        const unsigned b = (unsigned)(g - col * K);
        const unsigned *o = off + col * (K + 1);
        s = slices_of(o[b + 1] - o[b], TASK_E);
        nt = s.nt;
        pa = bucket_posA[g];
        pb = bucket_posB[g];
      }
      G1X29 acc = G1X29::identity();
      for (unsigned j = sub; j < nt; j += 8) g1x29_add(acc, g1x29_load(partials[partial_pos(s, pa, pb, j)]));
      for (int m = 1; m < 8; m <<= 1) {
        const G1X29 other = g1x_shfl_xor(acc, m);
        g1x29_add(acc, other);
      }
      if (nt && sub == 0) buckets[g] = g1x29_store(acc);
    }
    return;
  }
  const unsigned first = large_blocks + medium_blocks, light_blocks = gridDim.x - first;
  const size_t total = (size_t)K * n_cols;
  for (size_t g = (blockIdx.x - first) * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)light_blocks * blockDim.x) {
    const size_t col = g / K;
    const unsigned b = (unsigned)(g - col * K);
    const unsigned *o = off + col * (K + 1);
    const Slices s = slices_of(o[b + 1] - o[b], TASK_E);
    const unsigned nt = s.nt;
    if (nt > (unsigned)MERGE_LIGHT) continue;
    G1X first = G1X::identity();
    if (nt) {
      const unsigned pa = bucket_posA[g], pb = bucket_posB[g];
      first = partials[partial_pos(s, pa, pb, 0)];
      if (nt > 1) {
        G1X29 acc = g1x29_load(first);
        G1X nxt = partials[partial_pos(s, pa, pb, 1)];
        for (unsigned j = 1; j < nt; ++j) {  // the load of partial j+1 is in flight while partial j is added
          const G1X cur = nxt;
          if (j + 1 < nt) nxt = partials[partial_pos(s, pa, pb, j + 1)];
          g1x29_add(acc, g1x29_load(cur));
        }
        first = g1x29_store(acc);
      }
    }
    buckets[g] = first;
  }
}

__device__ __forceinline__ G1X g1x_mul_pow2(G1X p, int k) {
  for (int i = 0; i < k; ++i) p = g1x_dbl(p);
  return p;
}
__device__ __forceinline__ G1X29 g1x29_mul_pow2(G1X29 p, int k) {
  for (int i = 0; i < k; ++i) p = g1x29_dbl(p);
  return p;
}

// ---- fast bucket reduction for 64 <= K <= 32768 -------------------------------------------------------
// bucket index idx = 64 a + b carries weight idx + 1, so
//     sum (idx+1) B = 64 * sum_a a R_a  +  sum_b (b+1) C_b ,   R_a = sum_b B[a][b],  C_b = sum_a B[a][b].
// k_msm_marginals: L lanes per row / column sum -- every lane adds up to 64/L buckets serially, then a butterfly over
// the L lanes.  L = 8 for calls with many columns (1.4 lane-additions per bucket and marginal instead of the 6 of a
// whole-wave butterfly), L = 64 for calls of a few columns (shortest dependent chain).  lane = sub * 8 + g: the 8 outputs of a wave sit in the low lane bits so that column sums read
// consecutive buckets across lanes.
// k_msm_weighted: two waves per MSM; lane a forms a * R_a by double-and-add (<= 7 bits) and a 6-step butterfly sums
// the lanes; then one lane normalises.
__global__ void __launch_bounds__(256) k_msm_marginals(const G1X *__restrict__ buckets, unsigned K, size_t n_cols, unsigned L /* lanes per output: 8 or 64 */,
                                                       unsigned w0, unsigned w_cnt /* outputs w0 .. w0 + w_cnt - 1 of every column */,
                                                       G1X *__restrict__ marg /* [n_cols][A + 64] */) {
  const unsigned A = K >> 6;
  const unsigned per_col = A + 64;
  const unsigned G = 64 / L;  // outputs per wave
  const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
  const unsigned lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
  const size_t o = wave * G + g;  // output index over all columns, within the [w0, w0 + w_cnt) slice
  const bool live = o < n_cols * w_cnt;
  const size_t col = live ? o / w_cnt : 0;
  const unsigned w = w0 + (unsigned)(o - col * w_cnt);
  const G1X *B = buckets + col * K;
  size_t base, stride;
  unsigned cnt;
  if (w < A) {  // row w: buckets w*64 + sub + L i
    base = (size_t)w * 64 + sub;
    stride = L;
    cnt = 64 / L;
  } else {      // column w - A: buckets (sub + L i) * 64 + (w - A)
    base = (size_t)sub * 64 + (w - A);
    stride = (size_t)L * 64;
    cnt = A > sub ? (A - sub + L - 1) / L : 0;
  }
  if (!live) cnt = 0;
  G1X29 v = G1X29::identity();
  for (unsigned i = 0; i < cnt; ++i) g1x29_add(v, g1x29_load(B[base + i * stride]));
  for (int m = (int)G; m < 64; m <<= 1) {
    const G1X29 other = g1x_shfl_xor(v, m);
    g1x29_add(v, other);
  }
  if (live && sub == 0) marg[col * per_col + w] = g1x29_store(v);
}

// one block per MSM: waves 0 .. ceil(A/64)-1 weight the row sums (64 a * R_a), the last wave the column sums ((b+1) * C_b).
// Every lane runs a double-and-add over exactly the bits its wave needs (log2 A for the rows, 7 for the columns); the row
// lanes then double six more times (the factor 64) while the column wave is still busy, so that after the butterflies one
// lane only adds the wave sums and normalises: 30 dependent point operations at K = 4096, 26 at K = 512 (it was 37).
// XYZZ: the sum leaves the kernel as it is (128 B, standard Montgomery form) and the caller normalises a whole round's points with
// one inversion on the host (zkfhe_g1_xyzz_to_affine) -- the 40 us Bernstein-Yang inversion of one lane is the tail of every call.
template <bool XYZZ>
__global__ void __launch_bounds__(576) k_msm_weighted(const G1X *__restrict__ marg, unsigned K, void *__restrict__ out) {
  __shared__ G1X sh[9];
  const unsigned A = K >> 6;
  const unsigned row_waves = (A + 63) / 64;
  const size_t col = blockIdx.x;
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const G1X *M = marg + col * (A + 64);
  const bool rows = wv < row_waves;
  const unsigned a = wv * 64 + lane;
  const G1X29 P = g1x29_load(rows ? (a < A ? M[a] : G1X::identity()) : M[A + lane]);
  const unsigned k = rows ? a : lane + 1;  // weights a (rows, times 64 below) and b + 1 (columns)
  int nbits = 7;
  if (rows) {
    nbits = 0;
    while ((1u << nbits) < A) ++nbits;
  }
  G1X29 W = G1X29::identity();
  for (int bit = nbits - 1; bit >= 0; --bit) {
    W = g1x29_dbl(W);
    if ((k >> bit) & 1) g1x29_add(W, P);
  }
  if (rows) W = g1x29_mul_pow2(W, 6);
  for (int m = 1; m < 64; m <<= 1) {
    const G1X29 other = g1x_shfl_xor(W, m);
    g1x29_add(W, other);
  }
  if (lane == 0) sh[wv] = g1x29_store(W);
  __syncthreads();
  if (threadIdx.x == 0) {
    G1X29 t = g1x29_load(sh[0]);
    for (unsigned w = 1; w <= row_waves; ++w) g1x29_add(t, g1x29_load(sh[w]));
    // back to the standard Montgomery form, then one inversion (or none: XYZZ)
    if (XYZZ) ((G1X *)out)[col] = g1x29_to_std(t);
    else ((G1Affine *)out)[col] = g1x_to_affine(g1x29_to_std(t));
  }
}

// K < 64 buckets (window_bits < 7: tiny bases and tests): one wave per MSM, lane b weights bucket b by b + 1
template <bool XYZZ>
__global__ void __launch_bounds__(64) k_msm_small(const G1X *__restrict__ buckets, unsigned K, void *__restrict__ out) {
  const size_t col = blockIdx.x;
  const unsigned lane = threadIdx.x;
  const G1X29 P = g1x29_load(lane < K ? buckets[col * K + lane] : G1X::identity());
  const unsigned k = lane + 1;
  G1X29 W = G1X29::identity();
  for (int bit = 6; bit >= 0; --bit) {
    W = g1x29_dbl(W);
    if ((k >> bit) & 1) g1x29_add(W, P);
  }
  for (int m = 1; m < 64; m <<= 1) {
    const G1X29 other = g1x_shfl_xor(W, m);
    g1x29_add(W, other);
  }
  if (lane == 0) {
    if (XYZZ) ((G1X *)out)[col] = g1x29_to_std(W);
    else ((G1Affine *)out)[col] = g1x_to_affine(g1x29_to_std(W));
  }
}

}  // namespace
