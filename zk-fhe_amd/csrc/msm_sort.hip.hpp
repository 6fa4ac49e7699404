// MSM bucket pipeline, stage 1 (included by msm.hip alone): signed-window digit extraction and the two counting sorts of the
// (bucket, table index, sign) entries.
#pragma once
#include "ctx.hpp"

namespace {
using namespace zk;

// (r-1)/2 as canonical limbs: scalars above it are negated
__device__ __forceinline__ bool fr_gt_half(const Fr &s) {
  const u32 H[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
  // compare s > H from the top limb
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    if (s.l[i] > H[i]) return true;
    if (s.l[i] < H[i]) return false;
  }
  return false;
}

// signed-window digits of the sign-magnitude scalar.  Calls f(w, bucket (1..2^(c-1)), negative)
template <class F>
__device__ __forceinline__ void for_each_digit(const Fr &mont, int c, int windows, F f) {
  Fr s = fp_from_mont<FrP>(mont);
  bool neg = fr_gt_half(s);
  if (neg) s = fp_neg<FrP>(s);  // r - s  (s != 0 here)
  u32 carry = 0;
  const u32 mask = (1u << c) - 1, halfv = 1u << (c - 1);
  // the scalar is shifted down by c bits per window (eight v_alignbit): indexing its limbs by the window's bit position put the
  // value into scratch memory (48 bytes per lane in every sort kernel)
  for (int w = 0; w < windows; ++w) {
    u32 v = (s.l[0] & mask) + carry;
#pragma unroll
    for (int i = 0; i < 7; ++i) s.l[i] = __builtin_amdgcn_alignbit(s.l[i + 1], s.l[i], (u32)c);
    s.l[7] >>= c;
    bool dneg = false;
    if (v > halfv) {
      v = (1u << c) - v;
      dneg = true;
      carry = 1;
    } else {
      carry = 0;
    }
    if (v) f(w, v, neg != dneg);
  }
}

// Histogram / scatter with LDS-privatised counters.  A workgroup owns a chunk of CHUNK scalars of ONE column and
// counts their digits in LDS (K+1 counters); only the non-zero bins touch global memory, with one atomic per
// (workgroup, bucket) instead of one per entry -- device-scope atomics are memory transactions on this chip
// (profiles/r1_pmc_traffic.md: 144 MB of writes per launch before this change).
constexpr unsigned SORT_CHUNK = 2048;   // scalars per workgroup
constexpr unsigned SORT_THREADS = 512;

// A sort workgroup's column and chunk, and its LDS counters at zero
template <unsigned THREADS>
__device__ __forceinline__ void sort_chunk_begin(unsigned chunks_per_col, unsigned *ctr, unsigned n_ctr, size_t &col, unsigned &chunk) {
  col = blockIdx.x / chunks_per_col;
  chunk = blockIdx.x % chunks_per_col;
  for (unsigned b = threadIdx.x; b < n_ctr; b += THREADS) ctr[b] = 0;
  __syncthreads();
}

__global__ void __launch_bounds__(SORT_THREADS) k_msm_hist(const Fr *__restrict__ scalars, size_t col_stride, size_t n, unsigned chunks_per_col, int c, int windows,
                                                          unsigned *__restrict__ hist /* [n_cols][K+1] */, unsigned K1) {
  extern __shared__ unsigned lh[];
  size_t col;
  unsigned chunk;
  sort_chunk_begin<SORT_THREADS>(chunks_per_col, lh, K1, col, chunk);
  const size_t i0 = (size_t)chunk * SORT_CHUNK, i1 = min(n, i0 + SORT_CHUNK);
  for (size_t i = i0 + threadIdx.x; i < i1; i += SORT_THREADS)
    for_each_digit(scalars[col * col_stride + i], c, windows, [&](int, u32 b, bool) { atomicAdd(&lh[b], 1u); });
  __syncthreads();
  unsigned *h = hist + col * K1;
  for (unsigned b = threadIdx.x; b < K1; b += SORT_THREADS) {
    const unsigned v = lh[b];
    if (v) atomicAdd(&h[b], v);
  }
}

// per column exclusive scan of hist[1..K] -> off[0..K]: bucket value v (1..K) owns sorted entries
// [off[v-1], off[v]); cursor[v] starts at off[v-1].  One block per column.
__global__ void __launch_bounds__(256) k_msm_scan(const unsigned *__restrict__ hist, unsigned *__restrict__ off,
                                                  unsigned *__restrict__ cursor, unsigned K1) {
  __shared__ unsigned part[256];
  const unsigned *h = hist + (size_t)blockIdx.x * K1;
  unsigned *o = off + (size_t)blockIdx.x * K1;
  unsigned *cu = cursor + (size_t)blockIdx.x * K1;
  const unsigned K = K1 - 1;
  const unsigned per = (K + 255) / 256;
  const unsigned lo = threadIdx.x * per, hi = min(lo + per, K);
  unsigned s = 0;
  for (unsigned b = lo; b < hi; ++b) s += h[b + 1];
  part[threadIdx.x] = s;
  __syncthreads();
  // exclusive scan of part (simple serial by one wave lane 0 is fine: 256 values)
  if (threadIdx.x == 0) {
    unsigned acc = 0;
    for (int i = 0; i < 256; ++i) {
      unsigned t = part[i];
      part[i] = acc;
      acc += t;
    }
  }
  __syncthreads();
  unsigned acc = part[threadIdx.x];
  for (unsigned b = lo; b < hi; ++b) {
    o[b] = acc;       // start of bucket b+1
    cu[b + 1] = acc;  // scatter cursor of bucket b+1
    acc += h[b + 1];
  }
  if (hi == K) o[K] = acc;  // total (every thread past the end writes the same value)
}

// scatter: count in LDS again, reserve one contiguous range per (workgroup, bucket) with a single global atomic,
// then rank the entries inside the range with LDS atomics: entries of a bucket coming from one workgroup land next
// to each other (fewer partial-line stores), and global atomics drop from one per entry to one per non-empty bin.
__global__ void __launch_bounds__(SORT_THREADS) k_msm_scatter(const Fr *__restrict__ scalars, size_t col_stride, size_t n, unsigned chunks_per_col, int c, int windows,
                                                             unsigned *__restrict__ cursor, unsigned K1, unsigned *__restrict__ entries,
                                                             size_t col_entries) {
  extern __shared__ unsigned lh[];  // [K1] counts, then running positions
  size_t col;
  unsigned chunk;
  sort_chunk_begin<SORT_THREADS>(chunks_per_col, lh, K1, col, chunk);
  const size_t i0 = (size_t)chunk * SORT_CHUNK, i1 = min(n, i0 + SORT_CHUNK);
  for (size_t i = i0 + threadIdx.x; i < i1; i += SORT_THREADS)
    for_each_digit(scalars[col * col_stride + i], c, windows, [&](int, u32 b, bool) { atomicAdd(&lh[b], 1u); });
  __syncthreads();
  unsigned *cu = cursor + col * K1;
  for (unsigned b = threadIdx.x; b < K1; b += SORT_THREADS) {
    const unsigned v = lh[b];
    lh[b] = v ? atomicAdd(&cu[b], v) : 0u;  // base position of this workgroup's run in bucket b
  }
  __syncthreads();
  unsigned *e = entries + col * col_entries;
  for (size_t i = i0 + threadIdx.x; i < i1; i += SORT_THREADS)
    for_each_digit(scalars[col * col_stride + i], c, windows, [&](int w, u32 b, bool neg) {
      const unsigned pos = atomicAdd(&lh[b], 1u);
      e[pos] = ((unsigned)w * (unsigned)n + (unsigned)i) | (neg ? 0x80000000u : 0u);
    });
}

// ---- two-level counting sort (K >= 2048 buckets: the long bases, n >= 2^15) -------------------------------------------
// With K = 8192 ... 32768 buckets a workgroup's 2048 scalars put about one entry into each LDS counter: the privatised
// histogram above saves nothing (one device-scope atomic per entry and bin, 128 KB of counters = one workgroup per CU) and every
// sorted entry is a lone 4-byte store into a 33 MB array (k = 19: 20 ms of a 170 ms proof in k_msm_hist + k_msm_scatter).
// Here the bucket id is split into a coarse part (NB = K >> L bins) and L fine bits that ride in the spare bits of the entry
// word (entry indices need log2(W n) bits):
//   k_msm_chist     coarse histogram per column (NB counters per workgroup, NB atomics per 2048 scalars);
//   k_msm_cscan     exclusive scan -> coarse segment bounds;
//   k_msm_cscatter  512 scalars per workgroup: entries ranked by coarse bin in LDS and copied out as contiguous runs
//                   (one reserved range per workgroup and bin) into the staging array, fine bits attached;
//   k_msm_fine      one workgroup per (column, coarse bin): histogram of the segment over its F = 2^L buckets, scan
//                   (-> off[], the bucket bounds every later kernel reads), and the placement inside the segment -- a
//                   window of a few hundred KB that the L2 holds until its lines are complete.
constexpr unsigned CH_SCALARS = 2048, CS_SCALARS = 512, CS_THREADS = 256, FINE_THREADS = 512, FINE_MAX = 256, FINE_COPIES = 8, FINE_CTRS = FINE_MAX * FINE_COPIES, FINE_TILE = 14336;
static_assert(FINE_CTRS == 4 * FINE_THREADS && FINE_TILE % (4 * FINE_THREADS) == 0, "k_msm_fine: four counters per thread, whole 16-byte loads per tile");

__global__ void __launch_bounds__(CS_THREADS) k_msm_chist(const Fr *__restrict__ scalars, size_t col_stride, size_t n, unsigned chunks_per_col, int c, int windows,
                                                         int L, unsigned NB, unsigned *__restrict__ chist /* [n_cols][NB] */) {
  extern __shared__ unsigned lh[];
  size_t col;
  unsigned chunk;
  sort_chunk_begin<CS_THREADS>(chunks_per_col, lh, NB, col, chunk);
  const size_t i0 = (size_t)chunk * CH_SCALARS, i1 = min(n, i0 + CH_SCALARS);
  for (size_t i = i0 + threadIdx.x; i < i1; i += CS_THREADS)
    for_each_digit(scalars[col * col_stride + i], c, windows, [&](int, u32 b, bool) { atomicAdd(&lh[(b - 1) >> L], 1u); });
  __syncthreads();
  for (unsigned g = threadIdx.x; g < NB; g += CS_THREADS) {
    const unsigned v = lh[g];
    if (v) atomicAdd(&chist[col * NB + g], v);
  }
}

// one thread per column: coff[col][0..NB] = exclusive scan of the coarse counts, ccursor = the segment starts
__global__ void __launch_bounds__(64) k_msm_cscan(const unsigned *__restrict__ chist, unsigned NB, size_t n_cols, unsigned *__restrict__ coff /* [n_cols][NB+1] */,
                                                  unsigned *__restrict__ ccursor /* [n_cols][NB] */) {
  const size_t col = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  unsigned acc = 0;
  for (unsigned g = 0; g < NB; ++g) {
    coff[col * (NB + 1) + g] = acc;
    ccursor[col * NB + g] = acc;
    acc += chist[col * NB + g];
  }
  coff[col * (NB + 1) + NB] = acc;
}

__global__ void __launch_bounds__(CS_THREADS) k_msm_cscatter(const Fr *__restrict__ scalars, size_t col_stride, size_t n, unsigned chunks_per_col, int c, int windows,
                                                            int L, unsigned NB, unsigned *__restrict__ ccursor, unsigned *__restrict__ stage, size_t stage_stride /* col_entries rounded up to four */) {
  extern __shared__ unsigned sh[];
  unsigned *cnt = sh, *loff = sh + NB, *gb = sh + 2 * NB, *buf = sh + 3 * NB;   // buf: CS_SCALARS * windows words
  size_t col;
  unsigned chunk;
  sort_chunk_begin<CS_THREADS>(chunks_per_col, cnt, NB, col, chunk);
  const size_t i0 = (size_t)chunk * CS_SCALARS, i1 = min(n, i0 + CS_SCALARS);
  for (size_t i = i0 + threadIdx.x; i < i1; i += CS_THREADS)
    for_each_digit(scalars[col * col_stride + i], c, windows, [&](int, u32 b, bool) { atomicAdd(&cnt[(b - 1) >> L], 1u); });
  __syncthreads();
  if (threadIdx.x < 64) {   // exclusive scan of cnt[0..NB) by the first wave: `per` consecutive bins per lane
    const unsigned per = (NB + 63) / 64, lo = threadIdx.x * per, hi = min(lo + per, NB);
    unsigned s = 0;
    for (unsigned g = lo; g < hi; ++g) s += cnt[g];
    unsigned inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(inc, d);
      if ((int)threadIdx.x >= d) inc += t;
    }
    unsigned acc = inc - s;
    for (unsigned g = lo; g < hi; ++g) {
      loff[g] = acc;
      acc += cnt[g];
    }
  }
  __syncthreads();
  for (unsigned g = threadIdx.x; g < NB; g += CS_THREADS) {
    const unsigned v = cnt[g];
    gb[g] = v ? atomicAdd(&ccursor[col * NB + g], v) : 0u;   // this workgroup's run inside the coarse segment
    cnt[g] = loff[g];                                        // from here on: the running position inside buf
  }
  __syncthreads();
  const unsigned fmask = (1u << L) - 1;
  const int fsh = 31 - L;
  for (size_t i = i0 + threadIdx.x; i < i1; i += CS_THREADS)
    for_each_digit(scalars[col * col_stride + i], c, windows, [&](int w, u32 b, bool neg) {
      const unsigned key = b - 1;
      const unsigned pos = atomicAdd(&cnt[key >> L], 1u);
      buf[pos] = ((unsigned)w * (unsigned)n + (unsigned)i) | ((key & fmask) << fsh) | (neg ? 0x80000000u : 0u);
    });
  __syncthreads();
  unsigned *dst_col = stage + col * stage_stride;
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (unsigned g = wv; g < NB; g += CS_THREADS / 64) {
    const unsigned base = loff[g], len = cnt[g] - base;
    unsigned *dst = dst_col + gb[g];
    for (unsigned k = lane; k < len; k += 64) dst[k] = buf[base + k];
  }
}

// exclusive scan over FINE_CTRS = 4 * FINE_THREADS counters in place (four consecutive counters per thread); returns nothing,
// every thread calls it
__device__ __forceinline__ void fine_scan_inplace(unsigned *ctr, unsigned *wsum /* [FINE_THREADS / 64] */) {
  const unsigned t = threadIdx.x, lane = t & 63;
  const uint4 c = *(const uint4 *)(ctr + 4 * t);
  const unsigned s = c.x + c.y + c.z + c.w;
  unsigned inc = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned u = __shfl_up(inc, d);
    if ((int)lane >= d) inc += u;
  }
  if (lane == 63) wsum[t >> 6] = inc;
  __syncthreads();
  unsigned pre = inc - s;
  for (unsigned w = 0; w < (t >> 6); ++w) pre += wsum[w];
  *(uint4 *)(ctr + 4 * t) = make_uint4(pre, pre + c.x, pre + c.x + c.y, pre + c.x + c.y + c.z);
  __syncthreads();
}

// One workgroup per (column, coarse bin).  Scattering the entries of the segment straight to their buckets is a lone 4-byte store
// per entry, and the chip retires ~105 G of those per second whatever the window they fall into (measured: 3.0 ms per 32 columns of
// 2^19, 0.46 ms with the stores left out).  So the segment is sorted tile by tile in LDS -- FINE_TILE entries: one returning atomic
// per entry gives its arrival rank, a scan the run starts, then placement in the LDS buffer -- and leaves as one contiguous run per
// bucket and tile (~56 entries on a full-width column).
// Witness columns and narrow top windows pile thousands of entries onto a few buckets, and LDS atomics on one address serialise
// (~10 cycles per lane, measured): every bucket has FINE_COPIES counters, lane l uses copy l % FINE_COPIES -- sub-buckets that sort
// next to each other, so the order inside a bucket changes and nothing else.
__global__ void __launch_bounds__(FINE_THREADS, 4) k_msm_fine(const unsigned *__restrict__ coff, unsigned NB, int L, const unsigned *__restrict__ stage, size_t stage_stride, size_t col_entries,
                                                             unsigned K1, unsigned *__restrict__ off, unsigned *__restrict__ entries) {
  extern __shared__ unsigned buf[];   // FINE_TILE words
  __shared__ __attribute__((aligned(16))) unsigned ctr[FINE_CTRS + 4];
  __shared__ unsigned gcur[FINE_MAX], wsum[FINE_THREADS / 64];
  const size_t col = blockIdx.x / NB;
  const unsigned g = blockIdx.x % NB;
  const unsigned F = 1u << L;
  const unsigned lo = coff[col * (NB + 1) + g], hi = coff[col * (NB + 1) + g + 1];
  const unsigned *src = stage + col * stage_stride;   // 16-byte aligned: the staging stride is a multiple of four entries
  const int fsh = 31 - L;
  const unsigned fmask = F - 1;
  const unsigned t = threadIdx.x, lane = t & 63, copy = lane % FINE_COPIES;
  for (unsigned i = t; i < FINE_CTRS + 4; i += FINE_THREADS) ctr[i] = 0;
  __syncthreads();
  const unsigned a0 = lo & ~3u;
  for (unsigned p0 = a0; p0 < hi; p0 += 4 * FINE_THREADS) {   // histogram of the whole segment
    const unsigned p = p0 + 4 * t;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p < hi) v = *(const uint4 *)(src + p);
    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p + j >= lo && p + j < hi) atomicAdd(&ctr[((w4[j] >> fsh) & fmask) * FINE_COPIES + copy], 1u);
  }
  __syncthreads();
  fine_scan_inplace(ctr, wsum);
  if (t < F) {
    const unsigned pre = lo + ctr[t * FINE_COPIES];
    off[col * K1 + (size_t)g * F + t] = pre;
    gcur[t] = pre;                       // where the next run of bucket t goes
  }
  if (g == NB - 1 && t == 0) off[col * K1 + (K1 - 1)] = hi;   // the column's total
  unsigned *e = entries + col * col_entries;
  const unsigned keep = 0x80000000u | ((1u << fsh) - 1);
  constexpr unsigned R = FINE_TILE / (4 * FINE_THREADS);
  for (unsigned t0 = a0; t0 < hi; t0 += FINE_TILE) {
    uint4 v[R];
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
      const unsigned p = t0 + 4 * (r * FINE_THREADS + t);
      v[r] = make_uint4(0, 0, 0, 0);
      if (p < hi) v[r] = *(const uint4 *)(src + p);
    }
    __syncthreads();   // the previous tile's runs are out, ctr is free
    for (unsigned i = t; i < FINE_CTRS + 4; i += FINE_THREADS) ctr[i] = 0;
    __syncthreads();
    unsigned arr[R][4];   // arrival rank of the entry inside its sub-bucket's run of this tile
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
      const unsigned p = t0 + 4 * (r * FINE_THREADS + t);
      const unsigned w4[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        arr[r][j] = 0;
        if (p + j >= lo && p + j < hi) arr[r][j] = atomicAdd(&ctr[((w4[j] >> fsh) & fmask) * FINE_COPIES + copy], 1u);
      }
    }
    __syncthreads();
    fine_scan_inplace(ctr, wsum);   // ctr[FINE_CTRS] stays 0: the last bucket's end comes from the tile's length below
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
      const unsigned p = t0 + 4 * (r * FINE_THREADS + t);
      const unsigned w4[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p + j >= lo && p + j < hi) buf[ctr[((w4[j] >> fsh) & fmask) * FINE_COPIES + copy] + arr[r][j]] = w4[j] & keep;
    }
    __syncthreads();
    const unsigned tile_lo = t0 < lo ? lo : t0, tile_hi = t0 + FINE_TILE < hi ? t0 + FINE_TILE : hi;
    for (unsigned f = t >> 6; f < F; f += FINE_THREADS / 64) {   // one wave per bucket run
      const unsigned b0 = ctr[f * FINE_COPIES], b1 = f + 1 < F ? ctr[(f + 1) * FINE_COPIES] : tile_hi - tile_lo;
      const unsigned *sp = buf + b0;
      unsigned *d = e + gcur[f];
      for (unsigned k = lane; k < b1 - b0; k += 64) d[k] = sp[k];
    }
    __syncthreads();
    if (t < F) gcur[t] += (t + 1 < F ? ctr[(t + 1) * FINE_COPIES] : tile_hi - tile_lo) - ctr[t * FINE_COPIES];
  }
}

}  // namespace
