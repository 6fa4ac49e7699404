// Wave- and workgroup-wide sums of G1X29 accumulators (shared by the MSM kernels of msm_bucket.hip.hpp, msm_table.hip.hpp and
// verify.hip).
#pragma once
#include "fq29.hip.hpp"

namespace zk {

__device__ __forceinline__ G1X29 g1x_shfl_down(const G1X29 &p, int delta) {
  G1X29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    r.x.l[i] = __shfl_down(p.x.l[i], delta);
    r.y.l[i] = __shfl_down(p.y.l[i], delta);
    r.zz.l[i] = __shfl_down(p.zz.l[i], delta);
    r.zzz.l[i] = __shfl_down(p.zzz.l[i], delta);
  }
  return r;
}

__device__ __forceinline__ G1X29 g1x_shfl_xor(const G1X29 &p, int mask) {
  G1X29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    r.x.l[i] = __shfl_xor(p.x.l[i], mask);
    r.y.l[i] = __shfl_xor(p.y.l[i], mask);
    r.zz.l[i] = __shfl_xor(p.zz.l[i], mask);
    r.zzz.l[i] = __shfl_xor(p.zzz.l[i], mask);
  }
  return r;
}

// Sum of 256 XYZZ points held one per thread -> thread 0.  Across the waves first, through LDS (waves 2, 3 hand theirs to
// waves 0, 1, then wave 1 to wave 0: three wave-wide additions), then a 6-step butterfly in wave 0 alone: 9 wave-wide
// additions where a 256-lane butterfly issues 26.
__device__ __forceinline__ G1X29 block_sum_256(G1X29 v, G1X *sh /* [128] */) {
  const unsigned wv = threadIdx.x >> 6;
  __syncthreads();
  if (wv >= 2) sh[threadIdx.x - 128] = g1x29_store(v);
  __syncthreads();
  if (wv < 2) g1x29_add(v, g1x29_load(sh[threadIdx.x]));
  __syncthreads();
  if (wv == 1) sh[threadIdx.x - 64] = g1x29_store(v);
  __syncthreads();
  if (wv == 0) {
    g1x29_add(v, g1x29_load(sh[threadIdx.x]));
    for (int m = 1; m < 64; m <<= 1) {
      const G1X29 other = g1x_shfl_xor(v, m);
      g1x29_add(v, other);
    }
  }
  return v;
}

}  // namespace zk
