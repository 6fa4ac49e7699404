// Device side of batch verification (zkfhe_bfv_verify_batch, host/verifier.cpp):
//   k_g1_decompress   32-byte compressed G1 points (host/point_encoding.hpp layout) -> Montgomery affine + a status per point
//   k_msm_segmented   many small MSMs over one shared array of affine points addressed by index:
//                     out[s] = sum_{t in [off[s], off[s+1])} scalar[t] * points[index[t]]
// A proof's SHPLONK combination F_j is one segment (its own ~320 points, the vk's fixed / sigma commitments shared by index,
// the generator, h1, h2); the batch combination sum_j r_j F_j and sum_j r_j W_j are two more segments over the F_j / W_j.
#include <hip/hip_runtime.h>

#include "ctx.hpp"
#include "fq29.hip.hpp"
#include "g1x29_wave.hip.hpp"
#include "../host/point_encoding.hpp"

using namespace zk;

namespace {

// BN254 q, and (q + 1) / 4: q = 3 mod 4, so a square y2 has the root y2^((q+1)/4)
__constant__ u32 Q_WORDS[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
__constant__ u32 SQRT_EXP[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};

// standard Montgomery (x 2^256) -> the 2^261 form of the nine-limb arithmetic: times to_mont(32) (fq29.hip.hpp g1_affine_to_29)
__device__ __forceinline__ Fq fq_times32(const Fq &m) {
  Fq c = Fq::zero();
  c.l[0] = 32;
  return m * fp_to_mont<FqP>(c);
}

// One lane per point.  status: ZKFHE_PT_OK, _X_NOT_REDUCED, _NOT_ON_CURVE, _BAD_IDENTITY; anything but OK leaves (0, 0).
// The checks and their order are those of the host decoder (host/proof_reader.hpp decode_point); any 32 bytes are accepted.
__global__ void __launch_bounds__(256) k_g1_decompress(const uint8_t *__restrict__ in, size_t n, u32 sign_bit, u32 id_bit, u32 x_mask,
                                                       G1Affine *__restrict__ out, int32_t *__restrict__ status) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 w[8];
  const uint8_t *b = in + 32 * i;
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = (u32)b[4 * k] | ((u32)b[4 * k + 1] << 8) | ((u32)b[4 * k + 2] << 16) | ((u32)b[4 * k + 3] << 24);
  const u32 b31 = w[7] >> 24;
  G1Affine r;
  r.x = Fq::zero();
  r.y = Fq::zero();
  bool ident;
  if (id_bit) {
    ident = (b31 & id_bit) != 0;
  } else {
    u32 any = 0;
    for (int k = 0; k < 8; ++k) any |= w[k];
    ident = any == 0;
  }
  if (ident) {
    // exactly one encoding: 31 zero bytes, then the identity bit alone
    u32 rest = w[7] & 0x00ffffffu;
    for (int k = 0; k < 7; ++k) rest |= w[k];
    out[i] = r;
    status[i] = (rest || b31 != id_bit) ? ZKFHE_PT_BAD_IDENTITY : ZKFHE_PT_OK;
    return;
  }
  const u32 sign = (b31 & sign_bit) ? 1u : 0u;
  w[7] = (w[7] & 0x00ffffffu) | ((b31 & x_mask) << 24);
  bool lt = false;   // x < q, most significant word first
  for (int k = 7; k >= 0; --k) {
    if (w[k] != Q_WORDS[k]) {
      lt = w[k] < Q_WORDS[k];
      break;
    }
  }
  if (!lt) {
    out[i] = r;
    status[i] = ZKFHE_PT_X_NOT_REDUCED;
    return;
  }
  Fq x;
  for (int k = 0; k < 8; ++k) x.l[k] = w[k];
  const Fq xm = fp_to_mont<FqP>(x);
  // y2 = x^3 + 3 and y = y2^((q+1)/4) in the nine-limb form (values below 2 p between steps)
  Fq three = Fq::zero();
  three.l[0] = 3;
  const F29 x29 = f29_unpack(fq_times32(xm));
  const F29 y2 = f29_canonical(f29_add(f29_mul(f29_sqr(x29), x29), f29_unpack(fq_times32(fp_to_mont<FqP>(three)))));
  const u32 ONE[9] = ZK_Q29_ONE;
  F29 y = f29_const(ONE);
  for (int bit = 253; bit >= 0; --bit) {
    y = f29_sqr(y);
    if ((SQRT_EXP[bit >> 5] >> (bit & 31)) & 1) y = f29_mul(y, y2);
  }
  const F29 yy = f29_canonical(f29_sqr(y));
  bool on = true;
  for (int k = 0; k < 9; ++k) on = on && yy.l[k] == y2.l[k];
  if (!on) {
    out[i] = r;
    status[i] = ZKFHE_PT_NOT_ON_CURVE;
    return;
  }
  const u32 K[9] = ZK_Q29_R256;   // x 2^261 -> x 2^256
  Fq ym = f29_pack(f29_canonical(f29_mul(y, f29_const(K))));
  if ((fp_from_mont<FqP>(ym).l[0] & 1u) != sign) ym = fp_neg<FqP>(ym);
  r.x = xm;
  r.y = ym;
  out[i] = r;
  status[i] = ZKFHE_PT_OK;
}

// Per term: the canonical scalar (bits to scan) and a bad-index flag; per point: the 2^261 form the additions read.
__global__ void __launch_bounds__(256) k_seg_prep_terms(const Fr *__restrict__ scalars, const uint32_t *__restrict__ index, size_t n_terms, size_t n_points,
                                                        Fr *__restrict__ canon, u32 *__restrict__ err) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n_terms) return;
  canon[t] = fp_from_mont<FrP>(scalars[t]);
  if (index[t] >= n_points) atomicOr(err, 1u);
}
__global__ void __launch_bounds__(256) k_seg_prep_points(const G1Affine *__restrict__ pts, size_t n, G1Affine *__restrict__ pts29) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  pts29[i] = g1_affine_to_29(pts[i]);
}

// One workgroup per segment, 256 lanes.  Lane l owns terms off[s] + l, + 256, ...; it runs ONE double-and-add over the bits of
// all its terms together (Straus: 254 doublings per lane whatever its term count, one mixed addition per set bit), from the
// highest bit any of them has -- the batch randomisers are 128-bit, so their segments double half as often.  Then the
// workgroup sum (block_sum_256) and one normalisation.  A segment of 1..256 terms costs one scalar multiplication of latency,
// a verification segment (~700 terms) three terms per lane.  Bad offsets / indices set *err and contribute nothing.
__global__ void __launch_bounds__(256) k_msm_segmented(const G1Affine *__restrict__ pts29, size_t n_points, const uint32_t *__restrict__ index,
                                                       const Fr *__restrict__ canon, size_t n_terms, const uint32_t *__restrict__ off,
                                                       G1Affine *__restrict__ out, u32 *__restrict__ err) {
  __shared__ G1X sh[128];
  const unsigned s = blockIdx.x;
  size_t lo = off[s], hi = off[s + 1];
  if (lo > hi || hi > n_terms) {
    if (threadIdx.x == 0) atomicOr(err, 2u);
    lo = hi = 0;
  }
  int top = -1;
  for (size_t t = lo + threadIdx.x; t < hi; t += 256) {
    const Fr &k = canon[t];
    for (int wd = 7; wd >= 0; --wd)
      if (k.l[wd]) {
        top = max(top, 32 * wd + 31 - __clz((int)k.l[wd]));
        break;
      }
  }
  G1X29 acc = G1X29::identity();
  for (int bit = top; bit >= 0; --bit) {
    acc = g1x29_dbl(acc);
    for (size_t t = lo + threadIdx.x; t < hi; t += 256) {
      if (!((canon[t].l[bit >> 5] >> (bit & 31)) & 1)) continue;
      const uint32_t idx = index[t];
      if (idx < n_points) g1x29_add_affine(acc, g1a29_load(pts29[idx]), false);
    }
  }
  acc = block_sum_256(acc, sh);
  if (threadIdx.x == 0) out[s] = g1x_to_affine(g1x29_to_std(acc));
}

}  // namespace

extern "C" {

int zkfhe_g1_decompress(zkfhe_ctx *ctx, const uint8_t *in_dev, size_t n, zkfhe_g1_affine *out_dev, int32_t *status_dev) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && in_dev && out_dev && status_dev);
  if (!n) return ZKFHE_OK;
  const zkhost::ptenc::Layout &L = zkhost::ptenc::layout();
  zk_prof_begin(ctx);
  k_g1_decompress<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>(in_dev, n, L.sign_bit, L.identity_bit, L.x_mask, (G1Affine *)out_dev, status_dev);
  ZK_LAUNCH_CHECK(ctx);
  zk_prof_end(ctx, ZKFHE_PROF_G1_DECOMPRESS, 32.0 * n);
  return ZKFHE_OK;
}

int zkfhe_msm_segmented(zkfhe_ctx *ctx, const zkfhe_g1_affine *points_dev, size_t n_points, const uint32_t *index_dev, const zkfhe_fr *scalars_dev,
                        size_t n_terms, const uint32_t *seg_off_dev, size_t n_segs, zkfhe_g1_affine *out_dev) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, ctx && seg_off_dev && out_dev && (points_dev || !n_points) && ((index_dev && scalars_dev) || !n_terms));
  ZK_ARG(ctx, n_segs < (1u << 31) && n_points < 0xffffffffu);
  if (!n_segs) return ZKFHE_OK;
  // stream-ordered temporaries: [err word | canonical scalars | points in the 2^261 form]
  const size_t bytes = 64 + n_terms * sizeof(Fr) + n_points * sizeof(G1Affine);
  void *tmp = nullptr;
  ZK_HIP(ctx, hipMallocAsync(&tmp, bytes, ctx->stream));
  u32 *err = (u32 *)tmp;
  Fr *canon = (Fr *)((char *)tmp + 64);
  G1Affine *pts29 = (G1Affine *)((char *)tmp + 64 + n_terms * sizeof(Fr));
  int rc = ZKFHE_OK;
  u32 err_host = 0;
  auto run = [&]() -> int {
    ZK_HIP(ctx, hipMemsetAsync(err, 0, 4, ctx->stream));
    if (n_terms) k_seg_prep_terms<<<zk_blocks(n_terms, 256), 256, 0, ctx->stream>>>((const Fr *)scalars_dev, index_dev, n_terms, n_points, canon, err);
    if (n_points) k_seg_prep_points<<<zk_blocks(n_points, 256), 256, 0, ctx->stream>>>((const G1Affine *)points_dev, n_points, pts29);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_begin(ctx);
    k_msm_segmented<<<(unsigned)n_segs, 256, 0, ctx->stream>>>(pts29, n_points, index_dev, canon, n_terms, seg_off_dev, (G1Affine *)out_dev, err);
    ZK_LAUNCH_CHECK(ctx);
    zk_prof_end(ctx, ZKFHE_PROF_MSM_SEGMENTED, 96.0 * n_terms);
    ZK_HIP(ctx, hipMemcpyAsync(&err_host, err, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, zk_wait(ctx));
    return ZKFHE_OK;
  };
  rc = run();
  (void)hipFreeAsync(tmp, ctx->stream);
  if (rc) return rc;
  if (err_host & 1u) return zk_fail_msg(ctx, ZKFHE_EINVAL, "zkfhe_msm_segmented: a point index is out of range");
  if (err_host & 2u) return zk_fail_msg(ctx, ZKFHE_EINVAL, "zkfhe_msm_segmented: segment offsets are not ascending within [0, n_terms]");
  return ZKFHE_OK;
}

}  // extern "C"
