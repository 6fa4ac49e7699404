// zkfhe_g1_fft: the radix-2 FFT over G1 points (halo2 best_fft::<G1>, g_to_lagrange), gfx950.
//
// One launch per stage, no waiting between workgroups inside a launch.  The points live in the accumulator form (XYZZ, 128 B) in
// scratch slot 0 between the stages -- no field inversion until the one per point of the store -- and the schedule (stage list,
// elements of a butterfly, twiddle index, bit reversal) is g1_fft_plan.hpp, whose index functions the kernels call.  A butterfly
// is one scalar multiplication t = w b and the two sums a + t, a - t (g1_fft_ladder.hip.hpp, the complete g1x_* functions); where
// the twiddle is 1 the multiplication is skipped.  Twiddles are public: nothing here is constant time.
// The ladder's table of multiples (b .. 4b, 512 B per butterfly) lives in scratch slot 1, read by digit: no per-thread array, no
// scratch memory, no LDS -- what bounds the waves per SIMD is the registers alone.
//   k_g1_fft_shared: stages with at least 64 blocks.  The 64 lanes of a wave take the same offset j of 64 blocks, hence the same
//                    twiddle; its words are made scalar registers, so the digits, the table index and the branches are the wave's.
//   k_g1_fft_window: the six stages with fewer blocks.  Every lane has its own twiddle; the fixed window keeps the lanes in step.
#include "ctx.hpp"
#include "g1_fft_ladder.hip.hpp"
#include "g1_fft_plan.hpp"

using namespace zk;

namespace {

// input element i (affine, identity = (0, 0)) -> slot bitrev(i), accumulator form
__global__ void __launch_bounds__(256) k_g1_fft_load(const G1Affine *__restrict__ in, G1X *__restrict__ x, int log_n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= ((size_t)1 << log_n)) return;
  x[g1_fft_bitrev(i, log_n)] = g1x_from_affine(in[i]);
}

__global__ void __launch_bounds__(256) k_g1_fft_store(const G1X *__restrict__ x, G1Affine *__restrict__ out, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = g1x_to_affine(x[i]);
}

// b, 2b, 3b, 4b of every butterfly of the launch: entry e, 16-byte word q of thread t at (e * 8 + q) * threads + t -- whatever
// digit a lane reads by, consecutive lanes touch consecutive words
struct G1FftTable {
  uint4 *at;        // the thread's word 0 of entry 0
  size_t threads;   // n / 2
  static __device__ __forceinline__ uint4 lo4(const Fq &f) { return make_uint4(f.l[0], f.l[1], f.l[2], f.l[3]); }
  static __device__ __forceinline__ uint4 hi4(const Fq &f) { return make_uint4(f.l[4], f.l[5], f.l[6], f.l[7]); }
  static __device__ __forceinline__ Fq join(const uint4 &a, const uint4 &b) {
    Fq f;
    f.l[0] = a.x, f.l[1] = a.y, f.l[2] = a.z, f.l[3] = a.w;
    f.l[4] = b.x, f.l[5] = b.y, f.l[6] = b.z, f.l[7] = b.w;
    return f;
  }
  __device__ __forceinline__ void put(int e, const G1X &p) {
    uint4 *s = at + (size_t)e * 8 * threads;
    s[0 * threads] = lo4(p.x), s[1 * threads] = hi4(p.x);
    s[2 * threads] = lo4(p.y), s[3 * threads] = hi4(p.y);
    s[4 * threads] = lo4(p.zz), s[5 * threads] = hi4(p.zz);
    s[6 * threads] = lo4(p.zzz), s[7 * threads] = hi4(p.zzz);
  }
  __device__ __forceinline__ G1X get(int e) const {
    const uint4 *s = at + (size_t)e * 8 * threads;
    G1X p;
    p.x = join(s[0 * threads], s[1 * threads]);
    p.y = join(s[2 * threads], s[3 * threads]);
    p.zz = join(s[4 * threads], s[5 * threads]);
    p.zzz = join(s[6 * threads], s[7 * threads]);
    return p;
  }
};
constexpr size_t G1FFT_TABLE_BYTES = (size_t)G1FFT_TABLE_ENTRIES * sizeof(G1X);   // per butterfly

// n / 2 is a multiple of 64 in every stage this kernel runs, so a wave is whole or absent: the readfirstlane below reads a value
// that every lane of the wave holds
__global__ void __launch_bounds__(G1FFT_WAVE) k_g1_fft_shared(G1X *__restrict__ x, uint4 *__restrict__ table, const Fr *__restrict__ tw, int log_n, int log_half) {
  const size_t threads = (size_t)1 << (log_n - 1);
  const size_t t = blockIdx.x * (size_t)G1FFT_WAVE + threadIdx.x;
  if (t >= threads) return;
  G1FftTable tab{table + t, threads};
  const G1FftButterfly bf = g1_fft_butterfly(G1FFT_SHARED, log_n, log_half, t);
  G1FftScalar k = g1_fft_scalar(tw[bf.tw], false, Fr::zero());
#pragma unroll
  for (int i = 0; i < 8; ++i) k.w[i] = (u32)__builtin_amdgcn_readfirstlane((int)k.w[i]);
  G1X b = x[bf.hi];
  if (!g1_fft_scalar_is_one(k)) b = g1x_mul_window(tab, b, k);
  G1X a = x[bf.lo];
  g1_fft_combine(a, b);
  x[bf.lo] = a;
  x[bf.hi] = b;
}

// SCALE: the last stage of an inverse call (g1_fft_plan.hpp): a and the twiddle carry n^-1
template <bool SCALE>
__global__ void __launch_bounds__(G1FFT_WAVE) k_g1_fft_window(G1X *__restrict__ x, uint4 *__restrict__ table, const Fr *__restrict__ tw, Fr n_inv, int log_n, int log_half) {
  const size_t threads = (size_t)1 << (log_n - 1);
  const size_t t = blockIdx.x * (size_t)G1FFT_WAVE + threadIdx.x;
  if (t >= threads) return;
  G1FftTable tab{table + t, threads};
  const G1FftButterfly bf = g1_fft_butterfly(G1FFT_WINDOW, log_n, log_half, t);
  const G1FftScalar k = g1_fft_scalar(tw[bf.tw], SCALE, n_inv);
  G1X b = x[bf.hi];
  if (!g1_fft_scalar_is_one(k)) b = g1x_mul_window(tab, b, k);
  G1X a = x[bf.lo];
  if (SCALE) a = g1x_mul_window(tab, a, g1_fft_scalar(n_inv, false, n_inv));
  g1_fft_combine(a, b);
  x[bf.lo] = a;
  x[bf.hi] = b;
}

}  // namespace

extern "C" int zkfhe_g1_fft(zkfhe_ctx *ctx, zkfhe_g1_affine *points_dev, int log_n, int inverse) {
  ZK_ENTER(ctx);
  if (!ctx) return ZKFHE_EINVAL;
  const G1FftPlan plan = g1_fft_plan(log_n, inverse != 0);
  if (!points_dev || plan.refused) return zk_fail_msg(ctx, ZKFHE_EINVAL, "g1_fft: points_dev is NULL or log_n is outside 1..20");
  const size_t n = (size_t)1 << log_n, half_n = n >> 1;
  const NttDomain *dom;
  ZK_CK(zk_domain(ctx, log_n, &dom));
  const Fr *tw = inverse ? dom->inv : dom->fwd;
  void *sc;
  ZK_CK(zk_scratch(ctx, 0, n * sizeof(G1X), &sc));
  G1X *x = (G1X *)sc;
  ZK_CK(zk_scratch(ctx, 1, half_n * G1FFT_TABLE_BYTES, &sc));
  uint4 *table = (uint4 *)sc;
  k_g1_fft_load<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>((const G1Affine *)points_dev, x, log_n);
  ZK_LAUNCH_CHECK(ctx);
  for (int s = 0; s < plan.n_stages; ++s) {
    const G1FftStage &st = plan.stage[s];
    zk_prof_begin(ctx);
    if (st.kind == G1FFT_SHARED) {
      // the plan puts the n^-1 in the last stage, which has one block: never here
      if (st.scale || (half_n & (G1FFT_WAVE - 1))) return zk_fail_msg(ctx, ZKFHE_EINVAL, "g1_fft: a shared-twiddle stage the kernel cannot run");
      k_g1_fft_shared<<<zk_blocks(half_n, G1FFT_WAVE), G1FFT_WAVE, 0, ctx->stream>>>(x, table, tw, log_n, st.log_half);
    } else if (st.scale) {
      k_g1_fft_window<true><<<zk_blocks(half_n, G1FFT_WAVE), G1FFT_WAVE, 0, ctx->stream>>>(x, table, tw, dom->n_inv, log_n, st.log_half);
    } else {
      k_g1_fft_window<false><<<zk_blocks(half_n, G1FFT_WAVE), G1FFT_WAVE, 0, ctx->stream>>>(x, table, tw, dom->n_inv, log_n, st.log_half);
    }
    ZK_LAUNCH_CHECK(ctx);
    // algorithmic bytes: every point read and written once per stage; ops: the scalar multiplications (none where the twiddle is 1)
    zk_prof_end(ctx, ZKFHE_PROF_G1_FFT, 2.0 * (double)n * sizeof(G1X));
    if (ctx->prof_on) ctx->prof_ops[ZKFHE_PROF_G1_FFT] += st.scale ? (double)n : (double)(half_n - (half_n >> st.log_half));
  }
  k_g1_fft_store<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>(x, (G1Affine *)points_dev, n);
  ZK_LAUNCH_CHECK(ctx);
  ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}
