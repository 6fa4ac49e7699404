// Batched NTT / iNTT / coset NTT over BN254 Fr for gfx950.
//
// Replaces halo2_proofs `arithmetic::best_fft` and `EvaluationDomain::{lagrange_to_coeff,
// coeff_to_extended, extended_to_coeff}` (third-party; reached from reference examples/bfv.rs:311;
// semantics restated in oracle/oracle.c orc_fft / orc_ntt / orc_coset_ntt).  The DFT is unique, so
// the algorithm is free: this is an autosort Stockham transform, natural order in and out, with no
// bit-reversal pass.
//
// Tile kernel (2^3 <= n <= 2^13): ONE workgroup per column, n/8 threads, 8 coefficients per thread
// held in VGPRs (64 VGPRs of data).  Each pass is a radix-8 (or final radix-4/2) butterfly done
// entirely in registers; between passes the column is transposed through LDS.  A 2^13 column is
// 256 KiB -- more than the 160 KiB LDS -- so the transpose moves the low and the high 16 bytes of
// every element in two rounds of ds_write_b128 / ds_read_b128 (144 KiB with the +1/8 padding that
// keeps the stride-8 writes of the first pass bank-conflict-free).  HBM traffic is the
// algorithmic minimum: every coefficient is read once and written once, both as full 2 KiB-per-wave
// coalesced runs; twiddles come from an omega^j table that all columns share (L2 resident).
//
// Larger n: the log2(n/2^13) DIF stages above the tile in a few passes over the whole vector (coalesced), then the tile
// kernel on each contiguous 2^13 block with a strided scatter to natural order.  Which passes, and through which buffers, is
// the plan of ntt_plan.hpp (host only, checked on the CPU); ntt_long_rows below runs it.  The extended domain stays
// coset-major (zkfhe_coset_ntt_batch), so the prover's longest transform has the length of a column.
#include <cstring>

#include "ctx.hpp"
#include "ntt_plan.hpp"
#include "ntt_tile.hip.hpp"
#include "fr29.hip.hpp"

using namespace zk;

namespace {

// one radix-2 DIF stage over vectors of length n (all columns): pairs (j, j+half) inside blocks of 2*half
//   a' = a + b ; b' = (a - b) * omega_n^(j * n/(2*half)),  j = index inside the half
// pre != nullptr (first pass of a coset extension): the n_cols transforms are `rows` coset rows of n_cols / rows input vectors;
// transform c reads input vector c / rows and multiplies element i by pre[(c % rows) * n + i] on the way in (the coset powers).
__global__ void __launch_bounds__(256) k_dif_stage(const Fr *src, Fr *data, size_t n_cols, int log_n, int log_half,
                                                   const Fr *__restrict__ tw_n /* omega_n^j, j < n/2, 2^261 form */,
                                                   const Fr *__restrict__ pre = nullptr, unsigned rows = 1) {
  const size_t half = (size_t)1 << log_half;
  const size_t per_col = (size_t)1 << (log_n - 1);
  const size_t total = n_cols * per_col;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t c = g >> (log_n - 1);
    const size_t i = g & (per_col - 1);
    const size_t j = i & (half - 1);
    const size_t blk = i >> log_half;
    const size_t w = (blk << (log_half + 1)) + j;
    const size_t o = (c << log_n) + w;
    Fr *p = data + o;
    Fr x, y;
    if (pre) {
      const size_t cs = c / rows, k1 = c - cs * rows;
      const Fr *ps = src + (cs << log_n) + w, *pp = pre + (k1 << log_n) + w;
      x = fr29_mul_const(ps[0], pp[0]);
      y = fr29_mul_const(ps[half], pp[half]);
    } else {
      x = src[o];   // src == data: in place
      y = src[o + half];
    }
    Fr s = x + y, d = x - y;
    const size_t e = j << (log_n - 1 - log_half);
    p[0] = s;
    p[half] = e ? fr29_mul_const(d, tw_n[e]) : d;
  }
}

// S consecutive radix-2 DIF stages (halves 2^log_half, 2^(log_half-1), ...) in one pass over memory: a thread holds the
// 2^S elements base + m * 2^(log_half - S + 1) of one block of 2^(log_half + 1) and runs the S butterfly levels in
// registers.  Long rows (k = 16 .. 19) used to make one full read+write of every column per stage.
template <int S>
__global__ void __launch_bounds__(256) k_dif_fused(const Fr *src, Fr *data, size_t n_cols, int log_n, int log_half, const Fr *__restrict__ tw_n,
                                                   const Fr *__restrict__ pre = nullptr, unsigned rows = 1 /* as in k_dif_stage */) {
  constexpr int R = 1 << S;
  const int log_q = log_half - S + 1;            // distance between the elements of a thread
  const size_t q = (size_t)1 << log_q;
  const size_t per_col = (size_t)1 << (log_n - S);
  const size_t total = n_cols * per_col;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t c = g >> (log_n - S);
    const size_t i = g & (per_col - 1);
    const size_t j0 = i & (q - 1);
    const size_t blk = i >> log_q;
    const size_t w = (blk << (log_half + 1)) + j0;
    const size_t o = (c << log_n) + w;
    Fr *p = data + o;
    Fr x[R];
    if (pre) {
      const size_t cs = c / rows, k1 = c - cs * rows;
      const Fr *ps = src + (cs << log_n) + w, *pp = pre + (k1 << log_n) + w;
#pragma unroll
      for (int m = 0; m < R; ++m) x[m] = fr29_mul_const(ps[(size_t)m << log_q], pp[(size_t)m << log_q]);
    } else {
      const Fr *ps = src + o;   // src == data: in place; otherwise the first pass of an out-of-place transform
#pragma unroll
      for (int m = 0; m < R; ++m) x[m] = ps[(size_t)m << log_q];
    }
#pragma unroll
    for (int t = 0; t < S; ++t) {
      const int h = R >> (t + 1);                // partner distance in units of q
      const int sh = log_n - 1 - (log_half - t); // twiddle exponent shift of this level
#pragma unroll
      for (int m = 0; m < R; ++m) {
        if (m & h) continue;
        const size_t j = j0 + ((size_t)(m & (h - 1)) << log_q);
        const Fr a = x[m], b = x[m + h];
        x[m] = a + b;
        const Fr d = a - b;
        const size_t e = j << sh;
        x[m + h] = e ? fr29_mul_const(d, tw_n[e]) : d;
      }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) p[(size_t)m << log_q] = x[m];
  }
}

// 3 + SB radix-2 DIF stages in ONE pass over memory (rows of 2^17 .. 2^19: the four to six stages above the 2^13 tile were two
// passes of k_dif_fused, each a full read and write of every row -- 18.7 ms of a k = 19 proof at 2.5 TB/s).  A workgroup of 128
// threads owns a tile of M = 2^(3+SB) positions m (stride q = 2^(log_half - 2 - SB) elements) x JJ = 1024 / M consecutive
// offsets: a thread runs three levels on m = g + (M/8) r in registers, the tile goes through LDS (two 16-byte halves per element,
// each half array contiguous across the lanes: no bank conflicts), and the thread runs the last SB levels on the eight
// consecutive m = 8u + r.  Loads and stores are runs of JJ * 32 bytes.
template <int SB>
__global__ void __launch_bounds__(128) k_dif_lds(const Fr *src, Fr *data, size_t n_cols, int log_n, int log_half, const Fr *__restrict__ tw_n,
                                                 const Fr *__restrict__ pre = nullptr, unsigned rows = 1 /* as in k_dif_stage */) {
  constexpr int S = 3 + SB, M = 1 << S, JJ = 1024 / M, G = M / 8;
  __shared__ uint4 sh_lo[1024], sh_hi[1024];
  const int log_q = log_half - S + 1;
  const int sh0 = log_n - 1 - log_half;
  const size_t tiles_per_col = (size_t)1 << (log_n - 10);
  const size_t total = n_cols * tiles_per_col;
  const unsigned jj = threadIdx.x % JJ, gu = threadIdx.x / JJ;   // gu: g in the first half, u in the second
  for (size_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const size_t c = tile >> (log_n - 10);
    const size_t i = (tile & (tiles_per_col - 1)) * JJ + jj;     // position among the n / M of the column
    const size_t j0 = i & (((size_t)1 << log_q) - 1);
    const size_t w = ((i >> log_q) << (log_half + 1)) + j0;
    const size_t o = (c << log_n) + w;
    Fr x[8];
    if (pre) {
      const size_t cs = c / rows, k1 = c - cs * rows;
      const Fr *ps = src + (cs << log_n) + w, *pp = pre + (k1 << log_n) + w;
#pragma unroll
      for (int r = 0; r < 8; ++r) x[r] = fr29_mul_const(ps[(size_t)(gu + G * r) << log_q], pp[(size_t)(gu + G * r) << log_q]);
    } else {
      const Fr *ps = src + o;
#pragma unroll
      for (int r = 0; r < 8; ++r) x[r] = ps[(size_t)(gu + G * r) << log_q];
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int hr = 4 >> t;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        if (r & hr) continue;
        const size_t j = j0 + ((size_t)(gu + G * (r & (hr - 1))) << log_q);
        const Fr a = x[r], b = x[r + hr];
        x[r] = a + b;
        const Fr d = a - b;
        const size_t e = j << (sh0 + t);
        x[r + hr] = e ? fr29_mul_const(d, tw_n[e]) : d;
      }
    }
    __syncthreads();   // the previous tile has been read
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const unsigned idx = (gu + G * r) * JJ + jj;
      sh_lo[idx] = make_uint4(x[r].l[0], x[r].l[1], x[r].l[2], x[r].l[3]);
      sh_hi[idx] = make_uint4(x[r].l[4], x[r].l[5], x[r].l[6], x[r].l[7]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const unsigned idx = (8 * gu + r) * JJ + jj;
      const uint4 lo = sh_lo[idx], hi = sh_hi[idx];
      x[r].l[0] = lo.x, x[r].l[1] = lo.y, x[r].l[2] = lo.z, x[r].l[3] = lo.w;
      x[r].l[4] = hi.x, x[r].l[5] = hi.y, x[r].l[6] = hi.z, x[r].l[7] = hi.w;
    }
#pragma unroll
    for (int t = 3; t < S; ++t) {
      const int hm = M >> (t + 1);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        if (r & hm) continue;
        const size_t j = j0 + ((size_t)(r & (hm - 1)) << log_q);
        const Fr a = x[r], b = x[r + hm];
        x[r] = a + b;
        const Fr d = a - b;
        const size_t e = j << (sh0 + t);
        x[r + hm] = e ? fr29_mul_const(d, tw_n[e]) : d;
      }
    }
    Fr *p = data + o;
#pragma unroll
    for (int r = 0; r < 8; ++r) p[(size_t)(8 * gu + r) << log_q] = x[r];
  }
}

__global__ void __launch_bounds__(256) k_pow_table(Fr base, Fr *__restrict__ out, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Fr r = Fr::one();
    Fr b = base;
    for (size_t e = i; e; e >>= 1) {
      if (e & 1) r = r * b;
      b = fp_sqr<FrP>(b);
    }
    out[i] = r;
  }
}

// out[i] = start * base^i
__global__ void __launch_bounds__(256) k_pow_table_scaled(Fr start, Fr base, Fr *__restrict__ out, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Fr r = start;
    Fr b = base;
    for (size_t e = i; e; e >>= 1) {
      if (e & 1) r = r * b;
      b = fp_sqr<FrP>(b);
    }
    out[i] = r;
  }
}

// extended_to_coeff combine: for each (column, i2 < n): the 2^lef values A[k1][i2] (k1-major rows of
// length n) hold, after the row iNTTs (scaled by n^-1), (1/n) sum_k2 F[k1][k2] w^(-i2 k2).  Then
// coefficient i1*n + i2 = g^-(i1*n+i2) * 2^-lef * sum_k1 A[k1][i2] * w_ext^(-k1 (i1*n + i2))
//                       = scale[i1*n+i2] * sum_k1 (A[k1][i2] * w_ext^(-k1 i2)) * w_E^(-k1 i1),  E = 2^lef.
// LEF in {1,2,3}.
template <int LEF>
__global__ void __launch_bounds__(256) k_ext_combine(const Fr *__restrict__ rows, Fr *__restrict__ out, size_t n_cols, int log_n,
                                                     const Fr *__restrict__ tw_ext_inv /* w_ext^-j, j < n*E */,
                                                     const Fr *__restrict__ scale /* 2^-lef g^-j, j < n*E */) {   // both tables in the 2^261 form
  constexpr int E = 1 << LEF;
  const size_t n = (size_t)1 << log_n;
  const size_t total = n_cols * n;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t c = g >> log_n, i2 = g & (n - 1);
    const Fr *src = rows + c * n * E;
    Fr v[E];
#pragma unroll
    for (int k1 = 0; k1 < E; ++k1) {
      Fr x = src[(size_t)k1 * n + i2];
      v[k1] = k1 ? fr29_mul_const(x, tw_ext_inv[(size_t)k1 * i2]) : x;
    }
    // DFT_E with root w_E^-1 = w_ext^-(n)
    Fr o[E];
#pragma unroll
    for (int i1 = 0; i1 < E; ++i1) {
      Fr acc = v[0];
#pragma unroll
      for (int k1 = 1; k1 < E; ++k1) {
        const int e = (k1 * i1) & (E - 1);
        acc = acc + (e ? fr29_mul_const(v[k1], tw_ext_inv[(size_t)e * n]) : v[k1]);
      }
      o[i1] = acc;
    }
    Fr *dst = out + c * n * E;
#pragma unroll
    for (int i1 = 0; i1 < E; ++i1) dst[(size_t)i1 * n + i2] = fr29_mul_const(o[i1], scale[(size_t)i1 * n + i2]);
  }
}

int launch_tile_dyn(zkfhe_ctx *ctx, int log_tile, const TileArgs &a, unsigned tiles, unsigned cols) {
#define ZK_TILE_LAUNCHER(k) zk_launch_tile_##k,
  static int (*const launchers[])(zkfhe_ctx *, const TileArgs &, unsigned, unsigned) = {ZK_TILE_SIZES(ZK_TILE_LAUNCHER)};
#undef ZK_TILE_LAUNCHER
  if (log_tile < 3 || log_tile > NTT_TILE_LOG) return zk_fail_msg(ctx, ZKFHE_EINVAL, "tile size out of range");
  return launchers[log_tile - 3](ctx, a, tiles, cols);
}

// The three shapes of a tile launch.  Each returns a TileArgs for columns of n = 2^log_n points cut into 2^log_tiles tiles; the
// fields it does not name stay zero, which the tile kernels read as "absent".

// Independent tiles, natural order: tile b of column c is the run of N = n points at (c 2^log_tiles + b) N, in and out.  No
// multiplier at the load (pre, pre13 and pre_tile_stride zero); post: one multiplier at the store (n^-1), or nullptr.
TileArgs tiles_independent(const Fr *in, Fr *out, int log_n, int log_tiles, const Fr *tw, const Fr *post) {
  const size_t n = (size_t)1 << log_n;
  TileArgs a{};
  a.in = in;
  a.out = out;
  a.in_tile_stride = n;
  a.col_stride_in = a.col_stride_out = n << log_tiles;
  a.tw = tw;
  a.post = post;
  a.log_tiles = log_tiles;
  a.in_len = (int)n;
  a.out_natural_tiles = 1;
  return a;
}

// One input fanned out to `rows` coset tiles: every tile of column c reads the same n coefficients at c n (in_tile_stride zero) and
// tile k1 multiplies them by its row of coset powers as it loads; the rows of a column come out densely, (c rows + k1) n.  The
// powers are either `pre` ([rows][n], 2^261 form) or, at n = 2^13, the tables of zk_pre13 (`pre13`; pre is then nullptr: that tile
// never reads it).  No multiplier at the store (post zero).
TileArgs tiles_fan_out(const Fr *in, Fr *out, int log_n, int lef, int rows, const Fr *tw, const Fr *pre, const void *pre13) {
  const size_t n = (size_t)1 << log_n;
  TileArgs a{};
  a.in = in;
  a.out = out;
  a.col_stride_in = n;
  a.col_stride_out = n * (size_t)rows;
  a.tw = tw;
  a.pre = pre;
  a.pre13 = pre13;
  a.pre_tile_stride = n;
  a.log_tiles = lef;
  a.in_len = (int)n;
  a.out_natural_tiles = 1;
  return a;
}

// The last stage of a long row: the 2^(log_n - 13) contiguous 2^13 blocks of a column, each transformed and scattered with stride
// 2^log_tiles from the bit-reversed block number (out_natural_tiles zero).  No multiplier at the load; post as above.
TileArgs tiles_scatter(const Fr *in, Fr *out, int log_n, const Fr *tw, const Fr *post) {
  TileArgs a{};
  a.in = in;
  a.out = out;
  a.in_tile_stride = (size_t)1 << NTT_TILE_LOG;
  a.col_stride_in = a.col_stride_out = (size_t)1 << log_n;
  a.tw = tw;
  a.post = post;
  a.log_tiles = log_n - NTT_TILE_LOG;
  a.in_len = 1 << NTT_TILE_LOG;
  return a;
}

}  // namespace

int zk_domain(zkfhe_ctx *ctx, int log_n, const NttDomain **out) {
  auto it = ctx->domains.find(log_n);
  if (it == ctx->domains.end()) {
    NttDomain d;
    struct Guard {   // the tables of a half-built domain are released on every early return
      NttDomain *d;
      ~Guard() {
        if (!d) return;
        (void)hipFree(d->fwd), (void)hipFree(d->inv), (void)hipFree(d->fwd29), (void)hipFree(d->inv29), (void)hipFree(d->n_inv29_dev);
      }
    } guard{&d};
    d.log_n = log_n;
    const size_t n = (size_t)1 << log_n;
    d.omega = zk_fr_root_of_unity(log_n);
    d.omega_inv = fp_inv<FrP>(d.omega);
    d.n_inv = fp_inv<FrP>(zk_fr_from_u64((uint64_t)n));
    ZK_HIP(ctx, hipMalloc((void **)&d.fwd, n * sizeof(Fr)));
    ZK_HIP(ctx, hipMalloc((void **)&d.inv, n * sizeof(Fr)));
    unsigned grid = zk_blocks(n, 256);
    if (grid > 4096) grid = 4096;
    k_pow_table<<<grid, 256, 0, ctx->stream>>>(d.omega, d.fwd, n);
    ZK_LAUNCH_CHECK(ctx);
    k_pow_table<<<grid, 256, 0, ctx->stream>>>(d.omega_inv, d.inv, n);
    ZK_LAUNCH_CHECK(ctx);
    const Fr c32 = zk_fr_to_29(Fr::one());   // 32 in the standard Montgomery form
    d.n_inv29 = d.n_inv * c32;
    ZK_HIP(ctx, hipMalloc((void **)&d.fwd29, n * sizeof(Fr)));
    ZK_HIP(ctx, hipMalloc((void **)&d.inv29, n * sizeof(Fr)));
    k_pow_table_scaled<<<grid, 256, 0, ctx->stream>>>(c32, d.omega, d.fwd29, n);
    ZK_LAUNCH_CHECK(ctx);
    k_pow_table_scaled<<<grid, 256, 0, ctx->stream>>>(c32, d.omega_inv, d.inv29, n);
    ZK_LAUNCH_CHECK(ctx);
    ZK_HIP(ctx, hipMalloc((void **)&d.n_inv29_dev, 64));
    ZK_HIP(ctx, zk_memcpy_async(ctx, d.n_inv29_dev, &d.n_inv29, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the source is a local of this function
    it = ctx->domains.emplace(log_n, d).first;
    guard.d = nullptr;
  }
  *out = &it->second;
  return ZKFHE_OK;
}

namespace {

// n = 2 and n = 4: log_n radix-2 stages in place on the destination, which leave n = 4 with outputs 1 and 2 exchanged.  The
// exchange (two strided copies out of a snapshot in scratch slot 0) and the n^-1 of the inverse (zkfhe_fr_scale) follow; no tile
// kernel exists below eight points.
int ntt_tiny(zkfhe_ctx *ctx, const Fr *src, Fr *data, size_t n_cols, int log_n, int inverse, const NttDomain *dom) {
  const size_t n = (size_t)1 << log_n, bytes = n_cols * n * sizeof(Fr);
  if (src) ZK_CK(zk_copy_d2d(ctx, data, src, bytes));
  const Fr *tw = inverse ? dom->inv29 : dom->fwd29;
  for (int s = log_n - 1; s >= 0; --s) {
    k_dif_stage<<<zk_blocks(n_cols * (n / 2), 256), 256, 0, ctx->stream>>>(data, data, n_cols, log_n, s, tw);
    ZK_LAUNCH_CHECK(ctx);
  }
  if (log_n == 2 || inverse) {
    void *p;
    ZK_CK(zk_scratch(ctx, 0, bytes, &p));
    Fr *tmp = (Fr *)p;
    ZK_CK(zk_copy_d2d(ctx, tmp, data, bytes));   // the snapshot is taken for every inverse, n = 2 included, where nothing reads it
    if (log_n == 2) {
      ZK_HIP(ctx, hipMemcpy2DAsync(data + 1, 4 * sizeof(Fr), tmp + 2, 4 * sizeof(Fr), sizeof(Fr), n_cols, hipMemcpyDeviceToDevice, ctx->stream));
      ZK_HIP(ctx, hipMemcpy2DAsync(data + 2, 4 * sizeof(Fr), tmp + 1, 4 * sizeof(Fr), sizeof(Fr), n_cols, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (inverse) ZK_CK(zkfhe_fr_scale(ctx, (const zkfhe_fr *)data, (const zkfhe_fr *)&dom->n_inv, (zkfhe_fr *)data, n_cols * n));
  }
  return ZKFHE_OK;
}

// 8 <= n <= 2^13: one tile per column
int ntt_one_tile(zkfhe_ctx *ctx, const Fr *src, Fr *data, size_t n_cols, int log_n, int inverse, const NttDomain *dom) {
  TileArgs a = tiles_independent(src ? src : data, data, log_n, 0, inverse ? dom->inv29 : dom->fwd29, inverse ? dom->n_inv29_dev : nullptr);
  if (log_n == NTT_TILE_LOG && a.in == a.out) {
    // the 2^13 tile cuts a column into two workgroups that both read all of it: in place it goes through scratch
    const size_t bytes = (n_cols << log_n) * sizeof(Fr);
    void *p;
    ZK_CK(zk_scratch(ctx, 0, bytes, &p));
    a.out = (Fr *)p;
    ZK_CK(launch_tile_dyn(ctx, log_n, a, 1, (unsigned)n_cols));
    return zk_copy_d2d(ctx, data, p, bytes);
  }
  return launch_tile_dyn(ctx, log_n, a, 1, (unsigned)n_cols);
}

// One pass of a plan (ntt_plan.hpp) over all rows.  pre: the coset powers, read by the pass that carries the multiplier.
int ntt_run_pass(zkfhe_ctx *ctx, const NttPass &ps, const Fr *in, Fr *out, size_t n_cols, int log_n, int inverse, const Fr *tw, const Fr *pre, unsigned rows,
                 const Fr *shifts_host) {
  const size_t n = (size_t)1 << log_n;
  if (!ps.coset) pre = nullptr;
  if (ps.kind == NTT_FOUR_STEP) return zk_dif8_pass(ctx, in, out, n_cols, log_n, ps.S, inverse, ps.coset ? shifts_host : nullptr, ps.coset ? rows : 1u);
  if (ps.kind == NTT_LDS) {
    const size_t tiles = n_cols * (n >> 10);
    unsigned grid = (unsigned)(tiles < (size_t)ctx->num_cu * 64 ? tiles : (size_t)ctx->num_cu * 64);
    if (ps.S == 6) k_dif_lds<3><<<grid, 128, 0, ctx->stream>>>(in, out, n_cols, log_n, ps.log_half, tw, pre, rows);
    else if (ps.S == 5) k_dif_lds<2><<<grid, 128, 0, ctx->stream>>>(in, out, n_cols, log_n, ps.log_half, tw, pre, rows);
    else k_dif_lds<1><<<grid, 128, 0, ctx->stream>>>(in, out, n_cols, log_n, ps.log_half, tw, pre, rows);
  } else {
    unsigned grid = zk_blocks(n_cols * (n >> ps.S), 256);
    unsigned cap = (unsigned)ctx->num_cu * 16;
    if (grid > cap) grid = cap;
    if (ps.S == 3) k_dif_fused<3><<<grid, 256, 0, ctx->stream>>>(in, out, n_cols, log_n, ps.log_half, tw, pre, rows);
    else if (ps.S == 2) k_dif_fused<2><<<grid, 256, 0, ctx->stream>>>(in, out, n_cols, log_n, ps.log_half, tw, pre, rows);
    else k_dif_stage<<<grid, 256, 0, ctx->stream>>>(in, out, n_cols, log_n, ps.log_half, tw, pre, rows);
  }
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

// 2^14 <= n <= 2^26: the plan's passes bring every row down to 2^13 blocks, the tile kernel transforms each block and scatters it
// to natural order.  What runs, and through which buffers, is ntt_plan.hpp.
int ntt_long_rows(zkfhe_ctx *ctx, const Fr *src, Fr *data, size_t n_cols, int log_n, int inverse, const NttDomain *dom, const Fr *pre, unsigned rows,
                  const Fr *shifts_host) {
  static const bool lds_pass = ntt_lds_pass_enabled(getenv("ZKFHE_NTT_LDS_PASS"));
  const size_t bytes = (n_cols << log_n) * sizeof(Fr);
  void *work;
  ZK_CK(zk_scratch(ctx, 0, bytes, &work));
  const NttPlan plan = ntt_plan(log_n, inverse != 0, src == nullptr, pre ? NTT_COSET_PRE : shifts_host ? NTT_COSET_SHIFTS : NTT_COSET_NONE, rows, lds_pass);
  if (plan.refused) return zk_fail_msg(ctx, ZKFHE_EINVAL, "bad argument: coset shifts on the host take a four-step size (2^16, 2^19) and at most four rows");
  const Fr *rd[3] = {src, data, (const Fr *)work};   // indexed by NttBuf
  Fr *wr[3] = {nullptr, data, (Fr *)work};           // no pass writes the source
  const Fr *tw = inverse ? dom->inv29 : dom->fwd29;
  for (int i = 0; i < plan.n_passes; ++i) ZK_CK(ntt_run_pass(ctx, plan.pass[i], rd[plan.pass[i].in], wr[plan.pass[i].out], n_cols, log_n, inverse, tw, pre, rows, shifts_host));
  const NttDomain *tdom;
  ZK_CK(zk_domain(ctx, NTT_TILE_LOG, &tdom));
  const TileArgs a = tiles_scatter(rd[plan.tile_in], wr[plan.tile_out], log_n, inverse ? tdom->inv29 : tdom->fwd29, inverse ? dom->n_inv29_dev : nullptr);
  ZK_CK(launch_tile_dyn(ctx, NTT_TILE_LOG, a, 1u << a.log_tiles, (unsigned)n_cols));
  if (plan.copy_back) ZK_CK(zk_copy_d2d(ctx, data, work, bytes));
  return ZKFHE_OK;
}

// src == nullptr: in place on cols_dev.  pre / shifts_host (long rows, forward, out of place only): the n_cols transforms are
// `rows` coset rows of the n_cols / rows vectors at src, each multiplied by the powers of its coset shift as the first pass loads it
// -- pre holds the powers ([rows][n], 2^261 form), shifts_host the `rows` shifts themselves (2^16 and 2^19, up to four rows).
int zk_ntt_impl(zkfhe_ctx *ctx, const zkfhe_fr *src_dev, zkfhe_fr *cols_dev, size_t n_cols, int log_n, int inverse, const Fr *pre = nullptr, unsigned rows = 1,
                const Fr *shifts_host = nullptr) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, (pre == nullptr && shifts_host == nullptr) || (src_dev != nullptr && !inverse && log_n > 13 && rows >= 1 && n_cols % rows == 0));
  ZK_ARG(ctx, !(pre && shifts_host));
  ZK_ARG(ctx, log_n >= 1 && log_n <= 26);
  if (!n_cols) return ZKFHE_OK;
  ZK_ARG(ctx, cols_dev != nullptr);
  ZK_ARG(ctx, n_cols < 65536);
  const NttDomain *dom;
  ZK_CK(zk_domain(ctx, log_n, &dom));
  if (log_n < 3) return ntt_tiny(ctx, (const Fr *)src_dev, (Fr *)cols_dev, n_cols, log_n, inverse, dom);
  if (log_n <= NTT_TILE_LOG) return ntt_one_tile(ctx, (const Fr *)src_dev, (Fr *)cols_dev, n_cols, log_n, inverse, dom);
  return ntt_long_rows(ctx, (const Fr *)src_dev, (Fr *)cols_dev, n_cols, log_n, inverse, dom, pre, rows, shifts_host);
}

// the shifts g w_ext^k1 of the first `rows` cosets (rows <= 8: the extension factor is at most 2^3)
void coset_shifts(const Fr &g, const Fr &w_ext, int rows, Fr (&out)[8]) {
  Fr shift = g;
  for (int k1 = 0; k1 < rows; ++k1) {
    out[k1] = shift;
    shift = shift * w_ext;
  }
}

// The second half of extended_to_coeff: the scale table 2^-lef g^-j, j < n 2^lef, into scratch slot 1, then k_ext_combine over
// the inverse-transformed coset rows.
int ext_combine(zkfhe_ctx *ctx, const Fr *rows, Fr *out, size_t n_cols, int log_n, int lef, const Fr &g, const NttDomain *edom) {
  const size_t n = (size_t)1 << log_n, ne = n << lef;
  void *p;
  ZK_CK(zk_scratch(ctx, 1, ne * sizeof(Fr), &p));
  Fr *scale = (Fr *)p;
  const Fr einv = fp_inv<FrP>(zk_fr_from_u64((uint64_t)1 << lef));
  const Fr ginv = fp_inv<FrP>(g);
  k_pow_table_scaled<<<zk_blocks(ne, 256), 256, 0, ctx->stream>>>(zk_fr_to_29(einv), ginv, scale, ne);
  ZK_LAUNCH_CHECK(ctx);
  const unsigned grid = zk_blocks(n_cols * n, 256);
  if (lef == 1) k_ext_combine<1><<<grid, 256, 0, ctx->stream>>>(rows, out, n_cols, log_n, edom->inv29, scale);
  else if (lef == 2) k_ext_combine<2><<<grid, 256, 0, ctx->stream>>>(rows, out, n_cols, log_n, edom->inv29, scale);
  else k_ext_combine<3><<<grid, 256, 0, ctx->stream>>>(rows, out, n_cols, log_n, edom->inv29, scale);
  ZK_LAUNCH_CHECK(ctx);
  return ZKFHE_OK;
}

}  // namespace

// Forward coset extension of the first `rows` cosets only (rows <= 2^lef; more are cut to 2^lef), written DENSELY: column c, coset
// k1 at out + (c * rows + k1) * n.  The prover's quotient has degree < 3n, so three of the four cosets determine it.  Row k1 is
// the transform of x[i] (g w_ext^k1)^i, and the powers reach the kernels in one of three ways:
//   n = 2^13: the tile's own tables (powers times the first-stage twiddles), built once per (g, lef, rows) by zk_pre13;
//   n = 2^16, 2^19 and up to four rows: the four-step pass folds them into its (cached) tables, from the shifts alone;
//   otherwise: a table of powers per call in scratch slot 1, filled here -- the only writer of that slot on the forward path --
//     and read by the first pass of the transform (long rows) or by the tile as it loads.
int zk_coset_ntt_rows(zkfhe_ctx *ctx, const Fr *in_dev, Fr *out_dev, size_t n_cols, int log_n, int lef, const Fr &g, int rows) {
  if (rows > (1 << lef)) rows = 1 << lef;
  if (!n_cols) return ZKFHE_OK;
  const size_t n = (size_t)1 << log_n, n_rows = n_cols * (size_t)rows;
  const NttDomain *dom, *edom;
  ZK_CK(zk_domain(ctx, log_n, &dom));
  ZK_CK(zk_domain(ctx, log_n + lef, &edom));
  if (log_n == NTT_TILE_LOG) {
    const void *pre13;
    ZK_CK(zk_pre13(ctx, g, lef, rows, false, &pre13));
    return launch_tile_dyn(ctx, log_n, tiles_fan_out(in_dev, out_dev, log_n, lef, rows, dom->fwd29, nullptr, pre13), (unsigned)rows, (unsigned)n_cols);
  }
  Fr shifts[8];
  coset_shifts(g, edom->omega, rows, shifts);
  if (ntt_four_step_size(log_n) && rows <= 4) return zk_ntt_impl(ctx, (const zkfhe_fr *)in_dev, (zkfhe_fr *)out_dev, n_rows, log_n, 0, nullptr, (unsigned)rows, shifts);
  void *p;
  ZK_CK(zk_scratch(ctx, 1, (size_t)rows * n * sizeof(Fr), &p));
  Fr *pre = (Fr *)p;
  const Fr c32 = zk_fr_to_29(Fr::one());
  for (int k1 = 0; k1 < rows; ++k1) {   // (g w_ext^k1)^i as constant operands of the nine-limb multiply (2^261 form)
    k_pow_table_scaled<<<zk_blocks(n, 256), 256, 0, ctx->stream>>>(c32, shifts[k1], pre + (size_t)k1 * n, n);
    ZK_LAUNCH_CHECK(ctx);
  }
  // long rows: one out-of-place transform of all (column, coset) rows into the destination, whose first pass multiplies by the powers
  if (log_n > NTT_TILE_LOG) return zk_ntt_impl(ctx, (const zkfhe_fr *)in_dev, (zkfhe_fr *)out_dev, n_rows, log_n, 0, pre, (unsigned)rows);
  return launch_tile_dyn(ctx, log_n, tiles_fan_out(in_dev, out_dev, log_n, lef, rows, dom->fwd29, pre, nullptr), (unsigned)rows, (unsigned)n_cols);
}

// lagrange_to_coeff followed by coeff_to_extended on `rows` cosets, for the prover's extend step.  At n = 2^13 the inverse
// transform runs out of place WITHOUT its final n^-1 (one product per coefficient less) and the coset tables carry the factor.
int zk_extend_lagrange(zkfhe_ctx *ctx, const Fr *lagr_dev, Fr *tmp_dev, Fr *out_dev, size_t n_cols, int log_n, int lef, const Fr &g, int rows) {
  if (!n_cols) return ZKFHE_OK;
  if (log_n != NTT_TILE_LOG || rows > (1 << lef)) {
    ZK_CK(zk_ntt_impl(ctx, (const zkfhe_fr *)lagr_dev, (zkfhe_fr *)tmp_dev, n_cols, log_n, 1));   // out of place: no copy
    return zk_coset_ntt_rows(ctx, tmp_dev, out_dev, n_cols, log_n, lef, g, rows);
  }
  const NttDomain *dom;
  ZK_CK(zk_domain(ctx, log_n, &dom));
  const void *pre13;
  ZK_CK(zk_pre13(ctx, g, lef, rows, true, &pre13));
  ZK_CK(launch_tile_dyn(ctx, log_n, tiles_independent(lagr_dev, tmp_dev, log_n, 0, dom->inv29, nullptr), 1, (unsigned)n_cols));
  return launch_tile_dyn(ctx, log_n, tiles_fan_out(tmp_dev, out_dev, log_n, lef, rows, dom->fwd29, nullptr, pre13), (unsigned)rows, (unsigned)n_cols);
}

extern "C" {

int zkfhe_ntt_batch(zkfhe_ctx *ctx, zkfhe_fr *cols_dev, size_t n_cols, int log_n, int inverse) { return zk_ntt_impl(ctx, nullptr, cols_dev, n_cols, log_n, inverse); }

int zkfhe_ntt_batch_to(zkfhe_ctx *ctx, const zkfhe_fr *in_dev, zkfhe_fr *out_dev, size_t n_cols, int log_n, int inverse) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, in_dev != nullptr && out_dev != nullptr && log_n >= 0 && log_n < 40);
  {
    // "not overlapping" is enforced, not only documented: at n = 2^13 two workgroups per column read all of it while the other
    // writes, and a partial overlap would corrupt the result silently
    const Fr *i0 = (const Fr *)in_dev, *o0 = (const Fr *)out_dev;
    const size_t span = n_cols << log_n;
    if (!(i0 + span <= o0 || o0 + span <= i0)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "zkfhe_ntt_batch_to: input and output must not overlap (zkfhe_ntt_batch transforms in place)");
  }
  return zk_ntt_impl(ctx, in_dev, out_dev, n_cols, log_n, inverse);
}

// forward: coeff_to_extended, row k1 of a column = NTT_n of x[i] (g w_ext^k1)^i (zk_coset_ntt_rows with every coset);
// inverse: extended_to_coeff, the row iNTTs (size n, scaled by n^-1) into scratch, then k_ext_combine across k1
int zkfhe_coset_ntt_batch(zkfhe_ctx *ctx, const zkfhe_fr *in_dev, zkfhe_fr *out_dev, size_t n_cols, int log_n,
                          int log_ext_factor, const zkfhe_fr *g_host, int inverse) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, log_n >= 3 && log_n + log_ext_factor <= 26);
  ZK_ARG(ctx, log_ext_factor >= 1 && log_ext_factor <= 3);
  ZK_ARG(ctx, g_host != nullptr);
  if (!n_cols) return ZKFHE_OK;
  ZK_ARG(ctx, in_dev != nullptr && out_dev != nullptr && n_cols < 65536);
  const int lef = log_ext_factor, E = 1 << lef;
  Fr g;
  memcpy(&g, g_host, 32);
  if (!inverse) return zk_coset_ntt_rows(ctx, (const Fr *)in_dev, (Fr *)out_dev, n_cols, log_n, lef, g, E);
  const NttDomain *dom, *edom;
  ZK_CK(zk_domain(ctx, log_n, &dom));
  ZK_CK(zk_domain(ctx, log_n + lef, &edom));
  const size_t bytes = ((n_cols << lef) << log_n) * sizeof(Fr);
  void *p;
  if (log_n > NTT_TILE_LOG) {
    // slot 2, not slot 0: the long-row transform takes slot 0 as its own work arena while it writes these rows
    ZK_CK(zk_scratch(ctx, 2, bytes, &p));
    ZK_CK(zk_ntt_impl(ctx, in_dev, (zkfhe_fr *)p, n_cols * E, log_n, 1));
  } else {
    ZK_CK(zk_scratch(ctx, 0, bytes, &p));   // a tile launch needs no arena of its own
    ZK_CK(launch_tile_dyn(ctx, log_n, tiles_independent((const Fr *)in_dev, (Fr *)p, log_n, lef, dom->inv29, dom->n_inv29_dev), (unsigned)E, (unsigned)n_cols));
  }
  return ext_combine(ctx, (const Fr *)p, (Fr *)out_dev, n_cols, log_n, lef, g, edom);
}

}  // extern "C"
