// Shared declarations of the circuit-level translation units (srs.hip, keygen.hip, prove.hip): handles, the per-context
// workspace, small host helpers.  Not part of the public ABI.
#pragma once
#include <chrono>
#include <ctime>
#include <cstdio>
#include <cstring>
#include <map>
#include <atomic>
#include <mutex>
#include <thread>
#include <stdexcept>

#include "../../include/zkfhe.h"
#include "bfv_circuit.hpp"
#include "bfv_phase0_fast.hpp"
#include "gpu_witness.hip.hpp"
#include "host_g2.hpp"    // the host G2 codec and the powers check that srs.hip borrows
#include "host_util.hpp"  // mont, mont_u64, canon, fr_pow, fr_inv, point_canon
#include "prover_kernels.hip.hpp"
#include "shplonk.hpp"
#include "transcript.hpp"
#include "prefix_cache.hpp"
#include "vk.hpp"

using namespace zkhost;
using zk::Fr;
using zk::G1Affine;

namespace zkhost {
CircuitConfig config_from_c(const zkfhe_bfv_config *c);
BfvParams params_from_c(const zkfhe_bfv_params *p);
}  // namespace zkhost

static const uint64_t COSET_G = 7;

#define CK(x)                 \
  do {                        \
    int rc__ = (x);           \
    if (rc__) return rc__;    \
  } while (0)

struct zkfhe_srs {
  uint32_t k = 0;
  zkfhe_basis *g = nullptr, *g_lagrange = nullptr;
  // the same Lagrange points with narrower windows, for columns of small values (advice, permuted lookups): their cost is
  // the per-bucket work (merge, marginals), not the additions, so 8x fewer buckets beats 30 % more windows
  zkfhe_basis *g_lagrange_small = nullptr;
  // point-range shard (zkfhe_srs_create_sharded): the bases above hold points [lo, hi) only and every commitment goes through
  // zkfhe_msm_batch_sharded over `comm`
  zkfhe_comm *comm = nullptr;
  size_t lo = 0, hi = 0;
  // what zkfhe_srs_save writes besides k: the points as they came (unsharded SRS only) and the verifier's half, raw
  // Montgomery coordinates x.c0 | x.c1 | y.c0 | y.c1
  std::vector<G1Affine> g_host, gl_host;
  uint8_t g2_raw[128], sg2_raw[128];
  bool have_g2 = false;
  // more than one rank, or a one-rank communicator with a real transport (the single-GPU test of the whole collective path)
  bool sharded() const { return comm != nullptr && zkfhe_comm_active(comm) != 0; }
};

// commitment MSM of `n_cols` full columns (stride n): the whole basis, or this rank's rows + all-gather + sum
static inline int srs_msm(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_basis *basis, const Fr *cols, size_t n_cols, G1Affine *dev_out) {
  if (!srs->sharded()) return zkfhe_msm_batch(ctx, basis, (const zkfhe_fr *)cols, n_cols, (zkfhe_g1_affine *)dev_out);
  // the collective runs on the communicator's stream: srs_join / srs_record before anything reads dev_out
  return zkfhe_msm_batch_sharded_async(ctx, srs->comm, basis, (const zkfhe_fr *)(cols + srs->lo), (size_t)1 << srs->k, n_cols, (zkfhe_g1_affine *)dev_out);
}

// Commitments the HOST reads (pinned result blocks of the workspace).  A slot is PT_SLOT = 128 bytes.  One GPU: the MSM stores
// the accumulator-form sum (zkfhe_g1_xyzz) and the host normalises all points of a Fiat-Shamir round with one field inversion
// (points_canon) -- halo2's create_proof batch-normalises a round's commitments the same way, and
// the 40 us inversion in one GPU lane at the end of every MSM call is gone.  Sharded SRS: the all-gathered partials are affine
// and so is their sum: those results are packed at a 64-byte stride in the same blocks (pt_stride).
static constexpr size_t PT_SLOT = sizeof(zk::G1X);
static inline size_t pt_stride(const zkfhe_srs *srs) { return srs->sharded() ? sizeof(G1Affine) : sizeof(zk::G1X); }
static inline int srs_msm_pts(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_basis *basis, const Fr *cols, size_t n_cols, void *pinned_out) {
  if (!srs->sharded()) return zkfhe_msm_batch_xyzz(ctx, basis, (const zkfhe_fr *)cols, n_cols, (zkfhe_g1_xyzz *)pinned_out);
  return zkfhe_msm_batch_sharded_async(ctx, srs->comm, basis, (const zkfhe_fr *)(cols + srs->lo), (size_t)1 << srs->k, n_cols, (zkfhe_g1_affine *)pinned_out);
}

static inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static inline unsigned grid_for(zkfhe_ctx *ctx, size_t work) {
  size_t b = (work + 255) / 256;
  size_t cap = (size_t)ctx->num_cu * 16;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// upload canonical values and convert to Montgomery on the device
static inline int upload_canon(zkfhe_ctx *ctx, Fr *dst, const U256 *src, size_t count) {
  ZK_HIP(ctx, zk_memcpy_async(ctx, dst, src, count * 32, hipMemcpyHostToDevice, ctx->stream));
  return zkfhe_fr_to_mont(ctx, (const zkfhe_fr *)dst, (zkfhe_fr *)dst, count);
}

#include "workspace.hpp"

// keygen.hip
int extend_cols(zkfhe_ctx *ctx, zkfhe_bfv_pk *pk, Workspace *ws, const Fr *lagr, size_t count, Fr *ext);

// commit `n_cols` columns straight into the pinned result block (the last MSM kernel stores its affine points there) and wait
static inline int commit_cols_out(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_basis *basis, const Fr *cols, size_t n_cols, Workspace *ws, std::vector<AffinePoint> &out);

// after srs_msm: host = false -> the context's stream waits for the commitments queued so far (a device-side reader follows);
// host = true -> the calling thread waits (for them and for everything queued on the context's stream before them)
static inline int srs_join(zkfhe_ctx *ctx, const zkfhe_srs *srs, bool host) {
  if (srs->sharded()) return zkfhe_comm_join(ctx, srs->comm, host ? 1 : 0);
  if (host) ZK_HIP(ctx, zk_wait(ctx));
  return ZKFHE_OK;
}
// an event behind the commitments queued so far (not behind the kernels the caller queues next)
static inline int srs_record(zkfhe_ctx *ctx, const zkfhe_srs *srs, hipEvent_t ev) {
  if (srs->sharded()) return zkfhe_comm_record_event(ctx, srs->comm, (void *)ev);
  ZK_HIP(ctx, hipEventRecord(ev, ctx->stream));
  return ZKFHE_OK;
}

// commit `n_cols` columns (device, Montgomery) and return canonical affine points
static inline int commit_cols(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_basis *basis, const Fr *cols, size_t n_cols, G1Affine *dev_out, std::vector<AffinePoint> &out) {
  CK(srs_msm(ctx, srs, basis, cols, n_cols, dev_out));
  CK(srs_join(ctx, srs, false));
  std::vector<G1Affine> h(n_cols);
  CK(zkfhe_download(ctx, h.data(), dev_out, n_cols * sizeof(G1Affine)));
  out.resize(n_cols);
  for (size_t i = 0; i < n_cols; ++i) out[i] = point_canon(h[i]);
  return ZKFHE_OK;
}

// n points of a pinned result block (written by srs_msm_pts / zkfhe_msm_sparse_xyzz, complete) -> canonical affine coordinates
static inline void points_canon(const zkfhe_srs *srs, const void *block, size_t n, AffinePoint *out) {
  if (srs->sharded()) {
    const G1Affine *a = (const G1Affine *)block;
    for (size_t i = 0; i < n; ++i) out[i] = point_canon(a[i]);
    return;
  }
  std::vector<G1Affine> a(n);
  zk::g1x_normalize_batch((const zk::G1X *)block, n, a.data());
  for (size_t i = 0; i < n; ++i) out[i] = point_canon(a[i]);
}

static inline int commit_cols_out(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_basis *basis, const Fr *cols, size_t n_cols, Workspace *ws, std::vector<AffinePoint> &out) {
  if (!ws->host_out || n_cols > ws->out_pts_cap) return commit_cols(ctx, srs, basis, cols, n_cols, (G1Affine *)ws->points.p, out);
  CK(srs_msm_pts(ctx, srs, basis, cols, n_cols, ws->out_pts()));
  CK(srs_join(ctx, srs, true));
  out.resize(n_cols);
  points_canon(srs, ws->out_pts(), n_cols, out.data());
  return ZKFHE_OK;
}

struct GpuPolyMul : PolyMulBackend {
  zkfhe_ctx *ctx;
  Workspace *ws;
  GpuPolyMul(zkfhe_ctx *c, Workspace *w) : ctx(c), ws(w) {}
  std::vector<BigInt> mul_u64(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) override;
  const U256 *mul_u64_raw(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) override;

 private:
  std::vector<U256> pageable;   // the product when it does not fit the pinned block
};


struct zkfhe_bfv_pk {
  CircuitConfig cfg;
  BfvParams prm;
  DevBuf fixed_l, sigma_l, fixed_ext, sigma_ext, l_ext, xs_ext, dpow, ext3_pw;
  std::vector<AffinePoint> fixed_commit, sigma_commit;
  U256 vk_digest;
  // structure of the phase-1 gate stream, recorded at keygen for the GPU witness generator
  size_t gate1_cells = 0, n_lookup_cells = 0, n_inv_slots = 0;
  // cosets of the extended domain the quotient is evaluated on: 3 (degree < 3n), or all 4 with ZKFHE_CHECK_QUOTIENT set when
  // the key is built (the fourth gives the degree check).  Every extended array has this many rows per column.
  int ext_rows = 3;
  DevBuf lookup_src, inv_slots, place_start, place_len;   // device: u32 lists
  // per-context prover workspaces: one proof at a time per zkfhe_ctx, any number of contexts (streams)
  // may prove concurrently against the same key (everything above is read-only after keygen)
  std::map<uint64_t, Workspace *> workspaces;   // keyed by zkfhe_ctx::uid (never reused), not by address
  std::mutex mu;
  // transcript state after `vk digest | pk0 | pk1`, per public key seen (prefix_cache.hpp); shared by the proofs in flight
  PrefixCache prefix;
  // transcript states of proofs announced ahead of time (zkfhe_bfv_pk_prehash): one-shot, consumed by the proof of the same inputs
  PreHash prehash;
};

