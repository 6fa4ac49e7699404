// The per-context prover workspace: its buffers, the named regions inside them (workspace_layout.hpp), the staging ring for the small
// tables of a proof.  Included by prover_internal.hpp, behind the helpers it uses (PT_SLOT, grid_for); allocation and release are in workspace.hip.
#pragma once
#include "workspace_layout.hpp"

struct zkfhe_bfv_pk;

struct DevBuf {
  int device = 0;  // not the context: a workspace outlives the zkfhe_ctx it was made for if the caller destroys that first
  void *p = nullptr;
  size_t bytes = 0;
  int alloc(zkfhe_ctx *c, size_t b) {
    device = c->device;
    bytes = b;
    return zkfhe_dev_alloc(c, b, &p);
  }
  void release() {
    if (p) {
      (void)hipSetDevice(device);
      (void)hipFree(p);
    }
    p = nullptr;
  }
  Fr *fr() const { return (Fr *)p; }
};

struct View {  // a slice of a larger device allocation
  void *p = nullptr;
  Fr *fr() const { return (Fr *)p; }
};

static_assert(PT_SLOT == wsl::PT_SLOT && sizeof(Fr) == wsl::FR, "workspace_layout.hpp counts in these units");

struct Workspace {
  wsl::Layout lay{};   // sizes and regions; the second-stage sizes are final once alloc_witness_buffers has run
  // every polynomial of one proof, Lagrange form, contiguous: [advice | la | ls | pz | lz | instance] (all_l) and the
  // same order on the extended coset (all_ext) -- one iNTT launch and one coset-NTT launch cover all of them
  DevBuf all_l, all_ext;
  View adv_l, la_l, ls_l, pz_l, lz_l, inst_l, adv_ext, la_ext, ls_ext, pz_ext, lz_ext, inst_ext;
  size_t inst_count = 0;   // rows of inst_l that hold public inputs of the last proof; the rest of the column is zero since allocation
  size_t n_all = 0;
  U256 *host_adv = nullptr;    // pinned [n_advice][n] witness table, reused by every proof on this context
  U256 *host_blind = nullptr;  // pinned staging for blinding rows / permuted lookup columns
  U256 *host_pool = nullptr;   // pinned staging for the coefficient arrays of the GPU witness generator
  U256 *host_poly = nullptr;   // pinned: the product of a phase-0 polynomial multiplication comes back here
  size_t host_poly_len = 0;
  uint8_t *ring = nullptr;      // pinned bump arena for the small tables of one proof: uploads from it need no host wait
  size_t ring_off = 0;
  static constexpr size_t RING_BYTES = wsl::RING_BYTES;
  // device mirror of the ring: stage() places a table in the ring and returns its address in the mirror, flush_staged() moves
  // everything staged since the last flush with ONE launch (a Fiat-Shamir round has a dozen small tables: expression groups,
  // powers, pointer / scalar lists, rotation sets ...)
  DevBuf dev_ring;
  size_t ring_flushed = 0;
  // the public inputs of the proof in flight, staged in the ring: the next flush converts them into the instance column (inst_l)
  const Fr *inst_src = nullptr;   // canonical values, in the ring (host address: the flush kernel reads the mapped ring)
  size_t inst_n = 0;
  bool inst_pending = false;
  // results that the host reads (commitments, evaluations, check flags) are WRITTEN by the kernels into this pinned,
  // device-visible block -- no device-to-host copy commands: [points | evaluations | flags]
  uint8_t *host_out = nullptr;
  size_t out_pts_cap = 0, out_ev_cap = 0;   // point slots, evaluations (0 until the block exists)
  uint8_t *host_pts = nullptr; // pinned: the phase-0 commitments (PT_SLOT bytes each), read after ev_pts
  hipEvent_t ev_pts = nullptr;
  // the random polynomial of the vanishing argument depends on no challenge: it is uploaded and committed at the start of
  // the proof on an auxiliary context (own stream, scratch and tickets) beside the phase-0 / witness work
  zkfhe_ctx *aux = nullptr;
  uint8_t *host_rand_pt = nullptr;  // pinned: the commitment (one PT_SLOT)
  hipEvent_t ev_rand = nullptr;
  // early phase-1 commitment (everything that does not depend on the phase-1 challenge): points + lookup error flag, pinned
  uint8_t *host_early = nullptr;   // PT_SLOT bytes per point
  int *host_early_err = nullptr;
  hipEvent_t ev_early = nullptr;
  DevBuf stream, pool, invtmp;  // device: phase-1 gate stream, coefficient arrays, deferred inverses
  DevBuf tmp_c, partials, h_ext, h_c, misc, points, num, den, small, evout, polyio;
  DevBuf qgather;   // one proof over W GPUs: the W shares of the quotient, [coset row][rank][n] (grow_qgather, by the first sharded proof)

  // the buffer behind an entry of the layout: a device buffer, or the pinned pointer
  DevBuf *device_buf(wsl::Buf b) {
    DevBuf *const d[] = {&all_l, &all_ext, &tmp_c, &partials, &h_ext, &h_c, &misc, &points, &num, &den, &small, &evout, &polyio, &stream, &pool, &invtmp, &dev_ring, &qgather};
    static_assert(sizeof(d) / sizeof(d[0]) == wsl::HOST_ADV, "one entry per device buffer of wsl::Buf, in its order");
    return d[b];
  }
  void **pinned_buf(wsl::Buf b) {
    void **const h[] = {(void **)&host_adv, (void **)&host_blind, (void **)&host_pool, (void **)&host_poly, (void **)&ring, (void **)&host_out, (void **)&host_pts,
                        (void **)&host_early, (void **)&host_early_err, (void **)&host_rand_pt};
    static_assert(sizeof(h) / sizeof(h[0]) == wsl::N_BUFS - wsl::HOST_ADV, "one entry per pinned buffer of wsl::Buf, in its order");
    return h[b - wsl::HOST_ADV];
  }
  void *base(wsl::Buf b) { return wsl::pinned(b) ? *pinned_buf(b) : device_buf(b)->p; }
  // a region of the layout: its address, and the bytes it may hold
  template <class T = Fr>
  T *at(wsl::Reg r) {
    return (T *)((char *)base(lay.reg[r].buf) + lay.reg[r].off);
  }
  size_t cap(wsl::Reg r) const { return lay.reg[r].len; }

  // one accessor per lent or carved region, named like it (workspace_layout.hpp says what each holds and when it is live):
  // ws->rand_c(), ws->sh_F(), ws->ext3_rows(), ws->out_flags() ...
#define X(name, reg, T) \
  T *name() { return at<T>(wsl::reg); }
  WSL_ACCESSORS(X)
#undef X
};

int up(zkfhe_ctx *ctx, Workspace *ws, void *dst, const void *src, size_t bytes);
int get_workspace(zkfhe_ctx *ctx, zkfhe_bfv_pk *pk, Workspace **out);
int alloc_witness_buffers(zkfhe_ctx *ctx, const zkfhe_bfv_pk *pk, Workspace *ws);   // second stage: sizes known only after keygen
int grow_qgather(zkfhe_ctx *ctx, Workspace *ws, size_t bytes);
void free_workspace(Workspace *ws);

// A small host table of the proof in flight -> device: copied into the pinned ring now, visible on the device (at the returned
// address) after the next flush_staged().  nullptr when the ring is full.  The ring is only recycled at the start of the next
// proof, after a stream sync.
static inline void *stage_table(Workspace *ws, const void *src, size_t bytes) {
  const size_t need = (bytes + 63) & ~(size_t)63;
  if (!ws->ring || !ws->dev_ring.p || ws->ring_off + need > Workspace::RING_BYTES) return nullptr;
  uint8_t *slot = ws->ring + ws->ring_off;
  memcpy(slot, src, bytes);
  void *dev = (char *)ws->dev_ring.p + ws->ring_off;
  ws->ring_off += need;
  return dev;
}
// The same for a block the caller fills in place before the next flush_staged(): *host = where to write, returns the device address
static inline void *stage_reserve(Workspace *ws, size_t bytes, void **host) {
  const size_t need = (bytes + 63) & ~(size_t)63;
  if (!ws->ring || !ws->dev_ring.p || ws->ring_off + need > Workspace::RING_BYTES) return nullptr;
  *host = ws->ring + ws->ring_off;
  void *dev = (char *)ws->dev_ring.p + ws->ring_off;
  ws->ring_off += need;
  return dev;
}
static inline int flush_staged(zkfhe_ctx *ctx, Workspace *ws) {
  // by a kernel that reads the mapped ring (zkp::k_ring_flush), not by a copy command: the runtime's copy path costs every proof of
  // a wave host time and a command of its own, and the same launch stores the instance column
  const size_t lo = ws->ring_flushed, hi = ws->ring_off;   // multiples of 64
  const size_t n16 = hi > lo ? (hi - lo) / 16 : 0;
  const size_t inst_n = ws->inst_pending ? ws->inst_n : 0, inst_zero = ws->inst_pending && ws->inst_count > ws->inst_n ? ws->inst_count - ws->inst_n : 0;
  if (n16 || ws->inst_pending) {
    if (n16 + inst_n + inst_zero) {
      zkp::k_ring_flush<<<grid_for(ctx, n16 + inst_n + inst_zero), 256, 0, ctx->stream>>>((const uint4 *)(ws->ring + lo), (uint4 *)((char *)ws->dev_ring.p + lo), n16, ws->inst_src,
                                                                                         ws->inst_l.fr(), inst_n, inst_zero);
      ZK_LAUNCH_CHECK(ctx);
    }
    ws->ring_flushed = hi;
    if (ws->inst_pending) ws->inst_count = ws->inst_n;
    ws->inst_pending = false;
  }
  return ZKFHE_OK;
}
#define STAGE(var, type, ws, src, bytes)                                                             \
  type *var = (type *)::stage_table((ws), (src), (bytes));                                                   \
  if (!var) return zk_fail_msg(ctx, ZKFHE_ENOMEM, "the proof's small tables do not fit the staging ring")
