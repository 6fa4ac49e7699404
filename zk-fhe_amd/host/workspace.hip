// The per-context prover workspace (workspace.hpp): allocated in two stages from the layout of workspace_layout.hpp, released by it.
#include "prover_internal.hpp"

int up(zkfhe_ctx *ctx, Workspace *ws, void *dst, const void *src, size_t bytes) {
  if (!bytes) return ZKFHE_OK;
  const size_t need = (bytes + 63) & ~(size_t)63;
  if (!ws->ring || ws->ring_off + need > Workspace::RING_BYTES) return zkfhe_upload(ctx, dst, src, bytes);
  uint8_t *slot = ws->ring + ws->ring_off;
  ws->ring_off += need;
  memcpy(slot, src, bytes);
  ZK_HIP(ctx, zk_memcpy_async(ctx, dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
  return ZKFHE_OK;
}

static wsl::Shape shape_of(const zkfhe_bfv_pk *pk) {
  const CircuitConfig &c = pk->cfg;
  return wsl::Shape{c.n(),     (unsigned)pk->ext_rows, c.n_advice(), c.n_fixed(), c.n_gate(),      c.n_gate0,      c.n_rlc,
                    c.n_lookup, c.n_perm(),             c.n_chunks(), pk->prm.N,   pk->gate1_cells, pk->n_inv_slots};
}

// every buffer of one stage, at the size the layout gives it
static int alloc_stage(zkfhe_ctx *ctx, Workspace *ws, bool second) {
  if (!wsl::consistent(ws->lay)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "prover workspace layout is inconsistent");
  for (unsigned i = 0; i < wsl::N_BUFS; ++i) {
    const wsl::Buf b = (wsl::Buf)i;
    if (wsl::second_stage(b) != second || b == wsl::QGATHER) continue;
    if (wsl::pinned(b)) ZK_HIP(ctx, hipHostMalloc(ws->pinned_buf(b), ws->lay.bytes[b], hipHostMallocDefault));
    else CK(ws->device_buf(b)->alloc(ctx, ws->lay.bytes[b]));
  }
  return ZKFHE_OK;
}

static int alloc_workspace(zkfhe_ctx *ctx, const zkfhe_bfv_pk *pk, Workspace *ws) {
  const CircuitConfig &c = pk->cfg;
  // the widest lists of ws->small: beta * delta^i per permutation column, the chunk / lookup totals
  if ((size_t)c.n_perm() > wsl::SMALL_SLOTS || (size_t)c.n_chunks() + c.n_lookup > wsl::SMALL_SLOTS)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "configuration too wide for the prover workspace (more than 4096 permutation columns)");
  ws->lay = wsl::make(shape_of(pk));   // gate1_cells and n_inv_slots are not known yet during keygen: no size of this stage reads them
  ws->n_all = ws->lay.n_all;
  CK(alloc_stage(ctx, ws, false));
  View *const views[] = {&ws->adv_l, &ws->la_l, &ws->ls_l, &ws->pz_l, &ws->lz_l, &ws->inst_l, &ws->adv_ext, &ws->la_ext, &ws->ls_ext, &ws->pz_ext, &ws->lz_ext, &ws->inst_ext};
  for (unsigned r = wsl::ADV_L; r <= wsl::INST_EXT; ++r) views[r]->p = ws->at((wsl::Reg)r);
  ZK_HIP(ctx, zk_memset_async(ctx, ws->inst_l.p, 0, c.n() * 32, ctx->stream));   // the prover only ever writes the public-input rows
  ws->inst_count = 0;
  memset(ws->host_adv, 0, ws->lay.bytes[wsl::HOST_ADV]);
  return ZKFHE_OK;
}

// buffers of the GPU witness generator and the pinned result blocks (sizes known only after keygen)
int alloc_witness_buffers(zkfhe_ctx *ctx, const zkfhe_bfv_pk *pk, Workspace *ws) {
  if (ws->stream.p) return ZKFHE_OK;
  ws->lay = wsl::make(shape_of(pk));
  CK(alloc_stage(ctx, ws, true));
  ws->host_poly_len = ws->lay.bytes[wsl::HOST_POLY] / 32;
  ws->out_pts_cap = ws->cap(wsl::OUT_POINTS) / PT_SLOT;
  ws->out_ev_cap = ws->cap(wsl::OUT_EVALS) / 32;
  memset(ws->host_out, 0, ws->lay.bytes[wsl::HOST_OUT]);
  ZK_HIP(ctx, hipEventCreateWithFlags(&ws->ev_pts, hipEventDisableTiming | hipEventBlockingSync));
  ZK_HIP(ctx, hipEventCreateWithFlags(&ws->ev_rand, hipEventDisableTiming | hipEventBlockingSync));
  ZK_HIP(ctx, hipEventCreateWithFlags(&ws->ev_early, hipEventDisableTiming | hipEventBlockingSync));
  if (zkfhe_ctx_create(ctx->device, nullptr, &ws->aux)) return zk_fail_msg(ctx, ZKFHE_EHIP, std::string("auxiliary context: ") + zkfhe_last_error(nullptr));
  return ZKFHE_OK;
}

// the buffer of the gathered shares of a sharded proof (quotient rows, SHPLONK sets), grown to `bytes`
int grow_qgather(zkfhe_ctx *ctx, Workspace *ws, size_t bytes) {
  if (ws->qgather.bytes >= bytes) return ZKFHE_OK;
  CK(zkfhe_sync(ctx));
  ws->qgather.release();
  return ws->qgather.alloc(ctx, bytes);
}

static void release_buffers(Workspace *ws) {
  for (unsigned i = 0; i < wsl::N_BUFS; ++i) {
    const wsl::Buf b = (wsl::Buf)i;
    if (!wsl::pinned(b)) {
      ws->device_buf(b)->release();
    } else if (*ws->pinned_buf(b)) {
      (void)hipHostFree(*ws->pinned_buf(b));
      *ws->pinned_buf(b) = nullptr;
    }
  }
}

void free_workspace(Workspace *ws) {
  (void)hipSetDevice(ws->all_l.device);
  release_buffers(ws);
  if (ws->ev_pts) (void)hipEventDestroy(ws->ev_pts);
  if (ws->ev_rand) (void)hipEventDestroy(ws->ev_rand);
  if (ws->ev_early) (void)hipEventDestroy(ws->ev_early);
  if (ws->aux) (void)zkfhe_ctx_destroy(ws->aux);
  delete ws;
}

int get_workspace(zkfhe_ctx *ctx, zkfhe_bfv_pk *pk, Workspace **out) {
  std::lock_guard<std::mutex> lock(pk->mu);
  auto it = pk->workspaces.find(ctx->uid);
  if (it == pk->workspaces.end()) {
    Workspace *ws = new Workspace();
    int rc = alloc_workspace(ctx, pk, ws);
    if (rc) {
      release_buffers(ws);
      delete ws;
      return rc;
    }
    it = pk->workspaces.emplace(ctx->uid, ws).first;
  }
  if (it->second->all_l.device != ctx->device) return zk_fail_msg(ctx, ZKFHE_EINVAL, "prover workspace belongs to another device");
  *out = it->second;
  return ZKFHE_OK;
}
