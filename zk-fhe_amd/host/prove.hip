// create_proof for the BFV circuit on one MI355X (include/zkfhe.h "prove"): replaces halo2 `create_proof` with
// ProverSHPLONK as driven by snark-verifier-sdk `gen_snark_shplonk` (third-party, reached from reference
// examples/bfv.rs:311; protocol restated in oracle/halo2_ref.py, which this file must match byte for byte for the same
// seed).  Host side: phase-0 witness (bfv_circuit.hpp), Fiat-Shamir transcript.  Device side: everything that touches a
// full column -- the phase-1 witness, blinding, MSM commits, (i)NTT / coset NTT, grand products, quotient evaluation,
// evaluations at x, SHPLONK polynomials.
#include "prover_internal.hpp"

namespace {

// counting-sort restatement of halo2's permute_expression_pair for 8-bit tables
void permute_lookup(const std::vector<U256> &input, size_t u, unsigned table_size, std::vector<U256> &a_perm, std::vector<U256> &s_perm) {
  std::vector<size_t> cnt(table_size, 0);
  for (size_t i = 0; i < u; ++i) {
    const U256 &v = input[i];
    if (v.l[1] | v.l[2] | v.l[3] || v.l[0] >= table_size) throw std::runtime_error("lookup input not in table");
    ++cnt[v.l[0]];
  }
  // table multiset over usable rows: values 0..table_size-1 once each, and 0 for the remaining rows
  std::vector<size_t> left(table_size, 1);
  left[0] = u - (table_size - 1);
  a_perm.assign(u, fe::zero());
  s_perm.assign(u, fe::zero());
  std::vector<size_t> holes;
  size_t pos = 0;
  for (unsigned v = 0; v < table_size; ++v)
    for (size_t k = 0; k < cnt[v]; ++k, ++pos) {
      a_perm[pos] = fe::from_u64(v);
      if (k == 0) {
        if (!left[v]) throw std::runtime_error("lookup input not in table");
        --left[v];
        s_perm[pos] = fe::from_u64(v);
      } else {
        holes.push_back(pos);
      }
    }
  size_t hi = 0;
  for (unsigned v = 0; v < table_size; ++v)
    for (size_t k = 0; k < left[v]; ++k) s_perm[holes[hi++]] = fe::from_u64(v);
}

// ---------------------------------------------------------------------------------------------------------------
// Phase-1 gate context on the GPU: the device twin of bfv_phase1 (examples/bfv.rs:167-304 through src/poly_chip.rs).
// One launch per PolyChip call, one thread per coefficient; the stream offset of every call is a pure function of
// the circuit shape and is cross-checked against the stream length recorded at keygen.
struct DevPoly {
  Fr *d = nullptr;
  size_t len = 0;
  uint64_t bits = 0;
};

class GpuPhase1 {
 public:
  GpuPhase1(zkfhe_ctx *c, const zkfhe_bfv_pk *k, Workspace *w) : ctx(c), pk(k), ws(w) {}

  // Everything that does not depend on the phase-1 challenge: the gadget launches (the four constrain_mul gates only
  // reserve their cells) and the deferred inversions.  Enqueued behind the phase-0 commitment, so the GPU works on it
  // while the host hashes that commitment and evaluates the RLC context.
  int launch(const BfvState &st) {
    const uint64_t Q = pk->prm.Q, T = pk->prm.T, B = pk->prm.B;
    stream = ws->stream.fr();
    pool_used = 0;
    off = 0;
    calls.clear();
    call_level.clear();
    produced.clear();
    // inputs: one pinned staging block.  While they fit (k = 13: 0.66 MB) the block is a piece of the proof's staging ring and
    // goes up with the gadget arguments in ONE copy; longer inputs keep their own block and their own DMA.
    h_used = 0;
    {
      const PolyChip *ins[14] = {&st.e0, &st.e1, &st.u, &st.m, &st.pk0_u, &st.quotient_0, &st.remainder_0, &st.quotient_0_times_cyclo, &st.expected_c0,
                                 &st.pk1_u, &st.quotient_1, &st.remainder_1, &st.quotient_1_times_cyclo, &st.expected_c1};
      size_t cells = 1 + 16;   // delta, the reserved gate cells
      for (const PolyChip *pc : ins) cells += pc->assigned_coefficients.size();
      in_host = ws->host_pool;
      in_dev = ws->pool.fr();
      in_ring = false;
      void *h = nullptr;
      if (cells * 32 <= ((size_t)1 << 20)) {
        void *d = stage_reserve(ws, cells * 32, &h);
        if (d) {
          in_host = (U256 *)h;
          in_dev = (Fr *)d;
          in_ring = true;
        }
      }
    }
    DevPoly e0 = stage(st.e0), e1 = stage(st.e1), u = stage(st.u), m = stage(st.m);
    DevPoly pk0_u = stage(st.pk0_u), q0 = stage(st.quotient_0), r0 = stage(st.remainder_0), q0c = stage(st.quotient_0_times_cyclo), xc0 = stage(st.expected_c0);
    DevPoly pk1_u = stage(st.pk1_u), q1 = stage(st.quotient_1), r1 = stage(st.remainder_1), q1c = stage(st.quotient_1_times_cyclo), xc1 = stage(st.expected_c1);
    in_host[h_used] = st.delta.value;
    const Fr *delta = in_dev + h_used;
    const uint64_t delta_bits = st.delta.value.bits();
    ++h_used;
    // the four gate cells of each constrain_mul (filled in by finish()), staged after the inputs
    mg_slot = h_used;
    n_mg = 0;
    h_used += 16;
    pool_used = h_used;
    if (!in_ring) ZK_HIP(ctx, zk_memcpy_async(ctx, ws->pool.p, ws->host_pool, mg_slot * 32, hipMemcpyHostToDevice, ctx->stream));

    CK(in_range(e0, B, Q));
    CK(in_range(e1, B, Q));
    CK(gadget(zkw::G_CHI_KEY, u, nullptr, nullptr, zkw::cpc_chi_key(), Q - 1, 0, Fr::zero()));
    CK(in_range(m, T / 2, Q));
    const int n_side = 2;
    for (int side = 0; side < n_side; ++side) {
      const DevPoly &pku = side ? pk1_u : pk0_u, &q = side ? q1 : q0, &r = side ? r1 : r0, &qc = side ? q1c : q0c;
      CK(mul_gate());                                                    // pk_i * u = pk_i_u
      DevPoly pku_r;
      CK(reduce_by_modulo(pku, Q, pku_r));
      CK(in_field(q, Q));
      CK(in_field(r, Q));
      // reduce_by_cyclo (src/poly_chip.rs:183-223)
      CK(mul_gate());                                                    // quotient * cyclo = quotient_times_cyclo
      DevPoly sum, sum_mod;
      CK(add(qc, r, sum));
      CK(reduce_by_modulo(sum, Q, sum_mod));
      if (sum_mod.len < pku_r.len) return zk_fail_msg(ctx, ZKFHE_EINVAL, "degree <= self.degree (src/poly_chip.rs:375)");
      DevPoly trimmed{sum_mod.d + (sum_mod.len - pku_r.len), pku_r.len, sum_mod.bits};
      CK(equal(trimmed, pku_r));
      const size_t N = pk->prm.N;
      if (r.len < N) return zk_fail_msg(ctx, ZKFHE_EINVAL, "degree <= self.degree (src/poly_chip.rs:375)");
      DevPoly acc{r.d + (r.len - N), N, r.bits};
      if (side == 0) {
        DevPoly m_delta, t;
        CK(scalar_mul(m, delta, delta_bits, m_delta));
        CK(add(acc, m_delta, t));
        CK(add(t, e0, acc));
      } else {
        DevPoly t;
        CK(add(acc, e1, t));
        acc = t;
      }
      DevPoly c_red;
      CK(reduce_by_modulo(acc, Q, c_red));
      CK(equal(c_red, side ? xc1 : xc0));
    }
    if (off != pk->gate1_cells) return zk_fail_msg(ctx, ZKFHE_EINVAL, "GPU witness stream length differs from the keygen circuit shape");
    CK(launch_levels());
    // deferred 1/x cells of is_zero: one batch inversion over the structural slot list
    if (pk->n_inv_slots) {
      const unsigned g = (unsigned)((pk->n_inv_slots + 255) / 256);
      zkw::k_gather<<<g, 256, 0, ctx->stream>>>(stream, (const unsigned *)pk->inv_slots.p, pk->n_inv_slots, ws->invtmp.fr());
      ZK_LAUNCH_CHECK(ctx);
      CK(zkfhe_fr_batch_invert(ctx, (zkfhe_fr *)ws->invtmp.p, pk->n_inv_slots));
      zkw::k_scatter<<<g, 256, 0, ctx->stream>>>(stream, (const unsigned *)pk->inv_slots.p, pk->n_inv_slots, ws->invtmp.fr());
      ZK_LAUNCH_CHECK(ctx);
    }
    return ZKFHE_OK;
  }

  // Everything of phase 1 except the cells that depend on the challenge: the reserved constrain_mul cells stay zero in the
  // stream, then stream -> gate columns (break points) and lookup columns.  The columns can be committed from here on;
  // patch() supplies the missing cells and the correction columns.
  int place_early(const zkp::RngRows &blind, unsigned zero_cols) {
    zkw::ZeroRuns z{};
    z.count = n_mg;
    for (unsigned i = 0; i < n_mg; ++i) z.at[i] = stream + mg_off[i];
    zkw::k_zero_runs<<<1, 64, 0, ctx->stream>>>(z);
    ZK_LAUNCH_CHECK(ctx);
    return place(blind, zero_cols);
  }
  // (gate column, row) of every reserved cell -- twice for a cell on a break point, whose value is repeated at the top of the
  // next column.  columns: the distinct affected gate columns, in ascending order.
  struct PatchPlan {
    std::vector<unsigned> columns;
    struct Cell {
      unsigned col_slot, row, value;
    };
    std::vector<Cell> cells;
  };
  PatchPlan patch_plan() const {
    PatchPlan p;
    const CircuitConfig &cfg = pk->cfg;
    std::vector<size_t> start(cfg.n_gate1, 0), len(cfg.n_gate1, 0);
    size_t s = 0;
    for (unsigned c = 0; c < cfg.n_gate1 && s < pk->gate1_cells; ++c) {
      start[c] = s;
      if (c < cfg.bp_gate1.size()) {
        len[c] = (size_t)cfg.bp_gate1[c] + 1;
        s += cfg.bp_gate1[c];
      } else {
        len[c] = pk->gate1_cells - s;
        s = pk->gate1_cells;
      }
    }
    for (unsigned i = 0; i < n_mg; ++i)
      for (unsigned j = 0; j < 4; ++j) {
        const size_t o = mg_off[i] + j;
        for (unsigned c = 0; c < cfg.n_gate1; ++c)
          if (len[c] && o >= start[c] && o < start[c] + len[c]) {
            size_t slot = std::find(p.columns.begin(), p.columns.end(), c) - p.columns.begin();
            if (slot == p.columns.size()) p.columns.push_back(c);
            p.cells.push_back({(unsigned)slot, (unsigned)(o - start[c]), 4 * i + j});
          }
      }
    return p;
  }
  // evals as in finish(): writes the reserved cells into the advice columns and into patch_cols[slot][row] (zeroed here);
  // terms (optional): the same cells as sparse MSM terms (row, slot, scalar)
  int patch(const U256 evals[12], const PatchPlan &plan, Fr *patch_cols, std::vector<zkfhe_sparse_term> *terms = nullptr) {
    const CircuitConfig &cfg = pk->cfg;
    const size_t n = cfg.n();
    Fr mg[16];
    for (int i = 0; i < 4; ++i) {
      mg[4 * i] = Fr::zero();
      for (int j = 0; j < 3; ++j) mg[4 * i + 1 + j] = mont(evals[3 * i + j]);
    }
    if (terms) {
      terms->clear();
      for (const auto &c : plan.cells) {
        if ((c.value & 3) == 0) continue;   // the first cell of a gate is the constant 0
        zkfhe_sparse_term t;
        memcpy(&t.scalar, &mg[c.value], 32);
        t.row = c.row;
        t.slot = c.col_slot;
        terms->push_back(t);
      }
    }
    if (plan.cells.size() > 64) return zk_fail_msg(ctx, ZKFHE_EINVAL, "too many challenge-dependent gate cells");
    zkw::PatchList list{};
    for (size_t t = 0; t < plan.cells.size(); ++t) {
      const auto &c = plan.cells[t];
      list.cells[t].dst_adv = ws->adv_l.fr() + ((size_t)cfg.n_gate0 + plan.columns[c.col_slot]) * n + c.row;
      list.cells[t].dst_patch = terms ? nullptr : patch_cols + (size_t)c.col_slot * n + c.row;   // dense correction columns only without the sparse MSM
      list.cells[t].value = c.value;
    }
    memcpy(list.values, mg, sizeof(mg));
    if (!terms) ZK_HIP(ctx, zk_memset_async(ctx, patch_cols, 0, plan.columns.size() * n * 32, ctx->stream));
    zkw::k_patch_cells<<<1, 64, 0, ctx->stream>>>(list, (unsigned)plan.cells.size());
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  }

  // evals[3 i .. 3 i + 2] = a(gamma), b(gamma), c(gamma) of the i-th constrain_mul: fill the reserved gate cells, then
  // stream -> gate columns (break points) and lookup columns
  int finish(const U256 evals[12], const zkp::RngRows &blind) {
    // the 16 values and their destinations are arguments of one small kernel that stores them (it used to be one upload and
    // four device copies, then a table in the staging ring)
    Fr mg[16];
    for (int i = 0; i < 4; ++i) {
      mg[4 * i] = Fr::zero();
      for (int j = 0; j < 3; ++j) mg[4 * i + 1 + j] = mont(evals[3 * i + j]);
    }
    zkw::PatchList list{};
    unsigned nc = 0;
    for (unsigned i = 0; i < n_mg; ++i)
      for (unsigned j = 0; j < 4; ++j) {
        list.cells[nc].dst_adv = stream + mg_off[i] + j;
        list.cells[nc].dst_patch = nullptr;
        list.cells[nc].value = 4 * i + j;
        ++nc;
      }
    memcpy(list.values, mg, sizeof(mg));
    if (nc) {
      zkw::k_patch_cells<<<1, 64, 0, ctx->stream>>>(list, nc);
      ZK_LAUNCH_CHECK(ctx);
    }
    return place(blind, 0);
  }

 private:
  // blind: the blinding rows u .. n - 1 of the phase-1 gate and lookup advice columns, drawn by the placement kernels (its counters
  // start at the first phase-1 gate column); zero_cols: that many columns behind the lookup columns are cleared by the same launch
  int place(const zkp::RngRows &blind, unsigned zero_cols) {
    const CircuitConfig &cfg = pk->cfg;
    const size_t n = cfg.n();
    const unsigned u = (unsigned)cfg.u();
    const unsigned g_place = grid_for(ctx, (size_t)cfg.n_gate1 * n);
    zkw::k_place<<<g_place + zkp::rng_tail_grid(blind, (size_t)cfg.n_gate1 * (n - u), 256), 256, 0, ctx->stream>>>(
        stream, (const unsigned *)pk->place_start.p, (const unsigned *)pk->place_len.p, cfg.n_gate1, n, ws->adv_l.fr() + (size_t)cfg.n_gate0 * n, blind, u, g_place);
    ZK_LAUNCH_CHECK(ctx);
    if (cfg.n_lookup) {
      if (pk->n_lookup_cells > (size_t)cfg.n_lookup * cfg.max_rows()) return zk_fail_msg(ctx, ZKFHE_EINVAL, "lookup cells do not fit the configured lookup columns");
      zkp::RngRows blind_lk = blind;
      blind_lk.ctr0 += (unsigned long long)(cfg.adv_lookup0() - cfg.n_gate0) * blind.ctr_col_stride;
      const unsigned g_lk = grid_for(ctx, (size_t)(cfg.n_lookup + zero_cols) * n);
      zkw::k_place_lookups<<<g_lk + zkp::rng_tail_grid(blind_lk, (size_t)cfg.n_lookup * (n - u), 256), 256, 0, ctx->stream>>>(
          stream, (const unsigned *)pk->lookup_src.p, pk->n_lookup_cells, (unsigned)cfg.max_rows(), n, cfg.n_lookup, ws->adv_l.fr() + (size_t)cfg.adv_lookup0() * n, blind_lk, u,
          zero_cols, g_lk);
      ZK_LAUNCH_CHECK(ctx);
    } else if (zero_cols) {
      ZK_HIP(ctx, zk_memset_async(ctx, ws->adv_l.fr() + (size_t)cfg.adv_rlc0() * n, 0, (size_t)zero_cols * n * 32, ctx->stream));
    }
    return ZKFHE_OK;
  }

  zkfhe_ctx *ctx;
  const zkfhe_bfv_pk *pk;
  Workspace *ws;
  Fr *stream = nullptr;
  size_t off = 0, pool_used = 0, h_used = 0, mg_slot = 0, mg_off[4] = {0, 0, 0, 0};
  unsigned n_mg = 0;
  U256 *in_host = nullptr;   // where the input polynomials are staged on the host ...
  Fr *in_dev = nullptr;      // ... and where the gadgets read them
  bool in_ring = false;

  DevPoly stage(const PolyChip &p) {
    DevPoly d;
    d.len = p.assigned_coefficients.size();
    d.bits = p.max_num_bits;
    d.d = in_dev + h_used;
    for (size_t i = 0; i < d.len; ++i) in_host[h_used + i] = p.assigned_coefficients[i].value;
    h_used += d.len;
    return d;
  }
  Fr *take(size_t len) {
    Fr *p = ws->pool.fr() + pool_used;
    pool_used += len;
    return p;
  }
  int gadget(int type, const DevPoly &a, const Fr *b, Fr *out, size_t cpc, uint64_t p0, uint64_t p1, const Fr &bound) {
    if (pool_used * 32 > ws->pool.bytes || (off + a.len * cpc) > pk->gate1_cells)
      return zk_fail_msg(ctx, ZKFHE_EINVAL, "GPU witness stream exceeds the keygen circuit shape");
    zkw::GadgetArgs g;
    g.type = type;
    g.a = a.d;
    g.b = b;
    g.out = out;
    g.stream = stream;
    g.base = off;
    g.cpc = cpc;
    g.count = a.len;
    g.p0 = p0;
    g.p1 = p1;
    g.bound = bound;
    // recorded in program order (the stream offsets follow examples/bfv.rs:171-301), launched level by level: a call's level
    // is one more than the level of the call that produced its inputs
    calls.push_back(g);
    call_level.push_back(level_of(a.d, a.len, b));
    if (out) produced.push_back({out, out + a.len, call_level.back()});
    off += a.len * cpc;
    return ZKFHE_OK;
  }
  struct Produced {
    const Fr *lo, *hi;
    int level;
  };
  std::vector<zkw::GadgetArgs> calls;
  std::vector<int> call_level;
  std::vector<Produced> produced;
  int level_of(const Fr *a, size_t len, const Fr *b) const {
    int lv = 0;
    for (const Produced &p : produced) {
      if (a < p.hi && a + len > p.lo) lv = std::max(lv, p.level + 1);
      if (b && b < p.hi && b + 1 > p.lo) lv = std::max(lv, p.level + 1);   // b: an array aligned with a, or one scalar
      if (b && b + len > p.lo && b < p.hi) lv = std::max(lv, p.level + 1);
    }
    return lv;
  }
  int launch_levels() {
    int max_level = 0;
    for (int l : call_level) max_level = std::max(max_level, l);
    std::vector<zkw::GadgetArgs> ordered;
    std::vector<size_t> first(max_level + 2, 0);
    for (int l = 0; l <= max_level; ++l) {
      first[l] = ordered.size();
      for (size_t i = 0; i < calls.size(); ++i)
        if (call_level[i] == l) ordered.push_back(calls[i]);
    }
    first[max_level + 1] = ordered.size();
    STAGE(dev, zkw::GadgetArgs, ws, ordered.data(), ordered.size() * sizeof(zkw::GadgetArgs));
    CK(flush_staged(ctx, ws));
    for (int l = 0; l <= max_level; ++l) {
      size_t longest = 0;
      for (size_t i = first[l]; i < first[l + 1]; ++i) longest = std::max(longest, ordered[i].count);
      if (first[l + 1] == first[l]) continue;
      zkw::k_gadget<<<dim3((unsigned)((longest + 255) / 256), (unsigned)(first[l + 1] - first[l])), 256, 0, ctx->stream>>>(dev + first[l]);
      ZK_LAUNCH_CHECK(ctx);
    }
    return ZKFHE_OK;
  }
  int in_range(const DevPoly &a, uint64_t z, uint64_t y) {
    if (!(z < y)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "z < y (src/poly_chip.rs:278)");
    return gadget(zkw::G_IN_RANGE, a, nullptr, nullptr, zkw::cpc_in_range(z, y), z, y, Fr::zero());
  }
  int in_field(const DevPoly &a, uint64_t q) { return gadget(zkw::G_IN_FIELD, a, nullptr, nullptr, zkw::cpc_in_field(q), q, 0, Fr::zero()); }
  int mul_gate() {
    if (off + 4 > pk->gate1_cells || n_mg >= 4) return zk_fail_msg(ctx, ZKFHE_EINVAL, "GPU witness stream exceeds the keygen circuit shape");
    mg_off[n_mg++] = off;
    off += 4;
    return ZKFHE_OK;
  }
  int reduce_by_modulo(const DevPoly &a, uint64_t q, DevPoly &out) {
    if (a.bits >= 192 || (q >> 63)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "reduce_by_modulo: operands too wide for the device divider (a < 2^192, q < 2^63)");
    // halo2-base div_mod: div < 2^num_bits / q + 1
    Fr bound;
    zkw::u64 rem;
    zkw::c_divmod(zkw::c_pow2((unsigned)a.bits), q, bound, rem);
    bound = zkw::c_add(bound, zkw::c_u64(1));
    out.d = take(a.len);
    out.len = a.len;
    out.bits = bits_u64(q);
    return gadget(zkw::G_DIV_MOD, a, nullptr, out.d, zkw::cpc_div_mod(q, bound), q, 0, bound);
  }
  int add(const DevPoly &a, const DevPoly &b, DevPoly &out) {
    if (b.len < a.len) return zk_fail_msg(ctx, ZKFHE_EINVAL, "add: operand lengths differ");
    out.d = take(a.len);
    out.len = a.len;
    out.bits = std::max(a.bits, b.bits) + 1;
    return gadget(zkw::G_ADD, a, b.d, out.d, 4, 0, 0, Fr::zero());
  }
  int scalar_mul(const DevPoly &a, const Fr *scalar, uint64_t scalar_bits, DevPoly &out) {
    out.d = take(a.len);
    out.len = a.len;
    out.bits = a.bits + scalar_bits;
    return gadget(zkw::G_SCALAR_MUL, a, scalar, out.d, 4, 0, 0, Fr::zero());
  }
  int equal(const DevPoly &a, const DevPoly &b) {
    if (b.len < a.len) return zk_fail_msg(ctx, ZKFHE_EINVAL, "constrain_equality: operand lengths differ");
    return gadget(zkw::G_EQUAL, a, b.d, nullptr, zkw::cpc_equal(), 0, 0, Fr::zero());
  }
};

struct OpenItem {
  zkp::EvalJob job;      // col: device pointer, Lagrange form; rot: rotation ids: 0,1,2,3, 4 = last (w^u), 5 = -1 (unused ones 0)
  U256 ev[4];            // canonical evaluations
};

// Admission gate of the GPU-heavy middle of a proof (grand products, their commitment, coset extension, quotient).  Proofs
// that start together move through the Fiat-Shamir rounds together: they all hash on the host at the same moments and all
// reach the light, serial end of the proof (evaluations, 758 Poseidon permutations, two one-column commitments) together, with
// the chip nearly idle.  Letting only a few proofs into the heavy part at a time -- first come, first served -- costs no
// throughput (that part is bound by the chip, a handful of proofs fill it) and spreads the proofs out: the serial end of one
// overlaps the heavy part of the next.  ZKFHE_GATE = proofs admitted at once (0 = no gate).
class HeavyGate {
 public:
  static HeavyGate &get() {
    static HeavyGate g;
    return g;
  }
  // returns whether a slot was taken (the gate may be switched while proofs are in flight: leave() only gives back what enter() took)
  bool enter() {
    std::unique_lock<std::mutex> l(mu);
    if (slots <= 0) return false;
    const uint64_t my = next_ticket++;
    cv.wait(l, [&] { return slots <= 0 || my < serving + (uint64_t)slots; });
    return true;
  }
  void leave() {
    {
      std::lock_guard<std::mutex> l(mu);
      ++serving;
    }
    cv.notify_all();
  }
  int set(int n) {
    int old;
    {
      std::lock_guard<std::mutex> l(mu);
      old = slots;
      if (n >= 0) slots = n;
    }
    cv.notify_all();
    return old;
  }

 private:
  HeavyGate() {
    if (const char *e = getenv("ZKFHE_GATE")) slots = atoi(e);
  }
  std::mutex mu;
  std::condition_variable cv;
  int slots = 0;
  uint64_t next_ticket = 0, serving = 0;   // tickets below `serving` have left; FIFO admission of serving .. serving + slots - 1
};
struct GateHold {
  bool held = false;
  void enter() { held = HeavyGate::get().enter(); }
  void leave() {
    if (held) HeavyGate::get().leave();
    held = false;
  }
  ~GateHold() { leave(); }
};

// ZKFHE_TRACE=1: host-side phase times of one proof on stderr
struct Trace {
  bool on;
  double t0, last, cpu_last;
  unsigned long tid;   // proofs in flight on other threads: their lines interleave
  static double thread_cpu_ms() {   // CPU time of the calling thread: what of a phase was work on this core and what was waiting
    timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
  }
  Trace() : on(getenv("ZKFHE_TRACE") != nullptr), t0(now_ms()), last(t0), cpu_last(on ? thread_cpu_ms() : 0), tid((unsigned long)std::hash<std::thread::id>()(std::this_thread::get_id()) % 10000) {}
  void mark(const char *what) {
    if (!on) return;
    const double t = now_ms(), c = thread_cpu_ms();
    fprintf(stderr, "[zkfhe trace %04lu] %8.3f ms (+%7.3f, cpu %6.3f) %s @%.3f\n", tid, t - t0, t - last, c - cpu_last, what, t);
    last = t;
    cpu_last = c;
  }
};

struct BackendGuard {
  GpuPolyMul gpu_mul;
  BackendGuard(zkfhe_ctx *ctx, Workspace *ws) : gpu_mul(ctx, ws) { poly_mul_backend() = &gpu_mul; }
  ~BackendGuard() { poly_mul_backend() = nullptr; }
};

// inverse of V[k1][m] = c_k1^m by Lagrange basis polynomials: column k1 of V^-1 holds the coefficients of
// L_k1(X) = prod_{j != k1} (X - c_j) / (c_k1 - c_j)
zkp::Mat3 vandermonde3_inverse(const Fr c[3]) {
  zkp::Mat3 vinv;
  for (int k1 = 0; k1 < 3; ++k1) {
    const Fr &a = c[(k1 + 1) % 3], &b = c[(k1 + 2) % 3];
    const Fr den = fr_inv((c[k1] - a) * (c[k1] - b));
    vinv.v[0 * 3 + k1] = a * b * den;              // X^0
    vinv.v[1 * 3 + k1] = (Fr::zero() - (a + b)) * den;  // X^1
    vinv.v[2 * 3 + k1] = den;                      // X^2
  }
  return vinv;
}

// interpolation through (pts[t], vals[t]), t < np <= 4: ascending coefficients, the unused ones zero
void interpolate4(const Fr *pts, const Fr *vals, size_t np, Fr rc[4]) {
  for (int q = 0; q < 4; ++q) rc[q] = Fr::zero();
  for (size_t i = 0; i < np; ++i) {
    Fr num[4] = {Fr::one(), Fr::zero(), Fr::zero(), Fr::zero()};   // prod_{t != i} (X - pts[t])
    Fr den = Fr::one();
    size_t deg = 0;
    for (size_t t = 0; t < np; ++t) {
      if (t == i) continue;
      for (size_t q = ++deg; q > 0; --q) num[q] = num[q - 1] - pts[t] * num[q];
      num[0] = Fr::zero() - pts[t] * num[0];
      den = den * (pts[i] - pts[t]);
    }
    const Fr scl = vals[i] * fr_inv(den);
    for (size_t q = 0; q <= deg; ++q) rc[q] = rc[q] + num[q] * scl;
  }
}

// a commitment batch [n_adv advice columns | la_0 .. | ls_0 ..] -> the advice points stay in pts, the points of the permuted
// lookup columns go to `permuted` in transcript order: la_0, ls_0, la_1, ls_1, ...
void split_permuted(std::vector<AffinePoint> &pts, size_t n_adv, std::vector<AffinePoint> &permuted) {
  const size_t nl = (pts.size() - n_adv) / 2;
  permuted.resize(2 * nl);
  for (size_t i = 0; i < nl; ++i) permuted[2 * i] = pts[n_adv + i], permuted[2 * i + 1] = pts[n_adv + nl + i];
  pts.resize(n_adv);
}

// One proof: the state that crosses a round of the protocol, one method per round (called in order by prove_impl).
struct Proof {
  zkfhe_ctx *const ctx;
  const zkfhe_srs *const srs;
  zkfhe_bfv_pk *const pk;
  const CircuitConfig &cfg;
  std::vector<U256> &instances;
  Trace &trace;
  Workspace *const ws;
  const NttDomain *const dom;
  const size_t n = cfg.n(), u = cfg.u(), nbl = n - u;   // rows, usable rows, blinding rows of an advice column
  const unsigned k = cfg.k;
  // The blinding stream (draw i = Blake2b(seed || i) mod r) is evaluated on the device, where each value is needed
  // (prover_kernels.hip.hpp k_rng_fill).  Draw order = oracle/halo2_ref.py: the blinding rows of every advice column in
  // column order, then per lookup its permuted input and permuted table, then the permutation and lookup products, then
  // the n coefficients of the random polynomial.
  zkp::RngSeed rseed;
  const uint64_t ctr_adv = 0, ctr_lk = (uint64_t)cfg.n_advice() * nbl, ctr_pz = ctr_lk + 2 * (uint64_t)cfg.n_lookup * nbl,
                 ctr_lz = ctr_pz + (uint64_t)cfg.n_chunks() * (nbl - 1), ctr_rand = ctr_lz + (uint64_t)cfg.n_lookup * (nbl - 1);
  Transcript tr{cfg.transcript};
  bool host_witness = false, early_p1 = false, early_rand = false, inst_via_ring = false;
  // one proof over several GPUs: rank r_sh of W_sh owns the permutation chunks [c_lo, c_hi) (see quotient()); one GPU owns them all
  const unsigned W_sh = srs->sharded() ? (unsigned)zkfhe_comm_world(srs->comm) : 1u, r_sh = srs->sharded() ? (unsigned)zkfhe_comm_rank(srs->comm) : 0u;
  const size_t c_lo = (size_t)cfg.n_chunks() * r_sh / W_sh, c_hi = (size_t)cfg.n_chunks() * (r_sh + 1) / W_sh;
  // the witness while it is built: phase 0 fills it, phase 1 completes it, the lookup round reads it
  BfvState st;
  Assigner as{cfg, false, ws->host_adv};   // host_adv is the workspace's pinned table (get_workspace): a null pointer here would mean a pageable table the kernels cannot read
  GpuPhase1 g1{ctx, pk, ws};
  std::vector<AffinePoint> permuted;   // commitments of the permuted lookup columns (split_permuted): the device paths commit them with the phase-1 advice
  U256 gamma_rlc;
  Fr beta, gamma, y, x;
  Fr *beta_delta_dev = nullptr;   // [n_perm] beta * delta^i
  Fr pts_rot[6];                  // x * w^rot by rotation id: 0,1,2,3 -> w^r ; 4 -> w^u ("last") ; 5 -> w^-1
  std::vector<OpenItem> items;    // the opened polynomials, in evaluation-write order (shplonk.hpp OpenLayout)
  size_t idx_H = 0;               // H(X) among them
  double t_wit = 0;               // when the phase-1 witness was queued: the end of the first of prove_impl's timings
  // the random polynomial, coefficients and Lagrange form: written on the auxiliary stream by setup() (one GPU), read from random_poly() on
  Fr *const rand_c = ws->rand_c(), *const rand_l = ws->rand_l();

  int rng_fill(hipStream_t stream, uint64_t ctr0, uint64_t ctr_col_stride, Fr *dst, size_t per_col, size_t col_stride, size_t n_cols) {
    if (!per_col || !n_cols) return ZKFHE_OK;
    zkp::k_rng_fill<<<grid_for(ctx, per_col * n_cols), 256, 0, stream>>>(rseed, ctr0, ctr_col_stride, dst, per_col, col_stride, n_cols);
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  }
  // the same draws by the kernel that writes the rest of the columns (zkp::RngRows): counters of column 0, counters per column
  zkp::RngRows blind_rows(uint64_t ctr0, uint64_t ctr_col_stride) const {
    return zkp::RngRows{rseed, ctr0, ctr_col_stride, 1};
  }
  const zkfhe_basis *small_basis() const { return srs->g_lagrange_small ? srs->g_lagrange_small : srs->g_lagrange; }
  bool owns_chunk(size_t j) const { return j >= c_lo && j < c_hi; }
  bool owns_col(size_t perm_col) const { return owns_chunk(perm_col / cfg.chunk()); }
  int setup() {
    // a previous proof on this context may have been abandoned on an error with copies from the pinned staging buffers still
    // queued: drain the stream before the buffers are rewritten (free when the stream is idle)
    CK(zkfhe_sync(ctx));
    CK(alloc_witness_buffers(ctx, pk, ws));
    ws->aux->cmd_owner = ctx;   // the auxiliary stream's commands are this proof's
    ws->aux->throughput = ctx->throughput;   // ... and run under its profile
    ws->ring_off = ws->ring_flushed = 0;
    ws->inst_pending = false;
    trace.mark("setup (workspace)");
    // random polynomial, early: its coefficients (the tail of the blinding stream) depend on no challenge, so they are drawn and
    // committed on the auxiliary stream beside the phase-0 / witness work.  The main stream is idle here (synchronised above)
    // and only touches this region again after waiting for ev_rand.  A sharded commitment is a collective: it stays on the
    // main stream, in protocol order.
    early_rand = !srs->sharded();
    if (!early_rand) return ZKFHE_OK;
    zkfhe_ctx *aux = ws->aux;
    CK(rng_fill(aux->stream, ctr_rand, 0, rand_c, n, n, 1));
    // the commitment is stored by the MSM's last kernel into pinned memory: no copy command
    if (int rc = zkfhe_msm_batch_xyzz(aux, srs->g, (const zkfhe_fr *)rand_c, 1, (zkfhe_g1_xyzz *)ws->host_rand_pt))
      return zk_fail_msg(ctx, rc, std::string("random polynomial commitment (auxiliary stream): ") + zkfhe_last_error(aux));
    // ... and its Lagrange form, which the evaluation round reads: one single-column transform less on the proof's critical path
    if (int rc = zkfhe_ntt_batch_to(aux, (const zkfhe_fr *)rand_c, (zkfhe_fr *)rand_l, 1, (int)k, 0))
      return zk_fail_msg(ctx, rc, std::string("random polynomial, Lagrange form (auxiliary stream): ") + zkfhe_last_error(aux));
    ZK_HIP(ctx, hipEventRecord(ws->ev_rand, aux->stream));
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ phase 0 witness
  // the phase-0 commitment (pts), with everything of phase 1 that does not wait for its challenge queued behind it
  int phase0(const char *input_json, const FastInput *words, std::vector<AffinePoint> &pts) {
    Context ctx0(CTX_PHASE0, false, false);
    std::vector<Cell> make_public;
    instances.clear();
    tr.common_scalar(pk->vk_digest);
    // the 5121 public inputs are hashed on a helper thread, started as soon as they are known: it runs beside the phase-0
    // precomputation, upload and commitment (a Poseidon sponge is one sequential chain of 2561 permutations here)
    // The first 2 N of them are pk0 | pk1 (examples/bfv.rs:118-119), the same for every encryption under one public key: the
    // transcript state behind them is kept per key (prefix_cache.hpp), and a proof that finds its key there starts from it --
    // 1 024 of the 2 561 permutations at k = 13.
    const auto on_public = [&](const std::vector<Cell> &pub) {
      instances.reserve(pub.size());
      for (const Cell &c : pub) instances.push_back(c.value);
      const size_t n_key = std::min<size_t>(instances.size(), 2 * (size_t)pk->prm.N);
      Transcript::State mid;
      if (input_json && pk->prehash.take(input_json, strlen(input_json), instances.data(), instances.size(), mid)) {
        tr.restore(mid);   // announced ahead of time (zkfhe_bfv_pk_prehash): `vk digest | public inputs` are absorbed already
      } else if (!n_key || !pk->prefix.capacity()) {
        tr.common_scalars_async(instances);
      } else if (pk->prefix.lookup(instances.data(), n_key, mid)) {
        tr.restore(mid);
        tr.common_scalars_async(std::vector<U256>(instances.begin() + (long)n_key, instances.end()));
      } else {
        PrefixCache *cache = &pk->prefix;
        std::vector<U256> key(instances.begin(), instances.begin() + (long)n_key);
        tr.common_scalars_async_marked(instances, n_key, [cache, key](const Transcript::State &st) { cache->insert(key.data(), key.size(), st); });
      }
    };
    // machine-word phase 0 (bfv_phase0_fast.hpp) for every input in its domain; anything else goes through the line-by-line
    // restatement of the reference, which also words the errors
    // words the values stage declines are rendered as the JSON that spells them and take the text path: the same outcome as
    // zkfhe_bfv_prove on that text by construction (the announcements of zkfhe_bfv_pk_prehash are keyed on text and serve text only)
    std::string rendered;
    if (words ? !bfv_phase0_fast_values(ctx0, *words, pk->prm, make_public, st, on_public)
              : !bfv_phase0_fast(ctx0, input_json, strlen(input_json), pk->prm, make_public, st, on_public)) {
      if (words) {
        rendered = render_input_json(*words);
        input_json = rendered.c_str();
      }
      const CircuitInput in = CircuitInput::parse_json(input_json);
      trace.mark("parse_json");
      st = bfv_phase0(ctx0, in, pk->prm, make_public, on_public);
    }
    trace.mark("bfv_phase0");
    as.place(ctx0, true);
    trace.mark("place phase 0");
    // the instance column's values ride up with the proof's first table flush (they are needed from the grand products on)
    if (instances.size() > n) return zk_fail_msg(ctx, ZKFHE_EINVAL, "more public inputs than rows");
    inst_via_ring = instances.size() * 32 <= ((size_t)1 << 20);   // long instance columns (k >= 18) keep their own copy
    if (inst_via_ring) {
      STAGE(staged, U256, ws, instances.data(), instances.size() * 32);
      // ... and the flush kernel that carries them converts them into the instance column on its way (the column is idle until the
      // grand products, and the previous proof on this workspace is complete)
      ws->inst_src = (const Fr *)(ws->ring + ((const uint8_t *)staged - (const uint8_t *)ws->dev_ring.p));
      ws->inst_n = instances.size();
      ws->inst_pending = true;
    }
    trace.mark("transcript: instances");
    CK(blind_and_upload(0, cfg.n_gate0));
    trace.mark("blind + upload phase 0");
    const char *witness_env = getenv("ZKFHE_WITNESS");
    host_witness = witness_env && strcmp(witness_env, "host") == 0;
    // see "Early phase-1 commitment" below.  On with the Poseidon transcript, whose challenge after the phase-0 commitment is
    // 2561 sequential permutations (the public inputs, ~20 ms of host time) away: measured on a wave of 20 concurrent proofs
    // +9 % (the GPU commits while every proof hashes), -1.5 % in steady state (two extra small commitments per proof).  With
    // Blake2b there is no hash to hide -- but on long rows (k >= 18) the RLC witness the host computes from that challenge is
    // (k = 19: 6 ms of Horner chains and placement with the GPU idle): 155.8 -> 151.5 ms per proof; at k = 16 it costs 0.7 ms.
    // ZKFHE_EARLY_P1=0 / 1 overrides.
    const char *early_env = getenv("ZKFHE_EARLY_P1");
    // Under the throughput profile (ctx.hpp) the hash is hidden behind other proofs' GPU work already: off wherever the Poseidon hash
    // is the only reason (59 launches per proof instead of 64).  The k >= 18 rule hides host RLC work and stays.  Measured with 16
    // streams, gate 4 and 768 timed proofs, four runs each (profiles/throughput_profile.md): off 285.7 against on 284.5 proofs/s
    // (+0.4 %) with the profile's chunks of 256 points in the few-column table sums -- but 279.2 against 281.9 (-1.0 %) with chunks of
    // 128: the two extra commitments are few-column table sums themselves.  The "-1.5 % in steady state" above is from before both.
    const bool early_want = early_env ? early_env[0] == '1' : ((cfg.transcript == TR_POSEIDON && !ctx->throughput) || k >= 18);
    early_p1 = early_want && !host_witness && cfg.n_lookup > 0 && cfg.lookup_bits == 8;
    if (host_witness) return commit_cols(ctx, srs, small_basis(), ws->adv_l.fr(), cfg.n_gate0, (G1Affine *)ws->points.p, pts);
    // the commitment's points come back through an event; the phase-1 gadget launches queue up behind the MSM
    CK(srs_msm_pts(ctx, srs, small_basis(), ws->adv_l.fr(), cfg.n_gate0, ws->host_pts));   // stored into pinned memory by the MSM itself
    CK(srs_record(ctx, srs, ws->ev_pts));   // sharded: behind the all-gather on the communicator's stream, which the gadget launches below overlap
    CK(g1.launch(st));
    if (early_p1) {
      // Early phase-1 commitment.  Of the phase-1 columns only the RLC columns and the 16 constrain_mul gate cells depend on
      // the challenge the transcript yields after the phase-0 commitment -- and with the Poseidon transcript that challenge
      // is 2561 sequential permutations away (the public inputs).  So the gate and lookup columns are placed, blinded,
      // permuted and committed NOW, with those cells zero and the RLC columns zero; afterwards the missing cells are
      // committed as sparse correction columns and added (a commitment is linear in its column).  Same points, same bytes.
      // the placement kernels draw the blinding rows of their columns and clear the RLC columns behind them
      CK(g1.place_early(blind_rows(ctr_adv + (uint64_t)cfg.n_gate0 * nbl, nbl), cfg.n_rlc));
      CK(permute_lookups(ws->host_early_err));   // pinned: written by the kernel, read by the host after ev_early
      CK(srs_msm_pts(ctx, srs, small_basis(), ws->adv_l.fr() + (size_t)cfg.n_gate0 * n, cfg.n_advice() - cfg.n_gate0 + 2 * cfg.n_lookup, ws->host_early));
      CK(srs_record(ctx, srs, ws->ev_early));
    }
    ZK_HIP(ctx, hipEventSynchronize(ws->ev_pts));
    pts.resize(cfg.n_gate0);
    points_canon(srs, ws->host_pts, cfg.n_gate0, pts.data());
    return ZKFHE_OK;
  }
  // advice columns [col_lo, col_hi) of the host table -> device, Montgomery form, with their blinding rows
  int blind_and_upload(unsigned col_lo, unsigned col_hi) {
    // the table is pinned and column-contiguous; the blinding rows u .. n-1 are drawn on the device.  The conversion kernel reads the
    // pinned table itself (hipHostMalloc memory is mapped into the device's address space): no copy command on the stream -- with twenty
    // proofs starting together the runtime's copy path cost each of them 2-5 ms of CPU before their first kernel (ZKFHE_UPLOAD=copy: one
    // DMA for the whole phase, then the conversion in place)
    const char *upload_env = getenv("ZKFHE_UPLOAD");   // read per proof, like ZKFHE_WITNESS / ZKFHE_EARLY_P1 (the tests switch it)
    const bool upload_by_copy = upload_env && !strcmp(upload_env, "copy");
    Fr *dst = ws->adv_l.fr() + (size_t)col_lo * n;
    if (!upload_by_copy) {
      zkp::k_to_mont_blind<<<grid_for(ctx, (size_t)(col_hi - col_lo) * n), 256, 0, ctx->stream>>>((const Fr *)as.t.advice[col_lo], dst, n, (unsigned)u, col_hi - col_lo,
                                                                                                   blind_rows(ctr_adv + (uint64_t)col_lo * nbl, nbl));
      ZK_LAUNCH_CHECK(ctx);
      return ZKFHE_OK;
    }
    ZK_HIP(ctx, zk_memcpy_async(ctx, dst, as.t.advice[col_lo], (size_t)(col_hi - col_lo) * n * 32, hipMemcpyHostToDevice, ctx->stream));
    CK(zkfhe_fr_to_mont(ctx, (const zkfhe_fr *)dst, (zkfhe_fr *)dst, (size_t)(col_hi - col_lo) * n));
    return rng_fill(ctx->stream, ctr_adv + (uint64_t)col_lo * nbl, nbl, dst + u, nbl, n, col_hi - col_lo);
  }
  // The device lookup permutation of every lookup column into la | ls, which also draws their blinding rows (la_i then ls_i, lookup by
  // lookup -- two interleaved runs of the stream).  err is pinned: raised by the kernel, read by the caller once the host has waited.
  int permute_lookups(int *err) {
    *err = 0;
    const zkp::RngRows blind_lk = blind_rows(ctr_lk, 2 * nbl);
    return zkw::lookup_permute(ctx, ws->adv_l.fr() + (size_t)cfg.adv_lookup0() * n, n, (unsigned)u, cfg.n_lookup, ws->la_l.fr(), ws->ls_l.fr(), err, nullptr, &blind_lk);
  }
  // ------------------------------------------------------------ phase 1 witness
  // The three ways to the phase-1 advice commitment (pts): host, device, and device with the early commitment; each records t_wit once its witness is queued.
  // ZKFHE_WITNESS=host: the whole witness on the host (the tests' reference for the device generator)
  int phase1_host(std::vector<AffinePoint> &pts) {
    Context ctx_gate(CTX_GATE1, false, false), ctx_rlc(CTX_RLC1, true, false);
    bfv_phase1(st, pk->prm, ctx_gate, ctx_rlc, gamma_rlc);
    as.place(ctx_gate, true);
    as.place(ctx_rlc, true);
    as.place_lookups(ctx_gate);
    t_wit = now_ms();
    CK(blind_and_upload(cfg.n_gate0, cfg.n_advice()));
    trace.mark("blind + upload phase 1");
    return commit_cols_out(ctx, srs, small_basis(), ws->adv_l.fr() + (size_t)cfg.n_gate0 * n, cfg.n_advice() - cfg.n_gate0, ws, pts);
  }
  int phase1_device(std::vector<AffinePoint> &pts) {
    const size_t n_adv1 = cfg.n_advice() - cfg.n_gate0;
    // RLC context on the host (6 K cells), gate context (1.2 M cells) on the device
    Context ctx_rlc(CTX_RLC1, true, false);
    U256 evals[12];
    bfv_phase1_rlc(st, ctx_rlc, gamma_rlc, evals);
    trace.mark("rlc context");
    as.place(ctx_rlc, true);
    trace.mark("place rlc");
    if (early_p1) return phase1_early_finish(evals, n_adv1, pts);
    CK(g1.finish(evals, blind_rows(ctr_adv + (uint64_t)cfg.n_gate0 * nbl, nbl)));   // blinding rows of the device-generated columns: same draw order as the host path
    trace.mark("gpu phase 1 (enqueue)");
    t_wit = now_ms();
    CK(blind_and_upload(cfg.adv_rlc0(), cfg.n_advice()));
    trace.mark("blind + upload phase 1");
    if (!cfg.n_lookup) return commit_cols_out(ctx, srs, small_basis(), ws->adv_l.fr() + (size_t)cfg.n_gate0 * n, n_adv1, ws, pts);
    // Single-expression lookups do not use theta, so the permuted columns can be built before the advice commitment is
    // hashed: one MSM call over [phase-1 advice | la | ls] (contiguous in all_l) instead of two, same points, same
    // transcript order, same draw order of the blinding values.
    if (cfg.lookup_bits != 8) return zk_fail_msg(ctx, ZKFHE_EINVAL, "the device lookup permutation is built for lookup_bits = 8");
    int *lookup_err = ws->out_flags() + 2;   // pinned
    CK(permute_lookups(lookup_err));
    CK(commit_cols_out(ctx, srs, small_basis(), ws->adv_l.fr() + (size_t)cfg.n_gate0 * n, n_adv1 + 2 * cfg.n_lookup, ws, pts));
    if (*lookup_err) return zk_fail_msg(ctx, ZKFHE_EINVAL, "lookup input not in table: a range check of the witness fails");
    split_permuted(pts, n_adv1, permuted);
    return ZKFHE_OK;
  }
  // the challenge-dependent rest of the early phase-1 commitment: the reserved gate cells (into the columns and into sparse
  // correction columns), the RLC columns; two small commitments, then early + correction on the host
  int phase1_early_finish(const U256 evals[12], size_t n_adv1, std::vector<AffinePoint> &pts) {
    const GpuPhase1::PatchPlan plan = g1.patch_plan();
    const size_t np = plan.columns.size();
    Fr *patch_cols = ws->patch_cols();
    std::vector<zkfhe_sparse_term> terms;
    const bool sparse = !srs->sharded() && zkfhe_basis_has_multiples(srs->g_lagrange);
    CK(g1.patch(evals, plan, patch_cols, sparse ? &terms : nullptr));
    CK(blind_and_upload(cfg.adv_rlc0(), cfg.n_advice()));
    // the correction points go into the pinned result block: [patched gate columns | RLC columns]
    if (np + cfg.n_rlc > ws->out_pts_cap)
      return zk_fail_msg(ctx, ZKFHE_EINVAL, "early phase-1 commitment: correction points do not fit the workspace (set ZKFHE_EARLY_P1=0)");
    uint8_t *fix_dev = ws->out_pts();   // pinned: the correction points are read by the host right below
    const size_t ps = pt_stride(srs);
    if (np && sparse) {
      // a dozen non-zero cells: one wave per correction column over the digit-multiple table
      STAGE(terms_dev, zkfhe_sparse_term, ws, terms.data(), terms.size() * sizeof(zkfhe_sparse_term));
      CK(flush_staged(ctx, ws));
      CK(zkfhe_msm_sparse_xyzz(ctx, srs->g_lagrange, terms_dev, terms.size(), np, (zkfhe_g1_xyzz *)fix_dev));   // sparse => one GPU => accumulator-form slots
    } else if (np) {
      CK(srs_msm_pts(ctx, srs, srs->g_lagrange, patch_cols, np, fix_dev));
    }
    if (cfg.n_rlc) CK(srs_msm_pts(ctx, srs, srs->g_lagrange, ws->adv_l.fr() + (size_t)cfg.adv_rlc0() * n, cfg.n_rlc, fix_dev + np * ps));
    CK(srs_join(ctx, srs, false));
    ZK_HIP(ctx, zk_wait(ctx));   // everything queued so far, the early commitment (ev_early) included
    if (*ws->host_early_err) return zk_fail_msg(ctx, ZKFHE_EINVAL, "lookup input not in table: a range check of the witness fails");
    // early commitment + correction, on the host (at most a handful of additions), in the form the slots hold; the sums are
    // normalised with the rest of the round below
    for (size_t t = 0; t < np; ++t) {
      if (srs->sharded()) {
        G1Affine &e = ((G1Affine *)ws->host_early)[plan.columns[t]];
        zk::G1X acc = zk::g1x_from_affine(e);
        zk::g1x_add_affine(acc, ((const G1Affine *)fix_dev)[t], false);
        e = zk::g1x_to_affine(acc);
      } else {
        zk::g1x_add(((zk::G1X *)ws->host_early)[plan.columns[t]], ((const zk::G1X *)fix_dev)[t]);
      }
    }
    for (unsigned j = 0; j < cfg.n_rlc; ++j) memcpy(ws->host_early + (size_t)(cfg.adv_rlc0() - cfg.n_gate0 + j) * ps, fix_dev + (np + j) * ps, ps);
    trace.mark("gpu phase 1 (enqueue)");
    t_wit = now_ms();
    trace.mark("blind + upload phase 1");
    pts.resize(n_adv1 + 2 * (size_t)cfg.n_lookup);
    points_canon(srs, ws->host_early, pts.size(), pts.data());   // one inversion for the round: advice | permuted inputs | permuted tables
    split_permuted(pts, n_adv1, permuted);
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ lookups: permuted input / table
  int lookup_columns() {
    if (!cfg.n_lookup) return ZKFHE_OK;
    if (host_witness) {   // the device paths committed la | ls with the phase-1 advice
      std::vector<U256> input, ap, sp;
      U256 *stA = ws->host_blind, *stS = ws->host_blind + (size_t)cfg.n_lookup * n;  // la | ls, as on the device
      for (unsigned i = 0; i < cfg.n_lookup; ++i) {
        input.assign(as.t.advice[cfg.adv_lookup0() + i], as.t.advice[cfg.adv_lookup0() + i] + u);
        permute_lookup(input, u, 1u << cfg.lookup_bits, ap, sp);
        U256 *colA = stA + (size_t)i * n, *colS = stS + (size_t)i * n;
        std::copy(ap.begin(), ap.end(), colA);
        std::copy(sp.begin(), sp.end(), colS);
        for (size_t r = u; r < n; ++r) colA[r] = colS[r] = fe::zero();
      }
      ZK_HIP(ctx, zk_memcpy_async(ctx, ws->la_l.p, ws->host_blind, 2 * (size_t)cfg.n_lookup * n * 32, hipMemcpyHostToDevice, ctx->stream));
      CK(zkfhe_fr_to_mont(ctx, (const zkfhe_fr *)ws->la_l.p, (zkfhe_fr *)ws->la_l.p, 2 * (size_t)cfg.n_lookup * n));
      CK(rng_fill(ctx->stream, ctr_lk, 2 * nbl, ws->la_l.fr() + u, nbl, n, cfg.n_lookup));
      CK(rng_fill(ctx->stream, ctr_lk + nbl, 2 * nbl, ws->ls_l.fr() + u, nbl, n, cfg.n_lookup));
      std::vector<AffinePoint> pts;
      CK(commit_cols_out(ctx, srs, small_basis(), ws->la_l.fr(), 2 * cfg.n_lookup, ws, pts));  // la | ls contiguous
      split_permuted(pts, 0, permuted);
    }
    tr.write_points(permuted);
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ permutation and lookup grand products
  zkp::PermArgs perm_args() const {
    zkp::PermArgs pa;
    pa.adv = ws->adv_l.fr();
    pa.constcol = pk->fixed_l.fr() + (size_t)cfg.fix_const() * n;
    pa.inst = ws->inst_l.fr();
    pa.sigma = pk->sigma_l.fr();
    pa.wpow = dom->fwd;
    pa.beta_delta = beta_delta_dev;
    pa.beta = beta;
    pa.gamma = gamma;
    pa.n_advice = cfg.n_advice();
    pa.n_perm = cfg.n_perm();
    pa.chunk = cfg.chunk();
    pa.n_chunks = cfg.n_chunks();
    pa.n = n;
    return pa;
  }
  // running products per column; long columns in segments (prover_kernels.hip.hpp), the segment products in `den`, whose factors the inversion consumed
  // blind: the blinding rows u + 1 .. n - 1 of the product columns (drawn per column, in order)
  int prefix_products(const Fr *ratio, Fr *z, size_t n_cols, const zkp::RngRows &blind, Fr *totals_dev) {
    const size_t nb_z = nbl - 1;
    if (n <= 65536) {   // measured at k = 16 (two segments): no gain over one workgroup per column; k = 19: 6.5 -> 1 ms per proof
      zkp::k_prefix_product<<<(unsigned)n_cols + zkp::rng_tail_grid(blind, n_cols * nb_z, 1024), 1024, 0, ctx->stream>>>(ratio, z, totals_dev, n, (unsigned)u, (unsigned)n_cols, blind);
      ZK_LAUNCH_CHECK(ctx);
      return ZKFHE_OK;
    }
    CK(rng_fill(ctx->stream, blind.ctr0, blind.ctr_col_stride, z + (u + 1), nb_z, n, n_cols));   // long columns: the blinding rows keep their own launch
    const unsigned seg_len = 32768, segs = (unsigned)(n / seg_len);   // u < n: the output row z[u] lies inside the last segment
    Fr *seg = ws->prefix_segments();
    if ((size_t)n_cols * segs * 32 > ws->cap(wsl::PREFIX_SEGMENTS)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "prefix products: segment buffer too small");
    zkp::k_prefix_seg_totals<<<dim3(segs, (unsigned)n_cols), 1024, 0, ctx->stream>>>(ratio, seg, n, (unsigned)u, seg_len);
    ZK_LAUNCH_CHECK(ctx);
    zkp::k_prefix_seg_scan<<<(unsigned)((n_cols + 63) / 64), 64, 0, ctx->stream>>>(seg, segs, (unsigned)n_cols, totals_dev);
    ZK_LAUNCH_CHECK(ctx);
    zkp::k_prefix_seg_apply<<<dim3(segs, (unsigned)n_cols), 1024, 0, ctx->stream>>>(ratio, seg, z, n, (unsigned)u, seg_len);
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  }
  int grand_products() {
    if (inst_via_ring) {
      CK(flush_staged(ctx, ws));   // nothing to launch when an earlier round's flush took the values along and stored the column
    } else {
      if (instances.size() < ws->inst_count)
        ZK_HIP(ctx, zk_memset_async(ctx, ws->inst_l.fr() + instances.size(), 0, (ws->inst_count - instances.size()) * 32, ctx->stream));
      CK(upload_canon(ctx, ws->inst_l.fr(), instances.data(), instances.size()));
      ws->inst_count = instances.size();
    }
    U256 dcan;
    memcpy(dcan.l, DELTA_CANON, 32);
    beta_delta_dev = ws->beta_delta();
    const size_t nch = cfg.n_chunks(), nb_z = nbl - 1;
    if (n <= 65536 && !ctx->chain_serial) return grand_products_side_by_side(mont(dcan));
    zkp::k_powers<<<1, 256, 0, ctx->stream>>>(beta, mont(dcan), beta_delta_dev, cfg.n_perm());
    ZK_LAUNCH_CHECK(ctx);
    zkp::k_perm_num_den<<<grid_for(ctx, nch * n), 256, 0, ctx->stream>>>(perm_args(), ws->num.fr(), ws->den.fr());
    ZK_LAUNCH_CHECK(ctx);
    CK(zkfhe_fr_batch_invert_mul(ctx, (const zkfhe_fr *)ws->den.p, (zkfhe_fr *)ws->num.p, nch * n));   // num <- num / den: the ratios, in one kernel
    Fr *totals_dev = ws->chunk_totals();
    CK(prefix_products(ws->num.fr(), ws->pz_l.fr(), nch, blind_rows(ctr_pz, nb_z), totals_dev));
    int *const closes = ws->out_flags();   // pinned: [0] permutation, [1] lookups -- read after the commitment of the products below
    closes[0] = closes[1] = 1;
    // chunk j starts where chunk j - 1 ended: the carries are the running product of the chunk totals, formed on the device
    zkp::k_chunk_carry<<<1, 1024, 0, ctx->stream>>>(totals_dev, (unsigned)nch, 0, closes);
    ZK_LAUNCH_CHECK(ctx);
    zkp::k_scale_rows<<<grid_for(ctx, nch * (u + 1)), 256, 0, ctx->stream>>>(ws->pz_l.fr(), totals_dev, n, (unsigned)(u + 1), (unsigned)nch);
    ZK_LAUNCH_CHECK(ctx);
    // ---------------------------------------------------------- lookup grand products
    if (cfg.n_lookup) {
      const size_t nl = cfg.n_lookup;
      zkp::k_lookup_num_den<<<grid_for(ctx, nl * n), 256, 0, ctx->stream>>>(ws->adv_l.fr() + (size_t)cfg.adv_lookup0() * n,
                                                                            pk->fixed_l.fr() + (size_t)cfg.fix_table() * n, ws->la_l.fr(), ws->ls_l.fr(),
                                                                            beta, gamma, (unsigned)nl, n, ws->num.fr(), ws->den.fr());
      ZK_LAUNCH_CHECK(ctx);
      CK(zkfhe_fr_batch_invert_mul(ctx, (const zkfhe_fr *)ws->den.p, (zkfhe_fr *)ws->num.p, nl * n));
      CK(prefix_products(ws->num.fr(), ws->lz_l.fr(), nl, blind_rows(ctr_lz, nb_z), totals_dev));
      zkp::k_chunk_carry<<<1, 1024, 0, ctx->stream>>>(totals_dev, (unsigned)nl, 1, closes + 1);
      ZK_LAUNCH_CHECK(ctx);
    }
    return commit_products();
  }
  // Short rows (every launch here is thin): the lookup products do not read what the permutation products write, so the two run as
  // columns of the same launches -- six launches instead of ten.  The lookup columns lie behind the permutation's in num / den, in the
  // product columns (pz | lz) and in the totals, and their blinding counters follow the permutation's (ctr_lz = ctr_pz + n_chunks *
  // (nbl - 1)): every buffer and every draw is the one of the sequence above.
  int grand_products_side_by_side(const Fr &delta) {
    const size_t nch = cfg.n_chunks(), nl = cfg.n_lookup, nb_z = nbl - 1;
    if ((nch + nl) * n * 32 > ws->num.bytes || (nch + nl) * n * 32 > ws->den.bytes) return zk_fail_msg(ctx, ZKFHE_EINVAL, "grand products: ratio buffers too small");
    Fr *const num_lk = ws->num.fr() + nch * n, *const den_lk = ws->den.fr() + nch * n;
    zkp::k_lookup_num_den_powers<<<(nl ? grid_for(ctx, nl * n) : 0u) + 1u, 256, 0, ctx->stream>>>(
        ws->adv_l.fr() + (size_t)cfg.adv_lookup0() * n, pk->fixed_l.fr() + (size_t)cfg.fix_table() * n, ws->la_l.fr(), ws->ls_l.fr(), beta, gamma, (unsigned)nl, n, num_lk, den_lk,
        beta, delta, beta_delta_dev, cfg.n_perm());
    ZK_LAUNCH_CHECK(ctx);
    zkp::k_perm_num_den<<<grid_for(ctx, nch * n), 256, 0, ctx->stream>>>(perm_args(), ws->num.fr(), ws->den.fr());
    ZK_LAUNCH_CHECK(ctx);
    CK(zk_fr_batch_invert_mul_joined(ctx, ws->den.fr(), ws->num.fr(), (nch + nl) * n));   // every ratio of both arguments
    Fr *totals_dev = ws->chunk_totals();   // [n_chunks | n_lookup]
    CK(prefix_products(ws->num.fr(), ws->pz_l.fr(), nch + nl, blind_rows(ctr_pz, nb_z), totals_dev));   // pz | lz contiguous
    int *const closes = ws->out_flags();
    closes[0] = closes[1] = 1;
    zkp::k_chunk_carry_both<<<nl ? 2 : 1, 1024, 0, ctx->stream>>>(totals_dev, (unsigned)nch, (unsigned)nl, closes);
    ZK_LAUNCH_CHECK(ctx);
    zkp::k_scale_rows<<<grid_for(ctx, nch * (u + 1)), 256, 0, ctx->stream>>>(ws->pz_l.fr(), totals_dev, n, (unsigned)(u + 1), (unsigned)nch);
    ZK_LAUNCH_CHECK(ctx);
    return commit_products();
  }
  int commit_products() {
    const size_t nch = cfg.n_chunks();
    int *const closes = ws->out_flags();
    std::vector<AffinePoint> pz_commit;
    CK(commit_cols_out(ctx, srs, srs->g_lagrange, ws->pz_l.fr(), nch + cfg.n_lookup, ws, pz_commit));  // pz | lz contiguous
    if (!closes[0]) return zk_fail_msg(ctx, ZKFHE_EINVAL, "permutation argument does not close: a copy constraint is violated");
    if (!closes[1]) return zk_fail_msg(ctx, ZKFHE_EINVAL, "lookup argument does not close");
    tr.write_points(pz_commit);   // permutation products, then lookup products
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ vanishing: random polynomial (coefficient form)
  int random_poly() {
    // committed at the start of the proof on the auxiliary stream ("random polynomial, early"): the last n draws of the stream
    if (early_rand) {
      ZK_HIP(ctx, hipEventSynchronize(ws->ev_rand));
      ZK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ws->ev_rand, 0));   // later reads of rand_c on the main stream
      AffinePoint rp;
      points_canon(srs, ws->host_rand_pt, 1, &rp);
      tr.write_point(rp);
    } else {
      CK(rng_fill(ctx->stream, ctr_rand, 0, rand_c, n, n, 1));
      std::vector<AffinePoint> rand_commit;
      CK(commit_cols_out(ctx, srs, srs->g, rand_c, 1, ws, rand_commit));
      tr.write_point(rand_commit[0]);
    }
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ quotient
  // once the gathers are queued: dst[j] = the sum of the W_sh shares of slot j of ws->qgather ([slot][rank][n]), j < slots
  int sum_shares(size_t slots, Fr *dst) {
    CK(zkfhe_comm_join(ctx, srs->comm, 0));
    for (size_t j = 0; j < slots; ++j) {
      zkp::k_sum_rows<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(ws->qgather.fr() + j * (size_t)W_sh * n, W_sh, n, dst + j * n);
      ZK_LAUNCH_CHECK(ctx);
    }
    return ZKFHE_OK;
  }
  zkp::QArgs quotient_args(const zkp::QGroup *groups_dev, int q_rows) const {
    zkp::QArgs qa;
    qa.adv = ws->adv_ext.fr();
    qa.fix = pk->fixed_ext.fr();
    qa.sig = pk->sigma_ext.fr();
    qa.pz = ws->pz_ext.fr();
    qa.lz = ws->lz_ext.fr();
    qa.la = ws->la_ext.fr();
    qa.ls = ws->ls_ext.fr();
    qa.inst = ws->inst_ext.fr();
    qa.lext = pk->l_ext.fr();
    qa.xs = pk->xs_ext.fr();
    qa.beta_delta = beta_delta_dev;
    qa.groups = groups_dev;
    qa.partials = ws->quotient_partials();
    qa.y = y;
    qa.beta = beta;
    qa.gamma = gamma;
    qa.gamma_rlc = mont(gamma_rlc);
    qa.log_n = k;
    qa.u = (unsigned)u;
    qa.n_gate = cfg.n_gate();
    qa.n_rlc = cfg.n_rlc;
    qa.adv_rlc0 = cfg.adv_rlc0();
    qa.fix_qrlc0 = cfg.fix_qrlc0();
    qa.fix_const = cfg.fix_const();
    qa.fix_table = cfg.fix_table();
    qa.adv_lookup0 = cfg.adv_lookup0();
    qa.n_lookup = cfg.n_lookup;
    qa.n_advice = cfg.n_advice();
    qa.n_perm = cfg.n_perm();
    qa.chunk = cfg.chunk();
    qa.n_chunks = cfg.n_chunks();
    qa.rows = (unsigned)q_rows;
    return qa;
  }
  // the G expression groups at the points [pt0, pt0 + count) of the extended domain, folded with the powers of y into h_ext
  int launch_quotient(zkp::QArgs &qa, size_t pt0, size_t count, size_t G, const Fr *ypow_dev, const Fr *zinv_dev) {
    qa.pt0 = pt0;
    qa.pt_count = count;
    const unsigned blocks = (unsigned)((count + 255) / 256);
    if (G) {   // a rank of a sharded proof may own no group
      zkp::k_quotient_partials<<<dim3(blocks, (unsigned)G), 256, 0, ctx->stream>>>(qa);
      ZK_LAUNCH_CHECK(ctx);
    }
    zkp::k_quotient_combine<<<blocks, 256, 0, ctx->stream>>>(ws->quotient_partials(), ypow_dev, (unsigned)G, zinv_dev, k, qa.rows, pt0, count, ws->h_ext.fr());
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  }
  // The quotient has degree < 3n, so three cosets determine it (one quarter less extension and evaluation work).  The
  // fourth coset is only needed for the degree check below (a violated gate shows up as a non-zero top quarter):
  // a key built with ZKFHE_CHECK_QUOTIENT=1 in the environment keeps it (pk->ext_rows).
  // (Extending the challenge-independent columns -- 264 of 402 -- right after the early commitment, on the main or on the
  // auxiliary stream, was measured and dropped: 165-172 proofs/s on a wave of 20 against 172-177 without, 185-192 in steady
  // state against 192-203; the smaller NTT batches and the extra launches cost more than the idle time they fill.)
  // One proof over several GPUs (srs->sharded()): besides the commitments (point ranges, comm.hip) the extension to the coset
  // domain and the quotient are sharded BY COLUMN.  Rank r owns the permutation chunks [nch r / W, nch (r+1) / W), hence the
  // advice columns of those chunks, their gates / RLC gates / lookups and the chunks' permutation terms; it extends only those
  // columns (plus the grand product of the chunk before its first one, which the chaining term reads), evaluates only the
  // expression groups that belong to them, and the W partial quotients (rows * n values each) are all-gathered and summed on
  // every rank.  With W = 1 everything is owned: the same code.
  int quotient(std::vector<AffinePoint> &h_commit) {
    const int q_rows = pk->ext_rows;
    const Fr wext = zk_fr_root_of_unity((int)k + 2);
    if (W_sh == 1) {
      CK(extend_cols(ctx, pk, ws, ws->all_l.fr(), ws->n_all, ws->all_ext.fr()));
    } else {
      const size_t ecol = n * (size_t)q_rows;
      auto ext_range = [&](const View &l, const View &e, size_t lo, size_t hi) -> int {
        if (hi <= lo) return ZKFHE_OK;
        return extend_cols(ctx, pk, ws, l.fr() + lo * n, hi - lo, e.fr() + lo * ecol);
      };
      const size_t a_lo = std::min<size_t>(c_lo * cfg.chunk(), cfg.n_advice()), a_hi = std::min<size_t>(c_hi * cfg.chunk(), cfg.n_advice());
      CK(ext_range(ws->adv_l, ws->adv_ext, a_lo, a_hi));
      const size_t l_lo = a_lo > cfg.adv_lookup0() ? std::min<size_t>(a_lo - cfg.adv_lookup0(), cfg.n_lookup) : 0;
      const size_t l_hi = a_hi > cfg.adv_lookup0() ? std::min<size_t>(a_hi - cfg.adv_lookup0(), cfg.n_lookup) : 0;
      CK(ext_range(ws->la_l, ws->la_ext, l_lo, l_hi));
      CK(ext_range(ws->ls_l, ws->ls_ext, l_lo, l_hi));
      CK(ext_range(ws->lz_l, ws->lz_ext, l_lo, l_hi));
      CK(ext_range(ws->pz_l, ws->pz_ext, c_lo ? c_lo - 1 : 0, c_hi));
      if (owns_col(cfg.perm_inst())) CK(ext_range(ws->inst_l, ws->inst_ext, 0, 1));
    }
    // expression groups, in the folding order of oracle/halo2_ref.py expressions_at: the expressions are numbered globally (the
    // power of y of a group is fixed by the number of its last expression); a group is a run of owned, consecutive units of one
    // kind, cut at the kernel's group sizes
    const size_t nch = cfg.n_chunks();
    std::vector<zkp::QGroup> groups;
    std::vector<size_t> last_e;  // global index of the last expression of each group
    size_t e = 0;
    auto run = [&](int type, size_t first, size_t count, size_t max_group, size_t expr_per_unit, const std::function<bool(size_t)> &owned) {
      size_t j = first;
      while (j < first + count) {
        if (!owned(j)) {
          e += expr_per_unit;
          ++j;
          continue;
        }
        size_t len = 0;
        while (j + len < first + count && len < max_group && owned(j + len)) ++len;
        groups.push_back(zkp::QGroup{type, (int)j, (int)len, 0});
        e += len * expr_per_unit;
        last_e.push_back(e - 1);
        j += len;
      }
    };
    run(zkp::QG_GATE, 0, cfg.n_gate(), 8, 1, [&](size_t j) { return owns_col(j); });
    run(zkp::QG_RLC, 0, cfg.n_rlc, cfg.n_rlc ? cfg.n_rlc : 1, 1, [&](size_t j) { return owns_col(cfg.adv_rlc0() + j); });
    run(zkp::QG_PERM_FIRST, 0, 1, 1, 1, [&](size_t) { return owns_chunk(0); });
    run(zkp::QG_PERM_LAST, 0, 1, 1, 1, [&](size_t) { return owns_chunk(nch - 1); });
    run(zkp::QG_PERM_C, 1, nch - 1, 32, 1, [&](size_t j) { return owns_chunk(j); });
    run(zkp::QG_PERM_D, 0, nch, 4, 1, [&](size_t j) { return owns_chunk(j); });
    run(zkp::QG_LOOKUP, 0, cfg.n_lookup, 3, 5, [&](size_t i) { return owns_col(cfg.adv_lookup0() + i); });
    // (The same expressions cut by COLUMN BLOCK instead of by kind -- k_quotient_blocks, round 5 -- read a quarter less and were 29 %
    // slower: tools/exp/patches/quotient_blocks.patch, profiles/r5_probes.md section 2.)
    const size_t E = e, G = groups.size();
    if (G > 96 || G * n * (size_t)q_rows * 32 > ws->cap(wsl::QUOTIENT_PARTIALS)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "too many quotient groups for the workspace");
    std::vector<Fr> ypow(G);
    for (size_t g = 0; g < G; ++g) ypow[g] = zk::zk_fr_to_29(fr_pow(y, E - 1 - last_e[g]));   // 2^261 form: constant operands of k_quotient_combine
    if (groups.empty()) groups.push_back(zkp::QGroup{});     // a rank that owns nothing still stages a (unread) entry
    if (ypow.empty()) ypow.push_back(Fr::zero());
    STAGE(groups_dev, zkp::QGroup, ws, groups.data(), groups.size() * sizeof(zkp::QGroup));
    STAGE(ypow_dev, Fr, ws, ypow.data(), ypow.size() * 32);
    const Fr gn = fr_pow(mont_u64(COSET_G), n), i4 = fr_pow(wext, n);
    Fr zinv[4], cur = gn;
    for (int t = 0; t < 4; ++t) {
      zinv[t] = zk::zk_fr_to_29(fr_inv(cur - Fr::one()));
      cur = cur * i4;
    }
    STAGE(zinv_dev, Fr, ws, zinv, 4 * 32);
    CK(flush_staged(ctx, ws));
    zkp::QArgs qa = quotient_args(groups_dev, q_rows);
    const size_t npts = n * (size_t)q_rows;
    if (W_sh == 1) {
      CK(launch_quotient(qa, 0, npts, G, ypow_dev, zinv_dev));
    } else {
      // h_ext receives this rank's share of the quotient (the sum over ITS expression groups); the W shares are gathered and added up
      // -- field addition is not an RCCL reduction either.  One coset row at a time: the share of row k1 (n values: 16 MB at k = 19)
      // goes onto the communicator's stream as soon as it is formed and travels over xGMI while the groups of row k1 + 1 are
      // evaluated; only the last row's gather is exposed.  (The callback transport of the tests completes each gather in place.)
      CK(grow_qgather(ctx, ws, (size_t)W_sh * npts * 32));
      for (int k1 = 0; k1 < q_rows; ++k1) {
        CK(launch_quotient(qa, (size_t)k1 * n, n, G, ypow_dev, zinv_dev));
        CK(zkfhe_comm_all_gather_async(ctx, srs->comm, ws->h_ext.fr() + (size_t)k1 * n, ws->qgather.fr() + (size_t)k1 * W_sh * n, n * 32));
      }
      CK(sum_shares((size_t)q_rows, ws->h_ext.fr()));
    }
    const Fr g = mont_u64(COSET_G);
    if (q_rows == 4) {
      CK(zkfhe_coset_ntt_batch(ctx, (const zkfhe_fr *)ws->h_ext.p, (zkfhe_fr *)ws->h_c.p, 1, (int)k, 2, (const zkfhe_fr *)&g, 1));
    } else {
      // three size-n inverse transforms, then the 3x3 Vandermonde solve per coefficient (prover_kernels.hip.hpp: k_ext3_combine)
      Fr *rows3 = ws->ext3_rows();              // in the partials, dead after the combine; 3n values
      const Fr *pw = pk->ext3_pw.fr();           // (g w_ext^t)^-i, resident in the key
      CK(zkfhe_ntt_batch_to(ctx, (const zkfhe_fr *)ws->h_ext.p, (zkfhe_fr *)rows3, 3, (int)k, 1));
      const Fr c[3] = {fr_pow(g, n), fr_pow(g * wext, n), fr_pow(g * wext * wext, n)};   // (g w_ext^t)^n
      zkp::k_ext3_combine<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(rows3, pw, vandermonde3_inverse(c), n, ws->h_c.fr());
      ZK_LAUNCH_CHECK(ctx);
    }
    CK(commit_cols_out(ctx, srs, srs->g, ws->h_c.fr(), 3, ws, h_commit));
    if (q_rows == 4) {
      // the quotient must have degree < 3n: a non-zero top quarter means a violated constraint
      std::vector<U256> top(8);
      CK(zkfhe_download(ctx, top.data(), ws->quotient_top(), 8 * 32));
      for (const auto &v : top)
        if (!v.is_zero()) return zk_fail_msg(ctx, ZKFHE_EINVAL, "quotient degree too high: a constraint is violated");
    }
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ evaluations at x * w^rot (barycentric, Lagrange form)
  void add_item(const Fr *lagr, std::initializer_list<int> rots) {
    OpenItem it{{lagr, 0, {0, 0, 0, 0}}};
    for (int r : rots) it.job.rot[it.job.n_rot++] = r;
    items.push_back(it);
  }
  // dst = sum over m < msz of pw[m] * (column pp[m]), n rows; pw in the 2^261 form.  Long lists in chunks of 48 members (partial
  // sums in the quotient's partials buffer, dead by then), then one small reduction
  int lincomb(const Fr *const *pp, const Fr *pw, unsigned msz, Fr *dst) {
    const unsigned per = 48, chunks = (msz + per - 1) / per;
    if (chunks > 1 && (size_t)chunks * n * 32 <= ws->cap(wsl::LINCOMB_SUMS)) {
      dim3 lg(grid_for(ctx, n), chunks);
      zkp::k_lincomb_ptrs_chunked<<<lg, 256, 0, ctx->stream>>>(pp, pw, msz, per, n, ws->lincomb_sums());
      ZK_LAUNCH_CHECK(ctx);
      zkp::k_sum_rows<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(ws->lincomb_sums(), chunks, n, dst);
    } else {
      zkp::k_lincomb_ptrs<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(pp, pw, msz, n, dst);
    }
    ZK_LAUNCH_CHECK(ctx);
    return ZKFHE_OK;
  }
  int evaluations() {
    Fr *H_c = ws->H_c(), *H_l = ws->H_l();
    const Fr xn = fr_pow(x, n);
    const Fr w = dom->omega;
    pts_rot[0] = x;
    pts_rot[1] = x * w;
    pts_rot[2] = pts_rot[1] * w;
    pts_rot[3] = pts_rot[2] * w;
    pts_rot[4] = x * fr_pow(w, u);
    pts_rot[5] = x * dom->omega_inv;
    const size_t nch = cfg.n_chunks();
    for (unsigned c = 0; c < cfg.n_advice(); ++c) {
      const Fr *p = ws->adv_l.fr() + (size_t)c * n;
      if (c < cfg.n_gate()) add_item(p, {0, 1, 2, 3});
      else if (c < cfg.adv_rlc0()) add_item(p, {0});
      else add_item(p, {0, 1, 2});
    }
    for (unsigned c = 0; c < cfg.n_fixed(); ++c) add_item(pk->fixed_l.fr() + (size_t)c * n, {0});
    idx_H = items.size();
    add_item(H_l, {0});
    add_item(rand_l, {0});
    for (unsigned c = 0; c < cfg.n_perm(); ++c) add_item(pk->sigma_l.fr() + (size_t)c * n, {0});
    for (unsigned j = 0; j < nch; ++j) {
      if (j + 1 != nch) add_item(ws->pz_l.fr() + (size_t)j * n, {0, 1, 4});
      else add_item(ws->pz_l.fr() + (size_t)j * n, {0, 1});
    }
    for (unsigned i = 0; i < cfg.n_lookup; ++i) {
      add_item(ws->lz_l.fr() + (size_t)i * n, {0, 1});
      add_item(ws->la_l.fr() + (size_t)i * n, {0, 5});
      add_item(ws->ls_l.fr() + (size_t)i * n, {0});
    }
    // the evaluation jobs (column, rotations) depend on no challenge: they are staged with the round's first tables
    std::vector<zkp::EvalJob> jobs(items.size());
    for (size_t i = 0; i < items.size(); ++i) jobs[i] = items[i].job;
    // H(X) = h0 + x^n h1 + x^2n h2, and the random polynomial, in Lagrange form
    const Fr sc[3] = {zk::zk_fr_to_29(Fr::one()), zk::zk_fr_to_29(xn), zk::zk_fr_to_29(xn * xn)};   // k_lincomb_ptrs takes its scalars in the 2^261 form
    const Fr *ptrs[3] = {ws->h_c.fr(), ws->h_c.fr() + n, ws->h_c.fr() + 2 * n};
    STAGE(ptrs_dev, const Fr *, ws, ptrs, sizeof(ptrs));
    STAGE(sc_dev, Fr, ws, sc, sizeof(sc));
    STAGE(pts_dev, Fr, ws, pts_rot, sizeof(pts_rot));   // the six evaluation points go up with the same flush
    STAGE(jobs_dev, zkp::EvalJob, ws, jobs.data(), jobs.size() * sizeof(zkp::EvalJob));   // ... and so does the evaluation job list
    Fr *bw = ws->bary_weights();  // [6][n]
    const bool side_by_side = n <= 65536 && !ctx->chain_serial;   // short rows: H(X) and the weights' denominators (which depend on x alone) in one launch
    if (side_by_side) {
      const chain::Job hjob{0, 3, 0, -1};
      STAGE(hjob_dev, chain::Job, ws, &hjob, sizeof(hjob));
      CK(flush_staged(ctx, ws));
      const unsigned gx = grid_for(ctx, n), tail_rows = (grid_for(ctx, 6 * n) + gx - 1) / gx;
      zkp::k_chain_jobs<zkp::TAIL_BARY><<<dim3(gx, 1 + tail_rows), 256, 0, ctx->stream>>>(hjob_dev, 1, ptrs_dev, sc_dev, n, H_c, nullptr, pts_dev, 6, dom->fwd, bw);
      ZK_LAUNCH_CHECK(ctx);
    } else {
      CK(flush_staged(ctx, ws));
      CK(lincomb(ptrs_dev, sc_dev, 3, H_c));
    }
    CK(zkfhe_ntt_batch_to(ctx, (const zkfhe_fr *)H_c, (zkfhe_fr *)H_l, 1, (int)k, 0));
    if (!early_rand) CK(zkfhe_ntt_batch_to(ctx, (const zkfhe_fr *)rand_c, (zkfhe_fr *)rand_l, 1, (int)k, 0));   // early: transformed on the auxiliary stream at the start
    if (!side_by_side) {
      zkp::k_bary_den<<<grid_for(ctx, 6 * n), 256, 0, ctx->stream>>>(dom->fwd, pts_dev, 6, n, bw);
      ZK_LAUNCH_CHECK(ctx);
    }
    CK(zkfhe_fr_batch_invert(ctx, (zkfhe_fr *)bw, 6 * n));
    const Fr c = zk::zk_fr_to_29((xn - Fr::one()) * dom->n_inv);   // the weights in the 2^261 form: the constant operand of k_eval_jobs' nine-limb products
    zkp::k_bary_weights<<<grid_for(ctx, 6 * n), 256, 0, ctx->stream>>>(dom->fwd, c, 6 * n, n, bw);
    ZK_LAUNCH_CHECK(ctx);
    DevBuf &od = ws->evout;
    // One proof over several GPUs, long rows (k >= 14): the evaluation jobs are sharded by index -- rank r takes jobs
    // [per r, per (r + 1)) with per = ceil(J / W), every Lagrange column being present on every rank -- and the scalars are
    // all-gathered (per * 128 bytes per rank).  Short rows are not worth a collective.
    const bool shard_open = W_sh > 1 && k >= 14;
    const size_t per_rank = shard_open ? (jobs.size() + W_sh - 1) / W_sh : jobs.size();
    const size_t j_lo = shard_open ? std::min(jobs.size(), per_rank * r_sh) : 0, j_hi = shard_open ? std::min(jobs.size(), j_lo + per_rank) : jobs.size();
    if (shard_open && (per_rank * W_sh * 4 * 32 > od.bytes || per_rank * (W_sh + 1) * 4 * 32 > ws->cap(wsl::EVAL_SLICE)))
      return zk_fail_msg(ctx, ZKFHE_EINVAL, "too many ranks for the evaluation gather buffers");
    Fr *ev_dst = shard_open ? ws->eval_slice() : od.fr();   // my slice first (the quotient's extended values are dead by now)
    // long columns: 16 row slices per job (partial sums in the dead quotient buffer), then one small reduction
    const unsigned slices = (n > 32768 && (size_t)16 * jobs.size() * 4 * 32 <= ws->cap(wsl::EVAL_SLICES)) ? 16u : 1u;
    if (j_hi > j_lo) {
      const zkp::EvalJob *jp = jobs_dev + j_lo;
      const unsigned nj = (unsigned)(j_hi - j_lo);
      if (slices == 1) {
        zkp::k_eval_jobs<<<nj, 256, 0, ctx->stream>>>(jp, bw, n, ev_dst + (shard_open ? 0 : j_lo * 4));
      } else {
        zkp::k_eval_jobs<<<dim3(nj, slices), 256, 0, ctx->stream>>>(jp, bw, n, ws->eval_slices());
        ZK_LAUNCH_CHECK(ctx);
        zkp::k_sum_rows<<<grid_for(ctx, (size_t)nj * 4), 256, 0, ctx->stream>>>(ws->eval_slices(), slices, (size_t)nj * 4, ev_dst + (shard_open ? 0 : j_lo * 4));
      }
      ZK_LAUNCH_CHECK(ctx);
    }
    if (shard_open) CK(zkfhe_comm_all_gather(ctx, srs->comm, ev_dst, od.p, per_rank * 4 * 32));   // rank-major = job order
    if (jobs.size() * 4 > ws->out_ev_cap) return zk_fail_msg(ctx, ZKFHE_EINVAL, "more evaluations than the result block holds");
    // canonical values straight into pinned memory (the conversion kernel stores them there): no copy command
    CK(zkfhe_fr_from_mont(ctx, (const zkfhe_fr *)od.p, (zkfhe_fr *)ws->out_ev(), jobs.size() * 4));
    ZK_HIP(ctx, zk_wait(ctx));
    trace.mark("evaluations (GPU)");
    const U256 *ev = ws->out_ev();
    for (size_t i = 0; i < items.size(); ++i)
      for (int r = 0; r < items[i].job.n_rot; ++r) items[i].ev[r] = ev[i * 4 + r];
    return ZKFHE_OK;
  }
  // ------------------------------------------------------------ SHPLONK (halo2 ProverSHPLONK; Lagrange form, commitments are basis independent)
  int shplonk() {
    const OpenLayout layout(cfg);
    if (items.size() != layout.count || idx_H != layout.H) return zk_fail_msg(ctx, ZKFHE_EINVAL, "opening layout mismatch");
    std::vector<U256> evs;
    evs.reserve(items.size() * 2);
    for (size_t i = 0; i < items.size(); ++i) {
      if (i == idx_H) continue;  // implied by the identity, not written
      for (int r = 0; r < items[i].job.n_rot; ++r) evs.push_back(items[i].ev[r]);
    }
    tr.write_scalars(evs);
    const Fr yq = mont(tr.squeeze());
    trace.mark("transcript: evaluations");
    std::vector<int> all_rots;
    const std::vector<OpenSet> sets = intermediate_sets(layout, open_queries(cfg, layout), all_rots);
    const size_t ns = sets.size();
    Fr *F = ws->sh_F();  // [ns][n]
    if (ns > wsl::MAX_SETS) return zk_fail_msg(ctx, ZKFHE_EINVAL, "too many rotation sets");
    std::vector<zkp::ShSet> shsets(ns);
    // pointer and scalar tables of every set are staged first and go up with one flush; then the launches
    std::vector<const Fr *const *> set_ptrs(ns);
    std::vector<const Fr *> set_pw(ns);
    // short rows, one GPU: the sets' lists lie behind each other and every chunk of every set is a job of one launch (chain_jobs.hpp)
    const bool side_by_side = n <= 65536 && !ctx->chain_serial && !(W_sh > 1 && k >= 14);
    std::vector<size_t> set_sizes(ns);
    for (size_t j = 0; j < ns; ++j) set_sizes[j] = sets[j].members.size();
    const chain::Plan plan = chain::plan(set_sizes);
    std::vector<const Fr *> all_ptrs;
    std::vector<Fr> all_pw;
    all_ptrs.reserve(plan.members);
    all_pw.reserve(plan.members);
    for (size_t j = 0; j < ns; ++j) {
      const auto &mem = sets[j].members;
      std::vector<const Fr *> ptrs(mem.size());
      std::vector<Fr> pw(mem.size());
      Fr cur = Fr::one();
      const size_t np = sets[j].rots.size();
      if (np > 4) return zk_fail_msg(ctx, ZKFHE_EINVAL, "too many points in a rotation set");
      Fr comb[4] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
      for (size_t m = 0; m < mem.size(); ++m) {
        ptrs[m] = items[mem[m]].job.col;
        pw[m] = zk::zk_fr_to_29(cur);   // 2^261 form: the constant operand of k_lincomb_ptrs
        for (size_t t = 0; t < np; ++t) comb[t] = comb[t] + cur * mont(items[mem[m]].ev[layout.eval_slot(mem[m], sets[j].rots[t])]);
        cur = cur * yq;
      }
      if (side_by_side) {
        all_ptrs.insert(all_ptrs.end(), ptrs.begin(), ptrs.end());
        all_pw.insert(all_pw.end(), pw.begin(), pw.end());
      } else {
        STAGE(pd, const Fr *, ws, ptrs.data(), mem.size() * sizeof(void *));
        STAGE(sd, Fr, ws, pw.data(), mem.size() * 32);
        set_ptrs[j] = pd;
        set_pw[j] = sd;
      }
      // r_j: interpolation through (pts, comb), ascending coefficients
      zkp::ShSet &S = shsets[j];
      S.n_pts = (int)np;
      for (size_t t = 0; t < 4; ++t) S.pts[t] = t < np ? pts_rot[sets[j].rots[t]] : Fr::zero();
      interpolate4(S.pts, comb, np, S.rc);
    }
    // v follows yq with nothing absorbed in between: it is squeezed here, and the sets (r_j, points, v^j) go up with the same flush
    const Fr v = mont(tr.squeeze());
    Fr vj = Fr::one();
    for (size_t j = 0; j < ns; ++j) {
      shsets[j].vj = vj;
      shsets[j].coef = Fr::zero();
      shsets[j].r_u = Fr::zero();
      vj = vj * v;
    }
    STAGE(sets_dev, zkp::ShSet, ws, shsets.data(), ns * sizeof(zkp::ShSet));
    Fr *zs = ws->sh_zs();   // [ns][n]
    Fr *hq = ws->sh_hq(), *Wq = ws->sh_Wq(), *dinv = ws->sh_dinv();   // [n] each
    if (side_by_side) {
      if ((size_t)plan.slots * n * 32 > ws->cap(wsl::LINCOMB_SUMS)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "SHPLONK: partial sums do not fit the quotient buffer");
      STAGE(ptrs_dev, const Fr *, ws, all_ptrs.data(), all_ptrs.size() * sizeof(void *));
      STAGE(pw_dev, Fr, ws, all_pw.data(), all_pw.size() * 32);
      STAGE(jobs_dev, chain::Job, ws, plan.jobs.data(), plan.jobs.size() * sizeof(chain::Job));
      const chain::Sum no_sum{};   // no chunked set: nothing is staged, but not from a null pointer
      STAGE(sums_dev, chain::Sum, ws, plan.sums.empty() ? &no_sum : plan.sums.data(), plan.sums.size() * sizeof(chain::Sum));
      CK(flush_staged(ctx, ws));
      const unsigned gx = grid_for(ctx, n), nj = (unsigned)plan.jobs.size(), tail_rows = (grid_for(ctx, ns * n) + gx - 1) / gx;
      // k_sh_zs rides along while the launch cannot reach the 7 waves per SIMD its registers allow (a workgroup is 4 waves, a CU has 4
      // SIMDs); a fuller launch keeps the jobs at their own 8 waves and k_sh_zs in a launch of its own
      if ((size_t)gx * (nj + tail_rows) <= (size_t)7 * ctx->num_cu) {
        zkp::k_chain_jobs<zkp::TAIL_ZS><<<dim3(gx, nj + tail_rows), 256, 0, ctx->stream>>>(jobs_dev, nj, ptrs_dev, pw_dev, n, F, ws->lincomb_sums(), sets_dev, (unsigned)ns, dom->fwd, zs);
        ZK_LAUNCH_CHECK(ctx);
      } else {
        zkp::k_chain_jobs<zkp::TAIL_NONE><<<dim3(gx, nj), 256, 0, ctx->stream>>>(jobs_dev, nj, ptrs_dev, pw_dev, n, F, ws->lincomb_sums(), nullptr, 0, nullptr, nullptr);
        ZK_LAUNCH_CHECK(ctx);
        zkp::k_sh_zs<<<grid_for(ctx, ns * n), 256, 0, ctx->stream>>>(sets_dev, (unsigned)ns, dom->fwd, n, zs);
        ZK_LAUNCH_CHECK(ctx);
      }
      if (!plan.sums.empty()) {
        zkp::k_chain_sums<<<dim3(gx, (unsigned)plan.sums.size()), 256, 0, ctx->stream>>>(sums_dev, ws->lincomb_sums(), n, F);
        ZK_LAUNCH_CHECK(ctx);
      }
    } else {
      CK(flush_staged(ctx, ws));
      // One proof over several GPUs, long rows: every rank sums its share of a set's members (a k_lincomb_ptrs over zero members
      // writes zeros), the W partial combinations of all sets are all-gathered (ns n values per rank) and added up.
      const bool shard_sets = W_sh > 1 && k >= 14;
      if (shard_sets) CK(grow_qgather(ctx, ws, (size_t)W_sh * ns * n * 32));   // [set][rank][n]: the buffer of the quotient shares, grown if there are more sets than coset rows
      for (size_t j = 0; j < ns; ++j) {
        const size_t all = sets[j].members.size();
        const size_t m_lo = shard_sets ? all * r_sh / W_sh : 0, m_hi = shard_sets ? all * (r_sh + 1) / W_sh : all;
        CK(lincomb(set_ptrs[j] + m_lo, set_pw[j] + m_lo, (unsigned)(m_hi - m_lo), F + j * n));
        // set j's share goes onto the communicator's stream as soon as it is formed (16 MB per rank at k = 19) and travels while the
        // next set is combined; the sums wait for the join below
        if (shard_sets) CK(zkfhe_comm_all_gather_async(ctx, srs->comm, F + j * n, ws->qgather.fr() + j * (size_t)W_sh * n, n * 32));
      }
      if (shard_sets) CK(sum_shares(ns, F));
      zkp::k_sh_zs<<<grid_for(ctx, ns * n), 256, 0, ctx->stream>>>(sets_dev, (unsigned)ns, dom->fwd, n, zs);
      ZK_LAUNCH_CHECK(ctx);
    }
    CK(zkfhe_fr_batch_invert(ctx, (zkfhe_fr *)zs, ns * n));
    zkp::k_sh_h<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(sets_dev, (unsigned)ns, F, zs, dom->fwd, n, hq);
    ZK_LAUNCH_CHECK(ctx);
    std::vector<AffinePoint> hq_commit, w_commit;
    CK(commit_cols_out(ctx, srs, srs->g_lagrange, hq, 1, ws, hq_commit));
    tr.write_point(hq_commit[0]);
    const Fr uu = mont(tr.squeeze());
    trace.mark("shplonk h (GPU)");
    Fr ztu = Fr::one();
    for (int r : all_rots) ztu = ztu * (uu - pts_rot[r]);
    // halo2 normalises the final quotient by the difference vanishing polynomial of the first set ("z_0_diff_inv"): every
    // coefficient below carries that factor, so the kernel is unchanged
    Fr z0_diff_inv = Fr::one();
    zkp::ShW shw{};   // the constants that depend on u: by kernel argument
    for (size_t j = 0; j < ns; ++j) {
      Fr zdiff = Fr::one();
      for (int r : all_rots)
        if (std::find(sets[j].rots.begin(), sets[j].rots.end(), r) == sets[j].rots.end()) zdiff = zdiff * (uu - pts_rot[r]);
      if (j == 0) z0_diff_inv = fr_inv(zdiff);
      shsets[j].coef = shsets[j].vj * zdiff * z0_diff_inv;
      Fr ru = shsets[j].rc[3];
      for (int q = 2; q >= 0; --q) ru = ru * uu + shsets[j].rc[q];
      shsets[j].r_u = ru;
      shw.coef[j] = shsets[j].coef;
      shw.r_u[j] = ru;
    }
    ztu = ztu * z0_diff_inv;
    zkp::k_sh_den<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(dom->fwd, uu, n, dinv);
    ZK_LAUNCH_CHECK(ctx);
    CK(zkfhe_fr_batch_invert(ctx, (zkfhe_fr *)dinv, n));
    zkp::k_sh_w<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(shw, (unsigned)ns, F, hq, ztu, dinv, n, Wq);
    ZK_LAUNCH_CHECK(ctx);
    CK(commit_cols_out(ctx, srs, srs->g_lagrange, Wq, 1, ws, w_commit));
    tr.write_point(w_commit[0]);
    return ZKFHE_OK;
  }
};

// input_json: the CircuitInput text; or words (input_json == nullptr): the same numbers as machine words (zkfhe_bfv_prove_words)
int prove_impl(zkfhe_ctx *ctx, const zkfhe_srs *srs, zkfhe_bfv_pk *pk, const char *input_json, const FastInput *words, const uint8_t seed[32],
               std::vector<uint8_t> &proof, std::vector<U256> &instances, float *timings) {
  const double t_start = now_ms();
  ctx->cmd_count[ZK_CMD_KERNEL] = ctx->cmd_count[ZK_CMD_COPY] = ctx->cmd_count[ZK_CMD_FILL] = 0;   // zkfhe_ctx_last_proof_commands: this proof's
  Trace trace;
  const NttDomain *dom;
  CK(zk_domain(ctx, (int)pk->cfg.k, &dom));
  Workspace *ws;
  CK(get_workspace(ctx, pk, &ws));
  BackendGuard guard(ctx, ws);
  // One profile per proof (ctx.hpp), chosen here and kept to the end whatever happens to the gate meanwhile: throughput when the
  // admission gate is on -- the caller says it keeps the chip full --, latency otherwise.  ZKFHE_PROFILE=latency|throughput overrides
  // (read per proof, like ZKFHE_EARLY_P1: the tests switch it).  The auxiliary context's launches belong to the same proof.
  {
    const char *profile_env = getenv("ZKFHE_PROFILE");
    bool throughput = !srs->sharded() && HeavyGate::get().set(-1) > 0;   // a sharded proof ignores the gate (its ranks must choose alike)
    if (profile_env && !strcmp(profile_env, "throughput")) throughput = true;
    else if (profile_env && !strcmp(profile_env, "latency")) throughput = false;
    ctx->throughput = throughput;   // the auxiliary context exists from setup() on and takes it there
  }
  Proof P{ctx, srs, pk, pk->cfg, instances, trace, ws, dom};
  memcpy(P.rseed.w, seed, 32);
  CK(P.setup());
  std::vector<AffinePoint> pts;   // the commitments of the round in flight
  CK(P.phase0(input_json, words, pts));
  trace.mark("commit phase 0 (GPU)");
  ctx->proof_marks[0] = (float)(now_ms() - t_start);
  for (const auto &p : pts) P.tr.write_point(p);
  P.gamma_rlc = P.tr.squeeze();
  ctx->proof_marks[1] = (float)(now_ms() - t_start);
  CK(P.host_witness ? P.phase1_host(pts) : P.phase1_device(pts));
  trace.mark("commit phase 1 (GPU)");
  P.tr.write_points(pts);
  P.tr.squeeze();  // theta: squeezed in protocol order, unused by single-expression lookups
  CK(P.lookup_columns());
  trace.mark("lookup permute + commit");
  P.beta = mont(P.tr.squeeze());
  P.gamma = mont(P.tr.squeeze());
  GateHold gate;
  if (!srs->sharded()) gate.enter();   // a sharded proof's collectives must not wait for another rank's admission order
  CK(P.grand_products());
  CK(P.random_poly());
  P.y = mont(P.tr.squeeze());
  const double t_commit = now_ms();
  trace.mark("grand products + commits");
  CK(P.quotient(pts));
  gate.leave();
  for (const auto &p : pts) P.tr.write_point(p);
  P.x = mont(P.tr.squeeze());
  const double t_quot = now_ms();
  trace.mark("quotient");
  CK(P.evaluations());
  CK(P.shplonk());
  proof = P.tr.out;
  const double t_end = now_ms();
  trace.mark("evaluations + shplonk");
  ctx->proof_marks[2] = (float)(t_end - t_start);
  if (timings) {
    timings[0] = (float)(P.t_wit - t_start);
    timings[1] = (float)(t_commit - P.t_wit);
    timings[2] = (float)(t_quot - t_commit);
    timings[3] = (float)(t_end - t_quot);
    timings[4] = (float)(t_end - t_start);
  }
  return ZKFHE_OK;
}

int prove_out(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_bfv_pk *pk, const char *input_json, const FastInput *words, const uint8_t seed[32],
              uint8_t *proof_out, size_t proof_cap, size_t *proof_len, uint8_t *instances_out, size_t *n_instances, float *timings_ms) {
  std::vector<uint8_t> proof;
  std::vector<U256> inst;
  CK(prove_impl(ctx, srs, const_cast<zkfhe_bfv_pk *>(pk), input_json, words, seed, proof, inst, timings_ms));
  if (proof.size() > proof_cap) return zk_fail_msg(ctx, ZKFHE_EINVAL, "proof buffer too small");
  memcpy(proof_out, proof.data(), proof.size());
  *proof_len = proof.size();
  if (n_instances) {
    const size_t have = *n_instances;
    *n_instances = inst.size();
    if (instances_out) {
      if (have < inst.size()) return zk_fail_msg(ctx, ZKFHE_EINVAL, "instance buffer too small (the required count is returned in *n_instances)");
      memcpy(instances_out, inst.data(), inst.size() * 32);
    }
  }
  return ZKFHE_OK;
}

}  // namespace

extern "C" {

int zkfhe_bfv_prove(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_bfv_pk *pk, const char *input_json, const uint8_t seed[32],
                    uint8_t *proof_out, size_t proof_cap, size_t *proof_len, uint8_t *instances_out, size_t *n_instances, float *timings_ms) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, srs && pk && input_json && seed && proof_out && proof_len);
  try {
    pos::BulkClientScope in_flight;   // transcript.hpp bulk_ok(): the hash service is shared by the provers in flight
    return prove_out(ctx, srs, pk, input_json, nullptr, seed, proof_out, proof_cap, proof_len, instances_out, n_instances, timings_ms);
  } catch (const std::exception &e) {
    return zk_fail_msg(ctx, ZKFHE_EINVAL, e.what());
  }
}

// zkfhe_bfv_prove on the input as machine words: the key's N words per polynomial, cyclo = x^N + 1.  Same proof, instances and
// return codes as zkfhe_bfv_prove on the JSON that spells the same numbers.
int zkfhe_bfv_prove_words(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_bfv_pk *pk, const zkfhe_bfv_words *words, const uint8_t seed[32],
                          uint8_t *proof_out, size_t proof_cap, size_t *proof_len, uint8_t *instances_out, size_t *n_instances, float *timings_ms) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, srs && pk && words && seed && proof_out && proof_len);
  const uint64_t *src[8] = {words->pk0, words->pk1, words->m, words->u, words->e0, words->e1, words->c0, words->c1};
  for (const uint64_t *p : src) ZK_ARG(ctx, p != nullptr);
  try {
    pos::BulkClientScope in_flight;
    const size_t N = pk->prm.N;
    FastInput in;
    for (int k = 0; k < 8; ++k) in.a[k].assign(src[k], src[k] + N);
    in.a[8].assign(N + 1, 0);
    in.a[8][0] = in.a[8][N] = 1;
    return prove_out(ctx, srs, pk, nullptr, &in, seed, proof_out, proof_cap, proof_len, instances_out, n_instances, timings_ms);
  } catch (const std::exception &e) {
    return zk_fail_msg(ctx, ZKFHE_EINVAL, e.what());
  }
}

// Admission gate of the GPU-heavy middle of the proofs of this process (HeavyGate above): n > 0 = that many proofs inside at once,
// 0 = no gate, negative = query.  Returns the previous setting.  For a service that keeps its streams full (measured: 16 streams,
// 4 slots: 224 proofs/s against 209); a batch that starts and ends together gains nothing from it.
int zkfhe_prover_gate(int n) { return HeavyGate::get().set(n); }

// halo2's permute_expression_pair for the 8-bit range table, as the prover runs it (gpu_witness.hip.hpp k_lookup_permute): the
// parity hook of SURVEY.md section 8a row P4.
int zkfhe_lookup_permute(zkfhe_ctx *ctx, const zkfhe_fr *cols_dev, size_t n_cols, size_t n, uint32_t usable_rows, zkfhe_fr *a_dev, zkfhe_fr *s_dev, int *not_in_table) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, cols_dev && a_dev && s_dev && not_in_table && n_cols > 0 && n_cols < 65536 && usable_rows <= n && usable_rows >= 256);
  void *flag;   // the flag, then the histogram of the sliced kernels (long columns)
  CK(zk_scratch(ctx, 3, 64 + n_cols * 256 * sizeof(unsigned), &flag));
  ZK_HIP(ctx, zk_memset_async(ctx, flag, 0, 4, ctx->stream));
  CK(zkw::lookup_permute(ctx, (const Fr *)cols_dev, n, usable_rows, (unsigned)n_cols, (Fr *)a_dev, (Fr *)s_dev, (int *)flag, (unsigned *)((char *)flag + 64)));
  return zkfhe_download(ctx, not_in_table, flag, 4);
}

// Announce the input of a proof that will be made later with this key: its public inputs (examples/bfv.rs:118-122) are parsed now
// and `vk digest | public inputs` is absorbed on a helper thread into a transcript state that the zkfhe_bfv_prove of the SAME input
// picks up (prefix_cache.hpp PreHash; one-shot).  Host only: no context, no GPU work.  started / taken / pending (optional) receive
// the counters of this key; input_json == NULL only queries them.
int zkfhe_bfv_pk_prehash(const zkfhe_bfv_pk *pk_c, const char *input_json, uint64_t *started, uint64_t *taken, uint64_t *pending) {
  if (!pk_c) return ZKFHE_EINVAL;
  zkfhe_bfv_pk *pk = const_cast<zkfhe_bfv_pk *>(pk_c);
  int rc = ZKFHE_OK;
  if (input_json) {
    const uint32_t kind = pk->cfg.transcript;
    const U256 digest = pk->vk_digest;
    const BfvParams prm = pk->prm;
    PrefixCache *cache = &pk->prefix;
    // everything on the helper thread: the caller gets its thread back after one copy of the text (2.3 MB of JSON at N = 16384 take 15 ms to parse)
    const bool ok = pk->prehash.start(input_json, strlen(input_json), [kind, digest, prm, cache](const std::string &text, std::vector<U256> &inst, Transcript::State &out) {
      struct PublicInputsKnown {};   // thrown by the callback: phase 0 stops as soon as the public inputs are complete
      try {
        Context ctx0(CTX_PHASE0, false, false);
        std::vector<Cell> make_public;
        BfvState st;
        const auto on_public = [&](const std::vector<Cell> &pub) {
          inst.reserve(pub.size());
          for (const Cell &c : pub) inst.push_back(c.value);
          throw PublicInputsKnown{};
        };
        if (!bfv_phase0_fast(ctx0, text.c_str(), text.size(), prm, make_public, st, on_public))
          (void)bfv_phase0(ctx0, CircuitInput::parse_json(text.c_str()), prm, make_public, on_public);
        throw std::runtime_error("phase 0 ended without public inputs");
      } catch (const PublicInputsKnown &) {
      }
      const size_t n_key = std::min<size_t>(inst.size(), 2 * (size_t)prm.N);
      Transcript tr(kind);
      tr.common_scalar(digest);
      Transcript::State mid;
      size_t from = 0;
      if (n_key && cache->capacity()) {
        if (cache->lookup(inst.data(), n_key, mid)) {
          tr.restore(mid);
        } else {
          tr.common_scalars_async(std::vector<U256>(inst.begin(), inst.begin() + (long)n_key));
          mid = tr.snapshot();
          cache->insert(inst.data(), n_key, mid);
        }
        from = n_key;
      }
      tr.common_scalars_async(std::vector<U256>(inst.begin() + (long)from, inst.end()));
      out = tr.snapshot();
    });
    if (!ok) rc = ZKFHE_EINVAL;   // PreHash::MAX_PENDING announced proofs are waiting already
  }
  pk->prehash.stats(started, taken, pending);
  return rc;
}

// The phase-1 gate stream exactly as the GPU witness generator produces it (gpu_witness.hip.hpp), for a caller-chosen
// challenge: the cells of examples/bfv.rs:171-301 in halo2-base order, canonical values.  This is the parity hook of
// tests compare it cell for cell with the oracle's restatement of src/poly_chip.rs.
int zkfhe_bfv_witness_stream(zkfhe_ctx *ctx, const zkfhe_bfv_pk *pk_c, const char *input_json, const uint8_t gamma_le[32], uint8_t *cells_out,
                             size_t cap_cells, size_t *n_cells) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, pk_c && input_json && gamma_le && n_cells);
  zkfhe_bfv_pk *pk = const_cast<zkfhe_bfv_pk *>(pk_c);
  *n_cells = pk->gate1_cells;
  if (!cells_out) return ZKFHE_OK;
  ZK_ARG(ctx, cap_cells >= pk->gate1_cells);
  try {
    Workspace *ws;
    CK(get_workspace(ctx, pk, &ws));
    CK(zkfhe_sync(ctx));
    BackendGuard guard(ctx, ws);
    Context ctx0(CTX_PHASE0, false, false), ctx_rlc(CTX_RLC1, true, false);
    std::vector<Cell> make_public;
    BfvState st;
    if (!bfv_phase0_fast(ctx0, input_json, strlen(input_json), pk->prm, make_public, st)) st = bfv_phase0(ctx0, CircuitInput::parse_json(input_json), pk->prm, make_public);
    U256 gamma, evals[12];
    memcpy(gamma.l, gamma_le, 32);
    if (!(gamma < fe::MOD)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "gamma is not a canonical Fr value");
    CK(alloc_witness_buffers(ctx, pk, ws));
    ws->ring_off = ws->ring_flushed = 0;   // the stream is idle (synchronised above): the staging ring starts over, as in a proof
    GpuPhase1 g1(ctx, pk, ws);
    CK(g1.launch(st));
    bfv_phase1_rlc(st, ctx_rlc, gamma, evals);
    CK(g1.finish(evals, zkp::RngRows{}));   // the cells only: no blinding rows here
    CK(zkfhe_fr_from_mont(ctx, (const zkfhe_fr *)ws->stream.p, (zkfhe_fr *)ws->stream.p, pk->gate1_cells));
    ZK_HIP(ctx, zk_memcpy_async(ctx, cells_out, ws->stream.p, pk->gate1_cells * 32, hipMemcpyDeviceToHost, ctx->stream));
    CK(zkfhe_sync(ctx));
    return ZKFHE_OK;
  } catch (const std::exception &e) {
    return zk_fail_msg(ctx, ZKFHE_EINVAL, e.what());
  }
}

}  // extern "C"
