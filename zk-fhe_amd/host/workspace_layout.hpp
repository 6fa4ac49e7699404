// The layout of the prover workspace (workspace.hpp): plain host code, no HIP.  For every device and pinned buffer its size, and for
// every buffer that is carved up or lent out a named region per use: where it lies, how long it is and in which steps of a proof it
// is live.  workspace.hip allocates from this table and the accessors of Workspace hand out its regions; consistent() says that every
// region lies inside its buffer and that two regions of one buffer that are live in the same step do not overlap.  Whether a column
// of scratch is free in some round is a lookup here.
//
// Sizes are bytes.  A field element is 32 bytes, a column n of them; a host-read point slot is 128 bytes (workspace.hpp PT_SLOT).
#pragma once
#include <cstddef>
#include <cstdint>

namespace wsl {

constexpr size_t FR = 32;
constexpr size_t PT_SLOT = 128;
constexpr size_t MAX_SETS = 8;       // SHPLONK rotation sets: F and zs have this many columns of misc each
constexpr size_t EVAL_POINTS = 6;    // x w^0..3, x w^u, x w^-1: one column of barycentric weights each
constexpr size_t SMALL_SLOTS = 4096; // beta delta^i per permutation column; the chunk / lookup totals start behind them
constexpr size_t RING_BYTES = (size_t)4 << 20;

// what the layout depends on.  gate1_cells and n_inv_slots are known only after keygen, which already needs a workspace: the buffers
// of the witness generator (second_stage() below) are sized from a second make() with them filled in; no size of the first
// stage reads them.
struct Shape {
  size_t n;          // rows, 2^k
  unsigned ext_rows; // cosets of the extended domain: 3, or 4 for a key that checks the quotient's degree
  unsigned n_advice, n_fixed, n_gate, n_gate0, n_rlc, n_lookup, n_perm, n_chunks;
  size_t N;          // BFV ring degree
  size_t gate1_cells, n_inv_slots;
};

// The steps of a proof in the order of prove_impl.  A round is split where a buffer changes hands inside it: the grand products'
// factors are consumed by the inversion before the scan borrows `den`, the quotient's partials by the combine before the
// interpolation borrows them.  (The serial grand products run RATIOS, SCAN twice: permutation, then lookups.)
enum Step : unsigned { KEYGEN, SETUP, PHASE1, PRODUCTS_RATIOS, PRODUCTS_SCAN, QUOTIENT_EVAL, QUOTIENT_INTERP, EVALS, SHPLONK, N_STEPS };
constexpr unsigned bit(Step s) { return 1u << s; }
constexpr unsigned span(Step a, Step b) { return (bit(b) << 1) - bit(a); }   // a .. b inclusive
constexpr unsigned PROOF = span(SETUP, SHPLONK), ALWAYS = span(KEYGEN, SHPLONK);

enum Buf : unsigned {
  // device, first stage (get_workspace)
  ALL_L, ALL_EXT, TMP_C, PARTIALS, H_EXT, H_C, MISC, POINTS, NUM, DEN, SMALL, EVOUT, POLYIO,
  // device, second stage (the first proof after keygen)
  STREAM, POOL, INVTMP, DEV_RING,
  // device, grown by the first sharded proof to ranks x max(ext_rows, rotation sets) columns: not sized here
  QGATHER,
  // pinned, first stage
  HOST_ADV, HOST_BLIND,
  // pinned, second stage
  HOST_POOL, HOST_POLY, RING, HOST_OUT, HOST_PTS, HOST_EARLY, HOST_EARLY_ERR, HOST_RAND_PT,
  N_BUFS
};
constexpr bool pinned(Buf b) { return b >= HOST_ADV; }
constexpr bool second_stage(Buf b) { return (b >= STREAM && b <= DEV_RING) || b >= HOST_POOL; }

enum Reg : unsigned {
  // all_l / all_ext: every polynomial of one proof, Lagrange form and on the extended coset, in one order
  ADV_L, LA_L, LS_L, PZ_L, LZ_L, INST_L, ADV_EXT, LA_EXT, LS_EXT, PZ_EXT, LZ_EXT, INST_EXT,
  // misc: 32 columns
  KEY_L_ROWS, BARY_WEIGHTS, RAND_C, RAND_L, H_COEFF, H_LAGR, SH_F, SH_ZS, SH_HQ, SH_WQ, SH_DINV,
  // small
  BETA_DELTA, CHUNK_TOTALS,
  // partials
  QUOTIENT_PARTIALS, EXT3_ROWS, EVAL_SLICES, LINCOMB_SUMS,
  // den, h_ext, h_c, tmp_c
  DEN_FACTORS, PREFIX_SEGMENTS, QUOTIENT_VALUES, EVAL_SLICE, QUOTIENT_COEFFS, QUOTIENT_TOP, EXTEND_SCRATCH, PATCH_COLS,
  // host_out
  OUT_POINTS, OUT_EVALS, OUT_FLAGS,
  N_REGS
};

// The accessors of Workspace, generated from this list: X(name, region, element type).  An accessor is the only way to an address
// inside a carved or lent buffer, and its name is the name of its region.
#define WSL_ACCESSORS(X)                                                                                                              \
  X(key_l_rows, KEY_L_ROWS, Fr) X(bary_weights, BARY_WEIGHTS, Fr) X(rand_c, RAND_C, Fr) X(rand_l, RAND_L, Fr) X(H_c, H_COEFF, Fr)      \
  X(H_l, H_LAGR, Fr) X(sh_F, SH_F, Fr) X(sh_zs, SH_ZS, Fr) X(sh_hq, SH_HQ, Fr) X(sh_Wq, SH_WQ, Fr) X(sh_dinv, SH_DINV, Fr)             \
  X(beta_delta, BETA_DELTA, Fr) X(chunk_totals, CHUNK_TOTALS, Fr) X(quotient_partials, QUOTIENT_PARTIALS, Fr)                         \
  X(ext3_rows, EXT3_ROWS, Fr) X(eval_slices, EVAL_SLICES, Fr) X(lincomb_sums, LINCOMB_SUMS, Fr) X(prefix_segments, PREFIX_SEGMENTS, Fr) \
  X(eval_slice, EVAL_SLICE, Fr) X(quotient_top, QUOTIENT_TOP, Fr) X(extend_scratch, EXTEND_SCRATCH, Fr) X(patch_cols, PATCH_COLS, Fr)  \
  X(out_pts, OUT_POINTS, uint8_t) X(out_ev, OUT_EVALS, U256) X(out_flags, OUT_FLAGS, int)

struct Region {
  const char *name;
  Buf buf;
  size_t off, len;
  unsigned live;   // bits of Step
};

struct Layout {
  size_t bytes[N_BUFS];
  Region reg[N_REGS];
  size_t n_all;   // columns of all_l
};

inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

inline Layout make(const Shape &s) {
  Layout L{};
  const size_t col = s.n * FR, ecol = (size_t)s.ext_rows * col;
  const size_t n_all = (size_t)s.n_advice + 3 * (size_t)s.n_lookup + s.n_chunks + 1;
  const size_t max_items = (size_t)s.n_advice + s.n_fixed + 2 + s.n_perm + s.n_chunks + 3 * (size_t)s.n_lookup;   // opened polynomials
  // quotient partials: one row set (ext_rows * n values) per expression group -- the groups the quotient round cuts (8 gates, all RLC
  // gates, 32 chaining terms, 4 permutation chunks, 3 lookups per group; a rank of a sharded proof evaluates a contiguous share: at
  // most one more group per kind), not a flat 96 x 4 columns (6 GB at k = 19).  At least 96 columns for the later rounds' sums.
  const size_t groups = ((size_t)s.n_gate + 7) / 8 + 1 + 2 + ((size_t)s.n_chunks + 31) / 32 + ((size_t)s.n_chunks + 3) / 4 + ((size_t)s.n_lookup + 2) / 3 + 8;
  const size_t n_prod = (size_t)s.n_chunks + s.n_lookup;   // grand-product columns: permutation chunks, then lookups
  const size_t out_pts = max_sz(n_all, s.n_perm) + 16;

  L.n_all = n_all;
  L.bytes[ALL_L] = n_all * col;
  L.bytes[ALL_EXT] = n_all * ecol;
  L.bytes[TMP_C] = max_sz(n_all, s.n_perm) * col;
  L.bytes[PARTIALS] = max_sz(groups * s.ext_rows, 96) * col;
  L.bytes[H_EXT] = 4 * col;
  L.bytes[H_C] = 4 * col;
  L.bytes[MISC] = 32 * col;
  L.bytes[POINTS] = max_sz(n_all, s.n_perm) * 64 + 64;
  L.bytes[NUM] = n_prod * col;
  L.bytes[DEN] = n_prod * col;
  L.bytes[SMALL] = (SMALL_SLOTS + n_prod) * FR;
  L.bytes[EVOUT] = (max_items + 64) * 4 * FR;   // + the padding of the sharded evaluations' all-gather (equal slices per rank)
  L.bytes[POLYIO] = 4 * col;
  L.bytes[STREAM] = (s.gate1_cells + 8) * FR;
  L.bytes[POOL] = 40 * (2 * s.N + 8) * FR;
  L.bytes[INVTMP] = (s.n_inv_slots + 8) * FR;
  L.bytes[DEV_RING] = RING_BYTES;
  L.bytes[QGATHER] = 0;
  L.bytes[HOST_ADV] = (size_t)s.n_advice * col;
  L.bytes[HOST_BLIND] = max_sz(2 * (size_t)s.n_lookup, 2) * col;
  L.bytes[HOST_POOL] = 24 * (2 * s.N + 8) * FR;
  L.bytes[HOST_POLY] = (2 * s.N + 8) * FR;
  L.bytes[RING] = RING_BYTES;
  L.bytes[HOST_OUT] = out_pts * PT_SLOT + max_items * 4 * FR + 256;
  L.bytes[HOST_PTS] = ((size_t)s.n_gate0 + 1) * PT_SLOT;
  L.bytes[HOST_EARLY] = ((size_t)s.n_advice + 2 * (size_t)s.n_lookup + 16) * PT_SLOT;
  L.bytes[HOST_EARLY_ERR] = 64;
  L.bytes[HOST_RAND_PT] = PT_SLOT;

  {   // [advice | la | ls | pz | lz | instance]: one iNTT launch and one coset-NTT launch cover all of them
    size_t o = 0;
    auto take = [&](Reg l, const char *ln, Reg e, const char *en, size_t cols) {
      L.reg[l] = {ln, ALL_L, o * col, cols * col, ALWAYS};
      L.reg[e] = {en, ALL_EXT, o * ecol, cols * ecol, bit(QUOTIENT_EVAL)};
      o += cols;
    };
    take(ADV_L, "adv_l", ADV_EXT, "adv_ext", s.n_advice);
    take(LA_L, "la_l", LA_EXT, "la_ext", s.n_lookup);
    take(LS_L, "ls_l", LS_EXT, "ls_ext", s.n_lookup);
    take(PZ_L, "pz_l", PZ_EXT, "pz_ext", s.n_chunks);
    take(LZ_L, "lz_l", LZ_EXT, "lz_ext", s.n_lookup);
    take(INST_L, "inst_l", INST_EXT, "inst_ext", 1);
  }
  // misc, by column.  Columns 6, 7 and 31 are free in every step; [0, 8) and [10, 32) are free from SETUP to QUOTIENT_INTERP.
  L.reg[KEY_L_ROWS] = {"key_l_rows", MISC, 0, 3 * col, bit(KEYGEN)};                // l_0, l_last, l_active before their extension
  L.reg[BARY_WEIGHTS] = {"bary_weights", MISC, 0, EVAL_POINTS * col, bit(EVALS)};
  // the random polynomial, coefficients and Lagrange form: written on the AUXILIARY stream at setup while the main stream runs phase
  // 0; the main stream waits for the event before the evaluation round.  rand_l is an opened column: SHPLONK sums it.
  L.reg[RAND_C] = {"rand_c", MISC, 8 * col, col, span(SETUP, EVALS)};
  L.reg[RAND_L] = {"rand_l", MISC, 9 * col, col, span(SETUP, SHPLONK)};
  L.reg[H_COEFF] = {"H_c", MISC, 10 * col, col, bit(EVALS)};
  L.reg[H_LAGR] = {"H_l", MISC, 11 * col, col, span(EVALS, SHPLONK)};               // opened, like rand_l
  L.reg[SH_F] = {"sh_F", MISC, 12 * col, MAX_SETS * col, bit(SHPLONK)};
  L.reg[SH_ZS] = {"sh_zs", MISC, 20 * col, MAX_SETS * col, bit(SHPLONK)};
  L.reg[SH_HQ] = {"sh_hq", MISC, 28 * col, col, bit(SHPLONK)};
  L.reg[SH_WQ] = {"sh_Wq", MISC, 29 * col, col, bit(SHPLONK)};
  L.reg[SH_DINV] = {"sh_dinv", MISC, 30 * col, col, bit(SHPLONK)};
  // small: the quotient reads beta delta^i again
  L.reg[BETA_DELTA] = {"beta_delta", SMALL, 0, SMALL_SLOTS * FR, span(PRODUCTS_RATIOS, QUOTIENT_EVAL)};
  L.reg[CHUNK_TOTALS] = {"chunk_totals", SMALL, SMALL_SLOTS * FR, n_prod * FR, span(PRODUCTS_RATIOS, PRODUCTS_SCAN)};
  // partials: the groups a proof cuts, the slices and the chunks depend on the rank count and on runtime lists, so each use names
  // the whole buffer as the room it may grow into and keeps its capacity test where it is used
  L.reg[QUOTIENT_PARTIALS] = {"quotient_partials", PARTIALS, 0, L.bytes[PARTIALS], bit(QUOTIENT_EVAL)};
  L.reg[EXT3_ROWS] = {"ext3_rows", PARTIALS, 0, 3 * col, bit(QUOTIENT_INTERP)};     // three-coset keys: the rows' inverse transforms
  L.reg[EVAL_SLICES] = {"eval_slices", PARTIALS, 0, L.bytes[PARTIALS], bit(EVALS)}; // long columns: 16 row slices per evaluation job
  L.reg[LINCOMB_SUMS] = {"lincomb_sums", PARTIALS, 0, L.bytes[PARTIALS], bit(SHPLONK)};   // chunks of 48 members: lincomb's, or the side-by-side plan's slots
  // den: the ratios' denominators until the inversion, then (long columns, n > 2^16) the segment products of the scan
  L.reg[DEN_FACTORS] = {"den", DEN, 0, L.bytes[DEN], bit(PRODUCTS_RATIOS)};
  L.reg[PREFIX_SEGMENTS] = {"prefix_segments", DEN, 0, s.n > 65536 ? n_prod * (s.n / 32768) * FR : 0, bit(PRODUCTS_SCAN)};
  // h_ext: the quotient on the coset rows; then a rank's slice of the sharded evaluations in front of the gathered ones
  L.reg[QUOTIENT_VALUES] = {"h_ext", H_EXT, 0, ecol, span(QUOTIENT_EVAL, QUOTIENT_INTERP)};
  L.reg[EVAL_SLICE] = {"eval_slice", H_EXT, 0, L.bytes[H_EXT], bit(EVALS)};
  // h_c: h0 | h1 | h2, and with four coset rows the top quarter, which must be zero
  L.reg[QUOTIENT_COEFFS] = {"h_c", H_C, 0, 3 * col, span(QUOTIENT_INTERP, EVALS)};
  L.reg[QUOTIENT_TOP] = {"quotient_top", H_C, 3 * col, s.ext_rows == 4 ? col : 0, bit(QUOTIENT_INTERP)};
  // tmp_c: coefficient forms on their way to the coset; the dense correction columns of the early phase-1 commitment (one per
  // phase-1 gate column at the most)
  L.reg[EXTEND_SCRATCH] = {"extend_scratch", TMP_C, 0, L.bytes[TMP_C], bit(KEYGEN) | bit(QUOTIENT_EVAL)};
  L.reg[PATCH_COLS] = {"patch_cols", TMP_C, 0, (size_t)(s.n_gate - s.n_gate0) * col, bit(PHASE1)};
  // host_out: what the host reads is written by the kernels into this block, [points | evaluations | flags]
  L.reg[OUT_POINTS] = {"out_pts", HOST_OUT, 0, out_pts * PT_SLOT, PROOF};
  L.reg[OUT_EVALS] = {"out_ev", HOST_OUT, out_pts * PT_SLOT, max_items * 4 * FR, PROOF};
  L.reg[OUT_FLAGS] = {"out_flags", HOST_OUT, out_pts * PT_SLOT + max_items * 4 * FR, 256, PROOF};
  return L;
}

// every region inside its buffer; no two regions of one buffer that share a step overlap.  *a, *b (optional): the offenders.
inline bool consistent(const Layout &L, const Region **a = nullptr, const Region **b = nullptr) {
  for (unsigned i = 0; i < N_REGS; ++i) {
    const Region &r = L.reg[i];
    if (!r.name || r.buf >= N_BUFS || r.off > L.bytes[r.buf] || r.len > L.bytes[r.buf] - r.off) {
      if (a) *a = &r;
      if (b) *b = nullptr;
      return false;
    }
    for (unsigned j = 0; j < i; ++j) {
      const Region &q = L.reg[j];
      if (q.buf == r.buf && (q.live & r.live) && q.len && r.len && q.off < r.off + r.len && r.off < q.off + q.len) {
        if (a) *a = &q;
        if (b) *b = &r;
        return false;
      }
    }
  }
  return true;
}

inline size_t total_bytes(const Layout &L, bool pinned_side) {
  size_t t = 0;
  for (unsigned b = 0; b < N_BUFS; ++b)
    if (pinned((Buf)b) == pinned_side) t += L.bytes[b];
  return t;
}

}  // namespace wsl
