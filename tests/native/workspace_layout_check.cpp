// The prover workspace's layout (zk-fhe_amd/host/workspace_layout.hpp) on the host alone, for the toy circuit (k = 9, N = 8), the pinned
// k = 13 layout of tests/golden/bfv/bfv_config.json, the k = 16 and k = 19 configurations of bench.py and the widest admissible shape
// (4096 permutation columns), each with 3 and 4 coset rows: the layout is consistent, every accessor of Workspace hands out a region
// of the table under its own name, and the device / pinned totals are the totals of the allocation formulas this table replaced less
// exactly the buffers it dropped.  A layout with two same-step regions pushed onto each other is reported inconsistent.
// Built plain and with -fsanitize=address,undefined by tests/test_workspace_layout_host.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstring>

#include "workspace_layout.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("line %d: %s fails (%s)\n", __LINE__, #cond, what); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// Column counts: the oracle's auto-configuration of the toy circuit, bfv_config.json, zkfhe_bfv_auto_config on bench.py's k16 / k19
// inputs; gate1_cells is the phase-1 gate stream of those circuits (the widest shape: 400 cells per column), n_inv_slots stands at 2 N.
// dev0 / pin0: total device and pinned bytes of one workspace by the formulas in use before this table existed, which allocated two
// more device buffers -- the evaluation job list (items * 72 + 256 bytes, items = the opened polynomials) and a 256-byte flag block,
// neither ever read -- and a flat 1 MiB for `small`, of which only (4096 + n_chunks + n_lookup) field elements are used.
struct Case {
  const char *name;
  unsigned k, ext_rows;
  size_t N;
  unsigned n_gate0, n_gate1, n_lookup, n_rlc;
  size_t gate1_cells, n_inv_slots;
  unsigned long long dev0, pin0;
};
const Case CASES[] = {
    {"toy", 9, 3, 8, 1, 20, 5, 1, 9540, 16, 13315264ull, 4851008ull},
    {"toy", 9, 4, 8, 1, 20, 5, 1, 9540, 16, 14265536ull, 4851008ull},
    {"k13", 13, 3, 1024, 3, 153, 36, 5, 1231992, 2048, 719165832ull, 76545728ull},
    {"k13", 13, 4, 1024, 3, 153, 36, 5, 1231992, 2048, 844470664ull, 76545728ull},
    {"k16", 16, 3, 4096, 2, 124, 34, 3, 8073420, 8192, 4913411504ull, 495358272ull},
    {"k16", 16, 4, 4096, 2, 124, 34, 3, 8073420, 8192, 5777438128ull, 495358272ull},
    {"k19", 19, 3, 16384, 1, 62, 17, 2, 32293068, 32768, 20476170752ull, 1976656320ull},
    {"k19", 19, 4, 16384, 1, 62, 17, 2, 32293068, 32768, 24066494976ull, 1976656320ull},
    {"widest", 9, 3, 8, 1, 4000, 92, 1, 1600000, 16, 711488192ull, 77536832ull},
    {"widest", 9, 4, 8, 1, 4000, 92, 1, 1600000, 16, 834990784ull, 77536832ull},
};

// the derived counts of CircuitConfig (bfv_circuit.hpp): permutation chunks of 2 columns
wsl::Shape shape_of(const Case &c) {
  wsl::Shape s{};
  s.n = (size_t)1 << c.k;
  s.ext_rows = c.ext_rows;
  s.n_gate0 = c.n_gate0;
  s.n_gate = c.n_gate0 + c.n_gate1;
  s.n_rlc = c.n_rlc;
  s.n_lookup = c.n_lookup;
  s.n_advice = s.n_gate + s.n_lookup + s.n_rlc;
  s.n_fixed = s.n_gate + s.n_rlc + 2;
  s.n_perm = s.n_advice + 2;
  s.n_chunks = (s.n_perm + 1) / 2;
  s.N = c.N;
  s.gate1_cells = c.gate1_cells;
  s.n_inv_slots = c.n_inv_slots;
  return s;
}

struct Accessor {
  const char *name;
  wsl::Reg reg;
};
#define X(name, reg, T) {#name, wsl::reg},
const Accessor ACCESSORS[] = {WSL_ACCESSORS(X)};
#undef X

void check(const Case &c) {
  char what[64];
  snprintf(what, sizeof what, "%s, %u coset rows", c.name, c.ext_rows);
  const wsl::Shape s = shape_of(c);
  const wsl::Layout L = wsl::make(s);
  const wsl::Region *a = nullptr, *b = nullptr;
  const bool ok = wsl::consistent(L, &a, &b);
  if (!ok) printf("%s: %s %s %s\n", what, a ? a->name : "?", b ? "overlaps" : "leaves its buffer", b ? b->name : "");
  CHECK(ok);
  // an accessor hands out a region of the table, the one of its name; no two accessors share one
  bool seen[wsl::N_REGS] = {};
  for (const Accessor &acc : ACCESSORS) {
    CHECK(acc.reg < wsl::N_REGS);
    if (acc.reg >= wsl::N_REGS) continue;
    CHECK(L.reg[acc.reg].name && !strcmp(L.reg[acc.reg].name, acc.name));
    CHECK(!seen[acc.reg]);
    seen[acc.reg] = true;
    CHECK(L.reg[acc.reg].live != 0 && L.reg[acc.reg].live < (1u << wsl::N_STEPS));
  }
  // the numeric layout of misc and small, and the constants the prover tests against
  const size_t col = s.n * 32;
  CHECK(L.bytes[wsl::MISC] == 32 * col);
  CHECK(L.reg[wsl::BARY_WEIGHTS].off == 0 && L.reg[wsl::BARY_WEIGHTS].len == 6 * col && wsl::EVAL_POINTS == 6);
  CHECK(L.reg[wsl::RAND_C].off == 8 * col && L.reg[wsl::RAND_L].off == 9 * col && L.reg[wsl::H_COEFF].off == 10 * col && L.reg[wsl::H_LAGR].off == 11 * col);
  CHECK(L.reg[wsl::SH_F].off == 12 * col && L.reg[wsl::SH_ZS].off == 20 * col && L.reg[wsl::SH_F].len == 8 * col && L.reg[wsl::SH_ZS].len == 8 * col && wsl::MAX_SETS == 8);
  CHECK(L.reg[wsl::SH_HQ].off == 28 * col && L.reg[wsl::SH_WQ].off == 29 * col && L.reg[wsl::SH_DINV].off == 30 * col);
  CHECK(L.reg[wsl::BETA_DELTA].off == 0 && L.reg[wsl::CHUNK_TOTALS].off == 4096 * 32);
  CHECK(s.n_perm <= wsl::SMALL_SLOTS && (size_t)s.n_chunks + s.n_lookup <= wsl::SMALL_SLOTS);
  // rand_c / rand_l are written on the auxiliary stream during setup: live from there to the evaluations at least
  CHECK((L.reg[wsl::RAND_C].live & wsl::span(wsl::SETUP, wsl::EVALS)) == wsl::span(wsl::SETUP, wsl::EVALS));
  CHECK((L.reg[wsl::RAND_L].live & wsl::span(wsl::SETUP, wsl::EVALS)) == wsl::span(wsl::SETUP, wsl::EVALS));
  // the four-coset layout: partials of groups x 4 rows, the fourth column of h_c
  CHECK(L.bytes[wsl::PARTIALS] % ((size_t)s.ext_rows * col) == 0 || L.bytes[wsl::PARTIALS] == 96 * col);
  CHECK(L.reg[wsl::QUOTIENT_TOP].len == (s.ext_rows == 4 ? col : 0));
  // totals: never above the old ones, and below them by exactly the dropped buffers
  const size_t items = (size_t)s.n_advice + s.n_fixed + 2 + s.n_perm + s.n_chunks + 3 * (size_t)s.n_lookup;
  const size_t dropped = (items * 72 + 256) + 256 + (((size_t)1 << 20) - (4096 + (size_t)s.n_chunks + s.n_lookup) * 32);
  const unsigned long long dev = wsl::total_bytes(L, false), pin = wsl::total_bytes(L, true);
  CHECK(dev <= c.dev0 && pin <= c.pin0);
  CHECK(c.dev0 - dev == dropped);
  CHECK(pin == c.pin0);
  // the second stage changes no size of the first: keygen allocates from a shape without gate1_cells / n_inv_slots
  wsl::Shape early = s;
  early.gate1_cells = early.n_inv_slots = 0;
  const wsl::Layout E = wsl::make(early);
  for (unsigned i = 0; i < wsl::N_BUFS; ++i)
    if (!wsl::second_stage((wsl::Buf)i)) CHECK(E.bytes[i] == L.bytes[i]);
}

}  // namespace

int main() {
  for (const Case &c : CASES) check(c);
  {
    // negative: H(X)'s coefficients pushed one column down, onto rand_l, which is live in the same step; and a region past its buffer
    const char *what = "negative cases";
    wsl::Layout L = wsl::make(shape_of(CASES[2]));
    const wsl::Region *a = nullptr, *b = nullptr;
    CHECK(wsl::consistent(L));
    L.reg[wsl::H_COEFF].off = L.reg[wsl::RAND_L].off;
    CHECK(!wsl::consistent(L, &a, &b));
    CHECK(a == &L.reg[wsl::RAND_L] && b == &L.reg[wsl::H_COEFF]);
    // the same two regions in different steps are no conflict
    L.reg[wsl::H_COEFF].live = wsl::bit(wsl::KEYGEN);
    CHECK(wsl::consistent(L));
    L = wsl::make(shape_of(CASES[2]));
    L.reg[wsl::SH_DINV].len += 2 * ((size_t)32 << 13);   // columns 30 .. 32 of 32
    CHECK(!wsl::consistent(L, &a, &b));
    CHECK(a == &L.reg[wsl::SH_DINV] && b == nullptr);
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
