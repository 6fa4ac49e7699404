// The proof's word count by the one opening layout (zk-fhe_amd/host/shplonk.hpp proof_words, OpenLayout) on the host alone, for the
// toy circuit (k = 9), the pinned k = 13 configuration of tests/golden/bfv/bfv_config.json and the widest shape the vk parser admits
// (4096 columns of every kind): proof_words equals the closed formula the batch verifier counted its reads by before the count moved
// to the layout (the independent statement, kept here), and the layout's evaluation words are the rotation counts of every item but H.
// With six arguments (k n_gate0 n_gate1 n_lookup n_rlc unusable_rows) it also prints "proof_words N" for that configuration.
// Built plain and with -fsanitize=address,undefined by tests/test_verifier_layout_host.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>

#include "shplonk.hpp"

using namespace zkhost;

namespace {

int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("line %d: %s fails (%s)\n", __LINE__, #cond, what); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// the reads of the opening, in count, as the batch verifier used to spell them
size_t closed_formula(const CircuitConfig &cfg) {
  size_t w = cfg.n_advice() + 3 * cfg.n_lookup + cfg.n_chunks() + 1 + 3 + 2;   // commitments, random, h pieces, h1, h2
  for (unsigned c = 0; c < cfg.n_advice(); ++c) w += c < cfg.n_gate() ? 4 : (c < cfg.adv_rlc0() ? 1 : 3);
  w += cfg.n_fixed() + 1 + cfg.n_perm() + 3 * (cfg.n_chunks() - 1) + 2 + 5 * cfg.n_lookup;   // fixed, random, sigma, z, lookups
  return w;
}

CircuitConfig config(unsigned k, unsigned g0, unsigned g1, unsigned lk, unsigned rlc, unsigned unusable) {
  CircuitConfig c;
  c.k = k, c.n_gate0 = g0, c.n_gate1 = g1, c.n_lookup = lk, c.n_rlc = rlc, c.unusable_rows = unusable;
  return c;
}

void check(const char *what, const CircuitConfig &cfg) {
  const OpenLayout L(cfg);
  size_t sum = 0;
  for (size_t i = 0; i < L.count; ++i)
    if (i != L.H) sum += L.rots[i].size();
  CHECK(L.eval_words() == sum);
  CHECK(proof_words(cfg) == closed_formula(cfg));
  CHECK(proof_words(cfg) == commit_words(cfg) + sum + 2);
  CHECK(L.rots[L.H].size() == 1 && L.count == cfg.n_advice() + cfg.n_fixed() + 2 + cfg.n_perm() + cfg.n_chunks() + 3 * (size_t)cfg.n_lookup);
}

}  // namespace

int main(int argc, char **argv) {
  check("toy", config(9, 1, 20, 5, 1, 9));
  check("k13", config(13, 3, 153, 36, 5, 109));
  check("widest", config(28, 4096, 4096, 4096, 4096, 109));
  if (argc == 7) {
    const CircuitConfig c = config(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    check("command line", c);
    printf("proof_words %zu\n", proof_words(c));
  }
  printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
