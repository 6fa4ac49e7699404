// The job list of zk-fhe_amd/host/chain_jobs.hpp on the host alone: for member counts around the chunk size of 48 and for 1, 6 and 8
// sets, every member lies in exactly one job, no job holds more than 48, a set's row is written by exactly one writer (its one job,
// or its sum), partial slots are used once and do not overlap, and the slots fit the prover's partial-sum buffer at k = 13.
// Built plain and with -fsanitize=address,undefined by tests/test_chain_jobs_host.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chain_jobs.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("line %d: %s fails (%s)\n", __LINE__, #cond, what); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// keygen.hip sizes ws->partials for at least 96 columns of n rows: the slots of one round must fit that at every k
constexpr unsigned PARTIAL_COLUMNS_MIN = 96;

void check(const std::vector<size_t> &sizes, const char *what) {
  const chain::Plan p = chain::plan(sizes);
  size_t members = 0;
  for (size_t m : sizes) members += m;
  CHECK(p.members == members);
  CHECK(p.first.size() == sizes.size());
  std::vector<int> seen(members, 0), slot_used(p.slots, 0), direct(sizes.size(), 0), summed(sizes.size(), 0), set_members(sizes.size(), 0);
  for (const chain::Job &j : p.jobs) {
    CHECK(j.m >= 1 && j.m <= chain::PER);
    CHECK(j.set < sizes.size());
    CHECK((size_t)j.first + j.m <= members);
    if (j.set >= sizes.size() || (size_t)j.first + j.m > members) continue;
    CHECK(j.first >= p.first[j.set] && j.first + j.m <= p.first[j.set] + sizes[j.set]);   // a job stays inside its set
    for (unsigned k = 0; k < j.m; ++k) ++seen[j.first + k];
    set_members[j.set] += (int)j.m;
    if (j.slot < 0) {
      ++direct[j.set];
    } else {
      CHECK((unsigned)j.slot < p.slots);
      if ((unsigned)j.slot < p.slots) ++slot_used[j.slot];
    }
  }
  for (size_t k = 0; k < members; ++k) CHECK(seen[k] == 1);
  for (unsigned s = 0; s < p.slots; ++s) CHECK(slot_used[s] == 1);
  std::vector<int> slot_summed(p.slots, 0);
  for (const chain::Sum &s : p.sums) {
    CHECK(s.set < sizes.size());
    CHECK(s.chunks >= 2 && s.slot0 + s.chunks <= p.slots);
    if (s.set >= sizes.size() || s.slot0 + s.chunks > p.slots) continue;
    ++summed[s.set];
    CHECK(s.chunks == (sizes[s.set] + chain::PER - 1) / chain::PER);
    for (unsigned c = 0; c < s.chunks; ++c) ++slot_summed[s.slot0 + c];
    // the slots of a sum are written by this set's jobs, in member order
    for (const chain::Job &j : p.jobs)
      if (j.slot >= (int)s.slot0 && j.slot < (int)(s.slot0 + s.chunks)) {
        CHECK(j.set == s.set);
        CHECK(j.first == p.first[s.set] + (unsigned)(j.slot - (int)s.slot0) * chain::PER);
      }
  }
  for (unsigned s = 0; s < p.slots; ++s) CHECK(slot_summed[s] == 1);
  for (size_t j = 0; j < sizes.size(); ++j) {
    CHECK(direct[j] + summed[j] == 1);   // one writer per destination row
    CHECK(direct[j] == (sizes[j] <= chain::PER ? 1 : 0));
    CHECK((size_t)set_members[j] == sizes[j]);
  }
  CHECK(p.slots <= PARTIAL_COLUMNS_MIN);
}

}  // namespace

int main() {
  const size_t counts[] = {1, 47, 48, 49, 96, 97};
  char what[128];
  for (size_t ns : {(size_t)1, (size_t)6, (size_t)8}) {
    for (size_t c = 0; c < 6; ++c) {   // every set of the same size
      snprintf(what, sizeof what, "%zu sets of %zu", ns, counts[c]);
      check(std::vector<size_t>(ns, counts[c]), what);
    }
    for (size_t rot = 0; rot < 6; ++rot) {   // the sizes mixed, every size in every position
      std::vector<size_t> sizes(ns);
      for (size_t j = 0; j < ns; ++j) sizes[j] = counts[(j + rot) % 6];
      snprintf(what, sizeof what, "%zu sets, sizes rotated by %zu", ns, rot);
      check(sizes, what);
    }
  }
  // the widest round the prover accepts: 8 sets; members as at k = 13 (some 600 in the widest set)
  check({640, 97, 49, 48, 1, 1, 300, 47}, "a k = 13 sized round");
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
