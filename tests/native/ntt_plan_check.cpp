// CPU check of csrc/ntt_plan.hpp: for every long-row call (log_n 14 .. 26, both directions, in place and out of place, no coset /
// a device table of coset powers / host shifts, 1 .. 8 rows, ZKFHE_NTT_LDS_PASS on and off) the list of passes equals the literal
// table below -- written out from the loop of the dispatcher this header replaced, by number of stages above the 2^13 tile -- and
// the buffer routing keeps the properties the kernels rely on.  Built and run by tests/test_ntt_plan_host.py (with the address and
// undefined-behaviour sanitizers).
//
//   ntt_plan_check --passes    prints no verdict but the plans themselves, one line per pass, for log_n 14 .. 26 x {no coset, a table
//                              (eight rows), shifts (four rows)} x LDS passes {on, off} x {out of place, in place}, forward:
//                                log_n=19 coset=table lds=1 in_place=0 pass=0 kind=lds S=6 first=1 carries_coset=1 in=src out=work
//                              A refused combination prints nothing.  tests/test_ntt_schedules_host.py holds these lines against the
//                              shapes that the GPU tests run (tests/ntt_schedules.py).
#include <cstdio>
#include <cstring>
#include <string>

#include "ntt_plan.hpp"

using namespace zk;

static int failures = 0;
static char cur[128] = "";
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      ++failures;                                                       \
      printf("case %s: %s fails (line %d)\n", cur, #cond, __LINE__);    \
    }                                                                   \
  } while (0)

// stages per pass, by stages above the tile (index 1 .. 13); L: the LDS pass, F: the four-step pass
static const char *const RADIX2_LDS_ON[14] = {nullptr, "1", "2", "3", "4L", "5L", "6L", "4L 3", "6L 2", "6L 3", "6L 4L", "6L 5L", "6L 6L", "6L 4L 3"};
static const char *const RADIX2_LDS_OFF[14] = {nullptr, "1", "2", "3", "3 1", "3 2", "3 3", "3 3 1", "3 3 2", "3 3 3", "3 3 3 1", "3 3 3 2", "3 3 3 3", "3 3 3 3 1"};

static std::string spelled(const NttPlan &p) {
  std::string s;
  for (int i = 0; i < p.n_passes; ++i) {
    if (i) s += ' ';
    s += std::to_string(p.pass[i].S);
    if (p.pass[i].kind == NTT_LDS) s += 'L';
    if (p.pass[i].kind == NTT_FOUR_STEP) s += 'F';
  }
  return s;
}

static void check(int log_n, bool inverse, bool in_place, NttCoset coset, unsigned rows, bool lds) {
  snprintf(cur, sizeof cur, "log_n=%d inverse=%d in_place=%d coset=%d rows=%u lds=%d", log_n, inverse, in_place, (int)coset, rows, lds);
  const int above = log_n - 13;
  const bool four_step_size = log_n == 16 || log_n == 19;
  const NttPlan p = ntt_plan(log_n, inverse, in_place, coset, rows, lds);

  // what is refused: coset multipliers on anything but a forward out-of-place call, and shifts that no four-step pass can take
  const bool legal = coset == NTT_COSET_NONE || (!inverse && !in_place && (coset == NTT_COSET_PRE || (four_step_size && rows <= 4)));
  CHECK(p.refused == !legal);
  if (p.refused || !legal) return;

  // the stage list
  std::string want = lds ? RADIX2_LDS_ON[above] : RADIX2_LDS_OFF[above];
  if (four_step_size && coset != NTT_COSET_PRE) want = above == 3 ? "3F" : "6F";
  if (spelled(p) != want) {
    ++failures;
    printf("case %s: passes [%s], expected [%s]\n", cur, spelled(p).c_str(), want.c_str());
  }
  CHECK(p.n_passes >= 1 && p.n_passes <= NTT_MAX_PASSES);

  int sum = 0, top = log_n - 1;
  NttBuf holds = in_place ? NTT_DST : NTT_SRC;   // where the rows are before the next pass
  for (int i = 0; i < p.n_passes && i < NTT_MAX_PASSES; ++i) {
    const NttPass &ps = p.pass[i];
    CHECK(ps.log_half == top);   // every pass continues where the one before stopped
    CHECK(ps.coset == (i == 0 && coset != NTT_COSET_NONE));
    CHECK(ps.in == holds && ps.out != NTT_SRC);
    CHECK((int)ps.out >= 0 && (int)ps.out <= 2 && (int)ps.in >= 0 && (int)ps.in <= 2);
    switch (ps.kind) {
      case NTT_FOUR_STEP:
        CHECK(four_step_size && ps.S == above && p.n_passes == 1 && coset != NTT_COSET_PRE);
        CHECK(coset == NTT_COSET_NONE || rows <= 4);
        break;
      case NTT_LDS:
        CHECK(lds && ps.S >= 4 && ps.S <= 6 && ps.log_half >= 9);   // JJ = 1024 >> S consecutive offsets exist
        break;
      case NTT_FUSED:
        CHECK(ps.S == 2 || ps.S == 3);
        break;
      case NTT_STAGE:
        CHECK(ps.S == 1);
        break;
      default:
        CHECK(!"a known kind");
    }
    if (coset == NTT_COSET_SHIFTS) CHECK(ps.kind == NTT_FOUR_STEP);
    sum += ps.S;
    top -= ps.S;
    holds = ps.out;
  }
  CHECK(sum == above && top == 12);

  // the tile stage and the copy back
  CHECK(p.tile_in == holds && p.tile_in != p.tile_out && p.tile_out != NTT_SRC);
  CHECK(p.copy_back == in_place);
  if (in_place) {
    CHECK(p.tile_out == NTT_WORK);   // what the copy brings back
    for (int i = 0; i < p.n_passes; ++i) CHECK(p.pass[i].in != NTT_SRC);   // there is no source
  } else {
    CHECK(p.tile_out == NTT_DST);
  }
}

static int print_passes() {
  static const char *const COSET[] = {"none", "table", "shifts"}, *const KIND[] = {"four_step", "lds", "fused", "stage"}, *const BUF[] = {"src", "dst", "work"};
  for (int log_n = 14; log_n <= 26; ++log_n)
    for (int coset = 0; coset < 3; ++coset)
      for (int lds = 1; lds >= 0; --lds)
        for (int in_place = 0; in_place < 2; ++in_place) {
          const NttPlan p = ntt_plan(log_n, false, in_place, (NttCoset)coset, coset == NTT_COSET_PRE ? 8 : coset == NTT_COSET_SHIFTS ? 4 : 1, lds);
          if (p.refused) continue;
          for (int i = 0; i < p.n_passes; ++i) {
            const NttPass &ps = p.pass[i];
            printf("log_n=%d coset=%s lds=%d in_place=%d pass=%d kind=%s S=%d first=%d carries_coset=%d in=%s out=%s\n", log_n, COSET[coset], lds, in_place, i,
                   KIND[ps.kind], ps.S, i == 0, (int)ps.coset, BUF[ps.in], BUF[ps.out]);
          }
        }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "--passes")) return print_passes();
  for (int log_n = 14; log_n <= 26; ++log_n)
    for (int inverse = 0; inverse < 2; ++inverse)
      for (int in_place = 0; in_place < 2; ++in_place)
        for (int lds = 0; lds < 2; ++lds) {
          check(log_n, inverse, in_place, NTT_COSET_NONE, 1, lds);
          for (unsigned rows = 1; rows <= 8; ++rows) {
            check(log_n, inverse, in_place, NTT_COSET_PRE, rows, lds);
            check(log_n, inverse, in_place, NTT_COSET_SHIFTS, rows, lds);
          }
        }
  {   // outside the long rows there is no plan
    strcpy(cur, "range");
    CHECK(ntt_plan(13, false, false, NTT_COSET_NONE, 1, true).refused);
    CHECK(ntt_plan(27, false, false, NTT_COSET_NONE, 1, true).refused);
    CHECK(ntt_plan(15, false, false, NTT_COSET_PRE, 0, true).refused);
  }
  {   // the knob
    strcpy(cur, "knob");
    CHECK(ntt_lds_pass_enabled(nullptr) && ntt_lds_pass_enabled("") && ntt_lds_pass_enabled("1") && ntt_lds_pass_enabled("yes"));
    CHECK(!ntt_lds_pass_enabled("0") && !ntt_lds_pass_enabled("00") && !ntt_lds_pass_enabled("0x"));
    CHECK(ntt_four_step_size(16) && ntt_four_step_size(19) && !ntt_four_step_size(13) && !ntt_four_step_size(17) && !ntt_four_step_size(22));
  }
  if (failures) {
    printf("ntt plan check: %d failure(s)\n", failures);
    return 1;
  }
  printf("ntt plan check: ok\n");
  return 0;
}
