// The plan of one long-row NTT call (ntt.hip, rows of 2^14 .. 2^26 points): which passes run the stages above the 2^13 tile, which
// buffer each of them reads and writes, where the tile stage reads and writes, and whether a copy back follows.  Plain host C++
// with no HIP in it: tests/native/ntt_plan_check.cpp checks every plan on the CPU, before any kernel is launched from one.
#pragma once

namespace zk {

constexpr int NTT_TILE_LOG = 13;     // the largest tile: a longer row is cut into 2^13 blocks by the passes planned here
constexpr int NTT_MAX_PASSES = 5;    // 13 stages above the tile in register passes of three

// ZKFHE_NTT_LDS_PASS: "0..." turns the LDS passes off (four or more stages then run as register passes of three); anything else,
// or unset, leaves them on.
inline bool ntt_lds_pass_enabled(const char *env) { return !(env && env[0] == '0'); }

// Rows of 2^16 and 2^19 (three / six stages above the tile) run those stages as ONE four-step pass (ntt_dif8.hip): constants for
// the size-8 / size-64 part, one streaming table product per element.  Every other length takes radix-2 passes with gathered
// twiddles.
inline bool ntt_four_step_size(int log_n) { return log_n - NTT_TILE_LOG == 3 || log_n - NTT_TILE_LOG == 6; }

enum NttPassKind {
  NTT_FOUR_STEP,   // zk_dif8_pass: all 3 or 6 stages
  NTT_LDS,         // k_dif_lds<S - 3>: 4 to 6 stages, one exchange through LDS
  NTT_FUSED,       // k_dif_fused<S>: 2 or 3 stages in registers
  NTT_STAGE        // k_dif_stage: one stage
};
// the coset multipliers of a forward extension: none, a device table of powers that the first radix-2 pass applies as it loads
// (`pre`), or the shifts on the host, which only the four-step pass can fold into its own tables
enum NttCoset { NTT_COSET_NONE, NTT_COSET_PRE, NTT_COSET_SHIFTS };
enum NttBuf { NTT_SRC, NTT_DST, NTT_WORK /* scratch slot 0 */ };

struct NttPass {
  NttPassKind kind;
  int S;          // stages: halves 2^log_half, 2^(log_half - 1), ..., 2^(log_half - S + 1)
  int log_half;
  bool coset;     // applies the coset multipliers (the first pass only: the later ones read scaled data)
  NttBuf in, out;
};

struct NttPlan {
  bool refused;   // the combination of arguments has no schedule; nothing else is filled in
  int n_passes;
  NttPass pass[NTT_MAX_PASSES];
  NttBuf tile_in, tile_out;   // never the same buffer: the 2^13 tile cannot run in place
  bool copy_back;             // scratch slot 0 -> destination, after the tiles
};

// Out of place, the first pass reads the source and writes scratch slot 0, the later passes run in place there and the tiles scatter
// into the destination: no copy anywhere.  In place, the passes run on the data, the tiles write slot 0 and one copy brings it back.
// Refused: coset multipliers on anything but a forward out-of-place call; host shifts where no four-step pass takes them (another
// size, or more than four rows: its table slots).
inline NttPlan ntt_plan(int log_n, bool inverse, bool in_place, NttCoset coset, unsigned rows, bool lds_pass) {
  NttPlan p{};
  const bool four_step = ntt_four_step_size(log_n) && coset != NTT_COSET_PRE;
  if (log_n <= NTT_TILE_LOG || log_n > 26 || (coset != NTT_COSET_NONE && (inverse || in_place || rows < 1)) ||
      (coset == NTT_COSET_SHIFTS && !(four_step && rows <= 4))) {
    p.refused = true;
    return p;
  }
  const NttBuf work = in_place ? NTT_DST : NTT_WORK;
  NttBuf from = in_place ? NTT_DST : NTT_SRC;
  auto add = [&](NttPassKind kind, int S, int log_half) {
    p.pass[p.n_passes] = {kind, S, log_half, p.n_passes == 0 && coset != NTT_COSET_NONE, from, work};
    ++p.n_passes;
    from = work;
  };
  int left = log_n - NTT_TILE_LOG;   // stages still above the tile; the next pass starts at half 2^(NTT_TILE_LOG + left - 1)
  if (four_step) {
    add(NTT_FOUR_STEP, left, log_n - 1);
    left = 0;
  }
  while (left > 0) {
    int S;
    NttPassKind kind;
    if (left >= 4 && lds_pass) {   // four to six stages in one pass through LDS (seven: four, then three in registers)
      S = left == 7 ? 4 : (left > 6 ? 6 : left);
      kind = NTT_LDS;
    } else {                       // up to three stages per pass over memory, in registers
      S = left >= 3 ? 3 : left;
      kind = S == 1 ? NTT_STAGE : NTT_FUSED;
    }
    add(kind, S, NTT_TILE_LOG + left - 1);
    left -= S;
  }
  p.tile_in = work;
  p.tile_out = in_place ? NTT_WORK : NTT_DST;
  p.copy_back = in_place;
  return p;
}

}  // namespace zk
