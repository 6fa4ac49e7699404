// The schedule of one G1 FFT call (g1_fft.hip): the stage list, which two elements a butterfly touches, which entry of the domain's
// twiddle table it reads, and the bit reversal of the load.  Plain C++ with no HIP in it; the index functions are constexpr, so the
// kernels call the very functions that tests/native/g1_fft_plan_check.cpp walks on the CPU against the naive double sum.
//
// Radix-2 decimation in time: the load writes element i of the input to slot bitrev(i); stage s (half = 2^s) combines the slots
// lo and hi = lo + half of every block of 2 half slots as (a, b) -> (a + w b, a - w b) with w = omega^(j * n / (2 half)), j the
// offset of lo in its block; after the last stage the slots hold the transform in natural order.  An inverse call reads the table
// of omega^-1 and carries its n^-1 in the LAST stage: (a, b) -> (n^-1 a + (n^-1 w) b, n^-1 a - (n^-1 w) b) -- the same group
// elements as a scaling pass over the result, for n / 2 further scalar multiplications instead of n.
#pragma once
#include <cstddef>

namespace zk {

constexpr int G1FFT_MAX_LOG = 20;
constexpr int G1FFT_WAVE = 64;   // lanes that run one scalar multiplication in lockstep

// How the butterflies of a stage are dealt to threads.  Thread t of n / 2:
//   G1FFT_SHARED: t = j * blocks + block.  A stage with at least `wave` blocks (a power of two) puts `wave` consecutive threads on
//                 the same j, i.e. the same twiddle: the ladder over its digits branches the same way in every lane, and the
//                 kernel holds the scalar in scalar registers.
//   G1FFT_WINDOW: t = block * half + j.  Fewer blocks than lanes: every lane has a twiddle of its own; the ladder's fixed window
//                 (the same doublings and one table addition per digit, whatever the digit) keeps the lanes in step.
enum G1FftKind { G1FFT_SHARED = 0, G1FFT_WINDOW = 1 };

struct G1FftStage {
  G1FftKind kind;
  int log_half;
  bool scale;   // the last stage of an inverse call: a and the twiddle are multiplied by n^-1
};

struct G1FftPlan {
  bool refused;   // log_n outside 1..G1FFT_MAX_LOG, or `wave` no power of two; nothing else is filled in
  int log_n;
  int n_stages;
  G1FftStage stage[G1FFT_MAX_LOG];
};

// `wave`: the launcher passes G1FFT_WAVE; the CPU check also passes 1, 2 and 4 to walk the shared-twiddle structure at sizes a naive
// reference can follow.
inline G1FftPlan g1_fft_plan(int log_n, bool inverse, int wave = G1FFT_WAVE) {
  G1FftPlan p{};
  if (log_n < 1 || log_n > G1FFT_MAX_LOG || wave < 1 || (wave & (wave - 1)) != 0) {
    p.refused = true;
    return p;
  }
  p.log_n = log_n;
  p.n_stages = log_n;
  for (int s = 0; s < log_n; ++s) {
    const size_t blocks = (size_t)1 << (log_n - 1 - s);
    p.stage[s] = {blocks >= (size_t)wave ? G1FFT_SHARED : G1FFT_WINDOW, s, inverse && s == log_n - 1};
  }
  return p;
}

// the smallest size at which a call launches more than one butterfly structure (every smaller one runs G1FFT_WINDOW stages only)
constexpr int G1FFT_FIRST_SHARED_LOG = 7;
static_assert(((size_t)1 << (G1FFT_FIRST_SHARED_LOG - 1)) == (size_t)G1FFT_WAVE, "the first stage of that size has exactly G1FFT_WAVE blocks");

constexpr size_t g1_fft_bitrev(size_t i, int log_n) {
  size_t r = 0;
  for (int b = 0; b < log_n; ++b) r |= ((i >> b) & 1) << (log_n - 1 - b);
  return r;
}

struct G1FftButterfly {
  size_t lo, hi;   // slots
  size_t tw;       // index into the domain's table of omega^j (forward) or omega^-j (inverse), j < n
};

constexpr G1FftButterfly g1_fft_butterfly(int kind, int log_n, int log_half, size_t t) {
  const int log_blocks = log_n - 1 - log_half;
  const size_t half = (size_t)1 << log_half;
  const size_t j = kind == G1FFT_SHARED ? t >> log_blocks : t & (half - 1);
  const size_t block = kind == G1FFT_SHARED ? t & (((size_t)1 << log_blocks) - 1) : t >> log_half;
  const size_t lo = (block << (log_half + 1)) + j;
  return {lo, lo + half, j << log_blocks};
}

}  // namespace zk
