// fr29_from_mont_weak (csrc/fr29.hip.hpp), the conversion the table MSM takes a scalar through, against the 8 x 32-bit fp_from_mont:
// host instantiation of the host+device code (the C body of the nine-limb reduction; on the device the tied form computes the same
// integers, tests/test_gpu_msm_scalar_prep.py).  Equal for every input below 2^256, except that a non-zero multiple of r gives r.
#include <cstdio>
#include <cstring>
#include "fr29.hip.hpp"
using namespace zk;

static u32 rng_state = 0x9e3779b9u;
static u32 rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
  return rng_state;
}

// x mod r for x < 2^256 (r > 2^253: at most five subtractions)
static Fr canonical(Fr x) {
  for (int k = 0; k < 6; ++k) {
    u32 t[8], br = 0;
    for (int i = 0; i < 8; ++i) t[i] = zk_subc(x.l[i], FrP::MOD[i], br, &br);
    if (!br)
      for (int i = 0; i < 8; ++i) x.l[i] = t[i];
  }
  return x;
}

int main() {
  int bad = 0, gave_r = 0;
  auto check = [&](const Fr &x) {
    const Fr a = fr29_from_mont_weak(x), b = fp_from_mont<FrP>(canonical(x));
    const bool is_r = !memcmp(a.l, FrP::MOD, 32);
    if (is_r) ++gave_r;
    if (is_r ? !(b.is_zero() && !x.is_zero()) : memcmp(a.l, b.l, 32) != 0) ++bad;
  };
  Fr x;
  for (int k = 0; k <= 5; ++k) {   // 0, r, 2 r, .. 5 r (the multiples of r below 2^256) and their neighbours
    u32 m[8] = {0}, c = 0;
    for (int j = 0; j < k; ++j) {
      c = 0;
      for (int i = 0; i < 8; ++i) m[i] = zk_addc(m[i], FrP::MOD[i], c, &c);
    }
    for (int d = -1; d <= 1; ++d) {
      if (k == 0 && d < 0) continue;
      for (int i = 0; i < 8; ++i) x.l[i] = m[i];
      if (d > 0) x.l[0] += 1;   // r is odd and its low limb is 1: no carry
      if (d < 0) x.l[0] -= 1;
      check(x);
    }
  }
  memset(x.l, 0xff, 32);
  check(x);
  for (int it = 0; it < 200000; ++it) {
    for (int i = 0; i < 8; ++i) x.l[i] = rnd();
    if (it % 3 == 0) x.l[7] &= 0x0fffffffu;
    if (it % 5 == 0) x.l[it % 8] = it & 1 ? 0xffffffffu : 0u;
    check(x);
  }
  printf("fr29_from_mont_weak: %d bad, r for %d inputs\n", bad, gave_r);
  return bad != 0 || gave_r != 5;
}
