// Small host helpers shared by the prover units (prover_internal.hpp) and the verifier units: Fr values in and out of
// Montgomery form, Fr power and inverse, G1 points between canonical and Montgomery coordinates.  Host C++ only.
#pragma once
#include "transcript.hpp"

namespace zkhost {

static inline zk::Fr mont(const U256 &v) { return fe::to_mont(v); }
static inline zk::Fr mont_u64(uint64_t v) { return fe::to_mont(fe::from_u64(v)); }
static inline U256 canon(const zk::Fr &f) { return fe::from_mont(f); }
static inline zk::Fr fr_pow(zk::Fr b, uint64_t e) {
  zk::Fr r = zk::Fr::one();
  while (e) {
    if (e & 1) r = r * b;
    b = b * b;
    e >>= 1;
  }
  return r;
}
static inline zk::Fr fr_inv(const zk::Fr &a) { return zk::fp_inv<zk::FrP>(a); }

// affine Montgomery <-> canonical coordinates; the identity is (0, 0) in both
static inline AffinePoint point_canon(const zk::G1Affine &p) {
  AffinePoint a;
  zk::Fq x = zk::fp_from_mont<zk::FqP>(p.x), y = zk::fp_from_mont<zk::FqP>(p.y);
  memcpy(a.x.l, x.l, 32);
  memcpy(a.y.l, y.l, 32);
  return a;
}
static inline zk::G1Affine point_mont(const AffinePoint &p) {
  zk::G1Affine a;
  memcpy(a.x.l, p.x.l, 32);
  memcpy(a.y.l, p.y.l, 32);
  a.x = zk::fp_to_mont<zk::FqP>(a.x);
  a.y = zk::fp_to_mont<zk::FqP>(a.y);
  return a;
}
// delta of the permutation argument (canonical): halo2's Fr::DELTA, a generator of the order-(r-1)/2^28 subgroup
static const uint64_t DELTA_CANON[4] = {0x870e56bbe533e9a2ULL, 0x5b5f898e5e963f25ULL, 0x64ec26aad4c86e71ULL, 0x09226b6e22c6f0caULL};
// the generator (1, 2)
static inline AffinePoint g1_generator() { return AffinePoint{fe::from_u64(1), fe::from_u64(2)}; }

}  // namespace zkhost
