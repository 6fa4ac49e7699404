// The host G2 arithmetic and the pairing check (host_g2.cpp, on pairing.hpp): the verifier's half of an SRS, the final check
// e(F, G2) e(-W, s G2) = 1 of a proof, and the raw / canonical G2 codec that the SRS side (srs.hip) borrows.
#pragma once
#include "pairing.hpp"
#include "transcript.hpp"

// the verifier's half of an SRS: G2 and s*G2 (the library's own setups derive s from a seed; an external ceremony supplies them)
struct SrsG2 {
  zkhost::pairing::Pt<zkhost::pairing::Fq2> g2, sg2;
};
SrsG2 srs_g2_from_seed(const uint8_t *srs_seed, size_t seed_len);
// reduced coordinates, on the twist y^2 = x^3 + 3/(9+i)  (subgroup membership is the caller's responsibility, as in halo2's ParamsKZG::read)
bool g2_from_canon(const uint8_t canon[128], zkhost::pairing::Pt<zkhost::pairing::Fq2> &p);
// e(F, G2) e(-W, s G2) = 1, i.e. e(W, s G2) = e(F, G2)
bool final_check(const zkhost::AffinePoint &F, const zkhost::AffinePoint &w_commit, const SrsG2 &srs);

// G2 and s G2 as raw Montgomery coordinates x.c0 | x.c1 | y.c0 | y.c1; raw <-> canonical
void zk_srs_g2_from_secret(const zkhost::U256 &s, uint8_t g2_raw[128], uint8_t sg2_raw[128]);
bool zk_g2_raw_to_canon(const uint8_t raw[128], uint8_t canon[128]);   // false: a coordinate is not reduced or the point is off the twist
bool zk_g2_canon_to_raw(const uint8_t canon[128], uint8_t raw[128]);
// e(A, s_g2) e(-B, g2) = 1 on the host (affine Montgomery G1 points, raw G2 coordinates): the powers check of zkfhe_srs_check
bool zk_srs_pairing_powers(const zk::G1Affine &A, const zk::G1Affine &B, const uint8_t g2_raw[128], const uint8_t sg2_raw[128]);
