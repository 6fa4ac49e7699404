// Part (a) of verification (opening.cpp): what one proof leaves for the final pairing check.
#pragma once
#include <vector>

#include "proof_reader.hpp"
#include "vk.hpp"

namespace zkhost {

// F = sum scal[i] * pts[i] (the SHPLONK combination) and W (= h2), to be checked as e(F, G2) e(-W, s G2) = 1
struct Opening {
  std::vector<zk::Fr> scal;
  std::vector<Pt> pts;
  Pt w;
};

// Transcript replay, instance evaluation, the expression fold and the SHPLONK scalars.  Throws the rejection reason of a
// malformed proof.  prefix (may be NULL): the transcript state after the vk digest and the first prefix_len instances (shared
// by the proofs of one public key in a batch); dec (may be NULL): pre-decoded points.
Opening open_proof(const Vk &vk, const std::vector<U256> &inst, const uint8_t *proof, size_t proof_len, const Transcript::State *prefix = nullptr,
                   size_t prefix_len = 0, const Decoded *dec = nullptr);

}  // namespace zkhost
