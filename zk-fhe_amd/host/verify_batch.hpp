// Batch verification (verify_batch.cpp): many proofs under one vk, their points decompressed and their SHPLONK combinations
// summed on the GPU, one pairing check for all.
#pragma once
#include <string>

#include "host_g2.hpp"
#include "opening.hpp"

namespace zkhost {

struct BatchItem {
  std::vector<U256> inst;
  const uint8_t *proof = nullptr;
  size_t len = 0;
  bool live = true;    // not rejected yet
  std::string why;
  zk::Fr r;            // randomiser (Montgomery)
  int group = -1;      // shared public-key prefix
  size_t words = 0, base = 0;
  Opening op;
  AffinePoint F, W;
};

// Verdict (live) and reason (why) of every item; items that arrive dead keep their reason.  Returns a ZKFHE_* code.
int verify_batch(zkfhe_ctx *ctx, const Vk &vk, const SrsG2 &srs, std::vector<BatchItem> &items);

}  // namespace zkhost
