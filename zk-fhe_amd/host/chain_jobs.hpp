// The job list of a round's linear combinations (prover_kernels.hip.hpp k_chain_jobs / k_chain_sums): plain host code, no HIP.
// A round sums several member lists ("sets": the SHPLONK rotation sets, or H(X)'s three pieces) that lie one behind the other in one
// pointer list and one scalar list.  A set is cut into chunks of at most PER members -- the split of the prover's lincomb() --, one job
// per chunk.  A set of one chunk writes its row of the destination directly; a longer one writes one slot of the partial-sum buffer per
// chunk, and one Sum record per such set says which slots add up to its row.  The partial sums are stored canonical, so the same chunks
// give the same words as the chunked kernel followed by the row sum.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace chain {

constexpr unsigned PER = 48;   // members per job

struct Job {
  uint32_t first;   // offset of the job's first member in the round's pointer list and in its scalar list
  uint32_t m;       // members, 1 .. PER (0 only for a set without members: the row is written as zeros)
  uint32_t set;     // the row of the destination the job belongs to
  int32_t slot;     // < 0: the job writes row `set` directly; else the slot of the partial-sum buffer it writes
};
struct Sum {
  uint32_t set, slot0, chunks;   // row `set` = the sum of slots [slot0, slot0 + chunks)
  uint32_t pad;
};
struct Plan {
  std::vector<Job> jobs;
  std::vector<Sum> sums;
  std::vector<uint32_t> first;   // per set: offset of its first member in the lists
  uint32_t members = 0;          // length of the lists
  uint32_t slots = 0;            // slots of the partial-sum buffer in use
};

// sizes[j]: the members of set j, in list order
inline Plan plan(const std::vector<size_t> &sizes) {
  Plan p;
  for (size_t j = 0; j < sizes.size(); ++j) {
    const uint32_t m = (uint32_t)sizes[j], chunks = m ? (m + PER - 1) / PER : 1;
    p.first.push_back(p.members);
    if (chunks > 1) p.sums.push_back(Sum{(uint32_t)j, p.slots, chunks, 0});
    for (uint32_t c = 0; c < chunks; ++c) {
      const uint32_t lo = c * PER, hi = lo + PER < m ? lo + PER : m;
      p.jobs.push_back(Job{p.members + lo, hi - lo, (uint32_t)j, chunks > 1 ? (int32_t)p.slots++ : -1});
    }
    p.members += m;
  }
  return p;
}

}  // namespace chain
