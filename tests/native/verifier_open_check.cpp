// The verifier's reader and opening (zk-fhe_amd/host/proof_reader.hpp, opening.cpp) on hostile bytes, on the host alone, linked with
// host_g2.cpp and the Poseidon cores.  Arguments: a vk file, the instances (32 bytes each), an accepted proof, the length of the
// public-key prefix of the instances.
//   1. the proof is accepted: its opening, summed, passes the pairing check;
//   2. every prefix of the proof at a word boundary is rejected as "proof truncated" and one extra word as "trailing bytes in proof";
//      each is opened from a heap copy of exactly its length, so a read past the end is the address sanitizer's to report;
//   3. opening from the transcript state after digest | prefix gives the same points, scalars and W as opening from the start;
//   4. opening from pre-decoded points (Decoded, filled by decode_point over every word) gives the same opening, and three bad words
//      in commitment 1 -- x >= q, an x with no root, the identity with a stray byte -- are refused with the same text on both paths.
// Built plain and with -fsanitize=address,undefined by tests/test_verifier_open_host.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "host_g2.hpp"
#include "opening.hpp"
#include "shplonk.hpp"

using namespace zkhost;
using zk::Fr;

// csrc/core.hip's, which the opening takes from the library: 7^((r-1)/2^28), squared down to the 2^log_n-th root
Fr zk_fr_root_of_unity(int log_n) {
  Fr c;
  const uint32_t w[8] = {0x60c37c9cu, 0xd34f1ed9u, 0xd39329c8u, 0x3215cf6du, 0x3dd31f74u, 0x98865ea9u, 0x166d18b7u, 0x03ddb9f5u};
  for (int i = 0; i < 8; ++i) c.l[i] = w[i];
  Fr r = zk::fp_to_mont<zk::FrP>(c);
  for (int i = 0; i < 28 - log_n; ++i) r = r * r;
  return r;
}

namespace {

int failures = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      printf("line %d: %s fails\n", __LINE__, #cond);      \
      ++failures;                                           \
    }                                                       \
  } while (0)

typedef std::vector<uint8_t> Bytes;
Bytes slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// a vk file the suite made itself: magic | 8 x u32 config | 2 x u32 counts | digest | fixed, sigma commitments (verifier.cpp parse_vk)
Vk read_vk(const Bytes &b) {
  uint32_t h[10];
  memcpy(h, b.data() + 8, 40);
  Vk vk;
  vk.cfg.k = h[0], vk.cfg.n_gate0 = h[1], vk.cfg.n_gate1 = h[2], vk.cfg.n_lookup = h[3], vk.cfg.n_rlc = h[4];
  vk.cfg.unusable_rows = h[5], vk.cfg.lookup_bits = h[6], vk.cfg.transcript = h[7];
  memcpy(vk.digest.l, b.data() + 48, 32);
  const uint8_t *p = b.data() + 80;
  for (auto *v : {&vk.fixed_commit, &vk.sigma_commit}) {
    v->resize(v == &vk.fixed_commit ? h[8] : h[9]);
    for (AffinePoint &a : *v) {
      memcpy(a.x.l, p, 32);
      memcpy(a.y.l, p + 32, 32);
      p += 64;
    }
  }
  CHECK(b.size() == 80 + 64 * ((size_t)h[8] + h[9]) && vk_digest(vk.cfg, vk.fixed_commit, vk.sigma_commit) == vk.digest);
  return vk;
}

// F = sum scal[i] * pts[i] by one double-and-add per term, then the pairing check against the suite's seeded SRS
bool accepted(const Opening &op) {
  zk::G1X total = zk::G1X::identity();
  for (size_t i = 0; i < op.pts.size(); ++i) {
    if (op.pts[i].p.is_identity()) continue;
    const U256 k = canon(op.scal[i]);
    const zk::G1Affine base = point_mont(op.pts[i].p);
    zk::G1X acc = zk::G1X::identity();
    for (int bit = 253; bit >= 0; --bit) {
      acc = zk::g1x_dbl(acc);
      if ((k.l[bit >> 6] >> (bit & 63)) & 1) zk::g1x_add_affine(acc, base, false);
    }
    zk::g1x_add(total, acc);
  }
  const char seed[] = "zkfhe-unsafe-srs";
  return final_check(point_canon(zk::g1x_to_affine(total)), op.w.p, srs_g2_from_seed((const uint8_t *)seed, sizeof(seed) - 1));
}

bool same(const Pt &a, const Pt &b) { return a.p.x == b.p.x && a.p.y == b.p.y && a.ref == b.ref; }
bool same(const Opening &a, const Opening &b) {
  bool ok = a.scal.size() == b.scal.size() && a.pts.size() == b.pts.size() && a.pts.size() == a.scal.size() && same(a.w, b.w);
  for (size_t i = 0; ok && i < a.pts.size(); ++i) ok = a.scal[i] == b.scal[i] && same(a.pts[i], b.pts[i]);
  return ok;
}

// every word of `proof` as decode_point sees it: what the batch verifier gets from the device
struct HostDecoded {
  std::vector<zk::G1Affine> pt;
  std::vector<int32_t> st;
  Decoded dec;
  explicit HostDecoded(const Bytes &proof) : pt(proof.size() / 32), st(proof.size() / 32) {
    for (size_t w = 0; w < st.size(); ++w) {
      AffinePoint a;
      st[w] = decode_point(proof.data() + 32 * w, a);
      pt[w] = point_mont(a);
    }
    dec = Decoded{pt.data(), st.data(), st.size()};
  }
};

template <class F>
std::string reason(const F &f) {
  try {
    f();
    return "";
  } catch (const std::exception &e) {
    return e.what();
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const Vk vk = read_vk(slurp(argv[1]));
  const Bytes ib = slurp(argv[2]), proof = slurp(argv[3]);
  const size_t prefix_len = (size_t)atoi(argv[4]), words = proof.size() / 32;
  std::vector<U256> inst(ib.size() / 32);
  memcpy(inst.data(), ib.data(), inst.size() * 32);
  CHECK(proof.size() % 32 == 0 && words == proof_words(vk.cfg) && prefix_len <= inst.size());
  // 1
  const Opening whole = open_proof(vk, inst, proof.data(), proof.size());
  CHECK(accepted(whole));
  // 2
  for (size_t w = 0; w < words; ++w) {
    const Bytes cut(proof.begin(), proof.begin() + 32 * w);
    CHECK(reason([&] { open_proof(vk, inst, cut.data(), cut.size()); }) == "proof truncated");
  }
  Bytes longer = proof;
  longer.resize(proof.size() + 32, 0);
  CHECK(reason([&] { open_proof(vk, inst, longer.data(), longer.size()); }) == "trailing bytes in proof");
  // 3
  {
    Transcript t(vk.cfg.transcript);
    t.common_scalar(vk.digest);
    for (size_t i = 0; i < prefix_len; ++i) t.common_scalar(inst[i]);
    const Transcript::State st = t.snapshot();
    CHECK(same(open_proof(vk, inst, proof.data(), proof.size(), &st, prefix_len), whole));
  }
  // 4
  {
    const HostDecoded d(proof);
    CHECK(same(open_proof(vk, inst, proof.data(), proof.size(), nullptr, 0, &d.dec), whole));
  }
  Bytes big(32), noroot(32, 0), stray(32, 0);
  U256 q7;
  fe::add_raw(q7, fe::Q_MOD, fe::from_u64(7));
  memcpy(big.data(), q7.l, 32);
  AffinePoint a;
  for (noroot[0] = 5; decode_point(noroot.data(), a) != ZKFHE_PT_NOT_ON_CURVE; ++noroot[0]) CHECK(noroot[0] < 200);
  stray[31] = ptenc::layout().identity_bit, stray[3] = 1;
  const std::pair<const Bytes *, const char *> bad[] = {
      {&big, "point x not reduced"}, {&noroot, "point not on curve"}, {&stray, "non-canonical encoding of the identity"}};
  for (const auto &bw : bad) {
    Bytes p = proof;
    memcpy(p.data() + 32, bw.first->data(), 32);   // commitment 1
    const HostDecoded d(p);
    const std::string host = reason([&] { open_proof(vk, inst, p.data(), p.size()); });
    CHECK(host == bw.second && host == reason([&] { open_proof(vk, inst, p.data(), p.size(), nullptr, 0, &d.dec); }));
  }
  printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
