// Host G2 and pairing glue (host_g2.hpp): the seed-derived verifier half of an SRS, the final pairing check, the raw / canonical
// G2 codec of the SRS side, and the G2 points of a saved SRS file.
#include "host_g2.hpp"

#include <cstdio>

#include "../../include/zkfhe.h"
#include "host_util.hpp"
#include "srs_secret.hpp"

using namespace zkhost;

SrsG2 srs_g2_from_seed(const uint8_t *srs_seed, size_t seed_len) {
  const U256 s = srs_secret(srs_seed, seed_len);
  SrsG2 r;
  r.g2 = pairing::g2_generator();
  r.sg2 = pairing::ec_mul(r.g2, s);
  return r;
}

bool final_check(const AffinePoint &F, const AffinePoint &w_commit, const SrsG2 &srs) {
  pairing::G1 Fp{F.x, F.y}, nW{w_commit.x, fe::zero()};
  if (!w_commit.is_identity()) fe::sub_raw(nW.y, fe::Q_MOD, w_commit.y);
  return pairing::pairing_product_is_one({{Fp, srs.g2}, {nW, srs.sg2}});
}

static void g2_to_raw(const pairing::Pt<pairing::Fq2> &p, uint8_t raw[128]) {
  const zk::Fq *c[4] = {&p.x.c[0], &p.x.c[1], &p.y.c[0], &p.y.c[1]};
  for (int i = 0; i < 4; ++i) memcpy(raw + 32 * i, c[i]->l, 32);
}
bool g2_from_canon(const uint8_t canon[128], pairing::Pt<pairing::Fq2> &p) {
  U256 c[4];
  memcpy(c, canon, 128);
  for (const auto &x : c)
    if (!(x < fe::Q_MOD)) return false;
  p.x.c = {pairing::fq_from_canon(c[0]), pairing::fq_from_canon(c[1])};
  p.y.c = {pairing::fq_from_canon(c[2]), pairing::fq_from_canon(c[3])};
  p.inf = false;
  return pairing::g2_on_curve(p);
}

void zk_srs_g2_from_secret(const U256 &s, uint8_t g2_raw[128], uint8_t sg2_raw[128]) {
  const pairing::Pt<pairing::Fq2> g = pairing::g2_generator();
  g2_to_raw(g, g2_raw);
  g2_to_raw(pairing::ec_mul(g, s), sg2_raw);
}
bool zk_g2_raw_to_canon(const uint8_t raw[128], uint8_t canon[128]) {
  for (int i = 0; i < 4; ++i) {
    zk::Fq m;
    memcpy(m.l, raw + 32 * i, 32);
    U256 lim;
    memcpy(lim.l, m.l, 32);
    if (!(lim < fe::Q_MOD)) return false;   // a Montgomery residue is reduced too
    const zk::Fq c = zk::fp_from_mont<zk::FqP>(m);
    memcpy(canon + 32 * i, c.l, 32);
  }
  pairing::Pt<pairing::Fq2> p;
  return g2_from_canon(canon, p);
}
bool zk_g2_canon_to_raw(const uint8_t canon[128], uint8_t raw[128]) {
  pairing::Pt<pairing::Fq2> p;
  if (!g2_from_canon(canon, p)) return false;
  g2_to_raw(p, raw);
  return true;
}
// zkfhe_srs_check (srs.hip): the final check of a proof with F = B, W = A (the inverse of that product).  false as well when a
// G2 point is not on the twist.
bool zk_srs_pairing_powers(const zk::G1Affine &A, const zk::G1Affine &B, const uint8_t g2_raw[128], const uint8_t sg2_raw[128]) {
  uint8_t canon[128];
  SrsG2 srs;
  if (!zk_g2_raw_to_canon(g2_raw, canon) || !g2_from_canon(canon, srs.g2)) return false;
  if (!zk_g2_raw_to_canon(sg2_raw, canon) || !g2_from_canon(canon, srs.sg2)) return false;
  return final_check(point_canon(B), point_canon(A), srs);
}

extern "C" int zkfhe_srs_file_g2(const char *path, uint32_t *k_out, uint8_t g2_le[128], uint8_t s_g2_le[128]) {
  if (!path || !g2_le || !s_g2_le) return ZKFHE_EINVAL;
  FILE *f = fopen(path, "rb");
  if (!f) return ZKFHE_EINVAL;
  uint32_t k = 0;
  uint8_t raw[256];
  bool ok = fread(&k, 4, 1, f) == 1 && k >= 1 && k <= 28;
  const long want = 4 + (long)2 * 64 * ((long)1 << (ok ? k : 1)) + 256;
  ok = ok && fseek(f, 0, SEEK_END) == 0 && ftell(f) == want && fseek(f, want - 256, SEEK_SET) == 0 && fread(raw, 256, 1, f) == 1;
  fclose(f);
  if (!ok) return ZKFHE_EINVAL;
  if (!zk_g2_raw_to_canon(raw, g2_le) || !zk_g2_raw_to_canon(raw + 128, s_g2_le)) return ZKFHE_EINVAL;
  if (k_out) *k_out = k;
  return ZKFHE_OK;
}
