// `verify` (reference README.md:48-52: halo2_proofs verify_proof + VerifierSHPLONK + one pairing check), on the
// host CPU like the reference's.  Mirrors oracle/halo2_ref.py `verify` (same transcript, same expression order,
// same SHPLONK combination) and is tested against oracle-made and GPU-made proofs.
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zkfhe.h"
#include "bfv_circuit.hpp"
#include "pairing.hpp"
#include "shplonk.hpp"
#include "srs_secret.hpp"
#include "transcript.hpp"
#include "vk.hpp"

using namespace zkhost;
using zk::Fr;

zk::Fr zk_fr_root_of_unity(int log_n);  // csrc/core.hip
// the SRS side (srs.hip) borrows the host G2 arithmetic of this file; declared in prover_internal.hpp as well
void zk_srs_g2_from_secret(const U256 &s, uint8_t g2_raw[128], uint8_t sg2_raw[128]);
bool zk_g2_raw_to_canon(const uint8_t raw[128], uint8_t canon[128]);
bool zk_g2_canon_to_raw(const uint8_t canon[128], uint8_t raw[128]);

namespace {

static const uint64_t DELTA_CANON_V[4] = {0x870e56bbe533e9a2ULL, 0x5b5f898e5e963f25ULL, 0x64ec26aad4c86e71ULL, 0x09226b6e22c6f0caULL};

Fr M(const U256 &v) { return fe::to_mont(v); }
Fr Mu(uint64_t v) { return fe::to_mont(fe::from_u64(v)); }
Fr fpow(Fr b, uint64_t e) {
  Fr r = Fr::one();
  while (e) {
    if (e & 1) r = r * b;
    b = b * b;
    e >>= 1;
  }
  return r;
}
Fr finv(const Fr &a) { return zk::fp_inv<zk::FrP>(a); }

// The proof's 32-byte words decompressed ahead of the replay (zkfhe_g1_decompress, batch path): word i's Montgomery point and
// status.  Words past n, and the single verifier (no Decoded at all), take the host square root instead.
struct Decoded {
  const zk::G1Affine *pt = nullptr;
  const int32_t *status = nullptr;
  size_t n = 0;
};

// A commitment as the opening uses it: its value and where it lives -- ref >= 0: the proof's 32-byte word ref; REF_GEN: the
// generator; REF_VK - i: the vk's commitment i (fixed ones, then sigma ones).  The batch path addresses device points by ref.
struct Pt {
  AffinePoint p;
  int32_t ref;
};
const int32_t REF_GEN = -1, REF_VK = -2;

struct Reader {
  const uint8_t *p;
  size_t len, pos = 0;
  Transcript tr;
  const Decoded *dec;
  Reader(uint32_t kind, const uint8_t *d, size_t l, const Decoded *dec_ = nullptr) : p(d), len(l), tr(kind), dec(dec_) {}
  void common_scalar(const U256 &s) { tr.common_scalar(s); }
  Pt read_point() {
    if (pos + 32 > len) throw std::runtime_error("proof truncated");
    const size_t word = pos / 32;
    uint8_t b[32];
    memcpy(b, p + pos, 32);
    pos += 32;
    AffinePoint a;
    const ptenc::Layout &L = ptenc::layout();
    if (dec && word < dec->n) {
      a.x = fe::zero();
      a.y = fe::zero();
      switch (dec->status[word]) {
        case ZKFHE_PT_OK: break;
        case ZKFHE_PT_X_NOT_REDUCED: throw std::runtime_error("point x not reduced");
        case ZKFHE_PT_NOT_ON_CURVE: throw std::runtime_error("point not on curve");
        default: throw std::runtime_error("non-canonical encoding of the identity");
      }
      const zk::G1Affine &m = dec->pt[word];
      if (!m.is_identity()) {
        const zk::Fq x = zk::fp_from_mont<zk::FqP>(m.x), y = zk::fp_from_mont<zk::FqP>(m.y);
        memcpy(a.x.l, x.l, 32);
        memcpy(a.y.l, y.l, 32);
      }
    } else if (ptenc::is_identity_encoding(b)) {
      // the identity has exactly one encoding (halo2curves rejects anything else)
      for (int i = 0; i < 31; ++i)
        if (b[i]) throw std::runtime_error("non-canonical encoding of the identity");
      if (b[31] != L.identity_bit) throw std::runtime_error("non-canonical encoding of the identity");
      a.x = fe::zero();
      a.y = fe::zero();
    } else {
      const unsigned sign = (b[31] & L.sign_bit) ? 1u : 0u;
      b[31] &= L.x_mask;
      memcpy(a.x.l, b, 32);
      static const U256 QMOD = {{0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}};
      if (!(a.x < QMOD)) throw std::runtime_error("point x not reduced");
      const zk::Fq x = pairing::fq_from_canon(a.x);
      const zk::Fq y2 = x * x * x + pairing::fq_from_u64(3);
      // sqrt: y = y2^((q+1)/4)
      uint32_t e[8];
      U256 ee;
      fe::add_raw(ee, QMOD, fe::one());
      for (int i = 0; i < 4; ++i) ee.l[i] = (ee.l[i] >> 2) | (i < 3 ? ee.l[i + 1] << 62 : 0);
      memcpy(e, ee.l, 32);
      zk::Fq y = zk::fp_pow<zk::FqP>(y2, e);
      if (!(y * y == y2)) throw std::runtime_error("point not on curve");
      zk::Fq yc = zk::fp_from_mont<zk::FqP>(y);
      if ((yc.l[0] & 1u) != sign) y = zk::fp_neg<zk::FqP>(y);
      yc = zk::fp_from_mont<zk::FqP>(y);
      memcpy(a.y.l, yc.l, 32);
    }
    tr.common_point(a);   // Poseidon: refuses the identity, as snark-verifier does
    return Pt{a, (int32_t)word};
  }
  U256 read_scalar() {
    if (pos + 32 > len) throw std::runtime_error("proof truncated");
    U256 s;
    memcpy(s.l, p + pos, 32);
    pos += 32;
    if (!(s < fe::MOD)) throw std::runtime_error("scalar not reduced");
    tr.common_scalar(s);
    return s;
  }
  U256 squeeze() { return tr.squeeze(); }
};

// host MSM over G1 (affine canonical in, XYZZ accumulate): small Pippenger, c = 8
zk::G1Affine to_dev_affine(const AffinePoint &p) {
  zk::G1Affine a;
  a.x = pairing::fq_from_canon(p.x);
  a.y = pairing::fq_from_canon(p.y);
  return a;
}
AffinePoint msm_host(const std::vector<Fr> &scalars, const std::vector<AffinePoint> &pts) {
  const int c = 8, W = 32;
  std::vector<U256> k(scalars.size());
  for (size_t i = 0; i < scalars.size(); ++i) k[i] = fe::from_mont(scalars[i]);
  std::vector<zk::G1Affine> base(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) base[i] = to_dev_affine(pts[i]);
  zk::G1X total = zk::G1X::identity();
  for (int w = W - 1; w >= 0; --w) {
    for (int d = 0; d < c; ++d) total = zk::g1x_dbl(total);
    std::vector<zk::G1X> buckets(255, zk::G1X::identity());
    for (size_t i = 0; i < k.size(); ++i) {
      const unsigned dgt = (unsigned)((k[i].l[(w * c) >> 6] >> ((w * c) & 63)) & 0xff);
      if (dgt) zk::g1x_add_affine(buckets[dgt - 1], base[i], false);
    }
    zk::G1X run = zk::G1X::identity(), sum = zk::G1X::identity();
    for (int b = 254; b >= 0; --b) {
      zk::g1x_add(run, buckets[b]);
      zk::g1x_add(sum, run);
    }
    zk::g1x_add(total, sum);
  }
  const zk::G1Affine r = zk::g1x_to_affine(total);
  AffinePoint out;
  const zk::Fq x = zk::fp_from_mont<zk::FqP>(r.x), y = zk::fp_from_mont<zk::FqP>(r.y);
  memcpy(out.x.l, x.l, 32);
  memcpy(out.y.l, y.l, 32);
  return out;
}

struct Vk {
  CircuitConfig cfg;
  std::vector<AffinePoint> fixed_commit, sigma_commit;
  U256 digest;
};

const char VK_MAGIC[8] = {'Z', 'K', 'F', 'H', 'E', 'V', 'K', '2'};

Vk parse_vk(const uint8_t *d, size_t len) {
  if (len < 8 + 10 * 4 + 32 || memcmp(d, VK_MAGIC, 8)) throw std::runtime_error("not a zkfhe vk file (ZKFHEVK2)");
  uint32_t h[10];
  memcpy(h, d + 8, 40);
  Vk vk;
  vk.cfg.k = h[0];
  vk.cfg.n_gate0 = h[1];
  vk.cfg.n_gate1 = h[2];
  vk.cfg.n_lookup = h[3];
  vk.cfg.n_rlc = h[4];
  vk.cfg.unusable_rows = h[5];
  vk.cfg.lookup_bits = h[6];
  vk.cfg.transcript = h[7];
  // bounds first: n(), u() and the root of unity are only defined for these (2-adicity of Fr is 28)
  if (vk.cfg.k < 3 || vk.cfg.k > 28) throw std::runtime_error("vk: k out of range");
  if (vk.cfg.unusable_rows < 4 || vk.cfg.unusable_rows >= vk.cfg.n()) throw std::runtime_error("vk: unusable_rows out of range");
  if (vk.cfg.n_gate0 > 4096 || vk.cfg.n_gate1 > 4096 || vk.cfg.n_lookup > 4096 || vk.cfg.n_rlc > 4096 || vk.cfg.n_gate() == 0)
    throw std::runtime_error("vk: column counts out of range");
  if (vk.cfg.lookup_bits == 0 || vk.cfg.lookup_bits > 20 || ((size_t)1 << vk.cfg.lookup_bits) > vk.cfg.max_rows()) throw std::runtime_error("vk: lookup_bits out of range");
  if (vk.cfg.transcript > TR_BLAKE2B) throw std::runtime_error("vk: unknown transcript kind");
  const size_t nf = h[8], ns = h[9];
  if (nf != vk.cfg.n_fixed() || ns != vk.cfg.n_perm()) throw std::runtime_error("vk commitment counts do not match its configuration");
  if (len != 8 + 40 + 32 + 64 * (nf + ns)) throw std::runtime_error("vk file has the wrong size");
  memcpy(vk.digest.l, d + 48, 32);
  const uint8_t *p = d + 80;
  static const U256 QMOD = {{0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}};
  auto rd = [&](std::vector<AffinePoint> &v, size_t cnt) {
    v.resize(cnt);
    for (size_t i = 0; i < cnt; ++i, p += 64) {
      memcpy(v[i].x.l, p, 32);
      memcpy(v[i].y.l, p + 32, 32);
      if (!(v[i].x < QMOD) || !(v[i].y < QMOD)) throw std::runtime_error("vk: commitment coordinate not reduced");
    }
  };
  rd(vk.fixed_commit, nf);
  rd(vk.sigma_commit, ns);
  // the digest is what the transcript starts from: it must be the digest OF this configuration and these commitments
  if (!(vk_digest(vk.cfg, vk.fixed_commit, vk.sigma_commit) == vk.digest)) throw std::runtime_error("vk digest does not match its contents");
  return vk;
}

struct Item {  // one opened polynomial
  int kind;    // 0 = commitment point, 1 = H (combination of the quotient pieces), 2 = generator
  Pt commit;
  std::vector<int> rots;  // 0,1,2,3 ; 4 = last ; 5 = -1
  std::vector<Fr> evals;
};

// the verifier's half of an SRS: G2 and s*G2 (the library's own setups derive s from a seed; an external ceremony supplies them)
struct SrsG2 {
  pairing::Pt<pairing::Fq2> g2, sg2;
};
SrsG2 srs_g2_from_seed(const uint8_t *srs_seed, size_t seed_len) {
  const U256 s = srs_secret(srs_seed, seed_len);
  SrsG2 r;
  r.g2 = pairing::g2_generator();
  r.sg2 = pairing::ec_mul(r.g2, s);
  return r;
}

// What the final check needs of one proof: F = sum scal[i] * pts[i] (the SHPLONK combination) and W (= h2), to be checked as
// e(F, G2) e(-W, s G2) = 1.
struct Opening {
  std::vector<Fr> scal;
  std::vector<Pt> pts;
  Pt w;
};

// Part (a) of verification: transcript replay, instance evaluation, the expression fold and the SHPLONK scalars.  Throws the
// rejection reason of a malformed proof.  prefix (may be NULL): the transcript state after the vk digest and the first
// prefix_len instances (shared by the proofs of one public key in a batch); dec (may be NULL): pre-decoded points.
Opening open_impl(const Vk &vk, const std::vector<U256> &inst, const uint8_t *proof, size_t proof_len, const Transcript::State *prefix = nullptr,
                  size_t prefix_len = 0, const Decoded *dec = nullptr) {
  const CircuitConfig &cfg = vk.cfg;
  const size_t n = cfg.n(), u = cfg.u();
  const Fr w = zk_fr_root_of_unity((int)cfg.k);
  // halo2 verify_proof: Error::InstanceTooLarge.  Without it L_{i+n} = L_i would let value move between instance i and i+n.
  if (inst.size() > u) throw std::runtime_error("more instances than usable rows");
  Reader tr(cfg.transcript, proof, proof_len, dec);
  size_t absorbed = 0;
  if (prefix) {
    tr.tr.restore(*prefix);
    absorbed = prefix_len;
  } else {
    tr.common_scalar(vk.digest);
  }
  for (size_t i = absorbed; i < inst.size(); ++i) tr.common_scalar(inst[i]);
  std::vector<Pt> adv_commit;
  for (unsigned c = 0; c < cfg.n_gate0; ++c) adv_commit.push_back(tr.read_point());
  const Fr gamma_rlc = M(tr.squeeze());
  for (unsigned c = cfg.n_gate0; c < cfg.n_advice(); ++c) adv_commit.push_back(tr.read_point());
  tr.squeeze();  // theta
  std::vector<Pt> la_commit, ls_commit;
  for (unsigned i = 0; i < cfg.n_lookup; ++i) {
    la_commit.push_back(tr.read_point());
    ls_commit.push_back(tr.read_point());
  }
  const Fr beta = M(tr.squeeze()), gamma = M(tr.squeeze());
  std::vector<Pt> pz_commit, lz_commit;
  for (unsigned j = 0; j < cfg.n_chunks(); ++j) pz_commit.push_back(tr.read_point());
  for (unsigned i = 0; i < cfg.n_lookup; ++i) lz_commit.push_back(tr.read_point());
  const Pt rand_commit = tr.read_point();
  const Fr y = M(tr.squeeze());
  Pt h_commit[3];
  for (auto &p : h_commit) p = tr.read_point();
  const Fr x = M(tr.squeeze());
  // ---- evaluations, in the prover's write order
  std::vector<Item> items;
  std::map<std::pair<int, int>, Fr> ev_adv, ev_pz, ev_lz, ev_la, ev_ls;
  std::vector<Fr> ev_fixed(cfg.n_fixed()), ev_sigma(cfg.n_perm());
  auto read_item = [&](const Pt &cm, std::vector<int> rots) {
    Item it;
    it.kind = 0;
    it.commit = cm;
    it.rots = rots;
    for (size_t r = 0; r < rots.size(); ++r) it.evals.push_back(M(tr.read_scalar()));
    items.push_back(it);
    return items.back().evals;
  };
  for (unsigned c = 0; c < cfg.n_advice(); ++c) {
    std::vector<int> rots = c < cfg.n_gate() ? std::vector<int>{0, 1, 2, 3} : (c < cfg.adv_rlc0() ? std::vector<int>{0} : std::vector<int>{0, 1, 2});
    const auto e = read_item(adv_commit[c], rots);
    for (size_t r = 0; r < rots.size(); ++r) ev_adv[{(int)c, rots[r]}] = e[r];
  }
  for (unsigned c = 0; c < cfg.n_fixed(); ++c) ev_fixed[c] = read_item(Pt{vk.fixed_commit[c], REF_VK - (int32_t)c}, {0})[0];
  const size_t h_slot = items.size();
  {
    Item it;
    it.kind = 1;
    it.rots = {0};
    it.evals = {Fr::zero()};
    items.push_back(it);
  }
  read_item(rand_commit, {0});
  for (unsigned c = 0; c < cfg.n_perm(); ++c) ev_sigma[c] = read_item(Pt{vk.sigma_commit[c], REF_VK - (int32_t)(cfg.n_fixed() + c)}, {0})[0];
  for (unsigned j = 0; j < cfg.n_chunks(); ++j) {
    std::vector<int> rots = j + 1 != cfg.n_chunks() ? std::vector<int>{0, 1, 4} : std::vector<int>{0, 1};
    const auto e = read_item(pz_commit[j], rots);
    for (size_t r = 0; r < rots.size(); ++r) ev_pz[{(int)j, rots[r]}] = e[r];
  }
  for (unsigned i = 0; i < cfg.n_lookup; ++i) {
    auto e = read_item(lz_commit[i], {0, 1});
    ev_lz[{(int)i, 0}] = e[0];
    ev_lz[{(int)i, 1}] = e[1];
    e = read_item(la_commit[i], {0, 5});
    ev_la[{(int)i, 0}] = e[0];
    ev_la[{(int)i, 5}] = e[1];
    ev_ls[{(int)i, 0}] = read_item(ls_commit[i], {0})[0];
  }
  // ---- Lagrange values and the instance evaluation at x
  const Fr xn = fpow(x, n), zh = xn - Fr::one(), ninv = finv(Mu(n));
  auto lagr_many = [&](size_t first, size_t count) {  // L_i(x) = w^i zh / (n (x - w^i)), batch inverted
    std::vector<Fr> den(count), wi(count);
    Fr cur = fpow(w, first);
    for (size_t i = 0; i < count; ++i) {
      wi[i] = cur;
      den[i] = x - cur;
      cur = cur * w;
    }
    std::vector<Fr> pre(count);
    Fr acc = Fr::one();
    for (size_t i = 0; i < count; ++i) {
      pre[i] = acc;
      acc = acc * den[i];
    }
    acc = finv(acc);
    std::vector<Fr> out(count);
    for (size_t i = count; i-- > 0;) {
      out[i] = wi[i] * zh * ninv * (acc * pre[i]);
      acc = acc * den[i];
    }
    return out;
  };
  Fr inst_x = Fr::zero();
  if (!inst.empty()) {
    const auto L = lagr_many(0, inst.size());
    for (size_t i = 0; i < inst.size(); ++i) inst_x = inst_x + M(inst[i]) * L[i];
  }
  const Fr l0 = lagr_many(0, 1)[0], llast = lagr_many(u, 1)[0];
  Fr lblind = Fr::zero();
  for (const Fr &v : lagr_many(u + 1, n - u - 1)) lblind = lblind + v;
  const Fr lactive = Fr::one() - llast - lblind;
  // ---- fold every constraint expression with y (order of oracle/halo2_ref.py expressions_at)
  Fr acc = Fr::zero();
  auto fold = [&](const Fr &e) { acc = acc * y + e; };
  for (unsigned j = 0; j < cfg.n_gate(); ++j)
    fold(ev_fixed[j] * (ev_adv[{(int)j, 0}] + ev_adv[{(int)j, 1}] * ev_adv[{(int)j, 2}] - ev_adv[{(int)j, 3}]));
  for (unsigned j = 0; j < cfg.n_rlc; ++j) {
    const int col = (int)(cfg.adv_rlc0() + j);
    fold(ev_fixed[cfg.fix_qrlc0() + j] * (ev_adv[{col, 0}] * gamma_rlc + ev_adv[{col, 1}] - ev_adv[{col, 2}]));
  }
  const int m = (int)cfg.n_chunks() - 1;
  const Fr one = Fr::one();
  fold(l0 * (one - ev_pz[{0, 0}]));
  fold(llast * (ev_pz[{m, 0}] * ev_pz[{m, 0}] - ev_pz[{m, 0}]));
  for (int j = 1; j <= m; ++j) fold(l0 * (ev_pz[{j, 0}] - ev_pz[{j - 1, 4}]));
  U256 dc;
  memcpy(dc.l, DELTA_CANON_V, 32);
  const Fr delta = M(dc);
  std::vector<Fr> dpow(cfg.n_perm());
  {
    Fr cur = Fr::one();
    for (auto &d : dpow) {
      d = cur;
      cur = cur * delta;
    }
  }
  auto permcol = [&](unsigned c) { return c < cfg.n_advice() ? ev_adv[{(int)c, 0}] : (c == cfg.perm_const() ? ev_fixed[cfg.fix_const()] : inst_x); };
  for (int j = 0; j <= m; ++j) {
    Fr left = ev_pz[{j, 1}], right = ev_pz[{j, 0}];
    for (unsigned c = j * cfg.chunk(); c < (j + 1) * cfg.chunk() && c < cfg.n_perm(); ++c) {
      const Fr v = permcol(c);
      left = left * (v + beta * ev_sigma[c] + gamma);
      right = right * (v + beta * dpow[c] * x + gamma);
    }
    fold(lactive * (left - right));
  }
  for (unsigned i = 0; i < cfg.n_lookup; ++i) {
    const Fr z0 = ev_lz[{(int)i, 0}], z1 = ev_lz[{(int)i, 1}], a = ev_adv[{(int)(cfg.adv_lookup0() + i), 0}], s = ev_fixed[cfg.fix_table()];
    const Fr ap = ev_la[{(int)i, 0}], apm = ev_la[{(int)i, 5}], sp = ev_ls[{(int)i, 0}];
    fold(l0 * (one - z0));
    fold(llast * (z0 * z0 - z0));
    fold(lactive * (z1 * ((ap + beta) * (sp + gamma)) - z0 * ((a + beta) * (s + gamma))));
    fold(l0 * (ap - sp));
    fold(lactive * ((ap - sp) * (ap - apm)));
  }
  items[h_slot].evals[0] = acc * finv(zh);
  // ---- SHPLONK (halo2 VerifierSHPLONK::verify_proof)
  const Fr yq = M(tr.squeeze()), v = M(tr.squeeze());
  const Pt h1 = tr.read_point();
  const Fr uu = M(tr.squeeze());
  const Pt h2 = tr.read_point();
  if (tr.pos != proof_len) throw std::runtime_error("trailing bytes in proof");
  Fr pts_rot[N_ROT_IDS];
  pts_rot[ROT_0] = x;
  pts_rot[ROT_1] = x * w;
  pts_rot[ROT_2] = pts_rot[1] * w;
  pts_rot[ROT_3] = pts_rot[2] * w;
  pts_rot[ROT_LAST] = x * fpow(w, u);
  pts_rot[ROT_PREV] = x * finv(w);
  const OpenLayout layout(cfg);
  if (items.size() != layout.count || h_slot != layout.H) throw std::logic_error("opening layout mismatch");
  std::vector<int> all_rots;
  const std::vector<OpenSet> sets = intermediate_sets(layout, open_queries(cfg, layout), all_rots);
  Opening op;
  std::vector<Fr> &scal = op.scal;
  std::vector<Pt> &pts = op.pts;
  Fr r_outer = Fr::zero(), vj = Fr::one(), z_0 = Fr::one(), z_0_diff_inv = Fr::one();
  for (size_t j = 0; j < sets.size(); ++j) {
    const auto &rots = sets[j].rots;
    Fr zdiff = Fr::one();
    for (int r : all_rots)
      if (std::find(rots.begin(), rots.end(), r) == rots.end()) zdiff = zdiff * (uu - pts_rot[r]);
    if (j == 0) {
      // normalised by the first set: its own vanishing polynomial multiplies h1, everything else is divided by z_diff_0
      for (int r : rots) z_0 = z_0 * (uu - pts_rot[r]);
      z_0_diff_inv = finv(zdiff);
      zdiff = Fr::one();
    } else {
      zdiff = zdiff * z_0_diff_inv;
    }
    const Fr coef = vj * zdiff;
    std::vector<Fr> comb(rots.size(), Fr::zero());
    Fr pw = Fr::one();
    for (size_t mi : sets[j].members) {
      const Item &it = items[mi];
      if (it.kind == 1) {
        Fr xp = Fr::one();
        for (int t = 0; t < 3; ++t) {
          pts.push_back(h_commit[t]);
          scal.push_back(coef * pw * xp);
          xp = xp * xn;
        }
      } else {
        pts.push_back(it.commit);
        scal.push_back(coef * pw);
      }
      for (size_t t = 0; t < rots.size(); ++t) comb[t] = comb[t] + pw * it.evals[layout.eval_slot(mi, rots[t])];
      pw = pw * yq;
    }
    // r_j(u) by Lagrange interpolation through (points of the set, comb)
    Fr ru = Fr::zero();
    for (size_t a = 0; a < rots.size(); ++a) {
      Fr num = Fr::one(), den = Fr::one();
      for (size_t b = 0; b < rots.size(); ++b)
        if (a != b) {
          num = num * (uu - pts_rot[rots[b]]);
          den = den * (pts_rot[rots[a]] - pts_rot[rots[b]]);
        }
      ru = ru + comb[a] * num * finv(den);
    }
    r_outer = r_outer + coef * ru;
    vj = vj * v;
  }
  AffinePoint gen;
  gen.x = fe::from_u64(1);
  gen.y = fe::from_u64(2);
  pts.push_back(Pt{gen, REF_GEN});
  scal.push_back(Fr::zero() - r_outer);
  pts.push_back(h1);
  scal.push_back(Fr::zero() - z_0);
  pts.push_back(h2);
  scal.push_back(uu);
  op.w = h2;
  return op;
}

// Part (b): e(F, G2) e(-W, s G2) = 1, i.e. e(h2, s G2) = e(F, G2)
bool final_check(const AffinePoint &F, const AffinePoint &w_commit, const SrsG2 &srs) {
  const pairing::Pt<pairing::Fq2> &g2 = srs.g2, &sg2 = srs.sg2;
  pairing::G1 Fp{F.x, F.y}, nW;
  nW.x = w_commit.x;
  nW.y = w_commit.is_identity() ? fe::zero() : [&] {
    static const U256 QMOD = {{0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}};
    U256 r;
    fe::sub_raw(r, QMOD, w_commit.y);
    return r;
  }();
  return pairing::pairing_product_is_one({{Fp, g2}, {nW, sg2}});
}

bool verify_impl(const Vk &vk, const std::vector<U256> &inst, const uint8_t *proof, size_t proof_len, const SrsG2 &srs) {
  const Opening op = open_impl(vk, inst, proof, proof_len);
  std::vector<AffinePoint> pts(op.pts.size());
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = op.pts[i].p;
  return final_check(msm_host(op.scal, pts), op.w.p, srs);
}

const U256 QMOD_C = {{0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}};

void g2_to_raw(const pairing::Pt<pairing::Fq2> &p, uint8_t raw[128]) {
  const zk::Fq *c[4] = {&p.x.c[0], &p.x.c[1], &p.y.c[0], &p.y.c[1]};
  for (int i = 0; i < 4; ++i) memcpy(raw + 32 * i, c[i]->l, 32);
}
bool g2_from_canon(const uint8_t canon[128], pairing::Pt<pairing::Fq2> &p) {
  U256 c[4];
  memcpy(c, canon, 128);
  for (const auto &x : c)
    if (!(x < QMOD_C)) return false;
  p.x.c = {pairing::fq_from_canon(c[0]), pairing::fq_from_canon(c[1])};
  p.y.c = {pairing::fq_from_canon(c[2]), pairing::fq_from_canon(c[3])};
  p.inf = false;
  return pairing::g2_on_curve(p);
}

}  // namespace

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
    if (!(lim < QMOD_C)) return false;   // a Montgomery residue is reduced too
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

// ---- batch verification (zkfhe_bfv_verify_batch) --------------------------------------------------------------------------
namespace {

// CPUs this process may run on: its affinity mask, capped by OMP_NUM_THREADS when set (never the machine's count)
unsigned usable_cpus() {
  unsigned n = 1;
  cpu_set_t cs;
  CPU_ZERO(&cs);
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) n = (unsigned)CPU_COUNT(&cs);
  if (const char *e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0 && (unsigned)v < n) n = (unsigned)v;
  }
  return n;
}
// f(i) for i < n on up to usable_cpus() threads; f must not throw
template <class F>
void parallel_for(size_t n, const F &f) {
  const size_t T = std::min<size_t>(usable_cpus(), n);
  if (T <= 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (size_t t = 0; t < T; ++t)
    th.emplace_back([&] {
      for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    });
  for (auto &x : th) x.join();
}

// 32-byte words of a well-formed proof under cfg (the reads of open_impl, in count): what the batch decompresses per proof
size_t proof_words(const CircuitConfig &cfg) {
  size_t w = cfg.n_advice() + 3 * cfg.n_lookup + cfg.n_chunks() + 1 + 3 + 2;   // commitments, random, h pieces, h1, h2
  for (unsigned c = 0; c < cfg.n_advice(); ++c) w += c < cfg.n_gate() ? 4 : (c < cfg.adv_rlc0() ? 1 : 3);
  w += cfg.n_fixed() + 1 + cfg.n_perm() + 3 * (cfg.n_chunks() - 1) + 2 + 5 * cfg.n_lookup;   // fixed, random, sigma, z, lookups
  return w;
}

// Public-key prefix of the BFV instance column: pk0 | pk1, the first 2 N of its 5 N + 1 values (prefix_cache.hpp); 0 otherwise
size_t bfv_key_prefix(size_t n_inst) { return n_inst > 1 && (n_inst - 1) % 5 == 0 ? 2 * ((n_inst - 1) / 5) : 0; }

void put_u64(Blake2b &h, uint64_t v) { h.update(&v, 8); }

AffinePoint canon_of(const zk::G1Affine &m) {
  AffinePoint a;
  a.x = fe::zero();
  a.y = fe::zero();
  if (m.is_identity()) return a;
  const zk::Fq x = zk::fp_from_mont<zk::FqP>(m.x), y = zk::fp_from_mont<zk::FqP>(m.y);
  memcpy(a.x.l, x.l, 32);
  memcpy(a.y.l, y.l, 32);
  return a;
}

struct BatchItem {
  std::vector<U256> inst;
  const uint8_t *proof = nullptr;
  size_t len = 0;
  bool live = true;    // not rejected yet
  std::string why;
  Fr r;                // randomiser (Montgomery)
  int group = -1;      // shared public-key prefix
  size_t words = 0, base = 0;
  Opening op;
  AffinePoint F, W;
};

// device buffer of one chunk, freed on every path
struct DevBuf {
  zkfhe_ctx *ctx;
  void *p = nullptr;
  explicit DevBuf(zkfhe_ctx *c) : ctx(c) {}
  ~DevBuf() {
    if (p) zkfhe_dev_free(ctx, p);
  }
};

#define VB_CK(x)            \
  do {                      \
    const int rc__ = (x);   \
    if (rc__) return rc__;  \
  } while (0)

const size_t BATCH_CHUNK = 256;   // proofs per device pass: ~30 MB of device memory at k = 13

int verify_batch(zkfhe_ctx *ctx, const Vk &vk, const SrsG2 &srs, std::vector<BatchItem> &items) {
  const CircuitConfig &cfg = vk.cfg;
  const size_t N = items.size();
  // ---- randomisers: bound to the vk and to every (instances, proof) of the batch, in order
  uint8_t D[64];
  {
    Blake2b h(64, "zkfhe-batch-D");
    for (const BatchItem &it : items) {
      put_u64(h, it.inst.size());
      for (const U256 &v : it.inst) h.update(v.l, 32);
      put_u64(h, it.len);
      h.update(it.proof, it.len);
    }
    h.digest(D);
  }
  for (size_t j = 0; j < N; ++j) {
    Blake2b h(64, "zkfhe-batch-r");
    h.update(vk.digest.l, 32);
    h.update(D, 64);
    put_u64(h, j);
    uint8_t d[64];
    h.digest(d);
    U256 r = fe::zero();
    memcpy(r.l, d, 16);   // 128 bits: below r, so already reduced
    if (r.is_zero()) r.l[0] = 1;
    items[j].r = M(r);
  }
  // ---- shared public keys: the transcript state after digest | pk0 | pk1, once per key with two proofs or more
  const size_t P = items.empty() ? 0 : bfv_key_prefix(items[0].inst.size());
  std::vector<Transcript::State> states;
  if (P) {
    std::map<std::string, int> key;
    std::vector<int> members;
    std::vector<size_t> leader;
    for (size_t j = 0; j < N; ++j) {
      BatchItem &it = items[j];
      if (!it.live || it.inst.size() < P || it.inst.size() > cfg.u()) continue;
      std::string k((const char *)it.inst.data(), P * 32);
      auto f = key.find(k);
      if (f == key.end()) {
        f = key.emplace(std::move(k), (int)members.size()).first;
        members.push_back(0);
        leader.push_back(j);
      }
      it.group = f->second;
      members[f->second]++;
    }
    states.resize(members.size());
    std::vector<char> ok(members.size(), 0);
    parallel_for(members.size(), [&](size_t g) {
      if (members[g] < 2) return;
      try {
        Transcript t(cfg.transcript);
        t.common_scalar(vk.digest);
        for (size_t i = 0; i < P; ++i) t.common_scalar(items[leader[g]].inst[i]);
        states[g] = t.snapshot();
        ok[g] = 1;
      } catch (...) {
      }
    });
    for (BatchItem &it : items)
      if (it.group >= 0 && !ok[it.group]) it.group = -1;
  }
  // ---- the vk's commitments and the generator, Montgomery, shared by every segment: device points [0, NV]
  std::vector<zk::G1Affine> vkpts;
  for (const AffinePoint &a : vk.fixed_commit) vkpts.push_back(to_dev_affine(a));
  for (const AffinePoint &a : vk.sigma_commit) vkpts.push_back(to_dev_affine(a));
  {
    AffinePoint gen;
    gen.x = fe::from_u64(1);
    gen.y = fe::from_u64(2);
    vkpts.push_back(to_dev_affine(gen));
  }
  const size_t NV = vkpts.size() - 1, PB = NV + 1;   // PB: first proof word
  const size_t cap_words = proof_words(cfg);
  zk::G1X A = zk::G1X::identity(), B = zk::G1X::identity();
  std::vector<size_t> cand;   // proofs that reach the pairing
  for (size_t c0 = 0; c0 < N; c0 += BATCH_CHUNK) {
    const size_t c1 = std::min(N, c0 + BATCH_CHUNK);
    size_t W = 0;
    for (size_t j = c0; j < c1; ++j) {
      BatchItem &it = items[j];
      it.words = it.live ? std::min(it.len / 32, cap_words) : 0;
      it.base = W;
      W += it.words;
    }
    const size_t n_pts = PB + W + (c1 - c0);   // + one F per proof
    // [points | compressed words | statuses]
    DevBuf buf(ctx);
    VB_CK(zkfhe_dev_alloc(ctx, n_pts * 64 + W * 32 + W * 4 + 64, &buf.p));
    uint8_t *d_pts = (uint8_t *)buf.p, *d_in = d_pts + n_pts * 64, *d_st = d_in + W * 32;
    VB_CK(zkfhe_upload(ctx, d_pts, vkpts.data(), vkpts.size() * 64));
    std::vector<zk::G1Affine> hpts(W);
    std::vector<int32_t> hst(W);
    if (W) {
      std::vector<uint8_t> hin(W * 32);
      for (size_t j = c0; j < c1; ++j)
        if (items[j].words) memcpy(&hin[items[j].base * 32], items[j].proof, items[j].words * 32);
      VB_CK(zkfhe_upload(ctx, d_in, hin.data(), hin.size()));
      VB_CK(zkfhe_g1_decompress(ctx, d_in, W, (zkfhe_g1_affine *)(d_pts + PB * 64), (int32_t *)d_st));
      VB_CK(zkfhe_download(ctx, hpts.data(), d_pts + PB * 64, W * 64));
      VB_CK(zkfhe_download(ctx, hst.data(), d_st, W * 4));
    }
    // ---- transcript replays on host threads, from the decompressed points
    parallel_for(c1 - c0, [&](size_t i) {
      BatchItem &it = items[c0 + i];
      if (!it.live) return;
      try {
        const Decoded dec{hpts.data() + it.base, hst.data() + it.base, it.words};
        it.op = open_impl(vk, it.inst, it.proof, it.len, it.group >= 0 ? &states[it.group] : nullptr, P, &dec);
        for (const Pt &q : it.op.pts)
          if (q.ref >= (int32_t)it.words) throw std::logic_error("batch verifier: a point outside the decompressed words");
      } catch (const std::exception &e) {
        it.live = false;
        it.why = e.what();
      }
    });
    // ---- segments: one per surviving proof, then sum r_j F_j and sum r_j W_j
    std::vector<uint32_t> idx, off{0};
    std::vector<Fr> sc;
    std::vector<size_t> seg;
    for (size_t j = c0; j < c1; ++j) {
      BatchItem &it = items[j];
      if (!it.live) continue;
      for (size_t t = 0; t < it.op.pts.size(); ++t) {
        const int32_t ref = it.op.pts[t].ref;
        idx.push_back((uint32_t)(ref >= 0 ? PB + it.base + ref : ref == REF_GEN ? NV : REF_VK - ref));
        sc.push_back(it.op.scal[t]);
      }
      off.push_back((uint32_t)idx.size());
      seg.push_back(j);
      it.op.scal.clear();
    }
    const size_t K = seg.size();
    if (!K) continue;
    const size_t FB = PB + W;   // F_j of segment k at FB + k
    for (size_t k = 0; k < K; ++k) {
      idx.push_back((uint32_t)(FB + k));
      sc.push_back(items[seg[k]].r);
    }
    for (size_t k = 0; k < K; ++k) {
      const BatchItem &it = items[seg[k]];
      idx.push_back((uint32_t)(PB + it.base + it.op.w.ref));
      sc.push_back(it.r);
    }
    const size_t T0 = off.back(), T = idx.size();
    off.push_back((uint32_t)(T0 + K));
    off.push_back((uint32_t)T);
    DevBuf tb(ctx);
    VB_CK(zkfhe_dev_alloc(ctx, T * 4 + T * 32 + off.size() * 4 + 2 * 64 + 256, &tb.p));
    uint8_t *d_sc = (uint8_t *)tb.p, *d_ab = d_sc + T * 32, *d_idx = d_ab + 128, *d_off = d_idx + ((T * 4 + 63) & ~(size_t)63);
    VB_CK(zkfhe_upload(ctx, d_sc, sc.data(), T * 32));
    VB_CK(zkfhe_upload(ctx, d_idx, idx.data(), T * 4));
    VB_CK(zkfhe_upload(ctx, d_off, off.data(), off.size() * 4));
    // F_j: segments [0, K) over the shared points; then the two weighted sums over the F_j and the proofs' h2 words
    VB_CK(zkfhe_msm_segmented(ctx, (const zkfhe_g1_affine *)d_pts, FB, (const uint32_t *)d_idx, (const zkfhe_fr *)d_sc, T0, (const uint32_t *)d_off, K,
                              (zkfhe_g1_affine *)(d_pts + FB * 64)));
    VB_CK(zkfhe_msm_segmented(ctx, (const zkfhe_g1_affine *)d_pts, FB + K, (const uint32_t *)d_idx, (const zkfhe_fr *)d_sc, T, (const uint32_t *)d_off + K, 2,
                              (zkfhe_g1_affine *)d_ab));
    std::vector<zk::G1Affine> F(K), AB(2);
    VB_CK(zkfhe_download(ctx, F.data(), d_pts + FB * 64, K * 64));
    VB_CK(zkfhe_download(ctx, AB.data(), d_ab, 128));
    zk::g1x_add_affine(A, AB[0], false);
    zk::g1x_add_affine(B, AB[1], false);
    for (size_t k = 0; k < K; ++k) {
      BatchItem &it = items[seg[k]];
      it.F = canon_of(F[k]);
      it.W = it.op.w.p;
      it.op = Opening();
      cand.push_back(seg[k]);
    }
  }
  if (cand.empty()) return ZKFHE_OK;
  // ---- one pairing for the whole batch; if it fails, each proof's own check from its F_j, W_j
  if (final_check(canon_of(zk::g1x_to_affine(A)), canon_of(zk::g1x_to_affine(B)), srs)) return ZKFHE_OK;   // every candidate holds
  std::vector<char> ok(cand.size(), 0);
  parallel_for(cand.size(), [&](size_t i) { ok[i] = final_check(items[cand[i]].F, items[cand[i]].W, srs) ? 1 : 0; });
  for (size_t i = 0; i < cand.size(); ++i) items[cand[i]].live = ok[i] != 0;
  return ZKFHE_OK;
}

}  // namespace

// zkfhe_srs_check (srs.hip): e(A, s_g2) e(-B, g2) = 1 for affine Montgomery points A, B and raw G2 coordinates -- the final check
// of a proof with F = B, W = A (the inverse of that product).  false as well when a G2 point is not on the twist.
bool zk_srs_pairing_powers(const zk::G1Affine &A, const zk::G1Affine &B, const uint8_t g2_raw[128], const uint8_t sg2_raw[128]) {
  uint8_t canon[128];
  SrsG2 srs;
  if (!zk_g2_raw_to_canon(g2_raw, canon) || !g2_from_canon(canon, srs.g2)) return false;
  if (!zk_g2_raw_to_canon(sg2_raw, canon) || !g2_from_canon(canon, srs.sg2)) return false;
  return final_check(canon_of(B), canon_of(A), srs);
}

extern "C" {

int zkfhe_srs_file_g2(const char *path, uint32_t *k_out, uint8_t g2_le[128], uint8_t s_g2_le[128]) {
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

int zkfhe_bfv_verify(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof, size_t proof_len,
                     const uint8_t *srs_seed, size_t seed_len, int *accepted, char *err, size_t err_len) {
  if (!vk_bytes || !proof || !accepted || (!instances && n_instances) || (!srs_seed && seed_len)) return ZKFHE_EINVAL;
  *accepted = 0;
  try {
    const Vk vk = parse_vk(vk_bytes, vk_len);
    std::vector<U256> inst(n_instances);
    if (n_instances) memcpy(inst.data(), instances, n_instances * 32);
    for (const auto &v : inst)
      if (!(v < fe::MOD)) throw std::runtime_error("instance not reduced");
    *accepted = verify_impl(vk, inst, proof, proof_len, srs_g2_from_seed(srs_seed, seed_len)) ? 1 : 0;
    return ZKFHE_OK;
  } catch (const std::exception &e) {
    if (err && err_len) snprintf(err, err_len, "%s", e.what());
    return ZKFHE_OK;  // a malformed proof is a rejected proof, not an API error
  }
}

int zkfhe_bfv_verify_g2(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof, size_t proof_len,
                        const uint8_t g2[128], const uint8_t s_g2[128], int *accepted, char *err, size_t err_len) {
  if (!vk_bytes || !proof || !accepted || !g2 || !s_g2 || (!instances && n_instances)) return ZKFHE_EINVAL;
  *accepted = 0;
  try {
    const Vk vk = parse_vk(vk_bytes, vk_len);
    std::vector<U256> inst(n_instances);
    if (n_instances) memcpy(inst.data(), instances, n_instances * 32);
    for (const auto &v : inst)
      if (!(v < fe::MOD)) throw std::runtime_error("instance not reduced");
    auto load = [](const uint8_t *b) {
      pairing::Pt<pairing::Fq2> p;
      // reduced coordinates, on the twist y^2 = x^3 + 3/(9+i)  (subgroup membership is the caller's responsibility, as in halo2's ParamsKZG::read)
      if (!g2_from_canon(b, p)) throw std::runtime_error("G2 point: a coordinate is not reduced or the point is not on the curve");
      return p;
    };
    SrsG2 srs;
    srs.g2 = load(g2);
    srs.sg2 = load(s_g2);
    *accepted = verify_impl(vk, inst, proof, proof_len, srs) ? 1 : 0;
    return ZKFHE_OK;
  } catch (const std::exception &e) {
    if (err && err_len) snprintf(err, err_len, "%s", e.what());
    return ZKFHE_OK;
  }
}

int zkfhe_bfv_verify_batch(zkfhe_ctx *ctx, const uint8_t *vk_bytes, size_t vk_len, size_t n_proofs, const uint8_t *const *instances,
                           const size_t *n_instances, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *srs_seed,
                           size_t seed_len, const uint8_t *g2, const uint8_t *s_g2, int *accepted, char *errs, size_t err_stride) {
  if (!ctx || !vk_bytes || !n_proofs || !instances || !n_instances || !proofs || !proof_lens || !accepted) return ZKFHE_EINVAL;
  if (!g2 != !s_g2 || (!g2 && !srs_seed && seed_len)) return ZKFHE_EINVAL;
  for (size_t j = 0; j < n_proofs; ++j)
    if ((!proofs[j] && proof_lens[j]) || (!instances[j] && n_instances[j])) return ZKFHE_EINVAL;
  for (size_t j = 0; j < n_proofs; ++j) {
    accepted[j] = 0;
    if (errs && err_stride) errs[j * err_stride] = 0;
  }
  auto put_err = [&](size_t j, const std::string &m) {
    if (errs && err_stride) snprintf(errs + j * err_stride, err_stride, "%s", m.c_str());
  };
  try {
    Vk vk;
    try {
      vk = parse_vk(vk_bytes, vk_len);
    } catch (const std::exception &e) {
      for (size_t j = 0; j < n_proofs; ++j) put_err(j, e.what());
      return ZKFHE_OK;
    }
    SrsG2 srs;
    std::string g2_err;
    if (g2) {
      if (!g2_from_canon(g2, srs.g2) || !g2_from_canon(s_g2, srs.sg2))
        g2_err = "G2 point: a coordinate is not reduced or the point is not on the curve";
    } else {
      srs = srs_g2_from_seed(srs_seed, seed_len);
    }
    std::vector<BatchItem> items(n_proofs);
    for (size_t j = 0; j < n_proofs; ++j) {
      BatchItem &it = items[j];
      it.inst.resize(n_instances[j]);
      if (n_instances[j]) memcpy(it.inst.data(), instances[j], n_instances[j] * 32);
      it.proof = proofs[j];
      it.len = proof_lens[j];
      for (const U256 &v : it.inst)
        if (!(v < fe::MOD)) {
          it.live = false;
          it.why = "instance not reduced";
          break;
        }
      if (it.live && !g2_err.empty()) {
        it.live = false;
        it.why = g2_err;
      }
    }
    const int rc = verify_batch(ctx, vk, srs, items);
    if (rc) return rc;
    for (size_t j = 0; j < n_proofs; ++j) {
      accepted[j] = items[j].live ? 1 : 0;
      if (!items[j].why.empty()) put_err(j, items[j].why);
    }
    return ZKFHE_OK;
  } catch (const std::bad_alloc &) {
    return ZKFHE_ENOMEM;
  } catch (const std::exception &) {
    return ZKFHE_EINVAL;
  }
}

}  // extern "C"
