// Part (a) of verification, on the host: replay the transcript over the proof, evaluate the instances, fold the constraint
// expressions and derive the SHPLONK scalars.  Mirrors oracle/halo2_ref.py `verify` (same transcript, same expression order,
// same SHPLONK combination).  Which polynomial is opened where, and in which order, is shplonk.hpp's OpenLayout alone.
#include "opening.hpp"

#include <algorithm>

#include "shplonk.hpp"

zk::Fr zk_fr_root_of_unity(int log_n);  // csrc/core.hip

namespace zkhost {
namespace {
using zk::Fr;

struct Open {  // what crosses a step of open_proof
  const Vk &vk;
  const CircuitConfig &cfg;
  const std::vector<U256> &inst;
  Reader tr;
  const OpenLayout L;
  const Fr w;
  std::vector<Pt> commit;  // per layout item; H has none (its three pieces are h_commit)
  Pt h_commit[3];
  Fr gamma_rlc, beta, gamma, y, x;
  std::vector<size_t> ev0;  // first slot of each item in ev
  std::vector<Fr> ev;       // evaluations by (item, slot); H's comes from the fold
  Fr xn, zh, inst_x, l0, llast, lactive;
  Open(const Vk &vk_, const std::vector<U256> &inst_, const uint8_t *proof, size_t len, const Decoded *dec)
      : vk(vk_), cfg(vk_.cfg), inst(inst_), tr(vk_.cfg.transcript, proof, len, dec), L(vk_.cfg), w(zk_fr_root_of_unity((int)vk_.cfg.k)) {}
  const Fr &at(size_t item, int rot) const { return ev[ev0[item] + L.eval_slot(item, rot)]; }
  const Fr &adv(unsigned c, int rot = ROT_0) const { return at(L.adv0 + c, rot); }
  const Fr &fixed(unsigned c) const { return at(L.fixed0 + c, ROT_0); }
  const Fr &sigma(unsigned c) const { return at(L.sigma0 + c, ROT_0); }
  const Fr &pz(unsigned j, int rot) const { return at(L.pz0 + j, rot); }
  const Fr &lz(unsigned i, int rot) const { return at(L.lk0 + 3 * i, rot); }      // lookup i: product,
  const Fr &la(unsigned i, int rot) const { return at(L.lk0 + 3 * i + 1, rot); }  // permuted input,
  const Fr &ls(unsigned i) const { return at(L.lk0 + 3 * i + 2, ROT_0); }         // permuted table
};
// The commitment rounds: vk digest (or the restored prefix state) and instances in, commitments read, challenges out
void replay_commitments(Open &o, const Transcript::State *prefix, size_t prefix_len) {
  const CircuitConfig &cfg = o.cfg;
  const OpenLayout &L = o.L;
  Reader &tr = o.tr;
  if (prefix) tr.tr.restore(*prefix);
  else tr.tr.common_scalar(o.vk.digest);
  for (size_t i = prefix ? prefix_len : 0; i < o.inst.size(); ++i) tr.tr.common_scalar(o.inst[i]);
  o.commit.resize(L.count);
  for (unsigned c = 0; c < cfg.n_gate0; ++c) o.commit[L.adv0 + c] = tr.read_point();
  o.gamma_rlc = tr.challenge();
  for (unsigned c = cfg.n_gate0; c < cfg.n_advice(); ++c) o.commit[L.adv0 + c] = tr.read_point();
  tr.challenge();  // theta
  for (unsigned i = 0; i < cfg.n_lookup; ++i) {
    o.commit[L.lk0 + 3 * i + 1] = tr.read_point();
    o.commit[L.lk0 + 3 * i + 2] = tr.read_point();
  }
  o.beta = tr.challenge();
  o.gamma = tr.challenge();
  for (unsigned j = 0; j < cfg.n_chunks(); ++j) o.commit[L.pz0 + j] = tr.read_point();
  for (unsigned i = 0; i < cfg.n_lookup; ++i) o.commit[L.lk0 + 3 * i] = tr.read_point();
  o.commit[L.rand] = tr.read_point();
  o.y = tr.challenge();
  for (auto &p : o.h_commit) p = tr.read_point();
  o.x = tr.challenge();
  // the columns the vk commits to
  for (unsigned c = 0; c < cfg.n_fixed(); ++c) o.commit[L.fixed0 + c] = Pt{o.vk.fixed_commit[c], REF_VK - (int32_t)c};
  for (unsigned c = 0; c < cfg.n_perm(); ++c) o.commit[L.sigma0 + c] = Pt{o.vk.sigma_commit[c], REF_VK - (int32_t)(cfg.n_fixed() + c)};
}
// The evaluations, in the layout's write order; H is the item that is not read
void read_evaluations(Open &o) {
  const OpenLayout &L = o.L;
  o.ev0.assign(L.count + 1, 0);
  for (size_t i = 0; i < L.count; ++i) o.ev0[i + 1] = o.ev0[i] + L.rots[i].size();
  o.ev.assign(o.ev0[L.count], Fr::zero());
  for (size_t i = 0; i < L.count; ++i)
    for (size_t t = 0; i != L.H && t < L.rots[i].size(); ++t) o.ev[o.ev0[i] + t] = mont(o.tr.read_scalar());
}
// L_i(x) = w^i zh / (n (x - w^i)) for i in [first, first + count), batch inverted
std::vector<Fr> lagr_many(const Open &o, const Fr &ninv, size_t first, size_t count) {
  std::vector<Fr> den(count), wi(count), pre(count), out(count);
  Fr cur = fr_pow(o.w, first), acc = Fr::one();
  for (size_t i = 0; i < count; ++i) {
    wi[i] = cur;
    den[i] = o.x - cur;
    cur = cur * o.w;
    pre[i] = acc;
    acc = acc * den[i];
  }
  acc = fr_inv(acc);
  for (size_t i = count; i-- > 0;) {
    out[i] = wi[i] * o.zh * ninv * (acc * pre[i]);
    acc = acc * den[i];
  }
  return out;
}
// Lagrange values and the instance evaluation at x
void lagrange_and_instances(Open &o) {
  const size_t n = o.cfg.n(), u = o.cfg.u();
  o.xn = fr_pow(o.x, n);
  o.zh = o.xn - Fr::one();
  const Fr ninv = fr_inv(mont_u64(n));
  o.inst_x = Fr::zero();
  if (!o.inst.empty()) {
    const auto L = lagr_many(o, ninv, 0, o.inst.size());
    for (size_t i = 0; i < o.inst.size(); ++i) o.inst_x = o.inst_x + mont(o.inst[i]) * L[i];
  }
  o.l0 = lagr_many(o, ninv, 0, 1)[0];
  o.llast = lagr_many(o, ninv, u, 1)[0];
  Fr lblind = Fr::zero();
  for (const Fr &v : lagr_many(o, ninv, u + 1, n - u - 1)) lblind = lblind + v;
  o.lactive = Fr::one() - o.llast - lblind;
}
// Fold every constraint expression with y (order of oracle/halo2_ref.py expressions_at): H's evaluation is the sum over zh
void fold_expressions(Open &o) {
  const CircuitConfig &cfg = o.cfg;
  const Fr one = Fr::one(), &l0 = o.l0, &llast = o.llast, &lactive = o.lactive, &beta = o.beta, &gamma = o.gamma;
  Fr acc = Fr::zero();
  auto fold = [&](const Fr &e) { acc = acc * o.y + e; };
  for (unsigned j = 0; j < cfg.n_gate(); ++j) fold(o.fixed(j) * (o.adv(j) + o.adv(j, ROT_1) * o.adv(j, ROT_2) - o.adv(j, ROT_3)));
  for (unsigned j = 0; j < cfg.n_rlc; ++j) {
    const unsigned col = cfg.adv_rlc0() + j;
    fold(o.fixed(cfg.fix_qrlc0() + j) * (o.adv(col) * o.gamma_rlc + o.adv(col, ROT_1) - o.adv(col, ROT_2)));
  }
  const unsigned m = cfg.n_chunks() - 1;
  fold(l0 * (one - o.pz(0, ROT_0)));
  fold(llast * (o.pz(m, ROT_0) * o.pz(m, ROT_0) - o.pz(m, ROT_0)));
  for (unsigned j = 1; j <= m; ++j) fold(l0 * (o.pz(j, ROT_0) - o.pz(j - 1, ROT_LAST)));
  U256 dc;
  memcpy(dc.l, DELTA_CANON, 32);
  const Fr delta = mont(dc);
  Fr dpow = Fr::one();   // delta^c
  for (unsigned j = 0; j <= m; ++j) {
    Fr left = o.pz(j, ROT_1), right = o.pz(j, ROT_0);
    for (unsigned c = j * cfg.chunk(); c < (j + 1) * cfg.chunk() && c < cfg.n_perm(); ++c) {
      const Fr v = c < cfg.n_advice() ? o.adv(c) : (c == cfg.perm_const() ? o.fixed(cfg.fix_const()) : o.inst_x);
      left = left * (v + beta * o.sigma(c) + gamma);
      right = right * (v + beta * dpow * o.x + gamma);
      dpow = dpow * delta;
    }
    fold(lactive * (left - right));
  }
  for (unsigned i = 0; i < cfg.n_lookup; ++i) {
    const Fr &z0 = o.lz(i, ROT_0), &z1 = o.lz(i, ROT_1), &a = o.adv(cfg.adv_lookup0() + i), &s = o.fixed(cfg.fix_table());
    const Fr &ap = o.la(i, ROT_0), &apm = o.la(i, ROT_PREV), &sp = o.ls(i);
    fold(l0 * (one - z0));
    fold(llast * (z0 * z0 - z0));
    fold(lactive * (z1 * ((ap + beta) * (sp + gamma)) - z0 * ((a + beta) * (s + gamma))));
    fold(l0 * (ap - sp));
    fold(lactive * ((ap - sp) * (ap - apm)));
  }
  o.ev[o.ev0[o.L.H]] = acc * fr_inv(o.zh);
}
// One point set of the multi-open: its members' commitments and scalars go to op, weighted by coef and the powers of yq;
// returns r_j(u), the Lagrange interpolation at u through (points of the set, the members' combined evaluations)
Fr set_terms(const Open &o, const OpenSet &set, const Fr &coef, const Fr &yq, const Fr *pts_rot, const Fr &uu, Opening &op) {
  const auto &rots = set.rots;
  std::vector<Fr> comb(rots.size(), Fr::zero());
  Fr pw = Fr::one();
  for (size_t mi : set.members) {
    if (mi == o.L.H) {
      Fr xp = Fr::one();
      for (int t = 0; t < 3; ++t) {
        op.pts.push_back(o.h_commit[t]);
        op.scal.push_back(coef * pw * xp);
        xp = xp * o.xn;
      }
    } else {
      op.pts.push_back(o.commit[mi]);
      op.scal.push_back(coef * pw);
    }
    for (size_t t = 0; t < rots.size(); ++t) comb[t] = comb[t] + pw * o.at(mi, rots[t]);
    pw = pw * yq;
  }
  Fr ru = Fr::zero();
  for (size_t a = 0; a < rots.size(); ++a) {
    Fr num = Fr::one(), den = Fr::one();
    for (size_t b = 0; b < rots.size(); ++b)
      if (a != b) {
        num = num * (uu - pts_rot[rots[b]]);
        den = den * (pts_rot[rots[a]] - pts_rot[rots[b]]);
      }
    ru = ru + comb[a] * num * fr_inv(den);
  }
  return ru;
}
// SHPLONK (halo2 VerifierSHPLONK::verify_proof): the last challenges and h1, h2, then every set's terms and the three closing ones
Opening shplonk_scalars(Open &o) {
  Reader &tr = o.tr;
  const Fr yq = tr.challenge(), v = tr.challenge();
  const Pt h1 = tr.read_point();
  const Fr uu = tr.challenge();
  const Pt h2 = tr.read_point();
  if (tr.pos != tr.len) throw std::runtime_error("trailing bytes in proof");
  Fr pts_rot[N_ROT_IDS];
  pts_rot[ROT_0] = o.x;
  for (int r = ROT_1; r <= ROT_3; ++r) pts_rot[r] = pts_rot[r - 1] * o.w;
  pts_rot[ROT_LAST] = o.x * fr_pow(o.w, o.cfg.u());
  pts_rot[ROT_PREV] = o.x * fr_inv(o.w);
  std::vector<int> all_rots;
  const std::vector<OpenSet> sets = intermediate_sets(o.L, open_queries(o.cfg, o.L), all_rots);
  Opening op;
  Fr r_outer = Fr::zero(), vj = Fr::one(), z_0 = Fr::one(), z_0_diff_inv = Fr::one();
  for (size_t j = 0; j < sets.size(); ++j) {
    const auto &rots = sets[j].rots;
    Fr zdiff = Fr::one();
    for (int r : all_rots)
      if (std::find(rots.begin(), rots.end(), r) == rots.end()) zdiff = zdiff * (uu - pts_rot[r]);
    if (j == 0) {
      // normalised by the first set: its own vanishing polynomial multiplies h1, everything else is divided by z_diff_0
      for (int r : rots) z_0 = z_0 * (uu - pts_rot[r]);
      z_0_diff_inv = fr_inv(zdiff);
      zdiff = Fr::one();
    } else {
      zdiff = zdiff * z_0_diff_inv;
    }
    const Fr coef = vj * zdiff;
    r_outer = r_outer + coef * set_terms(o, sets[j], coef, yq, pts_rot, uu, op);
    vj = vj * v;
  }
  op.pts.insert(op.pts.end(), {Pt{g1_generator(), REF_GEN}, h1, h2});
  op.scal.insert(op.scal.end(), {Fr::zero() - r_outer, Fr::zero() - z_0, uu});
  op.w = h2;
  return op;
}

}  // namespace

Opening open_proof(const Vk &vk, const std::vector<U256> &inst, const uint8_t *proof, size_t proof_len, const Transcript::State *prefix,
                   size_t prefix_len, const Decoded *dec) {
  // halo2 verify_proof: Error::InstanceTooLarge.  Without it L_{i+n} = L_i would let value move between instance i and i+n.
  if (inst.size() > vk.cfg.u()) throw std::runtime_error("more instances than usable rows");
  Open o(vk, inst, proof, proof_len, dec);
  replay_commitments(o, prefix, prefix_len);
  read_evaluations(o);
  lagrange_and_instances(o);
  fold_expressions(o);
  return shplonk_scalars(o);
}

}  // namespace zkhost
