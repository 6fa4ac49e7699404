// `verify` (reference README.md:48-52: halo2_proofs verify_proof + VerifierSHPLONK + one pairing check), on the host CPU like
// the reference's; tested against oracle-made and GPU-made proofs.  This file: the vk parser, the host MSM, one proof's
// verification and the three C entry points.  The rest of the verifier:
//   proof_reader.hpp   untrusted bytes -> points and scalars, absorbed into the transcript
//   opening.cpp        transcript replay, expression fold, SHPLONK scalars: what one proof leaves for the pairing (open_proof)
//   host_g2.cpp        the verifier's half of an SRS, the final pairing check, the G2 codec
//   verify_batch.cpp   many proofs, one pairing: the part that runs on the GPU
#include <cstdio>

#include "verify_batch.hpp"

using namespace zkhost;
using zk::Fr;

namespace {

// host MSM over G1 (affine canonical in, XYZZ accumulate): small Pippenger, c = 8
AffinePoint msm_host(const std::vector<Fr> &scalars, const std::vector<Pt> &pts) {
  const int c = 8, W = 32;
  std::vector<U256> k(scalars.size());
  for (size_t i = 0; i < scalars.size(); ++i) k[i] = fe::from_mont(scalars[i]);
  std::vector<zk::G1Affine> base(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) base[i] = point_mont(pts[i].p);
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
  return point_canon(zk::g1x_to_affine(total));
}

const char VK_MAGIC[8] = {'Z', 'K', 'F', 'H', 'E', 'V', 'K', '2'};
Vk parse_vk(const uint8_t *d, size_t len) {
  if (len < 8 + 10 * 4 + 32 || memcmp(d, VK_MAGIC, 8)) throw std::runtime_error("not a zkfhe vk file (ZKFHEVK2)");
  uint32_t h[10];
  memcpy(h, d + 8, 40);
  Vk vk;
  vk.cfg.k = h[0], vk.cfg.n_gate0 = h[1], vk.cfg.n_gate1 = h[2], vk.cfg.n_lookup = h[3], vk.cfg.n_rlc = h[4];
  vk.cfg.unusable_rows = h[5], vk.cfg.lookup_bits = h[6], vk.cfg.transcript = h[7];
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
  auto rd = [&](std::vector<AffinePoint> &v, size_t cnt) {
    v.resize(cnt);
    for (size_t i = 0; i < cnt; ++i, p += 64) {
      memcpy(v[i].x.l, p, 32);
      memcpy(v[i].y.l, p + 32, 32);
      if (!(v[i].x < fe::Q_MOD) || !(v[i].y < fe::Q_MOD)) throw std::runtime_error("vk: commitment coordinate not reduced");
    }
  };
  rd(vk.fixed_commit, nf);
  rd(vk.sigma_commit, ns);
  // the digest is what the transcript starts from: it must be the digest OF this configuration and these commitments
  if (!(vk_digest(vk.cfg, vk.fixed_commit, vk.sigma_commit) == vk.digest)) throw std::runtime_error("vk digest does not match its contents");
  return vk;
}
// copies an instance array; NULL, or the rejection reason when a value is not reduced (the copy is complete either way)
const char *load_instances(const uint8_t *src, size_t n, std::vector<U256> &out) {
  out.resize(n);
  if (n) memcpy(out.data(), src, n * 32);
  for (const U256 &v : out)
    if (!(v < fe::MOD)) return "instance not reduced";
  return nullptr;
}

const char *const G2_REJECT = "G2 point: a coordinate is not reduced or the point is not on the curve";
// part (a), the opening, then part (b): F by the host MSM and the pairing check
bool verify_impl(const Vk &vk, const std::vector<U256> &inst, const uint8_t *proof, size_t proof_len, const SrsG2 &srs) {
  const Opening op = open_proof(vk, inst, proof, proof_len);
  return final_check(msm_host(op.scal, op.pts), op.w.p, srs);
}
// one proof behind the argument checks; make_srs runs after the vk and the instances have been accepted
template <class MakeSrs>
int verify_one(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof, size_t proof_len,
               const MakeSrs &make_srs, int *accepted, char *err, size_t err_len) {
  *accepted = 0;
  try {
    const Vk vk = parse_vk(vk_bytes, vk_len);
    std::vector<U256> inst;
    if (const char *bad = load_instances(instances, n_instances, inst)) throw std::runtime_error(bad);
    *accepted = verify_impl(vk, inst, proof, proof_len, make_srs()) ? 1 : 0;
    return ZKFHE_OK;
  } catch (const std::exception &e) {
    if (err && err_len) snprintf(err, err_len, "%s", e.what());
    return ZKFHE_OK;  // a malformed proof is a rejected proof, not an API error
  }
}

}  // namespace

extern "C" {

int zkfhe_bfv_verify(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof, size_t proof_len,
                     const uint8_t *srs_seed, size_t seed_len, int *accepted, char *err, size_t err_len) {
  if (!vk_bytes || !proof || !accepted || (!instances && n_instances) || (!srs_seed && seed_len)) return ZKFHE_EINVAL;
  return verify_one(vk_bytes, vk_len, instances, n_instances, proof, proof_len, [&] { return srs_g2_from_seed(srs_seed, seed_len); }, accepted, err, err_len);
}

int zkfhe_bfv_verify_g2(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof, size_t proof_len,
                        const uint8_t g2[128], const uint8_t s_g2[128], int *accepted, char *err, size_t err_len) {
  if (!vk_bytes || !proof || !accepted || !g2 || !s_g2 || (!instances && n_instances)) return ZKFHE_EINVAL;
  auto load = [&] {
    SrsG2 srs;
    if (!g2_from_canon(g2, srs.g2) || !g2_from_canon(s_g2, srs.sg2)) throw std::runtime_error(G2_REJECT);
    return srs;
  };
  return verify_one(vk_bytes, vk_len, instances, n_instances, proof, proof_len, load, accepted, err, err_len);
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
    const bool g2_bad = g2 && (!g2_from_canon(g2, srs.g2) || !g2_from_canon(s_g2, srs.sg2));
    if (!g2) srs = srs_g2_from_seed(srs_seed, seed_len);
    std::vector<BatchItem> items(n_proofs);
    for (size_t j = 0; j < n_proofs; ++j) {
      BatchItem &it = items[j];
      it.proof = proofs[j];
      it.len = proof_lens[j];
      const char *bad = load_instances(instances[j], n_instances[j], it.inst);
      if (!bad && g2_bad) bad = G2_REJECT;
      if (bad) {
        it.live = false;
        it.why = bad;
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
