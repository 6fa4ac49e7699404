// The verifier's reader of untrusted proof bytes: 32-byte words in, canonical points and scalars out, each absorbed into the
// transcript.  A point word is decoded on the host (decode_point) or taken from what k_g1_decompress (csrc/verify.hip) made
// of it (Decoded); both give a ZKFHE_PT_* status, and one function turns a status into the rejection text.  Host C++ only.
#pragma once
#include <stdexcept>

#include "../../include/zkfhe.h"
#include "host_util.hpp"
#include "point_encoding.hpp"

namespace zkhost {

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

// 32 bytes -> status and canonical point ((0, 0) unless ZKFHE_PT_OK); the checks and their order are k_g1_decompress's
inline int32_t decode_point(const uint8_t *word, AffinePoint &a) {
  const ptenc::Layout &L = ptenc::layout();
  uint8_t b[32];
  memcpy(b, word, 32);
  a.x = a.y = fe::zero();
  if (ptenc::is_identity_encoding(b)) {
    // the identity has exactly one encoding (halo2curves rejects anything else)
    for (int i = 0; i < 31; ++i)
      if (b[i]) return ZKFHE_PT_BAD_IDENTITY;
    return b[31] != L.identity_bit ? ZKFHE_PT_BAD_IDENTITY : ZKFHE_PT_OK;
  }
  const unsigned sign = (b[31] & L.sign_bit) ? 1u : 0u;
  b[31] &= L.x_mask;
  U256 xc;
  memcpy(xc.l, b, 32);
  if (!(xc < fe::Q_MOD)) return ZKFHE_PT_X_NOT_REDUCED;
  zk::Fq x, three = zk::Fq::zero();
  memcpy(x.l, b, 32);
  three.l[0] = 3;
  x = zk::fp_to_mont<zk::FqP>(x);
  const zk::Fq y2 = x * x * x + zk::fp_to_mont<zk::FqP>(three);
  // sqrt: y = y2^((q+1)/4)
  uint32_t e[8];
  U256 ee;
  fe::add_raw(ee, fe::Q_MOD, fe::one());
  for (int i = 0; i < 4; ++i) ee.l[i] = (ee.l[i] >> 2) | (i < 3 ? ee.l[i + 1] << 62 : 0);
  memcpy(e, ee.l, 32);
  zk::Fq y = zk::fp_pow<zk::FqP>(y2, e);
  if (!(y * y == y2)) return ZKFHE_PT_NOT_ON_CURVE;
  if ((zk::fp_from_mont<zk::FqP>(y).l[0] & 1u) != sign) y = zk::fp_neg<zk::FqP>(y);
  const zk::Fq yc = zk::fp_from_mont<zk::FqP>(y);
  a.x = xc;
  memcpy(a.y.l, yc.l, 32);
  return ZKFHE_PT_OK;
}

inline const char *point_reject_text(int32_t status) {
  switch (status) {
    case ZKFHE_PT_X_NOT_REDUCED: return "point x not reduced";
    case ZKFHE_PT_NOT_ON_CURVE: return "point not on curve";
    default: return "non-canonical encoding of the identity";
  }
}

struct Reader {
  const uint8_t *p;
  size_t len, pos = 0;
  Transcript tr;
  const Decoded *dec;
  Reader(uint32_t kind, const uint8_t *d, size_t l, const Decoded *dec_ = nullptr) : p(d), len(l), tr(kind), dec(dec_) {}
  Pt read_point() {
    if (pos + 32 > len) throw std::runtime_error("proof truncated");
    const size_t word = pos / 32;
    AffinePoint a;
    const int32_t st = dec && word < dec->n ? dec->status[word] : decode_point(p + pos, a);
    pos += 32;
    if (st != ZKFHE_PT_OK) throw std::runtime_error(point_reject_text(st));
    if (dec && word < dec->n) a = point_canon(dec->pt[word]);
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
  zk::Fr challenge() { return mont(tr.squeeze()); }
};

}  // namespace zkhost
