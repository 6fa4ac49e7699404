// What the BFV key switch (bfv_key_switch.hip) decomposes: a digit source is a small struct, passed by value as the first argument
// of k_key_switch / k_key_switch_digit, whose at(k, n, q) gives the workgroup of polynomial k a callable d -> the coefficient of
// degree d, below Q.  Also the monomial and pack gathers that bfv_pack.hip shares with the pack source.  A source names the
// profiling slots of its two kernels and the bytes it reads per coefficient, which the launcher's algorithmic-bytes figures use.
#pragma once
#include "rns_ntt.hip.hpp"

namespace zkrns {

// degree d of x^k v for k < 2N, v one polynomial in CircuitInput order
__device__ __forceinline__ uint64_t mono_coeff(const uint64_t *__restrict__ v, unsigned d, unsigned k, unsigned n, uint64_t q) {
  const unsigned j = (d + 2 * n - k) & (2 * n - 1);
  const uint64_t x = v[n - 1 - (j & (n - 1))];
  return j >= n && x ? q - x : x;
}

// degree d of sigma_g(e - x^s o), or of sigma_g(e) where o is null (auto_coeff of the difference; ginv = g^-1 mod 2N, s < N)
__device__ __forceinline__ uint64_t pack_src(const uint64_t *__restrict__ e, const uint64_t *__restrict__ o, unsigned d, unsigned ginv, unsigned s,
                                             unsigned n, uint64_t q) {
  const unsigned j = (d * ginv) & (2 * n - 1), jj = j & (n - 1);   // d ginv < 2^15 2^16
  uint64_t x = e[n - 1 - jj];
  if (o) x = sub_q(x, mono_coeff(o, jj, s, n, q), q);
  return j >= n && x ? q - x : x;
}

// The operands of a pack level: pair p = (group p / h, i = p % h) reads polynomial (p / h) gstride + i of e[comp] and of o[comp]
// (o[comp] null: a trace level, no odd operand)
struct PackOps {
  const uint64_t *e[2], *o[2];
  size_t h, gstride;
  __device__ __forceinline__ size_t at(size_t p) const { return (p / h) * gstride + p % h; }
};

// src ([c][N], CircuitInput order) itself: the relinearization of c^2
struct SrcPlain {
  const uint64_t *src;
  static constexpr int serial_slot = ZKFHE_PROF_BFV_RELIN, digit_slot = ZKFHE_PROF_BFV_KEY_SWITCH_WIDE;
  double bytes() const { return 8.0; }
  __device__ __forceinline__ auto at(size_t k, unsigned n, uint64_t) const {
    const uint64_t *s = src + k * n;
    return [=](unsigned d) { return s[n - 1 - d]; };
  }
};

// sigma_g(src), ginv = g^-1 mod 2N: the Galois key switch of c1
struct SrcGalois {
  const uint64_t *src;
  unsigned ginv;
  static constexpr int serial_slot = ZKFHE_PROF_BFV_GALOIS, digit_slot = ZKFHE_PROF_BFV_KEY_SWITCH_WIDE;
  double bytes() const { return 8.0; }
  __device__ __forceinline__ auto at(size_t k, unsigned n, uint64_t q) const {
    const uint64_t *s = src + k * n;
    const unsigned gi = ginv;
    return [=](unsigned d) { return auto_coeff(s, d, gi, n, q); };
  }
};

// sigma_g(e1 - x^s o1) of pair k of a pack level, read straight from the two operands (no odd operand: sigma_g(e1), a trace level)
struct SrcPack {
  PackOps op;
  unsigned s, ginv;
  static constexpr int serial_slot = ZKFHE_PROF_BFV_PACK, digit_slot = ZKFHE_PROF_BFV_PACK;
  double bytes() const { return op.o[1] ? 16.0 : 8.0; }
  __device__ __forceinline__ auto at(size_t k, unsigned n, uint64_t q) const {
    const size_t a = op.at(k);
    const uint64_t *e = op.e[1] + a * n, *o = op.o[1] ? op.o[1] + a * n : nullptr;
    const unsigned sh = s, gi = ginv;
    return [=](unsigned d) { return pack_src(e, o, d, gi, sh, n, q); };
  }
};

}  // namespace zkrns
