// A register-resident nine-limb Fr value for kernels that multiply DATA by DATA (the quotient, the grand products, the batch
// inversion): the signed lazy limbs Lz<LO, HI, V> of fq29.hip.hpp / lz29.hip.hpp with the products of mont29.hip.hpp over r.
//
// Memory keeps the library's standard form: x 2^256 mod r, canonical, 8 x u32.  The nine-limb product divides by 2^261, so of the two
// operands of a product one is in the standard form ("S": x 2^256) and one carries 2^261 ("C": x 2^261) -- the result is S again:
//   mul(S, C) = S     mul(C, C) = C     mul(S, S) would be x y 2^251: never written.
// Both forms come out of the same packed word by regrouping its bits, 27 shift / mask operations either way:
//   fr9_load(w)     S: the plain regrouping, value w < r                                      Lz<0, 1, 1>
//   fr9_load32(w)   C: the regrouping five bits up, value 32 w < 32 r (not reduced)            Lz<0, 1, 32>
//   fr9_times32(a)  the same five bits on a tight value in registers: a product result that is the C operand of the next product
// fr9_cc(a) takes a C value to x 2^266 (one product with the constant 2^266 mod r): against it an S operand gives a C result, which a
// loop needs when the sum it multiplies by has to be in the C form (v + beta sigma + gamma in the permutation argument: the running
// product stays S, the factor is C, and beta, resp. the thread's x, is turned once before the loop).
//
// Bounds are part of the type, as everywhere on Lz: -LO 2^29 < l[i] < HI 2^29 for i < 8, |value| < V r.  Addition and subtraction are
// lz_add / lz_sub (nine v_add / v_sub); carries are propagated (fr9_norm = lz_norm) only where a product's limb bound asks for it.
// A product's exact value is (a b + m r) / 2^261 with 0 <= m < 2^261, so |a b| < K 2^261 r gives a value in (-K r, (K + 1) r): with
// 2^261 / r = 169.29.. the products here take V1 V2 <= 160 and return Lz<0, 1, 2>, or V1 V2 <= 338 (< 2 x 169.29) and return
// Lz<0, 1, 3>; an operand's value stays below 127 r, so that its top limb is below 2^29 like the others.  The column bound does not
// depend on the values: nine products of limbs whose bounds multiply to at most 2 (below 2 2^58 each), nine m_j r_(k-j) below 2^58
// and the carry: 27 2^58 + 2^35 < 2^63, inside the signed accumulator.
// fr9_store gives the canonical packed word -- bit for bit what fp_mul / fp_add would have stored.
#pragma once
#include "lz29.hip.hpp"

namespace zk {

using Fr9S = Lz<0, 1, 1>;    // a canonical column value, S form
using Fr9C = Lz<0, 1, 32>;   // the same word read five bits up: C form, not reduced
template <int VV>
using Fr9P = Lz<0, 1, (VV <= 160 ? 2 : 3)>;   // what a product of total bound VV returns

ZK_HD Fr9S fr9_load(const Fr &w) { return lz_load(w); }
ZK_HD Fr9S fr9_one() { return lz_load(Fr::one()); }
ZK_HD Fr9C fr9_load32(const Fr &w) {
  Fr9C r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int bit = 29 * i - 5;   // limb i holds bits [29 i - 5, 29 i + 24) of the word
    if (i == 0) {
      r.l[0] = (int)((w.l[0] << 5) & q29::MASK);
    } else {
      const int k = bit >> 5, sh = bit & 31;
      u32 v = w.l[k] >> sh;
      if (sh > 3 && k + 1 < 8) v |= w.l[k + 1] << (32 - sh);
      r.l[i] = (int)(v & q29::MASK);   // the top limb is bits 227 .. 255: 29 bits as well
    }
  }
  return r;
}
// 32 a for a tight value: the limbs regrouped five bits up (limbs 0..7 must be non-negative: Lz<0, 1, V>)
template <int V>
ZK_HD Lz<0, 1, 32 * V> fr9_times32(const Lz<0, 1, V> &a) {
  static_assert(V <= 3, "times32: the result is a product's operand -- its top limb, below 32 V r / 2^232 + 1, stays below 2^29");
  Lz<0, 1, 32 * V> r;
  r.l[0] = (int)(((u32)a.l[0] << 5) & q29::MASK);
#pragma unroll
  for (int i = 1; i < 8; ++i) r.l[i] = (int)((((u32)a.l[i] << 5) & q29::MASK) | ((u32)a.l[i - 1] >> 24));
  r.l[8] = a.l[8] * 32 + (a.l[7] >> 24);
  return r;
}
template <int LO, int HI, int V>
ZK_HD Lz<0, 1, V> fr9_norm(const Lz<LO, HI, V> &a) { return lz_norm(a); }

// a b / 2^261 mod r
template <int L1, int H1, int V1, int L2, int H2, int V2>
ZK_HD Fr9P<V1 * V2> fr9_mul(const Lz<L1, H1, V1> &a, const Lz<L2, H2, V2> &b) {
  static_assert((L1 > H1 ? L1 : H1) * (L2 > H2 ? L2 : H2) <= 2, "product: |a_j b_i| below 2^59");
  static_assert(V1 * V2 <= 338 && V1 <= 127 && V2 <= 127, "product: |a b| < 2 2^261 r");
#ifdef ZK_MONT29_TIED
  return mont29i_mul_v<fr29_mod, Fr9P<V1 * V2>>(a, b);
#else
  return mont29_c<fr29_mod, long long, int, Fr9P<V1 * V2>>(a, b);
#endif
}
// a^2 / 2^261 mod r (a C: the square in the C form).  Value in [0, 3 r).
template <int LO, int HI, int V>
ZK_HD Fr9P<V * V> fr9_sqr(const Lz<LO, HI, V> &a) {
  static_assert(LO <= 1 && HI <= 1, "square: limbs below 2^29 in magnitude");
  static_assert(V * V <= 338, "square: a^2 < 2 2^261 r");
#ifdef ZK_MONT29_TIED
  return mont29i_sqr<fr29_mod, Fr9P<V * V>>(a);
#else
  return mont29_c<fr29_mod, long long, int, Fr9P<V * V>, true>(a, a);
#endif
}
// (a b + c d) / 2^261 mod r with one reduction: eighteen products below 2^58 in magnitude per column and nine m_j r_(k-j)
template <int L1, int H1, int V1, int L2, int H2, int V2, int L3, int H3, int V3, int L4, int H4, int V4>
ZK_HD Fr9P<V1 * V2 + V3 * V4> fr9_mul2(const Lz<L1, H1, V1> &a, const Lz<L2, H2, V2> &b, const Lz<L3, H3, V3> &c, const Lz<L4, H4, V4> &d) {
  static_assert(L1 <= 1 && H1 <= 1 && L2 <= 1 && H2 <= 1 && L3 <= 1 && H3 <= 1 && L4 <= 1 && H4 <= 1, "two-product form: limbs below 2^29 in magnitude");
  static_assert(V1 * V2 + V3 * V4 <= 338 && V1 <= 127 && V2 <= 127 && V3 <= 127 && V4 <= 127, "two-product form: |a b + c d| < 2 2^261 r");
#ifdef ZK_MONT29_TIED
  return mont29i_mul2<fr29_mod, Fr9P<V1 * V2 + V3 * V4>>(a, b, c, d);
#else
  return mont29_c<fr29_mod, long long, int, Fr9P<V1 * V2 + V3 * V4>>(a, b, c, d);
#endif
}

// C -> x 2^266: the operand that makes (S, CC) -> C
template <int LO, int HI, int V>
ZK_HD Fr9P<V> fr9_cc(const Lz<LO, HI, V> &c) {
  constexpr u32 K[9] = /* 2^266 mod r */ {0x0fffead7u, 0x1d5444f4u, 0x04438aa5u, 0x03b4d096u, 0x134c84dau, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
  Fr9S k;
#pragma unroll
  for (int i = 0; i < 9; ++i) k.l[i] = (int)K[i];
  return fr9_mul(c, k);
}

// canonical packed word of any value below 16 r in magnitude
template <int LO, int HI, int V>
ZK_HD Fr fr9_store(const Lz<LO, HI, V> &a) { return lz_store(a); }

// ---- the expressions the prover's kernels share (and the element-wise test entry runs) --------------------------------------------
// One factor of the permutation argument in the C form: v + t + gamma, with t = beta sigma or beta delta^c x already a C product
ZK_HD Lz<0, 1, 66> fr9_perm_factor(const Fr9C &v, const Lz<0, 1, 2> &t, const Fr9C &gamma) { return fr9_norm(lz_add(lz_add(v, t), gamma)); }
// acc * f for the running product (S) and such a factor
template <int V>
ZK_HD Lz<0, 1, 3> fr9_perm_step(const Lz<0, 1, V> &acc, const Lz<0, 1, 66> &f) { return lz_widen<0, 1, 3>(fr9_mul(acc, f)); }
// (a + beta)(s + gamma) of the lookup argument: a, beta S; s, gamma C
ZK_HD Lz<0, 1, 2> fr9_lookup_term(const Fr9S &a, const Fr9S &beta, const Lz<0, 1, 64> &s_gamma) { return fr9_mul(lz_add(a, beta), s_gamma); }
ZK_HD Lz<0, 1, 64> fr9_lookup_sum(const Fr9C &s, const Fr9C &gamma) { return fr9_norm(lz_add(s, gamma)); }

}  // namespace zk
