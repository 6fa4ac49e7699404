// BN254 Fq in radix 2^29 (nine u32 limbs, Montgomery with R' = 2^261) for the EC kernels of the MSM.
//
// Why: the 8 x 32-bit product-scanning multiply (bn254.hip.hpp fp_mul) spends half of its issue slots on carries -- every
// v_mad_u64_u32 is followed by s_nop + v_addc_co_u32 (9.9 cycles per pair against 5.3 for the multiply-add alone,
// profiles/r1_microbench.md).  With 29-bit limbs a column of a*b + m*p is at most 18 (27 for the fused two-product form)
// terms below 2^58: they add up in ONE 64-bit accumulator with no carry-out, so a product is 162 plain multiply-adds and
// 18 shift/mask pairs.  The seven spare bits of R' also allow lazy reduction: a product only needs a*b < 2^261 p, i.e.
// operands below 11 p, and returns a value below 2 p -- additions and subtractions in the point formulas do not reduce.
//
// Scope: registers only.  In memory a value stays one packed 256-bit word (the layout of zk::Fq, so tables, partials and
// buckets keep their size); what changes is the Montgomery constant: the MSM tables and accumulators hold x * 2^261 mod p.
// g1x29_to_std() converts a result back to the library's standard form (x * 2^256 mod p, canonical) before normalisation.
//
// Two forms live here; the products of both are wrappers of the one nine-limb Montgomery multiply of mont29.hip.hpp.  F29 with f29_add / f29_sub / f29_mul ...: unsigned limbs < 2^29 (the top limb holds whatever is left: values stay
// < 2^261), carries propagated after every addition, a multiple of p added before every subtraction; the comment of each function states
// the bound on its VALUE (as a multiple of p) it needs and gives.  The Fr kernels that multiply data by table constants (fr29.hip.hpp), the
// radix-2..16 NTT tiles and the square root of the batch verifier use it.
// Lz<LO, HI, V> with lz_add / lz_sub / lq_mul / lq_sqr / lq_mul2 (second half of the file): SIGNED lazy limbs whose bounds are part of the type.
// The point arithmetic of the MSM (g1x29_add_affine, g1x29_add, g1x29_dbl) is written on it and on nothing else: an addition or subtraction
// is nine v_add / v_sub with no carry chain and no multiple of p, one mixed addition propagates carries ONCE (x3, which collects four terms),
// the accumulator stays unreduced from one addition to the next, and the equal-x test is one multiply and one compare on limb 0.  Against
// the normalising form this takes about 200 of the 2500 VALU instructions of a mixed addition away (profiles/msm_lazy_limbs.md).
#pragma once
#include "mont29.hip.hpp"

namespace zk {

struct F29 {
  u32 l[9];
};

namespace q29 {
constexpr u32 INV = 0x04866389u;  // -q^-1 mod 2^29 (MASK: mont29.hip.hpp)
#define ZK_Q29_P \
  { 0x187cfd47u, 0x010460b6u, 0x1c72a34fu, 0x02d522d0u, 0x1585d978u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu }
#define ZK_Q29_2P \
  { 0x10f9fa8eu, 0x0208c16du, 0x18e5469eu, 0x05aa45a1u, 0x0b0bb2f0u, 0x05b68181u, 0x014dc282u, 0x1cb84c68u, 0x0060c89cu }
#define ZK_Q29_3P \
  { 0x0976f7d5u, 0x030d2224u, 0x1557e9edu, 0x087f6872u, 0x00918c68u, 0x0891c242u, 0x01f4a3c3u, 0x0b14729cu, 0x00912cebu }
#define ZK_Q29_4P \
  { 0x01f3f51cu, 0x041182dbu, 0x11ca8d3cu, 0x0b548b43u, 0x161765e0u, 0x0b6d0302u, 0x029b8504u, 0x197098d0u, 0x00c19139u }
#define ZK_Q29_8P \
  { 0x03e7ea38u, 0x082305b6u, 0x03951a78u, 0x16a91687u, 0x0c2ecbc0u, 0x16da0605u, 0x05370a08u, 0x12e131a0u, 0x01832273u }
#define ZK_Q29_ONE /* 2^261 mod p: the Montgomery form of 1 */ \
  { 0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u }
#define ZK_Q29_R256 /* 2^256 mod p as a plain integer: multiplying by it turns x 2^261 into x 2^256 */ \
  { 0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u }
}  // namespace q29

ZK_HD F29 f29_zero() {
  F29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = 0;
  return r;
}
ZK_HD F29 f29_const(const u32 (&c)[9]) {
  F29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = c[i];
  return r;
}
ZK_HD bool f29_is_literal_zero(const F29 &a) {
  u32 o = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) o |= a.l[i];
  return o == 0;
}
ZK_HD bool f29_eq(const F29 &a, const u32 (&c)[9]) {
  u32 o = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) o |= a.l[i] ^ c[i];
  return o == 0;
}

// packed 256-bit word (8 x u32) <-> nine 29-bit limbs.  Packing needs value < 2^256.
ZK_HD F29 f29_unpack(const Fq &w) {
  F29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int bit = 29 * i, k = bit >> 5, sh = bit & 31;
    u32 v = w.l[k] >> sh;
    if (sh > 3 && k + 1 < 8) v |= w.l[k + 1] << (32 - sh);
    r.l[i] = i < 8 ? (v & q29::MASK) : v;
  }
  return r;
}
ZK_HD Fq f29_pack(const F29 &a) {
  Fq w;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // word k holds bits 32k .. 32k+31: limb i = floor(32k / 29) from bit 32k - 29i, then the next limb(s)
    const int i = (32 * k) / 29, sh = 32 * k - 29 * i;
    u32 v = a.l[i] >> sh;
    v |= a.l[i + 1] << (29 - sh);
    if (29 - sh + 29 < 32 && i + 2 < 9) v |= a.l[i + 2] << (58 - sh);
    w.l[k] = v;
  }
  return w;
}

// signed carry propagation: t[i] in (-2^31, 2^31), total value >= 0  ->  limbs < 2^29 (top limb: the rest)
ZK_HD F29 f29_normalise(const int (&t)[9]) {
  F29 r;
  int c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int v = t[i] + c;
    r.l[i] = (u32)v & q29::MASK;
    c = v >> 29;  // arithmetic shift: floor division
  }
  r.l[8] = (u32)(t[8] + c);
  return r;
}

// a + b: value = a + b
ZK_HD F29 f29_add(const F29 &a, const F29 &b) {
  int t[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) t[i] = (int)(a.l[i] + b.l[i]);
  return f29_normalise(t);
}
// a - b + k p for a constant multiple kp >= b: value = a + kp - b > 0
ZK_HD F29 f29_sub(const F29 &a, const F29 &b, const u32 (&kp)[9]) {
  int t[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) t[i] = (int)a.l[i] - (int)b.l[i] + (int)kp[i];
  return f29_normalise(t);
}
ZK_HD F29 f29_neg(const F29 &b, const u32 (&kp)[9]) {  // kp - b
  int t[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) t[i] = (int)kp[i] - (int)b.l[i];
  return f29_normalise(t);
}
ZK_HD F29 f29_dbl(const F29 &a) { return f29_add(a, a); }

#define F29_FN(name) f29_##name
#define F29_P ZK_Q29_P
#define F29_2P ZK_Q29_2P
#define F29_3P ZK_Q29_3P
#define F29_INV q29::INV
#include "f29_field.inc"
#undef F29_FN
#undef F29_P
#undef F29_2P
#undef F29_3P
#undef F29_INV

// ---- lazy signed limbs with compile-time bounds: the form of the point arithmetic below (and, over Fr, of the NTT butterflies:
// lz29.hip.hpp) ------------------------------------------------------------------------------------------------------------
// f29_add / f29_sub / f29_neg above propagate carries after every operation (24 dependent operations) and add a multiple of p
// so that a difference stays positive, although the nine-limb product needs neither.  Here a value is nine SIGNED limbs,
// value = sum l[i] 2^(29 i) of either sign; addition and subtraction are nine v_add / v_sub and nothing else, and a carry
// propagation is written (lz_norm) only where a bound would otherwise be exceeded.
// Lz<LO, HI, V>: -LO 2^29 < l[i] < HI 2^29 for i < 8 (a sum of LO negated and HI plain limbs below 2^29 each) and |value| < V p; the top
// limb is what is left: |l[8]| < (V + 1) 2^22.
// Every operation states its result bound in its return type and static_asserts what it needs, so arithmetic that compiles
// cannot overflow.  "Tight" is Lz<0, 1, V>: limbs 0..7 in [0, 2^29), a signed top limb.
template <int LO, int HI, int V>
struct Lz {
  int l[9];
};

template <int V>
ZK_HD Lz<0, 1, V> lz_from_f29(const F29 &a) {   // caller's promise: a has tight limbs and a value below V p
  Lz<0, 1, V> r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = (int)a.l[i];
  return r;
}
// the same limbs under a wider bound (never a narrower one)
template <int LO2, int HI2, int V2, int LO, int HI, int V>
ZK_HD Lz<LO2, HI2, V2> lz_widen(const Lz<LO, HI, V> &a) {
  static_assert(LO2 >= LO && HI2 >= HI && V2 >= V, "a bound can only be widened");
  Lz<LO2, HI2, V2> r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = a.l[i];
  return r;
}
template <int L1, int H1, int V1, int L2, int H2, int V2>
ZK_HD Lz<L1 + L2, H1 + H2, V1 + V2> lz_add(const Lz<L1, H1, V1> &a, const Lz<L2, H2, V2> &b) {
  static_assert(L1 + L2 <= 4 && H1 + H2 <= 4, "limb overflow");
  Lz<L1 + L2, H1 + H2, V1 + V2> r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + b.l[i];
  return r;
}
template <int L1, int H1, int V1, int L2, int H2, int V2>
ZK_HD Lz<L1 + H2, H1 + L2, V1 + V2> lz_sub(const Lz<L1, H1, V1> &a, const Lz<L2, H2, V2> &b) {
  static_assert(L1 + H2 <= 4 && H1 + L2 <= 4, "limb overflow");
  Lz<L1 + H2, H1 + L2, V1 + V2> r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] - b.l[i];
  return r;
}
template <int LO, int HI, int V>
ZK_HD Lz<HI, LO, V> lz_neg(const Lz<LO, HI, V> &a) {
  Lz<HI, LO, V> r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = -a.l[i];
  return r;
}
// neg ? -a : a
template <int LO, int HI, int V>
ZK_HD Lz<(LO > HI ? LO : HI), (LO > HI ? LO : HI), V> lz_cneg(const Lz<LO, HI, V> &a, bool neg) {
  Lz<(LO > HI ? LO : HI), (LO > HI ? LO : HI), V> r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = neg ? -a.l[i] : a.l[i];
  return r;
}
template <int LO, int HI, int V>
ZK_HD bool lz_is_literal_zero(const Lz<LO, HI, V> &a) {
  int o = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) o |= a.l[i];
  return o == 0;
}

// Carry propagation: limbs 0..7 back into [0, 2^29), the value unchanged.  A limb typed HI = h is a sum of h terms each at most
// 2^29 - 1, so l + carry (|carry| <= 4) stays inside int32 for h = 4; likewise on the negative side.
template <int LO, int HI, int V>
ZK_HD Lz<0, 1, V> lz_norm(const Lz<LO, HI, V> &a) {
  Lz<0, 1, V> r;
  int c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int v = a.l[i] + c;
    r.l[i] = v & (int)q29::MASK;
    c = v >> 29;                // arithmetic: floor
  }
  r.l[8] = a.l[8] + c;
  return r;
}

// ---- Fq: what the MSM's point arithmetic adds to the above -- products of two VARIABLE operands -----------------------------
using LqT = Lz<0, 1, 2>;   // what a product returns (tight limbs, value in (-p, 2 p)); any tight value below 2 p in magnitude
using LqX = Lz<0, 1, 8>;   // an x coordinate of the accumulator: r^2 - ppp - 2 qq after carry propagation, not reduced

// Montgomery product a b / 2^261 mod p for |a b| < 2^261 p = 169.29 p^2: value in (-p, 2 p), tight limbs.  Column k: nine a_j b_(k-j)
// below 2 2^58 in magnitude (one operand's limbs below 2^30 and the other's below 2^29, or the like: the product of the two limb bounds
// is at most 2), nine m_j p_(k-j) below 2^58 and the carry below 2^35: 27 2^58 + 2^35 < 2^63.
template <int L1, int H1, int V1, int L2, int H2, int V2>
ZK_HD LqT lq_mul(const Lz<L1, H1, V1> &a, const Lz<L2, H2, V2> &b) {
  static_assert((L1 > H1 ? L1 : H1) * (L2 > H2 ? L2 : H2) <= 2, "product: |a_j b_i| below 2^59");
  static_assert(V1 * V2 <= 160 && V1 <= 64 && V2 <= 64, "product: |a b| < 2^261 p");
#ifdef ZK_MONT29_TIED
  return mont29i_mul_v<f29_mod, LqT>(a, b);
#else
  return mont29_c<f29_mod, long long, int, LqT>(a, b);
#endif
}
// a^2 / 2^261 mod p for limbs of either sign below 2^29: the cross products a_j a_i (j < i) once, against the doubled limb 2 a_i.
// A column is at most four doubled terms below 2^59, one square and nine reduction terms below 2^58: 18 2^58 < 2^63.  Value in [0, 2 p).
template <int LO, int HI, int V>
ZK_HD LqT lq_sqr(const Lz<LO, HI, V> &a) {
  static_assert(LO <= 1 && HI <= 1, "square: limbs below 2^29 in magnitude");
  static_assert(V * V <= 160, "square: a^2 < 2^261 p");
#ifdef ZK_MONT29_TIED
  return mont29i_sqr<f29_mod, LqT>(a);
#else
  return mont29_c<f29_mod, long long, int, LqT, true>(a, a);
#endif
}
// (a b + c d) / 2^261 mod p with one reduction, all four operands variable: eighteen products below 2^58 in magnitude per column (every
// limb below 2^29 in magnitude) and nine m_j p_(k-j) below 2^58: 27 2^58 + 2^35 < 2^63.  Value in (-p, 2 p).
template <int L1, int H1, int V1, int L2, int H2, int V2, int L3, int H3, int V3, int L4, int H4, int V4>
ZK_HD LqT lq_mul2(const Lz<L1, H1, V1> &a, const Lz<L2, H2, V2> &b, const Lz<L3, H3, V3> &c, const Lz<L4, H4, V4> &d) {
  static_assert(L1 <= 1 && H1 <= 1 && L2 <= 1 && H2 <= 1 && L3 <= 1 && H3 <= 1 && L4 <= 1 && H4 <= 1, "two-product form: limbs below 2^29 in magnitude");
  static_assert(V1 * V2 + V3 * V4 <= 160 && V1 <= 64 && V2 <= 64 && V3 <= 64 && V4 <= 64, "two-product form: |a b + c d| < 2^261 p");
#ifdef ZK_MONT29_TIED
  return mont29i_mul2<f29_mod, LqT>(a, b, c, d);
#else
  return mont29_c<f29_mod, long long, int, LqT>(a, b, c, d);
#endif
}

// value (either sign, |v| < 16 p) -> the same residue in [0, 2 p) (in fact below 1.04 p), tight limbs, top limb included.
// q = floor(t m / 2^16) with t = floor(l[8] / 2^13) and m = 169 for t >= 0, 170 for t < 0 never exceeds v / p and falls short of it by
// less than 1.1 (lz29.hip.hpp lz_weak has the argument: 169 < 2^261 / p = 169.29.. < 170 for both BN254 moduli); |q| <= 17.
// In 32-bit operations only, unlike lz_weak: q p_i = q (p_i mod 2^15) + (q floor(p_i / 2^15) mod 2^14) 2^15 + floor(q floor(p_i / 2^15) / 2^14) 2^29,
// two terms below 2^20 and 2^29 and a carry into the next limb.  The 64-bit form sign-extends every limb into a register PAIR, and the
// register allocator then keeps the accumulator's 36 limbs in the even halves of 36 pairs throughout k_msm_table: the addition loop ran
// out of aligned pairs for its multiply-adds and spilled the prefetched table point (180 bytes of scratch against 8).
template <int LO, int HI, int V>
ZK_HD LqT lq_weak(const Lz<LO, HI, V> &a) {
  static_assert(V <= 16, "weak reduction: |value| below 16 p");
  if constexpr (LO != 0 || HI != 1) {
    return lq_weak(lz_norm(a));
  } else {
    constexpr u32 P[9] = ZK_Q29_P;
    const int t = a.l[8] >> 13;
    const int q = (t * (169 - (t >> 31))) >> 16;
    LqT r;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ql = q * (int)(P[i] & 0x7fffu), qh = q * (int)(P[i] >> 15);
      const int v = a.l[i] - ql - ((qh & 0x3fff) << 15) + c;
      r.l[i] = v & (int)q29::MASK;
      c = (v >> 29) - (qh >> 14);
    }
    r.l[8] = a.l[8] - q * (int)P[8] + c;
    return r;
  }
}
// packed word of a representative in [0, 2 p) -- what partials and buckets hold in memory
template <int LO, int HI, int V>
ZK_HD Fq lq_pack(const Lz<LO, HI, V> &a) {
  const LqT w = lq_weak(a);
  F29 o;
#pragma unroll
  for (int i = 0; i < 9; ++i) o.l[i] = (u32)w.l[i];
  return f29_pack(o);
}
// canonical packed word
template <int LO, int HI, int V>
ZK_HD Fq lq_pack_canonical(const Lz<LO, HI, V> &a) {
  const LqT w = lq_weak(a);
  F29 o;
#pragma unroll
  for (int i = 0; i < 9; ++i) o.l[i] = (u32)w.l[i];
  return f29_pack(f29_canonical(o));
}
ZK_HD LqT lq_unpack(const Fq &w) { return lz_from_f29<2>(f29_unpack(w)); }   // caller's promise: a packed value below 2 p

// Is the value 0 mod p?  Cheap reject first: limb 0 has no incoming carry, so a value k p (|k| < V) has l[0] = k p_0 mod 2^29, i.e.
// l[0] p_0^-1 mod 2^29 = k is within V of zero -- one multiply, one add, one mask, one compare, wrong for 2 V in 2^29 of the other values.
// The full test (a weak reduction) is on the rare path.
template <int LO, int HI, int V>
ZK_HD bool lq_is_zero_mod_p(const Lz<LO, HI, V> &a) {
  static_assert(V <= 16, "zero test: |value| below 16 p");
  constexpr u32 PINV0 = (0u - q29::INV) & q29::MASK;   // p_0^-1 mod 2^29
  if ((((u32)a.l[0] * PINV0 + (u32)V) & q29::MASK) > 2u * V) return false;   // almost always
  constexpr u32 P1[9] = ZK_Q29_P;
  const LqT w = lq_weak(a);   // [0, 2 p): zero or p
  F29 o;
#pragma unroll
  for (int i = 0; i < 9; ++i) o.l[i] = (u32)w.l[i];
  return f29_is_literal_zero(o) || f29_eq(o, P1);
}

// ---- G1 in XYZZ coordinates over lazy limbs.  An accumulator's coordinates stay as the formulas leave them from one addition to
// the next: y, zz, zzz are product results (LqT), x is a carry-propagated r^2 - ppp - 2 qq (LqX); the bounds below show that the next
// addition accepts exactly these types, so a chain of any length needs no reduction.  Values are reduced into [0, 2 p) only where a
// point is packed to memory (g1x29_store) and made canonical where it leaves the kernel (g1x29_to_std).  Identity: zz = literal 0.
struct G1A29 {  // affine, canonical coordinates (table entries); identity (0, 0)
  F29 x, y;
  ZK_HD bool is_identity() const { return f29_is_literal_zero(x) && f29_is_literal_zero(y); }
};
struct G1X29 {
  LqX x;
  LqT y, zz, zzz;
  static ZK_HD G1X29 identity() {
    G1X29 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.x.l[i] = r.y.l[i] = r.zz.l[i] = r.zzz.l[i] = 0;
    return r;
  }
  ZK_HD bool is_identity() const { return lz_is_literal_zero(zz); }
};

// memory forms: zk::G1Affine / zk::G1X hold packed 256-bit words in the 2^261 Montgomery form
ZK_HD G1A29 g1a29_load(const G1Affine &p) {
  G1A29 r;
  r.x = f29_unpack(p.x);
  r.y = f29_unpack(p.y);
  return r;
}
ZK_HD G1X29 g1x29_load(const G1X &p) {   // what g1x29_store wrote: representatives below 2 p
  G1X29 r;
  r.x = lz_widen<0, 1, 8>(lq_unpack(p.x));
  r.y = lq_unpack(p.y);
  r.zz = lq_unpack(p.zz);
  r.zzz = lq_unpack(p.zzz);
  return r;
}
ZK_HD G1X g1x29_store(const G1X29 &p) {
  G1X r;
  r.x = lq_pack(p.x);
  r.y = lq_pack(p.y);
  r.zz = lq_pack(p.zz);
  r.zzz = lq_pack(p.zzz);
  return r;
}

// 2 P for affine P (not the identity).  The rare path of the additions and the ladder of the tail kernels: carries are propagated
// wherever that keeps the bounds simple.  |px| < 8 p, |py| < 2 p.
template <int LX, int HX, int VX, int LY, int HY, int VY>
ZK_HD G1X29 g1x29_from_affine_dbl(const Lz<LX, HX, VX> &px, const Lz<LY, HY, VY> &py) {
  static_assert(VX <= 8 && VY <= 2, "doubling: coordinate bounds");
  G1X29 r;
  const auto u = lz_norm(lz_add(py, py));                        // tight, 4 p
  const LqT v = lq_sqr(u);
  const LqT w = lq_mul(u, v);
  const LqT s = lq_mul(px, v);
  const LqT xx = lq_sqr(px);
  const auto m = lz_norm(lz_add(lz_add(xx, xx), xx));            // tight, 6 p
  const auto x3 = lz_norm(lz_sub(lz_sub(lq_sqr(m), s), s));      // tight, 6 p
  // (x, y, zz, zzz) and (x, -y, zz, -zzz) are the same point: -y3 = m (x3 - s) + w py needs no negated copy of w next to w
  r.y = lq_mul2(m, lz_sub(x3, s), w, py);                        // 6 p 8 p + 2 p 2 p = 52 p^2
  r.x = lz_widen<0, 1, 8>(x3);
  r.zz = v;
  r.zzz = lz_norm(lz_neg(w));
  return r;
}
ZK_HD G1X29 g1x29_dbl(const G1X29 &p) {
  if (p.is_identity()) return p;
  G1X29 r = g1x29_from_affine_dbl(p.x, p.y);   // the same formulas, then the Z factors
  r.zz = lq_mul(r.zz, p.zz);
  r.zzz = lq_mul(r.zzz, p.zzz);
  return r;
}

// The common tail of both additions: p = u2 - u1, r = s2 - s1 (neither 0 mod p), u1, s1 and the Z factors of the sum.
//   x3 = r^2 - ppp - 2 qq: limbs in (-3 2^29, 2^29), |x3| < 8 p; ONE carry propagation makes it tight (it enters two products and is
//        the next addition's x: u2 - x3 is below 10 p, its square below 100 p^2 < 169 p^2 -- no reduction);
//   y3 = r (qq - x3) - s1 ppp: 4 p 10 p + 2 p 2 p = 44 p^2.
template <int VU>
ZK_HD void g1x29_add_tail(G1X29 &acc, const Lz<1, 1, VU> &p, const Lz<1, 1, 4> &r, const Lz<0, 1, VU - 2> &u1, const LqT &s1, const LqT &zz, const LqT &zzz) {
  // in the order that lets every operand die as early as possible (pp after three uses, the old zz, p, u1, zzz after one)
  const LqT pp = lq_sqr(p);
  acc.zz = lq_mul(zz, pp);
  const LqT ppp = lq_mul(p, pp);
  const LqT qq = lq_mul(u1, pp);
  acc.zzz = lq_mul(zzz, ppp);
  const LqX x3 = lz_norm(lz_sub(lz_sub(lz_sub(lq_sqr(r), ppp), qq), qq));
  acc.y = lq_mul2(r, lz_sub(qq, x3), lz_neg(s1), ppp);
  acc.x = x3;
}

// acc += (neg ? -q : q), q affine canonical.  The sign of the entry goes into q.y limb by limb (no multiple of p, no carries).
ZK_HD void g1x29_add_affine(G1X29 &acc, const G1A29 &q, bool neg) {
  constexpr u32 ONE[9] = ZK_Q29_ONE;
  if (q.is_identity()) return;
  const Lz<0, 1, 1> qx = lz_from_f29<1>(q.x);
  const Lz<1, 1, 1> qy = lz_cneg(lz_from_f29<1>(q.y), neg);
  if (acc.is_identity()) {
    acc.x = lz_widen<0, 1, 8>(qx);
    acc.y = lz_widen<0, 1, 2>(lz_norm(qy));
    acc.zz = lz_from_f29<2>(f29_const(ONE));
    acc.zzz = acc.zz;
    return;
  }
  const LqT u2 = lq_mul(qx, acc.zz);
  const LqT s2 = lq_mul(qy, acc.zzz);
  const Lz<1, 1, 10> p = lz_sub(u2, acc.x);
  const Lz<1, 1, 4> r = lz_sub(s2, acc.y);
  if (lq_is_zero_mod_p(p)) {
    if (lq_is_zero_mod_p(r)) acc = g1x29_from_affine_dbl(qx, qy);
    else acc = G1X29::identity();
    return;
  }
  g1x29_add_tail(acc, p, r, acc.x, acc.y, acc.zz, acc.zzz);
}

// acc += q, both XYZZ
ZK_HD void g1x29_add(G1X29 &acc, const G1X29 &q) {
  if (q.is_identity()) return;
  if (acc.is_identity()) {
    acc = q;
    return;
  }
  const LqT u1 = lq_mul(acc.x, q.zz);   // 8 p 2 p
  const LqT u2 = lq_mul(q.x, acc.zz);
  const LqT s1 = lq_mul(acc.y, q.zzz);
  const LqT s2 = lq_mul(q.y, acc.zzz);
  const Lz<1, 1, 4> p = lz_sub(u2, u1);
  const Lz<1, 1, 4> r = lz_sub(s2, s1);
  if (lq_is_zero_mod_p(p)) {
    if (lq_is_zero_mod_p(r)) acc = g1x29_dbl(acc);
    else acc = G1X29::identity();
    return;
  }
  const LqT zz = lq_mul(acc.zz, q.zz);
  const LqT zzz = lq_mul(acc.zzz, q.zzz);
  g1x29_add_tail(acc, p, r, u1, s1, zz, zzz);
}

// XYZZ in the 2^261 form -> the library's standard XYZZ (canonical coordinates, Montgomery with 2^256)
ZK_HD G1X g1x29_to_std(const G1X29 &p) {
  constexpr u32 K[9] = ZK_Q29_R256;
  if (p.is_identity()) return G1X::identity();
  const Lz<0, 1, 1> k = lz_from_f29<1>(f29_const(K));
  G1X r;
  r.x = lq_pack_canonical(lq_mul(p.x, k));
  r.y = lq_pack_canonical(lq_mul(p.y, k));
  r.zz = lq_pack_canonical(lq_mul(p.zz, k));
  r.zzz = lq_pack_canonical(lq_mul(p.zzz, k));
  return r;
}
// standard affine point (canonical, 2^256 form) -> packed affine in the 2^261 form (what the MSM tables hold): x * 32
ZK_HD G1Affine g1_affine_to_29(const G1Affine &p) {
  if (p.is_identity()) return p;
  Fq c = Fq::zero();
  c.l[0] = 32;
  const Fq k = fp_to_mont<FqP>(c);
  G1Affine r;
  r.x = p.x * k;
  r.y = p.y * k;
  return r;
}

}  // namespace zk
