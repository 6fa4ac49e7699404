// Modulus-dependent part of the radix-2^29 field arithmetic (see fq29.hip.hpp): included once per field with
//   F29_FN(name)  -> the function name (f29_##name for Fq, fr29_##name for Fr)
//   F29_P, F29_2P, F29_3P  -> limb initialisers of p, 2p, 3p;  F29_INV -> -p^-1 mod 2^29
// Both BN254 moduli have floor(2^261 / p) = 169, which f29_weak_reduce relies on.
// Gives F29_FN(mod) too: the modulus in the form the nine-limb products of mont29.hip.hpp take it.
// value < 16 p  ->  the same residue below 2 p (in fact below 1.03 p): q = floor(v / 2^245) * 169 >> 16 underestimates v / p by
// less than one (169 = floor(2^261 / p))
ZK_HD F29 F29_FN(weak_reduce)(const F29 &a) {
  const u32 P[9] = F29_P;
  const u32 q = ((a.l[8] >> 13) * 169u) >> 16;
  F29 r;
  long long c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const long long v = (long long)a.l[i] - (long long)((u64)q * P[i]) + c;
    r.l[i] = (u32)v & q29::MASK;
    c = v >> 29;
  }
  r.l[8] = (u32)((long long)a.l[8] - (long long)((u64)q * P[8]) + c);
  return r;
}
// value < 4 p -> canonical (< p)
ZK_HD F29 F29_FN(canonical)(const F29 &a) {
  const u32 P[9] = F29_P;
  F29 r = F29_FN(weak_reduce)(a);  // < 2 p
  int t[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) t[i] = (int)r.l[i] - (int)P[i];
  // r - p: negative iff the propagated top limb is negative
  int c = 0;
  u32 o[9];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int v = t[i] + c;
    o[i] = (u32)v & q29::MASK;
    c = v >> 29;
  }
  const int top = t[8] + c;
  o[8] = (u32)top;
  if (top >= 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = o[i];
  }
  return r;
}
// value in (0, 4 p): is it 0 mod p?  (differences u2 - u1 + 2p of two representatives below 2 p)
ZK_HD bool F29_FN(is_zero_mod_p)(const F29 &a) {
  const u32 P1[9] = F29_P, P2[9] = F29_2P, P3[9] = F29_3P;
  if (a.l[0] != P1[0] && a.l[0] != P2[0] && a.l[0] != P3[0]) return false;  // almost always
  return f29_eq(a, P1) || f29_eq(a, P2) || f29_eq(a, P3);
}

// the modulus as the nine-limb products take it (mont29.hip.hpp); lq_ and lz_ products use it too
struct F29_FN(mod) {
  static constexpr u32 INV = F29_INV;
  static constexpr u32 P[9] = F29_P;
};
// Montgomery product a b / 2^261 mod p.  Needs a * b < 2^261 p (e.g. both below 11 p); gives a value below 2 p.
ZK_HD F29 F29_FN(mul)(const F29 &a, const F29 &b) {
#ifdef ZK_MONT29_TIED
  return mont29u_mul_v<F29_FN(mod), F29>(a, b);
#else
  return mont29_c<F29_FN(mod), u64, u32, F29>(a, b);
#endif
}
// a^2 / 2^261 mod p: the cross products a_j a_i (j < i) once, against the doubled limb 2 a_i -- 45 product multiply-adds
// instead of 81 (column sums stay below 2^63: four doubled terms below 2^59, one square and nine reduction terms below 2^58).
ZK_HD F29 F29_FN(sqr)(const F29 &a) {
#ifdef ZK_MONT29_TIED
  return mont29u_sqr<F29_FN(mod), F29>(a);
#else
  return mont29_c<F29_FN(mod), u64, u32, F29, true>(a, a);
#endif
}
// (a b + c d) / 2^261 mod p with one reduction.  Needs a b + c d < 2^261 p; gives a value below 2 p.
ZK_HD F29 F29_FN(mul2)(const F29 &a, const F29 &b, const F29 &c, const F29 &d) {
#ifdef ZK_MONT29_TIED
  return mont29u_mul2<F29_FN(mod), F29>(a, b, c, d);
#else
  return mont29_c<F29_FN(mod), u64, u32, F29>(a, b, c, d);
#endif
}
