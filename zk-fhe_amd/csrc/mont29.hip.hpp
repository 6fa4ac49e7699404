// The nine-limb, radix-2^29 product-scanning Montgomery multiply (R' = 2^261) that every 29-bit field function rests on: f29_ / fr29_
// mul, sqr, mul2 (f29_field.inc), lq_mul, lq_sqr, lq_mul2 (fq29.hip.hpp) and lz_mul, lz_mul2, lz_mul4u (lz29.hip.hpp) are typed wrappers
// of what is here, and keep the bounds they need and give next to them.
//
// A column of a * b + m * p adds up in ONE 64-bit accumulator with no carry-out; after column k < 9 the step m_k = (low word * inv) mod 2^29
// makes the low 29 bits zero, after column k >= 9 they are limb k - 9 of the result.  Two forms:
//   * mont29_c: the C body -- the host pass, the native CPU checks and -DZK_MAD_C (ZKFHE_EXTRA_FLAGS), and lz_mul4u everywhere;
//   * mont29u_* / mont29i_* (mont29_tied.inc, written by tools/gen_tied_products.py): ON THE DEVICE the products are generated inline
//     assembly since round 6, one asm statement per COLUMN on the running accumulator.  Left to the compiler, `acc += (u64)a * b` after
//     the shift by 29 is reassociated so that the previous column's carry is added last: every column starts in a register pair of its own and
//     a v_lshl_add_u64 joins it to the carry -- 17 of a product's ~240 instructions, up to eleven accumulator pairs in flight.  Tied to one
//     pair the joins go (k_msm_table's addition loop: 277 -> 39; k_ntt13: 246 -> 220 VGPRs).  One statement per multiply-add was tried first
//     and lost: the compiler cannot see into an asm statement and puts a wait state before every VALU read of a register one defines (~150
//     s_nop per product); inside ONE statement it inserts nothing, and the step m_k between two statements costs one wait state per column.
//     Measured (profiles/r6_probes.md section 2): k_msm_table -6 %, k_msm_accumulate -3..4 %, k_ntt13 unchanged, the driver's wave +4.5 %,
//     96 steps +4 %, one proof alone -2 % (faster), bit-exact.
// Both are exact integer arithmetic: the order of a column's terms does not matter, the results are bit-identical.
#pragma once
#include "bn254.hip.hpp"

namespace zk {
namespace q29 {
constexpr u32 MASK = (1u << 29) - 1;   // of a limb, whatever the modulus
}

// one product term a_j b_i of a column.  SQR (b is a): the cross products once, against the doubled limb 2 a_i
template <bool SQR, class Acc, class Limb, class A, class B>
ZK_HD void mont29_term(Acc &acc, const A &a, const B &b, int j, int i) {
  if (SQR && j > i) return;
  const Limb y = (Limb)b.l[i];
  acc += (Acc)(Limb)a.l[j] * (Acc)(SQR && j < i ? y * 2 : y);
}
template <bool SQR, class Acc, class Limb>
ZK_HD void mont29_terms(Acc &, int, int) {}
template <bool SQR, class Acc, class Limb, class A, class B, class... Rest>
ZK_HD void mont29_terms(Acc &acc, int j, int i, const A &a, const B &b, const Rest &...rest) {
  mont29_term<SQR, Acc, Limb>(acc, a, b, j, i);
  mont29_terms<SQR, Acc, Limb>(acc, j, i, rest...);
}

// (a0 b0 + a1 b1 + ...) / 2^261 mod p for the operand pairs a0, b0, a1, b1, ... (one, two or four pairs; SQR: one pair a, a).
// M: the modulus (INV = -p^-1 mod 2^29, P[9]); Acc, Limb: u64, u32 or long long, int; R: the result type (limbs 0..7 in [0, 2^29), the
// top limb what is left).  The caller's bounds keep every column sum inside Acc.
template <class M, class Acc, class Limb, class R, bool SQR = false, class... Ops>
ZK_HD R mont29_c(const Ops &...ops) {
  Limb m[9];
  R r;
  Acc acc = 0;
#pragma unroll
  for (int k = 0; k < 17; ++k) {
#pragma unroll
    for (int j = (k < 9 ? 0 : k - 8); j <= (k < 9 ? k : 8); ++j) {
      mont29_terms<SQR, Acc, Limb>(acc, j, k - j, ops...);
      if (j < k) acc += (Acc)m[j] * (Acc)(Limb)M::P[k - j];
    }
    if (k < 9) {
      m[k] = (Limb)(((u32)acc * M::INV) & q29::MASK);
      acc += (Acc)m[k] * (Acc)(Limb)M::P[0];
    } else {
      r.l[k - 9] = (Limb)((u32)acc & q29::MASK);
    }
    acc >>= 29;   // exact for k < 9 (the low 29 bits are zero); arithmetic for a signed Acc: floor
  }
  r.l[8] = (Limb)acc;
  return r;
}

#if defined(__HIP_DEVICE_COMPILE__) && !defined(ZK_MAD_C)
#define ZK_MONT29_TIED 1
#define MONT29_FN(name) mont29u_##name
#define MONT29_MAD "v_mad_u64_u32"
#define MONT29_SHR "v_lshrrev_b64"
#define MONT29_ACC u64
#define MONT29_LIMB u32
#include "mont29_tied.inc"
#undef MONT29_FN
#undef MONT29_MAD
#undef MONT29_SHR
#undef MONT29_ACC
#undef MONT29_LIMB
#define MONT29_FN(name) mont29i_##name
#define MONT29_MAD "v_mad_i64_i32"
#define MONT29_SHR "v_ashrrev_i64"
#define MONT29_ACC long long
#define MONT29_LIMB int
#include "mont29_tied.inc"
#undef MONT29_FN
#undef MONT29_MAD
#undef MONT29_SHR
#undef MONT29_ACC
#undef MONT29_LIMB
#endif

}  // namespace zk
