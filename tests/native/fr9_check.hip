// Host-side check of csrc/fr9.hip.hpp (the register-resident nine-limb Fr value of the quotient, lookup, scan and batch-inversion
// kernels) against the standard 8 x 32-bit Fr arithmetic of bn254.hip.hpp: both loads, the register-level regrouping, the products at
// the extreme members of every bound they declare, the canonical store, and the expressions as the kernels compose them
// (v + b s + g, z1 A - z0 B, the Horner step, the inversion chains) on random operands and on every combination of the edge
// operands 0, 1, r - 1, r - 2, 2^253, 2^253 - 1 and the limb-wise largest canonical value.
// Prints `fr9: N bad` (random operands) and `fr9 edges: N bad`.
#include "fr9.hip.hpp"
#include <cstdio>
#include <random>
using namespace zk;

static std::mt19937_64 rng(99);
static Fr rand_fr() {
  Fr a;
  for (;;) {
    for (int i = 0; i < 8; ++i) a.l[i] = (u32)rng();
    a.l[7] &= 0x3fffffff;
    bool lt = false;
    for (int i = 7; i >= 0; --i) {
      if (a.l[i] != FrP::MOD[i]) { lt = a.l[i] < FrP::MOD[i]; break; }
    }
    if (lt) return a;
  }
}
static bool eq(const Fr &a, const Fr &b) {
  for (int i = 0; i < 8; ++i) if (a.l[i] != b.l[i]) return false;
  return true;
}
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)
static Fr small(u32 v) { Fr a = Fr::zero(); a.l[0] = v; return a; }
static Fr times32(Fr a) { for (int i = 0; i < 5; ++i) a = fp_dbl<FrP>(a); return a; }
// sum l[i] 2^(29 i) mod r, canonical, for limbs of either sign: Horner's rule in the standard arithmetic, independent of the code under test
static Fr val9(const long long (&l)[9]) {
  Fr acc = Fr::zero();
  for (int i = 8; i >= 0; --i) {
    for (int k = 0; k < 29; ++k) acc = fp_dbl<FrP>(acc);
    const long long v = l[i];
    const Fr lo = small((u32)((v < 0 ? -v : v) & 0xffff)), hi = small((u32)((v < 0 ? -v : v) >> 16));
    Fr t = hi;
    for (int k = 0; k < 16; ++k) t = fp_dbl<FrP>(t);
    t = fp_add<FrP>(t, lo);
    acc = v < 0 ? fp_sub<FrP>(acc, t) : fp_add<FrP>(acc, t);
  }
  return acc;
}
template <int LO, int HI, int V>
static Fr val(const Lz<LO, HI, V> &a) {
  long long l[9];
  for (int i = 0; i < 9; ++i) l[i] = a.l[i];
  return val9(l);
}
// the limbs inside what the type declares; the top limb below 2^29 in magnitude, as a product's operand needs it, and inside |value| < V r
template <int LO, int HI, int V>
static bool limbs_ok(const Lz<LO, HI, V> &a) {
  for (int i = 0; i < 8; ++i)
    if (!((long long)a.l[i] > -(long long)LO * (1ll << 29) - (LO == 0) && (long long)a.l[i] < (long long)HI * (1ll << 29) + (HI == 0))) return false;
  const long long top = a.l[8];
  return top > -(long long)(V + 1) * (1ll << 22) && top < (long long)(V + 1) * (1ll << 22) && top > -(1ll << 29) && top < (1ll << 29);
}
// the extreme member of a bound: every lower limb at the edge of its range on the given side, the top limb as large as |value| < V r lets it be
template <int LO, int HI, int V>
static Lz<LO, HI, V> extreme(bool negative) {
  Lz<LO, HI, V> r;
  const u32 P[9] = ZK_R29_P;
  if (negative && LO == 0) {
    for (int i = 0; i < 8; ++i) r.l[i] = 0;
    r.l[8] = -(int)(V * P[8]);
    return r;
  }
  for (int i = 0; i < 8; ++i) r.l[i] = negative ? -LO * ((1 << 29) - 1) : HI * ((1 << 29) - 1);
  const int room = (int)(V * P[8]) - (LO > HI ? LO : HI) - 1;
  r.l[8] = negative ? -room : room;
  return r;
}
static Fr r_minus(u32 k) {
  Fr a;
  for (int i = 0; i < 8; ++i) a.l[i] = FrP::MOD[i];
  a.l[0] -= k;
  return a;
}
static Fr pow2(int e) { Fr a = Fr::zero(); a.l[e >> 5] = 1u << (e & 31); return a; }
static Fr largest_limbwise() {   // limbs 0..7 all ones, the top limb one below the modulus's: canonical, packed
  const u32 P[9] = ZK_R29_P;
  F29 w;
  for (int i = 0; i < 8; ++i) w.l[i] = q29::MASK;
  w.l[8] = P[8] - 1;
  return fr29_pack(w);
}

// a product's result: limbs tight, the value inside what its type says, the residue right, the store canonical
template <class A, class B>
static void check_mul(const A &a, const B &b, const char *what, int it) {
  CHECK(limbs_ok(a) && limbs_ok(b), "%s: the test's own operands leave their declared bound at %d", what, it);
  const auto r = fr9_mul(a, b);
  CHECK(limbs_ok(r), "%s: result outside its type at %d", what, it);
  CHECK(eq(times32(val(r)), fp_mul<FrP>(val(a), val(b))), "%s mismatch at %d", what, it);
  CHECK(eq(fr9_store(r), val(r)), "%s: store mismatch at %d", what, it);
}
template <class A>
static void check_sqr(const A &a, const char *what, int it) {
  CHECK(limbs_ok(a), "%s: the test's own operand leaves its declared bound at %d", what, it);
  const auto r = fr9_sqr(a);
  CHECK(limbs_ok(r) && r.l[8] >= 0, "%s: result outside its type at %d", what, it);
  CHECK(eq(times32(val(r)), fp_mul<FrP>(val(a), val(a))), "%s mismatch at %d", what, it);
  CHECK(eq(fr9_store(r), val(r)), "%s: store mismatch at %d", what, it);
}
template <class A, class B, class C, class D>
static void check_mul2(const A &a, const B &b, const C &c, const D &d, const char *what, int it) {
  CHECK(limbs_ok(a) && limbs_ok(b) && limbs_ok(c) && limbs_ok(d), "%s: the test's own operands leave their declared bound at %d", what, it);
  const auto r = fr9_mul2(a, b, c, d);
  CHECK(limbs_ok(r), "%s: result outside its type at %d", what, it);
  CHECK(eq(times32(val(r)), fp_add<FrP>(fp_mul<FrP>(val(a), val(b)), fp_mul<FrP>(val(c), val(d)))), "%s mismatch at %d", what, it);
  CHECK(eq(fr9_store(r), val(r)), "%s: store mismatch at %d", what, it);
}

static void bound_checks() {
  for (int s = 0; s < 2; ++s)
    for (int t = 0; t < 2; ++t) {
      const int it = s * 2 + t;
      // fr9_mul: the limb bounds multiply to 2, V1 V2 <= 338, V <= 127
      check_mul(extreme<2, 2, 2>(s), extreme<1, 1, 127>(t), "mul (2,2) 2 r x (1,1) 127 r", it);
      check_mul(extreme<1, 1, 127>(s), extreme<2, 2, 2>(t), "mul (1,1) 127 r x (2,2) 2 r", it);
      check_mul(extreme<2, 2, 5>(s), extreme<0, 1, 66>(t), "mul (2,2) 5 r x (0,1) 66 r", it);
      check_mul(extreme<1, 2, 18>(s), extreme<1, 1, 18>(t), "mul (1,2) 18 r x (1,1) 18 r", it);
      check_mul(extreme<0, 2, 2>(s), extreme<0, 1, 64>(t), "mul (0,2) 2 r x (0,1) 64 r: the lookup term", it);
      check_mul(extreme<0, 1, 3>(s), extreme<0, 1, 66>(t), "mul 3 r x 66 r: the permutation step", it);
      check_mul(extreme<0, 1, 3>(s), extreme<0, 1, 32>(t), "mul 3 r x 32 r", it);
      check_mul(extreme<0, 1, 2>(s), extreme<0, 1, 32>(t), "mul 2 r x 32 r", it);
      check_mul(extreme<1, 1, 64>(s), extreme<1, 1, 2>(t), "mul (1,1) 64 r x (1,1) 2 r", it);
      check_mul(extreme<0, 1, 32>(s), extreme<0, 1, 1>(t), "mul 32 r x r: fr9_cc", it);
      check_mul(extreme<0, 1, 1>(s), extreme<0, 1, 96>(t), "mul r x 96 r", it);
      // fr9_mul2: limbs below 2^29, the sum of the two bounds <= 338
      check_mul2(extreme<0, 1, 3>(s), extreme<0, 1, 32>(t), extreme<0, 1, 32>(s), extreme<1, 1, 6>(t), "mul2 Horner step of PERM_D", it);
      check_mul2(extreme<0, 1, 3>(s), extreme<0, 1, 32>(t), extreme<0, 1, 32>(t), extreme<1, 1, 6>(s), "mul2 Horner step of PERM_D, crossed signs", it);
      check_mul2(extreme<1, 1, 13>(s), extreme<1, 1, 13>(t), extreme<1, 1, 13>(s), extreme<1, 1, 13>(t), "mul2 13 r four times", it);
      check_mul2(extreme<1, 1, 13>(s), extreme<1, 1, 13>(t), extreme<1, 1, 13>(!s), extreme<1, 1, 13>(t), "mul2 13 r four times, cancelling", it);
      check_mul2(extreme<1, 1, 127>(s), extreme<1, 1, 1>(t), extreme<1, 1, 1>(s), extreme<1, 1, 127>(t), "mul2 127 r x r twice", it);
      check_mul2(extreme<0, 1, 32>(s), extreme<0, 1, 2>(t), extreme<0, 1, 32>(s), extreme<1, 0, 2>(t), "mul2 z1 A - z0 B", it);
    }
  for (int s = 0; s < 2; ++s) {
    check_sqr(extreme<1, 1, 18>(s), "sqr (1,1) 18 r", s);
    check_sqr(extreme<0, 1, 1>(s), "sqr r", s);
    // the regrouping by five bits: 32 a, tight limbs, a top limb below 2^29
    const auto e3 = extreme<0, 1, 3>(s);
    const auto e2 = extreme<0, 1, 2>(s);
    CHECK(limbs_ok(fr9_times32(e3)) && eq(val(fr9_times32(e3)), times32(val(e3))), "times32 at 3 r, sign %d", s);
    CHECK(limbs_ok(fr9_times32(e2)) && eq(val(fr9_times32(e2)), times32(val(e2))), "times32 at 2 r, sign %d", s);
    check_mul(extreme<0, 1, 1>(s), fr9_times32(e3), "mul r x times32(3 r)", s);
    // the store at the widest value the kernels reach (differences of running products: 6 r)
    CHECK(eq(fr9_store(extreme<1, 1, 6>(s)), val(extreme<1, 1, 6>(s))), "store (1,1) 6 r, sign %d", s);
    CHECK(eq(fr9_store(extreme<0, 1, 3>(s)), val(extreme<0, 1, 3>(s))), "store 3 r, sign %d", s);
  }
}

// the expressions as the kernels write them, against the standard arithmetic
static void check_expressions(const Fr &a, const Fr &b, const Fr &c, const Fr &d, const Fr &e, int it) {
  // loads
  const Fr9S A = fr9_load(a);
  const Fr9C A32 = fr9_load32(a);
  CHECK(limbs_ok(A) && eq(val(A), a), "load mismatch at %d", it);
  CHECK(limbs_ok(A32) && eq(val(A32), times32(a)), "load32 mismatch at %d", it);
  bool same = true;
  const auto A32r = fr9_times32(A);
  for (int i = 0; i < 9; ++i) same = same && A32r.l[i] == A32.l[i];
  CHECK(same, "times32(load) is not load32 at %d", it);
  CHECK(eq(fr9_store(A), a), "store(load) mismatch at %d", it);
  // products
  CHECK(eq(fr9_store(fr9_mul(A, fr9_load32(b))), fp_mul<FrP>(a, b)), "mul mismatch at %d", it);
  CHECK(eq(fr9_store(fr9_cc(fr9_sqr(A))), fp_sqr<FrP>(a)), "sqr mismatch at %d", it);
  CHECK(eq(fr9_store(fr9_mul2(A, fr9_load32(b), fr9_load32(c), fr9_load(d))), fp_mul2<FrP>(a, b, c, d)), "mul2 mismatch at %d", it);
  CHECK(eq(fr9_store(fr9_mul(fr9_load(c), fr9_times32(fr9_mul(A, fr9_load32(b))))), fp_mul<FrP>(fp_mul<FrP>(a, b), c)), "regrouped chain mismatch at %d", it);
  // v + b s + g and a step of the running product: a (b + c d + e)
  const auto f = fr9_perm_factor(fr9_load32(b), fr9_mul(fr9_load(d), fr9_cc(fr9_load32(c))), fr9_load32(e));
  const Fr fw = fp_add<FrP>(fp_add<FrP>(b, fp_mul<FrP>(c, d)), e);
  CHECK(limbs_ok(f) && eq(val(f), times32(fw)), "permutation factor mismatch at %d", it);
  CHECK(eq(fr9_store(fr9_perm_step(A, f)), fp_mul<FrP>(a, fw)), "permutation step mismatch at %d", it);
  // (a + b)(c + d), and z1 A - z0 B with z1 = e, z0 = a
  const auto t1 = fr9_lookup_term(A, fr9_load(b), fr9_lookup_sum(fr9_load32(c), fr9_load32(d)));
  const Fr t1w = fp_mul<FrP>(fp_add<FrP>(a, b), fp_add<FrP>(c, d));
  CHECK(eq(fr9_store(t1), t1w), "lookup term mismatch at %d", it);
  const auto t2 = fr9_lookup_term(fr9_load(d), fr9_load(b), fr9_lookup_sum(fr9_load32(e), fr9_load32(c)));
  const Fr t2w = fp_mul<FrP>(fp_add<FrP>(d, b), fp_add<FrP>(e, c));
  CHECK(eq(fr9_store(fr9_mul2(fr9_load32(e), t1, fr9_load32(a), lz_neg(t2))), fp_mul2<FrP>(e, t1w, fp_neg<FrP>(a), t2w)), "z1 A - z0 B mismatch at %d", it);
  // the quotient's Horner steps: acc y + u v with differences and products as v, acc kept in limbs
  Lz<0, 1, 3> acc = lz_widen<0, 1, 3>(fr9_mul(fr9_load32(c), lz_sub(fr9_one(), A)));
  Fr accw = fp_mul<FrP>(c, fp_sub<FrP>(Fr::one(), a));
  const Fr9C y = fr9_load32(e);
  acc = lz_widen<0, 1, 3>(fr9_mul2(acc, y, fr9_load32(b), lz_sub(fr9_mul(A, A32), A)));
  accw = fp_mul2<FrP>(accw, e, b, fp_sub<FrP>(fp_mul<FrP>(a, a), a));
  acc = lz_widen<0, 1, 3>(fr9_mul2(acc, y, fr9_load32(d), fr9_norm(lz_sub(lz_add(A, fr9_mul(fr9_load(b), fr9_load32(c))), fr9_load(d)))));
  accw = fp_mul2<FrP>(accw, e, d, fp_sub<FrP>(fp_add<FrP>(a, fp_mul<FrP>(b, c)), d));
  acc = lz_widen<0, 1, 3>(fr9_mul(acc, y));
  accw = fp_mul<FrP>(accw, e);
  // running products of six factors each and the Horner step over their difference
  Lz<0, 1, 3> left = lz_widen<0, 1, 3>(A), right = lz_widen<0, 1, 3>(fr9_load(b));
  Fr leftw = a, rightw = b;
  const Fr in[5] = {a, b, c, d, e};
  const auto beta = fr9_cc(fr9_load32(c)), x = fr9_cc(fr9_load32(d));
  for (int k = 0; k < 6; ++k) {
    const Fr v = in[k % 5], sg = in[(k + 2) % 5], bd = in[(k + 3) % 5];
    left = fr9_perm_step(left, fr9_perm_factor(fr9_load32(v), fr9_mul(fr9_load(sg), beta), fr9_load32(e)));
    right = fr9_perm_step(right, fr9_perm_factor(fr9_load32(v), fr9_mul(fr9_load(bd), x), fr9_load32(e)));
    leftw = fp_mul<FrP>(leftw, fp_add<FrP>(fp_add<FrP>(v, fp_mul<FrP>(c, sg)), e));
    rightw = fp_mul<FrP>(rightw, fp_add<FrP>(fp_add<FrP>(v, fp_mul<FrP>(bd, d)), e));
    CHECK(limbs_ok(left) && limbs_ok(right), "running product outside its type at %d step %d", it, k);
  }
  acc = lz_widen<0, 1, 3>(fr9_mul2(acc, y, fr9_load32(b), lz_sub(left, right)));
  accw = fp_mul2<FrP>(accw, e, b, fp_sub<FrP>(leftw, rightw));
  CHECK(limbs_ok(acc) && eq(fr9_store(acc), accw), "Horner chain mismatch at %d", it);
  // the inversion's chains: a prefix product whose every state is stored, the backward pass from the inverse
  Lz<0, 1, 2> p = lz_widen<0, 1, 2>(fr9_one());
  Fr pw = Fr::one(), tmp[5];
  for (int k = 0; k < 5; ++k) {
    tmp[k] = fr9_store(p);
    CHECK(eq(tmp[k], pw), "prefix state mismatch at %d step %d", it, k);
    if (!in[k].is_zero()) p = fr9_mul(p, fr9_load32(in[k])), pw = fp_mul<FrP>(pw, in[k]);
  }
  p = lz_widen<0, 1, 2>(fr9_load(fp_inv<FrP>(fr9_store(p))));
  for (int k = 4; k >= 0; --k) {
    if (in[k].is_zero()) continue;
    const auto inv = fr9_mul(p, fr9_load32(tmp[k]));
    p = fr9_mul(p, fr9_load32(in[k]));
    CHECK(eq(fr9_store(inv), fp_inv<FrP>(in[k])), "inverse mismatch at %d element %d", it, k);
    CHECK(eq(fr9_store(fr9_mul(inv, fr9_load32(in[(k + 1) % 5]))), fp_mul<FrP>(in[(k + 1) % 5], fp_inv<FrP>(in[k]))), "quotient mismatch at %d element %d", it, k);
  }
}

int main() {
  for (int it = 0; it < 20000; ++it) check_expressions(rand_fr(), rand_fr(), rand_fr(), rand_fr(), rand_fr(), it);
  printf("fr9: %d bad\n", bad);
  const int random_bad = bad;
  bad = 0;
  bound_checks();
  Fr edge[7] = {Fr::zero(), small(1), r_minus(1), r_minus(2), pow2(253), pow2(253), largest_limbwise()};
  edge[5].l[7] -= 1;   // 2^253 - 1
  for (int i = 0; i < 7; ++i) edge[5].l[i] = 0xffffffffu;
  int it = 0;
  for (int i0 = 0; i0 < 7; ++i0)
    for (int i1 = 0; i1 < 7; ++i1)
      for (int i2 = 0; i2 < 7; ++i2)
        for (int i3 = 0; i3 < 7; ++i3)
          for (int i4 = 0; i4 < 7; ++i4) check_expressions(edge[i0], edge[i1], edge[i2], edge[i3], edge[i4], it++);
  printf("fr9 edges: %d bad\n", bad);
  return random_bad != 0 || bad != 0;
}
