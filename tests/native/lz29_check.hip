// Host-side check of csrc/lz29.hip.hpp (signed lazy radix-2^29 values of the 2^13 NTT tile) against the standard 8 x 32-bit Fr
// arithmetic of bn254.hip.hpp: products with loose signed operands, the fused two-product form, carry propagation, the weak
// reduction of values of either sign up to 16 r, and the canonical store -- on the radix-8 butterfly network of ntt13.hip.
// Random operands first (`lz29: N bad`), then the largest operands each declared bound admits, both signs, against the largest
// canonical twiddle, r - 1 and random twiddles, and every multiple of r a weak reduction can meet (`lz29 edges: N bad`).
#include "lz29.hip.hpp"
#include <cstdio>
#include <random>
using namespace zk;

static std::mt19937_64 rng(77);
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
// the integer a stored value stands for, as a standard field element: a column value is x 2^256 as is; a product against a
// twiddle w 2^261 is x w 2^256 again
static Lw tw_of(const Fr &w) { return lw_unpack(zk_fr_to_29(w)); }

// ---- the largest operands each declared bound admits (tests/native/lq29_check.hip has the same for Fq) ----------------------------
static int edge_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (edge_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)
static Fr small(u32 v) { Fr a = Fr::zero(); a.l[0] = v; return a; }
static Fr times32(Fr a) { for (int i = 0; i < 5; ++i) a = fp_dbl<FrP>(a); return a; }
// sum l[i] 2^(29 i) mod r, canonical, for limbs of either sign: Horner's rule in the standard arithmetic, independent of the code under test
static Fr val9(const long long (&l)[9]) {
  Fr acc = Fr::zero();
  for (int i = 8; i >= 0; --i) {
    for (int k = 0; k < 29; ++k) acc = fp_dbl<FrP>(acc);
    const long long v = l[i];
    const Fr lo = small((u32)((v < 0 ? -v : v) & 0xffff)), hi = small((u32)((v < 0 ? -v : v) >> 16));   // |v| < 2^32 in two halves below r
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
static Fr val(const Lw &a) {
  long long l[9];
  for (int i = 0; i < 9; ++i) l[i] = a.l[i];
  return val9(l);
}
// the limbs inside what the type declares: -LO 2^29 < l[i] < HI 2^29, a side typed 0 admitting 0 itself (lz_neg of non-negative limbs is typed HI = 0)
template <int LO, int HI, int V>
static bool limbs_ok(const Lz<LO, HI, V> &a) {
  for (int i = 0; i < 8; ++i)
    if (!((long long)a.l[i] > -(long long)LO * (1ll << 29) - (LO == 0) && (long long)a.l[i] < (long long)HI * (1ll << 29) + (HI == 0))) return false;
  const long long top = a.l[8];
  return top > -(long long)(V + 1) * (1ll << 22) && top < (long long)(V + 1) * (1ll << 22);
}
// the extreme member of a bound: every lower limb at the edge of its range on the given side, the top limb as large as |value| < V r lets it be
template <int LO, int HI, int V>
static Lz<LO, HI, V> extreme(bool negative) {
  Lz<LO, HI, V> r;
  const u32 P[9] = ZK_R29_P;
  if (negative && LO == 0) {   // non-negative limbs, negative value: the lower limbs at zero
    for (int i = 0; i < 8; ++i) r.l[i] = 0;
    r.l[8] = -(int)(V * P[8]);
    return r;
  }
  for (int i = 0; i < 8; ++i) r.l[i] = negative ? -LO * ((1 << 29) - 1) : HI * ((1 << 29) - 1);   // a limb typed h is a sum of h terms below 2^29
  const int room = (int)(V * P[8]) - (LO > HI ? LO : HI) - 1;
  r.l[8] = negative ? -room : room;
  return r;
}
// k r + d with tight limbs 0..7 and a signed top limb (|k| <= 15, d in {-1, 0, 1}: the -1 of k = 0 borrows through every limb)
static Lz<0, 1, 16> multiple_of_r(int k, int d) {
  const u32 P[9] = ZK_R29_P;
  Lz<0, 1, 16> r;
  long long c = d;
  for (int i = 0; i < 9; ++i) {
    const long long v = (long long)k * (long long)P[i] + c;
    r.l[i] = i < 8 ? (int)(v & (long long)q29::MASK) : (int)v;
    c = v >> 29;
  }
  return r;
}
static Lw largest_twiddle() {   // limb-wise the largest canonical constant: limbs 0..7 all ones, the top limb one below the modulus's
  const u32 P[9] = ZK_R29_P;
  Lw w;
  for (int i = 0; i < 8; ++i) w.l[i] = q29::MASK;
  w.l[8] = P[8] - 1;
  return w;
}
static Fr r_minus_1() {
  Fr a;
  for (int i = 0; i < 8; ++i) a.l[i] = FrP::MOD[i];
  a.l[0] -= 1;
  return a;
}
static bool tight(const LzT &a) {   // what a product promises: limbs 0..7 in [0, 2^29), value in (-r, 2 r)
  const u32 P[9] = ZK_R29_P;
  for (int i = 0; i < 8; ++i) if (a.l[i] < 0 || a.l[i] > (int)q29::MASK) return false;
  return a.l[8] >= -(int)P[8] - 1 && a.l[8] <= 2 * (int)P[8];
}
// weak reduction and stores of one value: tight non-negative limbs below 2 r, the residue kept, the store canonical
template <int LO, int HI, int V>
static void check_reduce(const Lz<LO, HI, V> &a, const char *what, int it) {
  const u32 P[9] = ZK_R29_P;
  CHECK(limbs_ok(a), "%s: the test's own operand leaves its declared bound at %d", what, it);
  const Fr want = val(a);
  const LzW w = lz_weak(a);
  CHECK(limbs_ok(w) && tight(w) && w.l[8] >= 0 && w.l[8] <= 2 * (int)P[8], "%s: weak result not tight at %d", what, it);
  CHECK(eq(val(w), want), "%s: weak changes the residue at %d", what, it);
  CHECK(eq(lz_store(a), want), "%s: store mismatch at %d", what, it);
}
template <class A>
static void check_mul(const A &a, const Lw &w, const char *what, int it) {
  CHECK(limbs_ok(a), "%s: the test's own operand leaves its declared bound at %d", what, it);
  const LzT r = lz_mul(a, w);
  CHECK(limbs_ok(r) && tight(r), "%s: result outside (-r, 2 r) or limbs not tight at %d", what, it);
  CHECK(eq(times32(val(r)), fp_mul<FrP>(val(a), val(w))), "%s mismatch at %d", what, it);
  check_reduce(r, what, it);
}
template <class A, class B>
static void check_mul2(const A &a, const Lw &w, const B &b, const Lw &v, const char *what, int it) {
  CHECK(limbs_ok(a) && limbs_ok(b), "%s: the test's own operands leave their declared bound at %d", what, it);
  const LzT r = lz_mul2(a, w, b, v);
  CHECK(limbs_ok(r) && tight(r), "%s: result outside (-r, 2 r) or limbs not tight at %d", what, it);
  CHECK(eq(times32(val(r)), fp_add<FrP>(fp_mul<FrP>(val(a), val(w)), fp_mul<FrP>(val(b), val(v)))), "%s mismatch at %d", what, it);
  check_reduce(r, what, it);
}
static void check_mul4u(const Lz<0, 1, 1> &a, const Lw &w, const Lz<0, 1, 1> &b, const Lw &v, const Lz<0, 1, 1> &c, const Lw &x, const Lz<0, 1, 1> &d, const Lw &y, int it) {
  const LzT r = lz_mul4u(a, w, b, v, c, x, d, y);
  CHECK(limbs_ok(r) && tight(r) && r.l[8] >= 0, "mul4u: result outside [0, 2 r) or limbs not tight at %d", it);
  const Fr want = fp_add<FrP>(fp_add<FrP>(fp_mul<FrP>(val(a), val(w)), fp_mul<FrP>(val(b), val(v))), fp_add<FrP>(fp_mul<FrP>(val(c), val(x)), fp_mul<FrP>(val(d), val(y))));
  CHECK(eq(times32(val(r)), want), "mul4u mismatch at %d", it);
  check_reduce(r, "mul4u", it);
}

static int edge_checks() {
  const u32 P[9] = ZK_R29_P;
  Lw tw[8];
  tw[0] = largest_twiddle();
  tw[1] = lw_unpack(r_minus_1());
  for (int i = 2; i < 8; ++i) tw[i] = tw_of(rand_fr());
  Lw w0 = tw[0], w1 = tw[0];   // the constants 0 and 1 as twiddles
  for (int i = 0; i < 9; ++i) w0.l[i] = w1.l[i] = 0;
  w1.l[0] = 1;
  Lz<0, 1, 1> big;   // the largest canonical data limb-wise
  for (int i = 0; i < 9; ++i) big.l[i] = (int)tw[0].l[i];
  const Lz<0, 1, 1> data[4] = {lz_zero(), lz_load(small(1)), lz_load(r_minus_1()), big};
  for (int t = 0; t < 8; ++t) {
    const Lw &w = tw[t];
    for (int s = 0; s < 2; ++s) {
      check_mul(extreme<2, 2, 160>(s), w, "mul extreme (2,2) 160 r", t * 2 + s);
      check_mul(extreme<1, 2, 160>(s), w, "mul extreme (1,2) 160 r", t * 2 + s);
      check_mul(extreme<2, 1, 160>(s), w, "mul extreme (2,1) 160 r", t * 2 + s);
      check_mul(extreme<2, 2, 16>(s), w, "mul extreme (2,2) 16 r", t * 2 + s);
      check_mul(extreme<1, 2, 16>(s), w, "mul extreme (1,2) 16 r", t * 2 + s);
      check_mul(extreme<2, 1, 16>(s), w, "mul extreme (2,1) 16 r", t * 2 + s);
      check_mul(extreme<0, 2, 16>(s), w, "mul extreme (0,2) 16 r", t * 2 + s);
      for (int s2 = 0; s2 < 2; ++s2)
        for (int u = 0; u < 8; ++u) check_mul2(extreme<1, 1, 80>(s), w, extreme<1, 1, 80>(s2), tw[u], "mul2 extreme 80 r twice", (t * 8 + u) * 4 + s * 2 + s2);
    }
    for (int i = 0; i < 4; ++i) {
      check_mul(data[i], w, "mul constant", t * 4 + i);
      check_mul(lz_neg(data[i]), w, "mul -constant", t * 4 + i);
      check_mul(extreme<2, 2, 160>(i & 1), i & 2 ? w1 : w0, "mul by the twiddles 0 and 1", t * 4 + i);
      check_mul2(data[i], w, data[(i + 1) & 3], tw[(t + 1) & 7], "mul2 constants", t * 4 + i);
      check_mul2(data[i], w, lz_neg(data[i]), w, "mul2 cancelling", t * 4 + i);
      check_mul4u(data[i], w, data[i], w, data[i], w, data[i], w, t * 4 + i);
      check_mul4u(data[i], w, data[(i + 1) & 3], tw[(t + 1) & 7], data[(i + 2) & 3], tw[(t + 2) & 7], data[(i + 3) & 3], tw[(t + 3) & 7], t * 4 + i);
    }
  }
  // weak reduction and store: the widest limbs, every multiple of r the bound admits and its two neighbours
  for (int s = 0; s < 2; ++s) {
    check_reduce(extreme<4, 4, 16>(s), "extreme (4,4) 16 r", s);
    check_reduce(extreme<0, 4, 16>(s), "extreme (0,4) 16 r", s);
    check_reduce(extreme<4, 0, 16>(s), "extreme (4,0) 16 r", s);
    check_reduce(extreme<0, 1, 16>(s), "extreme (0,1) 16 r", s);
  }
  for (int k = -15; k <= 15; ++k)
    for (int d = -1; d <= 1; ++d) {
      const auto x = multiple_of_r(k, d);
      const Fr want = d == 0 ? Fr::zero() : d == 1 ? small(1) : r_minus_1();
      CHECK(eq(val(x), want), "k r + d: the test's own value is wrong at k = %d, d = %d", k, d);
      check_reduce(x, "k r + d", k * 3 + d);
      check_reduce(lz_widen<4, 4, 16>(x), "k r + d as (4,4)", k * 3 + d);
      CHECK(eq(lz_store(x), want) && eq(lz_store(lz_widen<4, 4, 16>(x)), want), "store(%d r + %d) mismatch", k, d);
      // the same value with loose limbs: limb 1 lent 2^29 to limb 0, limb 2 borrowing from limb 3 (LO = HI = 2)
      Lz<2, 2, 16> y = lz_widen<2, 2, 16>(x);
      y.l[0] += 1 << 29; y.l[1] -= 1;
      y.l[2] -= 1 << 29; y.l[3] += 1;
      CHECK(limbs_ok(y) && eq(val(y), want) && eq(lz_store(y), want), "store(%d r + %d) with loose limbs mismatch", k, d);
    }
  // the canonical store of a weakly reduced value at the edges of its subtraction
  for (int k = 0; k < 2; ++k)
    for (int d = -1; d <= 1; ++d) {
      if (k == 0 && d < 0) continue;
      const auto x = multiple_of_r(k, d);           // 0, 1, r - 1, r, r + 1
      const auto y = multiple_of_r(k + 1, -1 - (d > 0));  // r - 1, (r - 2), 2 r - 1, 2 r - 2
      LzW wx, wy;
      for (int i = 0; i < 9; ++i) { wx.l[i] = x.l[i]; wy.l[i] = y.l[i]; }
      CHECK(eq(lz_store_weak(wx), val(x)), "store_weak(%d r + %d) mismatch", k, d);
      CHECK(eq(lz_store_weak(wy), val(y)), "store_weak(%d r - %d) mismatch", k + 1, 1 + (d > 0));
    }
  {
    LzW w;
    const auto x = multiple_of_r(1, 0);
    for (int i = 0; i < 9; ++i) w.l[i] = x.l[i];
    CHECK(eq(lz_store_weak(w), Fr::zero()) && w.l[8] == (int)P[8], "store_weak(r) is not 0");
  }
  return edge_bad;
}

int main() {
  int bad = 0;
  for (int it = 0; it < 100000; ++it) {
    const Fr a = rand_fr(), b = rand_fr(), c = rand_fr(), d = rand_fr(), w = rand_fr(), v = rand_fr();
    const auto A = lz_load(a), B = lz_load(b), C = lz_load(c), D = lz_load(d);
    // store of loose values of either sign: a + b - c - d, a - b - c - d (|value| < 4 r), and a sum of sixteen terms
    const auto s1 = lz_sub(lz_add(A, B), lz_add(C, D));
    if (!eq(lz_store(s1), fp_sub<FrP>(fp_add<FrP>(a, b), fp_add<FrP>(c, d)))) { if (bad++ < 5) printf("store(a+b-c-d) mismatch at %d\n", it); }
    const auto s2 = lz_sub(lz_sub(A, B), lz_add(C, D));
    if (!eq(lz_store(s2), fp_sub<FrP>(fp_sub<FrP>(a, b), fp_add<FrP>(c, d)))) { if (bad++ < 5) printf("store(a-b-c-d) mismatch at %d\n", it); }
    const auto n4 = lz_norm(lz_add(lz_add(A, B), lz_add(C, D)));            // (0,1), < 4 r
    const auto s16 = lz_add(lz_add(n4, n4), lz_add(n4, n4));                   // (0,4), < 16 r
    Fr want16 = fp_add<FrP>(fp_add<FrP>(a, b), fp_add<FrP>(c, d));
    want16 = fp_dbl<FrP>(fp_dbl<FrP>(want16));
    if (!eq(lz_store(s16), want16)) { if (bad++ < 5) printf("store(16 terms) mismatch at %d\n", it); }
    const auto m16 = lz_sub(lz_sub(lz_zero(), lz_add(n4, n4)), n4);           // (3,1): -12 terms
    const Fr want4 = fp_add<FrP>(fp_add<FrP>(a, b), fp_add<FrP>(c, d));
    const Fr want12 = fp_add<FrP>(fp_dbl<FrP>(want4), want4);   // three times the four-term sum
    if (!eq(lz_store(m16), fp_neg<FrP>(want12))) { if (bad++ < 5) printf("store(-12 terms) mismatch at %d\n", it); }
    // products: tight, loose-positive (0,2), loose-signed (2,2) and (1,2), negative values
    const Lw W = tw_of(w), V = tw_of(v);
    if (!eq(lz_store(lz_mul(A, W)), fp_mul<FrP>(a, w))) { if (bad++ < 5) printf("mul mismatch at %d\n", it); }
    if (!eq(lz_store(lz_mul(lz_add(A, B), W)), fp_mul<FrP>(fp_add<FrP>(a, b), w))) { if (bad++ < 5) printf("mul(a+b) mismatch at %d\n", it); }
    const auto x22 = lz_sub(lz_add(A, B), lz_add(C, D));   // (2,2)
    if (!eq(lz_store(lz_mul(x22, W)), fp_mul<FrP>(fp_sub<FrP>(fp_add<FrP>(a, b), fp_add<FrP>(c, d)), w))) { if (bad++ < 5) printf("mul(2,2) mismatch at %d\n", it); }
    const auto x21 = lz_sub(lz_sub(A, B), C);              // (2,1)
    if (!eq(lz_store(lz_mul(x21, W)), fp_mul<FrP>(fp_sub<FrP>(fp_sub<FrP>(a, b), c), w))) { if (bad++ < 5) printf("mul(2,1) mismatch at %d\n", it); }
    // a product of a product (signed top limb) and of a weakly reduced value
    const LzT p1 = lz_mul(x22, W);
    if (!eq(lz_store(lz_mul(p1, V)), fp_mul<FrP>(fp_mul<FrP>(fp_sub<FrP>(fp_add<FrP>(a, b), fp_add<FrP>(c, d)), w), v))) { if (bad++ < 5) printf("mul(mul) mismatch at %d\n", it); }
    if (!eq(lz_store(lz_mul(lz_weak(s16), V)), fp_mul<FrP>(want16, v))) { if (bad++ < 5) printf("mul(weak) mismatch at %d\n", it); }
    if (!eq(lz_store(lz_mul2(A, W, B, V)), fp_add<FrP>(fp_mul<FrP>(a, w), fp_mul<FrP>(b, v)))) { if (bad++ < 5) printf("mul2 mismatch at %d\n", it); }
    // the two-product form on signed operands (limbs of either sign below 2^29: differences of column values) and the unsigned
    // four-product form on canonical data -- the radix-4 first stage of the quarter-column 2^13 tile
    if (!eq(lz_store(lz_mul2(lz_sub(A, C), W, lz_sub(B, D), V)), fp_add<FrP>(fp_mul<FrP>(fp_sub<FrP>(a, c), w), fp_mul<FrP>(fp_sub<FrP>(b, d), v)))) { if (bad++ < 5) printf("mul2(signed) mismatch at %d\n", it); }
    {
      const Lw WC = tw_of(c), WD = tw_of(d);   // any canonical constants will do
      const Fr want = fp_add<FrP>(fp_add<FrP>(fp_mul<FrP>(a, w), fp_mul<FrP>(b, v)), fp_add<FrP>(fp_mul<FrP>(c, c), fp_mul<FrP>(d, d)));
      const LzT got4 = lz_mul4u(A, W, B, V, C, WC, D, WD);
      if (!eq(lz_store(got4), want)) { if (bad++ < 5) printf("mul4u mismatch at %d\n", it); }
      bool ok4 = got4.l[8] >= 0;
      for (int i = 0; i < 8; ++i) ok4 = ok4 && got4.l[i] >= 0 && got4.l[i] < (1 << 29);
      if (!ok4) { if (bad++ < 5) printf("mul4u result not tight at %d\n", it); }
    }
    // weak: result limbs tight, value in [0, 2 r)
    const LzT wk = lz_weak(m16);
    bool tight = wk.l[8] >= 0;
    for (int i = 0; i < 8; ++i) tight = tight && wk.l[i] >= 0 && wk.l[i] < (1 << 29);
    if (!tight) { if (bad++ < 5) printf("weak result not tight at %d\n", it); }
  }
  printf("lz29: %d bad\n", bad);
  const int ebad = edge_checks();
  printf("lz29 edges: %d bad\n", ebad);
  return bad != 0 || ebad != 0;
}
