// Host-side check of the lazy signed-limb arithmetic over Fq in csrc/fq29.hip.hpp (Lz<LO, HI, V>, lq_mul / lq_sqr / lq_mul2 and the
// point operations of the MSM kernels written on them) against the standard 8 x 32-bit arithmetic of bn254.hip.hpp.  The value a
// limb vector stands for is computed here by Horner's rule in the standard arithmetic, independently of the code under test.  The host
// pass compiles the C bodies of the products (what -DZK_MAD_C selects on the device); the generated assembly runs on the same
// extreme operands in tests/native/tied_products_check.hip.
#include "fq29.hip.hpp"
#include <cstdio>
#include <random>
using namespace zk;

static std::mt19937_64 rng(4242);
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static Fq rand_fq() {
  Fq a;
  for (;;) {
    for (int i = 0; i < 8; ++i) a.l[i] = (u32)rng();
    a.l[7] &= 0x3fffffff;
    bool lt = false;
    for (int i = 7; i >= 0; --i) {
      if (a.l[i] != FqP::MOD[i]) { lt = a.l[i] < FqP::MOD[i]; break; }
    }
    if (lt) return a;
  }
}
static bool eq(const Fq &a, const Fq &b) {
  for (int i = 0; i < 8; ++i) if (a.l[i] != b.l[i]) return false;
  return true;
}
static Fq small(u32 v) { Fq a = Fq::zero(); a.l[0] = v; return a; }
static Fq times32(Fq a) { for (int i = 0; i < 5; ++i) a = fp_dbl<FqP>(a); return a; }
// sum l[i] 2^(29 i) mod p, canonical, for limbs of either sign
template <int LO, int HI, int V>
static Fq val(const Lz<LO, HI, V> &a) {
  Fq acc = Fq::zero();
  for (int i = 8; i >= 0; --i) {
    for (int k = 0; k < 29; ++k) acc = fp_dbl<FqP>(acc);
    const long long v = a.l[i];
    const Fq lo = small((u32)((v < 0 ? -v : v) & 0xffff)), hi = small((u32)((v < 0 ? -v : v) >> 16));   // |v| < 2^32 in two halves below p
    Fq t = hi;
    for (int k = 0; k < 16; ++k) t = fp_dbl<FqP>(t);
    t = fp_add<FqP>(t, lo);
    acc = v < 0 ? fp_sub<FqP>(acc, t) : fp_add<FqP>(acc, t);
  }
  return acc;
}
template <int LO, int HI, int V>
static bool limbs_ok(const Lz<LO, HI, V> &a) {
  for (int i = 0; i < 8; ++i)
    if (!((long long)a.l[i] > -(long long)LO * (1ll << 29) - (LO == 0) && (long long)a.l[i] < (long long)HI * (1ll << 29))) return false;
  const long long top = a.l[8];
  return top > -(long long)(V + 1) * (1ll << 22) && top < (long long)(V + 1) * (1ll << 22);
}
// the extreme member of a bound: every lower limb at the edge of its range on the given side, the top limb as large as |value| < V p lets it be
template <int LO, int HI, int V>
static Lz<LO, HI, V> extreme(bool negative) {
  Lz<LO, HI, V> r;
  const u32 P[9] = ZK_Q29_P;
  if (negative && LO == 0) {   // non-negative limbs, negative value: the lower limbs at zero
    for (int i = 0; i < 8; ++i) r.l[i] = 0;
    r.l[8] = -(int)(V * P[8]);
    return r;
  }
  for (int i = 0; i < 8; ++i) r.l[i] = negative ? -LO * ((1 << 29) - 1) : HI * ((1 << 29) - 1);   // a limb typed h is a sum of h terms below 2^29
  // V p has top limb V P[8] and lower limbs above zero; |lower limbs| of r are below max(LO, HI) 2^232, i.e. below max(LO, HI) top units
  const int room = (int)(V * P[8]) - (LO > HI ? LO : HI) - 1;
  r.l[8] = negative ? -room : room;
  return r;
}

static G1Affine rand_point() {
  G1Affine g;
  g.x = fp_to_mont<FqP>(small(1)); g.y = fp_to_mont<FqP>(small(2));
  G1X acc = G1X::identity();
  const unsigned k = 2 + (unsigned)(rng() % 5000);
  for (int bit = 13; bit >= 0; --bit) { acc = g1x_dbl(acc); if ((k >> bit) & 1) g1x_add_affine(acc, g, false); }
  return g1x_to_affine(acc);
}
static bool same_point(const G1X29 &p29, const G1X &pstd) {
  if (p29.is_identity() || pstd.is_identity()) return p29.is_identity() && pstd.is_identity();
  const G1Affine a = g1x_to_affine(g1x29_to_std(p29)), b = g1x_to_affine(pstd);
  return eq(a.x, b.x) && eq(a.y, b.y);
}
static bool acc_ok(const G1X29 &a) { return limbs_ok(a.x) && limbs_ok(a.y) && limbs_ok(a.zz) && limbs_ok(a.zzz); }
// another representative of the same accumulator: k p added to a coordinate, carries propagated -- tight limbs, values up to the bound
template <int V>
static Lz<0, 1, V> shifted(const Lz<0, 1, V> &a, int k) {
  const u32 P[9] = ZK_Q29_P;
  const LqT w = lq_weak(a);   // [0, 1.04 p)
  Lz<0, 1, V> r;
  long long c = 0;
  for (int i = 0; i < 9; ++i) {
    const long long v = (long long)w.l[i] + (long long)k * (long long)P[i] + c;
    r.l[i] = i < 8 ? (int)(v & (long long)q29::MASK) : (int)v;
    c = v >> 29;
  }
  return r;
}

template <class A, class B>
static void check_mul(const A &a, const B &b, const char *what, int it) {
  const LqT r = lq_mul(a, b);
  CHECK(limbs_ok(r), "%s: result not tight at %d", what, it);
  CHECK(eq(times32(val(r)), fp_mul<FqP>(val(a), val(b))), "%s mismatch at %d", what, it);
}
template <class A>
static void check_sqr(const A &a, const char *what, int it) {
  const LqT r = lq_sqr(a);
  CHECK(limbs_ok(r) && r.l[8] >= 0, "%s: result not tight at %d", what, it);
  CHECK(eq(times32(val(r)), fp_mul<FqP>(val(a), val(a))), "%s mismatch at %d", what, it);
}
template <class A, class B, class C, class D>
static void check_mul2(const A &a, const B &b, const C &c, const D &d, const char *what, int it) {
  const LqT r = lq_mul2(a, b, c, d);
  CHECK(limbs_ok(r), "%s: result not tight at %d", what, it);
  CHECK(eq(times32(val(r)), fp_add<FqP>(fp_mul<FqP>(val(a), val(b)), fp_mul<FqP>(val(c), val(d)))), "%s mismatch at %d", what, it);
}

static void field_checks() {
  Fq pm1 = Fq::zero();
  for (int i = 0; i < 8; ++i) pm1.l[i] = FqP::MOD[i];
  pm1.l[0] -= 1;
  for (int it = 0; it < 60000; ++it) {
    Fq a = rand_fq(), b = rand_fq(), c = rand_fq(), d = rand_fq();
    if (it < 27) {   // every pair of 0, 1, p - 1, and the same as third and fourth operands
      const Fq e[3] = {Fq::zero(), small(1), pm1};
      a = e[it % 3]; b = e[(it / 3) % 3]; c = e[(it / 9) % 3]; d = e[it % 3];
    }
    const Lz<0, 1, 1> A = lz_from_f29<1>(f29_unpack(a)), B = lz_from_f29<1>(f29_unpack(b)), C = lz_from_f29<1>(f29_unpack(c)), D = lz_from_f29<1>(f29_unpack(d));
    CHECK(eq(val(A), a), "val/unpack mismatch at %d", it);
    // additions, subtractions, carry propagation, weak reduction, canonical packing
    const auto s4 = lz_sub(lz_add(A, B), lz_add(C, D));            // (2,2), 4 p
    const Fq w4 = fp_sub<FqP>(fp_add<FqP>(a, b), fp_add<FqP>(c, d));
    CHECK(eq(val(s4), w4) && eq(val(lz_norm(s4)), w4) && limbs_ok(lz_norm(s4)), "add/sub/norm mismatch at %d", it);
    const LqT wk = lq_weak(lz_sub(lz_sub(lz_neg(lz_norm(s4)), lz_norm(s4)), lz_add(lz_norm(s4), lz_norm(s4))));   // -4 s4: (4,0), 16 p
    bool tight = wk.l[8] >= 0;
    for (int i = 0; i < 8; ++i) tight = tight && wk.l[i] >= 0 && wk.l[i] < (1 << 29);
    CHECK(tight, "weak result not tight at %d", it);
    CHECK(eq(val(wk), fp_neg<FqP>(fp_dbl<FqP>(fp_dbl<FqP>(w4)))), "weak mismatch at %d", it);
    CHECK(eq(lq_pack_canonical(s4), w4), "canonical pack mismatch at %d", it);
    CHECK(eq(val(lq_unpack(lq_pack(s4))), w4), "pack mismatch at %d", it);
    // the zero test: k p for every k the bound admits, and a non-zero value
    {
      const int k = (int)(rng() % 19) - 9;
      Lz<0, 1, 10> zero10;
      for (int i = 0; i < 9; ++i) zero10.l[i] = 0;
      const Lz<1, 1, 10> zk = lz_widen<1, 1, 10>(shifted(zero10, k));
      CHECK(lq_is_zero_mod_p(zk), "zero test misses %d p at %d", k, it);
      CHECK(lq_is_zero_mod_p(lz_sub(lz_widen<0, 1, 2>(A), lz_widen<0, 1, 8>(A))), "zero test misses a - a at %d", it);
      CHECK(lq_is_zero_mod_p(lz_widen<1, 1, 10>(lz_sub(A, B))) == eq(a, b), "zero test on a - b wrong at %d", it);
      Lz<1, 1, 10> off = zk;   // k p + 2^29 j: the same low limb, another value
      off.l[1] += 1;
      CHECK(!lq_is_zero_mod_p(off), "zero test accepts k p + 2^29 at %d", it);
    }
    // products: tight, signed (1,1) and (2,2) operands
    const auto X = lz_sub(A, B), Y = lz_sub(C, D);      // (1,1), 2 p
    check_mul(A, B, "mul(tight)", it);
    check_mul(X, Y, "mul(signed)", it);
    check_mul(s4, C, "mul((2,2), tight)", it);
    check_mul(C, s4, "mul(tight, (2,2))", it);
    check_mul(lq_mul(X, Y), lq_mul(A, D), "mul(product, product)", it);
    check_sqr(A, "sqr(tight)", it);
    check_sqr(X, "sqr(signed)", it);
    check_sqr(lz_neg(A), "sqr(negative)", it);
    check_mul2(A, B, C, D, "mul2(tight)", it);
    check_mul2(X, Y, lz_neg(A), D, "mul2(signed)", it);
    check_mul2(lz_neg(C), lz_neg(D), Y, X, "mul2(negative)", it);
  }
  // the largest values the declared bounds admit, both signs
  for (int sa = 0; sa < 2; ++sa)
    for (int sb = 0; sb < 2; ++sb) {
      check_mul(extreme<2, 2, 16>(sa), extreme<1, 1, 10>(sb), "mul extreme (2,2)x(1,1)", sa * 2 + sb);
      check_mul(extreme<1, 1, 10>(sa), extreme<2, 2, 16>(sb), "mul extreme (1,1)x(2,2)", sa * 2 + sb);
      check_mul(extreme<1, 1, 10>(sa), extreme<0, 1, 2>(sb), "mul extreme p x pp", sa * 2 + sb);
      check_mul(extreme<0, 1, 8>(sa), extreme<0, 1, 2>(sb), "mul extreme x x pp", sa * 2 + sb);
      check_mul(extreme<1, 1, 12>(sa), extreme<1, 1, 13>(sb), "mul extreme 12 p x 13 p", sa * 2 + sb);
      check_mul2(extreme<1, 1, 4>(sa), extreme<1, 1, 10>(sb), extreme<1, 0, 2>(sa), extreme<0, 1, 2>(sb), "mul2 extreme (addition)", sa * 2 + sb);
      check_mul2(extreme<1, 1, 12>(sa), extreme<1, 1, 10>(sb), extreme<1, 1, 10>(sb), extreme<1, 1, 4>(sa), "mul2 extreme 160 p^2", sa * 2 + sb);
      check_mul2(extreme<1, 1, 12>(sa), extreme<1, 1, 10>(sb), extreme<1, 1, 10>(!sb), extreme<1, 1, 4>(!sa), "mul2 extreme one sign", sa * 2 + sb);
    }
  for (int sa = 0; sa < 2; ++sa) {
    check_sqr(extreme<1, 1, 12>(sa), "sqr extreme 12 p", sa);
    check_sqr(extreme<1, 1, 10>(sa), "sqr extreme p", sa);
    check_sqr(extreme<0, 1, 8>(sa), "sqr extreme x", sa);
    const LqT w = lq_weak(extreme<4, 4, 16>(sa));
    CHECK(limbs_ok(w) && w.l[8] >= 0 && eq(val(w), val(extreme<4, 4, 16>(sa))), "weak extreme %d", sa);
  }
}

static void point_checks() {
  for (int it = 0; it < 2000; ++it) {
    G1Affine p = rand_point(), q = rand_point();
    while (eq(q.x, p.x)) q = rand_point();   // q = +-p would make the sums below the identity
    if (it == 0) { p.x = fp_to_mont<FqP>(small(1)); p.y = fp_to_mont<FqP>(small(2)); }   // the generator: coordinates 1 and 2
    const G1A29 p29 = g1a29_load(g1_affine_to_29(p)), q29 = g1a29_load(g1_affine_to_29(q));
    G1A29 id29;
    id29.x = id29.y = f29_zero();
    for (int neg = 0; neg < 2; ++neg) {
      // empty accumulator, identity entry
      G1X s = G1X::identity();
      G1X29 s29 = G1X29::identity();
      g1x29_add_affine(s29, id29, neg);
      CHECK(s29.is_identity(), "identity entry into an empty accumulator at %d", it);
      g1x_add_affine(s, p, neg); g1x29_add_affine(s29, p29, neg);
      CHECK(same_point(s29, s) && acc_ok(s29), "empty accumulator mismatch at %d", it);
      g1x29_add_affine(s29, id29, !neg);
      CHECK(same_point(s29, s), "identity entry mismatch at %d", it);
      // mixed addition, then Q = P through the addition (doubling) with either sign, on a one-entry and on a general accumulator
      G1X d = s; G1X29 d29 = s29;
      g1x_add_affine(d, p, neg); g1x29_add_affine(d29, p29, neg);
      CHECK(same_point(d29, d) && acc_ok(d29), "mixed doubling (affine accumulator) mismatch at %d", it);
      g1x_add_affine(s, q, it & 1); g1x29_add_affine(s29, q29, it & 1);
      CHECK(same_point(s29, s) && acc_ok(s29), "mixed add mismatch at %d", it);
      const G1Affine sa = g1x_to_affine(s);
      const G1A29 sa29 = g1a29_load(g1_affine_to_29(sa));
      {
        G1X e = s; G1X29 e29 = s29;   // acc = S in XYZZ, entry = S or -S in affine
        g1x_add_affine(e, sa, false); g1x29_add_affine(e29, sa29, false);
        CHECK(same_point(e29, e) && !e29.is_identity() && acc_ok(e29), "mixed doubling mismatch at %d", it);
        G1X29 c29 = s29;
        g1x29_add_affine(c29, sa29, true);
        CHECK(c29.is_identity(), "mixed cancellation mismatch at %d", it);
        G1X n = G1X::identity(); G1X29 n29 = G1X29::identity();   // acc = -S (built with neg), entry = -S: doubling; entry = S: cancellation
        g1x_add_affine(n, q, !(it & 1)); g1x29_add_affine(n29, q29, !(it & 1));
        g1x_add_affine(n, p, !neg); g1x29_add_affine(n29, p29, !neg);
        G1X29 m29 = n29;
        g1x_add_affine(n, sa, true); g1x29_add_affine(n29, sa29, true);
        CHECK(same_point(n29, n) && !n29.is_identity(), "mixed doubling of -S mismatch at %d", it);
        g1x29_add_affine(m29, sa29, false);
        CHECK(m29.is_identity(), "mixed cancellation of -S mismatch at %d", it);
      }
      // full addition, doubling through it, cancellation through it, the doubling itself
      G1X t = s; G1X29 t29 = s29;
      g1x_add(t, d); g1x29_add(t29, d29);
      CHECK(same_point(t29, t) && acc_ok(t29), "full add mismatch at %d", it);
      if (t.is_identity()) continue;   // 3 p = +-q: nothing left to double or cancel
      G1X e = t; G1X29 e29 = t29;
      g1x_add(e, t); g1x29_add(e29, t29);
      CHECK(same_point(e29, e) && acc_ok(e29), "full doubling mismatch at %d", it);
      CHECK(same_point(g1x29_dbl(t29), g1x_dbl(t)) && acc_ok(g1x29_dbl(t29)), "dbl mismatch at %d", it);
      {
        G1X29 m29 = t29;   // -T: the same x, zz, zzz and the negated y
        m29.y = lz_widen<0, 1, 2>(lz_norm(lz_neg(lq_weak(t29.y))));
        G1X29 c29 = t29;
        g1x29_add(c29, m29);
        CHECK(c29.is_identity(), "full cancellation mismatch at %d", it);
        G1X29 i29 = t29;
        g1x29_add(i29, G1X29::identity());
        G1X29 j29 = G1X29::identity();
        g1x29_add(j29, t29);
        CHECK(same_point(i29, t) && same_point(j29, t), "full add with the identity mismatch at %d", it);
      }
      // the same operations on the extreme representatives of the accumulator the types admit: x + k p up to +-8 p, y, zz, zzz down to -p
      for (int k = -7; k <= 6; k += 13) {
        G1X29 x29 = t29;
        x29.x = shifted(t29.x, k);
        x29.y = shifted(t29.y, k < 0 ? -1 : 0);
        x29.zz = shifted(t29.zz, k < 0 ? 0 : -1);
        x29.zzz = shifted(t29.zzz, -1);
        CHECK(acc_ok(x29) && same_point(x29, t), "shifted representative mismatch at %d", it);
        G1X u = t; G1X29 u29 = x29;
        g1x_add_affine(u, q, neg); g1x29_add_affine(u29, q29, neg);
        CHECK(same_point(u29, u) && acc_ok(u29), "mixed add on an extreme representative mismatch at %d (k = %d)", it, k);
        u = t; u29 = x29;
        g1x_add(u, s); g1x29_add(u29, s29);
        CHECK(same_point(u29, u) && acc_ok(u29), "full add on an extreme representative mismatch at %d (k = %d)", it, k);
        u = s; u29 = s29;
        g1x_add(u, t); g1x29_add(u29, x29);
        CHECK(same_point(u29, u) && acc_ok(u29), "full add of an extreme representative mismatch at %d (k = %d)", it, k);
        u29 = x29;
        g1x29_add(u29, t29);   // the same point under two representatives: doubling
        CHECK(same_point(u29, g1x_dbl(t)), "full doubling across representatives mismatch at %d (k = %d)", it, k);
        CHECK(same_point(g1x29_dbl(x29), g1x_dbl(t)), "dbl of an extreme representative mismatch at %d (k = %d)", it, k);
        const G1Affine ta = g1x_to_affine(t);
        const G1A29 ta29 = g1a29_load(g1_affine_to_29(ta));
        u29 = x29;
        g1x29_add_affine(u29, ta29, false);
        CHECK(same_point(u29, g1x_dbl(t)), "mixed doubling on an extreme representative mismatch at %d (k = %d)", it, k);
        u29 = x29;
        g1x29_add_affine(u29, ta29, true);
        CHECK(u29.is_identity(), "mixed cancellation on an extreme representative mismatch at %d (k = %d)", it, k);
        CHECK(same_point(g1x29_load(g1x29_store(x29)), t), "store/load of an extreme representative mismatch at %d (k = %d)", it, k);
      }
      CHECK(same_point(g1x29_load(g1x29_store(t29)), t), "store/load mismatch at %d", it);
    }
  }
}

// one accumulator, 12 000 mixed additions with no canonicalisation in between  (48 entries with random signs),
// the type's limb bounds checked after every one, the point compared at the end and at a few places on the way
static void chain_check() {
  const int NPTS = 48, N = 12000;
  G1Affine pts[NPTS];
  G1A29 pts29[NPTS];
  for (int i = 0; i < NPTS; ++i) { pts[i] = rand_point(); pts29[i] = g1a29_load(g1_affine_to_29(pts[i])); }
  G1X s = G1X::identity();
  G1X29 s29 = G1X29::identity();
  int limb_bad = 0;
  for (int i = 0; i < N; ++i) {
    const int j = (int)(rng() % NPTS);
    const bool neg = (rng() >> 17) & 1;
    g1x_add_affine(s, pts[j], neg);
    g1x29_add_affine(s29, pts29[j], neg);
    if (!acc_ok(s29)) ++limb_bad;
    if (i == 10 || i == 1000) CHECK(same_point(s29, s), "chain mismatch after %d additions", i + 1);
  }
  CHECK(limb_bad == 0, "chain: accumulator outside its declared bounds after %d additions", limb_bad);
  CHECK(same_point(s29, s), "chain mismatch after %d additions", N);
  // and a chain of full additions of lazy accumulators
  G1X t = G1X::identity();
  G1X29 t29 = G1X29::identity();
  for (int i = 0; i < 2000; ++i) {
    g1x_add_affine(s, pts[i % NPTS], false); g1x29_add_affine(s29, pts29[i % NPTS], false);
    g1x_add(t, s); g1x29_add(t29, s29);
    if (i % 97 == 0) { t = g1x_dbl(t); t29 = g1x29_dbl(t29); }
    if (!acc_ok(t29)) ++limb_bad;
  }
  CHECK(limb_bad == 0, "full chain: accumulator outside its declared bounds %d times", limb_bad);
  CHECK(same_point(t29, t), "full chain mismatch");
}

int main() {
  field_checks();
  point_checks();
  chain_check();
  printf("lq29: %d bad\n", bad);
  return bad != 0;
}
