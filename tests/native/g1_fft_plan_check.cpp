// csrc/g1_fft_plan.hpp + csrc/g1_fft_ladder.hip.hpp on the CPU: the schedule the launcher of zkfhe_g1_fft walks and the butterfly
// arithmetic its kernels run, for every log_n from 1 to 6, both directions, against the naive double sum.
//
// Every input point is a known multiple p_j G of the generator (the identity is p_j = 0), so the naive sum
// out[i] = sum_j w^(+-ij) p_j G is taken in the scalar field, one term per (i, j), and mapped to the group by one scalar
// multiplication that shares no code with the ladders under test (bit by bit, mixed additions).  Results are compared as canonical
// affine Montgomery limbs, byte for byte.
//
// Stage structures: with the launcher's wave of 64 lanes, sizes up to 2^6 run window stages only; the plan is also made for waves
// of 1, 2 and 4 lanes, which puts the shared-twiddle structure (and, at wave 1, its n^-1 stage) on these sizes.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "g1_fft_ladder.hip.hpp"
#include "g1_fft_plan.hpp"

using namespace zk;

static int failures = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++failures;                     \
      printf("FAIL %s: ", #cond);     \
      printf(__VA_ARGS__);            \
      printf("\n");                   \
    }                                 \
  } while (0)

static Fr fr_u64(uint64_t v) {
  Fr t = Fr::zero();
  t.l[0] = (u32)v, t.l[1] = (u32)(v >> 32);
  return fp_to_mont<FrP>(t);
}

// halo2's omega for 2^log_n: ROOT_OF_UNITY = 7^((r - 1) / 2^28), squared down
static Fr root_of_unity(int log_n) {
  const u32 w[8] = {0x60c37c9cu, 0xd34f1ed9u, 0xd39329c8u, 0x3215cf6du, 0x3dd31f74u, 0x98865ea9u, 0x166d18b7u, 0x03ddb9f5u};
  Fr c;
  for (int i = 0; i < 8; ++i) c.l[i] = w[i];
  Fr r = fp_to_mont<FrP>(c);
  for (int i = 0; i < 28 - log_n; ++i) r = fp_sqr<FrP>(r);
  return r;
}

static G1Affine generator() {
  G1Affine g;
  Fq t = Fq::zero();
  t.l[0] = 1;
  g.x = fp_to_mont<FqP>(t);
  t.l[0] = 2;
  g.y = fp_to_mont<FqP>(t);
  return g;
}

// k G, k in Montgomery form: the reference's own ladder (mixed additions, bit by bit through an index)
static G1Affine ref_mul_gen(const Fr &k) {
  const Fr s = fp_from_mont<FrP>(k);
  const G1Affine g = generator();
  G1X acc = G1X::identity();
  for (int bit = 255; bit >= 0; --bit) {
    acc = g1x_dbl(acc);
    if ((s.l[bit >> 5] >> (bit & 31)) & 1) g1x_add_affine(acc, g, false);
  }
  return g1x_to_affine(acc);
}

struct Tables {
  std::vector<Fr> fwd, inv;
  Fr n_inv;
};

static Tables tables(int log_n) {
  const size_t n = (size_t)1 << log_n;
  Tables t;
  const Fr w = root_of_unity(log_n), wi = fp_inv<FrP>(w);
  t.fwd.assign(n, Fr::one());
  t.inv.assign(n, Fr::one());
  for (size_t j = 1; j < n; ++j) t.fwd[j] = t.fwd[j - 1] * w, t.inv[j] = t.inv[j - 1] * wi;
  t.n_inv = fp_inv<FrP>(fr_u64(n));
  return t;
}

// what zkfhe_g1_fft does, stage by stage, thread by thread
static std::vector<G1Affine> walk(const G1FftPlan &plan, bool inverse, int wave, const Tables &tb, const std::vector<G1Affine> &in) {
  const int log_n = plan.log_n;
  const size_t n = (size_t)1 << log_n;
  const std::vector<Fr> &tw = inverse ? tb.inv : tb.fwd;
  std::vector<G1X> x(n);
  std::vector<int> seen(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t r = g1_fft_bitrev(i, log_n);
    CHECK(r < n && g1_fft_bitrev(r, log_n) == i, "bitrev log_n %d i %zu", log_n, i);
    x[r] = g1x_from_affine(in[i]);
  }
  for (int s = 0; s < plan.n_stages; ++s) {
    const G1FftStage &st = plan.stage[s];
    std::fill(seen.begin(), seen.end(), 0);
    size_t wave_tw = 0;
    for (size_t t = 0; t < n / 2; ++t) {
      const G1FftButterfly bf = g1_fft_butterfly(st.kind, log_n, st.log_half, t);
      CHECK(bf.lo < bf.hi && bf.hi < n && bf.tw < n / 2, "butterfly out of range: log_n %d stage %d t %zu", log_n, s, t);
      if (bf.hi >= n || bf.tw >= n) return {};
      ++seen[bf.lo], ++seen[bf.hi];
      if (st.kind == G1FFT_SHARED) {   // the lanes of a wave must hold one twiddle
        if (t % wave == 0) wave_tw = bf.tw;
        CHECK(bf.tw == wave_tw, "lanes of a wave differ in twiddle: log_n %d stage %d t %zu", log_n, s, t);
      }
      const G1FftScalar k = g1_fft_scalar(tw[bf.tw], st.scale, tb.n_inv);
      G1X a = x[bf.lo], b = x[bf.hi];
      G1FftHostTable tab;
      if (!g1_fft_scalar_is_one(k)) b = g1x_mul_window(tab, b, k);
      if (st.scale) a = g1x_mul_window(tab, a, g1_fft_scalar(tb.n_inv, false, tb.n_inv));
      g1_fft_combine(a, b);
      x[bf.lo] = a, x[bf.hi] = b;
    }
    for (size_t i = 0; i < n; ++i) CHECK(seen[i] == 1, "slot %zu touched %d times: log_n %d stage %d", i, seen[i], log_n, s);
  }
  std::vector<G1Affine> out(n);
  for (size_t i = 0; i < n; ++i) out[i] = g1x_to_affine(x[i]);
  return out;
}

static void check_plans() {
  for (int log_n = -1; log_n <= G1FFT_MAX_LOG + 1; ++log_n)
    for (int inverse = 0; inverse < 2; ++inverse) {
      const G1FftPlan p = g1_fft_plan(log_n, inverse != 0);
      CHECK(p.refused == (log_n < 1 || log_n > G1FFT_MAX_LOG), "refusal at log_n %d", log_n);
      if (p.refused) continue;
      CHECK(p.n_stages == log_n, "stage count at log_n %d", log_n);
      bool any_shared = false;
      for (int s = 0; s < p.n_stages; ++s) {
        const G1FftStage &st = p.stage[s];
        const size_t blocks = (size_t)1 << (log_n - 1 - s);
        CHECK(st.log_half == s, "stage order at log_n %d", log_n);
        CHECK((st.kind == G1FFT_SHARED) == (blocks >= (size_t)G1FFT_WAVE), "stage kind at log_n %d stage %d", log_n, s);
        CHECK(st.scale == (inverse && s == log_n - 1), "n^-1 stage at log_n %d stage %d", log_n, s);
        // what k_g1_fft_shared relies on: whole waves, and never the n^-1 stage
        if (st.kind == G1FFT_SHARED) CHECK(!st.scale && (((size_t)1 << (log_n - 1)) % G1FFT_WAVE) == 0, "shared stage at log_n %d stage %d", log_n, s);
        any_shared |= st.kind == G1FFT_SHARED;
      }
      CHECK(any_shared == (log_n >= G1FFT_FIRST_SHARED_LOG), "first size with a shared stage: log_n %d", log_n);
    }
  CHECK(g1_fft_plan(4, false, 3).refused && g1_fft_plan(4, false, 0).refused, "a wave that is no power of two");
}

int main() {
  check_plans();
  std::mt19937_64 rng(20240607);
  auto rand_fr = [&]() {
    Fr t;
    for (int i = 0; i < 8; ++i) t.l[i] = (u32)rng();
    t.l[7] &= 0x0fffffffu;   // < 2^252 < r: a reduced residue (read as a Montgomery form, whatever value that is)
    return t;
  };
  // the ladder alone at the edges of its digits: k G for small k (every digit value next to zeros), k = r - 1 = -1 (the longest
  // run of carries), a lone top bit, the identity as the base, and random scalars
  {
    std::vector<Fr> ks;
    for (uint64_t v = 0; v <= 40; ++v) ks.push_back(fr_u64(v));
    ks.push_back(fp_neg<FrP>(Fr::one()));
    ks.push_back(fp_neg<FrP>(fr_u64(4)));
    Fr top = Fr::zero();
    top.l[7] = 0x20000000u;   // 2^253
    ks.push_back(fp_to_mont<FrP>(top));
    for (int i = 0; i < 24; ++i) ks.push_back(rand_fr());
    const G1X g = g1x_from_affine(generator());
    for (const Fr &k : ks) {
      G1FftHostTable tab;
      const G1Affine got = g1x_to_affine(g1x_mul_window(tab, g, g1_fft_scalar(k, false, k))), want = ref_mul_gen(k);
      CHECK(memcmp(&got, &want, sizeof(G1Affine)) == 0, "ladder differs from the reference multiplication");
      CHECK(g1x_mul_window(tab, G1X::identity(), g1_fft_scalar(k, false, k)).is_identity(), "k times the identity");
    }
  }
  int cases = 0;
  for (int log_n = 1; log_n <= 6; ++log_n) {
    const size_t n = (size_t)1 << log_n;
    const Tables tb = tables(log_n);
    // the inputs as scalars p_j (P_j = p_j G): random; all G; P_j = w^j G; all identity; identity at the odd indices; one point alone
    std::vector<std::vector<Fr>> inputs;
    std::vector<Fr> v(n);
    for (auto &e : v) e = rand_fr();
    inputs.push_back(v);
    inputs.push_back(std::vector<Fr>(n, Fr::one()));
    inputs.push_back(tb.fwd);
    inputs.push_back(std::vector<Fr>(n, Fr::zero()));
    for (size_t j = 0; j < n; ++j) v[j] = (j & 1) ? Fr::zero() : rand_fr();
    inputs.push_back(v);
    v.assign(n, Fr::zero());
    v[n - 1] = rand_fr();
    inputs.push_back(v);
    for (size_t which = 0; which < inputs.size(); ++which) {
      const std::vector<Fr> &p = inputs[which];
      std::vector<G1Affine> pts(n);
      for (size_t j = 0; j < n; ++j) pts[j] = ref_mul_gen(p[j]);
      for (int inverse = 0; inverse < 2; ++inverse) {
        const std::vector<Fr> &tw = inverse ? tb.inv : tb.fwd;
        std::vector<G1Affine> want(n);
        for (size_t i = 0; i < n; ++i) {
          Fr sum = Fr::zero();
          for (size_t j = 0; j < n; ++j) sum = sum + tw[(i * j) & (n - 1)] * p[j];
          if (inverse) sum = sum * tb.n_inv;
          want[i] = ref_mul_gen(sum);
        }
        if (inverse && which == 1)   // all G: G at index 0, the identity elsewhere
          for (size_t i = 0; i < n; ++i) CHECK(want[i].is_identity() == (i != 0), "reference of the all-G input");
        if (inverse && which == 2 && n > 1)   // w^j G: G at index 1
          for (size_t i = 0; i < n; ++i) CHECK(want[i].is_identity() == (i != 1), "reference of the w^j G input");
        for (int wave : {G1FFT_WAVE, 1, 2, 4}) {
          const G1FftPlan plan = g1_fft_plan(log_n, inverse != 0, wave);
          CHECK(!plan.refused, "plan refused");
          if (wave == G1FFT_WAVE)
            for (int s = 0; s < plan.n_stages; ++s) CHECK(plan.stage[s].kind == G1FFT_WINDOW, "a size below 2^7 has window stages only");
          if (wave == 1)
            for (int s = 0; s < plan.n_stages; ++s) CHECK(plan.stage[s].kind == G1FFT_SHARED, "wave 1 shares every stage");
          const std::vector<G1Affine> got = walk(plan, inverse != 0, wave, tb, pts);
          CHECK(got.size() == n && memcmp(got.data(), want.data(), n * sizeof(G1Affine)) == 0, "log_n %d input %zu inverse %d wave %d differs from the naive sum", log_n,
                which, inverse, wave);
          ++cases;
        }
      }
    }
  }
  if (failures) {
    printf("g1 fft plan check: %d failure(s)\n", failures);
    return 1;
  }
  printf("g1 fft plan check: ok (%d transforms)\n", cases);
  return 0;
}
