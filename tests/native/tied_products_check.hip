// The nine-limb radix-2^29 Montgomery products as the DEVICE runs them -- the generated inline assembly of csrc/mont29_tied.inc
// (mont29u_* and mont29i_*: mul_v, mul_s, sqr, mul2) -- at the largest operands each wrapper's declared bound admits, both signs, next
// to the host's C body (mont29_c) and the standard 8 x 32-bit arithmetic of bn254.hip.hpp.
//
// ONE case list for both sides: tied_case() evaluates a case and returns the canonical packed result.  A kernel calls it on the device
// (one case per lane), main() calls it on the host, where every product is the C body; the third party is fp_mul<> on the values the
// limb vectors stand for, computed here by Horner's rule independently of the code under test.  The constant of mul_s has to be the
// same in every lane of a wave: it is a kernel argument, one launch per constant (the first with every case, the others with the
// cases that read it).
//   tied_products_check          device, host and reference; needs a GPU
//   tied_products_check --host   host against the reference only (all a plain C++ build of this file, `-x c++`, can do)
// Prints `tied products: N bad`; the exit status is non-zero on any mismatch or HIP error.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "lz29.hip.hpp"
#include <random>
#include <vector>
using namespace zk;

enum Kind {
  // Fr, signed (mont29i_*): the NTT tile's products and its reductions
  LZ_MUL_22, LZ_MUL_12, LZ_MUL_21, LZ_MUL_S, LZ_MUL2, LZ_MUL4U, LZ_STORE_44, LZ_STORE_WEAK,
  // Fr, unsigned (mont29u_*)
  FR29_MUL, FR29_SQR, FR29_MUL2,
  // Fq, signed: the MSM's point arithmetic
  LQ_MUL_22_11, LQ_MUL_11_22, LQ_MUL_12_13, LQ_SQR, LQ_MUL2, LQ_STORE_44,
  // Fq, unsigned
  F29_MUL, F29_SQR, F29_MUL2,
  N_KINDS
};
static const char *const KIND_NAME[N_KINDS] = {
  "lz_mul (2,2)", "lz_mul (1,2)", "lz_mul (2,1)", "lz_mul<uniform>", "lz_mul2", "lz_mul4u", "lz_store (4,4)", "lz_store_weak",
  "fr29_mul", "fr29_sqr", "fr29_mul2", "lq_mul (2,2)x(1,1)", "lq_mul (1,1)x(2,2)", "lq_mul 12 p x 13 p", "lq_sqr", "lq_mul2", "lq_pack_canonical (4,4)",
  "f29_mul", "f29_sqr", "f29_mul2"};

struct Rec {
  int kind;
  int op[8][9];   // operands as limb vectors; a kind uses the first 1, 2, 4 or 8
};
struct Out {
  u32 l[8];
};

template <class T>
ZK_HD T as(const int (&l)[9]) {
  T r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = (decltype(+r.l[0]))l[i];
  return r;
}
ZK_HD Out out_of(const Fr &a) {
  Out o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.l[i] = a.l[i];
  return o;
}
ZK_HD Out out_of(const Fq &a) {
  Out o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.l[i] = a.l[i];
  return o;
}
ZK_HD LzW as_weak(const int (&l)[9]) {
  LzW r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = l[i];
  return r;
}

// the case list: what each kind computes, on either side
ZK_HD Out tied_case(const Rec &c, const Lw &uc) {
  switch (c.kind) {
    case LZ_MUL_22: return out_of(lz_store(lz_mul(as<Lz<2, 2, 160>>(c.op[0]), as<Lw>(c.op[1]))));
    case LZ_MUL_12: return out_of(lz_store(lz_mul(as<Lz<1, 2, 160>>(c.op[0]), as<Lw>(c.op[1]))));
    case LZ_MUL_21: return out_of(lz_store(lz_mul(as<Lz<2, 1, 160>>(c.op[0]), as<Lw>(c.op[1]))));
    case LZ_MUL_S: return out_of(lz_store(lz_mul<true>(as<Lz<2, 2, 160>>(c.op[0]), uc)));
    case LZ_MUL2: return out_of(lz_store(lz_mul2(as<Lz<1, 1, 80>>(c.op[0]), as<Lw>(c.op[1]), as<Lz<1, 1, 80>>(c.op[2]), as<Lw>(c.op[3]))));
    case LZ_MUL4U:
      return out_of(lz_store(lz_mul4u(as<Lz<0, 1, 1>>(c.op[0]), as<Lw>(c.op[1]), as<Lz<0, 1, 1>>(c.op[2]), as<Lw>(c.op[3]), as<Lz<0, 1, 1>>(c.op[4]), as<Lw>(c.op[5]),
                                      as<Lz<0, 1, 1>>(c.op[6]), as<Lw>(c.op[7]))));
    case LZ_STORE_44: return out_of(lz_store(as<Lz<4, 4, 16>>(c.op[0])));
    case LZ_STORE_WEAK: return out_of(lz_store_weak(as_weak(c.op[0])));
    case FR29_MUL: return out_of(fr29_pack(fr29_canonical(fr29_mul(as<F29>(c.op[0]), as<F29>(c.op[1])))));
    case FR29_SQR: return out_of(fr29_pack(fr29_canonical(fr29_sqr(as<F29>(c.op[0])))));
    case FR29_MUL2: return out_of(fr29_pack(fr29_canonical(fr29_mul2(as<F29>(c.op[0]), as<F29>(c.op[1]), as<F29>(c.op[2]), as<F29>(c.op[3])))));
    case LQ_MUL_22_11: return out_of(lq_pack_canonical(lq_mul(as<Lz<2, 2, 16>>(c.op[0]), as<Lz<1, 1, 10>>(c.op[1]))));
    case LQ_MUL_11_22: return out_of(lq_pack_canonical(lq_mul(as<Lz<1, 1, 10>>(c.op[0]), as<Lz<2, 2, 16>>(c.op[1]))));
    case LQ_MUL_12_13: return out_of(lq_pack_canonical(lq_mul(as<Lz<1, 1, 12>>(c.op[0]), as<Lz<1, 1, 13>>(c.op[1]))));
    case LQ_SQR: return out_of(lq_pack_canonical(lq_sqr(as<Lz<1, 1, 12>>(c.op[0]))));
    case LQ_MUL2:
      return out_of(lq_pack_canonical(lq_mul2(as<Lz<1, 1, 12>>(c.op[0]), as<Lz<1, 1, 10>>(c.op[1]), as<Lz<1, 1, 10>>(c.op[2]), as<Lz<1, 1, 4>>(c.op[3]))));
    case LQ_STORE_44: return out_of(lq_pack_canonical(as<Lz<4, 4, 16>>(c.op[0])));
    case F29_MUL: return out_of(f29_pack(f29_canonical(f29_mul(as<F29>(c.op[0]), as<F29>(c.op[1])))));
    case F29_SQR: return out_of(f29_pack(f29_canonical(f29_sqr(as<F29>(c.op[0])))));
    case F29_MUL2: return out_of(f29_pack(f29_canonical(f29_mul2(as<F29>(c.op[0]), as<F29>(c.op[1]), as<F29>(c.op[2]), as<F29>(c.op[3])))));
  }
  Out z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z.l[i] = 0xffffffffu;
  return z;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(256) k_tied_cases(const Rec *__restrict__ recs, Out *__restrict__ out, int n, Lw uc) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  out[i] = tied_case(recs[i], uc);
}
#endif

// ---- host: the cases ---------------------------------------------------------------------------------------------------------
static std::mt19937_64 rng(2961);
struct L9 {
  int l[9];
};
static const u32 PR[9] = ZK_R29_P, PQ[9] = ZK_Q29_P;

// the extreme member of Lz<LO, HI, V>: every lower limb at the edge of its range on the given side, the top limb as large as |value| < V p lets it be
static L9 extreme(const u32 (&P)[9], int LO, int HI, int V, bool negative) {
  L9 r;
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
static L9 largest(const u32 (&P)[9]) {   // limb-wise the largest canonical constant
  L9 r;
  for (int i = 0; i < 8; ++i) r.l[i] = (int)q29::MASK;
  r.l[8] = (int)P[8] - 1;
  return r;
}
static L9 multiple(const u32 (&P)[9], int k, int d) {   // k p + d, tight limbs 0..7, signed top limb
  L9 r;
  long long c = d;
  for (int i = 0; i < 9; ++i) {
    const long long v = (long long)k * (long long)P[i] + c;
    r.l[i] = i < 8 ? (int)(v & (long long)q29::MASK) : (int)v;
    c = v >> 29;
  }
  return r;
}
static L9 rand_canonical() {   // below 2^253, so below both moduli
  Fq w;
  for (int i = 0; i < 8; ++i) w.l[i] = (u32)rng();
  w.l[7] &= 0x1fffffffu;
  const F29 u = f29_unpack(w);
  L9 r;
  for (int i = 0; i < 9; ++i) r.l[i] = (int)u.l[i];
  return r;
}
static L9 comb(const L9 &a, int sa, const L9 &b, int sb) {
  L9 r;
  for (int i = 0; i < 9; ++i) r.l[i] = sa * a.l[i] + sb * b.l[i];
  return r;
}
static L9 norm(const L9 &a) {   // carry propagation: limbs 0..7 into [0, 2^29)
  L9 r;
  int c = 0;
  for (int i = 0; i < 8; ++i) {
    const int v = a.l[i] + c;
    r.l[i] = v & (int)q29::MASK;
    c = v >> 29;
  }
  r.l[8] = a.l[8] + c;
  return r;
}
// a random member of Lz<LO, HI, .>: HI canonical values added, LO subtracted
static L9 rand_loose(int LO, int HI) {
  L9 r = comb(rand_canonical(), 0, rand_canonical(), 0);
  for (int i = 0; i < HI; ++i) r = comb(r, 1, rand_canonical(), 1);
  for (int i = 0; i < LO; ++i) r = comb(r, 1, rand_canonical(), -1);
  return r;
}

static std::vector<Rec> cases, uniform_cases;   // all of them; those that read the constant of mul_s
static void push(int kind, std::initializer_list<L9> ops) {
  Rec r;
  memset(&r, 0, sizeof r);
  r.kind = kind;
  int k = 0;
  for (const L9 &o : ops) memcpy(r.op[k++], o.l, sizeof o.l);
  cases.push_back(r);
}

static void build_cases() {
  const int RANDOM = 300;
  const L9 zero = multiple(PR, 0, 0), one = multiple(PR, 0, 1);
  for (int f = 0; f < 2; ++f) {   // Fr, then the Fq twins
    const u32(&P)[9] = f ? PQ : PR;
    std::vector<L9> consts = {largest(P), multiple(P, 1, -1), zero, one, rand_canonical(), rand_canonical(), rand_canonical()};
    for (const L9 &w : consts)
      for (int s = 0; s < 2; ++s) {
        if (!f) {
          push(LZ_MUL_22, {extreme(P, 2, 2, 160, s), w});
          push(LZ_MUL_12, {extreme(P, 1, 2, 160, s), w});
          push(LZ_MUL_21, {extreme(P, 2, 1, 160, s), w});
          push(LZ_MUL_22, {extreme(P, 2, 2, 16, s), w});
          push(LZ_MUL_12, {extreme(P, 1, 2, 16, s), w});
          push(LZ_MUL_21, {extreme(P, 2, 1, 16, s), w});
          push(LZ_MUL_S, {extreme(P, 2, 2, 160, s)});
          push(LZ_MUL_S, {extreme(P, 2, 2, 16, s)});
          for (const L9 &d : {zero, one, multiple(P, 1, -1), largest(P)}) {
            push(LZ_MUL_22, {comb(d, s ? -1 : 1, d, 0), w});
            push(LZ_MUL_S, {comb(d, s ? -1 : 1, d, 0)});
            push(LZ_MUL2, {comb(d, s ? -1 : 1, d, 0), w, d, consts[0]});
            push(LZ_MUL4U, {d, w, d, w, d, w, d, w});
            push(LZ_MUL4U, {d, w, largest(P), consts[1], multiple(P, 1, -1), consts[0], one, w});
          }
          for (const L9 &v : consts)
            for (int s2 = 0; s2 < 2; ++s2) push(LZ_MUL2, {extreme(P, 1, 1, 80, s), w, extreme(P, 1, 1, 80, s2), v});
        } else {
          for (int s2 = 0; s2 < 2; ++s2) {
            push(LQ_MUL_22_11, {extreme(P, 2, 2, 16, s), extreme(P, 1, 1, 10, s2)});
            push(LQ_MUL_11_22, {extreme(P, 1, 1, 10, s), extreme(P, 2, 2, 16, s2)});
            push(LQ_MUL_12_13, {extreme(P, 1, 1, 12, s), extreme(P, 1, 1, 13, s2)});
            push(LQ_MUL2, {extreme(P, 1, 1, 12, s), extreme(P, 1, 1, 10, s2), extreme(P, 1, 1, 10, s2), extreme(P, 1, 1, 4, s)});
            push(LQ_MUL2, {extreme(P, 1, 1, 12, s), extreme(P, 1, 1, 10, s2), extreme(P, 1, 1, 10, !s2), extreme(P, 1, 1, 4, !s)});
          }
          push(LQ_MUL_22_11, {extreme(P, 2, 2, 16, s), w});
          push(LQ_MUL_11_22, {w, extreme(P, 2, 2, 16, s)});
          push(LQ_MUL_12_13, {comb(w, s ? -1 : 1, w, 0), w});
          push(LQ_SQR, {extreme(P, 1, 1, 12, s)});
          push(LQ_SQR, {comb(w, s ? -1 : 1, w, 0)});
          push(LQ_MUL2, {w, w, comb(w, s ? -1 : 1, w, 0), w});
        }
        // the unsigned products at 11 p: 11 p 11 p + 6 p 8 p = 169 p^2 < 2^261 p for the two-product form, and 13 p squared
        const int m = f ? F29_MUL : FR29_MUL, q = f ? F29_SQR : FR29_SQR, m2 = f ? F29_MUL2 : FR29_MUL2;
        push(m, {extreme(P, 0, 1, 11, false), extreme(P, 0, 1, 11, false)});
        push(m, {extreme(P, 0, 1, 11, false), w});
        push(m, {w, extreme(P, 0, 1, 11, false)});
        push(m, {w, w});
        push(q, {extreme(P, 0, 1, 11, false)});
        push(q, {extreme(P, 0, 1, 13, false)});
        push(q, {w});
        push(m2, {extreme(P, 0, 1, 11, false), extreme(P, 0, 1, 11, false), extreme(P, 0, 1, 6, false), extreme(P, 0, 1, 8, false)});
        push(m2, {extreme(P, 0, 1, 11, false), w, w, extreme(P, 0, 1, 11, false)});
        push(m2, {w, w, w, w});
      }
    // reductions and stores: the widest limbs, every multiple of p within 16 p and its two neighbours, tight and loose
    const int st = f ? LQ_STORE_44 : LZ_STORE_44;
    for (int s = 0; s < 2; ++s)
      for (int lo = 0; lo <= 4; lo += 4)
        for (int hi = 0; hi <= 4; hi += 4)
          if (lo + hi) push(st, {extreme(P, lo, hi, 16, s)});
    for (int k = -15; k <= 15; ++k)
      for (int d = -1; d <= 1; ++d) {
        L9 x = multiple(P, k, d);
        push(st, {x});
        x.l[0] += 1 << 29; x.l[1] -= 1;
        x.l[2] -= 1 << 29; x.l[3] += 1;
        push(st, {x});
      }
    if (!f) {
      push(LZ_STORE_WEAK, {zero});
      push(LZ_STORE_WEAK, {one});
      for (int k = 1; k <= 2; ++k)
        for (int d = -2; d <= (k == 1 ? 1 : -1); ++d) push(LZ_STORE_WEAK, {multiple(P, k, d)});   // r - 2, r - 1, r, r + 1, 2 r - 2, 2 r - 1
    }
    for (int it = 0; it < RANDOM; ++it) {
      const L9 a = rand_canonical(), b = rand_canonical(), c = rand_canonical(), d = rand_canonical();
      if (!f) {
        push(LZ_MUL_22, {rand_loose(2, 2), a});
        push(LZ_MUL_12, {rand_loose(1, 2), a});
        push(LZ_MUL_21, {rand_loose(2, 1), a});
        push(LZ_MUL_S, {rand_loose(2, 2)});
        push(LZ_MUL2, {rand_loose(1, 1), a, rand_loose(1, 1), b});
        push(LZ_MUL4U, {a, b, c, d, b, c, d, a});
        push(LZ_STORE_44, {rand_loose(4, 4)});
      } else {
        push(LQ_MUL_22_11, {rand_loose(2, 2), rand_loose(1, 1)});
        push(LQ_MUL_11_22, {rand_loose(1, 1), rand_loose(2, 2)});
        push(LQ_MUL_12_13, {rand_loose(1, 1), rand_loose(1, 0)});
        push(LQ_SQR, {rand_loose(1, 1)});
        push(LQ_MUL2, {rand_loose(1, 1), rand_loose(0, 1), rand_loose(1, 1), rand_loose(1, 0)});
        push(LQ_STORE_44, {rand_loose(4, 4)});
      }
      push(f ? F29_MUL : FR29_MUL, {a, norm(rand_loose(0, 4))});   // the unsigned form wants tight limbs: sums of canonical values, carries propagated
      push(f ? F29_SQR : FR29_SQR, {norm(rand_loose(0, 4))});
      push(f ? F29_MUL2 : FR29_MUL2, {a, norm(rand_loose(0, 4)), norm(rand_loose(0, 2)), c});
    }
  }
}

// ---- host: the reference -------------------------------------------------------------------------------------------------------
// sum l[i] 2^(29 i) mod p, canonical, for limbs of either sign, in the standard arithmetic
template <class PP, class F>
static F val(const int (&l)[9]) {
  F acc = F::zero();
  for (int i = 8; i >= 0; --i) {
    for (int k = 0; k < 29; ++k) acc = fp_dbl<PP>(acc);
    const long long v = l[i];
    const unsigned long long m = (unsigned long long)(v < 0 ? -v : v);
    F lo = F::zero(), hi = F::zero();
    lo.l[0] = (u32)(m & 0xffff);
    hi.l[0] = (u32)(m >> 16);
    for (int k = 0; k < 16; ++k) hi = fp_dbl<PP>(hi);
    const F t = fp_add<PP>(hi, lo);
    acc = v < 0 ? fp_sub<PP>(acc, t) : fp_add<PP>(acc, t);
  }
  return acc;
}
// is `got` what the reference says?  Products: 32 got = sum a_k b_k / 2^256 (the standard Montgomery product); stores: got = a
template <class PP, class F>
static bool reference_ok(const Rec &c, const Lw &uc, const Out &got) {
  F g;
  for (int i = 0; i < 8; ++i) g.l[i] = got.l[i];
  for (int i = 7; i >= 0; --i) {   // canonical: below the modulus
    if (g.l[i] != PP::MOD[i]) { if (g.l[i] > PP::MOD[i]) return false; break; }
    if (i == 0) return false;
  }
  int pairs = 1;
  bool sqr = false;
  switch (c.kind) {
    case LZ_STORE_44: case LZ_STORE_WEAK: case LQ_STORE_44: {
      const F want = val<PP, F>(c.op[0]);
      return memcmp(&want, &g, 32) == 0;
    }
    case LZ_MUL2: case FR29_MUL2: case LQ_MUL2: case F29_MUL2: pairs = 2; break;
    case LZ_MUL4U: pairs = 4; break;
    case FR29_SQR: case LQ_SQR: case F29_SQR: sqr = true; break;
    default: break;
  }
  F want = F::zero();
  for (int k = 0; k < pairs; ++k) {
    const F a = val<PP, F>(c.op[2 * k]);
    int ul[9];
    for (int i = 0; i < 9; ++i) ul[i] = (int)uc.l[i];
    const F b = sqr ? a : c.kind == LZ_MUL_S ? val<PP, F>(ul) : val<PP, F>(c.op[2 * k + 1]);
    want = fp_add<PP>(want, fp_mul<PP>(a, b));
  }
  for (int i = 0; i < 5; ++i) g = fp_dbl<PP>(g);
  return memcmp(&want, &g, 32) == 0;
}

#if defined(__HIPCC__)
#define HIP_OK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error: %s at %s\n", hipGetErrorString(e_), #x); return 2; } } while (0)
// the first launch runs every case against the first constant of mul_s, each later one only the cases that read the constant
static int run_on_device(const std::vector<Lw> &uniform, std::vector<Out> &dev) {
  const int n = (int)cases.size(), ns = (int)uniform_cases.size();
  Rec *d_recs = nullptr;
  Out *d_out = nullptr;
  HIP_OK(hipMalloc(&d_recs, (size_t)(n + ns) * sizeof(Rec)));
  HIP_OK(hipMalloc(&d_out, (size_t)n * sizeof(Out)));
  HIP_OK(hipMemcpy(d_recs, cases.data(), (size_t)n * sizeof(Rec), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_recs + n, uniform_cases.data(), (size_t)ns * sizeof(Rec), hipMemcpyHostToDevice));
  for (size_t u = 0; u < uniform.size(); ++u) {
    const int m = u ? ns : n;
    HIP_OK(hipMemset(d_out, 0xee, (size_t)n * sizeof(Out)));
    k_tied_cases<<<(m + 255) / 256, 256>>>(u ? d_recs + n : d_recs, d_out, m, uniform[u]);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dev.data() + (u ? n + (u - 1) * (size_t)ns : 0), d_out, (size_t)m * sizeof(Out), hipMemcpyDeviceToHost));
  }
  HIP_OK(hipFree(d_recs));
  HIP_OK(hipFree(d_out));
  return 0;
}
#else
static int run_on_device(const std::vector<Lw> &, std::vector<Out> &) {
  printf("built without a device pass: only --host\n");
  return 2;
}
#endif

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && !strcmp(argv[1], "--host");
  build_cases();
  const int n = (int)cases.size();
  // the constants of mul_s, one launch each
  std::vector<Lw> uniform;
  for (const L9 &w : {largest(PR), multiple(PR, 1, -1), multiple(PR, 0, 0), multiple(PR, 0, 1), rand_canonical(), rand_canonical()}) uniform.push_back(as<Lw>(w.l));
  for (const Rec &c : cases)
    if (c.kind == LZ_MUL_S) uniform_cases.push_back(c);
  const int ns = (int)uniform_cases.size();
  std::vector<Out> dev(n + (uniform.size() - 1) * (size_t)ns);
  if (!host_only) {
    const int rc = run_on_device(uniform, dev);
    if (rc) return rc;
  }
  int bad = 0, per_kind[N_KINDS] = {};
  for (size_t u = 0; u < uniform.size(); ++u) {
    const std::vector<Rec> &list = u ? uniform_cases : cases;
    const Out *d = dev.data() + (u ? n + (u - 1) * (size_t)ns : 0);
    for (int i = 0; i < (int)list.size(); ++i) {
      const Rec &c = list[i];
      const Out host = tied_case(c, uniform[u]);
      const bool fq = c.kind >= LQ_MUL_22_11;
      const bool ref = fq ? reference_ok<FqP, Fq>(c, uniform[u], host) : reference_ok<FrP, Fr>(c, uniform[u], host);
      const bool same = host_only || memcmp(&host, &d[i], sizeof(Out)) == 0;
      if (u == 0) ++per_kind[c.kind];
      if (!ref || !same) {
        if (bad++ < 20)
          printf("%s, case %d, constant %zu: %s%s\n", KIND_NAME[c.kind], i, u, ref ? "" : "host differs from the 8 x 32-bit reference; ", same ? "" : "device differs from host");
      }
    }
  }
  for (int k = 0; k < N_KINDS; ++k) printf("  %-26s %5d cases\n", KIND_NAME[k], per_kind[k]);
  printf("%d cases, %d of them against each of %zu constants of mul_s, %zu launches (%s)\n", n, ns, uniform.size(), host_only ? (size_t)0 : uniform.size(), host_only ? "host and reference" : "device, host and reference");
  printf("tied products: %d bad\n", bad);
  return bad != 0;
}
