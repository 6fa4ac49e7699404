// The arithmetic of one G1 FFT butterfly (g1_fft.hip), host + device: the twiddle as a canonical scalar, the scalar multiplication
// ladder and the (a, t) -> (a + t, a - t) step, all on the complete XYZZ functions of bn254.hip.hpp -- equal and opposite summands,
// identity operands and zero digits take the branches those functions have, nothing here assumes them away.
// tests/native/g1_fft_plan_check.cpp runs exactly this code on the CPU.
#pragma once
#include "bn254.hip.hpp"

namespace zk {

struct G1FftScalar {
  u32 w[8];   // canonical (not Montgomery), little-endian, < r < 2^254
};

// the domain table's entry (Montgomery form), times n^-1 where the stage carries it, as the integer the ladder walks
ZK_HD G1FftScalar g1_fft_scalar(const Fr &tw, bool scale, const Fr &n_inv) {
  const Fr c = fp_from_mont<FrP>(scale ? fp_mul<FrP>(tw, n_inv) : tw);
  G1FftScalar k;
#pragma unroll
  for (int i = 0; i < 8; ++i) k.w[i] = c.l[i];
  return k;
}

ZK_HD bool g1_fft_scalar_is_one(const G1FftScalar &k) {
  u32 o = k.w[0] ^ 1u;
#pragma unroll
  for (int i = 1; i < 8; ++i) o |= k.w[i];
  return o == 0;
}

// k <<= B: the ladder reads the scalar from the top by shifting it, never by a computed index (a per-thread array indexed at run
// time lives in scratch memory)
template <int B>
ZK_HD void g1_fft_scalar_shl(G1FftScalar &k) {
#pragma unroll
  for (int i = 7; i > 0; --i) k.w[i] = (k.w[i] << B) | (k.w[i - 1] >> (32 - B));
  k.w[0] <<= B;
}

constexpr int G1FFT_TABLE_ENTRIES = 4;   // b, 2b, 3b, 4b

// k * b with a fixed signed three-bit window (Booth, radix 8): k = sum d_i 8^i over 85 digits d_i in [-4, 4],
// d_i = -4 k[3i+2] + 2 k[3i+1] + k[3i] + k[3i-1], read from the top.  Every digit costs three doublings and one addition of
// +-(|d| b) from the table (none for a zero digit, one in eight): 255 doublings and about 75 additions whatever the scalar, so
// lanes with different scalars stay in step, and lanes that share one (G1FFT_SHARED stages) branch together on its digits.
// tab holds b, 2b, 3b, 4b (put(e, p), get(e), e = |d| - 1) and is the caller's: device memory in the kernels, an array on the host.
// One doubling site and one addition site: the table is filled by repeated addition of b, whose first step is the doubling case
// of the complete addition.
template <class Tab>
ZK_HD G1X g1x_mul_window(Tab &tab, const G1X &b, G1FftScalar k) {
  {
    G1X m = b;
    tab.put(0, m);
#pragma unroll 1
    for (int e = 1; e < G1FFT_TABLE_ENTRIES; ++e) {
      g1x_add(m, b);
      tab.put(e, m);
    }
  }
  g1_fft_scalar_shl<1>(k);   // bit 254 (zero: r < 2^254) to the top: 85 windows of three bits cover bits 254..0
  G1X acc = G1X::identity();
  int phase = 0;
#pragma unroll 1
  for (int i = 0; i < 255; ++i) {
    acc = g1x_dbl(acc);
    if (++phase == 3) {
      phase = 0;
      const u32 v = k.w[7] >> 28;   // the window's three bits and the bit below it
      g1_fft_scalar_shl<3>(k);
      const int d = (int)((v + 1) >> 1) - (int)(v & 8u);
      if (d != 0) {
        G1X q = tab.get((d < 0 ? -d : d) - 1);
        if (d < 0) q.y = fp_neg<FqP>(q.y);
        g1x_add(acc, q);
      }
    }
  }
  return acc;
}

struct G1FftHostTable {
  G1X t[G1FFT_TABLE_ENTRIES];
  void put(int i, const G1X &p) { t[i] = p; }
  const G1X &get(int i) const { return t[i]; }
};

// (a, t) -> (a + t, a - t)
ZK_HD void g1_fft_combine(G1X &a, G1X &t) {
  G1X s = a;
  g1x_add(s, t);
  g1x_add(a, g1x_neg(t));
  t = a;
  a = s;
}

}  // namespace zk
