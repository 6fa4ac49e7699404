// The structured reference string on one MI355X (include/zkfhe.h "SRS"): replaces halo2-scaffold `gen_srs` /
// ParamsKZG::setup (third-party, reached from reference examples/bfv.rs:311; README.md:34 "unsafe" seeded setup).
#include <sys/random.h>
#include <unistd.h>

#include "prover_internal.hpp"
#include "srs_secret.hpp"

// The monomial half of an SRS (g: the quotient pieces, the random polynomial -- calls of one to three columns) gets this share of
// the table budget of the Lagrange half (every wide commitment): 13-bit digits (43 GB) under the 160 GB service profile, 11 (13 GB)
// under the library default of 48 GB.  A wider table there buys nothing a proof can measure and costs tens of GB.
static constexpr double ZK_MONOMIAL_TABLE_SHARE = 0.3;

extern "C" {

static int srs_create_impl(zkfhe_ctx *ctx, zkfhe_comm *comm, uint32_t k, const uint8_t *seed, size_t seed_len, zkfhe_srs **out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, out != nullptr && k >= 3 && k <= 20 && (seed != nullptr || seed_len == 0));
  const size_t n = (size_t)1 << k;
  size_t lo = 0, hi = n;
  if (comm) zkfhe_comm_point_range(comm, n, &lo, &hi);   // this rank's bases
  const size_t nl = hi - lo;
  ZK_ARG(ctx, nl > 0);
  const U256 s_canon = srs_secret(seed, seed_len);   // srs_secret.hpp: the reference's ChaCha20 derivation or the seeded one
  const Fr s = mont(s_canon);
  const NttDomain *dom;
  CK(zk_domain(ctx, (int)k, &dom));
  // everything this function owns until it succeeds: released on every early return (an error code of a later step used
  // to leak the two buffers and the half-built SRS with its bases)
  struct Guard {
    zkfhe_ctx *ctx;
    DevBuf sc, pts;
    zkfhe_srs *srs = nullptr;
    ~Guard() {
      sc.release();
      pts.release();
      if (srs) zkfhe_srs_destroy(ctx, srs);
    }
  } guard{ctx};
  DevBuf &sc = guard.sc, &pts = guard.pts;
  CK(sc.alloc(ctx, nl * 32));
  CK(pts.alloc(ctx, nl * 64));
  G1Affine gen;
  gen.x = zk::fp_to_mont<zk::FqP>([] { zk::Fq t = zk::Fq::zero(); t.l[0] = 1; return t; }());
  gen.y = zk::fp_to_mont<zk::FqP>([] { zk::Fq t = zk::Fq::zero(); t.l[0] = 2; return t; }());
  std::vector<G1Affine> host(nl);
  zkfhe_srs *srs = guard.srs = new zkfhe_srs();
  srs->k = k;
  srs->comm = comm;
  srs->lo = lo;
  srs->hi = hi;
  const unsigned gr = (unsigned)((nl + 255) / 256);
  for (int which = 0; which < 2; ++which) {
    if (which == 0) {
      zkp::k_powers<<<gr, 256, 0, ctx->stream>>>(fr_pow(s, lo), s, sc.fr(), nl);   // s^(lo + i)
      ZK_LAUNCH_CHECK(ctx);
    } else {
      zkp::k_srs_den<<<gr, 256, 0, ctx->stream>>>(dom->fwd + lo, s, mont_u64(n), sc.fr(), nl);
      ZK_LAUNCH_CHECK(ctx);
      CK(zkfhe_fr_batch_invert(ctx, (zkfhe_fr *)sc.p, nl));
      zkp::k_srs_li<<<gr, 256, 0, ctx->stream>>>(dom->fwd + lo, fr_pow(s, n) - Fr::one(), sc.fr(), nl);
      ZK_LAUNCH_CHECK(ctx);
    }
    zkp::k_fill_point<<<gr, 256, 0, ctx->stream>>>(gen, (G1Affine *)pts.p, nl);
    ZK_LAUNCH_CHECK(ctx);
    CK(zkfhe_g1_mul(ctx, (const zkfhe_g1_affine *)pts.p, (const zkfhe_fr *)sc.p, (zkfhe_g1_affine *)pts.p, nl));
    CK(zkfhe_download(ctx, host.data(), pts.p, nl * 64));
    // the monomial half serves the calls of 1-3 columns only (random polynomial, quotient pieces): half the table budget
    CK(zk_basis_create_scaled(ctx, (const zkfhe_g1_affine *)host.data(), nl, 0, which == 0 ? ZK_MONOMIAL_TABLE_SHARE : 1.0, which == 0 ? &srs->g : &srs->g_lagrange));
    if (!comm) (which == 0 ? srs->g_host : srs->gl_host) = host;   // zkfhe_srs_save writes them
    if (which == 1) {
      static int small_c = -1;
      if (small_c < 0) {
        const char *e = getenv("ZKFHE_SMALL_C");
        small_c = e ? atoi(e) : 10;
      }
      if (small_c > 0 && k >= 12 && k <= 14 && !zkfhe_basis_has_multiples(srs->g_lagrange)) CK(zkfhe_basis_create(ctx, (const zkfhe_g1_affine *)host.data(), nl, small_c, &srs->g_lagrange_small));
    }
  }
  zk_srs_g2_from_secret(s_canon, srs->g2_raw, srs->sg2_raw);
  srs->have_g2 = true;
  guard.srs = nullptr;   // success: the caller owns it (the buffers go with the guard)
  *out = srs;
  return ZKFHE_OK;
}

int zkfhe_srs_create(zkfhe_ctx *ctx, uint32_t k, const uint8_t *seed, size_t seed_len, zkfhe_srs **out) {
  return srs_create_impl(ctx, nullptr, k, seed, seed_len, out);
}

int zkfhe_srs_create_sharded(zkfhe_ctx *ctx, zkfhe_comm *comm, uint32_t k, const uint8_t *seed, size_t seed_len, zkfhe_srs **out) {
  if (!comm) return zk_fail_msg(ctx, ZKFHE_EINVAL, "comm is NULL");
  return srs_create_impl(ctx, comm, k, seed, seed_len, out);
}

int zkfhe_srs_from_points(zkfhe_ctx *ctx, uint32_t k, const zkfhe_g1_affine *g_host, const zkfhe_g1_affine *g_lagrange_host, zkfhe_srs **out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, out != nullptr && g_host != nullptr && g_lagrange_host != nullptr && k >= 3 && k <= 20);
  const size_t n = (size_t)1 << k;
  zkfhe_srs *srs = new zkfhe_srs();
  srs->k = k;
  srs->hi = n;
  srs->g_host.assign((const G1Affine *)g_host, (const G1Affine *)g_host + n);
  srs->gl_host.assign((const G1Affine *)g_lagrange_host, (const G1Affine *)g_lagrange_host + n);
  int rc = zk_basis_create_scaled(ctx, g_host, n, 0, ZK_MONOMIAL_TABLE_SHARE, &srs->g);
  if (!rc) rc = zk_basis_create_scaled(ctx, g_lagrange_host, n, 0, 1.0, &srs->g_lagrange);
  if (!rc && k >= 12 && k <= 14 && !zkfhe_basis_has_multiples(srs->g_lagrange)) rc = zkfhe_basis_create(ctx, g_lagrange_host, n, 10, &srs->g_lagrange_small);
  if (rc) {
    zkfhe_srs_destroy(ctx, srs);
    return rc;
  }
  *out = srs;
  return ZKFHE_OK;
}

int zkfhe_srs_g2(const zkfhe_srs *srs, uint8_t g2_le[128], uint8_t s_g2_le[128]) {
  if (!srs || !g2_le || !s_g2_le || !srs->have_g2) return ZKFHE_EINVAL;
  return zk_g2_raw_to_canon(srs->g2_raw, g2_le) && zk_g2_raw_to_canon(srs->sg2_raw, s_g2_le) ? ZKFHE_OK : ZKFHE_EINVAL;
}

int zkfhe_srs_set_g2(zkfhe_srs *srs, const uint8_t g2_le[128], const uint8_t s_g2_le[128]) {
  if (!srs || !g2_le || !s_g2_le) return ZKFHE_EINVAL;
  uint8_t a[128], b[128];
  if (!zk_g2_canon_to_raw(g2_le, a) || !zk_g2_canon_to_raw(s_g2_le, b)) return ZKFHE_EINVAL;
  memcpy(srs->g2_raw, a, 128);
  memcpy(srs->sg2_raw, b, 128);
  srs->have_g2 = true;
  return ZKFHE_OK;
}

// halo2 ParamsKZG::write (SerdeFormat::RawBytes): u32 k | g | g_lagrange | g2 | s_g2, raw Montgomery coordinates
int zkfhe_srs_save(zkfhe_ctx *ctx, const zkfhe_srs *srs, const char *path) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, srs && path);
  const size_t n = (size_t)1 << srs->k;
  if (srs->sharded()) return zk_fail_msg(ctx, ZKFHE_EINVAL, "zkfhe_srs_save: a sharded SRS holds only a slice of the points");
  if (srs->g_host.size() != n || srs->gl_host.size() != n)
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "zkfhe_srs_save: this SRS keeps no host copy of its points (made over a communicator, or zkfhe_srs_drop_host_copy was called)");
  if (!srs->have_g2) return zk_fail_msg(ctx, ZKFHE_EINVAL, "zkfhe_srs_save: the SRS has no G2 half (zkfhe_srs_set_g2)");
  // written aside under a name of this process' own and renamed into place: two ranks (or two CLI runs) that both find the file
  // missing and derive it at once never write into each other's temporary, and a reader sees the old file, none, or a whole one
  static std::atomic<unsigned> serial{0};
  const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid()) + "." + std::to_string(serial.fetch_add(1));
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("cannot write ") + tmp);
  const uint32_t k = srs->k;
  bool ok = fwrite(&k, 4, 1, f) == 1 && fwrite(srs->g_host.data(), 64, n, f) == n && fwrite(srs->gl_host.data(), 64, n, f) == n &&
            fwrite(srs->g2_raw, 128, 1, f) == 1 && fwrite(srs->sg2_raw, 128, 1, f) == 1;
  ok = (fclose(f) == 0) && ok;
  if (!ok || rename(tmp.c_str(), path) != 0) {
    remove(tmp.c_str());
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("writing ") + path + " failed");
  }
  return ZKFHE_OK;
}

// An unsharded SRS keeps host copies of both point vectors (64 B x 2^k each: 128 MB at k = 20) only so that zkfhe_srs_save can write
// them; a prover that has saved (or never will) gives them back with this.  Saving afterwards is refused with a message that says so.
int zkfhe_srs_drop_host_copy(zkfhe_srs *srs) {
  if (!srs) return ZKFHE_EINVAL;
  std::vector<G1Affine>().swap(srs->g_host);
  std::vector<G1Affine>().swap(srs->gl_host);
  return ZKFHE_OK;
}

int zkfhe_srs_load(zkfhe_ctx *ctx, const char *path, zkfhe_srs **out) {
  ZK_ENTER(ctx);
  ZK_ARG(ctx, path && out);
  *out = nullptr;
  FILE *f = fopen(path, "rb");
  if (!f) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("cannot open ") + path);
  uint32_t k = 0;
  std::vector<G1Affine> g, gl;
  uint8_t raw[256], canon[128];
  bool ok = fread(&k, 4, 1, f) == 1 && k >= 3 && k <= 20;
  if (ok) {
    const size_t n = (size_t)1 << k;
    g.resize(n), gl.resize(n);
    ok = fread(g.data(), 64, n, f) == n && fread(gl.data(), 64, n, f) == n && fread(raw, 256, 1, f) == 1 && fgetc(f) == EOF;
  }
  fclose(f);
  if (!ok) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(path) + ": not a params file (u32 k | 2^k g | 2^k g_lagrange | g2 | s_g2, RawBytes), or k outside 3..20");
  // what halo2's RawBytes read checks: reduced coordinates, y^2 = x^3 + 3 (the identity (0, 0) cannot occur in an SRS)
  const zk::Fq three = zk::fp_to_mont<zk::FqP>([] { zk::Fq t = zk::Fq::zero(); t.l[0] = 3; return t; }());
  const U256 &QM = fe::Q_MOD;
  for (const auto *v : {&g, &gl})
    for (const G1Affine &p : *v) {
      U256 x, y;
      memcpy(x.l, p.x.l, 32);
      memcpy(y.l, p.y.l, 32);
      if (!(x < QM) || !(y < QM) || !(p.y * p.y == p.x * p.x * p.x + three)) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(path) + ": a G1 point is not on the curve");
    }
  if (!zk_g2_raw_to_canon(raw, canon) || !zk_g2_raw_to_canon(raw + 128, canon)) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string(path) + ": a G2 point is not on the curve");
  zkfhe_srs *srs = nullptr;
  CK(zkfhe_srs_from_points(ctx, k, (const zkfhe_g1_affine *)g.data(), (const zkfhe_g1_affine *)gl.data(), &srs));
  memcpy(srs->g2_raw, raw, 128);
  memcpy(srs->sg2_raw, raw + 128, 128);
  srs->have_g2 = true;
  *out = srs;
  return ZKFHE_OK;
}

// ---- an SRS from a ceremony's monomial powers (include/zkfhe.h) ------------------------------------------------------------------

// what zkfhe_srs_load asks of a G1 point: reduced coordinates, y^2 = x^3 + 3
static bool srs_g1_on_curve(const G1Affine &p) {
  const U256 &QM = fe::Q_MOD;
  static const zk::Fq three = zk::fp_to_mont<zk::FqP>([] { zk::Fq t = zk::Fq::zero(); t.l[0] = 3; return t; }());
  U256 x, y;
  memcpy(x.l, p.x.l, 32);
  memcpy(y.l, p.y.l, 32);
  return x < QM && y < QM && p.y * p.y == p.x * p.x * p.x + three;
}

// g_host: at least 2^k points, checked here; g2_raw / sg2_raw: raw coordinates already checked, or both NULL.  `who` prefixes
// every refusal.  Everything the arguments alone decide is refused before the first device call.
static int srs_from_monomial_impl(zkfhe_ctx *ctx, const char *who, uint32_t k, const G1Affine *g_host, const uint8_t *g2_raw, const uint8_t *sg2_raw, zkfhe_srs **out) {
  const std::string pre = std::string(who) + ": ";
  const size_t n = (size_t)1 << k;
  for (size_t i = 0; i < n; ++i) {
    if (g_host[i].is_identity()) return zk_fail_msg(ctx, ZKFHE_EINVAL, pre + "g[" + std::to_string(i) + "] is the identity, which no power of s is");
    if (!srs_g1_on_curve(g_host[i])) return zk_fail_msg(ctx, ZKFHE_EINVAL, pre + "g[" + std::to_string(i) + "] has a coordinate >= p or is not on the curve");
  }
  // g_lagrange[i] = L_i(s) G = n^-1 sum_j w^(-ij) g[j]: halo2's g_to_lagrange, an inverse FFT over the points
  std::vector<G1Affine> gl(n);
  {
    struct Guard {
      DevBuf pts;
      ~Guard() { pts.release(); }
    } guard;
    CK(guard.pts.alloc(ctx, n * sizeof(G1Affine)));
    CK(zkfhe_upload(ctx, guard.pts.p, g_host, n * sizeof(G1Affine)));
    CK(zkfhe_g1_fft(ctx, (zkfhe_g1_affine *)guard.pts.p, (int)k, 1));
    CK(zkfhe_download(ctx, gl.data(), guard.pts.p, n * sizeof(G1Affine)));
  }
  zkfhe_srs *srs = nullptr;
  CK(zkfhe_srs_from_points(ctx, k, (const zkfhe_g1_affine *)g_host, (const zkfhe_g1_affine *)gl.data(), &srs));
  if (g2_raw) {
    memcpy(srs->g2_raw, g2_raw, 128);
    memcpy(srs->sg2_raw, sg2_raw, 128);
    srs->have_g2 = true;
  }
  *out = srs;
  return ZKFHE_OK;
}

int zkfhe_srs_from_monomial(zkfhe_ctx *ctx, uint32_t k, const zkfhe_g1_affine *g_host, size_t n_g, const uint8_t g2_le[128], const uint8_t s_g2_le[128], zkfhe_srs **out) {
  ZK_ENTER(ctx);
  if (!ctx) return ZKFHE_EINVAL;
  if (!out || !g_host) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_from_monomial: a NULL argument");
  *out = nullptr;
  if ((g2_le == nullptr) != (s_g2_le == nullptr)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_from_monomial: g2 and s_g2 come together or not at all");
  if (k < 3 || k > 20) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_from_monomial: k outside 3..20");
  if (n_g < ((size_t)1 << k)) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_from_monomial: " + std::to_string(n_g) + " powers are fewer than 2^k");
  uint8_t a[128], b[128];
  if (g2_le && (!zk_g2_canon_to_raw(g2_le, a) || !zk_g2_canon_to_raw(s_g2_le, b)))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_from_monomial: a G2 point has a coordinate >= p or is not on the twist curve");
  return srs_from_monomial_impl(ctx, "srs_from_monomial", k, (const G1Affine *)g_host, g2_le ? a : nullptr, g2_le ? b : nullptr, out);
}

int zkfhe_srs_load_downsized(zkfhe_ctx *ctx, const char *path, uint32_t k, zkfhe_srs **out) {
  ZK_ENTER(ctx);
  if (!ctx) return ZKFHE_EINVAL;
  if (!out || !path) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_load_downsized: a NULL argument");
  *out = nullptr;
  if (k < 3 || k > 20) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_load_downsized: k outside 3..20");
  FILE *f = fopen(path, "rb");
  if (!f) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("srs_load_downsized: cannot open ") + path);
  // u32 k_file | g[2^k_file] | g_lagrange[2^k_file] | g2 | s_g2: the head of g and the 256-byte tail are read, the rest is skipped
  uint32_t kf = 0;
  const size_t n = (size_t)1 << k;
  std::vector<G1Affine> g;
  uint8_t raw[256], canon[128];
  bool framed = fread(&kf, 4, 1, f) == 1 && kf >= 1 && kf <= 28;
  const long long want = framed ? 4 + 2 * 64 * ((long long)1 << kf) + 256 : 0;
  framed = framed && fseeko(f, 0, SEEK_END) == 0 && (long long)ftello(f) == want;
  const bool large_enough = framed && kf >= k;
  bool ok = large_enough;
  if (ok) {
    g.resize(n);
    ok = fseeko(f, 4, SEEK_SET) == 0 && fread(g.data(), 64, n, f) == n && fseeko(f, (off_t)(want - 256), SEEK_SET) == 0 && fread(raw, 256, 1, f) == 1;
  }
  fclose(f);
  if (!framed) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("srs_load_downsized: ") + path + " is not a params file (u32 k | 2^k g | 2^k g_lagrange | g2 | s_g2, RawBytes): short or misframed");
  if (!large_enough) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("srs_load_downsized: ") + path + " holds k = " + std::to_string(kf) + ", fewer powers than 2^" + std::to_string(k));
  if (!ok) return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("srs_load_downsized: reading ") + path + " failed");
  if (!zk_g2_raw_to_canon(raw, canon) || !zk_g2_raw_to_canon(raw + 128, canon))
    return zk_fail_msg(ctx, ZKFHE_EINVAL, std::string("srs_load_downsized: ") + path + ": a G2 point has a coordinate >= p or is not on the twist curve");
  return srs_from_monomial_impl(ctx, "srs_load_downsized", k, g.data(), raw, raw + 128, out);
}

// ---- zkfhe_srs_check ---------------------------------------------------------------------------------------------------------------

// count scalars below 2^253 (< r) from the ChaCha20 keystream of the seed, canonical; `stream` separates the draws of one check
static void srs_check_scalars(const uint8_t seed[32], uint32_t stream, U256 *out, size_t count) {
  uint8_t block[64];
  for (size_t i = 0; i < count; i += 2) {
    const uint64_t ctr = i / 2;
    const uint32_t cn[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), stream, 0};
    chacha20_block(seed, cn, block);
    block[31] &= 0x1f, block[63] &= 0x1f;
    memcpy(out[i].l, block, 32);
    if (i + 1 < count) memcpy(out[i + 1].l, block + 32, 32);
  }
}

int zkfhe_srs_check(zkfhe_ctx *ctx, const zkfhe_srs *srs, const uint8_t seed[32], uint32_t *failed) {
  ZK_ENTER(ctx);
  if (!ctx) return ZKFHE_EINVAL;
  if (!srs || !failed) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_check: a NULL argument");
  *failed = 0;
  if (srs->sharded()) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_check: a sharded SRS holds only a slice of the points");
  if (!srs->have_g2) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_check: the SRS has no G2 half (zkfhe_srs_set_g2)");
  uint8_t own[32];
  if (!seed) {
    if (getrandom(own, 32, 0) != 32) return zk_fail_msg(ctx, ZKFHE_EINVAL, "srs_check: no seed given and the operating system gave no randomness (getrandom)");
    seed = own;
  }
  const uint32_t k = srs->k;
  const size_t n = (size_t)1 << k;
  uint32_t bad = 0;
  struct Guard {
    DevBuf cols, evals, pts;
    ~Guard() { cols.release(), evals.release(), pts.release(); }
  } guard;
  CK(guard.cols.alloc(ctx, 2 * n * 32));
  CK(guard.evals.alloc(ctx, n * 32));
  CK(guard.pts.alloc(ctx, 4 * sizeof(G1Affine)));
  G1Affine *pts = (G1Affine *)guard.pts.p;
  std::vector<U256> h(2 * n);
  G1Affine res[4];
  // powers: columns (r, 0) and (0, r) over g give A = sum r_i g[i] and B = sum r_i g[i + 1] = s A
  srs_check_scalars(seed, 0, h.data(), n - 1);
  h[n - 1] = h[n] = fe::zero();
  memcpy(h[n + 1].l, h[0].l, (n - 1) * 32);
  CK(upload_canon(ctx, guard.cols.fr(), h.data(), 2 * n));
  CK(zkfhe_msm_batch(ctx, srs->g, (const zkfhe_fr *)guard.cols.p, 2, (zkfhe_g1_affine *)pts));
  // Lagrange: the commitment of the coefficients c under g is the commitment of the evaluations NTT(c) under g_lagrange
  ZK_HIP(ctx, zk_wait(ctx));   // h is read by the copy above until here
  srs_check_scalars(seed, 1, h.data(), n);
  CK(upload_canon(ctx, guard.cols.fr(), h.data(), n));
  CK(zkfhe_ntt_batch_to(ctx, (const zkfhe_fr *)guard.cols.p, (zkfhe_fr *)guard.evals.p, 1, (int)k, 0));
  CK(zkfhe_msm_batch(ctx, srs->g, (const zkfhe_fr *)guard.cols.p, 1, (zkfhe_g1_affine *)(pts + 2)));
  CK(zkfhe_msm_batch(ctx, srs->g_lagrange, (const zkfhe_fr *)guard.evals.p, 1, (zkfhe_g1_affine *)(pts + 3)));
  CK(zkfhe_download(ctx, res, pts, sizeof(res)));
  if (memcmp(&res[2], &res[3], sizeof(G1Affine)) != 0) bad |= ZKFHE_SRS_BAD_LAGRANGE;
  uint8_t canon[128];
  const bool g2_ok = zk_g2_raw_to_canon(srs->g2_raw, canon) && zk_g2_raw_to_canon(srs->sg2_raw, canon);
  if (!g2_ok || !zk_srs_pairing_powers(res[0], res[1], srs->g2_raw, srs->sg2_raw)) bad |= ZKFHE_SRS_BAD_POWERS;
  // g[0]: the first column of the powers check with every scalar but the first zero would do; the host copy is at hand more often
  G1Affine gen, g0;
  gen.x = zk::fp_to_mont<zk::FqP>([] { zk::Fq t = zk::Fq::zero(); t.l[0] = 1; return t; }());
  gen.y = zk::fp_to_mont<zk::FqP>([] { zk::Fq t = zk::Fq::zero(); t.l[0] = 2; return t; }());
  if (!srs->g_host.empty()) {
    g0 = srs->g_host[0];
  } else {
    CK(zkfhe_memset_dev(ctx, guard.cols.p, 0, n * 32));
    const Fr one = Fr::one();
    CK(zkfhe_upload(ctx, guard.cols.p, &one, 32));
    CK(zkfhe_msm_batch(ctx, srs->g, (const zkfhe_fr *)guard.cols.p, 1, (zkfhe_g1_affine *)pts));
    CK(zkfhe_download(ctx, &g0, pts, sizeof(G1Affine)));
  }
  if (!g2_ok || memcmp(&g0, &gen, sizeof(G1Affine)) != 0) bad |= ZKFHE_SRS_BAD_GENERATOR;
  *failed = bad;
  return ZKFHE_OK;
}

int zkfhe_srs_table_bits(const zkfhe_srs *srs, int *wide_calls) {
  if (wide_calls) *wide_calls = 0;
  return srs ? zkfhe_basis_table_bits(srs->g_lagrange, wide_calls) : 0;
}

// What the digit-multiple tables of this SRS look like: bits[0] / bits[1] = digit width of the monomial (g) and Lagrange halves
// (0: none), *bytes = resident bytes of both, *narrowed = 1 when a half got a narrower table than its budget allowed because the
// device did not have the room (another SRS alive, other tenants) -- the calls are then slower, never wrong.  All outputs optional.
int zkfhe_srs_table_info(const zkfhe_srs *srs, int bits[2], uint64_t *bytes, int *narrowed) {
  if (!srs) return ZKFHE_EINVAL;
  int n0 = 0, n1 = 0;
  const size_t b0 = zkfhe_basis_table_bytes(srs->g, &n0), b1 = zkfhe_basis_table_bytes(srs->g_lagrange, &n1);
  if (bits) {
    bits[0] = zkfhe_basis_table_bits(srs->g, nullptr);
    bits[1] = zkfhe_basis_table_bits(srs->g_lagrange, nullptr);
  }
  if (bytes) *bytes = (uint64_t)b0 + (uint64_t)b1;
  if (narrowed) *narrowed = (n0 | n1) ? 1 : 0;
  return ZKFHE_OK;
}

int zkfhe_srs_destroy(zkfhe_ctx *ctx, zkfhe_srs *srs) {
  ZK_ENTER(ctx);
  if (!srs) return ZKFHE_OK;
  zkfhe_basis_destroy(ctx, srs->g);
  zkfhe_basis_destroy(ctx, srs->g_lagrange);
  zkfhe_basis_destroy(ctx, srs->g_lagrange_small);
  delete srs;
  return ZKFHE_OK;
}

}  // extern "C"
