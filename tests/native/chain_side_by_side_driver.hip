// Runs every launch that puts independent bodies of zk-fhe_amd/host/prover_kernels.hip.hpp side by side and, on the same inputs, the
// sequence of launches it replaces (the prover's ZKFHE_CHAIN=serial path), with the prover's block sizes and grids.  It decides
// nothing: tests/test_gpu_chain_side_by_side.py writes the inputs and compares the two sets of output files.
//
//   chain_side_by_side_driver <dir>    reads <dir>/cases.txt and <dir>/in/CASE.*, writes <dir>/out/CASE.{old,new,split}.BUFFER.bin
//
// cases.txt, one case per line, tokens separated by blanks (a field scalar is 64 hexadecimal digits, most significant first):
//   gp CASE n u n_advice chunk n_lookup beta gamma delta seed0 seed1 seed2 seed3 ctr_pz
//        inputs adv [n_advice][n], const [n], inst [n], sigma [n_advice + 2][n], wpow [n], a / la / ls [n_lookup][n], table [n]
//        old: k_powers, k_perm_num_den, ratios, k_prefix_product, k_chunk_carry, k_scale_rows, then k_lookup_num_den, ratios,
//             k_prefix_product, k_chunk_carry(check_ones)          new: the six launches of Proof::grand_products_side_by_side
//        (the ratios num / den come from a kernel of this file, one inversion per element: the library's batch inversion gives the
//        same canonical words and is not part of the header under test)
//        outputs bd, num, den, z, totals, closes -- the lookup half behind the permutation half in both sequences
//   sh CASE n n_cols n_sets m_0 .. m_{n_sets-1}
//        inputs cols [n_cols][n], s29 [sum m], sets [n_sets] ShSet records, wpow [n]; member k reads column (7 k + 3) mod n_cols
//        old: per set k_lincomb_ptrs or k_lincomb_ptrs_chunked + k_sum_rows (chunks of 48), then k_sh_zs
//        new: k_chain_jobs<TAIL_ZS> and k_chain_sums                  outputs F, zs, and the new sequence's partial slots
//        split: k_chain_jobs<TAIL_NONE>, k_sh_zs, k_chain_sums        outputs F, zs
//   ev CASE n        inputs h [3][n], s29 [3], pts [6], wpow [n]
//        old: k_lincomb_ptrs, k_bary_den                              new: k_chain_jobs<TAIL_BARY>         outputs H, bw
// Every output buffer starts as bytes 0xA5 and carries a guard column behind its last row.  Every input file must have exactly the
// size the case implies (exit status 2, nothing launched).  After every launch the status is read and the device synchronised; on the
// first error the case's name is printed and the program ends with status 1 without launching anything more.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "prover_kernels.hip.hpp"

using zk::Fr;

namespace {

std::string cur_case = "(none)", dir;
unsigned num_cu = 0;

[[noreturn]] void bad_case(const std::string &why) {
  fprintf(stderr, "chain_side_by_side_driver: case %s: %s\n", cur_case.c_str(), why.c_str());
  exit(2);
}
void hip_ok(hipError_t e, const char *what) {
  if (e == hipSuccess) return;
  printf("chain_side_by_side_driver: HIP error in case %s (%s): %s\n", cur_case.c_str(), what, hipGetErrorString(e));
  fflush(stdout);
  _exit(1);   // nothing more is launched, freed or copied on a device that reported an error
}
void launched(const char *kernel) {
  hip_ok(hipGetLastError(), kernel);
  hip_ok(hipDeviceSynchronize(), kernel);
}
unsigned grid_for(size_t work) {   // prover_internal.hpp
  const size_t b = (work + 255) / 256, cap = (size_t)num_cu * 16;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

struct Args {
  std::vector<std::string> t;
  size_t pos = 0;
  const std::string &next() {
    if (pos >= t.size()) bad_case("too few arguments");
    return t[pos++];
  }
  unsigned long long num() {
    const std::string &s = next();
    char *end = nullptr;
    const unsigned long long v = strtoull(s.c_str(), &end, 10);
    if (s.empty() || *end) bad_case("not a number: " + s);
    return v;
  }
  Fr scalar() {
    const std::string &s = next();
    if (s.size() != 64) bad_case("a field scalar takes 64 hexadecimal digits");
    Fr v;
    for (int i = 0; i < 8; ++i) v.l[i] = (zk::u32)strtoul(s.substr(64 - 8 * (i + 1), 8).c_str(), nullptr, 16);
    return v;
  }
  void done() {
    if (pos != t.size()) bad_case("too many arguments");
  }
};

// the input file <dir>/in/CASE.NAME, exactly `bytes` long, on the device (an empty array: one unused byte)
template <class T>
const T *input(const char *name, size_t bytes) {
  std::vector<char> host(bytes + 1);
  if (bytes) {
    std::ifstream f(dir + "/in/" + cur_case + "." + name, std::ios::binary);
    f.read(host.data(), bytes + 1);
    if (!f.eof() || (size_t)f.gcount() != bytes) bad_case(std::string("input ") + name + " has not the size the case implies");
  }
  char *d = nullptr;
  hip_ok(hipMalloc(&d, bytes + 1), "hipMalloc");
  hip_ok(hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy");
  return (const T *)d;
}
template <class T>
T *upload(const std::vector<T> &v) {
  T *d = nullptr;
  hip_ok(hipMalloc(&d, v.size() * sizeof(T) + 1), "hipMalloc");
  hip_ok(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
  return d;
}
// an output buffer of `words` field words and `guard` more behind them, all bytes 0xA5
struct Out {
  Fr *p = nullptr;
  size_t bytes = 0;
};
Out output(size_t words, size_t guard) {
  Out o;
  o.bytes = (words + guard) * 32;
  hip_ok(hipMalloc(&o.p, o.bytes), "hipMalloc");
  hip_ok(hipMemset(o.p, 0xA5, o.bytes), "hipMemset");
  return o;
}
void dump(const char *which, const char *name, const Out &o) {
  std::vector<char> host(o.bytes);
  hip_ok(hipMemcpy(host.data(), o.p, o.bytes, hipMemcpyDeviceToHost), "hipMemcpy");
  std::ofstream f(dir + "/out/" + cur_case + "." + which + "." + name + ".bin", std::ios::binary);
  f.write(host.data(), o.bytes);
  if (!f) bad_case(std::string("cannot write the output ") + name);
}

// num[i] <- num[i] / den[i], zero where den[i] is zero: the words zkfhe_fr_batch_invert_mul stores
__global__ void __launch_bounds__(256) k_test_ratio(const Fr *__restrict__ den, Fr *__restrict__ num, size_t total) {
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x)
    num[g] = den[g].is_zero() ? Fr::zero() : num[g] * zk::fp_inv<zk::FrP>(den[g]);
}
void ratios(const Fr *den, Fr *num, size_t total) {
  if (!total) return;
  k_test_ratio<<<grid_for(total), 256>>>(den, num, total);
  launched("k_test_ratio");
}

struct GpBufs {
  Out bd, num, den, z, totals, closes;
};
GpBufs gp_bufs(size_t n, size_t n_perm, size_t cols) {
  GpBufs b{output(n_perm, 8), output(cols * n, n), output(cols * n, n), output(cols * n, n), output(cols, 8), output(1, 0)};
  const int ones[2] = {1, 1};   // the host sets both flags before the launches
  hip_ok(hipMemcpy(b.closes.p, ones, sizeof(ones), hipMemcpyHostToDevice), "hipMemcpy");
  return b;
}
void gp_dump(const char *which, const GpBufs &b) {
  dump(which, "bd", b.bd), dump(which, "num", b.num), dump(which, "den", b.den), dump(which, "z", b.z), dump(which, "totals", b.totals), dump(which, "closes", b.closes);
}

void run_gp(Args &a) {
  const size_t n = a.num();
  const unsigned u = a.num(), n_advice = a.num(), chunk = a.num(), nl = a.num();
  if (n < 2 || n > 65536 || u + 1 >= n || chunk < 1 || n_advice < 1 || n_advice > 4094 || nl > 64) bad_case("2 <= n <= 65536, u + 1 < n, chunk >= 1, 1 <= n_advice <= 4094, n_lookup <= 64");
  const unsigned n_perm = n_advice + 2, nch = (n_perm + chunk - 1) / chunk;
  const Fr beta = a.scalar(), gamma = a.scalar(), delta = a.scalar();
  zkp::RngRows blind;
  blind.on = 1;
  for (int i = 0; i < 4; ++i) blind.seed.w[i] = a.num();
  const unsigned long long ctr_pz = a.num(), nb_z = n - u - 1;
  blind.ctr_col_stride = nb_z;
  a.done();
  zkp::PermArgs pa;
  pa.adv = input<Fr>("adv", (size_t)n_advice * n * 32), pa.constcol = input<Fr>("const", n * 32), pa.inst = input<Fr>("inst", n * 32);
  pa.sigma = input<Fr>("sigma", (size_t)n_perm * n * 32), pa.wpow = input<Fr>("wpow", n * 32);
  pa.beta = beta, pa.gamma = gamma, pa.n_advice = n_advice, pa.n_perm = n_perm, pa.chunk = chunk, pa.n_chunks = nch, pa.n = n;
  const Fr *ac = input<Fr>("a", (size_t)nl * n * 32), *table = input<Fr>("table", n * 32), *la = input<Fr>("la", (size_t)nl * n * 32), *ls = input<Fr>("ls", (size_t)nl * n * 32);
  const size_t cols = nch + nl;
  {   // ---- the sequence of ten launches
    GpBufs b = gp_bufs(n, n_perm, cols);
    int *closes = (int *)b.closes.p;
    zkp::k_powers<<<1, 256>>>(beta, delta, b.bd.p, n_perm);
    launched("k_powers");
    pa.beta_delta = b.bd.p;
    zkp::k_perm_num_den<<<grid_for((size_t)nch * n), 256>>>(pa, b.num.p, b.den.p);
    launched("k_perm_num_den");
    ratios(b.den.p, b.num.p, (size_t)nch * n);
    blind.ctr0 = ctr_pz;
    zkp::k_prefix_product<<<nch + zkp::rng_tail_grid(blind, (size_t)nch * nb_z, 1024), 1024>>>(b.num.p, b.z.p, b.totals.p, n, u, nch, blind);
    launched("k_prefix_product");
    zkp::k_chunk_carry<<<1, 1024>>>(b.totals.p, nch, 0, closes);
    launched("k_chunk_carry");
    zkp::k_scale_rows<<<grid_for((size_t)nch * (u + 1)), 256>>>(b.z.p, b.totals.p, n, u + 1, nch);
    launched("k_scale_rows");
    if (nl) {
      Fr *num = b.num.p + (size_t)nch * n, *den = b.den.p + (size_t)nch * n;
      zkp::k_lookup_num_den<<<grid_for((size_t)nl * n), 256>>>(ac, table, la, ls, beta, gamma, nl, n, num, den);
      launched("k_lookup_num_den");
      ratios(den, num, (size_t)nl * n);
      blind.ctr0 = ctr_pz + (unsigned long long)nch * nb_z;   // ctr_lz
      zkp::k_prefix_product<<<nl + zkp::rng_tail_grid(blind, (size_t)nl * nb_z, 1024), 1024>>>(num, b.z.p + (size_t)nch * n, b.totals.p + nch, n, u, nl, blind);
      launched("k_prefix_product");
      zkp::k_chunk_carry<<<1, 1024>>>(b.totals.p + nch, nl, 1, closes + 1);
      launched("k_chunk_carry");
    }
    gp_dump("old", b);
  }
  {   // ---- side by side: six launches
    GpBufs b = gp_bufs(n, n_perm, cols);
    zkp::k_lookup_num_den_powers<<<(nl ? grid_for((size_t)nl * n) : 0u) + 1u, 256>>>(ac, table, la, ls, beta, gamma, nl, n, b.num.p + (size_t)nch * n, b.den.p + (size_t)nch * n, beta,
                                                                                      delta, b.bd.p, n_perm);
    launched("k_lookup_num_den_powers");
    pa.beta_delta = b.bd.p;
    zkp::k_perm_num_den<<<grid_for((size_t)nch * n), 256>>>(pa, b.num.p, b.den.p);
    launched("k_perm_num_den");
    ratios(b.den.p, b.num.p, cols * n);
    blind.ctr0 = ctr_pz;
    zkp::k_prefix_product<<<(unsigned)cols + zkp::rng_tail_grid(blind, cols * nb_z, 1024), 1024>>>(b.num.p, b.z.p, b.totals.p, n, u, (unsigned)cols, blind);
    launched("k_prefix_product");
    zkp::k_chunk_carry_both<<<nl ? 2 : 1, 1024>>>(b.totals.p, nch, nl, (int *)b.closes.p);
    launched("k_chunk_carry_both");
    zkp::k_scale_rows<<<grid_for((size_t)nch * (u + 1)), 256>>>(b.z.p, b.totals.p, n, u + 1, nch);
    launched("k_scale_rows");
    gp_dump("new", b);
  }
}

void run_sh(Args &a) {
  const size_t n = a.num();
  const unsigned n_cols = a.num(), ns = a.num();
  if (n < 1 || n > 65536 || n_cols < 1 || ns < 1 || ns > 8) bad_case("1 <= n <= 65536, n_cols >= 1, 1 <= n_sets <= 8");
  std::vector<size_t> sizes(ns);
  for (auto &m : sizes) {
    m = a.num();
    if (m < 1 || m > 4096) bad_case("1 <= members <= 4096");
  }
  a.done();
  const chain::Plan plan = chain::plan(sizes);
  const size_t slots = 16;   // of the partial-sum buffer
  unsigned max_chunks = 1;
  for (const auto &s : plan.sums) max_chunks = s.chunks > max_chunks ? s.chunks : max_chunks;
  if (plan.slots > slots || max_chunks > slots) bad_case("more partial sums than the buffer of 16 slots holds");
  const Fr *cols = input<Fr>("cols", (size_t)n_cols * n * 32), *s29 = input<Fr>("s29", (size_t)plan.members * 32), *wpow = input<Fr>("wpow", n * 32);
  const zkp::ShSet *sets = input<zkp::ShSet>("sets", ns * sizeof(zkp::ShSet));
  std::vector<const Fr *> ptrs(plan.members);
  for (size_t k = 0; k < ptrs.size(); ++k) ptrs[k] = cols + ((7 * k + 3) % n_cols) * n;
  const Fr *const *pd = upload(ptrs);
  const unsigned gx = grid_for(n);
  {   // ---- one set after the other (Proof::lincomb), then k_sh_zs
    Out F = output(ns * n, n), zs = output(ns * n, n), partial = output(slots * n, n);
    for (unsigned j = 0; j < ns; ++j) {
      const unsigned m = (unsigned)sizes[j], chunks = (m + chain::PER - 1) / chain::PER;
      const Fr *const *pp = pd + plan.first[j];
      const Fr *pw = s29 + plan.first[j];
      if (chunks > 1) {
        zkp::k_lincomb_ptrs_chunked<<<dim3(gx, chunks), 256>>>(pp, pw, m, chain::PER, n, partial.p);
        launched("k_lincomb_ptrs_chunked");
        zkp::k_sum_rows<<<gx, 256>>>(partial.p, chunks, n, F.p + (size_t)j * n);
        launched("k_sum_rows");
      } else {
        zkp::k_lincomb_ptrs<<<gx, 256>>>(pp, pw, m, n, F.p + (size_t)j * n);
        launched("k_lincomb_ptrs");
      }
    }
    zkp::k_sh_zs<<<grid_for(ns * n), 256>>>(sets, ns, wpow, n, zs.p);
    launched("k_sh_zs");
    dump("old", "F", F), dump("old", "zs", zs);
  }
  {   // ---- side by side: two launches
    Out F = output(ns * n, n), zs = output(ns * n, n), partial = output(slots * n, n);
    const chain::Job *jobs = upload(plan.jobs);
    const chain::Sum *sums = upload(plan.sums);
    const unsigned nj = (unsigned)plan.jobs.size(), tail_rows = (grid_for(ns * n) + gx - 1) / gx;
    zkp::k_chain_jobs<zkp::TAIL_ZS><<<dim3(gx, nj + tail_rows), 256>>>(jobs, nj, pd, s29, n, F.p, partial.p, sets, ns, wpow, zs.p);
    launched("k_chain_jobs<TAIL_ZS>");
    if (!plan.sums.empty()) {
      zkp::k_chain_sums<<<dim3(gx, (unsigned)plan.sums.size()), 256>>>(sums, partial.p, n, F.p);
      launched("k_chain_sums");
    }
    dump("new", "F", F), dump("new", "zs", zs), dump("new", "partial", partial);
  }
  {   // ---- the jobs alone and k_sh_zs behind them: what the prover launches when the merged launch would fill the chip
    Out F = output(ns * n, n), zs = output(ns * n, n), partial = output(slots * n, n);
    const chain::Job *jobs = upload(plan.jobs);
    const chain::Sum *sums = upload(plan.sums);
    const unsigned nj = (unsigned)plan.jobs.size();
    zkp::k_chain_jobs<zkp::TAIL_NONE><<<dim3(gx, nj), 256>>>(jobs, nj, pd, s29, n, F.p, partial.p, nullptr, 0, nullptr, nullptr);
    launched("k_chain_jobs<TAIL_NONE>");
    zkp::k_sh_zs<<<grid_for(ns * n), 256>>>(sets, ns, wpow, n, zs.p);
    launched("k_sh_zs");
    if (!plan.sums.empty()) {
      zkp::k_chain_sums<<<dim3(gx, (unsigned)plan.sums.size()), 256>>>(sums, partial.p, n, F.p);
      launched("k_chain_sums");
    }
    dump("split", "F", F), dump("split", "zs", zs);
  }
}

void run_ev(Args &a) {
  const size_t n = a.num();
  a.done();
  if (n < 1 || n > 65536) bad_case("1 <= n <= 65536");
  const Fr *h = input<Fr>("h", 3 * n * 32), *s29 = input<Fr>("s29", 3 * 32), *pts = input<Fr>("pts", 6 * 32), *wpow = input<Fr>("wpow", n * 32);
  const Fr *const *pd = upload(std::vector<const Fr *>{h, h + n, h + 2 * n});
  const unsigned gx = grid_for(n);
  {
    Out H = output(n, n), bw = output(6 * n, n);
    zkp::k_lincomb_ptrs<<<gx, 256>>>(pd, s29, 3, n, H.p);
    launched("k_lincomb_ptrs");
    zkp::k_bary_den<<<grid_for(6 * n), 256>>>(wpow, pts, 6, n, bw.p);
    launched("k_bary_den");
    dump("old", "H", H), dump("old", "bw", bw);
  }
  {
    Out H = output(n, n), bw = output(6 * n, n);
    const chain::Job *job = upload(std::vector<chain::Job>{chain::Job{0, 3, 0, -1}});
    const unsigned tail_rows = (grid_for(6 * n) + gx - 1) / gx;
    zkp::k_chain_jobs<zkp::TAIL_BARY><<<dim3(gx, 1 + tail_rows), 256>>>(job, 1, pd, s29, n, H.p, nullptr, pts, 6, wpow, bw.p);
    launched("k_chain_jobs<TAIL_BARY>");
    dump("new", "H", H), dump("new", "bw", bw);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <directory>\n", argv[0]);
    return 2;
  }
  static_assert(sizeof(zkp::ShSet) == 11 * 32 + 16, "the test writes ShSet records of 368 bytes");
  static_assert(sizeof(chain::Job) == 16 && sizeof(chain::Sum) == 16, "job records of 16 bytes");
  dir = argv[1];
  std::ifstream list(dir + "/cases.txt");
  if (!list) {
    fprintf(stderr, "no %s/cases.txt\n", dir.c_str());
    return 2;
  }
  hipDeviceProp_t prop;
  hip_ok(hipGetDeviceProperties(&prop, 0), "hipGetDeviceProperties");
  num_cu = (unsigned)prop.multiProcessorCount;
  std::string line;
  unsigned runs = 0;
  while (std::getline(list, line)) {
    Args a;
    std::istringstream ss(line);
    for (std::string tok; ss >> tok;) a.t.push_back(tok);
    if (a.t.empty() || a.t[0][0] == '#') continue;
    const std::string cmd = a.next();
    cur_case = a.next();
    if (cmd == "gp") run_gp(a);
    else if (cmd == "sh") run_sh(a);
    else if (cmd == "ev") run_ev(a);
    else bad_case("unknown command " + cmd);
    ++runs;
  }
  printf("chain side by side: %u cases run\n", runs);
  return 0;
}
