// Launches the kernels of zk-fhe_amd/host/prover_kernels.hip.hpp alone, with the prover's block sizes, on arrays read from files.
// It holds no reference and decides nothing: tests/prover_kernel_cases.py writes the inputs and knows the expected outputs,
// tests/test_gpu_prover_kernels.py compares.
//
//   prover_kernels_driver <dir>      reads <dir>/cases.txt and <dir>/in/*.bin, writes <dir>/out/<buffer>.bin
//
// cases.txt, one command per line, tokens separated by blanks:
//   buf NAME BYTES FILE|-     a device buffer: the contents of <dir>/in/FILE (exactly BYTES long), or BYTES sentinel bytes 0xA5
//                             (a 32-byte word of them is no canonical field element, so an untouched row shows)
//   run CASE KERNEL ARGS...   one launch (or the prover's short sequence of launches); the arguments of every KERNEL are listed at
//                             its branch below.  A buffer argument is NAME or NAME+BYTEOFFSET, a field scalar 64 hexadecimal
//                             digits (the 256-bit word, most significant digit first), everything else a decimal number.
//   dump NAME                 the buffer -> <dir>/out/NAME.bin
// Every buffer argument is checked against the extent the kernel reads or writes before the launch (exit status 2: the case list is
// wrong, nothing was launched for that case).  After every launch the status is read and the device synchronised; on the first error
// the case's name is printed and the program ends with status 1 without launching anything more.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "prover_kernels.hip.hpp"

using zk::Fr;

namespace {

struct Buf {
  char *p = nullptr;
  size_t bytes = 0;
};
std::map<std::string, Buf> bufs;
std::string cur_case = "(none)";
std::string dir;

[[noreturn]] void bad_case(const std::string &why) {
  fprintf(stderr, "prover_kernels_driver: case %s: %s\n", cur_case.c_str(), why.c_str());
  exit(2);
}
void hip_ok(hipError_t e, const char *what) {
  if (e == hipSuccess) return;
  printf("prover_kernels_driver: HIP error in case %s (%s): %s\n", cur_case.c_str(), what, hipGetErrorString(e));
  fflush(stdout);
  _exit(1);   // nothing more is launched, freed or copied on a device that reported an error
}
void launched(const char *kernel) {
  hip_ok(hipGetLastError(), kernel);
  hip_ok(hipDeviceSynchronize(), kernel);
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
  unsigned grid() {
    const unsigned long long g = num();
    if (g < 1 || g > 65535) bad_case("a grid has 1 to 65535 workgroups");
    return (unsigned)g;
  }
  // a buffer argument of which the kernel touches `need` bytes
  char *ptr(size_t need) {
    std::string s = next();
    size_t off = 0;
    const size_t plus = s.find('+');
    if (plus != std::string::npos) {
      off = strtoull(s.c_str() + plus + 1, nullptr, 10);
      s = s.substr(0, plus);
    }
    auto it = bufs.find(s);
    if (it == bufs.end()) bad_case("no buffer " + s);
    if (off > it->second.bytes || need > it->second.bytes - off) bad_case("buffer " + s + " is too small for this launch");
    return it->second.p + off;
  }
  Fr *fr(size_t words) { return (Fr *)ptr(words * 32); }
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

// a small table built on the host (jobs, pointers) -> the device; kept until the program ends
template <class T>
T *upload(const std::vector<T> &v) {
  T *d = nullptr;
  hip_ok(hipMalloc(&d, v.size() * sizeof(T) + 1), "hipMalloc");
  hip_ok(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
  return d;
}

void run(Args &a) {
  cur_case = a.next();
  const std::string k = a.next();
  if (k == "powers") {   // GRID n start base out
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const Fr start = a.scalar(), base = a.scalar();
    Fr *out = a.fr(n);
    a.done();
    zkp::k_powers<<<grid, 256>>>(start, base, out, n);
    launched("k_powers");
  } else if (k == "perm") {   // GRID n n_advice n_perm chunk adv const inst sigma wpow beta_delta beta gamma num den
    const unsigned grid = a.grid();
    zkp::PermArgs pa;
    pa.n = a.num();
    pa.n_advice = a.num(), pa.n_perm = a.num(), pa.chunk = a.num();
    if (pa.chunk == 0 || pa.n_perm != pa.n_advice + 2) bad_case("n_perm is n_advice + 2, chunk >= 1");
    pa.n_chunks = (pa.n_perm + pa.chunk - 1) / pa.chunk;
    pa.adv = a.fr(pa.n_advice * pa.n), pa.constcol = a.fr(pa.n), pa.inst = a.fr(pa.n), pa.sigma = a.fr(pa.n_perm * pa.n);
    pa.wpow = a.fr(pa.n), pa.beta_delta = a.fr(pa.n_perm);
    pa.beta = a.scalar(), pa.gamma = a.scalar();
    Fr *num = a.fr(pa.n_chunks * pa.n), *den = a.fr(pa.n_chunks * pa.n);
    a.done();
    zkp::k_perm_num_den<<<grid, 256>>>(pa, num, den);
    launched("k_perm_num_den");
  } else if (k == "lookup") {   // GRID n n_lookup a table la ls beta gamma num den
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned nl = a.num();
    const Fr *ac = a.fr(nl * n), *table = a.fr(n), *la = a.fr(nl * n), *ls = a.fr(nl * n);
    const Fr beta = a.scalar(), gamma = a.scalar();
    Fr *num = a.fr(nl * n), *den = a.fr(nl * n);
    a.done();
    zkp::k_lookup_num_den<<<grid, 256>>>(ac, table, la, ls, beta, gamma, nl, n, num, den);
    launched("k_lookup_num_den");
  } else if (k == "prefix") {   // n u n_cols ratio z total on seed0 seed1 seed2 seed3 ctr0 ctr_col_stride -- the prover's grid
    const size_t n = a.num();
    const unsigned u = a.num(), n_cols = a.num();
    if (u >= n || n > 65536 * 64) bad_case("u < n");
    const Fr *ratio = a.fr(n_cols * n);
    Fr *z = a.fr(n_cols * n), *total = a.fr(n_cols);
    zkp::RngRows blind;
    blind.on = (int)a.num();
    for (int i = 0; i < 4; ++i) blind.seed.w[i] = a.num();
    blind.ctr0 = a.num(), blind.ctr_col_stride = a.num();
    a.done();
    zkp::k_prefix_product<<<n_cols + zkp::rng_tail_grid(blind, (size_t)n_cols * (n - u - 1), 1024), 1024>>>(ratio, z, total, n, u, n_cols, blind);
    launched("k_prefix_product");
  } else if (k == "prefix_seg") {   // n u n_cols seg_len ratio seg z total -- the prover's three launches
    const size_t n = a.num();
    const unsigned u = a.num(), n_cols = a.num(), seg_len = a.num();
    if (u >= n || seg_len == 0 || n % seg_len) bad_case("u < n, seg_len divides n");
    const unsigned segs = (unsigned)(n / seg_len);
    const Fr *ratio = a.fr(n_cols * n);
    Fr *seg = a.fr((size_t)n_cols * segs), *z = a.fr(n_cols * n), *total = a.fr(n_cols);
    a.done();
    zkp::k_prefix_seg_totals<<<dim3(segs, n_cols), 1024>>>(ratio, seg, n, u, seg_len);
    launched("k_prefix_seg_totals");
    zkp::k_prefix_seg_scan<<<(n_cols + 63) / 64, 64>>>(seg, segs, n_cols, total);
    launched("k_prefix_seg_scan");
    zkp::k_prefix_seg_apply<<<dim3(segs, n_cols), 1024>>>(ratio, seg, z, n, u, seg_len);
    launched("k_prefix_seg_apply");
  } else if (k == "carry") {   // count check_ones total closes
    const unsigned count = a.num();
    const int check_ones = (int)a.num();
    if (count < 1 || count > 4096) bad_case("1 <= count <= 4096");
    Fr *total = a.fr(count);
    int *closes = (int *)a.ptr(sizeof(int));
    a.done();
    zkp::k_chunk_carry<<<1, 1024>>>(total, count, check_ones, closes);
    launched("k_chunk_carry");
  } else if (k == "scale") {   // GRID n rows n_cols z carry
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned rows = a.num(), n_cols = a.num();
    if (rows > n) bad_case("rows <= n");
    Fr *z = a.fr(n_cols * n);
    const Fr *carry = a.fr(n_cols);
    a.done();
    zkp::k_scale_rows<<<grid, 256>>>(z, carry, n, rows, n_cols);
    launched("k_scale_rows");
  } else if (k == "qcombine") {   // log_n rows n_groups pt0 pt_count partials ypow zinv h_ext -- the prover's grid
    const unsigned log_n = a.num(), rows = a.num(), n_groups = a.num();
    const size_t pt0 = a.num(), pt_count = a.num(), ne = ((size_t)1 << log_n) * rows;
    if (log_n > 20 || pt_count < 1 || pt0 + pt_count > ne) bad_case("the points lie inside the rows");
    const Fr *partials = a.fr(n_groups * ne), *ypow = a.fr(n_groups), *zinv = a.fr(rows);
    Fr *h_ext = a.fr(ne);
    a.done();
    zkp::k_quotient_combine<<<(unsigned)((pt_count + 255) / 256), 256>>>(partials, ypow, n_groups, zinv, log_n, rows, pt0, pt_count, h_ext);
    launched("k_quotient_combine");
  } else if (k == "ext3") {   // n rows3 pw h_c v0 .. v8 -- the prover's grid
    const size_t n = a.num();
    const Fr *rows3 = a.fr(3 * n), *pw = a.fr(3 * n);
    Fr *h_c = a.fr(4 * n);
    zkp::Mat3 m;
    for (int i = 0; i < 9; ++i) m.v[i] = a.scalar();
    a.done();
    zkp::k_ext3_combine<<<(unsigned)((n + 255) / 256), 256>>>(rows3, pw, m, n, h_c);
    launched("k_ext3_combine");
  } else if (k == "bary_den") {   // GRID n n_pts wpow pts out
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned n_pts = a.num();
    const Fr *wpow = a.fr(n), *pts = a.fr(n_pts);
    Fr *out = a.fr(n_pts * n);
    a.done();
    zkp::k_bary_den<<<grid, 256>>>(wpow, pts, n_pts, n, out);
    launched("k_bary_den");
  } else if (k == "bary_weights") {   // GRID n total wpow c inout
    const unsigned grid = a.grid();
    const size_t n = a.num(), total = a.num();
    const Fr *wpow = a.fr(n);
    const Fr c = a.scalar();
    Fr *inout = a.fr(total);
    a.done();
    zkp::k_bary_weights<<<grid, 256>>>(wpow, c, total, n, inout);
    launched("k_bary_weights");
  } else if (k == "eval") {   // n slices GRID_SUM n_jobs bw partial out {col n_rot rot0 rot1 rot2 rot3}...; 6 weight rows
    const size_t n = a.num();
    const unsigned slices = a.num(), grid_sum = a.grid(), nj = a.num();
    if (nj < 1 || slices < 1 || n / slices == 0) bad_case("at least one job and one row per slice");
    const Fr *bw = a.fr(6 * n);
    Fr *partial = a.fr((size_t)slices * nj * 4), *out = a.fr((size_t)nj * 4);
    std::vector<zkp::EvalJob> jobs(nj);
    for (auto &j : jobs) {
      j.col = a.fr(n);
      j.n_rot = (int)a.num();
      if (j.n_rot < 1 || j.n_rot > 4) bad_case("1 <= n_rot <= 4");
      for (int r = 0; r < 4; ++r) {
        j.rot[r] = (int)a.num();
        if (j.rot[r] < 0 || j.rot[r] >= 6) bad_case("a rotation index is below 6");
      }
    }
    a.done();
    const zkp::EvalJob *jd = upload(jobs);
    if (slices == 1) {
      zkp::k_eval_jobs<<<nj, 256>>>(jd, bw, n, out);
      launched("k_eval_jobs");
    } else {
      zkp::k_eval_jobs<<<dim3(nj, slices), 256>>>(jd, bw, n, partial);
      launched("k_eval_jobs");
      zkp::k_sum_rows<<<grid_sum, 256>>>(partial, slices, (size_t)nj * 4, out);
      launched("k_sum_rows");
    }
  } else if (k == "lincomb") {   // GRID n per m partial out s29 ptr...; per = 0: the plain kernel, else the chunked one and k_sum_rows
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned per = a.num(), m = a.num();
    if (m < 1) bad_case("m >= 1");
    const unsigned chunks = per ? (m + per - 1) / per : 1;
    Fr *partial = a.fr((size_t)chunks * n), *out = a.fr(n);
    const Fr *s29 = a.fr(m);
    std::vector<const Fr *> ptrs(m);
    for (auto &p : ptrs) p = a.fr(n);
    a.done();
    const Fr *const *pd = upload(ptrs);
    if (!per) {
      zkp::k_lincomb_ptrs<<<grid, 256>>>(pd, s29, m, n, out);
      launched("k_lincomb_ptrs");
    } else {
      zkp::k_lincomb_ptrs_chunked<<<dim3(grid, chunks), 256>>>(pd, s29, m, per, n, partial);
      launched("k_lincomb_ptrs_chunked");
      zkp::k_sum_rows<<<grid, 256>>>(partial, chunks, n, out);
      launched("k_sum_rows");
    }
  } else if (k == "sh_zs") {   // GRID n n_sets sets wpow zs
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned ns = a.num();
    const zkp::ShSet *sets = (const zkp::ShSet *)a.ptr(ns * sizeof(zkp::ShSet));
    const Fr *wpow = a.fr(n);
    Fr *zs = a.fr(ns * n);
    a.done();
    zkp::k_sh_zs<<<grid, 256>>>(sets, ns, wpow, n, zs);
    launched("k_sh_zs");
  } else if (k == "sh_h") {   // GRID n n_sets sets F zs_inv wpow hq
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned ns = a.num();
    const zkp::ShSet *sets = (const zkp::ShSet *)a.ptr(ns * sizeof(zkp::ShSet));
    const Fr *F = a.fr(ns * n), *zs_inv = a.fr(ns * n), *wpow = a.fr(n);
    Fr *hq = a.fr(n);
    a.done();
    zkp::k_sh_h<<<grid, 256>>>(sets, ns, F, zs_inv, wpow, n, hq);
    launched("k_sh_h");
  } else if (k == "sh_den") {   // n wpow u out -- the prover's grid
    const size_t n = a.num();
    const Fr *wpow = a.fr(n);
    const Fr u = a.scalar();
    Fr *out = a.fr(n);
    a.done();
    zkp::k_sh_den<<<(unsigned)((n + 255) / 256), 256>>>(wpow, u, n, out);
    launched("k_sh_den");
  } else if (k == "sh_w") {   // GRID n n_sets F hq inv W ztu coef0..7 r_u0..7
    const unsigned grid = a.grid();
    const size_t n = a.num();
    const unsigned ns = a.num();
    if (ns < 1 || ns > 8) bad_case("1 <= n_sets <= 8");
    const Fr *F = a.fr(ns * n), *hq = a.fr(n), *inv = a.fr(n);
    Fr *W = a.fr(n);
    const Fr ztu = a.scalar();
    zkp::ShW w;
    for (int j = 0; j < 8; ++j) w.coef[j] = a.scalar();
    for (int j = 0; j < 8; ++j) w.r_u[j] = a.scalar();
    a.done();
    zkp::k_sh_w<<<grid, 256>>>(w, ns, F, hq, ztu, inv, n, W);
    launched("k_sh_w");
  } else {
    bad_case("no kernel " + k);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <directory>\n", argv[0]);
    return 2;
  }
  static_assert(sizeof(zkp::ShSet) == 11 * 32 + 16, "tests/prover_kernel_cases.py writes ShSet records of 368 bytes");
  dir = argv[1];
  std::ifstream list(dir + "/cases.txt");
  if (!list) {
    fprintf(stderr, "no %s/cases.txt\n", dir.c_str());
    return 2;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::string line;
  unsigned runs = 0;
  std::vector<char> host;
  while (std::getline(list, line)) {
    Args a;
    std::istringstream ss(line);
    for (std::string tok; ss >> tok;) a.t.push_back(tok);
    if (a.t.empty() || a.t[0][0] == '#') continue;
    const std::string cmd = a.next();
    if (cmd == "buf") {
      cur_case = "buf " + a.t[1];
      const std::string name = a.next();
      Buf b;
      b.bytes = a.num();
      const std::string file = a.next();
      a.done();
      if (bufs.count(name) || b.bytes == 0) bad_case("a buffer is declared once and is not empty");
      hip_ok(hipMalloc(&b.p, b.bytes), "hipMalloc");
      if (file == "-") {
        hip_ok(hipMemset(b.p, 0xA5, b.bytes), "hipMemset");
      } else {
        std::ifstream f(dir + "/in/" + file, std::ios::binary);
        host.resize(b.bytes + 1);
        f.read(host.data(), b.bytes + 1);
        if (!f.eof() || (size_t)f.gcount() != b.bytes) bad_case("file " + file + " has not the declared size");
        hip_ok(hipMemcpy(b.p, host.data(), b.bytes, hipMemcpyHostToDevice), "hipMemcpy");
      }
      hip_ok(hipDeviceSynchronize(), "buf");
      bufs[name] = b;
    } else if (cmd == "run") {
      run(a);
      ++runs;
    } else if (cmd == "dump") {
      cur_case = "dump " + a.t[1];
      const std::string name = a.next();
      a.done();
      auto it = bufs.find(name);
      if (it == bufs.end()) bad_case("no buffer " + name);
      host.resize(it->second.bytes);
      hip_ok(hipMemcpy(host.data(), it->second.p, it->second.bytes, hipMemcpyDeviceToHost), "hipMemcpy");
      std::ofstream f(dir + "/out/" + name + ".bin", std::ios::binary);
      f.write(host.data(), it->second.bytes);
      if (!f) bad_case("cannot write the output of " + name);
    } else {
      cur_case = line;
      bad_case("unknown command");
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("prover kernels: %u cases run, %zu buffers, %.0f ms\n", runs, bufs.size(), ms);
  return 0;
}
