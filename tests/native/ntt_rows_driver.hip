// Calls the prover's two NTT entry points that the C API does not reach -- zk_coset_ntt_rows (the first `rows` cosets of an
// extension, written densely) and zk_extend_lagrange (Lagrange columns -> coefficients -> coset rows) -- and the plain transforms
// zkfhe_ntt_batch / zkfhe_ntt_batch_to, on columns read from files.  The plain calls are here for the one thing a child process can
// do and the Python binding cannot: run with ZKFHE_NTT_LDS_PASS=0, which the library reads once per process.
// It holds no reference and decides nothing: tests/test_gpu_ntt_rows.py writes the inputs, knows the expected outputs and compares.
//
//   ntt_rows_driver <dir>      reads <dir>/cases.txt, <dir>/g.bin (the coset generator, 32 bytes) and the input files <dir>/in/<IN>
//
// cases.txt, one case per line, of two kinds.  <IN> holds COLS columns of 2^LOG_N words of 32 bytes.
//   rows NAME LOG_N LEF ROWS COLS IN
//     out/NAME.rows.bin   zk_coset_ntt_rows(columns as coefficients): COLS * ROWS * n words, then GUARD bytes that must stay 0xA5
//     out/NAME.ext.bin    zk_extend_lagrange(columns as Lagrange values), out: the same shape and guard
//     out/NAME.tmp.bin    its tmp: COLS * n words and the guard
//     out/NAME.src.bin    the input buffer after both calls (it must come back untouched)
//   plain NAME LOG_N COLS IN CALLS      CALLS: the sum of 1 (forward, out of place), 2 (forward, in place), 4 (inverse, out of place)
//                                       and 8 (inverse, in place)
//     out/NAME.fwd_to.bin, .inv_to.bin   zkfhe_ntt_batch_to into a fresh buffer: COLS * n words and the guard
//     out/NAME.fwd_in.bin, .inv_in.bin   zkfhe_ntt_batch on a copy of the input, and the guard behind it
//     out/NAME.src.bin                   the input buffer after the calls out of place (it must come back untouched)
// The first line of output says whether ZKFHE_NTT_LDS_PASS leaves the LDS passes on ("LDS passes: on" / "off").
// On the first error the case's name and the library's message are printed and the program ends with status 1 without calling
// anything more.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "ntt_plan.hpp"

using zk::Fr;

namespace {

constexpr size_t GUARD = 4096;
zkfhe_ctx *ctx = nullptr;
std::string cur_case = "(none)", dir;

void ok(int rc, const char *what) {
  if (rc == ZKFHE_OK) return;
  printf("ntt_rows_driver: case %s: %s failed (%d): %s\n", cur_case.c_str(), what, rc, zkfhe_last_error(ctx));
  fflush(stdout);
  _exit(1);   // nothing more is launched, freed or copied on a device that reported an error
}

std::vector<char> read_file(const std::string &path, size_t bytes) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> v(bytes);
  if (!f || !f.read(v.data(), (std::streamsize)bytes) || f.peek() != EOF) {
    fprintf(stderr, "ntt_rows_driver: %s is not %zu bytes long\n", path.c_str(), bytes);
    exit(2);
  }
  return v;
}

// a device buffer of `bytes` and the guard behind it, all 0xA5 (a 32-byte word of them is no canonical field element)
char *fresh(size_t bytes) {
  void *p = nullptr;
  ok(zkfhe_dev_alloc(ctx, bytes + GUARD, &p), "zkfhe_dev_alloc");
  ok(zkfhe_memset_dev(ctx, p, 0xA5, bytes + GUARD), "zkfhe_memset_dev");
  return (char *)p;
}

void dump(const std::string &name, const char *dev, size_t bytes) {
  std::vector<char> h(bytes);
  ok(zkfhe_download(ctx, h.data(), dev, bytes), "zkfhe_download");
  std::ofstream f(dir + "/out/" + name, std::ios::binary);
  if (!f.write(h.data(), (std::streamsize)bytes)) {
    fprintf(stderr, "ntt_rows_driver: cannot write %s\n", name.c_str());
    exit(2);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ntt_rows_driver <dir>\n");
    return 2;
  }
  dir = argv[1];
  if (zkfhe_ctx_create(0, nullptr, &ctx) != ZKFHE_OK) {
    printf("ntt_rows_driver: no context: %s\n", zkfhe_last_error(nullptr));
    return 1;
  }
  // what the library will read when it plans its first long row, by the function it reads it with
  printf("LDS passes: %s\n", zk::ntt_lds_pass_enabled(getenv("ZKFHE_NTT_LDS_PASS")) ? "on" : "off");
  Fr g;
  {
    const std::vector<char> gb = read_file(dir + "/g.bin", 32);
    memcpy(&g, gb.data(), 32);
  }
  std::ifstream cases(dir + "/cases.txt");
  std::string line;
  int n_cases = 0;
  while (std::getline(cases, line)) {
    std::istringstream ss(line);
    std::string kind, in_name;
    int log_n = 0, lef = 1, rows = 1, calls = 0;
    size_t cols = 0;
    if (!(ss >> kind >> cur_case >> log_n)) continue;
    const bool plain = kind == "plain";
    if (plain ? !(ss >> cols >> in_name >> calls) : !(kind == "rows" && (ss >> lef >> rows >> cols >> in_name))) {
      fprintf(stderr, "ntt_rows_driver: cannot read the line of case %s\n", cur_case.c_str());
      return 2;
    }
    // at most 2^25 words (1 GiB) per buffer
    if (log_n < 3 || log_n > 20 || lef < 1 || lef > 3 || rows < 1 || rows > (1 << lef) || cols < 1 || cols > 1024 || calls < 0 || calls > 15 ||
        (cols << log_n) * (size_t)rows > ((size_t)1 << 25) || in_name.find('/') != std::string::npos) {
      fprintf(stderr, "ntt_rows_driver: case %s is outside what this driver sizes its buffers for\n", cur_case.c_str());
      return 2;
    }
    const size_t n = (size_t)1 << log_n, in_bytes = cols * n * sizeof(Fr), out_bytes = in_bytes * (size_t)rows;
    const std::vector<char> host = read_file(dir + "/in/" + in_name, in_bytes);
    char *src = fresh(in_bytes);
    ok(zkfhe_upload(ctx, src, host.data(), in_bytes), "zkfhe_upload");

    if (plain) {
      char *out = fresh(in_bytes);
      for (int inverse = 0; inverse < 2; ++inverse) {
        const std::string dirn = inverse ? ".inv" : ".fwd";
        if (calls & (inverse ? 4 : 1)) {
          ok(zkfhe_memset_dev(ctx, out, 0xA5, in_bytes + GUARD), "zkfhe_memset_dev");
          ok(zkfhe_ntt_batch_to(ctx, (const zkfhe_fr *)src, (zkfhe_fr *)out, cols, log_n, inverse), "zkfhe_ntt_batch_to");
          ok(zkfhe_sync(ctx), "zkfhe_sync");
          dump(cur_case + dirn + "_to.bin", out, in_bytes + GUARD);
        }
        if (calls & (inverse ? 8 : 2)) {
          ok(zkfhe_memset_dev(ctx, out, 0xA5, in_bytes + GUARD), "zkfhe_memset_dev");
          ok(zkfhe_upload(ctx, out, host.data(), in_bytes), "zkfhe_upload");
          ok(zkfhe_ntt_batch(ctx, (zkfhe_fr *)out, cols, log_n, inverse), "zkfhe_ntt_batch");
          ok(zkfhe_sync(ctx), "zkfhe_sync");
          dump(cur_case + dirn + "_in.bin", out, in_bytes + GUARD);
        }
      }
      dump(cur_case + ".src.bin", src, in_bytes + GUARD);
      ok(zkfhe_dev_free(ctx, src), "zkfhe_dev_free");
      ok(zkfhe_dev_free(ctx, out), "zkfhe_dev_free");
      ++n_cases;
      continue;
    }

    char *out = fresh(out_bytes), *tmp = fresh(in_bytes);
    ok(zk_coset_ntt_rows(ctx, (const Fr *)src, (Fr *)out, cols, log_n, lef, g, rows), "zk_coset_ntt_rows");
    ok(zkfhe_sync(ctx), "zkfhe_sync");
    dump(cur_case + ".rows.bin", out, out_bytes + GUARD);

    ok(zkfhe_memset_dev(ctx, out, 0xA5, out_bytes + GUARD), "zkfhe_memset_dev");
    ok(zk_extend_lagrange(ctx, (const Fr *)src, (Fr *)tmp, (Fr *)out, cols, log_n, lef, g, rows), "zk_extend_lagrange");
    ok(zkfhe_sync(ctx), "zkfhe_sync");
    dump(cur_case + ".ext.bin", out, out_bytes + GUARD);
    dump(cur_case + ".tmp.bin", tmp, in_bytes + GUARD);
    dump(cur_case + ".src.bin", src, in_bytes + GUARD);

    ok(zkfhe_dev_free(ctx, src), "zkfhe_dev_free");
    ok(zkfhe_dev_free(ctx, out), "zkfhe_dev_free");
    ok(zkfhe_dev_free(ctx, tmp), "zkfhe_dev_free");
    ++n_cases;
  }
  ok(zkfhe_ctx_destroy(ctx), "zkfhe_ctx_destroy");
  printf("%d cases run\n", n_cases);
  return 0;
}
