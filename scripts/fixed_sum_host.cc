// Host restatement of the grouped sums' fixed-point format (socceraction_amd/csrc/sa_fixed.h):
// the same header the kernels compile, driven from a file.  Plain C++, no HIP:
//
//     g++ -O1 -std=c++17 scripts/fixed_sum_host.cc -o fixed_sum_host
//     fixed_sum_host IN OUT
//
// IN (little endian):  int32 mode, int32 E, int64 n, int64 n_groups, then
//   mode 0 (sum):      f64 value[n], int32 key[n]
//   mode 1 (finalise): int64 limbs[n][3]
// OUT: mode 0: int64 limbs[n_groups][3], int64 count[n_groups], int64 err, f64 sum[n_groups]
//              (the rules of sa_group_sums: key -1 skips, NaN adds nothing, an error drops the row)
//      mode 1: f64 sum[n]
// tests/test_ratings_host.py compares both with a Python-integer restatement.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../socceraction_amd/csrc/sa_fixed.h"

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T>
static bool write_n(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    perror(argv[1]);
    return 2;
  }
  int32_t head[2];
  int64_t dims[2];
  if (fread(head, sizeof(head), 1, in) != 1 || fread(dims, sizeof(dims), 1, in) != 1) {
    fprintf(stderr, "short header\n");
    return 2;
  }
  const int mode = head[0], E = head[1];
  const int64_t n = dims[0], G = dims[1];
  if (mode < 0 || mode > 1 || E < SA_FX_EXP_MIN || E > SA_FX_EXP_MAX || n < 0 || n >= SA_FX_MAX_ROWS ||
      G < 0 || G >= SA_FX_MAX_ROWS) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<double> out;
  std::vector<int64_t> limbs, count;
  int64_t err = 0;
  if (mode == 0) {
    std::vector<double> val;
    std::vector<int32_t> key;
    if (!read_n(in, val, (size_t)n) || !read_n(in, key, (size_t)n)) {
      fprintf(stderr, "short input\n");
      return 2;
    }
    limbs.assign((size_t)G * 3, 0);
    count.assign((size_t)G, 0);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t k = key[(size_t)i];
      if (k == -1) continue;
      if (k < 0 || k >= G) {
        err |= 1;
        continue;
      }
      uint32_t m[3];
      int neg;
      const int q = sa_fx_quantize(val[(size_t)i], E, m, &neg);
      if (q & (SA_FX_NONFINITE | SA_FX_RANGE)) {
        err |= q;
        continue;
      }
      for (int j = 0; j < 3; ++j) limbs[(size_t)k * 3 + j] += neg ? -(int64_t)m[j] : (int64_t)m[j];
      ++count[(size_t)k];
    }
    out.resize((size_t)G);
    for (int64_t g = 0; g < G; ++g)
      out[(size_t)g] = sa_fx_finalize(limbs[(size_t)g * 3], limbs[(size_t)g * 3 + 1], limbs[(size_t)g * 3 + 2], E);
  } else {
    std::vector<int64_t> l;
    if (!read_n(in, l, (size_t)n * 3)) {
      fprintf(stderr, "short input\n");
      return 2;
    }
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      out[(size_t)i] = sa_fx_finalize(l[(size_t)i * 3], l[(size_t)i * 3 + 1], l[(size_t)i * 3 + 2], E);
  }
  fclose(in);
  FILE* o = fopen(argv[2], "wb");
  if (!o) {
    perror(argv[2]);
    return 2;
  }
  bool ok = true;
  if (mode == 0) ok = write_n(o, limbs) && write_n(o, count) && fwrite(&err, sizeof(err), 1, o) == 1;
  ok = ok && write_n(o, out);
  if (fclose(o) != 0 || !ok) {
    fprintf(stderr, "write failed\n");
    return 2;
  }
  return 0;
}
