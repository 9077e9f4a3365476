// Stand-alone host check of sa_select_rows' argument validation, for a sanitizer build on a
// machine without a GPU: every call below returns before any HIP call.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer scripts/select_args_main.cc \
//       socceraction_amd/csrc/sa_select.hip socceraction_amd/csrc/sa_api.hip -o select_args_main
//   ./select_args_main
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/socceraction_amd.h"

static int failures = 0;

static void expect(int rc, int want, const char* word, const char* what) {
  const char* msg = sa_last_error();
  const bool ok = rc == want && (!word || (msg && strstr(msg, word)));
  if (!ok) {
    ++failures;
    printf("FAIL %s: rc %d (want %d), message '%s' (want '%s')\n", what, rc, want, msg ? msg : "", word ? word : "");
  }
}

int main() {
  void* const fake = (void*)256;  // never dereferenced on the host
  sa_block f = {fake, 3, 0, 128}, i = {fake, 2, 0, 128};
  int64_t* const rows = (int64_t*)fake;
  int64_t* const bits = (int64_t*)fake;
  auto call = [&](const sa_block* fb, const sa_block* ib, const int64_t* b, int64_t words_in, int32_t n_bool,
                  int64_t n, const int64_t* r, int64_t m, void* fo, void* io, int64_t ld, int64_t* bo,
                  int64_t words_out) {
    return sa_select_rows(fb, ib, 0, b, words_in, n_bool, n, r, m, fo, io, ld, bo, words_out, nullptr);
  };
  expect(call(nullptr, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "descriptor", "null f");
  expect(call(&f, nullptr, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "descriptor", "null i");
  expect(call(&f, &i, bits, 16, 5, -1, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "negative", "n < 0");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, -1, fake, fake, 112, bits, 2), SA_EINVAL, "negative", "m < 0");
  expect(call(&f, &i, bits, 16, -1, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "negative", "n_bool < 0");
  expect(call(&f, &i, bits, -1, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "negative", "words_in < 0");
  sa_block neg = {fake, -1, 0, 128};
  expect(call(&neg, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "negative", "n_cols < 0");
  expect(call(&f, &i, bits, 16, 5, 1000, nullptr, 100, fake, fake, 112, bits, 2), SA_EINVAL, "null row list", "rows");
  sa_block nodata = {nullptr, 3, 0, 128};
  expect(call(&nodata, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "null numeric", "data");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, 100, nullptr, fake, 112, bits, 2), SA_EINVAL, "null numeric", "f_out");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, 100, fake, nullptr, 112, bits, 2), SA_EINVAL, "null numeric", "i_out");
  expect(call(&f, &i, nullptr, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "null bitmap", "bits");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 112, nullptr, 2), SA_EINVAL, "null bitmap", "bits_out");
  for (int64_t tile : {0, 8, 24, 130}) {
    sa_block odd = {fake, 3, 0, tile};
    expect(call(&odd, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "multiples of 16", "tile");
    expect(call(&f, &odd, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "multiples of 16", "tile");
  }
  expect(call(&f, &i, bits, 15, 5, 1000, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "words_in * 64 < n", "words_in");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 112, bits, 1), SA_EINVAL, "fewer than m", "words_out");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 96, bits, 2), SA_EINVAL, "output tile", "ld < m");
  expect(call(&f, &i, bits, 16, 5, 1000, rows, 100, fake, fake, 104, bits, 2), SA_EINVAL, "output tile", "ld % 16");
  expect(call(&f, &i, bits, 0, 5, 0, rows, 100, fake, fake, 112, bits, 2), SA_EINVAL, "empty table", "n == 0");
  expect(call(&f, &i, bits, INT64_MAX, 5, INT64_MAX, rows, INT64_MAX, fake, fake, 112, bits, 2), SA_EINVAL,
         "too many rows", "m = 2^63 - 1");
  // nothing to do: SA_OK, no launch
  expect(call(&f, &i, nullptr, 16, 5, 1000, nullptr, 0, nullptr, nullptr, 16, nullptr, 1), SA_OK, nullptr, "m == 0");
  sa_block none = {nullptr, 0, 0, 128};
  expect(call(&none, &none, nullptr, 16, 0, 1000, nullptr, 100, nullptr, nullptr, 112, nullptr, 2), SA_OK, nullptr,
         "no columns");
  if (failures) {
    printf("%d argument checks FAILED\n", failures);
    return 1;
  }
  printf("sa_select_rows argument checks ok\n");
  return 0;
}
