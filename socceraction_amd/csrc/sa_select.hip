// Row gather over bitmap-form feature blocks (the shot rows of the expected-goals notebook,
// public-notebooks/EXTRA-build-expected-goals-model.ipynb `Xi[shot_idx]`; any row list: per-type
// models, a compact held-out set, resamples with replacement).
//
// The features of n actions sit in HBM as two tiled numeric blocks [tiles, C, R] and the bool
// features as Arrow bitmaps [n_bool, words] (bit i of word w = row 64w + i).  sa_select_rows
// copies the m listed rows, in list order, into one-tile numeric blocks [1, C, ld] and bitmaps
// [n_bool, ceil(m / 64)]: what every consumer of feature blocks takes, m rows long.
//
// Bitmaps: one wave owns one output word j.  Lane i reads rows[64j + i] once and keeps its source
// (word, bit); per bool column every lane loads that column's source word (ascending rows: the
// lanes of a wave hit the same or neighbouring words), extracts its bit, and one __ballot is the
// output word.  The ballots of 64 columns are collected so that lane c holds column c's word and
// the wave stores them with one 8-byte store per lane.  Lanes at or beyond m vote 0: the tail
// bits of the last word are clear.
// Numeric: lanes run along the output row q of a group of SEL_COLS columns, so the stores of a
// wave are contiguous; a row's tile and offset are computed once per group.  Element bits are
// copied as integers (NaN payloads and -0.0 survive); rows m .. ld - 1 are written as zeros.
// Every output element has one writer: plain stores, no atomics.  A row number outside [0, n) is
// the caller's error (ops.select_rows raises before the launch); the kernels clamp it, so it
// cannot read outside the blocks.
#include <hip/hip_runtime.h>

#include "sa_common.h"
#include "sa_internal.h"

namespace sa {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_COLS = 8;  // numeric columns per thread

__device__ __forceinline__ int64_t select_clamp(int64_t r, int64_t n) {
  SA_DCHECK(r >= 0 && r < n, r);
  return r < 0 ? 0 : (r >= n ? n - 1 : r);
}

__global__ __launch_bounds__(SEL_THREADS) void select_bits_kernel(const uint64_t* __restrict__ src, int64_t words_in,
                                                                  int32_t n_bool, int64_t n,
                                                                  const int64_t* __restrict__ rows, int64_t m,
                                                                  uint64_t* __restrict__ dst, int64_t words_out,
                                                                  int64_t words_used) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (j >= words_used) return;
  const int64_t q = j * 64 + lane;
  const bool live = q < m;
  const int64_t r = live ? select_clamp(rows[q], n) : 0;
  const int64_t word = r >> 6;
  const int bit = (int)(r & 63);
  for (int32_t c0 = 0; c0 < n_bool; c0 += 64) {
    const int cols = n_bool - c0 < 64 ? n_bool - c0 : 64;
    uint64_t mine = 0;
#pragma unroll 8
    for (int k = 0; k < cols; ++k) {
      const uint64_t v = src[(int64_t)(c0 + k) * words_in + word];
      const uint64_t ball = __ballot(live && ((v >> bit) & 1u));
      if (lane == k) mine = ball;
    }
    if (lane < cols) dst[(int64_t)(c0 + lane) * words_out + j] = mine;
  }
}

template <class T>
__global__ __launch_bounds__(SEL_THREADS) void select_num_kernel(const T* __restrict__ src, int32_t C, int64_t R,
                                                                 int64_t n, const int64_t* __restrict__ rows,
                                                                 int64_t m, T* __restrict__ dst, int64_t ld) {
  const int64_t q = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
  if (q >= ld) return;
  const int32_t c0 = (int32_t)blockIdx.y * SEL_COLS;
  const int32_t c1 = c0 + SEL_COLS < C ? c0 + SEL_COLS : C;
  if (q >= m) {  // the padding of the one output tile
    for (int32_t c = c0; c < c1; ++c) dst[(int64_t)c * ld + q] = T(0);
    return;
  }
  const int64_t r = select_clamp(rows[q], n);
  const int64_t tile = r / R, off = r - tile * R;
  const T* p = src + tile * C * R + off;
  if (c1 - c0 == SEL_COLS) {  // (block-uniform) a whole group: its loads in flight together
    T v[SEL_COLS];
#pragma unroll
    for (int k = 0; k < SEL_COLS; ++k) v[k] = p[(int64_t)(c0 + k) * R];
#pragma unroll
    for (int k = 0; k < SEL_COLS; ++k) dst[(int64_t)(c0 + k) * ld + q] = v[k];
    return;
  }
  for (int32_t c = c0; c < c1; ++c) dst[(int64_t)c * ld + q] = p[(int64_t)c * R];
}

template <class T>
static int select_num(const sa_block* blk, int64_t n, const int64_t* rows, int64_t m, void* out, int64_t ld,
                      hipStream_t st, const char* what) {
  if (blk->n_cols == 0) return SA_OK;
  const dim3 grid((unsigned)((ld + SEL_THREADS - 1) / SEL_THREADS), (unsigned)((blk->n_cols + SEL_COLS - 1) / SEL_COLS));
  hipLaunchKernelGGL(select_num_kernel<T>, grid, dim3(SEL_THREADS), 0, st, (const T*)blk->data, blk->n_cols,
                     blk->tile_rows, n, rows, m, (T*)out, ld);
  return check_launch(what);
}

}  // namespace sa

using namespace sa;

extern "C" int sa_select_rows(const sa_block* f_blk, const sa_block* i_blk, int32_t f32, const int64_t* bits,
                              int64_t words_in, int32_t n_bool, int64_t n, const int64_t* rows, int64_t m,
                              void* f_out, void* i_out, int64_t ld_out, int64_t* bits_out, int64_t words_out,
                              void* stream) {
  if (!f_blk || !i_blk) return fail(SA_EINVAL, "bad sa_select_rows arguments: null block descriptor");
  if (n < 0 || m < 0 || n_bool < 0 || f_blk->n_cols < 0 || i_blk->n_cols < 0 || words_in < 0 || words_out < 0 ||
      ld_out < 0)
    return fail(SA_EINVAL, "bad sa_select_rows arguments: negative size");
  if (n_bool > 65535 || f_blk->n_cols > 65535 || i_blk->n_cols > 65535) return fail(SA_EINVAL, "too many columns");
  if (m == 0 || (n_bool == 0 && f_blk->n_cols == 0 && i_blk->n_cols == 0)) return SA_OK;
  if (!rows) return fail(SA_EINVAL, "null row list");
  if (n == 0) return fail(SA_EINVAL, "rows selected from an empty table");
  if (m > ((int64_t)1 << 37)) return fail(SA_EINVAL, "too many rows selected");
  const sa_block* blks[2] = {f_blk, i_blk};
  const void* outs[2] = {f_out, i_out};
  for (int k = 0; k < 2; ++k) {
    if (blks[k]->n_cols == 0) continue;
    if (!blks[k]->data || !outs[k]) return fail(SA_EINVAL, "null numeric block");
    if (blks[k]->tile_rows < 16 || blks[k]->tile_rows % 16)
      return fail(SA_EINVAL, "numeric block tiles must be multiples of 16 rows");
  }
  if ((f_blk->n_cols || i_blk->n_cols) && (ld_out < m || ld_out % 16))
    return fail(SA_EINVAL, "the output tile must hold m rows and be a multiple of 16 rows");
  const int64_t words_used = (m + 63) / 64;
  if (n_bool) {
    if (!bits || !bits_out) return fail(SA_EINVAL, "null bitmap");
    if (words_in < (n + 63) / 64) return fail(SA_EINVAL, "source bitmaps hold fewer than n rows (words_in * 64 < n)");
    if (words_out < words_used) return fail(SA_EINVAL, "output bitmaps hold fewer than m rows");
  }
  const hipStream_t st = (hipStream_t)stream;
  if (n_bool) {
    const unsigned grid = (unsigned)((words_used + SEL_WAVES - 1) / SEL_WAVES);
    hipLaunchKernelGGL(select_bits_kernel, dim3(grid), dim3(SEL_THREADS), 0, st, (const uint64_t*)bits, words_in,
                       n_bool, n, rows, m, (uint64_t*)bits_out, words_out, words_used);
    if (int rc = check_launch("select_bits_kernel")) return rc;
  }
  if (f32) {
    if (int rc = select_num<uint32_t>(f_blk, n, rows, m, f_out, ld_out, st, "select_num_kernel (f32)")) return rc;
    return select_num<uint32_t>(i_blk, n, rows, m, i_out, ld_out, st, "select_num_kernel (i32f)");
  }
  if (int rc = select_num<uint64_t>(f_blk, n, rows, m, f_out, ld_out, st, "select_num_kernel (f64)")) return rc;
  return select_num<uint64_t>(i_blk, n, rows, m, i_out, ld_out, st, "select_num_kernel (i64)");
}
