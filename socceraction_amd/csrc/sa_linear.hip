// Logistic regression on the feature blocks (the first model of the expected-goals notebook,
// public-notebooks/EXTRA-build-expected-goals-model.ipynb `LogisticRegression().fit(X, y)`): the
// gradient, Hessian and loss of a coefficient vector, and the predictor.
//
// A model reads d columns of bitmap-form feature blocks (bool features as Arrow bitmaps, numeric
// blocks tiled [tiles, C, R] as f64 + i64 or both as f32) in model order; its design matrix has
// D = d + 1 columns, the last one the constant 1 of the intercept.  Per row
//     z = b + sum_j beta_j x_j   (float64, column order, every product and add rounded),
//     p = 1 / (1 + exp(-z)),  r = p - y,  w = p (1 - p),  loss = max(z, 0) + log1p(exp(-|z|)) - y z
// and sa_logit_moments sums T = D (D + 1) / 2 + D + 1 items over the rows:
//     the upper triangle of (w x_j) x_k, row-major (item j D - j (j - 1) / 2 + k - j, j <= k),
//     then the D gradient terms r x_k, then the loss.
// Every term is quantised to the fixed-point limbs of sa_fixed.h (scale exponents: E_j + E_k - 2
// for the triangle, as w <= 1/4; E_k for the gradient; loss_exp for the loss) and the limbs are
// added as integers: no floating-point sum crosses rows, lanes or workgroups, so the 3 T limb
// sums are the same for any row order, row mask padding and grid.
//
// Two kernels.  logit_rows_kernel, one thread per row: z over the model's columns (coalesced
// column reads), then w, r, the loss and a "takes part" flag into a row buffer [4][n].  A row
// outside the mask, or one with a NaN or infinite feature (which also sets the error word), has
// flag 0 and adds nothing.
// logit_pairs_kernel: the items are the cells of a (D + 2) x D table -- row j < D: (w x_j) x_k for
// k >= j; row D: r x_k; row D + 1: the loss, in the constant column -- cut into blocks of
// SA_LOGIT_BLOCK_J x SA_LOGIT_BLOCK_K cells, one block per blockIdx.y (a block without an item
// leaves at once).  A workgroup of 256 threads takes tiles of SA_LOGIT_TILE_ROWS rows
// (grid-stride over blockIdx.x); per tile it stages in LDS only its block's columns: the 16
// left factors A_j = w x_j (or r, or the loss) and the 64 x_k values, row-major (a wave reads one
// row's 64 neighbouring x_k: no bank conflicts; A_j is a broadcast).  So the LDS a workgroup
// needs does not grow with the model's width.  Lane l of wave v owns column k0 + l and the four
// rows j0 + 4 v .. + 3: per staged row it reads x_k once, skips the row when it is zero (one-hot
// columns), and otherwise quantises each non-zero product and adds its limbs to int64 registers.
// A workgroup ends with one 64-bit integer global atomic per non-zero limb sum: 3 per item and
// workgroup, none per row.
//
// A term at or beyond its scale exponent sets SA_LOGIT_ERR_RANGE and adds nothing.
#include "sa_fixed.h"
#include "sa_internal.h"

using namespace sa;

namespace {
constexpr int LG_THREADS = 256;
constexpr int LG_TILE = SA_LOGIT_TILE_ROWS;
constexpr int LG_JB = SA_LOGIT_BLOCK_J;
constexpr int LG_KB = SA_LOGIT_BLOCK_K;
constexpr int LG_WAVES = LG_THREADS / 64;
constexpr int LG_IPT = LG_JB / LG_WAVES;  // items per thread: rows of the block
constexpr int LG_XS = LG_KB + 1;          // row stride of the staged x_k values
static_assert(LG_TILE == 64 && LG_KB == 64 && LG_JB % LG_WAVES == 0, "lanes run along a tile's rows and a block's k");
static_assert(SA_LOGIT_ERR_NAN == SA_FX_NAN && SA_LOGIT_ERR_NONFINITE == SA_FX_NONFINITE &&
                  SA_LOGIT_ERR_RANGE == SA_FX_RANGE,
              "error bits");
typedef unsigned long long u64;

struct LogitIn {
  const void* f;         // f64 (f32) block
  const void* ib;        // i64 (f32) block
  const uint64_t* bits;  // [n_bool][words]
  int64_t Rf, Ri, words;
  int32_t Cf, Ci, n_bool;
};

// by value in the kernel arguments: 2.5 KiB at the widest model
struct LogitCols {
  uint16_t slot[SA_LOGIT_MAX_COLS];  // kind << 14 | column (kind 0: bitmap row, 1: f block, 2: i block)
  int16_t E[SA_LOGIT_MAX_COLS + 1];  // scale exponents of the D design columns
};

// x of (slot, row) as a double.  The caller guarantees row < n.
template <bool F32>
__device__ __forceinline__ double logit_x(const LogitIn& in, uint32_t slot, int64_t row) {
  const int kind = (int)(slot >> 14), col = (int)(slot & 0x3FFF);
  if (kind == 0) {
    SA_DGUARD(col < in.n_bool && (row >> 6) < in.words, col, return 0.0);
    return (double)((in.bits[(int64_t)col * in.words + (row >> 6)] >> (row & 63)) & 1u);
  }
  const int64_t R = kind == 1 ? in.Rf : in.Ri;
  const int32_t C = kind == 1 ? in.Cf : in.Ci;
  SA_DGUARD(col < C, col, return 0.0);
  const int64_t tile = row / R, off = row - tile * R;
  const int64_t at = (tile * C + col) * R + off;
  if (F32) return (double)static_cast<const float*>(kind == 1 ? in.f : in.ib)[at];
  if (kind == 1) return static_cast<const double*>(in.f)[at];
  return (double)static_cast<const int64_t*>(in.ib)[at];
}

// rowbuf [4][n]: w, r, loss, takes part (1.0 / 0.0)
template <bool F32>
__global__ __launch_bounds__(LG_THREADS) void logit_rows_kernel(LogitIn in, LogitCols C, int d,
                                                                const double* __restrict__ beta,
                                                                const uint8_t* __restrict__ y,
                                                                const uint8_t* __restrict__ mask, int64_t n,
                                                                double* __restrict__ rowbuf,
                                                                uint32_t* __restrict__ gerr) {
  const int64_t row = (int64_t)blockIdx.x * LG_THREADS + threadIdx.x;
  if (row >= n) return;
  double w = 0.0, r = 0.0, loss = 0.0, live = 0.0;
  if (!mask || mask[row]) {
    double z = beta[d];
    int bad = 0;
    for (int c = 0; c < d; ++c) {
      const double x = logit_x<F32>(in, C.slot[c], row);
      bad |= sa_fx_classify(x, SA_FX_EXP_MAX) & (SA_FX_NAN | SA_FX_NONFINITE);
      const double t = beta[c] * x;
      z = z + t;
    }
    if (bad) {
      atomicOr(gerr, (uint32_t)bad);  // the row adds nothing
    } else {
      const double yy = y[row] ? 1.0 : 0.0;
      const double p = 1.0 / (1.0 + exp(-z));
      r = p - yy;
      w = p * (1.0 - p);
      loss = (z > 0.0 ? z : 0.0) + log1p(exp(-fabs(z))) - yy * z;
      live = 1.0;
    }
  }
  rowbuf[row] = w;
  rowbuf[n + row] = r;
  rowbuf[2 * n + row] = loss;
  rowbuf[3 * n + row] = live;
}

template <bool F32>
__global__ __launch_bounds__(LG_THREADS) void logit_pairs_kernel(LogitIn in, LogitCols C, int d, int loss_exp,
                                                                 const double* __restrict__ rowbuf, int64_t n,
                                                                 int64_t n_tiles, int n_kb,
                                                                 int64_t* __restrict__ limbs,
                                                                 uint32_t* __restrict__ gerr) {
  __shared__ double A[LG_TILE * LG_JB];   // [row][j - j0]: w x_j, r or the loss
  __shared__ double XK[LG_TILE * LG_XS];  // [row][k - k0]
  const int D = d + 1;
  const int j0 = ((int)blockIdx.y / n_kb) * LG_JB, k0 = ((int)blockIdx.y % n_kb) * LG_KB;
  const int k_last = k0 + LG_KB - 1 < D - 1 ? k0 + LG_KB - 1 : D - 1;
  // (block-uniform) rows j < D hold items at k >= j; rows D and D + 1 in every block of columns
  if (!((j0 < D && k_last >= j0) || (j0 + LG_JB - 1 >= D && j0 < D + 2))) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int k = k0 + lane;
  const int PH = D * (D + 1) / 2;
  [[maybe_unused]] const int T = PH + D + 1;

  int item[LG_IPT], iE[LG_IPT];
  int64_t acc[LG_IPT][3];
  bool any = false;
#pragma unroll
  for (int i = 0; i < LG_IPT; ++i) {
    const int j = j0 + wv * LG_IPT + i;
    acc[i][0] = acc[i][1] = acc[i][2] = 0;
    item[i] = -1;
    iE[i] = 0;
    if (k < D) {
      if (j < D && k >= j) {
        item[i] = j * D - j * (j - 1) / 2 + (k - j);
        iE[i] = (int)C.E[j] + (int)C.E[k] - 2;
      } else if (j == D) {
        item[i] = PH + k;
        iE[i] = C.E[k];
      } else if (j == D + 1 && k == D - 1) {
        item[i] = PH + D;
        iE[i] = loss_exp;
      }
    }
    any = any || item[i] >= 0;
  }

  uint32_t err = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    {  // stage: lanes along the rows (coalesced loads), waves over the block's columns
      const int64_t row = tile * LG_TILE + lane;
      const bool live = row < n && rowbuf[3 * n + row] != 0.0;
      for (int c = wv; c < LG_KB; c += LG_WAVES) {
        const int kk = k0 + c;
        double x = 0.0;
        if (live && kk < D) x = kk == d ? 1.0 : logit_x<F32>(in, C.slot[kk], row);
        XK[lane * LG_XS + c] = x;
      }
      const double w = live ? rowbuf[row] : 0.0;
      for (int c = wv; c < LG_JB; c += LG_WAVES) {
        const int j = j0 + c;
        double a = 0.0;
        if (live) {
          if (j < d) a = w * logit_x<F32>(in, C.slot[j], row);
          else if (j == d) a = w * 1.0;
          else if (j == D) a = rowbuf[n + row];
          else if (j == D + 1) a = rowbuf[2 * n + row];
        }
        A[lane * LG_JB + c] = a;
      }
    }
    __syncthreads();
    if (any) {
      for (int r = 0; r < LG_TILE; ++r) {
        const double xk = XK[r * LG_XS + lane];
        if (xk == 0.0) continue;  // a zero adds nothing
#pragma unroll
        for (int i = 0; i < LG_IPT; ++i) {
          if (item[i] < 0) continue;
          const double t = A[r * LG_JB + wv * LG_IPT + i] * xk;
          if (t == 0.0) continue;
          uint32_t m[3];
          int neg;
          const int rc = sa_fx_quantize(t, iE[i], m, &neg);
          if (rc != SA_FX_OK) {
            err |= (uint32_t)rc;
            continue;
          }
          if (neg) {
            acc[i][0] -= (int64_t)m[0], acc[i][1] -= (int64_t)m[1], acc[i][2] -= (int64_t)m[2];
          } else {
            acc[i][0] += (int64_t)m[0], acc[i][1] += (int64_t)m[1], acc[i][2] += (int64_t)m[2];
          }
        }
      }
    }
    __syncthreads();  // the next tile's stage overwrites A and XK
  }
#pragma unroll
  for (int i = 0; i < LG_IPT; ++i) {
    if (item[i] < 0) continue;
    SA_DGUARD(item[i] < T, item[i], continue);
#pragma unroll
    for (int l = 0; l < 3; ++l)
      if (acc[i][l]) atomicAdd(reinterpret_cast<u64*>(limbs) + (int64_t)item[i] * 3 + l, (u64)acc[i][l]);
  }
  if (err) atomicOr(gerr, err);
}

// one thread per row: p = 1 / (1 + exp(-z)), z as above
template <bool F32, class TO>
__global__ __launch_bounds__(LG_THREADS) void logit_predict_kernel(LogitIn in, LogitCols C, int d,
                                                                   const double* __restrict__ beta, int64_t n,
                                                                   TO* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * LG_THREADS + threadIdx.x;
  if (row >= n) return;
  double z = beta[d];
  for (int c = 0; c < d; ++c) {
    const double t = beta[c] * logit_x<F32>(in, C.slot[c], row);
    z = z + t;
  }
  out[row] = (TO)(1.0 / (1.0 + exp(-z)));
}

// The argument checks both entry points share; fills the kernels' descriptors.
int logit_args(const char* who, const sa_block* f_blk, const sa_block* i_blk, const int64_t* bits, int64_t words,
               int32_t n_bool, const int32_t* slots, int32_t d, const double* beta, int64_t n, LogitIn* in,
               LogitCols* C) {
  if (!f_blk || !i_blk) return fail(SA_EINVAL, "%s: null block descriptor", who);
  if (d < 0 || d > SA_LOGIT_MAX_COLS) return fail(SA_EINVAL, "%s: d must be 0..%d", who, SA_LOGIT_MAX_COLS);
  if (n < 0 || n >= SA_FX_MAX_ROWS) return fail(SA_EINVAL, "%s: n must be in [0, 2^30)", who);
  if (n_bool < 0 || f_blk->n_cols < 0 || i_blk->n_cols < 0 || words < 0)
    return fail(SA_EINVAL, "%s: negative size", who);
  if (!beta || (d && !slots)) return fail(SA_EINVAL, "%s: null pointer", who);
  for (int c = 0; c < d; ++c) {
    const int kind = slots[c] >> 24, col = slots[c] & 0xFFFFFF;
    if (kind == 0) {
      if (col >= n_bool) return fail(SA_EINVAL, "%s: slot %d names bitmap row %d of %d", who, c, col, n_bool);
      if (!bits) return fail(SA_EINVAL, "%s: null bitmaps", who);
      if (words < (n + 63) / 64) return fail(SA_EINVAL, "%s: the bitmaps hold fewer than n rows", who);
    } else if (kind == 1 || kind == 2) {
      const sa_block* b = kind == 1 ? f_blk : i_blk;
      if (col >= b->n_cols) return fail(SA_EINVAL, "%s: slot %d names column %d of %d", who, c, col, b->n_cols);
      if (n && !b->data) return fail(SA_EINVAL, "%s: null numeric block", who);
      if (b->tile_rows < 16 || b->tile_rows % 16)
        return fail(SA_EINVAL, "%s: numeric block tiles must be multiples of 16 rows", who);
    } else {
      return fail(SA_EINVAL, "%s: slot %d has an unknown kind", who, c);
    }
    if (col >= (1 << 14)) return fail(SA_EINVAL, "%s: slot %d: column numbers stay below 16384", who, c);
    C->slot[c] = (uint16_t)((kind << 14) | col);
  }
  in->f = f_blk->data, in->ib = i_blk->data, in->bits = (const uint64_t*)bits;
  in->Rf = f_blk->tile_rows, in->Ri = i_blk->tile_rows, in->words = words;
  in->Cf = f_blk->n_cols, in->Ci = i_blk->n_cols, in->n_bool = n_bool;
  return SA_OK;
}
}  // namespace

extern "C" int sa_logit_moments(const sa_block* f_blk, const sa_block* i_blk, int32_t f32, const int64_t* bits,
                                int64_t words, int32_t n_bool, const int32_t* slots, int32_t d,
                                const double* beta, const int32_t* col_exp, int32_t loss_exp, const uint8_t* y,
                                const uint8_t* row_mask, int64_t n, int32_t grid_x, double* rowbuf, int64_t* limbs,
                                uint32_t* err, void* stream) {
  LogitIn in = {};
  LogitCols C = {};
  if (int rc = logit_args("sa_logit_moments", f_blk, i_blk, bits, words, n_bool, slots, d, beta, n, &in, &C)) return rc;
  if (!col_exp || !limbs || !err || (n && (!y || !rowbuf))) return fail(SA_EINVAL, "sa_logit_moments: null pointer");
  if (grid_x < 0) return fail(SA_EINVAL, "sa_logit_moments: grid_x < 0");
  // every item's exponent stays a scale exponent: E_j + E_k - 2 in [SA_FX_EXP_MIN, SA_FX_EXP_MAX]
  for (int c = 0; c <= d; ++c) {
    if (col_exp[c] < SA_LOGIT_EXP_MIN || col_exp[c] > SA_LOGIT_EXP_MAX)
      return fail(SA_EINVAL, "sa_logit_moments: col_exp[%d] = %d is outside [%d, %d]", c, col_exp[c],
                  SA_LOGIT_EXP_MIN, SA_LOGIT_EXP_MAX);
    C.E[c] = (int16_t)col_exp[c];
  }
  if (loss_exp < SA_FX_EXP_MIN || loss_exp > SA_FX_EXP_MAX)
    return fail(SA_EINVAL, "sa_logit_moments: loss_exp = %d is outside [%d, %d]", loss_exp, SA_FX_EXP_MIN,
                SA_FX_EXP_MAX);
  const int D = d + 1;
  const int64_t T = (int64_t)D * (D + 1) / 2 + D + 1;
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = check_hip(hipMemsetAsync(limbs, 0, sizeof(int64_t) * 3 * (size_t)T, st), "memset limbs")) return rc;
  if (int rc = check_hip(hipMemsetAsync(err, 0, sizeof(uint32_t), st), "memset error word")) return rc;
  if (n == 0) return SA_OK;
  const dim3 rows_grid((unsigned)((n + LG_THREADS - 1) / LG_THREADS));
  if (f32)
    hipLaunchKernelGGL(logit_rows_kernel<true>, rows_grid, dim3(LG_THREADS), 0, st, in, C, (int)d, beta, y, row_mask,
                       n, rowbuf, err);
  else
    hipLaunchKernelGGL(logit_rows_kernel<false>, rows_grid, dim3(LG_THREADS), 0, st, in, C, (int)d, beta, y, row_mask,
                       n, rowbuf, err);
  if (int rc = check_launch("logit_rows_kernel")) return rc;
  const int64_t n_tiles = (n + LG_TILE - 1) / LG_TILE;
  const int n_jb = (D + 2 + LG_JB - 1) / LG_JB, n_kb = (D + LG_KB - 1) / LG_KB;
  int64_t gx = grid_x;
  if (gx == 0) {
    int64_t used = 0;  // blocks that hold an item (the kernel's own test)
    for (int jb = 0; jb < n_jb; ++jb)
      for (int kb = 0; kb < n_kb; ++kb) {
        const int j0 = jb * LG_JB, k0 = kb * LG_KB;
        const int k_last = k0 + LG_KB - 1 < D - 1 ? k0 + LG_KB - 1 : D - 1;
        used += (j0 < D && k_last >= j0) || (j0 + LG_JB - 1 >= D && j0 < D + 2);
      }
    gx = (int64_t)device_cus(current_device()) * SA_LOGIT_WG_PER_CU / used;
    if (gx < 1) gx = 1;
  }
  if (gx > n_tiles) gx = n_tiles;
  const dim3 grid((unsigned)gx, (unsigned)(n_jb * n_kb));
  if (f32)
    hipLaunchKernelGGL(logit_pairs_kernel<true>, grid, dim3(LG_THREADS), 0, st, in, C, (int)d, (int)loss_exp,
                       (const double*)rowbuf, n, n_tiles, n_kb, limbs, err);
  else
    hipLaunchKernelGGL(logit_pairs_kernel<false>, grid, dim3(LG_THREADS), 0, st, in, C, (int)d, (int)loss_exp,
                       (const double*)rowbuf, n, n_tiles, n_kb, limbs, err);
  return check_launch("logit_pairs_kernel");
}

extern "C" int sa_logit_predict(const sa_block* f_blk, const sa_block* i_blk, int32_t f32, const int64_t* bits,
                                int64_t words, int32_t n_bool, const int32_t* slots, int32_t d,
                                const double* beta, int64_t n, int32_t out_f32, void* out, void* stream) {
  LogitIn in = {};
  LogitCols C = {};
  if (int rc = logit_args("sa_logit_predict", f_blk, i_blk, bits, words, n_bool, slots, d, beta, n, &in, &C)) return rc;
  if (n == 0) return SA_OK;
  if (!out) return fail(SA_EINVAL, "sa_logit_predict: null output");
  const dim3 grid((unsigned)((n + LG_THREADS - 1) / LG_THREADS));
  const hipStream_t st = (hipStream_t)stream;
#define LG_PREDICT(F32, TO) \
  hipLaunchKernelGGL((logit_predict_kernel<F32, TO>), grid, dim3(LG_THREADS), 0, st, in, C, (int)d, beta, n, (TO*)out)
  if (f32 && out_f32) LG_PREDICT(true, float);
  else if (f32) LG_PREDICT(true, double);
  else if (out_f32) LG_PREDICT(false, float);
  else LG_PREDICT(false, double);
#undef LG_PREDICT
  return check_launch("logit_predict_kernel");
}
