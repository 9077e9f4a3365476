// Reproducible histogram gradient boosting on the VAEP feature blocks (gfx950): the `fit` between
// `compute_features` / `compute_labels` and `rate` (reference vaep/base.py:139-213), trained where
// the features already are.  Binary logistic loss, depth-limited trees on pre-binned features,
// xgboost's `hist` rules (float32 values, `x < threshold` goes left, missing goes right).
//
// The arithmetic contract (DESIGN.md §3 "Boosted-tree training", restated in numpy in
// tests/boost_reference.py) makes the trained model the same bit for bit from run to run and for
// any row order: gradients are quantised to int32 at scale 2^30, every histogram is an int64 sum
// (LDS integer atomics, then 64-bit integer global atomics: integer addition commutes), a split's
// gain is a fixed sequence of IEEE float64 operations on those sums, and the arg-max is reduced in
// index order (no float atomics anywhere).
//
// Data: numeric features as a feature-major uint8 bin matrix [F_num, ld] (sa_boost_bin); bool
// features stay the Arrow bitmaps the feature pass writes (bit i of word w = row 64w + i): a bool
// column's histogram is "bit set" (bin 1) against "node total minus bit set" (bin 0).  A row's
// node is its heap index in the round's complete tree (root 0, children 2k+1 / 2k+2), one byte;
// SA_BOOST_NO_NODE marks a row that takes no part (a held-out row).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "sa_common.h"
#include "sa_internal.h"

using namespace sa;

namespace {
typedef unsigned long long u64;
constexpr int BINS = 256;
constexpr int NO_NODE = SA_BOOST_NO_NODE;
constexpr int BB_THREADS = 256;                       // sa_boost_bin: 4 rows per thread
constexpr int BB_TILE = SA_BOOST_BIN_TILE;
constexpr int HB_THREADS = 256;                       // sa_boost_hist_bits
constexpr int HB_TILE = SA_BOOST_BITS_TILE;           // rows per workgroup
constexpr int HB_WORDS = HB_TILE / 64;
constexpr int HB_ACC_BYTES = SA_BOOST_BITS_ACC_BYTES; // LDS for the (column, node) sums of one pass
constexpr int HN_THREADS = 256;                       // sa_boost_hist_bins: 4 rows per thread and step
constexpr int HN_TILE = SA_BOOST_BINS_TILE;
constexpr int HN_FG = SA_BOOST_FEATURE_GROUP;
static_assert(BB_TILE == BB_THREADS * 4 && HN_TILE == HN_THREADS * 4 && HB_TILE % 64 == 0, "tile shapes");
static_assert(sizeof(sa_boost_node) == 48, "sa_boost_node layout");

__device__ __forceinline__ void add64(int64_t* p, int64_t v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

// ---------------------------------------------------------------------------------------- bins
// bin(x) = #{i : c_i <= x32}, NaN -> 255.  One workgroup per (row tile, numeric feature); the
// feature's cut table is staged in LDS and searched by bisection; 4 rows per thread, one 4-B store.
template <int KIND>  // 0: f64 / i64 blocks, 1: float32 blocks
__global__ __launch_bounds__(BB_THREADS) void boost_bin_kernel(sa_block Bf, sa_block Bi, const int32_t* __restrict__ slots,
                                                                const int32_t* __restrict__ num_feat,
                                                                const int32_t* __restrict__ cut_start,
                                                                const float* __restrict__ cuts, int64_t n,
                                                                uint8_t* __restrict__ bins, int64_t ld) {
  __shared__ float lc[BINS];
  const int r = blockIdx.y;
  const int f = num_feat[r];
  const int c0 = cut_start[f];
  int m = cut_start[f + 1] - c0;
  m = m < 0 ? 0 : (m > SA_BOOST_MAX_CUTS ? SA_BOOST_MAX_CUTS : m);
  for (int i = threadIdx.x; i < m; i += BB_THREADS) lc[i] = cuts[c0 + i];
  __syncthreads();
  const int64_t j0 = (int64_t)blockIdx.x * BB_TILE + (int64_t)threadIdx.x * 4;
  if (j0 >= n) return;
  const int32_t slot = slots[r];
  const bool isf = (slot >> 24) == 1;
  const sa_block& B = isf ? Bf : Bi;
  const int64_t col = slot & 0xFFFFFF;
  SA_DGUARD(col < B.n_cols, col, return);
  uint32_t packed = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t j = j0 + q;
    if (j >= n) break;  // the padding rows of the group: bin 0
    const int64_t t = j / B.tile_rows;
    const int64_t at = (t * B.n_cols + col) * B.tile_rows + (j - t * B.tile_rows);
    float x;
    if (KIND == 1)
      x = ((const float*)B.data)[at];
    else if (isf)
      x = (float)((const double*)B.data)[at];
    else
      x = (float)(double)((const int64_t*)B.data)[at];  // the predictor's int64 -> double -> float
    uint32_t b;
    if (isnan(x)) {
      b = SA_BOOST_MISSING_BIN;
    } else {
      int lo = 0, hi = m;  // the first cut > x
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lc[mid] <= x)
          lo = mid + 1;
        else
          hi = mid;
      }
      b = (uint32_t)lo;
    }
    packed |= b << (8 * q);
  }
  *reinterpret_cast<uint32_t*>(bins + (int64_t)r * ld + j0) = packed;
}

// ---------------------------------------------------------------------------------------- gradients
__device__ __host__ __forceinline__ u64 fmix64(u64 z) {  // splitmix64's finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

struct grad_tuning {  // sa_boost_grad's weights and row sample: the TUNED kernel alone reads it
  const float* weight;
  float spw, scale;
  const int64_t* keys;
  u64 round_base, thr;
};

// TUNED (contract items 13, 14 and 16): the effective weight we = w * (y ? s : 1) folded in before
// the quantisation at scale 2^(30 - e) (|g| <= we <= 2^e keeps |gq| <= 2^30), and the round's row
// sample from a counter hash of (seed, round, row key): a row outside it gets gq = hq = 0 -- the
// histogram kernels skip zero adds -- and still walks the tree.  Each product is its own statement.
// With every tuning argument neutral the two instantiations compute the same bits (g * 1.0f is g, the
// scale is 2^30, thr = 2^32 skips the hash); sa_boost_grad then launches the shorter one.
template <bool TUNED>
__global__ __launch_bounds__(256) void boost_grad_kernel(const float* __restrict__ margin, const uint8_t* __restrict__ y,
                                                          const uint8_t* __restrict__ mask, int64_t n,
                                                          int32_t* __restrict__ gq, int32_t* __restrict__ hq,
                                                          float* __restrict__ p_out, uint8_t* __restrict__ node,
                                                          grad_tuning tu) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const float m = margin[j];
  const float p = 1.0f / (1.0f + expf(-m));
  if (p_out) p_out[j] = p;
  if (gq) {
    const bool pos = y[j] != 0;
    bool in = true;
    if (TUNED) {
      const u64 key = tu.keys ? (u64)tu.keys[j] : (u64)j;
      in = tu.thr > 0xFFFFFFFFull || (fmix64(tu.round_base + key) >> 32) < tu.thr;
    }
    int32_t gi = 0, hi = 0;
    if (in) {
      const float yy = pos ? 1.0f : 0.0f;
      float g = p - yy;
      float h = p * (1.0f - p);
      float scale = 1073741824.0f;
      if (TUNED) {
        const float w = tu.weight ? tu.weight[j] : 1.0f;
        const float we = w * (pos ? tu.spw : 1.0f);
        g = g * we;
        h = h * we;
        scale = tu.scale;
      }
      const float gs = g * scale;
      const float hs = h * scale;
      gi = (int32_t)rintf(gs);
      hi = (int32_t)rintf(hs);
    }
    gq[j] = gi;
    hq[j] = hi;
  }
  if (node) node[j] = (!mask || mask[j]) ? 0 : NO_NODE;
}

// fit_batch's row keys: fm(game_id) + action_id, wrapping (contract item 16)
__global__ __launch_bounds__(256) void boost_row_keys_kernel(const int64_t* __restrict__ game_id,
                                                              const int64_t* __restrict__ action_id, int64_t n,
                                                              int64_t* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  keys[j] = (int64_t)(fmix64((u64)game_id[j]) + (u64)action_id[j]);
}

// ---------------------------------------------------------------------------------------- bitmaps
// One workgroup per tile of HB_TILE rows: the rows' gq, hq and level-local node are staged in LDS
// once; then work item (column c, word w) -- adjacent threads take adjacent words of one column:
// coalesced 8-B loads, and a dense column's words spread over threads -- visits its set bits only
// and adds the row's gradients to the LDS sums of (c, node) with LDS integer atomics.  The sums
// of `cc` columns fit LDS at a time; each pass ends with one 64-bit global atomic per non-zero sum.
__global__ __launch_bounds__(HB_THREADS) void boost_hist_bits_kernel(
    const u64* __restrict__ bits, int64_t wstride, const int32_t* __restrict__ bit_rows,
    const int32_t* __restrict__ bit_feat, int n_bool, const int32_t* __restrict__ gq, const int32_t* __restrict__ hq,
    const uint8_t* __restrict__ node, int64_t n, int node0, int n_nodes, int F, int cc, int64_t* __restrict__ hist,
    sa_boost_node* __restrict__ tree, int add_totals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hb_lds[];
  u64* acc = reinterpret_cast<u64*>(hb_lds);                                // [cc][n_nodes][2]
  int32_t* sg = reinterpret_cast<int32_t*>(hb_lds + (size_t)cc * n_nodes * 16);  // [HB_TILE]
  int32_t* sh = sg + HB_TILE;
  uint8_t* sn = reinterpret_cast<uint8_t*>(sh + HB_TILE);
  __shared__ u64 ltot[2 * SA_BOOST_MAX_LEVEL_NODES];
  const int tid = threadIdx.x;
  const int64_t R0 = (int64_t)blockIdx.x * HB_TILE;
  const int nacc = cc * n_nodes * 2;
  for (int i = tid; i < nacc; i += HB_THREADS) acc[i] = 0;
  if (tid < 2 * SA_BOOST_MAX_LEVEL_NODES) ltot[tid] = 0;
  for (int i = tid; i < HB_TILE; i += HB_THREADS) {
    const int64_t r = R0 + i;
    int k = NO_NODE;
    int32_t g = 0, h = 0;
    if (r < n) {
      const int nd = (int)node[r] - node0;
      if (nd >= 0 && nd < n_nodes && node[r] != NO_NODE) {
        k = nd;
        g = gq[r];
        h = hq[r];
      }
    }
    sn[i] = (uint8_t)k;
    sg[i] = g;
    sh[i] = h;
  }
  __syncthreads();
  if (add_totals) {  // the nodes' totals: this thread's rows, then one global atomic per node
    for (int i = tid; i < HB_TILE; i += HB_THREADS) {
      const int k = sn[i];
      if (k == NO_NODE) continue;
      if (sg[i]) atomicAdd(&ltot[2 * k], (u64)(int64_t)sg[i]);
      if (sh[i]) atomicAdd(&ltot[2 * k + 1], (u64)(int64_t)sh[i]);
    }
    __syncthreads();
    if (tid < 2 * n_nodes && ltot[tid]) {
      sa_boost_node* t = tree + node0 + (tid >> 1);
      add64((tid & 1) ? &t->H : &t->G, (int64_t)ltot[tid]);
    }
  }
  const int64_t n_words = (n + 63) / 64;
  for (int c0 = 0; c0 < n_bool; c0 += cc) {
    const int ncol = n_bool - c0 < cc ? n_bool - c0 : cc;
    for (int it = tid; it < ncol * HB_WORDS; it += HB_THREADS) {
      const int c = it / HB_WORDS, w = it - c * HB_WORDS;
      const int64_t gw = R0 / 64 + w;
      if (gw >= n_words) continue;
      u64 word = bits[(int64_t)bit_rows[c0 + c] * wstride + gw];
      const int64_t rb = gw * 64;
      if (rb + 64 > n) word &= (1ull << (n - rb)) - 1;  // rows >= n never count
      u64* A = acc + (size_t)c * n_nodes * 2;
      while (word) {
        const int b = __builtin_ctzll(word);
        word &= word - 1;
        const int i = w * 64 + b;
        const int k = sn[i];
        if (k == NO_NODE) continue;
        if (sg[i]) atomicAdd(&A[2 * k], (u64)(int64_t)sg[i]);
        if (sh[i]) atomicAdd(&A[2 * k + 1], (u64)(int64_t)sh[i]);
      }
    }
    __syncthreads();
    for (int i = tid; i < ncol * n_nodes * 2; i += HB_THREADS) {
      const u64 v = acc[i];
      if (!v) continue;
      acc[i] = 0;
      const int c = i / (n_nodes * 2), rem = i - c * n_nodes * 2;
      const int k = rem >> 1, f = bit_feat[c0 + c];
      SA_DGUARD(f >= 0 && f < F, f, continue);
      add64(hist + (((int64_t)k * F + f) * BINS + 1) * 2 + (rem & 1), (int64_t)v);
    }
    __syncthreads();
  }
}

// bin 0 of every bool column = the node's total minus bin 1 (after the sums above are complete)
__global__ __launch_bounds__(256) void boost_bits_fill_kernel(const int32_t* __restrict__ bit_feat, int n_bool,
                                                               int node0, int n_nodes, int F, int64_t* __restrict__ hist,
                                                               const sa_boost_node* __restrict__ tree) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_bool * n_nodes) return;
  const int k = i / n_bool, f = bit_feat[i - k * n_bool];
  SA_DGUARD(f >= 0 && f < F, f, return);
  int64_t* h = hist + ((int64_t)k * F + f) * BINS * 2;
  h[0] = tree[node0 + k].G - h[2];
  h[1] = tree[node0 + k].H - h[3];
}

// ---------------------------------------------------------------------------------------- bins
// Workgroup (x, y): feature group y (fg features), row steps x, x + gridDim.x, ...; an int64
// histogram [fg][n_nodes][256][2] in LDS, filled with LDS integer atomics from coalesced 4-B
// reads of 4 rows' bins, flushed once at the end with 64-bit global atomics (zero entries skipped).
// ROWS: list entry r is row num_rows[r] of the bin matrix (a round's column sample) instead of row r.
template <bool ROWS>
__global__ __launch_bounds__(HN_THREADS) void boost_hist_bins_kernel(
    const uint8_t* __restrict__ bins, int64_t ld, const int32_t* __restrict__ num_feat,
    const int32_t* __restrict__ num_rows, int n_bin_rows, int n_num,
    const int32_t* __restrict__ gq, const int32_t* __restrict__ hq, const uint8_t* __restrict__ node, int64_t n,
    int node0, int n_nodes, int F, int fg, int64_t* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hn_lds[];
  u64* H = reinterpret_cast<u64*>(hn_lds);  // [fg][n_nodes][256][2]
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * fg;
  const int nf = n_num - r0 < fg ? n_num - r0 : fg;
  const int nh = nf * n_nodes * BINS * 2;
  for (int i = tid; i < nh; i += HN_THREADS) H[i] = 0;
  __syncthreads();
  const int64_t steps = (n + HN_TILE - 1) / HN_TILE;
  for (int64_t s = blockIdx.x; s < steps; s += gridDim.x) {
    const int64_t j0 = s * HN_TILE + (int64_t)tid * 4;
    if (j0 >= n) continue;
    const uint32_t nd4 = *reinterpret_cast<const uint32_t*>(node + j0);
    int k[4];
    int32_t g[4], h[4];
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int raw = (int)((nd4 >> (8 * q)) & 0xFF);
      const int nd = raw - node0;
      const bool in = j0 + q < n && raw != NO_NODE && nd >= 0 && nd < n_nodes;
      k[q] = in ? nd : -1;
      g[q] = in ? gq[j0 + q] : 0;
      h[q] = in ? hq[j0 + q] : 0;
      any |= in;
    }
    if (!any) continue;
    for (int fi = 0; fi < nf; ++fi) {
      int row = r0 + fi;
      if (ROWS) {
        row = num_rows[r0 + fi];
        if (row < 0 || row >= n_bin_rows) continue;  // never read outside the matrix
      }
      const uint32_t b4 = *reinterpret_cast<const uint32_t*>(bins + (int64_t)row * ld + j0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (k[q] < 0) continue;
        u64* e = H + ((size_t)(fi * n_nodes + k[q]) * BINS + ((b4 >> (8 * q)) & 0xFF)) * 2;
        if (g[q]) atomicAdd(e, (u64)(int64_t)g[q]);
        if (h[q]) atomicAdd(e + 1, (u64)(int64_t)h[q]);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nh; i += HN_THREADS) {
    const u64 v = H[i];
    if (!v) continue;
    const int fi = i / (n_nodes * BINS * 2), rem = i - fi * n_nodes * BINS * 2;
    const int k = rem / (BINS * 2), e = rem - k * BINS * 2;
    const int f = num_feat[r0 + fi];
    SA_DGUARD(f >= 0 && f < F, f, continue);
    add64(hist + ((int64_t)k * F + f) * BINS * 2 + e, (int64_t)v);
  }
}

// ---------------------------------------------------------------------------------------- splits
// contract item 15: T(G) = G > a ? G - a : (G < -a ? G + a : 0); with a == 0, T(G) == G exactly
__device__ __forceinline__ double l1_shrink(double G, double a) { return G > a ? G - a : (G < -a ? G + a : 0.0); }

__device__ __forceinline__ double split_gain(double GL, double HL, double GR, double HR, double G, double H,
                                             double lambda, double alpha) {
  const double TL = l1_shrink(GL, alpha), TR = l1_shrink(GR, alpha), TG = l1_shrink(G, alpha);
  return ((TL * TL) / (HL + lambda) + (TR * TR) / (HR + lambda)) - (TG * TG) / (H + lambda);
}

// a candidate (gain, index) beats another on a larger gain, then on the lower index
__device__ __forceinline__ bool better(double ga, int ia, double gb, int ib) {
  return ga > gb || (ga == gb && ia < ib);
}

// One workgroup per (node, feature): the inclusive scan over the feature's bins, the float64 gain
// of every cut and the best cut (largest gain, then the lowest cut) -> best_gain / best_cut
// (-inf / -1 when no cut is valid, and for a feature outside the round's column sample: fmask[f]
// == 0).  `s` = 2^(e - 30) turns the integer sums into weighted sums (contract item 14).
__global__ __launch_bounds__(BINS) void boost_scan_kernel(const int64_t* __restrict__ hist,
                                                           const int32_t* __restrict__ cut_start, int F, int node0,
                                                           double lambda, double mcw, double alpha, double s,
                                                           const uint8_t* __restrict__ fmask,
                                                           const sa_boost_node* __restrict__ tree,
                                                           double* __restrict__ best_gain,
                                                           int32_t* __restrict__ best_cut) {
  __shared__ int64_t sg[2][BINS], sh[2][BINS];
  __shared__ double rg[BINS];
  __shared__ int ri[BINS];
  const int k = blockIdx.y, f = blockIdx.x, i = threadIdx.x;
  const sa_boost_node nd = tree[node0 + k];
  if ((!nd.exists && node0 != 0) || (fmask && !fmask[f])) {  // (the root always exists)
    if (i == 0) {
      best_gain[(int64_t)k * F + f] = -INFINITY;
      best_cut[(int64_t)k * F + f] = -1;
    }
    return;
  }
  int m = cut_start[f + 1] - cut_start[f];
  m = m < 0 ? 0 : (m > SA_BOOST_MAX_CUTS ? SA_BOOST_MAX_CUTS : m);
  const int64_t* h = hist + ((int64_t)k * F + f) * BINS * 2;
  sg[0][i] = h[2 * i];
  sh[0][i] = h[2 * i + 1];
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < BINS; d <<= 1) {  // integer sums: any order gives the same prefix
    sg[cur ^ 1][i] = sg[cur][i] + (i >= d ? sg[cur][i - d] : 0);
    sh[cur ^ 1][i] = sh[cur][i] + (i >= d ? sh[cur][i - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  double gain = -INFINITY;
  int idx = -1;
  if (i < m) {
    const int64_t gl = sg[cur][i], hl = sh[cur][i];
    const double G = (double)nd.G * s, H = (double)nd.H * s;
    const double GL = (double)gl * s, HL = (double)hl * s;
    const double GR = (double)(nd.G - gl) * s, HR = (double)(nd.H - hl) * s;
    if (HL >= mcw && HR >= mcw) {
      const double v = split_gain(GL, HL, GR, HR, G, H, lambda, alpha);
      if (!isnan(v)) {
        gain = v;
        idx = i;
      }
    }
  }
  rg[i] = gain;
  ri[i] = idx;
  __syncthreads();
  for (int d = BINS / 2; d > 0; d >>= 1) {
    if (i < d && ri[i + d] >= 0 && (ri[i] < 0 || better(rg[i + d], ri[i + d], rg[i], ri[i]))) {
      rg[i] = rg[i + d];
      ri[i] = ri[i + d];
    }
    __syncthreads();
  }
  if (i == 0) {
    best_gain[(int64_t)k * F + f] = rg[0];
    best_cut[(int64_t)k * F + f] = ri[0];
  }
}

// One workgroup per node: the best feature (largest gain, then the lowest feature index), the
// node's leaf value, and -- when it splits -- its record and its children's totals.
__global__ __launch_bounds__(256) void boost_decide_kernel(const int64_t* __restrict__ hist,
                                                            const int32_t* __restrict__ cut_start,
                                                            const float* __restrict__ cuts, int F, int node0,
                                                            int leaf_only, double lambda, double gamma, double eta,
                                                            double alpha, double s,
                                                            const double* __restrict__ best_gain,
                                                            const int32_t* __restrict__ best_cut,
                                                            sa_boost_node* __restrict__ tree) {
  __shared__ double rg[256];
  __shared__ int rf[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  sa_boost_node* nd = tree + node0 + k;
  if (!nd->exists && node0 != 0) return;  // (the root always exists)
  double gain = -INFINITY;
  int bf = -1;
  if (!leaf_only)
    for (int f = tid; f < F; f += 256) {  // ascending f: a later equal gain does not replace
      const double v = best_gain[(int64_t)k * F + f];
      if (best_cut[(int64_t)k * F + f] >= 0 && (bf < 0 || v > gain)) {
        gain = v;
        bf = f;
      }
    }
  rg[tid] = gain;
  rf[tid] = bf;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d && rf[tid + d] >= 0 && (rf[tid] < 0 || better(rg[tid + d], rf[tid + d], rg[tid], rf[tid]))) {
      rg[tid] = rg[tid + d];
      rf[tid] = rf[tid + d];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double G = (double)nd->G * s, H = (double)nd->H * s;
  nd->value = (float)(eta * (-(l1_shrink(G, alpha) / (H + lambda))));
  nd->exists = 1;
  nd->feature = -1;
  nd->cut = -1;
  nd->thr = 0.0f;
  nd->gain = 0.0;
  const int f = rf[0];
  if (leaf_only || f < 0 || !(rg[0] > gamma)) return;
  const int cut = best_cut[(int64_t)k * F + f];
  const int64_t* h = hist + ((int64_t)k * F + f) * BINS * 2;
  int64_t gl = 0, hl = 0;
  for (int b = 0; b <= cut; ++b) {
    gl += h[2 * b];
    hl += h[2 * b + 1];
  }
  nd->feature = f;
  nd->cut = cut;
  nd->thr = cuts[cut_start[f] + cut];
  nd->gain = rg[0];
  sa_boost_node* L = tree + 2 * (node0 + k) + 1;
  L[0].G = gl;
  L[0].H = hl;
  L[0].exists = 1;
  L[0].feature = -1;
  L[1].G = nd->G - gl;
  L[1].H = nd->H - hl;
  L[1].exists = 1;
  L[1].feature = -1;
}

// ---------------------------------------------------------------------------------------- advance
// ADD = false: a row in a split node of the level moves to the child its bitmap bit or bin picks
// (bit set / bin > cut: right).  ADD = true: every row's margin gains its node's leaf value.
template <bool ADD>
__global__ __launch_bounds__(256) void boost_advance_kernel(const sa_boost_node* __restrict__ tree, int node0,
                                                             int n_nodes, const int32_t* __restrict__ fmap,
                                                             const u64* __restrict__ bits, int64_t wstride,
                                                             const uint8_t* __restrict__ bins, int64_t ld, int64_t n,
                                                             uint8_t* __restrict__ node, float* __restrict__ margin) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int raw = node[j];
  if (raw == NO_NODE) return;
  if (ADD) {
    margin[j] = margin[j] + tree[raw].value;
    return;
  }
  const int nd = raw - node0;
  if (nd < 0 || nd >= n_nodes) return;
  const int f = tree[raw].feature;
  if (f < 0) return;
  const int32_t slot = fmap[f];
  const int64_t row = slot & 0xFFFFFF;
  bool right;
  if ((slot >> 24) == 0)
    right = (bits[row * wstride + (j >> 6)] >> (j & 63)) & 1;
  else
    right = (int)bins[row * ld + j] > tree[raw].cut;
  node[j] = (uint8_t)(2 * raw + 1 + (right ? 1 : 0));
}

// ---------------------------------------------------------------------------------------- apply
// One finished tree applied to a list of rows (the held-out rows of a round; every row when the
// kept trees are replayed): one thread per list entry.  The workgroup stages what the walk reads
// of the round's node table -- at most 127 records of 48 bytes -- in LDS once, as 12 bytes per
// node: the split feature's place (fmap resolved; -1 = leaf), its cut and the node's value.  The
// walk is the predictor's: bit set / bin > cut goes right, so the missing bin 255 goes right; at
// most max_depth steps, so the node index stays below 2^(max_depth+1) - 1.  The bitmap and bin
// reads are gathers by row.  A list entry whose row is outside [0, n) is left untouched.
constexpr int AP_THREADS = 256;
constexpr int AP_NODES = (2 << SA_BOOST_MAX_DEPTH) - 1;

__global__ __launch_bounds__(AP_THREADS) void boost_apply_kernel(const sa_boost_node* __restrict__ tree, int max_depth,
                                                                  const int32_t* __restrict__ fmap,
                                                                  const u64* __restrict__ bits, int64_t wstride,
                                                                  const uint8_t* __restrict__ bins, int64_t ld,
                                                                  const int64_t* __restrict__ rows, int64_t n_rows,
                                                                  int64_t n, float* __restrict__ margin,
                                                                  float* __restrict__ p) {
  __shared__ int32_t s_slot[AP_NODES];
  __shared__ int32_t s_cut[AP_NODES];
  __shared__ float s_val[AP_NODES];
  const int n_nodes = (2 << max_depth) - 1;
  for (int k = threadIdx.x; k < n_nodes; k += AP_THREADS) {
    const int f = tree[k].feature;
    int32_t slot = -1;
    if (f >= 0) {
      slot = fmap[f];
      // a split on a kind of feature whose data was not passed cannot be walked: the walk ends here
      if (slot < 0 || ((slot >> 24) == 0 ? bits == nullptr : bins == nullptr)) slot = -1;
    }
    s_slot[k] = slot;
    s_cut[k] = tree[k].cut;
    s_val[k] = tree[k].value;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t j = rows ? rows[i] : i;
  if (j < 0 || j >= n) return;
  int node = 0;
  for (int d = 0; d < max_depth; ++d) {
    const int32_t slot = s_slot[node];
    if (slot < 0) break;
    const int64_t row = slot & 0xFFFFFF;
    bool right;
    if ((slot >> 24) == 0)
      right = (bits[row * wstride + (j >> 6)] >> (j & 63)) & 1;
    else
      right = (int)bins[row * ld + j] > s_cut[node];
    node = 2 * node + 1 + (right ? 1 : 0);
  }
  const float m = margin[i] + s_val[node];
  margin[i] = m;
  if (p) p[i] = 1.0f / (1.0f + expf(-m));
}

// ---------------------------------------------------------------------------------------- exchange
// The level histogram's used entries as one contiguous buffer of (G, H) pairs, for the ranks' one
// integer all-reduce per level.  pairs [n_bool + n_num]: a node's payload
// pairs as dense pair offsets feature * 256 + bin -- every bool feature's bin 1, then every numeric
// feature's bins 0 .. m and 255.  Payload: `head` pairs (the root's totals at level 0), the bool
// pairs of every node, the numeric pairs of every node.  Payload pair i of the body is dense pair
// exchange_dense(i); one thread per pair, one 16-B load and one 16-B store, no atomics.
typedef long long pair64 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int64_t exchange_dense(int64_t i, const int32_t* __restrict__ pairs, int n_bool, int n_num,
                                                  int n_nodes, int F) {
  const int64_t nb = (int64_t)n_nodes * n_bool;
  int k, j;
  if (i < nb) {
    k = (int)(i / n_bool);
    j = (int)(i - (int64_t)k * n_bool);
  } else {
    k = (int)((i - nb) / n_num);
    j = n_bool + (int)((i - nb) - (int64_t)k * n_num);
  }
  return (int64_t)k * F * BINS + pairs[j];
}

__global__ __launch_bounds__(256) void boost_hist_pack_kernel(const pair64* __restrict__ hist,
                                                               const sa_boost_node* __restrict__ tree,
                                                               const int32_t* __restrict__ pairs, int n_bool, int n_num,
                                                               int n_nodes, int F, int head, pair64* __restrict__ payload) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - head;
  if (i >= (int64_t)n_nodes * (n_bool + n_num)) return;
  if (i < 0) {  // level 0: this rank's root totals
    payload[0] = pair64{(long long)tree[0].G, (long long)tree[0].H};
    return;
  }
  const int64_t d = exchange_dense(i, pairs, n_bool, n_num, n_nodes, F);
  SA_DGUARD(d >= 0 && d < (int64_t)n_nodes * F * BINS, d, return);
  payload[head + i] = hist[d];
}

__global__ __launch_bounds__(256) void boost_hist_unpack_kernel(const pair64* __restrict__ payload,
                                                                 const int32_t* __restrict__ pairs, int n_bool,
                                                                 int n_num, int n_nodes, int F, int head,
                                                                 pair64* __restrict__ hist,
                                                                 sa_boost_node* __restrict__ tree) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - head;
  if (i >= (int64_t)n_nodes * (n_bool + n_num)) return;
  if (i < 0) {  // level 0: the summed root totals (G, H: the record's first 16 bytes)
    *reinterpret_cast<pair64*>(&tree[0].G) = payload[0];
    return;
  }
  const int64_t d = exchange_dense(i, pairs, n_bool, n_num, n_nodes, F);
  SA_DGUARD(d >= 0 && d < (int64_t)n_nodes * F * BINS, d, return);
  hist[d] = payload[head + i];
}

// level-local node range [node0, node0 + n_nodes): one whole level of the heap, at most 32 nodes
bool level_ok(int node0, int n_nodes) {
  return n_nodes >= 1 && n_nodes <= SA_BOOST_MAX_LEVEL_NODES && (n_nodes & (n_nodes - 1)) == 0 &&
         node0 == n_nodes - 1;
}

// a bitmap argument: 8-byte aligned words and a byte stride that holds n rows
bool bits_ok(const uint64_t* bits, int64_t bits_stride, int64_t n) {
  return bits_stride % 8 == 0 && bits_stride >= 8 * ((n + 63) / 64) && ((uintptr_t)bits & 7u) == 0;
}

}  // namespace

extern "C" int sa_boost_bin(const sa_block* f64_blk, const sa_block* i64_blk, int32_t f32, const int32_t* slots,
                            const int32_t* num_feat, const int32_t* cut_start, const float* cuts, int32_t n_num,
                            int64_t n, uint8_t* bins, int64_t ld, void* stream) {
  if (n < 0 || n_num < 0 || ld < n || ld % 4 != 0) return fail(SA_EINVAL, "sa_boost_bin: bad sizes");
  if (n_num > 0 && (!slots || !num_feat || !cut_start || !cuts || !bins || ((uintptr_t)bins & 3u)))
    return fail(SA_EINVAL, "sa_boost_bin: null or misaligned pointer");
  sa_block z{nullptr, 0, 0, 16};
  const sa_block Bf = f64_blk ? *f64_blk : z, Bi = i64_blk ? *i64_blk : z;
  if (Bf.tile_rows < 1 || Bi.tile_rows < 1) return fail(SA_EINVAL, "sa_boost_bin: bad tile");
  if (n == 0 || n_num == 0) return SA_OK;
  const dim3 grid((unsigned)((n + BB_TILE - 1) / BB_TILE), (unsigned)n_num);
  return with_flags([&](auto F32) {
    hipLaunchKernelGGL((boost_bin_kernel<F32() ? 1 : 0>), grid, dim3(BB_THREADS), 0, (hipStream_t)stream, Bf, Bi, slots,
                       num_feat, cut_start, cuts, n, bins, ld);
    return check_launch("boost_bin_kernel");
  }, f32 != 0);
}

extern "C" int sa_boost_grad(const float* margin, const uint8_t* y, const uint8_t* row_mask, int64_t n,
                             const float* weight, float scale_pos_weight, int32_t shift, const int64_t* row_keys,
                             uint64_t seed, int64_t round, uint64_t thr, int32_t* gq, int32_t* hq, float* p,
                             uint8_t* node, void* stream) {
  if (n < 0 || !margin || (gq && (!hq || !y)) || (!gq && hq)) return fail(SA_EINVAL, "sa_boost_grad: bad arguments");
  if (shift < 0 || shift > SA_BOOST_MAX_SHIFT || !(scale_pos_weight > 0.0f) || std::isinf(scale_pos_weight) ||
      round < 0 || thr > (1ull << 32))
    return fail(SA_EINVAL, "sa_boost_grad: bad parameters");
  if (n == 0) return SA_OK;
  const u64 round_base = fmix64(fmix64((u64)seed ^ SA_BOOST_SALT_ROWS) + (u64)round);
  const grad_tuning tu{weight, scale_pos_weight, std::ldexp(1.0f, 30 - shift), row_keys, round_base, (u64)thr};
  const dim3 grid((unsigned)((n + 255) / 256));
  const bool plain = !weight && scale_pos_weight == 1.0f && shift == 0 && !row_keys && thr == (1ull << 32);
  return with_flags([&](auto TUNED) {
    hipLaunchKernelGGL((boost_grad_kernel<TUNED()>), grid, dim3(256), 0, (hipStream_t)stream, margin, y, row_mask, n,
                       gq, hq, p, node, tu);
    return check_launch("boost_grad_kernel");
  }, !plain);
}

extern "C" int sa_boost_row_keys(const int64_t* game_id, const int64_t* action_id, int64_t n, int64_t* keys,
                                 void* stream) {
  if (n < 0 || (n > 0 && (!game_id || !action_id || !keys))) return fail(SA_EINVAL, "sa_boost_row_keys: bad arguments");
  if (n == 0) return SA_OK;
  hipLaunchKernelGGL(boost_row_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     game_id, action_id, n, keys);
  return check_launch("boost_row_keys_kernel");
}

extern "C" int sa_boost_hist_bits(const uint64_t* bits, int64_t bits_stride, const int32_t* bit_rows,
                                  const int32_t* bit_feat, int32_t n_bool, const int32_t* gq, const int32_t* hq,
                                  const uint8_t* node, int64_t n, int32_t node0, int32_t n_nodes, int32_t n_features,
                                  int64_t* hist, sa_boost_node* tree, int32_t add_totals, void* stream) {
  if (n < 0 || n_bool < 0 || n_features < 1 || !level_ok(node0, n_nodes))
    return fail(SA_EINVAL, "sa_boost_hist_bits: bad sizes");
  if (!gq || !hq || !node || !hist || !tree) return fail(SA_EINVAL, "sa_boost_hist_bits: null pointer");
  if (n_bool > 0 && (!bits || !bit_rows || !bit_feat || !bits_ok(bits, bits_stride, n)))
    return fail(SA_EINVAL, "sa_boost_hist_bits: bad bitmaps");
  if (n == 0) return SA_OK;
  int cc = HB_ACC_BYTES / (n_nodes * 16);
  if (cc > n_bool) cc = n_bool;
  if (cc < 1) cc = 1;
  const size_t lds = (size_t)cc * n_nodes * 16 + (size_t)HB_TILE * 9;
  hipLaunchKernelGGL(boost_hist_bits_kernel, dim3((unsigned)((n + HB_TILE - 1) / HB_TILE)), dim3(HB_THREADS), lds,
                     (hipStream_t)stream, (const u64*)bits, bits_stride / 8, bit_rows, bit_feat, n_bool, gq, hq, node,
                     n, node0, n_nodes, n_features, cc, hist, tree, add_totals);
  if (int rc = check_launch("boost_hist_bits_kernel")) return rc;
  if (n_bool == 0) return SA_OK;
  const int items = n_bool * n_nodes;
  hipLaunchKernelGGL(boost_bits_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     bit_feat, n_bool, node0, n_nodes, n_features, hist, tree);
  return check_launch("boost_bits_fill_kernel");
}

extern "C" int sa_boost_hist_bins(const uint8_t* bins, int64_t ld, const int32_t* num_feat, const int32_t* num_rows,
                                  int32_t n_bin_rows, int32_t n_num, const int32_t* gq, const int32_t* hq,
                                  const uint8_t* node, int64_t n, int32_t node0, int32_t n_nodes, int32_t n_features,
                                  int64_t* hist, void* stream) {
  if (n < 0 || n_num < 0 || n_features < 1 || ld < n || ld % 4 != 0 || !level_ok(node0, n_nodes) ||
      (num_rows && n_bin_rows < 1))
    return fail(SA_EINVAL, "sa_boost_hist_bins: bad sizes");
  if (!gq || !hq || !node || !hist || ((uintptr_t)node & 3u))
    return fail(SA_EINVAL, "sa_boost_hist_bins: null or misaligned pointer");
  if (n_num > 0 && (!bins || !num_feat || ((uintptr_t)bins & 3u)))
    return fail(SA_EINVAL, "sa_boost_hist_bins: null or misaligned bins");
  if (n == 0 || n_num == 0) return SA_OK;
  int fg = HN_FG;
  while (fg > 1 && fg * n_nodes > 32) fg >>= 1;  // [fg][n_nodes][256][2] int64 <= 128 KB of LDS
  const size_t lds = (size_t)fg * n_nodes * BINS * 16;
  const int64_t steps = (n + HN_TILE - 1) / HN_TILE;
  const int groups = (n_num + fg - 1) / fg;
  int64_t gx = (int64_t)device_cus(current_device()) * SA_BOOST_BINS_WG_PER_CU / groups;
  if (gx < SA_BOOST_BINS_MIN_GRID_X) gx = SA_BOOST_BINS_MIN_GRID_X;
  if (gx > steps) gx = steps;
  return with_flags([&](auto ROWS) {
    hipLaunchKernelGGL((boost_hist_bins_kernel<ROWS()>), dim3((unsigned)gx, (unsigned)groups), dim3(HN_THREADS), lds,
                       (hipStream_t)stream, bins, ld, num_feat, num_rows, n_bin_rows, n_num, gq, hq, node, n, node0,
                       n_nodes, n_features, fg, hist);
    return check_launch("boost_hist_bins_kernel");
  }, num_rows != nullptr);
}

extern "C" int sa_boost_split(const int64_t* hist, const int32_t* cut_start, const float* cuts, int32_t n_features,
                              int32_t node0, int32_t n_nodes, int32_t leaf_only, double reg_lambda,
                              double min_child_weight, double gamma, double learning_rate, double reg_alpha,
                              int32_t shift, const uint8_t* feature_mask, double* best_gain, int32_t* best_cut,
                              sa_boost_node* tree, void* stream) {
  if (!(reg_alpha >= 0.0) || std::isinf(reg_alpha) || shift < 0 || shift > SA_BOOST_MAX_SHIFT)
    return fail(SA_EINVAL, "sa_boost_split: bad parameters");
  const bool leaf_level = n_nodes == 2 * SA_BOOST_MAX_LEVEL_NODES && node0 == n_nodes - 1;  // below the deepest level
  if (n_features < 1 || !(level_ok(node0, n_nodes) || leaf_level)) return fail(SA_EINVAL, "sa_boost_split: bad sizes");
  if (!tree || (!leaf_only && (!hist || !cut_start || !cuts || !best_gain || !best_cut)))
    return fail(SA_EINVAL, "sa_boost_split: null pointer");
  if (!leaf_only && n_nodes > SA_BOOST_MAX_LEVEL_NODES) return fail(SA_EINVAL, "sa_boost_split: level too deep");
  if (!(reg_lambda >= 0.0) || !(min_child_weight >= 0.0) || std::isnan(gamma) || std::isnan(learning_rate))
    return fail(SA_EINVAL, "sa_boost_split: bad parameters");
  hipStream_t st = (hipStream_t)stream;
  const double s = std::ldexp(1.0, shift - 30);  // an exact power of two: 2^-30 with no weights
  if (!leaf_only) {
    hipLaunchKernelGGL(boost_scan_kernel, dim3((unsigned)n_features, (unsigned)n_nodes), dim3(BINS), 0, st, hist,
                       cut_start, n_features, node0, reg_lambda, min_child_weight, reg_alpha, s, feature_mask, tree,
                       best_gain, best_cut);
    if (int rc = check_launch("boost_scan_kernel")) return rc;
  }
  hipLaunchKernelGGL(boost_decide_kernel, dim3((unsigned)n_nodes), dim3(256), 0, st, hist, cut_start, cuts, n_features,
                     node0, leaf_only, reg_lambda, gamma, learning_rate, reg_alpha, s, best_gain, best_cut, tree);
  return check_launch("boost_decide_kernel");
}

extern "C" int sa_boost_advance(const sa_boost_node* tree, int32_t node0, int32_t n_nodes, const int32_t* fmap,
                                const uint64_t* bits, int64_t bits_stride, const uint8_t* bins, int64_t ld, int64_t n,
                                uint8_t* node, float* margin, void* stream) {
  if (n < 0 || !tree || !node) return fail(SA_EINVAL, "sa_boost_advance: bad arguments");
  if (!margin) {
    if (!level_ok(node0, n_nodes) || !fmap) return fail(SA_EINVAL, "sa_boost_advance: bad level");
    if (bits && !bits_ok(bits, bits_stride, n)) return fail(SA_EINVAL, "sa_boost_advance: bad bitmaps");
    if (bins && ld < n) return fail(SA_EINVAL, "sa_boost_advance: bad bins");
  }
  if (n == 0) return SA_OK;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  return with_flags([&](auto ADD) {
    hipLaunchKernelGGL((boost_advance_kernel<ADD()>), grid, block, 0, (hipStream_t)stream, tree, node0, n_nodes, fmap,
                       (const u64*)bits, bits_stride / 8, bins, ld, n, node, margin);
    return check_launch("boost_advance_kernel");
  }, margin != nullptr);
}

extern "C" int sa_boost_apply(const sa_boost_node* tree, int32_t max_depth, const int32_t* fmap, const uint64_t* bits,
                              int64_t bits_stride, const uint8_t* bins, int64_t ld, const int64_t* rows,
                              int64_t n_rows, int64_t n, float* margin, float* p, void* stream) {
  if (n < 0 || n_rows < 0 || max_depth < 1 || max_depth > SA_BOOST_MAX_DEPTH || ld < n)
    return fail(SA_EINVAL, "sa_boost_apply: bad sizes");
  if (!tree || !fmap || !margin) return fail(SA_EINVAL, "sa_boost_apply: null pointer");
  if (bits && !bits_ok(bits, bits_stride, n)) return fail(SA_EINVAL, "sa_boost_apply: bad bitmaps");
  if (n_rows > (int64_t)0x7FFFFFFF * AP_THREADS) return fail(SA_EINVAL, "sa_boost_apply: too many rows");
  if (n_rows == 0) return SA_OK;
  hipLaunchKernelGGL(boost_apply_kernel, dim3((unsigned)((n_rows + AP_THREADS - 1) / AP_THREADS)), dim3(AP_THREADS), 0,
                     (hipStream_t)stream, tree, (int)max_depth, fmap, (const u64*)bits, bits_stride / 8, bins, ld, rows,
                     n_rows, n, margin, p);
  return check_launch("boost_apply_kernel");
}

namespace {
static_assert(offsetof(sa_boost_node, G) == 0 && offsetof(sa_boost_node, H) == 8, "the totals are one 16-byte pair");

// what pack and unpack share: the level, the pair table's sizes and the 16-byte alignment of the pair accesses
int exchange_args(const char* name, const void* hist, const void* tree, const int32_t* pairs, int32_t n_pair_bool,
                  int32_t n_pair_num, int32_t node0, int32_t n_nodes, int32_t n_features, const void* payload) {
  if (n_pair_bool < 0 || n_pair_num < 0 || n_features < 1 || !level_ok(node0, n_nodes) || n_pair_bool > n_features ||
      (int64_t)n_pair_bool + n_pair_num > (int64_t)n_features * BINS)
    return fail(SA_EINVAL, "%s: bad sizes", name);
  if (!hist || !tree || !payload || (n_pair_bool + n_pair_num > 0 && !pairs))
    return fail(SA_EINVAL, "%s: null pointer", name);
  if (((uintptr_t)hist | (uintptr_t)tree | (uintptr_t)payload) & 15u)
    return fail(SA_EINVAL, "%s: hist, tree and payload must be 16-byte aligned", name);
  return SA_OK;
}
}  // namespace

extern "C" int sa_boost_hist_pack(const int64_t* hist, const sa_boost_node* tree, const int32_t* pairs,
                                  int32_t n_pair_bool, int32_t n_pair_num, int32_t node0, int32_t n_nodes,
                                  int32_t n_features, int64_t* payload, void* stream) {
  if (int rc = exchange_args("sa_boost_hist_pack", hist, tree, pairs, n_pair_bool, n_pair_num, node0, n_nodes,
                             n_features, payload))
    return rc;
  const int head = node0 == 0;
  const int64_t items = head + (int64_t)n_nodes * (n_pair_bool + n_pair_num);
  if (items == 0) return SA_OK;
  hipLaunchKernelGGL(boost_hist_pack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const pair64*)hist, tree, pairs, n_pair_bool, n_pair_num, n_nodes, n_features, head,
                     (pair64*)payload);
  return check_launch("boost_hist_pack_kernel");
}

extern "C" int sa_boost_hist_unpack(const int64_t* payload, const int32_t* pairs, int32_t n_pair_bool,
                                    int32_t n_pair_num, const int32_t* bit_feat, int32_t n_bool, int32_t node0,
                                    int32_t n_nodes, int32_t n_features, int64_t* hist, sa_boost_node* tree,
                                    void* stream) {
  if (int rc = exchange_args("sa_boost_hist_unpack", hist, tree, pairs, n_pair_bool, n_pair_num, node0, n_nodes,
                             n_features, payload))
    return rc;
  if (n_bool < 0 || n_bool > n_pair_bool || (n_bool > 0 && !bit_feat))
    return fail(SA_EINVAL, "sa_boost_hist_unpack: bad bool feature list");
  const int head = node0 == 0;
  const int64_t items = head + (int64_t)n_nodes * (n_pair_bool + n_pair_num);
  if (items > 0) {
    hipLaunchKernelGGL(boost_hist_unpack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const pair64*)payload, pairs, n_pair_bool, n_pair_num, n_nodes, n_features,
                       head, (pair64*)hist, tree);
    if (int rc = check_launch("boost_hist_unpack_kernel")) return rc;
  }
  if (n_bool == 0) return SA_OK;
  // every listed bool feature's bin 0 from the global totals and the summed bin 1 (the fill of sa_boost_hist_bits)
  const int fill = n_bool * n_nodes;
  hipLaunchKernelGGL(boost_bits_fill_kernel, dim3((unsigned)((fill + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     bit_feat, n_bool, node0, n_nodes, n_features, hist, tree);
  return check_launch("boost_bits_fill_kernel");
}
