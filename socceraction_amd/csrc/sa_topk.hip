// Exact, deterministic, filtered top-k of one device column (the last cell of the reference's
// notebook 4: the most valuable actions of a selection).  A row is eligible when its byte of
// `keep` is non-zero (keep == NULL: every row) and its value is not NaN.  The eligible rows are
// ranked by value -- descending for largest, -0.0 == +0.0 -- then by ascending row number, and the
// first k of that order are selected.  A radix select over order-preserving integer keys finds the
// k-th key T digit by digit (one histogram and one pick launch per digit, most significant first,
// chained on the stream through a small device state record); every row better than T is written
// through a cursor, and of the rows equal to T exactly the lowest-numbered ones that fill the k
// slots: per-chunk tie counts, their exclusive scan, and an ordered rank inside the workgroup.
// Every count is an integer, so the selection is a function of the (row, value, keep) set only:
// the same for any grid, chunking or run.  No float atomics, no inline assembly.
#include "sa_internal.h"

using namespace sa;

namespace {
constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_ROWS = 4;                     // consecutive rows per thread (one 4-B keep load)
constexpr int TK_TILE = TK_THREADS * TK_ROWS;  // rows a workgroup loads at a time
constexpr int TK_CHUNK = SA_TOP_CHUNK_ROWS;    // contiguous rows per workgroup and loop step
constexpr int TK_BITS = SA_TOP_DIGIT_BITS;
constexpr int TK_BINS = 1 << TK_BITS;
constexpr int TK_PICK_BINS = TK_BINS / TK_THREADS;  // bins per thread of the pick
// Wave-aggregated adds per row slot before the per-lane LDS atomics.  0: none -- measured the
// fastest on the MI355X (DESIGN.md "Filtered top-k"); -DSA_TOP_AGG_ROUNDS=N builds the variants
// scripts/top_rows_time.py prices against it.
#ifndef SA_TOP_AGG_ROUNDS
#define SA_TOP_AGG_ROUNDS 0
#endif
constexpr int TK_AGG_ROUNDS = SA_TOP_AGG_ROUNDS;
static_assert(TK_CHUNK % TK_TILE == 0, "chunk shape");
static_assert(TK_BINS % TK_THREADS == 0, "pick shape");
typedef unsigned long long u64;

// the words of the state record (SA_TOP_STATE_WORDS of them)
enum { ST_PREFIX = 0, ST_ABOVE = 1, ST_REM = 2, ST_ELIGIBLE = 3, ST_TIES = 4, ST_TAKE = 5, ST_M = 6, ST_CURSOR = 7 };

template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
  typedef uint32_t type;
};
template <>
struct KeyOf<double> {
  typedef uint64_t type;
};

// The order key: the unsigned integer of the value's width whose order is the numeric order
// (-0.0 folded onto +0.0, the sign-flip map), complemented for smallest-first so that the
// select always looks for the highest keys.
template <typename T>
__device__ inline typename KeyOf<T>::type order_key(T v, int largest) {
  typedef typename KeyOf<T>::type K;
  constexpr K SIGN = (K)1 << (sizeof(K) * 8 - 1);
  K b;
  __builtin_memcpy(&b, &v, sizeof(b));
  if (b == SIGN) b = 0;
  const K key = (b & SIGN) ? (K)~b : (K)(b | SIGN);
  return largest ? key : (K)~key;
}

// The digits, most significant first: digit `pass` is bits [lo, hi) of the key.
template <typename K>
struct Digit {
  int lo, hi;
  __host__ __device__ explicit Digit(int pass) {
    constexpr int W = sizeof(K) * 8;
    hi = W - pass * TK_BITS;
    lo = hi > TK_BITS ? hi - TK_BITS : 0;
  }
  // the bits above the digit agree (nothing is above digit 0)
  __device__ bool under(K key, K prefix) const {
    constexpr int W = sizeof(K) * 8;
    return hi >= W || (key >> hi) == (prefix >> hi);
  }
  __device__ int of(K key) const { return (int)((key >> lo) & (K)((1u << (hi - lo)) - 1u)); }
};

constexpr int passes_of(int f32) { return ((f32 ? 32 : 64) + TK_BITS - 1) / TK_BITS; }

// Rows r .. r + TK_ROWS - 1 of the chunk that ends at `end`; rows past the end are never read:
// their keep byte is 0.  keep == NULL keeps every row read.
template <typename T>
__device__ inline void load_rows(const T* __restrict__ v, const uint8_t* __restrict__ keep, int64_t r, int64_t end,
                                 int vec, T vv[TK_ROWS], uint8_t kk[TK_ROWS]) {
  if (vec && r + TK_ROWS <= end) {  // r is a multiple of 4; keep is 4-byte and v 16-byte aligned
    if (keep) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(keep + r);
      kk[0] = (uint8_t)w, kk[1] = (uint8_t)(w >> 8), kk[2] = (uint8_t)(w >> 16), kk[3] = (uint8_t)(w >> 24);
    } else {
      kk[0] = kk[1] = kk[2] = kk[3] = 1;
    }
    if constexpr (sizeof(T) == 4) {
      const float4 x = *reinterpret_cast<const float4*>(v + r);
      vv[0] = x.x, vv[1] = x.y, vv[2] = x.z, vv[3] = x.w;
    } else {
      const double2* q = reinterpret_cast<const double2*>(v + r);
      const double2 a = q[0], b = q[1];
      vv[0] = a.x, vv[1] = a.y, vv[2] = b.x, vv[3] = b.y;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < TK_ROWS; ++j) {
    const bool in = r + j < end;
    kk[j] = in ? (keep ? keep[r + j] : (uint8_t)1) : (uint8_t)0;
    vv[j] = in ? v[r + j] : (T)0;
  }
}

// ------------------------------------------------------------------------------- digit histogram
// hist[d] += the eligible rows under the state's prefix whose digit `pass` is d.  A workgroup
// counts in LDS and flushes its non-zero bins with one integer atomic each.  The first digit of a
// float64 is its sign and exponent: a rating column crowds into a handful of bins, where the
// lanes' LDS atomics meet on one address.  The aggregated form of that add is kept for
// TK_AGG_ROUNDS > 0: the lowest waiting lane names its bin, a ballot finds the lanes that hold the
// same one, and that lane adds the popcount; after TK_AGG_ROUNDS distinct bins the lanes still
// waiting (a spread-out digit) add on their own.  On 16M VAEP values the crowded first pass costs
// 0.042 ms with the plain atomics against 0.025 ms for a spread-out digit, and 0.044 / 0.101 ms
// with 2 / 8 aggregated rounds: the plain add is the default.
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void top_hist_kernel(const T* __restrict__ v,
                                                              const uint8_t* __restrict__ keep, int64_t n, int vec,
                                                              int largest, int pass, const u64* __restrict__ state,
                                                              uint32_t* __restrict__ hist) {
  typedef typename KeyOf<T>::type K;
  __shared__ uint32_t lh[TK_BINS];
  for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) lh[i] = 0;
  __syncthreads();
  const Digit<K> dg(pass);
  const K prefix = (K)state[ST_PREFIX];
  const int lane = threadIdx.x & 63;
  const int64_t n_chunks = (n + TK_CHUNK - 1) / TK_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * TK_CHUNK;
    const int64_t end = base + TK_CHUNK < n ? base + TK_CHUNK : n;
    for (int64_t row0 = base; row0 < end; row0 += TK_TILE) {
      T vv[TK_ROWS];
      uint8_t kk[TK_ROWS];
      load_rows<T>(v, keep, row0 + (int64_t)threadIdx.x * TK_ROWS, end, vec, vv, kk);
#pragma unroll
      for (int j = 0; j < TK_ROWS; ++j) {
        const K key = order_key<T>(vv[j], largest);
        bool active = kk[j] != 0 && vv[j] == vv[j] && dg.under(key, prefix);
        const int d = dg.of(key);
        SA_DGUARD(d >= 0 && d < TK_BINS, d, active = false);
        for (int round = 0; round < TK_AGG_ROUNDS; ++round) {
          const u64 waiting = __ballot(active);
          if (!waiting) break;
          const int leader = __ffsll((long long)waiting) - 1;
          const int bin = __shfl(d, leader, 64);
          const bool same = active && d == bin;
          const u64 group = __ballot(same);
          if (lane == leader) atomicAdd(&lh[bin], (uint32_t)__popcll(group));
          active = active && !same;
        }
        if (active) atomicAdd(&lh[d], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) {
    const uint32_t cnt = lh[i];
    if (cnt) atomicAdd(hist + i, cnt);
  }
}

// ------------------------------------------------------------------------------- pick
// One workgroup: scan the histogram from the top bin, find the bin that holds the rem-th best
// eligible row under the prefix, append its digit, move the rows of the bins above it to
// `above`, and clear the histogram.  Digit 0 sees every eligible row: with fewer than k of them
// the rank sought becomes their number (all are selected), with none the result is empty.
// The last digit leaves T in ST_PREFIX, the number of rows equal to T in ST_TIES, of those to
// take in ST_TAKE and m = above + take in ST_M.
__global__ __launch_bounds__(TK_THREADS) void top_pick_kernel(int bits, int64_t k, int pass, u64* __restrict__ state,
                                                              uint32_t* __restrict__ hist) {
  __shared__ u64 wave_total[TK_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int hi = bits - pass * TK_BITS;
  const int lo = hi > TK_BITS ? hi - TK_BITS : 0;
  const bool last = lo == 0;
  const u64 prefix = state[ST_PREFIX], above = state[ST_ABOVE];
  u64 rem = pass == 0 ? (u64)k : state[ST_REM];
  // thread t holds bins TK_BINS - 1 - (t * TK_PICK_BINS + i), i = 0 .. TK_PICK_BINS - 1: top down
  uint32_t cnt[TK_PICK_BINS];
  u64 sum = 0;
#pragma unroll
  for (int i = 0; i < TK_PICK_BINS; ++i) {
    const int b = TK_BINS - 1 - (t * TK_PICK_BINS + i);
    SA_DCHECK(b >= 0 && b < TK_BINS, b);
    cnt[i] = hist[b];
    hist[b] = 0;
    sum += cnt[i];
  }
  u64 incl = sum;  // inclusive scan over the wave, then over the waves
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 up = (u64)__shfl_up((long long)incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();  // also: every thread has read the state
  u64 total = 0;
#pragma unroll
  for (int w = 0; w < TK_WAVES; ++w) {
    if (w < wave) incl += wave_total[w];
    total += wave_total[w];
  }
  if (pass == 0) {
    if (total < rem) rem = total;  // fewer eligible rows than k: all of them
    if (t == 0) {
      state[ST_ELIGIBLE] = total;
      if (total == 0) state[ST_REM] = 0;  // ST_M stays 0: the empty result
    }
  }
  if (rem == 0) return;  // nothing eligible: the later digits find empty histograms
  u64 acc = incl - sum;  // rows in the bins above this thread's
  if (!(acc < rem && rem <= incl)) return;
  // the one thread whose bins hold the rem-th row
#pragma unroll
  for (int i = 0; i < TK_PICK_BINS; ++i) {
    if (acc + cnt[i] >= rem) {
      const u64 bin = (u64)(TK_BINS - 1 - (t * TK_PICK_BINS + i));
      const u64 take = rem - acc;  // 1 <= take <= cnt[i]
      state[ST_PREFIX] = prefix | (bin << lo);
      state[ST_ABOVE] = above + acc;
      state[ST_REM] = take;
      if (last) {
        state[ST_TIES] = cnt[i];
        state[ST_TAKE] = take;
        state[ST_M] = above + acc + take;
      }
      return;
    }
    acc += cnt[i];
  }
}

// ------------------------------------------------------------------------------- ties per chunk
// chunk_ties[c] = the eligible rows of chunk c whose key equals T.
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void top_tie_count_kernel(const T* __restrict__ v,
                                                                   const uint8_t* __restrict__ keep, int64_t n,
                                                                   int vec, int largest,
                                                                   const u64* __restrict__ state,
                                                                   int32_t* __restrict__ chunk_ties) {
  typedef typename KeyOf<T>::type K;
  __shared__ int part[TK_WAVES];
  const K thr = (K)state[ST_PREFIX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_chunks = (n + TK_CHUNK - 1) / TK_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * TK_CHUNK;
    const int64_t end = base + TK_CHUNK < n ? base + TK_CHUNK : n;
    int mine = 0;
    for (int64_t row0 = base; row0 < end; row0 += TK_TILE) {
      T vv[TK_ROWS];
      uint8_t kk[TK_ROWS];
      load_rows<T>(v, keep, row0 + (int64_t)threadIdx.x * TK_ROWS, end, vec, vv, kk);
#pragma unroll
      for (int j = 0; j < TK_ROWS; ++j)
        mine += kk[j] != 0 && vv[j] == vv[j] && order_key<T>(vv[j], largest) == thr;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if (lane == 0) part[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < TK_WAVES; ++w) s += part[w];
      SA_DCHECK(c >= 0 && c < n_chunks, c);
      chunk_ties[c] = s;
    }
    __syncthreads();  // part[] is free for the next chunk
  }
}

// ------------------------------------------------------------------------------- collect
// rows[0 .. above): the eligible rows whose key is higher than T, in cursor order;
// rows[above + q], q < take: the q-th lowest-numbered eligible row whose key equals T.  The rank q
// of a tied row = chunk_base[its chunk] (the ties of the chunks before it) + the ties before it
// in the chunk, from the running count of the tiles done, a scan over the waves and one over the lanes.
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void top_collect_kernel(const T* __restrict__ v,
                                                                 const uint8_t* __restrict__ keep, int64_t n, int vec,
                                                                 int largest, int64_t k, u64* __restrict__ state,
                                                                 const int64_t* __restrict__ chunk_base,
                                                                 int64_t* __restrict__ rows) {
  typedef typename KeyOf<T>::type K;
  __shared__ int wave_ties[TK_WAVES];
  const K thr = (K)state[ST_PREFIX];
  const int64_t above = (int64_t)state[ST_ABOVE], take = (int64_t)state[ST_TAKE];
  if (state[ST_M] == 0) return;  // nothing eligible
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_chunks = (n + TK_CHUNK - 1) / TK_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * TK_CHUNK;
    const int64_t end = base + TK_CHUNK < n ? base + TK_CHUNK : n;
    int64_t before = chunk_base[c];       // ties in front of the tile being read
    const bool rank_ties = before < take;  // one decision per workgroup and chunk
    for (int64_t row0 = base; row0 < end; row0 += TK_TILE) {
      T vv[TK_ROWS];
      uint8_t kk[TK_ROWS];
      const int64_t r = row0 + (int64_t)threadIdx.x * TK_ROWS;
      load_rows<T>(v, keep, r, end, vec, vv, kk);
      bool tie[TK_ROWS];
      int mine = 0;
#pragma unroll
      for (int j = 0; j < TK_ROWS; ++j) {
        const K key = order_key<T>(vv[j], largest);
        const bool ok = kk[j] != 0 && vv[j] == vv[j];
        tie[j] = ok && key == thr;
        mine += tie[j];
        if (ok && key > thr) {
          const int64_t slot = (int64_t)atomicAdd(state + ST_CURSOR, 1ull);
          SA_DCHECK(slot >= 0 && slot < above && slot < k, slot);
          if (slot < above && slot < k) rows[slot] = r + j;
        }
      }
      if (!rank_ties) continue;
      int incl = mine;  // inclusive scan over the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      if (lane == 63) wave_ties[wave] = incl;
      __syncthreads();
      int64_t rank = before + (incl - mine);
      int tile_ties = 0;
#pragma unroll
      for (int w = 0; w < TK_WAVES; ++w) {
        if (w < wave) rank += wave_ties[w];
        tile_ties += wave_ties[w];
      }
#pragma unroll
      for (int j = 0; j < TK_ROWS; ++j) {
        if (!tie[j]) continue;
        if (rank < take) {
          const int64_t slot = above + rank;
          SA_DCHECK(slot >= 0 && slot < k, slot);
          if (slot < k) rows[slot] = r + j;
        }
        ++rank;
      }
      before += tile_ties;
      __syncthreads();  // wave_ties[] is free for the next tile
    }
  }
}

int check_column(const char* who, const void* values, int64_t n) {
  if (n < 0) return fail(SA_EINVAL, "%s: n < 0", who);
  if (n > INT32_MAX) return fail(SA_EINVAL, "%s: n must be below 2^31", who);
  if (!values && n > 0) return fail(SA_EINVAL, "%s: null pointer", who);
  return SA_OK;
}

int check_k(const char* who, int64_t k) {
  if (k < 1 || k > SA_TOP_MAX_K) return fail(SA_EINVAL, "%s: k must be in [1, %d]", who, SA_TOP_MAX_K);
  return SA_OK;
}

// 16-byte values and 4-byte keep bytes per thread when both columns allow it
bool vec_ok(const void* values, const void* keep) { return aligned16(values) && ((uintptr_t)keep & 3u) == 0; }

dim3 rows_grid(int64_t n) {
  const int64_t n_chunks = (n + TK_CHUNK - 1) / TK_CHUNK;
  const int64_t resident = (int64_t)device_cus(current_device()) * SA_TOP_WG_PER_CU;
  return dim3((unsigned)(n_chunks < resident ? n_chunks : resident));
}
}  // namespace

extern "C" int sa_top_passes(int32_t f32) { return passes_of(f32); }

extern "C" int sa_top_hist(const void* values, int32_t f32, const uint8_t* keep, int64_t n, int32_t largest,
                           int32_t pass, const uint64_t* state, uint32_t* hist, void* stream) {
  if (int rc = check_column("sa_top_hist", values, n)) return rc;
  if (pass < 0 || pass >= passes_of(f32)) return fail(SA_EINVAL, "sa_top_hist: pass out of range");
  if (!state || !hist) return fail(SA_EINVAL, "sa_top_hist: null pointer");
  if (n == 0) return SA_OK;
  const int vec = vec_ok(values, keep);
  const u64* st = reinterpret_cast<const u64*>(state);
  if (f32)
    hipLaunchKernelGGL(top_hist_kernel<float>, rows_grid(n), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       static_cast<const float*>(values), keep, n, vec, (int)(largest != 0), (int)pass, st, hist);
  else
    hipLaunchKernelGGL(top_hist_kernel<double>, rows_grid(n), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       static_cast<const double*>(values), keep, n, vec, (int)(largest != 0), (int)pass, st, hist);
  return check_launch("top_hist_kernel");
}

extern "C" int sa_top_pick(int32_t f32, int64_t k, int32_t pass, uint64_t* state, uint32_t* hist, void* stream) {
  if (int rc = check_k("sa_top_pick", k)) return rc;
  if (pass < 0 || pass >= passes_of(f32)) return fail(SA_EINVAL, "sa_top_pick: pass out of range");
  if (!state || !hist) return fail(SA_EINVAL, "sa_top_pick: null pointer");
  hipLaunchKernelGGL(top_pick_kernel, dim3(1), dim3(TK_THREADS), 0, (hipStream_t)stream, f32 ? 32 : 64, k, (int)pass,
                     reinterpret_cast<u64*>(state), hist);
  return check_launch("top_pick_kernel");
}

extern "C" int sa_top_tie_count(const void* values, int32_t f32, const uint8_t* keep, int64_t n, int32_t largest,
                                const uint64_t* state, int32_t* chunk_ties, void* stream) {
  if (int rc = check_column("sa_top_tie_count", values, n)) return rc;
  if (!state || !chunk_ties) return fail(SA_EINVAL, "sa_top_tie_count: null pointer");
  if (n == 0) return SA_OK;
  const int vec = vec_ok(values, keep);
  const u64* st = reinterpret_cast<const u64*>(state);
  if (f32)
    hipLaunchKernelGGL(top_tie_count_kernel<float>, rows_grid(n), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       static_cast<const float*>(values), keep, n, vec, (int)(largest != 0), st, chunk_ties);
  else
    hipLaunchKernelGGL(top_tie_count_kernel<double>, rows_grid(n), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       static_cast<const double*>(values), keep, n, vec, (int)(largest != 0), st, chunk_ties);
  return check_launch("top_tie_count_kernel");
}

extern "C" int sa_top_collect(const void* values, int32_t f32, const uint8_t* keep, int64_t n, int32_t largest,
                              int64_t k, uint64_t* state, const int64_t* chunk_base, int64_t* rows, void* stream) {
  if (int rc = check_column("sa_top_collect", values, n)) return rc;
  if (int rc = check_k("sa_top_collect", k)) return rc;
  if (!state || !chunk_base || !rows) return fail(SA_EINVAL, "sa_top_collect: null pointer");
  if (n == 0) return SA_OK;
  const int vec = vec_ok(values, keep);
  u64* st = reinterpret_cast<u64*>(state);
  if (f32)
    hipLaunchKernelGGL(top_collect_kernel<float>, rows_grid(n), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       static_cast<const float*>(values), keep, n, vec, (int)(largest != 0), k, st, chunk_base, rows);
  else
    hipLaunchKernelGGL(top_collect_kernel<double>, rows_grid(n), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       static_cast<const double*>(values), keep, n, vec, (int)(largest != 0), k, st, chunk_base, rows);
  return check_launch("top_collect_kernel");
}
