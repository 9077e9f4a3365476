// Binary classification scores on the device (the last cell of the reference's notebook 3 and
// VAEP.score: Brier score, log loss and AUROC of one label column against one probability column).
// Every score is a function of the multiset of (label, probability) rows only: the Brier and
// log-loss terms are quantised to the fixed-point limbs of sa_fixed.h and added as integers, and
// the AUROC is the integer U2 = sum over (positive, negative) pairs of 2 * [p_pos > p_neg] +
// [p_pos == p_neg], counted by looking every majority-class row up in the sorted keys of the
// minority class.  Integer sums are associative, so the results are the same bit for bit for any
// row order, chunking or batch split.  No float atomics, no inline assembly.
#include <float.h>

#include "sa_fixed.h"
#include "sa_internal.h"

using namespace sa;

namespace {
constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_ROWS = 4;                      // consecutive rows per thread (one 4-B label load)
constexpr int MT_TILE = MT_THREADS * MT_ROWS;   // rows a workgroup loads at a time
constexpr int MT_CHUNK = SA_METRIC_CHUNK_ROWS;  // contiguous rows per workgroup and loop step
constexpr int MT_SAMPLE = SA_AUC_LDS_SAMPLE;    // sorted keys the count kernel keeps in LDS
constexpr int MT_STAGE = 2 * MT_TILE;           // keys the compaction collects in LDS before a flush
static_assert(MT_CHUNK % MT_TILE == 0, "chunk shape");
typedef unsigned long long u64;

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

// The order key of a probability p >= 0: its own bit pattern, -0.0 mapped to +0.0.
__device__ inline uint32_t order_key(float p) {
  uint32_t b;
  __builtin_memcpy(&b, &p, sizeof(b));
  return b == 0x80000000u ? 0u : b;
}
__device__ inline uint64_t order_key(double p) {
  uint64_t b;
  __builtin_memcpy(&b, &p, sizeof(b));
  return b == 0x8000000000000000ull ? 0ull : b;
}

// Rows r .. r + MT_ROWS - 1 of the chunk that ends at `end`; rows past the end are never read:
// their label is 255 and the number of rows read is returned.
template <typename T>
__device__ inline int load_rows(const uint8_t* __restrict__ y, const T* __restrict__ p, int64_t r, int64_t end,
                                int vec, uint8_t yy[MT_ROWS], T pp[MT_ROWS]) {
  if (vec && r + MT_ROWS <= end) {  // r is a multiple of 4; y is 4-byte and p 16-byte aligned
    const uint32_t w = *reinterpret_cast<const uint32_t*>(y + r);
    yy[0] = (uint8_t)w, yy[1] = (uint8_t)(w >> 8), yy[2] = (uint8_t)(w >> 16), yy[3] = (uint8_t)(w >> 24);
    if constexpr (sizeof(T) == 4) {
      const float4 x = *reinterpret_cast<const float4*>(p + r);
      pp[0] = x.x, pp[1] = x.y, pp[2] = x.z, pp[3] = x.w;
    } else {
      const double2* q = reinterpret_cast<const double2*>(p + r);
      const double2 a = q[0], b = q[1];
      pp[0] = a.x, pp[1] = a.y, pp[2] = b.x, pp[3] = b.y;
    }
    return MT_ROWS;
  }
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < MT_ROWS; ++j) {
    const bool in = r + j < end;
    yy[j] = in ? y[r + j] : (uint8_t)255;
    pp[j] = in ? p[r + j] : (T)0;
    cnt += in;
  }
  return cnt;
}

__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += (u64)__shfl_down((long long)v, d, 64);
  return v;  // lane 0 holds the wave's total
}

// vals[0..N) of every thread -> one 64-bit integer atomic per value and workgroup.  Every thread
// of the workgroup calls it (one unconditional barrier).
template <int N>
__device__ inline void block_add(const u64 vals[N], u64* __restrict__ out) {
  __shared__ u64 part[MT_WAVES][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const u64 s = wave_sum(vals[i]);
    if (lane == 0) part[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < MT_WAVES; ++w) s += part[w][threadIdx.x];
    if (s) atomicAdd(out + threadIdx.x, s);
  }
}

// ------------------------------------------------------------------------------- the sums
// out: count[2] (rows, positives) then limbs[2][3] (Brier, log loss), contiguous or not.
template <typename T>
__global__ __launch_bounds__(MT_THREADS) void metric_sums_kernel(const uint8_t* __restrict__ y,
                                                                 const T* __restrict__ p, int64_t n, int vec,
                                                                 int64_t* __restrict__ count,
                                                                 int64_t* __restrict__ limbs,
                                                                 uint32_t* __restrict__ gerr) {
  const T eps = sizeof(T) == 4 ? (T)FLT_EPSILON : (T)DBL_EPSILON;
  const T hi = (T)1 - eps;
  u64 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // rows, positives, Brier limbs, log-loss limbs
  uint32_t err = 0;
  const int64_t n_chunks = (n + MT_CHUNK - 1) / MT_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * MT_CHUNK;
    const int64_t end = base + MT_CHUNK < n ? base + MT_CHUNK : n;
    for (int64_t row0 = base; row0 < end; row0 += MT_TILE) {
      uint8_t yy[MT_ROWS];
      T pp[MT_ROWS];
      const int cnt = load_rows<T>(y, p, row0 + (int64_t)threadIdx.x * MT_ROWS, end, vec, yy, pp);
#pragma unroll
      for (int j = 0; j < MT_ROWS; ++j) {
        if (j >= cnt) continue;
        const T v = pp[j];
        uint32_t e = 0;
        if (v != v) e |= SA_METRIC_ERR_NAN;
        else if (!(v >= (T)0 && v <= (T)1)) e |= SA_METRIC_ERR_RANGE;
        if (yy[j] > 1) e |= SA_METRIC_ERR_LABEL;
        if (e) {  // the row adds nothing
          err |= e;
          continue;
        }
        const bool pos = yy[j] == 1;
        // sklearn's log_loss: the complement in p's dtype, both clipped to [eps, 1 - eps]
        T q = pos ? v : (T)1 - v;
        q = q < eps ? eps : (q > hi ? hi : q);
        const double d = (double)v - (pos ? 1.0 : 0.0);
        const double term[2] = {d * d, -log((double)q)};
        const int E[2] = {SA_METRIC_BRIER_EXP, SA_METRIC_LOGLOSS_EXP};
        acc[0] += 1;
        acc[1] += pos;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          uint32_t m[3];
          int neg;
          sa_fx_quantize(term[t], E[t], m, &neg);  // 0 <= term < 2^E: always SA_FX_OK, never negative
#pragma unroll
          for (int i = 0; i < 3; ++i) acc[2 + t * 3 + i] += m[i];
        }
      }
    }
  }
  block_add<2>(acc, reinterpret_cast<u64*>(count));
  block_add<6>(acc + 2, reinterpret_cast<u64*>(limbs));
  if (err) atomicOr(gerr, err);
}

// ------------------------------------------------------------------------------- AUROC
// The keys of the rows whose label is `minority`, compacted in unspecified order.  A workgroup
// collects its keys in an LDS stage (the waves take ranges of it with one LDS atomic per wave and
// tile) and moves the stage to keys[] when another tile might not fit and when it is done: one
// global atomic on the cursor and coalesced stores per flush.  At most `cap` keys are written.
template <typename K>
__device__ inline void keys_flush(const K* stage, int* fill, u64* gbase, K* __restrict__ keys, int64_t cap,
                                  u64* __restrict__ cursor) {
  // every thread of the workgroup, after a barrier behind the last add to *fill
  const int f = *fill;
  if (threadIdx.x == 0 && f) *gbase = atomicAdd(cursor, (u64)f);
  __syncthreads();
  const int64_t g = (int64_t)*gbase;
  for (int i = threadIdx.x; i < f; i += MT_THREADS)
    if (g + i < cap) keys[g + i] = stage[i];
  __syncthreads();
  if (threadIdx.x == 0) *fill = 0;
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(MT_THREADS) void auc_keys_kernel(const uint8_t* __restrict__ y, const T* __restrict__ p,
                                                              int64_t n, int vec, int minority,
                                                              typename KeyOf<T>::type* __restrict__ keys,
                                                              int64_t cap, u64* __restrict__ cursor) {
  typedef typename KeyOf<T>::type K;
  __shared__ K stage[MT_STAGE];
  __shared__ u64 gbase;
  __shared__ int fill;
  if (threadIdx.x == 0) {
    fill = 0;
    gbase = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t n_chunks = (n + MT_CHUNK - 1) / MT_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * MT_CHUNK;
    const int64_t end = base + MT_CHUNK < n ? base + MT_CHUNK : n;
    for (int64_t row0 = base; row0 < end; row0 += MT_TILE) {  // before a tile: fill <= MT_STAGE - MT_TILE
      uint8_t yy[MT_ROWS];
      T pp[MT_ROWS];
      const int cnt = load_rows<T>(y, p, row0 + (int64_t)threadIdx.x * MT_ROWS, end, vec, yy, pp);
      int mine = 0;
#pragma unroll
      for (int j = 0; j < MT_ROWS; ++j) mine += (j < cnt && yy[j] == minority);
      int incl = mine;  // inclusive scan over the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      const int total = __shfl(incl, 63, 64);
      int start = 0;
      if (lane == 63 && total) start = atomicAdd(&fill, total);
      start = __shfl(start, 63, 64);
      int at = start + (incl - mine);
#pragma unroll
      for (int j = 0; j < MT_ROWS; ++j) {
        if (j < cnt && yy[j] == minority) {
          if (at < MT_STAGE) stage[at] = order_key(pp[j]);  // always: a tile adds at most MT_TILE keys
          ++at;
        }
      }
      // The wave whose add took the stage past the mark sees it in its own atomic's result, and
      // the barrier's reduction hands ONE decision to every thread: all of them flush or none.
      const bool past = total && start + total > MT_STAGE - MT_TILE;
      if (__syncthreads_or(past)) keys_flush<K>(stage, &fill, &gbase, keys, cap, cursor);
    }
  }
  keys_flush<K>(stage, &fill, &gbase, keys, cap, cursor);  // behind the last tile's barrier
}

// #keys < x (strict = false: <= x) among K[lo .. hi), K sorted ascending, by bisection
template <typename K>
__device__ inline int64_t bound(const K* __restrict__ keys, int64_t lo, int64_t hi, K x, bool upper) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const K k = keys[mid];
    if (upper ? k <= x : k < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The same over the LDS sample (int indices)
template <typename K>
__device__ inline int bound_lds(const K* s, int ns, K x, bool upper) {
  int lo = 0, hi = ns;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const K k = s[mid];
    if (upper ? k <= x : k < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// lower (upper = false) or upper bound of x in the m sorted keys: the sample keys[i * step],
// i < ns, decides the top levels in LDS; `step` keys of global memory hold the rest.
template <typename K>
__device__ inline int64_t sampled_bound(const K* __restrict__ keys, int64_t m, const K* s, int ns, int64_t step, K x,
                                        bool upper) {
  const int j = bound_lds(s, ns, x, upper);  // samples before x: keys[(j - 1) * step] is, keys[j * step] is not
  if (step == 1) return j;                   // the sample is the whole array
  if (j == 0) return 0;
  const int64_t lo = (int64_t)(j - 1) * step + 1;
  const int64_t hi = j < ns ? (int64_t)j * step : m;
  return bound(keys, lo, hi, x, upper);
}

template <typename T>
__global__ __launch_bounds__(MT_THREADS) void auc_count_kernel(const uint8_t* __restrict__ y, const T* __restrict__ p,
                                                               int64_t n, int vec,
                                                               const typename KeyOf<T>::type* __restrict__ keys,
                                                               int64_t m, int minority, u64* __restrict__ u2) {
  typedef typename KeyOf<T>::type K;
  __shared__ K sample[MT_SAMPLE];
  const int64_t step = (m + MT_SAMPLE - 1) / MT_SAMPLE;  // >= 1 (m >= 1)
  const int ns = (int)((m + step - 1) / step);           // <= MT_SAMPLE; (ns - 1) * step < m
  for (int i = threadIdx.x; i < ns; i += MT_THREADS) sample[i] = keys[(int64_t)i * step];
  __syncthreads();
  const int majority = 1 - minority;
  u64 acc = 0;
  const int64_t n_chunks = (n + MT_CHUNK - 1) / MT_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * MT_CHUNK;
    const int64_t end = base + MT_CHUNK < n ? base + MT_CHUNK : n;
    for (int64_t row0 = base; row0 < end; row0 += MT_TILE) {
      uint8_t yy[MT_ROWS];
      T pp[MT_ROWS];
      const int cnt = load_rows<T>(y, p, row0 + (int64_t)threadIdx.x * MT_ROWS, end, vec, yy, pp);
#pragma unroll
      for (int j = 0; j < MT_ROWS; ++j) {
        if (j >= cnt || yy[j] != majority) continue;
        const K x = order_key(pp[j]);
        const int64_t lower = sampled_bound<K>(keys, m, sample, ns, step, x, false);
        // without a tie the two bounds coincide: the second search runs for tied keys only
        int64_t upper = lower;
        if (lower < m && keys[lower] == x) upper = sampled_bound<K>(keys, m, sample, ns, step, x, true);
        const int64_t ties = upper - lower;
        // minority = positives: the positives above this negative count twice; minority =
        // negatives: the negatives below this positive do
        acc += (u64)(2 * (minority ? m - upper : lower) + ties);
      }
    }
  }
  block_add<1>(&acc, u2);
}

int check_rows(const char* who, const void* y, const void* p, int64_t n) {
  if (n < 0) return fail(SA_EINVAL, "%s: n < 0", who);
  if (n >= SA_FX_MAX_ROWS) return fail(SA_EINVAL, "%s: n must be below 2^30", who);
  if (!y || !p) return fail(SA_EINVAL, "%s: null pointer", who);
  return SA_OK;
}

// 4-byte labels and 16-byte probabilities per thread when both columns allow it
bool vec_ok(const void* y, const void* p) { return ((uintptr_t)y & 3u) == 0 && aligned16(p); }

dim3 rows_grid(int64_t n) {
  const int64_t n_chunks = (n + MT_CHUNK - 1) / MT_CHUNK;
  const int64_t resident = (int64_t)device_cus(current_device()) * SA_METRIC_WG_PER_CU;
  return dim3((unsigned)(n_chunks < resident ? n_chunks : resident));
}
}  // namespace

extern "C" int sa_metric_sums(const uint8_t* y, const void* p, int32_t f32, int64_t n, int64_t* count, int64_t* limbs,
                              uint32_t* err, void* stream) {
  if (int rc = check_rows("sa_metric_sums", y, p, n)) return rc;
  if (!count || !limbs || !err) return fail(SA_EINVAL, "sa_metric_sums: null pointer");
  if (n == 0) return SA_OK;
  const int vec = vec_ok(y, p);
  if (f32)
    hipLaunchKernelGGL(metric_sums_kernel<float>, rows_grid(n), dim3(MT_THREADS), 0, (hipStream_t)stream, y,
                       static_cast<const float*>(p), n, vec, count, limbs, err);
  else
    hipLaunchKernelGGL(metric_sums_kernel<double>, rows_grid(n), dim3(MT_THREADS), 0, (hipStream_t)stream, y,
                       static_cast<const double*>(p), n, vec, count, limbs, err);
  return check_launch("metric_sums_kernel");
}

extern "C" int sa_metric_finalize(const int64_t* count, const int64_t* limbs, double* out) {
  if (!count || !limbs || !out) return fail(SA_EINVAL, "sa_metric_finalize: null pointer");
  if (count[0] < 1) return fail(SA_EINVAL, "sa_metric_finalize: no rows");
  const double n = (double)count[0];  // exact: below 2^30
  out[0] = sa_fx_finalize(limbs[0], limbs[1], limbs[2], SA_METRIC_BRIER_EXP) / n;
  out[1] = sa_fx_finalize(limbs[3], limbs[4], limbs[5], SA_METRIC_LOGLOSS_EXP) / n;
  return SA_OK;
}

extern "C" int sa_auc_keys(const uint8_t* y, const void* p, int32_t f32, int64_t n, int32_t minority, void* keys,
                           int64_t capacity, uint64_t* cursor, void* stream) {
  if (int rc = check_rows("sa_auc_keys", y, p, n)) return rc;
  if (minority != 0 && minority != 1) return fail(SA_EINVAL, "sa_auc_keys: minority must be 0 or 1");
  if (capacity < 0) return fail(SA_EINVAL, "sa_auc_keys: capacity < 0");
  if (!keys || !cursor) return fail(SA_EINVAL, "sa_auc_keys: null pointer");
  if (n == 0) return SA_OK;
  const int vec = vec_ok(y, p);
  if (f32)
    hipLaunchKernelGGL(auc_keys_kernel<float>, rows_grid(n), dim3(MT_THREADS), 0, (hipStream_t)stream, y,
                       static_cast<const float*>(p), n, vec, (int)minority, static_cast<uint32_t*>(keys), capacity,
                       reinterpret_cast<u64*>(cursor));
  else
    hipLaunchKernelGGL(auc_keys_kernel<double>, rows_grid(n), dim3(MT_THREADS), 0, (hipStream_t)stream, y,
                       static_cast<const double*>(p), n, vec, (int)minority, static_cast<uint64_t*>(keys), capacity,
                       reinterpret_cast<u64*>(cursor));
  return check_launch("auc_keys_kernel");
}

extern "C" int sa_auc_count(const uint8_t* y, const void* p, int32_t f32, int64_t n, const void* sorted_keys,
                            int64_t m, int32_t minority, uint64_t* u2, void* stream) {
  if (int rc = check_rows("sa_auc_count", y, p, n)) return rc;
  if (minority != 0 && minority != 1) return fail(SA_EINVAL, "sa_auc_count: minority must be 0 or 1");
  if (m < 1 || m > n) return fail(SA_EINVAL, "sa_auc_count: m must be in [1, n]");
  if (!sorted_keys || !u2) return fail(SA_EINVAL, "sa_auc_count: null pointer");
  const int vec = vec_ok(y, p);
  if (f32)
    hipLaunchKernelGGL(auc_count_kernel<float>, rows_grid(n), dim3(MT_THREADS), 0, (hipStream_t)stream, y,
                       static_cast<const float*>(p), n, vec, static_cast<const uint32_t*>(sorted_keys), m,
                       (int)minority, reinterpret_cast<u64*>(u2));
  else
    hipLaunchKernelGGL(auc_count_kernel<double>, rows_grid(n), dim3(MT_THREADS), 0, (hipStream_t)stream, y,
                       static_cast<const double*>(p), n, vec, static_cast<const uint64_t*>(sorted_keys), m,
                       (int)minority, reinterpret_cast<u64*>(u2));
  return check_launch("auc_count_kernel");
}
