// Grouped sums that do not depend on summation order (the player / team rating tables of the
// reference's notebooks: A.groupby(key)[values].sum()).  Every value is quantised to the
// fixed-point limbs of sa_fixed.h and the limbs are added as integers -- in an LDS table per
// workgroup, then with 64-bit integer global atomics -- so the table is the same bit for bit for
// any order, chunking, batch split or device count.  group_finalize_kernel rounds each total to
// f64 once.  No float atomics, no inline assembly.
#include "sa_fixed.h"
#include "sa_internal.h"

using namespace sa;

namespace {
constexpr int GS_THREADS = 256;
constexpr int GS_ROWS = 4;                       // consecutive rows per thread (one 16-B key load)
constexpr int GS_TILE = GS_THREADS * GS_ROWS;    // rows a workgroup loads at a time
constexpr int GS_CHUNK = SA_GROUP_CHUNK_ROWS;    // contiguous rows per chunk (a multiple of GS_TILE)
constexpr int GS_SLOTS = SA_GROUP_LDS_SLOTS;     // LDS table slots (a power of two)
constexpr int GS_EMPTY = -1;
static_assert(GS_CHUNK % GS_TILE == 0 && (GS_SLOTS & (GS_SLOTS - 1)) == 0, "chunk / table shape");
typedef unsigned long long u64;

struct GroupCols {
  const void* col[SA_GROUP_MAX_COLS];
  int32_t E[SA_GROUP_MAX_COLS];
};

// LDS: [GS_SLOTS][3V] limb sums (int64), [GS_SLOTS] row counts, [GS_SLOTS] keys, the occupancy
constexpr size_t gs_lds_bytes(int V) { return (size_t)GS_SLOTS * (3 * V * 8 + 4 + 4) + 16; }

__device__ inline unsigned gs_hash(int key) { return ((unsigned)key * SA_GROUP_HASH_MUL) >> (32 - __builtin_ctz(GS_SLOTS)); }

// The slot of `key` (open addressing, linear probing), claiming an empty one if the key has
// none; -1 when every slot holds another key.
__device__ inline int gs_find_slot(int* keys, int* occ, int key) {
  const unsigned h = gs_hash(key);
  for (int p = 0; p < GS_SLOTS; ++p) {
    const int s = (int)((h + p) & (GS_SLOTS - 1));
    const int cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == key) return s;
    if (cur == GS_EMPTY) {
      const int old = atomicCAS(&keys[s], GS_EMPTY, key);
      if (old == GS_EMPTY) {
        atomicAdd(occ, 1);
        return s;
      }
      if (old == key) return s;
    }
  }
  return -1;
}

// Add the table to the global tables (one 64-bit integer atomic per non-zero word) and clear it.
// Every thread of the workgroup calls it.
template <int V>
__device__ inline void gs_flush(u64* limbs, int* cnt, int* keys, int* occ, bool ident, int G,
                                int64_t* __restrict__ glimbs, int64_t* __restrict__ gcount) {
  constexpr int W = 3 * V;
  __syncthreads();
  const int used = ident ? G : GS_SLOTS;
  for (int i = threadIdx.x; i < used * (W + 1); i += GS_THREADS) {
    const int slot = i / (W + 1), w = i - slot * (W + 1);
    const int key = ident ? slot : keys[slot];
    if (key < 0) continue;
    SA_DGUARD(key < G, key, continue);
    if (w < W) {
      const u64 x = limbs[slot * W + w];
      if (x) {
        atomicAdd(reinterpret_cast<u64*>(glimbs) + (int64_t)key * W + w, x);
        limbs[slot * W + w] = 0;
      }
    } else {
      const int c = cnt[slot];
      if (c) {
        atomicAdd(reinterpret_cast<u64*>(gcount) + key, (u64)c);
        cnt[slot] = 0;
      }
    }
  }
  __syncthreads();
  if (!ident) {
    for (int i = threadIdx.x; i < GS_SLOTS; i += GS_THREADS) keys[i] = GS_EMPTY;
    if (threadIdx.x == 0) *occ = 0;
  }
  __syncthreads();
}

template <int V, typename T>
__global__ __launch_bounds__(GS_THREADS) void group_sums_kernel(const int32_t* __restrict__ keyp, GroupCols C,
                                                                int64_t n, int G, int vec,
                                                                int64_t* __restrict__ glimbs,
                                                                int64_t* __restrict__ gcount,
                                                                uint32_t* __restrict__ gerr) {
  constexpr int W = 3 * V;
  extern __shared__ u64 gs_lds[];
  u64* limbs = gs_lds;
  int* cnt = reinterpret_cast<int*>(limbs + GS_SLOTS * W);
  int* keys = cnt + GS_SLOTS;
  int* occ = keys + GS_SLOTS;
  const bool ident = G <= GS_SLOTS;  // the slot is the code itself
  const int tid = threadIdx.x;
  for (int i = tid; i < GS_SLOTS * W; i += GS_THREADS) limbs[i] = 0;
  for (int i = tid; i < GS_SLOTS; i += GS_THREADS) {
    cnt[i] = 0;
    keys[i] = GS_EMPTY;
  }
  if (tid == 0) *occ = 0;
  __syncthreads();

  uint32_t err = 0;
  const int64_t n_chunks = (n + GS_CHUNK - 1) / GS_CHUNK;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * GS_CHUNK;
    const int64_t end = base + GS_CHUNK < n ? base + GS_CHUNK : n;
    for (int64_t row0 = base; row0 < end; row0 += GS_TILE) {
      const int64_t r = row0 + (int64_t)tid * GS_ROWS;
      int key[GS_ROWS];
      double val[V][GS_ROWS];
      if (vec && r + GS_ROWS <= end) {  // 16-B loads: r is a multiple of 4 and the columns are aligned
        const int4 k = *reinterpret_cast<const int4*>(keyp + r);
        key[0] = k.x, key[1] = k.y, key[2] = k.z, key[3] = k.w;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if constexpr (sizeof(T) == 4) {
            const float4 x = *reinterpret_cast<const float4*>(static_cast<const float*>(C.col[v]) + r);
            val[v][0] = x.x, val[v][1] = x.y, val[v][2] = x.z, val[v][3] = x.w;  // widened exactly
          } else {
            const double2* p = reinterpret_cast<const double2*>(static_cast<const double*>(C.col[v]) + r);
            const double2 a = p[0], b = p[1];
            val[v][0] = a.x, val[v][1] = a.y, val[v][2] = b.x, val[v][3] = b.y;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < GS_ROWS; ++j) {
          const bool in = r + j < end;
          key[j] = in ? keyp[r + j] : GS_EMPTY;
#pragma unroll
          for (int v = 0; v < V; ++v) val[v][j] = in ? (double)static_cast<const T*>(C.col[v])[r + j] : 0.0;
        }
      }
      // rows that add: key -1 is skipped; a key outside [0, G) or a value that is infinite or
      // out of its column's range flags the error and drops the whole row
      unsigned pend = 0;
#pragma unroll
      for (int j = 0; j < GS_ROWS; ++j) {
        if (key[j] == GS_EMPTY) continue;
        if ((unsigned)key[j] >= (unsigned)G) {
          err |= SA_GROUP_ERR_KEY;
          continue;
        }
        int bad = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) bad |= sa_fx_classify(val[v][j], C.E[v]);
        bad &= SA_FX_NONFINITE | SA_FX_RANGE;
        if (bad) {
          err |= bad;  // SA_GROUP_ERR_NONFINITE / SA_GROUP_ERR_RANGE are the same bits
          continue;
        }
        pend |= 1u << j;
      }
      for (;;) {
#pragma unroll
        for (int j = 0; j < GS_ROWS; ++j) {
          if (!(pend >> j & 1)) continue;
          const int slot = ident ? key[j] : gs_find_slot(keys, occ, key[j]);
          if (slot < 0) continue;  // the table is full: after the flush below
          SA_DGUARD(slot < GS_SLOTS, slot, { pend &= ~(1u << j); continue; });
          u64* L = limbs + slot * W;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            uint32_t m[3];
            int neg;
            if (sa_fx_quantize(val[v][j], C.E[v], m, &neg) != SA_FX_OK) continue;  // NaN adds nothing
#pragma unroll
            for (int i = 0; i < 3; ++i)
              if (m[i]) atomicAdd(L + v * 3 + i, neg ? (u64)(-(int64_t)m[i]) : (u64)m[i]);
          }
          atomicAdd(cnt + slot, 1);
          pend &= ~(1u << j);
        }
        // Flush when a row is still waiting for a slot or more than half the slots are taken.
        // Each thread reads the occupancy BEFORE the barrier, after its own inserts (the thread
        // whose claim crossed the half sees it: LDS operations of a wave run in order), and the
        // barrier's reduction hands ONE decision to every thread, so all of them take the
        // barriers of the flush or none does, whatever the waves' timing.  After a flush the
        // table is empty: the next pass either places the waiting rows or finds nothing to do
        // and leaves.
        const bool full =
            !ident && __hip_atomic_load(occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > GS_SLOTS / 2;
        if (!__syncthreads_or(pend != 0 || full)) break;
        gs_flush<V>(limbs, cnt, keys, occ, ident, G, glimbs, gcount);
      }
    }
    gs_flush<V>(limbs, cnt, keys, occ, ident, G, glimbs, gcount);  // the chunk ends
  }
  if (err) atomicOr(gerr, err);
}

// one thread per (group, column): the three limb sums -> f64 out[v * G + g]
__global__ __launch_bounds__(256) void group_finalize_kernel(const int64_t* __restrict__ limbs, int G, int V,
                                                             GroupCols C, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)G * V) return;
  const int g = (int)(i / V), v = (int)(i - (int64_t)g * V);
  const int64_t* s = limbs + i * 3;
  out[(int64_t)v * G + g] = sa_fx_finalize(s[0], s[1], s[2], C.E[v]);
}

static_assert(SA_GROUP_ERR_NONFINITE == SA_FX_NONFINITE && SA_GROUP_ERR_RANGE == SA_FX_RANGE, "error bits");

int check_exps(const char* who, const int32_t* scale_exp, int n_cols, GroupCols* C) {
  for (int v = 0; v < n_cols; ++v) {
    if (scale_exp[v] < SA_FX_EXP_MIN || scale_exp[v] > SA_FX_EXP_MAX)
      return fail(SA_EINVAL, "%s: scale_exp[%d] = %d is outside [%d, %d]", who, v, scale_exp[v], SA_FX_EXP_MIN,
                  SA_FX_EXP_MAX);
    C->E[v] = scale_exp[v];
  }
  return SA_OK;
}

template <typename T>
void launch_sums(int V, dim3 grid, hipStream_t st, const int32_t* key, const GroupCols& C, int64_t n, int G, int vec,
                 int64_t* limbs, int64_t* count, uint32_t* err) {
#define GS_CASE(NV)                                                                                             \
  case NV:                                                                                                      \
    hipLaunchKernelGGL((group_sums_kernel<NV, T>), grid, dim3(GS_THREADS), gs_lds_bytes(NV), st, key, C, n, G, \
                       vec, limbs, count, err);                                                                 \
    break;
  switch (V) {
    GS_CASE(1) GS_CASE(2) GS_CASE(3) GS_CASE(4) GS_CASE(5) GS_CASE(6) GS_CASE(7) GS_CASE(8)
  }
#undef GS_CASE
}
}  // namespace

extern "C" int sa_group_sums(const int32_t* key, const void* const* cols, int32_t n_cols, int32_t f32, int64_t n,
                             int32_t n_groups, const int32_t* scale_exp, int64_t* limbs, int64_t* count,
                             uint32_t* err, void* stream) {
  if (n_cols < 1 || n_cols > SA_GROUP_MAX_COLS)
    return fail(SA_EINVAL, "sa_group_sums: n_cols must be 1..%d", SA_GROUP_MAX_COLS);
  if (n < 0) return fail(SA_EINVAL, "sa_group_sums: n < 0");
  if (n_groups < 1) return fail(SA_EINVAL, "sa_group_sums: n_groups < 1");
  if (!key || !cols || !scale_exp || !limbs || !count || !err) return fail(SA_EINVAL, "sa_group_sums: null pointer");
  GroupCols C = {};
  bool vec = aligned16(key);
  for (int v = 0; v < n_cols; ++v) {
    if (!cols[v]) return fail(SA_EINVAL, "sa_group_sums: null column %d", v);
    C.col[v] = cols[v];
    vec = vec && aligned16(cols[v]);
  }
  if (int rc = check_exps("sa_group_sums", scale_exp, n_cols, &C)) return rc;
  if (n == 0) return SA_OK;
  const int64_t n_chunks = (n + GS_CHUNK - 1) / GS_CHUNK;
  const int64_t resident = (int64_t)device_cus(current_device()) * SA_GROUP_WG_PER_CU;
  const dim3 grid((unsigned)(n_chunks < resident ? n_chunks : resident));
  if (f32)
    launch_sums<float>(n_cols, grid, (hipStream_t)stream, key, C, n, n_groups, (int)vec, limbs, count, err);
  else
    launch_sums<double>(n_cols, grid, (hipStream_t)stream, key, C, n, n_groups, (int)vec, limbs, count, err);
  return check_launch("group_sums_kernel");
}

extern "C" int sa_group_finalize(const int64_t* limbs, int32_t n_groups, int32_t n_cols, const int32_t* scale_exp,
                                 double* out, void* stream) {
  if (n_cols < 1 || n_cols > SA_GROUP_MAX_COLS)
    return fail(SA_EINVAL, "sa_group_finalize: n_cols must be 1..%d", SA_GROUP_MAX_COLS);
  if (n_groups < 1) return fail(SA_EINVAL, "sa_group_finalize: n_groups < 1");
  if (!limbs || !scale_exp || !out) return fail(SA_EINVAL, "sa_group_finalize: null pointer");
  GroupCols C = {};
  if (int rc = check_exps("sa_group_finalize", scale_exp, n_cols, &C)) return rc;
  const int64_t items = (int64_t)n_groups * n_cols;
  hipLaunchKernelGGL(group_finalize_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, limbs, n_groups, n_cols, C, out);
  return check_launch("group_finalize_kernel");
}
