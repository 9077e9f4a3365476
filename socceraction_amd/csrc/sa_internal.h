// Host-side helpers shared by the C-ABI entry points (error reporting, launch checks, scratch).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/socceraction_amd.h"
#include "sa_debug.h"

namespace sa {
// Records a printf-style message in the thread-local error slot and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// Maps a pending launch error (hipGetLastError) to SA_EHIP.
int check_launch(const char* what);
int check_hip(hipError_t e, const char* what);
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// Compute units and LDS bytes per workgroup of device `dev`, queried once per device (256 /
// 64 KiB when the query fails).
int device_cus(int dev);
int device_lds_max(int dev);
// The current device (0 when the query fails).
int current_device();

// Runtime flags -> template arguments: calls the generic lambda `f` with one std::true_type /
// std::false_type per flag, in the flags' order, and returns its int.  In the lambda a flag is a
// constant (`kernel<A(), E()>`), so a launch's argument list is written once; a combination with
// no kernel is excluded there by `if constexpr`, which also keeps it from being instantiated.
template <class F, class... Rest>
int with_flags(F&& f, bool flag, Rest... rest) {
  if constexpr (sizeof...(rest) == 0) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
  } else {
    return flag ? with_flags([&](auto... r) { return f(std::true_type{}, r...); }, rest...)
                : with_flags([&](auto... r) { return f(std::false_type{}, r...); }, rest...);
  }
}

// Library-owned device scratch (the cached per-device arena of sa_api.hip).  acquire returns a
// slot of at least `bytes` that no other call is using; release hands it back once the work
// enqueued on `st` is done with it (stream-ordered reuse).
struct Scratch {
  void* ptr = nullptr;
  int slot = -1;
};
int scratch_acquire(size_t bytes, hipStream_t st, Scratch* out);
void scratch_release(const Scratch& s, hipStream_t st);
// A slot held for a scope, released against the stream it was acquired on.  The release records
// an event there, so the guard outlives the last enqueue that uses the memory.
struct ScratchGuard {
  Scratch s;
  hipStream_t st = nullptr;
  ScratchGuard() = default;
  ScratchGuard(const ScratchGuard&) = delete;
  ScratchGuard& operator=(const ScratchGuard&) = delete;
  ~ScratchGuard() { scratch_release(s, st); }
  int acquire(size_t bytes, hipStream_t stream) { return scratch_acquire(bytes, st = stream, &s); }
  template <class T>
  T* at(size_t byte_offset = 0) const { return reinterpret_cast<T*>(static_cast<char*>(s.ptr) + byte_offset); }
};

// Argument checks shared by the xT entry points.  A grid: l, w >= 1 and l * w (in 64 bits) at
// most max_cells; 46340: the C x C transition counts are indexed in int32.
inline int check_grid(int l, int w, int64_t max_cells = 46340) {
  if (l >= 1 && w >= 1 && (int64_t)l * w <= max_cells) return SA_OK;
  return fail(SA_EINVAL, "bad l or w (l, w >= 1 and l * w <= %lld)", (long long)max_cells);
}
inline int check_xy_columns(const sa_frame& F) {  // what the xT passes read of frames[0]
  return F.type_id && F.result_id && F.c0 && F.c1 && F.c2 && F.c3 ? SA_OK : fail(SA_EINVAL, "null input column");
}
// The kernels' vector loads: the coordinate columns (and `out`) 16-byte aligned, the ids even.
inline bool coords_vec_ok(const sa_frame& F, const void* out = nullptr) {
  return aligned16(F.c0) && aligned16(F.c1) && aligned16(F.c2) && aligned16(F.c3) && aligned16(out) &&
         ((uintptr_t)F.type_id & 1u) == 0 && ((uintptr_t)F.result_id & 1u) == 0;
}

// The host loop of a solve that launches once per iteration: enqueue(it) launches iteration it,
// which leaves dflags[it] != 0 when some cell moved by more than eps.  The flags come back every
// 8 iterations (one copy, one synchronise); *n_iter = the first iteration, counted from 1, whose
// flag is 0, or -1 when max_iter comes first.
template <class Enqueue>
int iterate_to_convergence(int max_iter, const int32_t* dflags, hipStream_t st, int* n_iter, Enqueue enqueue) {
  int32_t hflags[8];
  *n_iter = -1;
  for (int it0 = 0; it0 < max_iter; it0 += 8) {
    const int nb = max_iter - it0 < 8 ? max_iter - it0 : 8;
    for (int k = 0; k < nb; ++k)
      if (int rc = enqueue(it0 + k)) return rc;
    if (int rc = check_hip(hipMemcpyAsync(hflags, dflags + it0, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st),
                           "copy flags"))
      return rc;
    if (int rc = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize")) return rc;
    for (int k = 0; k < nb && *n_iter < 0; ++k)
      if (hflags[k] == 0) *n_iter = it0 + k + 1;
    if (*n_iter > 0) break;
  }
  return SA_OK;
}

// Large-grid xT (sa_xt_large.hip).  xt_band_ok: the band-owned count holds a grid of C cells;
// xt_count_bands: that count of one batch, added into the caller's counts.  xt_compact_*: the
// compact form of count rows and one value iteration over it (C <= 9472).
bool xt_band_ok(int C);
int xt_count_bands(const sa_actions& A, const uint32_t* cells, int64_t n, int l, int w, int64_t* shot,
                   int64_t* goal, int64_t* move, int32_t* trans, int32_t* err, uint32_t* codes, hipStream_t st);
bool xt_compact_ok(int C);
size_t xt_compact_bytes(int C, int nrows);
int xt_compact_build(const int32_t* cnt_rows, int C, int nrows, uint32_t* ell, int32_t* row_len, hipStream_t st);
int xt_compact_iterate(const uint32_t* ell, const int32_t* row_len, const int32_t* cnt_rows, const int64_t* move,
                       const double* gs, const double* pmove, int C, int rb, int nrows, const double* x, double eps,
                       double* xo, const int32_t* flag_prev, int32_t* flag_out, hipStream_t st);
// The whole value iteration over the compact form of every row (sa_xt_solve_compact):
// reordered sums under an error bound, or the reference's order (SA_XT_SOLVE_EXACT, or when the
// bound cannot decide); *path = SA_XT_PATH_*.  xt_out (optional): the reordered path also
// writes the final iterate there (the surface).  Synchronises the stream.
// hook (optional): work enqueued right after the one-launch reordered solve, before the host
// waits for its status (sa_xt_fit_rate_interp_codes: the rate of the surface the solve writes);
// hook->ran says whether it was.
struct SolveHook {
  int (*fn)(void* ctx);
  void* ctx;
  bool ran;
};
int xt_compact_solve(const uint32_t* ell, const int32_t* row_len, const int32_t* cnt_rows, const int64_t* move,
                     const double* gs, const double* pmove, int C, double eps, int max_iter, int flags,
                     double* heat, int* n_iter, int* path, hipStream_t st, double* xt_out = nullptr,
                     SolveHook* hook = nullptr);
}  // namespace sa
