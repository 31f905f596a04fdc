// common.h -- shared internals of libgcg_spmm.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/gcg_spmm.h"
#include "layout.h"

namespace gcg {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;

// Record a printf-style message as this thread's gcg_last_error() and return `st`.
gcg_status fail(gcg_status st, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define GCG_HIP_CHECK(expr)                                                            \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return ::gcg::fail(GCG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));  \
  } while (0)

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  return static_cast<int>(std::min<int64_t>(std::max<int64_t>(g, 1), 4096));
}

namespace {  // small device helpers, one copy per translation unit

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Butterfly reductions over the wave (lane ^ 32, 16, ..., 1), float or double: the same order
// for every lane, every launch, and the result in every lane.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

}  // namespace
}  // namespace gcg
