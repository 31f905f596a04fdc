// segment_kernels.h -- what geo.hip, kmeans.hip and neighbours.hip share: the grid-stride
// helpers and the class pointer of a sorted label list (internal, not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gcg {
namespace {

__device__ __forceinline__ int64_t grid_start() {
  return static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
}
__device__ __forceinline__ int64_t grid_stride() {
  return static_cast<int64_t>(gridDim.x) * blockDim.x;
}

// ptr[c] = the first position of class c in the sorted labels (ptr[C] = N).
[[maybe_unused]] __global__ void class_ptr_kernel(int64_t N, int64_t C,
                                                  const int32_t* __restrict__ sorted,
                                                  int32_t* __restrict__ ptr) {
  for (int64_t p = grid_start(); p <= N; p += grid_stride()) {
    const int64_t prev = p == 0 ? -1 : sorted[p - 1];
    const int64_t cur = p == N ? C : sorted[p];
    for (int64_t c = prev + 1; c <= cur; ++c) ptr[c] = static_cast<int32_t>(p);
  }
}

}  // namespace
}  // namespace gcg
