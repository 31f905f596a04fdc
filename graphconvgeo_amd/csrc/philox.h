// philox.h -- Philox4x32-10 (Random123) and the dropout keep rule of include/gcg_spmm.h.
// Internal; host and device. One call yields the decisions of four consecutive logical
// columns (4 * (j >> 2) .. + 3) of one logical row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gcg {

struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                          uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(kM0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(kM1) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += kW0;
    k1 += kW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The parameters of one dropout stream, as the C-ABI takes them (step already read).
struct DropKey {
  uint32_t k0, k1, step, stream_id, threshold;
  float scale;
};

// The four words of logical row i, logical columns 4 * j4 .. 4 * j4 + 3.
__host__ __device__ __forceinline__ Philox4 drop_words(const DropKey& d, int64_t i, int64_t j4) {
  return philox4x32_10(static_cast<uint32_t>(i), static_cast<uint32_t>(j4), d.step, d.stream_id,
                       d.k0, d.k1);
}

// keep ? fl32(v * scale) : +0.0 for one element, given its word.
__host__ __device__ __forceinline__ float drop_apply(const DropKey& d, uint32_t word, float v) {
  return word >= d.threshold ? v * d.scale : 0.0f;
}

// One element (i, j): its own Philox call (scattered columns, scalar paths).
__host__ __device__ __forceinline__ float drop_element(const DropKey& d, int64_t i, int64_t j,
                                                       float v) {
  return drop_apply(d, drop_words(d, i, j >> 2).w[j & 3], v);
}

}  // namespace gcg
