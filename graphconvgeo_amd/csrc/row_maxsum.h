// row_maxsum.h -- the (max, sum of exp(x - max)) fold of one wide float32 row by one workgroup of
// 256 threads: the first pass of softmax_xent_csr_kernel (softmax_csr.hip) and the whole of
// row_lse_kernel (vocab_stats.hip). Stated once, so both give a row the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

namespace gcg {
namespace {

// A running (max, sum of exp(x - max)) pair. An empty pair is (-inf, 0).
struct MaxSum {
  float m, s;
};

// The union of two pairs. Symmetric in its arguments bit for bit (max and + commute), so both
// lanes of a butterfly exchange hold the same result.
__device__ __forceinline__ MaxSum merge(MaxSum a, MaxSum b) {
  const float m = fmaxf(a.m, b.m);
  if (m == -INFINITY) return MaxSum{m, 0.0f};
  return MaxSum{m, a.s * expf(a.m - m) + b.s * expf(b.m - m)};
}

__device__ __forceinline__ MaxSum wave_merge(MaxSum v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v = merge(v, MaxSum{__shfl_xor(v.m, off), __shfl_xor(v.s, off)});
  return v;
}

// The four columns 4 q .. 4 q + 3 of a row (-inf past N): one 16-B load where the row is 16-B
// aligned and the quad is whole, four 4-B loads otherwise -- the same values either way.
__device__ __forceinline__ float4 load_quad(const float* __restrict__ z, int q, int N, bool vec) {
  const int j = 4 * q;
  if (vec && j + 4 <= N) return *reinterpret_cast<const float4*>(z + j);
  float4 v;
  v.x = z[j];  // j < N: the caller's loop bound
  v.y = j + 1 < N ? z[j + 1] : -INFINITY;
  v.z = j + 2 < N ? z[j + 2] : -INFINITY;
  v.w = j + 3 < N ? z[j + 3] : -INFINITY;
  return v;
}

// The pair of the row z[0, N), in every thread of the workgroup (kBlock threads, all of them
// calling). Thread t folds the quads t, t + 256, ... in order: the quad's maximum first (one
// rescale of the running sum per quad), then its four terms in column order; the lanes merge by
// an xor butterfly (32, 16, .. 1), the waves as ((w0 + w1) + w2) + w3 through red_m / red_s
// (kWavesPerBlock floats each; one barrier inside, and the caller puts one between this call's
// reads of them and its next write). A fixed function of the row's N values.
__device__ __forceinline__ MaxSum block_row_maxsum(const float* z, int N, bool vec, float* red_m,
                                                   float* red_s) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int quads = (N + 3) / 4;
  MaxSum acc{-INFINITY, 0.0f};
  for (int q = tid; q < quads; q += kBlock) {
    const float4 v = load_quad(z, q, N, vec);
    const float qm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (qm > acc.m) {
      acc.s = acc.s * expf(acc.m - qm);
      acc.m = qm;
    }
    if (acc.m != -INFINITY) {
      acc.s = acc.s + expf(v.x - acc.m);
      acc.s = acc.s + expf(v.y - acc.m);
      acc.s = acc.s + expf(v.z - acc.m);
      acc.s = acc.s + expf(v.w - acc.m);
    }
  }
  acc = wave_merge(acc);
  if (lane == 0) {
    red_m[wave] = acc.m;
    red_s[wave] = acc.s;
  }
  __syncthreads();
  MaxSum row{red_m[0], red_s[0]};
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) row = merge(row, MaxSum{red_m[w], red_s[w]});
  return row;
}

}  // namespace
}  // namespace gcg
