// softmax_csr.hip -- softmax cross-entropy of a wide logits row against a sparse soft target
// (reference loc2lang.py:193-196 on the l1-normalised bag of words of loc2lang.py:253, which
// the reference densifies per batch): the row losses and the logits' gradient in one launch,
// the target read as the CSR row it is.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "row_maxsum.h"

using namespace gcg;

namespace {

constexpr int64_t kMaxCols = int64_t{1} << 24;

// One workgroup of 256 threads per row (rows blockIdx.x, + gridDim.x, ...).
//   1. the row's MaxSum (block_row_maxsum, row_maxsum.h): thread t folds the quads t, t + 256,
//      ... in order, the lanes merge by an xor butterfly, the waves as ((w0 + w1) + w2) + w3.
//   2. thread t adds the target entries t, t + 256, ... of the row: y (for T) and
//      y * (lse - z[col]); lanes by the butterfly, waves in order.
//   3. after a barrier (out may be the logits: every z[col] has been read), out = (s T) * p.
//   4. after a second barrier the entries are subtracted: out[col] -= s * y.
// Nothing here depends on M, the grid, or another row.
__global__ __launch_bounds__(kBlock) void softmax_xent_csr_kernel(
    int64_t M, int N, const float* logits, int64_t ldl, int64_t y_rows,
    const int32_t* __restrict__ y_indptr, const int32_t* __restrict__ y_indices,
    const float* __restrict__ y_vals, const int32_t* __restrict__ rows, float scale,
    const float* __restrict__ scale_dev, float* out, int64_t ldo,
    float* __restrict__ loss_rows) {
  __shared__ float red_m[kWavesPerBlock], red_s[kWavesPerBlock], red_t[kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int quads = (N + 3) / 4;
  const float s = scale * (scale_dev != nullptr ? *scale_dev : 1.0f);

  for (int64_t i = blockIdx.x; i < M; i += gridDim.x) {
    const float* z = logits + i * ldl;
    const bool vec = (reinterpret_cast<uintptr_t>(z) & 15) == 0;
    const MaxSum row = block_row_maxsum(z, N, vec, red_m, red_s);
    const float lse = row.m + logf(row.s);

    float T = 1.0f;  // y_indptr NULL: out = softmax
    int32_t k0 = 0, k1 = 0;
    bool bad_row = false;
    if (y_indptr != nullptr) {
      const int64_t yr = rows != nullptr ? rows[i] : i;
      bad_row = yr < 0 || yr >= y_rows;
      if (!bad_row) {
        k0 = y_indptr[yr];
        k1 = y_indptr[yr + 1];
      }
      float t_sum = 0.0f, l_sum = 0.0f;
      for (int64_t k = static_cast<int64_t>(k0) + tid; k < k1; k += kBlock) {
        const int32_t col = y_indices[k];
        if (col < 0 || col >= N) continue;
        const float y = y_vals[k];
        t_sum = t_sum + y;
        l_sum = l_sum + y * (lse - z[col]);
      }
      t_sum = wave_sum(t_sum);
      l_sum = wave_sum(l_sum);
      __syncthreads();  // red_s has been read by every thread
      if (lane == 0) {
        red_t[wave] = t_sum;
        red_s[wave] = l_sum;
      }
      __syncthreads();
      T = ((red_t[0] + red_t[1]) + red_t[2]) + red_t[3];
      if (tid == 0 && loss_rows != nullptr)
        loss_rows[i] = bad_row ? NAN : ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
    }
    if (out != nullptr) {
      __syncthreads();  // every z[col] of the row has been read: out may be the logits
      float* o = out + i * ldo;
      const bool ovec = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
      const float sT = y_indptr != nullptr ? s * T : 1.0f;
      const float inv = 1.0f / row.s;
      for (int q = tid; q < quads; q += kBlock) {
        const float4 v = load_quad(z, q, N, vec);
        const int j = 4 * q;
        float4 g;
        // an empty target row (T = 0) is a zero row whatever the logits hold
        g.x = sT == 0.0f ? 0.0f : sT * (expf(v.x - row.m) * inv);
        g.y = sT == 0.0f ? 0.0f : sT * (expf(v.y - row.m) * inv);
        g.z = sT == 0.0f ? 0.0f : sT * (expf(v.z - row.m) * inv);
        g.w = sT == 0.0f ? 0.0f : sT * (expf(v.w - row.m) * inv);
        if (ovec && j + 4 <= N) {
          *reinterpret_cast<float4*>(o + j) = g;
        } else {
          o[j] = g.x;
          if (j + 1 < N) o[j + 1] = g.y;
          if (j + 2 < N) o[j + 2] = g.z;
          if (j + 3 < N) o[j + 3] = g.w;
        }
      }
      if (y_indptr != nullptr) {
        __threadfence_block();
        __syncthreads();  // the row is written: its entries are subtracted in place
        for (int64_t k = static_cast<int64_t>(k0) + tid; k < k1; k += kBlock) {
          const int32_t col = y_indices[k];
          if (col < 0 || col >= N) continue;
          o[col] = o[col] - s * y_vals[k];
        }
      }
    }
    __syncthreads();  // the slots are rewritten for the next row
  }
}

}  // namespace

extern "C" {

gcg_status gcg_softmax_xent_csr_f32(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                    int64_t y_rows, const int32_t* y_indptr,
                                    const int32_t* y_indices, const float* y_vals,
                                    const int32_t* rows, float scale, const float* scale_dev,
                                    float* out, int64_t ldo, float* loss_rows,
                                    gcg_stream_t stream) {
  const char* fn = "gcg_softmax_xent_csr_f32";
  if (M < 0 || M > INT32_MAX || N < 1 || N > kMaxCols || y_rows < 0 || y_rows > INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes M=%lld N=%lld y_rows=%lld (1 <= N <= 2^24)",
                fn, static_cast<long long>(M), static_cast<long long>(N),
                static_cast<long long>(y_rows));
  if (ldl < N || (out != nullptr && ldo < N))
    return fail(GCG_ERR_INVALID_ARG, "%s: row stride below N = %lld", fn,
                static_cast<long long>(N));
  if (M == 0) return GCG_OK;
  if (logits == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL logits", fn);
  if (y_indptr != nullptr) {
    if (y_indices == nullptr || y_vals == nullptr || loss_rows == nullptr)
      return fail(GCG_ERR_INVALID_ARG, "%s: a target needs y_indices, y_vals and loss_rows", fn);
    if (rows == nullptr && y_rows < M)
      return fail(GCG_ERR_INVALID_ARG, "%s: the target has %lld rows, the logits %lld", fn,
                  static_cast<long long>(y_rows), static_cast<long long>(M));
  } else if (out == nullptr) {
    return fail(GCG_ERR_INVALID_ARG, "%s: neither a target nor out", fn);
  }
  if (!aligned(logits, 4) || !aligned(y_indptr, 4) || !aligned(y_indices, 4) ||
      !aligned(y_vals, 4) || !aligned(rows, 4) || !aligned(scale_dev, 4) || !aligned(out, 4) ||
      !aligned(loss_rows, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(M, int64_t{1} << 20));
  hipLaunchKernelGGL(softmax_xent_csr_kernel, dim3(grid), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), M, static_cast<int>(N), logits, ldl,
                     y_rows, y_indptr, y_indices, y_vals, rows, scale, scale_dev, out, ldo,
                     loss_rows);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
