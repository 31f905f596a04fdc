// dropout.hip -- dropout with a counter-based (Philox4x32-10) mask keyed on the element's
// logical coordinates (include/gcg_spmm.h): the dense pass (lasagne.layers.dropout on the
// hidden layer, mlpconv.py:210-211; the dense Zipf-head block of X) and the pass over the
// stored values of a CSR (SparseInputDropoutLayer, mlpconv.py:37-58), for X and for X^T.
// The fused backward lives beside relu_backward_kernel in csr_ops.hip.
#include <hip/hip_runtime.h>

#include "common.h"
#include "philox.h"

using namespace gcg;

namespace {

// One thread per group of four consecutive columns of one row: one Philox call per group when
// the logical columns are the stored ones (COLS = false), one per element when they come from
// col_ids. VEC: 16-B loads / stores on whole groups; the ragged last group of a row
// (K % 4 != 0) and the unaligned layout go element-wise and never touch a column >= K.
// X and Y may alias (each element is read, then written, by the same thread).
template <bool VEC, bool COLS>
__global__ __launch_bounds__(256) void dropout_kernel(int64_t M, int64_t K, int64_t K4,
                                                      const float* X, int64_t ldx, float* Y,
                                                      int64_t ldy, DropKey d,
                                                      const int32_t* __restrict__ step_dev,
                                                      int64_t row0,
                                                      const int32_t* __restrict__ col_ids) {
  d.step = static_cast<uint32_t>(*step_dev);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  // (row, group) of this thread and of one grid stride: no division inside the loop
  int64_t r = idx / K4, g = idx - r * K4;
  const int64_t dr = stride / K4, dg = stride - dr * K4;
  while (r < M) {
    const int64_t c = g * 4, i = row0 + r;
    const float* xr = X + r * ldx + c;
    float* yr = Y + r * ldy + c;
    if (VEC && c + 4 <= K) {
      float4 v = *reinterpret_cast<const float4*>(xr);
      if constexpr (COLS) {
        v.x = drop_element(d, i, col_ids[c], v.x);
        v.y = drop_element(d, i, col_ids[c + 1], v.y);
        v.z = drop_element(d, i, col_ids[c + 2], v.z);
        v.w = drop_element(d, i, col_ids[c + 3], v.w);
      } else {
        const Philox4 w = drop_words(d, i, g);
        v.x = drop_apply(d, w.w[0], v.x);
        v.y = drop_apply(d, w.w[1], v.y);
        v.z = drop_apply(d, w.w[2], v.z);
        v.w = drop_apply(d, w.w[3], v.w);
      }
      *reinterpret_cast<float4*>(yr) = v;
    } else {
      Philox4 w = {};
      if constexpr (!COLS) w = drop_words(d, i, g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e < K) {
          if constexpr (COLS) yr[e] = drop_element(d, i, col_ids[c + e], xr[e]);
          else yr[e] = drop_apply(d, w.w[e], xr[e]);
        }
      }
    }
    g += dg;
    r += dr;
    if (g >= K4) {
      g -= K4;
      ++r;
    }
  }
}

// Stored entries per workgroup of csr_dropout_kernel: the work is cut by nonzeros (CSR(X^T) of
// a bag-of-words matrix has Zipf row lengths; its longest row holds a constant share of all
// entries), so a long row spans many workgroups and a run of short rows shares one.
constexpr int kCsrSlice = 2048;

// Largest r in [lo, hi] with indptr[r] <= k: the storage row of entry k (indptr[r + 1] > k
// follows, empty rows are passed over). Never leaves [lo, hi], whatever indptr holds.
__device__ __forceinline__ int64_t row_of_entry(const int32_t* __restrict__ indptr, int64_t k,
                                                int64_t lo, int64_t hi) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (indptr[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void csr_dropout_kernel(int64_t n_rows, int64_t nnz,
                                                          const int32_t* __restrict__ indptr,
                                                          const int32_t* __restrict__ indices,
                                                          const float* vals, float* vals_out,
                                                          int transposed, DropKey d,
                                                          const int32_t* __restrict__ step_dev) {
  d.step = static_cast<uint32_t>(*step_dev);
  const int64_t s0 = static_cast<int64_t>(blockIdx.x) * kCsrSlice;
  const int64_t s1 = min(nnz, s0 + kCsrSlice);
  if (s0 >= s1) return;
  // the slice's first and last storage rows (uniform), then every entry's row between them,
  // walking forward: a thread's entries ascend, so its row never goes back
  const int64_t r_first = row_of_entry(indptr, s0, 0, n_rows - 1);
  const int64_t r_last = row_of_entry(indptr, s1 - 1, r_first, n_rows - 1);
  int64_t r = r_first;
  for (int64_t k = s0 + threadIdx.x; k < s1; k += 256) {
    r = row_of_entry(indptr, k, r, r_last);
    const int64_t c = indices[k];
    const float v = vals[k];
    vals_out[k] = transposed ? drop_element(d, c, r, v) : drop_element(d, r, c, v);
  }
}

DropKey drop_key(uint32_t threshold, float scale, uint64_t seed, uint32_t stream_id) {
  return DropKey{static_cast<uint32_t>(seed & 0xffffffffu), static_cast<uint32_t>(seed >> 32), 0u,
                 stream_id, threshold, scale};
}

}  // namespace

extern "C" {

gcg_status gcg_dropout_f32(int64_t M, int64_t K, const float* X, int64_t ldx, float* Y,
                           int64_t ldy, uint32_t threshold, float scale, uint64_t seed,
                           const int32_t* step_dev, uint32_t stream_id, int64_t row0,
                           const int32_t* col_ids, gcg_stream_t stream) {
  if (M < 0 || K < 0 || row0 < 0)
    return fail(GCG_ERR_INVALID_ARG, "gcg_dropout_f32: bad sizes M=%lld K=%lld row0=%lld",
                static_cast<long long>(M), static_cast<long long>(K),
                static_cast<long long>(row0));
  if (M == 0 || K == 0) return GCG_OK;
  if (X == nullptr || Y == nullptr || step_dev == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_dropout_f32: null operand");
  if (ldx < K || ldy < K) return fail(GCG_ERR_INVALID_ARG, "gcg_dropout_f32: ld < K");
  if (!aligned(X, 4) || !aligned(Y, 4) || !aligned(step_dev, 4) || !aligned(col_ids, 4))
    return fail(GCG_ERR_MISALIGNED, "gcg_dropout_f32: operand not 4-B aligned");
  const int64_t K4 = (K + 3) / 4;
  if (M > INT64_MAX / K4) return fail(GCG_ERR_INVALID_ARG, "gcg_dropout_f32: M * K overflows");
  const bool vec = ldx % 4 == 0 && ldy % 4 == 0 && aligned(X, 16) && aligned(Y, 16);
  const DropKey d = drop_key(threshold, scale, seed, stream_id);
  const dim3 grid(grid_for(M * K4));
  auto st = static_cast<hipStream_t>(stream);
#define GCG_DROPOUT_LAUNCH(V, C)                                                              \
  hipLaunchKernelGGL((dropout_kernel<V, C>), grid, dim3(256), 0, st, M, K, K4, X, ldx, Y, ldy, \
                     d, step_dev, row0, col_ids)
  if (vec) {
    if (col_ids != nullptr) GCG_DROPOUT_LAUNCH(true, true);
    else GCG_DROPOUT_LAUNCH(true, false);
  } else {
    if (col_ids != nullptr) GCG_DROPOUT_LAUNCH(false, true);
    else GCG_DROPOUT_LAUNCH(false, false);
  }
#undef GCG_DROPOUT_LAUNCH
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_csr_dropout_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                               const int32_t* indptr, const int32_t* indices, const float* vals,
                               float* vals_out, int transposed, uint32_t threshold, float scale,
                               uint64_t seed, const int32_t* step_dev, uint32_t stream_id,
                               gcg_stream_t stream) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || nnz > INT32_MAX || n_rows >= INT32_MAX ||
      (transposed != 0 && transposed != 1))
    return fail(GCG_ERR_INVALID_ARG, "gcg_csr_dropout_f32: bad sizes");
  if (nnz == 0) return GCG_OK;
  if (n_rows == 0 || n_cols == 0)
    return fail(GCG_ERR_INVALID_ARG, "gcg_csr_dropout_f32: nnz > 0 in an empty matrix");
  if (indptr == nullptr || indices == nullptr || vals == nullptr || vals_out == nullptr ||
      step_dev == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_csr_dropout_f32: null operand");
  if (!aligned(indptr, 4) || !aligned(indices, 4) || !aligned(vals, 4) ||
      !aligned(vals_out, 4) || !aligned(step_dev, 4))
    return fail(GCG_ERR_MISALIGNED, "gcg_csr_dropout_f32: operand not 4-B aligned");
  const DropKey d = drop_key(threshold, scale, seed, stream_id);
  const dim3 grid(static_cast<unsigned>((nnz + kCsrSlice - 1) / kCsrSlice));
  hipLaunchKernelGGL(csr_dropout_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                     n_rows, nnz, indptr, indices, vals, vals_out, transposed, d, step_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
