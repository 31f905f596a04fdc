// csr_ops.hip -- device CSR utilities around the SpMM: validation (scipy check_format on
// upload), CSR transpose (the X^T of Theano's grad of S.dot(X, W), mlpconv.py:71), and the
// deterministic scatter-add of rows (grad of Y[target_indices], mlpconv.py:94, with the
// duplicates tensormain.py:226 draws).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "scratch.h"
#include "index_kernels.h"
#include "philox.h"

using namespace gcg;

namespace {


__global__ void validate_kernel(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                const int32_t* __restrict__ indptr,
                                const int32_t* __restrict__ indices, int32_t* status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n_rows; i += stride) {
    const int32_t v = indptr[i];
    bool bad = (i == 0 && v != 0) || (i == n_rows && v != nnz) || v < 0 || v > nnz ||
               (i < n_rows && indptr[i + 1] < v);
    if (bad) atomicMax(status, int32_t(GCG_ERR_BAD_CSR));
  }
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < nnz; j += stride) {
    const int32_t c = indices[j];
    if (c < 0 || c >= n_cols) atomicMax(status, int32_t(GCG_ERR_BAD_CSR));
  }
}

// seg_ptr[r] = number of sorted keys < r (lower bound), r in [0, n_rows].
__global__ void lower_bound_kernel(const int32_t* __restrict__ sorted_keys, int64_t n,
                                   int64_t n_rows, int32_t* __restrict__ seg_ptr) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r <= n_rows; r += stride) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted_keys[mid] < r) lo = mid + 1; else hi = mid;
    }
    seg_ptr[r] = static_cast<int32_t>(lo);
  }
}

// out[r] += sum over i in segment r (ascending i) of src[sorted_pos[i]]; one wave per row.
__global__ __launch_bounds__(kBlock) void scatter_add_kernel(int64_t n_rows,
                                                             const int32_t* __restrict__ seg_ptr,
                                                             const int32_t* __restrict__ sorted_pos,
                                                             const float* __restrict__ src,
                                                             int64_t lds, int64_t K,
                                                             float* __restrict__ out, int64_t ldo) {
  const int64_t r = uniform(static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6));
  if (r >= n_rows) return;
  const int s = uniform(seg_ptr[r]), e = uniform(seg_ptr[r + 1]);
  if (s == e) return;
  const int lane = threadIdx.x & (kWave - 1);
  float* orow = out + r * ldo;
  for (int64_t c = lane; c < K; c += kWave) {
    float acc = orow[c];
    for (int i = s; i < e; ++i) acc = acc + src[static_cast<int64_t>(sorted_pos[i]) * lds + c];
    orow[c] = acc;
  }
}

__global__ void permute_transpose_kernel(int64_t nnz, const int32_t* __restrict__ perm,
                                         const int32_t* __restrict__ row_of,
                                         const float* __restrict__ vals,
                                         int32_t* __restrict__ out_indices,
                                         float* __restrict__ out_vals) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < nnz; k += stride) {
    const int32_t j = perm[k];
    out_indices[k] = row_of[j];
    out_vals[k] = vals[j];
  }
}

// The scratch of a stable sort of n int32 keys that carry their positions (iota): the sorted
// keys, the positions, then `extra` more arrays of n for the caller, hipcub's temporary. The
// sorted positions go to the caller's `perm`. take_exact: nothing to sort, empty arrays.
struct SortSpace {
  int32_t *keys_out, *iota, *extra[2];
  Tmp tmp;
  size_t total;
};

gcg_status sort_space(const char* fn, int64_t n, int end_bit, int extra, void* workspace,
                      SortSpace* s) {
  Carver cv(workspace);
  s->keys_out = cv.take_exact<int32_t>(n);
  s->iota = cv.take_exact<int32_t>(n);
  for (int i = 0; i < extra; ++i) s->extra[i] = cv.take_exact<int32_t>(n);
  auto* k = reinterpret_cast<uint32_t*>(s->keys_out);
  TmpSize ts;
  ts.add(GCG_CUB(DeviceRadixSort::SortPairs, k, k, s->iota, s->iota, static_cast<int>(n), 0, end_bit));
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

// iota, then keys -> keys_out with the positions -> perm.
gcg_status sort_with_positions(const SortSpace& s, int64_t n, int end_bit, const int32_t* keys,
                               int32_t* perm, hipStream_t st) {
  hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n)), dim3(256), 0, st, s.iota, n);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, reinterpret_cast<const uint32_t*>(keys),
      reinterpret_cast<uint32_t*>(s.keys_out), s.iota, perm, static_cast<int>(n), 0, end_bit, st)));
  return GCG_OK;
}

// Rectify backward + bias gradient in one pass (Theano's grad of
// rectify(S.dot(H, Z) + b), mlpconv.py:75-77): g = gY where Y > 0 else 0, written to g_out
// (may alias gY), and per-block column partial sums of g. Block = 4 waves; wave w takes rows
// r0 + w, r0 + w + 4, ...; lanes span the columns in dwordx4 (or dword) pieces. MASK = false:
// column sums of gY only (Y and g_out unused) -- the bias gradient of a dense projection.
constexpr int kReluMinRows = 512;   // rows per block at least ...
constexpr int kReluMaxBlocks = 1024;  // ... and at most this many blocks (partial rows)
constexpr int kReluMaxK4 = 4;       // dwordx4 column pieces per lane (K <= 1024 on the vector path)

int64_t relu_rows_per_block(int64_t M) {
  const int64_t r = (M + kReluMaxBlocks - 1) / kReluMaxBlocks;
  return std::max<int64_t>(kReluMinRows, (r + 3) / 4 * 4);
}

// GATE: the mask comes from the gate bytes of the SpMM epilogue (2 / 1 / 0 -> g, g/2, 0:
// Theano's 0.5*(1 + sgn(x)) rectify gradient) instead of Y > 0.
__device__ __forceinline__ float gate_apply(float g, uint32_t code) {
  return code == 2u ? g : (code == 1u ? 0.5f * g : 0.0f);
}

// Where the mask of the pass comes from: none (g = t), Y > 0, or the gate bytes.
enum MaskSource { kMaskNone, kMaskY, kMaskGate };

// Both kernels are the one pass of rectify_backward_pass.inc (see there for why it is included
// and not called). MASK = false: column sums of gY only -- the bias gradient of a projection.
template <int VEC, bool MASK, bool GATE = false>
__global__ __launch_bounds__(256) void relu_backward_kernel(
    int64_t M, int K, int64_t rows_per_block, const float* gY, int64_t ldg,
    const float* __restrict__ Y, int64_t ldy, float* g_out, int64_t ldo,
    float* __restrict__ partial, const uint8_t* __restrict__ gate = nullptr,
    int64_t ldgate = 0) {
  constexpr MaskSource kMask = GATE ? kMaskGate : (MASK ? kMaskY : kMaskNone);
  constexpr bool kDrop = false;
  const DropKey d{};  // (unread without kDrop)
  const int64_t row0 = 0;
#include "rectify_backward_pass.inc"
}

// The gradient of drop(rectify(.)) (gcg_dropout_relu_backward_f32): the dropout mask, then the
// gate rule (GATE = false: g = t), in the same single pass.
template <int VEC, bool GATE>
__global__ __launch_bounds__(256) void dropout_relu_backward_kernel(
    int64_t M, int K, int64_t rows_per_block, const float* gY, int64_t ldg, float* g_out,
    int64_t ldo, float* __restrict__ partial, const uint8_t* __restrict__ gate, int64_t ldgate,
    DropKey d, const int32_t* __restrict__ step_dev, int64_t row0) {
  constexpr MaskSource kMask = GATE ? kMaskGate : kMaskNone;
  constexpr bool kDrop = true;
  const float* const Y = nullptr;  // (unread without kMaskY)
  const int64_t ldy = 0;
  d.step = static_cast<uint32_t>(*step_dev);
#include "rectify_backward_pass.inc"
}

// The pass for any K (gcg_rectify_backward_wide_f32): the columns in slabs of kReluSlab, the slab
// in blockIdx.y. A workgroup runs the included pass on its slab as on a matrix of that slab's
// columns -- the names the pass reads (K, gY, g_out, gate, partial) are the slab's here -- so row
// blocks, wave interleave, accumulation order and partials are the narrow kernels', which are
// not touched. Slab s keeps its partials (one row of its own width per row block) behind those
// of the slabs before it, all of full width: partial_all + n_blocks * kReluSlab * s.
constexpr int kReluSlab = 64 * 4 * kReluMaxK4;

// A slab's DropKey: the pass numbers a slab's columns from 0, the mask wants the logical column
// kReluSlab * s + c. The pass calls drop_words / drop_element with its `d`; for this type they
// resolve to the two overloads below, which add the slab's offset (a multiple of 4 columns).
struct SlabDropKey : DropKey {
  int col0;
};

__device__ __forceinline__ Philox4 drop_words(const SlabDropKey& d, int64_t i, int64_t j4) {
  return drop_words(static_cast<const DropKey&>(d), i, j4 + (d.col0 >> 2));
}

__device__ __forceinline__ float drop_element(const SlabDropKey& d, int64_t i, int64_t j, float v) {
  return drop_element(static_cast<const DropKey&>(d), i, j + d.col0, v);
}

template <int VEC, bool DROP, bool GATE>
__global__ __launch_bounds__(256) void rectify_backward_wide_kernel(
    int64_t M, int k_all, int64_t rows_per_block, const float* gY_all, int64_t ldg,
    float* g_all, int64_t ldo, float* __restrict__ partial_all,
    const uint8_t* __restrict__ gate_all, int64_t ldgate, DropKey key,
    const int32_t* __restrict__ step_dev, int64_t row0) {
  constexpr MaskSource kMask = GATE ? kMaskGate : kMaskNone;
  constexpr bool kDrop = DROP;
  const int col0 = static_cast<int>(blockIdx.y) * kReluSlab;
  const int K = min(kReluSlab, k_all - col0);
  const float* const gY = gY_all + col0;
  float* const g_out = g_all + col0;
  const uint8_t* const gate = GATE ? gate_all + col0 : nullptr;
  float* const partial = partial_all + static_cast<int64_t>(gridDim.x) * col0;
  const float* const Y = nullptr;  // (unread without kMaskY)
  const int64_t ldy = 0;
  SlabDropKey d{key, col0};  // (unread without kDrop)
  if constexpr (DROP) d.step = static_cast<uint32_t>(*step_dev);
#include "rectify_backward_pass.inc"
}

// out[c] = sum over the partial rows of partial[b][c], in a fixed order: workgroup = 16 waves
// over 64 columns; wave w sums rows w, w + 16, ... in order, then wave 0 adds the 16 in order.
__global__ __launch_bounds__(1024) void column_sum_kernel(int64_t n_blocks, int K,
                                                         const float* __restrict__ partial,
                                                         float* __restrict__ out) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int cc = c < K ? c : K - 1;
  float s = 0.f;
#pragma unroll 4
  for (int64_t b = w; b < n_blocks; b += 16) s += partial[b * K + cc];
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && c < K) {
    float t = red[0][lane];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += red[i][lane];
    out[c] = t;
  }
}

// lasagne.updates.adam (mlpconv.py:263) for one parameter, every elementwise op of the step in
// one pass (the trainer's update otherwise runs ~8 torch kernels per parameter):
//   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= a_t*m / (sqrt(v) + eps)
// a_t = lr*sqrt(1-b2^t)/(1-b1^t) is read on the device (a captured HIP graph replays it).
__global__ __launch_bounds__(256) void adam_kernel(int64_t n, float* __restrict__ p,
                                                   const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ step_dev, float b1,
                                                   float b2, float eps) {
  const float a_t = *step_dev;
  const float c1 = 1.0f - b1, c2 = 1.0f - b2;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gi = g[i];
    const float mi = b1 * m[i] + c1 * gi;
    const float vi = b2 * v[i] + c2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - (a_t * mi) / (sqrtf(vi) + eps);
  }
}

// lasagne.updates.adamax (loc2lang.py:207) for one parameter, in adam_kernel's shape:
//   m = b1*m + (1-b1)*g;  u = max(b2*u, |g|);  p -= a_t*m / (u + eps)
// a_t = lr/(1-b1^t) is read on the device.
__global__ __launch_bounds__(256) void adamax_kernel(int64_t n, float* __restrict__ p,
                                                     const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ u,
                                                     const float* __restrict__ step_dev, float b1,
                                                     float b2, float eps) {
  const float a_t = *step_dev;
  const float c1 = 1.0f - b1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gi = g[i];
    const float mi = b1 * m[i] + c1 * gi;
    const float ui = fmaxf(b2 * u[i], fabsf(gi));
    m[i] = mi;
    u[i] = ui;
    p[i] = p[i] - (a_t * mi) / (ui + eps);
  }
}

// lasagne.regularization l1 / l2 of one weight (mlpconv.py:235-243): partial sums of |w| and
// w*w over a fixed grid (kPenBlocks blocks, grid-stride order fixed by the grid), one pair per
// block; then ONE thread adds the pairs in block order -- deterministic, graph-capturable.
constexpr int kPenBlocks = 256;

__global__ __launch_bounds__(256) void l1l2_partial_kernel(int64_t n, const float* __restrict__ w,
                                                           float* __restrict__ part) {
  __shared__ float s1[256], s2[256];
  float a = 0.f, q = 0.f;
  const int64_t stride = static_cast<int64_t>(kPenBlocks) * 256;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
    const float x = w[i];
    a += fabsf(x);
    q += x * x;
  }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = q;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (static_cast<int>(threadIdx.x) < h) {
      s1[threadIdx.x] += s1[threadIdx.x + h];
      s2[threadIdx.x] += s2[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = s1[0];
    part[2 * blockIdx.x + 1] = s2[0];
  }
}

// out = ((acc_in ? *acc_in : 0) + l1 * sum|w|) + l2 * sum w^2 (acc_in may alias out).
__global__ __launch_bounds__(64) void l1l2_finish_kernel(const float* __restrict__ part, float l1,
                                                         float l2, const float* acc_in,
                                                         float* out) {
  if (threadIdx.x != 0) return;
  float a = 0.f, q = 0.f;
  for (int b = 0; b < kPenBlocks; ++b) {
    a += part[2 * b];
    q += part[2 * b + 1];
  }
  const float base = acc_in != nullptr ? *acc_in : 0.f;
  out[0] = (base + a * l1) + q * l2;
}

// d/dw of l1 * sum|w| + l2 * sum w^2, times the upstream gradient: s * (l1 sgn(w) + 2 l2 w)
// (Theano's grad of abs is sgn, 0 at 0).
__global__ __launch_bounds__(256) void l1l2_grad_kernel(int64_t n, const float* __restrict__ w,
                                                        float l1, float l2,
                                                        const float* __restrict__ scale_dev,
                                                        float* __restrict__ dw) {
  const float s = scale_dev != nullptr ? *scale_dev : 1.0f;
  const float c1 = s * l1, c2 = s * (2.0f * l2);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = w[i];
    const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
    dw[i] = c1 * sg + c2 * x;
  }
}

}  // namespace

extern "C" {

gcg_status gcg_adam_step_f32(int64_t n, float* p, const float* g, float* m, float* v,
                             const float* step_dev, float beta1, float beta2, float eps,
                             gcg_stream_t stream) {
  if (n < 0 || (n > 0 && (p == nullptr || g == nullptr || m == nullptr || v == nullptr ||
                          step_dev == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_adam_step_f32: bad arguments");
  if (n == 0) return GCG_OK;
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     n, p, g, m, v, step_dev, beta1, beta2, eps);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_adamax_step_f32(int64_t n, float* p, const float* g, float* m, float* u,
                               const float* step_dev, float beta1, float beta2, float eps,
                               gcg_stream_t stream) {
  if (n < 0 || (n > 0 && (p == nullptr || g == nullptr || m == nullptr || u == nullptr ||
                          step_dev == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_adamax_step_f32: bad arguments");
  if (n == 0) return GCG_OK;
  hipLaunchKernelGGL(adamax_kernel, dim3(grid_for(n)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n, p, g, m, u, step_dev, beta1, beta2, eps);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_l1l2_penalty_f32(int64_t n, const float* W, float l1, float l2,
                                const float* acc_in, float* out, void* workspace,
                                size_t workspace_bytes, gcg_stream_t stream) {
  if (n < 0 || (n > 0 && W == nullptr) || out == nullptr || workspace == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_l1l2_penalty_f32: bad arguments");
  if (workspace_bytes < GCG_L1L2_WORKSPACE_BYTES || !aligned(workspace, 4))
    return fail(GCG_ERR_INVALID_ARG, "gcg_l1l2_penalty_f32: workspace needs %d aligned bytes",
                GCG_L1L2_WORKSPACE_BYTES);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(l1l2_partial_kernel, dim3(kPenBlocks), dim3(256), 0, st, n, W, part);
  hipLaunchKernelGGL(l1l2_finish_kernel, dim3(1), dim3(64), 0, st, part, l1, l2, acc_in, out);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_l1l2_grad_f32(int64_t n, const float* W, float l1, float l2,
                             const float* scale_dev, float* dW, gcg_stream_t stream) {
  if (n < 0 || (n > 0 && (W == nullptr || dW == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_l1l2_grad_f32: bad arguments");
  if (n == 0) return GCG_OK;
  hipLaunchKernelGGL(l1l2_grad_kernel, dim3(grid_for(n)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n, W, l1, l2, scale_dev, dW);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_csr_validate(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* indptr,
                            const int32_t* indices, int32_t* status_dev, gcg_stream_t stream) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || indptr == nullptr || status_dev == nullptr ||
      (nnz > 0 && indices == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "bad args to gcg_csr_validate");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(validate_kernel, dim3(grid_for(std::max(n_rows + 1, nnz))), dim3(256), 0, st,
                     n_rows, n_cols, nnz, indptr, indices, status_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_index_csr(int64_t n_idx, const int32_t* idx, int64_t n_rows, int32_t* seg_ptr,
                         int32_t* sorted_pos, void* workspace, size_t workspace_bytes,
                         size_t* workspace_needed, gcg_stream_t stream) {
  if (n_idx < 0 || n_idx > INT32_MAX || n_rows < 0 || n_rows >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "bad sizes");
  const int end_bit = bits_to_count(n_rows + 1);
  SortSpace s;
  if (gcg_status rc = sort_space("gcg_index_csr", n_idx, end_bit, 0, workspace, &s)) return rc;
  if (workspace_needed) *workspace_needed = s.total;
  if (seg_ptr == nullptr && sorted_pos == nullptr) return GCG_OK;  // sizing query
  if (seg_ptr == nullptr || (n_idx > 0 && (idx == nullptr || sorted_pos == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "NULL buffer");
  // (this entry and the transpose have never asked the workspace for an alignment: 1)
  if (s.total > 0)  // nothing to sort and no temporary: no workspace
    if (gcg_status rc = check_workspace("gcg_index_csr", workspace, workspace_bytes, s.total, 1))
      return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_idx > 0)
    if (gcg_status rc = sort_with_positions(s, n_idx, end_bit, idx, sorted_pos, st)) return rc;
  hipLaunchKernelGGL(lower_bound_kernel, dim3(grid_for(n_rows + 1)), dim3(256), 0, st, s.keys_out,
                     n_idx, n_rows, seg_ptr);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_scatter_add_rows_f32(int64_t n_rows, const int32_t* seg_ptr,
                                    const int32_t* sorted_pos, const float* src, int64_t lds,
                                    int64_t K, float* out, int64_t ldo, gcg_stream_t stream) {
  if (n_rows < 0 || n_rows > INT32_MAX || K < 0 || lds < K || ldo < K || seg_ptr == nullptr ||
      (K > 0 && out == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "bad args to gcg_scatter_add_rows_f32");
  if (n_rows == 0 || K == 0) return GCG_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(scatter_add_kernel, dim3((n_rows + kWavesPerBlock - 1) / kWavesPerBlock),
                     dim3(kBlock), 0, st, n_rows, seg_ptr, sorted_pos, src, lds, K, out, ldo);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_csr_transpose_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                 const int32_t* indptr, const int32_t* indices,
                                 const float* vals, int32_t* out_indptr, int32_t* out_indices,
                                 float* out_vals, void* workspace, size_t workspace_bytes,
                                 size_t* workspace_needed, gcg_stream_t stream) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || nnz > INT32_MAX || n_cols >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "bad sizes");
  const int end_bit = bits_to_count(n_cols + 1);
  SortSpace s;  // sorted columns, iota, then perm and row_of
  if (gcg_status rc = sort_space("gcg_csr_transpose_f32", nnz, end_bit, 2, workspace, &s)) return rc;
  if (workspace_needed) *workspace_needed = s.total;
  if (out_indptr == nullptr && out_indices == nullptr && out_vals == nullptr) return GCG_OK;
  if (out_indptr == nullptr || indptr == nullptr ||
      (nnz > 0 && (indices == nullptr || vals == nullptr || out_indices == nullptr || out_vals == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "NULL buffer");
  if (s.total > 0)  // no entry and no temporary: no workspace
    if (gcg_status rc = check_workspace("gcg_csr_transpose_f32", workspace, workspace_bytes, s.total, 1))
      return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t *perm = s.extra[0], *row_of = s.extra[1];
  if (nnz > 0) {
    if (gcg_status rc = sort_with_positions(s, nnz, end_bit, indices, perm, st)) return rc;
    hipLaunchKernelGGL(expand_rows_kernel, dim3(grid_for(n_rows)), dim3(256), 0, st, n_rows, indptr, row_of);
    GCG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(permute_transpose_kernel, dim3(grid_for(nnz)), dim3(256), 0, st, nnz, perm,
                       row_of, vals, out_indices, out_vals);
    GCG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(lower_bound_kernel, dim3(grid_for(n_cols + 1)), dim3(256), 0, st, s.keys_out,
                     nnz, n_cols, out_indptr);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_relu_backward_f32_workspace_bytes(int64_t M, int64_t K, size_t* bytes) {
  if (M < 0 || K < 0 || bytes == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_relu_backward_f32_workspace_bytes: bad args");
  const int64_t rpb = relu_rows_per_block(M);
  *bytes = sizeof(float) * static_cast<size_t>((M + rpb - 1) / rpb) * K;
  return GCG_OK;
}

namespace {

// What the dropout entry adds to the pass: the stream's key (its step is read on the device)
// and the logical row of row 0.
struct DropArgs {
  DropKey key;
  const int32_t* step_dev;
  int64_t row0;
};

// The host side of the pass for all four entries: gcg_relu_backward_f32 (kMaskY),
// gcg_relu_backward_gate_f32 (kMaskGate), gcg_column_sum_f32 (kMaskNone, no g_out) and
// gcg_dropout_relu_backward_f32 (drop; kMaskGate or kMaskNone, g_out always written).
gcg_status rectify_backward(const char* fn, MaskSource mask, const DropArgs* drop, int64_t M,
                            int64_t K, const float* gY, int64_t ldg, const float* Y, int64_t ldy,
                            const uint8_t* gate, int64_t ldgate, float* g_out, int64_t ldo,
                            float* bias_grad, void* workspace, size_t workspace_bytes,
                            gcg_stream_t stream) {
  if (M < 0 || K < 0 || K > 64 * 4 * kReluMaxK4 || (drop != nullptr && drop->row0 < 0))
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes M=%lld K=%lld (K <= %d)", fn,
                static_cast<long long>(M), static_cast<long long>(K), 64 * 4 * kReluMaxK4);
  auto st = static_cast<hipStream_t>(stream);
  if (M == 0 || K == 0) {  // an empty sum is zero
    if (bias_grad != nullptr && K > 0)
      GCG_HIP_CHECK(hipMemsetAsync(bias_grad, 0, sizeof(float) * K, st));
    return GCG_OK;
  }
  const bool use_y = mask == kMaskY, store = mask != kMaskNone || drop != nullptr;
  const bool bad_gate =
      mask == kMaskGate && (ldgate < K || ldgate % 4 != 0 || !aligned(gate, 4));
  // (the gate is looked at before the operands without dropout and after them with it: a call
  // with both wrong keeps the status each entry has always given)
  if (bad_gate && drop == nullptr)
    return fail(GCG_ERR_MISALIGNED, "%s: gate needs ldgate >= K, ldgate %% 4 == 0, 4-B base", fn);
  if (gY == nullptr || (store && g_out == nullptr) || (use_y && Y == nullptr) ||
      (!store && bias_grad == nullptr) || (drop != nullptr && drop->step_dev == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: null operand", fn);
  if (ldg < K || (store && ldo < K) || (use_y && ldy < K))
    return fail(GCG_ERR_INVALID_ARG, "%s: ld < K", fn);
  if (bad_gate)
    return fail(GCG_ERR_MISALIGNED, "%s: gate needs ldgate >= K, ldgate %% 4 == 0, 4-B base", fn);
  if (!aligned(gY, 4) || (store && !aligned(g_out, 4)) || (use_y && !aligned(Y, 4)) ||
      (drop != nullptr && !aligned(drop->step_dev, 4)))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const int64_t rpb = relu_rows_per_block(M);
  const int64_t n_blocks = (M + rpb - 1) / rpb;
  const size_t need = sizeof(float) * static_cast<size_t>(n_blocks) * K;
  if (workspace == nullptr || workspace_bytes < need)  // the kernel always writes partials
    return fail(GCG_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  if (!aligned(workspace, 4)) return fail(GCG_ERR_MISALIGNED, "%s: workspace alignment", fn);
  float* part = static_cast<float*>(workspace);
  const bool vec = ldg % 4 == 0 && aligned(gY, 16) &&
                   (!store || (ldo % 4 == 0 && aligned(g_out, 16))) &&
                   (!use_y || (ldy % 4 == 0 && aligned(Y, 16)));
  if (!vec && K > 64 * kReluMaxK4)
    return fail(GCG_ERR_MISALIGNED, "%s: K > %d needs 16-B rows (ld %% 4 == 0)", fn,
                64 * kReluMaxK4);
  const dim3 grid(static_cast<unsigned>(n_blocks));
#define GCG_PASS_LAUNCH(V, MK)                                                                  \
  if (drop != nullptr)                                                                          \
    hipLaunchKernelGGL((dropout_relu_backward_kernel<V, MK == kMaskGate>), grid, dim3(256), 0,  \
                       st, M, int(K), rpb, gY, ldg, g_out, ldo, part, gate, ldgate, drop->key,  \
                       drop->step_dev, drop->row0);                                             \
  else                                                                                          \
    hipLaunchKernelGGL((relu_backward_kernel<V, MK != kMaskNone, MK == kMaskGate>), grid,       \
                       dim3(256), 0, st, M, int(K), rpb, gY, ldg, Y, ldy, g_out, ldo, part,     \
                       gate, ldgate)
  if (vec) {
    if (mask == kMaskGate) { GCG_PASS_LAUNCH(4, kMaskGate); }
    else if (mask == kMaskY) { GCG_PASS_LAUNCH(4, kMaskY); }
    else { GCG_PASS_LAUNCH(4, kMaskNone); }
  } else {
    if (mask == kMaskGate) { GCG_PASS_LAUNCH(1, kMaskGate); }
    else if (mask == kMaskY) { GCG_PASS_LAUNCH(1, kMaskY); }
    else { GCG_PASS_LAUNCH(1, kMaskNone); }
  }
#undef GCG_PASS_LAUNCH
  GCG_HIP_CHECK(hipGetLastError());
  if (bias_grad != nullptr) {
    hipLaunchKernelGGL(column_sum_kernel, dim3(static_cast<unsigned>((K + 63) / 64)), dim3(1024),
                       0, st, n_blocks, int(K), part, bias_grad);
    GCG_HIP_CHECK(hipGetLastError());
  }
  return GCG_OK;
}

// The host side of the pass in slabs (gcg_rectify_backward_wide_f32): rectify_backward's checks
// without the K cap and without Y, one launch with the slab in gridDim.y, then column_sum_kernel
// on every slab's partials.
gcg_status rectify_backward_wide(const char* fn, const DropArgs* drop, int64_t M, int64_t K,
                                 const float* gY, int64_t ldg, const uint8_t* gate,
                                 int64_t ldgate, float* g_out, int64_t ldo, float* bias_grad,
                                 void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  // (at most 65535 slabs: gridDim.y)
  if (M < 0 || K < 0 || K > int64_t{65535} * kReluSlab || (drop != nullptr && drop->row0 < 0))
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes M=%lld K=%lld", fn,
                static_cast<long long>(M), static_cast<long long>(K));
  if (gate == nullptr && drop == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: neither gate nor dropout (gcg_column_sum_f32 sums)", fn);
  auto st = static_cast<hipStream_t>(stream);
  if (M == 0 || K == 0) {  // an empty sum is zero
    if (bias_grad != nullptr && K > 0)
      GCG_HIP_CHECK(hipMemsetAsync(bias_grad, 0, sizeof(float) * K, st));
    return GCG_OK;
  }
  if (gY == nullptr || g_out == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: null operand", fn);
  if (ldg < K || ldo < K) return fail(GCG_ERR_INVALID_ARG, "%s: ld < K", fn);
  if (gate != nullptr && (ldgate < K || ldgate % 4 != 0 || !aligned(gate, 4)))
    return fail(GCG_ERR_MISALIGNED, "%s: gate needs ldgate >= K, ldgate %% 4 == 0, 4-B base", fn);
  if (!aligned(gY, 4) || !aligned(g_out, 4) || (drop != nullptr && !aligned(drop->step_dev, 4)))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const int64_t rpb = relu_rows_per_block(M);
  const int64_t n_blocks = (M + rpb - 1) / rpb;
  const size_t need = sizeof(float) * static_cast<size_t>(n_blocks) * K;
  if (workspace == nullptr || workspace_bytes < need)  // the kernel always writes partials
    return fail(GCG_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  if (!aligned(workspace, 4)) return fail(GCG_ERR_MISALIGNED, "%s: workspace alignment", fn);
  float* part = static_cast<float*>(workspace);
  const bool vec = ldg % 4 == 0 && aligned(gY, 16) && ldo % 4 == 0 && aligned(g_out, 16);
  if (!vec && K > 64 * kReluMaxK4)
    return fail(GCG_ERR_MISALIGNED, "%s: K > %d needs 16-B rows (ld %% 4 == 0)", fn,
                64 * kReluMaxK4);
  const int64_t slabs = (K + kReluSlab - 1) / kReluSlab;
  const dim3 grid(static_cast<unsigned>(n_blocks), static_cast<unsigned>(slabs));
  const DropKey key = drop != nullptr ? drop->key : DropKey{};
  const int32_t* step_dev = drop != nullptr ? drop->step_dev : nullptr;
  const int64_t row0 = drop != nullptr ? drop->row0 : 0;
#define GCG_WIDE_LAUNCH(V, D, G)                                                                \
  hipLaunchKernelGGL((rectify_backward_wide_kernel<V, D, G>), grid, dim3(256), 0, st, M,        \
                     int(K), rpb, gY, ldg, g_out, ldo, part, gate, ldgate, key, step_dev, row0)
  const bool has_gate = gate != nullptr;
  if (vec) {
    if (drop == nullptr) { GCG_WIDE_LAUNCH(4, false, true); }
    else if (has_gate) { GCG_WIDE_LAUNCH(4, true, true); }
    else { GCG_WIDE_LAUNCH(4, true, false); }
  } else {
    if (drop == nullptr) { GCG_WIDE_LAUNCH(1, false, true); }
    else if (has_gate) { GCG_WIDE_LAUNCH(1, true, true); }
    else { GCG_WIDE_LAUNCH(1, true, false); }
  }
#undef GCG_WIDE_LAUNCH
  GCG_HIP_CHECK(hipGetLastError());
  if (bias_grad != nullptr)
    for (int64_t s = 0; s < slabs; ++s) {
      const int64_t c0 = s * kReluSlab, ks = std::min<int64_t>(kReluSlab, K - c0);
      hipLaunchKernelGGL(column_sum_kernel, dim3(static_cast<unsigned>((ks + 63) / 64)),
                         dim3(1024), 0, st, n_blocks, int(ks), part + n_blocks * c0,
                         bias_grad + c0);
      GCG_HIP_CHECK(hipGetLastError());
    }
  return GCG_OK;
}

}  // namespace

gcg_status gcg_rectify_backward_wide_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                         const uint8_t* gate, int64_t ldgate, float* g_out,
                                         int64_t ldo, float* bias_grad, void* workspace,
                                         size_t workspace_bytes, uint32_t threshold, float scale,
                                         uint64_t seed, const int32_t* step_dev,
                                         uint32_t stream_id, int64_t row0, gcg_stream_t stream) {
  const DropArgs drop{{static_cast<uint32_t>(seed & 0xffffffffu),
                       static_cast<uint32_t>(seed >> 32), 0u, stream_id, threshold, scale},
                      step_dev, row0};
  return rectify_backward_wide("gcg_rectify_backward_wide_f32",
                               step_dev != nullptr ? &drop : nullptr, M, K, gY, ldg, gate, ldgate,
                               g_out, ldo, bias_grad, workspace, workspace_bytes, stream);
}

gcg_status gcg_relu_backward_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                 const float* Y, int64_t ldy, float* g_out, int64_t ldo,
                                 float* bias_grad, void* workspace, size_t workspace_bytes,
                                 gcg_stream_t stream) {
  return rectify_backward("gcg_relu_backward_f32", kMaskY, nullptr, M, K, gY, ldg, Y, ldy, nullptr,
                          0, g_out, ldo, bias_grad, workspace, workspace_bytes, stream);
}

gcg_status gcg_relu_backward_gate_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                      const uint8_t* gate, int64_t ldgate, float* g_out,
                                      int64_t ldo, float* bias_grad, void* workspace,
                                      size_t workspace_bytes, gcg_stream_t stream) {
  if (M > 0 && K > 0 && gate == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_relu_backward_gate_f32: gate is NULL");
  return rectify_backward("gcg_relu_backward_gate_f32", kMaskGate, nullptr, M, K, gY, ldg, nullptr,
                          0, gate, ldgate, g_out, ldo, bias_grad, workspace, workspace_bytes,
                          stream);
}

gcg_status gcg_dropout_relu_backward_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                         const uint8_t* gate, int64_t ldgate, float* g_out,
                                         int64_t ldo, float* bias_grad, void* workspace,
                                         size_t workspace_bytes, uint32_t threshold, float scale,
                                         uint64_t seed, const int32_t* step_dev,
                                         uint32_t stream_id, int64_t row0, gcg_stream_t stream) {
  const DropArgs drop{{static_cast<uint32_t>(seed & 0xffffffffu),
                       static_cast<uint32_t>(seed >> 32), 0u, stream_id, threshold, scale},
                      step_dev, row0};
  return rectify_backward("gcg_dropout_relu_backward_f32", gate != nullptr ? kMaskGate : kMaskNone,
                          &drop, M, K, gY, ldg, nullptr, 0, gate, ldgate, g_out, ldo, bias_grad,
                          workspace, workspace_bytes, stream);
}

gcg_status gcg_column_sum_f32(int64_t M, int64_t K, const float* X, int64_t ldx, float* out,
                              void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  return rectify_backward("gcg_column_sum_f32", kMaskNone, nullptr, M, K, X, ldx, nullptr, 0,
                          nullptr, 0, nullptr, 0, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
