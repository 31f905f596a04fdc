// vocab_stats.hip -- what the analyses of the location-to-language model need of a chunk of
// logits (reference loc2lang.py:516-614, 755-766): the row log-sum-exp, and per word the two
// column sums S = sum_n p and T = sum_n p log p of p = softmax(z), from which the entropy of the
// l1-normalised column is log S - T / S. The n x V probabilities are never written.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "row_maxsum.h"

using namespace gcg;

namespace {

constexpr int64_t kMaxCols = int64_t{1} << 24;
constexpr int kRows = 8;  // rows of a column whose loads are in flight together

// One workgroup of 256 threads per row (rows blockIdx.x, + gridDim.x, ...): the float32
// (max, sum) fold of softmax_xent_csr_kernel's first pass, then the log and the add in double.
__global__ __launch_bounds__(kBlock) void row_lse_kernel(int64_t M, int N, const float* logits,
                                                         int64_t ldl, double* __restrict__ lse) {
  __shared__ float red_m[kWavesPerBlock], red_s[kWavesPerBlock];
  for (int64_t i = blockIdx.x; i < M; i += gridDim.x) {
    const float* z = logits + i * ldl;
    const bool vec = (reinterpret_cast<uintptr_t>(z) & 15) == 0;
    const MaxSum row = block_row_maxsum(z, N, vec, red_m, red_s);
    if (threadIdx.x == 0) lse[i] = static_cast<double>(row.m) + log(static_cast<double>(row.s));
    __syncthreads();  // the slots are rewritten for the next row
  }
}

// One row's term of a column: a = z - lse, p = exp(a); S += p, T += p a (0 when p == 0: a logit
// of -inf, or an underflow, is 0 log 0 = 0).
__device__ __forceinline__ void add_row(float z, double lse, double& S, double& T) {
  const double a = static_cast<double>(z) - lse;
  const double p = exp(a);
  S = S + p;
  T = T + (p > 0.0 ? p * a : 0.0);
}

// One thread per column, one wave per workgroup (64 consecutive columns: a 256-B segment of every
// row). The thread takes the rows 0 .. M - 1 one at a time, in row order, onto the running S[j]
// and T[j] it read at the start; so rows split over consecutive calls give the bits of one call.
// kRows rows are loaded ahead of the kRows being added (the exponentials are independent, the
// adds are in order); lse[i] is uniform over the wave.
__global__ __launch_bounds__(kWave) void softmax_column_stats_kernel(
    int64_t M, int N, const float* __restrict__ logits, int64_t ldl,
    const double* __restrict__ lse, double* __restrict__ S, double* __restrict__ T) {
  const int j = blockIdx.x * kWave + threadIdx.x;
  if (j >= N) return;
  const float* z = logits + j;
  double s = S[j], t = T[j];
  float cur[kRows] = {}, nxt[kRows] = {};
  const int64_t whole = M / kRows * kRows;
  if (whole > 0) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) cur[r] = z[r * ldl];
  }
  for (int64_t i = 0; i < whole; i += kRows) {
    if (i + kRows < whole) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) nxt[r] = z[(i + kRows + r) * ldl];
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) add_row(cur[r], lse[i + r], s, t);
#pragma unroll
    for (int r = 0; r < kRows; ++r) cur[r] = nxt[r];
  }
  for (int64_t i = whole; i < M; ++i) add_row(z[i * ldl], lse[i], s, t);
  S[j] = s;
  T[j] = t;
}

gcg_status check_logits(const char* fn, int64_t M, int64_t N, int64_t ldl) {
  if (M < 0 || M > INT32_MAX || N < 1 || N > kMaxCols)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes M=%lld N=%lld (1 <= N <= 2^24)", fn,
                static_cast<long long>(M), static_cast<long long>(N));
  if (ldl < N)
    return fail(GCG_ERR_INVALID_ARG, "%s: row stride below N = %lld", fn,
                static_cast<long long>(N));
  return GCG_OK;
}

}  // namespace

extern "C" {

gcg_status gcg_row_lse_f64(int64_t M, int64_t N, const float* logits, int64_t ldl, double* lse,
                           gcg_stream_t stream) {
  const char* fn = "gcg_row_lse_f64";
  if (const gcg_status st = check_logits(fn, M, N, ldl)) return st;
  if (M == 0) return GCG_OK;
  if (logits == nullptr || lse == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL logits or lse", fn);
  if (!aligned(logits, 4) || !aligned(lse, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: logits not 4-B or lse not 8-B aligned", fn);
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(M, int64_t{1} << 20));
  hipLaunchKernelGGL(row_lse_kernel, dim3(grid), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), M, static_cast<int>(N), logits, ldl, lse);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_softmax_column_stats_f64(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                        const double* lse, double* S, double* T,
                                        gcg_stream_t stream) {
  const char* fn = "gcg_softmax_column_stats_f64";
  if (const gcg_status st = check_logits(fn, M, N, ldl)) return st;
  if (M == 0) return GCG_OK;
  if (logits == nullptr || lse == nullptr || S == nullptr || T == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL logits, lse, S or T", fn);
  if (!aligned(logits, 4) || !aligned(lse, 8) || !aligned(S, 8) || !aligned(T, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: logits not 4-B or lse, S, T not 8-B aligned", fn);
  const unsigned grid = static_cast<unsigned>((N + kWave - 1) / kWave);
  hipLaunchKernelGGL(softmax_column_stats_kernel, dim3(grid), dim3(kWave), 0,
                     static_cast<hipStream_t>(stream), M, static_cast<int>(N), logits, ldl, lse, S,
                     T);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
