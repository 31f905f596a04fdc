// neighbours.hip -- the dialect-embedding evaluation of main.py (eval_embeddings 364-384,
// nearest_neighbours 108-162, recall_at_k 230-281) on resident float32 embeddings
// (include/gcg_spmm.h): the min-max + l1 preprocessing, the rank of every gold word in its
// query's full ordering of the V words, and an exact kneighbors for k <= 1024.
//
// One distance, one order. d2(q, e) is dist2_step applied to j = 0, 1, ..., D - 1 in that
// order on one float32 accumulator that starts at +0: a subtraction rounded once (dist2_diff)
// and one fused multiply-add (dist2_add). Every kernel below computes a (query, row) pair
// through these in that order (columns past D are staged as zeros: fma(0, 0, acc) == acc, bit
// for bit), so a pair has the same bits wherever it is computed. Words are ordered by
// dist2_key: (d2, row) ascending. d2 >= +0, so its float bits order as an unsigned integer and
// the pair packs into one uint64. Counts are integers (integer atomics are order-free); nothing
// here depends on the grid.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cmath>

#include "scratch.h"
#include "segment_kernels.h"

using namespace gcg;

namespace {

constexpr int kRowTile = 256;              // rows of E per workgroup: one per thread
constexpr int kColChunk = 32;              // columns staged through LDS per step (128 B a row)
constexpr int kRowPitch = kColChunk + 4;   // floats; 9 16-B slots: ds_read_b128 conflict-free
constexpr int kQueryTile = 32;             // queries per workgroup (Q > kQueryTileSmall)
constexpr int kQueryTileSmall = 8;         // ... for Q <= 8; queries sorted at a time in kneighbors
constexpr int kSlotCap = 2048;             // pairs of a query tile counted in LDS; more: in HBM
constexpr int kMaxK = 1024;                // kneighbors' largest k
constexpr int kMergeBuf = 2 * kMaxK;       // the merge's LDS buffer: [running top | new chunk]
constexpr int kMergeSlice = 8 * kMaxK;     // candidates per first-level merge workgroup ...
constexpr int kMergeSplitMax = 64;         // ... of at most this many per query
constexpr int kMinMaxCols = 64;            // columns per workgroup of the column min/max
constexpr int kMinMaxRows = 1024;          // rows per workgroup of the column min/max
constexpr uint64_t kNoKey = ~uint64_t{0};  // sorts after every (d2, row)

// ---- the one definition of a squared distance and of the order ---------------------------
__device__ __forceinline__ float dist2_diff(float q, float e) { return q - e; }
__device__ __forceinline__ float dist2_add(float acc, float d) { return __fmaf_rn(d, d, acc); }
__device__ __forceinline__ float dist2_step(float acc, float q, float e) {
  return dist2_add(acc, dist2_diff(q, e));
}

__device__ __forceinline__ uint64_t dist2_key(float d2, int64_t row) {
  return (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | static_cast<uint32_t>(row);
}

__device__ __forceinline__ bool finite4(float4 v) {
  return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
}

// acc[i] = d2(query q0 + i, row v0 + threadIdx.x) for i < TQ. The rows' columns pass through
// LDS in chunks of 32 (coalesced 16-B loads when `vec`: 16-B aligned bases and strides a
// multiple of 4; the next chunk is loaded into registers while this one is computed); a thread
// reads its own row as 16-B slots and the queries as broadcasts. Rows past V and queries past Q
// are zeros (their results are not used). *status = 1 for a non-finite element.
template <int TQ>
__device__ __forceinline__ void tile_dist2(int64_t V, int64_t D, const float* __restrict__ E,
                                           int64_t lde, int64_t v0, int64_t Q,
                                           const float* __restrict__ Qm, int64_t ldq, int64_t q0,
                                           bool vec, float* s_e, float* s_q, float (&acc)[TQ],
                                           int32_t* status) {
  constexpr int kEPer = kRowTile * kColChunk / 4 / 256;    // float4 per thread per chunk: 8
  constexpr int kQPer = (TQ * kColChunk + 255) / 256;      // floats per thread per chunk
  const int t = threadIdx.x;
  float4 re[kEPer];
  float rq[kQPer];
  bool bad = false;

  auto fetch = [&](int64_t c0) {
#pragma unroll
    for (int i = 0; i < kEPer; ++i) {
      const int idx = t + 256 * i, r = idx >> 3, c4 = idx & 7;
      const int64_t row = v0 + r, col = c0 + 4 * c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < V && col < D) {
        const float* p = E + row * lde + col;
        if (vec && col + 3 < D) {
          v = *reinterpret_cast<const float4*>(p);
        } else {
          v.x = p[0];
          if (col + 1 < D) v.y = p[1];
          if (col + 2 < D) v.z = p[2];
          if (col + 3 < D) v.w = p[3];
        }
      }
      bad |= !finite4(v);
      re[i] = v;
    }
#pragma unroll
    for (int i = 0; i < kQPer; ++i) {
      const int idx = t + 256 * i, qi = idx / kColChunk, c = idx % kColChunk;
      float v = 0.f;
      if (qi < TQ && q0 + qi < Q && c0 + c < D) v = Qm[(q0 + qi) * ldq + c0 + c];
      bad |= !isfinite(v);
      rq[i] = v;
    }
  };

#pragma unroll
  for (int i = 0; i < TQ; ++i) acc[i] = 0.f;
  fetch(0);
  for (int64_t c0 = 0; c0 < D; c0 += kColChunk) {
    __syncthreads();  // the chunk before is consumed
#pragma unroll
    for (int i = 0; i < kEPer; ++i) {
      const int idx = t + 256 * i, r = idx >> 3, c4 = idx & 7;
      *reinterpret_cast<float4*>(s_e + r * kRowPitch + 4 * c4) = re[i];
    }
#pragma unroll
    for (int i = 0; i < kQPer; ++i) {
      const int idx = t + 256 * i;
      if (idx < TQ * kColChunk) s_q[idx] = rq[i];
    }
    __syncthreads();
    if (c0 + kColChunk < D) fetch(c0 + kColChunk);
#pragma unroll 2
    for (int c4 = 0; c4 < kColChunk / 4; ++c4) {
      const float4 e = *reinterpret_cast<const float4*>(s_e + t * kRowPitch + 4 * c4);
#pragma unroll
      for (int i = 0; i < TQ; ++i) {
        const float4 q = *reinterpret_cast<const float4*>(s_q + i * kColChunk + 4 * c4);
        float a = acc[i];
        a = dist2_step(a, q.x, e.x);
        a = dist2_step(a, q.y, e.y);
        a = dist2_step(a, q.z, e.z);
        a = dist2_step(a, q.w, e.w);
        acc[i] = a;
      }
    }
  }
  if (bad) *status = 1;
}

// ---- sorting in LDS -----------------------------------------------------------------------
// Sorts every aligned block of n keys of a[0 .. total) ascending (n, total powers of two,
// n <= total): the bitonic network whose first step of a merge mirrors, so every block ascends.
__device__ __forceinline__ void cmpx(uint64_t* a, int i, int j) {
  const uint64_t x = a[i], y = a[j];
  if (y < x) {
    a[i] = y;
    a[j] = x;
  }
}

__device__ void bitonic_blocks(uint64_t* a, int total, int n) {
  const int half = total / 2;
  for (int k = 2; k <= n; k <<= 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < half; i += 256) {
      const int h = k >> 1, blk = i / h, off = i % h;
      cmpx(a, blk * k + off, blk * k + k - 1 - off);
    }
    for (int j = k >> 2; j >= 1; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < half; i += 256) cmpx(a, (i / j) * 2 * j + i % j, (i / j) * 2 * j + i % j + j);
    }
  }
  __syncthreads();
}

// ---- the preprocessing: MinMaxScaler(0, 1), then l1 rows -----------------------------------
// Workgroup (cx, ry) owns columns [64 cx, 64 cx + 64) of rows [1024 ry, 1024 ry + 1024): thread
// (c = t % 64, g = t / 64) folds rows g, g + 4, ... in ascending order, then the four groups in
// ascending g. pmin / pmax[ry * D + col].
__global__ __launch_bounds__(256) void colminmax_partial_kernel(
    int64_t V, int64_t D, const float* __restrict__ E, int64_t lde, float* __restrict__ pmin,
    float* __restrict__ pmax, int32_t* __restrict__ status) {
  __shared__ float s_lo[256], s_hi[256];
  const int t = threadIdx.x, c = t % kMinMaxCols, g = t / kMinMaxCols;
  const int64_t col = static_cast<int64_t>(blockIdx.x) * kMinMaxCols + c;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * kMinMaxRows;
  const int64_t r1 = min(r0 + kMinMaxRows, V);
  float lo = INFINITY, hi = -INFINITY;
  bool bad = false;
  if (col < D) {
    for (int64_t r = r0 + g; r < r1; r += 256 / kMinMaxCols) {
      const float x = E[r * lde + col];
      bad |= !isfinite(x);
      lo = fminf(lo, x);
      hi = fmaxf(hi, x);
    }
  }
  if (bad) *status = 1;
  s_lo[t] = lo;
  s_hi[t] = hi;
  __syncthreads();
  if (g == 0 && col < D) {
    for (int k = 1; k < 256 / kMinMaxCols; ++k) {
      lo = fminf(lo, s_lo[t + k * kMinMaxCols]);
      hi = fmaxf(hi, s_hi[t + k * kMinMaxCols]);
    }
    pmin[static_cast<int64_t>(blockIdx.y) * D + col] = lo;
    pmax[static_cast<int64_t>(blockIdx.y) * D + col] = hi;
  }
}

// One thread per column: the partials in ascending row block, then sklearn's arithmetic in
// float64: scale = 1 / (max - min) (1 where max == min), offset = 0 - min * scale.
__global__ void colscale_kernel(int64_t D, int64_t nblocks, const float* __restrict__ pmin,
                                const float* __restrict__ pmax, double* __restrict__ scale,
                                double* __restrict__ offset) {
  for (int64_t col = grid_start(); col < D; col += grid_stride()) {
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t b = 0; b < nblocks; ++b) {
      lo = fminf(lo, pmin[b * D + col]);
      hi = fmaxf(hi, pmax[b * D + col]);
    }
    const double range = static_cast<double>(hi) - static_cast<double>(lo);
    const double s = range == 0.0 ? 1.0 : 1.0 / range;
    scale[col] = s;
    offset[col] = 0.0 - static_cast<double>(lo) * s;
  }
}

// One wave per row, twice over it: y_j = x_j * scale_j + offset_j in float64; lane l adds
// |y_j| for j = l, l + 64, ... in ascending order, the lanes fold in the fixed butterfly
// l ^ 32, 16, ..., 1; then out_j = float(y_j / sum), or float(y_j) when the sum is 0.
__global__ __launch_bounds__(256) void scale_l1_rows_kernel(
    int64_t V, int64_t D, const float* __restrict__ E, int64_t lde,
    const double* __restrict__ scale, const double* __restrict__ offset, float* __restrict__ out,
    int64_t ldo) {
  const int lane = threadIdx.x % kWave;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) / kWave;
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (256 / kWave);
  for (int64_t r = wave; r < V; r += nwaves) {
    const float* x = E + r * lde;
    double sum = 0.0;
    for (int64_t j = lane; j < D; j += kWave)
      sum += fabs(static_cast<double>(x[j]) * scale[j] + offset[j]);
    sum = wave_sum(sum);
    float* y = out + r * ldo;
    for (int64_t j = lane; j < D; j += kWave) {
      const double v = static_cast<double>(x[j]) * scale[j] + offset[j];
      y[j] = static_cast<float>(sum == 0.0 ? v : v / sum);
    }
  }
}

// ---- the ranks ------------------------------------------------------------------------------
// pair_ptr must be 0 = ptr[0] <= ptr[1] <= ... <= ptr[Q] = P; a violation raises *status = 3.
__global__ void pair_ptr_check_kernel(int64_t Q, int64_t P, const int32_t* __restrict__ ptr,
                                      int32_t* __restrict__ status) {
  for (int64_t q = grid_start(); q <= Q; q += grid_stride()) {
    const int64_t a = ptr[q];
    bool ok = a >= 0 && a <= P;
    if (q == 0) ok = ok && a == 0;
    if (q == Q) ok = ok && a == P;
    if (q < Q) ok = ok && a <= ptr[q + 1];
    if (!ok) atomicMax(status, 3);
  }
}

// sptr = ptr where it passed the check, else all zeros (every segment empty): nothing after
// this reads outside [0, P). pair_q[p] = the query of pair p.
__global__ void pair_ptr_expand_kernel(int64_t Q, const int32_t* __restrict__ ptr,
                                       const int32_t* __restrict__ status,
                                       int32_t* __restrict__ sptr, int32_t* __restrict__ pair_q) {
  const bool ok = *status != 3;
  for (int64_t q = grid_start(); q <= Q; q += grid_stride()) {
    sptr[q] = ok ? ptr[q] : 0;
    if (ok && q < Q)
      for (int64_t p = ptr[q]; p < ptr[q + 1]; ++p) pair_q[p] = static_cast<int32_t>(q);
  }
}

// key[p] = dist2_key(d2(q_p, w_p), w_p): one wave per pair. The lanes load 64 columns at a
// time and take their differences; every lane then runs the one chain of fused multiply-adds
// over them in ascending column order (a lane past D holds 0: fma(0, 0, acc) == acc). A word
// outside [0, V) raises *status = 2 and a non-finite distance 1; both sort last.
__global__ __launch_bounds__(256) void pair_threshold_kernel(
    int64_t V, int64_t D, const float* __restrict__ E, int64_t lde, const float* __restrict__ Qm,
    int64_t ldq, int64_t P, const int32_t* __restrict__ pair_q,
    const int32_t* __restrict__ pair_word, uint64_t* __restrict__ key,
    int32_t* __restrict__ status) {
  const int lane = threadIdx.x % kWave;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) / kWave;
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (256 / kWave);
  for (int64_t p = wave; p < P; p += nwaves) {  // uniform over the wave
    const int64_t q = pair_q[p], w = pair_word[p];
    uint64_t k = kNoKey;
    int32_t raise = 0;
    if (q >= 0) {  // q < 0: pair_ptr failed its check
      if (w < 0 || w >= V) {
        raise = 2;
      } else {
        const float* x = Qm + q * ldq;
        const float* e = E + w * lde;
        float acc = 0.f;
        for (int64_t j0 = 0; j0 < D; j0 += kWave) {
          const int64_t j = j0 + lane;
          const float d = j < D ? dist2_diff(x[j], e[j]) : 0.f;
#pragma unroll
          for (int l = 0; l < kWave; ++l) {
            const float dl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), l));
            acc = dist2_add(acc, dl);
          }
        }
        if (isfinite(acc)) k = dist2_key(acc, w);
        else raise = 1;
      }
    }
    if (lane == 0) {
      key[p] = k;
      if (raise != 0) atomicMax(status, raise);
    }
  }
}

__global__ void iota_kernel(int64_t n, int32_t* __restrict__ out) {
  for (int64_t i = grid_start(); i < n; i += grid_stride()) out[i] = static_cast<int32_t>(i);
}

// Workgroup (x, y) owns rows [256 x, 256 x + 256) and queries [TQ y, TQ y + TQ). skey holds
// every query's thresholds ascending (segment [sptr[q], sptr[q + 1])). A row with key x adds 1
// to slot i = the first threshold of its query above x, when there is one: the rank of the
// threshold at sorted position i is then the sum of slots [sptr[q], i]. A tile with at most
// kSlotCap pairs copies its thresholds into LDS (the rows' staging buffer, free by then), counts
// in LDS and adds its non-zero slots to `slot` at the end; a larger one searches skey and adds
// to `slot` directly.
template <int TQ>
__global__ __launch_bounds__(256) void neighbour_count_kernel(
    int64_t V, int64_t D, const float* __restrict__ E, int64_t lde, int64_t Q,
    const float* __restrict__ Qm, int64_t ldq, bool vec, const int32_t* __restrict__ sptr,
    const uint64_t* __restrict__ skey, int32_t* __restrict__ slot, int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) float s_e[kRowTile * kRowPitch];
  __shared__ __attribute__((aligned(16))) float s_q[TQ * kColChunk];
  __shared__ int32_t s_cnt[kSlotCap];
  __shared__ int32_t s_ptr[TQ + 1];
  __shared__ uint64_t s_max[TQ];
  const int t = threadIdx.x;
  const int64_t v0 = static_cast<int64_t>(blockIdx.x) * kRowTile;
  const int64_t q0 = static_cast<int64_t>(blockIdx.y) * TQ;
  const int nq = static_cast<int>(min(static_cast<int64_t>(TQ), Q - q0));
  const int32_t s0 = sptr[q0], s1 = sptr[q0 + nq];
  if (s1 == s0) return;  // no pair in this query tile (uniform)
  const bool in_lds = s1 - s0 <= kSlotCap;
  if (t <= TQ) s_ptr[t] = sptr[q0 + min(t, nq)];
  if (t < nq) {
    const int32_t a = sptr[q0 + t], b = sptr[q0 + t + 1];
    s_max[t] = b > a ? skey[b - 1] : 0;
  }
  if (in_lds)
    for (int i = t; i < s1 - s0; i += 256) s_cnt[i] = 0;
  float acc[TQ];
  tile_dist2<TQ>(V, D, E, lde, v0, Q, Qm, ldq, q0, vec, s_e, s_q, acc, status);  // syncs inside
  // the rows' staging buffer is free now: a tile that counts in LDS searches its keys there too
  static_assert(kSlotCap * sizeof(uint64_t) <= kRowTile * kRowPitch * sizeof(float), "keys fit");
  uint64_t* s_key = reinterpret_cast<uint64_t*>(s_e);
  if (in_lds) {
    __syncthreads();
    for (int i = t; i < s1 - s0; i += 256) s_key[i] = skey[s0 + i];
    __syncthreads();
  }
  const int64_t v = v0 + t;
  if (v < V) {
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      if (i >= nq) break;
      int32_t lo = s_ptr[i], hi = s_ptr[i + 1];
      if (hi == lo) continue;
      const uint64_t x = dist2_key(acc[i], v);
      if (!(x < s_max[i])) continue;  // above every threshold of this query
      while (lo < hi) {               // the first position whose key is > x
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((in_lds ? s_key[mid - s0] : skey[mid]) > x) hi = mid;
        else lo = mid + 1;
      }
      if (in_lds) atomicAdd(&s_cnt[lo - s0], 1);
      else atomicAdd(&slot[lo], 1);
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int i = t; i < s1 - s0; i += 256) {
      const int32_t c = s_cnt[i];
      if (c != 0) atomicAdd(&slot[s0 + i], c);
    }
  }
}

// One workgroup per query: rank[sperm[i]] = slot[sptr[q]] + ... + slot[i], in chunks of 256
// (an inclusive scan in LDS and a carry).
__global__ __launch_bounds__(256) void slot_scan_kernel(int64_t Q, const int32_t* __restrict__ sptr,
                                                        const int32_t* __restrict__ slot,
                                                        const int32_t* __restrict__ sperm,
                                                        int32_t* __restrict__ rank) {
  __shared__ int32_t s[256];
  const int t = threadIdx.x;
  for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
    const int32_t a = sptr[q], b = sptr[q + 1];
    int32_t carry = 0;
    for (int32_t base = a; base < b; base += 256) {
      const int32_t i = base + t;
      __syncthreads();
      s[t] = i < b ? slot[i] : 0;
      __syncthreads();
      for (int h = 1; h < 256; h <<= 1) {
        const int32_t add = t >= h ? s[t - h] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
      }
      if (i < b) rank[sperm[i]] = carry + s[t];
      carry += s[255];
    }
  }
}

// ---- kneighbors -----------------------------------------------------------------------------
// Workgroup (x, y): the keys of rows [256 x, 256 x + 256) for queries [TQ y, TQ y + TQ), eight
// queries at a time: each query's 256 keys sorted in LDS, the first kk = min(k, 256) go to
// cand[(q * ntiles + x) * kk ..]. Rows past V carry kNoKey.
template <int TQ>
__global__ __launch_bounds__(256) void knn_tile_kernel(
    int64_t V, int64_t D, const float* __restrict__ E, int64_t lde, int64_t Q,
    const float* __restrict__ Qm, int64_t ldq, bool vec, int kk, uint64_t* __restrict__ cand,
    int32_t* __restrict__ status) {
  constexpr int kGroup = kQueryTileSmall;
  __shared__ __attribute__((aligned(16))) float s_e[kRowTile * kRowPitch];
  __shared__ __attribute__((aligned(16))) float s_q[TQ * kColChunk];
  __shared__ uint64_t s_key[kGroup * kRowTile];
  const int t = threadIdx.x;
  const int64_t v0 = static_cast<int64_t>(blockIdx.x) * kRowTile;
  const int64_t q0 = static_cast<int64_t>(blockIdx.y) * TQ;
  float acc[TQ];
  tile_dist2<TQ>(V, D, E, lde, v0, Q, Qm, ldq, q0, vec, s_e, s_q, acc, status);
  const int64_t v = v0 + t;
#pragma unroll
  for (int g = 0; g < TQ; g += kGroup) {
    if (q0 + g >= Q) break;  // uniform
#pragma unroll
    for (int i = 0; i < kGroup; ++i)
      s_key[i * kRowTile + t] = v < V ? dist2_key(acc[g + i], v) : kNoKey;
    bitonic_blocks(s_key, kGroup * kRowTile, kRowTile);
    for (int i = 0; i < kGroup && q0 + g + i < Q; ++i)
      for (int r = t; r < kk; r += 256)
        cand[((q0 + g + i) * gridDim.x + blockIdx.x) * kk + r] = s_key[i * kRowTile + r];
    __syncthreads();  // the keys are read before the next group overwrites them
  }
}

// Workgroup (q, s): the k smallest, ascending, of slice s of query q's ncand candidates (nsplit
// slices of `per` keys). The LDS buffer holds the running 1024 smallest in front and the next
// 1024 candidates behind; one sort of the 2048 per chunk. With out_key the k keys go to
// out_key[(q * nsplit + s) * k ..] (the first level of two); without, to dist2 / index.
__global__ __launch_bounds__(256) void knn_merge_kernel(int64_t ncand, int64_t per, int k,
                                                        const uint64_t* __restrict__ cand,
                                                        uint64_t* __restrict__ out_key,
                                                        float* __restrict__ dist2,
                                                        int32_t* __restrict__ index) {
  __shared__ uint64_t s[kMergeBuf];
  const int t = threadIdx.x;
  const int64_t q = blockIdx.x;
  const uint64_t* c = cand + q * ncand;
  const int64_t lo = static_cast<int64_t>(blockIdx.y) * per, hi = min(ncand, lo + per);
  for (int i = t; i < kMaxK; i += 256) s[i] = kNoKey;
  for (int64_t base = lo; base < hi; base += kMaxK) {
    for (int i = t; i < kMaxK; i += 256) s[kMaxK + i] = base + i < hi ? c[base + i] : kNoKey;
    bitonic_blocks(s, kMergeBuf, kMergeBuf);
  }
  __syncthreads();
  for (int r = t; r < k; r += 256) {
    if (out_key != nullptr) {
      out_key[(q * gridDim.y + blockIdx.y) * k + r] = s[r];
    } else {
      dist2[q * k + r] = __uint_as_float(static_cast<uint32_t>(s[r] >> 32));
      index[q * k + r] = static_cast<int32_t>(static_cast<uint32_t>(s[r]));
    }
  }
}

// ---- host side --------------------------------------------------------------------------------
constexpr int64_t kMaxRows = INT32_MAX - 1;
constexpr int64_t kMaxQueries = int64_t{65535} * kQueryTileSmall;  // grid.y

int64_t minmax_blocks(int64_t V) { return (V + kMinMaxRows - 1) / kMinMaxRows; }
int64_t row_tiles(int64_t V) { return (V + kRowTile - 1) / kRowTile; }
// slices of a query's ncand candidates in the first of two merge levels (1: one level)
int64_t merge_splits(int64_t ncand) {
  return std::min<int64_t>(kMergeSplitMax, (ncand + kMergeSlice - 1) / kMergeSlice);
}

struct RankSpace {
  int32_t *sptr, *pair_q, *iota, *sperm, *slot;
  uint64_t *key, *skey;
  Tmp tmp;
  size_t total;
};

gcg_status rank_space(const char* fn, int64_t Q, int64_t P, void* workspace, RankSpace* s) {
  Carver cv(workspace);
  s->sptr = cv.take<int32_t>(Q + 1);
  s->pair_q = cv.take<int32_t>(P);
  s->iota = cv.take<int32_t>(P);
  s->sperm = cv.take<int32_t>(P);
  s->slot = cv.take<int32_t>(P);
  s->key = cv.take<uint64_t>(P);
  s->skey = cv.take<uint64_t>(P);
  TmpSize ts;
  if (P > 0 && Q > 0)
    ts.add(GCG_CUB(DeviceSegmentedRadixSort::SortPairs, s->key, s->skey, s->iota, s->sperm,
        static_cast<int>(P), static_cast<int>(Q), s->sptr, s->sptr));
  return ts.take(fn, cv, &s->tmp, &s->total);
}

bool matrix_ok(int64_t rows, int64_t D, int64_t ld) { return rows >= 0 && D >= 1 && ld >= D; }

bool can_vectorize(const float* E, int64_t lde) { return aligned(E, 16) && lde % 4 == 0; }

}  // namespace

extern "C" {

int32_t gcg_neighbours_tile(int32_t which) {
  switch (which) {
    case GCG_NEIGHBOURS_ROW_TILE: return kRowTile;
    case GCG_NEIGHBOURS_QUERY_TILE: return kQueryTile;
    case GCG_NEIGHBOURS_QUERY_TILE_SMALL: return kQueryTileSmall;
    case GCG_NEIGHBOURS_SLOT_CAP: return kSlotCap;
    case GCG_NEIGHBOURS_COL_CHUNK: return kColChunk;
    case GCG_NEIGHBOURS_MAX_K: return kMaxK;
    case GCG_NEIGHBOURS_MINMAX_ROWS: return kMinMaxRows;
    case GCG_NEIGHBOURS_MERGE_SLICE: return kMergeSlice;
    default: return 0;
  }
}

gcg_status gcg_minmax_l1_rows_f32_workspace_bytes(int64_t V, int64_t D, size_t* bytes) {
  if (bytes == nullptr || V < 0 || V > kMaxRows || D < 1 || D > INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "gcg_minmax_l1_rows_f32_workspace_bytes: bad sizes or null bytes");
  Carver cv(nullptr);
  cv.take<float>(minmax_blocks(V) * D);
  cv.take<float>(minmax_blocks(V) * D);
  cv.take<double>(D);
  cv.take<double>(D);
  *bytes = cv.used;
  return GCG_OK;
}

gcg_status gcg_minmax_l1_rows_f32(int64_t V, int64_t D, const float* E, int64_t lde, float* out,
                                  int64_t ldo, int32_t* status_dev, void* workspace,
                                  size_t workspace_bytes, gcg_stream_t stream) {
  if (V > kMaxRows || D > INT32_MAX || !matrix_ok(V, D, lde) || ldo < D)
    return fail(GCG_ERR_INVALID_ARG, "gcg_minmax_l1_rows_f32: bad sizes V=%lld D=%lld lde=%lld ldo=%lld",
                static_cast<long long>(V), static_cast<long long>(D), static_cast<long long>(lde),
                static_cast<long long>(ldo));
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_minmax_l1_rows_f32: null status_dev");
  if (!aligned(status_dev, 4)) return fail(GCG_ERR_MISALIGNED, "gcg_minmax_l1_rows_f32: status_dev misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (V == 0) return GCG_OK;
  if (E == nullptr || out == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_minmax_l1_rows_f32: null operand");
  if (!aligned(E, 4) || !aligned(out, 4) || !aligned(workspace, 256))
    return fail(GCG_ERR_MISALIGNED, "gcg_minmax_l1_rows_f32: operand not aligned (workspace: 256 B)");
  size_t need = 0;
  (void)gcg_minmax_l1_rows_f32_workspace_bytes(V, D, &need);
  if (gcg_status s = check_workspace("gcg_minmax_l1_rows_f32", workspace, workspace_bytes, need, 256))
    return s;
  const int64_t nb = minmax_blocks(V);
  Carver cv(workspace);
  float* pmin = cv.take<float>(nb * D);
  float* pmax = cv.take<float>(nb * D);
  double* scale = cv.take<double>(D);
  double* offset = cv.take<double>(D);
  const int64_t cb = (D + kMinMaxCols - 1) / kMinMaxCols;
  if (nb > 65535) return fail(GCG_ERR_INVALID_ARG, "gcg_minmax_l1_rows_f32: V too large");
  hipLaunchKernelGGL(colminmax_partial_kernel, dim3(static_cast<unsigned>(cb), static_cast<unsigned>(nb)),
                     dim3(256), 0, st, V, D, E, lde, pmin, pmax, status_dev);
  hipLaunchKernelGGL(colscale_kernel, dim3(grid_for(D)), dim3(256), 0, st, D, nb, pmin, pmax, scale,
                     offset);
  const int64_t wg = std::min<int64_t>((V + 3) / 4, 16384);
  hipLaunchKernelGGL(scale_l1_rows_kernel, dim3(static_cast<unsigned>(wg)), dim3(256), 0, st, V, D, E,
                     lde, scale, offset, out, ldo);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_neighbour_ranks_f32_workspace_bytes(int64_t Q, int64_t P, size_t* bytes) {
  if (bytes == nullptr || Q < 0 || Q > kMaxQueries || P < 0 || P > INT32_MAX - 1)
    return fail(GCG_ERR_INVALID_ARG, "gcg_neighbour_ranks_f32_workspace_bytes: bad sizes or null bytes");
  RankSpace s;
  gcg_status rc = rank_space("gcg_neighbour_ranks_f32_workspace_bytes", Q, P, nullptr, &s);
  if (rc != GCG_OK) return rc;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_neighbour_ranks_f32(int64_t V, int64_t D, const float* E, int64_t lde, int64_t Q,
                                   const float* queries, int64_t ldq, int64_t P,
                                   const int32_t* pair_ptr, const int32_t* pair_word,
                                   int32_t* rank, int32_t* status_dev, void* workspace,
                                   size_t workspace_bytes, gcg_stream_t stream) {
  if (V > kMaxRows || D > INT32_MAX || !matrix_ok(V, D, lde) || !matrix_ok(Q, D, ldq) ||
      Q > kMaxQueries || P < 0 || P > INT32_MAX - 1)
    return fail(GCG_ERR_INVALID_ARG, "gcg_neighbour_ranks_f32: bad sizes V=%lld D=%lld Q=%lld P=%lld",
                static_cast<long long>(V), static_cast<long long>(D), static_cast<long long>(Q),
                static_cast<long long>(P));
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_neighbour_ranks_f32: null status_dev");
  if (!aligned(status_dev, 4)) return fail(GCG_ERR_MISALIGNED, "gcg_neighbour_ranks_f32: status_dev misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (P == 0) return GCG_OK;
  if (Q == 0 || V == 0) return fail(GCG_ERR_INVALID_ARG, "gcg_neighbour_ranks_f32: pairs but no query or no row");
  if (E == nullptr || queries == nullptr || pair_ptr == nullptr || pair_word == nullptr || rank == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_neighbour_ranks_f32: null operand");
  if (!aligned(E, 4) || !aligned(queries, 4) || !aligned(pair_ptr, 4) || !aligned(pair_word, 4) ||
      !aligned(rank, 4) || !aligned(workspace, 256))
    return fail(GCG_ERR_MISALIGNED, "gcg_neighbour_ranks_f32: operand not aligned (workspace: 256 B)");
  RankSpace s;
  gcg_status rc = rank_space("gcg_neighbour_ranks_f32", Q, P, workspace, &s);
  if (rc != GCG_OK) return rc;
  if ((rc = check_workspace("gcg_neighbour_ranks_f32", workspace, workspace_bytes, s.total, 256)))
    return rc;
  GCG_HIP_CHECK(hipMemsetAsync(rank, 0, P * sizeof(int32_t), st));
  GCG_HIP_CHECK(hipMemsetAsync(s.slot, 0, P * sizeof(int32_t), st));
  GCG_HIP_CHECK(hipMemsetAsync(s.pair_q, 0xff, P * sizeof(int32_t), st));
  hipLaunchKernelGGL(pair_ptr_check_kernel, dim3(grid_for(Q + 1)), dim3(256), 0, st, Q, P, pair_ptr,
                     status_dev);
  hipLaunchKernelGGL(pair_ptr_expand_kernel, dim3(grid_for(Q + 1)), dim3(256), 0, st, Q, pair_ptr,
                     status_dev, s.sptr, s.pair_q);
  hipLaunchKernelGGL(pair_threshold_kernel, dim3(grid_for(P * kWave)), dim3(256), 0, st, V, D, E, lde,
                     queries, ldq, P, s.pair_q, pair_word, s.key, status_dev);
  hipLaunchKernelGGL(iota_kernel, dim3(grid_for(P)), dim3(256), 0, st, P, s.iota);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceSegmentedRadixSort::SortPairs, s.key, s.skey, s.iota, s.sperm,
      static_cast<int>(P), static_cast<int>(Q), s.sptr, s.sptr + 1, 0, 64, st)));
  const bool vec = can_vectorize(E, lde);
  if (Q <= kQueryTileSmall) {
    hipLaunchKernelGGL(neighbour_count_kernel<kQueryTileSmall>,
                       dim3(static_cast<unsigned>(row_tiles(V)), 1), dim3(256), 0, st, V, D, E, lde, Q,
                       queries, ldq, vec, s.sptr, s.skey, s.slot, status_dev);
  } else {
    const unsigned gy = static_cast<unsigned>((Q + kQueryTile - 1) / kQueryTile);
    hipLaunchKernelGGL(neighbour_count_kernel<kQueryTile>,
                       dim3(static_cast<unsigned>(row_tiles(V)), gy), dim3(256), 0, st, V, D, E, lde, Q,
                       queries, ldq, vec, s.sptr, s.skey, s.slot, status_dev);
  }
  hipLaunchKernelGGL(slot_scan_kernel, dim3(static_cast<unsigned>(std::min<int64_t>(Q, 65536))), dim3(256),
                     0, st, Q, s.sptr, s.slot, s.sperm, rank);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_kneighbors_f32_workspace_bytes(int64_t V, int64_t Q, int64_t k, size_t* bytes) {
  if (bytes == nullptr || V < 1 || V > kMaxRows || Q < 0 || Q > kMaxQueries || k < 1 || k > kMaxK ||
      k > V)
    return fail(GCG_ERR_INVALID_ARG,
                "gcg_kneighbors_f32_workspace_bytes: need 1 <= k <= min(V, %d), Q >= 0, non-null bytes", kMaxK);
  const int64_t ncand = row_tiles(V) * std::min<int64_t>(k, kRowTile);
  Carver cv(nullptr);
  cv.take<uint64_t>(static_cast<size_t>(Q) * ncand);
  cv.take<uint64_t>(static_cast<size_t>(Q) * merge_splits(ncand) * k);
  *bytes = cv.used;
  return GCG_OK;
}

gcg_status gcg_kneighbors_f32(int64_t V, int64_t D, const float* E, int64_t lde, int64_t Q,
                              const float* queries, int64_t ldq, int64_t k, float* dist2,
                              int32_t* index, int32_t* status_dev, void* workspace,
                              size_t workspace_bytes, gcg_stream_t stream) {
  if (V < 1 || V > kMaxRows || D > INT32_MAX || !matrix_ok(V, D, lde) || !matrix_ok(Q, D, ldq) ||
      Q > kMaxQueries)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kneighbors_f32: bad sizes V=%lld D=%lld Q=%lld",
                static_cast<long long>(V), static_cast<long long>(D), static_cast<long long>(Q));
  if (k < 1 || k > kMaxK || k > V)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kneighbors_f32: need 1 <= k <= min(V, %d), got k=%lld", kMaxK,
                static_cast<long long>(k));
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_kneighbors_f32: null status_dev");
  if (!aligned(status_dev, 4)) return fail(GCG_ERR_MISALIGNED, "gcg_kneighbors_f32: status_dev misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (Q == 0) return GCG_OK;
  if (E == nullptr || queries == nullptr || dist2 == nullptr || index == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kneighbors_f32: null operand");
  if (!aligned(E, 4) || !aligned(queries, 4) || !aligned(dist2, 4) || !aligned(index, 4) ||
      !aligned(workspace, 256))
    return fail(GCG_ERR_MISALIGNED, "gcg_kneighbors_f32: operand not aligned (workspace: 256 B)");
  size_t need = 0;
  (void)gcg_kneighbors_f32_workspace_bytes(V, Q, k, &need);
  if (gcg_status s = check_workspace("gcg_kneighbors_f32", workspace, workspace_bytes, need, 256))
    return s;
  const int kk = static_cast<int>(std::min<int64_t>(k, kRowTile));
  const int64_t nt = row_tiles(V);
  const int64_t ncand = nt * kk, nsplit = merge_splits(ncand);
  Carver cv(workspace);
  uint64_t* cand = cv.take<uint64_t>(static_cast<size_t>(Q) * ncand);
  uint64_t* part = cv.take<uint64_t>(static_cast<size_t>(Q) * nsplit * k);
  const bool vec = can_vectorize(E, lde);
  if (Q <= kQueryTileSmall) {
    hipLaunchKernelGGL(knn_tile_kernel<kQueryTileSmall>, dim3(static_cast<unsigned>(nt), 1), dim3(256), 0,
                       st, V, D, E, lde, Q, queries, ldq, vec, kk, cand, status_dev);
  } else {
    const unsigned gy = static_cast<unsigned>((Q + kQueryTile - 1) / kQueryTile);
    hipLaunchKernelGGL(knn_tile_kernel<kQueryTile>, dim3(static_cast<unsigned>(nt), gy), dim3(256), 0, st,
                       V, D, E, lde, Q, queries, ldq, vec, kk, cand, status_dev);
  }
  if (nsplit > 1) {  // two levels: slices of the candidates, then the slices' k each
    const int64_t per = (ncand + nsplit - 1) / nsplit;
    hipLaunchKernelGGL(knn_merge_kernel, dim3(static_cast<unsigned>(Q), static_cast<unsigned>(nsplit)),
                       dim3(256), 0, st, ncand, per, static_cast<int>(k), cand, part, nullptr, nullptr);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(static_cast<unsigned>(Q)), dim3(256), 0, st, nsplit * k,
                       nsplit * k, static_cast<int>(k), part, nullptr, dist2, index);
  } else {
    hipLaunchKernelGGL(knn_merge_kernel, dim3(static_cast<unsigned>(Q)), dim3(256), 0, st, ncand, ncand,
                       static_cast<int>(k), cand, nullptr, dist2, index);
  }
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
