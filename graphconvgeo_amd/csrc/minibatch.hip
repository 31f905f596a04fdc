// minibatch.hip -- the mini-batch MLP trainer's own kernels (reference mlp.py:96-311, driven by
// tensormain.main_justinputconv): the column grouping of every batch of an epoch at once, and
// the one-pass update of the sparse-input weight W1 (data gradient of the batch's touched rows,
// L1/L2 penalty gradient and Lasagne Adam in a single sweep over W1, m, v; or, for loc2lang's
// no-MDN baseline, the data gradient and Lasagne Adamax: the same kernel on another rule).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "scratch.h"
#include "philox.h"

using namespace gcg;

namespace {

// ---- epoch segmentation -----------------------------------------------------------------

// len[p] = nonzeros of row perm[p] (0 for a row outside [0, n_rows)), len[n_sel] = 0.
__global__ void mb_row_len_kernel(int64_t n_rows, const int32_t* __restrict__ indptr,
                                  const int32_t* __restrict__ perm, int64_t n_sel,
                                  int32_t* __restrict__ len) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p <= n_sel; p += stride) {
    int32_t n = 0;
    if (p < n_sel) {
      const int32_t r = perm[p];
      if (r >= 0 && r < n_rows) n = max(indptr[r + 1] - indptr[r], 0);
    }
    len[p] = n;
  }
}

// One wave per selected row p (position p % batch of batch p / batch): entry j of the row goes
// to slot sel_ptr[p] + j with key (p / batch) * F + column and payload (position, value bits).
// Entries enumerate the batches in order, each batch's rows in order, each row in storage
// order; the stable sort by key keeps that order inside a (batch, column) segment.
__global__ __launch_bounds__(kBlock) void mb_expand_kernel(
    int64_t n_rows, int64_t F, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const int32_t* __restrict__ perm, int64_t n_sel, int64_t batch, int64_t nnz_sel,
    uint32_t sentinel, const int32_t* __restrict__ sel_ptr, uint32_t* __restrict__ key,
    uint64_t* __restrict__ payload) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); p < n_sel;
       p += wstride) {
    const int32_t r = perm[p];
    if (r < 0 || r >= n_rows) continue;
    const int32_t s = indptr[r];
    const int32_t n = indptr[r + 1] - s;
    const int64_t base = sel_ptr[p];
    const uint32_t kb = static_cast<uint32_t>((p / batch) * F);
    const uint64_t pos = static_cast<uint64_t>(p % batch) << 32;
    for (int32_t j = lane; j < n; j += kWave) {
      const int64_t e = base + j;
      if (e < 0 || e >= nnz_sel) break;  // a caller's nnz_sel below the rows' real total
      const int32_t c = indices[s + j];
      key[e] = (c >= 0 && c < F) ? kb + static_cast<uint32_t>(c) : sentinel;
      payload[e] = pos | __float_as_uint(vals[s + j]);
    }
  }
}

// mb_expand_kernel with input dropout (gcg_minibatch_segment_dropout): every selected entry is
// masked by the keep rule of philox.h -- logical row = the row's id in X, logical column = its
// column, step = *step_dev + the batch's index in the call -- and the masked value goes both
// into the sort payload (so ent_val is masked for the W1 step) and into vals_drop at the
// entry's own CSR slot (so the existing forward reads it). A row is in at most one batch of an
// epoch's order, so no slot is written twice.
__global__ __launch_bounds__(kBlock) void mb_expand_dropout_kernel(
    int64_t n_rows, int64_t F, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const int32_t* __restrict__ perm, int64_t n_sel, int64_t batch, int64_t nnz_sel,
    uint32_t sentinel, const int32_t* __restrict__ sel_ptr, uint32_t* __restrict__ key,
    uint64_t* __restrict__ payload, DropKey d, const int32_t* __restrict__ step_dev,
    float* __restrict__ vals_drop) {
  const uint32_t step0 = static_cast<uint32_t>(*step_dev);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); p < n_sel;
       p += wstride) {
    const int32_t r = perm[p];
    if (r < 0 || r >= n_rows) continue;
    const int32_t s = indptr[r];
    const int32_t n = indptr[r + 1] - s;
    const int64_t base = sel_ptr[p];
    const int64_t b = p / batch;
    const uint32_t kb = static_cast<uint32_t>(b * F);
    const uint64_t pos = static_cast<uint64_t>(p % batch) << 32;
    d.step = step0 + static_cast<uint32_t>(b);
    for (int32_t j = lane; j < n; j += kWave) {
      const int64_t e = base + j;
      if (e < 0 || e >= nnz_sel) break;  // a caller's nnz_sel below the rows' real total
      const int32_t c = indices[s + j];
      const float v = drop_element(d, r, c, vals[s + j]);
      vals_drop[s + j] = v;
      key[e] = (c >= 0 && c < F) ? kb + static_cast<uint32_t>(c) : sentinel;
      payload[e] = pos | __float_as_uint(v);
    }
  }
}

// Slots past the rows' real total (a caller's nnz_sel above it): sentinel keys, sorted last and
// left outside every batch's segment range.
__global__ void mb_tail_kernel(const int32_t* __restrict__ sel_ptr, int64_t n_sel, int64_t nnz_sel,
                               uint32_t sentinel, uint32_t* __restrict__ key,
                               uint64_t* __restrict__ payload) {
  const int64_t first = max(static_cast<int64_t>(sel_ptr[n_sel]), int64_t{0});
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = first + static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < nnz_sel;
       e += stride) {
    key[e] = sentinel;
    payload[e] = 0;
  }
}

// Sorted payloads -> (position, value); flag[k] = 1 where a segment starts.
__global__ void mb_unpack_kernel(int64_t n, const uint32_t* __restrict__ key,
                                 const uint64_t* __restrict__ payload, int32_t* __restrict__ ent_pos,
                                 float* __restrict__ ent_val, int32_t* __restrict__ flag) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint64_t q = payload[k];
    ent_pos[k] = static_cast<int32_t>(q >> 32);
    ent_val[k] = __uint_as_float(static_cast<uint32_t>(q));
    flag[k] = (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
  }
}

// Segment s (= inclusive count of flags - 1) starts at entry k: its key, column and start; the
// last entry closes the list (seg_ptr[n_seg] = n) and publishes n_seg.
__global__ void mb_segments_kernel(int64_t n, int64_t F, int64_t seg_cap,
                                   const uint32_t* __restrict__ key,
                                   const int32_t* __restrict__ flag,
                                   const int32_t* __restrict__ count, uint32_t* __restrict__ seg_key,
                                   int32_t* __restrict__ seg_col, int32_t* __restrict__ seg_ptr,
                                   int32_t* __restrict__ n_seg) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride) {
    const int64_t c = count[k];
    if (flag[k] != 0 && c >= 1 && c <= seg_cap) {
      seg_key[c - 1] = key[k];
      seg_col[c - 1] = static_cast<int32_t>(key[k] % static_cast<uint64_t>(F));
      seg_ptr[c - 1] = static_cast<int32_t>(k);
    }
    if (k == n - 1) {
      const int64_t m = min(max(c, int64_t{0}), seg_cap);
      seg_ptr[m] = static_cast<int32_t>(n);
      *n_seg = static_cast<int32_t>(m);
    }
  }
}

// batch_seg_ptr[b] = first segment whose key is >= b * F, b in [0, n_batches].
__global__ void mb_batch_bounds_kernel(int64_t n_batches, int64_t F,
                                       const uint32_t* __restrict__ seg_key,
                                       const int32_t* __restrict__ n_seg,
                                       int32_t* __restrict__ batch_seg_ptr) {
  const int32_t n = *n_seg;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; b <= n_batches;
       b += stride) {
    const uint64_t want = static_cast<uint64_t>(b) * static_cast<uint64_t>(F);
    int32_t lo = 0, hi = n;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (seg_key[mid] < want) lo = mid + 1; else hi = mid;
    }
    batch_seg_ptr[b] = lo;
  }
}

// The scratch of the segmentation, in the order of the take calls. Two regions are shared on
// purpose: the sort's key input is dead once the keys are sorted and then holds the run flags,
// its payload input then holds the flags' running count.
struct SegSpace {
  int64_t seg_cap;
  int end_bit;
  uint32_t *key_in, *key_out;
  uint64_t *pay_in, *pay_out;
  int32_t *flag, *count;  // key_in | flag, pay_in | count
  int32_t *len, *sel_ptr;
  uint32_t* seg_key;
  int32_t* n_seg;
  Tmp tmp;
  size_t total;
};

// The arguments, then the fixed arrays (plain arithmetic, no HIP device), then with `sized` the
// hipcub temporary behind them: rocPRIM sizes it for the device's architecture, so that half
// needs a HIP device. A null workspace is the sizing pass.
gcg_status seg_space(const char* fn, int64_t n_sel, int64_t batch, int64_t F, int64_t nnz_sel,
                     void* workspace, bool sized, SegSpace* s) {
  if (n_sel < 0 || batch <= 0 || F <= 0 || nnz_sel < 0 || n_sel % batch != 0)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes n_sel=%lld batch=%lld n_cols=%lld nnz_sel=%lld "
                "(n_sel must be a multiple of batch)", fn, static_cast<long long>(n_sel),
                static_cast<long long>(batch), static_cast<long long>(F),
                static_cast<long long>(nnz_sel));
  const int64_t nb = n_sel / batch;
  // keys are batch * F + column in 32 bits, with nb * F itself kept free as the sentinel
  if (n_sel >= INT32_MAX || nnz_sel > INT32_MAX || F > INT32_MAX ||
      (nb > 0 && F > (int64_t{0xffffffff} - 1) / nb))
    return fail(GCG_ERR_INVALID_ARG, "%s: %lld batches x %lld columns (or %lld entries) do not fit "
                "the 32-bit sort key", fn, static_cast<long long>(nb), static_cast<long long>(F),
                static_cast<long long>(nnz_sel));
  s->seg_cap = std::min<int64_t>(nnz_sel, nb * F) + 1;
  // nb * F is below 2^32 here (rejected above otherwise), so this never exceeds 32 bits
  s->end_bit = bits_to_hold(static_cast<uint64_t>(nb) * static_cast<uint64_t>(F));
  // take_exact throughout: an empty selection has empty arrays
  Carver cv(workspace);
  s->key_in = cv.take_exact<uint32_t>(nnz_sel);
  s->key_out = cv.take_exact<uint32_t>(nnz_sel);
  s->pay_in = cv.take_exact<uint64_t>(nnz_sel);
  s->pay_out = cv.take_exact<uint64_t>(nnz_sel);
  s->flag = reinterpret_cast<int32_t*>(s->key_in);
  s->count = reinterpret_cast<int32_t*>(s->pay_in);
  s->len = cv.take_exact<int32_t>(n_sel + 1);
  s->sel_ptr = cv.take_exact<int32_t>(n_sel + 1);
  s->seg_key = cv.take_exact<uint32_t>(s->seg_cap);
  s->n_seg = cv.take_exact<int32_t>(1);
  const int n = static_cast<int>(std::max<int64_t>(nnz_sel, 1));
  // (the scans are sized through a const input, as they always were: the library keeps that
  // instantiation of rocPRIM's kernels)
  auto in = [](const int32_t* p) { return p; };
  TmpSize ts;
  if (sized) {
    ts.add(GCG_CUB(DeviceRadixSort::SortPairs, s->key_in, s->key_out, s->pay_in, s->pay_out, n, 0,
        s->end_bit));
    ts.add(GCG_CUB(DeviceScan::ExclusiveSum, in(s->len), s->sel_ptr, static_cast<int>(n_sel + 1)));
    ts.add(GCG_CUB(DeviceScan::InclusiveSum, in(s->flag), s->count, n));
  }
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

// ---- the W1 step ------------------------------------------------------------------------

// Rows of W1 per workgroup (one segment lookup per workgroup). 4, 8 and 16 measured the same
// within noise at 64 nonzeros per row, 8 a little ahead at ~700 (profiles/mlp/w1_variants.jsonl).
constexpr int kStepRows = 8;

// The update rule of the step, one element at a time. Both take the data gradient d and the
// element's parameter and two state values; a rule's constants are computed once per thread.
//
// Adam: the gradient g = d + (l1 sgn(w) + 2 l2 w) in l1l2_grad_kernel's expression, then
// adam_kernel's update (csr_ops.hip), bit for bit.
struct AdamRule {
  float c1, c2, a_t, b1, b2, ca, cb, eps;
  __device__ AdamRule(float l1, float l2, float a_t_, float b1_, float b2_, float eps_)
      : c1(l1), c2(2.0f * l2), a_t(a_t_), b1(b1_), b2(b2_), ca(1.0f - b1_), cb(1.0f - b2_),
        eps(eps_) {}
  __device__ __forceinline__ void operator()(float& p, float& m, float& v, float d) const {
    const float x = p;
    const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
    const float gi = d + (c1 * sg + c2 * x);
    const float mi = b1 * m + ca * gi;
    const float vi = b2 * v + cb * gi * gi;
    m = mi;
    v = vi;
    p = x - (a_t * mi) / (sqrtf(vi) + eps);
  }
};

// Adamax without a penalty (loc2lang's build has none): g = d, then adamax_kernel's update
// (csr_ops.hip), bit for bit; the second state is u.
struct AdamaxRule {
  float a_t, b1, b2, ca, eps;
  __device__ AdamaxRule(float, float, float a_t_, float b1_, float b2_, float eps_)
      : a_t(a_t_), b1(b1_), b2(b2_), ca(1.0f - b1_), eps(eps_) {}
  __device__ __forceinline__ void operator()(float& p, float& m, float& u, float d) const {
    const float mi = b1 * m + ca * d;
    const float ui = fmaxf(b2 * u, fabsf(d));
    m = mi;
    u = ui;
    p = p - (a_t * mi) / (ui + eps);
  }
};

// A workgroup owns kStepRows consecutive rows of W1. Its segment candidates are the (at most
// kStepRows) segments of this batch whose column falls into those rows: a 64-ary search for the
// first (every lane probes one element per round: 2-3 rounds of one coalesced load instead of
// 13-17 dependent ones), then one coalesced read. A wave takes (row, 64 x VEC column chunk)
// units; a row with a segment accumulates d = sum val * G[pos, :] over the segment in order
// (product and sum rounded separately), every other row has d = +0. The entries of a segment are
// wave-uniform, so they come through scalar loads, four ahead; handing them out by readlane from
// one coalesced load per 64 instead measured 1.4-1.6x slower (profiles/mlp/w1_variants.jsonl).
// A segment is never split across waves: its sum keeps the entries' order, which is what makes
// the step bitwise the composed kernels' and reproducible. W, m, v are requested before the
// gather and used after it. Lanes past K gather column 0 (in bounds, unused).
template <int VEC, typename Rule>
__global__ __launch_bounds__(kBlock) void w1_step_kernel(
    int64_t F, int K, float* __restrict__ P, float* __restrict__ M, float* __restrict__ V,
    const float* __restrict__ G, int64_t ldg, const int32_t* __restrict__ seg_range,
    const int32_t* __restrict__ seg_col, const int32_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ ent_pos, const float* __restrict__ ent_val, float l1, float l2,
    const float* __restrict__ step_dev, float b1, float b2, float eps) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kStepRows;
  const int nr = static_cast<int>(min<int64_t>(kStepRows, F - r0));
  const int sb = uniform(seg_range[0]), se = uniform(seg_range[1]);
  // first segment in [sb, se) whose column is >= r0 (se if none)
  int lo = sb, hi = se;
  while (hi > lo) {
    const int step = (hi - lo + kWave - 1) / kWave;
    const int idx = lo + lane * step;
    const bool lt = idx < hi && seg_col[idx] < r0;
    const int cnt = __popcll(__ballot(lt));  // the probes below r0 are a prefix of the lanes
    if (cnt == 0) {
      hi = lo;
    } else {
      const int nlo = lo + (cnt - 1) * step + 1;
      hi = min(lo + cnt * step, hi);
      lo = nlo;
    }
  }
  const int cand = (lane < kStepRows && lo + lane < se) ? seg_col[lo + lane] : -1;
  const Rule step_element(l1, l2, *step_dev, b1, b2, eps);
  const int chunks = (K + kWave * VEC - 1) / (kWave * VEC);
  for (int t = w; t < nr * chunks; t += kWavesPerBlock) {
    const int i = t / chunks, ch = t - i * chunks;
    const int64_t r = r0 + i;
    const unsigned long long hit = __ballot(cand == static_cast<int>(r));
    int s = 0, e = 0;
    if (hit != 0) {
      const int idx = __ffsll(hit) - 1;
      s = uniform(seg_ptr[lo + idx]);
      e = uniform(seg_ptr[lo + idx + 1]);
    }
    const int c = (ch * kWave + lane) * VEC;
    const bool on = c < K;
    const float* gcol = G + (on ? c : 0);
    const int64_t o = r * K + (on ? c : 0);
    if constexpr (VEC == 4) {
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f), m = p, v = p, d = p;
      if (on) {
        p = *reinterpret_cast<const float4*>(P + o);
        m = *reinterpret_cast<const float4*>(M + o);
        v = *reinterpret_cast<const float4*>(V + o);
      }
#pragma unroll 4
      for (int j = s; j < e; ++j) {
        const float a = ent_val[j];
        const float4 g = *reinterpret_cast<const float4*>(gcol + static_cast<int64_t>(ent_pos[j]) * ldg);
        d.x = d.x + a * g.x; d.y = d.y + a * g.y; d.z = d.z + a * g.z; d.w = d.w + a * g.w;
      }
      if (on) {
        step_element(p.x, m.x, v.x, d.x);
        step_element(p.y, m.y, v.y, d.y);
        step_element(p.z, m.z, v.z, d.z);
        step_element(p.w, m.w, v.w, d.w);
        *reinterpret_cast<float4*>(M + o) = m;
        *reinterpret_cast<float4*>(V + o) = v;
        *reinterpret_cast<float4*>(P + o) = p;
      }
    } else {
      float p = 0.f, m = 0.f, v = 0.f, d = 0.f;
      if (on) {
        p = P[o];
        m = M[o];
        v = V[o];
      }
#pragma unroll 4
      for (int j = s; j < e; ++j)
        d = d + ent_val[j] * gcol[static_cast<int64_t>(ent_pos[j]) * ldg];
      if (on) {
        step_element(p, m, v, d);
        M[o] = m;
        V[o] = v;
        P[o] = p;
      }
    }
  }
}

// Both segmentation calls: `drop` NULL is gcg_minibatch_segment, otherwise the expand pass masks
// (mb_expand_dropout_kernel); every other launch is shared.
gcg_status segment_impl(const char* fn, int64_t n_rows, int64_t n_cols, const int32_t* indptr,
                        const int32_t* indices, const float* vals, const int32_t* perm,
                        int64_t n_sel, int64_t batch, int64_t nnz_sel, int32_t* batch_seg_ptr,
                        int32_t* seg_col, int32_t* seg_ptr, int32_t* ent_pos, float* ent_val,
                        void* workspace, size_t workspace_bytes, gcg_stream_t stream,
                        const DropKey* drop, const int32_t* step_dev, float* vals_drop) {
  if (n_rows < 0 || n_rows >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n_rows", fn);
  SegSpace s;
  if (gcg_status rc = seg_space(fn, n_sel, batch, n_cols, nnz_sel, workspace, false, &s)) return rc;
  if (indptr == nullptr || batch_seg_ptr == nullptr || seg_col == nullptr || seg_ptr == nullptr ||
      (n_sel > 0 && perm == nullptr) ||
      (nnz_sel > 0 && (indices == nullptr || vals == nullptr || ent_pos == nullptr ||
                       ent_val == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL buffer", fn);
  // the fixed arrays first (host arithmetic), then the whole with the hipcub temporary
  if (gcg_status rc = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return rc;
  if (gcg_status rc = seg_space(fn, n_sel, batch, n_cols, nnz_sel, workspace, true, &s)) return rc;
  if (gcg_status rc = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nb = n_sel / batch;
  if (nnz_sel == 0) {  // no entry: every batch's range is empty
    GCG_HIP_CHECK(hipMemsetAsync(batch_seg_ptr, 0, sizeof(int32_t) * (nb + 1), st));
    GCG_HIP_CHECK(hipMemsetAsync(seg_ptr, 0, sizeof(int32_t), st));
    return GCG_OK;
  }
  const uint32_t sentinel = static_cast<uint32_t>(nb * n_cols);
  const int n = static_cast<int>(nnz_sel);

  hipLaunchKernelGGL(mb_row_len_kernel, dim3(grid_for(n_sel + 1)), dim3(256), 0, st, n_rows, indptr,
                     perm, n_sel, s.len);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.len, s.sel_ptr, static_cast<int>(n_sel + 1),
      st)));
  const int64_t row_blocks = (n_sel + kWavesPerBlock - 1) / kWavesPerBlock;
  const dim3 expand_grid(
      static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(row_blocks, 1), 1 << 20)));
  if (drop == nullptr)
    hipLaunchKernelGGL(mb_expand_kernel, expand_grid, dim3(kBlock), 0, st, n_rows, n_cols, indptr,
                       indices, vals, perm, n_sel, batch, nnz_sel, sentinel, s.sel_ptr, s.key_in,
                       s.pay_in);
  else
    hipLaunchKernelGGL(mb_expand_dropout_kernel, expand_grid, dim3(kBlock), 0, st, n_rows, n_cols,
                       indptr, indices, vals, perm, n_sel, batch, nnz_sel, sentinel, s.sel_ptr,
                       s.key_in, s.pay_in, *drop, step_dev, vals_drop);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mb_tail_kernel, dim3(64), dim3(256), 0, st, s.sel_ptr, n_sel, nnz_sel,
                     sentinel, s.key_in, s.pay_in);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, s.key_in, s.key_out, s.pay_in, s.pay_out, n, 0,
      s.end_bit, st)));
  // from here key_in and pay_in are dead: their regions hold the run flags and their count
  hipLaunchKernelGGL(mb_unpack_kernel, dim3(grid_for(nnz_sel)), dim3(256), 0, st, nnz_sel,
                     s.key_out, s.pay_out, ent_pos, ent_val, s.flag);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::InclusiveSum, s.flag, s.count, n, st)));
  hipLaunchKernelGGL(mb_segments_kernel, dim3(grid_for(nnz_sel)), dim3(256), 0, st, nnz_sel, n_cols,
                     s.seg_cap, s.key_out, s.flag, s.count, s.seg_key, seg_col, seg_ptr, s.n_seg);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mb_batch_bounds_kernel, dim3(grid_for(nb + 1)), dim3(256), 0, st, nb, n_cols,
                     s.seg_key, s.n_seg, batch_seg_ptr);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

// Both W1 steps: the checks and the launch, the kernel instantiated on the update rule.
template <typename Rule>
gcg_status w1_step_impl(const char* fn, int64_t F, int64_t K, float* W, float* m, float* v,
                        const float* G, int64_t ldg, int64_t batch, const int32_t* seg_range,
                        const int32_t* seg_col, const int32_t* seg_ptr, const int32_t* ent_pos,
                        const float* ent_val, float l1, float l2, const float* step_dev,
                        float beta1, float beta2, float eps, gcg_stream_t stream) {
  if (F < 0 || K < 0 || batch < 0 || F > INT32_MAX || K > INT32_MAX || ldg < K)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes F=%lld K=%lld batch=%lld ldg=%lld", fn,
                static_cast<long long>(F), static_cast<long long>(K),
                static_cast<long long>(batch), static_cast<long long>(ldg));
  if (F == 0 || K == 0) return GCG_OK;
  if (W == nullptr || m == nullptr || v == nullptr || seg_range == nullptr || seg_col == nullptr ||
      seg_ptr == nullptr || step_dev == nullptr ||
      (batch > 0 && (G == nullptr || ent_pos == nullptr || ent_val == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(W, 4) || !aligned(m, 4) || !aligned(v, 4) || !aligned(G, 4) ||
      !aligned(seg_range, 4) || !aligned(step_dev, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((F + kStepRows - 1) / kStepRows));
  const bool vec = K % 4 == 0 && ldg % 4 == 0 && aligned(G, 16) && aligned(W, 16) &&
                   aligned(m, 16) && aligned(v, 16);
  if (vec)
    hipLaunchKernelGGL((w1_step_kernel<4, Rule>), grid, dim3(kBlock), 0, st, F, static_cast<int>(K),
                       W, m, v, G, ldg, seg_range, seg_col, seg_ptr, ent_pos, ent_val, l1, l2,
                       step_dev, beta1, beta2, eps);
  else
    hipLaunchKernelGGL((w1_step_kernel<1, Rule>), grid, dim3(kBlock), 0, st, F, static_cast<int>(K),
                       W, m, v, G, ldg, seg_range, seg_col, seg_ptr, ent_pos, ent_val, l1, l2,
                       step_dev, beta1, beta2, eps);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // namespace

extern "C" {

gcg_status gcg_minibatch_segment_sizes(int64_t n_sel, int64_t batch, int64_t n_cols,
                                       int64_t nnz_sel, int64_t* seg_capacity,
                                       size_t* workspace_bytes) {
  const char* fn = "gcg_minibatch_segment_sizes";
  SegSpace s;
  // the capacity alone needs no HIP device
  if (gcg_status rc = seg_space(fn, n_sel, batch, n_cols, nnz_sel, nullptr, workspace_bytes != nullptr, &s))
    return rc;
  if (seg_capacity != nullptr) *seg_capacity = s.seg_cap;
  if (workspace_bytes != nullptr) *workspace_bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_minibatch_segment(int64_t n_rows, int64_t n_cols, const int32_t* indptr,
                                 const int32_t* indices, const float* vals, const int32_t* perm,
                                 int64_t n_sel, int64_t batch, int64_t nnz_sel,
                                 int32_t* batch_seg_ptr, int32_t* seg_col, int32_t* seg_ptr,
                                 int32_t* ent_pos, float* ent_val, void* workspace,
                                 size_t workspace_bytes, gcg_stream_t stream) {
  return segment_impl("gcg_minibatch_segment", n_rows, n_cols, indptr, indices, vals, perm, n_sel,
                      batch, nnz_sel, batch_seg_ptr, seg_col, seg_ptr, ent_pos, ent_val, workspace,
                      workspace_bytes, stream, nullptr, nullptr, nullptr);
}

gcg_status gcg_minibatch_segment_dropout(int64_t n_rows, int64_t n_cols, const int32_t* indptr,
                                         const int32_t* indices, const float* vals,
                                         const int32_t* perm, int64_t n_sel, int64_t batch,
                                         int64_t nnz_sel, int32_t* batch_seg_ptr, int32_t* seg_col,
                                         int32_t* seg_ptr, int32_t* ent_pos, float* ent_val,
                                         float* vals_drop, void* workspace, size_t workspace_bytes,
                                         uint32_t threshold, float scale, uint64_t seed,
                                         const int32_t* step_dev, uint32_t stream_id,
                                         gcg_stream_t stream) {
  const char* fn = "gcg_minibatch_segment_dropout";
  if (step_dev == nullptr || (nnz_sel > 0 && vals_drop == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL buffer", fn);
  if (!aligned(step_dev, 4) || !aligned(vals_drop, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const DropKey d{static_cast<uint32_t>(seed & 0xffffffffu), static_cast<uint32_t>(seed >> 32), 0u,
                  stream_id, threshold, scale};
  return segment_impl(fn, n_rows, n_cols, indptr, indices, vals, perm, n_sel, batch, nnz_sel,
                      batch_seg_ptr, seg_col, seg_ptr, ent_pos, ent_val, workspace, workspace_bytes,
                      stream, &d, step_dev, vals_drop);
}

gcg_status gcg_minibatch_w1_step_f32(int64_t F, int64_t K, float* W, float* m, float* v,
                                     const float* G, int64_t ldg, int64_t batch,
                                     const int32_t* seg_range, const int32_t* seg_col,
                                     const int32_t* seg_ptr, const int32_t* ent_pos,
                                     const float* ent_val, float l1, float l2,
                                     const float* step_dev, float beta1, float beta2, float eps,
                                     gcg_stream_t stream) {
  return w1_step_impl<AdamRule>("gcg_minibatch_w1_step_f32", F, K, W, m, v, G, ldg, batch,
                                seg_range, seg_col, seg_ptr, ent_pos, ent_val, l1, l2, step_dev,
                                beta1, beta2, eps, stream);
}

gcg_status gcg_minibatch_w1_adamax_step_f32(int64_t F, int64_t K, float* W, float* m, float* u,
                                            const float* G, int64_t ldg, int64_t batch,
                                            const int32_t* seg_range, const int32_t* seg_col,
                                            const int32_t* seg_ptr, const int32_t* ent_pos,
                                            const float* ent_val, const float* step_dev,
                                            float beta1, float beta2, float eps,
                                            gcg_stream_t stream) {
  return w1_step_impl<AdamaxRule>("gcg_minibatch_w1_adamax_step_f32", F, K, W, m, u, G, ldg, batch,
                                  seg_range, seg_col, seg_ptr, ent_pos, ent_val, 0.f, 0.f,
                                  step_dev, beta1, beta2, eps, stream);
}

}  // extern "C"
