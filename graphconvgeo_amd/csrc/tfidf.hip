// tfidf.hip -- the arithmetic half of DataLoader.tfidf (reference data.py:378-397, sklearn's
// TfidfVectorizer at ngram_range (1, 1)) over token ids: counting a chunk of whole documents into a
// canonical count CSR, document frequencies, vocabulary pruning and column renumbering, and the
// tf-idf weighting with its row norm. Tokenising and the term dictionary stay on the host
// (graphconvgeo_amd/tfidf.py).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "scratch.h"

using namespace gcg;

namespace {

// A dropped token (id outside [0, V)): every sorted bit set, and the bit above the document's
// bits, which no kept key has, so the dropped tokens sort behind every document.
constexpr uint64_t kDropped = ~uint64_t{0};

// ---- count --------------------------------------------------------------------------------

// One wave per document: token j of document d goes to slot j (the chunk's tokens are its
// documents' tokens in order) as key d << vbits | term, after the rank map when there is one.
// Slots no document covers keep the kDropped the buffer was filled with.
__global__ __launch_bounds__(kBlock) void tfidf_keys_kernel(
    int64_t n_docs, int64_t V, int vbits, const int64_t* __restrict__ doc_ptr,
    const int32_t* __restrict__ tokens, int64_t n_tokens, const int32_t* __restrict__ rank,
    uint64_t* __restrict__ key) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t first = doc_ptr[0];
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); d < n_docs;
       d += wstride) {
    const int64_t s = max(doc_ptr[d] - first, int64_t{0});
    const int64_t e = min(doc_ptr[d + 1] - first, n_tokens);
    for (int64_t j = s + lane; j < e; j += kWave) {
      int32_t t = tokens[j];
      if (rank != nullptr && t >= 0 && t < V) t = rank[t];
      key[j] = (t >= 0 && t < V) ? (static_cast<uint64_t>(d) << vbits) | static_cast<uint64_t>(t)
                                 : kDropped;
    }
  }
}

// Runs of the sorted keys that are entries: all but a last run of dropped tokens.
__device__ __forceinline__ int64_t entry_runs(const int32_t* num_runs, const uint64_t* uniq) {
  int64_t n = *num_runs;
  if (n > 0 && uniq[n - 1] == kDropped) --n;
  return n;
}

// Run k -> entry base + k: its term and its length. With `cols` (the term-ordered document
// frequency) every one of the n_tokens slots gets the entry's term, or V behind the entries;
// without it and with `df`, one integer atomic per entry.
__global__ void tfidf_decode_kernel(int64_t n_tokens, int64_t V, int vbits,
                                    const uint64_t* __restrict__ uniq,
                                    const int32_t* __restrict__ run_len,
                                    const int32_t* __restrict__ num_runs,
                                    const int64_t* __restrict__ nnz_dev, int64_t capacity,
                                    int32_t* __restrict__ indices, int32_t* __restrict__ counts,
                                    unsigned long long* __restrict__ df,
                                    int32_t* __restrict__ cols) {
  const int64_t n = entry_runs(num_runs, uniq), base = *nnz_dev;
  if (base < 0 || base + n > capacity) return;
  const uint64_t mask = (uint64_t{1} << vbits) - 1;
  const int64_t upto = cols != nullptr ? n_tokens : n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < upto; k += stride) {
    if (k < n) {
      const int32_t term = static_cast<int32_t>(uniq[k] & mask);
      indices[base + k] = term;
      counts[base + k] = run_len[k];
      if (cols != nullptr) cols[k] = term;
      else if (df != nullptr) atomicAdd(df + term, 1ull);
    } else {
      cols[k] = static_cast<int32_t>(V);
    }
  }
}

// The term-ordered document frequency: run r of the chunk's sorted columns is one term and the
// number of rows that hold it. Terms of different runs differ, so the add needs no atomic.
__global__ void tfidf_df_runs_kernel(int64_t V, const int32_t* __restrict__ term,
                                     const int32_t* __restrict__ run_len,
                                     const int32_t* __restrict__ num_runs,
                                     unsigned long long* __restrict__ df) {
  const int64_t n = *num_runs;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
    const int32_t t = term[r];
    if (t >= 0 && t < V) df[t] += static_cast<unsigned long long>(run_len[r]);
  }
}

// indptr[d] = base + the first entry whose key is >= d << vbits, d in [0, n_docs].
__global__ void tfidf_indptr_kernel(int64_t n_docs, int vbits, const uint64_t* __restrict__ uniq,
                                    const int32_t* __restrict__ num_runs,
                                    const int64_t* __restrict__ nnz_dev, int64_t capacity,
                                    int32_t* __restrict__ indptr) {
  const int64_t n = entry_runs(num_runs, uniq), base = *nnz_dev;
  if (base < 0 || base + n > capacity) return;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= n_docs; d += stride) {
    const uint64_t want = static_cast<uint64_t>(d) << vbits;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (uniq[mid] < want) lo = mid + 1; else hi = mid;
    }
    indptr[d] = static_cast<int32_t>(base + lo);
  }
}

// The chunk is done: the running entry count moves on, or the chunk did not fit.
__global__ void tfidf_advance_kernel(const uint64_t* __restrict__ uniq,
                                     const int32_t* __restrict__ num_runs, int64_t capacity,
                                     int64_t* __restrict__ nnz_dev, int32_t* __restrict__ status_dev) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t n = entry_runs(num_runs, uniq), base = *nnz_dev;
  if (base < 0 || base + n > capacity) *status_dev = GCG_ERR_WORKSPACE;
  else *nnz_dev = base + n;
}

// The scratch of a count, in the order of the take calls. The sorted keys are dead once the
// runs are encoded, and the term-ordered document frequency then sorts the entries' columns
// in their region: sorted keys | columns, sorted columns.
struct CountSpace {
  int vbits, end_bit, cbits;
  uint64_t *key_a, *key_b;  // keys, then the unique keys | sorted keys
  int32_t *cols, *cols_sorted;
  int32_t *run_len, *term, *term_len, *num_runs;  // (terms and lengths of the column runs)
  Tmp tmp;
  size_t total;
};

// The arguments, then the fixed arrays (no HIP device), then with `sized` the hipcub temporary:
// rocPRIM sizes it for the device's architecture, so that half needs a HIP device.
gcg_status count_space(const char* fn, int64_t n_docs, int64_t n_tokens, int64_t V, void* workspace,
                       bool sized, CountSpace* s) {
  if (n_docs < 0 || n_docs >= INT32_MAX || n_tokens < 0 || n_tokens >= INT32_MAX || V < 1 ||
      V >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes n_docs=%lld n_tokens=%lld n_terms=%lld "
                "(each below 2^31 - 1, n_terms >= 1)", fn, static_cast<long long>(n_docs),
                static_cast<long long>(n_tokens), static_cast<long long>(V));
  s->vbits = bits_to_hold(static_cast<uint64_t>(V - 1));
  s->end_bit = s->vbits + bits_to_hold(static_cast<uint64_t>(std::max<int64_t>(n_docs, 1) - 1)) + 1;
  s->cbits = bits_to_hold(static_cast<uint64_t>(V));
  // take_exact throughout: a chunk without tokens has empty arrays
  const size_t n8 = align_up(static_cast<size_t>(n_tokens) * 8, 256);
  const size_t n4 = align_up(static_cast<size_t>(n_tokens) * 4, 256);
  Carver cv(workspace);
  s->key_a = cv.take_exact<uint64_t>(n_tokens);
  s->key_b = cv.take_bytes<uint64_t>(std::max(n8, 2 * n4));
  s->cols = reinterpret_cast<int32_t*>(s->key_b);
  s->cols_sorted = s->cols ? s->cols + n4 / 4 : nullptr;
  s->run_len = cv.take_exact<int32_t>(n_tokens);
  s->term = cv.take_exact<int32_t>(n_tokens);
  s->term_len = cv.take_exact<int32_t>(n_tokens);
  s->num_runs = cv.take_bytes<int32_t>(256);  // [0] the keys' runs, [1] the columns'
  const int n = static_cast<int>(std::max<int64_t>(n_tokens, 1));
  TmpSize ts;
  if (sized) {
    ts.add(GCG_CUB(DeviceRadixSort::SortKeys, s->key_a, s->key_b, n, 0, s->end_bit));
    ts.add(GCG_CUB(DeviceRunLengthEncode::Encode, s->key_b, s->key_a, s->run_len, s->num_runs, n));
    ts.add(GCG_CUB(DeviceRadixSort::SortKeys, s->cols, s->cols_sorted, n, 0, s->cbits));
    ts.add(GCG_CUB(DeviceRunLengthEncode::Encode, s->cols_sorted, s->term, s->term_len, s->num_runs, n));
  }
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

// ---- select -------------------------------------------------------------------------------

__global__ void tfidf_keep_kernel(int64_t V, const int64_t* __restrict__ df, int64_t lo, int64_t hi,
                                  int32_t* __restrict__ keep) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < V; t += stride)
    keep[t] = (df[t] >= lo && df[t] <= hi) ? 1 : 0;
}

__global__ void tfidf_renumber_kernel(int64_t V, const int64_t* __restrict__ df,
                                      const int32_t* __restrict__ keep,
                                      const int32_t* __restrict__ pos, int32_t* __restrict__ new_id,
                                      int64_t* __restrict__ kept_df, int64_t* __restrict__ n_kept) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < V; t += stride) {
    const int32_t k = keep[t], p = pos[t];
    new_id[t] = k ? p : -1;
    if (k) kept_df[p] = df[t];
    if (t == V - 1) *n_kept = static_cast<int64_t>(p) + k;
  }
}

__global__ void tfidf_idf_kernel(int64_t n_terms, const int64_t* __restrict__ df, double n_docs,
                                 double* __restrict__ idf) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_terms; t += stride)
    idf[t] = log((1.0 + n_docs) / (1.0 + static_cast<double>(df[t]))) + 1.0;
}

// ---- column compaction --------------------------------------------------------------------

__device__ __forceinline__ bool kept_column(int32_t c, int64_t V, const int32_t* new_id) {
  return c >= 0 && c < V && new_id[c] >= 0;
}

// One wave per row: len[r] = entries of row r whose column is kept; len[n_rows] = 0.
__global__ __launch_bounds__(kBlock) void tfidf_row_kept_kernel(
    int64_t n_rows, int64_t V, int64_t nnz, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int32_t* __restrict__ new_id,
    int32_t* __restrict__ len) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); r <= n_rows;
       r += wstride) {
    int32_t n = 0;
    if (r < n_rows) {
      const int64_t s = max<int64_t>(indptr[r], 0), e = min<int64_t>(indptr[r + 1], nnz);
      for (int64_t j0 = s; j0 < e; j0 += kWave) {
        const int64_t j = j0 + lane;
        const bool k = j < e && kept_column(indices[j], V, new_id);
        n += __popcll(__ballot(k));
      }
    }
    if (lane == 0) len[r] = n;
  }
}

// One wave per row: the kept entries, in the row's order, to out_indptr[r] onwards with their
// new column. new_id grows with the old id, so a sorted row stays sorted.
__global__ __launch_bounds__(kBlock) void tfidf_compact_kernel(
    int64_t n_rows, int64_t V, int64_t nnz, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ new_id, const int32_t* __restrict__ out_indptr, int64_t capacity,
    int32_t* __restrict__ out_indices, int32_t* __restrict__ out_counts) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); r < n_rows;
       r += wstride) {
    const int64_t s = max<int64_t>(indptr[r], 0), e = min<int64_t>(indptr[r + 1], nnz);
    int64_t o = out_indptr[r];
    for (int64_t j0 = s; j0 < e; j0 += kWave) {
      const int64_t j = j0 + lane;
      const int32_t c = j < e ? indices[j] : -1;
      const bool k = kept_column(c, V, new_id);
      const unsigned long long m = __ballot(k);
      const int64_t at = o + __popcll(m & ((1ull << lane) - 1));
      if (k && at >= 0 && at < capacity) {
        out_indices[at] = new_id[c];
        out_counts[at] = counts[j];
      }
      o += __popcll(m);
    }
  }
}

// ---- weighting ----------------------------------------------------------------------------

enum { kNormNone = 0, kNormL1 = 1, kNormL2 = 2 };

__device__ __forceinline__ double term_weight(int32_t count, int32_t col, int64_t n_cols,
                                              const double* idf, int binary, int sublinear) {
  double tf = binary ? 1.0 : static_cast<double>(count);
  if (sublinear) tf = log(tf) + 1.0;
  if (idf != nullptr && col >= 0 && col < n_cols) tf = tf * idf[col];
  return tf;
}

// One wave per row, everything in double: lane l folds entries l, l + 64, ... in that order, the
// butterfly folds the lanes -- the same order every launch, no atomics -- and the one rounding
// to float32 is the store. An empty or zero-norm row is left as it is.
__global__ __launch_bounds__(kBlock) void tfidf_weight_kernel(
    int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int32_t* __restrict__ counts,
    const double* __restrict__ idf, int binary, int sublinear, int norm, float* __restrict__ vals) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); r < n_rows;
       r += wstride) {
    const int64_t s = max<int64_t>(indptr[r], 0), e = min<int64_t>(indptr[r + 1], nnz);
    double denom = 0.0;
    if (norm != kNormNone) {
      double acc = 0.0;
      for (int64_t j = s + lane; j < e; j += kWave) {
        const double x = term_weight(counts[j], indices[j], n_cols, idf, binary, sublinear);
        acc = acc + (norm == kNormL2 ? x * x : fabs(x));
      }
      acc = wave_sum(acc);
      denom = norm == kNormL2 ? sqrt(acc) : acc;
    }
    for (int64_t j = s + lane; j < e; j += kWave) {
      const double x = term_weight(counts[j], indices[j], n_cols, idf, binary, sublinear);
      vals[j] = static_cast<float>(denom != 0.0 ? x / denom : x);
    }
  }
}

int wave_grid(int64_t rows) {
  const int64_t g = (rows + kWavesPerBlock - 1) / kWavesPerBlock;
  return static_cast<int>(std::min<int64_t>(std::max<int64_t>(g, 1), 1 << 16));
}

gcg_status compact_sizes(const char* fn, int64_t n_rows, int64_t V, int64_t nnz) {
  if (n_rows < 0 || n_rows >= INT32_MAX || V < 1 || V >= INT32_MAX || nnz < 0 || nnz > INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes n_rows=%lld n_terms=%lld nnz=%lld", fn,
                static_cast<long long>(n_rows), static_cast<long long>(V),
                static_cast<long long>(nnz));
  return GCG_OK;
}

// The scratch of a selection: the keep flags, their exclusive sum, hipcub's temporary.
struct SelectSpace {
  int32_t *keep, *pos;
  Tmp tmp;
  size_t total;
};

gcg_status select_space(const char* fn, int64_t n_terms, void* workspace, bool sized,
                        SelectSpace* s) {
  if (n_terms < 1 || n_terms >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n_terms=%lld", fn, static_cast<long long>(n_terms));
  Carver cv(workspace);
  s->keep = cv.take_exact<int32_t>(n_terms);
  s->pos = cv.take_exact<int32_t>(n_terms);
  TmpSize ts;
  if (sized) {
    ts.add(GCG_CUB(DeviceScan::ExclusiveSum, s->keep, s->pos, static_cast<int>(n_terms)));
  }
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

// The scratch of a compaction's sizing call: the kept entries per row (n_rows + 1), hipcub's
// temporary for their exclusive sum into out_indptr. The callers have validated n_rows.
struct CompactSpace {
  int32_t* len;
  Tmp tmp;
  size_t total;
};

gcg_status compact_space(const char* fn, int64_t n_rows, void* workspace, CompactSpace* s) {
  Carver cv(workspace);
  s->len = cv.take_exact<int32_t>(n_rows + 1);
  TmpSize ts;
  ts.add(GCG_CUB(DeviceScan::ExclusiveSum, s->len, s->len, static_cast<int>(n_rows + 1)));
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

}  // namespace

extern "C" {

gcg_status gcg_tfidf_count_workspace_bytes(int64_t n_docs, int64_t n_tokens, int64_t n_terms,
                                           size_t* bytes) {
  const char* fn = "gcg_tfidf_count_workspace_bytes";
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  CountSpace s;
  if (const gcg_status st = count_space(fn, n_docs, n_tokens, n_terms, nullptr, true, &s)) return st;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_tfidf_count(int64_t n_docs, int64_t n_terms, int64_t n_tokens,
                           const int64_t* doc_ptr, const int32_t* tokens, const int32_t* rank,
                           int32_t* indptr, int32_t* indices, int32_t* counts, int64_t capacity,
                           int64_t* nnz_dev, int64_t* df, int32_t df_mode, int32_t* status_dev,
                           void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  const char* fn = "gcg_tfidf_count";
  CountSpace s;
  if (const gcg_status st = count_space(fn, n_docs, n_tokens, n_terms, nullptr, false, &s)) return st;
  const bool sizing = indptr == nullptr && indices == nullptr && counts == nullptr;
  if (!sizing && (indptr == nullptr || indices == nullptr || counts == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: indptr, indices and counts are all NULL (sizing) or "
                "none is", fn);
  if (doc_ptr == nullptr || nnz_dev == nullptr || status_dev == nullptr ||
      (n_tokens > 0 && tokens == nullptr) || workspace == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL doc_ptr, tokens, nnz_dev, status_dev or workspace",
                fn);
  if (capacity < 0 || capacity > INT32_MAX || (df_mode != 0 && df_mode != 1))
    return fail(GCG_ERR_INVALID_ARG, "%s: capacity %lld outside [0, 2^31) or df_mode %d not 0 / 1",
                fn, static_cast<long long>(capacity), static_cast<int>(df_mode));
  if (!aligned(doc_ptr, 8) || !aligned(nnz_dev, 8) || !aligned(df, 8) || !aligned(tokens, 4) ||
      !aligned(rank, 4) || !aligned(indptr, 4) || !aligned(indices, 4) || !aligned(counts, 4) ||
      !aligned(status_dev, 4) || !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: a buffer is not aligned to its element size", fn);
  if (const gcg_status st = count_space(fn, n_docs, n_tokens, n_terms, workspace, true, &s))
    return st;
  if (const gcg_status st = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return st;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n = static_cast<int>(n_tokens);
  // a sizing call only moves nnz_dev on: no capacity to exceed, nothing else written
  const int64_t cap = sizing ? INT64_MAX : capacity;
  GCG_HIP_CHECK(hipMemsetAsync(s.num_runs, 0, 256, st));
  if (n_tokens > 0) {
    GCG_HIP_CHECK(hipMemsetAsync(s.key_a, 0xff, static_cast<size_t>(n_tokens) * 8, st));
    hipLaunchKernelGGL(tfidf_keys_kernel, dim3(wave_grid(n_docs)), dim3(kBlock), 0, st, n_docs,
                       n_terms, s.vbits, doc_ptr, tokens, n_tokens, rank, s.key_a);
    GCG_HIP_CHECK(hipGetLastError());
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortKeys, s.key_a, s.key_b, n, 0, s.end_bit, st)));
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRunLengthEncode::Encode, s.key_b, s.key_a, s.run_len, s.num_runs, n,
        st)));
  }
  const bool ordered = !sizing && df != nullptr && df_mode == 1 && n_tokens > 0;
  if (!sizing) {
    // the sorted keys are dead: with the ordered df the entries' columns take their region
    hipLaunchKernelGGL(tfidf_decode_kernel, dim3(grid_for(std::max<int64_t>(n_tokens, 1))),
                       dim3(256), 0, st, n_tokens, n_terms, s.vbits, s.key_a, s.run_len,
                       s.num_runs, nnz_dev, cap, indices, counts,
                       reinterpret_cast<unsigned long long*>(df), ordered ? s.cols : nullptr);
    GCG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tfidf_indptr_kernel, dim3(grid_for(n_docs + 1)), dim3(256), 0, st, n_docs,
                       s.vbits, s.key_a, s.num_runs, nnz_dev, cap, indptr);
    GCG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(tfidf_advance_kernel, dim3(1), dim3(kWave), 0, st, s.key_a, s.num_runs, cap,
                     nnz_dev, status_dev);
  GCG_HIP_CHECK(hipGetLastError());
  if (ordered) {
    // The columns were written only where the chunk fitted; a chunk that did not fit has set
    // status_dev, and the caller drops everything, df included.
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortKeys, s.cols, s.cols_sorted, n, 0, s.cbits, st)));
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRunLengthEncode::Encode, s.cols_sorted, s.term, s.term_len,
        s.num_runs + 1, n, st)));
    hipLaunchKernelGGL(tfidf_df_runs_kernel, dim3(grid_for(n_tokens)), dim3(256), 0, st, n_terms,
                       s.term, s.term_len, s.num_runs + 1,
                       reinterpret_cast<unsigned long long*>(df));
    GCG_HIP_CHECK(hipGetLastError());
  }
  return GCG_OK;
}

gcg_status gcg_tfidf_select_workspace_bytes(int64_t n_terms, size_t* bytes) {
  const char* fn = "gcg_tfidf_select_workspace_bytes";
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  SelectSpace s;
  if (const gcg_status st = select_space(fn, n_terms, nullptr, true, &s)) return st;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_tfidf_select(int64_t n_terms, const int64_t* df, int64_t lo, int64_t hi,
                            int32_t* new_id, int64_t* kept_df, int64_t* n_kept_dev,
                            void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  const char* fn = "gcg_tfidf_select";
  SelectSpace s;
  if (const gcg_status st = select_space(fn, n_terms, nullptr, false, &s)) return st;
  if (df == nullptr || new_id == nullptr || kept_df == nullptr || n_kept_dev == nullptr ||
      workspace == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL df, new_id, kept_df, n_kept_dev or workspace", fn);
  if (!aligned(df, 8) || !aligned(kept_df, 8) || !aligned(n_kept_dev, 8) || !aligned(new_id, 4) ||
      !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: a buffer is not aligned to its element size", fn);
  if (const gcg_status st = select_space(fn, n_terms, workspace, true, &s)) return st;
  if (const gcg_status st = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return st;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tfidf_keep_kernel, dim3(grid_for(n_terms)), dim3(256), 0, st, n_terms, df, lo,
                     hi, s.keep);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.keep, s.pos, static_cast<int>(n_terms), st)));
  hipLaunchKernelGGL(tfidf_renumber_kernel, dim3(grid_for(n_terms)), dim3(256), 0, st, n_terms, df,
                     s.keep, s.pos, new_id, kept_df, n_kept_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_tfidf_idf_f64(int64_t n_terms, const int64_t* df, int64_t n_docs, double* idf,
                             gcg_stream_t stream) {
  const char* fn = "gcg_tfidf_idf_f64";
  if (n_terms < 0 || n_docs < 0)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes n_terms=%lld n_docs=%lld", fn,
                static_cast<long long>(n_terms), static_cast<long long>(n_docs));
  if (n_terms == 0) return GCG_OK;
  if (df == nullptr || idf == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL df or idf", fn);
  if (!aligned(df, 8) || !aligned(idf, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: df or idf not 8-B aligned", fn);
  hipLaunchKernelGGL(tfidf_idf_kernel, dim3(grid_for(n_terms)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n_terms, df, static_cast<double>(n_docs), idf);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_tfidf_compact_workspace_bytes(int64_t n_rows, size_t* bytes) {
  const char* fn = "gcg_tfidf_compact_workspace_bytes";
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  if (n_rows < 0 || n_rows >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n_rows=%lld", fn, static_cast<long long>(n_rows));
  CompactSpace s;
  if (const gcg_status st = compact_space(fn, n_rows, nullptr, &s)) return st;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_tfidf_compact(int64_t n_rows, int64_t n_terms, int64_t nnz, const int32_t* indptr,
                             const int32_t* indices, const int32_t* counts, const int32_t* new_id,
                             int32_t* out_indptr, int32_t* out_indices, int32_t* out_counts,
                             int64_t capacity, void* workspace, size_t workspace_bytes,
                             gcg_stream_t stream) {
  const char* fn = "gcg_tfidf_compact";
  if (const gcg_status st = compact_sizes(fn, n_rows, n_terms, nnz)) return st;
  if ((out_indices == nullptr) != (out_counts == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: out_indices and out_counts are both NULL (sizing) or "
                "neither is", fn);
  const bool sizing = out_indices == nullptr;
  if (indptr == nullptr || new_id == nullptr || out_indptr == nullptr ||
      (nnz > 0 && (indices == nullptr || counts == nullptr)) || (sizing && workspace == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL indptr, indices, counts, new_id, out_indptr or "
                "workspace", fn);
  if (capacity < 0) return fail(GCG_ERR_INVALID_ARG, "%s: negative capacity", fn);
  if (!aligned(indptr, 4) || !aligned(indices, 4) || !aligned(counts, 4) || !aligned(new_id, 4) ||
      !aligned(out_indptr, 4) || !aligned(out_indices, 4) || !aligned(out_counts, 4) ||
      !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: a buffer is not aligned to its element size", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (sizing) {  // out_indptr alone: out_indptr[n_rows] is the entry count the second call needs
    CompactSpace s;
    if (const gcg_status rc = compact_space(fn, n_rows, workspace, &s)) return rc;
    if (const gcg_status rc = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return rc;
    hipLaunchKernelGGL(tfidf_row_kept_kernel, dim3(wave_grid(n_rows + 1)), dim3(kBlock), 0, st,
                       n_rows, n_terms, nnz, indptr, indices, new_id, s.len);
    GCG_HIP_CHECK(hipGetLastError());
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.len, out_indptr, static_cast<int>(n_rows + 1),
        st)));
    return GCG_OK;
  }
  if (n_rows == 0) return GCG_OK;
  hipLaunchKernelGGL(tfidf_compact_kernel, dim3(wave_grid(n_rows)), dim3(kBlock), 0, st, n_rows,
                     n_terms, nnz, indptr, indices, counts, new_id, out_indptr, capacity,
                     out_indices, out_counts);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_tfidf_weight_f32(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* indptr,
                                const int32_t* indices, const int32_t* counts, const double* idf,
                                int32_t binary, int32_t sublinear_tf, int32_t norm, float* vals,
                                gcg_stream_t stream) {
  const char* fn = "gcg_tfidf_weight_f32";
  if (const gcg_status st = compact_sizes(fn, n_rows, n_cols, nnz)) return st;
  if (norm != kNormNone && norm != kNormL1 && norm != kNormL2)
    return fail(GCG_ERR_INVALID_ARG, "%s: norm %d is none of GCG_TFIDF_NORM_*", fn,
                static_cast<int>(norm));
  if (n_rows == 0 || nnz == 0) return GCG_OK;
  if (indptr == nullptr || indices == nullptr || counts == nullptr || vals == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL indptr, indices, counts or vals", fn);
  if (!aligned(indptr, 4) || !aligned(indices, 4) || !aligned(counts, 4) || !aligned(vals, 4) ||
      !aligned(idf, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: a buffer is not aligned to its element size", fn);
  hipLaunchKernelGGL(tfidf_weight_kernel, dim3(wave_grid(n_rows)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), n_rows, n_cols, nnz, indptr, indices, counts,
                     idf, binary != 0, sublinear_tf != 0, norm, vals);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
