// graph_build.hip -- graph construction on the device: the mention-graph projection
// (data.py:226-250, gcg_project_mention_graph) and the normalized operator
// H = D^-1/2 (A+I) D^-1/2 from an undirected edge list (tensormain.py:170-181,
// gcg_normalize_adjacency_f32).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "scratch.h"

using namespace gcg;

namespace {

// ---- graph operator construction (tensormain.py:170-180) -------------------------------
// Edge (u, v) -> keys u*n+v and v*n+u, plus i*n+i for every node (setdiag(1)).
__global__ void edge_keys_kernel(int64_t n, int64_t n_edges, const int32_t* __restrict__ u,
                                 const int32_t* __restrict__ v, int self_loops,
                                 uint64_t* __restrict__ keys, int32_t* __restrict__ status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n_edges; e += stride) {
    const int64_t a = u[e], b = v[e];
    if (a < 0 || b < 0 || a >= n || b >= n) {
      atomicMax(status, int32_t(GCG_ERR_BAD_CSR));
      keys[2 * e] = keys[2 * e + 1] = static_cast<uint64_t>(n) * n;  // sorts past every real key
      continue;
    }
    keys[2 * e] = static_cast<uint64_t>(a) * n + b;
    keys[2 * e + 1] = static_cast<uint64_t>(b) * n + a;
  }
  if (self_loops)
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
      keys[2 * n_edges + i] = static_cast<uint64_t>(i) * n + i;
}

// Sorted unique keys -> CSR: indices, and row_start flags via lower bound on rows.
__global__ void keys_to_csr_kernel(int64_t n, const uint64_t* __restrict__ keys,
                                   const int64_t* __restrict__ n_unique,
                                   int32_t* __restrict__ indices) {
  const int64_t m = *n_unique;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < m; k += stride)
    indices[k] = static_cast<int32_t>(keys[k] % static_cast<uint64_t>(n));
}

__global__ void row_ptr_from_keys_kernel(int64_t n, const uint64_t* __restrict__ keys,
                                         const int64_t* __restrict__ n_unique,
                                         int32_t* __restrict__ indptr) {
  const int64_t m = *n_unique;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r <= n; r += stride) {
    const uint64_t target = static_cast<uint64_t>(r) * n;  // first key of row r
    int64_t lo = 0, hi = m;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    indptr[r] = static_cast<int32_t>(lo);
  }
}

// d_i^-1/2 in float64 exactly as numpy: 1.0 / sqrt(double(deg)), inf -> 0.
__global__ void dinv_kernel(int64_t n, const int32_t* __restrict__ indptr, double* __restrict__ dinv) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double d = static_cast<double>(indptr[i + 1] - indptr[i]);
    dinv[i] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
  }
}

// H_ij = float32( float64(d_i^-1/2 * d_j^-1/2) ): the D*adj*D entry, then .astype(float32).
__global__ void norm_vals_kernel(int64_t n, const int32_t* __restrict__ indptr,
                                 const int32_t* __restrict__ indices,
                                 const double* __restrict__ dinv, float* __restrict__ vals) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
    const double di = dinv[r];
    for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k)
      vals[k] = static_cast<float>(di * dinv[indices[k]]);
  }
}


// ---- mention-graph projection (data.py:226-250 after the celebrity filter, data.py:364-370)
// g: undirected graph over n_nodes ids; ids < n_targets are users (each with a self loop, as
// get_graph adds), ids >= n_targets are mention-only nodes. Projection: for every surviving
// node m, connect every pair of its user neighbours (m itself included when m is a user,
// through its self loop). Edges are unweighted and deduplicated.

// Incidence (a, b) -> both directed keys a*M+b, b*M+a; self pairs and bad ids -> sentinel.
__global__ void incidence_keys_kernel(int64_t n_nodes, int64_t n_inc, const int32_t* __restrict__ a,
                                      const int32_t* __restrict__ b, uint64_t* __restrict__ keys,
                                      int32_t* __restrict__ status) {
  const uint64_t M = static_cast<uint64_t>(n_nodes), sentinel = M * M;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n_inc; e += stride) {
    const int64_t x = a[e], y = b[e];
    if (x < 0 || y < 0 || x >= n_nodes || y >= n_nodes) {
      atomicMax(status, int32_t(GCG_ERR_BAD_CSR));
      keys[2 * e] = keys[2 * e + 1] = sentinel;
    } else if (x == y) {
      keys[2 * e] = keys[2 * e + 1] = sentinel;  // self loops are implicit for users
    } else {
      keys[2 * e] = static_cast<uint64_t>(x) * M + y;
      keys[2 * e + 1] = static_cast<uint64_t>(y) * M + x;
    }
  }
}

// CSR (over all M nodes) of the deduplicated keys; sentinel keys sort last and are excluded.
__global__ void adj_ptr_kernel(int64_t n_nodes, const uint64_t* __restrict__ keys,
                               const int64_t* __restrict__ n_unique, int64_t* __restrict__ ptr) {
  const uint64_t M = static_cast<uint64_t>(n_nodes);
  const int64_t m = *n_unique;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r <= n_nodes; r += stride) {
    const uint64_t target = static_cast<uint64_t>(r) * M;
    int64_t lo = 0, hi = m;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    ptr[r] = lo;
  }
}

// Per node m: alive? (users always; mention nodes iff 1 < degree <= threshold, data.py:364-369)
// and t(m) = number of user neighbours that survive, + 1 for m itself when m is a user.
__global__ void target_count_kernel(int64_t n_targets, int64_t n_nodes, int celebrity,
                                    const int64_t* __restrict__ ptr, const uint64_t* __restrict__ keys,
                                    int64_t* __restrict__ tcount, int64_t* __restrict__ npairs) {
  const uint64_t M = static_cast<uint64_t>(n_nodes);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; m < n_nodes; m += stride) {
    const int64_t deg = ptr[m + 1] - ptr[m];
    const bool alive = m < n_targets || (deg != 1 && deg <= celebrity);
    int64_t t = 0;
    if (alive) {
      for (int64_t k = ptr[m]; k < ptr[m + 1]; ++k)
        if (static_cast<int64_t>(keys[k] % M) < n_targets) ++t;
      if (m < n_targets) ++t;
    }
    tcount[m] = t;
    npairs[m] = t * (t - 1) / 2;
  }
}

// Sorted list T(m) of user neighbours (+ m itself for users) at toff[m].
__global__ void target_fill_kernel(int64_t n_targets, int64_t n_nodes, const int64_t* __restrict__ ptr,
                                   const uint64_t* __restrict__ keys, const int64_t* __restrict__ tcount,
                                   const int64_t* __restrict__ toff, int32_t* __restrict__ tlist) {
  const uint64_t M = static_cast<uint64_t>(n_nodes);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; m < n_nodes; m += stride) {
    if (tcount[m] == 0) continue;
    int64_t o = toff[m];
    bool self_done = m >= n_targets;
    for (int64_t k = ptr[m]; k < ptr[m + 1]; ++k) {
      const int64_t nb = static_cast<int64_t>(keys[k] % M);
      if (nb >= n_targets) continue;
      if (!self_done && m < nb) { tlist[o++] = static_cast<int32_t>(m); self_done = true; }
      tlist[o++] = static_cast<int32_t>(nb);
    }
    if (!self_done) tlist[o++] = static_cast<int32_t>(m);
  }
}

// Pair q of node m's list (row-major over i < j) -> key T[i]*N + T[j] (T sorted, so T[i] < T[j]).
__global__ void pair_keys_kernel(int64_t n_nodes, int64_t n_targets, int64_t total,
                                 const int64_t* __restrict__ poff, const int64_t* __restrict__ tcount,
                                 const int64_t* __restrict__ toff, const int32_t* __restrict__ tlist,
                                 uint64_t* __restrict__ keys) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < total; g += stride) {
    int64_t lo = 0, hi = n_nodes;  // last m with poff[m] <= g
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (poff[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t m = lo, t = tcount[m];
    int64_t q = g - poff[m];
    // row i holds (t - 1 - i) pairs; i from the closed form, then fixed up in integers
    double disc = static_cast<double>(2 * t - 1) * (2 * t - 1) - 8.0 * static_cast<double>(q);
    int64_t i = static_cast<int64_t>((static_cast<double>(2 * t - 1) - sqrt(disc > 0 ? disc : 0.0)) / 2.0);
    if (i < 0) i = 0;
    auto row_start = [t](int64_t r) { return r * (2 * t - r - 1) / 2; };
    while (i > 0 && row_start(i) > q) --i;
    while (i + 1 < t && row_start(i + 1) <= q) ++i;
    const int64_t j = i + 1 + (q - row_start(i));
    const int64_t base = toff[m];
    keys[g] = static_cast<uint64_t>(tlist[base + i]) * static_cast<uint64_t>(n_targets) +
              static_cast<uint64_t>(tlist[base + j]);
  }
}

__global__ void decode_pairs_kernel(int64_t n_targets, const uint64_t* __restrict__ keys,
                                    const int64_t* __restrict__ n_unique, int32_t* __restrict__ u,
                                    int32_t* __restrict__ v) {
  const int64_t m = *n_unique;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < m; k += stride) {
    u[k] = static_cast<int32_t>(keys[k] / static_cast<uint64_t>(n_targets));
    v[k] = static_cast<int32_t>(keys[k] % static_cast<uint64_t>(n_targets));
  }
}

// The scratch of the normalisation: the m edge keys, their sorted copy (then the unique keys go
// back to `keys`), the n inverse root degrees, hipcub's temporary. take_exact: no edge or no
// node, empty arrays.
struct NormSpace {
  uint64_t *keys, *sorted;
  double* dinv;
  Tmp tmp;
  size_t total;
};

gcg_status norm_space(const char* fn, int64_t n, int64_t m, int end_bit, int64_t* nnz_dev,
                      void* workspace, NormSpace* s) {
  Carver cv(workspace);
  s->keys = cv.take_exact<uint64_t>(m);
  s->sorted = cv.take_exact<uint64_t>(m);
  s->dinv = cv.take_exact<double>(n);
  TmpSize ts;
  ts.add(GCG_CUB(DeviceRadixSort::SortKeys, s->keys, s->sorted, static_cast<int>(m), 0, end_bit));
  ts.add(GCG_CUB(DeviceSelect::Unique, s->sorted, s->keys, nnz_dev, static_cast<int>(m)));
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}
}  // namespace

extern "C" {

gcg_status gcg_normalize_adjacency_f32(int64_t n, int64_t n_edges, const int32_t* u,
                                       const int32_t* v, int self_loops, int32_t* indptr,
                                       int32_t* indices, float* vals, int64_t* nnz_dev,
                                       void* workspace, size_t workspace_bytes,
                                       size_t* workspace_needed, int32_t* status_dev,
                                       gcg_stream_t stream) {
  if (n < 0 || n >= INT32_MAX || n_edges < 0 || (n > 0 && static_cast<double>(n) * n > 1.8e19))
    return fail(GCG_ERR_INVALID_ARG, "bad sizes");
  const int64_t m = 2 * n_edges + (self_loops ? n : 0);
  if (m > INT32_MAX) return fail(GCG_ERR_INVALID_ARG, "too many entries for int32 CSR");
  const char* fn = "gcg_normalize_adjacency_f32";
  const int end_bit = bits_to_hold(static_cast<uint64_t>(n) * n);
  NormSpace s;
  if (gcg_status rc = norm_space(fn, n, m, end_bit, nnz_dev, workspace, &s)) return rc;
  if (workspace_needed) *workspace_needed = s.total;
  if (indptr == nullptr && indices == nullptr && vals == nullptr) return GCG_OK;  // sizing
  if (indptr == nullptr || nnz_dev == nullptr || status_dev == nullptr ||
      (m > 0 && (indices == nullptr || vals == nullptr)) || (n_edges > 0 && (u == nullptr || v == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "NULL buffer");
  // (the entry has never asked the workspace for an alignment: 1)
  if (gcg_status rc = check_workspace(fn, workspace, workspace_bytes, s.total, 1)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint64_t *keys = s.keys, *sorted = s.sorted;
  double* dinv = s.dinv;
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  GCG_HIP_CHECK(hipMemsetAsync(nnz_dev, 0, sizeof(int64_t), st));
  if (m > 0) {
    hipLaunchKernelGGL(edge_keys_kernel, dim3(grid_for(std::max(n_edges, n))), dim3(256), 0, st, n,
                       n_edges, u, v, self_loops, keys, status_dev);
    GCG_HIP_CHECK(hipGetLastError());
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortKeys, keys, sorted, static_cast<int>(m), 0, end_bit,
        st)));
    // Duplicate edges collapse (binary adjacency, as networkx holds one edge per pair).
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceSelect::Unique, sorted, keys, nnz_dev, static_cast<int>(m), st)));
    hipLaunchKernelGGL(keys_to_csr_kernel, dim3(grid_for(m)), dim3(256), 0, st, n, keys, nnz_dev, indices);
    GCG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(row_ptr_from_keys_kernel, dim3(grid_for(n + 1)), dim3(256), 0, st, n, keys,
                     nnz_dev, indptr);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(dinv_kernel, dim3(grid_for(n)), dim3(256), 0, st, n, indptr, dinv);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(norm_vals_kernel, dim3(grid_for(n)), dim3(256), 0, st, n, indptr, indices, dinv, vals);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_project_mention_graph(int64_t n_targets, int64_t n_nodes, int64_t n_inc,
                                     const int32_t* a, const int32_t* b, int celebrity_threshold,
                                     int32_t* out_u, int32_t* out_v, int64_t capacity,
                                     int64_t* n_edges, int32_t* status_dev, gcg_stream_t stream) {
  if (n_targets < 0 || n_nodes < n_targets || n_nodes >= INT32_MAX || n_inc < 0 ||
      n_edges == nullptr || status_dev == nullptr || (n_inc > 0 && (a == nullptr || b == nullptr)) ||
      2 * n_inc > INT32_MAX || (out_u == nullptr) != (out_v == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "bad args to gcg_project_mention_graph");
  const bool sizing = out_u == nullptr;
  *n_edges = 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (n_targets < 2) return GCG_OK;
  const int64_t m2 = 2 * n_inc;
  const uint64_t M = static_cast<uint64_t>(n_nodes);
  const char* fn = "gcg_project_mention_graph";
  const int adj_bits = bits_to_hold(M * M);
  // 1. symmetric, deduplicated adjacency of g
  uint64_t *keys = nullptr, *keys2 = nullptr;
  int64_t *cnt = nullptr, *ptr = nullptr, *tcount = nullptr, *npairs = nullptr, *toff = nullptr,
          *poff = nullptr;
  Tmp tmp;
  const int n = static_cast<int>(std::max<int64_t>(m2, 1));
  TmpSize ts;
  ts.add(GCG_CUB(DeviceRadixSort::SortKeys, keys, keys2, n, 0, adj_bits));
  ts.add(GCG_CUB(DeviceSelect::Unique, keys2, keys, cnt, n));
  ts.add(GCG_CUB(DeviceScan::ExclusiveSum, tcount, toff, static_cast<int>(n_nodes)));
  if (gcg_status rc = ts.status(fn)) return rc;
  DevMem mem;
  GCG_HIP_CHECK(alloc_carved(mem, st, [&](Carver& cv) {
    keys = cv.take<uint64_t>(m2);
    keys2 = cv.take<uint64_t>(m2);
    cnt = cv.take<int64_t>(2);
    ptr = cv.take<int64_t>(n_nodes + 1);
    tcount = cv.take<int64_t>(n_nodes);
    npairs = cv.take<int64_t>(n_nodes);
    toff = cv.take<int64_t>(n_nodes);
    poff = cv.take<int64_t>(n_nodes);
    tmp = {cv.take<char>(ts.bytes), ts.bytes};
  }));
  GCG_HIP_CHECK(hipMemsetAsync(cnt, 0, 2 * sizeof(int64_t), st));
  if (m2 > 0) {
    hipLaunchKernelGGL(incidence_keys_kernel, dim3(grid_for(n_inc)), dim3(256), 0, st, n_nodes, n_inc, a, b,
                       keys, status_dev);
    GCG_HIP_CHECK(hipGetLastError());
    GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceRadixSort::SortKeys, keys, keys2, static_cast<int>(m2), 0, adj_bits,
        st)));
    GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceSelect::Unique, keys2, keys, cnt, static_cast<int>(m2), st)));
  }
  hipLaunchKernelGGL(adj_ptr_kernel, dim3(grid_for(n_nodes + 1)), dim3(256), 0, st, n_nodes, keys, cnt,
                     ptr);
  // 2-3. celebrity filter, user-neighbour lists, pair counts
  hipLaunchKernelGGL(target_count_kernel, dim3(grid_for(n_nodes)), dim3(256), 0, st, n_targets, n_nodes,
                     celebrity_threshold, ptr, keys, tcount, npairs);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, tcount, toff, static_cast<int>(n_nodes), st)));
  GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, npairs, poff, static_cast<int>(n_nodes), st)));
  int64_t last[4] = {0, 0, 0, 0};  // toff[M-1], tcount[M-1], poff[M-1], npairs[M-1]
  GCG_HIP_CHECK(hipMemcpyAsync(&last[0], toff + n_nodes - 1, 8, hipMemcpyDeviceToHost, st));
  GCG_HIP_CHECK(hipMemcpyAsync(&last[1], tcount + n_nodes - 1, 8, hipMemcpyDeviceToHost, st));
  GCG_HIP_CHECK(hipMemcpyAsync(&last[2], poff + n_nodes - 1, 8, hipMemcpyDeviceToHost, st));
  GCG_HIP_CHECK(hipMemcpyAsync(&last[3], npairs + n_nodes - 1, 8, hipMemcpyDeviceToHost, st));
  GCG_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t n_tlist = last[0] + last[1], P = last[2] + last[3];
  if (sizing) {  // capacity query: the number of pairs bounds the number of edges
    *n_edges = P;
    return GCG_OK;
  }
  if (P == 0) return GCG_OK;
  if (P > INT32_MAX) return fail(GCG_ERR_INVALID_ARG, "%lld projected pairs exceed the int32 sort range", (long long)P);
  // 4 needs the pairs' keys, their sorted copy and hipcub's temporary to dedupe them
  const uint64_t N = static_cast<uint64_t>(n_targets);
  const int pair_bits = bits_to_hold(N * N);
  int32_t* tlist = nullptr;
  uint64_t *pk = nullptr, *pk2 = nullptr;
  int64_t* ucnt = nullptr;
  Tmp tmp2;
  TmpSize ts2;
  ts2.add(GCG_CUB(DeviceRadixSort::SortKeys, pk, pk2, static_cast<int>(P), 0, pair_bits));
  ts2.add(GCG_CUB(DeviceSelect::Unique, pk2, pk, ucnt, static_cast<int>(P)));
  if (gcg_status rc = ts2.status(fn)) return rc;
  DevMem mem2;
  GCG_HIP_CHECK(alloc_carved(mem2, st, [&](Carver& cv) {
    tlist = cv.take<int32_t>(n_tlist);
    pk = cv.take<uint64_t>(P);
    pk2 = cv.take<uint64_t>(P);
    ucnt = cv.take<int64_t>(1);
    tmp2 = {cv.take<char>(ts2.bytes), ts2.bytes};
  }));
  hipLaunchKernelGGL(target_fill_kernel, dim3(grid_for(n_nodes)), dim3(256), 0, st, n_targets, n_nodes,
                     ptr, keys, tcount, toff, tlist);
  hipLaunchKernelGGL(pair_keys_kernel, dim3(grid_for(P)), dim3(256), 0, st, n_nodes, n_targets, P,
                     poff, tcount, toff, tlist, pk);
  GCG_HIP_CHECK(hipGetLastError());
  // 4. dedupe pairs
  GCG_HIP_CHECK(tmp2.run(GCG_CUB(DeviceRadixSort::SortKeys, pk, pk2, static_cast<int>(P), 0, pair_bits, st)));
  GCG_HIP_CHECK(tmp2.run(GCG_CUB(DeviceSelect::Unique, pk2, pk, ucnt, static_cast<int>(P), st)));
  int64_t n_unique = 0;
  GCG_HIP_CHECK(hipMemcpyAsync(&n_unique, ucnt, 8, hipMemcpyDeviceToHost, st));
  GCG_HIP_CHECK(hipStreamSynchronize(st));
  if (n_unique > capacity)
    return fail(GCG_ERR_WORKSPACE, "output capacity %lld < %lld edges", (long long)capacity, (long long)n_unique);
  hipLaunchKernelGGL(decode_pairs_kernel, dim3(grid_for(n_unique)), dim3(256), 0, st, n_targets, pk, ucnt,
                     out_u, out_v);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(hipStreamSynchronize(st));
  *n_edges = n_unique;
  return GCG_OK;
}

}  // extern "C"
