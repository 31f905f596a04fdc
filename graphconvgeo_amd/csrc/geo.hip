// geo.hip -- the geolocation side of the model (include/gcg_spmm.h): the k-d-tree region
// labels of KDTreeClustering (kdtree.py:84-151), the per-class medians and the brute-force
// nearest class of DataLoader.assignClasses (data.py:399-419), the haversine distance and
// tensormain.geo_eval's distances and Acc@161 count (tensormain.py:38-54). All float64.
//
// The tree is built level by level. Every node is a contiguous segment [head, end) of two
// id lists, one sorted by latitude and one by longitude inside every segment, so a node's
// bounds are its segment ends and its median is its middle. A split partitions both lists
// stably by `value[dim] > split` (left child first), which keeps them sorted inside the
// children; the final segment order is the reference's pre-order leaf numbering.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "haversine.h"
#include "scratch.h"
#include "segment_kernels.h"

using namespace gcg;

namespace {

// medians staged per LDS tile of nearest_class_kernel: 3 doubles each, 48 KiB, so two
// workgroups still share a CU's LDS
constexpr int kClassTile = 2048;

// locs (N x 2 row-major) -> vals[0..N) latitudes, vals[N..2N) longitudes; ids = 0..N-1;
// a non-finite coordinate raises *status.
__global__ void split_coords_kernel(int64_t N, const double* __restrict__ locs,
                                    double* __restrict__ vals, int32_t* __restrict__ ids,
                                    int32_t* __restrict__ status) {
  for (int64_t i = grid_start(); i < N; i += grid_stride()) {
    const double la = locs[2 * i], lo = locs[2 * i + 1];
    if (!isfinite(la) || !isfinite(lo)) *status = 1;
    vals[i] = la;
    vals[N + i] = lo;
    ids[i] = static_cast<int32_t>(i);
  }
}

__global__ void tree_init_kernel(int64_t N, int32_t* __restrict__ head, int32_t* __restrict__ end,
                                 int32_t* __restrict__ done) {
  for (int64_t p = grid_start(); p < N; p += grid_stride()) {
    head[p] = 0;
    if (p == 0) {
      end[0] = static_cast<int32_t>(N);
      done[0] = 0;
    }
  }
}

// np.median of the sorted run ids[s, s + n) of v: the middle value, or (a + b) / 2.
// v[stride * id] is point id's coordinate.
__device__ __forceinline__ double sorted_median(const double* __restrict__ v, int64_t stride,
                                                const int32_t* __restrict__ ids, int64_t s,
                                                int64_t n) {
  const int64_t m = s + n / 2;
  if (n & 1) return v[stride * ids[m]];
  return (v[stride * ids[m - 1]] + v[stride * ids[m]]) / 2.0;
}

// One thread per position; the thread at an open node's head decides the node
// (kdtree.py:85-95): leaf, or (dim, split). *any_split: 1 when some node splits; 2 when the
// input check failed, which the root's thread reports on the first level, where it is the only
// node (so the level's one readback carries both).
__global__ void tree_node_kernel(int64_t N, int64_t bucket, const double* __restrict__ vals,
                                 const int32_t* __restrict__ ids0,
                                 const int32_t* __restrict__ ids1,
                                 const int32_t* __restrict__ head, const int32_t* __restrict__ end,
                                 int32_t* __restrict__ done, int32_t* __restrict__ dim,
                                 double* __restrict__ split, int32_t* __restrict__ any_split,
                                 const int32_t* __restrict__ status) {
  for (int64_t p = grid_start(); p < N; p += grid_stride()) {
    if (head[p] != p || done[p]) continue;
    if (p == 0 && *status != 0) {
      *any_split = 2;
      continue;
    }
    const int64_t e = end[p], n = e - p;
    bool leaf = n <= bucket;
    if (!leaf) {
      const double* v0 = vals;
      const double* v1 = vals + N;
      const double min0 = v0[ids0[p]], max0 = v0[ids0[e - 1]];
      const double min1 = v1[ids1[p]], max1 = v1[ids1[e - 1]];
      const int d = (max1 - min1 > max0 - min0) ? 1 : 0;  // np.argmax: a tie gives axis 0
      const double mn = d ? min1 : min0, mx = d ? max1 : max0;
      if (mn == mx) {
        leaf = true;  // zero width: the node stays a leaf however full it is
      } else {
        double s = sorted_median(d ? v1 : v0, 1, d ? ids1 : ids0, p, n);
        // kdtree.py:94-95 (split == max -> min); the same for a midpoint that left [min, max)
        // by overflow, so both children are non-empty whatever the input
        if (!(s >= mn && s < mx)) s = mn;
        dim[p] = d;
        split[p] = s;
        *any_split = 1;
      }
    }
    if (leaf) {
      done[p] = 1;
      dim[p] = -1;
    }
  }
}

// flags[L * (N + 1) + p] = 1 when the point at position p of list L goes to the right child.
__global__ void tree_flag_kernel(int64_t N, const double* __restrict__ vals,
                                 const int32_t* __restrict__ ids0,
                                 const int32_t* __restrict__ ids1,
                                 const int32_t* __restrict__ head, const int32_t* __restrict__ dim,
                                 const double* __restrict__ split, int32_t* __restrict__ flags) {
  for (int64_t q = grid_start(); q < 2 * N; q += grid_stride()) {
    const int64_t L = q >= N, p = q - L * N;
    const int32_t h = head[p], d = dim[h];
    int32_t f = 0;
    if (d >= 0) f = vals[d * N + (L ? ids1 : ids0)[p]] > split[h];
    flags[L * (N + 1) + p] = f;
    if (p == 0) flags[L * (N + 1) + N] = 0;
  }
}

// Stable partition of both lists inside every split node from the exclusive scan `ex` of the
// flags; the node's head thread (list 0) opens the two children.
__global__ void tree_scatter_kernel(int64_t N, const int32_t* __restrict__ flags,
                                    const int32_t* __restrict__ ex,
                                    const int32_t* __restrict__ ids0,
                                    const int32_t* __restrict__ ids1,
                                    const int32_t* __restrict__ head, const int32_t* __restrict__ end,
                                    const int32_t* __restrict__ dim, int32_t* __restrict__ ids0_out,
                                    int32_t* __restrict__ ids1_out, int32_t* __restrict__ head_out,
                                    int32_t* __restrict__ end_out, int32_t* __restrict__ done) {
  for (int64_t q = grid_start(); q < 2 * N; q += grid_stride()) {
    const int64_t L = q >= N, p = q - L * N, b = L * (N + 1);
    const int32_t h = head[p], e = end[h];
    int32_t pos = static_cast<int32_t>(p), new_head = h;
    if (dim[h] >= 0) {
      const int32_t ones_before = ex[b + p] - ex[b + h];
      const int32_t ones = ex[b + e] - ex[b + h];
      const int32_t mid = e - ones;  // the right child's head
      if (flags[b + p]) {
        pos = mid + ones_before;
        new_head = mid;
      } else {
        pos = static_cast<int32_t>(p) - ones_before;
      }
      if (L == 0 && p == h) {
        end_out[h] = mid;
        end_out[mid] = e;
        done[mid] = 0;
      }
    } else if (L == 0 && p == h) {
      end_out[h] = e;
    }
    if (L) {
      ids1_out[pos] = ids1[p];
    } else {
      ids0_out[pos] = ids0[p];
      head_out[pos] = new_head;
    }
  }
}

__global__ void tree_head_flag_kernel(int64_t N, const int32_t* __restrict__ head,
                                      int32_t* __restrict__ flags) {
  for (int64_t p = grid_start(); p < N; p += grid_stride()) flags[p] = head[p] == p;
}

// inc = inclusive scan of the head flags: position p lies in leaf inc[p] - 1.
__global__ void tree_label_kernel(int64_t N, const int32_t* __restrict__ inc,
                                  const int32_t* __restrict__ head,
                                  const int32_t* __restrict__ ids0, int32_t* __restrict__ labels,
                                  int32_t* __restrict__ leaf_ptr, int64_t* __restrict__ n_leaves) {
  for (int64_t p = grid_start(); p < N; p += grid_stride()) {
    const int32_t c = inc[p] - 1;
    labels[ids0[p]] = c;
    if (head[p] == p) leaf_ptr[c] = static_cast<int32_t>(p);
    if (p == N - 1) {
      leaf_ptr[c + 1] = static_cast<int32_t>(N);
      *n_leaves = c + 1;
    }
  }
}

// out[c] = (median latitude, median longitude) of segment c of the two sorted lists.
__global__ void segment_medians_kernel(int64_t C, int64_t N, const double* __restrict__ lat,
                                       const double* __restrict__ lon, int64_t stride,
                                       const int32_t* __restrict__ ptr,
                                       const int32_t* __restrict__ perm_lat,
                                       const int32_t* __restrict__ perm_lon,
                                       double* __restrict__ out) {
  for (int64_t c = grid_start(); c < C; c += grid_stride()) {
    const int64_t s = ptr[c], n = ptr[c + 1] - s;
    const bool ok = n > 0 && s >= 0 && s + n <= N;
    out[2 * c] = ok ? sorted_median(lat, stride, perm_lat, s, n) : NAN;
    out[2 * c + 1] = ok ? sorted_median(lon, stride, perm_lon, s, n) : NAN;
  }
}

// keys[p] = labels[ids[p]] (a label outside [0, C) raises *status and sorts as class 0).
__global__ void gather_labels_kernel(int64_t N, int64_t C, const int32_t* __restrict__ labels,
                                     const int32_t* __restrict__ ids, int32_t* __restrict__ keys,
                                     int32_t* __restrict__ status) {
  for (int64_t p = grid_start(); p < N; p += grid_stride()) {
    int32_t l = labels[ids[p]];
    if (l < 0 || l >= C) {
      *status = 1;
      l = 0;
    }
    keys[p] = l;
  }
}

// (haversine_rad, the distance itself: haversine.h)
__global__ void haversine_kernel(int64_t M, const double* __restrict__ A,
                                 const double* __restrict__ B, double two_r,
                                 double* __restrict__ out) {
  for (int64_t i = grid_start(); i < M; i += grid_stride()) {
    const double lat1 = A[2 * i] * kDegToRad, lat2 = B[2 * i] * kDegToRad;
    out[i] = haversine_rad(lat1, cos(lat1), A[2 * i + 1] * kDegToRad, lat2, cos(lat2),
                           B[2 * i + 1] * kDegToRad, two_r);
  }
}

// One query per thread; the medians pass through LDS in tiles of kClassTile (radians and
// cos(lat) precomputed once per workgroup), each query keeping its running (distance, index)
// minimum: strict < keeps the first index on a tie.
__global__ __launch_bounds__(256) void nearest_class_kernel(int64_t M, int64_t C,
                                                            const double* __restrict__ locs,
                                                            const double* __restrict__ medians,
                                                            double two_r, int32_t* __restrict__ idx,
                                                            double* __restrict__ dist) {
  __shared__ double s_lat[kClassTile], s_lng[kClassTile], s_cos[kClassTile];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool active = i < M;
  double lat1 = 0.0, lng1 = 0.0, cos1 = 1.0;
  if (active) {
    lat1 = locs[2 * i] * kDegToRad;
    lng1 = locs[2 * i + 1] * kDegToRad;
    cos1 = cos(lat1);
  }
  double best = INFINITY;
  int32_t best_c = 0;
  for (int64_t t0 = 0; t0 < C; t0 += kClassTile) {
    const int tn = static_cast<int>(min(static_cast<int64_t>(kClassTile), C - t0));
    __syncthreads();
    for (int j = threadIdx.x; j < tn; j += 256) {
      const double la = medians[2 * (t0 + j)] * kDegToRad;
      s_lat[j] = la;
      s_lng[j] = medians[2 * (t0 + j) + 1] * kDegToRad;
      s_cos[j] = cos(la);
    }
    __syncthreads();
    if (active) {
      for (int j = 0; j < tn; ++j) {
        const double d = haversine_rad(lat1, cos1, lng1, s_lat[j], s_cos[j], s_lng[j], two_r);
        if (d < best) {
          best = d;
          best_c = static_cast<int32_t>(t0 + j);
        }
      }
    }
  }
  if (active) {
    idx[i] = best_c;
    if (dist != nullptr) dist[i] = best;
  }
}

// dist[i] = distance from locs[i] to the median of its predicted class; *count += rows under
// the threshold (strict <). A prediction outside [0, C) raises *status (its distance is NaN).
template <typename P>
__global__ __launch_bounds__(256) void geo_eval_kernel(int64_t M, int64_t C,
                                                       const P* __restrict__ pred,
                                                       const double* __restrict__ locs,
                                                       const double* __restrict__ medians,
                                                       double two_r, double threshold,
                                                       double* __restrict__ dist,
                                                       unsigned long long* __restrict__ count,
                                                       int32_t* __restrict__ status) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  int under = 0;
  if (i < M) {
    const int64_t c = static_cast<int64_t>(pred[i]);
    double d = NAN;
    if (c < 0 || c >= C) {
      *status = 1;
    } else {
      const double lat1 = locs[2 * i] * kDegToRad, lat2 = medians[2 * c] * kDegToRad;
      d = haversine_rad(lat1, cos(lat1), locs[2 * i + 1] * kDegToRad, lat2, cos(lat2),
                        medians[2 * c + 1] * kDegToRad, two_r);
      under = d < threshold;
    }
    dist[i] = d;
  }
  const int n = __syncthreads_count(under);
  if (threadIdx.x == 0 && n > 0) atomicAdd(count, static_cast<unsigned long long>(n));
}

constexpr int64_t kMaxPoints = (int64_t{1} << 30) - 2;  // 2N + 2 scan items fit int32

bool radius_ok(double r) { return std::isfinite(r) && r > 0.0; }

}  // namespace

extern "C" {

gcg_status gcg_kdtree_fit_f64(int64_t N, const double* locs, int64_t bucket_size,
                              int32_t* labels, int32_t* perm_lat, int32_t* perm_lon,
                              int32_t* leaf_ptr, int64_t* n_clusters_host, int64_t* depth_host,
                              int64_t* readbacks_host, int32_t* status_dev, gcg_stream_t stream) {
  if (N < 0 || N > kMaxPoints)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kdtree_fit_f64: bad N=%lld", static_cast<long long>(N));
  if (bucket_size < 1)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kdtree_fit_f64: bucket_size=%lld < 1",
                static_cast<long long>(bucket_size));
  if (n_clusters_host == nullptr || status_dev == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kdtree_fit_f64: null n_clusters_host / status_dev");
  *n_clusters_host = 0;
  if (depth_host) *depth_host = 0;
  if (readbacks_host) *readbacks_host = 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N == 0) {
    GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
    return GCG_OK;
  }
  if (locs == nullptr || labels == nullptr || perm_lat == nullptr || perm_lon == nullptr ||
      leaf_ptr == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kdtree_fit_f64: null operand");
  if (!aligned(locs, 8) || !aligned(labels, 4) || !aligned(perm_lat, 4) || !aligned(perm_lon, 4) ||
      !aligned(leaf_ptr, 4) || !aligned(status_dev, 4))
    return fail(GCG_ERR_MISALIGNED, "gcg_kdtree_fit_f64: operand not aligned to its element");
  const int n = static_cast<int>(N), n_scan = 2 * n + 2;
  const size_t ib = static_cast<size_t>(N) * sizeof(int32_t);
  double *vals = nullptr, *keys = nullptr, *split = nullptr;
  int32_t *iota = nullptr, *ids[2][2] = {}, *head[2] = {}, *end[2] = {}, *done = nullptr,
          *dim = nullptr, *flags = nullptr, *ex = nullptr, *any_split = nullptr;
  int64_t* n_leaves = nullptr;
  Tmp tmp;
  TmpSize ts;
  ts.add(GCG_CUB(DeviceRadixSort::SortPairs, vals, keys, iota, ids[0][0], n));
  ts.add(GCG_CUB(DeviceScan::ExclusiveSum, flags, ex, n_scan));
  ts.add(GCG_CUB(DeviceScan::InclusiveSum, flags, ex, n));
  if (gcg_status rc = ts.status("gcg_kdtree_fit_f64")) return rc;
  DevMem mem;
  GCG_HIP_CHECK(alloc_carved(mem, st, [&](Carver& cv) {
    vals = cv.take<double>(2 * N);
    keys = cv.take<double>(N);
    iota = cv.take<int32_t>(N);
    for (auto& pair : ids)
      for (auto& m : pair) m = cv.take<int32_t>(N);
    for (auto& m : head) m = cv.take<int32_t>(N);
    for (auto& m : end) m = cv.take<int32_t>(N);
    done = cv.take<int32_t>(N);
    dim = cv.take<int32_t>(N);
    split = cv.take<double>(N);
    flags = cv.take<int32_t>(n_scan);
    ex = cv.take<int32_t>(n_scan);
    any_split = cv.take<int32_t>(1);
    n_leaves = cv.take<int64_t>(1);
    tmp = {cv.take<char>(ts.bytes), ts.bytes};
  }));
  const dim3 g1(grid_for(N)), g2(grid_for(2 * N)), blk(256);

  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(split_coords_kernel, g1, blk, 0, st, N, locs, vals, iota, status_dev);
  GCG_HIP_CHECK(hipGetLastError());
  // presort: ids[d][0] = the point ids by coordinate d
  for (int d = 0; d < 2; ++d) {
    GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, vals + d * N, keys, iota, ids[d][0], n, 0, 64,
        st)));
  }
  hipLaunchKernelGGL(tree_init_kernel, g1, blk, 0, st, N, head[0], end[0], done);
  GCG_HIP_CHECK(hipGetLastError());

  int cur = 0;
  int64_t depth = 0, readbacks = 0;
  for (;;) {
    GCG_HIP_CHECK(hipMemsetAsync(any_split, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(tree_node_kernel, g1, blk, 0, st, N, bucket_size, vals,
                       ids[0][cur], ids[1][cur], head[cur], end[cur], done, dim, split, any_split,
                       status_dev);
    GCG_HIP_CHECK(hipGetLastError());
    // the level's one scalar readback: did any node split (2: the input check failed)
    int32_t host = 0;
    GCG_HIP_CHECK(hipMemcpyAsync(&host, any_split, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GCG_HIP_CHECK(hipStreamSynchronize(st));
    ++readbacks;
    if (host == 2) {
      if (readbacks_host) *readbacks_host = readbacks;
      return fail(GCG_ERR_INVALID_ARG, "gcg_kdtree_fit_f64: non-finite coordinate");
    }
    if (host == 0) break;
    if (++depth > N) return fail(GCG_ERR_HIP, "gcg_kdtree_fit_f64: tree deeper than N");
    const int nxt = cur ^ 1;
    hipLaunchKernelGGL(tree_flag_kernel, g2, blk, 0, st, N, vals, ids[0][cur],
                       ids[1][cur], head[cur], dim, split, flags);
    GCG_HIP_CHECK(hipGetLastError());
    GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, flags, ex, n_scan, st)));
    hipLaunchKernelGGL(tree_scatter_kernel, g2, blk, 0, st, N, flags, ex, ids[0][cur],
                       ids[1][cur], head[cur], end[cur], dim, ids[0][nxt], ids[1][nxt], head[nxt],
                       end[nxt], done);
    GCG_HIP_CHECK(hipGetLastError());
    cur = nxt;
  }
  // leaves in segment order = the reference's pre-order numbering
  hipLaunchKernelGGL(tree_head_flag_kernel, g1, blk, 0, st, N, head[cur], flags);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceScan::InclusiveSum, flags, ex, n, st)));
  hipLaunchKernelGGL(tree_label_kernel, g1, blk, 0, st, N, ex, head[cur],
                     ids[0][cur], labels, leaf_ptr, n_leaves);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(hipMemcpyAsync(perm_lat, ids[0][cur], ib, hipMemcpyDeviceToDevice, st));
  GCG_HIP_CHECK(hipMemcpyAsync(perm_lon, ids[1][cur], ib, hipMemcpyDeviceToDevice, st));
  int64_t nl = 0;
  GCG_HIP_CHECK(hipMemcpyAsync(&nl, n_leaves, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  GCG_HIP_CHECK(hipStreamSynchronize(st));
  ++readbacks;
  *n_clusters_host = nl;
  if (depth_host) *depth_host = depth;
  if (readbacks_host) *readbacks_host = readbacks;
  return GCG_OK;
}

gcg_status gcg_segment_medians_f64(int64_t C, int64_t N, const double* locs, const int32_t* ptr,
                                   const int32_t* perm_lat, const int32_t* perm_lon,
                                   double* medians, gcg_stream_t stream) {
  if (C < 0 || N < 0 || N > kMaxPoints || C > INT32_MAX - 1)
    return fail(GCG_ERR_INVALID_ARG, "gcg_segment_medians_f64: bad sizes");
  if (C == 0) return GCG_OK;
  if (ptr == nullptr || medians == nullptr ||
      (N > 0 && (locs == nullptr || perm_lat == nullptr || perm_lon == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_segment_medians_f64: null operand");
  if (!aligned(locs, 8) || !aligned(medians, 8) || !aligned(ptr, 4) || !aligned(perm_lat, 4) ||
      !aligned(perm_lon, 4))
    return fail(GCG_ERR_MISALIGNED, "gcg_segment_medians_f64: operand not aligned to its element");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(segment_medians_kernel, dim3(grid_for(C)), dim3(256), 0, st, C, N, locs,
                     locs + 1, int64_t{2}, ptr, perm_lat, perm_lon, medians);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_class_medians_f64(int64_t N, const double* locs, const int32_t* labels, int64_t C,
                                 double* medians, int32_t* status_dev, gcg_stream_t stream) {
  if (N < 0 || N > kMaxPoints || C < 0 || C > INT32_MAX - 1)
    return fail(GCG_ERR_INVALID_ARG, "gcg_class_medians_f64: bad sizes");
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_class_medians_f64: null status_dev");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (C == 0) {
    if (N > 0) return fail(GCG_ERR_INVALID_ARG, "gcg_class_medians_f64: points but no class");
    return GCG_OK;
  }
  if (medians == nullptr || (N > 0 && (locs == nullptr || labels == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_class_medians_f64: null operand");
  if (!aligned(locs, 8) || !aligned(medians, 8) || !aligned(labels, 4) || !aligned(status_dev, 4))
    return fail(GCG_ERR_MISALIGNED, "gcg_class_medians_f64: operand not aligned to its element");
  const int n = static_cast<int>(N);
  const int lbits = bits_to_count(C);
  double *vals = nullptr, *keys = nullptr;
  int32_t *iota = nullptr, *by_val = nullptr, *lab = nullptr, *lab_sorted = nullptr,
          *perm[2] = {}, *ptr = nullptr;
  Tmp tmp;
  TmpSize ts;
  if (N > 0) {
    ts.add(GCG_CUB(DeviceRadixSort::SortPairs, vals, keys, iota, by_val, n));
    ts.add(GCG_CUB(DeviceRadixSort::SortPairs, lab, lab_sorted, by_val, perm[0], n, 0, lbits));
    if (gcg_status rc = ts.status("gcg_class_medians_f64")) return rc;
  }
  DevMem mem;
  GCG_HIP_CHECK(alloc_carved(mem, st, [&](Carver& cv) {
    vals = cv.take<double>(2 * N);
    keys = cv.take<double>(N);
    iota = cv.take<int32_t>(N);
    by_val = cv.take<int32_t>(N);
    lab = cv.take<int32_t>(N);
    lab_sorted = cv.take<int32_t>(N);
    for (auto& m : perm) m = cv.take<int32_t>(N);
    ptr = cv.take<int32_t>(C + 1);
    tmp = {cv.take<char>(ts.bytes), ts.bytes};
  }));
  const dim3 g1(grid_for(N)), blk(256);
  if (N > 0) {
    hipLaunchKernelGGL(split_coords_kernel, g1, blk, 0, st, N, locs, vals, iota,
                       status_dev);
    GCG_HIP_CHECK(hipGetLastError());
    // by value, then (stably) by class: each class's run is sorted by the coordinate
    for (int d = 0; d < 2; ++d) {
      GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, vals + d * N, keys, iota, by_val, n, 0, 64,
          st)));
      hipLaunchKernelGGL(gather_labels_kernel, g1, blk, 0, st, N, C, labels, by_val, lab,
                         status_dev);
      GCG_HIP_CHECK(hipGetLastError());
      GCG_HIP_CHECK(tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, lab, lab_sorted, by_val, perm[d], n, 0, lbits,
          st)));
    }
  }
  hipLaunchKernelGGL(class_ptr_kernel, dim3(grid_for(N + 1)), blk, 0, st, N, C, lab_sorted,
                     ptr);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(segment_medians_kernel, dim3(grid_for(C)), blk, 0, st, C, N,
                     vals, vals + N, int64_t{1}, ptr, perm[0], perm[1], medians);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_haversine_km_f64(int64_t M, const double* a, const double* b,
                                double earth_radius_km, double* out, gcg_stream_t stream) {
  if (M < 0 || !radius_ok(earth_radius_km))
    return fail(GCG_ERR_INVALID_ARG, "gcg_haversine_km_f64: bad M or radius");
  if (M == 0) return GCG_OK;
  if (a == nullptr || b == nullptr || out == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_haversine_km_f64: null operand");
  if (!aligned(a, 8) || !aligned(b, 8) || !aligned(out, 8))
    return fail(GCG_ERR_MISALIGNED, "gcg_haversine_km_f64: operand not 8-B aligned");
  hipLaunchKernelGGL(haversine_kernel, dim3(grid_for(M)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), M, a, b, 2 * earth_radius_km, out);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_nearest_class_f64(int64_t M, const double* locs, int64_t C, const double* medians,
                                 double earth_radius_km, int32_t* index, double* distance,
                                 gcg_stream_t stream) {
  if (M < 0 || C < 0 || C > INT32_MAX || M > (int64_t{1} << 38) || !radius_ok(earth_radius_km))
    return fail(GCG_ERR_INVALID_ARG, "gcg_nearest_class_f64: bad sizes or radius");
  if (M == 0) return GCG_OK;
  if (C == 0) return fail(GCG_ERR_INVALID_ARG, "gcg_nearest_class_f64: no class to choose from");
  if (locs == nullptr || medians == nullptr || index == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_nearest_class_f64: null operand");
  if (!aligned(locs, 8) || !aligned(medians, 8) || !aligned(index, 4) || !aligned(distance, 8))
    return fail(GCG_ERR_MISALIGNED, "gcg_nearest_class_f64: operand not aligned to its element");
  const dim3 grid(static_cast<unsigned>((M + 255) / 256));
  hipLaunchKernelGGL(nearest_class_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                     M, C, locs, medians, 2 * earth_radius_km, index, distance);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_geo_eval_f64(int64_t M, const void* pred, int pred_is_int64, const double* locs,
                            int64_t C, const double* medians, double earth_radius_km,
                            double threshold_km, double* distance, int64_t* count_dev,
                            int32_t* status_dev, gcg_stream_t stream) {
  if (M < 0 || C < 0 || M > (int64_t{1} << 38) || !radius_ok(earth_radius_km) ||
      (pred_is_int64 != 0 && pred_is_int64 != 1) || std::isnan(threshold_km))
    return fail(GCG_ERR_INVALID_ARG, "gcg_geo_eval_f64: bad sizes, radius or threshold");
  if (count_dev == nullptr || status_dev == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_geo_eval_f64: null count_dev / status_dev");
  if (!aligned(count_dev, 8) || !aligned(status_dev, 4))
    return fail(GCG_ERR_MISALIGNED, "gcg_geo_eval_f64: count_dev / status_dev misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st));
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (M == 0) return GCG_OK;
  if (pred == nullptr || locs == nullptr || distance == nullptr || (C > 0 && medians == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "gcg_geo_eval_f64: null operand");
  if (!aligned(pred, pred_is_int64 ? 8 : 4) || !aligned(locs, 8) || !aligned(medians, 8) ||
      !aligned(distance, 8))
    return fail(GCG_ERR_MISALIGNED, "gcg_geo_eval_f64: operand not aligned to its element");
  const dim3 grid(static_cast<unsigned>((M + 255) / 256));
  auto* count = reinterpret_cast<unsigned long long*>(count_dev);
  if (pred_is_int64)
    hipLaunchKernelGGL(geo_eval_kernel<int64_t>, grid, dim3(256), 0, st, M, C,
                       static_cast<const int64_t*>(pred), locs, medians, 2 * earth_radius_km,
                       threshold_km, distance, count, status_dev);
  else
    hipLaunchKernelGGL(geo_eval_kernel<int32_t>, grid, dim3(256), 0, st, M, C,
                       static_cast<const int32_t*>(pred), locs, medians, 2 * earth_radius_km,
                       threshold_km, distance, count, status_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
