// kmeans.hip -- the k-means initialisation of the Gaussian components (include/gcg_spmm.h):
// get_cluster_centers of lang2loc.py:473-478, lang2loc_mdnshared.py:127-185 and
// loc2lang.py:326-371 as full Lloyd k-means on resident float64 coordinates: the assignment,
// the centre update, the k-means++ seeding and the per-cluster statistics.
//
// Every squared distance is d = (x0 - c0) * (x0 - c0) + (x1 - c1) * (x1 - c1) with each
// operation rounded once (the library is built with -ffp-contract=off) and strict < keeps the
// lowest index on a tie. No sum depends on the launch grid or on timing: members are summed by
// fixed strides and fixed trees, never with floating-point atomics.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cmath>

#include "scratch.h"
#include "segment_kernels.h"

using namespace gcg;

namespace {

// centres staged per LDS tile of kmeans_assign_kernel: one 16-B (c0, c1) pair each, 16 KiB
constexpr int kCentreTile = 1024;
// points per thread of kmeans_assign_kernel: one broadcast LDS read serves this many distances
constexpr int kAssignPts = 4;
constexpr int kAssignBlockPts = 256 * kAssignPts;
// consecutive points per thread / per workgroup of the seeding kernels
constexpr int kPpPts = 8;
constexpr int kPpBlockPts = 256 * kPpPts;
constexpr int64_t kMaxPoints = (int64_t{1} << 30) - 2;  // geo.hip's limit

// The sum of v over the 256 threads of a workgroup in a fixed tree: s[t] += s[t + h] for
// h = 128, 64, ..., 1. Every thread returns the total.
__device__ __forceinline__ double block_sum(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();  // s may still be read from the call before
  s[t] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) s[t] += s[t + h];
    __syncthreads();
  }
  return s[0];
}

__device__ __forceinline__ double sq_dist(double x0, double x1, double c0, double c1) {
  const double a = x0 - c0, b = x1 - c1;
  return a * a + b * b;
}

// Thread t of workgroup g owns points g * 1024 + t + 256 p, p = 0..3. The centres pass through
// LDS in tiles; every lane reads the same 16-B pair (a broadcast) and keeps a running
// (distance, index) minimum per point. partials[g] = the workgroup's sum of the minima: each
// thread adds its points in ascending p, then block_sum.
__global__ __launch_bounds__(256) void kmeans_assign_kernel(
    int64_t N, int64_t C, const double* __restrict__ locs, const double* __restrict__ centers,
    const int32_t* __restrict__ prev, int32_t* __restrict__ labels, double* __restrict__ dist2,
    double* __restrict__ partials, int32_t* __restrict__ changed, int32_t* __restrict__ status) {
  __shared__ double2 s_c[kCentreTile];
  __shared__ double s_red[256];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kAssignBlockPts + threadIdx.x;
  double x0[kAssignPts], x1[kAssignPts], best[kAssignPts];
  int32_t best_c[kAssignPts];
#pragma unroll
  for (int p = 0; p < kAssignPts; ++p) {
    const int64_t i = base + p * 256;
    x0[p] = x1[p] = 0.0;
    if (i < N) {
      x0[p] = locs[2 * i];
      x1[p] = locs[2 * i + 1];
      if (!isfinite(x0[p]) || !isfinite(x1[p])) *status = 1;
    }
    best[p] = INFINITY;
    best_c[p] = 0;
  }
  for (int64_t t0 = 0; t0 < C; t0 += kCentreTile) {
    const int tn = static_cast<int>(min(static_cast<int64_t>(kCentreTile), C - t0));
    __syncthreads();
    for (int j = threadIdx.x; j < tn; j += 256)
      s_c[j] = make_double2(centers[2 * (t0 + j)], centers[2 * (t0 + j) + 1]);
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < tn; ++j) {
      const double2 c = s_c[j];
#pragma unroll
      for (int p = 0; p < kAssignPts; ++p) {
        const double d = sq_dist(x0[p], x1[p], c.x, c.y);
        if (d < best[p]) {
          best[p] = d;
          best_c[p] = static_cast<int32_t>(t0 + j);
        }
      }
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int p = 0; p < kAssignPts; ++p) {
    const int64_t i = base + p * 256;
    if (i < N) {
      labels[i] = best_c[p];
      if (dist2 != nullptr) dist2[i] = best[p];
      if (changed != nullptr && prev != nullptr && prev[i] != best_c[p]) *changed = 1;
      sum += best[p];
    }
  }
  if (partials != nullptr) {
    const double total = block_sum(sum, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
  }
}

// *out = the sum of partials[0..n): thread t adds partials[t], partials[t + 256], ... in
// ascending order, then block_sum. One workgroup.
__global__ __launch_bounds__(256) void sum_partials_kernel(int64_t n,
                                                           const double* __restrict__ partials,
                                                           double* __restrict__ out) {
  __shared__ double s_red[256];
  double sum = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += 256) sum += partials[b];
  const double total = block_sum(sum, s_red);
  if (threadIdx.x == 0) *out = total;
}

// keys[i] = labels[i], ids[i] = i (a label outside [0, C) raises *status and sorts as 0).
__global__ void label_keys_kernel(int64_t N, int64_t C, const int32_t* __restrict__ labels,
                                  int32_t* __restrict__ keys, int32_t* __restrict__ ids,
                                  int32_t* __restrict__ status) {
  for (int64_t i = grid_start(); i < N; i += grid_stride()) {
    int32_t l = labels[i];
    if (l < 0 || l >= C) {
      *status = 1;
      l = 0;
    }
    keys[i] = l;
    ids[i] = static_cast<int32_t>(i);
  }
}

// One workgroup per cluster segment [ptr[c], ptr[c+1]) of ids (ascending point index inside a
// segment): thread t adds members t, t + 256, ... of the segment in that order, then block_sum.
// The launch grid only decides which workgroup takes which cluster.
__global__ __launch_bounds__(256) void kmeans_update_kernel(
    int64_t C, const double* __restrict__ locs, const int32_t* __restrict__ ptr,
    const int32_t* __restrict__ ids, const double* prev, double* centers,
    int32_t* __restrict__ counts) {
  __shared__ double s_red[256];
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const int64_t b = ptr[c], e = ptr[c + 1];
    double a0 = 0.0, a1 = 0.0;
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
      const int64_t i = ids[p];
      a0 += locs[2 * i];
      a1 += locs[2 * i + 1];
    }
    const double t0 = block_sum(a0, s_red), t1 = block_sum(a1, s_red);
    if (threadIdx.x == 0) {
      const int64_t n = e - b;
      counts[c] = static_cast<int32_t>(n);
      const double k0 = n > 0 ? t0 / static_cast<double>(n) : prev[2 * c];
      const double k1 = n > 0 ? t1 / static_cast<double>(n) : prev[2 * c + 1];
      centers[2 * c] = k0;
      centers[2 * c + 1] = k1;
    }
  }
}

// The inverse softplus and the inverse softsign of mdn.cluster_params.
__device__ __forceinline__ double raw_sigma(double s) { return s + log1p(-exp(-s)); }
__device__ __forceinline__ double raw_corxy(double c) { return c / (1.0 - fabs(c)); }

// One workgroup per cluster segment, two passes over its members with update's summation
// order: the deviations from the segment's first member f give the mean f + sum / n, then the
// deviations from that mean give the (co)variances.
__global__ __launch_bounds__(256) void cluster_stats_kernel(
    int64_t C, const double* __restrict__ locs, const int32_t* __restrict__ ptr,
    const int32_t* __restrict__ ids, int raw, double* __restrict__ means,
    double* __restrict__ sigmas, double* __restrict__ corxys, int32_t* __restrict__ counts) {
  __shared__ double s_red[256];
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const int64_t b = ptr[c], e = ptr[c + 1], n = e - b;
    double std0 = 1.0, std1 = 1.0, cor = 0.0;
    if (n > 0) {  // uniform over the workgroup
      const int64_t f = ids[b];
      const double f0 = locs[2 * f], f1 = locs[2 * f + 1];
      double a0 = 0.0, a1 = 0.0;
      for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int64_t i = ids[p];
        a0 += locs[2 * i] - f0;
        a1 += locs[2 * i + 1] - f1;
      }
      const double m0 = block_sum(a0, s_red) / static_cast<double>(n);
      const double m1 = block_sum(a1, s_red) / static_cast<double>(n);
      double q00 = 0.0, q11 = 0.0, q01 = 0.0;
      for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int64_t i = ids[p];
        const double d0 = (locs[2 * i] - f0) - m0, d1 = (locs[2 * i + 1] - f1) - m1;
        q00 += d0 * d0;
        q11 += d1 * d1;
        q01 += d0 * d1;
      }
      const double v00 = block_sum(q00, s_red), v11 = block_sum(q11, s_red);
      const double v01 = block_sum(q01, s_red);
      if (threadIdx.x == 0) {
        means[2 * c] = f0 + m0;
        means[2 * c + 1] = f1 + m1;
      }
      if (n > 1) {
        const double dof = static_cast<double>(n - 1);
        const double s0 = sqrt(v00 / dof), s1 = sqrt(v11 / dof);
        const double r = (v01 / dof) / (s0 * s1);
        if (s0 > 0.0 && s1 > 0.0 && !isnan(r)) {  // false for a zero variance and for a NaN
          std0 = s0;
          std1 = s1;
          cor = r;
        }
      }
    }
    if (threadIdx.x == 0) {
      sigmas[2 * c] = raw ? raw_sigma(std0) : std0;
      sigmas[2 * c + 1] = raw ? raw_sigma(std1) : std1;
      corxys[c] = raw ? raw_corxy(cor) : cor;
      if (counts != nullptr) counts[c] = static_cast<int32_t>(n);
    }
  }
}

// Round 0 of the seeding: the input checks and centre 0 = point floor(u[0] * N).
__global__ void pp_first_kernel(int64_t N, int64_t C, const double* __restrict__ locs,
                                const double* __restrict__ u, int32_t* __restrict__ chosen,
                                int32_t* __restrict__ status) {
  for (int64_t i = grid_start(); i < N; i += grid_stride()) {
    if (!isfinite(locs[2 * i]) || !isfinite(locs[2 * i + 1])) atomicMax(status, 2);
    if (i < C && !(u[i] >= 0.0 && u[i] < 1.0)) atomicMax(status, 3);
    if (i == 0) {
      const double t = u[0] * static_cast<double>(N);
      int64_t j = 0;
      if (t >= static_cast<double>(N)) j = N - 1;
      else if (t > 0.0) j = static_cast<int64_t>(t);
      chosen[0] = static_cast<int32_t>(j);
    }
  }
}

// d2[i] = min(d2[i], |x_i - x_c|^2) for the centre c = chosen[k - 1] just picked (`first`:
// no earlier value). Thread t of workgroup g owns the 8 consecutive points from
// g * 2048 + 8 t; bsum[g] = the workgroup's sum of d2: ascending inside a thread, then
// block_sum.
__global__ __launch_bounds__(256) void pp_distance_kernel(int64_t N, const double* __restrict__ locs,
                                                          const int32_t* __restrict__ chosen,
                                                          int64_t k, int first,
                                                          double* __restrict__ d2,
                                                          double* __restrict__ bsum) {
  __shared__ double s_red[256];
  const int64_t c = chosen[k - 1];
  const double c0 = locs[2 * c], c1 = locs[2 * c + 1];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kPpBlockPts + threadIdx.x * kPpPts;
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < kPpPts; ++q) {
    const int64_t i = base + q;
    if (i < N) {
      double d = sq_dist(locs[2 * i], locs[2 * i + 1], c0, c1);
      if (!first) {
        const double old = d2[i];
        if (old < d) d = old;
      }
      d2[i] = d;
      acc += d;
    }
  }
  const double total = block_sum(acc, s_red);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// Centre k = the first i with S_i > u[k] * S_{N-1}, clamped to the last i with d2[i] > 0,
// where S is the inclusive prefix sum of d2 in index order, taken in three levels, each added
// in ascending order: 256 chunks of ceil(nb / 256) workgroup sums, the workgroup sums inside
// the chunk that crosses the target, and inside that workgroup's 2048 points the thread sums
// before a thread and then the thread's own points up to i. Where no prefix exceeds the target
// (u[k] * S rounds to S, or two levels round apart) the pick is the last point with d2 > 0 at
// that level. One workgroup.
__global__ __launch_bounds__(256) void pp_select_kernel(int64_t N, int64_t nb,
                                                        const double* __restrict__ d2,
                                                        const double* __restrict__ bsum,
                                                        const double* __restrict__ u, int64_t k,
                                                        int32_t* __restrict__ chosen,
                                                        int32_t* __restrict__ status) {
  __shared__ double s_pre[256];
  __shared__ double s_target;
  __shared__ int64_t s_blk;
  __shared__ int s_found, s_first, s_last;
  const int t = threadIdx.x;
  const int64_t per = (nb + 255) / 256;
  {
    const int64_t b0 = min(t * per, nb), b1 = min(b0 + per, nb);
    double mine = 0.0;
    for (int64_t b = b0; b < b1; ++b) mine += bsum[b];
    s_pre[t] = mine;
  }
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int j = 0; j < 256; ++j) total += s_pre[j];
    const double target = u[k] * total;
    int chunk = -1, last_nz = -1;
    double run = 0.0, pre = 0.0, pre_nz = 0.0;
    for (int j = 0; j < 256; ++j) {
      const double v = s_pre[j], nxt = run + v;
      if (v > 0.0) {
        last_nz = j;
        pre_nz = run;
        if (chunk < 0 && nxt > target) {
          chunk = j;
          pre = run;
        }
      }
      run = nxt;
    }
    int found = chunk >= 0;
    if (!found) {
      chunk = last_nz;
      pre = pre_nz;
    }
    if (!(total > 0.0) || !(target >= 0.0)) chunk = -1;  // no distinct point left, or a NaN
    int64_t blk = -1;
    if (chunk >= 0) {
      // the chunk's workgroups in ascending order: the first whose inclusive prefix exceeds
      // the target, or the chunk's last one with a positive sum
      const int64_t c0 = chunk * per, c1 = min(c0 + per, nb);
      int64_t last_b = -1;
      double r = pre, pre_b = pre;
      for (int64_t b = c0; b < c1 && blk < 0; ++b) {
        const double v = bsum[b], nxt = r + v;
        if (v > 0.0) {
          last_b = b;
          pre_b = r;
          if (found && nxt > target) blk = b;
        }
        r = nxt;
      }
      if (blk < 0) blk = last_b;
      pre = pre_b;
    }
    s_found = found;
    s_blk = blk;
    s_target = target;
    s_pre[0] = pre;
    s_first = INT_MAX;
    s_last = -1;
  }
  __syncthreads();
  const int64_t blk = s_blk;
  if (blk < 0) {
    if (t == 0) {
      chosen[k] = 0;
      atomicMax(status, 1);
    }
    return;
  }
  const double target = s_target, pre = s_pre[0];
  const int found = s_found;
  const int64_t base = blk * kPpBlockPts + static_cast<int64_t>(t) * kPpPts;
  double v[kPpPts], mine = 0.0;
#pragma unroll
  for (int q = 0; q < kPpPts; ++q) {
    v[q] = base + q < N ? d2[base + q] : 0.0;
    mine += v[q];
  }
  __syncthreads();  // every thread has read s_pre[0]
  s_pre[t] = mine;
  __syncthreads();
  if (t == 0) {
    double run = pre;
    for (int j = 0; j < 256; ++j) {
      const double m = s_pre[j];
      s_pre[j] = run;
      run += m;
    }
  }
  __syncthreads();
  double run = s_pre[t];
  int first = INT_MAX, last = -1;
#pragma unroll
  for (int q = 0; q < kPpPts; ++q) {
    run += v[q];
    if (v[q] > 0.0) {
      last = static_cast<int>(base + q);
      if (found && first == INT_MAX && run > target) first = last;
    }
  }
  if (first != INT_MAX) atomicMin(&s_first, first);
  if (last >= 0) atomicMax(&s_last, last);
  __syncthreads();
  if (t == 0) {
    int pick = s_first != INT_MAX ? s_first : s_last;
    if (pick < 0) {
      pick = 0;
      atomicMax(status, 1);
    }
    chosen[k] = pick;
  }
}

// The scratch of the label sort.
struct SortSpace {
  int32_t *keys, *keys_sorted, *iota, *ids, *ptr;
  Tmp tmp;
  size_t total;
};

gcg_status sort_space(const char* fn, int64_t N, int64_t C, void* workspace, SortSpace* s) {
  Carver cv(workspace);
  s->keys = cv.take<int32_t>(N);
  s->keys_sorted = cv.take<int32_t>(N);
  s->iota = cv.take<int32_t>(N);
  s->ids = cv.take<int32_t>(N);
  s->ptr = cv.take<int32_t>(C + 1);
  TmpSize ts;
  if (N > 0)
    ts.add(GCG_CUB(DeviceRadixSort::SortPairs, s->keys, s->keys_sorted, s->iota, s->ids, static_cast<int>(N),
        0, bits_to_count(C)));
  return ts.take(fn, cv, &s->tmp, &s->total);
}

// ids = the point indices grouped by label, ascending inside a label (a stable sort of
// (label, index)); ptr[c] = the head of cluster c's segment.
gcg_status sort_by_label(int64_t N, int64_t C, const int32_t* labels, const SortSpace& s,
                         int32_t* status_dev, hipStream_t st) {
  if (N > 0) {
    hipLaunchKernelGGL(label_keys_kernel, dim3(grid_for(N)), dim3(256), 0, st, N, C, labels,
                       s.keys, s.iota, status_dev);
    GCG_HIP_CHECK(hipGetLastError());
    GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, s.keys, s.keys_sorted, s.iota, s.ids,
        static_cast<int>(N), 0, bits_to_count(C), st)));
  }
  hipLaunchKernelGGL(class_ptr_kernel, dim3(grid_for(N + 1)), dim3(256), 0, st, N, C,
                     s.keys_sorted, s.ptr);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

bool sizes_ok(int64_t N, int64_t C) {
  return N >= 0 && N <= kMaxPoints && C >= 0 && C <= INT32_MAX - 1;
}

int64_t assign_blocks(int64_t N) { return (N + kAssignBlockPts - 1) / kAssignBlockPts; }
int64_t pp_blocks(int64_t N) { return (N + kPpBlockPts - 1) / kPpBlockPts; }
int segment_grid(int64_t C) { return static_cast<int>(std::min<int64_t>(C, 65536)); }

}  // namespace

extern "C" {

int32_t gcg_kmeans_centre_tile(void) { return kCentreTile; }

gcg_status gcg_kmeans_assign_f64_workspace_bytes(int64_t N, size_t* bytes) {
  if (bytes == nullptr || N < 0 || N > kMaxPoints)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_assign_f64_workspace_bytes: bad N or null bytes");
  Carver cv(nullptr);
  cv.take<double>(assign_blocks(N));
  *bytes = cv.used;
  return GCG_OK;
}

gcg_status gcg_kmeans_assign_f64(int64_t N, const double* locs, int64_t C, const double* centers,
                                 const int32_t* prev_labels, int32_t* labels, double* dist2,
                                 double* inertia_dev, int32_t* changed_dev, int32_t* status_dev,
                                 void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  if (!sizes_ok(N, C))
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_assign_f64: bad sizes N=%lld C=%lld",
                static_cast<long long>(N), static_cast<long long>(C));
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_assign_f64: null status_dev");
  if (!aligned(status_dev, 4) || !aligned(changed_dev, 4) || !aligned(inertia_dev, 8))
    return fail(GCG_ERR_MISALIGNED, "gcg_kmeans_assign_f64: status / changed / inertia misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (changed_dev) GCG_HIP_CHECK(hipMemsetAsync(changed_dev, 0, sizeof(int32_t), st));
  if (N == 0) {
    if (inertia_dev) GCG_HIP_CHECK(hipMemsetAsync(inertia_dev, 0, sizeof(double), st));
    return GCG_OK;
  }
  if (C == 0) return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_assign_f64: no centre to choose from");
  if (locs == nullptr || centers == nullptr || labels == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_assign_f64: null operand");
  if (!aligned(locs, 8) || !aligned(centers, 8) || !aligned(labels, 4) ||
      !aligned(prev_labels, 4) || !aligned(dist2, 8) || !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "gcg_kmeans_assign_f64: operand not aligned to its element");
  const int64_t nb = assign_blocks(N);
  double* partials = nullptr;
  if (inertia_dev != nullptr) {
    size_t need = 0;
    (void)gcg_kmeans_assign_f64_workspace_bytes(N, &need);
    if (gcg_status s = check_workspace("gcg_kmeans_assign_f64", workspace, workspace_bytes, need, 8))
      return s;
    partials = static_cast<double*>(workspace);
  }
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, N, C,
                     locs, centers, prev_labels, labels, dist2, partials, changed_dev, status_dev);
  GCG_HIP_CHECK(hipGetLastError());
  if (inertia_dev != nullptr) {
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, nb, partials, inertia_dev);
    GCG_HIP_CHECK(hipGetLastError());
  }
  return GCG_OK;
}

gcg_status gcg_kmeans_update_f64_workspace_bytes(int64_t N, int64_t C, size_t* bytes) {
  if (bytes == nullptr || !sizes_ok(N, C))
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_update_f64_workspace_bytes: bad sizes or null bytes");
  SortSpace s;
  gcg_status rc = sort_space("gcg_kmeans_update_f64_workspace_bytes", N, C, nullptr, &s);
  if (rc != GCG_OK) return rc;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_kmeans_update_f64(int64_t N, const double* locs, const int32_t* labels, int64_t C,
                                 const double* prev_centers, double* centers, int32_t* counts,
                                 int32_t* status_dev, void* workspace, size_t workspace_bytes,
                                 gcg_stream_t stream) {
  if (!sizes_ok(N, C)) return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_update_f64: bad sizes");
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_update_f64: null status_dev");
  if (!aligned(status_dev, 4)) return fail(GCG_ERR_MISALIGNED, "gcg_kmeans_update_f64: status_dev misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (C == 0) {
    if (N > 0) return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_update_f64: points but no cluster");
    return GCG_OK;
  }
  if (prev_centers == nullptr || centers == nullptr || counts == nullptr ||
      (N > 0 && (locs == nullptr || labels == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_update_f64: null operand");
  if (!aligned(locs, 8) || !aligned(prev_centers, 8) || !aligned(centers, 8) ||
      !aligned(labels, 4) || !aligned(counts, 4) || !aligned(workspace, 256))
    return fail(GCG_ERR_MISALIGNED, "gcg_kmeans_update_f64: operand not aligned (workspace: 256 B)");
  SortSpace s;
  gcg_status rc = sort_space("gcg_kmeans_update_f64", N, C, workspace, &s);
  if (rc != GCG_OK) return rc;
  if ((rc = check_workspace("gcg_kmeans_update_f64", workspace, workspace_bytes, s.total, 256))) return rc;
  rc = sort_by_label(N, C, labels, s, status_dev, st);
  if (rc != GCG_OK) return rc;
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(segment_grid(C)), dim3(256), 0, st, C, locs, s.ptr,
                     s.ids, prev_centers, centers, counts);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_kmeans_pp_f64_workspace_bytes(int64_t N, size_t* bytes) {
  if (bytes == nullptr || N < 0 || N > kMaxPoints)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_pp_f64_workspace_bytes: bad N or null bytes");
  Carver cv(nullptr);
  cv.take<double>(N);
  cv.take<double>(pp_blocks(N));
  *bytes = cv.used;
  return GCG_OK;
}

gcg_status gcg_kmeans_pp_f64(int64_t N, const double* locs, int64_t C, const double* u_dev,
                             int32_t* indices, int32_t* status_dev, void* workspace,
                             size_t workspace_bytes, gcg_stream_t stream) {
  if (N < 0 || N > kMaxPoints || C < 1 || C > N)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_pp_f64: need 1 <= C <= N, got N=%lld C=%lld",
                static_cast<long long>(N), static_cast<long long>(C));
  if (locs == nullptr || u_dev == nullptr || indices == nullptr || status_dev == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "gcg_kmeans_pp_f64: null operand");
  if (!aligned(locs, 8) || !aligned(u_dev, 8) || !aligned(indices, 4) || !aligned(status_dev, 4) ||
      !aligned(workspace, 256))
    return fail(GCG_ERR_MISALIGNED, "gcg_kmeans_pp_f64: operand not aligned (workspace: 256 B)");
  size_t need = 0;
  (void)gcg_kmeans_pp_f64_workspace_bytes(N, &need);
  if (gcg_status s = check_workspace("gcg_kmeans_pp_f64", workspace, workspace_bytes, need, 256))
    return s;
  Carver cv(workspace);
  double* d2 = cv.take<double>(N);
  const int64_t nb = pp_blocks(N);
  double* bsum = cv.take<double>(nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(pp_first_kernel, dim3(grid_for(N)), dim3(256), 0, st, N, C, locs, u_dev,
                     indices, status_dev);
  GCG_HIP_CHECK(hipGetLastError());
  // the rounds are sequential on the stream; the picked index never leaves the device
  for (int64_t k = 1; k < C; ++k) {
    hipLaunchKernelGGL(pp_distance_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, N,
                       locs, indices, k, k == 1 ? 1 : 0, d2, bsum);
    hipLaunchKernelGGL(pp_select_kernel, dim3(1), dim3(256), 0, st, N, nb, d2, bsum, u_dev, k,
                       indices, status_dev);
  }
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_cluster_stats_f64_workspace_bytes(int64_t N, int64_t C, size_t* bytes) {
  return gcg_kmeans_update_f64_workspace_bytes(N, C, bytes);
}

gcg_status gcg_cluster_stats_f64(int64_t N, const double* locs, const int32_t* labels, int64_t C,
                                 int raw, double* means, double* sigmas, double* corxys,
                                 int32_t* counts, int32_t* status_dev, void* workspace,
                                 size_t workspace_bytes, gcg_stream_t stream) {
  if (!sizes_ok(N, C) || (raw != 0 && raw != 1))
    return fail(GCG_ERR_INVALID_ARG, "gcg_cluster_stats_f64: bad sizes or raw");
  if (status_dev == nullptr) return fail(GCG_ERR_INVALID_ARG, "gcg_cluster_stats_f64: null status_dev");
  if (!aligned(status_dev, 4)) return fail(GCG_ERR_MISALIGNED, "gcg_cluster_stats_f64: status_dev misaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  if (C == 0) {
    if (N > 0) return fail(GCG_ERR_INVALID_ARG, "gcg_cluster_stats_f64: points but no cluster");
    return GCG_OK;
  }
  if (means == nullptr || sigmas == nullptr || corxys == nullptr ||
      (N > 0 && (locs == nullptr || labels == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "gcg_cluster_stats_f64: null operand");
  if (!aligned(locs, 8) || !aligned(means, 8) || !aligned(sigmas, 8) || !aligned(corxys, 8) ||
      !aligned(labels, 4) || !aligned(counts, 4) || !aligned(workspace, 256))
    return fail(GCG_ERR_MISALIGNED, "gcg_cluster_stats_f64: operand not aligned (workspace: 256 B)");
  SortSpace s;
  gcg_status rc = sort_space("gcg_cluster_stats_f64", N, C, workspace, &s);
  if (rc != GCG_OK) return rc;
  if ((rc = check_workspace("gcg_cluster_stats_f64", workspace, workspace_bytes, s.total, 256))) return rc;
  rc = sort_by_label(N, C, labels, s, status_dev, st);
  if (rc != GCG_OK) return rc;
  hipLaunchKernelGGL(cluster_stats_kernel, dim3(segment_grid(C)), dim3(256), 0, st, C, locs, s.ptr,
                     s.ids, raw, means, sigmas, corxys, counts);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
