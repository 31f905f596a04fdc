// grid.hip -- the grid representation of loc2lang's no-MDN baseline (reference loc2lang.py:298-322,
// grid_representation): every coordinate becomes a sparse row over a regular lat/lon grid, an
// entry 1/haversine_km for every grid point nearer than the radius, the row l1-normalised.
// All float64; the stored value is rounded to float32 once.
//
// A count pass (entries per row, and the row's norm), an exclusive scan, a fill pass. One wave
// owns one coordinate. The grid's coordinate tables come from the host (numpy's arange doubles)
// and go through LDS once per workgroup: latitudes as radians and cos(lat), longitudes as radians.
// A wave does not look at all P = n_lat * n_lon columns but at a window that contains every
// column in range (include/gcg_spmm.h has the proof); `exhaustive` makes the window the whole
// grid on the same code path. Both passes enumerate the window through scan_row and evaluate
// candidates through haversine_rad on the same inputs, so they take the same decisions bit for
// bit. The window's candidates are packed 64 at a time in ascending column order; a ballot and
// a prefix popcount give each kept candidate its slot in the row. The row's sum adds the k-th
// kept weight into lane k % 64 and folds the lanes by the fixed butterfly: its order depends on
// the kept entries alone, not on the window, the launch or a chunking of the rows.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "haversine.h"
#include "scratch.h"

using namespace gcg;

namespace {

// doubles of LDS the three tables may take (2 n_lat + n_lon): 48 KiB
constexpr int64_t kMaxTable = 6144;
// beyond this many radians a longitude is not reduced: the row takes every longitude
constexpr double kMaxLon = 64.0 * kPi;

struct GridArgs {
  int n_lat, n_lon;
  double radius, two_r;
  double dlat;      // radius / R with its margin: no row further than this in latitude is in range
  double sin_half;  // sin(radius / 2R)
  int exhaustive;
};

// first index in [0, n) with t[i] >= x (n if none); t ascending, in LDS, x wave-uniform
__device__ __forceinline__ int lower_bound(const double* t, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// first index with t[i] > x
__device__ __forceinline__ int upper_bound(const double* t, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// position of the j-th set bit of mask (j < popcount(mask))
__device__ __forceinline__ int nth_set_bit(unsigned long long mask, int j) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = __popcll(mask & (((1ull << w) - 1ull) << pos));
    if (j >= c) {
      j -= c;
      pos += w;
    }
  }
  return pos;
}

// The window of one coordinate as a sequence of column ranges [lo, hi) of latitude rows, in
// ascending column order. Every value here is wave-uniform.
struct Window {
  const GridArgs& g;
  const double *s_lat, *s_cos, *s_lon;
  double lat1, cos1, lon1;
  bool all_lon;  // this coordinate's longitude is not reduced: every row takes all longitudes
  int j, j_end;  // latitude rows left
  // the current row's intervals lon1 + 2 pi k +- h, k ascending
  bool open;
  double h, k, k_end;
  int prev_end;

  __device__ Window(const GridArgs& g_, const double* la, const double* co, const double* lo,
                    double lat1_, double cos1_, double lon1_)
      : g(g_), s_lat(la), s_cos(co), s_lon(lo), lat1(lat1_), cos1(cos1_), lon1(lon1_) {
    all_lon = g.exhaustive || !(fabs(lon1) <= kMaxLon);
    if (g.exhaustive) {
      j = 0;
      j_end = g.n_lat;
    } else {
      j = max(lower_bound(s_lat, g.n_lat, lat1 - g.dlat) - 1, 0);
      j_end = min(upper_bound(s_lat, g.n_lat, lat1 + g.dlat) + 1, g.n_lat);
    }
    open = false;
  }

  // the next non-empty range: true and (row, lo, hi), or false when the window is done
  __device__ bool next(int& row, int& lo, int& hi) {
    for (;;) {
      if (j >= j_end) return false;
      if (!open) {
        const double c = cos1 * s_cos[j];
        // sin(dlon / 2) <= sin_half / sqrt(c); a bound of 1 or more (or no bound) is every longitude
        const double q = (c > 0.0) ? g.sin_half / sqrt(c) : 2.0;
        if (all_lon || !(q < 1.0)) {
          row = j++;
          lo = 0;
          hi = g.n_lon;
          return true;
        }
        h = 2.0 * asin(q) * (1.0 + 1e-9) + 1e-12;
        const double first = s_lon[0], last = s_lon[g.n_lon - 1];
        k = ceil((first - h - lon1) / (2.0 * kPi)) - 1.0;
        k_end = floor((last + h - lon1) / (2.0 * kPi)) + 1.0;
        prev_end = 0;
        open = true;
      }
      while (k <= k_end) {
        const double centre = lon1 + 2.0 * kPi * k;
        k += 1.0;
        int a = lower_bound(s_lon, g.n_lon, centre - h) - 1;
        int b = upper_bound(s_lon, g.n_lon, centre + h) + 1;
        a = max(a, prev_end);
        b = min(b, g.n_lon);
        if (a < b) {
          prev_end = b;
          row = j;
          lo = a;
          hi = b;
          return true;
        }
      }
      open = false;
      ++j;
    }
  }
};

// One coordinate's window, 64 candidates at a time: emit(keep, slot, column, d) for every lane
// of every chunk, slot = the kept candidate's position in the row. Returns the row's entries.
template <typename Emit>
__device__ __forceinline__ int scan_row(const GridArgs& g, const double* s_lat, const double* s_cos,
                                        const double* s_lon, double lat1, double lon1, int lane,
                                        Emit&& emit) {
  const double cos1 = cos(lat1);
  Window win(g, s_lat, s_cos, s_lon, lat1, cos1, lon1);
  int row = 0, lo = 0, hi = 0;
  bool have = win.next(row, lo, hi);
  int base = 0;
  while (have) {
    // pack up to 64 candidates from consecutive ranges
    int filled = 0, my_row = -1, my_col = 0;
    while (have && filled < kWave) {
      const int take = min(kWave - filled, hi - lo);
      if (lane >= filled && lane < filled + take) {
        my_row = row;
        my_col = lo + (lane - filled);
      }
      filled += take;
      lo += take;
      if (lo >= hi) have = win.next(row, lo, hi);
    }
    const bool valid = my_row >= 0;
    double d = INFINITY;
    if (valid)
      d = haversine_rad(lat1, cos1, lon1, s_lat[my_row], s_cos[my_row], s_lon[my_col], g.two_r);
    const bool keep = valid && d < g.radius;
    const unsigned long long mask = __ballot(keep);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    emit(keep, mask, base, pre, valid ? my_row * g.n_lon + my_col : 0, d);
    base += __popcll(mask);
  }
  return base;
}

// dynamic LDS: lat radians [n_lat], cos(lat) [n_lat], lon radians [n_lon]
__device__ __forceinline__ void stage_tables(const GridArgs& g, const double* __restrict__ lats,
                                             const double* __restrict__ lons, double* s) {
  for (int i = threadIdx.x; i < g.n_lat; i += kBlock) {
    const double la = lats[i] * kDegToRad;
    s[i] = la;
    s[g.n_lat + i] = cos(la);
  }
  for (int i = threadIdx.x; i < g.n_lon; i += kBlock) s[2 * g.n_lat + i] = lons[i] * kDegToRad;
  __syncthreads();
}

__device__ __forceinline__ bool coord_ok(double lat, double lon) {
  return isfinite(lat) && isfinite(lon) && fabs(lat) <= 90.0;
}

// counts[i] = entries of row i (counts[n] = 0); norm[i] = the row's sum of 1/d in float64, or -Z
// when Z >= 1 columns lie at distance zero. A bad coordinate raises info[1] and counts nothing.
__global__ __launch_bounds__(kBlock) void grid_count_kernel(
    int64_t n, const double* __restrict__ coords, const double* __restrict__ lats,
    const double* __restrict__ lons, GridArgs g, int64_t* __restrict__ counts,
    double* __restrict__ norm, int64_t* __restrict__ info) {
  extern __shared__ double s_tab[];
  stage_tables(g, lats, lons, s_tab);
  const double *s_lat = s_tab, *s_cos = s_tab + g.n_lat, *s_lon = s_tab + 2 * g.n_lat;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[n] = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); i < n;
       i += wstride) {
    const double lat = coords[2 * i], lon = coords[2 * i + 1];
    if (!coord_ok(lat, lon)) {
      if (lane == 0) {
        info[1] = 1;
        counts[i] = 0;
        norm[i] = 0.0;
      }
      continue;
    }
    double acc = 0.0;
    int zeros = 0;
    const int cnt = scan_row(
        g, s_lat, s_cos, s_lon, lat * kDegToRad, lon * kDegToRad, lane,
        [&](bool keep, unsigned long long mask, int base, int pre, int, double d) {
          const bool zero = keep && d == 0.0;
          zeros += __popcll(__ballot(zero));
          const double w = (keep && !zero) ? 1.0 / d : 0.0;
          // the kept candidate of slot s adds into lane s % 64: lane L takes the j-th kept one
          const int jth = (lane - base) & (kWave - 1);
          const bool take = jth < __popcll(mask);
          const int src = take ? nth_set_bit(mask, jth) : lane;
          const double ws = __shfl(w, src);
          acc = acc + (take ? ws : 0.0);
          (void)pre;
        });
    const double total = wave_sum(acc);
    if (lane == 0) {
      counts[i] = cnt;
      norm[i] = zeros > 0 ? -static_cast<double>(zeros) : total;
    }
  }
}

// indptr = the scanned counts, clamped to int32 (the caller refuses a total past it); info[0] =
// the total in int64.
__global__ void grid_indptr_kernel(int64_t n, const int64_t* __restrict__ offs,
                                   int32_t* __restrict__ indptr, int64_t* __restrict__ info) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += stride) {
    const int64_t o = offs[i];
    indptr[i] = static_cast<int32_t>(min(o, static_cast<int64_t>(INT32_MAX)));
    if (i == n) info[0] = o;
  }
}

// Row i's entries into indices / values at indptr[i]: the same enumeration as the count pass.
// A slot outside the row's range (inputs that differ from the count pass's) is dropped.
__global__ __launch_bounds__(kBlock) void grid_fill_kernel(
    int64_t n, const double* __restrict__ coords, const double* __restrict__ lats,
    const double* __restrict__ lons, GridArgs g, const int32_t* __restrict__ indptr,
    const double* __restrict__ norm, int64_t nnz, int32_t* __restrict__ indices,
    float* __restrict__ values) {
  extern __shared__ double s_tab[];
  stage_tables(g, lats, lons, s_tab);
  const double *s_lat = s_tab, *s_cos = s_tab + g.n_lat, *s_lon = s_tab + 2 * g.n_lat;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); i < n;
       i += wstride) {
    const double lat = coords[2 * i], lon = coords[2 * i + 1];
    if (!coord_ok(lat, lon)) continue;
    const int64_t s = indptr[i], len = static_cast<int64_t>(indptr[i + 1]) - s;
    if (len <= 0) continue;
    const double nm = norm[i];
    scan_row(g, s_lat, s_cos, s_lon, lat * kDegToRad, lon * kDegToRad, lane,
             [&](bool keep, unsigned long long, int base, int pre, int col, double d) {
               const int64_t slot = base + pre;
               if (!keep || slot >= len || s + slot >= nnz || s < 0) return;
               double v;
               if (nm < 0.0)
                 v = (d == 0.0) ? 1.0 / -nm : 0.0;
               else
                 v = (1.0 / d) / nm;
               indices[s + slot] = col;
               values[s + slot] = static_cast<float>(v);
             });
  }
}

struct GridSpace {
  int64_t *counts, *offs;
  Tmp tmp;
  size_t total;
};

gcg_status grid_space(const char* fn, int64_t n, void* workspace, bool sized, GridSpace* s) {
  if (n < 0 || n >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n=%lld", fn, static_cast<long long>(n));
  Carver cv(workspace);
  s->counts = cv.take<int64_t>(n + 1);
  s->offs = cv.take<int64_t>(n + 1);
  TmpSize ts;
  if (sized) ts.add(GCG_CUB(DeviceScan::ExclusiveSum, s->counts, s->offs, static_cast<int>(n + 1)));
  return ts.take(fn, cv, &s->tmp, &s->total);
}

// The checks both passes share, and the kernels' constants.
gcg_status grid_args(const char* fn, int64_t n, const double* coords, int64_t n_lat,
                     const double* lats, int64_t n_lon, const double* lons, double radius_km,
                     double earth_radius_km, int exhaustive, GridArgs* g) {
  if (n < 0 || n >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n=%lld", fn, static_cast<long long>(n));
  if (n_lat < 1 || n_lon < 1 || n_lat > INT32_MAX || n_lon > INT32_MAX ||
      n_lat * n_lon > INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad grid %lld x %lld (1 .. 2^31 - 1 columns)", fn,
                static_cast<long long>(n_lat), static_cast<long long>(n_lon));
  if (2 * n_lat + n_lon > kMaxTable)
    return fail(GCG_ERR_INVALID_ARG, "%s: 2 * %lld latitudes + %lld longitudes exceed the %lld "
                "table entries that fit LDS", fn, static_cast<long long>(n_lat),
                static_cast<long long>(n_lon), static_cast<long long>(kMaxTable));
  if (!(std::isfinite(earth_radius_km) && earth_radius_km > 0.0))
    return fail(GCG_ERR_INVALID_ARG, "%s: earth_radius_km must be positive and finite", fn);
  if (!(radius_km > 0.0 && radius_km < kPi * earth_radius_km))
    return fail(GCG_ERR_INVALID_ARG, "%s: radius_km must lie in (0, pi * earth_radius_km)", fn);
  if (exhaustive != 0 && exhaustive != 1)
    return fail(GCG_ERR_INVALID_ARG, "%s: exhaustive must be 0 or 1", fn);
  if (n > 0 && (coords == nullptr || lats == nullptr || lons == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL coords, lats or lons", fn);
  if (!aligned(coords, 8) || !aligned(lats, 8) || !aligned(lons, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: coords, lats or lons not 8-B aligned", fn);
  g->n_lat = static_cast<int>(n_lat);
  g->n_lon = static_cast<int>(n_lon);
  g->radius = radius_km;
  g->two_r = 2 * earth_radius_km;
  g->dlat = radius_km / earth_radius_km * (1.0 + 1e-9) + 1e-12;
  g->sin_half = std::sin(radius_km / (2 * earth_radius_km));
  g->exhaustive = exhaustive;
  return GCG_OK;
}

dim3 row_grid(int64_t n) {
  const int64_t blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3(static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(blocks, 1), 8192)));
}

size_t table_bytes(const GridArgs& g) { return sizeof(double) * (2 * g.n_lat + g.n_lon); }

}  // namespace

extern "C" {

gcg_status gcg_grid_count_f64_workspace_bytes(int64_t n, size_t* bytes) {
  const char* fn = "gcg_grid_count_f64_workspace_bytes";
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  GridSpace s;
  if (gcg_status rc = grid_space(fn, n, nullptr, n > 0, &s)) return rc;
  *bytes = n > 0 ? s.total : 0;
  return GCG_OK;
}

gcg_status gcg_grid_count_f64(int64_t n, const double* coords, int64_t n_lat, const double* lats,
                              int64_t n_lon, const double* lons, double radius_km,
                              double earth_radius_km, int exhaustive, int32_t* indptr,
                              double* norm, int64_t* info_dev, void* workspace,
                              size_t workspace_bytes, gcg_stream_t stream) {
  const char* fn = "gcg_grid_count_f64";
  GridArgs g;
  if (gcg_status rc = grid_args(fn, n, coords, n_lat, lats, n_lon, lons, radius_km,
                                earth_radius_km, exhaustive, &g))
    return rc;
  if (n == 0) return GCG_OK;
  if (indptr == nullptr || norm == nullptr || info_dev == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL indptr, norm or info_dev", fn);
  if (!aligned(indptr, 4) || !aligned(norm, 8) || !aligned(info_dev, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: indptr, norm or info_dev not aligned to its element", fn);
  GridSpace s;
  // the fixed arrays first (host arithmetic), then the whole with the hipcub temporary
  if (gcg_status rc = grid_space(fn, n, workspace, false, &s)) return rc;
  if (gcg_status rc = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return rc;
  if (gcg_status rc = grid_space(fn, n, workspace, true, &s)) return rc;
  if (gcg_status rc = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(info_dev, 0, 2 * sizeof(int64_t), st));
  hipLaunchKernelGGL(grid_count_kernel, row_grid(n), dim3(kBlock), table_bytes(g), st, n, coords,
                     lats, lons, g, s.counts, norm, info_dev);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.counts, s.offs,
                                  static_cast<int>(n + 1), st)));
  hipLaunchKernelGGL(grid_indptr_kernel, dim3(grid_for(n + 1)), dim3(256), 0, st, n, s.offs,
                     indptr, info_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_grid_fill_f64(int64_t n, const double* coords, int64_t n_lat, const double* lats,
                             int64_t n_lon, const double* lons, double radius_km,
                             double earth_radius_km, int exhaustive, const int32_t* indptr,
                             const double* norm, int64_t nnz, int32_t* indices, float* values,
                             gcg_stream_t stream) {
  const char* fn = "gcg_grid_fill_f64";
  GridArgs g;
  if (gcg_status rc = grid_args(fn, n, coords, n_lat, lats, n_lon, lons, radius_km,
                                earth_radius_km, exhaustive, &g))
    return rc;
  if (nnz < 0 || nnz > INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad nnz=%lld", fn, static_cast<long long>(nnz));
  if (n == 0 || nnz == 0) return GCG_OK;
  if (indptr == nullptr || norm == nullptr || indices == nullptr || values == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL indptr, norm, indices or values", fn);
  if (!aligned(indptr, 4) || !aligned(norm, 8) || !aligned(indices, 4) || !aligned(values, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: an operand is not aligned to its element", fn);
  hipLaunchKernelGGL(grid_fill_kernel, row_grid(n), dim3(kBlock), table_bytes(g),
                     static_cast<hipStream_t>(stream), n, coords, lats, lons, g, indptr, norm, nnz,
                     indices, values);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
