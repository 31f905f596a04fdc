/* A plain C99 caller of the geolocation entries of include/gcg_spmm.h on the GPU: the k-d-tree
 * labels of five points (the width tie -> axis 0 case: 3 leaves), their medians read off the
 * tree's sorted lists and through the general entry, the nearest class, the haversine distance
 * and geo_eval's distances and count -- hipMalloc'd buffers on a stream, no Python, no torch.
 * Exit code 0 = all checks passed; prints "geo abi ok". */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "gcg_spmm.h"

#define CHECK_HIP(x)                                                       \
  do {                                                                     \
    hipError_t e_ = (x);                                                   \
    if (e_ != hipSuccess) {                                                \
      printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
      return 10;                                                           \
    }                                                                      \
  } while (0)
#define CHECK_GCG(x)                                                           \
  do {                                                                         \
    gcg_status s_ = (x);                                                       \
    if (s_ != GCG_OK) {                                                        \
      printf("gcg status %d at line %d: %s\n", (int)s_, __LINE__, gcg_last_error()); \
      return 11;                                                               \
    }                                                                          \
  } while (0)
#define EXPECT(c)                                     \
  do {                                                \
    if (!(c)) {                                       \
      printf("line %d: %s is false\n", __LINE__, #c); \
      return 12;                                      \
    }                                                 \
  } while (0)

int main(void) {
  enum { N = 5 };
  const double locs[N * 2] = {0, 0, 1, 1, 0, 1, 1, 0, .5, .25};
  const int32_t want_labels[N] = {0, 2, 1, 2, 0};
  const double want_med[6] = {0.25, 0.125, 0.0, 1.0, 1.0, 0.5};
  const double radius = 6371.0088;
  hipStream_t st;
  CHECK_HIP(hipStreamCreate(&st));
  double *d_locs, *d_med, *d_med2, *d_dist;
  int32_t *d_labels, *d_plat, *d_plon, *d_ptr, *d_status, *d_idx;
  int64_t* d_count;
  CHECK_HIP(hipMalloc((void**)&d_locs, sizeof(locs)));
  CHECK_HIP(hipMalloc((void**)&d_med, sizeof(want_med)));
  CHECK_HIP(hipMalloc((void**)&d_med2, sizeof(want_med)));
  CHECK_HIP(hipMalloc((void**)&d_dist, sizeof(double) * N));
  CHECK_HIP(hipMalloc((void**)&d_labels, sizeof(int32_t) * N));
  CHECK_HIP(hipMalloc((void**)&d_plat, sizeof(int32_t) * N));
  CHECK_HIP(hipMalloc((void**)&d_plon, sizeof(int32_t) * N));
  CHECK_HIP(hipMalloc((void**)&d_ptr, sizeof(int32_t) * (N + 1)));
  CHECK_HIP(hipMalloc((void**)&d_idx, sizeof(int32_t) * N));
  CHECK_HIP(hipMalloc((void**)&d_status, sizeof(int32_t)));
  CHECK_HIP(hipMalloc((void**)&d_count, sizeof(int64_t)));
  CHECK_HIP(hipMemcpyAsync(d_locs, locs, sizeof(locs), hipMemcpyHostToDevice, st));

  /* argument checks come back as a status, before any launch */
  int64_t nc = -1, depth = -1, rb = -1;
  EXPECT(gcg_kdtree_fit_f64(N, d_locs, 0, d_labels, d_plat, d_plon, d_ptr, &nc, &depth, &rb,
                            d_status, st) == GCG_ERR_INVALID_ARG);
  EXPECT(strstr(gcg_last_error(), "bucket_size") != NULL);

  CHECK_GCG(gcg_kdtree_fit_f64(N, d_locs, 2, d_labels, d_plat, d_plon, d_ptr, &nc, &depth, &rb,
                               d_status, st));
  EXPECT(nc == 3 && depth == 2 && rb == depth + 2);
  int32_t labels[N], ptr[N + 1];
  CHECK_HIP(hipMemcpyAsync(labels, d_labels, sizeof(labels), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipMemcpyAsync(ptr, d_ptr, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, st));
  CHECK_GCG(gcg_segment_medians_f64(nc, N, d_locs, d_ptr, d_plat, d_plon, d_med, st));
  CHECK_GCG(gcg_class_medians_f64(N, d_locs, d_labels, nc, d_med2, d_status, st));
  double med[6], med2[6];
  int32_t status = -1;
  CHECK_HIP(hipMemcpyAsync(med, d_med, sizeof(med), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipMemcpyAsync(med2, d_med2, sizeof(med2), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipStreamSynchronize(st));
  EXPECT(status == 0);
  EXPECT(memcmp(labels, want_labels, sizeof(labels)) == 0);
  EXPECT(ptr[0] == 0 && ptr[1] == 2 && ptr[2] == 3 && ptr[3] == 5);
  EXPECT(memcmp(med, want_med, sizeof(med)) == 0 && memcmp(med2, want_med, sizeof(med2)) == 0);

  /* every point is nearest to its own class's median here, at a known distance */
  CHECK_GCG(gcg_nearest_class_f64(N, d_locs, nc, d_med, radius, d_idx, d_dist, st));
  int32_t idx[N];
  double near[N], dist[N];
  CHECK_HIP(hipMemcpyAsync(idx, d_idx, sizeof(idx), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipMemcpyAsync(near, d_dist, sizeof(near), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipStreamSynchronize(st));
  EXPECT(memcmp(idx, want_labels, sizeof(idx)) == 0);
  EXPECT(near[2] == 0.0);

  /* geo_eval with the true labels as predictions gives the same distances; all under 161 km */
  int64_t count = -1;
  CHECK_GCG(gcg_geo_eval_f64(N, d_labels, 0, d_locs, nc, d_med, radius, 161.0, d_dist, d_count,
                             d_status, st));
  CHECK_HIP(hipMemcpyAsync(dist, d_dist, sizeof(dist), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipStreamSynchronize(st));
  EXPECT(status == 0 && count == N);
  for (int i = 0; i < N; ++i) EXPECT(fabs(dist[i] - near[i]) < 1e-9);
  /* a prediction outside [0, C) is reported, never a silently wrong distance */
  CHECK_GCG(gcg_geo_eval_f64(N, d_labels, 0, d_locs, 2, d_med, radius, 161.0, d_dist, d_count,
                             d_status, st));
  CHECK_HIP(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipStreamSynchronize(st));
  EXPECT(status == 1);

  /* a quarter of a great circle: (0, 0) to (0, 90) */
  const double ab[4] = {0, 0, 0, 90};
  double quarter = 0;
  CHECK_HIP(hipMemcpyAsync(d_med, ab, sizeof(ab), hipMemcpyHostToDevice, st));
  CHECK_GCG(gcg_haversine_km_f64(1, d_med, d_med + 2, radius, d_dist, st));
  CHECK_HIP(hipMemcpyAsync(&quarter, d_dist, sizeof(double), hipMemcpyDeviceToHost, st));
  CHECK_HIP(hipStreamSynchronize(st));
  EXPECT(fabs(quarter - 10007.557221017962) < 1e-6);

  CHECK_HIP(hipFree(d_locs)); CHECK_HIP(hipFree(d_med)); CHECK_HIP(hipFree(d_med2));
  CHECK_HIP(hipFree(d_dist)); CHECK_HIP(hipFree(d_labels)); CHECK_HIP(hipFree(d_plat));
  CHECK_HIP(hipFree(d_plon)); CHECK_HIP(hipFree(d_ptr)); CHECK_HIP(hipFree(d_idx));
  CHECK_HIP(hipFree(d_status)); CHECK_HIP(hipFree(d_count));
  CHECK_HIP(hipStreamDestroy(st));
  printf("geo abi ok\n");
  return 0;
}
