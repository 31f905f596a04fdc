// haversine.h -- the great-circle distance every geolocation kernel shares (geo.hip, grid.hip),
// stated once so that they take the same decisions on the same inputs. All float64.
#pragma once

#include <hip/hip_runtime.h>

namespace gcg {
namespace {  // one copy per translation unit

constexpr double kPi = 3.14159265358979323846;
constexpr double kDegToRad = kPi / 180.0;

// The haversine package's distance between points given in radians; `a` is clamped to 1 so
// that rounding at antipodal points cannot produce a NaN.
__device__ __forceinline__ double haversine_rad(double lat1, double cos1, double lng1, double lat2,
                                                double cos2, double lng2, double two_r) {
  const double sa = sin((lat2 - lat1) * 0.5), so = sin((lng2 - lng1) * 0.5);
  const double a = sa * sa + cos1 * cos2 * (so * so);
  return two_r * asin(sqrt(fmin(a, 1.0)));
}

}  // namespace
}  // namespace gcg
