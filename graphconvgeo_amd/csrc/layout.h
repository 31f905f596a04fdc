// layout.h -- host arithmetic of scratch layouts: alignment, radix-sort bit widths and the
// carver that places arrays in a workspace. Standard library only (no HIP), so a host-only
// program can include and check it (tests/c/layout_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace gcg {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Sort bits of a key that numbers n things (ids 0 .. n - 1), 1 .. 31.
inline int bits_to_count(int64_t n) {
  int b = 1;
  while (b < 31 && (int64_t{1} << b) < n) ++b;
  return b;
}

// Sort bits that hold every value in [0, max_value], 1 .. 64.
inline int bits_to_hold(uint64_t max_value) {
  int b = 1;
  while (b < 64 && (uint64_t{1} << b) <= max_value) ++b;
  return b;
}

constexpr size_t kScratchAlign = 256;

// Hands out consecutive 256-B aligned arrays of a scratch buffer. A null base is the sizing
// pass: the same sequence of calls, null pointers, the same `used`. The order of the calls is
// the layout.
struct Carver {
  char* p;
  size_t used = 0;
  explicit Carver(void* base) : p(static_cast<char*>(base)) {}
  // n elements and at least one: an empty array still gets an address of its own.
  template <typename T> T* take(size_t n) { return take_bytes<T>(std::max<size_t>(n, 1) * sizeof(T)); }
  // Exactly n elements: no bytes for n == 0, and the pointer is then the next array's.
  template <typename T> T* take_exact(size_t n) { return take_bytes<T>(n * sizeof(T)); }
  // A region sized in bytes, for arrays that deliberately share it.
  template <typename T> T* take_bytes(size_t bytes) {
    T* out = p ? reinterpret_cast<T*>(p + used) : nullptr;
    used += align_up(bytes, kScratchAlign);
    return out;
  }
};

}  // namespace gcg
