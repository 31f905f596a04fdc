// layout_check.cpp -- host-only check of csrc/layout.h: the carver and the bit-width helpers.
// Built with g++ -fsanitize=address,undefined by tests/test_layout.py; no HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../graphconvgeo_amd/csrc/layout.h"

using namespace gcg;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++failures;                                         \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
    }                                                     \
  } while (0)

struct Span {
  char* p;
  size_t bytes;
};

enum Floor { kOne, kExact, kBytes };

// One take sequence: arrays of 1-, 4- and 8-byte elements with the counts `n`, each taken the
// way `how` says. Returns `used`; with a base, also every array's span.
size_t carve(void* base, const std::vector<size_t>& n, const std::vector<Floor>& how,
             std::vector<Span>* spans) {
  Carver cv(base);
  for (size_t i = 0; i < n.size(); ++i) {
    const size_t before = cv.used;
    char* p = nullptr;
    size_t bytes = 0;
    switch (i % 3) {
      case 0:
        bytes = n[i] * 4;
        p = reinterpret_cast<char*>(how[i] == kOne     ? cv.take<int32_t>(n[i])
                                    : how[i] == kExact ? cv.take_exact<int32_t>(n[i])
                                                       : cv.take_bytes<int32_t>(bytes));
        break;
      case 1:
        bytes = n[i] * 8;
        p = reinterpret_cast<char*>(how[i] == kOne     ? cv.take<uint64_t>(n[i])
                                    : how[i] == kExact ? cv.take_exact<uint64_t>(n[i])
                                                       : cv.take_bytes<uint64_t>(bytes));
        break;
      default:
        bytes = n[i];
        p = how[i] == kOne     ? cv.take<char>(n[i])
            : how[i] == kExact ? cv.take_exact<char>(n[i])
                               : cv.take_bytes<char>(bytes);
    }
    const size_t grew = cv.used - before;
    // what each choice promises for the bytes it consumes
    if (how[i] == kOne) {
      CHECK(grew == align_up(std::max<size_t>(bytes, i % 3 == 0 ? 4 : i % 3 == 1 ? 8 : 1), 256),
            "take(%zu) grew %zu", n[i], grew);
      CHECK(grew >= 256, "a floored array has bytes of its own, grew %zu", grew);
    } else {
      CHECK(grew == align_up(bytes, 256), "exact take(%zu) grew %zu", n[i], grew);
      if (bytes == 0) CHECK(grew == 0, "an exact empty array takes nothing, grew %zu", grew);
    }
    CHECK(grew >= bytes, "array of %zu bytes got %zu", bytes, grew);
    if (base == nullptr) CHECK(p == nullptr, "sizing pass returned a pointer");
    if (spans != nullptr) spans->push_back({p, bytes});
  }
  return cv.used;
}

void check_carver(const std::vector<size_t>& n, const std::vector<Floor>& how) {
  const size_t need = carve(nullptr, n, how, nullptr);
  CHECK(need % 256 == 0, "used %zu is not a multiple of 256", need);
  // exactly `need` bytes: the sanitizer sees any write past an array's share
  char* buf = static_cast<char*>(std::aligned_alloc(256, std::max<size_t>(need, 256)));
  std::vector<Span> spans;
  const size_t used = carve(buf, n, how, &spans);
  CHECK(used == need, "null-base pass says %zu, real pass %zu", need, used);
  for (size_t i = 0; i < spans.size(); ++i) {
    CHECK(reinterpret_cast<uintptr_t>(spans[i].p) % 256 == 0, "array %zu not 256-B aligned", i);
    CHECK(spans[i].p >= buf && spans[i].p + spans[i].bytes <= buf + need, "array %zu outside", i);
    std::memset(spans[i].p, static_cast<int>(i + 1), spans[i].bytes);
    for (size_t j = 0; j < i; ++j) {
      const bool apart = spans[j].p + spans[j].bytes <= spans[i].p ||
                         spans[i].p + spans[i].bytes <= spans[j].p;
      CHECK(apart, "arrays %zu and %zu overlap", j, i);
      // floored arrays are told apart by address even when they are empty
      if (how[i] == kOne && how[j] == kOne) CHECK(spans[i].p != spans[j].p, "same address");
    }
  }
  for (size_t i = 0; i < spans.size(); ++i)  // nobody wrote into another array's share
    for (size_t b = 0; b < spans[i].bytes; ++b)
      if (spans[i].p[b] != static_cast<char>(i + 1)) {
        CHECK(false, "array %zu byte %zu overwritten", i, b);
        break;
      }
  std::free(buf);
}

// ---- bit widths: brute-force definitions ----------------------------------------------------

int hold_brute(uint64_t v) {  // the least b in 1 .. 64 with v < 2^b
  for (int b = 1; b < 64; ++b)
    if (static_cast<unsigned __int128>(v) < (static_cast<unsigned __int128>(1) << b)) return b;
  return 64;
}

int count_brute(int64_t n) {  // the least b in 1 .. 31 with ids 0 .. n - 1 below 2^b, else 31
  for (int b = 1; b < 31; ++b)
    if (static_cast<__int128>(n) <= (static_cast<__int128>(1) << b)) return b;
  return 31;
}

// minibatch.hip's former helper, capped at 32 bits
int key_bits_32(uint64_t max_key) {
  int b = 1;
  while (b < 32 && (uint64_t{1} << b) <= max_key) ++b;
  return b;
}

void check_bits() {
  std::vector<uint64_t> v{0, 1, 2};
  for (int k = 1; k <= 63; ++k) {
    const uint64_t p = uint64_t{1} << k;
    v.push_back(p - 1);
    v.push_back(p);
    v.push_back(p + 1);
  }
  v.push_back(~uint64_t{0});
  for (uint64_t x : v) {
    CHECK(bits_to_hold(x) == hold_brute(x), "bits_to_hold(%llu) = %d, brute force %d",
          static_cast<unsigned long long>(x), bits_to_hold(x), hold_brute(x));
    if (x <= static_cast<uint64_t>(INT64_MAX)) {
      const int64_t n = static_cast<int64_t>(x);
      CHECK(bits_to_count(n) == count_brute(n), "bits_to_count(%lld) = %d, brute force %d",
            static_cast<long long>(n), bits_to_count(n), count_brute(n));
    }
  }
  // the segmentation accepts batches x columns up to 2^32 - 2 (2^32 - 1 is the largest key and
  // the product itself stays free as the sentinel): there the 64-capped helper is the old one
  const uint64_t top = 0xfffffffeull;
  for (uint64_t x : v)
    if (x <= top) CHECK(bits_to_hold(x) == key_bits_32(x), "differs from the 32-capped at %llu",
                        static_cast<unsigned long long>(x));
  for (uint64_t x = 0; x <= top; x += 65521)
    CHECK(bits_to_hold(x) == key_bits_32(x), "differs from the 32-capped at %llu",
          static_cast<unsigned long long>(x));
  CHECK(bits_to_hold(top) == key_bits_32(top) && bits_to_hold(top) == 32, "at 2^32 - 2");
}

}  // namespace

int main() {
  const std::vector<size_t> counts{0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000};
  // every count with every floor choice, between two neighbours that would be overwritten
  for (size_t n : counts)
    for (Floor f : {kOne, kExact, kBytes})
      for (int shift = 0; shift < 3; ++shift) {  // shift: each element size meets each count
        std::vector<size_t> ns(static_cast<size_t>(shift), 3);
        std::vector<Floor> how(static_cast<size_t>(shift), kOne);
        ns.insert(ns.end(), {5, n, 7});
        how.insert(how.end(), {kOne, f, kExact});
        check_carver(ns, how);
      }
  // only empty arrays, of each kind and mixed
  check_carver({0, 0, 0, 0, 0, 0}, {kOne, kOne, kOne, kOne, kOne, kOne});
  check_carver({0, 0, 0, 0, 0, 0}, {kExact, kExact, kExact, kExact, kExact, kExact});
  check_carver({0, 0, 0, 0, 0, 0}, {kOne, kExact, kBytes, kExact, kOne, kBytes});
  // a layout like the library's: many arrays, a temporary at the end
  check_carver({40, 40, 40, 40, 6, 6, 41, 1, 3071}, {kExact, kExact, kExact, kExact, kExact, kExact,
                                                     kExact, kExact, kExact});
  check_carver({9, 9, 9, 9, 4, 0}, {kOne, kOne, kOne, kOne, kOne, kOne});
  check_bits();
  if (failures != 0) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("layout ok\n");
  return 0;
}
