// scratch.h -- the HIP side of scratch: stream-ordered device memory, the hipcub temporary and
// the caller-workspace size contract. Where the arrays sit is layout.h's Carver.
#pragma once

#include "common.h"

namespace gcg {

// Stream-ordered scratch of a call: freed on the stream it was allocated on when it leaves scope.
struct DevMem {
  void* p = nullptr;
  hipStream_t s = nullptr;
  ~DevMem() { if (p) (void)hipFreeAsync(p, s); }
  hipError_t alloc(size_t bytes, hipStream_t st) {
    s = st;
    return hipMallocAsync(&p, std::max<size_t>(bytes, 16), st);
  }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};

// A hipcub call is passed as a callable (void* tmp, size_t& bytes) -> hipError_t. GCG_CUB writes
// one from the primitive and the arguments after those two:
// GCG_CUB(DeviceScan::ExclusiveSum, in, out, n, stream).
#define GCG_CUB(prim, ...) \
  [&](void* cub_tmp, size_t& cub_bytes) { return hipcub::prim(cub_tmp, cub_bytes, __VA_ARGS__); }

// The temporary itself. hipcub takes the byte count by reference, so every run gets a fresh copy.
struct Tmp {
  void* p = nullptr;
  size_t bytes = 0;
  template <typename Call> hipError_t run(Call&& call) const {
    size_t b = bytes;
    return call(p, b);
  }
};

// The largest temporary over several sizing calls (tmp is null in each); the first failure
// stops the chain. take / take_exact end a layout: the temporary behind the arrays carved so
// far, floored at one byte or not as Carver's, then the total. No call added: no temporary.
struct TmpSize {
  size_t bytes = 0;
  hipError_t err = hipSuccess;
  template <typename Call> void add(Call&& call) {
    size_t b = 0;
    if (err == hipSuccess) err = call(static_cast<void*>(nullptr), b);
    bytes = std::max(bytes, b);
  }
  gcg_status take(const char* fn, Carver& cv, Tmp* tmp, size_t* total = nullptr) const {
    return place(fn, cv, cv.take<char>(bytes), tmp, total);
  }
  gcg_status take_exact(const char* fn, Carver& cv, Tmp* tmp, size_t* total = nullptr) const {
    return place(fn, cv, cv.take_exact<char>(bytes), tmp, total);
  }
  gcg_status status(const char* fn) const {
    if (err == hipSuccess) return GCG_OK;
    return fail(GCG_ERR_HIP, "%s: hipcub sizing: %s", fn, hipGetErrorString(err));
  }
  gcg_status place(const char* fn, const Carver& cv, char* p, Tmp* tmp, size_t* total) const {
    if (gcg_status st = status(fn)) return st;
    *tmp = {p, bytes};
    if (total != nullptr) *total = cv.used;
    return GCG_OK;
  }
};

// One allocation for the scratch of a function: `carve(Carver&)` takes the arrays, once over a
// null base for the size and once over the memory.
template <typename Carve> hipError_t alloc_carved(DevMem& mem, hipStream_t st, Carve&& carve) {
  Carver size(nullptr);
  carve(size);
  const hipError_t e = mem.alloc(size.used, st);
  if (e != hipSuccess) return e;
  Carver cv(mem.p);
  carve(cv);
  return hipSuccess;
}

// The size contract of a caller's workspace: NULL or fewer than `need` bytes is
// GCG_ERR_WORKSPACE, a base off `align` bytes GCG_ERR_MISALIGNED.
inline gcg_status check_workspace(const char* fn, const void* workspace, size_t workspace_bytes,
                                  size_t need, size_t align) {
  if (workspace == nullptr || workspace_bytes < need)
    return fail(GCG_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  if (!aligned(workspace, align))
    return fail(GCG_ERR_MISALIGNED, "%s: workspace not %zu-B aligned", fn, align);
  return GCG_OK;
}

}  // namespace gcg
