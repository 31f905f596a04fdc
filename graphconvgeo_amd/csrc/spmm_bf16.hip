// spmm_bf16.hip -- CSR x dense SpMM with the dense operand stored in bf16 (gfx950 / CDNA4).
//
// Y = act(H . widen(Zb) + b): the gathered rows are bf16 (uint16_t storage), every element is
// widened exactly (bf16 -> f32 is a 16-bit shift), product and sum stay f32, in storage order,
// mul and add rounded separately (-ffp-contract=off). For Zr = widen(bf16(Z)) the result is
// bitwise scipy float32 H @ Zr: the only approximation is the one round-to-nearest-even per
// operand element that gcg_rows_f32_to_bf16 makes. The gather is the SpMM's byte term
// (4 K nnz of a 51.7 GB World launch); here it is 2 K nnz.
//
// The float32 path (spmm.hip) is untouched: this translation unit has its own kernel and shares
// only the helpers of spmm_shared.h, the plan object and the fix-up kernel (f32 workspace).
//
//   * One wave per task as in spmm_rows_kernel; a lane owns VB consecutive columns per chunk:
//     VB = 8 (one 16-B gather per lane and nonzero, a 512-column panel in one instruction) or
//     VB = 1 (the narrow fallback: any ldz, 2-B aligned Z). The f32 kernel's two-chunk shape at
//     half width (8-B gathers of 4 bf16) was built and measured slower: World K = 300 power-law
//     3.91 vs 3.77 ms, uniform 4.74 vs 4.08 (profiles/bf16_gather/ab_layout.jsonl); not kept.
//   * The (col, val) pairs of a batch are one coalesced vector load per wave (lane u holds
//     nonzero u), prefetched one batch ahead and moved to SGPRs with readlane: U can exceed the
//     16 that scalar-loaded pairs allow before the SGPRs spill, and a gathered row costs half
//     the VGPRs of an f32 one.
//   * A masked last vector: K % VB != 0 reads Zb's padding columns [K, roundVB(K)) inside the row
//     (ldz % 8 == 0 implies ldz >= round8(K)); their products are never stored.
//   * ordered plans: whole-workgroup rows (coop_row) and hub rows cut into two column slices
//     (coop_slice), the storage-order sum handed from wave to wave through LDS as in spmm.hip.
//   * No narrow-row SUB path: narrow K runs one row per wave.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spmm_shared.h"

using namespace gcg;

// Gathered rows in flight per wave on large launches. Measured, Twitter-World K = 300, one box,
// interleaved (profiles/bf16_gather/ab_layout.jsonl), U = 16 / 24 / 32 (116 / 163 / ~195 VGPRs:
// 4 / 3 / 2 waves per SIMD): power-law (planned, gather hint) 3.32 / 3.77 / 5.05 ms, uniform
// (one row per wave) 4.19 / 4.08 / 4.57 ms. So planned launches take 16, plan-less ones 24.
#ifndef GCG_BF16_U_PLAN
#define GCG_BF16_U_PLAN 16
#endif
#ifndef GCG_BF16_U_ROW
#define GCG_BF16_U_ROW 24
#endif

namespace {

constexpr int kSmallU = 8;    // rows in flight per wave on small launches (occupancy first)
constexpr int kPlanU = GCG_BF16_U_PLAN;
constexpr int kRowU = GCG_BF16_U_ROW;
static_assert(kPlanU >= 2 && kPlanU <= kWave && kRowU >= 2 && kRowU <= kWave,
              "one lane per nonzero of a batch");

// VB bf16 elements as loaded: 16 B or one element.
template <int VB>
struct Raw {
  uint32_t w[(VB + 1) / 2];
};

template <int VB>
__device__ __forceinline__ Raw<VB> load_raw(const uint16_t* __restrict__ row, uint32_t off) {
  // a wave-uniform row base and a 32-bit unsigned byte offset: an SGPR-base load, no 64-bit
  // per-lane address
  const char* p = reinterpret_cast<const char*>(row) + off * static_cast<uint32_t>(sizeof(uint16_t));
  Raw<VB> r;
  if constexpr (VB == 8) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    r.w[0] = t.x; r.w[1] = t.y; r.w[2] = t.z; r.w[3] = t.w;
  } else {
    r.w[0] = *reinterpret_cast<const uint16_t*>(p);
  }
  return r;
}

// Non-temporal gather: the gather hint's cold columns.
template <int VB>
__device__ __forceinline__ Raw<VB> load_raw_nt(const uint16_t* __restrict__ row, uint32_t off) {
  const char* p = reinterpret_cast<const char*>(row) + off * static_cast<uint32_t>(sizeof(uint16_t));
  Raw<VB> r;
  if constexpr (VB == 8) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    const u4v t = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
    r.w[0] = t[0]; r.w[1] = t[1]; r.w[2] = t[2]; r.w[3] = t[3];
  } else {
    r.w[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
  }
  return r;
}

// Element q widened to f32: exact (the bf16 bits are the f32's upper half).
template <int VB>
__device__ __forceinline__ float widen(const Raw<VB>& r, int q) {
  if constexpr (VB == 1) return __builtin_bit_cast(float, r.w[0] << 16);
  const uint32_t w = r.w[q >> 1];
  return __builtin_bit_cast(float, (q & 1) ? (w & 0xffff0000u) : (w << 16));
}

// A lane's VB accumulators of a chunk as NH vectors of HV floats: the epilogue (bias, gate,
// rectify, Y stores) runs on 16-B halves through the helpers of spmm_shared.h.
template <int VB>
struct Lay {
  static constexpr int HV = VB >= 4 ? 4 : 1;
  static constexpr int NH = VB / HV;
};

// acc += v * widen(z), element by element, each operation rounded.
template <int VB>
__device__ __forceinline__ void fma_row(Vec<Lay<VB>::HV> (&acc)[Lay<VB>::NH], float v,
                                        const Raw<VB>& z) {
#pragma unroll
  for (int q = 0; q < VB; ++q) {
    float& a = acc[q / Lay<VB>::HV].x[q % Lay<VB>::HV];
    a = a + v * widen<VB>(z, q);
  }
}

// Accumulate nonzeros [s, e) of one row (s < e), storage order, U gathers in flight.
template <int VB, int NCH, int U, int HC>
__device__ __forceinline__ void accumulate_range(int s, int e, const int32_t* __restrict__ indices,
                                                 const float* __restrict__ vals,
                                                 const uint16_t* __restrict__ Z, int64_t ldz,
                                                 const int (&gcol)[NCH],
                                                 Vec<Lay<VB>::HV> (&acc)[NCH][Lay<VB>::NH]) {
  const int lane = threadIdx.x & (kWave - 1);
  const int lu = min(lane, U - 1);
  // lane u holds nonzero j0 + u, clamped into the row
  auto load_idx = [&](int j0, int& ci, float& vi) {
    const int jj = min(j0 + lu, e - 1);
    ci = indices[jj];
    vi = vals[jj];
  };
  int ci, cin;
  float vi, vin;
  load_idx(s, ci, vi);
  int j = s;
  for (; j + U <= e; j += U) {
    Raw<VB> z[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = __builtin_amdgcn_readlane(ci, u);
      const uint16_t* zrow = Z + static_cast<int64_t>(HC ? (c & 0x7fffffff) : c) * ldz;
      if (HC && c < 0) {  // gather hint: sign bit = cold column
#pragma unroll
        for (int k = 0; k < NCH; ++k) z[u][k] = load_raw_nt<VB>(zrow, gcol[k]);
      } else {
#pragma unroll
        for (int k = 0; k < NCH; ++k) z[u][k] = load_raw<VB>(zrow, gcol[k]);
      }
    }
    // the next batch's pairs land while the gathers fly (base clamped into the row)
    load_idx(j + U, cin, vin);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float v =
          __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vi), u));
#pragma unroll
      for (int k = 0; k < NCH; ++k) fma_row<VB>(acc[k], v, z[u][k]);
    }
    ci = cin;
    vi = vin;
  }
  const int rem = e - j;  // wave-uniform, < U
  if (rem > 0) {
    Raw<VB> z[U][NCH];
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
      if (u < rem) {
        const int c = __builtin_amdgcn_readlane(ci, u) & (HC ? 0x7fffffff : -1);
        const uint16_t* zrow = Z + static_cast<int64_t>(c) * ldz;
#pragma unroll
        for (int k = 0; k < NCH; ++k) z[u][k] = load_raw<VB>(zrow, gcol[k]);
      }
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
      if (u < rem) {
        const float v =
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vi), u));
#pragma unroll
        for (int k = 0; k < NCH; ++k) fma_row<VB>(acc[k], v, z[u][k]);
      }
  }
}

// Bias, gate bytes, rectify and the Y stores of one lane's chunk; everything past column K is
// masked (bias loads, gate bytes, Y stores).
template <int VB>
__device__ __forceinline__ void epilogue(Vec<Lay<VB>::HV> (&acc)[Lay<VB>::NH], int col, int K,
                                         float* __restrict__ yrow, const float* __restrict__ bias,
                                         int act, uint8_t* __restrict__ grow) {
  constexpr int HV = Lay<VB>::HV;
  constexpr int TL = HV == 4 ? 1 : 0;
#pragma unroll
  for (int h = 0; h < Lay<VB>::NH; ++h) {
    const int c = col + h * HV;
    if (c >= K) continue;
    Vec<HV> a = acc[h];
    if (bias != nullptr) {
      const Vec<HV> bv = load_bias<HV, TL>(bias, c, K);
#pragma unroll
      for (int q = 0; q < HV; ++q) a.x[q] = a.x[q] + bv.x[q];
    }
    if (grow != nullptr) store_gate_t<HV, TL>(grow, c, K, a);
#pragma unroll
    for (int q = 0; q < HV; ++q) a.x[q] = apply_act(a.x[q], act);
    store_out<HV, TL>(yrow, c, K, a);
  }
}

// One long row of an ordered plan by a whole workgroup: spmm.hip coop_row with bf16 gathers.
// The kWavesPerBlock waves gather kWavesPerBlock x U consecutive nonzeros per batch; wave w adds
// its U products to the running row sum in LDS, in order, then wave w + 1 continues: every
// addition is the single-wave loop's, in the same order.
template <int VB, int NCH, int U>
__device__ __forceinline__ void coop_row(int p, const int32_t* __restrict__ indptr,
                                         const int32_t* __restrict__ indices,
                                         const float* __restrict__ vals,
                                         const int32_t* __restrict__ out_rows,
                                         const uint16_t* __restrict__ Z, int64_t ldz,
                                         const int (&col)[NCH], const int (&gcol)[NCH],
                                         const bool (&on)[NCH], int K, float* __restrict__ Y,
                                         int64_t ldy, const float* __restrict__ bias, int act,
                                         uint8_t* __restrict__ gate, int64_t ldgate,
                                         float* __restrict__ sacc) {
  constexpr int HV = Lay<VB>::HV;
  constexpr int NH = Lay<VB>::NH;
  constexpr int WPB = kWavesPerBlock;
  constexpr int B = WPB * U;  // nonzeros per batch
  const int wave = uniform(static_cast<int>(threadIdx.x >> 6));
  const int lane = threadIdx.x & (kWave - 1);
  const int r = out_rows ? uniform(out_rows[p]) : p;
  const int s = uniform(indptr[r]);
  const int e = uniform(indptr[r + 1]);  // coop rows are never empty
  auto slot = [&](int k, int h) { return sacc + ((k * kWave + lane) * NH + h) * HV; };
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int q = 0; q < HV; ++q) slot(k, h)[q] = 0.0f;
  }
  const int lu = min(lane, U - 1);
  auto load_idx = [&](int j0, int& ci, float& vi) {
    const int jj = min(j0 + lu, e - 1);
    ci = indices[jj];
    vi = vals[jj];
  };
  Raw<VB> z[U][NCH];
  auto gather = [&](int ci) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = __builtin_amdgcn_readlane(ci, u) & 0x7fffffff;  // the hint's cold bit
      const uint16_t* zrow = Z + static_cast<int64_t>(c) * ldz;
#pragma unroll
      for (int k = 0; k < NCH; ++k) z[u][k] = load_raw<VB>(zrow, gcol[k]);
    }
  };
  int ci, cin;
  float vi, vin;
  load_idx(s + wave * U, ci, vi);
  gather(ci);
  load_idx(s + B + wave * U, cin, vin);
  lds_handover_barrier();
  for (int b = s; b < e; b += B) {
    for (int st = 0; st < WPB; ++st) {
      if (st == wave) {
        const int n = min(U, max(0, e - (b + wave * U)));  // this wave's nonzeros, uniform
        Vec<HV> acc[NCH][NH];
#pragma unroll
        for (int k = 0; k < NCH; ++k)
#pragma unroll
          for (int h = 0; h < NH; ++h) acc[k][h] = *reinterpret_cast<const Vec<HV>*>(slot(k, h));
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (u < n) {
            const float v = __builtin_bit_cast(
                float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vi), u));
#pragma unroll
            for (int k = 0; k < NCH; ++k) fma_row<VB>(acc[k], v, z[u][k]);
          }
#pragma unroll
        for (int k = 0; k < NCH; ++k)
#pragma unroll
          for (int h = 0; h < NH; ++h) *reinterpret_cast<Vec<HV>*>(slot(k, h)) = acc[k][h];
        // the next batch's gathers fly while the later waves of this batch add
        ci = cin;
        vi = vin;
        gather(ci);
        load_idx(b + 2 * B + wave * U, cin, vin);
      }
      lds_handover_barrier();
    }
  }
  if (wave != 0) return;
  float* yrow = Y + static_cast<int64_t>(p) * ldy;
  uint8_t* grow = gate != nullptr ? gate + static_cast<int64_t>(p) * ldgate : nullptr;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    if (!on[k]) continue;
    Vec<HV> a[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) a[h] = *reinterpret_cast<const Vec<HV>*>(slot(k, h));
    epilogue<VB>(a, col[k], K, yrow, bias, act, grow);
  }
}

// Main kernel: the task encoding of spmm_rows_kernel (spmm.hip).
//   tasks == nullptr : task w = the row of position w                   (plan-less path)
//   task.w <  0      : rows of positions [task.x, task.y)
//   task.w >= 0      : position task.x, nonzeros [task.y, task.z) -> workspace slot task.w
// The first n_coop tasks take a whole workgroup each: whole rows, or {position, slice, -4,
// slices} column slices of a hub row (SLC = 1 kernels, one-chunk layout: each slice sums all
// the row's nonzeros for its share of the panel's columns, rounded up to whole lanes).
template <int VB, int NCH, int U, int HC, int SLC>
__global__ __launch_bounds__(kBlock) void spmm_bf16z_kernel(
    const int4* __restrict__ tasks, int n_tasks, int n_coop, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const int32_t* __restrict__ out_rows, const uint16_t* __restrict__ Z, int64_t ldz, int K,
    float* __restrict__ Y, int64_t ldy, const float* __restrict__ bias, int act,
    float* __restrict__ ws, int64_t ldws, uint8_t* __restrict__ gate, int64_t ldgate) {
  constexpr int HV = Lay<VB>::HV;
  constexpr int NH = Lay<VB>::NH;
  constexpr int kCols = kWave * VB * NCH;  // columns per panel
  const int blk = static_cast<int>(blockIdx.x);
  const int lane = threadIdx.x & (kWave - 1);
  const int panel0 = static_cast<int>(blockIdx.y) * kCols;

  int col[NCH], gcol[NCH];  // output column / clamped gather column
  bool on[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    col[k] = panel0 + (k * kWave + lane) * VB;
    on[k] = col[k] < K;
    gcol[k] = on[k] ? col[k] : panel0;
  }
  if (blk < n_coop) {  // a whole-workgroup long row or a slice of one (uniform across the block)
    __shared__ __attribute__((aligned(16))) float sacc[kCols];
    const int4 t0 = tasks[blk];
    if (uniform(t0.z) == -4) {  // {position, slice, -4, slices}
      if constexpr (SLC && NCH == 1) {
        const int sl = uniform(t0.y), n_sl = uniform(t0.w);
        const int wp = min(kCols, K - panel0);  // panel width
        const int wsl = ((wp + n_sl - 1) / n_sl + VB - 1) / VB * VB;
        const int c0 = panel0 + sl * wsl;
        const int c1 = min(c0 + wsl, panel0 + wp);
        if (c0 >= c1) return;  // an empty slice (narrow last panel)
        int scol[1], sgcol[1];
        bool son[1];
        scol[0] = c0 + lane * VB;
        son[0] = scol[0] < c1;
        sgcol[0] = son[0] ? scol[0] : c0;
        coop_row<VB, 1, U>(uniform(t0.x), indptr, indices, vals, out_rows, Z, ldz, scol, sgcol,
                           son, K, Y, ldy, bias, act, gate, ldgate, sacc);
        return;
      } else {
        // a sliced plan on a kernel without slices: slice 0 runs the whole row
        if (uniform(t0.y) != 0) return;
      }
    }
    coop_row<VB, NCH, U>(uniform(t0.x), indptr, indices, vals, out_rows, Z, ldz, col, gcol, on, K,
                         Y, ldy, bias, act, gate, ldgate, sacc);
    return;
  }
  const int w = uniform(n_coop + (blk - n_coop) * kWavesPerBlock + (threadIdx.x >> 6));
  if (w >= n_tasks) return;

  int4 t;
  if (tasks != nullptr) {
    t = tasks[w];
    t.x = uniform(t.x); t.y = uniform(t.y); t.z = uniform(t.z); t.w = uniform(t.w);
  } else {
    t = make_int4(w, w + 1, -1, -1);
  }

  Vec<HV> acc[NCH][NH];
  auto clear = [&]() {
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int q = 0; q < HV; ++q) acc[k][h].x[q] = 0.0f;
  };
  if (t.w >= 0) {  // a segment of a split row: its partial sum goes to the f32 workspace
    clear();
    if (t.y < t.z) accumulate_range<VB, NCH, U, HC>(t.y, t.z, indices, vals, Z, ldz, gcol, acc);
    float* dst = ws + static_cast<int64_t>(t.w) * ldws;  // ldws = round4(K): whole halves fit
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int h = 0; h < NH; ++h)
        if (col[k] + h * HV < K) store_vec<HV>(dst + col[k] + h * HV, acc[k][h]);
    return;
  }

  for (int p = t.x; p < t.y; ++p) {
    const int r = out_rows ? uniform(out_rows[p]) : p;
    const int s = uniform(indptr[r]);
    const int e = uniform(indptr[r + 1]);
    clear();
    if (s < e) accumulate_range<VB, NCH, U, HC>(s, e, indices, vals, Z, ldz, gcol, acc);
    float* yrow = Y + static_cast<int64_t>(p) * ldy;
    uint8_t* grow = gate != nullptr ? gate + static_cast<int64_t>(p) * ldgate : nullptr;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
      if (on[k]) epilogue<VB>(acc[k], col[k], K, yrow, bias, act, grow);
  }
}

// ------------------------------------------------------------------------------------
// f32 rows -> bf16 rows, round to nearest even. NaN -> the quiet NaN 0x7FC0 (as torch's CPU
// conversion), +-Inf kept, finite values above the bf16 range round to Inf as RNE prescribes.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

// One thread per 8 destination columns: two 16-B loads, one 16-B store; columns [K, ldd) are
// written as zero. HBM-bound (4 B read, 2 B written per element), one pass, no LDS.
__global__ __launch_bounds__(256) void rows_to_bf16_vec8_kernel(int64_t n_vec, int vpr, int K,
                                                                const float* __restrict__ src,
                                                                int64_t lds,
                                                                uint16_t* __restrict__ dst,
                                                                int64_t ldd) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_vec;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t row = i / vpr;
    const int c = static_cast<int>(i - row * vpr) * 8;
    const float* s = src + row * lds + c;
    float x[8];
    if (c + 8 <= K) {  // lds % 4 == 0 and a 16-B base: both halves are aligned loads
      const float4 a = *reinterpret_cast<const float4*>(s);
      const float4 b = *reinterpret_cast<const float4*>(s + 4);
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
      x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = c + q < K ? s[q] : 0.0f;
    }
    uint4 o;
    o.x = bf16_rne(x[0]) | (bf16_rne(x[1]) << 16);
    o.y = bf16_rne(x[2]) | (bf16_rne(x[3]) << 16);
    o.z = bf16_rne(x[4]) | (bf16_rne(x[5]) << 16);
    o.w = bf16_rne(x[6]) | (bf16_rne(x[7]) << 16);
    *reinterpret_cast<uint4*>(dst + row * ldd + c) = o;
  }
}

// Any layout: one thread per destination element.
__global__ __launch_bounds__(256) void rows_to_bf16_scalar_kernel(int64_t n_el, int64_t K,
                                                                  const float* __restrict__ src,
                                                                  int64_t lds,
                                                                  uint16_t* __restrict__ dst,
                                                                  int64_t ldd) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t row = i / ldd, c = i - row * ldd;
    dst[row * ldd + c] = static_cast<uint16_t>(c < K ? bf16_rne(src[row * lds + c]) : 0u);
  }
}

// ------------------------------------------------------------------------------------
// Launch dispatch.
// ------------------------------------------------------------------------------------
struct Args {
  const int4* tasks;
  int n_tasks;  // plan-less: output rows
  int n_coop;
  const int32_t* indptr;
  const int32_t* indices;
  const float* vals;
  const int32_t* out_rows;
  const uint16_t* Z;
  int64_t ldz;
  int K;
  float* Y;
  int64_t ldy;
  const float* bias;
  int act;
  float* ws;
  int64_t ldws;
  uint8_t* gate;
  int64_t ldgate;
};

template <int VB, int NCH, int U, int HC, int SLC>
void launch_k(const Args& a, hipStream_t stream) {
  constexpr int kCols = kWave * VB * NCH;
  const dim3 grid(a.n_coop + (a.n_tasks - a.n_coop + kWavesPerBlock - 1) / kWavesPerBlock,
                  (a.K + kCols - 1) / kCols);
  hipLaunchKernelGGL((spmm_bf16z_kernel<VB, NCH, U, HC, SLC>), grid, dim3(kBlock), 0, stream,
                     a.tasks, a.n_tasks, a.n_coop, a.indptr, a.indices, a.vals, a.out_rows, a.Z,
                     a.ldz, a.K, a.Y, a.ldy, a.bias, a.act, a.ws, a.ldws, a.gate, a.ldgate);
}

// The wide layouts: the deep batch for the launches the f32 path gives its own (a gather hint,
// planned tasks of >= 256 nonzeros: kPlanU; one row per wave on a large graph: kRowU), else
// kSmallU -- more waves per SIMD matter more than the batch on a small graph.
template <int VB, int NCH>
void launch_wide(const Args& a, bool big, bool hint, bool sliced, hipStream_t stream) {
  if (hint) {
    if (sliced) return launch_k<VB, NCH, kPlanU, 1, 1>(a, stream);
    return launch_k<VB, NCH, kPlanU, 1, 0>(a, stream);
  }
  if (big && a.tasks == nullptr) return launch_k<VB, NCH, kRowU, 0, 0>(a, stream);
  if (big) {
    if (sliced) return launch_k<VB, NCH, kPlanU, 0, 1>(a, stream);
    return launch_k<VB, NCH, kPlanU, 0, 0>(a, stream);
  }
  if (sliced) return launch_k<VB, NCH, kSmallU, 0, 1>(a, stream);
  launch_k<VB, NCH, kSmallU, 0, 0>(a, stream);
}

// 16-B conditions of the wide layouts; anything else gathers single elements (VB = 1).
bool wide_ok(const Args& a) {
  return a.ldz % 8 == 0 && aligned(a.Z, 16) && a.ldy % 4 == 0 && aligned(a.Y, 16) &&
         (a.bias == nullptr || aligned(a.bias, 16)) && (a.ws == nullptr || aligned(a.ws, 16));
}

gcg_status launch(const Args& a, int64_t task_nnz, const int32_t* hint, bool sliced,
                  hipStream_t stream) {
  if (a.n_tasks <= 0 || a.K <= 0) return GCG_OK;
  if (wide_ok(a)) {
    Args h = a;
    if (hint != nullptr) h.indices = hint;
    const bool big = task_nnz >= 256 || (a.tasks == nullptr && a.n_tasks >= 65536);
    launch_wide<8, 1>(h, big, hint != nullptr, sliced, stream);
  } else if (a.K <= kWave) {
    launch_k<1, 1, kSmallU, 0, 0>(a, stream);
  } else {
    launch_k<1, 4, kSmallU, 0, 0>(a, stream);
  }
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status check_operands(const uint16_t* Z, int64_t ldz, float* Y, int64_t ldy, int64_t K,
                          const float* bias, int act) {
  // grid.y of the fix-up kernel is ceil(K / 64) <= 65535
  if (K < 0 || K > int64_t{65535} * kWave) return fail(GCG_ERR_INVALID_ARG, "bad K=%lld", (long long)K);
  if (K > 0 && (Z == nullptr || Y == nullptr)) return fail(GCG_ERR_INVALID_ARG, "Z or Y is NULL");
  if (ldz < K || ldy < K) return fail(GCG_ERR_INVALID_ARG, "ldz=%lld / ldy=%lld < K=%lld",
                                      (long long)ldz, (long long)ldy, (long long)K);
  if (!aligned(Z, 2)) return fail(GCG_ERR_MISALIGNED, "Z (bf16) not 2-byte aligned");
  if (!aligned(Y, 4) || (bias && !aligned(bias, 4)))
    return fail(GCG_ERR_MISALIGNED, "Y/bias not 4-byte aligned");
  if (act != GCG_ACT_NONE && act != GCG_ACT_RELU) return fail(GCG_ERR_INVALID_ARG, "bad act=%d", act);
  return GCG_OK;
}

}  // namespace

extern "C" {

gcg_status gcg_rows_f32_to_bf16(int64_t n, int64_t K, const float* src, int64_t lds,
                                uint16_t* dst, int64_t ldd, gcg_stream_t stream) {
  if (n < 0 || K < 0 || K > INT32_MAX) return fail(GCG_ERR_INVALID_ARG, "bad n=%lld / K=%lld", (long long)n, (long long)K);
  if (lds < K || ldd < K) return fail(GCG_ERR_INVALID_ARG, "lds=%lld / ldd=%lld < K=%lld",
                                      (long long)lds, (long long)ldd, (long long)K);
  if (n == 0 || ldd == 0) return GCG_OK;
  if (src == nullptr || dst == nullptr) return fail(GCG_ERR_INVALID_ARG, "src or dst is NULL");
  if (!aligned(src, 4) || !aligned(dst, 2)) return fail(GCG_ERR_MISALIGNED, "src / dst not element aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ldd % 8 == 0 && lds % 4 == 0 && aligned(src, 16) && aligned(dst, 16)) {
    const int vpr = static_cast<int>(ldd / 8);
    const int64_t n_vec = n * vpr;
    hipLaunchKernelGGL(rows_to_bf16_vec8_kernel, dim3(grid_for(n_vec) * 4), dim3(256), 0, st,
                       n_vec, vpr, int(K), src, lds, dst, ldd);
  } else {
    hipLaunchKernelGGL(rows_to_bf16_scalar_kernel, dim3(grid_for(n * ldd) * 4), dim3(256), 0, st,
                       n * ldd, K, src, lds, dst, ldd);
  }
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_spmm_csr_bf16z_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                  const int32_t* indptr, const int32_t* indices,
                                  const float* vals, const uint16_t* Zb, int64_t ldz, int64_t K,
                                  float* Y, int64_t ldy, const float* bias, int act,
                                  const int32_t* out_rows, int64_t n_out, uint8_t* gate,
                                  int64_t ldgate, gcg_stream_t stream) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || n_rows > INT32_MAX || nnz > INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "bad CSR shape n_rows=%lld n_cols=%lld nnz=%lld",
                (long long)n_rows, (long long)n_cols, (long long)nnz);
  if (out_rows == nullptr) n_out = n_rows;
  if (n_out < 0 || n_out > INT32_MAX) return fail(GCG_ERR_INVALID_ARG, "bad n_out=%lld", (long long)n_out);
  if (gcg_status st = check_operands(Zb, ldz, Y, ldy, K, bias, act)) return st;
  if (gcg_status st = check_gate(gate, ldgate, K, act)) return st;
  if (n_out > 0 && indptr == nullptr) return fail(GCG_ERR_INVALID_ARG, "indptr is NULL");
  if (nnz > 0 && (indices == nullptr || vals == nullptr)) return fail(GCG_ERR_INVALID_ARG, "indices/vals NULL");
  if (n_out == 0 || K == 0) return GCG_OK;
  const Args a{nullptr, int(n_out), 0, indptr, indices, vals, out_rows, Zb, ldz, int(K), Y, ldy,
               bias, act, nullptr, 0, gate, ldgate};
  return launch(a, 0, nullptr, false, static_cast<hipStream_t>(stream));
}

gcg_status gcg_spmm_csr_bf16z_f32_planned(const gcg_spmm_plan* plan, const int32_t* indptr,
                                          const int32_t* indices, const float* vals,
                                          const uint16_t* Zb, int64_t ldz, int64_t K, float* Y,
                                          int64_t ldy, const float* bias, int act, uint8_t* gate,
                                          int64_t ldgate, void* workspace,
                                          size_t workspace_bytes, const int32_t* gather_hint,
                                          gcg_stream_t stream) {
  if (plan == nullptr) return fail(GCG_ERR_INVALID_ARG, "plan is NULL");
  if (gcg_status st = check_operands(Zb, ldz, Y, ldy, K, bias, act)) return st;
  if (gcg_status st = check_gate(gate, ldgate, K, act)) return st;
  if (plan->n_out > 0 && indptr == nullptr) return fail(GCG_ERR_INVALID_ARG, "indptr is NULL");
  if (plan->nnz > 0 && (indices == nullptr || vals == nullptr)) return fail(GCG_ERR_INVALID_ARG, "indices/vals NULL");
  if (K == 0 || plan->n_tasks == 0) return GCG_OK;
  size_t need = 0;
  gcg_spmm_plan_workspace_bytes(plan, K, &need);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return fail(GCG_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
  if (need > 0 && !aligned(workspace, 16)) return fail(GCG_ERR_MISALIGNED, "workspace not 16-byte aligned");
  const int64_t ldws = (K + 3) & ~int64_t{3};
  float* ws = need > 0 ? static_cast<float*>(workspace) : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Args a{plan->tasks, plan->n_tasks, plan->n_coop, indptr, indices, vals, plan->out_rows,
               Zb, ldz, int(K), Y, ldy, bias, act, ws, ldws, gate, ldgate};
  if (gcg_status s = launch(a, plan->task_nnz, gather_hint, plan->n_sliced > 0, st)) return s;
  return launch_spmm_fixup(plan, ws, ldws, int(K), Y, ldy, bias, act, gate, ldgate, st);
}

}  // extern "C"
