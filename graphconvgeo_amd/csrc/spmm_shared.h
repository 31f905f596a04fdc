// spmm_shared.h -- internals shared by the SpMM translation units (spmm.hip: float32 dense
// operand; spmm_bf16.hip: bf16 dense operand): the per-component vector helpers, the epilogue
// stores, the LDS hand-over barrier and the plan object. Not part of the C-ABI.
#pragma once

#include "common.h"

// The plan is one object for both operand types: it depends on H only.
struct gcg_spmm_plan {
  int64_t n_rows = 0, n_cols = 0, nnz = 0, n_out = 0;
  int ordered = 0;
  int64_t task_nnz = 0;
  int n_tasks = 0, n_long = 0, n_coop = 0, n_coop_rows = 0, n_sliced = 0;
  int64_t n_slots = 0, max_task_nnz = 0;
  int4* tasks = nullptr;     // device
  int4* longs = nullptr;     // device
  int32_t* out_rows = nullptr;  // device copy (nullptr = identity)
};

namespace gcg {

// Launches spmm_fixup_kernel (spmm.hip) for the split rows of a fast plan: adds the f32 segment
// sums of the workspace in order and applies the epilogue.
gcg_status launch_spmm_fixup(const gcg_spmm_plan* plan, const float* ws, int64_t ldws, int K,
                             float* Y, int64_t ldy, const float* bias, int act, uint8_t* gate,
                             int64_t ldgate, hipStream_t stream);

namespace {  // one copy per translation unit

// ------------------------------------------------------------------------------------
// Vector helpers. Explicit per-component arithmetic keeps the rounding sequence
// exactly acc = acc + (v * z) per element.
// ------------------------------------------------------------------------------------
template <int VEC>
struct Vec {
  float x[VEC];
};

template <int VEC>
__device__ __forceinline__ Vec<VEC> load_vec(const float* __restrict__ p) {
  Vec<VEC> r;
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.x[0] = t.x; r.x[1] = t.y; r.x[2] = t.z; r.x[3] = t.w;
  } else if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r.x[0] = t.x; r.x[1] = t.y;
  } else {
    r.x[0] = *p;
  }
  return r;
}

// Non-temporal load: the gather hint's cold columns (HC = 1, gcg_spmm_csr_f32_planned_hint).
template <int VEC>
__device__ __forceinline__ Vec<VEC> load_vec_nt(const float* __restrict__ p) {
  Vec<VEC> r;
  if constexpr (VEC == 4) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v t = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
    r.x[0] = t[0]; r.x[1] = t[1]; r.x[2] = t[2]; r.x[3] = t[3];
  } else {
#pragma unroll
    for (int q = 0; q < VEC; ++q) r.x[q] = __builtin_nontemporal_load(p + q);
  }
  return r;
}

// Round 5: the dwordx4 output rows are stored non-temporal -- Y is written once and read by
// the next kernel long after L2 has turned over, and the default policy let it evict the gather
// hint's hot Z rows: World power-law 6.19-6.25 -> 6.15-6.18 ms, uniform 9.20-9.21 -> 9.13-9.16,
// the Twitter-US step's SpMMs -0.5..-1.3 % (profiles/r05/spmm_nontemporal_y.jsonl). Round 2
// measured the same change neutral, before the gather hint kept a hot set in L2.
template <int VEC>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const Vec<VEC>& v) {
  if constexpr (VEC == 4) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(f4v{v.x[0], v.x[1], v.x[2], v.x[3]}, reinterpret_cast<f4v*>(p));
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v.x[0], v.x[1]);
  } else {
    *p = v.x[0];
  }
}

__device__ __forceinline__ float apply_act(float y, int act) {
  // lasagne.nonlinearities.rectify -> theano.tensor.nnet.relu(x) = 0.5 * (x + abs(x))
  return act == GCG_ACT_RELU ? 0.5f * (y + fabsf(y)) : y;
}

// Rectify gate of a pre-activation x: Theano's relu(x) = 0.5*(x + |x|) has the gradient
// 0.5*g*(1 + sgn(x)) (mlpconv.py:77 via lasagne rectify), i.e. g, g/2 or 0 for x > 0, x == 0,
// x < 0. The byte keeps 2 * that factor: 2, 1, 0 (NaN -> 0). Read by gcg_relu_backward_gate_f32.
__device__ __forceinline__ uint32_t gate_code(float x) {
  return x > 0.0f ? 2u : (x == 0.0f ? 1u : 0u);
}

template <int VEC>
__device__ __forceinline__ void store_gate(uint8_t* __restrict__ p, const Vec<VEC>& v) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<uint32_t*>(p) = gate_code(v.x[0]) | (gate_code(v.x[1]) << 8) |
                                      (gate_code(v.x[2]) << 16) | (gate_code(v.x[3]) << 24);
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<uint16_t*>(p) =
        static_cast<uint16_t>(gate_code(v.x[0]) | (gate_code(v.x[1]) << 8));
  } else {
    *p = static_cast<uint8_t>(gate_code(v.x[0]));
  }
}

// Masked last vector (round 4, TL = 1): a width K that is not a multiple of VEC still runs the
// VEC-wide gathers when Z's rows are padded to a multiple of VEC (empty_dense: K = 930 -> 932
// floats). The last vector of a row reads Z's padding columns [K, roundVEC(K)) -- products
// that are never stored -- while bias loads, Y stores and gate bytes past K are masked.
// Full vectors (c + VEC <= K) take the plain path; TL = 0 compiles exactly the old code.
template <int VEC, int TL>
__device__ __forceinline__ Vec<VEC> load_bias(const float* __restrict__ b, int c, int K) {
  if (!TL || c + VEC <= K) return load_vec<VEC>(b + c);
  Vec<VEC> r;
#pragma unroll
  for (int q = 0; q < VEC; ++q) r.x[q] = c + q < K ? b[c + q] : 0.0f;
  return r;
}

template <int VEC, int TL>
__device__ __forceinline__ void store_out(float* __restrict__ yrow, int c, int K,
                                          const Vec<VEC>& v) {
  if (!TL || c + VEC <= K) {
    store_vec<VEC>(yrow + c, v);
    return;
  }
#pragma unroll
  for (int q = 0; q < VEC; ++q)
    if (c + q < K) yrow[c + q] = v.x[q];
}

template <int VEC, int TL>
__device__ __forceinline__ void store_gate_t(uint8_t* __restrict__ grow, int c, int K,
                                             const Vec<VEC>& v) {
  if (!TL || c + VEC <= K) return store_gate<VEC>(grow + c, v);
#pragma unroll
  for (int q = 0; q < VEC; ++q)
    if (c + q < K) grow[c + q] = static_cast<uint8_t>(gate_code(v.x[q]));
}
// Barrier for LDS hand-over between the waves of a workgroup: retires this wave's LDS
// operations only (the gathers stay in flight across it), then s_barrier.
__device__ __forceinline__ void lds_handover_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

inline gcg_status check_gate(const uint8_t* gate, int64_t ldgate, int64_t K, int act) {
  if (gate == nullptr) return GCG_OK;
  if (act != GCG_ACT_RELU) return fail(GCG_ERR_INVALID_ARG, "gate needs act = GCG_ACT_RELU");
  if (ldgate < K || ldgate % 4 != 0) return fail(GCG_ERR_INVALID_ARG, "ldgate=%lld: need >= K and %% 4 == 0", (long long)ldgate);
  if (!aligned(gate, 4)) return fail(GCG_ERR_MISALIGNED, "gate not 4-byte aligned");
  return GCG_OK;
}

}  // namespace
}  // namespace gcg
