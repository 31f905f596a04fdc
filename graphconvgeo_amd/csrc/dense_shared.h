// dense_shared.h -- what the dense translation units share: dense_gemm.hip (plain and f32-fused
// GEMM), dense_nt.hip (NT GEMM), dense_fused.hip (the bf16x6 fused output layer and the row
// epilogue) and dense_tn.hip (split-K TN). Every kernel template is defined in one of them only;
// a file that needs another's kernel calls the gcg::launch_* function declared here.
//
// Reference (Theano graph, host BLAS):
//   ConvolutionDenseLayer.get_output_for   T.dot(h, W) + b, softmax     mlpconv.py:86-95
//   MLPCONV.fit loss                        categorical_crossentropy(    mlpconv.py:229-230
//                                           softmax(logits), y).mean()
//   Theano grads of both                    (softmax - onehot)/T, g.W^T, h^T.g
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>

#include "common.h"
#include "scratch.h"

// ---------------------------------------------------------------------------------------
// Tile lists: every family's tiles are written here once. The `tile` argument of an entry point
// counts a list's rows in order, gcg_dense_tile_count reports the counts below, and each file
// builds its table and its dispatch to the instantiations from the same list.
// ---------------------------------------------------------------------------------------
#define GCG_TILE_ONE(...) +1

// Plain products (gcg_gemm): tile 0 = B through LDS, gemm_bl_kernel<G, WC>; tile 1 = B from L2
// straight to registers, gemm_kernel<RT, G, WR, WC, PF> with the register prefetch. The
// shape within a tile is a function of N (pick_gemm_shape).
#define GCG_GEMM_BL_TILES(X) X(4, 4) X(4, 2) X(5, 1) X(4, 1) X(3, 1) X(2, 1) X(1, 1)
#define GCG_GEMM_REG_TILES(X)                                                                 \
  X(4, 4, 1, 4, 1) X(4, 2, 1, 4, 1) X(4, 3, 1, 4, 1)                                          \
  X(2, 1, 4, 1, 1) X(2, 2, 4, 1, 1) X(2, 3, 4, 1, 1) X(2, 4, 4, 1, 1) X(2, 5, 4, 1, 1)
constexpr int kGemmTileCount = 1;

// The fused output layer on the f32 MFMA (gemm_kernel EPI = 1, RT = 2, WC = 4): tiles 1..5 = the
// B register set split into this many rotating parts (0: one set, no split). G = 4 has every
// row, G = 2 and 3 the rows up to 4 parts, G = 1 its one register-prefetch form.
#define GCG_FUSED_PARTS(X) X(0) X(2) X(4) X(8) X(16)
constexpr int kFusedTileCount = 0 GCG_FUSED_PARTS(GCG_TILE_ONE);
// ... on the bf16 matrix cores (gemm_fused6_kernel): tiles 1..3, see launch_fused6.
constexpr int kFused6TileCount = 3;

// NT GEMM on the f32 MFMA (gemm_nt_kernel): X(RT, G, WR, WC, S, PF, KC, BF), tile = row number.
// BF = 1: the tile that also runs bf16x6 with both operands split in the loop (no workspace).
// Measured on one MI355X (tools/exp_gemm_nt.py, TFLOP/s on 840k x 300 x 930 / 840k x 930 x 300
// / 450k x 300 x 256 / 450k x 256 x 300): 16-deep chunks in a 4-stage ring (2,1,4,1,4,KC=16):
// 48 KB, 3 workgroups per CU, three chunks of DMA in flight: 118.0 / 118.0 / 114.4 / 111.2
// against 108.6 / 113.3 / 112.2 / 109.9 for the 32-deep 2-stage tile; 256 x 64 116 / 117.5;
// 128 x 128 91-115; 64 x 64 106-111. BM = 128 x BN = 64 with 48-72 KB of LDS runs 2-3
// workgroups per CU: one workgroup's barrier, DMA wait and epilogue overlap the others' MFMAs.
#define GCG_NT_TILES(X)                                                                       \
  X(2, 1, 4, 1, 4, 0, 16, 0) /*  0: default, 128 x 64, 16-deep chunks, 4 stages */            \
  X(2, 1, 4, 1, 2, 0, 32, 0) /*  1: 32-deep chunks, 2 stages */                               \
  X(2, 1, 4, 1, 2, 1, 32, 1) /*  2: ... both 16-deep steps' fragments read first */           \
  X(2, 1, 4, 1, 3, 1, 32, 0) /*  3: ... 3 stages */                                           \
  X(4, 1, 4, 1, 2, 0, 32, 0) /*  4: 256 x 64 */                                               \
  X(2, 2, 4, 1, 2, 0, 32, 0) /*  5: 128 x 128 */                                              \
  X(2, 1, 2, 2, 2, 0, 32, 0) /*  6: 2 x 2 waves */                                            \
  X(2, 1, 4, 1, 3, 0, 16, 0) /*  7: 16-deep, 3 stages */                                      \
  X(4, 1, 4, 1, 4, 0, 16, 0) /*  8: 256 x 64, 16-deep */                                      \
  X(2, 2, 4, 1, 4, 0, 16, 0) /*  9: 128 x 128, 16-deep */                                     \
  X(1, 1, 4, 1, 4, 0, 16, 0) /* 10: 64 x 64, 16-deep */
constexpr int kNtTileCount = 0 GCG_NT_TILES(GCG_TILE_ONE) - 1;  // tile 0 is a row

// bf16x6 NT tiles with the weight's planes pre-split: X(RT, G, WR, WC, S), tile = row number
// from 1. S = 0: gemm_nt3r_kernel (A in registers), S = 1: the same with the weight planes read
// one slot ahead (PL), S = 2: gemm_nt3_kernel (A through the LDS-DMA ring).
// Measured (tools/exp_gemm_bf16x6.py, one box, f32-equivalent TFLOP/s; f32 MFMA kernel 113-119):
//   shape (M x K x N)     LDS A: 2,1,4,1,2  2,2,4,1,2  2,1,4,2,2 | register A: 2,1,4,1  2,2,4,1  4,1,4,1
//   840k x 300 x 930           146          151-156     154-155  |             164-165  170-172  151-154
//   840k x 930 x 300           167          165-166     155      |             159-160  164      154-157
//   1.4M x 300 x 930           146          151-152     154-155  |             165-166  171      151
//   450k x 300 x 256           138-141      155         154-155  |             155-157  168-170  141-142
//   450k x 256 x 300           136          138-139     134-137  |             143-145  142      129
// Default: register A, 128 rows x 64 G columns, G in 1..3:
//                       G = 1      G = 2      G = 3
//   840k x 300 x 930    166-168    171-173    175-176   (N padded to 960 / 1024 / 960)
//   840k x 930 x 300    162-163    166        170-172   (320 / 384 / 384)
//   450k x 300 x 256    157-160    170-172    122       (256 / 256 / 384)
//   450k x 256 x 300    144.5      142-144    137-138   (320 / 384 / 384)
// Rule: the G padding N least (ties: the larger G -- fewer re-reads of A); for K > 512 the
// largest G within 1.25 x the least padding (a long k loop amortises the wider tile's waste).
#define GCG_NT3_TILES(X)                                                                      \
  X(2, 1, 4, 1, 0) /* 1: register A, 128 x 64 */                                              \
  X(2, 2, 4, 1, 0) /* 2: register A, 128 x 128 */                                             \
  X(2, 3, 4, 1, 0) /* 3: register A, 128 x 192 */                                             \
  X(4, 1, 4, 1, 0) /* 4: register A, 256 x 64 */                                              \
  X(2, 1, 4, 1, 2) /* 5: LDS A, 128 x 64 */                                                   \
  X(2, 2, 4, 1, 2) /* 6: LDS A, 128 x 128 */                                                  \
  X(2, 1, 4, 2, 2) /* 7: LDS A, 2 column waves */                                             \
  X(4, 1, 4, 1, 2) /* 8: LDS A, 256 x 64 */                                                   \
  X(2, 3, 4, 1, 1) /* 9: register A, 128 x 192, weight planes read one slot ahead (PL) */
constexpr int kNt3TileCount = 0 GCG_NT3_TILES(GCG_TILE_ONE);

// Split-K TN layouts (gemm_tn_partial_kernel): X(MG, NG, PD, WM, OCC). gcg_gemm_tn tile = row
// number from 1; each was measured by a script that is no longer in the tree, and the default
// (tn_plan) is a function of the shape only. GCG_TN_STACKED: the forms only the default takes,
// M / 64 < 4 waves stacked along M (4 waves: tile 5).
#define GCG_TN_TILES(X)                                                                       \
  X(1, 2, 8, 1, 0)  /* 1: round-2 workgroup tiles (4 waves side by side, 64 x 256 NG) */      \
  X(1, 3, 8, 0, 0)  /* 2: per-wave 64 x 192, 1 wave per SIMD, 8-deep ring */                  \
  X(1, 2, 8, 0, 0)  /* 3: per-wave 64 x 128, 1 wave per SIMD */                               \
  X(1, 3, 12, 0, 0) /* 4: per-wave 64 x 192, 12-deep ring */                                  \
  X(1, 1, 8, 4, 0)  /* 5: 4 waves stacked along M */                                          \
  X(1, 3, 3, 0, 2)  /* 6: per-wave 64 x 192, 2 waves per SIMD (the default at N = 930) */     \
  X(1, 2, 6, 0, 2)  /* 7: per-wave 64 x 128, 2 waves per SIMD */
#define GCG_TN_STACKED(X) X(1, 1, 8, 1, 0) X(1, 1, 8, 2, 0) X(1, 1, 8, 3, 0)
constexpr int kTnTileCount = 0 GCG_TN_TILES(GCG_TILE_ONE);

namespace gcg {

// C = act(A . B + bias) operands of the NT family (B = Bt, N x K).
struct NtArgs {
  int M, N, K;
  const float *A, *Bt, *bias;
  int64_t lda, ldb, ldc;
  int act;
  float* C;
};

// The fused output layer's operands: P . W + b -> softmax, cross-entropy, hits, and the logits
// gradient or the probabilities in C (gcg_project_softmax_xent).
struct FusedArgs {
  int M, N, K;
  const float *A, *B, *bias;
  int64_t lda, ldb, ldc;
  float* C;
  const int32_t* labels;
  float scale;
  const float* scale_dev;
  float *loss_rows, *correct_rows;
  const float* row_w;
};

// dense_gemm.hip: the fused layer on the f32 MFMA, gemm_kernel<..., EPI = 1> (tile 0..5).
gcg_status launch_gemm_fused_f32(const FusedArgs& a, int tile, hipStream_t st);
// dense_nt.hip: split3_rows_kernel, the bf16 planes of N rows of K elements (element (n, k) at
// Bt + n * ldb + k * kstride) into `out`; n_out > 0: the fused layer's layout, zero rows up to n_out.
gcg_status launch_split3_rows(int N, int K, const float* Bt, int64_t ldb, int64_t kstride,
                              int n_out, unsigned* out, hipStream_t st);

namespace {  // one copy per translation unit

using f4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// f32 products on the bf16 matrix cores ("bf16x6", MX = 1 below): x = x0 + x1 + x2 with each
// plane the round-to-nearest bf16 of what the planes before it left (8 significant bits each,
// |x1| <= 2^-9 |x|, |x2| <= 2^-17 |x|, x - (x0 + x1 + x2) <= 2^-26 |x|). a . b keeps the six
// plane products of order <= 2^-16 -- a0b0, a0b1, a1b0, a0b2, a1b1, a2b0 -- each exact in the
// f32 accumulator; the dropped a1b2 + a2b1 + a2b2 are <= 2^-25 |a||b|, below f32 rounding. NaN
// propagates (through plane 0 and the NaN residuals); an infinite or > 3.39e38 operand gives a
// non-finite tile, which f32_tile below recomputes with f32 products (f32 semantics).
using f8 = __attribute__((ext_vector_type(8))) float;
using bf8 = __attribute__((ext_vector_type(8))) __bf16;

using f2 = __attribute__((ext_vector_type(2))) float;
using bf2 = __attribute__((ext_vector_type(2))) __bf16;
using u4v = __attribute__((ext_vector_type(4))) unsigned;

// one pair: packed bf16 (v_cvt_pk_bf16_f32) and the f32 residual x - bf16(x), unpacked from the
// packed word by a shift / mask instead of a second conversion
__device__ __forceinline__ unsigned split_pair(f2& x) {
  const unsigned p = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf2));
  const f2 h = {__builtin_bit_cast(float, p << 16), __builtin_bit_cast(float, p & 0xffff0000u)};
  x = x - h;
  return p;
}
__device__ __forceinline__ void split3(const f8 x, bf8& h0, bf8& h1, bf8& h2) {
  u4v p0, p1, p2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f2 r = {x[2 * i], x[2 * i + 1]};
    p0[i] = split_pair(r);
    p1[i] = split_pair(r);
    p2[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf2));
  }
  h0 = __builtin_bit_cast(bf8, p0);
  h1 = __builtin_bit_cast(bf8, p1);
  h2 = __builtin_bit_cast(bf8, p2);
}
__device__ __forceinline__ f4 mfma_bf(bf8 a, bf8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// The six plane products of one A fragment (planes a[0] a[1] a[2]) and one B fragment (b0 b1
// b2) into c, smallest planes first. A lane's 32-deep fragment holds k = kc0 + 4q + i (low
// half, elements 0-3) and kc0 + 16 + 4q + i (high half). TP = the packed K tail (round 6): a
// chunk with r = K - kc0 <= 16 live k has both fragments' high halves zero, so every MFMA
// carries two plane products instead -- the high half holding another plane of the low half's
// k: a2b0 + a1b1, a0b2 + a1b0, a0b1 + a0b0, 3 MFMAs instead of 6. K = 300 ends in such a chunk
// (12 live k): the projection and the fused layer issue 57 MFMAs per output tile, not 60.
// The A side is packed once per chunk in place (pack_tail_a: the same three registers per
// fragment), the B side per slot. Every bf16x6 kernel packs the same way (bitwise equal).
// Kernels take the packed tail as a template flag the host sets from K, and peel the last
// chunk out of the K loop: a runtime branch between the two MFMA paths inside one kernel
// doubled the register pressure (100s of VGPRs spilled). Measured (one box, three rounds,
// profiles/r06/tail_packed_fence_ab.jsonl): NT projection 191.4 -> 199.0 TF, dP 179.7 ->
// 183.5 TF, fused layer unchanged (its last chunk waits on the weight-plane loads).
__device__ __forceinline__ bf8 lohi(bf8 lo, bf8 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 8, 9, 10, 11);
}
__device__ __forceinline__ void pack_tail_a(bf8 (&a)[3]) {
  const bf8 a0 = a[0], a1 = a[1], a2 = a[2];
  a[0] = lohi(a2, a1);
  a[1] = lohi(a0, a1);
  a[2] = lohi(a0, a0);
}
template <bool TP>
__device__ __forceinline__ f4 mfma6(const bf8 (&a)[3], bf8 b0, bf8 b1, bf8 b2, f4 c) {
  if constexpr (TP) {  // a packed by pack_tail_a
    c = mfma_bf(a[0], lohi(b0, b1), c);
    c = mfma_bf(a[1], lohi(b2, b0), c);
    return mfma_bf(a[2], lohi(b1, b0), c);
  } else {
    c = mfma_bf(a[2], b0, c);
    c = mfma_bf(a[1], b1, c);
    c = mfma_bf(a[0], b2, c);
    c = mfma_bf(a[1], b0, c);
    c = mfma_bf(a[0], b1, c);
    return mfma_bf(a[0], b0, c);
  }
}

// f32 semantics for the bf16x6 kernels (round 5). Three bf16 planes cannot carry an infinite
// operand (plane 0 = +-Inf, the residual Inf - Inf = NaN) nor one above bf16's largest finite
// value, 3.39e38 < FLT_MAX (plane 0 rounds to Inf); either leaves a NaN or Inf in the wave's
// accumulators, and so does a product or sum that overflows. A wave whose tile holds any
// non-finite value after the K loop (a wave-uniform ballot) recomputes its tile with f32 MFMA
// products (v_mfma_f32_16x16x4_f32) straight from global memory, in the f32 kernels' k order
// (16-deep steps, step s takes k = k0 + 4q + s, k >= K zeroed): Inf propagates, Inf * 0 and
// Inf - Inf give NaN, overflow gives Inf -- the f32 MFMA kernel's result for that tile. Finite
// data of sane range never takes the branch (~1 v_cmp_class per accumulator element).
// Padding rows never count: every kernel clamps the rows it loads past M (and NT kernels the
// weight rows past N) to the last valid one, so a padding row is non-finite only when a valid
// row is. MASKCOL: only columns < N count -- for the fused layer's in-register weight split
// (FX = 0), whose last vector reads the weight's padding columns [N, round4(N)), which may hold
// anything (a NaN there must not send the tile down the slow f32 path); every other
// kernel reads zeros or clamped columns past N and keeps the one-compare-per-element check (the
// masked form costs the fused layer ~2 % at the end of its K loop, PMC r06).
template <int RT, int G, bool MASKCOL = false>
__device__ __forceinline__ bool tile_nonfinite(const f4 (&acc)[RT][G][4], int N, int colw, int j) {
  if constexpr (!MASKCOL) {
    // x * 0 is 0 for finite x and NaN for Inf / NaN: one packed FMA per two accumulators
    // (round 6: the fused layer +2 % against a v_cmp_class per accumulator and the SGPR ors;
    // profiles/r06/dense_ab.jsonl)
    f2 s = {0.f, 0.f};
    const f2 z = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s = __builtin_elementwise_fma(f2{acc[t][g][e][0], acc[t][g][e][1]}, z, s);
          s = __builtin_elementwise_fma(f2{acc[t][g][e][2], acc[t][g][e][3]}, z, s);
        }
    return __builtin_amdgcn_ballot_w64(s[0] != s[0] || s[1] != s[1]) != 0;
  }
  bool bad = false;
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool col_in = !MASKCOL || colw + 64 * g + 4 * j + e < N;
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= col_in && !__builtin_isfinite(acc[t][g][e][r]);
    }
  return __builtin_amdgcn_ballot_w64(bad) != 0;
}
// B element (k, column n) at B + n * bn + k * bk (NT: Bt, bn = ldbt, bk = 1; fused: W, bn = 1,
// bk = ldw). rowb = the first row of the wave's 16 RT-row band; columns colw + 64 g + 4 j + e.
template <int RT, int G>
__device__ __forceinline__ void f32_tile(f4 (&acc)[RT][G][4], int M, int N, int K,
                                         const float* __restrict__ A, int64_t lda, int64_t rowb,
                                         const float* __restrict__ B, int64_t bn, int64_t bk,
                                         int colw, int j, int q) {
  int64_t ar[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t r = rowb + 16 * t + j;
    ar[t] = (r < M ? r : M - 1) * lda;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][g][e] = f4{0.f, 0.f, 0.f, 0.f};
  }
  for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * q + s;
      const bool kin = k < K;
      float a[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t) a[t] = kin ? A[ar[t] + k] : 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = colw + 64 * g + 4 * j + e;
          const float b = (kin && c < N) ? B[c * bn + static_cast<int64_t>(k) * bk] : 0.f;
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t][g][e] = mfma4(a[t], b, acc[t][g][e]);
        }
    }
  }
}

template <int W>
__device__ __forceinline__ float reduce16_max(float v) {
#pragma unroll
  for (int o = 1; o < W; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int W>
__device__ __forceinline__ float reduce16_sum(float v) {
#pragma unroll
  for (int o = 1; o < W; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W>
__device__ __forceinline__ int reduce16_min(int v) {
#pragma unroll
  for (int o = 1; o < W; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

constexpr float kNegInf = -std::numeric_limits<float>::infinity();

// Reductions over the 16 lanes of a DPP row (lanes 16q .. 16q + 15: one output row of the
// MFMA layout) with DPP lane swaps -- quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror -- instead of ds_bpermute shuffles. Every lane of the row ends with the same
// value (each step combines a and b as op(a, b) in one lane and op(b, a) in its partner).
// Round 6: each step is ONE DPP-sourced VALU op (v_add_f32_dpp / v_min_i32_dpp / v_max_f32_dpp)
// instead of a v_mov_b32_dpp and the op -- the row reductions are 64 of the fused epilogue's
// per-wave steps. update_dpp with bound_ctrl lets the compiler fold the permute into the add /
// min (every lane of these row-internal permutations is valid, so bound_ctrl never applies).
// fmaxf keeps canonicalising maxes around a folded permute, so the max is written out: the
// s_nop 1 covers the VALU-write -> DPP-read hazard the compiler cannot see inside the asm. Same
// values as the two-instruction forms: a + b == b + a, min / max commute (max over quiet NaNs
// keeps fmaxf's maxNum: a NaN operand gives the other).
template <int CTRL>
__device__ __forceinline__ float upd_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                               CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int upd_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
#define GCG_MAX_DPP(v, CTRL_ASM)                                                             \
  asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 " CTRL_ASM                              \
               " row_mask:0xf bank_mask:0xf bound_ctrl:1"                                  \
               : "=v"(v) : "v"(v))
__device__ __forceinline__ float row16_max(float v) {
  GCG_MAX_DPP(v, "quad_perm:[1,0,3,2]");
  GCG_MAX_DPP(v, "quad_perm:[2,3,0,1]");
  GCG_MAX_DPP(v, "row_half_mirror");
  GCG_MAX_DPP(v, "row_mirror");
  return v;
}
#undef GCG_MAX_DPP
__device__ __forceinline__ float row16_sum(float v) {
  v = v + upd_f<0xB1>(v);
  v = v + upd_f<0x4E>(v);
  v = v + upd_f<0x141>(v);
  return v + upd_f<0x140>(v);
}
__device__ __forceinline__ int row16_min(int v) {
  v = min(v, upd_i<0xB1>(v));
  v = min(v, upd_i<0x4E>(v));
  v = min(v, upd_i<0x141>(v));
  return min(v, upd_i<0x140>(v));
}

// ---- LDS-DMA and buffer-descriptor helpers (the image layouts: dense_nt.hip) ----
typedef __attribute__((address_space(1))) const void* glds_src_t;
typedef __attribute__((address_space(3))) void* glds_dst_t;

// 16 B per lane into LDS through a buffer descriptor (base + byte range; reads past the range
// return 0), lane byte offset voff
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), static_cast<short>(0), bytes,
                                           0x00020000);
}
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t r, float* lds_wave_base, int voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(lds_wave_base),
                                           16, voff, 0, 0, 0);
}

// the same with the non-temporal policy (a stream read once, e.g. the fused layer's A rows)
__device__ __forceinline__ void blds16_nt(__amdgpu_buffer_rsrc_t r, float* lds_wave_base, int voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(lds_wave_base),
                                           16, voff, 0, 0, 2);
}

__device__ __forceinline__ void glds16(const float* src, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(reinterpret_cast<glds_src_t>(reinterpret_cast<uintptr_t>(src)),
                                   (glds_dst_t)(lds_wave_base), 16, 0, 0);
}

// Swizzle key of image row r (see gemm_nt_kernel, dense_nt.hip). 4-slot rows: pi((r >> 2) & 3),
// pi = {0, 2, 3, 1}, the permutation that makes every ds_read_b128 lane group {0-3,12-15,20-27},
// ... of rows j = 0..15 x slots q land on distinct bank quads.
template <int SL>
__device__ __forceinline__ int nt_key(int r) {
  if constexpr (SL == 8) return r & 7;
  else return (0x78 >> (2 * ((r >> 2) & 3))) & 3;  // pi packed 2 bits each: 0, 2, 3, 1
}

// ---- Host side ----

// The packed K tail: the last 32-deep chunk holds <= 16 live k (mfma6, TP).
inline bool packed_tail(int K) { return K - 32 * ((K - 1) / 32) <= 16; }
// launch(std::true_type) for a K with the packed tail, launch(std::false_type) otherwise: the
// kernels take the tail as a template flag.
template <typename Launch>
gcg_status with_packed_tail(int K, Launch&& launch) {
  return packed_tail(K) ? launch(std::true_type{}) : launch(std::false_type{});
}

// Sizes of a product: the first (rows streamed: M, or TN's R) may be 0, the others not.
inline gcg_status check_sizes(const char* fn, const char (&names)[4], int64_t a, int64_t b,
                              int64_t c) {
  if (a >= 0 && b > 0 && c > 0 && a <= INT32_MAX && b <= INT32_MAX && c <= INT32_MAX) return GCG_OK;
  return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes %c=%lld %c=%lld %c=%lld", fn, names[0],
              static_cast<long long>(a), names[1], static_cast<long long>(b), names[2],
              static_cast<long long>(c));
}

inline gcg_status check_act(const char* fn, int act) {
  if (act == GCG_ACT_NONE || act == GCG_ACT_RELU) return GCG_OK;
  return fail(GCG_ERR_INVALID_ARG, "%s: unknown act %d", fn, act);
}

inline gcg_status check_dense(const char* fn, const float* p, int64_t ld, int64_t cols, bool vec4) {
  if (p == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: null operand", fn);
  if (ld < cols) return fail(GCG_ERR_INVALID_ARG, "%s: leading dimension %lld < %lld", fn,
                             static_cast<long long>(ld), static_cast<long long>(cols));
  if (vec4 && (ld % 4 != 0 || !aligned(p, 16)))
    return fail(GCG_ERR_MISALIGNED, "%s: operand needs a 16-B aligned base and ld %% 4 == 0", fn);
  if (!aligned(p, 4)) return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  return GCG_OK;
}

// Per-call arithmetic and tile: the math and tile arguments of the entry points.
inline gcg_status check_opts(const char* fn, int op, int math, int tile) {
  const int n = gcg_dense_tile_count(op, math);
  if (n < 0) return fail(GCG_ERR_INVALID_ARG, "%s: math %d not available for this product", fn, math);
  if (tile < 0 || tile > n)
    return fail(GCG_ERR_INVALID_ARG, "%s: tile %d outside 0..%d", fn, tile, n);
  return GCG_OK;
}

// gemm_kernel / gemm_fused6_kernel read B through a 32-bit buffer range (K * ldb * 4 bytes)
inline gcg_status check_b_range(const char* fn, int64_t K, int64_t ldb) {
  if (K * ldb * 4 < (int64_t{1} << 31)) return GCG_OK;
  return fail(GCG_ERR_INVALID_ARG, "%s: B of %lld x %lld floats exceeds the 2 GB buffer range", fn,
              static_cast<long long>(K), static_cast<long long>(ldb));
}

// check_workspace for the entries that take the byte count signed: a negative count holds nothing.
inline gcg_status check_workspace_i64(const char* fn, const void* ws, int64_t ws_bytes,
                                      int64_t need) {
  return check_workspace(fn, ws, static_cast<size_t>(std::max<int64_t>(ws_bytes, 0)),
                         static_cast<size_t>(need), 16);
}

}  // namespace
}  // namespace gcg
