// dense_tn.hip -- C = scale * A^T . B by split-K (gcg_gemm_tn): the weight gradients h^T . g /
// P^T . G: each split's partial tiles in exact f32 (gemm_tn_partial_kernel) or bf16x6
// (gemm_tn6_partial_kernel), summed in split order by gemm_tn_reduce_kernel.
#include "dense_shared.h"

using namespace gcg;

namespace {

// ---------------------------------------------------------------------------------------
// C = scale * A^T . B, the weight gradients h^T . g / P^T . G (Theano's grad of T.dot(h, W)
// w.r.t. W, mlpconv.py:88): reduction over R ~ 10^6 rows into a small M x N output.
// Split-K: blockIdx.z owns rows [z*rows_per_split, ...); each wave keeps a 64*MG x 64*NG
// accumulator tile. Lane (j, q) loads ONE dwordx4 of A's row t and one of B's row t per
// 64-wide group (t = t0 + q): element e of the A vector is row-slot j of the MFMA tile that
// owns the C rows m0 + 4j + e, element e' of the B vector the column-slot j of the tile owning
// the C columns n0 + 4j + e' -- so 2 loads feed 16 v_mfma_f32_16x16x4_f32 and a lane's
// accumulators hold 4 adjacent C columns (dwordx4 partial stores). A ring of PD register
// sets keeps PD steps of loads in flight. Partials [split][Mp][Np] are summed in split order
// by gemm_tn_reduce_kernel (deterministic), which applies scale (a device scalar).
// ---------------------------------------------------------------------------------------
// WM = 1: the workgroup's 4 waves sit side by side along N (tile 64*MG x 256*NG): they load
// the same A rows, and each 64-row band of C re-reads B. WM > 1 (round 3): WM waves stacked
// along M (tile 64*MG*WM x 64*NG, WM = 5 covers M = 300 in one tile): B -- the wide operand,
// G at 840k x 930 -- is read once per row and shared by the WM waves through L1, and the N
// tiles of one split (same XCD, remap) share A through L2.
// WM = 0 (round 3): every wave owns its own 64*MG x 64*NG tile, enumerated m fastest over
// (m tile, n tile, split), 4 consecutive wave tiles per workgroup (the 4 waves of a workgroup
// then share their B rows through L1), one wave per SIMD: the accumulators of a wide NG (3 or
// 5: N = 930 in 960 columns instead of the 1024 of 256-column workgroup tiles) live in the
// 512-register file beside a deep load ring.
// OCC = 2 keeps a per-wave (WM = 0) tile at 2 waves per SIMD (<= 256 registers: a shallow ring),
// so it can share CUs with kernels running beside it on other streams.
template <int MG, int NG, int PD, int WM = 1, int OCC = 0>
__global__ __launch_bounds__(WM <= 1 ? 256 : 64 * WM, (WM == 0 && OCC != 2) ? 1 : 2) void gemm_tn_partial_kernel(
    int R, int M, int N, const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
    int64_t ldb, int rows_per_split, float* __restrict__ part, int Mp, int Np, int mt, int nt,
    int remap) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  // 1-D grid of mt x nt x S tiles, m fastest. remap: XCD-aware bijection (workgroup b runs on
  // XCD b % 8; each XCD walks one contiguous range of tiles), so the mt x nt tiles of one
  // split -- which read the same rows of A and B -- share one XCD's L2.
  const int nwg = static_cast<int>(gridDim.x), b = static_cast<int>(blockIdx.x);
  int tile = b;
  if (remap) {
    const int xcd = b % 8, qq = nwg / 8, rr = nwg % 8;
    tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + b / 8;
  }
  const int wt = WM == 0 ? 4 * tile + wave : tile;  // WM = 0: the wave's own tile
  const int bx = wt % mt, by = (wt / mt) % nt, bz = wt / (mt * nt);
  const int m0 = WM == 0   ? bx * (64 * MG)
                 : WM == 1 ? bx * (64 * MG)
                           : bx * (64 * MG * WM) + wave * (64 * MG);
  const int n0 = WM == 0   ? by * (64 * NG)
                 : WM == 1 ? by * (256 * NG) + wave * (64 * NG)
                           : by * (64 * NG);
  // a wave wholly past N (or M), or past the last split, leaves at once (no LDS, no barriers)
  if (n0 >= N || (WM != 1 && m0 >= M)) return;
  if (static_cast<int64_t>(bz) * rows_per_split >= R) return;
  const int t_begin = bz * rows_per_split;
  const int t_end = min(R, t_begin + rows_per_split);
  const int m4 = (M + 3) & ~3, n4 = (N + 3) & ~3;
  int acol[MG], bcol[NG];
#pragma unroll
  for (int g = 0; g < MG; ++g) {
    const int c = m0 + 64 * g + 4 * j;
    acol[g] = c < m4 ? c : 0;  // rows of C past M: computed on a valid column, never stored
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int c = n0 + 64 * g + 4 * j;
    bcol[g] = c < n4 ? c : 0;
  }
  f4 acc[MG][NG][4][4];
#pragma unroll
  for (int a = 0; a < MG; ++a)
#pragma unroll
    for (int b = 0; b < NG; ++b)
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) acc[a][b][ea][eb] = f4{0.f, 0.f, 0.f, 0.f};

  f4 ra[PD][MG], rb[PD][NG];
  // A and B rows through buffer descriptors re-based at the step's first row (scalar work): the
  // range check covers only the rows left in the split, so rows past it read as 0 -- no per-lane
  // row clamp, select or 64-bit address arithmetic (round 3; the per-lane byte offsets are
  // constants). Host: lda, ldb < 2^27.
  uint32_t aoff[MG], boff[NG];
#pragma unroll
  for (int g = 0; g < MG; ++g) aoff[g] = static_cast<uint32_t>((q * static_cast<int>(lda) + acol[g]) * 4);
#pragma unroll
  for (int g = 0; g < NG; ++g) boff[g] = static_cast<uint32_t>((q * static_cast<int>(ldb) + bcol[g]) * 4);
  auto load = [&](int u, int t0) {
    // (readfirstlane: the descriptor must be provably wave-uniform, or hipcc emits a waterfall)
    const int left = __builtin_amdgcn_readfirstlane(min(max(t_end - t0, 0), 4));  // rows in split
    const int tb = __builtin_amdgcn_readfirstlane(left > 0 ? t0 : t_begin);
    const auto ar = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(A + static_cast<int64_t>(tb) * lda), static_cast<short>(0),
        left * static_cast<int>(lda) * 4, 0x00020000);
    const auto br = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(B + static_cast<int64_t>(tb) * ldb), static_cast<short>(0),
        left * static_cast<int>(ldb) * 4, 0x00020000);
#pragma unroll
    for (int g = 0; g < MG; ++g)
      ra[u][g] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ar, aoff[g], 0, 0));
#pragma unroll
    for (int g = 0; g < NG; ++g)
      rb[u][g] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(br, boff[g], 0, 0));
  };
  auto compute = [&](int u) {
#pragma unroll
    for (int a = 0; a < MG; ++a)
#pragma unroll
      for (int b = 0; b < NG; ++b)
#pragma unroll
        for (int ea = 0; ea < 4; ++ea)
#pragma unroll
          for (int eb = 0; eb < 4; ++eb)
            acc[a][b][ea][eb] = mfma4(ra[u][a][ea], rb[u][b][eb], acc[a][b][ea][eb]);
  };
  // steps of 4 rows; the ring is refilled PD steps ahead (loads past t_end are zeroed)
#pragma unroll
  for (int u = 0; u < PD; ++u) {
    load(u, t_begin + 4 * u);
    __builtin_amdgcn_sched_barrier(0);  // issue order = ring order (counted waits below)
  }
  // The scheduling barriers pin each refill behind its step's MFMAs: without them the machine
  // scheduler sinks every load next to its use (to cut register pressure) and the ring is gone
  // -- one exposed load latency per step (round 2, ISA: vmcnt(0) before each step's MFMAs).
  for (int t0 = t_begin; t0 < t_end; t0 += 4 * PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      compute(u);
      __builtin_amdgcn_sched_barrier(0);
      load(u, t0 + 4 * (u + PD));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // partial tile: lane holds C[m0 + 64a + 16q + 4r + ea][n0 + 64b + 4j + eb] in acc[a][b][ea][eb][r]
  float* dst = part + static_cast<int64_t>(bz) * Mp * Np;
#pragma unroll
  for (int a = 0; a < MG; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ea = 0; ea < 4; ++ea) {
        const int m = m0 + 64 * a + 16 * q + 4 * r + ea;
        float* row = dst + static_cast<int64_t>(m) * Np;
#pragma unroll
        for (int b = 0; b < NG; ++b) {
          const int n = n0 + 64 * b + 4 * j;
          *reinterpret_cast<f4*>(row + n) = f4{acc[a][b][ea][0][r], acc[a][b][ea][1][r],
                                               acc[a][b][ea][2][r], acc[a][b][ea][3][r]};
        }
      }
}

// gemm_tn6_partial_kernel (round 6): gemm_tn_partial_kernel's split-K A^T . B (the weight
// gradients dW2 = P^T . G and X_head^T . G) on the bf16 matrix cores (bf16x6, mfma6). Each wave
// owns a 64 (m) x 64 (n) tile of one split: per 32-row chunk, lane (j, q) loads rows
// t0 + 4q + i and t0 + 16 + 4q + i (i < 4) of A and B as dwordx4 of 4 adjacent columns (the
// fused layer's in-register weight load), which gives, for each of its 4 column slots e
// (column m0 + 4j + e), the 8 k-values of its MFMA fragment in the bf16x6 kernels' k order;
// the fragments are split into planes in registers. The D row rho of block (eA, eB) is
// m = m0 + 4 rho + eA, its column j is n = n0 + 4j + eB, so each lane stores 4 adjacent n of
// 16 rows. Rows past the split come from a buffer range that reads 0; columns past M / N are
// computed on a clamped column and never reach C (the reduce kernel reads m < M, n < N). A tile
// whose accumulators are not finite is recomputed with f32 products (v_mfma_f32_16x16x4_f32,
// one row t per k step) -- f32 semantics, as the other bf16x6 kernels.
__global__ __launch_bounds__(256, 2) void gemm_tn6_partial_kernel(
    int R, int M, int N, const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
    int64_t ldb, int rows_per_split, float* __restrict__ part, int Mp, int Np, int mt, int nt) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int nwg = static_cast<int>(gridDim.x), b = static_cast<int>(blockIdx.x);
  const int xcd = b % 8, qq = nwg / 8, rr = nwg % 8;  // XCD-aware order, as gemm_tn_partial
  const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + b / 8;
  const int wt = 4 * tile + wave;
  const int bx = wt % mt, by = (wt / mt) % nt, bz = wt / (mt * nt);
  const int m0 = bx * 64, n0 = by * 64;
  if (m0 >= M || n0 >= N) return;  // wave-uniform; no barriers in this kernel
  if (static_cast<int64_t>(bz) * rows_per_split >= R) return;
  const int t_begin = bz * rows_per_split;
  const int rows = min(R, t_begin + rows_per_split) - t_begin;
  const int m4 = (M + 3) & ~3, n4 = (N + 3) & ~3;
  const int ac = m0 + 4 * j < m4 ? m0 + 4 * j : 0;
  const int bc = n0 + 4 * j < n4 ? n0 + 4 * j : 0;
  const int lda4 = static_cast<int>(lda) * 4, ldb4 = static_cast<int>(ldb) * 4;
  const float* Ab = A + static_cast<int64_t>(t_begin) * lda;
  const float* Bb = B + static_cast<int64_t>(t_begin) * ldb;
  const int aoff = 4 * q * lda4 + ac * 4, boff = 4 * q * ldb4 + bc * 4;
  const int nch = (rows + 31) / 32;
  auto load = [&](int c, f4 (&xa)[8], f4 (&xb)[8]) {
    const int live = min(rows - 32 * c, 32);  // rows of this chunk inside the split
    const auto ra = brsrc(Ab + static_cast<int64_t>(32 * c) * lda, live * lda4);
    const auto rb = brsrc(Bb + static_cast<int64_t>(32 * c) * ldb, live * ldb4);
    // (the row offset in the VGPR offset, which the range check covers: rows past the split
    // must read 0, they are the next split's)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xa[i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, aoff + i * lda4, 0, 0));
      xa[4 + i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, aoff + (16 + i) * lda4, 0, 0));
      xb[i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rb, boff + i * ldb4, 0, 0));
      xb[4 + i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rb, boff + (16 + i) * ldb4, 0, 0));
    }
  };
  f4 acc[4][4];
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = f4{0.f, 0.f, 0.f, 0.f};
  f4 xa[8], xb[8], na[8], nb[8];
  load(0, xa, xb);
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) load(c + 1, na, nb);  // one chunk ahead
    bf8 ap[4][3];
#pragma unroll
    for (int ea = 0; ea < 4; ++ea) {
      const f8 y = {xa[0][ea], xa[1][ea], xa[2][ea], xa[3][ea], xa[4][ea], xa[5][ea], xa[6][ea], xa[7][ea]};
      split3(y, ap[ea][0], ap[ea][1], ap[ea][2]);
    }
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) {
      const f8 y = {xb[0][eb], xb[1][eb], xb[2][eb], xb[3][eb], xb[4][eb], xb[5][eb], xb[6][eb], xb[7][eb]};
      bf8 b0, b1, b2;
      split3(y, b0, b1, b2);
      // the chunk's six plane products into a fresh accumulator, then one f32 add into the
      // tile's: a split's thousands of rows cost one rounding of the running sum per 32 rows,
      // not six (accumulated straight into the running sum, World dW2 came out ~3 x less
      // accurate than the f32 kernel's, whose MFMA adds 4 rows per rounding)
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
        acc[ea][eb] += mfma6<false>(ap[ea], b0, b1, b2, f4{0.f, 0.f, 0.f, 0.f});
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      xa[i] = na[i];
      xb[i] = nb[i];
    }
  }
  // f32 semantics for Inf / huge operands (x * 0 is NaN only for a non-finite x)
  f2 sn = {0.f, 0.f};
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) {
      sn = __builtin_elementwise_fma(f2{acc[ea][eb][0], acc[ea][eb][1]}, f2{0.f, 0.f}, sn);
      sn = __builtin_elementwise_fma(f2{acc[ea][eb][2], acc[ea][eb][3]}, f2{0.f, 0.f}, sn);
    }
  if (__builtin_amdgcn_ballot_w64(sn[0] != sn[0] || sn[1] != sn[1]) != 0) {
#pragma unroll
    for (int ea = 0; ea < 4; ++ea)
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = f4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < rows; t += 4) {  // k step: row t + q
      const int live = min(rows - t, 4);
      const auto ra = brsrc(Ab + static_cast<int64_t>(t) * lda, live * lda4);
      const auto rb = brsrc(Bb + static_cast<int64_t>(t) * ldb, live * ldb4);
      const f4 a = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, q * lda4 + ac * 4, 0, 0));
      const f4 bv = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rb, q * ldb4 + bc * 4, 0, 0));
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = mfma4(a[ea], bv[eb], acc[ea][eb]);
    }
  }
  float* pt = part + static_cast<int64_t>(bz) * Mp * Np;
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 4 * (4 * q + r) + ea;
      const f4 o = {acc[ea][0][r], acc[ea][1][r], acc[ea][2][r], acc[ea][3][r]};
      *reinterpret_cast<f4*>(pt + static_cast<int64_t>(m) * Np + n0 + 4 * j) = o;
    }
}

// C[m][n] = scale * sum over the S split partials part[s][m][n], deterministic. One workgroup
// per (row m, 64 column quads): wave w of the 8 sums the splits s = w, w + 8, ... (4 loads in
// flight per lane), then the 8 wave sums are added in wave order through LDS. (One thread per
// output quad summing all S serially left ~1 wave per CU in flight: 0.57 ms for Twitter-US.)
constexpr int kTnRedWaves = 8;
__global__ __launch_bounds__(64 * kTnRedWaves) void gemm_tn_reduce_kernel(
    int M, int N, int S, const float* __restrict__ part, int Mp, int Np,
    const float* __restrict__ scale_dev, float* __restrict__ C, int64_t ldc, int vec) {
  __shared__ f4 red[kTnRedWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nq = (N + 3) / 4;
  for (int m = blockIdx.y; m < M; m += gridDim.y) {  // grid.y <= 65535
  if (m != static_cast<int>(blockIdx.y)) __syncthreads();  // red is reused
  const int qd = static_cast<int>(blockIdx.x) * 64 + lane;  // column quad
  const int qc = qd < nq ? qd : nq - 1;
  const float* src = part + static_cast<int64_t>(m) * Np + 4 * qc;
  const int64_t stride = static_cast<int64_t>(Mp) * Np;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  int s = w;
  for (; s + 3 * kTnRedWaves < S; s += 4 * kTnRedWaves) {
    const f4 v0 = *reinterpret_cast<const f4*>(src + s * stride);
    const f4 v1 = *reinterpret_cast<const f4*>(src + (s + kTnRedWaves) * stride);
    const f4 v2 = *reinterpret_cast<const f4*>(src + (s + 2 * kTnRedWaves) * stride);
    const f4 v3 = *reinterpret_cast<const f4*>(src + (s + 3 * kTnRedWaves) * stride);
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; s < S; s += kTnRedWaves) acc += *reinterpret_cast<const f4*>(src + s * stride);
  red[w][lane] = acc;
  __syncthreads();
  if (w != 0 || qd >= nq) continue;
  f4 t = red[0][lane];
#pragma unroll
  for (int i = 1; i < kTnRedWaves; ++i) t += red[i][lane];
  const float sc = scale_dev ? *scale_dev : 1.0f;
  const int n = 4 * qd;
  float* crow = C + static_cast<int64_t>(m) * ldc;
  const f4 o = {t.x * sc, t.y * sc, t.z * sc, t.w * sc};
  if (vec && n + 3 < N) {
    *reinterpret_cast<f4*>(crow + n) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < N) crow[n + e] = o[e];
  }
  }
}

struct TnPlan {
  int mg, ng, pd, wm = 1, occ = 0;  // tile variant (wm: waves stacked along M; occ: see kernel)
  int mt, nt, S, rows_per_split, Mp, Np;
};

// gcg_gemm_tn tile 1..n: {MG, NG, PD, WM, OCC}, the rows of GCG_TN_TILES
#define GCG_TN_ROW(mg, ng, pd, wm, occ) {mg, ng, pd, wm, occ},
constexpr int kTnTiles[][5] = {GCG_TN_TILES(GCG_TN_ROW)};
#undef GCG_TN_ROW

TnPlan tn_plan(int64_t R, int64_t M, int64_t N, int tile = 0, bool bf16x6 = false) {
  TnPlan p;
  // Default: per-wave 64 x 64*NG tiles (WM = 0), NG = 3 or 2, whichever pads N less (ties: 3,
  // fewer loads per MFMA). The round-2 workgroup tiles (WM = 1: 4 waves side by side, 64 x
  // 256*NG) padded N = 930 to 1024 columns -- 15 % of the MFMAs computed discarded columns.
  // World dW2 840k x 300 x 930: 960 padded columns, 105.8 -> 121.7 TFLOP/s; US dW2 270k x 300
  // x 256 (NG = 2): 87-103 -> 118.
  // NG = 3 runs at 2 waves per SIMD (PD = 3: 246 VGPRs, accumulators included) over ~8192 wave
  // tiles: 129 vs 123 TFLOP/s at 1 wave per SIMD standalone, and inside the training step -- where
  // the weight gradient shares the chip with the SpMM gathers on the main stream -- the shorter,
  // CU-sharing waves overlap better: World step 44.4 -> 43.2 ms. NG = 2 (US dW2, N = 256)
  // measured best at 1 wave per SIMD, PD = 8, ~2048 tiles, in both settings. (The scripts that
  // measured the numbers of this function are no longer in the tree.)
  p.mg = 1, p.pd = 8;
  int64_t slots = 2048;
  {
    const int64_t pad3 = (N + 191) / 192 * 192, pad2 = (N + 127) / 128 * 128;
    p.wm = 0, p.ng = pad3 <= pad2 ? 3 : 2;
    if (p.ng == 3) p.pd = 3, p.occ = 2, slots = 8192;
  }
  // M <= 256 in whole 64-row bands and N <= 512 (the X-head gradient G^T.Xh: 1.4M x 300 x 256
  // as 300 x 256 with the roles below): M/64 waves stacked along M -- A (the narrow operand) is
  // then split over the waves and B read once per row: 85-89 -> 112-115 TFLOP/s. Not for the
  // 300 x 930 dW2 (73-82 vs 106 TFLOP/s: its 8-15 N tiles re-read A).
  const bool stacked = M <= 256 && M % 64 == 0 && N <= 512;
  if (stacked) p.ng = 1, p.pd = 8, p.occ = 0, p.wm = static_cast<int>(M / 64), slots = 2048;
  if (tile > 0) {  // an explicit alternative (caller-checked range)
    const int* t = kTnTiles[tile - 1];
    p.mg = t[0], p.ng = t[1], p.pd = t[2], p.wm = t[3], p.occ = t[4], slots = 2048;
  }
#ifndef GCG_TN6_SLOTS  // wave tiles per launch: 4096 / 8192 / 16384 within noise, 32768 -3 %
#define GCG_TN6_SLOTS 8192  // (variant libraries, tools/gpu/tn_slots.sh, profiles/r06/tn6_slots_ab.txt)
#endif
  if (bf16x6) p.mg = 1, p.ng = 1, p.pd = 0, p.wm = 0, p.occ = 0, slots = GCG_TN6_SLOTS;  // gemm_tn6
  const int tm = 64 * p.mg * std::max(1, p.wm);          // C rows per tile
  const int tn = (p.wm == 1 ? 256 : 64) * p.ng;          // C columns per tile
  p.mt = static_cast<int>((M + tm - 1) / tm);
  p.nt = static_cast<int>((N + tn - 1) / tn);
  // ~`slots` tiles per launch (2048: 2 workgroups per CU of the 256 CUs; per-wave tiles at 1
  // wave per SIMD: 2 rounds of the 1024 SIMDs -- 1 round measured the same speed with 2x longer
  // serial sums), at least 256 rows per split, 16-row aligned
  const int64_t want = std::max<int64_t>(1, slots / std::max(1, p.mt * p.nt));
  const int64_t max_s = std::max<int64_t>(1, R / 256);
  p.S = static_cast<int>(std::min(want, max_s));
  int64_t rps = (R + p.S - 1) / p.S;
  rps = (rps + 15) / 16 * 16;
  p.rows_per_split = static_cast<int>(std::max<int64_t>(rps, 16));
  p.S = static_cast<int>((R + p.rows_per_split - 1) / p.rows_per_split);
  p.Mp = p.mt * tm;
  p.Np = p.nt * tn;
  return p;
}

size_t tn_workspace_bytes(const TnPlan& p) {
  return sizeof(float) * static_cast<size_t>(p.S) * p.Mp * p.Np;
}

gcg_status gemm_tn_impl(const char* fn, int64_t R, int64_t M, int64_t N, const float* A,
                        int64_t lda, const float* B, int64_t ldb, const float* scale_dev,
                        float* C, int64_t ldc, int math, int tile, void* workspace,
                        size_t workspace_bytes, gcg_stream_t stream) {
  gcg_status st;
  if ((st = check_opts(fn, GCG_DENSE_GEMM_TN, math, tile)) != GCG_OK) return st;
  if ((st = check_sizes(fn, "RMN", R, M, N)) != GCG_OK) return st;
  // dwordx4 row reads at columns < round4(M) / round4(N)
  if ((st = check_dense(fn, A, lda, (M + 3) & ~int64_t{3}, true)) != GCG_OK) return st;
  if ((st = check_dense(fn, B, ldb, (N + 3) & ~int64_t{3}, true)) != GCG_OK) return st;
  if ((st = check_dense(fn, C, ldc, N, false)) != GCG_OK) return st;
  if (lda >= (int64_t{1} << 27) || ldb >= (int64_t{1} << 27))  // 4-row buffer ranges < 2 GB
    return fail(GCG_ERR_INVALID_ARG, "%s: leading dimension too large", fn);
  auto s = static_cast<hipStream_t>(stream);
  if (R == 0) {
    for (int64_t m = 0; m < M; ++m)
      GCG_HIP_CHECK(hipMemsetAsync(C + m * ldc, 0, sizeof(float) * N, s));
    return GCG_OK;
  }
  const bool bf = math == GCG_MATH_BF16X6;
  const TnPlan p = tn_plan(R, M, N, tile, bf);
  if ((st = check_workspace(fn, workspace, workspace_bytes, tn_workspace_bytes(p), 16)) != GCG_OK)
    return st;
  float* part = static_cast<float*>(workspace);
  int64_t n_tiles = int64_t{p.mt} * p.nt * p.S;
  if (n_tiles > INT32_MAX) return fail(GCG_ERR_INVALID_ARG, "%s: too many tiles", fn);
  if (p.wm == 0) n_tiles = (n_tiles + 3) / 4;  // 4 wave tiles per workgroup
  const dim3 grid(static_cast<unsigned>(n_tiles));
  constexpr int remap = 1;  // XCD-aware tile order (+1-3 % dW2, +14 % X head)
  if (bf) {
    hipLaunchKernelGGL(gemm_tn6_partial_kernel, grid, dim3(256), 0, s, int(R), int(M), int(N), A,
                       lda, B, ldb, p.rows_per_split, part, p.Mp, p.Np, p.mt, p.nt);
  } else
#define GCG_TN_CASE(MG_, NG_, PD_, WM_, OCC_)                                                \
  if (p.mg == MG_ && p.ng == NG_ && p.pd == PD_ && p.wm == WM_ && p.occ == OCC_) {           \
    hipLaunchKernelGGL((gemm_tn_partial_kernel<MG_, NG_, PD_, WM_, OCC_>), grid,             \
                       dim3(WM_ <= 1 ? 256 : 64 * WM_), 0, s, int(R), int(M), int(N), A, lda, \
                       B, ldb, p.rows_per_split, part, p.Mp, p.Np, p.mt, p.nt, remap);       \
  } else
  GCG_TN_TILES(GCG_TN_CASE)
  GCG_TN_STACKED(GCG_TN_CASE)
  { return fail(GCG_ERR_INVALID_ARG, "%s: no TN tile MG=%d NG=%d PD=%d WM=%d OCC=%d", fn, p.mg,
                p.ng, p.pd, p.wm, p.occ); }
#undef GCG_TN_CASE
  GCG_HIP_CHECK(hipGetLastError());
  const int vec = (ldc % 4 == 0 && aligned(C, 16)) ? 1 : 0;
  const dim3 rgrid(static_cast<unsigned>(((N + 3) / 4 + 63) / 64),
                   static_cast<unsigned>(std::min<int64_t>(M, 65535)));
  hipLaunchKernelGGL(gemm_tn_reduce_kernel, rgrid, dim3(64 * kTnRedWaves), 0, s, int(M), int(N),
                     p.S, part, p.Mp, p.Np, scale_dev, C, ldc, vec);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // namespace

extern "C" {

gcg_status gcg_gemm_tn_workspace_bytes(int64_t R, int64_t M, int64_t N, int32_t math,
                                       int32_t tile, size_t* bytes) {
  const char* fn = "gcg_gemm_tn_workspace_bytes";
  gcg_status s;
  if ((s = check_opts(fn, GCG_DENSE_GEMM_TN, math, tile)) != GCG_OK) return s;
  if (R < 0 || M <= 0 || N <= 0 || R > INT32_MAX || M > INT32_MAX || N > INT32_MAX ||
      bytes == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes", fn);
  if (R == 0) { *bytes = 0; return GCG_OK; }
  *bytes = tn_workspace_bytes(tn_plan(R, M, N, tile, math == GCG_MATH_BF16X6));
  return GCG_OK;
}

gcg_status gcg_gemm_tn_f32_workspace_bytes(int64_t R, int64_t M, int64_t N, size_t* bytes) {
  return gcg_gemm_tn_workspace_bytes(R, M, N, GCG_MATH_F32, 0, bytes);
}

gcg_status gcg_gemm_tn(int64_t R, int64_t M, int64_t N, const float* A, int64_t lda,
                       const float* B, int64_t ldb, const float* scale_dev, float* C, int64_t ldc,
                       int32_t math, int32_t tile, void* workspace, size_t workspace_bytes,
                       gcg_stream_t stream) {
  return gemm_tn_impl("gcg_gemm_tn", R, M, N, A, lda, B, ldb, scale_dev, C, ldc, math, tile,
                      workspace, workspace_bytes, stream);
}

gcg_status gcg_gemm_tn_f32(int64_t R, int64_t M, int64_t N, const float* A, int64_t lda,
                           const float* B, int64_t ldb, const float* scale_dev, float* C,
                           int64_t ldc, void* workspace, size_t workspace_bytes,
                           gcg_stream_t stream) {
  return gemm_tn_impl("gcg_gemm_tn_f32", R, M, N, A, lda, B, ldb, scale_dev, C, ldc,
                      GCG_MATH_F32, 0, workspace, workspace_bytes, stream);
}

}  // extern "C"
