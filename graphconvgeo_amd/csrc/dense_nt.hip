// dense_nt.hip -- C = act(A . Bt^T + bias) with both operands k-contiguous (gcg_gemm_nt): the
// projection h.W with the weight stored transposed and its input gradient dP = G.W2^T, in exact
// f32 (gemm_nt_kernel) or bf16x6 over the weight's planes, pre-split once per call by
// split3_rows_kernel (gemm_nt3r_kernel, gemm_nt3_kernel).
#include "dense_shared.h"

using namespace gcg;

namespace {

// ---------------------------------------------------------------------------------------
// gemm_nt_kernel<RT, G, WR, WC, S, PF, KC>: C = act(A . Bt^T + bias), both operands
// k-contiguous (A: M x K row-major, Bt: N x K row-major -- the weight stored transposed, as
// graphconvgeo_amd.dense keeps it), staged into LDS by the async LDS-DMA
// (global_load_lds_dwordx4) through an S-deep ring of KC-deep k chunks (KC = 32 or 16).
//
//   * LDS image per stage: [BM + BN rows][KC floats], SL = KC/4 slots of 16 B per row, slot s
//     of image row r stored at slot s ^ key(r): key = r & 7 for 8-slot rows, a permutation of
//     (r >> 2) & 3 for 4-slot rows -- chosen so that each 16-lane group of a fragment read
//     (16 consecutive image rows, slots q) hits 16 distinct bank quads: conflict-free
//     ds_read_b128. The DMA writes LDS linearly (wave base + 16 B per lane), so the swizzle is
//     applied to the per-lane GLOBAL source address (the involution s' <-> s ^ key(r)).
//   * B image row order: within each 64-column group, row 16e + j holds column 4j + e, so
//     the fragment of the strided MFMA tile e (columns 4j + e, j = 0..15) is 16 consecutive
//     image rows, and a lane ends up with 4 ADJACENT output columns (acc[t][g][0..3]) ->
//     dwordx4 stores; the register layout of gemm_kernel (gemm_epilogue.inc).
//   * A fragment: one ds_read_b128 per 16-row tile per 16-deep step gives the lane its 4
//     k-values of the 4 v_mfma_f32_16x16x4_f32 substeps (k = k0 + 4q + e, permuted
//     identically for A and B); B likewise, one ds_read_b128 per 16-column tile.
//   * Sync: ONE raw s_barrier per chunk, after a counted `s_waitcnt vmcnt` that retires the
//     chunk's own DMA (S = 2: vmcnt(0); S = 3: the next stage stays in flight). The barrier
//     also fences the buffer the next DMA overwrites: every wave finished reading it (its
//     MFMAs consumed the reads) before arriving. All LDS is one __shared__ array (a second
//     object makes hipcc drain the DMA queue before every ds_read).
//   * K tail: source addresses are clamped into the row; in the step that reaches past K the
//     fragment elements at k >= K are zeroed in registers (both operands, so garbage in the
//     operands' padding never meets a finite factor). Until round 2 the last chunk's k >= K
//     elements were zeroed in LDS by a 24-iteration loop per thread plus an extra barrier, once
//     per tile (~10 % of a K = 300 tile). Rows past M / columns past N read clamped rows and
//     are never stored.
//   * XCD-aware order (MI355X_MICROARCH.md: workgroup b runs on XCD b % 8): workgroup b takes
//     logical tile remap(b), each XCD walking one contiguous range of tiles in row-block-major
//     order, so the N / BN column tiles of a row block share one XCD's L2 copy of its A rows.
// Numerics: exact f32 products, f32 accumulation in k order k0 + 4q + e inside each 16-deep
// step (as gemm_kernel): equal to BLAS sgemm within f32 rounding.
// ---------------------------------------------------------------------------------------
template <int RT, int G, int WR, int WC, int S, int KC>
struct NtCfg {
  static constexpr int NW = WR * WC;
  static constexpr int NT = 64 * NW;
  static constexpr int BM = 16 * RT * WR;
  static constexpr int BN = 64 * G * WC;
  static constexpr int SL = KC / 4;               // 16-B slots per image row
  static constexpr int RPI = 64 / SL;             // image rows per DMA instruction (1 KB)
  static constexpr int ROWS = BM + BN;            // image rows per stage
  static constexpr int STAGE = ROWS * KC;         // floats per stage
  static constexpr int NGLDS = ROWS / RPI;        // DMA wave-instructions per stage
  static constexpr int PER_WAVE = NGLDS / NW;     // (exact when S >= 3)
  static constexpr int FLOATS = S * STAGE;
  static constexpr int LDS_BYTES = FLOATS * 4;
  static constexpr int OCC_LDS = (160 * 1024) / LDS_BYTES;  // workgroups per CU the LDS allows
  static constexpr int OCC = OCC_LDS < 1 ? 1 : (OCC_LDS > 4 ? 4 : OCC_LDS);
  static_assert(KC == 16 || KC == 32, "4- or 8-slot image rows");
  static_assert(ROWS % RPI == 0, "whole DMA instructions per stage");
  static_assert(S == 2 || NGLDS % NW == 0, "S >= 3 needs the same DMA count on every wave");
  static_assert(S >= 2 && S <= 6, "2..6 stages");
};

template <int RT, int G, int WR, int WC, int S, int PF, int KC, int MX = 0>
__global__ __launch_bounds__(64 * WR * WC, (NtCfg<RT, G, WR, WC, S, KC>::OCC)) void
gemm_nt_kernel(int M, int N, int K, const float* __restrict__ A, int64_t lda,
               const float* __restrict__ Bt, int64_t ldb, const float* __restrict__ bias, int act,
               float* __restrict__ Cout, int64_t ldc, int n_col_tiles) {
  constexpr bool TP = (MX & 2) != 0;  // the packed K tail (mfma6; MX & 1: bf16x6)
  using Cfg = NtCfg<RT, G, WR, WC, S, KC>;
  constexpr int EPI = 0;  // plain epilogue only (gemm_epilogue.inc names the EPI = 1 operands)
  const int32_t* labels = nullptr;
  float scale = 0.f;
  const float* scale_dev = nullptr;
  float* loss_rows = nullptr;
  float* correct_rows = nullptr;
  const float* row_w = nullptr;
  (void)labels; (void)scale; (void)scale_dev; (void)loss_rows; (void)correct_rows; (void)row_w;
  constexpr int NT = Cfg::NT, BM = Cfg::BM, BN = Cfg::BN, STAGE = Cfg::STAGE;
  constexpr int SL = Cfg::SL, RPI = Cfg::RPI;
  __shared__ __attribute__((aligned(16))) float smem[Cfg::FLOATS];
  float (*red)[WC][BM] = nullptr;  // (EPI = 1 only)
  (void)red;

  // XCD-aware bijective remap of the 1-D grid (cdna_hip_programming.md T1).
  const int nwg = static_cast<int>(gridDim.x);
  const int b = static_cast<int>(blockIdx.x);
  const int xcd = b % 8, qq = nwg / 8, rr = nwg % 8;
  const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + b / 8;
  const int row_tile = tile / n_col_tiles, col_tile = tile % n_col_tiles;
  const int64_t row0 = static_cast<int64_t>(row_tile) * BM;
  const int col0 = col_tile * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int j = lane & 15, q = lane >> 4;
  const int colw = col0 + wc * G * 64;  // this wave's first output column (epilogue)

  // ---- DMA source rows: this wave's instructions i = wave + NW * u cover image rows
  // RPI*i .. RPI*i + RPI-1; lane -> row RPI*i + lane / SL, LDS slot lane % SL, global slot
  // (lane % SL) ^ key(row).
  constexpr int NU = (Cfg::NGLDS + Cfg::NW - 1) / Cfg::NW;  // instructions per wave (max)
  const float* src[NU];
  int kofs[NU];  // 4 * global slot
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int i = wave + Cfg::NW * u;
    const int r = RPI * i + lane / SL;
    const int sl = (lane % SL) ^ nt_key<SL>(r);
    kofs[u] = 4 * sl;
    if (r < BM) {
      const int64_t gr = row0 + r;
      src[u] = A + (gr < M ? gr : static_cast<int64_t>(M) - 1) * lda;
    } else {
      const int rb = r - BM;                       // B image row: group, tile e, lane j
      const int n = col0 + (rb & ~63) + 4 * (rb & 15) + ((rb >> 4) & 3);
      src[u] = Bt + static_cast<int64_t>(n < N ? n : N - 1) * ldb;
    }
  }
  const int kmax4 = (K - 1) & ~3;  // last 16-B segment holding a valid k
  auto issue = [&](int chunk) {
    float* stage = smem + (chunk % S) * STAGE;
    const int kc0 = chunk * KC;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int i = wave + Cfg::NW * u;
      if (NU * Cfg::NW != Cfg::NGLDS && i >= Cfg::NGLDS) break;  // wave-uniform
      int k = kc0 + kofs[u];
      k = k < kmax4 ? k : kmax4;
      glds16(src[u] + k, stage + i * 256);  // instruction i fills 1 KB of the image
    }
  };
  auto lds_barrier = [&]() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  f4 acc[RT][G][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][g][e] = f4{0.f, 0.f, 0.f, 0.f};

  // bias of this lane's output columns, loaded now so its latency hides behind the K loop
  f4 bv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bv[g] = f4{0.f, 0.f, 0.f, 0.f};
    const int c = colw + 64 * g + 4 * j;
    if (bias != nullptr) {
      if (c + 3 < N) {
        bv[g] = f4{bias[c], bias[c + 1], bias[c + 2], bias[c + 3]};
      } else {
        if (c < N) bv[g].x = bias[c];
        if (c + 1 < N) bv[g].y = bias[c + 1];
        if (c + 2 < N) bv[g].z = bias[c + 2];
      }
    }
  }

  const int n_chunks = (K + KC - 1) / KC;
  const int arow0 = wr * 16 * RT + j;       // A image row of tile 0 (lane j)
  const int brow0 = BM + wc * G * 64 + j;   // B image row of group 0, tile e = 0 (lane j)
  auto frag = [&](const float* stage, int row, int slot) -> f4 {
    return *reinterpret_cast<const f4*>(stage + row * KC + 4 * (slot ^ nt_key<SL>(row)));
  };
  auto mfma_step = [&](const f4 (&af)[RT], const f4 (&bf)[G][4]) {
#pragma unroll
    for (int ss = 0; ss < 4; ++ss)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][g][e] = mfma4(af[t][ss], bf[g][e][ss], acc[t][g][e]);
  };
  // zero the elements of a step's fragments at k >= K: lane (j, q) holds k = kb + 4q + e
  auto mask_step = [&](f4 (&af)[RT], f4 (&bf)[G][4], int kb) {
    const int lim = K - kb - 4 * q;  // elements e < lim are inside K
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = e < lim;
#pragma unroll
      for (int t = 0; t < RT; ++t) af[t][e] = in ? af[t][e] : 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) bf[g][e2][e] = in ? bf[g][e2][e] : 0.f;
    }
  };
  auto read_step = [&](const float* stage, int h, f4 (&af)[RT], f4 (&bf)[G][4]) {
#pragma unroll
    for (int t = 0; t < RT; ++t) af[t] = frag(stage, arow0 + 16 * t, 4 * h + q);
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) bf[g][e] = frag(stage, brow0 + 64 * g + 16 * e, 4 * h + q);
  };

#pragma unroll
  for (int c = 0; c < S - 1; ++c)
    if (c < n_chunks) issue(c);
  // one chunk; tp: the packed K tail (mfma6), only the peeled last chunk of a TP kernel (MX & 2,
  // chosen by the host when that chunk holds <= 16 live k)
  auto chunk_body = [&](int c, auto tp) {
    // retire this chunk's DMA (leave the later stages in flight), then one barrier
    if constexpr (S == 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (c + S - 2 < n_chunks) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"((S - 2) * Cfg::PER_WAVE) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    lds_barrier();
    const float* stage = smem + (c % S) * STAGE;
    const int kc0 = c * KC;
    if (c + S - 1 < n_chunks) issue(c + S - 1);
    // K tail: a step reaching past K has its k >= K fragment elements zeroed in registers
    // (wave-uniform branch, last chunk only); the LDS there holds clamped re-reads / padding
    if constexpr (KC == 16) {
      f4 af[RT], bf[G][4];
      read_step(stage, 0, af, bf);
      if (kc0 + 16 > K) mask_step(af, bf, kc0);
      mfma_step(af, bf);
    } else if constexpr ((MX & 1) != 0) {
      // bf16x6: the chunk's two 16-deep fragment sets are one 32-deep bf16 MFMA operand (lane
      // (j, q) holds k = kc0 + 4q + {0..3} and kc0 + 16 + 4q + {0..3}, the same for A and B)
      f4 af0[RT], bf0[G][4], af1[RT], bf1[G][4];
      read_step(stage, 0, af0, bf0);
      read_step(stage, 1, af1, bf1);
      if (kc0 + 16 > K) mask_step(af0, bf0, kc0);
      if (kc0 + 32 > K) mask_step(af1, bf1, kc0 + 16);
      bf8 ap[RT][3];
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const f8 x = {af0[t][0], af0[t][1], af0[t][2], af0[t][3],
                      af1[t][0], af1[t][1], af1[t][2], af1[t][3]};
        split3(x, ap[t][0], ap[t][1], ap[t][2]);
      }
      auto mm = [&](auto tp) {  // tp: the packed K tail (mfma6)
        constexpr bool TPC = decltype(tp)::value;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f8 y = {bf0[g][e][0], bf0[g][e][1], bf0[g][e][2], bf0[g][e][3],
                          bf1[g][e][0], bf1[g][e][1], bf1[g][e][2], bf1[g][e][3]};
            bf8 b0, b1, b2;
            split3(y, b0, b1, b2);
#pragma unroll
            for (int t = 0; t < RT; ++t)
              acc[t][g][e] = mfma6<TPC>(ap[t], b0, b1, b2, acc[t][g][e]);
          }
      };
      if constexpr (decltype(tp)::value) {
#pragma unroll
        for (int t = 0; t < RT; ++t) pack_tail_a(ap[t]);
      }
      mm(tp);
    } else if constexpr (PF) {
      // both 16-deep steps' fragments first: the second step's LDS reads are in flight
      // during the first step's MFMAs (counted lgkmcnt waits)
      f4 af0[RT], bf0[G][4], af1[RT], bf1[G][4];
      read_step(stage, 0, af0, bf0);
      read_step(stage, 1, af1, bf1);
      if (kc0 + 16 > K) mask_step(af0, bf0, kc0);
      mfma_step(af0, bf0);
      if (kc0 + 16 < K) {
        if (kc0 + 32 > K) mask_step(af1, bf1, kc0 + 16);
        mfma_step(af1, bf1);
      }
    } else {
      f4 af[RT], bf[G][4];
      read_step(stage, 0, af, bf);
      if (kc0 + 16 > K) mask_step(af, bf, kc0);
      mfma_step(af, bf);
      if (kc0 + 16 < K) {
        read_step(stage, 1, af, bf);
        if (kc0 + 32 > K) mask_step(af, bf, kc0 + 16);
        mfma_step(af, bf);
      }
    }
  };
  const int n_full = TP ? n_chunks - 1 : n_chunks;
  for (int c = 0; c < n_full; ++c) chunk_body(c, std::false_type{});
  if constexpr (TP) chunk_body(n_full, std::true_type{});
  if constexpr (MX != 0) {  // bf16x6: f32 semantics for Inf / huge operands (f32_tile)
    if (tile_nonfinite<RT, G>(acc, N, colw, j))
      f32_tile<RT, G>(acc, M, N, K, A, lda, row0 + wr * 16 * RT, Bt, ldb, 1, colw, j, q);
  }
#define GCG_EPI_BV_READY
#include "gemm_epilogue.inc"
#undef GCG_EPI_BV_READY
}

// ---------------------------------------------------------------------------------------
// bf16x6 NT GEMM with the weight side pre-split (round 4): C = act(A . Bt^T + bias) with
// Bt's three bf16 planes written once per call by split3_rows_kernel into a workspace laid out
// [N][Kc][3][32] bf16 (Kc = ceil(K / 32) chunks, zeros past K), each 32-element plane chunk in
// the k order of the MFMA operand (position 8q + w holds k = 4q + w for w < 4, 16 + 4q + w - 4
// after), so a lane's B fragment of one plane is ONE 16-B LDS read and no B conversion is left
// in the loop. A stays f32 (staged exactly as gemm_nt_kernel's KC = 32 image) and is split in
// registers. LDS stage: [BM rows][8 slots] f32, then per plane [BN rows][4 slots] (64-B rows,
// swizzle nt_key<4>, the conflict-free 4-slot layout of the KC = 16 kernel), all through the
// LDS-DMA ring. The B image keeps gemm_nt_kernel's strided row order (row 16e + j of a 64-column
// group holds column 4j + e), so the accumulator layout and the epilogue are the same.
// ---------------------------------------------------------------------------------------
// (element (n, k) at Bt + n * ldb + k * kstride: kstride = 1 for the NT weight Bt, ldw for the
// fused layer's W read column-wise; planes for n in [N, n_out) are zero)
__global__ __launch_bounds__(256) void split3_rows_kernel(int N, int K, int Kc,
                                                          const float* __restrict__ Bt, int64_t ldb,
                                                          unsigned* __restrict__ out,
                                                          int64_t kstride = 1, int n_out = 0) {
  const int n_rows = n_out > N ? n_out : N;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;  // (n, chunk, q)
  if (i >= static_cast<int64_t>(n_rows) * Kc * 4) return;
  const int q = static_cast<int>(i & 3);
  const int64_t nc = i >> 2;
  const int n = static_cast<int>(nc / Kc), c = static_cast<int>(nc % Kc);
  const float* row = Bt + static_cast<int64_t>(n < N ? n : 0) * ldb;
  f8 x;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const int k = 32 * c + (w < 4 ? 4 * q + w : 16 + 4 * q + (w - 4));
    x[w] = (k < K && n < N) ? row[static_cast<int64_t>(k) * kstride] : 0.f;
  }
  bf8 h[3];
  split3(x, h[0], h[1], h[2]);
  if (n_out > 0) {
    // fused layer's layout [c][plane][n / 64][n % 4][(n % 64) / 4][q]: the 16 lanes j of one
    // (column group, slot e, plane) read 16 x 64 contiguous bytes
    const int gq = n >> 6, e = n & 3, jj = (n & 63) >> 2, ng = (n_rows + 63) >> 6;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const int64_t pos = ((((static_cast<int64_t>(c) * 3 + p) * ng + gq) * 4 + e) * 16 + jj) * 16 + 4 * q;
      *reinterpret_cast<u4v*>(out + pos) = __builtin_bit_cast(u4v, h[p]);
    }
    return;
  }
  // [n][c][plane][32 bf16]: plane p's lane-q fragment is the 16 B at (nc * 3 + p) * 64 + 16 q
#pragma unroll
  for (int p = 0; p < 3; ++p)
    *reinterpret_cast<u4v*>(out + (nc * 3 + p) * 16 + 4 * q) = __builtin_bit_cast(u4v, h[p]);
}

template <int RT, int G, int WR, int WC, int S>
struct Nt3Cfg {
  static constexpr int NW = WR * WC;
  static constexpr int BM = 16 * RT * WR;
  static constexpr int BN = 64 * G * WC;
  static constexpr int A_FLOATS = BM * 32;          // [BM][8 slots of 16 B]
  static constexpr int P_FLOATS = BN * 16;          // one plane: [BN][4 slots of 16 B]
  static constexpr int STAGE = A_FLOATS + 3 * P_FLOATS;
  static constexpr int NGA = BM / 8;                // DMA wave-instructions (1 KB each)
  static constexpr int NGP = BN / 16;               // ... per plane
  static constexpr int NG = NGA + 3 * NGP;
  static constexpr int NU = (NG + NW - 1) / NW;
  static constexpr int PER_WAVE = NG / NW;          // (exact when S >= 3)
  static constexpr int FLOATS = S * STAGE;
  static constexpr int OCC_LDS = (160 * 1024) / (FLOATS * 4);
  static constexpr int OCC = OCC_LDS < 1 ? 1 : (OCC_LDS > 4 ? 4 : OCC_LDS);
  static_assert(S == 2 || NG % NW == 0, "S >= 3 needs the same DMA count on every wave");
  static_assert(S >= 2 && S <= 4, "2..4 stages");
};

template <int RT, int G, int WR, int WC, int S, bool TP = false>  // TP: the packed K tail
__global__ __launch_bounds__(64 * WR * WC, (Nt3Cfg<RT, G, WR, WC, S>::OCC)) void
gemm_nt3_kernel(int M, int N, int K, const float* __restrict__ A, int64_t lda,
                const unsigned* __restrict__ Bs, const float* __restrict__ Bt, int64_t ldbt, const float* __restrict__ bias, int act,
                float* __restrict__ Cout, int64_t ldc, int n_col_tiles) {
  using Cfg = Nt3Cfg<RT, G, WR, WC, S>;
  constexpr int EPI = 0;
  const int32_t* labels = nullptr;
  float scale = 0.f;
  const float* scale_dev = nullptr;
  float* loss_rows = nullptr;
  float* correct_rows = nullptr;
  const float* row_w = nullptr;
  (void)labels; (void)scale; (void)scale_dev; (void)loss_rows; (void)correct_rows; (void)row_w;
  constexpr int BM = Cfg::BM, BN = Cfg::BN, STAGE = Cfg::STAGE, NW = Cfg::NW, NU = Cfg::NU;
  __shared__ __attribute__((aligned(16))) float smem[Cfg::FLOATS];
  float (*red)[WC][BM] = nullptr;
  (void)red;

  const int nwg = static_cast<int>(gridDim.x);
  const int b = static_cast<int>(blockIdx.x);
  const int xcd = b % 8, qq = nwg / 8, rr = nwg % 8;
  const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + b / 8;
  const int row_tile = tile / n_col_tiles, col_tile = tile % n_col_tiles;
  const int64_t row0 = static_cast<int64_t>(row_tile) * BM;
  const int col0 = col_tile * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int j = lane & 15, q = lane >> 4;
  const int colw = col0 + wc * G * 64;
  const int Kc = (K + 31) / 32;

  // DMA sources, through buffer descriptors re-based every chunk (scalar work only; the lane
  // offsets are constants): instruction i < NGA fills A image rows 8i .. 8i+7 (8 slots, key
  // r & 7), the others plane p = (i - NGA) / NGP, plane rows 16 ib .. 16 ib + 15 (4 slots, key
  // nt_key<4>). A's range ends at the tile's last row's round4(K): the K-tail chunk's segments
  // past it read 0 (rows inside read their neighbours' floats, zeroed in registers below).
  static_assert(Cfg::NGA % NW == 0, "A and B DMA instructions split at a whole u");
  constexpr int UA = Cfg::NGA / NW;
  int voff[NU];
  const int rows_here = static_cast<int>(M - row0 < BM ? M - row0 : BM);
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int i = wave + NW * u;
    if (u < UA) {
      const int r = 8 * i + lane / 8;
      const int rl = r < rows_here ? r : rows_here - 1;
      voff[u] = (rl * static_cast<int>(lda) + 4 * ((lane % 8) ^ (r & 7))) * 4;
    } else {
      const int ib = i - Cfg::NGA;
      const int p = ib / Cfg::NGP;
      const int rb = (ib % Cfg::NGP) * 16 + lane / 4;
      const int sl = (lane % 4) ^ nt_key<4>(rb);
      int n = col0 + (rb & ~63) + 4 * (rb & 15) + ((rb >> 4) & 3);
      n = n < N ? n : N - 1;
      voff[u] = ((n * Kc) * 3 + p) * 64 + 16 * sl;
    }
  }
  const int a_bytes = ((rows_here - 1) * static_cast<int>(lda) + ((K + 3) & ~3)) * 4;
  const int b_bytes = N * Kc * 192;
  auto issue = [&](int chunk) {
    float* stage = smem + (chunk % S) * STAGE;
    const auto ra = brsrc(A + row0 * lda + 32 * chunk, a_bytes - 128 * chunk);
    const auto rbs = brsrc(Bs + 48 * chunk, b_bytes - 192 * chunk);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int i = wave + NW * u;
      if (NU * NW != Cfg::NG && i >= Cfg::NG) break;  // wave-uniform
      blds16(u < UA ? ra : rbs, stage + i * 256, voff[u]);
    }
  };
  auto lds_barrier = [&]() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  f4 acc[RT][G][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][g][e] = f4{0.f, 0.f, 0.f, 0.f};

  f4 bv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bv[g] = f4{0.f, 0.f, 0.f, 0.f};
    const int c = colw + 64 * g + 4 * j;
    if (bias != nullptr) {
      if (c + 3 < N) {
        bv[g] = f4{bias[c], bias[c + 1], bias[c + 2], bias[c + 3]};
      } else {
        if (c < N) bv[g].x = bias[c];
        if (c + 1 < N) bv[g].y = bias[c + 1];
        if (c + 2 < N) bv[g].z = bias[c + 2];
      }
    }
  }

  const int arow0 = wr * 16 * RT + j;
  const int brow0 = wc * G * 64 + j;
  for (int c = 0; c < S - 1; ++c)
    if (c < Kc) issue(c);
  // one chunk; tp: the packed K tail (mfma6), only the peeled last chunk of a TP kernel
  auto chunk_body = [&](int c, auto tp) {
    if constexpr (S == 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (c + S - 2 < Kc) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"((S - 2) * Cfg::PER_WAVE) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    lds_barrier();
    const float* stage = smem + (c % S) * STAGE;
    const int kc0 = c * 32;
    if (c + S - 1 < Kc) issue(c + S - 1);
    // A fragments (two 16-B reads per tile), masked past K, split into planes
    bf8 ap[RT][3];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int r = arow0 + 16 * t;
      const f4 lo = *reinterpret_cast<const f4*>(stage + r * 32 + 4 * (q ^ (r & 7)));
      const f4 hi = *reinterpret_cast<const f4*>(stage + r * 32 + 4 * ((4 + q) ^ (r & 7)));
      f8 x = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (kc0 + 32 > K) {
        const int lim = K - kc0 - 4 * q;  // lo element w: k = kc0 + 4q + w; hi: + 16
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          x[w] = w < lim ? x[w] : 0.f;
          x[4 + w] = 16 + w < lim ? x[4 + w] : 0.f;
        }
      }
      split3(x, ap[t][0], ap[t][1], ap[t][2]);
    }
    const float* bsec = stage + Cfg::A_FLOATS;
    auto mm = [&](auto tp) {  // tp: the packed K tail (mfma6)
      constexpr bool TPC = decltype(tp)::value;
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int rb = brow0 + 64 * g + 16 * e;
          const int so = rb * 16 + 4 * (q ^ nt_key<4>(rb));
          const bf8 b0 = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + so));
          const bf8 b1 = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + Cfg::P_FLOATS + so));
          const bf8 b2 = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + 2 * Cfg::P_FLOATS + so));
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[t][g][e] = mfma6<TPC>(ap[t], b0, b1, b2, acc[t][g][e]);
        }
    };
    if constexpr (decltype(tp)::value) {
#pragma unroll
      for (int t = 0; t < RT; ++t) pack_tail_a(ap[t]);
    }
    mm(tp);
  };
  const int n_full = TP ? Kc - 1 : Kc;
  for (int c = 0; c < n_full; ++c) chunk_body(c, std::false_type{});
  if constexpr (TP) chunk_body(n_full, std::true_type{});
  if (tile_nonfinite<RT, G>(acc, N, colw, j))  // f32 semantics for Inf / huge operands
    f32_tile<RT, G>(acc, M, N, K, A, lda, row0 + wr * 16 * RT, Bt, ldbt, 1, colw, j, q);
#define GCG_EPI_BV_READY
#include "gemm_epilogue.inc"
#undef GCG_EPI_BV_READY
}

// gemm_nt3r_kernel<RT, G, WR, WC>: gemm_nt3_kernel with A loaded straight into registers (each
// wave owns its 16 RT rows, so an LDS stage of A is shared by nobody when WC = 1): two
// dwordx4 buffer loads per row tile and chunk through a descriptor re-based every chunk, one
// chunk ahead (two register sets, the chunk loop unrolled by two), while only the weight's
// planes go through the LDS-DMA ring (12 KB per 64 columns and chunk, two stages), so more
// workgroups fit per CU.
template <int RT, int G, int WR, int WC>
struct Nt3rCfg {
  static constexpr int NW = WR * WC;
  static constexpr int BM = 16 * RT * WR;
  static constexpr int BN = 64 * G * WC;
  static constexpr int P_FLOATS = BN * 16;
  static constexpr int STAGE = 3 * P_FLOATS;
  static constexpr int NGP = BN / 16;
  static constexpr int NG = 3 * NGP;
  static constexpr int NU = (NG + NW - 1) / NW;
  static constexpr int FLOATS = 2 * STAGE;
  static constexpr int OCC_LDS = (160 * 1024) / (FLOATS * 4);
  static constexpr int OCC_REG = RT * G >= 4 ? 2 : 4;  // 4 x 4 accumulator tiles: <= 256 VGPRs
  static constexpr int OCC = OCC_LDS < 1 ? 1 : (OCC_LDS > OCC_REG ? OCC_REG : OCC_LDS);
};

template <int RT, int G, int WR, int WC, int V = 0>
__global__ __launch_bounds__(64 * WR * WC, (Nt3rCfg<RT, G, WR, WC>::OCC)) void
gemm_nt3r_kernel(int M, int N, int K, const float* __restrict__ A, int64_t lda,
                 const unsigned* __restrict__ Bs, const float* __restrict__ Bt, int64_t ldbt, const float* __restrict__ bias, int act,
                 float* __restrict__ Cout, int64_t ldc, int n_col_tiles) {
  using Cfg = Nt3rCfg<RT, G, WR, WC>;
  constexpr bool PL = (V & 1) != 0;
  constexpr bool TP = (V & 2) != 0;
  constexpr int EPI = 0;
  const int32_t* labels = nullptr;
  float scale = 0.f;
  const float* scale_dev = nullptr;
  float* loss_rows = nullptr;
  float* correct_rows = nullptr;
  const float* row_w = nullptr;
  (void)labels; (void)scale; (void)scale_dev; (void)loss_rows; (void)correct_rows; (void)row_w;
  constexpr int BM = Cfg::BM, BN = Cfg::BN, STAGE = Cfg::STAGE, NW = Cfg::NW, NU = Cfg::NU;
  __shared__ __attribute__((aligned(16))) float smem[Cfg::FLOATS];
  float (*red)[WC][BM] = nullptr;
  (void)red;

  const int nwg = static_cast<int>(gridDim.x);
  const int b = static_cast<int>(blockIdx.x);
  const int xcd = b % 8, qq = nwg / 8, rr = nwg % 8;
  const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + b / 8;
  const int row_tile = tile / n_col_tiles, col_tile = tile % n_col_tiles;
  const int64_t row0 = static_cast<int64_t>(row_tile) * BM;
  const int col0 = col_tile * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int j = lane & 15, q = lane >> 4;
  const int colw = col0 + wc * G * 64;
  const int Kc = (K + 31) / 32;
  const int rows_here = static_cast<int>(M - row0 < BM ? M - row0 : BM);

  // weight planes: LDS-DMA instruction i fills plane p = i / NGP, rows 16 (i % NGP) .. + 15
  int voff[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int i = wave + NW * u;
    const int p = i / Cfg::NGP;
    const int rb = (i % Cfg::NGP) * 16 + lane / 4;
    const int sl = (lane % 4) ^ nt_key<4>(rb);
    int n = col0 + (rb & ~63) + 4 * (rb & 15) + ((rb >> 4) & 3);
    n = n < N ? n : N - 1;
    voff[u] = ((n * Kc) * 3 + p) * 64 + 16 * sl;
  }
  // A: lane (j, q) of row tile t reads row wr*16RT + 16t + j, k = 4q..4q+3 and 16+4q..16+4q+3
  int aoff[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    int r = wr * 16 * RT + 16 * t + j;
    r = r < rows_here ? r : rows_here - 1;
    aoff[t] = (r * static_cast<int>(lda) + 4 * q) * 4;
  }
  const int a_bytes = ((rows_here - 1) * static_cast<int>(lda) + ((K + 3) & ~3)) * 4;
  const int b_bytes = N * Kc * 192;
  auto issue_b = [&](int chunk) {
    float* stage = smem + (chunk & 1) * STAGE;
    const auto rbs = brsrc(Bs + 48 * chunk, b_bytes - 192 * chunk);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int i = wave + NW * u;
      if (NU * NW != Cfg::NG && i >= Cfg::NG) break;  // wave-uniform
      blds16(rbs, stage + i * 256, voff[u]);
    }
  };
  // (A keeps the default policy: the N / BN column tiles of a row block re-read its rows from
  // L2 -- non-temporal A loads measured 3.5-17 % slower, profiles/r05/nontemporal_streams.jsonl)
  auto load_a = [&](int chunk, f4 (&lo)[RT], f4 (&hi)[RT]) {
    const auto ra = brsrc(A + row0 * lda + 32 * chunk, a_bytes - 128 * chunk);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      lo[t] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, aoff[t], 0, 0));
      hi[t] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, aoff[t] + 64, 0, 0));
    }
  };

  f4 acc[RT][G][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][g][e] = f4{0.f, 0.f, 0.f, 0.f};

  f4 bv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bv[g] = f4{0.f, 0.f, 0.f, 0.f};
    const int c = colw + 64 * g + 4 * j;
    if (bias != nullptr) {
      if (c + 3 < N) {
        bv[g] = f4{bias[c], bias[c + 1], bias[c + 2], bias[c + 3]};
      } else {
        if (c < N) bv[g].x = bias[c];
        if (c + 1 < N) bv[g].y = bias[c + 1];
        if (c + 2 < N) bv[g].z = bias[c + 2];
      }
    }
  }

  const int brow0 = wc * G * 64 + j;
  // tp: the packed K tail (mfma6) -- only the peeled last chunk of a TP kernel
  auto step = [&](int c, f4 (&lo)[RT], f4 (&hi)[RT], f4 (&nlo)[RT], f4 (&nhi)[RT], auto tp) {
    constexpr bool TPC = decltype(tp)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // chunk c: its A registers and B planes
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (c + 1 < Kc) {
      issue_b(c + 1);
      load_a(c + 1, nlo, nhi);
    }
    const int kc0 = c * 32;
    const float* bsec = smem + (c & 1) * STAGE;
    // PL = 1: the weight planes of slot (g, e) + 1 are read from LDS before slot (g, e)'s
    // MFMAs are issued (the scheduler is fenced at each slot), so a read's latency hides behind
    // RT x 6 MFMAs instead of being waited on right before its own
    auto rd_planes = [&](int ge, bf8 (&bb)[3]) {
      const int rb = brow0 + 64 * (ge >> 2) + 16 * (ge & 3);
      const int so = rb * 16 + 4 * (q ^ nt_key<4>(rb));
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bb[p] = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + p * Cfg::P_FLOATS + so));
    };
    bf8 bq[2][3];
    if constexpr (PL) rd_planes(0, bq[0]);
    bf8 ap[RT][3];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      f8 x = {lo[t][0], lo[t][1], lo[t][2], lo[t][3], hi[t][0], hi[t][1], hi[t][2], hi[t][3]};
      if (kc0 + 32 > K) {
        const int lim = K - kc0 - 4 * q;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          x[w] = w < lim ? x[w] : 0.f;
          x[4 + w] = 16 + w < lim ? x[4 + w] : 0.f;
        }
      }
      split3(x, ap[t][0], ap[t][1], ap[t][2]);
    }
    auto mm = [&](auto tp) {  // tp: the packed K tail (mfma6)
      constexpr bool TPC = decltype(tp)::value;
      if constexpr (PL) {
#pragma unroll
        for (int ge = 0; ge < 4 * G; ++ge) {
          if (ge + 1 < 4 * G) rd_planes(ge + 1, bq[(ge + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
          const int g = ge >> 2, e = ge & 3;
          const bf8 (&bb)[3] = bq[ge & 1];
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[t][g][e] = mfma6<TPC>(ap[t], bb[0], bb[1], bb[2], acc[t][g][e]);
        }
        return;
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int rb = brow0 + 64 * g + 16 * e;
          const int so = rb * 16 + 4 * (q ^ nt_key<4>(rb));
          const bf8 b0 = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + so));
          const bf8 b1 = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + Cfg::P_FLOATS + so));
          const bf8 b2 = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(bsec + 2 * Cfg::P_FLOATS + so));
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[t][g][e] = mfma6<TPC>(ap[t], b0, b1, b2, acc[t][g][e]);
        }
    };
    if constexpr (TPC) {
#pragma unroll
      for (int t = 0; t < RT; ++t) pack_tail_a(ap[t]);
    }
    mm(tp);
  };
  f4 alo[RT], ahi[RT], blo[RT], bhi[RT];
  issue_b(0);
  load_a(0, alo, ahi);
  // TP (V & 2, chosen by the host when the last chunk holds <= 16 live k): the loop runs the
  // full chunks and the last one is peeled, packed (no branch between two MFMA paths in one
  // kernel: that doubled the register pressure and spilled)
  const int Kf = TP ? Kc - 1 : Kc;
  for (int c = 0; c < Kf; c += 2) {
    step(c, alo, ahi, blo, bhi, std::false_type{});
    if (c + 1 < Kf) step(c + 1, blo, bhi, alo, ahi, std::false_type{});
  }
  if constexpr (TP) {
    if (Kf & 1) {  // the tail's A arrived in the second set
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        alo[t] = blo[t];
        ahi[t] = bhi[t];
      }
    }
    step(Kf, alo, ahi, blo, bhi, std::true_type{});
  }
  if (tile_nonfinite<RT, G>(acc, N, colw, j))  // f32 semantics for Inf / huge operands
    f32_tile<RT, G>(acc, M, N, K, A, lda, row0 + wr * 16 * RT, Bt, ldbt, 1, colw, j, q);
#define GCG_EPI_BV_READY
// C is written once and read by the next kernel long after L2 has turned over (840k x 930 =
// 3.1 GB): non-temporal stores keep the weight planes and the row blocks' A in L2 (K = 300
// projections +4 %, K = 930 unchanged, profiles/r05/nontemporal_streams.jsonl)
#define GCG_EPI_NT true
#include "gemm_epilogue.inc"
#undef GCG_EPI_BV_READY
#undef GCG_EPI_NT
}

// ---- Host side ----

// One launch of an NT kernel over M x N in BM x BN tiles (1-D grid, XCD-aware order in the kernel).
template <int BM, int BN, int THREADS, typename Kernel, typename... Extra>
gcg_status launch_nt_grid(Kernel kernel, const NtArgs& a, hipStream_t st, Extra... extra) {
  const int64_t rt = (a.M + BM - 1) / BM, ct = (a.N + BN - 1) / BN;
  if (rt * ct > 0x7fffffffLL) return fail(GCG_ERR_INVALID_ARG, "gemm_nt: M too large");
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(rt * ct)), dim3(THREADS), 0, st, a.M, a.N,
                     a.K, a.A, a.lda, extra..., a.Bt, a.ldb, a.bias, a.act, a.C, a.ldc,
                     static_cast<int>(ct));
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

template <int RT, int G, int WR, int WC, int S>
gcg_status launch_nt3_t(const NtArgs& a, const unsigned* Bs, hipStream_t st) {
  return with_packed_tail(a.K, [&](auto tp) {
    return launch_nt_grid<16 * RT * WR, 64 * G * WC, 64 * WR * WC>(
        gemm_nt3_kernel<RT, G, WR, WC, S, decltype(tp)::value>, a, st, Bs);
  });
}

template <int RT, int G, int WR, int WC, int V>  // V = 1: weight planes one slot ahead (PL)
gcg_status launch_nt3r_t(const NtArgs& a, const unsigned* Bs, hipStream_t st) {
  return with_packed_tail(a.K, [&](auto tp) {
    return launch_nt_grid<16 * RT * WR, 64 * G * WC, 64 * WR * WC>(
        gemm_nt3r_kernel<RT, G, WR, WC, V | (decltype(tp)::value ? 2 : 0)>, a, st, Bs);
  });
}

// MX = 1: bf16x6 with both operands split in the loop; only that form has a packed tail
template <int RT, int G, int WR, int WC, int S, int PF, int KC, int MX>
gcg_status launch_nt_t(const NtArgs& a, hipStream_t st) {
  auto launch = [&](auto tp) {
    return launch_nt_grid<16 * RT * WR, 64 * G * WC, 64 * WR * WC>(
        gemm_nt_kernel<RT, G, WR, WC, S, PF, KC, MX | (decltype(tp)::value ? 2 : 0)>, a, st);
  };
  if constexpr (MX == 1) return with_packed_tail(a.K, launch);
  else return launch(std::false_type{});
}

// A row of GCG_NT_TILES; in_loop: its bf16x6 form (rows with BF = 1 only)
template <int RT, int G, int WR, int WC, int S, int PF, int KC, int BF>
gcg_status launch_nt_row(bool in_loop, const NtArgs& a, hipStream_t st) {
  if constexpr (BF != 0) {
    if (in_loop) return launch_nt_t<RT, G, WR, WC, S, PF, KC, 1>(a, st);
  }
  return launch_nt_t<RT, G, WR, WC, S, PF, KC, 0>(a, st);
}

// tile: gcg_gemm_nt's f32 tile, or kNtInLoop: bf16x6 with both operands split in the loop (128 x
// 64, 32-deep, 2 stages -- the row of GCG_NT_TILES with BF = 1)
constexpr int kNtInLoop = -1;
gcg_status launch_nt(int tile, hipStream_t st, const NtArgs& a) {
  int row = 0;
#define GCG_NT_CASE(rt_, g_, wr_, wc_, s_, pf_, kc_, bf_)                                      \
  if (tile == kNtInLoop ? bf_ != 0 : tile == row++)                                            \
    return launch_nt_row<rt_, g_, wr_, wc_, s_, pf_, kc_, bf_>(tile == kNtInLoop, a, st);
  GCG_NT_TILES(GCG_NT_CASE)
#undef GCG_NT_CASE
  return fail(GCG_ERR_INVALID_ARG, "gemm_nt: no tile %d", tile);
}

// A row of GCG_NT3_TILES
template <int RT, int G, int WR, int WC, int S>
gcg_status launch_nt3_row(const NtArgs& a, const unsigned* Bs, hipStream_t st) {
  if constexpr (S == 2) return launch_nt3_t<RT, G, WR, WC, S>(a, Bs, st);
  else return launch_nt3r_t<RT, G, WR, WC, S>(a, Bs, st);
}

// tile: gcg_gemm_nt's bf16x6 tile, 1..kNt3TileCount
gcg_status launch_nt3(int tile, hipStream_t st, const NtArgs& a, const unsigned* Bs) {
  int row = 1;
#define GCG_NT3_CASE(rt_, g_, wr_, wc_, s_)                                                    \
  if (tile == row++) return launch_nt3_row<rt_, g_, wr_, wc_, s_>(a, Bs, st);
  GCG_NT3_TILES(GCG_NT3_CASE)
#undef GCG_NT3_CASE
  return fail(GCG_ERR_INVALID_ARG, "gemm_nt bf16x6: no tile %d", tile);
}

// The default's column groups G (register A, 128 rows x 64 G columns): see GCG_NT3_TILES' rule.
int pick_nt3_groups(int64_t N, int64_t K) {
  int64_t pad[4] = {0, 0, 0, 0}, least = INT64_MAX;
  for (int g = 1; g <= 3; ++g) {
    pad[g] = (N + 64 * g - 1) / (64 * g) * (64 * g);
    least = std::min(least, pad[g]);
  }
  int best = 1;
  for (int g = 1; g <= 3; ++g)
    if (pad[g] == least || (K > 512 && 4 * pad[g] <= 5 * least)) best = g;
  return best;
}
// The register-A 128-row tile of G column groups: tiles 1 and 2, and at G = 3 tile 9, which
// reads the weight planes one slot ahead (PL, bitwise the same products in the same
// order): 840k x 930 x 300 172.5-173.0 -> 176.1-176.8, 840k x 300 x 930 176.0-176.8 vs
// 174.9-177.1 (profiles/r05/nt_planes_ahead.jsonl); at G = 1 / 2 the fenced schedule lost
// (164 / 153 vs 169 / 172), so they keep the compiler's
int nt3_reg_tile(int g) { return g == 3 ? 9 : g; }

gcg_status gemm_nt_impl(const char* fn, int64_t M, int64_t N, int64_t K, const float* A,
                        int64_t lda, const float* Bt, int64_t ldbt, const float* bias, int act,
                        float* C, int64_t ldc, int math, int tile, void* ws, int64_t ws_bytes,
                        gcg_stream_t stream) {
  gcg_status s;
  if ((s = check_opts(fn, GCG_DENSE_GEMM_NT, math, tile)) != GCG_OK) return s;
  if ((s = check_sizes(fn, "MNK", M, N, K)) != GCG_OK) return s;
  if ((s = check_act(fn, act)) != GCG_OK) return s;
  // both operands are read as 16-B k-segments up to round4(K)
  if ((s = check_dense(fn, A, lda, (K + 3) & ~int64_t{3}, true)) != GCG_OK) return s;
  if ((s = check_dense(fn, Bt, ldbt, (K + 3) & ~int64_t{3}, true)) != GCG_OK) return s;
  if ((s = check_dense(fn, C, ldc, N, true)) != GCG_OK) return s;
  if (bias != nullptr && !aligned(bias, 4)) return fail(GCG_ERR_MISALIGNED, "%s: bias", fn);
  NtArgs a{int(M), int(N), int(K), A, Bt, bias, lda, ldbt, ldc, act, C};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (math == GCG_MATH_F32) {
    if (M == 0) return GCG_OK;
    return launch_nt(tile, st, a);
  }
  // bf16x6. Planes or A tiles past the 32-bit buffer offsets: both operands split in the loop.
  if (ws != nullptr && (gcg_gemm_nt_bf16x6_workspace(N, K) > INT32_MAX || 256 * lda * 4 > INT32_MAX / 2)) {
    if (tile != 0) return fail(GCG_ERR_INVALID_ARG, "%s: operands too large for tile %d", fn, tile);
    ws = nullptr;
  }
  if (ws == nullptr) {
    if (tile != 0) return fail(GCG_ERR_INVALID_ARG, "%s: tile %d needs the plane workspace", fn, tile);
    if (M == 0) return GCG_OK;
    return launch_nt(kNtInLoop, st, a);
  }
  if ((s = check_workspace_i64(fn, ws, ws_bytes, gcg_gemm_nt_bf16x6_workspace(N, K))) != GCG_OK)
    return s;
  if (M == 0) return GCG_OK;
  const int Kc = static_cast<int>((K + 31) / 32);
  if ((s = launch_split3_rows(int(N), int(K), Bt, ldbt, 1, 0, static_cast<unsigned*>(ws), st)) != GCG_OK)
    return s;
  const auto* wsp = static_cast<const unsigned*>(ws);
  if (tile != 0) return launch_nt3(tile, st, a, wsp);
  // Ragged column split (round 6): the 192-column tile over N's whole 192-column blocks and
  // the narrowest tile over the rest, when that pads less than the one shape the picker
  // chose. dP = G.W2^T at N = 300, K = 930: the picker's 128 x 192 tile (two passes over A)
  // computes 384 columns; 192 + 128 computes 320, with the same two passes over A. Every
  // output element is the same products in the same order (bitwise the one-shape result).
  const int g = pick_nt3_groups(N, K);
  const int64_t bn = 64 * g, pad_pick = (N + bn - 1) / bn * bn;
  const int64_t n_main = N / 192 * 192, r = N - n_main, gr = (r + 63) / 64;
  if (n_main > 0 && r > 0 && n_main + 64 * gr < pad_pick) {
    NtArgs a1 = a;
    a1.N = static_cast<int>(n_main);
    if ((s = launch_nt3(nt3_reg_tile(3), st, a1, wsp)) != GCG_OK) return s;
    NtArgs a2 = a;  // columns n_main .. N - 1: their weight rows, planes, bias and outputs
    a2.N = static_cast<int>(r);
    a2.Bt = Bt + n_main * ldbt;
    a2.bias = bias != nullptr ? bias + n_main : nullptr;
    a2.C = C + n_main;
    return launch_nt3(nt3_reg_tile(static_cast<int>(gr)), st, a2, wsp + n_main * Kc * 48);
  }
  return launch_nt3(nt3_reg_tile(g), st, a, wsp);
}

}  // namespace

gcg_status gcg::launch_split3_rows(int N, int K, const float* Bt, int64_t ldb, int64_t kstride,
                                   int n_out, unsigned* out, hipStream_t st) {
  const int Kc = (K + 31) / 32;
  const int64_t threads = int64_t{std::max(N, n_out)} * Kc * 4;  // one per (row, chunk, q)
  hipLaunchKernelGGL(split3_rows_kernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256),
                     0, st, N, K, Kc, Bt, ldb, out, kstride, n_out);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

extern "C" {

gcg_status gcg_gemm_nt(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                       const float* Bt, int64_t ldbt, const float* bias, int act, float* C,
                       int64_t ldc, int32_t math, int32_t tile, void* ws, int64_t ws_bytes,
                       gcg_stream_t stream) {
  return gemm_nt_impl("gcg_gemm_nt", M, N, K, A, lda, Bt, ldbt, bias, act, C, ldc, math, tile, ws,
                      ws_bytes, stream);
}

int64_t gcg_gemm_nt_workspace(int64_t N, int64_t K, int32_t math) {
  return math == GCG_MATH_BF16X6 ? gcg_gemm_nt_bf16x6_workspace(N, K) : 0;
}

gcg_status gcg_gemm_nt_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                           const float* Bt, int64_t ldbt, const float* bias, int act, float* C,
                           int64_t ldc, gcg_stream_t stream) {
  return gemm_nt_impl("gcg_gemm_nt_f32", M, N, K, A, lda, Bt, ldbt, bias, act, C, ldc,
                      GCG_MATH_F32, 0, nullptr, 0, stream);
}

int64_t gcg_gemm_nt_bf16x6_workspace(int64_t N, int64_t K) {
  if (N <= 0 || K <= 0) return 0;
  return N * ((K + 31) / 32) * 192;
}

gcg_status gcg_gemm_nt_f32_bf16x6(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                                  const float* Bt, int64_t ldbt, const float* bias, int act,
                                  float* C, int64_t ldc, void* ws, int64_t ws_bytes,
                                  gcg_stream_t stream) {
  return gemm_nt_impl("gcg_gemm_nt_f32_bf16x6", M, N, K, A, lda, Bt, ldbt, bias, act, C, ldc,
                      GCG_MATH_BF16X6, 0, ws, ws_bytes, stream);
}

}  // extern "C"
