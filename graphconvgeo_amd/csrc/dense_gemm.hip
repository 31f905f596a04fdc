// dense_gemm.hip -- C = A.B on the CDNA4 matrix cores with exact f32 products: the plain
// products (gcg_gemm) and the f32 form of the fused output layer (gcg_project_softmax_xent with
// math f32, reached through gcg::launch_gemm_fused_f32).
//
// Kernels:
//   gemm_kernel<RT, G, WR, WC, EPI>  C = A.B (+ bias, rectify) with v_mfma_f32_16x16x4_f32
//       (exact f32 in / f32 accumulate). EPI = 1 fuses the whole output row: bias, softmax,
//       cross-entropy against int32 labels, first-index argmax, and writes either
//       (softmax - onehot) * scale (the logits gradient) or the probabilities.
//   gemm_bl_kernel<G, WC, EPI>       the same product with B staged through LDS and shared by
//       4 row bands (the plain products' default; see pick_gemm_shape).
//
// Work decomposition (64-wide waves, 4 per workgroup, WR x WC of them):
//   workgroup tile  BM = 16*RT*WR rows  x  BN = 64*G*WC columns
//   wave tile       16*RT rows x 64*G columns = RT x (4G) MFMA 16x16 tiles
// A (rows x K) is staged through LDS in KC-deep chunks (double-buffered through registers),
// shared by the WC waves of a row band. B (K x N, row-major, e.g. W: 1.1 MB at K=300,
// C=930, L2-resident) is read straight into VGPRs: lane (j = l&15, q = l>>4) loads ONE
// dwordx4 B[k][c0 + 4j .. 4j+3] per k-step and uses its 4 floats as the B fragment of 4
// different 16-column tiles (tile e covers columns c0 + 4j + e). The accumulator registers
// then hold 4 adjacent columns per lane for every row -> dwordx4 stores, no shuffles.
// The k order inside a 16-deep step is permuted consistently for A and B (step e uses
// k = k0 + 4q + e), so each lane reads A as one dwordx4 from LDS as well.
#include "dense_shared.h"

using namespace gcg;

namespace {

template <int RT, int G, int WR, int WC, int EPI, int PF>
__global__ __launch_bounds__(64 * WR * WC, (PF == 1 && WR * WC == 4) ? 1 : 2) void gemm_kernel(
    int M, int N, int K, const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
    int64_t ldb, const float* __restrict__ bias, int act, float* __restrict__ Cout, int64_t ldc,
    const int32_t* __restrict__ labels, float scale, const float* __restrict__ scale_dev,
    float* __restrict__ loss_rows, float* __restrict__ correct_rows,
    const float* __restrict__ row_w) {
  constexpr int NT = 64 * WR * WC;  // threads per workgroup (4 or 8 waves)
  static_assert(WR * WC == 4 || WR * WC == 8, "4 or 8 waves per workgroup");
  constexpr int BM = 16 * RT * WR;
  constexpr int BN = 64 * G * WC;
  constexpr int KC = 32;                   // k depth of one LDS chunk
  constexpr int A4 = BM * KC / 4 / NT;     // A dwordx4 per thread per chunk
  static_assert(A4 >= 1 && BM * KC / 4 % NT == 0, "A chunk must split evenly");
  // A chunk image: unpadded 128-B rows of 8 slots (16 B each), slot s of row r stored at slot
  // s ^ ((r >> 1) & 7). A fragment ds_read_b128 is serviced in 4 lane groups of 16, each
  // holding every j = 0..15 once with two q values ({0-3,12-15} with q, {4-11} with q + 1 or
  // the reverse, MI355X_MICROARCH.md §LDS): with this key the 16 starting dwords of a group
  // are 16 distinct multiples of 4 mod 64 -- conflict-free (the 36-float padded rows of round
  // 1-2 gave 2-way conflicts there: 13 % of the LDS cycles, PMC r02). The 8-lane groups of
  // the ds_write_b128 still cover one whole row each: conflict-free too.
  __shared__ float As[2][BM][KC];
  auto aslot = [](int r, int slot) { return (slot ^ ((r >> 1) & 7)) * 4; };
  __shared__ float red[4][WC][BM];  // epilogue row reductions: sum, label logit, argmax, max
  // EPI = 1: the bias of the workgroup's columns and the labels of its rows, staged in LDS
  // at the start so the epilogue reads them from LDS instead of waiting on global loads
  __shared__ float sbias[EPI == 1 ? BN : 1];
  __shared__ int slab[EPI == 1 ? BM : 1];
  __shared__ float srw[EPI == 1 ? BM : 1];  // row weights (target multiplicities), 1 if none

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: uniform branches
  const int wr = wave / WC, wc = wave % WC;
  const int j = lane & 15, q = lane >> 4;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int colw = blockIdx.y * BN + wc * G * 64;  // this wave's first column
  const int n4 = (N + 3) & ~3;                     // columns B may be read at (<= ldb)

  // Per-lane B column offsets (clamped in range; out-of-range columns are never stored).
  int bcol[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int c = colw + 64 * g + 4 * j;
    bcol[g] = c < n4 ? c : 0;
  }

  f4 acc[RT][G][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][g][e] = f4{0.f, 0.f, 0.f, 0.f};

  // ---- A staging: chunk c covers k in [c*KC, c*KC + KC) ----
  // Branch-free: row and column are clamped into the operand and out-of-range elements are
  // zeroed by selects, so the loop body is straight-line and hipcc keeps counted vmcnt waits
  // (a branchy load makes it drain every load in flight). A 16-B load at a clamped column
  // stays inside the 16-B aligned block of a valid element, hence inside the allocation.
  const int kmax4 = (K - 1) & ~3;  // last 4-aligned column start with a valid element
  // The out-of-range elements are zeroed when the registers are written to LDS (store_a), not
  // right after the load: a select on the loaded value makes hipcc wait for the load there,
  // at the top of the chunk, instead of at the chunk's end.
  f4 areg[A4];
  int avalid[A4];  // valid elements of areg[i]: 0..4 (0 for a row past M)
  auto load_a = [&](int kc0) {
#pragma unroll
    for (int i = 0; i < A4; ++i) {
      const int idx = tid + NT * i;
      const int r = idx / (KC / 4), k = kc0 + (idx % (KC / 4)) * 4;
      const int64_t gr = row0 + r;
      const int64_t rr = gr < M ? gr : M - 1;
      const int kk = k < kmax4 ? k : kmax4;
      areg[i] = *reinterpret_cast<const f4*>(A + rr * lda + kk);
      avalid[i] = gr < M ? min(max(K - k, 0), 4) : 0;
    }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A4; ++i) {
      const int idx = tid + NT * i;
      const int r = idx / (KC / 4), slot = idx % (KC / 4);
      f4 v = areg[i];
      v.x = avalid[i] > 0 ? v.x : 0.f;
      v.y = avalid[i] > 1 ? v.y : 0.f;
      v.z = avalid[i] > 2 ? v.z : 0.f;
      v.w = avalid[i] > 3 ? v.w : 0.f;
      *reinterpret_cast<f4*>(&As[buf][r][aslot(r, slot)]) = v;
    }
  };
  // Workgroup barrier for the LDS hand-off only: waits for this wave's LDS traffic, not for
  // its global loads (a __syncthreads() fence would drain the B prefetch every chunk).
  auto lds_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  // ---- B fragments for one 16-deep k-step: bf[g][e] = B[k0 + 4q + e][bcol[g] .. +3] ----
  // Fragments (g, e) with unit u = 4g + e in [u0, u1) only (the split ping-pong body loads
  // one part of the set at a time).
  // B is read through a buffer descriptor re-based at row k0 for every step (scalar work): the
  // range check returns 0 for rows past K (A is 0 there as well), so the per-lane row clamp and
  // 64-bit row addresses of round 2 (~48 VALU per 16-deep step, VALU that lowered the clock this
  // MFMA loop holds) are gone; the per-lane byte offsets are constants. Host: K * ldb * 4 < 2^31.
  uint32_t boff[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      boff[g][e] = static_cast<uint32_t>(((4 * q + e) * static_cast<int>(ldb) + bcol[g]) * 4);
  auto load_b = [&](f4 (&bf)[G][4], int k0, int u0 = 0, int u1 = 4 * G) {
    const int kb = k0 < K ? k0 : K;  // a prefetch past K gets an empty range: zeros
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(B + static_cast<int64_t>(kb) * ldb), static_cast<short>(0),
        (K - kb) * static_cast<int>(ldb) * 4, 0x00020000);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (4 * g + e >= u0 && 4 * g + e < u1)
          bf[g][e] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, boff[g][e], 0, 0));
  };

  const int arow = wr * 16 * RT + j;
  // Skipping groups past N (a wave-uniform branch per step and group) measured faster with the
  // register-prefetch (PF = 1) body -- without it hipcc shuffles the accumulators through
  // AGPR copies and spills -- and slower with the single-buffer body.
  constexpr bool SKIP = PF != 0;
  const int ngv = min(G, max(0, (N - colw + 63) / 64));  // groups with a column < N
  auto compute = [&](const f4 (&bf)[G][4], int buf, int s, int u0 = 0, int u1 = 4 * G) {
    f4 af[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
      af[t] = *reinterpret_cast<const f4*>(&As[buf][arow + 16 * t][aslot(arow + 16 * t, 4 * s + q)]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (4 * g + e < u0 || 4 * g + e >= u1) continue;  // compile-time after unrolling
        if (SKIP && g >= ngv) continue;  // scalar branch: group entirely past N
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          acc[t][g][0] = mfma4(af[t][e], bf[g][e].x, acc[t][g][0]);
          acc[t][g][1] = mfma4(af[t][e], bf[g][e].y, acc[t][g][1]);
          acc[t][g][2] = mfma4(af[t][e], bf[g][e].z, acc[t][g][2]);
          acc[t][g][3] = mfma4(af[t][e], bf[g][e].w, acc[t][g][3]);
        }
      }
  };

  // Main loop, one 32-deep chunk (two 16-deep steps) per iteration, straight-line: B
  // ping-pongs between two register sets (step 2c in b0, 2c+1 in b1, each loaded one step
  // ahead), A chunk c+1 is loaded to registers during chunk c and written to the other LDS
  // buffer after it.
  static_assert(KC == 32, "two 16-deep steps per chunk");
  __builtin_assume(K > 0);  // checked on the host: the main loop runs at least once
  const int n_chunks = (K + KC - 1) / KC;
  load_a(0);
  if constexpr (EPI == 1) {
    for (int c = tid; c < BN; c += NT) {
      const int gc = blockIdx.y * BN + c;
      // columns past N: -inf, so their softmax weight is exactly 0 (no mask in the epilogue)
      sbias[c] = gc < N ? (bias != nullptr ? bias[gc] : 0.f) : kNegInf;
    }
    for (int r = tid; r < BM; r += NT) {
      const int64_t row = row0 + r;
      int y = (labels != nullptr && row < M) ? labels[row] : -1;
      // -1: no label; a label outside [0, N) becomes -2: NaN loss, no hit, no onehot
      if (labels != nullptr && (y < 0 || y >= N)) y = -2;
      slab[r] = y;
      srw[r] = (row_w != nullptr && row < M) ? row_w[row] : 1.f;
    }
    // (issued beside the first A chunk's loads; visible after the barrier below)
  }
  store_a(0);
  lds_barrier();
  f4 b0[G][4];
  if constexpr (PF >= 2) {
    // Split ping-pong in one register set: b0's 4G fragments (g, e) are cut into NP = PF
    // parts that rotate, each part loaded for the next 16-deep step as soon as its MFMAs for
    // this step are issued, so a wave computes the other parts while a part's loads are in
    // flight (PF = 1's latency hiding at PF = 0's register count, which keeps 2 workgroups
    // per CU). Every accumulator still sees e = 0..3 in order: bitwise equal to PF = 0.
    constexpr int NP = PF, NU = 4 * G;
    static_assert(NU % NP == 0, "parts split the fragments evenly");
    // The prologue issues the parts in ring order (scheduling barriers; K > 0 is assumed so
    // the loads are not sunk past a zero-trip branch): hipcc merges the preheader's and the
    // back-edge's outstanding loads at the loop header and otherwise drains the ring there
    // (vmcnt(2)); now every wait is counted (vmcnt(15..16)). Measured neutral (the kernel runs
    // at a power-limited clock), kept for the cleaner schedule. Pinning the loop body as well
    // measured slower: 93.0-95.0 vs 96.2 TFLOP/s.
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      load_b(b0, 0, p * NU / NP, (p + 1) * NU / NP);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (int c = 0; c < n_chunks; ++c) {
      const int buf = c & 1;
      const int k0 = c * KC;
      load_a(k0 + KC);  // past K: clamped and zeroed, never used
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        // the second 16-deep step of the last chunk lies wholly past K (A is zero there):
        // skip its MFMAs and the refills, which would only fetch rows past K
        if (st == 1 && k0 + 16 >= K) break;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          compute(b0, buf, st, p * NU / NP, (p + 1) * NU / NP);
          load_b(b0, k0 + 16 * (st + 1), p * NU / NP, (p + 1) * NU / NP);
        }
      }
      store_a(buf ^ 1);
      lds_barrier();
    }
  } else if constexpr (PF) {
    f4 b1[G][4];
    load_b(b0, 0);
    for (int c = 0; c < n_chunks; ++c) {
      const int buf = c & 1;
      const int k0 = c * KC;
      load_a(k0 + KC);  // past K: clamped and zeroed, never used
      load_b(b1, k0 + 16);
      compute(b0, buf, 0);
      load_b(b0, k0 + 32);
      if (k0 + 16 < K) compute(b1, buf, 1);
      store_a(buf ^ 1);
      lds_barrier();
    }
  } else {
    // One B register set: a wave waits for its step's loads while the other wave(s) on
    // its SIMD compute (8-wave workgroups, 2 waves per SIMD).
    for (int c = 0; c < n_chunks; ++c) {
      const int buf = c & 1;
      const int k0 = c * KC;
      load_a(k0 + KC);
      load_b(b0, k0);
      compute(b0, buf, 0);
      if (k0 + 16 < K) {
        load_b(b0, k0 + 16);
        compute(b0, buf, 1);
      }
      store_a(buf ^ 1);
      lds_barrier();
    }
  }

#define GCG_EPI_BV_READY
#define GCG_EPI_LABELS_LDS
  f4 bv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if constexpr (EPI == 1) {
      bv[g] = *reinterpret_cast<const f4*>(&sbias[wc * G * 64 + 64 * g + 4 * j]);
    } else {
      bv[g] = f4{0.f, 0.f, 0.f, 0.f};
      const int c = colw + 64 * g + 4 * j;
      if (bias != nullptr) {
        if (c < N) bv[g].x = bias[c];
        if (c + 1 < N) bv[g].y = bias[c + 1];
        if (c + 2 < N) bv[g].z = bias[c + 2];
        if (c + 3 < N) bv[g].w = bias[c + 3];
      }
    }
  }
#include "gemm_epilogue.inc"
#undef GCG_EPI_BV_READY
#undef GCG_EPI_LABELS_LDS
}

// ---------------------------------------------------------------------------------------
// gemm_bl_kernel<G, WC, EPI>: the same product and epilogues with B staged through LDS.
// Workgroup = 4 row bands (WR = 4) x WC column waves, wave tile 16 rows x 64*G columns
// (RT = 1), workgroup tile 64 x 64*G*WC. Per 32-deep k chunk the workgroup copies A[64 x 32]
// and B[32 x BN] to LDS once; the 4 row bands share every B fragment, so B leaves L2 once per
// 64 rows (gemm_kernel: once per 16*RT rows per wave) and a fragment read costs LDS latency
// instead of L2 latency. The next chunk's loads are issued into registers before the current
// chunk's MFMAs and written to LDS after them (one LDS buffer, two barriers per chunk).
// LDS B image: row k at k*BN floats; lanes (j, q) of one ds_read_b128 group read rows
// k0+4q+e, columns 4j..4j+3: BN % 16 == 0 keeps every 16-lane group on 64 distinct banks.
// ---------------------------------------------------------------------------------------
template <int G, int WC, int EPI>
__global__ __launch_bounds__(256 * WC, WC == 1 ? 2 : 1) void gemm_bl_kernel(
    int M, int N, int K, const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
    int64_t ldb, const float* __restrict__ bias, int act, float* __restrict__ Cout, int64_t ldc,
    const int32_t* __restrict__ labels, float scale, const float* __restrict__ scale_dev,
    float* __restrict__ loss_rows, float* __restrict__ correct_rows,
    const float* __restrict__ row_w) {
  constexpr int RT = 1, WR = 4;
  constexpr int NT = 64 * WR * WC;
  constexpr int BM = 16 * RT * WR;  // 64
  constexpr int BN = 64 * G * WC;
  constexpr int KC = BN >= 512 ? 16 : 32;  // k depth of one chunk: wide B -> fewer staging VGPRs
  constexpr int KP = KC + 4;
  constexpr int AT = BM * KC / 4 < NT ? BM * KC / 4 : NT;  // threads staging A (whole waves)
  constexpr int A4 = BM * KC / 4 / AT;
  constexpr int B4 = KC * BN / 4 / NT;
  static_assert(AT % 64 == 0 && A4 >= 1 && BM * KC / 4 % AT == 0, "A chunk must split evenly");
  static_assert(B4 >= 1 && KC * BN / 4 % NT == 0, "B chunk must split evenly");
  static_assert(BN % 16 == 0, "conflict-free B fragment reads");
  // NB = 2 LDS buffers (one barrier per chunk) for the 8-wave tiles, which hold a CU alone
  // anyway; the 4-wave tiles keep one buffer (two barriers) so 2-3 workgroups share a CU
  constexpr int NB = (WC >= 2 && (2 * (BM * KP + KC * BN) + 4 * WC * BM) * 4 <= 160 * 1024) ? 2 : 1;
  __shared__ float As[NB][BM][KP];
  __shared__ float Bs[NB][KC][BN];
  __shared__ float red[4][WC][BM];  // epilogue row reductions: sum, label logit, argmax, max

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int j = lane & 15, q = lane >> 4;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int colb = blockIdx.y * BN;          // workgroup's first column
  const int colw = colb + wc * G * 64;       // this wave's first column
  const int n4 = (N + 3) & ~3;

  f4 acc[RT][G][4];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[0][g][e] = f4{0.f, 0.f, 0.f, 0.f};

  // Branch-free staging loads (clamped addresses, zeroed by selects): see gemm_kernel.
  const int kmax4 = (K - 1) & ~3;
  f4 areg[A4], breg[B4];
  const bool a_stager = tid < AT;  // wave-uniform
  auto load_chunk = [&](int kc0) {
#pragma unroll
    for (int i = 0; i < A4; ++i) {
      const int idx = (a_stager ? tid : tid - AT) + AT * i;  // non-stagers: a harmless copy
      const int r = idx / (KC / 4), k = kc0 + (idx % (KC / 4)) * 4;
      const int64_t gr = row0 + r;
      const int64_t rr = gr < M ? gr : M - 1;
      const int kk = k < kmax4 ? k : kmax4;
      f4 v = *reinterpret_cast<const f4*>(A + rr * lda + kk);
      const bool rowok = gr < M;
      v.x = (rowok && k < K) ? v.x : 0.f;
      v.y = (rowok && k + 1 < K) ? v.y : 0.f;
      v.z = (rowok && k + 2 < K) ? v.z : 0.f;
      v.w = (rowok && k + 3 < K) ? v.w : 0.f;
      areg[i] = v;
    }
#pragma unroll
    for (int i = 0; i < B4; ++i) {
      const int idx = tid + NT * i;
      const int kr = idx / (BN / 4), c = colb + (idx % (BN / 4)) * 4;
      int k = kc0 + kr;
      k = k < K ? k : K - 1;         // A is zero there; any finite B row does
      const int cc = c < n4 ? c : 0;  // columns past N: never stored (masked in EPI = 1)
      breg[i] = *reinterpret_cast<const f4*>(B + static_cast<int64_t>(k) * ldb + cc);
    }
  };
  auto store_chunk = [&](int buf) {
    if (a_stager) {
#pragma unroll
      for (int i = 0; i < A4; ++i) {
        const int idx = tid + AT * i;
        *reinterpret_cast<f4*>(&As[buf][idx / (KC / 4)][(idx % (KC / 4)) * 4]) = areg[i];
      }
    }
#pragma unroll
    for (int i = 0; i < B4; ++i) {
      const int idx = tid + NT * i;
      *reinterpret_cast<f4*>(&Bs[buf][idx / (BN / 4)][(idx % (BN / 4)) * 4]) = breg[i];
    }
  };
  auto lds_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  const int arow = wr * 16 + j;
  const int bl = wc * G * 64 + 4 * j;  // this lane's column inside the LDS B image
  auto compute_step = [&](int buf, int s) {
    const f4 af = *reinterpret_cast<const f4*>(&As[buf][arow][s * 16 + 4 * q]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // all G fragments of this k first (no branch between them: the reads stay in flight
      // together), then 4G MFMAs; groups past N compute on clamped columns, never stored
      const float* brow = &Bs[buf][s * 16 + 4 * q + e][bl];
      f4 bf[G];
#pragma unroll
      for (int g = 0; g < G; ++g) bf[g] = *reinterpret_cast<const f4*>(brow + 64 * g);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        acc[0][g][0] = mfma4(af[e], bf[g].x, acc[0][g][0]);
        acc[0][g][1] = mfma4(af[e], bf[g].y, acc[0][g][1]);
        acc[0][g][2] = mfma4(af[e], bf[g].z, acc[0][g][2]);
        acc[0][g][3] = mfma4(af[e], bf[g].w, acc[0][g][3]);
      }
    }
  };

  const int n_chunks = (K + KC - 1) / KC;
  load_chunk(0);
  store_chunk(0);
  lds_barrier();
  for (int c = 0; c < n_chunks; ++c) {
    const int k0 = c * KC;
    const int buf = NB == 2 ? (c & 1) : 0;
    const bool more = c + 1 < n_chunks;
    if (more) load_chunk(k0 + KC);  // in flight during this chunk's MFMAs
    compute_step(buf, 0);
    if (KC == 32 && k0 + 16 < K) compute_step(buf, 1);
    if (more) {
      // two buffers: the other one was last read in chunk c-1, before the barrier that
      // ended it; one buffer: wait until every wave is done reading this chunk
      if (NB == 1) lds_barrier();
      store_chunk(NB == 2 ? buf ^ 1 : 0);
      lds_barrier();
    }
  }
#include "gemm_epilogue.inc"
}

// ---- Host side ----

struct Shape {
  int RT, G, WR, WC, PF = 1;
  int BL = 0;  // 1: gemm_bl_kernel (B through LDS; RT = 1, WR = 4)
  int bm() const { return 16 * RT * WR; }
  int bn() const { return 64 * G * WC; }
};

// The instantiation of a shape, from the tile lists of dense_shared.h. EPI = 0 (plain products):
// the LDS-B tiles (gemm_bl_kernel, the default) and the register-B tiles (gcg_gemm tile 1).
// EPI = 1 (the fused output layer on the f32 MFMA): row bands keeping a whole output row of up
// to 1024 columns in one workgroup, the B register set split into PF rotating parts (the default
// 8 at G = 4, 4 below).
template <int EPI>
gcg_status launch_gemm(const Shape& s, hipStream_t st, const FusedArgs& a, int act) {
  const dim3 grid(static_cast<unsigned>((a.M + s.bm() - 1) / s.bm()),
                  static_cast<unsigned>((a.N + s.bn() - 1) / s.bn()));
#define GCG_GEMM_ARGS                                                                          \
  0, st, a.M, a.N, a.K, a.A, a.lda, a.B, a.ldb, a.bias, act, a.C, a.ldc, a.labels, a.scale,    \
      a.scale_dev, a.loss_rows, a.correct_rows, a.row_w
#define GCG_GEMM_BL_CASE(g, wc)                                                                \
  if (s.BL && s.G == g && s.WC == wc) {                                                        \
    hipLaunchKernelGGL((gemm_bl_kernel<g, wc, EPI>), grid, dim3(256 * (wc)), GCG_GEMM_ARGS);   \
    GCG_HIP_CHECK(hipGetLastError());                                                          \
    return GCG_OK;                                                                             \
  }
#define GCG_GEMM_CASE(rt, g, wr, wc, pf)                                                       \
  if (!s.BL && s.RT == rt && s.G == g && s.WR == wr && s.WC == wc && s.PF == pf) {             \
    hipLaunchKernelGGL((gemm_kernel<rt, g, wr, wc, EPI, pf>), grid, dim3(64 * (wr) * (wc)),    \
                       GCG_GEMM_ARGS);                                                         \
    GCG_HIP_CHECK(hipGetLastError());                                                          \
    return GCG_OK;                                                                             \
  }
  if constexpr (EPI == 0) {
    GCG_GEMM_BL_TILES(GCG_GEMM_BL_CASE)
    GCG_GEMM_REG_TILES(GCG_GEMM_CASE)
  } else {
    GCG_GEMM_CASE(2, 1, 1, 4, 1)
    // G = 4: every split of the B set; G = 2, 3: up to 4 parts (pick_fused_shape)
#define GCG_GEMM_PARTS_CASE(pf)                                                                \
  GCG_GEMM_CASE(2, 4, 1, 4, pf)                                                                \
  if constexpr (pf <= 4) {                                                                     \
    GCG_GEMM_CASE(2, 3, 1, 4, pf)                                                              \
    GCG_GEMM_CASE(2, 2, 1, 4, pf)                                                              \
  }
    GCG_FUSED_PARTS(GCG_GEMM_PARTS_CASE)
#undef GCG_GEMM_PARTS_CASE
  }
#undef GCG_GEMM_CASE
#undef GCG_GEMM_BL_CASE
#undef GCG_GEMM_ARGS
  return fail(GCG_ERR_INVALID_ARG, "gemm: no tile instantiated for RT=%d G=%d WR=%d WC=%d PF=%d",
              s.RT, s.G, s.WR, s.WC, s.PF);
}

// Plain products (gcg_gemm). Tile 0, B through LDS (gemm_bl_kernel), measured on the train
// step's shapes (by a script that is no longer in the tree; TFLOP/s, B-from-L2 gemm_kernel ->
// LDS-B):
//   840k x 300 x 930  93.5 -> 96.7 (16 waves x 256 columns)   1.4M x 300 x 930  94.5 -> 97.0
//   840k x 930 x 300  90.9 -> 105.1 (4 waves x 320 columns)   1.4M x 930 x 300  91.6 -> 105.7
// Tile 1: B from L2 straight to registers (gemm_kernel), the same k order (bitwise equal).
Shape pick_gemm_shape(int64_t N, int tile) {
  const int groups = static_cast<int>((N + 63) / 64);
  if (tile == 0) {
    if (groups <= 5) return Shape{1, std::max(groups, 1), 4, 1, 0, 1};
    if (groups <= 8) return Shape{1, 4, 4, 2, 0, 1};
    return Shape{1, 4, 4, 4, 0, 1};  // 1024 columns per workgroup, grid.y for the rest
  }
  if (groups <= 5) return Shape{2, std::max(groups, 1), 4, 1};  // one wave spans all columns
  return Shape{4, std::min(4, (groups + 3) / 4), 1, 4};         // RT = 4, 1 workgroup per CU
}

// The fused output layer on the f32 MFMA (gemm_kernel EPI = 1): the workgroup holds the whole
// row (WC = 4, G = ceil(N / 256)), measured on Twitter-World's 840k x 300 x 930 (TFLOP/s):
//   RT = 4, B ping-pong, 1 workgroup per CU          78.7
//   RT = 2, one B set, 2 workgroups per CU           85.0-87.4: the second workgroup hides B
//       latency and overlaps the other's softmax epilogue + stores
//   ... + B set split into 2 / 4 / 8 / 16 rotating parts, groups past N skipped
//                                                    92.3, 96.4, 96.8, 95.4  <- 8 parts
// `parts` (tiles 1..5, GCG_FUSED_PARTS) only reorders MFMAs between distinct accumulators.
#define GCG_FUSED_PART(pf) pf,
constexpr int kFusedParts[] = {GCG_FUSED_PARTS(GCG_FUSED_PART)};
#undef GCG_FUSED_PART
Shape pick_fused_shape(int64_t N, int parts) {
  const int groups = static_cast<int>((N + 63) / 64);
  const int g = std::min(4, (groups + 3) / 4);
  if (g < 2) return Shape{2, 1, 1, 4};
  const int sp = parts < 0 ? 8 : parts;
  const int np = sp >= 8 && g == 4 ? (sp >= 16 ? 16 : 8) : sp >= 4 ? 4 : sp >= 2 ? 2 : 0;
  return Shape{2, g, 1, 4, np};
}

// gcg_gemm: validation, then the tile.
gcg_status gemm_impl(const char* fn, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                     const float* B, int64_t ldb, const float* bias, int act, float* C,
                     int64_t ldc, gcg_stream_t stream, int math, int tile) {
  gcg_status s;
  if ((s = check_opts(fn, GCG_DENSE_GEMM, math, tile)) != GCG_OK) return s;
  if ((s = check_sizes(fn, "MNK", M, N, K)) != GCG_OK) return s;
  if ((s = check_act(fn, act)) != GCG_OK) return s;
  if ((s = check_dense(fn, A, lda, K, true)) != GCG_OK) return s;
  // B is read as dwordx4 at columns < round4(N): its row stride must cover them.
  if ((s = check_dense(fn, B, ldb, (N + 3) & ~int64_t{3}, true)) != GCG_OK) return s;
  if ((s = check_dense(fn, C, ldc, N, true)) != GCG_OK) return s;
  if (M == 0) return GCG_OK;
  if ((s = check_b_range(fn, K, ldb)) != GCG_OK) return s;
  const FusedArgs a{int(M), int(N), int(K), A, B, bias, lda, ldb, ldc, C,
                    nullptr, 0.f, nullptr, nullptr, nullptr, nullptr};
  return launch_gemm<0>(pick_gemm_shape(N, tile), static_cast<hipStream_t>(stream), a, act);
}

}  // namespace

gcg_status gcg::launch_gemm_fused_f32(const FusedArgs& a, int tile, hipStream_t st) {
  return launch_gemm<1>(pick_fused_shape(a.N, tile == 0 ? -1 : kFusedParts[tile - 1]), st, a,
                        GCG_ACT_NONE);
}

extern "C" {

int32_t gcg_dense_tile_count(int32_t op, int32_t math) {
  const bool f32 = math == GCG_MATH_F32, bf = math == GCG_MATH_BF16X6;
  switch (op) {
    case GCG_DENSE_GEMM: return f32 ? kGemmTileCount : -1;
    case GCG_DENSE_GEMM_NT: return f32 ? kNtTileCount : bf ? kNt3TileCount : -1;
    case GCG_DENSE_FUSED: return f32 ? kFusedTileCount : bf ? kFused6TileCount : -1;
    case GCG_DENSE_GEMM_TN: return f32 ? kTnTileCount : bf ? 0 : -1;
    default: return -1;
  }
}

gcg_status gcg_gemm(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                    int64_t ldb, const float* bias, int act, float* C, int64_t ldc, int32_t math,
                    int32_t tile, gcg_stream_t stream) {
  return gemm_impl("gcg_gemm", M, N, K, A, lda, B, ldb, bias, act, C, ldc, stream, math, tile);
}

gcg_status gcg_gemm_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                        const float* B, int64_t ldb, const float* bias, int act, float* C,
                        int64_t ldc, gcg_stream_t stream) {
  return gemm_impl("gcg_gemm_f32", M, N, K, A, lda, B, ldb, bias, act, C, ldc, stream,
                   GCG_MATH_F32, 0);
}

}  // extern "C"
