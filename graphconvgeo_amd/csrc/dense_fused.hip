// dense_fused.hip -- the fused output layer P . W + b -> softmax, cross-entropy, hits and the
// logits gradient or the probabilities (gcg_project_softmax_xent), and the same row epilogue for
// logits that already exist (gcg_softmax_xent).
// gemm_fused6_kernel is the layer on the bf16 matrix cores (bf16x6); its f32 form is
// gemm_kernel<..., EPI = 1> of dense_gemm.hip and its weight pre-split split3_rows_kernel of
// dense_nt.hip (gcg::launch_gemm_fused_f32, gcg::launch_split3_rows). softmax_xent_rows_kernel:
// the reference order, where the logits come out of the H SpMM (mlpconv.py:90-94).
#include "dense_shared.h"

using namespace gcg;

namespace {

// ---------------------------------------------------------------------------------------
// gemm_fused6_kernel<RT, G>: the fused output layer (gemm_kernel EPI = 1: P . W + b -> softmax,
// cross-entropy, hits, logits gradient / probabilities) with the products on the bf16 matrix
// cores (bf16x6, as gcg_gemm_nt_f32_bf16x6; round 4). A workgroup owns 16 RT whole rows: 4
// waves x 64 G columns (N <= 256 G). A goes through the LDS-DMA ring (the nt3 image: [BM][8
// slots], key r & 7; each wave reads all rows) and is split in registers; the weight W
// (K x N, L2-resident) is read straight into registers as f32, one dwordx4 of 4 adjacent columns
// per lane and k row -- rows k0 + 4q + i and k0 + 16 + 4q + i (i < 4) give, per column, the 8
// k-values of the lane's bf16 operand in the A image's k order -- and split in registers; the
// next 64-column group's 8 loads are in flight while a group computes. Weight rows past K read
// as 0 (buffer range), A's elements past K are zeroed before the split, W's padding columns
// are handled by the epilogue's straddle guard. All LDS (ring, row reductions, bias, labels,
// row weights) is one array: a second __shared__ object makes hipcc drain the DMA queue.
// Round 5: A (each row read by exactly one workgroup) is DMA'd and the logits gradient stored
// with the non-temporal policy, so these streams (1 GB in, 3.1 GB out at Twitter-World) stop
// evicting the weight planes every workgroup re-reads from L2: World 139.4-140.1 -> 147.6-148.6
// TF (bf16x6), Twitter-US and the f32 forms unchanged (profiles/r05/nontemporal_streams.jsonl).
// ---------------------------------------------------------------------------------------
// CS = 1 (round 5, FX only): the A chunk is split cooperatively -- each of the workgroup's
// threads splits one 16-B k-quad of one row (BM x 8 quads = the thread count) and writes its
// three planes to an LDS image ([plane][BM rows][4 slots of 16 B], key nt_key<4>, the NT
// kernel's conflict-free B image), then every wave reads its RT x 3 plane fragments from it --
// instead of all WR x WC waves splitting all BM rows in registers; one more barrier per chunk.
// TP: the packed K tail (mfma6): the last chunk peeled, packed (host: when it holds <= 16 k).
template <int RT, int G, int WR = 1, int WC = 4, int SB = 0, int FX = 0, int CS = 0, bool TP = false>
__global__ __launch_bounds__(64 * WR * WC, WR * WC == 4 ? 2 : 1) void gemm_fused6_kernel(
    int M, int N, int K, const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
    int64_t ldb, const float* __restrict__ bias, float* __restrict__ Cout, int64_t ldc,
    const int32_t* __restrict__ labels, float scale, const float* __restrict__ scale_dev,
    float* __restrict__ loss_rows, float* __restrict__ correct_rows,
    const float* __restrict__ row_w, const unsigned* __restrict__ Wsplit = nullptr) {
  constexpr int EPI = 1, S = 2;
  constexpr int BM = 16 * RT * WR, BN = 64 * G * WC;
  constexpr int STAGE = BM * 32;                 // A image floats per stage
  constexpr int NGA = BM / 8;                    // A DMA wave-instructions per stage
  constexpr int UA = NGA / (WR * WC);
  static_assert(NGA % (WR * WC) == 0, "whole A DMA instructions per wave");
  constexpr int OFF_RED = S * STAGE, OFF_BIAS = OFF_RED + 4 * WC * BM;
  constexpr int OFF_LAB = OFF_BIAS + BN, OFF_RW = OFF_LAB + BM;
  constexpr int OFF_PL = OFF_RW + BM, PL_FLOATS = BM * 16;  // (CS) plane p image at p * PL_FLOATS
  __shared__ __attribute__((aligned(16))) float smem[OFF_PL + (CS ? 3 * PL_FLOATS : 0)];
  static_assert(!CS || (FX && BM * 8 == 64 * WR * WC), "CS: one k-quad of one row per thread");
  float (*red)[WC][BM] = reinterpret_cast<float (*)[WC][BM]>(smem + OFF_RED);
  float* sbias = smem + OFF_BIAS;
  int* slab = reinterpret_cast<int*>(smem + OFF_LAB);
  float* srw = smem + OFF_RW;
  const int act = GCG_ACT_NONE;
  (void)act;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int j = lane & 15, q = lane >> 4;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int colw = wc * G * 64;
  const int Kc = (K + 31) / 32;
  const int rows_here = static_cast<int>(M - row0 < BM ? M - row0 : BM);
  const int n4 = (N + 3) & ~3;

  // A DMA: instruction i = wave + WC u fills image rows 8i .. 8i + 7
  int voff[UA];
#pragma unroll
  for (int u = 0; u < UA; ++u) {
    const int r = 8 * (wave + WR * WC * u) + lane / 8;
    const int rl = r < rows_here ? r : rows_here - 1;
    voff[u] = (rl * static_cast<int>(lda) + 4 * ((lane % 8) ^ (r & 7))) * 4;
  }
  const int a_bytes = ((rows_here - 1) * static_cast<int>(lda) + ((K + 3) & ~3)) * 4;
  auto issue_a = [&](int chunk) {
    float* stage = smem + (chunk & 1) * STAGE;
    const auto ra = brsrc(A + row0 * lda + 32 * chunk, a_bytes - 128 * chunk);
#pragma unroll
    for (int u = 0; u < UA; ++u) blds16_nt(ra, stage + (wave + WR * WC * u) * 256, voff[u]);
  };
  // W: lane offsets (row 4q, column of group g); rows i and 16 + i through the scalar offset
  int bofs[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int c = colw + 64 * g + 4 * j;
    bofs[g] = ((4 * q) * static_cast<int>(ldb) + (c < n4 ? c : 0)) * 4;
  }
  const int ldb4 = static_cast<int>(ldb) * 4;
  auto load_w = [&](int chunk, int g, f4 (&w)[8]) {
    const int k0 = 32 * chunk;
    const auto rw = brsrc(B + static_cast<int64_t>(k0) * ldb, (K - k0) * ldb4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rw, bofs[g], i * ldb4, 0));
      w[4 + i] = __builtin_bit_cast(
          f4, __builtin_amdgcn_raw_buffer_load_b128(rw, bofs[g], (16 + i) * ldb4, 0));
    }
  };

  f4 acc[RT][G][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][g][e] = f4{0.f, 0.f, 0.f, 0.f};

  for (int c = tid; c < BN; c += 64 * WR * WC)  // columns past N: -inf (softmax weight 0)
    sbias[c] = c < N ? (bias != nullptr ? bias[c] : 0.f) : kNegInf;
  for (int r = tid; r < BM; r += 64 * WR * WC) {
    const int64_t row = row0 + r;
    int y = (labels != nullptr && row < M) ? labels[row] : -1;
    if (labels != nullptr && (y < 0 || y >= N)) y = -2;  // outside [0, N): NaN loss, no hit
    slab[r] = y;
    srw[r] = (row_w != nullptr && row < M) ? row_w[row] : 1.f;
  }
  __syncthreads();
  // the bias is the accumulators' starting value (b + sum of products), so the epilogue adds
  // nothing per element; columns past N start at 0 and become -inf in the epilogue (round 6:
  // +3 %, every wave of the CU's one workgroup runs the epilogue with the matrix pipe idle)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const f4 bb = *reinterpret_cast<const f4*>(&sbias[colw + 64 * g + 4 * j]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float b0 = colw + 64 * g + 4 * j + e < N ? bb[e] : 0.f;
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t][g][e] = f4{b0, b0, b0, b0};
    }
  }

  const int ngv = min(G, max(0, (N - colw + 63) / 64));  // groups with a column < N
  const int arow0 = wr * 16 * RT + j;
  f4 w0[8], w1[8];
  issue_a(0);
  if constexpr (!FX) {
    if (ngv > 0) load_w(0, 0, w0);
  }
  // (tp in the group forms below: the packed K tail, mfma6)
  auto group = [&](int c, int g, const bf8 (&ap)[RT][3], const f4 (&w)[8], f4 (&wn)[8], auto tp) {
    constexpr bool TPC = decltype(tp)::value;
    // prefetch the next group (or the next chunk's first) into the other set
    if (g + 1 < ngv) load_w(c, g + 1, wn);
    else if (c + 1 < Kc && ngv > 0) load_w(c + 1, 0, wn);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f8 y = {w[0][e], w[1][e], w[2][e], w[3][e], w[4][e], w[5][e], w[6][e], w[7][e]};
      bf8 b0, b1, b2;
      split3(y, b0, b1, b2);
#pragma unroll
      for (int t = 0; t < RT; ++t)
        acc[t][g][e] = mfma6<TPC>(ap[t], b0, b1, b2, acc[t][g][e]);
    }
  };
  // SB = 1 (one W register set, for tiles whose accumulators leave no room for two): the next
  // group's loads go into the set as soon as its last column slot is split, so they fly during
  // that slot's MFMAs and the other waves' work
  auto group_sb = [&](int c, int g, const bf8 (&ap)[RT][3], f4 (&w)[8], auto tp) {
    constexpr bool TPC = decltype(tp)::value;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f8 y = {w[0][e], w[1][e], w[2][e], w[3][e], w[4][e], w[5][e], w[6][e], w[7][e]};
      bf8 b0, b1, b2;
      split3(y, b0, b1, b2);
      if (e == 3) {
        if (g + 1 < ngv) load_w(c, g + 1, w);
        else if (c + 1 < Kc && ngv > 0) load_w(c + 1, 0, w);
      }
#pragma unroll
      for (int t = 0; t < RT; ++t)
        acc[t][g][e] = mfma6<TPC>(ap[t], b0, b1, b2, acc[t][g][e]);
    }
  };
  // FX = 1: W's bf16 planes pre-split into a workspace [BN][Kc][3][32] (split3_rows_kernel, zero
  // past N): per group and chunk 12 loads of 16 B (4 column slots x 3 planes) and no split; the
  // slot's column n = colw + 64 g + e + 4 j gives the scalar part (colw + 64 g + e) * Kc * 192
  // layout (split3_rows_kernel, n_out = BN): [c][plane][BN / 64][e][j][q], 16 B per (j, q)
  const int wlane = 64 * j + 16 * q;
  constexpr int NG64 = BN / 64;
  // the 3 planes of slot e (columns colw + 64 g + e + 4 j) of one chunk and group
  auto load_slot = [&](int chunk, int g, int e, f4 (&wp)[12]) {
    // one chunk = 3 planes x NG64 groups x 4 slots x 1024 B
    const auto rs = brsrc(Wsplit + chunk * 3 * NG64 * 1024, (Kc - chunk) * 3 * NG64 * 4096);
    const int gq = colw / 64 + g;
#pragma unroll
    for (int p = 0; p < 3; ++p)
      wp[3 * e + p] = __builtin_bit_cast(
          f4, __builtin_amdgcn_raw_buffer_load_b128(rs, wlane, ((p * NG64 + gq) * 4 + e) * 1024, 0));
  };
  auto load_p = [&](int chunk, int g, f4 (&wp)[12]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) load_slot(chunk, g, e, wp);
  };
  // one register set, refilled slot by slot: once slot e's MFMAs are issued its registers take
  // the next group's (or the next chunk's first group's) slot e, so each load has three slots
  // of MFMAs (and the other waves' work) to land in
  auto group_fx = [&](int c, int g, const bf8 (&ap)[RT][3], f4 (&wp)[12], auto tp) {
    constexpr bool TPC = decltype(tp)::value;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bf8 b0 = __builtin_bit_cast(bf8, wp[3 * e]);
      const bf8 b1 = __builtin_bit_cast(bf8, wp[3 * e + 1]);
      const bf8 b2 = __builtin_bit_cast(bf8, wp[3 * e + 2]);
#pragma unroll
      for (int t = 0; t < RT; ++t)
        acc[t][g][e] = mfma6<TPC>(ap[t], b0, b1, b2, acc[t][g][e]);
      if (g + 1 < ngv) load_slot(c, g + 1, e, wp);
      else if (c + 1 < Kc && ngv > 0) load_slot(c + 1, 0, e, wp);
    }
  };
  f4 wpl[FX ? 12 : 1];
  // one chunk; wa holds its first group's W on entry. G even: the next chunk's first group
  // ends in wa again, G odd (G = 1, 3): in wb, so the loop alternates the sets (a wave whose
  // live-group count has the other parity -- it straddles N -- moves it)
  auto chunk = [&](int c, f4 (&wa)[8], f4 (&wb)[8], auto tp) {
    // A(c) landed. FX with live groups: the last 12 loads issued (this chunk's first group of
    // planes, prefetched by the previous chunk's last group or the prologue) may still fly
    if (FX && ngv > 0) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (and W's prefetch)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (c + 1 < Kc) issue_a(c + 1);
    const int kc0 = 32 * c;
    const float* stage = smem + (c & 1) * STAGE;
    bf8 ap[RT][3];
    if constexpr (CS) {
      // thread (row r = tid / 8, quad kq = tid % 8: k = kc0 + 4 kq .. + 3) splits its 4 floats;
      // MFMA operand position of k: slot q = kq & 3, half kq >> 2 (low: k = 4q + w, high: 16 +
      // 4q + w) -- 8 B of the slot per plane
      const int r = tid >> 3, kq = tid & 7;
      f4 x = *reinterpret_cast<const f4*>(stage + r * 32 + 4 * (kq ^ (r & 7)));
      if (kc0 + 32 > K) {
        const int lim = K - kc0 - 4 * kq;
#pragma unroll
        for (int w = 0; w < 4; ++w) x[w] = w < lim ? x[w] : 0.f;
      }
      f2 lo2 = {x[0], x[1]}, hi2 = {x[2], x[3]};
      unsigned pw[3][2];
      pw[0][0] = split_pair(lo2);
      pw[0][1] = split_pair(hi2);
      pw[1][0] = split_pair(lo2);
      pw[1][1] = split_pair(hi2);
      pw[2][0] = __builtin_bit_cast(unsigned, __builtin_convertvector(lo2, bf2));
      pw[2][1] = __builtin_bit_cast(unsigned, __builtin_convertvector(hi2, bf2));
      const int so = r * 16 + 4 * ((kq & 3) ^ nt_key<4>(r)) + 2 * (kq >> 2);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        using u2v = __attribute__((ext_vector_type(2))) unsigned;
        *reinterpret_cast<u2v*>(smem + OFF_PL + p * PL_FLOATS + so) = u2v{pw[p][0], pw[p][1]};
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int rr = arow0 + 16 * t;
        const int ro = rr * 16 + 4 * (q ^ nt_key<4>(rr));
#pragma unroll
        for (int p = 0; p < 3; ++p)
          ap[t][p] = __builtin_bit_cast(bf8, *reinterpret_cast<const f4*>(smem + OFF_PL + p * PL_FLOATS + ro));
      }
    }
#pragma unroll
    for (int t = 0; t < (CS ? 0 : RT); ++t) {
      const int r = arow0 + 16 * t;
      const f4 lo = *reinterpret_cast<const f4*>(stage + r * 32 + 4 * (q ^ (r & 7)));
      const f4 hi = *reinterpret_cast<const f4*>(stage + r * 32 + 4 * ((4 + q) ^ (r & 7)));
      f8 x = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
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
    auto groups = [&](auto tp) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (g >= ngv) break;  // wave-uniform: groups wholly past N
        if constexpr (FX) {
          group_fx(c, g, ap, wpl, tp);
        } else if constexpr (SB) {
          group_sb(c, g, ap, wa, tp);
        } else if (g % 2 == 0) {
          group(c, g, ap, wa, wb, tp);
        } else {
          group(c, g, ap, wb, wa, tp);
        }
      }
    };
    if constexpr (decltype(tp)::value) {
#pragma unroll
      for (int t = 0; t < RT; ++t) pack_tail_a(ap[t]);
    }
    groups(tp);
    // the last live group (ngv - 1) prefetched the next chunk's first into wb when ngv is odd
    if (!SB && !FX && ngv > 0 && c + 1 < Kc) {
      const bool in_b = (ngv & 1) != 0;
      if constexpr (G % 2 == 0) {
        if (in_b) {
#pragma unroll
          for (int i = 0; i < 8; ++i) wa[i] = wb[i];
        }
      } else {
        if (!in_b) {
#pragma unroll
          for (int i = 0; i < 8; ++i) wb[i] = wa[i];
        }
      }
    }
  };
  if constexpr (FX) {
    if (ngv > 0) load_p(0, 0, wpl);
  }
  const int Kf = TP ? Kc - 1 : Kc;  // full chunks; TP: the last one peeled, packed
  if constexpr (G % 2 == 0 || SB || FX) {
    for (int c = 0; c < Kf; ++c) chunk(c, w0, w1, std::false_type{});
    if constexpr (TP) chunk(Kf, w0, w1, std::true_type{});
  } else {
    for (int c = 0; c < Kf; c += 2) {
      chunk(c, w0, w1, std::false_type{});
      if (c + 1 < Kf) chunk(c + 1, w1, w0, std::false_type{});
    }
    if constexpr (TP) {
      if (Kf & 1) {  // the tail's first group arrived in the second set
#pragma unroll
        for (int i = 0; i < 8; ++i) w0[i] = w1[i];
      }
      chunk(Kf, w0, w1, std::true_type{});
    }
  }
  if (tile_nonfinite<RT, G, FX == 0>(acc, N, colw, j)) {  // f32 semantics (see tile_nonfinite)
    f32_tile<RT, G>(acc, M, N, K, A, lda, row0 + wr * 16 * RT, B, 1, ldb, colw, j, q);
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = colw + 64 * g + 4 * j + e;
        const float b0 = c < N ? sbias[c] : 0.f;
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][g][e][r] += b0;
      }
  }
#define GCG_EPI_BV_READY
#define GCG_EPI_LABELS_LDS
#define GCG_EPI_BIAS_IN_ACC
#define GCG_EPI_NT true
  f4 bv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) bv[g] = *reinterpret_cast<const f4*>(&sbias[colw + 64 * g + 4 * j]);
#include "gemm_epilogue.inc"
#undef GCG_EPI_BV_READY
#undef GCG_EPI_LABELS_LDS
#undef GCG_EPI_BIAS_IN_ACC
#undef GCG_EPI_NT
}

// One wave per row: the row (N <= 256*NV) is read once into registers, then max, sum of
// exp, label logit and first-index argmax, then dlogits / probabilities. In-place safe.
template <int NV>
__global__ __launch_bounds__(256) void softmax_xent_rows_kernel(
    int M, int N, const float* __restrict__ L, int64_t ldl, const int32_t* __restrict__ labels,
    float scale, const float* __restrict__ scale_dev, float* O, int64_t ldo,
    float* __restrict__ loss_rows, float* __restrict__ correct_rows,
    const float* __restrict__ row_w, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float w = row_w != nullptr ? row_w[row] : 1.f;  // target multiplicity (1 if none)
  const float* lrow = L + row * ldl;
  f4 v[NV];
  float m = kNegInf;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 4 * (lane + 64 * i);
    if (vec && c + 3 < N) {
      v[i] = *reinterpret_cast<const f4*>(lrow + c);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = (c + e < N) ? lrow[c + e] : kNegInf;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, v[i][e]);
  }
  m = reduce16_max<64>(m);
  // a label outside [0, N) gets a NaN loss (never a silent wrong class); -1 = no labels
  int y = labels ? labels[row] : -1;
  const bool bad_y = labels != nullptr && (y < 0 || y >= N);
  y = bad_y ? -1 : y;
  float s = 0.f, x = 0.f;
  int a = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * (lane + 64 * i) + e;
      s += expf(v[i][e] - m);
      x += (c == y) ? v[i][e] : 0.f;
      a = (v[i][e] == m && c < a) ? c : a;
    }
  s = reduce16_sum<64>(s);
  x = reduce16_sum<64>(x);
  a = reduce16_min<64>(a);
  if (labels != nullptr && lane == 0) {
    loss_rows[row] = bad_y ? std::numeric_limits<float>::quiet_NaN() : w * ((m + logf(s)) - x);
    if (correct_rows) correct_rows[row] = (!bad_y && a == y) ? w : 0.f;
  }
  if (O == nullptr) return;  // loss / accuracy only
  if (scale_dev != nullptr) scale *= *scale_dev;
  if (labels != nullptr) scale *= w;
  const float inv = 1.0f / s;
  float* orow = O + row * ldo;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 4 * (lane + 64 * i);
    if (c >= N) continue;
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float p = expf(v[i][e] - m) * inv;
      if (labels != nullptr) p = (p - ((c + e) == y ? 1.f : 0.f)) * scale;
      o[e] = p;
    }
    if (vec && c + 3 < N) {
      *reinterpret_cast<f4*>(orow + c) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < N) orow[c + e] = o[e];
    }
  }
}

// ---- Host side ----

// One gemm_fused6_kernel launch over M rows in bands of 16 RT WR, with the packed K tail when
// the last chunk holds <= 16 k. wsp: the weight's pre-split planes (FX = 1), else null.
template <int RT, int G, int WR, int WC, int SB, int FX, int CS>
gcg_status launch_fused6_t(const FusedArgs& a, const unsigned* wsp, hipStream_t st) {
  constexpr int BM = 16 * RT * WR;
  return with_packed_tail(a.K, [&](auto tp) -> gcg_status {
    hipLaunchKernelGGL((gemm_fused6_kernel<RT, G, WR, WC, SB, FX, CS, decltype(tp)::value>),
                       dim3(static_cast<unsigned>((int64_t{a.M} + BM - 1) / BM)), dim3(64 * WR * WC),
                       0, st, a.M, a.N, a.K, a.A, a.lda, a.B, a.ldb, a.bias, a.C, a.ldc, a.labels,
                       a.scale, a.scale_dev, a.loss_rows, a.correct_rows, a.row_w, wsp);
    GCG_HIP_CHECK(hipGetLastError());
    return GCG_OK;
  });
}

// The 32-row form (RT = 2, 4 waves of 64 G columns) at the G that holds N: g in 1..GMAX
template <int FX, int CS, int GMAX>
gcg_status launch_fused6_rows32(int g, const FusedArgs& a, const unsigned* wsp, hipStream_t st) {
  switch (std::min(g, GMAX)) {
    case 1: return launch_fused6_t<2, 1, 1, 4, 0, FX, CS>(a, wsp, st);
    case 2: return launch_fused6_t<2, 2, 1, 4, 0, FX, CS>(a, wsp, st);
    case 3: return launch_fused6_t<2, 3, 1, 4, 0, FX, CS>(a, wsp, st);
    default:
      if constexpr (GMAX >= 4) return launch_fused6_t<2, 4, 1, 4, 0, FX, CS>(a, wsp, st);
      return fail(GCG_ERR_INVALID_ARG, "fused layer: N=%d", a.N);
  }
}

// The fused output layer on the bf16 matrix cores (gemm_fused6_kernel). ws != NULL: the weight's
// planes pre-split into it (FX = 1); tile 3 = 64 rows x 8 waves of 128 columns at N > 768 (the
// planes read once per 64 rows, half the 32-row form's L2 reads), else 32 rows x 4 waves, with
// the A chunk split cooperatively into LDS planes (CS = 1; World 144.5-145.1 -> 152.2-152.8 TF,
// Twitter-US 117-118 -> 120-122, profiles/r05/fused_cooperative_split.jsonl); tile 0 = tile 3;
// tile 1 = the 32-row form at any N with every wave splitting A in registers (bitwise the
// in-register weight split); tile 2 = the 64-row form likewise (N > 768 only). Every CS form is
// bitwise its CS = 0 form. ws == NULL: the weight split in every workgroup's registers, 32 rows x
// 4 waves.
gcg_status launch_fused6(const FusedArgs& a, hipStream_t st, void* ws, int tile) {
  const int g = (a.N + 255) / 256;
  if (ws == nullptr) {
    if (tile != 0)
      return fail(GCG_ERR_INVALID_ARG, "fused layer: tile %d needs the plane workspace", tile);
    return launch_fused6_rows32<0, 0, 4>(g, a, nullptr, st);
  }
  if (tile == 0) tile = 3;
  if (tile == 2 && g != 4)
    return fail(GCG_ERR_INVALID_ARG, "fused layer: the 64-row tile needs N > 768 (N=%d)", a.N);
  const bool wide = g == 4 && tile != 1;
  // the weight's planes for the tile's BN columns
  gcg_status s = launch_split3_rows(a.N, a.K, a.B, 1, a.ldb, wide ? 1024 : 256 * g,
                                    static_cast<unsigned*>(ws), st);
  if (s != GCG_OK) return s;
  const auto* wsp = static_cast<const unsigned*>(ws);
  if (wide && tile == 3) return launch_fused6_t<4, 2, 1, 8, 0, 1, 1>(a, wsp, st);
  if (wide) return launch_fused6_t<4, 2, 1, 8, 0, 1, 0>(a, wsp, st);
  // (the cooperative A split at g = 4 is the 64-row form above: N > 768 with tile 3 is wide)
  if (tile == 3) return launch_fused6_rows32<1, 1, 3>(g, a, wsp, st);
  return launch_fused6_rows32<1, 0, 4>(g, a, wsp, st);
}

// gcg_project_softmax_xent: validation, then the tile of (math, tile).
gcg_status fused_impl(const char* fn, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                      const float* B, int64_t ldb, const float* bias, float* C, int64_t ldc,
                      const int32_t* labels, float scale, const float* scale_dev,
                      float* loss_rows, float* correct_rows, const float* row_w,
                      gcg_stream_t stream, int math, int tile, void* ws = nullptr) {
  gcg_status s;
  if ((s = check_opts(fn, GCG_DENSE_FUSED, math, tile)) != GCG_OK) return s;
  if ((s = check_sizes(fn, "MNK", M, N, K)) != GCG_OK) return s;
  if (N > 1024)
    return fail(GCG_ERR_INVALID_ARG, "%s: N=%lld > 1024 columns per fused row", fn,
                static_cast<long long>(N));
  if ((s = check_dense(fn, A, lda, K, true)) != GCG_OK) return s;
  // B is read as dwordx4 at columns < round4(N): its row stride must cover them.
  if ((s = check_dense(fn, B, ldb, (N + 3) & ~int64_t{3}, true)) != GCG_OK) return s;
  if (!(C == nullptr && labels != nullptr) && (s = check_dense(fn, C, ldc, N, true)) != GCG_OK)
    return s;
  if (labels != nullptr && loss_rows == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: labels given without loss_rows", fn);
  if (row_w != nullptr && !aligned(row_w, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: row_weight not 4-B aligned", fn);
  if (M == 0) return GCG_OK;
  if ((s = check_b_range(fn, K, ldb)) != GCG_OK) return s;
  const FusedArgs a{int(M), int(N), int(K), A, B, bias, lda, ldb, ldc, C,
                    labels, scale, scale_dev, loss_rows, correct_rows, row_w};
  auto st = static_cast<hipStream_t>(stream);
  if (math == GCG_MATH_BF16X6) return launch_fused6(a, st, ws, tile);
  return launch_gemm_fused_f32(a, tile, st);
}

}  // namespace

extern "C" {

int64_t gcg_project_softmax_xent_workspace(int64_t N, int64_t K, int32_t math) {
  if (math != GCG_MATH_BF16X6 || N <= 0 || N > 1024 || K <= 0) return 0;
  return int64_t{1024} * ((K + 31) / 32) * 192;
}

int64_t gcg_project_softmax_xent_bf16x6_workspace(int64_t N, int64_t K) {
  return gcg_project_softmax_xent_workspace(N, K, GCG_MATH_BF16X6);
}

gcg_status gcg_project_softmax_xent(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                                    const float* W, int64_t ldw, const float* bias,
                                    const int32_t* labels, float scale, const float* scale_dev,
                                    float* out, int64_t ldo, float* loss_rows,
                                    float* correct_rows, const float* row_weight, int32_t math,
                                    int32_t tile, void* ws, int64_t ws_bytes,
                                    gcg_stream_t stream) {
  const char* fn = "gcg_project_softmax_xent";
  if (math == GCG_MATH_BF16X6 && ws != nullptr) {  // NULL: the weight split in the loop
    gcg_status s = check_workspace_i64(fn, ws, ws_bytes, gcg_project_softmax_xent_workspace(N, K, math));
    if (s != GCG_OK) return s;
    if (int64_t{1024} * ((K + 31) / 32) * 192 > INT32_MAX) {  // 32-bit plane offsets
      if (tile != 0) return fail(GCG_ERR_INVALID_ARG, "%s: K too large for tile %d", fn, tile);
      ws = nullptr;
    }
  }
  return fused_impl(fn, M, N, K, A, lda, W, ldw, bias, out, ldo, labels, scale, scale_dev,
                    loss_rows, correct_rows, row_weight, stream, math, tile, ws);
}

gcg_status gcg_project_softmax_xent_f32(int64_t M, int64_t N, int64_t K, const float* A,
                                        int64_t lda, const float* W, int64_t ldw,
                                        const float* bias, const int32_t* labels, float scale,
                                        const float* scale_dev, float* out, int64_t ldo,
                                        float* loss_rows, float* correct_rows,
                                        gcg_stream_t stream) {
  return fused_impl("gcg_project_softmax_xent_f32", M, N, K, A, lda, W, ldw, bias, out, ldo,
                    labels, scale, scale_dev, loss_rows, correct_rows, nullptr, stream,
                    GCG_MATH_F32, 0);
}

gcg_status gcg_project_softmax_xent_weighted_f32(int64_t M, int64_t N, int64_t K,
                                                 const float* A, int64_t lda, const float* W,
                                                 int64_t ldw, const float* bias,
                                                 const int32_t* labels, float scale,
                                                 const float* scale_dev, float* out,
                                                 int64_t ldo, float* loss_rows,
                                                 float* correct_rows, const float* row_weight,
                                                 gcg_stream_t stream) {
  return fused_impl("gcg_project_softmax_xent_weighted_f32", M, N, K, A, lda, W, ldw, bias, out,
                    ldo, labels, scale, scale_dev, loss_rows, correct_rows, row_weight, stream,
                    GCG_MATH_F32, 0);
}

gcg_status gcg_project_softmax_xent_weighted_ws_f32(
    int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw,
    const float* bias, const int32_t* labels, float scale, const float* scale_dev, float* out,
    int64_t ldo, float* loss_rows, float* correct_rows, const float* row_weight, void* ws,
    int64_t ws_bytes, gcg_stream_t stream) {
  return gcg_project_softmax_xent(M, N, K, A, lda, W, ldw, bias, labels, scale, scale_dev, out,
                                  ldo, loss_rows, correct_rows, row_weight, GCG_MATH_BF16X6, 0, ws,
                                  ws_bytes, stream);
}

gcg_status gcg_softmax_xent_f32(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                const int32_t* labels, float scale, const float* scale_dev,
                                float* out, int64_t ldo, float* loss_rows, float* correct_rows,
                                gcg_stream_t stream) {
  return gcg_softmax_xent_weighted_f32(M, N, logits, ldl, labels, scale, scale_dev, out, ldo,
                                       loss_rows, correct_rows, nullptr, stream);
}

gcg_status gcg_softmax_xent_weighted_f32(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                         const int32_t* labels, float scale,
                                         const float* scale_dev, float* out, int64_t ldo,
                                         float* loss_rows, float* correct_rows,
                                         const float* row_weight, gcg_stream_t stream) {
  const char* fn = "gcg_softmax_xent_f32";
  if (M < 0 || N <= 0 || M > INT32_MAX || N > 4096)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes M=%lld N=%lld (N <= 4096)", fn,
                static_cast<long long>(M), static_cast<long long>(N));
  gcg_status s;
  if ((s = check_dense(fn, logits, ldl, N, false)) != GCG_OK) return s;
  if (out != nullptr && (s = check_dense(fn, out, ldo, N, false)) != GCG_OK) return s;
  if (labels != nullptr && loss_rows == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: labels given without loss_rows", fn);
  if (out == nullptr && labels == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: nothing to compute (no out, no labels)", fn);
  if (M == 0) return GCG_OK;
  const int vec = (ldl % 4 == 0 && aligned(logits, 16) &&
                   (out == nullptr || (ldo % 4 == 0 && aligned(out, 16)))) ? 1 : 0;
  const int nv = static_cast<int>((N + 255) / 256);
  dim3 grid(static_cast<unsigned>((M + 3) / 4));
  auto st = static_cast<hipStream_t>(stream);
#define GCG_SX_CASE(v)                                                                       \
  if (nv <= v) {                                                                             \
    hipLaunchKernelGGL(softmax_xent_rows_kernel<v>, grid, dim3(256), 0, st, int(M), int(N), \
                       logits, ldl, labels, scale, scale_dev, out, ldo, loss_rows,          \
                       correct_rows, row_weight, vec);                                       \
    GCG_HIP_CHECK(hipGetLastError());                                                        \
    return GCG_OK;                                                                           \
  }
  GCG_SX_CASE(1)
  GCG_SX_CASE(2)
  GCG_SX_CASE(4)
  GCG_SX_CASE(8)
  GCG_SX_CASE(16)
#undef GCG_SX_CASE
  return fail(GCG_ERR_INVALID_ARG, "%s: N too large", fn);
}

}  // extern "C"
