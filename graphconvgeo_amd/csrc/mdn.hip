// mdn.hip -- the mixture-density location head (reference lang2loc.py:143-244): a row of
// 6 * C raw outputs read as a mixture of C bivariate Gaussians over (lat, lon). The fused
// negative log-likelihood with its gradient, the reference's "mixture" / "pi" prediction rule,
// and the transform of the raw outputs into (mus, sigmas, corxy, pis) the two are built from.
// Below them the shared-component model (lang2loc_mdnshared.py) and, on its components, the
// Gaussian layer of the inverse model (loc2lang.py) with its parameter gradients.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

using namespace gcg;

namespace {

constexpr int kMaxComp = 1024;
constexpr float kLatScale = 90.0f, kLonScale = 180.0f, kSigmaScale = 10.0f;
constexpr float kLog2Pi = 1.8378770664093453f;   // log(2 pi)
constexpr float kInv2Pi = 0.15915494309189535f;  // 0.5 / pi

// ---- the transforms of one component (lang2loc.py:143-160) ----------------------------------

// softplus in its stable form: max(x, 0) + log1p(exp(-|x|)).
__device__ __forceinline__ float softplus(float x) {
  return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
}

// The sigmoid, softplus's derivative, without overflow on either side.
__device__ __forceinline__ float sigmoid(float x) {
  const float t = expf(-fabsf(x));
  return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
}

// rho = softsign(t) and 1 - rho^2 = (1 + 2|t|) / (1 + |t|)^2 from the raw value (no
// cancellation as |rho| -> 1).
struct Corr {
  float rho, q, inv1;  // inv1 = 1 / (1 + |t|); d rho / d t = inv1^2
};
__device__ __forceinline__ Corr corr_of(float t) {
  const float a = fabsf(t);
  const float inv1 = 1.0f / (1.0f + a);
  return Corr{t * inv1, (1.0f + 2.0f * a) * (inv1 * inv1), inv1};
}

// Butterfly reductions over the wave: the same order for every lane, every launch.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

// The two halves of a log-sum-exp, kept apart: logsumexp = max + log(sum), while a softmax
// weight is exp(x - max) / sum -- formed from the sum, it does not inherit the rounding of
// max + log(sum) at the magnitude of max (|e| reaches 1e4 where a sigma is small).
struct Lse {
  float max, sum;
};

// Of a lane's N values across the wave (inactive slots hold -inf).
template <int N>
__device__ __forceinline__ Lse wave_lse(const float (&x)[N]) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < N; ++i) m = fmaxf(m, x[i]);
  m = wave_max(m);
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < N; ++i) s = s + expf(x[i] - m);
  return Lse{m, wave_sum(s)};
}

// A mean against its target: d = y - S tanh(x) and d mu / d x = S (1 - tanh(x)^2). The one
// place that leaves float32: |mu| reaches 180, so mu rounded to float32 is off by up to 8e-6,
// and y - mu amplifies that without bound as the mean closes in on its target -- which is where
// training takes it. tanh and the difference are formed in double and rounded once.
struct Mean {
  float d, dmu;
};
__device__ __forceinline__ Mean mean_of(float x, float S, float y) {
  const double t = tanh(static_cast<double>(x));
  return Mean{static_cast<float>(static_cast<double>(y) - static_cast<double>(S) * t),
              static_cast<float>(static_cast<double>(S) * (1.0 - t * t))};
}

// ---- NLL and gradient -----------------------------------------------------------------------

// One wave per row; lane l owns the components l, l + 64, ... (N = ceil(C / 64) of them), so
// each of the six planes is read coalesced. Pass 1 forms e_c (kept in registers), the
// log-sum-exp gives the row's loss, pass 2 re-reads the row (cache-resident) and writes the
// gradient of (upstream / B) * loss_r with respect to every raw output.
template <int N>
__global__ __launch_bounds__(kBlock) void mdn_nll_kernel(
    int64_t B, int C, const float* __restrict__ O, int64_t ldo, const float* __restrict__ Y,
    const float* __restrict__ scale_dev, float* __restrict__ dO, int64_t ldd,
    float* __restrict__ loss_rows) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* o = O + r * ldo;
  const float y1 = Y[2 * r], y2 = Y[2 * r + 1];

  float lg[N], e[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * kWave;
    lg[i] = c < C ? o[5 * C + c] : -INFINITY;
  }
  const Lse lp = wave_lse<N>(lg);
  const float log_sum_pi = logf(lp.sum);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * kWave;
    e[i] = -INFINITY;
    if (c < C) {
      const float s1 = kSigmaScale * softplus(o[2 * C + c]);
      const float s2 = kSigmaScale * softplus(o[3 * C + c]);
      const Corr k = corr_of(o[4 * C + c]);
      const float u1 = mean_of(o[c], kLatScale, y1).d / s1;
      const float u2 = mean_of(o[C + c], kLonScale, y2).d / s2;
      const float z = (u1 * u1 + u2 * u2) - 2.0f * k.rho * (u1 * u2);
      e[i] = ((((-0.5f * z) / k.q - kLog2Pi) - (logf(s1) + logf(s2))) - 0.5f * logf(k.q)) +
             ((lg[i] - lp.max) - log_sum_pi);
    }
  }
  const Lse le = wave_lse<N>(e);
  if (lane == 0 && loss_rows != nullptr) loss_rows[r] = -(le.max + logf(le.sum));
  if (dO == nullptr) return;

  const float up = (scale_dev != nullptr ? *scale_dev : 1.0f) / static_cast<float>(B);
  float* g = dO + r * ldd;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * kWave;
    if (c < C) {
      const float w = expf(e[i] - le.max) / le.sum;  // the component's responsibility
      const float pi = expf(lg[i] - lp.max) / lp.sum;
      const Mean m1 = mean_of(o[c], kLatScale, y1), m2 = mean_of(o[C + c], kLonScale, y2);
      const float r1 = o[2 * C + c], r2 = o[3 * C + c];
      const float s1 = kSigmaScale * softplus(r1), s2 = kSigmaScale * softplus(r2);
      const Corr k = corr_of(o[4 * C + c]);
      const float u1 = m1.d / s1, u2 = m2.d / s2;
      const float z = (u1 * u1 + u2 * u2) - 2.0f * k.rho * (u1 * u2);
      const float a1 = (u1 - k.rho * u2) / k.q, a2 = (u2 - k.rho * u1) / k.q;
      // d e / d mu_i = a_i / s_i, d e / d s_i = (u_i a_i - 1) / s_i,
      // d e / d rho = (u1 u2 + rho (1 - z / q)) / q; d loss / d e = -w
      const float m = -(w * up);
      g[c] = m * (a1 / s1) * m1.dmu;
      g[C + c] = m * (a2 / s2) * m2.dmu;
      g[2 * C + c] = m * ((u1 * a1 - 1.0f) / s1) * (kSigmaScale * sigmoid(r1));
      g[3 * C + c] = m * ((u2 * a2 - 1.0f) / s2) * (kSigmaScale * sigmoid(r2));
      g[4 * C + c] = m * ((u1 * u2 + k.rho * (1.0f - z / k.q)) / k.q) * (k.inv1 * k.inv1);
      g[5 * C + c] = (pi - w) * up;
    }
  }
}

// *loss = (sum of rows in a fixed order) / B: thread t adds rows t, t + 256, ... in order, then
// a halving tree over the 256 partials. One workgroup, no atomics.
__global__ __launch_bounds__(256) void mdn_mean_kernel(int64_t B, const float* __restrict__ rows,
                                                       float* __restrict__ loss) {
  __shared__ float part[256];
  float s = 0.0f;
  for (int64_t r = threadIdx.x; r < B; r += 256) s = s + rows[r];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (static_cast<int>(threadIdx.x) < h) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = part[0] / static_cast<float>(B);
}

// ---- the four arrays of f_predict -----------------------------------------------------------

// One wave per row: mus [B, 2, C], sigmas [B, 2, C], corxy [B, C], pis [B, C], contiguous, with
// the device functions the two kernels beside it use.
template <int N>
__global__ __launch_bounds__(kBlock) void mdn_unpack_kernel(
    int64_t B, int C, const float* __restrict__ O, int64_t ldo, float* __restrict__ mus,
    float* __restrict__ sigmas, float* __restrict__ corxy, float* __restrict__ pis) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* o = O + r * ldo;
  float lg[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * kWave;
    lg[i] = c < C ? o[5 * C + c] : -INFINITY;
  }
  const Lse lp = wave_lse<N>(lg);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = lane + i * kWave;
    if (c < C) {
      mus[(2 * r) * C + c] = kLatScale * tanhf(o[c]);
      mus[(2 * r + 1) * C + c] = kLonScale * tanhf(o[C + c]);
      sigmas[(2 * r) * C + c] = kSigmaScale * softplus(o[2 * C + c]);
      sigmas[(2 * r + 1) * C + c] = kSigmaScale * softplus(o[3 * C + c]);
      corxy[r * C + c] = corr_of(o[4 * C + c]).rho;
      pis[r * C + c] = expf(lg[i] - lp.max) / lp.sum;
    }
  }
}

// ---- prediction -----------------------------------------------------------------------------

// The better of two (score, index) candidates: the higher score, the lower index on a tie.
__device__ __forceinline__ void take_better(float& s, int& i, float s2, int i2) {
  if (s2 > s || (s2 == s && i2 < i)) {
    s = s2;
    i = i2;
  }
}

// One workgroup per row. Six planes of the row are staged in LDS once:
//   mu1, mu2, a1 = sqrt(h) / s1, a2 = sqrt(h) / s2 with h = 0.5 / (1 - rho^2), rho,
//   w = pi * (0.5 / pi) / (s1 s2) * sqrt(1 / (1 - rho^2))
// so that the density of component k at x is w_k * exp(-(v1^2 + v2^2 - 2 rho v1 v2)),
// v_i = (x_i - mu_i) a_i -- the reference's expression with the factor -0.5 / (1 - rho^2) moved
// inside the square. Thread t scores the candidates t, t + 256, ...: the sum over k ascending,
// every lane reading the same k (an LDS broadcast). method 1 scores a candidate by its logit.
__global__ __launch_bounds__(kBlock) void mdn_predict_kernel(
    int64_t B, int C, const float* __restrict__ O, int64_t ldo, int method,
    int32_t* __restrict__ idx, float* __restrict__ latlon) {
  extern __shared__ float lds[];
  __shared__ float best_s[kWavesPerBlock];
  __shared__ int best_i[kWavesPerBlock];
  float* mu1 = lds;
  float* mu2 = lds + C;
  float* a1 = lds + 2 * C;
  float* a2 = lds + 3 * C;
  float* rho = lds + 4 * C;
  float* wgt = lds + 5 * C;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  for (int64_t r = blockIdx.x; r < B; r += gridDim.x) {
    const float* o = O + r * ldo;
    // the softmax of the logits over the workgroup: max, then the sum
    float m = -INFINITY;
    for (int c = tid; c < C; c += kBlock) m = fmaxf(m, o[5 * C + c]);
    m = wave_max(m);
    if (lane == 0) best_s[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(best_s[0], best_s[1]), fmaxf(best_s[2], best_s[3]));
    __syncthreads();
    float s = 0.0f;
    for (int c = tid; c < C; c += kBlock) s = s + expf(o[5 * C + c] - m);
    s = wave_sum(s);
    if (lane == 0) best_s[wave] = s;
    __syncthreads();
    const float sum_pi = (best_s[0] + best_s[1]) + (best_s[2] + best_s[3]);
    for (int c = tid; c < C; c += kBlock) {
      const float s1 = kSigmaScale * softplus(o[2 * C + c]);
      const float s2 = kSigmaScale * softplus(o[3 * C + c]);
      const Corr k = corr_of(o[4 * C + c]);
      const float qi = 1.0f / k.q;
      const float sh = sqrtf(0.5f * qi);
      mu1[c] = kLatScale * tanhf(o[c]);
      mu2[c] = kLonScale * tanhf(o[C + c]);
      a1[c] = sh / s1;
      a2[c] = sh / s2;
      rho[c] = k.rho;
      wgt[c] = method == 0 ? expf(o[5 * C + c] - m) / sum_pi * kInv2Pi * ((1.0f / s1) * (1.0f / s2)) * sqrtf(qi)
                           : o[5 * C + c];
    }
    __syncthreads();
    float bs = -INFINITY;
    int bi = INT32_MAX;
    for (int c = tid; c < C; c += kBlock) {
      float score;
      if (method == 0) {
        const float x1 = mu1[c], x2 = mu2[c];
        score = 0.0f;
        for (int k = 0; k < C; ++k) {
          const float v1 = (x1 - mu1[k]) * a1[k], v2 = (x2 - mu2[k]) * a2[k];
          const float z = (v1 * v1 + v2 * v2) - 2.0f * rho[k] * (v1 * v2);
          score = score + wgt[k] * expf(-z);
        }
      } else {
        score = wgt[c];
      }
      take_better(bs, bi, score, c);  // ascending c: a later equal score never replaces
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      take_better(bs, bi, __shfl_xor(bs, off), __shfl_xor(bi, off));
    if (lane == 0) {
      best_s[wave] = bs;
      best_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kWavesPerBlock; ++w) take_better(bs, bi, best_s[w], best_i[w]);
      // every score NaN leaves no winner: component 0, in bounds
      const int win = (bi >= 0 && bi < C) ? bi : 0;
      if (idx != nullptr) idx[r] = win;
      latlon[2 * r] = mu1[win];
      latlon[2 * r + 1] = mu2[win];
    }
    __syncthreads();  // the planes and the slots are rewritten for the next row
  }
}

gcg_status check_layout(const char* fn, int64_t B, int64_t C, int64_t ldo) {
  if (B < 0 || B > INT32_MAX || C < 1 || C > kMaxComp)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes B=%lld C=%lld (1 <= C <= %d)", fn,
                static_cast<long long>(B), static_cast<long long>(C), kMaxComp);
  if (ldo < 6 * C)
    return fail(GCG_ERR_INVALID_ARG, "%s: row stride %lld < 6 C = %lld", fn,
                static_cast<long long>(ldo), static_cast<long long>(6 * C));
  return GCG_OK;
}

unsigned row_blocks(int64_t B) {
  return static_cast<unsigned>((B + kWavesPerBlock - 1) / kWavesPerBlock);
}

// N = components per lane, rounded up to a power of two (register arrays of that size).
#define GCG_MDN_DISPATCH(C, LAUNCH)      \
  do {                                   \
    if ((C) <= 64) LAUNCH(1);            \
    else if ((C) <= 128) LAUNCH(2);      \
    else if ((C) <= 256) LAUNCH(4);      \
    else if ((C) <= 512) LAUNCH(8);      \
    else LAUNCH(16);                     \
  } while (0)

// ---- the shared-component model (lang2loc_mdnshared.py:306-327, 379-414, 482-487) -----------
// One set of C Gaussians for the whole model: mus [C, 2] raw, sigmas = softplus(raw [C, 2]),
// rho = softsign(raw [C]); the network only gives the mixture logits L [B, C].

constexpr int kSharedPlanes = 5;     // s1, s2, rho, q, k of every component, in double
constexpr int kSharedRowsMin = 4;    // rows per workgroup: one per wave ...
constexpr int kSharedMaxGroups = 512;  // ... until the grid would pass two workgroups per CU

// Rows per workgroup: a multiple of the waves, a function of B alone.
int64_t shared_rows_per_group(int64_t B) {
  const int64_t per = kSharedRowsMin * kSharedMaxGroups;
  return kSharedRowsMin * std::max<int64_t>(1, (B + per - 1) / per);
}
int64_t shared_groups(int64_t B) {
  const int64_t R = shared_rows_per_group(B);
  return (B + R - 1) / R;
}

// What depends on the component alone, once per call, in double: P [5, C] = s1, s2, rho, q and
//   k = -log(2 pi) - (log s1 + log s2) - 0.5 log q, the row-independent part of e.
// Double because e is: two components that compete for a row have |e| of 30 .. 1e4 there, and
// their responsibilities hang on the difference -- float32 transforms and a float32 e leave
// ulp(|e|) in it.
__global__ __launch_bounds__(kBlock) void mdn_shared_prep_kernel(
    int C, const float* __restrict__ sig, const float* __restrict__ cor, double* __restrict__ P) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  const double r1 = sig[2 * c], r2 = sig[2 * c + 1], a = fabs(static_cast<double>(cor[c]));
  const double s1 = fmax(r1, 0.0) + log1p(exp(-fabs(r1)));
  const double s2 = fmax(r2, 0.0) + log1p(exp(-fabs(r2)));
  const double inv1 = 1.0 / (1.0 + a);
  const double q = (1.0 + 2.0 * a) * (inv1 * inv1);
  P[c] = s1;
  P[C + c] = s2;
  P[2 * C + c] = cor[c] * inv1;
  P[3 * C + c] = q;
  P[4 * C + c] = (-1.8378770664093453 - (log(s1) + log(s2))) - 0.5 * log(q);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// Workgroup g walks the rows [g R, (g + 1) R), wave w of it the rows g R + w (R / 4) ... in
// order, one row at a time with the lanes across the components as in mdn_nll_kernel: loss_rows
// and dL are per-row work. e is formed in double from the float32 difference y - mu and the
// double constants, its maximum M over the row taken in double, and x = e - M rounded to
// float32 (evaluated twice rather than kept: 16 doubles per lane at C = 1024); everything after
// -- exp, the sums, the gradient terms -- is float32. Each lane keeps the five sums of its
// components over its wave's rows in registers (row order); the waves add theirs into LDS in
// wave order (((w0 + w1) + w2) + w3) and the workgroup writes one [5, C] partial. The factors
// that depend on the component alone are left to mdn_shared_finish_kernel.
template <int N>
__global__ __launch_bounds__(kBlock) void mdn_shared_nll_kernel(
    int64_t B, int C, int64_t R, const float* __restrict__ L, int64_t ldl,
    const float* __restrict__ Y, const float* __restrict__ mus, const double* __restrict__ P,
    const float* __restrict__ scale_dev, float* __restrict__ dL, int64_t lddl,
    float* __restrict__ partials, float* __restrict__ loss_rows) {
  extern __shared__ float lds[];  // [5, C]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t per_wave = R / kWavesPerBlock;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * R + wave * per_wave;
  const int64_t r1 = std::min<int64_t>(r0 + per_wave, B);
  const bool want_grad = dL != nullptr || partials != nullptr;
  const float up = (scale_dev != nullptr ? *scale_dev : 1.0f) / static_cast<float>(B);

  float acc[5][N];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int i = 0; i < N; ++i) acc[j][i] = 0.0f;

  for (int64_t r = r0; r < r1; ++r) {
    const float* l = L + r * ldl;
    const float y1 = Y[2 * r], y2 = Y[2 * r + 1];
    float lg[N], x[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = lane + i * kWave;
      lg[i] = c < C ? l[c] : -INFINITY;
    }
    const Lse lp = wave_lse<N>(lg);
    const double log_sum_pi = log(static_cast<double>(lp.sum));
    // e of the lane's i-th component, -inf past C
    auto e_of = [&](int i) -> double {
      const int c = lane + i * kWave;
      if (c >= C) return -INFINITY;
      const double rho = P[2 * C + c];
      const double u1 = static_cast<double>(y1 - mus[2 * c]) / P[c];
      const double u2 = static_cast<double>(y2 - mus[2 * c + 1]) / P[C + c];
      const double z = (u1 * u1 + u2 * u2) - 2.0 * rho * (u1 * u2);
      return ((-0.5 * z) / P[3 * C + c] + P[4 * C + c]) +
             (static_cast<double>(lg[i] - lp.max) - log_sum_pi);
    };
    double M = -INFINITY;
#pragma unroll
    for (int i = 0; i < N; ++i) M = fmax(M, e_of(i));
    M = wave_max(M);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      x[i] = static_cast<float>(e_of(i) - M);
      s = s + expf(x[i]);
    }
    const float sum_e = wave_sum(s);
    if (lane == 0 && loss_rows != nullptr)
      loss_rows[r] = static_cast<float>(-(M + static_cast<double>(logf(sum_e))));
    if (!want_grad) continue;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = lane + i * kWave;
      if (c < C) {
        const float w = expf(x[i]) / sum_e;  // the component's responsibility
        if (dL != nullptr) dL[r * lddl + c] = (expf(lg[i] - lp.max) / lp.sum - w) * up;
        if (partials != nullptr) {
          const float s1 = static_cast<float>(P[c]), s2 = static_cast<float>(P[C + c]);
          const float rho = static_cast<float>(P[2 * C + c]), q = static_cast<float>(P[3 * C + c]);
          const float u1 = (y1 - mus[2 * c]) / s1, u2 = (y2 - mus[2 * c + 1]) / s2;
          const float z = (u1 * u1 + u2 * u2) - 2.0f * rho * (u1 * u2);
          const float a1 = (u1 - rho * u2) / q, a2 = (u2 - rho * u1) / q;
          acc[0][i] = acc[0][i] + w * (a1 / s1);
          acc[1][i] = acc[1][i] + w * (a2 / s2);
          acc[2][i] = acc[2][i] + w * ((u1 * a1 - 1.0f) / s1);
          acc[3][i] = acc[3][i] + w * ((u2 * a2 - 1.0f) / s2);
          acc[4][i] = acc[4][i] + w * ((u1 * u2 + rho * (1.0f - z / q)) / q);
        }
      }
    }
  }
  if (partials == nullptr) return;  // uniform over the workgroup

  for (int w = 0; w < kWavesPerBlock; ++w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const int c = lane + i * kWave;
          if (c < C) lds[j * C + c] = w == 0 ? acc[j][i] : lds[j * C + c] + acc[j][i];
        }
    }
    __syncthreads();
  }
  float* out = partials + static_cast<int64_t>(blockIdx.x) * 5 * C;
  for (int t = threadIdx.x; t < 5 * C; t += kBlock) out[t] = lds[t];
}

// dparams[j][c] = factor_j(c) * (partial of workgroup 0 + 1 + ... in order): thread per (j, c).
//   d mus: -s/B; d sigmas_raw: -s/B * sigmoid(raw); d corxy_raw: -s/B / (1 + |raw|)^2
__global__ __launch_bounds__(kBlock) void mdn_shared_finish_kernel(
    int64_t B, int C, int groups, const float* __restrict__ partials,
    const float* __restrict__ sig, const float* __restrict__ cor,
    const float* __restrict__ scale_dev, float* __restrict__ dparams) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 5 * C) return;
  float s = 0.0f;
  for (int g = 0; g < groups; ++g) s = s + partials[static_cast<int64_t>(g) * 5 * C + t];
  const int j = t / C, c = t - j * C;
  const float up = (scale_dev != nullptr ? *scale_dev : 1.0f) / static_cast<float>(B);
  float f = -up;
  if (j == 2 || j == 3) f = f * sigmoid(sig[2 * c + (j - 2)]);
  if (j == 4) {
    const Corr k = corr_of(cor[c]);
    f = f * (k.inv1 * k.inv1);
  }
  dparams[t] = f * s;
}

// Dt[j C + i]: the density of component j at the mean of component i, in mdn_predict_kernel's
// factoring. Workgroup j, threads over the candidates i (consecutive in memory).
__global__ __launch_bounds__(kBlock) void mdn_shared_density_kernel(
    int C, const float* __restrict__ mus, const float* __restrict__ sig,
    const float* __restrict__ cor, float* __restrict__ Dt) {
  const int j = blockIdx.x;
  const float s1 = softplus(sig[2 * j]), s2 = softplus(sig[2 * j + 1]);
  const Corr k = corr_of(cor[j]);
  const float qi = 1.0f / k.q;
  const float sh = sqrtf(0.5f * qi);
  const float a1 = sh / s1, a2 = sh / s2;
  const float wgt = kInv2Pi * ((1.0f / s1) * (1.0f / s2)) * sqrtf(qi);
  const float m1 = mus[2 * j], m2 = mus[2 * j + 1];
  for (int i = threadIdx.x; i < C; i += kBlock) {
    const float v1 = (mus[2 * i] - m1) * a1, v2 = (mus[2 * i + 1] - m2) * a2;
    const float z = (v1 * v1 + v2 * v2) - 2.0f * k.rho * (v1 * v2);
    Dt[static_cast<int64_t>(j) * C + i] = wgt * expf(-z);
  }
}

constexpr int kPredTile = 4;  // rows per workgroup of the shared prediction

// A workgroup takes kPredTile rows: wave w softmaxes row w of the tile into LDS
// (lanes striding over the components, as the NLL does), then thread t scores the candidates
// t, t + 256, ... (NC of them) of every row of the tile at once: score[row][i] = sum over j
// ascending of pi[row][j] * Dt[j][i], each Dt element read once per tile and pi[row][j] an LDS
// broadcast. A row's numbers do not depend on the tile it falls in. method 1 scores by the logit.
template <int NC>
__global__ __launch_bounds__(kBlock) void mdn_shared_predict_kernel(
    int64_t B, int C, const float* __restrict__ L, int64_t ldl, const float* __restrict__ Dt,
    const float* __restrict__ mus, int method, int32_t* __restrict__ idx,
    float* __restrict__ latlon) {
  extern __shared__ float pis[];  // [kPredTile, C]
  __shared__ float best_s[kPredTile][kWavesPerBlock];
  __shared__ int best_i[kPredTile][kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kPredTile;
  const int rows = static_cast<int>(std::min<int64_t>(kPredTile, B - r0));

  for (int t = wave; t < kPredTile; t += kWavesPerBlock) {
    float* p = pis + t * C;
    if (t >= rows) {  // a short tile: its spare rows score nothing and are not written
      for (int c = lane; c < C; c += kWave) p[c] = 0.0f;
      continue;
    }
    const float* l = L + (r0 + t) * ldl;
    if (method != 0) {
      for (int c = lane; c < C; c += kWave) p[c] = l[c];
      continue;
    }
    float m = -INFINITY;
    for (int c = lane; c < C; c += kWave) m = fmaxf(m, l[c]);
    m = wave_max(m);
    float s = 0.0f;
    for (int c = lane; c < C; c += kWave) s = s + expf(l[c] - m);
    s = wave_sum(s);
    for (int c = lane; c < C; c += kWave) p[c] = expf(l[c] - m) / s;
  }
  __syncthreads();

  float score[kPredTile][NC];
  if (method == 0) {
#pragma unroll
    for (int t = 0; t < kPredTile; ++t)
#pragma unroll
      for (int i = 0; i < NC; ++i) score[t][i] = 0.0f;
#pragma unroll 8
    for (int j = 0; j < C; ++j) {
      float d[NC];
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = tid + i * kBlock;
        d[i] = c < C ? Dt[static_cast<int64_t>(j) * C + c] : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < kPredTile; ++t) {
        const float pj = pis[t * C + j];
#pragma unroll
        for (int i = 0; i < NC; ++i) score[t][i] = score[t][i] + pj * d[i];
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < kPredTile; ++t)
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = tid + i * kBlock;
        score[t][i] = c < C ? pis[t * C + c] : -INFINITY;
      }
  }

#pragma unroll
  for (int t = 0; t < kPredTile; ++t) {
    float bs = -INFINITY;
    int bi = INT32_MAX;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = tid + i * kBlock;
      if (c < C) take_better(bs, bi, score[t][i], c);  // ascending c
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      take_better(bs, bi, __shfl_xor(bs, off), __shfl_xor(bi, off));
    if (lane == 0) {
      best_s[t][wave] = bs;
      best_i[t][wave] = bi;
    }
  }
  __syncthreads();
  if (tid < rows) {
    float bs = best_s[tid][0];
    int bi = best_i[tid][0];
    for (int w = 1; w < kWavesPerBlock; ++w) take_better(bs, bi, best_s[tid][w], best_i[tid][w]);
    // every score NaN leaves no winner: component 0, in bounds
    const int win = (bi >= 0 && bi < C) ? bi : 0;
    const int64_t r = r0 + tid;
    if (idx != nullptr) idx[r] = win;
    latlon[2 * r] = mus[2 * win];
    latlon[2 * r + 1] = mus[2 * win + 1];
  }
}

gcg_status check_shared(const char* fn, int64_t B, int64_t C, int64_t ldl) {
  if (B < 0 || B > INT32_MAX || C < 1 || C > kMaxComp)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes B=%lld C=%lld (1 <= C <= %d)", fn,
                static_cast<long long>(B), static_cast<long long>(C), kMaxComp);
  if (ldl < C)
    return fail(GCG_ERR_INVALID_ARG, "%s: row stride %lld < C = %lld", fn,
                static_cast<long long>(ldl), static_cast<long long>(C));
  return GCG_OK;
}

// The workspace of gcg_mdn_shared_nll_f32: P [5, C] doubles, the partials [groups, 5, C], B row
// losses.
size_t shared_nll_bytes(int64_t B, int64_t C) {
  return sizeof(float) * static_cast<size_t>((2 * kSharedPlanes + 5 * shared_groups(B)) * C + B);
}

// ---- the Gaussian layer of the inverse model (loc2lang.py:174; lasagne_layers.py:156-214) ---
// The shared-component model's Gaussians as a layer: G[r][c] = the density of component c at the
// coordinate of row r, and the gradient of the five parameter planes from an upstream dG.

// One (row, component) in double: the exponent e = -0.5 z / q + k and what the five gradient
// terms are built from. The difference x - mu is formed in double too (two float32 values:
// exact), so that a parameter's sum over the rows keeps its meaning when an upstream dG of
// either sign makes the rows cancel -- under the NLL the weights are responsibilities, all
// positive, and float32 terms do (mdn_shared_nll_kernel).
struct BigausTerm {
  double u1, u2, z, e;
};
__device__ __forceinline__ BigausTerm bigaus_term(float x1, float x2, float m1, float m2,
                                                  double s1, double s2, double rho, double q,
                                                  double k) {
  BigausTerm t;
  t.u1 = (static_cast<double>(x1) - static_cast<double>(m1)) / s1;
  t.u2 = (static_cast<double>(x2) - static_cast<double>(m2)) / s2;
  t.z = (t.u1 * t.u1 + t.u2 * t.u2) - 2.0 * rho * (t.u1 * t.u2);
  t.e = (-0.5 * t.z) / q + k;
  return t;
}

constexpr int kLayerRows = 8;  // rows per workgroup of the forward

// Thread t of workgroup (bx, by) owns component c = bx * 256 + t: its constants once, in double
// and in mdn_shared_prep_kernel's expressions, then the row tiles by, by + gridDim.y, ... of 8
// rows each. X is a broadcast load, G a coalesced store; a value depends on its row and
// component alone. exp is double and G is rounded once.
__global__ __launch_bounds__(kBlock) void bigaus_layer_kernel(
    int64_t B, int C, const float* __restrict__ X, const float* __restrict__ mus,
    const float* __restrict__ sig, const float* __restrict__ cor, float* __restrict__ G,
    int64_t ldg) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  const double r1 = sig[2 * c], r2 = sig[2 * c + 1], a = fabs(static_cast<double>(cor[c]));
  const double s1 = fmax(r1, 0.0) + log1p(exp(-fabs(r1)));
  const double s2 = fmax(r2, 0.0) + log1p(exp(-fabs(r2)));
  const double inv1 = 1.0 / (1.0 + a);
  const double q = (1.0 + 2.0 * a) * (inv1 * inv1);
  const double rho = cor[c] * inv1;
  const double k = (-1.8378770664093453 - (log(s1) + log(s2))) - 0.5 * log(q);
  const float m1 = mus[2 * c], m2 = mus[2 * c + 1];
  for (int64_t r0 = static_cast<int64_t>(blockIdx.y) * kLayerRows; r0 < B;
       r0 += static_cast<int64_t>(gridDim.y) * kLayerRows) {
    const int64_t stop = std::min<int64_t>(r0 + kLayerRows, B);
    for (int64_t r = r0; r < stop; ++r)
      G[r * ldg + c] = static_cast<float>(
          exp(bigaus_term(X[2 * r], X[2 * r + 1], m1, m2, s1, s2, rho, q, k).e));
  }
}

// Workgroup g takes the rows [g R, (g + 1) R) of mdn_shared_nll_kernel's grouping; its thread t
// (of 256) owns the components t, t + 256, ... and adds each one's five terms over the
// workgroup's rows in row order, in double, the weight of a row being dG[r][c] * G[r][c] with G
// recomputed as the forward computes it (P holds the constants mdn_shared_prep_kernel wrote).
// X is a broadcast load, dG a coalesced one. One [5, C] partial of doubles per workgroup; no
// sum crosses a thread here, so there is nothing to add between waves.
__global__ __launch_bounds__(kBlock) void bigaus_layer_backward_kernel(
    int64_t B, int C, int64_t R, const float* __restrict__ X, const float* __restrict__ mus,
    const double* __restrict__ P, const float* __restrict__ dG, int64_t lddg,
    double* __restrict__ partials) {
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * R;
  const int64_t r1 = std::min<int64_t>(r0 + R, B);
  double* out = partials + static_cast<int64_t>(blockIdx.x) * 5 * C;
  for (int c = threadIdx.x; c < C; c += kBlock) {
    const double s1 = P[c], s2 = P[C + c], rho = P[2 * C + c], q = P[3 * C + c];
    const double k = P[4 * C + c];
    const float m1 = mus[2 * c], m2 = mus[2 * c + 1];
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, acc4 = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
      const BigausTerm t = bigaus_term(X[2 * r], X[2 * r + 1], m1, m2, s1, s2, rho, q, k);
      const double w = static_cast<double>(dG[r * lddg + c]) * exp(t.e);
      const double a1 = (t.u1 - rho * t.u2) / q, a2 = (t.u2 - rho * t.u1) / q;
      acc0 = acc0 + w * (a1 / s1);
      acc1 = acc1 + w * (a2 / s2);
      acc2 = acc2 + w * ((t.u1 * a1 - 1.0) / s1);
      acc3 = acc3 + w * ((t.u2 * a2 - 1.0) / s2);
      acc4 = acc4 + w * ((t.u1 * t.u2 + rho * (1.0 - t.z / q)) / q);
    }
    out[c] = acc0;
    out[C + c] = acc1;
    out[2 * C + c] = acc2;
    out[3 * C + c] = acc3;
    out[4 * C + c] = acc4;
  }
}

// dparams[j][c] = float32(factor_j(c) * (partial of workgroup 0 + 1 + ... in order)), the sum and
// the factor in double: thread per (j, c).
//   d mus: s; d sigmas_raw: s * sigmoid(raw); d corxy_raw: s / (1 + |raw|)^2
__global__ __launch_bounds__(kBlock) void bigaus_layer_finish_kernel(
    int C, int groups, const double* __restrict__ partials, const float* __restrict__ sig,
    const float* __restrict__ cor, const float* __restrict__ scale_dev,
    float* __restrict__ dparams) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 5 * C) return;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s = s + partials[static_cast<int64_t>(g) * 5 * C + t];
  const int j = t / C, c = t - j * C;
  double f = scale_dev != nullptr ? static_cast<double>(*scale_dev) : 1.0;
  if (j == 2 || j == 3) {
    const double x = sig[2 * c + (j - 2)], e = exp(-fabs(x));
    f = f * (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));
  }
  if (j == 4) {
    const double inv1 = 1.0 / (1.0 + fabs(static_cast<double>(cor[c])));
    f = f * (inv1 * inv1);
  }
  dparams[t] = static_cast<float>(f * s);
}

// The workspace of gcg_bigaus_layer_backward_f32: P [5, C] and the partials [groups, 5, C], doubles.
size_t bigaus_backward_bytes(int64_t B, int64_t C) {
  return sizeof(double) * static_cast<size_t>((kSharedPlanes + 5 * shared_groups(B)) * C);
}

}  // namespace

extern "C" {

gcg_status gcg_mdn_nll_f32(int64_t B, int64_t C, const float* O, int64_t ldo, const float* Y,
                           const float* scale_dev, float* dO, int64_t ldd, float* loss_rows,
                           float* loss, void* workspace, size_t workspace_bytes,
                           gcg_stream_t stream) {
  const char* fn = "gcg_mdn_nll_f32";
  if (gcg_status s = check_layout(fn, B, C, ldo)) return s;
  if (dO != nullptr && ldd < 6 * C)
    return fail(GCG_ERR_INVALID_ARG, "%s: gradient row stride %lld < 6 C", fn,
                static_cast<long long>(ldd));
  if (B == 0) return GCG_OK;
  if (O == nullptr || Y == nullptr || loss == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(O, 4) || !aligned(Y, 4) || !aligned(dO, 4) || !aligned(loss_rows, 4) ||
      !aligned(loss, 4) || !aligned(scale_dev, 4) || !aligned(workspace, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  float* rows = loss_rows;
  if (rows == nullptr) {  // the row losses the mean is taken of need a home
    if (workspace == nullptr || workspace_bytes < sizeof(float) * static_cast<size_t>(B))
      return fail(GCG_ERR_WORKSPACE, "%s: without loss_rows the workspace holds them: %zu < %zu "
                  "bytes", fn, workspace_bytes, sizeof(float) * static_cast<size_t>(B));
    rows = static_cast<float*>(workspace);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int c = static_cast<int>(C);
#define GCG_MDN_NLL(N)                                                                        \
  hipLaunchKernelGGL((mdn_nll_kernel<N>), dim3(row_blocks(B)), dim3(kBlock), 0, st, B, c, O, \
                     ldo, Y, scale_dev, dO, ldd, rows)
  GCG_MDN_DISPATCH(C, GCG_MDN_NLL);
#undef GCG_MDN_NLL
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mdn_mean_kernel, dim3(1), dim3(256), 0, st, B, rows, loss);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_mdn_unpack_f32(int64_t B, int64_t C, const float* O, int64_t ldo, float* mus,
                              float* sigmas, float* corxy, float* pis, gcg_stream_t stream) {
  const char* fn = "gcg_mdn_unpack_f32";
  if (gcg_status s = check_layout(fn, B, C, ldo)) return s;
  if (B == 0) return GCG_OK;
  if (O == nullptr || mus == nullptr || sigmas == nullptr || corxy == nullptr || pis == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(O, 4) || !aligned(mus, 4) || !aligned(sigmas, 4) || !aligned(corxy, 4) ||
      !aligned(pis, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int c = static_cast<int>(C);
#define GCG_MDN_UNPACK(N)                                                                       \
  hipLaunchKernelGGL((mdn_unpack_kernel<N>), dim3(row_blocks(B)), dim3(kBlock), 0, st, B, c, O, \
                     ldo, mus, sigmas, corxy, pis)
  GCG_MDN_DISPATCH(C, GCG_MDN_UNPACK);
#undef GCG_MDN_UNPACK
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_mdn_predict_f32(int64_t B, int64_t C, const float* O, int64_t ldo, int method,
                               int32_t* idx, float* latlon, gcg_stream_t stream) {
  const char* fn = "gcg_mdn_predict_f32";
  if (gcg_status s = check_layout(fn, B, C, ldo)) return s;
  if (method != 0 && method != 1)
    return fail(GCG_ERR_INVALID_ARG, "%s: method %d is neither 0 (mixture) nor 1 (pi)", fn, method);
  if (B == 0) return GCG_OK;
  if (O == nullptr || latlon == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(O, 4) || !aligned(idx, 4) || !aligned(latlon, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(B, int64_t{1} << 16));
  hipLaunchKernelGGL(mdn_predict_kernel, dim3(grid), dim3(kBlock),
                     sizeof(float) * 6 * static_cast<size_t>(C), static_cast<hipStream_t>(stream),
                     B, static_cast<int>(C), O, ldo, method, idx, latlon);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_mdn_shared_nll_f32_workspace_bytes(int64_t B, int64_t C, size_t* bytes) {
  const char* fn = "gcg_mdn_shared_nll_f32_workspace_bytes";
  if (gcg_status s = check_shared(fn, B, C, C)) return s;
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = shared_nll_bytes(B, C);
  return GCG_OK;
}

gcg_status gcg_mdn_shared_nll_f32(int64_t B, int64_t C, const float* L, int64_t ldl,
                                  const float* Y, const float* mus, const float* sigmas_raw,
                                  const float* corxy_raw, const float* scale_dev, float* dL,
                                  int64_t lddl, float* dparams, float* loss_rows, float* loss,
                                  void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  const char* fn = "gcg_mdn_shared_nll_f32";
  if (gcg_status s = check_shared(fn, B, C, ldl)) return s;
  if (dL != nullptr && lddl < C)
    return fail(GCG_ERR_INVALID_ARG, "%s: gradient row stride %lld < C", fn,
                static_cast<long long>(lddl));
  if (B == 0) return GCG_OK;
  if (L == nullptr || Y == nullptr || mus == nullptr || sigmas_raw == nullptr ||
      corxy_raw == nullptr || loss == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(L, 4) || !aligned(Y, 4) || !aligned(mus, 4) || !aligned(sigmas_raw, 4) ||
      !aligned(corxy_raw, 4) || !aligned(scale_dev, 4) || !aligned(dL, 4) ||
      !aligned(dparams, 4) || !aligned(loss_rows, 4) || !aligned(loss, 4) ||
      !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B (workspace: 8-B) aligned", fn);
  if (workspace == nullptr || workspace_bytes < shared_nll_bytes(B, C))
    return fail(GCG_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes "
                "(gcg_mdn_shared_nll_f32_workspace_bytes)", fn, workspace_bytes,
                shared_nll_bytes(B, C));
  const int c = static_cast<int>(C);
  const int64_t R = shared_rows_per_group(B);
  const int groups = static_cast<int>(shared_groups(B));
  double* P = static_cast<double*>(workspace);
  float* base = static_cast<float*>(workspace) + 2 * kSharedPlanes * C;
  float* partials = dparams != nullptr ? base : nullptr;
  float* rows = loss_rows != nullptr ? loss_rows : base + 5 * static_cast<int64_t>(groups) * C;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned cblocks = static_cast<unsigned>((C + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(mdn_shared_prep_kernel, dim3(cblocks), dim3(kBlock), 0, st, c,
                     sigmas_raw, corxy_raw, P);
  GCG_HIP_CHECK(hipGetLastError());
#define GCG_MDN_SHARED_NLL(N)                                                                  \
  hipLaunchKernelGGL((mdn_shared_nll_kernel<N>), dim3(groups), dim3(kBlock),                   \
                     sizeof(float) * 5 * static_cast<size_t>(C), st, B, c, R, L, ldl, Y, mus,  \
                     P, scale_dev, dL, lddl, partials, rows)
  GCG_MDN_DISPATCH(C, GCG_MDN_SHARED_NLL);
#undef GCG_MDN_SHARED_NLL
  GCG_HIP_CHECK(hipGetLastError());
  if (dparams != nullptr) {
    hipLaunchKernelGGL(mdn_shared_finish_kernel, dim3((5 * c + kBlock - 1) / kBlock),
                       dim3(kBlock), 0, st, B, c, groups, partials, sigmas_raw, corxy_raw,
                       scale_dev, dparams);
    GCG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(mdn_mean_kernel, dim3(1), dim3(256), 0, st, B, rows, loss);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_mdn_shared_density_f32(int64_t C, const float* mus, const float* sigmas_raw,
                                      const float* corxy_raw, float* Dt, gcg_stream_t stream) {
  const char* fn = "gcg_mdn_shared_density_f32";
  if (gcg_status s = check_shared(fn, 0, C, C)) return s;
  if (mus == nullptr || sigmas_raw == nullptr || corxy_raw == nullptr || Dt == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(mus, 4) || !aligned(sigmas_raw, 4) || !aligned(corxy_raw, 4) || !aligned(Dt, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  hipLaunchKernelGGL(mdn_shared_density_kernel, dim3(static_cast<unsigned>(C)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), static_cast<int>(C), mus, sigmas_raw,
                     corxy_raw, Dt);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_mdn_shared_predict_f32(int64_t B, int64_t C, const float* L, int64_t ldl,
                                      const float* Dt, const float* mus, int method,
                                      int32_t* idx, float* latlon, gcg_stream_t stream) {
  const char* fn = "gcg_mdn_shared_predict_f32";
  if (gcg_status s = check_shared(fn, B, C, ldl)) return s;
  if (method != 0 && method != 1)
    return fail(GCG_ERR_INVALID_ARG, "%s: method %d is neither 0 (mixture) nor 1 (pi)", fn, method);
  if (B == 0) return GCG_OK;
  if (L == nullptr || mus == nullptr || latlon == nullptr || (method == 0 && Dt == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(L, 4) || !aligned(Dt, 4) || !aligned(mus, 4) || !aligned(idx, 4) ||
      !aligned(latlon, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const unsigned grid = static_cast<unsigned>((B + kPredTile - 1) / kPredTile);
  const size_t lds = sizeof(float) * kPredTile * static_cast<size_t>(C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int c = static_cast<int>(C);
#define GCG_MDN_SHARED_PREDICT(NC)                                                             \
  hipLaunchKernelGGL((mdn_shared_predict_kernel<NC>), dim3(grid), dim3(kBlock), lds, st, B, c, \
                     L, ldl, Dt, mus, method, idx, latlon)
  if (C <= kBlock) GCG_MDN_SHARED_PREDICT(1);
  else if (C <= 2 * kBlock) GCG_MDN_SHARED_PREDICT(2);
  else GCG_MDN_SHARED_PREDICT(4);
#undef GCG_MDN_SHARED_PREDICT
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_bigaus_layer_f32(int64_t B, int64_t C, const float* X, const float* mus,
                                const float* sigmas_raw, const float* corxy_raw, float* G,
                                int64_t ldg, gcg_stream_t stream) {
  const char* fn = "gcg_bigaus_layer_f32";
  if (gcg_status s = check_shared(fn, B, C, ldg)) return s;
  if (B == 0) return GCG_OK;
  if (X == nullptr || mus == nullptr || sigmas_raw == nullptr || corxy_raw == nullptr ||
      G == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(X, 4) || !aligned(mus, 4) || !aligned(sigmas_raw, 4) || !aligned(corxy_raw, 4) ||
      !aligned(G, 4))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B aligned", fn);
  const unsigned tiles = static_cast<unsigned>(
      std::min<int64_t>((B + kLayerRows - 1) / kLayerRows, 65535));
  hipLaunchKernelGGL(bigaus_layer_kernel,
                     dim3(static_cast<unsigned>((C + kBlock - 1) / kBlock), tiles), dim3(kBlock),
                     0, static_cast<hipStream_t>(stream), B, static_cast<int>(C), X, mus,
                     sigmas_raw, corxy_raw, G, ldg);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

gcg_status gcg_bigaus_layer_backward_f32_workspace_bytes(int64_t B, int64_t C, size_t* bytes) {
  const char* fn = "gcg_bigaus_layer_backward_f32_workspace_bytes";
  if (gcg_status s = check_shared(fn, B, C, C)) return s;
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = bigaus_backward_bytes(B, C);
  return GCG_OK;
}

gcg_status gcg_bigaus_layer_backward_f32(int64_t B, int64_t C, const float* X, const float* mus,
                                         const float* sigmas_raw, const float* corxy_raw,
                                         const float* dG, int64_t lddg, const float* scale_dev,
                                         float* dparams, void* workspace, size_t workspace_bytes,
                                         gcg_stream_t stream) {
  const char* fn = "gcg_bigaus_layer_backward_f32";
  if (gcg_status s = check_shared(fn, B, C, lddg)) return s;
  if (B == 0) return GCG_OK;
  if (X == nullptr || mus == nullptr || sigmas_raw == nullptr || corxy_raw == nullptr ||
      dG == nullptr || dparams == nullptr)
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL operand", fn);
  if (!aligned(X, 4) || !aligned(mus, 4) || !aligned(sigmas_raw, 4) || !aligned(corxy_raw, 4) ||
      !aligned(dG, 4) || !aligned(scale_dev, 4) || !aligned(dparams, 4) || !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: operand not 4-B (workspace: 8-B) aligned", fn);
  if (workspace == nullptr || workspace_bytes < bigaus_backward_bytes(B, C))
    return fail(GCG_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes "
                "(gcg_bigaus_layer_backward_f32_workspace_bytes)", fn, workspace_bytes,
                bigaus_backward_bytes(B, C));
  const int c = static_cast<int>(C);
  const int64_t R = shared_rows_per_group(B);
  const int groups = static_cast<int>(shared_groups(B));
  double* P = static_cast<double*>(workspace);
  double* partials = P + kSharedPlanes * C;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mdn_shared_prep_kernel, dim3(static_cast<unsigned>((C + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, st, c, sigmas_raw, corxy_raw, P);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bigaus_layer_backward_kernel, dim3(groups), dim3(kBlock), 0, st, B, c, R, X,
                     mus, P, dG, lddg, partials);
  GCG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bigaus_layer_finish_kernel, dim3((5 * c + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, st, c, groups, partials, sigmas_raw, corxy_raw, scale_dev,
                     dparams);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
