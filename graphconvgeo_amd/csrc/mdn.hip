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
constexpr double kLog2Pi = 1.8378770664093453;                                   // log(2 pi)
constexpr float kLog2PiF = 1.8378770664093453f, kInv2Pi = 0.15915494309189535f;  // and 0.5 / pi

// ---- the bivariate Gaussian, stated once ----------------------------------------------------
// Each formula of the models below, in T = float or double as its caller computes it: built
// with -ffp-contract=off, an inlined piece rounds as its expression reads (exp(float) is expf).

// softplus in its stable form: max(x, 0) + log1p(exp(-|x|)).
template <typename T>
__device__ __forceinline__ T softplus(T x) {
  return fmax(x, T(0)) + log1p(exp(-fabs(x)));
}

// The sigmoid, softplus's derivative, without overflow on either side.
template <typename T>
__device__ __forceinline__ T sigmoid(T x) {
  const T t = exp(-fabs(x));
  return x >= T(0) ? T(1) / (T(1) + t) : t / (T(1) + t);
}

// rho = softsign(t) and 1 - rho^2 = (1 + 2|t|) / (1 + |t|)^2 from the raw value (no
// cancellation as |rho| -> 1).
template <typename T>
struct Corr {
  T rho, q, inv1;  // inv1 = 1 / (1 + |t|); d rho / d t = inv1^2
};
template <typename T>
__device__ __forceinline__ Corr<T> corr_of(T t) {
  const T a = fabs(t);
  const T inv1 = T(1) / (T(1) + a);
  return Corr<T>{t * inv1, (T(1) + T(2) * a) * (inv1 * inv1), inv1};
}

// What depends on a shared component alone, in double: s1, s2 = softplus(raw), rho, q = 1 -
// rho^2 and k = -log(2 pi) - (log s1 + log s2) - 0.5 log q, the row-independent part of e.
// Double because e is: two components that compete for a row have |e| of 30 .. 1e4 there, and
// their responsibilities hang on the difference -- float32 transforms and a float32 e leave
// ulp(|e|) in it.
struct Component {
  double s1, s2, rho, q, k;
};
__device__ __forceinline__ Component component_constants(float r1, float r2, float cor) {
  const double s1 = softplus<double>(r1), s2 = softplus<double>(r2);
  const Corr<double> cr = corr_of<double>(cor);
  return Component{s1, s2, cr.rho, cr.q, (-kLog2Pi - (log(s1) + log(s2))) - 0.5 * log(cr.q)};
}

// z = u1^2 + u2^2 - 2 rho u1 u2 of the scaled differences u_i = d_i / s_i. The caller forms
// the differences: where and in which precision is what the models differ in.
template <typename T>
struct Quad {
  T u1, u2, z;
};
template <typename T>
__device__ __forceinline__ T quad_z(T u1, T u2, T rho) {
  return (u1 * u1 + u2 * u2) - T(2) * rho * (u1 * u2);
}
template <typename T>
__device__ __forceinline__ Quad<T> quad(T d1, T d2, T s1, T s2, T rho) {
  const T u1 = d1 / s1, u2 = d2 / s2;
  return Quad<T>{u1, u2, quad_z(u1, u2, rho)};
}

// The exponent e = -0.5 z / q + k of a shared component (k: component_constants).
__device__ __forceinline__ double exponent(double z, double q, double k) {
  return (-0.5 * z) / q + k;
}

// d e / d (mu1, mu2, s1, s2, rho), in that order, with a_i = (u_i - rho u_j) / q:
//   a_i / s_i, (u_i a_i - 1) / s_i, (u1 u2 + rho (1 - z / q)) / q
template <typename T>
struct GradTerms {
  T d[5];
};
template <typename T>
__device__ __forceinline__ GradTerms<T> grad_terms(Quad<T> t, T s1, T s2, T rho, T q) {
  const T a1 = (t.u1 - rho * t.u2) / q, a2 = (t.u2 - rho * t.u1) / q;
  return GradTerms<T>{{a1 / s1, a2 / s2, (t.u1 * a1 - T(1)) / s1, (t.u2 * a2 - T(1)) / s2,
                       (t.u1 * t.u2 + rho * (T(1) - t.z / q)) / q}};
}

// d parameter / d raw of plane j (mus lat, lon; sigmas lat, lon; corxy) of shared component c:
// 1, sigmoid(raw), 1 / (1 + |raw|)^2.
template <typename T>
__device__ __forceinline__ T chain_factor(int j, int c, const float* __restrict__ sig,
                                          const float* __restrict__ cor) {
  if (j == 2 || j == 3) return sigmoid<T>(sig[2 * c + (j - 2)]);
  if (j == 4) {
    const T inv1 = corr_of<T>(cor[c]).inv1;
    return inv1 * inv1;
  }
  return T(1);
}

// dparams[j][c] = float32(lead * chain_factor_j(c) * (partial of workgroup 0 + 1 + ... in
// order)), the sum and the factor in T: thread per (j, c).
template <typename T>
__device__ __forceinline__ void finish_partials(int C, int groups, const T* __restrict__ partials,
                                                const float* __restrict__ sig,
                                                const float* __restrict__ cor, T lead,
                                                float* __restrict__ dparams) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 5 * C) return;
  T s = T(0);
  for (int g = 0; g < groups; ++g) s = s + partials[static_cast<int64_t>(g) * 5 * C + t];
  const int j = t / C, c = t - j * C;
  dparams[t] = static_cast<float>((lead * chain_factor<T>(j, c, sig, cor)) * s);
}

// The better of two (score, index) candidates: the higher score, the lower index on a tie.
__device__ __forceinline__ void take_better(float& s, int& i, float s2, int i2) {
  if (s2 > s || (s2 == s && i2 < i)) {
    s = s2;
    i = i2;
  }
}

// The best candidate of the wave, in every lane and in the wave's slot.
__device__ __forceinline__ void wave_best(float& s, int& i, int lane, float& slot_s, int& slot_i) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    take_better(s, i, __shfl_xor(s, off), __shfl_xor(i, off));
  if (lane == 0) {
    slot_s = s;
    slot_i = i;
  }
}

// The winner among wave 0's candidate (s, i) and the other waves' slots (ss, si). Every score NaN
// leaves no winner: component 0, in bounds.
__device__ __forceinline__ int winner_of(float s, int i, const float* ss, const int* si, int C) {
  for (int w = 1; w < kWavesPerBlock; ++w) take_better(s, i, ss[w], si[w]);
  return (i >= 0 && i < C) ? i : 0;
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
      // the sigmas are kSigmaScale * softplus here; the shared components' are not scaled
      const float s1 = kSigmaScale * softplus(o[2 * C + c]);
      const float s2 = kSigmaScale * softplus(o[3 * C + c]);
      const Corr<float> k = corr_of(o[4 * C + c]);
      const Quad<float> t = quad(mean_of(o[c], kLatScale, y1).d,
                                 mean_of(o[C + c], kLonScale, y2).d, s1, s2, k.rho);
      // log(2 pi), the log-sigmas and 0.5 log q leave one after another here, not as the
      // shared components' precomputed k: another rounding, kept
      e[i] = ((((-0.5f * t.z) / k.q - kLog2PiF) - (logf(s1) + logf(s2))) - 0.5f * logf(k.q)) +
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
      const Corr<float> k = corr_of(o[4 * C + c]);
      const GradTerms<float> de = grad_terms(quad(m1.d, m2.d, s1, s2, k.rho), s1, s2, k.rho, k.q);
      const float m = -(w * up);  // d loss / d e = -w
      g[c] = m * de.d[0] * m1.dmu;
      g[C + c] = m * de.d[1] * m2.dmu;
      g[2 * C + c] = m * de.d[2] * (kSigmaScale * sigmoid(r1));
      g[3 * C + c] = m * de.d[3] * (kSigmaScale * sigmoid(r2));
      g[4 * C + c] = m * de.d[4] * (k.inv1 * k.inv1);
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

// One workgroup per row. Six planes of the row are staged in LDS once:
//   mu1, mu2, a1 = sqrt(h) / s1, a2 = sqrt(h) / s2 with h = 0.5 / (1 - rho^2), rho,
//   w = pi * (0.5 / pi) / (s1 s2) * sqrt(1 / (1 - rho^2))
// so that the density of component k at x is w_k * exp(-(v1^2 + v2^2 - 2 rho v1 v2)),
// v_i = (x_i - mu_i) a_i -- the reference's expression with the factor -0.5 / (1 - rho^2) moved
// inside the square. Thread t scores the candidates t, t + 256, ...: the sum over k ascending,
// every lane reading the same k (an LDS broadcast). method 1 scores a candidate by its logit.
// The factors and the term are written out here and in mdn_shared_density_kernel, not shared:
// through inlined helpers the vectoriser packs the score loop another way and a row takes 0.5 %
// (helpers for the factors alone) to 6 % (for the term too) longer at C = 900
// (profiles/mdn/refactor_ab.md).
__global__ __launch_bounds__(kBlock) void mdn_predict_kernel(
    int64_t B, int C, const float* __restrict__ O, int64_t ldo, int method,
    int32_t* __restrict__ idx, float* __restrict__ latlon) {
  extern __shared__ float lds[];
  __shared__ float best_s[kWavesPerBlock];
  __shared__ int best_i[kWavesPerBlock];
  float *mu1 = lds, *mu2 = lds + C, *a1 = lds + 2 * C, *a2 = lds + 3 * C;
  float *rho = lds + 4 * C, *wgt = lds + 5 * C;
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
      const Corr<float> k = corr_of(o[4 * C + c]);
      const float qi = 1.0f / k.q;
      const float sh = sqrtf(0.5f * qi);
      mu1[c] = kLatScale * tanhf(o[c]);
      mu2[c] = kLonScale * tanhf(o[C + c]);
      a1[c] = sh / s1;
      a2[c] = sh / s2;
      rho[c] = k.rho;
      // the weight opens (pi * 1 / 2 pi) here, the density table's 1 / 2 pi: another rounding, kept
      wgt[c] = method == 0 ? expf(o[5 * C + c] - m) / sum_pi * kInv2Pi *
                                 ((1.0f / s1) * (1.0f / s2)) * sqrtf(qi)
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
    wave_best(bs, bi, lane, best_s[wave], best_i[wave]);
    __syncthreads();
    if (tid == 0) {
      const int win = winner_of(bs, bi, best_s, best_i, C);
      if (idx != nullptr) idx[r] = win;
      latlon[2 * r] = mu1[win];
      latlon[2 * r + 1] = mu2[win];
    }
    __syncthreads();  // the planes and the slots are rewritten for the next row
  }
}

// B rows of `planes` (6: a raw output, 1: logits or densities) times C columns at stride ld.
gcg_status check_sizes(const char* fn, int64_t B, int64_t C, int64_t ld, int planes) {
  if (B < 0 || B > INT32_MAX || C < 1 || C > kMaxComp)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes B=%lld C=%lld (1 <= C <= %d)", fn,
                static_cast<long long>(B), static_cast<long long>(C), kMaxComp);
  if (ld < planes * C)
    return fail(GCG_ERR_INVALID_ARG, "%s: row stride %lld < %s = %lld", fn,
                static_cast<long long>(ld), planes == 1 ? "C" : "6 C",
                static_cast<long long>(planes * C));
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

// component_constants of every component, once per call: P [5, C] = s1, s2, rho, q, k.
__global__ __launch_bounds__(kBlock) void mdn_shared_prep_kernel(
    int C, const float* __restrict__ sig, const float* __restrict__ cor, double* __restrict__ P) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  const Component comp = component_constants(sig[2 * c], sig[2 * c + 1], cor[c]);
  P[c] = comp.s1;
  P[C + c] = comp.s2;
  P[2 * C + c] = comp.rho;
  P[3 * C + c] = comp.q;
  P[4 * C + c] = comp.k;
}

gcg_status launch_prep(int64_t C, const float* sig, const float* cor, double* P, hipStream_t st) {
  hipLaunchKernelGGL(mdn_shared_prep_kernel, dim3(static_cast<unsigned>((C + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, st, static_cast<int>(C), sig, cor, P);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
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
      const Quad<double> t = quad<double>(y1 - mus[2 * c], y2 - mus[2 * c + 1], P[c], P[C + c],
                                          P[2 * C + c]);  // float32 differences, widened
      return exponent(t.z, P[3 * C + c], P[4 * C + c]) +
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
          const GradTerms<float> de = grad_terms(
              quad(y1 - mus[2 * c], y2 - mus[2 * c + 1], s1, s2, rho), s1, s2, rho, q);
#pragma unroll
          for (int j = 0; j < 5; ++j) acc[j][i] = acc[j][i] + w * de.d[j];
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

// finish_partials in float32 with the NLL's leading factor -scale / B.
__global__ __launch_bounds__(kBlock) void mdn_shared_finish_kernel(
    int64_t B, int C, int groups, const float* __restrict__ partials,
    const float* __restrict__ sig, const float* __restrict__ cor,
    const float* __restrict__ scale_dev, float* __restrict__ dparams) {
  const float up = (scale_dev != nullptr ? *scale_dev : 1.0f) / static_cast<float>(B);
  finish_partials<float>(C, groups, partials, sig, cor, -up, dparams);
}

// Dt[j C + i]: the density of component j at the mean of component i, in mdn_predict_kernel's
// factoring. Workgroup j, threads over the candidates i (consecutive in memory).
__global__ __launch_bounds__(kBlock) void mdn_shared_density_kernel(
    int C, const float* __restrict__ mus, const float* __restrict__ sig,
    const float* __restrict__ cor, float* __restrict__ Dt) {
  const int j = blockIdx.x;
  const float s1 = softplus(sig[2 * j]), s2 = softplus(sig[2 * j + 1]);
  const Corr<float> k = corr_of(cor[j]);
  const float qi = 1.0f / k.q;
  const float sh = sqrtf(0.5f * qi);
  const float a1 = sh / s1, a2 = sh / s2;
  // the weight opens 1 / 2 pi here, mdn_predict_kernel's (pi * 1 / 2 pi): another rounding, kept
  const float wgt = kInv2Pi * ((1.0f / s1) * (1.0f / s2)) * sqrtf(qi);
  const float m1 = mus[2 * j], m2 = mus[2 * j + 1];
  for (int i = threadIdx.x; i < C; i += kBlock) {
    const float v1 = (mus[2 * i] - m1) * a1, v2 = (mus[2 * i + 1] - m2) * a2;
    Dt[static_cast<int64_t>(j) * C + i] = wgt * expf(-quad_z(v1, v2, k.rho));
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
    wave_best(bs, bi, lane, best_s[t][wave], best_i[t][wave]);
  }
  __syncthreads();
  if (tid < rows) {
    const int win = winner_of(best_s[tid][0], best_i[tid][0], best_s[tid], best_i[tid], C);
    const int64_t r = r0 + tid;
    if (idx != nullptr) idx[r] = win;
    latlon[2 * r] = mus[2 * win];
    latlon[2 * r + 1] = mus[2 * win + 1];
  }
}

// The workspace of gcg_mdn_shared_nll_f32: P [5, C] doubles, the partials [groups, 5, C], B row
// losses.
size_t shared_nll_bytes(int64_t B, int64_t C) {
  return sizeof(float) * static_cast<size_t>((2 * kSharedPlanes + 5 * shared_groups(B)) * C + B);
}

// ---- the Gaussian layer of the inverse model (loc2lang.py:174; lasagne_layers.py:156-214) ---
// The shared-component model's Gaussians as a layer: G[r][c] = the density of component c at the
// coordinate of row r, and the gradient of the five parameter planes from an upstream dG.

// One (row, component) in double. The difference x - mu is formed in double too (two float32
// values: exact), so that a parameter's sum over the rows keeps its meaning when an upstream dG
// of either sign makes the rows cancel -- under the NLL the weights are responsibilities, all
// positive, and float32 terms do (mdn_shared_nll_kernel).
__device__ __forceinline__ Quad<double> bigaus_quad(const float* __restrict__ X, int64_t r,
                                                    float m1, float m2, const Component& comp) {
  return quad(static_cast<double>(X[2 * r]) - static_cast<double>(m1),
              static_cast<double>(X[2 * r + 1]) - static_cast<double>(m2), comp.s1, comp.s2,
              comp.rho);
}

constexpr int kLayerRows = 8;  // rows per workgroup of the forward

// Thread t of workgroup (bx, by) owns component c = bx * 256 + t: its component_constants
// once, then the row tiles by, by + gridDim.y, ... of 8 rows each. X is a broadcast load, G a
// coalesced store; a value depends on its row and component alone. exp is double and G is
// rounded once.
__global__ __launch_bounds__(kBlock) void bigaus_layer_kernel(
    int64_t B, int C, const float* __restrict__ X, const float* __restrict__ mus,
    const float* __restrict__ sig, const float* __restrict__ cor, float* __restrict__ G,
    int64_t ldg) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  const Component comp = component_constants(sig[2 * c], sig[2 * c + 1], cor[c]);
  const float m1 = mus[2 * c], m2 = mus[2 * c + 1];
  for (int64_t r0 = static_cast<int64_t>(blockIdx.y) * kLayerRows; r0 < B;
       r0 += static_cast<int64_t>(gridDim.y) * kLayerRows) {
    const int64_t stop = std::min<int64_t>(r0 + kLayerRows, B);
    for (int64_t r = r0; r < stop; ++r)
      G[r * ldg + c] =
          static_cast<float>(exp(exponent(bigaus_quad(X, r, m1, m2, comp).z, comp.q, comp.k)));
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
    const Component comp{P[c], P[C + c], P[2 * C + c], P[3 * C + c], P[4 * C + c]};
    const float m1 = mus[2 * c], m2 = mus[2 * c + 1];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = r0; r < r1; ++r) {
      const Quad<double> t = bigaus_quad(X, r, m1, m2, comp);
      const double w = static_cast<double>(dG[r * lddg + c]) * exp(exponent(t.z, comp.q, comp.k));
      const GradTerms<double> de = grad_terms(t, comp.s1, comp.s2, comp.rho, comp.q);
#pragma unroll
      for (int j = 0; j < 5; ++j) acc[j] = acc[j] + w * de.d[j];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) out[j * C + c] = acc[j];
  }
}

// finish_partials in double with the layer's leading factor, scale.
__global__ __launch_bounds__(kBlock) void bigaus_layer_finish_kernel(
    int C, int groups, const double* __restrict__ partials, const float* __restrict__ sig,
    const float* __restrict__ cor, const float* __restrict__ scale_dev,
    float* __restrict__ dparams) {
  finish_partials<double>(C, groups, partials, sig, cor,
                          scale_dev != nullptr ? static_cast<double>(*scale_dev) : 1.0, dparams);
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
  if (gcg_status s = check_sizes(fn, B, C, ldo, 6)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, ldo, 6)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, ldo, 6)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, C, 1)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, ldl, 1)) return s;
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
  if (gcg_status s = launch_prep(C, sigmas_raw, corxy_raw, P, st)) return s;
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
  if (gcg_status s = check_sizes(fn, 0, C, C, 1)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, ldl, 1)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, ldg, 1)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, C, 1)) return s;
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
  if (gcg_status s = check_sizes(fn, B, C, lddg, 1)) return s;
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
  if (gcg_status s = launch_prep(C, sigmas_raw, corxy_raw, P, st)) return s;
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
