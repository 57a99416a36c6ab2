// The SMSD mixture-density head's own arithmetic (reference smsd.py:127-164,
// 224-264, 277-292, 295-372): everything between the three linear heads'
// outputs and the loss / the sampled style vector.
//
//   mtts_mdn_params_fwd/bwd   pi = softmax(pi_logits) over K;
//                             sigma = softplus(sigma_raw + noise_scale * eps)
//                             (torch's threshold form: x for x > 20), eps given
//                             or drawn here; backward: d pi_logits, d sigma_raw
//                             and the scalar d noise_scale.
//   mtts_mixture_nll_fwd/bwd  -mean_b logsumexp_k(log(pi_bk + 1e-8) +
//                             log N(y_b | mu_bk, var)), var by mode; the
//                             default mode takes ROW b's variance for every
//                             component of row b (the documented formula; the
//                             reference's (B,) + (B, K) broadcast is not
//                             reproduced).  Backward: d pi, d mu, d sigma, d y.
//   mtts_mixture_sample       k by inverse CDF over pi (k = 0 .. K-1, a
//                             sequential fp32 sum), then mu_k + std * z.
//   mtts_relu_dropout         y = relu(x) * keep / (1 - p) (dropout.hip's mask
//                             and seed plumbing); backward masks by y > 0.
//   mtts_mdn_layernorm_*      the head's input LayerNorm at the widths ln.hip
//                             does not take (any cols).
//
// One 256-thread workgroup per row; fp32 math on fp32 / bf16 I/O read as it is;
// no atomics; every sum in a fixed order (a lane's strided elements in index
// order, the 64-lane butterfly, then the four wave partials left to right), so
// results are bit-identical from run to run and a row's result does not depend
// on the other rows of the launch.  K <= MTTS_MDN_MAX_K, any d >= 1.  The work
// is tiny (rows x K x d with K = 5, d = 256 in train.py), so the loads are
// plain element loads (any d, any alignment), not 16-byte pieces; only
// relu_dropout, which also serves large tensors, moves 16-byte pieces.
//
// Random numbers: counter-based, a function of (row seed, row draw count,
// stream tag, index) alone:
//   key = mix64(seed + draw * golden)
//   n(tag, i) = mix64((key ^ tag * 0xD6E8FEB86659FD93) + i * golden) >> 40
//   u = (n + 0.5) * 2^-24            (the token sampler's uniform, sample.hip)
//   tag 1, i = 0: the component pick, first k with u * total < cdf_k (else K-1)
//   tags 2, 3, i = j: z[2j] = r cos(t), z[2j+1] = r sin(t), r = sqrt(-2 ln u_2),
//                     t = 2 pi u_3 (Box-Muller; |z| <= sqrt(50 ln 2) = 5.89)
//   tags 4, 5: the same for the NoiseNet eps (draw = 0, i over the row's sigma_raw)
// -ln u is taken as in sample.hip (u or 1 - u exact in fp32), with the precise
// logf / log1pf / sqrtf / sincosf.
#include "common.h"

namespace mtts {
namespace {

constexpr int kT = 256;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kTagMul = 0xD6E8FEB86659FD93ull;
enum { kTagComp = 1, kTagZ = 2, kTagEps = 4 };
constexpr float kHalfLog2Pi = 0.9189385332046727f;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's finalizer (as dropout.hip, sample.hip)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t stream_key(uint64_t seed, uint64_t draw) { return mix64(seed + draw * kGolden); }
__device__ __forceinline__ uint32_t draw24(uint64_t key, int tag, uint64_t i) {
  return (uint32_t)(mix64((key ^ ((uint64_t)tag * kTagMul)) + i * kGolden) >> 40);
}
// u = (n + 0.5) * 2^-24 (rounded to fp32 above 1/2: one part in 2^25)
__device__ __forceinline__ float unit_u(uint32_t n) { return (float)(2 * n + 1) * 0x1p-25f; }
// -ln u, good to a few ulp over the whole range (u or 1 - u exact in fp32)
__device__ __forceinline__ float neg_log_u(uint32_t n) {
  if (n < (1u << 23)) return -logf((float)(2 * n + 1) * 0x1p-25f);
  return -log1pf(-((float)(2 * ((1u << 24) - 1 - n) + 1) * 0x1p-25f));
}
// standard normals 2j and 2j + 1 of the stream (tag, tag + 1)
__device__ __forceinline__ void normal_pair(uint64_t key, int tag, uint64_t j, float& z0, float& z1) {
  const float r = sqrtf(2.f * neg_log_u(draw24(key, tag, j)));
  float s, c;
  sincosf(6.2831853071795865f * unit_u(draw24(key, tag + 1, j)), &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// fixed-order workgroup sum: butterfly per wave, then the wave partials left to right
__device__ __forceinline__ float block_sum(float v, float* ws) {
  v = wave_sum(v);
  block_sync();   // a previous use of ws is over
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  block_sync();
  return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__device__ __forceinline__ float softplus_precise(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus_slope(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }

// elements of sigma per row
__host__ __device__ __forceinline__ int64_t sigma_len(int mode, int K, int d) {
  return mode == MTTS_MDN_SHARED ? 1 : mode == MTTS_MDN_ISOTROPIC ? K : mode == MTTS_MDN_DIAGONAL ? (int64_t)K * d : 0;
}

// ------------------------------------------------------------------ parameters
// the pre-activation of element i of row b: sigma_raw + noise_scale * eps
template <typename T>
__device__ __forceinline__ float pre_act(const MttsMdnParamsArgs& a, int b, int64_t i, float ns, uint64_t key,
                                         float& e) {
  float x = ldf((const T*)a.sigma_raw + b * a.sraw_rs + i);
  e = 0.f;
  if (a.noise == MTTS_MDN_NOISE_GIVEN) {
    e = ldf((const T*)a.eps + b * a.eps_rs + i);
  } else if (a.noise == MTTS_MDN_NOISE_DRAWN) {
    float z0, z1;
    normal_pair(key, kTagEps, (uint64_t)(i >> 1), z0, z1);
    e = (i & 1) ? z1 : z0;
  }
  if (a.noise != MTTS_MDN_NOISE_NONE) x = x + ns * e;
  return x;
}

template <typename T>
__global__ __launch_bounds__(kT) void mdn_params_fwd_kernel(MttsMdnParamsArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
  const T* lg = (const T*)a.pi_logits + b * a.logits_rs;
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmaxf(m, ldf(lg + k));
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(ldf(lg + k) - m);
  if (tid < K) stf((T*)a.pi + b * a.pi_rs + tid, expf(ldf(lg + tid) - m) / s);
  const int64_t S = sigma_len(a.mode, K, a.d);
  if (S == 0) return;
  uint64_t key = 0;
  float ns = 0.f;
  if (a.noise != MTTS_MDN_NOISE_NONE) ns = *a.noise_scale;
  if (a.noise == MTTS_MDN_NOISE_DRAWN) {
    const int64_t base = a.seed_in ? *a.seed_in : 0;
    if (a.seed_out && b == 0 && tid == 0) *a.seed_out = base;
    key = stream_key((uint64_t)a.row_seed[b] + (uint64_t)base, 0);
  }
  for (int64_t i = tid; i < S; i += kT) {
    float e;
    const float x = pre_act<T>(a, b, i, ns, key, e);
    stf((T*)a.sigma + b * a.sigma_rs + i, softplus_precise(x));
  }
}

template <typename T>
__global__ __launch_bounds__(kT) void mdn_params_bwd_kernel(MttsMdnParamsBwdArgs g) {
  const MttsMdnParamsArgs& a = g.f;
  __shared__ float ws[4];
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
  // the softmax again from the logits (K <= 32 terms): a stored bf16 pi would add its rounding
  const T* lg = (const T*)a.pi_logits + b * a.logits_rs;
  const T* dpi = (const T*)g.dpi + b * g.dpi_rs;
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmaxf(m, ldf(lg + k));
  float s = 0.f, dot = 0.f;
  for (int k = 0; k < K; ++k) {
    const float e = expf(ldf(lg + k) - m);
    s += e;
    dot += ldf(dpi + k) * e;
  }
  dot /= s;
  if (tid < K) stf((T*)g.dlogits + b * g.dlogits_rs + tid, expf(ldf(lg + tid) - m) / s * (ldf(dpi + tid) - dot));
  const int64_t S = sigma_len(a.mode, K, a.d);
  if (S == 0) return;
  uint64_t key = 0;
  float ns = 0.f;
  if (a.noise != MTTS_MDN_NOISE_NONE) ns = *a.noise_scale;
  if (a.noise == MTTS_MDN_NOISE_DRAWN)
    key = stream_key((uint64_t)a.row_seed[b] + (uint64_t)(a.seed_in ? *a.seed_in : 0), 0);
  float part = 0.f;
  for (int64_t i = tid; i < S; i += kT) {
    float e;
    const float x = pre_act<T>(a, b, i, ns, key, e);
    const float d = ldf((const T*)g.dsigma + b * g.dsigma_rs + i) * softplus_slope(x);
    stf((T*)g.dsigma_raw + b * g.dsraw_rs + i, d);
    part += d * e;
  }
  part = block_sum(part, ws);
  if (tid == 0) g.workspace[b] = part;
}

// one workgroup: out[0] = scale * (sum of v[0 .. n) in a fixed order)
__global__ __launch_bounds__(kT) void mdn_sum_kernel(const float* __restrict__ v, int n, float scale,
                                                     float* __restrict__ out) {
  __shared__ float ws[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kT) s += v[i];
  s = block_sum(s, ws);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// ------------------------------------------------------------------------ loss
// lw[k] = log(pi_k + 1e-8) + log N(y | mu_k, var); ss[k] = sum_j (y_j - mu_kj)^2
// (diagonal: sum_j (y_j - mu_kj)^2 / var_kj).  Wave w takes k = w, w + 4, ...
template <typename T>
__device__ __forceinline__ void log_weights(const MttsMixtureNllArgs& a, int b, float* lw, float* ss) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, K = a.K, d = a.d;
  const T* y = (const T*)a.y + b * a.y_rs;
  const T* mu = (const T*)a.mu + b * a.mu_rs;
  const T* sg = (const T*)a.sigma + b * a.sigma_rs;
  const T* pi = (const T*)a.pi + b * a.pi_rs;
  for (int k = wave; k < K; k += kT / 64) {
    float acc = 0.f, accl = 0.f;
    for (int j = lane; j < d; j += 64) {
      const float diff = ldf(y + j) - ldf(mu + (int64_t)k * d + j);
      if (a.mode == MTTS_MDN_DIAGONAL) {
        const float s = ldf(sg + (int64_t)k * d + j), var = s * s;
        acc += diff * diff / var;
        accl += logf(var);
      } else {
        acc += diff * diff;
      }
    }
    acc = wave_sum(acc);
    accl = wave_sum(accl);
    if (lane == 0) {
      float logp;
      if (a.mode == MTTS_MDN_DIAGONAL) {
        logp = -kHalfLog2Pi * d - 0.5f * accl - 0.5f * acc;
      } else {
        float var = 0.01f;
        if (a.mode == MTTS_MDN_SHARED) { const float s = ldf(sg); var = s * s; }
        if (a.mode == MTTS_MDN_ISOTROPIC) { const float s = ldf(sg + k); var = s * s; }
        logp = -kHalfLog2Pi * d - 0.5f * d * logf(var) - 0.5f * acc / var;
      }
      lw[k] = logf(ldf(pi + k) + 1e-8f) + logp;
      ss[k] = acc;
    }
  }
  block_sync();
}

template <typename T>
__global__ __launch_bounds__(kT) void mixture_nll_fwd_kernel(MttsMixtureNllArgs a) {
  __shared__ float lw[MTTS_MDN_MAX_K], ss[MTTS_MDN_MAX_K];
  const int b = blockIdx.x;
  log_weights<T>(a, b, lw, ss);
  if (threadIdx.x == 0) {
    float m = -INFINITY;
    for (int k = 0; k < a.K; ++k) m = fmaxf(m, lw[k]);
    float s = 0.f;
    for (int k = 0; k < a.K; ++k) s += expf(lw[k] - m);
    a.lse[b] = m + logf(s);
  }
}

template <typename T>
__global__ __launch_bounds__(kT) void mixture_nll_bwd_kernel(MttsMixtureNllBwdArgs g) {
  const MttsMixtureNllArgs& a = g.f;
  __shared__ float lw[MTTS_MDN_MAX_K], ss[MTTS_MDN_MAX_K], rk[MTTS_MDN_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, d = a.d;
  log_weights<T>(a, b, lw, ss);
  const float w = -g.grad_loss[0] / (float)a.rows;     // d loss / d lse_b
  const T* y = (const T*)a.y + b * a.y_rs;
  const T* mu = (const T*)a.mu + b * a.mu_rs;
  const T* sg = (const T*)a.sigma + b * a.sigma_rs;
  const T* pi = (const T*)a.pi + b * a.pi_rs;
  if (tid < K) {
    const float r = expf(lw[tid] - a.lse[b]);          // responsibility of component tid
    rk[tid] = r;
    stf((T*)g.dpi + b * g.dpi_rs + tid, w * r / (ldf(pi + tid) + 1e-8f));
    if (a.mode == MTTS_MDN_ISOTROPIC) {
      const float s = ldf(sg + tid);
      stf((T*)g.dsigma + b * g.dsigma_rs + tid, w * r * (ss[tid] / (s * s) - (float)d) / s);
    }
  }
  block_sync();
  if (a.mode == MTTS_MDN_SHARED && tid == 0) {
    const float s = ldf(sg), var = s * s;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc += rk[k] * (ss[k] / var - (float)d);
    stf((T*)g.dsigma + b * g.dsigma_rs, w * acc / s);
  }
  float ivar = 100.f;                                   // fixed: 1 / 0.01
  if (a.mode == MTTS_MDN_SHARED) { const float s = ldf(sg); ivar = 1.f / (s * s); }
  for (int j = tid; j < d; j += kT) {
    const float yj = ldf(y + j);
    float dyj = 0.f;
    for (int k = 0; k < K; ++k) {
      const int64_t at = (int64_t)k * d + j;
      const float diff = yj - ldf(mu + at);
      float iv = ivar;
      if (a.mode == MTTS_MDN_ISOTROPIC) { const float s = ldf(sg + k); iv = 1.f / (s * s); }
      if (a.mode == MTTS_MDN_DIAGONAL) {
        const float s = ldf(sg + at);
        iv = 1.f / (s * s);
        stf((T*)g.dsigma + b * g.dsigma_rs + at, w * rk[k] * (diff * diff * iv - 1.f) / s);
      }
      const float dm = w * rk[k] * diff * iv;
      stf((T*)g.dmu + b * g.dmu_rs + at, dm);
      dyj -= dm;
    }
    stf((T*)g.dy + b * g.dy_rs + j, dyj);
  }
}

// --------------------------------------------------------------------- sampler
template <typename T>
__global__ __launch_bounds__(kT) void mixture_sample_kernel(MttsMixtureSampleArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, d = a.d;
  const T* pi = (const T*)a.pi + b * a.pi_rs;
  const T* mu = (const T*)a.mu + b * a.mu_rs;
  const T* sg = (const T*)a.sigma + b * a.sigma_rs;
  const uint64_t key = stream_key((uint64_t)a.seed[b] + (uint64_t)(a.seed_in ? *a.seed_in : 0),
                                  a.draw ? (uint64_t)a.draw[b] : 0);
  const float u = unit_u(draw24(key, kTagComp, 0));
  float total = 0.f;
  for (int k = 0; k < K; ++k) total += ldf(pi + k);
  int kk = K - 1;
  float cdf = 0.f;
  for (int k = 0; k < K - 1; ++k) {
    cdf += ldf(pi + k);
    if (u * total < cdf) { kk = k; break; }
  }
  if (a.component && tid == 0) a.component[b] = kk;
  float sd = 0.1f;                                      // fixed
  if (a.mode == MTTS_MDN_SHARED) sd = ldf(sg);
  if (a.mode == MTTS_MDN_ISOTROPIC) sd = ldf(sg + kk);
  T* out = (T*)a.out + b * a.out_rs;
  for (int j = tid; 2 * j < d; j += kT) {
    float z[2];
    normal_pair(key, kTagZ, (uint64_t)j, z[0], z[1]);
    for (int h = 0; h < 2; ++h) {
      const int e = 2 * j + h;
      if (e < d) {
        const int64_t at = (int64_t)kk * d + e;
        const float s = a.mode == MTTS_MDN_DIAGONAL ? ldf(sg + at) : sd;
        stf(out + e, ldf(mu + at) + s * z[h]);
      }
    }
  }
}

// ------------------------------------------------------- LayerNorm, any width
// The head's input LayerNorm at widths ln.hip does not take (not a multiple of
// 64): y = (x - mean) rstd w + b per row, two passes over the row (mean, then
// the centred sum of squares), biased variance; mean and rstd saved.  Backward:
// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w, one workgroup per row;
// dw, db by one thread per column over the rows in index order.
template <typename T>
__global__ __launch_bounds__(kT) void rowln_fwd_kernel(MttsRowLNArgs a) {
  __shared__ float ws[4];
  const int r = blockIdx.x, n = a.cols;
  const T* x = (const T*)a.x + r * a.x_rs;
  float s = 0.f;
  for (int c = threadIdx.x; c < n; c += kT) s += ldf(x + c);
  const float mean = block_sum(s, ws) / (float)n;
  float q = 0.f;
  for (int c = threadIdx.x; c < n; c += kT) { const float v = ldf(x + c) - mean; q += v * v; }
  const float rstd = 1.f / sqrtf(block_sum(q, ws) / (float)n + a.eps);
  if (threadIdx.x == 0) { a.mean[r] = mean; a.rstd[r] = rstd; }
  T* y = (T*)a.y + r * a.y_rs;
  for (int c = threadIdx.x; c < n; c += kT) stf(y + c, (ldf(x + c) - mean) * rstd * a.w[c] + a.b[c]);
}

template <typename T>
__global__ __launch_bounds__(kT) void rowln_bwd_kernel(MttsRowLNBwdArgs g) {
  const MttsRowLNArgs& a = g.f;
  __shared__ float ws[4];
  const int r = blockIdx.x, n = a.cols;
  const T* x = (const T*)a.x + r * a.x_rs;
  const T* dy = (const T*)g.dy + r * g.dy_rs;
  const float mean = a.mean[r], rstd = a.rstd[r];
  float s1 = 0.f, s2 = 0.f;
  for (int c = threadIdx.x; c < n; c += kT) {
    const float gv = ldf(dy + c) * a.w[c];
    s1 += gv;
    s2 += gv * (ldf(x + c) - mean) * rstd;
  }
  const float c1 = block_sum(s1, ws) / (float)n;
  const float c2 = block_sum(s2, ws) / (float)n;
  T* dx = (T*)g.dx + r * g.dx_rs;
  for (int c = threadIdx.x; c < n; c += kT) {
    const float xh = (ldf(x + c) - mean) * rstd;
    stf(dx + c, rstd * (ldf(dy + c) * a.w[c] - c1 - xh * c2));
  }
}

template <typename T>
__global__ __launch_bounds__(kT) void rowln_wgrad_kernel(MttsRowLNBwdArgs g) {
  const MttsRowLNArgs& a = g.f;
  const int c = blockIdx.x * kT + threadIdx.x;
  if (c >= a.cols) return;
  float dw = 0.f, db = 0.f;
  for (int r = 0; r < a.rows; ++r) {
    const float d = ldf((const T*)g.dy + r * g.dy_rs + c);
    dw += d * (ldf((const T*)a.x + r * a.x_rs + c) - a.mean[r]) * a.rstd[r];
    db += d;
  }
  g.dw[c] = dw;
  g.db[c] = db;
}

// ---------------------------------------------------------------- relu_dropout
// forward (yf == nullptr): out = x > 0 and kept ? x * scale : 0, dropout.hip's
// mask (one 64-bit hash per element pair, its low / high half against thresh);
// backward: out = yf > 0 ? x * scale : 0 (x = dy, yf = the forward's output).
template <typename T>
__global__ __launch_bounds__(kT) void relu_dropout_kernel(const T* __restrict__ x, const T* __restrict__ yf,
                                                          T* __restrict__ out, int64_t n, uint64_t seed,
                                                          uint32_t thresh, float scale,
                                                          const int64_t* __restrict__ seed_in,
                                                          int64_t* __restrict__ seed_out) {
  constexpr int V = 16 / sizeof(T);
  if (!yf && seed_in) {
    const int64_t base = *seed_in;
    if (seed_out && blockIdx.x == 0 && threadIdx.x == 0) *seed_out = base;
    seed += (uint64_t)base;
  }
  const int64_t nv = n / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t v = t0; v < nv; v += stride) {
    float f[V], o[V];
    ld_vec<T, V>(x + v * V, f);
    if (yf) {
      float y[V];
      ld_vec<T, V>(yf + v * V, y);
#pragma unroll
      for (int q = 0; q < V; ++q) o[q] = y[q] > 0.f ? f[q] * scale : 0.f;
    } else {
#pragma unroll
      for (int q = 0; q < V / 2; ++q) {
        const uint64_t h = mix64(seed + (uint64_t)(v * (V / 2) + q) * kGolden);
        o[2 * q] = (f[2 * q] > 0.f && (uint32_t)h >= thresh) ? f[2 * q] * scale : 0.f;
        o[2 * q + 1] = (f[2 * q + 1] > 0.f && (uint32_t)(h >> 32) >= thresh) ? f[2 * q + 1] * scale : 0.f;
      }
    }
    st_vec<T, V>(out + v * V, o);
  }
  // the n % V elements past the last whole piece, one per thread
  for (int64_t i = nv * V + t0; i < n; i += stride) {
    const float f = ldf(x + i);
    float o;
    if (yf) {
      o = ldf(yf + i) > 0.f ? f * scale : 0.f;
    } else {
      const uint64_t h = mix64(seed + (uint64_t)(i >> 1) * kGolden);
      o = (f > 0.f && (uint32_t)(h >> (32 * (i & 1))) >= thresh) ? f * scale : 0.f;
    }
    stf(out + i, o);
  }
}

// ---------------------------------------------------------------------- checks
int check_shape(const char* who, int rows, int K, int d, int mode, int dtype) {
  MTTS_CHECK(dtype == MTTS_F32 || dtype == MTTS_BF16, "%s: dtype must be F32 or BF16", who);
  MTTS_CHECK(rows > 0 && d > 0, "%s: rows=%d d=%d must be positive", who, rows, d);
  MTTS_CHECK(K >= 1 && K <= MTTS_MDN_MAX_K, "%s: K=%d must be in [1, %d]", who, K, MTTS_MDN_MAX_K);
  MTTS_CHECK(mode >= MTTS_MDN_SHARED && mode <= MTTS_MDN_FIXED, "%s: unknown variance mode %d", who, mode);
  return MTTS_OK;
}

// sigma: present with a row of sigma_len elements unless the mode is fixed
int check_sigma(const char* who, int mode, int K, int d, const void* sigma, int64_t rs) {
  if (mode == MTTS_MDN_FIXED) return MTTS_OK;
  MTTS_CHECK(sigma, "%s: null sigma in a mode that has one", who);
  MTTS_CHECK(rs >= sigma_len(mode, K, d), "%s: sigma row stride %lld below the mode's %lld elements", who,
             (long long)rs, (long long)sigma_len(mode, K, d));
  return MTTS_OK;
}

int check_params(const char* who, const MttsMdnParamsArgs* a) {
  MTTS_CHECK(a && a->pi_logits && a->pi, "%s: null pointer", who);
  int rc = check_shape(who, a->rows, a->K, a->d, a->mode, a->dtype);
  if (rc) return rc;
  MTTS_CHECK(a->logits_rs >= a->K && a->pi_rs >= a->K, "%s: pi row strides below K", who);
  MTTS_CHECK(a->noise >= MTTS_MDN_NOISE_NONE && a->noise <= MTTS_MDN_NOISE_DRAWN, "%s: unknown noise kind %d", who,
             a->noise);
  if (a->mode == MTTS_MDN_FIXED) {
    MTTS_CHECK(a->noise == MTTS_MDN_NOISE_NONE, "%s: the fixed mode has no sigma to perturb", who);
    return MTTS_OK;
  }
  const int64_t S = sigma_len(a->mode, a->K, a->d);
  MTTS_CHECK(a->sigma_raw && a->sraw_rs >= S, "%s: null sigma_raw or its row stride below %lld", who, (long long)S);
  rc = check_sigma(who, a->mode, a->K, a->d, a->sigma, a->sigma_rs);
  if (rc) return rc;
  if (a->noise != MTTS_MDN_NOISE_NONE) MTTS_CHECK(a->noise_scale, "%s: noise without noise_scale", who);
  if (a->noise == MTTS_MDN_NOISE_GIVEN)
    MTTS_CHECK(a->eps && a->eps_rs >= S, "%s: null eps or its row stride below %lld", who, (long long)S);
  if (a->noise == MTTS_MDN_NOISE_DRAWN) MTTS_CHECK(a->row_seed, "%s: drawn noise without row seeds", who);
  return MTTS_OK;
}

int check_nll(const char* who, const MttsMixtureNllArgs* a) {
  MTTS_CHECK(a && a->y && a->pi && a->mu && a->loss && a->lse, "%s: null pointer", who);
  int rc = check_shape(who, a->rows, a->K, a->d, a->mode, a->dtype);
  if (rc) return rc;
  MTTS_CHECK(a->y_rs >= a->d && a->pi_rs >= a->K && a->mu_rs >= (int64_t)a->K * a->d, "%s: a row stride is too short",
             who);
  return check_sigma(who, a->mode, a->K, a->d, a->sigma, a->sigma_rs);
}

int check_rowln(const char* who, const MttsRowLNArgs* a) {
  MTTS_CHECK(a && a->x && a->w && a->b && a->y && a->mean && a->rstd, "%s: null pointer", who);
  MTTS_CHECK(a->dtype == MTTS_F32 || a->dtype == MTTS_BF16, "%s: dtype must be F32 or BF16", who);
  MTTS_CHECK(a->rows > 0 && a->cols > 0, "%s: rows=%d cols=%d must be positive", who, a->rows, a->cols);
  MTTS_CHECK(a->x_rs >= a->cols && a->y_rs >= a->cols, "%s: a row stride is below cols", who);
  return MTTS_OK;
}

}  // namespace
}  // namespace mtts

using namespace mtts;

#define MDN_LAUNCH(kernel, dtype, grid, st, ...)                                              \
  do {                                                                                        \
    if ((dtype) == MTTS_F32) hipLaunchKernelGGL(kernel<float>, dim3(grid), dim3(kT), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel<bf16_t>, dim3(grid), dim3(kT), 0, st, __VA_ARGS__);        \
  } while (0)

extern "C" int mtts_mdn_params_fwd(const MttsMdnParamsArgs* a, void* stream) {
  int rc = check_params("mdn_params_fwd", a);
  if (rc) return rc;
  MDN_LAUNCH(mdn_params_fwd_kernel, a->dtype, a->rows, (hipStream_t)stream, *a);
  MTTS_LAUNCH_CHECK("mdn_params_fwd");
  return MTTS_OK;
}

extern "C" int mtts_mdn_params_bwd(const MttsMdnParamsBwdArgs* g, void* stream) {
  MTTS_CHECK(g, "mdn_params_bwd: null pointer");
  const MttsMdnParamsArgs* a = &g->f;
  int rc = check_params("mdn_params_bwd", a);
  if (rc) return rc;
  MTTS_CHECK(g->dpi && g->dlogits && g->dpi_rs >= a->K && g->dlogits_rs >= a->K,
             "mdn_params_bwd: null pi gradient or a row stride below K");
  const int64_t S = sigma_len(a->mode, a->K, a->d);
  if (S > 0) {
    MTTS_CHECK(g->dsigma && g->dsigma_raw && g->workspace && g->dsigma_rs >= S && g->dsraw_rs >= S,
               "mdn_params_bwd: null sigma gradient / workspace or a row stride below %lld", (long long)S);
    MTTS_CHECK(a->noise == MTTS_MDN_NOISE_NONE || g->dnoise_scale, "mdn_params_bwd: null dnoise_scale");
  }
  hipStream_t st = (hipStream_t)stream;
  MDN_LAUNCH(mdn_params_bwd_kernel, a->dtype, a->rows, st, *g);
  if (S > 0 && g->dnoise_scale)
    hipLaunchKernelGGL(mdn_sum_kernel, dim3(1), dim3(kT), 0, st, (const float*)g->workspace, a->rows, 1.f,
                       g->dnoise_scale);
  MTTS_LAUNCH_CHECK("mdn_params_bwd");
  return MTTS_OK;
}

extern "C" int mtts_mixture_nll_fwd(const MttsMixtureNllArgs* a, void* stream) {
  int rc = check_nll("mixture_nll_fwd", a);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  MDN_LAUNCH(mixture_nll_fwd_kernel, a->dtype, a->rows, st, *a);
  hipLaunchKernelGGL(mdn_sum_kernel, dim3(1), dim3(kT), 0, st, (const float*)a->lse, a->rows, -1.f / (float)a->rows,
                     a->loss);
  MTTS_LAUNCH_CHECK("mixture_nll_fwd");
  return MTTS_OK;
}

extern "C" int mtts_mixture_nll_bwd(const MttsMixtureNllBwdArgs* g, void* stream) {
  MTTS_CHECK(g, "mixture_nll_bwd: null pointer");
  const MttsMixtureNllArgs* a = &g->f;
  int rc = check_nll("mixture_nll_bwd", a);
  if (rc) return rc;
  MTTS_CHECK(g->grad_loss && g->dy && g->dpi && g->dmu, "mixture_nll_bwd: null gradient pointer");
  MTTS_CHECK(g->dy_rs >= a->d && g->dpi_rs >= a->K && g->dmu_rs >= (int64_t)a->K * a->d,
             "mixture_nll_bwd: a gradient row stride is too short");
  rc = check_sigma("mixture_nll_bwd (dsigma)", a->mode, a->K, a->d, g->dsigma, g->dsigma_rs);
  if (rc) return rc;
  MDN_LAUNCH(mixture_nll_bwd_kernel, a->dtype, a->rows, (hipStream_t)stream, *g);
  MTTS_LAUNCH_CHECK("mixture_nll_bwd");
  return MTTS_OK;
}

extern "C" int mtts_mixture_sample(const MttsMixtureSampleArgs* a, void* stream) {
  MTTS_CHECK(a && a->pi && a->mu && a->seed && a->out, "mixture_sample: null pointer");
  int rc = check_shape("mixture_sample", a->rows, a->K, a->d, a->mode, a->dtype);
  if (rc) return rc;
  MTTS_CHECK(a->pi_rs >= a->K && a->mu_rs >= (int64_t)a->K * a->d && a->out_rs >= a->d,
             "mixture_sample: a row stride is too short");
  rc = check_sigma("mixture_sample", a->mode, a->K, a->d, a->sigma, a->sigma_rs);
  if (rc) return rc;
  MDN_LAUNCH(mixture_sample_kernel, a->dtype, a->rows, (hipStream_t)stream, *a);
  MTTS_LAUNCH_CHECK("mixture_sample");
  return MTTS_OK;
}

extern "C" int mtts_mdn_layernorm_fwd(const MttsRowLNArgs* a, void* stream) {
  int rc = check_rowln("mdn_layernorm_fwd", a);
  if (rc) return rc;
  MDN_LAUNCH(rowln_fwd_kernel, a->dtype, a->rows, (hipStream_t)stream, *a);
  MTTS_LAUNCH_CHECK("mdn_layernorm_fwd");
  return MTTS_OK;
}

extern "C" int mtts_mdn_layernorm_bwd(const MttsRowLNBwdArgs* g, void* stream) {
  MTTS_CHECK(g, "mdn_layernorm_bwd: null pointer");
  const MttsRowLNArgs* a = &g->f;
  int rc = check_rowln("mdn_layernorm_bwd", a);
  if (rc) return rc;
  MTTS_CHECK(g->dy && g->dx && g->dw && g->db, "mdn_layernorm_bwd: null gradient pointer");
  MTTS_CHECK(g->dy_rs >= a->cols && g->dx_rs >= a->cols, "mdn_layernorm_bwd: a gradient row stride is below cols");
  hipStream_t st = (hipStream_t)stream;
  MDN_LAUNCH(rowln_bwd_kernel, a->dtype, a->rows, st, *g);
  MDN_LAUNCH(rowln_wgrad_kernel, a->dtype, (a->cols + kT - 1) / kT, st, *g);
  MTTS_LAUNCH_CHECK("mdn_layernorm_bwd");
  return MTTS_OK;
}

extern "C" int mtts_relu_dropout(const MttsReluDropoutArgs* a, void* stream) {
  MTTS_CHECK(a && a->x && a->out, "relu_dropout: null pointer");
  MTTS_CHECK(a->dtype == MTTS_F32 || a->dtype == MTTS_BF16, "relu_dropout: dtype must be f32 or bf16");
  MTTS_CHECK(a->n >= 0, "relu_dropout: n=%lld must not be negative", (long long)a->n);
  MTTS_CHECK(a->p >= 0.f && a->p < 1.f, "relu_dropout: p=%f must be in [0, 1)", (double)a->p);
  MTTS_CHECK(((uintptr_t)a->x | (uintptr_t)a->out | (uintptr_t)a->y_fwd) % 16 == 0,
             "relu_dropout: x / y_fwd / out must be 16-byte aligned");
  if (a->n == 0) return MTTS_OK;
  const uint32_t thresh = (uint32_t)fmin((double)a->p * 4294967296.0, 4294967295.0);
  const float scale = 1.f / (1.f - a->p);
  const int64_t nv = a->n / (a->dtype == MTTS_F32 ? 4 : 8) + 1;
  const int blocks = (int)std::min<int64_t>((nv + kT - 1) / kT, 2048);
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == MTTS_F32)
    hipLaunchKernelGGL(relu_dropout_kernel<float>, dim3(blocks), dim3(kT), 0, st, (const float*)a->x,
                       (const float*)a->y_fwd, (float*)a->out, a->n, a->seed, thresh, scale, a->seed_in, a->seed_out);
  else
    hipLaunchKernelGGL(relu_dropout_kernel<bf16_t>, dim3(blocks), dim3(kT), 0, st, (const bf16_t*)a->x,
                       (const bf16_t*)a->y_fwd, (bf16_t*)a->out, a->n, a->seed, thresh, scale, a->seed_in,
                       a->seed_out);
  MTTS_LAUNCH_CHECK("relu_dropout");
  return MTTS_OK;
}
