// Fused gradient-norm clipping + Adam over a whole parameter list (SURVEY.md
// §8f row 4; reference train.py:232-235: clip_grad_norm_(decoder.parameters(),
// 1.0) then torch.optim.Adam.step()).  Three launches per step, independent of
// the number of tensors:
//   1. per-chunk partial sums of g^2 (64 Ki elements per block, float4),
//   2. one block: total = sqrt(sum of partials) in a fixed order,
//      coef = min(1, max_norm / (total + 1e-6))   (clip_grad_norm_'s formula;
//      NaN when the norm is NaN, as torch's clamp gives),
//      t = ++(*step_counter) and the bias corrections (device-side, so the
//      whole training step can be captured in a hipGraph and replayed),
//   3. per-chunk Adam on (p, g*coef, m, v) with torch's update:
//        m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2
//        p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// (plus L2 weight decay g += wd*p before the moments, as torch.optim.Adam).
// HBM: reads g twice and p, m, v once, writes p, m, v: 32 B per parameter
// (torch: foreach norm + clip rewrite + fused Adam = 40 B and more launches).
// Gradients are left unclipped (the update uses g*coef).
#include "common.h"

namespace mtts {

constexpr int64_t kAdamChunk = 65536;   // elements per block
constexpr int kAdamBlock = 256;

template <class Tensor>
__device__ __forceinline__ int find_tensor(const Tensor* __restrict__ t, int n, int64_t blk) {
  int lo = 0, hi = n - 1;  // last tensor with chunk0 <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].chunk0 <= blk) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  block_sync();
  float s = 0.f;
  if (threadIdx.x == 0) {
    for (int i = 0; i < kAdamBlock / 64; ++i) s += red[i];
  }
  return s;
}

// one chunk's sum of g^2 into partial[blk]; both descriptor kinds carry g, n, chunk0
template <class Tensor>
__device__ __forceinline__ void sumsq_chunk(const Tensor* __restrict__ ts, int n, float* __restrict__ partial) {
  __shared__ float red[kAdamBlock / 64];
  const int64_t blk = blockIdx.x;
  const Tensor t = ts[find_tensor(ts, n, blk)];
  const int64_t e0 = (blk - t.chunk0) * kAdamChunk;
  const int64_t e1 = min(t.n, e0 + kAdamChunk);
  float s = 0.f;
  const bool vec = ((uintptr_t)t.g % 16) == 0;
  if (vec) {
    const int64_t v0 = e0 / 4, v1 = e1 / 4;  // e0 is a multiple of 4
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(t.g);
    for (int64_t i = v0 + threadIdx.x; i < v1; i += kAdamBlock) {
      const float4 g = g4[i];
      s = fmaf(g.x, g.x, fmaf(g.y, g.y, fmaf(g.z, g.z, fmaf(g.w, g.w, s))));
    }
    for (int64_t i = v1 * 4 + threadIdx.x; i < e1; i += kAdamBlock) s = fmaf(t.g[i], t.g[i], s);
  } else {
    for (int64_t i = e0 + threadIdx.x; i < e1; i += kAdamBlock) s = fmaf(t.g[i], t.g[i], s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blk] = s;
}

__global__ __launch_bounds__(kAdamBlock) void sumsq_kernel(const MttsAdamTensor* __restrict__ ts, int n,
                                                           float* __restrict__ partial) {
  sumsq_chunk(ts, n, partial);
}

struct AdamHyper {
  float lr, b1, b2, eps, wd;
};

// one block: total grad norm, clip coefficient, and the step's bias
// corrections from the device step counter (so a captured hipGraph replays
// correct steps): out = {total, coef, lr / (1 - b1^t), sqrt(1 - b2^t)}
__global__ __launch_bounds__(kAdamBlock) void norm_final_kernel(const float* __restrict__ partial, int64_t nchunks,
                                                                float max_norm, int* __restrict__ step_counter,
                                                                const AdamHyper h, float* __restrict__ out) {
  __shared__ float red[kAdamBlock / 64];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < nchunks; i += kAdamBlock) s += partial[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float total = sqrtf(s);
    out[0] = total;
    // torch's clamp(max_norm / (total + 1e-6), max=1): a NaN norm gives a NaN
    // coefficient (fminf would return 1 and hide it), so one NaN gradient
    // element turns every parameter NaN, as clip_grad_norm_ does
    const float ratio = max_norm / (total + 1e-6f);
    out[1] = max_norm > 0.f ? (ratio > 1.f ? 1.f : ratio) : 1.f;
    const int t = step_counter[0] + 1;
    step_counter[0] = t;
    const double bc1 = 1.0 - pow((double)h.b1, (double)t), bc2 = 1.0 - pow((double)h.b2, (double)t);
    out[2] = (float)(h.lr / bc1);
    out[3] = (float)sqrt(bc2);
  }
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float coef, float step_size,
                                          float bc2_sqrt, const AdamHyper& h) {
  g *= coef;
  if (h.wd != 0.f) g = fmaf(h.wd, p, g);
  m = fmaf(h.b1, m, (1.f - h.b1) * g);
  v = fmaf(h.b2, v, (1.f - h.b2) * g * g);
  const float denom = sqrtf(v) / bc2_sqrt + h.eps;
  p -= step_size * (m / denom);
}

__global__ __launch_bounds__(kAdamBlock) void adam_kernel(const MttsAdamTensor* __restrict__ ts, int n,
                                                          const float* __restrict__ norm, const AdamHyper h) {
  const int64_t blk = blockIdx.x;
  const MttsAdamTensor t = ts[find_tensor(ts, n, blk)];
  const float coef = norm[1], step_size = norm[2], bc2_sqrt = norm[3];
  const int64_t e0 = (blk - t.chunk0) * kAdamChunk;
  const int64_t e1 = min(t.n, e0 + kAdamChunk);
  const bool vec = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) % 16) == 0;
  int64_t tail = e0;
  if (vec) {
    const int64_t v0 = e0 / 4, v1 = e1 / 4;
    float4* p4 = reinterpret_cast<float4*>(t.p);
    const float4* g4 = reinterpret_cast<const float4*>(t.g);
    float4* m4 = reinterpret_cast<float4*>(t.m);
    float4* q4 = reinterpret_cast<float4*>(t.v);
    for (int64_t i = v0 + threadIdx.x; i < v1; i += kAdamBlock) {
      float4 p = p4[i], m = m4[i], v = q4[i];
      const float4 g = g4[i];
      adam_elem(p.x, g.x, m.x, v.x, coef, step_size, bc2_sqrt, h);
      adam_elem(p.y, g.y, m.y, v.y, coef, step_size, bc2_sqrt, h);
      adam_elem(p.z, g.z, m.z, v.z, coef, step_size, bc2_sqrt, h);
      adam_elem(p.w, g.w, m.w, v.w, coef, step_size, bc2_sqrt, h);
      p4[i] = p; m4[i] = m; q4[i] = v;
    }
    tail = v1 * 4;
  }
  for (int64_t i = tail + threadIdx.x; i < e1; i += kAdamBlock)
    adam_elem(t.p[i], t.g[i], t.m[i], t.v[i], coef, step_size, bc2_sqrt, h);
}

// ------------------------------------------------------------------ AdamW
// mtts_clip_adamw (mtts.h): the same three launches over parameter groups,
// with the learning-rate schedule, decoupled decay, EMA weights and the
// non-finite guard.  Everything that differs between steps or groups is a
// launch-uniform scalar finished by the one-block kernel and read by group
// index in the element pass; the per-element arithmetic of an L2 group is
// adam_elem itself.
__global__ __launch_bounds__(kAdamBlock) void adamw_sumsq_kernel(const MttsAdamWTensor* __restrict__ ts, int n,
                                                                 float* __restrict__ partial) {
  sumsq_chunk(ts, n, partial);
}

struct AdamWHyper {
  float b1, b2, eps, max_norm;
  int ngroups, ema_warmup, skip_nonfinite;
  double ema_decay;
  uint64_t active;
  MttsLrSchedule sched;
};

// f(t) of mtts.h, in double
__device__ __forceinline__ double lr_factor(const MttsLrSchedule& s, int t) {
  const double W = (double)s.warmup_steps, r = s.min_ratio;
  if (t <= s.warmup_steps) return (double)t / W;
  if (s.kind == MTTS_LR_CONSTANT) return 1.0;
  if (s.kind == MTTS_LR_INV_SQRT) return fmax(r, sqrt(fmax(W, 1.0) / (double)t));
  const double x = fmin(1.0, ((double)t - W) / ((double)s.total_steps - W));
  if (s.kind == MTTS_LR_COSINE) return r + (1.0 - r) * 0.5 * (1.0 + cos(3.14159265358979323846 * x));
  return r + (1.0 - r) * (1.0 - x);
}

// one block: the clip norm over chunks [0, clip_chunks) in norm_final_kernel's
// order, the finiteness of the sum over all chunks, the schedule, and thread
// g finishes group g's scalars from its own step counter
__global__ __launch_bounds__(kAdamBlock) void adamw_final_kernel(const float* __restrict__ partial, int64_t nchunks,
                                                                 int64_t clip_chunks,
                                                                 const MttsAdamWGroup* __restrict__ groups,
                                                                 int* __restrict__ group_steps,
                                                                 int* __restrict__ skipped, const AdamWHyper h,
                                                                 float* __restrict__ out) {
  __shared__ float red[kAdamBlock / 64], red2[kAdamBlock / 64];
  __shared__ int steps[MTTS_ADAMW_MAX_GROUPS];
  __shared__ int skip;
  float s = 0.f, rest = 0.f;
  for (int64_t i = threadIdx.x; i < clip_chunks; i += kAdamBlock) s += partial[i];
  for (int64_t i = clip_chunks + threadIdx.x; i < nchunks; i += kAdamBlock) rest += partial[i];
  if (threadIdx.x < h.ngroups) steps[threadIdx.x] = group_steps[threadIdx.x];
  s = block_sum(s, red);
  rest = block_sum(rest, red2);
  if (threadIdx.x == 0) {
    const float total = sqrtf(s);
    out[0] = total;
    const float ratio = h.max_norm / (total + 1e-6f);  // a NaN norm stays NaN: norm_final_kernel
    out[1] = h.max_norm > 0.f ? (ratio > 1.f ? 1.f : ratio) : 1.f;
    // an fp32 overflow of the sum over finite gradients counts as non-finite too
    const int bad = h.skip_nonfinite && !isfinite(s + rest);
    if (bad) skipped[0] += 1;
    out[4] = bad ? 1.f : 0.f;
    skip = bad;
  }
  block_sync();
  int t = 0;
  for (int g = 0; g < h.ngroups; ++g) t = max(t, steps[g]);
  t += 1;
  const double f = lr_factor(h.sched, t);
  if (threadIdx.x == 0) {
    out[2] = (float)f;
    const double d = h.ema_warmup ? fmin(h.ema_decay, (1.0 + t) / (10.0 + t)) : h.ema_decay;
    out[3] = (float)(1.0 - d);
  }
  const int g = threadIdx.x;
  if (g >= h.ngroups) return;
  const MttsAdamWGroup gr = groups[g];
  const double lr_t = (double)gr.lr * f;
  out[MTTS_ADAMW_OUT_LR + g] = (float)lr_t;
  if (skip || !((h.active >> g) & 1)) return;
  const int tg = steps[g] + 1;
  group_steps[g] = tg;
  const double bc1 = 1.0 - pow((double)h.b1, (double)tg), bc2 = 1.0 - pow((double)h.b2, (double)tg);
  out[MTTS_ADAMW_OUT_STEP + g] = (float)(lr_t / bc1);
  out[MTTS_ADAMW_OUT_BC2 + g] = (float)sqrt(bc2);
  out[MTTS_ADAMW_OUT_DECAY + g] = gr.decoupled ? (float)(1.0 - lr_t * (double)gr.weight_decay) : 1.f;
}

struct AdamWStep {
  float coef, step_size, bc2_sqrt, decay, one_minus_d;
  bool decoupled;
  AdamHyper h;  // wd: the L2 term only (0 for a decoupled group)
};

template <bool EMA>
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float& e, const AdamWStep& s) {
  if (s.decoupled) p *= s.decay;
  adam_elem(p, g, m, v, s.coef, s.step_size, s.bc2_sqrt, s.h);
  if (EMA) e = fmaf(s.one_minus_d, p - e, e);
}

template <bool EMA>
__device__ __forceinline__ void adamw_chunk(const MttsAdamWTensor& t, int64_t e0, int64_t e1, const AdamWStep& s) {
  // ema is NULL without EMA: it does not enter the alignment decision then
  const bool vec = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq |
                     (uintptr_t)t.ema) % 16) == 0;
  int64_t tail = e0;
  float none = 0.f;
  if (vec) {
    const int64_t v0 = e0 / 4, v1 = e1 / 4;
    float4* p4 = reinterpret_cast<float4*>(t.p);
    const float4* g4 = reinterpret_cast<const float4*>(t.g);
    float4* m4 = reinterpret_cast<float4*>(t.exp_avg);
    float4* q4 = reinterpret_cast<float4*>(t.exp_avg_sq);
    float4* e4 = reinterpret_cast<float4*>(t.ema);
    for (int64_t i = v0 + threadIdx.x; i < v1; i += kAdamBlock) {
      float4 p = p4[i], m = m4[i], v = q4[i], e = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 g = g4[i];
      if (EMA) e = e4[i];
      adamw_elem<EMA>(p.x, g.x, m.x, v.x, e.x, s);
      adamw_elem<EMA>(p.y, g.y, m.y, v.y, e.y, s);
      adamw_elem<EMA>(p.z, g.z, m.z, v.z, e.z, s);
      adamw_elem<EMA>(p.w, g.w, m.w, v.w, e.w, s);
      p4[i] = p; m4[i] = m; q4[i] = v;
      if (EMA) e4[i] = e;
    }
    tail = v1 * 4;
  }
  for (int64_t i = tail + threadIdx.x; i < e1; i += kAdamBlock)
    adamw_elem<EMA>(t.p[i], t.g[i], t.exp_avg[i], t.exp_avg_sq[i], EMA ? t.ema[i] : none, s);
}

__global__ __launch_bounds__(kAdamBlock) void adamw_kernel(const MttsAdamWTensor* __restrict__ ts, int n,
                                                           const MttsAdamWGroup* __restrict__ groups,
                                                           const float* __restrict__ out, float b1, float b2,
                                                           float eps) {
  if (out[4] != 0.f) return;  // skipped step: before any tensor element is loaded
  const int64_t blk = blockIdx.x;
  const MttsAdamWTensor t = ts[find_tensor(ts, n, blk)];
  const MttsAdamWGroup gr = groups[t.group];
  AdamWStep s;
  s.coef = gr.clip ? out[1] : 1.f;
  s.step_size = out[MTTS_ADAMW_OUT_STEP + t.group];
  s.bc2_sqrt = out[MTTS_ADAMW_OUT_BC2 + t.group];
  s.decay = out[MTTS_ADAMW_OUT_DECAY + t.group];
  s.one_minus_d = out[3];
  s.decoupled = gr.decoupled != 0;
  s.h.lr = 0.f;  // unused: step_size carries it
  s.h.b1 = b1;
  s.h.b2 = b2;
  s.h.eps = eps;
  s.h.wd = gr.decoupled ? 0.f : gr.weight_decay;
  const int64_t e0 = (blk - t.chunk0) * kAdamChunk;
  const int64_t e1 = min(t.n, e0 + kAdamChunk);
  if (t.ema) adamw_chunk<true>(t, e0, e1, s);
  else adamw_chunk<false>(t, e0, e1, s);
}

}  // namespace mtts

using namespace mtts;

extern "C" int64_t mtts_adam_chunks(int64_t numel) { return numel <= 0 ? 0 : (numel + kAdamChunk - 1) / kAdamChunk; }

extern "C" int64_t mtts_adam_workspace(int64_t total_chunks) { return total_chunks * 4 + 256; }

extern "C" int mtts_clip_adam(const MttsAdamTensor* tensors, int ntensors, int64_t total_chunks, int* step_counter,
                              float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                              void* workspace, float* norm_out, void* stream) {
  MTTS_CHECK(tensors && ntensors > 0 && total_chunks > 0 && workspace && step_counter && norm_out,
             "clip_adam: bad args");
  MTTS_CHECK(total_chunks < (1ll << 31), "clip_adam: too many chunks");
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  if (max_norm > 0.f) {
    hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)total_chunks), dim3(kAdamBlock), 0, st, tensors, ntensors,
                       partial);
    MTTS_LAUNCH_CHECK("clip_adam sumsq");
  }
  AdamHyper h;
  h.lr = lr;
  h.b1 = beta1;
  h.b2 = beta2;
  h.eps = eps;
  h.wd = weight_decay;
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(kAdamBlock), 0, st, partial, max_norm > 0.f ? total_chunks : 0,
                     max_norm, step_counter, h, norm_out);
  MTTS_LAUNCH_CHECK("clip_adam norm");
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)total_chunks), dim3(kAdamBlock), 0, st, tensors, ntensors, norm_out,
                     h);
  MTTS_LAUNCH_CHECK("clip_adam adam");
  return MTTS_OK;
}

extern "C" int mtts_clip_adamw(const MttsAdamWTensor* tensors, int ntensors, const MttsAdamWGroup* groups,
                               const MttsAdamWArgs* a, int* group_steps, int* skipped, void* workspace, float* out,
                               void* stream) {
  MTTS_CHECK(tensors && ntensors > 0 && groups && a && group_steps && skipped && workspace && out,
             "clip_adamw: bad args");
  MTTS_CHECK(a->ngroups > 0 && a->ngroups <= MTTS_ADAMW_MAX_GROUPS, "clip_adamw: 1..%d groups",
             MTTS_ADAMW_MAX_GROUPS);
  MTTS_CHECK(a->total_chunks > 0 && a->total_chunks < (1ll << 31), "clip_adamw: bad chunk count");
  MTTS_CHECK(a->clip_chunks >= 0 && a->clip_chunks <= a->total_chunks, "clip_adamw: clip_chunks outside the list");
  MTTS_CHECK(a->ngroups == 64 || (a->active_groups >> a->ngroups) == 0, "clip_adamw: active group past ngroups");
  const MttsLrSchedule& s = a->schedule;
  MTTS_CHECK(s.kind >= MTTS_LR_CONSTANT && s.kind <= MTTS_LR_INV_SQRT && s.warmup_steps >= 0,
             "clip_adamw: bad schedule");
  MTTS_CHECK((s.kind != MTTS_LR_COSINE && s.kind != MTTS_LR_LINEAR) || s.total_steps > s.warmup_steps,
             "clip_adamw: cosine / linear schedule needs total_steps > warmup_steps");
  MTTS_CHECK(s.min_ratio >= 0.0 && s.min_ratio <= 1.0, "clip_adamw: min_ratio outside [0, 1]");
  MTTS_CHECK(a->ema_decay >= 0.0 && a->ema_decay < 1.0, "clip_adamw: ema_decay outside [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  // the sum always runs: without clipping it still feeds the reported norm and the non-finite guard
  hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)a->total_chunks), dim3(kAdamBlock), 0, st, tensors, ntensors,
                     partial);
  MTTS_LAUNCH_CHECK("clip_adamw sumsq");
  AdamWHyper h;
  h.b1 = a->beta1;
  h.b2 = a->beta2;
  h.eps = a->eps;
  h.max_norm = a->max_norm;
  h.ngroups = a->ngroups;
  h.ema_warmup = a->ema_warmup;
  h.skip_nonfinite = a->skip_nonfinite;
  h.ema_decay = a->ema_decay;
  h.active = a->active_groups;
  h.sched = s;
  hipLaunchKernelGGL(adamw_final_kernel, dim3(1), dim3(kAdamBlock), 0, st, partial, a->total_chunks, a->clip_chunks,
                     groups, group_steps, skipped, h, out);
  MTTS_LAUNCH_CHECK("clip_adamw final");
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)a->total_chunks), dim3(kAdamBlock), 0, st, tensors, ntensors,
                     groups, out, a->beta1, a->beta2, a->eps);
  MTTS_LAUNCH_CHECK("clip_adamw adamw");
  return MTTS_OK;
}
