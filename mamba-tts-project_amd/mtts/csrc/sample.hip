// Token sampler in HIP: the end of an autoregressive decode step
// (mamba_decoder.py:188-256 returns logits and leaves the draw to the caller).
// One launch turns (rows, V) logits into one token per row: temperature,
// top-k, nucleus (top-p) and a Gumbel-max draw from a counter-based hash, so
// a float64 reference can reproduce every token (include/mtts.h, ABI 15).
//
// One workgroup per row: a single wave for V <= 256 (every reduction stays in
// the wave: no LDS round trip, no barrier), 4 waves for longer rows, so that a
// thread walks at most 4 entries per pass up to V = 1024 (one wave over 1024
// entries measured slower: 16 dependent LDS reads per pass and 16 Gumbel
// draws per lane, +99 us per token against +39).  A thread owns the entries
// v = tid + threads * j in every pass, so the row staged in LDS (V <= 4096;
// longer rows are re-read from L2) is per-thread storage and needs no barrier
// of its own.
//   * order-free selection: both filters are thresholds on the logit.  With
//     key(x) the monotone uint32 image of a float, top-k keeps key >= K, K the
//     smallest key with #{key_w > K} < top_k, and top-p keeps key >= K2, K2
//     the smallest key with sum_{key_w > K2} e_w < top_p * Z: two bisections
//     over the key space (<= 32 block reductions each, one barrier per
//     reduction on alternating LDS slots).  Ties share a key, so they stay or
//     go together, as the definition asks.
//   * the draw: u = ((h >> 40) + 0.5) * 2^-24 needs 25 significant bits above
//     1/2; there -log(u) is taken as -log1p(-(1 - u)) with 1 - u exact in
//     fp32, so the Gumbel noise is good to a few ulp over the whole range
//     (precise logf / log1pf, not v_log_f32).
//   * (score, index) pairs reduce as one uint64 max: key(score) << 32 | ~index
//     gives the largest score and, on ties, the lowest index.
// The step counter is read by every workgroup and advanced by a one-workgroup
// launch behind the sampler (which also recounts the unfinished rows), so
// nothing depends on the order in which workgroups run and there are no
// atomics in global memory.
//
// The same kernel has a per-row form (mtts_sample_tokens_rows): temperature,
// top-k, top-p, seed, draw count, repetition penalty and length cap are read
// per row from device arrays, and the Gumbel counter is the row's own
// (seed_r, draw_r, v).  The penalty window (<= 256 history columns) becomes a
// small LDS set before the first pass, and load() tests membership, so the
// LDS-staged row is penalised as it is staged and a longer row on every
// re-read; every pass downstream sees the penalised value.  The scalar form
// instantiates none of this.
//
// The slot form (mtts_sample_tokens_slots) is the per-row form for a decode
// session whose rows are requests admitted at different times: the history
// column is the row's own draw count instead of the shared step, a finished
// row keeps its history until the host has taken it, and the launch behind
// the sampler advances the positions of the unfinished rows only.  One more
// instantiation (kSlots); the other two compile none of it.
//
// The host side is one front end for the three entry points: the argument
// checks they share (check_sample_args, with the per-row and slot forms' own
// in check_sample_rows_args), one dtype x wave-count launch switch and one
// launch behind the sampler (launch_sample, sample_advance_kernel<kSlots>).
// An entry point holds its name and the few checks that are its alone.
//
// Token log-probabilities (mtts_sample_tokens*_lp, include/mtts.h): the same
// kernel with a fourth trait, kLogprob, whose parameter struct carries the two
// output pointers behind the form's own arguments.  Once the token is known
// the row is walked once more -- exp(x_v - m) summed per thread in the order of
// every other pass, one block_sum, and thread 0 forms (x_t - m) - log(sum) --
// on the row as load() made it (bias, NaN fold, penalty), at temperature 1 and
// before any truncation.  The instantiations without the trait compile none of
// it and keep their argument layout.
#include "common.h"

#include <math.h>

#include <string>
#include <type_traits>

namespace mtts {
namespace {

constexpr int kSampleThreads = 256;
constexpr int kSampleCache = 4096;   // row entries staged in LDS (4-wave form)
constexpr int kSampleWaveV = 256;    // longest row of the one-wave form (all of it staged)

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's finalizer (as dropout.hip)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// monotone image of a float: a < b  <=>  fkey(a) < fkey(b) (no NaN; -0 was folded into +0)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__device__ __forceinline__ uint64_t bits_of(uint64_t v) { return v; }
__device__ __forceinline__ uint64_t bits_of(uint32_t v) { return v; }
__device__ __forceinline__ uint64_t bits_of(float v) { return __float_as_uint(v); }
__device__ __forceinline__ void from_bits(uint64_t b, uint64_t& v) { v = b; }
__device__ __forceinline__ void from_bits(uint64_t b, uint32_t& v) { v = (uint32_t)b; }
__device__ __forceinline__ void from_bits(uint64_t b, float& v) { v = __uint_as_float((uint32_t)b); }

struct OpSum {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// Reduction over the workgroup's NW (1 or 4) waves in a fixed order (the same value in
// every thread, the same bits in every run).  One barrier per call: calls
// alternate between two slot rows, and a wave can only write a row again
// after every wave has passed the barrier of the call in between.
template <int NW, typename T, typename Op>
__device__ __forceinline__ T block_red(T v, Op op, uint64_t (*slots)[4], int& phase) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = op(v, __shfl_xor(v, o));
  if constexpr (NW == 1) return v;
  uint64_t* s = slots[phase];
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = bits_of(v);
  block_sync();
  T r0, r1, r2, r3;
  from_bits(s[0], r0); from_bits(s[1], r1); from_bits(s[2], r2); from_bits(s[3], r3);
  return op(op(r0, r1), op(r2, r3));
}

// The bisections' sums (32 + 32 of them per row): the wave part on DPP /
// permlane moves (common.h wave_sum) instead of six ds_bpermute round trips.
// A count goes through as a float: exact below 2^24, the vocabulary's bound.
template <int NW>
__device__ __forceinline__ float block_sum(float v, uint64_t (*slots)[4], int& phase) {
  v = wave_sum(v);
  if constexpr (NW == 1) return v;
  uint64_t* s = slots[phase];
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = bits_of(v);
  block_sync();
  float r0, r1, r2, r3;
  from_bits(s[0], r0); from_bits(s[1], r1); from_bits(s[2], r2); from_bits(s[3], r3);
  return (r0 + r1) + (r2 + r3);
}

// -log(-log(u)), u = (n + 0.5) * 2^-24 for the 24-bit n
__device__ __forceinline__ float gumbel(uint32_t n) {
  float a;
  if (n < (1u << 23)) {
    a = -logf((float)(2 * n + 1) * 0x1p-25f);                       // u <= 1/2: exact in fp32
  } else {
    a = -log1pf(-((float)(2 * ((1u << 24) - 1 - n) + 1) * 0x1p-25f));   // 1 - u exact
  }
  return -logf(a);
}

struct SampleParams {
  MttsSampleArgs a;
  static constexpr bool kRows = false;
  static constexpr bool kSlots = false;
  static constexpr bool kLogprob = false;
};
struct SampleRowsParams {   // the per-row form: controls read from device arrays (mtts_sample_tokens_rows)
  MttsSampleRowsArgs a;
  static constexpr bool kRows = true;
  static constexpr bool kSlots = false;
  static constexpr bool kLogprob = false;
};
struct SampleSlotsParams {  // the slot form: the per-row form on the row's own history column (mtts_sample_tokens_slots)
  MttsSampleRowsArgs a;
  static constexpr bool kRows = true;
  static constexpr bool kSlots = true;
  static constexpr bool kLogprob = false;
};
template <typename P>
struct WithLogprob : P {    // P's form that also writes the token's log-probability (mtts_sample_tokens*_lp)
  MttsSampleLogprobOut lp;
  static constexpr bool kLogprob = true;
};

// The per-row form's penalty window as a set: open addressing over kWinSlots
// LDS words (-1 = empty).  At most MTTS_SAMPLE_WINDOW_MAX = kWinSlots / 2
// distinct ids go in, so an empty word always ends a probe.  Which word an id
// lands in depends on the order of the inserts; whether it is found does not.
constexpr int kWinSlots = 512;
static_assert(kWinSlots >= 2 * MTTS_SAMPLE_WINDOW_MAX && (kWinSlots & (kWinSlots - 1)) == 0, "window set too small");
__device__ __forceinline__ uint32_t win_hash(int id) { return ((uint32_t)id * 0x9E3779B1u) >> 23; }   // 9 bits
__device__ __forceinline__ void win_insert(int* tab, int id) {
  uint32_t h = win_hash(id);
  for (int i = 0; i < kWinSlots; ++i) {
    const int old = atomicCAS(&tab[h], -1, id);
    if (old == -1 || old == id) return;
    h = (h + 1) & (kWinSlots - 1);
  }
}
__device__ __forceinline__ bool win_has(const int* tab, int id) {
  uint32_t h = win_hash(id);
  for (int i = 0; i < kWinSlots; ++i) {
    const int e = tab[h];
    if (e == id) return true;
    if (e == -1) return false;
    h = (h + 1) & (kWinSlots - 1);
  }
  return false;
}

template <typename T, int NW, typename P>
__global__ __launch_bounds__(NW * 64) void sample_kernel(const P prm) {
  constexpr int kThreads = NW * 64;
  constexpr int kCache = NW == 1 ? kSampleWaveV : kSampleCache;
  constexpr bool kRows = P::kRows;
  constexpr bool kSlots = P::kSlots;
  constexpr bool kLogprob = P::kLogprob;
  const auto& p = prm.a;
  __shared__ float xs[kCache];
  __shared__ float es[kCache];
  __shared__ uint64_t slots[2][4];
  __shared__ int wtab[kRows ? kWinSlots : 1];
  int phase = 0;
  const int row = blockIdx.x, tid = threadIdx.x, V = p.vocab;
  int step = 0, col;
  if constexpr (kSlots) {
    col = p.draw[row];   // the row's own column: neither *step nor step0 enters
  } else {
    step = p.step ? *p.step : 0;
    col = step - p.step0;
  }
  int64_t* const hist = (p.history && col >= 0 && col < p.hist_cols) ? p.history + (int64_t)row * p.hist_ld + col
                                                                     : nullptr;
  int64_t* const tok_out = p.tokens + (int64_t)row * p.tok_stride;
  float* lp_out = nullptr;    // this launch's log-probability and its history column: the token's column, by the same rule
  float* lp_hist = nullptr;
  if constexpr (kLogprob) {
    if (prm.lp.logprob) lp_out = prm.lp.logprob + row;
    if (prm.lp.logprob_history && col >= 0 && col < p.hist_cols)
      lp_hist = prm.lp.logprob_history + (int64_t)row * prm.lp.lp_ld + col;
  }
  // this row's controls: kernel arguments, or (per-row form) device arrays with
  // the header's effective rules, so that no value can index or loop out of range.
  // All read here, the length cap included, in one batch of loads.
  float T_, top_p_, theta = 1.f;
  int top_k_, drawn = 0;
  int64_t cap = INT64_MAX;
  if constexpr (kRows) {
    T_ = p.temperature[row];
    top_k_ = p.top_k[row];
    top_p_ = p.top_p[row];
    drawn = p.draw[row];
    if (p.penalty) theta = p.penalty[row];
    if (p.max_length) cap = p.max_length[row];
    if (!(top_p_ > 0.f && top_p_ < 1.f)) top_p_ = 1.f;
  } else {
    T_ = p.temperature;
    top_k_ = p.top_k;
    top_p_ = p.top_p;
  }
  if (p.finished && p.finished[row] != 0) {   // past its end of sequence: pad, length frozen
    if (tid == 0) {
      *tok_out = p.pad_id;
      if constexpr (!kSlots) {   // a slot keeps its finished request's tokens until the host takes them
        if (hist) *hist = p.pad_id;
      }
      if constexpr (kLogprob) {   // 0.0 wherever pad_id went
        if (lp_out) *lp_out = 0.f;
        if constexpr (!kSlots) {
          if (lp_hist) *lp_hist = 0.f;
        }
      }
    }
    return;
  }
  const T* __restrict__ lg = reinterpret_cast<const T*>(p.logits) + (int64_t)row * p.ld;
  const float* __restrict__ bias = p.bias ? p.bias + (int64_t)row * p.bias_ld : nullptr;
  const bool cached = V <= kCache;
  bool pen = false;   // the repetition penalty applies to this row (uniform in the workgroup)
  if constexpr (kRows) {
    int n = p.window < MTTS_SAMPLE_WINDOW_MAX ? p.window : MTTS_SAMPLE_WINDOW_MAX;
    n = n < drawn ? n : drawn;
    n = n < col ? n : col;
    pen = theta > 0.f && theta != 1.f && theta < INFINITY && n > 0 && p.history != nullptr;
    if (pen) {
      for (int i = tid; i < kWinSlots; i += kThreads) wtab[i] = -1;
      block_sync();
      const int64_t* const hrow = p.history + (int64_t)row * p.hist_ld;
      for (int j = tid; j < n; j += kThreads) {
        const int c = col - n + j;                     // >= 0: n <= col
        if (c >= p.hist_cols) continue;
        const int64_t id = hrow[c];
        if (id >= 0 && id < (int64_t)V) win_insert(wtab, (int)id);   // checked before it indexes anything
      }
      block_sync();
    }
  }
  auto load = [&](int v) {
    float x = ldf(lg + v);
    if (bias) x += bias[v];
    if (!(x == x)) x = -INFINITY;   // NaN counts as -inf
    if constexpr (kRows) {
      if (pen && win_has(wtab, v)) x = x > 0.f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta);
    }
    if (x == 0.f) x = 0.f;          // -0 and +0 tie: one key
    return x;
  };
  auto X = [&](int v) { return cached ? xs[v] : load(v); };

  // row maximum and its lowest index
  uint64_t best = 0;
  for (int v = tid; v < V; v += kThreads) {
    const float x = load(v);
    if (cached) xs[v] = x;
    const uint64_t c = ((uint64_t)fkey(x) << 32) | (uint32_t)~(uint32_t)v;
    best = c > best ? c : best;
  }
  best = block_red<NW>(best, OpMax(), slots, phase);
  const uint32_t kmax = (uint32_t)(best >> 32);
  const float m = unkey(kmax);
  int64_t token = (int64_t)(uint32_t)~(uint32_t)best;
  if (m == -INFINITY) {
    token = p.pad_id;               // no finite candidate
  } else if (T_ > 0.f && m < INFINITY) {
    const float invT = 1.f / T_;
    uint32_t K = 0;
    if (top_k_ > 0 && top_k_ < V) {
      const uint32_t k = (uint32_t)top_k_;
      uint32_t lo = 0, hi = kmax;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t cnt = 0;
#pragma unroll 4
        for (int v = tid; v < V; v += kThreads) cnt += fkey(X(v)) > mid ? 1u : 0u;
        if ((uint32_t)block_sum<NW>((float)cnt, slots, phase) < k) hi = mid; else lo = mid + 1;
      }
      K = lo;
    }
    if (top_p_ < 1.f) {
      // e_v = exp((x_v - m) / T) over the top-k survivors (0 elsewhere; exp(-inf) = 0)
      auto E = [&](int v, float x) { return fkey(x) >= K ? expf((x - m) * invT) : 0.f; };
      float z = 0.f;
      for (int v = tid; v < V; v += kThreads) {
        const float e = E(v, X(v));
        if (cached) es[v] = e;
        z += e;
      }
      z = block_sum<NW>(z, slots, phase);
      const float target = top_p_ * z;
      uint32_t lo = K, hi = kmax;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        float s = 0.f;
#pragma unroll 4
        for (int v = tid; v < V; v += kThreads) {
          const float x = X(v);
          if (fkey(x) > mid) s += cached ? es[v] : E(v, x);
        }
        s = block_sum<NW>(s, slots, phase);
        if (s < target) hi = mid; else lo = mid + 1;
      }
      K = lo;
    }
    // Gumbel-max draw over the kept set
    uint64_t seed, c0;
    if constexpr (kRows) {   // the row's own stream: (seed_r, draw_r, v), wherever the row sits
      seed = (uint64_t)p.seed[row];
      c0 = (uint64_t)(int64_t)drawn * (uint64_t)V;
    } else {
      seed = p.seed ? (uint64_t)*p.seed : 0ull;
      c0 = ((uint64_t)(int64_t)step * (uint64_t)p.rows + (uint64_t)row) * (uint64_t)V;
    }
    uint64_t pick = 0;
    for (int v = tid; v < V; v += kThreads) {
      const float x = X(v);
      if (x > -INFINITY && fkey(x) >= K) {
        const uint64_t h = mix64(seed + (c0 + (uint64_t)v) * 0x9E3779B97F4A7C15ull);
        const float score = x / T_ + gumbel((uint32_t)(h >> 40));
        const uint64_t c = ((uint64_t)fkey(score) << 32) | (uint32_t)~(uint32_t)v;
        pick = c > pick ? c : pick;
      }
    }
    pick = block_red<NW>(pick, OpMax(), slots, phase);
    token = (int64_t)(uint32_t)~(uint32_t)pick;   // the row maximum is always kept: pick != 0
  }
  if constexpr (kLogprob) {
    // log softmax(x)[token] at temperature 1 over the whole row; m not finite (no
    // finite candidate, or a +inf logit): NaN.  Before the bookkeeping below.
    float lp = __builtin_nanf("");
    if (m > -INFINITY && m < INFINITY) {
      float z = 0.f;
      for (int v = tid; v < V; v += kThreads) z += expf(X(v) - m);   // exp(-inf) = 0
      z = block_sum<NW>(z, slots, phase);
      // xs[token] was staged by another thread: four waves have passed the
      // barrier of the sum above since, one wave has met none yet
      if constexpr (NW == 1) block_sync();
      if (tid == 0) lp = (X((int)token) - m) - logf(z);
    }
    if (tid == 0) {
      if (lp_out) *lp_out = lp;
      if (lp_hist) *lp_hist = lp;
    }
  }
  if (tid == 0) {
    *tok_out = token;
    if (hist) *hist = token;
    if constexpr (kRows) {
      p.draw[row] = drawn + 1;
      if (p.length) {
        const int64_t len = p.length[row] + 1;
        p.length[row] = len;
        if (p.finished && len >= cap) p.finished[row] = 1;
      }
    } else {
      if (p.length) p.length[row] += 1;
    }
    if (p.finished && p.eos_id >= 0 && token == p.eos_id) p.finished[row] = 1;
  }
}

// Behind the sampler: count the unfinished rows and advance the counters
// (pos_rows > 0: `pos` holds that many per-row positions, all moved in lockstep).
// kGateOnFinished, the slot form's: a per-row position moves only when its row
// is unfinished after the draw, so a row idling past its end stays inside
// pos_embed however long its slot waits for a request.
template <bool kGateOnFinished>
__global__ __launch_bounds__(kSampleThreads) void sample_advance_kernel(int* step, int* pos, const int* finished,
                                                                        int rows, int* unfinished, int advance,
                                                                        int pos_rows) {
  __shared__ uint64_t slots[2][4];
  int phase = 0;
  uint32_t done = 0;
  if (unfinished) {
    for (int r = threadIdx.x; r < rows; r += kSampleThreads) done += finished[r] != 0 ? 1u : 0u;
    done = block_red<4>(done, OpSum(), slots, phase);
  }
  if (threadIdx.x == 0) {
    if (unfinished) *unfinished = rows - (int)done;
    if (advance) {
      if (step) *step += 1;
      if (pos && pos_rows <= 0) *pos += 1;
    }
  }
  if (advance && pos && pos_rows > 0)
    for (int r = threadIdx.x; r < pos_rows; r += kSampleThreads)
      if (!kGateOnFinished || !finished || finished[r] == 0) pos[r] += 1;
}

// ---- host side: one front end for the three entry points --------------------
// Each helper returns the status of its first failing check (MTTS_CHECK returns
// from the function it stands in) and the entry point hands it on; `name` is
// the entry point's, so every message keeps its prefix, and the checks fire in
// the order they always had: null pointers, [per-row arrays], dtype, sizes,
// strides, [the form's own: `form_checks`], ids, history, unfinished.
template <typename A, typename F>
int check_sample_args(const A* a, const char* name, F form_checks) {
  MTTS_CHECK(a && a->logits && a->tokens, "%s: null pointer", name);
  if constexpr (std::is_same_v<A, MttsSampleRowsArgs>)
    MTTS_CHECK(a->temperature && a->top_k && a->top_p && a->seed && a->draw,
               "%s: temperature, top_k, top_p, seed and draw are required", name);
  MTTS_CHECK(a->dtype == MTTS_F32 || a->dtype == MTTS_BF16, "%s: dtype must be f32 or bf16", name);
  MTTS_CHECK(a->rows >= 1 && a->vocab >= 1 && a->vocab <= (1 << 24), "%s: rows=%d vocab=%d out of range", name,
             a->rows, a->vocab);
  MTTS_CHECK(a->ld >= a->vocab && a->bias_ld >= 0 && (a->bias_ld == 0 || a->bias_ld >= a->vocab),
             "%s: row stride below vocab", name);
  if (const int s = form_checks()) return s;
  MTTS_CHECK(a->pad_id >= 0 && a->pad_id < a->vocab && a->eos_id < a->vocab,
             "%s: pad_id=%d / eos_id=%d outside the vocabulary", name, a->pad_id, a->eos_id);
  MTTS_CHECK(!a->history || (a->hist_cols >= 0 && a->hist_ld >= a->hist_cols), "%s: bad history shape", name);
  MTTS_CHECK(!a->unfinished || a->finished, "%s: unfinished needs finished", name);
  return MTTS_OK;
}

// The per-row and slot forms: the checks above around their window and length-cap rules.
int check_sample_rows_args(const MttsSampleRowsArgs* a, const char* name) {
  return check_sample_args(a, name, [=]() -> int {
    MTTS_CHECK(a->window >= 0 && a->window <= MTTS_SAMPLE_WINDOW_MAX, "%s: window=%d outside [0, %d]", name,
               a->window, MTTS_SAMPLE_WINDOW_MAX);
    MTTS_CHECK(a->window == 0 || a->history, "%s: window=%d needs history", name, a->window);
    MTTS_CHECK(!a->max_length || (a->finished && a->length), "%s: max_length needs finished and length", name);
    return MTTS_OK;
  });
}

// The _lp entry points' own checks, behind every check of the form they extend.
template <typename A>
int check_logprob_out(const A* a, const MttsSampleLogprobOut* lp, const char* name) {
  MTTS_CHECK(lp && (lp->logprob || lp->logprob_history), "%s: no logprob output", name);
  MTTS_CHECK(!lp->logprob_history || lp->lp_ld >= a->hist_cols, "%s: bad logprob history shape", name);
  return MTTS_OK;
}

// One dtype x wave-count switch (one wave up to kSampleWaveV entries, else four).
template <typename P>
void launch_sample_kernel(const P& prm, hipStream_t st) {
  const bool f32 = prm.a.dtype == MTTS_F32;
  const dim3 grid(prm.a.rows);
  if (prm.a.vocab <= kSampleWaveV) {
    if (f32) hipLaunchKernelGGL((sample_kernel<float, 1, P>), grid, dim3(64), 0, st, prm);
    else hipLaunchKernelGGL((sample_kernel<bf16_t, 1, P>), grid, dim3(64), 0, st, prm);
  } else {
    if (f32) hipLaunchKernelGGL((sample_kernel<float, 4, P>), grid, dim3(kSampleThreads), 0, st, prm);
    else hipLaunchKernelGGL((sample_kernel<bf16_t, 4, P>), grid, dim3(kSampleThreads), 0, st, prm);
  }
}

// The sampler for P's form -- with `lp`, the instantiation that also writes the
// log-probabilities -- and, when asked for, the launch behind it.
template <typename P, typename A>
int launch_sample(const A* a, const char* name, hipStream_t st, const MttsSampleLogprobOut* lp = nullptr) {
  if (lp) {
    WithLogprob<P> prm;
    prm.a = *a;
    prm.lp = *lp;
    launch_sample_kernel(prm, st);
  } else {
    P prm;
    prm.a = *a;
    launch_sample_kernel(prm, st);
  }
  MTTS_LAUNCH_CHECK(name);
  if (a->advance || a->unfinished) {
    hipLaunchKernelGGL(sample_advance_kernel<P::kSlots>, dim3(1), dim3(kSampleThreads), 0, st, a->step, a->pos,
                       a->finished, a->rows, a->unfinished, a->advance, a->pos_rows);
    MTTS_LAUNCH_CHECK((std::string(name) + " (advance)").c_str());
  }
  return MTTS_OK;
}

}  // namespace
}  // namespace mtts

using namespace mtts;

// Each form's entry point and its _lp twin share one body: `want_lp` adds the
// two checks of the outputs behind all of the form's own.
static int sample_tokens_entry(const MttsSampleArgs* a, const char* name, bool want_lp,
                               const MttsSampleLogprobOut* lp, void* stream) {
  const int s = check_sample_args(a, name, [=]() -> int {
    MTTS_CHECK(a->temperature >= 0.f, "%s: temperature=%f must be >= 0", name, (double)a->temperature);
    MTTS_CHECK(a->top_k >= 0, "%s: top_k=%d must be >= 0", name, a->top_k);
    MTTS_CHECK(a->top_p > 0.f && a->top_p <= 1.f, "%s: top_p=%f must be in (0, 1]", name, (double)a->top_p);
    return MTTS_OK;
  });
  if (s) return s;
  MTTS_CHECK(!a->advance || a->step, "%s: advance needs step", name);
  MTTS_CHECK(a->pos_rows >= 0, "%s: pos_rows=%d must be >= 0", name, a->pos_rows);
  if (want_lp)
    if (const int e = check_logprob_out(a, lp, name)) return e;
  return launch_sample<SampleParams>(a, name, (hipStream_t)stream, want_lp ? lp : nullptr);
}

static int sample_tokens_rows_entry(const MttsSampleRowsArgs* a, const char* name, bool want_lp,
                                    const MttsSampleLogprobOut* lp, void* stream) {
  if (const int s = check_sample_rows_args(a, name)) return s;
  MTTS_CHECK(!a->advance || a->step, "%s: advance needs step", name);
  MTTS_CHECK(a->pos_rows >= 0, "%s: pos_rows=%d must be >= 0", name, a->pos_rows);
  if (want_lp)
    if (const int e = check_logprob_out(a, lp, name)) return e;
  return launch_sample<SampleRowsParams>(a, name, (hipStream_t)stream, want_lp ? lp : nullptr);
}

static int sample_tokens_slots_entry(const MttsSampleRowsArgs* a, const char* name, bool want_lp,
                                     const MttsSampleLogprobOut* lp, void* stream) {
  if (const int s = check_sample_rows_args(a, name)) return s;
  MTTS_CHECK(!(a->advance && a->pos) || a->pos_rows == 0 || a->pos_rows == a->rows,
             "%s: pos_rows=%d must be 0 or rows=%d", name, a->pos_rows, a->rows);
  if (want_lp)
    if (const int e = check_logprob_out(a, lp, name)) return e;
  return launch_sample<SampleSlotsParams>(a, name, (hipStream_t)stream, want_lp ? lp : nullptr);
}

extern "C" int mtts_sample_tokens(const MttsSampleArgs* a, void* stream) {
  return sample_tokens_entry(a, "sample_tokens", false, nullptr, stream);
}
extern "C" int mtts_sample_tokens_rows(const MttsSampleRowsArgs* a, void* stream) {
  return sample_tokens_rows_entry(a, "sample_tokens_rows", false, nullptr, stream);
}
extern "C" int mtts_sample_tokens_slots(const MttsSampleRowsArgs* a, void* stream) {
  return sample_tokens_slots_entry(a, "sample_tokens_slots", false, nullptr, stream);
}
extern "C" int mtts_sample_tokens_lp(const MttsSampleArgs* a, const MttsSampleLogprobOut* lp, void* stream) {
  return sample_tokens_entry(a, "sample_tokens_lp", true, lp, stream);
}
extern "C" int mtts_sample_tokens_rows_lp(const MttsSampleRowsArgs* a, const MttsSampleLogprobOut* lp,
                                          void* stream) {
  return sample_tokens_rows_entry(a, "sample_tokens_rows_lp", true, lp, stream);
}
extern "C" int mtts_sample_tokens_slots_lp(const MttsSampleRowsArgs* a, const MttsSampleLogprobOut* lp,
                                           void* stream) {
  return sample_tokens_slots_entry(a, "sample_tokens_slots_lp", true, lp, stream);
}
