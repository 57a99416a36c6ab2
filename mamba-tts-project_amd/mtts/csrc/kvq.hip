// Conditioning K / V as OCP FP8 (e4m3fn) with one fp32 scale per (row, head)
// (include/mtts.h mtts_kv_quantize_fp8): what the fp8 instantiation of the
// split-key single-query attention (attn.hip) reads.  Two launches over
// (row * head, chunk of kChunk keys) workgroups, so one admitted request at
// 5248 keys and 8 heads runs on 168 workgroups, not 8:
//   1. kvq_amax_kernel: max |x| of the chunk's counted keys, as the bits of
//      the absolute value (for non-negative floats the unsigned order is the
//      float order, infinities and NaNs sort last): exact in any order.
//   2. kvq_convert_kernel: every workgroup reduces its row's few partials to
//      the scale, divides (IEEE), rounds to e4m3fn in integer arithmetic and
//      stores the chunk head-major, 8 bytes per lane; zero bytes from the
//      row's count to kv_len.
// A lane owns 8 consecutive columns of one key (16-byte loads for bf16, two
// for fp32), head_dim / 8 lanes a key, as the decode attention kernels.
#include <type_traits>

#include "common.h"

namespace {

using mtts::bf16_t;

constexpr int kChunk = 256;   // keys per workgroup

// fp32 -> e4m3fn code, round to nearest even: 0x7F / 0xFF (NaN) from 480 up in
// magnitude (464..480 round to the code of 480, which is the NaN code) and for
// NaN, no infinity; below 2^-6 the subnormal codes in steps of 2^-9, rounded
// by one fp32 add of 2^14 (whose ulp is 2^-9).  The bits torch's cast to
// float8_e4m3fn gives.
__host__ __device__ __forceinline__ uint32_t f32_to_e4m3fn(float f) {
#ifdef __HIP_DEVICE_COMPILE__
  uint32_t u = __float_as_uint(f);
#else
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
#endif
  const uint32_t sign = (u >> 24) & 0x80u;
  u &= 0x7fffffffu;
  uint32_t r;
  if (u >= 0x43f00000u) {          // >= 480, infinity, NaN
    r = 0x7fu;
  } else if (u < 0x3c800000u) {    // < 2^-6: subnormal codes
#ifdef __HIP_DEVICE_COMPILE__
    r = __float_as_uint(__uint_as_float(u) + 16384.f) - 0x46800000u;
#else
    float g;
    __builtin_memcpy(&g, &u, 4);
    g += 16384.f;
    __builtin_memcpy(&r, &g, 4);
    r -= 0x46800000u;
#endif
  } else {                         // rebias 127 -> 7, round the 20 dropped bits to even
    const uint32_t odd = (u >> 20) & 1u;
    r = (u - 0x3c000000u + 0x7ffffu + odd) >> 20;
  }
  return r | sign;
}

template <typename T>
__device__ __forceinline__ void ld8(const T* p, float* v) {
  if constexpr (std::is_same<T, bf16_t>::value) {
    const uint4 x = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) v[2 * e] = __uint_as_float(w[e] << 16), v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
  } else {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
}

__device__ __forceinline__ int row_keys(const int32_t* kv_lens, int r, int kv_len) {
  if (!kv_lens) return kv_len;
  const int n = kv_lens[r];
  return n < 0 ? 0 : (n < kv_len ? n : kv_len);
}

__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
    v = v > w ? v : w;
  }
  return v;
}

template <typename T, int HD>
__global__ __launch_bounds__(256) void kvq_amax_kernel(MttsKvQuantizeFp8Args a, uint32_t* part, int nchunk) {
  constexpr int G = HD / 8, NG = 256 / G;
  __shared__ uint32_t sw[4];
  const int rh = blockIdx.x, chunk = blockIdx.y, r = rh / a.heads, h = rh % a.heads;
  const int n = row_keys(a.kv_lens, r, a.kv_len), k0 = chunk * kChunk;
  const int k1 = k0 + kChunk < n ? k0 + kChunk : n;
  const int g = threadIdx.x / G, d0 = threadIdx.x % G * 8;
  const T* xb = (const T*)a.x + (int64_t)r * a.x_bs + h * HD + d0;
  uint32_t m = 0;
  for (int j = k0 + g; j < k1; j += NG) {
    float v[8];
    ld8(xb + (int64_t)j * a.x_ls, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t u = __float_as_uint(v[e]) & 0x7fffffffu;
      m = m > u ? m : u;
    }
  }
  m = wave_umax(m);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = m;
  mtts::block_sync();
  if (threadIdx.x == 0) {
    const uint32_t a01 = sw[0] > sw[1] ? sw[0] : sw[1], a23 = sw[2] > sw[3] ? sw[2] : sw[3];
    part[(int64_t)rh * nchunk + chunk] = a01 > a23 ? a01 : a23;   // 0 for a chunk at or past the count
  }
}

template <typename T, int HD>
__global__ __launch_bounds__(256) void kvq_convert_kernel(MttsKvQuantizeFp8Args a, const uint32_t* part, int nchunk) {
  constexpr int G = HD / 8, NG = 256 / G;
  const int rh = blockIdx.x, chunk = blockIdx.y, r = rh / a.heads, h = rh % a.heads;
  const int n = row_keys(a.kv_lens, r, a.kv_len), k0 = chunk * kChunk;
  const int k1 = k0 + kChunk < a.kv_len ? k0 + kChunk : a.kv_len;
  uint32_t m = 0;
  for (int i = 0; i < nchunk; ++i) {   // the same few words in every thread: exact, so no order to keep
    const uint32_t u = part[(int64_t)rh * nchunk + i];
    m = m > u ? m : u;
  }
  const float scale = m == 0 ? 1.f : (m >= 0x7f800000u ? __uint_as_float(0x7fc00000u) : __uint_as_float(m) / 448.f);
  if (chunk == 0 && threadIdx.x == 0) a.scale[(int64_t)r * a.scale_bs + h] = scale;
  const int g = threadIdx.x / G, d0 = threadIdx.x % G * 8;
  const T* xb = (const T*)a.x + (int64_t)r * a.x_bs + h * HD + d0;
  uint8_t* ob = a.out + (int64_t)r * a.out_bs + (int64_t)h * a.kv_len * HD + d0;
  for (int j = k0 + g; j < k1; j += NG) {
    uint2 w = make_uint2(0u, 0u);
    if (j < n) {
      float v[8];
      ld8(xb + (int64_t)j * a.x_ls, v);
      uint32_t c[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) c[e] = f32_to_e4m3fn(v[e] / scale);
      w.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
      w.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    }
    *reinterpret_cast<uint2*>(ob + (int64_t)j * HD) = w;
  }
}

int chunks_of(int kv_len) { return kv_len > 0 ? (kv_len + kChunk - 1) / kChunk : 1; }

template <typename T, int HD>
void launch(const MttsKvQuantizeFp8Args* a, hipStream_t st) {
  const int nchunk = chunks_of(a->kv_len);
  const dim3 grid(a->rows * a->heads, nchunk);
  uint32_t* part = (uint32_t*)a->workspace;
  hipLaunchKernelGGL((kvq_amax_kernel<T, HD>), grid, dim3(256), 0, st, *a, part, nchunk);
  hipLaunchKernelGGL((kvq_convert_kernel<T, HD>), grid, dim3(256), 0, st, *a, (const uint32_t*)part, nchunk);
}

template <typename T>
void dispatch(const MttsKvQuantizeFp8Args* a, hipStream_t st) {
  switch (a->head_dim) {
    case 16: launch<T, 16>(a, st); break;
    case 32: launch<T, 32>(a, st); break;
    case 64: launch<T, 64>(a, st); break;
    default: launch<T, 128>(a, st); break;
  }
}

bool head_dim_ok(int hd) { return hd == 16 || hd == 32 || hd == 64 || hd == 128; }

}  // namespace

extern "C" int64_t mtts_kv_quantize_fp8_workspace(int rows, int heads, int head_dim, int kv_len) {
  if (rows < 0 || heads <= 0 || kv_len < 0 || !head_dim_ok(head_dim)) return 0;
  return (int64_t)rows * heads * chunks_of(kv_len) * 4;
}

extern "C" int mtts_kv_quantize_fp8(const MttsKvQuantizeFp8Args* a, void* stream) {
  MTTS_CHECK(a, "kv_quantize_fp8: null args");
  MTTS_CHECK(a->dtype == MTTS_F32 || a->dtype == MTTS_BF16, "kv_quantize_fp8: dtype must be F32 or BF16");
  MTTS_CHECK(head_dim_ok(a->head_dim), "kv_quantize_fp8: head_dim %d not in {16,32,64,128}", a->head_dim);
  MTTS_CHECK(a->rows >= 0 && a->heads > 0 && a->kv_len >= 0, "kv_quantize_fp8: bad sizes (rows %d, heads %d, kv_len %d)",
             a->rows, a->heads, a->kv_len);
  if (a->rows == 0 || a->kv_len == 0) return MTTS_OK;
  MTTS_CHECK(a->x && a->out && a->scale, "kv_quantize_fp8: null x / out / scale");
  const int64_t al = a->dtype == MTTS_BF16 ? 8 : 4;
  MTTS_CHECK(((uintptr_t)a->x & 15) == 0 && a->x_bs % al == 0 && a->x_ls % al == 0,
             "kv_quantize_fp8: x and its strides x_bs / x_ls must be 16-byte aligned");
  const int64_t row_bytes = (int64_t)a->heads * a->kv_len * a->head_dim;
  MTTS_CHECK(((uintptr_t)a->out & 7) == 0 && a->out_bs % 8 == 0 && a->out_bs >= row_bytes,
             "kv_quantize_fp8: out and out_bs must be 8-byte aligned, out_bs >= %lld bytes", (long long)row_bytes);
  MTTS_CHECK(((uintptr_t)a->scale & 3) == 0 && a->scale_bs >= a->heads,
             "kv_quantize_fp8: scale must be 4-byte aligned, scale_bs >= heads = %d", a->heads);
  MTTS_CHECK(!a->kv_lens || ((uintptr_t)a->kv_lens & 3) == 0, "kv_quantize_fp8: kv_lens must be 4-byte aligned");
  const int64_t need = mtts_kv_quantize_fp8_workspace(a->rows, a->heads, a->head_dim, a->kv_len);
  MTTS_CHECK(a->workspace && ((uintptr_t)a->workspace & 3) == 0 && a->workspace_bytes >= need,
             "kv_quantize_fp8: workspace of %lld bytes, need %lld (4-byte aligned, mtts_kv_quantize_fp8_workspace)",
             (long long)(a->workspace ? a->workspace_bytes : 0), (long long)need);
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == MTTS_BF16) dispatch<bf16_t>(a, st);
  else dispatch<float>(a, st);
  MTTS_LAUNCH_CHECK("kv_quantize_fp8");
  return MTTS_OK;
}
