// LayerNorm forward/backward, fp32 statistics (SURVEY.md §2.7 K3;
// nanoGPT LayerNorm: F.layer_norm(x, w.shape, w, b, 1e-5), optional bias).
//
// Residual-stream dtype XT: the normalised output h and the branch tensors are
// bf16, the residual stream x / s = x + branch and its gradient are XT — fp32 by
// default, which is nanoGPT's autocast contract (fp32 embedding output, fp32 + bf16
// residual adds, fp32 LayerNorm input), or bf16 (opt-in, half the residual bytes).
// With XT = fp32 the fused backward writes the residual gradient in fp32 and, for
// the branch GEMMs, a bf16 copy of it in the same pass.
//
// Layout: one 64-lane wave owns one row; lane l holds columns
// (k*64 + l)*8 .. +8 for k < NK, so a row of C <= 512*NK bf16 values lives in
// registers (NK*8 floats per lane) and is read from HBM exactly once.
// 4 waves (rows) per 256-thread block -> N/4 blocks (3072 for GPT-2 124M),
// far more than the 256 CUs.
//
// Backward: dx = rstd * (dy*w - mean(dy*w) - xhat * mean(dy*w*xhat)) per row;
// dw = sum_rows dy*xhat, db = sum_rows dy are accumulated per lane in
// registers across the rows a block visits, reduced across the block's 4
// waves in LDS and written as one partial row per block; nsa_colsum_accum then
// reduces the partial rows (split over row ranges, fp32 atomics) into the flat
// gradient buffer.  Backward rows are software-pipelined (next row's loads in
// flight while the current row is reduced).
//
// Widths: C % 8 == 0; forward C <= 8192 (16 register groups), backward C <= 5120 (its
// 2 x [4][C] fp32 accumulators are 32·C bytes of the workgroup's 160 KiB of LDS); wider
// backward calls return hipErrorInvalidValue before any launch.
#include <type_traits>

#include "common.h"

namespace {

// 8 consecutive elements of a bf16 or fp32 row as raw 16-byte words
template <typename T>
struct Raw8 {
  static constexpr int W = sizeof(T) / 2;  // uint4 words: 1 for bf16, 2 for fp32
  uint4 u[W];
};

template <typename T>
__device__ __forceinline__ Raw8<T> ld_raw(const T* p) {
  Raw8<T> r;
#pragma unroll
  for (int i = 0; i < Raw8<T>::W; ++i) r.u[i] = reinterpret_cast<const uint4*>(p)[i];
  return r;
}

__device__ __forceinline__ void unpack_raw(const Raw8<bf16_t>& r, float (&f)[8]) { unpack8(r.u[0], f); }
__device__ __forceinline__ void unpack_raw(const Raw8<float>& r, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    f[4 * i + 0] = __uint_as_float(r.u[i].x);
    f[4 * i + 1] = __uint_as_float(r.u[i].y);
    f[4 * i + 2] = __uint_as_float(r.u[i].z);
    f[4 * i + 3] = __uint_as_float(r.u[i].w);
  }
}

__device__ __forceinline__ void load8x(const bf16_t* p, float (&f)[8]) { load8(p, f); }
__device__ __forceinline__ void load8x(const float* p, float (&f)[8]) { unpack_raw(ld_raw(p), f); }
__device__ __forceinline__ void store8x(bf16_t* p, const float (&f)[8]) { store8(p, f); }
__device__ __forceinline__ void store8x(float* p, const float (&f)[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}

// nontemporal variants (NT): the residual stream, its gradient and the branch tensors are
// streamed once per pass; the normalised output and the bf16 gradient copy (read by the
// next GEMM) keep normal stores
typedef unsigned ln_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 ld16n(const void* p) {
  if constexpr (NT) {
    const ln_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const ln_u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const uint4*>(p);
  }
}
template <bool NT>
__device__ __forceinline__ void st16n(void* p, uint4 u) {
  if constexpr (NT) {
    ln_u32x4 v;
    v.x = u.x;
    v.y = u.y;
    v.z = u.z;
    v.w = u.w;
    __builtin_nontemporal_store(v, reinterpret_cast<ln_u32x4*>(p));
  } else {
    *reinterpret_cast<uint4*>(p) = u;
  }
}
template <bool NT, typename T>
__device__ __forceinline__ Raw8<T> ld_raw_n(const T* p) {
  Raw8<T> r;
#pragma unroll
  for (int i = 0; i < Raw8<T>::W; ++i) r.u[i] = ld16n<NT>(reinterpret_cast<const uint4*>(p) + i);
  return r;
}
template <bool NT, bool H = false>
__device__ __forceinline__ void load8n(const bf16_t* p, float (&f)[8]) { unpack8e<H>(ld16n<NT>(p), f); }
template <bool NT>
__device__ __forceinline__ void load8xn(const bf16_t* p, float (&f)[8]) { load8n<NT>(p, f); }
template <bool NT>
__device__ __forceinline__ void load8xn(const float* p, float (&f)[8]) { unpack_raw(ld_raw_n<NT>(p), f); }
template <bool NT>
__device__ __forceinline__ void store8xn(bf16_t* p, const float (&f)[8]) {
  st16n<NT>(p, make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7])));
}
template <bool NT>
__device__ __forceinline__ void store8xn(float* p, const float (&f)[8]) {
  st16n<NT>(p, make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])));
  st16n<NT>(p + 4,
            make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]), __float_as_uint(f[6]), __float_as_uint(f[7])));
}

// Split-plane fp32 residual gradient (bf16 compute, fp32 stream).  An [N, C] fp32 gradient
// is stored as two 16-bit planes in the same 4·N·C bytes: hi = bf16(g) (the branch GEMMs'
// operand, read in place), then lo = bits(g) − (hi << 16) as int16, so hi, lo give g back bit
// for bit.  hi rounds to nearest with ties away from zero ((bits + 0x8000) >> 16): then lo
// spans exactly [−0x8000, 0x7fff] — round-to-nearest-even would need the 65537th value
// +0x8000 at a tie rounded down.  It differs from torch's bf16 cast only at exact ties (low 16
// bits 0x8000); infinities round-trip, a NaN keeps a quiet-NaN hi and decodes to a NaN.  The
// backward thereby writes 4 bytes per element where fp32 + a bf16 copy wrote 6.
__device__ __forceinline__ void split8(const float (&f)[8], uint4& hi, uint4& lo) {
  uint32_t h[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t u = __float_as_uint(f[j]);
    h[j] = (u & 0x7fffffffu) > 0x7f800000u ? ((u >> 16) | 0x40u) : ((u + 0x8000u) >> 16);
    l[j] = (u - (h[j] << 16)) & 0xffffu;
  }
  hi = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  lo = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
}
__device__ __forceinline__ void unsplit8(uint4 hi, uint4 lo, float (&f)[8]) {
  const uint32_t hw[4] = {hi.x, hi.y, hi.z, hi.w}, lw[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int32_t l0 = (int32_t)(int16_t)(lw[i] & 0xffffu), l1 = (int32_t)(int16_t)(lw[i] >> 16);
    f[2 * i] = __uint_as_float((hw[i] << 16) + (uint32_t)l0);
    f[2 * i + 1] = __uint_as_float((hw[i] & 0xffff0000u) + (uint32_t)l1);
  }
}

// The fp16-compute form (dtype float16): hi = fp16(g) rounded to nearest even (torch's cast:
// the branch GEMMs' fp16 operand), lo = (g - hi) * 2^(39 - E) as int16, E = hi's exponent
// field (at least 1).  g - hi is exact (Sterbenz) and, for a normal hi, an integer multiple of
// 2^(E - 39) no larger than 2^13 of them, so hi + lo * 2^(E - 39) gives g back bit for bit for
// every |g| >= 2^-14.  Below that, g is kept to 2^-39 absolute (a loss-scaled gradient that
// small is < 2^-30 before unscaling).  |g| >= 65520 stores an fp16 inf and decodes to inf,
// as does an infinity; a NaN stays NaN (the dynamic loss scale skips such a step either way,
// as it does when autocast's fp16 branch gradient overflows).
__device__ __forceinline__ void split8h(const float (&f)[8], uint4& hi, uint4& lo) {
  uint32_t h[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // g as an fp32 value first: without the barrier the compiler fuses the producing FMA and
    // this cast into v_fma_mix (one rounding of the exact result, which differs from torch's
    // cast of the fp32 gradient at fp32 values that are exact fp16 ties)
    float g = f[j];
    asm volatile("" : "+v"(g));
    const _Float16 hv = (_Float16)g;
    h[j] = __builtin_bit_cast(uint16_t, hv);
    const int e = (int)((h[j] >> 10) & 31u);
    const float r = g - (float)hv;
    const int q = e == 31 ? 0 : (int)__builtin_rintf(__builtin_amdgcn_ldexpf(r, 39 - (e > 1 ? e : 1)));
    l[j] = (uint32_t)q & 0xffffu;
  }
  hi = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  lo = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
}
__device__ __forceinline__ void unsplit8h(uint4 hi, uint4 lo, float (&f)[8]) {
  const uint32_t hw[4] = {hi.x, hi.y, hi.z, hi.w}, lw[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t hb = (hw[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    const int q = (int)(int16_t)((lw[i >> 1] >> (16 * (i & 1))) & 0xffffu);
    const int e = (int)((hb >> 10) & 31u);
    f[i] = (float)__builtin_bit_cast(_Float16, (uint16_t)hb) +
           __builtin_amdgcn_ldexpf((float)q, (e > 1 ? e : 1) - 39);
  }
}

// value as stored in the residual stream (bf16 rounding for a bf16 stream)
__device__ __forceinline__ float as_stream(float v, bf16_t*) { return bf2f(f2bf(v)); }
__device__ __forceinline__ float as_stream(float v, float*) { return v; }

// H: the 16-bit tensors (branch, weights, output) are fp16 (dtype float16; fp32 stream only)
// DROP: the branch's resid dropout fused (a separate instantiation: with the mask code
// compiled in, the p = 0 GPT-2 forward ran 192.5 -> 198.7 us per call)
template <int NK, typename XT, bool NT = false, bool H = false, bool DROP = false>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const XT* __restrict__ x, const bf16_t* __restrict__ res,
                                                    XT* __restrict__ sum_out, const bf16_t* __restrict__ w,
                                                    const bf16_t* __restrict__ b, bf16_t* __restrict__ y,
                                                    float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                    int N, int C, float eps, uint32_t dthresh = 0u,
                                                    float dscale = 1.0f, uint64_t dsalt = 0ull) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const XT* xr = x + (int64_t)row * C;
  const uint64_t dseed = DROP ? nsa_seed(dsalt) : 0ull;
  float v[NK][8];
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = (k * 64 + lane) * 8;
    if (c < C) {
      load8xn<NT>(xr + c, v[k]);
      if (res) {  // fused residual add: s = x + res, written out (XT) and normalised
        float rv[8];
        load8n<NT, H>(res + (int64_t)row * C + c, rv);
        if (DROP) {
          // the branch's resid dropout, fused: the mask and the 16-bit rounding of
          // nsa_dropout (elementwise.hip) for the same [N, C] element index, so the sum is
          // bit for bit x + dropout(res)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float t = rv[j] * dscale;
            asm volatile("" : "+v"(t));  // an fp32 product first, as nsa_dropout (no v_mad_mix)
            rv[j] = nsa_keep(dseed, (uint64_t)row * C + c + j, dthresh) ? e2f<H>(f2e<H>(t)) : 0.0f;
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] = as_stream(v[k][j] + rv[j], (XT*)nullptr);
        store8xn<NT>(sum_out + (int64_t)row * C + c, v[k]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[k][j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = 0.0f;
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float ss = 0.0f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = (k * 64 + lane) * 8;
    if (c < C) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[k][j] - mean;
        ss += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = (k * 64 + lane) * 8;
    if (c < C) {
      float wf[8], bfv[8], o[8];
      load8e<H>(w + c, wf);
      if (b) {
        load8e<H>(b + c, bfv);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) bfv[j] = 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[k][j] - mean) * rstd * wf[j] + bfv[j];
      store8e<H>(y + (int64_t)row * C + c, o);
    }
  }
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
}

#ifndef NSA_LNB_MINW
#define NSA_LNB_MINW 1  // min waves per SIMD (a tighter budget spills: the kernel needs ~130 VGPRs)
#endif
// PIPE: the next row's x / dy / dres vectors are loaded (as raw 16-byte words)
// while the current row is reduced and written (one overlapped memory round trip
// per row); !PIPE: one row at a time, memory parallelism from occupancy instead.
// xhat and dy*w are recomputed from the raw words in the second pass rather than
// kept in registers (VGPRs set this kernel's occupancy, VALU is idle).
// SPLIT (fp32 stream): bit 0 — dres is a split-plane gradient (split8, or split8h for
// fp16 compute); bit 1 — dx is written split (its hi plane is the branch copy, dx_branch unused)
template <int NK, bool PIPE, typename XT, bool NT = false, bool H = false, int SPLIT = 0>
__global__ __launch_bounds__(256, NSA_LNB_MINW) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const XT* __restrict__ x,
                                                    const bf16_t* __restrict__ w, const float* __restrict__ mean_in,
                                                    const float* __restrict__ rstd_in, const XT* __restrict__ dres,
                                                    XT* __restrict__ dx, bf16_t* __restrict__ dx_branch,
                                                    float* __restrict__ dw_part, float* __restrict__ db_part, int N,
                                                    int C) {
  // dw / db partial sums live in LDS, one [C] slice per wave (no sharing inside
  // the row loop): 2 x [4][C] fp32.  Keeping them in registers cost 32 VGPRs.
  extern __shared__ __attribute__((aligned(16))) float red[];
  float* accw = red + (threadIdx.x >> 6) * C;
  float* accb = red + 4 * C + (threadIdx.x >> 6) * C;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  uint4 wraw[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = min((k * 64 + lane) * 8, C - 8);
    wraw[k] = *reinterpret_cast<const uint4*>(w + c);
    if ((k * 64 + lane) * 8 < C) {
      *reinterpret_cast<float4*>(accw + (k * 64 + lane) * 8) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(accw + (k * 64 + lane) * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(accb + (k * 64 + lane) * 8) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(accb + (k * 64 + lane) * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const int row_step = gridDim.x * 4;
  int row = blockIdx.x * 4 + wv;
  Raw8<XT> nx[NK], nr[NK];
  uint4 nd[NK];
#define NSA_LNB_LOAD(R)                                                                  \
  _Pragma("unroll") for (int k = 0; k < NK; ++k) {                                       \
    const int c = min((k * 64 + lane) * 8, C - 8);                                       \
    const int64_t off = (int64_t)min((R), N - 1) * C + c;                                \
    nx[k] = ld_raw_n<NT>(x + off);                                                       \
    nd[k] = ld16n<NT>(dy + off);                                                         \
    if constexpr (SPLIT & 1) {                                                           \
      const uint16_t* hp = reinterpret_cast<const uint16_t*>(dres);                      \
      nr[k].u[0] = ld16n<NT>(hp + off);                                                  \
      nr[k].u[Raw8<XT>::W - 1] = ld16n<NT>(hp + (int64_t)N * C + off);                    \
    } else if (dres) {                                                                   \
      nr[k] = ld_raw_n<NT>(dres + off);                                                  \
    }                                                                                    \
  }
  if (PIPE) NSA_LNB_LOAD(row)
  for (; row < N; row += row_step) {
    if (!PIPE) NSA_LNB_LOAD(row)
    const float mean = mean_in[row];
    const float rstd = rstd_in[row];
    Raw8<XT> cx[NK], cr[NK];
    uint4 cd[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      cx[k] = nx[k];
      cd[k] = nd[k];
      cr[k] = nr[k];
    }
    if (PIPE) NSA_LNB_LOAD(row + row_step)
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int c = (k * 64 + lane) * 8;
      if (c < C) {
        float xv[8], dv[8], wf[8], aw[8], ab[8];
        unpack_raw(cx[k], xv);
        unpack8e<H>(cd[k], dv);
        unpack8e<H>(wraw[k], wf);
        float4* pw = reinterpret_cast<float4*>(accw + c);
        float4* pb = reinterpret_cast<float4*>(accb + c);
        *reinterpret_cast<float4*>(aw) = pw[0];
        *reinterpret_cast<float4*>(aw + 4) = pw[1];
        *reinterpret_cast<float4*>(ab) = pb[0];
        *reinterpret_cast<float4*>(ab + 4) = pb[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (xv[j] - mean) * rstd;
          const float g = dv[j] * wf[j];
          s1 += g;
          s2 += g * xh;
          aw[j] += dv[j] * xh;
          ab[j] += dv[j];
        }
        pw[0] = *reinterpret_cast<float4*>(aw);
        pw[1] = *reinterpret_cast<float4*>(aw + 4);
        pb[0] = *reinterpret_cast<float4*>(ab);
        pb[1] = *reinterpret_cast<float4*>(ab + 4);
      }
    }
    const float m1 = wave_sum(s1) / (float)C;
    const float m2 = wave_sum(s2) / (float)C;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int c = (k * 64 + lane) * 8;
      if (c < C) {
        float xv[8], dv[8], wf[8], o[8];
        unpack_raw(cx[k], xv);
        unpack8e<H>(cd[k], dv);
        unpack8e<H>(wraw[k], wf);
        float rv[8];  // gradient arriving through the residual path of the fused add
        if (dres) {
          if constexpr ((SPLIT & 1) && H) unsplit8h(cr[k].u[0], cr[k].u[Raw8<XT>::W - 1], rv);
          else if constexpr (SPLIT & 1) unsplit8(cr[k].u[0], cr[k].u[Raw8<XT>::W - 1], rv);
          else unpack_raw(cr[k], rv);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) rv[j] = 0.0f;
        }
        // explicit fused multiply-adds: the same roundings in every instantiation (the
        // split-plane and plain forms agree bit for bit, whatever the compiler contracts)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (xv[j] - mean) * rstd;
          const float t = __builtin_fmaf(-xh, m2, __builtin_fmaf(dv[j], wf[j], -m1));
          o[j] = __builtin_fmaf(rstd, t, rv[j]);
        }
        if constexpr (SPLIT & 2) {  // hi plane: plain store (the branch GEMMs read it next)
          uint4 hi, lo;
          if constexpr (H) split8h(o, hi, lo);
          else split8(o, hi, lo);
          uint16_t* hp = reinterpret_cast<uint16_t*>(dx);
          *reinterpret_cast<uint4*>(hp + (int64_t)row * C + c) = hi;
          st16n<NT>(hp + (int64_t)N * C + (int64_t)row * C + c, lo);
        } else {
          store8xn<NT>(dx + (int64_t)row * C + c, o);
          if (dx_branch) store8e<H>(dx_branch + (int64_t)row * C + c, o);  // 16-bit copy for the branch GEMMs
        }
      }
    }
  }
#undef NSA_LNB_LOAD
  (void)wv;
  // block reduction of the per-wave dw/db slices (4 waves -> 1 partial row)
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    dw_part[(int64_t)blockIdx.x * C + c] = red[c] + red[C + c] + red[2 * C + c] + red[3 * C + c];
    if (db_part)
      db_part[(int64_t)blockIdx.x * C + c] = red[4 * C + c] + red[5 * C + c] + red[6 * C + c] + red[7 * C + c];
  }
}

// nontemporal streams in the LayerNorm passes (default; NSA_LN_NT=0 turns them off, read once;
// nsa_ln_set_nt switches them for A/B runs).  GPT-2 124M step, same box, interleaved: 462.7 / 463.3 ms without,
// 461.6 / 461.7 ms with
int& ln_nt_flag() {  // resolved once from NSA_LN_NT (0 = plain); nsa_ln_set_nt for A/B
  static int f = [] {
    const char* e = getenv("NSA_LN_NT");
    return !(e && e[0] == '0') ? 1 : 0;
  }();
  return f;
}
bool ln_nt() { return ln_nt_flag() != 0; }

template <int NK, typename XT, bool H = false>
hipError_t launch_fwd(const void* x, const void* res, void* sum_out, const void* w, const void* b, void* y,
                      void* mean, void* rstd, int N, int C, float eps, hipStream_t s, float p = 0.0f,
                      uint64_t salt = 0ull) {
  const uint32_t th = p > 0.0f ? nsa_drop_thresh(p) : 0u;
  const float dscale = p > 0.0f && p < 1.0f ? 1.0f / (1.0f - p) : 0.0f;
  const bool nt = ln_nt() && (int64_t)N * C * (int64_t)sizeof(XT) >= NSA_NT_MIN_BYTES;
#define NSA_LN_FWD_GO(NT_, DROP_)                                                                             \
  ln_fwd_kernel<NK, XT, NT_, H, DROP_><<<(N + 3) / 4, 256, 0, s>>>(                                            \
      (const XT*)x, (const bf16_t*)res, (XT*)sum_out, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y,          \
      (float*)mean, (float*)rstd, N, C, eps, th, dscale, salt)
  if (th && res) {
    if (nt) NSA_LN_FWD_GO(true, true);
    else NSA_LN_FWD_GO(false, true);
  } else {
    if (nt) NSA_LN_FWD_GO(true, false);
    else NSA_LN_FWD_GO(false, false);
  }
#undef NSA_LN_FWD_GO
  return hipGetLastError();
}

// The backward's dw / db accumulators take 8·C·4 bytes of dynamic LDS, and a workgroup can have
// the CU's 160 KiB: C <= 5120.  (The forward keeps rows in registers: C <= 8192.)  Launches
// above 64 KiB, up to all 160, need no function attribute on this runtime (measured at
// C = 2056, 4104 and 5120).
constexpr int kLnBwdMaxC = 5120;
inline bool ln_bwd_c_ok(int C) { return C > 0 && C % 8 == 0 && C <= kLnBwdMaxC; }

template <int NK, bool PIPE, typename XT, bool NT, bool H>
hipError_t launch_bwd_split(int split, const void* dy, const void* x, const void* w, const void* mean,
                            const void* rstd, const void* dres, void* dx, void* dx_branch, void* dw_part,
                            void* db_part, int N, int C, int nblk, hipStream_t s) {
#define NSA_LNB_GO(SP)                                                                                  \
  ln_bwd_kernel<NK, PIPE, XT, NT, H, SP><<<nblk, 256, 8 * C * sizeof(float), s>>>(                      \
      (const bf16_t*)dy, (const XT*)x, (const bf16_t*)w, (const float*)mean, (const float*)rstd,         \
      (const XT*)dres, (XT*)dx, (bf16_t*)dx_branch, (float*)dw_part, (float*)db_part, N, C)
  if constexpr (std::is_same<XT, float>::value) {
    switch (split) {
      case 1: NSA_LNB_GO(1); return hipGetLastError();
      case 2: NSA_LNB_GO(2); return hipGetLastError();
      case 3: NSA_LNB_GO(3); return hipGetLastError();
      default: break;
    }
  }
  NSA_LNB_GO(0);
#undef NSA_LNB_GO
  return hipGetLastError();
}

template <int NK, typename XT, bool H = false>
hipError_t launch_bwd(const void* dy, const void* x, const void* w, const void* mean, const void* rstd,
                      const void* dres, void* dx, void* dx_branch, void* dw_part, void* db_part, int N, int C,
                      int nblk, hipStream_t s) {
  // bit 30 of nblk selects the non-pipelined body (A/B timing); bits 28-29 the split planes
  const bool pipe = !(nblk & (1 << 30));
  const int split = (nblk >> 28) & 3;
  nblk &= (1 << 28) - 1;
  if (split && !std::is_same<XT, float>::value) return hipErrorInvalidValue;
  if ((split & 1) && dres == nullptr) return hipErrorInvalidValue;
  if (pipe && ln_nt() && (int64_t)N * C * (int64_t)sizeof(XT) >= NSA_NT_MIN_BYTES)
    return launch_bwd_split<NK, true, XT, true, H>(split, dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part,
                                                   db_part, N, C, nblk, s);
  if (pipe)
    return launch_bwd_split<NK, true, XT, false, H>(split, dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part,
                                                    db_part, N, C, nblk, s);
  return launch_bwd_split<NK, false, XT, false, H>(split, dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part,
                                                   db_part, N, C, nblk, s);
}

}  // namespace

#define NSA_NK_SWITCH(NK_EXPR, CALL)                      \
  switch (NK_EXPR) {                                        \
    case 1: { constexpr int K_ = 1; return CALL; }          \
    case 2: { constexpr int K_ = 2; return CALL; }          \
    case 3: { constexpr int K_ = 3; return CALL; }          \
    case 4: { constexpr int K_ = 4; return CALL; }          \
    case 5:                                                 \
    case 6: { constexpr int K_ = 6; return CALL; }          \
    case 7:                                                 \
    case 8: { constexpr int K_ = 8; return CALL; }          \
    default:                                                \
      if ((NK_EXPR) <= 16) { constexpr int K_ = 16; return CALL; } \
      return hipErrorInvalidValue;                          \
  }

// y = LN(x [+ res]) ; with res != NULL also writes sum_out = x + res.
// x / sum_out are bf16 (nsa_layernorm_fwd) or fp32 (nsa_layernorm_fwd_x32); res, w, b, y bf16.
NSA_API hipError_t nsa_layernorm_fwd(const void* x, const void* res, void* sum_out, const void* w, const void* b,
                                     void* y, void* mean, void* rstd, int N, int C, float eps, hipStream_t s) {
  if (C % 8 != 0) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512, (launch_fwd<K_, bf16_t>(x, res, sum_out, w, b, y, mean, rstd, N, C, eps, s)));
}

NSA_API hipError_t nsa_layernorm_fwd_x32(const void* x, const void* res, void* sum_out, const void* w, const void* b,
                                         void* y, void* mean, void* rstd, int N, int C, float eps, hipStream_t s) {
  if (C % 8 != 0) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512, (launch_fwd<K_, float>(x, res, sum_out, w, b, y, mean, rstd, N, C, eps, s)));
}

// dx = LN'(dy) [+ dres]; per-block dw/db partial rows for nsa_colsum_accum
NSA_API hipError_t nsa_layernorm_bwd(const void* dy, const void* x, const void* w, const void* mean,
                                     const void* rstd, const void* dres, void* dx, void* dw_part, void* db_part,
                                     int N, int C, int nblk, hipStream_t s) {
  if (!ln_bwd_c_ok(C)) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512, (launch_bwd<K_, bf16_t>(dy, x, w, mean, rstd, dres, dx, nullptr, dw_part, db_part,
                                                         N, C, nblk, s)));
}

// fp32 residual stream: x, dres, dx fp32; dx_branch (optional) = bf16(dx) for the branch GEMMs
NSA_API hipError_t nsa_layernorm_bwd_x32(const void* dy, const void* x, const void* w, const void* mean,
                                         const void* rstd, const void* dres, void* dx, void* dx_branch,
                                         void* dw_part, void* db_part, int N, int C, int nblk, hipStream_t s) {
  if (!ln_bwd_c_ok(C)) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512, (launch_bwd<K_, float>(dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part, db_part,
                                                        N, C, nblk, s)));
}

// nsa_layernorm_bwd_x32 with split-plane residual gradients (bf16 compute): split bit 0 —
// dres is split (split8: hi plane then lo plane in its 4·N·C bytes), bit 1 — dx is written
// split, its hi plane being the bf16 branch gradient (dx_branch unused)
NSA_API hipError_t nsa_layernorm_bwd_x32s(const void* dy, const void* x, const void* w, const void* mean,
                                          const void* rstd, const void* dres, void* dx, void* dx_branch,
                                          void* dw_part, void* db_part, int N, int C, int nblk, int split,
                                          hipStream_t s) {
  if (!ln_bwd_c_ok(C) || split < 0 || split > 3 || (nblk & ~(1 << 30)) >= (1 << 28))
    return hipErrorInvalidValue;
  nblk |= split << 28;
  NSA_NK_SWITCH((C + 511) / 512, (launch_bwd<K_, float>(dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part, db_part,
                                                        N, C, nblk, s)));
}

// nsa_layernorm_bwd_x32s for fp16 compute (split8h planes: the hi plane is the fp16 branch gradient)
NSA_API hipError_t nsa_layernorm_bwd_x32s_h(const void* dy, const void* x, const void* w, const void* mean,
                                            const void* rstd, const void* dres, void* dx, void* dx_branch,
                                            void* dw_part, void* db_part, int N, int C, int nblk, int split,
                                            hipStream_t s) {
  if (!ln_bwd_c_ok(C) || split < 0 || split > 3 || (nblk & ~(1 << 30)) >= (1 << 28))
    return hipErrorInvalidValue;
  nblk |= split << 28;
  NSA_NK_SWITCH((C + 511) / 512, (launch_bwd<K_, float, true>(dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part,
                                                              db_part, N, C, nblk, s)));
}

// nsa_layernorm_fwd_x32 with the branch's dropout fused (res must be given): sum_out =
// x + dropout_p(res) with nsa_dropout's mask for `seed` (the branch gradient takes the same
// mask through nsa_dropout in the backward)
NSA_API hipError_t nsa_layernorm_fwd_x32d(const void* x, const void* res, void* sum_out, const void* w, const void* b,
                                          void* y, void* mean, void* rstd, int N, int C, float eps, float p,
                                          uint64_t seed, hipStream_t s) {
  if (C % 8 != 0 || res == nullptr) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512,
                (launch_fwd<K_, float>(x, res, sum_out, w, b, y, mean, rstd, N, C, eps, s, p, seed)));
}
NSA_API hipError_t nsa_layernorm_fwd_x32d_h(const void* x, const void* res, void* sum_out, const void* w,
                                            const void* b, void* y, void* mean, void* rstd, int N, int C, float eps,
                                            float p, uint64_t seed, hipStream_t s) {
  if (C % 8 != 0 || res == nullptr) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512,
                (launch_fwd<K_, float, true>(x, res, sum_out, w, b, y, mean, rstd, N, C, eps, s, p, seed)));
}

// dropout step counter of this translation unit (nsa_rng_advance / nsa_rng_set bump all of them)
NSA_DEFINE_RNG_ADVANCE(nsa_rng_advance_ln)

// fp16 branch / weights / output with the fp32 stream (dtype float16)
NSA_API hipError_t nsa_layernorm_fwd_x32_h(const void* x, const void* res, void* sum_out, const void* w, const void* b,
                                           void* y, void* mean, void* rstd, int N, int C, float eps, hipStream_t s) {
  if (C % 8 != 0) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512,
                (launch_fwd<K_, float, true>(x, res, sum_out, w, b, y, mean, rstd, N, C, eps, s)));
}
NSA_API hipError_t nsa_layernorm_bwd_x32_h(const void* dy, const void* x, const void* w, const void* mean,
                                           const void* rstd, const void* dres, void* dx, void* dx_branch,
                                           void* dw_part, void* db_part, int N, int C, int nblk, hipStream_t s) {
  if (!ln_bwd_c_ok(C)) return hipErrorInvalidValue;
  NSA_NK_SWITCH((C + 511) / 512, (launch_bwd<K_, float, true>(dy, x, w, mean, rstd, dres, dx, dx_branch, dw_part,
                                                              db_part, N, C, nblk, s)));
}

// stream size (N * C * sizeof of the stream's element) from which the nontemporal instantiations are taken
NSA_API int64_t nsa_ln_nt_min_bytes() { return NSA_NT_MIN_BYTES; }

// set the streaming-store policy of the LayerNorm kernels (on < 0: keep); returns the old one
NSA_API int nsa_ln_set_nt(int on) {
  const int prev = ln_nt_flag();
  if (on >= 0) ln_nt_flag() = on ? 1 : 0;
  return prev;
}
