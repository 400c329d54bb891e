// Declarations shared by the bf16 decode kernels (decode.hip) and their int8-weight forms
// (decode_q8.hip): the layout of an attention partial, the single-row prologue arguments and
// the small helpers both files use.  The prologue bodies themselves are the function-body
// fragments decode_row_prologue.h and decode_skinny_ln_prologue.h.
#pragma once

#include "common.h"

#include <stdlib.h>

#include <algorithm>
#include <type_traits>

namespace {

constexpr int DA_D = 64;        // head dim of the decode-attention kernel
constexpr int DA_PO = 4;          // o[] offset in a partial: 16-byte aligned for vector reads
constexpr int DA_PART = DA_PO + DA_D;  // m, l, (pad), o[64]
constexpr int DA_CHUNK = 256;   // keys per workgroup of the attention partial kernel (one per thread)

// What the decode linears' entry points accept (ops/functional.py mirrors these)
constexpr int ROW_MAX_K = 8192;           // single-row prologue kernels: the row x[K] as fp32 in LDS
constexpr int SKINNY_LN_MAX_K = 1920;     // skinny LayerNorm kernels: the LDS image [16][K + 8] bf16
constexpr int ATTN_MAX_WEIGHTS = 16384;   // PRO_ATTN: heads * n_split chunk weights in LDS behind the row
constexpr int GEMV_MAX_ROWS = 8;          // vector GEMV: 8 x rows partial sums per lane
constexpr int SKINNY_GROUP_ROWS = 16;     // one 16-row MFMA group: the skinny LayerNorm and int8 kernels
constexpr int SKINNY_MAX_ROWS = 64;       // bf16 skinny GEMM: 4 groups
constexpr int ROW_K_BF16 = 8, ROW_K_Q8 = 16;         // K granule of the vector kernels: k per 16-byte weight piece
constexpr int SKINNY_K_BF16 = 32, SKINNY_K_Q8 = 64;  // K granule of the skinny kernels: k per lane group's unit

// int8 -> fp32 (two's-complement bytes, exact): the int8 weights of decode_q8.hip and the
// int8 KV-cache rows of decode.hip
// byte j of a dword as a float
__device__ __forceinline__ float q8f(uint32_t w, int j) { return (float)(int)(int8_t)(w >> (8 * j)); }

// the 8 values of two dwords (k order: byte 0 of lo first)
__device__ __forceinline__ void unpack8q(uint32_t lo, uint32_t hi, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = q8f(lo, j);
    f[4 + j] = q8f(hi, j);
  }
}

// Single-row decode linear with its input's producer in the prologue: every workgroup
// builds the row x[K] (bf16-rounded, in LDS) itself, then streams its NC weight rows:
//   PRO_LN     s = res + branch (fp32; written to res_out by workgroup 0), x = LN(s)
//   PRO_EMB_LN s = wte[*tok] + wpe[*pos] (written to res_out by workgroup 0), x = LN(s)
//   PRO_ATTN   x = the flash-decoding combine of the attention partials (ws, H heads)
//   y = act(x W^T + bias)
// The recomputation is cheap (K <= 8192 values, L2-resident) and removes the separate
// add+LayerNorm / combine / embedding launch per linear: at batch 1 each launch costs a
// few microseconds of fixed overhead against ~1-10 us of weight streaming.  The first
// K piece of the weights is loaded before the prologue, so its latency overlaps it.
// res_out must not alias res.
enum { PRO_LN = 0, PRO_ATTN = 1, PRO_EMB_LN = 2 };

struct RowPro {
  const float* res;
  const bf16_t* branch;
  float* res_out;
  const bf16_t* lw;
  const bf16_t* lb;
  float eps;
  const float* ws;
  int n_split;
  const int64_t* tok;
  const int64_t* pos;
  const bf16_t* wte;
  const bf16_t* wpe;
  int64_t* pos_inc;  // PRO_LN: incremented by one thread after the row (the decode step's position)
};

// V values per lane -> lane holds the wave-wide sum of value `index` (halve-and-exchange
// butterfly)
template <int V>
__device__ __forceinline__ float wave_reduce_multi(float (&v)[V], int lane, int& index) {
  int cnt = V;
  index = 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    if (cnt > 1) {
      const bool upper = (lane & off) != 0;
      const int h = cnt / 2;
#pragma unroll
      for (int i = 0; i < V / 2; ++i) {
        if (i < h) {
          const float send = upper ? v[i] : v[i + h];
          const float keep = upper ? v[i + h] : v[i];
          v[i] = keep + __shfl_xor(send, off, 64);
        }
      }
      if (upper) index += h;
      cnt = h;
    } else {
      v[0] += __shfl_xor(v[0], off, 64);
    }
  }
  return v[0];
}

// Host side of the single-row prologue linears (nsa_gemv_ln / _emb_ln / _attn and their _q8
// forms): the argument checks (false: refuse; granule = ROW_K_BF16 or ROW_K_Q8), the RowPro of
// each prologue and the dynamic LDS of the launch.
bool row_linear_ok(int N, int K, int granule, int act, int out_f32) {
  return K % granule == 0 && K <= ROW_MAX_K && N >= 1 && !(act && out_f32);
}
bool row_ln_ok(const void* res, const void* branch, const void* res_out, int N, int K, int granule, int act,
               int out_f32) {
  return row_linear_ok(N, K, granule, act, out_f32) && !(branch && (!res_out || res_out == res));
}
bool row_emb_ln_ok(const void* res_out, int N, int K, int granule, int act, int out_f32) {
  return row_linear_ok(N, K, granule, act, out_f32) && res_out;
}
bool row_attn_ok(int n_split, int N, int K, int act, int out_f32) {  // K = H * DA_D: on either granule
  return row_linear_ok(N, K, DA_D, act, out_f32) && n_split >= 1 && (K / DA_D) * n_split <= ATTN_MAX_WEIGHTS;
}

RowPro row_ln(const void* res, const void* branch, void* res_out, const void* lw, const void* lb, float eps,
              void* pos_inc) {
  RowPro a{};
  a.res = (const float*)res;
  a.branch = (const bf16_t*)branch;
  a.res_out = (float*)res_out;
  a.lw = (const bf16_t*)lw;
  a.lb = (const bf16_t*)lb;
  a.eps = eps;
  a.pos_inc = (int64_t*)pos_inc;
  return a;
}
RowPro row_emb_ln(const void* tok, const void* pos, const void* wte, const void* wpe, void* res_out, const void* lw,
                  const void* lb, float eps) {
  RowPro a = row_ln(nullptr, nullptr, res_out, lw, lb, eps, nullptr);
  a.tok = (const int64_t*)tok;
  a.pos = (const int64_t*)pos;
  a.wte = (const bf16_t*)wte;
  a.wpe = (const bf16_t*)wpe;
  return a;
}
RowPro row_attn(const void* ws, int n_split) {
  RowPro a{};
  a.ws = (const float*)ws;
  a.n_split = n_split;
  return a;
}
// the row, plus the chunk weights of the attention combine
template <int PRO>
size_t row_lds_bytes(const RowPro& a, int K) {
  return (size_t)(K + (PRO == PRO_ATTN ? (K / DA_D) * a.n_split : 0)) * sizeof(float);
}

// The epilogue of every decode linear is one of three instantiations: GELU (bf16 out), fp32 out,
// plain bf16 (the entry points refuse act && out_f32).  launch(int_c<ACT>, bool_constant<OUTF>)
// is a generic lambda that names the kernel with decltype(..)::value.
template <int V>
using int_c = std::integral_constant<int, V>;

template <typename F>
void epilogue_dispatch(int act, int out_f32, F&& launch) {
  if (act)
    launch(int_c<1>{}, std::false_type{});
  else if (out_f32)
    launch(int_c<0>{}, std::true_type{});
  else
    launch(int_c<0>{}, std::false_type{});
}

// NSA_GEMV_GRID: workgroup cap of the single-row GEMVs (default 1024: 4 per CU)
int gemv_row_grid() {
  static const int g = [] {
    const char* e = getenv("NSA_GEMV_GRID");
    return e ? std::max(1, atoi(e)) : 1024;
  }();
  return g;
}

}  // namespace
