// Declarations shared by the bf16 decode kernels (decode.hip) and their int8-weight forms
// (decode_q8.hip): the layout of an attention partial, the single-row prologue arguments and
// the small helpers both files use.  The prologue bodies themselves are the function-body
// fragments decode_row_prologue.h and decode_skinny_ln_prologue.h.
#pragma once

#include "common.h"

#include <stdlib.h>

#include <algorithm>

namespace {

constexpr int DA_D = 64;        // head dim of the decode-attention kernel
constexpr int DA_PO = 4;          // o[] offset in a partial: 16-byte aligned for vector reads
constexpr int DA_PART = DA_PO + DA_D;  // m, l, (pad), o[64]
constexpr int DA_CHUNK = 256;   // keys per workgroup of the attention partial kernel (one per thread)

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

// NSA_GEMV_GRID: workgroup cap of the single-row GEMVs (default 1024: 4 per CU)
int gemv_row_grid() {
  static const int g = [] {
    const char* e = getenv("NSA_GEMV_GRID");
    return e ? std::max(1, atoi(e)) : 1024;
  }();
  return g;
}

}  // namespace
