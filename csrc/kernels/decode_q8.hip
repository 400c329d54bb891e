// Int8-weight forms of the weight-streaming decode kernels of decode.hip (the serving path
// with Decoder(..., quantize="int8")): the weight of every linear is stored as one int8 per
// element with one fp32 scale per output row (ops.quantize_rows_int8), so a decode step
// streams half the bytes of the bf16 step.  All six compute
//   y[m, n] = act((sum_k x[m, k] q[n, k]) scale[n] + bias[n])
// with x the bf16-rounded activation row the bf16 kernel forms, fp32 accumulation and the
// scale applied once per output in the epilogue.  int8 -> float is exact, so the results
// differ from the bf16 kernels run on the dequantized weights by summation order alone.
//
// The prologues (residual add + LayerNorm, embedding + LayerNorm, flash-decoding combine)
// are the bf16 kernels' own: one source, the function-body fragments decode_row_prologue.h
// and decode_skinny_ln_prologue.h, which decode.hip includes inline in its kernels and this
// file as the bodies of row_prologue() and skinny_ln_prologue().  The single-row ones store
// the row to LDS in another order here (hx() below, through the fragment's NSA_HS macro).
// They are shared as text, not as a function: calling a function from decode.hip's
// gemv_row_kernel changes the compiled code of the bf16 kernels (register allocation,
// occupancy), while textual inclusion leaves the kernels of both files as they were.  The
// declarations both files use (RowPro, PRO_*, the partial layout, wave_reduce_multi,
// gemv_row_grid) are in decode_rows.h.
#include "decode_rows.h"

#include <math.h>

#include <algorithm>

namespace {

// LDS position of x[k].  A lane multiplies one 16-byte weight piece (k = 16 g .. 16 g + 15)
// with 16 values of x; k-contiguous rows would put lane g at a 64-byte stride, all 64 lanes
// of a read on 4 of the 64 banks.  The 16 values sit as four float4 at [j][g] (j = (k / 4) % 4,
// nck = K / 16 chunks), so the lanes of a wave read consecutive 16-byte vectors.
__device__ __forceinline__ int hx(int k, int nck) { return (((k >> 2) & 3) * nck + (k >> 4)) * 4 + (k & 3); }

// The row x[K] into hs[] at hx(k) (256 threads; stat: 2 x 4 floats of LDS; PRO_ATTN also uses
// hs[K ..] for the chunk weights).  The caller's barrier after it publishes hs[].
template <int PRO>
__device__ __forceinline__ void row_prologue(const RowPro& a, float* hs, float (*stat)[4], int K) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nck = K / 16;
#define NSA_HS(k) hx(k, nck)
#include "decode_row_prologue.h"
#undef NSA_HS
}

// Prologue of the skinny GEMMs with the residual add + LayerNorm in front (256 threads):
// x = LN(res + branch) of the M batch rows as bf16 in xs ([16][K + 8], padded rows).  The
// caller's barrier after it publishes xs[].
__device__ __forceinline__ void skinny_ln_prologue(const float* __restrict__ res, const bf16_t* __restrict__ branch,
                                                   float* __restrict__ s_out, const bf16_t* __restrict__ lw,
                                                   const bf16_t* __restrict__ lb, float eps, bf16_t* xs, int M,
                                                   int K) {
  const int KP = K + 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#include "decode_skinny_ln_prologue.h"
}

// ---------------------------------------------------------------------------
// int8 -> bf16 (two's-complement bytes, exact; q8f / unpack8q, the fp32 forms, are in
// decode_rows.h)
// ---------------------------------------------------------------------------
// bytes j, j + 1 of a dword as a packed bf16 pair.  An int8 value has at most 7
// significant bits, so the high half of its fp32 form is already its exact bf16: the two
// high halves are packed by one byte permute, without a rounding convert.
__device__ __forceinline__ uint32_t q8bf2(uint32_t w, int j) {
  return __builtin_amdgcn_perm(__float_as_uint(q8f(w, j + 1)), __float_as_uint(q8f(w, j)), 0x07060302u);
}
// the 8 weights of two dwords as one MFMA fragment (8 bf16)
__device__ __forceinline__ bf16x8 q8frag(uint32_t lo, uint32_t hi) {
  const uint4 u = {q8bf2(lo, 0), q8bf2(lo, 2), q8bf2(hi, 0), q8bf2(hi, 2)};
  return __builtin_bit_cast(bf16x8, u);
}

// ---------------------------------------------------------------------------
// Decode linear, int8 weights, M <= 8 rows on the vector ALU with a K loop (nsa_gemv's
// counterpart for 2 .. NSA_GEMV_MAX_ROWS rows, and for one row wider than 8192).
// A lane's 16-byte load carries 16 weights of one row: chunk g covers k = 16g .. 16g+15.
// KW of the workgroup's 4 waves split K and the other 4 / KW wave sets take further
// columns: a workgroup covers (4 / KW) * NC output columns.
// ---------------------------------------------------------------------------
template <int M, int ACT, bool OUTF, int NC, int KW>
__global__ __launch_bounds__(256) void gemv_q8_kernel(const bf16_t* __restrict__ x, const int8_t* __restrict__ Wq,
                                                      const float* __restrict__ scale,
                                                      const bf16_t* __restrict__ bias, void* __restrict__ y, int rows,
                                                      int N, int K) {
  constexpr int V = NC * M, CG = 4 / KW;
  __shared__ float red[4][V];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kw = w % KW, cg = w / KW;
  const int n0 = (blockIdx.x * CG + cg) * NC;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  const int nchunk = K / 16;
#pragma unroll 2
  for (int g = kw * 64 + lane; g < nchunk; g += 64 * KW) {
    const int k = 16 * g;
    uint4 q[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = *reinterpret_cast<const uint4*>(Wq + (int64_t)min(n0 + c, N - 1) * K + k);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float xf[M][8];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if (m < rows) load8(x + (int64_t)m * K + k + 8 * h, xf[m]);
        else
#pragma unroll
          for (int j = 0; j < 8; ++j) xf[m][j] = 0.0f;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float wf[8];
        unpack8q(h ? q[c].z : q[c].x, h ? q[c].w : q[c].y, wf);
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[c * M + m] = fmaf(xf[m][j], wf[j], acc[c * M + m]);
      }
    }
  }
  int idx;
  const float v = wave_reduce_multi<V>(acc, lane, idx);
  // lanes below the last split's offset hold duplicates: the first of each group writes
  constexpr int DUP = 64 / V;  // lanes per value
  if ((lane & (DUP - 1)) == 0) red[w][idx] = v;
  __syncthreads();
  if (tid < CG * V) {
    const int g = tid / V, i = tid % V;
    const int c = i / M, m = i % M, n = (blockIdx.x * CG + g) * NC + c;
    if (m < rows && n < N) {
      float o = 0.0f;
#pragma unroll
      for (int q = 0; q < KW; ++q) o += red[g * KW + q][i];
      o *= scale[n];
      if (bias) o += bf2f(bias[n]);
      if (ACT == 1) o = nsa_gelu(o);
      if constexpr (OUTF)
        reinterpret_cast<float*>(y)[(int64_t)m * N + n] = o;
      else
        reinterpret_cast<bf16_t*>(y)[(int64_t)m * N + n] = f2bf(o);
    }
  }
}

// ---------------------------------------------------------------------------
// One decode row, int8 weights: the single-row kernels.  KW of the workgroup's 4 waves split
// K and the other 4 / KW wave sets take further columns (BN = (4 / KW) * NC columns per
// block); a lane owns chunks g = kw * 64 + lane + p * 64 * KW, p < P, so KW * P * 64 >= K / 16
// covers the row (q8_cfg: every K <= 8192 with P <= 2) and all weight loads of a block issue
// together, with no K loop: chunks past the end re-read the last chunk against a zeroed x
// (branch-free), rows past N re-read row N - 1 and are not stored.
// ---------------------------------------------------------------------------
// the fewest waves along K that cover the row in one pass; two passes beyond 4096:
// f(int_c<KW>, int_c<P>)
template <typename F>
void q8_cfg(int K, F&& f) {
  const int nck = K / 16;
  if (nck <= 64)
    f(int_c<1>{}, int_c<1>{});
  else if (nck <= 128)
    f(int_c<2>{}, int_c<1>{});
  else if (nck <= 256)
    f(int_c<4>{}, int_c<1>{});
  else
    f(int_c<4>{}, int_c<2>{});  // nck <= 512 (callers check)
}
// the weights of block row set n0 into wp (all P * NC loads in flight together)
template <int NC, int P>
__device__ __forceinline__ void q8_load_block(const int8_t* __restrict__ Wq, int n0, int N, int K, const int (&gc)[P],
                                              uint4 (&wp)[P][NC]) {
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c)
      wp[p][c] = *reinterpret_cast<const uint4*>(Wq + (int64_t)min(n0 + c, N - 1) * K + 16 * gc[p]);
}
// acc[c] = sum over the lane's chunks of x . w
template <int NC, int P>
__device__ __forceinline__ void q8_dot_block(const float (&xr)[P][16], const uint4 (&wp)[P][NC], float (&acc)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float wf[8];
      unpack8q(wp[p][c].x, wp[p][c].y, wf);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[c] = fmaf(xr[p][j], wf[j], acc[c]);
      unpack8q(wp[p][c].z, wp[p][c].w, wf);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[c] = fmaf(xr[p][8 + j], wf[j], acc[c]);
    }
}

// y[n] = act((x . Wq[n]) scale[n] + bias[n]) with the producer of x in the prologue
// (gemv_row_kernel's counterpart).  Each workgroup loops over column blocks cb, cb +
// gridDim.x, ...; the first block's weights are issued before the prologue and the next
// block's before the reduction; x stays in registers across the blocks.
template <int PRO, int ACT, bool OUTF, int NC, int KW, int P>
__global__ __launch_bounds__(256) void gemv_row_q8_kernel(const RowPro a, const int8_t* __restrict__ Wq,
                                                          const float* __restrict__ scale,
                                                          const bf16_t* __restrict__ bias, void* __restrict__ y,
                                                          int N, int K) {
  extern __shared__ __attribute__((aligned(16))) float hs[];  // [K] input row at hx(k)
  constexpr int CG = 4 / KW, BN = CG * NC;  // wave sets / columns per block
  __shared__ float red[4][NC];
  __shared__ float stat[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kw = w % KW, cg = w / KW;
  const int nchunk = K / 16;
  const int nblk = (N + BN - 1) / BN;
  int gc[P];
  bool live[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int g = kw * 64 + lane + p * 64 * KW;
    live[p] = g < nchunk;
    gc[p] = live[p] ? g : nchunk - 1;
  }
  int cb = blockIdx.x;
  uint4 wp[P][NC];
  q8_load_block<NC, P>(Wq, cb * BN + cg * NC, N, K, gc, wp);
  row_prologue<PRO>(a, hs, stat, K);
  __syncthreads();
  float xr[P][16];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float4 v = reinterpret_cast<const float4*>(hs)[j * nchunk + gc[p]];
      if (!live[p]) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      xr[p][4 * j] = v.x;
      xr[p][4 * j + 1] = v.y;
      xr[p][4 * j + 2] = v.z;
      xr[p][4 * j + 3] = v.w;
    }
  for (; cb < nblk; cb += gridDim.x) {
    float acc[NC];
    q8_dot_block<NC, P>(xr, wp, acc);
    const int nb = cb + gridDim.x;
    if (nb < nblk) q8_load_block<NC, P>(Wq, nb * BN + cg * NC, N, K, gc, wp);  // in flight during the reduction
    int idx;
    const float v = wave_reduce_multi<NC>(acc, lane, idx);
    if ((lane & (64 / NC - 1)) == 0) red[w][idx] = v;
    __syncthreads();
    if (tid < BN) {
      const int g = tid / NC, c = tid % NC;
      const int n = cb * BN + tid;
      if (n < N) {
        float o = 0.0f;
#pragma unroll
        for (int q = 0; q < KW; ++q) o += red[g * KW + q][c];
        o *= scale[n];
        if (bias) o += bf2f(bias[n]);
        if (ACT == 1) o = nsa_gelu(o);
        if constexpr (OUTF)
          reinterpret_cast<float*>(y)[n] = o;
        else
          reinterpret_cast<bf16_t*>(y)[n] = f2bf(o);
      }
    }
    __syncthreads();  // red[] is rewritten by the next block
  }
  if constexpr (PRO == PRO_LN)
    if (a.pos_inc && blockIdx.x == 0 && tid == 0) *a.pos_inc += 1;
}

// The same for a row x that is already in memory (nsa_gemv_q8 at one row): one block per
// workgroup, x read with the weights.
template <int ACT, bool OUTF, int NC, int KW, int P>
__global__ __launch_bounds__(256) void gemv1_q8_kernel(const bf16_t* __restrict__ x, const int8_t* __restrict__ Wq,
                                                       const float* __restrict__ scale,
                                                       const bf16_t* __restrict__ bias, void* __restrict__ y, int N,
                                                       int K) {
  constexpr int CG = 4 / KW, BN = CG * NC;
  __shared__ float red[4][NC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kw = w % KW, cg = w / KW;
  const int nchunk = K / 16;
  int gc[P];
  bool live[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int g = kw * 64 + lane + p * 64 * KW;
    live[p] = g < nchunk;
    gc[p] = live[p] ? g : nchunk - 1;
  }
  uint4 wp[P][NC];
  q8_load_block<NC, P>(Wq, blockIdx.x * BN + cg * NC, N, K, gc, wp);
  float xr[P][16];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    float lo[8], hi[8];
    load8(x + 16 * gc[p], lo);
    load8(x + 16 * gc[p] + 8, hi);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xr[p][j] = live[p] ? lo[j] : 0.0f;
      xr[p][8 + j] = live[p] ? hi[j] : 0.0f;
    }
  }
  float acc[NC];
  q8_dot_block<NC, P>(xr, wp, acc);
  int idx;
  const float v = wave_reduce_multi<NC>(acc, lane, idx);
  if ((lane & (64 / NC - 1)) == 0) red[w][idx] = v;
  __syncthreads();
  if (tid < BN) {
    const int g = tid / NC, c = tid % NC;
    const int n = blockIdx.x * BN + tid;
    if (n < N) {
      float o = 0.0f;
#pragma unroll
      for (int q = 0; q < KW; ++q) o += red[g * KW + q][c];
      o *= scale[n];
      if (bias) o += bf2f(bias[n]);
      if (ACT == 1) o = nsa_gelu(o);
      if constexpr (OUTF)
        reinterpret_cast<float*>(y)[n] = o;
      else
        reinterpret_cast<bf16_t*>(y)[n] = f2bf(o);
    }
  }
}

template <int PRO>
hipError_t launch_gemv_row_q8(const RowPro& a, const void* Wq, const void* scale, const void* bias, void* y, int N,
                              int K, int act, int out_f32, hipStream_t s) {
  const size_t lds = row_lds_bytes<PRO>(a, K);
  const int8_t* w = (const int8_t*)Wq;
  const float* sc = (const float*)scale;
  const bf16_t* b = (const bf16_t*)bias;
  q8_cfg(K, [&](auto KW, auto P) {
    // columns per wave set: 4 as the bf16 kernel, 2 where one wave covers K (K <= 1024: 8 columns per
    // block; measured per token at batch 1, GPT-2 124M: 0.309 ms with 2, 0.319 with 4; bf16 0.336)
    constexpr int kw = decltype(KW)::value, nc = kw == 1 ? 2 : 4;
    // at most gemv_row_grid() workgroups, each looping over column blocks
    constexpr int bn = (4 / kw) * nc;
    const int nblk = (N + bn - 1) / bn;
    const unsigned grid = (unsigned)std::min(nblk, gemv_row_grid());
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      gemv_row_q8_kernel<PRO, decltype(ACT)::value, decltype(OUTF)::value, nc, kw, decltype(P)::value>
          <<<grid, 256, lds, s>>>(a, w, sc, b, y, N, K);
    });
  });
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Skinny GEMM (2..16 decode rows on the matrix cores), int8 weights.  As in
// skinny_gemm_kernel the weight is the A operand of v_mfma_f32_16x16x32_bf16 (lane l: row
// n0 + (l & 15)) and X^T the B operand (lane l: batch row l & 15).  A lane's 16-byte weight
// load holds 16 consecutive k of its row, the k of a 64-wide unit u being
//   64 u + 16 (l >> 4) + 8 h + i,   h = 0, 1 (the MFMA), i = 0 .. 7 (the fragment element),
// so one load feeds two MFMAs, and the X fragment of MFMA h is the 16 bytes of the batch
// row at the same k: the two fragments permute k alike, which a dot product does not see.
// The 8 bytes of a fragment become bf16 in registers (q8frag).  Any N: weight rows past
// the end read row N - 1 and their outputs are not stored.
// ---------------------------------------------------------------------------
template <int ACT, bool OUTF>
__device__ __forceinline__ void skinny_q8_epilogue(const f32x4& acc, float (*red)[4][64],
                                                   const float* __restrict__ scale, const bf16_t* __restrict__ bias,
                                                   void* __restrict__ yv, int M, int N, int n0) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // C layout: lane l holds column m = l & 15 of the 16-row group, rows n = 4 (l >> 4) + i
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  const int n = tid & 15, m = tid >> 4;  // n fastest: coalesced stores
  if (m < M && n0 + n < N) {
    const int i = n & 3, ln = 16 * (n >> 2) + m;
    float o = red[0][i][ln] + red[1][i][ln] + red[2][i][ln] + red[3][i][ln];
    o *= scale[n0 + n];
    if (bias) o += bf2f(bias[n0 + n]);
    if constexpr (ACT == 1) o = nsa_gelu(o);
    if constexpr (OUTF)
      reinterpret_cast<float*>(yv)[(int64_t)m * N + n0 + n] = o;
    else
      reinterpret_cast<bf16_t*>(yv)[(int64_t)m * N + n0 + n] = f2bf(o);
  }
}

// UN 64-wide units per wave in flight; units past the end re-read the last unit with a zero
// weight fragment (branch-free, so every load of a round issues before any wait)
template <int ACT, bool OUTF, int UN>
__global__ __launch_bounds__(256) void skinny_gemm_q8_kernel(const bf16_t* __restrict__ x,
                                                             const int8_t* __restrict__ Wq,
                                                             const float* __restrict__ scale,
                                                             const bf16_t* __restrict__ bias, void* __restrict__ yv,
                                                             int M, int N, int K) {
  __shared__ float red[4][4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int g = lane >> 4, c = lane & 15;
  const int8_t* wrow = Wq + (int64_t)min(n0 + c, N - 1) * K + 16 * g;
  const bf16_t* xrow = x + (int64_t)min(c, M - 1) * K + 16 * g;
  f32x4 acc = f32x4{};
  const int U = K / 64;  // wave w takes units w, w + 4, w + 8, ...
  for (int u0 = w; u0 < U; u0 += 4 * UN) {
    uint4 a[UN], b[UN][2];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int uu = u0 + 4 * j;
      const int uc = uu < U ? uu : U - 1;
      a[j] = *reinterpret_cast<const uint4*>(wrow + 64 * uc);
      if (uu >= U) a[j] = uint4{0u, 0u, 0u, 0u};
      b[j][0] = *reinterpret_cast<const uint4*>(xrow + 64 * uc);
      b[j][1] = *reinterpret_cast<const uint4*>(xrow + 64 * uc + 8);
    }
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q8frag(a[j].x, a[j].y), __builtin_bit_cast(bf16x8, b[j][0]), acc,
                                                    0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q8frag(a[j].z, a[j].w), __builtin_bit_cast(bf16x8, b[j][1]), acc,
                                                    0, 0, 0);
    }
  }
  skinny_q8_epilogue<ACT, OUTF>(acc, red, scale, bias, yv, M, N, n0);
}

// The same with the residual add + LayerNorm in the prologue (skinny_ln_gemm_kernel's
// counterpart): the first round of weight loads is issued before the prologue and each
// round prefetches the next, so the weight stream overlaps the LayerNorm.
template <int ACT, bool OUTF>
__global__ __launch_bounds__(256) void skinny_ln_gemm_q8_kernel(const float* __restrict__ res,
                                                                const bf16_t* __restrict__ branch,
                                                                float* __restrict__ s_out,
                                                                const bf16_t* __restrict__ lw,
                                                                const bf16_t* __restrict__ lb, float eps,
                                                                const int8_t* __restrict__ Wq,
                                                                const float* __restrict__ scale,
                                                                const bf16_t* __restrict__ bias,
                                                                void* __restrict__ yv, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [16][K + 8]
  __shared__ float red[4][4][64];
  const int KP = K + 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int g = lane >> 4, c = lane & 15;
  const int8_t* wrow = Wq + (int64_t)min(n0 + c, N - 1) * K + 16 * g;
  const int U = K / 64;
  constexpr int UN = 4;
  uint4 a[UN];
  auto load_a = [&](int u0, uint4 (&dst)[UN]) {
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int uu = u0 + 4 * j;
      dst[j] = *reinterpret_cast<const uint4*>(wrow + 64 * (uu < U ? uu : U - 1));
      if (uu >= U) dst[j] = uint4{0u, 0u, 0u, 0u};
    }
  };
  load_a(w, a);
  skinny_ln_prologue(res, branch, s_out, lw, lb, eps, xs, M, K);
  __syncthreads();
  f32x4 acc = f32x4{};
  for (int u0 = w; u0 < U; u0 += 4 * UN) {
    uint4 b[UN][2];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int uu = u0 + 4 * j;
      const bf16_t* xp = xs + c * KP + 64 * (uu < U ? uu : U - 1) + 16 * g;
      b[j][0] = *reinterpret_cast<const uint4*>(xp);
      b[j][1] = *reinterpret_cast<const uint4*>(xp + 8);
    }
    uint4 an[UN];
    const bool more = u0 + 4 * UN < U;  // wave-uniform
    if (more) load_a(u0 + 4 * UN, an);
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q8frag(a[j].x, a[j].y), __builtin_bit_cast(bf16x8, b[j][0]), acc,
                                                    0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q8frag(a[j].z, a[j].w), __builtin_bit_cast(bf16x8, b[j][1]), acc,
                                                    0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < UN; ++j) a[j] = an[j];
    }
  }
  skinny_q8_epilogue<ACT, OUTF>(acc, red, scale, bias, yv, M, N, n0);
}

}  // namespace

// y[rows, N] = act((x[rows, K] Wq[N, K]^T) * scale[N] + b), rows <= 8, any N, K % 16 == 0;
// Wq int8, scale fp32, x / b bf16; act: 0 none, 1 exact-erf GELU; out_f32: y is fp32.
NSA_API hipError_t nsa_gemv_q8(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int rows,
                               int N, int K, int act, int out_f32, hipStream_t s) {
  if (rows < 1 || rows > GEMV_MAX_ROWS || K % ROW_K_Q8 || K < ROW_K_Q8 || N < 1 || (act && out_f32))
    return hipErrorInvalidValue;
  const bf16_t* xb = (const bf16_t*)x;
  const int8_t* w = (const int8_t*)Wq;
  const float* sc = (const float*)scale;
  const bf16_t* b = (const bf16_t*)bias;
  auto launch = [&](auto M) {  // the K loop of the multi-row kernel
    const unsigned grid = (unsigned)((N + 7) / 8);
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      gemv_q8_kernel<decltype(M)::value, decltype(ACT)::value, decltype(OUTF)::value, 8, 4>
          <<<grid, 256, 0, s>>>(xb, w, sc, b, y, rows, N, K);
    });
  };
  if (rows == 1 && K <= ROW_MAX_K) {
    // one row: 2 columns per wave set (narrow outputs need many small workgroups to keep
    // enough weight bytes in flight), as the bf16 kernel's NSA_GEMV1_NC default
    q8_cfg(K, [&](auto KW, auto P) {
      constexpr int bn = (4 / decltype(KW)::value) * 2;
      const unsigned g1 = (unsigned)((N + bn - 1) / bn);
      epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
        gemv1_q8_kernel<decltype(ACT)::value, decltype(OUTF)::value, 2, decltype(KW)::value, decltype(P)::value>
            <<<g1, 256, 0, s>>>(xb, w, sc, b, y, N, K);
      });
    });
  } else if (rows == 1)  // wider than ROW_MAX_K
    launch(int_c<1>{});
  else if (rows == 2)
    launch(int_c<2>{});
  else if (rows <= 4)
    launch(int_c<4>{});
  else
    launch(int_c<8>{});
  return hipGetLastError();
}

// nsa_gemv_ln with int8 weights: K % 16 == 0, K <= 8192, any N
NSA_API hipError_t nsa_gemv_ln_q8(const void* res, const void* branch, void* res_out, const void* lw, const void* lb,
                                  const void* Wq, const void* scale, const void* bias, void* y, int N, int K,
                                  float eps, int act, int out_f32, void* pos_inc, hipStream_t s) {
  if (K < ROW_K_Q8 || !row_ln_ok(res, branch, res_out, N, K, ROW_K_Q8, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row_q8<PRO_LN>(row_ln(res, branch, res_out, lw, lb, eps, pos_inc), Wq, scale, bias, y, N, K, act,
                                    out_f32, s);
}

// nsa_gemv_emb_ln with an int8 linear (the wte / wpe rows stay bf16)
NSA_API hipError_t nsa_gemv_emb_ln_q8(const void* tok, const void* pos, const void* wte, const void* wpe,
                                      void* res_out, const void* lw, const void* lb, const void* Wq, const void* scale,
                                      const void* bias, void* y, int N, int K, float eps, int act, int out_f32,
                                      hipStream_t s) {
  if (K < ROW_K_Q8 || !row_emb_ln_ok(res_out, N, K, ROW_K_Q8, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row_q8<PRO_EMB_LN>(row_emb_ln(tok, pos, wte, wpe, res_out, lw, lb, eps), Wq, scale, bias, y, N,
                                        K, act, out_f32, s);
}

// nsa_gemv_attn with int8 weights (K = H * 64: a multiple of 16)
NSA_API hipError_t nsa_gemv_attn_q8(const void* ws, int n_split, const void* Wq, const void* scale, const void* bias,
                                    void* y, int N, int K, int act, int out_f32, hipStream_t s) {
  if (K < DA_D || !row_attn_ok(n_split, N, K, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row_q8<PRO_ATTN>(row_attn(ws, n_split), Wq, scale, bias, y, N, K, act, out_f32, s);
}

// y[rows, N] = act((x[rows, K] Wq[N, K]^T) * scale[N] + b) for 2 <= rows <= 16, any N, K % 64 == 0
NSA_API hipError_t nsa_skinny_gemm_q8(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                      int rows, int N, int K, int act, int out_f32, hipStream_t s) {
  if (rows < 1 || rows > SKINNY_GROUP_ROWS || K % SKINNY_K_Q8 || K < SKINNY_K_Q8 || N < 1 || (act && out_f32))
    return hipErrorInvalidValue;
  const unsigned grid = (unsigned)((N + 15) / 16);
  auto launch = [&](auto UN) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      skinny_gemm_q8_kernel<decltype(ACT)::value, decltype(OUTF)::value, decltype(UN)::value><<<grid, 256, 0, s>>>(
          (const bf16_t*)x, (const int8_t*)Wq, (const float*)scale, (const bf16_t*)bias, y, rows, N, K);
    });
  };
  // 4 units (1024 k over the workgroup) in flight per round up to K = 1024, 8 beyond
  if (K <= 1024)
    launch(int_c<4>{});
  else
    launch(int_c<8>{});
  return hipGetLastError();
}

// nsa_skinny_ln_gemm with int8 weights: any N, K % 64 == 0, K <= 1920
NSA_API hipError_t nsa_skinny_ln_gemm_q8(const void* res, const void* branch, void* s_out, const void* lw,
                                         const void* lb, float eps, const void* Wq, const void* scale,
                                         const void* bias, void* y, int rows, int N, int K, int act, int out_f32,
                                         hipStream_t s) {
  if (rows < 1 || rows > SKINNY_GROUP_ROWS || K % SKINNY_K_Q8 || K < SKINNY_K_Q8 || K > SKINNY_LN_MAX_K || N < 1 ||
      (act && out_f32) || (branch && !s_out))
    return hipErrorInvalidValue;
  if (!branch) s_out = nullptr;  // s is res itself: nothing to write (as the single-row kernel)
  const unsigned grid = (unsigned)((N + 15) / 16);
  const size_t lds = (size_t)16 * (K + 8) * sizeof(bf16_t);
  epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
    skinny_ln_gemm_q8_kernel<decltype(ACT)::value, decltype(OUTF)::value><<<grid, 256, lds, s>>>(
        (const float*)res, (const bf16_t*)branch, (float*)s_out, (const bf16_t*)lw, (const bf16_t*)lb, eps,
        (const int8_t*)Wq, (const float*)scale, (const bf16_t*)bias, y, rows, N, K);
  });
  return hipGetLastError();
}
