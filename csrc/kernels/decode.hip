// Incremental decoding (serving path): KV-cache append and single-query attention
// over the cache for gfx950.  nanoGPT's generate() re-runs the whole context for
// every new token (reference sample.py -> model.generate, SURVEY.md §2.3 U-M11 /
// U-S1); runtime/decode.py keeps per-layer K/V caches instead and replays one
// token's forward as a HIP graph, so the position of the token being decoded lives
// in device memory (`pos`) and every kernel here reads it there: nothing in the
// captured step depends on a host value that changes between tokens.
//
// Cache layout: K and V as [B, H, Tmax, D] bf16, one 128-byte row per key at D = 64
// (a wave reads 64 consecutive rows = 8 KiB contiguous for the scores, and one
// 128-byte row per key for the weighted V sum).
//
// Attention (flash-decoding): the cache is split into 256-key chunks; workgroup
// (b*H + h, s) scores its chunk's keys (one key per thread, q in LDS), forms the
// chunk-local softmax (max m, sum l) and the chunk's weighted V sum o, and writes
// (m, l, o[64]) to a workspace; a combine kernel rescales the chunks to the global
// max.  Chunks past `pos` write an empty partial (m = -inf) and exit, so the grid is
// fixed by Tmax (graph-safe) while the work follows the live context length.
//
// Int8 caches (Decoder(..., kv_quantize="int8")): K and V as int8 [B, H, Tmax, 64], one
// 64-byte row per key, with one fp32 scale per row ([B, H, Tmax], one tensor each for K and
// V); a row stands for q * scale (ops.quantize_cache_rows: scale = absmax / 127, q =
// rint(x / scale)).  The partial kernel is the bf16 one instantiated on the cache's element
// type: same grid, chunks and workspace, so the combine kernel and the nsa_gemv_attn
// prologues read its partials unchanged.
//
// Also here: the weight-streaming decode linears (GEMV / skinny GEMM with their prologues)
// and the per-row position advance.  The step's sampler is sample.hip; the chunk body of the
// attention and its combine kernel are decode_attn.h (shared with decode_shared.hip).
#include "decode_attn.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>

namespace {

// ROWS (nsa_kv_append_rows): row b of qkv goes to cache row rows[b] of a cache of Bc rows (an
// admission into a running batch); an index outside 0 .. Bc - 1 writes nothing.
template <bool ROWS>
__global__ __launch_bounds__(256) void kv_append_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                        bf16_t* __restrict__ vc, const int64_t* __restrict__ pos_dev,
                                                        int pos0, int B, int S, int H, int D, int Tmax,
                                                        const int64_t* __restrict__ rows, int Bc) {
  // one thread per 16-byte chunk of a K or V row: index = (((b*S + s)*2 + kv)*H + h)*cpr + c
  const int cpr = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)B * S * 2 * H * cpr;
  if (i >= total) return;
  const int c = (int)(i % cpr);
  int64_t r = i / cpr;
  const int hh = (int)(r % H);
  r /= H;
  const int kv = (int)(r & 1);
  r >>= 1;
  const int s = (int)(r % S);
  const int b = (int)(r / S);
  const int p = (pos_dev ? (int)*pos_dev : pos0) + s;
  if (p < 0 || p >= Tmax) return;
  const int C = H * D;
  int64_t cb = b;  // the cache row
  if (ROWS) {
    cb = rows[b];
    if (cb < 0 || cb >= Bc) return;
  }
  const bf16_t* src = qkv + ((int64_t)b * S + s) * 3 * C + (1 + kv) * C + hh * D + c * 8;
  bf16_t* dst = (kv ? vc : kc) + ((cb * H + hh) * Tmax + p) * D + c * 8;
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}

// kv_append_kernel for int8 caches (D = 64): an 8-lane group per K or V row, lane c holds the
// row's values 8c .. 8c+7; index = (((b*S + s)*2 + kv)*H + h)*8 + c.  The row's absmax meets in
// three shuffles inside the group (groups never straddle the early exits: 256 and the total are
// multiples of 8, and the position and, with ROWS, the cache row are the group's).  ROWS: as above.
template <bool ROWS>
__global__ __launch_bounds__(256) void kv_append_kv8_kernel(const bf16_t* __restrict__ qkv, int8_t* __restrict__ kq,
                                                            float* __restrict__ ksc, int8_t* __restrict__ vq,
                                                            float* __restrict__ vsc,
                                                            const int64_t* __restrict__ pos_dev, int pos0, int B,
                                                            int S, int H, int Tmax,
                                                            const int64_t* __restrict__ rows, int Bc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)B * S * 2 * H * 8;
  if (i >= total) return;
  const int c = (int)(i & 7);
  int64_t r = i >> 3;
  const int hh = (int)(r % H);
  r /= H;
  const int kv = (int)(r & 1);
  r >>= 1;
  const int s = (int)(r % S);
  const int b = (int)(r / S);
  const int p = (pos_dev ? (int)*pos_dev : pos0) + s;
  if (p < 0 || p >= Tmax) return;
  int64_t cb = b;  // the cache row
  if (ROWS) {
    cb = rows[b];
    if (cb < 0 || cb >= Bc) return;
  }
  const int C = H * DA_D;
  float x[8];
  load8(qkv + ((int64_t)b * S + s) * 3 * C + (1 + kv) * C + hh * DA_D + c * 8, x);
  float am = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(x[j]));
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) am = fmaxf(am, __shfl_xor(am, off, 64));
  const float sc = kv8_scale(am);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = kv8_quant(x[j], sc);
  const int64_t row = (cb * H + hh) * Tmax + p;
  *reinterpret_cast<uint2*>((kv ? vq : kq) + row * DA_D + c * 8) =
      uint2{kv8_pack4(x[0], x[1], x[2], x[3]), kv8_pack4(x[4], x[5], x[6], x[7])};
  if (c == 0) (kv ? vsc : ksc)[row] = sc;
}

// grid (B*H, n_split), 256 threads; pos_dev[b * pos_stride] is row b's position.  Workgroup
// (b*H + h, s) runs decode_attn_chunk (decode_attn.h) on chunk s of row b's caches.
// CT: the cache's element type (bf16_t, or int8_t with the per-row scales in cs: the last
// argument, empty in the bf16 form, whose other arguments sit where they always did).
template <typename CT>
__global__ __launch_bounds__(256) void decode_attn_partial_kernel(const bf16_t* __restrict__ qkv,
                                                                  const CT* __restrict__ kc,
                                                                  const CT* __restrict__ vc, CT* kc_w, CT* vc_w,
                                                                  const int64_t* __restrict__ pos_dev,
                                                                  int pos_stride, float* __restrict__ ws, int H,
                                                                  int Tmax, float scale_log2, int append,
                                                                  const CacheScales<CT> cs) {
  const int bh = blockIdx.x, s = blockIdx.y, n_split = gridDim.y;
  const int b = bh / H, hh = bh % H;
  const int C = H * DA_D;
  // the query's own position = the newest key: one for the batch (pos_stride 0) or one per
  // row (pos_stride 1); b comes from blockIdx, so every branch on it is workgroup-uniform
  const int pos = (int)pos_dev[(int64_t)b * pos_stride];
  decode_attn_chunk<CT>(qkv + (int64_t)b * 3 * C + hh * DA_D, kc, vc, kc_w, vc_w, cs, (int64_t)bh * Tmax, pos, Tmax,
                        s * DA_CHUNK, ws + ((int64_t)bh * n_split + s) * DA_PART, C, scale_log2, append);
}

// The per-row decode step's position update: an unfinished row moves on by one, a
// finished row stays where it is (it is fed the same token at the same position again).
__global__ void pos_advance_kernel(int64_t* __restrict__ pos, const int64_t* __restrict__ done, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && done[b] == 0) pos[b] += 1;
}

// ---------------------------------------------------------------------------
// Decode linear: y[m, n] = act(sum_k x[m, k] W[n, k] + b[n]) for M <= 8 rows (the
// decode batch), bf16 in / out, fp32 accumulation.  At these M every nn.Linear is a
// weight stream: one kernel with the bias (and GELU) in its epilogue replaces the
// library GEMM plus the bias-broadcast copy `addmm` issues, two launches per linear.
// Workgroup = 8 output columns; its 4 waves split K (16-byte pieces: chunk
// g = (it * 4 + wave) * 64 + lane covers k = 8g .. 8g+7), each lane keeps 8 x M partial
// dot products, a butterfly (halve-and-exchange) shuffle reduction leaves each lane
// with one (column, row) total over the wave, and the 4 waves meet in LDS.
// ---------------------------------------------------------------------------
template <int M, int ACT, bool OUTF, int NC = 8>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                   const bf16_t* __restrict__ bias, void* __restrict__ y, int rows,
                                                   int N, int K) {
  constexpr int V = NC * M;
  __shared__ float red[4][V];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * NC;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0f;
  const int nchunk = K / 8;
#pragma unroll 4
  for (int g = w * 64 + lane; g < nchunk; g += 256) {
    const int k = 8 * g;
    float xf[M][8];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (m < rows) load8(x + (int64_t)m * K + k, xf[m]);
      else
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[m][j] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float wf[8];
      load8(W + (int64_t)min(n0 + c, N - 1) * K + k, wf);
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c * M + m] = fmaf(xf[m][j], wf[j], acc[c * M + m]);
    }
  }
  int idx;
  const float v = wave_reduce_multi<V>(acc, lane, idx);
  // lanes below the last split's offset hold duplicates: the first of each group writes
  constexpr int DUP = 64 / V;  // lanes per value
  if ((lane & (DUP - 1)) == 0) red[w][idx] = v;
  __syncthreads();
  if (tid < V) {
    const int c = tid / M, m = tid % M, n = n0 + c;
    if (m < rows && n < N) {
      float o = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      if (bias) o += bf2f(bias[n]);
      if (ACT == 1) o = nsa_gelu(o);
      if constexpr (OUTF)
        reinterpret_cast<float*>(y)[(int64_t)m * N + n] = o;
      else
        reinterpret_cast<bf16_t*>(y)[(int64_t)m * N + n] = f2bf(o);
    }
  }
}

// Single-row decode linear with its input's producer in the prologue (decode_rows.h: PRO_*,
// RowPro): the row x[K] is built in LDS by decode_row_prologue.h, k-contiguous.
template <int PRO, int ACT, bool OUTF, int NC>
__global__ __launch_bounds__(256) void gemv_row_kernel(const RowPro a, const bf16_t* __restrict__ W,
                                                       const bf16_t* __restrict__ bias, void* __restrict__ y, int N,
                                                       int K) {
  extern __shared__ float hs[];  // [K] input row
  __shared__ float red[4][NC];
  __shared__ float stat[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nchunk = K / 8, g0 = w * 64 + lane;
  const int nblk = (N + NC - 1) / NC;
  int cb = blockIdx.x;  // column blocks cb, cb + gridDim.x, ...: the prologue runs once per workgroup
  uint4 wp[NC];  // first K piece of the next block's weight rows, in flight ahead of use
  if (g0 < nchunk) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      wp[c] = *reinterpret_cast<const uint4*>(W + (int64_t)min(cb * NC + c, N - 1) * K + 8 * g0);
  }
  // prologue: the row x[K] into hs[k]
#define NSA_HS(k) (k)
#include "decode_row_prologue.h"
#undef NSA_HS
  __syncthreads();
  for (; cb < nblk; cb += gridDim.x) {
    const int n0 = cb * NC;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
    if (g0 < nchunk) {
      float xf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) xf[j] = hs[8 * g0 + j];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float wf[8];
        unpack8(wp[c], wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c] = fmaf(xf[j], wf[j], acc[c]);
      }
    }
    for (int g = g0 + 256; g < nchunk; g += 256) {
      const int k = 8 * g;
      float xf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) xf[j] = hs[k + j];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float wf[8];
        load8(W + (int64_t)min(n0 + c, N - 1) * K + k, wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c] = fmaf(xf[j], wf[j], acc[c]);
      }
    }
    const int nb = cb + gridDim.x;
    if (nb < nblk && g0 < nchunk) {  // next block's first piece: in flight during the reduction
#pragma unroll
      for (int c = 0; c < NC; ++c)
        wp[c] = *reinterpret_cast<const uint4*>(W + (int64_t)min(nb * NC + c, N - 1) * K + 8 * g0);
    }
    int idx;
    const float v = wave_reduce_multi<NC>(acc, lane, idx);
    if ((lane & (64 / NC - 1)) == 0) red[w][idx] = v;
    __syncthreads();
    if (tid < NC) {
      const int n = n0 + tid;
      if (n < N) {
        float o = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
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

// NSA_GEMV_NC: output columns per workgroup block (2, 4, 8 or 16)
int env_nc(const char* name) {  // 0: unset
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return v == 2 || v == 4 || v == 8 || v == 16 ? v : 0;
}
int gemv_row_nc() {  // default 4: measured per-token decode (graph) 124M 0.372 / 1.5B 2.065 ms at 8, 0.336 / 1.901 at 4
  static const int n = env_nc("NSA_GEMV_NC");
  return n ? n : 4;
}

// NSA_GEMV1_NC: columns per workgroup of the plain one-row GEMV (default 2: the narrow
// MLP down-projection, N = C, gets C / 2 workgroups; 4 / 8 measured 1-3% slower per token)
int gemv1_nc() {
  static const int n = env_nc("NSA_GEMV1_NC");
  return n ? n : 2;
}

template <int PRO>
hipError_t launch_gemv_row(const RowPro& a, const void* W, const void* bias, void* y, int N, int K, int act,
                           int out_f32, hipStream_t s) {
  const size_t lds = row_lds_bytes<PRO>(a, K);
  const bf16_t* w = (const bf16_t*)W;
  const bf16_t* b = (const bf16_t*)bias;
  // at most gemv_row_grid() workgroups, each looping over column blocks (the vocabulary
  // head: ~6 blocks per workgroup instead of one prologue per 8 columns)
  const int nc = gemv_row_nc();
  const int nblk = (N + nc - 1) / nc;
  const unsigned grid = (unsigned)std::min(nblk, gemv_row_grid());
  auto launch = [&](auto NC) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      gemv_row_kernel<PRO, decltype(ACT)::value, decltype(OUTF)::value, decltype(NC)::value>
          <<<grid, 256, lds, s>>>(a, w, b, y, N, K);
    });
  };
  if (nc == 16)
    launch(int_c<16>{});
  else if (nc == 4)
    launch(int_c<4>{});
  else if (nc == 2)
    launch(int_c<2>{});
  else
    launch(int_c<8>{});
  return hipGetLastError();
}

}  // namespace

// K/V rows of qkv [B, S, 3C] -> caches [B, H, Tmax, D] at positions p0 .. p0+S-1 where
// p0 = *pos (int64 device scalar) or, with pos == NULL, the host value pos0.
NSA_API hipError_t nsa_kv_append(const void* qkv, void* kc, void* vc, const void* pos, int pos0, int B, int S, int H,
                                 int D, int Tmax, hipStream_t s) {
  if (D % 8 || B < 1 || S < 1) return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * S * 2 * H * (D / 8);
  kv_append_kernel<false><<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
      (const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (const int64_t*)pos, pos0, B, S, H, D, Tmax, nullptr, B);
  return hipGetLastError();
}

// nsa_kv_append into chosen cache rows: the K / V rows of qkv [n, S, 3C] go to cache row rows[j]
// (int64 [n] on the device, distinct, each < B) of caches [B, H, Tmax, D]; one launch for any n.
NSA_API hipError_t nsa_kv_append_rows(const void* qkv, void* kc, void* vc, const void* rows, int pos0, int n, int B,
                                      int S, int H, int D, int Tmax, hipStream_t s) {
  if (D % 8 || n < 1 || B < 1 || S < 1 || pos0 < 0 || !rows) return hipErrorInvalidValue;
  const int64_t total = (int64_t)n * S * 2 * H * (D / 8);
  kv_append_kernel<true><<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
      (const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, nullptr, pos0, n, S, H, D, Tmax, (const int64_t*)rows, B);
  return hipGetLastError();
}

// nsa_kv_append for int8 caches (D = 64): every K / V row of qkv is quantized (one fp32 scale
// per row into ksc / vsc [B, H, Tmax]) and stored at its position.
NSA_API hipError_t nsa_kv_append_kv8(const void* qkv, void* kq, void* ksc, void* vq, void* vsc, const void* pos,
                                     int pos0, int B, int S, int H, int D, int Tmax, hipStream_t s) {
  if (D != DA_D || B < 1 || S < 1 || H < 1 || Tmax < 1) return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * S * 2 * H * 8;
  kv_append_kv8_kernel<false><<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
      (const bf16_t*)qkv, (int8_t*)kq, (float*)ksc, (int8_t*)vq, (float*)vsc, (const int64_t*)pos, pos0, B, S, H, Tmax,
      nullptr, B);
  return hipGetLastError();
}

// nsa_kv_append_rows for int8 caches (D = 64): the same quantizer, into cache rows rows[j].
NSA_API hipError_t nsa_kv_append_rows_kv8(const void* qkv, void* kq, void* ksc, void* vq, void* vsc, const void* rows,
                                          int pos0, int n, int B, int S, int H, int D, int Tmax, hipStream_t s) {
  if (D != DA_D || n < 1 || B < 1 || S < 1 || H < 1 || Tmax < 1 || pos0 < 0 || !rows) return hipErrorInvalidValue;
  const int64_t total = (int64_t)n * S * 2 * H * 8;
  kv_append_kv8_kernel<true><<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
      (const bf16_t*)qkv, (int8_t*)kq, (float*)ksc, (int8_t*)vq, (float*)vsc, nullptr, pos0, n, S, H, Tmax,
      (const int64_t*)rows, B);
  return hipGetLastError();
}

// Single-query causal attention of the newest token (position *pos) over the caches.
// qkv: [B, 1, 3C] (q | k | v); out: [B, C] bf16; ws: B*H*ceil(Tmax/256)*68 fp32.
// append != 0: the new token's K / V are taken from qkv and stored at *pos (fused
// kv_append); otherwise the caches must already hold position *pos.  out == NULL leaves
// the partials in ws for nsa_gemv_attn.
// CT = int8_t: int8 caches with their per-row scales ksc / vsc (fp32 [B, H, Tmax])
template <typename CT>
static hipError_t decode_attn_launch(const void* qkv, void* kc, void* vc, void* ksc, void* vsc, const void* pos,
                                     int pos_stride, void* ws, void* out, int B, int H, int D, int Tmax, float scale,
                                     int append, hipStream_t s) {
  if (D != DA_D || B < 1 || H < 1 || Tmax < 1) return hipErrorInvalidValue;
  CacheScales<CT> cs;
  if constexpr (sizeof(CT) == 1) {
    if (!ksc || !vsc) return hipErrorInvalidValue;
    cs.k = (float*)ksc;
    cs.v = (float*)vsc;
  }
  const int n_split = (Tmax + DA_CHUNK - 1) / DA_CHUNK;
  decode_attn_partial_kernel<CT><<<dim3(B * H, n_split), 256, 0, s>>>(
      (const bf16_t*)qkv, (const CT*)kc, (const CT*)vc, (CT*)kc, (CT*)vc, (const int64_t*)pos, pos_stride, (float*)ws,
      H, Tmax, scale * 1.4426950408889634f, append, cs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !out) return e;  // out == NULL: the consumer combines (nsa_gemv_attn)
  decode_attn_combine_kernel<<<B * H, 64, 0, s>>>((const float*)ws, (bf16_t*)out, H, n_split);
  return hipGetLastError();
}

NSA_API hipError_t nsa_decode_attn(const void* qkv, void* kc, void* vc, const void* pos, void* ws, void* out, int B,
                                   int H, int D, int Tmax, float scale, int append, hipStream_t s) {
  return decode_attn_launch<bf16_t>(qkv, kc, vc, nullptr, nullptr, pos, 0, ws, out, B, H, D, Tmax, scale, append, s);
}

// The same with one position per row: pos is int64[B], row b attends over keys
// 0 .. pos[b] and (append) stores its K / V at pos[b].  Same kernels, same partials.
NSA_API hipError_t nsa_decode_attn_rows(const void* qkv, void* kc, void* vc, const void* pos, void* ws, void* out,
                                        int B, int H, int D, int Tmax, float scale, int append, hipStream_t s) {
  return decode_attn_launch<bf16_t>(qkv, kc, vc, nullptr, nullptr, pos, 1, ws, out, B, H, D, Tmax, scale, append, s);
}

// The same two over int8 caches: kq / vq int8 [B, H, Tmax, 64], ksc / vsc fp32 [B, H, Tmax], a
// row standing for q * scale.  append quantizes the new token's K / V rows into them.  Same
// grid, same partials in ws, same combine.
NSA_API hipError_t nsa_decode_attn_kv8(const void* qkv, void* kq, void* ksc, void* vq, void* vsc, const void* pos,
                                       void* ws, void* out, int B, int H, int D, int Tmax, float scale, int append,
                                       hipStream_t s) {
  return decode_attn_launch<int8_t>(qkv, kq, vq, ksc, vsc, pos, 0, ws, out, B, H, D, Tmax, scale, append, s);
}

NSA_API hipError_t nsa_decode_attn_rows_kv8(const void* qkv, void* kq, void* ksc, void* vq, void* vsc,
                                            const void* pos, void* ws, void* out, int B, int H, int D, int Tmax,
                                            float scale, int append, hipStream_t s) {
  return decode_attn_launch<int8_t>(qkv, kq, vq, ksc, vsc, pos, 1, ws, out, B, H, D, Tmax, scale, append, s);
}

// pos[b] += 1 for every row with done[b] == 0 (int64[B] each): the per-row step's advance.
NSA_API hipError_t nsa_pos_advance(void* pos, const void* done, int B, hipStream_t s) {
  if (B < 1 || !pos || !done) return hipErrorInvalidValue;
  pos_advance_kernel<<<(B + 63) / 64, 64, 0, s>>>((int64_t*)pos, (const int64_t*)done, B);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Decode linear for a batch of 2 .. 64 rows on the matrix cores ("skinny GEMM").
// The vector GEMV keeps 8 x M fp32 partial dot products per lane and reduces them by
// shuffles, so its VALU cost grows with M; in round 2, from 2 rows on, the then-used
// library GEMM beat it while running at a few % of the MFMA rate (GPT-2 1.5B batch 8
// decoded at 4.2 ms/token against 1.9 at batch 1; no library GEMM is on this path any
// more: M > SKINNY_MAX_ROWS goes to our small-tile / NT kernels).  Here the weight is
// streamed once through v_mfma_f32_16x16x32_bf16 with the roles swapped:
//   Y^T[n, m] = W[n, k] · X^T[k, m]      A = 16 weight rows (lane l: row n0 + (l & 15),
//                                         16 contiguous bytes of it), B = X^T (lane l:
//                                         batch row m = l & 15 of a 16-row group),
// so every lane's weight load is a 16-byte piece of one weight row, and MT 16-row
// groups of X share each weight fragment.  Workgroup = 16 output columns; its NW = 4 waves
// take interleaved 32-wide K units (8 in flight per wave), then meet in
// LDS; the epilogue adds the bias, applies exact-erf GELU and stores Y[m, n] for m < M.
// Rows past M read row M - 1 (valid memory) and are never stored.
// ---------------------------------------------------------------------------
template <int MT, int ACT, bool OUTF, int NW = 4>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_kernel(const bf16_t* __restrict__ x,
                                                              const bf16_t* __restrict__ W,
                                                              const bf16_t* __restrict__ bias, void* __restrict__ yv,
                                                              int M, int N, int K) {
  __shared__ float red[NW][MT][4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int g = lane >> 4, c = lane & 15;
  const bf16_t* wrow = W + (int64_t)(n0 + c) * K + 8 * g;
  const bf16_t* xrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) xrow[t] = x + (int64_t)min(16 * t + c, M - 1) * K + 8 * g;
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{};
  const int U = K / 32;  // 32-wide K units; wave w takes units w, w + NW, w + 2 NW, ...
  // UN units per wave in flight; units past the end re-read the last unit with a zero
  // weight fragment (branch-free, so every load of an iteration issues before any wait)
  constexpr int UN = 8;
  for (int u0 = w; u0 < U; u0 += NW * UN) {
    uint4 a[UN], b[UN][MT];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int uu = u0 + NW * j;
      const int uc = uu < U ? uu : U - 1;
      a[j] = *reinterpret_cast<const uint4*>(wrow + 32 * uc);
      if (uu >= U) a[j] = uint4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int t = 0; t < MT; ++t) b[j][t] = *reinterpret_cast<const uint4*>(xrow[t] + 32 * uc);
    }
#pragma unroll
    for (int j = 0; j < UN; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[j]),
                                                         __builtin_bit_cast(bf16x8, b[j][t]), acc[t], 0, 0, 0);
  }
  // C layout: lane l holds column m = l & 15 of the 16-row group, rows n = 4 (l >> 4) + i
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[w][t][i][lane] = acc[t][i];
  __syncthreads();
  // 16 columns x 16 MT batch rows: thread e -> (m, n) with n fastest (coalesced stores)
  for (int e = tid; e < 16 * 16 * MT; e += NW * 64) {
    const int n = e & 15, m = e >> 4;
    if (m >= M) break;
    const int t = m >> 4, mc = m & 15;
    const int i = n & 3, ln = 16 * (n >> 2) + mc;
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < NW; ++q) v += red[q][t][i][ln];
    if (bias) v += bf2f(bias[n0 + n]);
    if constexpr (ACT == 1) v = nsa_gelu(v);
    if constexpr (OUTF)
      reinterpret_cast<float*>(yv)[(int64_t)m * N + n0 + n] = v;
    else
      reinterpret_cast<bf16_t*>(yv)[(int64_t)m * N + n0 + n] = f2bf(v);
  }
}

// y[rows, N] = act(x[rows, K] W[N, K]^T + b) for 2 <= rows <= 64 (N % 16 == 0, K % 32 == 0)
NSA_API hipError_t nsa_skinny_gemm(const void* x, const void* W, const void* bias, void* y, int rows, int N, int K,
                                   int act, int out_f32, hipStream_t s) {
  if (rows < 1 || rows > SKINNY_MAX_ROWS || N % 16 || K % SKINNY_K_BF16 || N < 16 || K < SKINNY_K_BF16 ||
      (act && out_f32))
    return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(N / 16);
  auto launch = [&](auto MT) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      skinny_gemm_kernel<decltype(MT)::value, decltype(ACT)::value, decltype(OUTF)::value>
          <<<grid, 256, 0, s>>>((const bf16_t*)x, (const bf16_t*)W, (const bf16_t*)bias, y, rows, N, K);
    });
  };
  // NW = 16 waves per workgroup (1024 threads) measured slower in the decode graph: GPT-2
  // 124M / 1.5B batch 8 0.733 / 3.84 ms/token vs 0.532 / 3.34 with NW = 4
  if (rows <= 16)
    launch(int_c<1>{});
  else if (rows <= 32)
    launch(int_c<2>{});
  else
    launch(int_c<4>{});
  return hipGetLastError();
}

// Skinny GEMM with the residual add + LayerNorm in the prologue (decode batches of
// 2..16 rows, the batch counterpart of gemv_row_kernel<PRO_LN>): every workgroup forms
// s = res + branch and x = LN(s) for all rows itself (wave w: rows w, w + 4, ...; a row of
// K <= 2048 lives in 32 registers per lane, two-pass mean / variance as nanoGPT's fp32
// LayerNorm), stores x as bf16 in LDS ([16][K + 8], padded rows) and reads the MFMA B
// fragments from there; workgroup 0 writes s (fp32).  The first round of weight loads is
// issued before the prologue and each round prefetches the next, so the weight stream
// overlaps the LayerNorm.  Removes the separate add+LayerNorm launch per linear.
template <int ACT, bool OUTF>
__global__ __launch_bounds__(256) void skinny_ln_gemm_kernel(const float* __restrict__ res,
                                                             const bf16_t* __restrict__ branch,
                                                             float* __restrict__ s_out, const bf16_t* __restrict__ lw,
                                                             const bf16_t* __restrict__ lb, float eps,
                                                             const bf16_t* __restrict__ W,
                                                             const bf16_t* __restrict__ bias, void* __restrict__ yv,
                                                             int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [16][K + 8]
  __shared__ float red[4][4][64];
  const int KP = K + 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int g = lane >> 4, c = lane & 15;
  const bf16_t* wrow = W + (int64_t)(n0 + c) * K + 8 * g;
  const int U = K / 32;
  constexpr int UN = 8;
  uint4 a[UN];
  auto load_a = [&](int u0, uint4 (&dst)[UN]) {
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int uu = u0 + 4 * j;
      dst[j] = *reinterpret_cast<const uint4*>(wrow + 32 * (uu < U ? uu : U - 1));
      if (uu >= U) dst[j] = uint4{0u, 0u, 0u, 0u};
    }
  };
  load_a(w, a);
  // prologue: LayerNorm of the M batch rows into LDS
#include "decode_skinny_ln_prologue.h"
  __syncthreads();
  f32x4 acc = f32x4{};
  for (int u0 = w; u0 < U; u0 += 4 * UN) {
    uint4 b[UN];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int uu = u0 + 4 * j;
      b[j] = *reinterpret_cast<const uint4*>(xs + c * KP + 32 * (uu < U ? uu : U - 1) + 8 * g);
    }
    uint4 an[UN];
    const bool more = u0 + 4 * UN < U;  // wave-uniform
    if (more) load_a(u0 + 4 * UN, an);
#pragma unroll
    for (int j = 0; j < UN; ++j)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[j]), __builtin_bit_cast(bf16x8, b[j]),
                                                    acc, 0, 0, 0);
    if (more) {
#pragma unroll
      for (int j = 0; j < UN; ++j) a[j] = an[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  {
    const int e = tid, n = e & 15, m = e >> 4;
    if (m < M) {
      const int i = n & 3, ln = 16 * (n >> 2) + m;
      float o = red[0][i][ln] + red[1][i][ln] + red[2][i][ln] + red[3][i][ln];
      if (bias) o += bf2f(bias[n0 + n]);
      if constexpr (ACT == 1) o = nsa_gelu(o);
      if constexpr (OUTF)
        reinterpret_cast<float*>(yv)[(int64_t)m * N + n0 + n] = o;
      else
        reinterpret_cast<bf16_t*>(yv)[(int64_t)m * N + n0 + n] = f2bf(o);
    }
  }
}

// (s, y) for 2..16 decode rows: s = res + branch (fp32, branch bf16 or NULL: s_out unused),
// y = act(LN(s) W^T + b); N % 16 == 0, K % 32 == 0, K <= 1920 (LDS image [16][K + 8] bf16)
NSA_API hipError_t nsa_skinny_ln_gemm(const void* res, const void* branch, void* s_out, const void* lw,
                                      const void* lb, float eps, const void* W, const void* bias, void* y, int rows,
                                      int N, int K, int act, int out_f32, hipStream_t s) {
  if (rows < 1 || rows > SKINNY_GROUP_ROWS || N % 16 || K % SKINNY_K_BF16 || N < 16 || K < SKINNY_K_BF16 ||
      K > SKINNY_LN_MAX_K || (act && out_f32) || (branch && !s_out))
    return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(N / 16);
  const size_t lds = (size_t)16 * (K + 8) * sizeof(bf16_t);
  if (!branch) s_out = nullptr;  // s is res itself: nothing to write (as the single-row kernel)
  epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
    skinny_ln_gemm_kernel<decltype(ACT)::value, decltype(OUTF)::value><<<grid, 256, lds, s>>>(
        (const float*)res, (const bf16_t*)branch, (float*)s_out, (const bf16_t*)lw, (const bf16_t*)lb, eps,
        (const bf16_t*)W, (const bf16_t*)bias, y, rows, N, K);
  });
  return hipGetLastError();
}

// Decode-batch linear y[rows, N] = act(x[rows, K] W[N, K]^T + b), rows <= 8, K % 8 == 0;
// act: 0 none, 1 exact-erf GELU; out_f32: y is fp32 (e.g. logits) instead of bf16.
// bias may be NULL.
NSA_API hipError_t nsa_gemv(const void* x, const void* W, const void* bias, void* y, int rows, int N, int K, int act,
                            int out_f32, hipStream_t s) {
  if (rows < 1 || rows > GEMV_MAX_ROWS || K % ROW_K_BF16 || N < 1 || (act && out_f32)) return hipErrorInvalidValue;
  auto launch = [&](auto M, auto NC) {  // M: rows the kernel is built for; NC: columns per workgroup
    const unsigned grid = (unsigned)((N + decltype(NC)::value - 1) / decltype(NC)::value);
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      gemv_kernel<decltype(M)::value, decltype(ACT)::value, decltype(OUTF)::value, decltype(NC)::value>
          <<<grid, 256, 0, s>>>((const bf16_t*)x, (const bf16_t*)W, (const bf16_t*)bias, y, rows, N, K);
    });
  };
  if (rows == 1) {
    // one row: NC columns per workgroup (narrow outputs need more, smaller workgroups to
    // keep enough weight bytes in flight)
    const int nc = gemv1_nc();
    if (nc == 2)
      launch(int_c<1>{}, int_c<2>{});
    else if (nc == 4)
      launch(int_c<1>{}, int_c<4>{});
    else
      launch(int_c<1>{}, int_c<8>{});
  } else if (rows == 2)
    launch(int_c<2>{}, int_c<8>{});
  else if (rows <= 4)
    launch(int_c<4>{}, int_c<8>{});
  else
    launch(int_c<8>{}, int_c<8>{});
  return hipGetLastError();
}

// One decode row: res_out = res + branch (if branch), h = LN(res [+ branch]) with (lw, lb),
// y = act(h W^T + bias) (fp32 y with out_f32).  K % 8 == 0, K <= 8192; res_out must not
// alias res.  pos_inc (may be NULL): an int64 the kernel increments once (the decode
// position, advanced by the step's last kernel instead of a separate add launch).
NSA_API hipError_t nsa_gemv_ln(const void* res, const void* branch, void* res_out, const void* lw, const void* lb,
                               const void* W, const void* bias, void* y, int N, int K, float eps, int act,
                               int out_f32, void* pos_inc, hipStream_t s) {
  if (!row_ln_ok(res, branch, res_out, N, K, ROW_K_BF16, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row<PRO_LN>(row_ln(res, branch, res_out, lw, lb, eps, pos_inc), W, bias, y, N, K, act, out_f32,
                                 s);
}

// First decode linear of a single-row step: res_out = wte[*tok] + wpe[*pos] (fp32, the
// residual stream), y = act(LN(res_out) W^T + bias).
NSA_API hipError_t nsa_gemv_emb_ln(const void* tok, const void* pos, const void* wte, const void* wpe, void* res_out,
                                   const void* lw, const void* lb, const void* W, const void* bias, void* y, int N,
                                   int K, float eps, int act, int out_f32, hipStream_t s) {
  if (!row_emb_ln_ok(res_out, N, K, ROW_K_BF16, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row<PRO_EMB_LN>(row_emb_ln(tok, pos, wte, wpe, res_out, lw, lb, eps), W, bias, y, N, K, act,
                                     out_f32, s);
}

// Single-row linear over the attention output: x = combine of the decode-attention
// partials ws (nsa_decode_attn with out == NULL, batch 1), K = H * 64.
NSA_API hipError_t nsa_gemv_attn(const void* ws, int n_split, const void* W, const void* bias, void* y, int N, int K,
                                 int act, int out_f32, hipStream_t s) {
  if (!row_attn_ok(n_split, N, K, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row<PRO_ATTN>(row_attn(ws, n_split), W, bias, y, N, K, act, out_f32, s);
}
