// MXFP4-weight forms of the weight-streaming decode kernels of decode.hip (the serving path
// with Decoder(..., quantize="mxfp4")): the weight of every linear is stored in the OCP MXFP4
// format (ops.quantize_mxfp4): E2M1 elements, two per byte (even k in the low nibble), in
// blocks of 32 along K with one E8M0 scale byte per block, 4.25 bits per weight.  All six compute
//   y[m, n] = act(sum_k x[m, k] fp4(q[n, k]) 2^(scale[n, k / 32] - 127) + bias[n])
// with x the bf16-rounded activation row the bf16 kernel forms and fp32 accumulation.  The block
// scale varies along K, so it cannot wait for the epilogue: it rides in the convert itself,
// v_cvt_scalef32_pk_{f32,bf16}_fp4 (two nibbles of a selected byte times an fp32 scale, one VALU
// instruction), as the fp32 with the bit pattern e << 23.  Every dequantized value is
// +-{0, .5, 1, 1.5, 2, 3, 4, 6} 2^s, exact in bf16 and in fp32, so the results differ from the
// bf16 kernels run on the dequantized weights by summation order alone.
//
// The prologues are the bf16 kernels' own, included as text as decode_q8.hip includes them
// (decode_row_prologue.h, decode_skinny_ln_prologue.h); declarations shared with the other two
// files are in decode_rows.h.
#include "decode_rows.h"

#include <math.h>

#include <algorithm>

namespace {

typedef float mx_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mx_bf16x2 __attribute__((ext_vector_type(2)));

// E8M0 scale byte e -> the fp32 2^(e - 127) (e in 1 .. 254: a normal number)
__device__ __forceinline__ float mx_scale(uint32_t e) { return __uint_as_float(e << 23); }

// ---------------------------------------------------------------------------
// One decode row.  A lane owns pieces of PB weight bytes = KP = 2 PB consecutive k of one
// weight row: PB = 16 is one MX block, PB = 8 half a block (two neighbouring lanes read the
// same scale byte).  Piece g covers k = KP g .. KP g + KP - 1.  As in the int8 kernels KW of
// the workgroup's 4 waves split K, the other 4 / KW wave sets take further columns, and a
// lane owns pieces g = kw * 64 + lane + p * 64 * KW, p < P: all weight and scale loads of a
// block of columns issue together, with no K loop.  Pieces past the end re-read the last
// piece and their weight dwords are zeroed (fp4 code 0: +0), branch-free; rows past N re-read
// row N - 1 and are not stored.
//
// Why two piece sizes.  K = 768 is 24 blocks: one block per lane keeps 24 of 64 lanes
// loading, half blocks 48 of 64, and at K = 1024 all 64.  The lanes of a wave that load, by K,
// for PB = 16 / PB = 8: 768 24/64 | 48/64; 1024 32/64 | 64/64; 1280 40/64 | 80/128; 1600
// 50/64 | 100/128; 3072 96/128 | 192/256; 6400 200/256 | 400/512.  Half blocks never load on
// fewer lanes; whole blocks need half the load instructions and leave more wave sets for
// columns.  mx_piece() holds the choice and the measurement behind it; NSA_MX4_PIECE (a
// compile-time override, for measuring only) forces one size.
// ---------------------------------------------------------------------------
template <int PB>
struct mx_vec;
template <>
struct mx_vec<8> {
  using type = uint2;
};
template <>
struct mx_vec<16> {
  using type = uint4;
};

template <int PB>
struct MxPiece {
  uint32_t d[PB / 4];  // 8 nibbles each: k = 8 j .. 8 j + 7 of the piece in dword j
  float s;             // the block's scale
};

// LDS position of x[k].  A lane multiplies one piece with KP values of x; k-contiguous rows
// would put lane g at a 4 KP-byte stride, all lanes of a read on a few banks.  The KP values
// sit as KP / 4 float4 at [j][g] (j = (k / 4) % (KP / 4), np = K / KP pieces), so the lanes of
// a wave read consecutive 16-byte vectors.
template <int KP>
__device__ __forceinline__ int hx(int k, int np) {
  return ((((k >> 2) % (KP / 4)) * np + k / KP) << 2) + (k & 3);
}

template <int PRO, int KP>
__device__ __forceinline__ void row_prologue(const RowPro& a, float* hs, float (*stat)[4], int K) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int np = K / KP;
#define NSA_HS(k) hx<KP>(k, np)
#include "decode_row_prologue.h"
#undef NSA_HS
}

__device__ __forceinline__ void skinny_ln_prologue(const float* __restrict__ res, const bf16_t* __restrict__ branch,
                                                   float* __restrict__ s_out, const bf16_t* __restrict__ lw,
                                                   const bf16_t* __restrict__ lb, float eps, bf16_t* xs, int M,
                                                   int K) {
  const int KP = K + 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#include "decode_skinny_ln_prologue.h"
}

// the fewest waves along K that cover the np pieces of a row in one pass, then passes:
// f(int_c<KW>, int_c<P>); np <= 512 (callers check K <= ROW_MAX_K)
template <typename F>
void mx_cfg(int np, F&& f) {
  if (np <= 64)
    f(int_c<1>{}, int_c<1>{});
  else if (np <= 128)
    f(int_c<2>{}, int_c<1>{});
  else if (np <= 256)
    f(int_c<4>{}, int_c<1>{});
  else
    f(int_c<4>{}, int_c<2>{});
}

// The piece size of a row of K: f(int_c<PB>).  Half blocks while they fit one wave (K <= 1024),
// whole blocks beyond.  Measured on an MI355X, us per launch of the LayerNorm-prologue kernel,
// weights rotated through 1 GiB so that every launch streams from HBM, medians of three
// alternated runs, PB = 8 / PB = 16 for (N, K): (2304, 768) 3.83 / 4.08; (3072, 768) 3.92 /
// 4.17; (50304, 768) 12.05 / 12.46 (and 8.61 / 12.69 for the plain kernel of the same shape);
// (4096, 1024) 4.02 / 4.24; (3840, 1280) 4.51 / 4.32; (5120, 1280) 5.23 / 4.78; (4800, 1600)
// 5.36 / 4.85; (6400, 1600) 5.84 / 5.49; (50304, 1600) 17.09 / 13.98; (2048, 2048) 4.15 / 4.06;
// (768, 3072) 7.77 / 7.62; (1600, 6400) 13.39 / 12.76.
template <typename F>
void mx_piece(int K, F&& f) {
#ifdef NSA_MX4_PIECE
  f(int_c<NSA_MX4_PIECE>{});
#else
  if (K <= 1024)
    f(int_c<8>{});
  else
    f(int_c<16>{});
#endif
}

// the pieces of block row set n0 into wp (all P * NC weight and scale loads in flight together)
template <int PB, int NC, int P>
__device__ __forceinline__ void mx_load_block(const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ scale,
                                              int n0, int N, int K, const int (&gc)[P], const bool (&live)[P],
                                              MxPiece<PB> (&wp)[P][NC]) {
  using V = typename mx_vec<PB>::type;
  const int KB = K / 2, nb = K / 32;
  V v[P][NC];
  uint8_t e[P][NC];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int64_t n = min(n0 + c, N - 1);
      v[p][c] = *reinterpret_cast<const V*>(Wq + n * KB + PB * gc[p]);
      e[p][c] = scale[n * nb + (PB * gc[p]) / 16];
    }
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      wp[p][c].d[0] = live[p] ? v[p][c].x : 0u;
      wp[p][c].d[1] = live[p] ? v[p][c].y : 0u;
      if constexpr (PB == 16) {
        wp[p][c].d[2] = live[p] ? v[p][c].z : 0u;
        wp[p][c].d[3] = live[p] ? v[p][c].w : 0u;
      }
      wp[p][c].s = mx_scale(e[p][c]);
    }
}

// acc[c] = sum over the lane's pieces of x . w: one packed convert per byte, two fp32 FMAs
template <int PB, int NC, int P>
__device__ __forceinline__ void mx_dot_block(const float (&xr)[P][2 * PB], const MxPiece<PB> (&wp)[P][NC],
                                             float (&acc)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int j = 0; j < PB / 4; ++j) {
        const uint32_t d = wp[p][c].d[j];
        const float s = wp[p][c].s;
        const mx_f32x2 f0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 0);
        const mx_f32x2 f1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 1);
        const mx_f32x2 f2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 2);
        const mx_f32x2 f3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, s, 3);
        acc[c] = fmaf(xr[p][8 * j + 0], f0.x, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 1], f0.y, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 2], f1.x, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 3], f1.y, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 4], f2.x, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 5], f2.y, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 6], f3.x, acc[c]);
        acc[c] = fmaf(xr[p][8 * j + 7], f3.y, acc[c]);
      }
}

// the lane's pieces: gc[p] the piece (clamped into the row), live[p] whether it exists
template <int KW, int P>
__device__ __forceinline__ void mx_pieces(int np, int kw, int lane, int (&gc)[P], bool (&live)[P]) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int g = kw * 64 + lane + p * 64 * KW;
    live[p] = g < np;
    gc[p] = live[p] ? g : np - 1;
  }
}

// the KW wave sets' partial sums of a block of BN columns -> y (256 threads; red[4][NC])
template <int ACT, bool OUTF, int NC, int KW>
__device__ __forceinline__ void mx_row_store(float (&acc)[NC], float (*red)[NC], const bf16_t* __restrict__ bias,
                                             void* __restrict__ y, int nbase, int N) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  constexpr int BN = (4 / KW) * NC;
  int idx;
  const float v = wave_reduce_multi<NC>(acc, lane, idx);
  if ((lane & (64 / NC - 1)) == 0) red[w][idx] = v;
  __syncthreads();
  if (tid < BN) {
    const int g = tid / NC, c = tid % NC;
    const int n = nbase + tid;
    if (n < N) {
      float o = 0.0f;
#pragma unroll
      for (int q = 0; q < KW; ++q) o += red[g * KW + q][c];
      if (bias) o += bf2f(bias[n]);
      if (ACT == 1) o = nsa_gelu(o);
      if constexpr (OUTF)
        reinterpret_cast<float*>(y)[n] = o;
      else
        reinterpret_cast<bf16_t*>(y)[n] = f2bf(o);
    }
  }
}

// y[n] = act(x . W[n] + bias[n]) with the producer of x in the prologue (gemv_row_kernel's
// counterpart).  Each workgroup loops over column blocks cb, cb + gridDim.x, ...; the first
// block's weights are issued before the prologue and the next block's before the reduction;
// x stays in registers across the blocks.
template <int PRO, int ACT, bool OUTF, int PB, int NC, int KW, int P>
__global__ __launch_bounds__(256) void gemv_row_mx4_kernel(const RowPro a, const uint8_t* __restrict__ Wq,
                                                           const uint8_t* __restrict__ scale,
                                                           const bf16_t* __restrict__ bias, void* __restrict__ y,
                                                           int N, int K) {
  extern __shared__ __attribute__((aligned(16))) float hs[];  // [K] input row at hx(k)
  constexpr int KP = 2 * PB, CG = 4 / KW, BN = CG * NC;
  __shared__ float red[4][NC];
  __shared__ float stat[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kw = w % KW, cg = w / KW;
  const int np = K / KP;
  const int nblk = (N + BN - 1) / BN;
  int gc[P];
  bool live[P];
  mx_pieces<KW, P>(np, kw, lane, gc, live);
  int cb = blockIdx.x;
  MxPiece<PB> wp[P][NC];
  mx_load_block<PB, NC, P>(Wq, scale, cb * BN + cg * NC, N, K, gc, live, wp);
  row_prologue<PRO, KP>(a, hs, stat, K);
  __syncthreads();
  float xr[P][KP];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < KP / 4; ++j) {
      const float4 v = reinterpret_cast<const float4*>(hs)[j * np + gc[p]];
      xr[p][4 * j] = v.x;
      xr[p][4 * j + 1] = v.y;
      xr[p][4 * j + 2] = v.z;
      xr[p][4 * j + 3] = v.w;
    }
  for (; cb < nblk; cb += gridDim.x) {
    float acc[NC];
    mx_dot_block<PB, NC, P>(xr, wp, acc);
    const int nb = cb + gridDim.x;
    if (nb < nblk) mx_load_block<PB, NC, P>(Wq, scale, nb * BN + cg * NC, N, K, gc, live, wp);  // during the reduction
    mx_row_store<ACT, OUTF, NC, KW>(acc, red, bias, y, cb * BN, N);
    __syncthreads();  // red[] is rewritten by the next block
  }
  if constexpr (PRO == PRO_LN)
    if (a.pos_inc && blockIdx.x == 0 && tid == 0) *a.pos_inc += 1;
}

// The same for a row x that is already in memory (nsa_gemv_mx4): one block per workgroup, x
// read with the weights.
template <int ACT, bool OUTF, int PB, int NC, int KW, int P>
__global__ __launch_bounds__(256) void gemv1_mx4_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ Wq,
                                                        const uint8_t* __restrict__ scale,
                                                        const bf16_t* __restrict__ bias, void* __restrict__ y, int N,
                                                        int K) {
  constexpr int KP = 2 * PB, CG = 4 / KW, BN = CG * NC;
  __shared__ float red[4][NC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kw = w % KW, cg = w / KW;
  int gc[P];
  bool live[P];
  mx_pieces<KW, P>(K / KP, kw, lane, gc, live);
  MxPiece<PB> wp[P][NC];
  mx_load_block<PB, NC, P>(Wq, scale, blockIdx.x * BN + cg * NC, N, K, gc, live, wp);
  float xr[P][KP];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < KP / 8; ++j) {
      float f[8];
      load8(x + KP * gc[p] + 8 * j, f);
#pragma unroll
      for (int i = 0; i < 8; ++i) xr[p][8 * j + i] = f[i];
    }
  float acc[NC];
  mx_dot_block<PB, NC, P>(xr, wp, acc);
  mx_row_store<ACT, OUTF, NC, KW>(acc, red, bias, y, blockIdx.x * BN, N);
}

template <int PRO>
hipError_t launch_gemv_row_mx4(const RowPro& a, const void* Wq, const void* scale, const void* bias, void* y, int N,
                               int K, int act, int out_f32, hipStream_t s) {
  const size_t lds = row_lds_bytes<PRO>(a, K);
  const uint8_t* w = (const uint8_t*)Wq;
  const uint8_t* sc = (const uint8_t*)scale;
  const bf16_t* b = (const bf16_t*)bias;
  mx_piece(K, [&](auto PB) {
    constexpr int pb = decltype(PB)::value;
    mx_cfg(K / (2 * pb), [&](auto KW, auto P) {
      // columns per wave set as the int8 kernel: 2 where one wave covers K, else 4
      constexpr int kw = decltype(KW)::value, nc = kw == 1 ? 2 : 4;
      constexpr int bn = (4 / kw) * nc;
      const int nblk = (N + bn - 1) / bn;
      const unsigned grid = (unsigned)std::min(nblk, gemv_row_grid());
      epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
        gemv_row_mx4_kernel<PRO, decltype(ACT)::value, decltype(OUTF)::value, pb, nc, kw, decltype(P)::value>
            <<<grid, 256, lds, s>>>(a, w, sc, b, y, N, K);
      });
    });
  });
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Skinny GEMM (2..16 decode rows on the matrix cores), MXFP4 weights.  As in
// skinny_gemm_kernel the weight is the A operand of v_mfma_f32_16x16x32_bf16 (lane l: row
// n0 + (l & 15)) and X^T the B operand (lane l: batch row l & 15).  A lane's 16-byte weight
// load is one MX block, 32 consecutive k of its row, the k of a 128-wide unit u being
//   128 u + 32 (l >> 4) + 8 h + i,   h = 0 .. 3 (the MFMA), i = 0 .. 7 (the fragment element),
// so one load and one scale byte feed four MFMAs, each fragment formed by four packed
// converts (dword h of the load), and the X fragment of MFMA h is the 16 bytes of the batch
// row at the same k: the two fragments permute k alike, which a dot product does not see.
// Wave w takes units w, w + 4, ...  K % 128 != 0 (1600: 12.5 units) leaves a last unit in
// which the upper lane groups have no block: liveness is per lane group (block 4 u + (l >> 4)
// < K / 32), a dead group reads the row's last block and X at the same clamped k against a
// zero weight fragment, branch-free, so every load of a round issues before any wait.  Any N:
// weight rows past the end read row N - 1 and their outputs are not stored.
// ---------------------------------------------------------------------------
struct MxBlock {
  uint4 q;    // 32 nibbles
  uint8_t e;  // the scale byte
};

// dword d (8 nibbles, k order) times the scale -> one MFMA fragment
__device__ __forceinline__ bf16x8 mx_frag(uint32_t d, float s) {
  const mx_bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0);
  const mx_bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
  const mx_bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2);
  const mx_bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
  const uint4 u = {__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1),
                   __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3)};
  return __builtin_bit_cast(bf16x8, u);
}

// the four MFMAs of one block against the X fragments b[0 .. 3]
__device__ __forceinline__ f32x4 mx_mfma4(const MxBlock& a, const uint4 (&b)[4], f32x4 acc) {
  const float s = mx_scale(a.e);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx_frag(a.q.x, s), __builtin_bit_cast(bf16x8, b[0]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx_frag(a.q.y, s), __builtin_bit_cast(bf16x8, b[1]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx_frag(a.q.z, s), __builtin_bit_cast(bf16x8, b[2]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx_frag(a.q.w, s), __builtin_bit_cast(bf16x8, b[3]), acc, 0, 0, 0);
  return acc;
}

// the lane's block of unit uu: block index clamped into the row, its weights zero when it is not there
__device__ __forceinline__ int mx_block_index(int uu, int g, int nb) { return min(4 * uu + g, nb - 1); }

template <int UN>
__device__ __forceinline__ void mx_load_units(const uint8_t* __restrict__ wrow, const uint8_t* __restrict__ srow,
                                              int u0, int g, int nb, MxBlock (&dst)[UN]) {
#pragma unroll
  for (int j = 0; j < UN; ++j) {
    const int bi = mx_block_index(u0 + 4 * j, g, nb);
    dst[j].q = *reinterpret_cast<const uint4*>(wrow + 16 * bi);
    dst[j].e = srow[bi];
    if (4 * (u0 + 4 * j) + g >= nb) dst[j].q = uint4{0u, 0u, 0u, 0u};
  }
}

template <int ACT, bool OUTF>
__device__ __forceinline__ void skinny_mx4_epilogue(const f32x4& acc, float (*red)[4][64],
                                                    const bf16_t* __restrict__ bias, void* __restrict__ yv, int M,
                                                    int N, int n0) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // C layout: lane l holds column m = l & 15 of the 16-row group, rows n = 4 (l >> 4) + i
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  const int n = tid & 15, m = tid >> 4;  // n fastest: coalesced stores
  if (m < M && n0 + n < N) {
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

// UN 128-wide units per wave in flight
template <int ACT, bool OUTF, int UN>
__global__ __launch_bounds__(256) void skinny_gemm_mx4_kernel(const bf16_t* __restrict__ x,
                                                              const uint8_t* __restrict__ Wq,
                                                              const uint8_t* __restrict__ scale,
                                                              const bf16_t* __restrict__ bias, void* __restrict__ yv,
                                                              int M, int N, int K) {
  __shared__ float red[4][4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int g = lane >> 4, c = lane & 15;
  const int nb = K / 32, U = (nb + 3) / 4;
  const int64_t n = min(n0 + c, N - 1);
  const uint8_t* wrow = Wq + n * (K / 2);
  const uint8_t* srow = scale + n * nb;
  const bf16_t* xrow = x + (int64_t)min(c, M - 1) * K;
  f32x4 acc = f32x4{};
  for (int u0 = w; u0 < U; u0 += 4 * UN) {
    MxBlock a[UN];
    uint4 b[UN][4];
    mx_load_units<UN>(wrow, srow, u0, g, nb, a);
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const bf16_t* xp = xrow + 32 * mx_block_index(u0 + 4 * j, g, nb);
#pragma unroll
      for (int h = 0; h < 4; ++h) b[j][h] = *reinterpret_cast<const uint4*>(xp + 8 * h);
    }
#pragma unroll
    for (int j = 0; j < UN; ++j) acc = mx_mfma4(a[j], b[j], acc);
  }
  skinny_mx4_epilogue<ACT, OUTF>(acc, red, bias, yv, M, N, n0);
}

// The same with the residual add + LayerNorm in the prologue (skinny_ln_gemm_kernel's
// counterpart): the first round of weight loads is issued before the prologue and each
// round prefetches the next, so the weight stream overlaps the LayerNorm.
template <int ACT, bool OUTF>
__global__ __launch_bounds__(256) void skinny_ln_gemm_mx4_kernel(const float* __restrict__ res,
                                                                 const bf16_t* __restrict__ branch,
                                                                 float* __restrict__ s_out,
                                                                 const bf16_t* __restrict__ lw,
                                                                 const bf16_t* __restrict__ lb, float eps,
                                                                 const uint8_t* __restrict__ Wq,
                                                                 const uint8_t* __restrict__ scale,
                                                                 const bf16_t* __restrict__ bias,
                                                                 void* __restrict__ yv, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [16][K + 8]
  __shared__ float red[4][4][64];
  const int KP = K + 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int g = lane >> 4, c = lane & 15;
  const int nb = K / 32, U = (nb + 3) / 4;
  const int64_t n = min(n0 + c, N - 1);
  const uint8_t* wrow = Wq + n * (K / 2);
  const uint8_t* srow = scale + n * nb;
  constexpr int UN = 2;  // 1024 k over the workgroup per round
  MxBlock a[UN];
  mx_load_units<UN>(wrow, srow, w, g, nb, a);
  skinny_ln_prologue(res, branch, s_out, lw, lb, eps, xs, M, K);
  __syncthreads();
  f32x4 acc = f32x4{};
  for (int u0 = w; u0 < U; u0 += 4 * UN) {
    uint4 b[UN][4];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const bf16_t* xp = xs + c * KP + 32 * mx_block_index(u0 + 4 * j, g, nb);
#pragma unroll
      for (int h = 0; h < 4; ++h) b[j][h] = *reinterpret_cast<const uint4*>(xp + 8 * h);
    }
    MxBlock an[UN];
    const bool more = u0 + 4 * UN < U;  // wave-uniform
    if (more) mx_load_units<UN>(wrow, srow, u0 + 4 * UN, g, nb, an);
#pragma unroll
    for (int j = 0; j < UN; ++j) acc = mx_mfma4(a[j], b[j], acc);
    if (more) {
#pragma unroll
      for (int j = 0; j < UN; ++j) a[j] = an[j];
    }
  }
  skinny_mx4_epilogue<ACT, OUTF>(acc, red, bias, yv, M, N, n0);
}

bool mx_k_ok(int K) { return K >= MX4_K && K % MX4_K == 0; }

}  // namespace

// y[1, N] = act(x[1, K] W[N, K]^T + b): one row, any N, K % 32 == 0, K <= 8192; Wq the nibble
// matrix [N, K / 2], scale the E8M0 bytes [N, K / 32], x / b bf16; act: 0 none, 1 exact-erf
// GELU; out_f32: y is fp32.  More rows belong to nsa_skinny_gemm_mx4.
NSA_API hipError_t nsa_gemv_mx4(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int rows,
                                int N, int K, int act, int out_f32, hipStream_t s) {
  if (rows != 1 || !mx_k_ok(K) || K > ROW_MAX_K || N < 1 || (act && out_f32)) return hipErrorInvalidValue;
  mx_piece(K, [&](auto PB) {
    constexpr int pb = decltype(PB)::value;
    mx_cfg(K / (2 * pb), [&](auto KW, auto P) {
      // 2 columns per wave set: narrow outputs need many small workgroups (as nsa_gemv_q8)
      constexpr int bn = (4 / decltype(KW)::value) * 2;
      const unsigned g1 = (unsigned)((N + bn - 1) / bn);
      epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
        gemv1_mx4_kernel<decltype(ACT)::value, decltype(OUTF)::value, pb, 2, decltype(KW)::value, decltype(P)::value>
            <<<g1, 256, 0, s>>>((const bf16_t*)x, (const uint8_t*)Wq, (const uint8_t*)scale, (const bf16_t*)bias, y,
                                N, K);
      });
    });
  });
  return hipGetLastError();
}

// nsa_gemv_ln with MXFP4 weights: K % 32 == 0, K <= 8192, any N
NSA_API hipError_t nsa_gemv_ln_mx4(const void* res, const void* branch, void* res_out, const void* lw, const void* lb,
                                   const void* Wq, const void* scale, const void* bias, void* y, int N, int K,
                                   float eps, int act, int out_f32, void* pos_inc, hipStream_t s) {
  if (K < MX4_K || !row_ln_ok(res, branch, res_out, N, K, MX4_K, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row_mx4<PRO_LN>(row_ln(res, branch, res_out, lw, lb, eps, pos_inc), Wq, scale, bias, y, N, K,
                                     act, out_f32, s);
}

// nsa_gemv_emb_ln with an MXFP4 linear (the wte / wpe rows stay bf16)
NSA_API hipError_t nsa_gemv_emb_ln_mx4(const void* tok, const void* pos, const void* wte, const void* wpe,
                                       void* res_out, const void* lw, const void* lb, const void* Wq,
                                       const void* scale, const void* bias, void* y, int N, int K, float eps, int act,
                                       int out_f32, hipStream_t s) {
  if (K < MX4_K || !row_emb_ln_ok(res_out, N, K, MX4_K, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row_mx4<PRO_EMB_LN>(row_emb_ln(tok, pos, wte, wpe, res_out, lw, lb, eps), Wq, scale, bias, y, N,
                                         K, act, out_f32, s);
}

// nsa_gemv_attn with MXFP4 weights (K = H * 64: a multiple of 32)
NSA_API hipError_t nsa_gemv_attn_mx4(const void* ws, int n_split, const void* Wq, const void* scale, const void* bias,
                                     void* y, int N, int K, int act, int out_f32, hipStream_t s) {
  if (K < DA_D || !row_attn_ok(n_split, N, K, act, out_f32)) return hipErrorInvalidValue;
  return launch_gemv_row_mx4<PRO_ATTN>(row_attn(ws, n_split), Wq, scale, bias, y, N, K, act, out_f32, s);
}

// y[rows, N] = act(x[rows, K] W[N, K]^T + b) for 1 <= rows <= 16, any N, K % 32 == 0
NSA_API hipError_t nsa_skinny_gemm_mx4(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                       int rows, int N, int K, int act, int out_f32, hipStream_t s) {
  if (rows < 1 || rows > SKINNY_GROUP_ROWS || !mx_k_ok(K) || N < 1 || (act && out_f32)) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)((N + 15) / 16);
  auto launch = [&](auto UN) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      skinny_gemm_mx4_kernel<decltype(ACT)::value, decltype(OUTF)::value, decltype(UN)::value><<<grid, 256, 0, s>>>(
          (const bf16_t*)x, (const uint8_t*)Wq, (const uint8_t*)scale, (const bf16_t*)bias, y, rows, N, K);
    });
  };
  // 2 units (1024 k over the workgroup) in flight per round up to K = 1024, 4 beyond: the
  // int8 kernel's k per round
  if (K <= 1024)
    launch(int_c<2>{});
  else
    launch(int_c<4>{});
  return hipGetLastError();
}

// nsa_skinny_ln_gemm with MXFP4 weights: any N, K % 32 == 0, K <= 1920
NSA_API hipError_t nsa_skinny_ln_gemm_mx4(const void* res, const void* branch, void* s_out, const void* lw,
                                          const void* lb, float eps, const void* Wq, const void* scale,
                                          const void* bias, void* y, int rows, int N, int K, int act, int out_f32,
                                          hipStream_t s) {
  if (rows < 1 || rows > SKINNY_GROUP_ROWS || !mx_k_ok(K) || K > SKINNY_LN_MAX_K || N < 1 || (act && out_f32) ||
      (branch && !s_out))
    return hipErrorInvalidValue;
  if (!branch) s_out = nullptr;  // s is res itself: nothing to write (as the single-row kernel)
  const unsigned grid = (unsigned)((N + 15) / 16);
  const size_t lds = (size_t)16 * (K + 8) * sizeof(bf16_t);
  epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
    skinny_ln_gemm_mx4_kernel<decltype(ACT)::value, decltype(OUTF)::value><<<grid, 256, lds, s>>>(
        (const float*)res, (const bf16_t*)branch, (float*)s_out, (const bf16_t*)lw, (const bf16_t*)lb, eps,
        (const uint8_t*)Wq, (const uint8_t*)scale, (const bf16_t*)bias, y, rows, N, K);
  });
  return hipGetLastError();
}
