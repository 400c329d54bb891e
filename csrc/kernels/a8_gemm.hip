// W8A8 prompt GEMM on the integer matrix path: y[M, N] (bf16) = act(f32(sum_k xq[m, k] Wq[n, k]) sx[m] sw[n] + bias[n]),
// xq int8 [M, K] with one fp32 scale per row (nsa_quantize_act_rows: dynamic per-token quantization of the bf16
// activations), Wq int8 [N, K] with one fp32 scale per row (ops.QuantWeight).  nsa_quant_gemm_q8 turns every int8
// weight into bf16 in registers and feeds v_mfma_f32_32x32x16_bf16, so it cannot beat the bf16 GEMM; this one
// feeds both int8 operands unconverted to v_mfma_i32_32x32x32_i8 (twice the k per instruction, no convert) and
// accumulates in int32: the sum is exact, so the output is pinned bit for bit by the epilogue's order alone.
// Any M >= 1 and N >= 1, K % 64 == 0, K <= 131072 (127 * 127 * K stays inside int32); no split of K, no workspace
// and no atomics: a launch is deterministic and can be captured.
//
// Workgroup and tile.  256 threads own A8_TILE_M = 128 rows x A8_TILE_N = 128 output columns (quant_gemm.hip's
// tile); the grid is (column tiles) x (row tiles).  Wave w owns the 32 columns n0 = 128 ct + 32 w .. + 31 and all
// four 32-row blocks: four 32x32 int32 accumulator blocks (64 registers).  Every weight element of the tile is
// fetched by exactly one wave.  NSA_A8_ROW_BLOCKS (compile-time override, for measuring only) makes the tile
// 32 x that many rows; 8 (a 256-row tile) halves the weight traffic per output at twice the LDS image.  Measured on
// an MI355X (GPT-2 1.5B block shapes, profiles/a8_op_bench.jsonl against a8_op_bench_rows256.jsonl): the 256-row
// tile is 5 - 18 % faster at 8,192 rows and at 1,024 rows x N >= 4800, and 1.5 - 1.6x slower at 1,024 rows x
// N = 1600 (52 tiles for 256 CUs), the shape of two of the four linears of a short prompt; 128 rows stays, and
// choosing the tile by the tile count at launch is the follow-up.
//
// The fragment plan.  The 32x32x32 int8 MFMA takes 16 consecutive k (one 16-byte register quad) of row l & 31
// from lane l, lane group h = l >> 5 supplying k = 16 h .. 16 h + 15 of the instruction's 32.  A lane's weight
// load is therefore one MFMA operand: piece 2 j + h (16 k) of row n0 + (l & 31) for the j-th MFMA step of a
// chunk, global -> registers in one 16-byte load, never through LDS and never converted.  The X operand of the
// same MFMA is the 16 bytes of row 32 t + (l & 31) at the same k from LDS: both operands take the same k from the
// same lane group, so whatever order the instruction gives the k inside a lane is invisible to the dot product
// (the argument of quant_gemm.hip; the exact tests confirm the lane / row / lane-group mapping).
//
// X through LDS.  The tile's X goes once through LDS as int8 in chunks of A8_CHUNK = 256 k, double-buffered and
// shared by the four waves: the 16-byte global loads of chunk i + 1 (X and weights) are issued before the MFMAs
// of chunk i and land in the other buffer behind one barrier per chunk (register staging, quant_gemm.hip's
// baseline; LDS-DMA staging was not tried).  A chunk is 8 MFMA steps: 8 weight loads of 16 bytes in flight per
// lane, twice nsa_quant_gemm_q8's, which is what the registers freed by the missing convert are spent on.
// The image is [128][256 + 16] bytes per buffer: 2 x 128 x 272 = 69632 bytes (139264 with 8 row blocks).  The row
// stride is 272 / 4 = 68 dwords = 4 mod 64.  The ds_read_b128 of lane (c, h) for step j starts at dword
// 68 c + 4 h + 8 j, bank 4 c + 4 h + const (mod 64): the 16 lanes of one pass (c .. c + 15 of one lane group)
// start 4 banks apart and cover the 64 banks once each; a pass never mixes lane groups (an unpadded row, stride
// 0 mod 64, would put all 16 lanes on 4 banks).  Staging writes consecutive 16-byte pieces from consecutive
// lanes.  The four X fragments of step s + 1 are read before the four MFMAs of step s.
//
// Epilogue.  r = (float)acc; r *= sx[m]; r *= sw[n]; r += bias[n]; GELU; bf16 round-to-nearest-even: every
// operation rounded to fp32 on its own, no contraction into a fused multiply-add (a8_scale_bias).  This order is
// the op's definition (ops.a8_linear's fallback states it in torch).
//
// Edges.  Rows past M are clamped on load (row M - 1 again) and not stored.  Weight rows past N re-read row
// N - 1 and are not stored; a wave whose 32 columns all lie past N only helps stage X.  K is whole 64s but not
// whole chunks: piece p is live while p < K / 16; a dead weight piece re-reads the row's last piece and is zeroed,
// branch-free, and X past K is staged as zeros, so every MFMA of a chunk runs.  y is stored 4 columns (8 bytes)
// at a time where N % 4 == 0 and y is 8-byte aligned, element by element otherwise.
//
// Tile order.  quant_gemm.hip's: workgroup ids are remapped so that an XCD gets consecutive tiles, and
// consecutive tiles walk the row tiles of one column tile first, so workgroups resident together on an XCD share
// a column tile's weights in L2.
//
// Registers (compiler summary, gfx950): 220 VGPRs + 64 AGPRs, no scratch, 69632 bytes of LDS: one workgroup per
// CU, one wave per SIMD (284 of a SIMD's 512 registers leave no room for a second wave); with 8 row blocks 256 + 181
// and 139264 bytes.  The quantizer: 43 / 44 VGPRs, 8 waves per SIMD.
//
// nsa_quantize_act_rows.  bf16 x[M, K] -> int8 q[M, K], fp32 sx[M] by the int8 KV cache's rule over a whole row
// (kv8_scale / kv8_quant of decode_rows.h: ops.quantize_cache_rows bit for bit).  A row is shared by T threads:
// a wave (K <= 2048, four rows per workgroup, no barrier) or the workgroup (T = 256).  A thread owns units of 16
// elements, t, t + T, ..: two 16-byte loads in, one 16-byte store out.  Its first QA_UNITS = 2 units stay in
// registers between the absmax pass and the quantize pass, so a row of up to 32 T elements (8192 at T = 256:
// every K the models use) is read from HBM once; units past that are read again in the second pass.
#include "decode_rows.h"

#ifndef NSA_A8_ROW_BLOCKS
#define NSA_A8_ROW_BLOCKS 4
#endif

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int A8_RB = NSA_A8_ROW_BLOCKS;  // 32-row blocks of a workgroup's tile
constexpr int A8_TILE_M = 32 * A8_RB;
constexpr int A8_TILE_N = 128;   // its output columns: one wave per 32
constexpr int A8_CHUNK = 256;    // k per LDS chunk of X
constexpr int A8_KP = A8_CHUNK + 16;  // padded row of the LDS image, bytes
constexpr int A8_MAX_K = 131072;  // 127 * 127 * K < 2^31
constexpr int QA_UNITS = 2;      // 16-element units a quantizer thread keeps in registers
static_assert(A8_RB == 4 || A8_RB == 8, "a tile is 128 or 256 rows: its chunk is shared out among 256 threads");

// acc sx sw + b as three separately rounded fp32 operations (hipcc contracts by default: switched off here)
__device__ __forceinline__ float a8_scale_bias(int acc, float sx, float sw, float b) {
#pragma clang fp contract(off)
  float r = (float)acc;
  r = r * sx;
  r = r * sw;
  return r + b;
}

template <int ACT>
__global__ __launch_bounds__(256) void a8_gemm_kernel(const int8_t* __restrict__ xq, const float* __restrict__ sx,
                                                      const int8_t* __restrict__ Wq, const float* __restrict__ sw,
                                                      const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int M,
                                                      int N, int K) {
  constexpr int RB = A8_RB, KP = A8_KP;
  constexpr int CP = A8_CHUNK / 16, UN = CP / 2;  // pieces per chunk; MFMA steps = weight loads in flight per lane
  constexpr int XC = CP, XR = 256 / XC;           // 16-byte pieces of a chunk row; rows the threads stage per pass
  constexpr int XV = A8_TILE_M / XR;              // 16-byte pieces of a chunk per thread
  extern __shared__ __attribute__((aligned(16))) int8_t xs[];  // [2][A8_TILE_M][KP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  // tile order: XCD v % 8 gets consecutive tiles u, and u walks the row tiles of one column tile first
  const int CT = gridDim.x, RT = gridDim.y, total = CT * RT;
  const int v = blockIdx.x + CT * blockIdx.y;
  const int xcd = v % 8, tq = total / 8, tr = total % 8;
  const int u = (xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq) + v / 8;
  const int m0 = (u % RT) * A8_TILE_M, n0 = (u / RT) * A8_TILE_N + 32 * w;
  const bool live = n0 < N;  // wave-uniform: a wave past N only helps staging X
  const int PT = K / 16;     // pieces of a row
  const int8_t* wrow = Wq + (int64_t)min(n0 + c, N - 1) * K;
  // staging: piece e = tid + 256 i of a chunk is tile row e / XC, byte offset 16 (e % XC)
  const int xr = tid / XC, xc = tid % XC;
  const int8_t* xcol = xq + (int64_t)m0 * K + 16 * xc;
  const int mlast = M - 1 - m0;  // the tile's last live row

  // pieces past PT: the weight piece is zero (the row's last piece re-read, branch-free) and X's are zeros
  auto load_a = [&](int p0, uint4 (&dst)[UN]) {
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int p = p0 + 2 * j + h;
      dst[j] = *reinterpret_cast<const uint4*>(wrow + 16 * (p < PT ? p : PT - 1));
      if (p >= PT) dst[j] = uint4{0u, 0u, 0u, 0u};
    }
  };
  auto load_x = [&](int p0, uint4 (&dst)[XV]) {
    const bool in = p0 + xc < PT;
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      dst[i] = uint4{0u, 0u, 0u, 0u};
      if (in) dst[i] = *reinterpret_cast<const uint4*>(xcol + (int64_t)min(xr + XR * i, mlast) * K + 16 * p0);
    }
  };
  auto store_x = [&](int buf, const uint4 (&src)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; ++i)
      *reinterpret_cast<uint4*>(xs + buf * A8_TILE_M * KP + (xr + XR * i) * KP + 16 * xc) = src[i];
  };

  i32x16 acc[RB];
#pragma unroll
  for (int t = 0; t < RB; ++t) acc[t] = i32x16{};
  uint4 a[UN], xv[XV];
  if (live) load_a(0, a);
  load_x(0, xv);
  store_x(0, xv);
  __syncthreads();
  int buf = 0;
  for (int p0 = 0; p0 < PT; p0 += CP, buf ^= 1) {
    const bool more = p0 + CP < PT;  // workgroup-uniform
    uint4 an[UN];
    if (more) {
      if (live) load_a(p0 + CP, an);
      load_x(p0 + CP, xv);
    }
    if (live) {
      const int8_t* xb = xs + buf * A8_TILE_M * KP + c * KP + 16 * h;
      // step s: the lane's piece 2 s + h on every row block.  The X fragments of step s + 1 are read before the
      // MFMAs of step s; the scheduling barriers keep the compiler from sinking them back to their use.
      auto frags = [&](int s, uint4 (&dst)[RB]) {
#pragma unroll
        for (int t = 0; t < RB; ++t) dst[t] = *reinterpret_cast<const uint4*>(xb + 32 * t * KP + 32 * s);
      };
      uint4 b[RB], bn[RB];
      frags(0, b);
#pragma unroll
      for (int s = 0; s < UN; ++s) {
        if (s + 1 < UN) frags(s + 1, bn);
        __builtin_amdgcn_sched_barrier(0);
        const i32x4 af = __builtin_bit_cast(i32x4, a[s]);
#pragma unroll
        for (int t = 0; t < RB; ++t)
          acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, __builtin_bit_cast(i32x4, b[t]), acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RB; ++t) b[t] = bn[t];
      }
    }
    if (more) {
      // the other buffer was last read before the barrier that ended the previous chunk
      store_x(buf ^ 1, xv);
      if (live) {
#pragma unroll
        for (int j = 0; j < UN; ++j) a[j] = an[j];
      }
    }
    __syncthreads();
  }
  if (!live) return;

  // C layout: lane l holds row m0 + 32 t + (l & 31), output columns n0 + 8 q + 4 (l >> 5) + i in
  // accumulator element 4 q + i
  const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0;
#pragma unroll
  for (int t = 0; t < RB; ++t) {
    const int m = m0 + 32 * t + c;
    if (m >= M) continue;
    const float sm = sx[m];
    bf16_t* yrow = y + (int64_t)m * N;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 8 * q + 4 * h;
      bf16_t o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ni = min(n + i, N - 1);  // past N: computed on column N - 1, not stored
        float r = a8_scale_bias(acc[t][4 * q + i], sm, sw[ni], bias ? bf2f(bias[ni]) : 0.0f);
        if constexpr (ACT == 1) r = nsa_gelu(r);
        o[i] = f2bf(r);
      }
      if (vec) {
        if (n < N)  // whole groups of 4
          *reinterpret_cast<uint2*>(yrow + n) =
              uint2{(uint32_t)o[0] | (uint32_t)o[1] << 16, (uint32_t)o[2] | (uint32_t)o[3] << 16};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < N) yrow[n + i] = o[i];
      }
    }
  }
}

template <int ACT>
hipError_t a8_launch(const void* xq, const void* sx, const void* Wq, const void* sw, const void* bias, void* y, int M,
                     int N, int K, hipStream_t s) {
  constexpr int lds = 2 * A8_TILE_M * A8_KP;
  static bool attr = [] {  // dynamic LDS above 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&a8_gemm_kernel<ACT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  }();
  if (!attr) return hipErrorInvalidValue;
  const dim3 grid((N + A8_TILE_N - 1) / A8_TILE_N, (M + A8_TILE_M - 1) / A8_TILE_M);
  a8_gemm_kernel<ACT><<<grid, 256, lds, s>>>((const int8_t*)xq, (const float*)sx, (const int8_t*)Wq, (const float*)sw,
                                             (const bf16_t*)bias, (bf16_t*)y, M, N, K);
  return hipGetLastError();
}

// One row per T threads: absmax, then q = kv8_quant(x, kv8_scale(absmax)); unit u (16 elements) of the row belongs
// to thread u % T, its first QA_UNITS units staying in registers between the two passes
template <int T>
__global__ __launch_bounds__(256) void quantize_act_rows_kernel(const bf16_t* __restrict__ x, int8_t* __restrict__ q,
                                                                float* __restrict__ sx, int M, int K) {
  constexpr int ROWS = 256 / T;
  __shared__ float wmax[4];
  const int tid = threadIdx.x, t = tid % T;
  const int64_t row = (int64_t)blockIdx.x * ROWS + tid / T;
  if (T == 64 && row >= M) return;  // wave-uniform, and the wave form has no barrier
  const int U = K / 16;
  const bf16_t* xrow = x + row * K;
  int8_t* qrow = q + row * K;
  auto load = [&](int u, uint4 (&d)[2]) {
    d[0] = *reinterpret_cast<const uint4*>(xrow + 16 * u);
    d[1] = *reinterpret_cast<const uint4*>(xrow + 16 * u + 8);
  };
  auto unit_max = [&](const uint4 (&d)[2], float am) {
    const uint32_t dw[8] = {d[0].x, d[0].y, d[0].z, d[0].w, d[1].x, d[1].y, d[1].z, d[1].w};
#pragma unroll
    for (int j = 0; j < 8; ++j)
      am = fmaxf(am, fmaxf(fabsf(__uint_as_float(dw[j] << 16)), fabsf(__uint_as_float(dw[j] & 0xffff0000u))));
    return am;
  };
  auto store = [&](int u, const uint4 (&d)[2], float sc) {
    const uint32_t dw[8] = {d[0].x, d[0].y, d[0].z, d[0].w, d[1].x, d[1].y, d[1].z, d[1].w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = kv8_pack4(kv8_quant(__uint_as_float(dw[2 * j] << 16), sc),
                       kv8_quant(__uint_as_float(dw[2 * j] & 0xffff0000u), sc),
                       kv8_quant(__uint_as_float(dw[2 * j + 1] << 16), sc),
                       kv8_quant(__uint_as_float(dw[2 * j + 1] & 0xffff0000u), sc));
    *reinterpret_cast<uint4*>(qrow + 16 * u) = uint4{o[0], o[1], o[2], o[3]};
  };

  uint4 held[QA_UNITS][2];
  float am = 0.0f;
#pragma unroll
  for (int i = 0; i < QA_UNITS; ++i) {
    if (t + T * i < U) {
      load(t + T * i, held[i]);
      am = unit_max(held[i], am);
    }
  }
  for (int u = t + T * QA_UNITS; u < U; u += T) {  // past the register-resident bound: read again below
    uint4 d[2];
    load(u, d);
    am = unit_max(d, am);
  }
  am = wave_max(am);
  if (T == 256) {
    if ((tid & 63) == 0) wmax[tid >> 6] = am;
    __syncthreads();
    am = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  }
  const float sc = kv8_scale(am);
  if (t == 0) sx[row] = sc;
#pragma unroll
  for (int i = 0; i < QA_UNITS; ++i)
    if (t + T * i < U) store(t + T * i, held[i], sc);
  for (int u = t + T * QA_UNITS; u < U; u += T) {
    uint4 d[2];
    load(u, d);
    store(u, d, sc);
  }
}

}  // namespace

// k per LDS chunk of X (ops/functional.py mirrors it: the tests take their K edges from it)
NSA_API int nsa_a8_gemm_chunk() { return A8_CHUNK; }
// the widest row nsa_quantize_act_rows reads once (mirrored as well)
NSA_API int nsa_quantize_act_rows_resident() { return 256 * 16 * QA_UNITS; }

// bf16 x [M, K] -> int8 q [M, K] and fp32 sx [M]: sx = absmax / 127 (1 for an all-zero row), q =
// clamp(rint(x / sx), -127, 127), ops.quantize_cache_rows over the whole row bit for bit.  Any M >= 1,
// K % 16 == 0; anything else is refused with hipErrorInvalidValue and nothing is launched.
NSA_API hipError_t nsa_quantize_act_rows(const void* x, void* q, void* sx, int M, int K, hipStream_t s) {
  if (M < 1 || K < 16 || K % 16 != 0 || !x || !q || !sx) return hipErrorInvalidValue;
  if (K <= 64 * 16 * QA_UNITS)
    quantize_act_rows_kernel<64><<<(unsigned)((M + 3) / 4), 256, 0, s>>>((const bf16_t*)x, (int8_t*)q, (float*)sx, M, K);
  else
    quantize_act_rows_kernel<256><<<(unsigned)M, 256, 0, s>>>((const bf16_t*)x, (int8_t*)q, (float*)sx, M, K);
  return hipGetLastError();
}

// y[M, N] (bf16) = act(f32(xq[M, K] Wq[N, K]^T) sx[m] sw[n] + b): int8 rows xq with their fp32 scales sx [M]
// (nsa_quantize_act_rows), int8 weights Wq with one fp32 scale per output column, sw [N]; any M >= 1 and N >= 1,
// K % 64 == 0 and K <= 131072; bias may be NULL, act 1: exact-erf GELU.  Rows are read in 16-byte pieces (16-byte
// aligned, as every allocation is).  Anything else is refused with hipErrorInvalidValue and nothing is launched.
NSA_API hipError_t nsa_a8_gemm(const void* xq, const void* sx, const void* Wq, const void* sw, const void* bias,
                               void* y, int M, int N, int K, int act, hipStream_t s) {
  if (M < 1 || (M + A8_TILE_M - 1) / A8_TILE_M > 65535 || N < 1 || K < 64 || K % 64 != 0 || K > A8_MAX_K || !xq ||
      !sx || !Wq || !sw || !y || act < 0 || act > 1)
    return hipErrorInvalidValue;
  return act ? a8_launch<1>(xq, sx, Wq, sw, bias, y, M, N, K, s) : a8_launch<0>(xq, sx, Wq, sw, bias, y, M, N, K, s);
}
