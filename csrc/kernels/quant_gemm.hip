// GEMM on quantized weights for any number of rows: y[M, N] (bf16) = act(x[M, K] (bf16) dequant(W)[N, K]^T + bias),
// W int8 with one fp32 scale per row (nsa_quant_gemm_q8: ops.QuantWeight) or MXFP4 nibbles with one E8M0 byte
// per block of 32 (nsa_quant_gemm_mx4: ops.MxWeight).  The decode kernels stop at 64 rows; this one serves the
// prompt passes of a quantized decoder, so that no bf16 copy of the block linears has to exist.  Any M >= 1
// and N >= 1, K % 64 == 0 (int8) / K % 32 == 0 (MXFP4); no split of K, no workspace and no atomics: every
// output element is one workgroup's sum in one fixed order, so a launch is deterministic and can be captured.
//
// Workgroup and tile.  256 threads own QG_TILE_M = 128 rows x QG_TILE_N = 128 output columns; the grid is
// (column tiles) x (row tiles).  Wave w owns the 32 columns n0 = 128 ct + 32 w .. + 31 and all 128 rows: four
// 32x32 fp32 accumulator blocks (64 registers) on v_mfma_f32_32x32x16_bf16, the plan of decode_tall.hip.
// Every weight element of the tile is fetched and dequantized by exactly one wave.
//
// The fragment plan.  Weights go global -> registers in 16-byte loads and are converted in registers; none
// passes through LDS.  A lane's load is a piece of P consecutive k of its row n0 + (l & 31):
//   mx4  P = 32: one MX block, with its E8M0 scale byte; it feeds NF = 4 MFMAs, the A fragment of MFMA f
//        being dword f through mx_frag (v_cvt_scalef32_pk_bf16_fp4: the block scale rides in the convert)
//   q8   P = 16; it feeds NF = 2 MFMAs, fragment f being dwords 2 f, 2 f + 1 through q8frag (exact: an int8
//        has 7 significant bits).  The row scale is not in the fragment: the accumulator holds the unscaled
//        integer-weight sum and the scale multiplies it once in the epilogue, before the bias (the rule of
//        the other _q8 kernels).
// The 32x32x16 MFMA takes k = 8 (l >> 5) .. + 7 from lane l, so lane group h = l >> 5 owns piece 2 j + h of
// the j-th unit of 2 P k: element i of MFMA f of that unit is k = 2 P j + P h + 8 f + i of the chunk.  The X
// fragment of the same MFMA is the 16 bytes of row 32 t + (l & 31) at the same k: both operands permute k
// alike, which a dot product does not see.
//
// X through LDS.  The tile's X goes once through LDS in chunks of CHUNK k, double-buffered and shared by the
// four waves: the 16-byte global loads of chunk i + 1 (and the weight loads of chunk i + 1) are issued before
// the MFMAs of chunk i and land in the other buffer behind one barrier per chunk.  CHUNK is 128 k for q8 and
// 256 k for mx4: UN = CHUNK / (2 P) = 4 weight loads of 16 bytes in flight per lane in both (mx4: plus their
// 4 scale bytes), half of what the bf16 tall kernel keeps in flight per lane, and as many bytes of the
// weight stream as the quantized wide kernel.  NSA_QGEMM_CHUNK_Q8 / NSA_QGEMM_CHUNK_MX4 (compile-time
// overrides, for measuring only) force another size.
// The image is [128][CHUNK + 8] bf16 per buffer: 2 x 128 x 136 x 2 = 69632 bytes for q8 and 2 x 128 x 264 x 2 =
// 135168 bytes for mx4.  Registers: q8 199 VGPRs + 64 AGPRs, mx4 254 + 64, no scratch: one workgroup per CU
// (one wave per SIMD) in both; a q8 chunk of 256 k (8 loads in flight) needs 256 + 86 and moves values
// through AGPRs, so it stays at 128.  The row stride is (CHUNK + 8) / 2 dwords = 4 mod 64 for both.  The ds_read_b128 of lane (c, h) starts at dword c stride + P h / 2 + 4 f + P j, bank
// 4 c + P h / 2 + const (mod 64): the 16 lanes of one pass (c .. c + 15 of one lane group) start 4 banks
// apart and cover the 64 banks once each, rotated by a constant; a pass never mixes lane groups (an unpadded
// row, stride 0 mod 64, would put all 16 lanes on 4 banks).  Staging writes consecutive 16-byte pieces from
// consecutive lanes.  One wave per SIMD and workgroup: the four X fragments of MFMA step s + 1 are read, and
// its weight fragment converted, before the four MFMAs of step s, as in the tall kernel.
//
// Edges.  Rows past M are clamped on load (row M - 1 again) and not stored.  Weight rows past N re-read row
// N - 1 and are not stored; a wave whose 32 columns all lie past N only helps stage X.  K is whole granules
// but not whole chunks: piece p0 + 2 j + h is live while it is below K / P; a dead piece re-reads the row's
// last piece (and its scale byte) and zeroes the weight dwords, branch-free, and X past K is staged as zeros,
// so the LDS image is always finite and every MFMA of a chunk runs.  y is stored 4 columns (8 bytes) at a
// time where N % 4 == 0 and y is 8-byte aligned, element by element otherwise.
//
// Tile order.  The dispatcher places workgroup v of the grid on XCD v % 8, and the XCDs' L2s are separate, so
// ids are first remapped to give an XCD consecutive tiles (the remap of gemm.hip), and consecutive tiles walk
// the row tiles of one column tile before moving to the next column tile.  Workgroups resident together on an
// XCD therefore share a column tile's weights in L2.  The weights rather than X: the weight loads feed the
// convert and the MFMA directly with only UN loads in flight per lane, so their latency is the exposed one and
// an L2 hit shortens it, while X is prefetched a whole chunk ahead through LDS for all four waves; and at the
// few row tiles of a short prompt or an admission (M <= 128 B) the walk covers all of X anyway.
#include "decode_rows.h"

#ifndef NSA_QGEMM_CHUNK_MX4
#define NSA_QGEMM_CHUNK_MX4 256
#endif
#ifndef NSA_QGEMM_CHUNK_Q8
#define NSA_QGEMM_CHUNK_Q8 128
#endif

namespace {

constexpr int QG_TILE_M = 128;  // rows of a workgroup's tile: 4 blocks of 32
constexpr int QG_TILE_N = 128;  // its output columns: one wave per 32
constexpr int QG_RB = QG_TILE_M / 32;

// the converts of decode_mx4.hip and decode_q8.hip (their file-local helpers, repeated here as in
// decode_wide_q.hip)
typedef __bf16 qg_bf16x2 __attribute__((ext_vector_type(2)));

// dword d (8 nibbles, k order) times the scale -> one MFMA fragment
__device__ __forceinline__ bf16x8 mx_frag(uint32_t d, float s) {
  const qg_bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0);
  const qg_bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
  const qg_bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2);
  const qg_bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
  const uint4 u = {__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1),
                   __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3)};
  return __builtin_bit_cast(bf16x8, u);
}

// bytes j, j + 1 of a dword as a packed bf16 pair: the high halves of the two exact fp32 forms
__device__ __forceinline__ uint32_t q8bf2(uint32_t w, int j) {
  return __builtin_amdgcn_perm(__float_as_uint(q8f(w, j + 1)), __float_as_uint(q8f(w, j)), 0x07060302u);
}
// the 8 weights of two dwords as one MFMA fragment
__device__ __forceinline__ bf16x8 q8frag(uint32_t lo, uint32_t hi) {
  const uint4 u = {q8bf2(lo, 0), q8bf2(lo, 2), q8bf2(hi, 0), q8bf2(hi, 2)};
  return __builtin_bit_cast(bf16x8, u);
}

// One weight format: P k per 16-byte piece, NF MFMAs per piece, GRANULE: what K must be a multiple of
struct QgMx4 {
  static constexpr int P = 32, NF = 4, GRANULE = 32, CHUNK = NSA_QGEMM_CHUNK_MX4;
  static constexpr bool BLOCK_SCALE = true;
  // a piece's dequantizing factor: the E8M0 byte e as the fp32 2^(e - 127)
  static __device__ __forceinline__ float factor(uint32_t e) { return __uint_as_float(e << 23); }
  static __device__ __forceinline__ bf16x8 frag(const uint4& d, int f, float s) {
    return mx_frag(f == 0 ? d.x : f == 1 ? d.y : f == 2 ? d.z : d.w, s);
  }
};
struct QgQ8 {
  static constexpr int P = 16, NF = 2, GRANULE = 64, CHUNK = NSA_QGEMM_CHUNK_Q8;
  static constexpr bool BLOCK_SCALE = false;
  static __device__ __forceinline__ float factor(uint32_t) { return 1.0f; }
  static __device__ __forceinline__ bf16x8 frag(const uint4& d, int f, float) {
    return f == 0 ? q8frag(d.x, d.y) : q8frag(d.z, d.w);
  }
};
static_assert(QgMx4::CHUNK % (2 * QgMx4::P) == 0 && QgQ8::CHUNK % (2 * QgQ8::P) == 0 && QgMx4::CHUNK <= 256 &&
                  QgQ8::CHUNK <= 256 && QgMx4::CHUNK >= 64 && QgQ8::CHUNK >= 64,
              "a chunk is whole units of 2 P k, its rows shared out among 256 threads, its image within the LDS");

template <typename F>
bool qg_shape_ok(int M, int N, int K) {
  // the row tiles are the grid's y dimension
  return M >= 1 && (M + QG_TILE_M - 1) / QG_TILE_M <= 65535 && N >= 1 && K >= F::GRANULE && K % F::GRANULE == 0;
}

template <typename F, int ACT>
__global__ __launch_bounds__(256) void quant_gemm_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ Wq,
                                                         const void* __restrict__ scale,
                                                         const bf16_t* __restrict__ bias, bf16_t* __restrict__ y,
                                                         int M, int N, int K) {
  constexpr int P = F::P, NF = F::NF, CH = F::CHUNK, RB = QG_RB;
  constexpr int KP = CH + 8;                 // padded row of the LDS image
  constexpr int CP = CH / P, UN = CP / 2;    // pieces per chunk; weight loads in flight per lane
  constexpr int XC = CH / 8, XR = 256 / XC;  // 16-byte pieces of a chunk row; rows the threads stage per pass
  constexpr int XV = QG_TILE_M / XR;         // 16-byte pieces of a chunk per thread
  constexpr int STEPS = UN * NF;             // MFMA steps (16 k each) per chunk
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [2][QG_TILE_M][KP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  // tile order: XCD v % 8 gets consecutive tiles u, and u walks the row tiles of one column tile first
  const int CT = gridDim.x, RT = gridDim.y, total = CT * RT;
  const int v = blockIdx.x + CT * blockIdx.y;
  const int xcd = v % 8, tq = total / 8, tr = total % 8;
  const int u = (xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq) + v / 8;
  const int m0 = (u % RT) * QG_TILE_M, n0 = (u / RT) * QG_TILE_N + 32 * w;
  const bool live = n0 < N;  // wave-uniform: a wave past N only helps staging X
  const int PT = K / P;      // pieces of a weight row
  const int64_t nrow = min(n0 + c, N - 1);
  const uint8_t* wrow = Wq + nrow * (F::BLOCK_SCALE ? K / 2 : K);
  const uint8_t* srow = reinterpret_cast<const uint8_t*>(scale) + nrow * (K / 32);  // mx4 only
  // staging: piece e = tid + 256 i of a chunk is tile row e / XC, k offset 8 (e % XC)
  const int xr = tid / XC, xc = tid % XC;
  const bf16_t* xcol = x + (int64_t)m0 * K + 8 * xc;
  const int mlast = M - 1 - m0;  // the tile's last live row

  // pieces past PT: the weight dwords are zero (the row's last piece re-read, branch-free) and X's pieces
  // are zeros
  auto load_a = [&](int p0, uint4 (&dst)[UN], uint32_t (&e)[UN]) {
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int p = p0 + 2 * j + h;
      const int pc = p < PT ? p : PT - 1;
      dst[j] = *reinterpret_cast<const uint4*>(wrow + 16 * pc);
      if constexpr (F::BLOCK_SCALE) e[j] = srow[pc];
      if (p >= PT) dst[j] = uint4{0u, 0u, 0u, 0u};
    }
  };
  auto load_x = [&](int p0, uint4 (&dst)[XV]) {
    const bool in = P * p0 + 8 * xc < K;
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      dst[i] = uint4{0u, 0u, 0u, 0u};
      if (in) dst[i] = *reinterpret_cast<const uint4*>(xcol + min(xr + XR * i, mlast) * K + P * p0);
    }
  };
  auto store_x = [&](int buf, const uint4 (&src)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; ++i)
      *reinterpret_cast<uint4*>(xs + buf * QG_TILE_M * KP + (xr + XR * i) * KP + 8 * xc) = src[i];
  };

  f32x16 acc[RB];
#pragma unroll
  for (int t = 0; t < RB; ++t) acc[t] = f32x16{};
  uint4 a[UN], xq[XV];
  uint32_t ae[UN] = {};
  if (live) load_a(0, a, ae);
  load_x(0, xq);
  store_x(0, xq);
  __syncthreads();
  int buf = 0;
  for (int p0 = 0; p0 < PT; p0 += CP, buf ^= 1) {
    const bool more = p0 + CP < PT;  // workgroup-uniform
    uint4 an[UN];
    uint32_t ane[UN] = {};
    if (more) {
      if (live) load_a(p0 + CP, an, ane);
      load_x(p0 + CP, xq);
    }
    if (live) {
      const bf16_t* xb = xs + buf * QG_TILE_M * KP + c * KP + P * h;
      // step s: piece s / NF of the lane, its MFMA f = s % NF (k offset 2 P (s / NF) + P h + 8 f) on every row
      // block.  The X fragments and the converted weight fragment of step s + 1 are made before the MFMAs
      // of step s; the scheduling barriers keep the compiler from sinking them back to their use.
      auto frags = [&](int s, uint4 (&dst)[RB]) {
#pragma unroll
        for (int t = 0; t < RB; ++t)
          dst[t] = *reinterpret_cast<const uint4*>(xb + 32 * t * KP + 2 * P * (s / NF) + 8 * (s % NF));
      };
      auto wfrag = [&](int s) { return F::frag(a[s / NF], s % NF, F::factor(ae[s / NF])); };
      uint4 b[RB], bn[RB];
      frags(0, b);
      bf16x8 af = wfrag(0), afn = af;
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        if (s + 1 < STEPS) {
          frags(s + 1, bn);
          afn = wfrag(s + 1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RB; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(bf16x8, b[t]), acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RB; ++t) b[t] = bn[t];
        af = afn;
      }
    }
    if (more) {
      // the other buffer was last read before the barrier that ended the previous chunk
      store_x(buf ^ 1, xq);
      if (live) {
#pragma unroll
        for (int j = 0; j < UN; ++j) {
          a[j] = an[j];
          ae[j] = ane[j];
        }
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
    bf16_t* yrow = y + (int64_t)m * N;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 8 * q + 4 * h;
      bf16_t o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ni = min(n + i, N - 1);  // past N: computed on column N - 1, not stored
        float r = acc[t][4 * q + i];
        if constexpr (!F::BLOCK_SCALE) r *= reinterpret_cast<const float*>(scale)[ni];
        if (bias) r += bf2f(bias[ni]);
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

template <typename F, int ACT>
hipError_t qg_launch(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int M, int N, int K,
                     hipStream_t s) {
  constexpr int lds = 2 * QG_TILE_M * (F::CHUNK + 8) * (int)sizeof(bf16_t);
  static bool attr = [] {  // dynamic LDS above 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&quant_gemm_kernel<F, ACT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  }();
  if (!attr) return hipErrorInvalidValue;
  const dim3 grid((N + QG_TILE_N - 1) / QG_TILE_N, (M + QG_TILE_M - 1) / QG_TILE_M);
  quant_gemm_kernel<F, ACT><<<grid, 256, lds, s>>>((const bf16_t*)x, (const uint8_t*)Wq, scale, (const bf16_t*)bias,
                                                   (bf16_t*)y, M, N, K);
  return hipGetLastError();
}

template <typename F>
hipError_t qg_gemm(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int M, int N, int K,
                   int act, hipStream_t s) {
  if (!qg_shape_ok<F>(M, N, K) || !x || !Wq || !scale || !y || act < 0 || act > 1) return hipErrorInvalidValue;
  return act ? qg_launch<F, 1>(x, Wq, scale, bias, y, M, N, K, s) : qg_launch<F, 0>(x, Wq, scale, bias, y, M, N, K, s);
}

}  // namespace

// k per LDS chunk of X (ops/functional.py mirrors these: the tests take their K edges from them)
NSA_API int nsa_quant_gemm_q8_chunk() { return QgQ8::CHUNK; }
NSA_API int nsa_quant_gemm_mx4_chunk() { return QgMx4::CHUNK; }

// y[M, N] (bf16) = act(x[M, K] Wq[N, K]^T scale[n] + b): int8 weights Wq [N, K], one fp32 scale per output
// column, scale [N]; any M >= 1 and N >= 1, K % 64 == 0; bias may be NULL, act 1: exact-erf GELU.  x and the
// weight rows are read in 16-byte pieces (16-byte aligned, as every allocation is).  Anything else is
// refused with hipErrorInvalidValue and nothing is launched.
NSA_API hipError_t nsa_quant_gemm_q8(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                     int M, int N, int K, int act, hipStream_t s) {
  return qg_gemm<QgQ8>(x, Wq, scale, bias, y, M, N, K, act, s);
}

// The same with MXFP4 weights: Wq the nibble matrix [N, K / 2], scale the E8M0 bytes [N, K / 32]; K % 32 == 0
NSA_API hipError_t nsa_quant_gemm_mx4(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                      int M, int N, int K, int act, hipStream_t s) {
  return qg_gemm<QgMx4>(x, Wq, scale, bias, y, M, N, K, act, s);
}
