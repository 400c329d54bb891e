// Decode linear for 17 .. 64 rows with quantized weights: nsa_wide_gemm (decode_wide.hip) streaming int8
// (nsa_wide_gemm_q8) or MXFP4 (nsa_wide_gemm_mx4) weights, 2x and 3.8x fewer bytes through the same
// workgroup: 256 threads, all rows as MT = 2 or 4 groups of 16, WIDE_TILE_N = 64 output columns (one wave
// per 16), X staged once per workgroup through LDS in double-buffered chunks that the four waves share,
// weights straight to registers as the A operand of v_mfma_f32_16x16x32_bf16, grid = (column tiles) x KS
// with the ticket, the fences and the fixed-order reduction of fp32 partials of the bf16 kernel (its
// header tells why each is there), counters left at zero after every launch.
//
// The fragment plan.  A lane's 16-byte weight load is a piece of P consecutive k of its row n0 + (l & 15):
//   mx4  P = 32: one MX block, with its E8M0 scale byte; it feeds NF = 4 MFMAs, the A fragment of MFMA h
//        being dword h through mx_frag (v_cvt_scalef32_pk_bf16_fp4: the block scale rides in the convert)
//   q8   P = 16; it feeds NF = 2 MFMAs, fragment h being dwords 2h, 2h + 1 through q8frag (exact: an int8
//        has 7 significant bits).  The row scale is not in the fragment: partials are unscaled integer-weight
//        sums, and the scale multiplies each output once, after the cross-split reduction and before the
//        bias, so the bits do not depend on the split's arrival order
// Lane group g = l >> 4 owns piece 4 j + g of the j-th unit of 4 P k, so element i of MFMA h of that unit
// is k = 4 P j + P g + 8 h + i of the chunk.  The X fragment of the same MFMA is the 16 bytes of batch row
// 16 t + (l & 15) at the same k: both fragments permute k alike, which a dot product does not see.
//
// K is split in granules (mx4: one block of 32; q8: one unit of 64), workgroup (tile, ks) taking the
// granules G ks / KS .. G (ks + 1) / KS - 1: uneven ranges, a partial last chunk.  A chunk starts at the
// range's first piece, not at a multiple of 4 P, and liveness is per lane group: piece p0 + 4 j + g is
// live while it is below the range's end (K = 1600 in mx4: 50 blocks, the last unit half dead).  A dead
// piece re-reads the range's last piece (and its scale byte) and zeroes the weight dwords, branch-free,
// and X past the range is staged as zeros, so the LDS image is always finite and every MFMA of a chunk
// runs.  Weight rows past N re-read row N - 1 and are not stored: any N >= 1.
//
// LDS image [16 MT][CHUNK + 8] bf16 per buffer.  The row stride is (CHUNK + 8) / 2 dwords = 4 mod 64 for
// CHUNK = 256 and 512.  The B fragment's ds_read_b128 of lane (c, g) starts at dword
// c stride + P g / 2 + 4 h + 2 P j, bank 4 c + P g / 2 + const (mod 64): the 16 lanes of one lane group
// (one quarter-wave, what a 128-bit read serves per pass) cover the banks 4 c .. 4 c + 3, c = 0 .. 15,
// rotated by a constant, each bank once.  The rotation P g / 2 (16 or 8 dwords) differs from the bf16
// kernel's 4 g, but a pass never mixes lane groups, so the read stays conflict-free; checked by this
// arithmetic for both P and both chunk sizes (an unpadded row, stride 0 mod 64, puts all 16 lanes on 4 banks).
// Staging writes consecutive 16-byte pieces from consecutive lanes.
//
// Chunk: 512 k for mx4 (4 weight loads per lane in flight; at 256 only 2, against the bf16 kernel's 8)
// and 256 k for q8 (4 loads).  At 64 rows the mx4 image is 2 x 64 x 520 x 2 = 133120 bytes: one workgroup
// per CU.  NSA_WIDEQ_CHUNK_MX4 / NSA_WIDEQ_CHUNK_Q8 (compile-time overrides, for measuring only) force
// another size.  The split rule is wide_ksplit_rule's in k: up to WIDE_TARGET_WGS workgroups of at least
// 32 WIDE_MIN_UNITS = 1024 k each.
//
// Workspace: as nsa_wide_gemm's, [counters: int per tile, 256-byte padded, zero between launches]
// [partials: per (tile, ks, wave, row group) 64 lanes x f32x4 in the accumulator layout].
#include "decode_rows.h"

#ifndef NSA_WIDEQ_CHUNK_MX4
#define NSA_WIDEQ_CHUNK_MX4 512
#endif
#ifndef NSA_WIDEQ_CHUNK_Q8
#define NSA_WIDEQ_CHUNK_Q8 256
#endif

namespace {

constexpr int WQ_MIN_K = 32 * WIDE_MIN_UNITS;  // the split rule: at least this many k per workgroup

// the converts of decode_mx4.hip and decode_q8.hip (their file-local helpers, repeated here)
typedef __bf16 wq_bf16x2 __attribute__((ext_vector_type(2)));

// dword d (8 nibbles, k order) times the scale -> one MFMA fragment
__device__ __forceinline__ bf16x8 mx_frag(uint32_t d, float s) {
  const wq_bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0);
  const wq_bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
  const wq_bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2);
  const wq_bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
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

// One weight format: P k per 16-byte piece, NF MFMAs per piece, RG pieces per split granule
struct WqMx4 {
  static constexpr int P = 32, NF = 4, RG = 1, CHUNK = NSA_WIDEQ_CHUNK_MX4;
  static constexpr bool BLOCK_SCALE = true;
  // a piece's dequantizing factor: the E8M0 byte e as the fp32 2^(e - 127)
  static __device__ __forceinline__ float factor(uint32_t e) { return __uint_as_float(e << 23); }
  static __device__ __forceinline__ bf16x8 frag(const uint32_t (&d)[4], int h, float s) { return mx_frag(d[h], s); }
};
struct WqQ8 {
  static constexpr int P = 16, NF = 2, RG = 4, CHUNK = NSA_WIDEQ_CHUNK_Q8;
  static constexpr bool BLOCK_SCALE = false;
  static __device__ __forceinline__ float factor(uint32_t) { return 1.0f; }
  static __device__ __forceinline__ bf16x8 frag(const uint32_t (&d)[4], int h, float) {
    return q8frag(d[2 * h], d[2 * h + 1]);
  }
};
static_assert(WqMx4::CHUNK % (4 * WqMx4::P) == 0 && WqQ8::CHUNK % (4 * WqQ8::P) == 0 && WqMx4::CHUNK <= 512 &&
                  WqQ8::CHUNK <= 512 && WqMx4::CHUNK >= 128 && WqQ8::CHUNK >= 128,
              "a chunk is whole units of 4 P k, its rows shared out among 256 threads, its image within the LDS");

int wq_tiles(int N) { return (N + WIDE_TILE_N - 1) / WIDE_TILE_N; }

template <typename F>
constexpr int wq_granule() {  // k per split granule: what K must be a multiple of
  return F::P * F::RG;
}

int wq_ksplit_rule(int N, int K) { return std::max(std::min(WIDE_TARGET_WGS / wq_tiles(N), K / WQ_MIN_K), 1); }

constexpr int64_t wq_counter_bytes(int tiles) { return ((int64_t)tiles * 4 + 255) / 256 * 256; }

template <typename F>
bool wq_shape_ok(int rows, int N, int K) {
  return rows >= 1 && rows <= WIDE_MAX_ROWS && N >= 1 && K >= wq_granule<F>() && K % wq_granule<F>() == 0;
}

int64_t wq_ws_bytes(int rows, int N, int ks) {
  if (ks <= 1) return 0;
  const int mt = rows <= 32 ? 2 : 4;
  return wq_counter_bytes(wq_tiles(N)) + (int64_t)wq_tiles(N) * ks * 4 * mt * 64 * sizeof(f32x4);
}

template <typename F, int MT, int ACT, bool OUTF>
__global__ __launch_bounds__(256) void wide_q_gemm_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ Wq,
                                                          const void* __restrict__ scale,
                                                          const bf16_t* __restrict__ bias, void* __restrict__ yv,
                                                          int M, int N, int K, int KS, int* counters, f32x4* parts) {
  constexpr int P = F::P, NF = F::NF, CH = F::CHUNK;
  constexpr int ROWS = 16 * MT, KP = CH + 8;  // KP: padded row of the LDS image
  constexpr int CP = CH / P, UN = CP / 4;     // pieces per chunk; weight loads in flight per lane
  constexpr int XC = CH / 8, XR = 256 / XC;   // 16-byte pieces of a chunk row; rows the threads stage per pass
  constexpr int XV = ROWS / XR;               // 16-byte pieces of a chunk per thread
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [2][ROWS][KP]
  __shared__ int ticket;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int tile = blockIdx.x, ks = blockIdx.y;
  const int n0 = tile * WIDE_TILE_N + 16 * w;
  const bool live = n0 < N;  // wave-uniform: a column group past N only helps staging X
  const int G = K / (P * F::RG);
  const int p_lo = F::RG * (int)((int64_t)G * ks / KS), p_hi = F::RG * (int)((int64_t)G * (ks + 1) / KS);
  const int64_t nrow = min(n0 + c, N - 1);
  const uint8_t* wrow = Wq + nrow * (F::BLOCK_SCALE ? K / 2 : K);
  const uint8_t* srow = reinterpret_cast<const uint8_t*>(scale) + nrow * (K / 32);  // mx4 only
  // staging: piece e = tid + 256 i of a chunk is row e / XC, k offset 8 (e % XC)
  const int xr = tid / XC, xc = tid % XC;
  int xo[XV];
#pragma unroll
  for (int i = 0; i < XV; ++i) xo[i] = min(xr + XR * i, M - 1) * K + 8 * xc;

  // pieces past p_hi: the weight dwords are zero (the range's last piece re-read, branch-free) and X's
  // pieces are zeros
  auto load_a = [&](int p0, uint4 (&dst)[UN], uint32_t (&e)[UN]) {
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int p = p0 + 4 * j + g;
      const int pc = p < p_hi ? p : p_hi - 1;
      dst[j] = *reinterpret_cast<const uint4*>(wrow + 16 * pc);
      if constexpr (F::BLOCK_SCALE) e[j] = srow[pc];
      if (p >= p_hi) dst[j] = uint4{0u, 0u, 0u, 0u};
    }
  };
  auto load_x = [&](int p0, uint4 (&dst)[XV]) {
    const bool in = P * p0 + 8 * xc < P * p_hi;
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      dst[i] = uint4{0u, 0u, 0u, 0u};
      if (in) dst[i] = *reinterpret_cast<const uint4*>(x + xo[i] + P * p0);
    }
  };
  auto store_x = [&](int buf, const uint4 (&src)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; ++i)
      *reinterpret_cast<uint4*>(xs + buf * ROWS * KP + (xr + XR * i) * KP + 8 * xc) = src[i];
  };

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{};
  uint4 a[UN], xq[XV];
  uint32_t ae[UN] = {};
  if (live) load_a(p_lo, a, ae);
  load_x(p_lo, xq);
  store_x(0, xq);
  __syncthreads();
  int buf = 0;
  for (int p0 = p_lo; p0 < p_hi; p0 += CP, buf ^= 1) {
    const bool more = p0 + CP < p_hi;  // workgroup-uniform
    uint4 an[UN];
    uint32_t ane[UN] = {};
    if (more) {
      if (live) load_a(p0 + CP, an, ane);
      load_x(p0 + CP, xq);
    }
    if (live) {
      const bf16_t* xb = xs + buf * ROWS * KP + c * KP + P * g;
#pragma unroll
      for (int j = 0; j < UN; ++j) {
        const uint32_t d[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
        const float s = F::factor(ae[j]);
#pragma unroll
        for (int h = 0; h < NF; ++h) {
          const bf16x8 af = F::frag(d, h, s);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const uint4 b = *reinterpret_cast<const uint4*>(xb + 16 * t * KP + 4 * P * j + 8 * h);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(bf16x8, b), acc[t], 0, 0, 0);
          }
        }
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

  if (KS > 1) {
    f32x4* mine = parts + (((int64_t)tile * KS + ks) * 4 + w) * MT * 64 + lane;
    if (live) {
#pragma unroll
      for (int t = 0; t < MT; ++t) mine[t * 64] = acc[t];
    }
    // the barrier orders the four waves' stores before thread 0, whose agent-scope release fence makes the
    // whole partial visible to the device before the ticket is
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      ticket = atomicAdd(counters + tile, 1);
    }
    __syncthreads();
    if (ticket != KS - 1) return;
    __threadfence();  // acquire: the last one in sees every earlier partial
    if (live) {
      const f32x4* p = parts + ((int64_t)tile * KS * 4 + w) * MT * 64 + lane;
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = p[t * 64];
      for (int q = 1; q < KS; ++q) {
        p += 4 * MT * 64;
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] += p[t * 64];
      }
    }
    if (tid == 0) counters[tile] = 0;  // for the next launch on this stream
  }
  if (!live) return;
  // C layout: lane l holds batch row m = 16 t + (l & 15), output columns n0 + 4 (l >> 4) + i
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + c;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + 4 * g + i;
      if (n >= N) continue;
      float v = acc[t][i];
      if constexpr (!F::BLOCK_SCALE) v *= reinterpret_cast<const float*>(scale)[n];
      if (bias) v += bf2f(bias[n]);
      if constexpr (ACT == 1) v = nsa_gelu(v);
      if constexpr (OUTF)
        reinterpret_cast<float*>(yv)[(int64_t)m * N + n] = v;
      else
        reinterpret_cast<bf16_t*>(yv)[(int64_t)m * N + n] = f2bf(v);
    }
  }
}

template <typename F, int MT, int ACT, bool OUTF>
hipError_t wq_launch(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int rows, int N,
                     int K, int ks, void* ws, hipStream_t s) {
  constexpr int lds = 2 * 16 * MT * (F::CHUNK + 8) * (int)sizeof(bf16_t);
  static bool attr = [] {  // dynamic LDS above 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&wide_q_gemm_kernel<F, MT, ACT, OUTF>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  }();
  if (!attr) return hipErrorInvalidValue;
  const int tiles = wq_tiles(N);
  wide_q_gemm_kernel<F, MT, ACT, OUTF><<<dim3(tiles, ks), 256, lds, s>>>(
      (const bf16_t*)x, (const uint8_t*)Wq, scale, (const bf16_t*)bias, y, rows, N, K, ks, (int*)ws,
      (f32x4*)((char*)ws + wq_counter_bytes(tiles)));
  return hipGetLastError();
}

// the guards of nsa_wide_gemm, then the launch
template <typename F>
hipError_t wq_gemm(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int rows, int N, int K,
                   int act, int out_f32, int ksplit, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (!wq_shape_ok<F>(rows, N, K) || (act && out_f32) || ksplit < 0 || ksplit > K / wq_granule<F>() || ksplit > 65535)
    return hipErrorInvalidValue;
  const int ks = ksplit ? ksplit : wq_ksplit_rule(N, K);
  if (ks > 1 && (!ws || (uintptr_t)ws % 16 || ws_bytes < wq_ws_bytes(rows, N, ks))) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto launch = [&](auto MT) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      e = wq_launch<F, decltype(MT)::value, decltype(ACT)::value, decltype(OUTF)::value>(x, Wq, scale, bias, y, rows,
                                                                                         N, K, ks, ws, s);
    });
  };
  if (rows <= 32)
    launch(int_c<2>{});
  else
    launch(int_c<4>{});
  return e;
}

template <typename F>
int64_t wq_ws_query(int rows, int N, int K, int ksplit) {
  if (!wq_shape_ok<F>(rows, N, K) || ksplit < 0) return 0;
  return wq_ws_bytes(rows, N, ksplit ? ksplit : wq_ksplit_rule(N, K));
}

}  // namespace

// The split the fixed rule picks for a shape (what ksplit = 0 means); 0 for a shape the kernel refuses
NSA_API int nsa_wide_gemm_mx4_ksplit(int rows, int N, int K) {
  return wq_shape_ok<WqMx4>(rows, N, K) ? wq_ksplit_rule(N, K) : 0;
}
NSA_API int nsa_wide_gemm_q8_ksplit(int rows, int N, int K) {
  return wq_shape_ok<WqQ8>(rows, N, K) ? wq_ksplit_rule(N, K) : 0;
}

// Bytes of workspace a launch with this ksplit needs (0: the rule's split); 0 when it uses none
NSA_API int64_t nsa_wide_gemm_mx4_ws_bytes(int rows, int N, int K, int ksplit) {
  return wq_ws_query<WqMx4>(rows, N, K, ksplit);
}
NSA_API int64_t nsa_wide_gemm_q8_ws_bytes(int rows, int N, int K, int ksplit) {
  return wq_ws_query<WqQ8>(rows, N, K, ksplit);
}

// y[rows, N] = act(x[rows, K] W[N, K]^T + b) for 1 <= rows <= 64, any N, K % 32 == 0; Wq the nibble matrix
// [N, K / 2], scale the E8M0 bytes [N, K / 32]; bias may be NULL, act 1: exact-erf GELU, out_f32: fp32 y.
// ksplit: workgroups along K (0: the rule's; at most K / 32).  ws: the workspace of ws_bytes (16-byte
// aligned, its counters zero; every launch leaves them zero), needed when the split is above 1.
NSA_API hipError_t nsa_wide_gemm_mx4(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                     int rows, int N, int K, int act, int out_f32, int ksplit, void* ws,
                                     int64_t ws_bytes, hipStream_t s) {
  return wq_gemm<WqMx4>(x, Wq, scale, bias, y, rows, N, K, act, out_f32, ksplit, ws, ws_bytes, s);
}

// The same with int8 weights Wq [N, K] and one fp32 scale per output column, scale [N]: any N, K % 64 == 0,
// ksplit at most K / 64
NSA_API hipError_t nsa_wide_gemm_q8(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                    int rows, int N, int K, int act, int out_f32, int ksplit, void* ws,
                                    int64_t ws_bytes, hipStream_t s) {
  return wq_gemm<WqQ8>(x, Wq, scale, bias, y, rows, N, K, act, out_f32, ksplit, ws, ws_bytes, s);
}
