// Decode linear for 65 .. 128 rows with quantized weights: nsa_tall_gemm (decode_tall.hip) streaming int8
// (nsa_tall_gemm_q8) or MXFP4 (nsa_tall_gemm_mx4) weights through the tall kernel's workgroup: 256 threads own
// all rows (RB = 3 or 4 blocks of 32) and TALL_TILE_N = 128 output columns, one wave per 32 on
// v_mfma_f32_32x32x16_bf16; X goes once per workgroup through the padded, double-buffered LDS image
// [32 RB][CHUNK + 8]; weights go straight to registers as the A operand; grid = (column tiles) x KS with the
// ticket, the fences and the fixed-order reduction of fp32 partials of the bf16 kernel (its header tells why each
// is there), counters left at zero after every launch.  Layouts, epilogues and refusals are those of
// nsa_wide_gemm_q8 / _mx4 (decode_wide_q.hip); fp32 accumulation on bf16 MFMAs, no integer MFMA.
//
// The fragment plan.  Lane l = (c, h) = (l & 31, l >> 5) holds weight row n0 + c.  Its 16-byte weight load is a
// piece of P consecutive k of that row, and the two lanes of a row take the two pieces of a unit of 2 P k:
//   q8   P = 16: the 16 int8 at k = 32 u + 16 h .. + 15 of unit u.  One load feeds NF = 2 MFMAs, fragment s being
//        dwords 2 s, 2 s + 1 through q8frag (exact: an int8 has 7 significant bits), so MFMA s of unit u multiplies
//        k = 32 u + 16 h + 8 s .. + 7: the bf16 tall kernel's K permutation, and the B fragment is read from the
//        image at the tall kernel's offsets.  The row scale is not in the fragment: partials are unscaled
//        integer-weight sums, and the scale multiplies each output once, after the cross-split reduction and before
//        the bias, so the bits do not depend on the split's arrival order
//   mx4  P = 32: one MX block with its E8M0 scale byte.  One load feeds NF = 4 MFMAs, the fragment of MFMA s being
//        dword s through mx_frag (v_cvt_scalef32_pk_bf16_fp4: the block scale rides in the convert).  The two
//        lanes of a row take the two blocks of a 64-k unit: MFMA s of unit j multiplies k = 64 j + 32 h + 8 s .. + 7
// In both, element i of MFMA s of the j-th unit of a chunk is k = 2 P j + P h + 8 s + i, and the X fragment of that
// MFMA is the 16 bytes of batch row 32 t + c at the same k: both fragments permute k alike, which a dot product
// does not see.  The C layout is the tall kernel's.
//
// K is split in granules (mx4: one block of 32; q8: 64 k, four pieces), workgroup (tile, ks) taking the granules
// G ks / KS .. G (ks + 1) / KS - 1: uneven ranges, a partial last chunk.  A chunk starts at the range's first
// piece, and liveness is per lane: piece p0 + 2 j + h is live while it is below the range's end (K = 1600 in mx4:
// 50 blocks, the last unit half dead).  A dead piece re-reads the range's last piece (and its scale byte) and
// zeroes the weight dwords, branch-free, and X past the range is staged as zeros, so the LDS image is always finite
// and every MFMA of a chunk runs.  Weight rows past N re-read row N - 1 and are never stored: any N >= 1.  Rows
// past `rows` in the last block are clamped reads (row rows - 1 again) and are never stored.
//
// LDS image [32 RB][CHUNK + 8] bf16 per buffer.  The row stride is (CHUNK + 8) / 2 dwords: 68 at CHUNK = 128, 132 at
// 256, both 4 mod 64.  The B fragment's ds_read_b128 of lane (c, h) starts at dword c stride + P h / 2 + 4 s + P j
// (+ 32 t stride = 0 mod 64 for row block t), bank 4 c + P h / 2 + const (mod 64).  A 128-bit read
// serves 16 lanes per pass: lanes 16 a .. 16 a + 15 share h = a >> 1 and have c = 16 (a & 1) .. + 15, so their start
// banks are 4 (c & 15) plus one constant (64 (a & 1) + P h / 2 + const), and the 16 four-bank spans cover the 64
// banks once.  The rotation P h / 2 (8 dwords for q8, as in the bf16 kernel; 16 for mx4) only moves the whole pass;
// an unpadded row (stride 0 mod 64) would put all 16 lanes on 4 banks.  Staging writes consecutive 16-byte pieces
// from consecutive lanes.
//
// Chunk: 256 k for q8 (8 weight loads per lane in flight, the bf16 kernel's count; the image at RB = 3 / 4 is
// 2 x 32 RB x 264 x 2 = 101376 / 135168 bytes, one workgroup per CU) and 128 k for mx4 (2 loads; 52224 / 69632
// bytes, two per CU).  The plan started from four loads in flight for both (q8 128, mx4 256); in the captured
// step that pairing was the slower one where the two differed by more than the repeat spread (q8 at 65 - 96
// rows, mx4 at 128 rows on the small model; docs/performance.md has both).  NSA_TALLQ_CHUNK_MX4 /
// NSA_TALLQ_CHUNK_Q8 (compile-time overrides, for measuring only) force another size.
//
// The split (tq_ksplit_rule) is tall_ksplit_rule's cost, a fixed function of the shape, with the format's weight
// bytes per 32 k in the stream term: 32 for q8, 17 for mx4 (16 bytes of nibbles and the scale byte).  The smaller
// stream makes the partials' round trip dearer against it, so the quantized forms split less than the bf16 kernel.
//
// Workspace: the tall kernel's, [counters: TALL_MAX_SPLIT_TILES ints, zero between launches][partials: per (tile,
// ks, wave, row block, quarter) 64 lanes x f32x4 in the accumulator layout].
#include "decode_rows.h"

#ifndef NSA_TALLQ_CHUNK_MX4
#define NSA_TALLQ_CHUNK_MX4 128
#endif
#ifndef NSA_TALLQ_CHUNK_Q8
#define NSA_TALLQ_CHUNK_Q8 256
#endif

namespace {

constexpr int TQ_MAX_ROWS = 128;  // RB = 3 and 4 only: the image of more rows at these chunks outgrows the LDS

// the converts of decode_mx4.hip and decode_q8.hip (their file-local helpers, repeated here)
typedef __bf16 tq_bf16x2 __attribute__((ext_vector_type(2)));

// dword d (8 nibbles, k order) times the scale -> one MFMA fragment
__device__ __forceinline__ bf16x8 mx_frag(uint32_t d, float s) {
  const tq_bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0);
  const tq_bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
  const tq_bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2);
  const tq_bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
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

// One weight format: P k per 16-byte piece, NF MFMAs per piece, RG pieces per split granule, STREAM32 bytes of
// weights (scales included) per 32 k of a row
struct TqMx4 {
  static constexpr int P = 32, NF = 4, RG = 1, STREAM32 = 17, CHUNK = NSA_TALLQ_CHUNK_MX4;
  static constexpr bool BLOCK_SCALE = true;
  // a piece's dequantizing factor: the E8M0 byte e as the fp32 2^(e - 127)
  static __device__ __forceinline__ float factor(uint32_t e) { return __uint_as_float(e << 23); }
  static __device__ __forceinline__ bf16x8 frag(const uint32_t (&d)[4], int s, float f) { return mx_frag(d[s], f); }
};
struct TqQ8 {
  static constexpr int P = 16, NF = 2, RG = 4, STREAM32 = 32, CHUNK = NSA_TALLQ_CHUNK_Q8;
  static constexpr bool BLOCK_SCALE = false;
  static __device__ __forceinline__ float factor(uint32_t) { return 1.0f; }
  static __device__ __forceinline__ bf16x8 frag(const uint32_t (&d)[4], int s, float) {
    return q8frag(d[2 * s], d[2 * s + 1]);
  }
};
static_assert((TqMx4::CHUNK == 64 || TqMx4::CHUNK == 128 || TqMx4::CHUNK == 256) &&
                  (TqQ8::CHUNK == 64 || TqQ8::CHUNK == 128 || TqQ8::CHUNK == 256),
              "a chunk is whole units of 2 P k, its rows shared out among 256 threads, its image within the LDS");

int tq_tiles(int N) { return (N + TALL_TILE_N - 1) / TALL_TILE_N; }
int tq_row_blocks(int rows) { return rows <= 96 ? 3 : 4; }

template <typename F>
constexpr int tq_granule() {  // k per split granule: what K must be a multiple of
  return F::P * F::RG;
}

// tall_ksplit_rule (decode_tall.hip) with F's bytes in the stream term: rounds x 32-wide units per workgroup x one
// unit of a tile's weights on each of TALL_SLOTS CUs, against KS x the fp32 partials written and read back, times
// TALL_PART_WEIGHT.  The smallest cost wins, the smaller split on a tie; at least TALL_MIN_UNITS units per workgroup.
template <typename F>
int tq_ksplit_rule(int rows, int N, int K) {
  const int tiles = tq_tiles(N), U = K / 32;
  if (tiles > TALL_MAX_SPLIT_TILES) return 1;
  const int64_t unit = (int64_t)TALL_SLOTS * TALL_TILE_N * F::STREAM32;
  const int64_t part = 2 * TALL_PART_WEIGHT * (int64_t)tiles * 32 * tq_row_blocks(rows) * TALL_TILE_N * sizeof(float);
  int best = 1;
  int64_t best_cost = INT64_MAX;
  for (int ks = 1; ks <= std::max(1, std::min(U / TALL_MIN_UNITS, TALL_MAX_KS)); ++ks) {
    const int64_t rounds = ((int64_t)tiles * ks + TALL_SLOTS - 1) / TALL_SLOTS;
    const int64_t cost = rounds * ((U + ks - 1) / ks) * unit + (ks > 1 ? ks * part : 0);
    if (cost < best_cost) best = ks, best_cost = cost;
  }
  return best;  // at most U / 8 <= K / granule
}

constexpr int64_t TQ_COUNTER_BYTES = (int64_t)TALL_MAX_SPLIT_TILES * sizeof(int);

template <typename F>
bool tq_shape_ok(int rows, int N, int K) {
  return rows >= 1 && rows <= TQ_MAX_ROWS && N >= 1 && K >= tq_granule<F>() && K % tq_granule<F>() == 0;
}

int64_t tq_ws_bytes(int rows, int N, int ks) {
  if (ks <= 1) return 0;
  return TQ_COUNTER_BYTES + (int64_t)tq_tiles(N) * ks * 4 * tq_row_blocks(rows) * 4 * 64 * sizeof(f32x4);
}

// VEC: N % 4 == 0 and y aligned for 4 columns at a time (the tall kernel's stores); otherwise column by column
template <typename F, int RB, int ACT, bool OUTF>
__global__ __launch_bounds__(256) void tall_q_gemm_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ Wq,
                                                          const void* __restrict__ scale,
                                                          const bf16_t* __restrict__ bias, void* __restrict__ yv,
                                                          int M, int N, int K, int KS, int vec, int* counters,
                                                          f32x4* parts) {
  constexpr int P = F::P, NF = F::NF, CH = F::CHUNK;
  constexpr int ROWS = 32 * RB, KP = CH + 8;  // KP: padded row of the LDS image
  constexpr int CP = CH / P, UN = CP / 2;     // pieces per chunk; weight loads in flight per lane
  constexpr int XC = CH / 8, XR = 256 / XC;   // 16-byte pieces of a chunk row; rows the threads stage per pass
  constexpr int XV = ROWS / XR;               // 16-byte pieces of a chunk per thread
  constexpr int STEPS = UN * NF;              // MFMA steps of a chunk, each on every row block
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [2][ROWS][KP]
  __shared__ int ticket;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const int tile = blockIdx.x, ks = blockIdx.y;
  const int n0 = tile * TALL_TILE_N + 32 * w;
  const bool live = n0 < N;  // wave-uniform: a wave past N only helps staging X
  const int G = K / (P * F::RG);
  const int p_lo = F::RG * (int)((int64_t)G * ks / KS), p_hi = F::RG * (int)((int64_t)G * (ks + 1) / KS);
  const int64_t nrow = min(n0 + c, N - 1);
  const uint8_t* wrow = Wq + nrow * (F::BLOCK_SCALE ? K / 2 : K);
  const uint8_t* srow = reinterpret_cast<const uint8_t*>(scale) + nrow * (K / 32);  // mx4 only
  // staging: piece e = tid + 256 i of a chunk is row e / XC, k offset 8 (e % XC)
  const int xr = tid / XC, xc = tid % XC;
  const bf16_t* xcol = x + 8 * xc;

  // pieces past p_hi: the weight dwords are zero (the range's last piece re-read, branch-free) and X's
  // pieces are zeros
  auto load_a = [&](int p0, uint4 (&dst)[UN], uint32_t (&e)[UN]) {
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int p = p0 + 2 * j + h;
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
      if (in) dst[i] = *reinterpret_cast<const uint4*>(xcol + (int64_t)min(xr + XR * i, M - 1) * K + P * p0);
    }
  };
  auto store_x = [&](int buf, const uint4 (&src)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; ++i)
      *reinterpret_cast<uint4*>(xs + buf * ROWS * KP + (xr + XR * i) * KP + 8 * xc) = src[i];
  };

  f32x16 acc[RB];
#pragma unroll
  for (int t = 0; t < RB; ++t) acc[t] = f32x16{};
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
      const bf16_t* xb = xs + buf * ROWS * KP + c * KP + P * h;
      // step st: unit st / NF, its MFMA st % NF (k offset 2 P (st / NF) + P h + 8 (st % NF)) on every row block.
      // One wave per SIMD: nobody else hides the LDS latency or the converts, so the RB X fragments and the
      // weight fragment of step st + 1 are made before and among the MFMAs of step st; the scheduling barriers
      // keep the compiler from sinking them back to their use.
      auto frags = [&](int st, uint4 (&dst)[RB]) {
#pragma unroll
        for (int t = 0; t < RB; ++t)
          dst[t] = *reinterpret_cast<const uint4*>(xb + 32 * t * KP + 2 * P * (st / NF) + 8 * (st % NF));
      };
      auto wfrag = [&](int st) {
        const uint4 v = a[st / NF];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
        return F::frag(d, st % NF, F::factor(ae[st / NF]));
      };
      uint4 b[RB], bn[RB];
      frags(0, b);
      bf16x8 af = wfrag(0), afn = af;
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        if (st + 1 < STEPS) frags(st + 1, bn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RB; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(bf16x8, b[t]), acc[t], 0, 0, 0);
          if (t == 0 && st + 1 < STEPS) afn = wfrag(st + 1);  // VALU in the shadow of the MFMAs
        }
        __builtin_amdgcn_sched_barrier(0);
        af = afn;
#pragma unroll
        for (int t = 0; t < RB; ++t) b[t] = bn[t];
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
    // quarter q of block t: accumulator elements 4 q .. 4 q + 3
    f32x4* mine = parts + (((int64_t)tile * KS + ks) * 4 + w) * RB * 4 * 64 + lane;
    if (live) {
#pragma unroll
      for (int t = 0; t < RB; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          mine[(4 * t + q) * 64] = f32x4{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
    }
    // the barrier orders the four waves' stores before thread 0, whose agent-scope release fence makes the
    // whole partial visible to the device before the ticket is taken
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      ticket = atomicAdd(counters + tile, 1);
    }
    __syncthreads();
    if (ticket != KS - 1) return;
    __threadfence();  // acquire: the last one in sees every earlier partial
    if (live) {
      const f32x4* p = parts + ((int64_t)tile * KS * 4 + w) * RB * 4 * 64 + lane;
#pragma unroll
      for (int t = 0; t < RB; ++t) acc[t] = f32x16{};
      for (int s = 0; s < KS; ++s, p += 4 * RB * 4 * 64) {
#pragma unroll
        for (int t = 0; t < RB; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 v = p[(4 * t + q) * 64];
            // the first partial is taken as it is (0 + v would turn -0 into +0)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][4 * q + i] = s ? acc[t][4 * q + i] + v[i] : v[i];
          }
      }
    }
    if (tid == 0) counters[tile] = 0;  // for the next launch on this stream
  }
  if (!live) return;
  // C layout: lane l holds batch row m = 32 t + (l & 31), output columns n0 + 8 q + 4 (l >> 5) + i
  // in accumulator element 4 q + i
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + 8 * q + 4 * h;
    if (n >= N) continue;
    // the group's row scales and biases, once for every row block; columns past N read column N - 1's
    float sc[4], bi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nn = min(n + i, N - 1);
      sc[i] = F::BLOCK_SCALE ? 1.0f : reinterpret_cast<const float*>(scale)[nn];
      bi[i] = bias ? bf2f(bias[nn]) : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < RB; ++t) {
      const int m = 32 * t + c;
      if (m >= M) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[t][4 * q + i];
        if constexpr (!F::BLOCK_SCALE) v[i] *= sc[i];
        if (bias) v[i] += bi[i];
        if constexpr (ACT == 1) v[i] = nsa_gelu(v[i]);
      }
      const int64_t o = (int64_t)m * N + n;
      if (vec) {  // kernel-uniform
        if constexpr (OUTF) {
          *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(yv) + o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
          const uint2 pk{(uint32_t)f2bf(v[0]) | (uint32_t)f2bf(v[1]) << 16,
                         (uint32_t)f2bf(v[2]) | (uint32_t)f2bf(v[3]) << 16};
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(yv) + o) = pk;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (n + i >= N) continue;
          if constexpr (OUTF)
            reinterpret_cast<float*>(yv)[o + i] = v[i];
          else
            reinterpret_cast<bf16_t*>(yv)[o + i] = f2bf(v[i]);
        }
      }
    }
  }
}

template <typename F, int RB, int ACT, bool OUTF>
hipError_t tq_launch(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int rows, int N,
                     int K, int ks, void* ws, hipStream_t s) {
  constexpr int lds = 2 * 32 * RB * (F::CHUNK + 8) * (int)sizeof(bf16_t);
  static bool attr = [] {  // dynamic LDS above 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&tall_q_gemm_kernel<F, RB, ACT, OUTF>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  }();
  if (!attr) return hipErrorInvalidValue;
  const int tiles = tq_tiles(N);
  const int vec = N % 4 == 0 && (uintptr_t)y % (OUTF ? 16 : 8) == 0;
  tall_q_gemm_kernel<F, RB, ACT, OUTF><<<dim3(tiles, ks), 256, lds, s>>>(
      (const bf16_t*)x, (const uint8_t*)Wq, scale, (const bf16_t*)bias, y, rows, N, K, ks, vec, (int*)ws,
      (f32x4*)((char*)ws + TQ_COUNTER_BYTES));
  return hipGetLastError();
}

// the guards of nsa_wide_gemm_q8 / _mx4 and the tall kernel's tile limit on a split, then the launch
template <typename F>
hipError_t tq_gemm(const void* x, const void* Wq, const void* scale, const void* bias, void* y, int rows, int N, int K,
                   int act, int out_f32, int ksplit, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (!tq_shape_ok<F>(rows, N, K) || (act && out_f32) || ksplit < 0 || ksplit > K / tq_granule<F>() || ksplit > 65535)
    return hipErrorInvalidValue;
  const int ks = ksplit ? ksplit : tq_ksplit_rule<F>(rows, N, K);
  if (ks > 1 && tq_tiles(N) > TALL_MAX_SPLIT_TILES) return hipErrorInvalidValue;
  if (ks > 1 && (!ws || (uintptr_t)ws % 16 || ws_bytes < tq_ws_bytes(rows, N, ks))) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto launch = [&](auto RB) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      e = tq_launch<F, decltype(RB)::value, decltype(ACT)::value, decltype(OUTF)::value>(x, Wq, scale, bias, y, rows,
                                                                                         N, K, ks, ws, s);
    });
  };
  if (tq_row_blocks(rows) == 3)
    launch(int_c<3>{});
  else
    launch(int_c<4>{});
  return e;
}

template <typename F>
int64_t tq_ws_query(int rows, int N, int K, int ksplit) {
  if (!tq_shape_ok<F>(rows, N, K) || ksplit < 0) return 0;
  return tq_ws_bytes(rows, N, ksplit ? ksplit : tq_ksplit_rule<F>(rows, N, K));
}

}  // namespace

// The split the fixed rule picks for a shape (what ksplit = 0 means); 0 for a shape the kernel refuses
NSA_API int nsa_tall_gemm_mx4_ksplit(int rows, int N, int K) {
  return tq_shape_ok<TqMx4>(rows, N, K) ? tq_ksplit_rule<TqMx4>(rows, N, K) : 0;
}
NSA_API int nsa_tall_gemm_q8_ksplit(int rows, int N, int K) {
  return tq_shape_ok<TqQ8>(rows, N, K) ? tq_ksplit_rule<TqQ8>(rows, N, K) : 0;
}

// Bytes of workspace a launch with this ksplit needs (0: the rule's split); 0 when it uses none
NSA_API int64_t nsa_tall_gemm_mx4_ws_bytes(int rows, int N, int K, int ksplit) {
  return tq_ws_query<TqMx4>(rows, N, K, ksplit);
}
NSA_API int64_t nsa_tall_gemm_q8_ws_bytes(int rows, int N, int K, int ksplit) {
  return tq_ws_query<TqQ8>(rows, N, K, ksplit);
}

// k per LDS chunk of X, as built (ops/functional.py mirrors the defaults)
NSA_API int nsa_tall_gemm_mx4_chunk() { return TqMx4::CHUNK; }
NSA_API int nsa_tall_gemm_q8_chunk() { return TqQ8::CHUNK; }

// y[rows, N] = act(x[rows, K] W[N, K]^T + b) for 1 <= rows <= 128, any N, K % 32 == 0; Wq the nibble matrix
// [N, K / 2], scale the E8M0 bytes [N, K / 32]; bias may be NULL, act 1: exact-erf GELU, out_f32: fp32 y.
// ksplit: workgroups along K (0: the rule's; at most K / 32, and 1 above TALL_MAX_SPLIT_TILES column tiles).
// ws: the workspace of ws_bytes (16-byte aligned, its counters zero; every launch leaves them zero), needed when
// the split is above 1; it is this entry's own, laid out as nsa_tall_gemm's.
NSA_API hipError_t nsa_tall_gemm_mx4(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                     int rows, int N, int K, int act, int out_f32, int ksplit, void* ws,
                                     int64_t ws_bytes, hipStream_t s) {
  return tq_gemm<TqMx4>(x, Wq, scale, bias, y, rows, N, K, act, out_f32, ksplit, ws, ws_bytes, s);
}

// The same with int8 weights Wq [N, K] and one fp32 scale per output column, scale [N]: any N, K % 64 == 0,
// ksplit at most K / 64
NSA_API hipError_t nsa_tall_gemm_q8(const void* x, const void* Wq, const void* scale, const void* bias, void* y,
                                    int rows, int N, int K, int act, int out_f32, int ksplit, void* ws,
                                    int64_t ws_bytes, hipStream_t s) {
  return tq_gemm<TqQ8>(x, Wq, scale, bias, y, rows, N, K, act, out_f32, ksplit, ws, ws_bytes, s);
}
