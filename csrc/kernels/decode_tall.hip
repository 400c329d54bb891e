// Decode linear for 65 .. 256 rows: y[rows, N] = act(x[rows, K] W[N, K]^T + bias), bf16, with the
// layouts, epilogues and refusals of nsa_wide_gemm (decode_wide.hip).
//
// The wide kernel's 16-column waves read one 1 KB B fragment from LDS per 16x16x32 MFMA (8 K MACs),
// and its double-buffered image of X outgrows the LDS above 64 rows.  Here a workgroup still owns
// all rows of its column tile, so no weight byte leaves HBM twice, but the tile is TALL_TILE_N = 128
// columns, one wave per 32, on v_mfma_f32_32x32x16_bf16: one 1 KB fragment read feeds 16 K MACs.
//
//   rows  instantiated by blocks of 32: RB = 3 / 4 / 6 / 8 (96 / 128 / 192 / 256 rows), 16 fp32
//         accumulators per lane and block.  Rows past `rows` in the last block are clamped reads
//         (row rows - 1 again) and are never stored.
//   X     staged once per workgroup through LDS in chunks of TALL_CHUNK = 128 k (4 units of 32),
//         double-buffered: 16-byte global loads of chunk i + 1 are in flight while chunk i is
//         multiplied, and land in the other buffer behind one barrier per chunk.  The image is
//         [32 RB][TALL_CHUNK + 8] bf16 (139 KB for both buffers at 256 rows): a row is 68 dwords,
//         so the 16 rows of one ds_read_b128 pass start 4 banks apart and cover the 64 banks once.
//   W     straight to registers as the A operand: lane l holds weight row n0 + (l & 31) and, of
//         every 32-wide unit, the 32 contiguous bytes k = 16 (l >> 5) .. + 15 as two 16-byte
//         loads; the two lanes of a row cover the unit's 64 bytes and the chunk's 8 loads in
//         flight 256 contiguous bytes of the row.  The MFMA wants k = 8 (l >> 5) .. + 7 per lane,
//         so K is permuted inside a unit: MFMA s (0, 1) of unit u multiplies k = 32 u + 16 (l >> 5)
//         + 8 s .. + 7, and the B fragment is read from the image at that same offset.  The next
//         chunk's loads are issued before the current chunk's MFMAs.
//   K     split across workgroups exactly as in the wide kernel: grid = (column tiles) x KS,
//         workgroup (tile, ks) takes the units U ks / KS .. U (ks + 1) / KS - 1.
//
// KS = 1 writes y from the accumulators.  KS > 1: fp32 partial tiles go to the workspace, thread 0
// fences (agent-scope release) and takes one ticket on the tile's counter; the workgroup that
// draws the last ticket fences (acquire), sums the KS partials in the order 0 .. KS - 1 (its own
// read back like the rest: the bits do not depend on who came last), applies the epilogue, stores
// y and puts the counter back to 0.  Nobody waits for anybody, and no fp32 atomic touches y.
//
// The partials grow with the rows (256 rows x 4800 columns x 4 B x KS passes c_attn's weights at
// KS = 2), so the split rule (tall_ksplit_rule) weighs their round trip against idle CUs.
//
// Workspace: [counters: TALL_MAX_SPLIT_TILES ints, zero between launches][partials: per (tile, ks,
// wave, row block, quarter) 64 lanes x f32x4 in the accumulator layout].  The counter region has one
// size for every shape, so the partials of one launch never land on the counters of another that
// shares the buffer; a shape with more tiles is not split (the rule gives 1, the entry refuses more).
//
// Occupancy: RB = 3 / 4 take 138 - 162 VGPRs and 52 / 70 KB of LDS, so two workgroups fit a CU at up
// to 128 rows; RB = 6 / 8 (104 / 139 KB, 256 VGPRs + 128 AGPRs at RB = 8) run one per CU.  The split
// rule counts one slot per CU at every row count.
#include "decode_rows.h"

namespace {

constexpr int TALL_UNITS = TALL_CHUNK / 32;  // 32-wide K units per chunk
constexpr int TALL_KP = TALL_CHUNK + 8;      // padded row of the LDS image

int tall_tiles(int N) { return (N + TALL_TILE_N - 1) / TALL_TILE_N; }
int tall_row_blocks(int rows) { return rows <= 96 ? 3 : rows <= 128 ? 4 : rows <= 192 ? 6 : 8; }

// The split of K, a fixed function of the shape.  Cost of a split in bytes the whole machine moves:
//   stream    rounds x units per workgroup x one unit of a tile's weights on each of TALL_SLOTS CUs
//             (a workgroup streams at a CU's share of the machine; rounds = workgroups / TALL_SLOTS, up)
//   partials  KS x (tiles x 32 RB x TALL_TILE_N fp32), written and read back, from KS = 2, times
//             TALL_PART_WEIGHT: they pass a release fence, and one workgroup per tile reads them all back
//             (the weight is what scripts/skinny_bench.py --ksplits measured at the GPT-2 shapes)
// The smallest cost wins, the smaller split on a tie; at least TALL_MIN_UNITS units per workgroup.
int tall_ksplit_rule(int rows, int N, int K) {
  const int tiles = tall_tiles(N), U = K / 32;
  if (tiles > TALL_MAX_SPLIT_TILES) return 1;
  const int64_t unit = (int64_t)TALL_SLOTS * TALL_TILE_N * 32 * sizeof(bf16_t);
  const int64_t part = 2 * TALL_PART_WEIGHT * (int64_t)tiles * 32 * tall_row_blocks(rows) * TALL_TILE_N * sizeof(float);
  int best = 1;
  int64_t best_cost = INT64_MAX;
  for (int ks = 1; ks <= std::max(1, std::min(U / TALL_MIN_UNITS, TALL_MAX_KS)); ++ks) {
    const int64_t rounds = ((int64_t)tiles * ks + TALL_SLOTS - 1) / TALL_SLOTS;
    const int64_t cost = rounds * ((U + ks - 1) / ks) * unit + (ks > 1 ? ks * part : 0);
    if (cost < best_cost) best = ks, best_cost = cost;
  }
  return best;
}

constexpr int64_t TALL_COUNTER_BYTES = (int64_t)TALL_MAX_SPLIT_TILES * sizeof(int);

bool tall_shape_ok(int rows, int N, int K) {
  return rows >= 1 && rows <= TALL_MAX_ROWS && N >= 16 && N % 16 == 0 && K >= SKINNY_K_BF16 && K % SKINNY_K_BF16 == 0;
}

int64_t tall_ws_bytes(int rows, int N, int K, int ks) {
  if (ks <= 1) return 0;
  return TALL_COUNTER_BYTES +
         (int64_t)tall_tiles(N) * ks * 4 * tall_row_blocks(rows) * 4 * 64 * sizeof(f32x4);
}

template <int RB, int ACT, bool OUTF>
__global__ __launch_bounds__(256) void tall_gemm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                        const bf16_t* __restrict__ bias, void* __restrict__ yv, int M,
                                                        int N, int K, int KS, int* counters, f32x4* parts) {
  constexpr int ROWS = 32 * RB;
  constexpr int XV = ROWS * (TALL_CHUNK / 8) / 256;  // 16-byte pieces of a chunk per thread
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [2][ROWS][TALL_KP]
  __shared__ int ticket;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const int tile = blockIdx.x, ks = blockIdx.y;
  const int n0 = tile * TALL_TILE_N + 32 * w;
  const bool live = n0 < N;  // wave-uniform: a wave past N only helps staging X
  const int U = K / 32;
  const int u_lo = (int)((int64_t)U * ks / KS), u_hi = (int)((int64_t)U * (ks + 1) / KS);
  // N % 16 == 0: the last live wave may own 16 columns only; its other lanes stream row N - 1 again
  const bf16_t* wrow = W + (int64_t)min(n0 + c, N - 1) * K + 16 * h;
  // staging: piece e = tid + 256 i of a chunk is row e / 16, k offset 8 (e % 16)
  const int xr = tid >> 4, xc = tid & 15;
  const bf16_t* xcol = x + 8 * xc;

  // units past u_hi: the weight fragment is zero (the last unit re-read, branch-free) and X's
  // pieces are zeros, so the LDS image is always finite and every MFMA of a chunk runs
  auto load_a = [&](int u0, uint4 (&dst)[2 * TALL_UNITS]) {
#pragma unroll
    for (int j = 0; j < TALL_UNITS; ++j) {
      const int uu = u0 + j;
      const bf16_t* p = wrow + 32 * (uu < u_hi ? uu : u_hi - 1);
      dst[2 * j] = *reinterpret_cast<const uint4*>(p);
      dst[2 * j + 1] = *reinterpret_cast<const uint4*>(p + 8);
      if (uu >= u_hi) dst[2 * j] = dst[2 * j + 1] = uint4{0u, 0u, 0u, 0u};
    }
  };
  auto load_x = [&](int u0, uint4 (&dst)[XV]) {
    const bool in = u0 + (xc >> 2) < u_hi;
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      dst[i] = uint4{0u, 0u, 0u, 0u};
      if (in) dst[i] = *reinterpret_cast<const uint4*>(xcol + (int64_t)min(xr + 16 * i, M - 1) * K + 32 * u0);
    }
  };
  auto store_x = [&](int buf, const uint4 (&src)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; ++i)
      *reinterpret_cast<uint4*>(xs + buf * ROWS * TALL_KP + (xr + 16 * i) * TALL_KP + 8 * xc) = src[i];
  };

  f32x16 acc[RB];
#pragma unroll
  for (int t = 0; t < RB; ++t) acc[t] = f32x16{};
  uint4 a[2 * TALL_UNITS], xq[XV];
  if (live) load_a(u_lo, a);
  load_x(u_lo, xq);
  store_x(0, xq);
  __syncthreads();
  int buf = 0;
  for (int u0 = u_lo; u0 < u_hi; u0 += TALL_UNITS, buf ^= 1) {
    const bool more = u0 + TALL_UNITS < u_hi;  // workgroup-uniform
    uint4 an[2 * TALL_UNITS];
    if (more) {
      if (live) load_a(u0 + TALL_UNITS, an);
      load_x(u0 + TALL_UNITS, xq);
    }
    if (live) {
      const bf16_t* xb = xs + buf * ROWS * TALL_KP + c * TALL_KP + 16 * h;
      // step j: unit j / 2, its MFMA j % 2 (k offset 32 (j / 2) + 16 h + 8 (j % 2)) on every row block.
      // One wave per SIMD: nobody else hides the LDS latency, so the RB fragments of step j + 1 are
      // read before the MFMAs of step j; the scheduling barriers keep the compiler from sinking each
      // read back to its use.
      auto frags = [&](int j, uint4 (&dst)[RB]) {
#pragma unroll
        for (int t = 0; t < RB; ++t)
          dst[t] = *reinterpret_cast<const uint4*>(xb + 32 * t * TALL_KP + 32 * (j >> 1) + 8 * (j & 1));
      };
      uint4 b[RB], bn[RB];
      frags(0, b);
#pragma unroll
      for (int j = 0; j < 2 * TALL_UNITS; ++j) {
        if (j + 1 < 2 * TALL_UNITS) frags(j + 1, bn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RB; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[j]),
                                                           __builtin_bit_cast(bf16x8, b[t]), acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RB; ++t) b[t] = bn[t];
      }
    }
    if (more) {
      // the other buffer was last read before the barrier that ended the previous chunk
      store_x(buf ^ 1, xq);
      if (live) {
#pragma unroll
        for (int j = 0; j < 2 * TALL_UNITS; ++j) a[j] = an[j];
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
    // the barrier orders the four waves' stores before thread 0, whose agent-scope release fence
    // (one L2 write-back per workgroup) makes the whole partial visible to the device before the
    // ticket is taken
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
  for (int t = 0; t < RB; ++t) {
    const int m = 32 * t + c;
    if (m >= M) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 8 * q + 4 * h;
      if (n >= N) continue;  // whole groups of 4: N % 16 == 0
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[t][4 * q + i];
        if (bias) v[i] += bf2f(bias[n + i]);
        if constexpr (ACT == 1) v[i] = nsa_gelu(v[i]);
      }
      if constexpr (OUTF) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(yv) + (int64_t)m * N + n) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
        const uint2 o{(uint32_t)f2bf(v[0]) | (uint32_t)f2bf(v[1]) << 16, (uint32_t)f2bf(v[2]) | (uint32_t)f2bf(v[3]) << 16};
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(yv) + (int64_t)m * N + n) = o;
      }
    }
  }
}

template <int RB, int ACT, bool OUTF>
hipError_t tall_launch(const void* x, const void* W, const void* bias, void* y, int rows, int N, int K, int ks,
                       void* ws, hipStream_t s) {
  constexpr int lds = 2 * 32 * RB * TALL_KP * (int)sizeof(bf16_t);
  static bool attr = [] {  // RB >= 4: dynamic LDS above 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&tall_gemm_kernel<RB, ACT, OUTF>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  }();
  if (!attr) return hipErrorInvalidValue;
  const int tiles = tall_tiles(N);
  tall_gemm_kernel<RB, ACT, OUTF><<<dim3(tiles, ks), 256, lds, s>>>(
      (const bf16_t*)x, (const bf16_t*)W, (const bf16_t*)bias, y, rows, N, K, ks, (int*)ws,
      (f32x4*)((char*)ws + TALL_COUNTER_BYTES));
  return hipGetLastError();
}

}  // namespace

// The split the fixed rule picks for a shape (what ksplit = 0 means); 0 for a shape the kernel refuses
NSA_API int nsa_tall_gemm_ksplit(int rows, int N, int K) {
  return tall_shape_ok(rows, N, K) ? tall_ksplit_rule(rows, N, K) : 0;
}

// Bytes of workspace a launch with this ksplit needs (0: the rule's split); 0 when it uses none
NSA_API int64_t nsa_tall_gemm_ws_bytes(int rows, int N, int K, int ksplit) {
  if (!tall_shape_ok(rows, N, K) || ksplit < 0) return 0;
  return tall_ws_bytes(rows, N, K, ksplit ? ksplit : tall_ksplit_rule(rows, N, K));
}

// y[rows, N] = act(x[rows, K] W[N, K]^T + b) for 1 <= rows <= 256, N % 16 == 0, K % 32 == 0; the
// arguments, the workspace contract and the refusals of nsa_wide_gemm, and one more: a split above 1
// with more than TALL_MAX_SPLIT_TILES column tiles (N > 131072).  The workspace is the tall kernel's
// own: its counter region is not where the wide kernel's is.  y and bias are read and
// written 4 columns at a time: y 8-byte (bf16) or 16-byte (fp32) aligned, as every allocation is.
NSA_API hipError_t nsa_tall_gemm(const void* x, const void* W, const void* bias, void* y, int rows, int N, int K,
                                 int act, int out_f32, int ksplit, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (!tall_shape_ok(rows, N, K) || (act && out_f32) || ksplit < 0 || ksplit > K / 32 || ksplit > 65535)
    return hipErrorInvalidValue;
  const int ks = ksplit ? ksplit : tall_ksplit_rule(rows, N, K);
  if (ks > 1 && tall_tiles(N) > TALL_MAX_SPLIT_TILES) return hipErrorInvalidValue;
  if (ks > 1 && (!ws || (uintptr_t)ws % 16 || ws_bytes < tall_ws_bytes(rows, N, K, ks))) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto launch = [&](auto RB) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      e = tall_launch<decltype(RB)::value, decltype(ACT)::value, decltype(OUTF)::value>(x, W, bias, y, rows, N, K,
                                                                                        ks, ws, s);
    });
  };
  switch (tall_row_blocks(rows)) {
    case 3: launch(int_c<3>{}); break;
    case 4: launch(int_c<4>{}); break;
    case 6: launch(int_c<6>{}); break;
    default: launch(int_c<8>{});
  }
  return e;
}
