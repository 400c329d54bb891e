// Decode linear for 17 .. 64 rows: y[rows, N] = act(x[rows, K] W[N, K]^T + bias), bf16, with
// the layouts and epilogues of nsa_skinny_gemm (decode.hip).
//
// The skinny kernel's workgroup owns 16 output columns, so at 64 rows each of its N / 16
// workgroups reads the whole X[64, K] from L2: four times the weight bytes in activation
// loads.  Here a workgroup owns all rows and WIDE_TILE_N = 64 columns, one wave per column
// group of 16, so X traffic equals the weight bytes:
//
//   X     staged once per workgroup through LDS in chunks of WIDE_CHUNK = 256 k (8 units of 32),
//         double-buffered: plain 16-byte global loads of chunk i + 1 are in flight while chunk i
//         is multiplied, and land in the other buffer behind one barrier per chunk.  The image is
//         [16 MT][WIDE_CHUNK + 8] bf16: with the 8-element pad the B fragment's ds_read_b128 (lane
//         l: row l & 15, k offset 8 (l >> 4)) is conflict-free, as in skinny_ln_gemm_kernel.  All
//         four waves read their B fragments from that one image.
//   W     straight to registers as the A operand of v_mfma_f32_16x16x32_bf16 (lane l: weight row
//         n0 + (l & 15), 16 contiguous bytes of it), the next chunk's 8 loads per lane issued
//         before the current chunk's MFMAs.  No weight byte is read by two waves.
//   K     split across workgroups: grid = (column tiles) x KS, workgroup (tile, ks) takes the units
//         U ks / KS .. U (ks + 1) / KS - 1 (U = K / 32; uneven ranges, partial last chunk).  KS is a
//         fixed rule of the shape (wide_ksplit_rule), 1 where the tiles alone fill the machine.
//
// KS = 1 writes y from the accumulators.  KS > 1: the workgroup writes its fp32 partial tile to
// the workspace, fences (agent-scope release: the L2s of the XCDs are not coherent among each
// other without it), and one thread takes a ticket on the tile's counter.  The workgroup that
// draws the last ticket fences (acquire), sums the KS partials in the order 0 .. KS - 1 (its own
// read back like the rest, so the bits do not depend on who came last), applies the epilogue,
// stores y and puts the counter back to 0.  Nobody waits for anybody, and no fp32 atomic touches y.
//
// Workspace: [counters: int per tile, 256-byte padded, zero between launches][partials: per
// (tile, ks, wave, row group) 64 lanes x f32x4 in the accumulator layout].
#include "decode_rows.h"

namespace {

constexpr int WIDE_UNITS = WIDE_CHUNK / 32;  // 32-wide K units per chunk: weight loads in flight per lane
constexpr int WIDE_KP = WIDE_CHUNK + 8;      // padded row of the LDS image

int wide_tiles(int N) { return (N + WIDE_TILE_N - 1) / WIDE_TILE_N; }

// The split of K: up to WIDE_TARGET_WGS workgroups, each with at least WIDE_MIN_UNITS units.  A split
// pays a release fence (an L2 write-back) per workgroup and the partials' round trip, so it is for
// the long-K, few-tile shapes only (mlp.c_proj); measured per shape by scripts/skinny_bench.py --ksplits.
int wide_ksplit_rule(int N, int K) {
  const int ks = std::min(WIDE_TARGET_WGS / wide_tiles(N), K / 32 / WIDE_MIN_UNITS);
  return std::max(ks, 1);
}

constexpr int64_t wide_counter_bytes(int tiles) { return ((int64_t)tiles * 4 + 255) / 256 * 256; }

bool wide_shape_ok(int rows, int N, int K) {
  return rows >= 1 && rows <= WIDE_MAX_ROWS && N >= 16 && N % 16 == 0 && K >= SKINNY_K_BF16 && K % SKINNY_K_BF16 == 0;
}

int64_t wide_ws_bytes(int rows, int N, int K, int ks) {
  if (ks <= 1) return 0;
  const int mt = rows <= 32 ? 2 : 4;
  return wide_counter_bytes(wide_tiles(N)) + (int64_t)wide_tiles(N) * ks * 4 * mt * 64 * sizeof(f32x4);
}

template <int MT, int ACT, bool OUTF>
__global__ __launch_bounds__(256) void wide_gemm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                        const bf16_t* __restrict__ bias, void* __restrict__ yv, int M,
                                                        int N, int K, int KS, int* counters, f32x4* parts) {
  constexpr int ROWS = 16 * MT;
  constexpr int XV = ROWS * (WIDE_CHUNK / 8) / 256;  // 16-byte pieces of a chunk per thread
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [2][ROWS][WIDE_KP]
  __shared__ int ticket;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int tile = blockIdx.x, ks = blockIdx.y;
  const int n0 = tile * WIDE_TILE_N + 16 * w;
  const bool live = n0 < N;  // wave-uniform: a column group past N only helps staging X
  const int U = K / 32;
  const int u_lo = (int)((int64_t)U * ks / KS), u_hi = (int)((int64_t)U * (ks + 1) / KS);
  const bf16_t* wrow = W + (int64_t)(live ? n0 + c : 0) * K + 8 * g;
  // staging: piece e = tid + 256 i of a chunk is row e / 32, k offset 8 (e % 32)
  const int xr = tid >> 5, xc = tid & 31;
  const bf16_t* xsrc[XV];
#pragma unroll
  for (int i = 0; i < XV; ++i) xsrc[i] = x + (int64_t)min(xr + 8 * i, M - 1) * K + 8 * xc;

  // units past u_hi: the weight fragment is zero (the last unit re-read, branch-free) and X's
  // pieces are zeros, so the LDS image is always finite and every MFMA of a chunk runs
  auto load_a = [&](int u0, uint4 (&dst)[WIDE_UNITS]) {
#pragma unroll
    for (int j = 0; j < WIDE_UNITS; ++j) {
      const int uu = u0 + j;
      dst[j] = *reinterpret_cast<const uint4*>(wrow + 32 * (uu < u_hi ? uu : u_hi - 1));
      if (uu >= u_hi) dst[j] = uint4{0u, 0u, 0u, 0u};
    }
  };
  auto load_x = [&](int u0, uint4 (&dst)[XV]) {
    const bool in = 32 * u0 + 8 * xc < 32 * u_hi;
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      dst[i] = uint4{0u, 0u, 0u, 0u};
      if (in) dst[i] = *reinterpret_cast<const uint4*>(xsrc[i] + 32 * u0);
    }
  };
  auto store_x = [&](int buf, const uint4 (&src)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; ++i)
      *reinterpret_cast<uint4*>(xs + buf * ROWS * WIDE_KP + (xr + 8 * i) * WIDE_KP + 8 * xc) = src[i];
  };

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{};
  uint4 a[WIDE_UNITS], xq[XV];
  if (live) load_a(u_lo, a);
  load_x(u_lo, xq);
  store_x(0, xq);
  __syncthreads();
  int buf = 0;
  for (int u0 = u_lo; u0 < u_hi; u0 += WIDE_UNITS, buf ^= 1) {
    const bool more = u0 + WIDE_UNITS < u_hi;  // workgroup-uniform
    uint4 an[WIDE_UNITS];
    if (more) {
      if (live) load_a(u0 + WIDE_UNITS, an);
      load_x(u0 + WIDE_UNITS, xq);
    }
    if (live) {
      const bf16_t* xb = xs + buf * ROWS * WIDE_KP + c * WIDE_KP + 8 * g;
#pragma unroll
      for (int j = 0; j < WIDE_UNITS; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const uint4 b = *reinterpret_cast<const uint4*>(xb + 16 * t * WIDE_KP + 32 * j);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[j]),
                                                           __builtin_bit_cast(bf16x8, b), acc[t], 0, 0, 0);
        }
    }
    if (more) {
      // the other buffer was last read before the barrier that ended the previous chunk
      store_x(buf ^ 1, xq);
      if (live) {
#pragma unroll
        for (int j = 0; j < WIDE_UNITS; ++j) a[j] = an[j];
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
    // the barrier orders the four waves' stores before thread 0, whose agent-scope release fence (one L2
    // write-back per workgroup instead of one per wave: the fences are what a split costs) makes
    // the whole partial visible to the device before the ticket is
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
      float v = acc[t][i];
      if (bias) v += bf2f(bias[n]);
      if constexpr (ACT == 1) v = nsa_gelu(v);
      if constexpr (OUTF)
        reinterpret_cast<float*>(yv)[(int64_t)m * N + n] = v;
      else
        reinterpret_cast<bf16_t*>(yv)[(int64_t)m * N + n] = f2bf(v);
    }
  }
}

template <int MT, int ACT, bool OUTF>
hipError_t wide_launch(const void* x, const void* W, const void* bias, void* y, int rows, int N, int K, int ks,
                       void* ws, hipStream_t s) {
  constexpr int lds = 2 * 16 * MT * WIDE_KP * (int)sizeof(bf16_t);
  static bool attr = [] {  // MT = 4: dynamic LDS above 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&wide_gemm_kernel<MT, ACT, OUTF>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  }();
  if (!attr) return hipErrorInvalidValue;
  const int tiles = wide_tiles(N);
  wide_gemm_kernel<MT, ACT, OUTF><<<dim3(tiles, ks), 256, lds, s>>>(
      (const bf16_t*)x, (const bf16_t*)W, (const bf16_t*)bias, y, rows, N, K, ks, (int*)ws,
      (f32x4*)((char*)ws + wide_counter_bytes(tiles)));
  return hipGetLastError();
}

}  // namespace

// The split the fixed rule picks for a shape (what ksplit = 0 means); 0 for a shape the kernel refuses
NSA_API int nsa_wide_gemm_ksplit(int rows, int N, int K) {
  return wide_shape_ok(rows, N, K) ? wide_ksplit_rule(N, K) : 0;
}

// Bytes of workspace a launch with this ksplit needs (0: the rule's split); 0 when it uses none
NSA_API int64_t nsa_wide_gemm_ws_bytes(int rows, int N, int K, int ksplit) {
  if (!wide_shape_ok(rows, N, K) || ksplit < 0) return 0;
  return wide_ws_bytes(rows, N, K, ksplit ? ksplit : wide_ksplit_rule(N, K));
}

// y[rows, N] = act(x[rows, K] W[N, K]^T + b) for 1 <= rows <= 64, N % 16 == 0, K % 32 == 0; bias may
// be NULL, act 1: exact-erf GELU, out_f32: fp32 y.  ksplit: workgroups along K (0: the rule's;
// at most K / 32).  ws: the workspace of ws_bytes (16-byte aligned, its counters zero; every launch
// leaves them zero), needed when the split is above 1; launches on one stream may share it.
NSA_API hipError_t nsa_wide_gemm(const void* x, const void* W, const void* bias, void* y, int rows, int N, int K,
                                 int act, int out_f32, int ksplit, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (!wide_shape_ok(rows, N, K) || (act && out_f32) || ksplit < 0 || ksplit > K / 32 || ksplit > 65535)
    return hipErrorInvalidValue;
  const int ks = ksplit ? ksplit : wide_ksplit_rule(N, K);
  if (ks > 1 && (!ws || (uintptr_t)ws % 16 || ws_bytes < wide_ws_bytes(rows, N, K, ks))) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto launch = [&](auto MT) {
    epilogue_dispatch(act, out_f32, [&](auto ACT, auto OUTF) {
      e = wide_launch<decltype(MT)::value, decltype(ACT)::value, decltype(OUTF)::value>(x, W, bias, y, rows, N, K,
                                                                                        ks, ws, s);
    });
  };
  if (rows <= 32)
    launch(int_c<2>{});
  else
    launch(int_c<4>{});
  return e;
}
