// Decode attention for a speculative step (Decoder(..., speculate=K)): S = K + 1 consecutive
// queries of one sequence against one cache.  qkv is [B, S, 3C]; query j of row b sits at
// position pos[b] + j, its K / V rows are stored at that cache row and it attends over keys
// 0 .. pos[b] + j, the j + 1 new rows of this launch included.
//
// One launch writes flash-decoding partials (m, l, o[64]) in the format of decode_attn.h, one
// per (row, query, head, 256-key chunk), chunks cut at absolute key positions; the combine of
// decode_attn.h, over B * S rows, turns them into the output [B, S, C].  Workgroup (b, h, s)
// fetches the K / V rows of chunk s once (a thread's key row and its 8 x 8 V tile stay in
// registers) and serves all S queries from them.  The new rows p .. p + S - 1 are taken from
// qkv, the bf16 bits this launch stores, never from the cache rows it writes: another
// workgroup may be the writer (decode_attn_chunk does the same with its one row).
//
// Per query the arithmetic is decode_attn_chunk's, operation for operation (the score's fmaf
// chain over the 64 dims, the wave maximum and sum, the 8-key fmaf chain of a V tile, the
// butterfly over a wave's key groups, the four waves summed in order), so output, partials and
// caches equal S successive nsa_decode_attn_rows(append) calls at pos + j bit for bit, and a
// token's attention does not depend on how positions were grouped into steps.  A key past a
// query's position carries p = 0 there as here; the V row it multiplies is the key's own
// (a live cache row or a new row of qkv: finite) where the single-query body reads the row at
// its position, and 0 * finite leaves the sum as it is.
//
// A dead query, pos[b] + j >= Tmax, stores nothing, and its partial of chunk 0 is (m, l, o) =
// (0, 1, 0) with every other chunk empty, so the combine gives it an output row of zeros
// (finite: it feeds the linears and the sampler; the all-empty row would give 0 / 0).
//
// The grid follows (B, S, H, Tmax) only, so a captured step serves every position.
#include "decode_attn.h"

namespace {

// grid (B * H, n_split), 256 threads; partial (b, j, h, s) at ws[(((b S + j) H + h) n_split + s) * 68]
template <int S>
__global__ __launch_bounds__(256) void decode_attn_spec_kernel(const bf16_t* __restrict__ qkv,
                                                               const bf16_t* __restrict__ kc,
                                                               const bf16_t* __restrict__ vc, bf16_t* kc_w,
                                                               bf16_t* vc_w, const int64_t* __restrict__ pos_dev,
                                                               float* __restrict__ ws, int H, int Tmax,
                                                               float scale_log2) {
  __shared__ __attribute__((aligned(16))) float qs[S][DA_D];
  __shared__ __attribute__((aligned(16))) float ps[S][DA_CHUNK];
  __shared__ float red[2][S][4];
  __shared__ float os[S][4][DA_D];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.x, s = blockIdx.y, n_split = gridDim.y;
  const int b = bh / H, hh = bh % H;
  const int C = H * DA_D;
  const int k0 = s * DA_CHUNK;
  // every branch below is on b, s and pos[b]: workgroup-uniform
  const int64_t p64 = pos_dev[b];
  const int p = (int)(p64 < 0 ? 0 : (p64 > Tmax ? Tmax : p64));  // rows at or past Tmax: all queries dead
  const int nlive = min(S, Tmax - p);                            // queries 0 .. nlive - 1 have a cache row
  const int pmax = p + nlive - 1;                                // the newest live key
  const int j0 = max(0, k0 - p);                                 // queries below j0 end before this chunk
  const bf16_t* qb = qkv + (int64_t)b * S * 3 * C + hh * DA_D;   // query j: qb + j * 3C (q | k | v, C apart)
  auto part_of = [&](int j) { return ws + ((((int64_t)b * S + j) * H + hh) * n_split + s) * DA_PART; };
  // the partials this workgroup does not compute: the empty one for a chunk beyond a live
  // query, and for a dead query (0, 1, 0) in chunk 0 (zeros out of the combine), empty elsewhere
  for (int e = tid; e < S * DA_PART; e += 256) {
    const int j = e / DA_PART, i = e % DA_PART;
    if (j < nlive ? j < j0 : true) {
      const bool dead0 = j >= nlive && s == 0;
      part_of(j)[i] = i == 0 ? (dead0 ? 0.0f : -INFINITY) : (i == 1 && dead0 ? 1.0f : 0.0f);
    }
  }
  if (j0 >= nlive) return;  // no live query reaches this chunk
  const int64_t row0 = (int64_t)bh * Tmax;
  // the chunk's loads, issued together: this thread's key row (key k0 + tid; a new row comes
  // from qkv, a key past the newest one reads a valid, unused row) ...
  const int key = k0 + tid;
  const bf16_t* krow = key >= p ? qb + (int64_t)min(key - p, S - 1) * 3 * C + C : kc + (row0 + key) * DA_D;
  uint4 ku[DA_D / 8];
#pragma unroll
  for (int c = 0; c < DA_D / 8; ++c) ku[c] = *reinterpret_cast<const uint4*>(krow + 8 * c);
  // ... and its V tile: keys k0 + 8 kg .. + 7 (clamped to the newest live key), dims 8 dg .. + 7
  const int kg = tid >> 3, dg = tid & 7;
  uint4 vu[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int kk = min(k0 + 8 * kg + i, pmax);
    const bf16_t* vr = kk >= p ? qb + (int64_t)(kk - p) * 3 * C + 2 * C : vc + (row0 + kk) * DA_D;
    vu[i] = *reinterpret_cast<const uint4*>(vr + 8 * dg);
  }
  // the live new rows of this chunk go to the cache for later steps: thread (j, k | v, piece)
  if (tid < S * 16) {
    const int j = tid >> 4, kv = (tid >> 3) & 1, c = tid & 7;
    const int pj = p + j;
    if (j < nlive && pj >= k0 && pj < k0 + DA_CHUNK)
      *reinterpret_cast<uint4*>((kv ? vc_w : kc_w) + (row0 + pj) * DA_D + 8 * c) =
          *reinterpret_cast<const uint4*>(qb + (int64_t)j * 3 * C + (1 + kv) * C + 8 * c);
  }
  for (int e = tid; e < S * DA_D; e += 256) qs[e / DA_D][e % DA_D] = bf2f(qb[(int64_t)(e / DA_D) * 3 * C + e % DA_D]);
  __syncthreads();
  float kf[DA_D];
#pragma unroll
  for (int c = 0; c < DA_D / 8; ++c) {
    float f[8];
    unpack8(ku[c], f);
#pragma unroll
    for (int e = 0; e < 8; ++e) kf[8 * c + e] = f[e];
  }
  // From here to the stores every query is computed, branch-free, so that the S independent
  // chains (dot product, wave reductions, V tile) interleave; a query that does not reach this
  // chunk works on valid, finite rows and is dropped at the stores.
  float sc[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    float acc = 0.0f;
#pragma unroll
    for (int d = 0; d < DA_D; ++d) acc = fmaf(qs[j][d], kf[d], acc);
    sc[j] = key <= p + j ? acc * scale_log2 : -INFINITY;
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const float m = wave_max(sc[j]);
    if (lane == 0) red[0][j][w] = m;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const float m = fmaxf(fmaxf(red[0][j][0], red[0][j][1]), fmaxf(red[0][j][2], red[0][j][3]));
    sc[j] = key <= p + j ? exp2f(sc[j] - m) : 0.0f;
    ps[j][tid] = sc[j];
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const float lw = wave_sum(sc[j]);
    if (lane == 0) red[1][j][w] = lw;
  }
  __syncthreads();
  float vf[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) unpack8(vu[i], vf[i]);
  float o[S][8];
#pragma unroll
  for (int j = 0; j < S; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[j][e] = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float pj = ps[j][8 * kg + i];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[j][e] = fmaf(pj, vf[i][e], o[j][e]);
    }
  }
#pragma unroll
  for (int off = 8; off < 64; off <<= 1)  // the wave's 8 key groups (lane bits 3..5)
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) o[j][e] += __shfl_xor(o[j][e], off, 64);
  if (lane < 8)
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) os[j][w][8 * lane + e] = o[j][e];
  __syncthreads();
  for (int e = tid; e < S * DA_D; e += 256) {
    const int j = e / DA_D, d = e % DA_D;
    if (j >= j0 && j < nlive) part_of(j)[DA_PO + d] = os[j][0][d] + os[j][1][d] + os[j][2][d] + os[j][3][d];
  }
  if (tid < S && tid >= j0 && tid < nlive) {
    float* part = part_of(tid);
    part[0] = fmaxf(fmaxf(red[0][tid][0], red[0][tid][1]), fmaxf(red[0][tid][2], red[0][tid][3]));
    part[1] = red[1][tid][0] + red[1][tid][1] + red[1][tid][2] + red[1][tid][3];
  }
}

template <int S>
hipError_t decode_attn_spec_launch(const void* qkv, void* kc, void* vc, const void* pos, void* ws, void* out, int B,
                                   int H, int Tmax, float scale, hipStream_t s) {
  const int n_split = (Tmax + DA_CHUNK - 1) / DA_CHUNK;
  decode_attn_spec_kernel<S><<<dim3(B * H, n_split), 256, 0, s>>>(
      (const bf16_t*)qkv, (const bf16_t*)kc, (const bf16_t*)vc, (bf16_t*)kc, (bf16_t*)vc, (const int64_t*)pos,
      (float*)ws, H, Tmax, scale * 1.4426950408889634f);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  decode_attn_combine_kernel<<<B * S * H, 64, 0, s>>>((const float*)ws, (bf16_t*)out, H, n_split);
  return hipGetLastError();
}

}  // namespace

// qkv: [B, S, 3C] bf16 (q | k | v), 2 <= S <= 8; kc / vc: bf16 [B, H, Tmax, 64]; pos: int64[B];
// ws: B * S * H * ceil(Tmax / 256) * 68 fp32; out: [B, S, C] bf16.  Query j of row b is at
// position pos[b] + j: its K / V rows are stored there and it attends over keys 0 .. pos[b] + j.
NSA_API hipError_t nsa_decode_attn_spec(const void* qkv, void* kc, void* vc, const void* pos, void* ws, void* out,
                                        int B, int S, int H, int D, int Tmax, float scale, hipStream_t s) {
  if (D != DA_D || B < 1 || H < 1 || Tmax < 1 || !qkv || !kc || !vc || !pos || !ws || !out)
    return hipErrorInvalidValue;
  if ((int64_t)B * H > 0x7fffffffLL / 8 || (Tmax + DA_CHUNK - 1) / DA_CHUNK > 65535) return hipErrorInvalidValue;
  switch (S) {
    case 2: return decode_attn_spec_launch<2>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    case 3: return decode_attn_spec_launch<3>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    case 4: return decode_attn_spec_launch<4>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    case 5: return decode_attn_spec_launch<5>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    case 6: return decode_attn_spec_launch<6>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    case 7: return decode_attn_spec_launch<7>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    case 8: return decode_attn_spec_launch<8>(qkv, kc, vc, pos, ws, out, B, H, Tmax, scale, s);
    default: return hipErrorInvalidValue;
  }
}
