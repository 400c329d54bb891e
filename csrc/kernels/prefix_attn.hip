// Prefill attention of a batch whose rows share a prompt prefix (Decoder.prefill_suffixes): the
// prefix's K / V are cached once, [1, H, Tp, 64] bf16 (rows 0 .. P - 1 live), and every row b
// brings S suffix tokens as packed projections qkv [B, S, 3C].  Query i of row b attends over
// prefix keys 0 .. P - 1 (all visible) followed by its own row's keys 0 .. i from qkv (causal).
// bf16, head dim 64, forward only, no dropout; one launch, no workspace; no input is written.
//
// Decomposition: a workgroup (4 waves) per (row, head, query tile), the key range of the tile,
// P + (last query of the tile) + 1 keys, dealt to the four waves in rounds of 4 x 32 keys (wave
// w, round r: keys 128 r + 32 w .. + 31), each wave keeping a running (m, l, o) per query that
// meet in LDS at the end.  The reason: the shapes this serves are suffixes of 8 - 128 tokens
// after prefixes of up to about 1000, so the long axis is the keys, not the queries.  A
// workgroup per 64-query tile with a wave per 16 queries would leave three waves of four idle
// for a suffix of 8 - 16 tokens and walk ~1000 keys serially in the fourth; dealing the keys
// keeps all four busy for any S and shortens the serial walk fourfold, at the price of one LDS
// merge per tile (68 floats per wave and query).  Not measured against the other form.
// A query tile is 16 queries (the MFMA's 16 columns) for S <= 16 and 32 (two column groups on
// the same K / V fragments) above: every tile reads the prefix's K / V again, from L2 (229 KB
// per tile at P = 896), and the V^T fragments cost 32 16-bit LDS reads per round whatever the
// number of column groups.  Measured at GPT-2 1.5B, batch 64, P = 896, S = 32 (rocprofv3 kernel
// trace, one box): 84.9 us per launch with 16-query tiles only, 77.1 us with 32-query ones (211
// instead of 144 registers, 2 waves per SIMD instead of 3); the flash forward on the 64 x 928
// materialised rows takes 347 us there.  That is about 150 TFLOP/s of useful work, far from the
// matrix cores' roof: the transposing LDS reads, the two barriers per round and the hi + lo P.V
// are what a later pass would attack.
//
// Fragment plan, that of shared_prompt_chunk (decode_shared.hip), with the 16 MFMA columns being
// 16 queries of one row instead of 16 batch rows:
//   S^T[key, q] = K[key, :] . Q[q, :]     v_mfma_f32_16x16x32_bf16, A = K rows straight from
//                                         global memory (prefix cache or qkv), B = Q^T
//   lane l holds the scores of query c = l & 15 against keys 4 (l >> 4) + i of each 16-key tile;
//   online softmax in fp32 on those (block max and sum: registers, then two shuffles);
//   O^T[d, q] = V^T[d, key] . p^T[key, q] A = V^T from LDS (the wave's own 32 rows), B = p as it
//                                         lies in the lanes, entering as hi + lo bf16 (two MFMAs
//                                         on the same A fragment: 16 bits of p)
// A key is one virtual index kk: kk < P is row kk of the prefix cache, kk >= P is token kk - P of
// the row's own qkv, so cache rows at or past P are never addressed.  Keys a query may not see
// (kk > P + i, or past the tile's range) score -inf by select; loads past the range are clamped
// to its last key and their V rows zeroed.  Padding queries are ordinary queries; columns past
// S in the last tile repeat query S - 1 and are not stored.
#include "common.h"

#include <math.h>

namespace {

constexpr int PA_D = 64;    // head dim
constexpr int PA_Q = 16;    // queries per column group: the MFMA's 16 columns
constexpr int PA_KB = 32;   // keys per wave and round: two 16-key tiles
constexpr int PA_VS = 72;   // bf16 elements per V row in LDS: 144 bytes (16-byte aligned rows; the
                            // four rows 4 g of a fragment read fall into different banks)
constexpr int PA_OS = 68;   // floats per o row in LDS

// NT column groups of 16 queries per workgroup.  grid B * H * nqt (nqt = ceil(S / (16 NT))), 256 threads
template <int NT>
__global__ __launch_bounds__(256) void prefix_attn_kernel(const bf16_t* __restrict__ qkv,
                                                          const bf16_t* __restrict__ pk,
                                                          const bf16_t* __restrict__ pv, bf16_t* __restrict__ out,
                                                          int S, int H, int Tp, int P, int nqt, float scale_log2) {
  constexpr int VBYTES = 4 * PA_KB * PA_VS * sizeof(bf16_t), OBYTES = 4 * NT * PA_Q * PA_OS * sizeof(float);
  // V rows of the round, [4 waves][32][PA_VS] bf16; after the last round the waves' o, [4][16 NT][PA_OS] fp32
  __shared__ __attribute__((aligned(16))) unsigned char smem[VBYTES > OBYTES ? VBYTES : OBYTES];
  __shared__ float msm[4][NT * PA_Q];
  __shared__ float lsm[4][NT * PA_Q];
  bf16_t* vsm = reinterpret_cast<bf16_t*>(smem);
  float* osm = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int C = H * PA_D;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int b = bh / H, hh = bh % H;
  const int q0 = qt * (NT * PA_Q);
  const int nq = min(NT * PA_Q, S - q0);  // live queries of this tile (>= 1)
  const int nk = P + q0 + nq;             // keys the tile's last query sees
  const int nround = (nk + 4 * PA_KB - 1) / (4 * PA_KB);
  const bf16_t* pkh = pk + (int64_t)hh * Tp * PA_D;
  const bf16_t* pvh = pv + (int64_t)hh * Tp * PA_D;
  const bf16_t* row0 = qkv + (int64_t)b * S * 3 * C + hh * PA_D;  // q of the row's token 0; k at + C, v at + 2C
  // K (kv = 1) or V (kv = 2) row of virtual key kk, clamped into the tile's range
  auto krow = [&](int kk, int kv) -> const bf16_t* {
    kk = min(kk, nk - 1);
    return kk < P ? (kv == 1 ? pkh : pvh) + (int64_t)kk * PA_D : row0 + (int64_t)(kk - P) * 3 * C + kv * C;
  };
  // Q^T: B fragments per column group (lane: query 16 n + c, dims 32 u + 8 g .. + 7); lim: the
  // last key this lane's query of group n sees
  uint4 qa[NT], qb[NT];
  int lim[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int qi = q0 + min(PA_Q * n + c, nq - 1);
    lim[n] = P + qi;
    const bf16_t* qrow = row0 + (int64_t)qi * 3 * C + 8 * g;
    qa[n] = *reinterpret_cast<const uint4*>(qrow);
    qb[n] = *reinterpret_cast<const uint4*>(qrow + 32);
  }
  // this wave's keys of a round: K as A fragments of the two 16-key tiles (lane: key c of the
  // tile, dims 32 u + 8 g .. + 7) and the 32 V rows, 16 bytes per lane and pass
  uint4 kn[2][2], vn[4];
  auto fetch = [&](int r) {
    const int kw = (4 * r + w) * PA_KB;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16_t* kr = krow(kw + 16 * t + c, 1) + 8 * g;
#pragma unroll
      for (int u = 0; u < 2; ++u) kn[t][u] = *reinterpret_cast<const uint4*>(kr + 32 * u);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = 64 * i + lane, kl = idx >> 3, pc = idx & 7;
      vn[i] = *reinterpret_cast<const uint4*>(krow(kw + kl, 2) + 8 * pc);
    }
  };
  fetch(0);
  float m[NT], l[NT];  // running maximum of query 16 n + c (log2 units) and this lane's share of its sum
  f32x4 o[NT][4];      // O^T: column q = 16 n + c, rows (dims) 16 dt + 4 g + i
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    m[n] = -INFINITY;
    l[n] = 0.0f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[n][dt] = f32x4{};
  }
  for (int r = 0; r < nround; ++r) {  // workgroup-uniform trip count: the barriers are safe
    const int kw = (4 * r + w) * PA_KB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // V rows into LDS; keys past the range as zeros
      const int idx = 64 * i + lane, kl = idx >> 3, pc = idx & 7;
      *reinterpret_cast<uint4*>(vsm + (PA_KB * w + kl) * PA_VS + 8 * pc) =
          kw + kl < nk ? vn[i] : uint4{0u, 0u, 0u, 0u};
    }
    uint4 kf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) kf[t][u] = kn[t][u];
    __syncthreads();
    if (r + 1 < nround) fetch(r + 1);  // the next round's rows fly under this round's arithmetic
    // V^T: A fragments per 16-dim tile (lane: dim 16 dt + c; k = 8 g + j -> key 4 g + j or 16 + 4 g + j - 4)
    uint4 vf[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      uint32_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kl = j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4);
        e[j] = vsm[(PA_KB * w + kl) * PA_VS + 16 * dt + c];
      }
      vf[dt] = uint4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
    }
    __syncthreads();  // vsm is rewritten by the next round (and by the merge after the last)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      float sc[8];
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[t][0]),
                                                          __builtin_bit_cast(bf16x8, qa[n]), f32x4{}, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[t][1]),
                                                    __builtin_bit_cast(bf16x8, qb[n]), a, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // C layout: column q = c, rows (keys) 4 g + i
          const float x = kw + 16 * t + 4 * g + i <= lim[n] ? a[i] * scale_log2 : -INFINITY;
          sc[4 * t + i] = x;
          bm = fmaxf(bm, x);
        }
      }
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float mn = fmaxf(m[n], bm);
      const float mu = mn == -INFINITY ? 0.0f : mn;  // no visible key yet: p = 2^-inf = 0
      const float alpha = exp2f(m[n] - mu);          // m = -inf: 0 (l and o are 0 then anyway)
      m[n] = mn;
      float ls = 0.0f;
      uint32_t ph[8], pl[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = exp2f(sc[j] - mu);
        ls += p;
        const bf16_t hi = f2bf(p);
        ph[j] = hi;
        pl[j] = f2bf(p - bf2f(hi));
      }
      l[n] = fmaf(l[n], alpha, ls);
      const uint4 bh4 =
          uint4{ph[0] | (ph[1] << 16), ph[2] | (ph[3] << 16), ph[4] | (ph[5] << 16), ph[6] | (ph[7] << 16)};
      const uint4 bl4 =
          uint4{pl[0] | (pl[1] << 16), pl[2] | (pl[3] << 16), pl[4] | (pl[5] << 16), pl[6] | (pl[7] << 16)};
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        f32x4 acc = o[n][dt] * alpha;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf[dt]),
                                                      __builtin_bit_cast(bf16x8, bl4), acc, 0, 0, 0);
        o[n][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf[dt]),
                                                           __builtin_bit_cast(bf16x8, bh4), acc, 0, 0, 0);
      }
    }
  }
  // the four waves' (m, l, o) -> the tile's rows.  The last barrier of the loop stands between
  // the last read of vsm and these writes to the same bytes.
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    float ln = l[n];
    ln += __shfl_xor(ln, 16, 64);
    ln += __shfl_xor(ln, 32, 64);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *reinterpret_cast<f32x4*>(osm + ((w * NT + n) * PA_Q + c) * PA_OS + 16 * dt + 4 * g) = o[n][dt];
    if (g == 0) {
      msm[w][n * PA_Q + c] = m[n];
      lsm[w][n * PA_Q + c] = ln;
    }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < NT; ++n) {  // thread (query ql, dims d4 .. d4 + 3) of each column group
    const int ql = n * PA_Q + (tid >> 4), d4 = 4 * (tid & 15);
    if (ql < nq) {
      // wave 0 holds key 0 < P, which every query sees, so M is finite and L > 0
      const float M = fmaxf(fmaxf(msm[0][ql], msm[1][ql]), fmaxf(msm[2][ql], msm[3][ql]));
      f32x4 acc = f32x4{};
      float L = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float f = exp2f(msm[q][ql] - M);  // a wave that saw no key of this query: 2^-inf = 0
        acc += f * *reinterpret_cast<const f32x4*>(osm + (q * NT * PA_Q + ql) * PA_OS + d4);
        L = fmaf(f, lsm[q][ql], L);
      }
      const float inv = 1.0f / L;
      *reinterpret_cast<uint2*>(out + ((int64_t)b * S + q0 + ql) * C + hh * PA_D + d4) =
          uint2{pack2(acc[0] * inv, acc[1] * inv), pack2(acc[2] * inv, acc[3] * inv)};
    }
  }
}

}  // namespace

// Attention of the suffix queries of a shared-prefix batch.  qkv: [B, S, 3C] bf16 (C = 64 H), the
// suffix tokens' packed projections, right-padded; pk / pv: [1, H, Tp, 64] bf16, the prefix
// caches, rows 0 .. P - 1 live (1 <= P <= Tp; later rows are never read); out: [B, S, C] bf16,
// every row written.  Query i of row b sees prefix keys 0 .. P - 1 and its row's keys 0 .. i.
NSA_API hipError_t nsa_prefix_attn(const void* qkv, const void* pk, const void* pv, void* out, int B, int S, int H,
                                   int Tp, int P, float scale, hipStream_t s) {
  if (B < 1 || S < 1 || H < 1 || P < 1 || P > Tp || !qkv || !pk || !pv || !out) return hipErrorInvalidValue;
  const int nt = S > PA_Q ? 2 : 1;
  const int nqt = (S + nt * PA_Q - 1) / (nt * PA_Q);
  const int64_t grid = (int64_t)B * H * nqt;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  const float scale_log2 = scale * 1.4426950408889634f;
  if (nt == 1)
    prefix_attn_kernel<1><<<(unsigned)grid, 256, 0, s>>>((const bf16_t*)qkv, (const bf16_t*)pk, (const bf16_t*)pv,
                                                         (bf16_t*)out, S, H, Tp, P, nqt, scale_log2);
  else
    prefix_attn_kernel<2><<<(unsigned)grid, 256, 0, s>>>((const bf16_t*)qkv, (const bf16_t*)pk, (const bf16_t*)pv,
                                                         (bf16_t*)out, S, H, Tp, P, nqt, scale_log2);
  return hipGetLastError();
}
