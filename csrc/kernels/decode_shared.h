// The pieces of the shared-prompt decode attention that decode_shared.hip and decode_beam.hip both
// launch: the prompt workgroup (one (head, 128-key chunk) of the prompt cache serving every batch row
// on the matrix cores) and the wide combine.  decode_shared.hip describes the whole launch.
#pragma once

#include "decode_attn.h"

namespace {

constexpr int SP_CHUNK = 128;  // prompt keys per workgroup: 32 per wave
constexpr int SP_VS = 72;      // bf16 elements per V row in LDS: 144 bytes (16-byte aligned rows; the
                               // four rows 4 g of a fragment read fall into different banks)
constexpr int SP_OS = 68;      // floats per o row in LDS

__device__ __forceinline__ void shared_prompt_chunk(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ pk,
                                                    const bf16_t* __restrict__ pv, int P, float* __restrict__ ws,
                                                    int B, int H, int Tp, int n_split, int hh, int s,
                                                    float scale_log2) {
  __shared__ __attribute__((aligned(16))) bf16_t vsm[SP_CHUNK * SP_VS];
  __shared__ __attribute__((aligned(16))) float osm[4][16][SP_OS];
  __shared__ float msm[4][16];
  __shared__ float lsm[4][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int C = H * DA_D;
  const int k0 = s * SP_CHUNK;
  P = min(P, Tp);
  if (k0 >= P) {  // chunk wholly past the prompt: the empty partial for every row
    for (int e = tid; e < B * DA_PART; e += 256) {
      const int b = e / DA_PART, i = e % DA_PART;
      ws[((int64_t)(b * H + hh) * n_split + s) * DA_PART + i] = i == 0 ? -INFINITY : 0.0f;
    }
    return;
  }
  const int kw = k0 + 32 * w;  // this wave's first key
  const bf16_t* pkh = pk + (int64_t)hh * Tp * DA_D;
  const bf16_t* pvh = pv + (int64_t)hh * Tp * DA_D;
  // K: A fragments of the two 16-key tiles (lane: key c of the tile, dims 32 u + 8 g .. + 7)
  uint4 kf[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bf16_t* krow = pkh + (int64_t)min(kw + 16 * t + c, Tp - 1) * DA_D + 8 * g;
#pragma unroll
    for (int u = 0; u < 2; ++u) kf[t][u] = *reinterpret_cast<const uint4*>(krow + 32 * u);
  }
  // q^T: B fragments (lane: batch row c of a 16-row group, dims 32 u + 8 g .. + 7); the first
  // group's are fetched with K and V, every later group's one group ahead
  const bf16_t* qbase = qkv + hh * DA_D + 8 * g;
  uint4 q0 = *reinterpret_cast<const uint4*>(qbase + (int64_t)min(c, B - 1) * 3 * C);
  uint4 q1 = *reinterpret_cast<const uint4*>(qbase + (int64_t)min(c, B - 1) * 3 * C + 32);
  // V: the wave's 32 rows into LDS, 16 bytes per lane and pass; dead keys as zeros (p = 0
  // times whatever the cache holds there must not be NaN)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = 64 * i + lane, kl = idx >> 3, pc = idx & 7;
    uint4 v = *reinterpret_cast<const uint4*>(pvh + (int64_t)min(kw + kl, Tp - 1) * DA_D + 8 * pc);
    if (kw + kl >= P) v = uint4{0u, 0u, 0u, 0u};
    *reinterpret_cast<uint4*>(vsm + (32 * w + kl) * SP_VS + 8 * pc) = v;
  }
  __syncthreads();
  // V^T: A fragments per 16-dim tile (lane: dim 16 dt + c; k = 8 g + j -> key 4 g + j or 16 + 4 g + j - 4)
  uint4 vf[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kl = j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4);
      e[j] = vsm[(32 * w + kl) * SP_VS + 16 * dt + c];
    }
    vf[dt] = uint4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
  }
  const int ngroup = (B + 15) / 16;
  for (int grp = 0; grp < ngroup; ++grp) {
    const uint4 qa = q0, qb = q1;
    if (grp + 1 < ngroup) {  // workgroup-uniform
      const bf16_t* qrow = qbase + (int64_t)min(16 * (grp + 1) + c, B - 1) * 3 * C;
      q0 = *reinterpret_cast<const uint4*>(qrow);
      q1 = *reinterpret_cast<const uint4*>(qrow + 32);
    }
    float sc[8];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[t][0]),
                                                        __builtin_bit_cast(bf16x8, qa), f32x4{}, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[t][1]),
                                                  __builtin_bit_cast(bf16x8, qb), a, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // C layout: column b = c, rows (keys) 4 g + i
        const float x = kw + 16 * t + 4 * g + i < P ? a[i] * scale_log2 : -INFINITY;
        sc[4 * t + i] = x;
        m = fmaxf(m, x);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mu = m == -INFINITY ? 0.0f : m;  // a wave with no live key: p = 2^-inf = 0
    float l = 0.0f;
    uint32_t ph[8], pl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = exp2f(sc[j] - mu);
      l += p;
      const bf16_t hi = f2bf(p);
      ph[j] = hi;
      pl[j] = f2bf(p - bf2f(hi));
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const uint4 bh4 = uint4{ph[0] | (ph[1] << 16), ph[2] | (ph[3] << 16), ph[4] | (ph[5] << 16), ph[6] | (ph[7] << 16)};
    const uint4 bl4 = uint4{pl[0] | (pl[1] << 16), pl[2] | (pl[3] << 16), pl[4] | (pl[5] << 16), pl[6] | (pl[7] << 16)};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      f32x4 o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf[dt]),
                                                        __builtin_bit_cast(bf16x8, bl4), f32x4{}, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf[dt]), __builtin_bit_cast(bf16x8, bh4),
                                                  o, 0, 0, 0);
      // C layout: column b = c, rows (dims) 16 dt + 4 g + i
      *reinterpret_cast<f32x4*>(&osm[w][c][16 * dt + 4 * g]) = o;
    }
    if (g == 0) {
      msm[w][c] = m;
      lsm[w][c] = l;
    }
    __syncthreads();
    {  // the four waves' partials -> one partial per row: thread (row bl, dims d4 .. d4 + 3)
      const int bl = tid >> 4, d4 = 4 * (tid & 15), b = 16 * grp + bl;
      if (b < B) {
        // wave 0 holds key k0 < P, so M is finite
        const float M = fmaxf(fmaxf(msm[0][bl], msm[1][bl]), fmaxf(msm[2][bl], msm[3][bl]));
        f32x4 o = f32x4{};
        float L = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float f = exp2f(msm[q][bl] - M);
          const f32x4 oq = *reinterpret_cast<const f32x4*>(&osm[q][bl][d4]);
          o += f * oq;
          L = fmaf(f, lsm[q][bl], L);
        }
        float* part = ws + ((int64_t)(b * H + hh) * n_split + s) * DA_PART;
        *reinterpret_cast<f32x4*>(part + DA_PO + d4) = o;
        if (d4 == 0) {
          part[0] = M;
          part[1] = L;
        }
      }
    }
    __syncthreads();  // osm / msm / lsm are rewritten by the next group
  }
}

// The combine of decode_attn.h for up to 64 partials per (row, head), with its loads side by
// side instead of in two dependent loops (this form has ceil(Tp / 128) + ceil(R / 256) partials,
// 12 at Tp = R = 1024 where the unshared form has 4, and the launch is all latency): lane s
// holds (m_s, l_s), the maximum and the sum meet in shuffles, and the o rows arrive 8 at a time,
// the first 8 requested before anything else.  grid B*H, 64 threads.
__global__ __launch_bounds__(64) void decode_attn_combine_wide_kernel(const float* __restrict__ ws,
                                                                      bf16_t* __restrict__ out, int H, int n_split) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const int b = bh / H, hh = bh % H;
  const float* part = ws + (int64_t)bh * n_split * DA_PART;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = part[min(j, n_split - 1) * DA_PART + DA_PO + d];
  float m = -INFINITY, l = 0.0f;
  if (d < n_split) {
    m = part[d * DA_PART];
    l = part[d * DA_PART + 1];
  }
  const float M = wave_max(m);
  const float f = exp2f(m - M);  // empty chunks and the lanes past n_split: 2^-inf = 0
  const float L = wave_sum(f * l);
  float o = 0.0f;
  for (int s0 = 0; s0 < n_split; s0 += 8) {
    if (s0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[min(s0 + j, n_split - 1) * DA_PART + DA_PO + d];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float fs = __shfl(f, (s0 + j) & 63, 64);
      o = fmaf(s0 + j < n_split ? fs : 0.0f, v[j], o);
    }
  }
  out[(int64_t)b * H * DA_D + hh * DA_D + d] = f2bf(o / L);
}

}  // namespace
