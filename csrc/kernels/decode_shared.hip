// Decode attention for a batch whose rows share one prompt (Decoder(..., shared_prompt=True)):
// the prompt's K / V are cached once, [1, H, Tp, 64] bf16 per layer, and every row keeps only
// the tokens it generated, [B, H, R, 64]: row b's token at absolute position p >= P (P = the
// prompt length, an int64 device scalar) lives in row-cache slot p - P.  A step then reads
// P + B n cache rows per head instead of B (P + n).
//
// One launch, two kinds of workgroup (the block index picks one; the branch is
// workgroup-uniform), both writing flash-decoding partials (m, l, o[64]) in the format of
// decode_attn.h, merged by a second launch (decode_attn_combine_wide_kernel below: the combine
// of decode_attn.h with its loads issued together; past 64 partials per row, that one itself):
//
//  * prompt work, blocks 0 .. H * npc - 1: workgroup (h, s) owns the 128 prompt keys of chunk
//    s of head h and serves every batch row from them.  Its K rows go from global memory
//    straight into MFMA A fragments (wave w: keys 32 w .. 32 w + 31 of the chunk, two 16-key
//    tiles) and its V rows into LDS, once; then for every group of 16 batch rows
//      S^T[key, b] = K[key, :] . q[b, :]      v_mfma_f32_16x16x32_bf16, A = K, B = q^T (both
//                                             bf16, fp32 accumulation: exact products)
//    leaves lane l with the scores of row b = l & 15 against keys 4 (l >> 4) + i of each tile,
//    the wave-local softmax (max, sum: registers, then two shuffles) runs on those, and
//      O^T[d, b] = V^T[d, key] . p^T[key, b]  A = V^T from LDS, B = p as it lies in the lanes
//    with p entering as hi + lo (two bf16 numbers whose sum carries 16 bits of p: one MFMA
//    each on the same A fragment), so the P.V product is as good as the fp32 one of the
//    per-row body.  The MFMA's k index is only a summation index: k = 8 g + j stands for key
//    4 g + j of tile 0 (j < 4) or of tile 1 (j >= 4), which is how the score tiles lie in the
//    registers, so p needs no lane movement.  The four waves' (m, l, o) meet in LDS and one
//    partial per (row, head, chunk) is stored.  Keys at or past P score -inf and their V rows
//    are zeroed; a chunk wholly past P stores empty partials and exits; rows past B inside
//    a 16-row group read row B - 1 and are never stored.
//  * row work, the blocks after those: workgroup (b, h, s) runs the per-row body
//    decode_attn_chunk on chunk s of row b's own cache with the position pos[b] - P, appending
//    the new token's K / V at that slot.
//
// The grid follows Tp and R only, so a captured step serves any prompt length.
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

// grid H * npc + B * H * nrc, 256 threads (npc = ceil(Tp / 128) prompt chunks, nrc = ceil(R / 256)
// row chunks); partial (b, h, s) at ws[((b H + h) (npc + nrc) + s) * 68], prompt chunks first
__global__ __launch_bounds__(256) void decode_attn_shared_kernel(const bf16_t* __restrict__ qkv,
                                                                 const bf16_t* __restrict__ pk,
                                                                 const bf16_t* __restrict__ pv,
                                                                 const bf16_t* __restrict__ kc,
                                                                 const bf16_t* __restrict__ vc, bf16_t* kc_w,
                                                                 bf16_t* vc_w, const int64_t* __restrict__ plen,
                                                                 const int64_t* __restrict__ pos_dev, int pos_stride,
                                                                 float* __restrict__ ws, int B, int H, int Tp, int R,
                                                                 int npc, int nrc, float scale_log2, int append) {
  const int n_split = npc + nrc;
  const int P = (int)*plen;
  const int blk = blockIdx.x;
  if (blk < H * npc) {
    shared_prompt_chunk(qkv, pk, pv, P, ws, B, H, Tp, n_split, blk / npc, blk % npc, scale_log2);
    return;
  }
  const int r = blk - H * npc;
  const int bh = r / nrc, s = r % nrc;
  const int b = bh / H, hh = bh % H;
  const int C = H * DA_D;
  // the row's newest key in its own cache: slot pos[b] - P (a negative slot gives empty partials)
  const int pos = (int)pos_dev[(int64_t)b * pos_stride] - P;
  decode_attn_chunk<bf16_t>(qkv + (int64_t)b * 3 * C + hh * DA_D, kc, vc, kc_w, vc_w, CacheScales<bf16_t>{},
                            (int64_t)bh * R, pos, R, s * DA_CHUNK,
                            ws + ((int64_t)bh * n_split + npc + s) * DA_PART, C, scale_log2, append);
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

hipError_t decode_attn_shared_launch(const void* qkv, const void* pk, const void* pv, void* kc, void* vc,
                                     const void* plen, const void* pos, int pos_stride, void* ws, void* out, int B,
                                     int H, int Tp, int R, float scale, int append, hipStream_t s) {
  if (B < 1 || H < 1 || Tp < 1 || R < 1 || !plen || !pos || !ws || !out) return hipErrorInvalidValue;
  const int npc = (Tp + SP_CHUNK - 1) / SP_CHUNK, nrc = (R + DA_CHUNK - 1) / DA_CHUNK;
  const int64_t grid = (int64_t)H * npc + (int64_t)B * H * nrc;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  decode_attn_shared_kernel<<<(unsigned)grid, 256, 0, s>>>(
      (const bf16_t*)qkv, (const bf16_t*)pk, (const bf16_t*)pv, (const bf16_t*)kc, (const bf16_t*)vc, (bf16_t*)kc,
      (bf16_t*)vc, (const int64_t*)plen, (const int64_t*)pos, pos_stride, (float*)ws, B, H, Tp, R, npc, nrc,
      scale * 1.4426950408889634f, append);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (npc + nrc <= 64)
    decode_attn_combine_wide_kernel<<<B * H, 64, 0, s>>>((const float*)ws, (bf16_t*)out, H, npc + nrc);
  else
    decode_attn_combine_kernel<<<B * H, 64, 0, s>>>((const float*)ws, (bf16_t*)out, H, npc + nrc);
  return hipGetLastError();
}

}  // namespace

// Single-query attention of every row's newest token over the shared prompt cache pk / pv
// ([1, H, Tp, 64] bf16, keys 0 .. *plen - 1) and the row's own cache kc / vc ([B, H, R, 64],
// slots 0 .. *pos - *plen).  qkv: [B, 1, 3C]; out: [B, C] bf16; ws: B * H * (ceil(Tp / 128) +
// ceil(R / 256)) * 68 fp32.  append != 0: the new token's K / V are taken from qkv and stored
// at slot *pos - *plen; otherwise the row caches must already hold that slot.  One position
// for the batch (pos: int64 device scalar).
NSA_API hipError_t nsa_decode_attn_shared(const void* qkv, const void* pk, const void* pv, void* kc, void* vc,
                                          const void* plen, const void* pos, void* ws, void* out, int B, int H,
                                          int Tp, int R, float scale, int append, hipStream_t s) {
  return decode_attn_shared_launch(qkv, pk, pv, kc, vc, plen, pos, 0, ws, out, B, H, Tp, R, scale, append, s);
}

// The same with one position per row (pos: int64[B]).
NSA_API hipError_t nsa_decode_attn_shared_rows(const void* qkv, const void* pk, const void* pv, void* kc, void* vc,
                                               const void* plen, const void* pos, void* ws, void* out, int B, int H,
                                               int Tp, int R, float scale, int append, hipStream_t s) {
  return decode_attn_shared_launch(qkv, pk, pv, kc, vc, plen, pos, 1, ws, out, B, H, Tp, R, scale, append, s);
}
