// The flash-decoding attention pieces shared by decode.hip (one cache per batch row) and
// decode_shared.hip (one prompt cache for the whole batch plus per-row caches): the body that
// turns one 256-key chunk of one (row, head)'s cache into a partial (m, l, o[64]), the int8
// cache-row quantizer it appends with, and the kernel that combines any number of partials.
#pragma once

#include "decode_rows.h"

#include <math.h>

namespace {

// One cache row's int8 form: scale = absmax / 127 (1 for an all-zero row), q = rint(x / scale)
// with a correctly rounded fp32 division (the build uses no fast-math), round-half-to-even and
// a clamp to +-127: ops.quantize_cache_rows bit for bit.
__device__ __forceinline__ float kv8_scale(float absmax) { return absmax > 0.0f ? absmax / 127.0f : 1.0f; }
__device__ __forceinline__ float kv8_quant(float x, float scale) {
  return fminf(fmaxf(rintf(x / scale), -127.0f), 127.0f);
}
// four integer-valued floats as the bytes of one dword (byte 0 first)
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
  return ((uint32_t)(int)a & 0xffu) | (((uint32_t)(int)b & 0xffu) << 8) | (((uint32_t)(int)c & 0xffu) << 16) |
         ((uint32_t)(int)d << 24);
}

// per-row scales of an int8 cache (fp32 [B, H, Tmax] each); nothing for a bf16 cache
template <typename CT>
struct CacheScales {};
template <>
struct CacheScales<int8_t> {
  float* k;
  float* v;
};

// One workgroup (256 threads), one chunk: keys k0 .. k0 + 255 of the cache rows row0 .. row0 +
// Tmax - 1 (row0 + key indexes kc / vc in 64-element rows and cs.k / cs.v), for the query whose
// q | k | v starts at qrow (C = H * 64 apart) and whose own position, the newest key, is pos.
// Writes the chunk's (m, l, o[64]) to part; a chunk beyond pos (or pos outside the cache) gives
// the empty partial.  Every branch on the arguments must be workgroup-uniform.
// append: also store the new token's K / V rows at position pos (kc_w / vc_w alias
// kc / vc; separate non-restrict pointers for the one write)
//
// One contract for both cache forms: the output is a function of the cache contents only, the
// row at pos included.  Without append every K and V row, pos too, is read from the cache and
// the k | v parts of qkv are not looked at; with append the result is what kv_append followed
// by a plain call gives, bit for bit, in the partials and in the output.
//
// CT: the cache's element type.  bf16_t: the rows hold the values.  int8_t: 64-byte rows with
// one fp32 scale per row in cs.k / cs.v (CacheScales: empty in the bf16 form).  A thread scores
// its key on the raw bytes (int8 -> float
// is exact) and multiplies by the key's scale once; ps[] holds p * vscale[key], so the V loop
// works on raw bytes too, while l sums the un-scaled p.  Appending, the workgroup whose chunk
// holds pos quantizes the new K and V rows itself (wave 0: K, wave 1: V; one value per lane),
// stores bytes and scale for later steps and leaves the quantized values in LDS (nq / nsc):
// the threads that meet position pos take the row from there in the same arithmetic as from
// the cache, never from the global row this launch writes.  So the output is a function of
// the cache contents only: append gives what kv_append followed by a plain call gives.
template <typename CT>
__device__ __forceinline__ void decode_attn_chunk(const bf16_t* __restrict__ qrow, const CT* __restrict__ kc,
                                                  const CT* __restrict__ vc, CT* kc_w, CT* vc_w,
                                                  const CacheScales<CT>& cs, int64_t row0, int pos, int Tmax, int k0,
                                                  float* __restrict__ part, int C, float scale_log2, int append) {
  constexpr bool KV8 = sizeof(CT) == 1;
  __shared__ float qs[DA_D];
  __shared__ float ps[DA_CHUNK];
  __shared__ float red[2][4];
  __shared__ float os[4][DA_D];
  __shared__ float nq[KV8 ? 2 : 1][DA_D];  // int8 caches, append: the new K / V rows, quantized (integers)
  __shared__ float nsc[2];                 // and their scales
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (k0 > pos || pos >= Tmax) {  // chunk beyond the live context (or no such cache row): empty partial
    if (tid < DA_PART) part[tid] = tid == 0 ? -INFINITY : 0.0f;
    return;
  }
  if (tid < DA_D) qs[tid] = bf2f(qrow[tid]);
  const int key = k0 + tid;
  const bool live = key <= pos;
  // int8 caches: this thread's key row (raw bytes) and its K / V scales; the row this launch
  // appends comes from LDS instead (fresh), and its loads go to the (valid, unused) q row, not
  // to the cache row being written
  [[maybe_unused]] const bool fresh = KV8 && append && key == pos;
  [[maybe_unused]] uint4 ku[DA_D / 16];
  [[maybe_unused]] float ks = 0.0f, vs = 0.0f;
  if constexpr (KV8) {
    if (live) {  // issued before the quantizer below, so their latency overlaps it
      const int64_t row = row0 + key;
      const uint4* krow = reinterpret_cast<const uint4*>(fresh ? (const int8_t*)qrow : kc + row * DA_D);
#pragma unroll
      for (int c = 0; c < DA_D / 16; ++c) ku[c] = krow[c];
      if (!fresh) {
        ks = cs.k[row];
        vs = cs.v[row];
      }
    }
    if (append && pos < k0 + DA_CHUNK && w < 2) {  // wave-uniform: all 64 lanes of waves 0 and 1
      const float x = bf2f(qrow[(1 + w) * C + lane]);
      const float s1 = kv8_scale(wave_max(fabsf(x)));
      const float qv = kv8_quant(x, s1);
      nq[w][lane] = qv;
      // lane l < 16 stores bytes 4l .. 4l+3 as one dword
      const float q0 = __shfl(qv, (4 * lane) & 63, 64), q1 = __shfl(qv, (4 * lane + 1) & 63, 64);
      const float q2 = __shfl(qv, (4 * lane + 2) & 63, 64), q3 = __shfl(qv, (4 * lane + 3) & 63, 64);
      const int64_t row = row0 + pos;
      if (lane < DA_D / 4)
        reinterpret_cast<uint32_t*>((w ? vc_w : kc_w) + row * DA_D)[lane] = kv8_pack4(q0, q1, q2, q3);
      if (lane == 0) {
        nsc[w] = s1;
        (w ? cs.v : cs.k)[row] = s1;
      }
    }
  } else {
    if (append && pos < k0 + DA_CHUNK && tid < 2 * (DA_D / 8)) {
      // this chunk holds position pos: store the new token's K / V rows for later steps
      // (appending, this kernel itself takes them straight from qkv, bitwise what it stores
      // here, so no write->read ordering)
      const int c = tid & 7, kv = tid >> 3;
      *reinterpret_cast<uint4*>((kv ? vc_w : kc_w) + (row0 + pos) * DA_D + 8 * c) =
          *reinterpret_cast<const uint4*>(qrow + (1 + kv) * C + 8 * c);
    }
  }
  __syncthreads();
  float sc = -INFINITY;
  if (live) {
    float acc = 0.0f;
    if constexpr (KV8) {
      if (fresh) {
        ks = nsc[0];
        vs = nsc[1];
      }
#pragma unroll
      for (int c = 0; c < DA_D / 16; ++c) {
        float kf[2][8];
        unpack8q(ku[c].x, ku[c].y, kf[0]);
        unpack8q(ku[c].z, ku[c].w, kf[1]);
        if (fresh)
#pragma unroll
          for (int j = 0; j < 16; ++j) kf[j >> 3][j & 7] = nq[0][16 * c + j];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = fmaf(qs[16 * c + j], kf[j >> 3][j & 7], acc);
      }
      acc *= ks;
    } else {
      // the new token's row comes from qkv when appending (this launch is what writes it to
      // the cache), as its V row does below; otherwise every row, pos included, is the cache's
      const bf16_t* krow = (append && key == pos) ? qrow + C : kc + (row0 + key) * DA_D;
#pragma unroll
      for (int c = 0; c < DA_D / 8; ++c) {
        float kf[8];
        load8(krow + 8 * c, kf);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(qs[8 * c + j], kf[j], acc);
      }
    }
    sc = acc * scale_log2;
  }
  float m = wave_max(sc);
  if (lane == 0) red[0][w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  const float p = live ? exp2f(sc - m) : 0.0f;
  const float lw = wave_sum(p);
  if (lane == 0) red[1][w] = lw;
  if constexpr (KV8) ps[tid] = live ? p * vs : 0.0f;  // a dead key has no scale to read
  else ps[tid] = p;
  __syncthreads();
  // weighted V sum: thread (key group kg = tid / 8: keys k0 + 8 kg .. +7; dims 8 dg .. +7)
  // issues its 8 16-byte row loads together (one 2-byte load per key and lane in a
  // 64-long dependent loop was the kernel's latency chain).  Keys past pos read the row
  // at pos (finite) and carry p = 0; the new token's row comes from qkv when appending
  // (this launch is what writes it to the cache).
  const int kg = tid >> 3, dg = tid & 7;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int kk = min(k0 + 8 * kg + j, pos);
    float vf[8];
    if constexpr (KV8) {  // 8-byte loads; the appended row from LDS as for K
      const bool vfresh = append && kk == pos;
      const int8_t* vr = vfresh ? (const int8_t*)qrow : vc + (row0 + kk) * DA_D;
      const uint2 u = *reinterpret_cast<const uint2*>(vr + 8 * dg);
      unpack8q(u.x, u.y, vf);
      if (vfresh)
#pragma unroll
        for (int e = 0; e < 8; ++e) vf[e] = nq[1][8 * dg + e];
    } else {
      const bf16_t* vr = (append && kk == pos) ? qrow + 2 * C : vc + (row0 + kk) * DA_D;
      load8(vr + 8 * dg, vf);
    }
    const float pj = ps[8 * kg + j];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(pj, vf[e], o[e]);
  }
#pragma unroll
  for (int off = 8; off < 64; off <<= 1)  // the wave's 8 key groups (lane bits 3..5)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] += __shfl_xor(o[e], off, 64);
  if (lane < 8)
#pragma unroll
    for (int e = 0; e < 8; ++e) os[w][8 * lane + e] = o[e];
  __syncthreads();
  if (tid < DA_D) part[DA_PO + tid] = os[0][tid] + os[1][tid] + os[2][tid] + os[3][tid];
  if (tid == 0) {
    part[0] = m;
    part[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// grid B*H, 64 threads: out[b, h*64 + d] = sum_s 2^(m_s - M) o_s[d] / sum_s 2^(m_s - M) l_s
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(const float* __restrict__ ws,
                                                                 bf16_t* __restrict__ out, int H, int n_split) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const int b = bh / H, hh = bh % H;
  const float* part = ws + (int64_t)bh * n_split * DA_PART;
  float M = -INFINITY;
  for (int s = 0; s < n_split; ++s) M = fmaxf(M, part[s * DA_PART]);
  float L = 0.0f, o = 0.0f;
  for (int s = 0; s < n_split; ++s) {
    const float f = exp2f(part[s * DA_PART] - M);  // empty chunks: 2^-inf = 0
    L = fmaf(f, part[s * DA_PART + 1], L);
    o = fmaf(f, part[s * DA_PART + DA_PO + d], o);
  }
  out[(int64_t)b * H * DA_D + hh * DA_D + d] = f2bf(o / L);
}

}  // namespace
