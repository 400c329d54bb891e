// Function-body fragment, not a header: the residual add + LayerNorm prologue of the skinny
// GEMMs (2..16 decode rows, 256 threads).  It is #included inside a function body: inline in
// decode.hip's skinny_ln_gemm_kernel, and as the body of decode_q8.hip's
// skinny_ln_prologue().  No include guard: every inclusion pastes the statements again.
//
// s = res + branch and x = LN(s) for the M batch rows (wave w: rows w, w + 4, ...; a row of
// K <= 2048 lives in 32 registers per lane, two-pass mean / variance as nanoGPT's fp32
// LayerNorm), x stored as bf16 in xs; rows M..15 are zeroed (they only feed output columns
// m >= M, which are never stored); workgroup 0 writes s (fp32).  The includer's barrier
// after it publishes xs[].
//
// Names it expects in scope:
//   res     const float*: the residual stream, [M][K] fp32
//   branch  const bf16_t*: the branch output added to it, [M][K], or null
//   s_out   float*: where workgroup 0 writes s, [M][K], or null (the entry points pass null
//           when there is no branch: s is res itself then and nothing is written)
//   lw, lb  const bf16_t*: LayerNorm weight and bias [K] (lb may be null)
//   eps     float: LayerNorm epsilon
//   xs      bf16_t*: LDS, [16][KP]
//   M       int: batch rows (<= 16)
//   K       int: row length (a multiple of 8, <= 2048)
//   KP      int: K + 8, the padded LDS row
//   lane    int: threadIdx.x & 63
//   w       int: threadIdx.x >> 6, the wave
  for (int m = M + w; m < 16; m += 4)
    for (int k = 8 * lane; k < K; k += 512) *reinterpret_cast<uint4*>(xs + m * KP + k) = uint4{0u, 0u, 0u, 0u};
  for (int m = w; m < M; m += 4) {
    const int mm = m;
    float v[4][8];
    float sum = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = (q * 64 + lane) * 8;
      if (k < K) {
        const float4 r0 = *reinterpret_cast<const float4*>(res + (int64_t)mm * K + k);
        const float4 r1 = *reinterpret_cast<const float4*>(res + (int64_t)mm * K + k + 4);
        v[q][0] = r0.x; v[q][1] = r0.y; v[q][2] = r0.z; v[q][3] = r0.w;
        v[q][4] = r1.x; v[q][5] = r1.y; v[q][6] = r1.z; v[q][7] = r1.w;
        if (branch) {
          float bv[8];
          load8(branch + (int64_t)mm * K + k, bv);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[q][e] += bv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += v[q][e];
      }
    }
    const float mean = wave_sum(sum) / (float)K;
    float sq = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if ((q * 64 + lane) * 8 < K)
#pragma unroll
        for (int e = 0; e < 8; ++e) sq = fmaf(v[q][e] - mean, v[q][e] - mean, sq);
    const float rstd = rsqrtf(wave_sum(sq) / (float)K + eps);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = (q * 64 + lane) * 8;
      if (k < K) {
        float wv[8], bv[8], o[8];
        load8(lw + k, wv);
        if (lb) {
          load8(lb + k, bv);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) bv[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[q][e] - mean) * rstd * wv[e] + bv[e];
        store8(xs + m * KP + k, o);
        if (blockIdx.x == 0 && s_out && m < M) {
          float* sp = s_out + (int64_t)m * K + k;
          *reinterpret_cast<float4*>(sp) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
          *reinterpret_cast<float4*>(sp + 4) = make_float4(v[q][4], v[q][5], v[q][6], v[q][7]);
        }
      }
    }
  }
