// Function-body fragment, not a header: the single-row prologue of the decode linears
// (decode_rows.h: PRO_LN, PRO_EMB_LN, PRO_ATTN).  It is #included inside a function body:
// inline in decode.hip's gemv_row_kernel, and as the body of decode_q8.hip's row_prologue().
// No include guard: every inclusion pastes the statements again.  (One source, shared as
// text: as a function called from gemv_row_kernel the same statements compile to other code.)
//
// Names it expects in scope:
//   a      const RowPro&: the prologue's arguments
//   hs     float*: LDS, the row x[K]; PRO_ATTN also uses hs[K ..] for the chunk weights
//   stat   float[2][4]: LDS, the per-wave partial sums of the two block reductions
//   K      int: row length
//   tid    int: threadIdx.x (256 threads)
//   lane   int: tid & 63
//   w      int: tid >> 6, the wave
//   PRO    int, compile-time: which prologue
//   NSA_HS(k)  macro: the index in hs[] of x[k] (the includer defines it and #undefs it
//          afterwards); it may use any name in scope at the inclusion
// It leaves x[K] in hs[] as bf16-rounded floats; the includer's barrier after it publishes hs[].
//
// K <= 2048 (every GPT-2 width): thread g owns x[8g .. 8g+7] and issues all of its loads
// at once (16-byte vectors), so the row costs one memory round trip and two block
// reductions; wider rows loop.
#ifndef NSA_HS
#error "decode_row_prologue.h: define NSA_HS(k), the hs[] index of x[k], before the inclusion"
#endif
  const bool vec = K <= 2048;
  const int g8 = 8 * tid;
  const bool own = vec && g8 < K;
  if constexpr (PRO == PRO_ATTN) {
    const int H = K / DA_D, ns = a.n_split;
    float* fs = hs + K;  // [H][ns] chunk weights 2^(m_s - M) / L
    for (int h = tid; h < H; h += 256) {
      const float* part = a.ws + (int64_t)h * ns * DA_PART;
      float M = -INFINITY;
#pragma unroll 4
      for (int sp = 0; sp < ns; ++sp) M = fmaxf(M, part[sp * DA_PART]);
      float L = 0.0f;
#pragma unroll 4
      for (int sp = 0; sp < ns; ++sp) L = fmaf(exp2f(part[sp * DA_PART] - M), part[sp * DA_PART + 1], L);
      const float inv = 1.0f / L;
      for (int sp = 0; sp < ns; ++sp) fs[h * ns + sp] = exp2f(part[sp * DA_PART] - M) * inv;  // empty: 0
    }
    __syncthreads();
    for (int k0 = g8; k0 < K; k0 += 8 * 256) {  // 8 dims of one head per thread and pass
      const int h = k0 / DA_D;
      const float* o = a.ws + (int64_t)h * ns * DA_PART + DA_PO + (k0 % DA_D);
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int sp = 0; sp < ns; ++sp) {
        const float f = fs[h * ns + sp];
        const float4 u0 = *reinterpret_cast<const float4*>(o + sp * DA_PART);
        const float4 u1 = *reinterpret_cast<const float4*>(o + sp * DA_PART + 4);
        acc[0] = fmaf(f, u0.x, acc[0]);
        acc[1] = fmaf(f, u0.y, acc[1]);
        acc[2] = fmaf(f, u0.z, acc[2]);
        acc[3] = fmaf(f, u0.w, acc[3]);
        acc[4] = fmaf(f, u1.x, acc[4]);
        acc[5] = fmaf(f, u1.y, acc[5]);
        acc[6] = fmaf(f, u1.z, acc[6]);
        acc[7] = fmaf(f, u1.w, acc[7]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) hs[NSA_HS(k0 + e)] = bf2f(f2bf(acc[e]));  // the bf16 attention output
    }
  } else {
    const bool write_s = PRO == PRO_EMB_LN || a.branch != nullptr;
    int64_t te = 0, pe = 0;
    if constexpr (PRO == PRO_EMB_LN) {
      te = *a.tok;
      pe = *a.pos;
    }
    float xv[8], lwv[8], lbv[8];
    float sum = 0.0f;
    if (vec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = lwv[e] = lbv[e] = 0.0f;
      if (own) {
        if constexpr (PRO == PRO_EMB_LN) {
          float e0[8], e1[8];
          load8(a.wte + te * K + g8, e0);
          load8(a.wpe + pe * K + g8, e1);
#pragma unroll
          for (int e = 0; e < 8; ++e) xv[e] = e0[e] + e1[e];
        } else {
          const float4 r0 = *reinterpret_cast<const float4*>(a.res + g8);
          const float4 r1 = *reinterpret_cast<const float4*>(a.res + g8 + 4);
          xv[0] = r0.x; xv[1] = r0.y; xv[2] = r0.z; xv[3] = r0.w;
          xv[4] = r1.x; xv[5] = r1.y; xv[6] = r1.z; xv[7] = r1.w;
          if (a.branch) {
            float bv[8];
            load8(a.branch + g8, bv);
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] += bv[e];
          }
        }
        load8(a.lw + g8, lwv);
        if (a.lb) load8(a.lb + g8, lbv);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += xv[e];
    } else {
      for (int k = tid; k < K; k += 256) {
        float v;
        if constexpr (PRO == PRO_EMB_LN) {
          v = bf2f(a.wte[te * K + k]) + bf2f(a.wpe[pe * K + k]);
        } else {
          v = a.res[k];
          if (a.branch) v += bf2f(a.branch[k]);
        }
        hs[NSA_HS(k)] = v;
        sum += v;
      }
    }
    sum = wave_sum(sum);
    if (lane == 0) stat[0][w] = sum;
    __syncthreads();
    const float mean = (stat[0][0] + stat[0][1] + stat[0][2] + stat[0][3]) / (float)K;
    float sq = 0.0f;
    if (vec) {
      if (own)
#pragma unroll
        for (int e = 0; e < 8; ++e) sq = fmaf(xv[e] - mean, xv[e] - mean, sq);
    } else {
      for (int k = tid; k < K; k += 256) {
        const float d = hs[NSA_HS(k)] - mean;
        sq = fmaf(d, d, sq);
      }
    }
    sq = wave_sum(sq);
    if (lane == 0) stat[1][w] = sq;
    __syncthreads();
    const float rstd = rsqrtf((stat[1][0] + stat[1][1] + stat[1][2] + stat[1][3]) / (float)K + a.eps);
    if (vec) {
      if (own) {
        if (blockIdx.x == 0 && write_s) {
          *reinterpret_cast<float4*>(a.res_out + g8) = make_float4(xv[0], xv[1], xv[2], xv[3]);
          *reinterpret_cast<float4*>(a.res_out + g8 + 4) = make_float4(xv[4], xv[5], xv[6], xv[7]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) hs[NSA_HS(g8 + e)] = bf2f(f2bf((xv[e] - mean) * rstd * lwv[e] + lbv[e]));
      }
    } else {
      for (int k = tid; k < K; k += 256) {
        const float sv = hs[NSA_HS(k)];
        if (blockIdx.x == 0 && write_s) a.res_out[k] = sv;
        float h = (sv - mean) * rstd * bf2f(a.lw[k]);
        if (a.lb) h += bf2f(a.lb[k]);
        hs[NSA_HS(k)] = bf2f(f2bf(h));  // the bf16 activation the LayerNorm kernel would hand the GEMM
      }
    }
  }
