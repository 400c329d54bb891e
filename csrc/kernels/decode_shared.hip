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
#include "decode_shared.h"

namespace {

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
