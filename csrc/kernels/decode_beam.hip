// Beam search on the decode path (Decoder(..., num_beams=W)): the W hypotheses are the rows of a
// shared-prompt decoder (decode_shared.hip: the prompt's K / V once, [1, H, Tp, 64], and row caches
// [W, H, R, 64] of the generated tokens), and every step each survivor continues one of the
// previous step's rows, its parent.  Nothing is ever copied between rows for that.  A survivor
// inherits its parent's text through the ancestry table src (int32 [W, R]): the key of beam w at
// row-cache slot t is the one row src[w, t] stored there, wherever the beam has been since.
//
//  * decode_attn_beam_kernel: the shared-prompt step attention with that indirection.  The prompt
//    workgroups are decode_shared.h's, unchanged.  A row workgroup (w, h, 256-slot chunk) runs
//    the per-row body with ANC set (decode_attn.h): every thread fetches its slot's row index,
//    then its K row through it, and the V rows are gathered through the indices left in LDS.
//    Same chunks, same order inside a chunk, same partials, same combine: for any src the
//    result is nsa_decode_attn_shared's on row caches gathered as kc_m[w, :, t] = kc[src[w, t],
//    :, t], bit for bit.  The new token's K / V go to (w, pos - P), from qkv, as there.
//  * beam_step_kernel: one workgroup closes a step on the device: it picks the W survivors
//    among the W x W candidates (every row's W most likely ids, nsa_token_logprobs with top = W),
//    writes what the next step feeds and what the result is read from, and permutes src.
#include "decode_shared.h"

namespace {

constexpr int BEAM_MAX = 8;  // beams: W * W candidates fit one wave, one per lane

// grid H * npc + B * H * nrc, 256 threads: decode_attn_shared_kernel's grid and partials, one
// position for the batch; src: int32 [B, R]
__global__ __launch_bounds__(256) void decode_attn_beam_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ pk, const bf16_t* __restrict__ pv,
    const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc, bf16_t* kc_w, bf16_t* vc_w,
    const int* __restrict__ src, const int64_t* __restrict__ plen, const int64_t* __restrict__ pos_dev,
    float* __restrict__ ws, int B, int H, int Tp, int R, int npc, int nrc, float scale_log2, int append) {
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
  const int pos = (int)*pos_dev - P;  // the newest slot (a negative one gives empty partials)
  decode_attn_chunk<bf16_t, true>(qkv + (int64_t)b * 3 * C + hh * DA_D, kc, vc, kc_w, vc_w, CacheScales<bf16_t>{},
                                  (int64_t)hh * R, pos, R, s * DA_CHUNK,
                                  ws + ((int64_t)bh * n_split + npc + s) * DA_PART, C, scale_log2, append,
                                  src + (int64_t)b * R, (int64_t)H * R, B, b);
}

// One workgroup of 256 threads, dynamic LDS W * R bytes.  n = *n_dev is the index of the token
// this step generates; n outside 0 .. R - 1 changes nothing.
//
// Selection (wave 0, lane c = w W + j: candidate j of beam w).  A live beam's candidate is worth
// scores[w] + top_lp[w, j], one fp32 addition; a finished beam offers (w, 0) alone, worth scores[w],
// with the stop token.  The order is (value descending, parent ascending, j ascending), which is
// (value descending, c ascending): a lane's rank is the number of candidates that come before it,
// counted against the values in LDS, and the lanes of rank < W write survivor slot rank.  Values
// compare as floats; -inf is a value like any other.
//
// Ancestry: src'[w', 0 .. n) = src[parent[w'], 0 .. n) and src'[w', n] = w', in place.  The live
// part of src goes through LDS (row indices fit a byte), with the barrier between the reads and
// the writes; entries past n are not touched.  All state is read before that barrier and written
// after it.
__global__ __launch_bounds__(256) void beam_step_kernel(const int* __restrict__ top_ids,
                                                        const float* __restrict__ top_lp, float* scores, int* done,
                                                        int* length, int* __restrict__ parent,
                                                        int64_t* __restrict__ tok, int* src,
                                                        int* __restrict__ bp_parent, int64_t* __restrict__ bp_token,
                                                        int* n_dev, int* __restrict__ all_done, int W, int R,
                                                        int64_t stop) {
  extern __shared__ unsigned char anc[];  // [W][R]: src[:, 0 .. n)
  __shared__ float cval[64];
  __shared__ int cok[64];
  __shared__ int s_parent[BEAM_MAX], s_done[BEAM_MAX], s_len[BEAM_MAX];
  __shared__ float s_score[BEAM_MAX];
  __shared__ int64_t s_tok[BEAM_MAX];
  const int tid = threadIdx.x;
  const int n = *n_dev;
  if (n < 0 || n >= R) return;  // workgroup-uniform
  const int nc = W * W;
  int w = 0, dn = 0, len = 0;
  float val = 0.0f;
  bool ok = false;
  if (tid < nc) {
    w = tid / W;
    const int j = tid - w * W;
    dn = done[w] != 0;
    len = length[w];
    val = scores[w];
    if (!dn) val = val + top_lp[tid];
    ok = !dn || j == 0;
  }
  if (tid < 64) {
    cval[tid] = val;
    cok[tid] = ok;
  }
  for (int e = tid; e < W * n; e += 256) {
    const int r = e / n, t = e - r * n;
    anc[r * R + t] = (unsigned char)src[r * R + t];
  }
  __syncthreads();
  if (ok) {
    int rank = 0;
    for (int c = 0; c < nc; ++c) {
      const float v = cval[c];
      rank += cok[c] && (v > val || (v == val && c < tid));
    }
    if (rank < W) {
      const int64_t t = dn ? (stop >= 0 ? stop : 0) : (int64_t)top_ids[tid];
      s_parent[rank] = w;
      s_tok[rank] = t;
      s_score[rank] = val;
      s_done[rank] = dn || (stop >= 0 && t == stop);
      s_len[rank] = len + (dn ? 0 : 1);
    }
  }
  __syncthreads();
  if (tid < W) {
    parent[tid] = s_parent[tid];
    tok[tid] = s_tok[tid];
    scores[tid] = s_score[tid];
    done[tid] = s_done[tid];
    length[tid] = s_len[tid];
    bp_parent[n * W + tid] = s_parent[tid];
    bp_token[n * W + tid] = s_tok[tid];
    src[tid * R + n] = tid;
  }
  for (int e = tid; e < W * n; e += 256) {
    const int r = e / n, t = e - r * n;
    src[r * R + t] = anc[s_parent[r] * R + t];
  }
  if (tid == 0) {
    int all = 1;
    for (int i = 0; i < W; ++i) all &= s_done[i];
    *all_done = all;
    *n_dev = n + 1;
  }
}

}  // namespace

// nsa_decode_attn_shared (one position for the batch: pos, an int64 device scalar) for the
// hypotheses of a beam search: row b's key at row-cache slot t is read from row src[b, t] (int32
// [B, R]; values are clamped to 0 .. B - 1) instead of row b.  Same caches, workspace, output and
// append rule; the caches are only ever written at (b, *pos - *plen).
NSA_API hipError_t nsa_decode_attn_beam(const void* qkv, const void* pk, const void* pv, void* kc, void* vc,
                                        const void* src, const void* plen, const void* pos, void* ws, void* out, int B,
                                        int H, int Tp, int R, float scale, int append, hipStream_t s) {
  if (B < 1 || H < 1 || Tp < 1 || R < 1 || !src || !plen || !pos || !ws || !out) return hipErrorInvalidValue;
  const int npc = (Tp + SP_CHUNK - 1) / SP_CHUNK, nrc = (R + DA_CHUNK - 1) / DA_CHUNK;
  const int64_t grid = (int64_t)H * npc + (int64_t)B * H * nrc;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  decode_attn_beam_kernel<<<(unsigned)grid, 256, 0, s>>>(
      (const bf16_t*)qkv, (const bf16_t*)pk, (const bf16_t*)pv, (const bf16_t*)kc, (const bf16_t*)vc, (bf16_t*)kc,
      (bf16_t*)vc, (const int*)src, (const int64_t*)plen, (const int64_t*)pos, (float*)ws, B, H, Tp, R, npc, nrc,
      scale * 1.4426950408889634f, append);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (npc + nrc <= 64)
    decode_attn_combine_wide_kernel<<<B * H, 64, 0, s>>>((const float*)ws, (bf16_t*)out, H, npc + nrc);
  else
    decode_attn_combine_kernel<<<B * H, 64, 0, s>>>((const float*)ws, (bf16_t*)out, H, npc + nrc);
  return hipGetLastError();
}

// One beam-search step's bookkeeping (ops.beam_select is the rule), 2 <= W <= 8 beams, in place
// on the device: top_ids (int32) / top_lp (fp32) [W, W] are every row's W most likely ids and
// their log-probabilities; scores fp32 [W], done / length / parent int32 [W], tok int64 [W] (the
// tokens the next step feeds), src int32 [W, R], bp_parent int32 / bp_token int64 [R, W] (row n:
// the survivors' parents and tokens), n and all_done int32 scalars; stop < 0: no stop token.
NSA_API hipError_t nsa_beam_step(const void* top_ids, const void* top_lp, void* scores, void* done, void* length,
                                 void* parent, void* tok, void* src, void* bp_parent, void* bp_token, void* n,
                                 void* all_done, int W, int R, int64_t stop, hipStream_t s) {
  if (W < 2 || W > BEAM_MAX || R < 1 || (int64_t)W * R > 60000) return hipErrorInvalidValue;
  if (!top_ids || !top_lp || !scores || !done || !length || !parent || !tok || !src || !bp_parent || !bp_token ||
      !n || !all_done)
    return hipErrorInvalidValue;
  beam_step_kernel<<<1, 256, (size_t)W * R, s>>>((const int*)top_ids, (const float*)top_lp, (float*)scores,
                                                 (int*)done, (int*)length, (int*)parent, (int64_t*)tok, (int*)src,
                                                 (int*)bp_parent, (int64_t*)bp_token, (int*)n, (int*)all_done, W, R,
                                                 stop);
  return hipGetLastError();
}
