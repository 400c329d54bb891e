// Log-probabilities of given tokens under raw logits (ops.token_logprobs states the rule): one
// workgroup per row of logits [M, >= V] (fp32 or bf16, row stride ld), for the id of row r
//   lp[r] = (l[id] - m) - log(sum_j exp(l[j] - m)),  m = max_j l[j],  j over columns 0 .. V - 1,
// and, with N > 0, the N most likely ids by (logit descending, id ascending) with their
// log-probabilities.  nsa_token_logprobs, two forms: the ids form (ids int64 [M]; a row whose id
// is outside 0 .. V - 1 writes nothing) and the decoder's step form (tok, pos, last; below).
//
// One summation order for every form, dtype and addressing mode.  The row is cut into groups of 8
// consecutive columns; group g belongs to thread g % NT, which takes its groups in ascending
// order and keeps 8 accumulators, one per column of a group: column i is added to accumulator
// (i / 8 % NT, i % 8) after every smaller column of that accumulator.  The last, partial group
// (V % 8 columns) is its thread's last.  Then ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) in
// the thread, an xor butterfly over the 64 lanes and one over the NT / 64 wave sums: the order
// depends on V and NT alone, NT on V alone, so an eager launch, a replayed one, the step form and
// the scoring path give the same bits for the same row.  exp and log are expf / logf (not the bare
// v_exp_f32 / v_log_f32), and the accumulation is not contracted.  Columns past V, and the padding of
// a short row, enter as -inf: they add +0 and never win the maximum (a row's maximum must be
// finite; NaN is not supported).
//
// Block size and the two regimes.  A decode step has 1 .. 64 rows and is latency-bound; scoring
// has thousands of rows and is bound by the row's 2 V or 4 V bytes.  Both want the row read from
// memory once with every load in flight together, so where a row fits the registers it stays
// there (KEEP: 7 groups = 56 values per thread; maximum, sum and the N selection rounds all run
// over registers):
//   V <= 14336:  256 threads, KEEP.  Char-level vocabularies: 4 waves per row and several rows
//                per CU, instead of 16 waves meeting at barriers over 65 columns;
//   V <= 57344:  1024 threads, KEEP.  GPT-2's 50257 / 50304: 13 x 16 bytes in flight per thread,
//                as the sampler has;
//   larger V:    256 threads, a loop over the groups per pass (2 + N passes; the re-reads come
//                from the caches).  No cap on V.
// Loads are 16-byte vectors (two per fp32 group, one per bf16 group) when the base and the row
// stride are 16-byte aligned and V >= 8, scalar loads of the same columns otherwise; the partial
// group is always scalar.  Alternatives: N rounds of a block-wide arg-max over 64-bit keys
// (order-preserving logit bits << 32 | ~id, -0 folded into +0: logits compare as floats), each
// round taking the largest key below the previous round's.  A slot past V holds id -1 and -inf.
//
// The step form replaces ids by the decoder's state: row b's id is tok[b], its position p =
// pos[b * pos_stride], and it writes lp[b * out_ld + p], top_ids / top_lp[(b * out_ld + p) * N ..].
// last (int64 [B]) is the position the row recorded last: a row with last[b] == p records nothing
// (it was finished before this sampler call: neither its position nor its token moved), every
// other row records and sets last[b] = p (a row that finishes in this call has a new p).  The one
// thread that writes a row's outputs is the only reader and writer of last[b].  Plain stores, no atomics.
//
// kernel-resource-usage (VGPRs / VGPR spills / SGPR spills / LDS bytes), the same for fp32 and
// bf16 input and for the vector and the scalar form of each (hipcc merges the scalar form's 8
// consecutive loads itself; the forms differ in the alignment they may assume), 12 instantiations:
//   256 threads, KEEP:   155 / 0 / 0 / 48   (3 rows per SIMD set: a 256-thread block may take up to 512)
//   1024 threads, KEEP:  128 / 0 / 0 / 192  (the cap of a 1024-thread block; with the partial group held
//                                            beside the 56 values instead of among them: 18 .. 19 spilled)
//   256 threads, loop:    96 / 0 / 0 / 48
#include "common.h"

namespace {

constexpr int LP_GROUP = 8;        // columns per group = accumulators per thread
constexpr int LP_KEEP_GROUPS = 7;  // groups per thread a KEEP instantiation holds in registers
constexpr int LP_MAX_TOP = 8;

__device__ __forceinline__ uint32_t lp_fkey(float f) {  // order-preserving bits; -0 as +0
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lp_key_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ float lp_load1(const float* p) { return *p; }
__device__ __forceinline__ float lp_load1(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void lp_load8(const float* p, float (&f)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}
__device__ __forceinline__ void lp_load8(const bf16_t* p, float (&f)[8]) { load8(p, f); }

// block reductions: a butterfly over the lanes, then one over the wave results (every thread
// gets the result; red[] holds NT / 64 entries)
template <int NW>
__device__ __forceinline__ float lp_block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();  // red[] may still be read from the previous reduction
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[lane & (NW - 1)];
#pragma unroll
  for (int off = NW / 2; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
  return r;
}
template <int NW>
__device__ __forceinline__ float lp_block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[lane & (NW - 1)];
#pragma unroll
  for (int off = NW / 2; off > 0; off >>= 1) r = fmaxf(r, __shfl_xor(r, off, 64));
  return r;
}
__device__ __forceinline__ uint64_t lp_shfl_xor64(uint64_t v, int off) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
  return ((uint64_t)hi << 32) | lo;
}
template <int NW>
__device__ __forceinline__ uint64_t lp_block_max64(uint64_t v, uint64_t* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = lp_shfl_xor64(v, off);
    v = o > v ? o : v;
  }
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  uint64_t r = red[lane & (NW - 1)];
#pragma unroll
  for (int off = NW / 2; off > 0; off >>= 1) {
    const uint64_t o = lp_shfl_xor64(r, off);
    r = o > r ? o : r;
  }
  return r;
}

template <typename T, bool VEC, int NT, bool KEEP>
__global__ __launch_bounds__(NT) void logprob_kernel(
    const T* __restrict__ logits, int V, int64_t ld, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ tok, const int64_t* __restrict__ pos, int pos_stride, int64_t* last,
    float* __restrict__ lp, int32_t* __restrict__ top_ids, float* __restrict__ top_lp, int64_t out_ld, int N) {
  constexpr int NW = NT / 64;
  constexpr float NEG_INF = -__builtin_inff();
  __shared__ float redf[NW];
  __shared__ uint64_t redk[NW];
  const int b = blockIdx.x, t = threadIdx.x;
  // block-uniform exits, all before the first barrier
  int64_t id, p = 0;
  if (ids) {
    id = ids[b];
  } else {
    p = pos[(int64_t)b * pos_stride];
    if (p < 0 || p >= out_ld || last[b] == p) return;  // recorded already: the row was finished before this call
    id = tok[b];
  }
  if (id < 0 || id >= V) return;
  const T* row = logits + (int64_t)b * ld;
  const int64_t out = (int64_t)b * out_ld + p;

  const int nfull = V / LP_GROUP;           // whole groups; group nfull is the partial one
  const int ntail = V - nfull * LP_GROUP;   // its columns, owned by thread nfull % NT
  const bool tail_mine = t == nfull % NT;
  auto load_group = [&](int g, float(&f)[LP_GROUP]) {
    const T* q = row + (int64_t)g * LP_GROUP;
    if constexpr (VEC) {
      lp_load8(q, f);
    } else {
#pragma unroll
      for (int e = 0; e < LP_GROUP; ++e) f[e] = lp_load1(q + e);
    }
  };
  // KEEP: the thread's whole groups t, t + NT, .. in registers, loaded unconditionally at a
  // clamped address and masked with bit operations (a select on a loaded value becomes a branch
  // around the load, and the loads would no longer be in flight together)
  float v[KEEP ? LP_KEEP_GROUPS * LP_GROUP : 1];
  if constexpr (KEEP) {
    if (nfull > 0) {
#pragma unroll
      for (int j = 0; j < LP_KEEP_GROUPS; ++j) {
        const int g = j * NT + t;
        float f[LP_GROUP];
        load_group(min(g, nfull - 1), f);
        const uint32_t live = (uint32_t)((g - nfull) >> 31);  // all ones for g < nfull
#pragma unroll
        for (int e = 0; e < LP_GROUP; ++e)
          v[j * LP_GROUP + e] = __uint_as_float((__float_as_uint(f[e]) & live) | (0xff800000u & ~live));
      }
    } else {
#pragma unroll
      for (int i = 0; i < LP_KEEP_GROUPS * LP_GROUP; ++i) v[i] = NEG_INF;
    }
  }
  // the partial group: in a KEEP instantiation it takes its place among the thread's groups (V <= 56 NT:
  // group nfull is one of them), otherwise its owner holds it beside the loop
  float tl[KEEP ? 1 : LP_GROUP];
  if constexpr (KEEP) {
    if (ntail > 0) {  // block-uniform
#pragma unroll
      for (int j = 0; j < LP_KEEP_GROUPS; ++j)
        if (j * NT + t == nfull) {
#pragma unroll
          for (int e = 0; e < LP_GROUP; ++e)
            if (e < ntail) v[j * LP_GROUP + e] = lp_load1(row + (int64_t)nfull * LP_GROUP + e);
        }
    }
  } else {
#pragma unroll
    for (int e = 0; e < LP_GROUP; ++e) tl[e] = NEG_INF;
    if (ntail > 0 && tail_mine) {
#pragma unroll
      for (int e = 0; e < LP_GROUP; ++e)
        if (e < ntail) tl[e] = lp_load1(row + (int64_t)nfull * LP_GROUP + e);
    }
  }
  // f(e, value, column, is a column of the row) over the thread's columns, in the order of the sum
  auto scan = [&](auto&& f) {
    if constexpr (KEEP) {
#pragma unroll
      for (int j = 0; j < LP_KEEP_GROUPS; ++j) {
#pragma unroll
        for (int e = 0; e < LP_GROUP; ++e) {
          const int i = (j * NT + t) * LP_GROUP + e;
          f(e, v[j * LP_GROUP + e], i, i < V);
        }
      }
    } else {
#pragma unroll 2
      for (int g = t; g < nfull; g += NT) {
        float x[LP_GROUP];
        load_group(g, x);
#pragma unroll
        for (int e = 0; e < LP_GROUP; ++e) f(e, x[e], g * LP_GROUP + e, true);
      }
#pragma unroll
      for (int e = 0; e < LP_GROUP; ++e) f(e, tl[e], nfull * LP_GROUP + e, tail_mine && e < ntail);
    }
  };

  float mt = NEG_INF;
  scan([&](int, float x, int, bool) { mt = fmaxf(mt, x); });
  const float m = lp_block_max<NW>(mt, redf);

  float acc[LP_GROUP];
#pragma unroll
  for (int e = 0; e < LP_GROUP; ++e) acc[e] = 0.0f;
  scan([&](int e, float x, int, bool) {
#pragma clang fp contract(off)
    const float d = x - m;
    const float w = expf(d);
    acc[e] = acc[e] + w;
  });
  float st;
  {
#pragma clang fp contract(off)
    st = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
  const float logz = logf(lp_block_sum<NW>(st, redf));

  if (t == 0) {
#pragma clang fp contract(off)
    const float d = lp_load1(row + id) - m;
    lp[out] = d - logz;
    if (!ids) last[b] = p;
  }
  // the N alternatives: round r takes the largest key below round r - 1's (key 0: no column left)
  uint64_t prev = ~0ull;
  for (int r = 0; r < N; ++r) {  // N is block-uniform
    uint64_t best = 0;
    scan([&](int, float x, int i, bool real) {
      const uint64_t k = real ? ((uint64_t)lp_fkey(x) << 32) | (uint64_t)(0xffffffffu - (uint32_t)i) : 0ull;
      if (k < prev && k > best) best = k;
    });
    best = lp_block_max64<NW>(best, redk);
    prev = best;
    if (t == 0) {
#pragma clang fp contract(off)
      const float d = lp_key_val((uint32_t)(best >> 32)) - m;
      top_ids[out * N + r] = best ? (int32_t)(0xffffffffu - (uint32_t)best) : -1;
      top_lp[out * N + r] = best ? d - logz : NEG_INF;
    }
  }
}

template <typename T>
hipError_t logprob_launch(const T* logits, int M, int V, int64_t ld, const int64_t* ids, const int64_t* tok,
                          const int64_t* pos, int pos_stride, int64_t* last, float* lp, int32_t* top_ids,
                          float* top_lp, int64_t out_ld, int N, hipStream_t s) {
  const bool vec = V >= LP_GROUP && ((uintptr_t)logits & 15) == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0;
#define LP_GO(NT, KEEP)                                                                                          \
  do {                                                                                                           \
    if (vec)                                                                                                     \
      logprob_kernel<T, true, NT, KEEP><<<M, NT, 0, s>>>(logits, V, ld, ids, tok, pos, pos_stride, last, lp,      \
                                                         top_ids, top_lp, out_ld, N);                            \
    else                                                                                                         \
      logprob_kernel<T, false, NT, KEEP><<<M, NT, 0, s>>>(logits, V, ld, ids, tok, pos, pos_stride, last, lp,     \
                                                          top_ids, top_lp, out_ld, N);                           \
  } while (0)
  // the block size is a function of V alone: every form of a row sums in the same order
  if (V <= 256 * LP_KEEP_GROUPS * LP_GROUP)
    LP_GO(256, true);
  else if (V <= 1024 * LP_KEEP_GROUPS * LP_GROUP)
    LP_GO(1024, true);
  else
    LP_GO(256, false);
#undef LP_GO
  return hipGetLastError();
}

}  // namespace

// Log-probabilities of one id per row of logits [M, >= V] (bf16 != 0: bf16, else fp32; row stride ld
// elements, 0 for one row read by every workgroup; unit column stride) over columns 0 .. V - 1, and
// the N (0 .. 8) most likely ids.
// ids form (ids int64 [M]; tok, pos, last NULL): row r writes lp[r * out_ld], top_ids / top_lp
// [r * out_ld * N ..]; a row whose id is outside 0 .. V - 1 writes nothing.
// Step form (ids NULL; tok int64 [M], pos int64 [M] or [1] with pos_stride 1 or 0, last int64 [M]):
// row b writes at b * out_ld + pos[b] unless last[b] equals that position, and sets last[b] to it.
// lp float [..], top_ids int32 and top_lp float [.., N] (both may be NULL when N is 0).
NSA_API hipError_t nsa_token_logprobs(const void* logits, int bf16, int M, int V, int64_t ld, const void* ids,
                                      const void* tok, const void* pos, int pos_stride, void* last, void* lp,
                                      void* top_ids, void* top_lp, int64_t out_ld, int N, hipStream_t s) {
  if (!logits || !lp || M < 1 || V < 1 || ld < 0 || out_ld < 1 || N < 0 || N > LP_MAX_TOP)
    return hipErrorInvalidValue;
  if (N > 0 && (!top_ids || !top_lp)) return hipErrorInvalidValue;
  if (ids ? (tok || pos || last) : (!tok || !pos || !last || (pos_stride != 0 && pos_stride != 1)))
    return hipErrorInvalidValue;
  if (bf16)
    return logprob_launch((const bf16_t*)logits, M, V, ld, (const int64_t*)ids, (const int64_t*)tok,
                          (const int64_t*)pos, pos_stride, (int64_t*)last, (float*)lp, (int32_t*)top_ids,
                          (float*)top_lp, out_ld, N, s);
  return logprob_launch((const float*)logits, M, V, ld, (const int64_t*)ids, (const int64_t*)tok,
                        (const int64_t*)pos, pos_stride, (int64_t*)last, (float*)lp, (int32_t*)top_ids,
                        (float*)top_lp, out_ld, N, s);
}
