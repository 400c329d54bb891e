// The device-side bookkeeping of a speculative decode step (Decoder(..., speculate=K)): which
// of a row's K drafted tokens the model itself would have produced, and what to draft next.
// One workgroup per row, so a row advances by a variable number of positions inside a captured
// graph; nothing here is read by the host.
//
// Accept (cand != NULL).  The step fed stok[b] = (tok[b], draft[0 .. K - 1]) at positions p ..
// p + K, p = pos[b], and cand[b, j] is the id drawn from logits row (b, j), the token of
// position p + j + 1, with the stream the plain decoder uses for that position.  A draft is
// kept iff it equals that draw: n is the largest count with draft[i] == cand[i] for all i < n,
// capped so that p + n + 1 <= limit = min(T, end[b]).  cand[0 .. n] go to gen[b, p + 1 ..], cut
// after the first stop token; pos[b] moves by the number emitted, tok[b] becomes the last one,
// done[b] is set at the stop token or at the limit, and stats[b] = (live steps, drafts offered
// = the cap, drafts accepted = emitted - 1) grows.  A done row changes nothing.
//
// Draft (always, after the accept).  History h = gen[b, 0 .. p] at the new p.  With a table:
// draft[i] = table[b, min(p + 1 + i, T)].  Otherwise prompt lookup: for n = N down to 1 the
// most recent earlier occurrence of the suffix h[p - n + 1 .. p] (start s, s + n <= p) is
// continued periodically, draft[i] = h[s + n + (i mod L)], L = p + 1 - (s + n), so a loop is
// drafted whole; no match at any n: draft[i] = h[p].  The search runs over end positions e =
// s + n - 1 < p: ml(e) = the number of trailing ids (at most N and e + 1) on which h[.. e] and
// h[.. p] agree, and the winner is the largest (ml, e), which is the rule above.  The kernel
// writes the next step's fed tokens stok[b] = (tok[b], draft), their positions spos[b, j] =
// min(p + j, T - 1) (the clamp keeps the position-embedding gather in bounds; the attention
// masks such a query and it is never accepted) and cpos[b, j] = min(p + j + 1, T), the
// position each draw is keyed by.  The history sits in LDS as int32 ids, loaded with all
// requests in flight.
#include "common.h"

namespace {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_MAX_K = 7;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64), lo = __shfl_xor((uint32_t)v, o, 64);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_step_kernel(
    int64_t* __restrict__ gen, int gen_ld, int T, int64_t* __restrict__ pos, int64_t* __restrict__ tok,
    int64_t* __restrict__ done, const int64_t* __restrict__ end, const int64_t* __restrict__ cand,
    int64_t* __restrict__ stok, int64_t* __restrict__ spos, int64_t* __restrict__ cpos,
    const int64_t* __restrict__ table, int table_ld, int64_t* __restrict__ stats, int K, int N, int stop_token) {
  extern __shared__ int hist[];  // T + 1 ids
  __shared__ int sh_p;
  __shared__ int64_t sh_tok;
  __shared__ unsigned long long sh_best[SPEC_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t* g = gen + (int64_t)b * gen_ld;
  const int64_t p64 = pos[b];
  int p = (int)(p64 < 0 ? 0 : (p64 > T ? T : p64));
  // history 0 .. p into LDS: four independent loads per thread and pass
  for (int i0 = 0; i0 <= p; i0 += 4 * SPEC_THREADS) {
    int64_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = g[min(i0 + u * SPEC_THREADS + tid, p)];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * SPEC_THREADS + tid;
      if (i <= p) hist[i] = (int)v[u];
    }
  }
  if (tid == 0) {
    int64_t t = tok[b];
    if (cand && !(done && done[b] != 0)) {
      int64_t limit = T;
      if (end && end[b] < limit) limit = end[b];
      if (p + 1 > limit) {  // no position left to draw for: the row only finishes
        if (done) done[b] = 1;
      } else {
        const int cap = (int)(limit - p - 1 < K ? limit - p - 1 : K);
        const int64_t* c = cand + (int64_t)b * (K + 1);
        const int64_t* d = stok + (int64_t)b * (K + 1) + 1;
        int n = 0;
        while (n < cap && d[n] == c[n]) ++n;
        int emitted = 0;
        bool fin = false;
        for (int i = 0; i <= n && !fin; ++i) {
          const int64_t id = c[i];
          g[p + 1 + i] = id;
          hist[p + 1 + i] = (int)id;
          t = id;
          ++emitted;
          fin = id == (int64_t)stop_token;
        }
        p += emitted;
        pos[b] = p;
        tok[b] = t;
        if (done && (fin || p >= limit)) done[b] = 1;
        if (stats) {
          stats[3 * b] += 1;
          stats[3 * b + 1] += cap;
          stats[3 * b + 2] += emitted - 1;
        }
      }
    }
    sh_p = p;
    sh_tok = t;
  }
  __syncthreads();
  p = sh_p;
  // the most recent end position with the longest agreement: (ml << 32) | e, 0 = no match
  unsigned long long best = 0;
  if (!table) {
    for (int e = p - 1 - tid; e >= 0; e -= SPEC_THREADS) {
      int ml = 0;
      while (ml < N && ml <= e && hist[e - ml] == hist[p - ml]) ++ml;
      const unsigned long long k = ml ? ((unsigned long long)ml << 32) | (uint32_t)e : 0ull;
      best = k > best ? k : best;
    }
    best = wave_max_u64(best);
    if (lane == 0) sh_best[w] = best;
  }
  __syncthreads();
  if (tid <= K) {
    int64_t id = sh_tok;
    if (tid > 0) {
      const int i = tid - 1;
      if (table) {
        id = table[(int64_t)b * table_ld + min(p + 1 + i, T)];
      } else {
        best = sh_best[0];
#pragma unroll
        for (int q = 1; q < SPEC_THREADS / 64; ++q) best = sh_best[q] > best ? sh_best[q] : best;
        if (best) {
          const int e = (int)(uint32_t)best, L = p - e;
          id = hist[e + 1 + i % L];
        } else {
          id = hist[p];
        }
      }
    }
    const int64_t o = (int64_t)b * (K + 1) + tid;
    stok[o] = id;
    spos[o] = min(p + tid, T - 1);
    if (cpos) cpos[o] = min(p + tid + 1, T);
  }
}

}  // namespace

// gen: int64 [B, gen_ld] (gen_ld > T: the token fed at every position); pos, tok: int64 [B];
// done (may be NULL), end (may be NULL: the limit is T): int64 [B]; cand: int64 [B, K + 1] or
// NULL (draft only); stok, spos, cpos (may be NULL): int64 [B, K + 1]; table: int64 [B, table_ld]
// (table_ld > T) or NULL (n-gram drafts, n <= N); stats: int64 [B, 3] or NULL; stop_token < 0:
// none.  1 <= K <= 7, N >= 1, T + 1 ids must fit the LDS (T <= 16000).
NSA_API hipError_t nsa_spec_step(void* gen, int gen_ld, int T, void* pos, void* tok, void* done, const void* end,
                                 const void* cand, void* stok, void* spos, void* cpos, const void* table,
                                 int table_ld, void* stats, int B, int K, int N, int stop_token, hipStream_t s) {
  if (B < 1 || K < 1 || K > SPEC_MAX_K || N < 1 || T < 1 || T > 16000 || gen_ld <= T) return hipErrorInvalidValue;
  if (!gen || !pos || !tok || !stok || !spos || (table && table_ld <= T)) return hipErrorInvalidValue;
  spec_step_kernel<<<B, SPEC_THREADS, (size_t)(T + 1) * sizeof(int), s>>>(
      (int64_t*)gen, gen_ld, T, (int64_t*)pos, (int64_t*)tok, (int64_t*)done, (const int64_t*)end,
      (const int64_t*)cand, (int64_t*)stok, (int64_t*)spos, (int64_t*)cpos, (const int64_t*)table, table_ld,
      (int64_t*)stats, K, N, stop_token);
  return hipGetLastError();
}
