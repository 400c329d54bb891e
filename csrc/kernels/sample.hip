// Device sampling for the serving path (nanoGPT sample.py: logits / temperature, keep the
// top_k, softmax, multinomial; plus nucleus / min-p filters): one row per workgroup, one
// launch, so the decode graph can feed the sampled token back without a host round trip
// (torch's topk / multinomial chain is ~20 launches and its segmented sort is not
// graph-replay safe here).
//
// One kernel body, sample_kernel<VEC4, FILT>.  With z = l / T, K the top-k set (ties with the
// k-th largest kept, as torch's `logits < v[:, [-1]]` mask; no top-k: every id),
// w_i = exp(z_i - max z) for i in K and Z = sum w, a token is kept iff it is in K and
//   top_p:  S_gt(i) = sum { w_j : j in K, z_j > z_i } < top_p Z   (ties at the edge kept),
//   min_p:  w_i >= min_p                                            (w of the arg-max is 1).
// Each of the 1024 threads keeps up to 52 logits of the row in registers as order-preserving
// uint32 keys (element j * 1024 + t: coalesced loads), and all three filters are "key >=
// threshold", so the kept set is { key >= max(thr_k, thr_p, thr_m) }:
//   thr_k = the k-th largest key;
//   thr_m = key(max + log2(min_p) / scale_log2), known right after the row maximum;
//   thr_p = the largest key x with G(x) = mass(keys >= x) >= top_p Z.  G is evaluated by one
//           fixed summation order (per-lane partials, then a tree), so it is monotone in x
//           in floating point as well and the search is well defined.
// The draw scans the kept weights in a fixed order and picks the first whose running sum
// exceeds u = uniform * sum w (uniform from the counter hash of (salt, row, position)).
//
// Candidate path (top_k <= 1024, the serving case; a nucleus; a min-p bound alone):
//  1. one wave finds a key lo0 with k .. 2k of the 1024 per-thread maxima >= it: the row's
//     k-th largest key is >= lo0 (k distinct elements are), so every top-k element is among
//     the keys >= lo0, and those live only in threads whose maximum is >= lo0: typically
//     ~k .. 2k keys.  Without a top-k, lo0 has 832 .. 928 of the maxima >= it (~1.7k .. 2.4k
//     keys of a shuffled row) and the path is taken iff mass(keys >= lo0) >= top_p Z: then
//     S_gt of every key below lo0 is >= top_p Z and none of them is kept.  A min-p bound
//     alone is its own lo0;
//  2. the candidates are compacted into LDS in (thread, j) order (deterministic), up to 4096;
//  3. thr_k exactly among them (one wave; a block-wide 16-ary search beyond 1024
//     candidates), thr_p by the mass-weighted 16-ary block search over them (~5 rounds);
//  4. wave 0 sums the kept candidates per lane, scans the lanes and picks.
// Bisection counts are ballots + scalar popcounts (no shuffles) and stop early (at exactly k
// entries >= mid for the exact select, inside the k .. 2k window for lo0).
// Wide path (k > 1024, no filter at all, > 4096 candidates, a nucleus wider than lo0,
// all-ties rows): bisection over the register keys with one block reduction per step, then
// a block-wide scan.  A mass step re-forms the 52 weights of a thread (the registers cannot
// hold keys and weights).  32 passes over 50k keys on one CU are ~70 us per row against a
// few us on the candidate path.
//
// FILT = false is the top-k sampler (nsa_sample_topk, nsa_sample_topk_rows: the serving
// default).  It compiles away top_p, min_p and stats: the min-p bound, the mass searches
// with their weight buffer and reduction scratch (12 KiB of LDS), both stats blocks, and the
// broadcast of thr_k to the waves that only the mass search needs, and it folds the
// smallest key on the wide path instead of beside the maximum; none of the filtered
// instantiation's registers or spills.  FILT = true with top_p >= 1 and min_p <= 0 takes
// the same steps (same thresholds, same summation order), so it draws the same ids.
//
// REQ = true is the serving queue's form (nsa_sample_requests), an instantiation of its own so
// that the four above keep their registers (kernel-resource-usage, VGPRs / VGPR spills / SGPR
// spills / LDS bytes: VEC4 FILT 128 / 25 / 74 / 53700, scalar FILT 128 / 14 / 74 / 53700, VEC4
// top-k 96 / 0 / 34 / 41220, scalar top-k 124 / 0 / 34 / 41220, with and without the REQ
// parameters in the signature; the REQ forms: 128 / 21 / 78, 128 / 14 / 78, 96 / 0 / 36,
// 124 / 0 / 36).  row_key[b] replaces b in the hash, so a request draws the same stream in
// whatever row it is served, and a row that writes its id at a position >= end[b] sets done[b]
// where the stop token sets it; both are read once, the end position by the writing thread alone.
//
// PEN = true is the penalised sampler (nsa_sample_penalized; the REQ parameters always present,
// so four more instantiations).  A row's counts (int32, how often every id occurs in the row's
// text) are loaded beside its logits, int4 beside float4 with the same clamped index and live
// mask, and the key is formed from penalize(logit, count): the repetition, frequency and presence
// penalties of ops.penalize_logits, bit for bit.  Everything after the load works on the keys, so
// the row maximum, the thresholds, the masses and the draw all see the penalised row, the stats'
// smallest kept logit is a penalised one, and the wide path's last-resort re-read penalises again.
// The loads go in two groups of 7 and 6 vectors (in_groups / count_fence): 13 count vectors
// beside 13 logit vectors do not fit the 128 VGPRs of a 1024-thread block, and left alone the
// scheduler serialises the 26 loads two at a time to stay below them.  The thread that writes
// the drawn id adds 1 to counts[b, id] with a plain load and store: the row's block is the
// table row's only writer and every load of it lies before the first barrier.  A skipped row
// (done[b] != 0) reads and writes none of it.  kernel-resource-usage of the four, VGPRs / VGPR
// spills / SGPR spills / LDS bytes: VEC4 FILT 128 / 14 / 86 / 53700, scalar FILT 128 / 21 / 90 /
// 53700, VEC4 top-k 125 / 0 / 42 / 41220, scalar top-k 109 / 0 / 42 / 41220 (waves per EU capped
// at 4, what a 1024-thread block occupies anyway, for these four alone).  The eight instantiations
// above compile to the instructions they compiled to before the PEN parameters existed (the
// assembly differs in the symbol name and the kernarg size, 120 -> 144 bytes, only), with the
// figures listed above.
//
// The chosen id is written to tok[b] and gen[b, pos] (pos = *pos, or pos[b] in the per-row
// form, where a row whose done[b] is set is skipped and a row that draws stop_token sets
// it).  stats (int32 [B, 2], may be NULL): the row's kept count and the bits of its
// smallest kept logit.
#include "common.h"

namespace {

constexpr int SMP_THREADS = 1024;
constexpr int SMP_CAP = 4096;  // top-k candidates compacted into LDS

__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_val(uint32_t k) {  // inverse of fkey
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <typename T>
__device__ __forceinline__ T block_reduce(T v, T* red, bool is_max) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(v, off, 64);
    v = is_max ? (o > v ? o : v) : v + o;
  }
  __syncthreads();  // red[] may still be read from the previous reduction
  if (lane == 0) red[w] = v;
  __syncthreads();
  T r = red[0];
  for (int i = 1; i < SMP_THREADS / 64; ++i) r = is_max ? (red[i] > r ? red[i] : r) : r + red[i];
  return r;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// k-th largest selection: the largest K in [lo, hi] with #{i : a[i] >= K} >= k (the
// k-th largest of a[] when count(a >= lo) >= k and count(a >= hi + 1) < k).  Counts
// come from ballots (v_cmp into a lane mask + a scalar popcount: no cross-lane
// shuffles), so a bisection step of one wave over 16 values per lane is ~40
// instructions with lo / hi in scalar registers.  a[] is zero-padded to a multiple of
// 256 entries (key 0 is below every threshold tried, which is >= lo + 1).

// 16 entries per lane of a[0..npad) (npad <= 1024): entries 256 j + 4 lane .. +3
__device__ __forceinline__ void load16_lds(const uint32_t* a, int npad, int lane, uint32_t (&v)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 256 * j + 4 * lane;
    const uint4 q = i < npad ? *reinterpret_cast<const uint4*>(a + i) : make_uint4(0, 0, 0, 0);
    v[4 * j] = q.x;
    v[4 * j + 1] = q.y;
    v[4 * j + 2] = q.z;
    v[4 * j + 3] = q.w;
  }
}

__device__ __forceinline__ uint32_t count16(const uint32_t (&v)[16], uint32_t th) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) c += (uint32_t)__popcll(__ballot(v[j] >= th));
  return c;
}

// one wave, up to 1024 entries held as v[16] per lane, no barriers.  Exact k-th largest
// by bisection that stops as soon as exactly k entries are >= mid (the answer is then
// the smallest of them): ~log2(n) + a few steps instead of 32.
__device__ uint32_t wave_kth16(const uint32_t (&v)[16], int k, uint32_t lo, uint32_t hi) {
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  while (lo < hi) {
    const uint32_t mid = lo + (uint32_t)(((uint64_t)hi - lo + 1) / 2);
    const uint32_t c = count16(v, mid);
    if (c == (uint32_t)k) {
      uint32_t m = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < 16; ++j) m = min(m, v[j] >= mid ? v[j] : 0xffffffffu);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, off, 64));
      return __builtin_amdgcn_readfirstlane(m);
    }
    if (c > (uint32_t)k)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// one wave: some K >= lo with k <= count(v >= K) <= kcap (or the exact k-th largest when
// no such K is met), for a lower bound that only has to keep the candidate set small
__device__ uint32_t wave_bound16(const uint32_t (&v)[16], int k, int kcap, uint32_t lo, uint32_t hi) {
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  while (lo < hi) {
    const uint32_t mid = lo + (uint32_t)(((uint64_t)hi - lo + 1) / 2);
    const uint32_t c = count16(v, mid);
    if (c >= (uint32_t)k) {
      lo = mid;
      if (c <= (uint32_t)kcap) break;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

// the whole 1024-thread block, up to 4096 entries in LDS: 16-ary search, per round wave
// w counts the entries >= the (w + 1)-th of 15 interior thresholds, one barrier, every
// wave narrows [lo, hi] to the bracket (8 rounds over the 32-bit key space); cnt[]
// holds 32 words of LDS (two alternating rounds)
__device__ uint32_t block_kth_largest(const uint32_t* a, int npad, int k, uint32_t lo, uint32_t hi, uint32_t* cnt) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  int round = 0;
  while (lo < hi) {
    const uint64_t span = (uint64_t)hi - lo + 1;
    uint32_t* cr = cnt + 16 * (round & 1);
    if (w < 15) {
      const uint64_t th = (uint64_t)lo + (span * (uint64_t)(w + 1) + 15) / 16;
      uint32_t c = 0;
      if (th <= hi) {
        const uint32_t t32 = (uint32_t)th;
        for (int i = 4 * lane; i < npad; i += 256) {  // uniform trip count (npad % 256 == 0)
          const uint4 q = *reinterpret_cast<const uint4*>(a + i);
          c += (uint32_t)(__popcll(__ballot(q.x >= t32)) + __popcll(__ballot(q.y >= t32)) +
                          __popcll(__ballot(q.z >= t32)) + __popcll(__ballot(q.w >= t32)));
        }
      }
      if (lane == 0) cr[w] = c;  // 0 above hi: never chosen (count(>= hi + 1) < k)
    }
    __syncthreads();  // the other half of cnt[] was last read before this barrier
    int best = 0;  // threshold 0 is lo itself
#pragma unroll
    for (int i = 1; i < 16; ++i)
      if (cr[i - 1] >= (uint32_t)k) best = i;
    best = __builtin_amdgcn_readfirstlane(best);
    const uint32_t nlo = best == 0 ? lo : (uint32_t)((uint64_t)lo + (span * (uint64_t)best + 15) / 16);
    const uint32_t nhi = best == 15 ? hi : (uint32_t)((uint64_t)lo + (span * (uint64_t)(best + 1) + 15) / 16 - 1);
    lo = nlo;
    hi = nhi;
    ++round;
  }
  __syncthreads();  // cnt[] free for the next call
  return lo;
}

constexpr int SMP_MAXC = 52;  // logits per thread kept in registers (V <= 53248: the GPT-2 vocab is 50304)
constexpr int SMP_PEN_GROUP = 7;  // penalised sampler: logit and count vectors (scalar loads: 4 times as many) in flight per group

// one wave: mass and number of the candidates a[i] >= th (wgt[i] their weights; npad % 256
// == 0, padding has weight 0 and key 0 < th): <= 64 adds per lane, then a butterfly (every
// lane: same value); the count from ballots
__device__ __forceinline__ float wave_mass_ge(const uint32_t* a, const float* wgt, int npad, int lane, uint32_t th,
                                              uint32_t& count) {
  float s = 0.0f;
  uint32_t c = 0;
  for (int i = 4 * lane; i < npad; i += 256) {  // uniform trip count
    const uint4 q = *reinterpret_cast<const uint4*>(a + i);
    const float4 f = *reinterpret_cast<const float4*>(wgt + i);
    s += q.x >= th ? f.x : 0.0f;
    s += q.y >= th ? f.y : 0.0f;
    s += q.z >= th ? f.z : 0.0f;
    s += q.w >= th ? f.w : 0.0f;
    c += (uint32_t)(__popcll(__ballot(q.x >= th)) + __popcll(__ballot(q.y >= th)) + __popcll(__ballot(q.z >= th)) +
                    __popcll(__ballot(q.w >= th)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  count = c;
  return s;
}

// the whole block: a threshold K in [lo, hi] that keeps what the largest K' in [lo, hi]
// with mass(a >= K') >= P keeps (lo when no K' above it has that mass); 1 <= lo, and hi >=
// every a[i]; clo = #(a >= lo).  block_kth_largest with masses for counts, and the counts beside them end
// the search as soon as the bracket holds a single candidate (K' is a candidate's key, so
// the bracket's lower end keeps the same set): the key space between two logits is mostly
// empty, ~5 rounds instead of 8.  ms[] / cs[] hold 32 words each.
__device__ uint32_t block_mass_threshold(const uint32_t* a, const float* wgt, int npad, float P, uint32_t lo,
                                         uint32_t hi, uint32_t clo, float* ms, uint32_t* cs) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  clo = __builtin_amdgcn_readfirstlane(clo);  // candidates >= lo
  uint32_t chi = 0;                           // candidates >= hi + 1
  int round = 0;
  while (lo < hi && clo - chi > 1) {
    const uint64_t span = (uint64_t)hi - lo + 1;
    float* mr = ms + 16 * (round & 1);
    uint32_t* cr = cs + 16 * (round & 1);
    if (w < 15) {
      const uint64_t th = (uint64_t)lo + (span * (uint64_t)(w + 1) + 15) / 16;
      uint32_t c = chi;
      const float s = th <= hi ? wave_mass_ge(a, wgt, npad, lane, (uint32_t)th, c) : -1.0f;  // above hi: never chosen
      if (lane == 0) {
        mr[w] = s;
        cr[w] = c;
      }
    }
    __syncthreads();  // the other halves of ms[] / cs[] were last read before this barrier
    int best = 0;     // threshold 0 is lo itself
#pragma unroll
    for (int i = 1; i < 16; ++i)
      if (mr[i - 1] >= P) best = i;
    best = __builtin_amdgcn_readfirstlane(best);
    const uint32_t nlo = best == 0 ? lo : (uint32_t)((uint64_t)lo + (span * (uint64_t)best + 15) / 16);
    const uint32_t nhi = best == 15 ? hi : (uint32_t)((uint64_t)lo + (span * (uint64_t)(best + 1) + 15) / 16 - 1);
    if (best > 0) clo = cr[best - 1];
    if (best < 15) chi = cr[best];
    lo = nlo;
    hi = nhi;
    ++round;
  }
  __syncthreads();  // ms[] / cs[] free for the next call
  return lo;
}

// 2^x for the mass sums (x <= 0): the bare v_exp_f32, without exp2f's range scaling for
// results below 2^-126, which no mass comparison can see
__device__ __forceinline__ float mass_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr int SMP_NUC_LO = 832, SMP_NUC_HI = 928;  // per-thread maxima >= lo0 on the nucleus-only path

// The repetition / frequency / presence penalties on a raw logit l of an id that occurs c times in
// the row's text (ops.penalize_logits states the rule): four separately rounded fp32 operations,
// a true division and no fused multiply-add (hipcc contracts by default: switched off here), so
// the result is the torch reference's bit for bit.  Selects, no branch: the loads stay in flight.
__device__ __forceinline__ float penalize(float l, int c, float rp, float pp, float fp) {
#pragma clang fp contract(off)
  const bool s = c > 0;
  float q = l / rp;
  asm("" : "+v"(q));  // opaque: a select on a division's result is turned into a branch around the division
  const float r = l * rp;
  const float x = s ? (l > 0.0f ? q : r) : l;
  const float f = fp * (float)c;
  const float y = x - f;
  return y - (s ? pp : 0.0f);
}

// N loads in groups of G: a group's loads, then its uses.  use(j) starts with count_fence on the
// count that load(j) fetched, and program order between the fences and the count loads on either
// side of them is kept: the counts of one group are in flight together, and those of the next
// wait until this group's keys are being formed, whatever the scheduler would like to hoist.
template <int G, int N, typename Load, typename Use>
__device__ __forceinline__ void in_groups(Load load, Use use) {
#pragma unroll
  for (int g = 0; g < (N + G - 1) / G; ++g) {
#pragma unroll
    for (int j = g * G; j < ((g + 1) * G < N ? (g + 1) * G : N); ++j) load(j);
#pragma unroll
    for (int j = g * G; j < ((g + 1) * G < N ? (g + 1) * G : N); ++j) use(j);
  }
}
__device__ __forceinline__ void count_fence(int& c) { asm volatile("" : "+v"(c) : : "memory"); }
__device__ __forceinline__ void count_fence(int4& c) {
  asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(c.z), "+v"(c.w) : : "memory");
}

template <bool VEC4, bool FILT, bool REQ, bool PEN = false>
__global__ __launch_bounds__(SMP_THREADS) __attribute__((amdgpu_waves_per_eu(4, PEN ? 4 : 8))) void sample_kernel(
    const float* __restrict__ logits, int V, int ld, float scale_log2, int top_k, float top_p, float min_p,
    uint64_t salt, const uint64_t* __restrict__ salt_dev, const int64_t* __restrict__ pos, int pos_stride,
    int64_t* __restrict__ tok, int64_t* __restrict__ gen, int gen_ld, int stop_token, int64_t* done,
    int32_t* __restrict__ stats, const int64_t* __restrict__ row_key, const int64_t* __restrict__ end,
    int32_t* counts, int cnt_ld, float rp, float pp, float fp) {
  __shared__ uint32_t redu[SMP_THREADS / 64];
  __shared__ float redf[SMP_THREADS / 64];
  __shared__ __attribute__((aligned(16))) uint32_t tmx[SMP_THREADS];
  __shared__ __attribute__((aligned(16))) uint32_t ck[SMP_CAP];
  __shared__ int ci[SMP_CAP];
  // the wide path's scan; with FILT also the candidate weights
  __shared__ __attribute__((aligned(16))) float cw[FILT ? SMP_CAP : SMP_THREADS];
  __shared__ uint32_t cnt16[32];
  __shared__ float ms16[32];
  __shared__ uint32_t lo_sh;
  __shared__ uint32_t wtot[SMP_THREADS / 64];
  float* scan = cw;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  // a finished row draws nothing: tok[b], gen, done[b] and stats stay as they are (block-uniform
  // exit before the first barrier; done[b] is only ever written by this row's own block)
  if (done && done[b] != 0) return;
  const float* row = logits + (int64_t)b * ld;
  // PEN: the row of the count table, read beside the logits and written once, by the thread that picks
  int32_t* crow = PEN ? counts + (int64_t)b * cnt_ld : nullptr;
  // element j * 1024 + t stays in registers as an order-preserving key (key 0 = padding,
  // below every real key)
  uint32_t key[SMP_MAXC];
  if (PEN && VEC4) {
    // the logits as below, with the counts of the same four ids beside them (int4 beside float4,
    // the same clamped index and live mask), group by group: a count register dies as soon as its
    // key exists, and 13 count vectors beside 13 logit vectors would not fit 128 VGPRs
    const float4* row4 = reinterpret_cast<const float4*>(row);
    const int4* crow4 = reinterpret_cast<const int4*>(crow);
    const int V4 = V / 4;
    float4 v[SMP_MAXC / 4];
    int4 c[SMP_MAXC / 4];
    in_groups<SMP_PEN_GROUP, SMP_MAXC / 4>(
        [&](int j) {
          v[j] = row4[min(j * SMP_THREADS + t, V4 - 1)];
          c[j] = crow4[min(j * SMP_THREADS + t, V4 - 1)];
        },
        [&](int j) {
          count_fence(c[j]);
          const uint32_t live = (uint32_t)((j * SMP_THREADS + t - V4) >> 31);
          key[4 * j + 0] = fkey(penalize(v[j].x, c[j].x, rp, pp, fp)) & live;
          key[4 * j + 1] = fkey(penalize(v[j].y, c[j].y, rp, pp, fp)) & live;
          key[4 * j + 2] = fkey(penalize(v[j].z, c[j].z, rp, pp, fp)) & live;
          key[4 * j + 3] = fkey(penalize(v[j].w, c[j].w, rp, pp, fp)) & live;
        });
  } else if (PEN) {
    float v[SMP_MAXC];
    int c[SMP_MAXC];
    in_groups<4 * SMP_PEN_GROUP, SMP_MAXC>(
        [&](int j) {
          v[j] = row[min(j * SMP_THREADS + t, V - 1)];
          c[j] = crow[min(j * SMP_THREADS + t, V - 1)];
        },
        [&](int j) {
          count_fence(c[j]);
          key[j] = fkey(penalize(v[j], c[j], rp, pp, fp)) & (uint32_t)((j * SMP_THREADS + t - V) >> 31);
        });
  } else if (VEC4) {  // element 4 * (j * 1024 + t) + e: 13 coalesced 16-byte loads per thread
    const float4* row4 = reinterpret_cast<const float4*>(row);
    const int V4 = V / 4;
#pragma unroll
    for (int j = 0; j < SMP_MAXC / 4; ++j) {
      const int i4 = j * SMP_THREADS + t;
      // unconditional clamped loads, all in flight together, and an AND mask rather than
      // a select (a select on a loaded value is turned into a branch around the load)
      const float4 v = row4[min(i4, V4 - 1)];
      const uint32_t live = (uint32_t)((i4 - V4) >> 31);  // all ones for i4 < V4
      key[4 * j + 0] = fkey(v.x) & live;
      key[4 * j + 1] = fkey(v.y) & live;
      key[4 * j + 2] = fkey(v.z) & live;
      key[4 * j + 3] = fkey(v.w) & live;
    }
  } else {  // element j * 1024 + t
#pragma unroll
    for (int j = 0; j < SMP_MAXC; ++j) {
      const int i = j * SMP_THREADS + t;
      const float v = row[min(i, V - 1)];
      key[j] = fkey(v) & (uint32_t)((i - V) >> 31);
    }
  }
  // key 0 is padding: every real key is > 0 (fkey sets the top bit or inverts a negative)
  // The smallest real key is wanted by the wide path alone.  Without FILT it is folded there,
  // off the candidate path that serving takes (folded here it cost that path 0.3 us of its
  // 15.7); with FILT it stays beside the maximum: folded late, the scalar-load instantiation
  // spills 20 VGPRs instead of 14.
  uint32_t kmax = 0, kmin = 0xffffffffu;
  auto fold_min = [&](int j) { kmin = min(kmin, key[j] ? key[j] : 0xffffffffu); };
#pragma unroll
  for (int j = 0; j < SMP_MAXC; ++j) {
    kmax = max(kmax, key[j]);
    if (FILT) fold_min(j);
  }
  const uint32_t tmax = kmax;
  kmax = block_reduce<uint32_t>(kmax, redu, true);
  const float m = key_val(kmax);
  const int p = (int)pos[(int64_t)b * pos_stride];  // shared (stride 0) or per-row (stride 1) position
  // the device salt (when given) is read at run time, so a captured sampling graph draws a
  // fresh stream whenever the caller rewrites it (one per generate call)
  const uint64_t sl = salt ^ (salt_dev ? *salt_dev : 0ull);
  // the stream is the row's, or (row_key) the request's: the same draws in whatever row it is served
  const uint64_t hk = REQ && row_key ? (uint64_t)row_key[b] : (uint64_t)b;
  const uint32_t hsh = nsa_hash(nsa_seed(sl), hk * 0x9E3779B97F4A7C15ull + (uint64_t)p);
  const float unif = (float)(hsh >> 8) * (1.0f / 16777216.0f);

  const bool use_k = top_k > 0 && top_k < V;
  const bool use_p = FILT && top_p < 1.0f;
  // min-p as a key threshold: w >= min_p  <=>  l >= max + log2(min_p) / scale_log2 (<= max)
  uint32_t thr_m = 0;
  if (FILT && min_p > 0.0f) {
    float lm = m + log2f(min_p) / scale_log2;
    if (lm == 0.0f) lm = -0.0f;  // a logit of -0 equals the bound
    thr_m = min(fkey(lm), kmax);
  }
  // mass of the register keys >= th (th >= 1: padding is never weighed): 52 adds per
  // thread, then the block tree; the same order for every th
  auto mass_ge = [&](uint32_t th) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < SMP_MAXC; ++j) s += key[j] >= th ? mass_exp2((key_val(key[j]) - m) * scale_log2) : 0.0f;
    return block_reduce<float>(s, redf, false);
  };
  float zall = 0.0f;  // Z over every key (nucleus without a top-k): mass_ge(1), formed below

  // candidate path: a lower bound lo0 of the final threshold with few keys >= it
  bool cand = false;
  uint32_t lo0 = 1;
  if (use_k ? top_k <= SMP_THREADS : use_p) {
    tmx[t] = tmax;
    __syncthreads();
    if (w == 0) {
      uint32_t v[16];
      load16_lds(tmx, SMP_THREADS, lane, v);
      // any K with k <= #(thread maxima >= K) bounds the row's k-th largest from below;
      // up to 2k maxima above it keep the candidate set small
      const uint32_t r = use_k ? wave_bound16(v, top_k, 2 * top_k, 0u, kmax)
                               : wave_bound16(v, SMP_NUC_LO, SMP_NUC_HI, 0u, kmax);
      if (lane == 0) lo_sh = r;
    }
    __syncthreads();
    lo0 = lo_sh;
    cand = true;
    if (!use_k) {
      lo0 = max(lo0, 1u);  // small rows: threads without a key have maximum 0 (padding)
      // Z and the mass at and above lo0 in one pass over the keys (the sums of mass_ge(1)
      // and mass_ge(lo0), term for term)
      float sa = 0.0f, sh = 0.0f;
#pragma unroll
      for (int j = 0; j < SMP_MAXC; ++j) {
        const float wj = mass_exp2((key_val(key[j]) - m) * scale_log2);
        sa += key[j] >= 1u ? wj : 0.0f;
        sh += key[j] >= lo0 ? wj : 0.0f;
      }
      zall = block_reduce<float>(sa, redf, false);
      // below lo0 nothing is kept iff the keys >= lo0 already hold top_p Z; a min-p
      // bound at or above lo0 cuts there whatever the nucleus is
      if (thr_m >= lo0)
        lo0 = thr_m;
      else
        cand = block_reduce<float>(sh, redf, false) >= top_p * zall;
    }
  } else if (!use_k && thr_m > 0) {
    lo0 = thr_m;
    cand = true;
  }
  if (cand) {  // block-uniform
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < SMP_MAXC; ++j) c += key[j] >= lo0 ? 1u : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t woff = 0, n = 0;
    for (int i = 0; i < SMP_THREADS / 64; ++i) {
      woff += i < w ? wtot[i] : 0u;
      n += wtot[i];
    }
    if (n <= (uint32_t)SMP_CAP) {  // block-uniform
      uint32_t q = woff + incl - c;
      int tt = t;
      asm volatile("" : "+v"(tt));  // opaque: the element ids below are recomputed, not kept live from the loads
#pragma unroll
      for (int j = 0; j < SMP_MAXC; ++j)
        if (key[j] >= lo0) {
          ck[q] = key[j];
          ci[q] = VEC4 ? 4 * ((j >> 2) * SMP_THREADS + tt) + (j & 3) : j * SMP_THREADS + tt;
          ++q;
        }
      const int npad = ((int)n + 255) & ~255;
      for (int i = (int)n + t; i < npad; i += SMP_THREADS) ck[i] = 0u;  // zero padding
      __syncthreads();
      uint32_t thr_k = lo0;  // no top-k: every candidate is in K
      if (use_k) {
        if (npad > 1024) {
          thr_k = block_kth_largest(ck, npad, top_k, lo0, kmax, cnt16);
        } else {
          if (w == 0) {
            uint32_t v[16];
            load16_lds(ck, npad, lane, v);
            thr_k = wave_kth16(v, top_k, lo0, kmax);
            if (FILT && lane == 0) lo_sh = thr_k;  // lo0 was read before the barriers above
          }
          if (FILT) {  // the mass search needs it in every wave; otherwise only wave 0 goes on
            __syncthreads();
            thr_k = lo_sh;
          }
        }
      }
      uint32_t thr = max(thr_k, thr_m);
      if (use_p) {
        for (int i = t; i < npad; i += SMP_THREADS)
          cw[i] = ck[i] ? mass_exp2((key_val(ck[i]) - m) * scale_log2) : 0.0f;
        __syncthreads();
        uint32_t nk = n;  // candidates in K
        const float Z = use_k ? wave_mass_ge(ck, cw, npad, lane, thr_k, nk) : zall;
        thr = max(thr, block_mass_threshold(ck, cw, npad, top_p * Z, thr_k, kmax, nk, ms16, cnt16));
      }
      if (w == 0) {
        const int per = ((int)n + 63) / 64, c0 = min((int)n, lane * per), c1 = min((int)n, c0 + per);
        float sum = 0.0f;
        uint32_t kept = 0, klow = 0xffffffffu;
        for (int i = c0; i < c1; ++i)
          if (ck[i] >= thr) {
            sum += exp2f((key_val(ck[i]) - m) * scale_log2);
            ++kept;
            klow = min(klow, ck[i]);
          }
        if (FILT && stats) {  // block-uniform
          kept = wave_sum_u32(kept);
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) klow = min(klow, (uint32_t)__shfl_xor((int)klow, off, 64));
          if (lane == 0) {
            stats[2 * b] = (int32_t)kept;
            stats[2 * b + 1] = (int32_t)__float_as_uint(key_val(klow));
          }
        }
        float run = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float o = __shfl_up(run, off, 64);
          if (lane >= off) run += o;
        }
        float before = __shfl_up(run, 1, 64);
        if (lane == 0) before = 0.0f;
        const float total = __shfl(run, 63, 64);
        const float u = unif * total;
        if ((u >= before && u < run) || (lane == 63 && u >= total)) {
          int pick = -1;
          float acc = before;
          for (int i = c0; i < c1; ++i) {
            if (ck[i] >= thr) {
              acc += exp2f((key_val(ck[i]) - m) * scale_log2);
              pick = ci[i];
              if (acc > u) break;
            }
          }
          for (int i = (int)n - 1; pick < 0 && i >= 0; --i)  // u >= total on an empty last chunk
            if (ck[i] >= thr) pick = ci[i];
          tok[b] = pick;
          gen[(int64_t)b * gen_ld + p] = pick;
          if (PEN && pick >= 0) crow[pick] = crow[pick] + 1;  // the row's only writer; its loads are behind a barrier
          // stop_token < 0: never (pick >= 0); end: the row's last position (read by the writer alone)
          if (done && (pick == stop_token || (REQ && end && (int64_t)p >= end[b]))) done[b] = 1;
        }
      }
      return;
    }
  }

  // wide path: every search runs over the register keys
  uint32_t thr = 1;  // keep every real key
  // the smallest real key, where the searches start (FILT: reduced whether or not one runs;
  // a condition on use_p here costs the VEC4 instantiation two more spilled VGPRs)
  uint32_t klo = 1;
  if (FILT || use_k) {
    if (!FILT) {
#pragma unroll
      for (int j = 0; j < SMP_MAXC; ++j) fold_min(j);
    }
    klo = ~block_reduce<uint32_t>(~kmin, redu, true);
  }
  if (use_k) {
    // exact k-th largest key by bisection over [key(min), key(max)]: the largest K with
    // count(key >= K) >= k; counts from registers, one block reduction per step
    uint32_t lo = klo, hi = kmax;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < SMP_MAXC; ++j) c += key[j] >= mid ? 1u : 0u;
      if (block_reduce<uint32_t>(c, redu, false) >= (uint32_t)top_k)
        lo = mid;
      else
        hi = mid - 1;
    }
    thr = lo;  // ties with the k-th largest are kept
  }
  if (use_p) {
    // the largest key x with G(x) >= top_p Z, from the k-th largest (or the smallest) key
    // or the min-p bound upwards: G is at most top_p Z below a bound that already cuts
    const float P = top_p * (use_k ? mass_ge(thr) : zall);
    uint32_t lo = max(max(thr, klo), thr_m), hi = kmax;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (mass_ge(mid) >= P)
        lo = mid;
      else
        hi = mid - 1;
    }
    thr = lo;
  }
  thr = max(thr, thr_m);
  float part = 0.0f;
  uint32_t kept = 0, klow = 0xffffffffu;
#pragma unroll
  for (int j = 0; j < SMP_MAXC; ++j)
    if (key[j] >= thr) {
      part += exp2f((key_val(key[j]) - m) * scale_log2);
      ++kept;
      klow = min(klow, key[j]);
    }
  if (FILT && stats) {  // block-uniform
    kept = block_reduce<uint32_t>(kept, redu, false);
    klow = ~block_reduce<uint32_t>(~klow, redu, true);
    if (t == 0) {
      stats[2 * b] = (int32_t)kept;
      stats[2 * b + 1] = (int32_t)__float_as_uint(key_val(klow));
    }
  }
  scan[t] = part;
  __syncthreads();
  // inclusive scan of the per-thread sums (Hillis-Steele over 1024 entries)
  for (int off = 1; off < SMP_THREADS; off <<= 1) {
    const float v = t >= off ? scan[t - off] : 0.0f;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const float total = scan[SMP_THREADS - 1];
  const float u = unif * total;
  const float before = t > 0 ? scan[t - 1] : 0.0f;
  // exactly one thread owns the crossing (u in [before, scan[t])); u >= total (rounding)
  // falls to the last thread
  const bool mine = (u >= before && u < scan[t]) || (t == SMP_THREADS - 1 && u >= total);
  if (mine) {
    int pick = -1, tt = t;
    asm volatile("" : "+v"(tt));
    float acc = before;
    bool found = false;
#pragma unroll
    for (int j = 0; j < SMP_MAXC; ++j) {
      if (!found && key[j] >= thr) {
        acc += exp2f((key_val(key[j]) - m) * scale_log2);
        pick = VEC4 ? 4 * ((j >> 2) * SMP_THREADS + tt) + (j & 3) : j * SMP_THREADS + tt;
        found = acc > u;
      }
    }
    if (pick < 0) {  // no kept element in this thread (u >= total on the last one): any kept one
      for (int i = V - 1; i >= 0; --i)
        if (fkey(PEN ? penalize(row[i], crow[i], rp, pp, fp) : row[i]) >= thr) {
          pick = i;
          break;
        }
    }
    tok[b] = pick;
    gen[(int64_t)b * gen_ld + p] = pick;
    if (PEN && pick >= 0) crow[pick] = crow[pick] + 1;
    if (done && (pick == stop_token || (REQ && end && (int64_t)p >= end[b]))) done[b] = 1;
  }
}

// the one launch of every entry point; filt: the instantiation with top_p, min_p and stats
hipError_t sample_launch(bool filt, const void* logits, int B, int V, int ld, float temperature, int top_k,
                         uint64_t salt, const void* salt_dev, const void* pos, int pos_stride, void* tok, void* gen,
                         int gen_ld, int stop_token, void* done, float top_p, float min_p, void* stats,
                         const void* row_key, const void* end, hipStream_t s, void* counts = nullptr, int cnt_ld = 0,
                         float rp = 1.0f, float pp = 0.0f, float fp = 0.0f) {
  if (B < 1 || V < 1 || V > SMP_THREADS * SMP_MAXC || !(temperature > 0.0f)) return hipErrorInvalidValue;
  if (pos_stride != 0 && pos_stride != 1) return hipErrorInvalidValue;
  if (!(top_p > 0.0f && top_p <= 1.0f) || !(min_p >= 0.0f && min_p < 1.0f)) return hipErrorInvalidValue;
  if (end && !done) return hipErrorInvalidValue;  // an end position finishes a row through its flag
  bool vec4 = V % 4 == 0 && ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  if (counts) {  // the penalised sampler reads int4 counts beside the float4 logits
    const auto finite = [](float x) { return x - x == 0.0f; };  // false for an infinity and for NaN
    if (cnt_ld < V || !(rp > 0.0f) || !finite(rp) || !finite(pp) || !finite(fp)) return hipErrorInvalidValue;
    vec4 = vec4 && cnt_ld % 4 == 0 && ((uintptr_t)counts & 15) == 0;
  }
  // REQ (a row key or an end position is given) is an instantiation of its own: the four others
  // compile both away and keep their registers
  const bool req = row_key || end;
  const auto kernel =
      counts ? (filt ? (vec4 ? sample_kernel<true, true, true, true> : sample_kernel<false, true, true, true>)
                     : (vec4 ? sample_kernel<true, false, true, true> : sample_kernel<false, false, true, true>))
      : req ? (filt ? (vec4 ? sample_kernel<true, true, true> : sample_kernel<false, true, true>)
                    : (vec4 ? sample_kernel<true, false, true> : sample_kernel<false, false, true>))
            : (filt ? (vec4 ? sample_kernel<true, true, false> : sample_kernel<false, true, false>)
                    : (vec4 ? sample_kernel<true, false, false> : sample_kernel<false, false, false>));
  kernel<<<B, SMP_THREADS, 0, s>>>((const float*)logits, V, ld, 1.4426950408889634f / temperature, top_k, top_p, min_p,
                                   salt, (const uint64_t*)salt_dev, (const int64_t*)pos, pos_stride, (int64_t*)tok,
                                   (int64_t*)gen, gen_ld, stop_token, (int64_t*)done, (int32_t*)stats,
                                   (const int64_t*)row_key, (const int64_t*)end, (int32_t*)counts, cnt_ld, rp, pp, fp);
  return hipGetLastError();
}

// Token histograms for the count table: workgroup i counts the first lengths[i] (NULL: S) ids of
// idx[i, :] into row rows[i] (NULL: i) of counts, after zeroing the row's V entries unless
// accumulate is set.  Ids outside 0 .. V - 1 are not counted, and a row outside 0 .. B - 1 is left out.
constexpr int CNT_THREADS = 256;

__global__ __launch_bounds__(CNT_THREADS) void token_counts_kernel(
    const int64_t* __restrict__ idx, int S, const int64_t* __restrict__ lengths, const int64_t* __restrict__ rows,
    int32_t* __restrict__ counts, int B, int ld, int V, int accumulate) {
  const int i = blockIdx.x, t = threadIdx.x;
  const int64_t r = rows ? rows[i] : (int64_t)i;
  if (r < 0 || r >= B) return;  // block-uniform, before the barrier
  int32_t* crow = counts + r * ld;
  if (!accumulate) {
    for (int v = t; v < V; v += CNT_THREADS) crow[v] = 0;
    __syncthreads();  // one workgroup owns the row: its zeros are in place before its adds
  }
  const int64_t len = lengths ? lengths[i] : (int64_t)S;
  const int n = (int)(len < 0 ? 0 : len > S ? S : len);
  const int64_t* src = idx + (int64_t)i * S;
  for (int j = t; j < n; j += CNT_THREADS) {
    const int64_t id = src[j];
    if (id >= 0 && id < V) atomicAdd(crow + id, 1);
  }
}

}  // namespace

// Top-k / temperature sampling of logits [B, V] (fp32, row stride ld) on the device:
// writes tok[b] and gen[b * gen_ld + *pos].  top_k <= 0 keeps every logit.  The uniform is a
// counter hash of (salt ^ *salt_dev, row, position); salt_dev may be NULL.
NSA_API hipError_t nsa_sample_topk(const void* logits, int B, int V, int ld, float temperature, int top_k,
                                   uint64_t salt, const void* salt_dev, const void* pos, void* tok, void* gen,
                                   int gen_ld, hipStream_t s) {
  return sample_launch(false, logits, B, V, ld, temperature, top_k, salt, salt_dev, pos, 0, tok, gen, gen_ld, -1,
                       nullptr, 1.0f, 0.0f, nullptr, nullptr, nullptr, s);
}

// The per-row form: row b draws at position pos[b * pos_stride] (pos_stride 1: int64[B];
// 0: one shared position).  done (int64[B], may be NULL): a row with done[b] != 0 is
// skipped (tok[b], gen and done[b] untouched); a row that draws stop_token (< 0: none)
// sets done[b] = 1 after writing the id.
NSA_API hipError_t nsa_sample_topk_rows(const void* logits, int B, int V, int ld, float temperature, int top_k,
                                        uint64_t salt, const void* salt_dev, const void* pos, int pos_stride,
                                        void* tok, void* gen, int gen_ld, int stop_token, void* done, hipStream_t s) {
  return sample_launch(false, logits, B, V, ld, temperature, top_k, salt, salt_dev, pos, pos_stride, tok, gen, gen_ld,
                       stop_token, done, 1.0f, 0.0f, nullptr, nullptr, nullptr, s);
}

// Top-k, nucleus and min-p sampling: top_p in (0, 1] (1: off), min_p in [0, 1) (0: off), the
// rest as nsa_sample_topk_rows.  stats (int32 [B, 2], may be NULL): the kept count and the
// bits of the smallest kept logit of every row that drew.
NSA_API hipError_t nsa_sample_filtered(const void* logits, int B, int V, int ld, float temperature, int top_k,
                                       float top_p, float min_p, uint64_t salt, const void* salt_dev, const void* pos,
                                       int pos_stride, void* tok, void* gen, int gen_ld, int stop_token, void* done,
                                       void* stats, hipStream_t s) {
  return sample_launch(true, logits, B, V, ld, temperature, top_k, salt, salt_dev, pos, pos_stride, tok, gen, gen_ld,
                       stop_token, done, top_p, min_p, stats, nullptr, nullptr, s);
}

// The serving queue's form: filt != 0 is nsa_sample_filtered (top_p, min_p, stats), otherwise
// nsa_sample_topk_rows, with two more per-row inputs, either of which may be NULL.  row_key
// (int64 [B]): the hash takes row_key[b] where it takes b, so a request draws the same stream
// in whatever row it is served.  end (int64 [B]; needs done): a row that has written its id at
// position p sets done[b] = 1 if p >= end[b], where the stop token sets it.
NSA_API hipError_t nsa_sample_requests(const void* logits, int B, int V, int ld, float temperature, int top_k,
                                       int filt, float top_p, float min_p, uint64_t salt, const void* salt_dev,
                                       const void* pos, int pos_stride, void* tok, void* gen, int gen_ld,
                                       int stop_token, void* done, void* stats, const void* row_key, const void* end,
                                       hipStream_t s) {
  if (!filt && (top_p != 1.0f || min_p != 0.0f || stats)) return hipErrorInvalidValue;
  return sample_launch(filt != 0, logits, B, V, ld, temperature, top_k, salt, salt_dev, pos, pos_stride, tok, gen,
                       gen_ld, stop_token, done, top_p, min_p, stats, row_key, end, s);
}

// The penalised sampler: nsa_sample_requests (row_key and end may be NULL) on logits that the
// kernel penalises as it loads them.  counts (int32 [B, cnt_ld], cnt_ld >= V): counts[b, v] is how
// often id v occurs in row b's text; with c = counts[b, v] and s = c > 0 a logit l is drawn as
//   ((s ? (l > 0 ? l / rp : l * rp) : l) - fp * c) - (s ? pp : 0),
// every operation rounded on its own (ops.penalize_logits), and the thread that writes the drawn
// id adds 1 to counts[b, id].  A row with done[b] != 0 neither reads nor writes its counts.  rp
// finite and > 0, pp and fp finite.
NSA_API hipError_t nsa_sample_penalized(const void* logits, int B, int V, int ld, float temperature, int top_k,
                                        int filt, float top_p, float min_p, uint64_t salt, const void* salt_dev,
                                        const void* pos, int pos_stride, void* tok, void* gen, int gen_ld,
                                        int stop_token, void* done, void* stats, const void* row_key, const void* end,
                                        void* counts, int cnt_ld, float rp, float pp, float fp, hipStream_t s) {
  if (!counts) return hipErrorInvalidValue;
  if (!filt && (top_p != 1.0f || min_p != 0.0f || stats)) return hipErrorInvalidValue;
  return sample_launch(filt != 0, logits, B, V, ld, temperature, top_k, salt, salt_dev, pos, pos_stride, tok, gen,
                       gen_ld, stop_token, done, top_p, min_p, stats, row_key, end, s, counts, cnt_ld, rp, pp, fp);
}

// Histograms of n prompts idx [n, S] (int64) into rows of the count table counts (int32 [B, V], row
// stride ld >= V): prompt i's first lengths[i] ids (int64 [n]; NULL: all S) into row rows[i]
// (int64 [n], distinct; NULL: row i), which is zeroed first unless accumulate != 0.  One launch,
// one workgroup per prompt.
NSA_API hipError_t nsa_token_counts(const void* idx, int n, int S, const void* lengths, const void* rows, void* counts,
                                    int B, int ld, int V, int accumulate, hipStream_t s) {
  if (n < 1 || S < 1 || B < 1 || V < 1 || ld < V || !idx || !counts) return hipErrorInvalidValue;
  token_counts_kernel<<<n, CNT_THREADS, 0, s>>>((const int64_t*)idx, S, (const int64_t*)lengths, (const int64_t*)rows,
                                                (int32_t*)counts, B, ld, V, accumulate);
  return hipGetLastError();
}
