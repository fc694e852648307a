// sampling.hip — the logits epilogue of DecodingTask._main_loop (whisper/decoding.py:696-703) for
// greedy decoding, as two small kernels per step (vocabulary-parallel partials, per-row decision) with
// no host synchronisation:
//   the stock logit rules and the timestamp mass rule (logit_rules.h)
//   -> GreedyDecoder.update at temperature 0 (decoding.py:277-293): argmax, log_softmax of the *filtered* logits,
//   sum_logprobs accumulation for rows not yet at EOT, EOT stickiness.
// What the rules need of a row's token history sits in `row_state`, kept up to date by the final kernel.
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "logit_rules.h"
#include "sample_noise.h"

namespace {

using namespace whk;

constexpr int SCHUNK = 1024;   // vocabulary entries per stage-1 workgroup (256 threads x 4)

// Temperature sampling (GreedyDecoder.update at temperature > 0, decoding.py:281-283: Categorical(logits / T).sample())
// as a Gumbel-max draw: argmax over the filtered entries of x / T + g, g = -log(-log(u)), u from a counter-based hash of
// (seed, step, row, token) — one uniform per entry, no state, the same partial / final kernel structure as the arg-max.
// The log-probability that is accumulated is the one of the UNSCALED filtered logits (decoding.py:285-287).
struct Pick {           // best perturbed key of a range: key, the entry's logit, its index; default: the empty range
  float key = WH_NEG_INF, x = WH_NEG_INF; int idx = 0x7fffffff;
};
__device__ __forceinline__ void pick_merge(Pick& a, float key, float x, int idx) {
  if (idx == 0x7fffffff) return;
  if (a.idx == 0x7fffffff || key > a.key || (key == a.key && idx < a.idx)) { a.key = key; a.x = x; a.idx = idx; }
}
__device__ __forceinline__ void pick_wave_reduce(Pick& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float key = __shfl_xor(a.key, o, 64);
    const float x = __shfl_xor(a.x, o, 64);
    const int idx = __shfl_xor(a.idx, o, 64);
    pick_merge(a, key, x, idx);
  }
}
// the two ranges of a 256-thread workgroup in LDS, beside BlockStats (logit_rules.h): `publish` in front of its barrier
struct BlockPicks {
  float key[2][4], x[2][4]; int idx[2][4];
  __device__ __forceinline__ void publish(Pick (&pk)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      pick_wave_reduce(pk[g]);
      if (lane == 0) { key[g][wave] = pk[g].key; x[g][wave] = pk[g].x; idx[g][wave] = pk[g].idx; }
    }
  }
  __device__ __forceinline__ Pick range(int g) const {
    Pick p;
    for (int w = 0; w < 4; ++w) pick_merge(p, key[g][w], x[g][w], idx[g][w]);
    return p;
  }
};
// standard Gumbel noise for (seed, step, row, token): hash and uniform of sample_noise.h.  The 23-bit uniform lies in
// [2^-24, 1 - 2^-24], strictly inside (0, 1) in fp32, so the noise is finite: about [-2.81, 16.64]
__device__ __forceinline__ float gumbel(uint32_t seed_lo, uint32_t seed_hi, int step, int row, int v) {
  const float u = sample_uniform_of_hash(sample_hash(seed_lo, seed_hi, step, row, v));
  return -logf(-logf(u));
}
constexpr int PSTRIDE = 8;      // floats per (row, chunk, range) partial: m, s, idx | key, x (sampling) | m, s, t (STATS)

// Per-token statistics (kernels.h TokenStatArgs).  The entropy of a range follows from a third online statistic next to
// {m, s}: t = sum (x - m) exp(x - m), so that H = -sum p log p = log s - t / s.  A shift of the maximum by d = m_old - m_new
// (<= 0) maps s -> s exp(d) and t -> (t + d s) exp(d).  It is a statistic of its own, with its own {m, s}: Stat<> and with it
// the chosen token, its log-probability and the beam kernels stay what they are.  t <= 0 and s >= 1 hold in fp32 as they do
// exactly (every term added is <= 0 resp. the maximum's own 1 is never scaled), so the entropy is never negative.
// The empty range is m = -inf and is never shifted: -inf - x times s = 0 would be NaN.
struct EStat { float m = WH_NEG_INF, s = 0.f, t = 0.f; };
__device__ __forceinline__ void estat_add(EStat& a, float x) {
  if (x == WH_NEG_INF) return;
  if (a.m == WH_NEG_INF) { a.m = x; a.s = 1.0f; a.t = 0.f; return; }
  if (x > a.m) { const float d = a.m - x, e = expf(d); a.t = (a.t + d * a.s) * e; a.s = a.s * e + 1.0f; a.m = x; }
  else { const float d = x - a.m, e = expf(d); a.s += e; a.t += d * e; }
}
__device__ __forceinline__ void estat_merge(EStat& a, const EStat& b) {
  if (b.m == WH_NEG_INF) return;
  if (a.m == WH_NEG_INF) { a = b; return; }
  if (b.m > a.m) { const float d = a.m - b.m, e = expf(d); a.t = (a.t + d * a.s) * e + b.t; a.s = a.s * e + b.s; a.m = b.m; }
  else { const float d = b.m - a.m, e = expf(d); a.t += (b.t + d * b.s) * e; a.s += b.s * e; }
}
struct BlockEStats {            // beside BlockStats, like BlockPicks: `publish` in front of its barrier
  float m[2][4], s[2][4], t[2][4];
  __device__ __forceinline__ void publish(EStat (&st)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)
        estat_merge(st[g], EStat{__shfl_xor(st[g].m, o, 64), __shfl_xor(st[g].s, o, 64), __shfl_xor(st[g].t, o, 64)});
      if (lane == 0) { m[g][wave] = st[g].m; s[g][wave] = st[g].s; t[g][wave] = st[g].t; }
    }
  }
  __device__ __forceinline__ EStat range(int g) const {
    EStat r;
    for (int w = 0; w < 4; ++w) estat_merge(r, EStat{m[g][w], s[g][w], t[g][w]});
    return r;
  }
};
constexpr int TOPMAX = whk::TOKEN_STATS_MAX_TOP;
constexpr int TOP_CHUNKS = 64;                       // chunks whose best entries the final kernel can pool
constexpr int TOP_POOL = 2 * TOP_CHUNKS * TOPMAX;    // both ranges x chunks x top_k
// the chunks' best entries in TokenStatArgs::scratch: values [R][nchunk][2][TOPMAX], then indices likewise
__device__ __forceinline__ float* top_part_val(const whk::TokenStatArgs& ts) { return (float*)ts.scratch; }
__device__ __forceinline__ int* top_part_idx(const whk::TokenStatArgs& ts, int R, int nchunk) {
  return (int*)ts.scratch + (int64_t)R * nchunk * 2 * TOPMAX;
}

// Stage 1: grid (chunks, rows).  Applies the filters to one 1024-entry slice of the row and reduces it
// to two partial statistics (text range, timestamp range): {max, sum exp(x - max), first arg-max}.
// All four logits of a thread are requested before any is used (one L2 round trip per workgroup).
// BIAS (phrase lists, kernels.h PhraseArgs): `boost` is added to the logit of every token that labels an edge out of the
// row's trie node or out of the root, BEFORE the filters — a LogitFilter at the front of the list; the logits buffer itself
// is left alone.  Root membership is one more coalesced load at the logits' own indices; the node's child_begin pair sits in
// `span` (left by the previous step's final kernel) and is asked for in the same batch.  Only the node's child tokens come
// one round trip later: 64 per wave in one coalesced load, of which those inside this workgroup's 1024-entry slice (usually
// none: the children of a node fall into few of the ~50 slices) are handed round as wave-uniform values.
// REP (repetition control, kernels.h RepArgs): stateless — everything comes from the row's own sampled tokens H, which the
// workgroup walks in tiles of 256 (one token per thread, one dependent round trip behind the position counter).  A token
// of H below eot that falls into this workgroup's slice sets its bit in `sh_pen` (the penalised SET: a token seen five times
// is marked once); where the ngram - 1 tokens before it equal the row's last ngram - 1 tokens it also sets its bit in
// `sh_ban`.  The contexts are compared in LDS (`sh_hist` keeps a tile and the 16 tokens before it), and only for the few
// tokens of the slice.  Penalty on the raw logit -> boost -> ban, all ahead of the stock filters.
constexpr int HTILE = 256;      // tokens of a row's history per pass (== the workgroup size)
constexpr int HLEAD = 16;       // tokens kept in front of a tile: the longest context (REP_MAX_NGRAM - 1) rounded up
static_assert(whk::REP_MAX_NGRAM - 1 <= HLEAD, "a context must fit in front of a tile");
// STATS (per-token statistics, kernels.h TokenStatArgs): the slice's entropy statistic goes out beside {m, s} in the partial's
// spare slots, and with top_k > 0 its top_k best EDITED entries per range are selected as beam.hip selects a beam's candidates
// (rounds of a workgroup arg-max over the four entries a thread holds) into the scratch of the statistics.  The logits are
// read once, as without it.
template <bool SAMPLE, bool BIAS, bool REP, bool STATS>
__global__ __launch_bounds__(256) void greedy_partial_kernel(whk::SampleArgs a, int nchunk, whk::PhraseArgs ph, whk::RepArgs rp,
                                                             whk::TokenStatArgs ts) {
  pin_kernargs(a);
  if constexpr (BIAS) pin_kernargs(ph);
  if constexpr (REP) pin_kernargs(rp);
  if constexpr (STATS) pin_kernargs(ts);
  asm volatile("" ::"s"(nchunk));
  __shared__ BlockEStats sh_es;      // unused, and so not allocated, without STATS
  __shared__ float sh_bv[STATS ? 4 : 1];
  __shared__ int sh_bi[STATS ? 4 : 1];
  __shared__ int sh_hist[REP ? HLEAD + HTILE : 1];
  __shared__ int sh_suffix[REP ? HLEAD : 1];
  __shared__ unsigned sh_pen[REP ? SCHUNK / 32 : 1], sh_ban[REP ? SCHUNK / 32 : 1];
  __shared__ BlockStats<!SAMPLE> sh_st;       // when sampling, the index travels with the Pick
  __shared__ BlockPicks sh_pk;
  const RuleArgs& r = a.rules;
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = blockIdx.x, k = blockIdx.y;
  const float* x = r.logits + (int64_t)k * r.logits_ld;
  float xv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = c * SCHUNK + j * 256 + tid;
    xv[j] = v < r.V ? x[v] : WH_NEG_INF;
  }
  int rootc[4] = {-1, -1, -1, -1}, vsb = 0, vse = 0;
  if constexpr (BIAS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = c * SCHUNK + j * 256 + tid;
      if (v < r.V) rootc[j] = ph.root_child[v];
    }
    vsb = load_agent_int(ph.span + 2 * k); vse = load_agent_int(ph.span + 2 * k + 1);
  }
  const RowPos pos = row_pos(r, k);
  const int ntok = pos.ntok, sample_begin = pos.sample_begin, L = pos.L;
  const int64_t* row = a.tokens + (int64_t)k * r.token_stride;
  // the final kernel of the previous step left what the rules need about this row's sampled tokens
  const TsWindow win = ts_window_load(r, pos, a.row_state, k);
  const int split = r.timestamp_begin >= 0 ? r.timestamp_begin : r.V;   // text range [0, split), timestamp range [split, V)

  bool hit[4] = {false, false, false, false};
  if constexpr (BIAS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hit[j] = rootc[j] >= 0;
    int sb = uniform(vsb), se = uniform(vse);
    if (L == 0 || sb < 0) sb = se = 0;       // a row's first sampled token is decided at the root
    if (se > ph.n_edges) se = ph.n_edges;
    const int lo = c * SCHUNK;
    for (int e0 = sb; e0 < se; e0 += 64) {
      const int e = e0 + lane;
      const int tk = e < se ? ph.child_token[e] : -1;
      unsigned long long m = __ballot((unsigned)(tk - lo) < (unsigned)SCHUNK);
      while (m) {                             // wave-uniform: the lanes whose child token lies in this slice
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        const int d = __builtin_amdgcn_readlane(tk, i) - lo - tid;
#pragma unroll
        for (int j = 0; j < 4; ++j) hit[j] = hit[j] || d == j * 256;
      }
    }
  }

  if constexpr (REP) {
    const int nctx = rp.ngram > 0 ? rp.ngram - 1 : 0;      // context length; ngram == 0: no ban
    const bool ban_on = rp.ngram > 0 && L >= nctx, pen_on = rp.penalty != 1.0f;
    const int lo = c * SCHUNK;
    if (tid < SCHUNK / 32) { sh_pen[tid] = 0u; sh_ban[tid] = 0u; }
    if (ban_on && tid < nctx) sh_suffix[tid] = (int)row[ntok - nctx + tid];        // s = the last ngram - 1 tokens of H
    // Every workgroup of the row walks the WHOLE history, also one whose slice turns out to hold none of the row's tokens:
    // which slices they fall in is only known after reading them.  The cost of the feature therefore grows with L in all
    // of a row's workgroups (V / 1024 of them), not only in those that end up with a bit set.
    for (int base = 0; base < L; base += HTILE) {          // L is workgroup-uniform
      const int g = base + tid;                            // this thread's position in H
      const int tok = g < L ? (int)row[sample_begin + g] : -1;
      int lead = -1;
      if (tid < HLEAD && base + tid - HLEAD >= 0) lead = (int)row[sample_begin + base + tid - HLEAD];
      if (base > 0) __syncthreads();                       // the previous tile has been compared
      sh_hist[HLEAD + tid] = tok;
      if (tid < HLEAD) sh_hist[tid] = lead;
      __syncthreads();
      const unsigned d = (unsigned)(tok - lo);
      if (g < L && tok >= 0 && tok < r.eot && d < (unsigned)SCHUNK) {
        if (pen_on) atomicOr(&sh_pen[d >> 5], 1u << (d & 31));
        if (ban_on && g >= nctx) {                         // H[g - nctx .. g - 1] == s ?  (i = g - nctx <= L - ngram)
          bool same = true;
          for (int q = 0; q < nctx; ++q) same = same && sh_hist[HLEAD + tid - nctx + q] == sh_suffix[q];
          if (same) atomicOr(&sh_ban[d >> 5], 1u << (d & 31));
        }
      }
    }
    __syncthreads();
  }

  Stat<!SAMPLE> st[2];
  Pick pk[2];
  EStat est[2];
  float xe[4] = {0.f, 0.f, 0.f, 0.f};      // STATS: the edited logits, valid where `live` has the entry's bit
  unsigned live = 0;
  const int step = ntok + pos.lag;         // the common position counter: the same for every row of a step
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = c * SCHUNK + j * 256 + tid;
    if (v >= r.V) continue;
    bool masked = rule_masked(r, pos, win, v);
    if constexpr (REP) {
      if ((sh_ban[(j * 256 + tid) >> 5] >> (tid & 31)) & 1u) masked = true;      // NoRepeatNGram: -inf, like a suppressed token
    }
    if (masked) continue;
    float xj = xv[j];
    if constexpr (REP) {                       // RepetitionPenalty: on the raw logit, ahead of the boost
      if ((sh_pen[(j * 256 + tid) >> 5] >> (tid & 31)) & 1u) {
        if (xj > 0.f) xj = xj / rp.penalty;
        else if (xj < 0.f) xj = xj * rp.penalty;
      }
    }
    if constexpr (BIAS) { if (hit[j]) xj += ph.boost; }
    if (v < split) stat_add(st[0], xj, v); else stat_add(st[1], xj, v);
    if constexpr (STATS) {
      if (v < split) estat_add(est[0], xj); else estat_add(est[1], xj);
      xe[j] = xj;
      live |= (xj != WH_NEG_INF ? 1u : 0u) << j;
    }
    if constexpr (SAMPLE) {
      if (xj != WH_NEG_INF) {
        const float key = xj * a.inv_temperature + gumbel(a.seed_lo, a.seed_hi, step, k, v);
        pick_merge(pk[v < split ? 0 : 1], key, xj, v);
      }
    }
  }
  if constexpr (SAMPLE) sh_pk.publish(pk);
  if constexpr (STATS) sh_es.publish(est);
  sh_st.reduce(st);
  if (tid < 2) {
    const auto t = sh_st.range(tid);
    float* o = a.partials + (((int64_t)k * nchunk + c) * 2 + tid) * PSTRIDE;   // nchunk == gridDim.x, passed as an argument:
                                                                               // gridDim sits in the implicit arguments (a second kernarg round trip)
    o[0] = t.m; o[1] = t.s;
    if constexpr (SAMPLE) { const Pick p = sh_pk.range(tid); o[2] = __int_as_float(p.idx); o[3] = p.key; o[4] = p.x; }
    else o[2] = __int_as_float(t.idx);
    if constexpr (STATS) { const EStat e = sh_es.range(tid); o[5] = e.m; o[6] = e.s; o[7] = e.t; }
  }
  if constexpr (STATS) {
    const int K = ts.top_k;                 // uniform; 0: log-probability and entropy alone
    if (K > 0) {
      const int lo = c * SCHUNK, hi = (lo + SCHUNK < r.V) ? lo + SCHUNK : r.V;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float* pv = top_part_val(ts) + (((int64_t)k * nchunk + c) * 2 + g) * TOPMAX;
        int* pi = top_part_idx(ts, r.R, nchunk) + (((int64_t)k * nchunk + c) * 2 + g) * TOPMAX;
        const bool has = g == 0 ? lo < split : hi > split;        // uniform
        if (!has) {
          if (tid < K) { pv[tid] = WH_NEG_INF; pi[tid] = NO_IDX; }
          continue;
        }
        unsigned avail = 0;                 // live entries of this range not yet taken
#pragma unroll
        for (int j = 0; j < 4; ++j) avail |= ((((live >> j) & 1u) != 0 && (lo + j * 256 + tid < split) == (g == 0)) ? 1u : 0u) << j;
        for (int kk = 0; kk < K; ++kk) {
          float bv = WH_NEG_INF; int bi = NO_IDX;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool on = ((avail >> j) & 1u) != 0;
            best_merge(bv, bi, on ? xe[j] : WH_NEG_INF, on ? lo + j * 256 + tid : NO_IDX);
          }
          block_best(bv, bi, sh_bv, sh_bi);
          if (tid == 0) { pv[kk] = bv; pi[kk] = bi; }
#pragma unroll
          for (int j = 0; j < 4; ++j) avail &= ~(((lo + j * 256 + tid == bi) ? 1u : 0u) << j);
        }
      }
    }
  }
}

// Stage 2: one workgroup per row merges the chunk partials, applies the "timestamp mass" rule and
// GreedyDecoder.update, and appends the token.
// BIAS: the row's trie node then follows the token — the edge out of the node, else the edge out of the root, else the
// root.  The whole workgroup finds it in one round trip that starts as soon as the token is known and runs beside the
// embedding gather: thread i asks for child i of the node (token and target), thread 0 for root_child[token]; a loop only
// for a node of more than 256 children.  Thread 0 stores the node (row_state slot 3) and its child_begin pair (`span`).
// STATS: the row's entropy statistic is merged beside {m, s}; thread 0 writes the step's log-probability (the value it
// accumulates) and entropy.  With top_k > 0 the chunks' best entries are pooled in LDS while the partials are merged, the text
// range's are dropped where the mass rule fired, and top_k rounds of a workgroup arg-max pick the row's — beam_row_kernel's
// selection, behind everything the next step waits for.
template <bool SAMPLE, bool BIAS, bool STATS>
__global__ __launch_bounds__(256) void greedy_final_kernel(whk::SampleArgs a, int nchunk, whk::PhraseArgs ph, whk::TokenStatArgs ts) {
  pin_kernargs(a);
  if constexpr (BIAS) pin_kernargs(ph);
  if constexpr (STATS) pin_kernargs(ts);
  asm volatile("" ::"s"(nchunk));
  __shared__ BlockEStats sh_es;      // unused, and so not allocated, without STATS
  __shared__ float sh_bv[STATS ? 4 : 1], pool_v[STATS ? TOP_POOL : 1], sh_norm[2];
  __shared__ int sh_bi[STATS ? 4 : 1], pool_i[STATS ? TOP_POOL : 1], sh_kind;
  __shared__ BlockStats<!SAMPLE> sh_st;
  __shared__ BlockPicks sh_pk;
  __shared__ int sh_next, sh_child;
  const RuleArgs& r = a.rules;
  const int tid = threadIdx.x, k = blockIdx.x;
  int vsb = 0, vse = 0;
  if constexpr (BIAS) { vsb = load_agent_int(ph.span + 2 * k); vse = load_agent_int(ph.span + 2 * k + 1); }
  const RowPos pos = row_pos(r, k);
  const int ntok = pos.ntok, lag = pos.lag;
  int64_t* row = a.tokens + (int64_t)k * r.token_stride;
  const bool ts_rules = r.timestamp_begin >= 0;
  Stat<!SAMPLE> st[2];
  Pick pk[2];
  EStat est[2];
  for (int c = tid; c < nchunk; c += 256) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const float* o = a.partials + (((int64_t)k * nchunk + c) * 2 + g) * PSTRIDE;
      if constexpr (STATS) estat_merge(est[g], EStat{o[5], o[6], o[7]});
      if constexpr (SAMPLE) {
        stat_merge(st[g], Stat<false>{o[0], o[1]});
        pick_merge(pk[g], o[3], o[4], __float_as_int(o[2]));
      } else {
        stat_merge(st[g], Stat<true>{o[0], o[1], __float_as_int(o[2])});
      }
    }
  }
  if constexpr (SAMPLE) sh_pk.publish(pk);
  if constexpr (BIAS) { if (tid == 0) sh_child = -1; }
  const int K = STATS ? ts.top_k : 0, npool = 2 * nchunk * K;      // uniform
  if constexpr (STATS) {
    sh_es.publish(est);
    for (int e = tid; e < npool; e += 256) {              // entry e: (chunk, range) = e / K, rank e % K
      const int cg = e / K, kk = e - cg * K;
      pool_v[e] = top_part_val(ts)[((int64_t)k * nchunk * 2 + cg) * TOPMAX + kk];
      pool_i[e] = top_part_idx(ts, r.R, nchunk)[((int64_t)k * nchunk * 2 + cg) * TOPMAX + kk];
    }
  }
  sh_st.reduce(st);
  if (tid == 0) {
    const int64_t last_tok = row[ntok - 1];
    bool text_masked;
    const auto fin = allowed_range(sh_st.range(0), sh_st.range(1), ts_rules, &text_masked);
    int next; float lp;
    if constexpr (SAMPLE) {                  // the Gumbel-max draw among the allowed entries; unscaled log-probability
      Pick p = sh_pk.range(1);
      if (!text_masked) { const Pick ptx = sh_pk.range(0); pick_merge(p, ptx.key, ptx.x, ptx.idx); }
      next = p.idx;
      lp = (p.x - fin.m) - logf(fin.s);
    } else {
      next = fin.idx;
      lp = -logf(fin.s);                     // log_softmax(filtered)[next] = x - max - log(sum exp(x - max)); x[next] == max
    }
    if (fin.m == WH_NEG_INF) { next = 0; lp = __builtin_nanf(""); }   // every logit filtered: argmax of all -inf
    if (last_tok != r.eot) r.sum_logprobs[k] += lp;
    else next = r.eot;
    if constexpr (STATS) {
      // kind 0: the list of the allowed entries, 1: of the timestamps alone (mass rule), 2: padding only
      const bool at_eot = last_tok == r.eot, none = fin.m == WH_NEG_INF;
      EStat ef = sh_es.range(1);
      if (!text_masked) { ef = sh_es.range(0); estat_merge(ef, sh_es.range(1)); }
      const int64_t col = (int64_t)k * ts.stride + ntok;
      if (ts.token_logprob) ts.token_logprob[col] = at_eot ? 0.f : lp;
      if (ts.entropy) ts.entropy[col] = at_eot ? 0.f : none ? __builtin_nanf("") : logf(ef.s) - ef.t / ef.s;
      sh_kind = (at_eot || none) ? 2 : text_masked ? 1 : 0;
      sh_norm[0] = fin.m; sh_norm[1] = none ? 0.f : logf(fin.s);
    }
    row[ntok] = next;
    if (a.step_tokens) a.step_tokens[k] = next;
    if (next != r.eot) *a.d_alive_step = ntok + lag;      // benign race: every writer stores the same value
    sh_next = next;
    if (ts_rules) {                                        // what the next step's window needs about this row (ts_window_of_state)
      int* st = a.row_state + 4 * k;
      const bool is_ts = next >= r.timestamp_begin;
      st[1] = st[0];
      st[0] = is_ts ? 1 : 0;
      if (is_ts) st[2] = next + 1;
    }
  }
  int sb = 0, se = 0, nxt = 0, tk0 = -1, cn0 = 0, rootc = -1;
  if constexpr (BIAS) {
    __syncthreads();
    nxt = sh_next;
    sb = uniform(vsb); se = uniform(vse);
    if (pos.L == 0 || sb < 0) sb = se = 0;     // a row's first sampled token leaves from the root
    if (se > ph.n_edges) se = ph.n_edges;
    if (sb + tid < se) { tk0 = ph.child_token[sb + tid]; cn0 = ph.child_node[sb + tid]; }
    if (tid == 0 && nxt >= 0 && nxt < r.V) rootc = ph.root_child[nxt];
  }
  if (a.x_next) {                             // the next step's input row: embedding of the token just chosen, at its index
    if constexpr (!BIAS) __syncthreads();
    int tok = sh_next;
    if (tok < 0) tok = 0;
    if (tok > r.V - 1) tok = r.V - 1;
    if (ntok < a.n_pos) {
      const float* pp = a.pos_emb + (int64_t)ntok * a.D;
      float* xr = a.x_next + (int64_t)k * a.D;
      if (a.emb_f16) {
        const half_t* e = (const half_t*)a.tok_emb + (int64_t)tok * a.D;
        for (int dd = tid; dd < a.D; dd += 256) xr[dd] = (float)e[dd] + pp[dd];
      } else {
        const float* e = (const float*)a.tok_emb + (int64_t)tok * a.D;
        for (int dd = tid; dd < a.D; dd += 256) xr[dd] = e[dd] + pp[dd];
      }
    }
  }
  if constexpr (BIAS) {
    if (tk0 == nxt) sh_child = cn0;           // child tokens are distinct within a node: at most one writer
    for (int e = sb + 256 + tid; e < se; e += 256)
      if (ph.child_token[e] == nxt) sh_child = ph.child_node[e];
    __syncthreads();
    if (tid == 0) {
      int ns = sh_child >= 0 ? sh_child : (rootc >= 0 ? rootc : 0);
      if (ns >= ph.n_nodes) ns = 0;
      int b = 0, e = 0;
      if (ns > 0) { b = ph.child_begin[ns]; e = ph.child_begin[ns + 1]; }
      a.row_state[4 * k + 3] = ns;
      ph.span[2 * k] = b; ph.span[2 * k + 1] = e;
    }
  }
  if constexpr (STATS) {
    if (K > 0) {
      __syncthreads();
      const int kind = uniform(sh_kind);      // the same in every lane: the branches below stay scalar
      const float M = sh_norm[0], LS = sh_norm[1];
      const int64_t col = ((int64_t)k * ts.stride + ntok) * K;
      if (kind == 2) {
        if (tid < K) { ts.top_token[col + tid] = -1; ts.top_logprob[col + tid] = WH_NEG_INF; }
        return;
      }
      if (kind == 1) {                      // entry e belongs to range (e / K) & 1: drop the text range's
        for (int e = tid; e < npool; e += 256)
          if (((e / K) & 1) == 0) pool_v[e] = WH_NEG_INF;
      }
      for (int kk = 0; kk < K; ++kk) {      // a thread reads the pool entries it wrote itself: no barrier in between
        float bv = WH_NEG_INF; int bi = NO_IDX;
        for (int e = tid; e < npool; e += 256)
          if (pool_v[e] != WH_NEG_INF) best_merge(bv, bi, pool_v[e], pool_i[e]);
        block_best(bv, bi, sh_bv, sh_bi);
        if (tid == 0) {
          // at temperature 0 entry 0 is the chosen token: -log s as the accumulated value is formed, not 0 - log s (-0 vs +0)
          float v = (!SAMPLE && kk == 0) ? -LS : (bv - M) - LS;
          if (bv == WH_NEG_INF) v = WH_NEG_INF;
          ts.top_token[col + kk] = (bi == NO_IDX) ? -1 : bi;
          ts.top_logprob[col + kk] = v;
        }
        for (int e = tid; e < npool; e += 256)
          if (pool_i[e] == bi) pool_v[e] = WH_NEG_INF;     // a token sits in exactly one (chunk, range)
      }
    }
  }
}

__global__ __launch_bounds__(256) void phrase_root_table_kernel(const int* __restrict__ child_begin, const int* __restrict__ child_token,
                                                                const int* __restrict__ child_node, int n_edges, int V,
                                                                int* __restrict__ root) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  int end = child_begin[1];
  if (end > n_edges) end = n_edges;
  if (e < end) {
    const int t = child_token[e];
    if (t >= 0 && t < V) root[t] = child_node[e];
  }
}

__global__ void phrase_span_kernel(const int* __restrict__ row_state, const int* __restrict__ child_begin, int n_nodes, int R,
                                   int* __restrict__ span) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int s = row_state[4 * r + 3];
  const bool inner = s > 0 && s < n_nodes;
  span[2 * r] = inner ? child_begin[s] : 0;
  span[2 * r + 1] = inner ? child_begin[s + 1] : 0;
}

// softmax(logits at <|startoftranscript|>)[no_speech] per row (decoding.py:689-693).  One workgroup of 1024 threads per
// row; every thread requests 8 logits before it folds any of them (the first version walked the row with one dependent
// L2 round trip per 256 entries: 72 us for 51866 entries; this form takes a handful of round trips).
__global__ __launch_bounds__(1024) void no_speech_kernel(const float* __restrict__ logits, int64_t row_stride,
                                                         int V, int no_speech, float* __restrict__ out) {
  __shared__ float sh_m[16], sh_s[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)blockIdx.x * row_stride;
  float m = WH_NEG_INF, s = 0.f;
  constexpr int UN = 8;
  for (int v0 = 0; v0 < V; v0 += 1024 * UN) {
    float xv[UN];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      int v = v0 + j * 1024 + tid; if (v > V - 1) v = V - 1;       // branch-free loads, masked at use
      xv[j] = x[v];
    }
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      if (v0 + j * 1024 + tid < V) {
        // a -inf logit adds nothing; while m is still -inf, expf(-inf - m) would be expf(NaN)
        if (xv[j] > m) { s = s * expf(m - xv[j]) + 1.0f; m = xv[j]; } else if (xv[j] != WH_NEG_INF) s += expf(xv[j] - m);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const float mn = fmaxf(m, m2);
    s = (mn == WH_NEG_INF) ? 0.f : s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
  }
  if (lane == 0) { sh_m[wave] = m; sh_s[wave] = s; }
  __syncthreads();
  if (tid == 0) {
    float M = sh_m[0];
    for (int w = 1; w < 16; ++w) M = fmaxf(M, sh_m[w]);
    float S = 0.f;
    for (int w = 0; w < 16; ++w) S += (sh_m[w] == WH_NEG_INF) ? 0.f : sh_s[w] * expf(sh_m[w] - M);
    out[blockIdx.x] = expf(x[no_speech] - M) / S;
  }
}

__global__ void gather_tokens_kernel(const int64_t* __restrict__ src, int64_t stride, int R,
                                     int64_t* __restrict__ dst) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < R) dst[r] = src[(int64_t)r * stride];
}

}  // namespace

namespace whk {

size_t greedy_sample_scratch_bytes(int R, int V) { return (size_t)R * ((V + SCHUNK - 1) / SCHUNK) * 2 * PSTRIDE * sizeof(float); }
size_t greedy_sample_top_scratch_bytes(int R, int V) { return (size_t)R * ((V + SCHUNK - 1) / SCHUNK) * 2 * TOPMAX * 2 * 4; }

template <bool SAMPLE, bool BIAS, bool STATS>
static void greedy_sample_launch3(const SampleArgs& a, const PhraseArgs& ph, const RepArgs* rep, const TokenStatArgs& ts, int nchunk,
                                  hipStream_t stream) {
  if (rep)      // repetition control lives in the partial kernel alone: the final kernel is the same with and without it
    hipLaunchKernelGGL(HIP_KERNEL_NAME(greedy_partial_kernel<SAMPLE, BIAS, true, STATS>), dim3(nchunk, a.rules.R), dim3(256), 0, stream, a, nchunk, ph, *rep, ts);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(greedy_partial_kernel<SAMPLE, BIAS, false, STATS>), dim3(nchunk, a.rules.R), dim3(256), 0, stream, a, nchunk, ph, RepArgs{0, 1.0f}, ts);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(greedy_final_kernel<SAMPLE, BIAS, STATS>), dim3(a.rules.R), dim3(256), 0, stream, a, nchunk, ph, ts);
}
template <bool SAMPLE, bool BIAS>
static void greedy_sample_launch(const SampleArgs& a, const PhraseArgs& ph, const RepArgs* rep, const TokenStatArgs* ts, int nchunk,
                                 hipStream_t stream) {
  if (ts) { greedy_sample_launch3<SAMPLE, BIAS, true>(a, ph, rep, *ts, nchunk, stream); return; }
  TokenStatArgs none;
  memset(&none, 0, sizeof(none));
  greedy_sample_launch3<SAMPLE, BIAS, false>(a, ph, rep, none, nchunk, stream);
}

hipError_t launch_greedy_sample(const SampleArgs& a, hipStream_t stream, const PhraseArgs* ph, const RepArgs* rep,
                                const TokenStatArgs* ts) {
  const int nchunk = (a.rules.V + SCHUNK - 1) / SCHUNK;
  if (!a.partials) return hipErrorInvalidValue;
  if (ts) {     // refused before anything is launched: nothing is written
    if (ts->top_k < 0 || ts->top_k > TOKEN_STATS_MAX_TOP || ts->stride < 1 || ts->stride < a.rules.token_stride)
      return hipErrorInvalidValue;
    if (ts->top_k > 0 && (!ts->top_token || !ts->top_logprob || !ts->scratch || nchunk > TOP_CHUNKS)) return hipErrorInvalidValue;
    if (!ts->token_logprob && !ts->entropy && !(ts->top_k > 0)) return hipErrorInvalidValue;
  }
  const bool sample = a.inv_temperature > 0.f;
  if (rep) {
    if (rep->ngram < 0 || rep->ngram > REP_MAX_NGRAM || !(rep->penalty > 0.f) || !(rep->penalty <= 3.402823466e38f))
      return hipErrorInvalidValue;
    if (rep->ngram == 0 && rep->penalty == 1.0f) rep = nullptr;      // both off: the kernels of a plain decode
  }
  if (a.rules.timestamp_begin >= 0 && !a.row_state) return hipErrorInvalidValue;   // the timestamp window comes from it
  if (ph) {
    if (!ph->child_begin || !ph->child_token || !ph->child_node || !ph->root_child || !ph->span || !a.row_state ||
        ph->n_nodes < 1 || ph->n_edges < 0)
      return hipErrorInvalidValue;
    if (sample) greedy_sample_launch<true, true>(a, *ph, rep, ts, nchunk, stream);
    else greedy_sample_launch<false, true>(a, *ph, rep, ts, nchunk, stream);
  } else {
    PhraseArgs none;
    memset(&none, 0, sizeof(none));
    if (sample) greedy_sample_launch<true, false>(a, none, rep, ts, nchunk, stream);
    else greedy_sample_launch<false, false>(a, none, rep, ts, nchunk, stream);
  }
  return hipGetLastError();
}

hipError_t launch_phrase_root_table(const int* child_begin, const int* child_token, const int* child_node, int n_edges,
                                    int V, int* root, hipStream_t stream) {
  if (!child_begin || !child_token || !child_node || !root || n_edges < 1 || V < 1) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(root, 0xff, (size_t)V * 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(phrase_root_table_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, stream, child_begin, child_token,
                     child_node, n_edges, V, root);
  return hipGetLastError();
}

hipError_t launch_phrase_span(const int* row_state, const int* child_begin, int n_nodes, int R, int* span, hipStream_t stream) {
  if (!row_state || !child_begin || !span || n_nodes < 1 || R < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(phrase_span_kernel, dim3((R + 63) / 64), dim3(64), 0, stream, row_state, child_begin, n_nodes, R, span);
  return hipGetLastError();
}

hipError_t launch_no_speech(const float* logits, int64_t row_stride, int R, int V, int no_speech,
                            float* out, hipStream_t stream) {
  hipLaunchKernelGGL(no_speech_kernel, dim3(R), dim3(1024), 0, stream, logits, row_stride, V, no_speech, out);
  return hipGetLastError();
}

hipError_t launch_gather_tokens(const int64_t* src, int64_t stride, int R, int64_t* dst, hipStream_t stream) {
  hipLaunchKernelGGL(gather_tokens_kernel, dim3((R + 63) / 64), dim3(64), 0, stream, src, stride, R, dst);
  return hipGetLastError();
}

}  // namespace whk
