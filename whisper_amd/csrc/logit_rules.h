/*
 * logit_rules.h — the stock logit rules of DecodingTask._main_loop (whisper/decoding.py:696-703), stated once for the
 * greedy / sampling epilogue (sampling.hip) and the beam-search epilogue (beam.hip):
 *   SuppressBlank (decoding.py:423-430) -> SuppressTokens (:433-438) -> ApplyTimestampRules (:441-505).
 * A row's logits are passed over once.  What depends on one entry alone is `rule_masked`, a predicate over (row position,
 * timestamp window, token).  The one rule that needs the whole row, "timestamp probability mass > best text token"
 * (:498-505), follows from separate online softmax statistics (`Stat`) of the text range [0, timestamp_begin) and of the
 * timestamp range: `allowed_range` returns those of what stays allowed, i.e. the normaliser of log_softmax over the
 * filtered row, without the row being read again.
 * The predicate and the two ways to a row's timestamp window are __host__ __device__: ktest.cpp evaluates the same text
 * without a launch (wht_rule_mask), as it does for the sampler's noise (sample_noise.h).
 */
#ifndef WH_LOGIT_RULES_H
#define WH_LOGIT_RULES_H

#include "common.h"
#include "kernels.h"

#define RULE_FN __host__ __device__ static inline

namespace whk {

// ---- where a row stands -------------------------------------------------------------------------------------------------
// Ragged prompts: row k holds `lag` fewer tokens than the longest row and its sample_begin is `lag` earlier; L = the number
// of tokens the row has sampled so far.
struct RowPos {
  int lag, ntok, sample_begin, L;
};
RULE_FN RowPos row_pos_of(const RuleArgs& r, int ntok_longest, int lag) {
  return RowPos{lag, ntok_longest - lag, r.sample_begin - lag, ntok_longest - r.sample_begin};
}
// both values are asked for before either is used (one round trip); they are workgroup-uniform and land in SGPRs
__device__ __forceinline__ RowPos row_pos(const RuleArgs& r, int k) {
  const int vl = load_agent_int(r.lag ? r.lag + k : r.d_ntok), vn = load_agent_int(r.d_ntok);
  return row_pos_of(r, uniform(vn), r.lag ? uniform(vl) : 0);
}

// ---- what ApplyTimestampRules needs of the row's sampled tokens H (decoding.py:456-481) -----------------------------------
// last_ts / pen_ts: the last / the one-before-last token of H is a timestamp (pen_ts also where H has fewer than two
// tokens); [lo, hi): the timestamps H forbids — up to the last one of H, that one included unless it may be repeated to
// close a pair (last_ts && !pen_ts).  All false / empty when the rules are off (timestamp_begin < 0).
struct TsWindow {
  bool last_ts, pen_ts; int lo, hi;
};
// from the state the greedy loop keeps per row (SampleArgs::row_state): {last token of H is a timestamp, the one before it
// is, value of the last timestamp of H + 1 (0: none)}
RULE_FN TsWindow ts_window_of_state(const RuleArgs& r, const RowPos& p, int s0, int s1, int s2) {
  TsWindow w = {false, false, 0, 0};
  if (r.timestamp_begin < 0) return w;
  w.last_ts = (p.L >= 1) && s0 != 0;
  w.pen_ts = (p.L < 2) || s1 != 0;
  if (s2 > 0) { w.lo = r.timestamp_begin; w.hi = (w.last_ts && !w.pen_ts) ? s2 - 1 : s2; }
  return w;
}
__device__ __forceinline__ TsWindow ts_window_load(const RuleArgs& r, const RowPos& p, const int* row_state, int k) {
  if (r.timestamp_begin < 0) return TsWindow{false, false, 0, 0};
  const int s0 = load_agent_int(row_state + 4 * k), s1 = load_agent_int(row_state + 4 * k + 1),
            s2 = load_agent_int(row_state + 4 * k + 2);
  return ts_window_of_state(r, p, uniform(s0), uniform(s1), uniform(s2));
}
// from H itself: `last` = the index in H of its last timestamp, -1 if it has none
RULE_FN TsWindow ts_window_of_history(const RuleArgs& r, const RowPos& p, const int64_t* row, int last) {
  TsWindow w = {false, false, 0, 0};
  const int TB = r.timestamp_begin;
  if (TB < 0) return w;
  w.last_ts = (p.L >= 1) && (row[p.ntok - 1] >= TB);
  w.pen_ts = (p.L < 2) || (row[p.ntok - 2] >= TB);
  if (last >= 0) { const int t = (int)row[p.sample_begin + last]; w.lo = TB; w.hi = (w.last_ts && !w.pen_ts) ? t : t + 1; }
  return w;
}
// ... with `last` found by the 256 threads of a workgroup (sh_last: one LDS word).  Two barriers.
__device__ __forceinline__ TsWindow ts_window_scan(const RuleArgs& r, const RowPos& p, const int64_t* row, int* sh_last) {
  if (threadIdx.x == 0) *sh_last = -1;
  __syncthreads();
  if (r.timestamp_begin >= 0) {
    for (int t = threadIdx.x; t < p.L; t += 256)
      if (row[p.sample_begin + t] >= r.timestamp_begin) atomicMax(sh_last, t);
  }
  __syncthreads();
  return ts_window_of_history(r, p, row, *sh_last);
}

// ---- the per-entry rules --------------------------------------------------------------------------------------------------
// true: token v < V is -inf for this row.  Consume it as a selection (a bit mask of the survivors, a `continue`), never as a
// conditional store of -inf into a register array of logits: beam.hip's `if (masked) xv[j] = -inf` was dropped by the
// compiler (empty if-body in the ISA; every filter silently off), which is what tools/isa_lint.py looks for since.
RULE_FN bool rule_masked(const RuleArgs& r, const RowPos& p, const TsWindow& w, int v) {
  const int TB = r.timestamp_begin;        // < 0: timestamp rules disabled (without_timestamps)
  bool masked = r.suppress_mask && r.suppress_mask[v];
  if (r.suppress_blank && p.L == 0 && (v == r.blank_token || v == r.eot)) masked = true;
  if (TB >= 0) {
    if (v == r.no_timestamps) masked = true;
    if (w.last_ts) {
      if (w.pen_ts) { if (v >= TB) masked = true; }
      else { if (v < r.eot) masked = true; }
    }
    if (v >= w.lo && v < w.hi) masked = true;
    if (p.L == 0) {
      if (v < TB) masked = true;
      if (r.max_initial_ts >= 0 && v > TB + r.max_initial_ts) masked = true;
    }
  }
  return masked;
}

// ---- online softmax statistics of a range ---------------------------------------------------------------------------------
// IDX: with the first arg-max (the smallest index among equal maxima).  Without it nothing is paid for an index.
constexpr int NO_IDX = 0x7fffffff;
template <bool IDX> struct Stat;            // default: the empty range
template <> struct Stat<false> { float m = WH_NEG_INF, s = 0.f; };
template <> struct Stat<true> { float m = WH_NEG_INF, s = 0.f; int idx = NO_IDX; };
template <bool IDX> __device__ __forceinline__ void stat_add(Stat<IDX>& a, float x, int i) {
  if (x == WH_NEG_INF) return;
  if (x > a.m) {
    a.s = a.s * expf(a.m - x) + 1.0f; a.m = x;
    if constexpr (IDX) a.idx = i;
  } else { a.s += expf(x - a.m); }   // x == a.m keeps the earlier (smaller) index: a thread's scan is ascending
}
// On a tie b.m == a.m both branches give a.s + b.s exactly, so the sums do not depend on whether an index is carried.
template <bool IDX> __device__ __forceinline__ void stat_merge(Stat<IDX>& a, const Stat<IDX>& b) {
  if (b.m == WH_NEG_INF) return;
  if (a.m == WH_NEG_INF) { a = b; return; }
  bool take = b.m > a.m;
  if constexpr (IDX) take = take || (b.m == a.m && b.idx < a.idx);
  if (take) {
    a.s = a.s * expf(a.m - b.m) + b.s; a.m = b.m;
    if constexpr (IDX) a.idx = b.idx;
  } else { a.s += b.s * expf(b.m - a.m); }
}
template <bool IDX> __device__ __forceinline__ void stat_wave_reduce(Stat<IDX>& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Stat<IDX> b{__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)};
    if constexpr (IDX) b.idx = __shfl_xor(a.idx, o, 64);
    stat_merge(a, b);
  }
}

// The two ranges of a 256-thread workgroup: `reduce` folds every thread's pair (wave reduce, lane 0 of each wave to LDS,
// barrier), after which any thread reads the workgroup's statistics of range g with `range`.  Lives in LDS.
template <bool IDX> struct BlockStatsIdx { int idx[2][4]; };
template <> struct BlockStatsIdx<false> {};
template <bool IDX> struct BlockStats : BlockStatsIdx<IDX> {
  float m[2][4], s[2][4];
  __device__ __forceinline__ void reduce(Stat<IDX> (&st)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      stat_wave_reduce(st[g]);
      if (lane == 0) { m[g][wave] = st[g].m; s[g][wave] = st[g].s; if constexpr (IDX) this->idx[g][wave] = st[g].idx; }
    }
    __syncthreads();
  }
  __device__ __forceinline__ Stat<IDX> range(int g) const {
    Stat<IDX> t;
    for (int w = 0; w < 4; ++w) {
      Stat<IDX> b{m[g][w], s[g][w]};
      if constexpr (IDX) b.idx = this->idx[g][w];
      stat_merge(t, b);
    }
    return t;
  }
};

// ---- selecting the best entries of a row (beam.hip: the K candidates; sampling.hip: the top-k alternatives) --------------------
// larger value wins; equal values: smaller index wins
__device__ __forceinline__ void best_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
// arg-max over the 256 threads of a workgroup; every thread receives the winner.  sh_v/sh_i: [4] scratch.
__device__ __forceinline__ void block_best(float& v, int& i, float* sh_v, int* sh_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    best_merge(v, i, v2, i2);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                        // scratch free (previous round read)
  if (lane == 0) { sh_v[wave] = v; sh_i[wave] = i; }
  __syncthreads();
  v = sh_v[0]; i = sh_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) best_merge(v, i, sh_v[w], sh_i[w]);
}

// ---- the timestamp mass rule (decoding.py:498-505) ------------------------------------------------------------------------
// tx / ts: the statistics of the filtered text / timestamp range.  Where the timestamps together are more probable than the
// best text token (logsumexp of their log-probabilities vs the largest text one, same normaliser) the text range is dropped.
// Returns the statistics of what stays allowed.
template <bool IDX>
__device__ __forceinline__ Stat<IDX> allowed_range(const Stat<IDX>& tx, const Stat<IDX>& ts, bool ts_rules, bool* text_masked) {
  *text_masked = false;
  if (ts_rules) {
    Stat<IDX> all = tx;
    stat_merge(all, ts);
    if (all.m != WH_NEG_INF) {
      const float lse_all = logf(all.s);
      const float ts_lp_max = (ts.m - all.m) - lse_all;
      const float ts_lse = (ts.m == WH_NEG_INF) ? WH_NEG_INF : ts_lp_max + logf(ts.s);
      const float text_lp_max = (tx.m == WH_NEG_INF) ? WH_NEG_INF : (tx.m - all.m) - lse_all;
      if (ts_lse > text_lp_max) *text_masked = true;
    }
  }
  Stat<IDX> fin = ts;
  if (!*text_masked) { fin = tx; stat_merge(fin, ts); }
  return fin;
}

}  // namespace whk

#endif
