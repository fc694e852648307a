// ktest.cpp — test-only C entry points over the shipped kernel launchers (libwhisper_hip_ktest.so).
// Linked from the same build/*.o objects as libwhisper_hip.so (Makefile), so tests/test_kernel_parity_gpu.py checks the
// bytes that ship.  Arguments are flat (pointers, ints, strides): every wrapper fills the launcher's struct itself, so
// the Python side mirrors no struct layout.  Each wrapper returns the launcher's hipError_t unchanged.
#include <string.h>

#include "kernels.h"
#include "logit_rules.h"
#include "sample_noise.h"

using namespace whk;

extern "C" {

// name of the kernel form the last launch_gemv / launch_attn_decode / launch_gemm / launch_merge_partials on this thread picked
const char* wht_last_form() { return g_form; }
void wht_clear_form() { g_form = ""; }
int wht_attn_decode_capacity(int dtype) { return attn_decode_capacity(dtype); }
int wht_gemv8_will_run(int R, int N, int K, int pro) { return gemv8_will_run(R, N, K, pro) ? 1 : 0; }
// the family launch_gemv would pick ("" = refused); launches nothing.  ld is x_ld (PRO_PLAIN) or xf_ld (PRO_LN)
const char* wht_gemv_family(int dtype, int pro, int epi, int R, int N, int K, int64_t ld, int ln_folded, int has_bias, int splits,
                            int H, int x_frag, int y_frag) {
  static const float some_bias = 0.f;
  GemvArgs a;
  memset(&a, 0, sizeof a);
  a.pro = pro; a.epi = epi; a.R = R; a.N = N; a.K = K; a.x_ld = a.xf_ld = ld; a.ln_folded = ln_folded;
  a.bias = has_bias ? &some_bias : nullptr; a.splits = splits; a.H = H; a.x_frag = x_frag; a.y_frag = y_frag;
  return gemv_family(a, dtype);
}

int wht_gemv(int dtype, int pro, const void* x, int64_t x_ld, const float* xf, int64_t xf_ld, const float* ln_w,
             const float* ln_b, int ln_folded, const void* part_o, const float* part_ml, int splits, int H, const void* W,
             const float* bias, int N, int K, int R, int x_frag, int y_frag, int epi, void* y, int64_t y_ld, float* resid,
             int64_t resid_ld, void* kcache, void* vcache, int64_t cache_bs, const int* d_pos, int D, const int* lag,
             int* bump, int bump_by, int* bump2, void* stream) {
  GemvArgs a;
  memset(&a, 0, sizeof a);
  a.pro = pro; a.x = x; a.x_ld = x_ld; a.xf = xf; a.xf_ld = xf_ld; a.ln_w = ln_w; a.ln_b = ln_b; a.ln_folded = ln_folded;
  a.part_o = part_o; a.part_ml = part_ml; a.splits = splits; a.H = H;
  a.W = W; a.bias = bias; a.N = N; a.K = K; a.R = R; a.x_frag = x_frag; a.y_frag = y_frag;
  a.epi = epi; a.y = y; a.y_ld = y_ld; a.resid = resid; a.resid_ld = resid_ld;
  a.kcache = kcache; a.vcache = vcache; a.cache_bs = cache_bs; a.d_pos = d_pos; a.D = D; a.lag = lag;
  a.bump = bump; a.bump_by = bump_by; a.bump2 = bump2;
  return launch_gemv(a, dtype, (hipStream_t)stream);
}

// LayerNorm behind the MFMAs (kernels.h) with explicit buffers.  Consumer: pro = PRO_LN_POST, xh = fp16(x - centre) in fragment
// order, xc = centres [R] (replaced by the row means) or NULL.  Producer: a PRO_PLAIN / PRO_COMBINE launch with EPI_RESID that
// also stores xh from xc.  First site: pro = PRO_LN with xc = where the row means go.  Every other argument as wht_gemv.
int wht_gemv_ln_post(int pro, const void* x, int64_t x_ld, int x_frag, const float* xf, int64_t xf_ld, const void* part_o,
                     const float* part_ml, int splits, int H, const void* W, const float* bias, int N, int K, int R, void* xh,
                     float* xc, int y_frag, int epi, void* y, int64_t y_ld, float* resid, int64_t resid_ld, void* kcache,
                     void* vcache, int64_t cache_bs, const int* d_pos, int D, const int* lag, void* stream) {
  GemvArgs a;
  memset(&a, 0, sizeof a);
  a.pro = pro; a.x = x; a.x_ld = x_ld; a.x_frag = x_frag; a.xf = xf; a.xf_ld = xf_ld; a.ln_folded = 1;
  a.part_o = part_o; a.part_ml = part_ml; a.splits = splits; a.H = H;
  a.W = W; a.bias = bias; a.N = N; a.K = K; a.R = R; a.xh = xh; a.xc = xc; a.y_frag = y_frag;
  a.epi = epi; a.y = y; a.y_ld = y_ld; a.resid = resid; a.resid_ld = resid_ld;
  a.kcache = kcache; a.vcache = vcache; a.cache_bs = cache_bs; a.d_pos = d_pos; a.D = D; a.lag = lag;
  return launch_gemv(a, 1, (hipStream_t)stream);
}
// the family of such a launch ("" = refused) and whether the decode step picks the form for LayerNorm -> W [N][K] at R rows
const char* wht_gemv_family_ln_post(int dtype, int pro, int epi, int R, int N, int K, int ln_folded, int has_xh, int has_xc) {
  static float some_f = 0.f;
  GemvArgs a;
  memset(&a, 0, sizeof a);
  a.pro = pro; a.epi = epi; a.R = R; a.N = N; a.K = K; a.x_ld = a.xf_ld = K; a.ln_folded = ln_folded; a.splits = 2; a.H = K / 64;
  a.xh = has_xh ? &some_f : nullptr; a.xc = has_xc ? &some_f : nullptr;
  return gemv_family(a, dtype);
}
int wht_gemv8_ln_post_pays(int R, int N, int K) { return gemv8_ln_post_pays(R, N, K) ? 1 : 0; }

int wht_merge_partials(const void* part_o, const float* part_ml, int splits, int R, int H, void* out, int64_t o_ld,
                       int dtype, int o_frag, void* stream) {
  return launch_merge_partials(part_o, part_ml, splits, R, H, out, o_ld, dtype, (hipStream_t)stream, o_frag);
}

int wht_attn_decode(int dtype, const void* q, int64_t q_ld, const void* k, int64_t k_ld, int64_t k_bs, const void* v,
                    int64_t v_ld, int64_t v_bs, int64_t kv_hs, int H, int R, int kv_group, int Tk, const int* d_len,
                    int len_plus, const int* lag, int splits, void* out, int64_t o_ld, int o_frag, void* part_o,
                    float* part_ml, int* merge_cnt, const void* vt, int64_t vt_ld, int64_t vt_bs, void* stream) {
  DecAttnArgs a;
  memset(&a, 0, sizeof a);
  a.q = q; a.q_ld = q_ld; a.k = k; a.k_ld = k_ld; a.k_bs = k_bs; a.v = v; a.v_ld = v_ld; a.v_bs = v_bs; a.kv_hs = kv_hs;
  a.H = H; a.R = R; a.kv_group = kv_group; a.Tk = Tk; a.d_len = d_len; a.len_plus = len_plus; a.lag = lag;
  a.splits = splits; a.out = out; a.o_ld = o_ld; a.o_frag = o_frag; a.part_o = part_o; a.part_ml = part_ml;
  a.merge_cnt = merge_cnt; a.vt = vt; a.vt_ld = vt_ld; a.vt_bs = vt_bs;
  return launch_attn_decode(a, dtype, (hipStream_t)stream);
}

int wht_gemm(int dtype, int out_f32, int batch, const void* A, int64_t lda, int64_t a_bs, const void* W, int64_t ldw,
             int64_t w_bs, void* C, int64_t ldc, int64_t c_bs, const float* bias, int bias_on_m, const float* res,
             int64_t ldr, int64_t r_bs, int res_mod, int act, int M, int N, int K, void* stream) {
  GemmArgs a;
  memset(&a, 0, sizeof a);
  a.A = A; a.lda = lda; a.a_bs = a_bs; a.W = W; a.ldw = ldw; a.w_bs = w_bs; a.C = C; a.ldc = ldc; a.c_bs = c_bs;
  a.bias = bias; a.bias_on_m = bias_on_m; a.res = res; a.ldr = ldr; a.r_bs = r_bs; a.res_mod = res_mod; a.act = act;
  a.M = M; a.N = N; a.K = K;
  return launch_gemm(a, dtype, out_f32, batch, (hipStream_t)stream);
}

int wht_attn_flash_f16(const void* q, int64_t q_ld, int64_t q_bs, const void* k, int64_t k_ld, int64_t k_bs,
                       const void* vt, int64_t vt_ld, int64_t vt_bs, void* out, int64_t o_ld, int64_t o_bs, int B, int H,
                       int T, int prescaled, int Tq, void* stream) {
  return launch_attn_flash_f16(q, q_ld, q_bs, k, k_ld, k_bs, vt, vt_ld, vt_bs, out, o_ld, o_bs, B, H, T, prescaled,
                               (hipStream_t)stream, Tq);
}

int wht_layernorm(const float* x, int64_t ldx, const float* w, const float* b, void* out, int64_t ldo, int64_t rows, int D,
                  int dtype, void* stream) {
  return launch_layernorm(x, ldx, w, b, out, ldo, rows, D, dtype, (hipStream_t)stream);
}

int wht_scatter_kv(const void* qkv, int R, int T0, int D, const int* d_offset, int n_ctx, void* kcache, void* vcache,
                   int dtype, void* stream) {
  return launch_scatter_kv(qkv, R, T0, D, d_offset, n_ctx, kcache, vcache, dtype, (hipStream_t)stream);
}

int wht_gather_cache(const void* src, void* dst, const int* src_idx, int R, int64_t row_bytes, int64_t used_bytes,
                     void* stream) {
  return launch_gather_cache(src, dst, src_idx, R, row_bytes, used_bytes, (hipStream_t)stream);
}

int wht_permute_groups(void* k_base, void* v_base, int n_layers, int64_t layer_bytes, int n_audio, int G, int64_t row_bytes,
                       int64_t used_bytes, const int* src_idx, const int* copy_from, int64_t pos_bytes, void* stream) {
  return launch_permute_groups(k_base, v_base, n_layers, layer_bytes, n_audio, G, row_bytes, used_bytes, src_idx, copy_from,
                               pos_bytes, (hipStream_t)stream);
}

int wht_replicate_row(void* base, int64_t layer_bytes, int n_layers, int64_t row_bytes, int src_row, int dst_row0, int G,
                      int64_t used_bytes, void* stream) {
  return launch_replicate_row(base, layer_bytes, n_layers, row_bytes, src_row, dst_row0, G, used_bytes, (hipStream_t)stream);
}

// the fused projection + log-sum-exp + target gather (score.hip); wht_score_slice / wht_score_scratch_bytes: the slice
// width the kernel's add chain follows from, and the partials it needs
int wht_score_slice() { return SCORE_BN; }
size_t wht_score_scratch_bytes(int64_t M, int V) { return score_scratch_bytes(M, V); }
int wht_score(int dtype, const void* xn, int64_t ldx, const void* W, int64_t ldw, const int* target, int M, int K, int V,
              int v_end, float* logprob, float* top_logprob, int* top_token, void* scratch, size_t scratch_bytes,
              void* stream) {
  return launch_score(xn, ldx, W, ldw, target, M, K, V, v_end, logprob, top_logprob, top_token, scratch, scratch_bytes,
                      dtype, (hipStream_t)stream);
}

// the rows and stock logit rules of a sampler or beam launch (RuleArgs) from the flat arguments
static RuleArgs rule_args(const float* logits, int64_t logits_ld, int R, int V, int64_t token_stride, const int* d_ntok,
                          const int* lag, int sample_begin, int eot, int timestamp_begin, int no_timestamps, int max_initial_ts,
                          int suppress_blank, int blank_token, const uint8_t* suppress_mask, float* sum_logprobs) {
  RuleArgs r;
  memset(&r, 0, sizeof r);
  r.logits = logits; r.logits_ld = logits_ld; r.R = R; r.V = V; r.token_stride = token_stride; r.d_ntok = d_ntok; r.lag = lag;
  r.sample_begin = sample_begin; r.eot = eot; r.timestamp_begin = timestamp_begin; r.no_timestamps = no_timestamps;
  r.max_initial_ts = max_initial_ts; r.suppress_blank = suppress_blank; r.blank_token = blank_token;
  r.suppress_mask = suppress_mask; r.sum_logprobs = sum_logprobs;
  return r;
}

// the two sampler launches of one decoding step (sampling.hip) with repetition control (RepArgs; (0, 1.0) = none).
// row_state: int [R][4], slot 3 = the row's trie node — a test puts a row into any node there; `span` ([R][2] ints,
// scratch) is filled here from those nodes, as the previous step's final kernel would have left it.  child_begin == NULL:
// the unbiased instantiations.
// `ts` (per-token statistics, TokenStatArgs) is handed on as given; NULL: the instantiations without them.
static int greedy_sample_any(const float* logits, int64_t logits_ld, int R, int V, int64_t* tokens, int64_t token_stride,
                             const int* d_ntok, const int* lag, int sample_begin, int eot, int timestamp_begin, int no_timestamps,
                             int max_initial_ts, int suppress_blank, int blank_token, const uint8_t* suppress_mask,
                             float* sum_logprobs, int64_t* step_tokens, int* d_alive_step, float* partials, size_t partials_bytes,
                             float temperature, uint64_t seed, int* row_state, int n_nodes, int n_edges, const int* child_begin,
                             const int* child_token, const int* child_node, const int* root_child, int* span, float boost,
                             int no_repeat_ngram_size, float repetition_penalty, const TokenStatArgs* ts, void* stream) {
  if (R < 1 || V < 1 || partials_bytes < greedy_sample_scratch_bytes(R, V)) return hipErrorInvalidValue;
  SampleArgs a;
  memset(&a, 0, sizeof a);
  a.rules = rule_args(logits, logits_ld, R, V, token_stride, d_ntok, lag, sample_begin, eot, timestamp_begin, no_timestamps,
                      max_initial_ts, suppress_blank, blank_token, suppress_mask, sum_logprobs);
  a.tokens = tokens; a.step_tokens = step_tokens; a.d_alive_step = d_alive_step; a.partials = partials; a.row_state = row_state;
  if (temperature > 0.f) {
    a.inv_temperature = 1.0f / temperature;
    a.seed_lo = (uint32_t)(seed & 0xffffffffu); a.seed_hi = (uint32_t)(seed >> 32);
  }
  const RepArgs rep{no_repeat_ngram_size, repetition_penalty};
  if (!child_begin) return launch_greedy_sample(a, (hipStream_t)stream, nullptr, &rep, ts);
  PhraseArgs ph;
  memset(&ph, 0, sizeof ph);
  ph.child_begin = child_begin; ph.child_token = child_token; ph.child_node = child_node; ph.root_child = root_child;
  ph.span = span; ph.n_nodes = n_nodes; ph.n_edges = n_edges; ph.boost = boost;
  const hipError_t e = launch_phrase_span(row_state, child_begin, n_nodes, R, span, (hipStream_t)stream);
  if (e != hipSuccess) return e;
  return launch_greedy_sample(a, (hipStream_t)stream, &ph, &rep, ts);
}
int wht_greedy_sample_rep(const float* logits, int64_t logits_ld, int R, int V, int64_t* tokens, int64_t token_stride,
                          const int* d_ntok, const int* lag, int sample_begin, int eot, int timestamp_begin, int no_timestamps,
                          int max_initial_ts, int suppress_blank, int blank_token, const uint8_t* suppress_mask,
                          float* sum_logprobs, int64_t* step_tokens, int* d_alive_step, float* partials, size_t partials_bytes,
                          float temperature, uint64_t seed, int* row_state, int n_nodes, int n_edges, const int* child_begin,
                          const int* child_token, const int* child_node, const int* root_child, int* span, float boost,
                          int no_repeat_ngram_size, float repetition_penalty, void* stream) {
  return greedy_sample_any(logits, logits_ld, R, V, tokens, token_stride, d_ntok, lag, sample_begin, eot, timestamp_begin,
                           no_timestamps, max_initial_ts, suppress_blank, blank_token, suppress_mask, sum_logprobs, step_tokens,
                           d_alive_step, partials, partials_bytes, temperature, seed, row_state, n_nodes, n_edges, child_begin,
                           child_token, child_node, root_child, span, boost, no_repeat_ngram_size, repetition_penalty, nullptr,
                           stream);
}
// ... with per-token statistics (TokenStatArgs) written to the column each row's token goes to: token_logprob / entropy
// [R][stat_stride], top_token / top_logprob [R][stat_stride][top_k]; any of them may be NULL.  top_scratch: the chunks' best
// entries (wht_greedy_sample_top_scratch_bytes; refused when smaller and top_k > 0).  The launcher's own refusals (top_k
// outside 0 .. 8, a missing top buffer, no buffer at all, stat_stride < token_stride) come back unchanged, nothing launched.
size_t wht_greedy_sample_top_scratch_bytes(int R, int V) { return greedy_sample_top_scratch_bytes(R, V); }
int wht_greedy_sample_stats(const float* logits, int64_t logits_ld, int R, int V, int64_t* tokens, int64_t token_stride,
                            const int* d_ntok, const int* lag, int sample_begin, int eot, int timestamp_begin, int no_timestamps,
                            int max_initial_ts, int suppress_blank, int blank_token, const uint8_t* suppress_mask,
                            float* sum_logprobs, int64_t* step_tokens, int* d_alive_step, float* partials, size_t partials_bytes,
                            float temperature, uint64_t seed, int* row_state, int n_nodes, int n_edges, const int* child_begin,
                            const int* child_token, const int* child_node, const int* root_child, int* span, float boost,
                            int no_repeat_ngram_size, float repetition_penalty, float* token_logprob, float* entropy, int top_k,
                            int* top_token, float* top_logprob, int64_t stat_stride, void* top_scratch, size_t top_scratch_bytes,
                            void* stream) {
  if (R < 1 || V < 1) return hipErrorInvalidValue;
  if (top_k > 0 && top_scratch && top_scratch_bytes < greedy_sample_top_scratch_bytes(R, V)) return hipErrorInvalidValue;
  TokenStatArgs ts;
  memset(&ts, 0, sizeof ts);
  ts.token_logprob = token_logprob; ts.entropy = entropy; ts.top_k = top_k; ts.top_token = top_token; ts.top_logprob = top_logprob;
  ts.stride = stat_stride; ts.scratch = top_scratch;
  return greedy_sample_any(logits, logits_ld, R, V, tokens, token_stride, d_ntok, lag, sample_begin, eot, timestamp_begin,
                           no_timestamps, max_initial_ts, suppress_blank, blank_token, suppress_mask, sum_logprobs, step_tokens,
                           d_alive_step, partials, partials_bytes, temperature, seed, row_state, n_nodes, n_edges, child_begin,
                           child_token, child_node, root_child, span, boost, no_repeat_ngram_size, repetition_penalty, &ts,
                           stream);
}
// ... and without it: launch_greedy_sample maps (0, 1.0) to the plain instantiations
int wht_greedy_sample(const float* logits, int64_t logits_ld, int R, int V, int64_t* tokens, int64_t token_stride,
                      const int* d_ntok, const int* lag, int sample_begin, int eot, int timestamp_begin, int no_timestamps,
                      int max_initial_ts, int suppress_blank, int blank_token, const uint8_t* suppress_mask,
                      float* sum_logprobs, int64_t* step_tokens, int* d_alive_step, float* partials, size_t partials_bytes,
                      float temperature, uint64_t seed, int* row_state, int n_nodes, int n_edges, const int* child_begin,
                      const int* child_token, const int* child_node, const int* root_child, int* span, float boost,
                      void* stream) {
  return wht_greedy_sample_rep(logits, logits_ld, R, V, tokens, token_stride, d_ntok, lag, sample_begin, eot, timestamp_begin,
                               no_timestamps, max_initial_ts, suppress_blank, blank_token, suppress_mask, sum_logprobs,
                               step_tokens, d_alive_step, partials, partials_bytes, temperature, seed, row_state, n_nodes,
                               n_edges, child_begin, child_token, child_node, root_child, span, boost, 0, 1.0f, stream);
}
// the stock logit rules on the host (logit_rules.h; nothing is launched): mask[v] = 1 where token v is -inf for a row that
// holds `row`: ntok - lag tokens, the last ntok - sample_begin of them sampled (both the longest row's, as on the device).
// The timestamp window, returned as {last_ts, pen_ts, lo, hi}, comes from `row_state` [3] where given, else from the tokens.
void wht_rule_mask(const int64_t* row, int ntok, int lag, int V, int sample_begin, int eot, int timestamp_begin,
                   int no_timestamps, int max_initial_ts, int suppress_blank, int blank_token, const uint8_t* suppress_mask,
                   const int* row_state, uint8_t* mask, int* window) {
  const RuleArgs r = rule_args(nullptr, 0, 1, V, 0, nullptr, nullptr, sample_begin, eot, timestamp_begin, no_timestamps,
                               max_initial_ts, suppress_blank, blank_token, suppress_mask, nullptr);
  const RowPos pos = row_pos_of(r, ntok, lag);
  int last = -1;                                     // the index in H of its last timestamp
  for (int t = 0; t < pos.L && timestamp_begin >= 0; ++t)
    if (row[pos.sample_begin + t] >= timestamp_begin) last = t;
  const TsWindow w = row_state ? ts_window_of_state(r, pos, row_state[0], row_state[1], row_state[2])
                               : ts_window_of_history(r, pos, row, last);
  window[0] = w.last_ts; window[1] = w.pen_ts; window[2] = w.lo; window[3] = w.hi;
  for (int v = 0; v < V; ++v) mask[v] = rule_masked(r, pos, w, v) ? 1 : 0;
}
size_t wht_greedy_sample_scratch_bytes(int R, int V) { return greedy_sample_scratch_bytes(R, V); }
// the sampler's noise (sample_noise.h) on the host; nothing is launched.  wht_sample_uniform_range: the uniforms of `count`
// consecutive values, from `first`, of the wht_sample_uniform_bits() top bits of a hash that the map uses
uint32_t wht_sample_hash(uint64_t seed, int step, int row, int token) {
  return sample_hash((uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), step, row, token);
}
float wht_sample_uniform_of_hash(uint32_t h) { return sample_uniform_of_hash(h); }
int wht_sample_uniform_bits() { return SAMPLE_UNIFORM_BITS; }
void wht_sample_uniform_range(uint32_t first, uint32_t count, float* out) {
  for (uint32_t i = 0; i < count; ++i) out[i] = sample_uniform_of_hash((first + i) << (32 - SAMPLE_UNIFORM_BITS));
}
// the hashes of `count` (seed, step, row, token) tuples in one call
void wht_sample_hash_many(const uint64_t* seed, const int* step, const int* row, const int* token, int64_t count, uint32_t* out) {
  for (int64_t i = 0; i < count; ++i) out[i] = wht_sample_hash(seed[i], step[i], row[i], token[i]);
}
int wht_phrase_root_table(const int* child_begin, const int* child_token, const int* child_node, int n_edges, int V, int* root,
                          void* stream) {
  return launch_phrase_root_table(child_begin, child_token, child_node, n_edges, V, root, (hipStream_t)stream);
}

// the fused attention launches of one decode step (xattn.hip): LayerNorm + projection + attention in one launch.  `mode` is
// passed through (bit 0: scalar-path polls); att_in / x_out and the other optional-stage fields stay null, except that
// `out_w` (cross) and `x_out` (self) are handed on as given so that a test can reach the launchers' refusal of the stages
// the shipped build does not contain.
int wht_xattn_supported(int D, int H, int R, int kv_group, int Tk, int splits) {
  return xattn_supported(D, H, R, kv_group, Tk, splits) ? 1 : 0;
}
int wht_sattn_supported(int D, int H, int R, int n_ctx) { return sattn_supported(D, H, R, n_ctx) ? 1 : 0; }
int wht_fused_mode(int kind) { return fused_mode(kind); }
int wht_xattn8(const float* xf, int64_t xf_ld, const void* W, const float* bias, int D, int H, int R, const void* k,
               int64_t k_ld, int64_t k_bs, const void* v, int64_t v_ld, int64_t v_bs, int Tk, int splits, void* out,
               int64_t o_ld, void* part_o, float* part_ml, unsigned long long* qg, const int* d_tick, int epoch, int layer,
               int* err, int mode, const void* out_w, void* stream) {
  XAttnArgs a;
  memset(&a, 0, sizeof a);
  a.xf = xf; a.xf_ld = xf_ld; a.W = W; a.bias = bias; a.D = D; a.H = H; a.R = R;
  a.k = k; a.k_ld = k_ld; a.k_bs = k_bs; a.v = v; a.v_ld = v_ld; a.v_bs = v_bs; a.Tk = Tk; a.splits = splits;
  a.out = out; a.o_ld = o_ld; a.part_o = part_o; a.part_ml = part_ml;
  a.qg = qg; a.d_tick = d_tick; a.epoch = epoch; a.layer = layer; a.err = err; a.mode = mode; a.out_w = out_w;
  return launch_xattn8(a, (hipStream_t)stream);
}
int wht_sattn8(const float* xf, int64_t xf_ld, const void* W, const float* bias, int D, int H, int R, void* kcache,
               void* vcache, int64_t cache_bs, const int* d_pos, const int* lag, void* q_out, void* out, int64_t o_ld,
               unsigned long long* qg, const int* d_tick, int epoch, int layer, int* err, int mode, float* x_out,
               void* stream) {
  SAttnArgs a;
  memset(&a, 0, sizeof a);
  a.xf = xf; a.xf_ld = xf_ld; a.W = W; a.bias = bias; a.D = D; a.H = H; a.R = R;
  a.kcache = kcache; a.vcache = vcache; a.cache_bs = cache_bs; a.d_pos = d_pos; a.lag = lag; a.q_out = q_out;
  a.out = out; a.o_ld = o_ld; a.qg = qg; a.d_tick = d_tick; a.epoch = epoch; a.layer = layer; a.err = err; a.mode = mode;
  a.x_out = x_out;
  return launch_sattn8(a, (hipStream_t)stream);
}

// one beam-search update (beam.hip): the three launches of launch_beam_step on caller-supplied buffers.  B, G, K and R
// are independent so that the launcher's own refusals can be reached; lag, lcp / copy_from and suppress_mask may be NULL.
// `scratch` (wht_beam_scratch_bytes(R, V) bytes) is carved with beam_scratch_carve; wht_beam_cand_offsets gives the byte
// offsets of cand_lp / cand_tok ([R][BEAM_KMAX] each) inside it, so a test reads the candidates the update kernel saw.
int wht_beam_kmax() { return BEAM_KMAX; }
size_t wht_beam_scratch_bytes(int R, int V) { return beam_scratch_bytes(R, V); }
void wht_beam_cand_offsets(int R, int V, int64_t* lp_off, int64_t* tok_off) {
  BeamArgs a;
  memset(&a, 0, sizeof a);
  const uintptr_t base = 4096;
  beam_scratch_carve(a, (void*)base, R, V);
  *lp_off = (int64_t)((uintptr_t)a.cand_lp - base);
  *tok_off = (int64_t)((uintptr_t)a.cand_tok - base);
}
int wht_beam_step(const float* logits, int64_t logits_ld, int B, int G, int K, int R, int V, const int64_t* tokens_in,
                  int64_t* tokens_out, int64_t token_stride, const int* d_ntok, const int* lag, int sample_begin, int eot,
                  int timestamp_begin, int no_timestamps, int max_initial_ts, int suppress_blank, int blank_token,
                  const uint8_t* suppress_mask, float* sum_logprobs, void* scratch, size_t scratch_bytes, int64_t* fin_tok,
                  int* fin_len, float* fin_score, int* fin_count, int max_candidates, int* src, int* lcp, int* copy_from,
                  int64_t* step_tokens, const int* done_prev, int* done_next, int* d_applied, int first, void* stream) {
  if (R < 1 || V < 1 || !scratch || scratch_bytes < beam_scratch_bytes(R, V)) return hipErrorInvalidValue;
  BeamArgs a;
  memset(&a, 0, sizeof a);
  a.rules = rule_args(logits, logits_ld, R, V, token_stride, d_ntok, lag, sample_begin, eot, timestamp_begin, no_timestamps,
                      max_initial_ts, suppress_blank, blank_token, suppress_mask, sum_logprobs);
  a.G = G; a.K = K; a.tokens_in = tokens_in; a.tokens_out = tokens_out;
  beam_scratch_carve(a, scratch, R, V);
  a.fin_tok = fin_tok; a.fin_len = fin_len; a.fin_score = fin_score; a.fin_count = fin_count;
  a.max_candidates = max_candidates; a.src = src; a.lcp = lcp; a.copy_from = copy_from; a.step_tokens = step_tokens;
  a.done_prev = done_prev; a.done_next = done_next; a.d_applied = d_applied; a.first = first;
  return launch_beam_step(a, B, (hipStream_t)stream);
}

// open-end dtw, end selection and back-trace (timing.hip) on caller-supplied cost matrices [clips][Nmax][Fmax]; d_rows /
// d_cols / d_closed device int [clips]; path (optional) as launch_dtw_backtrace_batch lays it out
int wht_dtw_open(const float* cost, const int* d_rows, const int* d_cols, const int* d_closed, int clips, int Nmax, int Fmax,
                 float end_slack, int8_t* trace, int64_t trace_bs, float* lastcol, int* end, int* jumps, int64_t jump_stride,
                 int* path, int64_t path_stride, int* path_len, void* stream) {
  if (!cost || !d_rows || !d_cols || !d_closed || !trace || !lastcol || !end || !jumps || !path_len || jump_stride < Nmax ||
      (path && path_stride < (int64_t)Nmax + Fmax))
    return hipErrorInvalidValue;
  const hipError_t e = launch_dtw_open_batch(cost, d_rows, d_cols, d_closed, clips, Nmax, Fmax, end_slack, trace, trace_bs,
                                             lastcol, end, (hipStream_t)stream);
  if (e != hipSuccess) return e;
  return launch_dtw_backtrace_batch(trace, trace_bs, end, d_cols, clips, Nmax, Fmax, jumps, jump_stride, path, path_stride,
                                    path_len, (hipStream_t)stream);
}

// generic attention (decoder prefill, non-flash cross attention, the fp32 encoder): every AttnArgs field as given
int wht_attn_generic(int dtype, int batch, const void* q, int64_t q_ld, int64_t q_bs, const void* k, int64_t k_ld, int64_t k_bs,
                     const void* v, int64_t v_ld, int64_t v_bs, void* out, int64_t o_ld, int64_t o_bs, int H, int Tq, int Tk,
                     const int* d_len, int causal, int kv_group, void* stream) {
  AttnArgs a;
  memset(&a, 0, sizeof a);
  a.q = q; a.q_ld = q_ld; a.q_bs = q_bs; a.k = k; a.k_ld = k_ld; a.k_bs = k_bs; a.v = v; a.v_ld = v_ld; a.v_bs = v_bs;
  a.out = out; a.o_ld = o_ld; a.o_bs = o_bs; a.H = H; a.Tq = Tq; a.Tk = Tk; a.d_len = d_len; a.causal = causal;
  a.kv_group = kv_group;
  return launch_attn_generic(a, batch, dtype, (hipStream_t)stream);
}

// the word-timestamp score planes: one (q, k, head), and every (row, pair) plane of a batch
int wht_cross_qk(const void* q, int64_t q_ld, const void* k, int64_t k_ld, int head, int n_tok, int Tk, float* out, int dtype,
                 void* stream) {
  return launch_cross_qk(q, q_ld, k, k_ld, head, n_tok, Tk, out, dtype, (hipStream_t)stream);
}
int wht_cross_qk_batch(const void* qcap, int64_t q_layer_stride, int64_t q_row_stride, int D, const void* cross_kv,
                       int64_t kv_layer_stride, int64_t kv_audio_stride, int kv_group, const int* d_layers, const int* d_heads,
                       int n_pairs, const int* d_ntok, int R, int Tmax, int Tk, float* out, int dtype, void* stream) {
  return launch_cross_qk_batch(qcap, q_layer_stride, q_row_stride, D, cross_kv, kv_layer_stride, kv_audio_stride, kv_group,
                               d_layers, d_heads, n_pairs, d_ntok, R, Tmax, Tk, out, dtype, (hipStream_t)stream);
}

// the alignment pipeline on a caller-owned scratch of 2 * clips * H * Tmax * Fmax floats: afterwards its first half holds
// softmax + z-norm, its second half the median
int wht_align_batch(const float* qk, const int* d_ntok, const int* d_nfr, int clips, int H, int Tmax, int Tk, int Fmax,
                    int width, int row_begin, int row_tail, float qk_scale, float* cost, int Nmax, float* scratch,
                    void* stream) {
  return launch_align_batch(qk, d_ntok, d_nfr, clips, H, Tmax, Tk, Fmax, width, row_begin, row_tail, qk_scale, cost, Nmax,
                            scratch, (hipStream_t)stream);
}
int wht_dtw(const float* x, int N, int M, int8_t* trace, void* stream) { return launch_dtw(x, N, M, trace, (hipStream_t)stream); }
int wht_dtw_batch(const float* cost, const int* d_ntok, const int* d_nfr, int clips, int Tmax, int Fmax, int row_begin,
                  int row_tail, int Nmax, int8_t* trace, int64_t trace_bs, void* stream) {
  return launch_dtw_batch(cost, d_ntok, d_nfr, clips, Tmax, Fmax, row_begin, row_tail, Nmax, trace, trace_bs,
                          (hipStream_t)stream);
}

// the small kernels around the encoder stem, the prefill and the sampler
int wht_mel_transpose(const void* mel, int mel_is_f16, int B, int n_mels, int F, void* out, int dtype, void* stream) {
  return launch_mel_transpose(mel, mel_is_f16, B, n_mels, F, out, dtype, (hipStream_t)stream);
}
int wht_embed(const int64_t* tokens, int64_t stride, int R, int T0, const void* tok_emb, const float* pos, const int* d_offset,
              const int* lag, int D, int n_vocab, float* x, int dtype, void* stream) {
  return launch_embed(tokens, stride, R, T0, tok_emb, pos, d_offset, lag, D, n_vocab, x, dtype, (hipStream_t)stream);
}
int wht_no_speech(const float* logits_row0, int64_t row_stride, int R, int V, int no_speech, float* out, void* stream) {
  return launch_no_speech(logits_row0, row_stride, R, V, no_speech, out, (hipStream_t)stream);
}
int wht_gather_rows(const float* x, const int* sel, int n_sel, int D, float* out, void* stream) {
  return launch_gather_rows(x, sel, n_sel, D, out, (hipStream_t)stream);
}
int wht_gather_tokens(const int64_t* src, int64_t stride, int R, int64_t* dst, void* stream) {
  return launch_gather_tokens(src, stride, R, dst, (hipStream_t)stream);
}

// flac.hip, stage by stage on a caller-supplied scratch (flac_scratch layout, >= wht_flac_scratch_bytes).  wht_flac_scan: the
// candidate list of file[first, size) -> host n_found [1] (all candidates; the list holds min(n_found, max_cand)), start / bs /
// prov [max_cand].  wht_flac_decode (after wht_flac_scan on the same scratch): every listed candidate decoded into pcm
// [staging_frames][ch] -> host end / rc [max_cand].  Both wait for the stream.
size_t wht_flac_scratch_bytes(size_t size, int ch, int64_t staging_frames, int max_cand) {
  return flac_scratch(nullptr, size, ch, staging_frames, max_cand).total_bytes;
}
int wht_flac_scan(const uint8_t* file, size_t size, size_t first, int ch, int bps, int max_block, int max_cand,
                  int64_t staging_frames, void* scratch, int* n_found, int64_t* start, int* bs, int64_t* prov, void* stream) {
  if (!file || !scratch || !n_found || !start || !bs || !prov || first >= size || max_cand < 1) return hipErrorInvalidValue;
  const FlacScratch s = flac_scratch(scratch, size, ch, staging_frames, max_cand);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_flac_scan(file, size, first, ch, bps, max_block, s, max_cand, st);
  if (e != hipSuccess) return e;
  int hdr[2];
  if ((e = hipMemcpyAsync(hdr, s.hdr, sizeof hdr, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  *n_found = hdr[1];
  const size_t n = (size_t)hdr[0];
  if ((e = hipMemcpy(start, s.start, n * 8, hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if ((e = hipMemcpy(bs, s.bs, n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return e;
  return hipMemcpy(prov, s.prov, n * 8, hipMemcpyDeviceToHost);
}
int wht_flac_decode(const uint8_t* file, size_t size, int ch, int bps, int max_cand, int64_t staging_frames, int32_t* pcm,
                    void* scratch, int64_t* end, int* rc, void* stream) {
  if (!file || !scratch || !pcm || !end || !rc || max_cand < 1) return hipErrorInvalidValue;
  const FlacScratch s = flac_scratch(scratch, size, ch, staging_frames, max_cand);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_flac_decode(file, size, ch, bps, s, max_cand, pcm, staging_frames, st);
  if (e != hipSuccess) return e;
  int n = 0;
  if ((e = hipMemcpyAsync(&n, s.hdr, sizeof n, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  if ((e = hipMemcpy(end, s.end, (size_t)n * 8, hipMemcpyDeviceToHost)) != hipSuccess) return e;
  return hipMemcpy(rc, s.rc, (size_t)n * 4, hipMemcpyDeviceToHost);
}

}  // extern "C"
