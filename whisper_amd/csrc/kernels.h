// kernels.h — internal launcher interface between api.cpp and the .hip kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// developer probe (tools/probe_decode.cpp builds the kernels with -DWH_PROBE): thread 0 of every
// workgroup records s_memtime at phase boundaries.  Compiled out of libwhisper_hip.so.
#ifdef WH_PROBE
#define WH_PROBE_FIELD long long* probe;
#define WH_PROBE_KVHS_FIELD int64_t kv_hs;   /* probe builds only: head stride of the cross K / V (0 = 64: heads side by side in a key row) */
#define WH_PROBE_AT(args, wg, i) \
  do { if ((args).probe && threadIdx.x == 0) (args).probe[(size_t)(wg) * 8 + (i)] = clock64(); } while (0)
#else
#define WH_PROBE_FIELD
#define WH_PROBE_KVHS_FIELD
#define WH_PROBE_AT(args, wg, i) do {} while (0)
#endif

// Developer A/B switches (tools/README.md): environment variables are read ONLY by the -DWH_DEV build
// (`make dev` -> libwhisper_hip_dev.so, loaded by the tools through WHISPER_AMD_LIB); in the shipped library every
// switch is the constant of the measured-faster form and its name does not exist in the binary.  The one variable the
// shipped library reads is WH_NO_GRAPH (api.cpp: decode steps launched eagerly — a support switch, not an experiment).
#ifdef WH_DEV
#include <stdlib.h>
#define WH_DEV_FLAG(name) ([] { static const bool v = [] { const char* e = getenv(name); return e && e[0] == '1'; }(); return v; }())
#define WH_DEV_INT(name) ([] { static const int v = [] { const char* e = getenv(name); return e ? atoi(e) : 0; }(); return v; }())
#else
#define WH_DEV_FLAG(name) false
#define WH_DEV_INT(name) 0
#endif

#include <atomic>
#include <stdio.h>
#include <string>
namespace whk {

// Form tag: every terminal dispatch branch of launch_gemv, launch_attn_decode, launch_gemm and launch_merge_partials stores
// a stable name of the kernel form it picked ("gemv8/LN/gs3/ks2/xw8/rt3", "rt<half,8>/pro<8,0,16,4>", "attn/group_diag").
// Host only, one store per host call, nothing on the device and no extra launch; decode steps replay from a graph, so the
// store costs nothing there.  Read by the kernel test library (ktest.cpp: wht_last_form) to prove every form is reached.
extern thread_local const char* g_form;
// a name built once per template instantiation (the pointer stays valid for the life of the process)
#define WH_FORM_NAME(...) ([&] { static const std::string s_ = [&] { char b_[96]; snprintf(b_, sizeof b_, __VA_ARGS__); \
                                                                     return std::string(b_); }(); return s_.c_str(); }())

// Dynamic LDS above 64 KB is a per-DEVICE function attribute (hipFuncSetAttribute): raise it once on every device this
// process launches `fn` on.  `c` is the call site's own cache (function-local static).
struct LdsAttr { std::atomic<int> done[64]; };
inline hipError_t raise_dynamic_lds(LdsAttr& c, const void* fn, int bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (c.done[dev].load(std::memory_order_acquire) == 1) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) c.done[dev].store(1, std::memory_order_release);
  else (void)hipGetLastError();
  return e;
}

// dtype: 0 = fp32, 1 = fp16 (matches WH_F32 / WH_F16)

// ---- mel.hip -------------------------------------------------------------------------------
hipError_t launch_log_mel(const float* audio, int64_t n_samples, int batch, int n_mels,
                          const float* filters, const float* tables, float* out, void* scratch,
                          hipStream_t stream);

// ---- gemm.hip ------------------------------------------------------------------------------
struct GemmArgs {
  const void* A; int64_t lda; int64_t a_bs;     // [M][K], row stride lda (elements), batch stride
  const void* W; int64_t ldw; int64_t w_bs;     // [N][K]
  void* C; int64_t ldc; int64_t c_bs;           // [M][N]
  const float* bias; int bias_on_m;             // per-n (default) or per-m bias
  const float* res; int64_t ldr; int64_t r_bs; int res_mod;  // fp32 residual, row index m % res_mod if res_mod>0
  int act;                                      // 0 none, 1 exact GELU
  int M, N, K;
  int tiles_m, tiles_n, persistent;             // filled by the launcher
  int serial_epilogue;                          // filled by the launcher: A/B switch WH_GEMM_SERIAL_EPILOGUE=1 (gemm.hip)
  WH_PROBE_FIELD
};
hipError_t launch_gemm(const GemmArgs& a, int dtype, int out_f32, int batch, hipStream_t stream);

// ---- elementwise.hip -----------------------------------------------------------------------
// mel [B][n_mels][F] (fp32 or fp16) -> [B][F+2][n_mels] element type with zero rows 0 and F+1
hipError_t launch_mel_transpose(const void* mel, int mel_is_f16, int B, int n_mels, int F, void* out,
                                int dtype, hipStream_t stream);
// fp32 x [rows][D] (row stride ldx) -> element-type out [rows][D] (row stride ldo)
hipError_t launch_layernorm(const float* x, int64_t ldx, const float* w, const float* b, void* out,
                            int64_t ldo, int64_t rows, int D, int dtype, hipStream_t stream);
// x[r*T0+t][:] = tok_emb[tokens[r*stride+t]][:] + pos[(offset - lag[r] + t)][:]   (fp32 out; lag may be null)
hipError_t launch_embed(const int64_t* tokens, int64_t stride, int R, int T0, const void* tok_emb,
                        const float* pos, const int* d_offset, const int* lag, int D, int n_vocab, float* x,
                        int dtype, hipStream_t stream);
// qkv [R*T0][3D] -> q [R*T0][D] is left in place (ld 3D); k,v rows scattered to caches [R][n_ctx][D]
hipError_t launch_scatter_kv(const void* qkv, int R, int T0, int D, const int* d_offset, int n_ctx,
                             void* kcache, void* vcache, int dtype, hipStream_t stream);
// out[i][:] = x[sel[i]][:] (fp32 rows of width D); sel device int array
hipError_t launch_gather_rows(const float* x, const int* sel, int n_sel, int D, float* out,
                              hipStream_t stream);
// dst rows <- src rows[src_idx[i]] : self-attention cache gather for beam search (rows of row_elems elements)
hipError_t launch_gather_cache(const void* src, void* dst, const int* src_idx, int R, int64_t row_bytes,
                               int64_t used_bytes, hipStream_t stream);
// in-place beam reorder of every layer's self-attention K and V cache in one launch; src_idx[i] must lie in the
// beam group of row i (groups of G consecutive rows), G <= 8.  copy_from (may be null): row i only needs the cache
// positions >= copy_from[i] of its source — below that the two rows already hold the same bytes (pos_bytes per position)
hipError_t launch_permute_groups(void* k_base, void* v_base, int n_layers, int64_t layer_bytes, int n_audio, int G,
                                 int64_t row_bytes, int64_t used_bytes, const int* src_idx, const int* copy_from,
                                 int64_t pos_bytes, hipStream_t stream);
// the first used_bytes of row src_row -> rows [dst_row0, dst_row0 + G) in each of n_layers slabs (layer_bytes apart)
hipError_t launch_replicate_row(void* base, int64_t layer_bytes, int n_layers, int64_t row_bytes, int src_row, int dst_row0,
                                int G, int64_t used_bytes, hipStream_t stream);
hipError_t launch_add_int(int* p, int v, hipStream_t stream);

// ---- attention.hip -------------------------------------------------------------------------
struct AttnArgs {
  const void* q; int64_t q_ld; int64_t q_bs;      // q rows [Tq] per batch row (element type), head h at cols h*64
  const void* k; int64_t k_ld; int64_t k_bs;      // keys  [Tk] per kv-batch
  const void* v; int64_t v_ld; int64_t v_bs;
  void* out; int64_t o_ld; int64_t o_bs;          // [Tq][H*64] element type
  int H; int Tq; int Tk;                          // Tk used when d_len == nullptr
  const int* d_len;                               // device: cached length BEFORE this call (Tk = *d_len + Tq), or null
  int causal;                                     // query t sees keys <= (Tk - Tq) + t
  int kv_group;                                   // kv batch index = batch / kv_group
  float* qk_out;                                  // unused (reserved)
};
// generic (any Tq/Tk, VALU) attention, used for fp32 parity mode and decoder prefill
hipError_t launch_attn_generic(const AttnArgs& a, int batch, int dtype, hipStream_t stream);
// MFMA flash attention for the encoder (fp16 only): q,k [B][T][..] rows, vt = V transposed [B][H*64][ldv];
// prescaled: q and k each carry sqrt(0.125 * log2 e) already (WH_WEIGHTS_ENC_QK_SCALED)
hipError_t launch_attn_flash_f16(const void* q, int64_t q_ld, int64_t q_bs, const void* k, int64_t k_ld,
                                 int64_t k_bs, const void* vt, int64_t vt_ld, int64_t vt_bs, void* out,
                                 int64_t o_ld, int64_t o_bs, int B, int H, int T, int prescaled, hipStream_t stream, int Tq = 0);
// single-query decode attention with split-K partials
struct DecAttnArgs {
  const void* q; int64_t q_ld;                    // [R][H*64]
  const void* k; int64_t k_ld; int64_t k_bs;      // key j of head h at k + b*k_bs + j*k_ld + h*kv_hs
  const void* v; int64_t v_ld; int64_t v_bs;
  int64_t kv_hs;                                  // head stride in elements: 0 means 64 (heads side by side in a row)
  int H; int R; int kv_group;
  int Tk; const int* d_len; int len_plus;         // Tk fixed, or *d_len + len_plus
  const int* lag;                                 // with d_len: row r holds lag[r] fewer keys (ragged prompts); may be null
  int splits;                                     // key-range splits
  void* out; int64_t o_ld;                        // splits==1: normalized output, element type
  int o_frag;                                     // splits==1, fp16: write `out` in fragment order (GemvArgs::x_frag below); o_ld ignored
  void* part_o; float* part_ml;                   // splits>1: [S][R][H][64] element type, normalised (o / l); (m, l) fp32 [S][R][H][2]
  // fp16, kv_group == 1, 2 <= splits <= 4: [R][H] tickets, all 0 between launches.  With it the last workgroup of a (row, head)
  // to finish merges the partials and writes `out` (o_ld / o_frag as for splits == 1): no merge launch, no PRO_COMBINE after it
  int* merge_cnt;
  // beam groups, fp16: V transposed per audio, row h*64+d holds the keys of head dim d (row stride vt_ld >= the
  // padded key count, pad columns finite).  With it the group kernel runs on the matrix cores; null: vector ALU form
  const void* vt; int64_t vt_ld; int64_t vt_bs;
  WH_PROBE_FIELD
};
constexpr int DEC_ATTN_MAX_SPLITS = 16;
// keys one workgroup of attn_decode can hold in registers (per split)
int attn_decode_capacity(int dtype);
hipError_t launch_attn_decode(const DecAttnArgs& a, int dtype, hipStream_t stream);
// scores of selected (layer, head) pairs: out[pair][t][j] = scale^2 * q[t]·k[j]
// batched: row r (grid.z = r * n_pairs + pair), queries qcap [layer][R][C][D] at positions [0, Tmax), keys of audio
// r / kv_group in cross_kv [layer][B * Tk][2D]; out [R][n_pairs][Tmax][Tk]; positions >= ntok[r] are skipped
hipError_t launch_cross_qk_batch(const void* qcap, int64_t q_layer_stride, int64_t q_row_stride, int D, const void* cross_kv,
                                 int64_t kv_layer_stride, int64_t kv_audio_stride, int kv_group, const int* d_layers,
                                 const int* d_heads, int n_pairs, const int* d_ntok, int R, int Tmax, int Tk, float* out,
                                 int dtype, hipStream_t stream);
hipError_t launch_cross_qk(const void* q, int64_t q_ld, const void* k, int64_t k_ld, int head, int n_tok,
                           int Tk, float* out, int dtype, hipStream_t stream);

// ---- xattn.hip: cross attention of one decode step with its LayerNorm + query projection inside the launch ----------
struct XAttnArgs {
  // projection: q = (W . LN(x) + bias) * d_head^-0.5, LayerNorm affine folded into W / bias (WH_WEIGHTS_DEC_LN_FOLDED)
  const float* xf; int64_t xf_ld;                 // fp32 residual rows [R][D]
  const void* W; const float* bias;               // fp16 [D][D], fp32 [D]
  int D, H, R;
  // cross K/V of row r (one audio per row): key j of head h at k + r*k_bs + j*k_ld + h*64
  // Only keys [0, Tk) of a row are read (slots past a split's end, and every slot of an empty trailing split, re-read a key
  // below Tk), Tk >= 1; nothing of k / v is written.
  const void* k; int64_t k_ld; int64_t k_bs;
  const void* v; int64_t v_ld; int64_t v_bs;
  int Tk, splits;
  void* out; int64_t o_ld;                        // splits == 1
  void* part_o; float* part_ml;                   // splits > 1 (layouts of DecAttnArgs)
  // hand-off of q between workgroups: 8-byte granules {2 x fp16, tag} [R][D/2]; tag = ((*d_tick + 1 + epoch) << 6) | (layer + 1)
  unsigned long long* qg; const int* d_tick; int epoch, layer;
  int* err;                                       // counts bounded spins that ran out (never on a healthy device)
  int mode;                                       // bit 0: granules fetched through the scalar memory path (fused_mode())
  // optional phase 0 (out_w != null): x_io[r][:] += out_w . att_in[r] + out_b (attn.out + residual, model.py:153) by the
  // producer workgroups before their LayerNorm; x_io == xf (in place), pflags = D / 8 eight-byte flag words (zero-initialised
  // once; tags never repeat), att_in = fp16 [R][D] attention rows of the self attention
  const void* att_in; const void* out_w; const float* out_b; float* x_io; unsigned long long* pflags;
  WH_PROBE_FIELD
  WH_PROBE_KVHS_FIELD
};
int fused_mode(int kind);
bool xattn_supported(int D, int H, int R, int kv_group, int Tk, int splits);
hipError_t launch_xattn8(const XAttnArgs& a, hipStream_t stream);
// self attention of one decode step with LayerNorm + QKV projection + KV-cache append inside the launch
struct SAttnArgs {
  const float* xf; int64_t xf_ld;                 // fp32 residual rows [R][D]
  const void* W; const float* bias;               // fp16 [3D][D] = [query; key; value], fp32 [3D] (LayerNorm folded in)
  int D, H, R;
  void* kcache; void* vcache; int64_t cache_bs;   // this layer's self K / V [R][n_ctx][D]; row r appends at *d_pos - lag[r]
  // With Tk = *d_pos - lag[r] + 1 >= 1: positions [0, Tk - 1) of row r are read and must hold the cached keys; position Tk - 1 is
  // the only one written (D elements of K and of V) and its old bytes never reach a result, even at Tk == 1 where the tile
  // loads them; positions >= Tk are neither read nor written.  launch_sattn8 refuses what sattn_supported does (cache_bs / D
  // stands in for n_ctx) with hipErrorNotSupported.
  const int* d_pos; const int* lag;               // lag may be null
  void* q_out;                                    // optional: the unscaled q rows [R][D] (what the two-launch form leaves)
  void* out; int64_t o_ld;                        // attention output [R][D] (when x_out is null)
  // optional third stage, attn.out + residual in the same launch: x_out[r][:] = xf[r][:] + out_w . attention[r] + out_b
  // (x_out must not alias xf); og = granules [R][D/2] the attention workgroups hand their outputs over in
  const void* out_w; const float* out_b; float* x_out; unsigned long long* og;
  unsigned long long* qg; const int* d_tick; int epoch, layer;   // granules [R][3D/2]; tag as in XAttnArgs
  int* err;
  int mode;                                       // bit 0: scalar-path polls
  WH_PROBE_FIELD
};
bool sattn_supported(int D, int H, int R, int n_ctx);
hipError_t launch_sattn8(const SAttnArgs& a, hipStream_t stream);

// ---- gemv.hip ------------------------------------------------------------------------------
enum { PRO_PLAIN = 0, PRO_LN = 1, PRO_COMBINE = 2, PRO_LN_POST = 3 };
enum { EPI_STORE = 0, EPI_QKV = 1, EPI_RESID = 2, EPI_GELU = 3, EPI_F32 = 4 };
struct GemvArgs {
  // prologue
  int pro;
  const void* x; int64_t x_ld;                    // PRO_PLAIN: element type [R][K]
  const float* xf; int64_t xf_ld;                 // PRO_LN: fp32 residual rows [R][K]
  const float* ln_w; const float* ln_b;
  int ln_folded;                                  // PRO_LN: ln_w == 1, ln_b == 0 (folded into W / bias at load time)
  const void* part_o; const float* part_ml; int splits; int H;  // PRO_COMBINE: [S][R][H][64] element type, [S][R][H][2]
  // weights
  const void* W; const float* bias; int N; int K; int R;
  // gemv8_kernel only (fp16, R <= 24; every other kernel ignores them — set them only where gemv8_will_run says so):
  int x_frag;                                     // PRO_PLAIN: x holds FRAGMENT-ORDER rows (below), K columns; x_ld ignored
  int y_frag;                                     // EPI_STORE / EPI_GELU: write y in fragment order (N % 64 == 0); y_ld ignored
  int w_ordered;                                  // set by the launcher (gemv.hip): weight wave-loads in memory order + a turn through LDS
  // LayerNorm applied AFTER the MFMAs (gemv8_kernel, fp16, folded LayerNorm, 9..24 rows; "LayerNorm behind the MFMAs" below):
  //   PRO_LN with xc != null: workgroup 0 also stores the row means it computed into xc[R] — the centres;
  //   EPI_RESID with xh != null also stores xh[frag_index(r, n, N)] = fp16(resid[r][n] - xc[r]), saturated to +-65504;
  //   PRO_LN_POST reads xh in fragment order (K columns) instead of the fp32 rows (xc unused: LayerNorm does not see a shift).
  void* xh; float* xc;
  // epilogue
  int epi;
  void* y; int64_t y_ld;                          // EPI_STORE / EPI_GELU (element type), EPI_F32 (float)
  float* resid; int64_t resid_ld;                 // EPI_RESID: resid[r][n] += y
  void* kcache; void* vcache; int64_t cache_bs; const int* d_pos; int D;  // EPI_QKV: row r appends at *d_pos - lag[r]
  const int* lag;                                 // EPI_QKV: per-row position lag (ragged prompts); may be null
  int* bump; int bump_by;                         // optional: *bump += bump_by once per launch (position counter)
  int* bump2;                                     // optional: *bump2 += 1 once per launch (the step tick of xattn.hip)
  int variant;                                    // 0 = shape heuristic; > 0 forces a kernel shape (tools/probe_decode); < 0 = heuristic without gemv8
  WH_PROBE_FIELD
};
hipError_t launch_gemv(const GemvArgs& a, int dtype, hipStream_t stream);
// Fragment order (fp16 activations that only travel from one launch of a decode step to the next: self-attention output ->
// attn.out, merged cross-attention output -> cross_attn.out, FC1 -> FC2).  A wave-load is 64 lanes x 16 bytes, and the memory
// pipeline of a CU takes ~58 cycles for one whose CONSECUTIVE lanes sit in different cache lines — the MFMA operand map read
// straight from row-major rows: lane 16 c + 8 half + i = row i, bytes 64 half + 16 c of a 128-byte block — against ~19.5 when
// lane l reads bytes [16 l, +16) of one contiguous KB (tools/ubench_ta.cpp, profiles/r06_fragment_order.txt: same 8 lines, same
// bytes).  With 2 - 3 row tiles a weight wave of a PRO_PLAIN launch issues 10 - 15 such x loads behind its 5 weight loads, so
// the PRODUCER writes the rows in the order the consumer's lanes want them: unit (row tile r / 8, K block k / 64) = 1 KB,
// lane 16 ((k & 31) >> 3) + 8 ((k >> 5) & 1) + r % 8 holds elements [k & ~7, +8).  Rows up to the next multiple of 8 must exist
// in the buffer (never written, read into output columns that are dropped).  FC2 of a 24-row step 11.0 -> 7.7 us, the D x D
// projections 4.9 -> 3.9; the same order for the WEIGHTS was measured too and is not used (D x D 4.9 -> 5.6 us: the 640-byte
// pieces of a 5-feature workgroup come off fewer HBM channels than five 128-byte lines 2.5 KB apart).
// element offset of x[r][k] in a fragment-order activation of K columns (K % 64 == 0)
static inline int64_t frag_index(int r, int k, int K) {
  return ((((int64_t)(r >> 3) * (K >> 6) + (k >> 6)) * 64 + 16 * ((k & 31) >> 3) + 8 * ((k >> 5) & 1) + (r & 7)) << 3) + (k & 7);
}
// LayerNorm behind the MFMAs.  With the affine part folded into W' / b' (WH_WEIGHTS_DEC_LN_FOLDED) LayerNorm is linear once the
// row statistics are known: for ANY per-row centre c, xc = x - c, m = mean_k(xc), v = mean_k(xc^2) - m^2, s_n = sum_k W'[n][k]:
//   y[r][n] = b'[n] + rsqrt(v_r + 1e-5) * (sum_k W'[n][k] xc[r][k] - m_r s_n)
// so an LN projection is a plain fragment-order projection on fp16(xc) whose statistics come out of the operands the weight waves
// hold anyway: no fp32 rows, no prologue waves, no barrier in front of the MFMAs.  The producer of x (the residual epilogue of
// attn.out / cross_attn.out / FC2) stores fp16(x - c) beside the fp32 residual.  Rounding x to fp16 loses the LayerNorm when
// |mean| >> std, hence the centre: c_r is the exact fp32 row mean at the layer's FIRST LayerNorm site (LN -> QKV, which keeps the
// LayerNorm prologue and has the mean in a register), stored by workgroup 0 of that launch into xc[r] and read by the producers
// behind it in stream order — one or two sub-layer updates away from the row they centre, which is small next to the row.  The
// centre is a function of the current step's data only: no state crosses steps, a captured step replays.  (A PRO_LN_POST launch
// could pass c + m on, but the mean of fp16-rounded values is off by the mean rounding error, ~2e-4 std / sqrt(K).)
// true when launch_gemv honours a fragment-order request for (R rows) x (N, K, pro), i.e. hands it to gemv8_kernel.  Asked about
// the canonical launch of that shape: fp16, packed rows (x_ld = xf_ld = K), folded LayerNorm (PRO_LN: the caller checks
// WH_WEIGHTS_DEC_LN_FOLDED itself), EPI_STORE, and for PRO_COMBINE splits = 2 and H = K / 64 heads.  A launch that differs
// from it (padded rows, EPI_F32 with N > 16384, other split counts) may still be refused: gemv.hip, gemv8_applies.
bool gemv8_will_run(int R, int N, int K, int pro);
// true where LayerNorm -> W [N][K] at R rows runs as PRO_LN_POST and that form is the faster one (gemv.hip; api.cpp::step_plan)
bool gemv8_ln_post_pays(int R, int N, int K);
// the kernel family launch_gemv picks for `a`, decided without launching: "gemv8", "rows48", "rows48_stream", "rows16_mf", "rt4",
// "rt8", or "" where it refuses (gemv.hip: pick_family; read by the kernel test library)
const char* gemv_family(const GemvArgs& a, int dtype);
// PRO_COMBINE's merge of the decode-attention partials as a launch of its own ([rows][H*64] in the element type)
hipError_t launch_merge_partials(const void* part_o, const float* part_ml, int splits, int R, int H, void* out,
                                 int64_t o_ld, int dtype, hipStream_t stream, int o_frag = 0);

// ---- logit_rules.h: what the greedy sampler and the beam update share -------------------------------------------------
// the rows of a step and the stock logit rules (SuppressBlank, SuppressTokens, ApplyTimestampRules) that apply to them
struct RuleArgs {
  const float* logits; int64_t logits_ld;   // row r at logits + r*logits_ld, V entries
  int R, V;
  int64_t token_stride;       // of the user's token buffer(s): [R][stride], current length *d_ntok
  const int* d_ntok;          // device: number of tokens currently in the longest row (== cached positions)
  const int* lag;             // ragged prompts: row r holds lag[r] fewer tokens, its sample_begin is lag[r] earlier; may be null
  int sample_begin, eot, timestamp_begin, no_timestamps, max_initial_ts, suppress_blank, blank_token;
  const uint8_t* suppress_mask;
  float* sum_logprobs;        // [R] in/out
};

// ---- sampling.hip --------------------------------------------------------------------------
struct SampleArgs {
  RuleArgs rules;
  int64_t* tokens;            // [R][rules.token_stride]
  int64_t* step_tokens;       // [R] next-step input tokens (may be null)
  int* d_alive_step;          // device: set to ntok by every row whose sampled token is not EOT
  float* partials;            // scratch: greedy_sample_scratch_bytes(R, V)
  float inv_temperature;      // 0: arg-max; > 0: sample from softmax(logits / T) (Gumbel-max, counter-based noise)
  uint32_t seed_lo, seed_hi;
  // optional: the final kernel also writes the next step's decoder input x_next[r][:] = tok_emb[token] + pos_emb[index of
  // the token] (model.py:236-240), so the step that follows needs no embedding launch; skipped when x_next is null
  float* x_next; const void* tok_emb; const float* pos_emb; int D, emb_f16, n_pos;
  // per-row state kept by the final kernel, {last sampled token is a timestamp, the one before it is, value of the last
  // sampled timestamp + 1 (0 = none), the row's trie node (PhraseArgs)}, zeroed before the first sample of a sequence: the
  // partial kernel's timestamp window.  Required with timestamp rules (timestamp_begin >= 0) or a phrase list, else may be null.
  int* row_state;
};
// Phrase biasing inside the sampler (include/whisper_hip.h, wh_task_set_phrases): a token trie in CSR form, node 0 the root.
// Row r's trie node lives in row_state[4 r + 3] (the slot the timestamp rules leave unused; row_state must then be given);
// `span` holds the child_begin pair of that node, {0, 0} at the root, whose edges `root_child` already answers — kept per
// row by the final kernel so that the partial kernel asks for it together with the logits instead of behind the state.
// Both are zeroed before the first sample of a sequence.
struct PhraseArgs {
  const int* child_begin;     // [n_nodes + 1]
  const int* child_token;     // [n_edges], ascending within a node
  const int* child_node;      // [n_edges]
  const int* root_child;      // [V]: the root's child reached by token v, or -1
  int* span;                  // [R][2]
  int n_nodes, n_edges;
  float boost;
};
// Repetition control inside the sampler (include/whisper_hip.h, wh_task_set_repetition).  It carries no state: both edits
// follow from the row's sampled tokens H = tokens[r][sample_begin - lag[r] .. length), which the partial kernel reads.
//   penalty != 1: every token of H below eot, as a SET, has its raw logit divided by `penalty` if positive, multiplied if
//                 negative (0 and -inf stay);
//   ngram >= 1:   every token below eot that followed an earlier occurrence of the row's last ngram - 1 tokens is -inf.
// Order: penalty -> phrase boost -> ban -> SuppressBlank / SuppressTokens / ApplyTimestampRules.
constexpr int REP_MAX_NGRAM = 16;
struct RepArgs {
  int ngram;                  // 0: off
  float penalty;              // 1: off; finite and > 0
};
// Per-token statistics of the sampler (include/whisper_hip.h, wh_task_set_token_stats): what the step knows about the
// distribution its token was chosen from — the edited and filtered row, the text range dropped where the timestamp mass rule
// fires.  Every buffer is indexed by the COLUMN of the token buffer that receives the step's token (row r, column = the row's
// own length, RowPos::ntok), so ragged prompts need nothing special; each may be null on its own.  A launch writes that one
// column and nothing else.
//   token_logprob [R][stride]         the fp32 value the final kernel adds to sum_logprobs
//   entropy       [R][stride]         -sum p log p in nats over the allowed entries
//   top_token / top_logprob [R][stride][top_k]   the top_k largest allowed entries, value descending, lower id first among
//                 equal values; log-probabilities against the normaliser of token_logprob; padded with (-1, -inf).  They rank
//                 the UNSCALED edited logits also at temperature > 0, like the accumulated log-probability.
// A row already at eot writes 0, 0, (-1, -inf)...; a row with every logit filtered NaN, NaN, (-1, -inf)....
constexpr int TOKEN_STATS_MAX_TOP = 8;
struct TokenStatArgs {
  float* token_logprob; float* entropy;
  int* top_token; float* top_logprob;
  int top_k;                  // 0 .. TOKEN_STATS_MAX_TOP; > 0 needs both top buffers and `scratch`
  int64_t stride;             // columns per row of the buffers above, >= rules.token_stride
  void* scratch;              // the chunks' best entries: greedy_sample_top_scratch_bytes(R, V); not read when top_k == 0
};
size_t greedy_sample_scratch_bytes(int R, int V);
// what a launch with top_k > 0 needs on top of it, in TokenStatArgs::scratch (a plain decode's scratch stays what it is)
size_t greedy_sample_top_scratch_bytes(int R, int V);
// ph == nullptr: the unbiased instantiations, which never look at the phrase arguments; rep == nullptr (or {0, 1}): the
// instantiations without repetition control, which never look at the row's history for it; ts == nullptr: the instantiations
// without statistics, which never look at the statistics arguments
hipError_t launch_greedy_sample(const SampleArgs& a, hipStream_t stream, const PhraseArgs* ph = nullptr,
                                const RepArgs* rep = nullptr, const TokenStatArgs* ts = nullptr);
// root[v] = child of the root reached by token v, else -1 (tokens outside [0, V) are ignored)
hipError_t launch_phrase_root_table(const int* child_begin, const int* child_token, const int* child_node, int n_edges,
                                    int V, int* root, hipStream_t stream);
// span[r] = child_begin pair of the node in row_state[4 r + 3], {0, 0} for the root or a node outside [0, n_nodes)
hipError_t launch_phrase_span(const int* row_state, const int* child_begin, int n_nodes, int R, int* span, hipStream_t stream);
hipError_t launch_no_speech(const float* logits_row0, int64_t row_stride, int R, int V, int no_speech,
                            float* out, hipStream_t stream);
// dst[r] = src[r*stride]
hipError_t launch_gather_tokens(const int64_t* src, int64_t stride, int R, int64_t* dst, hipStream_t stream);

// ---- beam.hip -------------------------------------------------------------------------------
constexpr int BEAM_KMAX = 9;   // candidates per row = beam + 1, beam <= 8
struct BeamArgs {
  RuleArgs rules;                           // R rows = segments x G beams; token_stride of tokens_in / tokens_out
  int G, K;                                 // K = G + 1
  const int64_t* tokens_in; int64_t* tokens_out;   // [R][stride] each; rows hold *d_ntok tokens
  float* part_stat; float* part_val; int* part_idx;   // scratch (beam_scratch_carve)
  float* cand_lp; int* cand_tok;            // [R][BEAM_KMAX] top-K log-probabilities / tokens of every row
  int64_t* fin_tok; int* fin_len; float* fin_score; int* fin_count;   // [B][max_candidates][stride], [B][mc], [B][mc], [B]
  int max_candidates;
  int* src;                                 // [R] out: row whose KV cache the new beam continues
  // optional (both or neither): lcp [B][8][8] in/out = number of leading cache positions at which two rows of a segment
  // hold identical K/V (initialise every entry to INT_MAX-like: "everything so far"); copy_from [R] out = first position
  // row r has to take from src[r] (below it the bytes are already the same)
  int* lcp; int* copy_from;
  int64_t* step_tokens;                     // [R] out: next step's input tokens
  const int* done_prev; int* done_next;     // [B] completion flags written by the previous / this update
  int* d_applied;                           // number of updates applied (not frozen)
  int first;                                // 1: first update — all beams of a segment hold the same prefix
};
size_t beam_scratch_bytes(int R, int V);
void beam_scratch_carve(BeamArgs& a, void* base, int R, int V);
// filters + log_softmax + top-(G+1) of every row, then the candidate bookkeeping of every segment (3 launches)
hipError_t launch_beam_step(const BeamArgs& a, int B, hipStream_t stream);

// ---- timing.hip ----------------------------------------------------------------------------
hipError_t launch_median_filter(const float* x, float* out, int64_t rows, int n, int width,
                                hipStream_t stream);
// dtw of one cost matrix [N][M] -> trace [(N + 1)][(M + 1)].  N <= DTW_OPEN_MAX_ROWS (below), as for every dtw launcher here:
// more rows are refused with hipErrorInvalidValue (n_text_ctx is 448)
hipError_t launch_dtw(const float* x, int N, int M, int8_t* trace, hipStream_t stream);
// batched find_alignment post-processing: clip b has ntok[b] token rows and nfr[b] frames (device arrays) inside slabs
// qk [clips][H][Tmax][Tk]; cost [clips][Nmax][Fmax] = -mean over heads of rows [row_begin, ntok[b] - row_tail);
// scratch: 2 * clips * H * Tmax * Fmax floats
hipError_t launch_align_batch(const float* qk, const int* d_ntok, const int* d_nfr, int clips, int H, int Tmax, int Tk,
                              int Fmax, int width, int row_begin, int row_tail, float qk_scale, float* cost, int Nmax,
                              float* scratch, hipStream_t stream);
// dtw of every clip's cost matrix; trace of clip b dense [(N_b + 1)][(F_b + 1)] at trace + b * trace_bs.
// Nmax <= DTW_OPEN_MAX_ROWS (below)
hipError_t launch_dtw_batch(const float* cost, const int* d_ntok, const int* d_nfr, int clips, int Tmax, int Fmax,
                            int row_begin, int row_tail, int Nmax, int8_t* trace, int64_t trace_bs, hipStream_t stream);
// open-end dtw: clip b's cost matrix [d_rows[b]][d_cols[b]] (row stride Fmax, slab of Nmax rows); trace as launch_dtw_batch
// (trace_bs >= (Nmax + 1) * (Fmax + 1)); lastcol [clips][Nmax] = accumulated cost of the last column; end [clips] = the row the
// path leaves the window at: d_rows[b] where d_closed[b] != 0, else the smallest i with lastcol[i-1] <= m + end_slack * |m|,
// m the column's minimum; 0 for an empty clip.  Pass `end` to launch_dtw_backtrace_batch as its row counts.
// Nmax <= DTW_OPEN_MAX_ROWS: the wavefront keeps three diagonals of Nmax + 1 floats in 64 KB of LDS.  The same limit holds
// for launch_dtw and launch_dtw_batch (the same wavefront, the same LDS, no raise_dynamic_lds).
constexpr int DTW_OPEN_MAX_ROWS = 5460;
hipError_t launch_dtw_open_batch(const float* cost, const int* d_rows, const int* d_cols, const int* d_closed, int clips,
                                 int Nmax, int Fmax, float end_slack, int8_t* trace, int64_t trace_bs, float* lastcol,
                                 int* end, hipStream_t stream);
// back-trace of every clip's trace (dense [(rows_b + 1)][(cols_b + 1)] at trace + b * trace_bs; d_rows / d_cols device
// arrays): jumps [clips][jump_stride] = frame at which each text index is first reached; optional right-aligned path
// [clips][2][path_stride] + path_len [clips]
hipError_t launch_dtw_backtrace_batch(const int8_t* trace, int64_t trace_bs, const int* d_rows, const int* d_cols, int clips,
                                      int max_rows, int max_cols, int* jumps, int64_t jump_stride, int* path,
                                      int64_t path_stride, int* path_len, hipStream_t stream);
// qk [H][T][Tk] -> softmax over first F frames, z-norm over tokens, median(width), -mean over heads of rows
// [row_begin,row_end) -> out [rows][F]; scratch: 2*H*T*F floats + 2 ints
hipError_t launch_align_matrix(const float* qk, int H, int T, int Tk, int F, int width, int row_begin,
                               int row_end, float qk_scale, float* out, float* scratch, hipStream_t stream);

// ---- chunk.hip -----------------------------------------------------------------------------
// L[f] = log10 of the mean mel power of frame f (definitions at the top of chunk.hip); mel fp32 [n_mels][frame_stride]
hipError_t launch_frame_level(const float* mel, int n_mels, int64_t frame_stride, int64_t content, float* level,
                              hipStream_t stream);
// cost[f] = max of level over [f - guard, f + guard] (guard <= 64), then the cut walk by one workgroup: cuts [max_cuts],
// n_cuts [1] (device)
hipError_t launch_speech_cuts(const float* level, int content, int min_frames, int max_frames, int guard, float* cost,
                              int* cuts, int* n_cuts, int max_cuts, hipStream_t stream);

// ---- resample.hip --------------------------------------------------------------------------
// interleaved PCM [n_frames][channels] (format: WH_PCM_* of include/whisper_hip.h; bits: full scale 2^(bits-1) of the signed
// integer formats) -> mono fp32 [n_out] on the 16-bit grid: down-mix, polyphase resampling with taps [2 * half + 1] (float64,
// device), quantisation — all in float64 (definitions at the top of resample.hip)
hipError_t launch_resample(const void* pcm, int format, int bits, int channels, int64_t n_frames, const double* taps, int up,
                           int down, int half, float* out, int64_t n_out, hipStream_t stream);
// outputs one workgroup takes so that the input span they reach fits its LDS; 0: not even one fits (down / up too large)
int resample_outputs_per_wg(int up, int down, int half);

// ---- flac.hip ------------------------------------------------------------------------------
// FLAC decoding, one lane per frame (stages and definitions at the top of flac.hip).  The scratch of one call, carved from one
// allocation; hdr .. rc (record_bytes from the base) is what the host downloads for the chain.
struct FlacScratch {
  int* hdr;             // [0] candidates listed (<= max_cand), [1] candidates found
  uint8_t* tail;        // the file's last min(size, 128) bytes
  int64_t* start;       // [max_cand] candidate offsets, ascending
  int64_t* end;         // [max_cand] offset behind the frame's CRC-16 (the start offset when the body did not parse)
  int* bs;              // [max_cand] block size by the header
  int* rc;              // [max_cand] decode status (flac_core.h: FLAC_OK, FLAC_E_*)
  size_t record_bytes;
  int64_t* prov;        // [max_cand] provisional position in the staging buffer, samples per channel
  int* tile_count;
  int* tile_base;
  int64_t* mv_from;     // compaction list, uploaded after the chain
  int64_t* mv_to;
  int* mv_len;
  int32_t* temp;        // [staging_frames][channels] second buffer of the compaction
  size_t total_bytes;
};
FlacScratch flac_scratch(void* base, size_t size, int channels, int64_t staging_frames, int max_cand);
// candidates of file[first, size) in offset order with their provisional positions (first < size)
hipError_t launch_flac_scan(const uint8_t* file, size_t size, size_t first, int ch, int bps, int max_block, const FlacScratch& s,
                            int max_cand, hipStream_t stream);
// every listed candidate decoded into pcm [staging_frames][ch] at its provisional position; end / rc / tail filled
hipError_t launch_flac_decode(const uint8_t* file, size_t size, int ch, int bps, const FlacScratch& s, int max_cand, int32_t* pcm,
                              int64_t staging_frames, hipStream_t stream);
// dst[mv_to[k] ..] = src[mv_from[k] ..], mv_len[k] samples, k < n_moves
hipError_t launch_flac_move(const int32_t* src, int32_t* dst, const FlacScratch& s, int n_moves, hipStream_t stream);

// ---- score.hip -----------------------------------------------------------------------------
// Teacher-forced scoring without the logits.  xn [M][K] (element type, row stride ldx), W = tok_emb [V][K], target [M]
// (device int32), 1 <= v_end <= V.  Per row m, over the columns v < v_end of logit = xn · Wᵀ:
//   logprob[m] = logit[target[m]] - log sum exp(logit)      (-inf when target[m] >= v_end)
//   top_logprob[m] / top_token[m] = the largest logit minus the same log-sum / the lowest id that attains it
//   target[m] < 0 (padded slot): logprob = 0, top_logprob = 0, top_token = -1
// top_logprob / top_token may be null.  scratch (16-byte aligned): score_scratch_bytes(M, V) bytes, one 16-byte partial
// per (row, SCORE_BN-column slice); two launches, no atomics, bit-identical from run to run.  K % 64 == 0 (fp16) / % 32 (fp32).
constexpr int SCORE_BN = 128;    // vocabulary columns per slice (one workgroup per 128 rows x one slice)
constexpr int SCORE_WGN = 2;     // waves side by side across a slice
size_t score_scratch_bytes(int64_t M, int V);
hipError_t launch_score(const void* xn, int64_t ldx, const void* W, int64_t ldw, const int* target, int M, int K, int V,
                        int v_end, float* logprob, float* top_logprob, int* top_token, void* scratch,
                        size_t scratch_bytes, int dtype, hipStream_t stream);
// target[r][i] = tokens[r * token_stride + first + i + 1] for i < n_out, or -1 where first + i + 1 >= n_tok[r] (all device)
hipError_t launch_score_targets(const int64_t* tokens, int64_t token_stride, const int* n_tok, int R, int n_out, int first,
                                int* target, hipStream_t stream);

}  // namespace whk
