# A/B helper for bit-identical variants of the library: one run prints a line of SHA-1 digests per leg — run it on two builds (or
# under two settings of a developer switch of libwhisper_hip_dev.so) and diff the output.  A leg that differs between two runs
# of the SAME build is not deterministic and says nothing.
#   python tools/step_hash.py [model]                (default large-v3; wide-v3 = the same widths at 2 layers, seconds)
#   WHISPER_AMD_LIB=whisper_amd/libwhisper_hip_dev.so WH_NO_TAIL_MERGE=1 python tools/step_hash.py wide-v3
# Legs:
#   greedy  — the device-side greedy loop, 40 tokens, at several row counts: tokens and summed log-probabilities; then the
#             loop's other forms: temperature sampling, a phrase list with repetition control, without timestamp rules,
#             ragged prompts
#   logits  — raw float32 logits of a host-driven prefill and of the 3 `step` calls behind it, over the task forms the step has
#             (fused / two-launch cross attention, fused self attention, in-launch merge, merge launch, ragged rows, fp32), the
#             few-row / GEMM / flash prefill paths and a capture-Q task
#   beam    — the device-side beam search, 8 steps: tokens, summed log-probabilities, finished lists and their scores; once
#             more with ragged prompts
#   score   — one teacher-forced scoring pass
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from whisper_amd import hip
from whisper_amd.phrases import PhraseList
from whisper_amd.synthetic import dims_for, synthetic_state_dict
from whisper_amd.tokenizer import get_tokenizer
dev = torch.device("cuda:0")
name = sys.argv[1] if len(sys.argv) > 1 else "large-v3"
N = 40
dims = dims_for(name)
sd = synthetic_state_dict(dims, seed=0, device=dev)
model = hip.HipModel(dims, hip.WH_F16, hip.pack_weights(sd, dims, hip.WH_F16, dev))
model32 = hip.HipModel(dims, hip.WH_F32, hip.pack_weights(sd, dims, hip.WH_F32, dev)); del sd
# STEP_HASH_TASK_FLAGS=64 (WH_TASK_LN_PROLOGUE): OR-ed into every task — the two settings agree to rounding, not bit for bit: compare
# the `tokens` digests of the greedy leg
model.debug_task_flags = model32.debug_task_flags = int(os.environ.get("STEP_HASH_TASK_FLAGS", "0"))
tok = get_tokenizer(True, num_languages=dims.n_vocab - 51765 - 1, language="en", task="transcribe")
init = list(tok.sot_sequence); T0 = len(init)
suppress = sorted(set(list(tok.non_speech_tokens) + [tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm, tok.no_speech, tok.eot]))
mask = torch.zeros(dims.n_vocab, dtype=torch.uint8); mask[suppress] = 1; mask = mask.to(dev)


def rules(max_steps, sample_begin=T0, timestamp_begin=tok.timestamp_begin, **kw):
    return hip.GreedyParams(sample_begin=sample_begin, max_steps=max_steps, n_ctx=dims.n_text_ctx, eot=tok.eot,
                            timestamp_begin=timestamp_begin, no_timestamps=tok.no_timestamps, max_initial_timestamp_index=50,
                            suppress_blank=1, blank_token=tok.encode(" ")[0], suppress_mask=mask.data_ptr(), **kw)


def sha(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:12]


g = torch.Generator(device=dev).manual_seed(4)
feats = (torch.randn(24, dims.n_audio_ctx, dims.n_audio_state, generator=g, device=dev)
         + 3.0 * torch.randn(24, 1, dims.n_audio_state, generator=g, device=dev)).half()
sot_index = tok.sot_sequence.index(tok.sot)

# ---- greedy loop ----
params = rules(N)
for B, two in ((24, False), (20, False), (16, False), (9, False), (8, True), (8, False), (3, True), (1, True)):
    task = hip.HipTask(model, B, 1, max(T0, 8), two_launch_cross=two)
    tokens = torch.zeros(B, T0 + N + 1, dtype=torch.int64, device=dev)
    tokens[:, :T0] = torch.tensor(init, device=dev)
    task.reset(); task.set_audio(feats[:B].contiguous())
    n, slp, nsp = task.greedy(tokens, params, sot_index, tok.no_speech)
    torch.cuda.synchronize()
    print(f"greedy {B:2d} rows{' two-launch cross' if two else '':17s} tokens {sha(tokens)}  sum_logprobs {sha(slp.float())}", flush=True)
    task.destroy()


# the loop's other forms.  prompt: the tokens every row starts with; with `lag`, row r starts with prompt[lag[r]:] (set_lag)
def greedy_leg(label, B, params, prompt=init, lag=None, phrases=None, repetition=None):
    P = len(prompt)
    task = hip.HipTask(model, B, 1, max(P, 8))
    tokens = torch.zeros(B, P + N + 1, dtype=torch.int64, device=dev)
    for r in range(B):
        own = prompt[lag[r]:] if lag else prompt
        tokens[r, :len(own)] = torch.tensor(own, device=dev)
    task.reset(); task.set_audio(feats[:B].contiguous())
    if lag:
        task.set_lag(lag)
    if phrases is not None:
        task.set_phrases(phrases.device_arrays(dev), phrases.boost)
    if repetition:
        task.set_repetition(*repetition)
    n, slp, _ = task.greedy(tokens, params, sot_index, -1 if lag else tok.no_speech)
    torch.cuda.synchronize()
    print(f"greedy {B:2d} rows {label:34s} tokens {sha(tokens)}  sum_logprobs {sha(slp.float())}", flush=True)
    task.destroy()


for B in (3, 24):
    greedy_leg("temperature 0.7", B, rules(N, temperature=0.7, seed=0x123456789abcdef))
rng = np.random.default_rng(0)
text_ok = np.array([t for t in range(300, tok.eot) if t not in set(suppress) | {tok.encode(" ")[0]}])
plist = PhraseList([rng.choice(text_ok, int(rng.integers(1, 7))).tolist() for _ in range(1000)], boost=1.0)
greedy_leg("phrase list + ngram 3 + penalty 1.3", 8, params, phrases=plist, repetition=(3, 1.3))
greedy_leg("without timestamps", 8, rules(N, timestamp_begin=-1))
long_prompt = [tok.sot_prev, 1000, 1001] + init
ragged = [0, 1, 2, 3, 0, 1, 2, 3]
greedy_leg("ragged prompts", 8, rules(N, sample_begin=len(long_prompt)), prompt=long_prompt, lag=ragged)


# ---- host-driven prefill + 3 steps: raw logits ----
def logits_leg(label, mdl, B, P, G=1, lag=None, **kw):
    R = B * G
    task = hip.HipTask(mdl, B, G, max(P, 8), **kw)
    gt = torch.Generator(device=dev).manual_seed(100 + R + P)
    toks = torch.randint(0, dims.n_vocab, (R, P + 3), generator=gt, device=dev)
    task.set_audio(feats[:B].to(mdl.torch_dtype).contiguous())
    if lag is not None:
        task.set_lag(lag)
    pre = task.prefill(toks[:, :P].contiguous())
    steps = [task.step(toks[:, P + i]) for i in range(3)]
    torch.cuda.synchronize()
    form = f"fused cross {int(task.fused_cross_attention)} self {int(task.fused_self_attention)}"
    print(f"logits {label:34s} ({form}, timeouts {task.handoff_timeouts()}) prefill {sha(pre)}  steps {sha(*steps)}", flush=True)
    task.destroy()


logits_leg("fp16  1 row", model, 1, 4)
logits_leg("fp16  8 rows", model, 8, 4)
logits_leg("fp16  8 rows two-launch cross", model, 8, 4, two_launch_cross=True)
logits_leg("fp16  8 rows fused self", model, 8, 4, fused_self=True)
for B in (12, 16, 20, 24):
    logits_leg(f"fp16 {B:2d} rows", model, B, 4)
logits_leg("fp32  3 rows", model32, 3, 4)
logits_leg("fp32 12 rows", model32, 12, 4)
logits_leg("fp16  8 rows ragged", model, 8, 4, lag=[0, 1, 2, 3, 0, 1, 2, 3])
logits_leg("fp16  4 rows x 40 tokens (GEMM)", model, 4, 40)
logits_leg("fp16  2 rows x 40 tokens capture-Q", model, 2, 40, capture_q=True)
logits_leg("fp16  3 rows x 40 tokens capture-Q", model, 3, 40, capture_q=True)      # 120 rows x tokens: the flash cross attention
logits_leg("fp16  2 x 5 rows (beam groups)", model, 2, 4, G=5)

# ---- beam search ----
for B, G, lag in ((2, 5, None), (8, 5, None), (2, 5, [0, 2])):      # lag: per segment, the beams of a segment share it
    R, steps = B * G, 8
    prompt = long_prompt if lag else init
    P = len(prompt)
    task = hip.HipTask(model, B, G, max(P, 8))
    tokens = torch.zeros(2, R, P + steps + 1, dtype=torch.int64, device=dev)
    for r in range(R):
        own = prompt[lag[r // G]:] if lag else prompt
        tokens[0, r, :len(own)] = torch.tensor(own, device=dev)
    task.set_audio(feats[:B].contiguous())
    if lag:
        task.set_lag([v for v in lag for _ in range(G)])
    bp = hip.BeamParams(rules=rules(steps, sample_begin=P), beam_size=G, max_candidates=G)
    n, slp, nsp, (fin_tok, fin_len, fin_score, fin_count) = task.beam(tokens, bp, sot_index, -1 if lag else tok.no_speech)
    torch.cuda.synchronize()
    print(f"beam {B} x {G}{' ragged' if lag else ''}: n_tokens {n} tokens {sha(tokens[0])}  sum_logprobs {sha(slp)}  "
          f"no_speech {sha(nsp) if nsp is not None else '-'}  "
          f"finished {sha(fin_tok, fin_len, fin_count)}  scores {sha(fin_score)}", flush=True)
    task.destroy()

# ---- scoring ----
task = hip.HipTask(model, 4, 1, 12)
gt = torch.Generator(device=dev).manual_seed(77)
toks = torch.randint(0, dims.n_vocab, (4, 12), generator=gt, device=dev)
task.set_audio(feats[:4].contiguous())
lp, top_lp, top_tok = task.score(toks, [12, 9, 12, 5], 3)
torch.cuda.synchronize()
print(f"score 4 rows x 12 tokens: logprob {sha(lp)}  top_logprob {sha(top_lp)}  top_token {sha(top_tok)}", flush=True)
task.destroy()
