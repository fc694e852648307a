"""Per-token statistics on the host: the float64 oracle against a brute-force restatement, the generator of the kernel test,
keyword validation, the result type, how transcribe cuts the lists with the tokens, the host-loop route against the oracle on
a stub Inference, the C ABI declaration, and the way the keywords travel to a sharded worker.  No GPU."""
import dataclasses
import importlib
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repetition_oracle as ro  # noqa: E402
import token_stats_cases as tc  # noqa: E402
import token_stats_oracle as tso  # noqa: E402

import whisper_amd  # noqa: E402
from whisper_amd import decoding, hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_model():
    dims = SimpleNamespace(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=2, n_vocab=51865,
                           n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=2)
    return SimpleNamespace(dims=dims, is_multilingual=True, device=torch.device("cpu"), num_languages=99)


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def _brute(x, k):
    """probabilities by plain exponentials (tiny rows: no overflow), entropy and top-k by an explicit selection"""
    allowed = [i for i in range(len(x)) if x[i] != -math.inf]
    if not allowed:
        return None
    Z = sum(math.exp(x[i]) for i in allowed)
    p = {i: math.exp(x[i]) / Z for i in allowed}
    H = -sum(p[i] * math.log(p[i]) for i in allowed)
    left, top = list(allowed), []
    while left and len(top) < k:
        best = left[0]
        for i in left[1:]:
            if x[i] > x[best]:                       # strictly: among equal values the earlier (lower) id stays
                best = i
        top.append(best)
        left.remove(best)
    return p, H, top


def test_oracle_against_brute_force_on_tiny_rows():
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(1, 9))
        x = (rng.integers(-64, 65, n) / 16.0).astype(np.float64)         # a coarse grid: ties are common
        x[rng.random(n) < 0.3] = -np.inf
        k = int(rng.integers(1, 9))
        want = _brute(x.tolist(), k)
        if want is None:
            lp, H, tt, tv = tso.row_stats(x, 0, k)
            assert math.isnan(lp) and math.isnan(H) and tt == [-1] * k and tv == [-math.inf] * k
            continue
        p, H, top = want
        chosen = top[0]
        lp, H2, tt, tv = tso.row_stats(x, chosen, k)
        assert abs(lp - math.log(p[chosen])) < 1e-12 and abs(H - H2) < 1e-12
        assert tt == top + [-1] * (k - len(top))
        assert all(abs(v - math.log(p[t])) < 1e-12 for t, v in zip(top, tv)) and tv[len(top):] == [-math.inf] * (k - len(top))
        assert 0.0 <= H2 + 1e-12 and H2 <= math.log(len(p)) + 1e-12
    assert tso.row_stats(np.array([1.0, 2.0]), 1, 3, ended=True) == (0.0, 0.0, [-1] * 3, [-math.inf] * 3)
    # equal values: the lower id first
    assert tso.top_k(np.array([0.0, 2.0, 2.0, -np.inf, 2.0]), 4)[0] == [1, 2, 4, 0]


def test_oracle_describes_the_edited_row():
    """penalty -> boost -> ban -> rules -> mass rule: a banned token is no alternative, and where the timestamps' mass wins
    the list holds timestamps only"""
    r = tc.rules(1000, with_ts=True)
    TB = r.timestamp_begin
    x = np.full(1000, -20.0)
    x[[300, 301, 302]] = [5.0, 4.0, 3.0]
    x[TB + 10: TB + 14] = 4.5                          # four timestamps at 4.5: their mass exceeds the best text token's
    tok, lp, H, tt, tv, xe = tso.step_stats(x, [TB + 3, 300, 301, 300], r, 5, n=2)
    assert tok == TB + 10 and tt[:4] == [TB + 10, TB + 11, TB + 12, TB + 13] and all(t >= TB for t in tt)
    x[TB + 10: TB + 14] = -20.0                        # now the text range stays; 301 followed 300 before: banned
    tok, lp, H, tt, tv, xe = tso.step_stats(x, [TB + 3, 300, 301, 300], r, 5, n=2)
    assert tok == 300 and 301 not in tt and tt[1] == 302 and xe[301] == -np.inf
    assert abs(sum(math.exp(v) for v in tso.log_softmax(xe) if v != -math.inf) - 1.0) < 1e-12


def test_the_generator_clears_the_mass_rule_margin_in_every_row():
    """tc.build asserts the margin of every row it generates: building every case of the kernel test here shows that none
    of them trips it (and that the rule fires in some rows and not in others)"""
    fired = set()
    for V, R, ts, L, k in tc.grid_cases():
        if k != 5 and V == 51866:                    # the rows do not depend on top_k; the large vocabulary once
            continue
        fired |= {w["fired"] for w in tc.build(V, R, ts, L, k)["want"]}
    for kw in tc.planted_cases().values():
        case = tc.build(**kw)
        assert len(case["want"]) == kw["R"]
    assert {True, False} <= fired
    assert tc.MASS_BOUND == (26 + 1) * 6 * 2.0 ** -24 + 2 * 2.0 ** -20 + 3 * 2.0 ** -16


# ---- keywords and the result type -------------------------------------------------------------------------------------------
def test_validation():
    for bad in (-1, 9, 2.0, "2", True):
        with pytest.raises(ValueError):
            decoding.check_token_stats(False, bad)
    with pytest.raises(ValueError):
        decoding.check_token_stats("yes", 0)
    assert decoding.check_token_stats() == (False, 0)
    assert decoding.check_token_stats(True, 0) == (True, 0)
    assert decoding.check_token_stats(False, 3) == (True, 3)              # top_logprobs implies token_logprobs
    assert decoding.check_token_stats(None, np.int64(8)) == (True, 8)
    model = _fake_model()
    task = decoding.DecodingTask(model, decoding.DecodingOptions(language="en"), top_logprobs=5)
    assert task.token_logprobs and task.top_logprobs == 5 and task._fused_greedy_ok(None)
    assert not decoding.DecodingTask(model, decoding.DecodingOptions(language="en")).token_logprobs
    for kw in (dict(token_logprobs=True), dict(top_logprobs=1)):
        with pytest.raises(ValueError, match="beam search"):
            decoding.DecodingTask(model, decoding.DecodingOptions(language="en", beam_size=2), **kw)
    decoding.DecodingTask(model, decoding.DecodingOptions(language="en", temperature=0.5, best_of=3), top_logprobs=2)
    tr = importlib.import_module("whisper_amd.transcribe")
    for bad in (dict(top_logprobs=9), dict(top_logprobs=-1), dict(token_logprobs=1.5)):
        with pytest.raises(ValueError):
            decoding.DecodingTask(model, decoding.DecodingOptions(language="en"), **bad)
        with pytest.raises(ValueError):
            decoding.decode_many(model, [], **bad)
        with pytest.raises(ValueError):
            tr.transcribe_batch(model, [np.zeros(16000, np.float32)], **bad)
        with pytest.raises(ValueError):
            tr.transcribe_chunked(model, np.zeros(16000, np.float32), **bad)
        with pytest.raises(ValueError):
            importlib.import_module("whisper_amd.launcher").transcribe_sharded(model, [np.zeros(16000, np.float32)], **bad)
    with pytest.raises(ValueError):
        hip.HipTask.set_token_stats(SimpleNamespace(), 9)


def test_detailed_result_leaves_the_reference_fields_alone():
    base = [(f.name, f.type, f.default, f.default_factory) for f in dataclasses.fields(decoding.DecodingResult)]
    assert [n for n, *_ in base] == ["audio_features", "language", "language_probs", "tokens", "text", "avg_logprob",
                                     "no_speech_prob", "temperature", "compression_ratio"]
    det = dataclasses.fields(decoding.DetailedDecodingResult)
    assert [(f.name, f.type, f.default, f.default_factory) for f in det[: len(base)]] == base
    assert [f.name for f in det[len(base):]] == ["token_logprobs", "token_entropies", "top_tokens", "top_logprobs"]
    assert issubclass(decoding.DetailedDecodingResult, decoding.DecodingResult)
    assert whisper_amd.DetailedDecodingResult is decoding.DetailedDecodingResult
    res = decoding.DetailedDecodingResult(audio_features=torch.zeros(1), language="en", token_logprobs=[-0.5])
    with pytest.raises(dataclasses.FrozenInstanceError):
        res.token_logprobs = []


# ---- transcribe: the lists are cut where the tokens are cut -----------------------------------------------------------------
def _one_window(worker, result):
    walk = worker._walk(None, torch.zeros(80, 6000))               # 30 s of content + the 30 s of padding
    window = next(walk)
    assert window.shape == (80, 3000)
    try:
        walk.send(result)
    except StopIteration as stop:
        return stop.value
    raise AssertionError("the window did not end the file")


@pytest.mark.parametrize("top", [0, 3])
def test_transcribe_cuts_the_lists_with_the_tokens(top):
    tr = importlib.import_module("whisper_amd.transcribe")
    model = _fake_model()
    tk = whisper_amd.tokenizer.get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    TB = tk.timestamp_begin
    hello, world, again = tk.encode(" hello"), tk.encode(" world"), tk.encode(" again")
    ids = [TB] + hello + [TB + 50, TB + 50] + world + [TB + 100, TB + 100] + again + [TB + 150]
    n = len(ids)
    lps = [-(j + 1) / 16 for j in range(n + 1)]                      # the last entry: the closing <|endoftext|>'s
    ents = [(j + 1) / 8 for j in range(n + 1)]
    tts = [[j, j + 1, -1][:top] for j in range(n + 1)]
    tvs = [[-0.25, -2.0, -math.inf][:top] for j in range(n + 1)]
    opts = dict(language="en", fp16=False, token_logprobs=True, top_logprobs=top)
    worker = tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None, opts)
    assert worker.repetition == dict(token_logprobs=True, top_logprobs=top)
    assert "token_logprobs" not in worker.decode_options and "top_logprobs" not in worker.decode_options
    result = decoding.DetailedDecodingResult(
        audio_features=torch.zeros(1), language="en", tokens=ids, text="hello world again", avg_logprob=-0.1,
        no_speech_prob=0.0, temperature=0.0, compression_ratio=1.0, token_logprobs=lps, token_entropies=ents,
        top_tokens=tts if top else [], top_logprobs=tvs if top else [])
    out = _one_window(worker, result)
    segs = out["segments"]
    assert [s["tokens"] for s in segs] == [[TB] + hello + [TB + 50], [TB + 50] + world + [TB + 100],
                                           [TB + 100] + again + [TB + 150]]
    at = 0
    for s in segs:
        m = len(s["tokens"])
        assert s["token_logprobs"] == lps[at: at + m] and s["token_entropies"] == ents[at: at + m]
        if top:
            assert s["top_logprobs"] == [[[t, v] for t, v in zip(tts[j], tvs[j])] for j in range(at, at + m)]
            assert all(len(e) == top for e in s["top_logprobs"])
        else:
            assert "top_logprobs" not in s
        at += m
    assert at == n                                                   # the <|endoftext|> entry belongs to no segment
    # without the keywords a segment has none of the keys
    plain = tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None,
                            dict(language="en", fp16=False))
    assert plain.repetition == {}
    seg = _one_window(plain, dataclasses.replace(result))["segments"][0]
    assert not {"token_logprobs", "token_entropies", "top_logprobs"} & set(seg)
    # get_writer("json") passes the keys through
    import io
    import json
    from whisper_amd.utils import get_writer
    buf = io.StringIO()
    get_writer("json", ".").write_result(out, buf)
    assert json.loads(buf.getvalue())["segments"][0]["token_logprobs"] == segs[0]["token_logprobs"]


def test_an_emptied_segment_empties_its_lists():
    tr = importlib.import_module("whisper_amd.transcribe")
    tk = whisper_amd.tokenizer.get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    TB = tk.timestamp_begin
    ids = [TB + 10, TB + 10]                                         # start == end: the segment carries no text
    worker = tr._Transcriber(_fake_model(), None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None,
                             dict(language="en", fp16=False, top_logprobs=2))
    result = decoding.DetailedDecodingResult(
        audio_features=torch.zeros(1), language="en", tokens=ids, text="", avg_logprob=-0.1, no_speech_prob=0.0,
        temperature=0.0, compression_ratio=1.0, token_logprobs=[-1.0, -2.0, -3.0], token_entropies=[1.0, 2.0, 3.0],
        top_tokens=[[1, 2]] * 3, top_logprobs=[[-1.0, -2.0]] * 3)
    rest = [TB] + tk.encode(" hello") + [TB + 1400]                  # the next window ends the file
    last = dataclasses.replace(result, tokens=rest, text="hello", token_logprobs=[-1.0] * (len(rest) + 1),
                               token_entropies=[1.0] * (len(rest) + 1), top_tokens=[[1, 2]] * (len(rest) + 1),
                               top_logprobs=[[-1.0, -2.0]] * (len(rest) + 1))
    walk = worker._walk(None, torch.zeros(80, 6000))
    next(walk)
    walk.send(result)
    with pytest.raises(StopIteration) as stop:
        walk.send(last)
    first, second = stop.value.value["segments"]
    assert first["tokens"] == [] and first["token_logprobs"] == [] and first["token_entropies"] == [] and first["top_logprobs"] == []
    assert second["tokens"] == rest and len(second["token_logprobs"]) == len(second["top_logprobs"]) == len(rest)


# ---- the host loop ----------------------------------------------------------------------------------------------------------
class _StubInference(decoding.Inference):
    """logits from a table: [step][row][vocabulary], on the dyadic grid; the first call returns them at every position"""

    def __init__(self, table: torch.Tensor, T0: int):
        self.table, self.T0 = table, T0

    def logits(self, tokens, audio_features):
        step = tokens.shape[1] - self.T0
        x = self.table[step].clone()
        return x[:, None, :].expand(-1, tokens.shape[1], -1).clone() if step == 0 else x[:, None, :]

    def rearrange_kv_cache(self, source_indices):
        pass


@pytest.mark.parametrize("top", [0, 4])
def test_host_loop_against_the_oracle(top):
    """a custom Inference forces the host loop: its four quantities come from the filtered logits in torch fp32 and must be
    float64's on the stub model — tokens and alternatives exactly (the logits lie on the dyadic grid), the values within
    1e-4 (fp32 log_softmax over 5e4 entries, far above its rounding)"""
    model = _fake_model()
    V, steps, B = model.dims.n_vocab, 6, 2
    opts = decoding.DecodingOptions(language="en", fp16=False, sample_len=steps)
    task = decoding.DecodingTask(model, opts, token_logprobs=True, top_logprobs=top, no_repeat_ngram_size=2)
    tk = task.tokenizer
    rng = np.random.default_rng(3)
    table = torch.from_numpy((rng.integers(-2560, 1921, (steps, B, V)) / 64.0).astype(np.float32))
    table[4, 0, tk.eot] = 50.0                                       # row 0 ends at its fifth token, row 1 never does
    table[:, 1, tk.eot] = -40.0
    task.inference = _StubInference(table, task.sample_begin)
    assert not task._fused_greedy_ok(None)
    results = task.run(torch.zeros(B, model.dims.n_audio_ctx, model.dims.n_audio_state))
    r = ro.SamplingRules(sample_begin=task.sample_begin, sot_index=task.sot_index, eot=tk.eot, n_ctx=448,
                         timestamp_begin=tk.timestamp_begin, no_timestamps=tk.no_timestamps,
                         max_initial_timestamp_index=task._max_initial_ts, suppress_blank=True,
                         blank_token=tk.encode(" ")[0], suppress_tokens=list(task._suppress))
    for b, res in enumerate(results):
        assert type(res) is decoding.DetailedDecodingResult
        sampled, n_entries = [], len(res.tokens) + (1 if b == 0 else 0)
        assert len(res.token_logprobs) == len(res.token_entropies) == n_entries
        assert (b == 0 and len(res.tokens) == 4) or (b == 1 and len(res.tokens) == steps)
        assert len(res.top_tokens) == len(res.top_logprobs) == (n_entries if top else 0)
        chosen = list(res.tokens) + [tk.eot]
        for s in range(n_entries):
            tok, lp, H, tt, tv, _ = tso.step_stats(table[s, b].numpy(), sampled, r, top, n=2)
            assert tok == chosen[s], (b, s)
            assert abs(res.token_logprobs[s] - lp) < 1e-4 and abs(res.token_entropies[s] - H) < 1e-4
            if top:
                assert res.top_tokens[s] == tt and res.top_tokens[s][0] == tok
                assert all(abs(a - w) < 1e-4 for a, w in zip(res.top_logprobs[s], tv))
            sampled.append(tok)
        if b == 0:
            assert abs(sum(res.token_logprobs) / (len(res.tokens) + 1) - res.avg_logprob) < 1e-5
    # padding and the special rows, directly
    x = torch.full((3, 6), -math.inf)
    x[0, [1, 4]] = torch.tensor([2.0, 2.0])
    x[2, :] = torch.arange(6.0)
    lp, H, tt, tv = decoding.step_token_stats(x, torch.tensor([1, 0, 0]), torch.tensor([False, False, True]), 3)
    assert tt.tolist() == [[1, 4, -1], [-1, -1, -1], [-1, -1, -1]]
    assert abs(lp[0].item() + math.log(2)) < 1e-6 and abs(H[0].item() - math.log(2)) < 1e-6 and tv[0, 2] == -math.inf
    assert math.isnan(lp[1].item()) and math.isnan(H[1].item()) and lp[2] == 0 and H[2] == 0
    assert (tv[1:] == -math.inf).all()


# ---- the C ABI and the sharded route ----------------------------------------------------------------------------------------
def test_the_setter_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    assert re.search(r"int wh_task_set_token_stats\(wh_task \*t, const wh_token_stats \*s, void \*stream\);", header)
    assert "#define WH_TOKEN_STATS_MAX_TOP 8" in header and "#define WH_ABI_VERSION 1" in header
    m = re.search(r"typedef struct wh_token_stats \{(.*?)\} wh_token_stats;", header, re.S)
    names = re.findall(r"\*?(\w+);", m.group(1))
    assert names == ["token_logprobs", "entropy", "top_k", "top_tokens", "top_logprobs", "stride"]
    assert [n for n, _ in hip.TokenStats._fields_] == names
    assert "wh_task_set_token_stats" in hip.SIGNATURES
    syms = subprocess.run(["nm", "-D", "--defined-only", hip.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT wh_task_set_token_stats\b", syms)
    assert hip.lib().wh_task_set_token_stats(None, None, None) != 0          # a null task: WH_ERR_ARG, no device needed


def test_the_keywords_reach_a_sharded_workers_options(monkeypatch):
    tr = importlib.import_module("whisper_amd.transcribe")
    launcher = importlib.import_module("whisper_amd.launcher")
    seen = {}

    def fake_batch(model, audios, **kwargs):
        seen.update(kwargs)
        # what transcribe_batch does with them: one worker per file, the keywords popped into `repetition`
        worker = tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None,
                                 {k: v for k, v in kwargs.items() if k != "batch_size"})
        seen["worker"] = worker
        return [{} for _ in audios]
    monkeypatch.setattr(tr, "transcribe_batch", fake_batch)
    out = launcher.transcribe_sharded(_fake_model(), [np.zeros(16000, np.float32)] * 2, language="en", top_logprobs=3)
    assert out == [{}, {}]
    assert seen["top_logprobs"] == 3
    assert seen["worker"].repetition == dict(token_logprobs=True, top_logprobs=3)
    assert seen["worker"]._options_for(0.0) == decoding.DecodingOptions(language="en", temperature=0.0)
