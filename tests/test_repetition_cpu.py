"""Repetition control on the host: the RepetitionPenalty and NoRepeatNGram filters against tests/repetition_oracle.py on
random rows and on hand-made histories, validation, where DecodingTask puts the filters and which route it then reports,
and how transcribe takes the keywords.  No GPU."""
import importlib
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repetition_oracle as ro  # noqa: E402

from whisper_amd import decoding  # noqa: E402

EOT = 100            # a small vocabulary: text 0 .. 99, <|endoftext|> 100, specials and timestamps above
V = 140
TS = 120             # first timestamp id


def _apply(filt, logits, tokens):
    out = logits.clone()
    filt.apply(out, tokens)
    return out


def _want_ban(x, H, n):
    want = x.clone()
    for t in ro.banned_set(H, n, EOT):
        want[t] = -np.inf
    return want


@pytest.mark.parametrize("H,n,banned", [
    ([5, 5, 5], 2, {5}),                       # a a a at n = 2: the context `a` was followed by a
    ([5, 6, 5], 2, {6}),
    ([5, 6, 7], 2, set()),                     # the last token never occurred before
    ([5, 6, 7, 5, 6], 3, {7}),
    ([5, 6, 7, 5, 6, 8, 5, 6], 3, {7, 8}),     # several matches, several tokens
    ([5, 6, 5], 1, {5, 6}),                    # n = 1: every sampled text token
    ([], 1, set()),
    ([], 2, set()),                            # L = n - 2: nothing
    ([5], 2, set()),                           # L = n - 1: a context, but no earlier occurrence
    ([5, 5], 2, {5}),                          # L = n: the match at the only admissible i
    ([5], 3, set()),                           # L = n - 2
    ([5, 5], 3, set()),                        # L = n - 1
    ([5, 5, 5], 3, {5}),                       # L = n
    ([TS + 1, 9, TS + 1], 2, {9}),             # a timestamp inside a context
    ([9, TS + 1, 9], 2, set()),                # the would-be-banned id is a timestamp: never banned
    ([9, EOT, 9], 2, set()),                   # ... or <|endoftext|> itself
    ([9, EOT - 1, 9], 2, {EOT - 1}),           # ... but the last text id is
    ([7, 8, 9, 7, 8], 2, {9}),                 # the match at i = 1; (7, 8) at i = 0 has another context
    ([8, 1, 2, 3, 8], 2, {1}),                 # the match at i = 0
    ([1, 2, 3, 8, 4, 8], 2, {4}),              # the match at the last admissible i = L - n
])
def test_banned_set_on_hand_made_histories(H, n, banned):
    assert ro.banned_set(H, n, EOT) == banned
    filt = decoding.NoRepeatNGram(n, EOT, sample_begin=2)
    assert filt.banned(H) == sorted(banned)
    x = torch.arange(V, dtype=torch.float32) / 8 - 3
    got = _apply(filt, x[None], torch.tensor([[0, 0] + H]))
    assert torch.equal(got[0], _want_ban(x, H, n))
    assert torch.isinf(got[0]).sum() == len(banned)


def test_filters_against_the_oracle_on_random_rows():
    rng = np.random.default_rng(0)
    hits = {"ban": 0, "pen": 0, "special": 0}
    for trial in range(60):
        R, T = 6, int(rng.integers(1, 40))
        n = int(rng.choice([1, 2, 3, 4, 16]))
        p = float(rng.choice([0.5, 1.3, 1.5, 2.0]))
        begins = rng.integers(0, min(T, 5) + 1, R).tolist()
        # a small alphabet so that n-grams do repeat; some timestamps and an <|endoftext|> among them
        tokens = rng.integers(0, 6, (R, T))
        tokens[rng.random((R, T)) < 0.15] = TS + 1
        tokens[rng.random((R, T)) < 0.03] = EOT
        if n == 16 and T >= 34:
            tokens[0, T - 15:] = tokens[0, T - 32: T - 17]          # a 15-token context that did occur before
        tokens = torch.from_numpy(tokens)
        logits = torch.from_numpy(rng.standard_normal((R, V)).astype(np.float32))
        logits[:, 3] = 0.0
        logits[:, 4] = -np.inf
        for ragged in (True, False):
            rb = begins if ragged else None
            got_b = _apply(decoding.NoRepeatNGram(n, EOT, 2, rb), logits, tokens)
            got_p = _apply(decoding.RepetitionPenalty(p, EOT, 2, rb), logits, tokens)
            for r_ in range(R):
                H = tokens[r_, (begins[r_] if ragged else 2):].tolist()
                assert torch.equal(got_b[r_], _want_ban(logits[r_], H, n)), (trial, r_)
                want = logits[r_].numpy().astype(np.float64)
                P = ro.penalised_set(H, EOT)
                ro.penalise(want, P, p)
                assert torch.equal(got_p[r_], torch.from_numpy(want.astype(np.float32))) or \
                    np.allclose(got_p[r_].numpy(), want, rtol=2.0 ** -23, atol=0, equal_nan=True), (trial, r_)
                untouched = [v for v in range(V) if v not in P]
                assert torch.equal(got_p[r_, untouched], logits[r_, untouched])
                hits["ban"] += len(ro.banned_set(H, n, EOT))
                hits["pen"] += len(P)
                hits["special"] += any(t >= EOT for t in H)
    assert hits["ban"] > 200 and hits["pen"] > 200 and hits["special"] > 50


def test_penalty_by_sign_and_once_per_token():
    x = torch.tensor([[6.0, -6.0, 0.0, -np.inf, 6.0, -6.0, 3.0]])
    H = [0, 1, 2, 3, 0, 0, 0, 0, 1]                      # 0 five times, 1 twice; 4, 5, 6 not sampled
    got = _apply(decoding.RepetitionPenalty(1.5, EOT, 1), x, torch.tensor([[9] + H]))
    assert got[0].tolist() == [4.0, -9.0, 0.0, -np.inf, 6.0, -6.0, 3.0]
    # below 1 it encourages; ids >= eot are never penalised
    x = torch.full((1, V), 2.0)
    got = _apply(decoding.RepetitionPenalty(0.5, EOT, 0), x, torch.tensor([[7, EOT, TS + 3, EOT + 1]]))
    assert got[0, 7] == 4.0 and (got[0] != 2.0).sum() == 1
    # the float64 step composes: penalty on the raw logit, the boost afterwards, then the ban
    r = ro.SamplingRules(sample_begin=0, sot_index=0, eot=EOT, timestamp_begin=None, suppress_blank=False, suppress_tokens=[])
    row = np.zeros(V)
    row[[5, 6, 7]] = [8.0, 3.0, 5.0]
    tok, lp, xf = ro.sampler_step(row, [5, 6, 5], r, n=2, penalty=2.0, boosted=[5, 6], boost=2.0)
    assert xf[5] == 8.0 / 2 + 2.0 and xf[6] == -np.inf and tok == 5          # 6 followed 5 before: banned whatever its boost
    assert ro.sampler_step(row, [5, 6, 5], r)[0] == 5 and ro.sampler_step(row, [5, 6, 5], r, penalty=2.0)[0] == 7


def test_validation():
    for bad in (-1, 17, 2.0, "2", True):
        with pytest.raises(ValueError):
            decoding.check_repetition(bad, 1.0)
    for bad in (0.0, -1.0, math.inf, math.nan, "1.5", True):
        with pytest.raises(ValueError):
            decoding.check_repetition(0, bad)
    assert decoding.check_repetition(0, 1.0) == (0, 1.0) and decoding.check_repetition(16, 0.5) == (16, 0.5)
    assert decoding.check_repetition(np.int64(3), np.float32(2.0)) == (3, 2.0)
    with pytest.raises(ValueError):
        decoding.NoRepeatNGram(0, EOT, 0)
    with pytest.raises(ValueError):
        decoding.RepetitionPenalty(0.0, EOT, 0)
    with pytest.raises(ValueError):
        decoding.NoRepeatNGram(2, EOT, 0, row_begin=[0, 0]).apply(torch.zeros(3, V), torch.zeros(3, 4, dtype=torch.int64))


def _fake_model():
    dims = SimpleNamespace(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=2, n_vocab=51865,
                           n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=2)
    return SimpleNamespace(dims=dims, is_multilingual=True, device=torch.device("cpu"), num_languages=99)


def test_decoding_task_places_the_filters_and_keeps_the_device_route():
    model = _fake_model()
    opts = decoding.DecodingOptions(language="en")
    plain = decoding.DecodingTask(model, opts)
    stock = [type(f) for f in plain.logit_filters]
    D = decoding
    both = D.DecodingTask(model, opts, no_repeat_ngram_size=2, repetition_penalty=1.3)
    assert [type(f) for f in both.logit_filters] == [D.RepetitionPenalty, D.NoRepeatNGram] + stock
    assert both.logit_filters[0].penalty == 1.3 and both.logit_filters[1].n == 2
    assert both.logit_filters[0].eot == both.logit_filters[1].eot == both.tokenizer.eot
    assert both.logit_filters[0].sample_begin == both.logit_filters[1].sample_begin == both.sample_begin
    assert both._stock_filters == both.logit_filters and both._fused_greedy_ok(None)
    assert both.ragged_limit() == plain.ragged_limit()
    # RepetitionPenalty -> PhraseBias -> NoRepeatNGram -> the stock filters
    full = D.DecodingTask(model, opts, phrases=["gfx950"], no_repeat_ngram_size=3, repetition_penalty=2.0)
    assert [type(f) for f in full.logit_filters] == [D.RepetitionPenalty, D.PhraseBias, D.NoRepeatNGram] + stock
    assert full._fused_greedy_ok(None)
    assert [type(f) for f in D.DecodingTask(model, opts, no_repeat_ngram_size=1).logit_filters] == [D.NoRepeatNGram] + stock
    assert [type(f) for f in D.DecodingTask(model, opts, repetition_penalty=1.1).logit_filters] == [D.RepetitionPenalty] + stock
    assert [type(f) for f in D.DecodingTask(model, opts, phrases=["a"], no_repeat_ngram_size=1).logit_filters] == \
        [D.PhraseBias, D.NoRepeatNGram] + stock
    for kw in (dict(temperature=0.4, best_of=3), dict(without_timestamps=True)):
        assert D.DecodingTask(model, D.DecodingOptions(language="en", **kw), no_repeat_ngram_size=2)._fused_greedy_ok(None)
    # off: nothing changes
    off = D.DecodingTask(model, opts, no_repeat_ngram_size=0, repetition_penalty=1.0)
    assert [type(f) for f in off.logit_filters] == stock
    # ragged prompts: every row from its own sample_begin
    task = D.DecodingTask(model, opts, prompts=[[1, 2, 3], None], no_repeat_ngram_size=2, repetition_penalty=1.5)
    assert task.logit_filters[0].row_begin == task.logit_filters[1].row_begin == [task.sample_begin, task.sample_begin - 4]
    # beam search: the host loop with the filters
    for kw in (dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.5)):
        beam = D.DecodingTask(model, D.DecodingOptions(language="en", beam_size=3), **kw)
        assert not beam._fused_greedy_ok(None) and not beam._fused_beam_ok() and not beam._beam_shape_ok()
        assert beam.ragged_limit() is None
    assert D.DecodingTask(model, D.DecodingOptions(language="en", beam_size=3))._fused_beam_ok()
    for bad in (dict(no_repeat_ngram_size=17), dict(no_repeat_ngram_size=-1), dict(repetition_penalty=0.0),
                dict(repetition_penalty=math.nan)):
        with pytest.raises(ValueError):
            D.DecodingTask(model, opts, **bad)


def test_transcribe_pops_the_keywords_before_the_options_are_built():
    tr = importlib.import_module("whisper_amd.transcribe")      # (the package attribute of that name is the function)
    model = _fake_model()
    opts = dict(language="en", no_repeat_ngram_size=2, repetition_penalty=1.3, beam_size=2)
    worker = tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None, opts)
    assert worker.repetition == dict(no_repeat_ngram_size=2, repetition_penalty=1.3)
    assert "no_repeat_ngram_size" not in worker.decode_options and "repetition_penalty" not in worker.decode_options
    assert worker._options_for(0.0) == decoding.DecodingOptions(language="en", beam_size=2, temperature=0.0)
    off = tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None,
                          dict(language="en", no_repeat_ngram_size=0, repetition_penalty=1.0))
    assert off.repetition == {}                                 # the decode call is then the one without the keywords
    for bad in (dict(no_repeat_ngram_size=17), dict(repetition_penalty=-2.0)):
        with pytest.raises(ValueError):
            tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None, dict(bad))
        with pytest.raises(ValueError):
            tr.transcribe_batch(model, [np.zeros(16000, np.float32)], **bad)
        with pytest.raises(ValueError):
            tr.transcribe_chunked(model, np.zeros(16000, np.float32), **bad)
        with pytest.raises(ValueError):
            importlib.import_module("whisper_amd.launcher").transcribe_sharded(model, [np.zeros(16000, np.float32)], **bad)
        with pytest.raises(ValueError):
            decoding.decode_many(model, [], **bad)
