"""Phrase lists on the host: the trie and its CSR form, validation, the CSR walk against the dict walk, the PhraseBias
filter against the walk, and where DecodingTask puts the filter and which route it then reports.  No GPU."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phrase_oracle  # noqa: E402

from whisper_amd import decoding  # noqa: E402
from whisper_amd.phrases import MAX_NODES, MAX_PHRASE_TOKENS, MAX_PHRASES, PhraseList, as_phrase_list  # noqa: E402
from whisper_amd.tokenizer import get_tokenizer  # noqa: E402


def _tokenizer():
    return get_tokenizer(True, num_languages=99, language="en", task="transcribe")


def _shared_prefix_list(rng, n_phrases=50, vocab=40):
    """phrases over a SMALL alphabet so that prefixes are shared, phrases start inside other phrases and a state's child
    token is often also a root child"""
    phrases = []
    while len(phrases) < n_phrases:
        stem = phrases[rng.integers(len(phrases))][: rng.integers(1, 4)] if phrases and rng.random() < 0.6 else []
        p = list(stem) + rng.integers(0, vocab, rng.integers(1, 5)).tolist()
        phrases.append(p[:6])
    return phrases


def test_csr_invariants():
    rng = np.random.default_rng(0)
    phrases = _shared_prefix_list(rng)
    pl = PhraseList(phrases, boost=2.0)
    begin, token, node = pl.child_begin, pl.child_token, pl.child_node
    assert begin.dtype == token.dtype == node.dtype == np.int32
    n_nodes = len({tuple(p[:i]) for p in phrases for i in range(len(p) + 1)})          # distinct prefixes, the empty one = root
    assert pl.n_nodes == n_nodes == begin.shape[0] - 1
    assert pl.n_edges == n_nodes - 1 == token.shape[0] == node.shape[0]                 # one edge into every node but the root
    assert begin[0] == 0 and begin[-1] == pl.n_edges and np.all(np.diff(begin) >= 0)
    for n in range(n_nodes):
        kids = token[begin[n]: begin[n + 1]]
        assert np.all(np.diff(kids) > 0)                                                 # ascending, distinct
    assert sorted(node.tolist()) == list(range(1, n_nodes))                              # every node reachable, exactly once
    seen, todo = {0}, [0]
    while todo:
        n = todo.pop()
        for c in node[begin[n]: begin[n + 1]].tolist():
            assert c not in seen
            seen.add(c)
            todo.append(c)
    assert seen == set(range(n_nodes))
    for p in phrases:                                                                    # every phrase ends at a terminal node
        assert pl.csr_walk(p) in pl.terminal


def test_duplicates_merge_and_prefix_phrase():
    pl = PhraseList([[5, 6, 7], [5, 6, 7], [5, 6], [9]], boost=1.0)
    assert pl.n_nodes == 5 and len(pl) == 4
    inner = pl.walk([5, 6])
    assert inner in pl.terminal and pl.children[inner] == {7: pl.walk([5, 6, 7])}        # the prefix ends at an inner node
    assert pl.child_begin.tolist() == [0, 2, 3, 4, 4, 4]
    assert pl.child_token.tolist() == [5, 9, 6, 7]
    same = PhraseList([[5, 6, 7], [5, 6], [9]], boost=1.0)
    for a, b in zip((pl.child_begin, pl.child_token, pl.child_node), (same.child_begin, same.child_token, same.child_node)):
        assert np.array_equal(a, b)


def test_strings_are_tokenised_with_a_leading_space():
    tk = _tokenizer()
    pl = PhraseList(["  Kubernetes ", "gfx950"], boost=2.5, tokenizer=tk)
    assert pl.phrases == [tuple(tk.encode(" Kubernetes")), tuple(tk.encode(" gfx950"))]
    assert as_phrase_list(pl, tk) is pl and as_phrase_list(None, tk) is None
    assert as_phrase_list(["gfx950"], tk, 7.0).boost == 7.0


@pytest.mark.parametrize("bad", [
    dict(phrases=[]), dict(phrases=[[1, 2], []]), dict(phrases=["  "], tok=True), dict(phrases=[[3, -1]]),
    dict(phrases=[[50257]], tok=True), dict(phrases=[[50364]], tok=True), dict(phrases=[[1]] * (MAX_PHRASES + 1)),
    dict(phrases=[list(range(MAX_PHRASE_TOKENS + 1))]),
    dict(phrases=[[a] + list(range(100, 100 + MAX_PHRASE_TOKENS - 1)) for a in range(MAX_NODES // (MAX_PHRASE_TOKENS) + 2)]),
    dict(phrases=[[1]], boost=0.0), dict(phrases=[[1]], boost=math.inf), dict(phrases=[[1]], boost=math.nan),
    dict(phrases=["word"]), dict(phrases="word", tok=True),
])
def test_validation(bad):
    with pytest.raises(ValueError):
        PhraseList(bad["phrases"], boost=bad.get("boost", 2.0), tokenizer=_tokenizer() if bad.get("tok") else None)


def test_limits_are_inclusive():
    PhraseList([[1]] * MAX_PHRASES, boost=-1.0)
    PhraseList([list(range(MAX_PHRASE_TOKENS))], boost=1.0)
    full = [[a] + list(range(100, 131)) for a in range(2047)] + [[3000 + i] for i in range(MAX_NODES - 1 - 2047 * 32)]
    assert PhraseList(full[:MAX_PHRASES], boost=1.0).n_nodes <= MAX_NODES
    with pytest.raises(ValueError):                      # a list built without a tokenizer is checked where it is used
        PhraseList([[60000]], boost=1.0).check_vocabulary(50257)


def test_csr_walk_equals_dict_walk():
    rng = np.random.default_rng(1)
    phrases = _shared_prefix_list(rng)
    pl = PhraseList(phrases, boost=2.0)
    spec = phrase_oracle.Trie(phrases)
    assert spec.children == pl.children
    reentered = shadowed = 0
    for h in range(1000):
        hist = []
        for _ in range(rng.integers(1, 7)):             # pieces: (part of) a phrase, the tail of one, or noise up to id 49
            p = phrases[rng.integers(len(phrases))]
            kind = rng.random()
            if kind < 0.5:
                hist += p[: rng.integers(1, len(p) + 1)]
            elif kind < 0.75:
                hist += p[rng.integers(len(p)):]        # enters a phrase from its middle
            else:
                hist += rng.integers(0, 50, rng.integers(1, 3)).tolist()
        s_dict = s_csr = s_spec = 0
        for t in hist:
            if s_dict and t in pl.children[s_dict] and t in pl.children[0]:
                shadowed += pl.children[s_dict][t] != pl.children[0][t]      # the edge out of the state must win
            if s_dict and t not in pl.children[s_dict] and t in pl.children[0]:
                reentered += 1
            s_dict, s_csr, s_spec = pl.step(s_dict, t), pl.csr_step(s_csr, t), spec.step(s_spec, t)
            assert s_dict == s_csr == s_spec
            kids = pl.child_token[pl.child_begin[s_csr]: pl.child_begin[s_csr + 1]].tolist()
            roots = pl.child_token[: pl.child_begin[1]].tolist()
            assert pl.boosted(s_dict) == set(kids) | set(roots) == spec.boosted(s_spec)
        assert pl.walk(hist) == pl.csr_walk(hist) == s_dict
    assert reentered > 100 and shadowed > 100            # the histories did exercise both cases


def test_phrase_bias_boosts_exactly_the_walks_set():
    rng = np.random.default_rng(2)
    phrases = _shared_prefix_list(rng)
    pl = PhraseList(phrases, boost=1.75)
    V, R, T = 64, 16, 12
    both = 0
    for trial in range(20):
        begins = rng.integers(1, 6, R).tolist()          # rows of different sample_begin
        tokens = torch.from_numpy(rng.integers(0, 40, (R, T)))
        for r_ in range(R):                               # end most rows inside a phrase
            p = phrases[rng.integers(len(phrases))]
            k = int(rng.integers(0, len(p) + 1))
            if k:
                tokens[r_, T - k:] = torch.tensor(p[:k])
        logits = torch.from_numpy(rng.standard_normal((R, V)).astype(np.float32))
        logits[:, 7] = -np.inf                            # a masked entry stays masked whatever the boost
        want = logits.clone()
        for r_ in range(R):
            state = pl.walk(tokens[r_, begins[r_]:].tolist())
            both += len(set(pl.children[state]) & set(pl.children[0])) if state else 0
            for t in pl.boosted(state):
                want[r_, t] += 1.75                       # once, also where t is a child of the state AND of the root
        decoding.PhraseBias(pl, sample_begin=99, row_begin=begins).apply(logits, tokens)
        assert torch.equal(logits, want)
    assert both > 0
    # one sample_begin for all rows
    logits = torch.zeros(R, V)
    decoding.PhraseBias(pl, sample_begin=3).apply(logits, tokens)
    for r_ in range(R):
        assert set(torch.nonzero(logits[r_])[:, 0].tolist()) == pl.boosted(pl.walk(tokens[r_, 3:].tolist()))


def _fake_model():
    dims = SimpleNamespace(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=2, n_vocab=51865,
                           n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=2)
    return SimpleNamespace(dims=dims, is_multilingual=True, device=torch.device("cpu"), num_languages=99)


def test_decoding_task_places_the_filter_first_and_keeps_the_device_route():
    model = _fake_model()
    opts = decoding.DecodingOptions(language="en")
    plain = decoding.DecodingTask(model, opts)
    for phrases in (["Kubernetes", "gfx950"], PhraseList(["Kubernetes"], boost=-2.0, tokenizer=_tokenizer())):
        task = decoding.DecodingTask(model, opts, phrases=phrases)
        assert type(task.logit_filters[0]) is decoding.PhraseBias and task.logit_filters[0].phrases is task.phrases
        assert [type(f) for f in task.logit_filters[1:]] == [type(f) for f in plain.logit_filters]
        assert task._stock_filters == task.logit_filters
        assert task._fused_greedy_ok(None) and task.ragged_limit() == plain.ragged_limit()
    assert decoding.DecodingTask(model, opts, phrases=["a b"]).phrases.boost == 3.0
    for kw in (dict(temperature=0.4, best_of=3), dict(without_timestamps=True)):
        assert decoding.DecodingTask(model, decoding.DecodingOptions(language="en", **kw), phrases=["gfx950"])._fused_greedy_ok(None)
    # ragged prompts: the filter walks every row from its own sample_begin
    task = decoding.DecodingTask(model, opts, prompts=[[1, 2, 3], None], phrases=["gfx950"])
    assert task.logit_filters[0].row_begin == [task.sample_begin, task.sample_begin - 4]
    # beam search: the host loop with the filter
    beam = decoding.DecodingTask(model, decoding.DecodingOptions(language="en", beam_size=3), phrases=["gfx950"])
    assert type(beam.logit_filters[0]) is decoding.PhraseBias
    assert not beam._fused_greedy_ok(None) and not beam._fused_beam_ok() and not beam._beam_shape_ok()
    assert beam.ragged_limit() is None
    assert decoding.DecodingTask(model, decoding.DecodingOptions(language="en", beam_size=3))._fused_beam_ok()
    # without a list nothing changes
    none = decoding.DecodingTask(model, opts, phrases=None)
    assert none.phrases is None and [type(f) for f in none.logit_filters] == [type(f) for f in plain.logit_filters]
    with pytest.raises(ValueError):
        decoding.DecodingTask(model, opts, phrases=[[51000]])          # a timestamp id


def test_transcribe_pops_the_keywords_before_the_options_are_built():
    import importlib
    tr = importlib.import_module("whisper_amd.transcribe")      # (the package attribute of that name is the function)
    model = _fake_model()
    opts = dict(language="en", phrases=["gfx950"], phrase_boost=50.0, beam_size=2)
    worker = tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None, opts)
    assert worker.phrases.boost == 50.0 and "phrases" not in worker.decode_options and "phrase_boost" not in worker.decode_options
    assert worker._options_for(0.0) == decoding.DecodingOptions(language="en", beam_size=2, temperature=0.0)
    kwargs = dict(phrases=["gfx950"], phrase_boost=4.0, fp16=False)
    tr._compile_phrases(model, kwargs)
    assert isinstance(kwargs["phrases"], PhraseList) and kwargs["phrases"].boost == 4.0 and "phrase_boost" not in kwargs
    assert tr._Transcriber(model, None, 0.0, 2.4, -1.0, 0.6, True, None, False, False, "", "", "0", None, dict(kwargs)).phrases \
        is kwargs["phrases"]
    with pytest.raises(ValueError):
        tr._pop_phrases(model, dict(phrase_boost=2.0))
