"""Per-token statistics end to end on the synthetic tiny checkpoint (fp32): wh_task_set_token_stats + wh_task_greedy against
the float32 oracle decode and against the same loop without statistics, the setter's statuses, and the Python layers
(decode, decode_many, transcribe).  The per-token bound, 2e-3, is the allowance tests/test_repetition_gpu.py gives the
summed value of such a decode.  The largest measured difference goes to token_stats_api_parity.json."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repetition_oracle as ro  # noqa: E402
import test_phrases_gpu as tp  # noqa: E402
import token_stats_oracle as tso  # noqa: E402
import whisper_amd  # noqa: E402
from oracle.decoding import SamplingRules  # noqa: E402
from test_phrases_gpu import micro, setup  # noqa: E402,F401  (module-scoped fixtures: the micro model, the checkpoint)
from whisper_amd import hip  # noqa: E402
from whisper_amd.decoding import DecodingTask, DetailedDecodingResult  # noqa: E402
from whisper_amd.phrases import PhraseList  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = [[1000, 1001, 50257], [50257], [1001, 50257]]       # one ragged batch: lag 0, 2, 1
LAG = [0, 2, 1]
N_STEPS, TOP, AUDIO_SEED = 14, 5, 3                        # audio seed chosen on the CPU: every oracle margin >= 1e-2
MEASURED = {}


def _rules(dims):
    r = tp._loop_rules(dims, 3, True)
    return SamplingRules(**{**r.__dict__, "sot_index": 2})


def _run(task, dev, r, dims, stats, begin=False, top=TOP, temperature=0.0):
    T0 = len(ROWS[0])
    tokens = torch.zeros(3, T0 + N_STEPS + 1, dtype=torch.int64, device=dev)
    for k, row in enumerate(ROWS):
        tokens[k, : len(row)] = torch.tensor(row)
        tokens[k, len(row): T0] = 50257                     # padding of a shorter prompt: any valid id
    mask = tp._mask(r, dims, dev)
    p = tp._params(r, N_STEPS, mask, dims, temperature, 77)
    task.reset()
    task.set_lag(LAG)
    if stats:
        task.set_token_stats(top)
    if begin:
        pend = task.greedy_begin(tokens, p, 2, -1)
        res = None
        while res is None:
            res = pend.poll()
    else:
        res = task.greedy(tokens, p, 2, -1)
    torch.cuda.synchronize()
    assert len(res) == (4 if stats else 3)
    return (tokens.cpu(), res[0], res[1].cpu()) + ((tuple(None if b is None else b.cpu() for b in res[3]),) if stats else ())


def test_greedy_with_statistics(micro, gpu_device):
    """3 rows, one ragged batch, 14 steps, top_k = 5: tokens and sum_logprobs bit-identical with statistics on and off, the
    fp32 sequential sum of a row's token_logprobs reproduces its sum_logprobs bit for bit, entry 0 of the alternatives is the
    token with the token's log-probability bitwise, greedy_begin + poll gives the same bytes, and every per-token value lies
    within 2e-3 of the float32 oracle decode; 0 <= entropy <= log(allowed entries)"""
    dims, om, models = micro
    r = _rules(dims)
    feats = tp._feats(dims, 3, seed=AUDIO_SEED)
    want = tso.greedy_decode_stats(om, feats, ROWS, N_STEPS, r, TOP)
    assert min(min(w["margin"]) for w in want) >= 1e-2
    task = hip.HipTask(models[hip.WH_F32], 3, 1, 8)
    try:
        task.set_audio(feats.to(gpu_device).contiguous())
        tok_off, n_off, lp_off = _run(task, gpu_device, r, dims, False)
        tok_on, n_on, lp_on, st = _run(task, gpu_device, r, dims, True)
        assert n_on == n_off and torch.equal(tok_on, tok_off)
        assert lp_on.numpy().tobytes() == lp_off.numpy().tobytes()
        tok_b, n_b, lp_b, st_b = _run(task, gpu_device, r, dims, True, begin=True)
        assert n_b == n_on and torch.equal(tok_b, tok_on) and lp_b.numpy().tobytes() == lp_on.numpy().tobytes()
        for a, b in zip(st, st_b):
            assert a.numpy().tobytes() == b.numpy().tobytes()
        tok_lp, ent, top_t, top_v = [b.numpy() for b in st]
        assert tok_lp.shape == ent.shape == tuple(tok_on.shape) and top_t.shape == top_v.shape == tuple(tok_on.shape) + (TOP,)
        worst = dict(logprob=0.0, entropy=0.0, top_logprob=0.0)
        for k, w in enumerate(want):
            begin = len(ROWS[k])
            assert tok_on[k, : len(w["tokens"])].tolist() == w["tokens"], k
            total = np.float32(0.0)
            for c in range(begin, tok_on.shape[1]):
                total = np.float32(total + tok_lp[k, c])                 # fp32, in the order of the steps
            assert total.tobytes() == lp_on[k].numpy().tobytes(), k
            # nothing outside the sampled columns was written
            assert (tok_lp[k, :begin] == 0).all() and (top_t[k, :begin] == -1).all() and (tok_lp[k, begin + N_STEPS:] == 0).all()
            for s in range(len(w["lp"])):
                c = begin + s
                assert top_t[k, c, 0] == tok_on[k, c] and top_v[k, c, 0].tobytes() == tok_lp[k, c].tobytes(), (k, s)
                assert (np.diff(top_v[k, c]) <= 0).all() and (top_t[k, c] >= 0).all()
                assert 0.0 <= ent[k, c] <= math.log(w["n_allowed"][s]) + 1e-5, (k, s, ent[k, c])
                worst["logprob"] = max(worst["logprob"], abs(float(tok_lp[k, c]) - w["lp"][s]))
                worst["entropy"] = max(worst["entropy"], abs(float(ent[k, c]) - w["H"][s]))
                worst["top_logprob"] = max(worst["top_logprob"], float(np.abs(top_v[k, c].astype(np.float64) - np.array(w["top_v"][s])).max()))
        print("largest difference from the float32 oracle decode:", worst)
        MEASURED.update(worst)
        assert max(worst.values()) <= 2e-3, worst
        # log-probabilities and entropy alone; sampling: the loop with statistics draws the tokens of the loop without
        _, _, lp_0, st_0 = _run(task, gpu_device, r, dims, True, top=0)
        assert st_0[2] is None and st_0[3] is None and st_0[0].numpy().tobytes() == st[0].numpy().tobytes()
        assert st_0[1].numpy().tobytes() == st[1].numpy().tobytes() and lp_0.numpy().tobytes() == lp_on.numpy().tobytes()
        s_off = _run(task, gpu_device, r, dims, False, temperature=0.8)
        s_on = _run(task, gpu_device, r, dims, True, temperature=0.8)
        assert torch.equal(s_on[0], s_off[0]) and s_on[2].numpy().tobytes() == s_off[2].numpy().tobytes()
        assert not torch.equal(s_on[0], tok_on)
    finally:
        task.close()


def test_setter_statuses_and_refusals(micro, gpu_device):
    """every status of wh_task_set_token_stats; NULL and wh_task_reset clear it; wh_task_greedy refuses a stride below its
    token_stride; wh_task_beam(_begin) refuse while statistics are set; wh_task_prefill / wh_task_step ignore them"""
    dims, om, models = micro
    model = models[hip.WH_F32]
    r = tp._loop_rules(dims, 1, True)
    feats = tp._feats(dims, 3, seed=AUDIO_SEED).to(gpu_device).contiguous()
    L = hip.lib()
    OK, ERR_ARG, ERR_STATE = 0, 1, 4
    task, beam = hip.HipTask(model, 3, 1, 8), hip.HipTask(model, 1, 2, 8)
    try:
        task.set_audio(feats)
        h, s = task.handle, hip.stream_ptr(task.stream)
        S = 1 + 8 + 1
        f = torch.zeros(3, S, dtype=torch.float32, device=gpu_device)
        e = torch.zeros(3, S, dtype=torch.float32, device=gpu_device)
        tt = torch.full((3, S, 8), -1, dtype=torch.int32, device=gpu_device)
        tv = torch.zeros(3, S, 8, dtype=torch.float32, device=gpu_device)

        def st(lp=f, en=e, k=5, t=tt, v=tv, stride=S):
            return C.byref(hip.TokenStats(token_logprobs=hip._ptr(lp), entropy=hip._ptr(en), top_k=k, top_tokens=hip._ptr(t),
                                          top_logprobs=hip._ptr(v), stride=stride))
        assert L.wh_task_set_token_stats(None, st(), None) == ERR_ARG
        for bad in (dict(k=-1), dict(k=9), dict(t=None), dict(v=None), dict(lp=None, en=None, k=0, t=None, v=None),
                    dict(stride=0), dict(stride=-3)):
            assert L.wh_task_set_token_stats(h, st(**bad), s) == ERR_ARG, bad
        for good in (dict(), dict(k=8), dict(k=0), dict(k=0, t=None, v=None), dict(lp=None), dict(en=None),
                     dict(lp=None, en=None), dict(k=1)):
            assert L.wh_task_set_token_stats(h, st(**good), s) == OK, good
        assert L.wh_task_set_token_stats(h, None, s) == OK                        # NULL clears
        tokens = torch.zeros(3, S, dtype=torch.int64, device=gpu_device)
        tokens[:, 0] = 50257
        mask = tp._mask(r, dims, gpu_device)
        p = tp._params(r, 8, mask, dims)
        plain = task.greedy(tokens.clone(), p, 0, -1)
        assert len(plain) == 3                                                   # cleared: the loop of before
        # a stride below the loop's token_stride
        task.reset()
        assert L.wh_task_set_token_stats(h, st(stride=S - 1), s) == OK
        with pytest.raises(hip.HipError):
            task.greedy(tokens.clone(), p, 0, -1)
        with pytest.raises(hip.HipError):
            task.greedy_begin(tokens.clone(), p, 0, -1)
        # wh_task_reset clears it; a begun loop refuses the setter and keeps its own setting
        task.reset()
        assert len(task.greedy(tokens.clone(), p, 0, -1)) == 3
        task.reset()
        work = tokens.clone()
        pend = task.greedy_begin(work, p, 0, -1)
        refused = L.wh_task_set_token_stats(h, st(), s)
        while pend.poll() is None:
            pass
        assert refused == ERR_STATE
        torch.cuda.synchronize()
        assert (f == 0).all() and (tt == -1).all()                              # the refused setting wrote nothing
        # prefill / step ignore the setting
        task.reset()
        raw = task.prefill(tokens[:, :1].contiguous())
        stepped = task.step(tokens[:, 0])
        task.reset()
        assert L.wh_task_set_token_stats(h, st(), s) == OK
        assert torch.equal(task.prefill(tokens[:, :1].contiguous()), raw) and torch.equal(task.step(tokens[:, 0]), stepped)
        torch.cuda.synchronize()
        assert (f == 0).all() and (e == 0).all() and (tt == -1).all() and (tv == 0).all()
        # the beam loop refuses while statistics are set
        beam.set_audio(feats[:1].contiguous())
        buf = torch.zeros(2, 2, S, dtype=torch.int64, device=gpu_device)
        buf[0, :, 0] = 50257
        bp = hip.BeamParams(rules=p, beam_size=2, max_candidates=2)
        bf = torch.zeros(2, S, dtype=torch.float32, device=gpu_device)
        one = C.byref(hip.TokenStats(token_logprobs=bf.data_ptr(), entropy=None, top_k=0, top_tokens=None, top_logprobs=None,
                                     stride=S))
        assert L.wh_task_set_token_stats(beam.handle, one, hip.stream_ptr(beam.stream)) == OK
        for call in (beam.beam, beam.beam_begin):
            with pytest.raises(hip.HipError) as err:
                call(buf, bp, 0, -1)
            assert L.wh_status_string(ERR_STATE).decode() in str(err.value)
        assert L.wh_task_set_token_stats(beam.handle, None, hip.stream_ptr(beam.stream)) == OK
        beam.beam(buf, bp, 0, -1)                                               # cleared: the beam loop runs
        torch.cuda.synchronize()
        assert (bf == 0).all()
    finally:
        task.close()
        beam.close()


def _task_rules(model, opts):
    t = DecodingTask(model, opts)
    tk = t.tokenizer
    return t, SamplingRules(sample_begin=t.sample_begin, sot_index=t.sot_index, eot=tk.eot, n_ctx=448,
                            timestamp_begin=None if opts.without_timestamps else tk.timestamp_begin,
                            no_timestamps=tk.no_timestamps, max_initial_timestamp_index=t._max_initial_ts, suppress_blank=True,
                            blank_token=tk.encode(" ")[0], suppress_tokens=list(t._suppress))


def _allowed_upper(r, V, sampled, n=0):
    """entries the per-entry rules (and the ban) leave: text far above the timestamps, so that the mass rule stays quiet —
    the rule can only shrink the set"""
    x = np.zeros(V)
    x[: r.eot] = 100.0
    return int(np.isfinite(ro.sampler_step(x, sampled, r, n=n)[2]).sum())


def _well_formed(res, r, V, top, n=0):
    assert type(res) is DetailedDecodingResult
    m = len(res.tokens)
    assert len(res.token_logprobs) == len(res.token_entropies) and m <= len(res.token_logprobs) <= m + 1
    closed = len(res.token_logprobs) == m + 1
    assert len(res.top_tokens) == len(res.top_logprobs) == (len(res.token_logprobs) if top else 0)
    if closed:
        assert abs(sum(res.token_logprobs) / (m + 1) - res.avg_logprob) < 1e-5
    chosen = list(res.tokens) + [r.eot]
    for s in range(len(res.token_logprobs)):
        assert res.token_logprobs[s] <= 0.0
        assert 0.0 <= res.token_entropies[s] <= math.log(_allowed_upper(r, V, chosen[:s], n)) + 1e-5, s
        if top:
            assert len(res.top_tokens[s]) == len(res.top_logprobs[s]) == top
            assert res.top_tokens[s][0] == chosen[s] and res.top_logprobs[s][0] == res.token_logprobs[s]
            assert all(a >= b for a, b in zip(res.top_logprobs[s], res.top_logprobs[s][1:]))
    return closed


def test_decode_and_decode_many_return_detailed_results(setup):
    model, mels, tk, _ = setup
    V = model.dims.n_vocab
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=12)
    _, r = _task_rules(model, opts)
    plain = whisper_amd.decode(model, mels[:3], opts)
    assert all(type(p) is whisper_amd.DecodingResult for p in plain)
    for kw, top in ((dict(token_logprobs=True), 0), (dict(top_logprobs=3), 3)):
        got = whisper_amd.decode(model, mels[:3], opts, **kw)
        for g, p in zip(got, plain):
            assert g.tokens == p.tokens and g.avg_logprob == p.avg_logprob
            _well_formed(g, r, V, top)
    # ragged prompts: every row's lists start at its own first sampled token
    prompts = [[1000, 1001, 1002, 1003, 1004], None, [2000, 2001]]
    ragged = whisper_amd.decode(model, mels[:3], opts, prompts=prompts, top_logprobs=2)
    for i, res in enumerate(ragged):
        alone = whisper_amd.decode(model, mels[i], whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=12,
                                                                              prompt=prompts[i]), top_logprobs=2)
        assert res.tokens == alone.tokens and res.top_tokens == alone.top_tokens, i
        assert np.allclose(res.token_logprobs, alone.token_logprobs, atol=1e-4)
        _well_formed(res, r, V, 2)
    # best_of: the statistics follow the sample the ranker selected
    sampled = whisper_amd.decode(model, mels[:2], whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=12,
                                                                             temperature=0.7, best_of=3), top_logprobs=2)
    for res in sampled:
        m = len(res.tokens)
        assert type(res) is DetailedDecodingResult and m <= len(res.token_logprobs) <= m + 1
        if len(res.token_logprobs) == m + 1:
            assert abs(sum(res.token_logprobs) / (m + 1) - res.avg_logprob) < 1e-5
    # the host loop (a custom filter) returns the same lists
    from whisper_amd.decoding import LogitFilter

    class Noop(LogitFilter):
        def apply(self, logits, tokens):
            return None
    task = DecodingTask(model, opts, top_logprobs=3)
    task.logit_filters.append(Noop())
    assert not task._fused_greedy_ok(None)
    fused = whisper_amd.decode(model, mels[:2], opts, top_logprobs=3)
    for f, g in zip(fused, task.run(mels[:2])):
        assert f.tokens == g.tokens and len(f.token_logprobs) == len(g.token_logprobs)
        assert np.allclose(f.token_logprobs, g.token_logprobs, atol=1e-4) and np.allclose(f.token_entropies, g.token_entropies, atol=1e-4)
        assert [t[0] for t in f.top_tokens] == [t[0] for t in g.top_tokens]
    with pytest.raises(ValueError):
        whisper_amd.decode(model, mels[:2], whisper_amd.DecodingOptions(language="en", fp16=False, beam_size=2), token_logprobs=True)
    # decode_many: two batches coalesced into one chain
    batches = [mels[0:2].float(), mels[2:3].float()]
    many = whisper_amd.decode_many(model, batches, opts, chain_rows=24, top_logprobs=3)
    assert [len(m) for m in many] == [2, 1]
    for res, p in zip([x for m in many for x in m], plain):
        assert res.tokens == p.tokens
        _well_formed(res, r, V, 3)


def test_transcribe_segments_carry_the_lists(setup):
    model, mels, tk, _ = setup
    audio = tp._audio(3)[: 16000 * 20]
    kw = dict(language="en", fp16=False, sample_len=16, temperature=0.0, condition_on_previous_text=False,
              no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None)
    base = whisper_amd.transcribe(model, audio, **kw)
    out = whisper_amd.transcribe(model, audio, top_logprobs=2, **kw)
    assert [s["tokens"] for s in out["segments"]] == [s["tokens"] for s in base["segments"]] and out["segments"]
    assert not {"token_logprobs", "token_entropies", "top_logprobs"} & set(base["segments"][0])
    some = 0
    for s in out["segments"]:
        m = len(s["tokens"])
        assert len(s["token_logprobs"]) == len(s["token_entropies"]) == len(s["top_logprobs"]) == m
        for t, lp, H, alt in zip(s["tokens"], s["token_logprobs"], s["token_entropies"], s["top_logprobs"]):
            assert lp <= 0.0 and 0.0 <= H <= math.log(model.dims.n_vocab)
            assert len(alt) == 2 and alt[0] == [t, lp] and alt[0][1] >= alt[1][1]
            some += 1
    assert some >= 3
    lp_only = whisper_amd.transcribe(model, audio, token_logprobs=True, **kw)
    assert "top_logprobs" not in lp_only["segments"][0]
    assert [s["token_logprobs"] for s in lp_only["segments"]] == [s["token_logprobs"] for s in out["segments"]]


def test_statistics_describe_the_edited_distribution(setup):
    """the forcing list [[a, b, c]] at boost 50 alone gives `a a a ...`; with no_repeat_ngram_size = 2 the bigram ban
    removes tokens at some steps: a banned token never appears among that step's alternatives, and the boosted
    continuation leads them where it is allowed"""
    model, mels, tk, (a, b, c, d) = setup
    V = model.dims.n_vocab
    pl = PhraseList([[a, b, c]], boost=50.0, tokenizer=tk)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=16)
    _, r = _task_rules(model, opts)
    res = whisper_amd.decode(model, mels[0], opts, phrases=pl, no_repeat_ngram_size=2, top_logprobs=8)
    _well_formed(res, r, V, 8, n=2)
    chosen = list(res.tokens) + [tk.eot]
    banned_steps = 0
    for s in range(len(res.token_logprobs)):
        ban = ro.banned_set(chosen[:s], 2, tk.eot)
        banned_steps += bool(ban)
        assert not ban & set(res.top_tokens[s]), (s, ban, res.top_tokens[s])
    assert banned_steps >= 3
    assert sum(t in (a, b, c) for t in res.tokens) >= 4                         # the list did decide text tokens
    forced = whisper_amd.decode(model, mels[0], opts, phrases=pl, top_logprobs=8)
    assert forced.tokens != res.tokens


def test_report(gpu_device):
    """runs last: the measured end-to-end differences, as a report of their own (the figures to be judged stand beside the
    kernel test's in profiles/token_stats_parity.json)"""
    from conftest import write_report
    assert MEASURED
    write_report("token_stats_api_parity.json", {"api_max_abs_difference_from_float32_oracle": dict(MEASURED, bound=2e-3)})
