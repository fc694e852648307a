"""Repetition control on the GPU: the sampler kernels with the REP flag against float64, wh_task_greedy +
wh_task_set_repetition against the CPU oracle, a property that holds whatever the model, the lifecycle, and the Python
interface (include/whisper_hip.h states the semantics, tests/repetition_oracle.py restates them).

The log-probability bound of the kernel test is the one tests/test_phrases_gpu.py derives in its module docstring
(`gamma(V)` plus the ulp terms).  It carries over unchanged because the inputs stay on the dyadic grid (multiples of 2^-6,
|x| < 64) and the penalty of the kernel test is 2: x / 2 and x * 2 are exact in fp32, as x + boost is, so the token must be
float64's and all the error is in log(sum exp(x - max)).  The helpers (guarded buffers, rules, micro model) are that file's.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_lib  # noqa: E402
import phrase_oracle  # noqa: E402
import repetition_oracle as ro  # noqa: E402
import test_phrases_gpu as tp  # noqa: E402
import whisper_amd  # noqa: E402
from oracle.decoding import SamplingRules  # noqa: E402
from test_phrases_gpu import micro, setup  # noqa: E402,F401  (module-scoped fixtures: the micro model, the checkpoint)
from whisper_amd import hip  # noqa: E402
from whisper_amd.phrases import PhraseList  # noqa: E402

pytestmark = pytest.mark.gpu

_P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
Buf, gamma, ulp32 = tp.Buf, tp.gamma, tp.ulp32


def klib():
    h = kernel_lib.lib()
    if not getattr(h, "_repetition_ready", False):
        h.wht_greedy_sample_rep.restype = _I
        h.wht_greedy_sample_rep.argtypes = [_P, _L, _I, _I, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P,
                                            ctypes.c_size_t, _F, ctypes.c_uint64, _P, _I, _I, _P, _P, _P, _P, _P, _F, _I, _F, _P]
        h.wht_greedy_sample_scratch_bytes.restype = ctypes.c_size_t
        h.wht_greedy_sample_scratch_bytes.argtypes = [_I, _I]
        h.wht_phrase_root_table.restype = _I
        h.wht_phrase_root_table.argtypes = [_P, _P, _P, _I, _I, _P, _P]
        h._repetition_ready = True
    return h


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sampler kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
ALT = 3                      # the unlisted, never sampled id that wins once the planted winners are edited away (45.0)
BOOSTED = 10                 # the one-phrase list [[10, 11, 12]]: at the root it boosts id 10
SUPPRESSED = 5
N_SCEN = 10


def _history(rng, r, V, L, n, scen, place):
    """a row's sampled tokens (length L) and the logits to plant, for one scenario; falls back to a plain random history
    where L is too short for the scenario.  Filler and context ids come from ranges nothing else uses."""
    fill = lambda k: rng.integers(300, 400, k).tolist()                      # noqa: E731
    nctx = max(n - 1, 0)
    ctx = rng.integers(100, 200, nctx).tolist()
    edge = [1023, 1024] if r.eot > 1024 else [r.eot - 1, 0]                  # slice edges; small vocabularies: the text range's ends
    target = {1: edge[0], 2: edge[1], 3: SUPPRESSED, 4: BOOSTED}.get(scen, 250)
    plant = {ALT: 45.0}
    if scen == 9:
        target_x = -10.0                                                     # a negative logit under the penalty
    elif scen == 4:
        target_x = 50.0 - 16.0                                               # the row's best only with the boost
    else:
        target_x = 50.0
    if scen == 7 and nctx:
        ctx[0] = r.no_timestamps + 6                                         # a timestamp inside the context
    if scen == 6:                                                            # the match at the last admissible i = L - n:
        if L < max(n, 1):                                                    # the history ends with n times the same token
            return fill(L), plant
        plant[250] = 50.0
        return fill(L - max(n, 1)) + [250] * max(n, 1), plant
    if scen == 8:                                                            # sampled but not banned: the penalty alone
        if L < 2:
            return fill(L), plant
        H = fill(L)
        H[L // 2] = 250
        H[0] = 250                                                           # (twice: penalised once)
        H[-1] = 299                                                          # a last token that never occurred before
        plant[250] = 50.0
        return H, plant
    k = 3 if scen == 5 else 1                                                # several matches banning several tokens
    need = k * (nctx + 1) + nctx
    if L < need:
        return fill(L), plant
    targets = [target, 251, 252][:k]
    occ = []
    for t in targets:
        occ += ctx + [t]
    start = [0, 250, 256 - nctx, L - need, 256 - (nctx + 1) // 2][place % 5]  # also across the 256-token tile boundary
    start = min(max(start, 0), L - need)
    H = fill(start) + occ + fill(L - need - start) + ctx
    assert len(H) == L
    for j, t in enumerate(targets):
        plant[t] = target_x - j
    return H, plant


def _case(V, R, mode, L, n, penalty, with_trie, idx):
    rng = np.random.default_rng(100000 * idx + 1000 * L + 10 * n + V + R)
    with_ts = mode != "nots"
    r = tp._rules(V, with_ts, suppress=(41, SUPPRESSED, 7))
    trie = phrase_oracle.Trie([[BOOSTED, 11, 12]])
    x = (rng.integers(-4095, 4096, (R, V)) / 64.0).astype(np.float32)        # multiples of 2^-6, |x| < 64
    x = np.minimum(x, 30.0).astype(np.float32)        # room for the planted entries, also above the timestamps' joint mass
    x[:, [BOOSTED, 11, 12]] = np.minimum(x[:, [BOOSTED, 11, 12]], 14.0)
    lag = [(3 * i) % 4 for i in range(R)] if mode == "lag" else [0] * R
    T0 = 6
    rows, sums, ended, hist = [], [], [], []
    for i in range(R):
        # the launches with L = n have exactly one admissible i: their row 0 is pinned to the scenario that matches there
        scen = 6 if (i == 0 and L == n and n >= 1) else (i + idx) % N_SCEN
        H, plant = _history(rng, r, V, L, n, scen, idx + i)
        at_eot = mode == "mid" and i % 7 == 6 and L >= 1
        if at_eot:
            H[-1] = r.eot
        for t, v in plant.items():
            x[i, t] = v
        rows.append([50258] * (T0 - lag[i]) + H)
        hist.append(H)
        sums.append(float(rng.integers(-64, 1)) / 4)
        ended.append(at_eot)
    ntok = T0 + L
    want = []
    for i in range(R):
        rr = SamplingRules(**{**r.__dict__, "sample_begin": T0 - lag[i]})
        boosted = sorted(trie.boosted(0)) if with_trie else []
        tok, lp, _ = ro.sampler_step(x[i], hist[i], rr, n, penalty, boosted, 16.0, ended=ended[i])
        plain = ro.sampler_step(x[i], hist[i], rr, 0, 1.0, boosted, 16.0, ended=ended[i])[0]
        want.append(dict(tok=tok, lp=lp, plain=plain))
    return dict(x=x, rows=rows, lag=lag, T0=T0, ntok=ntok, sums=sums, r=r, trie=trie, want=want, with_ts=with_ts,
                with_trie=with_trie, n=n, penalty=penalty, hist=hist)


def _launch(case, V, R, temperature=0.0, seed=0):
    h = klib()
    r, x = case["r"], case["x"]
    TB = r.timestamp_begin if case["with_ts"] else -1
    stride = case["ntok"] + 3
    tokens = np.full((R, stride), -7, dtype=np.int64)
    rs = np.zeros((R, 4), dtype=np.int32)
    for i, row in enumerate(case["rows"]):
        tokens[i, : len(row)] = row
        sampled = case["hist"][i]
        if case["with_ts"]:
            stamps = [t for t in sampled if t >= TB]
            rs[i, 0] = int(len(sampled) >= 1 and sampled[-1] >= TB)
            rs[i, 1] = int(len(sampled) >= 2 and sampled[-2] >= TB)
            rs[i, 2] = stamps[-1] + 1 if stamps else 0
    begin, token, node = case["trie"].csr()
    mask = np.zeros(V, dtype=np.uint8)
    mask[list(r.suppress_tokens)] = 1
    nbytes = h.wht_greedy_sample_scratch_bytes(R, V)
    b = dict(x=Buf(x), tokens=Buf(tokens), ntok=Buf(np.array([case["ntok"]], np.int32)), lag=Buf(np.array(case["lag"], np.int32)),
             mask=Buf(mask), sums=Buf(np.array(case["sums"], np.float32)), step=Buf(np.full(R, -7, np.int64)),
             alive=Buf(np.array([-5], np.int32)), part=Buf(np.zeros(nbytes // 4, np.float32)), rs=Buf(rs), begin=Buf(begin),
             token=Buf(token), node=Buf(node), root=Buf(np.full(V, 77, np.int32)), span=Buf(np.full((R, 2), 77, np.int32)))
    trie_on = case["with_trie"]
    if trie_on:
        assert h.wht_phrase_root_table(b["begin"].ptr(), b["token"].ptr(), b["node"].ptr(), len(token), V, b["root"].ptr(), None) == 0
    pt = (lambda name: b[name].ptr()) if trie_on else (lambda name: None)
    rc = h.wht_greedy_sample_rep(b["x"].ptr(), V, R, V, b["tokens"].ptr(), stride, b["ntok"].ptr(),
                                 b["lag"].ptr() if any(case["lag"]) else None, case["T0"], r.eot, TB, r.no_timestamps,
                                 r.max_initial_timestamp_index, 1, r.blank_token, b["mask"].ptr(), b["sums"].ptr(),
                                 b["step"].ptr(), b["alive"].ptr(), b["part"].ptr(), nbytes, temperature, seed, b["rs"].ptr(),
                                 len(begin) - 1, len(token), pt("begin"), pt("token"), pt("node"), pt("root"), pt("span"),
                                 16.0, case["n"], case["penalty"], None)
    assert rc == 0
    torch.cuda.synchronize()
    for name, buf in b.items():
        assert buf.guards_intact(), name
    assert np.array_equal(b["x"].get().view(np.uint32), x.view(np.uint32)), "the logits buffer must not be written"
    return {k: v.get() for k, v in b.items()}, rs


def _plan(mode):
    """(L, n, penalty) of every launch of one case.  The grid: every n in {1, 2, 3, 16} with the history lengths n - 2, n - 1,
    n, 255, 256, 257 and 300 + n, the ban on in EVERY one of them, alone and together with the penalty in turn (two launches each, so that
    each meets a launch with the phrase list and one without).  Length 0 is
    the `first` mode (there with every n); `nots` and `lag` run it once more for every n (`mid` cannot: a row with no
    sampled token is at its first).  Beside the grid: the penalty alone at lengths 1, 256 and 300, and five more ban
    launches around the tile boundary and at lengths no multiple of anything."""
    grid = []
    for n in (1, 2, 3, 16):
        if mode == "first":
            lengths = [0]
        else:
            lengths = sorted({L for L in (n - 2, n - 1, n, 255, 256, 257, 300 + n) if L >= (1 if mode == "mid" else 0)})
        grid += [(L, n) for L in lengths]
    plan = [(L, n, (1.0, 2.0)[j // 2 % 2]) for j, (L, n) in enumerate(grid)]    # in pairs: the phrase list alternates singly
    if mode != "first":
        plan += [(1, 0, 2.0), (256, 0, 2.0), (300, 0, 2.0)]
        plan += [(300, 16, 2.0), (257, 3, 1.0), (256, 2, 2.0), (41, 16, 1.0), (47, 16, 2.0)]
    return plan


@pytest.mark.parametrize("mode", ["mid", "first", "nots", "lag"])
@pytest.mark.parametrize("R", [1, 3, 24])
@pytest.mark.parametrize("V", [1000, 1025, 51866])
def test_sampler_kernels_against_float64(gpu_device, V, R, mode):
    """greedy_partial_kernel <*, *, true> + greedy_final_kernel through wht_greedy_sample_rep.  Histories of length
    n - 2, n - 1, n, 255, 256, 257 and about 300 for every n in {1, 2, 3, 16}, each with the ban on (`_plan`; length 0 is
    the `first` mode and, once more, `nots` and `lag`), and the penalty alone beside them; row 0 of every L = n launch
    holds the one match such a history admits (i = 0 = L - n), every other row one of ten scenarios in turn: a banned token that
    is the row's arg-max, one at a slice edge (ids 1023 and 1024; the ends of the text range in the small vocabularies),
    one that is also suppressed, one that is also the boosted phrase token (all three flags on, every second launch has
    the list), three matches banning three tokens, the match at the last admissible i, a timestamp inside the context, a
    sampled token under the penalty alone (seen twice, penalised once), a negative logit under the penalty; contexts
    placed at the start, across the 256-token tile boundary and at the end; rows already at <|endoftext|> (`mid`); the
    timestamp rules mid-sequence, at the first token, off, and ragged rows.  Token exact, log-probability within the
    bound of test_phrases_gpu.py, timestamp-rule state as before, guard bytes intact, logits untouched.
    The edit must have decided the token in at least 5 rows per mode — except `first`: H is empty at a row's first token,
    so both sets are empty by definition and the edited row is the plain one (which is what is asserted there)."""
    decided = 0
    for idx, (L, n, penalty) in enumerate(_plan(mode)):
        case = _case(V, R, mode, L, n, penalty, with_trie=idx % 2 == 0, idx=idx)
        out, rs0 = _launch(case, V, R)
        TB = case["r"].timestamp_begin
        for i, w in enumerate(case["want"]):
            m = len(case["rows"][i])
            assert out["tokens"][i, m] == w["tok"] == out["step"][i], (idx, L, n, penalty, i, out["tokens"][i, m], w)
            assert out["tokens"][i, m + 1] == -7 and list(out["tokens"][i, :m]) == case["rows"][i]
            if case["with_ts"]:
                is_ts = w["tok"] >= TB
                assert list(out["rs"][i, :3]) == [int(is_ts), rs0[i, 0], w["tok"] + 1 if is_ts else rs0[i, 2]]
            else:
                assert list(out["rs"][i, :3]) == [0, 0, 0]
            if w["lp"] is None:                            # the row had ended: nothing accumulated, bit for bit
                assert out["sums"][i] == np.float32(case["sums"][i]) and w["tok"] == case["r"].eot
            else:
                total = case["sums"][i] + w["lp"]
                bound = gamma(V) + 3 * ulp32(w["lp"]) + ulp32(total)
                assert abs(float(out["sums"][i]) - total) <= bound, (idx, L, n, i, float(out["sums"][i]), total, bound)
            if mode == "first":
                assert w["tok"] == w["plain"] and w["tok"] >= TB
            decided += w["tok"] != w["plain"]
    print("rows whose token the edit decided:", decided)
    if mode != "first":
        assert decided >= 5


def test_sampling_instantiation_never_draws_the_banned_token(gpu_device):
    """<true, false, true>: temperature 1.  The Gumbel noise of the 23-bit uniform lies in [-2.81, 16.64] and spans less than
    20.2 (test_phrases_gpu.py) and the logits are drawn with |x| < 12, a spread of 24.  Token a sits 48 > 20.2 above token b and b 48 > 20.2 + 24 above
    everything else: without the ban a is drawn with certainty, with it (n = 1, a sampled before) a is never drawn and b
    is, with certainty.  Its log-probability is x[b] - log-sum-exp of the EDITED row (a at -inf)."""
    V, R, a, b_ = 51866, 24, 1234, 4321
    rng = np.random.default_rng(5)
    r = tp._rules(V, with_ts=False)
    x = (rng.integers(-767, 768, (R, V)) / 64.0).astype(np.float32)
    x[:, b_] = 12.0 + 48.0
    x[:, a] = 12.0 + 96.0
    spread = float(np.delete(x, [a, b_], axis=1).max() - x.min())
    assert 48.0 > (17.33 + 2.86) + spread
    H = [100, a, 101]
    case = dict(x=x, rows=[[50258] * 6 + H] * R, hist=[H] * R, lag=[0] * R, T0=6, ntok=9, sums=[0.0] * R, r=r,
                trie=phrase_oracle.Trie([[BOOSTED]]), with_ts=False, with_trie=False, n=1, penalty=1.0)
    out, _ = _launch(case, V, R, temperature=1.0, seed=0x1234567890)
    for i in range(R):
        xe = x[i].astype(np.float64)
        xe[[100, a, 101]] = -np.inf
        m = xe.max()
        lp = xe[b_] - m - math.log(np.exp(xe - m).sum())
        assert out["tokens"][i, 9] != a
        assert out["tokens"][i, 9] == b_
        assert abs(float(out["sums"][i]) - lp) <= gamma(V) + 4 * ulp32(lp) + 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# 2. the device-side loop through the C ABI against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _run_greedy(task, dev, init, r, dims, n_steps, B, n=0, penalty=1.0, phrases=None, boost=0.0, begin=False,
                temperature=0.0, seed=0):
    tokens = torch.zeros(B, len(init) + n_steps + 1, dtype=torch.int64, device=dev)
    tokens[:, : len(init)] = torch.tensor(init)
    mask = tp._mask(r, dims, dev)
    p = tp._params(r, n_steps, mask, dims, temperature, seed)
    if phrases is not None:
        task.set_phrases(PhraseList(phrases, boost=boost).device_arrays(dev), boost)
    if n or penalty != 1.0:
        task.set_repetition(n, penalty)
    if begin:
        pend = task.greedy_begin(tokens, p, 0, -1)
        res = None
        while res is None:
            res = pend.poll()
        count, lp, _ = res
    else:
        count, lp, _ = task.greedy(tokens, p, 0, -1)
    torch.cuda.synchronize()
    return tokens[:, :count].cpu(), lp.cpu()


# audio seeds found on the CPU (24 steps, 2 rows) so that conditions (a) and (b) of the test hold: (with_ts, n, penalty) -> seed
LOOP_SEEDS = {(True, 1, 1.0): 8, (True, 2, 1.0): 21, (True, 0, 1.5): 8, (True, 2, 1.5): 8,
              (False, 1, 1.0): 6, (False, 0, 1.5): 6, (False, 2, 1.5): 6}


@pytest.mark.parametrize("with_ts,n,penalty", sorted(LOOP_SEEDS, reverse=True),
                         ids=[("ts" if k[0] else "nots") + f"_n{k[1]}_p{k[2]}" for k in sorted(LOOP_SEEDS, reverse=True)])
def test_task_greedy_with_repetition_against_the_oracle(micro, gpu_device, with_ts, n, penalty):
    """wh_task_set_repetition + wh_task_greedy, fp32 strict engine, 2 rows x 24 steps, against repetition_oracle's decode:
    token ids exact, sum_logprobs within 2e-3 (the bound of test_kernels_gpu.py::test_fused_greedy).  The audio seed of
    every configuration was chosen on the CPU so that (a) the edited path leaves the plain one in at least 3 positions of
    at least one row and (b) the oracle's smallest margin between the best and second-best allowed logit is >= 1e-2 —
    both asserted here.
    n = 2 alone WITHOUT timestamps is not among the configurations: on random weights a repeated bigram is rare, the ban
    was set on at most one step per row and never changed the path for any of the audio seeds 0 .. 199, so no seed gives
    condition (a) (with timestamps seed 21 does: 7 positions).  n = 2 is decided by
    test_no_repeat_property_under_a_forcing_list below, and without timestamps it runs here together with the penalty."""
    dims, om, models = micro
    B, n_steps = 2, 24
    init = [50257] + ([] if with_ts else [tp._loop_rules(dims, 1).no_timestamps])
    r = tp._loop_rules(dims, len(init), with_ts)
    feats = tp._feats(dims, B, seed=LOOP_SEEDS[(with_ts, n, penalty)])
    want = ro.repetition_greedy_decode(om, feats, init, n_steps, r, n, penalty)
    base = ro.repetition_greedy_decode(om, feats, init, n_steps, r)
    m = min(want["tokens"].shape[1], base["tokens"].shape[1])
    assert (want["tokens"][:, :m] != base["tokens"][:, :m]).sum(dim=1).max() >= 3             # (a)
    assert min(want["margins"]) >= 1e-2, min(want["margins"])                                 # (b)
    task = hip.HipTask(models[hip.WH_F32], B, 1, 8)
    try:
        task.set_audio(feats.to(gpu_device).contiguous())
        got, lp = _run_greedy(task, gpu_device, init, r, dims, n_steps, B, n, penalty)
        print("sum_logprobs", lp.tolist(), want["sum_logprobs"])
        assert torch.equal(got, want["tokens"])
        assert np.allclose(lp.numpy(), np.array(want["sum_logprobs"]), atol=2e-3)
    finally:
        task.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a property that holds whatever the model
# ---------------------------------------------------------------------------------------------------------------------
def _sampled(row, r, T0):
    """a row's sampled tokens up to (not including) <|endoftext|>"""
    out = []
    for t in row[T0:].tolist():
        if t == r.eot:
            break
        out.append(t)
    return out


def _assert_property(got, r, n, min_text=6):
    for row in got:
        H = _sampled(row, r, 1)
        text = [t for t in H if t < r.eot]
        assert len(text) >= min_text, H
        if n == 2:
            assert ro.repeated_bigrams(H, r.eot) == [], H
        else:
            assert len(set(text)) == len(text), H


@pytest.mark.parametrize("dt", [hip.WH_F32, hip.WH_F16], ids=["f32", "f16"])
@pytest.mark.parametrize("B,G,temperature", [(3, 1, 0.0), (24, 1, 0.0), (2, 2, 0.5)], ids=["3rows", "24rows", "best_of2"])
def test_no_repeat_property_under_a_forcing_list(micro, gpu_device, dt, B, G, temperature):
    """The set-up of test_phrases_gpu.py::test_forced_walk: the one-phrase list [[a, b, c]] at boost 50 decides every
    text token, and alone it gives the text `a a a a ...`.  With no_repeat_ngram_size = 2 no bigram of a row's sampled tokens
    whose second element is a text token occurs twice, and every row still has at least 6 text tokens; with n = 1 no text
    token occurs twice.  fp32 and fp16; 3 rows, 24 rows, best_of = 2 at temperature 0.5.  The 3-row fp16 case also through
    greedy_begin / poll, and on a task whose hand-offs are forced to expire: the re-run on the two-launch kernels gives the
    tokens of a task that runs them from the start."""
    dims, om, models = micro
    model = models[dt]
    r = tp._loop_rules(dims, 1, True)
    a, b, c, d = tp._forced_ids(r)
    R = B * G
    feats = tp._feats(dims, B, seed=5).to(gpu_device, model.torch_dtype).contiguous()
    task = hip.HipTask(model, B, G, 8)
    kw = dict(phrases=[[a, b, c]], boost=50.0, temperature=temperature, seed=99)
    try:
        task.set_audio(feats)
        forced, _ = _run_greedy(task, gpu_device, [50257], r, dims, 24, R, **kw)
        if temperature == 0:
            assert any(ro.repeated_bigrams(_sampled(row, r, 1), r.eot) for row in forced)   # the list alone does repeat
        results = {}
        for n in (2, 1):
            task.reset()
            got, lp = _run_greedy(task, gpu_device, [50257], r, dims, 24, R, n=n, **kw)
            _assert_property(got, r, n, min_text=6 if n == 2 else 1)
            results[n] = (got, lp)
        if dt == hip.WH_F16 and (B, G) == (3, 1):
            task.reset()
            polled, lp2 = _run_greedy(task, gpu_device, [50257], r, dims, 24, R, n=2, begin=True, **kw)
            assert torch.equal(polled, results[2][0]) and torch.equal(lp2, results[2][1])
    finally:
        task.close()
    if dt == hip.WH_F16 and (B, G) == (3, 1):
        ref = hip.HipTask(model, B, 1, 8, two_launch_self=True, two_launch_cross=True)
        flaky = hip.HipTask(model, B, 1, 8, expire_handoffs=True)
        try:
            ref.set_audio(feats)
            want, want_lp = _run_greedy(ref, gpu_device, [50257], r, dims, 24, R, n=2, **kw)
            flaky.set_audio(feats)
            assert flaky.fused_cross_attention
            rerun, rerun_lp = _run_greedy(flaky, gpu_device, [50257], r, dims, 24, R, n=2, **kw)
            assert flaky.handoff_fallbacks == 1
            assert torch.equal(rerun, want) and torch.equal(rerun_lp, want_lp)
            _assert_property(rerun, r, 2)
        finally:
            ref.close()
            flaky.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. lifecycle
# ---------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_statuses(micro, gpu_device):
    """every status of wh_task_set_repetition; (0, 1.0) and wh_task_reset clear it — a decode on the task afterwards equals
    a decode on a fresh task; wh_task_beam(_begin) refuse while it is set; wh_task_prefill / wh_task_step ignore it."""
    dims, om, models = micro
    B, n_steps = 3, 24
    r = tp._loop_rules(dims, 1, True)
    feats = tp._feats(dims, B, seed=28).to(gpu_device).contiguous()
    model = models[hip.WH_F32]
    L = hip.lib()
    fresh = hip.HipTask(model, B, 1, 8)
    try:
        fresh.set_audio(feats)
        plain, plain_lp = _run_greedy(fresh, gpu_device, [50257], r, dims, n_steps, B)
    finally:
        fresh.close()
    task = hip.HipTask(model, B, 1, 8)
    beam = hip.HipTask(model, 1, 2, 8)
    try:
        task.set_audio(feats)
        h, s = task.handle, hip.stream_ptr(task.stream)
        assert L.wh_task_set_repetition(None, 2, 1.5, None) == 1                 # WH_ERR_ARG
        for bad in ((-1, 1.0), (17, 1.0), (2, 0.0), (2, -1.5), (0, math.inf), (0, -math.inf), (0, math.nan)):
            assert L.wh_task_set_repetition(h, bad[0], bad[1], s) == 1, bad
        for good in ((16, 1.0), (0, 0.5), (1, 3.0e38), (0, 1.0)):
            assert L.wh_task_set_repetition(h, good[0], good[1], s) == 0, good
        edited, _ = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B, n=1, penalty=1.5)
        assert not torch.equal(edited, plain)
        task.reset()                                                           # ... which cleared it
        again, again_lp = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B)
        assert torch.equal(again, plain) and torch.equal(again_lp, plain_lp)
        task.reset()
        task.set_repetition(1, 1.5)
        task.set_repetition(0, 1.0)                                            # (0, 1.0) clears
        again, again_lp = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B)
        assert torch.equal(again, plain) and torch.equal(again_lp, plain_lp)
        # refused while a begun loop is pending; the loop that is running keeps its own setting
        task.reset()
        tokens = torch.zeros(B, 1 + n_steps + 1, dtype=torch.int64, device=gpu_device)
        tokens[:, 0] = 50257
        mask = tp._mask(r, dims, gpu_device)
        p = tp._params(r, n_steps, mask, dims)
        pend = task.greedy_begin(tokens, p, 0, -1)
        refused = L.wh_task_set_repetition(h, 1, 1.5, s)
        while pend.poll() is None:
            pass
        assert refused == 4                                                    # WH_ERR_STATE
        torch.cuda.synchronize()
        assert torch.equal(tokens[:, : plain.shape[1]].cpu(), plain)

        beam.set_audio(feats[:1].contiguous())
        buf = torch.zeros(2, 2, 1 + 8 + 1, dtype=torch.int64, device=gpu_device)
        buf[0, :, 0] = 50257
        bp = hip.BeamParams(rules=tp._params(r, 8, mask, dims), beam_size=2, max_candidates=2)
        for setting in ((2, 1.0), (0, 1.5)):
            beam.set_repetition(*setting)
            with pytest.raises(hip.HipError):
                beam.beam(buf, bp, 0, -1)
            with pytest.raises(hip.HipError):
                beam.beam_begin(buf, bp, 0, -1)
        beam.set_repetition(0, 1.0)
        beam.beam(buf, bp, 0, -1)                                              # cleared: the beam loop runs
        # wh_task_prefill / wh_task_step ignore the setting: raw logits
        task.reset()
        raw = task.prefill(tokens[:, :1].contiguous())
        stepped = task.step(tokens[:, 0])
        task.reset()
        task.set_repetition(1, 4.0)
        assert torch.equal(task.prefill(tokens[:, :1].contiguous()), raw)
        assert torch.equal(task.step(tokens[:, 0]), stepped)
    finally:
        task.close()
        beam.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. Python
# ---------------------------------------------------------------------------------------------------------------------
def _no_repeated_bigram(tokens, eot):
    return ro.repeated_bigrams([t for t in tokens], eot) == []


def test_decode_fused_route_equals_host_loop(setup):
    """decode(..., no_repeat_ngram_size=2, repetition_penalty=1.3) on the device-side loop against the same task pushed
    onto the host loop by a no-op filter (RepetitionPenalty + NoRepeatNGram + wh_task_step): fp32, tokens equal,
    avg_logprob within 1e-4 — form and bound of tests/test_api_gpu.py::test_generic_loop_equals_fused; greedy with and
    without timestamps, and with a phrase list between the two filters"""
    from whisper_amd.decoding import DecodingTask, LogitFilter

    class Noop(LogitFilter):
        def apply(self, logits, tokens):
            return None
    model, mels, tk, _ = setup
    rep = dict(no_repeat_ngram_size=2, repetition_penalty=1.3)
    for kw, extra in ((dict(), {}), (dict(without_timestamps=True), {}), (dict(), dict(phrases=tp._moderate(setup)))):
        opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=20, **kw)
        fused = whisper_amd.decode(model, mels[:2], opts, **rep, **extra)
        task = DecodingTask(model, opts, **rep, **extra)
        assert task._fused_greedy_ok(None)
        task.logit_filters.append(Noop())
        assert not task._fused_greedy_ok(None)
        generic = task.run(mels[:2])
        plain = whisper_amd.decode(model, mels[:2], opts, **extra)
        for f, g in zip(fused, generic):
            assert f.tokens == g.tokens and abs(f.avg_logprob - g.avg_logprob) < 1e-4
            assert _no_repeated_bigram(f.tokens, tk.eot)
        assert [f.tokens for f in fused] != [p.tokens for p in plain]       # the options did change the path
    with pytest.raises(ValueError):
        whisper_amd.decode(model, mels[:2], opts, no_repeat_ngram_size=17)
    with pytest.raises(ValueError):
        whisper_amd.decode(model, mels[:2], opts, repetition_penalty=0.0)


def test_ragged_prompts_and_decode_many_with_repetition(setup):
    model, mels, tk, _ = setup
    rep = dict(no_repeat_ngram_size=2, repetition_penalty=1.3)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=16)
    prompts = [[1000, 1001, 1002, 1003, 1004], None, [2000, 2001]]
    together = whisper_amd.decode(model, mels[:3], opts, prompts=prompts, **rep)
    for i, p in enumerate(prompts):
        alone = whisper_amd.decode(model, mels[i], whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=16, prompt=p),
                                   **rep)
        assert together[i].tokens == alone.tokens, i
        assert abs(together[i].avg_logprob - alone.avg_logprob) < 1e-4
    batches = [mels[0:2].float(), mels[2:3].float(), mels[3:6].float()]
    many = whisper_amd.decode_many(model, batches, opts, chain_rows=24, **rep)
    plain = whisper_amd.decode_many(model, batches, opts, chain_rows=24)
    assert [len(m) for m in many] == [2, 1, 3]
    flat = [r for m in many for r in m]
    for i, res in enumerate(flat):
        alone = whisper_amd.decode(model, mels[i], opts, **rep)
        assert res.tokens == alone.tokens, i
        assert _no_repeated_bigram(res.tokens, tk.eot)
    assert [r.tokens for r in flat] != [r.tokens for m in plain for r in m]


def test_beam_search_with_repetition_runs_the_host_route(setup):
    """beam 3 with the forcing list [[a, b, c]] at boost 50 (alone: `a a a ...`) and no_repeat_ngram_size = 2: the host
    loop with the filters; the winner honours the ban"""
    from whisper_amd.decoding import DecodingTask
    model, mels, tk, (a, b, c, d) = setup
    pl = PhraseList([[a, b, c]], boost=50.0, tokenizer=tk)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=14, beam_size=3)
    assert not DecodingTask(model, opts, phrases=pl, no_repeat_ngram_size=2)._fused_beam_ok()
    assert not DecodingTask(model, opts, no_repeat_ngram_size=2)._fused_beam_ok()
    res = whisper_amd.decode(model, mels[0], opts, phrases=pl, no_repeat_ngram_size=2)
    text = [t for t in res.tokens if t < tk.eot]
    assert len(text) >= 4 and text[0] == a, text
    assert _no_repeated_bigram(res.tokens, tk.eot), res.tokens


def test_transcribe_with_repetition(setup):
    model, mels, tk, (a, b, c, d) = setup
    audio = np.concatenate([tp._audio(3), tp._audio(4)])[: 16000 * 45]
    kw = dict(language="en", fp16=False, sample_len=16, temperature=0.0, condition_on_previous_text=False,
              no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None)
    forced = whisper_amd.transcribe(model, audio, phrases=[[a, b, c]], phrase_boost=50.0, **kw)
    out = whisper_amd.transcribe(model, audio, phrases=[[a, b, c]], phrase_boost=50.0, no_repeat_ngram_size=2, **kw)

    def windows(result):
        by_seek = {}
        for seg in result["segments"]:
            by_seek.setdefault(seg["seek"], []).extend(seg["tokens"])
        return by_seek
    assert any(not _no_repeated_bigram(w, tk.eot) for w in windows(forced).values())       # the list alone does repeat
    assert len(windows(out)) >= 2
    for seek, toks in windows(out).items():
        assert len([t for t in toks if t < tk.eot]) >= 3 and _no_repeated_bigram(toks, tk.eot), (seek, toks)
    # the defaults are the call without the keywords
    base = whisper_amd.transcribe(model, audio, **kw)
    off = whisper_amd.transcribe(model, audio, no_repeat_ngram_size=0, repetition_penalty=1.0, **kw)
    assert [s["tokens"] for s in off["segments"]] == [s["tokens"] for s in base["segments"]] and off["text"] == base["text"]
    with pytest.raises(ValueError):
        whisper_amd.transcribe(model, audio, no_repeat_ngram_size=-1, **kw)
