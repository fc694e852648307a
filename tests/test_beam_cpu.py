"""tests/beam_oracle.py on the CPU: the float64 candidate reference against oracle.decoding.apply_filters +
F.log_softmax(...).topk, and the extended update model (step_tokens, fin_len, applied, lcp' / copy_from, the frozen
branch) over multi-step runs."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle  # noqa: E402
from oracle.decoding import SamplingRules, apply_filters  # noqa: E402

V, EOT, NO_TS, TB = 96, 60, 69, 70


def _rules(with_ts, max_initial):
    return SamplingRules(sample_begin=3, sot_index=0, eot=EOT, timestamp_begin=TB if with_ts else None, no_timestamps=NO_TS,
                         max_initial_timestamp_index=max_initial, suppress_blank=True, blank_token=5,
                         suppress_tokens=[3, 7, 41, EOT + 1, NO_TS - 1])


HISTORIES = {
    "L0": [], "L1_text": [10], "L1_ts": [TB + 2], "text_text": [10, 11], "ts_text": [TB + 2, 11], "text_ts": [10, TB + 4],
    "ts_ts": [TB + 2, TB + 2], "long": [TB + 1, TB + 1, 12, 13, TB + 6, TB + 6, 14],
}


def test_candidates_equal_apply_filters_log_softmax_topk():
    """Every filter state (L = 0, L = 1, the four last / penultimate combinations, rules off) and max_initial_timestamp_index
    0 / 4 / 50 / None.  fp32 normal logits: log-probabilities agree to fp32 (4 ulp of the value + 4 ulp of the normaliser),
    tokens are equal wherever the float64 gap to both neighbours in the order exceeds that; the finite entries only —
    torch.topk picks arbitrary ids among -inf, the reference gives (-inf, 0)."""
    rng = np.random.default_rng(0)
    K = 6
    checked = fired = quiet = short = 0
    for with_ts in (True, False):
        for max_initial in (0, 4, 50, None):
            for name, hist in HISTORIES.items():
                if not with_ts:
                    hist = [t for t in hist if t < TB]
                for trial in range(6):
                    r = _rules(with_ts, max_initial)
                    x = rng.standard_normal(V).astype(np.float32) * 3
                    if with_ts and trial % 2:
                        x[TB:] += np.float32(rng.uniform(-4, 4))           # both sides of the mass rule
                    want = torch.from_numpy(x.copy())
                    apply_filters(want, hist, r)
                    n_fin = int(torch.isfinite(want).sum())
                    lp = F.log_softmax(want.float(), -1)
                    wv, wi = lp.topk(K)
                    tok, val, info = beam_oracle.candidates(x, hist, r, K, with_info=True)
                    xf, _ = beam_oracle.filtered_float64(x, hist, r)
                    assert np.array_equal(np.isfinite(xf), torch.isfinite(want).numpy()), (with_ts, max_initial, name)
                    n = min(K, n_fin)
                    short += n < K
                    assert np.all(np.isneginf(val[n:])) and np.all(tok[n:] == 0)
                    full = np.sort(xf[np.isfinite(xf)])[::-1]
                    full = full - full[0] - np.log(np.exp(full - full[0]).sum()) if full.size else full
                    for k in range(n):
                        tol = 4 * 2.0 ** -23 * (abs(val[k]) + abs(info["lse"]) + 1)
                        assert abs(float(wv[k]) - val[k]) <= tol, (name, k, float(wv[k]), val[k])
                        gap = min([abs(full[k] - full[j]) for j in (k - 1, k + 1) if 0 <= j < full.size] or [np.inf])
                        if gap > 2 * tol:
                            assert int(wi[k]) == tok[k], (name, k)
                            checked += 1
                    if with_ts and hist is not None and np.isfinite(info["margin"]):
                        fired += info["fired"]
                        quiet += not info["fired"]
    assert checked > 2000 and fired > 20 and quiet > 20 and short >= 12      # L = 0 with max_initial 0 / 4 leaves 1 / 5 entries


def test_candidates_order_ties_and_missing_entries():
    r = _rules(True, None)
    x = np.full(V, -np.inf, dtype=np.float32)
    x[[20, 9, 33]] = [1.5, 1.5, -2.0]
    tok, lp = beam_oracle.candidates(x, [10, 11], r, 5)
    assert tok.tolist() == [9, 20, 33, 0, 0] and lp[0] == lp[1] and np.isneginf(lp[3:]).all()      # equal values: id ascending
    tok, lp = beam_oracle.candidates(np.full(V, -np.inf, dtype=np.float32), [10, 11], r, 4)
    assert tok.tolist() == [0] * 4 and np.isneginf(lp).all()                                       # no NaN
    # a single timestamp that ties the text maximum: "not greater", the rule stays quiet and the smaller id comes first
    x = np.full(V, -np.inf, dtype=np.float32)
    x[[30, TB + 3]] = 2.25
    tok, lp, info = beam_oracle.candidates(x, [10, 11], r, 3, with_info=True)
    assert not info["fired"] and info["margin"] == 0.0 and info["n_ts"] == 1 and tok.tolist() == [30, TB + 3, 0]
    x[TB + 4] = -30.0
    tok, lp, info = beam_oracle.candidates(x, [10, 11], r, 3, with_info=True)
    assert info["fired"] and tok.tolist() == [TB + 3, TB + 4, 0]


def test_extended_update_model_over_random_runs():
    """The outputs the model gained, over runs like those of test_host_logic.py's BeamSearchDecoder comparison (which keeps
    holding the model's tokens, sums, lists and sources): step_tokens are the rows' last tokens, fin_len the lengths of the
    listed sequences, `applied` counts the updates that were not frozen, the frozen branch returns the identity, and a cache
    moved by src / copy_from alone (rows take from their source only the positions from copy_from on) always equals the full
    gather, with lcp' keeping its meaning."""
    rng = np.random.default_rng(1)
    frozen_seen = 0
    for trial in range(60):
        G, B, Vs = int(rng.integers(2, 9)), int(rng.integers(1, 4)), int(rng.integers(14, 40))
        eot, K, R = Vs - 3, G + 1, B * G
        mc = int(rng.choice([1, max(1, G // 2), G, 2 * G]))
        st = dict(tokens=[[1, 2, 3] for _ in range(R)], sums=np.zeros(R, np.float32), fin=[[] for _ in range(B)], done=[0] * B,
                  applied=0, lcp=[[[beam_oracle.LCP_START] * 8 for _ in range(8)] for _ in range(B)])
        cache = [[tuple(st["tokens"][i][: p + 1]) for p in range(3)] for i in range(R)]
        for step in range(14):
            lg = rng.standard_normal((B, Vs)).repeat(G, 0) if step == 0 else rng.standard_normal((R, Vs))
            lg[:, eot] += float(rng.choice([0, 1.5, 3.0]))
            lp = F.log_softmax(torch.tensor(lg, dtype=torch.float32), -1).numpy()
            order = np.lexsort((np.arange(Vs)[None, :].repeat(R, 0), -lp), axis=-1)[:, :K]
            was_done, before, length = all(st["done"]), st, len(st["tokens"][0])
            st, src = beam_oracle.beam_update_model(st, np.take_along_axis(lp, order, 1), order, step == 0, G, K, eot, mc)
            assert st["fin_len"] == [[len(s) for s, _ in f] for f in st["fin"]]
            assert all(n <= mc for n in map(len, st["fin"]))
            if was_done:
                frozen_seen += 1
                assert src == list(range(R)) and st["copy_from"] == [0] * R and st["step_tokens"] == [None] * R
                assert st["applied"] == before["applied"] and st["lcp"] is before["lcp"] and st["done"] == [1] * B
                assert st["tokens"] == before["tokens"] and np.array_equal(st["sums"], before["sums"])
                continue
            assert st["applied"] == before["applied"] + 1
            assert st["step_tokens"] == [row[-1] for row in st["tokens"]]
            old = [list(c) for c in cache]
            for i in range(R):
                if src[i] != i:
                    cache[i][st["copy_from"][i]:length] = old[src[i]][st["copy_from"][i]:length]
            for i in range(R):
                assert cache[i] == old[src[i]], (trial, step, i)
                au = i // G
                for j in range(au * G, au * G + G):
                    n = st["lcp"][au][i - au * G][j - au * G]
                    assert n <= length and cache[i][:n] == cache[j][:n]
                cache[i].append(tuple(st["tokens"][i]))
    assert frozen_seen > 20
