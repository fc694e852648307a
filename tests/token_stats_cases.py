"""Inputs of the per-token statistics kernel test (tests/test_token_stats_gpu.py) and what float64 expects of them; host
only, so that tests/test_token_stats_cpu.py can check the generator without a GPU.

Logits lie on the dyadic grid of tests/test_phrases_gpu.py (multiples of 2^-6, |x| < 64).  Every edit is exact in fp32 as
well: the boost is 16, and the logits of the tokens a penalty of 1.25 can touch are multiples of 5 * 2^-6, so that x / 1.25
(a multiple of 4 * 2^-6) and x * 1.25 (a multiple of 25 * 2^-8) are exact.  The edited row is therefore the same numbers in
fp32 and in float64, and token, top-k order and padding must agree exactly.

Every row must clear the margin of the timestamp-mass rule (MASS_BOUND, derived in tests/test_beam_gpu.py): asserted here
when a case is built, so that no row is ever left out of a comparison.
"""
import math

import numpy as np

import phrase_oracle
import repetition_oracle as ro
import token_stats_oracle as tso
from oracle.decoding import SamplingRules

GAMMA_BEAM = (26 + 1) * 6 * 2.0 ** -24
MASS_BOUND = GAMMA_BEAM + 2 * 2.0 ** -20 + 3 * 2.0 ** -16        # tests/test_beam_gpu.py (checked equal on the CPU)
T0 = 6                       # the longest row's sample_begin
BOOSTED = 10                 # the one-phrase list [[10, 11, 12]]: at the root it boosts id 10
BOOST = 16.0
VS, RS, TOPS, LENGTHS = (1000, 1025, 2048, 51866), (1, 3), (1, 5, 8), (0, 1, 2, 17)


def rules(V, with_ts=True, suppress=(41, 5, 7)):
    """the rules of tests/test_phrases_gpu.py"""
    eot, no_ts = (50257, 50364) if V > 51000 else (V - 200, V - 151)
    return SamplingRules(sample_begin=2, sot_index=0, eot=eot, n_ctx=448, timestamp_begin=no_ts + 1 if with_ts else None,
                         no_timestamps=no_ts, max_initial_timestamp_index=50, suppress_blank=True, blank_token=220,
                         suppress_tokens=sorted(suppress))


def history(rng, r, L, i, with_ts):
    """a row's sampled tokens: text ids from [300, 400), with the timestamp patterns the rules distinguish"""
    TB = r.timestamp_begin
    text = lambda k: rng.integers(300, 400, k).tolist()         # noqa: E731
    if L == 0:
        return []
    if not with_ts:
        return text(L)
    if L == 1:
        return [[TB + 3], text(1)][i % 2]
    tail = [[TB + 5, 100], [100, TB + 9], [TB + 9, TB + 9], [100, 101]][i % 4]
    return ([TB + 3] + text(L - 3) if L >= 3 else []) + tail


def build(V, R, with_ts, L, top_k, seed=0, lag=None, rep=None, plant=None):
    """one launch.  lag: ragged rows; rep: (ngram, penalty, with_trie); plant(x, i, r, H): edits row i's logits in place and
    may return `ended` (the row's last token is <|endoftext|>)."""
    rng = np.random.default_rng(7919 * seed + 131 * L + 17 * top_k + V + R + (1 if with_ts else 0))
    r = rules(V, with_ts)
    x = (rng.integers(-2560, 1921, (R, V)) / 64.0).astype(np.float32)          # multiples of 2^-6 in [-40, 30]
    x[:, [BOOSTED, 11, 12]] = np.minimum(x[:, [BOOSTED, 11, 12]], 10.0)
    lag = list(lag) if lag is not None else [0] * R
    n, penalty, with_trie = rep if rep is not None else (0, 1.0, False)
    trie = phrase_oracle.Trie([[BOOSTED, 11, 12]])
    hist, rows, ended, sums = [], [], [], []
    for i in range(R):
        H = history(rng, r, L, i, with_ts)
        if rep is not None and L >= 3 and H[-1] < r.eot:
            H[-3:] = [H[-1], 250 + i, H[-1]]           # a b a: the bigram ban forbids b, the row's best but for the edits
            x[i, 250 + i] = 40.0
        if with_trie:
            x[i, BOOSTED] = 25.0                       # among the row's best only with the boost
        if with_ts and i % 2 == 0:
            x[i, 200 + i] = 45.0                       # a text token above the timestamps' joint mass: the rule stays quiet
        end = False
        if plant is not None:
            end = bool(plant(x, i, r, H))
        if penalty != 1.0:                             # the penalised logits on the grid where the penalty is exact
            P = sorted(t for t in ro.penalised_set(H, r.eot) if t < V)
            x[i, P] = (np.round(x[i, P] * 64 / 5) * 5 / 64).astype(np.float32)
        hist.append(H), rows.append([50258] * (T0 - lag[i]) + H), ended.append(end)
        sums.append(float(rng.integers(-64, 1)) / 4)
    want = []
    for i in range(R):
        rr = SamplingRules(**{**r.__dict__, "sample_begin": T0 - lag[i]})
        info = {}
        boosted = sorted(trie.boosted(0)) if with_trie else []
        tok, lp, H_, tt, tv, xe = tso.step_stats(x[i], hist[i], rr, top_k, ended=ended[i], info=info, n=n, penalty=penalty,
                                                 boosted=boosted, boost=BOOST)
        fired = None
        if with_ts and info and np.isfinite(info["ts_lse"]) and np.isfinite(info["text_max"]):
            margin = abs(info["ts_lse"] - info["text_max"])
            assert margin > MASS_BOUND, ("mass-rule margin", V, R, L, i, margin)
            fired = info["ts_lse"] > info["text_max"]
        elif with_ts and info:
            fired = info["ts_lse"] > info["text_max"]
        m = xe.max()
        LS = math.log(np.exp(xe - m).sum()) if m != -np.inf else math.nan
        want.append(dict(tok=tok, lp=lp, H=H_, top_t=tt, top_v=tv, xe=xe, LS=LS, fired=fired, ended=ended[i],
                         n_allowed=int(np.isfinite(xe).sum())))
    return dict(V=V, R=R, x=x, rows=rows, hist=hist, lag=lag, T0=T0, ntok=T0 + L, sums=sums, r=r, with_ts=with_ts, trie=trie,
                with_trie=with_trie, n=n, penalty=penalty, top_k=top_k, want=want)


# ---- planted rows -----------------------------------------------------------------------------------------------------------
def plant_chunk_edge(x, i, r, H):
    """equal maxima at ids 1023 and 1024: the last entry of the first 1024-entry chunk and the first of the second"""
    x[i, [1023, 1024]] = 50.0


def plant_one_thread(x, i, r, H):
    """equal maxima in the four entries thread 44 of the first chunk holds (ids 44 + 256 j)"""
    x[i, [44, 300, 556, 812]] = 50.0


def plant_few(x, i, r, H):
    """three finite entries: fewer than a top-k of 5 or 8"""
    keep = x[i, [10, 700, 701]].copy()
    x[i, :] = -np.inf
    x[i, [10, 700, 701]] = keep


def plant_special(x, i, r, H):
    """row 1: every logit filtered; row 2: already at <|endoftext|>"""
    if i == 1:
        x[i, :] = -np.inf
    if i == 2:
        H[-1] = r.eot
        return True


def grid_cases():
    """(V, R, with_ts, L, top_k) of the grid: every combination"""
    return [(V, R, ts, L, k) for V in VS for R in RS for ts in (True, False) for L in LENGTHS for k in TOPS]


def planted_cases():
    """name -> build() arguments of the planted launches"""
    out = {}
    for V in (2048, 51866):
        for ts in (False, True):
            out[f"chunk_edge-{V}-{'ts' if ts else 'nots'}"] = dict(V=V, R=3, with_ts=ts, L=2, top_k=5, plant=plant_chunk_edge)
            out[f"one_thread-{V}-{'ts' if ts else 'nots'}"] = dict(V=V, R=3, with_ts=ts, L=2, top_k=5, plant=plant_one_thread)
    for k in (5, 8):
        out[f"few-{k}"] = dict(V=1025, R=3, with_ts=False, L=2, top_k=k, plant=plant_few)
    for V in (1000, 51866):
        out[f"special-{V}"] = dict(V=V, R=3, with_ts=True, L=2, top_k=5, plant=plant_special)
    out["lag"] = dict(V=51866, R=3, with_ts=True, L=2, top_k=5, lag=[0, 3, 2])
    for V in (1025, 51866):
        out[f"edits-{V}"] = dict(V=V, R=3, with_ts=True, L=17, top_k=8, rep=(2, 1.25, True))
    return out
