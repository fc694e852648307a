"""Restatement of temperature sampling (whisper_amd/csrc/sampling.hip at T > 0, sample_noise.h) for the tests, in plain numpy.
No project code is used here.

  h   = hash(seed_lo, seed_hi, step, row, token)       uint32, bit-exact with sample_noise.h
  u   = ((h >> 9) + 0.5) * 2^-23                       float32, bit-exact (every step is exact in fp32)
  g   = -log(-log u)                                   float64
  key = x / T + g                                      float64, x the FILTERED row, T the temperature as the float32 the
                                                       launch receives
  token = arg-max of the keys over the finite entries of x, lowest id among equal keys
  log-probability = x[token] - log-sum-exp(x): the one of the UNSCALED row

The filtered float64 row is the one phrase_oracle.sampler_step / repetition_oracle.sampler_step return (bias, penalty, ban,
the stock filters and the timestamp-mass rule).

Decidability.  The kernel forms the key in fp32, so its arg-max is the restatement's only where the best key leads:
  EPS_KEY = 2 * 2^-24 * max|x / T|      the rounding of 1 / T and of the product x * (1 / T)
          + 2^-22                       -logf(u) at 2 ulp: a relative error of the inner logarithm is an absolute one of the outer
          + 2 * ulp32(17.4)             the outer logf at 2 ulp, |g| < 17.4
          + ulp32(max|key|)             the final add
(the 2 ulp of logf are the assumption tests/test_phrases_gpu.py already makes; nobody has measured them).  A row is decidable
when its best key beats every other by more than 2 * EPS_KEY and, where the timestamp rules are on, the two sides of the
timestamp-mass rule differ by more than MASS_EPS: the kernel compares (ts_max - all_max) - L + logf(ts_sum) with
(text_max - all_max) - L, L = logf(all_sum) the same float on both sides.  On the dyadic-grid inputs of the tests the two
differences of maxima are exact; logf(ts_sum) carries the relative error of the sum, gamma(V), and 2 ulp of its own; the two
subtractions and the addition round once each at the magnitude of their results.
"""
import math
from typing import Optional, Sequence

import numpy as np

import phrase_oracle
import repetition_oracle

UNIFORM_BITS = 23
SCHUNK = 1024                # sampling.hip: vocabulary entries per stage-1 workgroup
_M32 = np.uint64(0xFFFFFFFF)


def gamma(V: int) -> float:
    """the relative error of a row's sum of exponentials (tests/test_phrases_gpu.py derives it)"""
    nchunk = (V + SCHUNK - 1) // SCHUNK
    return (26 + (nchunk + 255) // 256 + 1) * 6 * 2.0 ** -24


def ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


# ------------------------------------------------------------------------------------------------------------ the noise
def _mul32(a, b):
    return (a * np.uint64(b)) & _M32


def fmix32(h):
    """on uint64 arrays that hold 32-bit values"""
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> np.uint64(13))
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> np.uint64(16))


def sample_hash(seed, step, row, token) -> np.ndarray:
    """uint32 hash of (seed, step, row, token); the arguments broadcast.  seed: the 64-bit noise key of the call"""
    seed = np.asarray(seed, dtype=np.uint64)
    lo, hi = seed & _M32, seed >> np.uint64(32)
    step = np.asarray(step, dtype=np.int64).astype(np.uint64) & _M32
    row = np.asarray(row, dtype=np.int64).astype(np.uint64) & _M32
    token = np.asarray(token, dtype=np.int64).astype(np.uint64) & _M32
    h = fmix32((_mul32(row, 0x9E3779B1) + step) & _M32) ^ lo
    h = fmix32(h ^ _mul32(token, 0x85EBCA77))
    return fmix32((h + hi) & _M32).astype(np.uint32)


def uniform_of_hash(h) -> np.ndarray:
    n = (np.asarray(h, dtype=np.uint32) >> np.uint32(32 - UNIFORM_BITS)).astype(np.float32)
    return (n + np.float32(0.5)) * np.float32(2.0 ** -UNIFORM_BITS)


def gumbel_of_uniform(u) -> np.ndarray:
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def gumbel(seed, step, row, token) -> np.ndarray:
    return gumbel_of_uniform(uniform_of_hash(sample_hash(seed, step, row, token)))


# ------------------------------------------------------------------------------------------------------------- one draw
def _lse(v: np.ndarray) -> float:
    m = v.max() if v.size else -np.inf
    return -np.inf if m == -np.inf else float(m + math.log(np.exp(v - m).sum()))


def draw(xf: np.ndarray, temperature: float, seed: int, step: int, row: int) -> dict:
    """the Gumbel-max draw from a filtered float64 row.  Returns tok, lp (log-probability of the unscaled row), margin (best
    minus second-best key; inf with one allowed entry), eps_key (module docstring).  Every entry filtered: token 0, lp NaN."""
    xf = np.asarray(xf, dtype=np.float64)
    ok = np.flatnonzero(xf != -np.inf)
    if ok.size == 0:
        return dict(tok=0, lp=float("nan"), margin=math.inf, eps_key=0.0)
    T = float(np.float32(temperature))
    scaled = xf[ok] / T
    keys = scaled + gumbel(seed, step, row, ok)
    best = int(np.argmax(keys))                       # the first of equal keys: `ok` is ascending
    if ok.size > 1:
        top2 = np.partition(keys, -2)[-2:]
        margin = float(top2[1] - top2[0])
    else:
        margin = math.inf
    eps = (2 * 2.0 ** -24 * float(np.abs(scaled).max()) + 2.0 ** -22 + 2 * ulp32(17.4) + ulp32(float(np.abs(keys).max())))
    tok = int(ok[best])
    return dict(tok=tok, lp=float(xf[tok] - _lse(xf[ok])), margin=margin, eps_key=eps)


def mass_margin(info: dict, V: int):
    """(|ts_lse - best text log-prob|, MASS_EPS) from the `info` of a sampler_step, or (inf, 0) where the rule has nothing to
    decide (timestamp rules off, or one side empty)"""
    if not info or info["ts_lse"] == -np.inf or info["text_max"] == -np.inf:
        return math.inf, 0.0
    L = info["all_lse"]
    sides = max(abs(info["ts_max"] - L), abs(info["ts_lse"] - L), abs(info["text_max"] - L))
    eps = gamma(V) + 2 * ulp32(info["ts_lse"] - info["ts_max"]) + 3 * ulp32(sides)
    return abs(info["ts_lse"] - info["text_max"]), eps


def filtered_row(logits: np.ndarray, sampled: Sequence[int], r, trie: Optional[phrase_oracle.Trie] = None, state: int = 0,
                 boost: float = 0.0, n: int = 0, penalty: float = 1.0, rep: bool = False) -> dict:
    """the float64 row after bias, penalty, ban, the stock filters and the timestamp-mass rule, with what decidability needs.
    rep: through repetition_oracle (penalty -> boost -> ban -> filters), else through phrase_oracle."""
    info = {}
    if len(sampled) == 0:
        state = 0
    if rep:
        boosted = sorted(trie.boosted(state)) if trie is not None else []
        _, _, xf = repetition_oracle.sampler_step(logits, sampled, r, n, penalty, boosted, boost, info=info)
    else:
        _, _, _, xf = phrase_oracle.sampler_step(logits, sampled, state, trie if trie is not None else phrase_oracle.Trie([]),
                                                 boost, r, info=info)
    mm, me = mass_margin(info, xf.shape[0])
    return dict(xf=xf, state=state, mass_margin=mm, mass_eps=me)


def sample_from(fr: dict, temperature: float, seed: int, step: int, row: int, r, trie: Optional[phrase_oracle.Trie] = None,
                ended: bool = False) -> dict:
    """one sampler step at T > 0 on a filtered_row: tok, lp (None: the row had ended, nothing is accumulated), state (the new
    trie node), margin, eps_key, mass_margin, mass_eps, decidable"""
    d = draw(fr["xf"], temperature, seed, step, row)
    d.update(mass_margin=fr["mass_margin"], mass_eps=fr["mass_eps"])
    d["decidable"] = d["margin"] > 2 * d["eps_key"] and fr["mass_margin"] > fr["mass_eps"]
    if ended:
        d.update(tok=r.eot, lp=None, decidable=True)
    d["state"] = trie.step(fr["state"], d["tok"]) if trie is not None else 0
    return d


def sampler_step(logits: np.ndarray, sampled: Sequence[int], r, temperature: float, seed: int, step: int, row: int,
                 trie: Optional[phrase_oracle.Trie] = None, state: int = 0, boost: float = 0.0, n: int = 0, penalty: float = 1.0,
                 rep: bool = False, ended: bool = False) -> dict:
    return sample_from(filtered_row(logits, sampled, r, trie, state, boost, n, penalty, rep), temperature, seed, step, row, r,
                       trie, ended)


# ----------------------------------------------------------------------------------------------------------- statistics
def mass_bins(p: np.ndarray, n_bins: int, n_draws: int, min_expected: float = 5.0):
    """contiguous id ranges of about equal mass under p: bin index per id (-1 where p == 0) and the bins' masses; neighbours are
    merged until every expected count n_draws * mass is >= min_expected"""
    ids = np.flatnonzero(p > 0)
    c = np.cumsum(p[ids])
    which = np.minimum((c - p[ids] / 2) * n_bins / c[-1], n_bins - 1).astype(np.int64)
    mass = np.bincount(which, weights=p[ids], minlength=n_bins)
    groups, cur, acc = [], [], 0.0                     # merge: walk the bins, closing a group once it is heavy enough
    for b in range(n_bins):
        cur.append(b)
        acc += mass[b]
        if acc / c[-1] * n_draws >= min_expected:
            groups.append(cur)
            cur, acc = [], 0.0
    if cur:                                            # a light tail joins the last group
        if groups:
            groups[-1] += cur
        else:
            groups.append(cur)
    label = np.empty(n_bins, np.int64)
    for g, members in enumerate(groups):
        label[members] = g
    out = np.full(p.shape[0], -1, np.int64)
    out[ids] = label[which]
    return out, np.asarray([mass[m].sum() for m in groups]) / c[-1]


def chi_square(counts: np.ndarray, expected: np.ndarray):
    """(chi-square, degrees of freedom) of one table of counts against expected counts of the same total"""
    counts, expected = np.asarray(counts, np.float64), np.asarray(expected, np.float64)
    return float(((counts - expected) ** 2 / expected).sum()), counts.size - 1


def z_of(chi2: float, dof: int) -> float:
    return (chi2 - dof) / math.sqrt(2.0 * dof) if dof > 0 else 0.0


def goodness_of_fit(tokens: Sequence[int], p: np.ndarray, n_bins: int = 8):
    """chi-square of drawn tokens against the distribution p over equal-mass bins; a token outside p's support adds inf"""
    tokens = np.asarray(tokens, np.int64)
    which, mass = mass_bins(p, n_bins, tokens.size)
    b = which[tokens]
    if (b < 0).any():
        return math.inf, max(mass.size - 1, 1)
    return chi_square(np.bincount(b, minlength=mass.size), mass * tokens.size)


def softmax_t(xf: np.ndarray, temperature: float) -> np.ndarray:
    s = np.asarray(xf, np.float64) / float(np.float32(temperature))
    m = s.max()
    e = np.where(s == -np.inf, 0.0, np.exp(s - m))
    return e / e.sum()
