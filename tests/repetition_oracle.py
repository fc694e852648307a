"""Restatement of repetition control (include/whisper_hip.h states the semantics) for the tests: the two set definitions
over plain lists, the float64 decision of ONE sampler step (what csrc/sampling.hip computes from a row of logits) and a
greedy decode with the two edits on oracle.OracleModel in float32 on the CPU.  No project code is used here.

H is a row's SAMPLED tokens in order (timestamps included; start-of-transcript sequence, prompt and prefix not), L = |H|.
  penalised set  P = { t in H : t < eot }                                  (a set: a token seen five times is in it once)
  banned set     B = { H[i + n - 1] : 0 <= i <= L - n, H[i .. i + n - 2] == s, H[i + n - 1] < eot }
                     with s the last n - 1 tokens of H, and only if L >= n - 1       (n = 1: s is empty, B = P)
Order of a step: penalty on the raw logit -> phrase boost -> ban -> SuppressBlank -> SuppressTokens -> ApplyTimestampRules.
"""
import math
from typing import Dict, List, Optional, Sequence, Set

import numpy as np
import torch
import torch.nn.functional as F

from oracle.decoding import SamplingRules, _first_logits, apply_filters


def penalised_set(H: Sequence[int], eot: int) -> Set[int]:
    return {int(t) for t in H if t < eot}


def banned_set(H: Sequence[int], n: int, eot: int) -> Set[int]:
    H = [int(t) for t in H]
    L = len(H)
    if n < 1 or L < n - 1:
        return set()
    s = H[L - (n - 1):]
    out = set()
    for i in range(0, L - n + 1):
        if H[i: i + n - 1] == s and H[i + n - 1] < eot:
            out.add(H[i + n - 1])
    return out


def penalise(x: np.ndarray, P: Set[int], p: float) -> None:
    """in place: x / p where positive, x * p where negative; zero and -inf stay"""
    for v in P:
        if x[v] > 0:
            x[v] = x[v] / p
        elif x[v] < 0 and x[v] != -np.inf:
            x[v] = x[v] * p


def sampler_step(logits: np.ndarray, sampled: Sequence[int], r: SamplingRules, n: int = 0, penalty: float = 1.0,
                 boosted: Sequence[int] = (), boost: float = 0.0, ended: bool = False, info: Optional[dict] = None):
    """One row, one step, in float64: penalty -> boost (`boosted`: the ids a phrase list boosts in the row's state) -> ban
    -> SuppressBlank -> SuppressTokens -> ApplyTimestampRules -> arg-max (lowest id among equal maxima) -> log_softmax of
    the edited row.  `ended`: the row's last token is <|endoftext|> (it stays there, nothing is accumulated).
    Returns (token, log-probability to accumulate or None, edited float64 row).
    `info`: a dict that receives, where the timestamp rules are on, the two sides of the timestamp-mass rule (ts_lse,
    text_max) with ts_max and the log-sum-exp of the whole row, all taken before the rule is applied."""
    x = np.asarray(logits, dtype=np.float64).copy()
    V = x.shape[0]
    L = len(sampled)
    if penalty != 1.0:
        penalise(x, {t for t in penalised_set(sampled, r.eot) if t < V}, penalty)
    for t in set(boosted):
        if t < V:
            x[t] += boost
    if n:
        for t in banned_set(sampled, n, r.eot):
            if t < V:
                x[t] = -np.inf
    if r.suppress_blank and L == 0:
        x[[r.blank_token, r.eot]] = -np.inf
    if r.suppress_tokens:
        x[list(r.suppress_tokens)] = -np.inf
    TB = r.timestamp_begin
    if TB is not None:
        if r.no_timestamps is not None:
            x[r.no_timestamps] = -np.inf
        last_ts = L >= 1 and sampled[-1] >= TB
        pen_ts = L < 2 or sampled[-2] >= TB
        if last_ts:
            if pen_ts:
                x[TB:] = -np.inf
            else:
                x[: r.eot] = -np.inf
        stamps = [t for t in sampled if t >= TB]
        if stamps:
            x[TB: stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1] = -np.inf
        if L == 0:
            x[:TB] = -np.inf
            if r.max_initial_timestamp_index is not None:
                x[TB + r.max_initial_timestamp_index + 1:] = -np.inf

        def lse(v):
            m = v.max() if v.size else -np.inf
            return -np.inf if m == -np.inf else m + math.log(np.exp(v - m).sum())
        if info is not None:                      # the two sides of the mass rule, before it is applied
            info.update(ts_lse=lse(x[TB:]), ts_max=x[TB:].max() if x[TB:].size else -np.inf,
                        text_max=x[:TB].max() if TB > 0 else -np.inf, all_lse=lse(x))
        if lse(x[TB:]) > (x[:TB].max() if TB > 0 else -np.inf):      # the same normaliser on both sides
            x[:TB] = -np.inf
    m = x.max()
    tok = int(np.flatnonzero(x == m)[0])
    lp = float(-math.log(np.exp(x - m).sum()))
    if ended:
        tok, lp = r.eot, None
    return tok, lp, x


def repetition_greedy_decode(model, feats: torch.Tensor, initial_tokens: List[int], sample_len: int, r: SamplingRules,
                             n: int = 0, penalty: float = 1.0) -> Dict:
    """oracle.greedy_decode with the two edits in front of the filters (float32, as the oracle decodes).  Returns tokens
    (R, len) incl. the initial ones, sum_logprobs, `margins`: for every decision of a row still running, best minus
    second-best allowed logit after the edits and the filters (inf when one token is allowed), and `ban_steps`: per row, the
    number of steps at which the banned set was not empty."""
    R = feats.shape[0]
    tokens = torch.tensor([list(initial_tokens)] * R, dtype=torch.int64)
    sum_lp = torch.zeros(R)
    cache = model.new_cache()
    margins, ban_steps = [], [0] * R
    for i in range(sample_len):
        if i == 0:
            logits, _ = _first_logits(model, feats, tokens, r, cache)
        else:
            logits = model.decoder(tokens[:, -1:], feats, cache)[:, -1]
        logits = logits.clone().float()
        nxt = torch.empty(R, dtype=torch.int64)
        for k in range(R):
            sampled = tokens[k, r.sample_begin:].tolist()
            if penalty != 1.0:
                idx = sorted(penalised_set(sampled, r.eot))
                if idx:
                    x = logits[k, idx]
                    logits[k, idx] = torch.where(x > 0, x / penalty, torch.where(x < 0, x * penalty, x))
            if n:
                ban = sorted(banned_set(sampled, n, r.eot))
                if ban:
                    logits[k, ban] = -np.inf
                    ban_steps[k] += 1
            apply_filters(logits[k], sampled, r)
            nxt[k] = int(logits[k].argmax())
            lp = F.log_softmax(logits[k].float(), dim=-1)[nxt[k]]
            if tokens[k, -1] != r.eot:
                sum_lp[k] += lp
                top = logits[k].topk(2).values
                margins.append(float(top[0] - top[1]))
            else:
                nxt[k] = r.eot
        tokens = torch.cat([tokens, nxt[:, None]], dim=-1)
        if bool((tokens[:, -1] == r.eot).all()) or tokens.shape[-1] > r.n_ctx:
            break
    return {"tokens": tokens, "sum_logprobs": sum_lp.tolist(), "margins": margins, "ban_steps": ban_steps}


def repeated_bigrams(text_and_stamps: Sequence[int], eot: int) -> List[tuple]:
    """bigrams of a row's sampled tokens whose second element is a text token (< eot) and that occur more than once"""
    seen, twice = set(), []
    for a, b in zip(text_and_stamps[:-1], text_and_stamps[1:]):
        if b < eot:
            if (a, b) in seen:
                twice.append((a, b))
            seen.add((a, b))
    return twice
