"""Float64 statement of the per-token statistics (include/whisper_hip.h, wh_task_set_token_stats) for the tests.  No project
code is used here.

The statistics describe the EDITED row of one sampler step, the row `repetition_oracle.sampler_step` returns: penalty ->
boost -> ban -> SuppressBlank -> SuppressTokens -> ApplyTimestampRules -> the timestamp-mass rule (which sets the text range
to -inf where it fires).  With A = the entries of that row that are finite ("allowed"), M = max A, S = sum exp(x - M):
  log-probability of token v   (x[v] - M) - log S
  entropy                      H = -sum_A p log p in nats, p = exp(x - M) / S
  top-k                        the k largest entries of A, value descending, the LOWER id first among equal values, each with
                               its log-probability; fewer than k allowed entries: padded with (-1, -inf)
A row whose last token is <|endoftext|> reports 0, 0, padding (it accumulates nothing); a row with nothing allowed NaN, NaN,
padding.
"""
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

import repetition_oracle as ro

PAD = (-1, -math.inf)


def log_softmax(x: np.ndarray) -> np.ndarray:
    """of the finite entries of a float64 row; -inf elsewhere (a row without finite entries: all NaN)"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    if m == -np.inf:
        return np.full_like(x, np.nan)
    return (x - m) - math.log(np.exp(x - m).sum())


def entropy(x: np.ndarray) -> float:
    lp = log_softmax(x)
    if np.isnan(lp).all():
        return math.nan
    ok = np.isfinite(lp)
    return float(-(np.exp(lp[ok]) * lp[ok]).sum())


def top_k(x: np.ndarray, k: int) -> Tuple[List[int], List[float]]:
    lp = log_softmax(x)
    x = np.asarray(x, dtype=np.float64)
    ids = np.flatnonzero(np.isfinite(x))
    ids = [int(i) for i in ids[np.lexsort((ids, -x[ids]))][:k]]        # value descending, id ascending
    toks = ids + [PAD[0]] * (k - len(ids))
    vals = [float(lp[i]) for i in ids] + [PAD[1]] * (k - len(ids))
    return toks, vals


def row_stats(edited: np.ndarray, chosen: Optional[int], k: int, ended: bool = False):
    """(token log-probability, entropy, top tokens, top log-probabilities) of one edited float64 row.  `chosen`: the token
    the step appended (the arg-max at temperature 0, the draw otherwise)."""
    x = np.asarray(edited, dtype=np.float64)
    if ended:
        return 0.0, 0.0, [PAD[0]] * k, [PAD[1]] * k
    if x.max() == -np.inf:
        return math.nan, math.nan, [PAD[0]] * k, [PAD[1]] * k
    toks, vals = top_k(x, k)
    return float(log_softmax(x)[chosen]), entropy(x), toks, vals


def step_stats(logits: np.ndarray, sampled: Sequence[int], r, k: int, chosen: Optional[int] = None, ended: bool = False,
               info: Optional[dict] = None, **edits):
    """one sampler step in float64: the token (`chosen` = None: the arg-max), and its statistics.  `edits`: n, penalty,
    boosted, boost of repetition_oracle.sampler_step.  Returns (token, logprob, entropy, top tokens, top logprobs, edited row)."""
    tok, _, x = ro.sampler_step(logits, sampled, r, ended=ended, info=info, **edits)
    if chosen is not None and not ended:
        tok = chosen
    return (tok,) + row_stats(x, tok, k, ended) + (x,)


def greedy_decode_stats(model, feats, row_tokens: Sequence[Sequence[int]], sample_len: int, r, top: int, n: int = 0,
                        penalty: float = 1.0):
    """`repetition_oracle.repetition_greedy_decode` (oracle.OracleModel, float32 on the CPU) with its per-step values kept,
    every row decoded alone from its own initial tokens (`row_tokens[k]`; the rows of a batch do not interact, so prompts of
    different lengths need nothing else; `r` describes the longest row).  Per row: tokens (initial ones included) and, per
    sampled token, the log-probability, the entropy, the top tokens / log-probabilities
    (float64 from the float32 filtered logits), the number of allowed entries and the margin between the best and the
    second-best allowed logit."""
    import torch

    from oracle.decoding import SamplingRules, _first_logits, apply_filters
    rows = []
    for k, init in enumerate(row_tokens):
        rk = SamplingRules(**{**r.__dict__, "sample_begin": len(init), "sot_index": r.sot_index - (r.sample_begin - len(init))})
        tokens = torch.tensor([list(init)], dtype=torch.int64)
        f = feats[k: k + 1]
        cache = model.new_cache()
        out = dict(lp=[], H=[], top_t=[], top_v=[], n_allowed=[], margin=[])
        for i in range(sample_len):
            logits = _first_logits(model, f, tokens, rk, cache)[0] if i == 0 else model.decoder(tokens[:, -1:], f, cache)[:, -1]
            x = logits[0].clone().float()
            sampled = tokens[0, rk.sample_begin:].tolist()
            if penalty != 1.0:
                idx = sorted(ro.penalised_set(sampled, rk.eot))
                if idx:
                    v = x[idx]
                    x[idx] = torch.where(v > 0, v / penalty, torch.where(v < 0, v * penalty, v))
            if n:
                ban = sorted(ro.banned_set(sampled, n, rk.eot))
                if ban:
                    x[ban] = -np.inf
            apply_filters(x, sampled, rk)
            tok = int(x.argmax())
            lp, H, tt, tv = row_stats(x.double().numpy(), tok, top)
            best = x.topk(2).values
            out["lp"].append(lp), out["H"].append(H), out["top_t"].append(tt), out["top_v"].append(tv)
            out["n_allowed"].append(int(torch.isfinite(x).sum())), out["margin"].append(float(best[0] - best[1]))
            tokens = torch.cat([tokens, torch.tensor([[tok]])], dim=-1)
            if tok == rk.eot or tokens.shape[-1] > rk.n_ctx:
                break
        out["tokens"] = tokens[0].tolist()
        rows.append(out)
    return rows
