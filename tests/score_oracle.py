"""float64 restatement of teacher-forced scoring: the kernel contract of whisper_amd/csrc/score.hip (`score_rows`) and
`whisper_amd.score()` (`score_hypotheses`, on oracle/model.py's decoder).  Plain torch on the CPU, no project kernel."""
import math
from typing import List, Optional, Sequence

import torch


def score_rows(logits: torch.Tensor, target: torch.Tensor, v_end: int):
    """logits float64 [M][V], target int [M], 1 <= v_end <= V  ->  (logprob [M], top_logprob [M], top_token [M]).

    Over the columns v < v_end: logprob = logit[target] - logsumexp; top_logprob = max logit - logsumexp; top_token = the
    lowest id among equal maxima.  target >= v_end: logprob = -inf.  target < 0 (padded slot): 0, 0, -1."""
    logits = logits.double()
    M, V = logits.shape
    assert 1 <= v_end <= V
    cut = logits[:, :v_end]
    lse = torch.logsumexp(cut, dim=1)
    mx = cut.max(dim=1).values
    # torch.argmax does not promise the first of equal maxima: take the lowest id explicitly
    ids = torch.arange(v_end).expand(M, v_end)
    top = torch.where(cut == mx[:, None], ids, torch.full_like(ids, v_end)).min(dim=1).values
    tgt = target.long()
    inside = (tgt >= 0) & (tgt < v_end)
    picked = cut.gather(1, tgt.clamp(0, v_end - 1)[:, None])[:, 0]
    logprob = torch.where(inside, picked - lse, torch.full_like(lse, -math.inf))
    top_lp = mx - lse
    pad = tgt < 0
    logprob = torch.where(pad, torch.zeros_like(logprob), logprob)
    top_lp = torch.where(pad, torch.zeros_like(top_lp), top_lp)
    top = torch.where(pad, torch.full_like(top, -1), top)
    return logprob, top_lp, top


def score_hypotheses(oracle_model, features: torch.Tensor, initial_tokens: Sequence[Sequence[int]],
                     hypotheses: Sequence[Sequence[Sequence[int]]], eot: int, v_end: Optional[int] = None):
    """`whisper_amd.score` restated: for clip b and hypothesis h the oracle decoder (oracle/model.py) is teacher-forced
    with initial_tokens[b] + h + [eot]; every hypothesis token and the closing eot are scored from the position before
    them (vocabulary="text": v_end = eot, and the closing eot is not scored).

    Returns per clip a list of dicts: token_logprobs, sum_logprob, avg_logprob, top_tokens, top_logprobs (float64)."""
    n_vocab = oracle_model.dims.n_vocab
    v_end = n_vocab if v_end is None else v_end
    out: List[List[dict]] = []
    for b, hyps in enumerate(hypotheses):
        res = []
        for h in hyps:
            init = list(initial_tokens[b])
            seq = init + list(h) + [eot]
            toks = torch.tensor([seq], dtype=torch.long)
            with torch.no_grad():
                logits = oracle_model.decoder(toks, features[b:b + 1].to(torch.float32))[0].double()
            n_scored = len(h) + (1 if v_end > eot else 0)
            first = len(init) - 1
            rows = logits[first:first + n_scored]
            tgt = torch.tensor(seq[first + 1:first + 1 + n_scored], dtype=torch.long)
            if n_scored:
                lp, tlp, tt = score_rows(rows, tgt, v_end)
            else:
                lp = tlp = torch.zeros(0, dtype=torch.float64)
                tt = torch.zeros(0, dtype=torch.long)
            s = float(lp.sum())
            res.append(dict(tokens=list(h), token_logprobs=lp, sum_logprob=s, avg_logprob=s / (len(h) + 1),
                            top_tokens=tt, top_logprobs=tlp))
        out.append(res)
    return out
