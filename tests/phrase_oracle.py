"""Restatement of phrase-list biasing (whisper_amd/phrases.py states the semantics) for the tests: a token trie over plain
dicts with its walk, the float64 decision of ONE sampler step (what csrc/sampling.hip computes from a row of logits), and a
biased greedy decode on oracle.OracleModel in float32 on the CPU.  No project code is used here."""
import math
from typing import Dict, List, Optional, Sequence, Set

import numpy as np
import torch
import torch.nn.functional as F

from oracle.decoding import SamplingRules, _first_logits, apply_filters


class Trie:
    """all phrases (token-id lists) in one trie, node 0 the root; nodes numbered in order of creation"""

    def __init__(self, phrases: Sequence[Sequence[int]]):
        self.children: List[Dict[int, int]] = [{}]
        for p in phrases:
            n = 0
            for t in p:
                if t not in self.children[n]:
                    self.children[n][t] = len(self.children)
                    self.children.append({})
                n = self.children[n][t]

    def step(self, state: int, token: int) -> int:
        if token in self.children[state]:           # the edge out of the state wins
            return self.children[state][token]
        return self.children[0].get(token, 0)       # else the edge out of the root, else the root

    def walk(self, tokens: Sequence[int], state: int = 0) -> int:
        for t in tokens:
            state = self.step(state, int(t))
        return state

    def boosted(self, state: int) -> Set[int]:
        return set(self.children[state]) | set(self.children[0])

    def csr(self):
        """(child_begin, child_token, child_node) int32 arrays, child tokens ascending within a node"""
        begin, token, node = [0], [], []
        for kids in self.children:
            for t in sorted(kids):
                token.append(t)
                node.append(kids[t])
            begin.append(len(token))
        return np.asarray(begin, np.int32), np.asarray(token, np.int32), np.asarray(node, np.int32)


def sampler_step(logits: np.ndarray, sampled: Sequence[int], state: int, trie: Trie, boost: float, r: SamplingRules,
                 ended: bool = False, info: Optional[dict] = None):
    """One row, one step, in float64: bias -> SuppressBlank -> SuppressTokens -> ApplyTimestampRules -> arg-max (lowest id
    among equal maxima) -> log_softmax of the filtered row.  `sampled`: the row's sampled tokens so far; the state counts
    as the root when there are none.  `ended`: the row's last token is <|endoftext|> (it stays there, nothing is
    accumulated).  Returns (token, log-probability to accumulate or None, new state, filtered float64 row).
    `info`: a dict that receives, where the timestamp rules are on, the two sides of the timestamp-mass rule (ts_lse,
    text_max) with ts_max and the log-sum-exp of the whole row, all taken before the rule is applied."""
    x = np.asarray(logits, dtype=np.float64).copy()
    if len(sampled) == 0:
        state = 0
    for t in trie.boosted(state):
        if t < x.shape[0]:
            x[t] += boost
    V = x.shape[0]
    L = len(sampled)
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
    assert V > tok
    return tok, lp, trie.step(state, tok), x


def biased_greedy_decode(model, feats: torch.Tensor, initial_tokens: List[int], sample_len: int, r: SamplingRules,
                         trie: Optional[Trie], boost: float) -> Dict:
    """oracle.greedy_decode with the phrase bias in front of the filters (float32, as the oracle decodes).  Returns tokens
    (R, n) incl. the initial ones, sum_logprobs, states (per row, after every step) and `margins`: for every step of every
    row still running, best minus second-best allowed logit after biasing and filtering (inf when one token is allowed)."""
    R = feats.shape[0]
    tokens = torch.tensor([list(initial_tokens)] * R, dtype=torch.int64)
    sum_lp = torch.zeros(R)
    cache = model.new_cache()
    state = [0] * R
    states, margins = [], []
    for i in range(sample_len):
        if i == 0:
            logits, _ = _first_logits(model, feats, tokens, r, cache)
        else:
            logits = model.decoder(tokens[:, -1:], feats, cache)[:, -1]
        logits = logits.clone()
        nxt = torch.empty(R, dtype=torch.int64)
        for k in range(R):
            sampled = tokens[k, r.sample_begin:].tolist()
            if trie is not None:
                idx = sorted(trie.boosted(state[k] if sampled else 0))
                logits[k, idx] += boost
            apply_filters(logits[k], sampled, r)
            nxt[k] = int(logits[k].argmax())
            lp = F.log_softmax(logits[k].float(), dim=-1)[nxt[k]]
            if tokens[k, -1] != r.eot:
                sum_lp[k] += lp
                top = logits[k].topk(2).values
                margins.append(float(top[0] - top[1]))
            else:
                nxt[k] = r.eot
            if trie is not None:
                state[k] = trie.step(state[k] if sampled else 0, int(nxt[k]))
        states.append(list(state))
        tokens = torch.cat([tokens, nxt[:, None]], dim=-1)
        if bool((tokens[:, -1] == r.eot).all()) or tokens.shape[-1] > r.n_ctx:
            break
    return {"tokens": tokens, "sum_logprobs": sum_lp.tolist(), "states": states, "margins": margins}
