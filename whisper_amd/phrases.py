"""Phrase lists ("hotwords"): boost given phrases while decoding — contextual biasing by shallow fusion over a token trie.

No counterpart in the reference, whose only handle is `initial_prompt` (it costs context, cannot be weighted, and is only
guaranteed to reach the first window).  The semantics, which the device-side sampler (csrc/sampling.hip), the host-loop
filter (`decoding.PhraseBias`) and the test oracle all restate:

* All phrases of a list go into one trie; node 0 is the root, duplicates merge, a phrase that is a prefix of another ends
  at an inner node.  The list has ONE scalar `boost` (finite, non-zero; negative discourages the phrases).
* Every decoded row carries a state, a trie node; it is the root when the row's first token is sampled.
* At a step with state s, `boost` is added to the raw fp32 logit of every token that labels an edge out of s or an edge out
  of the root (once where it labels both) — before SuppressBlank / SuppressTokens / ApplyTimestampRules, like a LogitFilter
  at the front of `logit_filters`.  A suppressed token stays suppressed; the timestamp-mass rule, log_softmax and
  `sum_logprobs` see the biased logits.
* After token t is chosen: the child of s reached by t, else the root's child reached by t, else the root.  A timestamp,
  <|endoftext|> or any token outside the list therefore returns the row to the root.

Two limits, both deliberate: there are no failure links other than to the root (after abandoning a phrase half-way, another
phrase is only picked up from its first token), and a boost already given to a phrase that is then abandoned is not taken
back.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Set, Tuple, Union

import numpy as np
import torch

MAX_PHRASES = 4096
MAX_PHRASE_TOKENS = 32
MAX_NODES = 65535
DEFAULT_BOOST = 3.0          # logit units: a listed token wins over an unlisted one the model prefers by up to e^3 ~ 20 x

Phrase = Union[str, Sequence[int]]


class PhraseList:
    """`phrases`: strings (tokenised as `tokenizer.encode(" " + phrase.strip())`) and / or token-id lists (taken as they are).
    Compiles the trie to CSR arrays — `child_begin` int32[n_nodes + 1], `child_token` int32[n_edges] (ascending within a
    node), `child_node` int32[n_edges] — and keeps the dict form, over which `step` / `walk` / `boosted` ARE the
    specification.  Raises ValueError for: an empty list or phrase; a token id < 0 or >= tokenizer.eot (specials and
    timestamps); more than 4096 phrases, 32 tokens in a phrase or 65535 nodes; a boost that is not finite or is 0; string
    phrases without a tokenizer.  Without a tokenizer the upper id bound is checked by `check_vocabulary` where the list is
    used (DecodingTask does)."""

    def __init__(self, phrases: Sequence[Phrase], boost: float = DEFAULT_BOOST, tokenizer=None):
        boost = float(boost)
        if not math.isfinite(boost) or boost == 0.0:
            raise ValueError(f"phrase boost must be finite and non-zero (got {boost})")
        if isinstance(phrases, (str, bytes)):
            raise ValueError("phrases must be a list of phrases, not one string")
        phrases = list(phrases)
        if not phrases:
            raise ValueError("empty phrase list")
        if len(phrases) > MAX_PHRASES:
            raise ValueError(f"{len(phrases)} phrases: at most {MAX_PHRASES} per list")
        self.boost = boost
        self.eot: Optional[int] = int(tokenizer.eot) if tokenizer is not None else None
        self.phrases: List[Tuple[int, ...]] = []
        for p in phrases:
            if isinstance(p, str):
                if tokenizer is None:
                    raise ValueError("string phrases need a tokenizer")
                ids = tokenizer.encode(" " + p.strip()) if p.strip() else []
            else:
                ids = [int(t) for t in (p.tolist() if hasattr(p, "tolist") else p)]
            if not ids:
                raise ValueError(f"empty phrase: {p!r}")
            if len(ids) > MAX_PHRASE_TOKENS:
                raise ValueError(f"phrase {p!r} has {len(ids)} tokens: at most {MAX_PHRASE_TOKENS}")
            if min(ids) < 0 or (self.eot is not None and max(ids) >= self.eot):
                raise ValueError(f"phrase {p!r}: token ids must lie in [0, <|endoftext|>) — no specials, no timestamps")
            self.phrases.append(tuple(ids))

        # the trie over dicts: children[n] maps a token to the child it leads to; nodes are numbered in order of creation
        self.children: List[Dict[int, int]] = [{}]
        self.terminal: Set[int] = set()
        for ids in self.phrases:
            n = 0
            for t in ids:
                nxt = self.children[n].get(t)
                if nxt is None:
                    nxt = len(self.children)
                    if nxt >= MAX_NODES:
                        raise ValueError(f"the phrase trie has more than {MAX_NODES} nodes")
                    self.children[n][t] = nxt
                    self.children.append({})
                n = nxt
            self.terminal.add(n)

        begin, token, node = [0], [], []
        for kids in self.children:
            for t in sorted(kids):
                token.append(t)
                node.append(kids[t])
            begin.append(len(token))
        self.child_begin = np.asarray(begin, dtype=np.int32)
        self.child_token = np.asarray(token, dtype=np.int32)
        self.child_node = np.asarray(node, dtype=np.int32)
        self._device: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        self._root_tokens: Dict[torch.device, torch.Tensor] = {}

    @property
    def n_nodes(self) -> int:
        return len(self.children)

    @property
    def n_edges(self) -> int:
        return int(self.child_token.shape[0])

    def check_vocabulary(self, eot: int) -> None:
        """every token id must lie below `eot` (a list built without a tokenizer has not been checked against one)"""
        if int(self.child_token.max()) >= eot:
            raise ValueError("phrase token ids must lie in [0, <|endoftext|>) — no specials, no timestamps")

    # -- the specification: a walk over the dicts -------------------------------------------------------------------
    def step(self, state: int, token: int) -> int:
        """the state after `token` was chosen in `state`: the edge out of the state wins over the edge out of the root"""
        nxt = self.children[state].get(token)
        if nxt is not None:
            return nxt
        return self.children[0].get(token, 0)

    def walk(self, tokens: Sequence[int], state: int = 0) -> int:
        """the state after a row sampled `tokens` (from the root: its whole sampled part)"""
        for t in tokens:
            state = self.step(state, int(t))
        return state

    def boosted(self, state: int) -> Set[int]:
        """the tokens whose logit receives `boost` (once) at a step in `state`"""
        return set(self.children[state]) | set(self.children[0])

    # -- the same walk over the CSR arrays (what the device does) ---------------------------------------------------------
    def csr_child(self, state: int, token: int) -> int:
        lo, hi = int(self.child_begin[state]), int(self.child_begin[state + 1])
        i = lo + int(np.searchsorted(self.child_token[lo:hi], token))
        return int(self.child_node[i]) if i < hi and int(self.child_token[i]) == token else -1

    def csr_step(self, state: int, token: int) -> int:
        nxt = self.csr_child(state, token)
        if nxt < 0:
            nxt = self.csr_child(0, token)
        return max(nxt, 0)

    def csr_walk(self, tokens: Sequence[int], state: int = 0) -> int:
        for t in tokens:
            state = self.csr_step(state, int(t))
        return state

    # -- device copies, one per device -------------------------------------------------------------------------------------
    def device_arrays(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(child_begin, child_token, child_node) as int32 tensors on `device`, uploaded once and kept with the list"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        got = self._device.get(device)
        if got is None:
            got = tuple(torch.from_numpy(a).to(device) for a in (self.child_begin, self.child_token, self.child_node))
            self._device[device] = got
        return got

    def root_tokens(self, device) -> torch.Tensor:
        """the tokens that label an edge out of the root, int64 on `device` (`PhraseBias` boosts them in every row)"""
        device = torch.device(device)
        got = self._root_tokens.get(device)
        if got is None:
            got = torch.tensor(sorted(self.children[0]), dtype=torch.int64, device=device)
            self._root_tokens[device] = got
        return got

    def __len__(self) -> int:
        return len(self.phrases)

    def __repr__(self) -> str:
        return f"PhraseList({len(self.phrases)} phrases, {self.n_nodes} nodes, boost={self.boost})"


def as_phrase_list(phrases, tokenizer, boost: Optional[float] = None) -> Optional[PhraseList]:
    """None, a PhraseList (taken as it is; `boost` must then be left unset) or a plain list of phrases"""
    if phrases is None:
        if boost is not None:
            raise ValueError("phrase_boost without phrases")
        return None
    if isinstance(phrases, PhraseList):
        if boost is not None and float(boost) != phrases.boost:
            raise ValueError("phrase_boost given with a PhraseList, which carries its own boost")
        return phrases
    return PhraseList(phrases, DEFAULT_BOOST if boost is None else boost, tokenizer)
