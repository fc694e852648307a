"""Host-only references of whisper_amd/csrc/beam.hip.

  candidates()            float64 reference of beam_partial_kernel + beam_row_kernel: the filters of
                          oracle.decoding.apply_filters, log-softmax and the K best (log-probability, token) pairs.
  beam_update_model()     line-by-line model of beam_update_kernel, with every output the kernel writes.
  shared_history_step()   the lcp' / copy_from recurrence of the update kernel (one segment).
tests/test_host_logic.py holds both models to BeamSearchDecoder on the CPU; tests/test_beam_gpu.py holds the kernels to them."""
import numpy as np

LCP_START = 0x7F7F7F7F          # hipMemsetAsync(0x7f): "everything so far"


def filtered_float64(logits, history, r):
    """One row through SuppressBlank / SuppressTokens / ApplyTimestampRules (oracle.decoding.apply_filters, same order) in
    float64.  Returns the filtered row and what the "timestamp mass" rule saw: dict(fired, margin, n_ts) with margin =
    |logsumexp(timestamps) - max(text)| (inf when one side is empty) and n_ts = finite timestamp entries."""
    x = np.array(logits, dtype=np.float64)
    L, ninf = len(history), -np.inf
    info = dict(fired=False, margin=np.inf, n_ts=0)
    if r.suppress_blank and L == 0:
        x[[r.blank_token, r.eot]] = ninf
    if r.suppress_tokens:
        x[list(r.suppress_tokens)] = ninf
    TB = r.timestamp_begin
    if TB is None:
        return x, info
    if r.no_timestamps is not None:
        x[r.no_timestamps] = ninf
    last_ts = L >= 1 and history[-1] >= TB
    pen_ts = L < 2 or history[-2] >= TB
    if last_ts:
        if pen_ts:
            x[TB:] = ninf
        else:
            x[: r.eot] = ninf
    stamps = [t for t in history if t >= TB]
    if stamps:
        last = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
        x[TB:last] = ninf
    if L == 0:
        x[:TB] = ninf
        if r.max_initial_timestamp_index is not None:
            x[TB + r.max_initial_timestamp_index + 1:] = ninf
    ts, tx = x[TB:], x[:TB]
    ts_fin, tx_fin = ts[np.isfinite(ts)], tx[np.isfinite(tx)]
    info["n_ts"] = int(ts_fin.size)
    if ts_fin.size:
        m = ts_fin.max()
        ts_lse = m + np.log(np.exp(ts_fin - m).sum())       # a single timestamp: exactly its logit
        if tx_fin.size:
            info["fired"] = bool(ts_lse > tx_fin.max())     # the common normaliser cancels
            info["margin"] = float(abs(ts_lse - tx_fin.max()))
        else:
            info["fired"] = True
        if info["fired"]:
            x[:TB] = ninf
    return x, info


def candidates(logits, history, rules, K, with_info=False):
    """float64 reference of the first two kernels for one row: filters, log-softmax, then the K best entries ordered by
    value descending, id ascending; (-inf, 0) for the missing ones when fewer than K finite entries remain.
    Returns (tokens [K] int, logprobs [K] float64) and, with_info, the mass rule's dict plus `lse` = log(sum exp(x - max))."""
    x, info = filtered_float64(logits, history, rules)
    ids = np.flatnonzero(np.isfinite(x))
    tok, lp = np.zeros(K, dtype=np.int64), np.full(K, -np.inf)
    info["lse"] = 0.0
    if ids.size:
        v = x[ids]
        m = v.max()
        lse = np.log(np.exp(v - m).sum())
        order = np.argsort(-v, kind="stable")[:K]             # ids ascend, the sort is stable: ties keep the smaller id first
        n = order.size
        tok[:n], lp[:n] = ids[order], (v[order] - m) - lse
        info["lse"] = float(lse)
    return (tok, lp, info) if with_info else (tok, lp)


def shared_history_step(lcp, src, length, G):
    """The shared-history recurrence of beam_update_kernel for one segment.  lcp[i][j] (8 x 8): rows i and j hold identical
    K/V at their first lcp[i][j] cache positions; src[i]: the old row (segment-local) new row i continues, < 0 for a row
    that was not kept.  New row i takes from its source only the positions from lcp[i][src[i]] on, and new rows i, j share
    what their sources shared (everything so far for equal sources).  Returns (lcp', copy_from [G])."""
    new_lcp = [[0] * 8 for _ in range(8)]
    for i in range(G):
        for j in range(G):
            if src[i] >= 0 and src[j] >= 0:
                new_lcp[i][j] = min(length, length if src[i] == src[j] else lcp[src[i]][src[j]])
    copy_from = [0 if src[i] < 0 else min(length, length if src[i] == i else lcp[i][src[i]]) for i in range(G)]
    return new_lcp, copy_from


def beam_update_model(state, cand_lp, cand_tok, first, G, K, eot, max_candidates):
    """Line-by-line Python model of beam_update_kernel (whisper_amd/csrc/beam.hip): one segment per workgroup, fp32
    scores, rank = stable descending order, walk until G sequences are kept.  `state`: tokens [R][len], sums [R] fp32,
    fin (list of (sequence, score) per segment, in insertion order), done (flags of the previous update); optional:
    applied (updates applied so far) and lcp (per segment an 8 x 8 table; absent = the kernel's lcp == NULL).
    Returns (new state, src).  The new state also holds what else the kernel writes: step_tokens [R] (None = not written),
    fin_len (per segment, the length of every finished sequence), applied, and with lcp the new tables and copy_from [R]."""
    tokens, sums, fin, done_prev = state["tokens"], state["sums"], state["fin"], state["done"]
    B, R = len(fin), len(tokens)
    applied, lcp = state.get("applied", 0), state.get("lcp")
    if all(done_prev):                                   # completed: later updates leave everything untouched
        out = dict(tokens=[list(r) for r in tokens], sums=sums.copy(), fin=fin, done=[1] * B, step_tokens=[None] * R,
                   fin_len=[[len(s) for s, _ in f] for f in fin], applied=applied)
        if lcp is not None:
            out.update(lcp=lcp, copy_from=[0] * R)
        return out, list(range(R))
    new_tokens, new_sums, src, done_next = [None] * R, sums.copy(), [None] * R, [0] * B
    step_tokens, new_lcp, copy_from = [None] * R, [None] * B, [None] * R
    for au in range(B):
        r0, N = au * G, G * K
        score = np.full(N, np.nan, np.float32)
        ctok, csrc = np.zeros(N, int), np.zeros(N, int)
        for c in range(N):
            j, kk = divmod(c, K)
            if (j == G - 1) if first else True:          # first update: every beam holds the same prefix
                score[c] = np.float32(sums[r0 + j]) + np.float32(cand_lp[r0 + j][kk])
            ctok[c], csrc[c] = cand_tok[r0 + j][kk], r0 + j
        order = {}
        for c in range(N):
            if score[c] != score[c]:
                continue
            rank = sum(1 for o in range(N) if score[o] == score[o] and (score[o] > score[c] or (score[o] == score[c] and o < c)))
            order[rank] = c
        kept, newly = [], []
        for i in range(K if first else N):
            if len(kept) >= G:
                break
            c = order[i]
            (newly if ctok[c] == eot else kept).append(c)
        for c in newly:
            if len(fin[au]) >= max_candidates:
                break
            fin[au].append((tuple(tokens[csrc[c]]) + (eot,), float(score[c])))
        for b, c in enumerate(kept):
            new_tokens[r0 + b] = list(tokens[csrc[c]]) + [int(ctok[c])]
            src[r0 + b], new_sums[r0 + b] = int(csrc[c]), score[c]
            step_tokens[r0 + b] = int(ctok[c])
        if lcp is not None:
            local = [int(csrc[kept[b]]) - r0 if b < len(kept) else -1 for b in range(G)]
            new_lcp[au], copy_from[r0:r0 + G] = shared_history_step(lcp[au], local, len(tokens[r0]), G)
        done_next[au] = 1 if len(fin[au]) >= max_candidates else 0
    out = dict(tokens=new_tokens, sums=new_sums, fin=fin, done=done_next, step_tokens=step_tokens,
               fin_len=[[len(s) for s, _ in f] for f in fin], applied=applied + 1)
    if lcp is not None:
        out.update(lcp=new_lcp, copy_from=copy_from)
    return out, src
