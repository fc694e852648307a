"""Teacher-forced scoring on the GPU: the fused projection + log-sum-exp + target gather kernel (score.hip) against
float64, wh_task_score against the prefill route, whisper_amd.score against the oracle decoder, and chained shapes.

Error bound of a log-probability (derived, not tuned).  The kernel's logit is an fp32-accumulated dot product of values
that are exact in the element type: its error is at most 2^-20 * sum_k |w_vk x_k| (C_DOT of test_kernel_parity_gpu.py)
and, once held as an fp32 value, one ulp32 of its magnitude.  With E = 2^-20 * max_v sum_k |w_vk x_k| + ulp32(max |logit|)
per row, the picked logit is off by at most E and the log-sum-exp (a monotone, 1-Lipschitz function of the logits in the
max norm) by at most E: 2E.  On top comes the fp32 summation of the sum of exponentials, GAMMA = chain * 2^-24 relative
(= absolute in the logarithm), where chain is the longest sequence of dependent additions a term goes through:
    SLICE / 8 = 16 values per lane, 2 cross-lane steps, 1 across the two waves of a slice  (score.hip, SCORE_BN = 128)
    + one addition per slice in the merge kernel (ceil(v_end / SLICE) of them, in slice order).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import kernel_lib
import oracle
import score_oracle
import whisper_amd
from whisper_amd import hip
from whisper_amd.synthetic import dims_for, save_checkpoint, synthetic_state_dict
from whisper_amd.tokenizer import get_tokenizer

pytestmark = pytest.mark.gpu

F16, F32 = 1, 0
SLICE = 128                  # score.hip SCORE_BN: vocabulary columns per slice; checked against the library below
IN_SLICE_CHAIN = SLICE // 8 + 2 + 1
GUARD = 4096
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def gamma(v_end):
    return (IN_SLICE_CHAIN + (v_end + SLICE - 1) // SLICE) * 2.0 ** -24


def ulp32(x):
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def klib():
    h = kernel_lib.lib()
    if not getattr(h, "_score_ready", False):
        h.wht_score_slice.restype = _I
        h.wht_score_slice.argtypes = []
        h.wht_score_scratch_bytes.restype = ctypes.c_size_t
        h.wht_score_scratch_bytes.argtypes = [_L, _I]
        h.wht_score.restype = _I
        h.wht_score.argtypes = [_I, _P, _L, _P, _L, _P, _I, _I, _I, _I, _P, _P, _P, _P, ctypes.c_size_t, _P]
        h._score_ready = True
    return h


class Buf:
    """n elements inside 0xFF guard bytes; the payload starts poisoned (0xFF) as well."""

    def __init__(self, n, tdt):
        es = torch.empty((), dtype=tdt).element_size()
        self.g = GUARD // es
        self.raw = torch.empty((n + 2 * self.g,), dtype=tdt, device="cuda:0")
        self.raw.view(torch.uint8).fill_(0xFF)
        self.t = self.raw[self.g:self.g + n]

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        b = self.raw.view(torch.uint8)
        gb = self.g * self.raw.element_size()
        return bool((b[:gb] == 0xFF).all() and (b[len(b) - gb:] == 0xFF).all())


_CASES = {}


def _case(M, K, V, dtype):
    """seeded inputs rounded to the element type, their float64 logits and abs-sums: computed once per (shape, dtype)"""
    key = (M, K, V, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(0)
        tdt = torch.float16 if dtype == F16 else torch.float32
        x = torch.randn(M, K, generator=g).to(tdt)
        W = (torch.randn(V, K, generator=g) / math.sqrt(K)).to(tdt)
        logits = x.double() @ W.double().T
        abssum = x.double().abs() @ W.double().abs().T
        _CASES.clear()                      # one case resident at a time: W alone is 0.5 GB in float64
        _CASES[key] = (x, W, logits, abssum)
    return _CASES[key]


def _v_ends(V):
    out = [V]
    if 50257 < V:
        out.append(50257)                   # the text vocabulary of the multilingual models (timing.py's cut)
    out.append(((V // 2) // SLICE) * SLICE + 1)   # one past a slice boundary: the last slice holds one column
    return out


def _targets(M, v_end, rnd, g):
    """round `rnd` of the forced targets: first / last column of the first / last slice, v_end - 1, one >= v_end, one
    padded slot, dealt over the rows M at a time; remaining rows draw a random id below v_end"""
    last0 = ((v_end - 1) // SLICE) * SLICE
    special = [0, min(SLICE - 1, v_end - 1), last0, v_end - 1, v_end + 3, -1, max(0, last0 - 1)]
    t = torch.randint(0, v_end, (M,), generator=g, dtype=torch.int32)
    for m in range(M):
        i = rnd * M + m
        if i < len(special):
            t[m] = special[i]
    return t, (len(special) + M - 1) // M


SHAPES = [(1, 384, 51865), (17, 384, 51865), (40, 1280, 51866), (130, 64, 1000)]


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("M,K,V", SHAPES)
def test_kernel_against_float64(gpu_device, M, K, V, dtype):
    h = klib()
    assert h.wht_score_slice() == SLICE
    x, W, logits, abssum = _case(M, K, V, dtype)
    tdt = x.dtype
    bx, bW = Buf(M * K, tdt), Buf(V * K, tdt)
    bx.t.copy_(x.reshape(-1)); bW.t.copy_(W.reshape(-1))
    x_bits, W_bits = bx.raw.view(torch.uint8).clone(), bW.raw.view(torch.uint8).clone()
    nbytes = h.wht_score_scratch_bytes(M, V)
    assert nbytes == ((V + SLICE - 1) // SLICE) * M * 16
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    left_out = total = 0
    for v_end in _v_ends(V):
        E = 2.0 ** -20 * abssum[:, :v_end].max(1).values + ulp32(logits[:, :v_end].abs().max(1).values)
        bound = 2 * E + gamma(v_end)
        srt = logits[:, :v_end].topk(2, dim=1).values if v_end > 1 else None
        rnd, rounds = 0, 1
        while rnd < rounds:
            tgt, rounds = _targets(M, v_end, rnd, g)
            bt = Buf(M, torch.int32); bt.t.copy_(tgt)
            blp, btl, btt = Buf(M, torch.float32), Buf(M, torch.float32), Buf(M, torch.int32)
            bs = Buf(nbytes // 4, torch.float32)
            rc = h.wht_score(dtype, bx.ptr(), K, bW.ptr(), K, bt.ptr(), M, K, V, v_end, blp.ptr(), btl.ptr(), btt.ptr(),
                             bs.ptr(), nbytes, stream)
            assert rc == 0
            torch.cuda.synchronize()
            for b in (bx, bW, bt, blp, btl, btt, bs):
                assert b.guards_intact(), "write outside a buffer's payload"
            assert torch.equal(bt.t.cpu(), tgt)
            used = ((v_end + SLICE - 1) // SLICE) * M * 4
            assert bool((bs.t[used:].view(torch.uint8) == 0xFF).all()), "partials beyond the slices below v_end"
            lp, tl, tt = blp.t.cpu().double(), btl.t.cpu().double(), btt.t.cpu().long()
            rlp, rtl, rtt = score_oracle.score_rows(logits, tgt, v_end)
            pad, out = tgt < 0, tgt >= v_end
            live = ~pad & ~out
            err = (lp - rlp).abs()
            print(f"M={M} K={K} V={V} dtype={dtype} v_end={v_end} round={rnd}: max err {float(err[live].max()) if live.any() else 0:.3e}"
                  f" bound {float(bound.min()):.3e}..{float(bound.max()):.3e}")
            assert bool((err[live] <= bound[live]).all())
            assert bool(torch.isneginf(lp[out]).all())
            assert bool((lp[pad] == 0).all() and (tl[pad] == 0).all() and (tt[pad] == -1).all())
            assert bool(((tl - rtl).abs()[~pad] <= bound[~pad]).all())
            if srt is not None:
                sure = ((srt[:, 0] - srt[:, 1]) > 4 * E) & ~pad
                assert torch.equal(tt[sure], rtt[sure])
                left_out += int((~sure & ~pad).sum()); total += int((~pad).sum())
            else:
                assert bool((tt[~pad] == 0).all())
            # The bound is not vacuous.  (1) A log-sum that misses the DOMINANT column (about 1e-3 of the mass) is caught in
            # every row; a typical column holds 1 / V of the mass, 2e-5, which is below the bound: the bound detects a lost
            # dominant column (or a lost slice), not the loss of any single column.  (2) A target one id off is caught in
            # every row: neighbouring logits lie about 1 apart.
            top = logits[:, :v_end].argmax(1)
            cut = logits[:, :v_end].clone()
            cut[torch.arange(M), top] = -math.inf
            if v_end > 1 and live.any():
                wrong_sum = logits.gather(1, tgt.clamp(0, v_end - 1).long()[:, None])[:, 0] - torch.logsumexp(cut, 1)
                assert bool(((lp - wrong_sum).abs()[live] > bound[live]).all())
                shifted = torch.where(tgt > 0, tgt - 1, tgt + 1)
                wrong_tgt, _, _ = score_oracle.score_rows(logits, shifted, v_end)
                assert bool(((lp - wrong_tgt).abs()[live] > bound[live]).all())
            if rnd == 0:                    # the same inputs give the same bits
                b2 = [Buf(M, torch.float32), Buf(M, torch.float32), Buf(M, torch.int32)]
                assert h.wht_score(dtype, bx.ptr(), K, bW.ptr(), K, bt.ptr(), M, K, V, v_end, b2[0].ptr(), b2[1].ptr(),
                                   b2[2].ptr(), bs.ptr(), nbytes, stream) == 0
                torch.cuda.synchronize()
                for a, b in zip((blp, btl, btt), b2):
                    assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32))
            rnd += 1
    assert torch.equal(bx.raw.view(torch.uint8), x_bits) and torch.equal(bW.raw.view(torch.uint8), W_bits)
    assert left_out <= 0.05 * max(total, 1)


def test_kernel_refuses_bad_arguments(gpu_device):
    h = klib()
    x = torch.zeros(4, 64, dtype=torch.float16, device="cuda:0")
    W = torch.zeros(200, 64, dtype=torch.float16, device="cuda:0")
    t = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    o = torch.zeros(4, dtype=torch.float32, device="cuda:0")
    s = torch.zeros(4 * 2 * 4, dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def call(K=64, v_end=200, nbytes=s.numel() * 4):
        return h.wht_score(F16, x.data_ptr(), 64, W.data_ptr(), 64, t.data_ptr(), 4, K, 200, v_end, o.data_ptr(), None, None,
                           s.data_ptr(), nbytes, st)
    assert call() == 0
    assert call(K=32) == kernel_lib.hipErrorInvalidValue
    assert call(v_end=0) == kernel_lib.hipErrorInvalidValue
    assert call(v_end=201) == kernel_lib.hipErrorInvalidValue
    assert call(nbytes=64) == kernel_lib.hipErrorInvalidValue
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# the C ABI and the public function, on a dims_for("tiny")-sized synthetic checkpoint
# ---------------------------------------------------------------------------------------------------------------
# fp32 engine against the oracle: test_api_gpu.py:62 holds teacher-forced prefill logits to 1e-3 of the reference's; a
# log-probability is a difference of two logit-scale values (the picked logit and the log-sum-exp), hence twice that
TOL_VS_ORACLE = 2 * 1e-3


def _features(n, dims, seed):
    """encoder-output stand-ins with a per-clip offset (a random-init encoder maps every audio to nearly the same
    features), exact in fp16 so that both engines and the oracle see the same numbers"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, dims.n_audio_ctx, dims.n_audio_state, generator=g) * 0.5
    f += torch.randn(n, 1, dims.n_audio_state, generator=g)
    return f.half().float()


@pytest.fixture(scope="module")
def tiny(gpu_device, tmp_path_factory):
    dims = dims_for("tiny")
    sd = synthetic_state_dict(dims, seed=1)
    path = str(tmp_path_factory.mktemp("score") / "tiny.pt")
    save_checkpoint(path, dims, sd)
    model = whisper_amd.load_model(path, device=gpu_device)
    tok = get_tokenizer(True, num_languages=dims.n_vocab - 51765 - 1, language="en", task="transcribe")
    rng = np.random.default_rng(4)
    hyps = [[rng.integers(300, 40000, n).tolist() for n in pair] for pair in ((14, 9), (5, 12), (11, 3))]
    return dims, sd, model, tok, hyps, _features(3, dims, 7)


def _route_bound(dims, sd, logits, v_end):
    """The kernel test's bound 2E + GAMMA plus the logits' own fp32 ulp, per row of `logits` (the prefill route's fp32
    logits [rows][>= v_end], float64).  The hidden states do not cross the C ABI, so the dot-product term of E uses
    sum_k |w_vk x_k| <= |w_v| |x| (Cauchy-Schwarz) with |x| <= max|ln.weight| sqrt(D) + |ln.bias| for the final LayerNorm's
    output; the ulp terms come from the logits themselves."""
    W = sd["decoder.token_embedding.weight"].double()[:v_end]
    xnorm = (float(sd["decoder.ln.weight"].double().abs().max()) * math.sqrt(dims.n_text_state)
             + float(sd["decoder.ln.bias"].double().norm()))
    u = ulp32(logits[:, :v_end].abs().max(1).values)
    E = 2.0 ** -20 * float(W.norm(dim=1).max()) * xnorm + u
    return 2 * E + gamma(v_end) + u


def _rows(tok, hyps):
    init = list(tok.sot_sequence)
    rows = [init + h + [tok.eot] for pair in hyps for h in pair]
    n_tok = [len(r) for r in rows]
    T0 = max(n_tok)
    return init, [r + [tok.eot] * (T0 - len(r)) for r in rows], n_tok, T0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_abi_against_the_prefill_route(tiny, gpu_device, dtype):
    """3 clips x 2 hypotheses of different lengths.  6 rows x 18 tokens = 108 > 96 and 6 x 15 = 90 > 48 selected rows:
    wh_task_prefill then runs the same GEMM kernels up to the final LayerNorm (and its logits through gemm.hip), so the two
    routes see the same hidden states.  Bound: the kernel test's 2E + GAMMA plus the prefill logits' own fp32 ulp."""
    dims, sd, model, tok, hyps, feats = tiny
    eng = model.engine(dtype)
    init, rows, n_tok, T0 = _rows(tok, hyps)
    assert T0 == 18
    first = len(init) - 1
    n_out = T0 - 1 - first
    tokens = torch.tensor(rows, device=gpu_device)
    f = feats.to(gpu_device, dtype).contiguous()
    heads = ([0, 1, 3], [0, 2, 5])
    out = {}
    for route in ("score", "prefill"):
        task = hip.HipTask(eng, 3, 2, T0, capture_q=True)
        try:
            task.set_audio(f)
            if route == "score":
                res = task.score(tokens, n_tok, first)
            else:
                res = task.prefill(tokens, sel=list(range(first, T0 - 1)))
            out[route] = (res, task.position, task.cross_qk(3, heads[0], heads[1], 0, T0).cpu())
        finally:
            task.close()
    (lp, tl, tt), pos, qk = out["score"]
    logits, pos_ref, qk_ref = out["prefill"]
    assert pos == pos_ref == T0
    assert torch.equal(qk, qk_ref)
    target = torch.tensor([[r[p + 1] if p + 1 < n else -1 for p in range(first, T0 - 1)] for r, n in zip(rows, n_tok)])
    l64 = logits.cpu().double().reshape(6 * n_out, -1)
    want = score_oracle.score_rows(l64, target.reshape(-1), dims.n_vocab)
    bound = _route_bound(dims, sd, l64, dims.n_vocab)
    err = (lp.cpu().double().reshape(-1) - want[0]).abs()
    err_top = (tl.cpu().double().reshape(-1) - want[1]).abs()
    print(f"abi vs prefill route {dtype}: max err {float(err.max()):.3e} / top {float(err_top.max()):.3e}, "
          f"bound {float(bound.min()):.3e}..{float(bound.max()):.3e}")
    assert bool((err <= bound).all()) and bool((err_top <= bound).all())
    assert torch.equal(tt.cpu().long().reshape(-1), want[2])      # the same logits bit for bit unless a tie is rounded apart
    assert int((target < 0).sum()) > 0 and bool((lp.cpu()[target < 0] == 0).all())


def test_abi_statuses(tiny, gpu_device):
    dims, sd, model, tok, hyps, feats = tiny
    eng = model.engine(torch.float32)
    task = hip.HipTask(eng, 1, 1, 8)
    L = hip.lib()
    try:
        task.set_audio(feats[:1].to(gpu_device).contiguous())
        tokens = torch.tensor([list(tok.sot_sequence) + [500, 600, tok.eot]], device=gpu_device)
        T0 = tokens.shape[1]
        o = torch.zeros(8, device=gpu_device)
        s = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu_device)

        def call(n=T0, first=2, v_end=dims.n_vocab, nbytes=s.numel()):
            arr = (ctypes.c_int32 * 1)(n)
            return L.wh_task_score(task.handle, tokens.data_ptr(), T0, T0, arr, first, v_end, o.data_ptr(), None, None,
                                   s.data_ptr(), nbytes, hip.stream_ptr(task.stream))
        assert call(first=-1) == 1 and call(first=T0 - 1) == 1 and call(v_end=0) == 1 and call(v_end=dims.n_vocab + 1) == 1
        assert call(n=0) == 1 and call(n=T0 + 1) == 1
        assert call(nbytes=256) == 2                                  # WH_ERR_WORKSPACE
        task.set_lag([1])
        assert call() == 4 and task.position == 0                     # WH_ERR_STATE: ragged prompts are not scored
        task.set_lag(None)
        # a begun loop is pending: refused until wh_task_poll has reported its end
        mask = torch.zeros(dims.n_vocab, dtype=torch.uint8, device=gpu_device)
        p = hip.GreedyParams(sample_begin=3, max_steps=4, n_ctx=dims.n_text_ctx, eot=tok.eot, timestamp_begin=tok.timestamp_begin,
                             no_timestamps=tok.no_timestamps, max_initial_timestamp_index=50, suppress_blank=1,
                             blank_token=tok.encode(" ")[0], suppress_mask=mask.data_ptr())
        loop_tokens = torch.zeros(1, 3 + 4 + 1, dtype=torch.int64, device=gpu_device)
        loop_tokens[0, :3] = torch.tensor(list(tok.sot_sequence), device=gpu_device)
        pend = task.greedy_begin(loop_tokens, p, 0, -1)
        refused = call()
        assert pend.wait() is not None
        assert refused == 4                                           # WH_ERR_STATE
        task.reset()
        assert L.wh_score_scratch_bytes(eng.handle, 1, T0 - 3) <= s.numel()
        assert call() == 0 and task.position == T0
    finally:
        task.close()


def test_score_against_the_oracle_decoder(tiny, gpu_device):
    dims, sd, model, tok, hyps, feats = tiny
    opts = whisper_amd.DecodingOptions(language="en", fp16=False)
    f = feats.to(gpu_device)
    got = whisper_amd.score(model, f, hyps, opts)
    om = oracle.OracleModel(dims, sd)
    init = list(tok.sot_sequence)
    want = score_oracle.score_hypotheses(om, feats, [init] * 3, hyps, tok.eot)
    worst = 0.0
    for b in range(3):
        for g, w in zip(got[b], want[b]):
            assert g.tokens == w["tokens"] and len(g.token_logprobs) == len(g.tokens) + 1 and g.language == "en"
            d = (torch.tensor(g.token_logprobs, dtype=torch.float64) - w["token_logprobs"]).abs().max().item()
            worst = max(worst, d)
            assert abs(g.sum_logprob - sum(g.token_logprobs)) < 1e-9
            assert g.avg_logprob == g.sum_logprob / (len(g.tokens) + 1)
            assert g.top_tokens == w["top_tokens"].tolist()
        assert (got[b][0].sum_logprob > got[b][1].sum_logprob) == (want[b][0]["sum_logprob"] > want[b][1]["sum_logprob"])
    print(f"score vs oracle decoder: max per-token err {worst:.3e} (tolerance {TOL_VS_ORACLE:.1e})")
    assert worst <= TOL_VS_ORACLE

    # strings and id lists give the same result; a flat list is one hypothesis
    text = "hello world"
    ids = tok.encode(" " + text)
    a = whisper_amd.score(model, f[:1], [[text]], opts)[0][0]
    b = whisper_amd.score(model, f[:1], [ids], opts)[0][0]
    assert a == b and a.tokens == ids

    # vocabulary="text" is timing.py's convention: log of _token_probs on the prefill logits of the same rows
    from whisper_amd.timing import _token_probs
    txt = whisper_amd.score(model, f, hyps, opts, vocabulary="text")
    _, rows, n_tok, T0 = _rows(tok, hyps)
    task = hip.HipTask(model.engine(torch.float32), 3, 2, T0)
    try:
        task.set_audio(f.contiguous())
        logits = task.prefill(torch.tensor(rows, device=gpu_device), sel=list(range(len(init) - 1, T0 - 2)))
    finally:
        task.close()
    r = 0
    for b in range(3):
        for h, g in zip(hyps[b], txt[b]):
            assert len(g.token_logprobs) == len(h)                    # the closing <|endoftext|> is not scored
            l64 = logits[r, :len(h)].double()
            p = _token_probs(l64[None], torch.tensor([h], device=gpu_device), tok.eot)[0].log().cpu()
            bound = _route_bound(dims, sd, l64.cpu(), tok.eot)
            assert bool(((torch.tensor(g.token_logprobs, dtype=torch.float64) - p).abs() <= bound).all())
            r += 1


def test_small_shape_agrees_with_the_few_row_prefill(tiny, gpu_device):
    """1 row x 12 tokens: wh_task_prefill runs its few-row kernels here, wh_task_score the GEMM form (include/whisper_hip.h:
    equal within rounding, not bitwise).  fp32 engine: each route is within TOL_VS_ORACLE of the oracle (the tolerance of
    test_score_against_the_oracle_decoder), so the two are within twice that of each other; the position is the same."""
    dims, sd, model, tok, hyps, feats = tiny
    eng = model.engine(torch.float32)
    row = list(tok.sot_sequence) + hyps[0][1][:8] + [tok.eot]
    tokens = torch.tensor([row], device=gpu_device)
    T0, first = len(row), 2
    f = feats[:1].to(gpu_device).contiguous()
    out = {}
    for route in ("score", "prefill"):
        task = hip.HipTask(eng, 1, 1, T0)
        try:
            task.set_audio(f)
            res = task.score(tokens, [T0], first)[0] if route == "score" else task.prefill(tokens, sel=list(range(first, T0 - 1)))
            out[route] = (res.cpu().double(), task.position)
        finally:
            task.close()
    want = score_oracle.score_rows(out["prefill"][0][0], torch.tensor(row[first + 1:]), dims.n_vocab)[0]
    err = (out["score"][0][0] - want).abs().max().item()
    print(f"small shape, GEMM form vs few-row prefill: max err {err:.3e}")
    assert out["score"][1] == out["prefill"][1] == T0
    assert err <= 2 * TOL_VS_ORACLE


def test_prompts_prefix_and_detected_language(tiny, gpu_device):
    """Per-clip prompts of different lengths (one clip without), a prefix, language=None: the rows of a chain then start their
    scored region at different positions (`first` is the chain's minimum).  Against the oracle decoder on hand-built initial
    tokens [<|startofprev|>, prompt, <|startoftranscript|>, detected language, <|transcribe|>, prefix], and bit-equal (fp32) to
    every clip scored alone with its prompt and language given in the options."""
    dims, sd, model, tok, hyps, feats = tiny
    f = feats.to(gpu_device)
    prompts = [[1000, 2000, 3000], None, [400]]
    prefix = [600, 700]
    opts = whisper_amd.DecodingOptions(language=None, fp16=False, prefix=prefix)
    got = whisper_amd.score(model, f, hyps, opts, prompts=prompts)
    _, lang_probs = model.detect_language(f)
    om = oracle.OracleModel(dims, sd)
    inits = []
    for b in range(3):
        lang = max(lang_probs[b], key=lang_probs[b].get)
        assert all(g.language == lang for g in got[b])
        sot = [tok.sot, tok.to_language_token(lang), tok.transcribe]
        inits.append(([tok.sot_prev] + prompts[b] if prompts[b] else []) + sot + prefix)
    assert len({len(i) for i in inits}) == 3
    want = score_oracle.score_hypotheses(om, feats, inits, hyps, tok.eot)
    for b in range(3):
        for g, w in zip(got[b], want[b]):
            assert len(g.token_logprobs) == len(g.tokens) + 1
            assert (torch.tensor(g.token_logprobs, dtype=torch.float64) - w["token_logprobs"]).abs().max().item() <= TOL_VS_ORACLE
            assert g.top_tokens == w["top_tokens"].tolist()
        alone = whisper_amd.score(model, f[b:b + 1], [hyps[b]], whisper_amd.DecodingOptions(
            language=got[b][0].language, fp16=False, prefix=prefix, prompt=prompts[b]))
        assert alone[0] == got[b]


def test_greedy_transcript_outscores_a_one_token_edit(gpu_device, tmp_path):
    """On the margin-conditioned checkpoint of oracle/condition.py (without_timestamps; every id >= <|endoftext|> suppressed,
    so the transcript is text only) the oracle's greedy token beats every other admissible token by >= 0.3 in the logits.
    Replacing the LAST token by that step's runner-up therefore costs the sum that margin: under vocabulary="text" the
    closing <|endoftext|>, the only later position, is not scored, and both tokens share the step's log-sum.  0.3 is far above
    the fp32 engine's 2e-3."""
    from oracle import condition
    dims = dims_for("tiny")
    sd = synthetic_state_dict(dims, seed=0)
    tok = get_tokenizer(True, num_languages=dims.n_vocab - 51765 - 1, language="en", task="transcribe")
    init = list(tok.sot_sequence_including_notimestamps)
    suppress = sorted(set(list(tok.non_speech_tokens) + list(range(tok.eot, dims.n_vocab))))
    rules = oracle.SamplingRules(sample_begin=len(init), sot_index=0, eot=tok.eot, n_ctx=dims.n_text_ctx, timestamp_begin=None,
                                 no_timestamps=None, suppress_tokens=suppress, blank_token=tok.encode(" ")[0],
                                 no_speech=tok.no_speech)
    om = oracle.OracleModel(dims, sd)
    feats = _features(1, dims, 11)
    n_steps = 8
    with torch.no_grad():
        condition.condition_greedy(om, feats, init, n_steps, rules, seed=5, margin=(0.35, 3.0), passes=2)
        dec = oracle.decoding.greedy_decode(om, feats, init, n_steps, rules, keep_logits=True)
    margin = condition.margins_of(dec)["min"]
    assert margin >= 0.3
    best = dec["tokens"][0, len(init):].tolist()
    runner = int(dec["step_logits"][-1][0].float().topk(2).indices[1])
    assert len(best) == n_steps and max(best) < tok.eot and runner < tok.eot and runner != best[-1]
    edited = best[:-1] + [runner]
    path = str(tmp_path / "conditioned.pt")
    save_checkpoint(path, dims, om.sd)
    model = whisper_amd.load_model(path, device=gpu_device)
    res = whisper_amd.score(model, feats.to(gpu_device), [[best, edited]],
                            whisper_amd.DecodingOptions(language="en", fp16=False, without_timestamps=True), vocabulary="text")[0]
    print("greedy", res[0].sum_logprob, "edited", res[1].sum_logprob, "oracle margin", margin)
    assert math.isfinite(res[1].sum_logprob)
    assert res[0].sum_logprob > res[1].sum_logprob + 0.3 - 2 * TOL_VS_ORACLE


def test_chained_shapes_equal_scoring_alone(tiny, gpu_device):
    """5 clips with 1, 3, 1 (of length 0), 2, 1 hypotheses, batch_rows=4: n_group = 3, one clip per chain, filler rows;
    every (clip, hypothesis) must come out as when it is scored alone — to the last bit in the fp32 engine"""
    dims, sd, model, tok, hyps, _ = tiny
    rng = np.random.default_rng(9)
    H = [[rng.integers(300, 40000, n).tolist() for n in ns] for ns in ((6,), (2, 9, 4), (0,), (7, 1), (5,))]
    f = _features(5, dims, 21).to(gpu_device)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False)
    got = whisper_amd.score(model, f, H, opts, batch_rows=4)
    assert [len(g) for g in got] == [1, 3, 1, 2, 1]
    assert got[2][0].tokens == [] and len(got[2][0].token_logprobs) == 1         # only the closing <|endoftext|>
    for b in range(5):
        for i, h in enumerate(H[b]):
            alone = whisper_amd.score(model, f[b:b + 1], [[h]], opts)[0][0]
            assert alone == got[b][i], (b, i)
    with pytest.raises(ValueError):
        whisper_amd.score(model, f, H[:4], opts)
