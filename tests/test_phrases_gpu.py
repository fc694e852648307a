"""Phrase lists on the GPU: the biased sampler kernels against float64, wh_task_greedy + wh_task_set_phrases against the
CPU oracle, forced walks, the loop's lifecycle, and the Python interface (whisper_amd/phrases.py states the semantics).

Error bound of a step's log-probability in the kernel test (derived, not tuned).  The inputs lie on a dyadic grid
(multiples of 2^-6, |x| < 64, the boost as well): x + boost, the differences x - max and the arg-max are exact in fp32, so
the token and the new trie node must equal float64's exactly, and all the error is in log(sum exp(x - max)):
  * every term is one expf (<= 1 ulp by the device library's table; taken as 2 ulp = 2^-22 relative) and every step of the
    reduction a term goes through is one online-softmax merge `s * expf(m - m') + s'`: one more expf (2^-22) and two fp32
    roundings (2 * 2^-24), i.e. at most 6 * 2^-24 relative per step;
  * the longest chain of dependent merges (sampling.hip): 4 entries per thread, 6 cross-lane steps, 4 waves in the partial
    kernel; ceil(nchunk / 256) partials per thread, 6 cross-lane steps, 4 waves, and the text / timestamp halves joined
    (2) in the final kernel: CHAIN = 26 + ceil(nchunk / 256);
  * a relative error of the sum is an absolute error of its logarithm: GAMMA = (CHAIN + 1) * 6 * 2^-24 (+ 1: the terms);
  * logf (<= 1 ulp, taken as 2), the subtraction that forms the log-probability when sampling, and the addition to the
    running sum: 3 ulp32(|logprob|) + ulp32(|sum|).
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_lib  # noqa: E402
import oracle  # noqa: E402
import phrase_oracle  # noqa: E402
import whisper_amd  # noqa: E402
from oracle.decoding import SamplingRules  # noqa: E402
from whisper_amd import hip  # noqa: E402
from whisper_amd.phrases import PhraseList  # noqa: E402
from whisper_amd.synthetic import dims_for, save_checkpoint, synthetic_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

SCHUNK = 1024                # sampling.hip: vocabulary entries per stage-1 workgroup
GUARD = 4096
_P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float


def gamma(V):
    nchunk = (V + SCHUNK - 1) // SCHUNK
    return (26 + (nchunk + 255) // 256 + 1) * 6 * 2.0 ** -24


def ulp32(x):
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def klib():
    h = kernel_lib.lib()
    if not getattr(h, "_phrases_ready", False):
        h.wht_greedy_sample.restype = _I
        h.wht_greedy_sample.argtypes = [_P, _L, _I, _I, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P,
                                        ctypes.c_size_t, _F, ctypes.c_uint64, _P, _I, _I, _P, _P, _P, _P, _P, _F, _P]
        h.wht_greedy_sample_scratch_bytes.restype = ctypes.c_size_t
        h.wht_greedy_sample_scratch_bytes.argtypes = [_I, _I]
        h.wht_phrase_root_table.restype = _I
        h.wht_phrase_root_table.argtypes = [_P, _P, _P, _I, _I, _P, _P]
        h._phrases_ready = True
    return h


class Buf:
    """a host array on the device inside 0xA5 guard bytes"""

    def __init__(self, arr: np.ndarray):
        self.n = arr.nbytes
        self.raw = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.raw[GUARD:GUARD + self.n] = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to("cuda:0")
        self.dtype, self.shape = arr.dtype, arr.shape

    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def get(self) -> np.ndarray:
        return self.raw[GUARD:GUARD + self.n].cpu().numpy().view(self.dtype).reshape(self.shape).copy()

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all() and (self.raw[GUARD + self.n:] == 0xA5).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the two sampler kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
def _rules(V, with_ts=True, suppress=()):
    eot, no_ts = (50257, 50364) if V > 51000 else (V - 200, V - 151)
    return SamplingRules(sample_begin=2, sot_index=0, eot=eot, n_ctx=448, timestamp_begin=no_ts + 1 if with_ts else None,
                         no_timestamps=no_ts, max_initial_timestamp_index=50, suppress_blank=True, blank_token=220,
                         suppress_tokens=sorted(suppress))


def _trie(V):
    """root children {10, 20, 40, 50, 60}; node(10) = {11, 20} (20 is a root child too); node(10 11) = {12} and node(40) = {41}
    and node(20) = {30}: fan-out 1; node(40 41): a leaf; node(50): fan-out 64, across the 1024-entry chunk boundary where the
    vocabulary allows it; node(60): fan-out 300 (more than one round of 256 in the final kernel)"""
    wide = list(range(990, 1054)) if V > 51000 else list(range(300, 364))
    phrases = [[10, 11, 12], [10, 20], [20, 30], [40, 41]] + [[50, t] for t in wide] + [[60, t] for t in range(400, 700)]
    return phrase_oracle.Trie(phrases), wide


# scenario -> (state as a token path, token planted to win WITH the boost (None: none), a rival planted 1.5 boosts above it)
def _scenarios(wide):
    return [
        ((), 20, False),                 # root: a phrase starts
        ((10, 11), 12, False),           # inner node, fan-out 1
        ((50,), wide[34], False),        # fan-out 64: id 1024, the first entry of the second chunk, in the large vocabulary
        ((50,), wide[33], False),        # ... and id 1023, the last entry of the first
        ((40, 41), 10, False),           # leaf: only the root's edges are boosted
        ((10,), 20, True),               # 20 is a child of the node AND of the root: boosted once, the rival wins
        ((40,), 41, False),              # 41 is in the suppress mask: it stays masked
        ((60,), 699, False),             # fan-out 300, the last child
        ((20,), None, False),            # nothing planted: an unlisted token wins, the node returns to the root
        ((10,), 40, False),              # not a child of the node but of the root: re-entry
    ]


def _case(V, R, mode, seed=0):
    """inputs of one launch and what float64 expects; everything on the host"""
    rng = np.random.default_rng(1000 * seed + V + R)
    trie, wide = _trie(V)
    with_ts = mode != "nots"
    r = _rules(V, with_ts, suppress=(41, 5, 7))
    boost = -16.0 if mode == "neg" else 16.0
    TB = r.timestamp_begin
    scen = _scenarios(wide)
    x = (rng.integers(-4095, 4096, (R, V)) / 64.0).astype(np.float32)          # multiples of 2^-6, |x| < 64
    x = np.minimum(x, 40.0).astype(np.float32)                                  # room above for the planted entries
    listed = sorted({t for kids in trie.children for t in kids})
    x[:, listed] = np.minimum(x[:, listed], 20.0)                               # ... also once a listed token is boosted
    lag = [(3 * i) % 4 for i in range(R)] if mode == "lag" else [0] * R
    T0 = 6                                                                      # the longest row's sample_begin
    rows, states, sums, ended = [], [], [], []
    for i in range(R):
        path, plant, rival = scen[(i + seed) % len(scen)]
        # (the rows of a step share one position counter: every row has sampled the same number of tokens)
        at_eot = mode == "mid" and i % 7 == 6
        if mode == "first":
            sampled = []
        elif not with_ts:
            sampled = [100, 101, 102]
        elif at_eot:
            sampled = [TB + 3, 100, r.eot]
        else:
            sampled = [[TB + 3, 100, 101], [TB + 3, 100, TB + 9], [TB + 3, TB + 3, 100], [100, TB + 1, TB + 1]][i % 4]
        state = trie.walk(path)
        if plant is not None:
            # with the boost the planted token is the row's best by one grid step; without it far from it
            x[i, plant] = (50.0 - boost) if boost > 0 else 50.0
            if boost < 0:
                x[i, 3] = 50.0 + boost + 1 / 64                                  # the unlisted id 3 wins once 16 are taken off
            if rival:
                x[i, 3] = x[i, plant] + 1.5 * boost
        rows.append([50258] * (T0 - lag[i]) + sampled)
        states.append(0 if mode == "first" else state)
        sums.append(float(rng.integers(-64, 1)) / 4)
        ended.append(at_eot)
    n_tok = [len(row) for row in rows]
    ntok = max(n + g for n, g in zip(n_tok, lag))
    assert all(n + g == ntok for n, g in zip(n_tok, lag)), "rows of one step share the common position counter"
    want = []
    for i in range(R):
        sampled = rows[i][T0 - lag[i]:]
        rr = SamplingRules(**{**r.__dict__, "sample_begin": T0 - lag[i]})
        tok, lp, ns, xf = phrase_oracle.sampler_step(x[i], sampled, states[i], trie, boost, rr, ended=ended[i])
        plain = phrase_oracle.sampler_step(x[i], sampled, 0, phrase_oracle.Trie([]), boost, rr, ended=ended[i])[0]
        want.append(dict(tok=tok, lp=lp, state=ns, plain=plain))
    return dict(x=x, rows=rows, lag=lag, T0=T0, ntok=ntok, states=states, sums=sums, r=r, trie=trie, boost=boost, want=want,
                with_ts=with_ts)


def _launch(case, V, R, temperature=0.0, seed=0):
    h = klib()
    r, x = case["r"], case["x"]
    TB = r.timestamp_begin if case["with_ts"] else -1
    stride = case["ntok"] + 3
    tokens = np.full((R, stride), -7, dtype=np.int64)
    rs = np.zeros((R, 4), dtype=np.int32)
    for i, row in enumerate(case["rows"]):
        tokens[i, : len(row)] = row
        sampled = row[case["T0"] - case["lag"][i]:]
        if case["with_ts"]:
            stamps = [t for t in sampled if t >= TB]
            rs[i, 0] = int(len(sampled) >= 1 and sampled[-1] >= TB)
            rs[i, 1] = int(len(sampled) >= 2 and sampled[-2] >= TB)
            rs[i, 2] = stamps[-1] + 1 if stamps else 0
        rs[i, 3] = case["states"][i]
    begin, token, node = case["trie"].csr()
    mask = np.zeros(V, dtype=np.uint8)
    mask[list(r.suppress_tokens)] = 1
    nbytes = h.wht_greedy_sample_scratch_bytes(R, V)
    b = dict(x=Buf(x), tokens=Buf(tokens), ntok=Buf(np.array([case["ntok"]], np.int32)), lag=Buf(np.array(case["lag"], np.int32)),
             mask=Buf(mask), sums=Buf(np.array(case["sums"], np.float32)), step=Buf(np.full(R, -7, np.int64)),
             alive=Buf(np.array([-5], np.int32)), part=Buf(np.zeros(nbytes // 4, np.float32)), rs=Buf(rs), begin=Buf(begin),
             token=Buf(token), node=Buf(node), root=Buf(np.full(V, 77, np.int32)), span=Buf(np.full((R, 2), 77, np.int32)))
    assert h.wht_phrase_root_table(b["begin"].ptr(), b["token"].ptr(), b["node"].ptr(), len(token), V, b["root"].ptr(), None) == 0
    rc = h.wht_greedy_sample(b["x"].ptr(), V, R, V, b["tokens"].ptr(), stride, b["ntok"].ptr(),
                             b["lag"].ptr() if any(case["lag"]) else None, case["T0"], r.eot, TB, r.no_timestamps,
                             r.max_initial_timestamp_index, 1, r.blank_token, b["mask"].ptr(), b["sums"].ptr(), b["step"].ptr(),
                             b["alive"].ptr(), b["part"].ptr(), nbytes, temperature, seed, b["rs"].ptr(), len(begin) - 1,
                             len(token), b["begin"].ptr(), b["token"].ptr(), b["node"].ptr(), b["root"].ptr(), b["span"].ptr(),
                             case["boost"], None)
    assert rc == 0
    torch.cuda.synchronize()
    for name, buf in b.items():
        assert buf.guards_intact(), name
    assert np.array_equal(b["x"].get().view(np.uint32), x.view(np.uint32)), "the logits buffer must not be written"
    root = b["root"].get()
    kids = case["trie"].children[0]
    assert all(root[t] == kids.get(t, -1) for t in list(kids) + [0, 1, V - 1]) and (root >= 0).sum() == len(kids)
    return {k: v.get() for k, v in b.items()}, rs, begin


@pytest.mark.parametrize("mode", ["mid", "first", "nots", "neg", "lag"])
@pytest.mark.parametrize("R", [1, 3, 24])
@pytest.mark.parametrize("V", [1000, 1025, 51866])
def test_sampler_kernels_against_float64(gpu_device, V, R, mode):
    """greedy_partial_kernel / greedy_final_kernel <false, true> through wht_greedy_sample: rows put into chosen trie nodes
    (root, fan-out 1 / 64 across a chunk boundary / 300, leaf, a token that is a child of the node and of the root, a boosted
    token in the suppress mask, re-entry from the root, an unlisted winner), with the timestamp rules at L >= 1 (`mid`, some
    rows already at <|endoftext|>), at L == 0 (`first`), off (`nots`), a negative boost and ragged rows.  Token and new node
    exact, the log-probability within the bound of the module docstring, the timestamp-rule state as before, guard bytes
    intact, logits untouched."""
    biased_differs = 0
    for seed in range((10 + R - 1) // R):                 # every scenario at every R
        case = _case(V, R, mode, seed)
        out, rs0, begin = _launch(case, V, R)
        TB = case["r"].timestamp_begin
        for i, w in enumerate(case["want"]):
            n = len(case["rows"][i])
            assert out["tokens"][i, n] == w["tok"] == out["step"][i], (i, out["tokens"][i, n], w)
            assert out["tokens"][i, n + 1] == -7 and list(out["tokens"][i, :n]) == case["rows"][i]
            assert out["rs"][i, 3] == w["state"], (i, out["rs"][i], w)
            s = w["state"]
            assert list(out["span"][i]) == ([begin[s], begin[s + 1]] if s else [0, 0])
            if case["with_ts"]:
                is_ts = w["tok"] >= TB
                assert list(out["rs"][i, :3]) == [int(is_ts), rs0[i, 0], w["tok"] + 1 if is_ts else rs0[i, 2]]
            else:
                assert list(out["rs"][i, :3]) == [0, 0, 0]
            if w["lp"] is None:                            # the row had ended: nothing accumulated, bit for bit
                assert out["sums"][i] == np.float32(case["sums"][i]) and w["tok"] == case["r"].eot and w["state"] == 0
            else:
                total = case["sums"][i] + w["lp"]
                bound = gamma(V) + 3 * ulp32(w["lp"]) + ulp32(total)
                assert abs(float(out["sums"][i]) - total) <= bound, (i, float(out["sums"][i]), total, bound)
            if mode == "first":
                assert w["tok"] >= TB                      # no boosted text token is chosen as the first token
            biased_differs += w["tok"] != w["plain"]
    if mode != "first":
        assert biased_differs >= 5                         # the bias did decide tokens: a kernel that ignored it fails above


def test_sampling_instantiation_draws_the_forced_token(gpu_device):
    """<true, true>: temperature 1, boost 48 on a one-phrase list.  The 23-bit uniform lies in [2^-24, 1 - 2^-24]
    (sample_noise.h), so the Gumbel noise -log(-log u) lies in [-2.81, 16.64]: a range of 19.5, for which 20.2 (17.33 + 2.86
    below) is an upper bound; the logits are drawn with |x| < 12: a range of 24; 48 / T = 48 > 44.2, so the boosted token's
    key exceeds every other key whatever the noise and it is drawn with certainty.  Its log-probability is the unscaled
    x + 48 - log-sum-exp of the biased row."""
    V, R, a = 51866, 24, 1234
    rng = np.random.default_rng(5)
    trie = phrase_oracle.Trie([[a]])
    r = _rules(V, with_ts=False)
    x = (rng.integers(-767, 768, (R, V)) / 64.0).astype(np.float32)
    assert 48.0 > (17.33 + 2.86) + (x.max() - x.min())
    case = dict(x=x, rows=[[50258] * 6 + [100]] * R, lag=[0] * R, T0=6, ntok=7, states=[0] * R, sums=[0.0] * R, r=r,
                trie=trie, boost=48.0, with_ts=False)
    out, _, _ = _launch(case, V, R, temperature=1.0, seed=0x1234567890)
    for i in range(R):
        xb = x[i].astype(np.float64)
        xb[a] += 48.0
        m = xb.max()
        lp = xb[a] - m - math.log(np.exp(xb - m).sum())
        assert out["tokens"][i, 7] == a and out["rs"][i, 3] == 1
        assert abs(float(out["sums"][i]) - lp) <= gamma(V) + 4 * ulp32(lp) + 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. the device-side loop through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro(gpu_device):
    dims = oracle.dims_for("micro.en")
    sd = oracle.synthetic_state_dict(dims, seed=1)
    om = oracle.OracleModel(dims, sd)
    models = {dt: hip.HipModel(dims, dt, hip.pack_weights(sd, dims, dt, gpu_device)) for dt in (hip.WH_F32, hip.WH_F16)}
    return dims, om, models


def _loop_rules(dims, T0, with_ts=True):
    """the rules tests/test_kernels_gpu.py decodes the micro model with"""
    eot = 50256
    sot = eot + 1
    transcribe = sot + 1 + (dims.n_vocab - 51765) + 1
    no_speech = transcribe + 3
    no_ts = no_speech + 1
    rng = np.random.default_rng(0)
    suppress = sorted(set(rng.integers(0, 50000, 80).tolist() + [sot, transcribe, transcribe - 1, no_speech]))
    return SamplingRules(sample_begin=T0, sot_index=0, eot=eot, n_ctx=dims.n_text_ctx,
                         timestamp_begin=(no_ts + 1) if with_ts else None, no_timestamps=no_ts,
                         max_initial_timestamp_index=50, suppress_blank=True, blank_token=220, suppress_tokens=suppress,
                         no_speech=no_speech)


def _params(r, n_steps, mask, dims, temperature=0.0, seed=0):
    p = hip.GreedyParams(sample_begin=r.sample_begin, max_steps=n_steps, n_ctx=dims.n_text_ctx, eot=r.eot,
                         timestamp_begin=r.timestamp_begin if r.timestamp_begin is not None else -1,
                         no_timestamps=r.no_timestamps, max_initial_timestamp_index=50, suppress_blank=1, blank_token=220,
                         suppress_mask=mask.data_ptr())
    p.temperature, p.seed = temperature, seed
    return p


def _mask(r, dims, dev):
    m = torch.zeros(dims.n_vocab, dtype=torch.uint8)
    m[list(r.suppress_tokens)] = 1
    return m.to(dev)


def _feats(dims, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, dims.n_audio_ctx, dims.n_audio_state, generator=g)


def _six_phrases(r):
    rng = np.random.default_rng(0)
    ok = [t for t in range(1000, 50000) if t not in set(r.suppress_tokens) and t != 220]
    a = rng.choice(ok, 8, replace=False).tolist()
    return [[a[0], a[1], a[2]], [a[0], a[1], a[3]], [a[0], a[4]], [a[5]], [a[5], a[6], a[0]], [a[1], a[7]]]


def _run_greedy(task, dev, init, r, dims, n_steps, B, phrases=None, boost=0.0, begin=False, temperature=0.0, seed=0):
    tokens = torch.zeros(B, len(init) + n_steps + 1, dtype=torch.int64, device=dev)
    tokens[:, : len(init)] = torch.tensor(init)
    mask = _mask(r, dims, dev)
    p = _params(r, n_steps, mask, dims, temperature, seed)
    if phrases is not None:
        task.set_phrases(PhraseList(phrases, boost=boost).device_arrays(dev), boost)
    if begin:
        pend = task.greedy_begin(tokens, p, 0, -1)
        res = None
        while res is None:
            res = pend.poll()
        n, lp, _ = res
    else:
        n, lp, _ = task.greedy(tokens, p, 0, -1)
    torch.cuda.synchronize()
    return tokens[:, :n].cpu(), lp.cpu()


@pytest.mark.parametrize("with_ts", [True, False])
def test_task_greedy_with_phrases_against_the_oracle(micro, gpu_device, with_ts):
    """wh_task_set_phrases + wh_task_greedy, fp32 strict engine, 3 rows x 40 steps, against phrase_oracle's biased decode:
    token ids exact, sum_logprobs within 2e-3 (the bound of test_kernels_gpu.py::test_fused_greedy).  Six phrases with
    shared prefixes at boost 3 (the model's logits have a standard deviation of 1 and span +-4.3); audio seed, phrase seed
    and boost were chosen on the CPU so that the biased path leaves the unbiased one in >= 5 positions of every row and the
    oracle's smallest margin between the best and second-best allowed logit is >= 1e-2 — both asserted here."""
    dims, om, models = micro
    B, n_steps, boost = 3, 40, 3.0
    init = [50257] + ([] if with_ts else [_loop_rules(dims, 1).no_timestamps])
    r = _loop_rules(dims, len(init), with_ts)
    feats = _feats(dims, B, seed=28)
    phrases = _six_phrases(r)
    want = phrase_oracle.biased_greedy_decode(om, feats, init, n_steps, r, phrase_oracle.Trie(phrases), boost)
    base = phrase_oracle.biased_greedy_decode(om, feats, init, n_steps, r, None, 0.0)
    n = min(want["tokens"].shape[1], base["tokens"].shape[1])
    assert (want["tokens"][:, :n] != base["tokens"][:, :n]).sum(dim=1).min() >= 5
    assert min(want["margins"]) >= 1e-2, min(want["margins"])
    task = hip.HipTask(models[hip.WH_F32], B, 1, 8)
    try:
        task.set_audio(feats.to(gpu_device).contiguous())
        got, lp = _run_greedy(task, gpu_device, init, r, dims, n_steps, B, phrases, boost)
        print("sum_logprobs", lp.tolist(), want["sum_logprobs"])
        assert torch.equal(got, want["tokens"])
        assert np.allclose(lp.numpy(), np.array(want["sum_logprobs"]), atol=2e-3)
    finally:
        task.close()


def _forced_ids(r):
    ok = [t for t in range(2000, 40000) if t not in set(r.suppress_tokens)]
    return ok[17], ok[4242], ok[9001], ok[123]


def _assert_forced(text, phrases):
    """every token of `text` is one the list boosts in the state the tokens before it lead to (phrase_oracle.Trie: the
    specification's walk); returns the states visited"""
    trie = phrase_oracle.Trie(phrases)
    state, states = 0, []
    for i, t in enumerate(text):
        assert t in trie.boosted(state), (i, t, state, text)
        state = trie.step(state, t)
        states.append(state)
    return states


def _text(row, r, T0):
    """the sampled text tokens of a row: without the timestamps, up to <|endoftext|>"""
    out = []
    for t in row[T0:].tolist():
        if t == r.eot:
            break
        if t < r.eot:
            out.append(t)
    return out


@pytest.mark.parametrize("dt", [hip.WH_F32, hip.WH_F16], ids=["f32", "f16"])
@pytest.mark.parametrize("B,G,temperature", [(3, 1, 0.0), (24, 1, 0.0), (2, 2, 0.5)], ids=["3rows", "24rows", "best_of2"])
def test_forced_walk(micro, gpu_device, dt, B, G, temperature):
    """A list at boost 50 — more than the model's whole logit spread, asserted from one prompt pass — decides every text
    token, whatever the model: each one must come from the boosted set of the row's node (`_assert_forced`), so the first
    labels a root edge, and with {[a, b, c], [b, d]} a `d` can never follow `a b`: the b after a is the edge out of node(a), which wins over
    the root's b -> d, and node(a b) boosts c, a and b only.  fp16 and fp32; 3 rows (the 8-row fused step), 24 rows, and
    best_of = 2 at temperature 0.5.
    The issue that asked for this test expected the text `a b c a b c ...`.  The specified rule does not give that: the
    root's edges are boosted in EVERY state, so after `a` both `a` (+50, root) and `b` (+50, node(a)) are candidates and the
    model's raw logits choose between them — with these weights the CPU oracle and the device both repeat `a` (text
    `a a a a ...`, 23 of 23 text tokens in row 0).  What is asserted here is what the rule does imply."""
    dims, om, models = micro
    model = models[dt]
    r = _loop_rules(dims, 1, True)
    a, b, c, d = _forced_ids(r)
    R = B * G
    feats = _feats(dims, B, seed=5).to(gpu_device, model.torch_dtype).contiguous()
    task = hip.HipTask(model, B, G, 8)
    try:
        task.set_audio(feats)
        first = torch.full((R, 1), 50257, dtype=torch.int64, device=gpu_device)
        logits = task.prefill(first)[:, 0]
        spread = float(logits.max() - logits.min())
        assert spread < 50.0 / max(temperature, 1.0) - (20.2 if temperature > 0 else 0.0), spread
        for phrases in ([[a, b, c]], [[a, b, c], [b, d]]):
            task.reset()
            got, _ = _run_greedy(task, gpu_device, [50257], r, dims, 24, R, phrases, 50.0, temperature=temperature, seed=99)
            for row in got:
                assert row[1] >= r.timestamp_begin                       # the initial timestamp
                text = _text(row, r, 1)
                assert len(text) >= 6, text
                _assert_forced(text, phrases)                           # (so the first is a root edge: a, or b in the second list)
    finally:
        task.close()


def test_lifecycle_and_statuses(micro, gpu_device):
    """begin + poll equals the blocking call; a task whose hand-offs are forced to expire re-runs from the prompt with the
    rows back at the root and gives the same tokens; wh_task_reset clears the list (the next loop is the unbiased one);
    every status of wh_task_set_phrases, and wh_task_beam(_begin) with a list set."""
    dims, om, models = micro
    B, n_steps = 3, 24
    r = _loop_rules(dims, 1, True)
    phrases, boost = _six_phrases(r), 3.0
    feats = _feats(dims, B, seed=28)
    L = hip.lib()
    for dt in (hip.WH_F32, hip.WH_F16):
        model = models[dt]
        f = feats.to(gpu_device, model.torch_dtype).contiguous()
        task = hip.HipTask(model, B, 1, 8)
        try:
            task.set_audio(f)
            plain, plain_lp = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B)
            task.reset()
            biased, lp = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B, phrases, boost)
            assert not torch.equal(biased, plain)
            task.reset()
            polled, lp2 = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B, phrases, boost, begin=True)
            assert torch.equal(polled, biased) and torch.equal(lp2, lp)
            task.reset()                                                   # ... which cleared the list
            again, again_lp = _run_greedy(task, gpu_device, [50257], r, dims, n_steps, B)
            assert torch.equal(again, plain) and torch.equal(again_lp, plain_lp)
        finally:
            task.close()
        if dt == hip.WH_F16:
            # hand-offs forced to expire: the loop is re-run from the prompt on the two-launch kernels, rows back at the root
            ref = hip.HipTask(model, B, 1, 8, two_launch_self=True, two_launch_cross=True)
            flaky = hip.HipTask(model, B, 1, 8, expire_handoffs=True)
            try:
                ref.set_audio(f)
                want, want_lp = _run_greedy(ref, gpu_device, [50257], r, dims, n_steps, B, phrases, boost)
                flaky.set_audio(f)
                assert flaky.fused_cross_attention
                rerun, rerun_lp = _run_greedy(flaky, gpu_device, [50257], r, dims, n_steps, B, phrases, boost)
                assert flaky.handoff_fallbacks == 1
                assert torch.equal(rerun, want) and torch.equal(rerun_lp, want_lp)
            finally:
                ref.close()
                flaky.close()

    model = models[hip.WH_F32]
    pl = PhraseList(phrases, boost=boost)
    begin, token, node = pl.device_arrays(gpu_device)

    def ph(**kw):
        v = dict(n_nodes=pl.n_nodes, n_edges=pl.n_edges, child_begin=begin.data_ptr(), child_token=token.data_ptr(),
                 child_node=node.data_ptr(), boost=boost)
        v.update(kw)
        return hip.Phrases(**v)
    task = hip.HipTask(model, B, 1, 8)
    beam = hip.HipTask(model, 1, 2, 8)
    try:
        task.set_audio(feats.to(gpu_device).contiguous())
        h = task.handle
        assert L.wh_task_set_phrases(None, ctypes.byref(ph()), None) == 1
        for bad in (ph(child_begin=None), ph(child_token=None), ph(child_node=None), ph(n_nodes=1, n_edges=0),
                    ph(n_nodes=65536, n_edges=65535), ph(n_edges=pl.n_edges + 1), ph(boost=0.0), ph(boost=math.inf),
                    ph(boost=math.nan)):
            assert L.wh_task_set_phrases(h, ctypes.byref(bad), None) == 1
        assert L.wh_task_set_phrases(h, ctypes.byref(ph()), hip.stream_ptr(task.stream)) == 0
        assert L.wh_task_set_phrases(h, None, None) == 0                    # NULL clears
        tokens = torch.zeros(B, 1 + n_steps + 1, dtype=torch.int64, device=gpu_device)
        tokens[:, 0] = 50257
        mask = _mask(r, dims, gpu_device)
        p = _params(r, n_steps, mask, dims)
        pend = task.greedy_begin(tokens, p, 0, -1)
        refused = L.wh_task_set_phrases(h, ctypes.byref(ph()), None)
        while pend.poll() is None:
            pass
        assert refused == 4                                                  # WH_ERR_STATE while a begun loop is pending
        torch.cuda.synchronize()
        assert torch.equal(tokens[:, : plain.shape[1]].cpu(), plain)       # ... and the cleared list left the loop unbiased

        beam.set_audio(feats[:1].to(gpu_device).contiguous())
        beam.set_phrases((begin, token, node), boost)
        buf = torch.zeros(2, 2, 1 + 8 + 1, dtype=torch.int64, device=gpu_device)
        buf[0, :, 0] = 50257
        bp = hip.BeamParams(rules=_params(r, 8, mask, dims), beam_size=2, max_candidates=2)
        with pytest.raises(hip.HipError):
            beam.beam(buf, bp, 0, -1)
        with pytest.raises(hip.HipError):
            beam.beam_begin(buf, bp, 0, -1)
        beam.set_phrases(None)
        beam.beam(buf, bp, 0, -1)                                            # without the list the beam loop runs
        # wh_task_step / wh_task_prefill ignore the list: raw logits
        task.reset()
        raw = task.prefill(tokens[:, :1].contiguous())
        task.reset()
        task.set_phrases((begin, token, node), 50.0)
        assert torch.equal(task.prefill(tokens[:, :1].contiguous()), raw)
        stepped = task.step(tokens[:, 0])
        task.reset()
        task.prefill(tokens[:, :1].contiguous())
        assert torch.equal(task.step(tokens[:, 0]), stepped)
    finally:
        task.close()
        beam.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. Python
# ---------------------------------------------------------------------------------------------------------------------
def _audio(seed, n=480000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = rng.standard_normal(n).astype(np.float32) * 0.05
    x += (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 1870 * t)).astype(np.float32)
    return x


@pytest.fixture(scope="module")
def setup(gpu_device, tmp_path_factory):
    dims = dims_for("micro.en")
    sd = synthetic_state_dict(dims, seed=1)
    path = str(tmp_path_factory.mktemp("ckpt") / "micro.en.pt")
    save_checkpoint(path, dims, sd)
    model = whisper_amd.load_model(path, device=gpu_device)
    mels = torch.stack([whisper_amd.pad_or_trim(whisper_amd.log_mel_spectrogram(_audio(3 + i), dims.n_mels, device=gpu_device),
                                                3000) for i in range(6)])
    from whisper_amd.decoding import DecodingTask
    tk = DecodingTask(model, whisper_amd.DecodingOptions(language="en")).tokenizer
    suppress = set(DecodingTask(model, whisper_amd.DecodingOptions(language="en"))._suppress)
    ok = [t for t in range(2000, 40000) if t not in suppress]
    return model, mels, tk, (ok[17], ok[4242], ok[9001], ok[123])


def _moderate(setup):
    model, mels, tk, (a, b, c, d) = setup
    return PhraseList([[a, b, c], [a, b, d], [a, c], [d], [d, c, a], [b, a]], boost=3.0, tokenizer=tk)


def test_decode_fused_route_equals_host_loop(setup):
    """decode(..., phrases=) on the device-side loop against the same task pushed onto the host loop by a no-op filter
    (PhraseBias + wh_task_step): fp32, tokens equal, avg_logprob within 1e-4 — form and bound of
    tests/test_api_gpu.py::test_generic_loop_equals_fused; greedy with and without timestamps"""
    from whisper_amd.decoding import DecodingTask, LogitFilter

    class Noop(LogitFilter):
        def apply(self, logits, tokens):
            return None
    model, mels, tk, _ = setup
    pl = _moderate(setup)
    for kw in (dict(), dict(without_timestamps=True)):
        opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=20, **kw)
        fused = whisper_amd.decode(model, mels[:2], opts, phrases=pl)
        task = DecodingTask(model, opts, phrases=pl)
        assert task._fused_greedy_ok(None)
        task.logit_filters.append(Noop())
        assert not task._fused_greedy_ok(None)
        generic = task.run(mels[:2])
        plain = whisper_amd.decode(model, mels[:2], opts)
        for f, g, p in zip(fused, generic, plain):
            assert f.tokens == g.tokens and abs(f.avg_logprob - g.avg_logprob) < 1e-4
            assert f.tokens != p.tokens                                    # the list did change the path


def test_ragged_prompts_and_decode_many_with_phrases(setup):
    model, mels, tk, _ = setup
    pl = _moderate(setup)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=16)
    prompts = [[1000, 1001, 1002, 1003, 1004], None, [2000, 2001]]
    together = whisper_amd.decode(model, mels[:3], opts, prompts=prompts, phrases=pl)
    for i, p in enumerate(prompts):
        alone = whisper_amd.decode(model, mels[i], whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=16, prompt=p),
                                   phrases=pl)
        assert together[i].tokens == alone.tokens, i
        assert abs(together[i].avg_logprob - alone.avg_logprob) < 1e-4
    batches = [mels[0:2].float(), mels[2:3].float(), mels[3:6].float()]
    many = whisper_amd.decode_many(model, batches, opts, chain_rows=24, phrases=pl)
    plain = whisper_amd.decode_many(model, batches, opts, chain_rows=24)
    assert [len(m) for m in many] == [2, 1, 3]
    flat = [r for m in many for r in m]
    for i, res in enumerate(flat):
        alone = whisper_amd.decode(model, mels[i], opts, phrases=pl)
        assert res.tokens == alone.tokens, i
    assert [r.tokens for r in flat] != [r.tokens for m in plain for r in m]


def test_beam_search_with_phrases_runs_the_host_route(setup):
    """beam 3 with a list at boost 50: the host loop with the PhraseBias filter; the winner's text is decided by the list
    (see test_forced_walk for why that is `every token from the boosted set of its state`, not `a b c a b c`)"""
    from whisper_amd.decoding import DecodingTask
    model, mels, tk, (a, b, c, d) = setup
    pl = PhraseList([[a, b, c]], boost=50.0, tokenizer=tk)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=14, beam_size=3)
    assert not DecodingTask(model, opts, phrases=pl)._fused_beam_ok()
    res = whisper_amd.decode(model, mels[0], opts, phrases=pl)
    text = [t for t in res.tokens if t < tk.eot]
    assert len(text) >= 6 and text[0] == a, text
    _assert_forced(text, [[a, b, c]])


def test_transcribe_with_phrases_and_without(setup):
    model, mels, tk, (a, b, c, d) = setup
    audio = np.concatenate([_audio(3), _audio(4)])[: 16000 * 45]
    kw = dict(language="en", fp16=False, sample_len=16, temperature=0.0, condition_on_previous_text=False,
              no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None)
    out = whisper_amd.transcribe(model, audio, phrases=[[a, b, c]], phrase_boost=50.0, **kw)
    assert len(out["segments"]) >= 1
    windows = 0
    for seg in out["segments"]:
        text = [t for t in seg["tokens"] if t < tk.eot]
        assert text, seg
    # every window is decided by the list (test_forced_walk): its text, segments in order, starts with a and every token
    # comes from the boosted set of the state before it
    by_seek = {}
    for seg in out["segments"]:
        by_seek.setdefault(seg["seek"], []).extend(t for t in seg["tokens"] if t < tk.eot)
    for seek, text in by_seek.items():
        windows += 1
        assert len(text) >= 3 and text[0] == a, (seek, text)
        _assert_forced(text, [[a, b, c]])
    assert windows >= 2
    # phrases=None is the call without the keyword
    base = whisper_amd.transcribe(model, audio, **kw)
    none = whisper_amd.transcribe(model, audio, phrases=None, **kw)
    assert [s["tokens"] for s in none["segments"]] == [s["tokens"] for s in base["segments"]] and none["text"] == base["text"]
    assert [s["avg_logprob"] for s in none["segments"]] == [s["avg_logprob"] for s in base["segments"]]
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=16)
    r0, r1 = whisper_amd.decode(model, mels[0], opts), whisper_amd.decode(model, mels[0], opts, phrases=None)
    assert r0.tokens == r1.tokens and r0.avg_logprob == r1.avg_logprob and r0.no_speech_prob == r1.no_speech_prob
