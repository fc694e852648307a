"""Per-token statistics of the sampler kernels (sampling.hip, STATS) against float64, through wht_greedy_sample_stats.

The inputs (tests/token_stats_cases.py) lie on the dyadic grid of tests/test_phrases_gpu.py and every edit is exact in fp32,
so the edited row is the same numbers in fp32 and float64: the token, the order of the top-k list and all padding must
equal float64's EXACTLY.  What is rounded is the normaliser and the entropy.

Log-probabilities.  lp = (x - M) - log S with x - M exact.  S carries the relative error GAMMA = tp.gamma(V) that
test_phrases_gpu.py derives for the chain of online-softmax merges (an absolute error of log S), logf is taken as 2 ulp, the
subtraction rounds once:
    |lp - lp64| <= GAMMA + 2 ulp32(LS) + ulp32(lp),   LS = log S.

Entropy.  H = log s - t / s with t = sum (x - m) exp(x - m) <= 0, carried through the same chain of merges as s, in a
statistic of its own whose {m, s} follow the same recurrences (so s has the error GAMMA again).  Write u = 2^-24.
  * A term enters as d * expf(d), d = x - m exact: expf 4 u (2 ulp), the product u, the addition u: 6 u.
  * A merge maps t -> (t + d s) * expf(d) [+ t'], d = m_old - m_new exact and <= 0.  Every term of t and of d s is <= 0, so
    nothing cancels and a relative error of the parts is at most that relative error of the sum.  The t part meets the
    addition (u), expf (4 u), the product (u) and the second addition (u): 7 u.  The d s part brings the error of s so far
    (6 u per step it went through) plus its own product (u) and then the same 7 u.  By induction a term that went through n
    steps carries at most 7 u n in t where it carries 6 u n in s: with the chain of test_phrases_gpu.py (CHAIN + 1 steps, the
    term's own included)
        GAMMA_T = (7 / 6) GAMMA                 relative, on |t|.
    (Contraction of t + d s into a fused multiply-add removes a rounding; it never adds one.)
  * Q = |t| / s = H - LS >= 0 is the mean of M - x.  The quotient has the relative error GAMMA_T + GAMMA and the division is
    taken as 2 ulp; log s has the absolute error GAMMA + 2 ulp32(LS); the final subtraction rounds once:
        |H - H64| <= GAMMA + 2 ulp32(LS) + Q (GAMMA_T + GAMMA) + 2 ulp32(Q) + ulp32(H).
  First order in GAMMA (1e-5): the products of two such errors are below 1e-9 Q.  Terms whose exp underflows fp32 add less
  than V * 128 * 2^-126 in all.
The top-k log-probabilities share the bound of lp; at temperature 0 entry 0 must equal the token's BITWISE.

The largest error / bound ratio per group goes to token_stats_parity.json (`test_report`, last).
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
import test_beam_gpu as tb  # noqa: E402
import test_phrases_gpu as tp  # noqa: E402
import token_stats_cases as tc  # noqa: E402
from test_phrases_gpu import Buf  # noqa: E402

pytestmark = pytest.mark.gpu

_P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
gamma, ulp32 = tp.gamma, tp.ulp32
REPORT = {}
POISON_F, POISON_I = np.float32(-777.25), np.int32(-777)


def klib():
    h = kernel_lib.lib()
    if not getattr(h, "_token_stats_ready", False):
        rep = [_P, _L, _I, _I, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_size_t, _F,
               ctypes.c_uint64, _P, _I, _I, _P, _P, _P, _P, _P, _F, _I, _F]
        h.wht_greedy_sample_rep.restype = _I
        h.wht_greedy_sample_rep.argtypes = rep + [_P]
        h.wht_greedy_sample_stats.restype = _I
        h.wht_greedy_sample_stats.argtypes = rep + [_P, _P, _I, _P, _P, _L, _P, ctypes.c_size_t, _P]
        for name in ("wht_greedy_sample_scratch_bytes", "wht_greedy_sample_top_scratch_bytes"):
            getattr(h, name).restype = ctypes.c_size_t
            getattr(h, name).argtypes = [_I, _I]
        h.wht_phrase_root_table.restype = _I
        h.wht_phrase_root_table.argtypes = [_P, _P, _P, _I, _I, _P, _P]
        h._token_stats_ready = True
    return h


def lp_bound(V, LS, lp):
    return gamma(V) + 2 * ulp32(LS) + ulp32(lp)


def entropy_bound(V, LS, H):
    Q = max(H - LS, 0.0)
    return gamma(V) + 2 * ulp32(LS) + Q * (gamma(V) * 7 / 6 + gamma(V)) + 2 * ulp32(Q) + ulp32(H)


def launch(case, stats=True, temperature=0.0, seed=0, top_k=None, null=(), stat_stride=None):
    """one step on guarded buffers.  stats=False: wht_greedy_sample_rep on identical inputs.  `null`: statistics buffers
    passed as NULL.  Returns (rc, buffers read back)."""
    h = klib()
    r, x, V, R = case["r"], case["x"], case["V"], case["R"]
    K = case["top_k"] if top_k is None else top_k
    TB = r.timestamp_begin if case["with_ts"] else -1
    stride = case["ntok"] + 3
    ss = stride + 2 if stat_stride is None else stat_stride       # wider than the token buffer: the column is what counts
    tokens = np.full((R, stride), -7, dtype=np.int64)
    rs = np.zeros((R, 4), dtype=np.int32)
    for i, row in enumerate(case["rows"]):
        tokens[i, : len(row)] = row
        H = case["hist"][i]
        if case["with_ts"]:
            stamps = [t for t in H if t >= TB]
            rs[i, 0] = int(len(H) >= 1 and H[-1] >= TB)
            rs[i, 1] = int(len(H) >= 2 and H[-2] >= TB)
            rs[i, 2] = stamps[-1] + 1 if stamps else 0
    begin, token, node = case["trie"].csr()
    mask = np.zeros(V, dtype=np.uint8)
    mask[list(r.suppress_tokens)] = 1
    nbytes, tbytes = h.wht_greedy_sample_scratch_bytes(R, V), h.wht_greedy_sample_top_scratch_bytes(R, V)
    Kb = max(min(K, 8), 1)
    b = dict(x=Buf(x), tokens=Buf(tokens), ntok=Buf(np.array([case["ntok"]], np.int32)), lag=Buf(np.array(case["lag"], np.int32)),
             mask=Buf(mask), sums=Buf(np.array(case["sums"], np.float32)), step=Buf(np.full(R, -7, np.int64)),
             alive=Buf(np.array([-5], np.int32)), part=Buf(np.zeros(nbytes // 4, np.float32)), rs=Buf(rs), begin=Buf(begin),
             token=Buf(token), node=Buf(node), root=Buf(np.full(V, 77, np.int32)), span=Buf(np.full((R, 2), 77, np.int32)),
             lp=Buf(np.full((R, ss), POISON_F)), ent=Buf(np.full((R, ss), POISON_F)),
             top_t=Buf(np.full((R, ss, Kb), POISON_I)), top_v=Buf(np.full((R, ss, Kb), POISON_F)),
             tpart=Buf(np.zeros(tbytes // 4, np.float32)))
    trie_on = case["with_trie"]
    if trie_on:
        assert h.wht_phrase_root_table(b["begin"].ptr(), b["token"].ptr(), b["node"].ptr(), len(token), V, b["root"].ptr(), None) == 0
    pt = (lambda name: b[name].ptr()) if trie_on else (lambda name: None)
    args = [b["x"].ptr(), V, R, V, b["tokens"].ptr(), stride, b["ntok"].ptr(), b["lag"].ptr() if any(case["lag"]) else None,
            case["T0"], r.eot, TB, r.no_timestamps, r.max_initial_timestamp_index, 1, r.blank_token, b["mask"].ptr(),
            b["sums"].ptr(), b["step"].ptr(), b["alive"].ptr(), b["part"].ptr(), nbytes, temperature, seed, b["rs"].ptr(),
            len(begin) - 1, len(token), pt("begin"), pt("token"), pt("node"), pt("root"), pt("span"), tc.BOOST, case["n"],
            case["penalty"]]
    sp = lambda name: None if name in null else b[name].ptr()       # noqa: E731
    if stats:
        rc = h.wht_greedy_sample_stats(*args, sp("lp"), sp("ent"), K, sp("top_t"), sp("top_v"), ss, b["tpart"].ptr(), tbytes, None)
    else:
        rc = h.wht_greedy_sample_rep(*args, None)
    torch.cuda.synchronize()
    for name, buf in b.items():
        assert buf.guards_intact(), name
    assert np.array_equal(b["x"].get().view(np.uint32), x.view(np.uint32)), "the logits buffer must not be written"
    out = {k: v.get() for k, v in b.items()}
    out["tokens0"], out["rs0"] = tokens, rs
    return rc, out


def only_column_written(case, out, K, null=()):
    """every element of the statistics buffers but row i's column still holds the poison"""
    for i, row in enumerate(case["rows"]):
        col = len(row)
        for name, poison in (("lp", POISON_F), ("ent", POISON_F), ("top_t", POISON_I), ("top_v", POISON_F)):
            a = out[name][i].copy()
            written = K > 0 if name.startswith("top") else True
            if name in null or not written:
                assert (a == poison).all(), (name, i)
                continue
            assert not (a[col] == poison).any(), (name, i, "the step's column is not written")
            a[col] = poison
            assert (a == poison).all(), (name, i, "another column was written")


def check(case, group, temperature=0.0, seed=0):
    """a launch with statistics against float64 and against the launch without them"""
    V, R, K = case["V"], case["R"], case["top_k"]
    rc, out = launch(case, True, temperature, seed)
    assert rc == 0
    rc0, ref = launch(case, False, temperature, seed)
    assert rc0 == 0
    for name in ("tokens", "step", "sums", "rs", "span", "alive"):      # invariance, bit for bit
        assert out[name].tobytes() == ref[name].tobytes(), (group, name)
    only_column_written(case, out, K)
    worst = REPORT.setdefault(group, {"logprob": 0.0, "entropy": 0.0, "top_logprob": 0.0})
    for i, w in enumerate(case["want"]):
        col = len(case["rows"][i])
        tok = int(out["tokens"][i, col])
        assert out["tokens"][i, col + 1] == -7 and list(out["tokens"][i, :col]) == case["rows"][i]
        lp, H = float(out["lp"][i, col]), float(out["ent"][i, col])
        tt, tv = out["top_t"][i, col].tolist(), out["top_v"][i, col].astype(np.float64).tolist()
        if w["ended"]:
            assert tok == case["r"].eot and lp == 0.0 and H == 0.0
            assert tt == [-1] * K and tv == [-math.inf] * K
            assert out["sums"][i] == np.float32(case["sums"][i])
            continue
        if w["n_allowed"] == 0:
            assert tok == 0 and math.isnan(lp) and math.isnan(H) and math.isnan(float(out["sums"][i]))
            assert tt == [-1] * K and tv == [-math.inf] * K
            continue
        if temperature == 0.0:
            assert tok == w["tok"], (group, i, tok, w["tok"])
            want_lp = w["lp"]
            # entry 0 is the chosen token, its log-probability the accumulated one bit for bit
            assert tt[0] == tok and out["top_v"][i, col, 0].tobytes() == out["lp"][i, col].tobytes(), (group, i)
        else:
            assert np.isfinite(w["xe"][tok]), (group, i, "a filtered token was drawn")
            want_lp = float((w["xe"][tok] - w["xe"].max()) - w["LS"])
        # the value written is the value accumulated: the same fp32 number
        assert np.float32(np.float32(case["sums"][i]) + out["lp"][i, col]).tobytes() == out["sums"][i].tobytes(), (group, i)
        print(f"{group} row {i}: lp {lp:.9g} want {want_lp:.9g} bound {lp_bound(V, w['LS'], want_lp):.3g} | "
              f"H {H:.9g} want {w['H']:.9g} bound {entropy_bound(V, w['LS'], w['H']):.3g}")
        worst["logprob"] = max(worst["logprob"], abs(lp - want_lp) / lp_bound(V, w["LS"], want_lp))
        worst["entropy"] = max(worst["entropy"], abs(H - w["H"]) / entropy_bound(V, w["LS"], w["H"]))
        assert abs(lp - want_lp) <= lp_bound(V, w["LS"], want_lp), (group, i, lp, want_lp)
        assert abs(H - w["H"]) <= entropy_bound(V, w["LS"], w["H"]), (group, i, H, w["H"])
        assert 0.0 <= H <= math.log(w["n_allowed"]) + entropy_bound(V, w["LS"], w["H"])
        assert tt == w["top_t"], (group, i, tt, w["top_t"])                 # order and padding exact
        for j in range(K):
            if w["top_t"][j] < 0:
                assert tv[j] == -math.inf
                continue
            bound = lp_bound(V, w["LS"], w["top_v"][j])
            worst["top_logprob"] = max(worst["top_logprob"], abs(tv[j] - w["top_v"][j]) / bound)
            assert abs(tv[j] - w["top_v"][j]) <= bound, (group, i, j, tv[j], w["top_v"][j])
        if w["fired"]:                                                      # the mass rule fired: timestamps only
            assert all(t < 0 or t >= case["r"].timestamp_begin for t in tt), (group, i, tt)
    return out


def test_mass_bound_is_the_beam_tests():
    assert tc.MASS_BOUND == tb.MASS_BOUND


@pytest.mark.parametrize("with_ts", [True, False], ids=["ts", "nots"])
@pytest.mark.parametrize("R", tc.RS)
@pytest.mark.parametrize("V", tc.VS)
def test_statistics_against_float64(gpu_device, V, R, with_ts):
    """every history length in {0, 1, 2, 17} with every top_k in {1, 5, 8}, arg-max and temperature 0.7: token (arg-max),
    top-k order and padding exact, log-probabilities and entropy within the bounds of the module docstring, the launch
    without statistics reproduced bit for bit, only the step's column written"""
    fired = set()
    for L in tc.LENGTHS:
        for k in tc.TOPS:
            case = tc.build(V, R, with_ts, L, k)
            for temperature in (0.0, 0.7):
                check(case, f"grid-{V}-{'ts' if with_ts else 'nots'}", temperature, seed=0x5eed0000 + L)
            fired |= {w["fired"] for w in case["want"]}
    if with_ts and R > 1:
        assert fired >= {True, False}            # the mass rule fired in some rows and stayed quiet in others


@pytest.mark.parametrize("name", sorted(tc.planted_cases()))
def test_planted_rows(gpu_device, name):
    """equal maxima across a chunk edge (ids 1023 / 1024) and within one thread's four entries, fewer than top_k finite
    entries, a fully filtered row, a row already at <|endoftext|>, ragged rows, and trie + bigram ban + penalty 1.25 together"""
    case = tc.build(**tc.planted_cases()[name])
    out = check(case, name.split("-")[0])
    K = case["top_k"]
    kind = name.split("-")[0]
    cols = [len(row) for row in case["rows"]]
    tops = [out["top_t"][i, c].tolist() for i, c in enumerate(cols)]
    if kind == "chunk_edge":
        hit = [t for t in tops if t[:2] == [1023, 1024]]
        assert hit, tops                                         # where both are allowed they lead, the lower id first
        for i, t in enumerate(tops):
            if t[:2] == [1023, 1024]:
                assert out["top_v"][i, cols[i], 0] == out["top_v"][i, cols[i], 1]
    if kind == "one_thread":
        assert [t for t in tops if t[:4] == [44, 300, 556, 812]], tops
    if kind == "few":
        assert all(t[3:] == [-1] * (K - 3) and sorted(t[:3]) == [10, 700, 701] for t in tops), tops
    if kind == "edits":
        w = case["want"][0]
        assert 250 not in tops[0] and tc.BOOSTED in tops[0]       # the banned token is no alternative, the boosted one is
        assert case["x"][0, 250] > case["x"][0, tc.BOOSTED]       # ... though the raw logits say the opposite
        assert w["xe"][250] == -np.inf
    if kind == "edits" or kind == "lag":
        check(case, kind, 0.7, seed=99)


def test_logprob_and_entropy_alone_and_single_buffers(gpu_device):
    """top_k = 0 writes neither top buffer; each buffer may be NULL on its own"""
    case = tc.build(51866, 3, True, 2, 5)
    rc, full = launch(case)
    assert rc == 0
    rc, out = launch(case, top_k=0)
    assert rc == 0
    only_column_written(case, out, 0)
    for name in ("lp", "ent"):
        cols = [len(row) for row in case["rows"]]
        assert all(out[name][i, c].tobytes() == full[name][i, c].tobytes() for i, c in enumerate(cols))
    for null in (("lp",), ("ent",), ("lp", "ent")):
        rc, out = launch(case, null=null)
        assert rc == 0
        only_column_written(case, out, 5, null)
        for name in {"lp", "ent", "top_t", "top_v"} - set(null):
            assert out[name].tobytes() == full[name].tobytes(), (null, name)
        assert out["tokens"].tobytes() == full["tokens"].tobytes() and out["sums"].tobytes() == full["sums"].tobytes()


def test_refusals_write_nothing(gpu_device):
    """top_k outside 0 .. 8, a missing top buffer, no buffer at all, a stride below the token buffer's: refused before
    anything is launched"""
    case = tc.build(1025, 3, True, 2, 5)
    for kw in (dict(top_k=9), dict(top_k=-1), dict(null=("top_t",)), dict(null=("top_v",)),
               dict(top_k=0, null=("lp", "ent")), dict(stat_stride=case["ntok"] + 2)):
        rc, out = launch(case, **kw)
        assert rc == kernel_lib.hipErrorInvalidValue, kw
        assert out["tokens"].tobytes() == out["tokens0"].tobytes() and out["rs"].tobytes() == out["rs0"].tobytes(), kw
        assert (out["step"] == -7).all() and out["alive"][0] == -5, kw
        assert out["sums"].tobytes() == np.array(case["sums"], np.float32).tobytes(), kw
        assert (out["part"] == 0).all() and (out["tpart"] == 0).all(), kw
        for name, poison in (("lp", POISON_F), ("ent", POISON_F), ("top_t", POISON_I), ("top_v", POISON_F)):
            assert (out[name] == poison).all(), (kw, name)


def test_report(gpu_device):
    """runs last: the largest error / bound ratio per group"""
    from conftest import write_report
    assert REPORT
    obj = {"bounds": {"GAMMA(51866)": gamma(51866), "GAMMA_T(51866)": gamma(51866) * 7 / 6, "MASS_BOUND": tc.MASS_BOUND},
           "kernel_max_ratio": dict(sorted(REPORT.items()))}
    write_report("token_stats_parity.json", obj)
    assert max(max(v.values()) for v in REPORT.values()) < 1.0
