"""beam.hip alone: beam_partial_kernel + beam_row_kernel against float64 (tests/beam_oracle.py::candidates) and
beam_update_kernel bit for bit against its line-by-line model (beam_oracle.beam_update_model), through wht_beam_step of
libwhisper_hip_ktest.so — launch_beam_step unchanged, on caller-supplied buffers inside guard bytes.

Error bound of a candidate's log-probability (derived from the kernels' reduction chain, not tuned).  The logits lie on a
dyadic grid (multiples of 2^-6, |x| < 64, or -inf): maxima, the differences x - max and the order of the values are exact in
fp32, so the K tokens must equal float64's exactly and all the error is in LS = log(sum exp(x - max)):
  * every term is one expf (<= 1 ulp by the device library's table; taken as 2 ulp = 2^-22 relative), and every step of the
    reduction a term goes through is one online-softmax step — stat_add `s * expf(m - x) + 1` / `s + expf(x - m)` or
    stat_merge `s * expf(m - m') + s'`: one more expf (2^-22) and two fp32 roundings (2 * 2^-24), at most 6 * 2^-24
    relative per step (terms that underflow, x - max < -87, are below 2^-126 each against a sum >= 1: nothing);
  * the longest chain of dependent steps: beam_partial_kernel — 4 entries per thread, 6 cross-lane steps (stat_wave_reduce),
    4 waves; beam_row_kernel — the per-thread chunk loop (nchunk <= 64 < 256: one step), 6 cross-lane steps, 4 waves, and
    the text / timestamp join (one stat_merge): CHAIN = 4 + 6 + 4 + 1 + 6 + 4 + 1 = 26;
  * a relative error of the sum is an absolute error of its logarithm: GAMMA = (CHAIN + 1) * 6 * 2^-24 (+ 1: the terms);
  * logf (<= 1 ulp, taken as 2): 2 ulp32(LS); the final subtraction (x - max) - LS, x - max exact: ulp32(|logprob|).
  bound = GAMMA + 2 ulp32(LS) + ulp32(logprob).
The "timestamp mass" decision compares T = ((ts.m - all.m) - logf(all.s)) + logf(ts.s) with X = (tx.m - all.m) - logf(all.s):
logf(all.s) is the same fp32 number on both sides, ts.s went through the chain without the join, log(ts.s) <= log 65536 < 16
(ulp32 = 2^-20), and the three roundings (the two differences, the sum) act on magnitudes below 256 (ulp32 <= 2^-16):
MASS_BOUND = GAMMA + 2 * 2^-20 + 3 * 2^-16 = 5.7e-5.  Every row a case generates must have a float64 margin
|lse(timestamps) - max(text)| above it — asserted when the case is built, on the host — except the planted exact tie, a single
finite timestamp equal to the text maximum, where both sides are exact (ts.s == 1, logf(1) == 0) and the rule stays quiet
("not greater") in the kernel and in float64 alike.

The update kernel is integer bookkeeping and single fp32 additions: fed the device's own cand_lp / cand_tok of the same
launch, the model must give every output bit for bit.

Before every launch the scratch and all outputs hold 0xFF; after it the guard bytes, the logits (NaN in the row gap:
logits_ld = 2 V) and tokens_in must be unchanged.  The largest error / bound ratio per case group goes to beam_parity.json."""
import copy
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle  # noqa: E402
import kernel_lib  # noqa: E402
from oracle.decoding import SamplingRules  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
KMAX = 9                       # kernels.h BEAM_KMAX (checked against wht_beam_kmax)
GAMMA = (26 + 1) * 6 * 2.0 ** -24
MASS_BOUND = GAMMA + 2 * 2.0 ** -20 + 3 * 2.0 ** -16
T0 = 6                         # the longest row's sample_begin
BLANK = 220
REPORT = {}

VT = [(1000, 850), (1024, 1000), (1025, 1024), (2048, 1024), (3000, 1500), (51864, 50363), (51865, 50364), (51866, 50365),
      (65536, 64000)]


def ulp32(x):
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def lp_bound(lp, lse):
    return GAMMA + 2 * ulp32(lse) + ulp32(lp)


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


def poison(shape, dtype):
    """0xFF bytes: -1 in the integer types, a NaN in fp32"""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xFF, np.uint8).view(dtype).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# cases: everything on the host
# ---------------------------------------------------------------------------------------------------------------------
def ids_of(V, TB):
    """eot, no_timestamps as in the multilingual vocabulary (eot 107 below timestamp_begin)"""
    return TB - 107, TB - 1


def stamp(V, TB, k):
    return TB + min(k, V - TB - 1)


def history(V, TB, kind, i):
    """the sampled tokens of row i: every last / penultimate combination at L >= 2, a 300-token history whose last
    timestamp sits at t = 3, t = 260 or t = 299 (the atomicMax walk in strides of 256)"""
    s = lambda k: stamp(V, TB, k)      # noqa: E731
    if kind == "L0":
        return []
    if kind == "L1":
        return [[100], [s(3)]][i % 2]
    if kind == "L3":
        return [[s(3), 100, 101], [s(3), 100, s(9)], [s(3), s(3), 100], [100, s(1), s(1)], [100, 101, 102], [100, 101, TB]][i % 6]
    if kind == "text":
        return [100, 101, 102]
    if kind == "L300":
        h = [100 + t % 50 for t in range(300)]
        h[3] = s(2)
        if i % 3 == 1:
            h[299] = s(9)                      # last = timestamp, penultimate = text: the stamp itself stays allowed
        if i % 3 == 2:
            h[260], h[261] = s(5), s(5)
        return h
    raise ValueError(kind)


def grid_logits(rng, R, V, narrow=None):
    """multiples of 2^-6, |x| < 40 (room above for planted entries, which stay below 64); every other row narrow
    (|x| < 12: many terms carry weight in the sum) unless told"""
    x = np.empty((R, V), np.float32)
    for i in range(R):
        lim = 767 if (i % 2 if narrow is None else narrow) else 2559
        x[i] = rng.integers(-lim, lim + 1, V) / 64.0
    return x


def make_case(V, TB, G, B, kind="L3", seed=0, ts_on=True, max_initial=50, lag=None, with_mask=True, first=None, mc=None,
              with_lcp=None, x=None, hist=None, eot_lift=True):
    rng = np.random.default_rng(1000 * seed + V + 7 * G + B)
    R, K = B * G, G + 1
    eot, no_ts = ids_of(V, TB)
    if x is None:
        x = grid_logits(rng, R, V)
        if eot_lift and kind != "L0":
            x[::3, eot] = 41.0                                         # EOT candidates for the update
    lag_rows = [0] * R if lag is None else [lag[i // G] for i in range(R)]
    L = len(history(V, TB, kind, 0)) if hist is None else len(hist[0])
    rows = []
    for i in range(R):
        h = history(V, TB, kind, i) if hist is None else hist[i]
        assert len(h) == L
        rows.append([eot + 1] * (T0 - lag_rows[i]) + list(h))
    mask = None
    if with_mask:
        mask = np.zeros(V, np.uint8)
        mask[rng.integers(0, eot, 40)] = 1
        mask[[eot + 1, eot + 2, TB - 2, TB - 3]] = 1                    # the specials
    first = (kind == "L0") if first is None else first
    with_lcp = (lag is None) if with_lcp is None else with_lcp
    ntok = T0 + L
    lens = [len(rows[au * G]) for au in range(B)]
    lcp = None
    if with_lcp:
        lcp = [[[beam_oracle.LCP_START] * 8 for _ in range(8)] for _ in range(B)] if first else \
            [rng.integers(0, lens[au] + 3, (8, 8)).tolist() for au in range(B)]
    return dict(V=V, TB=TB, ts_on=ts_on, G=G, B=B, K=K, R=R, x=x, rows=rows, ntok=ntok, lag=lag_rows if lag is not None else None,
                max_initial=max_initial, mask=mask, sums=(rng.integers(-64, 1, R) / 4.0).astype(np.float32), eot=eot, no_ts=no_ts,
                fin=[[] for _ in range(B)], mc=G if mc is None else mc, done=[0] * B, applied=0, lcp=lcp, first=int(first),
                stride=ntok + 3)


def rules_of(case, i):
    lag = case["lag"][i] if case["lag"] else 0
    suppress = np.flatnonzero(case["mask"]).tolist() if case["mask"] is not None else []
    return SamplingRules(sample_begin=T0 - lag, sot_index=0, eot=case["eot"], timestamp_begin=case["TB"] if case["ts_on"] else None,
                         no_timestamps=case["no_ts"], max_initial_timestamp_index=None if case["max_initial"] < 0 else case["max_initial"],
                         suppress_blank=True, blank_token=BLANK, suppress_tokens=suppress)


def expected(case, K=None, mutate=None):
    """float64 candidates of every row ([R][K] tokens, log-probabilities, per-row info).  The margin of the mass rule is
    asserted here, on the host, for every row.  `mutate(rules)`: a deliberately wrong reference (the controls)."""
    K = case["K"] if K is None else K
    toks, lps, infos = [], [], []
    for i in range(case["R"]):
        r = rules_of(case, i)
        if mutate:
            mutate(r)
        t, v, info = beam_oracle.candidates(case["x"][i], case["rows"][i][r.sample_begin:], r, K, with_info=True)
        if not mutate and np.isfinite(info["margin"]):
            assert info["margin"] > MASS_BOUND or (info["margin"] == 0.0 and info["n_ts"] == 1), (i, info)
        toks.append(t), lps.append(v), infos.append(info)
    return np.array(toks), np.array(lps), infos


# ---------------------------------------------------------------------------------------------------------------------
# one launch
# ---------------------------------------------------------------------------------------------------------------------
def launch(case, B=None, G=None, K=None, R=None, V=None, expect_rc=0, tokens_out_before=None, tokens_in=None):
    h = kernel_lib.lib()
    assert h.wht_beam_kmax() == KMAX
    cV, cR, cB, mc, stride = case["V"], case["R"], case["B"], case["mc"], case["stride"]
    B, G, K = cB if B is None else B, case["G"] if G is None else G, case["K"] if K is None else K
    R, V = cR if R is None else R, cV if V is None else V
    xg = np.full((cR, 2 * cV), np.nan, np.float32)                      # logits_ld = 2 V, NaN in the gap
    xg[:, :cV] = case["x"]
    tokens = np.full((cR, stride), -7, np.int64) if tokens_in is None else tokens_in.copy()
    for i, row in enumerate(case["rows"]):
        assert tokens_in is None or tokens[i, : len(row)].tolist() == row
        tokens[i, : len(row)] = row
    fin_tok, fin_len, fin_score = poison((cB, mc, stride), np.int64), poison((cB, mc), np.int32), poison((cB, mc), np.float32)
    for au, lst in enumerate(case["fin"]):
        for n, (seq, score) in enumerate(lst):
            fin_tok[au, n, : len(seq)], fin_len[au, n], fin_score[au, n] = seq, len(seq), np.float32(score)
    nbytes = h.wht_beam_scratch_bytes(max(R, cR), max(V, cV))
    lp_off, tok_off = ctypes.c_int64(), ctypes.c_int64()
    h.wht_beam_cand_offsets(cR, cV, ctypes.byref(lp_off), ctypes.byref(tok_off))
    assert 0 < lp_off.value < tok_off.value == lp_off.value + cR * KMAX * 4 <= nbytes - cR * KMAX * 4
    tout = poison((cR, stride), np.int64) if tokens_out_before is None else tokens_out_before
    b = dict(x=Buf(xg), tokens_in=Buf(tokens), tokens_out=Buf(tout), ntok=Buf(np.array([case["ntok"]], np.int32)),
             lag=Buf(np.array(case["lag"] or [0] * cR, np.int32)), mask=Buf(case["mask"] if case["mask"] is not None else np.zeros(cV, np.uint8)),
             sums=Buf(case["sums"]), scratch=Buf(poison((nbytes,), np.uint8)), fin_tok=Buf(fin_tok), fin_len=Buf(fin_len),
             fin_score=Buf(fin_score), fin_count=Buf(np.array([len(f) for f in case["fin"]], np.int32)), src=Buf(poison((cR,), np.int32)),
             lcp=Buf(np.array(case["lcp"] if case["lcp"] is not None else np.zeros((cB, 8, 8)), np.int32).reshape(cB, 64)),
             copy_from=Buf(poison((cR,), np.int32)), step=Buf(poison((cR,), np.int64)), done_prev=Buf(np.array(case["done"], np.int32)),
             done_next=Buf(poison((cB,), np.int32)), applied=Buf(np.array([case["applied"]], np.int32)))
    before = {k: v.get() for k, v in b.items()}
    rc = h.wht_beam_step(b["x"].ptr(), 2 * cV, B, G, K, R, V, b["tokens_in"].ptr(), b["tokens_out"].ptr(), stride, b["ntok"].ptr(),
                         b["lag"].ptr() if case["lag"] else None, T0, case["eot"], case["TB"] if case["ts_on"] else -1, case["no_ts"],
                         case["max_initial"], 1, BLANK, b["mask"].ptr() if case["mask"] is not None else None, b["sums"].ptr(),
                         b["scratch"].ptr(), nbytes, b["fin_tok"].ptr(), b["fin_len"].ptr(), b["fin_score"].ptr(), b["fin_count"].ptr(),
                         mc, b["src"].ptr(), b["lcp"].ptr() if case["lcp"] is not None else None,
                         b["copy_from"].ptr() if case["lcp"] is not None else None, b["step"].ptr(), b["done_prev"].ptr(),
                         b["done_next"].ptr(), b["applied"].ptr(), case["first"], None)
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    out = {k: v.get() for k, v in b.items()}
    for name, buf in b.items():
        assert buf.guards_intact(), name
    unchanged = ("x", "tokens_in", "ntok", "lag", "mask", "done_prev") if rc == 0 else tuple(b)
    for name in unchanged:
        assert np.array_equal(out[name].view(np.uint8), before[name].view(np.uint8)), f"{name} was written"
    if rc == 0:
        sc = out["scratch"]
        out["cand_lp"] = sc[lp_off.value: lp_off.value + cR * KMAX * 4].view(np.float32).reshape(cR, KMAX)
        out["cand_tok"] = sc[tok_off.value: tok_off.value + cR * KMAX * 4].view(np.int32).reshape(cR, KMAX)
        out["tokens_out_before"] = before["tokens_out"]
        out["before"] = before
    return out


def compare_candidates(case, out, want):
    """-> (all tokens exact and all log-probabilities within the bound, largest error / bound)"""
    toks, lps, infos = want
    K, ok, worst = case["K"], True, 0.0
    for i in range(case["R"]):
        for k in range(K):
            got_t, got_v = int(out["cand_tok"][i, k]), float(out["cand_lp"][i, k])
            if got_t != toks[i][k] or math.isnan(got_v) or math.isinf(got_v) != math.isinf(lps[i][k]):
                ok = False
                continue
            if math.isinf(got_v):
                ok = ok and got_v < 0 and lps[i][k] < 0
                continue
            ratio = abs(got_v - lps[i][k]) / lp_bound(lps[i][k], infos[i]["lse"])
            worst = max(worst, ratio)
            ok = ok and ratio <= 1.0
    return ok, worst


def check_candidates(case, out, group, want=None):
    want = expected(case) if want is None else want
    ok, worst = compare_candidates(case, out, want)
    print(f"{group}: V={case['V']} TB={case['TB']} G={case['G']} B={case['B']} largest error / bound = {worst:.4f}")
    REPORT[group] = max(REPORT.get(group, 0.0), worst)
    if not ok:
        for i in range(case["R"]):
            print(i, out["cand_tok"][i, :case["K"]].tolist(), want[0][i].tolist(), out["cand_lp"][i, :case["K"]].tolist(), want[1][i].tolist())
    assert ok, group
    assert (bits(out["cand_lp"][:, case["K"]:]) == 0xFFFFFFFF).all() and (out["cand_tok"][:, case["K"]:] == -1).all()
    return want


def check_update(case, out):
    """every output of beam_update_kernel against the model fed with the device's own candidates"""
    G, K, B, R, mc, stride = case["G"], case["K"], case["B"], case["R"], case["mc"], case["stride"]
    st = dict(tokens=[list(r) for r in case["rows"]], sums=case["sums"].copy(), fin=copy.deepcopy(case["fin"]), done=list(case["done"]),
              applied=case["applied"])
    if case["lcp"] is not None:
        st["lcp"] = copy.deepcopy(case["lcp"])
    frozen = all(case["done"])
    new, src = beam_oracle.beam_update_model(st, out["cand_lp"][:, :K], out["cand_tok"][:, :K], bool(case["first"]), G, K, case["eot"], mc)
    stale = out["tokens_out_before"]
    for i in range(R):
        row = new["tokens"][i]
        assert row is not None and out["tokens_out"][i, : len(row)].tolist() == row, (i, out["tokens_out"][i].tolist(), row)
        assert np.array_equal(out["tokens_out"][i, len(row):], stale[i, len(row):]), i
        assert len(row) == len(case["rows"][i]) + (0 if frozen else 1)
    assert np.array_equal(bits(out["sums"]), bits(new["sums"])), (out["sums"], new["sums"])
    assert out["src"].tolist() == src
    assert out["step"].tolist() == [-1 if t is None else t for t in new["step_tokens"]]
    for au in range(B):
        n = len(new["fin"][au])
        assert out["fin_count"][au] == n
        for k in range(mc):
            if k < n:
                seq, score = new["fin"][au][k]
                assert out["fin_len"][au, k] == len(seq) == new["fin_len"][au][k]
                assert out["fin_tok"][au, k, : len(seq)].tolist() == list(seq) and (out["fin_tok"][au, k, len(seq):] == -1).all()
                assert bits(out["fin_score"][au, k]) == bits(np.float32(score)), (au, k)
            else:
                assert out["fin_len"][au, k] == -1 and (out["fin_tok"][au, k] == -1).all() and bits(out["fin_score"][au, k]) == 0xFFFFFFFF
    assert out["done_next"].tolist() == new["done"]
    assert int(out["applied"][0]) == new["applied"]
    if case["lcp"] is not None:
        assert out["lcp"].reshape(B, 8, 8).tolist() == new["lcp"]
        assert out["copy_from"].tolist() == new["copy_from"]
    else:
        assert (out["copy_from"] == -1).all()
    return new, src


def advance(case, new, out):
    """the next launch's case: the state the model (== the device) left"""
    nxt = dict(case)
    nxt.update(rows=[list(r) for r in new["tokens"]], sums=np.array(new["sums"], np.float32), fin=new["fin"], done=list(new["done"]),
               applied=new["applied"], first=0, ntok=case["ntok"] + (0 if all(case["done"]) else 1))
    if case["lcp"] is not None:
        nxt["lcp"] = new["lcp"]
    return nxt


# ---------------------------------------------------------------------------------------------------------------------
# a. candidates against float64 (every launch is also held to the update model)
# ---------------------------------------------------------------------------------------------------------------------
GB = [(2, 1), (5, 3), (8, 1), (2, 3), (5, 1), (8, 3)]
MODES = [dict(kind="L0", max_initial=50), dict(kind="L0", max_initial=0), dict(kind="L0", max_initial=-1), dict(kind="L1"),
         dict(kind="L3"), dict(kind="L300"), dict(kind="L3", ts_on=False), dict(kind="L3", with_mask=False),
         dict(kind="L3", lag=[0, 2, 5])]


def mode_cases(V, TB):
    n = VT.index((V, TB))
    for m, mode in enumerate(MODES):
        G, B = GB[(n + m) % len(GB)]
        if "lag" in mode:
            B = 3
        yield make_case(V, TB, G, B, seed=m, **mode)


@pytest.mark.parametrize("V,TB", VT)
def test_candidates_against_float64(gpu_device, V, TB):
    """The vocabulary tail of a chunk, timestamp_begin on a chunk edge (the `has == false` branches) and inside a chunk;
    L = 0 with max_initial_timestamp_index 50 / 0 / none, L = 1, every last / penultimate combination, 300-token histories,
    rules off, a null mask, ragged rows; G in {2, 5, 8} x B in {1, 3}."""
    for case in mode_cases(V, TB):
        out = launch(case)
        check_candidates(case, out, "candidates")
        check_update(case, out)


def test_full_pool_forty_rows(gpu_device):
    """V = 65536 with beam 8: nchunk = 64 and 2 * 64 * 9 = POOL_MAX entries, pool_v / pool_i exactly full; 5 x 8 = 40 rows"""
    case = make_case(65536, 64000, 8, 5, kind="L3", seed=11)
    out = launch(case)
    check_candidates(case, out, "full_pool")
    check_update(case, out)


def few_finite_case(G, seed=0):
    """rows with exactly 0, 1, G (= K - 1) and K finite entries after the filters, once inside one chunk and once one per
    chunk, in two segments; the rows left over are ordinary ones"""
    V, TB, B = 51865, 50364, 2
    K = G + 1
    case = make_case(V, TB, G, B, kind="text", seed=seed, eot_lift=False)
    rng = np.random.default_rng(seed)
    plans = [(n, spread) for n in (0, 1, G, K) for spread in (False, True)]
    counts = {}
    for i in range(min(case["R"], len(plans))):
        n, spread = plans[(i + 4 * seed) % len(plans)]
        ids = [c * 1024 + 17 + c for c in range(n)] if spread else [5000 + 3 * c for c in range(n)]
        if i % 2 and n:
            ids[-1] = case["eot"]                                   # an EOT among the few
        assert not case["mask"][ids].any() and BLANK not in ids
        row = np.full(V, -np.inf, np.float32)
        row[ids] = rng.integers(-640, 641, n) / 64.0
        case["x"][i] = row
        counts[i] = n
    return case, counts


@pytest.mark.parametrize("G", [2, 5, 8])
def test_rows_with_few_finite_logits(gpu_device, G):
    """fewer than K finite logits: the kernel's `(-inf, token 0)` candidates, no NaN; the update keeps a -inf candidate
    only where a segment has nothing finite left (held to the model, whose rank puts them behind every finite score)"""
    for seed in range(2 if G == 2 else 1):
        case, counts = few_finite_case(G, seed)
        out = launch(case)
        want = check_candidates(case, out, "few_finite")
        for i, n in counts.items():
            assert np.isfinite(want[1][i]).sum() == min(n, case["K"]) and np.isfinite(out["cand_lp"][i, :case["K"]]).sum() == n
            assert (out["cand_tok"][i, n:case["K"]] == 0).all() and not np.isnan(out["cand_lp"][i, :case["K"]]).any()
        new, src = check_update(case, out)
        # -inf candidates are kept only when nothing finite is left: a kept -inf score implies every finite non-EOT
        # candidate of the segment was kept too
        for au in range(case["B"]):
            r0 = au * G
            kept_inf = sum(np.isneginf(new["sums"][r0:r0 + G]))
            sc = (case["sums"][r0:r0 + G, None] + out["cand_lp"][r0:r0 + G, :case["K"]]).reshape(-1)
            finite_live = int((np.isfinite(sc) & (out["cand_tok"][r0:r0 + G, :case["K"]].reshape(-1) != case["eot"])).sum())
            assert kept_inf == max(0, G - finite_live), (au, kept_inf, finite_live)


def tie_case(V, TB, G, B):
    """exact ties of the maximum planted above everything else (60 > the 40 cap): 256 apart (one thread's entries), adjacent,
    in different chunks, three-fold, and across timestamp_begin"""
    case = make_case(V, TB, G, B, kind="text", seed=3, eot_lift=False)
    x, eot = case["x"], case["eot"]
    free = [t for t in range(300, eot - 300) if not case["mask"][t]]
    a = free[0]
    same_thread = [t for t in free if t > a and (t - a) % 256 == 0 and t // 1024 == a // 1024]
    other_chunk = [t for t in free if t // 1024 != a // 1024]
    adjacent = [t for t in free if not case["mask"][t + 1]]
    plans = [[a, same_thread[0]], [adjacent[5], adjacent[5] + 1], [a, other_chunk[0] if other_chunk else free[-1]],
             [free[9], same_thread[-1], free[-1]]]
    for i in range(case["R"] - 1):
        x[i, plans[i % len(plans)]] = 60.0
        x[i, TB:] = np.minimum(x[i, TB:], 30.0)
        if i % 5 == 4:
            x[i, eot] = 60.0                                           # ... and an EOT tying a text token, inside one row
    # across timestamp_begin: text and timestamps tie at the top.  With several timestamps the mass rule fires (three
    # timestamps at the maximum: margin log 3) and only they are left; with a single finite timestamp it ties exactly, the
    # rule stays quiet and the text id comes first
    r = case["R"] - 1
    x[r, TB:] = np.minimum(x[r, TB:], 30.0)
    x[r, [free[7], TB, stamp(V, TB, 4), stamp(V, TB, 9)]] = 60.0
    return case


@pytest.mark.parametrize("V,TB,G,B", [(3000, 1500, 5, 2), (1025, 1024, 2, 3), (51865, 50364, 8, 1)])
def test_planted_ties_of_the_maximum(gpu_device, V, TB, G, B):
    """equal values: the smaller id comes first — inside one thread's four entries, between neighbours, across chunks and
    across timestamp_begin; (1025, 1024) holds the exact tie of the single timestamp with the text maximum"""
    case = tie_case(V, TB, G, B)
    want = expected(case)
    top = want[1][:, 0]
    assert sum(want[1][i, 1] == top[i] for i in range(case["R"])) >= case["R"] - 1          # the ties are in the reference
    if V - TB == 1:
        info = want[2][case["R"] - 1]
        assert info["margin"] == 0.0 and not info["fired"] and want[0][case["R"] - 1, 1] == TB
    out = launch(case)
    check_candidates(case, out, "ties", want)
    check_update(case, out)


def mass_case(V, TB, seed=0):
    """64 rows, logits on the grid in [-12, 12), the timestamp range of every row shifted so that logsumexp(timestamps) -
    max(text) lands near a target drawn from [-6, 6): rows on both sides of the decision"""
    G, B = 8, 8
    case = make_case(V, TB, G, B, kind="text", seed=seed, eot_lift=False, x=np.zeros((G * B, V), np.float32))
    rng = np.random.default_rng(77 + seed + V)
    x = (rng.integers(-768, 768, (G * B, V)) / 64.0).astype(np.float32)
    case["x"] = x
    for i in range(G * B):
        _, info = beam_oracle.filtered_float64(x[i], case["rows"][i][T0:], rules_of(case, i))
        d0 = (1 if info["fired"] else -1) * info["margin"]
        target = rng.integers(-384, 384) / 64.0
        if V - TB == 1 and i == 0:
            target = 0.0                                # planted: the single timestamp ties the text maximum exactly
        x[i, TB:] += np.float32(round((target - d0) * 64) / 64.0)
    assert np.abs(x).max() < 64
    return case


MASS_VT = [(1000, 850), (1025, 1024), (2048, 1024), (51864, 50363), (51866, 50365), (65536, 64000)]


@pytest.mark.parametrize("V,TB", MASS_VT)
def test_timestamp_mass_rule_on_both_sides(gpu_device, V, TB):
    """the rule decided from two online-softmax statistics: every row's float64 margin exceeds MASS_BOUND (asserted in
    expected(), none left out), at least a quarter of the rows fire it and at least a quarter do not"""
    case = mass_case(V, TB)
    want = expected(case)
    fired = sum(info["fired"] for info in want[2])
    print("fired", fired, "of", case["R"], "smallest margin", min(info["margin"] for info in want[2]))
    assert 4 * fired >= case["R"] and 4 * (case["R"] - fired) >= case["R"]
    if V - TB == 1:
        assert want[2][0]["margin"] == 0.0 and not want[2][0]["fired"]
    out = launch(case)
    check_candidates(case, out, "mass_rule", want)
    check_update(case, out)


def test_bound_is_not_vacuous(gpu_device):
    """the right reference passes; each wrong one fails: suppress mask dropped, timestamp_begin off by one, the K-th
    candidate swapped with the (K + 1)-th, cand_lp shifted by 4 x bound"""
    V, TB, G, B = 3000, 1500, 5, 3
    case = make_case(V, TB, G, B, kind="L3", seed=5)
    masked = int(np.flatnonzero(case["mask"])[0])
    case["x"][0, masked] = 45.0                              # a masked id that would win
    assert case["rows"][5][-1] == TB                          # history ending in timestamp_begin itself (history(), i % 6 == 5)
    want = expected(case)
    out = launch(case)
    ok, worst = compare_candidates(case, out, want)
    assert ok and worst <= 1.0

    def drop_mask(r):
        r.suppress_tokens = []

    def tb_plus_one(r):
        r.timestamp_begin += 1
    assert not compare_candidates(case, out, expected(case, mutate=drop_mask))[0]
    assert not compare_candidates(case, out, expected(case, mutate=tb_plus_one))[0]
    t1, v1, infos = expected(case, K=case["K"] + 1)
    swapped = (np.delete(t1, case["K"] - 1, axis=1), np.delete(v1, case["K"] - 1, axis=1), infos)
    assert not compare_candidates(case, out, swapped)[0]
    for sign in (1, -1):
        shifted = want[1] + sign * 4 * np.array([[lp_bound(v, infos[i]["lse"]) for v in want[1][i]] for i in range(case["R"])])
        assert not compare_candidates(case, out, (want[0], shifted, want[2]))[0]


# ---------------------------------------------------------------------------------------------------------------------
# b. the update kernel, bit-exact against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 5, 8])
def test_first_update(gpu_device, G):
    """first = 1: identical rows (what the loop feeds), then differing rows — only beam G - 1 counts"""
    V, TB, B = 3000, 1500, 3
    case = make_case(V, TB, G, B, kind="L0", seed=1)
    for au in range(B):
        case["x"][au * G:(au + 1) * G] = case["x"][au * G]
    case["sums"][:] = 0
    out = launch(case)
    check_candidates(case, out, "update")
    new, src = check_update(case, out)
    assert src == [au * G + G - 1 for au in range(B) for _ in range(G)]
    case = make_case(V, TB, G, B, kind="L0", seed=2)          # differing rows and sums
    out = launch(case)
    new, src = check_update(case, out)
    assert src == [au * G + G - 1 for au in range(B) for _ in range(G)]
    last = out["cand_tok"][[au * G + G - 1 for au in range(B)], :G]
    assert out["step"].reshape(B, G).tolist() == last.tolist()


@pytest.mark.parametrize("G", [2, 5, 8])
def test_score_ties_across_source_rows(gpu_device, G):
    """two beams with equal sums and identical logits: equal scores from different source rows, the lower candidate index
    first; the EOT logit ties the best text logit, so an EOT candidate ties a text candidate as well"""
    V, TB, B = 1025, 1024, 2
    case = make_case(V, TB, G, B, kind="text", seed=4, eot_lift=False)
    for au in range(B):
        r0 = au * G
        case["x"][r0 + 1] = case["x"][r0]
        case["sums"][r0 + 1] = case["sums"][r0] = 0.0
        best = int(np.argmax(np.where(case["mask"][:case["no_ts"]] == 0, case["x"][r0, :case["no_ts"]], -np.inf)))
        case["x"][r0:r0 + 2, case["eot"]] = case["x"][r0, best]
    out = launch(case)
    check_candidates(case, out, "update")
    new, src = check_update(case, out)
    for au in range(B):
        r0 = au * G
        assert np.array_equal(bits(out["cand_lp"][r0]), bits(out["cand_lp"][r0 + 1]))          # the tie is real
        at = out["cand_tok"][r0, :case["K"]].tolist().index(case["eot"])
        top = bits(out["cand_lp"][r0, :case["K"]]) == bits(out["cand_lp"][r0, 0])
        assert top[at] and top.sum() >= 2                                                       # EOT ties the best text token


def eot_heavy_case(G, B, mc, counts, seed=0, done=None):
    """every row's best candidate is EOT (its logit far above the rest): a step's EOT list holds G entries; the segment's
    list holds counts[au] sequences at entry"""
    V, TB = 2048, 1024
    case = make_case(V, TB, G, B, kind="text", seed=seed, mc=mc, eot_lift=False)
    case["x"][:, case["eot"]] = 50.0
    case["sums"] = (-np.arange(case["R"]) / 4.0).astype(np.float32)
    n = len(case["rows"][0])
    case["fin"] = [[(tuple([7] * (n - 1 - k % 2) + [case["eot"]]), -1.5 * (k + 1)) for k in range(counts[au])] for au in range(B)]
    if done is not None:
        case["done"] = done
    return case


@pytest.mark.parametrize("G", [2, 5, 8])
def test_max_candidates_reached_inside_one_eot_list(gpu_device, G):
    """max_candidates in {1, G // 2, G, 2 G}: the list fills in the middle of one step's EOT list; one segment is full at
    entry while the others are not"""
    for mc in sorted({1, max(1, G // 2), G, 2 * G}):
        counts = [max(0, mc - (G - 1)), mc, max(0, mc - 1)]        # G EOT candidates meet room for G - 1, none and one
        case = eot_heavy_case(G, 3, mc, counts, seed=mc, done=[0, 1, 0])
        out = launch(case)
        new, src = check_update(case, out)
        assert out["fin_count"].tolist() == [mc] * 3 and out["done_next"].tolist() == [1, 1, 1]
    # a list that does not fill: completion flags stay down
    case = eot_heavy_case(G, 2, 3 * G, [0, G - 1], seed=9)
    out = launch(case)
    check_update(case, out)
    assert out["fin_count"].tolist() == [G, 2 * G - 1] and out["done_next"].tolist() == [0, 0]


def test_last_token_slot_lag_without_lcp_and_frozen_updates(gpu_device):
    """len = token_stride - 1 (the new token lands in the row's last slot, in tokens_out and in fin_tok); lag set with lcp
    null; then two further updates after completion: only tokens_out, src, copy_from and done_next may change and d_applied
    does not move"""
    G, B = 5, 3
    case = eot_heavy_case(G, B, 2, [1, 1, 1], seed=2)
    case["stride"] = case["ntok"] + 1
    out = launch(case)
    new, _ = check_update(case, out)
    assert (out["tokens_out"][:, -1] != -1).all() and (out["fin_tok"][:, 1, -1] == case["eot"]).all()
    assert out["done_next"].tolist() == [1] * B

    ragged = make_case(3000, 1500, G, B, kind="L3", seed=6, lag=[0, 2, 5], mc=1)
    assert ragged["lcp"] is None
    ragged["x"][:, ragged["eot"]] = 50.0                        # completes at once
    out = launch(ragged)
    new, _ = check_update(ragged, out)
    assert out["done_next"].tolist() == [1] * B and [len(new["tokens"][au * G]) for au in range(B)] == [10, 8, 5]
    for with_lcp in (False, True):
        cur = advance(ragged, new, out)
        if with_lcp:
            cur["lcp"] = [np.arange(64).reshape(8, 8).tolist() for _ in range(B)]
        for _ in range(2):
            o = launch(cur)
            nxt, src = check_update(cur, o)                       # the model's frozen branch: identity, nothing else moves
            assert src == list(range(cur["R"])) and int(o["applied"][0]) == cur["applied"] == 1
            for name in ("sums", "fin_tok", "fin_len", "fin_score", "fin_count", "step", "lcp", "applied"):
                assert np.array_equal(o[name].view(np.uint8), o["before"][name].view(np.uint8)), name
            cur = advance(cur, nxt, o)


# ---------------------------------------------------------------------------------------------------------------------
# c. a multi-step run with a real cache
# ---------------------------------------------------------------------------------------------------------------------
def stamp_bytes(layer, which, history_tokens):
    """64 bytes that identify (cache, layer, token history) — what a decoder would have computed from that history"""
    rng = np.random.default_rng([layer, which, len(history_tokens)] + [int(t) for t in history_tokens])
    return rng.integers(0, 256, 64, dtype=np.uint8)


@pytest.mark.parametrize("G", [2, 5, 8])
def test_multi_step_run_with_a_cache(gpu_device, G):
    """B = 3, 24 updates, the token buffers ping-ponged as api.cpp::beam_update does, the EOT logit lifted so that the lists
    fill and the run completes.  Toy K and V caches (2 layers x R rows x 32 positions x 64 bytes): before each update position
    len - 1 of every row is stamped from the row's token history; after wht_beam_step, wht_permute_groups with the device's
    src and copy_from must leave in every row's first `len` positions what the full gather old[src[i]] gives, and the bytes
    beyond untouched.  Every step's outputs equal the model's."""
    h = kernel_lib.lib()
    V, TB, B, NL, NPOS, PB = 3000, 1500, 3, 2, 32, 64
    R = B * G
    case = make_case(V, TB, G, B, kind="L0", seed=20 + G, mc=G)
    case["stride"] = T0 + 24 + 2
    case["sums"][:] = 0
    rng = np.random.default_rng(G)
    row_bytes, layer_bytes = NPOS * PB, R * NPOS * PB
    cache = [rng.integers(0, 256, (NL, R, NPOS, PB), dtype=np.uint8) for _ in range(2)]         # K, V; stale bytes everywhere
    for i in range(R):                                                                            # the prompt's positions
        for p in range(T0 - 1):
            for which in range(2):
                for layer in range(NL):
                    cache[which][layer, i, p] = stamp_bytes(layer, which, case["rows"][i][: p + 1])
    tok_bufs = [None, poison((R, case["stride"]), np.int64)]                                     # the two token buffers: in, out
    completed_at, moved, full = None, 0, 0
    for step in range(24):
        n = len(case["rows"][0])
        frozen = all(case["done"])
        for i in range(R):
            for which in range(2):
                for layer in range(NL):
                    cache[which][layer, i, n - 1] = stamp_bytes(layer, which, case["rows"][i])
        x = grid_logits(rng, R, V)
        if step == 0:
            for au in range(B):
                x[au * G:(au + 1) * G] = x[au * G]
        x[:, case["eot"]] = np.where(rng.random(R) < 0.5, 41.0, x[:, case["eot"]])            # lifted: the lists fill
        case["x"] = x
        out = launch(case, tokens_out_before=tok_bufs[1], tokens_in=tok_bufs[0])
        if step % 4 == 0:
            check_candidates(case, out, "multi_step")
        new, src = check_update(case, out)
        kb, vb = Buf(cache[0]), Buf(cache[1])
        src_b, cf_b = Buf(out["src"]), Buf(out["copy_from"])
        assert h.wht_permute_groups(kb.ptr(), vb.ptr(), NL, layer_bytes, B, G, row_bytes, n * PB, src_b.ptr(), cf_b.ptr(), PB, None) == 0
        torch.cuda.synchronize()
        assert kb.guards_intact() and vb.guards_intact()
        for which, buf in enumerate((kb, vb)):
            got = buf.get()
            want = cache[which].copy()
            want[:, :, :n] = cache[which][:, src, :n]                                           # the full gather
            assert np.array_equal(got, want), (step, which)
            cache[which] = got
        moved += sum(n - c for i, c in enumerate(out["copy_from"].tolist()) if src[i] != i)
        full += sum(n for i in range(R) if src[i] != i)
        tok_bufs = [out["tokens_out"], out["tokens_in"]]                                       # ping-pong
        case = advance(case, new, out)
        if all(case["done"]) and completed_at is None:
            completed_at = step
        assert frozen == (completed_at is not None and step > completed_at)
    assert completed_at is not None and completed_at < 22, "the run completes and at least two frozen updates follow"
    assert case["applied"] == completed_at + 1
    assert moved < full                                                                          # the shared history did save copies


# ---------------------------------------------------------------------------------------------------------------------
# d. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu_device):
    """hipErrorInvalidValue, and every buffer as it was, for K != G + 1, G = 9, R != B * G and V = 65537 (65 chunks)"""
    case = make_case(3000, 1500, 5, 2, kind="L3", seed=8)
    bad = kernel_lib.hipErrorInvalidValue
    launch(case, K=5, expect_rc=bad)
    launch(case, K=7, expect_rc=bad)
    launch(case, G=9, K=10, expect_rc=bad)
    launch(case, R=9, expect_rc=bad)
    launch(case, B=3, expect_rc=bad)
    launch(case, V=65537, expect_rc=bad)
    out = launch(case)                                            # ... and the same buffers are accepted as they stand
    check_candidates(case, out, "candidates")
    check_update(case, out)


def test_report(gpu_device):
    """runs last: the largest error / bound ratio per case group, to beam_parity.json"""
    from conftest import write_report
    write_report("beam_parity.json", {"bounds": {"GAMMA": GAMMA, "MASS_BOUND": MASS_BOUND}, "max_ratio": dict(sorted(REPORT.items()))})
    assert REPORT and max(REPORT.values()) < 1.0
