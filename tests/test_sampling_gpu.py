"""Temperature sampling on the GPU: greedy_partial_kernel<true, *, *> / greedy_final_kernel<true, *> (sampling.hip) through
wht_greedy_sample and wht_greedy_sample_rep against the float64 restatement of tests/sampling_oracle.py, on the inputs of
tests/sampling_cases.py (tests/test_sampling_cpu.py bounds their undecidable share without a GPU).

For a DECIDABLE row (sampling_oracle's docstring: the best key leads by more than 2 * EPS_KEY and the timestamp-mass rule's
sides differ by more than MASS_EPS) the drawn token, the token in step_tokens, the row state and the trie node equal the
restatement's exactly.  An undecidable row is skipped for the token alone — what follows from the token is checked against
the token the kernel drew — and at most 0.5 % of a parametrisation's rows may be undecidable.  The accumulated
log-probability lies within gamma(V) + 4 ulp32(lp) + ulp32(sum) (tests/test_phrases_gpu.py derives gamma and the ulp terms;
one more ulp32(lp) for the subtraction x[token] - max that the sampling instantiation adds).  Guard bytes intact, logits
untouched, nothing written behind the new token.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_cases as sc  # noqa: E402
import sampling_oracle as so  # noqa: E402
import test_phrases_gpu as tp  # noqa: E402
import test_repetition_gpu as trep  # noqa: E402
import whisper_amd  # noqa: E402

pytestmark = pytest.mark.gpu

Buf, ulp32 = tp.Buf, tp.ulp32
REPORT = {"cases": {}, "z_gpu": {}}


def test_bounds_are_the_phrase_module_s():
    for V in (1000, 1025, 51866, 300000):
        assert so.gamma(V) == tp.gamma(V)
    for v in (0.0, 1e-3, 17.4, -63.0, 1 << 20):
        assert so.ulp32(v) == tp.ulp32(v)


# ---------------------------------------------------------------------------------------------------------------------
# launching a family
# ---------------------------------------------------------------------------------------------------------------------
def _static(fam):
    """the buffers no launch writes: logits, suppress mask, the trie and its root table"""
    h = tp.klib()
    V, r = fam["V"], fam["r"]
    mask = np.zeros(V, dtype=np.uint8)
    mask[list(r.suppress_tokens)] = 1
    st = dict(x=Buf(fam["x"]), mask=Buf(mask))
    if fam["trie"] is not None:
        begin, token, node = fam["trie"].csr()
        st.update(begin=Buf(begin), token=Buf(token), node=Buf(node), root=Buf(np.full(V, 77, np.int32)))
        assert h.wht_phrase_root_table(st["begin"].ptr(), st["token"].ptr(), st["node"].ptr(), len(token), V, st["root"].ptr(),
                                       None) == 0
        st["csr"] = (begin, token)
    return st


def _launch(fam, la, st, temperature=None):
    """one launch of the two sampler kernels over a family's buffers; returns the buffers it may write and the row state it
    started from"""
    h = trep.klib() if fam["rep"] else tp.klib()
    V, R, r = fam["V"], fam["R"], fam["r"]
    T0, L = la["T0"], len(fam["hist"][0])
    TB = r.timestamp_begin if fam["with_ts"] else -1
    ntok = T0 + L
    stride = ntok + 3
    tokens = np.full((R, stride), -7, dtype=np.int64)
    rs = np.zeros((R, 4), dtype=np.int32)
    for i, H in enumerate(fam["hist"]):
        row = [50258] * (T0 - fam["lag"][i]) + list(H)
        tokens[i, : len(row)] = row
        if fam["with_ts"]:
            stamps = [t for t in H if t >= TB]
            rs[i, 0] = int(len(H) >= 1 and H[-1] >= TB)
            rs[i, 1] = int(len(H) >= 2 and H[-2] >= TB)
            rs[i, 2] = stamps[-1] + 1 if stamps else 0
        rs[i, 3] = fam["states"][i]
    nbytes = h.wht_greedy_sample_scratch_bytes(R, V)
    b = dict(tokens=Buf(tokens), ntok=Buf(np.array([ntok], np.int32)), lag=Buf(np.array(fam["lag"], np.int32)),
             sums=Buf(np.array(fam["sums"], np.float32)), step=Buf(np.full(R, -7, np.int64)), alive=Buf(np.array([-5], np.int32)),
             part=Buf(np.zeros(nbytes // 4, np.float32)), rs=Buf(rs), span=Buf(np.full((R, 2), 77, np.int32)))
    with_trie = fam["trie"] is not None
    pt = (lambda name: st[name].ptr()) if with_trie else (lambda name: None)
    n_nodes, n_edges = (len(st["csr"][0]) - 1, len(st["csr"][1])) if with_trie else (0, 0)
    head = (st["x"].ptr(), V, R, V, b["tokens"].ptr(), stride, b["ntok"].ptr(), b["lag"].ptr() if any(fam["lag"]) else None, T0,
            r.eot, TB, r.no_timestamps, r.max_initial_timestamp_index, 1, r.blank_token, st["mask"].ptr(), b["sums"].ptr(),
            b["step"].ptr(), b["alive"].ptr(), b["part"].ptr(), nbytes, la["temperature"] if temperature is None else temperature,
            la["seed"], b["rs"].ptr(), n_nodes, n_edges, pt("begin"), pt("token"), pt("node"), pt("root"),
            b["span"].ptr() if with_trie else None, fam["boost"])
    if fam["rep"]:
        rc = h.wht_greedy_sample_rep(*head, fam["n"], fam["penalty"], None)
    else:
        rc = h.wht_greedy_sample(*head, None)
    assert rc == 0
    torch.cuda.synchronize()
    for name, buf in b.items():
        assert buf.guards_intact(), name
    return {k: v.get() for k, v in b.items()}, rs


def _static_untouched(fam, st):
    for name, buf in st.items():
        if name != "csr":
            assert buf.guards_intact(), name
    assert np.array_equal(st["x"].get().view(np.uint32), fam["x"].view(np.uint32)), "the logits buffer must not be written"


def _check(fam, la, st, out, rs0, want, tally):
    """one launch against the restatement; tally: rows / skipped / worst log-probability error over its bound"""
    V, r = fam["V"], fam["r"]
    TB = r.timestamp_begin
    L = len(fam["hist"][0])
    got_tokens = []
    for i, w in enumerate(want):
        n = la["T0"] - fam["lag"][i] + L
        got = int(out["tokens"][i, n])
        got_tokens.append(got)
        assert got == out["step"][i], (i, got, out["step"][i])
        assert out["tokens"][i, n + 1] == -7 and list(out["tokens"][i, :n]) == [50258] * (n - L) + list(fam["hist"][i])
        if w["lp"] is None:                                # the row had ended: nothing accumulated, bit for bit
            assert got == r.eot and out["sums"][i] == np.float32(fam["sums"][i]), (i, got, out["sums"][i])
        else:
            tally["rows"] += 1
            if w["decidable"]:
                assert got == w["tok"], (i, got, w, la)
            else:
                tally["skipped"] += 1
            assert 0 <= got < V and fam["rows"][i]["xf"][got] != -np.inf, (i, got)       # never a filtered entry
            if got == w["tok"]:
                total = fam["sums"][i] + w["lp"]
                bound = so.gamma(V) + 4 * ulp32(w["lp"]) + ulp32(total)
                err = abs(float(out["sums"][i]) - total)
                tally["lp_ratio"] = max(tally["lp_ratio"], err / bound)
                assert err <= bound, (i, float(out["sums"][i]), total, bound, la)
        if fam["with_ts"]:                                 # the state the next step's timestamp rules read
            is_ts = got >= TB
            assert list(out["rs"][i, :3]) == [int(is_ts), rs0[i, 0], got + 1 if is_ts else rs0[i, 2]], (i, out["rs"][i])
        else:
            assert list(out["rs"][i, :3]) == [0, 0, 0]
        if fam["trie"] is not None:                        # the trie node follows the drawn token
            s = fam["trie"].step(fam["rows"][i]["state"], got) if w["lp"] is not None else 0
            begin = st["csr"][0]
            assert out["rs"][i, 3] == s, (i, out["rs"][i], s)
            assert list(out["span"][i]) == ([begin[s], begin[s + 1]] if s else [0, 0])
        else:
            assert out["rs"][i, 3] == fam["states"][i]
    return got_tokens


def _run_families(families, name, keep_draws=False):
    tally = dict(rows=0, skipped=0, lp_ratio=0.0)
    draws = {}
    for fam in families:
        fam["rows"] = sc.filtered_rows(fam)
        want = sc.expected(fam, fam["rows"])
        st = _static(fam)
        for la, w in zip(fam["launches"], want):
            out, rs0 = _launch(fam, la, st)
            got = _check(fam, la, st, out, rs0, w, tally)
            if keep_draws:
                for i, t in enumerate(got):
                    if w[i]["lp"] is not None:
                        draws.setdefault((i, la["temperature"]), []).append(t)
        _static_untouched(fam, st)
    share = tally["skipped"] / max(tally["rows"], 1)
    REPORT["cases"][name] = dict(rows=tally["rows"], skipped_share=share, lp_error_over_bound=tally["lp_ratio"])
    print(name, REPORT["cases"][name])
    assert tally["rows"] > 0 and tally["skipped"] <= sc.MAX_UNDECIDABLE * tally["rows"], tally
    return draws


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _ids(params):
    return [f"{V}-{R}-{mode}" for V, R, mode in params]


@pytest.mark.parametrize("V,R,mode", sc.PLAIN_PARAMS, ids=_ids(sc.PLAIN_PARAMS))
def test_plain_against_the_restatement(gpu_device, V, R, mode):
    """<true, false, false> + <true, false> (child_begin = NULL): one chunk, one entry into a second chunk, the real vocabulary;
    1, 3 and 24 rows; the timestamp rules mid-sequence (some rows at <|endoftext|>: sum unchanged bit for bit), at the first
    token, off, and ragged rows; T in {0.5, 1, 2, 0.7}; seeds with both words set, the high word zero, the low word zero; the
    step varied through the prompt length.  256 launches over one set of logits in the small vocabularies, 16 in the large.
    Where there are 256, the kernel's own draws are held to softmax(x / T) as well: chi-square over 8 equal-mass bins per (row,
    T), 64 draws each, pooled; |z| < 5 as in tests/test_sampling_cpu.py."""
    name = f"plain/{V}-{R}-{mode}"
    fam = sc.plain_family(V, R, mode)
    draws = _run_families([fam], name, keep_draws=len(fam["launches"]) >= 256)
    if draws:
        chi, dof = 0.0, 0
        for (i, T), toks in sorted(draws.items()):
            assert len(toks) == len(fam["launches"]) // 4
            c, d = so.goodness_of_fit(toks, so.softmax_t(fam["rows"][i]["xf"], T), 8)
            chi, dof = chi + c, dof + d
        z = so.z_of(chi, dof)
        REPORT["z_gpu"][name] = z
        print("z", name, z, "dof", dof)
        assert dof >= 4 and abs(z) < 5, (z, dof)


@pytest.mark.parametrize("V,R,mode", sc.PHRASE_PARAMS, ids=_ids(sc.PHRASE_PARAMS))
def test_phrase_list_against_the_restatement(gpu_device, V, R, mode):
    """<true, true, false> + <true, true>: the scenario table of tests/test_phrases_gpu.py at boost 4, where the noise decides
    among boosted and unboosted entries; token, trie node and child span exact"""
    fams = sc.families_of("phrase", V, R, mode)
    _run_families(fams, f"phrase/{V}-{R}-{mode}")


@pytest.mark.parametrize("V,R,mode", sc.REP_PARAMS, ids=_ids(sc.REP_PARAMS))
def test_repetition_against_the_restatement(gpu_device, V, R, mode):
    """<true, false, true> and <true, true, true>: the plan and scenarios of tests/test_repetition_gpu.py (every n, histories around
    the 256-token tile, the penalty), every second launch with the phrase list at boost 4 as well"""
    fams = sc.families_of("rep", V, R, mode)
    assert any(f["trie"] is not None for f in fams) and any(f["trie"] is None for f in fams)
    _run_families(fams, f"rep/{V}-{R}-{mode}")


@pytest.mark.parametrize("top", [True, False], ids=["largest_u", "smallest_u"])
def test_edge_entry(gpu_device, top):
    """The entry whose hash has its top 24 bits set (largest uniform; the 24-bit map that sample_noise.h replaced gives
    u == 1.0f and an infinite key there: a library built with it draws this token, row 7 -> 12738) has the lowest logit of
    its row and is not masked: the kernel draws the restatement's token, with a finite log-probability.  The same with the
    top 24 bits clear: the smallest uniform."""
    fam, prow, ptok = sc.edge_family(top)
    fam["rows"] = sc.filtered_rows(fam)
    want = sc.expected(fam, fam["rows"])[0]
    assert fam["rows"][prow]["xf"][ptok] == -63.0 and want[prow]["decidable"] and want[prow]["tok"] != ptok
    st = _static(fam)
    tally = dict(rows=0, skipped=0, lp_ratio=0.0)
    out, rs0 = _launch(fam, fam["launches"][0], st)
    got = _check(fam, fam["launches"][0], st, out, rs0, want, tally)
    assert got[prow] == want[prow]["tok"] != ptok
    assert np.isfinite(out["sums"]).all()
    assert tally["skipped"] <= sc.MAX_UNDECIDABLE * tally["rows"]
    REPORT["cases"]["edge/" + ("largest_u" if top else "smallest_u")] = dict(
        rows=tally["rows"], skipped_share=tally["skipped"] / tally["rows"], lp_error_over_bound=tally["lp_ratio"])


@pytest.mark.parametrize("mode", ["mid", "first", "nots", "lag"])
def test_cold_limit_on_the_device(gpu_device, mode):
    """T = 1e-6 on logits that are pairwise different multiples of 2^-6: the scaled logits are 15625 apart, the noise spans
    less than 20, so the sampling instantiation gives the tokens of the T = 0 launch for every row, and its sums lie within
    the sampling bound of the float64 log-probability of that token"""
    fam = sc.plain_family(1025, 24, mode, n_launches=3, unique=True)
    fam["rows"] = sc.filtered_rows(fam)
    st = _static(fam)
    for la in fam["launches"]:
        cold, _ = _launch(fam, la, st, temperature=1e-6)
        greedy, _ = _launch(fam, la, st, temperature=0.0)
        L = len(fam["hist"][0])
        for i in range(fam["R"]):
            n = la["T0"] - fam["lag"][i] + L
            assert cold["tokens"][i, n] == greedy["tokens"][i, n] == cold["step"][i], (i, cold["tokens"][i, n], greedy["tokens"][i, n])
            assert list(cold["rs"][i]) == list(greedy["rs"][i])
            if fam["ended"][i]:
                assert cold["sums"][i] == greedy["sums"][i] == np.float32(fam["sums"][i])
                continue
            xf = fam["rows"][i]["xf"]
            tok = int(cold["tokens"][i, n])
            assert tok == int(np.argmax(xf))
            m = xf.max()
            total = fam["sums"][i] - math.log(np.exp(xf - m).sum())
            bound = so.gamma(fam["V"]) + 4 * ulp32(total - fam["sums"][i]) + ulp32(total)
            assert abs(float(cold["sums"][i]) - total) <= bound and abs(float(greedy["sums"][i]) - total) <= bound
    _static_untouched(fam, st)


def test_every_entry_filtered(gpu_device):
    """a row whose logits are all -inf: token 0 and a NaN sum in the sampling instantiation too (sampling.hip: `every logit
    filtered`); its neighbours are drawn as usual"""
    fam = sc.plain_family(1025, 3, "nots", n_launches=4)
    fam["x"][1, :] = -np.inf
    fam["rows"] = sc.filtered_rows(fam)
    want = sc.expected(fam, fam["rows"])
    st = _static(fam)
    for la, w in zip(fam["launches"], want):
        assert w[1]["tok"] == 0 and math.isnan(w[1]["lp"])
        out, _ = _launch(fam, la, st)
        n = la["T0"] + 3
        assert out["tokens"][1, n] == 0 == out["step"][1] and math.isnan(float(out["sums"][1]))
        for i in (0, 2):
            assert w[i]["decidable"] and out["tokens"][i, n] == w[i]["tok"]
            total = fam["sums"][i] + w[i]["lp"]
            assert abs(float(out["sums"][i]) - total) <= so.gamma(1025) + 4 * ulp32(w[i]["lp"]) + ulp32(total)
    _static_untouched(fam, st)


def test_timestamp_rules_need_the_row_state(gpu_device):
    """wht_greedy_sample with timestamp rules on and no row_state: hipErrorInvalidValue and every buffer as it was (the
    partial kernel takes the rules' window from the state alone).  R = 1, V = 1025: two vocabulary chunks, the second of one
    entry.  The same call with the rules off (timestamp_begin = -1) is accepted."""
    h = tp.klib()
    V, T0, stride = 1025, 3, 6
    x = np.random.default_rng(5).standard_normal((1, V)).astype(np.float32)
    tokens = np.full((1, stride), -7, dtype=np.int64)
    tokens[0, :T0] = 50258
    nbytes = h.wht_greedy_sample_scratch_bytes(1, V)
    b = dict(x=Buf(x), mask=Buf(np.zeros(V, np.uint8)), tokens=Buf(tokens), ntok=Buf(np.array([T0], np.int32)),
             sums=Buf(np.array([-1.5], np.float32)), step=Buf(np.full(1, -7, np.int64)), alive=Buf(np.array([-5], np.int32)),
             part=Buf(np.zeros(nbytes // 4, np.float32)))
    before = {k: v.get() for k, v in b.items()}

    def call(TB):
        rc = h.wht_greedy_sample(b["x"].ptr(), V, 1, V, b["tokens"].ptr(), stride, b["ntok"].ptr(), None, T0, 1000, TB, 1001, 5, 1,
                                 220, b["mask"].ptr(), b["sums"].ptr(), b["step"].ptr(), b["alive"].ptr(), b["part"].ptr(), nbytes,
                                 0.0, 0, None, 0, 0, None, None, None, None, None, 0.0, None)
        torch.cuda.synchronize()
        for name, buf in b.items():
            assert buf.guards_intact(), name
        return rc

    assert call(1002) == tp.kernel_lib.hipErrorInvalidValue
    for name, buf in b.items():
        assert np.array_equal(buf.get().view(np.uint8), before[name].view(np.uint8)), f"{name} was written"
    assert call(-1) == 0
    out = {k: v.get() for k, v in b.items()}
    want = np.where((np.arange(V) == 220) | (np.arange(V) == 1000), -np.inf, x[0].astype(np.float64))     # SuppressBlank at L = 0
    assert out["tokens"][0, T0] == out["step"][0] == int(np.argmax(want)) and out["alive"][0] == T0
    assert np.array_equal(out["tokens"][0, :T0], tokens[0, :T0]) and np.array_equal(out["tokens"][0, T0 + 1:], tokens[0, T0 + 1:])
    assert np.array_equal(out["x"].view(np.uint32), x.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the loop's plumbing: seed words, step counter, row numbering
# ---------------------------------------------------------------------------------------------------------------------
LOGIT_SLACK = 2e-4      # the loop's own logits against a second pass over the same prompt: the bound test_api_gpu.py::
                        # test_device_sampling (c) holds the two passes' log-probabilities to


def test_main_loop_feeds_the_hash(gpu_device, tmp_path):
    """DecodingTask._main_loop on the micro model, fp32, sample_len = 1, best_of = 8: each of the 8 rows' first tokens equals
    the restatement's draw for (the seed the task draws from torch's generator, step = number of prompt tokens, row = the
    row's index), over 16 torch seeds, from the engine's own first-step logits taken through the torch filters.  This pins
    the seed words, the step counter and the numbering of grouped rows.  The logits the loop samples from come from a pass
    of their own, so a row counts as decidable when its best key leads by more than 2 * (EPS_KEY + LOGIT_SLACK / T)."""
    from whisper_amd import decoding
    from whisper_amd.decoding import DecodingTask
    from whisper_amd.synthetic import dims_for, save_checkpoint, synthetic_state_dict
    dims = dims_for("micro.en")
    path = str(tmp_path / "micro.en.pt")
    save_checkpoint(path, dims, synthetic_state_dict(dims, seed=1))
    model = whisper_amd.load_model(path, device=gpu_device)
    mel = whisper_amd.pad_or_trim(whisper_amd.log_mel_spectrogram(tp._audio(3), dims.n_mels, device=gpu_device), 3000)
    T = 0.7
    opts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=1, temperature=T, best_of=8)
    probe = DecodingTask(model, opts)
    assert probe._fused_greedy_ok(None)
    feats = probe._get_audio_features(mel[None])
    rows = torch.tensor([probe.initial_tokens]).repeat(8, 1).to(gpu_device)
    logits = probe.inference.logits(rows, feats)[:, -1].clone()
    probe.inference.cleanup_caching()
    for f in probe.logit_filters:
        f.apply(logits, rows)
    xf = logits.double().cpu().numpy()
    step = rows.shape[1]
    skipped = checked = 0
    for k in range(16):
        torch.manual_seed(500 + k)
        seed = decoding._draw_seed()
        assert 0 <= seed < 2 ** 62 and (seed >> 32) != 0
        torch.manual_seed(500 + k)
        task = DecodingTask(model, opts)
        toks, sums, _ = task._main_loop(feats, rows.clone())
        assert toks.shape == (8, step + 1)
        for i in range(8):
            w = so.draw(xf[i], T, seed, step, i)
            got = int(toks[i, -1])
            assert xf[i, got] != -np.inf
            if w["margin"] > 2 * (w["eps_key"] + LOGIT_SLACK / T):
                checked += 1
                assert got == w["tok"], (k, i, got, w)
                assert abs(float(sums[i]) - w["lp"]) < LOGIT_SLACK
            else:
                skipped += 1
    print("rows checked", checked, "skipped", skipped)
    REPORT["cases"]["main_loop"] = dict(rows=checked + skipped, skipped_share=skipped / 128, lp_error_over_bound=None)
    assert skipped <= sc.MAX_UNDECIDABLE * 128


def test_report(gpu_device):
    """runs last: per case the share of skipped rows and the largest log-probability error over its bound, and the chi-square
    z values of the restatement's draws (computed here as tests/test_sampling_cpu.py computes them) and of the GPU's"""
    from conftest import write_report
    import test_sampling_cpu as cpu
    z_cpu = {way: {str(T): v for T, v in cpu.distribution_z(way).items()} for way in ("seeds", "steps", "seed_hi")}
    write_report("sampling_parity.json", {"cap_skipped_share": sc.MAX_UNDECIDABLE, "cases": dict(sorted(REPORT["cases"].items())),
                                          "z_cpu": z_cpu, "z_gpu": dict(sorted(REPORT["z_gpu"].items()))})
    assert REPORT["cases"] and REPORT["z_gpu"]
    assert all(abs(v) < 5 for d in z_cpu.values() for v in d.values())
