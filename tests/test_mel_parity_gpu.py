"""wh_log_mel (whisper_amd/csrc/mel.hip) element by element against the float64 reference of tests/mel_ref.py, under its
power-domain bound (derived in mel_ref's module docstring; C_MEL in parity_ref.py): twelve signal classes at both stock
filterbanks, the frame counts around a workgroup of 16 frames, the global maximum across a batch, scratch reuse, filterbanks
that reach the branches the stock banks never take, and the refusals.  Every call runs on guarded buffers: `audio` and
`filters` stay as they were, every entry of `out` is written and finite, nothing is written outside a payload.  The last test
writes each case's largest error / bound to mel_parity.json."""
import numpy as np
import pytest
import torch

import mel_ref as mr
import oracle
from parity_ref import C_MEL, Buf, _stream

pytestmark = pytest.mark.gpu

WH_OK, WH_ERR_ARG = 0, 1
REPORT = {}
FILTERS = {n: oracle.mel_filterbank(n) for n in (80, 128)}
_SIG = {}


def _signals(n):
    if n not in _SIG:
        _SIG[n] = mr.signals(n)
    return _SIG[n]


def _buf_from(a, tdt=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(tdt).reshape(-1)
    b = Buf(t.numel(), tdt)
    b.t.copy_(t)
    return b


def _scratch():
    from whisper_amd import hip
    return Buf(hip.MEL_SCRATCH_BYTES, torch.uint8)


def _log_mel(audio, filters, scratch=None):
    """one wh_log_mel call on guarded buffers -> float32 [B][n_mels][n // 160] on the CPU, the invariants checked"""
    from whisper_amd import hip
    audio = np.atleast_2d(np.asarray(audio, dtype=np.float32))
    filters = np.asarray(filters, dtype=np.float32)
    B, n = audio.shape
    n_mels, nf = filters.shape[0], n // 160
    ab, fb, ob = _buf_from(audio), _buf_from(filters), Buf(B * n_mels * nf, torch.float32)
    sb = scratch if scratch is not None else _scratch()
    for b in (ab, fb, ob, sb):
        b.snapshot()
    rc = hip.lib().wh_log_mel(ab.ptr(), n, B, n_mels, fb.ptr(), ob.ptr(), sb.ptr(), _stream())
    assert rc == WH_OK, rc
    torch.cuda.synchronize()
    assert not ab.changed().any(), "audio was written"
    assert not fb.changed().any(), "filters were written"
    sb.changed()                                                   # guard bytes of the scratch
    assert ob.changed().all(), "entries of out not written"        # the fill is a NaN pattern: a finite value differs from it
    got = ob.t.view(B, n_mels, nf).cpu()
    assert torch.isfinite(got).all()
    return got


def _check(key, got, ref, bound):
    ratio = float((np.abs(got.double().numpy() - ref) / bound).max())
    REPORT[key] = max(REPORT.get(key, 0.0), ratio)
    print(f"{key}: error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (key, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ 1. signal classes
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("name", mr.CLASSES)
def test_signal_classes(gpu_device, name, n_mels):
    """B = 1, n = 32000: 200 frames, 13 workgroups.  On `tone440` the kernel's output also tells the perturbed references
    apart (symmetric window, frames one sample late, tap 200 dropped)"""
    a = _signals(mr.N_CLASS)[name]
    got = _log_mel(a, FILTERS[n_mels])
    ref, bound = mr.mel_ref(a, FILTERS[n_mels])
    _check(f"class/{name}/{n_mels}", got, ref, bound)
    if name == "tone440":
        for kw in (dict(symmetric_window=True), dict(shift=1), dict(drop_tap200=True)):
            pert = mr.mel_ref(a, FILTERS[n_mels], **kw)[0]
            assert (np.abs(got.double().numpy() - pert) / bound).max() > 100.0, kw


# --------------------------------------------------------------------------------------------- 2. frame-count edges
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("n,frames", [(201, 1), (319, 1), (320, 2), (2400, 15), (2560, 16), (2719, 16), (2720, 17)])
def test_frame_count_edges(gpu_device, n, frames, n_mels):
    """one partly filled workgroup, exactly one, one plus a single frame; at 201 samples every tap reflects"""
    for name in ("speech+pad", "tone440"):
        a = _signals(n)[name]
        got = _log_mel(a, FILTERS[n_mels])
        assert got.shape == (1, n_mels, frames)
        ref, bound = mr.mel_ref(a, FILTERS[n_mels])
        _check(f"frames/{name}/{n_mels}", got, ref, bound)


# ------------------------------------------------------------------------------------- 3. the maximum across a batch
@pytest.mark.parametrize("n_mels", [80, 128])
def test_global_maximum_across_the_batch(gpu_device, n_mels):
    s = _signals(mr.N_CLASS)
    F = FILTERS[n_mels]
    a = np.stack([s["full-scale noise"], s["zeros"], s["quiet"]])
    ref, bound = mr.mel_ref(a, F)
    # the loud clip's floor decides every entry of the other two
    assert np.ptp(ref[1:]) == 0.0 and abs(ref[1, 0, 0] - (ref[0].max() - 2.0)) < 1e-12
    got = _log_mel(a, F)
    _check(f"batch/loud+zeros+quiet/{n_mels}", got, ref, bound)
    assert (np.abs(got.double().numpy() - mr.mel_ref(a, F, max_per_clip=True)[0]) / bound)[2].max() > 100.0
    a = np.stack([s["quiet"], s["zeros"]])
    ref, bound = mr.mel_ref(a, F)
    _check(f"batch/quiet+zeros/{n_mels}", _log_mel(a, F), ref, bound)


# ------------------------------------------------------------------------------------------------- 4. scratch reuse
def test_scratch_reuse_and_repeatability(gpu_device):
    """one scratch buffer through a loud and then a quiet clip: the second result is bit-equal to the quiet clip's with a
    fresh scratch (a maximum left over from the first call would raise its floor); and the same call twice gives the same
    bits (the maximum over workgroups does not depend on their order)"""
    s = _signals(mr.N_CLASS)
    F = FILTERS[80]
    shared = _scratch()
    loud = _log_mel(s["full-scale noise"], F, shared)
    quiet = _log_mel(s["quiet"], F, shared)
    fresh = _log_mel(s["quiet"], F)
    assert torch.equal(quiet.view(torch.int32), fresh.view(torch.int32))
    assert loud.max() - quiet.max() > 1.0                          # a stale maximum would have shown: floors 8.8 decades apart
    again = _log_mel(s["full-scale noise"], F)
    assert torch.equal(loud.view(torch.int32), again.view(torch.int32))


# ------------------------------------------------------------------------------------------- 5. custom filterbanks
def _banks():
    rng = np.random.default_rng(21)
    w = lambda k: (0.002 + 0.05 * rng.random(k)).astype(np.float32)
    dense = w(8 * 201).reshape(8, 201)                             # band of 201 taps: the loop past MAXBAND = 16 runs
    edges = np.zeros((7, 201), dtype=np.float32)
    edges[1, 40:56] = w(16)                                        # row 0 stays all zero; exactly 16 taps
    edges[2, 60:77] = w(17)                                        # exactly 17
    edges[3, 190:201] = w(11)                                      # band_lo + t runs past bin 200
    edges[4, 0:3] = w(3)                                           # from DC
    edges[5, 100] = 0.03                                           # one tap
    edges[6, 20:50:7] = w(5)                                       # zeros inside the band
    one = np.zeros((1, 201), dtype=np.float32)
    one[0, 10:31] = w(21)                                          # n_mels = 1
    lo, hi = mr.band_of(edges)
    assert lo.tolist() == [201, 40, 60, 190, 0, 100, 20] and hi.tolist() == [-1, 55, 76, 200, 2, 100, 48]
    return {"dense8": dense, "edges7": edges, "one": one}


@pytest.mark.parametrize("bank", ["dense8", "edges7", "one"])
def test_custom_filterbanks(gpu_device, bank):
    """17 frames (a full workgroup and a single frame) of four classes"""
    F = _banks()[bank]
    for name in ("noise+sines", "tone7990", "speech+pad", "dc+tiny"):
        a = _signals(2720)[name]
        got = _log_mel(a, F)
        ref, bound = mr.mel_ref(a, F)
        _check(f"bank/{bank}/{name}", got, ref, bound)


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(gpu_device):
    """n = 200 (reflect padding needs more than 200 samples), n_mels = 129, n_mels = 0 and batch = 0: WH_ERR_ARG, and
    nothing is written"""
    from whisper_amd import hip
    ab, fb, ob, sb = Buf(4000, torch.float32), Buf(129 * 201, torch.float32), Buf(129 * 25, torch.float32), _scratch()
    ab.t.fill_(0.25); fb.t.fill_(0.01)
    for b in (ab, fb, ob, sb):
        b.snapshot()
    for n, batch, n_mels in [(200, 1, 80), (4000, 1, 129), (4000, 1, 0), (4000, 0, 80)]:
        rc = hip.lib().wh_log_mel(ab.ptr(), n, batch, n_mels, fb.ptr(), ob.ptr(), sb.ptr(), _stream())
        assert rc == WH_ERR_ARG, (n, batch, n_mels, rc)
    torch.cuda.synchronize()
    for b in (ab, fb, ob, sb):
        assert not b.changed().any()


# ------------------------------------------------------------------------------------------------------ 7. report
def test_report(gpu_device):
    """runs last: the largest error / bound of every case above, with the constant, goes to mel_parity.json"""
    from conftest import write_report
    expected = ([f"class/{c}/{m}" for c in mr.CLASSES for m in (80, 128)]
                + [f"frames/{c}/{m}" for c in ("speech+pad", "tone440") for m in (80, 128)]
                + [f"batch/{c}/{m}" for c in ("loud+zeros+quiet", "quiet+zeros") for m in (80, 128)]
                + [f"bank/{b}/{c}" for b in ("dense8", "edges7", "one") for c in ("noise+sines", "tone7990", "speech+pad", "dc+tiny")])
    write_report("mel_parity.json", {"bounds": {"C_MEL": C_MEL}, "max_ratio": dict(sorted(REPORT.items()))})
    missing = sorted(set(expected) - set(REPORT))
    assert not missing, f"cases that recorded nothing: {missing}"
    assert all(r <= 1.0 for r in REPORT.values())
