"""tests/mel_ref.py without a GPU: the float64 log-mel reference against the oracle, the float32 model of mel_kernel against
the reference's power-domain bound (the 4x margin behind parity_ref.C_MEL), and the bound's own teeth — it is small on most
entries, and every perturbed reference (window, frame shift, a dropped tap, padding mode, which frame is dropped, the scope
of the maximum, the floor) leaves it somewhere."""
import numpy as np
import pytest
import torch

import mel_ref as mr
import oracle
from parity_ref import C_MEL

SIG = mr.signals()
FILTERS = {n: oracle.mel_filterbank(n) for n in (80, 128)}
_CACHE = {}


def _ref(name, n_mels):
    key = (name, n_mels)
    if key not in _CACHE:
        _CACHE[key] = mr.mel_ref(SIG[name], FILTERS[n_mels])
    return _CACHE[key]


def _power(name, resync):
    key = ("power", name, resync)
    if key not in _CACHE:
        _CACHE[key] = mr.emulate_power_fp32(SIG[name], resync)
    return _CACHE[key]


def test_signal_classes():
    assert tuple(SIG) == mr.CLASSES and len(SIG) == 12
    again = mr.signals()
    for name, a in SIG.items():
        assert a.dtype == np.float32 and a.shape == (mr.N_CLASS,) and np.array_equal(a, again[name]), name
        assert np.abs(a).max() <= 1.0
    assert not SIG["zeros"].any() and np.count_nonzero(SIG["click"]) == 1
    assert not SIG["speech+pad"][mr.N_CLASS // 2:].any() and SIG["speech+pad"][: mr.N_CLASS // 2].any()
    for name in ("quiet", "speech+pad"):                           # on the 16-bit grid
        assert np.array_equal(SIG[name] * 32768.0, np.round(SIG[name] * 32768.0)), name


@pytest.mark.parametrize("n_mels", [80, 128])
def test_reference_equals_the_oracle(n_mels):
    """every class alone and a batch of three (the maximum is global over the batch): 1e-12 against the oracle in float64"""
    F = FILTERS[n_mels]
    for name in mr.CLASSES:
        want = oracle.log_mel_spectrogram(SIG[name][None], F, dtype=torch.float64, keep_dtype=True).numpy()
        assert want.dtype == np.float64
        got = _ref(name, n_mels)[0]
        assert got.shape == want.shape == (1, n_mels, mr.N_CLASS // 160)
        assert np.abs(got - want).max() <= 1e-12, name
    a = np.stack([SIG["full-scale noise"], SIG["zeros"], SIG["quiet"]])
    want = oracle.log_mel_spectrogram(a, F, dtype=torch.float64, keep_dtype=True).numpy()
    got, bound = mr.mel_ref(a, F)
    assert np.abs(got - want).max() <= 1e-12
    assert np.isfinite(bound).all() and (bound > 0).all()


@pytest.mark.parametrize("n_mels", [80, 128])
def test_model_stays_inside_a_quarter_of_the_bound(n_mels):
    """the float32 model of mel_kernel (16-tap resync) against float64: at most 0.25 of the bound on every class — C_MEL is
    four times the model's peak (modelled: at most 0.19)"""
    worst = {}
    for name in mr.CLASSES:
        ref, bound = _ref(name, n_mels)
        got = mr.emulate_finish_fp32(_power(name, 16), FILTERS[n_mels])
        assert got.dtype == np.float32 and np.isfinite(got).all()
        worst[name] = float((np.abs(got - ref) / bound).max())
    print(f"n_mels={n_mels} C_MEL=2^{np.log2(C_MEL):.0f} model / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.25, worst


def test_spectrum_error_of_the_model():
    """the constant itself: the model's spectrum error, as the error of sqrt(P) against float64 (a lower estimate of |dX|),
    over S_f stays inside C_MEL on every class, bin and frame.  Eleven classes peak at 2^-21.6 or below; `click` reaches
    2^-20.9 on the frames that hold the one sample: S_f is a single tap there, so the drift of one rotated twiddle (up to
    15 rotations since its re-read) is not averaged over other taps.  On the output that is 0.11 of the bound"""
    peak = 0.0
    for name in mr.CLASSES:
        a = SIG[name].astype(np.float64)
        xp = np.pad(a, (mr.HALF, mr.HALF), mode="reflect")
        idx = (np.arange(mr.N_CLASS // 160) * mr.HOP)[:, None] + np.arange(mr.N_FFT)[None, :]
        fr = xp[idx] * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(mr.N_FFT) / mr.N_FFT))
        mag = np.abs(np.fft.rfft(fr, axis=-1)).T                               # [201][F]
        S = np.abs(fr).sum(-1)[None, :]
        got = np.sqrt(_power(name, 16)[0].astype(np.float64))
        if S.max() > 0:
            peak = max(peak, float((np.abs(got - mag) / np.where(S > 0, S, 1.0)).max()))
    print(f"model |dX| / S_f peak = 2^{np.log2(peak):.2f}")
    assert peak <= C_MEL


@pytest.mark.parametrize("n_mels", [80, 128])
def test_bound_is_not_vacuous(n_mels):
    """a condition on the reference alone: per class at least half of all entries are bounded by 2e-5"""
    med = {name: float(np.median(_ref(name, n_mels)[1])) for name in mr.CLASSES}
    print(f"n_mels={n_mels} median bound:", {k: f"{v:.2e}" for k, v in med.items()})
    assert max(med.values()) <= 2e-5, med


# perturbation -> the classes that must see it.  tone_bin25, click and zeros cannot see the tap-200 drop (their centre tap
# carries nothing or the bin is orthogonal to it), dc+tiny cannot see the shift, zeros sees nothing
PERTURBED = {
    "symmetric_window": (dict(symmetric_window=True), ("tone440", "noise+sines", "tone7990", "full-scale noise")),
    "shift": (dict(shift=1), ("tone440", "noise+sines", "tone7990", "click")),
    "drop_tap200": (dict(drop_tap200=True), ("tone440", "noise+sines", "full-scale noise", "dc+tiny")),
    "edge_pad": (dict(edge_pad=True), ("tone440", "quiet", "square")),
    "drop_first": (dict(drop_first=True), ("tone440", "click", "speech+pad")),
    "floor": (dict(floor=7.0), ("tone440", "speech+pad", "click")),
}


@pytest.mark.parametrize("what", sorted(PERTURBED))
@pytest.mark.parametrize("n_mels", [80, 128])
def test_perturbed_reference_leaves_the_bound(what, n_mels):
    kw, classes = PERTURBED[what]
    for name in classes:
        ref, bound = _ref(name, n_mels)
        pert = mr.mel_ref(SIG[name], FILTERS[n_mels], **kw)[0]
        ratio = float((np.abs(pert - ref) / bound).max())
        print(f"{what} n_mels={n_mels} {name}: {ratio:.3g}")
        assert ratio > 100.0, (what, name, ratio)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_per_clip_maximum_leaves_the_bound(n_mels):
    """a loud and a quiet clip in one batch: the loud clip's floor decides the quiet clip's entries"""
    a = np.stack([SIG["full-scale noise"], SIG["quiet"]])
    ref, bound = mr.mel_ref(a, FILTERS[n_mels])
    pert = mr.mel_ref(a, FILTERS[n_mels], max_per_clip=True)[0]
    ratio = np.abs(pert - ref) / bound
    assert ratio[0].max() == 0.0 and ratio[1].max() > 100.0, (ratio[0].max(), ratio[1].max())


def test_what_the_resync_buys():
    """recorded, not asserted: the model with the twiddle rotated through all 208 taps without a table re-read.  It reaches the
    bound (ratios 0.4 - 1.06; the 16-tap resync keeps them at or below 0.14)"""
    out = {}
    for n_mels in (80, 128):
        for name in mr.CLASSES:
            ref, bound = _ref(name, n_mels)
            r = [float((np.abs(mr.emulate_finish_fp32(_power(name, rs), FILTERS[n_mels]) - ref) / bound).max()) for rs in (16, 208)]
            out[f"{name}/{n_mels}"] = (round(r[0], 3), round(r[1], 3))
    print("model / bound at resync (16, 208):", out)
