"""The reference, the bound and the score classes of tests/test_flash_range_gpu.py (tests/flash_ref.py), checked without a GPU:
the fp32 emulation of attn_flash_f16_kernel's order of operations stays inside the unchanged flash bound
_ulp(ref, F16) + C_ATT_MFMA * pv for every class on both forms (so the bound is reachable over the whole score domain and not
tuned to a GPU's output), the perturbed references fail it, every class reaches the branch of the deferred rescale it was built
for (counted in the emulation), and test_attn_flash's own randn inputs reach next to none of them — which is why the classes
exist.  The generic attention kernel's emulation is held to its own bound over the same classes."""
import pytest
import torch

import flash_ref as fr
import prefill_align_ref as pr
from parity_ref import C_ATT_MFMA, F16, F32, _tdt, _ulp

SHAPES = ((200, 150), (1500, 64))      # (T, Tq): ragged last tile of 8 and of 28 keys; 5 waves (the last one padded) and 2
H = 2
_CACHE = {}


def _case(cls, T, Tq, prescaled):
    """inputs, reference, bound, emulation and its counts of one case, computed once"""
    key = (cls, T, Tq, prescaled)
    if key not in _CACHE:
        q, k, v = fr.flash_inputs(cls, T, Tq, H, seed=T + Tq + fr.CLASSES.index(cls), prescaled=prescaled)
        ref, pv, _ = fr.flash_ref(q, k, v, H, prescaled)
        stats = {}
        out, fires, unmoved = fr.flash_emulate(q, k, v, H, prescaled, p_stats=stats)
        _CACHE[key] = dict(q=q, k=k, v=v, ref=ref, bound=_ulp(ref, F16) + C_ATT_MFMA * pv, out=out, fires=fires, unmoved=unmoved,
                           stats=stats)
    return _CACHE[key]


@pytest.mark.parametrize("prescaled", [0, 1])
@pytest.mark.parametrize("cls", fr.CLASSES)
def test_emulation_within_bound_and_bound_not_vacuous(cls, prescaled):
    for (T, Tq) in SHAPES:
        c = _case(cls, T, Tq, prescaled)
        assert torch.isfinite(c["out"]).all(), f"{cls} T={T}: the emulation is not finite"
        r = pr.ratio(c["out"], c["ref"], c["bound"])
        print(f"flash/prescaled{prescaled}/{cls} T={T} Tq={Tq}: emulation error / bound = {r:.3f}")
        assert r <= 1.0, f"{cls} T={T} Tq={Tq}: fp32 emulation at error / bound = {r:.3f}"
        pert = fr.flash_ref(c["q"], c["k"], c["v"], H, prescaled, drop=fr.drop_kind(cls))[0]
        rp = pr.ratio(pert, c["ref"], c["bound"])
        assert rp > 1.0, f"{cls} T={T}: the bound does not see the {fr.drop_kind(cls)} key dropped (ratio {rp:.3f})"


@pytest.mark.parametrize("prescaled", [0, 1])
def test_classes_reach_the_deferred_branch(prescaled):
    for (T, Tq) in SHAPES:
        tiles, waves = (T + 63) // 64, (Tq + 31) // 32
        get = lambda cls: _case(cls, T, Tq, prescaled)                               # noqa: E731
        for cls in ("ramp", "one_lane"):
            assert get(cls)["fires"] == (tiles - 1) * waves * H, f"{cls}: the rescale does not fire on every tile"
        assert get("ramp")["unmoved"] == 0
        # 31 of 32 lanes of every firing wave (the padded wave: its real lanes but the riser)
        assert get("one_lane")["unmoved"] == (tiles - 1) * H * (Tq - sum(1 for t in range(Tq) if t % 32 == 5))
        for cls in ("late_peak", "deep_first"):
            assert get(cls)["fires"] == waves * H, f"{cls}: not exactly one rescale per wave and head"
        for cls in ("early_peak10", "early_peak12"):
            c = get(cls)
            assert c["fires"] == 0
            assert c["stats"]["subnormal"] > c["stats"]["total"] / 2, f"{cls}: P is not mostly fp16-subnormal: {c['stats']}"
        for cls in ("normal", "equal", "deep", "high"):
            assert get(cls)["fires"] == 0, cls


@pytest.mark.parametrize("prescaled", [0, 1])
def test_randn_inputs_hardly_reach_it(prescaled):
    """test_kernel_parity_gpu.test_attn_flash's own inputs (same seeds): the deferred branch fires at most once after tile 0
    in all of (2, 20, 1500, 1500) and never in (2, 6, 129, 129)"""
    for (B, Hh, T, Tq, most) in ((2, 20, 1500, 1500, 1), (2, 6, 129, 129, 0)):
        g = torch.Generator().manual_seed(B * 1000 + Hh * 100 + T + Tq)
        q = torch.randn(B, Tq, Hh * 64, generator=g).half()
        k = torch.randn(B, T, Hh * 64, generator=g).half()
        v = torch.randn(B, T, Hh * 64, generator=g).half()
        if prescaled:
            q, k = (q.float() * fr.PRESCALE).half(), (k.float() * fr.PRESCALE).half()
        fires = sum(fr.flash_emulate(q[b], k[b], v[b], Hh, prescaled)[1] for b in range(B))
        chances = B * Hh * ((Tq + 31) // 32) * ((T + 63) // 64 - 1)
        print(f"prescaled{prescaled} ({B}, {Hh}, {T}, {Tq}): {fires} rescales after tile 0 in {chances} (wave, tile) chances")
        assert fires <= most


@pytest.mark.parametrize("cls", ["deep", "deep_first"])
def test_first_tile_factor(cls):
    """every score of a query's first tile below -128 (exp2 domain): exp2(-mx) is +inf, and 0 * inf = NaN for the rest of
    the launch.  Nothing has been accumulated on the first tile, so any finite factor will do, and the kernel's is
    exp2(-max(mx, 0)) (attention.hip); the unscaled form starts from exp2(-inf - m) = 0."""
    q, k, v = fr.flash_inputs(cls, 200, 150, H, seed=5, prescaled=1)
    assert not torch.isfinite(fr.flash_emulate(q, k, v, H, 1, first_alpha_exp2=True)[0]).any()
    assert torch.isfinite(fr.flash_emulate(q, k, v, H, 1)[0]).all()
    q, k, v = fr.flash_inputs(cls, 200, 150, H, seed=5, prescaled=0)
    assert torch.isfinite(fr.flash_emulate(q, k, v, H, 0)[0]).all()


def test_score_domain():
    """every class stays within |s| <= 190 natural (the bound carries no term for the fp32 rounding of a score), and the
    steering values are exact in fp16 before the prescale"""
    for cls in fr.CLASSES:
        for (T, Tq) in SHAPES:
            q, k, _ = fr.flash_inputs(cls, T, Tq, H, seed=1, prescaled=0)
            for h in range(H):
                s = (q[:, 64 * h:64 * h + 64].double() @ k[:, 64 * h:64 * h + 64].double().T) * 0.125
                assert s.abs().max().item() <= 190.0, (cls, T, s.abs().max().item())
            if cls == "ramp":
                assert torch.equal(k[:, 0].double(), 8.0 * (torch.arange(T) // 64).double())


GENERIC_SHAPE = (200, 33)              # (Tk, Tq) of test_flash_range_gpu's generic-attention cases


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("cls", fr.GENERIC_CLASSES)
def test_generic_attention_emulation_over_the_classes(cls, dtype):
    """attn_generic_kernel's fp32 emulations (its dot products as matrix products, and as the serial chains they are) against
    generic_attn_bound over the classes that kernel is run on, at the shape of the GPU cases.  flash_ref.GENERIC_CLASSES
    names the classes left out, with the ratios the emulations reach there."""
    Tk, Tq = GENERIC_SHAPE
    q, k, v = (x.to(_tdt(dtype)) for x in fr.flash_inputs(cls, Tk, Tq, H, seed=77, prescaled=0))
    lim = torch.full((Tq,), Tk)
    a = pr.generic_attn_ref(q.double(), k.double(), v.double(), H, lim)
    bound = pr.generic_attn_bound(a, dtype)
    for (how, got) in (("matrix products", pr.generic_attn_emulate(q, k, v, H, lim, dtype)),
                       ("serial chains", fr.generic_emulate_serial(q, k, v, H, dtype))):
        r = pr.ratio(got, a["ref"], bound)
        print(f"attn_generic<{'half' if dtype == F16 else 'float'}>/cross/{cls}: emulation ({how}) error / bound = {r:.3f}")
        assert r <= 1.0
    if cls in fr.PEAK_CLASSES:
        pert = fr.flash_ref(q, k, v, H, 0, drop="dominant")[0]
    else:
        pert = pr.generic_attn_ref(q.double(), k.double(), v.double(), H, lim, drop_last=True)["ref"]
    assert pr.ratio(pert, a["ref"], bound) > 1.0
