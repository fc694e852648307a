"""attn_flash_f16_kernel against float64 over wide score ranges, through libwhisper_hip_ktest.so (tests/kernel_lib.py), with
test_kernel_parity_gpu.test_attn_flash's harness and its unchanged bound _ulp(ref, F16) + C_ATT_MFMA * sum p |v| / sum p.

test_attn_flash feeds randn scores, under which the kernel's deferred rescale (the reference maximum of a lane moves only
when a query of its wave has outgrown it by 2^6) fires once per launch or never, nothing underflows and no P is an fp16
subnormal.  The score classes of tests/flash_ref.py reach what it leaves out: a rescale on every tile, lanes that ride through a
firing wave unmoved, a reference held at an early peak with fp16-subnormal P behind it, the ragged tile's mask meeting a
rescale, scores near -144 and +144 (exp2 domain) and a first tile far below the rest.  tests/test_flash_ref_cpu.py shows on
the CPU that an fp32 restatement of the kernel stays inside the bound over all of them and that they reach those branches.

Every case: guard bytes and row gaps unwritten, V^T pad columns 60000 (finite, must not reach the output), the output
finite and within the bound per element, and the bound fails the reference with the dominant key (peak classes) or the last key
dropped.  `equal` is also held to the float64 column mean of v.  The generic attention kernel runs the classes of
flash_ref.GENERIC_CLASSES (which names the ones left out, and why) under its own bound.  The largest error / bound ratio of
every form is written to flash_range_parity.json by conftest.write_report.
"""
import pytest
import torch

import flash_ref as fr
import prefill_align_ref as pr
from kernel_lib import hipSuccess, lib
from parity_ref import C_ATT_MFMA, C_ATT_VALU, F16, F32, Buf, _dev, _stream, _tdt, _ulp

pytestmark = pytest.mark.gpu

REPORT = {}                  # form -> largest error / bound ratio

SMALL, PREFILL, ENCODER = (2, 2, 200, 150), (1, 2, 1500, 64), (1, 2, 1500, 1500)        # (B, H, T, Tq)
CASES = ([(cls,) + SMALL for cls in fr.CLASSES]
         + [(cls,) + PREFILL for cls in ("ramp", "one_lane", "early_peak10", "deep_first", "late_peak")]
         + [(cls,) + ENCODER for cls in ("ramp", "early_peak10")])
GENERIC_SHAPE = (2, 2, 33, 200)                                                         # (R, H, Tq, Tk)


def _check(form, got, ref, bound, what=""):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{form} {what}: non-finite output"
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"{form} {what}: error / bound = {ratio:.3f}")
    REPORT[form] = max(REPORT.get(form, 0.0), float(ratio))
    assert ratio <= 1.0, f"{form} {what}: error / bound = {ratio:.3f}"
    return ratio


def _sensitive(ref, pert, bound, what):
    """the bound must not be vacuous: the perturbed reference fails it somewhere."""
    r = ((pert - ref).abs() / bound).max().item()
    assert r > 1.0, f"bound too loose to see {what} (ratio {r:.3f})"


@pytest.mark.parametrize("prescaled", [0, 1])
@pytest.mark.parametrize("cls,B,H,T,Tq", CASES, ids=[f"{c[0]}-{c[3]}x{c[4]}" for c in CASES])
def test_flash_range(gpu_device, cls, B, H, T, Tq, prescaled):
    dev = _dev()
    D = H * 64
    ld = D + 64
    qkv = [fr.flash_inputs(cls, T, Tq, H, seed=1000 * b + T + Tq + fr.CLASSES.index(cls), prescaled=prescaled) for b in range(B)]
    q, k, v = (torch.stack([x[i] for x in qkv]) for i in range(3))
    vt_ld = (T + 63) // 64 * 64 + 8
    qb, kb = Buf(B * Tq * ld, torch.float16), Buf(B * T * ld, torch.float16)
    qb.t.view(B, Tq, ld)[:, :, :D] = q.to(dev)
    kb.t.view(B, T, ld)[:, :, :D] = k.to(dev)
    vtt = torch.full((B, D, vt_ld), 60000.0).half()           # pad columns: finite
    vtt[:, :, :T] = v.transpose(1, 2)
    vb = Buf(B * D * vt_ld, torch.float16)
    vb.t.copy_(vtt.reshape(-1).to(dev))
    out = Buf(B * Tq * ld, torch.float16)
    for b in (qb, kb, vb, out):
        b.snapshot()
    e = lib().wht_attn_flash_f16(qb.ptr(), ld, Tq * ld, kb.ptr(), ld, T * ld, vb.ptr(), vt_ld, D * vt_ld, out.ptr(), ld,
                                 Tq * ld, B, H, T, prescaled, Tq, _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not qb.changed().any() and not kb.changed().any() and not vb.changed().any(), "an input was written"
    assert not out.changed().view(B, Tq, ld)[:, :, D:].any(), "row gap written"
    got = out.t.view(B, Tq, ld)[:, :, :D].cpu()
    refs = [fr.flash_ref(q[b], k[b], v[b], H, prescaled) for b in range(B)]
    ref = torch.stack([r[0] for r in refs])
    bound = _ulp(ref, F16) + C_ATT_MFMA * torch.stack([r[1] for r in refs])
    form = f"flash/prescaled{prescaled}/{cls}"
    what = f"B={B} H={H} T={T} Tq={Tq}"
    _check(form, got, ref, bound, what)
    pert = torch.stack([fr.flash_ref(q[b], k[b], v[b], H, prescaled, drop=fr.drop_kind(cls))[0] for b in range(B)])
    _sensitive(ref, pert, bound, f"the {fr.drop_kind(cls)} key dropped")
    if cls == "equal":
        mean = v.double().mean(1, keepdim=True).expand(B, Tq, D)
        _check(form, got, mean, _ulp(mean, F16) + C_ATT_MFMA * v.double().abs().mean(1, keepdim=True).expand(B, Tq, D),
               what + " against the column mean of v")


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("cls", fr.GENERIC_CLASSES)
def test_generic_range(gpu_device, cls, dtype):
    """attn_generic_kernel, non-causal over interleaved K / V rows as the prefill cross attention launches it, on the score
    classes whose fp32 emulations stay inside generic_attn_bound (tests/test_flash_ref_cpu.py).  Left out, with the ratio the
    emulations reach (half / float): ramp 2.88 / 5.00, one_lane 0.50 / 2.83, deep 1.91 / 4.00, high 1.91 / 3.55 — the bound
    has no term for the fp32 rounding of a score of 24 to 100 itself — and early_peak12 0.50 / 1.16: 196 tail terms of the
    serial P.V chain, each rounded at the ulp of the dominant fourth term (flash_ref.GENERIC_CLASSES).  The kernel itself
    measured 1.164 there on an MI355X, the figure generic_emulate_serial gives for the same inputs; early_peak10: 0.875."""
    R, H, Tq, Tk = GENERIC_SHAPE
    D, tdt = H * 64, _tdt(dtype)
    o_ld = D + 32
    es = torch.empty((), dtype=tdt).element_size()
    qkv = [fr.flash_inputs(cls, Tk, Tq, H, seed=500 * r + 77 + fr.CLASSES.index(cls), prescaled=0) for r in range(R)]
    q, k, v = (torch.stack([x[i] for x in qkv]).to(tdt) for i in range(3))      # fp16 values: exact in fp32
    qb, kvb = Buf(q.numel(), tdt), Buf(2 * k.numel(), tdt)
    qb.t.copy_(q.reshape(-1).to(_dev()))
    kvb.t.copy_(torch.cat([k, v], 2).reshape(-1).to(_dev()))
    out = Buf(R * Tq * o_ld, tdt)
    for b in (qb, kvb, out):
        b.snapshot()
    e = lib().wht_attn_generic(dtype, R, qb.ptr(), D, Tq * D, kvb.ptr(), 2 * D, Tk * 2 * D, kvb.ptr() + D * es, 2 * D,
                               Tk * 2 * D, out.ptr(), o_ld, Tq * o_ld, H, Tq, Tk, None, 0, 1, _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not qb.changed().any() and not kvb.changed().any(), "an input was written"
    assert not out.changed().view(R, Tq, o_ld)[:, :, D:].any(), "row gap written"
    got = out.t.view(R, Tq, o_ld)[:, :, :D].cpu()
    lim = torch.full((Tq,), Tk)
    refs = [pr.generic_attn_ref(q[r].double(), k[r].double(), v[r].double(), H, lim) for r in range(R)]
    ref = torch.stack([a["ref"] for a in refs])
    bound = torch.stack([pr.generic_attn_bound(a, dtype) for a in refs])
    _check(f"attn_generic<{'half' if dtype == F16 else 'float'}>/cross/{cls}", got, ref, bound, f"Tk={Tk} Tq={Tq}")
    if cls in fr.PEAK_CLASSES:
        pert = torch.stack([fr.flash_ref(q[r], k[r], v[r], H, 0, drop="dominant")[0] for r in range(R)])
    else:
        pert = torch.stack([pr.generic_attn_ref(q[r].double(), k[r].double(), v[r].double(), H, lim, drop_last=True)["ref"]
                            for r in range(R)])
    _sensitive(ref, pert, bound, f"the {fr.drop_kind(cls)} key dropped")


EXPECTED_FORMS = ([f"flash/prescaled{p}/{cls}" for p in (0, 1) for cls in fr.CLASSES]
                  + [f"attn_generic<{t}>/cross/{cls}" for t in ("half", "float") for cls in fr.GENERIC_CLASSES])


def test_coverage_and_report(gpu_device):
    """runs last: every (class, form) pair was recorded, and the largest error / bound ratio of each is written to
    flash_range_parity.json"""
    from conftest import write_report
    write_report("flash_range_parity.json", {"bounds": {"C_ATT_MFMA": C_ATT_MFMA, "C_ATT_VALU": C_ATT_VALU},
                                             "max_ratio": dict(sorted(REPORT.items()))})
    assert sorted(REPORT) == sorted(EXPECTED_FORMS), f"forms not recorded: {sorted(set(EXPECTED_FORMS) - set(REPORT))}"
