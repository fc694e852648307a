"""LayerNorm behind the MFMAs (whisper_amd/csrc/kernels.h) on the GPU, kernel by kernel through libwhisper_hip_ktest.so.

Every case runs the chain of one decoder layer:
  first site   LayerNorm projection with its prologue (PRO_LN) that also stores the row means of x0 — the centres;
  producer     a residual projection (EPI_RESID): x1 = x0 + W_p a + b_p in fp32, and beside it fp16(x1 - centre) in
               fragment order;
  consumer     the projection with LayerNorm behind the MFMAs (PRO_LN_POST) on that copy.
Checked against float64: the stored means (1e-5 (|mu| + sigma)), x1 (the GEMV bound of test_kernel_parity_gpu.py), the
fp16 copy (bit for bit the fp32 difference rounded, pad rows untouched), and the consumer's outputs against the true
LayerNorm projection of x1 with the bound of tests/ln_post_ref.py (derived there, checked on the CPU in
tests/test_ln_post_cpu.py).  A perturbed reference (two rows swapped, the last k-term dropped) must miss the bound; inputs,
pad rows and row gaps must stay unwritten; gemv_family must name gemv8 for the new argument sets.  Rows: 9, 15, 16, 17, 23,
24 (two and three row tiles, full and ragged); row mean / std 0 and 30.  The largest error / bound per form is written to
ln_post_parity.json by conftest.write_report (the judged copy: profiles/ln_post_parity.json).
"""
import ctypes
import math

import pytest
import torch

from kernel_lib import hipSuccess, last_form, lib
from ln_post_ref import centred_fp16, ln_post_slack, ln_true
from parity_ref import C_DOT, F16, F32, Buf, _dev, _stream, _ulp

pytestmark = pytest.mark.gpu

PLAIN, LN, COMBINE, LN_POST = 0, 1, 2, 3
STORE, QKV, RESID, GELU = 0, 1, 2, 3
ROWS = [9, 15, 16, 17, 23, 24]
RATIOS = [0.0, 30.0]
REPORT = {}

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _lib():
    h = lib()
    h.wht_gemv_ln_post.restype = _I
    h.wht_gemv_ln_post.argtypes = [_I, _P, _L, _I, _P, _L, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _I, _P, _L, _P, _L,
                                   _P, _P, _L, _P, _I, _P, _P]
    h.wht_gemv_family_ln_post.restype = ctypes.c_char_p
    h.wht_gemv_family_ln_post.argtypes = [_I] * 9
    h.wht_gemv8_ln_post_pays.restype = _I
    h.wht_gemv8_ln_post_pays.argtypes = [_I, _I, _I]
    return h


def _frag_index(R, K, device):
    r = torch.arange(R, device=device).view(-1, 1)
    k = torch.arange(K, device=device).view(1, -1)
    return (((((r >> 3) * (K >> 6) + (k >> 6)) * 64 + 16 * ((k & 31) >> 3) + 8 * ((k >> 5) & 1) + (r & 7)) << 3) + (k & 7))


def _record(form, ratio):
    REPORT[form] = max(REPORT.get(form, 0.0), float(ratio))


def _check(form, got, ref, bound, what):
    got = got.double()
    assert torch.isfinite(got).all(), f"{form} {what}: non-finite output"
    ratio = ((got - ref).abs() / bound).max().item()
    _record(form, ratio)
    assert ratio <= 1.0, f"{form} {what}: error / bound = {ratio:.3f}"


_WEIGHTS = {}


def _weights(N, K, seed, scale=None):
    """fp16 W [N][K] and fp32 bias [N] on the device, made once per shape"""
    key = (N, K, seed)
    if key not in _WEIGHTS:
        g = torch.Generator(device="cpu").manual_seed(seed * 7919 + N * 17 + K)
        W = (torch.randn(N, K, generator=g) * (scale if scale is not None else K ** -0.5)).half().to(_dev())
        b = (torch.randn(N, generator=g) * 0.5).float().to(_dev())
        _WEIGHTS[key] = (W, b)
    return _WEIGHTS[key]


def _chain(R, K, Kp, ratio, seed):
    """first site + producer [K][Kp]; returns (x1 fp32 [R][K] as the kernel left it, the fp16 copy's buffer, its form)"""
    h, dev = _lib(), _dev()
    g = torch.Generator(device="cpu").manual_seed(seed * 104729 + R * 131 + K * 7 + Kp + int(ratio))
    R8 = (R + 7) // 8 * 8
    std = 0.7
    x0 = torch.randn(R, K, generator=g, dtype=torch.float64) * std
    x0 = (x0 - x0.mean(1, keepdim=True) + ratio * x0.std(1, unbiased=False, keepdim=True)).float()

    # ---- first site: PRO_LN (8 features) that stores the row means
    W0, b0 = _weights(8, K, 1)
    xf = Buf(R * K, torch.float32)
    xf.t.copy_(x0.reshape(-1).to(dev))
    cen = Buf(R, torch.float32)
    y0 = Buf(R * 8, torch.float16)
    xf.snapshot()
    assert h.wht_gemv_family_ln_post(1, LN, STORE, R, 8, K, 1, 0, 1) == b"gemv8"
    e = h.wht_gemv_ln_post(LN, None, 0, 0, xf.ptr(), K, None, None, 0, 0, W0.data_ptr(), b0.data_ptr(), 8, K, R, None, cen.ptr(),
                           0, STORE, y0.ptr(), 8, None, 0, None, None, 0, None, 0, None, _stream())
    assert e == hipSuccess, f"first site R={R} K={K}: hipError {e}"
    torch.cuda.synchronize()
    assert last_form().startswith("gemv8/LN/"), last_form()
    assert not xf.changed().any()
    xd0 = x0.double().to(dev)
    mu0, sig0 = xd0.mean(1), xd0.std(1, unbiased=False)
    c = cen.t.clone()
    assert ((c.double() - mu0).abs() <= 1e-5 * (mu0.abs() + sig0)).all(), f"R={R} K={K}: stored means off"
    pre0, _, _ = ln_true(xd0, W0.double(), b0.double())
    assert ((y0.t.view(R, 8).double() - pre0).abs() <= 0.02 * (1 + pre0.abs())).all()      # the launch did its own job too

    # ---- producer: resid = x0 + Wp a + bp, fp16 copy beside it
    Wp, bp = _weights(K, Kp, 2, scale=0.3 * std * Kp ** -0.5)
    a = torch.randn(R, Kp, generator=g).half().to(dev)
    abuf = Buf(R * Kp, torch.float16)
    abuf.t.copy_(a.reshape(-1))
    resid = Buf(R * K, torch.float32)
    resid.t.copy_(x0.reshape(-1).to(dev))
    xh = Buf(R8 * K, torch.float16)                                # pad rows stay NaN
    for b in (abuf, xh, cen):
        b.snapshot()
    assert h.wht_gemv_family_ln_post(1, PLAIN, RESID, R, K, Kp, 1, 1, 1) == b"gemv8"
    e = h.wht_gemv_ln_post(PLAIN, abuf.ptr(), Kp, 0, None, 0, None, None, 0, 0, Wp.data_ptr(), bp.data_ptr(), K, Kp, R, xh.ptr(),
                           cen.ptr(), 0, RESID, None, 0, resid.ptr(), K, None, None, 0, None, 0, None, _stream())
    assert e == hipSuccess, f"producer R={R} N={K} K={Kp}: hipError {e}"
    torch.cuda.synchronize()
    form = last_form()
    assert form.startswith("gemv8/plain/"), form
    assert not abuf.changed().any() and not cen.changed().any(), f"{form}: an input buffer was written"
    x1 = resid.t.view(R, K).clone()
    ad, Wpd = a.double(), Wp.double()
    ref = xd0 + ad @ Wpd.T + bp.double().view(1, -1)
    bound = _ulp(ref, F32) + C_DOT * (ad.abs() @ Wpd.abs().T + bp.double().abs().view(1, -1))
    _check(form + "+xh", x1, ref, bound, f"producer R={R} N={K} K={Kp}")
    drop = ad[:, Kp - 1:Kp] * Wpd[:, Kp - 1].view(1, -1)
    assert (drop.abs() / bound).max().item() > 1.0
    idx = _frag_index(R, K, dev).reshape(-1)
    want = centred_fp16(x1, c).reshape(-1)
    assert torch.equal(xh.t[idx].view(torch.int16), want.view(torch.int16)), f"{form}: fp16 copy is not fp16(x1 - centre)"
    mask = torch.zeros(R8 * K, dtype=torch.bool, device=dev)
    mask[idx] = True
    assert not (xh.changed() & ~mask).any(), f"{form}: fragment-order pad rows written"
    return x1, xh, cen


def _consumer(R, N, K, epi, x1, xh, frag=False, lag=None):
    h, dev = _lib(), _dev()
    R8 = (R + 7) // 8 * 8
    W, bias = _weights(N, K, 3)
    ybuf = kc = vc = pos = lagb = None
    D = N // 3
    if epi == QKV:
        ybuf = Buf(R * D, torch.float16)
        kc, vc = Buf(R * 9 * D, torch.float16), Buf(R * 9 * D, torch.float16)
        pos = torch.tensor([6], dtype=torch.int32, device=dev)
        lagb = torch.tensor(lag, dtype=torch.int32, device=dev)
    else:
        ybuf = Buf(R8 * N if frag else R * N, torch.float16)
    bufs = [b for b in (xh, ybuf, kc, vc) if b is not None]
    for b in bufs:
        b.snapshot()
    Wsnap = W.clone()
    assert h.wht_gemv_family_ln_post(1, LN_POST, epi, R, N, K, 1, 1, 0) == b"gemv8"
    e = h.wht_gemv_ln_post(LN_POST, None, 0, 0, None, 0, None, None, 0, 0, W.data_ptr(), bias.data_ptr(), N, K, R, xh.ptr(), None,
                           int(frag), epi, ybuf.ptr(), D if epi == QKV else N, None, 0, kc.ptr() if kc else None,
                           vc.ptr() if vc else None, 9 * D, pos.data_ptr() if pos is not None else None, D,
                           lagb.data_ptr() if lagb is not None else None, _stream())
    assert e == hipSuccess, f"consumer R={R} N={N} K={K} epi={epi}: hipError {e}"
    torch.cuda.synchronize()
    form = last_form()
    assert form.startswith("gemv8/LNpost/"), form
    assert not xh.changed().any() and torch.equal(W, Wsnap), f"{form}: an input buffer was written"

    xd, Wd, bd = x1.double(), W.double(), bias.double()
    pre, mu, var = ln_true(xd, Wd, bd)
    slack = ln_post_slack(xd, Wd, bd, pre, mu, var)
    ref = pre
    if epi == QKV:
        got = torch.empty(R, N, dtype=torch.float64, device=dev)
        got[:, :D] = ybuf.t.view(R, D).double()
        for name, cb, c0 in (("k", kc, D), ("v", vc, 2 * D)):
            written = cb.changed().view(R, 9, D)
            for r in range(R):
                p = 6 - lag[r]
                assert written[r, p].all() and not written[r, :p].any() and not written[r, p + 1:].any(), \
                    f"{form}: {name} cache of row {r} written outside position {p}"
                got[r, c0:c0 + D] = cb.t.view(R, 9, D)[r, p].double()
    else:
        if epi == GELU:
            ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
            slack = 1.13 * slack + 4.2e-7 + 2.0 ** -22 * pre.abs()          # |gelu'| <= 1.13; the kernel's erf form
        if frag:
            idx = _frag_index(R, N, dev).reshape(-1)
            got = ybuf.t[idx].view(R, N)
            mask = torch.zeros(R8 * N, dtype=torch.bool, device=dev)
            mask[idx] = True
            assert not (ybuf.changed() & ~mask).any(), f"{form}: fragment-order pad rows written"
        else:
            got = ybuf.t.view(R, N)
    bound = _ulp(ref, F16) + slack
    _check(form, got, ref, bound, f"consumer R={R} N={N} K={K} epi={epi}")
    if epi != GELU:
        swapped = ref[[1, 0] + list(range(2, R))]
        assert ((swapped - ref).abs() / bound).max().item() > 1.0, "bound too loose to see two rows swapped"
        xn = (xd - mu) / torch.sqrt(var + 1e-5)
        drop = xn[:, K - 1:K] * Wd[:, K - 1].view(1, -1)
        assert (drop.abs() / bound).max().item() > 1.0, "bound too loose to see the last k-term dropped"


# consumer (N, K), epilogue, fragment-order output, producer K
CASES = [
    (40, 64, STORE, False, 64),
    (24, 320, STORE, False, 64),
    (1032, 384, STORE, False, 1536),
    (1280, 1280, STORE, False, 1280),
    (3840, 1280, QKV, False, 1280),
    (5120, 1280, GELU, True, 5120),
]


@pytest.mark.parametrize("N,K,epi,frag,Kp", CASES)
def test_ln_post_chain(gpu_device, N, K, epi, frag, Kp):
    for R in ROWS:
        for ratio in RATIOS:
            x1, xh, _ = _chain(R, K, Kp, ratio, seed=N)
            _consumer(R, N, K, epi, x1, xh, frag=frag, lag=[r % 3 for r in range(R)] if epi == QKV else None)


def test_ln_post_dispatch(gpu_device):
    """gemv_family of the new argument sets, and where the decode step picks the form"""
    h = _lib()
    fam = h.wht_gemv_family_ln_post
    for R in ROWS:
        assert fam(1, LN_POST, STORE, R, 1280, 1280, 1, 1, 0) == b"gemv8"
        assert fam(1, PLAIN, RESID, R, 1280, 5120, 1, 1, 1) == b"gemv8"
        assert fam(1, COMBINE, RESID, R, 1280, 1280, 1, 1, 1) == b"gemv8"
    for R in (1, 8, 25, 40):                                      # never at <= 8 rows or beyond 24
        assert fam(1, LN_POST, STORE, R, 1280, 1280, 1, 1, 0) == b""
        assert not h.wht_gemv8_ln_post_pays(R, 1280, 1280)
    assert fam(0, LN_POST, STORE, 16, 1280, 1280, 1, 1, 0) == b""           # fp32 engine
    assert fam(1, LN_POST, STORE, 16, 1280, 1280, 0, 1, 0) == b""           # LayerNorm not folded
    assert fam(1, LN_POST, STORE, 16, 1280, 1280, 1, 1, 1) == b""           # a consumer takes no centres
    assert fam(1, PLAIN, RESID, 16, 1288, 1280, 1, 1, 1) == b""             # the copy needs whole 64-column blocks
    assert fam(1, PLAIN, STORE, 16, 1280, 1280, 1, 1, 1) == b""             # only a residual epilogue stores the copy
    # the decode step: the one-slot shapes (gemv.hip, gemv8_ln_post_pays)
    for R in ROWS:
        assert h.wht_gemv8_ln_post_pays(R, 1280, 1280) and h.wht_gemv8_ln_post_pays(R, 1152, 384)
        assert not h.wht_gemv8_ln_post_pays(R, 3840, 1280) and not h.wht_gemv8_ln_post_pays(R, 5120, 1280)


def test_ln_post_report(gpu_device):
    """largest error / bound per form of this module's runs -> ln_post_parity.json by conftest.write_report (the judged copy:
    profiles/ln_post_parity.json)"""
    if not REPORT:                                                 # run alone: one small chain
        x1, xh, _ = _chain(9, 64, 64, 30.0, seed=40)
        _consumer(9, 40, 64, STORE, x1, xh)
    from conftest import write_report
    write_report("ln_post_parity.json", {k: round(v, 4) for k, v in sorted(REPORT.items())})
    assert max(REPORT.values()) <= 1.0
