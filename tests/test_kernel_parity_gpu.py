"""Per-element parity of the shipped GEMV, decode-attention, GEMM, flash-attention, LayerNorm and copy kernels against a
float64 reference, through libwhisper_hip_ktest.so (tests/kernel_lib.py: the same kernel objects as libwhisper_hip.so).

Reference: torch float64 on the same fp16- / fp32-rounded inputs, rounded to the element type exactly where the kernel
stores an intermediate (read from the kernels):
  GEMV  PRO_PLAIN ........ none (x is the input); output rounded once (fp16 / fp32 store, EPI_RESID and EPI_F32 fp32).
        PRO_LN ........... the normalised rows (LDS / register tile in the element type: gemv_kernel, gemv8_kernel,
                           rows48*, gemv_stream_kernel), then the output.
        PRO_COMBINE ...... the fp16 / fp32 partials [S][R][H][64] (an input here), the merged rows (stored in the element
                           type before the projection), then the output.
  merge_partials ......... the partials (input), then the output.
  decode attention ....... q * 0.125 (exact in fp16), the per-split partials o / l in the element type when splits > 1
                           (split boundaries: ceil(Tk / S) rounded up to the form's key granule), then the output.
  GEMM ................... output only (fp32 accumulation, fp32 epilogue).  flash: output only (P enters the MFMA as
                           fp16: covered by the flash bound below).  LayerNorm: output only.
What is left is fp32 accumulation plus the final rounding.  Per element:

  |y - ref| <= ulp_out(|ref|) + C_DOT * sum_k |w_k x_k|                     (GEMV, GEMM; C_DOT = 2^-20)
  |o - ref| <= ulp_out(|ref|) + C_ATT * sum_j p_j |v_j| / sum_j p_j         (attention; C_ATT per form, below)

plus, for PRO_LN, sum_k |w_k| * (the ulp of x^_k where x^_k lies within the kernel's fp32 LayerNorm error of a rounding
boundary of the element type, else that error itself), and for GELU the activation's own error (4.2e-7 + 2^-22 |pre|)
after the 1.13 Lipschitz factor.  Every case also checks that its bound is not vacuous: a perturbed reference (the last
k-term dropped, two rows swapped, the last key dropped) must fail it.  The largest measured error / bound ratio of every
form is written to kernel_parity.json by conftest.write_report.

Poison: every buffer is allocated with guard bytes around it, and everything a launch must not write (guards, row gaps
of strided outputs, fragment-order pad rows, cache positions other than the appended one) is filled with 0xFF (NaN in
fp16 and fp32) and must come back unchanged.  Declared don't-care inputs (x columns beyond K, fragment-order pad rows,
K / V cache slots at or beyond the cached length) hold NaN, vt pad columns hold large finite values (the contract says
finite); the kept outputs must be finite and within the bound.
"""
import math

import pytest
import torch

from kernel_lib import family_of_tag, gemv_family, hipErrorInvalidValue, hipSuccess, last_form, lib
from parity_ref import (C_ATT_MFMA, C_ATT_VALU, C_DOT, F16, F32, GUARD, Buf, _dev, _flip_slack, _merge_ref,  # noqa: F401
                        _r, _stream, _tdt, _ulp, attn_bound, attn_ref, ln_rows_ref)

pytestmark = pytest.mark.gpu

PLAIN, LN, COMBINE = 0, 1, 2
STORE, QKV, RESID, GELU, EPI_F32 = 0, 1, 2, 3, 4

REPORT = {}                  # form -> largest error / bound ratio
FORMS = set()                # every form tag seen


def _record(form, ratio):
    FORMS.add(form)
    REPORT[form] = max(REPORT.get(form, 0.0), float(ratio))


def _check(form, got, ref, bound, what=""):
    got = got.double()
    assert torch.isfinite(got).all(), f"{form} {what}: non-finite output"
    ratio = ((got - ref).abs() / bound).max().item()
    _record(form, ratio)
    assert ratio <= 1.0, f"{form} {what}: error / bound = {ratio:.3f}"
    return ratio


def _sensitive(ref, pert, bound, what):
    """the bound must not be vacuous: the perturbed reference fails it somewhere."""
    r = ((pert - ref).abs() / bound).max().item()
    assert r > 1.0, f"bound too loose to see {what} (ratio {r:.3f})"


def _frag_index(R, K, device):
    """element offsets [R][K] of x[r][k] in a fragment-order activation (kernels.h frag_index)"""
    r = torch.arange(R, device=device).view(-1, 1)
    k = torch.arange(K, device=device).view(1, -1)
    return (((((r >> 3) * (K >> 6) + (k >> 6)) * 64 + 16 * ((k & 31) >> 3) + 8 * ((k >> 5) & 1) + (r & 7)) << 3) + (k & 7))


# ----------------------------------------------------------------------------------------------------------- GEMV
def _gemv_case(dtype, R, N, K, pro=PLAIN, epi=STORE, bias=True, ln_folded=True, splits=1, H=None, x_ld=None, y_ld=None,
               resid_ld=None, frag=False, mean=0.0, std=1.0, bias_vals=None, w_scale=None, lag=None, seed=0):
    """one launch_gemv against float64; returns (form, the kept outputs as [R][N] in the output type, error / bound)"""
    g = torch.Generator(device="cpu").manual_seed(seed * 7919 + R * 131 + N * 17 + K + pro * 5 + epi)
    dev, tdt = _dev(), _tdt(dtype)
    x_ld = x_ld or K
    W = (torch.randn(N, K, generator=g) * (w_scale if w_scale is not None else K ** -0.5)).to(tdt).to(dev)
    Wd = W.double()
    bvec = None
    if bias:
        bvec = bias_vals.float().to(dev) if bias_vals is not None else (torch.randn(N, generator=g) * 0.5).float().to(dev)
    R8 = (R + 7) // 8 * 8

    # ---- prologue inputs and the float64 rows the kernel multiplies
    xbuf = xf = lnw = lnb = po = pml = None
    ln_slack = None
    if pro == PLAIN:
        xv = torch.randn(R, K, generator=g).to(tdt)
        if frag:
            xbuf = Buf(R8 * K, tdt)                                # pad rows 8*ceil(R/8) stay NaN
            idx = _frag_index(R, K, "cpu").reshape(-1).to(dev)
            xbuf.t[idx] = xv.reshape(-1).to(dev)
        else:
            xbuf = Buf(R * x_ld, tdt)                              # columns K..x_ld-1 stay NaN
            xbuf.t.view(R, x_ld)[:, :K] = xv.to(dev)
        X = xv.double().to(dev)
    elif pro == LN:
        xf_ld = x_ld
        xv = (torch.randn(R, K, generator=g, dtype=torch.float64) * std + mean).float()
        xf = Buf(R * xf_ld, torch.float32)
        xf.t.view(R, xf_ld)[:, :K] = xv.to(dev)
        if ln_folded:
            lw, lb = torch.ones(K), torch.zeros(K)
        else:
            lw, lb = 1.0 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        lnw, lnb = lw.float().to(dev), lb.float().to(dev)
        xn, X, delta, _, _ = ln_rows_ref(xv.double().to(dev), lnw, lnb, dtype)    # parity_ref: the kernel's fp32 LayerNorm error
        ln_slack = _flip_slack(xn, X, delta, Wd.abs(), dtype)
    else:
        H = K // 64
        po = Buf(splits * R * H * 64, tdt)
        pml = Buf(splits * R * H * 2, torch.float32)
        o = torch.randn(splits, R, H, 64, generator=g).to(tdt)
        m = torch.randn(splits, R, H, generator=g).float() * 3
        l = (torch.rand(splits, R, H, generator=g) * 20 + 0.5).float()
        if splits > 1:                                             # an empty split: m = -inf, l = 0 (its o is 0)
            m[splits - 1, 0, 0] = float("-inf")
            l[splits - 1, 0, 0] = 0.0
            o[splits - 1, 0, 0] = 0
        po.t.copy_(o.reshape(-1).to(dev))
        pml.t.view(splits, R, H, 2)[..., 0] = m.to(dev)
        pml.t.view(splits, R, H, 2)[..., 1] = l.to(dev)
        xm, merr = _merge_ref(o, m, l)                              # [R][H][64]
        xm, merr = xm.reshape(R, K).to(dev), merr.reshape(R, K).to(dev)
        X = _r(xm, dtype)
        ln_slack = _flip_slack(xm, X, merr, Wd.abs(), dtype)      # the merged rows are stored in the element type

    # ---- outputs
    ybuf = resid = kc = vc = pos = lagb = None
    y_ld = y_ld or N
    if epi in (STORE, GELU):
        ybuf = Buf(R8 * N if frag else R * y_ld, tdt)
    elif epi == EPI_F32:
        ybuf = Buf(R * y_ld, torch.float32)
    elif epi == RESID:
        resid_ld = resid_ld or N
        resid = Buf(R * resid_ld, torch.float32)
        r0 = torch.randn(R, N, generator=g).float() * 4
        resid.t.view(R, resid_ld)[:, :N] = r0.to(dev)
    elif epi == QKV:
        D = N // 3
        n_ctx = 9
        ybuf = Buf(R * y_ld, tdt)
        kc, vc = Buf(R * n_ctx * D, tdt), Buf(R * n_ctx * D, tdt)
        pos = torch.tensor([6], dtype=torch.int32, device=dev)
        if lag is not None:
            lagb = torch.tensor(lag, dtype=torch.int32, device=dev)
    bump = torch.tensor([5, 7], dtype=torch.int32, device=dev)
    bufs = [b for b in (xbuf, xf, po, pml, ybuf, resid, kc, vc) if b is not None]
    for b in bufs:
        b.snapshot()

    lib().wht_clear_form()
    e = lib().wht_gemv(dtype, pro, xbuf.ptr() if xbuf else None, x_ld, xf.ptr() if xf else None, x_ld,
                       lnw.data_ptr() if lnw is not None else None, lnb.data_ptr() if lnb is not None else None,
                       1 if ln_folded else 0, po.ptr() if po else None, pml.ptr() if pml else None, splits, H or 0,
                       W.data_ptr(), bvec.data_ptr() if bvec is not None else None, N, K, R, int(frag and pro == PLAIN),
                       int(frag and epi in (STORE, GELU)), epi, ybuf.ptr() if ybuf else None, y_ld,
                       resid.ptr() if resid else None, resid_ld or 0, kc.ptr() if kc else None, vc.ptr() if vc else None,
                       9 * (N // 3), pos.data_ptr() if pos is not None else None, N // 3,
                       lagb.data_ptr() if lagb is not None else None, bump.data_ptr(), 3, bump.data_ptr() + 4, _stream())
    assert e == hipSuccess, f"launch_gemv R={R} N={N} K={K} pro={pro} epi={epi}: hipError {e}"
    torch.cuda.synchronize()
    form = last_form()
    assert form, "no form tag"
    assert gemv_family(dtype, pro, epi, R, N, K, x_ld, int(ln_folded), int(bias), splits, H or 0, frag) == family_of_tag(form)
    assert bump.tolist() == [8, 8], f"{form}: bump / bump2 moved {bump.tolist()} (want [8, 8])"
    for b in (xbuf, xf, po, pml):                                  # inputs are not written
        if b is not None:
            assert not b.changed().any(), f"{form}: an input buffer was written"

    # ---- float64 reference of the projection
    pre = X @ Wd.T + (bvec.double().view(1, -1) if bvec is not None else 0.0)
    sabs = X.abs() @ Wd.abs().T + (bvec.double().abs().view(1, -1) if bvec is not None else 0.0)
    slack = C_DOT * sabs + (ln_slack if ln_slack is not None else 0.0)
    drop = X[:, K - 1:K] * Wd[:, K - 1].view(1, -1)                # the last k-term of every output

    if epi == RESID:
        r0d = r0.double().to(dev)
        ref = r0d + pre
        got = resid.t.view(R, resid_ld)[:, :N]
        bound = _ulp(ref, F32) + slack
        written = resid.changed().view(R, resid_ld)
        assert not written[:, N:].any(), f"{form}: residual row gap written"
    elif epi == QKV:
        D = N // 3
        ref = pre
        lg = torch.tensor(lag if lag is not None else [0] * R, device=dev)
        got = torch.empty(R, N, dtype=torch.float64, device=dev)
        got[:, :D] = ybuf.t.view(R, y_ld)[:, :D].double()
        for name, cb, c0 in (("k", kc, D), ("v", vc, 2 * D)):
            written = cb.changed().view(R, 9, D)
            for r in range(R):
                p = 6 - int(lg[r])
                assert written[r, p].all() and not written[r, :p].any() and not written[r, p + 1:].any(), \
                    f"{form}: {name} cache of row {r} written outside position {p}"
                got[r, c0:c0 + D] = cb.t.view(R, 9, D)[r, p].double()
        assert not ybuf.changed().view(R, y_ld)[:, D:].any(), f"{form}: q rows written beyond D"
        bound = _ulp(ref, dtype) + slack
    else:
        ref = pre
        if epi == GELU:
            ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
            slack = 1.13 * slack + 4.2e-7 + 2.0 ** -22 * pre.abs()
        odt = F32 if epi == EPI_F32 else dtype
        bound = _ulp(ref, odt) + slack
        if frag and epi in (STORE, GELU):
            idx = _frag_index(R, N, "cpu").to(dev)
            got = ybuf.t[idx.reshape(-1)].view(R, N)
            written = ybuf.changed()
            mask = torch.zeros_like(written)
            mask[idx.reshape(-1)] = True
            assert not (written & ~mask).any(), f"{form}: fragment-order pad rows written"
        else:
            got = ybuf.t.view(R, y_ld)[:, :N]
            written = ybuf.changed().view(R, y_ld)
            assert not written[:, N:].any(), f"{form}: output row gap written"
    ratio = _check(form, got, ref, bound, f"R={R} N={N} K={K} pro={pro} epi={epi} dt={dtype}")
    if epi != GELU:
        if pro == LN and abs(mean) > 1 and R >= 2:
            _sensitive(ref, ref[[1, 0] + list(range(2, R))], bound, "two rows swapped")
        else:
            _sensitive(ref, ref - drop, bound, "the last k-term dropped")
    return form, got, ratio


GEMV_R = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 40, 47, 48, 49, 96, 97]
GEMV_D = [384, 512, 768, 1024, 1280]


def _shapes(D):
    return [(D, D), (3 * D, D), (4 * D, D), (D, 4 * D)]


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("D", GEMV_D)
def test_gemv_released_shapes(gpu_device, dtype, D):
    """every R of GEMV_R x the four projection shapes of width D, PRO_PLAIN + EPI_STORE and folded PRO_LN (K <= 1280)"""
    Rs = GEMV_R if D in (384, 1280) else [1, 5, 8, 16, 24, 40, 49, 97]
    for R in Rs:
        for (N, K) in _shapes(D):
            _gemv_case(dtype, R, N, K, PLAIN, STORE)
            if K <= 1280:
                _gemv_case(dtype, R, N, K, LN, STORE if N != 3 * D else QKV, lag=[r % 3 for r in range(R)] if N == 3 * D else None)


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("R", [1, 8, 17, 24, 40])
@pytest.mark.parametrize("N", [51864, 51866])
def test_gemv_logits(gpu_device, dtype, R, N):
    """tied logits: LayerNorm (not folded) + EPI_F32 without bias (the streaming forms)"""
    for K in (384, 1280):
        _gemv_case(dtype, R, N, K, LN, EPI_F32, bias=False, ln_folded=False)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_gemv_tails_strides_epilogues(gpu_device, dtype):
    """N not a multiple of 8 / 16 / 64, K a multiple of 64 but not of 128, padded strides, every epilogue, unfolded LN"""
    for R in (1, 3, 8, 9, 16, 24, 25, 48):
        for N in (8, 72, 100, 1000, 1284, 2056):
            for K in (64, 192, 384, 1344):
                if dtype == F32 and K % 32:
                    continue
                _gemv_case(dtype, R, N, K, PLAIN, STORE, x_ld=K + 72, y_ld=N + 8, bias=(N % 2 == 0))
        for (N, K) in ((512, 512), (2048, 512), (1280, 5120), (1544, 384)):
            _gemv_case(dtype, R, N, K, PLAIN, RESID, resid_ld=N + 4)
            _gemv_case(dtype, R, N, K, PLAIN, GELU)
            if K <= 1280:
                _gemv_case(dtype, R, N, K, LN, GELU, ln_folded=(R % 2 == 0))
                _gemv_case(dtype, R, N, K, LN, RESID, ln_folded=False, x_ld=K + 4, resid_ld=N + 4)
                _gemv_case(dtype, R, N, K, LN, EPI_F32, y_ld=N + 4)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_gemv_combine(gpu_device, dtype):
    """PRO_COMBINE with 1 .. 4 splits (an empty split m = -inf, l = 0 in each), H = 6 / 20"""
    for R in (1, 2, 8, 9, 16, 17, 24, 40):
        for H in (6, 20):
            for S in (1, 2, 3, 4):
                for N in (H * 64, 2 * H * 64):
                    _gemv_case(dtype, R, N, H * 64, COMBINE, STORE, splits=S, H=H)


def test_gemv_large_mean_ln_and_gelu_sweep(gpu_device):
    """LayerNorm rows of mean 50, std 0.05; GELU pre-activations swept over [-12, 12] through the bias"""
    for dtype in (F16, F32):
        for R in (2, 8, 24, 40):
            for (N, K) in ((1280, 1280), (3840, 1280), (5120, 1280), (1536, 384)):
                _gemv_case(dtype, R, N, K, LN, STORE, mean=50.0, std=0.05, ln_folded=(N != 1536))
        for R in (1, 8, 16, 40):
            bias = torch.linspace(-12.0, 12.0, 4096)
            _gemv_case(dtype, R, 4096, 1024, PLAIN, GELU, bias_vals=bias, w_scale=1e-3)
            _gemv_case(dtype, R, 4096, 1024, LN, GELU, bias_vals=bias, w_scale=1e-3)


def test_gemv_fragment_order_bit_exact(gpu_device):
    """wherever gemv8_will_run: x_frag / y_frag launches equal the row-major launch bit for bit (replaces the
    tools/probe_gemv8 PROBE_FRAG=1 check of DESIGN §4); pad rows hold NaN and are never written"""
    n = 0
    for R in (1, 3, 8, 9, 15, 16, 17, 24):
        for (N, K) in ((384, 384), (1536, 384), (1280, 1280), (5120, 1280), (1280, 5120), (3840, 1280)):
            if not lib().wht_gemv8_will_run(R, N, K, PLAIN):
                continue
            for epi in (STORE, GELU):
                _, row, _ = _gemv_case(F16, R, N, K, PLAIN, epi, seed=3)
                _, frg, _ = _gemv_case(F16, R, N, K, PLAIN, epi, seed=3, frag=True)
                assert torch.equal(row.view(torch.int16), frg.view(torch.int16)), (R, N, K, epi)
                n += 1
    assert n >= 20


# ------------------------------------------------------------------------------------------------ merge partials
@pytest.mark.parametrize("dtype", [F16, F32])
def test_merge_partials(gpu_device, dtype):
    dev, tdt = _dev(), _tdt(dtype)
    for S in range(1, 17):
        for (R, H) in ((1, 6), (7, 20), (24, 20)):
            for frag in ((False, True) if dtype == F16 else (False,)):
                g = torch.Generator().manual_seed(S * 100 + R + H)
                o = torch.randn(S, R, H, 64, generator=g).to(tdt)
                m = torch.randn(S, R, H, generator=g) * 4
                l = torch.rand(S, R, H, generator=g) * 30 + 0.5
                if S > 1:
                    m[S - 1, :, 0] = float("-inf"); l[S - 1, :, 0] = 0; o[S - 1, :, 0] = 0
                po, pml = Buf(S * R * H * 64, tdt), Buf(S * R * H * 2, torch.float32)
                po.t.copy_(o.reshape(-1).to(dev))
                pml.t.view(S, R, H, 2)[..., 0] = m.to(dev)
                pml.t.view(S, R, H, 2)[..., 1] = l.to(dev)
                R8, K = (R + 7) // 8 * 8, H * 64
                o_ld = K + 16
                out = Buf(R8 * K if frag else R * o_ld, tdt)
                out.snapshot()
                lib().wht_clear_form()
                e = lib().wht_merge_partials(po.ptr(), pml.ptr(), S, R, H, out.ptr(), o_ld, dtype, int(frag), _stream())
                assert e == hipSuccess
                torch.cuda.synchronize()
                form = last_form()
                ref, merr = _merge_ref(o, m, l)
                ref, merr = ref.reshape(R, K).to(dev), merr.reshape(R, K).to(dev)
                md, ld = m.double(), l.double()
                w = torch.where(torch.isinf(md), torch.zeros_like(md), torch.exp(md - md.max(0).values)) * ld
                w = w / w.sum(0)
                if frag:
                    idx = _frag_index(R, K, "cpu").reshape(-1).to(dev)
                    got = out.t[idx].view(R, K)
                    mask = torch.zeros(out.t.numel(), dtype=torch.bool, device=dev); mask[idx] = True
                    assert not (out.changed() & ~mask).any(), "pad rows written"
                else:
                    got = out.t.view(R, o_ld)[:, :K]
                    assert not out.changed().view(R, o_ld)[:, K:].any(), "row gap written"
                bound = _ulp(ref, dtype) + merr
                _check(form, got, ref, bound, f"S={S} R={R} H={H}")
                if S > 1:       # drop split 0
                    w2 = w.clone(); w2[0] = 0; w2 = w2 / w2.sum(0).clamp_min(1e-300)
                    pert = (w2.unsqueeze(-1) * o.double()).sum(0).reshape(R, K).to(dev)
                    _sensitive(ref, pert, bound, "a split dropped")


# --------------------------------------------------------------------------------------------- decode attention
def _granule(form, dtype):
    unit = 8 if dtype == F16 else 4
    if form.startswith("attn/rounds"):
        return 4 * unit
    if form.startswith("attn/self") or form.startswith("attn/group<"):
        return 8 * unit
    return 128                                                     # group_diag / group_mfma


def _attn_case(dtype, H, R, Tk, splits, kv_group=1, vt=False, vt_short=False, kv_hs=0, o_frag=False, self_len=None,
               lags=None, len_plus=1, merge=False, peak=0.0, seed=0):
    """one launch_attn_decode (+ launch_merge_partials when splits > 1 and no in-launch merge) against float64"""
    dev, tdt = _dev(), _tdt(dtype)
    g = torch.Generator().manual_seed(seed * 31 + H * 7 + R * 3 + Tk + splits * 1000 + kv_group * 97)
    B = R // kv_group
    D = H * 64
    hs = kv_hs or 64
    cap = Tk if self_len is None else 12 * 64 if Tk <= 12 * 64 else Tk         # cache rows hold n_ctx positions
    k_ld = (H - 1) * hs + 64 + (8 if kv_hs else 0)
    k_bs = cap * k_ld
    q = torch.randn(R, D, generator=g).to(tdt)
    kk = torch.randn(B, cap, k_ld, generator=g).to(tdt)
    vv = torch.randn(B, cap, k_ld, generator=g).to(tdt)
    if peak:
        # a few keys per (audio, head) aligned with the queries: logits up to +-peak
        for b in range(B):
            for h in range(H):
                j = int(torch.randint(0, Tk, (1,), generator=g))
                qh = q[b * kv_group, h * 64:(h + 1) * 64].double()
                kk[b, j, h * hs:h * hs + 64] = (qh / qh.norm() * peak / 0.125 / qh.norm()).to(tdt)
    lens = [Tk] * R
    if self_len is not None:
        lens = [Tk - (lags[r] if lags else 0) for r in range(R)]
        for r in range(R):                                       # slots at / beyond the cached length: NaN
            kk[r, lens[r]:] = float("nan"); vv[r, lens[r]:] = float("nan")
    kb, vb, qb = Buf(B * k_bs, tdt), Buf(B * k_bs, tdt), Buf(R * D, tdt)
    kb.t.copy_(kk.reshape(-1).to(dev)); vb.t.copy_(vv.reshape(-1).to(dev)); qb.t.copy_(q.reshape(-1).to(dev))
    vtb, vt_ld = None, 0
    if vt:
        chunk = (Tk + splits - 1) // splits
        vt_ld = splits * ((chunk + 127) // 128 * 128) - (1 if vt_short else 0)
        vtt = torch.full((B, H * 64, vt_ld), 60000.0 if dtype == F16 else 1e30).to(tdt)   # pad columns: finite
        for h in range(H):
            vtt[:, h * 64:(h + 1) * 64, :min(Tk, vt_ld)] = vv[:, :min(Tk, vt_ld), h * hs:h * hs + 64].transpose(1, 2)
        vtb = Buf(B * H * 64 * vt_ld, tdt)
        vtb.t.copy_(vtt.reshape(-1).to(dev))
    R8 = (R + 7) // 8 * 8
    o_ld = D + 64
    out = Buf(R8 * D if o_frag else R * o_ld, tdt)
    po = Buf(splits * R * H * 64, tdt) if splits > 1 else None
    pml = Buf(splits * R * H * 2, torch.float32) if splits > 1 else None
    cnt = torch.zeros(R * H, dtype=torch.int32, device=dev) if merge else None
    dlen = torch.tensor([Tk - len_plus], dtype=torch.int32, device=dev) if self_len is not None else None
    lagt = torch.tensor(lags, dtype=torch.int32, device=dev) if lags else None
    for b in (kb, vb, qb, out) + ((vtb,) if vtb else ()):
        b.snapshot()

    def launch():
        lib().wht_clear_form()
        e = lib().wht_attn_decode(dtype, qb.ptr(), D, kb.ptr(), k_ld, k_bs, vb.ptr(), k_ld, k_bs, kv_hs, H, R, kv_group, Tk,
                                  dlen.data_ptr() if dlen is not None else None, len_plus,
                                  lagt.data_ptr() if lagt is not None else None, splits, out.ptr(), o_ld, int(o_frag),
                                  po.ptr() if po else None, pml.ptr() if pml else None,
                                  cnt.data_ptr() if cnt is not None else None, vtb.ptr() if vtb else None, vt_ld,
                                  H * 64 * vt_ld, _stream())
        assert e == hipSuccess, f"launch_attn_decode H={H} R={R} Tk={Tk} S={splits} G={kv_group}: hipError {e}"
        f = last_form()
        if splits > 1 and not merge:
            e = lib().wht_merge_partials(po.ptr(), pml.ptr(), splits, R, H, out.ptr(), o_ld, dtype, int(o_frag), _stream())
            assert e == hipSuccess
        torch.cuda.synchronize()
        return f

    form = launch()
    for b in (kb, vb, qb) + ((vtb,) if vtb else ()):
        assert not b.changed().any(), f"{form}: an input was written"
    if o_frag:
        idx = _frag_index(R, D, "cpu").reshape(-1).to(dev)
        got = out.t[idx].view(R, D)
        mask = torch.zeros(out.t.numel(), dtype=torch.bool, device=dev); mask[idx] = True
        assert not (out.changed() & ~mask).any(), f"{form}: pad rows written"
    else:
        got = out.t.view(R, o_ld)[:, :D]
        assert not out.changed().view(R, o_ld)[:, D:].any(), f"{form}: row gap written"
    if merge:
        assert (cnt == 0).all(), f"{form}: merge tickets not back at 0"
        first = got.clone()
        launch()
        second = (out.t[idx].view(R, D) if o_frag else out.t.view(R, o_ld)[:, :D])
        assert torch.equal(first.view(torch.int16), second.view(torch.int16)), f"{form}: two launches differ"
        assert (cnt == 0).all()

    # ---- float64 reference with the kernel's split boundaries and fp16 / fp32 partials
    gran = _granule(form, dtype)
    qs = _r(q.double() * 0.125, dtype)
    a = attn_ref(qs, lambda r, h: (kk[r // kv_group, :, h * hs:h * hs + 64].double(), vv[r // kv_group, :, h * hs:h * hs + 64].double()),
                 lens, splits, gran, dtype, H, peak=bool(peak))
    c = C_ATT_MFMA if ("diag" in form or "mfma" in form) else C_ATT_VALU
    ref, pert, bound = a["ref"].to(dev), a["pert"].to(dev), attn_bound(a, splits, c, dtype).to(dev)
    _check(form + ("/merge" if merge else ""), got, ref, bound, f"H={H} R={R} Tk={Tk} S={splits} G={kv_group}")
    if min(lens) >= 2:
        _sensitive(ref, pert, bound, "the last key dropped")
    return form


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("H", [6, 20])
def test_attn_decode_cross(gpu_device, dtype, H):
    """fixed Tk (cross attention): Tk at the 1 / 64 / capacity edges, 448 and 1500, splits 1 .. 16 (empty splits where
    Tk < splits), the 8 / 9, 12 / 13 and 16 round boundaries of the chunk"""
    cap = lib().wht_attn_decode_capacity(dtype)
    unit = 8 if dtype == F16 else 4
    tks = [1, 2, 63, 64, 65, cap - 1, cap, 448, 1500]
    for Tk in tks:
        for S in (1, 2, 3, 4, 5, 8, 16):
            if -(-Tk // S) > 16 * 4 * unit:
                continue
            _attn_case(dtype, H, 2, Tk, S)
    # rounds of 4 x unit keys per split: 8 / 9, 12 / 13, 16 rounds
    for rounds in (8, 9, 12, 13, 16):
        _attn_case(dtype, H, 3, rounds * 4 * unit, 1)
        _attn_case(dtype, H, 2, rounds * 4 * unit * 3 - 5, 3)
    _attn_case(dtype, H, 4, 1500, 4 if dtype == F16 else 8, peak=30.0)
    _attn_case(dtype, H, 4, 300, 1 if dtype == F16 else 2, peak=30.0)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_attn_decode_self_and_strides(gpu_device, dtype):
    """self attention (d_len + len_plus, per-row lag, NaN past each row's length), head stride kv_hs, o_frag"""
    cap = lib().wht_attn_decode_capacity(dtype)
    for H in (6, 20):
        for Tk in (1, 2, 63, 64, 65, cap - 1, cap, 448):
            lags = [0, 1, 0, 2] if Tk > 2 else None
            s_min = -(-Tk // cap)                                   # callers size splits with the capacity
            if s_min == 1:
                _attn_case(dtype, H, 4, Tk, 1, self_len=True, lags=lags)          # the eager one-split path
            if Tk >= 64:
                _attn_case(dtype, H, 4, Tk, max(3, s_min), self_len=True, lags=lags)
        _attn_case(dtype, H, 3, 1500, 3 if dtype == F16 else 6, kv_hs=128)
        _attn_case(dtype, H, 3, 500, 1 if dtype == F16 else 2, kv_hs=96)
        if dtype == F16:
            _attn_case(dtype, H, 9, 1500, 3, o_frag=True)
            _attn_case(dtype, H, 5, 300, 1, o_frag=True)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_attn_decode_beam_groups(gpu_device, dtype):
    """kv_group 2 / 5 / 8 with vt (diag and MFMA forms, fp16) and without it; vt_ld one short of the padded key count
    falls to the vector-ALU group form"""
    for G in (2, 5, 8):
        for (Tk, S) in ((1, 1), (65, 1), (300, 1), (448, 1), (1500, 3), (1500, 4), (700, 16)):
            if -(-Tk // S) > 16 * 4 * (8 if dtype == F16 else 4):
                continue                                           # beyond one split's register tile (callers never ask)
            for H in (6, 20):
                _attn_case(dtype, H, G * 2, Tk, S, kv_group=G)
                if dtype == F16:
                    _attn_case(dtype, H, G * 2, Tk, S, kv_group=G, vt=True)
                    _attn_case(dtype, H, G * 2, Tk, S, kv_group=G, vt=True, vt_short=True)


def test_attn_decode_inlaunch_merge(gpu_device):
    """merge_cnt with 2 / 3 / 4 splits: tickets back at 0, two launches bit-identical, o_frag"""
    for S in (2, 3, 4):
        for H in (6, 20):
            for R in (1, 8, 16):
                _attn_case(F16, H, R, 1000 if S == 2 else 1500, S, merge=True)
                _attn_case(F16, H, R, 1000 if S == 2 else 1500, S, merge=True, o_frag=True)
                _attn_case(F16, H, R, 100, S, merge=True, self_len=True, lags=None)


# --------------------------------------------------------------------------------------------------------- GEMM
def _gemm_case(dtype, M, N, K, out_f32=False, bias=0, res_mod=None, resid=False, act=0, batch=1, lda=None, ldc=None,
               seed=0, bias_vals=None, w_scale=None):
    """launch_gemm: C = act(A W^T + bias) (+ res[m % res_mod]); bias 1 = per n, 2 = per m"""
    dev, tdt = _dev(), _tdt(dtype)
    g = torch.Generator().manual_seed(seed + M * 3 + N * 5 + K * 7 + bias * 11 + act * 13 + batch)
    lda, ldc = lda or K, ldc or N
    odt = torch.float32 if (out_f32 or dtype == F32) else tdt
    A = Buf(batch * M * lda, tdt)
    av = torch.randn(batch, M, K, generator=g).to(tdt)
    A.t.view(batch, M, lda)[:, :, :K] = av.to(dev)
    W = (torch.randn(batch, N, K, generator=g) * (w_scale if w_scale is not None else K ** -0.5)).to(tdt).to(dev)
    bv = None
    if bias:
        bv = (torch.randn(N if bias == 1 else M, generator=g) * 0.5).float().to(dev)
        if bias_vals is not None:
            bv = bias_vals.float().to(dev)
    rv, rrows = None, 0
    if resid:
        rrows = res_mod or M
        rv = (torch.randn(batch, rrows, N, generator=g) * 2).float().to(dev)
    C = Buf(batch * M * ldc, odt)
    C.snapshot(); A.snapshot()
    lib().wht_clear_form()
    e = lib().wht_gemm(dtype, int(out_f32), batch, A.ptr(), lda, M * lda, W.data_ptr(), K, N * K, C.ptr(), ldc, M * ldc,
                       bv.data_ptr() if bv is not None else None, int(bias == 2), rv.data_ptr() if rv is not None else None,
                       N, rrows * N, res_mod or 0, act, M, N, K, _stream())
    assert e == hipSuccess, f"launch_gemm M={M} N={N} K={K}: hipError {e}"
    torch.cuda.synchronize()
    form = last_form()
    assert not A.changed().any()
    written = C.changed().view(batch, M, ldc)
    assert not written[:, :, N:].any(), f"{form}: row gap written"
    Ad, Wd = av.double().to(dev), W.double()
    pre = Ad @ Wd.transpose(1, 2)
    sabs = Ad.abs() @ Wd.abs().transpose(1, 2)
    if bv is not None:
        bb = bv.double().view(1, 1, -1) if bias == 1 else bv.double().view(1, -1, 1)
        pre, sabs = pre + bb, sabs + bb.abs()
    slack = C_DOT * sabs
    ref = pre
    if act:
        ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        slack = 1.13 * slack + 4.2e-7 + 2.0 ** -22 * pre.abs()
    if rv is not None:
        idx = torch.arange(M, device=dev) % rrows
        ref = ref + rv.double()[:, idx]
    got = C.t.view(batch, M, ldc)[:, :, :N]
    bound = _ulp(ref, F32 if odt == torch.float32 else F16) + slack
    _check(form, got, ref, bound, f"M={M} N={N} K={K} dt={dtype} f32={out_f32} bias={bias} act={act} res={resid}")
    if not act:
        _sensitive(ref, ref - Ad[:, :, K - 1:K] * Wd[:, :, K - 1].unsqueeze(1), bound, "the last k-term dropped")
    return form


def test_gemm(gpu_device):
    """the row kernel (fp16 in / out, no residual, large M x N) and every launch_shape tiling; M from 1 to 12000, N tails,
    both bias modes, residual with res_mod, GELU, out_f32, batch strides"""
    for M in (1, 17, 1500, 3000, 12000):
        for (N, K) in ((1280, 1280), (3840, 1280), (5120, 1280), (1280, 5120), (384, 384), (1536, 384), (1284, 640)):
            if M * N * K > 12000 * 1280 * 1280:
                continue
            _gemm_case(F16, M, N, K, bias=1)
            if M >= 1500:
                _gemm_case(F16, M, N, K, bias=1, act=1)
                _gemm_case(F16, M, N, K, bias=2)
                _gemm_case(F16, M, N, K, bias=1, resid=True, res_mod=(1500 if M % 1500 == 0 else None))
                _gemm_case(F16, M, N, K, out_f32=True)
    for M in (1, 17, 300, 1500):
        for (N, K) in ((384, 384), (1000, 256), (1536, 384), (4, 64)):
            _gemm_case(F16, M, N, K, bias=1, act=(M % 2))
            _gemm_case(F16, M, N, K, bias=1, resid=True, res_mod=(7 if M > 7 else None))
            _gemm_case(F32, M, N, K, bias=2, act=1)
            _gemm_case(F32, M, N, K, resid=True)
    for (bias, act) in ((0, 0), (0, 1), (2, 1)):       # the row kernel's remaining epilogue instantiations
        _gemm_case(F16, 12000, 1280, 1280, bias=bias, act=act)
    _gemm_case(F16, 1500, 1280, 1280, bias=1, batch=3, lda=1288, ldc=1288)
    _gemm_case(F16, 200, 1536, 384, bias=1, act=1, batch=4, lda=392, ldc=1544)
    _gemm_case(F32, 200, 512, 384, bias=1, batch=2, lda=416, ldc=520, resid=True)
    sweep = torch.linspace(-12.0, 12.0, 4096)
    for M in (1500, 3000):                    # GELU pre-activations over [-12, 12]: the row kernel (gelu_erf_f16out) and tiles
        _gemm_case(F16, M, 4096, 1280, bias=1, act=1, bias_vals=sweep, w_scale=1e-3)
        _gemm_case(F16, M, 4096, 1280, bias=1, act=1, bias_vals=sweep, w_scale=1e-3, out_f32=True)


# -------------------------------------------------------------------------------------------------------- flash
@pytest.mark.parametrize("prescaled", [0, 1])
def test_attn_flash(gpu_device, prescaled):
    dev = _dev()
    for (B, H, T, Tq) in ((1, 6, 1, 1), (1, 6, 2, 2), (2, 6, 63, 63), (1, 6, 64, 64), (1, 20, 65, 65), (1, 6, 127, 127),
                          (1, 6, 128, 128), (2, 6, 129, 129), (2, 20, 1500, 1500), (2, 6, 1500, 17), (1, 6, 129, 3)):
        g = torch.Generator().manual_seed(B * 1000 + H * 100 + T + Tq)
        D = H * 64
        ld = D + 64
        q = torch.randn(B, Tq, D, generator=g).half()
        k = torch.randn(B, T, D, generator=g).half()
        v = torch.randn(B, T, D, generator=g).half()
        if prescaled:
            f = math.sqrt(0.125 * math.log2(math.e))
            q, k = (q.float() * f).half(), (k.float() * f).half()
        vt_ld = (T + 63) // 64 * 64 + 8
        qb, kb = Buf(B * Tq * ld, torch.float16), Buf(B * T * ld, torch.float16)
        qb.t.view(B, Tq, ld)[:, :, :D] = q.to(dev)
        kb.t.view(B, T, ld)[:, :, :D] = k.to(dev)
        vtt = torch.full((B, D, vt_ld), 60000.0).half()           # pad columns: finite
        vtt[:, :, :T] = v.transpose(1, 2)
        vb = Buf(B * D * vt_ld, torch.float16)
        vb.t.copy_(vtt.reshape(-1).to(dev))
        out = Buf(B * Tq * ld, torch.float16)
        out.snapshot()
        e = lib().wht_attn_flash_f16(qb.ptr(), ld, Tq * ld, kb.ptr(), ld, T * ld, vb.ptr(), vt_ld, D * vt_ld, out.ptr(), ld,
                                     Tq * ld, B, H, T, prescaled, Tq, _stream())
        assert e == hipSuccess
        torch.cuda.synchronize()
        assert not out.changed().view(B, Tq, ld)[:, :, D:].any(), "row gap written"
        got = out.t.view(B, Tq, ld)[:, :, :D].double()
        qd, kd, vd = q.double().to(dev), k.double().to(dev), v.double().to(dev)
        ref = torch.empty(B, Tq, D, dtype=torch.float64, device=dev)
        pv = torch.empty_like(ref)
        pert = torch.empty_like(ref)
        for h in range(H):
            sl = slice(h * 64, h * 64 + 64)
            s = qd[:, :, sl] @ kd[:, :, sl].transpose(1, 2)
            s = s * math.log(2.0) if prescaled else s * 0.125
            p = torch.softmax(s, -1)
            ref[:, :, sl] = p @ vd[:, :, sl]
            pv[:, :, sl] = p @ vd[:, :, sl].abs()
            if T >= 2:
                pert[:, :, sl] = torch.softmax(s[:, :, :T - 1], -1) @ vd[:, :T - 1, sl]
        bound = _ulp(ref, F16) + C_ATT_MFMA * pv
        _check(f"flash/prescaled{prescaled}", got, ref, bound, f"B={B} H={H} T={T} Tq={Tq}")
        if T >= 2:
            _sensitive(ref, pert, bound, "the last key dropped")


# ---------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dtype", [F16, F32])
def test_layernorm(gpu_device, dtype):
    dev, tdt = _dev(), _tdt(dtype)
    for D in (256, 260, 384, 1280, 2048):
        for rows in (1, 3, 5, 1501):
            for (mean, std) in ((0.0, 1.0), (50.0, 0.05)):
                g = torch.Generator().manual_seed(D + rows + int(mean))
                ldx, ldo = D + 12, D + 8
                x = (torch.randn(rows, D, generator=g, dtype=torch.float64) * std + mean).float()
                w = (1 + 0.2 * torch.randn(D, generator=g)).float().to(dev)
                b = (0.1 * torch.randn(D, generator=g)).float().to(dev)
                xb = Buf(rows * ldx, torch.float32)
                xb.t.view(rows, ldx)[:, :D] = x.to(dev)
                out = Buf(rows * ldo, tdt)
                out.snapshot()
                e = lib().wht_layernorm(xb.ptr(), ldx, w.data_ptr(), b.data_ptr(), out.ptr(), ldo, rows, D, dtype, _stream())
                assert e == hipSuccess
                torch.cuda.synchronize()
                assert not out.changed().view(rows, ldo)[:, D:].any(), "row gap written"
                xd = x.double().to(dev)
                mu = xd.mean(1, keepdim=True)
                var = ((xd - mu) ** 2).mean(1, keepdim=True)
                ref = (xd - mu) / torch.sqrt(var + 1e-5) * w.double() + b.double()
                delta = 2.0 ** -19 * (mu.abs() / torch.sqrt(var + 1e-5) + 1.0) * (ref.abs() + b.double().abs() + 1.0)
                bound = _ulp(ref, dtype) + delta
                _check(f"layernorm<{'half' if dtype == F16 else 'float'}>", out.t.view(rows, ldo)[:, :D], ref, bound,
                       f"D={D} rows={rows} mean={mean}")
                if rows >= 2:
                    _sensitive(ref, ref[[1, 0] + list(range(2, rows))], bound, "two rows swapped")


# ------------------------------------------------------------------------------------------------- copy kernels
def test_copy_kernels_exact(gpu_device):
    """scatter_kv, gather_cache, permute_groups (identity, swaps, 3-cycles, G = 1 / 5 / 8, copy_from) and replicate_row
    (source inside the destination range): bit-exact, nothing outside the destination rows written"""
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    # scatter_kv: qkv [R*T0][3D] -> caches [R][n_ctx][D] at positions *d_offset + t
    for dtype in (F16, F32):
        tdt = _tdt(dtype)
        R, T0, D, n_ctx, off = 3, 5, 384, 16, 7
        qkv = torch.randn(R * T0, 3 * D, generator=g).to(tdt).to(dev)
        kc, vc = Buf(R * n_ctx * D, tdt), Buf(R * n_ctx * D, tdt)
        kc.snapshot(); vc.snapshot()
        d_off = torch.tensor([off], dtype=torch.int32, device=dev)
        assert lib().wht_scatter_kv(qkv.data_ptr(), R, T0, D, d_off.data_ptr(), n_ctx, kc.ptr(), vc.ptr(), dtype,
                                    _stream()) == hipSuccess
        torch.cuda.synchronize()
        for cb, c0 in ((kc, D), (vc, 2 * D)):
            c = cb.t.view(R, n_ctx, D)
            w = cb.changed().view(R, n_ctx, D)
            assert w[:, off:off + T0].all() and not w[:, :off].any() and not w[:, off + T0:].any()
            assert torch.equal(c[:, off:off + T0].reshape(R * T0, D).view(torch.uint8),
                               qkv[:, c0:c0 + D].contiguous().view(torch.uint8))
    FORMS.add("scatter_kv")
    # gather_cache: dst row i <- first used_bytes of src row src_idx[i]
    R, row_bytes, used = 6, 4096, 2048 + 512
    src = torch.randint(0, 256, (R * row_bytes,), generator=g, dtype=torch.uint8).to(dev)
    dst = Buf(R * row_bytes, torch.uint8); dst.snapshot()
    idx = torch.tensor([5, 0, 0, 3, 2, 5], dtype=torch.int32, device=dev)
    assert lib().wht_gather_cache(src.data_ptr(), dst.ptr(), idx.data_ptr(), R, row_bytes, used, _stream()) == hipSuccess
    torch.cuda.synchronize()
    d = dst.t.view(R, row_bytes)
    assert torch.equal(d[:, :used], src.view(R, row_bytes)[idx.long(), :used])
    assert not dst.changed().view(R, row_bytes)[:, used:].any()
    FORMS.add("gather_cache")
    # permute_groups: in place, K and V caches of n_layers layers, groups of G rows
    for (G, perm_of) in ((1, lambda a: [0]), (5, lambda a: [0, 1, 2, 3, 4] if a == 0 else [1, 0, 3, 4, 2]),
                         (8, lambda a: [7, 7, 2, 0, 1, 5, 6, 3] if a == 0 else [2, 0, 1, 3, 4, 5, 6, 7])):
        for use_copy_from in (False, True):
            n_layers, n_audio, row_bytes, pos_bytes = 2, 2, 2048, 64
            used = 1536
            layer_bytes = n_audio * G * row_bytes + 256
            kb = torch.randint(0, 256, (n_layers * layer_bytes,), generator=g, dtype=torch.uint8).to(dev)
            vb = torch.randint(0, 256, (n_layers * layer_bytes,), generator=g, dtype=torch.uint8).to(dev)
            src_idx = [a * G + j for a in range(n_audio) for j in perm_of(a)]
            cf = [int(torch.randint(0, used // pos_bytes + 1, (1,), generator=g)) for _ in src_idx] if use_copy_from else None
            want = []
            for base in (kb, vb):
                wv = base.clone()
                for L in range(n_layers):
                    for a in range(n_audio):
                        for j in range(G):
                            i = a * G + j
                            s0 = L * layer_bytes + src_idx[i] * row_bytes
                            d0 = L * layer_bytes + i * row_bytes
                            lo = cf[i] * pos_bytes if cf else 0
                            wv[d0 + lo:d0 + used] = base[s0 + lo:s0 + used]
                want.append(wv)
            si = torch.tensor(src_idx, dtype=torch.int32, device=dev)
            cft = torch.tensor(cf, dtype=torch.int32, device=dev) if cf else None
            assert lib().wht_permute_groups(kb.data_ptr(), vb.data_ptr(), n_layers, layer_bytes, n_audio, G, row_bytes, used,
                                            si.data_ptr(), cft.data_ptr() if cft is not None else None, pos_bytes,
                                            _stream()) == hipSuccess
            torch.cuda.synchronize()
            assert torch.equal(kb, want[0]) and torch.equal(vb, want[1]), (G, use_copy_from)
    FORMS.add("permute_groups")
    # replicate_row: rows [dst_row0, dst_row0 + G) <- row src_row, the source inside the destination range
    for (src_row, dst0, G) in ((2, 0, 5), (0, 0, 4), (4, 1, 3)):
        n_layers, row_bytes, used = 3, 1024, 772
        layer_bytes = 6 * row_bytes
        base = torch.randint(0, 256, (n_layers * layer_bytes,), generator=g, dtype=torch.uint8).to(dev)
        want = base.clone().view(n_layers, 6, row_bytes)
        for L in range(n_layers):
            for j in range(G):
                want[L, dst0 + j, :used] = want[L, src_row, :used].clone()
        assert lib().wht_replicate_row(base.data_ptr(), layer_bytes, n_layers, row_bytes, src_row, dst0, G, used,
                                       _stream()) == hipSuccess
        torch.cuda.synchronize()
        assert torch.equal(base.view(n_layers, 6, row_bytes), want), (src_row, dst0, G)
    FORMS.add("replicate_row")


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals(gpu_device):
    """every request kernels.h says a launcher refuses is refused on the host with hipErrorInvalidValue (nothing runs)"""
    dev = _dev()
    L = lib()
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=dev)
    fbuf = torch.zeros(1 << 18, dtype=torch.float32, device=dev)
    cnt = torch.zeros(64, dtype=torch.int32, device=dev)
    p, pf, s = buf.data_ptr(), fbuf.data_ptr(), _stream()
    # x_frag / y_frag where gemv8 does not run: 30 rows; fp32; K = 5184 beyond its cover
    assert not L.wht_gemv8_will_run(30, 384, 384, PLAIN)
    for (dt, R, N, K, xf, yf) in ((F16, 30, 384, 384, 1, 0), (F16, 30, 384, 384, 0, 1), (F32, 4, 384, 384, 1, 0),
                                  (F16, 4, 384, 5184, 1, 0)):
        e = L.wht_gemv(dt, PLAIN, p, K, None, 0, None, None, 0, None, None, 1, 0, p, None, N, K, R, xf, yf, STORE, p, N,
                       None, 0, None, None, 0, None, 0, None, None, 0, None, s)
        assert e == hipErrorInvalidValue, (dt, R, N, K, xf, yf, e)

    def attn(dtype, R, Tk, S, G=1, merge=True):
        return L.wht_attn_decode(dtype, p, 384, p, 384, 384 * 600, p, 384, 384 * 600, 0, 6, R, G, Tk, None, 0, None, S, p,
                                 384, 0, p, pf, cnt.data_ptr() if merge else None, None, 0, 0, s)
    assert attn(F16, 2, 1500, 5) == hipErrorInvalidValue                   # in-launch merge: splits 5
    assert attn(F16, 2, 1500, 1) == hipErrorInvalidValue                   # ... splits 1
    assert attn(F32, 2, 200, 2) == hipErrorInvalidValue                    # ... fp32
    assert attn(F16, 4, 200, 2, G=2) == hipErrorInvalidValue               # ... kv_group > 1
    assert attn(F16, 2, 600, 1, merge=False) == hipErrorInvalidValue       # 19 rounds of 32 keys > 16
    assert attn(F16, 2, 1500, 17, merge=False) == hipErrorInvalidValue     # splits > DEC_ATTN_MAX_SPLITS
    assert L.wht_merge_partials(p, pf, 17, 2, 6, p, 384, F16, 0, s) == hipErrorInvalidValue
    for D in (2052, 258):
        assert L.wht_layernorm(pf, D, pf, pf, p, D, 2, D, F16, s) == hipErrorInvalidValue
    assert L.wht_permute_groups(p, p, 1, 1 << 16, 1, 9, 1024, 512, cnt.data_ptr(), None, 0, s) == hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (buf == 0).all() and (fbuf == 0).all() and (cnt == 0).all()


# ----------------------------------------------------------------------------------------------------- coverage
# Every terminal branch of the four dispatchers (whk::g_form) plus the other launchers under test.  Not reachable, and so
# not listed: attn/group_mfma<1> / <2> (the beam-group matrix-core kernels of round 5) — with vt the diagonal kernel takes
# every request whose vt_ld >= 64, and vt_ld >= splits x 128 is required first; only the developer switch
# WH_GROUP_ATTN_HALF_LINES of the -DWH_DEV build selects them.
EXPECTED_FORMS = [
    "attn/group<float>", "attn/group<half>", "attn/group_diag", "attn/rounds<float,12>", "attn/rounds<float,16>",
    "attn/rounds<float,8>", "attn/rounds<half,12>", "attn/rounds<half,12>/merge", "attn/rounds<half,16>",
    "attn/rounds<half,16>/merge", "attn/rounds<half,8>", "attn/self<float>", "attn/self<half>",
    "attn/self<half>/merge", "flash/prescaled0", "flash/prescaled1", "gather_cache", "gemm/rows<0,0>", "gemm/rows<0,1>",
    "gemm/rows<0,2>", "gemm/rows<1,0>", "gemm/rows<1,1>", "gemm/rows<1,2>", "gemm/tile<float,float,1,1>",
    "gemm/tile<float,float,1,2>",
    "gemm/tile<float,float,2,2>", "gemm/tile<half,float,1,1>", "gemm/tile<half,float,1,2>",
    "gemm/tile<half,float,2,2>", "gemm/tile<half,float,4,4>", "gemm/tile<half,half,1,1>", "gemm/tile<half,half,1,2>",
    "gemm/tile<half,half,2,2>", "gemm/tile<half,half,4,4>", "gemv8/LN/gs1/ks4/xw8/rt1", "gemv8/LN/gs1/ks4/xw8/rt2",
    "gemv8/LN/gs1/ks4/xw8/rt3", "gemv8/LN/gs2/ks4/xw8/rt1", "gemv8/LN/gs2/ks4/xw8/rt2", "gemv8/LN/gs2/ks4/xw8/rt3",
    "gemv8/LN/gs3/ks2/xw8/rt2", "gemv8/LN/gs3/ks2/xw8/rt3", "gemv8/LN/gs3/ks4/xw4/rt1",
    "gemv8/combine2/gs1/ks4/xw8/rt1", "gemv8/combine2/gs1/ks4/xw8/rt2", "gemv8/combine2/gs1/ks4/xw8/rt3",
    "gemv8/combine3/gs1/ks4/xw8/rt1", "gemv8/combine3/gs1/ks4/xw8/rt2", "gemv8/combine3/gs1/ks4/xw8/rt3",
    "gemv8/combine4/gs1/ks4/xw8/rt1", "gemv8/combine4/gs1/ks4/xw8/rt2", "gemv8/combine4/gs1/ks4/xw8/rt3",
    "gemv8/plain/gs1/ks16/xw0/rt1", "gemv8/plain/gs1/ks16/xw0/rt2", "gemv8/plain/gs1/ks16/xw0/rt3",
    "gemv8/plain/gs1/ks4/xw0/rt1", "gemv8/plain/gs1/ks4/xw0/rt2", "gemv8/plain/gs1/ks4/xw0/rt3",
    "gemv8/plain/gs1/ks4/xw0/rt6", "layernorm<float>", "layernorm<half>", "merge<float,16>", "merge<float,4>",
    "merge<half,16>", "merge<half,4>", "permute_groups", "replicate_row", "rows16_mf<half,16>/pro<4,0,16,1>",
    "rows16_mf<half,16>/pro<4,0,16,4>", "rows16_mf<half,16>/pro<4,0,4,1>", "rows16_mf<half,16>/pro<4,0,8,1>",
    "rows16_mf<half,16>/pro<4,0,8,2>", "rows16_mf<half,16>/pro<4,1,4,1>", "rows48", "rows48_stream",
    "rt<float,4>/pro<8,0,16,1>", "rt<float,4>/pro<8,0,4,1>", "rt<float,4>/pro<8,0,8,1>", "rt<float,4>/pro<8,1,4,1>",
    "rt<float,8>/pro<8,0,16,1>", "rt<float,8>/pro<8,0,4,1>", "rt<float,8>/pro<8,0,8,1>", "rt<float,8>/pro<8,1,4,1>",
    "rt<half,4>/pro<8,0,8,1>", "rt<half,8>/pro<8,0,8,1>", "scatter_kv", "stream<float,4>", "stream<float,8>",
    "stream<half,4>", "stream<half,8>",
]


def test_coverage_and_report(gpu_device):
    """runs last: the forms the cases above reached equal EXPECTED_FORMS, and the largest error / bound ratio per form is
    written to kernel_parity.json.  A form no case reaches fails, and so does a form missing from the list."""
    from conftest import write_report
    write_report("kernel_parity.json", {"bounds": {"C_DOT": C_DOT, "C_ATT_VALU": C_ATT_VALU, "C_ATT_MFMA": C_ATT_MFMA},
                                        "max_ratio": dict(sorted(REPORT.items())), "forms": sorted(FORMS)})
    unexpected, unreached = sorted(FORMS - set(EXPECTED_FORMS)), sorted(set(EXPECTED_FORMS) - FORMS)
    assert not unexpected and not unreached, f"forms not in EXPECTED_FORMS: {unexpected}; forms no case reached: {unreached}"
