"""Per-element parity of the prefill, word-timestamp, alignment, encoder-stem and small kernels against float64, through
libwhisper_hip_ktest.so — the kernels that tests/test_kernel_parity_gpu.py and its siblings leave to the whole-model tests.
The references, bounds and perturbations live in tests/prefill_align_ref.py (checked on the CPU by
tests/test_prefill_align_ref_cpu.py); the pattern is that of test_kernel_parity_gpu.py: every case goes through _check,
guard bytes and everything a launch must not write hold 0xFF and must come back unchanged, declared don't-care inputs hold
NaN, and _sensitive shows that the bound sees the named perturbations.

  attn_generic_kernel ...... ulp_out + C_ATT_VALU sum p |v| / sum p + 2^-21 sum p (1 + |s - m|) |v| / sum p: parity_ref.attn_bound
                             with one split.  The last term is the __expf argument error (exp2 of a rounded product), which
                             grows with |s - m|; the constant is not widened.
  cross_qk* ................ ulp_f32 + C_DOT * 0.125 * sum |q_d k_d|.  fp32 runs cross_qk_batch_kernel<float>, fp16 the MFMA
                             kernel; cross_qk_batch_kernel<half> is unreachable in the shipped library (the MFMA form takes
                             every fp16 request whose D is a multiple of 8, and D is a multiple of 64; the switch back is
                             read by the developer build only), so it is not tested.
  launch_align_batch ....... staged: (a) w0 against float64 softmax + z-norm with prefill_align_ref.align_stage_a's bound,
                             (b) w1 bit-equal to oracle.timing.median_filter of the GPU's own w0, (c) cost against the float64
                             head mean of the GPU's own w1 (ulp + H 2^-24 sum_h |w1|), and end to end with the stage-(a)
                             bound carried through the median window and the mean.  A clip of one frame has a softmax of
                             exactly 1 and a std of 0 over its tokens: 0 / 0 = NaN in the reference, the oracle and the
                             kernel alike; there the check is "NaN where the reference is NaN".
  encoder stem ............. mel_transpose bit-equal; conv1 and conv2 launched as api.cpp does, each against float64 conv1d +
                             exact GELU (+ pos) of the GPU's own input with test_kernel_parity_gpu._gemm_case's bound including
                             its GELU term.  conv1 of 80 mels reads K = 256 > 240 elements per row: the 256-element slack
                             behind the last row holds large finite values — the contract is "finite" (the weight columns
                             there are zero), as for the V^T pad columns.
  embed, gathers ........... bit-equal.   no_speech: prefill_align_ref.no_speech_ref's relative bound.
"""
import math

import numpy as np
import pytest
import torch

import prefill_align_ref as pr
from kernel_lib import hipErrorInvalidValue, hipSuccess, lib
from parity_ref import C_ATT_VALU, C_DOT, F16, F32, Buf, _dev, _stream, _tdt, _ulp

pytestmark = pytest.mark.gpu

REPORT = {}                  # form -> largest error / bound ratio
H2, D = 2, 128


def _record(form, ratio):
    REPORT[form] = max(REPORT.get(form, 0.0), float(ratio))


def _check(form, got, ref, bound, what=""):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{form} {what}: non-finite output"
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"{form} {what}: error / bound = {ratio:.3f}")
    _record(form, ratio)
    assert ratio <= 1.0, f"{form} {what}: error / bound = {ratio:.3f}"
    return ratio


def _sensitive(ref, pert, bound, what):
    """the bound must not be vacuous: the perturbed reference fails it somewhere."""
    r = ((pert - ref).abs() / bound).max().item()
    assert r > 1.0, f"bound too loose to see {what} (ratio {r:.3f})"


def _exact(form, got, want, what=""):
    assert torch.equal(got.cpu().contiguous().view(torch.uint8), want.cpu().contiguous().view(torch.uint8)), f"{form} {what}: not bit-equal"
    _record(form, 0.0)


def _nm(dtype):
    return "half" if dtype == F16 else "float"


def _buf_from(t, tdt=None):
    """a guarded device buffer holding the CPU tensor t"""
    b = Buf(t.numel(), tdt or t.dtype)
    b.t.copy_(t.reshape(-1).to(_dev()))
    return b


def _ints(v):
    return torch.tensor(v, dtype=torch.int32, device=_dev())


# ------------------------------------------------------------------------------------------- generic attention
@pytest.mark.parametrize("dtype", [F16, F32])
def test_attn_generic_self(gpu_device, dtype):
    """causal prefill self-attention: Tk = *d_len + Tq read on the device, q inside [R][Tq][3D] rows, K / V caches
    [R][96][D] with NaN at and beyond d_len + Tq.  (60, 17) crosses the 64-key tile inside one query block; (10, 70) has a
    block whose first queries see nothing of its last tile."""
    R, C, tdt, dev = 3, 96, _tdt(dtype), _dev()
    o_ld = D + 32
    for (d_len, Tq) in ((0, 1), (0, 16), (0, 17), (3, 5), (60, 17), (10, 70), (0, 64), (1, 64)):
        q, k, v = pr.attn_inputs(dtype, R, R, Tq, C, H2, seed=1000 + d_len * 100 + Tq)
        qkv = torch.full((R, Tq, 3 * D), float("nan")).to(tdt)
        qkv[:, :, :D] = q
        kp, vp = k.clone(), v.clone()
        kp[:, d_len + Tq:] = float("nan"); vp[:, d_len + Tq:] = float("nan")
        qb, kb, vb = _buf_from(qkv), _buf_from(kp), _buf_from(vp)
        out = Buf(R * Tq * o_ld, tdt)
        dl = _ints([d_len])
        for b in (qb, kb, vb, out):
            b.snapshot()
        e = lib().wht_attn_generic(dtype, R, qb.ptr(), 3 * D, Tq * 3 * D, kb.ptr(), D, C * D, vb.ptr(), D, C * D, out.ptr(), o_ld,
                                   Tq * o_ld, H2, Tq, 0, dl.data_ptr(), 1, 1, _stream())
        assert e == hipSuccess
        torch.cuda.synchronize()
        for b in (qb, kb, vb):
            assert not b.changed().any(), "an input was written"
        assert not out.changed().view(R, Tq, o_ld)[:, :, D:].any(), "row gap written"
        got = out.t.view(R, Tq, o_ld)[:, :, :D].cpu()
        lim = d_len + 1 + torch.arange(Tq)
        refs = [pr.generic_attn_ref(q[b].double(), k[b].double(), v[b].double(), H2, lim) for b in range(R)]
        ref = torch.stack([a["ref"] for a in refs])
        bound = torch.stack([pr.generic_attn_bound(a, dtype) for a in refs])
        _check(f"attn_generic<{_nm(dtype)}>/self", got, ref, bound, f"d_len={d_len} Tq={Tq}")
        if d_len + Tq >= 2:
            pert = torch.stack([pr.generic_attn_ref(q[b].double(), k[b].double(), v[b].double(), H2, lim, drop_last=True)["ref"]
                                for b in range(R)])
            _sensitive(ref, pert, bound, "the last key dropped")
        pert = torch.stack([pr.generic_attn_ref(q[b].double(), k[b].double(), v[b].double(), H2, lim + 1)["ref"] for b in range(R)])
        _sensitive(ref, pert, bound, "the mask shifted by one")


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("G", [1, 3])
def test_attn_generic_cross(gpu_device, dtype, G):
    """non-causal prefill cross attention over interleaved K / V rows (k_ld = v_ld = 2D), rows b of audio b / kv_group"""
    R, tdt = 6, _tdt(dtype)
    A = R // G
    o_ld = D + 32
    es = torch.empty((), dtype=tdt).element_size()
    for Tk in (1, 63, 64, 65, 1500):
        for Tq in (1, 15, 16, 33):
            q, k, v = pr.attn_inputs(dtype, R, A, Tq, Tk, H2, seed=Tk * 7 + Tq + G)
            qb, kvb = _buf_from(q), _buf_from(torch.cat([k, v], 2))
            out = Buf(R * Tq * o_ld, tdt)
            for b in (qb, kvb, out):
                b.snapshot()
            e = lib().wht_attn_generic(dtype, R, qb.ptr(), D, Tq * D, kvb.ptr(), 2 * D, Tk * 2 * D, kvb.ptr() + D * es, 2 * D,
                                       Tk * 2 * D, out.ptr(), o_ld, Tq * o_ld, H2, Tq, Tk, None, 0, G, _stream())
            assert e == hipSuccess
            torch.cuda.synchronize()
            assert not qb.changed().any() and not kvb.changed().any(), "an input was written"
            assert not out.changed().view(R, Tq, o_ld)[:, :, D:].any(), "row gap written"
            got = out.t.view(R, Tq, o_ld)[:, :, :D].cpu()
            lim = torch.full((Tq,), Tk)
            refs = [pr.generic_attn_ref(q[b].double(), k[b // G].double(), v[b // G].double(), H2, lim) for b in range(R)]
            ref = torch.stack([a["ref"] for a in refs])
            bound = torch.stack([pr.generic_attn_bound(a, dtype) for a in refs])
            _check(f"attn_generic<{_nm(dtype)}>/cross", got, ref, bound, f"Tk={Tk} Tq={Tq} G={G}")
            if Tk >= 2:
                pert = torch.stack([pr.generic_attn_ref(q[b].double(), k[b // G].double(), v[b // G].double(), H2, lim,
                                                        drop_last=True)["ref"] for b in range(R)])
                _sensitive(ref, pert, bound, "the last key dropped")
            if G == 3:
                pert = torch.stack([pr.generic_attn_ref(q[b].double(), k[b % 2].double(), v[b % 2].double(), H2, lim)["ref"]
                                    for b in range(R)])
                _sensitive(ref, pert, bound, "audio b % 2 instead of b / 3")


# ---------------------------------------------------------------------------------------------------- cross QK
@pytest.mark.parametrize("dtype", [F16, F32])
def test_cross_qk_single(gpu_device, dtype):
    """cross_qk_kernel: head 1 of 2, q rows inside a [n_tok][3D] buffer, keys in interleaved K / V rows"""
    tdt, head = _tdt(dtype), 1
    for n_tok in (1, 5):
        for Tk in (1, 255, 256, 257, 1500):
            g = torch.Generator().manual_seed(n_tok * 10000 + Tk)
            q = torch.randn(n_tok, D, generator=g).to(tdt)
            k = torch.randn(Tk, D, generator=g).to(tdt)
            qkv = torch.full((n_tok, 3 * D), float("nan")).to(tdt); qkv[:, :D] = q
            kv = torch.full((Tk, 2 * D), float("nan")).to(tdt); kv[:, :D] = k
            qb, kb = _buf_from(qkv), _buf_from(kv)
            out = Buf(n_tok * Tk, torch.float32)
            for b in (qb, kb, out):
                b.snapshot()
            assert lib().wht_cross_qk(qb.ptr(), 3 * D, kb.ptr(), 2 * D, head, n_tok, Tk, out.ptr(), dtype, _stream()) == hipSuccess
            torch.cuda.synchronize()
            assert not qb.changed().any() and not kb.changed().any(), "an input was written"
            out.changed()                                          # the guards
            sl, other = slice(64, 128), slice(0, 64)
            ref, bound = pr.cross_qk_ref(q[:, sl].double(), k[:, sl].double())
            _check(f"cross_qk<{_nm(dtype)}>", out.t.view(n_tok, Tk), ref, bound, f"n_tok={n_tok} Tk={Tk}")
            _sensitive(ref, pr.cross_qk_ref(q[:, other].double(), k[:, other].double())[0], bound, "the head swapped")
            _sensitive(ref, pr.cross_qk_ref(q[:, sl].double(), k[:, sl].double(), drop_last_d=True)[0], bound, "the last d term dropped")


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("G", [1, 3])
def test_cross_qk_batch(gpu_device, dtype, G):
    """every (row, pair) plane of a batch: fp32 on the vector ALU, fp16 on the matrix cores (token rows clamped to
    ntok - 1, frames to Tk - 1, 16-frame sub-tiles, token tiles skipped per clip).  qcap rows at and beyond ntok[r] hold NaN,
    the V halves of the key rows too; output rows t >= ntok[r] are left alone."""
    tdt = _tdt(dtype)
    R, L, C, Tmax = 3, 2, 72, 70
    layers, heads, ntok = [0, 1, 1], [1, 0, 1], [1, 17, 70]
    A = R // G
    form = "cross_qk_batch/mfma" if dtype == F16 else "cross_qk_batch<float>"
    for Tk in (1, 15, 16, 17, 127, 128, 129, 1500):
        g = torch.Generator().manual_seed(Tk * 3 + G)
        q = torch.randn(L, R, C, D, generator=g).to(tdt)
        k = torch.randn(L, A, Tk, D, generator=g).to(tdt)
        qp = q.clone()
        for r in range(R):
            qp[:, r, ntok[r]:] = float("nan")
        kv = torch.full((L, A, Tk, 2 * D), float("nan")).to(tdt); kv[..., :D] = k
        qb, kb = _buf_from(qp), _buf_from(kv)
        out = Buf(R * 3 * Tmax * Tk, torch.float32)
        for b in (qb, kb, out):
            b.snapshot()
        dl, dh, dn = _ints(layers), _ints(heads), _ints(ntok)
        e = lib().wht_cross_qk_batch(qb.ptr(), R * C * D, C * D, D, kb.ptr(), A * Tk * 2 * D, Tk * 2 * D, G, dl.data_ptr(),
                                     dh.data_ptr(), 3, dn.data_ptr(), R, Tmax, Tk, out.ptr(), dtype, _stream())
        assert e == hipSuccess
        torch.cuda.synchronize()
        assert not qb.changed().any() and not kb.changed().any(), "an input was written"
        written = out.changed().view(R, 3, Tmax, Tk).cpu()
        got = out.t.view(R, 3, Tmax, Tk).cpu()
        for r in range(R):
            assert not written[r, :, ntok[r]:].any(), f"{form}: rows t >= ntok[{r}] written"
            assert written[r, :, :ntok[r]].all(), f"{form}: a score of row {r} not written"
            for p in range(3):
                sl, other = slice(heads[p] * 64, heads[p] * 64 + 64), slice((1 - heads[p]) * 64, (1 - heads[p]) * 64 + 64)
                qq, kk = q[layers[p], r, :ntok[r]].double(), k[layers[p], r // G].double()
                ref, bound = pr.cross_qk_ref(qq[:, sl], kk[:, sl])
                _check(form, got[r, p, :ntok[r]], ref, bound, f"Tk={Tk} G={G} r={r} pair={p}")
                _sensitive(ref, pr.cross_qk_ref(qq[:, other], kk[:, other])[0], bound, "the head swapped")
                _sensitive(ref, pr.cross_qk_ref(qq[:, sl], kk[:, sl], drop_last_d=True)[0], bound, "the last d term dropped")


# --------------------------------------------------------------------------------------------------- alignment
def _align_case(width, scale, nfr):
    dev = _dev()
    clips, H, Tmax, Fmax, Tk, rb, rt = 3, 3, 40, 300, 320, 1, 1
    ntok, Nmax = [2, 9, 40], 38
    qk = pr.align_inputs(clips, H, Tmax, Tk, seed=width * 10 + int(scale * 2) + nfr[0])
    qp = qk.clone()
    for b in range(clips):
        qp[b, :, :, nfr[b]:] = float("nan")
        qp[b, :, ntok[b]:] = float("nan")
    qb = _buf_from(qp)
    per = H * Tmax * Fmax
    scratch, cost = Buf(2 * clips * per, torch.float32), Buf(clips * Nmax * Fmax, torch.float32)
    for b in (qb, scratch, cost):
        b.snapshot()
    dn, df = _ints(ntok), _ints(nfr)
    e = lib().wht_align_batch(qb.ptr(), dn.data_ptr(), df.data_ptr(), clips, H, Tmax, Tk, Fmax, width, rb, rt, scale, cost.ptr(),
                              Nmax, scratch.ptr(), _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not qb.changed().any(), "qk was written"
    wr = scratch.changed().view(2, clips, H, Tmax, Fmax).cpu()
    w = scratch.t.view(2, clips, H, Tmax, Fmax).cpu()
    cw, cg = cost.changed().view(clips, Nmax, Fmax).cpu(), cost.t.view(clips, Nmax, Fmax).cpu()
    from oracle.timing import median_filter
    what = f"width={width} scale={scale}"
    for b in range(clips):
        T, F = ntok[b], nfr[b]
        rows = T - rb - rt
        inside = torch.zeros(H, Tmax, Fmax, dtype=torch.bool); inside[:, :T, :F] = True
        for half in (0, 1):
            assert torch.equal(wr[half, b], inside), f"align {what}: w{half} of clip {b} written outside [T][F] or not all of it"
        cin = torch.zeros(Nmax, Fmax, dtype=torch.bool); cin[:rows, :F] = True
        assert torch.equal(cw[b], cin), f"align {what}: cost slab of clip {b} written outside its rows x frames"
        w0, w1 = w[0, b, :, :T, :F], w[1, b, :, :T, :F]
        w0r, b0, w1r, b1, costr, bc = pr.align_chain_ref(qk[b].double(), T, F, scale, width, rb, rt)
        # (a) softmax + z-norm
        if F == 1:                                                 # 0 / 0 over identical softmax values: NaN on both sides
            assert torch.isnan(w0r).all() and torch.isnan(w0).all() and torch.isnan(w1).all()
        else:
            _check("align/softmax_znorm", w0, w0r, b0, f"{what} clip {b}")
        # (b) the median is an order statistic: bit-equal to the oracle's on the GPU's own w0
        med = torch.from_numpy(np.ascontiguousarray(median_filter(w0.contiguous().numpy(), width)))
        nan = torch.isnan(med)
        assert torch.equal(nan, torch.isnan(w1))
        form_b = f"align/median<{width}>" if width <= 13 else "align/median_generic"
        _exact(form_b + ("/passthrough" if F <= width // 2 else ""), torch.where(nan, torch.zeros_like(w1), w1),
               torch.where(nan, torch.zeros_like(med), med), f"{what} clip {b}")
        if rows <= 0:
            continue
        # (c) the head mean of the GPU's own w1, and the whole chain with the propagated bound
        c2, bc2 = pr.head_mean_ref(w1, T, rb, rt)
        _check("align/head_mean", cg[b, :rows, :F], c2, bc2, f"{what} clip {b}")
        _check("align/end_to_end", cg[b, :rows, :F], costr, bc, f"{what} clip {b}")
        if b == 2:
            q2 = qk[b].double()
            _sensitive(w0r, pr.align_stage_a(q2, T, F, scale, soft_frames=F + 1)[0], b0, "softmax over F + 1 frames")
            _sensitive(w0r, pr.align_stage_a(q2, T, F, scale, unbiased=True)[0], b0, "the unbiased std")
            _sensitive(costr, pr.align_chain_ref(q2, T, F, scale, width, rb, rt, shift=1)[4], bc, "the window shifted by one")
            _sensitive(costr, pr.align_chain_ref(q2, T, F, scale, width, rb + 1, rt - 1)[4], bc, "row_begin off by one")
            _sensitive(c2, pr.head_mean_ref(w1, T, rb + 1, rt - 1)[0], bc2, "row_begin off by one (head mean)")


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("width", [1, 3, 5, 7, 9, 11, 13, 15])
def test_align_batch(gpu_device, width, scale):
    """three ragged clips (tokens 2 / 9 / 40, frames 1 / 37 / 300) inside (40, 300) slabs of 320-key score rows; with
    row_begin = row_tail = 1 the two-token clip has no cost rows and nothing of its slab is written"""
    _align_case(width, scale, [1, 37, 300])


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_align_batch_passthrough(gpu_device, scale):
    """width 7 over clips of 1 and of 3 frames: F <= W / 2, the row is handed on unchanged"""
    _align_case(7, scale, [3, 37, 300])
    assert "align/median<7>/passthrough" in REPORT


# ------------------------------------------------------------------------------------------------ encoder stem
@pytest.mark.parametrize("mel_f16", [0, 1])
@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("n_mels", [80, 128])
def test_encoder_stem(gpu_device, n_mels, dtype, mel_f16):
    """mel_transpose -> conv1 -> conv2 with the launches of wh_encode: F = 70 frames (a ragged 32-frame transpose block),
    T = 35 (GEMM row tails), B = 2; conv1 with lda = n_mels < K = kc1, conv2 with lda = 2D < K = 3D, the positional
    embedding as a residual shared by the batch (r_bs = 0), fp32 output"""
    from whisper_amd.hip import _conv_as_gemm
    dev, tdt = _dev(), _tdt(dtype)
    F, B = 70, 2
    T, kc1 = F // 2, (3 * n_mels + 63) // 64 * 64
    nm = _nm(dtype)
    mel, w1, b1, w2, b2, pos = pr.stem_inputs(n_mels, D, F, B, dtype, seed=n_mels + dtype)
    mel_in = mel.half() if mel_f16 else mel
    melb = _buf_from(mel_in)
    melT = Buf(B * (F + 2) * n_mels + 256, tdt)
    melb.snapshot(); melT.snapshot()
    assert lib().wht_mel_transpose(melb.ptr(), mel_f16, B, n_mels, F, melT.ptr(), dtype, _stream()) == hipSuccess
    torch.cuda.synchronize()
    assert not melb.changed().any()
    assert not melT.changed()[B * (F + 2) * n_mels:].any(), "mel_transpose wrote behind its last row"
    want = torch.zeros(B, F + 2, n_mels, dtype=tdt)
    want[:, 1:F + 1] = mel_in.to(tdt).transpose(1, 2)
    _exact(f"mel_transpose<{'half' if mel_f16 else 'float'},{nm}>", melT.t[:B * (F + 2) * n_mels].view(B, F + 2, n_mels), want)

    # ---- conv1: M = F rows of K = kc1 elements, lda = n_mels apart; the slack behind the last row: large finite values
    melT.t[B * (F + 2) * n_mels:] = 60000.0 if dtype == F16 else 1e30
    W1 = _conv_as_gemm(w1, kc1).to(dev)
    b1d, b2d, posd = b1.to(dev), b2.to(dev), pos.to(dev)
    c1 = Buf(B * (F + 2) * D, tdt)
    c1v = c1.t.view(B, F + 2, D)
    c1v[:, 0] = 0; c1v[:, F + 1] = 0
    melT.snapshot(); c1.snapshot()
    es = c1.t.element_size()
    e = lib().wht_gemm(dtype, int(dtype != F16), B, melT.ptr(), n_mels, (F + 2) * n_mels, W1.data_ptr(), kc1, 0, c1.ptr() + D * es,
                       D, (F + 2) * D, b1d.data_ptr(), 0, None, 0, 0, 0, 1, F, D, kc1, _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not melT.changed().any()
    wr = c1.changed().view(B, F + 2, D)
    assert not wr[:, 0].any() and not wr[:, F + 1].any(), "conv1 wrote a pad row"
    x = want[:, 1:F + 1]                                           # the GPU's melT, bit-equal to `want`
    ref1, bound1 = pr.conv_gelu_ref(x, w1, b1, 1, dtype)
    _check(f"stem/conv1<{nm}>", c1v[:, 1:F + 1], ref1, bound1, f"n_mels={n_mels}")
    _sensitive(ref1, pr.conv_gelu_ref(x, w1, b1, 1, dtype, flip=True)[0], bound1, "the tap order reversed")

    # ---- conv2: M = T rows of K = 3D elements, lda = 2D apart, + pos, fp32 out
    W2 = _conv_as_gemm(w2, 3 * D).to(dev)
    xo = Buf(B * T * D, torch.float32)
    c1.snapshot(); xo.snapshot()
    e = lib().wht_gemm(dtype, 1, B, c1.ptr(), 2 * D, (F + 2) * D, W2.data_ptr(), 3 * D, 0, xo.ptr(), D, T * D, b2d.data_ptr(), 0,
                       posd.data_ptr(), D, 0, 0, 1, T, D, 3 * D, _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not c1.changed().any()
    xo.changed()
    c1own = c1v[:, 1:F + 1].cpu()
    ref2, bound2 = pr.conv_gelu_ref(c1own, w2, b2, 2, F32, pos=pos)
    _check(f"stem/conv2<{nm}>", xo.t.view(B, T, D), ref2, bound2, f"n_mels={n_mels}")
    _sensitive(ref2, pr.conv_gelu_ref(c1own, w2, b2, 2, F32, pos=pos, flip=True)[0], bound2, "the tap order reversed")
    _sensitive(ref2, pr.conv_gelu_ref(c1own, w2, b2, 2, F32, pos=pos, offset=1)[0], bound2, "the stride-2 rows offset by one")


@pytest.mark.parametrize("T", [35, 1500])
def test_gemm_vt_form(gpu_device, T):
    """V^T = Wv . X^T as wh_encode launches it: A = the weight shared by the batch (a_bs = 0), W = the activations per batch
    (w_bs = T D), bias on m, ldc = 1536 with the pad columns poisoned"""
    dev, B, VT_LD = _dev(), 2, 1536
    g = torch.Generator().manual_seed(T)
    wv = (torch.randn(D, D, generator=g) * D ** -0.5).half()
    xn = torch.randn(B, T, D, generator=g).half()
    bias = (torch.randn(D, generator=g) * 0.5).float().to(dev)
    ab, wb = _buf_from(wv), _buf_from(xn)
    vt = Buf(B * D * VT_LD, torch.float16)
    for b in (ab, wb, vt):
        b.snapshot()
    e = lib().wht_gemm(F16, 0, B, ab.ptr(), D, 0, wb.ptr(), D, T * D, vt.ptr(), VT_LD, D * VT_LD, bias.data_ptr(), 1, None, 0, 0, 0,
                       0, D, T, D, _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not ab.changed().any() and not wb.changed().any()
    assert not vt.changed().view(B, D, VT_LD)[:, :, T:].any(), "V^T pad columns written"
    wd, xd, bd = wv.double(), xn.double(), bias.double().cpu().view(1, -1, 1)
    ref = wd @ xd.transpose(1, 2) + bd
    bound = _ulp(ref, F16) + C_DOT * (wd.abs() @ xd.abs().transpose(1, 2) + bd.abs())
    _check("gemm/vt_form", vt.t.view(B, D, VT_LD)[:, :, :T], ref, bound, f"T={T}")
    _sensitive(ref, ref - wd[:, D - 1].view(1, -1, 1) * xd[:, :, D - 1].unsqueeze(1), bound, "the last k-term dropped")


# ----------------------------------------------------------------------------------------------- small kernels
@pytest.mark.parametrize("dtype", [F16, F32])
def test_embed(gpu_device, dtype):
    """x[r T0 + t] = float(emb[clamp(token)]) + pos[offset - lag[r] + t], bit-equal to the fp32 computation"""
    dev, tdt = _dev(), _tdt(dtype)
    R, De, n_vocab, stride, n_pos = 3, 384, 50, 9, 16
    g = torch.Generator().manual_seed(4 + dtype)
    emb = torch.randn(n_vocab, De, generator=g).to(tdt)
    pos = torch.randn(n_pos, De, generator=g).float()
    embb, posb = _buf_from(emb), _buf_from(pos)
    for T0 in (1, 5):
        for (offset, lag) in ((0, None), (7, None), (7, [0, 2, 7])):
            toks = torch.randint(0, n_vocab, (R, stride), generator=g)
            toks[0, 0], toks[R - 1, T0 - 1] = -1, n_vocab
            toks[:, T0:] = 1 << 40                                  # beyond T0: never read (would clamp to the last row)
            tb = _buf_from(toks)
            x = Buf(R * T0 * De, torch.float32)
            off = _ints([offset])
            lg = _ints(lag) if lag else None
            for b in (embb, posb, tb, x):
                b.snapshot()
            e = lib().wht_embed(tb.ptr(), stride, R, T0, embb.ptr(), posb.ptr(), off.data_ptr(), lg.data_ptr() if lag else None, De,
                                n_vocab, x.ptr(), dtype, _stream())
            assert e == hipSuccess
            torch.cuda.synchronize()
            assert not embb.changed().any() and not posb.changed().any() and not tb.changed().any()
            x.changed()
            want = torch.empty(R, T0, De)
            for r in range(R):
                for t in range(T0):
                    tok = min(max(int(toks[r, t]), 0), n_vocab - 1)
                    want[r, t] = emb[tok].float() + pos[offset - (lag[r] if lag else 0) + t]
            _exact(f"embed<{_nm(dtype)}>", x.t.view(R, T0, De), want, f"T0={T0} offset={offset} lag={lag}")


@pytest.mark.parametrize("V", [1, 1000, 8192, 8193, 51866])
def test_no_speech(gpu_device, V):
    """softmax(row)[no_speech] of three rows `row_stride` apart: a plain one, one with -inf entries (among them the first
    ones a thread folds), one whose answer lies 80 below a dominant logit"""
    x, ns = pr.no_speech_inputs(V, seed=V)
    stride = V + 13
    rows = torch.full((3, stride), float("nan")); rows[:, :V] = x
    xb = _buf_from(rows)
    out = Buf(3, torch.float32)
    xb.snapshot(); out.snapshot()
    assert lib().wht_no_speech(xb.ptr(), stride, 3, V, ns, out.ptr(), _stream()) == hipSuccess
    torch.cuda.synchronize()
    assert not xb.changed().any()
    out.changed()
    ref, bound = pr.no_speech_ref(x, ns)
    _check("no_speech", out.t, ref, bound, f"V={V}")
    if V > 1:
        _sensitive(ref, pr.no_speech_ref(x, ns, drop_last=True)[0], bound, "the last logit dropped")


def test_gathers_exact(gpu_device):
    """gather_rows / gather_tokens with repeated and out-of-order indices"""
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    for De in (300, 384):
        x = torch.randn(7, De, generator=g).float()
        sel = [6, 0, 0, 3, 6, 2, 5, 1, 1]
        xb, out, ds = _buf_from(x), Buf(len(sel) * De, torch.float32), _ints(sel)
        xb.snapshot(); out.snapshot()
        assert lib().wht_gather_rows(xb.ptr(), ds.data_ptr(), len(sel), De, out.ptr(), _stream()) == hipSuccess
        torch.cuda.synchronize()
        assert not xb.changed().any()
        out.changed()
        _exact("gather_rows", out.t.view(len(sel), De), x[sel])
    R, stride = 70, 11
    src = torch.randint(-5, 1 << 40, (R, stride), generator=g)
    sb, dst = _buf_from(src), Buf(R, torch.int64)
    sb.snapshot(); dst.snapshot()
    assert lib().wht_gather_tokens(sb.ptr(), stride, R, dst.ptr(), _stream()) == hipSuccess
    torch.cuda.synchronize()
    assert not sb.changed().any()
    dst.changed()
    _exact("gather_tokens", dst.t, src[:, 0])


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals_and_dtw_rows(gpu_device):
    """more (row, pair) planes than grid.z holds, and more dtw rows than three diagonals in 64 KB of LDS hold
    (DTW_OPEN_MAX_ROWS = 5460), are refused on the host with hipErrorInvalidValue before anything is launched; 700 rows
    still run and give the oracle's trace"""
    from oracle.timing import dtw_trace
    dev, L, s = _dev(), lib(), _stream()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    ib = torch.zeros(64, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    assert L.wht_cross_qk_batch(p, 0, 0, 128, p, 0, 0, 1, ib.data_ptr(), ib.data_ptr(), 3, ib.data_ptr(), 21846, 1, 1, p, F16,
                                s) == hipErrorInvalidValue
    for N in (5461, 8192):
        assert L.wht_dtw(p, N, 4, p, s) == hipErrorInvalidValue
        assert L.wht_dtw_batch(p, ib.data_ptr(), ib.data_ptr(), 1, N, 4, 0, 0, N, p, (N + 1) * 5, s) == hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (buf == 0).all() and (ib == 0).all()
    N, M = 700, 50
    x = torch.randn(N, M, generator=torch.Generator().manual_seed(2)).float()
    want = torch.from_numpy(dtw_trace(x.numpy()))
    xb, dn, dm = _buf_from(x), _ints([N]), _ints([M])
    for batch in (False, True):
        tr = Buf((N + 1) * (M + 1), torch.int8)
        xb.snapshot(); tr.snapshot()
        if batch:
            e = L.wht_dtw_batch(xb.ptr(), dn.data_ptr(), dm.data_ptr(), 1, N, M, 0, 0, N, tr.ptr(), (N + 1) * (M + 1), s)
        else:
            e = L.wht_dtw(xb.ptr(), N, M, tr.ptr(), s)
        assert e == hipSuccess
        torch.cuda.synchronize()
        assert not xb.changed().any()
        tr.changed()
        _exact("dtw_batch" if batch else "dtw", tr.t.view(N + 1, M + 1), want)


# ----------------------------------------------------------------------------------------------------- coverage
EXPECTED_FORMS = sorted(
    [f"attn_generic<{t}>/{k}" for t in ("half", "float") for k in ("self", "cross")]
    + ["cross_qk<half>", "cross_qk<float>", "cross_qk_batch/mfma", "cross_qk_batch<float>"]
    + ["align/softmax_znorm", "align/head_mean", "align/end_to_end", "align/median_generic", "align/median_generic/passthrough"]
    + [f"align/median<{w}>" for w in (1, 3, 5, 7, 9, 11, 13)] + [f"align/median<{w}>/passthrough" for w in (3, 5, 7, 9, 11, 13)]
    + [f"mel_transpose<{i},{o}>" for i in ("half", "float") for o in ("half", "float")]
    + [f"stem/{c}<{t}>" for c in ("conv1", "conv2") for t in ("half", "float")]
    + ["gemm/vt_form", "embed<half>", "embed<float>", "no_speech", "gather_rows", "gather_tokens", "dtw", "dtw_batch"])


def test_coverage_and_report(gpu_device):
    """runs last: every form above was recorded, and each form's largest error / bound ratio goes to
    prefill_align_parity.json"""
    from conftest import write_report
    write_report("prefill_align_parity.json", {"bounds": {"C_DOT": C_DOT, "C_ATT_VALU": C_ATT_VALU, "U": pr.U},
                                               "max_ratio": dict(sorted(REPORT.items()))})
    missing, extra = sorted(set(EXPECTED_FORMS) - set(REPORT)), sorted(set(REPORT) - set(EXPECTED_FORMS))
    assert not missing and not extra, f"forms no case recorded: {missing}; forms not in EXPECTED_FORMS: {extra}"
    assert all(r <= 1.0 for r in REPORT.values())
