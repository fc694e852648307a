"""The references and bounds of tests/test_prefill_align_parity_gpu.py (tests/prefill_align_ref.py), checked without a GPU:
for every form a plain fp32 emulation of the kernel's order of operations passes the bound (so the bound is reachable and
not tuned to a GPU's output), every named perturbation of the reference fails it, the alignment reference equals
oracle.timing.alignment_matrix's arithmetic and the stem reference equals oracle.model's conv front end."""
import math
import types

import numpy as np
import pytest
import torch

import prefill_align_ref as pr
from parity_ref import F16, F32, _tdt


def _passes(got, ref, bound, what):
    r = pr.ratio(got, ref, bound)
    assert r <= 1.0, f"{what}: fp32 emulation at error / bound = {r:.3f}"


def _fails(ref, pert, bound, what):
    r = pr.ratio(pert, ref, bound)
    assert r > 1.0, f"{what}: the bound does not see it (ratio {r:.3f})"


@pytest.mark.parametrize("dtype", [F16, F32])
def test_generic_attention_bound(dtype):
    H, C = 2, 96
    for (d_len, Tq) in ((0, 1), (0, 17), (3, 5), (60, 17), (10, 70), (1, 64)):
        q, k, v = pr.attn_inputs(dtype, 1, 1, Tq, C, H, seed=d_len * 100 + Tq)
        qd, kd, vd = q[0].double(), k[0].double(), v[0].double()
        lim = d_len + 1 + torch.arange(Tq)
        a = pr.generic_attn_ref(qd, kd, vd, H, lim)
        bound = pr.generic_attn_bound(a, dtype)
        _passes(pr.generic_attn_emulate(q[0], k[0], v[0], H, lim, dtype), a["ref"], bound, f"self {d_len},{Tq}")
        if d_len + Tq >= 2:
            _fails(a["ref"], pr.generic_attn_ref(qd, kd, vd, H, lim, drop_last=True)["ref"], bound, "the last key dropped")
        _fails(a["ref"], pr.generic_attn_ref(qd, kd, vd, H, lim + 1)["ref"], bound, "the mask shifted by one")
    for (Tk, Tq) in ((1, 1), (63, 15), (65, 16), (1500, 33)):
        q, k, v = pr.attn_inputs(dtype, 6, 2, Tq, Tk, H, seed=Tk + Tq)
        lim = torch.full((Tq,), Tk)
        for b in (1, 5):
            qd = q[b].double()
            a = pr.generic_attn_ref(qd, k[b // 3].double(), v[b // 3].double(), H, lim)
            bound = pr.generic_attn_bound(a, dtype)
            _passes(pr.generic_attn_emulate(q[b], k[b // 3], v[b // 3], H, lim, dtype), a["ref"], bound, f"cross {Tk},{Tq}")
            if Tk >= 2:
                _fails(a["ref"], pr.generic_attn_ref(qd, k[b // 3].double(), v[b // 3].double(), H, lim, drop_last=True)["ref"],
                       bound, "the last key dropped")
            if b % 2 != b // 3:
                _fails(a["ref"], pr.generic_attn_ref(qd, k[b % 2].double(), v[b % 2].double(), H, lim)["ref"], bound,
                       "audio b % 2 instead of b / 3")


@pytest.mark.parametrize("dtype", [F16, F32])
def test_cross_qk_bound(dtype):
    for (T, Tk) in ((1, 1), (5, 257), (70, 129), (17, 1500)):
        g = torch.Generator().manual_seed(T + Tk)
        q = torch.randn(T, 128, generator=g).to(_tdt(dtype))
        k = torch.randn(Tk, 128, generator=g).to(_tdt(dtype))
        ref, bound = pr.cross_qk_ref(q[:, 64:].double(), k[:, 64:].double())
        _passes(pr.cross_qk_emulate(q[:, 64:], k[:, 64:]), ref, bound, f"cross_qk {T},{Tk}")
        _fails(ref, pr.cross_qk_ref(q[:, :64].double(), k[:, :64].double())[0], bound, "the head swapped")
        _fails(ref, pr.cross_qk_ref(q[:, 64:].double(), k[:, 64:].double(), drop_last_d=True)[0], bound, "the last d term dropped")


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_alignment_bounds(scale):
    H, rb, rt = 3, 1, 1
    qk = pr.align_inputs(3, H, 40, 320, seed=int(scale * 10))
    for width in (1, 3, 5, 7, 9, 11, 13, 15):
        for (b, T, F) in ((0, 2, 3), (1, 9, 37), (2, 40, 300)):
            w0r, b0, w1r, b1, costr, bc = pr.align_chain_ref(qk[b].double(), T, F, scale, width, rb, rt)
            w0, w1, cost = pr.align_emulate(qk[b], T, F, scale, width, rb, rt)
            _passes(w0, w0r, b0, f"stage a clip {b}")
            _passes(w1, w1r, b1, f"median clip {b} width {width}")
            c2, bc2 = pr.head_mean_ref(w1, T, rb, rt)
            if T > 2:
                _passes(cost, c2, bc2, f"head mean clip {b}")
                _passes(cost, costr, bc, f"end to end clip {b} width {width}")
        # the perturbations, on the clip every width filters (T = 40, F = 300)
        q2 = qk[2].double()
        _fails(w0r, pr.align_stage_a(q2, 40, 300, scale, soft_frames=301)[0], b0, "softmax over F + 1 frames")
        _fails(w0r, pr.align_stage_a(q2, 40, 300, scale, unbiased=True)[0], b0, "the unbiased std")
        _fails(costr, pr.align_chain_ref(q2, 40, 300, scale, width, rb, rt, shift=1)[4], bc, "the window shifted by one")
        _fails(costr, pr.align_chain_ref(q2, 40, 300, scale, width, rb + 1, rt - 1)[4], bc, "row_begin off by one")
        _fails(costr, pr.align_chain_ref(q2, 40, 300, scale, width, rb, rt, unbiased=True)[4], bc, "the unbiased std, end to end")


def test_alignment_degenerate_clip():
    """one frame: the softmax is exactly 1 for every token, its std over the tokens 0, and 0 / 0 = NaN — in the float64
    reference, in the fp32 emulation and in oracle.timing alike"""
    qk = pr.align_inputs(1, 3, 2, 8, seed=3)
    w0r, _ = pr.align_stage_a(qk[0].double(), 2, 1, 1.0)
    w0, w1, _ = pr.align_emulate(qk[0], 2, 1, 1.0, 7, 1, 1)
    assert torch.isnan(w0r).all() and torch.isnan(w0).all() and torch.isnan(w1).all()


def test_alignment_reference_is_the_oracles():
    """oracle.timing.alignment_matrix on the same qk (a stand-in model that only hands the scores over).  Its softmax and
    z-norm run in the scores' float64; its median_filter stores float32 and its head mean runs on those: the agreement is
    float64 round-off up to the median and (H + 1) float32 roundings of the largest |w1| behind it"""
    from oracle.timing import alignment_matrix
    H, T, F, n_sot = 3, 40, 300, 1
    qk = pr.align_inputs(1, H, T, 2 * F, seed=5)[0].double()

    class Model:
        def decoder(self, toks, feats, cache, keep_qk=False):
            self.last_qk = [qk[h][None, None] for h in range(H)]
            return torch.zeros(1, T, 4)

    for width in (1, 7, 15):
        for scale in (1.0, 0.5):
            got, _ = alignment_matrix(Model(), list(range(T)), None, 2 * F, [(h, 0) for h in range(H)], n_sot, width, scale)
            _, _, w1, _, cost, _ = pr.align_chain_ref(qk, T, F, scale, width, n_sot, 1)
            tol = (H + 1) * 2.0 ** -24 * w1.abs().max().item() + 1e-12
            assert got.shape == tuple(cost.shape)
            assert np.abs(got.astype(np.float64) + cost.numpy()).max() <= tol
    # up to the median the arithmetic is float64 on both sides
    w = (qk[:, :, :F] * 0.5).softmax(-1)
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    assert ((w - mean) / std - pr.align_stage_a(qk, T, F, 0.5)[0]).abs().max().item() < 1e-11
    from oracle.timing import median_filter
    x = torch.randn(5, 37).float().numpy()
    for width in (1, 3, 5, 7, 9, 11, 13, 15):
        assert np.array_equal(median_filter(x, width), pr.median_f64(x, width))


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("n_mels", [80, 128])
def test_stem_bounds(dtype, n_mels):
    D, F, B = 128, 70, 2
    tdt = _tdt(dtype)
    mel, w1, b1, w2, b2, pos = pr.stem_inputs(n_mels, D, F, B, dtype, seed=n_mels)
    x = mel.to(tdt).transpose(1, 2)
    ref1, bound1 = pr.conv_gelu_ref(x, w1, b1, 1, dtype)
    c1 = pr.conv_gelu_emulate(x, w1, b1, 1, tdt)
    _passes(c1, ref1, bound1, "conv1")
    _fails(ref1, pr.conv_gelu_ref(x, w1, b1, 1, dtype, flip=True)[0], bound1, "conv1: the tap order reversed")
    ref2, bound2 = pr.conv_gelu_ref(c1, w2, b2, 2, F32, pos=pos)
    _passes(pr.conv_gelu_emulate(c1, w2, b2, 2, torch.float32, pos=pos), ref2, bound2, "conv2")
    _fails(ref2, pr.conv_gelu_ref(c1, w2, b2, 2, F32, pos=pos, flip=True)[0], bound2, "conv2: the tap order reversed")
    _fails(ref2, pr.conv_gelu_ref(c1, w2, b2, 2, F32, pos=pos, offset=1)[0], bound2, "conv2: the stride-2 rows offset by one")


def test_stem_reference_is_the_oracles():
    """oracle.model.OracleModel.encoder with no blocks is the conv front end followed by ln_post"""
    from oracle.model import OracleModel
    D, F, B, n_mels = 128, 70, 2, 80
    mel, w1, b1, w2, b2, pos = pr.stem_inputs(n_mels, D, F, B, F32, seed=9)
    sd = {"encoder.conv1.weight": w1, "encoder.conv1.bias": b1, "encoder.conv2.weight": w2, "encoder.conv2.bias": b2,
          "encoder.positional_embedding": pos, "encoder.ln_post.weight": torch.ones(D), "encoder.ln_post.bias": torch.zeros(D)}
    dims = types.SimpleNamespace(n_audio_layer=0, n_audio_head=2)
    want = OracleModel(dims, sd, dtype=torch.float64).encoder(mel)
    ref1, _ = pr.conv_gelu_ref(mel.transpose(1, 2), w1, b1, 1, F32)
    ref2, _ = pr.conv_gelu_ref(ref1, w2, b2, 2, F32, pos=pos)
    mine = torch.nn.functional.layer_norm(ref2, (D,), eps=1e-5)
    assert (mine - want).abs().max().item() < 1e-11


def test_conv_packer_is_the_conv():
    """whisper_amd.hip._conv_as_gemm: overlapping rows of the padded, transposed input times the packed weight = conv1d"""
    from whisper_amd.hip import _conv_as_gemm
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 9, 5, generator=g, dtype=torch.float64)             # [B][F][C]
    w = torch.randn(4, 5, 3, generator=g, dtype=torch.float64)
    W = _conv_as_gemm(w, 64)
    assert W.shape == (4, 64) and (W[:, 15:] == 0).all()
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1))[0]
    rows = torch.stack([xp[t:t + 3].reshape(-1) for t in range(9)])
    want = torch.nn.functional.conv1d(x.transpose(1, 2), w, padding=1)[0].T
    assert (rows @ W[:, :15].T - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("V", [1, 1000, 8192, 8193, 51866])
def test_no_speech_bound(V):
    x, ns = pr.no_speech_inputs(V, seed=V)
    ref, bound = pr.no_speech_ref(x, ns)
    got = pr.no_speech_emulate(x, ns)
    assert torch.isfinite(got).all()
    _passes(got, ref, bound, f"no_speech V={V}")
    if V > 1:
        _fails(ref, pr.no_speech_ref(x, ns, drop_last=True)[0], bound, "the last logit dropped")
        # the recurrence without the -inf guard: expf(-inf - -inf) in every thread whose first logit is -inf
        assert math.isnan(pr.no_speech_emulate(x, ns, guard_inf=False)[1].item())
