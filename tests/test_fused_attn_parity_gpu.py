"""Per-element parity of the two fused attention launches of the decode step (whisper_amd/csrc/xattn.hip: xattn8_kernel,
sattn8_kernel) against float64, through libwhisper_hip_ktest.so (wht_xattn8 / wht_sattn8: the shipped objects).

Every stage the launch leaves visible is checked on its own, with the references of tests/parity_ref.py (checked against
oracle/model.py by tests/test_fused_attn_ref_cpu.py) and the bounds of tests/test_kernel_parity_gpu.py:

  q (cross: read back from the granules; self: q_out, the appended cache rows and all three granule planes)
      tag of every granule of rows < R exactly ((tick + 1 + epoch) << 6) | (layer + 1), rows >= R untouched;
      |8 payload - (W . LN(x) + b)| <= ulp_f16 + C_DOT sum |w x| + the LayerNorm rounding-flip slack (the PRO_LN GEMV
      bound), plus 8 * 2^-25 where |q| < 2^-10: the payload is the fp16 projection times 0.125, which is exact only while
      the product stays normal; and bit-equal to wht_gemv(PRO_LN) on the same inputs (times 0.125 for q).
  attention, from the kernel's OWN q (so the two stages' errors do not add up)
      per split (splits > 1; boundaries ceil(Tk / S) rounded up to 64 keys; an empty split holds o = 0, m = -inf, l = 0):
        |o_s - ref| <= ulp_f16 + C_ATT_VALU sum p |v| / sum p + 2^-21 sum p (1 + |s - m|) |v| / sum p
        |m_s - ref| <= E + ulp_f32,  E = 2^-20 max_j sum_d |q_d k_jd|   (a score is 64 fp16 products summed in fp32)
        |l_s - ref| <= l (2^-20 + 2.02 E) + 2^-21 sum_j p_j (1 + |s_j - m|)
            (every p_j = exp(s_j - m) moves by the errors of s_j and of m, by the exp argument's rounding, and the sum by its
            own 2^-20)
      merged output (wht_merge_partials on the partials, or `out` itself at one split): the attention bound of the existing
      file, unchanged, with C_ATT_VALU — the fused kernel sums a key range from 8 instead of 4 waves' partial sums and gets
      no looser constant for it.  The two-launch wht_attn_decode runs on the same q / K / V with its own split boundaries;
      both kernels' error / bound ratios go to fused_attn_parity.json.
  self attention: bit-equal altogether (q, appended K / V, output) to wht_gemv(PRO_LN, EPI_QKV) + the self form of
      wht_attn_decode, as the kernel's comment claims.

No constant of the existing file changes; the m / l constants above are new checks (the existing file judges the merged
output only) and follow from the fp32 formats as stated.

Poison: every buffer sits inside 0xFF guards; what a launch must not write (row gaps, unused outputs, granule rows >= R,
every cache byte other than the appended rows) is 0xFF and must come back byte-identical; don't-care inputs (x columns
beyond D, keys at or beyond Tk, cache positions at or beyond the cached length) hold NaN.  After every launch *err == 0.
Every family shows its bounds are not vacuous: a perturbed reference (last K block of the projection dropped, two rows
swapped, last key dropped, new key taken from the cache's old bytes, one split boundary moved by 32 keys) must fail.
"""
import pytest
import torch

from kernel_lib import hipSuccess, last_form, lib
from parity_ref import (C_ATT_VALU, C_DOT, F16, Buf, _dev, _r, _stream, _ulp, attn_bound, attn_ref, ln_gemv_ref,
                        self_block_ref)

pytestmark = pytest.mark.gpu

LN, STORE, QKV = 1, 0, 1
REPORT = {}                  # family -> {"fused": .., "two_launch": .., ...}: largest error / bound ratio
NAN_PAIR = 0x7E007E00        # two fp16 NaNs: the payload of a stale granule


def _record(family, key, ratio):
    d = REPORT.setdefault(family, {})
    d[key] = max(d.get(key, 0.0), float(ratio))


def _within(family, key, got, ref, bound, what):
    got = got.double()
    assert torch.isfinite(got).all(), f"{family} {what}: non-finite {key}"
    ratio = ((got - ref).abs() / bound).max().item()
    _record(family, key, ratio)
    assert ratio <= 1.0, f"{family} {what}: {key} error / bound = {ratio:.3f}"


def _fails(ref, pert, bound, what):
    r = ((pert - ref).abs() / bound).max().item()
    assert r > 1.0, f"bound too loose to see {what} (ratio {r:.3f})"


def _tag(tick, epoch, layer):
    return ((tick + 1 + epoch) << 6) | (layer + 1)


def _gran_read(qg, n):
    """(tags [8][n] int64, payload [8][2n] fp16) of a granule buffer of 8 rows x n granules"""
    tags = (qg.t.view(8, n) >> 32) & 0xFFFFFFFF
    pay = qg.t.view(torch.float16).view(8, n, 4)[:, :, :2].reshape(8, 2 * n)
    return tags, pay


def _gran_stale(qg, n, tick, epoch, layer):
    """NaN payloads under plausible wrong tags: the previous tick, this tick with another layer, tag 0 (one per row, in turn)"""
    tags = [_tag(tick - 1, epoch, layer), _tag(tick, epoch, layer + 1), 0]
    rows = torch.tensor([(tags[r % 3] << 32) | NAN_PAIR for r in range(8)], dtype=torch.int64, device=_dev())
    qg.t.view(8, n).copy_(rows.view(8, 1).expand(8, n))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _x_rows(kind, R, D, g):
    x = torch.randn(R, D, generator=g, dtype=torch.float64) * 1.3 + 0.2
    if kind == "mean1e3":
        x = torch.randn(R, D, generator=g, dtype=torch.float64) + 1e3
    elif kind == "const":
        x[0] = 2.5                                                 # variance 0
    return x.float()


def _gemv_ln(xf, xf_ld, W, bias, N, D, R, epi, y, y_ld, kc=None, vc=None, cache_bs=0, pos=None, lag=None):
    one, zero = torch.ones(D, device=_dev()), torch.zeros(D, device=_dev())
    lib().wht_clear_form()
    e = lib().wht_gemv(F16, LN, None, 0, xf.ptr(), xf_ld, one.data_ptr(), zero.data_ptr(), 1, None, None, 1, 0, W.data_ptr(),
                       bias.data_ptr(), N, D, R, 0, 0, epi, y.ptr(), y_ld, None, 0, kc.ptr() if kc else None,
                       vc.ptr() if vc else None, cache_bs, pos.data_ptr() if pos is not None else None, D if kc else 0,
                       lag.data_ptr() if lag is not None else None, None, 0, None, _stream())
    assert e == hipSuccess, f"wht_gemv: hipError {e}"
    torch.cuda.synchronize()
    return last_form()


# ------------------------------------------------------------------------------------------------ cross attention
def _xattn_case(family, D, R, Tk, S, mode=1, layout="inter", xkind="normal", skind="normal", stale=False, shift=False,
                seed=0):
    """one wht_xattn8 launch (three with `stale`) against float64, stage by stage"""
    dev = _dev()
    H = D // 64
    what = f"D={D} R={R} Tk={Tk} S={S} mode={mode} {layout} {xkind} {skind}"
    assert lib().wht_xattn_supported(D, H, R, 1, Tk, S), what
    g = torch.Generator().manual_seed(seed * 7919 + D * 13 + R * 131 + Tk * 17 + S)
    tick, epoch, layer = 41 + seed, 3, 5
    W = (torch.randn(D, D, generator=g) * D ** -0.5).half().to(dev)
    bias = (torch.randn(D, generator=g) * 0.5).float().to(dev)
    xf_ld = D if layout == "inter" else D + 8
    xb = Buf(R * xf_ld, torch.float32)                             # columns D .. xf_ld - 1 stay NaN

    def set_x(kind):
        xv = _x_rows(kind, R, D, g).to(dev)
        xb.t.view(R, xf_ld)[:, :D] = xv
        return xv
    xv = set_x(xkind)

    # ---- K / V: keys >= Tk of every row are NaN (0xFF); the product's interleaved layout, or two buffers with their own strides
    cap = Tk + 3
    kh = torch.randn(R, Tk, D, generator=g).half()
    vh = torch.randn(R, Tk, D, generator=g).half()
    chunk = -(-(-(-Tk // S)) // 64) * 64
    if skind != "normal":
        pre0, _, _ = ln_gemv_ref(xv, W, bias, F16)
        q0 = _r(_r(pre0, F16) * 0.125, F16).cpu().view(R, H, 64)     # the scaled q the kernel will hold (to its rounding)
        unit = (q0 / (q0 * q0).sum(-1, keepdim=True)).view(R, 1, D)  # unit[r, 0, head h] . q = 1
        if skind == "equal":                                        # all keys of a row alike: all-equal scores
            kh[:] = kh[:, :1].clone()
        elif skind == "peak":                                       # one key dominant by more than 30
            kh[:, Tk // 3] = (kh[:, Tk // 3].double() + unit[:, 0] * 40).half()
        elif skind == "underflow":                                  # the last non-empty split's maximum > 90 below the global one
            lo = (Tk - 1) // chunk * chunk
            assert lo > 0
            kh[:, lo:] = (kh[:, lo:].double() * 0.2 - unit * 50).half()
            kh[:, 1] = (unit[:, 0] * 50).half()
    if layout == "inter":
        k_ld = v_ld = 2 * D
        k_bs = v_bs = cap * 2 * D
        kvb = Buf(R * k_bs, torch.float16)
        kvb.t.view(R, cap, 2 * D)[:, :Tk, :D] = kh.to(dev)
        kvb.t.view(R, cap, 2 * D)[:, :Tk, D:] = vh.to(dev)
        kptr, vptr, kvbufs = kvb.ptr(), kvb.ptr() + 2 * D, (kvb,)
    else:
        k_ld, v_ld = D + 16, D + 64
        k_bs, v_bs = cap * k_ld + 24, cap * v_ld + 8
        kb, vb = Buf(R * k_bs, torch.float16), Buf(R * v_bs, torch.float16)
        kb.t.view(R, k_bs)[:, :cap * k_ld].view(R, cap, k_ld)[:, :Tk, :D] = kh.to(dev)
        vb.t.view(R, v_bs)[:, :cap * v_ld].view(R, cap, v_ld)[:, :Tk, :D] = vh.to(dev)
        kptr, vptr, kvbufs = kb.ptr(), vb.ptr(), (kb, vb)
    kv = lambda r, h: (kh[r, :, h * 64:(h + 1) * 64].double(), vh[r, :, h * 64:(h + 1) * 64].double())

    o_ld = D + 64
    out = Buf(R * o_ld, torch.float16)
    po, pml = Buf(S * R * H * 64, torch.float16), Buf(S * R * H * 2, torch.float32)
    qg = Buf(8 * (D // 2), torch.int64)
    d_tick = torch.tensor([tick], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    y = Buf(R * D, torch.float16)
    out2 = Buf(R * o_ld, torch.float16)
    po2, pml2 = Buf(S * R * H * 64, torch.float16), Buf(S * R * H * 2, torch.float32)

    def launch(tick_now):
        for b in (po, pml):
            b.raw.view(torch.uint8).fill_(0xFF)
        for b in (xb, out, po, pml, qg) + kvbufs:
            b.snapshot()
        e = lib().wht_xattn8(xb.ptr(), xf_ld, W.data_ptr(), bias.data_ptr(), D, H, R, kptr, k_ld, k_bs, vptr, v_ld, v_bs, Tk,
                             S, out.ptr(), o_ld, po.ptr(), pml.ptr(), qg.ptr(), d_tick.data_ptr(), epoch, layer,
                             err.data_ptr(), mode, None, _stream())
        assert e == hipSuccess, f"wht_xattn8 {what}: hipError {e}"
        torch.cuda.synchronize()
        assert err.item() == 0, f"{what}: {err.item()} hand-off spins ran out"
        assert d_tick.item() == tick_now
        for b in (xb,) + kvbufs:
            assert not b.changed().any(), f"{what}: an input was written"
        # ---- granules: rows < R carry this launch's tag, rows >= R are untouched
        tags, pay = _gran_read(qg, D // 2)
        assert (tags[:R] == _tag(tick_now, epoch, layer)).all(), f"{what}: wrong granule tag"
        assert not qg.changed().view(8, D // 2)[R:].any(), f"{what}: granules of rows >= R written"
        # ---- outputs: splits == 1 writes `out` rows only, splits > 1 the partials only
        if S == 1:
            w = out.changed().view(R, o_ld)
            assert w[:, :D].all() and not w[:, D:].any(), f"{what}: out row gap written / row not written"
            assert not po.changed().any() and not pml.changed().any(), f"{what}: partials written at one split"
        else:
            assert not out.changed().any(), f"{what}: out written with splits"
            assert po.changed().all() and pml.changed().all(), f"{what}: a partial was not written"
        return pay[:R].clone()

    def check(xv, pay, first):
        # ---- stage 1: q against float64 and against the two-launch projection
        pre, slack, _ = ln_gemv_ref(xv, W, bias, F16)
        qb = _ulp(pre, F16) + slack + (pre.abs() < 2.0 ** -10) * 2.0 ** -22
        _within(family, "fused_q", pay.double() * 8.0, pre, qb, what)
        form = _gemv_ln(xb, xf_ld, W, bias, D, D, R, STORE, y, D)
        want = (y.t.view(R, D).float() * 0.125).half()
        assert torch.equal(_bits(pay), _bits(want)), f"{what}: q differs from wht_gemv ({form}) x 0.125"
        if first:
            if xkind == "normal":
                _fails(pre, ln_gemv_ref(xv, W, bias, F16, drop_last_block=True)[0], qb, "the last K block dropped")
            if R >= 2:
                _fails(pre, pre[[1, 0] + list(range(2, R))], qb, "two rows swapped")
        # ---- stage 2: attention from the kernel's own q
        qs = pay.double().cpu()
        peak = skind in ("peak", "underflow")
        a = attn_ref(qs, kv, [Tk] * R, S, 64, F16, H, peak=peak)
        if S > 1:
            pk = po.t.view(S, R, D).double().cpu()
            ml = pml.t.view(S, R, H, 2).double().cpu()
            empty = torch.isinf(a["pm"])
            for s in range(S):
                assert bool(empty[s].all()) == (s * chunk >= Tk) and bool(empty[s].any()) == (s * chunk >= Tk)
            assert (pk[empty.repeat_interleave(64, 2)] == 0).all(), f"{what}: an empty split's o is not 0"
            assert (ml[..., 0][empty] == float("-inf")).all() and (ml[..., 1][empty] == 0).all(), f"{what}: empty split (m, l)"
            live = ~empty
            E = 2.0 ** -20 * a["pe_s"]
            bo = _ulp(a["po"], F16) + C_ATT_VALU * a["ppv"] + 2.0 ** -21 * a["ppe"]
            bm = E + _ulp(a["pm"].clamp_min(-1e30), 0)
            bl = a["pl"] * (2.0 ** -20 + 2.02 * E) + 2.0 ** -21 * a["plw"]
            lv = live.repeat_interleave(64, 2)
            _within(family, "fused_part_o", pk[lv], a["po"][lv], bo[lv], what)
            _within(family, "fused_part_m", ml[..., 0][live], a["pm"][live], bm[live], what)
            _within(family, "fused_part_l", ml[..., 1][live], a["pl"][live], bl[live], what)
            if shift and first and Tk > chunk + 32:
                sh = attn_ref(qs, kv, [Tk] * R, S, 64, F16, H, peak=peak, shift=(1, 32))
                for s in (0, 1):
                    _fails(a["pl"][s], sh["pl"][s], bl[s], "one split boundary moved by 32 keys")
            e = lib().wht_merge_partials(po.ptr(), pml.ptr(), S, R, H, out.ptr(), o_ld, F16, 0, _stream())
            assert e == hipSuccess
            torch.cuda.synchronize()
            w = out.changed().view(R, o_ld)
            assert not w[:, D:].any()
        got = out.t.view(R, o_ld)[:, :D].cpu()
        bound = attn_bound(a, S, C_ATT_VALU, F16)
        _within(family, "fused", got, a["ref"], bound, what)
        if first and Tk >= 2:
            _fails(a["ref"], a["pert"], bound, "the last key dropped")
        # ---- the two-launch kernel on the same q / K / V (its own boundaries: rounds of 32 keys)
        lib().wht_clear_form()
        out2.snapshot()
        e = lib().wht_attn_decode(F16, y.ptr(), D, kptr, k_ld, k_bs, vptr, v_ld, v_bs, 0, H, R, 1, Tk, None, 0, None, S,
                                  out2.ptr(), o_ld, 0, po2.ptr(), pml2.ptr(), None, None, 0, 0, _stream())
        assert e == hipSuccess, f"wht_attn_decode {what}: hipError {e}"
        form2 = last_form()
        if S > 1:
            assert lib().wht_merge_partials(po2.ptr(), pml2.ptr(), S, R, H, out2.ptr(), o_ld, F16, 0, _stream()) == hipSuccess
        torch.cuda.synchronize()
        assert form2.startswith("attn/rounds<half"), form2
        a2 = attn_ref(qs, kv, [Tk] * R, S, 32, F16, H, peak=peak)
        _within(family, "two_launch", out2.t.view(R, o_ld)[:, :D].cpu(), a2["ref"], attn_bound(a2, S, C_ATT_VALU, F16), what)
        return got

    if not stale:
        check(xv, launch(tick), True)
        return
    # ---- stale granules: the same launch over NaN payloads under wrong tags gives the same bits ...
    pay = launch(tick)
    got = check(xv, pay, True)
    parts = (_bits(po.t).clone(), pml.t.view(torch.int32).clone())
    _gran_stale(qg, D // 2, tick, epoch, layer)
    if S == 1:
        out.raw.view(torch.uint8).fill_(0xFF)
    pay2 = launch(tick)
    assert torch.equal(_bits(pay2), _bits(pay)), f"{what}: stale granules changed q"
    if S == 1:
        assert torch.equal(_bits(out.t.view(R, o_ld)[:, :D].cpu()), _bits(got)), f"{what}: stale granules changed the result"
    else:
        assert torch.equal(_bits(po.t), parts[0]) and torch.equal(pml.t.view(torch.int32), parts[1]), \
            f"{what}: stale granules changed the result"
    # ... and the next tick with another x follows the new x (the granules of this tick are the stale ones now)
    d_tick.fill_(tick + 1)
    xv2 = set_x("normal")
    out.raw.view(torch.uint8).fill_(0xFF)
    pay3 = launch(tick + 1)
    assert not torch.equal(_bits(pay3), _bits(pay))
    check(xv2, pay3, False)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D,R,Tk,S", [(1280, 8, 1500, 3), (1280, 6, 1500, 4), (1280, 1, 1500, 16)])
def test_xattn_headline_instantiations(gpu_device, D, R, Tk, S, mode):
    """NL = 8 (the headline), NL = 6, and NL = 4 with the empty trailing splits 12 - 15 whose clamp used to point at key k0
    >= 1536: every key at or beyond Tk is NaN here and 3 keys further the row (for the last row: the allocation) ends"""
    _xattn_case("headline", D, R, Tk, S, mode=mode, shift=(mode == 1))


def test_xattn_single_split_store(gpu_device):
    """splits == 1: `out` written directly, o_ld > D; Tk around the 64-key round"""
    for i, Tk in enumerate((1, 7, 63, 64, 65, 511, 512)):
        _xattn_case("single_split", 64, 8, Tk, 1, mode=i & 1)


def test_xattn_row_clamps(gpu_device):
    """R below 8: rows aw + 4 >= R fall back to row R - 1 in the projection; the smallest legal split count per R"""
    for R in (1, 2, 3, 5, 7, 8):
        _xattn_case("row_clamps", 128, R, 200, -(-8 // R), mode=R & 1, shift=True)


@pytest.mark.parametrize("D", [320, 448, 576, 960, 1216])
def test_xattn_k_block_tails(gpu_device, D):
    """nblk = 5, 7, 9, 15, 19: the clamped weight blocks and the masked LayerNorm tail of the projection"""
    for S in (1, 2):
        for mode in ((0, 1) if D == 448 else (S & 1,)):
            _xattn_case("k_block_tails", D, 8, 130, S, mode=mode, shift=True)


def test_xattn_mostly_empty_splits(gpu_device):
    """Tk < 64 (S - 1): only the first two of 8 splits hold keys"""
    _xattn_case("empty_splits", 128, 1, 100, 8)
    _xattn_case("empty_splits", 1280, 2, 100, 8, mode=0)
    _xattn_case("empty_splits", 64, 8, 20, 8)


@pytest.mark.parametrize("D,R,Tk,S", [(1280, 8, 1500, 3), (320, 8, 130, 2), (64, 8, 65, 1), (128, 3, 200, 3), (128, 1, 1500, 16)])
def test_xattn_separate_kv_strides(gpu_device, D, R, Tk, S):
    """separate K and V buffers, k_ld != v_ld, a gap in k_bs, xf_ld > D (the gaps hold NaN)"""
    _xattn_case("strides", D, R, Tk, S, layout="sep", mode=R & 1)


@pytest.mark.parametrize("D,R,Tk,S,mode", [(128, 3, 200, 3, 0), (128, 3, 200, 3, 1), (64, 8, 65, 1, 0), (64, 8, 65, 1, 1),
                                           (1280, 8, 1500, 3, 1)])
def test_xattn_stale_granules(gpu_device, D, R, Tk, S, mode):
    """NaN payloads under the previous tick's tag, another layer's tag and tag 0 are never taken; the next tick follows the new x"""
    _xattn_case("stale", D, R, Tk, S, mode=mode, stale=True)


@pytest.mark.parametrize("xkind", ["mean1e3", "const"])
def test_xattn_layernorm_edges(gpu_device, xkind):
    """rows of mean 1e3 and spread 1; a constant row (variance 0)"""
    _xattn_case("edges_ln", 128, 4, 200, 2, xkind=xkind)
    _xattn_case("edges_ln", 1216, 8, 130, 1, xkind=xkind, mode=0)


@pytest.mark.parametrize("skind", ["peak", "equal", "underflow"])
def test_xattn_score_edges(gpu_device, skind):
    """a key dominant by more than 30; all-equal scores; a split whose maximum lies > 90 below the global one"""
    _xattn_case("edges_scores", 128, 4, 200, 2, skind=skind)
    _xattn_case("edges_scores", 1280, 8, 1500, 3, skind=skind)


# ------------------------------------------------------------------------------------------------- self attention
def _sattn_case(family, D, R, pos, lags=None, mode=0, old_nan=False, stale=False, seed=0):
    """one wht_sattn8 launch against float64 and against wht_gemv(PRO_LN, EPI_QKV) + the self form of wht_attn_decode"""
    dev = _dev()
    H = D // 64
    what = f"D={D} R={R} pos={pos} lags={lags} mode={mode}"
    n_ctx = 448 if pos >= 440 else pos + 5
    assert lib().wht_sattn_supported(D, H, R, n_ctx), what
    g = torch.Generator().manual_seed(seed * 7919 + D * 13 + R * 131 + pos * 17)
    tick, epoch, layer = 77 + seed, 1, 2
    W = (torch.randn(3 * D, D, generator=g) * D ** -0.5).half().to(dev)
    bias = (torch.randn(3 * D, generator=g) * 0.5).float().to(dev)
    xf_ld = D + 4
    xb = Buf(R * xf_ld, torch.float32)
    xv = _x_rows("normal", R, D, g).to(dev)
    xb.t.view(R, xf_ld)[:, :D] = xv
    at = [pos - (lags[r] if lags else 0) for r in range(R)]
    assert min(at) >= 0 and max(at) < n_ctx
    kc0 = torch.randn(R, n_ctx, D, generator=g).half()
    vc0 = torch.randn(R, n_ctx, D, generator=g).half()
    for r in range(R):                             # positions behind the new one: NaN; the slot itself: NaN or old finite bytes
        kc0[r, at[r] + (0 if old_nan else 1):] = float("nan")
        vc0[r, at[r] + (0 if old_nan else 1):] = float("nan")
    cache_bs = n_ctx * D
    kc, vc, kc2, vc2 = (Buf(R * cache_bs, torch.float16) for _ in range(4))
    for b, src in ((kc, kc0), (vc, vc0), (kc2, kc0), (vc2, vc0)):
        b.t.copy_(src.reshape(-1).to(dev))
    o_ld = D + 64
    out, out2 = Buf(R * o_ld, torch.float16), Buf(R * o_ld, torch.float16)
    q_out, y2 = Buf(R * D, torch.float16), Buf(R * 3 * D, torch.float16)
    n = 3 * D // 2
    qg = Buf(8 * n, torch.int64)
    if stale:
        _gran_stale(qg, n, tick, epoch, layer)
    d_pos = torch.tensor([pos], dtype=torch.int32, device=dev)
    lagt = torch.tensor(lags, dtype=torch.int32, device=dev) if lags else None
    d_tick = torch.tensor([tick], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for b in (xb, kc, vc, out, q_out, qg):
        b.snapshot()
    e = lib().wht_sattn8(xb.ptr(), xf_ld, W.data_ptr(), bias.data_ptr(), D, H, R, kc.ptr(), vc.ptr(), cache_bs,
                         d_pos.data_ptr(), lagt.data_ptr() if lagt is not None else None, q_out.ptr(), out.ptr(), o_ld,
                         qg.ptr(), d_tick.data_ptr(), epoch, layer, err.data_ptr(), mode, None, _stream())
    assert e == hipSuccess, f"wht_sattn8 {what}: hipError {e}"
    torch.cuda.synchronize()
    assert err.item() == 0, f"{what}: {err.item()} hand-off spins ran out"
    assert d_pos.item() == pos and d_tick.item() == tick
    assert not xb.changed().any(), f"{what}: x written"
    # ---- what was written: the appended rows only, q_out, the out rows, the granules of rows < R
    knew = torch.empty(R, D, dtype=torch.float16, device=dev)
    vnew = torch.empty_like(knew)
    for name, cb, dst in (("k", kc, knew), ("v", vc, vnew)):
        w = cb.changed().view(R, n_ctx, D)
        for r in range(R):
            # (a slot that held finite bytes may keep an element that happens to equal the new one: the bit-equality with
            # the two-launch form below covers the slot's content either way)
            assert (w[r, at[r]].all() or not old_nan) and not w[r, :at[r]].any() and not w[r, at[r] + 1:].any(), \
                f"{what}: {name} cache of row {r} written outside position {at[r]}"
            dst[r] = cb.t.view(R, n_ctx, D)[r, at[r]]
    assert q_out.changed().all()
    w = out.changed().view(R, o_ld)
    assert w[:, :D].all() and not w[:, D:].any(), f"{what}: out row gap written / row not written"
    tags, pay = _gran_read(qg, n)
    assert (tags[:R] == _tag(tick, epoch, layer)).all(), f"{what}: wrong granule tag"
    assert not qg.changed().view(8, n)[R:].any(), f"{what}: granules of rows >= R written"
    qv = q_out.t.view(R, D)
    planes = torch.cat([(qv.float() * 0.125).half(), knew, vnew], 1)
    assert torch.equal(_bits(pay[:R]), _bits(planes)), f"{what}: granule planes differ from q_out x 0.125 / the appended rows"
    # ---- projection against float64; attention from the kernel's own q / k / v
    qkv = torch.cat([qv, knew, vnew], 1)
    pre, slack, kcr, vcr, lens, a = self_block_ref(xv, W, bias, kc0.double(), vc0.double(), pos, lags, F16, H, qkv=qkv.double())
    pb = _ulp(pre, F16) + slack
    _within(family, "fused_qkv", qkv, pre, pb, what)
    _fails(pre, ln_gemv_ref(xv, W, bias, F16, drop_last_block=True)[0], pb, "the last K block dropped")
    if R >= 2:
        _fails(pre, pre[[1, 0] + list(range(2, R))], pb, "two rows swapped")
    assert lens == [p + 1 for p in at]
    got = out.t.view(R, o_ld)[:, :D].cpu()
    bound = attn_bound(a, 1, C_ATT_VALU, F16)
    _within(family, "fused", got, a["ref"], bound, what)
    if min(lens) >= 2:
        _fails(a["ref"], a["pert"], bound, "the last (new) key dropped")
    if not old_nan:                                # the new key / value taken from the bytes the slot held before
        old = attn_ref(_r(qv.double().cpu() * 0.125, F16),
                       lambda r, h: (kc0[r, :, h * 64:(h + 1) * 64].double(), vc0[r, :, h * 64:(h + 1) * 64].double()), lens, 1,
                       64, F16, H)
        _fails(a["ref"], old["ref"], bound, "the new key taken from the cache's old bytes")
    # ---- bit-equal altogether to the two-launch form
    form = _gemv_ln(xb, xf_ld, W, bias, 3 * D, D, R, QKV, y2, 3 * D, kc2, vc2, cache_bs, d_pos, lagt)
    lib().wht_clear_form()
    e = lib().wht_attn_decode(F16, y2.ptr(), 3 * D, kc2.ptr(), D, cache_bs, vc2.ptr(), D, cache_bs, 0, H, R, 1, pos + 1,
                              d_pos.data_ptr(), 1, lagt.data_ptr() if lagt is not None else None, 1, out2.ptr(), o_ld, 0,
                              None, None, None, None, 0, 0, _stream())
    assert e == hipSuccess, f"wht_attn_decode {what}: hipError {e}"
    torch.cuda.synchronize()
    assert last_form() == "attn/self<half>"
    assert torch.equal(_bits(qv), _bits(y2.t.view(R, 3 * D)[:, :D])), f"{what}: q differs from wht_gemv ({form})"
    assert torch.equal(kc.t.view(torch.int16), kc2.t.view(torch.int16)) and \
        torch.equal(vc.t.view(torch.int16), vc2.t.view(torch.int16)), f"{what}: the caches differ from wht_gemv's ({form})"
    got2 = out2.t.view(R, o_ld)[:, :D].cpu()
    _within(family, "two_launch", got2, a["ref"], bound, what)
    assert torch.equal(_bits(got), _bits(got2)), f"{what}: output differs from the two-launch form"


@pytest.mark.parametrize("D", [64, 128, 320, 768, 1280])
def test_sattn_shapes(gpu_device, D):
    """every D x R at Tk = 2, 65 and 448 (pos = Tk - 1), both poll modes"""
    for R in (1, 3, 8):
        for i, Tk in enumerate((2, 65, 448)):
            _sattn_case("self_shapes", D, R, Tk - 1, mode=(i + R) & 1)


@pytest.mark.parametrize("Tk", [1, 2, 63, 64, 65, 128, 129, 447, 448])
def test_sattn_cached_lengths(gpu_device, Tk):
    """Tk through d_pos: 1 (nothing cached: every masked tile slot loads position 0, the slot being appended, whose old bytes
    are NaN here — the kernel must select 0 for them, not multiply by 0), the 64-key rounds, and the full context; lag == nullptr"""
    for (D, R) in ((128, 3), (1280, 8)):
        for mode in (0, 1):
            _sattn_case("self_lengths", D, R, Tk - 1, mode=mode, old_nan=(Tk == 1 or mode == 1))
    if Tk == 1:
        for D in (64, 320, 768):
            _sattn_case("self_lengths", D, 8, 0, old_nan=True)


def test_sattn_ragged_rows(gpu_device):
    """per-row lag: rows on both sides of a 64-key round boundary (Tk_r = 67 - lag[r] = 67, 64, 66, 63, 65, ...)"""
    lag8 = [0, 3, 1, 4, 2, 0, 5, 1]
    for (D, R) in ((128, 8), (1280, 8), (320, 3), (768, 5)):
        for mode in (0, 1):
            _sattn_case("self_ragged", D, R, 66, lags=lag8[:R], mode=mode)
    _sattn_case("self_ragged", 128, 8, 5, lags=lag8, old_nan=True)     # row 6 appends at position 0


def test_sattn_stale_granules(gpu_device):
    for (D, R, pos, mode) in ((128, 3, 65, 0), (128, 3, 65, 1), (1280, 8, 130, 0), (1280, 8, 130, 1)):
        _sattn_case("self_stale", D, R, pos, mode=mode, stale=True)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(gpu_device):
    """what the launchers refuse is refused on the host: a non-zero hipError_t, nothing launched, nothing written"""
    dev = _dev()
    L = lib()
    assert L.wht_fused_mode(0) == 1 and L.wht_fused_mode(1) == 0        # shipped defaults: scalar polls (cross), vector (self)
    buf = torch.zeros(1 << 22, dtype=torch.float16, device=dev)
    fbuf = torch.zeros(1 << 20, dtype=torch.float32, device=dev)
    ibuf = torch.zeros(64, dtype=torch.int32, device=dev)
    p, pf, pi, s = buf.data_ptr(), fbuf.data_ptr(), ibuf.data_ptr(), _stream()

    def xa(D, R, Tk, S, H=None, k_ld=None, out_w=None):
        H = D // 64 if H is None else H
        k_ld = 2 * D if k_ld is None else k_ld
        return L.wht_xattn8(pf, D, p, pf, D, H, R, p, k_ld, Tk * k_ld, p, k_ld, Tk * k_ld, Tk, S, p, D, p, pf, p, pi, 0, 0,
                            pi + 4, 1, out_w, s)

    assert L.wht_xattn_supported(128, 2, 4, 1, 100, 2) and L.wht_sattn_supported(128, 2, 4, 448)   # the shapes varied below
    for (what, args, kw) in (("R = 9", (1280, 9, 1500, 3), {}), ("D = 1344", (1344, 8, 1500, 3), {}),
                             ("D = 96", (96, 8, 100, 1), {"H": 1}), ("H * 64 != D", (128, 8, 100, 1), {"H": 3}),
                             ("S H R < D / 8", (1280, 1, 1500, 4), {}), ("chunk > 512 keys", (1280, 8, 1500, 2), {}),
                             ("Tk = 0", (128, 8, 0, 1), {}), ("splits = 0", (128, 8, 100, 0), {}),
                             ("k_ld * 2048 overflows", (128, 8, 100, 1), {"k_ld": 1 << 20}),
                             ("out_w in the shipped build", (128, 4, 100, 2), {"out_w": p})):
        assert xa(*args, **kw) != hipSuccess, f"wht_xattn8 took {what}"
        if what not in ("k_ld * 2048 overflows", "out_w in the shipped build", "Tk = 0"):
            a = args
            assert not L.wht_xattn_supported(a[0], kw.get("H", a[0] // 64), a[1], 1, a[2], a[3]), what

    def sa(D, R, H=None, n_ctx=448, x_out=None):
        H = D // 64 if H is None else H
        return L.wht_sattn8(pf, D, p, pf, D, H, R, p, p + (1 << 22), n_ctx * D, pi, None, p, p, D, p, pi + 4, 0, 0, pi + 8, 0,
                            x_out, s)
    for (what, args, kw) in (("R = 9", (1280, 9), {}), ("R = 0", (128, 0), {}), ("D = 1344", (1344, 8), {}),
                             ("D = 96", (96, 8), {"H": 1}), ("D = 0", (0, 8), {"H": 0}), ("H * 64 != D", (128, 8), {"H": 3}),
                             ("H R > 3 D / 8", (64, 8), {"H": 4}), ("n_ctx = 449", (128, 8), {"n_ctx": 449}),
                             ("x_out in the shipped build", (128, 4), {"x_out": pf})):
        assert sa(*args, **kw) != hipSuccess, f"wht_sattn8 took {what}"
    assert not L.wht_sattn_supported(1280, 20, 9, 448) and not L.wht_sattn_supported(128, 2, 8, 449)
    torch.cuda.synchronize()
    assert (buf == 0).all() and (fbuf == 0).all() and (ibuf == 0).all()


# -------------------------------------------------------------------------------------------------------- report
def test_report(gpu_device):
    """runs last: every family was measured for the fused and the two-launch kernel, every ratio is <= 1, and the figures
    go to fused_attn_parity.json"""
    from conftest import write_report
    write_report("fused_attn_parity.json", {"bounds": {"C_DOT": C_DOT, "C_ATT_VALU": C_ATT_VALU, "E_SCORE": 2.0 ** -20,
                                                       "L_SUM": 2.0 ** -20, "EXP_ARG": 2.0 ** -21},
                                            "max_ratio": {k: dict(sorted(v.items())) for k, v in sorted(REPORT.items())}})
    want = {"headline", "single_split", "row_clamps", "k_block_tails", "empty_splits", "strides", "stale", "edges_ln",
            "edges_scores", "self_shapes", "self_lengths", "self_ragged", "self_stale"}
    assert set(REPORT) == want, sorted(set(REPORT) ^ want)
    for fam, d in REPORT.items():
        assert "fused" in d and "two_launch" in d, fam
        assert max(d.values()) <= 1.0, (fam, d)
