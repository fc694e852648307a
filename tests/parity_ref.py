"""Shared pieces of the per-element kernel parity suites (tests/test_kernel_parity_gpu.py, tests/test_fused_attn_parity_gpu.py):
guarded device buffers, the ulp / rounding-flip / merge budgets and the float64 references of the LayerNorm-folded projection
and of the split single-query attention.  Not a test module.  The reference functions run on whatever device their inputs
are on (the attention reference on the CPU; prefill_align_ref.py, the sibling module of test_prefill_align_parity_gpu.py, builds its
bounds from the constants and helpers here); with dtype == F64 nothing is rounded, which is the form
tests/test_fused_attn_ref_cpu.py checks against oracle/model.py.  The bounds are derived in test_kernel_parity_gpu.py's
module docstring."""
import torch

F32, F16, F64 = 0, 1, 2      # F64: references only (no rounding of intermediates)
C_DOT = 2.0 ** -20
# log-mel (tests/mel_ref.py): the fp32 spectrum X_k of a frame against float64 is within C_MEL * S_f, S_f = sum_j |x_j| w_j
# the absolute sum of the windowed frame.  The numpy float32 model of mel_kernel (mel_ref.emulate_fp32: both folds, the
# twiddle rotation re-read every 16 taps) was fitted at a peak of 2^-22.0 of S_f over twelve signal classes, all bins and
# frames: a margin of 4, which tests/test_mel_ref_cpu.py asserts as "the model stays at or below a quarter of the output
# bound" (it reaches 0.14).  Measured on |X| directly the restated model peaks at 2^-21.6, and at 2^-20.9 on the frames of
# the `click` class whose S_f is one tap (test_spectrum_error_of_the_model)
C_MEL = 2.0 ** -20
# attention: C_ATT * (sum p |v| / sum p).  The VALU forms keep p in fp32; the MFMA forms (beam-group diag / mfma, flash)
# round p to fp16 before the P.V product (2^-11 relative), and flash's unscaled form sums l from the fp32 p
C_ATT_VALU = 2.0 ** -20
C_ATT_MFMA = 2.0 ** -10
GUARD = 4096                 # guard bytes in front of and behind every buffer


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tdt(dtype):
    return {F16: torch.float16, F32: torch.float32, F64: torch.float64}[dtype]


class Buf:
    """A device buffer of `n` elements inside 0xFF guard bytes; `.t` is the payload view, `.raw` the whole allocation."""

    def __init__(self, n, tdt):
        es = torch.empty((), dtype=tdt).element_size()
        self.g = GUARD // es
        self.raw = torch.full((n + 2 * self.g,), 0, dtype=tdt, device=_dev())
        self.raw.view(torch.uint8).fill_(0xFF)
        self.t = self.raw[self.g:self.g + n]
        self.snap = None

    def ptr(self):
        return self.t.data_ptr()

    def snapshot(self):
        self.snap = self.raw.view(torch.uint8).clone()

    def changed(self):
        """byte mask (payload elements) of what differs from the snapshot; guard bytes must be untouched."""
        now = self.raw.view(torch.uint8)
        diff = now != self.snap
        es = self.raw.element_size()
        gb = self.g * es
        assert not diff[:gb].any() and not diff[len(diff) - gb:].any(), "write outside the allocation's payload"
        return diff[gb:len(diff) - gb].view(-1, es).any(1)


def _ulp(x, dtype):
    """ulp of |x| in the output type (x float64)."""
    a = x.abs().clamp_min(2.0 ** -14 if dtype == F16 else 2.0 ** -126)         # subnormals: the ulp of the smallest normal
    e = torch.floor(torch.log2(a))
    return torch.exp2(e - (10 if dtype == F16 else 23))


def _flip_slack(xd, X, delta, Wabs, dtype):
    """slack on y = X W^T for rows X = round(xd) the kernel computed with an fp32 error up to `delta` per element before
    rounding to the element type: an element within delta of a rounding boundary may round the other way (a whole ulp),
    every other one rounds identically; fp32 rows carry delta itself"""
    if dtype == F16:
        u = _ulp(xd, F16)
        near = ((xd - X).abs() - u / 2).abs() <= delta
        return (near * u + delta) @ Wabs.T
    return delta @ Wabs.T


def _merge_ref(o, m, l):
    """float64 merge of normalised partials o [S][..][64] with (m, l) [S][..]; returns (merged, merge error budget).
    The kernels weight split s by exp(m_s - M) in fp32: the argument's rounding is ~|m_s - M| 2^-24 relative"""
    md, ld, od = m.double(), l.double(), o.double()
    M = md.max(0).values
    w = torch.where(torch.isinf(md), torch.zeros_like(md), torch.exp(md - M)) * ld
    w = w / w.sum(0)
    x = (w.unsqueeze(-1) * od).sum(0)
    arg = torch.where(torch.isinf(md), torch.zeros_like(md), (md - M).abs())
    err = 2.0 ** -21 * (w.unsqueeze(-1) * (1.0 + arg.unsqueeze(-1)) * od.abs()).sum(0)
    return x, err


def _r(x, dtype):
    return x.to(_tdt(dtype)).double()


# ------------------------------------------------------------------------------------------ LayerNorm + projection
def ln_rows_ref(xd, lnw, lnb, dtype):
    """float64 LayerNorm (eps 1e-5) of the rows xd [R][K] with affine (lnw, lnb): (xn, X, delta, mu, var) — xn exact,
    X = xn rounded to the element type (what the kernel multiplies), delta the kernel's fp32 LayerNorm error on xn: one-pass
    mean of K values then a two-pass variance; it grows with |mean| / std (the mean's rounding shifts every centred value)"""
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    xn = (xd - mu) / torch.sqrt(var + 1e-5) * lnw.double() + lnb.double()
    X = _r(xn, dtype)
    delta = 2.0 ** -19 * (mu.abs() / torch.sqrt(var + 1e-5) + 1.0) * (xn.abs() + lnb.double().abs() + 1.0)
    return xn, X, delta, mu, var


def ln_gemv_ref(xv, W, bias, dtype, drop_last_block=False):
    """the LayerNorm-folded projection W . LN(x) + bias (affine folded into W / bias: LN without one) in float64 on the
    element-type-rounded normalised rows.  xv [R][K] fp32 values, W [N][K], bias [N] or None.  Returns (pre, slack, X):
    |y - pre| <= ulp_out(pre) + slack is the PRO_LN GEMV bound (C_DOT * sum |w x| + the rounding-flip slack of the rows).
    drop_last_block: the perturbed reference of the non-vacuity checks — the last 64-wide K block left out."""
    xd = xv.double()
    K = xd.shape[1]
    one, zero = torch.ones(K, device=xd.device), torch.zeros(K, device=xd.device)
    xn, X, delta, _, _ = ln_rows_ref(xd, one, zero, dtype)
    Wd = W.double()
    bd = bias.double().view(1, -1) if bias is not None else 0.0
    Kk = K - 64 if drop_last_block else K
    pre = X[:, :Kk] @ Wd[:, :Kk].T + bd
    sabs = X.abs() @ Wd.abs().T + (bd.abs() if bias is not None else 0.0)
    slack = C_DOT * sabs + (_flip_slack(xn, X, delta, Wd.abs(), dtype) if dtype != F64 else 0.0)
    return pre, slack, X


# ------------------------------------------------------------------------------------------------- attention
def split_chunk(T, splits, gran):
    """keys per split: ceil(T / splits) rounded up to the kernel form's key granule"""
    chunk = -(-T // splits)
    return -(-chunk // gran) * gran


def attn_ref(qs, kv, lens, splits, gran, dtype, H, peak=False, shift=None):
    """float64 single-query attention with a kernel's split boundaries and element-type partials.
    qs [R][H*64] float64: the SCALED queries as the kernel multiplies them; kv(r, h) -> (keys, values) float64 [>= lens[r]][64];
    lens[r] keys per row.  shift = (split index, keys): that split's lower boundary moved (a perturbed reference).
    Returns a dict of CPU float64 tensors:
      ref, pv, pe, pfl, pert [R][D] .. the merged output; sum p |v| / sum p; the same with every p weighted by 1 + |s - m|
                                       (fp32 scores: exp(s - m) carries ~|s - m| 2^-24 relative error from the argument); the
                                       rounding-flip slack of the partials; the reference with the last (peak: the dominant)
                                       key dropped
      po, ppv, ppe [S][R][D], pm, pl, pe_s [S][R][H] .. per split: the exact normalised partial (empty: 0), its two error
                                       weights, its maximum (empty: -inf), its sum of exp(s - m) (empty: 0),
                                       max_j sum_d |q_d k_jd| (the weight of a score's own fp32 error) and
                                       plw = sum_j p_j (1 + |s_j - m|) (the exp-argument weight of l)"""
    R, D = qs.shape
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    out = {k: z(R, D) for k in ("ref", "pv", "pe", "pfl", "pert")}
    out.update(po=z(splits, R, D), ppv=z(splits, R, D), ppe=z(splits, R, D), pl=z(splits, R, H), pe_s=z(splits, R, H),
               plw=z(splits, R, H),
               pm=torch.full((splits, R, H), float("-inf"), dtype=torch.float64))
    for r in range(R):
        T = lens[r]
        chunk = split_chunk(T, splits, gran)
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            kh, vh = kv(r, h)
            kh, vh = kh[:T], vh[:T]
            s = kh @ qs[r, sl]
            sa = kh.abs() @ qs[r, sl].abs()
            for drop_last in ((False, True) if T >= 2 else (False,)):
                ms, ls, os_, fl = [], [], [], []
                for sp in range(splits):
                    k0, k1 = sp * chunk, min(T, (sp + 1) * chunk)
                    if shift is not None and not drop_last:
                        if sp == shift[0]:
                            k0 = max(0, min(T, k0 + shift[1]))
                        if sp + 1 == shift[0]:
                            k1 = max(0, min(T, k1 + shift[1]))
                    if k1 <= k0:
                        continue
                    keep = torch.ones(k1 - k0, dtype=torch.bool)
                    if drop_last:       # the last key (peaked scores: the peak key, the only one that matters there)
                        j = int(s.argmax()) if peak else T - 1
                        if k0 <= j < k1:
                            keep[j - k0] = False
                    if not keep.any():
                        continue
                    ss = s[k0:k1][keep]
                    m = ss.max()
                    p = torch.exp(ss - m)
                    o = (p @ vh[k0:k1][keep]) / p.sum()
                    ms.append(m); ls.append(p.sum()); os_.append(_r(o, dtype) if splits > 1 else o)
                    # a partial within the kernel's fp32 error of a rounding boundary may round the other way
                    de = (p * (1.0 + (ss - m).abs())) @ vh[k0:k1][keep].abs() / p.sum() * 2.0 ** -20
                    u = _ulp(o, dtype)
                    fl.append((((o - os_[-1]).abs() - u / 2).abs() <= de) * u if splits > 1 and dtype != F64
                              else torch.zeros_like(o))
                    if not drop_last:
                        out["po"][sp, r, sl], out["pm"][sp, r, h], out["pl"][sp, r, h] = o, m, p.sum()
                        out["ppv"][sp, r, sl] = (p @ vh[k0:k1].abs()) / p.sum()
                        out["ppe"][sp, r, sl] = de * 2.0 ** 20
                        out["pe_s"][sp, r, h] = sa[k0:k1].max()
                        out["plw"][sp, r, h] = (p * (1.0 + (ss - m).abs())).sum()
                M = max(ms)
                w = torch.stack([torch.exp(m - M) * l for m, l in zip(ms, ls)])
                o = (w.unsqueeze(1) * torch.stack(os_)).sum(0) / w.sum()
                if not drop_last:
                    out["pfl"][r, sl] = (w.unsqueeze(1) * torch.stack(fl)).sum(0) / w.sum()
                if drop_last:
                    out["pert"][r, sl] = o
                else:
                    out["ref"][r, sl] = o
                    p = torch.exp(s - s.max())
                    out["pv"][r, sl] = (p @ vh.abs()) / p.sum()
                    out["pe"][r, sl] = (p * (1.0 + (s - s.max()).abs())) @ vh.abs() / p.sum()
    return out


def attn_bound(a, splits, c, dtype):
    """the attention bound on the merged output of attn_ref's result `a`: the output ulp, C_ATT * sum p |v| / sum p, the
    exp-argument term, and with splits the merge's own exp weights plus the partials' rounding flips"""
    bound = _ulp(a["ref"], dtype) + c * a["pv"] + 2.0 ** -21 * a["pe"]
    if splits > 1:                                                 # the split merge (merge_partials or in-launch)
        bound = bound + 2.0 ** -21 * a["pe"] + a["pfl"]
    return bound


# ------------------------------------------------------------------- the two attention blocks of one decode step
def cross_block_ref(xv, W, bias, keys, vals, Tk, splits, gran, dtype, H, qs=None, **kw):
    """`cross_attn_ln` + `cross_attn.query` + the single-query attention over Tk cached keys: q = W . LN(x) + bias rounded to
    the element type, times 0.125, then attn_ref.  keys / vals [R][>= Tk][H*64] float64 (CPU).  qs: the scaled queries to
    attend with instead (a kernel's own).  Returns (pre, slack, attn_ref's dict)."""
    pre, slack, _ = ln_gemv_ref(xv, W, bias, dtype)
    if qs is None:
        qs = _r(_r(pre, dtype) * 0.125, dtype)
    a = attn_ref(qs.cpu(), lambda r, h: (keys[r, :, h * 64:(h + 1) * 64], vals[r, :, h * 64:(h + 1) * 64]), [Tk] * xv.shape[0],
                 splits, gran, dtype, H, **kw)
    return pre, slack, a


def self_block_ref(xv, W, bias, kc, vc, pos, lags, dtype, H, qkv=None, **kw):
    """`attn_ln` + `attn.query / key / value` + the cache append + the single-query attention over the cache: qkv = W . LN(x)
    + bias ([R][3D], rounded to the element type), k and v of row r stored at cache position pos - lags[r], attention of
    q * 0.125 over positions [0, pos - lags[r]].  kc, vc [R][n_ctx][D] float64 CPU (not modified).  qkv: the rounded
    projection to go on with instead (a kernel's own).  Returns (pre, slack, kc', vc', lens, attn_ref's dict)."""
    R, D = xv.shape[0], W.shape[1]
    pre, slack, _ = ln_gemv_ref(xv, W, bias, dtype)
    if qkv is None:
        qkv = _r(pre, dtype)
    qkv = qkv.cpu()
    kc, vc = kc.clone(), vc.clone()
    lens = []
    for r in range(R):
        p = pos - (lags[r] if lags else 0)
        kc[r, p], vc[r, p] = qkv[r, D:2 * D], qkv[r, 2 * D:]
        lens.append(p + 1)
    qs = _r(qkv[:, :D] * 0.125, dtype)
    a = attn_ref(qs, lambda r, h: (kc[r, :, h * 64:(h + 1) * 64], vc[r, :, h * 64:(h + 1) * 64]), lens, 1, 64, dtype, H, **kw)
    return pre, slack, kc, vc, lens, a
