"""Float64 references, per-element bounds, named perturbations and plain fp32 emulations of the prefill, word-timestamp,
alignment, encoder-stem and small kernels (tests/test_prefill_align_parity_gpu.py checks the kernels against them,
tests/test_prefill_align_ref_cpu.py checks the references and bounds themselves without a GPU).  Not a test module; a
sibling of parity_ref.py, whose constants (C_DOT, C_ATT_VALU) and helpers (_ulp, attn_bound) every bound here is built from.
Everything runs on CPU tensors.

The only constants that do not come from parity_ref.py are those of the alignment stage-(a) bound (align_stage_a) and of the
no_speech bound (no_speech_ref).  Both are sums of fp32 rounding steps counted off the kernels, in units of U = 2^-24:
  one fp32 multiply, add, subtract, divide or sqrt .......... U relative (round to nearest)
  expf(a) ................................................... 2 U relative (one ulp), plus the error of its argument a:
                                                              a rounded subtraction x - m carries U |x - m| into the exponent
  a sum of n non-negative fp32 terms, depth d ............... d U relative (gamma_d)
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

from parity_ref import C_ATT_VALU, C_DOT, F16, F32, _tdt, _ulp, attn_bound

U = 2.0 ** -24
NEG_INF = float("-inf")


def ratio(got, ref, bound):
    """largest |got - ref| / bound (NaN if anything is NaN)"""
    r = (got.double() - ref).abs() / bound
    return float("nan") if torch.isnan(r).any() else r.max().item()


# ------------------------------------------------------------------------------------------- generic attention
def generic_attn_ref(q, k, v, H, limit, drop_last=False):
    """float64 attention of the queries q [Tq][H*64] over the keys k, v [>= max limit][H*64] of their audio, scores
    q.k * 0.125, query t seeing keys [0, limit[t]) (limit: LongTensor [Tq]; causal with a cache of d_len: d_len + t + 1).
    drop_last: every query with two keys or more loses its last one (a perturbed reference).
    Returns attn_bound's dict: ref, pv = sum p |v| / sum p, pe = the same with p weighted by 1 + |s - m|."""
    n = int(limit.max())
    k, v = k[:n], v[:n]
    lim = torch.where(limit >= 2, limit - 1, limit) if drop_last else limit
    vis = torch.arange(n).view(1, -1) < lim.view(-1, 1)
    out = {key: torch.zeros_like(q) for key in ("ref", "pv", "pe")}
    for h in range(H):
        sl = slice(h * 64, h * 64 + 64)
        s = ((q[:, sl] @ k[:, sl].T) * 0.125).masked_fill(~vis, NEG_INF)
        m = s.max(1, keepdim=True).values
        p = torch.exp(s - m)
        p = p / p.sum(1, keepdim=True)
        dist = torch.where(vis, (s - m).abs(), torch.zeros_like(s))
        out["ref"][:, sl] = p @ v[:, sl]
        out["pv"][:, sl] = p @ v[:, sl].abs()
        out["pe"][:, sl] = (p * (1.0 + dist)) @ v[:, sl].abs()
    return out


def generic_attn_bound(a, dtype):
    """attn_generic_kernel is all fp32 vector ALU with one split: ulp_out + C_ATT_VALU sum p |v| / sum p, plus parity_ref's
    exp-argument term 2^-21 sum p (1 + |s - m|) |v| / sum p — the kernel's __expf(s - m) is exp2 of a rounded product, so its
    relative error grows with |s - m| (the same term every decode-attention form carries in attn_bound)."""
    return attn_bound(a, 1, C_ATT_VALU, dtype)


def generic_attn_emulate(q, k, v, H, limit, dtype):
    """attn_generic_kernel's order of operations in fp32: 64-key tiles, scores scaled after the dot product, online
    softmax with the running maximum (a tile that is fully masked for a query leaves its state alone), o / l at the end,
    one rounding to the element type"""
    q32, k32, v32 = q.float(), k.float(), v.float()
    Tq, n = q.shape[0], int(limit.max())
    out = torch.zeros(Tq, H * 64)
    for h in range(H):
        sl = slice(h * 64, h * 64 + 64)
        m = torch.full((Tq,), NEG_INF)
        l = torch.zeros(Tq)
        o = torch.zeros(Tq, 64)
        for k0 in range(0, n, 64):
            k1 = min(n, k0 + 64)
            s = (q32[:, sl] @ k32[k0:k1, sl].T) * 0.125
            vis = torch.arange(k0, k1).view(1, -1) < limit.view(-1, 1)
            s = s.masked_fill(~vis, NEG_INF)
            mn = torch.maximum(m, s.max(1).values)
            dead = mn == NEG_INF
            alpha = torch.where(dead, torch.ones_like(mn), torch.exp(m - torch.where(dead, torch.zeros_like(mn), mn)))
            p = torch.where(vis, torch.exp(s - torch.where(dead, torch.zeros_like(mn), mn).view(-1, 1)), torch.zeros_like(s))
            l = l * alpha + p.sum(1)
            o = o * alpha.view(-1, 1) + p @ v32[k0:k1, sl]
            m = mn
        out[:, sl] = o / l.view(-1, 1)
    return out.to(_tdt(dtype))


# ---------------------------------------------------------------------------------------------------- cross QK
def cross_qk_ref(q, k, drop_last_d=False):
    """float64 score plane q [T][64] . k [Tk][64] * 0.125 and its bound ulp_f32 + C_DOT * 0.125 * sum |q_d k_d| (fp32
    accumulation of 64 products on the vector ALU or, fp16, on the matrix cores; fp32 output)"""
    d = 63 if drop_last_d else 64
    ref = (q[:, :d] @ k[:, :d].T) * 0.125
    bound = _ulp(ref, F32) + C_DOT * 0.125 * (q.abs() @ k.abs().T)
    return ref, bound


def cross_qk_emulate(q, k):
    return ((q.float() @ k.float().T) * 0.125).float()


# --------------------------------------------------------------------------------------------------- alignment
def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _window(F, width, shift=0):
    """[F][width] source indices of the sliding window (reflect padding), optionally shifted (a perturbation)"""
    return _reflect(np.arange(F)[:, None] - width // 2 + shift + np.arange(width)[None, :], F)


def median_f64(x, width, shift=0):
    """sliding median of odd `width` along the last axis with reflect padding in the array's own precision; a row no
    longer than width // 2 is returned unchanged (align_median_kernel, oracle.timing.median_filter)"""
    F = x.shape[-1]
    if F <= width // 2:
        return x
    return np.sort(x[..., _window(F, width, shift)], -1)[..., width // 2]


def window_max(b, width):
    """max of a per-element error bound over each median window: |median(x + e) - median(x)| <= max |e| over the window"""
    F = b.shape[-1]
    if F <= width // 2:
        return b
    return b[..., _window(F, width)].max(-1)


def align_stage_a(qk, T, F, scale, soft_frames=None, unbiased=False):
    """float64 softmax over the first F frames of qk [H][>= T][>= F] * scale, then the z-norm of every (head, frame) column
    over the T tokens with the biased std; returns (z, bound) [H][T][F].  soft_frames / unbiased: perturbed references
    (softmax over F + 1 frames; the unbiased std).

    Bound, per element, from align_softmax_kernel and align_znorm_kernel (U = 2^-24):
      x = qk * scale (U |x| into the exponent), e = expf(x - m) (U |x - m| from the subtraction, 2 U for expf, and U for the
      stored e): a_j = |x_j| + |x_j - m| + 3.  The sum s of F such terms has depth D_F = ceil(F / 256) + 6 + 2 (a thread's
      serial part, 6 shuffle levels, 4 waves) and inherits the p-weighted mean of the a_j; the division adds U:
          rel(w_j) = U (a_j + sum_j' p_j' a_j' + D_F + 1)                         dw = rel(w) w
      mean over T tokens, summed serially (gamma_T) and divided (U):   dmean = mean_t dw + (T + 1) U mean
      d = w - mean: the cancellation — dd = dw + dmean + U |d|, which relative to the result is (|w| + |mean|) / sd
      var = sum d^2 (fma chain, gamma_T) / T, sd = sqrt(var / T):   rel(sd) = sum_t |d_t| dd_t / (T sd^2) + (T / 2 + 2) U
      z = d / sd:   bound = dd / sd + |z| (rel(sd) + U)"""
    Fs = soft_frames or F
    x = qk[:, :T, :Fs].double() * scale
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    pf = e / e.sum(-1, keepdim=True)
    p = pf[..., :F]
    mean = p.mean(1, keepdim=True)
    d = p - mean
    var = (d * d).sum(1, keepdim=True) / T
    sd = torch.sqrt(var * T / (T - 1)) if unbiased else torch.sqrt(var)
    z = d / sd
    a = x.abs() + (x - m).abs() + 3.0
    depth_f = math.ceil(F / 256) + 6 + 2
    dw = (U * (a + (pf * a).sum(-1, keepdim=True) + depth_f + 1.0))[..., :F] * p
    dmean = dw.mean(1, keepdim=True) + (T + 1) * U * mean
    dd = dw + dmean + U * d.abs()
    rel_sd = (d.abs() * dd).sum(1, keepdim=True) / (T * var) + (T / 2 + 2) * U
    return z, dd / torch.sqrt(var) + z.abs() * (rel_sd + U)


def head_mean_ref(w1, T, row_begin, row_tail):
    """float64 -mean over heads of rows [row_begin, T - row_tail) of w1 [H][T][F] and the bound of align_head_mean_kernel on
    it: ulp_f32 + H 2^-24 sum_h |w1| (a serial H-term sum and a division)"""
    H = w1.shape[0]
    rows = w1[:, row_begin:T - row_tail].double()
    cost = -rows.mean(0)
    return cost, _ulp(cost, F32) + H * U * rows.abs().sum(0)


def align_chain_ref(qk, T, F, scale, width, row_begin, row_tail, shift=0, **kw):
    """the whole float64 chain of one clip: (w0, b0, w1, b1, cost, bcost) with the stage-(a) bound carried through the
    median (window_max) and the head mean; shift: the median window moved (a perturbed reference)"""
    w0, b0 = align_stage_a(qk, T, F, scale, **kw)
    w1 = torch.from_numpy(median_f64(w0.numpy(), width, shift))
    b1 = torch.from_numpy(window_max(b0.numpy(), width))
    cost, bc = head_mean_ref(w1, T, row_begin, row_tail)
    return w0, b0, w1, b1, cost, bc + b1[:, row_begin:T - row_tail].mean(0)


def align_emulate(qk, T, F, scale, width, row_begin, row_tail):
    """the four kernels in fp32 in their order of operations (token and head sums serial); the median through
    oracle.timing.median_filter.  Returns (w0, w1, cost) float32"""
    from oracle.timing import median_filter
    x = qk[:, :T, :F].float() * torch.tensor(scale, dtype=torch.float32)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    w = e / e.sum(-1, keepdim=True)
    mean = torch.zeros_like(w[:, 0])
    for t in range(T):
        mean = mean + w[:, t]
    mean = mean / torch.tensor(float(T))
    var = torch.zeros_like(mean)
    for t in range(T):
        var = var + (w[:, t] - mean) ** 2
    sd = torch.sqrt(var / torch.tensor(float(T)))
    w0 = (w - mean.unsqueeze(1)) / sd.unsqueeze(1)
    w1 = torch.from_numpy(median_filter(w0.numpy(), width).copy())
    s = torch.zeros_like(w1[0, row_begin:T - row_tail])
    for h in range(w1.shape[0]):
        s = s + w1[h, row_begin:T - row_tail]
    return w0, w1, -(s / torch.tensor(float(w1.shape[0])))


# ------------------------------------------------------------------------------------------------ encoder stem
def conv_gelu_ref(x, w, b, stride, odt, flip=False, offset=0, pos=None):
    """float64 gelu(conv1d(x, w, b, stride, padding=1)) (+ pos) of the rows x [B][F][C] (w [D][C][3], b [D]) as [B][T][D],
    with test_kernel_parity_gpu's GEMM bound including its GELU term: ulp_out + 1.13 C_DOT sum |a w| + 4.2e-7 + 2^-22 |pre|.
    flip: the three taps in reverse order; offset: the input rows moved down by `offset` (perturbed references)."""
    xi = x.double().transpose(1, 2)
    if offset:
        xi = Fn.pad(xi, (offset, 0))[..., :xi.shape[-1]]
    wd, bd = (w.flip(-1) if flip else w).double(), b.double()
    pre = Fn.conv1d(xi, wd, bd, stride=stride, padding=1).transpose(1, 2)
    sabs = Fn.conv1d(xi.abs(), wd.abs(), bd.abs(), stride=stride, padding=1).transpose(1, 2)
    ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    slack = 1.13 * C_DOT * sabs + 4.2e-7 + 2.0 ** -22 * pre.abs()
    if pos is not None:
        ref = ref + pos.double()
    return ref, _ulp(ref, odt) + slack


def conv_gelu_emulate(x, w, b, stride, out_tdt, pos=None):
    """fp32 accumulation of the element-type inputs, fp32 GELU (+ pos), one rounding to the output type"""
    y = Fn.gelu(Fn.conv1d(x.float().transpose(1, 2), w.float(), b.float(), stride=stride, padding=1).transpose(1, 2))
    if pos is not None:
        y = y + pos.float()
    return y.to(out_tdt)


# --------------------------------------------------------------------------------------------------- no_speech
def no_speech_ref(x, ns, drop_last=False):
    """float64 softmax(x [R][V])[:, ns] and its bound.  drop_last: the last logit left out (a perturbed reference).

    Bound from no_speech_kernel (U = 2^-24): a thread folds n_t = ceil(V / 1024) logits into (m, s), one expf (2 U), one
    multiply and one add per step; six shuffle levels and the 16-term sum of the first thread follow, each step again at
    most 4 U: 4 (n_t + 6 + 16) U.  Every expf argument is a rounded difference, and the rescales a term goes through
    telescope to x_j - M: 2 U sum_j p_j |x_j - M|.  The numerator expf(x_ns - M) adds U |x_ns - M| + 2 U, the division U:
        |out - ref| <= ulp_f32(ref) + ref U (4 (n_t + 22) + 2 sum_j p_j |x_j - M| + |x_ns - M| + 3)"""
    x = x.double()
    V = x.shape[1]
    xx = x[:, :V - 1] if drop_last else x
    M = xx.max(1, keepdim=True).values
    e = torch.exp(xx - M)
    S = e.sum(1, keepdim=True)
    p = e / S
    dist = torch.where(torch.isinf(xx), torch.zeros_like(xx), (xx - M).abs())
    ref = (torch.exp(x[:, ns:ns + 1] - M) / S).squeeze(1)
    n_t = math.ceil(V / 1024)
    rel = U * (4.0 * (n_t + 22) + 2.0 * (p * dist).sum(1) + (x[:, ns] - M.squeeze(1)).abs() + 3.0)
    return ref, _ulp(ref, F32) + ref * rel


def no_speech_emulate(x, ns, guard_inf=True):
    """no_speech_kernel's recurrence in fp32 (numpy): 1024 threads, strided logits, the wave butterfly, the 16-wave merge.
    guard_inf=False: the recurrence as it was before a -inf logit was skipped while the running maximum is still -inf"""
    x = x.float().numpy()
    R, V = x.shape
    out = np.zeros(R, dtype=np.float32)
    tid = np.arange(1024)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            m = np.full(1024, -np.inf, dtype=np.float32)
            s = np.zeros(1024, dtype=np.float32)
            for v0 in range(0, V, 1024):
                idx = v0 + tid
                valid = idx < V
                xv = x[r, np.minimum(idx, V - 1)]
                up = valid & (xv > m)
                add = valid & ~up & ((xv != -np.inf) if guard_inf else True)
                s_up = (s * np.exp(m - xv) + np.float32(1.0)).astype(np.float32)
                s_add = (s + np.exp(xv - m)).astype(np.float32)
                s = np.where(up, s_up, np.where(add, s_add, s))
                m = np.where(up, xv, m)
            o = 32
            while o:
                m2, s2 = m[tid ^ o], s[tid ^ o]
                mn = np.maximum(m, m2)
                s = np.where(mn == -np.inf, np.float32(0), s * np.exp(m - mn) + s2 * np.exp(m2 - mn)).astype(np.float32)
                m = mn
                o >>= 1
            wm, ws = m[::64], s[::64]
            Mx = wm.max()
            S = np.float32(0)
            for w in range(16):
                S = np.float32(S + (np.float32(0) if wm[w] == -np.inf else ws[w] * np.exp(wm[w] - Mx)))
            out[r] = np.exp(x[r, ns] - Mx) / S
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------- inputs
def attn_inputs(dtype, R, audios, Tq, n_keys, H, seed):
    """q [R][Tq][H*64], k, v [audios][n_keys][H*64] in the element type (values exactly representable there), CPU"""
    g = torch.Generator().manual_seed(seed)
    tdt = _tdt(dtype)
    return (torch.randn(R, Tq, H * 64, generator=g).to(tdt), torch.randn(audios, n_keys, H * 64, generator=g).to(tdt),
            torch.randn(audios, n_keys, H * 64, generator=g).to(tdt))


def align_inputs(clips, H, Tmax, Tk, seed):
    """qk [clips][H][Tmax][Tk] fp32 with a standard deviation of 2"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(clips, H, Tmax, Tk, generator=g) * 2.0).float()


def no_speech_inputs(V, seed):
    """three rows of V logits: plain (the last logit raised so that it carries visible mass), some -inf entries (among
    them the first ones a thread meets), one logit 80 above the rest; and the index asked for"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, V, generator=g).float() * 2.0
    x[0, V - 1] = 6.0
    ns = V // 2
    if V > 1:
        x[1, :min(V, 1500):3] = NEG_INF
        x[1, V - 1] = NEG_INF
        x[1, ns] = 0.5
        x[2, ns] = x[2].max()                   # the answer is e^-80: still a normal fp32 number
        x[2, (ns + 1) % V] = x[2, ns] + 80.0
    return x, ns


def stem_inputs(n_mels, D, F, B, dtype, seed):
    """mel [B][n_mels][F] fp32, conv1 w [D][n_mels][3] / b, conv2 w [D][D][3] / b, pos [F / 2][D]; weights in the element type"""
    g = torch.Generator().manual_seed(seed)
    tdt = _tdt(dtype)
    mel = torch.randn(B, n_mels, F, generator=g).float()
    w1 = (torch.randn(D, n_mels, 3, generator=g) * (3 * n_mels) ** -0.5).to(tdt)
    b1 = (torch.randn(D, generator=g) * 0.5).float()
    w2 = (torch.randn(D, D, 3, generator=g) * (3 * D) ** -0.5).to(tdt)
    b2 = (torch.randn(D, generator=g) * 0.5).float()
    pos = torch.randn(F // 2, D, generator=g).float()
    return mel, w1, b1, w2, b2, pos
