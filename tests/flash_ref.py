"""Score classes, the float64 reference and a plain fp32 emulation of attn_flash_f16_kernel (attention.hip), the only attention
kernel here that does not rescale on every tile: a lane's reference maximum moves only when some query of its 32-query wave
has outgrown it by more than 2^DEFER.  tests/test_flash_range_gpu.py checks the kernel against the reference over these
classes, tests/test_flash_ref_cpu.py checks the reference, the bound and the classes themselves without a GPU.  Not a test
module; a sibling of parity_ref.py and prefill_align_ref.py.  Everything runs on CPU tensors.

Scores are steered through one coordinate per head: q[:, 64 h] = a_t, k[:, 64 h] = b_j, the other 63 coordinates randn * 0.5
(a score noise of 0.25 natural), so the natural score is a_t b_j / 8 + noise with every steering value exact in fp16.  a = 8
unless the class says otherwise:

  normal ........ a = 0: unsteered scores, the control
  ramp .......... b_j = 8 (j // 64): every tile's maximum is 11.5 (exp2 domain) above the last: the rescale fires on every tile
  one_lane ...... b as ramp, a_t = 8 where t % 32 == 5, else -8: one query of a wave rises, 31 fall and ride through a firing
                  wave unmoved (delta = 0 / m_new = m_run)
  early_peak10,
  early_peak12 .. b_3 = 10 or 12, else 0: the reference stays at tile 0 and every later P is 2^-14.4 or 2^-17.3, an fp16
                  subnormal; those keys carry 6.8 % or 0.9 % of the mass at T = 1500
  late_peak ..... b_{T-1} = 30: the dominant key is the last valid key of the ragged tile: the mask and a rescale meet
  deep .......... b_j = -100: every score is -144 (exp2 domain): shift invariance and the first tile's factor
  deep_first .... b_j = -100 for j < 64, else 0: only the first tile is deep, a rescale follows the first tile's factor
  high .......... b_j = +100: cancellation in sacc - delta and in fma(s, c, -m)
  equal ......... every row of k equals k[0]: every output is the plain mean of v

All scores stay within |s| <= 190 natural, where the fp32 rounding of a score (2^-24 |s|) is below 2^-15 relative in p: far
inside C_ATT_MFMA.  Beyond that range the bound would need that term.
"""
import math

import numpy as np
import torch

from parity_ref import _tdt

CLASSES = ("normal", "ramp", "one_lane", "early_peak10", "early_peak12", "late_peak", "deep", "deep_first", "high", "equal")
PEAK_CLASSES = ("early_peak10", "early_peak12", "late_peak")     # one key dominates: the perturbation that counts drops it
# attn_generic_kernel (fp32 vector ALU, bound C_ATT_VALU = 2^-20) is run over the classes whose fp32 emulations — both
# prefill_align_ref.generic_attn_emulate and generic_emulate_serial below — stay inside generic_attn_bound in both element
# types at (Tk, Tq) = (200, 33).  Left out, with the largest error / bound of the emulations over three seeds, half / float:
#   ramp 2.88 / 5.00, one_lane 0.50 / 2.83, deep 1.91 / 4.00, high 1.91 / 3.55: the bound has a term for |s - m| but none
#     for the fp32 rounding of the score itself, 2^-24 |s| before the 0.125, at |s| of 24 to 100 on keys that carry weight;
#   early_peak12 0.50 / 1.16 (serial; 0.65 as matrix products): the dominant key is the fourth term of the serial P.V chain
#     and the 196 that follow are each rounded at its ulp, a random walk of which C_ATT_VALU * pv is about 3.3 standard
#     deviations, over 8448 outputs.  early_peak10 reaches 0.98 the same way and stays.
GENERIC_CLASSES = ("normal", "early_peak10", "late_peak", "deep_first", "equal")
DEFER = 6.0
PRESCALE = math.sqrt(0.125 * math.log2(math.e))                  # on q and on k: q.k is then the exp2 argument
NEG_INF = float("-inf")


def drop_kind(cls):
    """the perturbed reference a class is held against: its dominant key dropped, or the last key"""
    return "dominant" if cls in PEAK_CLASSES else "last"


def flash_inputs(cls, T, Tq, H, seed, prescaled):
    """fp16 q [Tq][H*64], k, v [T][H*64] of one batch entry for a score class (module docstring).  prescaled: q and k are
    multiplied by sqrt(0.125 log2 e) and rounded to fp16 again; the reference is computed from the rounded tensors."""
    assert cls in CLASSES, cls
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Tq, H * 64, generator=g) * 0.5
    k = torch.randn(T, H * 64, generator=g) * 0.5
    v = torch.randn(T, H * 64, generator=g)
    a = torch.full((Tq,), 0.0 if cls == "normal" else 8.0)
    b = torch.zeros(T)
    if cls in ("ramp", "one_lane"):
        b = 8.0 * (torch.arange(T) // 64).float()
    if cls == "one_lane":
        a = torch.where(torch.arange(Tq) % 32 == 5, 8.0, -8.0)
    if cls.startswith("early_peak"):
        b[3] = float(cls[len("early_peak"):])
    if cls == "late_peak":
        b[T - 1] = 30.0
    if cls == "deep":
        b[:] = -100.0
    if cls == "deep_first":
        b[:64] = -100.0
    if cls == "high":
        b[:] = 100.0
    for h in range(H):
        q[:, 64 * h] = a
        k[:, 64 * h] = b
    if cls == "equal":
        k = k[:1].expand(T, -1).clone()
    q, k, v = q.half(), k.half(), v.half()
    if prescaled:
        q, k = (q.float() * PRESCALE).half(), (k.float() * PRESCALE).half()
    return q, k, v


def flash_ref(q, k, v, H, prescaled, drop=None):
    """float64 softmax(q.k * 0.125) v per head (prescaled: softmax of 2^(q.k)).  Returns (ref, pv, sv) [Tq][H*64]:
    pv = sum p |v| / sum p, sv = sum_j |v_j| / L with L = sum_j e^(s_j - max) — the weight of an error that is absolute in P.
    drop = "dominant": every query loses its arg-max key; drop = "last": the last key is left out (perturbed references)."""
    qd, kd, vd = q.double(), k.double(), v.double()
    if drop == "last":
        kd, vd = kd[:-1], vd[:-1]
    c = math.log(2.0) if prescaled else 0.125
    ref = torch.zeros(q.shape[0], H * 64, dtype=torch.float64)
    pv, sv = torch.zeros_like(ref), torch.zeros_like(ref)
    for h in range(H):
        sl = slice(h * 64, h * 64 + 64)
        s = (qd[:, sl] @ kd[:, sl].T) * c
        if drop == "dominant":
            s = s.scatter(1, s.argmax(1, keepdim=True), NEG_INF)
        e = torch.exp(s - s.max(1, keepdim=True).values)
        L = e.sum(1, keepdim=True)
        ref[:, sl] = (e @ vd[:, sl]) / L
        pv[:, sl] = (e @ vd[:, sl].abs()) / L
        sv[:, sl] = vd[:, sl].abs().sum(0, keepdim=True) / L
    return ref, pv, sv


def _fma32(a, b, c):
    """fp32 fma of numpy arrays: the product of two fp32 values and the sum are exact enough in float64 for one rounding"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def generic_emulate_serial(q, k, v, H, dtype):
    """attn_generic_kernel over all keys (non-causal) with its two dot products as the serial fma chains they are, which
    prefill_align_ref.generic_attn_emulate states as matrix products: s = fma over d = 0 .. 63 (the steering coordinate
    first), acc = o * alpha, then fma over the 64 keys of the tile in order, __expf as exp2 of a rounded product.  The order
    matters where one early term dominates: every later addition is rounded at that term's ulp."""
    q, k, v = q.float().numpy(), k.float().numpy(), v.float().numpy()
    Tq, Tk = q.shape[0], k.shape[0]
    log2e = np.float32(1.4426950408889634)
    expf = lambda x: np.exp2((x * log2e).astype(np.float32).astype(np.float64)).astype(np.float32)       # noqa: E731
    out = np.zeros((Tq, H * 64), np.float32)
    with np.errstate(invalid="ignore"):
        for h in range(H):
            qh, kh, vh = (x[:, h * 64:h * 64 + 64] for x in (q, k, v))
            m, l, o = np.full(Tq, -np.inf, np.float32), np.zeros(Tq, np.float32), np.zeros((Tq, 64), np.float32)
            for k0 in range(0, Tk, 64):
                k1 = min(Tk, k0 + 64)
                s = np.zeros((Tq, k1 - k0), np.float32)
                for d in range(64):
                    s = _fma32(qh[:, d:d + 1], kh[None, k0:k1, d], s)
                s = s * np.float32(0.125)
                mn = np.maximum(m, s.max(1))
                alpha = np.where(np.isinf(m), np.float32(0), expf(m - mn))
                p = expf(s - mn[:, None])
                l = l * alpha + p.sum(1, dtype=np.float64).astype(np.float32)
                o = o * alpha[:, None]
                for j in range(k1 - k0):
                    o = _fma32(p[:, j:j + 1], vh[None, k0 + j], o)
                m = mn
            out[:, h * 64:h * 64 + 64] = o / l[:, None]
    return torch.from_numpy(out).to(_tdt(dtype))


def flash_emulate(q, k, v, H, prescaled, first_alpha_exp2=False, p_stats=None):
    """attn_flash_f16_kernel's order of operations in fp32: 64-key tiles, 32-query waves (the last one padded with copies of
    row Tq - 1, as the kernel clamps its query row), the wave-uniform deferral as written, P rounded to fp16 before P.V, l from
    the fp16 P (prescaled) or from the fp32 p (unscaled), o * (1 / l) rounded to fp16.  The keys past T of the ragged tile are
    left out, which is what their -inf scores amount to (p = 0, no part in the maximum).

    Returns (out fp16 [Tq][H*64], fires, unmoved): the (head, wave, tile) rescales after tile 0, and the lanes of real queries
    inside those firing waves whose own reference did not move.
    first_alpha_exp2: the prescaled first tile scales the (still empty) accumulators by exp2(-mx) instead of
    exp2(-max(mx, 0)), as the kernel did before: inf where mx < -128, and 0 * inf = NaN from then on.
    p_stats: a dict that receives "total" and "subnormal", the number of P entries of real queries and how many of them are
    nonzero and below the smallest normal fp16 (2^-14)."""
    Tq, T = q.shape[0], k.shape[0]
    W = (Tq + 31) // 32
    rows = torch.arange(W * 32).clamp_max(Tq - 1)
    real = (torch.arange(W * 32) < Tq).view(1, W, 32)
    q32 = q.float()[rows].view(W * 32, H, 64).transpose(0, 1)            # [H][W * 32][64]
    k32 = k.float().view(T, H, 64).transpose(0, 1)
    v32 = v.float().view(T, H, 64).transpose(0, 1)
    c = torch.tensor(1.4426950408889634, dtype=torch.float32) * 0.125    # SCALE_LOG2E
    o = torch.zeros(H, W * 32, 64)
    l = torch.zeros(H, W * 32)
    m = torch.zeros(H, W * 32) if prescaled else torch.full((H, W * 32), NEG_INF)
    fires = unmoved = total = subnormal = 0

    def per_wave(x):         # a per-wave flag [H][W] as a per-lane one [H][W * 32]
        return x.unsqueeze(-1).expand(H, W, 32).reshape(H, W * 32)

    for kt in range((T + 63) // 64):
        k0, k1 = kt * 64, min(T, kt * 64 + 64)
        s = q32 @ k32[:, k0:k1].transpose(1, 2)                          # [H][W * 32][keys]
        if prescaled:
            s = s - m.unsqueeze(-1)                                      # the accumulators start at -m_run
            mx = s.max(-1).values
            fw = (mx.view(H, W, 32) > DEFER).any(-1) | (kt == 0)
            delta = torch.where(per_wave(fw), mx if kt == 0 else mx.clamp_min(0.0), torch.zeros_like(mx))
            alpha = torch.exp2(-delta if first_alpha_exp2 else -delta.clamp_min(0.0))
            s = s - delta.unsqueeze(-1)
            still = delta == 0
            m = m + delta
            p16 = torch.exp2(s).half()
            l = l * alpha + p16.float().sum(-1)
        else:
            mxs = s.max(-1).values * c
            fw = (mxs > m + DEFER).view(H, W, 32).any(-1)
            m_new = torch.where(per_wave(fw), torch.maximum(m, mxs), m)
            alpha = torch.exp2(m - m_new)                                # 0 on the first tile (m = -inf)
            still = m_new == m
            m = m_new
            p = torch.exp2((s.double() * c.double() - m.double().unsqueeze(-1)).float())      # one rounding: the fma
            l = l * alpha + p.sum(-1)
            p16 = p.half()
        o = o * alpha.unsqueeze(-1) + p16.float() @ v32[:, k0:k1]
        if kt > 0:
            fires += int(fw.sum())
            unmoved += int((fw.unsqueeze(-1) & still.view(H, W, 32) & real).sum())
        pr = p16.view(H, W, 32, -1)[real.expand(H, W, 32)]
        total += pr.numel()
        subnormal += int(((pr > 0) & (pr.float() < 2.0 ** -14)).sum())
    if p_stats is not None:
        p_stats.update(total=total, subnormal=subnormal)
    out = (o * (1.0 / l).unsqueeze(-1)).half()
    return out.transpose(0, 1).reshape(W * 32, H * 64)[:Tq], fires, unmoved
