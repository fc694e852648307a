"""LayerNorm behind the MFMAs (whisper_amd/csrc/kernels.h), on the CPU: the algebra in float64, and the error bound of
tests/ln_post_ref.py held against an emulation of the kernel's arithmetic (fp16 operands, fp32 sums).  The bound is derived in
ln_post_ref.py's docstring; tests/test_ln_post_gpu.py holds the kernels to the same function.

What is shown here:
  * in float64, without rounding, the formula equals the LayerNorm projection for any centre;
  * with the centre within one standard deviation of the row mean the emulated result meets the bound at row mean / std of
    0, 3 and 30, for random weights and for a weight row aligned with the rounding errors (the worst case of the leading term);
  * the bound is not vacuous: two rows swapped, or the last k-term dropped, break it;
  * the centring is needed: with c = 0 at mean / std = 30 the aligned weight row misses the bound.
"""
import pytest
import torch

from ln_post_ref import centred_fp16, ln_post_bound, ln_post_emulate, ln_true

SHAPES = [(40, 64), (24, 320), (72, 1280)]
RATIOS = [0.0, 3.0, 30.0]          # row mean / std
R = 9


def _rows(K, ratio, std, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, K, generator=g, dtype=torch.float64) * std
    x = x - x.mean(1, keepdim=True) + ratio * x.std(1, unbiased=False, keepdim=True)
    return x.float()


def _weights(N, K, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(N, K, generator=g) * K ** -0.5).half(), (torch.randn(N, generator=g) * 0.5).float()


def _ratio(x32, c32, W16, b32):
    xd, Wd, bd = x32.double(), W16.double(), b32.double()
    pre, mu, var = ln_true(xd, Wd, bd)
    bound = ln_post_bound(xd, Wd, bd, pre, mu, var)
    y, _ = ln_post_emulate(centred_fp16(x32, c32), W16, b32)
    assert torch.isfinite(y).all()
    return ((y.double() - pre).abs() / bound).max().item(), pre, bound


def _aligned(x32, c32, W16, row=0):
    """W with row 0 replaced by |w| sign(rounding error of x[row] - c[row]): every term of sum_k W_k e_k has one sign"""
    xc = x32.double()[row] - c32.double()[row]
    e = centred_fp16(x32, c32)[row].double() - xc
    W = W16.clone()
    W[0] = (W16[0].abs().float() * torch.sign(e).float()).half()
    return W


def test_formula_is_layernorm_in_float64():
    for (N, K) in SHAPES:
        x = _rows(K, 3.0, 1.0, 1).double()
        W16, b = _weights(N, K, 1)
        Wd, bd = W16.double(), b.double()
        pre, _, _ = ln_true(x, Wd, bd)
        for c in (0.0, 2.5, -7.0):
            xc = x - c
            m = xc.mean(1, keepdim=True)
            v = (xc * xc).mean(1, keepdim=True) - m * m
            y = bd.view(1, -1) + torch.rsqrt(v + 1e-5) * (xc @ Wd.T - m * Wd.sum(1).view(1, -1))
            assert (y - pre).abs().max().item() < 1e-9


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("std", [1.0, 0.03, 40.0])
def test_bound_holds_with_admissible_centre(ratio, std):
    worst = 0.0
    for si, (N, K) in enumerate(SHAPES):
        x = _rows(K, ratio, std, 10 * si + 3)
        W16, b = _weights(N, K, si)
        mu = x.double().mean(1)
        sig = x.double().std(1, unbiased=False)
        for u in (-1.0, -0.5, 0.0, 0.7, 1.0):
            c = (mu + u * sig).float()
            # never outside the contract through the fp32 rounding of c itself
            c = torch.where((c.double() - mu).abs() > sig, mu.float(), c)
            r, _, _ = _ratio(x, c, W16, b)
            ra, _, _ = _ratio(x, c, _aligned(x, c, W16), b)
            worst = max(worst, r, ra)
            assert r <= 1.0 and ra <= 1.0, f"N={N} K={K} mean/std={ratio} std={std} c=mu{u:+}sig: error / bound {r:.3f} / {ra:.3f}"
    print(f"mean/std={ratio} std={std}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("ratio", RATIOS)
def test_bound_is_not_vacuous(ratio):
    for si, (N, K) in enumerate(SHAPES):
        x = _rows(K, ratio, 1.0, 10 * si + 5)
        W16, b = _weights(N, K, si)
        c = x.double().mean(1).float()
        _, pre, bound = _ratio(x, c, W16, b)
        swapped = pre[[1, 0] + list(range(2, R))]
        assert ((swapped - pre).abs() / bound).max().item() > 1.0, "two rows swapped pass the bound"
        xd = x.double()
        mu = xd.mean(1, keepdim=True)
        xn = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + 1e-5)
        drop = xn[:, K - 1:K] * W16.double()[:, K - 1].view(1, -1)
        assert (drop.abs() / bound).max().item() > 1.0, "the last k-term dropped passes the bound"


def test_uncentred_rows_miss_the_bound():
    """c = 0 at mean / std = 30: the rows are rounded to fp16 at 30 std, the aligned weight row collects the errors"""
    for si, (N, K) in enumerate(SHAPES):
        x = _rows(K, 30.0, 1.0, 10 * si + 7)
        W16, b = _weights(N, K, si)
        zero = torch.zeros(R)
        r, _, _ = _ratio(x, zero, _aligned(x, zero, W16), b)
        assert r > 1.0, f"N={N} K={K}: c = 0 at mean/std = 30 meets the bound ({r:.3f}) — the bound would not need the centring"
        c = x.double().mean(1).float()
        rc, _, _ = _ratio(x, c, _aligned(x, c, W16), b)
        assert rc <= 1.0
