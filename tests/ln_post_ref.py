"""LayerNorm behind the MFMAs (whisper_amd/csrc/kernels.h): the float64 reference, the error bound and an emulation of the
kernel's arithmetic, shared by tests/test_ln_post_cpu.py (which derives and checks the bound) and tests/test_ln_post_gpu.py
(which holds the kernels to it).  Not a test module.

The projection.  With the LayerNorm affine part folded into W / b, a per-row centre c, xc = x - c, m = mean_k(xc),
v = mean_k(xc^2) - m^2 and s_n = sum_k W[n][k]:

    y[r][n] = b[n] + rsqrt(v_r + 1e-5) * (sum_k W[n][k] xt[r][k] - m_r s_n),        xt = fp16(xc)

where m, v are taken from xt — the very values that were multiplied.  In exact arithmetic this IS the LayerNorm projection
of the rows xt (LayerNorm does not see a shift), so against the true projection of x the error is (a) what rounding x - c
to fp16 does to a LayerNorm projection, (b) the fp32 arithmetic.  The contract on the centre: |c - mean(x)| <= std(x) (the
decode step centres with the exact row mean at the layer's first LayerNorm site, LN -> QKV, of the same step).

The bound (ln_post_bound), per output, sig = std(x), s = sqrt(var + 1e-5), r = 1 / s, pre = the true projection:

  (a) e = xt - xc, |e_k| <= eps_k = (2^-11 + 2^-23) (|x_k - mu| + sig) + 2^-25 : half an fp16 ulp of a value that is at most
      |x_k - mu| + sig for every admissible centre, the fp32 subtraction in front of it, the fp16 subnormal quantum.
      y~ - y = r~ sum_k W_k (e_k - mean e) + (r~ / r - 1)(y - b).  The standard deviation is 1-Lipschitz in the rms of a
      perturbation, so |s~ - s| <= rho = rms(eps), |r~ / r - 1| <= eta = rho / (s - rho):
          r (1 + eta) sum_k |W_k| (eps_k + mean eps) + eta |pre - b|
      Its leading part is 2^-11 |x - c| rstd |W| summed over k.
  (b) C_DOT = 2^-20 per fp32 dot product of K terms, as everywhere in parity_ref.py, with A_k = |x_k - mu| + sig >= |xt_k|:
          the MFMA sum          C_DOT r sum_k |W_k| A_k
          s_n, times |m|        C_DOT r (sig + mean eps) sum_k |W_k|
          m, times |s_n|        C_DOT r mean(A) sum_k |W_k|
          v = E[xt^2] - m^2     E[xt^2] and m^2 each carry C_DOT of themselves, E <= mean(A^2), m^2 <= 2 sig^2 (never a
                                cancellation that matters: |m| <= sig makes E <= 2 var + ...); through rsqrt
                                (C_DOT (mean(A^2) + 2 sig^2) / (2 (var + 1e-5)) + 2^-21) |pre - b|
          the closing FMAs      2^-22 |pre|
  plus one ulp of the output type at pre (rounding, and a flip across a boundary).

A centre outside the contract is NOT covered: with c = 0 and mean / std = 30 the rows are rounded at 30 sig instead of <= 2
sig or so, and a weight row aligned with the rounding errors shows 4 x the bound (test_ln_post_cpu.py) — the reason the
centring exists.
"""
import torch

C_DOT = 2.0 ** -20


def _ulp16(x):
    a = x.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def ln_true(xd, Wd, bd):
    """float64 LayerNorm projection (eps 1e-5, affine folded): (pre [R][N], mu [R][1], var [R][1])"""
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    xn = (xd - mu) / torch.sqrt(var + 1e-5)
    return xn @ Wd.T + (bd.view(1, -1) if bd is not None else 0.0), mu, var


def ln_post_bound(xd, Wd, bd, pre, mu, var):
    """bound on |y - pre| for an fp16 output (module docstring); xd [R][K], Wd [N][K], bd [N] or None, all float64"""
    return _ulp16(pre) + ln_post_slack(xd, Wd, bd, pre, mu, var)


def ln_post_slack(xd, Wd, bd, pre, mu, var):
    """the bound without the output's ulp (what an epilogue function is applied to)"""
    sig = torch.sqrt(var)
    s = torch.sqrt(var + 1e-5)
    r = 1.0 / s
    A = (xd - mu).abs() + sig
    eps = (2.0 ** -11 + 2.0 ** -23) * A + 2.0 ** -25
    ebar = eps.mean(1, keepdim=True)
    rho = torch.sqrt((eps ** 2).mean(1, keepdim=True))
    eta = rho / (s - rho)
    Wa = Wd.abs()
    wsum = Wa.sum(1).view(1, -1)
    lin = pre - (bd.view(1, -1) if bd is not None else 0.0)
    rounding = r * (1 + eta) * ((eps + ebar) @ Wa.T) + eta * lin.abs()
    dot = C_DOT * r * (A @ Wa.T)
    sn = C_DOT * r * (sig + ebar) * wsum
    mm = C_DOT * r * A.mean(1, keepdim=True) * wsum
    vv = (C_DOT * ((A ** 2).mean(1, keepdim=True) + 2 * var) / (2 * (var + 1e-5)) + 2.0 ** -21) * lin.abs()
    return rounding + dot + sn + mm + vv + 2.0 ** -22 * pre.abs()


def centred_fp16(x32, c32):
    """what a producer stores: fp16(x - c) computed in fp32, saturated to the fp16 range"""
    return (x32.float() - c32.float().view(-1, 1)).clamp(-65504.0, 65504.0).half()


def ln_post_emulate(xt, W16, b32):
    """the kernel's arithmetic on the fp16 rows xt [R][K] and fp16 weights W16 [N][K]: fp16 products summed in fp32 (torch
    sums in another order than the MFMAs — covered by C_DOT), fp32 statistics of xt, the epilogue formula; returns fp16 y"""
    K = xt.shape[1]
    xf, Wf = xt.float(), W16.float()
    dot = xf @ Wf.T
    m = xf.sum(1, keepdim=True) / K
    v = ((xf * xf).sum(1, keepdim=True) / K - m * m).clamp_min(0.0)
    sn = Wf.sum(1).view(1, -1)
    y = torch.rsqrt(v + 1e-5) * (dot - m * sn)
    if b32 is not None:
        y = y + b32.float().view(1, -1)
    return y.half(), m
