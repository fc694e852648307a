"""The float64 references of tests/parity_ref.py that tests/test_fused_attn_parity_gpu.py judges the fused attention
kernels by, checked here — without a GPU — against oracle/model.py's own cross- and self-attention blocks on a tiny random
configuration: the LayerNorm-folded projection, the split attention with its merge, and the append followed by attend.
With dtype F64 the references round nothing, so they must agree with the oracle (float64 activations) to 1e-12."""
from types import SimpleNamespace

import torch

from oracle.model import OracleModel
from parity_ref import F64, _merge_ref, attn_ref, cross_block_ref, ln_gemv_ref, self_block_ref

TOL = 1e-12
D, H, R = 128, 2, 3


def _oracle(seed):
    """one decoder block's attention weights, random, with a non-trivial LayerNorm affine; (oracle, folded weights)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * sc
    p = "decoder.blocks.0"
    sd = {}
    for ln in ("attn_ln", "cross_attn_ln"):
        sd[f"{p}.{ln}.weight"], sd[f"{p}.{ln}.bias"] = 1.0 + 0.2 * rn(D), 0.1 * rn(D)
    for lin in ("attn.query", "attn.key", "attn.value", "cross_attn.query"):
        sd[f"{p}.{lin}.weight"] = rn(D, D, sc=D ** -0.5)
        if not lin.endswith("key"):
            sd[f"{p}.{lin}.bias"] = rn(D, sc=0.5)
    om = OracleModel(SimpleNamespace(n_text_head=H), sd, dtype=torch.float64)
    sd = {k: v.double() for k, v in om.sd.items()}                 # the fp32 values the oracle holds

    def fold(ln, lins):
        """W' = W diag(ln.weight), b' = b + W ln.bias — the load-time fold the kernels' weights carry"""
        ws, bs = [], []
        for lin in lins:
            W = sd[f"{p}.{lin}.weight"]
            b = sd.get(f"{p}.{lin}.bias", torch.zeros(D, dtype=torch.float64))
            ws.append(W * sd[f"{p}.{ln}.weight"].view(1, -1))
            bs.append(b + W @ sd[f"{p}.{ln}.bias"])
        return torch.cat(ws), torch.cat(bs)
    return om, p, fold


def test_ln_folded_projection_matches_oracle():
    om, p, fold = _oracle(1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(R, D, generator=g, dtype=torch.float64) * 1.5 + 0.7
    W, b = fold("cross_attn_ln", ["cross_attn.query"])
    pre, slack, X = ln_gemv_ref(x, W, b, F64)
    want = om._lin(om._ln(x.unsqueeze(1), p + ".cross_attn_ln"), p + ".cross_attn.query")[:, 0]
    assert (pre - want).abs().max() < TOL
    assert (slack > 0).all()
    # the perturbed reference of the GPU file really leaves a K block out
    pert, _, _ = ln_gemv_ref(x, W, b, F64, drop_last_block=True)
    assert (pert - (X[:, :D - 64] @ W[:, :D - 64].T + b)).abs().max() < TOL and (pert - pre).abs().max() > 1e-3


def test_cross_block_with_splits_and_merge_matches_oracle():
    om, p, fold = _oracle(3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(R, D, generator=g, dtype=torch.float64)
    W, b = fold("cross_attn_ln", ["cross_attn.query"])
    for (Tk, S, gran) in ((1, 1, 64), (70, 1, 64), (70, 2, 64), (200, 3, 64), (200, 3, 32), (100, 8, 64), (130, 4, 32)):
        K = torch.randn(R, Tk + 2, D, generator=g, dtype=torch.float64)
        V = torch.randn(R, Tk + 2, D, generator=g, dtype=torch.float64)
        K[:, Tk:], V[:, Tk:] = float("nan"), float("nan")          # never read
        pre, _, a = cross_block_ref(x, W, b, K, V, Tk, S, gran, F64, H)
        q = om._lin(om._ln(x.unsqueeze(1), p + ".cross_attn_ln"), p + ".cross_attn.query")
        want, _ = om._attend(q, K[:, :Tk], V[:, :Tk], H, None)
        assert (pre - q[:, 0]).abs().max() < TOL
        assert (a["ref"] - want[:, 0]).abs().max() < TOL, (Tk, S, gran)
        # the per-split partials (what the kernels store) merge to the same rows; empty splits are (0, -inf, 0)
        merged, _ = _merge_ref(a["po"].view(S, R, H, 64), a["pm"], a["pl"])
        assert (merged.reshape(R, D) - want[:, 0]).abs().max() < TOL, (Tk, S, gran)
        chunk = -(-(-(-Tk // S)) // gran) * gran
        for s in range(S):
            if s * chunk >= Tk:
                assert (a["po"][s] == 0).all() and torch.isinf(a["pm"][s]).all() and (a["pl"][s] == 0).all()
            else:
                assert torch.isfinite(a["pm"][s]).all() and (a["pl"][s] >= 1.0).all()
        if Tk >= 2:                                                  # the perturbed references differ from the reference
            assert (a["pert"] - a["ref"]).abs().max() > 1e-6
    K = torch.randn(R, 200, D, generator=g, dtype=torch.float64)
    V = torch.randn(R, 200, D, generator=g, dtype=torch.float64)
    _, _, a = cross_block_ref(x, W, b, K, V, 200, 3, 64, F64, H)
    _, _, s = cross_block_ref(x, W, b, K, V, 200, 3, 64, F64, H, shift=(1, 32))
    assert (a["ref"] - s["ref"]).abs().max() < TOL                   # a moved boundary changes the partials, not their merge
    assert (a["pl"][1] - s["pl"][1]).abs().max() > 1e-3


def test_self_block_append_then_attend_matches_oracle():
    om, p, fold = _oracle(5)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(R, D, generator=g, dtype=torch.float64)
    W, b = fold("attn_ln", ["attn.query", "attn.key", "attn.value"])
    n_ctx = 80
    for (pos, lags) in ((0, None), (1, None), (5, [0, 3, 1]), (66, [0, 3, 1]), (79, [2, 0, 15])):
        kc = torch.randn(R, n_ctx, D, generator=g, dtype=torch.float64)
        vc = torch.randn(R, n_ctx, D, generator=g, dtype=torch.float64)
        for r in range(R):                                           # the slot to append to and everything behind it: never read
            at = pos - (lags[r] if lags else 0)
            kc[r, at:], vc[r, at:] = float("nan"), float("nan")
        pre, _, kc2, vc2, lens, a = self_block_ref(x, W, b, kc, vc, pos, lags, F64, H)
        h = om._ln(x.unsqueeze(1), p + ".attn_ln")
        q, k, v = (om._lin(h, f"{p}.attn.{n}") for n in ("query", "key", "value"))
        assert (pre - torch.cat([q, k, v], 2)[:, 0]).abs().max() < TOL
        for r in range(R):                                           # oracle/model.py:104-109: concatenate, then attend
            at = lens[r] - 1
            kk = torch.cat([kc[r:r + 1, :at], k[r:r + 1]], 1)
            vv = torch.cat([vc[r:r + 1, :at], v[r:r + 1]], 1)
            want, _ = om._attend(q[r:r + 1], kk, vv, H, at)
            assert (a["ref"][r] - want[0, 0]).abs().max() < TOL, (pos, lags, r)
            assert torch.equal(kc2[r, at], pre[r, D:2 * D]) and torch.equal(vc2[r, at], pre[r, 2 * D:])
            assert torch.isnan(kc2[r, at + 1:]).all() and torch.equal(kc2[r, :at], kc[r, :at])
