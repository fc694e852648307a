"""numpy restatement of the three definitions behind transcribe_chunked (whisper_amd/csrc/chunk.hip), and
the test signal the chunking tests share.

  level : L[f] = log10( (1 / n_mels) * sum_m 10^(4 M[m][f] - 4) )
  cost  : C[f] = max L[g] over max(0, f - W) <= g <= min(content - 1, f + W)
  walk  : a = 0; while content - a > hi: c = the f in [a + lo, a + hi] with the smallest C, the largest f among equal
          minima; emit c; a = c
"""
import numpy as np


def level(mel, dtype=np.float64):
    m = np.asarray(mel).astype(dtype)
    return np.log10(np.power(dtype(10), dtype(4) * m - dtype(4)).sum(axis=0, dtype=dtype) / dtype(m.shape[0]))


def cost(L, W):
    L = np.asarray(L)
    n = len(L)
    pad = np.concatenate([np.full(W, -np.inf, L.dtype), L, np.full(W, -np.inf, L.dtype)])
    return np.max(np.stack([pad[j: j + n] for j in range(2 * W + 1)]), axis=0)


def walk(C, content, lo=1500, hi=3000):
    a, cuts = 0, []
    while content - a > hi:
        window = np.asarray(C[a + lo: a + hi + 1])
        a = a + lo + int(np.flatnonzero(window == window.min())[-1])
        cuts.append(a)
    return cuts


def burst(rng, n):
    """the bursts of tests/test_api_gpu.py::audio, drawn from a running generator"""
    t = np.arange(n) / 16000.0
    x = rng.standard_normal(n).astype(np.float32) * 0.05
    return x + (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 1870 * t)).astype(np.float32)


def make_signal(gap_noise=0.0, n_bursts=40, seed=0):
    """n_bursts bursts of 3 - 12 s, each followed by a gap of 0.6 - 2.0 s (digital zero, or gap_noise * N(0, 1)), closed by
    a 5 s burst: about 366 s for 40.  Returns (samples fp32, gaps) with gaps = [(first sample, end sample), ...]."""
    rng = np.random.default_rng(seed)
    parts, gaps, at = [], [], 0
    for _ in range(n_bursts):
        n = int(rng.uniform(3.0, 12.0) * 16000)
        parts.append(burst(rng, n))
        at += n
        g = int(rng.uniform(0.6, 2.0) * 16000)
        parts.append((rng.standard_normal(g) * gap_noise).astype(np.float32) if gap_noise else np.zeros(g, np.float32))
        gaps.append((at, at + g))
        at += g
    parts.append(burst(rng, 5 * 16000))
    return np.concatenate(parts), gaps


def in_gap(cut, gaps, W, hop=160):
    """is frame `cut` inside one of the constructed gaps (sample ranges), at least W frames from both of its edges"""
    return any(start / hop + W <= cut <= end / hop - W for start, end in gaps)
