"""Float64 restatement of the device-side audio ingest (DESIGN.md §5b "Device-side ingest"; csrc/resample.hip), in numpy and
independent of whisper_amd.audio.resample_taps.  For input rate `rate`, target `sr`, g = gcd(rate, sr), up = sr / g,
down = rate / g, M = max(up, down), half = 10 M:

    taps[j] = up * w[j + half] * sinc(j / M) / M / S         -half <= j <= half,  w = numpy.kaiser(2 half + 1, 5.0),
                                                             S = sum_j w[j + half] * sinc(j / M) / M
    mono[k] = (sum over channels of pcm[k][c]) / (channels * full_scale)              0 <= k < n_in
    y[m]    = sum_k taps[m * down - k * up] * mono[k]                                 0 <= m < n_out = ceil(n_in * up / down)
    out[m]  = clip(rint(32768 * y[m]), -32768, 32767) / 32768

with samples outside [0, n_in) taken as zero: scipy.signal.resample_poly(mono, up, down) with its default window, then the
16-bit quantisation of the host path.  rate == sr: no filter (y = mono)."""
from math import gcd

import numpy as np


def ratio(rate: int, sr: int):
    g = gcd(int(rate), int(sr))
    return int(sr) // g, int(rate) // g


def taps(rate: int, sr: int):
    """(taps float64 [2 half + 1], half)"""
    up, down = ratio(rate, sr)
    m = max(up, down)
    half = 10 * m
    j = np.arange(-half, half + 1).astype(np.float64)
    h = np.kaiser(2 * half + 1, 5.0) * np.sinc(j / m) / m
    return up * h / h.sum(), half


def full_scale(pcm: np.ndarray, bits: int) -> float:
    if pcm.dtype == np.uint8:
        return 128.0
    return float(2 ** (bits - 1)) if pcm.dtype.kind == "i" else 1.0


def mono(pcm: np.ndarray, bits: int) -> np.ndarray:
    """pcm [frames][channels] as stored (uint8: offset 128) -> float64 [frames]"""
    x = pcm.astype(np.int64) - 128 if pcm.dtype == np.uint8 else pcm.astype(np.int64 if pcm.dtype.kind == "i" else np.float64)
    return x.sum(axis=1).astype(np.float64) / (pcm.shape[1] * full_scale(pcm, bits))


def resample(x: np.ndarray, rate: int, sr: int) -> np.ndarray:
    """y of the definition, float64 [ceil(n * up / down)]"""
    up, down = ratio(rate, sr)
    n = len(x)
    if up == down:
        return x.astype(np.float64)
    t, half = taps(rate, sr)
    n_out = -(-n * up // down)
    m = np.arange(n_out, dtype=np.int64)
    c = m * down + half
    q, k_hi = c % up, c // up                               # output m meets tap index q + i up at input k_hi - i
    y = np.zeros(n_out, dtype=np.float64)
    for i in range((2 * half) // up + 1):
        idx, k = q + i * up, k_hi - i
        ok = (idx <= 2 * half) & (k >= 0) & (k < n)
        y[ok] += t[idx[ok]] * x[k[ok]]
    return y


def quantise(y: np.ndarray) -> np.ndarray:
    return (np.clip(np.rint(32768.0 * y), -32768, 32767) / 32768.0).astype(np.float32)


def ingest(pcm: np.ndarray, rate: int, sr: int = 16000, bits: int = 16) -> np.ndarray:
    """the whole definition: stored PCM [frames][channels] -> float32 [n_out] on the 16-bit grid"""
    return quantise(resample(mono(pcm, bits), rate, sr))


# ---- test signals ---------------------------------------------------------------------------------------------------------
FORMATS = ("u8", "s16", "s24", "s32", "f32")


def signal(n: int, channels: int, rate: int, seed: int) -> np.ndarray:
    """float64 [n][channels] on the 16-bit grid: 0.3 sine + 0.1 noise per channel (different pitches), fixed seed"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] / float(rate)
    x = 0.3 * np.sin(2 * np.pi * (220.0 + 110.0 * np.arange(channels)[None, :]) * t) + 0.1 * rng.standard_normal((n, channels))
    return np.clip(np.round(x * 32768.0), -32768, 32767) / 32768.0


def store(x: np.ndarray, fmt: str):
    """the signal as a reader would hold it: (array in the stored type, bits)"""
    if fmt == "u8":
        return np.clip(np.round(x * 128.0) + 128, 0, 255).astype(np.uint8), 8
    if fmt == "s16":
        return np.round(x * 32768.0).astype(np.int16), 16
    if fmt == "s24":
        return np.round(x * 8388608.0).astype(np.int32), 24
    if fmt == "s32":
        return np.round(x * 2147483648.0).astype(np.int64).astype(np.int32), 32
    if fmt == "f32":
        return x.astype(np.float32), 32
    raise ValueError(fmt)
