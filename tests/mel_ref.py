"""Float64 reference of the log-mel front end (whisper_amd/csrc/mel.hip) with a per-element bound, the signal classes it is
checked on, and a numpy float32 model of mel_kernel's arithmetic.  Not a test module: tests/test_mel_ref_cpu.py checks the
reference, the bound and the model without a GPU, tests/test_mel_parity_gpu.py holds the kernel to the bound.

The bound lives in the power domain.  A flat tolerance on the output cannot work: the output is a logarithm, so the error of
a mel row is relative to THAT ROW's power, while the fp32 error of a DFT bin is relative to the frame's energy — a quiet bin
beside a loud one (a pure tone, DC, a padded window) is where mel_kernel's two folds and its rotated twiddles lose digits.

  S_f   = sum_j |x_j| w_j                      the absolute sum of the windowed frame
  dX    = C_MEL * S_f                          fp32 spectrum against float64, any bin of the frame (C_MEL: parity_ref.py)
  dP_k  = 2 sqrt(P_k) dX + dX^2                power of bin k
  dPm   = F . dP + n_band 2^-24 Pm             mel row: the filter applied to dP, plus the worst case of a non-negative fma sum
                                               over the n_band taps between the row's first and last non-zero weight
  lo, hi = max(Pm - dPm, 0), Pm + dPm          the interval of the mel power; M_lo, M_hi the log10 of their clamped maxima
  bound = max(ref - g(lo, M_lo), g(hi, M_hi) - ref) + U_OUT

with g(Pm, M) = (max(log10(max(Pm, 1e-10)), M - 8) + 4) / 4 the finish, which is monotone in both arguments: the interval is
carried through it as it is, nothing is linearised.  U_OUT = 2^-21 (|4 ref - 4| + 4) / 4 + 2^-23 covers log10f at 2 ulp of
|log10| = |4 ref - 4| (the figure of the HIP math API's accuracy table for log10f; the OCML documentation itself is not part of
the ROCm tree this was written against), the rounded add of 4 and the final fp32 rounding."""
import numpy as np

from parity_ref import C_MEL

N_FFT, HOP, HALF, NBIN = 400, 160, 200, 201
SR = 16000
N_CLASS = 32000                                 # 200 frames: 13 workgroups of 16, the last half filled

CLASSES = ("noise+sines", "tone440", "tone_bin25", "tone7990", "square", "dc+tiny", "zeros", "click", "quiet", "speech+pad",
           "tone+noise-90dB", "full-scale noise")


def signals(n=N_CLASS):
    """{class: float32 [n]}, deterministic"""
    t = np.arange(n) / float(SR)
    rng = lambda seed: np.random.default_rng(seed)
    tone = lambda f, a: a * np.sin(2 * np.pi * f * t)
    half = n // 2
    th = t[:half]
    dur = max(half, 1) / float(SR)
    chirp = np.zeros(n)
    # linear chirp 200 -> 800 Hz over the first half under a Hann envelope, on the 16-bit grid; zeros behind it
    chirp[:half] = 0.5 * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(half) / max(half, 1))) * \
        np.sin(2 * np.pi * (200.0 * th + 0.5 * (600.0 / dur) * th * th))
    chirp = np.round(chirp * 32768.0) / 32768.0
    click = np.zeros(n)
    click[min(n - 1, 5003 if n > 5003 else n // 2)] = 1.0
    out = {
        "noise+sines": rng(10).standard_normal(n).astype(np.float32) * 0.05
        + (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 1870 * t)).astype(np.float32),
        "tone440": tone(440.0, 0.5),
        "tone_bin25": tone(1000.0, 0.5),
        "tone7990": tone(7990.0, 0.9),
        "square": np.where(np.sin(2 * np.pi * 313.0 * t) >= 0, 1.0, -1.0),
        "dc+tiny": 0.5 + 1e-4 * rng(11).standard_normal(n),
        "zeros": np.zeros(n),
        "click": click,
        "quiet": np.round(rng(12).standard_normal(n)) / 32768.0,
        "speech+pad": chirp,
        "tone+noise-90dB": tone(440.0, 0.5) + 0.5 * 10.0 ** (-90.0 / 20.0) * rng(13).standard_normal(n),
        "full-scale noise": np.clip(rng(14).standard_normal(n), -1.0, 1.0),
    }
    assert tuple(out) == CLASSES
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def band_of(filters):
    """(lo, hi) per filter row: first and last non-zero tap; (201, -1) for an all-zero row, as mel_bands_kernel leaves it"""
    nz = np.asarray(filters) != 0
    lo = np.where(nz.any(1), nz.argmax(1), NBIN)
    hi = np.where(nz.any(1), NBIN - 1 - nz[:, ::-1].argmax(1), -1)
    return lo.astype(np.int64), hi.astype(np.int64)


def _finish(Pm, M, floor=8.0):
    return (np.maximum(np.log10(np.maximum(Pm, 1e-10)), M - floor) + 4.0) / 4.0


def _log_max(Pm, per_clip):
    """log10 of the clamped maximum: over the whole batch (whisper/audio.py:155), or per clip (a perturbation)"""
    lg = np.log10(np.maximum(Pm, 1e-10))
    return lg.max(axis=(1, 2), keepdims=True) if per_clip else lg.max()


def mel_ref(audio, filters, symmetric_window=False, shift=0, drop_tap200=False, edge_pad=False, drop_first=False,
            max_per_clip=False, floor=8.0):
    """float64 log-mel of audio [B][n] (or [n]) under filters [n_mels][201] -> (ref, bound), both [B][n_mels][n // 160]:
    reflect pad 200, periodic Hann, rfft, last frame dropped, power, filterbank, clamp(1e-10).log10(), global max over the
    whole batch, max(., M - 8), (. + 4) / 4 — whisper/audio.py:110-157, as oracle.log_mel_spectrogram states it.  The keywords
    are the perturbed references of the non-vacuity checks: a symmetric Hann window, frames `shift` samples late, tap 200 (the
    centre sample) dropped, edge-replicate padding, the first frame dropped instead of the last, the maximum per clip, and
    M - `floor`.  The bound (module docstring) is that of the unperturbed kernel either way."""
    x = np.asarray(audio, dtype=np.float64)
    x = x[None] if x.ndim == 1 else x
    F = np.asarray(filters, dtype=np.float64)
    B, n = x.shape
    nf = n // HOP
    i = np.arange(N_FFT)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * i / (N_FFT - 1 if symmetric_window else N_FFT))
    if drop_tap200:
        w = w.copy()
        w[HALF] = 0.0
    xp = np.pad(x, ((0, 0), (HALF, HALF)), mode="edge" if edge_pad else "reflect")
    first = 1 if drop_first else 0
    idx = (np.arange(first, first + nf) * HOP + shift)[:, None] + i[None, :]
    fr = xp[:, idx] * w                                            # [B][nf][400]
    spec = np.fft.rfft(fr, axis=-1)
    P = (spec.real ** 2 + spec.imag ** 2).transpose(0, 2, 1)       # [B][201][nf]
    Pm = F @ P
    M = _log_max(Pm, max_per_clip)
    ref = _finish(Pm, M, floor)

    S = np.abs(fr).sum(-1)[:, None, :]                             # [B][1][nf]
    dX = C_MEL * S
    dP = 2.0 * np.sqrt(P) * dX + dX * dX
    lo_t, hi_t = band_of(F)
    n_band = np.maximum(hi_t - lo_t + 1, 0).astype(np.float64)[None, :, None]
    dPm = F @ dP + n_band * 2.0 ** -24 * Pm
    lo, hi = np.maximum(Pm - dPm, 0.0), Pm + dPm
    g_lo, g_hi = _finish(lo, _log_max(lo, max_per_clip), floor), _finish(hi, _log_max(hi, max_per_clip), floor)
    u_out = 2.0 ** -21 * (np.abs(4.0 * ref - 4.0) + 4.0) / 4.0 + 2.0 ** -23
    bound = np.maximum(ref - g_lo, g_hi - ref) + u_out
    return ref, bound


# ------------------------------------------------------------------------------------------- float32 model of mel_kernel
def mel_tables():
    """cos / sin(2 pi i / 400) and the periodic Hann window as api.cpp: mel_tables builds them: float64, rounded once"""
    i = np.arange(N_FFT)
    return (np.cos(2.0 * np.pi * i / 400.0).astype(np.float32), np.sin(2.0 * np.pi * i / 400.0).astype(np.float32),
            (0.5 - 0.5 * np.cos(2.0 * np.pi * i / 400.0)).astype(np.float32))


def _fma(a, b, c):
    """a * b + c with one rounding: the product of two float32 is exact in float64 (the float64 sum's own rounding, 2^-53, is
    the model's only departure from a fused multiply-add)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def emulate_power_fp32(audio, resync=16):
    """the float32 power spectrum [B][201][n // 160] as mel_kernel forms it: the tap fold e[j] = x[j] + x[400 - j], d[j] =
    x[j] - x[400 - j] of the windowed frame (taps 0 and 200 single), one lane per bin pair (k, 200 - k) with even and odd taps
    in accumulators of their own, the twiddle advanced by a rotation in registers and re-read from the table every `resync`
    taps over 208 zero-padded taps, X[k] = E + O and X[200 - k] = E - O, bin 100 written by both (the second write stays)"""
    f32 = np.float32
    x = np.asarray(audio, dtype=np.float32)
    x = x[None] if x.ndim == 1 else x
    B, n = x.shape
    nf = n // HOP
    cos_t, sin_t, win = mel_tables()
    xp = np.pad(x, ((0, 0), (HALF, HALF)), mode="reflect")
    base = np.arange(nf) * HOP
    ntap = (HALF + 1 + resync - 1) // resync * resync
    ev = np.zeros((ntap, B, nf), dtype=f32)
    od = np.zeros((ntap, B, nf), dtype=f32)
    for j in range(HALF + 1):
        x1 = xp[:, base + j] * win[j]
        if j == 0 or j == HALF:
            ev[j] = x1
        else:
            x2 = xp[:, base + N_FFT - j] * win[N_FFT - j]
            ev[j], od[j] = x1 + x2, x1 - x2
    k = np.arange(HALF // 2 + 1)                                  # 0 .. 100
    ct, st = cos_t[k][:, None, None], sin_t[k][:, None, None]     # rotation by one tap
    re = np.zeros((2, len(k), B, nf), dtype=f32)
    im = np.zeros((2, len(k), B, nf), dtype=f32)
    for j0 in range(0, ntap, resync):
        idx = (k * j0) % N_FFT
        c, s = cos_t[idx][:, None, None], sin_t[idx][:, None, None]
        for jj in range(resync):
            j = j0 + jj
            p = j & 1
            re[p] = _fma(c, ev[j][None], re[p])
            im[p] = _fma(s, od[j][None], im[p])
            cn = _fma(c, ct, -(s * st))
            s = _fma(s, ct, c * st)
            c = cn
    rk, ik = re[0] + re[1], im[0] + im[1]
    rm, imm = re[0] - re[1], im[0] - im[1]
    pk, pm = rk * rk + ik * ik, rm * rm + imm * imm
    P = np.zeros((NBIN, B, nf), dtype=f32)
    P[k] = pk
    P[HALF - k] = pm
    return np.ascontiguousarray(P.transpose(1, 0, 2))


def emulate_finish_fp32(P, filters):
    """mel rows of the float32 power spectrum P [B][201][F] as mel_kernel sums them (one fma per tap, first to last non-zero
    tap in order), log10f of the clamp, the global maximum and mel_finish_kernel"""
    f32 = np.float32
    F = np.asarray(filters, dtype=np.float32)
    lo, hi = band_of(F)
    B, _, nf = P.shape
    acc = np.zeros((B, F.shape[0], nf), dtype=f32)
    for m in range(F.shape[0]):
        for kk in range(lo[m], hi[m] + 1):
            acc[:, m] = _fma(F[m, kk], P[:, kk], acc[:, m])
    v = np.log10(np.maximum(acc, f32(1e-10)).astype(np.float64)).astype(f32)
    floor_v = f32(v.max() - f32(8.0))
    return ((np.maximum(v, floor_v) + f32(4.0)) / f32(4.0)).astype(f32)


def emulate_fp32(audio, filters, resync=16):
    """numpy float32 model of wh_log_mel -> float32 [B][n_mels][n // 160].  It follows mel_kernel's order of operations, with
    a single rounding per multiply-add; it is not meant to be bit-equal to the GPU (the compiler is free to contract the
    remaining products and sums, and log10f is not correctly rounded there)"""
    return emulate_finish_fp32(emulate_power_fp32(audio, resync), filters)
