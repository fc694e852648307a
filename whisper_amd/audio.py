"""Audio front end of whisper_amd — the reference's `whisper/audio.py` surface (constants :13-22, load_audio :25,
pad_or_trim :65, mel_filters :91, log_mel_spectrogram :110) with the spectrogram computed by the fused HIP
kernel (csrc/mel.hip) instead of torch.stft + a dense matmul."""
from __future__ import annotations

import os
import struct
import subprocess
from functools import lru_cache
from typing import Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import hip
from .utils import exact_div

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE          # 480000 samples per 30 s window
N_FRAMES = exact_div(N_SAMPLES, HOP_LENGTH)     # 3000 mel frames per window
N_SAMPLES_PER_TOKEN = HOP_LENGTH * 2            # conv2 has stride 2
FRAMES_PER_SECOND = exact_div(SAMPLE_RATE, HOP_LENGTH)
TOKENS_PER_SECOND = exact_div(SAMPLE_RATE, N_SAMPLES_PER_TOKEN)


def _parse_wav(path: str):
    """Minimal RIFF/WAVE reader (PCM 8/16/24/32-bit and float32/64): (samples [frames][channels] in their stored type — uint8,
    int16, int32, float32, float64; 24-bit sign-extended to int32 —, sample rate, bits per sample), or None for a file it
    cannot read.  The samples are a view of the file's bytes wherever the stored type allows it."""
    with open(path, "rb") as f:
        data = bytearray(os.fstat(f.fileno()).st_size)
        data = memoryview(data)[: f.readinto(data)]
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        return None
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        tag, size = bytes(data[pos: pos + 4]), struct.unpack("<I", data[pos + 4: pos + 8])[0]
        body = data[pos + 8: pos + 8 + size]
        if tag == b"fmt ":
            if len(body) < 16:
                return None                                   # truncated fmt chunk: not a file we can read
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE:                              # WAVE_FORMAT_EXTENSIBLE: the real format tag is the first
                if len(body) < 26:                            # two bytes of the SubFormat GUID (1 = PCM, 3 = IEEE float)
                    return None
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
        elif tag == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        return None
    code, channels, rate, _, _, bits = fmt
    if channels == 0 or rate == 0:
        return None
    if code == 3 and bits == 32:
        x = np.frombuffer(pcm[: len(pcm) // 4 * 4], "<f4")
    elif code == 3 and bits == 64:
        x = np.frombuffer(pcm[: len(pcm) // 8 * 8], "<f8")
    elif code == 1 and bits == 16:
        x = np.frombuffer(pcm[: len(pcm) // 2 * 2], "<i2")
    elif code == 1 and bits == 32:
        x = np.frombuffer(pcm[: len(pcm) // 4 * 4], "<i4")
    elif code == 1 and bits == 24:
        b = np.frombuffer(pcm[: len(pcm) // 3 * 3], np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = v - ((v & 0x800000) << 1)
    elif code == 1 and bits == 8:
        x = np.frombuffer(pcm, np.uint8)
    else:
        return None
    return x[: len(x) // channels * channels].reshape(-1, channels), rate, bits


def _pcm_to_float(pcm: np.ndarray, bits: int) -> np.ndarray:
    """stored samples (`_parse_wav`, `decode_flac`) -> float32 in [-1, 1): uint8 is offset binary, the signed integer types
    have full scale 2^(bits-1)"""
    if pcm.dtype == np.uint8:
        return (pcm.astype(np.float32) - 128.0) / 128.0
    if pcm.dtype.kind == "i":
        return pcm.astype(np.float32) / float(1 << (bits - 1))
    return pcm.astype(np.float32)


def _read_wav(path: str, sr: int) -> Optional[np.ndarray]:
    parsed = _parse_wav(path)
    if parsed is None:
        return None
    pcm, rate, bits = parsed
    return _to_mono_s16(_pcm_to_float(pcm, bits), rate, sr)


@lru_cache(maxsize=None)
def resample_taps(rate: int, sr: int) -> np.ndarray:
    """The filter scipy.signal.resample_poly(x, up, down) designs by default for up / down = sr / rate in lowest terms, as
    float64 [2 * half + 1] with half = 10 * max(up, down) (centre at index half): a Kaiser(5.0)-windowed sinc with cutoff
    1 / max(up, down), unit gain at DC, times up.  [1.0] when rate == sr.  Read-only (the array is cached)."""
    from math import gcd
    g = gcd(int(rate), int(sr))
    up, down = int(sr) // g, int(rate) // g
    if up == down:
        taps = np.ones(1, dtype=np.float64)
    else:
        m = max(up, down)
        half = 10 * m
        h = np.kaiser(2 * half + 1, 5.0) * np.sinc(np.arange(-half, half + 1, dtype=np.float64) / m) / m
        taps = up * h / h.sum()
    taps.setflags(write=False)
    return taps


def _to_mono_s16(x: np.ndarray, rate: int, sr: int) -> np.ndarray:
    """[frames][channels] float in [-1, 1) -> what `ffmpeg -ac 1 -ar sr -f s16le` hands the reference: equal-weight
    down-mix, linear-phase polyphase resampling, 16-bit quantisation."""
    x = x.mean(axis=1)
    if rate != sr:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(rate), int(sr))
        x = resample_poly(x, sr // g, rate // g).astype(np.float32)
    # ffmpeg's s16le round trip quantises to 16 bits; mirror it so both routes agree
    return (np.clip(np.round(x * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


_AUDIO_LIB = None


def _audio_lib():
    """whisper_amd/libwhisper_audio.so (csrc/flac_decode.c, plain C built by `make -C whisper_amd/csrc`)"""
    global _AUDIO_LIB
    if _AUDIO_LIB is None:
        import ctypes as C
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libwhisper_audio.so")
        if not os.path.isfile(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C whisper_amd/csrc`")
        lib = C.CDLL(path)
        lib.wh_flac_decode.restype = C.c_int
        lib.wh_flac_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.wh_flac_free.restype = None
        lib.wh_flac_free.argtypes = [C.POINTER(C.c_int32)]
        lib.wh_flac_error.restype = C.c_char_p
        lib.wh_flac_error.argtypes = [C.c_int]
        _AUDIO_LIB = lib
    return _AUDIO_LIB


def decode_flac(data: bytes):
    """FLAC bytes -> (int32 samples [frames][channels], sample_rate, bits_per_sample); CRC-8/16 of every frame and
    the STREAMINFO MD5 of the decoded audio are verified by the decoder (RuntimeError otherwise)."""
    import ctypes as C
    lib = _audio_lib()
    ptr, n, ch, rate, bps = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    rc = lib.wh_flac_decode(data, len(data), C.byref(ptr), C.byref(n), C.byref(ch), C.byref(rate), C.byref(bps))
    if rc != 0:
        raise RuntimeError(f"Failed to load audio: {lib.wh_flac_error(rc).decode()}")
    try:
        pcm = np.ctypeslib.as_array(ptr, shape=(n.value * ch.value,)).reshape(n.value, ch.value).copy()
    finally:
        lib.wh_flac_free(ptr)
    return pcm, rate.value, bps.value


def _parse_flac(path: str):
    """(int32 samples [frames][channels], sample rate, bits per sample) of a FLAC file, None for any other file"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"fLaC" and data[:3] != b"ID3":
        return None
    return decode_flac(data)


def _read_flac(path: str, sr: int) -> Optional[np.ndarray]:
    parsed = _parse_flac(path)
    if parsed is None:
        return None
    pcm, rate, bps = parsed
    return _to_mono_s16(_pcm_to_float(pcm, bps), rate, sr)


def _sniff(file: str) -> Optional[str]:
    """"wav" / "flac" from the first bytes of `file` (a FLAC stream may follow an ID3v2 tag, which the native decoder skips),
    None for any other container — or for something that is no readable file"""
    try:
        with open(file, "rb") as f:
            head = f.read(12)
            if head[:4] == b"RIFF" and head[8:12] == b"WAVE":
                return "wav"
            if head[:3] == b"ID3" and len(head) >= 10:
                f.seek(10 + ((head[6] & 127) << 21 | (head[7] & 127) << 14 | (head[8] & 127) << 7 | (head[9] & 127)))
                head = f.read(4)
            return "flac" if head[:4] == b"fLaC" else None
    except OSError:
        return None


MAX_DEVICE_CHANNELS = 8             # wh_resample: 1 - 8 channels


def parse_flac_info(data) -> Optional["hip.FlacInfo"]:
    """The metadata of a FLAC file held in memory, as csrc/flac_decode.c reads it: an ID3v2 tag is skipped, STREAMINFO gives
    rate, channels, sample size, sample count and block sizes, the first frame follows the last metadata block.  None for
    anything the host decoder would refuse at this point (it is the one to say why)."""
    n, pos = len(data), 0
    if n >= 10 and bytes(data[:3]) == b"ID3":
        pos = 10 + ((data[6] & 127) << 21 | (data[7] & 127) << 14 | (data[8] & 127) << 7 | (data[9] & 127))
    if pos + 4 > n or bytes(data[pos: pos + 4]) != b"fLaC":
        return None
    pos += 4
    info = None
    while True:
        if pos + 4 > n:
            return None
        last, kind = data[pos] >> 7, data[pos] & 127
        size = data[pos + 1] << 16 | data[pos + 2] << 8 | data[pos + 3]
        pos += 4
        if pos + size > n:
            return None
        if kind == 0:
            if size < 34:
                return None
            q = data[pos: pos + 34]
            info = dict(min_block=q[0] << 8 | q[1], max_block=q[2] << 8 | q[3], sample_rate=q[10] << 12 | q[11] << 4 | q[12] >> 4,
                        channels=((q[12] >> 1) & 7) + 1, bits_per_sample=((q[12] & 1) << 4 | q[13] >> 4) + 1,
                        total_samples=(q[13] & 15) << 32 | q[14] << 24 | q[15] << 16 | q[16] << 8 | q[17])
        pos += size
        if last:
            break
    if info is None or info["sample_rate"] == 0 or info["max_block"] < 16 or not 4 <= info["bits_per_sample"] <= 32:
        return None
    return hip.FlacInfo(first_frame=pos, **info)


class _FlacFile:
    """a FLAC file read but not decoded: what `_ingest_host(..., decode_on_device=True)` hands `_ingest_device`"""
    __slots__ = ("data", "info")

    def __init__(self, data, info):
        self.data, self.info = data, info


def _ingest_host(file: str, sr: int, decode_on_device: bool = False):
    """Host half of the device-side ingest (thread-safe; the FLAC decoder releases the GIL): the stored PCM of a WAV / FLAC
    file as (pcm, rate, bits).  Everything the native route does not take — another container (an ID3-tagged MP3 included), a
    WAV / FLAC the native readers refuse (an encoding they do not know, a stream that fails its checks), more than 8
    channels — goes the way `load_audio(file, sr)` goes, ffmpeg first, and comes back as samples.
    `decode_on_device`: a FLAC file the device decoder takes (4 - 24 bits per sample, a sample count in STREAMINFO, a first
    frame inside the file) is only read here, and comes back as a `_FlacFile`."""
    kind, parsed = _sniff(file), None
    if decode_on_device and kind == "flac":
        with open(file, "rb") as f:
            data = bytearray(os.fstat(f.fileno()).st_size)
            data = data[: f.readinto(data)]
        info = parse_flac_info(data)
        if (info is not None and info.bits_per_sample <= 24 and info.total_samples > 0 and info.channels <= MAX_DEVICE_CHANNELS
                and info.first_frame < len(data)):
            return _FlacFile(data, info)
    if kind == "wav":
        parsed = _parse_wav(file)
    elif kind == "flac":
        try:
            parsed = _parse_flac(file)
        except RuntimeError:                              # the host route decides: ffmpeg may read it, else it raises the same
            parsed = None
    if parsed is not None and 1 <= parsed[0].shape[1] <= MAX_DEVICE_CHANNELS:
        return parsed
    return load_audio(file, sr)


def _ingest_device(staged, file: str, sr: int, device: torch.device) -> torch.Tensor:
    """Device half: upload the PCM in its stored width, then down-mix + resample + quantise in one kernel (hip.resample) on
    the calling thread's current stream; samples that came from the host route are uploaded as they are.  A `_FlacFile` is
    uploaded as the bytes it is and decoded there (hip.flac_decode_device); its int32 PCM goes into the same hip.resample.
    Whatever the device decoder refuses or rejects is handed to `_ingest_host`: the host decoder decides, or raises."""
    if isinstance(staged, _FlacFile):
        info = staged.info
        rc, pcm, _ = hip.flac_decode_device(torch.frombuffer(staged.data, dtype=torch.uint8).to(device), info)
        if rc == 0:
            try:
                return hip.resample(pcm, info.sample_rate, sr, info.bits_per_sample)
            except hip.HipLimitError:
                staged = load_audio(file, sr)
        else:
            staged = _ingest_host(file, sr)
    if isinstance(staged, tuple):
        pcm, rate, bits = staged
        try:
            pcm = np.require(pcm, requirements=["C", "A", "W"])     # a copy only for a sample array at an odd file offset
            return hip.resample(torch.from_numpy(pcm).to(device), rate, sr, bits)
        except hip.HipLimitError:                         # a rate pair whose filter the kernel does not take
            staged = load_audio(file, sr)
    return torch.from_numpy(staged).to(device)


def ingest_options(device_ingest) -> Optional[dict]:
    """`device_ingest` of the entry points -> the keywords `load_audio(path, device=model.device, ...)` gets beyond `device`:
    None for False (host ingest), {} for True, {"decode_on_device": True} for "decode" (FLAC files are decoded on the GPU
    as well)."""
    if isinstance(device_ingest, str):
        if device_ingest != "decode":
            raise ValueError(f'device_ingest must be False, True or "decode" (got {device_ingest!r})')
        return {"decode_on_device": True}
    return {} if device_ingest else None


def load_audio(file: str, sr: int = SAMPLE_RATE, device: Optional[Union[str, torch.device]] = None,
               decode_on_device: bool = False):
    """Decode `file` to mono float32 at `sr` Hz.  Same contract as the reference (audio.py:25-62): ffmpeg does
    the decoding / down-mixing / resampling; a RuntimeError is raised when it fails.  When the ffmpeg binary
    does not exist, RIFF/WAVE files are read natively and FLAC files through the native decoder of
    csrc/flac_decode.c (frame CRCs and the stream's MD5 signature are verified).

    `device` (a GPU; no counterpart in the reference): the result is a torch.float32 tensor on that device, and WAV / FLAC
    files never touch ffmpeg or scipy — they are parsed natively, the stored PCM is uploaded and one HIP kernel
    (csrc/resample.hip) does the down-mix, the polyphase resampling and the 16-bit quantisation in float64.  It evaluates the
    same filter as the NATIVE host route (scipy's resample_poly, taken when ffmpeg is absent), which accumulates in float32:
    those two agree to one 16-bit step, on all but about 0.1 % of the samples exactly.  Against ffmpeg's own
    resampler — the host route where ffmpeg is installed — no bound is claimed or has been measured: it is a different
    filter, as it always was for the native route.  Other containers, WAV / FLAC files the native readers refuse, files with
    more than 8 channels and rate pairs whose filter the kernel does not take go the host route (ffmpeg first) and are
    uploaded.  hip.HipError without a GPU.

    `decode_on_device` (with `device`; opt-in): a FLAC file is not decoded on the host either.  Its bytes are uploaded and
    csrc/flac.hip decodes it there, one lane per frame, to the int32 PCM the host decoder produces, bit for bit — so the
    result equals the one without the flag.  The one difference: this route verifies every frame's CRC-8 and CRC-16, the
    unbroken chain of frames and the sample count, but not the STREAMINFO MD5 signature.  What it does not take (32-bit
    FLAC, a stream without a sample count) or rejects goes to the host decoder exactly as without the flag."""
    if device is not None:
        device = torch.device(device)
        hip.require_gpu(device)
        if decode_on_device:
            return _ingest_device(_ingest_host(file, sr, True), file, sr, device)
        return _ingest_device(_ingest_host(file, sr), file, sr, device)
    cmd = ["ffmpeg", "-nostdin", "-threads", "0", "-i", file, "-f", "s16le", "-ac", "1",
           "-acodec", "pcm_s16le", "-ar", str(sr), "-"]
    try:
        out = subprocess.run(cmd, capture_output=True, check=True).stdout
    except FileNotFoundError:
        wav = None
        if os.path.isfile(file):
            wav = _read_wav(file, sr)
            if wav is None:
                wav = _read_flac(file, sr)
        if wav is None:
            raise RuntimeError("Failed to load audio: ffmpeg is not installed and the file is neither RIFF/WAVE nor FLAC")
        return wav
    except subprocess.CalledProcessError as e:
        raise RuntimeError(f"Failed to load audio: {e.stderr.decode()}") from e
    return np.frombuffer(out, np.int16).flatten().astype(np.float32) / 32768.0


def pad_or_trim(array, length: int = N_SAMPLES, *, axis: int = -1):
    """Zero-pad or cut `array` along `axis` to exactly `length` entries (audio.py:65-88); numpy or torch."""
    n = array.shape[axis]
    if torch.is_tensor(array):
        if n > length:
            array = array.narrow(axis, 0, length)
        elif n < length:
            pads = [0, 0] * array.ndim
            pads[2 * (array.ndim - 1 - (axis % array.ndim)) + 1] = length - n
            array = F.pad(array, pads)
        return array
    if n > length:
        array = array.take(indices=range(length), axis=axis)
    elif n < length:
        widths = [(0, 0)] * array.ndim
        widths[axis] = (0, length - n)
        array = np.pad(array, widths)
    return array


def _slaney_mel_matrix(n_mels: int) -> np.ndarray:
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels=n_mels) recomputed (Slaney scale + area norm): the
    matrix the reference ships as assets/mel_filters.npz (audio.py:92-107).  Agrees with the asset to ~4e-9."""
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)

    def to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    bins = np.linspace(0, SAMPLE_RATE / 2, 1 + N_FFT // 2)
    edges = to_hz(np.linspace(to_mel(0.0), to_mel(SAMPLE_RATE / 2.0), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - bins[None, :]
    rising = -ramps[:-2] / width[:-1, None]
    falling = ramps[2:] / width[1:, None]
    tri = np.maximum(0.0, np.minimum(rising, falling))
    tri *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return tri.astype(np.float32)


@lru_cache(maxsize=None)
def mel_filters(device, n_mels: int) -> torch.Tensor:
    assert n_mels in {80, 128}, f"Unsupported n_mels: {n_mels}"
    return torch.from_numpy(_slaney_mel_matrix(n_mels)).to(device)


def log_mel_spectrogram(audio: Union[str, np.ndarray, torch.Tensor], n_mels: int = 80, padding: int = 0,
                        device: Optional[Union[str, torch.device]] = None) -> torch.Tensor:
    """(n_mels, n_frames) log-mel spectrogram, computed on the GPU by the HIP kernel.

    Same arguments as the reference (audio.py:110-115).  `device=None` keeps a GPU tensor where it is and
    sends host audio to the current GPU; the result lives on that GPU (the reference leaves it on the
    audio's device).  The global `max - 8` clamp spans the whole input, batched input included, exactly
    like audio.py:155."""
    if not torch.is_tensor(audio):
        if isinstance(audio, str):
            audio = load_audio(audio)
        audio = torch.from_numpy(np.ascontiguousarray(audio))
    if device is not None:
        audio = audio.to(device)
    elif not audio.is_cuda:
        if not torch.cuda.is_available():
            raise hip.HipError("log_mel_spectrogram: no ROCm GPU visible (whisper_amd has no CPU path)")
        audio = audio.to("cuda")
    hip.require_gpu(audio.device)
    audio = audio.float()
    if padding > 0:
        audio = F.pad(audio, (0, padding))
    lead = audio.shape[:-1]
    flat = audio.reshape(-1, audio.shape[-1]) if audio.dim() != 1 else audio
    out = hip.log_mel(flat, mel_filters(audio.device, n_mels))
    return out.reshape(*lead, n_mels, out.shape[-1]) if audio.dim() > 2 else out
