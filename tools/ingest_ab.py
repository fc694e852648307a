"""Audio ingest on the host against ingest on the device, and what it does to ONE long file end to end.

Writes the signal of tools/chunked_ab.py (bursts of 3 - 12 s separated by gaps) as a 44.1 kHz and as a 48 kHz stereo 16-bit
WAV, and its first 20 s as a 24-bit stereo FLAC, then reports in one process:
  * the host stage: `load_audio(path)` (ffmpeg if the box has it, else the native reader + numpy down-mix + scipy
    resample_poly + quantisation, one thread);
  * the device stage `load_audio(path, device=gpu)` split into parse (host clock), upload and kernel (HIP events on the
    current stream), and as a whole (host clock around a call that ends in a synchronise);
  * `transcribe_chunked(path)` wall time with `device_ingest` off and on: large-v3 dimensions, synthetic weights, fp16,
    the settings of chunked_ab.py.  `device_ingest=False` is what the entry point did before the option existed.
Every leg runs once untimed, then `repeats` times; medians and the spread (max - min over min) are printed.

    python tools/ingest_ab.py [minutes=20] [sample_len=64] [batch_size=24] [repeats=5]
"""
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chunk_oracle import make_signal                                     # noqa: E402
from whisper_amd import audio as A                                       # noqa: E402
from whisper_amd import hip                                              # noqa: E402
from whisper_amd.model import ModelDimensions, Whisper                   # noqa: E402
from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict   # noqa: E402

minutes = float(sys.argv[1]) if len(sys.argv) > 1 else 20.0
sample_len = int(sys.argv[2]) if len(sys.argv) > 2 else 64
batch_size = int(sys.argv[3]) if len(sys.argv) > 3 else 24
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
assert torch.cuda.is_available(), "ingest_ab.py measures on the GPU"
dev = torch.device("cuda:0")


def render(x16k: np.ndarray, rate: int) -> np.ndarray:
    """the 16 kHz signal at `rate`, stereo (linear interpolation: the content only has to be the same for both routes)"""
    n = int(len(x16k) * rate / 16000)
    left = np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(x16k)), x16k)
    right = 0.8 * left + 0.01 * np.random.default_rng(rate).standard_normal(n)
    return np.stack([left, right], axis=1)


def write_wav(path: str, x: np.ndarray, rate: int) -> None:
    with wave.open(path, "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2").tobytes())


def stats(ts):
    return float(np.median(ts)), 100.0 * (max(ts) - min(ts)) / max(min(ts), 1e-12)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stages(path: str):
    """one device ingest with its three stages timed apart: (parse s, upload s, kernel s)"""
    t0 = time.perf_counter()
    pcm, rate, bits = A._ingest_host(path, A.SAMPLE_RATE)
    parse = time.perf_counter() - t0
    pcm = np.require(pcm, requirements=["C", "A", "W"])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    d = torch.from_numpy(pcm).to(dev)
    ev[1].record()
    hip.resample(d, rate, A.SAMPLE_RATE, bits)
    ev[2].record()
    torch.cuda.synchronize()
    return parse, ev[0].elapsed_time(ev[1]) / 1e3, ev[1].elapsed_time(ev[2]) / 1e3


def ingest_legs(path: str, label: str, seconds: float):
    host, whole, parts = [], [], []
    for rep in range(repeats + 1):                                       # rep 0 untimed: page cache, filter upload, first launch
        h, _ = timed(lambda: A.load_audio(path))
        w, _ = timed(lambda: A.load_audio(path, device=dev))
        p = stages(path)
        if rep:
            host.append(h)
            whole.append(w)
            parts.append(p)
    (hm, hs), (wm, ws) = stats(host), stats(whole)
    pm = [stats([p[i] for p in parts]) for i in range(3)]
    print(f"{label}: host ingest {1e3 * hm:8.1f} ms ({seconds / hm:8.0f} audio-s/s, spread {hs:.1f} %) | device ingest "
          f"{1e3 * wm:8.1f} ms ({seconds / wm:8.0f} audio-s/s, spread {ws:.1f} %) = parse {1e3 * pm[0][0]:.1f} + upload "
          f"{1e3 * pm[1][0]:.1f} + kernel {1e3 * pm[2][0]:.2f} ms (spreads {pm[0][1]:.0f} / {pm[1][1]:.0f} / {pm[2][1]:.0f} %) | "
          f"host / device {hm / wm:.1f} x", flush=True)


dims = dims_for("large-v3")
model = Whisper(ModelDimensions(**dims_dict(dims)), synthetic_state_dict(dims, seed=0, device=dev), device=dev)
x, _ = make_signal(gap_noise=1e-4, n_bursts=int(minutes * 60 / 8.8))
seconds = len(x) / 16000.0
kw = dict(language="en", temperature=0.0, fp16=True, sample_len=sample_len, no_speech_threshold=None, logprob_threshold=None,
          compression_ratio_threshold=None)
print(f"large-v3 dims (synthetic weights, fp16), {seconds:.0f} s of audio, sample_len {sample_len}, batch_size {batch_size}, "
      f"{repeats} repeats; ffmpeg {'present: the host stage is ffmpeg' if shutil.which('ffmpeg') else 'absent: the host stage is the native reader + scipy'}",
      flush=True)

with tempfile.TemporaryDirectory() as td:
    files = []
    for rate in (44100, 48000):
        path = os.path.join(td, f"long_{rate}.wav")
        write_wav(path, render(x, rate), rate)
        files.append((path, f"{rate} Hz stereo s16 WAV"))
    try:
        from test_audio_io import write_flac                             # the tests' small FLAC writer (pure Python: 20 s only)
        head = render(x[: 16000 * 20], 44100)
        flac = os.path.join(td, "head.flac")
        with open(flac, "wb") as f:
            f.write(write_flac(np.round(head * 8388608.0 * 0.99).astype(np.int32), 44100, 24, 32768, lambda fi: (1, ["verbatim"] * 2)))
        ingest_legs(flac, "20 s, 44100 Hz stereo s24 FLAC", 20.0)
    except Exception as e:                                               # noqa: BLE001 — the FLAC leg is optional
        print(f"FLAC leg skipped: {type(e).__name__}: {e}", flush=True)

    for path, label in files:
        ingest_legs(path, f"{seconds:.0f} s, {label}", seconds)

    for path, label in files:
        times = {False: [], True: []}
        for rep in range(repeats + 1):                                   # rep 0 untimed: every shape of both legs
            for on in (False, True):
                t, out = timed(lambda: model.transcribe_chunked(path, batch_size=batch_size, device_ingest=on, **kw))
                if rep:
                    times[on].append(t)
                    print(f"run {rep} {label} device_ingest={on!s:5}: {t:7.3f} s wall, {seconds / t:7.1f} audio-s/s, "
                          f"{len(out['chunks'])} chunks", flush=True)
        (fm, fs), (nm, ns) = stats(times[False]), stats(times[True])
        print(f"transcribe_chunked, {label}: device_ingest=False median {fm:.3f} s ({seconds / fm:.1f} audio-s/s, spread {fs:.1f} %), "
              f"device_ingest=True median {nm:.3f} s ({seconds / nm:.1f} audio-s/s, spread {ns:.1f} %): {fm / nm:.2f} x", flush=True)
