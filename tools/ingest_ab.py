"""Audio ingest on the host against ingest on the device, and what it does to ONE long file end to end.

Writes the signal of tools/chunked_ab.py (bursts of 3 - 12 s separated by gaps) as a 44.1 kHz and as a 48 kHz stereo 16-bit
WAV, and its first 20 s as a 24-bit stereo FLAC, then reports in one process:
  * the host stage: `load_audio(path)` (ffmpeg if the box has it, else the native reader + numpy down-mix + scipy
    resample_poly + quantisation, one thread);
  * the device stage `load_audio(path, device=gpu)` split into parse (host clock), upload and kernel (HIP events on the
    current stream), and as a whole (host clock around a call that ends in a synchronise);
  * `transcribe_chunked(path)` wall time with `device_ingest` off and on: large-v3 dimensions, synthetic weights, fp16,
    the settings of chunked_ab.py.  `device_ingest=False` is what the entry point did before the option existed.
  * the FLAC legs (`legs` = "flac" or "all"): the whole signal at 44.1 kHz stereo as a 16-bit and as a 24-bit FLAC
    (tests/flac_writer.py: encode_stream_fast), ingested three ways — on the host, with `device_ingest=True` (host decoder,
    device resampler) and with `device_ingest="decode"` (csrc/flac.hip) — each split into file read / decode / upload /
    resample, and `transcribe_chunked` end to end for the three.  The decode leg of the new route is held against
    wh_flac_decode of `base_audio_lib` on the same bytes in the same run: build that library from the parent commit's
    csrc/flac_decode.c (default: the current library, which says nothing about a change to the host decoder).
Every leg runs once untimed, then `repeats` times; medians and the spread (max - min over min) are printed.

    python tools/ingest_ab.py [minutes=20] [sample_len=64] [batch_size=24] [repeats=5] [legs=wav|flac|all] [base_audio_lib]
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
legs = sys.argv[5] if len(sys.argv) > 5 else "wav"
base_audio_lib = sys.argv[6] if len(sys.argv) > 6 else None
assert legs in ("wav", "flac", "all"), legs
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


def host_decoder(path_or_none):
    """wh_flac_decode of a libwhisper_audio.so (None: the one the package loads) as bytes -> seconds"""
    import ctypes as C
    lib = A._audio_lib() if path_or_none is None else C.CDLL(path_or_none)
    lib.wh_flac_decode.restype = C.c_int
    lib.wh_flac_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.wh_flac_free.restype, lib.wh_flac_free.argtypes = None, [C.POINTER(C.c_int32)]

    def run(data: bytes) -> float:
        ptr, n, ch, rate, bps = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
        t0 = time.perf_counter()
        rc = lib.wh_flac_decode(data, len(data), C.byref(ptr), C.byref(n), C.byref(ch), C.byref(rate), C.byref(bps))
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        lib.wh_flac_free(ptr)
        return dt
    return run


def decode_stages(path: str):
    """one `decode_on_device` ingest with its stages timed apart: (file read s, upload s, decode s, resample s, candidates,
    chained frames)"""
    t0 = time.perf_counter()
    staged = A._ingest_host(path, A.SAMPLE_RATE, True)
    read = time.perf_counter() - t0
    assert isinstance(staged, A._FlacFile), "the device decoder does not take this file"
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    d = torch.frombuffer(staged.data, dtype=torch.uint8).to(dev)
    ev[1].record()
    rc, pcm, st = hip.flac_decode_device(d, staged.info)
    ev[2].record()
    assert rc == 0, rc
    hip.resample(pcm, staged.info.sample_rate, A.SAMPLE_RATE, staged.info.bits_per_sample)
    ev[3].record()
    torch.cuda.synchronize()
    return (read,) + tuple(ev[i].elapsed_time(ev[i + 1]) / 1e3 for i in range(3)) + (st[0], st[1])


def flac_legs(path: str, label: str, seconds: float):
    with open(path, "rb") as f:
        data = f.read()
    base, new = host_decoder(base_audio_lib), host_decoder(None)
    t = {k: [] for k in ("base", "new", "host", "true", "decode")}
    true_parts, dec_parts = [], []
    for rep in range(repeats + 1):                                       # rep 0 untimed
        row = dict(base=base(data), new=new(data), host=timed(lambda: A.load_audio(path))[0],
                   true=timed(lambda: A.load_audio(path, device=dev))[0],
                   decode=timed(lambda: A.load_audio(path, device=dev, decode_on_device=True))[0])
        tp, dp = stages(path), decode_stages(path)
        if rep:
            for k, v in row.items():
                t[k].append(v)
            true_parts.append(tp)
            dec_parts.append(dp)
    assert torch.equal(A.load_audio(path, device=dev, decode_on_device=True), A.load_audio(path, device=dev))
    m = {k: stats(v) for k, v in t.items()}
    tpm = [stats([p[i] for p in true_parts]) for i in range(3)]
    dpm = [stats([p[i] for p in dec_parts]) for i in range(4)]
    which = "the parent commit's build" if base_audio_lib else "the current library"
    print(f"{label} ({len(data) / 1e6:.1f} MB, {dec_parts[0][4]} frame candidates, {dec_parts[0][5]} chained): host decoder of {which} "
          f"{1e3 * m['base'][0]:.1f} ms (spread {m['base'][1]:.1f} %), host decoder of this tree {1e3 * m['new'][0]:.1f} ms "
          f"(spread {m['new'][1]:.1f} %)", flush=True)
    print(f"{label}: host ingest {1e3 * m['host'][0]:.1f} ms ({seconds / m['host'][0]:.0f} audio-s/s, spread {m['host'][1]:.1f} %) | "
          f"device_ingest=True {1e3 * m['true'][0]:.1f} ms ({seconds / m['true'][0]:.0f} audio-s/s, spread {m['true'][1]:.1f} %) = "
          f"read + host decode {1e3 * tpm[0][0]:.1f} + upload {1e3 * tpm[1][0]:.1f} + resample {1e3 * tpm[2][0]:.2f} ms "
          f"(spreads {tpm[0][1]:.0f} / {tpm[1][1]:.0f} / {tpm[2][1]:.0f} %) | device_ingest=\"decode\" {1e3 * m['decode'][0]:.1f} ms "
          f"({seconds / m['decode'][0]:.0f} audio-s/s, spread {m['decode'][1]:.1f} %) = read {1e3 * dpm[0][0]:.1f} + upload "
          f"{1e3 * dpm[1][0]:.1f} + decode {1e3 * dpm[2][0]:.1f} + resample {1e3 * dpm[3][0]:.2f} ms (spreads {dpm[0][1]:.0f} / "
          f"{dpm[1][1]:.0f} / {dpm[2][1]:.0f} / {dpm[3][1]:.0f} %)", flush=True)
    gain, both = m["base"][0] / dpm[2][0], m["base"][1] + dpm[2][1]
    print(f"{label}: decode leg, host {1e3 * m['base'][0]:.1f} ms vs device {1e3 * dpm[2][0]:.1f} ms: {gain:.2f} x; the two spreads "
          f"together are {both:.1f} %, so the device leg is {'FASTER' if gain > 1 + both / 100 else 'NOT faster'} beyond them", flush=True)


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

    flacs = []
    if legs in ("flac", "all"):
        from flac_writer import encode_stream_fast
        stereo = render(x, 44100)
        for bps in (16, 24):
            path = os.path.join(td, f"long_s{bps}.flac")
            with open(path, "wb") as f:
                f.write(encode_stream_fast(np.round(stereo * (1 << (bps - 1)) * 0.99).astype(np.int32), 44100, bps))
            flacs.append((path, f"44100 Hz stereo s{bps} FLAC"))
        for path, label in flacs:
            flac_legs(path, f"{seconds:.0f} s, {label}", seconds)
        for path, label in flacs:
            times = {False: [], True: [], "decode": []}
            for rep in range(repeats + 1):
                for on in (False, True, "decode"):
                    t, out = timed(lambda: model.transcribe_chunked(path, batch_size=batch_size, device_ingest=on, **kw))
                    if rep:
                        times[on].append(t)
            line = ", ".join(f"device_ingest={on!r} median {stats(v)[0]:.3f} s ({seconds / stats(v)[0]:.1f} audio-s/s, spread "
                             f"{stats(v)[1]:.1f} %)" for on, v in times.items())
            print(f"transcribe_chunked, {label}: {line}", flush=True)
    if legs == "flac":
        files = []

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
