"""Device-side audio ingest, the parts that need no GPU (DESIGN.md §5b "Device-side ingest"): the float64 restatement
(tests/resample_oracle.py) against scipy, audio.resample_taps against the restatement, the C ABI of wh_resample, and the
split of the native readers into parse + convert leaving load_audio's result bit for bit what it was."""
import ctypes as C
import os
import re
import subprocess
import wave

import numpy as np
import pytest
import torch

import resample_oracle as R
from whisper_amd import audio as A
from whisper_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JFK = os.path.join(ROOT, "tests", "golden", "jfk_head.flac")
RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000, 12345)          # 12345 -> 16000: up 3200, down 2469


@pytest.mark.parametrize("rate", RATES)
def test_restatement_equals_scipy(rate):
    """the restatement IS scipy.signal.resample_poly with its default window, in float64: equal lengths, < 1e-12"""
    signal = pytest.importorskip("scipy.signal")
    x = R.signal(5 * rate + 17, 1, rate, seed=rate)[:, 0]
    up, down = R.ratio(rate, 16000)
    want = signal.resample_poly(x, up, down)
    got = R.resample(x, rate, 16000)
    assert got.dtype == np.float64 and got.shape == want.shape == (-(-len(x) * up // down),)
    assert np.abs(got - want).max() < 1e-12


def test_restatement_short_inputs_and_identity():
    signal = pytest.importorskip("scipy.signal")
    for rate in RATES:
        up, down = R.ratio(rate, 16000)
        for n in (1, 7, 26):
            x = R.signal(n, 1, rate, seed=n)[:, 0]
            want = signal.resample_poly(x, up, down)
            got = R.resample(x, rate, 16000)
            assert got.shape == want.shape and np.abs(got - want).max() < 1e-12, (rate, n)
    x = R.signal(100, 1, 16000, seed=1)[:, 0]
    assert np.array_equal(R.resample(x, 16000, 16000), x)


@pytest.mark.parametrize("rate", RATES)
def test_resample_taps(rate):
    want, half = R.taps(rate, 16000)
    got = A.resample_taps(rate, 16000)
    up, _ = R.ratio(rate, 16000)
    assert got.dtype == np.float64 and got.shape == (2 * half + 1,)
    assert np.abs(got - want).max() < 1e-15
    assert abs(got.sum() - up) < 1e-12
    assert not got.flags.writeable                                        # cached: nobody edits it
    assert np.array_equal(got, got[::-1])                                 # linear phase


def test_resample_taps_same_rate_and_other_targets():
    assert A.resample_taps(16000, 16000).tolist() == [1.0]
    assert np.abs(A.resample_taps(16000, 8000) - R.taps(16000, 8000)[0]).max() < 1e-15


def test_wh_resample_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+wh_resample\s*\(", code)
    for i, name in enumerate(("WH_PCM_U8", "WH_PCM_S16", "WH_PCM_S32", "WH_PCM_F32", "WH_PCM_F64")):
        assert re.search(rf"\b{name}\s*=\s*{i}\b", code) and getattr(hip, name) == i
    limit = re.search(r"#define\s+WH_RESAMPLE_MAX_TAPS\s+\(1\s*<<\s*(\d+)\)", code)
    assert limit and hip.RESAMPLE_MAX_TAPS == 1 << int(limit.group(1))
    assert "wh_resample" in hip.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", hip.lib_path()], check=True, capture_output=True, text=True).stdout
    assert "wh_resample" in [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert re.search(r"^KERNELS\s*\+?=.*\bresample\b", open(os.path.join(ROOT, "whisper_amd", "csrc", "Makefile")).read(), re.M)
    assert "wh_resample" not in open(os.path.join(ROOT, "include", "whisper_audio.h")).read()


def test_wh_resample_refuses_bad_arguments_without_gpu():
    """status 1 before any device work: null pointers, channels outside 1 - 8, up / down < 1 or not coprime, a wrong n_out,
    an unknown format, bits outside the format's range; status 5 for a filter beyond the compiled-in limits; an empty input
    succeeds"""
    lib = hip.lib()
    p = C.c_void_p(1 << 20)                                               # never dereferenced: every call below returns first
    S16 = hip.WH_PCM_S16

    def call(pcm=p, fmt=S16, bits=16, ch=2, n=441, taps=p, up=160, down=441, half=4410, out=p, n_out=160):
        return lib.wh_resample(pcm, fmt, bits, ch, n, taps, up, down, half, out, n_out, None)
    assert call(pcm=None) == 1 and call(taps=None) == 1 and call(out=None) == 1
    assert call(ch=0) == 1 and call(ch=9) == 1
    assert call(up=0) == 1 and call(down=0) == 1 and call(up=-160) == 1
    assert call(up=320, down=882, half=8820) == 1                         # not in lowest terms
    assert call(n_out=159) == 1 and call(n_out=161) == 1 and call(n=442) == 1      # n_out != ceil(n * up / down)
    assert call(n=-1, n_out=0) == 1
    assert call(fmt=5) == 1 and call(fmt=-1) == 1
    assert call(bits=17) == 1 and call(bits=0) == 1
    assert call(fmt=hip.WH_PCM_S32, bits=33) == 1 and call(fmt=hip.WH_PCM_U8, bits=16) == 1
    assert call(half=-1) == 1
    assert call(half=hip.RESAMPLE_MAX_TAPS // 2) == 5                     # 2 half + 1 taps: one more than the limit
    assert call(up=1, down=4000, half=40000, n=4000, n_out=1) == 5        # one output's span of input exceeds a workgroup's LDS
    assert call(n=0, n_out=0) == 0                                        # nothing to do, nothing written
    assert b"limit" in lib.wh_status_string(5)


def _no_ffmpeg(monkeypatch):
    def run(*a, **k):
        raise FileNotFoundError("ffmpeg")
    monkeypatch.setattr(subprocess, "run", run)


def _write_wav(path, pcm, rate, width, channels=2):
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def test_load_audio_is_the_parse_plus_the_host_path(tmp_path, monkeypatch):
    """load_audio(path) without `device` returns exactly _to_mono_s16 of the parsed PCM (the readers were split into parse +
    convert; nothing else changed), for a 44.1 kHz stereo WAV, the other stored widths and the head of jfk.flac"""
    pytest.importorskip("scipy")
    _no_ffmpeg(monkeypatch)
    x = R.signal(44100 + 17, 2, 44100, seed=3)
    pcm, _ = R.store(x, "s16")
    path = str(tmp_path / "a.wav")
    _write_wav(path, pcm.astype("<i2"), 44100, 2)
    parsed, rate, bits = A._parse_wav(path)
    assert (rate, bits) == (44100, 16) and parsed.dtype == np.int16 and np.array_equal(parsed, pcm)
    got = A.load_audio(path)
    want = A._to_mono_s16(pcm.astype(np.float32) / 32768.0, 44100, 16000)           # what the reader did before the split
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got, A._to_mono_s16(A._pcm_to_float(parsed, bits), rate, 16000))

    pcm8, _ = R.store(x, "u8")
    path8 = str(tmp_path / "b.wav")
    _write_wav(path8, pcm8, 44100, 1)
    parsed8, _, bits8 = A._parse_wav(path8)
    assert parsed8.dtype == np.uint8 and bits8 == 8 and np.array_equal(parsed8, pcm8)
    want8 = A._to_mono_s16((pcm8.astype(np.float32) - 128.0) / 128.0, 44100, 16000)
    assert np.array_equal(A.load_audio(path8), want8)

    pcm24, _ = R.store(x, "s24")
    path24 = str(tmp_path / "c.wav")
    raw = pcm24.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(len(pcm24), -1)
    _write_wav(path24, raw, 44100, 3)
    parsed24, _, bits24 = A._parse_wav(path24)
    assert parsed24.dtype == np.int32 and bits24 == 24 and np.array_equal(parsed24, pcm24)
    want24 = A._to_mono_s16(pcm24.astype(np.float32) / 8388608.0, 44100, 16000)
    assert np.array_equal(A.load_audio(path24), want24)

    with open(JFK, "rb") as f:
        fpcm, frate, fbps = A.decode_flac(f.read())
    got = A.load_audio(JFK)
    want = A._to_mono_s16(fpcm.astype(np.float32) / float(1 << (fbps - 1)), frate, 16000)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    parsed = A._parse_flac(JFK)
    assert np.array_equal(parsed[0], fpcm) and parsed[1:] == (frate, fbps)
    assert A._parse_flac(path) is None and A._parse_wav(JFK) is None


def test_device_ingest_keywords_exist(monkeypatch):
    """`device_ingest` (default False) on the batch entry points; `transcribe` keeps the reference's parameter list and takes
    it among its keywords without handing it on to DecodingOptions; `audio.load_audio` has `device`, the package-level
    `load_audio` stays the reference's (file, sr)"""
    import inspect

    import whisper_amd
    from whisper_amd import launcher
    import importlib
    T = importlib.import_module("whisper_amd.transcribe")          # (the package attribute of that name is the function)
    for fn in (whisper_amd.transcribe_batch, whisper_amd.transcribe_chunked, launcher.transcribe_sharded):
        assert inspect.signature(fn).parameters["device_ingest"].default is False, fn.__name__
    assert inspect.signature(A.load_audio).parameters["device"].default is None
    assert list(inspect.signature(whisper_amd.load_audio).parameters) == ["file", "sr"]
    seen = {}

    def run(self, audio, mel=None):
        seen.update(options=dict(self.decode_options), audio=audio)
        return {}
    monkeypatch.setattr(T._Transcriber, "run", run)
    x = np.zeros(16000, dtype=np.float32)
    for flag in (False, True):
        whisper_amd.transcribe(None, x, device_ingest=flag, language="en")
        assert seen["options"] == {"language": "en"} and seen["audio"] is x      # arrays are untouched by the option


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_device_ingest_needs_a_gpu(tmp_path):
    with pytest.raises(hip.HipError):
        A.load_audio(JFK, device="cuda")
    with pytest.raises(hip.HipError):
        A.load_audio(JFK, device="cpu")
    with pytest.raises(hip.HipError):
        hip.resample(torch.zeros(10, 2, dtype=torch.int16), 44100)
    from whisper_amd.transcribe import _load_all
    with pytest.raises(hip.HipError):
        _load_all([JFK], torch.device("cuda"))


# ---- what the native route does not take goes the host route -------------------------------------------------------------
def _fake_ffmpeg(monkeypatch, calls):
    """an `ffmpeg` that answers every file with 100 samples of value 7 (s16le), and records the files it was asked for"""
    class Done:
        stdout = np.full(100, 7, dtype="<i2").tobytes()

    def run(cmd, **k):
        assert cmd[0] == "ffmpeg"
        calls.append(cmd[cmd.index("-i") + 1])
        return Done()
    monkeypatch.setattr(subprocess, "run", run)


def test_device_route_falls_back_to_the_host_route(tmp_path, monkeypatch):
    """_ingest_host hands on stored PCM only for what the native route takes.  An ID3-tagged file that is no FLAC (an MP3), a
    9-channel WAV, a WAV encoding the reader does not know, a FLAC the decoder refuses and a missing file all reach
    `load_audio(file, sr)` — ffmpeg where it exists — and come back as samples; with no ffmpeg the host route's own error
    is raised.  A rate pair the kernel refuses (HipLimitError) falls back in _ingest_device."""
    import struct
    mp3 = str(tmp_path / "song.mp3")
    open(mp3, "wb").write(b"ID3\x04\x00\x00\x00\x00\x00\x10" + b"\0" * 16 + b"\xff\xfb\x90\x00" + b"\0" * 400)
    wide = str(tmp_path / "wide.wav")
    _write_wav(wide, np.zeros((50, 9), dtype="<i2"), 44100, 2, channels=9)
    adpcm = str(tmp_path / "adpcm.wav")
    body = b"fmt " + struct.pack("<IHHIIHH", 16, 2, 1, 16000, 8000, 256, 4) + b"data" + struct.pack("<I", 64) + b"\0" * 64
    open(adpcm, "wb").write(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body)
    broken = str(tmp_path / "broken.flac")
    data = bytearray(open(JFK, "rb").read())
    data[len(data) // 2] ^= 0x40
    open(broken, "wb").write(bytes(data))
    tagged = str(tmp_path / "tagged.flac")                                 # an ID3v2 tag in front of a real FLAC stream: native
    open(tagged, "wb").write(b"ID3\x04\x00\x00\x00\x00\x00\x10" + b"\0" * 16 + open(JFK, "rb").read())
    stereo = str(tmp_path / "ok.wav")
    _write_wav(stereo, np.zeros((50, 2), dtype="<i2"), 44100, 2)
    assert [A._sniff(p) for p in (mp3, wide, adpcm, broken, tagged, stereo, JFK, str(tmp_path / "missing"))] == \
        [None, "wav", "wav", "flac", "flac", "wav", "flac", None]

    calls = []
    _fake_ffmpeg(monkeypatch, calls)
    want = np.full(100, 7 / 32768.0, dtype=np.float32)
    for path in (mp3, wide, adpcm, broken, str(tmp_path / "missing")):
        got = A._ingest_host(path, 16000)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want), path
    assert calls == [mp3, wide, adpcm, broken, str(tmp_path / "missing")]
    for path, shape in ((tagged, (16 * 4608, 2)), (JFK, (16 * 4608, 2)), (stereo, (50, 2))):
        pcm, rate, bits = A._ingest_host(path, 16000)                      # native: ffmpeg is not asked
        assert pcm.shape == shape and rate == 44100
    assert len(calls) == 5

    # the device half: samples from the host route are uploaded as they are; a refused rate pair goes back to the host route
    cpu = torch.device("cpu")                                              # stands in for the GPU: nothing here launches
    assert torch.equal(A._ingest_device(want, mp3, 16000, cpu), torch.from_numpy(want))
    seen = []

    def refuse(pcm, rate, sr, bits):
        seen.append((tuple(pcm.shape), rate, sr, bits))
        raise hip.HipLimitError("filter too long")
    monkeypatch.setattr(hip, "resample", refuse)
    got = A._ingest_device(A._ingest_host(stereo, 16000), stereo, 16000, cpu)
    assert seen == [((50, 2), 44100, 16000, 16)] and calls[-1] == stereo and torch.equal(got, torch.from_numpy(want))
    monkeypatch.setattr(hip, "require_gpu", lambda device: None)
    assert torch.equal(A.load_audio(mp3, device=cpu), torch.from_numpy(want)) and calls[-1] == mp3
    from whisper_amd.transcribe import _load_all
    out = _load_all([mp3, want, wide], cpu)
    assert torch.equal(out[0], torch.from_numpy(want)) and out[1] is want and torch.equal(out[2], torch.from_numpy(want))

    # no ffmpeg: the host route's own errors, not a crash of the sniffing
    _no_ffmpeg(monkeypatch)
    for path in (mp3, adpcm, broken, str(tmp_path / "missing")):
        with pytest.raises(RuntimeError):
            A._ingest_host(path, 16000)
