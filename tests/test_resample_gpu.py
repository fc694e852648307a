"""Device-side audio ingest on the GPU (DESIGN.md §5b "Device-side ingest"; csrc/resample.hip): the kernel against the
float64 restatement of its definition (tests/resample_oracle.py) over every stored format, channel count, rate and the
awkward lengths; against the host path it stands in for; through load_audio on the head of jfk.flac; and the file-level
entry points with `device_ingest=True` equal to the same calls handed the device-loaded tensors.

What may differ from the restatement: only samples where 32768 y lies within float64 rounding error of a tie (another order
of summation).  So a case may differ in at most max(1, n_out // 100000) samples, each by one 16-bit step."""
import os
import wave

import numpy as np
import pytest
import torch

import chunk_oracle
import resample_oracle as R
import whisper_amd
from whisper_amd import audio as A
from whisper_amd import hip
from whisper_amd.synthetic import dims_for, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JFK = os.path.join(GOLDEN, "jfk_head.flac")
RATES = (8000, 11025, 12345, 22050, 32000, 44100, 48000, 96000)
REPORT = {}


def report(key, value):
    from conftest import write_report
    REPORT[key] = value
    write_report("resample.json", REPORT)


def on_device(pcm, rate, bits, dev):
    return hip.resample(torch.from_numpy(pcm).to(dev), rate, 16000, bits)


def steps_of(samples):
    """float32 samples -> their integer 16-bit steps, after checking that every one of them IS on the 16-bit grid"""
    s = samples.astype(np.float64) * 32768.0
    assert np.array_equal(s, np.rint(s)) and s.min(initial=0) >= -32768 and s.max(initial=0) <= 32767
    return s.astype(np.int64)


def check_case(got_t, pcm, rate, bits, tag):
    up, down = R.ratio(rate, 16000)
    assert got_t.dtype == torch.float32 and got_t.is_cuda and got_t.shape == (-(-len(pcm) * up // down),), tag
    got, want = got_t.cpu().numpy(), R.ingest(pcm, rate, 16000, bits)
    diff = np.abs(steps_of(got) - steps_of(want))
    n_diff = int((diff > 0).sum())
    print(tag, "n_out", len(got), "differ", n_diff, "max steps", int(diff.max(initial=0)))
    assert diff.max(initial=0) <= 1, tag
    assert n_diff <= max(1, len(got) // 100000), (tag, n_diff)
    return n_diff


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("rate", RATES)
def test_kernel_equals_restatement(gpu_device, rate, fmt):
    """{u8, s16, s24 in int32, s32, f32} x {1, 2, 6} channels x the eight rates x lengths {1, 7, fewer frames than half / up,
    5 s + 17}: length, dtype, 16-bit grid, at most one step from the restatement, at most max(1, n_out // 100000) samples
    differing at all"""
    up, down = R.ratio(rate, 16000)
    short = max(1, 10 * max(up, down) // up - 1)
    total = 0
    for channels in (1, 2, 6):
        for n in (1, 7, short, 5 * rate + 17):
            pcm, bits = R.store(R.signal(n, channels, rate, seed=rate + 10 * channels + n % 7), fmt)
            total += check_case(on_device(pcm, rate, bits, gpu_device), pcm, rate, bits, f"{fmt}/{rate}/{channels}ch/{n}")
    report(f"restatement_{fmt}_{rate}", {"samples_differing": total})


def test_kernel_long_input_and_mono_vector(gpu_device):
    """95 s + 7 frames at 44.1 kHz stereo (16 000 workgroups; the last one partly filled); a 1-d tensor is one channel"""
    rate, n = 44100, 95 * 44100 + 7
    pcm, bits = R.store(R.signal(n, 2, rate, seed=95), "s16")
    n_diff = check_case(on_device(pcm, rate, bits, gpu_device), pcm, rate, bits, "s16/44100/2ch/95s")
    report("restatement_95s", {"samples": -(-n * 160 // 441), "samples_differing": n_diff})
    mono = np.ascontiguousarray(pcm[:44100, 0])
    got = hip.resample(torch.from_numpy(mono).to(gpu_device), rate)
    assert torch.equal(got, on_device(mono[:, None], rate, 16, gpu_device))
    assert hip.resample(torch.zeros(0, 2, dtype=torch.int16, device=gpu_device), rate).shape == (0,)
    f64 = R.signal(4000, 2, rate, seed=2)
    check_case(hip.resample(torch.from_numpy(f64).to(gpu_device), rate), f64, rate, 0, "f64/44100/2ch/4000")


@pytest.mark.parametrize("rate", RATES)
def test_full_scale_square_wave_clips(gpu_device, rate):
    """full-scale square waves at s16: the filter overshoots at every edge, so the clip to [-32768, 32767] is exercised"""
    n = rate + 17
    period = max(2, rate // 200)
    hi = (np.arange(n) // period) % 2 == 0
    pcm = np.where(hi, 32767, -32768).astype(np.int16)[:, None].repeat(2, axis=1)
    got = on_device(pcm, rate, 16, gpu_device)
    check_case(got, pcm, rate, 16, f"square/{rate}")
    y = R.resample(R.mono(pcm, 16), rate, 16000)
    assert y.max() * 32768 > 32767.5 and y.min() * 32768 < -32768.5              # the signal does leave the range
    g = got.cpu().numpy()
    assert g.max() == np.float32(32767 / 32768) and g.min() == np.float32(-1.0)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_same_rate_is_downmix_and_quantise(gpu_device, fmt):
    """rate == 16000: no filter; the output equals down-mix + quantisation EXACTLY (ties included: x.5 is exact in float64)"""
    for channels in (1, 2, 6):
        pcm, bits = R.store(R.signal(16000 + 17, channels, 16000, seed=channels), fmt)
        got = on_device(pcm, 16000, bits, gpu_device).cpu().numpy()
        want = R.quantise(R.mono(pcm, bits))
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fmt, channels)


def test_device_path_against_host_path(gpu_device):
    """the device path against the host path it stands in for (audio._to_mono_s16: scipy's resample_poly, accumulating in
    float32), 5 s + 17 frames of stereo s16 per rate: never more than one 16-bit step apart, and the share of samples that
    differ — recorded per rate — stays below 0.5 % (the host path's own distance from the definition is <= 0.11 %; the
    device path adds float64 ties only)."""
    pytest.importorskip("scipy")
    shares = {}
    for rate in RATES:
        pcm, bits = R.store(R.signal(5 * rate + 17, 2, rate, seed=rate), "s16")
        got = steps_of(on_device(pcm, rate, bits, gpu_device).cpu().numpy())
        host = steps_of(A._to_mono_s16(A._pcm_to_float(pcm, bits), rate, 16000))
        assert got.shape == host.shape
        diff = np.abs(got - host)
        shares[str(rate)] = {"samples": len(got), "differing": int((diff > 0).sum()), "share": float((diff > 0).mean()),
                             "max_steps": int(diff.max())}
        print("device vs host", rate, shares[str(rate)])
    report("device_vs_host_path", shares)
    for rate, r in shares.items():
        assert r["max_steps"] <= 1, (rate, r)
        assert r["share"] < 0.005, (rate, r)


def test_jfk_head_through_load_audio(gpu_device):
    """load_audio(jfk_head.flac, device=gpu) — 24-bit stereo FLAC at 44.1 kHz, uploaded as the decoder's int32 — against
    load_audio of the whole file (tests/golden/jfk_tiny_en.npz) over the first n - 16 samples, the comparison
    tests/test_audio_io.py makes for the host path: at most one step anywhere; the share of differing samples is recorded"""
    got_t = A.load_audio(JFK, device=gpu_device)
    assert got_t.dtype == torch.float32 and got_t.device == gpu_device and got_t.dim() == 1
    got = steps_of(got_t.cpu().numpy())
    assert got.shape[0] == -(-16 * 4608 * 16000 // 44100)
    whole = np.load(os.path.join(GOLDEN, "jfk_tiny_en.npz"))["jfk_pcm16"].astype(np.int64)
    n = got.shape[0] - 16
    diff = np.abs(got[:n] - whole[:n])
    report("jfk_head_vs_host_golden", {"samples": n, "differing": int((diff > 0).sum()), "share": float((diff > 0).mean()),
                                      "max_steps": int(diff.max())})
    print("jfk head", REPORT["jfk_head_vs_host_golden"])
    assert diff.max() <= 1
    with open(JFK, "rb") as f:
        pcm, rate, bps = A.decode_flac(f.read())
    check_case(got_t, pcm, rate, bps, "jfk_head")                          # and it is the definition applied to the decoded PCM
    assert torch.equal(A.load_audio(JFK, device="cuda"), got_t)


def test_log_mel_of_device_ingested_audio(gpu_device):
    """log_mel_spectrogram of the device-ingested jfk head against that of the host-loaded one (80 and 128 mels): the
    largest absolute difference is recorded and must stay below 8e-4.  The bound set before anything was measured was 1e-3
    (one 16-bit step on ~0.05 % of the samples moves the energy of a frame far less than the front end's 1e-4
    kernel-against-float64 bound; the factor 10 was margin for the log of near-silent bins), to be tightened to what was
    observed: 4.7e-4 at 80 mels, 6.7e-4 at 128 on an MI355X (profiles/resample.json).  Both inputs and the mel kernel are
    deterministic, so the figure does not move from run to run."""
    pytest.importorskip("scipy")
    with open(JFK, "rb") as f:
        pcm, rate, bps = A.decode_flac(f.read())
    host = A._to_mono_s16(A._pcm_to_float(pcm, bps), rate, 16000)
    dev_audio = A.load_audio(JFK, device=gpu_device)
    out = {}
    for n_mels in (80, 128):
        a = whisper_amd.log_mel_spectrogram(dev_audio, n_mels)
        b = whisper_amd.log_mel_spectrogram(host, n_mels, device=gpu_device)
        assert a.shape == b.shape
        out[str(n_mels)] = float((a - b).abs().max().item())
    report("log_mel_max_abs_diff_jfk_head", out)
    print("log-mel device-ingested vs host-loaded", out)
    assert max(out.values()) < 8e-4, out


# ---- the file-level entry points ------------------------------------------------------------------------------------------
def _write_wav(path, x16k, seed):
    """a 44.1 kHz stereo 16-bit WAV whose content is the 16 kHz test signal, linearly interpolated (any band-limited-ish
    signal will do: both routes read the same file)"""
    n = int(len(x16k) * 44100 / 16000)
    t = np.arange(n) * (16000 / 44100)
    left = np.interp(t, np.arange(len(x16k)), x16k)
    right = 0.8 * left + 0.01 * np.random.default_rng(seed).standard_normal(n)
    pcm = np.clip(np.round(np.stack([left, right], axis=1) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def setup(gpu_device, tmp_path_factory):
    dims = dims_for("micro.en")
    d = tmp_path_factory.mktemp("ingest")
    ckpt = str(d / "micro.en.pt")
    save_checkpoint(ckpt, dims, synthetic_state_dict(dims, seed=1))
    model = whisper_amd.load_model(ckpt, device=gpu_device)
    long_wav, short_wav = str(d / "long.wav"), str(d / "short.wav")
    _write_wav(long_wav, chunk_oracle.make_signal(1e-4, n_bursts=9, seed=4)[0], 1)        # ~80 s: transcribe_chunked cuts it
    _write_wav(short_wav, chunk_oracle.burst(np.random.default_rng(7), 16000 * 21), 2)
    return model, [long_wav, short_wav, JFK]


KW = dict(temperature=0.0, fp16=False, language="en", sample_len=12, no_speech_threshold=None, logprob_threshold=None,
          compression_ratio_threshold=None)


def same_result(a, b):
    assert a["text"] == b["text"] and a["language"] == b["language"] and len(a["segments"]) == len(b["segments"])
    for s, t in zip(a["segments"], b["segments"]):
        assert s["tokens"] == t["tokens"] and s["text"] == t["text"]
        assert (s["seek"], s["start"], s["end"]) == (t["seek"], t["start"], t["end"])
    assert a.get("chunks") == b.get("chunks")


def test_transcribe_batch_device_ingest(setup, gpu_device):
    """transcribe_batch(paths, device_ingest=True) == transcribe_batch of load_audio(path, device=gpu) tensors;
    device_ingest=False == transcribe_batch of load_audio(path) arrays (what it returned before the option existed)"""
    model, paths = setup
    tensors = [A.load_audio(p, device=gpu_device) for p in paths]
    got = model.transcribe_batch(paths, batch_size=4, device_ingest=True, **KW)
    want = model.transcribe_batch(tensors, batch_size=4, **KW)
    assert len(got) == len(want) == 3 and all(len(r["segments"]) >= 1 for r in got)
    for a, b in zip(got, want):
        same_result(a, b)
    lanes = model.transcribe_batch(paths, batch_size=2, in_flight=2, device_ingest=True, **KW)
    for a, b in zip(lanes, want):
        same_result(a, b)
    arrays = [A.load_audio(p) for p in paths]
    off = model.transcribe_batch(paths, batch_size=4, device_ingest=False, **KW)
    for a, b, c in zip(off, model.transcribe_batch(arrays, batch_size=4, **KW), model.transcribe_batch(paths, batch_size=4, **KW)):
        same_result(a, b)
        same_result(a, c)
    passed = model.transcribe_batch(arrays, batch_size=4, device_ingest=True, **KW)     # arrays are untouched by the option
    for a, b in zip(passed, off):
        same_result(a, b)


def test_transcribe_and_chunked_device_ingest(setup, gpu_device):
    model, paths = setup
    for i, p in enumerate(paths):
        tensor, array = A.load_audio(p, device=gpu_device), A.load_audio(p)
        same_result(model.transcribe(p, device_ingest=True, **KW), model.transcribe(tensor, **KW))
        same_result(model.transcribe(p, device_ingest=False, **KW), model.transcribe(array, **KW))
        got = model.transcribe_chunked(p, batch_size=4, device_ingest=True, **KW)
        same_result(got, model.transcribe_chunked(tensor, batch_size=4, **KW))
        same_result(model.transcribe_chunked(p, batch_size=4, device_ingest=False, **KW),
                    model.transcribe_chunked(array, batch_size=4, **KW))
        if i == 0:
            assert len(got["chunks"]) >= 2                                  # the long file really was cut


def test_transcribe_sharded_device_ingest(setup, gpu_device):
    """launcher.transcribe_sharded(device_ingest=True) on one GPU (no process group: this rank takes every file) == the
    device-loaded tensors through transcribe_batch; without the option == the host-loaded arrays"""
    from whisper_amd import launcher
    model, paths = setup
    got = launcher.transcribe_sharded(model, paths, None, batch_size=4, device_ingest=True, **KW)
    want = model.transcribe_batch([A.load_audio(p, device=gpu_device) for p in paths], batch_size=4, **KW)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        same_result(a, b)
    off = launcher.transcribe_sharded(model, paths, None, batch_size=4, **KW)
    for a, b in zip(off, model.transcribe_batch([A.load_audio(p) for p in paths], batch_size=4, **KW)):
        same_result(a, b)


def test_refused_inputs(gpu_device, tmp_path):
    """a rate pair whose filter exceeds the table limit raises HipLimitError before anything is built or launched; more than
    8 channels and unknown dtypes are refused; a 9-channel WAV through load_audio(device=...) takes the host route"""
    x = torch.zeros(100, 2, dtype=torch.int16, device=gpu_device)
    with pytest.raises(hip.HipLimitError):
        hip.resample(x, 500009)                                            # prime: 20 * 500009 + 1 taps > 2^23
    with pytest.raises(hip.HipError):
        hip.resample(torch.zeros(100, 9, dtype=torch.int16, device=gpu_device), 44100)
    with pytest.raises(ValueError):
        hip.resample(torch.zeros(100, 2, dtype=torch.int64, device=gpu_device), 44100)
    pytest.importorskip("scipy")
    pcm = np.round(R.signal(4410, 9, 44100, seed=9) * 32768.0).astype("<i2")
    path = str(tmp_path / "wide.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(9)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm.tobytes())
    got = A.load_audio(path, device=gpu_device)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), A.load_audio(path))
