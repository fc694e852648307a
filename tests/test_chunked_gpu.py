"""transcribe_chunked on the GPU (DESIGN.md §5b "Cutting a file at pauses"): the level kernel against the float64
restatement of its definition, cost and cuts EXACT against the restatement run on the device's own level, the chunked
transcription equal to `transcribe(clip_timestamps=[a, b])` chunk by chunk, short and degenerate files equal to `transcribe`."""
import os

import numpy as np
import pytest
import torch

import chunk_oracle
import whisper_amd
from whisper_amd import hip
from whisper_amd.synthetic import dims_for, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu
JFK = os.path.join(os.path.dirname(__file__), "golden", "jfk_head.flac")
N_FRAMES = 3000


@pytest.fixture(scope="module")
def signals():
    return {"zero_gaps": chunk_oracle.make_signal(0.0)[0], "noise_gaps": chunk_oracle.make_signal(1e-4)[0]}


def device_mel(x, n_mels, dev):
    """the whole-file spectrogram as transcribe computes it (30 s of padding), and the number of frames of the file"""
    mel = whisper_amd.log_mel_spectrogram(x, n_mels, padding=480000, device=dev)
    return mel, mel.shape[-1] - N_FRAMES


def test_frame_level(gpu_device, signals):
    """hip.frame_level against the float64 restatement, on the device's own spectrograms of the test signal and of the head
    of jfk.flac, 80 and 128 mels: 1e-4 absolute, the project's fp32-against-float64 bound for log-mel values (an fp32 sum of
    <= 128 positive terms is good to ~1e-5 relative = 4e-6 in log10)."""
    from conftest import write_report
    report = {}
    inputs = dict(signals, jfk_head=whisper_amd.load_audio(JFK))
    for name, x in inputs.items():
        for n_mels in (80, 128):
            mel, content = device_mel(x, n_mels, gpu_device)
            got = hip.frame_level(mel, content).cpu().numpy()
            want = chunk_oracle.level(mel[:, :content].cpu().numpy(), np.float64)
            assert got.shape == want.shape == (content,) and got.dtype == np.float32
            report[f"{name}_{n_mels}"] = {"frames": content, "max_abs_err": float(np.abs(got - want).max()),
                                          "level_min": float(want.min()), "level_max": float(want.max())}
            print(name, n_mels, report[f"{name}_{n_mels}"])
    write_report("chunk_level.json", report)
    for key, r in report.items():
        assert r["max_abs_err"] < 1e-4, (key, r)


@pytest.mark.parametrize("W", [0, 10, 64])
@pytest.mark.parametrize("min_frames", [500, 1500, 3000])
def test_cost_and_cuts_exact(gpu_device, signals, W, min_frames):
    """cost and walk of the restatement on the level DOWNLOADED from the device: hip.speech_cuts returns the same integer
    list, and its cost is bit-equal to the restatement's sliding max"""
    for name, x in signals.items():
        mel, content = device_mel(x, 80, gpu_device)
        level = hip.frame_level(mel, content)
        cuts, cost = hip.speech_cuts(level, min_frames, N_FRAMES, W)
        want_cost = chunk_oracle.cost(level.cpu().numpy(), W)
        assert np.array_equal(cost.cpu().numpy().view(np.uint32), want_cost.view(np.uint32)), (name, W)
        want = chunk_oracle.walk(want_cost, content, min_frames, N_FRAMES)
        assert cuts == want, (name, W, min_frames)
        assert len(cuts) >= 10
        sizes = np.diff([0] + cuts + [content])
        assert sizes.max() <= N_FRAMES and sizes[:-1].min() >= min_frames


def test_cuts_on_ties(gpu_device):
    """a random level with injected plateaus of exactly equal minima: the walk takes the LAST frame of a plateau (the tie
    rule sits inside the kernel's reduction: across lanes, across waves, across a thread's strided frames); without a cost
    buffer (cost_out = NULL) the cuts are the same"""
    import ctypes as C
    rng = np.random.default_rng(5)
    n = 40000
    L = rng.standard_normal(n).astype(np.float32)
    for at in range(1200, n - 3000, 2100):
        L[at: at + int(rng.integers(30, 1400))] = -7.25             # plateaus longer and shorter than the 1024 threads
    L[n - 900:] = -7.25
    level = torch.from_numpy(L).to(gpu_device)
    for W, lo in ((0, 1500), (10, 1500), (3, 1), (64, 2000)):
        cuts, cost = hip.speech_cuts(level, lo, N_FRAMES, W)
        want_cost = chunk_oracle.cost(L, W)
        assert np.array_equal(cost.cpu().numpy().view(np.uint32), want_cost.view(np.uint32))
        want = chunk_oracle.walk(want_cost, n, lo, N_FRAMES)
        assert cuts == want, (W, lo)
        assert any(want_cost[c] == -7.25 and want_cost[c + 1] > -7.25 for c in cuts)        # a plateau's last frame was taken
        out = torch.full((64,), -1, dtype=torch.int32, device=gpu_device)
        count = torch.zeros(1, dtype=torch.int32, device=gpu_device)
        if n // lo <= 64:
            rc = hip.lib().wh_speech_cuts(level.data_ptr(), n, lo, N_FRAMES, W, None, out.data_ptr(), count.data_ptr(), 64,
                                          hip.stream_ptr(torch.cuda.current_stream(gpu_device)))
            assert rc == 0 and out[: int(count.item())].tolist() == want
    assert whisper_amd.plan_chunks(level[None].expand(4, n), 3000) == [(0, 3000)]           # no cut, nothing launched


@pytest.fixture(scope="module", params=["micro.en", "micro-v3"])
def setup(request, gpu_device, tmp_path_factory):
    """the synthetic checkpoints of tests/test_api_gpu.py::setup"""
    name = request.param
    dims = dims_for(name)
    path = str(tmp_path_factory.mktemp("ckpt") / f"{name}.pt")
    save_checkpoint(path, dims, synthetic_state_dict(dims, seed=1))
    return dims, whisper_amd.load_model(path, device=gpu_device)


def count_rows(monkeypatch):
    """rows of every DecodingTask.run call from here on"""
    from whisper_amd.decoding import DecodingTask
    rows, run = [], DecodingTask.run

    def counted(self, mel):
        rows.append(int(mel.shape[0]))
        return run(self, mel)
    monkeypatch.setattr(DecodingTask, "run", counted)
    return rows


@pytest.mark.parametrize("cond,beam", [(False, None), (True, None), (True, 3)])
def test_chunked_equals_clip_by_clip(setup, gpu_device, signals, monkeypatch, cond, beam):
    """transcribe_chunked on the test signal: its chunks are the plan of the cut kernels (= the restatement on the device's
    level), and the segments of every chunk equal those of `transcribe(x, clip_timestamps=[a, b])` — tokens, seeks, bounds,
    word times, avg_logprob, compared as test_api_gpu.py::test_transcribe_batch_equals_sequential compares them — while the
    driver really decoded the chunks' windows as batches of 8 rows.  fp32 strict engine."""
    dims, model = setup
    x = signals["zero_gaps"]
    kw = dict(temperature=0.0, fp16=False, language="en", sample_len=12, word_timestamps=True,
              condition_on_previous_text=cond, no_speech_threshold=None, logprob_threshold=None,
              compression_ratio_threshold=None)
    if beam:
        kw["beam_size"] = beam
    rows = count_rows(monkeypatch)
    got = model.transcribe_chunked(x, batch_size=8, **kw)
    chunk_rows = list(rows)
    assert set(got) == {"text", "segments", "language", "chunks"} and got["language"] == "en"

    mel, content = device_mel(x, dims.n_mels, gpu_device)
    want_cuts = chunk_oracle.walk(chunk_oracle.cost(hip.frame_level(mel, content).cpu().numpy(), 10), content, 1500, N_FRAMES)
    bounds = [0] + want_cuts + [content]
    assert got["chunks"] == [(a / 100.0, b / 100.0) for a, b in zip(bounds[:-1], bounds[1:])]
    assert whisper_amd.plan_chunks(mel, content) == list(zip(bounds[:-1], bounds[1:]))
    assert len(got["chunks"]) >= 10
    assert max(chunk_rows) == 8 and chunk_rows.count(8) >= 1, chunk_rows          # the driver batched
    assert [s["id"] for s in got["segments"]] == list(range(len(got["segments"])))

    n_segments, texts = 0, []
    for a, b in got["chunks"]:
        g = [s for s in got["segments"] if round(100 * a) <= s["seek"] < round(100 * b)]
        w = model.transcribe(x, clip_timestamps=[a, b], **kw)
        ws = w["segments"]
        assert len(g) == len(ws) >= 1
        assert [s["tokens"] for s in g] == [s["tokens"] for s in ws]
        assert [s["seek"] for s in g] == [s["seek"] for s in ws]
        assert [s["text"] for s in g] == [s["text"] for s in ws]
        assert np.allclose([[s["start"], s["end"]] for s in g], [[s["start"], s["end"]] for s in ws])
        gw = [[v["start"], v["end"]] for s in g for v in s["words"]]
        ww = [[v["start"], v["end"]] for s in ws for v in s["words"]]
        assert np.allclose(gw, ww, atol=0.0201)
        assert np.allclose([s["avg_logprob"] for s in g], [s["avg_logprob"] for s in ws], atol=1e-4)
        n_segments += len(g)
        texts.append(w["text"])
    assert n_segments == len(got["segments"])                                      # every segment belongs to one chunk
    assert got["text"] == "".join(texts)


SHORT = {
    "clip_11s": lambda: chunk_oracle.burst(np.random.default_rng(31), 176000),
    "empty": lambda: np.zeros(0, dtype=np.float32),
    "short": lambda: chunk_oracle.burst(np.random.default_rng(31), 4960),
    "silence": lambda: np.zeros(16000 * 12, dtype=np.float32),
    "one_window": lambda: chunk_oracle.burst(np.random.default_rng(33), 480000),      # exactly 3000 frames
}


@pytest.mark.parametrize("case", list(SHORT))
def test_short_files_equal_transcribe(setup, monkeypatch, case):
    """at most 30 s: no cut, and every field of the result is what `transcribe` returns (default thresholds on, word
    timestamps); the cut kernels are not launched"""
    dims, model = setup
    x = SHORT[case]()
    kw = dict(temperature=0.0, fp16=False, language="en", sample_len=12, condition_on_previous_text=True, word_timestamps=True)
    want = model.transcribe(x, **kw)
    monkeypatch.setattr(hip, "frame_level", lambda *a, **k: pytest.fail("cut kernels launched for a file without a cut"))
    got = model.transcribe_chunked(x, batch_size=8, **kw)
    assert set(got) == set(want) | {"chunks"}
    assert {k: got[k] for k in want} == want
    assert got["chunks"] == ([] if len(x) == 0 else [(0.0, (len(x) // 160) / 100.0)])
    if case == "empty":
        assert got["segments"] == [] and got["text"] == ""
        if model.is_multilingual:                    # language detection on a window that is all padding, as transcribe
            assert (model.transcribe_chunked(x, temperature=0.0, fp16=False, sample_len=4)["language"]
                    == model.transcribe(x, temperature=0.0, fp16=False, sample_len=4)["language"])


def test_refused_arguments(setup):
    dims, model = setup
    x = chunk_oracle.burst(np.random.default_rng(1), 16000)
    with pytest.raises(ValueError):
        model.transcribe_chunked(x, clip_timestamps=[0.0, 0.5])
    with pytest.raises(ValueError):
        model.transcribe_chunked(x, clip_timestamps="0")
    for bad in (dict(min_chunk_s=0.0), dict(min_chunk_s=31.0), dict(min_chunk_s=-1.0), dict(guard_s=0.65), dict(batch_size=0)):
        with pytest.raises(ValueError):
            model.transcribe_chunked(x, **bad)


def test_language_detected_once(gpu_device, signals, monkeypatch, tmp_path):
    """a multilingual model and no language given: ONE detection on the head of the file, and every chunk decodes in it"""
    dims = dims_for("micro-v3")
    path = str(tmp_path / "micro-v3.pt")
    save_checkpoint(path, dims, synthetic_state_dict(dims, seed=1))
    model = whisper_amd.load_model(path, device=gpu_device)
    calls, detect = [], type(model).detect_language

    def counted(self, mel, *a, **k):
        calls.append(tuple(mel.shape))
        return detect(self, mel, *a, **k)
    monkeypatch.setattr(type(model), "detect_language", counted)
    x = signals["noise_gaps"][: 16000 * 100]
    kw = dict(temperature=0.0, fp16=False, sample_len=6, no_speech_threshold=None, logprob_threshold=None,
              compression_ratio_threshold=None)
    got = model.transcribe_chunked(x, batch_size=4, **kw)
    assert len(calls) == 1 and calls[0] == (dims.n_mels, N_FRAMES)
    monkeypatch.undo()
    assert got["language"] == model.transcribe(x[: 16000 * 30], **kw)["language"]
    assert len(got["chunks"]) >= 3 and len(got["segments"]) >= len(got["chunks"])
