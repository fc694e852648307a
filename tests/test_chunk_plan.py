"""The cut plan of transcribe_chunked without a GPU: the numpy restatement of its three definitions (tests/chunk_oracle.py,
which the GPU tests hold the kernels to) behaves as DESIGN.md §5b says on the test signal, and the C entry points refuse
bad arguments before any device work."""
import numpy as np
import pytest

import chunk_oracle
from oracle import mel as oracle_mel
from whisper_amd import hip

W, LO, HI = 10, 1500, 3000


@pytest.fixture(scope="module", params=[0.0, 1e-4], ids=["zero_gaps", "noise_gaps"])
def signal(request):
    return chunk_oracle.make_signal(gap_noise=request.param)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_cuts_fall_into_gaps(signal, n_mels):
    x, gaps = signal
    mel = oracle_mel.log_mel_spectrogram(x, oracle_mel.mel_filterbank(n_mels), padding=480000).numpy()
    content = mel.shape[1] - 3000
    assert content == len(x) // 160 and content > 10 * HI
    mel = mel[:, :content]
    L64, L32 = chunk_oracle.level(mel, np.float64), chunk_oracle.level(mel, np.float32)
    assert L32.dtype == np.float32
    cuts = chunk_oracle.walk(chunk_oracle.cost(L64, W), content, LO, HI)
    print(f"n_mels={n_mels}: {len(cuts)} cuts, max |L32 - L64| = {np.abs(L32 - L64).max():.3g}, "
          f"chunks {np.diff([0] + cuts + [content]).tolist()}")
    assert len(cuts) >= 10
    for c in cuts:
        assert chunk_oracle.in_gap(c, gaps, W), c
    sizes = np.diff([0] + cuts + [content])
    assert sizes.max() <= HI and sizes[:-1].min() >= LO
    assert chunk_oracle.walk(chunk_oracle.cost(L32, W), content, LO, HI) == cuts      # the float32 level gives the same cuts
    assert np.abs(L32 - L64).max() < 1e-4


def test_walk_tie_rule_and_short_input():
    C = np.ones(7000)
    C[2000:2400] = -3.0                      # a plateau of equal minima inside the first search range [1500, 3000]
    assert chunk_oracle.walk(C, 7000, LO, HI)[0] == 2399           # the LAST frame of the plateau
    C[5399 - 20: 5399] = -5.0
    assert chunk_oracle.walk(C, 7000, LO, HI) == [2399, 5398]
    for content in (0, 1, 2999, 3000):
        assert chunk_oracle.walk(np.zeros(content), content, LO, HI) == []
    assert chunk_oracle.walk(np.zeros(3001), 3001, LO, HI) == [3000]
    # the sliding max: +-W around every frame, clipped at the ends
    L = np.arange(10.0)[::-1].copy()
    assert chunk_oracle.cost(L, 0).tolist() == L.tolist()
    assert chunk_oracle.cost(L, 2).tolist() == [9, 9, 9, 8, 7, 6, 5, 4, 3, 2]


def test_cut_entry_points_validate_without_gpu():
    """wh_frame_level / wh_speech_cuts return status 1 on null or out-of-range arguments before touching the device"""
    lib = hip.lib()
    assert lib.wh_frame_level(None, 80, 6000, 3000, None, None) == 1
    assert lib.wh_frame_level(1 << 20, 0, 6000, 3000, 1 << 21, None) == 1                 # no mel rows
    assert lib.wh_frame_level(1 << 20, 80, 100, 3000, 1 << 21, None) == 1                 # stride shorter than the content
    p = 1 << 20                                                                          # never dereferenced: refused first
    assert lib.wh_speech_cuts(None, 9000, 1500, 3000, 10, None, None, None, 8, None) == 1
    assert lib.wh_speech_cuts(p, 9000, 1500, 3000, 65, None, p, p, 8, None) == 1          # guard > 64
    assert lib.wh_speech_cuts(p, 9000, 1500, 3000, -1, None, p, p, 8, None) == 1
    assert lib.wh_speech_cuts(p, 9000, 0, 3000, 10, None, p, p, 8, None) == 1             # min_frames < 1
    assert lib.wh_speech_cuts(p, 9000, 3001, 3000, 10, None, p, p, 8, None) == 1          # min_frames > max_frames
    assert lib.wh_speech_cuts(p, 9000, 1500, 3000, 10, None, p, p, 5, None) == 1          # max_cuts < 9000 / 1500
    assert lib.wh_speech_cuts(p, 0, 1500, 3000, 10, None, p, p, 8, None) == 1


def test_chunk_arguments_are_checked():
    import whisper_amd
    for bad in (dict(min_chunk_s=0.0), dict(min_chunk_s=30.5), dict(guard_s=0.65), dict(guard_s=-0.1)):
        with pytest.raises(ValueError):
            whisper_amd.plan_chunks(None, 9000, **bad)
    assert whisper_amd.plan_chunks(None, 0) == [] and whisper_amd.plan_chunks(None, 3000) == [(0, 3000)]    # nothing launched


def test_chunked_host_logic_equals_clip_by_clip(monkeypatch):
    """transcribe_chunked without a GPU: a stand-in model whose decode is a function of (window, temperature, prompt), the
    oracle's spectrogram and the restatement in place of the cut kernels.  Every chunk's segments are those of
    `transcribe(clip_timestamps=[a, b])`, the windows were decoded in batches, the ladder was climbed, the language was
    detected once, and a file without a cut takes the path of `transcribe`."""
    import sys
    import torch
    import whisper_amd
    from test_host_logic import _FunctionalModel
    from whisper_amd import decoding as mine
    from whisper_amd.tokenizer import get_tokenizer
    mine_tr = sys.modules["whisper_amd.transcribe"]
    tk = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    filt = oracle_mel.mel_filterbank(80)
    monkeypatch.setattr(mine_tr, "log_mel_spectrogram",
                        lambda a, n_mels=80, padding=0, device=None: oracle_mel.log_mel_spectrogram(a, filt, padding=padding))
    monkeypatch.setattr(hip, "frame_level", lambda mel, content: torch.from_numpy(chunk_oracle.level(mel[:, :content].numpy())))

    def cuts(level, lo, hi, W):
        C = chunk_oracle.cost(level.numpy(), W)
        return chunk_oracle.walk(C, len(C), lo, hi), torch.from_numpy(C)
    monkeypatch.setattr(hip, "speech_cuts", cuts)

    x, gaps = chunk_oracle.make_signal(1e-4, n_bursts=16)
    for kw in (dict(temperature=(0.0, 0.2, 0.4, 0.6)), dict(temperature=(0.0, 0.2), condition_on_previous_text=False,
                                                            initial_prompt="alpha")):
        ma, mb = _FunctionalModel(mine.DecodingResult, tk), _FunctionalModel(mine.DecodingResult, tk)
        got = mine_tr.transcribe_chunked(mb, x, batch_size=4, fp16=False, **kw)
        assert mb.detect_calls == [1] and got["language"] in ("en", "de", "fr")
        assert len(got["chunks"]) >= 5 and got["chunks"][0][0] == 0.0 and got["chunks"][-1][1] == (len(x) // 160) / 100.0
        assert all(a[1] == b[0] for a, b in zip(got["chunks"], got["chunks"][1:]))
        assert all(chunk_oracle.in_gap(round(100 * b), gaps, 10) for _, b in got["chunks"][:-1])
        assert [s["id"] for s in got["segments"]] == list(range(len(got["segments"])))
        texts, n = [], 0
        for a, b in got["chunks"]:
            want = mine_tr.transcribe(ma, x, clip_timestamps=[a, b], language=got["language"], fp16=False, **kw)
            mine_segments = [{**s, "id": i} for i, s in
                             enumerate(s for s in got["segments"] if round(100 * a) <= s["seek"] < round(100 * b))]
            assert mine_segments == want["segments"] and len(mine_segments) >= 1
            texts.append(want["text"])
            n += len(mine_segments)
        assert n == len(got["segments"]) and got["text"] == "".join(texts)
        assert sum(n for n, _ in mb.calls) == sum(n for n, _ in ma.calls)            # the same decodes in total
        assert max(n for n, _ in mb.calls) == 4 and len(mb.calls) < len(ma.calls)    # ... as batches of batch_size rows
    assert {s["temperature"] for s in got["segments"]} >= {0.0, 0.2}                 # the ladder was climbed

    # at most 30 s: exactly transcribe's result, and nothing of the cut path runs
    monkeypatch.setattr(hip, "frame_level", lambda *a, **k: pytest.fail("cut kernels launched for a file without a cut"))
    for n in (0, 4960, 480000):
        ma, mb = _FunctionalModel(mine.DecodingResult, tk), _FunctionalModel(mine.DecodingResult, tk)
        want = mine_tr.transcribe(ma, x[:n], fp16=False)
        got = mine_tr.transcribe_chunked(mb, x[:n], fp16=False)
        assert {k: got[k] for k in want} == want and mb.calls == ma.calls
        assert got["chunks"] == ([(0.0, (n // 160) / 100.0)] if n else [])
    with pytest.raises(ValueError):
        mine_tr.transcribe_chunked(mb, x, clip_timestamps="0")
    with pytest.raises(ValueError):
        mine_tr.transcribe_chunked(mb, x, min_chunk_s=40.0)
    assert whisper_amd.Whisper.transcribe_chunked is mine_tr.transcribe_chunked
