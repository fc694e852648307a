"""Forced alignment on the GPU (whisper_amd/align.py, timing.find_alignment_open_batch, the open-end DTW of timing.hip) against
the float32 CPU oracle of tests/align_oracle.py: the kernels alone through the test library, one window on an alignment-
conditioned 4-layer checkpoint, and `align` / `align_batch` end to end on synthetic files with planted encoder features."""
import base64
import gzip
import sys
import zlib

import numpy as np
import pytest
import torch

import align_oracle as ao
import oracle
from oracle import condition

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 1), (8, 40), (33, 129), (200, 750), (0, 9)]       # (N, M); the last: a clip without tokens
CLOSED = [0, 1, 0, 1, 0, 0, 0]


def _ragged_costs(seed):
    rng = np.random.default_rng(seed)
    Nmax, Fmax = max(n for n, _ in SHAPES), max(m for _, m in SHAPES)
    slab = np.zeros((len(SHAPES), Nmax, Fmax), dtype=np.float32)
    mats = []
    for b, (N, M) in enumerate(SHAPES):
        x = rng.standard_normal((N, M)).astype(np.float32)
        if N >= 8:                                   # a ridge that leaves the window two thirds down the rows
            inside = max(1, 2 * N // 3)
            for i in range(inside):
                x[i, i * M // inside: (i + 1) * M // inside] -= 2
        slab[b, :N, :M] = x
        mats.append(x)
    return slab, mats


@pytest.mark.parametrize("end_slack", [0.01, 0.0])
def test_open_dtw_kernels_equal_the_oracle(gpu_device, end_slack):
    """wht_dtw_open (open-end wavefront, end selection, back-trace from `end`) on one ragged batch of random float32 costs:
    the last column bit for bit, `end`, the jump frames, the path and its length as the float32 numpy oracle gives them"""
    from whisper_amd import hip
    slab, mats = _ragged_costs(7)
    rows, cols = [n for n, _ in SHAPES], [m for _, m in SHAPES]
    trace, lastcol, end, jumps, path, plen = hip.dtw_open_ktest(torch.from_numpy(slab).to(gpu_device), rows, cols, CLOSED,
                                                                end_slack)
    torch.cuda.synchronize()
    trace, lastcol, end, jumps, path, plen = (t.cpu().numpy() for t in (trace, lastcol, end, jumps, path, plen))
    open_ends = []
    for b, (N, M) in enumerate(SHAPES):
        want = ao.dtw_open(mats[b], bool(CLOSED[b]), end_slack)
        assert end[b] == want["end"], (b, end[b], want["end"])
        if N == 0:
            assert plen[b] == 0
            continue
        assert lastcol[b, :N].tobytes() == want["lastcol"].tobytes(), b             # bit-equal
        assert np.array_equal(trace[b, : (N + 1) * (M + 1)].reshape(N + 1, M + 1), want["trace"]), b
        e, n = want["end"], want["path"].shape[1]
        assert plen[b] == n and np.array_equal(jumps[b, :e], want["jumps"]), b
        assert np.array_equal(path[b][:, path.shape[2] - n:], want["path"]), b
        if not CLOSED[b]:
            open_ends.append((N, e))
    assert any(e < N for N, e in open_ends), open_ends            # the open end is exercised: some path leaves early


def test_closed_everywhere_equals_todays_dtw(gpu_device):
    """closed = 1 in every clip: trace, jumps and path of dtw_trace + dtw_backtrace, clip by clip"""
    from whisper_amd import hip
    slab, mats = _ragged_costs(11)
    rows, cols = [n for n, _ in SHAPES], [m for _, m in SHAPES]
    trace, _, end, jumps, path, plen = hip.dtw_open_ktest(torch.from_numpy(slab).to(gpu_device), rows, cols, [1] * len(SHAPES),
                                                          0.01)
    assert end.cpu().tolist() == rows
    for b, (N, M) in enumerate(SHAPES):
        if N == 0:
            continue
        tr = hip.dtw_trace(torch.from_numpy(mats[b]).to(gpu_device))
        j0, p0 = hip.dtw_backtrace(tr)
        assert torch.equal(trace[b, : (N + 1) * (M + 1)].reshape(N + 1, M + 1), tr), b
        assert torch.equal(jumps[b, :N], j0) and int(plen[b]) == p0.shape[1], b
        assert torch.equal(path[b][:, path.shape[2] - p0.shape[1]:], p0), b


# ---- an alignment-conditioned 4-layer checkpoint ----------------------------------------------------------------------
SENTENCE = (" the quick brown fox jumps over the lazy dog and keeps running for a while longer than anyone expected it to,"
            " numbers like 1234567 and 3.14159 split into several tokens, as do names such as Przybyszewski and others too,"
            " which is why the list goes on.")


# Planted audio features: unit noise + FEAT_GAIN * time code.  At unit gain a spoken row gains about 40 cost units and a row
# behind the window's end next to nothing: the regime the slack rule was specified for (30 ... 100 per spoken row).
# alignment_features' own default, 4, makes the cross-attention softmax so sharp that the side lobes of the time code (its
# periods near 331 and 604 frames) become ridges of their own: candidate rows 49 ... 52, planted 322 frames behind the
# window's end, then attend to its last frames, the last column falls by another ~30 there, and the CPU oracle ends at rows
# 52 ... 60 of 61 for every end_slack in 0.002 ... 0.02.  That is a second ridge in the inputs, not an open end.
FEAT_GAIN = 1.0
FRAMES_PER_TOKEN, FIRST_FRAME = 11, 12                  # condition_alignment defaults: position p is spoken at frame 12 + 11 p


class _Conditioned:
    def __init__(self, device):
        from whisper_amd.model import ModelDimensions, Whisper
        from whisper_amd.synthetic import dims_dict
        from whisper_amd.tokenizer import get_tokenizer
        self.dims = dims = oracle.dims_for("tiny")                       # 4 + 4 layers, D = 384, 6 heads of 64
        sd = oracle.synthetic_state_dict(dims, seed=4)
        L = dims.n_text_layer
        self.heads = sorted([(L - 1, 1), (L - 1, 4), (L - 2, 0), (L - 2, 3)])
        self.info = condition.condition_alignment(sd, dims, self.heads, seed=1)              # defaults: 11 frames per token from 12
        self.om = oracle.OracleModel(dims, sd)
        self.model = Whisper(ModelDimensions(**dims_dict(dims)), sd, device=device)
        mask = np.zeros((dims.n_text_layer, dims.n_text_head), dtype=bool)
        for l, h in self.heads:
            mask[l, h] = True
        self.model.set_alignment_heads(base64.b85encode(gzip.compress(mask.tobytes())))
        self.tok = get_tokenizer(True, num_languages=self.model.num_languages, language="en", task="transcribe")
        self._feats = {}

    def feats(self, seed):
        if seed not in self._feats:
            self._feats[seed] = condition.alignment_features(self.dims, 1, self.info["U_a"], seed=seed, feat_gain=FEAT_GAIN)
        return self._feats[seed]

    # the seam: align() obtains encoder output only through model.encoder(batch of mel windows).  A random-init encoder
    # cannot produce the time code, so every window gets planted features, seeded by the window's own first mel values.
    @staticmethod
    def seed_of(mel_window):
        return zlib.crc32(mel_window[0, :32].half().cpu().numpy().tobytes()) % 1000

    def encoder(self, mel):
        return torch.cat([self.feats(self.seed_of(m)) for m in mel]).to(mel.device).to(mel.dtype)


@pytest.fixture(scope="module")
def cond(gpu_device):
    c = _Conditioned(gpu_device)
    yield c
    for eng in list(c.model._engines.values()):
        eng.drop_cached_tasks()
    c.model._engines.clear()
    torch.cuda.empty_cache()


def test_one_window_equals_the_oracle_and_finds_the_planted_end(cond, gpu_device):
    """60 candidate tokens, 300 frames, 3 feature seeds, one call at the default end_slack.  (a) The device's own cost
    matrices fed to the oracle: the last column bit for bit, `end` and every jump equal.  (b) Against the planted ridge
    (condition_alignment defaults: position p is spoken at frame 12 + 11 p): `end` within 2 rows of
    floor((F - 1 - 12) / 11) - n_prefix = 23, n_prefix = 3 = the sot rows in front of the row that times the first text token.
    The CPU oracle on the fp32 model gives 24 for feature seeds 0 ... 11 at end_slack 0.005 ... 0.02 (FEAT_GAIN above)."""
    from whisper_amd.timing import find_alignment_open_batch
    text = cond.tok.encode(SENTENCE + SENTENCE)[:60]
    assert len(text) == 60
    feats = torch.cat([cond.feats(s) for s in (3, 4, 5)]).to(gpu_device)
    n_sot = len(cond.tok.sot_sequence)
    expect = (300 - 1 - FIRST_FRAME) // FRAMES_PER_TOKEN - n_sot
    assert expect == 23
    details = []
    got = find_alignment_open_batch(cond.model, cond.tok, [text] * 3, None, [600] * 3, [False] * 3, audio_features=feats,
                                    details=details)
    for b, d in enumerate(details):
        assert d["cost"].shape == (61, 300)
        want = ao.dtw_open(d["cost"], False, 0.01)
        print(f"seed {3 + b}: end {d['end']} oracle {want['end']} planted {expect}")
        assert d["end"] == want["end"] and np.array_equal(d["jumps"], want["jumps"]), b
        assert d["lastcol"].tobytes() == want["lastcol"].tobytes()
        words, n_tokens = got[b]
        assert n_tokens == sum(len(w.tokens) for w in words) < d["end"]
        assert abs(d["end"] - expect) <= 2, (b, d["end"], expect)


# ---- end to end --------------------------------------------------------------------------------------------------------
def _audio(seconds, seed):
    return (np.random.default_rng(seed).standard_normal(int(seconds * 16000)) * 0.05).astype(np.float32)


def _transcript(tok, n_tokens):
    """whole words of SENTENCE repeated, about n_tokens tokens"""
    al = sys.modules["whisper_amd.align"]
    words, _, _ = al._split_transcript(tok, SENTENCE * (n_tokens // 40 + 1), 219)
    out, n = [], 0
    for w in words:
        if n + len(w) > n_tokens:
            break
        out.append(w)
        n += len(w)
    return tok.decode([t for w in out for t in w]), out


FILES = [(70.0, 300, 21), (45.0, 150, 22), (20.0, 60, 23)]                # seconds, transcript tokens, audio seed


@pytest.fixture(scope="module")
def aligned(cond):
    """model.align on file 0, with the planted encoder installed"""
    import whisper_amd  # noqa: F401
    seconds, n_tokens, seed = FILES[0]
    text, words = _transcript(cond.tok, n_tokens)
    real = cond.model.encoder
    cond.model.encoder = cond.encoder
    try:
        result = cond.model.align(_audio(seconds, seed), text, language="en")
    finally:
        cond.model.encoder = real
    return text, words, result


def test_align_equals_the_oracle_walk(cond, aligned, gpu_device):
    """`model.align` on a synthetic 70 s file with a ~300-token transcript (fp16 engine) against the oracle walk on the fp32
    oracle model with the same planted features: the same windows, the same number of words accepted in each, every word
    start and end within one token-grid step (0.02 s)"""
    import whisper_amd
    from whisper_amd.audio import N_FRAMES, N_SAMPLES, pad_or_trim
    text, words, result = aligned
    seconds, _, seed = FILES[0]
    assert 280 <= sum(len(w) for w in words) <= 300
    mel = whisper_amd.log_mel_spectrogram(_audio(seconds, seed), cond.dims.n_mels, padding=N_SAMPLES, device=gpu_device)
    feats_of = lambda seek: cond.feats(cond.seed_of(pad_or_trim(mel[:, seek: seek + N_FRAMES], N_FRAMES)))
    aligner = ao.model_window_aligner(cond.om, cond.tok, words, feats_of, cond.heads, 0.01)
    cap = cond.dims.n_text_ctx // 2 - len(cond.tok.sot_sequence) - 2
    want = ao.walk([len(w) for w in words], mel.shape[-1] - N_FRAMES, cap, 100, aligner)
    print("windows", result["windows"])
    assert len(want["windows"]) == len(result["windows"]) == 3 and want["left_over"] == 0 and result["skipped_windows"] == 0
    assert [w["closed"] for w in result["windows"]] == [False, False, True]
    for got, w in zip(result["windows"], want["windows"]):
        assert (got["seek"], got["frames"], got["closed"], got["candidates"]) == (w["seek"], w["frames"], w["closed"], w["candidates"])
        assert got["accepted"] == len(w["times"]) > 0
    # merge_punctuations off for the word-by-word comparison: compare the raw walk through the segments' token counts
    flat = [(w["seek"] / 100.0 + s, w["seek"] / 100.0 + e) for w in want["windows"] for s, e in w["times"]]
    raw = sys.modules["whisper_amd.align"]
    real = cond.model.encoder
    cond.model.encoder = cond.encoder
    try:
        plain = raw.align(cond.model, _audio(seconds, seed), text, language="en", prepend_punctuations="", append_punctuations="")
    finally:
        cond.model.encoder = real
    got_words = [w for s in plain["segments"] for w in s["words"]]
    assert len(got_words) == len(flat) == len(words) and all(w["aligned"] for w in got_words)
    worst = max(max(abs(g["start"] - s), abs(g["end"] - e)) for g, (s, e) in zip(got_words, flat))
    print("worst word-time difference vs the oracle walk:", worst)
    assert worst <= 0.02 + 1e-6
    # against the planted ridge: the path changes from row r - 1 to row r between the frames the two rows are planted at, so
    # a word whose first token sits in row r of its window begins within half a token spacing, and one frame for the grid,
    # of the midpoint 12 + 11 (n_sot + r) - 5.5 (the oracle walk: at most 4.5 frames off).  Not asked of a window's first
    # word (the path starts at frame 0) nor of the last word of the closed window (the path is pinned to the window's end).
    n_sot, at, off = len(cond.tok.sot_sequence), 0, []
    for w in want["windows"]:
        row = 0
        for k in range(len(w["times"])):
            last_of_closed = w["closed"] and k == len(w["times"]) - 1
            if k > 0 and not last_of_closed:
                mid = FIRST_FRAME + FRAMES_PER_TOKEN * (n_sot + row) - FRAMES_PER_TOKEN / 2
                off.append(abs((got_words[at]["start"] - w["seek"] / 100.0) * 50 - mid))
            row += len(words[at])
            at += 1
    print("worst word start against the planted ridge, in frames:", max(off), "of", len(off), "words")
    assert len(off) >= len(words) - 4 and max(off) <= FRAMES_PER_TOKEN / 2 + 1
    # ... and each open window takes every word the planted ridge ends in front of its guard, give or take one
    for w in want["windows"][:2]:
        rows_in_front = (w["frames"] // 2 - 50 - FIRST_FRAME + FRAMES_PER_TOKEN // 2) // FRAMES_PER_TOKEN - n_sot
        fit, used = 0, 0
        while used + len(words[w["first"] + fit]) <= rows_in_front:
            used += len(words[w["first"] + fit])
            fit += 1
        print("window at", w["seek"], "accepted", len(w["times"]), "planted", fit)
        assert abs(len(w["times"]) - fit) <= 1
    assert plain["text"] == text and [w["word"] for w in got_words] == [cond.tok.decode(w) for w in words]
    starts = [w["start"] for w in got_words]
    assert all(b >= a for a, b in zip(starts, starts[1:])) and got_words[-1]["end"] <= seconds


def test_align_batch_equals_align_per_file(cond, aligned):
    """three files of different lengths walked in lock step (3, 2 and 1 windows): windows, words and times of `align` file by
    file; probabilities to the fp16 engine's batch-shape dependence (2e-2)"""
    import whisper_amd
    texts = [_transcript(cond.tok, n)[0] for _, n, _ in FILES]
    audios = [_audio(s, seed) for s, _, seed in FILES]
    real = cond.model.encoder
    cond.model.encoder = cond.encoder
    try:
        batch = whisper_amd.align_batch(cond.model, audios, texts, batch_size=24, language="en")
        single = [aligned[2]] + [cond.model.align(a, t, language="en") for a, t in zip(audios[1:], texts[1:])]
    finally:
        cond.model.encoder = real
    assert [len(r["windows"]) for r in batch] == [3, 2, 1]
    for b, s in zip(batch, single):
        assert b["windows"] == s["windows"] and b["text"] == s["text"] and b["skipped_windows"] == s["skipped_windows"] == 0
        assert len(b["segments"]) == len(s["segments"])
        for sb, ss in zip(b["segments"], s["segments"]):
            assert (sb["start"], sb["end"], sb["text"], sb["tokens"]) == (ss["start"], ss["end"], ss["text"], ss["tokens"])
            assert [(w["word"], w["start"], w["end"], w["aligned"]) for w in sb["words"]] == \
                   [(w["word"], w["start"], w["end"], w["aligned"]) for w in ss["words"]]
            assert all(abs(x["probability"] - y["probability"]) <= 2e-2 for x, y in zip(sb["words"], ss["words"]))


def test_list_of_lines_and_srt_writer(cond, aligned, tmp_path):
    """a List[str] transcript gives one segment per item; get_writer("srt") accepts both result shapes"""
    from whisper_amd.utils import get_writer
    text, words, result = aligned
    seconds, n_tokens, seed = FILES[2]
    _, w20 = _transcript(cond.tok, n_tokens)
    lines = [cond.tok.decode([t for w in w20[a: a + 7] for t in w]).strip() for a in range(0, len(w20), 7)]
    real = cond.model.encoder
    cond.model.encoder = cond.encoder
    try:
        by_line = cond.model.align(_audio(seconds, seed), lines, language="en")
    finally:
        cond.model.encoder = real
    assert [s["text"] for s in by_line["segments"]] == [" " + l for l in lines]
    assert all(s["start"] == s["words"][0]["start"] and s["end"] == s["words"][-1]["end"] for s in by_line["segments"])
    assert all(b["start"] >= a["end"] - 1e-9 for a, b in zip(by_line["segments"], by_line["segments"][1:]))
    for name, res in (("lines", by_line), ("text", result)):
        get_writer("srt", str(tmp_path))(res, f"{name}.wav")
        srt = (tmp_path / f"{name}.srt").read_text()
        assert srt.count("-->") == len(res["segments"]) and res["segments"][0]["text"].strip() in srt
