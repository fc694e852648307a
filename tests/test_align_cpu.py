"""Forced alignment without a GPU: the float32 oracle of the open-end DTW on hand-made matrices, the window walk of
whisper_amd/align.py against its restatement in tests/align_oracle.py with a fake aligner, and the argument checks."""
import sys

import numpy as np
import pytest

import align_oracle as ao
import oracle
import whisper_amd  # noqa: F401
from whisper_amd.tokenizer import get_tokenizer

al = sys.modules["whisper_amd.align"]            # the module: `whisper_amd.align` itself is the function


def _ridge(N, M, rows_inside, frames_per_row, tail_gain=0.0, seed=0):
    """cost matrix [N][M]: noise in [0, 0.1), -1 along a diagonal ridge that gives `frames_per_row` frames to each of the first
    `rows_inside` rows and reaches the last column there; the rows behind it gain `tail_gain` in the last column only"""
    x = np.random.default_rng(seed).random((N, M), dtype=np.float32) * np.float32(0.1)
    assert rows_inside * frames_per_row == M
    for i in range(rows_inside):
        x[i, i * frames_per_row: (i + 1) * frames_per_row] -= 1
    x[rows_inside:, M - 1] -= np.float32(tail_gain)
    return x


def test_oracle_closed_flag_takes_every_row_and_equals_the_plain_dtw():
    x = _ridge(12, 40, 8, 5)
    got = ao.dtw_open(x, True, 0.01)
    assert got["end"] == 12
    assert np.array_equal(got["trace"], oracle.dtw_trace(x))
    assert np.array_equal(got["path"], oracle.dtw_path(x))
    assert got["lastcol"].dtype == np.float32 and got["lastcol"].shape == (12,)


def test_oracle_ridge_leaves_the_window_at_a_known_row():
    """8 of 12 rows lie inside; every row behind them gains up to 0.1 in the last column (tail_gain 0.1 less noise in
    [0, 0.1)), so the arg-min is the last row, and the slack rule at end_slack 0.02 (2 % of |m| ~ 38 is 0.76 > 4 x 0.1)
    finds the row where the ridge ends"""
    x = _ridge(12, 40, 8, 5, tail_gain=0.1)
    lastcol = ao.dtw_open(x, False, 0.0)["lastcol"]
    assert int(np.argmin(lastcol)) + 1 == 12                          # the plateau drifts downwards: arg-min overshoots
    assert ao.dtw_open(x, False, 0.0)["end"] == 12                    # end_slack = 0 reproduces the arg-min
    got = ao.dtw_open(x, False, 0.02)
    assert got["end"] == 8, (got["end"], lastcol)
    assert len(got["jumps"]) == 8 and got["path"][0, -1] == 7 and got["path"][1, -1] == 39
    assert np.array_equal(got["jumps"], 5 * np.arange(8))             # the planted ridge, row by row


def test_oracle_slack_zero_is_the_first_argmin_and_ties_take_the_smallest_row():
    x = np.zeros((6, 4), dtype=np.float32)
    x[0] = -1                                   # D[1][M] = -4; every further row adds exactly 0: a six-way tie
    got = ao.dtw_open(x, False, 0.0)
    assert np.array_equal(got["lastcol"], np.full(6, -4, np.float32))
    assert got["end"] == 1
    x[3, 3] = -0.5                              # rows 4.. are better by 0.5: the smallest of THEM
    assert ao.dtw_open(x, False, 0.0)["end"] == 4
    assert ao.dtw_open(x, False, 0.125)["end"] == 1      # bound = -4.5 + 0.5625: the first plateau is inside it again
    empty = ao.dtw_open(np.zeros((0, 5), np.float32), False, 0.01)
    assert empty["end"] == 0 and empty["path"].shape == (2, 0)


# ---- the window walk ---------------------------------------------------------------------------------------------------
def _fake_aligner(seconds_per_word, lengths, silent=()):
    """every word takes `seconds_per_word`; a window holds the words that END inside it; windows starting in `silent`
    (seek ranges, frames) hold none"""
    calls = []

    def align_window(seek, frames, first, n, closed):
        calls.append((seek, frames, first, n, closed))
        if any(a <= seek < b for a, b in silent):
            return []
        out, t = [], 0.0
        for _ in range(n):
            if not closed and t + seconds_per_word > frames / 100.0:
                break
            out.append((round(t, 2), round(t + seconds_per_word, 2)))
            t += seconds_per_word
        return out

    return align_window, calls


def _drive(lengths, content_frames, cap, guard_frames, align_window):
    """whisper_amd.align._walk driven as align_batch drives it"""
    gen = al._walk([[0] * n for n in lengths], content_frames, cap, guard_frames)
    try:
        req = next(gen)
        while True:
            req = gen.send([(s, e, 0.5) for s, e in align_window(*req)])
    except StopIteration as stop:
        return stop.value


@pytest.mark.parametrize("content_s,n_words,silent", [(70, 150, ()), (70, 400, ()), (95, 150, ((2900, 6000),)), (12, 20, ())])
def test_walk_equals_the_oracle_walk(content_s, n_words, silent):
    lengths = [1 + (k % 3) for k in range(n_words)]
    cap, guard = 219, 100
    want = ao.walk(lengths, content_s * 100, cap, guard, _fake_aligner(0.4, lengths, silent)[0])
    windows, skipped = _drive(lengths, content_s * 100, cap, guard, _fake_aligner(0.4, lengths, silent)[0])
    assert skipped == want["skipped"] and len(windows) == len(want["windows"])
    for w, o in zip(windows, want["windows"]):
        assert (w["seek"], w["frames"], w["closed"], w["first"], w["candidates"]) == \
               (o["seek"], o["frames"], o["closed"], o["first"], o["candidates"])
        assert [t[:2] for t in w["times"]] == o["times"]


def test_walk_progress_last_window_closed_skip_and_left_over():
    lengths = [2] * 150
    # 0.4 s per word: 72 words end inside the first 29 s of a 30 s window
    windows, skipped = _drive(lengths, 7000, 219, 100, _fake_aligner(0.4, lengths)[0])
    assert skipped == 0 and [w["closed"] for w in windows] == [False, False, True]
    assert [len(w["times"]) for w in windows] == [72, 72, 6] and windows[1]["seek"] == 2880 and windows[1]["first"] == 72
    assert all(b["seek"] > a["seek"] for a, b in zip(windows, windows[1:]))
    assert windows[-1]["frames"] == 7000 - windows[-1]["seek"]           # content frames only
    assert windows[0]["candidates"] == 109                                # 109 two-token words <= 219 tokens
    # a silent stretch: the window that starts in it accepts nothing, seek moves by window - guard
    windows, skipped = _drive(lengths, 9500, 219, 100, _fake_aligner(0.4, lengths, ((2800, 5000),))[0])
    assert skipped == 1 and windows[1]["times"] == [] and windows[2]["seek"] == windows[1]["seek"] + 2900
    assert sum(len(w["times"]) for w in windows) == 150
    # more words than the audio holds: the walk ends with the audio, the rest is left over
    lengths = [2] * 400
    windows, skipped = _drive(lengths, 7000, 219, 100, _fake_aligner(0.4, lengths)[0])
    placed = sum(len(w["times"]) for w in windows)
    assert placed < 400 and not windows[-1]["closed"]
    assert ao.walk(lengths, 7000, 219, 100, _fake_aligner(0.4, lengths)[0])["left_over"] == 400 - placed


def _state(tok, text, windows, skipped, content_frames=7000):
    st = al._FileState.__new__(al._FileState)
    st.words, st.item, st.n_items = al._split_transcript(tok, text, 219)
    st.content_frames, st.outcome = content_frames, (windows, skipped)
    return st


def test_result_segments_for_str_and_list_and_left_over_words():
    tok = get_tokenizer(True, language="en", task="transcribe")
    text = ["Hello there, world.", "This is it!", "And a tail"]
    st = _state(tok, text, None, 0)
    assert st.n_items == 3 and [len([k for k in st.item if k == i]) for i in range(3)] == [5, 4, 3]
    times = [(0.5 * k, 0.5 * k + 0.5, 0.9) for k in range(12)]
    # window 0 takes 6 words (item 0 and the first word of item 1), window 1 three more; the last three are left over
    windows = [dict(seek=0, frames=3000, closed=False, first=0, candidates=12, times=times[:6]),
               dict(seek=300, frames=3000, closed=False, first=6, candidates=6, times=times[:3])]
    st.outcome = (windows, 0)
    res = al._result(tok, st, "en", "\"'“¿([{-", "\"'.。,，!！?？:：”)]}、")
    assert [s["text"] for s in res["segments"]] == [" Hello there, world.", " This is it!", " And a tail"]
    assert res["text"] == "".join(" " + t for t in text) and res["language"] == "en" and res["skipped_windows"] == 0
    s0, s1, s2 = res["segments"]
    assert [w["word"] for w in s0["words"]] == [" Hello", " there,", " world."]          # punctuation merged
    # (merge_punctuations glues text and tokens; the times stay the word's own, as in add_word_timestamps)
    assert (s0["start"], s0["end"]) == (0.0, 2.0) and s0["words"][1] == dict(word=" there,", start=0.5, end=1.0,
                                                                              probability=0.9, aligned=True)
    assert (s1["start"], s1["end"]) == (2.5, 4.0)                     # first word in window 0, the rest in window 1 (+3 s)
    assert [w["aligned"] for w in s2["words"]] == [False] * 3
    assert all((w["start"], w["end"], w["probability"]) == (70.0, 70.0, 0.0) for w in s2["words"])
    assert [w["accepted"] for w in res["windows"]] == [6, 3]
    # one str: a segment per window, the left-over words in one more
    st = _state(tok, " ".join(text), windows, 0)
    res = al._result(tok, st, "en", "", "")
    assert [len(s["words"]) for s in res["segments"]] == [6, 3, 3] and [s["seek"] for s in res["segments"]] == [0, 300, 0]
    assert res["segments"][1]["start"] == 3.0 and not any(w["aligned"] for w in res["segments"][2]["words"])
    # token ids are taken as they are
    ids = tok.encode(" Hello there")
    assert al._split_transcript(tok, ids, 219)[0] == [[i] for i in ids]


def test_an_empty_line_keeps_the_segments_in_order():
    """an empty item of a List[str] transcript: a segment without words, placed where the segment before it ends"""
    tok = get_tokenizer(True, language="en", task="transcribe")
    st = _state(tok, ["", "Hello there", "  ", "world"], None, 0)
    times = [(1.0 + 0.5 * k, 1.5 + 0.5 * k, 0.9) for k in range(3)]
    st.outcome = ([dict(seek=0, frames=3000, closed=True, first=0, candidates=3, times=times)], 0)
    res = al._result(tok, st, "en", "", "")
    assert [(s["start"], s["end"], len(s["words"])) for s in res["segments"]] == [(0.0, 0.0, 0), (1.0, 2.0, 2), (2.0, 2.0, 0),
                                                                                  (2.0, 2.5, 1)]
    assert all(b["start"] >= a["end"] for a, b in zip(res["segments"], res["segments"][1:]))


def test_argument_checks():
    tok = get_tokenizer(True, language="en", task="transcribe")
    with pytest.raises(ValueError):
        al.align_batch(None, ["a.wav"], [], batch_size=1)
    with pytest.raises(ValueError):
        al.align_batch(None, [], [], batch_size=0)
    with pytest.raises(ValueError):
        al.align_batch(None, [], [], guard_s=30.0)
    with pytest.raises(ValueError):
        al.align_batch(None, [], [], end_slack=-0.1)
    with pytest.raises(TypeError):
        al._split_transcript(tok, ["a", 3], 219)
    with pytest.raises(ValueError):
        al._split_transcript(tok, [tok.eot], 219)
    with pytest.raises(ValueError):
        al._split_transcript(tok, " word", 0)
    assert al._split_transcript(tok, "   ", 219)[0] == []
    from whisper_amd.timing import find_alignment_open_batch
    with pytest.raises(ValueError):
        find_alignment_open_batch(None, tok, [[1]], None, [3000], [])
    with pytest.raises(ValueError):
        find_alignment_open_batch(None, tok, [[1]], None, [3000], [False], end_slack=-1.0)
    assert find_alignment_open_batch(None, tok, [[], []], None, [3000, 10], [False, True]) == [([], 0), ([], 0)]
