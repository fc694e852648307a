"""The result writers (txt / vtt / srt / tsv / json) against the reference's on randomly
generated transcripts with word timings, for every combination of the subtitle layout options.  CPU only; the reference's
outputs are stored in tests/golden/writers_reference.pt.gz (tests/refgolden.py, tests/golden/make_golden_host.py)."""
import io
import itertools
import json
import random

import pytest
from refgolden import raises, store_fixture

from whisper_amd import utils as U


def _result(seed, with_words=True):
    rnd = random.Random(seed)
    vocab = ["the", "a", "quick", "brown", "fox", "jumps", "over", "lazy", "dog,", "and", "then", "-->", "it's", "über",
             "naïve", "tab\there", "end."]
    t, segments = rnd.uniform(0, 2), []
    for _ in range(rnd.randint(1, 7)):
        words = []
        if rnd.random() < 0.3:
            t += rnd.uniform(3.1, 6.0)                     # long pause between segments
        for _ in range(rnd.randint(0 if rnd.random() < 0.2 else 1, 14)):
            d = rnd.uniform(0.05, 0.6)
            words.append({"word": " " + rnd.choice(vocab), "start": round(t, 2), "end": round(t + d, 2),
                          "probability": rnd.random()})
            t += d + (rnd.uniform(3.2, 4.0) if rnd.random() < 0.05 else rnd.uniform(0, 0.2))
        seg = {"id": len(segments), "seek": 0, "start": words[0]["start"] if words else round(t, 2),
               "end": words[-1]["end"] if words else round(t, 2), "text": "".join(w["word"] for w in words),
               "tokens": [1, 2, 3], "temperature": 0.0, "avg_logprob": -0.3, "compression_ratio": 1.2,
               "no_speech_prob": 0.01}
        if with_words:
            seg["words"] = words
        segments.append(seg)
    return {"text": "".join(s["text"] for s in segments), "segments": segments, "language": "en"}


_store = store_fixture("writers_reference")


@pytest.fixture
def ref_utils(_store):
    """the reference's whisper.utils while recording; None otherwise (it is only read inside expect(...))"""
    return None if _store.ref is None else _store.ref.utils


@pytest.fixture
def expect(_store, request):
    return _store.expect_for(request.node.name)


def test_writers_match_reference(ref_utils, expect, tmp_path):
    grids = list(itertools.product([None, 12, 28, 60], [None, 1, 2, 3], [False, True], [None, 1, 3, 5]))
    for seed in range(12):
        for with_words in (True, False):
            res = _result(seed, with_words)
            for fmt in ("txt", "vtt", "srt", "tsv", "json"):
                cases = grids if fmt in ("vtt", "srt") else grids[:1]

                def theirs():
                    outs = []
                    for width, lines, hl, per_line in cases:
                        kw = dict(max_line_width=width, max_line_count=lines, highlight_words=hl, max_words_per_line=per_line)
                        out = io.StringIO()
                        ref_utils.get_writer(fmt, str(tmp_path)).write_result(res, file=out, options=dict(kw))
                        outs.append(out.getvalue())
                    return outs
                for (width, lines, hl, per_line), theirs_text in zip(cases, expect(theirs), strict=True):
                    kw = dict(max_line_width=width, max_line_count=lines, highlight_words=hl, max_words_per_line=per_line)
                    mine = io.StringIO()
                    U.get_writer(fmt, str(tmp_path)).write_result(res, file=mine, options=dict(kw))
                    assert mine.getvalue() == theirs_text, (seed, with_words, fmt, kw)
    # keyword arguments instead of the options dict, and the file-naming __call__ / "all" paths
    res = _result(99)
    a = io.StringIO()
    U.WriteSRT(str(tmp_path)).write_result(res, file=a, max_line_width=20, max_line_count=2, highlight_words=True)

    def theirs_srt():
        b = io.StringIO()
        ref_utils.WriteSRT(str(tmp_path)).write_result(res, file=b, max_line_width=20, max_line_count=2, highlight_words=True)
        return b.getvalue()
    assert a.getvalue() == expect(theirs_srt)
    (tmp_path / "mine").mkdir()
    U.get_writer("all", str(tmp_path / "mine"))(res, "/some/dir/clip.flac", {"max_line_width": 30, "max_line_count": 2})

    def theirs_files():
        (tmp_path / "ref").mkdir()
        ref_utils.get_writer("all", str(tmp_path / "ref"))(res, "/some/dir/clip.flac", {"max_line_width": 30, "max_line_count": 2})
        return {ext: (tmp_path / "ref" / f"clip.{ext}").read_text(encoding="utf-8") for ext in ("txt", "vtt", "srt", "tsv", "json")}
    theirs_all = expect(theirs_files)
    for ext in ("txt", "vtt", "srt", "tsv", "json"):
        assert (tmp_path / "mine" / f"clip.{ext}").read_text(encoding="utf-8") == theirs_all[ext]


def test_writers_known_output():
    """runs anywhere: a hand-checked transcript"""
    res = {"text": " Hello world. Bye", "language": "en", "segments": [
        {"start": 0.0, "end": 1.5, "text": " Hello world.", "words": [
            {"word": " Hello", "start": 0.0, "end": 0.6, "probability": 0.9},
            {"word": " world.", "start": 0.7, "end": 1.5, "probability": 0.8}]},
        {"start": 5.0, "end": 5.4, "text": " Bye", "words": [{"word": " Bye", "start": 5.0, "end": 5.4, "probability": 0.7}]}]}
    out = io.StringIO()
    U.WriteVTT(".").write_result(res, file=out)
    assert out.getvalue() == "WEBVTT\n\n00:00.000 --> 00:01.500\nHello world.\n\n00:05.000 --> 00:05.400\nBye\n\n"
    out = io.StringIO()
    U.WriteSRT(".").write_result(res, file=out, highlight_words=True)
    assert out.getvalue().startswith("1\n00:00:00,000 --> 00:00:00,600\n<u>Hello</u> world.\n\n2\n00:00:00,600 --> 00:00:00,700\nHello world.\n\n"
                                     "3\n00:00:00,700 --> 00:00:01,500\nHello <u>world.</u>\n\n4\n00:00:05,000 --> 00:00:05,400\n<u>Bye</u>\n\n")
    out = io.StringIO()
    U.WriteTSV(".").write_result(res, file=out)
    assert out.getvalue() == "start\tend\ttext\n0\t1500\tHello world.\n5000\t5400\tBye\n"
    out = io.StringIO()
    U.WriteTXT(".").write_result(res, file=out)
    assert out.getvalue() == "Hello world.\nBye\n"
    out = io.StringIO()
    U.WriteJSON(".").write_result(res, file=out)
    assert json.loads(out.getvalue()) == res
    with pytest.raises(KeyError):
        U.get_writer("docx", ".")


def test_small_helpers_match_reference(ref_utils, expect):
    """exact_div, compression_ratio, format_timestamp, get_start / get_end (utils.py:24-82) on random inputs"""
    RU = ref_utils
    rnd = random.Random(9)
    for _ in range(200):
        y, k = rnd.randint(1, 50), rnd.randint(0, 99)
        assert U.exact_div(y * k, y) == expect(lambda: RU.exact_div(y * k, y)) == k
    for x, y in ((480000, 160), (3000, 2), (0, 7)):
        assert U.exact_div(x, y) == expect(lambda: RU.exact_div(x, y))
    for bad in ((10, 3), (7, 2)):
        with pytest.raises(AssertionError):
            U.exact_div(*bad)
        assert expect(lambda: raises(AssertionError, lambda: RU.exact_div(*bad))) is not None
    words = ["the", "quick", "über", "naïve", "日本語", "a", " ", "\n", "and and and and"]
    for _ in range(100):
        text = " ".join(rnd.choice(words) for _ in range(rnd.randint(1, 60)))
        assert U.compression_ratio(text) == expect(lambda: RU.compression_ratio(text))
    for _ in range(300):
        s = rnd.choice([0.0, rnd.uniform(0, 70), rnd.uniform(3500, 3700), rnd.uniform(0, 1e5), 59.9996, 3599.9999])
        for hours, mark in ((False, "."), (True, ","), (False, ","), (True, ".")):
            assert U.format_timestamp(s, hours, mark) == expect(lambda: RU.format_timestamp(s, hours, mark))
    with pytest.raises(AssertionError):
        U.format_timestamp(-1.0)
    for seed in range(40):
        segs = _result(seed)["segments"]                  # both index s["words"]: word-timed segments only
        assert (U.get_start(segs), U.get_end(segs)) == expect(lambda: (RU.get_start(segs), RU.get_end(segs)))
        empty = [dict(s, words=[]) for s in segs]
        assert (U.get_start(empty), U.get_end(empty)) == expect(lambda: (RU.get_start(empty), RU.get_end(empty)))
    assert (U.get_start([]), U.get_end([])) == expect(lambda: (RU.get_start([]), RU.get_end([])))
