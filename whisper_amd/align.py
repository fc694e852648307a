"""Forced alignment: word times for a transcript the caller already has (no counterpart in the reference).

    result  = model.align("talk.flac", text, language="en")             # str, List[str] (one segment per item) or token ids
    results = whisper.align_batch(model, files, texts, batch_size=24)    # many files in lock step

No decode loop runs: every 30 s window costs one encoder pass and one teacher-forced prefill of the NEXT candidate words of
the transcript, and an open-end DTW (timing.find_alignment_open_batch) decides how many of them are spoken inside the
window.  The walk over the windows:

  1. the whole-file log-mel spectrogram is computed once (as transcribe_chunked does; `device_ingest` likewise);
  2. the transcript is split into words (tokenizer.split_to_word_tokens);
  3. at `seek`, the candidates are the whole words from the cursor on while their token count stays
     <= n_text_ctx // 2 - len(sot_sequence) - 2;
  4. the window is CLOSED when the candidates are all the remaining words and the window reaches the end of the content:
     every candidate is aligned inside the content frames;
  5. otherwise it is OPEN: of the words the open-end DTW returns, those that end at or before
     (window length - guard_s) are accepted — the last second of a window is where a word may be cut;
  6. `seek` moves to the end of the last accepted word (on the 0.02 s token grid);
  7. when no word is accepted, `seek` moves on by (window - guard) and result["skipped_windows"] counts it;
  8. words left over when the audio ends are appended at the end of the audio with zero duration, probability 0.0 and
     "aligned": False.

`guard_s` (1.0 s) is unmeasured.  `end_slack` (0.01) is the best of {0.002, 0.005, 0.01, 0.02} on ONE synthetic,
alignment-conditioned 4-layer checkpoint (profiles/align_ab.txt): there it finds the planted end within one row when every
spoken row gains about 40 cost units, and overshoots by tens of rows when the planted features are so strong that the
rows behind the end find a ridge of their own inside the window.  The guard is what keeps such surplus
rows out of the result.  Nothing is claimed about accuracy on real speech.  tests/align_oracle.py restates the walk on
the CPU.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, List, Optional, Sequence, Union

import numpy as np
import torch

from .audio import FRAMES_PER_SECOND, N_FRAMES, N_SAMPLES, TOKENS_PER_SECOND, ingest_options, load_audio, log_mel_spectrogram, pad_or_trim
from .timing import WordTiming, find_alignment_open_batch, merge_punctuations
from .tokenizer import LANGUAGES, Tokenizer, get_tokenizer

if TYPE_CHECKING:
    from .model import Whisper

Text = Union[str, Sequence[str], Sequence[int]]
FRAMES_PER_TOKEN = FRAMES_PER_SECOND // TOKENS_PER_SECOND          # 2 mel frames per 0.02 s


def _check_arguments(batch_size: int, guard_s: float, end_slack: float) -> None:
    if batch_size < 1:
        raise ValueError(f"batch_size must be at least 1 (got {batch_size})")
    if not 0.0 <= guard_s < N_FRAMES / FRAMES_PER_SECOND:
        raise ValueError(f"guard_s must lie in [0, 30) seconds (got {guard_s})")
    if not end_slack >= 0.0:
        raise ValueError(f"end_slack must be >= 0 (got {end_slack})")


def _split_transcript(tokenizer: Tokenizer, text: Text, cap: int):
    """-> (words: token list per word, item: index of the text item each word belongs to, n_items or None for one text)"""
    if isinstance(text, str):
        items, n_items = [tokenizer.encode(" " + text.strip())] if text.strip() else [[]], None
    elif len(text) > 0 and all(isinstance(t, str) for t in text):
        items, n_items = [tokenizer.encode(" " + t.strip()) if t.strip() else [] for t in text], len(text)
    elif all(isinstance(t, (int, np.integer)) for t in text):
        items, n_items = [[int(t) for t in text]], None
        if any(t < 0 or t >= tokenizer.eot for t in items[0]):
            raise ValueError("token ids must be text tokens (0 <= id < <|endoftext|>)")
    else:
        raise TypeError("text must be a str, a list of str (one segment per item) or a list of token ids")
    words, item = [], []
    for k, toks in enumerate(items):
        if not toks:
            continue
        _, word_tokens = tokenizer.split_to_word_tokens(list(toks) + [tokenizer.eot])
        for wt in word_tokens[:-1]:
            if len(wt) > cap:
                raise ValueError(f"a single word of {len(wt)} tokens does not fit one window ({cap} candidate tokens)")
            if wt:
                words.append(list(wt))
                item.append(k)
    return words, item, n_items


def _walk(words: List[List[int]], content_frames: int, cap: int, guard_frames: int):
    """The window walk of the module docstring as a generator: yields (seek, frames, first word, words, closed) for the
    next window — in mel frames — and is sent [(start_s, end_s, probability), ...] of the leading candidate words the
    open-end DTW placed inside it (times relative to the window).  Returns (windows, skipped): per window a dict with
    "seek", "frames", "closed", "first", "candidates" and "times" (of the accepted words)."""
    windows, skipped = [], 0
    cursor, seek = 0, 0
    while cursor < len(words) and content_frames - seek >= FRAMES_PER_TOKEN:
        frames = min(N_FRAMES, content_frames - seek)
        n, used = 0, 0
        while cursor + n < len(words) and used + len(words[cursor + n]) <= cap:
            used += len(words[cursor + n])
            n += 1
        closed = cursor + n == len(words) and seek + N_FRAMES >= content_frames
        times = yield seek, frames, cursor, n, closed
        times = list(times)[:n]
        if not closed:
            limit = (frames - guard_frames) / FRAMES_PER_SECOND
            k = 0
            while k < len(times) and times[k][1] <= limit + 1e-9:
                k += 1
            times = times[:k]
        windows.append(dict(seek=seek, frames=frames, closed=closed, first=cursor, candidates=n, times=times))
        if times:
            cursor += len(times)
            seek += int(round(times[-1][1] * TOKENS_PER_SECOND)) * FRAMES_PER_TOKEN
        else:
            skipped += 1
            if closed or frames - guard_frames < FRAMES_PER_TOKEN:
                break
            seek += frames - guard_frames
    return windows, skipped


class _FileState:
    def __init__(self, mel: torch.Tensor, words, item, n_items, cap: int, guard_frames: int):
        self.mel, self.words, self.item, self.n_items = mel, words, item, n_items
        self.content_frames = mel.shape[-1] - N_FRAMES
        self.gen = _walk(words, self.content_frames, cap, guard_frames)
        self.request, self.outcome = None, None
        self.advance(None)

    def advance(self, value) -> None:
        try:
            self.request = self.gen.send(value) if value is not None else next(self.gen)
        except StopIteration as stop:
            self.request, self.outcome = None, stop.value


def _step(model: "Whisper", tokenizer: Tokenizer, states: List[_FileState], dtype: torch.dtype, end_slack: float,
          medfilt_width: int, qk_scale: float) -> None:
    """one window of every live file: ONE encoder call on the batch of windows, ONE find_alignment_open_batch call"""
    mels, tokens, frames, closed = [], [], [], []
    for st in states:
        seek, n_frames, first, n, is_closed = st.request
        mels.append(pad_or_trim(st.mel[:, seek: seek + N_FRAMES], N_FRAMES))
        tokens.append([t for w in st.words[first: first + n] for t in w])
        frames.append(n_frames)
        closed.append(is_closed)
    features = model.encoder(torch.stack(mels).to(model.device).to(dtype))
    found = find_alignment_open_batch(model, tokenizer, tokens, None, frames, closed, end_slack=end_slack,
                                      medfilt_width=medfilt_width, qk_scale=qk_scale, audio_features=features)
    for st, (timings, _) in zip(states, found):
        _, _, first, n, _ = st.request
        st.advance(_times_of_candidates(timings, st.words[first: first + n]))


def _times_of_candidates(timings: List[WordTiming], candidates: List[List[int]]):
    """(start, end, probability) of the leading candidate words, read off the returned words by token boundaries (the split
    of a window's tokens is that of the whole transcript wherever a word boundary falls on one of its own)"""
    begin_of, end_of, at = {}, {}, 0
    for k, w in enumerate(timings):
        begin_of[at] = k
        at += len(w.tokens)
        end_of[at] = k
    out, at = [], 0
    for cand in candidates:
        a, b = at, at + len(cand)
        if a not in begin_of or b not in end_of:
            break
        ws = timings[begin_of[a]: end_of[b] + 1]
        n_tok = sum(len(w.tokens) for w in ws)
        out.append((ws[0].start, ws[-1].end, float(sum(w.probability * len(w.tokens) for w in ws) / n_tok)))
        at = b
    return out


def _result(tokenizer: Tokenizer, st: _FileState, language: str, prepend_punctuations: str, append_punctuations: str) -> dict:
    windows, skipped = st.outcome
    end_of_audio = round(st.content_frames / FRAMES_PER_SECOND, 2)
    # (segment key, WordTiming in absolute time, aligned) in transcript order
    placed = []
    for wi, win in enumerate(windows):
        offset = win["seek"] / FRAMES_PER_SECOND
        for k, (start, end, prob) in enumerate(win["times"]):
            g = win["first"] + k
            toks = st.words[g]
            key = st.item[g] if st.n_items is not None else wi
            placed.append((key, WordTiming(tokenizer.decode(toks), list(toks), offset + start, offset + end, prob), True))
    for g in range(len(placed), len(st.words)):
        toks = st.words[g]
        key = st.item[g] if st.n_items is not None else len(windows)
        placed.append((key, WordTiming(tokenizer.decode(toks), list(toks), end_of_audio, end_of_audio, 0.0), False))
    segments = []
    keys = range(st.n_items) if st.n_items is not None else sorted({key for key, _, _ in placed})
    for key in keys:
        group = [(w, ok) for k, w, ok in placed if k == key]
        tokens = [t for w, _ in group for t in w.tokens]
        aligned = {id(w): ok for w, ok in group}
        # punctuation is glued within runs of aligned words only: a left-over word keeps its flag
        for run in (True, False):
            merge_punctuations([w for w, ok in group if ok == run], prepend_punctuations, append_punctuations)
        words = [dict(word=w.word, start=round(w.start, 2), end=round(w.end, 2), probability=w.probability,
                      aligned=aligned[id(w)]) for w, _ in group if w.word]
        seek = windows[key]["seek"] if st.n_items is None and key < len(windows) else 0
        # an item without words (an empty line) sits where the segment before it ends: segment times stay in order
        empty_at = segments[-1]["end"] if segments else 0.0
        segments.append(dict(id=len(segments), seek=seek, start=words[0]["start"] if words else empty_at,
                             end=words[-1]["end"] if words else empty_at, text=tokenizer.decode(tokens), tokens=tokens,
                             words=words))
    return dict(text="".join(s["text"] for s in segments), segments=segments, language=language,
                skipped_windows=skipped,
                windows=[dict(seek=w["seek"], frames=w["frames"], closed=w["closed"], candidates=w["candidates"],
                              accepted=len(w["times"])) for w in windows])


def align_batch(model: "Whisper", audios: Sequence[Union[str, np.ndarray, torch.Tensor]], texts: Sequence[Text], *,
                batch_size: int = 24, language: Optional[str] = None, fp16: bool = True, guard_s: float = 1.0,
                end_slack: float = 0.01, medfilt_width: int = 7, qk_scale: float = 1.0, device_ingest: bool = False,
                prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、") -> List[dict]:
    """`align` for many files, walked in lock step: every step is one encoder call and one find_alignment_open_batch call for
    the next window of up to `batch_size` files (within one file the walk is sequential: a window's start is the end of the
    last word of the window before).  Results equal `align` file by file.  `language`: one for all files; None detects it on
    the first 30 s of every file (multilingual models)."""
    if len(audios) != len(texts):
        raise ValueError(f"{len(audios)} audio inputs but {len(texts)} transcripts")
    _check_arguments(batch_size, guard_s, end_slack)
    dtype = torch.float16 if fp16 and model.device != torch.device("cpu") else torch.float32
    guard_frames = int(round(guard_s * TOKENS_PER_SECOND)) * FRAMES_PER_TOKEN
    results: List[Optional[dict]] = [None] * len(audios)
    ingest = ingest_options(device_ingest)       # False / True / "decode", as in transcribe
    waiting = list(range(len(audios)))
    live: List[tuple] = []                       # (file index, state, tokenizer, language)

    def admit() -> None:
        while waiting and len(live) < batch_size:
            i = waiting.pop(0)
            audio = audios[i]
            if ingest is not None and isinstance(audio, str):
                audio = load_audio(audio, device=model.device, **ingest)
            mel = log_mel_spectrogram(audio, model.dims.n_mels, padding=N_SAMPLES, device=model.device)
            lang = language
            if lang is None:
                if model.is_multilingual:
                    _, probs = model.detect_language(pad_or_trim(mel, N_FRAMES).to(model.device).to(dtype))
                    lang = max(probs, key=probs.get)
                else:
                    lang = "en"
            elif lang.lower() not in LANGUAGES:
                lang = get_tokenizer(True, language=lang).language        # a language NAME: validated and mapped to its code
            tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=lang,
                                      task="transcribe")
            cap = model.dims.n_text_ctx // 2 - len(tokenizer.sot_sequence) - 2
            state = _FileState(mel, *_split_transcript(tokenizer, texts[i], cap), cap, guard_frames)
            live.append((i, state, tokenizer, lang))

    admit()
    while live:
        for entry in [e for e in live if e[1].request is None]:
            i, state, tokenizer, lang = entry
            results[i] = _result(tokenizer, state, lang, prepend_punctuations, append_punctuations)
            live.remove(entry)
        admit()
        todo = [e for e in live if e[1].request is not None]
        # one call per tokenizer (the sot sequence carries the language)
        for lang in sorted({e[3] for e in todo}):
            group = [e for e in todo if e[3] == lang]
            _step(model, group[0][2], [e[1] for e in group], dtype, end_slack, medfilt_width, qk_scale)
    return results


def align(model: "Whisper", audio: Union[str, np.ndarray, torch.Tensor], text: Text, **kwargs) -> dict:
    """Word times for `text` — a str, a list of str (one segment per item) or a list of text token ids — spoken in `audio`
    (what `transcribe` accepts).  Returns the dict `transcribe(word_timestamps=True)` returns — `text`, `segments` with
    `words` (each with "aligned": False only where the audio ended before the word), `language` — so `get_writer` works
    on it, plus `skipped_windows` and `windows` (seek, frames, closed, candidates, accepted of every window walked).
    A str or token-id text gives one segment per window.  Keywords: `language`, `fp16`, `guard_s` (1.0: words ending in the
    last second of an open window are left to the next one), `end_slack` (0.01, see find_alignment_open_batch),
    `medfilt_width`, `qk_scale`, `device_ingest`, `prepend_punctuations`, `append_punctuations`."""
    kwargs.pop("batch_size", None)
    return align_batch(model, [audio], [text], batch_size=1, **kwargs)[0]
