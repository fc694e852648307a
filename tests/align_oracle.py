"""CPU oracle of forced alignment (whisper_amd/align.py, timing.find_alignment_open_batch): the open-end DTW in float32
numpy — accumulated cost of the last column, the slack rule for the end row, the walk from there — and the window walk
over a long file, written against an abstract "align this window" callable.  Every DTW cell is ONE float32 add of
x + min(three), as on the device, so the device's last column is expected bit for bit."""
import numpy as np

N_FRAMES = 3000                 # mel frames per window
FRAMES_PER_SECOND = 100
TOKENS_PER_SECOND = 50


def dtw_open(x: np.ndarray, closed: bool, end_slack: float) -> dict:
    """x float32 [N][M] -> {"lastcol" float32 [N] (D[i][M], i = 1..N), "end", "trace" int8 [N+1][M+1], "path" int [2][len]
    walked from (end, M), "jumps" int [end]: the frame at which each row is first reached}.  N == 0: end 0, empty path."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, M = x.shape
    if N == 0 or M == 0:
        return dict(lastcol=np.zeros(0, np.float32), end=0, trace=np.zeros((N + 1, M + 1), np.int8),
                    path=np.zeros((2, 0), np.int64), jumps=np.zeros(0, np.int64))
    D = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    D[0, 0] = 0
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    # anti-diagonal by anti-diagonal (cells of one diagonal are independent): the three-way rule of whisper/timing.py:95-100
    # (c0 strictly smallest, then c1 strictly smallest, else c2), one float32 add per cell
    for k in range(2, N + M + 1):
        i = np.arange(max(1, k - M), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.int8)
        cm = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        D[i, j] = x[i - 1, j - 1] + cm                  # float32 + float32 -> float32
        trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    lastcol = D[1:, M].copy()
    if closed:
        end = N
    else:
        m = np.float32(lastcol.min())
        bound = np.float32(m + np.float32(np.float32(end_slack) * np.abs(m)))
        end = int(np.nonzero(lastcol <= bound)[0][0]) + 1
    i, j, path = end, M, []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = 2 if i == 0 else 1 if j == 0 else trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path, dtype=np.int64)[::-1].T
    first = np.pad(np.diff(path[0]), (1, 0), constant_values=1).astype(bool)
    return dict(lastcol=lastcol, end=end, trace=trace, path=path, jumps=path[1][first])


def words_in_front_of(word_lengths, jumps):
    """[(start_s, end_s)] of the leading words whose rows, and the row that ends them, lie in front of row len(jumps)"""
    out, at = [], 0
    for n in word_lengths:
        if at + n >= len(jumps):
            break
        out.append((jumps[at] / TOKENS_PER_SECOND, jumps[at + n] / TOKENS_PER_SECOND))
        at += n
    return out


def walk(word_lengths, content_frames: int, cap: int, guard_frames: int, align_window):
    """The window walk.  `align_window(seek, frames, first, n, closed)` -> [(start_s, end_s), ...] of the leading
    candidates it places in the window, relative to the window.  Returns {"windows": [{seek, frames, closed, first,
    candidates, times}], "skipped", "left_over": words the audio ended before}."""
    windows, skipped, cursor, seek = [], 0, 0, 0
    n_words = len(word_lengths)
    while cursor < n_words and content_frames - seek >= 2:
        frames = min(N_FRAMES, content_frames - seek)
        n, used = 0, 0
        while cursor + n < n_words and used + word_lengths[cursor + n] <= cap:
            used += word_lengths[cursor + n]
            n += 1
        closed = cursor + n == n_words and seek + N_FRAMES >= content_frames
        times = list(align_window(seek, frames, cursor, n, closed))[:n]
        if not closed:
            limit = (frames - guard_frames) / FRAMES_PER_SECOND
            times = [t for k, t in enumerate(times) if all(u[1] <= limit + 1e-9 for u in times[: k + 1])]
        windows.append(dict(seek=seek, frames=frames, closed=closed, first=cursor, candidates=n, times=times))
        if times:
            cursor += len(times)
            seek += 2 * int(round(times[-1][1] * TOKENS_PER_SECOND))
        else:
            skipped += 1
            if closed or frames - guard_frames < 2:
                break
            seek += frames - guard_frames
    return dict(windows=windows, skipped=skipped, left_over=n_words - cursor)


def model_window_aligner(om, tokenizer, words, feats_of_window, heads, end_slack: float, medfilt_width: int = 7):
    """`align_window` for `walk` on the fp32 oracle model: teacher-forced pass over [sot, <|notimestamps|>, candidates, eot],
    oracle.alignment_matrix over the window's frames, dtw_open.  `feats_of_window(seek)` -> (1, n_audio_ctx, D) features."""
    import torch

    import oracle
    n_sot = len(tokenizer.sot_sequence)

    def align_window(seek, frames, first, n, closed):
        cand = words[first: first + n]
        text = [t for w in cand for t in w]
        if not text:
            return []
        tokens = [*tokenizer.sot_sequence, tokenizer.no_timestamps, *text, tokenizer.eot]
        with torch.no_grad():
            matrix, _ = oracle.alignment_matrix(om, tokens, feats_of_window(seek), frames, heads, n_sot, medfilt_width)
        got = dtw_open(-matrix, closed, end_slack)
        return words_in_front_of([len(w) for w in cand], got["jumps"])

    return align_window
