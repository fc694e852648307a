"""One long recording: `model.transcribe(x)` (a 1-row decode chain from start to end) against
`model.transcribe_chunked(x, batch_size=24)` (the file cut at pauses, the chunks' windows decoded as 24-row chains), in one
process, on large-v3 dimensions with synthetic weights and a 20-minute signal built like the chunking tests' signal
(bursts of 3 - 12 s separated by gaps of 0.6 - 2.0 s).  temperature 0, thresholds off, fixed sample_len, fp16 engine.
Both legs run once untimed (every shape warmed), then alternate three times; a host clock around calls that end in a
synchronise.  With synthetic weights the timestamp tokens that drive `seek` are arbitrary, so the two legs decode different
numbers of windows: time per window is printed beside the totals.

    python tools/chunked_ab.py [minutes=20] [sample_len=64] [batch_size=24]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chunk_oracle import make_signal                                     # noqa: E402
from whisper_amd.decoding import DecodingTask                            # noqa: E402
from whisper_amd.model import ModelDimensions, Whisper                   # noqa: E402
from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict   # noqa: E402

minutes = float(sys.argv[1]) if len(sys.argv) > 1 else 20.0
sample_len = int(sys.argv[2]) if len(sys.argv) > 2 else 64
batch_size = int(sys.argv[3]) if len(sys.argv) > 3 else 24
assert torch.cuda.is_available(), "chunked_ab.py measures on the GPU"
dev = torch.device("cuda:0")

dims = dims_for("large-v3")
model = Whisper(ModelDimensions(**dims_dict(dims)), synthetic_state_dict(dims, seed=0, device=dev), device=dev)
x, _ = make_signal(gap_noise=1e-4, n_bursts=int(minutes * 60 / 8.8))    # a burst and its gap last 8.8 s on average
seconds = len(x) / 16000.0
kw = dict(language="en", temperature=0.0, fp16=True, sample_len=sample_len, no_speech_threshold=None, logprob_threshold=None,
          compression_ratio_threshold=None)

rows = []
run = DecodingTask.run


def counted(self, mel):
    rows.append(int(mel.shape[0]))
    return run(self, mel)


DecodingTask.run = counted


def leg(chunked: bool):
    del rows[:]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.transcribe_chunked(x, batch_size=batch_size, **kw) if chunked else model.transcribe(x, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, sum(rows), max(rows), len(rows), out


print(f"large-v3 dims (synthetic weights, fp16), {seconds:.0f} s of audio, sample_len {sample_len}, batch_size {batch_size}", flush=True)
for chunked in (False, True):                                            # untimed: every shape of both legs
    t, windows, widest, calls, out = leg(chunked)
    print(f"warm-up {'chunked' if chunked else 'transcribe'}: {t:.2f} s, {windows} windows in {calls} decode calls, widest "
          f"{widest} rows" + (f", {len(out['chunks'])} chunks" if chunked else ""), flush=True)
times = {False: [], True: []}
per_window = {False: [], True: []}
for rep in range(3):
    for chunked in (False, True):
        t, windows, widest, calls, _ = leg(chunked)
        times[chunked].append(t)
        per_window[chunked].append(t / windows)
        print(f"run {rep} {'transcribe_chunked' if chunked else 'transcribe        '}: {t:7.3f} s wall, {windows:4d} windows in "
              f"{calls:4d} calls (widest {widest:2d} rows), {seconds / t:7.1f} audio-s/s, {1e3 * t / windows:7.2f} ms per window",
              flush=True)
for chunked in (False, True):
    ts = times[chunked]
    print(f"{'transcribe_chunked' if chunked else 'transcribe        '}: median {seconds / np.median(ts):.1f} audio-s/s "
          f"({np.median(ts):.3f} s), spread over repeats {100 * (max(ts) - min(ts)) / min(ts):.1f} %, "
          f"{1e3 * np.median(per_window[chunked]):.2f} ms per window")
print(f"chunked / sequential: {np.median(times[False]) / np.median(times[True]):.2f} x audio-s/s, "
      f"{np.median(per_window[False]) / np.median(per_window[True]):.2f} x per window")
