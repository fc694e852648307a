"""Timing of forced alignment (whisper_amd/align.py) against transcribe(word_timestamps=True) on the same audio, and the
`end`-vs-planted error of the open-end DTW for several `end_slack` values.

    python tools/align_ab.py [--model large-v3] [--files 24] [--seconds 120] [--runs 3] [--skip-transcribe]

Part 1: seeded synthetic weights, synthetic audio, fp16 engine; `align` of one file, `align_batch` of --files files, and
`transcribe(word_timestamps=True, sample_len 64)` of one file — the decode route that existed before, unchanged by this feature —
each as wall time after a warm-up, median of --runs.  The transcript aligned is arbitrary text (random-init weights say
nothing about where it is spoken): the figure is throughput, not accuracy.
Part 2: the 4-layer alignment-conditioned checkpoint of tests/test_align_gpu.py (oracle/condition.py), 60 candidate tokens,
300 frames, feature seeds 0..--seeds: histogram of end - planted for end_slack in {0.002, 0.005, 0.01, 0.02, 0.1}, once
with planted features at unit gain (a spoken row gains ~40 cost units: the regime the slack rule is meant for) and once at
alignment_features' default gain 4 (the time code's side lobes become ridges of their own).
One JSON line per result; keep the output in profiles/align_ab.txt."""
import argparse
import base64
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import whisper_amd                                                            # noqa: E402
from whisper_amd.model import ModelDimensions, Whisper                        # noqa: E402
from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict   # noqa: E402
from whisper_amd.tokenizer import get_tokenizer                               # noqa: E402

SENTENCE = " the quick brown fox jumps over the lazy dog and keeps running for a while longer than anyone expected it to."


def timed(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out)


def part_timing(a, dev):
    dims = dims_for(a.model)
    model = Whisper(ModelDimensions(**dims_dict(dims)), synthetic_state_dict(dims, seed=0, device=dev), device=dev)
    rng = np.random.default_rng(0)
    audios = [(rng.standard_normal(int(a.seconds * 16000)) * 0.05).astype(np.float32) for _ in range(a.files)]
    text = SENTENCE * int(a.seconds / 60.0 * 7 + 1)                 # ~150 words per minute
    med, best = timed(lambda: model.align(audios[0], text, language="en"), a.runs)
    print(json.dumps({"model": a.model, "route": "align", "files": 1, "audio_s": a.seconds, "s_median": round(med, 4),
                      "s_min": round(best, 4), "audio_s_per_s": round(a.seconds / med, 1)}), flush=True)
    med, best = timed(lambda: whisper_amd.align_batch(model, audios, [text] * a.files, batch_size=a.files, language="en"), a.runs)
    print(json.dumps({"model": a.model, "route": "align_batch", "files": a.files, "audio_s": a.seconds * a.files,
                      "s_median": round(med, 4), "s_min": round(best, 4), "audio_s_per_s": round(a.seconds * a.files / med, 1)}), flush=True)
    if not a.skip_transcribe:
        med, best = timed(lambda: model.transcribe(audios[0], language="en", word_timestamps=True, sample_len=64,
                                                   temperature=0.0, condition_on_previous_text=False), a.runs)
        print(json.dumps({"model": a.model, "route": "transcribe(word_timestamps=True, sample_len=64)", "files": 1,
                          "audio_s": a.seconds, "s_median": round(med, 4), "s_min": round(best, 4),
                          "audio_s_per_s": round(a.seconds / med, 1)}), flush=True)


def part_end_slack(a, dev):
    from oracle import condition
    from whisper_amd.timing import find_alignment_open_batch
    dims = dims_for("tiny")
    sd = synthetic_state_dict(dims, seed=4)
    L = dims.n_text_layer
    heads = sorted([(L - 1, 1), (L - 1, 4), (L - 2, 0), (L - 2, 3)])
    info = condition.condition_alignment(sd, dims, heads, seed=1)
    model = Whisper(ModelDimensions(**dims_dict(dims)), sd, device=dev)
    mask = np.zeros((dims.n_text_layer, dims.n_text_head), dtype=bool)
    for l, h in heads:
        mask[l, h] = True
    model.set_alignment_heads(base64.b85encode(gzip.compress(mask.tobytes())))
    tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    text = tok.encode(SENTENCE * 4)[:60]
    planted = (300 - 1 - 12) // 11 - len(tok.sot_sequence)
    for gain in (1.0, 4.0):
        feats = torch.cat([condition.alignment_features(dims, 1, info["U_a"], seed=s, feat_gain=gain)
                           for s in range(a.seeds)]).to(dev)
        for slack in (0.002, 0.005, 0.01, 0.02, 0.1):
            details = []
            find_alignment_open_batch(model, tok, [text] * a.seeds, None, [600] * a.seeds, [False] * a.seeds,
                                      end_slack=slack, audio_features=feats, details=details)
            err = [d["end"] - planted for d in details]
            hist = {str(e): err.count(e) for e in sorted(set(err))}
            print(json.dumps({"checkpoint": "tiny dims, alignment-conditioned", "feat_gain": gain, "candidates": 60,
                              "frames": 300, "planted_end": planted, "end_slack": slack,
                              "end_minus_planted_histogram": hist, "within_2": sum(abs(e) <= 2 for e in err),
                              "of": len(err)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--files", type=int, default=24)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=12)
    ap.add_argument("--skip-transcribe", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    part_end_slack(a, dev)
    if not a.skip_timing:
        part_timing(a, dev)


if __name__ == "__main__":
    main()
