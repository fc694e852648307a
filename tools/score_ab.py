"""A/B of teacher-forced scoring: the logits route (wh_task_prefill with every scored position selected, then torch
log_softmax + gather — what timing.py's _token_probs does) against wh_task_score (csrc/score.hip), same tensors.

    python tools/score_ab.py [--model large-v3] [--rows 24,8] [--pos 224] [--runs 7] [--routes prefill,score]

Synthetic seeded weights (generated on the device), random encoder-feature stand-ins, fp16 engine.  Per (rows, route):
median / min wall time per call from HIP events around the call (warm-up first, routes interleaved round by round), and
the peak torch.cuda.max_memory_allocated above the level before the call.  WHISPER_AMD_LIB selects the library, so the
prefill route can also be timed on a build that has no wh_task_score (--routes prefill).  One JSON line per result."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from whisper_amd import hip                                                   # noqa: E402
from whisper_amd.synthetic import dims_for, synthetic_state_dict              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--rows", default="24,8")
    ap.add_argument("--pos", type=int, default=224)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", default="prefill,score")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dims = dims_for(a.model)
    routes = a.routes.split(",")
    if "score" not in routes:                   # a library built before wh_task_score existed
        hip.SIGNATURES.pop("wh_task_score", None)
        hip.SIGNATURES.pop("wh_score_scratch_bytes", None)
    sd = synthetic_state_dict(dims, seed=0, device=dev)
    eng = hip.HipModel(dims, hip.WH_F16, hip.pack_weights(sd, dims, hip.WH_F16, dev))
    del sd
    first = 3                                   # sot sequence of 4 tokens: the first scored position
    T0 = first + a.pos + 1
    g = torch.Generator(device=dev).manual_seed(1)
    for R in [int(r) for r in a.rows.split(",")]:
        feats = (torch.randn(R, dims.n_audio_ctx, dims.n_audio_state, generator=g, device=dev) * 0.5).half()
        tokens = torch.randint(300, 40000, (R, T0), generator=g, device=dev)
        n_tok = [T0] * R
        target = tokens[:, first + 1:].contiguous()
        task = hip.HipTask(eng, R, 1, T0)
        task.set_audio(feats.contiguous())

        def run(route):
            task.reset()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if route == "score":
                lp = task.score(tokens, n_tok, first)[0]
            else:
                logits = task.prefill(tokens, sel=list(range(first, T0 - 1)))
                lp = torch.log_softmax(logits, dim=-1).gather(2, target[:, :, None])[:, :, 0]
                del logits
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, lp

        times = {r: [] for r in routes}
        peak, last = {}, {}
        for i in range(a.warmup + a.runs):
            for r in routes:                    # interleaved: both routes see the same clocks and cache state
                ms, pk, lp = run(r)
                if i >= a.warmup:
                    times[r].append(ms)
                    peak[r] = max(peak.get(r, 0), pk)
                last[r] = lp
        for r in routes:
            print(json.dumps({"model": a.model, "rows": R, "positions": a.pos, "route": r, "lib": os.path.basename(hip.lib_path()),
                              "ms_median": round(statistics.median(times[r]), 3), "ms_min": round(min(times[r]), 3),
                              "runs": a.runs, "peak_bytes": int(peak[r]),
                              # the partials the task keeps between calls (held before the call: not part of the peak delta)
                              "held_scratch_bytes": int(task._score_scratch.numel()) if r == "score" else 0}))
        if len(routes) == 2:
            d = (last[routes[0]].double() - last[routes[1]].double()).abs().max().item()
            print(json.dumps({"rows": R, "max_abs_logprob_difference_between_routes": d}))
        task.destroy()
        del task, feats, tokens


if __name__ == "__main__":
    main()
