"""A/B of phrase-list biasing in the greedy decode loop, one process, large-v3 dimensions with synthetic weights (fp16):

  (a) plain    the unbiased device-side loop                      DecodingTask(model, options)
  (b) device   the biased device-side loop (csrc/sampling.hip)    DecodingTask(model, options, phrases=list)
  (c) host     the same result through the host loop: the PhraseBias filter, one wh_task_step and a full logits
               read-back per token — the only route there was before the sampler took the list (forced here by a no-op
               filter behind the stock ones)

    python tools/phrases_ab.py [--model large-v3] [--rows 8,24] [--sample-len 64] [--phrases 1000] [--boost 1.0]
                               [--passes 5] [--out profiles/phrases_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/phrases_ab.py --passes 2 --routes plain,device --out ''

The list: `--phrases` random phrases of 1-6 unsuppressed text tokens, at a boost small enough that the path mostly stays
the model's own (reported: the share of sampled tokens that differ from the unbiased decode).  Wall time per decode of
`rows` clips (HIP events around DecodingTask.run, encoder output given, one warm-up pass, routes interleaved pass by
pass so that all see the same clocks); per route the median and the spread (max - min) over the passes.  The two sampler
kernels' own times with and without the list come from the rocprofv3 run above (tools/prof_summary.py reads its stats);
this script appends nothing it has not measured."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import whisper_amd                                                             # noqa: E402
from whisper_amd.decoding import DecodingTask, LogitFilter                     # noqa: E402
from whisper_amd.model import ModelDimensions, Whisper                         # noqa: E402
from whisper_amd.phrases import PhraseList                                     # noqa: E402
from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict    # noqa: E402


class _Noop(LogitFilter):
    def apply(self, logits, tokens):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--rows", default="8,24")
    ap.add_argument("--sample-len", type=int, default=64)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--boost", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--routes", default="plain,device,host")
    ap.add_argument("--out", default="profiles/phrases_ab.txt")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dims = dims_for(a.model)
    model = Whisper(ModelDimensions(**dims_dict(dims)), synthetic_state_dict(dims, seed=0, device=dev), device=dev)
    opts = whisper_amd.DecodingOptions(language="en", fp16=True, sample_len=a.sample_len)
    probe = DecodingTask(model, opts)
    banned = set(probe._suppress) | {probe.tokenizer.encode(" ")[0]}
    rng = np.random.default_rng(0)
    ok = np.array([t for t in range(300, probe.tokenizer.eot) if t not in banned])
    phrases = [rng.choice(ok, int(rng.integers(1, 7))).tolist() for _ in range(a.phrases)]
    plist = PhraseList(phrases, boost=a.boost, tokenizer=probe.tokenizer)
    routes = a.routes.split(",")
    lines = [f"{a.model} dims (synthetic weights, fp16), greedy, sample_len {a.sample_len}, {len(plist)} phrases / "
             f"{plist.n_nodes} trie nodes, boost {a.boost}, {a.passes} passes, routes interleaved"]
    g = torch.Generator(device=dev).manual_seed(1)
    for R in [int(r) for r in a.rows.split(",")]:
        feats = (torch.randn(R, dims.n_audio_ctx, dims.n_audio_state, generator=g, device=dev) * 0.5).half()

        def run(route):
            task = DecodingTask(model, opts, phrases=None if route == "plain" else plist)
            if route == "host":
                task.logit_filters.append(_Noop())
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = task.run(feats)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), [r.tokens for r in res]

        times = {r: [] for r in routes}
        toks = {}
        for i in range(1 + a.passes):
            for r in routes:
                ms, toks[r] = run(r)
                if i:
                    times[r].append(ms)
        out = {"rows": R}
        for r in routes:
            out[r] = {"ms_per_pass": [round(t, 2) for t in times[r]], "ms_median": round(statistics.median(times[r]), 2),
                      "spread_ms": round(max(times[r]) - min(times[r]), 2)}
        if "plain" in toks and "device" in toks:
            n = sum(len(t) for t in toks["plain"])
            out["tokens_changed_by_the_list"] = round(
                sum(x != y for p, d in zip(toks["plain"], toks["device"]) for x, y in zip(p, d)) / max(n, 1), 3)
        if "host" in toks and "device" in toks:
            out["device_equals_host_tokens"] = toks["host"] == toks["device"]
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
    if a.out:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), a.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
