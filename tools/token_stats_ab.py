"""A/B of the per-token statistics in the greedy decode loop at the headline shape: large-v3 dimensions with synthetic
weights (fp16), 24 rows, 224 steps.

  (a) off      the device-side loop without statistics                     DecodingTask(model, options)
  (b) lp       log-probability + entropy per token (csrc/sampling.hip)     DecodingTask(model, options, token_logprobs=True)
  (c) top5     ... and the 5 most probable alternatives                    DecodingTask(model, options, top_logprobs=5)
  (p) parent   route (a) from ANOTHER tree (--parent-tree: a built checkout of the parent commit, its own package and its
               own libwhisper_hip.so, neither of which knows the keywords)

    python tools/token_stats_ab.py [--rows 24] [--sample-len 224] [--passes 5] [--rounds 3] [--parent-tree DIR]
                                   [--out profiles/token_stats_ab.txt]

The method of tools/repetition_ab.py: one package and one library per process, so every leg runs in a child process of its
own (this script with --child and --tree): per round one child on the parent's tree (route off) and one on this tree (the
three routes interleaved pass by pass), the rounds alternating so that both builds see the same clocks.  A child times
DecodingTask.run (encoder output given; HIP events around the call, one warm-up pass) and reports the milliseconds per
decode of every pass and the steps the decode took; ms per step = ms per decode / steps, the prompt pass included.  The
timed call includes what the Python layer does with the statistics (copying the buffers to the host, cutting the lists).
The parent process never opens the GPU.  Per route the median over all passes of all rounds and the spread (max - min);
`off` against `parent`: the difference of the medians beside the larger of the two spreads.  This script writes nothing
it has not measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = {"off": {}, "lp": {"token_logprobs": True}, "top5": {"top_logprobs": 5}}


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree))  # the tree under test: its package loads the library built beside it
    import torch
    import whisper_amd
    routes = a.routes.split(",")
    from whisper_amd.decoding import DecodingTask
    from whisper_amd.model import ModelDimensions, Whisper
    from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict
    dev = torch.device("cuda:0")
    dims = dims_for(a.model)
    model = Whisper(ModelDimensions(**dims_dict(dims)), synthetic_state_dict(dims, seed=0, device=dev), device=dev)
    opts = whisper_amd.DecodingOptions(language="en", fp16=True, sample_len=a.sample_len)
    g = torch.Generator(device=dev).manual_seed(1)
    feats = (torch.randn(a.rows, dims.n_audio_ctx, dims.n_audio_state, generator=g, device=dev) * 0.5).half()

    def run(route):
        task = DecodingTask(model, opts, **KEYWORDS[route])
        assert task._fused_greedy_ok(None)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = task.run(feats)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), res

    times, last = {r: [] for r in routes}, {}
    for i in range(1 + a.passes):
        for r in routes:
            ms, last[r] = run(r)
            if i:
                times[r].append(ms)
    toks = {r: [x.tokens for x in last[r]] for r in routes}
    out = {"package": os.path.dirname(os.path.abspath(whisper_amd.__file__)), "ms": times,
           "steps": {r: min(max(len(t) for t in toks[r]) + 1, a.sample_len) for r in routes},
           "same_tokens_as_off": {r: toks[r] == toks["off"] for r in routes if "off" in toks}}
    if "top5" in last:
        out["entries_per_row"] = [len(x.token_logprobs) for x in last["top5"]][:4]
    print("RESULT " + json.dumps(out), flush=True)


def spawn(a, routes, tree=ROOT):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)                  # nothing but --tree decides which package a child imports
    env.pop("WHISPER_AMD_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--routes", routes, "--model", a.model,
           "--rows", str(a.rows), "--sample-len", str(a.sample_len), "--passes", str(a.passes)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--sample-len", type=int, default=224)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="profiles/token_stats_ab.txt")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--routes", default="off,lp,top5")
    a = ap.parse_args()
    if a.child:
        return child(a)
    ms = {"parent": [], "off": [], "lp": [], "top5": []}
    steps, same, entries = {}, None, None
    for _ in range(a.rounds):
        if a.parent_tree:
            r = spawn(a, "off", a.parent_tree)
            assert os.path.samefile(os.path.dirname(r["package"]), a.parent_tree), r["package"]
            ms["parent"] += r["ms"]["off"]
            steps["parent"] = r["steps"]["off"]
        r = spawn(a, "off,lp,top5")
        for route in ("off", "lp", "top5"):
            ms[route] += r["ms"][route]
            steps[route] = r["steps"][route]
        same, entries = r["same_tokens_as_off"], r.get("entries_per_row")
    lines = [f"{a.model} dims (synthetic weights, fp16), greedy, {a.rows} rows, sample_len {a.sample_len}; lp = token_logprobs "
             f"(log-probability + entropy), top5 = top_logprobs 5; {a.rounds} rounds x {a.passes} passes, a child process per "
             f"build and round, builds alternating; ms per step = ms per decode / steps (prompt pass and the Python layer's "
             f"handling of the lists included)"]
    summary = {}
    for route, t in ms.items():
        if not t:
            continue
        med = statistics.median(t)
        summary[route] = {"ms_per_decode_median": round(med, 2), "spread_ms": round(max(t) - min(t), 2), "steps": steps[route],
                          "ms_per_step_median": round(med / steps[route], 4), "ms_per_decode": [round(x, 2) for x in t]}
        lines.append(json.dumps({route: summary[route]}))
    verdict = {"same_tokens_as_off": same, "entries_per_row_first_rows": entries}
    if "parent" in summary:
        d = summary["off"]["ms_per_decode_median"] - summary["parent"]["ms_per_decode_median"]
        spread = max(summary["off"]["spread_ms"], summary["parent"]["spread_ms"])
        verdict.update(off_minus_parent_ms=round(d, 2), larger_spread_ms=spread, off_equals_parent_within_spread=abs(d) <= spread)
    for route in ("lp", "top5"):
        d = summary[route]["ms_per_decode_median"] - summary["off"]["ms_per_decode_median"]
        verdict[f"{route}_minus_off_ms_per_decode"] = round(d, 2)
        verdict[f"{route}_minus_off_us_per_step"] = round(1000 * (summary[route]["ms_per_step_median"] - summary["off"]["ms_per_step_median"]), 2)
    lines.append(json.dumps(verdict))
    print("\n".join(lines), flush=True)
    if a.out:
        path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
