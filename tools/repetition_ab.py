"""A/B of repetition control in the greedy decode loop at the headline shape: large-v3 dimensions with synthetic weights
(fp16), 24 rows.

  (a) off      the device-side loop without the options            DecodingTask(model, options)
  (b) on       the device-side loop with them (csrc/sampling.hip)  DecodingTask(model, options, no_repeat_ngram_size=,
                                                                                repetition_penalty=)
  (p) parent   route (a) from ANOTHER tree (--parent-tree: a built checkout of the parent commit, its own package and its
               own libwhisper_hip.so, neither of which knows the options)

    python tools/repetition_ab.py [--rows 24] [--sample-len 96] [--ngram 3] [--penalty 1.1] [--passes 5] [--rounds 3]
                                  [--parent-tree DIR] [--out profiles/repetition_ab.txt]

One package and one library per process, so every leg runs in a child process of its own (this script with --child and
--tree): per round one child on the parent's tree (route off) and one on this tree (routes off and on, interleaved pass by pass), the rounds
alternating so that both builds see the same clocks.  A child times DecodingTask.run (encoder output given; HIP events
around the call, one warm-up pass) and reports the milliseconds per decode of every pass and the steps the decode took
(the longest row's sampled tokens + 1); ms per step = ms per decode / steps, the prompt pass included.  The parent process
never opens the GPU.  Per route the median over all passes of all rounds and the spread (max - min); `off` against
`parent`: the difference of the medians beside the larger of the two spreads.  This script writes nothing it has not
measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
        kw = dict(no_repeat_ngram_size=a.ngram, repetition_penalty=a.penalty) if route == "on" else {}
        task = DecodingTask(model, opts, **kw)
        assert task._fused_greedy_ok(None)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = task.run(feats)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), [r.tokens for r in res]

    times, toks = {r: [] for r in routes}, {}
    for i in range(1 + a.passes):
        for r in routes:
            ms, toks[r] = run(r)
            if i:
                times[r].append(ms)
    out = {"package": os.path.dirname(os.path.abspath(whisper_amd.__file__)), "ms": times,
           "steps": {r: min(max(len(t) for t in toks[r]) + 1, a.sample_len) for r in routes}}
    if "off" in toks and "on" in toks:
        n = sum(len(t) for t in toks["off"])
        out["tokens_changed"] = round(sum(x != y for p, d in zip(toks["off"], toks["on"]) for x, y in zip(p, d)) / max(n, 1), 3)
    print("RESULT " + json.dumps(out), flush=True)


def spawn(a, routes, tree=ROOT):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)                  # nothing but --tree decides which package a child imports
    env.pop("WHISPER_AMD_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--routes", routes, "--model", a.model, "--rows", str(a.rows),
           "--sample-len", str(a.sample_len), "--ngram", str(a.ngram), "--penalty", str(a.penalty), "--passes", str(a.passes)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--sample-len", type=int, default=96)
    ap.add_argument("--ngram", type=int, default=3)
    ap.add_argument("--penalty", type=float, default=1.1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="profiles/repetition_ab.txt")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--routes", default="off,on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    ms = {"parent": [], "off": [], "on": []}
    steps, changed = {}, None
    for _ in range(a.rounds):
        if a.parent_tree:
            r = spawn(a, "off", a.parent_tree)
            assert os.path.samefile(os.path.dirname(r["package"]), a.parent_tree), r["package"]
            ms["parent"] += r["ms"]["off"]
            steps["parent"] = r["steps"]["off"]
        r = spawn(a, "off,on")
        ms["off"] += r["ms"]["off"]
        ms["on"] += r["ms"]["on"]
        steps.update(off=r["steps"]["off"], on=r["steps"]["on"])
        changed = r.get("tokens_changed")
    lines = [f"{a.model} dims (synthetic weights, fp16), greedy, {a.rows} rows, sample_len {a.sample_len}, on = "
             f"no_repeat_ngram_size {a.ngram} + repetition_penalty {a.penalty}; {a.rounds} rounds x {a.passes} passes, a child "
             f"process per build and round, builds alternating; ms per step = ms per decode / steps (prompt pass included)"]
    summary = {}
    for route, t in ms.items():
        if not t:
            continue
        med = statistics.median(t)
        summary[route] = {"ms_per_decode_median": round(med, 2), "spread_ms": round(max(t) - min(t), 2), "steps": steps[route],
                          "ms_per_step_median": round(med / steps[route], 4), "ms_per_decode": [round(x, 2) for x in t]}
        lines.append(json.dumps({route: summary[route]}))
    verdict = {"tokens_changed_by_the_options": changed}
    if "parent" in summary:
        d = summary["off"]["ms_per_decode_median"] - summary["parent"]["ms_per_decode_median"]
        spread = max(summary["off"]["spread_ms"], summary["parent"]["spread_ms"])
        verdict.update(off_minus_parent_ms=round(d, 2), larger_spread_ms=spread, off_equals_parent_within_spread=abs(d) <= spread)
    d_on = summary["on"]["ms_per_decode_median"] - summary["off"]["ms_per_decode_median"]
    verdict.update(on_minus_off_ms_per_decode=round(d_on, 2),
                   on_minus_off_us_per_step=round(1000 * (summary["on"]["ms_per_step_median"] - summary["off"]["ms_per_step_median"]), 2))
    lines.append(json.dumps(verdict))
    print("\n".join(lines), flush=True)
    if a.out:
        path = os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
