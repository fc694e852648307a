#!/usr/bin/env python
"""The tie rule of dtw_cpu (whisper/timing.py:82-105) from the LIVE reference (build container only; the reference checkout
is not on the GPU box):

    python tests/golden/make_golden_dtw_ties.py   ->  tests/golden/dtw_ties.npz

Cost matrices whose entries are 0, 1, 2 or 3 (every accumulated cost is a small integer, exact in float32, and most cells
see two or three equal predecessors) and an all-constant matrix.  dtw_cpu returns only the path; its trace matrix is what it
hands to backtrace(), which is wrapped here to keep a copy (after backtrace has forced the borders, timing.py:61-62).
Stored per case: the input (int8), the trace (int8) and the path (int16)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "shims"), "/root/reference"]

import whisper.timing as rt  # noqa: E402  (the reference; tests/shims/numba makes @numba.jit the identity)


def cases():
    rng = np.random.default_rng(5)
    return {
        "q37x64": rng.integers(0, 4, size=(37, 64)).astype(np.float32),
        "q120x200": rng.integers(0, 4, size=(120, 200)).astype(np.float32),
        "const9x14": np.full((9, 14), 2.0, dtype=np.float32),
    }


def main():
    kept = []
    plain = rt.backtrace

    def keeping(trace):
        path = plain(trace)
        kept.append(np.array(trace))
        return path

    rt.backtrace = keeping
    out = {}
    for name, x in cases().items():
        path = rt.dtw_cpu(x.astype(np.float64))                    # as dtw() calls it: x.double().cpu().numpy(), timing.py:151
        trace = kept.pop()
        assert not kept and trace.shape == (x.shape[0] + 1, x.shape[1] + 1)
        assert np.isin(trace, (0, 1, 2)).all()
        out[name + "_x"] = x.astype(np.int8)
        out[name + "_trace"] = trace.astype(np.int8)
        out[name + "_path"] = np.asarray(path).astype(np.int16)
        print(name, x.shape, "path length", path.shape[1], "codes", np.bincount(trace.astype(np.int64).ravel(), minlength=3).tolist())
    path = os.path.join(HERE, "dtw_ties.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
