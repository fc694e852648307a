"""The word-timestamp kernels of timing.hip where the rest of the suite does not look.  Everything here is an exact comparison:
the median is an order statistic and every DTW cell is one float32 add, so the oracle's bits are expected.

  median    every width the launcher instantiates that test_median_filter leaves out (1, 5, 9, 11), and the generic kernel
            (15, 31, 63), on rows with many equal neighbours, signed zeros, and the lengths at which the launcher copies
            (n <= W // 2) or every window index reflects (n = W // 2 + 1).  NaN inputs are out of scope: fminf / fmaxf drop
            a NaN where the reference's sort puts it last.
  dtw ties  the three wavefronts (dtw_kernel, dtw_batch_kernel, dtw_open_batch_kernel) restate dtw_cpu's rule on equal
            predecessors — diagonal only if strictly smallest, then up only if strictly smallest, else left.  Normal floats
            never tie; costs in {0, 1, 2, 3} (sums exact in float32) and a constant matrix tie in most cells.  The oracle's
            own rule on such matrices is pinned to the reference by tests/test_oracle_golden.py::test_dtw_tie_rule.
  rows      more rows than the 1024 threads of the one workgroup cover in a pass, up to DTW_OPEN_MAX_ROWS = 5460."""
import numpy as np
import pytest
import torch

import align_oracle as ao
import oracle
from kernel_lib import hipSuccess, lib
from parity_ref import Buf, _dev, _stream

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------- median
def _median_rows(kind, rows, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.standard_normal((rows, n)).astype(np.float32)
    if kind == "levels":                                           # four values: most windows hold equal neighbours
        return rng.integers(0, 4, size=(rows, n)).astype(np.float32) * 0.5 - 0.75
    x = np.where(rng.random((rows, n)) < 0.5, 0.0, -0.0).astype(np.float32)          # signed zeros among a few +-1
    big = rng.random((rows, n))
    x[big < 0.15] = 1.0
    x[big > 0.85] = -1.0
    x.flat[0], x.flat[-1] = 0.0, -0.0                              # both signs present whatever the size
    return x


@pytest.mark.parametrize("width", [1, 5, 9, 11, 15, 31, 63])
def test_median_widths_and_edges(gpu_device, width):
    """bit-equal to oracle.median_filter (signed zeros: equal by value — which of two equal zeros a sort leaves in the middle
    is not defined).  Shapes: 7 x 301 and 3 x 100 (neither a multiple of the 256-thread block), n = W // 2 (the copy),
    n = W // 2 + 1 (every window index but the centre reflects) and n = 1"""
    from whisper_amd import hip
    pad = width // 2
    shapes = [(7, 301), (3, 100), (5, pad + 1), (5, 1)] + ([(5, pad)] if pad > 0 else [])
    for rows, n in shapes:
        assert (rows * n) % 256 != 0
        for kind in ("random", "levels", "zeros"):
            x = _median_rows(kind, rows, n, seed=width * 100 + n)
            want = np.ascontiguousarray(oracle.median_filter(x, width))
            got = hip.median_filter(torch.from_numpy(x).to(gpu_device), width).cpu().numpy()
            what = f"width={width} rows={rows} n={n} {kind}"
            assert got.shape == want.shape, what
            if kind == "zeros":
                assert np.array_equal(got, want), what
            else:
                assert got.tobytes() == want.tobytes(), what
            if n <= pad:
                assert got.tobytes() == x.tobytes(), what           # timing.py:22-24: returned unchanged


# ----------------------------------------------------------------------------------------------------- dtw ties
TIE_SIZES = [(1, 1), (1, 50), (50, 1), (37, 64), (447, 300)]
ROW_SIZES = [(1025, 8), (2049, 5), (5460, 3)]
_COSTS = {}


def _cost(kind, N, M):
    """(x float32 [N][M], trace int8 [N+1][M+1] of the oracle), made once"""
    key = (kind, N, M)
    if key not in _COSTS:
        rng = np.random.default_rng(N * 1000 + M)
        if kind == "ties":
            x = rng.integers(0, 4, size=(N, M)).astype(np.float32)
        elif kind == "const":
            x = np.full((N, M), 2.0, dtype=np.float32)
        else:
            x = rng.standard_normal((N, M)).astype(np.float32)
        _COSTS[key] = (x, oracle.dtw_trace(x))
    return _COSTS[key]


def _dtw_single(x):
    """wht_dtw on guarded buffers -> int8 trace [N+1][M+1] on the device; x unchanged, all of the trace written, nothing else"""
    N, M = x.shape
    xb, tr = Buf(N * M, torch.float32), Buf((N + 1) * (M + 1), torch.int8)
    xb.t.copy_(torch.from_numpy(x).reshape(-1))
    xb.snapshot(); tr.snapshot()
    assert lib().wht_dtw(xb.ptr(), N, M, tr.ptr(), _stream()) == hipSuccess
    torch.cuda.synchronize()
    assert not xb.changed().any()
    assert tr.changed().all()                                      # the fill is -1, every code is 0, 1 or 2
    return tr.t.view(N + 1, M + 1).clone()


def _dtw_batch(mats):
    """wht_dtw_batch over ragged clips in one slab (row_begin = row_tail = 1: clip b has ntok - 2 rows), NaN around each clip's
    costs -> [int8 trace [N+1][M+1] per clip]; each clip's trace dense at the head of its stride, the rest untouched"""
    clips = len(mats)
    Nmax, Fmax = max(x.shape[0] for x in mats), max(x.shape[1] for x in mats)
    slab = np.full((clips, Nmax, Fmax), np.nan, dtype=np.float32)
    for b, x in enumerate(mats):
        slab[b, :x.shape[0], :x.shape[1]] = x
    stride = (Nmax + 1) * (Fmax + 1)
    xb, tr = Buf(slab.size, torch.float32), Buf(clips * stride, torch.int8)
    xb.t.copy_(torch.from_numpy(slab).reshape(-1))
    ntok = torch.tensor([x.shape[0] + 2 for x in mats], dtype=torch.int32, device=_dev())
    nfr = torch.tensor([x.shape[1] for x in mats], dtype=torch.int32, device=_dev())
    xb.snapshot(); tr.snapshot()
    e = lib().wht_dtw_batch(xb.ptr(), ntok.data_ptr(), nfr.data_ptr(), clips, Nmax + 2, Fmax, 1, 1, Nmax, tr.ptr(), stride, _stream())
    assert e == hipSuccess
    torch.cuda.synchronize()
    assert not xb.changed().any()
    wr = tr.changed().view(clips, stride).cpu()
    out = []
    for b, x in enumerate(mats):
        used = (x.shape[0] + 1) * (x.shape[1] + 1)
        assert wr[b, :used].all() and not wr[b, used:].any(), f"clip {b}: trace written outside its (N + 1) x (M + 1) or not all of it"
        out.append(tr.t.view(clips, stride)[b, :used].view(x.shape[0] + 1, x.shape[1] + 1).clone())
    return out


def _same_trace(got, want, what):
    assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want), f"{what}: trace differs from the oracle's"


def _same_path(trace_dev, x, what):
    from whisper_amd import hip
    _, path = hip.dtw_backtrace(trace_dev.contiguous())
    assert np.array_equal(path.cpu().numpy(), oracle.dtw_path(x)), f"{what}: path differs from the oracle's"


@pytest.mark.parametrize("kind", ["ties", "const"])
def test_dtw_ties_single(gpu_device, kind):
    for N, M in TIE_SIZES:
        x, want = _cost(kind, N, M)
        got = _dtw_single(x)
        _same_trace(got, want, f"dtw {kind} {N}x{M}")
        _same_path(got, x, f"dtw {kind} {N}x{M}")


@pytest.mark.parametrize("kind", ["ties", "const"])
def test_dtw_ties_batch(gpu_device, kind):
    mats = [_cost(kind, N, M)[0] for N, M in TIE_SIZES]
    for (N, M), got in zip(TIE_SIZES, _dtw_batch(mats)):
        _same_trace(got, _cost(kind, N, M)[1], f"dtw_batch {kind} {N}x{M}")
        _same_path(got, _cost(kind, N, M)[0], f"dtw_batch {kind} {N}x{M}")


@pytest.mark.parametrize("kind", ["ties", "const"])
def test_dtw_ties_open(gpu_device, kind):
    """wht_dtw_open: closed clips give the plain trace and path; open clips the float32 numpy oracle's last column (bit for
    bit), end row, trace, jumps and path from there"""
    from whisper_amd import hip
    mats = [_cost(kind, N, M)[0] for N, M in TIE_SIZES]
    Nmax, Fmax = max(n for n, _ in TIE_SIZES), max(m for _, m in TIE_SIZES)
    slab = np.zeros((len(mats), Nmax, Fmax), dtype=np.float32)
    for b, x in enumerate(mats):
        slab[b, :x.shape[0], :x.shape[1]] = x
    rows, cols = [n for n, _ in TIE_SIZES], [m for _, m in TIE_SIZES]
    for closed, slack in ((1, 0.01), (0, 0.0), (0, 0.01)):
        trace, lastcol, end, jumps, path, plen = hip.dtw_open_ktest(torch.from_numpy(slab).to(gpu_device), rows, cols,
                                                                    [closed] * len(mats), slack)
        torch.cuda.synchronize()
        trace, lastcol, end, jumps, path, plen = (t.cpu().numpy() for t in (trace, lastcol, end, jumps, path, plen))
        for b, (N, M) in enumerate(TIE_SIZES):
            what = f"dtw_open {kind} {N}x{M} closed={closed} slack={slack}"
            want = ao.dtw_open(mats[b], bool(closed), slack)
            got_trace = trace[b, : (N + 1) * (M + 1)].reshape(N + 1, M + 1)
            assert np.array_equal(got_trace, want["trace"]), what
            assert lastcol[b, :N].tobytes() == want["lastcol"].tobytes(), what
            assert end[b] == want["end"], what
            n = want["path"].shape[1]
            assert plen[b] == n and np.array_equal(path[b][:, path.shape[2] - n:], want["path"]), what
            assert np.array_equal(jumps[b, :want["end"]], want["jumps"]), what
            if closed:
                assert end[b] == N and np.array_equal(got_trace, _cost(kind, N, M)[1]), what
                assert np.array_equal(want["path"], oracle.dtw_path(mats[b])), what


# ------------------------------------------------------------------------------- rows past one pass of the workgroup
@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("N,M", ROW_SIZES)
def test_dtw_rows_past_one_pass(gpu_device, N, M, kind):
    """the kernels stride rows by the 1024 threads of their one workgroup: one row past a pass, one past two, and the most
    rows the launchers take (three diagonals of N + 1 floats in 64 KB of LDS)"""
    x, want = _cost(kind, N, M)
    _same_trace(_dtw_single(x), want, f"dtw {kind} {N}x{M}")
    _same_trace(_dtw_batch([x])[0], want, f"dtw_batch {kind} {N}x{M}")
