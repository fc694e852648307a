"""Temperature sampling without a GPU: the noise of whisper_amd/csrc/sample_noise.h through the host entries of
libwhisper_hip_ktest.so (nothing is launched), the restatement of tests/sampling_oracle.py against it bit for bit, and the
statistics of the restatement's own draws — this is where the hash's quality is judged, because it is cheap here.

The chi-square tests reduce every table to z = (chi^2 - dof) / sqrt(2 dof), which is close to standard normal for the
degrees of freedom used here (>= 56), and assert |z| < 5: a correct sampler fails one such assertion about once in 10^6.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_lib  # noqa: E402
import phrase_oracle  # noqa: E402
import sampling_cases as sc  # noqa: E402
import sampling_oracle as so  # noqa: E402


def lib_hashes(seed, step, row, token):
    n = len(seed)
    arrs = [np.ascontiguousarray(seed, np.uint64), np.ascontiguousarray(step, np.int32), np.ascontiguousarray(row, np.int32),
            np.ascontiguousarray(token, np.int32)]
    out = np.empty(n, np.uint32)
    kernel_lib.lib().wht_sample_hash_many(*[a.ctypes.data for a in arrs], n, out.ctypes.data)
    return out


def lib_uniform_sweep():
    """the library's uniform for every value of the bits of a hash that it uses"""
    h = kernel_lib.lib()
    bits = h.wht_sample_uniform_bits()
    out = np.empty(1 << bits, np.float32)
    h.wht_sample_uniform_range(0, 1 << bits, out.ctypes.data)
    return bits, out


def test_uniform_range():
    """Every hash gives 0 < u < 1 strictly in fp32, u non-decreasing in the bits the map uses, and a finite float32 Gumbel
    value.  All values of those bits are swept through the library's host entry, and the remaining low bits are shown not to
    matter, so this covers all 2^32 hashes.
    Against the 24-bit map this pull request replaces, ((h >> 8) + 0.5) * 2^-24, the test fails at the top value alone:
    n + 0.5 rounds to 2^24 at n = 2^24 - 1, u == 1.0f and -log(-log u) = +inf."""
    h = kernel_lib.lib()
    bits, u = lib_uniform_sweep()
    low = (1 << (32 - bits)) - 1
    rng = np.random.default_rng(0)
    for v in rng.integers(0, 2 ** 32, 2000).tolist() + [0, 2 ** 32 - 1]:
        assert h.wht_sample_uniform_of_hash(v) == h.wht_sample_uniform_of_hash(v | low) == u[v >> (32 - bits)]
    assert u.min() > 0.0 and u.max() < 1.0, (float(u.min()), float(u.max()), int(np.argmax(u)))
    assert (np.diff(u) >= 0).all()
    with np.errstate(divide="ignore"):
        g = -np.log(-np.log(u))
    assert g.dtype == np.float32 and np.isfinite(g).all(), int(np.flatnonzero(~np.isfinite(g))[0])
    # the range the comments and documents state
    assert u[0] == np.float32(2.0 ** -24) and u[-1] == np.float32(1 - 2.0 ** -24)
    assert -2.82 < g.min() < -2.81 and 16.63 < g.max() < 16.65


def test_restatement_equals_library():
    """the restated hash and uniform equal the library's bit for bit: 10^5 random tuples, the edges of every argument, and the
    uniform over all the values of the bits it uses"""
    V = 51866
    rng = np.random.default_rng(1)
    n = 100000
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    step = rng.integers(0, 448, n)
    row = rng.integers(0, 48, n)
    token = rng.integers(0, V, n)
    edges = [(s, st, r, t) for s in (0, 0xDEADBEEF << 32, 0xDEADBEEF, 2 ** 64 - 1, 0x123456789ABCDEF)
             for st in (0, 447) for r in (0, 47) for t in (0, V - 1)]
    seed = np.concatenate([seed, np.array([e[0] for e in edges], np.uint64)])
    step = np.concatenate([step, [e[1] for e in edges]])
    row = np.concatenate([row, [e[2] for e in edges]])
    token = np.concatenate([token, [e[3] for e in edges]])
    want = lib_hashes(seed, step, row, token)
    got = so.sample_hash(seed, step, row, token)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    h = kernel_lib.lib()
    assert h.wht_sample_hash(int(seed[5]), int(step[5]), int(row[5]), int(token[5])) == int(want[5])
    assert len(set(want.tolist())) > 0.999 * len(want)                       # (not a constant)
    bits, u = lib_uniform_sweep()
    assert bits == so.UNIFORM_BITS
    mine = so.uniform_of_hash((np.arange(1 << bits, dtype=np.uint64) << np.uint64(32 - bits)).astype(np.uint32))
    assert mine.dtype == np.float32 and np.array_equal(mine.view(np.uint32), u.view(np.uint32))
    lu = np.array([h.wht_sample_uniform_of_hash(int(v)) for v in want[:2000]], np.float32)
    assert np.array_equal(lu.view(np.uint32), so.uniform_of_hash(want[:2000]).view(np.uint32))


def test_edge_tuples():
    """the tuples the GPU edge case plants: the hash of the first has its top 24 bits set (the largest uniform; 1.0f under the
    24-bit map), the hash of the second has them clear (the smallest)"""
    for tup, top in ((sc.EDGE_TOP, True), (sc.EDGE_BOTTOM, False)):
        seed, step, row, token = tup
        assert tup == sc.find_edge(top, first_seed=seed, max_seeds=1)          # the search is deterministic
        h = int(lib_hashes([seed], [step], [row], [token])[0])
        assert h >> 8 == (0xFFFFFF if top else 0)
        u = kernel_lib.lib().wht_sample_uniform_of_hash(h)
        assert u == (float(np.float32(1 - 2.0 ** -24)) if top else 2.0 ** -24)
        assert row < sc.EDGE_R and token < sc.EDGE_V and step == sc.EDGE_STEP
        fam, prow, ptok = sc.edge_family(top)
        want = sc.expected(fam)[0]
        assert want[prow]["tok"] != ptok and math.isfinite(want[prow]["lp"])
        assert fam["x"][prow].min() == fam["x"][prow, ptok] == -63.0


# --------------------------------------------------------------------------------------------------------- distribution
DIST_V, DIST_ROWS, DIST_DRAWS = 1025, 8, 2000
DIST_T = (0.5, 1.0, 2.0)


def dist_rows():
    """8 filtered rows of 1025 entries: normal logits of spread 1 .. 3, a tenth of the entries filtered"""
    rng = np.random.default_rng(2)
    rows = []
    for i in range(DIST_ROWS):
        x = rng.standard_normal(DIST_V) * (1.0 + 2.0 * i / (DIST_ROWS - 1))
        x[rng.random(DIST_V) < 0.1] = -np.inf
        rows.append(x)
    return rows


def vary(way, n, row):
    """(seed, step) of n draws: over seeds; over steps at one seed; over the high seed word alone"""
    rng = np.random.default_rng(100 + row)
    if way == "seeds":
        return rng.integers(0, 2 ** 62, n).astype(np.uint64), np.full(n, 5)
    if way == "steps":
        return np.full(n, 0x0123456789ABCDEF, np.uint64), np.arange(n)
    return (np.arange(1, n + 1).astype(np.uint64) << np.uint64(32)) | np.uint64(0x9ABCDEF0), np.full(n, 5)


def draw_many(xf, temperatures, seed, step, row):
    """the restatement's draws for arrays of (seed, step): {T: tokens}.  The noise does not depend on T and is formed once."""
    ok = np.flatnonzero(xf != -np.inf)
    g = so.gumbel(np.asarray(seed)[:, None], np.asarray(step)[:, None], row, ok[None, :])
    return {T: ok[np.argmax(xf[ok][None, :] / float(np.float32(T)) + g, axis=1)] for T in temperatures}


def distribution_z(way):
    """{T: z} of the restatement's draws against softmax(x / T), 8 equal-mass bins per row, pooled over the 8 rows"""
    chi = {T: [0.0, 0] for T in DIST_T}
    for i, xf in enumerate(dist_rows()):
        seed, step = vary(way, DIST_DRAWS, i)
        for T, toks in draw_many(xf, DIST_T, seed, step, i).items():
            c, d = so.goodness_of_fit(toks, so.softmax_t(xf, T), 8)
            chi[T][0] += c
            chi[T][1] += d
    return {T: so.z_of(c, d) for T, (c, d) in chi.items()}


@pytest.mark.parametrize("way", ["seeds", "steps", "seed_hi"])
def test_distribution(way):
    """the restatement's draws follow softmax(x / T): V = 1025, 8 rows, 2000 draws per row, T in {0.5, 1, 2}, the draw varied
    over seeds, over steps at one seed, and over the high seed word alone.  Measured with the 23-bit map, pooled over the rows (56 degrees of freedom): z between -1.8 and -0.05."""
    z = distribution_z(way)
    print("z", way, z)                 # (tests/test_sampling_gpu.py::test_report writes them to sampling_parity.json)
    for T, v in z.items():
        assert abs(v) < 5, (way, T, v)


def joint_z(tok_a, tok_b, p):
    """z of the 8 x 8 table of the bin indices of paired draws against the product of the bins' masses"""
    which, mass = so.mass_bins(p, 8, len(tok_a))
    k = mass.size
    table = np.bincount(which[tok_a] * k + which[tok_b], minlength=k * k)
    c, d = so.chi_square(table, np.outer(mass, mass).reshape(-1) * len(tok_a))
    return so.z_of(c, d)


@pytest.mark.parametrize("T", DIST_T)
def test_independence(T):
    """from identical logits, the draws of rows i and i + 1 at one seed and step are independent, and so are those of steps s
    and s + 1 of one row: chi-square of the joint table of bin indices, 2000 pairs each, over seeds"""
    xf = dist_rows()[3]
    p = so.softmax_t(xf, T)
    seed, _ = vary("seeds", DIST_DRAWS, 0)
    zs = {}
    for i in (0, 23, 46):
        a = draw_many(xf, [T], seed, np.full(DIST_DRAWS, 7), i)[T]
        b = draw_many(xf, [T], seed, np.full(DIST_DRAWS, 7), i + 1)[T]
        zs[f"rows {i},{i + 1}"] = joint_z(a, b, p)
    for s in (0, 100, 446):
        a = draw_many(xf, [T], seed, np.full(DIST_DRAWS, s), 2)[T]
        b = draw_many(xf, [T], seed, np.full(DIST_DRAWS, s + 1), 2)[T]
        zs[f"steps {s},{s + 1}"] = joint_z(a, b, p)
    print("z", T, zs)
    for k, v in zs.items():
        assert abs(v) < 5, (T, k, v)


# ----------------------------------------------------------------------------------------------------------- cold limit
@pytest.mark.parametrize("mode", ["mid", "first", "nots", "lag"])
def test_cold_limit(mode):
    """T = 2^-20 on the 2^-6 grid: neighbouring logits are 2^14 apart after the scaling, the noise spans less than 20, so the draw
    is the arg-max token of the T = 0 oracle, for every row"""
    fam = sc.plain_family(1025, 24, mode, n_launches=6, unique=True)
    for la in fam["launches"]:
        la["temperature"] = 2.0 ** -20
    for launch in sc.expected(fam):
        for i, w in enumerate(launch):
            tok, lp, _, _ = phrase_oracle.sampler_step(fam["x"][i], fam["hist"][i], 0, phrase_oracle.Trie([]), 0.0, fam["r"],
                                                       ended=fam["ended"][i])
            assert w["tok"] == tok and w["decidable"]
            assert (w["lp"] is None and lp is None) or abs(w["lp"] - lp) < 1e-12


# --------------------------------------------------------------------------------------------------------- decidability
def _ids(params):
    return [f"{V}-{R}-{mode}" for V, R, mode in params]


@pytest.mark.parametrize("V,R,mode", sc.PLAIN_PARAMS, ids=_ids(sc.PLAIN_PARAMS))
def test_decidability_plain(V, R, mode):
    """for the exact inputs of the GPU module's plain cases, the share of rows whose token fp32 cannot decide is within the cap"""
    bad, total = sc.undecidable_share(sc.families_of("plain", V, R, mode))
    print("undecidable", bad, "of", total)
    assert total > 0 and bad <= sc.MAX_UNDECIDABLE * total


@pytest.mark.parametrize("V,R,mode", sc.PHRASE_PARAMS, ids=_ids(sc.PHRASE_PARAMS))
def test_decidability_phrases(V, R, mode):
    bad, total = sc.undecidable_share(sc.families_of("phrase", V, R, mode))
    print("undecidable", bad, "of", total)
    assert total > 0 and bad <= sc.MAX_UNDECIDABLE * total


@pytest.mark.parametrize("V,R,mode", sc.REP_PARAMS, ids=_ids(sc.REP_PARAMS))
def test_decidability_repetition(V, R, mode):
    bad, total = sc.undecidable_share(sc.families_of("rep", V, R, mode))
    print("undecidable", bad, "of", total)
    assert total > 0 and bad <= sc.MAX_UNDECIDABLE * total
