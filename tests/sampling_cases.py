"""The inputs of every kernel case of tests/test_sampling_gpu.py, generated on the host alone, and what the restatement
(tests/sampling_oracle.py) expects of them.  tests/test_sampling_cpu.py replays the same families without a GPU to bound the
share of rows whose draw fp32 cannot decide.

A FAMILY is one set of buffers — logits, rules, per-row sampled histories, trie / repetition settings — with a list of
launches over it that vary what the noise is keyed by: the seed (both words set, the high word zero, the low word zero), the
step (through the prompt length T0; the filtered row does not depend on it) and the temperature.  All logits lie on the
dyadic grid of tests/test_phrases_gpu.py (multiples of 2^-6, |x| < 64; boost 4 and penalty 2 keep them there), so x - max
is exact in fp32 and every error of a key is in EPS_KEY (sampling_oracle's docstring).
"""
import numpy as np

import phrase_oracle
import sampling_oracle as so
import test_phrases_gpu as tp
import test_repetition_gpu as trep

TEMPERATURES = (0.5, 1.0, 2.0, 0.7)     # three exact reciprocals and one that is not
MAX_UNDECIDABLE = 0.005                 # the cap on the share of a parametrisation's rows whose token is not compared
BOOST = 4.0                             # moderate: the noise decides among boosted and unboosted entries

PLAIN_PARAMS = [(V, R, mode) for V in (1000, 1025, 51866) for R in (1, 3, 24) for mode in ("mid", "first", "nots", "lag")]
PHRASE_PARAMS = [(V, R, mode) for V in (1025, 51866) for R in (3, 24) for mode in ("mid", "first", "nots", "lag")]
REP_PARAMS = [(V, R, mode) for (V, R) in ((1025, 3), (1025, 24), (51866, 3)) for mode in ("mid", "first", "nots", "lag")]

# (seed, step, row, token) whose hash has its top 24 bits set / clear: the largest and the smallest uniform.  Found by
# `find_edge` below over seeds 1, 2, ... at V = 51866, R = 24, step 9; tests/test_sampling_cpu.py confirms them.
EDGE_STEP, EDGE_V, EDGE_R = 9, 51866, 24
EDGE_TOP = (15, 9, 7, 12738)
EDGE_BOTTOM = (5, 9, 0, 47439)


def find_edge(top: bool, first_seed: int = 1, max_seeds: int = 400):
    want = 0xFFFFFF if top else 0
    tok = np.arange(EDGE_V)
    for seed in range(first_seed, first_seed + max_seeds):
        for row in range(EDGE_R):
            hit = np.flatnonzero((so.sample_hash(seed, EDGE_STEP, row, tok) >> np.uint32(8)) == want)
            if hit.size:
                t = int(hit[0])
                if t not in (5, 7, 41, 220) and t < 50257:
                    return seed, EDGE_STEP, row, t
    raise AssertionError("no edge tuple found")


def seeds_for(rng, n):
    """n noise keys, in turn with both words set, the high word zero, the low word zero"""
    out = []
    for i in range(n):
        lo, hi = int(rng.integers(1, 2 ** 32)), int(rng.integers(1, 2 ** 30))     # (the loop draws keys below 2^62)
        out.append([(hi << 32) | lo, lo, hi << 32][i % 3])
    return out


def _histories(r, R, mode):
    TB = r.timestamp_begin
    hist, ended = [], []
    for i in range(R):
        at_eot = mode == "mid" and i % 7 == 6
        if mode == "first":
            H = []
        elif mode == "nots":
            H = [100, 101, 102]
        elif at_eot:
            H = [TB + 3, 100, r.eot]
        else:
            H = [[TB + 3, 100, 101], [TB + 3, 100, TB + 9], [TB + 3, TB + 3, 100], [100, TB + 1, TB + 1]][i % 4]
        hist.append(H)
        ended.append(at_eot)
    return hist, ended


def plain_family(V, R, mode, n_launches=None, unique=False, salt=0):
    """<true, false, false>: no list, no repetition control.  Logits in [-4, 4]; in every second row five text entries are
    raised by 6.5 so that the timestamp-mass rule goes both ways (the timestamps' joint mass is about max + 3 in the small
    vocabularies, max + 5 in the large one).  unique: every entry of a row has a value of its own (a permutation of the grid;
    V <= 8192), for the cold limit, where equal maxima would be told apart by the noise."""
    rng = np.random.default_rng(7000 + 13 * V + 101 * R + {"mid": 0, "first": 1, "nots": 2, "lag": 3}[mode] + 1000003 * salt)
    with_ts = mode != "nots"
    r = tp._rules(V, with_ts, suppress=(41, 5, 7))
    if unique:
        assert V <= 8192
        x = np.stack([(rng.permutation(V) - V // 2) / 64.0 for _ in range(R)]).astype(np.float32)
    else:
        x = (rng.integers(-256, 257, (R, V)) / 64.0).astype(np.float32)
        for i in range(1, R, 2):
            x[i, rng.integers(300, r.eot - 1, 5)] += np.float32(6.5)
    hist, ended = _histories(r, R, mode)
    lag = [(3 * i) % 4 for i in range(R)] if mode == "lag" else [0] * R
    sums = [float(rng.integers(-64, 1)) / 4 for _ in range(R)]
    if n_launches is None:
        n_launches = 16 if V > 51000 else 256
    seeds = seeds_for(rng, n_launches)
    launches = [dict(T0=4 + j % 7, temperature=TEMPERATURES[j % 4], seed=seeds[j]) for j in range(n_launches)]
    return dict(V=V, R=R, x=x, r=r, with_ts=with_ts, hist=hist, ended=ended, lag=lag, sums=sums, trie=None, states=[0] * R,
                boost=0.0, rep=False, n=0, penalty=1.0, launches=launches)


def phrase_families(V, R, mode):
    """the scenario table of tests/test_phrases_gpu.py (rows put into chosen trie nodes) at boost 4: one family per scenario
    offset, four launches each"""
    out = []
    for k in range((10 + R - 1) // R):
        c = tp._case(V, R, mode, k)
        rng = np.random.default_rng(81000 + V + 7 * R + k)
        hist = [row[c["T0"] - c["lag"][i]:] for i, row in enumerate(c["rows"])]
        ended = [len(H) > 0 and H[-1] == c["r"].eot for H in hist]
        launches = [dict(T0=c["T0"], temperature=TEMPERATURES[(j + k) % 4], seed=s) for j, s in enumerate(seeds_for(rng, 4))]
        out.append(dict(V=V, R=R, x=c["x"], r=c["r"], with_ts=c["with_ts"], hist=hist, ended=ended, lag=c["lag"], sums=c["sums"],
                        trie=c["trie"], states=c["states"], boost=BOOST, rep=False, n=0, penalty=1.0, launches=launches))
    return out


def rep_families(V, R, mode):
    """the plan and the scenario table of tests/test_repetition_gpu.py (histories around the tile boundary, every n, the
    penalty), every second one with the one-phrase list at boost 4 as well: one family per plan entry, two launches each"""
    out = []
    for idx, (L, n, penalty) in enumerate(trep._plan(mode)):
        c = trep._case(V, R, mode, L, n, penalty, with_trie=idx % 2 == 0, idx=idx)
        rng = np.random.default_rng(91000 + V + 7 * R + idx)
        ended = [len(H) > 0 and H[-1] == c["r"].eot for H in c["hist"]]
        launches = [dict(T0=c["T0"], temperature=TEMPERATURES[(j + idx) % 4], seed=s) for j, s in enumerate(seeds_for(rng, 2))]
        out.append(dict(V=V, R=R, x=c["x"], r=c["r"], with_ts=c["with_ts"], hist=c["hist"], ended=ended, lag=c["lag"],
                        sums=c["sums"], trie=c["trie"] if c["with_trie"] else None, states=[0] * R, boost=BOOST, rep=True, n=n,
                        penalty=penalty, launches=launches))
    return out


def edge_family(top: bool):
    """the planted row of the edge case: the token whose uniform is the largest (smallest) the map gives has the lowest logit of
    its row, far below the others, and is not masked"""
    seed, step, row, token = EDGE_TOP if top else EDGE_BOTTOM
    fam = plain_family(EDGE_V, EDGE_R, "nots", n_launches=1, salt=5 + int(top))
    fam["x"][row, token] = np.float32(-63.0)
    L = len(fam["hist"][0])
    fam["launches"] = [dict(T0=step - L, temperature=1.0, seed=seed)]
    return fam, row, token


def filtered_rows(fam):
    with np.errstate(invalid="ignore", divide="ignore"):
        return [so.filtered_row(fam["x"][i], fam["hist"][i], fam["r"], fam["trie"], fam["states"][i], fam["boost"], fam["n"],
                                fam["penalty"], fam["rep"]) for i in range(fam["R"])]


def expected(fam, rows=None):
    """per launch, per row: what the restatement draws (sampling_oracle.sample_from)"""
    rows = rows if rows is not None else filtered_rows(fam)
    L = len(fam["hist"][0])
    out = []
    for la in fam["launches"]:
        step = la["T0"] + L                       # the common position counter: prompt plus sampled tokens of the longest row
        out.append([so.sample_from(rows[i], la["temperature"], la["seed"], step, i, fam["r"], fam["trie"], fam["ended"][i])
                    for i in range(fam["R"])])
    return out


def undecidable_share(families):
    """(rows whose token fp32 cannot decide, rows that draw) over the launches of some families"""
    bad = total = 0
    for fam in families:
        for launch in expected(fam):
            for w in launch:
                if w["lp"] is not None:
                    total += 1
                    bad += not w["decidable"]
    return bad, total


def families_of(kind, V, R, mode):
    if kind == "plain":
        return [plain_family(V, R, mode)]
    return phrase_families(V, R, mode) if kind == "phrase" else rep_families(V, R, mode)
