"""Which kernel family launch_gemv picks (gemv.hip: pick_family), asked through libwhisper_hip_ktest.so without a GPU:
wht_gemv_family launches nothing.

tests/golden/gemv_dispatch_parent.txt is the dispatch as the parent of the pick_family refactor made it: one line per
distinct argument tuple of the gemv cases of test_kernel_parity_gpu.py (the tests that call _gemv_case), recorded on the
GPU with the form tag the parent's library reported.  No test and no tool rewrites that file: a change that retunes a
threshold edits the lines it moves by hand, and the diff shows what moved."""
import os

from kernel_lib import family_of_tag, gemv_family, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "gemv_dispatch_parent.txt")

F16, F32 = 1, 0
PLAIN, LN, COMBINE = 0, 1, 2
STORE, QKV, RESID, GELU, EPI_F32 = 0, 1, 2, 3, 4


def family(dtype=F16, pro=PLAIN, epi=STORE, R=8, N=1280, K=1280, ld=None, ln_folded=1, has_bias=1, splits=1, H=0, x_frag=0,
           y_frag=0) -> str:
    return lib().wht_gemv_family(dtype, pro, epi, R, N, K, ld if ld is not None else K, ln_folded, has_bias, splits, H,
                                 x_frag, y_frag).decode()


def read_table():
    rows = []
    with open(TABLE) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("#") and "parent" in lines[0], "the header line names the parent commit"
    for line in lines[1:]:
        args, tag = line.split(" -> ")
        rows.append((tuple(int(v) for v in args.split()), tag))
    return rows


def test_table_matches_pick_family():
    """every recorded launch goes to the family of the tag the parent reported, and the table reaches every gemv form"""
    from test_kernel_parity_gpu import EXPECTED_FORMS
    rows = read_table()
    assert len(rows) > 1000 and [a for a, _ in rows] == sorted(set(a for a, _ in rows)), "sorted, one line per tuple"
    wrong = []
    for (dtype, R, N, K, pro, epi, ld, ln_folded, has_bias, splits, H, frag), tag in rows:
        got = gemv_family(dtype, pro, epi, R, N, K, ld, ln_folded, has_bias, splits, H, frag)
        if got != family_of_tag(tag):
            wrong.append((dtype, R, N, K, pro, epi, ld, ln_folded, has_bias, splits, H, frag, tag, got))
    assert not wrong, f"{len(wrong)} launches moved, the first: {wrong[:5]}"
    gemv_forms = {t for t in EXPECTED_FORMS if t.startswith(("gemv8/", "rows48", "rows16_mf<", "rt<", "stream<"))}
    assert len(gemv_forms) == 47
    missing = sorted(gemv_forms - {tag for _, tag in rows})
    assert not missing, f"forms of EXPECTED_FORMS the table never reaches: {missing}"


# corners that no test launches: (keyword arguments of family(), the family read from the dispatch before pick_family)
CORNERS = [
    (dict(R=8, ld=1284), "rt8"), (dict(R=16, ld=1284), "rows16_mf"),                    # x_ld % 8 != 0
    (dict(pro=LN, ln_folded=0, R=8), "rt8"), (dict(pro=LN, ln_folded=0, R=3), "rt4"),
    (dict(pro=LN, ln_folded=0, R=40, N=5120), "rows16_mf"),
    (dict(pro=LN, R=40, N=5120), "rows48"), (dict(pro=LN, R=40, N=1280), "rows16_mf"),
    (dict(pro=LN, R=49, N=5120), "rows16_mf"), (dict(pro=LN, R=97, N=5120), "rows16_mf"),
    (dict(pro=LN, ln_folded=0, epi=EPI_F32, has_bias=0, N=51866, R=17), "rows48_stream"),
    (dict(pro=LN, ln_folded=0, epi=EPI_F32, has_bias=0, N=51866, R=16), "rows16_mf"),
    (dict(pro=LN, ln_folded=0, epi=EPI_F32, has_bias=0, N=51866, R=8), "rt8"),
    (dict(pro=LN, ln_folded=0, epi=EPI_F32, has_bias=0, N=51866, R=4), "rt4"),
    (dict(pro=LN, ln_folded=0, epi=EPI_F32, has_bias=1, N=51866, R=17), "rows16_mf"),
    (dict(N=1280, K=5120, R=24), "gemv8"), (dict(N=1280, K=5120, R=40), "rows16_mf"),
    (dict(N=1280, K=5184, R=40), "rt8"),
    (dict(N=1000, K=192, R=48), "gemv8"), (dict(N=1000, K=192, R=97), "rt8"),
    (dict(pro=LN, K=1344, R=8), "rt8"), (dict(pro=LN, K=1344, R=16), "rt8"),
    (dict(pro=COMBINE, H=20, K=1280, splits=1, R=8), "rt8"), (dict(pro=COMBINE, H=20, K=1280, splits=1, R=16), "rows16_mf"),
    (dict(pro=COMBINE, H=20, K=1280, splits=5, R=8), "rt8"),
    (dict(pro=COMBINE, H=24, K=1536, splits=2, R=8), "rt8"), (dict(pro=COMBINE, H=24, K=1536, splits=2, R=16), "rt8"),
    (dict(N=1 << 20, K=2048, R=8), "rt8"),                                              # N * K reaches 2^31
    (dict(x_frag=1, R=30), ""), (dict(x_frag=1, K=5184, R=4), ""), (dict(dtype=F32, x_frag=1, R=4), ""),
    (dict(R=0), ""),
    (dict(dtype=F32, R=4), "rt4"), (dict(dtype=F32, R=8, K=1280), "rt8"), (dict(dtype=F32, R=8, K=3136), "rt4"),
]


def test_corners_nothing_launches():
    wrong = [(kw, want, family(**kw)) for kw, want in CORNERS if family(**kw) != want]
    assert not wrong, wrong


def test_gemv8_will_run_is_the_canonical_launch():
    """gemv8_will_run(R, N, K, pro) is true exactly when the canonical launch of that shape (kernels.h: fp16, packed rows,
    folded LayerNorm, EPI_STORE, PRO_COMBINE as 2 splits of K / 64 heads) goes to gemv8"""
    n_true = 0
    for R in range(0, 31):
        for D in (384, 512, 768, 1024, 1280):
            for (N, K) in ((D, D), (3 * D, D), (4 * D, D), (D, 4 * D)):
                for pro in (PLAIN, LN, COMBINE):
                    will = bool(lib().wht_gemv8_will_run(R, N, K, pro))
                    fam = family(F16, pro, STORE, R, N, K, K, 1, 1, 2, K // 64)
                    assert will == (fam == "gemv8"), (R, N, K, pro, will, fam)
                    n_true += will
    assert n_true > 0
    assert not lib().wht_gemv8_will_run(8, 1536, 1536, COMBINE)          # H = 24 > 20: the launcher always refused it
