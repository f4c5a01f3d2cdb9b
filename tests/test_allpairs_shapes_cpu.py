"""The premises of tests/test_gpu_allpairs_wide.py, checked without a GPU: the restated plan of the wide all-pairs consumer
(tests/support/allpairs_shapes.py) gives the long splits the cases are named for, the case lists reach every default instance,
every planted maximum and every tie group sits in the tile, ring position, split and half-wave group it is meant for and IS the
float64 reference's answer, and every case keeps the wide kernel's reference-free sum in range (so that no call can silently be
repeated with the narrow kernel)."""
import os

import numpy as np
import pytest

from tests.support import allpairs_shapes as ap


def test_restated_plan_gives_the_long_splits():
    for d in ap.D_INSTANCES + ap.D_EDGES:
        p = ap.plan_of("LONG4", d)
        assert (p["row_tiles"], p["splits"], p["cols_per_split"], p["tiles"], p["last_cols"]) == (64, 4, 1024, [32, 32, 32, 29], 5)
        assert ap.n_rows_of("LONG4", d) == (32768 if d <= 256 else 16384)
    for d in ap.D_INSTANCES:
        p = ap.plan_of("LONG1", d)
        assert (p["row_tiles"], p["splits"], p["cols_per_split"], p["tiles"], p["last_cols"]) == (256, 1, 2048, [63], 15)
        assert ap.n_rows_of("LONG1", d) == (131072 if d <= 256 else 65536)
        p = ap.plan_of("TINY33", d)
        assert (p["splits"], p["tiles"], p["last_cols"]) == (1, [2], 1) and p["row_tiles"] == (1 if d <= 256 else 2)
        p = ap.plan_of("TINY5", d)
        assert (p["splits"], p["tiles"], p["last_cols"]) == (1, [1], 5)
        assert p["row_tiles"] == (2 if d <= 256 else 3) and 513 - (p["row_tiles"] - 1) * p["tile_rows"] == 1
    p = ap.plan_of("LONG1_ODD", 256)
    assert (p["row_tiles"], p["tiles"], p["last_cols"]) == (256, [63], 15) and ap.n_rows_of("LONG1_ODD", 256) - 255 * p["tile_rows"] == 1
    # rows = None at the two long tables is an ordinary call: few row tiles, 128-column splits of four tiles
    assert ap.wide_plan(ap.N_LONG4, ap.N_LONG4, 256)["tiles"] == [4] * 31 + [1] and ap.wide_plan(ap.N_LONG1, ap.N_LONG1, 300)["tiles"] == [4] * 15 + [3]
    # ... which is all the shapes of test_all_score_streamed_consumer get
    assert ap.wide_plan(700, 700, 50)["tiles"] == [4, 4, 4, 4, 4, 2] and ap.wide_plan(3000, 3000, 128)["tiles"] == [4] * 23 + [2]
    assert max(max(ap.wide_plan(n, r, d)["tiles"]) for n, d in ((700, 50), (3000, 128), (1029, 256), (600, 300)) for r in (n, 523)) == 4


def test_plan_restatement_still_stands_in_the_source():
    # drift guard: the restatement copies these lines of bf16_shape, column_split and reduce_once.  If this fails after an edit
    # of all_score.hip, the plan may have changed: update tests/support/allpairs_shapes.py (or, after a mere reformat, the
    # texts below)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc", "all_score.hip")).read()
    for text in ("const int ks_need = (n_emb + 15) / 16;",
                 "const int KS = ks_need <= 4 ? 4 : ks_need <= 8 ? 8 : ks_need <= 16 ? 16 : 32;",
                 "const int want = std::max(1, std::min({cdiv(n_node, 128), cdiv(target_workgroups, row_tiles), max_splits}));",
                 "const int cps = cdiv(cdiv(n_node, want), 128) * 128;",
                 "return {cdiv(n_node, cps), cps};",
                 "const bool wide = allow_wide && precision == 1 && n_rows >= 512 && !getenv(\"GG_ALLPAIRS_NARROW\");",
                 "const int tile_rows = wide ? (KS <= 16 ? 512 : 256) : 32 * RB;",
                 "const ColumnSplit cs = column_split(n, row_tiles, wide ? 256 : 2048);",
                 "if (KS <= 4) { GG_BF16_X32(4, 2, 8); }",
                 "else if (KS <= 8) { GG_BF16_X32(8, 2, 8); }",
                 "else if (KS <= 16) { if (one_wave) { GG_BF16_X32(16, 4, 4); } else { GG_BF16_X32(16, 2, 8); } }",
                 "else { GG_BF16_X32(32, 1, 8); }",
                 "static const bool one_wave = getenv(\"GG_K7_NW4\") != nullptr;",
                 "const int n_tiles = (cend - cbeg + 31) >> 5;"):
        assert text in src, "all_score.hip no longer contains %r: restate the plan in tests/support/allpairs_shapes.py" % text


def test_cases_reach_every_default_instance_and_the_one_wave_instance():
    want = {(4, 2, 8), (8, 2, 8), (16, 2, 8), (32, 1, 8)}
    for name in ("LONG4", "LONG1", "TINY33", "TINY5"):
        got = {(p["KS"], p["RB"], p["NW"]) for p in (ap.plan_of(n, d) for n, d in ap.EXACT_CASES if n == name)}
        assert got == want, name  # (each with the log-sum-exp and without: the GPU test calls both)
    assert {(p["KS"], p["RB"], p["NW"]) for p in (ap.plan_of(n, d) for n, d in ap.DENSE_CASES)} == want
    p = ap.plan_of(*ap.NW4_CASE, nw4=True)
    assert (p["KS"], p["RB"], p["NW"], p["tile_rows"], p["tiles"]) == (16, 4, 4, 512, [32, 32, 32, 29])
    # the k edges: d = 8 one k-step of eight values, d = 64 and d = 512 a full KS, d = 65 and d = 257 one value in the next k-step
    assert [ap.bf16_shape(d) for d in ap.D_EDGES] == [4, 4, 8, 32, 32]
    assert len(ap.EXACT_CASES) == len(set(ap.EXACT_CASES)) == 22


def test_planted_columns_sit_where_the_sweep_has_not_been():
    """geometry alone (d does not move a column)"""
    for name, odd in (("LONG4", True), ("LONG1", True)):
        p, g = ap.plan_of(name, 256), ap.GEOMETRY[name]
        at = [ap.where(p, c) for c in g["singles"]]
        assert {t % 4 for s, t, c, h in at if t >= 4} == {0, 1, 2, 3}            # every position of the four-buffer ring, past the prologue
        assert all(sum(1 for s, t, c, h in at if t >= 4 and t % 4 == r) >= 2 for r in range(4))
        assert {h for s, t, c, h in at} == {0, 1}                                 # both half-wave column groups
        last = ap.where(p, g["n"] - 1)
        assert g["n"] - 1 in g["singles"] and last[:2] == (p["splits"] - 1, p["tiles"][-1] - 1) and last[2] == p["last_cols"] - 1
        assert p["tiles"][-1] % 2 == 1 and p["tiles"][-1] > 3                     # an odd number of tiles, the winner in the last
        if p["splits"] > 1:
            assert any(s > 0 and t == 0 and c == 0 for s, t, c, h in at)         # the first column of a split > 0
        kinds = set()
        for grp in g["groups"]:
            assert list(grp) == sorted(grp)
            (s0, t0, c0, h0), (s1, t1, c1, h1) = ap.where(p, grp[0]), ap.where(p, grp[-1])
            if (s0, t0) == (s1, t1):
                kinds.add("lanes" if c1 == c0 + 4 else "registers" if c1 == c0 + 8 and h0 == h1 else "?")
            elif s0 == s1:
                assert t1 > t0 >= 4 or len(grp) > 2
                kinds.add("tiles, one lane" if (c0 % 8) // 4 == (c1 % 8) // 4 else "tiles, two lanes")
            else:
                kinds.add("splits")
        assert kinds == {"lanes", "registers", "tiles, one lane", "tiles, two lanes"} | ({"splits"} if p["splits"] > 1 else set())
    p33, p5 = ap.plan_of("TINY33", 50), ap.plan_of("TINY5", 50)
    assert ap.where(p33, 32) == (0, 1, 0, 0) and ap.where(p5, 4) == (0, 0, 4, 1)


@pytest.mark.parametrize("name,d", ap.EXACT_CASES)
def test_exact_cases_are_exact_planted_and_in_range(name, d):
    c = ap.exact_case(name, d)
    E, n = c["E"], c["n"]
    assert E.shape == (n, d) and set(np.unique(E)) <= {-1.0, 0.0, 1.0} and np.count_nonzero(E, axis=1).max() <= ap.NNZ
    assert np.array_equal(ap.bf16_round(E), E)
    assert np.all(np.count_nonzero(E[:, 16 * ((d - 1) // 16):], axis=1) >= 1)  # the last k-step that holds data is never all zero
    for b in (c["bias_a"], c["bias_b"]):
        assert np.array_equal(b, np.rint(b)) and b.min() >= -3 and b.max() <= 3 and np.array_equal(ap.bf16_round(b), b)
    # the float64 product is the integer product
    some = np.random.RandomState(d).randint(0, n, 8)
    Gi = E[some].astype(np.int64) @ E.astype(np.int64).T
    assert np.array_equal(ap.gram(E)[some], Gi) and np.abs(Gi).max() + 3 < 2 ** 24
    # every planted column is the answer for its source row (and for itself: a copy); ties go to the lowest column, and with
    # the last member raised by one, to the last
    ra, rb = c["ref_a"], c["ref_b"]
    for col in c["singles"]:
        u = c["source"][col]
        assert ra["argmax"][u] == rb["argmax"][u] == col and ra["max"][u] == np.count_nonzero(E[u]) + ap.BIAS_WIN
    for grp in c["groups"]:
        u = c["source"][grp[0]]
        assert all(c["source"][m] == u for m in grp)
        assert ra["argmax"][u] == grp[0] and rb["argmax"][u] == grp[-1]
        assert ra["max"][u] == np.count_nonzero(E[u]) + ap.BIAS_TIE and rb["max"][u] == ra["max"][u] + 1
        for m in grp:
            assert ra["argmax"][m] == grp[0] and rb["argmax"][m] == grp[-1]
    # requested rows: repeats, not sorted inside any workgroup's rows, the planted rows present, the last row tile as planned
    rows, p = c["rows"], c["plan"]
    assert len(rows) == c["n_rows"] and rows.min() >= 0 and rows.max() < n and len(np.unique(rows)) < len(rows)
    assert set(c["sources"]) | set(c["source"]) <= set(rows.tolist())
    for t in range(p["row_tiles"]):
        tile = rows[t * p["tile_rows"]:(t + 1) * p["tile_rows"]]
        assert len(tile) == 1 or np.any(np.diff(tile) < 0)
    # the range of the wide kernel's reference-free sum, by the reference alone
    assert ap.in_range(ra) and ap.in_range(rb)
    assert ap.lse_bound(ra, max(p["tiles"])) < 2e-3 * max(abs(ra["lo"]), abs(ra["hi"])) / 50  # far inside the band of the float test


@pytest.mark.parametrize("name,d", ap.DENSE_CASES)
def test_dense_cases_are_in_range(name, d):
    c = ap.dense_case(name, d)
    assert ap.in_range(c["ref"]) and c["ref"]["hi"] > 20  # in range, and far from the few units of the sparse tables
