"""The premises of tests/test_gpu_classifier_shapes.py, checked without a GPU: the restated launch plan of the classifier's
sweep names exactly the six k-chunked instances and the case lists reach every one of the 64 template instances; the closed
forms of the exact row accounting (tests/support/classifier_shapes.py) equal the float64 restatements to float32 rounding and
keep every partial sum below 2^24."""
import os

import numpy as np
import pytest

from tests.support import classifier_ml_ref as ml_ref
from tests.support import classifier_ref as ref
from tests.support import classifier_shapes as cs


def test_restated_plan_names_the_six_chunked_instances():
    chunked = {}
    for CT in range(1, 5):
        for DT in range(1, 9):
            p = cs.sweep_plan(32 * CT, 32 * DT)
            assert (p["CT"], p["DT"]) == (CT, DT) and sum(p["chunks"]) == 32 * DT
            assert p["lds"] <= cs.NC_LDS and p["KW"] % 4 == 0 and all(k % 2 == 0 for k in p["chunks"])
            if p["KW"] < 32 * DT:
                chunked[(CT, DT)] = p["chunks"]
    assert set(chunked) == cs.CHUNKED
    assert chunked == {(4, 5): [152, 8], (4, 6): [136, 56], (4, 7): [120, 104], (4, 8): [104, 104, 48], (3, 7): [184, 40],
                       (3, 8): [160, 96]}
    # drift guard: the restatement copies these constants and these lines of row_tile_plan from the header the classifier's and
    # the k-means sweep share.  If this fails after an edit of row_tiles.h, the plan may have changed: update
    # tests/support/classifier_shapes.py (or, after a mere reformat, the texts below)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc", "row_tiles.h")).read()
    for text in ("constexpr int RT_ROWS = 64;", "constexpr int RT_MAX_GRID = 512;", "constexpr size_t RT_LDS = 150 * 1024;",
                 "int KW = (int)((RT_LDS - fixed) / (sizeof(float) * 32 * CT)) - 1;", "KW = KW >= ld ? ld : (KW / 4) * 4;",
                 "const size_t fixed = sizeof(float) * RT_ROWS * ((size_t)(32 * DT + 1) + (32 * CT + 1));"):
        assert text in src, "row_tiles.h no longer contains %r: restate row_tile_plan in tests/support/classifier_shapes.py" % text


def test_cases_reach_every_instance_and_every_path():
    small = {(cs.sweep_plan(C, cs.ld_of(d))["CT"], cs.sweep_plan(C, cs.ld_of(d))["DT"]) for C, d in cs.INSTANCE_CASES}
    assert small == {(CT, DT) for CT in range(1, 5) for DT in range(1, 9)}  # x 2 variants: all 64 entries of nc_sweeps
    assert cs.cdiv(cs.M_SMALL, cs.NC_RT) == 3 and cs.M_SMALL % cs.NC_RT == 2
    # ragged: every case is over a tile edge in C or d; the last chunks differ from the full-tile ones
    plans = {(C, d): cs.sweep_plan(C, cs.ld_of(d)) for C, d in cs.RAGGED_CASES}
    assert plans[(96, 225)]["chunks"] == [160, 68] and plans[(127, 161)]["chunks"] == [136, 28] and plans[(128, 193)]["chunks"] == [120, 76]
    assert plans[(97, 129)]["chunks"] == [132]  # (4, 5) at ld = 132: resident after all
    assert plans[(3, 1)]["chunks"] == [4] and plans[(2, 3)]["chunks"] == [4]
    # multi-tile: more tiles than workgroups, a second and a third trip of the persistent loop, short last tiles
    for M, d, C in cs.MULTI_TILE_CASES:
        assert cs.cdiv(M, cs.NC_RT) > cs.NC_MAX_GRID and cs.grid_of(M) == cs.NC_MAX_GRID
    assert cs.cdiv(cs.M1, 64) == 513 and cs.M1 - 512 * 64 == 1
    assert cs.cdiv(cs.M2, 64) == 1062 and 1062 - 2 * 512 == 38 and cs.M2 - 1061 * 64 == 5
    last = {(d, C): cs.sweep_plan(C, cs.ld_of(d))["chunks"] for d, C in cs.MULTI_TILE_SHAPES}
    assert last[(224, 96)] == [184, 40] and last[(160, 128)] == [152, 8] and last[(256, 128)] == [104, 104, 48]
    assert last[(8, 2)] == [8] and last[(50, 40)] == [52]
    # predict: more than 48 KiB of LDS, three trips of the row loop
    for C, d in cs.PREDICT_CASES:
        assert 4 * (C * (d + 1) + 4 * d) > 48 * 1024
    assert cs.cdiv(cs.M_PREDICT, 4 * 1024) == 3


def _one_ulp(got, want64):
    """|got - want| within one float32 spacing of the float64 value"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    return np.all(np.abs(got - want64) <= np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64))


@pytest.mark.parametrize("M,d,C", cs.MULTI_TILE_CASES + [(cs.M_SMALL, 256, 128), (cs.M_SMALL, 3, 2)])
def test_closed_forms_equal_the_float64_restatement(M, d, C):
    rs = np.random.RandomState(M + d + C)
    nodes = cs.draw_nodes(rs, M)
    X = cs.int_tables(d)[0][nodes]
    W, b = np.zeros((C, d)), np.zeros(C)
    assert cs.headroom(X, C) < 2 ** 24
    Y = cs.draw_label_sets(rs, M, C)
    assert Y[1].all() and not Y[2].any() and Y[:, C - 1].sum() == 1
    loss, gW, gb = ml_ref.lossgrad(X, Y, W, b, 0.0, np.float64)
    eW, eb = cs.exact_sigmoid(X, Y)
    assert eW.dtype == np.float32 and eb.dtype == np.float32
    assert _one_ulp(eW, gW) and _one_ulp(eb, gb) and loss == pytest.approx(C * np.log(2), rel=1e-12)
    assert np.any(eW != 0) and np.all(eb != 0)
    if cs.is_pow2(C):
        y = cs.draw_labels(rs, M, C)
        assert not np.any(y == C - 1)
        loss, gW, gb = ref.lossgrad(X, y, W, b, 0.0, np.float64)
        eW, eb = cs.exact_softmax(X, y, C)
        assert _one_ulp(eW, gW) and _one_ulp(eb, gb) and loss == pytest.approx(np.log(C), rel=1e-12)
        assert eb[C - 1] == np.float32(1.0 / C)  # the class without a row: M / C over M

