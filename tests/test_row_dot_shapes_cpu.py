"""The premises of the width tests of the training path (tests/test_gpu_walk_widths.py and the width tests of
tests/test_gpu_graph_softmax.py and tests/test_gpu_steps.py), checked without a GPU: the dispatch lines that
tests/support/row_dot_shapes.py restates are still in the sources; the case lists reach every template instance of the four
kernels that run the spec-S1 row dot; the bit-exact comparison of the walks is sensitive to every part of a row at every width;
and the fp32 score error of the tables, which the graph-softmax tolerance at wide rows is derived from, is the recorded one."""
import os

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.helpers import load_small
from tests.support import row_dot_shapes as rd

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc")


def test_restated_dispatch_is_still_in_the_sources():
    # drift guard: tests/support/row_dot_shapes.py copies these lines.  If this fails after an edit of a source file, the dispatch
    # may have changed: update ld_of / nch_of / instance_of / path_reward_taken / wide and the case lists there (or, after a mere
    # reformat, the texts below)
    copied = {
        "walk_sample.hip": ("const int nch = (a.nchunk + 15) / 16;",
                            "if (nch <= 1) rc = run_levels_and_finish<1>(ctx, a, total_walks);",
                            "else if (nch == 2) rc = run_levels_and_finish<2>(ctx, a, total_walks);",
                            "else if (nch <= 4) rc = run_levels_and_finish<4>(ctx, a, total_walks);",
                            "else if (nch <= 8) rc = run_levels_and_finish<8>(ctx, a, total_walks);"),
        "graph_softmax.hip": ("const int nchunk = ctx->ld / 4, nch = (nchunk + 15) / 16;",
                              "if (nch <= 1) GS_FILL(1);", "else if (nch == 2) GS_FILL(2);", "else if (nch <= 4) GS_FILL(4);",
                              "else GS_FILL(8);"),
        "prepare.hip": ("const int nch = (ctx->ld / 4 + 15) / 16;",
                        "const bool path_reward = window <= 2 && nch <= 4 && ctx->ld % 4 == 0 && !getenv(\"GG_NO_PATH_REWARD\");",
                        "if (nch <= 1) GG_PATH_REWARD(1);", "else if (nch == 2) GG_PATH_REWARD(2);", "else GG_PATH_REWARD(4);"),
        "steps.hip": ("return ctx->sg_threshold > 0 && ctx->ld <= 256 && ctx->cfg.optimizer != GG_OPT_ADAM_DENSE && !getenv(\"GG_NO_STAGED_GRAD\");",
                      "if (which == 0 && whole && ctx->g_paths_valid && ctx->cfg.window_size <= 2 && ctx->ld <= 256 && !getenv(\"GG_NO_PATH_GRAD\")) {"),
        "gg_api.hip": ("if (n_node <= 0 || n_emb <= 0 || n_emb > 512 || !emb_gen || !emb_dis || !cfg)",),
    }
    for name, texts in copied.items():
        src = open(os.path.join(CSRC, name)).read()
        for text in texts:
            assert text in src, "%s no longer contains %r: restate the dispatch in tests/support/row_dot_shapes.py" % (name, text)
    # the restatement itself, at the edges of every rung
    assert [rd.ld_of(d) for d in (1, 4, 5, 509, 512)] == [4, 4, 8, 512, 512]
    assert [rd.nch_of(d) for d in (1, 64, 65, 128, 129, 192, 256, 257, 509, 512)] == [1, 1, 2, 2, 3, 3, 4, 5, 8, 8]
    assert [rd.instance_of(d) for d in (1, 64, 65, 128, 129, 192, 256, 257, 509, 512)] == [1, 1, 2, 2, 4, 4, 4, 8, 8, 8]
    assert rd.MAX_EMB == 512 and max(rd.WIDTHS) == rd.MAX_EMB
    with pytest.raises(AssertionError):
        rd.instance_of(513)
    assert [rd.path_reward_taken(d, 2) for d in (64, 128, 256, 257, 512)] == [True, True, True, False, False]
    assert not rd.path_reward_taken(64, 3)
    assert [rd.wide(d) for d in (253, 256, 257, 260)] == [False, False, True, True]


def test_cases_reach_every_instance_of_the_four_kernels():
    every = {1, 2, 4, 8}
    assert set(rd.INSTANCE_WIDTHS) <= set(rd.WIDTHS)
    assert {rd.instance_of(d) for d in rd.INSTANCE_WIDTHS} == every
    assert sorted(d for d in rd.INSTANCE_WIDTHS if rd.instance_of(d) == 8) == [257, 512]  # <8> at its narrowest and widest
    # level_score_kernel<NCH>: the modes that run the level pipeline
    level_modes = {"levels", "hybrid2", "share_all", "share_off"}
    assert {rd.instance_of(d) for d, m in rd.WALK_CASES if m in level_modes} == every
    for mode in rd.WALK_MODES:  # ... and every mode at every instance
        assert {rd.instance_of(d) for d, m in rd.WALK_CASES if m == mode} == every, mode
    assert {d for d, m in rd.WALK_CASES if m == "levels"} == set(rd.WIDTHS) == {d for d, m in rd.WALK_CASES if m == "finisher"}
    assert len(set(rd.WALK_CASES)) == len(rd.WALK_CASES) == 5 * 5 + 8 * 2
    # walk_sample_kernel<NCH, LAZY>: in a mode in which the finisher really scores hops
    assert set(rd.FINISHER_SCORES) <= set(rd.WALK_MODES) and set(rd.FINISHER_SCORES) <= set(rd.LAZY_MODES)
    for mode in rd.FINISHER_SCORES:
        assert rd.walk_env(mode)["GG_WALK_LEVELS"] in ("0", "2")
    whole = {(rd.instance_of(d), False) for d, m in rd.WALK_CASES if m in rd.FINISHER_SCORES}
    lazy = {(rd.instance_of(d), True) for gi, cap, d, m in rd.LAZY_CASES if m in rd.FINISHER_SCORES}
    assert whole | lazy == {(i, z) for i in every for z in (False, True)}
    assert {d for gi, cap, d, m in rd.LAZY_CASES} >= {128, 256, 257, 512}
    assert {(gi, cap) for gi, cap, d, m in rd.LAZY_CASES} == {(1, 8), (3, 8)}
    # the hub list at a wide row goes through score_block<8> (finisher) and the levels' hub path
    assert rd.instance_of(rd.HUB_WIDTH) == 8 and rd.HUB_LEAVES + 1 > 1024 and {m for d, m in rd.HUB_CASES} == {"finisher", "levels"}
    # gs_fill_kernel<NCH>
    assert {rd.instance_of(d) for d in rd.GS_WIDTHS} == every and set(rd.GS_WIDTHS) >= {129, 256, 257, 512}
    assert set(rd.GS_WIDTHS) == set(rd.E_SCORE)
    # path_reward_kernel<NCH>, and the declined case
    assert {rd.path_reward_instance(d) for d in rd.REWARD_WIDTHS} == {1, 2, 4, None}
    assert set(rd.REWARD_WIDTHS) >= {65, 128, 129, 257, 512}
    assert [d for d in rd.REWARD_WIDTHS if not rd.path_reward_taken(d, 2)] == [257, 512]
    # both sides of ld <= 256 for the staged gradient and the whole-walk passes
    assert {rd.wide(d) for d in rd.PASS_WIDTHS} == {False, True} and set(rd.PASS_WIDTHS) == {256, 260, 512}
    # the environment of the modes: what tests/test_gpu_walk.py's walk_mode fixture sets for these names
    assert rd.walk_env("levels") == {"GG_WALK_LEVELS": "64"} and rd.walk_env("finisher") == {"GG_WALK_LEVELS": "0"}
    assert rd.walk_env("hybrid2") == {"GG_WALK_LEVELS": "2"}
    assert rd.walk_env("share_all") == {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "2"}
    assert rd.walk_env("share_off") == {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0"}


@pytest.fixture(scope="module")
def small1():
    g, n, graph = load_small(1)
    rowptr, col = orc.graph_to_csr(n, graph)
    roots = np.arange(n, dtype=np.int32)
    off, nbr, base, dmax = orc.c_build_trees(n, rowptr, col, roots)
    deg = (rowptr[1:] - rowptr[:-1]).astype(np.int32)
    return n, roots, deg, off, nbr, base, dmax


def _oracle_walks(small1, E, b):
    """samples and path lengths of one D round and one G round (20 walks per root), seed 99, as run_both drives them"""
    n, roots, deg, off, nbr, base, dmax = small1
    nbr = nbr.copy()
    Ep = orc.pad_rows(E)
    out = []
    for r, (for_d, nw) in enumerate(((True, deg), (False, np.full(n, 20, np.int32)))):
        res = orc.c_walk_sample(Ep, b, off, nbr, base, roots, roots, nw, for_d, 99, r, dmax + 3)
        out += [res["samples"], res["path_len"]]
    return np.concatenate(out)


@pytest.mark.parametrize("d", rd.WIDTHS)
def test_walks_change_when_any_part_of_a_row_is_dropped(small1, d):
    """A kernel that drops its last float4 chunk, a whole slot of its instance (64 columns: one chunk per lane), or runs the <4>
    instance on a 512-wide row computes the scores of a table with those columns zeroed: the oracle's walks on such a table must
    differ from the walks on the whole table, or the bit-exact comparison could not see it."""
    n = small1[0]
    E, b = rd.table(n, d)
    assert E.dtype == np.float32 and b.dtype == np.float32 and E.shape == (n, d)
    whole = _oracle_walks(small1, E, b)
    assert len(whole) > 1000
    last = (rd.ld_of(d) // 4 - 1) * 4  # first column of the last float4 chunk
    cuts = [(last, d)] + [(c, min(c + 64, d)) for c in range(0, d, 64)]
    if d > 256:
        cuts.append((256, d))  # what the <4> instance would leave out
    for lo, hi in cuts:
        Z = E.copy()
        Z[:, lo:hi] = 0
        changed = int(np.count_nonzero(_oracle_walks(small1, Z, b) != whole))
        assert changed >= 1, "d = %d: zeroing columns [%d, %d) changes no sample and no path length" % (d, lo, hi)


def test_score_error_of_the_graph_softmax_tables():
    """e(d) of tests/support/row_dot_shapes.py (E_SCORE): the largest |fp32 score - float64 score| over the edges of load_small(3),
    the fp32 score in the oracle's k-ordered fmaf chain.  The recorded value must not be below the measured one (the tolerance
    derived from it would be too tight for the reason it is derived from) and not more than 1 % above it."""
    g, n, graph = load_small(3)
    rowptr, col = orc.graph_to_csr(n, graph)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    for d in rd.GS_WIDTHS:
        E, b = rd.table(n, d)
        s32 = orc.c_all_score_rows(orc.pad_rows(E), b, np.arange(n, dtype=np.int32))[src, col]
        s64 = np.einsum("ij,ij->i", E[src].astype(np.float64), E[col].astype(np.float64)) + b[col].astype(np.float64)
        assert np.std(s64[src != col]) == pytest.approx(1.0, abs=0.25)  # table()'s scaling: scores of order 1 (self-loops: sqrt(d))
        e = float(np.abs(s32.astype(np.float64) - s64).max())
        print("d = %3d: e(d) = %.4e (recorded %.4e)" % (d, e, rd.E_SCORE[d]))
        assert e <= rd.E_SCORE[d] <= 1.01 * e, (d, e)
    # the derived bound: at least the file's own tolerance, and the formula beyond it
    assert rd.logp_tolerance(6, 8, 1e-4) == 1e-4
    assert rd.logp_tolerance(512, 8, 1e-4) == pytest.approx(20 * rd.E_SCORE[512])
