"""Recommendation evaluator on the host (no GPU): hand-computed P@K / R@K on a toy graph (ties included), the results line
format, and the argument checks of Engine.topk that happen before the device is touched."""
import numpy as np
import pytest

from graphgan_amd.evaluation import recommendation as rec


def _write(path, edges):
    with open(path, "w") as f:
        f.writelines("%d\t%d\n" % e for e in edges)
    return str(path)


# 6 nodes.  Embeddings (1-d and 2-d mixes) chosen so that the rankings are easy to write down:
#   e0 = (1, 0), e1 = (1, 0), e2 = (0.5, 0), e3 = (0.5, 0), e4 = (0, 1), e5 = (-1, 0)
# scores of node 0: s(0, 1) = 1, s(0, 2) = s(0, 3) = 0.5 (a tie: column 2 first), s(0, 4) = 0, s(0, 5) = -1
EMB = np.array([[1, 0], [1, 0], [0.5, 0], [0.5, 0], [0, 1], [-1, 0]], dtype=np.float64)
TRAIN = [(0, 1), (4, 5)]        # excluded for the ranking: 0 - 1, 4 - 5 (and every node itself)
TEST = [(0, 3), (2, 0), (4, 2)]  # undirected: T(0) = {2, 3}, T(2) = {0, 4}, T(3) = {0}, T(4) = {2}


def test_host_ranking_excludes_self_and_training_neighbours_and_breaks_ties_by_column():
    nb = rec._neighbour_sets(TRAIN, 6)
    got = rec.host_topk(EMB, [0, 2, 4], nb, 6)
    # node 0: eligible 2, 3, 4, 5 -> 0.5 (2), 0.5 (3), 0 (4), -1 (5); padded with -1
    assert got[0].tolist() == [2, 3, 4, 5, -1, -1]
    # node 2: eligible 0, 1, 3, 4, 5 -> 0.5 (0), 0.5 (1), 0.25 (3), 0 (4), -0.5 (5)
    assert got[1].tolist() == [0, 1, 3, 4, 5, -1]
    # node 4: eligible 0, 1, 2, 3 (5 is a neighbour): all score 0 -> column order
    assert got[2].tolist() == [0, 1, 2, 3, -1, -1]


def test_precision_recall_by_hand(tmp_path):
    tr, te = _write(tmp_path / "train.txt", TRAIN), _write(tmp_path / "test.txt", TEST)
    res = rec.RecommendEval("unused", tr, te, 6, 2, emd=EMB, ks=(1, 2, 3)).eval_recommendation()
    # queries 0, 2, 3, 4 (the nodes with a test edge); rankings:
    #   0: [2, 3, 4, ...]  T = {2, 3}
    #   2: [0, 1, 3, ...]  T = {0, 4}
    #   3: [0, 1, 2, ...]  (0.5, 0.5, 0.25)  T = {0}
    #   4: [0, 1, 2, ...]  (all 0: column order)  T = {2}
    # K = 1: hits 1, 1, 1, 0 -> P = 3/4,  R = (1/2 + 1/2 + 1 + 0) / 4
    # K = 2: hits 2, 1, 1, 0 -> P = 4/8,  R = (1 + 1/2 + 1 + 0) / 4
    # K = 3: hits 2, 1, 1, 1 -> P = 5/12, R = (1 + 1/2 + 1 + 1) / 4
    want = {1: (3 / 4, 2.0 / 4), 2: (4 / 8, 2.5 / 4), 3: (5 / 12, 3.5 / 4)}
    for K in (1, 2, 3):
        assert res[K][0] == pytest.approx(want[K][0], abs=1e-15) and res[K][1] == pytest.approx(want[K][1], abs=1e-15)


def test_precision_recall_of_a_given_ranking():
    ranked = np.array([[3, 2, -1], [5, 4, 0]])
    t = [set() for _ in range(6)]
    t[1], t[2] = {2, 3}, {0}
    res = rec.precision_recall(ranked, [1, 2], t, (1, 3))
    assert res[1] == (0.5, 0.25)
    assert res[3] == pytest.approx(((2 / 3 + 1 / 3) / 2, (1 + 1) / 2))


def test_results_line_format():
    line = rec.format_results("gen", {2: (0.5, 0.25), 10: (0.1, 1.0), 20: (0.05, 1.0)}, (2, 10, 20))
    assert line == "gen:P@2=0.5 R@2=0.25 P@10=0.1 R@10=1.0 P@20=0.05 R@20=1.0\n"


def test_evaluator_rejects_k_outside_the_device_range(tmp_path):
    with pytest.raises(ValueError):
        rec.RecommendEval("unused", "t", "t", 6, 2, emd=EMB, ks=(0, 10))
    with pytest.raises(ValueError):
        rec.RecommendEval("unused", "t", "t", 6, 2, emd=EMB, ks=(300,))


def test_config_knobs():
    from graphgan_amd import config
    assert tuple(config.engine_rec_ks) == (2, 10, 20) and config.engine_rec_precision == "fp32"


def test_engine_topk_validates_before_the_device():
    """Engine.topk rejects a bad k / which / precision with ValueError before any library call (no context needed)"""
    import graphgan_amd as ga
    eng = ga.Engine.__new__(ga.Engine)  # no device context: a call that reached the library would fail differently
    eng.n_node = 10
    for bad in (dict(k=0), dict(k=257), dict(k=2.5), dict(which=2), dict(precision="fp16")):
        with pytest.raises(ValueError):
            eng.topk([0], **bad)
