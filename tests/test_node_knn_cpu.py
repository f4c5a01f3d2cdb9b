"""The host side of the k-NN node classifier (graphgan_amd/evaluation/node_knn.py, graph_gan.py's engine_nc_knn, the
``python -m graphgan_amd.neighbors`` command line) -- the vote and its tie rule, the float64 neighbour query against a
pair-by-pair loop, the split, the results line and its place, both refusals -- and the C ABI's declaration of gg_topk_metric."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nknn():
    from graphgan_amd.evaluation import node_knn
    return node_knn


def test_header_declares_and_library_exports_gg_topk_metric():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = ["gg_ctx*", "int32_t", "constint32_t*", "int32_t", "int32_t", "int32_t", "int32_t", "int32_t", "constint32_t*", "int64_t", "int32_t*",
            "float*", "double*"]
    m = re.search(r"int\s+gg_topk_metric\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/graphgan_hip.h does not declare gg_topk_metric"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == want
    assert len(_lib.SIGNATURES["gg_topk_metric"][1]) == len(args)
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "gg_topk_metric") and hasattr(_lib.lib, "gg_topk_metric")
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays


def test_every_topk_instance_is_audited_by_the_build():
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    m = re.search(r"^topk_score\.o: AUDIT = 'topk_\(f32\|bf16\)_kernel' (\d+) ", mk, flags=re.M)
    assert m and int(m.group(1)) == 5 * 3 * 2  # (fp32 + 4 bf16 widths) x metrics x (with, without a bitmap)


def test_vote_majority_and_the_tie_rule(nknn):
    nbr = np.array([[2, 1, 1, 0, 2],    # 1 and 2 tie with two votes: 2 stands first
                    [1, 2, 2, 0, 1],    # the same tie: 1 stands first
                    [0, 1, 2, 3, 3],    # a plain majority that stands last
                    [3, 2, 1, 0, 4],    # all tie: the nearest neighbour's class
                    [4, 4, 0, 0, 1],    # 4 and 0 tie: 4 stands first
                    [1, 0, 0, 1, 2]])   # 1 and 0 tie: 1 stands first, although 0 is the lower class
    assert nknn.vote(nbr, 5).tolist() == [2, 1, 3, 3, 4, 1]
    assert nknn.vote(np.array([[3], [0]]), 4).tolist() == [3, 0]        # k = 1: the nearest neighbour
    assert nknn.vote(np.array([[0, 0, 0]]), 1).tolist() == [0]
    # against the definition, row by row
    rs = np.random.RandomState(4)
    nbr = rs.randint(0, 6, size=(200, 7))
    want = []
    for row in nbr.tolist():
        best = max(row.count(c) for c in set(row))
        want.append(next(c for c in row if row.count(c) == best))
    assert nknn.vote(nbr, 6).tolist() == want


def _loop_neighbours(X, queries, cand, k, metric, exclude_self):
    """the definition pair by pair: (t descending, id ascending)"""
    h = [float(np.dot(x, x)) for x in X]
    w = [1.0 / math.sqrt(v) if v > 0 else 0.0 for v in h]
    cols, scores = [], []
    for u in queries:
        items = []
        for c in sorted(set(cand)):
            if exclude_self and c == u:
                continue
            s = float(np.dot(X[u], X[c]))
            t = s * w[c] if metric == "cosine" else s - 0.5 * h[c] if metric == "l2" else s
            items.append((-t, c))
        items.sort()
        items = items[:k]
        val = [(-t) * w[u] if metric == "cosine" else max(0.0, h[u] - 2.0 * (-t)) if metric == "l2" else -t for t, _ in items]
        pad = k - len(items)
        cols.append([c for _, c in items] + [-1] * pad)
        scores.append(val + [np.inf if metric == "l2" else -np.inf] * pad)
    return np.array(cols), np.array(scores)


@pytest.mark.parametrize("metric", ["dot", "cosine", "l2"])
def test_host_neighbours_against_the_pair_loop(nknn, metric):
    rs = np.random.RandomState(11)
    X = rs.randint(-1, 2, size=(60, 6)).astype(np.float64)  # small integers: ties are frequent, every t is exact
    X[7] = 0.0
    X[20] = 0.0
    queries = np.array([0, 7, 59, 7, 33])
    cand = np.array([5, 7, 20, 59, 58, 5, 0, 1, 2, 3, 33, 40, 41])
    for k, ex in ((1, False), (4, True), (12, True), (20, False)):
        col, score = nknn.host_neighbours(X, queries, cand, k, metric=metric, exclude_self=ex, block=2)
        want_col, want_score = _loop_neighbours(X, queries.tolist(), cand.tolist(), k, metric, ex)
        assert np.array_equal(col, want_col), (metric, k, ex)
        assert np.array_equal(score, want_score), (metric, k, ex)
        for c, row in zip(col, score):  # nearest first, the padding behind
            if metric == "l2":
                assert np.all(row[:-1] <= row[1:]) and np.all(row[c < 0] == np.inf)
            else:
                assert np.all(row[:-1] >= row[1:]) and np.all(row[c < 0] == -np.inf)
    with pytest.raises(ValueError, match="metric"):
        nknn.host_neighbours(X, queries, cand, 3, metric="manhattan")


def _two_blobs(n=120, d=6, seed=2):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 3, size=n)
    centres = 4.0 * rs.randn(3, d)
    return centres[y] + rs.randn(n, d), y


def test_split_is_the_classifiers_and_the_evaluator_classifies(nknn, tmp_path):
    from graphgan_amd.evaluation import node_classification as nc
    X, y = _two_blobs()
    n = len(X)
    path = str(tmp_path / "labels.txt")
    labelled = np.arange(0, n, 2)
    with open(path, "w") as f:
        f.writelines("%d %d\n" % (v, 7 * y[v]) for v in labelled)
    ev = nknn.NodeKnnEval(path, n, X.shape[1], emd=X, k=5, metric="l2", train_ratio=0.75, seed=3)
    ref = nc.NodeClassifyEval(None, path, n, X.shape[1], emd=X, train_ratio=0.75, seed=3)
    for a, b in zip(ev.split(), ref.split()):
        assert np.array_equal(a, b)
    tr_n, tr_y, te_n, te_y, n_class = ev.split()
    res = ev.eval_node_knn()
    assert (res["k"], res["metric"], res["n_train"], res["n_test"]) == (5, "l2", len(tr_n), len(te_n)) and res["n_train"] == 45
    # the same protocol spelled out
    class_of = dict(zip(tr_n.tolist(), tr_y.tolist()))
    col, _ = _loop_neighbours(X, te_n.tolist(), tr_n.tolist(), 5, "l2", False)
    pred = nknn.vote(np.array([[class_of[c] for c in row] for row in col.tolist()]), n_class)
    assert (res["acc"], res["macro_f1"]) == nc.metrics(te_y, pred, n_class) and res["acc"] > 0.9
    line = nknn.format_results("gen", res)
    assert line == "gen_knn:acc=%s macro_f1=%s k=5 metric=l2 n_train=45 n_test=15\n" % (str(res["acc"]), str(res["macro_f1"]))
    for bad, text in ((dict(k=0), "k must be"), (dict(k=257), "k must be"), (dict(k=True), "k must be"), (dict(metric="l1"), "metric"),
                      (dict(engine=object(), precision="fp16"), "precision")):
        with pytest.raises(ValueError, match=text):
            nknn.NodeKnnEval(path, n, X.shape[1], **dict(dict(emd=X), **bad))
    with pytest.raises(ValueError, match="needs an engine or the embedding matrix"):
        nknn.NodeKnnEval(path, n, X.shape[1])
    with pytest.raises(ValueError, match="k = 46 exceeds the 45 training nodes"):
        nknn.NodeKnnEval(path, n, X.shape[1], emd=X, k=46, train_ratio=0.75, seed=3).eval_node_knn()


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def _labels_for(cfg, n, tmp_path, count=None):
    rs = np.random.RandomState(5)
    nodes = np.sort(rs.permutation(n)[:count or n // 4])
    cfg.labels_filename = str(tmp_path / "labels.txt")
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d\t%d\n" % (v, 10 * int(c)) for v, c in zip(nodes, rs.randint(0, 4, size=len(nodes))))
    return nodes


def test_config_knobs_default_off():
    from graphgan_amd import config
    assert config.engine_nc_knn is False
    assert (config.engine_knn_k, config.engine_knn_metric, config.engine_knn_precision) == (10, "cosine", "fp32")


def test_evaluation_lines_with_and_without_the_knob(nknn, tmp_path):
    from graphgan_amd import utils
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    assert cfg.engine_nc_knn is False
    _labels_for(cfg, n, tmp_path)
    cfg.engine_emb_spectrum = cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    want = GraphGAN.evaluation(g)  # the knob's default: off
    del cfg.engine_nc_knn, cfg.engine_knn_k, cfg.engine_knn_metric, cfg.engine_knn_precision
    assert GraphGAN.evaluation(g) == want and len(want) == 5  # a user's config without the knobs
    assert open(cfg.result_filename).read() == "".join(want + want) and "_knn" not in "".join(want)
    cfg.engine_nc_knn = True  # the other knobs absent: their defaults
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "gen_spec", "dis_spec", "gen_knn", "dis_knn", "gen_nll"]
    assert lines[:4] == want[:4] and lines[6] == want[4]
    for i, (mode, line) in enumerate(zip(cfg.modes, lines[4:6])):
        emd = utils.read_embeddings(cfg.emb_filenames[i], n_node=n, n_embed=cfg.n_emb)
        res = nknn.NodeKnnEval(cfg.labels_filename, n, cfg.n_emb, emd=emd, k=10, metric="cosine", train_ratio=0.9, seed=g.seed).eval_node_knn()
        assert line == nknn.format_results(mode, res)
        assert re.fullmatch(r"%s_knn:acc=\S+ macro_f1=\S+ k=10 metric=cosine n_train=\d+ n_test=\d+\n" % mode, line)
    assert open(cfg.result_filename).read() == "".join(want + want + lines)
    cfg.engine_knn_k, cfg.engine_knn_metric = 3, "l2"
    assert " k=3 metric=l2 " in GraphGAN.evaluation(g)[4]


def test_both_refusals_come_before_anything_is_computed(tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_node_knn
    cfg, g, n = _layout(tmp_path)
    cfg.engine_nc_knn = True
    cfg.labels_filename = str(tmp_path / "no_such_labels.txt")
    with pytest.raises(ValueError, match="engine_nc_knn needs labels: config.labels_filename does not exist"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    with pytest.raises(ValueError, match="labels_filename"):
        _check_node_knn(types.SimpleNamespace(engine_nc_knn=True))
    _labels_for(cfg, n, tmp_path, count=10)  # 9 training nodes
    with pytest.raises(ValueError, match="k = 10 exceeds the 9 training nodes"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    cfg.engine_knn_k = 9
    assert len(GraphGAN.evaluation(g)) == 4
    cfg.engine_knn_metric = "manhattan"
    with pytest.raises(ValueError, match="engine_knn_metric"):
        GraphGAN.evaluation(g)
    _check_node_knn(types.SimpleNamespace())  # knobs absent: nothing to check


def test_command_line_on_the_host(nknn, tmp_path):
    from graphgan_amd import neighbors
    rs = np.random.RandomState(6)
    ids = np.array([3, 4, 9, 10, 11, 20, 21, 22, 40])
    X = rs.randint(-2, 3, size=(len(ids), 4)).astype(np.float64)
    emb, out, nodes = str(tmp_path / "x.emb"), str(tmp_path / "nn.tsv"), str(tmp_path / "ids.txt")
    with open(emb, "w") as f:
        f.write("%d\t4\n" % len(ids))
        for i in rs.permutation(len(ids)):  # rows in any order
            f.write("%d\t%s\n" % (ids[i], "\t".join(repr(float(v)) for v in X[i])))
    for metric in ("cosine", "l2", "dot"):
        assert neighbors.main(["--emb", emb, "--k", "3", "--metric", metric, "--host", "--out", out]) == 0
        rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
        assert len(rows) == 3 * len(ids) and all(len(r) == 3 for r in rows)
        col, score = _loop_neighbours(X, list(range(len(ids))), list(range(len(ids))), 3, metric, True)
        assert [int(r[0]) for r in rows] == np.repeat(ids, 3).tolist()
        assert [int(r[1]) for r in rows] == ids[col].ravel().tolist()
        assert [float(r[2]) for r in rows] == score.ravel().tolist()
        assert all(r[0] != r[1] for r in rows)  # self excluded
    with open(nodes, "w") as f:
        f.write("21\n4 40\n")
    assert neighbors.main(["--emb", emb, "--k", "2", "--nodes", nodes, "--host", "--out", out]) == 0  # the default metric: cosine
    rows = [ln.split("\t") for ln in open(out)]
    col, _ = _loop_neighbours(X, [6, 1, 8], list(range(len(ids))), 2, "cosine", True)
    assert [int(r[0]) for r in rows] == [21, 21, 4, 4, 40, 40] and [int(r[1]) for r in rows] == ids[col].ravel().tolist()
    for bad in (["--k", "0"], ["--k", "9"], ["--k", "2", "--metric", "l1"]):
        with pytest.raises(SystemExit):
            neighbors.main(["--emb", emb, "--host", "--out", out] + bad)
    with open(nodes, "w") as f:
        f.write("5\n")
    with pytest.raises(SystemExit):
        neighbors.main(["--emb", emb, "--k", "2", "--nodes", nodes, "--host", "--out", out])
