"""The host side of node clustering (graphgan_amd/evaluation/node_clustering.py, graph_gan.py's engine_node_clustering): the
partition scores on hand tables, the float64 k-means (stop rule, tie rule, empty clusters, seeding) on blobs, the results line,
the knobs -- and the C ABI's declaration of gg_kmeans_step / gg_kmeans_fit."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests.support import kmeans_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ncl():
    from graphgan_amd.evaluation import node_clustering
    return node_clustering


def test_header_declares_and_library_exports_the_kmeans_entry_points():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {
        "gg_kmeans_step": ["gg_ctx*", "int", "constint32_t*", "int64_t", "int", "constfloat*", "constint32_t*", "int32_t*", "float*", "float*",
                           "int32_t*", "double*"],
        "gg_kmeans_fit": ["gg_ctx*", "int", "constint32_t*", "int64_t", "int", "int", "float*", "constint32_t*", "int32_t*", "float*", "int32_t*",
                          "double*", "int32_t*", "int32_t*", "double*"],
    }
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name)
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9  # additive: the ABI number stays


def test_kmeans_kernels_are_audited_by_the_build():
    csrc = os.path.join(ROOT, "graphgan_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^OBJ = .*\bkmeans\.o\b", mk, flags=re.M) and re.search(r"^AUDITED = .*\bkmeans\.o\b", mk, flags=re.M)
    assert "km_[a-z_]*kernel" in mk
    remarks = os.path.join(csrc, "kmeans.remarks")
    assert os.path.exists(remarks), "kmeans.remarks is written by the build (make -C graphgan_amd/csrc)"
    text = open(remarks).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 66 and all("km_" in x and "kernel" in x for x in names), names  # kernels only: nothing behind a call
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 66


# ---- the scores
def test_metrics_on_the_hand_table(ncl):
    res = ncl.cluster_metrics([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2])
    assert res["nmi"] == pytest.approx(0.5158037429793889, rel=1e-14)
    assert res["ari"] == pytest.approx(0.24242424242424243, rel=1e-14)
    assert res["purity"] == 5 / 6
    assert ncl.contingency([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2]).tolist() == [[2, 1, 0], [0, 1, 2]]


def test_metrics_at_the_ends(ncl):
    u = np.array([3, 3, 7, 7, 7, 1, 1, 3])
    assert ncl.cluster_metrics(u, 10 - u) == dict(nmi=pytest.approx(1.0, rel=1e-15), ari=1.0, purity=1.0)  # a relabelling of itself
    assert ncl.cluster_metrics([4, 4, 4], [0, 0, 0]) == dict(nmi=1.0, ari=1.0, purity=1.0)  # two single-cluster partitions
    res = ncl.cluster_metrics([0, 0, 1, 1], [0, 1, 0, 1])
    assert res["nmi"] == pytest.approx(0.0, abs=1e-15) and res["ari"] == pytest.approx(-0.5, rel=1e-15) and res["purity"] == 0.5


# ---- the host k-means
@pytest.mark.parametrize("k,d,per", kr.BLOB_SHAPES)
def test_host_kmeans_on_blobs_from_a_good_start(ncl, k, d, per):
    X, labels, first = kr.blobs(k, d, per)
    assert X.dtype == np.float32 and X.shape == (k * per, d) and np.array_equal(labels[first], np.arange(k))
    res = ncl.host_kmeans_fit(X, X[first], 100)
    assert res["iters"] == 2 and res["converged"] is True and len(res["inertia"]) == 2
    assert np.array_equal(res["assign"], labels) and res["counts"].tolist() == [per] * k
    assert ncl.cluster_metrics(labels, res["assign"]) == dict(nmi=pytest.approx(1.0, rel=1e-14), ari=1.0, purity=1.0)
    means = np.stack([X[labels == c].astype(np.float64).mean(axis=0) for c in range(k)])
    assert np.allclose(res["centroids"], means, rtol=0, atol=1e-12)
    a, dist2 = ncl.host_assign(X, res["centroids"])  # the returned state is consistent and a fixed point
    assert np.array_equal(a, res["assign"]) and np.array_equal(dist2, res["dist2"]) and float(dist2.sum()) == res["inertia"][-1]
    assert res["inertia"][1] <= res["inertia"][0]


def test_host_kmeans_stop_rule_without_a_last_update(ncl):
    X, labels, first = kr.blobs(5, 16, 60)
    start = X[kr.bad_start(labels, first)].astype(np.float64)
    one = ncl.host_kmeans_fit(X, start, 1)
    assert one["iters"] == 1 and one["converged"] is False and np.array_equal(one["centroids"], start)  # no update at max_iters
    full = ncl.host_kmeans_fit(X, start, 100)
    assert full["converged"] and 2 <= full["iters"] < 100 and (np.diff(full["inertia"]) <= 1e-9 * full["inertia"][0]).all()
    cut = ncl.host_kmeans_fit(X, start, full["iters"] - 1)
    assert cut["iters"] == full["iters"] - 1 and not cut["converged"]
    a, _ = ncl.host_assign(X, cut["centroids"])
    assert np.array_equal(a, cut["assign"])
    with pytest.raises(ValueError, match="max_iters"):
        ncl.host_kmeans_fit(X, start, 0)


def test_host_kmeans_ties_and_the_empty_cluster(ncl):
    X, labels, first = kr.blobs(5, 16, 60)
    start = X[first].astype(np.float64)
    start[4] = start[1]  # two identical centroids: every tie goes to cluster 1, cluster 4 gets no row
    res = ncl.host_kmeans_fit(X, start, 1)
    assert res["counts"][4] == 0 and (res["counts"][:4] > 0).all() and not (res["assign"] == 4).any()
    # a sixth centroid far from every row stays empty through the whole fit, keeps its bits and is counted as empty
    start = np.concatenate([X[first].astype(np.float64), np.full((1, 16), 100.0 + 1.0 / 3)])
    res = ncl.host_kmeans_fit(X, start, 100)
    assert res["converged"] and res["iters"] == 2 and res["counts"].tolist() == [60] * 5 + [0]
    assert np.array_equal(res["centroids"][5], start[5]) and int((res["counts"] == 0).sum()) == 1
    assert np.array_equal(res["assign"], labels)
    a, _ = ncl.host_assign(np.zeros((3, 2)), np.ones((4, 2)))  # all scores tie: the lowest cluster
    assert a.tolist() == [0, 0, 0]


def test_host_seeding_follows_the_stated_rule(ncl):
    from graphgan_amd.engine import kmeans_pp_positions
    X, labels, _ = kr.blobs(5, 16, 60)
    pos = ncl.host_kmeans_seed(X, 5, 3)
    assert pos.dtype == np.int64 and pos.shape == (5,) and (pos >= 0).all() and (pos < len(X)).all()
    assert np.array_equal(pos, ncl.host_kmeans_seed(X, 5, 3)) and not np.array_equal(pos, ncl.host_kmeans_seed(X, 5, 4))
    assert sorted(labels[pos].tolist()) == [0, 1, 2, 3, 4]  # D^2 sampling on separated blobs: one centre per blob
    # the rule, restated
    rs = np.random.RandomState([3, 0x4B4D])
    want = [int(rs.randint(len(X)))]
    X64 = X.astype(np.float64)
    while len(want) < 5:
        cum = np.cumsum(kr.f64_dist(X64, X64[want]).min(axis=1))
        want.append(min(int(np.searchsorted(cum, rs.random_sample() * cum[-1], side="right")), len(X) - 1))
    assert [int(labels[p]) for p in pos] == [int(labels[p]) for p in want]  # (two float64 forms of one distance: the blob, not the bit)
    # total == 0: uniform draws
    rs = np.random.RandomState([9, 0x4B4D])
    assert kmeans_pp_positions(7, 3, 9, lambda chosen: np.zeros(7)).tolist() == [int(rs.randint(7)) for _ in range(3)]
    # a draw at the very end of the cumulative sum stays inside
    assert (kmeans_pp_positions(4, 4, 1, lambda chosen: np.array([0.0, 0.0, 0.0, 1.0])) <= 3).all()


# ---- the evaluator and graph_gan.evaluation()
def _write_emb(path, emb):
    with open(path, "w") as f:
        f.write("%d\t%d\n" % emb.shape)
        for i, row in enumerate(np.asarray(emb, dtype=np.float64).tolist()):
            f.write(str(i) + "\t" + "\t".join(repr(x) for x in row) + "\n")


def _blob_files(tmp_path, k=5, d=16, per=60):
    X, labels, _ = kr.blobs(k, d, per)
    emb, lab = str(tmp_path / "blobs.emb"), str(tmp_path / "labels.txt")
    _write_emb(emb, X)
    with open(lab, "w") as f:
        f.writelines("%d %d\n" % (i, 100 + 3 * int(c)) for i, c in enumerate(labels))
    return X, labels, emb, lab


def test_evaluator_on_blobs_and_the_results_line(ncl, tmp_path):
    X, labels, emb, lab = _blob_files(tmp_path)
    ev = ncl.NodeClusterEval(emb, lab, len(X), X.shape[1], n_init=4, max_iters=100, seed=0)
    res = ev.eval_node_clustering()
    assert res["nmi"] == pytest.approx(1.0, rel=1e-14) and res["ari"] == 1.0 and res["purity"] == 1.0
    assert (res["k"], res["n"], res["empty"]) == (5, 300, 0) and 2 <= res["iters"] <= 100
    want_inertia = sum(((X[labels == c].astype(np.float64) - X[labels == c].astype(np.float64).mean(axis=0)) ** 2).sum() for c in range(5))
    assert res["inertia"] == pytest.approx(want_inertia, rel=1e-9)
    line = ncl.format_results("gen", res)
    assert line == "gen_cluster:NMI=%s ARI=1.0 purity=1.0 inertia=%s k=5 n=300 iters=%d empty=0\n" % (str(res["nmi"]), str(res["inertia"]), res["iters"])
    assert re.fullmatch(r"gen_cluster:NMI=\S+ ARI=\S+ purity=\S+ inertia=\S+ k=\d+ n=\d+ iters=\d+ empty=\d+\n", line)
    assert ncl.NodeClusterEval(emb, lab, len(X), X.shape[1], emd=X.astype(np.float64)).eval_node_clustering() == res  # emd = the text
    two = ncl.NodeClusterEval(emb, lab, len(X), X.shape[1], k=2, n_init=1).eval_node_clustering()
    assert two["k"] == 2 and two["purity"] == pytest.approx(2 / 5) and 0.0 < two["nmi"] < 1.0
    with pytest.raises(ValueError, match="fewer than k"):
        ncl.NodeClusterEval(emb, _few_labels(tmp_path), len(X), X.shape[1], emd=X, k=4).eval_node_clustering()
    for bad in (dict(k=-1), dict(k=129), dict(k=2.5), dict(n_init=0), dict(max_iters=0), dict(max_iters=True)):
        with pytest.raises(ValueError, match="node clustering"):
            ncl.NodeClusterEval(emb, lab, len(X), X.shape[1], emd=X, **bad)


def _few_labels(tmp_path):
    path = str(tmp_path / "few.txt")
    with open(path, "w") as f:
        f.write("0 1\n5 2\n9 1\n")
    return path


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def _labels_for(cfg, n, tmp_path):
    """a labels file over two thirds of the fixture's nodes, 4 label values"""
    rs = np.random.RandomState(5)
    nodes = np.sort(rs.permutation(n)[:2 * n // 3])
    cfg.labels_filename = str(tmp_path / "labels.txt")
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d\t%d\n" % (v, 10 * int(c)) for v, c in zip(nodes, rs.randint(0, 4, size=len(nodes))))
    return nodes


def test_config_knobs_default_off():
    from graphgan_amd import config
    assert config.engine_node_clustering is False
    assert (config.engine_cluster_k, config.engine_cluster_n_init, config.engine_cluster_max_iters) == (0, 4, 100)


def test_evaluation_lines_with_and_without_the_knob(ncl, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    assert cfg.engine_node_clustering is False
    want = GraphGAN.evaluation(g)  # the knob's default: off
    del cfg.engine_node_clustering
    assert GraphGAN.evaluation(g) == want and len(want) == 2  # a user's config without the knob
    assert open(cfg.result_filename).read() == "".join(want + want) and "_cluster" not in "".join(want)
    nodes = _labels_for(cfg, n, tmp_path)
    cfg.engine_node_clustering, cfg.engine_cluster_n_init, cfg.engine_cluster_max_iters = True, 2, 30
    cfg.engine_link_rank, cfg.engine_gen_nll = True, True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    lines = GraphGAN.evaluation(g)
    assert lines[:2] == want and len(lines) == 7
    assert [ln.split(":")[0] for ln in lines[2:]] == ["gen_rank", "dis_rank", "gen_cluster", "dis_cluster", "gen_nll"]
    for i, (mode, line) in enumerate(zip(cfg.modes, lines[4:6])):
        ev = ncl.NodeClusterEval(cfg.emb_filenames[i], cfg.labels_filename, n, cfg.n_emb, n_init=2, max_iters=30, seed=g.seed)
        res = ev.eval_node_clustering()
        assert line == ncl.format_results(mode, res)
        assert (res["k"], res["n"]) == (4, len(nodes)) and 0.0 <= res["nmi"] <= 1.0 and -1.0 <= res["ari"] <= 1.0 and 0.25 <= res["purity"] <= 1.0
    assert open(cfg.result_filename).read() == "".join(want + want + lines)
    cfg.engine_cluster_k = 7
    assert " k=7 " in GraphGAN.evaluation(g)[4]


def test_evaluation_with_the_knob_needs_the_labels_file(tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_node_clustering
    cfg, g, _ = _layout(tmp_path)
    cfg.engine_node_clustering = True
    cfg.labels_filename = str(tmp_path / "no_such_labels.txt")
    with pytest.raises(ValueError, match="engine_node_clustering needs labels.*labels_filename"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
    with pytest.raises(ValueError, match="labels_filename"):
        _check_node_clustering(types.SimpleNamespace(engine_node_clustering=True))
    _check_node_clustering(types.SimpleNamespace())  # knob absent: nothing to check
