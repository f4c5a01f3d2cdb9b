"""The host side of the silhouette (graphgan_amd/evaluation/node_silhouette.py, graph_gan.py's engine_cluster_silhouette): the
float64 references against a pair-by-pair double loop, singleton and empty clusters, the tie rule, the results line and its
place, the knobs -- and the C ABI's declaration of gg_silhouette."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests.support import silhouette_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nsil():
    from graphgan_amd.evaluation import node_silhouette
    return node_silhouette


def test_header_declares_and_library_exports_gg_silhouette():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = ["gg_ctx*", "int", "constint32_t*", "constint32_t*", "int64_t", "int", "constint64_t*", "int64_t", "int", "float*", "float*", "float*",
            "int32_t*", "double*", "double*"]
    m = re.search(r"int\s+gg_silhouette\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/graphgan_hip.h does not declare gg_silhouette"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == want
    assert len(_lib.SIGNATURES["gg_silhouette"][1]) == len(args)
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "gg_silhouette")
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9  # additive: the ABI number stays


def test_silhouette_kernels_are_audited_by_the_build():
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJ = .*\bsilhouette\.o\b", mk, flags=re.M) and re.search(r"^AUDITED = .*\bsilhouette\.o\b", mk, flags=re.M)
    assert "sil_(f32|bf16)_kernel" in mk


def _points(m=40, d=5, k=4, seed=3):
    rs = np.random.RandomState(seed)
    assign = rs.randint(0, k, size=m)
    X = rs.randn(m, d) + 2.0 * assign[:, None]
    return X, assign


def _same(got, want, rel=1e-12):
    for key in ("sil", "a", "b"):
        assert np.allclose(got[key], want[key], rtol=rel, atol=1e-12), key
    assert np.array_equal(np.asarray(got["nearest"]), want["nearest"])
    assert got["mean"] == pytest.approx(want["mean"], rel=rel, abs=1e-12)


def test_float64_references_against_the_double_loop(nsil):
    X, assign = _points()
    want = sr.brute_force(X, assign, 4)
    assert -1.0 <= want["sil"].min() and want["sil"].max() <= 1.0 and 0.0 < want["mean"] < 1.0
    _same(sr.float64_ref(X, assign, 4), want)
    _same(nsil.host_silhouette(X, assign, k=4), want)
    _same(nsil.host_silhouette(X, assign, k=4, block=7), want)  # ragged row blocks
    assert nsil.host_silhouette(X, assign)["mean"] == pytest.approx(want["mean"], rel=1e-12)  # k = max(assign) + 1
    rows = np.array([39, 0, 17, 17, 5])
    part = nsil.host_silhouette(X, assign, k=4, rows=rows)
    for key in ("sil", "a", "b", "nearest"):
        assert np.allclose(part[key], np.asarray(want[key])[rows], rtol=1e-12, atol=1e-12)
    assert part["mean"] == pytest.approx(float(want["sil"][rows].sum() / 5), rel=1e-12)
    _same(sr.float64_ref(X, assign, 4, rows=rows), dict(sil=want["sil"][rows], a=want["a"][rows], b=want["b"][rows], nearest=want["nearest"][rows],
                                                         mean=float(want["sil"][rows].sum() / 5)))


def test_singleton_and_empty_clusters(nsil):
    X, assign = _points(m=30, k=3)
    assign = assign * 2        # clusters 0, 2, 4 of k = 7: 1, 3, 5, 6 are empty
    assign[11] = 5             # and a singleton
    want = sr.brute_force(X, assign, 7)
    assert want["sil"][11] == 0.0 and want["a"][11] == 0.0 and want["b"][11] > 0.0 and want["nearest"][11] in (0, 2, 4)
    assert set(want["nearest"].tolist()) <= {0, 2, 4, 5}
    for got in (sr.float64_ref(X, assign, 7), nsil.host_silhouette(X, assign, k=7)):
        _same(got, want)
        assert got["sil"][11] == 0.0 and got["a"][11] == 0.0
    same = np.zeros((6, 3))    # every distance 0: max(a, b) = 0 -> sil = 0
    got = nsil.host_silhouette(same, [0, 0, 0, 1, 1, 1], k=2)
    assert not got["sil"].any() and got["mean"] == 0.0 and not sr.float64_ref(same, [0, 0, 0, 1, 1, 1], 2)["sil"].any()
    for bad, text in ((dict(assign=[0, 0, 0, 0, 0, 0], k=2), "non-empty"), (dict(assign=[0, 1, 2, 0, 1, 2], k=2), "assign outside"),
                      (dict(assign=[0, 1, 0, 1, 0, 1], k=2, rows=[6]), "rows outside"), (dict(assign=[0, 1], k=2), "one cluster per row")):
        with pytest.raises(ValueError, match=text):
            nsil.host_silhouette(same, bad.pop("assign"), **bad)


def test_ties_go_to_the_lowest_cluster(nsil):
    t = np.array([20] * 4 + [30] * 3 + [40] * 4)
    X = sr.exact_table(t, 8, 2)
    for assign, near_mid in (([0] * 4 + [1] * 3 + [2] * 4, 0), ([1] * 4 + [0] * 3 + [2] * 4, 1), ([2] * 4 + [0] * 3 + [1] * 4, 1)):
        assign = np.array(assign)
        mid = np.arange(4, 7)
        for got in (sr.brute_force(X, assign, 3), sr.float64_ref(X, assign, 3), nsil.host_silhouette(X, assign, k=3),
                    sr.fp32_closed_form(t, 2, assign, 3)):
            assert np.all(np.asarray(got["nearest"])[mid] == near_mid), (assign, got["nearest"])
            assert np.all(np.asarray(got["b"])[mid] == 20.0) and np.all(np.asarray(got["a"])[mid] == 0.0) and np.all(np.asarray(got["sil"])[mid] == 1.0)


def test_fp32_closed_form_is_the_definition_on_exact_tables():
    rs = np.random.RandomState(8)
    t, assign = rs.randint(0, 64, size=90), rs.randint(0, 5, size=90)
    for d, q in ((8, 2), (50, 4), (128, 1)):
        X = sr.exact_table(t, d, q)
        assert np.array_equal(sr.float64_ref(X, assign, 5)["dist"], q * np.abs(t[:, None] - t[None, :]).astype(np.float64))
        assert np.array_equal(sr.round_bf16(X), X)
        got, want = sr.fp32_closed_form(t, q, assign, 5), sr.float64_ref(X, assign, 5)
        assert np.array_equal(got["nearest"], want["nearest"])
        for key in ("a", "b"):  # one rounding each; sil = (b - a) / max: the roundings of a, b, b - a and the division, absolute
            assert got[key].dtype == np.float32 and np.allclose(got[key], want[key], rtol=sr.U, atol=0)
        assert got["sil"].dtype == np.float32 and np.allclose(got["sil"], want["sil"], rtol=0, atol=4 * sr.U)
    # round to nearest, ties to even: 1 + 2^-8 and 1 + 3 2^-8 are halfway between neighbours
    assert np.array_equal(sr.round_bf16(np.array([1.0, 1.00390625, 1.01171875, 1.005], dtype=np.float32)),
                          np.array([1.0, 1.0, 1.015625, 1.0078125], dtype=np.float32))


# ---- the evaluator and graph_gan.evaluation()
def test_evaluator_on_blobs_and_the_results_line(nsil):
    from tests.support import kmeans_ref as kr
    X, labels, _ = kr.blobs(5, 16, 60)
    X = X.astype(np.float64)
    n = len(X)
    nodes = np.arange(n)
    ev = nsil.NodeSilhouetteEval(n, 16, emd=X)
    res = ev.eval_node_silhouette(nodes, labels, labels, 5)
    want = sr.float64_ref(X, labels, 5)["mean"]
    assert res["sil"] == pytest.approx(want, rel=1e-12) and res["label_sil"] == res["sil"] and res["sil"] > 0.5
    assert (res["k"], res["n"], res["rows"], res["precision"]) == (5, n, n, "float64")
    line = nsil.format_results("gen", res)
    assert line == "gen_sil:sil=%s label_sil=%s k=5 n=%d rows=%d precision=float64\n" % (str(res["sil"]), str(res["label_sil"]), n, n)
    assert re.fullmatch(r"gen_sil:sil=\S+ label_sil=\S+ k=\d+ n=\d+ rows=\d+ precision=\S+\n", line)
    shuffled = np.random.RandomState(1).permutation(labels)
    res2 = ev.eval_node_silhouette(nodes, shuffled, labels, 5)
    assert res2["sil"] == res["sil"] and res2["label_sil"] < 0.05 < res["sil"]
    # a sample: the stated draw, every sampled row against all columns
    sub = nsil.NodeSilhouetteEval(n, 16, emd=X, max_rows=50, seed=9).eval_node_silhouette(nodes, labels, labels, 5)
    rows = np.sort(np.random.RandomState([9, 0x5349]).choice(n, size=50, replace=False))
    assert np.array_equal(nsil.sample_positions(n, 50, 9), rows) and nsil.sample_positions(n, 0, 9) is None and nsil.sample_positions(n, n, 9) is None
    assert sub["rows"] == 50 and sub["sil"] == pytest.approx(sr.float64_ref(X, labels, 5, rows=rows)["mean"], rel=1e-12)
    # one non-empty cluster: no silhouette
    one = ev.eval_node_silhouette(nodes, np.zeros(n, dtype=np.int64), labels, 5)
    assert np.isnan(one["label_sil"]) and one["sil"] == res["sil"]
    for bad in (dict(max_rows=-1), dict(max_rows=2.5), dict(max_rows=True)):
        with pytest.raises(ValueError, match="node silhouette"):
            nsil.NodeSilhouetteEval(n, 16, emd=X, **bad)
    with pytest.raises(ValueError, match="node silhouette"):
        nsil.NodeSilhouetteEval(n, 16)
    with pytest.raises(ValueError, match="precision"):
        nsil.NodeSilhouetteEval(n, 16, engine=object(), precision="fp16")


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def _labels_for(cfg, n, tmp_path):
    rs = np.random.RandomState(5)
    nodes = np.sort(rs.permutation(n)[:n // 4])
    cfg.labels_filename = str(tmp_path / "labels.txt")
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d\t%d\n" % (v, 10 * int(c)) for v, c in zip(nodes, rs.randint(0, 4, size=len(nodes))))
    return nodes


def test_config_knobs_default_off():
    from graphgan_amd import config
    assert config.engine_cluster_silhouette is False
    assert (config.engine_sil_precision, config.engine_sil_max_rows) == ("fp32", 0)


def test_evaluation_lines_with_and_without_the_knob(nsil, tmp_path):
    from graphgan_amd import utils
    from graphgan_amd.evaluation import node_clustering as ncl
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    assert cfg.engine_cluster_silhouette is False
    nodes = _labels_for(cfg, n, tmp_path)
    cfg.engine_node_clustering, cfg.engine_cluster_n_init, cfg.engine_cluster_max_iters = True, 2, 30
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    want = GraphGAN.evaluation(g)  # the knob's default: off
    del cfg.engine_cluster_silhouette, cfg.engine_sil_precision, cfg.engine_sil_max_rows
    assert GraphGAN.evaluation(g) == want and len(want) == 5  # a user's config without the knobs
    assert open(cfg.result_filename).read() == "".join(want + want) and "_sil" not in "".join(want)
    cfg.engine_cluster_silhouette = True
    lines = GraphGAN.evaluation(g)
    assert len(lines) == 7 and lines[:4] == want[:4] and lines[6] == want[4]
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "gen_cluster", "dis_cluster", "gen_sil", "dis_sil", "gen_nll"]
    for i, (mode, line) in enumerate(zip(cfg.modes, lines[4:6])):
        emd = utils.read_embeddings(cfg.emb_filenames[i], n_node=n, n_embed=cfg.n_emb)
        nce = ncl.NodeClusterEval(cfg.emb_filenames[i], cfg.labels_filename, n, cfg.n_emb, n_init=2, max_iters=30, seed=g.seed)
        nce.eval_node_clustering()
        fit = nce.last_partition
        assert np.array_equal(fit["nodes"], nodes) and fit["k"] == 4
        X = np.asarray(emd, dtype=np.float64)[nodes]
        res = dict(sil=sr.float64_ref(X, fit["assign"], 4)["mean"], label_sil=sr.float64_ref(X, fit["classes"], 4)["mean"], k=4, n=len(nodes),
                   rows=len(nodes), precision="float64")
        m = re.fullmatch(r"%s_sil:sil=(\S+) label_sil=(\S+) k=4 n=%d rows=%d precision=float64\n" % (mode, len(nodes), len(nodes)), line)
        assert m, line
        assert float(m.group(1)) == pytest.approx(res["sil"], rel=1e-9) and float(m.group(2)) == pytest.approx(res["label_sil"], rel=1e-9)
        assert -1.0 <= float(m.group(2)) < float(m.group(1)) <= 1.0  # k-means' own partition beats random labels
    assert open(cfg.result_filename).read() == "".join(want + want + lines)
    cfg.engine_sil_max_rows = 100
    assert " rows=100 " in GraphGAN.evaluation(g)[4]


def test_the_silhouette_knob_needs_the_clustering_knob(tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_node_clustering
    cfg, g, _ = _layout(tmp_path)
    cfg.engine_cluster_silhouette = True
    with pytest.raises(ValueError, match="engine_cluster_silhouette needs engine_node_clustering"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
    with pytest.raises(ValueError, match="engine_node_clustering"):
        _check_node_clustering(types.SimpleNamespace(engine_cluster_silhouette=True))
    cfg.engine_node_clustering = True
    cfg.labels_filename = str(tmp_path / "no_such_labels.txt")
    with pytest.raises(ValueError, match="labels_filename"):
        GraphGAN.evaluation(g)
    _check_node_clustering(types.SimpleNamespace())  # knobs absent: nothing to check
