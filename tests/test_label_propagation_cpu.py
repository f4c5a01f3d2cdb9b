"""The host side of the label-spreading baseline (graphgan_amd/evaluation/label_propagation.py, graph_gan.py's
engine_nc_graph_baseline, the ``python -m graphgan_amd.propagate`` command line) -- the coefficients, the float64 recursion against a
dense restatement, scikit-learn's LabelSpreading and the closed form, the prediction rules, the results line, its place and its
cache, the refusals -- and the C ABI's declaration of gg_neighbor_sum / gg_label_spread."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests.support import label_spread_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lp():
    from graphgan_amd.evaluation import label_propagation
    return label_propagation


@pytest.fixture(scope="module")
def lh():
    from graphgan_amd.evaluation import link_heuristics
    return link_heuristics


def test_header_declares_and_library_exports_the_two_symbols():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {"gg_neighbor_sum": ["gg_ctx*", "constfloat*", "int32_t", "constfloat*", "constfloat*", "constint32_t*", "int64_t", "float*", "double*"],
            "gg_label_spread": ["gg_ctx*", "constint32_t*", "constuint32_t*", "int64_t", "int32_t", "double", "int32_t", "constfloat*", "constfloat*",
                                "constint32_t*", "int64_t", "float*", "float*", "double*"]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name) and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["gg_label_spread"][1][5] is ctypes.c_double
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "neighbour-sum sweep" in open(_lib.HEADER_PATH).read()


def test_chunk_length_and_audit_are_in_step_with_the_source():
    from graphgan_amd import _lib
    from graphgan_amd.engine import Engine
    src = open(os.path.join(ROOT, "graphgan_amd", "csrc", "graph_prop.hip")).read()
    m = re.search(r"constexpr int GP_CHUNK = (\d+);", src)
    assert m and int(m.group(1)) == _lib.NEIGHBOR_SUM_CHUNK == Engine.NEIGHBOR_SUM_CHUNK == ref.CHUNK
    m = re.search(r"constexpr int GP_MAX_COL = (\d+);", src)
    assert m and int(m.group(1)) == _lib.NEIGHBOR_SUM_MAX_COL == 128
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    assert re.search(r"^graph_prop\.o: AUDIT = 'gp_\[a-z0-9_\]\*kernel' 16 ", mk, flags=re.M)  # 12 sweeps, 2 hub reducers, Y0, row gather
    assert re.search(r"^AUDITED = .*\bgraph_prop\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\bgraph_prop\.o\b", mk, flags=re.M)
    assert len(re.findall(r"gp_sweep_kernel<(\d+), EPI>", src)) == 6  # ONE sweep kernel, six widths, the epilogue a template argument
    assert "fmaf" not in src and "atomicAdd" not in src  # no fused multiply-add, no floating-point atomics


def test_spread_coefficients_against_float64(lp):
    deg = np.array([0, 1, 2, 3, 4, 7, 100, 5157])
    for alpha in (0.9, 0.5, 0.123):
        s, a, b = lp.spread_coefficients(deg, alpha)
        assert s.dtype == np.float32 and a.dtype == np.float32 and isinstance(b, np.float32)
        assert s[0] == 0 and a[0] == 0 and s[1] == 1 and s[4] == 0.5 and a[1] == np.float32(alpha)
        d = deg[1:].astype(np.float64)
        assert np.array_equal(s[1:], (1.0 / np.sqrt(d)).astype(np.float32)) and np.array_equal(a[1:], (alpha / np.sqrt(d)).astype(np.float32))
        assert np.max(np.abs(s[1:] * np.sqrt(d) - 1.0)) <= 2.0 ** -24 and np.max(np.abs(a[1:] * np.sqrt(d) / alpha - 1.0)) <= 2.0 ** -24
        assert b == np.float32(1.0 - alpha) and abs(float(b) - (1.0 - alpha)) <= 2.0 ** -25
        rs, ra, rb = ref.coefficients(deg, alpha)
        assert np.array_equal(s, rs) and np.array_equal(a, ra) and b == rb
    assert lp.spread_coefficients(deg, 0.9)[2] != np.float32(1) - np.float32(0.9)  # (rounded once from float64, not an fp32 subtraction)


def _multigraph(seed, n=60, e=260):
    """random edges with duplicates (both orientations) and self-loops; nodes n - 3 .. n - 1 stay isolated"""
    rs = np.random.RandomState(seed)
    edges = rs.randint(0, n - 3, size=(e, 2))
    edges = np.concatenate([edges, edges[:40], edges[40:80, ::-1], np.repeat(np.arange(0, 20, 2), 2).reshape(-1, 2)])
    return n, edges[rs.permutation(len(edges))]


def test_host_recursion_equals_the_dense_restatement(lp, lh):
    n, edges = _multigraph(1)
    rs = np.random.RandomState(2)
    ptr, adj = lh.set_adjacency(edges, n)
    src, dst = ref.pair_set(n, edges)
    assert np.array_equal(np.diff(ptr), ref.degrees(n, src)) and np.array_equal(adj, dst) and np.all(np.diff(ptr)[-3:] == 0)
    A, aAs, b = ref.dense_S(n, src, dst, 0.8)
    assert np.array_equal(A, A.T) and not np.diag(A).any() and A.max() == 1.0  # a set: duplicates and self-loops do not count
    train = np.sort(rs.permutation(n)[:15])
    for labels, Y in ((rs.randint(0, 4, 15), None), (None, rs.random_sample((15, 4)) < 0.4)):
        if Y is None:
            Y = np.zeros((15, 4), bool)
            Y[np.arange(15), labels] = True
        else:
            labels = Y
        Y0 = ref.one_hot(n, train, Y)
        F = Y0.copy()
        for T in range(1, 6):
            prev, F = F, aAs @ F + b * Y0
            got = lp.host_label_spread(ptr, adj, train, labels, 4, alpha=0.8, iters=T)
            assert got["F"].dtype == np.float64 and np.max(np.abs(got["F"] - F)) <= 1e-14, T
            assert abs(got["delta"] - np.max(np.abs(F - prev))) <= 1e-14
        sub = np.array([5, 59, 5, 0])
        assert np.array_equal(lp.host_label_spread(ptr, adj, train, labels, 4, alpha=0.8, iters=5, out_nodes=sub)["F"], got["F"][sub])
        assert not got["F"][-3:].any()  # isolated and unlabelled: nothing arrives
    X = rs.standard_normal((n, 3))
    assert np.max(np.abs(lp.host_neighbor_sum(ptr, adj, X) - A @ X)) <= 1e-13
    assert np.array_equal(lp.host_neighbor_sum(ptr, adj, np.ones((n, 1), np.int64))[:, 0], np.diff(ptr))


@pytest.mark.parametrize("seed", (0, 1))
def test_scikit_learn_label_spreading_on_the_planted_partition(lp, lh, seed):
    sk = pytest.importorskip("sklearn.semi_supervised")
    n = 256
    edges, lab, train, test = ref.planted_partition(seed)
    src, dst = ref.pair_set(n, edges)
    A = ref.dense_S(n, src, dst, 0.9)[0]
    y = np.full(n, -1)
    y[train] = lab[train]
    model = sk.LabelSpreading(kernel=lambda X, Z: A, alpha=0.9, max_iter=30, tol=0.0)
    model.fit(np.zeros((n, 1)), y)
    ptr, adj = lh.set_adjacency(edges, n)
    Y = np.zeros((len(train), 4), bool)
    Y[np.arange(len(train)), lab[train]] = True
    F = lp.host_label_spread(ptr, adj, train, lab[train], 4, alpha=0.9, iters=30)["F"]
    assert F.sum(axis=1).min() > 0  # (every node is reached: the rows can be normalised)
    diff = np.max(np.abs(F / F.sum(axis=1, keepdims=True) - model.label_distributions_))
    print("largest difference to scikit-learn: %.3e" % diff)
    assert diff <= 1e-6
    pred, unreached = lp.predict(F, Y)
    assert unreached == 0 and np.array_equal(pred, model.transduction_)
    assert np.mean(pred[test] == lab[test]) > 0.9


def test_closed_form(lp, lh):
    """F_T -> (1 - alpha) (I - alpha S)^-1 Y0; at alpha = 0.5 the remainder (alpha S)^T is below 2^-60 after 60 iterations"""
    n = 256
    edges, lab, train, _ = ref.planted_partition(0)
    src, dst = ref.pair_set(n, edges)
    _, aAs, b = ref.dense_S(n, src, dst, 0.5)
    Y = np.zeros((len(train), 4), bool)
    Y[np.arange(len(train)), lab[train]] = True
    want = b * np.linalg.solve(np.eye(n) - aAs, ref.one_hot(n, train, Y))
    ptr, adj = lh.set_adjacency(edges, n)
    got = lp.host_label_spread(ptr, adj, train, lab[train], 4, alpha=0.5, iters=60)
    assert np.max(np.abs(got["F"] - want)) <= 1e-13 and got["delta"] <= 2.0 ** -58


def test_prediction_rules(lp, lh):
    Y = np.array([[1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]], bool)  # frequencies 1, 2, 2: the fallback is class 1
    F = np.array([[0.2, 0.5, 0.5], [0.3, 0.3, 0.1], [0.0, 0.0, 0.0], [0.0, 0.0, 1e-30], [0.7, 0.1, 0.7]])
    pred, unreached = lp.predict(F, Y)
    assert pred.tolist() == [1, 0, 1, 2, 0] and unreached == 1 and pred.dtype == np.int64  # ties to the lowest class; the all-zero row
    assert lp.predict(F.astype(np.float32), Y)[0].tolist() == [1, 0, 1, 2, 0]
    # multi-label top-k: the k_i largest, ties to the lower class; the all-zero row takes the k_i most frequent training labels
    ml, unreached = lp.predict(F, Y, k=[2, 1, 2, 3, 1])
    assert unreached == 1 and ml.dtype == np.bool_
    assert ml.tolist() == [[False, True, True], [True, False, False], [False, True, True], [True, True, True], [True, False, False]]
    assert lp.predict(F, Y, k=[0] * 5)[0].sum() == 0
    # a second component without a training label, end to end on the host
    edges = np.array([(i, (i + 1) % 30) for i in range(30)] + [(30 + i, 30 + (i + 1) % 30) for i in range(30)])
    ptr, adj = lh.set_adjacency(edges, 60)
    res = lp.host_label_spread(ptr, adj, [0, 5, 10, 15, 20], [2, 1, 2, 1, 0], 3, iters=40, out_nodes=[3, 29, 31, 45, 59])
    pred, unreached = lp.predict(res["F"], lp.label_matrix("t", [2, 1, 2, 1, 0], 5, 3))
    assert unreached == 3 and pred[2:].tolist() == [1, 1, 1] and not res["F"][2:].any() and res["F"][:2].all()


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def _write_labels(cfg, n, multilabel=False):
    """labels for 300 nodes of the fixture: the node id's residue (and, multi-label, a second label for every third node)"""
    cfg.labels_filename = os.path.join(os.path.dirname(cfg.result_filename), "labels.txt")
    nodes = np.random.RandomState(5).permutation(n)[:300]
    with open(cfg.labels_filename, "w") as f:
        for v in nodes.tolist():
            f.write("%d %d%s\n" % (v, v % 5, " %d" % (5 + v % 2) if multilabel and v % 3 == 0 else ""))


def test_config_knob_defaults():
    from graphgan_amd import config
    assert config.engine_nc_graph_baseline is False and config.engine_lsp_alpha == 0.9 and config.engine_lsp_iters == 30


def test_evaluation_lines_with_and_without_the_knob(lp, tmp_path, monkeypatch):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    _write_labels(cfg, n)
    assert cfg.engine_nc_graph_baseline is False
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    cfg.engine_lp_heuristics = True
    want = GraphGAN.evaluation(g)  # the knob's default: off
    del cfg.engine_nc_graph_baseline
    assert GraphGAN.evaluation(g) == want and [ln.split(":")[0] for ln in want] == ["gen", "dis", "graph_lp", "gen_nll"]  # a config without the knob
    assert open(cfg.result_filename).read() == "".join(want + want) and "graph_nc" not in "".join(want)
    cfg.engine_nc_graph_baseline, cfg.engine_lsp_alpha, cfg.engine_lsp_iters = True, 0.8, 12
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_lp", "graph_nc", "gen_nll"]  # after graph_lp, before gen_nll
    assert lines[:3] == want[:3] and lines[4] == want[3]
    direct = lp.LabelSpreadEval(cfg.train_filename, cfg.labels_filename, n, train_ratio=0.9, seed=0, alpha=0.8, iters=12).eval_label_spread()
    assert lines[3] == lp.format_results(direct)
    assert re.fullmatch(r"graph_nc:acc=\S+ macro_f1=\S+ alpha=0\.8 iters=12 delta=\S+ unreached=\d+ n_train=270 n_test=30\n", lines[3])
    assert lines[3] == "graph_nc:" + " ".join("%s=%s" % (k, str(direct[k])) for k in
                                              ("acc", "macro_f1", "alpha", "iters", "delta", "unreached", "n_train", "n_test")) + "\n"
    assert 0.0 <= direct["acc"] <= 1.0 and direct["delta"] > 0
    # the second evaluation repeats the cached string: nothing is computed again
    monkeypatch.setattr(lp.LabelSpreadEval, "eval_label_spread", lambda self: pytest.fail("the line was computed twice"))
    assert GraphGAN.evaluation(g) == lines and g._graph_nc_line == lines[3]
    assert open(cfg.result_filename).read() == "".join(want + want + lines + lines)


def test_multilabel_line(lp, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN
    from graphgan_amd.evaluation import node_classification as nc
    cfg, g, n = _layout(tmp_path)
    _write_labels(cfg, n, multilabel=True)
    cfg.engine_nc_graph_baseline, cfg.engine_nc_multilabel = True, True
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_nc"]
    assert re.fullmatch(r"graph_nc:acc=\S+ micro_f1=\S+ macro_f1=\S+ alpha=0\.9 iters=30 delta=\S+ unreached=\d+ n_train=270 n_test=30\n", lines[2])
    ev = lp.LabelSpreadEval(cfg.train_filename, cfg.labels_filename, n, multilabel=True)
    assert lines[2] == lp.format_results(ev.eval_label_spread(), True)
    # the metrics are ml_metrics of the top-k prediction on the classifier's split
    tr_n, tr_y, te_n, te_y, n_class = ev.split()
    nce = nc.NodeClassifyEval(None, cfg.labels_filename, n, 4, emd=np.zeros((n, 4)), multilabel=True)
    assert np.array_equal(nce.split()[0], tr_n) and np.array_equal(nce.split()[2], te_n) and n_class == 7
    pred, _ = lp.predict(ev.spread(tr_n, tr_y, n_class, te_n)["F"], tr_y, k=te_y.sum(axis=1))
    assert np.array_equal(pred.sum(axis=1), te_y.sum(axis=1))
    assert "micro_f1=%s " % str(nc.ml_metrics(te_y, pred)["micro_f1"]) in lines[2]


def test_refusals_come_before_anything_is_computed(lp, lh, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_nc_graph_baseline
    cfg, g, n = _layout(tmp_path)
    cfg.engine_nc_graph_baseline = True
    cfg.labels_filename = str(tmp_path / "no_such_labels.txt")
    with pytest.raises(ValueError, match="engine_nc_graph_baseline needs labels: config.labels_filename does not exist"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    with pytest.raises(ValueError, match="labels_filename"):
        _check_nc_graph_baseline(types.SimpleNamespace(engine_nc_graph_baseline=True))
    _write_labels(cfg, n)
    for alpha in (0.0, 1.0, -0.1, 1.5, "0.9", True):
        cfg.engine_lsp_alpha = alpha
        with pytest.raises(ValueError, match=r"engine_lsp_alpha must lie in \(0, 1\)"):
            _check_nc_graph_baseline(cfg)
    cfg.engine_lsp_alpha = 0.9
    for iters in (0, -3, 2.5, True):
        cfg.engine_lsp_iters = iters
        with pytest.raises(ValueError, match="engine_lsp_iters must be an integer >= 1"):
            _check_nc_graph_baseline(cfg)
    cfg.engine_lsp_iters = 30
    cfg.engine_nc_multilabel, cfg.engine_nc_ml_protocol = True, "threshold"
    with pytest.raises(ValueError, match="'topk' protocol only"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    cfg.engine_nc_ml_protocol = "topk"
    _check_nc_graph_baseline(cfg)
    _check_nc_graph_baseline(types.SimpleNamespace())  # the knob absent: nothing to check
    _check_nc_graph_baseline(types.SimpleNamespace(engine_nc_graph_baseline=False, engine_lsp_alpha=7))
    # the module's own refusals, with the texts of the ABI
    ptr, adj = lh.set_adjacency([[0, 1], [1, 2]], 4)
    hs = lp.host_label_spread
    for call, text in ((lambda: hs(ptr, adj, [0, 4], [0, 1], 2), r"train_nodes\[1\] = 4 out of range \[0, 4\)"),
                       (lambda: hs(ptr, adj, [0, 1, 0], [0, 1, 1], 2), r"train_nodes\[2\] = 0 repeats train_nodes\[0\]"),
                       (lambda: hs(ptr, adj, [0, 1], [0, 2], 2), r"label_bits row 1 has a bit set at a position >= n_class = 2"),
                       (lambda: hs(ptr, adj, [0, 1], [[0], [1, 2]], 2), r"label_bits row 1 has a bit set at a position >= n_class = 2"),
                       (lambda: hs(ptr, adj, [0, 1], [0, 1], 2, alpha=1.0), r"alpha = 1.0 outside \(0, 1\)"),
                       (lambda: hs(ptr, adj, [0, 1], [0, 1], 2, iters=0), r"iters = 0 is below 1"),
                       (lambda: hs(ptr, adj, [0, 1], [0, 1], 129), r"n_class = 129 outside \[1, 128\]"),
                       (lambda: hs(ptr, adj, [0, 1], [0, 1], 0), r"n_class = 0 outside \[1, 128\]"),
                       (lambda: hs(ptr, adj, [0, 1], [0, 1], 2, out_nodes=[-1]), r"out_nodes\[0\] = -1 out of range \[0, 4\)"),
                       (lambda: hs(ptr, adj, [0, 1], np.zeros((2, 3), bool), 2), r"labels must be"),
                       (lambda: lp.LabelSpreadEval("t", "l", 4, alpha=2.0), r"alpha = 2.0 outside \(0, 1\)")):
        with pytest.raises(ValueError, match=text):
            call()


def test_command_line_on_the_host(lp, lh, tmp_path):
    from graphgan_amd import propagate
    n = 256
    edges, lab, train, test = ref.planted_partition(0)
    tfile, lfile, out = (str(tmp_path / x) for x in ("train.txt", "labels.txt", "pred.tsv"))
    np.savetxt(tfile, edges, fmt="%d")
    with open(lfile, "w") as f:
        f.write("".join("%d %d\n" % (v, 100 + 10 * lab[v]) for v in train.tolist()) + "257 100\n")  # (a labelled node behind the graph's ids)
    assert propagate.main(["--train", tfile, "--labels", lfile, "--out", out, "--host", "--alpha", "0.8", "--iters", "20"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert [int(r[0]) for r in rows] == test.tolist() + [256] and all(len(r) == 3 for r in rows)  # every unlabelled node, 256 isolated
    ptr, adj = lh.set_adjacency(edges, 258)
    tr = np.concatenate([train, [257]])
    F = lp.host_label_spread(ptr, adj, tr, np.concatenate([lab[train], [0]]), 4, alpha=0.8, iters=20, out_nodes=test)["F"]
    assert [int(r[1]) for r in rows[:-1]] == (100 + 10 * np.argmax(F, axis=1)).tolist()
    assert [float(r[2]) for r in rows[:-1]] == F.max(axis=1).tolist()
    freq = np.bincount(np.concatenate([lab[train], [0]]), minlength=4)
    assert rows[-1] == ["256", str(100 + 10 * int(np.argmax(freq))), "0.0"]  # unreached: the most frequent label, score 0
    assert np.mean(np.array([int(r[1]) for r in rows[:-1]]) == 100 + 10 * lab[test]) > 0.9
    # multi-label: k = the mean label count rounded half up, the labels in the order of their scores
    with open(lfile, "w") as f:
        f.write("".join("%d %d %d\n" % (v, lab[v], 4 + lab[v] % 2) for v in train.tolist()))
    assert propagate.main(["--train", tfile, "--labels", lfile, "--out", out, "--host", "--multilabel"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert len(rows) == len(test) and all(len(r[1].split()) == 2 for r in rows)
    for bad in (["--alpha", "1.0"], ["--iters", "0"]):
        with pytest.raises(SystemExit):
            propagate.main(["--train", tfile, "--labels", lfile, "--out", out, "--host"] + bad)
    with pytest.raises(SystemExit):
        propagate.main(["--train", tfile, "--out", out, "--host"])
