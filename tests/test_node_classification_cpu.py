"""Node classification without a GPU: the ABI's three symbols, utils.read_labels, the split, the metrics against sklearn, the
objective against sklearn's LogisticRegression, the evaluator's host fallback, and the build audit of classifier.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.support import classifier_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphgan_amd", "csrc")
NAMES = ("gg_classifier_lossgrad", "gg_classifier_fit", "gg_classifier_predict")


def test_symbols_are_declared_bound_and_exported():
    from graphgan_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M | re.S)
        assert m, name
        n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert getattr(raw, name) is not None
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.header_abi_version() == _lib.ABI_VERSION == 9  # additive symbols: the number stays
    for limit in ("2 <= n_class <= 128", "ties to the LOWEST class", "same bits"):
        assert limit in header


def test_engine_methods_exist():
    from graphgan_amd.engine import Engine
    for name in ("classifier_lossgrad", "classifier_fit", "classifier_predict"):
        assert callable(getattr(Engine, name))


def test_read_labels_remaps_arbitrary_values(tmp_path):
    from graphgan_amd import utils
    p = tmp_path / "labels.txt"
    p.write_text("7 100\n\n2\t-5\n5 42\n   \n0 100\n3 42\n")
    nodes, classes, values = utils.read_labels(str(p), 8)
    assert nodes.dtype == np.int64 and classes.dtype == np.int64
    assert nodes.tolist() == [0, 2, 3, 5, 7]
    assert values.tolist() == [-5, 42, 100]
    assert classes.tolist() == [2, 0, 1, 1, 2]


def test_read_labels_rejects_duplicates_and_bad_ids(tmp_path):
    from graphgan_amd import utils
    p = tmp_path / "dup.txt"
    p.write_text("1 0\n2 1\n1 1\n")
    with pytest.raises(ValueError, match="twice"):
        utils.read_labels(str(p), 4)
    p.write_text("1 0\n4 1\n")
    with pytest.raises(ValueError, match="outside"):
        utils.read_labels(str(p), 4)
    p.write_text("-1 0\n")
    with pytest.raises(ValueError, match="outside"):
        utils.read_labels(str(p), 4)


@pytest.mark.parametrize("L,ratio", [(10, 0.9), (101, 0.9), (7, 0.5), (1000, 0.25)])
def test_split_is_deterministic_disjoint_and_sized(L, ratio):
    from graphgan_amd.evaluation import node_classification as nc
    tr, te = nc.split_nodes(L, ratio, 3)
    tr2, te2 = nc.split_nodes(L, ratio, 3)
    assert np.array_equal(tr, tr2) and np.array_equal(te, te2)
    assert len(tr) == int(np.ceil(ratio * L)) and len(tr) + len(te) == L
    assert sorted(tr.tolist() + te.tolist()) == list(range(L))
    rt, re_ = ref.split(L, ratio, 3)
    assert np.array_equal(tr, rt) and np.array_equal(te, re_)
    if L > 10:
        assert not np.array_equal(tr, nc.split_nodes(L, ratio, 4)[0])


def test_split_raises_on_an_empty_side():
    from graphgan_amd.evaluation import node_classification as nc
    with pytest.raises(ValueError, match="test"):
        nc.split_nodes(5, 1.0, 0)
    with pytest.raises(ValueError, match="training"):
        nc.split_nodes(5, 0.0, 0)


def test_metrics_equal_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    from graphgan_amd.evaluation import node_classification as nc
    rs = np.random.RandomState(5)
    for C, n in ((2, 50), (5, 200), (40, 300), (7, 9)):
        truth = rs.randint(0, C, size=n)
        pred = np.where(rs.rand(n) < 0.6, truth, rs.randint(0, C, size=n))
        if C == 5:
            truth[truth == 3] = 2  # class 3 only ever predicted; class 4 never predicted
            pred[pred == 4] = 0
        acc, f1 = nc.metrics(truth, pred, C)
        labels = sorted(set(truth.tolist()) | set(pred.tolist()))
        assert acc == pytest.approx(skm.accuracy_score(truth, pred), abs=1e-15)
        assert f1 == pytest.approx(skm.f1_score(truth, pred, labels=labels, average="macro", zero_division=0), abs=1e-12)
        racc, rf1 = ref.metrics(truth, pred)
        assert acc == pytest.approx(racc, abs=1e-15) and f1 == pytest.approx(rf1, abs=1e-12)


def test_reference_fit_reaches_the_optimum_of_the_same_objective():
    """pins the objective: sklearn minimises sum_i nll_i + |W|^2 / (2 C_sk), i.e. ours times M with C_sk = 1 / (l2 M)"""
    lm = pytest.importorskip("sklearn.linear_model")
    M, d, C, l2 = 600, 8, 5, 1e-2
    table, nodes, y = ref.planted(M, d, C, 1000, 11)
    X = table[nodes].astype(np.float64)
    W, b, losses = ref.fit(X, y, C, 2000, 0.05, l2)
    ours = float(ref.lossgrad(X, y, W, b, l2)[0])
    clf = lm.LogisticRegression(C=1.0 / (l2 * M), solver="lbfgs", tol=1e-10, max_iter=10000).fit(X, y)
    theirs = float(ref.lossgrad(X, y, clf.coef_, clf.intercept_, l2)[0])
    assert abs(ours - theirs) <= 1e-3, (ours, theirs)
    assert ours >= theirs - 1e-6  # (theirs is the minimum)
    assert losses[0] == pytest.approx(np.log(C), abs=1e-12)


def test_host_fallback_matches_the_reference_lossgrad_and_fit():
    from graphgan_amd.evaluation import node_classification as nc
    table, nodes, y = ref.planted(300, 12, 4, 500, 2)
    X = table[nodes].astype(np.float64)
    rs = np.random.RandomState(0)
    W, b = 0.1 * rs.randn(4, 12), 0.1 * rs.randn(4)
    for got, want in zip(nc.host_lossgrad(X, y, W, b, 1e-3), ref.lossgrad(X, y, W, b, 1e-3)):
        assert np.allclose(got, want, rtol=0, atol=1e-12)
    for got, want in zip(nc.host_fit(X, y, 4, 30, 0.05, 1e-4), ref.fit(X, y, 4, 30, 0.05, 1e-4)):
        assert np.allclose(got, want, rtol=0, atol=1e-10)


def test_evaluator_host_fallback_on_planted_files(tmp_path):
    from graphgan_amd.evaluation import node_classification as nc
    M, d, C, N = 400, 16, 5, 600
    table, nodes, y = ref.planted(M, d, C, N, 7)
    emb, lab = tmp_path / "planted.emb", tmp_path / "labels.txt"
    with open(emb, "w") as f:
        f.write("%d\t%d\n" % (N, d))
        for i in range(N):
            f.write(str(i) + "\t" + "\t".join(repr(float(x)) for x in table[i]) + "\n")
    values = np.array([3, 10, 11, 50, 99])
    lab.write_text("".join("%d %d\n" % (v, values[c]) for v, c in zip(nodes.tolist(), y.tolist())))
    ev = nc.NodeClassifyEval(str(emb), str(lab), N, d, seed=0)
    res = ev.eval_node_classification()
    assert res["acc"] == 1.0 and res["macro_f1"] == 1.0
    assert (res["n_train"], res["n_test"]) == (360, 40)
    assert nc.format_results("gen", res) == "gen:acc=1.0 macro_f1=1.0 n_train=360 n_test=40\n"
    again = nc.NodeClassifyEval(str(emb), str(lab), N, d, emd=table.astype(np.float64), seed=0).eval_node_classification()
    assert again == res


def test_config_has_the_knobs():
    from graphgan_amd import config
    assert config.labels_filename.endswith("/data/" + config.app + "/" + config.dataset + "_labels.txt")
    assert (config.engine_nc_train_ratio, config.engine_nc_iters, config.engine_nc_lr, config.engine_nc_l2) == (0.9, 200, 0.05, 1e-4)


AUDIT = ("nc_[a-z_]*kernel", 35, "node-classification kernels")


def test_scratch_check_accepts_classifier_and_rejects_a_spill(tmp_path):
    remarks = os.path.join(CSRC, "classifier.remarks")
    assert os.path.exists(remarks), "classifier.remarks is written by the build (make -C graphgan_amd/csrc)"
    check = os.path.join(CSRC, "check_no_scratch.sh")
    args = [str(a) for a in AUDIT]
    ok = subprocess.run(["bash", check, remarks] + args, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert "no scratch, no spill" in ok.stdout and AUDIT[2] in ok.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"classifier\.o: AUDIT = '%s' %d '%s'" % (re.escape(AUDIT[0]), AUDIT[1], AUDIT[2]), mk)
    assert re.search(r"^AUDITED = .*\bclassifier\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\bclassifier\.o\b", mk, flags=re.M)
    text = open(remarks).read()
    m = re.search(r"(Function Name: \S*nc_sweep_kernel\S*.*?ScratchSize \[bytes/lane\]: )0", text, flags=re.S)
    assert m
    p = tmp_path / "bad.remarks"
    p.write_text(text[:m.end() - 1] + "832" + text[m.end():])
    res = subprocess.run(["bash", check, str(p)] + args, capture_output=True, text=True)
    assert res.returncode != 0 and "spills" in res.stderr
