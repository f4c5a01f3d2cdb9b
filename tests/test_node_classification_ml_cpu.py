"""Multi-label node classification without a GPU: the ABI's three additive symbols, utils.read_multilabels, the bit packing, the
metrics against sklearn and a hand-computed example, the host fallback against the numpy restatement
tests/support/classifier_ml_ref.py, the evaluator on planted files, the config knobs and the results line."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.support import classifier_ml_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gg_classifier_ml_lossgrad", "gg_classifier_ml_fit", "gg_classifier_ml_predict")


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
    for text in ("softplus(z) = max(z, 0) + log1p(e)", "logit descending, then class ascending", "an exact 0 is not predicted"):
        assert text in header


def test_engine_methods_exist():
    from graphgan_amd.engine import Engine
    for name in ("classifier_ml_lossgrad", "classifier_ml_fit", "classifier_ml_predict"):
        assert callable(getattr(Engine, name))


def test_read_multilabels_unions_lines_and_remaps_values(tmp_path):
    from graphgan_amd import utils
    p = tmp_path / "labels.txt"
    p.write_text("7 100 42\n\n2\t-5\n5 42\n   \n0   100\t-5  7\n7 42\n7 7\n2 -5\n")
    nodes, Y, values = utils.read_multilabels(str(p), 8)
    assert nodes.dtype == np.int64 and Y.dtype == np.bool_ and values.dtype == np.int64
    assert nodes.tolist() == [0, 2, 5, 7]
    assert values.tolist() == [-5, 7, 42, 100]
    assert Y.astype(int).tolist() == [[1, 1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 1, 1]]
    # the single-label reader still refuses the same file
    with pytest.raises(ValueError):
        utils.read_labels(str(p), 8)
    p.write_text("1 0\n2 1\n1 1\n")
    with pytest.raises(ValueError, match="twice"):
        utils.read_labels(str(p), 4)
    nodes, Y, values = utils.read_multilabels(str(p), 4)
    assert nodes.tolist() == [1, 2] and Y.tolist() == [[True, True], [False, True]]


def test_read_multilabels_rejects_bad_input(tmp_path):
    from graphgan_amd import utils
    p = tmp_path / "bad.txt"
    p.write_text("1 0\n4 1\n")
    with pytest.raises(ValueError, match="outside"):
        utils.read_multilabels(str(p), 4)
    p.write_text("-1 0\n")
    with pytest.raises(ValueError, match="outside"):
        utils.read_multilabels(str(p), 4)
    p.write_text("1 0\n2\n")
    with pytest.raises(ValueError, match="node label"):
        utils.read_multilabels(str(p), 4)
    p.write_text("".join("%d %d\n" % (i % 4, i) for i in range(129)))
    with pytest.raises(ValueError, match="128"):
        utils.read_multilabels(str(p), 4)
    p.write_text("".join("%d %d\n" % (i % 4, i) for i in range(128)))
    assert utils.read_multilabels(str(p), 4)[1].shape == (4, 128)


HAND_T = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=bool)
HAND_P = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 1], [0, 0, 0]], dtype=bool)


def test_ml_metrics_hand_example():
    """4 x 3: class 0 TP 2 -> F1 1; class 1 TP 1 FN 1 -> 2/3; class 2 FP 1 -> 0 (present: predicted).  Rows 0 and 3 match."""
    from graphgan_amd.evaluation import node_classification as nc
    for fn in (nc.ml_metrics, ref.ml_metrics):
        got = fn(HAND_T, HAND_P)
        assert got["acc"] == pytest.approx(0.5, abs=1e-15)
        assert got["micro_f1"] == pytest.approx(2 * 3 / (2 * 3 + 1 + 1), abs=1e-15)
        assert got["macro_f1"] == pytest.approx((1.0 + 2.0 / 3.0 + 0.0) / 3.0, abs=1e-15)
    # a class absent from truth and prediction does not count
    T4, P4 = np.pad(HAND_T, ((0, 0), (0, 1))), np.pad(HAND_P, ((0, 0), (0, 1)))
    assert nc.ml_metrics(T4, P4) == nc.ml_metrics(HAND_T, HAND_P)


def test_ml_metrics_equal_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    from graphgan_amd.evaluation import node_classification as nc
    rs = np.random.RandomState(5)
    for C, n in ((2, 50), (5, 200), (40, 300), (7, 9)):
        truth = rs.rand(n, C) < 0.2
        pred = np.where(rs.rand(n, C) < 0.7, truth, rs.rand(n, C) < 0.2)
        if C == 5:
            truth[:, 3] = False  # class 3 only ever predicted
            pred[:, 4] = False   # class 4 never predicted
            truth[:, 1] = pred[:, 1] = False  # class 1 absent
        got = nc.ml_metrics(truth, pred)
        present = np.flatnonzero(truth.any(axis=0) | pred.any(axis=0)).tolist()
        assert got["acc"] == pytest.approx(skm.accuracy_score(truth, pred), abs=1e-15)
        assert got["micro_f1"] == pytest.approx(skm.f1_score(truth, pred, labels=present, average="micro", zero_division=0), abs=1e-12)
        assert got["macro_f1"] == pytest.approx(skm.f1_score(truth, pred, labels=present, average="macro", zero_division=0), abs=1e-12)
        want = ref.ml_metrics(truth, pred)
        for key in ("acc", "micro_f1", "macro_f1"):
            assert got[key] == pytest.approx(want[key], abs=1e-12)


@pytest.mark.parametrize("C", [31, 32, 33, 64, 65, 128])
def test_bit_packing_round_trips(C):
    from graphgan_amd.engine import pack_label_bits, unpack_label_bits
    rs = np.random.RandomState(C)
    Y = rs.rand(37, C) < 0.3
    Y[0], Y[1] = False, True  # no label; every label
    Y[2] = False
    Y[2, [0, C - 1]] = True
    bits = pack_label_bits(Y, C)
    CW = (C + 31) // 32
    assert bits.dtype == np.uint32 and bits.shape == (37, CW) and bits.flags.c_contiguous
    for i in (1, 2, 5):
        for c in range(C):
            assert bool((int(bits[i, c >> 5]) >> (c & 31)) & 1) == bool(Y[i, c])
    if C % 32:
        assert not np.any(bits[:, -1] >> np.uint32(C % 32))  # no bit behind n_class
    assert np.array_equal(unpack_label_bits(bits, C), Y)
    assert np.array_equal(pack_label_bits(Y.astype(np.int64), C), bits)


def test_host_fallback_matches_the_reference():
    from graphgan_amd.evaluation import node_classification as nc
    table, nodes, Y = ref.planted(300, 12, 6, 500, 2)
    X = table[nodes].astype(np.float64)
    rs = np.random.RandomState(0)
    W, b = 0.1 * rs.randn(6, 12), 0.1 * rs.randn(6)
    for got, want in zip(nc.host_ml_lossgrad(X, Y, W, b, 1e-3), ref.lossgrad(X, Y, W, b, 1e-3)):
        assert np.allclose(got, want, rtol=0, atol=1e-12)
    fitted = nc.host_ml_fit(X, Y, 30, 0.05, 1e-4)
    for got, want in zip(fitted, ref.fit(X, Y, 30, 0.05, 1e-4)):
        assert np.allclose(got, want, rtol=0, atol=1e-10)
    assert fitted[2][0] == pytest.approx(6 * np.log(2), abs=1e-12)
    z = ref.logits(X, fitted[0], fitted[1])
    k = Y.sum(axis=1)
    assert np.array_equal(nc.host_ml_predict(X, fitted[0], fitted[1], k), ref.predict_topk(z, k))
    assert np.array_equal(nc.host_ml_predict(X, fitted[0], fitted[1]), ref.predict_threshold(z))
    # ties go to the lower class; an exact 0 is not predicted
    Wt, bt = np.zeros((4, 12)), np.array([1.0, 0.0, 1.0, 0.0])
    assert nc.host_ml_predict(X[:2], Wt, bt, [1, 3]).tolist() == [[True, False, False, False], [True, True, True, False]]
    assert nc.host_ml_predict(X[:1], Wt, bt).tolist() == [[True, False, True, False]]


def test_reference_is_stable_at_saturated_logits():
    """softplus / sigmoid in the stable forms: +-200 gives a finite loss and gradient entries of exactly 0 - y or 1 - y, in
    float32 too, where log(1 + exp(z)) overflows"""
    X = np.zeros((4, 3))
    Y = np.array([[1, 0], [0, 1], [1, 1], [0, 0]], dtype=bool)
    b = np.array([200.0, -200.0])
    for dtype in (np.float64, np.float32):
        loss, gW, gb = ref.lossgrad(X, Y, np.zeros((2, 3)), b, 0.0, dtype)
        assert np.isfinite(loss) and loss == pytest.approx((2 * 200.0 + 2 * 200.0) / 4, rel=1e-6)
        assert gb.tolist() == [0.5, -0.5]
    with np.errstate(over="ignore"):
        assert np.isinf(np.log(np.float32(1) + np.exp(np.float32(200.0))))


def _write_planted(tmp_path, table, nodes, Y, values):
    emb, lab = tmp_path / "planted.emb", tmp_path / "labels.txt"
    with open(emb, "w") as f:
        f.write("%d\t%d\n" % table.shape)
        for i in range(len(table)):
            f.write(str(i) + "\t" + "\t".join(repr(float(x)) for x in table[i]) + "\n")
    with open(lab, "w") as f:  # the first label on a line of its own, the others together: the reader takes the union
        for v, y in zip(nodes.tolist(), Y):
            cs = np.flatnonzero(y)
            f.write("%d %d\n" % (v, values[cs[0]]))
            if len(cs) > 1:
                f.write("%d\t%s\n" % (v, " ".join(str(values[c]) for c in cs[1:])))
    return str(emb), str(lab)


def test_evaluator_host_fallback_recovers_planted_labels(tmp_path):
    from graphgan_amd.evaluation import node_classification as nc
    M, d, C, N = 400, 16, 5, 600
    table, nodes, Y = ref.planted(M, d, C, N, 7)
    emb, lab = _write_planted(tmp_path, table, nodes, Y, np.array([3, 10, 11, 50, 99]))
    ev = nc.NodeClassifyEval(emb, lab, N, d, seed=0, multilabel=True)
    tr_n, tr_y, te_n, te_y, n_class = ev.split()
    single = nc.split_nodes(M, 0.9, 0)  # the SAME split as the single-label evaluator's
    order = np.sort(nodes)
    assert np.array_equal(tr_n, order[single[0]]) and np.array_equal(te_n, order[single[1]]) and n_class == C
    assert np.array_equal(te_y, Y[np.argsort(nodes)][single[1]])
    res = ev.eval_node_classification()
    assert sorted(res) == ["acc", "macro_f1", "micro_f1", "n_test", "n_train"]
    assert res["acc"] >= 0.95 and res["micro_f1"] >= 0.95 and res["macro_f1"] >= 0.95
    assert (res["n_train"], res["n_test"]) == (360, 40)
    again = nc.NodeClassifyEval(emb, lab, N, d, emd=table.astype(np.float64), seed=0, multilabel=True).eval_node_classification()
    assert again == res
    thr = nc.NodeClassifyEval(emb, lab, N, d, emd=table.astype(np.float64), seed=0, multilabel=True, ml_protocol="threshold")
    assert thr.eval_node_classification()["micro_f1"] >= 0.8
    with pytest.raises(ValueError, match="ml_protocol"):
        nc.NodeClassifyEval(emb, lab, N, d, emd=table, multilabel=True, ml_protocol="best")
    with pytest.raises(ValueError, match="twice"):  # without the knob the file is refused as before
        nc.NodeClassifyEval(emb, lab, N, d, emd=table).eval_node_classification()


def test_config_has_the_knobs():
    from graphgan_amd import config
    assert config.engine_nc_multilabel is False
    assert config.engine_nc_ml_protocol == "topk"
    assert (config.engine_nc_train_ratio, config.engine_nc_iters, config.engine_nc_lr, config.engine_nc_l2) == (0.9, 200, 0.05, 1e-4)


def test_format_ml_results_field_order():
    from graphgan_amd.evaluation import node_classification as nc
    res = dict(n_test=40, macro_f1=0.5, acc=1.0, n_train=360, micro_f1=0.25)
    assert nc.format_ml_results("gen", res) == "gen:acc=1.0 micro_f1=0.25 macro_f1=0.5 n_train=360 n_test=40\n"


def test_makefile_audits_the_new_kernels():
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^classifier\.o: AUDIT = ((?:.*\\\n)*.*)", mk, flags=re.M).group(1)
    assert "'nc_[a-z_]*kernel' 35 'node-classification kernels'" in rule
    assert "nc_ml_predict_kernel" in rule and re.search(r"Lb1E' 32 ", rule)
    remarks = os.path.join(ROOT, "graphgan_amd", "csrc", "classifier.remarks")
    assert os.path.exists(remarks), "classifier.remarks is written by the build (make -C graphgan_amd/csrc)"
    names = re.findall(r"Function Name: (\S+)", open(remarks).read())
    assert sum("nc_sweep_kernel" in n and "Lb1E" in n for n in names) == 32
    assert sum("nc_sweep_kernel" in n and "Lb0E" in n for n in names) == 32
    assert sum("nc_ml_predict_kernel" in n for n in names) == 1
