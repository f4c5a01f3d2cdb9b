"""Multi-label node classification on the device (gg_classifier_ml_* / Engine.classifier_ml_*, NodeClassifyEval(multilabel=True),
graph_gan.py's engine_nc_multilabel) against the numpy restatement tests/support/classifier_ml_ref.py.  Tolerances are derived as
in test_gpu_node_classification.py: dev = max |float32 reference - float64 reference| on the test's own inputs, and the device
must lie within max(8 dev, 1e-6) of the float64 reference (classifier_ref.tol)."""
import ctypes

import numpy as np
import pytest

from tests.support import classifier_harness as harness
from tests.support import classifier_ml_ref as ref
from tests.support.classifier_harness import N_TABLE, compare, tables

pytestmark = pytest.mark.gpu

# (M, d, C): the 64-row tile edge (63, 64, 65), the 32-column tiles (d = 8 -> 1, 50 -> 2, 128 -> 4, 256 -> 8), the mask-word
# edges (C = 31, 32, 33, 64, 65, 128); (997, 256, 128) is the one shape HERE whose W is staged in k-chunks (the other chunked
# instances, C > 64 at d > 192 and C > 96 at d > 152, are in test_gpu_classifier_shapes.py)
LOSSGRAD_CASES = [(1, 8, 2), (63, 8, 31), (64, 8, 32), (65, 8, 33), (997, 50, 64), (65, 50, 65), (63, 128, 40), (997, 128, 128),
                  (64, 256, 5), (997, 256, 128)]


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def engine_of():
    yield harness.engine_of
    harness.close_engines()


def random_labels(rs, M, C):
    """0 - 3 labels per row (rows without a label occur), row 1 with every label"""
    Y = np.zeros((M, C), dtype=bool)
    for i, n in enumerate(rs.randint(0, 4, size=M).tolist()):
        Y[i, rs.permutation(C)[:n]] = True
    if M > 2:
        Y[1] = True
        Y[2] = False
    return Y


@pytest.mark.parametrize("M,d,C", LOSSGRAD_CASES)
def test_lossgrad_matches_float64(engine_of, M, d, C):
    eng = engine_of(d)
    rs = np.random.RandomState(M * 1000 + d + C)
    nodes = rs.randint(0, N_TABLE, size=M)
    if M > 2:
        nodes[M // 2] = nodes[0]  # a repeated node id
        nodes[-1] = nodes[0]
    Y = random_labels(rs, M, C)
    W = (0.5 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    l2 = 1e-3
    for which in (0, 1):
        X = tables(d)[which][nodes]
        r64 = ref.lossgrad(X, Y, W, b, l2, np.float64)
        r32 = ref.lossgrad(X, Y, W, b, l2, np.float32)
        got = eng.classifier_ml_lossgrad(nodes, Y, W, b, which=which, l2=l2)
        compare("ml lossgrad (%d, %d, %d) which %d" % (M, d, C, which), ("loss", "gW", "gb"), (got["loss"], got["gW"], got["gb"]), r64, r32)
    # packed masks are taken as they are
    from graphgan_amd.engine import pack_label_bits
    packed = eng.classifier_ml_lossgrad(nodes, pack_label_bits(Y, C), W, b, which=1, l2=l2)
    assert packed["loss"] == got["loss"] and np.array_equal(packed["gW"].view(np.uint32), got["gW"].view(np.uint32))
    r0 = ref.lossgrad(tables(d)[0][nodes], Y, W, b, l2)[1]
    r1 = ref.lossgrad(tables(d)[1][nodes], Y, W, b, l2)[1]
    assert np.max(np.abs(r0 - r1)) > 1e-3  # (the two tables give different gradients: `which` is honoured)


def test_saturated_logits_stay_finite_and_exact(engine_of):
    """b[c] = +-200 with matching and opposing labels: log(1 + exp z) is inf in float32 here; the stable forms give a finite
    loss and gradient entries of exactly 0 - y or 1 - y"""
    M, d, C = 130, 8, 40
    eng = engine_of(d)
    rs = np.random.RandomState(77)
    nodes = rs.randint(0, N_TABLE, size=M)
    Y = random_labels(rs, M, C)
    W = (0.05 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    hot, cold = [0, 7, 33, 39], [1, 8, 32, 38]
    b[hot], b[cold] = 200.0, -200.0
    Y[::2, 0], Y[1::2, 0] = True, False  # both labels under either saturation
    Y[::3, 1], Y[1::3, 1] = True, False
    X = tables(d)[0][nodes]
    r64 = ref.lossgrad(X, Y, W, b, 0.0, np.float64)
    r32 = ref.lossgrad(X, Y, W, b, 0.0, np.float32)
    got = eng.classifier_ml_lossgrad(nodes, Y, W, b, which=0, l2=0.0)
    assert np.isfinite(got["loss"]) and np.all(np.isfinite(got["gW"])) and np.all(np.isfinite(got["gb"]))
    with np.errstate(over="ignore"):
        assert np.isinf(np.log(np.float32(1) + np.exp(np.float32(200.0))))
    compare("ml saturation", ("loss", "gW", "gb"), (got["loss"], got["gW"], got["gb"]), r64, r32)
    # sigmoid is exactly 1 / 0 there: gb[c] is an exact count over M
    for c in hot:
        assert got["gb"][c] == np.float32(np.sum(~Y[:, c])) / np.float32(M), c
    for c in cold:
        assert got["gb"][c] == np.float32(-np.sum(Y[:, c])) / np.float32(M), c


_fits = {}
FIT_CASES = [(997, 8, 5), (1500, 50, 33), (4099, 128, 40)]


@pytest.fixture(scope="module")
def fits():
    """planted data, the two reference fits and the device fit of one shape, made once"""
    def get(M, d, C):
        key = (M, d, C)
        if key not in _fits:
            import graphgan_amd
            table, nodes, Y = ref.planted(M, d, C, M + 1000, 7 * M + d)
            eng = graphgan_amd.Engine(table, table[::-1].copy())
            X = table[nodes]
            r64 = ref.fit(X, Y, 100, 0.05, 1e-4, np.float64)
            r32 = ref.fit(X, Y, 100, 0.05, 1e-4, np.float32)
            got = eng.classifier_ml_fit(nodes, Y, C, which=0, iters=100, lr=0.05, l2=1e-4)
            _fits[key] = dict(table=table, nodes=nodes, Y=Y, eng=eng, r64=r64, r32=r32, got=got)
        return _fits[key]
    yield get
    for f in _fits.values():
        f["eng"].close()
    _fits.clear()


@pytest.mark.parametrize("M,d,C", FIT_CASES)
def test_fit_matches_float64(fits, M, d, C):
    f = fits(M, d, C)
    got = f["got"]
    assert got["loss"].shape == (100,) and got["ms"] > 0
    assert got["loss"][0] == pytest.approx(C * np.log(2), rel=1e-6)  # (zeros: the loss before update 1)
    compare("ml fit (%d, %d, %d)" % (M, d, C), ("W", "b", "loss"), (got["W"], got["b"], got["loss"]), f["r64"], f["r32"])
    assert got["loss"][-1] < 0.5 * got["loss"][0]
    again = f["eng"].classifier_ml_fit(f["nodes"], f["Y"], C, which=0, iters=100, lr=0.05, l2=1e-4)
    for key in ("W", "b", "loss"):
        assert np.array_equal(again[key].view(np.uint32), got[key].view(np.uint32)), key


@pytest.mark.parametrize("M,d,C", FIT_CASES)
def test_predict_matches_float64(fits, M, d, C):
    f = fits(M, d, C)
    eng, nodes, Y = f["eng"], f["nodes"], f["Y"]
    W, b = f["got"]["W"], f["got"]["b"]
    X = f["table"][nodes]
    z64, z32 = ref.logits(X, W, b, np.float64), ref.logits(X, W, b, np.float32)
    t = ref.tol(z32, z64)
    k = Y.sum(axis=1)
    pred, z = eng.classifier_ml_predict(nodes, W, b, which=0, k=k, logits=True)
    assert pred.dtype == np.bool_ and pred.shape == (M, C)
    err = float(np.max(np.abs(z.astype(np.float64) - z64)))
    print("ml predict (%d, %d, %d): logits err %.3g tol %.3g" % (M, d, C, err, t))
    assert err <= t
    # top-k: the rows whose k-th and (k + 1)-th float64 logits are further apart than the tolerance
    clear = ref.topk_gap(z64, k) > t
    assert np.mean(~clear) <= 0.01
    assert np.array_equal(pred[clear], ref.predict_topk(z64, k)[clear])
    assert np.array_equal(pred.sum(axis=1), k)
    assert np.array_equal(eng.classifier_ml_predict(nodes, W, b, which=0, k=k), pred)
    # threshold: the entries whose float64 logit is further from 0 than the tolerance
    thr, z2 = eng.classifier_ml_predict(nodes, W, b, which=0, logits=True)
    assert np.array_equal(z2.view(np.uint32), z.view(np.uint32))
    sure = np.abs(z64) > t
    assert np.mean(~sure) <= 0.01
    assert np.array_equal(thr[sure], ref.predict_threshold(z64)[sure])
    assert np.array_equal(thr, z > 0)  # (on the device's own logits the rule is exact)
    # k = 0: no bits; k = C: all bits
    assert not eng.classifier_ml_predict(nodes[:70], W, b, k=np.zeros(70, dtype=np.int64)).any()
    assert eng.classifier_ml_predict(nodes[:70], W, b, k=np.full(70, C)).all()
    # the planted sets are recovered
    assert np.mean(np.all(pred == Y, axis=1)) >= 0.95


def test_predict_exact_ties_go_to_the_lower_class(engine_of):
    eng = engine_of(50)
    rs = np.random.RandomState(9)
    C, n = 128, 200
    sign = (5.0 * np.sign(tables(50)[0][:n].mean(axis=0))).astype(np.float32)
    for lo, hi in ((1, 3), (5, 70), (64, 127)):
        W = (0.01 * rs.randn(C, 50)).astype(np.float32)
        b = np.zeros(C, dtype=np.float32)
        W[lo] = W[hi] = sign
        b[lo] = b[hi] = 100.0  # the two identical rows come first everywhere
        one, z = eng.classifier_ml_predict(np.arange(n), W, b, k=np.ones(n, dtype=np.int32), logits=True)
        assert np.array_equal(z[:, lo].view(np.uint32), z[:, hi].view(np.uint32))
        want = np.zeros((n, C), dtype=bool)
        want[:, lo] = True
        assert np.array_equal(one, want)
        want[:, hi] = True
        assert np.array_equal(eng.classifier_ml_predict(np.arange(n), W, b, k=np.full(n, 2)), want)
    # all logits exactly 0: the threshold rule predicts nothing, top-k the lowest classes
    W0, b0 = np.zeros((C, 50), dtype=np.float32), np.zeros(C, dtype=np.float32)
    assert not eng.classifier_ml_predict(np.arange(n), W0, b0).any()
    low = eng.classifier_ml_predict(np.arange(n), W0, b0, k=np.full(n, 66))
    assert low[:, :66].all() and not low[:, 66:].any()


def assert_same_front_end(eng, nodes, W, b, which):
    """both prediction kernels on the same (nodes, W, b): the same logit bits, and top-1 is the argmax -> (pred, logits)"""
    pred, z = eng.classifier_predict(nodes, W, b, which=which, logits=True)
    one, z_ml = eng.classifier_ml_predict(nodes, W, b, which=which, k=np.ones(len(nodes), dtype=np.int32), logits=True)
    assert np.array_equal(z.view(np.uint32), z_ml.view(np.uint32))
    want = np.zeros(one.shape, dtype=bool)
    want[np.arange(len(nodes)), pred] = True
    assert np.array_equal(one, want)
    return pred, z


# d: 50 is ld = 52, a padded tail; C: one lane-class, exactly one register per lane, the second register (lane + 64) in use,
# both registers full; M (inside): 1, 5 (the workgroup's second pass has one wavefront working), 4100 (the grid is capped at
# 1024 workgroups x 4 rows: the row-stride loop runs a second time)
@pytest.mark.parametrize("d", [8, 50, 256])
@pytest.mark.parametrize("C", [2, 64, 65, 128])
def test_both_predict_kernels_give_the_same_logit_bits(engine_of, d, C):
    """the two kernels share one front end (W and the row in LDS, the dot product in ascending k, + b): no tolerance"""
    eng = engine_of(d)
    rs = np.random.RandomState(1000 * d + C)
    W = (0.5 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    for M in (1, 5, 4100):
        nodes = rs.randint(0, N_TABLE, size=M)
        for which in ((0, 1) if (d, C) == (50, 65) else (0,)):
            pred, z = assert_same_front_end(eng, nodes, W, b, which)
            assert z.shape == (M, C) and np.all(np.isfinite(z))
            assert np.array_equal(pred, np.argmax(z, axis=1))  # (on the device's own logits the rule is exact: numpy's first maximum)


def test_both_predict_kernels_agree_on_an_exact_tie(engine_of):
    """two equal rows of W with equal biases: the two maximal logits are the same bits in both kernels and both take the lower"""
    eng = engine_of(50)
    rs = np.random.RandomState(9)
    C, n = 128, 200
    sign = (5.0 * np.sign(tables(50)[0][:n].mean(axis=0))).astype(np.float32)
    for lo, hi in ((1, 3), (5, 70), (64, 127)):
        W = (0.01 * rs.randn(C, 50)).astype(np.float32)
        b = np.zeros(C, dtype=np.float32)
        W[lo] = W[hi] = sign
        b[lo] = b[hi] = 100.0  # the two identical rows come first everywhere
        pred, z = assert_same_front_end(eng, np.arange(n), W, b, 0)
        assert np.array_equal(z[:, lo].view(np.uint32), z[:, hi].view(np.uint32))
        assert np.all(z[:, lo] > np.delete(z, [lo, hi], axis=1).max(axis=1))
        assert np.all(pred == lo)


def _write_labels(path, nodes, Y, values):
    with open(path, "w") as f:  # the first label on a line of its own, the others together: the reader takes the union
        for v, y in zip(np.asarray(nodes).tolist(), Y):
            cs = np.flatnonzero(y)
            f.write("%d %d\n" % (v, values[cs[0]]))
            if len(cs) > 1:
                f.write("%d\t%s\n" % (v, " ".join(str(values[c]) for c in cs[1:])))
    return str(path)


@pytest.mark.parametrize("protocol", ["topk", "threshold"])
def test_evaluator_engine_equals_host_fallback(fits, tmp_path, protocol):
    from graphgan_amd.evaluation import node_classification as nc
    M, d, C = FIT_CASES[1]
    f = fits(M, d, C)
    lab = _write_labels(tmp_path / "labels.txt", f["nodes"], f["Y"], 10 * np.arange(C) + 3)
    n = len(f["table"])
    dev_ev = nc.NodeClassifyEval("unused", lab, n, d, engine=f["eng"], which=0, seed=5, iters=100, multilabel=True, ml_protocol=protocol)
    host_ev = nc.NodeClassifyEval("unused", lab, n, d, emd=f["table"].astype(np.float64), seed=5, iters=100, multilabel=True,
                                  ml_protocol=protocol)
    for a, b in zip(dev_ev.split()[:4], host_ev.split()[:4]):
        assert np.array_equal(a, b)
    single = nc.split_nodes(M, 0.9, 5)
    assert np.array_equal(dev_ev.split()[0], np.sort(f["nodes"])[single[0]])  # the same split as the single-label evaluator's
    dev, host = dev_ev.eval_node_classification(), host_ev.eval_node_classification()
    assert dev == host
    assert sorted(dev) == ["acc", "macro_f1", "micro_f1", "n_test", "n_train"]
    if protocol == "topk":
        assert dev["acc"] >= 0.95 and dev["micro_f1"] >= 0.95 and dev["macro_f1"] >= 0.95
    assert (dev["n_train"], dev["n_test"]) == (1350, 150)


def test_graph_gan_multilabel_app_writes_the_result_lines(tmp_path):
    """graph_gan.py with engine_nc_multilabel on the CA-GrQc fixture: one acc / micro_f1 / macro_f1 line per mode whose values
    are those of the host fallback on the engine's tables; with the knob off the same file is refused"""
    from graphgan_amd.evaluation import node_classification as nc
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    d, n, graph = write_reference_layout(base)
    lab = str(tmp_path / "labels.txt")
    rs = np.random.RandomState(1)
    labelled = np.sort(rs.permutation(n)[:800])
    deg = np.array([len(graph.get(int(v), ())) for v in labelled])
    with open(lab, "w") as f:  # degree-derived labels; the nodes of degree >= 6 carry a second one
        for v, dg in zip(labelled.tolist(), deg.tolist()):
            f.write("%d\t%d\n" % (v, min(dg, 4) * 7 - 2))
            if dg >= 6:
                f.write("%d\t%d\n" % (v, 50))
    assert np.sum(deg >= 6) > 20
    cfg = make_cfg(base, app="node_classification", labels_filename=lab, n_epochs=0, engine_nc_iters=60, engine_nc_multilabel=True)
    from graphgan_amd.graph_gan import GraphGAN
    g = GraphGAN(cfg)
    g.train()
    lines = open(cfg.result_filename).read().splitlines()
    assert len(lines) == 2
    for i, (mode, line) in enumerate(zip(("gen", "dis"), lines)):
        host = nc.NodeClassifyEval("unused", lab, g.n_node, cfg.n_emb, emd=g.engine.get_embeddings(i).astype(np.float64),
                                   seed=cfg.engine_seed, iters=60, multilabel=True).eval_node_classification()
        assert line + "\n" == nc.format_ml_results(mode, host)
        fields = line[len(mode) + 1:].split(" ")
        assert [x.split("=")[0] for x in fields] == ["acc", "micro_f1", "macro_f1", "n_train", "n_test"]
        assert (host["n_train"], host["n_test"]) == (720, 80)
    cfg.engine_nc_multilabel = False
    with pytest.raises(ValueError, match="twice"):
        g.evaluation(g)
    g.engine.close()


def test_invalid_arguments_name_the_cause(ga, engine_of):
    from graphgan_amd import _lib
    eng = engine_of(8)
    L = _lib.lib
    nodes = np.arange(10, dtype=np.int32)
    bits = np.zeros((10, 5), dtype=np.uint32)  # (wide enough for 129 classes)
    out = np.zeros(129 * 8 + 200, dtype=np.float32)
    W = np.zeros((129, 8), dtype=np.float32)
    pred = np.zeros((10, 5), dtype=np.uint32)
    k = np.zeros(10, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def lossgrad(which, nodes, bits, C, W=W, loss=out):
        return L.gg_classifier_ml_lossgrad(eng._ctx, which, p(nodes), p(bits), 10, C, p(W), p(W), 0.0, p(loss), p(out), p(out))

    def predict(which, nodes, C, k, pred=pred):
        return L.gg_classifier_ml_predict(eng._ctx, which, p(nodes), 10, C, p(W), p(W), p(k), p(pred), None)

    def last():
        return L.gg_last_error(eng._ctx).decode()

    bits5 = np.zeros((10, 1), dtype=np.uint32)
    assert lossgrad(0, nodes, bits5, 1) == _lib.GG_EINVAL and "n_class = 1 outside [2, 128]" in last()
    assert lossgrad(0, nodes, bits, 129) == _lib.GG_EINVAL and "n_class = 129 outside [2, 128]" in last()
    stray = bits5.copy()
    stray[3, 0] = (1 << 2) | (1 << 6)
    assert lossgrad(0, nodes, stray, 5) == _lib.GG_EINVAL and "row 3" in last() and "bit 6" in last() and "n_class = 5" in last()
    stray33 = np.zeros((10, 2), dtype=np.uint32)
    stray33[9, 1] = 1 << 1
    assert lossgrad(0, nodes, stray33, 33) == _lib.GG_EINVAL and "row 9" in last() and "bit 33" in last()
    stray33[9, 1] = 1  # class 32: legal
    assert lossgrad(0, nodes, stray33, 33) == 0
    n_bad = nodes.copy()
    n_bad[7] = N_TABLE
    assert lossgrad(0, n_bad, bits5, 5) == _lib.GG_EINVAL and "node id %d" % N_TABLE in last()
    assert lossgrad(2, nodes, bits5, 5) == _lib.GG_EINVAL and "which must be 0" in last()
    assert lossgrad(0, nodes, None, 5) == _lib.GG_EINVAL and "label_bits is NULL" in last()
    assert lossgrad(0, None, bits5, 5) == _lib.GG_EINVAL and "nodes is NULL" in last()
    assert lossgrad(0, nodes, bits5, 5, W=None) == _lib.GG_EINVAL and "must not be NULL" in last()
    assert lossgrad(0, nodes, bits5, 5, loss=None) == _lib.GG_EINVAL and "must not be NULL" in last()
    assert L.gg_classifier_ml_fit(eng._ctx, 0, p(n_bad), p(bits5), 10, 5, 3, 0.05, 0.0, p(W), p(W), None, None) == _lib.GG_EINVAL
    assert "gg_classifier_ml_fit" in last() and "node id" in last()
    assert L.gg_classifier_ml_fit(eng._ctx, 0, p(nodes), p(stray), 10, 5, 3, 0.05, 0.0, p(W), p(W), None, None) == _lib.GG_EINVAL
    assert "row 3" in last()
    assert L.gg_classifier_ml_fit(eng._ctx, 0, p(nodes), p(bits5), 10, 5, 3, 0.05, 0.0, None, p(W), None, None) == _lib.GG_EINVAL
    assert "must not be NULL" in last()
    k_bad = k.copy()
    k_bad[4] = 6
    assert predict(0, nodes, 5, k_bad) == _lib.GG_EINVAL and "k = 6" in last() and "row 4" in last()
    k_bad[4] = -1
    assert predict(0, nodes, 5, k_bad) == _lib.GG_EINVAL and "k = -1" in last() and "row 4" in last()
    k_bad[4] = 5  # k = n_class: legal
    assert predict(0, nodes, 5, k_bad) == 0
    assert predict(2, nodes, 5, k) == _lib.GG_EINVAL and "which" in last()
    assert predict(0, nodes, 129, k) == _lib.GG_EINVAL and "n_class = 129" in last()
    assert predict(0, n_bad, 5, None) == _lib.GG_EINVAL and "node id" in last()
    assert predict(0, nodes, 5, None, pred=None) == _lib.GG_EINVAL and "must not be NULL" in last()
    # the Python layer refuses the same before the ABI
    Wok, bok = np.zeros((5, 8), dtype=np.float32), np.zeros(5, dtype=np.float32)
    Y = np.zeros((10, 5), dtype=bool)
    with pytest.raises(ValueError, match="n_class"):
        eng.classifier_ml_fit(nodes, np.zeros((10, 1), dtype=bool), 1)
    with pytest.raises(ValueError, match="n_class"):
        eng.classifier_ml_fit(nodes, np.zeros((10, 129), dtype=bool), 129)
    with pytest.raises(ValueError, match="n_class = 5"):
        eng.classifier_ml_fit(nodes, stray, 5)
    with pytest.raises(ValueError, match="labels must be"):
        eng.classifier_ml_fit(nodes, np.zeros((10, 4), dtype=bool), 5)
    with pytest.raises(ValueError, match="0 and 1"):
        eng.classifier_ml_lossgrad(nodes, 2 * np.ones((10, 5), dtype=np.int64), Wok, bok)
    with pytest.raises(ValueError, match="node id"):
        eng.classifier_ml_lossgrad(n_bad, Y, Wok, bok)
    with pytest.raises(ValueError, match="which"):
        eng.classifier_ml_predict(nodes, Wok, bok, which=2)
    with pytest.raises(ValueError, match="k outside"):
        eng.classifier_ml_predict(nodes, Wok, bok, k=np.full(10, 6))
    with pytest.raises(ValueError, match="k outside"):
        eng.classifier_ml_predict(nodes, Wok, bok, k=np.full(10, -1))
    with pytest.raises(ValueError, match="one per node"):
        eng.classifier_ml_predict(nodes, Wok, bok, k=np.zeros(9, dtype=np.int64))
    # the engine still works
    res = eng.classifier_ml_lossgrad(nodes, Y, Wok, bok)
    assert res["loss"] == pytest.approx(5 * np.log(2), rel=1e-6)
    assert np.array_equal(res["gb"], np.full(5, 0.5, dtype=np.float32))
