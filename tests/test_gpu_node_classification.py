"""Node classification on the device (gg_classifier_* / Engine.classifier_*, NodeClassifyEval, graph_gan.py's app) against the
numpy restatement tests/support/classifier_ref.py.  Tolerances are derived, not fixed: for every compared quantity
dev = max |float32 reference - float64 reference| on the test's own inputs, and the device must lie within max(8 dev, 1e-6)
of the float64 reference (classifier_ref.tol)."""
import os

import numpy as np
import pytest

from tests.support import classifier_harness as harness
from tests.support import classifier_ref as ref
from tests.support.classifier_harness import N_TABLE, compare, tables

pytestmark = pytest.mark.gpu

# (M, d, C): row counts around the 64-row tile, d around the 32-column tiles (8 -> 1, 50 -> 2, 128 -> 4, 256 -> 8), C around the
# 32-class tiles; (997, 256, 128) is the one shape HERE whose W is staged in k-chunks (the other chunked instances, C > 64 at
# d > 192 and C > 96 at d > 152, are in test_gpu_classifier_shapes.py)
LOSSGRAD_CASES = [(1, 8, 2), (63, 8, 5), (64, 8, 40), (65, 8, 128), (997, 8, 2),
                  (1, 50, 40), (63, 50, 128), (64, 50, 2), (65, 50, 5), (997, 50, 40),
                  (1, 128, 128), (63, 128, 2), (64, 128, 5), (65, 128, 40), (997, 128, 40), (997, 128, 128),
                  (1, 256, 5), (63, 256, 40), (64, 256, 128), (65, 256, 2), (997, 256, 128)]


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def engine_of():
    yield harness.engine_of
    harness.close_engines()


@pytest.mark.parametrize("M,d,C", LOSSGRAD_CASES)
def test_lossgrad_matches_float64(engine_of, M, d, C):
    eng = engine_of(d)
    rs = np.random.RandomState(M * 1000 + d + C)
    nodes = rs.randint(0, N_TABLE, size=M)
    if M > 2:
        nodes[M // 2] = nodes[0]  # a repeated node id
        nodes[-1] = nodes[0]
    y = rs.randint(0, C - 1, size=M) if C > 2 else np.zeros(M, dtype=np.int64)  # class C - 1 has no row
    W = (0.5 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    l2 = 1e-3
    for which in (0, 1):
        X = tables(d)[which][nodes]
        r64 = ref.lossgrad(X, y, W, b, l2, np.float64)
        r32 = ref.lossgrad(X, y, W, b, l2, np.float32)
        got = eng.classifier_lossgrad(nodes, y, W, b, which=which, l2=l2)
        compare("lossgrad (%d, %d, %d) which %d" % (M, d, C, which), ("loss", "gW", "gb"), (got["loss"], got["gW"], got["gb"]), r64, r32)
    r0 = ref.lossgrad(tables(d)[0][nodes], y, W, b, l2)[1]
    r1 = ref.lossgrad(tables(d)[1][nodes], y, W, b, l2)[1]
    assert np.max(np.abs(r0 - r1)) > 1e-3  # (the two tables give different gradients: `which` is honoured)


_fits = {}


def planted_fit(eng_of, M, d, C):
    """planted data, the three reference fits and the device fit of one shape, made once"""
    key = (M, d, C)
    if key not in _fits:
        import graphgan_amd
        table, nodes, y = ref.planted(M, d, C, M + 1000, 7 * M + d)
        eng = graphgan_amd.Engine(table, table[::-1].copy())
        X = table[nodes]
        r64 = ref.fit(X, y, C, 100, 0.05, 1e-4, np.float64)
        r32 = ref.fit(X, y, C, 100, 0.05, 1e-4, np.float32)
        got = eng.classifier_fit(nodes, y, C, which=0, iters=100, lr=0.05, l2=1e-4)
        _fits[key] = dict(table=table, nodes=nodes, y=y, eng=eng, r64=r64, r32=r32, got=got)
    return _fits[key]


@pytest.fixture(scope="module")
def fits():
    yield lambda M, d, C: planted_fit(None, M, d, C)
    for f in _fits.values():
        f["eng"].close()
    _fits.clear()


FIT_CASES = [(997, 8, 5), (1500, 50, 7), (4099, 128, 40)]


@pytest.mark.parametrize("M,d,C", FIT_CASES)
def test_fit_matches_float64(fits, M, d, C):
    f = fits(M, d, C)
    got = f["got"]
    assert got["loss"].shape == (100,) and got["ms"] > 0
    assert got["loss"][0] == pytest.approx(np.log(C), abs=1e-5)  # (zeros: the loss before update 1)
    compare("fit (%d, %d, %d)" % (M, d, C), ("W", "b", "loss"), (got["W"], got["b"], got["loss"]), f["r64"], f["r32"])
    assert got["loss"][-1] < 0.5 * got["loss"][0]


@pytest.mark.parametrize("M,d,C", FIT_CASES[:2])
def test_fit_twice_gives_the_same_bits(fits, M, d, C):
    f = fits(M, d, C)
    again = f["eng"].classifier_fit(f["nodes"], f["y"], C, which=0, iters=100, lr=0.05, l2=1e-4)
    for k in ("W", "b", "loss"):
        assert np.array_equal(again[k].view(np.uint32), f["got"][k].view(np.uint32)), k


@pytest.mark.parametrize("M,d,C", FIT_CASES)
def test_predict_matches_float64(fits, M, d, C):
    f = fits(M, d, C)
    W, b = f["got"]["W"], f["got"]["b"]
    rs = np.random.RandomState(3)
    nodes = np.concatenate([f["nodes"][:700], rs.randint(0, len(f["table"]), size=301)])
    X = f["table"][nodes]
    z64, z32 = ref.logits(X, W, b, np.float64), ref.logits(X, W, b, np.float32)
    t = ref.tol(z32, z64)
    pred, z = f["eng"].classifier_predict(nodes, W, b, which=0, logits=True)
    err = float(np.max(np.abs(z.astype(np.float64) - z64)))
    print("predict (%d, %d, %d): logits err %.3g tol %.3g" % (M, d, C, err, t))
    assert err <= t
    top2 = np.sort(z64, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > t
    assert np.mean(~clear) <= 0.01
    assert np.array_equal(pred[clear], np.argmax(z64, axis=1)[clear])
    assert np.array_equal(f["eng"].classifier_predict(nodes, W, b, which=0), pred)
    # the planted classes are recovered
    assert np.mean(f["eng"].classifier_predict(f["nodes"], W, b) == f["y"]) >= 0.95


def test_predict_exact_tie_goes_to_the_lowest_class(engine_of):
    eng = engine_of(50)
    rs = np.random.RandomState(9)
    for C, pair in ((5, (1, 3)), (128, (70, 5)), (128, (64, 127))):
        W = (0.01 * rs.randn(C, 50)).astype(np.float32)
        b = np.zeros(C, dtype=np.float32)
        hi, lo = max(pair), min(pair)
        W[lo] = W[hi] = (5.0 * np.sign(tables(50)[0][:200].mean(axis=0))).astype(np.float32)
        b[lo] = b[hi] = 100.0  # the two identical rows win everywhere
        pred, z = eng.classifier_predict(np.arange(200), W, b, logits=True)
        assert np.array_equal(z[:, lo].view(np.uint32), z[:, hi].view(np.uint32))
        assert np.all(pred == lo)


def _write_planted(tmp_path, table, nodes, y):
    lab = tmp_path / "labels.txt"
    lab.write_text("".join("%d %d\n" % (v, 10 * c + 3) for v, c in zip(nodes.tolist(), y.tolist())))
    return str(lab)


def test_evaluator_engine_equals_host_fallback(fits, tmp_path):
    from graphgan_amd.evaluation import node_classification as nc
    M, d, C = FIT_CASES[1]
    f = fits(M, d, C)
    lab = _write_planted(tmp_path, f["table"], f["nodes"], f["y"])
    n = len(f["table"])
    dev_ev = nc.NodeClassifyEval("unused", lab, n, d, engine=f["eng"], which=0, seed=5, iters=100)
    host_ev = nc.NodeClassifyEval("unused", lab, n, d, emd=f["table"].astype(np.float64), seed=5, iters=100)
    for a, b in zip(dev_ev.split()[:4], host_ev.split()[:4]):
        assert np.array_equal(a, b)
    dev, host = dev_ev.eval_node_classification(), host_ev.eval_node_classification()
    assert dev == host
    assert dev["acc"] >= 0.95 and dev["macro_f1"] >= 0.95
    assert (dev["n_train"], dev["n_test"]) == (1350, 150)


def test_graph_gan_node_classification_app_writes_the_result_lines(tmp_path):
    """graph_gan.py with app = "node_classification" on the CA-GrQc fixture: one acc / macro_f1 line per mode whose values are
    those of the host fallback on the engine's tables"""
    from graphgan_amd.evaluation import node_classification as nc
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    d, n, graph = write_reference_layout(base)
    lab = str(tmp_path / "labels.txt")
    rs = np.random.RandomState(1)
    labelled = np.sort(rs.permutation(n)[:800])
    deg = np.array([len(graph.get(int(v), ())) for v in labelled])
    classes = np.minimum(deg, 4) * 7 - 2  # five label values that the embeddings say something about
    with open(lab, "w") as f:
        f.writelines("%d\t%d\n" % (v, c) for v, c in zip(labelled.tolist(), classes.tolist()))
    cfg = make_cfg(base, app="node_classification", labels_filename=lab, n_epochs=0, engine_nc_iters=60)
    # (make_cfg derives the paths from the base config's app, link_prediction: where write_reference_layout put the files)
    from graphgan_amd.graph_gan import GraphGAN
    g = GraphGAN(cfg)
    g.train()
    lines = open(cfg.result_filename).read().splitlines()
    assert len(lines) == 2
    for i, (mode, line) in enumerate(zip(("gen", "dis"), lines)):
        host = nc.NodeClassifyEval("unused", lab, g.n_node, cfg.n_emb, emd=g.engine.get_embeddings(i).astype(np.float64),
                                   seed=cfg.engine_seed, iters=60).eval_node_classification()
        assert line + "\n" == nc.format_results(mode, host)
        fields = line[len(mode) + 1:].split(" ")
        assert [x.split("=")[0] for x in fields] == ["acc", "macro_f1", "n_train", "n_test"]
        assert (host["n_train"], host["n_test"]) == (720, 80)
    del cfg.labels_filename
    with pytest.raises(ValueError, match="labels_filename"):
        g.evaluation(g)
    g.engine.close()


def test_node_classification_app_needs_no_test_edges(tmp_path):
    """a graph with compact ids and NO test-edge file: the app runs (the reader gets ""), engine_gen_nll raises clearly"""
    from tests.test_gpu_e2e import make_cfg
    base, n, dim = str(tmp_path), 60, 8
    os.makedirs(os.path.join(base, "data"))
    rs = np.random.RandomState(4)
    with open(os.path.join(base, "data", "train.txt"), "w") as f:
        f.writelines("%d\t%d\n" % (v, (v + k) % n) for v in range(n) for k in (1, 7))
    with open(os.path.join(base, "data", "pre.emb"), "w") as f:
        f.write("%d %d\n" % (n, dim))
        f.writelines(str(v) + " " + " ".join(repr(float(x)) for x in rs.randn(dim)) + "\n" for v in range(n))
    with open(os.path.join(base, "data", "labels.txt"), "w") as f:
        f.writelines("%d %d\n" % (v, v % 3) for v in range(0, n, 2))
    cfg = make_cfg(base, app="node_classification", n_emb=dim, n_epochs=0, engine_nc_iters=5,
                   train_filename=base + "/data/train.txt", test_filename=base + "/data/absent_test.txt",
                   pretrain_emb_filename_d=base + "/data/pre.emb", pretrain_emb_filename_g=base + "/data/pre.emb",
                   labels_filename=base + "/data/labels.txt")
    from graphgan_amd.graph_gan import GraphGAN
    g = GraphGAN(cfg)
    assert g.n_node == n
    g.train()
    lines = open(cfg.result_filename).read().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis"] and all("n_train=27 n_test=3" in ln for ln in lines)
    cfg.engine_gen_nll = True
    with pytest.raises(ValueError, match="engine_gen_nll"):
        g.evaluation(g)
    g.engine.close()


def test_invalid_arguments_name_the_cause(ga, engine_of):
    import ctypes
    from graphgan_amd import _lib
    eng = engine_of(8)
    nodes = np.arange(10, dtype=np.int32)
    y = np.zeros(10, dtype=np.int32)
    out = np.zeros(129 * 8 + 200, dtype=np.float32)
    W = np.zeros((129, 8), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def lossgrad(which, nodes, y, C):
        return _lib.lib.gg_classifier_lossgrad(eng._ctx, which, p(nodes), p(y), len(nodes), C, p(W), p(W), 0.0, p(out), p(out), p(out))

    def last():
        return _lib.lib.gg_last_error(eng._ctx).decode()

    assert lossgrad(0, nodes, y, 1) == _lib.GG_EINVAL and "n_class = 1 outside [2, 128]" in last()
    assert lossgrad(0, nodes, y, 129) == _lib.GG_EINVAL and "n_class = 129 outside [2, 128]" in last()
    y_bad = y.copy()
    y_bad[3] = 5
    assert lossgrad(0, nodes, y_bad, 5) == _lib.GG_EINVAL and "label 5" in last() and "n_class = 5" in last()
    n_bad = nodes.copy()
    n_bad[7] = N_TABLE
    assert lossgrad(0, n_bad, y, 5) == _lib.GG_EINVAL and "node id %d" % N_TABLE in last()
    assert lossgrad(2, nodes, y, 5) == _lib.GG_EINVAL and "which must be 0" in last()
    pred = np.zeros(10, dtype=np.int32)
    assert _lib.lib.gg_classifier_predict(eng._ctx, 2, p(nodes), 10, 5, p(W), p(W), p(pred), None) == _lib.GG_EINVAL and "which" in last()
    assert _lib.lib.gg_classifier_fit(eng._ctx, 0, p(n_bad), p(y), 10, 5, 3, 0.05, 0.0, p(W), p(W), None, None) == _lib.GG_EINVAL
    assert "node id" in last()
    # the Python layer refuses the same before the ABI
    Wok = np.zeros((5, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="n_class"):
        eng.classifier_fit(nodes, y, 1)
    with pytest.raises(ValueError, match="n_class"):
        eng.classifier_fit(nodes, y, 129)
    with pytest.raises(ValueError, match="label"):
        eng.classifier_fit(nodes, y_bad, 5)
    with pytest.raises(ValueError, match="node id"):
        eng.classifier_lossgrad(n_bad, y, Wok, Wok[:, 0].copy())
    with pytest.raises(ValueError, match="which"):
        eng.classifier_predict(nodes, Wok, Wok[:, 0].copy(), which=2)
    # the engine still works
    assert np.isfinite(eng.classifier_lossgrad(nodes, y, Wok, Wok[:, 0].copy())["loss"])
