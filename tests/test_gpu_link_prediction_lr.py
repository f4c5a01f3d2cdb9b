"""Learned link prediction on the device (gg_edge_classifier_* / Engine.edge_classifier_*, LinkPredictLREval, graph_gan.py's
engine_lp_classifier) against the numpy restatement tests/support/edge_classifier_ref.py.  Tolerances are derived as in
test_gpu_node_classification.py: dev = max |float32 reference - float64 reference| on the test's own inputs, and the device must
lie within max(8 dev, 1e-6) of the float64 reference (classifier_ref.tol).  The trip-structure sizes come from the restated launch
plan (edge_classifier_ref.M_*), and at those sizes the sweep is checked bit for bit against closed forms on integer tables."""
import ctypes

import numpy as np
import pytest

from tests.support import classifier_harness as harness
from tests.support import edge_classifier_ref as ref
from tests.support.classifier_harness import N_TABLE, compare, tables
from tests.support.classifier_shapes import bits_equal, int_tables

pytestmark = pytest.mark.gpu

OPS = ref.OPERATORS
D_CASES = [1, 3, 8, 50, 128, 200, 256]  # 1, 3: padded to ld = 4; 50, 200: a ragged last float4 group; 128, 200, 256: 2 and 4 pieces per lane
M_CASES = [1, 2, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def engine_of():
    yield harness.engine_of
    harness.close_engines()


_int_engines = {}


@pytest.fixture(scope="module")
def int_engine_of():
    """the engine on classifier_shapes.int_tables(d) (entries in {-1, 0, 1}), made once per d"""
    def get(d):
        if d not in _int_engines:
            import graphgan_amd
            _int_engines[d] = graphgan_amd.Engine(*int_tables(d))
        return _int_engines[d]
    yield get
    for e in _int_engines.values():
        e.close()
    _int_engines.clear()


def draw_edges(rs, M):
    """random pairs; from M = 4 on: a repeated edge, a reversed copy of an edge and a self-pair (M = 2: the reversed copy)"""
    u, v = rs.randint(0, N_TABLE, size=M), rs.randint(0, N_TABLE, size=M)
    if M >= 2:
        u[-1], v[-1] = v[0], u[0]
    if M >= 4:
        u[1], v[1] = u[0], v[0]
        v[2] = u[2]
    return u, v


def outputs(res):
    return res["loss"], res["gw"], res["gb"]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("d", D_CASES)
def test_lossgrad_matches_float64(engine_of, d, op):
    eng = engine_of(d)
    for M in M_CASES:
        rs = np.random.RandomState(M * 1000 + d + OPS.index(op))
        u, v = draw_edges(rs, M)
        y = rs.randint(0, 2, size=M)
        w = (0.5 * rs.randn(d)).astype(np.float32)
        b = np.float32(0.5 * rs.randn() + 0.1)
        assert b != 0
        for which in ((0, 1) if M == 130 else (0,)):
            T = tables(d)[which]
            r64 = ref.lossgrad(T[u], T[v], y, w, b, 1e-3, op, np.float64)
            r32 = ref.lossgrad(T[u], T[v], y, w, b, 1e-3, op, np.float32)
            got = eng.edge_classifier_lossgrad(u, v, y, w, b, op=op, which=which, l2=1e-3)
            compare("edge lossgrad %s (M %d, d %d) which %d" % (op, M, d, which), ("loss", "gw", "gb"), outputs(got), r64, r32)
        if M == 130:  # the operator by its number; and `which` is honoured
            num = eng.edge_classifier_lossgrad(u, v, y, w, b, op=OPS.index(op), which=1, l2=1e-3)
            assert num["loss"] == got["loss"] and bits_equal(num["gw"], got["gw"])
            g0 = ref.lossgrad(tables(d)[0][u], tables(d)[0][v], y, w, b, 1e-3, op)[1]
            assert np.max(np.abs(g0 - r64[1])) > 1e-4


@pytest.mark.parametrize("M", [ref.M_SECOND_TRIP, ref.M_THREE_TRIPS_MIN, ref.M_THREE_TRIPS])
@pytest.mark.parametrize("d", [8, 128, 256])
def test_trip_structure_exact_on_integer_tables(int_engine_of, d, M):
    """M from the launch plan: workgroup 0 alone takes a second trip with one valid edge / every workgroup takes two trips and
    workgroup 0 (workgroups 0 .. 36, the last trip with 5 edges) a third.  Integer tables, zero parameters: gw and gb bit for bit."""
    assert ref.second_trip_single_edge(M) if M == ref.M_SECOND_TRIP else ref.two_and_three_trips_ragged(M)
    eng = int_engine_of(d)
    rs = np.random.RandomState(d + M)
    u, v = draw_edges(rs, M)
    y = rs.randint(0, 2, size=M)
    w0 = np.zeros(d, dtype=np.float32)
    for op in OPS:
        which = OPS.index(op) & 1
        T = int_tables(d)[which]
        num, den = ref.int_features(T[u], T[v], op)
        assert ref.headroom(num) < 2 ** 24
        gw, gb = ref.exact(T[u], T[v], y, op)
        got = eng.edge_classifier_lossgrad(u, v, y, w0, 0.0, op=op, which=which, l2=0.0)
        assert bits_equal(got["gw"], gw), (op, int(np.sum(got["gw"] != gw)))
        assert np.float32(got["gb"]) == gb
        assert got["loss"] == pytest.approx(np.log(2), rel=1e-6)
        assert np.any(gw != 0)


@pytest.mark.parametrize("d,M", [(50, 130), (256, 997), (3, 65)])
def test_exchanging_the_ends_changes_no_bit(engine_of, d, M):
    eng = engine_of(d)
    rs = np.random.RandomState(d * M)
    u, v = draw_edges(rs, M)
    y = rs.randint(0, 2, size=M)
    w = (0.5 * rs.randn(d)).astype(np.float32)
    for op in OPS:
        a = eng.edge_classifier_lossgrad(u, v, y, w, 0.25, op=op, which=0, l2=1e-3)
        b = eng.edge_classifier_lossgrad(v, u, y, w, 0.25, op=op, which=0, l2=1e-3)
        assert np.float32(a["loss"]).view(np.uint32) == np.float32(b["loss"]).view(np.uint32), op
        assert bits_equal(a["gw"], b["gw"]) and np.float32(a["gb"]).view(np.uint32) == np.float32(b["gb"]).view(np.uint32), op
        za = eng.edge_classifier_predict(u, v, w, 0.25, op=op)
        assert bits_equal(za, eng.edge_classifier_predict(v, u, w, 0.25, op=op)), op
        again = eng.edge_classifier_lossgrad(u, v, y, w, 0.25, op=op, which=0, l2=1e-3)
        assert again["loss"] == a["loss"] and bits_equal(again["gw"], a["gw"]) and again["gb"] == a["gb"]  # the same call, the same bits


def test_saturated_logits_stay_finite_and_exact():
    """rows scaled until the logits pass +-200: log(1 + exp z) is inf in float32 there; the stable forms give a finite loss, and
    on the edges whose float64 sigmoid rounds (to float32) to the label the gradient is exactly 0.  Logits inside the bands
    where that rounding is decided (15 .. 19 and -120 .. -88) are left out of the input."""
    import graphgan_amd
    d, S = 8, 60.0
    T = (tables(d)[0] * np.float32(S)).astype(np.float32)
    eng = graphgan_amd.Engine(T, T)
    try:
        rs = np.random.RandomState(77)
        u, v = rs.randint(0, N_TABLE, size=400), rs.randint(0, N_TABLE, size=400)
        w = (0.5 * rs.randn(d)).astype(np.float32)
        b = np.float32(0.3)
        z = ref.logits(T[u], T[v], w, b, "hadamard")
        keep = ~(((z > 15) & (z < 19)) | ((z < -88) & (z > -120)))
        u, v, z = u[keep][:260], v[keep][:260], z[keep][:260]
        assert z.max() > 200 and z.min() < -200 and len(z) == 260
        y = np.where(rs.rand(len(z)) < 0.7, z > 0, rs.rand(len(z)) < 0.5).astype(np.int64)
        with np.errstate(over="ignore"):
            assert np.isinf(np.log(np.float32(1) + np.exp(np.float32(200.0))))
        r64 = ref.lossgrad(T[u], T[v], y, w, b, 0.0, "hadamard", np.float64)
        r32 = ref.lossgrad(T[u], T[v], y, w, b, 0.0, "hadamard", np.float32)
        got = eng.edge_classifier_lossgrad(u, v, y, w, b, op="hadamard", l2=0.0)
        assert np.isfinite(got["loss"]) and np.all(np.isfinite(got["gw"])) and np.isfinite(got["gb"])
        compare("edge saturation", ("loss", "gw", "gb"), outputs(got), r64, r32)
        e = np.exp(-np.abs(z))
        sig32 = (np.where(z >= 0, 1.0, e) / (1.0 + e)).astype(np.float32)
        settled = sig32 == y.astype(np.float32)
        assert settled.sum() >= 40 and (y[settled] == 1).any() and (y[settled] == 0).any()
        only = eng.edge_classifier_lossgrad(u[settled], v[settled], y[settled], w, b, op="hadamard", l2=0.0)
        assert np.all(only["gw"] == 0) and only["gb"] == 0 and np.isfinite(only["loss"])
    finally:
        eng.close()


FIT_CASES = [(130, 8), (4000, 50), (4000, 128)]
_fits = {}


@pytest.fixture(scope="module")
def fits(engine_of):
    """edges labelled by a planted (w*, b*), the two reference fits and the device fit of one (M, d, op), made once"""
    def get(M, d, op):
        key = (M, d, op)
        if key not in _fits:
            eng, T = engine_of(d), tables(d)[0]
            rs = np.random.RandomState(7 * M + d + OPS.index(op))
            u, v = draw_edges(rs, M)
            zs = ref.logits(T[u], T[v], 4.0 * rs.randn(d), 0.0, op)
            y = (zs > np.median(zs)).astype(np.int64)
            r64 = ref.fit(T[u], T[v], y, 100, 0.05, 1e-4, op, np.float64)
            r32 = ref.fit(T[u], T[v], y, 100, 0.05, 1e-4, op, np.float32)
            got = eng.edge_classifier_fit(u, v, y, op=op, which=0, iters=100, lr=0.05, l2=1e-4)
            _fits[key] = dict(u=u, v=v, y=y, eng=eng, T=T, r64=r64, r32=r32, got=got)
        return _fits[key]
    yield get
    _fits.clear()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("M,d", FIT_CASES)
def test_fit_matches_float64(fits, M, d, op):
    f = fits(M, d, op)
    got = f["got"]
    assert got["loss"].shape == (100,) and got["ms"] > 0 and got["w"].shape == (d,)
    assert got["loss"][0] == pytest.approx(np.log(2), rel=1e-6)  # (zeros: the loss before update 1)
    compare("edge fit %s (%d, %d)" % (op, M, d), ("w", "b", "loss"), (got["w"], got["b"], got["loss"]), f["r64"], f["r32"])
    assert got["loss"][-1] < got["loss"][0]
    again = f["eng"].edge_classifier_fit(f["u"], f["v"], f["y"], op=op, which=0, iters=100, lr=0.05, l2=1e-4)
    assert bits_equal(again["w"], got["w"]) and again["b"] == got["b"] and bits_equal(again["loss"], got["loss"])
    # from given parameters: the second half of the trajectory is NOT the continuation (Adam's moments start again) but its
    # first loss is the loss at those parameters
    cont = f["eng"].edge_classifier_fit(f["u"], f["v"], f["y"], op=op, which=0, iters=1, lr=0.05, l2=1e-4, w=got["w"], b=got["b"])
    at = f["eng"].edge_classifier_lossgrad(f["u"], f["v"], f["y"], got["w"], got["b"], op=op, which=0, l2=1e-4)
    assert cont["loss"][0] == np.float32(at["loss"])


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("M,d", FIT_CASES)
def test_predict_matches_float64(fits, M, d, op):
    f = fits(M, d, op)
    w, b = f["got"]["w"], f["got"]["b"]
    z64 = ref.logits(f["T"][f["u"]], f["T"][f["v"]], w, b, op, np.float64)
    z32 = ref.logits(f["T"][f["u"]], f["T"][f["v"]], w, np.float32(b), op, np.float32)
    z = f["eng"].edge_classifier_predict(f["u"], f["v"], w, b, op=op, which=0)
    assert z.dtype == np.float32 and z.shape == (M,)
    compare("edge predict %s (%d, %d)" % (op, M, d), ("logits",), (z,), (z64,), (z32,))
    assert np.mean((z > 0) == (f["y"] == 1)) > 0.6  # the planted labels are learnt


def test_predict_over_three_trips(engine_of):
    """M_PREDICT: every workgroup of edge_predict_kernel takes two trips, workgroups 0 .. 17 a third, the last with 7 edges"""
    M, d = ref.M_PREDICT, 50
    assert ref.trip_counts(M, ref.predict_grid(M)) == (2, 3, 18, 7)
    eng, T = engine_of(d), tables(d)[1]
    rs = np.random.RandomState(M)
    u, v = draw_edges(rs, M)
    w = (0.5 * rs.randn(d)).astype(np.float32)
    for op in ("l1", "hadamard"):
        z = eng.edge_classifier_predict(u, v, w, -0.2, op=op, which=1)
        z64 = ref.logits(T[u], T[v], w, np.float32(-0.2), op, np.float64)
        z32 = ref.logits(T[u], T[v], w, np.float32(-0.2), op, np.float32)
        compare("edge predict %s (M_PREDICT, %d)" % (op, d), ("logits",), (z,), (z64,), (z32,))


@pytest.mark.parametrize("op", OPS)
def test_evaluator_engine_equals_host_fallback(tmp_path, op):
    import graphgan_amd
    from graphgan_amd.evaluation import link_prediction_lr as lplr
    c = ref.planted_case(op, tmp_path)
    T = c["table"]
    eng = graphgan_amd.Engine(T, T[::-1].copy())
    try:
        args = (c["train"], c["test"], c["test_neg"], c["n"], c["d"])
        dev_ev = lplr.LinkPredictLREval(*args, engine=eng, which=0, operator=op, seed=3)
        host_ev = lplr.LinkPredictLREval(*args, emd=T.astype(np.float64), operator=op, seed=3)
        sets = host_ev.read_sets()
        for a, b in zip(sets, dev_ev.read_sets()):
            assert np.array_equal(a, b)
        # no logit is close enough to the threshold or to a logit of the other class to change a metric: the gaps of the float64
        # restatement against the tolerance of the fitted logits
        u, v, y, tu, tv, ty = sets
        w64, b64, _ = ref.fit(T[u], T[v], y, 200, 0.05, 1e-4, op, np.float64)
        w32, b32, _ = ref.fit(T[u], T[v], y, 200, 0.05, 1e-4, op, np.float32)
        z64 = ref.logits(T[tu], T[tv], w64, b64, op, np.float64)
        z32 = ref.logits(T[tu], T[tv], w32, b32, op, np.float32)
        t = ref.tol(z32, z64)
        gap = z64[ty == 1].min() - z64[ty == 0].max()
        print("evaluator %s: smallest score gap %.4g, smallest |logit| %.4g, tol %.3g" % (op, gap, np.abs(z64).min(), t))
        assert gap > 2 * t and np.abs(z64).min() > t
        z_dev = dev_ev.logits(sets)[0]
        assert np.max(np.abs(z_dev.astype(np.float64) - z64)) <= t
        dev, host = dev_ev.eval_link_prediction(), host_ev.eval_link_prediction()
        assert dev == host
        assert dev == dict(acc=1.0, macro_f1=1.0, auc=1.0, n_train=180, n_test=60)
    finally:
        eng.close()


def test_graph_gan_writes_the_lp_lines(tmp_path):
    """graph_gan.py with engine_lp_classifier on the CA-GrQc fixture: after the app's own lines one _lp line per mode, equal to
    a direct evaluator call on the engine's tables"""
    from graphgan_amd.evaluation import link_prediction_lr as lplr
    from graphgan_amd.graph_gan import GraphGAN
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    write_reference_layout(base)
    cfg = make_cfg(base, n_epochs=0, engine_lp_classifier=True, engine_lp_iters=60, engine_lp_operator="l1", engine_seed=5)
    g = GraphGAN(cfg)
    g.train()
    lines = open(cfg.result_filename).read().splitlines()
    assert len(lines) == 4 and lines[0].startswith("gen:0.") and lines[1].startswith("dis:0.")
    for i, (mode, line) in enumerate(zip(("gen", "dis"), lines[2:])):
        direct = lplr.LinkPredictLREval(cfg.train_filename, cfg.test_filename, cfg.test_neg_filename, g.n_node, cfg.n_emb, engine=g.engine,
                                        which=i, operator="l1", iters=60, seed=5).eval_link_prediction()
        assert line + "\n" == lplr.format_results(mode, direct)
        assert line.startswith(mode + "_lp:acc=")
        assert [x.split("=")[0] for x in line[len(mode) + 4:].split(" ")] == ["acc", "macro_f1", "auc", "n_train", "n_test"]
        assert direct["n_test"] == 2 * 1449 and direct["n_train"] == 2 * 13046 and 0.5 < direct["auc"] < 1.0  # (the fixture's edge counts)
    g.engine.close()


def test_invalid_arguments_name_the_cause(engine_of):
    from graphgan_amd import _lib
    eng = engine_of(8)
    L = _lib.lib
    u, v = np.arange(10, dtype=np.int32), np.arange(10, dtype=np.int32)[::-1].copy()
    y = (np.arange(10) & 1).astype(np.int32)
    w, b = np.zeros(8, dtype=np.float32), np.zeros(1, dtype=np.float32)
    out = np.zeros(16, dtype=np.float32)
    inf, nan = float("inf"), float("nan")
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def lossgrad(which=0, op=0, u=u, v=v, y=y, m=10, w=w, b=b, l2=0.0, loss=out, gw=out, gb=out):
        return L.gg_edge_classifier_lossgrad(eng._ctx, which, op, p(u), p(v), p(y), m, p(w), p(b), l2, p(loss), p(gw), p(gb))

    def fit(which=0, op=0, u=u, v=v, y=y, m=10, iters=3, lr=0.05, l2=0.0, w=w, b=b):
        return L.gg_edge_classifier_fit(eng._ctx, which, op, p(u), p(v), p(y), m, iters, lr, l2, p(w), p(b), None, None)

    def predict(which=0, op=0, u=u, v=v, m=10, w=w, b=b, z=out):
        return L.gg_edge_classifier_predict(eng._ctx, which, op, p(u), p(v), m, p(w), p(b), p(z))

    def last():
        return L.gg_last_error(eng._ctx).decode()

    def refused(rc, fn, *words):
        text = last()
        assert rc == _lib.GG_EINVAL and fn in text and all(x in text for x in words), (rc, text)

    u_bad, v_bad, y_bad = u.copy(), v.copy(), y.copy()
    u_bad[7], v_bad[4], y_bad[6] = N_TABLE, -1, 2
    for call, fn in ((lossgrad, "gg_edge_classifier_lossgrad"), (fit, "gg_edge_classifier_fit"), (predict, "gg_edge_classifier_predict")):
        refused(call(which=2), fn, "which must be 0")
        refused(call(op=4), fn, "op = 4 outside [0, 3]")
        refused(call(op=-1), fn, "op = -1 outside [0, 3]")
        refused(call(m=0), fn, "m = 0 outside [1, 2^31 - 1]")
        refused(call(m=2 ** 31), fn, "outside [1, 2^31 - 1]")
        refused(call(u=None), fn, "u is NULL")
        refused(call(v=None), fn, "v is NULL")
        refused(call(u=u_bad), fn, "node id u = %d" % N_TABLE, "entry 7")
        refused(call(v=v_bad), fn, "node id v = -1", "entry 4")
        refused(call(w=None), fn, "must not be NULL")
        refused(call(b=None), fn, "must not be NULL")
    for call, fn in ((lossgrad, "gg_edge_classifier_lossgrad"), (fit, "gg_edge_classifier_fit")):
        refused(call(y=None), fn, "y is NULL")
        refused(call(y=y_bad), fn, "y = 2", "entry 6")
        refused(call(l2=-1.0), fn, "l2 must be finite and >= 0")
        refused(call(l2=inf), fn, "l2 must be finite and >= 0")
        refused(call(l2=nan), fn, "l2 must be finite and >= 0")
    refused(lossgrad(loss=None), "gg_edge_classifier_lossgrad", "must not be NULL")
    refused(lossgrad(gw=None), "gg_edge_classifier_lossgrad", "must not be NULL")
    refused(lossgrad(gb=None), "gg_edge_classifier_lossgrad", "must not be NULL")
    refused(predict(z=None), "gg_edge_classifier_predict", "must not be NULL")
    refused(fit(iters=0), "gg_edge_classifier_fit", "iters = 0 outside [1, 1000000]")
    refused(fit(iters=1000001), "gg_edge_classifier_fit", "iters = 1000001 outside [1, 1000000]")
    refused(fit(lr=0.0), "gg_edge_classifier_fit", "lr must be finite and > 0")
    refused(fit(lr=-0.1), "gg_edge_classifier_fit", "lr must be finite and > 0")
    refused(fit(lr=inf), "gg_edge_classifier_fit", "lr must be finite and > 0")
    assert not out.any() and not w.any()  # nothing was launched, nothing written
    # n_emb <= 256
    import graphgan_amd
    wide = graphgan_amd.Engine(np.zeros((20, 260), dtype=np.float32), np.zeros((20, 260), dtype=np.float32))
    try:
        w260 = np.zeros(260, dtype=np.float32)
        rc = L.gg_edge_classifier_predict(wide._ctx, 0, 0, p(u), p(v), 10, p(w260), p(b), p(out))
        text = L.gg_last_error(wide._ctx).decode()
        assert rc == _lib.GG_EINVAL and "gg_edge_classifier_predict" in text and "n_emb <= 256 (got 260)" in text
        rc = L.gg_edge_classifier_fit(wide._ctx, 0, 0, p(u), p(v), p(y), 10, 3, 0.05, 0.0, p(w260), p(b), None, None)
        assert rc == _lib.GG_EINVAL and "gg_edge_classifier_fit" in L.gg_last_error(wide._ctx).decode()
        rc = L.gg_edge_classifier_lossgrad(wide._ctx, 0, 0, p(u), p(v), p(y), 10, p(w260), p(b), 0.0, p(out), p(w260), p(out))
        assert rc == _lib.GG_EINVAL and "n_emb <= 256" in L.gg_last_error(wide._ctx).decode()
    finally:
        wide.close()
    # the Python layer refuses the same before the ABI
    with pytest.raises(ValueError, match="operator"):
        eng.edge_classifier_lossgrad(u, v, y, w, 0.0, op="cosine")
    with pytest.raises(ValueError, match="operator"):
        eng.edge_classifier_predict(u, v, w, 0.0, op=4)
    with pytest.raises(ValueError, match="which"):
        eng.edge_classifier_fit(u, v, y, which=2)
    with pytest.raises(ValueError, match="node id"):
        eng.edge_classifier_fit(u_bad, v, y)
    with pytest.raises(ValueError, match="0 / 1"):
        eng.edge_classifier_fit(u, v, y_bad)
    with pytest.raises(ValueError, match="one length"):
        eng.edge_classifier_predict(u, v[:9], w, 0.0)
    with pytest.raises(ValueError, match="iters"):
        eng.edge_classifier_fit(u, v, y, iters=0)
    with pytest.raises(ValueError, match="lr must be"):
        eng.edge_classifier_fit(u, v, y, lr=0.0)
    with pytest.raises(ValueError, match="w must be"):
        eng.edge_classifier_predict(u, v, np.zeros(9, dtype=np.float32), 0.0)
    # self-pairs are legal, and the engine still works
    res = eng.edge_classifier_lossgrad(u, u, y, w, 0.0, op="l2")
    assert res["loss"] == pytest.approx(np.log(2), rel=1e-6) and res["gb"] == 0.0 and not res["gw"].any()
