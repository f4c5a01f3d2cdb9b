"""The classifier's sweep (graphgan_amd/csrc/classifier.hip, nc_sweep_kernel<CT, DT, ML>) at the shapes its launch plan
(graphgan_amd/csrc/row_tiles.h, row_tile_plan) makes different: every one of the 64 template instances, the six whose W is staged in k-chunks, more tiles than workgroups (the
persistent loop, the prefetch, the accumulators carried across tiles, a 512-partial stage), the predict kernels above 48 KiB of
LDS with a row loop of three trips, and saturated softmax logits.

Two kinds of comparison only.  EXACT: on tables of {-1, 0, 1} at W = 0, b = 0, l2 = 0 the gradients have closed forms that the
device must give bit for bit (tests/support/classifier_shapes.py; premises in tests/test_classifier_shapes_cpu.py) -- this
counts every row once, in any summation order; likewise ties and run-to-run reproducibility.  DERIVED: random weights against
the float64 restatement within classifier_ref.tol = max(8 |float32 reference - float64 reference|, 1e-6) on the test's own
inputs, as in test_gpu_node_classification.py.  The loss is a float64 sum all the way to the reducer (the stage holds each workgroup's loss partial as two
floats): at M = 130 a partial rounded to ONE float moves the mean by more than this rule allows."""
import numpy as np
import pytest

from tests.support import classifier_ml_ref as ml_ref
from tests.support import classifier_ref as ref
from tests.support import classifier_shapes as cs

pytestmark = pytest.mark.gpu

N_TABLE = cs.N_TABLE
SOFTMAX, SIGMOID = "softmax", "sigmoid"


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


_tables = {}


def tables(d, kind="rand"):
    """two different tables [N_TABLE, d] (generator, discriminator), made once per d: random, or of {-1, 0, 1}"""
    if (d, kind) not in _tables:
        if kind == "int":
            _tables[(d, kind)] = cs.int_tables(d)
        else:
            rs = np.random.RandomState(100 + d)
            _tables[(d, kind)] = ((0.3 * rs.randn(N_TABLE, d)).astype(np.float32), (0.3 * rs.randn(N_TABLE, d) + 0.05).astype(np.float32))
    return _tables[(d, kind)]


# Engines are cached per (d, kind of table) as in the two sister files, but this file meets 18 values of d x 2 kinds: at most
# MAX_ENGINES stay open, the oldest is closed when another is needed.  A closed engine is simply made again on the next request,
# so eviction costs time, never correctness; it costs nothing as long as the parametrised cases stay sorted by d (they are: see
# the sorted(...) lists below), because a d is then finished before its engines can become the oldest.
_engines = {}
MAX_ENGINES = 8


@pytest.fixture(scope="module")
def engine_of(ga):
    def get(d, kind="rand"):
        key = (d, kind)
        if key not in _engines:
            while len(_engines) >= MAX_ENGINES:
                _engines.pop(next(iter(_engines))).close()
            _engines[key] = ga.Engine(*tables(d, kind))
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()
    _tables.clear()


def compare(tag, names, got, r64, r32):
    for name, g, w64, w32 in zip(names, got, r64, r32):
        t = ref.tol(w32, w64)
        err = float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w64)))
        print("%s %s: err %.3g tol %.3g" % (tag, name, err, t))
        assert err <= t, (tag, name, err, t)


def exact_leg(engine_of, variant, M, d, C, seed):
    """check A: integer tables, zero parameters -> the closed forms bit for bit (softmax: C a power of two)"""
    if variant == SOFTMAX and not cs.is_pow2(C):
        return
    eng = engine_of(d, "int")
    rs = np.random.RandomState(seed)
    nodes = cs.draw_nodes(rs, M)
    which = 0 if variant == SOFTMAX else 1
    X = tables(d, "int")[which][nodes]
    W, b = np.zeros((C, d), dtype=np.float32), np.zeros(C, dtype=np.float32)
    if variant == SOFTMAX:
        y = cs.draw_labels(rs, M, C)
        assert cs.headroom(X, C) < 2 ** 24
        want_W, want_b = cs.exact_softmax(X, y, C)
        got = eng.classifier_lossgrad(nodes, y, W, b, which=which, l2=0.0)
        assert got["loss"] == pytest.approx(np.log(C), rel=1e-6)
    else:
        Y = cs.draw_label_sets(rs, M, C)
        assert cs.headroom(X, 2) < 2 ** 24
        want_W, want_b = cs.exact_sigmoid(X, Y)
        got = eng.classifier_ml_lossgrad(nodes, Y, W, b, which=which, l2=0.0)
        assert got["loss"] == pytest.approx(C * np.log(2), rel=1e-6)
    tag = "exact %s (%d, %d, %d)" % (variant, M, d, C)
    bad_b = np.flatnonzero(got["gb"].view(np.uint32) != want_b.view(np.uint32))
    bad_W = np.argwhere(got["gW"].view(np.uint32) != want_W.view(np.uint32))
    print("%s: %d of %d gb and %d of %d gW entries differ" % (tag, len(bad_b), C, len(bad_W), C * d))
    assert len(bad_b) == 0, (tag, "gb", bad_b[:8], got["gb"][bad_b[:8]] * np.float32(M), want_b[bad_b[:8]] * np.float32(M))
    assert len(bad_W) == 0, (tag, "gW", bad_W[:8])


def parity_leg(engine_of, variant, M, d, C, seed):
    """random weights, l2 = 1e-3, both tables, against the float64 restatement within ref.tol"""
    eng = engine_of(d)
    rs = np.random.RandomState(seed)
    nodes = cs.draw_nodes(rs, M)
    labels = cs.draw_labels(rs, M, C) if variant == SOFTMAX else cs.draw_label_sets(rs, M, C)
    W = (0.5 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    l2 = 1e-3
    lossgrad, call = (ref.lossgrad, eng.classifier_lossgrad) if variant == SOFTMAX else (ml_ref.lossgrad, eng.classifier_ml_lossgrad)
    gW = []
    for which in (0, 1):
        X = tables(d)[which][nodes]
        r64 = lossgrad(X, labels, W, b, l2, np.float64)
        r32 = lossgrad(X, labels, W, b, l2, np.float32)
        got = call(nodes, labels, W, b, which=which, l2=l2)
        compare("%s (%d, %d, %d) which %d" % (variant, M, d, C, which), ("loss", "gW", "gb"), (got["loss"], got["gW"], got["gb"]), r64, r32)
        gW.append(r64[1])
    assert np.max(np.abs(gW[0] - gW[1])) > 1e-3  # (the two tables give different gradients: `which` is honoured)


def test_cases_reach_all_64_instances():
    reached = {(v, cs.sweep_plan(C, cs.ld_of(d))["CT"], cs.sweep_plan(C, cs.ld_of(d))["DT"]) for v in (SOFTMAX, SIGMOID) for C, d in cs.INSTANCE_CASES}
    assert reached == {(v, CT, DT) for v in (SOFTMAX, SIGMOID) for CT in range(1, 5) for DT in range(1, 9)}
    chunked = {(p["CT"], p["DT"]) for p in (cs.sweep_plan(C, cs.ld_of(d)) for C, d in cs.INSTANCE_CASES) if len(p["chunks"]) > 1}
    assert chunked == cs.CHUNKED


# B. every instance at M = 130 (three tiles, the last with 2 rows), ordered by d
@pytest.mark.parametrize("variant", [SOFTMAX, SIGMOID])
@pytest.mark.parametrize("C,d", sorted(cs.INSTANCE_CASES + cs.RAGGED_CASES, key=lambda cd: (cd[1], cd[0])))
def test_every_instance(engine_of, variant, C, d):
    M = cs.M_SMALL
    exact_leg(engine_of, variant, M, d, C, 11 * C + d)
    parity_leg(engine_of, variant, M, d, C, 13 * C + d)


# C. more tiles than workgroups
@pytest.mark.parametrize("variant", [SOFTMAX, SIGMOID])
@pytest.mark.parametrize("M,d,C", sorted(cs.MULTI_TILE_CASES, key=lambda c: (c[1], c[0])))
def test_multi_tile_sweep(engine_of, variant, M, d, C):
    assert cs.cdiv(M, cs.NC_RT) > cs.NC_MAX_GRID
    exact_leg(engine_of, variant, M, d, C, M + 11 * C + d)
    parity_leg(engine_of, variant, M, d, C, M + 13 * C + d)


@pytest.mark.parametrize("variant,C", [(SOFTMAX, 7), (SIGMOID, 33)])
def test_multi_tile_fit_matches_float64_and_repeats(ga, variant, C):
    """30 steps of Adam over 513 tiles on planted data against the float64 fit; a second run gives the same bits"""
    M, d, iters = cs.M1, 50, 30
    assert cs.cdiv(M, cs.NC_RT) > cs.NC_MAX_GRID
    r = ref if variant == SOFTMAX else ml_ref
    table, nodes, labels = r.planted(M, d, C, M + 1000, 7 * M + d)
    X = table[nodes]
    if variant == SOFTMAX:
        r64, r32 = (ref.fit(X, labels, C, iters, 0.05, 1e-4, dt) for dt in (np.float64, np.float32))
    else:
        r64, r32 = (ml_ref.fit(X, labels, iters, 0.05, 1e-4, dt) for dt in (np.float64, np.float32))
    eng = ga.Engine(table, table[::-1].copy())
    try:
        fit = eng.classifier_fit if variant == SOFTMAX else eng.classifier_ml_fit
        got = fit(nodes, labels, C, which=0, iters=iters, lr=0.05, l2=1e-4)
        again = fit(nodes, labels, C, which=0, iters=iters, lr=0.05, l2=1e-4)
    finally:
        eng.close()
    assert got["loss"].shape == (iters,)
    compare("%s fit (%d, %d, %d)" % (variant, M, d, C), ("W", "b", "loss"), (got["W"], got["b"], got["loss"]), r64, r32)
    assert got["loss"][-1] < got["loss"][0]
    for key in ("W", "b", "loss"):
        assert cs.bits_equal(again[key], got[key]), key


# D. the predict kernels with 66 - 132 KiB of W in LDS and three trips of the row loop
@pytest.mark.parametrize("C,d", cs.PREDICT_CASES)
def test_predict_large_lds_many_rows(engine_of, C, d):
    eng, m = engine_of(d), cs.M_PREDICT
    rs = np.random.RandomState(17 * C + d)
    nodes = cs.draw_nodes(rs, m)
    W = (0.5 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    X = tables(d)[1][nodes]
    z64, z32 = ref.logits(X, W, b, np.float64), ref.logits(X, W, b, np.float32)
    t = ref.tol(z32, z64)
    # argmax
    pred, z = eng.classifier_predict(nodes, W, b, which=1, logits=True)
    err = float(np.max(np.abs(z.astype(np.float64) - z64)))
    print("predict (%d, %d, %d): logits err %.3g tol %.3g" % (m, d, C, err, t))
    assert err <= t
    top2 = np.sort(z64, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > t
    assert np.mean(~clear) <= 0.01
    assert np.array_equal(pred[clear], np.argmax(z64, axis=1)[clear])
    assert np.array_equal(eng.classifier_predict(nodes, W, b, which=1), pred)
    # top-k and threshold
    k = rs.randint(0, 6, size=m)
    k[:3] = (0, C, 1)
    sets, zm = eng.classifier_ml_predict(nodes, W, b, which=1, k=k, logits=True)
    err = float(np.max(np.abs(zm.astype(np.float64) - z64)))
    print("ml predict (%d, %d, %d): logits err %.3g tol %.3g" % (m, d, C, err, t))
    assert err <= t
    clear = ml_ref.topk_gap(z64, k) > t
    assert np.mean(~clear) <= 0.01
    assert np.array_equal(sets[clear], ml_ref.predict_topk(z64, k)[clear])
    assert np.array_equal(sets.sum(axis=1), k)
    thr, z2 = eng.classifier_ml_predict(nodes, W, b, which=1, logits=True)
    assert cs.bits_equal(z2, zm)
    sure = np.abs(z64) > t
    assert np.mean(~sure) <= 0.01
    assert np.array_equal(thr[sure], ml_ref.predict_threshold(z64)[sure])
    assert np.array_equal(thr, zm > 0)  # (on the device's own logits the rule is exact)


def test_predict_exact_ties_go_to_the_lower_class_at_the_largest_shape(engine_of):
    C, d, n, lo, hi = 128, 256, 200, 64, 127
    eng = engine_of(d)
    rs = np.random.RandomState(9)
    W = (0.01 * rs.randn(C, d)).astype(np.float32)
    b = np.zeros(C, dtype=np.float32)
    W[lo] = W[hi] = np.sign(tables(d)[0][:n].mean(axis=0)).astype(np.float32)
    b[lo] = b[hi] = 100.0  # the two identical rows come first everywhere
    pred, z = eng.classifier_predict(np.arange(n), W, b, logits=True)
    assert cs.bits_equal(z[:, lo], z[:, hi])
    assert np.all(z[:, lo] > 50.0) and np.all(np.delete(z, (lo, hi), axis=1) < 1.0)
    assert np.all(pred == lo)
    one, zm = eng.classifier_ml_predict(np.arange(n), W, b, k=np.ones(n, dtype=np.int32), logits=True)
    assert cs.bits_equal(zm[:, lo], zm[:, hi])
    want = np.zeros((n, C), dtype=bool)
    want[:, lo] = True
    assert np.array_equal(one, want)
    want[:, hi] = True
    assert np.array_equal(eng.classifier_ml_predict(np.arange(n), W, b, k=np.full(n, 2)), want)


# E. softmax saturation
def test_softmax_saturated_logits_stay_finite_and_exact(engine_of):
    """b[c] = +-200: exp(z) is inf in float32 and exp(z - max) underflows to 0 for the cold classes; the max-subtracted form
    gives a finite loss and gradient.  With ONE hot class its probability is exactly 1 on every row and every other exactly 0:
    gb is an exact count over M"""
    M, d, C = 130, 8, 40
    eng = engine_of(d)
    rs = np.random.RandomState(78)
    nodes = cs.draw_nodes(rs, M)
    X = tables(d)[0][nodes]
    W = (0.05 * rs.randn(C, d)).astype(np.float32)
    hot, cold = [0, 7, 33, 39], [1, 8, 32, 38]
    y = rs.randint(0, C, size=M)
    y[0:40:2], y[1:40:2] = np.resize(hot, 20), np.resize(cold, 20)  # labels on both kinds
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(200.0))) and np.exp(np.float32(-190.0)) == 0
    for tag, hot_now in (("several hot classes", hot), ("one hot class", hot[2:3])):
        b = (0.5 * rs.randn(C)).astype(np.float32)
        b[cold] = -200.0
        b[hot_now] = 200.0
        r64 = ref.lossgrad(X, y, W, b, 0.0, np.float64)
        r32 = ref.lossgrad(X, y, W, b, 0.0, np.float32)
        got = eng.classifier_lossgrad(nodes, y, W, b, which=0, l2=0.0)
        assert np.isfinite(got["loss"]) and np.all(np.isfinite(got["gW"])) and np.all(np.isfinite(got["gb"]))
        compare("softmax saturation, " + tag, ("loss", "gW", "gb"), (got["loss"], got["gW"], got["gb"]), r64, r32)
    h = hot[2]
    n = np.bincount(y, minlength=C)
    assert 0 < n[h] < M and np.abs(X @ W.T).max() < 5.0  # (no logit comes within 190 of the hot one)
    for c in range(C):
        want = np.float32(M - n[c] if c == h else -n[c]) / np.float32(M)
        assert got["gb"][c] == want, (c, got["gb"][c], want)
