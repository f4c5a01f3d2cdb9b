"""The neighbour-sum sweep (gg_neighbor_sum, Engine.neighbor_sum), label spreading iterated on it (gg_label_spread,
Engine.label_spread) and the graph_nc results line on the device.

Three kinds of comparison (tests/support/label_spread_ref.py).  EXACT: inputs in {-1, 0, 1} and power-of-two scales against an int64
closed form -- every partial sum is representable, so any order of the adds gives the same bits and a leaked padding column or a
lost chunk would change an integer.  BIT CONTRACT: a node's row is the same bits whatever else was requested, and a fit of T
iterations equals T primitive calls composed on the host.  BAND: Gaussian inputs against float64 inside a bound derived in the test
from the inputs; each case prints its err / tol ("errtol ..." lines, collected in profiles/r22_label_spread_errtol.txt)."""
import ctypes

import numpy as np
import pytest

from tests.support import label_spread_ref as ref

pytestmark = pytest.mark.gpu

N_COLS = (1, 2, 3, 4, 5, 8, 31, 32, 33, 40, 64, 127, 128)  # every lanes-per-row instance (1 .. 32) and the ragged widths


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def engine_for(ga, n, edges=None):
    table = np.zeros((n, 4), np.float32)  # (the sweep reads no embedding)
    eng = ga.Engine(table, table)
    if edges is not None:
        eng.set_graph_csr(*ga.edges_to_csr(n, edges))
    return eng


@pytest.fixture(scope="module")
def hub(ga):
    """the graph with the probes and the two hubs, resident, with its pair set and degrees: shared, never changed"""
    n, edges, info = ref.hub_graph()
    src, dst = ref.pair_set(n, edges)
    deg = ref.degrees(n, src)
    assert ga.Engine.NEIGHBOR_SUM_CHUNK == ref.CHUNK
    assert deg[info["probes"]].tolist() == list(ref.LENGTHS) and deg[info["hub_a"]] == ref.HUB_A and deg[info["hub_b"]] == ref.HUB_B
    assert deg[info["isolated"]] == 0 and len(edges) > len(src) // 2  # (duplicates and self-loops are in the lists)
    eng = engine_for(ga, n, edges)
    assert eng.distinct_degrees().tolist() == deg.tolist()
    yield dict(n=n, src=src, dst=dst, deg=deg, eng=eng, **info)
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def exact_inputs(n, n_col, rs):
    """X in {-1, 0, 1}, scales signed powers of two 2^-3 .. 2^3, and the int64 closed form's pieces"""
    X = rs.randint(-1, 2, size=(n, n_col)).astype(np.int64)
    ki, ko = rs.randint(-3, 4, n), rs.randint(-3, 4, n)
    sign = rs.choice([-1.0, 1.0], n)
    return X, ki, sign, ko


def exact_ref(g, X, ki=None, sign=None, ko=None):
    """float64 of the exact result: the int64 sum of X * 2^(ki + 3) * sign, times 2^-3 and the out scale"""
    n = g["n"]
    Xi = X if ki is None else X * ((1 << (ki + 3)) * sign.astype(np.int64))[:, None]
    H = ref.neighbor_sum(n, g["src"], g["dst"], Xi).astype(np.float64)
    if ki is not None:
        H /= 8.0
    return H if ko is None else H * (2.0 ** ko)[:, None]


@pytest.mark.parametrize("n_col", N_COLS)
def test_neighbor_sum_is_exact_at_every_width(hub, n_col):
    g, rs = hub, np.random.RandomState(100 + n_col)
    eng, n = g["eng"], g["n"]
    X, ki, sign, ko = exact_inputs(n, n_col, rs)
    res = eng.neighbor_sum(X)
    assert res["out"].dtype == np.float32 and res["out"].shape == (n, n_col) and res["ms"] >= 0.0
    assert np.array_equal(res["out"].astype(np.float64), exact_ref(g, X)), "no scales"
    in_s, out_s = (sign * 2.0 ** ki).astype(np.float32), (2.0 ** ko).astype(np.float32)
    got = eng.neighbor_sum(X, in_scale=in_s, out_scale=out_s)["out"]
    assert np.array_equal(got.astype(np.float64), exact_ref(g, X, ki, sign, ko)), "both scales"
    got = eng.neighbor_sum(X, in_scale=in_s)["out"]
    assert np.array_equal(got.astype(np.float64), exact_ref(g, X, ki, sign)), "in_scale"
    assert not np.any(res["out"][g["isolated"]]) and not np.any(np.signbit(res["out"][g["isolated"]]))  # no neighbour: +0
    # NULL scales and scales of 1.0: the same bits
    ones = np.ones(n, np.float32)
    assert np.array_equal(bits(eng.neighbor_sum(X, in_scale=ones, out_scale=ones)["out"]), bits(res["out"]))


def test_chunk_edges_of_both_hubs(hub):
    """the entries at list positions 511, 512, 1023, 1024 (and the first and the last) as the ONLY nonzero rows: a chunk that
    drops its first or last entry, or a finishing step that skips a chunk, loses exactly one of them"""
    g = hub
    eng, n, C = g["eng"], g["n"], ref.CHUNK
    lists = {g["hub_a"]: g["a_list"], g["hub_b"]: np.arange(ref.HUB_B)}
    for h, lst in lists.items():
        assert np.array_equal(lst, g["dst"][g["src"] == h])  # (the sorted distinct list of the hub)
        pos = [0, C - 1, C, 2 * C - 1, 2 * C, 3 * C - 1, 3 * C, len(lst) - 1] + ([4 * C - 1, 4 * C] if len(lst) > 4 * C else [])
        X = np.zeros((n, 5), np.int64)
        X[lst[pos], 0] = 1
        X[lst[pos], 4] = 1 << np.arange(len(pos))  # (which of them arrived)
        for p in pos:  # one at a time, and all of them
            X1 = np.zeros((n, 5), np.int64)
            X1[lst[p], 2] = 1
            assert eng.neighbor_sum(X1, nodes=[h])["out"][0].tolist() == [0, 0, 1, 0, 0], p
        out = eng.neighbor_sum(X)["out"]
        assert np.array_equal(out.astype(np.float64), exact_ref(g, X))
        assert out[h].tolist() == [len(pos), 0, 0, 0, (1 << len(pos)) - 1]


def test_requests_do_not_change_a_nodes_bits(hub):
    g, rs = hub, np.random.RandomState(7)
    eng, n = g["eng"], g["n"]
    X = rs.standard_normal((n, 40)).astype(np.float32)
    in_s, out_s = (rs.standard_normal(n).astype(np.float32) for _ in range(2))
    full = eng.neighbor_sum(X, in_s, out_s)["out"]
    assert np.array_equal(bits(eng.neighbor_sum(X, in_s, out_s)["out"]), bits(full))  # a rerun
    perm = rs.permutation(n)
    assert np.array_equal(bits(eng.neighbor_sum(X, in_s, out_s, nodes=perm)["out"]), bits(full[perm]))  # None against a permutation
    special = np.array([g["hub_a"], g["hub_b"], g["isolated"]] + g["probes"].tolist())
    for m in (1, 63, 64, 65):
        nodes = np.concatenate([special, rs.randint(0, n, 65)])[:m] if m > 1 else np.array([g["hub_b"]])
        assert np.array_equal(bits(eng.neighbor_sum(X, in_s, out_s, nodes=nodes)["out"]), bits(full[nodes])), m  # a subset
    rep = np.array([g["hub_a"], 5, g["hub_a"], 5, g["probes"][9], g["hub_a"]])
    assert np.array_equal(bits(eng.neighbor_sum(X, in_s, out_s, nodes=rep)["out"]), bits(full[rep]))  # repeated ids (a hub among them)
    empty = eng.neighbor_sum(X, nodes=np.zeros(0, np.int64))
    assert empty["out"].shape == (0, 40)  # m = 0


def test_more_tasks_than_one_launch_has_wavefronts(ga):
    n, rs = 70000, np.random.RandomState(3)
    edges = rs.randint(0, n, size=(200000, 2)).astype(np.int32)
    src, dst = ref.pair_set(n, edges)
    eng = engine_for(ga, n, edges)
    X = rs.randint(-1, 2, size=(n, 8)).astype(np.int64)
    out = eng.neighbor_sum(X)["out"]
    assert np.array_equal(out.astype(np.int64), ref.neighbor_sum(n, src, dst, X))
    perm = rs.permutation(n)
    assert np.array_equal(bits(eng.neighbor_sum(X, nodes=perm)["out"]), bits(out[perm]))
    eng.close()


def test_a_new_graph_drops_the_plan(ga):
    """the second graph moves the hub to another node and shortens it: a kept plan would split the wrong node"""
    n, rs = 1500, np.random.RandomState(4)
    X = rs.randint(-1, 2, size=(n, 3)).astype(np.int64)
    eng = engine_for(ga, n)
    outs = []
    for hub_node, hub_deg in ((0, 1200), (7, 600), (0, 1200)):
        others = np.setdiff1d(np.arange(n), [hub_node])
        edges = np.concatenate([np.stack([np.full(hub_deg, hub_node), others[:hub_deg]], axis=1), rs.randint(0, n, size=(2000, 2))]).astype(np.int32)
        eng.set_graph_csr(*ga.edges_to_csr(n, edges))
        src, dst = ref.pair_set(n, edges)
        outs.append(eng.neighbor_sum(X)["out"])
        assert np.array_equal(outs[-1].astype(np.int64), ref.neighbor_sum(n, src, dst, X)), (hub_node, hub_deg)
        assert np.array_equal(eng.neighbor_sum(X, nodes=[hub_node, 3])["out"], outs[-1][[hub_node, 3]])
    assert not np.array_equal(outs[0][0], outs[1][0])
    eng.close()


@pytest.mark.parametrize("n_col", (1, 5, 40, 128))
def test_neighbor_sum_gaussian_inside_the_band(hub, n_col):
    """tol[v, c] = (deg(v) + 2) 2^-24 |out_scale[v]| sum_w |in_scale[w] X[w, c]|: deg products, deg - 1 adds in any order and the
    final multiply, each within one unit roundoff of a partial result that the sum of the absolute terms bounds"""
    g, rs = hub, np.random.RandomState(200 + n_col)
    eng, n = g["eng"], g["n"]
    X = rs.standard_normal((n, n_col)).astype(np.float32)
    in_s, out_s = (rs.standard_normal(n).astype(np.float32) for _ in range(2))
    got = eng.neighbor_sum(X, in_s, out_s)["out"].astype(np.float64)
    want = ref.neighbor_sum(n, g["src"], g["dst"], X.astype(np.float64), in_s.astype(np.float64), out_s.astype(np.float64))
    tol = (g["deg"] + 2.0)[:, None] * ref.U * ref.neighbor_sum(n, g["src"], g["dst"], np.abs(X.astype(np.float64)), np.abs(in_s.astype(np.float64)),
                                                                np.abs(out_s.astype(np.float64)))
    err = np.abs(got - want)
    ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)))
    print("errtol case=neighbor_sum_gaussian n_col=%d max_err=%.3e max_err_over_tol=%.4f" % (n_col, err.max(), ratio))
    assert np.all(err <= tol)
    assert np.all(got[tol[:, 0] == 0] == 0)


def train_set(g, n_class, multi, rs):
    n = g["n"]
    train = np.sort(np.concatenate([rs.permutation(g["pool"])[:400], [g["hub_a"], g["probes"][7]]]))
    if multi:
        Y = rs.random_sample((len(train), n_class)) < min(0.5, 3.0 / n_class)
        Y[np.arange(len(train)), rs.randint(0, n_class, len(train))] = True
        Y[0, n_class - 1] = True  # (the last bit of the last word)
        return train, Y, Y
    y = rs.randint(0, n_class, len(train))
    y[0] = n_class - 1
    Y = np.zeros((len(train), n_class), bool)
    Y[np.arange(len(train)), y] = True
    return train, y, Y


@pytest.mark.parametrize("multi", (False, True))
@pytest.mark.parametrize("n_class", (3, 40, 128))
def test_label_spread_equals_the_composed_primitive(ga, hub, n_class, multi):
    """iters = T against T neighbor_sum(in_scale = s) calls with numpy float32 a * H + base on the host, bit for bit, on the graph
    with the hubs (the finishing step's epilogue too)"""
    from graphgan_amd.evaluation import label_propagation as lprop
    g, rs = hub, np.random.RandomState(300 + n_class + multi)
    eng, n, alpha = g["eng"], g["n"], 0.9
    train, labels, Y = train_set(g, n_class, multi, rs)
    s, a, b = lprop.spread_coefficients(g["deg"], alpha)
    assert s.dtype == a.dtype == np.float32 and isinstance(b, np.float32)
    assert np.array_equal(bits(s), bits(ref.coefficients(g["deg"], alpha)[0])) and np.array_equal(bits(a), bits(ref.coefficients(g["deg"], alpha)[1]))
    Y0 = ref.one_hot(n, train, Y).astype(np.float32)
    base = np.where(Y0 != 0, b, np.float32(0)).astype(np.float32)
    F, composed = Y0, {}
    for t in range(1, 8):
        H = eng.neighbor_sum(F, in_scale=s)["out"]
        F = a[:, None] * H + base
        assert F.dtype == np.float32
        composed[t] = F
    for T in (1, 2, 7):
        res = eng.label_spread(train, labels, n_class, alpha=alpha, iters=T)
        assert res["F"].dtype == np.float32 and res["F"].shape == (n, n_class)
        assert np.array_equal(bits(res["F"]), bits(composed[T])), T
        prev = composed[T - 1] if T > 1 else Y0
        assert np.float32(res["delta"]) == np.max(np.abs(composed[T] - prev)), T  # fp32 subtraction, an order-independent maximum
    sub = np.array([g["hub_b"], g["isolated"], 0, g["hub_b"], g["probes"][6]])
    res = eng.label_spread(train, labels, n_class, alpha=alpha, iters=7, out_nodes=sub)
    assert np.array_equal(bits(res["F"]), bits(composed[7][sub]))
    if multi:  # label lists are the same labels
        lists = [np.flatnonzero(r).tolist() for r in Y]
        assert np.array_equal(bits(eng.label_spread(train, lists, n_class, alpha=alpha, iters=2)["F"]), bits(composed[2]))


@pytest.fixture(scope="module")
def ring(ga):
    n = 257
    edges = ref.circulant(n)
    eng = engine_for(ga, n, edges)
    yield dict(n=n, edges=edges, eng=eng)
    eng.close()


def test_label_spread_is_exact_on_the_circulant_graph(ring):
    """4-regular: s = 1/2, a = alpha / 2 = 1/4, b = 1/2.  Every value is a dyadic number of at most 3T + 3 bits, so while
    3T + 3 <= 24 every order of the adds is exact and F_T equals the float64 host evaluator bit for bit"""
    from graphgan_amd.evaluation import label_propagation as lprop
    from graphgan_amd.evaluation import link_heuristics as lheur
    n, eng, rs = ring["n"], ring["eng"], np.random.RandomState(1)
    train = np.sort(rs.permutation(n)[:n // 2])
    y = rs.randint(0, 5, len(train))
    ptr, adj = lheur.set_adjacency(ring["edges"], n)
    assert np.all(np.diff(ptr) == 4)
    src, dst = ref.pair_set(n, ring["edges"])
    Y = np.zeros((len(train), 5), bool)
    Y[np.arange(len(train)), y] = True
    for T in range(1, 7):
        dev = eng.label_spread(train, y, 5, alpha=0.5, iters=T)
        host = lprop.host_label_spread(ptr, adj, train, y, 5, alpha=0.5, iters=T)
        assert np.array_equal(dev["F"].astype(np.float64), host["F"]), T
        assert np.array_equal(host["F"], ref.label_spread(n, src, dst, ref.one_hot(n, train, Y), 0.5, T)), T
        assert dev["delta"] == host["delta"] and dev["delta"] > 0, T


@pytest.mark.parametrize("multilabel", (False, True))
def test_graph_nc_line_with_an_engine_is_string_equal_to_the_host_evaluators(ring, tmp_path, multilabel):
    from graphgan_amd.evaluation import label_propagation as lprop
    n, rs = ring["n"], np.random.RandomState(2)
    train_file, labels_file = str(tmp_path / "train.txt"), str(tmp_path / "labels.txt")
    np.savetxt(train_file, ring["edges"], fmt="%d")
    nodes = np.sort(rs.permutation(n)[:200])
    with open(labels_file, "w") as f:
        for v in nodes.tolist():
            labs = sorted(set(rs.randint(0, 5, rs.randint(1, 4)).tolist())) if multilabel else [int(rs.randint(0, 5))]
            f.write("%d %s\n" % (v, " ".join(str(10 * c) for c in labs)))
    kw = dict(train_ratio=0.5, seed=3, alpha=0.5, iters=6, multilabel=multilabel)
    dev = lprop.LabelSpreadEval(train_file, labels_file, n, engine=ring["eng"], **kw).eval_label_spread()
    host = lprop.LabelSpreadEval(train_file, labels_file, n, **kw).eval_label_spread()
    assert lprop.format_results(dev, multilabel) == lprop.format_results(host, multilabel)
    line = lprop.format_results(dev, multilabel)
    assert line.startswith("graph_nc:acc=") and ("micro_f1=" in line) == multilabel and line.endswith(" unreached=0 n_train=100 n_test=100\n")
    assert " alpha=0.5 iters=6 delta=" in line and dev["delta"] > 0


def test_delta_is_the_largest_change_of_the_last_iteration(hub, ga):
    g, rs = hub, np.random.RandomState(9)
    eng, n = g["eng"], g["n"]
    train, y, _ = train_set(g, 7, False, rs)
    for T in (2, 5):
        now, before = eng.label_spread(train, y, 7, iters=T), eng.label_spread(train, y, 7, iters=T - 1)
        assert np.float32(now["delta"]) == np.max(np.abs(now["F"] - before["F"])) and now["delta"] > 0
    # a graph whose lists hold self-loops only: no node has a neighbour, F_1 = b Y0 = F_2
    m = 300
    loops = np.repeat(np.arange(m), 2).reshape(-1, 2).astype(np.int32)
    e2 = engine_for(ga, m, loops)
    assert not e2.distinct_degrees().any()
    tr, lab = np.arange(0, m, 3), np.arange(0, m, 3) % 4
    two = e2.label_spread(tr, lab, 4, alpha=0.9, iters=2)
    assert two["delta"] == 0.0 and np.array_equal(np.flatnonzero(two["F"].any(axis=1)), tr)
    assert np.array_equal(np.unique(two["F"]), np.array([0, np.float32(1.0 - 0.9)], np.float32))
    assert np.float32(e2.label_spread(tr, lab, 4, alpha=0.9, iters=1)["delta"]) == np.float32(1) - np.float32(1.0 - 0.9)  # |b - 1|
    e2.close()


@pytest.mark.parametrize("seed", (0, 1))
def test_planted_partition_inside_the_recursions_band(ga, seed):
    from graphgan_amd.evaluation import label_propagation as lprop
    from graphgan_amd.evaluation import link_heuristics as lheur
    n = 256
    edges, lab, train, test = ref.planted_partition(seed)
    assert len(train) == 26 and len(test) == 230
    src, dst = ref.pair_set(n, edges)
    Y = np.zeros((26, 4), bool)
    Y[np.arange(26), lab[train]] = True
    F64, E = ref.label_spread(n, src, dst, ref.one_hot(n, train, Y), 0.9, 30, band=True)
    ptr, adj = lheur.set_adjacency(edges, n)
    host = lprop.host_label_spread(ptr, adj, train, lab[train], 4, alpha=0.9, iters=30)["F"]
    assert np.max(np.abs(host - F64)) <= 1e-13  # (the package's float64 run: another order of the same sums)
    eng = engine_for(ga, n, edges)
    dev = eng.label_spread(train, lab[train], 4, alpha=0.9, iters=30)
    eng.close()
    err = np.abs(dev["F"].astype(np.float64) - host)
    print("errtol case=planted_partition seed=%d max_err=%.3e max_err_over_band=%.4f" % (seed, err.max(), float(np.max(np.where(E > 0, err / np.where(E > 0, E, 1.0), 0.0)))))
    assert np.all(err <= E)
    top = np.sort(host[test], axis=1)
    decided = (top[:, -1] - top[:, -2]) > 2 * E[test].max(axis=1)
    assert np.sum(~decided) <= 0.01 * len(test)
    p_dev, _ = lprop.predict(dev["F"][test], Y)
    p_host, _ = lprop.predict(host[test], Y)
    assert np.array_equal(p_dev[decided], p_host[decided])
    print("planted partition seed=%d: accuracy %.4f (host %.4f), %d of %d test nodes left out" % (
        seed, np.mean(p_dev == lab[test]), np.mean(p_host == lab[test]), int(np.sum(~decided)), len(test)))


def test_unreached_nodes_fall_back_to_the_most_frequent_label(ga):
    """two rings; only the first holds training labels, so no label ever reaches the second: its rows stay exactly zero"""
    from graphgan_amd.evaluation import label_propagation as lprop
    n = 60
    edges = np.array([(i, (i + 1) % 30) for i in range(30)] + [(30 + i, 30 + (i + 1) % 30) for i in range(30)], np.int32)
    eng = engine_for(ga, n, edges)
    train, y = np.array([0, 5, 10, 15, 20]), np.array([2, 1, 2, 1, 0])  # labels 1 and 2 tie in frequency: the lower wins
    test = np.array([3, 29, 31, 45, 59])
    res = eng.label_spread(train, y, 3, iters=40, out_nodes=test)
    eng.close()
    assert not res["F"][2:].any() and res["F"][:2].all()
    pred, unreached = lprop.predict(res["F"], lprop.label_matrix("t", y, 5, 3))
    assert unreached == 3 and pred[2:].tolist() == [1, 1, 1] and pred[0] == int(np.argmax(res["F"][0]))


def test_refusals_name_the_function_and_the_value(ga):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    X = np.zeros((n, 3), np.float32)
    for call, name in ((lambda: eng.neighbor_sum(X), "gg_neighbor_sum"),):  # no graph (label_spread asks for the degrees first)
        with pytest.raises(ga.GraphGANHipError) as ei:
            call()
        assert ei.value.code == ga.GG_EINVAL and "%s: needs the training graph (gg_set_graph_csr)" % name in str(ei.value)
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tr, tb = np.array([1, 2], np.int32), np.array([[1], [2]], np.uint32)
    sa, Fo, dl = np.ones(n, np.float32), np.zeros((n, 3), np.float32), ctypes.c_float(-1.0)

    def raw_ls(tr=tr, tb=tb, m_train=2, C=3, alpha=0.9, iters=2, s=sa, a=sa, on=None, m_out=0, F=Fo, ctx=None):
        return lambda: _lib.check(L.gg_label_spread(eng._ctx, p(tr), p(tb), m_train, C, alpha, iters, p(s), p(a), p(on), m_out, p(F), ctypes.byref(dl), None),
                                  eng._ctx)

    with pytest.raises(ga.GraphGANHipError) as ei:
        raw_ls()()
    assert "gg_label_spread: needs the training graph (gg_set_graph_csr)" in str(ei.value)
    ring_edges = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int32)
    eng.set_graph_csr(*ga.edges_to_csr(n, ring_edges))

    def refused(call, text, exc=None):
        with pytest.raises(exc or ga.GraphGANHipError) as ei:
            call()
        assert text in str(ei.value), str(ei.value)
        if exc is None:
            assert ei.value.code == ga.GG_EINVAL

    # through Engine: the Python layer refuses the same things, before the ABI
    V = ValueError
    refused(lambda: eng.neighbor_sum(np.zeros((n, 129), np.float32)), "neighbor_sum: n_col = 129 outside [1, 128]", V)
    refused(lambda: eng.neighbor_sum(np.zeros((n, 0), np.float32)), "neighbor_sum: n_col = 0 outside [1, 128]", V)
    refused(lambda: eng.neighbor_sum(np.zeros((n + 1, 3), np.float32)), "neighbor_sum: X must be a float matrix [50, n_col]", V)
    refused(lambda: eng.neighbor_sum(X, nodes=[0, 3, 50]), "neighbor_sum: nodes[2] = 50 out of range [0, 50)", V)
    refused(lambda: eng.neighbor_sum(X, nodes=[-1, 3]), "neighbor_sum: nodes[0] = -1 out of range [0, 50)", V)
    refused(lambda: eng.neighbor_sum(X, in_scale=np.ones(n + 1)), "neighbor_sum: in_scale must be a float array [50]", V)
    refused(lambda: eng.neighbor_sum(X, out_scale=np.ones((n, 1))), "neighbor_sum: out_scale must be a float array [50]", V)
    ls = eng.label_spread
    refused(lambda: ls([1, 2], [0, 1], 129), "label_spread: n_class = 129 outside [1, 128]", V)
    refused(lambda: ls([1, 2], [0, 1], 0), "label_spread: n_class = 0 outside [1, 128]", V)
    refused(lambda: ls([1, 50], [0, 1], 3), "label_spread: train_nodes[1] = 50 out of range [0, 50)", V)
    refused(lambda: ls([1, 2, 1], [0, 1, 2], 3), "label_spread: train_nodes[2] = 1 repeats train_nodes[0]", V)
    refused(lambda: ls([1, 2], [0, 1], 3, alpha=1.0), "label_spread: alpha = 1.0 outside (0, 1)", V)
    refused(lambda: ls([1, 2], [0, 1], 3, alpha=0.0), "label_spread: alpha = 0.0 outside (0, 1)", V)
    refused(lambda: ls([1, 2], [0, 1], 3, iters=0), "label_spread: iters = 0 is below 1", V)
    refused(lambda: ls([1, 2], [0, 3], 3), "label_spread: label_bits row 1 has a bit set at a position >= n_class = 3", V)
    refused(lambda: ls([1, 2], [[0], [1, 3]], 3), "label_spread: label_bits row 1 has a bit set at a position >= n_class = 3", V)
    refused(lambda: ls([1, 2], [0, 1], 3, out_nodes=[0, -2]), "label_spread: out_nodes[1] = -2 out of range [0, 50)", V)
    refused(lambda: ls([1, 2], np.zeros((2, 4), bool), 3), "label_spread: labels must be", V)

    # through the C ABI
    out = np.zeros((n, 3), np.float32)
    nodes2 = np.array([0, 7], np.int32)

    def raw_ns(X=X, n_col=3, in_s=None, out_s=None, nodes=nodes2, m=2, out=out):
        return lambda: _lib.check(L.gg_neighbor_sum(eng._ctx, p(X), n_col, p(in_s), p(out_s), p(nodes), m, p(out), None), eng._ctx)

    raw_ns()()  # (kernel_ms may be NULL)
    for bad in (dict(X=None), dict(out=None)):
        refused(raw_ns(**bad), "gg_neighbor_sum: X and out must not be NULL")
    refused(raw_ns(m=-1), "gg_neighbor_sum: m = -1 is negative")
    refused(raw_ns(n_col=0), "gg_neighbor_sum: n_col = 0 outside [1, 128]")
    refused(raw_ns(n_col=129), "gg_neighbor_sum: n_col = 129 outside [1, 128]")
    refused(raw_ns(nodes=np.array([0, 50], np.int32)), "gg_neighbor_sum: nodes[1] = 50 out of range [0, 50)")
    raw_ns(X=None, out=None, m=0)()  # m == 0 succeeds and touches nothing
    for bad in (dict(tr=None), dict(tb=None)):
        refused(raw_ls(**bad), "gg_label_spread: train_nodes and label_bits must not be NULL")
    for bad in (dict(s=None), dict(a=None)):
        refused(raw_ls(**bad), "gg_label_spread: s and a must not be NULL")
    refused(raw_ls(F=None), "gg_label_spread: F_out must not be NULL")
    refused(raw_ls(m_train=-1), "gg_label_spread: m_train = -1 is negative")
    refused(raw_ls(on=nodes2, m_out=-2), "gg_label_spread: m_out = -2 is negative")
    refused(raw_ls(C=0), "gg_label_spread: n_class = 0 outside [1, 128]")
    refused(raw_ls(C=129), "gg_label_spread: n_class = 129 outside [1, 128]")
    refused(raw_ls(alpha=1.0), "gg_label_spread: alpha = 1 outside (0, 1)")
    refused(raw_ls(alpha=-0.5), "gg_label_spread: alpha = -0.5 outside (0, 1)")
    refused(raw_ls(iters=0), "gg_label_spread: iters = 0 is below 1")
    refused(raw_ls(tr=np.array([1, 50], np.int32)), "gg_label_spread: train_nodes[1] = 50 out of range [0, 50)")
    refused(raw_ls(tr=np.array([4, 4], np.int32)), "gg_label_spread: train_nodes[1] = 4 repeats train_nodes[0]")
    refused(raw_ls(tb=np.array([[1], [8]], np.uint32)), "gg_label_spread: label_bits row 1 has a bit set at a position >= n_class = 3")
    refused(raw_ls(on=np.array([0, 99], np.int32), m_out=2), "gg_label_spread: out_nodes[1] = 99 out of range [0, 50)")
    # m_out = 0: the fit runs, no row is written, delta comes back
    from graphgan_amd.evaluation import label_propagation as lprop
    s_c, a_c, _ = lprop.spread_coefficients(eng.distinct_degrees(), 0.9)
    Fo[:] = -7.0
    raw_ls(on=nodes2, m_out=0, F=None, s=s_c, a=a_c)()
    assert dl.value > 0.0 and np.all(Fo == -7.0)
    res = eng.label_spread([1, 2], [0, 1], 3, iters=2, out_nodes=np.zeros(0, np.int64))
    assert res["F"].shape == (0, 3) and res["delta"] == dl.value
    res = eng.neighbor_sum(np.ones((n, 3), np.float32), nodes=[0, 7])  # the engine stays usable
    assert res["out"].tolist() == [[2.0] * 3] * 2
    eng.close()
