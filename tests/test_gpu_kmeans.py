"""k-means on the device (graphgan_amd/csrc/kmeans.hip: gg_kmeans_step / gg_kmeans_fit, Engine.kmeans_*) and the NodeClusterEval
evaluator on an engine, at the smallest shapes at which the sweep can go wrong (tests/support/classifier_shapes.py restates the
launch plan the sweep shares with the classifier's, graphgan_amd/csrc/row_tiles.h, row_tile_plan: every (CT, DT) instance, ragged edges, more tiles than workgroups).

Three kinds of comparison.  EXACT: on tables of {-1, 0, 1} with table rows as centroids every dot product, h_c (a multiple of
1/2, at most 128), score, dist2, sum (|value| < 2^24) and the inertia is an integer or half-integer, exact in float32 in any
order, so the outputs equal an int64 closed form (tests/support/kmeans_ref.py, int_step) -- a dropped or doubled row, a stale
tile or a partial summed twice changes an integer.  BITWISE: the fit against gg_kmeans_step (the same kernels on the same grid).
DERIVED: Gaussian tables against float64 inside the bands of kmeans_ref (4 (d + 2) 2^-24 (|x|^2 + max |c|^2) per row for the
argmin and dist2; count_c 2^-24 sum_{i in c} |x_ij| per entry of a float32 sum of count_c terms).

Set GG_KMEANS_ERRTOL to a path to get the err / tol of every derived case appended there."""
import ctypes
import os
import types

import numpy as np
import pytest

from tests.support import classifier_shapes as cs
from tests.support import kmeans_ref as kr

pytestmark = pytest.mark.gpu

U = kr.U


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


_tables = {}


def tables(d, kind):
    if (d, kind) not in _tables:
        if kind == "int":
            _tables[(d, kind)] = cs.int_tables(d)
        else:
            rs = np.random.RandomState(100 + d)
            _tables[(d, kind)] = ((0.3 * rs.randn(cs.N_TABLE, d)).astype(np.float32), (0.3 * rs.randn(cs.N_TABLE, d) + 0.05).astype(np.float32))
    return _tables[(d, kind)]


_engines = {}
MAX_ENGINES = 6  # (the cases are sorted by d: a d is finished before its engine becomes the oldest)


@pytest.fixture(scope="module")
def engine_of(ga):
    def get(d, kind):
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


def report(tag, err, tol):
    ratio = float(np.max(err / np.maximum(tol, 1e-300))) if np.size(err) else 0.0
    line = "%s: err/tol %.4g" % (tag, ratio)
    print(line)
    path = os.environ.get("GG_KMEANS_ERRTOL")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    return ratio


# ---- 1. exact row accounting on integer tables
def exact_leg(engine_of, M, d, k, seed, which=0, twin=False):
    eng = engine_of(d, "int")
    rs = np.random.RandomState(seed)
    nodes = cs.draw_nodes(rs, M)
    ids = rs.randint(0, cs.N_TABLE, size=k)
    if twin:
        ids[-1] = ids[0]  # two identical centroids: the higher one gets nothing
    T = tables(d, "int")[which]
    want = kr.int_step(T[nodes], T[ids])
    by_id = eng.kmeans_step(nodes, centroid_nodes=ids, which=which)
    by_value = eng.kmeans_step(nodes, centroids=T[ids], which=which)
    tag = "exact (M %d, d %d, k %d)" % (M, d, k)
    for key in ("assign", "counts"):
        assert np.array_equal(by_id[key], by_value[key]), (tag, key)
    for key in ("dist2", "sums"):
        assert cs.bits_equal(by_id[key], by_value[key]), (tag, key)
    assert by_id["inertia"] == by_value["inertia"]
    bad = np.flatnonzero(by_id["assign"] != want["assign"])
    assert len(bad) == 0, (tag, "assign", bad[:8], by_id["assign"][bad[:8]], want["assign"][bad[:8]])
    assert np.array_equal(by_id["dist2"].astype(np.float64), want["dist2"]), (tag, "dist2")
    assert np.array_equal(by_id["counts"], want["counts"]), (tag, "counts", by_id["counts"], want["counts"])
    bad = np.argwhere(by_id["sums"].astype(np.float64) != want["sums"])
    assert len(bad) == 0, (tag, "sums", bad[:8])
    assert by_id["inertia"] == float(want["inertia"]), (tag, "inertia", by_id["inertia"], want["inertia"])
    assert int(by_id["counts"].sum()) == M
    alone = eng.kmeans_step(nodes, centroid_nodes=ids, which=which, sums=False)  # the assign-only sweep: the same bits
    assert np.array_equal(alone["assign"], by_id["assign"]) and cs.bits_equal(alone["dist2"], by_id["dist2"]) and alone["inertia"] == by_id["inertia"]
    if twin:
        assert by_id["counts"][-1] == 0 and not by_id["sums"][-1].any()
    return want["ties"]


def test_cases_reach_all_32_instances():
    reached = {(cs.sweep_plan(k, cs.ld_of(d))["CT"], cs.sweep_plan(k, cs.ld_of(d))["DT"]) for k, d in cs.INSTANCE_CASES}
    assert reached == {(CT, DT) for CT in range(1, 5) for DT in range(1, 9)}


@pytest.mark.parametrize("k,d", sorted(cs.INSTANCE_CASES + cs.RAGGED_CASES, key=lambda kd: (kd[1], kd[0])))
def test_step_exact_on_every_instance(engine_of, k, d):
    ties = exact_leg(engine_of, cs.M_SMALL, d, k, 11 * k + d, which=k & 1)
    print("ties on %.0f %% of the rows" % (100 * ties))


@pytest.mark.parametrize("M,d,k", [(1, 8, 2), (63, 33, 33), (64, 33, 33), (65, 33, 33), (cs.M_SMALL, 8, 1), (cs.M_SMALL, 161, 1),
                                   (3, 33, 128)])
def test_step_exact_at_the_edges(engine_of, M, d, k):
    """one row, a tile less one, a full tile, a tile plus one; k = 1 (seeding calls it); fewer rows than clusters"""
    exact_leg(engine_of, M, d, k, 7 * M + k + d)


@pytest.mark.parametrize("k,d", [(40, 8), (97, 129)])
def test_step_exact_with_two_identical_centroids(engine_of, k, d):
    ties = exact_leg(engine_of, cs.M_SMALL, d, k, 5 * k + d, twin=True)
    assert ties > 0  # (every row ties between the twins at least where they are the nearest)


@pytest.mark.parametrize("M,d,k", sorted(cs.MULTI_TILE_CASES, key=lambda c: (c[1], c[0])))
def test_step_exact_with_more_tiles_than_workgroups(engine_of, M, d, k):
    assert cs.cdiv(M, cs.NC_RT) > cs.NC_MAX_GRID
    exact_leg(engine_of, M, d, k, M + 11 * k + d, which=1)


# ---- 2. gg_kmeans_step against float64 on Gaussian tables
GAUSS_CASES = sorted([(d, k) for k, d in cs.RAGGED_CASES] + [(128, 40), (256, 128)])  # (d, k)


def check_step_against_float64(tag, X, C, got, k):
    """the derived checks of one sweep: rows X float32 [M, d], centroids C float32 [k, d]"""
    M, d = X.shape
    D = kr.f64_dist(X, C)
    band = kr.band(X, C)
    a = got["assign"].astype(np.int64)
    assert a.min() >= 0 and a.max() < k
    own = D[np.arange(M), a]
    r1 = report(tag + " argmin", own - D.min(axis=1), band)
    r2 = report(tag + " dist2", np.abs(got["dist2"].astype(np.float64) - own), band)
    assert r1 <= 1.0 and r2 <= 1.0, (tag, r1, r2)
    print("%s: %d of %d rows differ from the float64 argmin" % (tag, int((a != D.argmin(axis=1)).sum()), M))
    assert got["inertia"] == pytest.approx(float(got["dist2"].astype(np.float64).sum()), rel=1e-12)
    if "counts" in got:
        assert np.array_equal(got["counts"], np.bincount(a, minlength=k))
        X64 = X.astype(np.float64)
        want, mass = np.zeros((k, d)), np.zeros((k, d))
        np.add.at(want, a, X64)
        np.add.at(mass, a, np.abs(X64))
        tol = got["counts"][:, None] * U * mass
        err = np.abs(got["sums"].astype(np.float64) - want)
        r3 = report(tag + " sums", err[tol > 0], tol[tol > 0])
        assert r3 <= 1.0 and not err[tol == 0].any(), (tag, r3)


@pytest.mark.parametrize("d,k", GAUSS_CASES)
def test_step_against_float64(engine_of, d, k):
    M = 1000
    eng = engine_of(d, "rand")
    rs = np.random.RandomState(31 * d + k)
    nodes = cs.draw_nodes(rs, M)
    for which in (0, 1):
        T = tables(d, "rand")[which]
        C = (T[rs.randint(0, cs.N_TABLE, size=k)] + 0.1 * rs.randn(k, d)).astype(np.float32)
        got = eng.kmeans_step(nodes, centroids=C, which=which)
        check_step_against_float64("step (M %d, d %d, k %d) which %d" % (M, d, k, which), T[nodes], C, got, k)


# ---- 3. gg_kmeans_fit
_blob_engines = {}


@pytest.fixture(scope="module")
def blob_engine(ga):
    """engine on a blob table: generator = the blobs, discriminator = the same rows in reverse order"""
    def get(shape):
        if shape not in _blob_engines:
            X, labels, first = kr.blobs(*shape)
            _blob_engines[shape] = (ga.Engine(X, X[::-1].copy()), X, labels, first)
        return _blob_engines[shape]
    yield get
    for e in _blob_engines.values():
        e[0].close()
    _blob_engines.clear()


def sum_tol(X, assign, k):
    """count_c 2^-24 sum_{i in c} |x_ij| -> float64 [k, d]"""
    mass = np.zeros((k, X.shape[1]))
    np.add.at(mass, assign, np.abs(X.astype(np.float64)))
    return np.bincount(assign, minlength=k)[:, None] * U * mass


@pytest.mark.parametrize("shape", kr.BLOB_SHAPES_GPU)
def test_fit_from_a_good_start(blob_engine, shape):
    """the reference's smallest margin is far above one band on these inputs (asserted): no float32 result can flip"""
    k, d, per = shape
    eng, X, labels, first = blob_engine(shape)
    nodes = np.arange(len(X))
    D = np.sort(kr.f64_dist(X, X[first]), axis=1)
    if k > 1:
        assert ((D[:, 1] - D[:, 0]) > 1e4 * kr.band(X, X[first])).all()
    res = eng.kmeans_fit(nodes, k, init=first, max_iters=100)
    assert res["iters"] == 2 and res["converged"] is True and res["inertia"].shape == (2,)
    assert np.array_equal(res["assign"], labels) and res["counts"].tolist() == [per] * k
    means = np.stack([X[labels == c].astype(np.float64).mean(axis=0) for c in range(k)])
    tol = sum_tol(X, labels, k) / per + U * np.abs(means)  # the sum bound over the count, and the division's rounding
    assert report("fit good start %r centroids" % (shape,), np.abs(res["centroids"].astype(np.float64) - means), tol) <= 1.0
    assert res["inertia"][1] <= res["inertia"][0]
    by_value = eng.kmeans_fit(nodes, init=X[first], max_iters=100)  # the start as values: the same bits
    assert cs.bits_equal(by_value["centroids"], res["centroids"]) and np.array_equal(by_value["inertia"], res["inertia"])


def check_consistent(eng, nodes, res, which=0):
    """(c): gg_kmeans_step at the returned centroids reproduces the returned state bit for bit"""
    step = eng.kmeans_step(nodes, centroids=res["centroids"], which=which)
    assert np.array_equal(step["assign"], res["assign"]) and cs.bits_equal(step["dist2"], res["dist2"])
    assert np.array_equal(step["counts"], res["counts"]) and step["inertia"] == res["inertia"][-1]
    return step


@pytest.mark.parametrize("shape", kr.BLOB_SHAPES_GPU)
def test_fit_chain_and_returned_state_from_a_bad_start(blob_engine, shape):
    """(b) + (c): cluster k - 1 starts on a second point of blob 0, so the float64 margins fall below one band and no trajectory
    comparison is meaningful: instead every update is checked against the sweep before it, bit for bit"""
    k, d, per = shape
    eng, X, labels, first = blob_engine(shape)
    nodes = np.arange(len(X))
    start = kr.bad_start(labels, first)
    fits = {T: eng.kmeans_fit(nodes, k, init=start, max_iters=T) for T in range(1, 6)}
    assert fits[1]["iters"] == 1 and not fits[1]["converged"] and cs.bits_equal(fits[1]["centroids"], X[start])  # no update at max_iters
    for T in range(1, 6):
        res = fits[T]
        assert res["iters"] <= T and res["inertia"].shape == (res["iters"],) and (res["converged"] or res["iters"] == T)
        step = check_consistent(eng, nodes, res)
        if T < 5 and not res["converged"]:
            want = kr.update_from_step(step, res["centroids"])
            assert cs.bits_equal(fits[T + 1]["centroids"], want), (shape, T)
            assert np.array_equal(fits[T + 1]["inertia"][:T], res["inertia"])
        if res["converged"]:  # a fixed point of the update
            assert cs.bits_equal(kr.update_from_step(step, res["centroids"]), res["centroids"])
    full = eng.kmeans_fit(nodes, k, init=start, max_iters=100)
    check_consistent(eng, nodes, full)
    assert full["converged"] and full["iters"] < 100
    # The inertia is non-increasing within the dist2 bands summed.  Every centroid is a row or a mean of rows, so |c|^2 <= max |x|^2
    # and S = sum_i band_i(X, X) covers every sweep.  True J(C', a') <= J(C', a_float64) + S (the argmin band) <= J(C', a) + S
    # <= J(C, a) + S (the mean minimises), and each reported inertia is within S of its true value: 3 S in all.
    slack = 3.0 * float(kr.band(X, X).sum())
    assert (np.diff(full["inertia"]) <= slack).all(), (full["inertia"], slack)
    assert int(full["counts"].sum()) == len(X) and np.array_equal(full["counts"], np.bincount(full["assign"], minlength=k))


def test_fit_is_deterministic_and_honours_which(blob_engine):
    shape = (5, 16, 60)
    eng, X, labels, first = blob_engine(shape)
    nodes = cs.draw_nodes(np.random.RandomState(3), 250) % len(X)
    start = X[kr.bad_start(labels, first)]
    one, two = (eng.kmeans_fit(nodes, init=start, max_iters=100) for _ in range(2))
    for key in ("centroids", "dist2"):
        assert cs.bits_equal(one[key], two[key]), key
    for key in ("assign", "counts", "inertia"):
        assert np.array_equal(one[key], two[key]), key
    assert (one["iters"], one["converged"]) == (two["iters"], two["converged"])
    other = eng.kmeans_fit(nodes, init=start, max_iters=100, which=1)  # table 1 holds the rows in reverse order
    host = eng.kmeans_fit(len(X) - 1 - nodes, init=start, max_iters=100, which=0)
    assert np.array_equal(other["assign"], host["assign"]) and cs.bits_equal(other["centroids"], host["centroids"])
    assert not np.array_equal(other["assign"], one["assign"])
    check_consistent(eng, nodes, other, which=1)


def test_fit_reports_an_empty_cluster_and_keeps_its_centroid(blob_engine):
    shape = (5, 16, 60)
    eng, X, labels, first = blob_engine(shape)
    nodes = np.arange(len(X))
    far = np.full((1, 16), 100.0 + 1.0 / 3, dtype=np.float32)
    start = np.concatenate([X[first], far])
    res = eng.kmeans_fit(nodes, 6, init=start, max_iters=100)
    assert res["converged"] and res["iters"] == 2 and res["counts"].tolist() == [60] * 5 + [0]
    assert cs.bits_equal(res["centroids"][5], far[0]) and np.array_equal(res["assign"], labels)
    twin = X[first].copy()
    twin[4] = twin[1]  # identical centroids: the higher index gets no row in the sweep
    res = eng.kmeans_fit(nodes, init=twin, max_iters=1)
    assert res["counts"][4] == 0 and (res["counts"][:4] > 0).all() and cs.bits_equal(res["centroids"], twin)


def test_argument_errors_name_the_limit(ga, blob_engine):
    eng, X, _, _ = blob_engine((5, 16, 60))
    lib, ctx = ga._lib.lib, eng._ctx
    n = len(X)
    nodes = np.arange(10, dtype=np.int32)
    cen = np.zeros((129, 16), dtype=np.float32)
    ids = np.zeros(129, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def step(nodes=nodes, k=2, centroids=cen, centroid_nodes=None, which=0):
        return lib.gg_kmeans_step(ctx, which, p(nodes), len(nodes), k, None if centroids is None else p(centroids),
                                  None if centroid_nodes is None else p(centroid_nodes), None, None, None, None, None)

    def fit(nodes=nodes, k=2, max_iters=3, init=None):
        return lib.gg_kmeans_fit(ctx, 0, p(nodes), len(nodes), k, max_iters, p(cen), None if init is None else p(init), None, None, None, None,
                                 None, None, None)

    outside = nodes.copy()
    outside[7] = n
    bad_ids = ids.copy()
    bad_ids[1] = -1
    cases = [(lambda: step(k=0), "k = 0 outside [1, 128]"), (lambda: step(k=129), "k = 129 outside [1, 128]"),
             (lambda: fit(k=0), "k = 0 outside [1, 128]"), (lambda: fit(k=129), "k = 129 outside [1, 128]"),
             (lambda: step(nodes=outside), "node id %d (entry 7) outside [0, %d)" % (n, n)),
             (lambda: fit(nodes=outside), "node id %d (entry 7) outside [0, %d)" % (n, n)),
             (lambda: step(centroids=cen, centroid_nodes=ids), "exactly one of centroids and centroid_nodes"),
             (lambda: step(centroids=None, centroid_nodes=None), "exactly one of centroids and centroid_nodes"),
             (lambda: step(centroids=None, centroid_nodes=bad_ids), "centroid_nodes[1] = -1 outside [0, %d)" % n),
             (lambda: fit(init=bad_ids), "init_nodes[1] = -1 outside [0, %d)" % n),
             (lambda: fit(max_iters=0), "max_iters = 0 outside [1, 1000000]"), (lambda: step(which=2), "which must be 0"),
             (lambda: lib.gg_kmeans_step(ctx, 0, p(nodes), 0, 2, p(cen), None, None, None, None, None, None), "m = 0 outside [1, 2^31 - 1]")]
    for call, text in cases:
        assert call() == ga.GG_EINVAL, text
        msg = lib.gg_last_error(ctx).decode()
        assert text in msg and ("gg_kmeans_step" in msg or "gg_kmeans_fit" in msg), (text, msg)
    for bad in (dict(centroids=X[:2], centroid_nodes=[0, 1]), dict(), dict(centroids=X[:2, :5]), dict(centroid_nodes=[0, n]),
                dict(centroids=X[:2], which=2)):
        with pytest.raises(ValueError, match="kmeans_step"):
            eng.kmeans_step(np.arange(10), **bad)
    for bad in (dict(init=None), dict(init=X[:3], k=2), dict(init=[0, 1], max_iters=0), dict(init=np.zeros((129, 16), np.float32)),
                dict(init=[0, -1])):
        with pytest.raises(ValueError, match="kmeans_fit"):
            eng.kmeans_fit(np.arange(10), **bad)
    with pytest.raises(ValueError, match="kmeans_seed"):
        eng.kmeans_seed(np.arange(10), 0, 1)
    res = eng.kmeans_fit(np.arange(10), init=[0, 1], max_iters=3)  # the engine stays usable
    assert int(res["counts"].sum()) == 10


# ---- 4. seeding
def test_seed_equals_the_rule_exactly_on_an_integer_table(engine_of):
    d, k, M = 33, 9, 700
    eng = engine_of(d, "int")
    T = tables(d, "int")[1]
    nodes = cs.draw_nodes(np.random.RandomState(77), M)
    X = T[nodes].astype(np.int64)
    for seed in (0, 1, 12345):
        rs = np.random.RandomState([seed, 0x4B4D])
        want = [int(rs.randint(M))]
        while len(want) < k:
            dist2 = np.stack([((X - X[p]) ** 2).sum(axis=1) for p in want]).min(axis=0)  # exact integers
            cum = np.cumsum(dist2.astype(np.float64))
            want.append(int(rs.randint(M)) if cum[-1] == 0 else min(int(np.searchsorted(cum, rs.random_sample() * cum[-1], side="right")), M - 1))
        got = eng.kmeans_seed(nodes, k, seed, which=1)
        assert got.dtype == np.int64 and got.tolist() == want
    same = np.full(50, nodes[0])  # every distance 0: the uniform draws
    rs = np.random.RandomState([4, 0x4B4D])
    assert eng.kmeans_seed(same, 3, 4, which=1).tolist() == [int(rs.randint(50)) for _ in range(3)]


def test_seed_on_blobs_is_valid_and_repeats(blob_engine):
    eng, X, labels, _ = blob_engine((33, 33, 10))
    nodes = np.arange(len(X))
    pos = eng.kmeans_seed(nodes, 33, 5)
    assert pos.shape == (33,) and pos.min() >= 0 and pos.max() < len(X)
    assert np.array_equal(pos, eng.kmeans_seed(nodes, 33, 5)) and not np.array_equal(pos, eng.kmeans_seed(nodes, 33, 6))
    assert len(set(labels[pos].tolist())) == 33  # D^2 sampling on separated blobs: one centre per blob


# ---- 5. end to end
def test_evaluation_appends_the_cluster_lines(ga, blob_engine, tmp_path):
    from graphgan_amd.evaluation import node_clustering as ncl
    from graphgan_amd.graph_gan import GraphGAN
    from tests.test_gpu_e2e import make_cfg
    shape = (5, 16, 60)
    eng, X, labels, _ = blob_engine(shape)
    n = len(X)
    eng.set_embeddings(0, X)
    eng.set_embeddings(1, X[::-1].copy())
    base = str(tmp_path)
    cfg = make_cfg(base, app="none", n_emb=16)
    os.makedirs(os.path.dirname(cfg.train_filename))
    os.makedirs(os.path.dirname(cfg.emb_filenames[0]))
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    test_edges = np.stack([np.arange(0, n, 7), (np.arange(0, n, 7) + 5) % n], axis=1)
    for path, edges in ((cfg.train_filename, ring), (cfg.test_filename, test_edges)):
        with open(path, "w") as f:
            f.writelines("%d\t%d\n" % (a, b) for a, b in edges.tolist())
    eng.set_graph_csr(*ga.edges_to_csr(n, ring))
    cfg.labels_filename = os.path.join(base, "labels.txt")
    with open(cfg.labels_filename, "w") as f:  # generator: node i has blob labels[i]; the file is shared, so the discriminator's rows
        f.writelines("%d %d\n" % (i, 7 * int(c)) for i, c in enumerate(labels))  # (reversed) cluster by labels[::-1] -- scored lower
    g = types.SimpleNamespace(config=cfg, engine=eng, n_node=n, seed=0, gen_likelihood=lambda: dict(nll=1.0, reach=1.0, n=3))
    cfg.engine_link_rank, cfg.engine_gen_nll = True, True
    want = GraphGAN.evaluation(g)  # the knob's default: off
    assert [ln.split(":")[0] for ln in want] == ["gen_rank", "dis_rank", "gen_nll"]
    cfg.engine_node_clustering = True
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen_rank", "dis_rank", "gen_cluster", "dis_cluster", "gen_nll"]
    assert lines[:2] + lines[4:] == want
    assert open(cfg.result_filename).read() == "".join(want + lines)
    gen = dict(f.split("=") for f in lines[2].strip().split(":")[1].split(" "))
    assert (float(gen["NMI"]), gen["ARI"], gen["purity"], gen["k"], gen["n"], gen["empty"]) == (pytest.approx(1.0, rel=1e-14), "1.0", "1.0", "5", "300", "0")
    # the engine-less float64 evaluator on the written .emb text: the same line but for the inertia's last digits
    eng.write_embeddings(0, cfg.emb_filenames[0])
    host = ncl.NodeClusterEval(cfg.emb_filenames[0], cfg.labels_filename, n, 16, seed=0).eval_node_clustering()
    hl = dict(f.split("=") for f in ncl.format_results("gen", host).strip().split(":")[1].split(" "))
    for key in ("NMI", "ARI", "purity", "k", "n", "iters", "empty"):
        assert gen[key] == hl[key], key
    means = np.stack([X[labels == c].astype(np.float64).mean(axis=0) for c in range(5)])
    assert abs(float(gen["inertia"]) - float(hl["inertia"])) <= float(kr.band(X, means).sum())
    del cfg.engine_node_clustering  # a user's config without the knob
    assert GraphGAN.evaluation(g) == want
