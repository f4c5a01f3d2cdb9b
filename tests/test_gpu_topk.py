"""Streamed top-K retrieval (gg_topk_scores / Engine.topk) and the recommendation evaluator on the device.

fp32 is checked EXACTLY: the reference of a row is the oracle's fp32 score row (orc.c_all_score_rows with zero bias: the
k-ordered fmaf chain of the matrix-core kernel), eligibility applied, stably sorted by (score descending, column
ascending) -- columns identical and scores equal under ==.  bf16 is checked against fp64 numpy on the bf16-rounded table."""
import os

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc, star_graph_edges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def _bf16_round(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, like v_cvt_pk_bf16_f32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _nbr_sets(rowptr, col):
    return [set(col[rowptr[v]:rowptr[v + 1]].tolist()) for v in range(len(rowptr) - 1)]


def rank_rows(S, rows, k, nbrs=None):
    """Reference ranking of score rows S [len(rows), n] (any float dtype): eligibility (nbrs given: not the row's node, not its
    neighbours), then a stable sort by (score descending, column ascending); first k, padded with -1 / -inf."""
    n = S.shape[1]
    cols = np.full((len(rows), k), -1, dtype=np.int64)
    scores = np.full((len(rows), k), -np.inf, dtype=S.dtype)
    idx_all = np.arange(n)
    for i, u in enumerate(rows):
        if nbrs is not None:
            elig = np.ones(n, dtype=bool)
            elig[u] = False
            if nbrs[u]:
                elig[list(nbrs[u])] = False
            idx = idx_all[elig]
        else:
            idx = idx_all
        s = S[i, idx]
        o = np.lexsort((idx, -s))[:k]
        cols[i, :len(o)] = idx[o]
        scores[i, :len(o)] = s[o]
    return cols, scores


def oracle_topk(E, rows, k, nbrs=None):
    S = orc.c_all_score_rows(orc.pad_rows(E), np.zeros(E.shape[0], np.float32), rows)
    return rank_rows(S, rows, k, nbrs)


def assert_exact(res, want):
    assert np.array_equal(res["col"], want[0]), np.argwhere(res["col"] != want[0])[:5]
    assert np.array_equal(res["score"], want[1].astype(np.float32))


def assert_bf16_close(res, E, rows, k, nbrs=None):
    """scores within 2e-3 max(1, max|S|) of fp64 on the bf16-rounded table; index sets equal except for columns whose reference
    score lies within that tolerance of the row's k-th score."""
    Eb = _bf16_round(E).astype(np.float64)
    S = Eb[rows] @ Eb.T
    wc, ws = rank_rows(S, rows, k, nbrs)
    tol = 2e-3 * max(1.0, np.abs(S).max())
    fin = np.isfinite(ws)
    assert np.array_equal(np.isfinite(res["score"]), fin)
    assert np.max(np.abs(res["score"][fin] - ws[fin]), initial=0.0) <= tol
    got_s = np.take_along_axis(S, np.maximum(res["col"], 0), 1)
    assert np.max(np.abs(res["score"][fin] - got_s[fin]), initial=0.0) <= tol  # each returned score belongs to its column
    for i in range(len(rows)):
        a, b = set(res["col"][i].tolist()) - {-1}, set(wc[i].tolist()) - {-1}
        kth = ws[i][fin[i]][-1] if fin[i].any() else -np.inf
        for c in a ^ b:
            assert abs(S[i, c] - kth) <= tol, (i, c, S[i, c], kth)


def _graph(ga, n, seed):
    """power-law graph with duplicated adjacency entries (a few edges listed twice)"""
    edges = ga.synth_powerlaw(n, 3, seed, seed + 1)
    edges = np.concatenate([edges, edges[:: max(1, len(edges) // 40)]])
    return ga.edges_to_csr(n, edges)


@pytest.mark.parametrize("n,d", [(700, 50), (3000, 128), (1029, 256), (300, 8), (600, 300)])
def test_topk_fp32_exact_against_the_oracle(ga, n, d):
    rs = np.random.RandomState(n + d)
    Eg = (rs.randn(n, d) * 0.5).astype(np.float32)
    Ed = (rs.randn(n, d) * 0.3).astype(np.float32)
    rowptr, col = _graph(ga, n, 7)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(Eg, Ed)
    eng.set_graph_csr(rowptr, col)
    rows = rs.randint(0, n, 97).astype(np.int32)
    rows[5] = rows[60]  # a repeated row
    all_rows = np.arange(n, dtype=np.int32)
    for which, E in ((0, Eg), (1, Ed)):
        S_rows = orc.c_all_score_rows(orc.pad_rows(E), np.zeros(n, np.float32), rows)
        S_all = orc.c_all_score_rows(orc.pad_rows(E), np.zeros(n, np.float32), all_rows) if which == 0 else None
        for k in (1, 10, 100, 256):
            for exclude in (False, True):
                res = eng.topk(rows, k=k, which=which, exclude=exclude)
                assert res["col"].shape == (len(rows), k) and res["kernel_ms"] > 0
                assert_exact(res, rank_rows(S_rows, rows, k, nbrs if exclude else None))
                if S_all is not None and k in (10, 256):
                    assert_exact(eng.topk(None, k=k, which=which, exclude=exclude), rank_rows(S_all, all_rows, k, nbrs if exclude else None))
    eng.close()


@pytest.mark.parametrize("n,d", [(700, 50), (3000, 128), (1029, 256), (300, 8), (600, 300)])
def test_topk_bf16_against_fp64_on_the_rounded_table(ga, n, d):
    rs = np.random.RandomState(n * 3 + d)
    Eg = (rs.randn(n, d) * 0.5).astype(np.float32)
    rowptr, col = _graph(ga, n, 9)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(Eg, Eg * np.float32(0.5))
    eng.set_graph_csr(rowptr, col)
    rows = rs.randint(0, n, 64).astype(np.int32)
    for which, E in ((0, Eg), (1, Eg * np.float32(0.5))):
        for k in (1, 10, 100):
            for exclude in (False, True):
                res = eng.topk(rows, k=k, which=which, precision="bf16", exclude=exclude)
                assert_bf16_close(res, E, rows, k, nbrs if exclude else None)
    eng.close()


def test_topk_more_rows_than_one_pass(ga):
    """the rows are processed in internal passes of 4 096: a call with more rows (repeats included) is the same as per row"""
    n, d = 5000, 32
    rs = np.random.RandomState(4)
    E = (rs.randn(n, d) * 0.4).astype(np.float32)
    rowptr, col = _graph(ga, n, 3)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    rows = rs.randint(0, n, 4500).astype(np.int32)
    res = eng.topk(rows, k=20, exclude=True)
    assert_exact(res, oracle_topk(E, rows, 20, _nbr_sets(rowptr, col)))
    full = eng.topk(None, k=5)
    assert_exact(full, oracle_topk(E, np.arange(n, dtype=np.int32), 5))
    eng.close()


def test_topk_ties_prefer_the_smaller_column(ga):
    """many duplicated embedding rows: whole groups of columns score exactly equal; the smaller column wins everywhere --
    inside a wavefront's list, across column splits and at the k boundary"""
    n, d = 6000, 24
    rs = np.random.RandomState(11)
    base = (rs.randn(12, d) * 0.5).astype(np.float32)
    E = base[rs.randint(0, 12, n)]
    eng = ga.Engine(E, E)
    rows = np.array([0, 1, 2, 3, 17, 999, 5999], dtype=np.int32)
    for k in (1, 7, 100, 256):
        want = oracle_topk(E, rows, k)
        res = eng.topk(rows, k=k)
        assert_exact(res, want)
        assert (np.diff(res["col"], axis=1)[np.diff(res["score"], axis=1) == 0] > 0).all()
    eng.close()


def test_topk_exclusion_at_a_hub(ga):
    """star graph: the hub's leaves outscore everything for the hub (and each other).  Excluded columns never enter a list --
    if they did they would raise the threshold and push the true answers out -- so the hub's list holds neither a neighbour
    nor the hub; the leaves' lists never hold the hub."""
    edges, n = star_graph_edges(30000)
    rowptr, col = ga.edges_to_csr(n, edges)
    nbrs = _nbr_sets(rowptr, col)
    d = 16
    rs = np.random.RandomState(2)
    E = (rs.randn(n, d) * 0.05).astype(np.float32)
    E[0, 0] += 1.0
    E[1:30001, 0] += 2.0
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    rows = np.array([0, 1, 2, 15, 29999, 30000, n - 1], dtype=np.int32)
    for prec in ("fp32", "bf16"):
        res = eng.topk(rows, k=256, exclude=True, precision=prec)
        hub = set(res["col"][0].tolist())
        assert not (hub & nbrs[0]) and 0 not in hub and -1 not in hub
        for i in range(1, 5):
            assert 0 not in res["col"][i] and rows[i] not in res["col"][i]
        if prec == "fp32":
            assert_exact(res, oracle_topk(E, rows, 256, nbrs))
    # without the exclusion the hub's list is leaves
    res = eng.topk(rows[:1], k=100)
    assert set(res["col"][0].tolist()) <= nbrs[0]
    eng.close()


def test_topk_row_with_fewer_eligible_columns_than_k(ga):
    """node 0 is linked to every node but five: its list is those five, then -1 / -inf"""
    n, d = 300, 8
    keep = {3, 77, 150, 151, 299}
    edges = np.array([(0, v) for v in range(1, n) if v not in keep] + [(5, 6), (6, 7)], dtype=np.int32)
    rowptr, col = ga.edges_to_csr(n, edges)
    E = (np.random.RandomState(5).randn(n, d)).astype(np.float32)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    for prec in ("fp32", "bf16"):
        res = eng.topk([0, 6], k=10, exclude=True, precision=prec)
        assert set(res["col"][0, :5].tolist()) == keep
        assert (res["col"][0, 5:] == -1).all() and np.isneginf(res["score"][0, 5:]).all()
        assert (res["col"][1] >= 0).all()
    want = oracle_topk(E, np.array([0, 6], np.int32), 10, _nbr_sets(rowptr, col))
    assert_exact(eng.topk([0, 6], k=10, exclude=True), want)
    eng.close()


def test_topk_argument_errors(ga):
    E = np.ones((50, 8), np.float32)
    eng = ga.Engine(E, E)
    with pytest.raises(ga.GraphGANHipError) as ei:
        eng.topk([0], k=3, exclude=True)  # no graph
    assert ei.value.code == ga.GG_EINVAL and "gg_set_graph_csr" in str(ei.value)
    with pytest.raises(ga.GraphGANHipError):
        eng.topk([50], k=3)
    for bad in (dict(k=0), dict(k=257), dict(which=2), dict(precision="fp16")):
        with pytest.raises(ValueError):
            eng.topk([0], **bad)
    assert eng.topk([], k=4)["col"].shape == (0, 4)
    eng.close()


@pytest.mark.parametrize("n,d", [(700, 50), (3000, 128)])
def test_topk_k1_equals_the_streamed_max(ga, n, d):
    """zero bias, no exclusion, k = 1: the top-1 is K7's max / argmax (gg_all_score_reduce, fp32) exactly"""
    E = (np.random.RandomState(d).randn(n, d) * 0.5).astype(np.float32)
    eng = ga.Engine(E, E)
    eng.set_bias(0, np.zeros(n, np.float32))
    rows = np.arange(0, n, 3, dtype=np.int32)
    ref = eng.all_score_reduce(rows, precision="fp32", logsumexp=False)
    res = eng.topk(rows, k=1)
    assert np.array_equal(res["col"][:, 0], ref["argmax"]) and np.array_equal(res["score"][:, 0], ref["max"])
    eng.close()


def test_topk_follows_training_steps(ga):
    """after d_step / g_step the result equals the oracle on the updated tables: nothing is cached stale"""
    n, d = 800, 32
    rs = np.random.RandomState(21)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    eng = ga.Engine(E, E * np.float32(0.7))
    rowptr, col = _graph(ga, n, 5)
    eng.set_graph_csr(rowptr, col)
    nbrs = _nbr_sets(rowptr, col)
    rows = rs.randint(0, n, 40).astype(np.int32)
    before = [eng.topk(rows, k=30, which=w, exclude=True) for w in (0, 1)]
    for it in range(3):
        u, v = rs.randint(0, n, 256).astype(np.int32), rs.randint(0, n, 256).astype(np.int32)
        eng.d_step(u, v, (rs.rand(256) < 0.5).astype(np.float32))
        eng.g_step(u, v, rs.rand(256).astype(np.float32))
        for w in (0, 1):
            res = eng.topk(rows, k=30, which=w, exclude=True)
            assert_exact(res, oracle_topk(eng.get_embeddings(w), rows, 30, nbrs))
    after = eng.topk(rows, k=30, which=0, exclude=True)
    assert not np.array_equal(before[0]["score"], after["score"])  # (the steps did move the scores)
    eng.close()


def test_topk_at_1m_nodes(ga):
    """the bench workload (10^6 nodes, d = 128, power-law graph): 64 rows, k = 100, exclusion of the graph's neighbours;
    fp32 exact against the oracle, bf16 against fp64 on the rounded table"""
    from graphgan_amd import workloads
    rowptr, col, E, _ = workloads.powerlaw_workload(10 ** 6)
    eng = ga.Engine(E, E, optimizer=ga.GG_OPT_SGD)
    eng.set_graph_csr(rowptr, col)
    rows = np.random.RandomState(8).choice(10 ** 6, 64, replace=False).astype(np.int32)
    rows[0] = int(np.argmax(np.diff(rowptr)))  # the largest hub
    nbrs = {int(u): set(col[rowptr[u]:rowptr[u + 1]].tolist()) for u in rows}
    nb = [nbrs.get(v, set()) for v in range(int(rows.max()) + 1)]
    res = eng.topk(rows, k=100, exclude=True)
    assert_exact(res, oracle_topk(E, rows, 100, nb))
    res = eng.topk(rows, k=100, exclude=True, precision="bf16")
    Eb = _bf16_round(E).astype(np.float64)
    S = Eb[rows] @ Eb.T
    wc, ws = rank_rows(S, rows, 100, nb)
    tol = 2e-3 * max(1.0, np.abs(S).max())
    assert np.max(np.abs(res["score"] - ws)) <= tol
    for i in range(len(rows)):
        assert not (set(res["col"][i].tolist()) & nb[rows[i]]) and rows[i] not in res["col"][i]
        for c in set(res["col"][i].tolist()) ^ set(wc[i].tolist()):
            assert abs(S[i, c] - ws[i, -1]) <= tol
    eng.close()


def test_topk_bf16_at_10m_nodes(ga):
    """BASELINE configs[4] size (10^7 nodes, d = 256), bf16: 32 rows, k = 100 against a chunked fp64 sweep of the rounded
    table -- also the at-size parity of the K7 family's bf16 tile stream"""
    from graphgan_amd import workloads
    _, _, E, _ = workloads.powerlaw_workload(10 ** 7, n_emb=256)
    eng = ga.Engine(E, E, optimizer=ga.GG_OPT_SGD)
    rows = np.random.RandomState(9).choice(10 ** 7, 32, replace=False).astype(np.int32)
    res = eng.topk(rows, k=100, precision="bf16")
    eng.close()
    A = _bf16_round(E[rows]).astype(np.float64)
    best_s = np.full((32, 0), -np.inf)
    best_c = np.zeros((32, 0), np.int64)
    smax = 0.0
    for c0 in range(0, 10 ** 7, 1 << 20):
        S = A @ _bf16_round(E[c0:c0 + (1 << 20)]).astype(np.float64).T
        smax = max(smax, float(np.abs(S).max()))
        part = np.argpartition(-S, 150, axis=1)[:, :150]
        best_s = np.concatenate([best_s, np.take_along_axis(S, part, 1)], 1)
        best_c = np.concatenate([best_c, part + c0], 1)
        o = np.argsort(-best_s, axis=1, kind="stable")[:, :200]
        best_s, best_c = np.take_along_axis(best_s, o, 1), np.take_along_axis(best_c, o, 1)
    tol = 2e-3 * max(1.0, smax)
    assert np.max(np.abs(res["score"] - best_s[:, :100])) <= tol
    for i in range(32):
        kth = best_s[i, 99]
        ref = set(best_c[i, :100].tolist())
        for c in set(res["col"][i].tolist()) ^ ref:
            j = np.flatnonzero(best_c[i] == c)
            s = best_s[i, j[0]] if len(j) else -np.inf  # (outside the 200 best: far below the k-th score)
            assert abs(s - kth) <= tol, (i, c)


def _ca_grqc_files(tmp_path):
    d, n, graph = load_ca_grqc()
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    for path, key in ((tr, "train"), (te, "test")):
        with open(path, "w") as f:
            f.writelines("%d\t%d\n" % (a, b) for a, b in d[key].tolist())
    return d, n, tr, te


def test_recommendation_evaluator_on_ca_grqc(ga, tmp_path):
    """engine path == a ranking of the oracle's fp32 rows (identical P@K / R@K); the float64 host path agrees within
    1 / (K n_queries)"""
    from graphgan_amd.evaluation import recommendation as rec
    d, n, tr, te = _ca_grqc_files(tmp_path)
    emb = ca_grqc_init_embeddings(d, n).astype(np.float32)
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng = ga.Engine(emb, emb * np.float32(0.5))
    eng.set_graph_csr(rowptr, col)
    ks = (2, 10, 20)
    dev = rec.RecommendEval("unused", tr, te, n, 50, engine=eng, which=0, ks=ks).eval_recommendation()
    test_nbrs = rec._neighbour_sets(d["test"].tolist(), n)
    queries = np.array([u for u in range(n) if test_nbrs[u]], dtype=np.int32)
    wc, _ = oracle_topk(emb, queries, 20, _nbr_sets(rowptr, col))
    assert dev == rec.precision_recall(wc, queries, test_nbrs, ks)
    host = rec.RecommendEval("unused", tr, te, n, 50, emd=emb.astype(np.float64), ks=ks).eval_recommendation()
    for K in ks:
        assert abs(dev[K][0] - host[K][0]) <= 1.0 / (K * len(queries)) + 1e-12
        assert abs(dev[K][1] - host[K][1]) <= 1.0 / (K * len(queries)) + 1e-12
        assert 0.0 < dev[K][0] <= 1.0 and 0.0 < dev[K][1] <= 1.0
    bf = rec.RecommendEval("unused", tr, te, n, 50, engine=eng, which=0, ks=ks, precision="bf16").eval_recommendation()
    assert abs(bf[20][1] - dev[20][1]) < 0.05
    eng.close()


def test_graph_gan_recommendation_app_writes_the_result_lines(tmp_path):
    """graph_gan.py with app = "recommendation" on the short schedule: one P@K / R@K line per mode, no test-negatives file"""
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    d, n, graph = write_reference_layout(base)
    os.remove(os.path.join(base, "data", "link_prediction", "CA-GrQc_test_neg.txt"))
    cfg = make_cfg(base, app="recommendation", n_epochs=1, n_epochs_dis=1, n_epochs_gen=1)
    for attr in ("train_filename", "test_filename", "test_neg_filename", "pretrain_emb_filename_d", "pretrain_emb_filename_g",
                 "result_filename"):
        setattr(cfg, attr, getattr(cfg, attr).replace("/recommendation/", "/link_prediction/"))
    cfg.emb_filenames = [p.replace("/recommendation/", "/link_prediction/") for p in cfg.emb_filenames]
    from graphgan_amd.graph_gan import GraphGAN
    g = GraphGAN(cfg)
    g.train()
    g.engine.close()
    lines = open(cfg.result_filename).read().splitlines()
    assert len(lines) >= 2
    for mode, line in zip(("gen", "dis"), lines[-2:]):
        assert line.startswith(mode + ":")
        fields = line[len(mode) + 1:].split(" ")
        assert [f.split("=")[0] for f in fields] == ["P@2", "R@2", "P@10", "R@10", "P@20", "R@20"]
        assert all(0.0 <= float(f.split("=")[1]) <= 1.0 for f in fields)
