"""The two-hop sweep on the device (gg_two_hop_topk / gg_two_hop_rank, Engine.two_hop_topk / two_hop_rank) and the graph_rank /
graph_rec results lines.

Everything is an integer, so every comparison is EXACT equality: with the restatement in sets, lists and ints
(tests/support/two_hop_ref.py), with Engine.pair_neighbors over all candidates, and with the host functions of
evaluation/graph_ranking.py.  The graphs take every path of the sweep: LDS and global tables, narrow and wide neighbour lists,
several scratch passes, long probe chains that wrap round, full and short lists."""
import ctypes

import numpy as np
import pytest

from tests.support import label_spread_ref as ls
from tests.support import two_hop_ref as ref

pytestmark = pytest.mark.gpu

MODES = (True, "self")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def engine_for(ga, n, edges=None):
    table = np.zeros((n, 4), np.float32)  # (the sweep reads no embedding)
    eng = ga.Engine(table, table)
    if edges is not None:
        eng.set_graph_csr(*ga.edges_to_csr(n, np.asarray(edges, dtype=np.int32).reshape(-1, 2)))
    return eng


def check_topk(res, N, rows, k, weights, exclude, dense=None):
    """device lists against the restatement, row by row"""
    assert res["col"].dtype == np.int32 and res["score"].dtype == np.uint64 and res["n_pos"].dtype == np.int32 and res["ms"] >= 0.0
    assert res["col"].shape == res["score"].shape == (len(rows), k)
    for i, u in enumerate(np.asarray(rows).tolist()):
        col, score, n_pos = ref.topk(N, u, k, weights, exclude, row=None if dense is None else dense[u])
        assert res["col"][i].tolist() == col and res["score"][i].tolist() == score and int(res["n_pos"][i]) == n_pos, (u, k, exclude)


def check_rank(res, N, u, v, weights, exclude, dense=None):
    assert res["rank"].dtype == res["n_cand"].dtype == np.int64 and res["score"].dtype == np.uint64
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        want = ref.rank(N, a, b, weights, exclude, row=None if dense is None else dense[a])
        got = {key: int(res[key][i]) for key in want}
        assert got == want, (a, b, exclude)


@pytest.fixture(scope="module")
def ladder(ga):
    """the degree ladder of the label-spreading tests, resident, with its neighbour sets, one weight array below 2^41 (sums pass
    2^32) and the dense rows of the restatement under no weights and under it: shared, never changed"""
    n, edges, info = ls.hub_graph(0)
    N = ref.neighbor_sets(n, edges)
    deg = np.array([len(s) for s in N])
    assert deg[info["probes"]].tolist() == list(ls.LENGTHS) and deg[info["hub_a"]] == ls.HUB_A and deg[info["hub_b"]] == ls.HUB_B
    assert deg[info["isolated"]] == 0
    rs = np.random.RandomState(5)
    w = rs.randint(0, 2 ** 41, n).astype(np.uint64)
    w[rs.permutation(n)[:20]] = 0  # (a reached node may still score 0)
    w[info["hub_b"]] = 2 ** 41 - 1
    eng = engine_for(ga, n, edges)
    assert eng.distinct_degrees().tolist() == deg.tolist()
    T = np.array([ref.expansion(N, u) for u in range(n)])
    cap = ga.Engine.TWO_HOP_LDS_CAP
    assert (T <= cap).sum() >= 10 and (T > cap).sum() >= 2000  # both table classes
    dense = {None: [ref.dense_row(N, u) for u in range(n)], "w": [ref.dense_row(N, u, w.tolist()) for u in range(n)]}
    assert max(max(r) for r in dense["w"]) > 2 ** 32
    special = np.array([info[k] for k in ("hub_a", "hub_b", "isolated")] + info["probes"].tolist())
    yield dict(n=n, N=N, deg=deg, eng=eng, w=w, T=T, dense=dense, special=special, **info)
    eng.close()


@pytest.mark.parametrize("exclude", MODES)
@pytest.mark.parametrize("weighted", (False, True))
def test_every_node_of_the_degree_ladder_against_the_restatement(ladder, weighted, exclude):
    g, rs = ladder, np.random.RandomState(11)
    eng, n, N = g["eng"], g["n"], g["N"]
    w, dense = (g["w"], g["dense"]["w"]) if weighted else (None, g["dense"][None])
    rows = np.arange(n)
    check_topk(eng.two_hop_topk(rows, k=7, weights=w, exclude=exclude), N, rows, 7, w, exclude, dense)
    sp = g["special"]
    check_topk(eng.two_hop_topk(sp, k=256, weights=w, exclude=exclude), N, sp, 256, w, exclude, dense)
    # one target per node: a random node, a neighbour, the node itself, the isolated node, in turn
    nb = np.array([min(N[u]) if N[u] else u for u in range(n)])
    v = np.choose(np.arange(n) % 4, [rs.randint(0, n, n), nb, rows, np.full(n, g["isolated"])])
    check_rank(eng.two_hop_rank(rows, v, weights=w, exclude=exclude), N, rows, v, w, exclude, dense)


def test_scores_equal_the_pair_neighbour_sweep_over_all_candidates(ladder):
    g, rs = ladder, np.random.RandomState(12)
    eng, n = g["eng"], g["n"]
    us = np.concatenate([g["special"], rs.randint(0, g["pool"], 8)])
    u, c = np.repeat(us, n), np.tile(np.arange(n), len(us))
    pn = eng.pair_neighbors(u, c, g["w"][None, :])
    for exclude in MODES:
        assert eng.two_hop_rank(u, c, exclude=exclude)["score"].tolist() == pn["cn"].tolist()
        assert eng.two_hop_rank(u, c, weights=g["w"], exclude=exclude)["score"].tolist() == pn["wsum"][0].tolist()
    assert pn["cn"][u == c].tolist() == g["deg"][us].tolist()  # c == u: S = the sum over N(u)


def stars(sizes):
    """one star per size: centre, then `size` leaves; -> (n, edges, centres, first leaves): a leaf's expansion is its centre's list"""
    edges, centres, firsts, nxt = [], [], [], 0
    for d in sizes:
        centres.append(nxt)
        firsts.append(nxt + 1)
        edges += [(nxt, nxt + 1 + j) for j in range(d)]
        nxt += d + 1
    return nxt, edges, centres, firsts


def test_queries_on_both_sides_of_the_lds_cap_and_across_it_after_a_new_graph(ga):
    cap = ga.Engine.TWO_HOP_LDS_CAP
    n_all = stars([cap, cap + 1, cap + 2])[0] + 1  # (room for the largest of the three graphs and one isolated last node)
    eng = engine_for(ga, n_all)
    w = np.random.RandomState(5).randint(1, 2 ** 41, n_all).astype(np.uint64)
    for shift in (0, 1, -2):  # the second and the third set_graph_csr move the queries: cap -> cap + 1 (global) -> cap - 2 (LDS), ...
        sizes = [cap - 1 + shift, cap + shift, cap + 1 + shift]
        _, edges, centres, firsts = stars(sizes)
        N = ref.neighbor_sets(n_all, edges)
        eng.set_graph_csr(*ga.edges_to_csr(n_all, np.array(edges, dtype=np.int32)))
        assert [ref.expansion(N, u) for u in firsts] == sizes
        q = np.array(firsts + [f + 3 for f in firsts] + centres)
        v = np.array([f + 1 for f in firsts] * 2 + [0, n_all - 1, centres[2] + 1])
        for exclude in MODES:
            for weights in (None, w):
                res = eng.two_hop_topk(q, k=256, weights=weights, exclude=exclude)
                check_topk(res, N, q, 256, weights, exclude)
                assert res["n_pos"][:3].tolist() == [d - 1 for d in sizes]  # the other leaves of the star
                check_rank(eng.two_hop_rank(q, v, weights=weights, exclude=exclude), N, q, v, weights, exclude)
    eng.close()


def test_probe_chains_that_are_long_and_wrap_round(ga):
    """ids a power of two apart land on one slot of every table, their mirror images at the top of the id range on the last slot"""
    n = 1 << 16
    a_nodes = [j << 12 for j in range(1, 16)] + [n - 1 - (j << 12) for j in range(15)]   # centre A: 30 + 1 entries -> 256 slots (LDS)
    b_nodes = [j << 13 for j in range(1, 8)] + [n - 1 - (j << 13) for j in range(7)] + list(range(20000, 22100))  # centre B: global, 8192 slots
    A, B, qa, qb = 100, 101, 102, 103
    edges = [(A, x) for x in a_nodes + [qa]] + [(B, x) for x in b_nodes + [qb]] + [(qa, a_nodes[0]), (a_nodes[3], b_nodes[2]), (qb, 21000)]
    N = ref.neighbor_sets(n, edges)
    assert ref.expansion(N, qa) < ga.Engine.TWO_HOP_LDS_CAP < ref.expansion(N, qb)
    eng = engine_for(ga, n, edges)
    w = np.random.RandomState(3).randint(1, 2 ** 41, n).astype(np.uint64)
    q = np.array([qa, qb, a_nodes[0], a_nodes[20], b_nodes[2], n - 1, 21000])
    v = np.array([a_nodes[29], b_nodes[13], n - 1, 0, b_nodes[0], a_nodes[1], n - 1 - (3 << 13)])
    for exclude in MODES:
        for weights in (None, w):
            check_topk(eng.two_hop_topk(q, k=64, weights=weights, exclude=exclude), N, q, 64, weights, exclude)
            check_rank(eng.two_hop_rank(q, v, weights=weights, exclude=exclude), N, q, v, weights, exclude)
    eng.close()


def test_a_small_scratch_cap_splits_the_global_tables_into_passes_without_changing_a_bit(ladder):
    g = ladder
    eng, n = g["eng"], g["n"]
    rows = np.concatenate([np.arange(30), g["special"]])  # 30 pool nodes (global tables of 8192 slots), the hubs, LDS queries between
    v = (rows * 7 + 1) % n
    table = 8192 * 12
    assert np.all(g["T"][:30] > eng.TWO_HOP_LDS_CAP) and 2 * min(int(g["T"][:30].max()), n) <= 8192
    for weights in (None, g["w"]):
        want_t = eng.two_hop_topk(rows, k=33, weights=weights)
        want_r = eng.two_hop_rank(rows, v, weights=weights)
        for scratch in (16 * table, 11 * table, table, 1):  # 32 global tables: 2 passes, 3 passes, one table per pass (twice)
            got_t = eng.two_hop_topk(rows, k=33, weights=weights, scratch_bytes=scratch)
            got_r = eng.two_hop_rank(rows, v, weights=weights, scratch_bytes=scratch)
            assert all(np.array_equal(got_t[key], want_t[key]) for key in ("col", "score", "n_pos")), scratch
            assert all(np.array_equal(got_r[key], want_r[key]) for key in ("rank", "n_cand", "score", "ahead", "n_pos", "pos_below")), scratch


@pytest.mark.parametrize("k", (1, 64, 65, 256))
def test_ties_and_lists_one_short_full_and_one_over(ga, k):
    """common neighbours on the circulant i ~ i +- 1, i +- 5 (mod 257), where almost every score ties; stars whose leaves have
    k - 1, k and k + 1 positive candidates, all tied"""
    n = 257
    edges = [(i, (i + d) % n) for i in range(n) for d in (1, 5)]
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    rows = np.arange(n)
    for exclude in MODES:
        check_topk(eng.two_hop_topk(rows, k=k, exclude=exclude), N, rows, k, None, exclude)
    v = (rows * 31 + 7) % n
    check_rank(eng.two_hop_rank(rows, v), N, rows, v, None, True)
    eng.close()
    n, edges, centres, firsts = stars([k, k + 1, k + 2])
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    q = np.array(firsts + [f + 1 for f in firsts])
    res = eng.two_hop_topk(q, k=k)
    assert res["n_pos"].tolist() == [k - 1, k, k + 1] * 2
    check_topk(res, N, q, k, None, True)
    assert (res["col"][0] == -1).sum() == 1 and (res["col"][1:3] >= 0).all() and res["score"][0, -1] == 0
    check_topk(eng.two_hop_topk(q, k=k, exclude="self"), N, q, k, None, "self")
    eng.close()


def test_empty_results_a_triangle_and_its_third_vertex_as_a_target(ga):
    # 0-1-2 a triangle; 3-4 an edge on its own; 5 isolated; 6-7-8 a path; 9 isolated and last
    n, edges = 10, [(0, 1), (1, 2), (0, 2), (3, 4), (6, 7), (7, 8), (1, 1), (0, 1)]
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    res = eng.two_hop_topk([5, 3, 0, 6], k=3)
    assert res["col"].tolist() == [[-1] * 3, [-1] * 3, [-1] * 3, [8, -1, -1]] and res["n_pos"].tolist() == [0, 0, 0, 1]
    assert res["score"].tolist() == [[0] * 3, [0] * 3, [0] * 3, [1, 0, 0]]
    res = eng.two_hop_topk([5, 3, 0, 6], k=3, exclude="self")  # (3 reaches only itself; 0 reaches 1 and 2 through each other)
    assert res["col"].tolist() == [[-1] * 3, [-1] * 3, [1, 2, -1], [8, -1, -1]] and res["n_pos"].tolist() == [0, 0, 2, 1]
    for exclude in MODES:
        rows = np.arange(n)
        check_topk(eng.two_hop_topk(rows, k=4, exclude=exclude), N, rows, 4, None, exclude)
        u, v = np.repeat(rows, n), np.tile(rows, n)  # every target of every query: v == u, neighbours, zero scores at 0, mid, n - 1
        r = eng.two_hop_rank(u, v, exclude=exclude)
        check_rank(r, N, u, v, None, exclude)
        at = int(np.flatnonzero((u == 0) & (v == 2))[0])
        assert int(r["score"][at]) == 1 and int(r["rank"][at]) == (1 if exclude is True else 2)  # a candidate under both; under "self" behind 1
        assert int(r["n_cand"][at]) == (n - 2 if exclude is True else n - 1)
    eng.close()


@pytest.fixture(scope="module")
def sparse(ga):
    """2 000 nodes of mean degree 3 with a few hubs: most scores are zero"""
    n, rs = 2000, np.random.RandomState(21)
    edges = np.concatenate([rs.randint(0, n, (3000, 2)), np.stack([np.repeat([7, 1500], 300), rs.randint(0, n, 600)], axis=1)])
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    from graphgan_amd.evaluation import link_heuristics as lh
    w = lh.node_weights(eng.distinct_degrees())[0]
    yield dict(n=n, N=N, eng=eng, w=w, edges=edges, adj=lh.set_adjacency(edges, n))
    eng.close()


def test_zero_score_targets_at_both_ends_and_mid_range_and_the_node_itself(sparse):
    g = sparse
    eng, n, N = g["eng"], g["n"], g["N"]
    rows = np.arange(0, n, 9)
    for target in (0, n - 1, n // 2, "self"):
        v = rows if target == "self" else np.full(len(rows), target)
        for exclude in MODES:
            res = eng.two_hop_rank(rows, v, weights=g["w"], exclude=exclude)
            check_rank(res, N, rows, v, g["w"], exclude)
            if target != "self":
                assert (res["score"] == 0).sum() > len(rows) // 2


def test_rank_and_topk_agree_wherever_the_target_is_listed(sparse, ladder):
    for g, weights in ((sparse, sparse["w"]), (sparse, None), (ladder, ladder["w"]), (ladder, None)):
        eng, n = g["eng"], g["n"]
        rows = np.arange(0, n, 3)
        for exclude in MODES:
            k = 16
            top = eng.two_hop_topk(rows, k=k, weights=weights, exclude=exclude)
            u, j = np.nonzero(top["col"] >= 0)
            r = eng.two_hop_rank(rows[u], top["col"][u, j], weights=weights, exclude=exclude)
            assert r["rank"].tolist() == (j + 1).tolist() and r["score"].tolist() == top["score"][u, j].tolist()
            # and the other way round: a random target with a score and rank <= k is listed at rank - 1
            v = np.random.RandomState(4).randint(0, n, len(rows))
            r = eng.two_hop_rank(rows, v, weights=weights, exclude=exclude)
            elig = np.array([b not in ref.excluded(g["N"], a, exclude) for a, b in zip(rows.tolist(), v.tolist())])
            hit = np.flatnonzero(elig & (r["score"] > 0) & (r["rank"] <= k))
            assert np.array_equal(top["col"][hit, r["rank"][hit] - 1], v[hit]) and np.array_equal(top["score"][hit, r["rank"][hit] - 1], r["score"][hit])
            listed = np.array([b in top["col"][i] for i, b in enumerate(v.tolist())])
            assert np.array_equal(listed, elig & (r["score"] > 0) & (r["rank"] <= k))


def test_requests_do_not_change_a_querys_bits(ladder):
    g, rs = ladder, np.random.RandomState(8)
    eng, n, w = g["eng"], g["n"], g["w"]
    rows = np.arange(n)
    v = rs.randint(0, n, n)
    base_t, base_r = eng.two_hop_topk(rows, k=9, weights=w), eng.two_hop_rank(rows, v, weights=w)
    keys_t, keys_r = ("col", "score", "n_pos"), ("rank", "n_cand", "score", "ahead", "n_pos", "pos_below")
    perm = rs.permutation(n)
    rep = np.concatenate([g["special"], g["special"][::-1], rs.randint(0, n, 200), [g["hub_b"]] * 5])
    for sel in (rows, perm, rep, perm[:63], g["special"][:1]):  # a rerun, permuted, repeated and subset queries
        got_t, got_r = eng.two_hop_topk(sel, k=9, weights=w), eng.two_hop_rank(sel, v[sel], weights=w)
        assert all(np.array_equal(got_t[key], base_t[key][sel]) for key in keys_t)
        assert all(np.array_equal(got_r[key], base_r[key][sel]) for key in keys_r)


def test_request_sizes_from_none_to_more_tasks_than_a_launch_has_workgroups(sparse):
    from graphgan_amd.evaluation import graph_ranking as gr
    g = sparse
    eng, n, w = g["eng"], g["n"], g["w"]
    ptr, adj = g["adj"]
    rows = np.arange(n)
    host_t = gr.host_two_hop_topk(ptr, adj, rows, 4, w, True)
    v_of = (rows * 13 + 5) % n
    host_r = gr.host_two_hop_rank(ptr, adj, rows, v_of, w, True)
    for m in (0, 1, 63, 64, 65, 70000):
        sel = np.random.RandomState(m).randint(0, n, m)
        t, r = eng.two_hop_topk(sel, k=4, weights=w), eng.two_hop_rank(sel, v_of[sel], weights=w)
        assert t["col"].shape == (m, 4) and r["rank"].shape == (m,)
        assert all(np.array_equal(t[key], host_t[key][sel]) for key in ("col", "score", "n_pos"))
        assert all(np.array_equal(r[key], host_r[key][sel]) for key in ("rank", "n_cand", "score", "ahead", "n_pos", "pos_below"))


def test_refusals_name_the_function_and_the_value(ga):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    for call, name in ((lambda: eng.two_hop_topk([0]), "gg_two_hop_topk"), (lambda: eng.two_hop_rank([0], [1]), "gg_two_hop_rank")):
        with pytest.raises(ga.GraphGANHipError) as ei:
            call()
        assert ei.value.code == ga.GG_EINVAL and "%s: needs the training graph (gg_set_graph_csr)" % name in str(ei.value)
    ring = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int32)
    eng.set_graph_csr(*ga.edges_to_csr(n, ring))

    def refused(call, text, exc=None):
        with pytest.raises(exc or ga.GraphGANHipError) as ei:
            call()
        assert text in str(ei.value), str(ei.value)
        if exc is None:
            assert ei.value.code == ga.GG_EINVAL

    # through Engine: the Python layer refuses the same things, before the ABI
    V = ValueError
    refused(lambda: eng.two_hop_topk([0], exclude=False), "two_hop_topk: exclude must be True or 'self', got False: S(u, u) >= S(u, c) for every c, so u would "
            "rank first for itself", V)
    refused(lambda: eng.two_hop_rank([0], [1], exclude=False), "two_hop_rank: exclude must be True or 'self', got False: S(u, u) >= S(u, c)", V)
    refused(lambda: eng.two_hop_topk([0], exclude="graph"), "two_hop_topk: exclude must be True or 'self', got 'graph'", V)
    refused(lambda: eng.two_hop_topk([0], exclude=1), "two_hop_topk: exclude must be True or 'self', got 1", V)
    for k in (0, 257, 2.0, True):
        refused(lambda: eng.two_hop_topk([0], k=k), "two_hop_topk: k must be an integer in [1, 256], got %r" % (k,), V)
    refused(lambda: eng.two_hop_topk([0, 3, 50]), "two_hop_topk: rows[2] = 50 out of range [0, 50)", V)
    refused(lambda: eng.two_hop_topk([-1, 50]), "two_hop_topk: rows[0] = -1 out of range [0, 50)", V)
    refused(lambda: eng.two_hop_rank([0, 50], [1, 2]), "two_hop_rank: u[1] = 50 out of range [0, 50)", V)
    refused(lambda: eng.two_hop_rank([0, 1], [1, -2]), "two_hop_rank: v[1] = -2 out of range [0, 50)", V)
    refused(lambda: eng.two_hop_rank([0, 1], [1]), "two_hop_rank: u and v must have the same length, got 2 and 1", V)
    refused(lambda: eng.two_hop_topk([0], weights=np.ones(49, np.uint64)), "two_hop_topk: weights must be None or 50 non-negative integers", V)
    refused(lambda: eng.two_hop_topk([0], weights=np.ones(50)), "two_hop_topk: weights must be None or 50 non-negative integers", V)
    refused(lambda: eng.two_hop_rank([0], [1], weights=-np.ones(50, np.int64)), "two_hop_rank: weights must be None or 50 non-negative integers", V)
    for s in (0, -4, 1.5):
        refused(lambda: eng.two_hop_topk([0], scratch_bytes=s), "two_hop_topk: scratch_bytes must be None or a positive integer, got %r" % (s,), V)
    refused(lambda: eng.two_hop_topk([0], weights=np.full(50, 2 ** 62, np.uint64)),
            "gg_two_hop_topk: the largest weight 4611686018427387904 times the largest degree 2 does not fit in 63 bits")

    # through the C ABI
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rows, tgt = np.array([0, 7], np.int32), np.array([2, 7], np.int32)
    col, sc, npos = np.full((3, 2), -7, np.int32), np.full((3, 2), 7, np.uint64), np.full(3, -7, np.int32)
    score, ahead, below = np.full(3, 7, np.uint64), np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    big = np.full(n, 2 ** 62, np.uint64)

    def raw_t(rows=rows, m=2, k=2, w=None, excl=2, scratch=0, col=col, sc=sc, npos=npos):
        return lambda: _lib.check(L.gg_two_hop_topk(eng._ctx, p(rows), m, k, p(w), excl, scratch, p(col), p(sc), p(npos), None), eng._ctx)

    def raw_r(u=rows, v=tgt, m=2, w=None, excl=2, scratch=0, score=score, ahead=ahead, npos=npos, below=below):
        return lambda: _lib.check(L.gg_two_hop_rank(eng._ctx, p(u), p(v), m, p(w), excl, scratch, p(score), p(ahead), p(npos), p(below), None), eng._ctx)

    raw_t()()  # (kernel_ms may be NULL)
    assert col.tolist() == [[2, 48], [5, 9], [-7, -7]] and sc.tolist() == [[1, 1], [1, 1], [7, 7]] and npos.tolist() == [2, 2, -7]  # only m rows are written
    raw_r()()
    assert score.tolist() == [1, 2, 7] and ahead.tolist() == [0, 0, -7] and npos.tolist() == [1, 2, -7] and below.tolist() == [0, 1, -7]
    refused(raw_t(m=-1), "gg_two_hop_topk: n_rows = -1 is negative")
    refused(raw_r(m=-3), "gg_two_hop_rank: m = -3 is negative")
    for k in (0, 257, -1):
        refused(raw_t(k=k), "gg_two_hop_topk: k = %d outside [1, 256]" % k)
    for e in (0, 3, -1):
        refused(raw_t(excl=e), "gg_two_hop_topk: exclude = %d is neither 1 (self) nor 2 (graph)" % e)
        refused(raw_r(excl=e), "gg_two_hop_rank: exclude = %d is neither 1 (self) nor 2 (graph)" % e)
    refused(raw_t(scratch=-1), "gg_two_hop_topk: scratch_bytes = -1 is negative")
    refused(raw_r(scratch=-8), "gg_two_hop_rank: scratch_bytes = -8 is negative")
    for kw in (dict(rows=None), dict(col=None), dict(sc=None), dict(npos=None)):
        refused(raw_t(**kw), "gg_two_hop_topk: rows, out_col, out_score and n_pos must not be NULL")
    for kw in (dict(u=None), dict(v=None), dict(score=None), dict(ahead=None), dict(npos=None), dict(below=None)):
        refused(raw_r(**kw), "gg_two_hop_rank: u, v, score, ahead, n_pos and pos_below must not be NULL")
    refused(raw_t(rows=np.array([50, 51], np.int32)), "gg_two_hop_topk: rows[0] = 50 out of range [0, 50)")
    refused(raw_t(rows=np.array([0, -2], np.int32)), "gg_two_hop_topk: rows[1] = -2 out of range [0, 50)")
    refused(raw_r(u=np.array([0, 50], np.int32)), "gg_two_hop_rank: u[1] = 50 out of range [0, 50)")
    refused(raw_r(v=np.array([-1, 50], np.int32)), "gg_two_hop_rank: v[0] = -1 out of range [0, 50)")
    refused(raw_t(w=big), "gg_two_hop_topk: the largest weight 4611686018427387904 times the largest degree 2 does not fit in 63 bits")
    refused(raw_r(w=big), "gg_two_hop_rank: the largest weight 4611686018427387904 times the largest degree 2 does not fit in 63 bits")
    raw_t(rows=None, m=0, col=None, sc=None, npos=None)()  # m == 0 succeeds and touches nothing
    raw_r(u=None, v=None, m=0, score=None, ahead=None, npos=None, below=None)()
    raw_t(excl=1)()  # the engine stays usable ("self": a ring has no triangle, so the neighbours are not reached either)
    assert col[:2].tolist() == [[2, 48], [5, 9]]
    eng.close()


def _files(tmp_path, train, test):
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    np.savetxt(tr, train, fmt="%d")
    np.savetxt(te, test, fmt="%d")
    return tr, te


def test_results_lines_with_an_engine_are_string_equal_to_the_host_evaluators_on_a_random_graph(ga, tmp_path):
    from graphgan_amd.evaluation import graph_ranking as gr
    n, rs = 400, np.random.RandomState(31)
    edges = rs.randint(0, n - 5, (1500, 2))
    train, test = edges[:1300], edges[1300:][edges[1300:, 0] != edges[1300:, 1]]
    tr, te = _files(tmp_path, train, test)
    eng = engine_for(ga, n, train)
    for cls, kw in ((gr.GraphRankEval, dict(ks=(1, 10, 100))), (gr.GraphRecEval, dict(ks=(2, 10, 256)))):
        dev, host = cls(tr, te, n, engine=eng, **kw).lines(), cls(tr, te, n, **kw).lines()
        assert dev == host and len(dev) == 3 and [ln.split(" ")[0].split("=")[1] for ln in dev] == ["cn", "aa", "ra"]
        assert all(ln.startswith("graph_rank:index=" if cls is gr.GraphRankEval else "graph_rec:index=") for ln in dev)
    eng.close()


def test_results_lines_on_ca_grqc_beside_the_embedding_lines(ga, tmp_path):
    from graphgan_amd.evaluation import graph_ranking as gr
    from graphgan_amd.evaluation import link_ranking as lrank
    from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc
    d, n, _ = load_ca_grqc()
    train, test = np.asarray(d["train"]), np.asarray(d["test"])
    tr, te = _files(tmp_path, train, test)
    emb = ca_grqc_init_embeddings(d, n).astype(np.float32)
    eng = ga.Engine(emb, emb)
    eng.set_graph_csr(*ga.edges_to_csr(n, train.astype(np.int32)))
    ks = (1, 10, 100)
    dev = gr.GraphRankEval(tr, te, n, engine=eng, ks=ks).lines() + gr.GraphRecEval(tr, te, n, engine=eng).lines()
    host = gr.GraphRankEval(tr, te, n, indices=("aa",), ks=ks).lines() + gr.GraphRecEval(tr, te, n, indices=("aa",)).lines()
    assert [dev[1], dev[4]] == host  # (the host runs one index: it is the slow side)
    emb_line = lrank.format_results("gen", lrank.LinkRankEval(None, tr, te, n, emb.shape[1], engine=eng, ks=ks).eval_link_ranking(), ks)
    print("CA-GrQc, shipped rows: " + emb_line.strip())  # reported, not gated
    for ln in dev:
        print("CA-GrQc, graph only:  " + ln.strip())
    eng.close()
