"""The push sweep on the device (gg_ppr_topk / gg_ppr_rank, Engine.ppr_topk / ppr_rank) and the graph_rank / graph_rec index=ppr
results lines.

Everything is an integer, so every comparison is EXACT equality -- on col, score, n_pos, ahead, pos_below, rank, rounds, converged
and residual -- with the restatement in dicts and ints (tests/support/ppr_ref.py) or, where a request is large, with the host
functions of evaluation/graph_ppr.py (which tests/test_graph_ppr_cpu.py holds against the restatement).  The graphs and the
parameters take every path of the sweep: tables in LDS and in global memory, narrow and wide neighbour lists, several scratch
passes, long probe chains that wrap round, full and short lists, zero rounds and cut-off rounds.

On the degree ladder the restatement in plain Python costs 0.1 ms, 8 ms and 0.1 s per root at the three parameter pairs (5, 17 000
and 250 000 pushed entries per root).  So every node is a root against the restatement at (0.5, 2^-8); at (0.15, 1e-4) every node
is a root against the host functions and every 8th node, the hubs, the probes and the isolated node against the restatement; at
(0.15, 2^-20) every 32nd node and those special nodes are roots."""
import ctypes

import numpy as np
import pytest

from tests.support import label_spread_ref as ls
from tests.support import ppr_ref as ref
from tests.support import two_hop_ref as th

pytestmark = pytest.mark.gpu

MODES = (True, "self")
ONE = ref.ONE
# (alpha, eps): on the ladder (n_node = 2066) E = min(n_node, 1 + B) is 2066, 513 and 2066: global, LDS and global tables
PARAMS = ((0.15, 1e-4), (0.5, 2.0 ** -8), (0.15, 2.0 ** -20))
KEYS_T = ("col", "score", "n_pos", "rounds", "converged", "residual")
KEYS_R = ("rank", "n_cand", "score", "ahead", "n_pos", "pos_below", "rounds", "converged", "residual")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def gp():
    from graphgan_amd.evaluation import graph_ppr
    return graph_ppr


def engine_for(ga, n, edges=None):
    table = np.zeros((n, 4), np.float32)  # (the sweep reads no embedding)
    eng = ga.Engine(table, table)
    if edges is not None:
        eng.set_graph_csr(*ga.edges_to_csr(n, np.asarray(edges, dtype=np.int32).reshape(-1, 2)))
    return eng


class Restated(object):
    """the restatement's dense rows of one graph and one parameter set, computed on first use and kept"""

    def __init__(self, N, alpha_q, eps_q, max_rounds=200):
        self.N, self.args, self.rows = N, (alpha_q, eps_q, max_rounds), {}

    def __getitem__(self, u):
        if u not in self.rows:
            self.rows[u] = ref.dense_row(self.N, u, *self.args)
        return self.rows[u]


def check_state(res, i, info):
    assert (int(res["rounds"][i]), int(res["converged"][i]), int(res["residual"][i])) == (info["rounds"], info["converged"], info["residual"])


def check_topk(res, R, rows, k, exclude):
    """device lists against the restatement, row by row"""
    assert res["col"].dtype == np.int32 and res["score"].dtype == np.uint64 and res["n_pos"].dtype == np.int32 and res["ms"] >= 0.0
    assert res["rounds"].dtype == res["converged"].dtype == np.int32 and res["residual"].dtype == np.uint64
    assert res["col"].shape == res["score"].shape == (len(rows), k)
    for i, u in enumerate(np.asarray(rows).tolist()):
        row, info = R[u]
        col, score, n_pos = th.topk(R.N, u, k, None, exclude, row=row)
        assert res["col"][i].tolist() == col and res["score"][i].tolist() == score and int(res["n_pos"][i]) == n_pos, (u, k, exclude)
        check_state(res, i, info)


def check_rank(res, R, u, v, exclude):
    assert res["rank"].dtype == res["n_cand"].dtype == np.int64 and res["score"].dtype == np.uint64
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        row, info = R[a]
        want = th.rank(R.N, a, b, None, exclude, row=row)
        assert {key: int(res[key][i]) for key in want} == want, (a, b, exclude)
        check_state(res, i, info)


def same(got, want, keys, sel=None):
    return all(np.array_equal(got[key], want[key] if sel is None else want[key][sel]) for key in keys)


@pytest.fixture(scope="module")
def ladder(ga, gp):
    """the degree ladder of the label-spreading tests, resident, with its neighbour sets and the restatement per parameter pair:
    shared, never changed"""
    n, edges, info = ls.hub_graph(0)
    N = ref.neighbor_sets(n, edges)
    deg = np.array([len(s) for s in N])
    assert deg[info["probes"]].tolist() == list(ls.LENGTHS) and deg[info["hub_a"]] == ls.HUB_A and deg[info["hub_b"]] == ls.HUB_B
    assert deg[info["isolated"]] == 0
    eng = engine_for(ga, n, edges)
    assert eng.distinct_degrees().tolist() == deg.tolist()
    cap = ga.Engine.PPR_LDS_CAP
    R = {}
    for alpha, eps in PARAMS:
        q = gp.quantise(alpha, eps)
        R[(alpha, eps)] = Restated(N, *q)
    E = [ref.bounds(n, *gp.quantise(*prm))[2] for prm in PARAMS]
    assert E[0] == n > cap and E[1] == 513 <= cap and E[2] == n  # both table classes
    special = np.array([info[k] for k in ("hub_a", "hub_b", "isolated")] + info["probes"].tolist())
    from graphgan_amd.evaluation import link_heuristics as lh
    yield dict(n=n, N=N, deg=deg, eng=eng, R=R, special=special, adj=lh.set_adjacency(edges, n), **info)
    eng.close()


@pytest.mark.parametrize("exclude", MODES)
@pytest.mark.parametrize("param", PARAMS)
def test_the_degree_ladder_against_the_restatement(ladder, gp, param, exclude):
    g, rs = ladder, np.random.RandomState(11)
    eng, n, N, R = g["eng"], g["n"], g["N"], g["R"][param]
    alpha, eps = param
    sp = g["special"]
    every = {PARAMS[0]: 8, PARAMS[1]: 1, PARAMS[2]: 32}[param]
    rows = np.unique(np.concatenate([np.arange(0, n, every), sp]))
    check_topk(eng.ppr_topk(rows, k=7, alpha=alpha, eps=eps, exclude=exclude), R, rows, 7, exclude)
    check_topk(eng.ppr_topk(sp, k=256, alpha=alpha, eps=eps, exclude=exclude), R, sp, 256, exclude)
    # one target per root: a random node, a neighbour, the root itself, the isolated node, in turn
    nb = np.array([min(N[u]) if N[u] else u for u in range(n)])
    v_all = np.choose(np.arange(n) % 4, [rs.randint(0, n, n), nb, np.arange(n), np.full(n, g["isolated"])])
    check_rank(eng.ppr_rank(rows, v_all[rows], alpha=alpha, eps=eps, exclude=exclude), R, rows, v_all[rows], exclude)
    if param == PARAMS[0]:  # every node as a root, against the host functions (the restatement takes 8 ms per root here)
        ptr, adj = g["adj"]
        rows = np.arange(n)
        assert same(eng.ppr_topk(rows, k=7, alpha=alpha, eps=eps, exclude=exclude), gp.host_ppr_topk(ptr, adj, rows, 7, alpha, eps, 200, exclude), KEYS_T)
        assert same(eng.ppr_rank(rows, v_all, alpha=alpha, eps=eps, exclude=exclude), gp.host_ppr_rank(ptr, adj, rows, v_all, alpha, eps, 200, exclude), KEYS_R)
    if exclude is True:
        infos = [R[u][1] for u in R.rows]
        assert all(i["converged"] == 1 for i in infos) and max(i["rounds"] for i in infos) >= 4
        assert all(i["sum_deg"] <= ref.bounds(n, *R.args[:2])[1] for i in infos)
        assert max(i["residual"] for i in infos) > 0 and R[g["isolated"]][1]["rounds"] == 1 and R[g["isolated"]][0][g["isolated"]] == ONE


def star(n, centre, leaves):
    return [(centre, x) for x in leaves]


def test_stars_that_fill_the_tables_on_both_sides_of_the_lds_cap(ga, gp):
    """E = min(n_node, 1 + B) does not depend on the graph: with eps = 1e-4 (B = 66 669) it is n_node.  A star over all nodes touches
    exactly E nodes -- the fullest table there is -- at n_node = cap - 1 and cap (LDS, 2048 slots) and cap + 1 (global, 4096 slots);
    a second and a third set_graph_csr move the centre."""
    cap = ga.Engine.PPR_LDS_CAP
    alpha, eps = 0.15, 1e-4
    q = gp.quantise(alpha, eps)
    for n in (cap - 1, cap, cap + 1):
        assert ref.bounds(n, *q)[2] == n
        eng = engine_for(ga, n)
        for centre in (0, n - 1, 517):
            leaves = [x for x in range(n) if x != centre]
            edges = star(n, centre, leaves)
            N = ref.neighbor_sets(n, edges)
            R = Restated(N, *q)
            eng.set_graph_csr(*ga.edges_to_csr(n, np.array(edges, dtype=np.int32)))
            rows = np.array([centre, leaves[0], leaves[-1], leaves[300]])
            v = np.array([leaves[5], centre, leaves[1], leaves[300]])
            assert len(R[centre][1]["touched"]) == n and len(R[leaves[0]][1]["touched"]) == n
            for exclude in MODES:
                check_topk(eng.ppr_topk(rows, k=256, alpha=alpha, eps=eps, exclude=exclude), R, rows, 256, exclude)
                check_rank(eng.ppr_rank(rows, v, alpha=alpha, eps=eps, exclude=exclude), R, rows, v, exclude)
        eng.close()


def test_parameters_that_put_the_bound_on_both_sides_of_the_lds_cap(ga, gp):
    """alpha = 0.5: kmin = eps_q / 2, and 1 + 2^40 // kmin is cap - 1, cap and cap + 1 on a graph with more nodes than that"""
    cap = ga.Engine.PPR_LDS_CAP
    n, rs = 1500, np.random.RandomState(2)
    edges = np.concatenate([rs.randint(0, n, (2500, 2)), np.array(star(n, 9, range(100, 300)))])
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    rows = np.concatenate([np.arange(0, n, 25), [9]])
    v = (rows * 11 + 2) % n
    got_E = []
    for kmin in (ONE // (cap - 2), ONE // (cap - 1), ONE // cap):
        eps_q = 2 * kmin
        alpha, eps = 0.5, eps_q / float(ONE)
        assert gp.quantise(alpha, eps) == (32768, eps_q)
        got_E.append(ref.bounds(n, 32768, eps_q)[2])
        R = Restated(N, 32768, eps_q)
        check_topk(eng.ppr_topk(rows, k=16, alpha=alpha, eps=eps), R, rows, 16, True)
        check_rank(eng.ppr_rank(rows, v, alpha=alpha, eps=eps, exclude="self"), R, rows, v, "self")
    assert got_E == [cap - 1, cap, cap + 1]
    eng.close()


@pytest.mark.parametrize("tables", ("lds", "global"))
def test_a_star_root_above_the_threshold_cut_and_just_below_it(ga, gp, tables):
    """the root pushes iff 2^40 >= eps_q deg: a centre with exactly 2^40 / eps_q leaves pushes once, one more leaf and nothing moves"""
    alpha, eps_q = (0.5, 1 << 32) if tables == "lds" else (0.15, 1 << 30)
    eps = eps_q / float(ONE)
    d = ONE // eps_q  # 256 and 1024
    edges = star(0, 0, range(1, d + 1)) + star(0, d + 1, range(d + 2, 2 * d + 3))
    n = 2 * d + 4  # (one isolated last node)
    q = gp.quantise(alpha, eps)
    assert q[1] == eps_q and (ref.bounds(n, *q)[2] <= ga.Engine.PPR_LDS_CAP) == (tables == "lds")
    N = ref.neighbor_sets(n, edges)
    assert len(N[0]) == d and len(N[d + 1]) == d + 1
    R = Restated(N, *q)
    eng = engine_for(ga, n, edges)
    rows = np.array([0, d + 1, 1, d + 2, n - 1])
    for exclude in MODES:
        res = eng.ppr_topk(rows, k=256, alpha=alpha, eps=eps, exclude=exclude)
        check_topk(res, R, rows, 256, exclude)
        assert res["rounds"][:2].tolist() == [1, 0] and res["converged"][:2].tolist() == [1, 1] and int(res["residual"][1]) == ONE
        assert res["n_pos"][1] == 0 and (res["col"][1] == -1).all() and (res["score"][1] == 0).all()
        v = np.array([3, d + 5, 0, d + 1, 0])
        r = eng.ppr_rank(rows, v, alpha=alpha, eps=eps, exclude=exclude)
        check_rank(r, R, rows, v, exclude)
        assert int(r["score"][1]) == 0 and int(r["n_pos"][1]) == 0 and int(r["rounds"][1]) == 0
    eng.close()


@pytest.mark.parametrize("tables", ("lds", "global"))
def test_probe_chains_that_are_long_and_wrap_round(ga, gp, tables):
    """ids a power of two apart land on one slot of the table, their mirror images at the top of the id range on the last slot.
    LDS: alpha = 0.5, eps = 2^-8, E = 513, 2048 slots; global: alpha = 0.5, eps_q = 2^30, E = 2049, 8192 slots."""
    n = 1 << 16
    alpha, eps_q, shift, slots = (0.5, 1 << 32, 12, 2048) if tables == "lds" else (0.5, 1 << 30, 13, 8192)
    eps = eps_q / float(ONE)
    q = gp.quantise(alpha, eps)
    E = ref.bounds(n, *q)[2]
    assert (E <= ga.Engine.PPR_LDS_CAP) == (tables == "lds") and slots // 4 < E <= slots // 2
    low = [j << shift for j in range(1, (n >> shift))]
    high = [n - 1 - x for x in low]
    assert {x % slots for x in low} == {0} and {x % slots for x in high} == {slots - 1} and len(low) >= 7
    A, qa = 100, 102
    edges = star(n, A, low + high + [qa]) + [(qa, low[0]), (low[1], high[2]), (high[0], slots - 1), (low[2], 0), (low[3], slots)]
    N = ref.neighbor_sets(n, edges)
    R = Restated(N, *q)
    assert len(R[A][1]["touched"]) >= len(low) + len(high) + 2 and R[A][1]["rounds"] >= 3
    eng = engine_for(ga, n, edges)
    rows = np.array([A, qa, low[0], high[-1], 0, slots - 1, n - 1])
    v = np.array([high[-1], low[-1], n - 1, 0, low[2], A, high[1]])
    for exclude in MODES:
        check_topk(eng.ppr_topk(rows, k=64, alpha=alpha, eps=eps, exclude=exclude), R, rows, 64, exclude)
        check_rank(eng.ppr_rank(rows, v, alpha=alpha, eps=eps, exclude=exclude), R, rows, v, exclude)
    eng.close()


@pytest.mark.parametrize("k", (1, 64, 256))
def test_ties_on_the_circulant(ga, gp, k):
    """i ~ i +- 1, i +- 5 (mod 257): every node has degree 4 and mirror images tie, so almost every score ties"""
    n = 257
    edges = [(i, (i + d) % n) for i in range(n) for d in (1, 5)]
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    rows = np.arange(n)
    for alpha, eps in ((0.15, 1e-4), (0.15, 2.0 ** -20)):
        R = Restated(N, *gp.quantise(alpha, eps))
        for exclude in MODES:
            res = eng.ppr_topk(rows, k=k, alpha=alpha, eps=eps, exclude=exclude)
            check_topk(res, R, rows, k, exclude)
        if k > 1:
            assert (res["score"][:, 0] == res["score"][:, 1]).all()  # the mirror image
        v = (rows * 31 + 7) % n
        check_rank(eng.ppr_rank(rows, v, alpha=alpha, eps=eps), R, rows, v, True)
    eng.close()


@pytest.mark.parametrize("max_rounds", (1, 2, 7))
def test_max_rounds_stops_where_the_restatement_stops(ladder, gp, max_rounds):
    g = ladder
    eng, n, N = g["eng"], g["n"], g["N"]
    rows = np.unique(np.concatenate([np.arange(0, n, 16), g["special"]]))
    v = (rows * 5 + 1) % n
    for alpha, eps in PARAMS[:2]:
        R = Restated(N, *gp.quantise(alpha, eps), max_rounds=max_rounds)
        res = eng.ppr_topk(rows, k=9, alpha=alpha, eps=eps, max_rounds=max_rounds)
        check_topk(res, R, rows, 9, True)
        check_rank(eng.ppr_rank(rows, v, alpha=alpha, eps=eps, max_rounds=max_rounds, exclude="self"), R, rows, v, "self")
        full = [g["R"][(alpha, eps)][u][1]["rounds"] for u in rows.tolist()]  # a query stops early only where it has converged
        assert res["rounds"].tolist() == [min(max_rounds, f) for f in full] and res["converged"].tolist() == [int(f <= max_rounds) for f in full]
        assert res["rounds"].max() == max_rounds or max(full) < max_rounds
        if (alpha, eps) == PARAMS[0]:
            assert (res["converged"] == 0).any() and res["converged"][rows == g["isolated"]].tolist() == [1]


def test_a_small_scratch_cap_splits_the_global_tasks_into_passes_without_changing_a_bit(ladder, gp):
    g = ladder
    eng, n = g["eng"], g["n"]
    alpha, eps = PARAMS[0]
    rows = np.concatenate([np.arange(19), g["special"]])  # 32 roots, each one global task
    assert len(rows) == 32
    v = (rows * 7 + 1) % n
    rows_r, v_r = np.repeat(rows, 2), np.stack([v, (v + 1) % n], axis=1).reshape(-1)  # the rank's tasks are runs of two queries
    slots = 8192
    assert slots // 4 < ref.bounds(n, *gp.quantise(alpha, eps))[2] == n <= slots // 2
    task = 8 * (2 * slots + slots // 2 + n + 3 * (n // 2))  # r, p, keys, shares, two frontier lists and the long-list indices (n is even)
    assert n % 2 == 0
    want_t = eng.ppr_topk(rows, k=33, alpha=alpha, eps=eps)
    want_r = eng.ppr_rank(rows_r, v_r, alpha=alpha, eps=eps)
    for scratch in (16 * task, 11 * task, task, 1):  # 32 tasks: 2 passes, 3 passes, one task per pass (twice)
        got_t = eng.ppr_topk(rows, k=33, alpha=alpha, eps=eps, scratch_bytes=scratch)
        got_r = eng.ppr_rank(rows_r, v_r, alpha=alpha, eps=eps, scratch_bytes=scratch)
        assert same(got_t, want_t, KEYS_T) and same(got_r, want_r, KEYS_R), scratch
    check_topk(want_t, g["R"][PARAMS[0]], rows, 33, True)


@pytest.mark.parametrize("param", PARAMS[:2])
def test_requests_do_not_change_a_querys_bits(ladder, param):
    g, rs = ladder, np.random.RandomState(8)
    eng, n = g["eng"], g["n"]
    kw = dict(alpha=param[0], eps=param[1])
    rows = np.arange(n)
    v = rs.randint(0, n, n)
    base_t, base_r = eng.ppr_topk(rows, k=9, **kw), eng.ppr_rank(rows, v, **kw)
    perm = rs.permutation(n)
    rep = np.concatenate([g["special"], g["special"][::-1], rs.randint(0, n, 200), [g["hub_b"]] * 5])
    for sel in (rows, perm, rep, perm[:63], g["special"][:1]):  # a rerun, permuted, repeated and subset queries
        got_t, got_r = eng.ppr_topk(sel, k=9, **kw), eng.ppr_rank(sel, v[sel], **kw)
        assert same(got_t, base_t, KEYS_T, sel) and same(got_r, base_r, KEYS_R, sel)


@pytest.mark.parametrize("param", PARAMS[:2])
def test_runs_of_equal_roots_share_a_push_and_keep_every_querys_bits(ladder, param):
    """runs of 1 .. 9 queries with one root, among them a run with one target repeated, against the same queries shuffled (runs of
    one, mostly) and against the restatement"""
    g, rs = ladder, np.random.RandomState(9)
    eng, n = g["eng"], g["n"]
    kw = dict(alpha=param[0], eps=param[1])
    roots = np.concatenate([g["special"], rs.randint(0, n, 40)])
    u = np.repeat(roots, 1 + np.arange(len(roots)) % 9)
    v = rs.randint(0, n, len(u))
    v[-3:] = v[-1]
    run = eng.ppr_rank(u, v, **kw)
    mix = rs.permutation(len(u))
    shuffled = eng.ppr_rank(u[mix], v[mix], **kw)
    assert same(shuffled, run, KEYS_R, mix)
    pick = rs.permutation(len(u))[:60]
    check_rank({key: run[key][pick] for key in KEYS_R}, g["R"][param], u[pick], v[pick], True)


@pytest.fixture(scope="module")
def sparse(ga):
    """2 000 nodes of mean degree 3 with a few hubs"""
    n, rs = 2000, np.random.RandomState(21)
    edges = np.concatenate([rs.randint(0, n, (3000, 2)), np.stack([np.repeat([7, 1500], 300), rs.randint(0, n, 600)], axis=1)])
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    from graphgan_amd.evaluation import link_heuristics as lh
    yield dict(n=n, N=N, eng=eng, edges=edges, adj=lh.set_adjacency(edges, n))
    eng.close()


@pytest.mark.parametrize("param", PARAMS[:2])
def test_request_sizes_from_none_to_more_tasks_than_a_launch_has_workgroups(sparse, gp, param):
    g = sparse
    eng, n = g["eng"], g["n"]
    ptr, adj = g["adj"]
    alpha, eps = param
    rows = np.arange(n)
    host_t = gp.host_ppr_topk(ptr, adj, rows, 4, alpha, eps)
    v_of = (rows * 13 + 5) % n
    host_r = gp.host_ppr_rank(ptr, adj, rows, v_of, alpha, eps)
    for m in (0, 1, 63, 64, 65, 70000):
        sel = np.random.RandomState(m).randint(0, n, m)
        t, r = eng.ppr_topk(sel, k=4, alpha=alpha, eps=eps), eng.ppr_rank(sel, v_of[sel], alpha=alpha, eps=eps)
        assert t["col"].shape == (m, 4) and r["rank"].shape == (m,) and t["rounds"].shape == r["residual"].shape == (m,)
        assert same(t, host_t, KEYS_T, sel) and same(r, host_r, KEYS_R, sel)
    # the host functions are held against the restatement on the CPU; here on a sample of this graph
    R = Restated(g["N"], *gp.quantise(alpha, eps))
    pick = np.arange(0, n, 97)
    check_topk({key: (host_t[key][pick] if key != "ms" else 0.0) for key in KEYS_T + ("ms",)}, R, pick, 4, True)


def test_rank_and_topk_agree_wherever_the_target_is_listed(sparse, ladder):
    for g, param in ((sparse, PARAMS[0]), (sparse, PARAMS[1]), (ladder, PARAMS[0]), (ladder, PARAMS[1])):
        eng, n = g["eng"], g["n"]
        kw = dict(alpha=param[0], eps=param[1])
        rows = np.arange(0, n, 3)
        for exclude in MODES:
            k = 16
            top = eng.ppr_topk(rows, k=k, exclude=exclude, **kw)
            u, j = np.nonzero(top["col"] >= 0)
            r = eng.ppr_rank(rows[u], top["col"][u, j], exclude=exclude, **kw)
            assert r["rank"].tolist() == (j + 1).tolist() and r["score"].tolist() == top["score"][u, j].tolist()
            # and the other way round: a random target with a score and rank <= k is listed at rank - 1
            v = np.random.RandomState(4).randint(0, n, len(rows))
            r = eng.ppr_rank(rows, v, exclude=exclude, **kw)
            elig = np.array([b not in th.excluded(g["N"], a, exclude) for a, b in zip(rows.tolist(), v.tolist())])
            hit = np.flatnonzero(elig & (r["score"] > 0) & (r["rank"] <= k))
            assert np.array_equal(top["col"][hit, r["rank"][hit] - 1], v[hit]) and np.array_equal(top["score"][hit, r["rank"][hit] - 1], r["score"][hit])
            listed = np.array([b in top["col"][i] for i, b in enumerate(v.tolist())])
            assert np.array_equal(listed, elig & (r["score"] > 0) & (r["rank"] <= k))


def test_refusals_name_the_function_and_the_value(ga):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    for call, name in ((lambda: eng.ppr_topk([0]), "gg_ppr_topk"), (lambda: eng.ppr_rank([0], [1]), "gg_ppr_rank")):
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
    refused(lambda: eng.ppr_topk([0], exclude=False), "ppr_topk: exclude must be True or 'self', got False", V)
    refused(lambda: eng.ppr_rank([0], [1], exclude=False), "ppr_rank: exclude must be True or 'self', got False", V)
    refused(lambda: eng.ppr_topk([0], exclude="graph"), "ppr_topk: exclude must be True or 'self', got 'graph'", V)
    for k in (0, 257, 2.0, True):
        refused(lambda: eng.ppr_topk([0], k=k), "ppr_topk: k must be an integer in [1, 256], got %r" % (k,), V)
    refused(lambda: eng.ppr_topk([0, 3, 50]), "ppr_topk: rows[2] = 50 out of range [0, 50)", V)
    refused(lambda: eng.ppr_rank([0, 50], [1, 2]), "ppr_rank: u[1] = 50 out of range [0, 50)", V)
    refused(lambda: eng.ppr_rank([0, 1], [1, -2]), "ppr_rank: v[1] = -2 out of range [0, 50)", V)
    refused(lambda: eng.ppr_rank([0, 1], [1]), "ppr_rank: u and v must have the same length, got 2 and 1", V)
    for s in (0, -4, 1.5):
        refused(lambda: eng.ppr_topk([0], scratch_bytes=s), "ppr_topk: scratch_bytes must be None or a positive integer, got %r" % (s,), V)
    for a, aq in ((0.0, 0), (1.0, 65536), (-0.1, -6554), (1e-6, 0)):
        refused(lambda: eng.ppr_topk([0], alpha=a), "graph ppr: alpha = %r gives alpha_q = %d outside [1, 65535]" % (a, aq), V)
    refused(lambda: eng.ppr_rank([0], [1], eps=0.01), "graph ppr: eps = 0.01 gives eps_q = 10995116278 outside [1, 4294967296]", V)
    refused(lambda: eng.ppr_rank([0], [1], eps=-1e-4), "graph ppr: eps = -0.0001 gives eps_q outside [1, 4294967296]", V)
    refused(lambda: eng.ppr_topk([0], eps=float("nan")), "graph ppr: alpha and eps must be finite", V)
    refused(lambda: eng.ppr_topk([0], alpha=0.15, eps=5e-12), "graph ppr: alpha_q * eps_q = 49150 is below 65536 (alpha = 0.15, eps = 5e-12)", V)
    for mr in (0, -1, 2.0, True):
        refused(lambda: eng.ppr_topk([0], max_rounds=mr), "ppr_topk: max_rounds must be a positive integer, got %r" % (mr,), V)
        refused(lambda: eng.ppr_rank([0], [1], max_rounds=mr), "ppr_rank: max_rounds must be a positive integer, got %r" % (mr,), V)

    # through the C ABI
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rows, tgt = np.array([0, 7], np.int32), np.array([2, 7], np.int32)
    col, sc, npos = np.full((3, 2), -7, np.int32), np.full((3, 2), 7, np.uint64), np.full(3, -7, np.int32)
    score, ahead, below = np.full(3, 7, np.uint64), np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    rounds, conv, resid = np.full(3, -7, np.int32), np.full(3, -7, np.int32), np.full(3, 7, np.uint64)
    AQ, EQ = 9830, 109951163

    def raw_t(rows=rows, m=2, k=2, aq=AQ, eq=EQ, mr=200, excl=2, scratch=0, col=col, sc=sc, npos=npos, rounds=rounds, conv=conv, resid=resid):
        return lambda: _lib.check(L.gg_ppr_topk(eng._ctx, p(rows), m, k, aq, eq, mr, excl, scratch, p(col), p(sc), p(npos), p(rounds), p(conv), p(resid), None),
                                  eng._ctx)

    def raw_r(u=rows, v=tgt, m=2, aq=AQ, eq=EQ, mr=200, excl=2, scratch=0, score=score, ahead=ahead, npos=npos, below=below, rounds=rounds, conv=conv,
              resid=resid):
        return lambda: _lib.check(L.gg_ppr_rank(eng._ctx, p(u), p(v), m, aq, eq, mr, excl, scratch, p(score), p(ahead), p(npos), p(below), p(rounds), p(conv),
                                                p(resid), None), eng._ctx)

    N = ref.neighbor_sets(n, ring)
    raw_t()()  # (kernel_ms may be NULL)
    want = [ref.topk(N, u, 2, AQ, EQ, 200) for u in (0, 7)]
    info = [ref.push(N, u, AQ, EQ, 200) for u in (0, 7)]
    assert col.tolist() == [w[0] for w in want] + [[-7, -7]] and sc.tolist() == [w[1] for w in want] + [[7, 7]]  # only m rows are written
    assert npos.tolist() == [w[2] for w in want] + [-7] and rounds.tolist() == [i["rounds"] for i in info] + [-7]
    assert conv.tolist() == [1, 1, -7] and resid.tolist() == [i["residual"] for i in info] + [7]
    raw_r()()
    want = [ref.rank(N, u, v, AQ, EQ, 200) for u, v in ((0, 2), (7, 7))]
    assert score.tolist() == [w["score"] for w in want] + [7] and ahead.tolist() == [w["ahead"] for w in want] + [-7]
    assert npos.tolist() == [w["n_pos"] for w in want] + [-7] and below.tolist() == [w["pos_below"] for w in want] + [-7]
    refused(raw_t(m=-1), "gg_ppr_topk: n_rows = -1 is negative")
    refused(raw_r(m=-3), "gg_ppr_rank: m = -3 is negative")
    refused(raw_t(m=1 << 31), "gg_ppr_topk: n_rows = 2147483648 does not fit in 31 bits")
    for k in (0, 257, -1):
        refused(raw_t(k=k), "gg_ppr_topk: k = %d outside [1, 256]" % k)
    for e in (0, 3, -1):
        refused(raw_t(excl=e), "gg_ppr_topk: exclude = %d is neither 1 (self) nor 2 (graph)" % e)
        refused(raw_r(excl=e), "gg_ppr_rank: exclude = %d is neither 1 (self) nor 2 (graph)" % e)
    refused(raw_t(scratch=-1), "gg_ppr_topk: scratch_bytes = -1 is negative")
    refused(raw_r(scratch=-8), "gg_ppr_rank: scratch_bytes = -8 is negative")
    for aq in (0, 65536, 1 << 20):
        refused(raw_t(aq=aq), "gg_ppr_topk: alpha_q = %d outside [1, 65535]" % aq)
        refused(raw_r(aq=aq), "gg_ppr_rank: alpha_q = %d outside [1, 65535]" % aq)
    for eq in (0, (1 << 32) + 1, 1 << 40):
        refused(raw_t(eq=eq), "gg_ppr_topk: eps_q = %d outside [1, 4294967296]" % eq)
        refused(raw_r(eq=eq), "gg_ppr_rank: eps_q = %d outside [1, 4294967296]" % eq)
    for mr in (0, -5):
        refused(raw_t(mr=mr), "gg_ppr_topk: max_rounds = %d is below 1" % mr)
        refused(raw_r(mr=mr), "gg_ppr_rank: max_rounds = %d is below 1" % mr)
    refused(raw_t(aq=9830, eq=6), "gg_ppr_topk: alpha_q * eps_q = 58980 is below 65536 (alpha_q = 9830, eps_q = 6)")
    refused(raw_r(aq=1, eq=65535), "gg_ppr_rank: alpha_q * eps_q = 65535 is below 65536 (alpha_q = 1, eps_q = 65535)")
    for kw in (dict(rows=None), dict(col=None), dict(sc=None), dict(npos=None), dict(rounds=None), dict(conv=None), dict(resid=None)):
        refused(raw_t(**kw), "gg_ppr_topk: rows, out_col, out_score, n_pos, rounds, converged and residual must not be NULL")
    for kw in (dict(u=None), dict(v=None), dict(score=None), dict(ahead=None), dict(npos=None), dict(below=None), dict(rounds=None), dict(conv=None),
               dict(resid=None)):
        refused(raw_r(**kw), "gg_ppr_rank: u, v, score, ahead, n_pos, pos_below, rounds, converged and residual must not be NULL")
    refused(raw_t(rows=np.array([50, 51], np.int32)), "gg_ppr_topk: rows[0] = 50 out of range [0, 50)")
    refused(raw_r(u=np.array([0, 50], np.int32)), "gg_ppr_rank: u[1] = 50 out of range [0, 50)")
    refused(raw_r(v=np.array([-1, 50], np.int32)), "gg_ppr_rank: v[0] = -1 out of range [0, 50)")
    raw_t(rows=None, m=0, col=None, sc=None, npos=None, rounds=None, conv=None, resid=None)()  # m == 0 succeeds and touches nothing
    raw_r(u=None, v=None, m=0, score=None, ahead=None, npos=None, below=None, rounds=None, conv=None, resid=None)()
    raw_t(aq=1, eq=65536, mr=1)()  # the smallest product the rule takes; the engine stays usable
    assert rounds[:2].tolist() == [1, 1] and conv[:2].tolist() == [0, 0]
    eng.close()


def _files(tmp_path, train, test):
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    np.savetxt(tr, train, fmt="%d")
    np.savetxt(te, test, fmt="%d")
    return tr, te


def test_results_lines_with_an_engine_are_string_equal_to_the_host_evaluators_on_a_random_graph(ga, gp, tmp_path):
    n, rs = 400, np.random.RandomState(31)
    edges = rs.randint(0, n - 5, (1500, 2))
    train, test = edges[:1300], edges[1300:][edges[1300:, 0] != edges[1300:, 1]]
    tr, te = _files(tmp_path, train, test)
    eng = engine_for(ga, n, train)
    for kw2 in (dict(), dict(alpha=0.5, eps=2.0 ** -8, max_rounds=3)):
        for cls, kw in ((gp.GraphPprRankEval, dict(ks=(1, 10, 100))), (gp.GraphPprRecEval, dict(ks=(2, 10, 256)))):
            dev, host = cls(tr, te, n, engine=eng, **kw, **kw2).lines(), cls(tr, te, n, **kw, **kw2).lines()
            assert dev == host and len(dev) == 1
            assert dev[0].startswith("graph_rank:index=ppr MRR=" if cls is gp.GraphPprRankEval else "graph_rec:index=ppr P@2=")
    eng.close()


def test_results_lines_on_ca_grqc_beside_the_two_hop_and_the_embedding_lines(ga, gp, tmp_path):
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
    dev = gp.GraphPprRankEval(tr, te, n, engine=eng, ks=ks).lines() + gp.GraphPprRecEval(tr, te, n, engine=eng).lines()
    host = gp.GraphPprRankEval(tr, te, n, ks=ks).lines() + gp.GraphPprRecEval(tr, te, n).lines()
    assert dev == host
    emb_line = lrank.format_results("gen", lrank.LinkRankEval(None, tr, te, n, emb.shape[1], engine=eng, ks=ks).eval_link_ranking(), ks)
    print("CA-GrQc, shipped rows: " + emb_line.strip())  # reported, not gated
    for ln in gr.GraphRankEval(tr, te, n, engine=eng, indices=("aa",), ks=ks).lines() + dev:
        print("CA-GrQc, graph only:  " + ln.strip())
    eng.close()
