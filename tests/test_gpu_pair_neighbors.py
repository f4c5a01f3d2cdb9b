"""The pair-neighbour sweep (gg_pair_neighbors / gg_distinct_degrees, Engine.pair_neighbors / distinct_degrees /
link_heuristics) and the graph_lp results line on the device.

Everything the sweep returns is an integer, so everything is checked EXACTLY against the definition restated with Python sets
and Python integers on the lists given to set_graph_csr: N(x) = the distinct entries of x's list other than x,
C(u, v) = (N(u) & N(v)) - {u, v}, cn = |C|, wsum = the sum of the weights over C."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_WEIGHT = 1 << 41


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def nbr_sets(rowptr, col):
    return [set(col[rowptr[x]:rowptr[x + 1]].tolist()) - {x} for x in range(len(rowptr) - 1)]


def ref_sweep(N, u, v, weights):
    cn, du, dv = [], [], []
    ws = [[] for _ in weights]
    wl = [w.tolist() for w in weights]
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        C = (N[a] & N[b]) - {a, b}
        cn.append(len(C))
        du.append(len(N[a]))
        dv.append(len(N[b]))
        for j, w in enumerate(wl):
            ws[j].append(sum(w[x] for x in C))
    return cn, du, dv, ws


def check_sweep(eng, N, u, v, rs, n_ws=(0, 1, 4)):
    """the sweep of the pairs with every number of weight arrays against the definition; returns the n_w = 4 result"""
    n = len(N)
    w4 = rs.randint(0, MAX_WEIGHT, size=(4, n)).astype(np.uint64)
    res = None
    for n_w in n_ws:
        w = w4[:n_w]
        res = eng.pair_neighbors(u, v, w if n_w else None)
        cn, du, dv, ws = ref_sweep(N, u, v, w)
        assert res["cn"].dtype == np.int32 and res["wsum"].dtype == np.uint64 and res["wsum"].shape == (n_w, len(cn))
        assert res["cn"].tolist() == cn, "cn, n_w = %d" % n_w
        assert res["deg_u"].tolist() == du and res["deg_v"].tolist() == dv, "degrees, n_w = %d" % n_w
        assert res["wsum"].tolist() == ws, "wsum, n_w = %d" % n_w
        assert res["kernel_ms"] >= 0.0
    return res


def engine_for(ga, n):
    table = np.zeros((n, 4), np.float32)  # (the sweep reads no embedding)
    return ga.Engine(table, table)


def multigraph(ga, n, n_edges, seed, isolated=3):
    """random edges with duplicates in both orientations and self-loops; the last ``isolated`` nodes have no edge"""
    rs = np.random.RandomState(seed)
    e = rs.randint(0, n - isolated, size=(n_edges, 2))
    loops = np.repeat(rs.randint(0, n - isolated, max(2, n // 20)), 2).reshape(-1, 2)
    e = np.concatenate([e, e[: n_edges // 8], e[n_edges // 8: n_edges // 4, ::-1], loops]).astype(np.int32)
    return ga.edges_to_csr(n, e[rs.permutation(len(e))])


LENGTHS = (0, 1, 2, 63, 64, 65, 129)


def test_every_combination_of_list_lengths(ga):
    """two probes of each length, every probe paired with every probe (u == v included): every group width (shorter list <= 8,
    <= 64, longer) against every length of the searched list; the pool is small, so the intersections are large"""
    rs = np.random.RandomState(1)
    n_probe, pool = 2 * len(LENGTHS), 180
    n = n_probe + pool
    edges = [(p, n_probe + int(x)) for p in range(n_probe) for x in rs.permutation(pool)[:LENGTHS[p % len(LENGTHS)]]]
    edges += [(n_probe + int(a), n_probe + int(b)) for a, b in rs.randint(0, pool, size=(300, 2))]  # the pool among itself
    rowptr, col = ga.edges_to_csr(n, np.array(edges, dtype=np.int32))
    N = nbr_sets(rowptr, col)
    assert [len(N[p]) for p in range(n_probe)] == list(LENGTHS) * 2
    eng = engine_for(ga, n)
    eng.set_graph_csr(rowptr, col)
    u, v = (x.ravel() for x in np.meshgrid(np.arange(n_probe), np.arange(n_probe), indexing="ij"))
    res = check_sweep(eng, N, u, v, rs)
    assert res["cn"].max() >= 64  # (129 against 129 of 180)
    # a probe against the pool nodes it lists (pairs that are edges) and against pool nodes at random
    pu = np.repeat(np.arange(n_probe), 20)
    check_sweep(eng, N, pu, rs.randint(n_probe, n, len(pu)), rs)
    for p in (3, 6, 13):
        mine = np.array(sorted(N[p]))
        check_sweep(eng, N, np.full(len(mine), p), mine, rs, n_ws=(1,))
    eng.close()


def test_duplicates_self_loops_isolated_nodes_and_edge_pairs(ga):
    n = 300
    rowptr, col = multigraph(ga, n, 1500, 2)
    N = nbr_sets(rowptr, col)
    raw = [col[rowptr[x]:rowptr[x + 1]].tolist() for x in range(n)]
    assert any(len(r) != len(set(r)) for r in raw) and any(r.count(x) == 2 for x, r in enumerate(raw))  # duplicates; a self-loop is listed twice
    assert all(len(N[x]) == 0 for x in range(n - 3, n))
    eng = engine_for(ga, n)
    eng.set_graph_csr(rowptr, col)
    rs = np.random.RandomState(3)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    u = np.concatenate([rs.randint(0, n, 2000), np.arange(n), src, [n - 1, n - 2, 0]])
    v = np.concatenate([rs.randint(0, n, 2000), np.arange(n), col, [n - 2, 5, n - 1]])  # random, u == v, every listed edge (loops too), isolated ends
    check_sweep(eng, N, u, v, rs)
    deg = eng.distinct_degrees()
    assert deg.dtype == np.int32 and deg.tolist() == [len(s) for s in N]
    want = [len(np.setdiff1d(np.unique(col[rowptr[x]:rowptr[x + 1]]), [x])) for x in range(n)]
    assert deg.tolist() == want
    eng.close()


def hub_lists(chunk, rs):
    """The neighbour lists of two hubs with 3 chunk + 17 and 4 chunk + 5 entries as one ascending sequence of nodes, each in
    the first list, the second, or both: about half of each list is common, and so are the first and the last entry of each
    list and the entries on both sides of every chunk edge (positions k chunk - 1 and k chunk of either list).
    -> (category per node: 'a', 'b' or 'c'), without the common last node."""
    ta, tb = 3 * chunk + 17 - 1, 4 * chunk + 5 - 1  # (the last entry of both lists is one common node, appended by the caller)
    edge_a = {0} | {k * chunk - 1 for k in range(1, 4)} | {k * chunk for k in range(1, 4)}
    edge_b = {0} | {k * chunk - 1 for k in range(1, 5)} | {k * chunk for k in range(1, 5)}
    la = lb = 0
    cats = []
    while la < ta or lb < tb:
        behind = "a" if la * tb <= lb * ta else "b"  # the list further from its length
        if la == ta:
            cat = "b"
        elif lb == tb:
            cat = "a"
        else:
            cat = "c" if rs.rand() < 0.27 else behind  # (about half of the shorter list)
            if (cat != "b" and la in edge_a) or (cat != "a" and lb in edge_b):
                cat = "c"
        la += cat != "b"
        lb += cat != "a"
        cats.append(cat)
    return cats


def test_hubs_longer_than_the_chunk(ga):
    """pairs whose SHORTER list is longer than the chunk are split into tasks that add into the outputs"""
    chunk = ga.Engine.PAIR_NEIGHBORS_CHUNK
    assert chunk >= 2
    rs = np.random.RandomState(4)
    cats = hub_lists(chunk, rs) + ["c"]
    A, B, first = 0, 1, 2
    ids = first + np.arange(len(cats))
    n = first + len(cats) + 40
    la = [int(x) for x, c in zip(ids, cats) if c != "b"]
    lb = [int(x) for x, c in zip(ids, cats) if c != "a"]
    assert len(la) == 3 * chunk + 17 and len(lb) == 4 * chunk + 5
    both = set(la) & set(lb)
    assert 0.35 * len(la) < len(both) < 0.65 * len(la)
    for lst in (la, lb):  # the first and last entry and both sides of every chunk edge are common
        assert all(lst[p] in both for p in [0, -1] + [k * chunk + o for k in range(1, len(lst) // chunk + 1) for o in (-1, 0)])
    tail = np.arange(n - 40, n)
    edges = [(A, x) for x in la] + [(B, x) for x in lb] + [(int(t), int(rs.choice(ids))) for t in tail for _ in range(3)]
    rowptr, col = ga.edges_to_csr(n, np.array(edges, dtype=np.int32)[rs.permutation(len(edges))])
    N = nbr_sets(rowptr, col)
    assert N[A] == set(la) and N[B] == set(lb)
    only_a = [x for x in la if x not in both and len(N[x]) == 1]
    only_b = [x for x in lb if x not in both and len(N[x]) == 1]
    assert len(only_a) > 10 and len(only_b) > 10  # degree-1 nodes
    eng = engine_for(ga, n)
    eng.set_graph_csr(rowptr, col)
    u = [A, B, A, B] + [A] * 10 + [B] * 10 + only_a[:10] + only_b[:10] + [A, B] * 5 + list(both)[:10] + tail.tolist()
    v = [B, A, A, B] + only_a[:10] + only_b[:10] + [B] * 10 + [A] * 10 + list(both)[:10] + [A, B] * 5 + [A] * 40
    res = check_sweep(eng, N, np.array(u), np.array(v), rs)
    assert res["cn"][:4].tolist() == [len(both), len(both), len(la), len(lb)]
    assert res["wsum"].max() > 1 << 50  # (sums far above 32 bits)
    # many copies of the split pairs in one call, between short pairs: the chunk tasks of different pairs do not mix
    uu = np.tile(np.array([A, 5, B, B, 7, A]), 50)
    vv = np.tile(np.array([B, A, B, A, 9, A]), 50)
    check_sweep(eng, N, uu, vv, rs, n_ws=(4,))
    eng.close()


@pytest.fixture(scope="module")
def dense(ga):
    """2 000 nodes of about 30 distinct neighbours: nearly every pair takes the 16-lane groups"""
    n = 2000
    rowptr, col = multigraph(ga, n, 28000, 5)
    eng = engine_for(ga, n)
    eng.set_graph_csr(rowptr, col)
    yield eng, nbr_sets(rowptr, col), n
    eng.close()


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_pair_counts_around_a_wavefront(dense, m):
    eng, N, n = dense
    rs = np.random.RandomState(6 + m)
    res = check_sweep(eng, N, rs.randint(0, n, m), rs.randint(0, n, m), rs)
    assert res["cn"].shape == (m,)


def test_more_tasks_than_one_grid_pass_and_the_bit_contract(dense):
    """70 000 pairs: more tasks of one group width than groups in its launch, so the groups stride; exchanging the ends,
    permuting the pairs and running again change no bit"""
    eng, N, n = dense
    rs = np.random.RandomState(7)
    m = 70000
    u, v = rs.randint(0, n, m), rs.randint(0, n, m)
    short = np.array([min(len(N[a]), len(N[b])) for a, b in zip(u.tolist(), v.tolist())])
    assert ((short > 8) & (short <= 64)).sum() > 2048 * 16  # (the largest launch: 2 048 workgroups of 16 groups)
    w = rs.randint(0, MAX_WEIGHT, size=(4, n)).astype(np.uint64)
    res = eng.pair_neighbors(u, v, w)
    cn, du, dv, ws = ref_sweep(N, u, v, w)
    assert res["cn"].tolist() == cn and res["deg_u"].tolist() == du and res["deg_v"].tolist() == dv and res["wsum"].tolist() == ws
    assert res["cn"].max() >= 3
    swapped = eng.pair_neighbors(v, u, w)
    assert np.array_equal(swapped["cn"], res["cn"]) and np.array_equal(swapped["wsum"], res["wsum"])
    assert np.array_equal(swapped["deg_u"], res["deg_v"]) and np.array_equal(swapped["deg_v"], res["deg_u"])
    perm = rs.permutation(m)
    permuted = eng.pair_neighbors(u[perm], v[perm], w)
    again = eng.pair_neighbors(u, v, w)
    for k in ("cn", "deg_u", "deg_v"):
        assert np.array_equal(permuted[k], res[k][perm]) and np.array_equal(again[k], res[k])
    assert np.array_equal(permuted["wsum"], res["wsum"][:, perm]) and np.array_equal(again["wsum"], res["wsum"])


def test_a_new_graph_drops_the_set_adjacency(ga):
    n = 400
    eng = engine_for(ga, n)
    rs = np.random.RandomState(8)
    u, v = rs.randint(0, n, 500), rs.randint(0, n, 500)
    results = []
    for seed, n_edges in ((9, 3000), (10, 1200), (9, 3000)):
        rowptr, col = multigraph(ga, n, n_edges, seed)
        eng.set_graph_csr(rowptr, col)
        N = nbr_sets(rowptr, col)
        assert eng.distinct_degrees().tolist() == [len(s) for s in N]
        results.append(check_sweep(eng, N, u, v, np.random.RandomState(11), n_ws=(2,)))
    assert not np.array_equal(results[0]["cn"], results[1]["cn"])
    assert np.array_equal(results[0]["cn"], results[2]["cn"]) and np.array_equal(results[0]["wsum"], results[2]["wsum"])
    eng.close()


def test_refusals_name_the_entry_point(ga):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    for call in (lambda: eng.pair_neighbors([0], [1]), lambda: eng.distinct_degrees()):  # no graph
        with pytest.raises(ga.GraphGANHipError) as ei:
            call()
        assert ei.value.code == ga.GG_EINVAL and "gg_set_graph_csr" in str(ei.value)
        assert "gg_pair_neighbors" in str(ei.value) or "gg_distinct_degrees" in str(ei.value)
    ring = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int32)
    eng.set_graph_csr(*ga.edges_to_csr(n, ring))

    def refused(call, text):
        with pytest.raises(ga.GraphGANHipError) as ei:
            call()
        assert ei.value.code == ga.GG_EINVAL and "gg_pair_neighbors" in str(ei.value) and text in str(ei.value), str(ei.value)

    refused(lambda: eng.pair_neighbors([0, 3, 50], [1, 2, 3]), "u[2] = 50 out of range [0, 50)")
    refused(lambda: eng.pair_neighbors([0, 3], [1, -1]), "v[1] = -1 out of range [0, 50)")
    refused(lambda: eng.pair_neighbors([0], [1], np.ones((5, n), np.uint64)), "n_w = 5 outside [0, 4]")
    # a sum may have max(deg) = 2 terms: weights of 2^62 could reach 2^63
    big = np.full((1, n), 1 << 62, dtype=np.uint64)
    refused(lambda: eng.pair_neighbors([0], [2], big), "does not fit in 63 bits")
    ok = eng.pair_neighbors([0], [2], big // 2 + (big // 2 - 1))  # (2^62 - 1) * 2 < 2^63
    assert ok["cn"].tolist() == [1] and ok["wsum"].tolist() == [[(1 << 62) - 1]]
    with pytest.raises(ValueError):
        eng.pair_neighbors([0, 1], [1])
    with pytest.raises(ValueError):
        eng.pair_neighbors([0], [1], np.ones((1, n + 1), np.uint64))
    # NULL outputs and a negative count, through the C ABI
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    u, v = np.array([0, 1], np.int32), np.array([2, 3], np.int32)
    out = [np.zeros(2, np.int32) for _ in range(3)]
    w, ws = np.ones(n, np.uint64), np.zeros(2, np.uint64)

    def raw(u=u, v=v, m=2, w=w, n_w=1, cn=out[0], du=out[1], dv=out[2], ws=ws):
        return lambda: _lib.check(L.gg_pair_neighbors(eng._ctx, p(u), p(v), m, p(w), n_w, p(cn), p(du), p(dv), p(ws), None), eng._ctx)

    raw()()  # (kernel_ms may be NULL)
    assert out[0].tolist() == [1, 1] and ws.tolist() == [1, 1]
    for bad in (dict(cn=None), dict(du=None), dict(dv=None)):
        refused(raw(**bad), "cn, deg_u and deg_v must not be NULL")
    for bad in (dict(w=None), dict(ws=None)):
        refused(raw(**bad), "weights and wsum must not be NULL when n_w > 0")
    for bad in (dict(u=None), dict(v=None)):
        refused(raw(**bad), "u and v must not be NULL")
    refused(raw(m=-1), "m = -1 is negative")
    refused(raw(n_w=-1), "n_w = -1 outside [0, 4]")
    raw(w=None, ws=None, n_w=0)()  # no weights: neither pointer is needed
    raw(u=None, v=None, m=0, cn=None, du=None, dv=None)()  # m == 0 succeeds and touches nothing
    with pytest.raises(ga.GraphGANHipError) as ei:
        _lib.check(L.gg_distinct_degrees(eng._ctx, None), eng._ctx)
    assert ei.value.code == ga.GG_EINVAL and "gg_distinct_degrees" in str(ei.value) and "must not be NULL" in str(ei.value)
    res = eng.pair_neighbors([0, 7], [2, 7])  # the engine stays usable
    assert res["cn"].tolist() == [1, 2] and res["deg_u"].tolist() == [2, 2] and res["wsum"].shape == (0, 2)
    eng.close()


def test_link_heuristics_against_the_unquantised_indices(ga):
    """cn, jaccard and pa are equal; aa and ra lie within the quantisation of the node weights: every weight is rint(2^40 x) of
    its value x, so within 2^-41 of it -- cn 2^-41 for a sum of cn terms -- and the float64 roundings of the two sides (the
    reference's cn - 1 additions and its terms, the one conversion of the integer sum) are below (cn + 1) 2^-52 of the value"""
    n = 500
    rowptr, col = multigraph(ga, n, 4000, 12)
    N = nbr_sets(rowptr, col)
    eng = engine_for(ga, n)
    eng.set_graph_csr(rowptr, col)
    rs = np.random.RandomState(13)
    u, v = np.concatenate([rs.randint(0, n, 3000), np.arange(n)]), np.concatenate([rs.randint(0, n, 3000), np.arange(n)])
    got = eng.link_heuristics(u, v)
    deg = np.array([len(s) for s in N], dtype=np.float64)
    for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        C = sorted((N[a] & N[b]) - {a, b})
        cn, den = len(C), len(N[a]) + len(N[b]) - len(C)
        assert got["cn"][i] == cn and got["pa"][i] == len(N[a]) * len(N[b]) and got["jaccard"][i] == (cn / den if den else 0.0)
        aa = float(np.sum(1.0 / np.log(deg[C]))) if cn else 0.0  # (a common neighbour of u != v has degree >= 2; of u == v: degree 1 weighs 0)
        if a == b:
            aa = float(np.sum([1.0 / np.log(deg[x]) for x in C if deg[x] >= 2]))
        ra = float(np.sum(1.0 / deg[C])) if cn else 0.0
        for key, ref in (("aa", aa), ("ra", ra)):
            assert abs(got[key][i] - ref) <= cn * 2.0 ** -41 + (cn + 1) * 2.0 ** -52 * ref, (key, i, got[key][i], ref)
    assert got["cn"].dtype == np.int64 and got["pa"].dtype == np.int64 and got["aa"].dtype == np.float64 and got["cn"].max() >= 5
    eng.close()


def test_results_line_equals_the_host_evaluators_on_a_random_graph(ga, tmp_path):
    from graphgan_amd.evaluation import link_heuristics as lh
    n = 600
    rs = np.random.RandomState(14)
    edges = np.concatenate([ga.synth_powerlaw(n, 4, 3, 4), rs.randint(0, n, size=(200, 2)), np.repeat(np.arange(0, 40, 4), 2).reshape(-1, 2)])
    edges = edges[rs.permutation(len(edges))]
    held = edges[:300]
    train = np.concatenate([edges[300:], edges[300:360, ::-1]])  # (some edges twice)
    files = [str(tmp_path / x) for x in ("train.txt", "test.txt", "neg.txt")]
    for path, rows in zip(files, (train, held, rs.randint(0, n, size=(300, 2)))):
        np.savetxt(path, rows, fmt="%d", delimiter="\t")
    eng = engine_for(ga, n)
    eng.set_graph_csr(*ga.edges_to_csr(n, train))
    dev_ev, host_ev = lh.LinkHeuristicsEval(*files, n, engine=eng), lh.LinkHeuristicsEval(*files, n)
    uu, vv, _ = host_ev.read_test()
    dev_sw, host_sw = dev_ev.sweep(uu, vv), host_ev.sweep(uu, vv)
    for k in ("cn", "deg_u", "deg_v", "wsum"):
        assert np.array_equal(dev_sw[k], host_sw[k]) and dev_sw[k].dtype == host_sw[k].dtype, k
    dev, host = dev_ev.eval_link_heuristics(), host_ev.eval_link_heuristics()
    assert dev == host and lh.format_results(dev) == lh.format_results(host)
    assert dev["n_test"] == 600 and all(0.0 <= dev[k] <= 1.0 for k in lh.INDICES)
    assert len(np.unique(dev_sw["cn"])) >= 3 and dev_sw["wsum"].max() > 1 << 40  # (the line is no constant's)
    eng.close()


def test_graph_gan_writes_the_graph_lp_line_on_ca_grqc(tmp_path):
    """graph_gan.py with engine_lp_heuristics on the CA-GrQc fixture: one graph_lp line after the *_lp lines, string-equal to the
    host evaluator's, and repeated from the cache by a second evaluation.  The line is printed beside the embedding's."""
    from graphgan_amd.evaluation import link_heuristics as lh
    from graphgan_amd.graph_gan import GraphGAN
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    write_reference_layout(base)
    cfg = make_cfg(base, n_epochs=0, engine_lp_heuristics=True, engine_lp_classifier=True)
    g = GraphGAN(cfg)
    g.train()
    lines = open(cfg.result_filename).read().splitlines(True)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "gen_lp", "dis_lp", "graph_lp"]
    host = lh.LinkHeuristicsEval(cfg.train_filename, cfg.test_filename, cfg.test_neg_filename, g.n_node).eval_link_heuristics()
    assert lines[4] == lh.format_results(host) == g._graph_lp_line
    assert host["n_test"] == 2 * 1449 and all(0.5 < host[k] < 1.0 for k in lh.INDICES)  # (the fixture's edge counts)
    print("CA-GrQc, shipped rows:\n" + "".join(lines))
    calls = []
    g.engine.pair_neighbors = lambda *a, **k: calls.append(a)  # a second evaluation computes nothing of the line again
    assert GraphGAN.evaluation(g)[4] == lines[4] and not calls
    g.engine.close()
