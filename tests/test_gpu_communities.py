"""The neighbour-mode sweep (gg_neighbor_mode, Engine.neighbor_mode), label propagation iterated on it (gg_label_propagation,
Engine.label_propagation), the partition edge counts (gg_partition_edges, Engine.partition_edges / modularity) and the
graph_cluster / *_mod results lines on the device.

Everything is an integer, so every comparison is EXACT equality with the restatement in dicts and sets
(tests/support/communities_ref.py), on a graph whose nodes take every path of the sweep: lane groups of 4, 16 and 64, the LDS
table, and the table in global memory."""
import ctypes

import numpy as np
import pytest

from tests.support import communities_ref as ref
from tests.support import label_spread_ref as ls

pytestmark = pytest.mark.gpu

TOP = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def engine_for(ga, n, edges=None):
    table = np.zeros((n, 4), np.float32)  # (the sweeps read no embedding)
    eng = ga.Engine(table, table)
    if edges is not None:
        eng.set_graph_csr(*ga.edges_to_csr(n, edges))
    return eng


@pytest.fixture(scope="module")
def ladder(ga):
    """the degree ladder with the hubs, one of them above the LDS table's capacity, resident, with its neighbour sets: shared,
    never changed"""
    cap = ga.Engine.NEIGHBOR_MODE_LDS_CAP
    n, edges, info = ref.ladder_graph(cap)
    assert n <= 70000
    N = ref.neighbor_sets(n, edges)
    deg = np.array([len(s) for s in N])
    assert deg[info["probes"]].tolist() == list(ls.LENGTHS) and deg[info["hub_a"]] == ls.HUB_A and deg[info["hub_b"]] == ls.HUB_B
    assert [int(deg[info[k]]) for k in ("p15", "p16", "p17")] == [15, 16, 17] and deg[info["isolated"]] == 0
    assert ls.HUB_A <= cap < deg[info["giant"]] == cap + 37  # hub A fills an LDS table, the giant does not fit one
    eng = engine_for(ga, n, edges)
    assert eng.distinct_degrees().tolist() == deg.tolist()
    special = np.array([info[k] for k in ("hub_a", "hub_b", "giant", "isolated", "p15", "p16", "p17")] + info["probes"].tolist())
    yield dict(n=n, N=N, deg=deg, eng=eng, special=special, edges=edges, **info)
    eng.close()


def colliding_labels(n):
    """labels 2^22 apart (every one lands on slot 0 of a table of up to 2^22 slots) and their mirror images below 2^31 - 1 (slot
    T - 1, so the probe chains wrap round), 2^31 - 1 itself among them"""
    j = (np.arange(n) // 2) % 500
    lab = np.where(np.arange(n) % 2 == 0, j << 22, TOP - (j << 22)).astype(np.int64)
    assert lab.min() >= 0 and lab.max() == TOP
    return lab


def test_neighbor_mode_on_every_path_under_general_label_fields(ladder):
    g, rs = ladder, np.random.RandomState(1)
    eng, n, N = g["eng"], g["n"], g["N"]
    fields = dict(distinct=rs.permutation(n), equal=np.full(n, 5), few=rs.randint(0, 3, n), colliding=colliding_labels(n),
                  wide=rs.randint(0, TOP, n))
    for name, labels in fields.items():
        for salt, keep in ((0, True), (0x9E3779B9, False)):
            res = eng.neighbor_mode(labels, salt=salt, keep=keep)
            assert res["out"].dtype == np.int32 and res["out"].shape == (n,) and res["ms"] >= 0.0
            want = ref.neighbor_mode(N, labels, salt, keep)
            assert res["out"].tolist() == want, (name, salt, keep, np.flatnonzero(res["out"] != np.array(want))[:5])
    out = eng.neighbor_mode(fields["distinct"])["out"]
    assert out[g["isolated"]] == fields["distinct"][g["isolated"]]  # no neighbour: the node's own label
    assert np.all(eng.neighbor_mode(fields["equal"])["out"] == 5)


@pytest.mark.parametrize("target", ("p16", "p17", "hub_a", "hub_b", "giant", 4, 8))
def test_exact_ties_are_decided_by_the_salt_and_by_keep(ladder, target):
    """the target's neighbours carry two labels exactly equally often (an odd one out carries a third)"""
    g = ladder
    eng, n, N = g["eng"], g["n"], g["N"]
    v = int(g[target]) if isinstance(target, str) else int(g["probes"][target])
    nb = sorted(N[v])
    A, B, C = 1000, 77, 3
    labels = np.full(n, C)
    labels[nb[:len(nb) // 2]] = A
    labels[nb[len(nb) // 2:2 * (len(nb) // 2)]] = B
    # three salts that do not all choose the same label
    salts = [0]
    winner = lambda s: A if (ref.fmix32(A ^ s), A) < (ref.fmix32(B ^ s), B) else B  # noqa: E731
    salts.append(next(s for s in range(1, 100) if winner(s) != winner(0)))
    salts.append(0xFFFFFFFF)
    for s in salts:
        got = eng.neighbor_mode(labels, salt=s, nodes=[v])["out"].tolist()
        assert got == [winner(s)] == ref.neighbor_mode(N, labels, s, True, [v]), (s, got)
        assert eng.neighbor_mode(labels, salt=s)["out"].tolist() == ref.neighbor_mode(N, labels, s, True)
    assert {winner(s) for s in salts} == {A, B}
    # the node's own label tied at the maximum: kept with keep, decided by the hash without
    s = salts[0]
    loser = B if winner(s) == A else A
    labels[v] = loser
    assert eng.neighbor_mode(labels, salt=s, keep=True, nodes=[v])["out"].tolist() == [loser] == ref.neighbor_mode(N, labels, s, True, [v])
    assert eng.neighbor_mode(labels, salt=s, keep=False, nodes=[v])["out"].tolist() == [winner(s)] == ref.neighbor_mode(N, labels, s, False, [v])
    labels[v] = C  # an own label below the maximum is not kept
    assert eng.neighbor_mode(labels, salt=s, keep=True, nodes=[v])["out"].tolist() == [winner(s)]


def test_requests_do_not_change_a_nodes_value(ladder):
    g, rs = ladder, np.random.RandomState(7)
    eng, n = g["eng"], g["n"]
    labels = np.where(rs.random_sample(n) < 0.5, rs.randint(0, 4, n), colliding_labels(n))
    full = eng.neighbor_mode(labels, salt=11)["out"]
    assert full.tolist() == ref.neighbor_mode(g["N"], labels, 11, True)
    assert np.array_equal(eng.neighbor_mode(labels, salt=11)["out"], full)  # a rerun
    perm = rs.permutation(n)
    assert np.array_equal(eng.neighbor_mode(labels, salt=11, nodes=perm)["out"], full[perm])  # None against a permutation
    for m in (1, 63, 64, 65):
        nodes = np.concatenate([g["special"], rs.randint(0, n, 65)])[:m] if m > 1 else np.array([g["giant"]])
        assert np.array_equal(eng.neighbor_mode(labels, salt=11, nodes=nodes)["out"], full[nodes]), m  # a subset
    rep = np.array([g["giant"], 5, g["hub_a"], g["giant"], 5, g["probes"][9], g["hub_a"], g["giant"]])
    assert np.array_equal(eng.neighbor_mode(labels, salt=11, nodes=rep)["out"], full[rep])  # repeated ids: a table per occurrence
    assert eng.neighbor_mode(labels, nodes=np.zeros(0, np.int64))["out"].shape == (0,)  # m = 0


@pytest.fixture(scope="module")
def big(ga):
    n, rs = 70000, np.random.RandomState(3)
    edges = rs.randint(0, n, size=(200000, 2)).astype(np.int32)
    N = ref.neighbor_sets(n, edges)
    deg = np.array([len(s) for s in N])
    assert ((deg > 4) & (deg <= 16)).sum() > 2048 * 16  # more 16-lane tasks than one launch has groups: they stride
    eng = engine_for(ga, n, edges)
    yield dict(n=n, N=N, eng=eng)
    eng.close()


def test_more_tasks_than_one_launch_has_groups(big):
    n, N, eng, rs = big["n"], big["N"], big["eng"], np.random.RandomState(4)
    labels = rs.randint(0, 50, n)
    out = eng.neighbor_mode(labels, salt=3, keep=False)["out"]
    assert out.tolist() == ref.neighbor_mode(N, labels, 3, False)
    perm = rs.permutation(n)
    assert np.array_equal(eng.neighbor_mode(labels, salt=3, keep=False, nodes=perm)["out"], out[perm])
    assign = rs.randint(-1, 128, n)
    res = eng.partition_edges(assign, 128)
    intra, tot = ref.partition_edges(N, assign, 128)
    assert res["intra"].tolist() == intra and res["tot"].tolist() == tot


def test_a_new_graph_drops_the_plans(ga):
    """the second graph moves the hub to another node and shortens it below the LDS table's capacity: a kept plan would send
    the wrong node to the table in global memory"""
    cap = ga.Engine.NEIGHBOR_MODE_LDS_CAP
    n, rs = cap + 400, np.random.RandomState(4)
    labels = rs.randint(0, 6, n)
    assign = rs.randint(-1, 3, n)
    eng = engine_for(ga, n)
    outs = []
    for hub_node, hub_deg in ((0, cap + 50), (7, 600), (0, cap + 50)):
        others = np.setdiff1d(np.arange(n), [hub_node])
        edges = np.concatenate([np.stack([np.full(hub_deg, hub_node), others[:hub_deg]], axis=1), rs.randint(0, n, size=(2000, 2))]).astype(np.int32)
        eng.set_graph_csr(*ga.edges_to_csr(n, edges))
        N = ref.neighbor_sets(n, edges)
        outs.append(eng.neighbor_mode(labels, salt=1, keep=False)["out"])
        assert outs[-1].tolist() == ref.neighbor_mode(N, labels, 1, False), (hub_node, hub_deg)
        assert np.array_equal(eng.neighbor_mode(labels, salt=1, keep=False, nodes=[hub_node, 3])["out"], outs[-1][[hub_node, 3]])
        res = eng.partition_edges(assign, 3)
        assert (res["intra"].tolist(), res["tot"].tolist()) == ref.partition_edges(N, assign, 3)
    eng.close()


def composed(eng, n, seed, T):
    """T iterations as 2 T neighbor_mode calls composed on the host -> (labels, iters, converged, changed)"""
    L, ids = np.arange(n, dtype=np.int32), range(n)
    changed, t, converged = [], 0, False
    while t < T and not converged:
        t += 1
        st = ref.side_state(seed, t)
        side = np.array([ref.fmix32(v ^ st) & 1 for v in ids])
        moved = 0
        for h in (0, 1):
            new = np.where(side == h, eng.neighbor_mode(L, salt=ref.salt_of(seed, t, h), keep=True)["out"], L).astype(np.int32)
            moved += int((new != L).sum())
            L = new
        changed.append(moved)
        converged = moved == 0
    return L, t, converged, changed


@pytest.mark.parametrize("T", (1, 2, 7))
def test_label_propagation_equals_the_composed_primitive(ladder, T):
    g = ladder
    eng, n = g["eng"], g["n"]
    for seed in (0, 0xFFFFFFFF):
        res = eng.label_propagation(seed=seed, max_iters=T)
        L, t, conv, changed = composed(eng, n, seed, T)
        assert res["labels"].dtype == np.int32 and res["changed"].dtype == np.int64 and res["ms"] >= 0.0
        assert res["labels"].tolist() == L.tolist() and res["iters"] == t and res["converged"] == conv and res["changed"].tolist() == changed
    want = ref.label_propagation(g["N"], 0xFFFFFFFF, T)
    assert (res["labels"].tolist(), res["iters"], res["converged"], res["changed"].tolist()) == want
    assert res["changed"][0] > 0 and res["labels"][g["isolated"]] == g["isolated"]


@pytest.mark.parametrize("seed", (0, 1))
def test_full_fit_on_the_planted_partition(ga, seed):
    from graphgan_amd.evaluation import graph_communities as gcomm
    n = 256
    edges, lab, _, _ = ls.planted_partition(seed)
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    for s in (0, 1, 2):
        res = eng.label_propagation(seed=s, max_iters=100)
        L, t, conv, changed = ref.label_propagation(N, s, 100)
        assert res["labels"].tolist() == L and res["iters"] == t and res["converged"] == conv and res["changed"].tolist() == changed
        assert conv and t < 100
        comm, k = gcomm.relabel(res["labels"])
        assert (comm.tolist(), k) == ref.relabel(L)
        q = eng.modularity(comm)
        assert q == ref.modularity(*ref.partition_edges(N, comm.tolist(), k))
        print("planted partition graph=%d seed=%d: iters=%d communities=%d Q=%.4f" % (seed, s, t, k, q))
    eng.close()


def test_full_fit_on_ca_grqc(ga):
    from graphgan_amd.evaluation import graph_communities as gcomm
    from tests.helpers import load_ca_grqc
    d, n, _ = load_ca_grqc()
    edges = np.asarray(d["train"])
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    res = eng.label_propagation(seed=0, max_iters=100)
    L, t, conv, changed = ref.label_propagation(N, 0, 100)
    assert res["labels"].tolist() == L and res["iters"] == t and res["converged"] == conv and res["changed"].tolist() == changed
    comm, k = gcomm.relabel(res["labels"])
    cnt = eng.partition_edges(comm, k)
    assert (cnt["intra"].tolist(), cnt["tot"].tolist()) == ref.partition_edges(N, comm.tolist(), k)
    print("CA-GrQc seed=0: iters=%d converged=%s communities=%d (with an edge: %d) Q=%.4f fit_ms=%.3f" % (
        t, conv, k, int((cnt["tot"] > 0).sum()), gcomm.modularity_from_counts(cnt["intra"], cnt["tot"]), res["ms"]))
    eng.close()


@pytest.mark.parametrize("n_label", (1, 2, 128, "n_node"))
def test_partition_edges_against_the_restatement(ladder, n_label):
    g, rs = ladder, np.random.RandomState(20)
    eng, n, N = g["eng"], g["n"], g["N"]
    k = n if n_label == "n_node" else n_label
    fields = [rs.randint(-1, k, n), np.where(rs.random_sample(n) < 0.5, -1, rs.randint(0, k, n)), np.full(n, k - 1), np.full(n, -1)]
    if k >= 128:
        fields.append(3 * rs.randint(0, k // 3, n))  # empty classes
    if k == n:
        fields.append(np.arange(n))  # singletons: no inner edge
    for assign in fields:
        for hub in ("hub_a", "hub_b", "giant"):
            assign[g[hub]] = rs.randint(0, k)  # (the chunked lists are always inside)
        res = eng.partition_edges(assign, k)
        intra, tot = ref.partition_edges(N, assign, k)
        assert res["intra"].dtype == res["tot"].dtype == np.int64 and res["ms"] >= 0.0
        assert res["intra"].tolist() == intra and res["tot"].tolist() == tot
        q, want = eng.modularity(assign), ref.modularity(intra, tot)
        assert q == want or (np.isnan(q) and np.isnan(want))
    assert np.isnan(eng.modularity(np.full(n, -1)))
    assert not eng.partition_edges(np.arange(n), n)["intra"].any()


def test_results_lines_with_an_engine_are_string_equal_to_the_host_evaluators(ga, tmp_path):
    from graphgan_amd.evaluation import graph_communities as gcomm
    n, rs = 256, np.random.RandomState(2)
    edges, lab, _, _ = ls.planted_partition(1)
    train_file, labels_file = str(tmp_path / "train.txt"), str(tmp_path / "labels.txt")
    np.savetxt(train_file, edges, fmt="%d")
    nodes = np.sort(rs.permutation(n)[:150])
    with open(labels_file, "w") as f:
        f.writelines("%d %d\n" % (v, 10 * lab[v]) for v in nodes.tolist())
    eng = engine_for(ga, n, edges)
    kw = dict(n_init=3, max_iters=100, seed=5)
    dev = gcomm.GraphCommunityEval(train_file, labels_file, n, engine=eng, **kw).eval_graph_communities()
    host = gcomm.GraphCommunityEval(train_file, labels_file, n, **kw).eval_graph_communities()
    line = gcomm.format_results(dev)
    assert line == gcomm.format_results(host)
    assert line.startswith("graph_cluster:NMI=") and " n=150 iters=" in line and line.endswith(" converged=True seed=%d\n" % dev["seed"])
    assert dev["seed"] in (5, 6, 7) and 0.0 < dev["Q"] < 1.0 and dev["NMI"] > 0.5
    # the *_mod lines of a partition of the labelled nodes
    part = dict(nodes=nodes, classes=lab[nodes], assign=rs.randint(0, 5, len(nodes)), k=5, n_labels=4)
    dev_m = gcomm.eval_cluster_modularity(gcomm.engine_sweeps(eng)[1], n, part)
    host_m = gcomm.eval_cluster_modularity(gcomm.host_sweeps(edges, n)[1], n, part)
    for mode in ("gen", "dis"):
        assert gcomm.format_modularity(mode, dev_m) == gcomm.format_modularity(mode, host_m)
    assert gcomm.format_modularity("gen", dev_m).startswith("gen_mod:Q=") and dev_m["label_Q"] > 0.3 > abs(dev_m["Q"]) and dev_m["edges"] > 0
    eng.close()


def test_refusals_name_the_function_and_the_value(ga):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    lab = np.arange(n, dtype=np.int32)
    for call, name in ((lambda: eng.neighbor_mode(lab), "gg_neighbor_mode"), (lambda: eng.label_propagation(), "gg_label_propagation"),
                       (lambda: eng.partition_edges(lab, n), "gg_partition_edges"), (lambda: eng.modularity(lab), "gg_partition_edges")):
        with pytest.raises(ga.GraphGANHipError) as ei:
            call()
        assert ei.value.code == ga.GG_EINVAL and "%s: needs the training graph (gg_set_graph_csr)" % name in str(ei.value)
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
    bad = lab.copy()
    bad[[7, 9]] = -3, -1
    refused(lambda: eng.neighbor_mode(bad), "neighbor_mode: labels[7] = -3 is negative", V)
    refused(lambda: eng.neighbor_mode(lab[:-1]), "neighbor_mode: labels must be an int array [50]", V)
    refused(lambda: eng.neighbor_mode(lab.astype(np.float32)), "neighbor_mode: labels must be an int array [50]", V)
    refused(lambda: eng.neighbor_mode(lab, nodes=[0, 3, 50]), "neighbor_mode: nodes[2] = 50 out of range [0, 50)", V)
    refused(lambda: eng.neighbor_mode(lab, nodes=[-1, 3]), "neighbor_mode: nodes[0] = -1 out of range [0, 50)", V)
    refused(lambda: eng.label_propagation(max_iters=0), "label_propagation: max_iters = 0 is below 1", V)
    refused(lambda: eng.label_propagation(max_iters=2.5), "label_propagation: max_iters = 2.5 is below 1", V)
    refused(lambda: eng.partition_edges(lab, 49), "partition_edges: assign[49] = 49 outside [-1, 49)", V)
    refused(lambda: eng.partition_edges(bad, 50), "partition_edges: assign[7] = -3 outside [-1, 50)", V)
    refused(lambda: eng.partition_edges(lab, 0), "partition_edges: n_label = 0 is below 1", V)
    refused(lambda: eng.partition_edges(lab[:-1], 50), "partition_edges: assign must be an int array [50]", V)
    refused(lambda: eng.modularity(bad), "modularity: assign[7] = -3 outside [-1, 50)", V)

    # through the C ABI
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out, nodes2 = np.full(n, -7, np.int32), np.array([0, 7], np.int32)
    it, cv, ch = ctypes.c_int32(), ctypes.c_int32(), np.zeros(4, np.int32)
    intra, tot = np.zeros(3, np.int64), np.zeros(3, np.int64)
    assign = (lab % 3).astype(np.int32)

    def raw_nm(labels=lab, nodes=nodes2, m=2, out=out):
        return lambda: _lib.check(L.gg_neighbor_mode(eng._ctx, p(labels), 5, 1, p(nodes), m, p(out), None), eng._ctx)

    def raw_lp(max_iters=4, labels=out, iters=it, conv=cv, changed=ch):
        return lambda: _lib.check(L.gg_label_propagation(eng._ctx, 0, max_iters, p(labels), None if iters is None else ctypes.byref(iters),
                                                         None if conv is None else ctypes.byref(conv), p(changed), None), eng._ctx)

    def raw_pe(assign=assign, k=3, intra=intra, tot=tot):
        return lambda: _lib.check(L.gg_partition_edges(eng._ctx, p(assign), k, p(intra), p(tot), None), eng._ctx)

    raw_nm()()  # (kernel_ms may be NULL)
    assert np.all(out[2:] == -7)  # only m rows are written
    assert out[:2].tolist() == ref.neighbor_mode(ref.neighbor_sets(n, ring_edges), lab, 5, True, [0, 7])  # (both neighbours once: the smaller hash)
    for kw in (dict(labels=None), dict(out=None)):
        refused(raw_nm(**kw), "gg_neighbor_mode: labels and out must not be NULL")
    refused(raw_nm(m=-1), "gg_neighbor_mode: m = -1 is negative")
    refused(raw_nm(labels=bad), "gg_neighbor_mode: labels[7] = -3 is negative")
    refused(raw_nm(nodes=np.array([0, 50], np.int32)), "gg_neighbor_mode: nodes[1] = 50 out of range [0, 50)")
    refused(raw_nm(nodes=np.array([-2, 5], np.int32)), "gg_neighbor_mode: nodes[0] = -2 out of range [0, 50)")
    raw_nm(labels=None, out=None, m=0)()  # m == 0 succeeds and touches nothing
    refused(raw_lp(max_iters=0), "gg_label_propagation: max_iters = 0 is below 1")
    refused(raw_lp(max_iters=-4), "gg_label_propagation: max_iters = -4 is below 1")
    for kw in (dict(labels=None), dict(iters=None), dict(conv=None), dict(changed=None)):
        refused(raw_lp(**kw), "gg_label_propagation: labels, iters, converged and changed must not be NULL")
    for kw in (dict(assign=None), dict(intra=None), dict(tot=None)):
        refused(raw_pe(**kw), "gg_partition_edges: assign, intra and tot must not be NULL")
    refused(raw_pe(k=0), "gg_partition_edges: n_label = 0 is below 1")
    refused(raw_pe(k=2), "gg_partition_edges: assign[2] = 2 outside [-1, 2)")
    refused(raw_pe(assign=np.where(bad < 0, bad, assign).astype(np.int32)), "gg_partition_edges: assign[7] = -3 outside [-1, 3)")
    raw_pe()()  # the engine stays usable
    assert int(tot.sum()) == 2 * n and int(intra.sum()) == 0  # a ring of 50 with classes v mod 3: the ends 49 - 0 differ too
    raw_lp()()
    assert 1 <= it.value <= 4 and ch[0] > 0
    eng.close()
