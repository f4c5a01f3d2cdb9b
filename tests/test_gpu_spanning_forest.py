"""The spanning-forest sweep on the device (gg_undirected_edges / gg_spanning_forest, Engine.undirected_edges / spanning_forest /
connected_components) and the edge-list split on it (graphgan_amd/split.py with an engine, the command line).

Everything is an integer and the minimum spanning forest under distinct keys is unique, so every comparison is EXACT equality
with the Kruskal restatement (tests/support/spanning_forest_ref.py); ``rounds`` is compared with the numpy rounds of the host
path and with the bound ceil(log2 n) + 1."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import communities_ref as cref
from tests.support import spanning_forest_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP32 = 2 ** 32 - 1


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def sp():
    from graphgan_amd import split
    return split


def engine_for(ga, n, edges=None):
    table = np.zeros((n, 4), np.float32)  # (the sweep reads no embedding)
    eng = ga.Engine(table, table)
    if edges is not None:
        eng.set_graph_csr(*ga.edges_to_csr(n, edges))
    return eng


def check(eng, sp, n, edges, seed=0, prio=None):
    """one call against the restatement, the host rounds and the bound -> the device's result"""
    E, forest, component, k = ref.forest_of(n, edges, seed, prio)
    m = len(E)
    got_E = eng.undirected_edges()
    assert got_E.dtype == np.int32 and got_E.shape == (m, 2) and got_E.tolist() == [list(e) for e in E]
    res = eng.spanning_forest(seed=seed, priority=prio, sweeps=True)
    assert res["forest"].dtype == np.uint8 and res["forest"].shape == (m,) and res["component"].dtype == np.int32 and res["ms"] >= 0.0
    bad = np.flatnonzero(res["forest"] != np.array(forest, dtype=np.uint8))
    assert bad.size == 0, (seed, bad[:5])
    assert res["component"].tolist() == component
    assert (res["m"], res["n_forest"], res["n_components"]) == (m, sum(forest), k)
    host = sp.host_spanning_forest(got_E, n, seed=seed, priority=prio)
    assert res["rounds"] == host["rounds"] <= math.ceil(math.log2(max(n, 2))) + 1
    assert res["sweep_live"].tolist() == host["sweep_live"].tolist() and res["sweep_hooks"].tolist() == host["sweep_hooks"].tolist()
    assert np.array_equal(host["forest"], res["forest"]) and np.array_equal(host["component"], res["component"])
    return res


SMALL = {
    "no_edge": lambda: (7, np.zeros((0, 2), np.int32)),
    "single_edge": lambda: (5, np.array([[3, 1]], np.int32)),
    "two_nodes": lambda: (2, np.array([[0, 1], [1, 0]], np.int32)),
    "cycle64": lambda: ref.cycle_graph(64),
    "cycle65": lambda: ref.cycle_graph(65),
    "k65": lambda: ref.complete_graph(65),
    "star": lambda: ref.star_graph(3 * 512 + 17),
    "star_hub_last": lambda: ref.star_graph(3 * 512 + 17, hub=3 * 512 + 17),
    "two_hubs": lambda: ref.two_hubs(3 * 512 + 17),
    "triangles": lambda: ref.triangles(1000, 37),
    "permuted_path": lambda: ref.permuted(*ref.path_graph(1025)),
    "permuted_triangles": lambda: ref.permuted(*ref.triangles(1000, 37)),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_graphs_against_kruskal(ga, sp, name):
    n, edges = SMALL[name]()
    eng = engine_for(ga, n, edges)
    for seed in (0, 1, 0xFFFFFFFF):
        res = check(eng, sp, n, edges, seed)
    m = res["m"]
    if m:
        rs = np.random.RandomState(1)
        for prio in (np.zeros(m, np.uint32), np.full(m, TOP32, np.uint32), rs.randint(0, 3, m) * (TOP32 // 2), rs.randint(0, 2 ** 32, m)):
            check(eng, sp, n, edges, prio=prio)
    if name == "no_edge":
        assert res["rounds"] == 0 and res["n_components"] == n and res["component"].tolist() == list(range(n)) and len(res["sweep_live"]) == 0
    if name in ("single_edge", "two_nodes"):
        assert res["rounds"] == 1 and res["n_forest"] == 1 and res["forest"].tolist() == [1]  # the two ends choose each other: one hook
    if name.startswith("permuted"):
        comp = res["component"]
        assert np.any(comp != np.arange(n)) and np.all(comp <= np.arange(n))
    eng.close()


def test_path_of_1025_nodes_one_round_hooks_a_chain_of_1024(ga, sp):
    n, edges = ref.path_graph(1025)
    eng = engine_for(ga, n, edges)
    m = n - 1
    up = check(eng, sp, n, edges, prio=np.arange(m))  # node v > 0 takes the edge behind it: one chain through every node
    assert up["rounds"] == 1 and up["sweep_hooks"].tolist() == [m, 0] and up["forest"].all() and not up["component"].any()
    down = check(eng, sp, n, edges, prio=np.arange(m)[::-1].copy())
    assert down["rounds"] == 1 and down["forest"].all()
    tie = check(eng, sp, n, edges, prio=np.full(m, 7))  # all equal: the tie falls to j, the ascending case again
    assert tie["rounds"] == 1 and tie["sweep_hooks"].tolist() == up["sweep_hooks"].tolist()
    mixed = check(eng, sp, n, edges, prio=np.where(np.arange(m) % 2, 0, TOP32))
    assert mixed["rounds"] == 2
    eng.close()


def test_duplicates_and_self_loops_in_the_csr(ga, sp):
    n, rs = 300, np.random.RandomState(2)
    base = rs.randint(0, n, size=(260, 2)).astype(np.int32)
    loops = np.stack([np.arange(0, n, 7)] * 2, axis=1).astype(np.int32)
    edges = np.concatenate([base, base[:100], base[50:150, ::-1], loops, loops[:5]])
    eng = engine_for(ga, n, edges[rs.permutation(len(edges))])
    res = check(eng, sp, n, edges)
    clean = engine_for(ga, n, base)
    res2 = clean.spanning_forest()
    assert np.array_equal(res["forest"], res2["forest"]) and np.array_equal(res["component"], res2["component"])
    assert np.array_equal(eng.undirected_edges(), clean.undirected_edges())
    eng.close()
    clean.close()


def test_degree_ladder(ga, sp):
    n, edges, info = cref.ladder_graph(ga.Engine.NEIGHBOR_MODE_LDS_CAP)
    eng = engine_for(ga, n, edges)
    for seed in (0, 1):
        res = check(eng, sp, n, edges, seed)
    assert res["component"][info["isolated"]] == info["isolated"]
    assert eng.connected_components().tolist() == res["component"].tolist()
    eng.close()


@pytest.fixture(scope="module")
def big(ga):
    n, edges = ref.random_graph()
    eng = engine_for(ga, n, edges)
    yield dict(n=n, edges=edges, eng=eng)
    eng.close()


def test_random_graph_many_blocks_thousands_of_components(big, sp):
    eng, n, edges = big["eng"], big["n"], big["edges"]
    res = check(eng, sp, n, edges, 0)
    assert res["m"] > 100000 and res["n_components"] > 2000 and res["rounds"] >= 5
    check(eng, sp, n, edges, 0xFFFFFFFF)
    check(eng, sp, n, edges, prio=np.random.RandomState(3).randint(0, 4, res["m"]))  # heavy ties: the edge index decides
    again = eng.spanning_forest(seed=0)  # a rerun is bit-equal
    assert np.array_equal(again["forest"], res["forest"]) and np.array_equal(again["component"], res["component"])
    assert (again["m"], again["n_forest"], again["n_components"], again["rounds"]) == (res["m"], res["n_forest"], res["n_components"], res["rounds"])
    assert eng.connected_components().tolist() == ref.forest_of(n, edges, 0)[2]


def test_ca_grqc_union(ga, sp):
    n, edges = ref.ca_grqc_union()
    eng = engine_for(ga, n, edges)
    for seed in (0, 1, 0xFFFFFFFF):
        res = check(eng, sp, n, edges, seed)
    assert (res["m"], res["n_forest"], res["n_components"]) == (14483, 4887, 355)
    print("CA-GrQc union: m=%d forest=%d components=%d rounds=%d ms=%.3f sweeps live=%s hooks=%s" % (
        res["m"], res["n_forest"], res["n_components"], res["rounds"], res["ms"], res["sweep_live"].tolist(), res["sweep_hooks"].tolist()))
    eng.close()


def test_a_new_graph_drops_the_edge_list(ga, sp):
    """the second graph joins the two components of the first with one more edge: a kept edge list would leave them apart"""
    n = 40
    first = np.array([(i, i + 1) for i in range(19)] + [(i, i + 1) for i in range(20, 39)], dtype=np.int32)
    eng = engine_for(ga, n, first)
    a = check(eng, sp, n, first)
    assert a["n_components"] == 2 and a["component"].tolist() == [0] * 20 + [20] * 20 and a["m"] == 38
    second = np.concatenate([first, [[5, 33]]]).astype(np.int32)
    eng.set_graph_csr(*ga.edges_to_csr(n, second))
    b = check(eng, sp, n, second)
    assert b["n_components"] == 1 and not b["component"].any() and b["m"] == 39 and len(eng.undirected_edges()) == 39
    eng.set_graph_csr(*ga.edges_to_csr(n, first))
    c = check(eng, sp, n, first)
    assert np.array_equal(c["forest"], a["forest"]) and np.array_equal(c["component"], a["component"])
    eng.close()


def test_refusals_and_null_outputs(ga, sp):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    for call, name in ((lambda: eng.undirected_edges(), "gg_undirected_edges"), (lambda: eng.spanning_forest(), "gg_undirected_edges"),
                       (lambda: eng.connected_components(), "gg_undirected_edges")):
        with pytest.raises(ga.GraphGANHipError) as ei:
            call()
        assert ei.value.code == ga.GG_EINVAL and "%s: needs the training graph (gg_set_graph_csr)" % name in str(ei.value)
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    stats = np.zeros(4, np.int64)

    def raw_sf(prio=None, n_prio=0, forest=None, component=None, stats=stats, seed=0):
        return lambda: _lib.check(L.gg_spanning_forest(eng._ctx, seed, p(prio), n_prio, p(forest), p(component), p(stats), None, None, None), eng._ctx)

    def refused(call, text, exc=None):
        with pytest.raises(exc or ga.GraphGANHipError) as ei:
            call()
        assert text in str(ei.value), str(ei.value)
        if exc is None:
            assert ei.value.code == ga.GG_EINVAL

    refused(raw_sf(), "gg_spanning_forest: needs the training graph (gg_set_graph_csr)")
    ring = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int32)
    eng.set_graph_csr(*ga.edges_to_csr(n, ring))
    m = n
    # through Engine
    V = ValueError
    refused(lambda: eng.spanning_forest(priority=np.zeros(m - 1, np.uint32)), "spanning_forest: priority must be a uint32 array [50]", V)
    refused(lambda: eng.spanning_forest(priority=np.zeros((m, 1), np.uint32)), "spanning_forest: priority must be a uint32 array [50]", V)
    refused(lambda: eng.spanning_forest(priority=np.zeros(m, np.float32)), "spanning_forest: priority must be a uint32 array [50]", V)
    refused(lambda: eng.spanning_forest(priority=np.full(m, -1)), "spanning_forest: priority must be a uint32 array [50]: a value outside [0, 2^32)", V)
    refused(lambda: eng.spanning_forest(priority=np.full(m, 2 ** 32)), "spanning_forest: priority must be a uint32 array [50]: a value outside [0, 2^32)", V)
    # through the C ABI
    prio = np.arange(m, dtype=np.uint32)
    refused(raw_sf(prio=prio, n_prio=m - 1), "gg_spanning_forest: priority has 49 entries, the graph has 50 undirected edges")
    refused(raw_sf(prio=prio, n_prio=m + 1), "gg_spanning_forest: priority has 51 entries, the graph has 50 undirected edges")
    refused(raw_sf(stats=None), "gg_spanning_forest: stats must not be NULL")
    with pytest.raises(ga.GraphGANHipError) as ei:
        _lib.check(L.gg_undirected_edges(eng._ctx, None, None), eng._ctx)
    assert ei.value.code == ga.GG_EINVAL and "gg_undirected_edges: m must not be NULL" in str(ei.value)
    # NULL outputs are accepted, each alone and both; the engine stays usable
    want = ref.forest_of(n, ring, prio=prio.tolist())
    forest, component = np.full(m + 3, 9, np.uint8), np.full(n + 3, -7, np.int32)
    raw_sf(prio=prio, n_prio=m)()
    assert stats.tolist() == [m, n - 1, 1, stats[3]] and 1 <= stats[3] <= 7
    raw_sf(prio=prio, n_prio=m, forest=forest)()
    assert forest[:m].tolist() == want[1] and np.all(forest[m:] == 9)
    raw_sf(prio=prio, n_prio=m, component=component)()
    assert component[:n].tolist() == want[2] and np.all(component[n:] == -7)
    forest[:] = 9
    raw_sf(forest=forest, component=component, n_prio=12345)()  # (n_prio is not read with prio NULL)
    assert forest[:m].tolist() == ref.forest_of(n, ring, 0)[1] and np.all(forest[m:] == 9)
    eng.close()


def test_split_with_an_engine_equals_the_host_path(ga, sp, big):
    for n, edges, eng, own in ((*ref.ca_grqc_union(), None, True), (big["n"], big["edges"], big["eng"], False)):
        eng = eng or engine_for(ga, n, edges)
        for kw in (dict(ratio=0.1, seed=0), dict(ratio=0.25, seed=3), dict(ratio=0.1, seed=0, protect="none")):
            dev, host = sp.split_edges(edges, n, engine=eng, **kw), sp.split_edges(edges, n, **kw)
            for x, y in zip(dev[:3], host[:3]):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            assert dev[3] == host[3]
        if own:
            with pytest.raises(ValueError, match="the engine's resident graph is not the graph of `edges`"):
                sp.split_edges(edges[:-5], n, engine=eng)
            eng.close()


def test_command_line_device_files_are_byte_equal_to_host(tmp_path):
    n, edges = ref.ca_grqc_union()
    src = str(tmp_path / "edges.txt")
    np.savetxt(src, edges, fmt="%d")
    outs = {}
    for mode, flag in (("dev", ["--device", "0"]), ("host", ["--host"])):
        prefix = str(tmp_path / mode)
        r = subprocess.run([sys.executable, "-m", "graphgan_amd.split", "--edges", src, "--out-prefix", prefix, "--ratio", "0.1", "--seed", "2"] + flag,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[mode] = (r.stdout, [open(prefix + s, "rb").read() for s in ("_train.txt", "_test.txt", "_test_neg.txt")])
    assert outs["dev"] == outs["host"]
    line = outs["dev"][0]
    assert line.startswith("nodes=%d edges=14483 components=355 " % n) and " test=1448 test_neg=1448 rounds=" in line and all(outs["dev"][1])
