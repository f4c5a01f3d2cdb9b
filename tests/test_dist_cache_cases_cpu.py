"""The CPU side of the distribution-cache matrix (tests/test_gpu_dist_cache.py): every precondition its lazy cases rest on,
asserted on the C oracle's own walks and on BFS levels computed here -- wherever the suite runs, with or without a GPU.

A lazy case names the launch in which a slot is rebuilt whole.  Whether a launch asks for a rebuild is decided by where its
walks stand, and walks are counter based: a property of (graph, tables, seed, stream), chosen in
tests/support/dist_cache_cases.py by scanning seeds against these very checks.  If a change to the oracle, the graph or the
seed breaks one of them, the GPU cases would pass while testing nothing: this file fails instead."""
import numpy as np
import pytest

from tests.support import dist_cache_cases as dc


def case_named(name):
    return [c for c in dc.LAZY_CASES if c["name"] == name][0]


def test_lazy_graph_shape():
    """Symmetric sorted adjacency; every regular tree is larger than the node limit, BFS numbered, exact through level 2 by the
    engine's build rule, and regular around levels 2 and 3 (a father and C children each); the two small components."""
    g = dc.lazy_graph()
    n, rowptr, col = g["n"], g["rowptr"], g["col"]
    assert n <= 1000 and g["E"].shape == (n, dc.D_LAZY)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    fwd = set(zip(src.tolist(), col.tolist()))
    assert all((v, u) in fwd for u, v in fwd) and all(u != v for u, v in fwd)
    for v in range(n):
        assert np.all(np.diff(col[rowptr[v]: rowptr[v + 1]]) > 0)
    deg = np.diff(rowptr)
    for t in g["trees"]:
        level, father, order = dc.bfs_levels(n, rowptr, col, t["root"])
        assert len(order) > dc.CAP                                    # larger than whole_max: built lazy
        assert deg[t["root"]] + 1 <= dc.CAP                           # (a root whose own children exceed the limit is built whole)
        assert np.array_equal(order, t["root"] + np.arange(len(order)))   # rank = node id - root id
        assert dc.predicted_exact_level(rowptr, level, order, dc.CAP) == (dc.L_EXACT, dc.LZS, dc.P_EXACT)
        kids = np.bincount(father[order[1:]], minlength=n)
        for lv in (dc.L_EXACT, dc.L_EXACT + 1):
            assert np.all(kids[order[level[order] == lv]] == dc.C)
        deep = order[level[order] == dc.L_EXACT + 2]
        hot = deep[kids[deep] > 0]
        assert len(hot) == (0 if t["kind"] == "quiet" else 1) and (len(hot) == 0 or int(hot[0]) == t["Z"])
        assert level.max() == (dc.L_EXACT + 2 if t["kind"] == "quiet" else dc.L_EXACT + 3)
        assert int(order[level[order] == dc.L_EXACT][0]) == t["F0"] and father[t["B"]] == t["A1"] != t["A0"]
        assert np.all(father[t["X"]] == t["B"]) and np.all(father[t["Y"]] == t["F0"])
    assert deg[g["pair_root"]] == 1 and deg[g["iso"]] == 0
    assert [t["kind"] for t in g["trees"]] == list(dc.KINDS)


@pytest.mark.parametrize("name", ["lazy_fallback_in_g", "lazy_fallback_in_g_arena1", "lazy_fallback_in_g_begin"])
def test_target_trees_are_rebuilt_in_the_g_launch_only(name):
    case = case_named(name)
    facts = dc.check_target(case, 0)
    targets = [f for kind, f in facts.values() if kind == "target"]
    assert len(targets) == 2 == case["fallback"][0][1] and case["fallback"][0][0] == 0
    for f in targets:
        # no D-mode walk (deg(root) walks, stream 0) stands on a non-leaf node of level L + 2 or deeper ...
        assert len(f["d_deep_nonleaf"]) == 0
        # ... at least one G-mode walk (n_sample walks, stream 1) does
        assert len(f["g_deep_nonleaf"]) >= 1
        # the D-mode walks stood on a level-(L+1) node with k >= 2 whose father is not the first level-L node ...
        assert len(f["d_L1_foreign"]) >= 1
        # ... and the G-mode walks on a level-(L+1) node under the first level-L node
        assert len(f["g_L1_first"]) >= 1
        # The D-mode walks stood on ONE level-L node: its list is the first in the pool whatever order a launch resolves lists in,
        # so the registered pool ranks are known, and at least one G-mode walk of the rerun would pick another node from the stale
        # entry than from its own distribution (restated with the spec's arithmetic): the defect changes an array, certainly.
        assert len(f["d_L_nodes"]) == 1 and int(f["d_L_nodes"][0]) != f["first_L"]
        assert len(f["changed"]) >= 1
    # the quiet tree of the same launch never asks
    for kind, f in facts.values():
        if kind == "quiet":
            assert len(f["d_deep_nonleaf"]) == 0 and len(f["g_deep_nonleaf"]) == 0


def test_epoch_case_walks_are_the_prepare_case_walks():
    """gg_epoch_add walks with streams 0 and 1 and the walks are keyed by root id, not slot: batch 0 of the epoch case is round 0
    of the prepare case for the target trees, batch 1 its quiet tree."""
    case, ep = case_named(dc.DEFECT_CASE), dc.EPOCH_CASE
    assert ep["seed"] == case["seed"] and ep["n_sample"] == case["n_sample"] and ep["env"] == case["env"]
    g = dc.lazy_graph()
    kinds = {t["root"]: t["kind"] for t in g["trees"]}
    assert [kinds.get(int(r)) for r in ep["batches"][0]] == ["target", "target", None, None]
    assert [kinds.get(int(r)) for r in ep["batches"][1]] == ["quiet"]
    assert set(ep["batches"][0].tolist()) | set(ep["batches"][1].tolist()) == set(case["roots"].tolist())


def test_loud_tree_is_rebuilt_in_the_d_launch():
    case = case_named("lazy_fallback_in_d")
    facts = dc.check_target(case, 0)
    assert sorted(kind for kind, _ in facts.values()) == ["loud", "quiet"]
    for kind, f in facts.values():
        assert len(f["d_deep_nonleaf"]) == (1 if kind == "loud" else 0)
        assert kind == "loud" or len(f["g_deep_nonleaf"]) == 0
    assert case["fallback"] == [(1, 0), (0, 0)]


def test_quiet_tree_never_asks_for_its_whole_tree():
    case = case_named("lazy_no_fallback")
    for r in range(case["rounds"]):
        for kind, f in dc.check_target(case, r).values():
            assert kind == "quiet" and len(f["d_deep_nonleaf"]) == 0 and len(f["g_deep_nonleaf"]) == 0
    assert case["fallback"] == [(0, 0), (0, 0)]


def test_every_root_status_occurs_and_every_case_has_work():
    """root_status 0 (walks), 1 (the pair's root in D-mode: its only child has no children) and 2 (the isolated node in D-mode:
    no walks requested) all occur in a lazy case; 1 again for the isolated node in G-mode (the tree only has a root)."""
    rounds = dc.oracle_rounds(case_named(dc.DEFECT_CASE))
    d, g = rounds[0]
    assert set(d["root_status"].tolist()) == {0, 1, 2}
    assert set(g["root_status"].tolist()) == {0, 1}
    for d, g in rounds:
        assert len(d["center"]) > 0 and len(g["node_1"]) > 0
    for case in dc.WHOLE_CASES[:1]:
        for d, g in dc.oracle_rounds(case):
            assert len(d["center"]) > 1000 and len(g["node_1"]) > 10000
    wg = dc.whole_graph()
    assert (np.diff(wg["rowptr"]) > 16).sum() > 50  # lists of more than one 16-candidate chunk
