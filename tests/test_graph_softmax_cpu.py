"""The generator's graph softmax on the host (no GPU): the float64 fallback of evaluation/generator_likelihood.py against an
enumeration of every walk and against the sampler mirror's end-node frequencies; the argument checks of
Engine.graph_softmax, the engine_gen_nll knob and the results line."""
import ctypes

import numpy as np
import pytest

from tests.support.graph_softmax_ref import chi2_pvalue_ok, enumerate_walks


@pytest.fixture(scope="module")
def gl():
    # (imported here, not at collection: the library is then loaded in the same order as by the rest of the suite)
    from graphgan_amd.evaluation import generator_likelihood
    return generator_likelihood


def _lists(tree, n, removed=()):
    """dict lists -> (off [n + 1], nbr) in the shape of gg_get_trees; a father in ``removed`` becomes -1 (Q3)."""
    off = np.zeros(n + 1, np.int64)
    nbr = []
    for v in range(n):
        lst = list(tree.get(v, []))
        if v in removed:
            lst[0] = -1
        nbr.extend(lst)
        off[v + 1] = len(nbr)
    return off, np.array(nbr, np.int64)


def _as_reference(tree, removed):
    """the reference's in-place view: a removed father entry is gone from the list"""
    return {v: (lst[1:] if v in removed else list(lst)) for v, lst in tree.items()}


# root 0: children 1, 2, 3; 1 -> 4, 5; 2 is a depth-1 leaf; 3 -> 6; 4 -> 7; 6 -> 8, 9
TREE = {0: [0, 1, 2, 3], 1: [0, 4, 5], 2: [0], 3: [0, 6], 4: [1, 7], 5: [1], 6: [3, 8, 9], 7: [4], 8: [6], 9: [6]}


def _check(gl, emb, bias, root, tree, n, for_d, removed=()):
    off, nbr = _lists(tree, n, removed)
    logp, a = gl.host_graph_softmax(emb, bias, root, off, nbr, for_d)
    P, A = enumerate_walks(emb, bias, root, _as_reference(tree, removed), for_d)
    want = np.full(n, -np.inf)
    for v, pv in P.items():
        want[v] = np.log(pv)
    assert np.array_equal(np.isfinite(logp), np.isfinite(want))
    fin = np.isfinite(want)
    assert np.max(np.abs(np.exp(logp[fin]) - np.exp(want[fin])), initial=0.0) <= 1e-12
    assert abs(a - A) <= 1e-12
    assert abs(np.exp(logp[fin]).sum() + a - 1.0) <= 1e-12
    return logp, a


@pytest.mark.parametrize("for_d", [False, True])
@pytest.mark.parametrize("removed", [(), (1,), (2,), (1, 2, 3)])
def test_host_fallback_equals_enumeration(gl, for_d, removed):
    rng = np.random.RandomState(1)
    n = 12  # nodes 10, 11 are not in the tree
    emb, bias = rng.normal(0, 0.8, (n, 5)), rng.normal(0, 0.5, n)
    logp, a = _check(gl, emb, bias, 0, TREE, n, for_d, removed)
    assert logp[0] == -np.inf and logp[10] == -np.inf and logp[11] == -np.inf
    if for_d or 2 in removed:
        assert a > 0.0  # the depth-1 leaf 2 is a dead end
        assert logp[2] == -np.inf
    else:
        assert a == 0.0 and np.isfinite(logp[2])
    if for_d or 1 in removed:
        assert logp[1] == -np.inf


def test_host_fallback_isolated_root_and_other_roots(gl):
    rng = np.random.RandomState(2)
    n = 12
    emb, bias = rng.normal(0, 1.0, (n, 4)), rng.normal(0, 0.5, n)
    logp, a = _check(gl, emb, bias, 11, {11: [11]}, n, False)
    assert a == 1.0 and np.all(logp == -np.inf)
    _, a = _check(gl, emb, bias, 11, {11: [11]}, n, True)
    assert a == 1.0
    tree = _reroot(TREE, 6)  # the same graph seen from node 6
    for for_d in (False, True):
        _check(gl, emb, bias, 6, tree, n, for_d)
        _check(gl, emb, bias, 6, tree, n, for_d, removed=(3,))


def test_host_fallback_against_the_sampler_mirror(gl):
    """10^5 walks of the reference's sampler restated on numpy (oracle.graphgan_oracle.GraphGANOracle.sample) on a 30-node
    graph: end-node frequencies against host_graph_softmax, chi^2 below its 1e-6 quantile"""
    from oracle import graphgan_oracle as orc
    rng = np.random.RandomState(3)
    n = 30
    edges = set()
    for v in range(1, n):
        edges.add((int(rng.randint(0, v)), v))
    while len(edges) < 45:
        a, b = sorted(rng.choice(n, 2, replace=False).tolist())
        edges.add((a, b))
    graph = {v: [] for v in range(n)}
    for a, b in sorted(edges):
        graph[a].append(b)
        graph[b].append(a)
    emb = rng.normal(0, 0.7, (n, 6))
    o = orc.GraphGANOracle(n, graph, emb, emb, rng="counter", seed=5)
    o.generator.b[:] = rng.normal(0, 0.5, n).astype(np.float32)
    E, b = o.generator.E.astype(np.float64), o.generator.b.astype(np.float64)
    for root in (0, 17):
        tree = o.trees[root]
        off, nbr = _lists(tree, n)
        logp, a = gl.host_graph_softmax(E, b, root, off, nbr, False)
        assert a == 0.0
        o.stream = 1
        samples, _ = o.sample(root, {v: list(lst) for v, lst in tree.items()}, 100_000, False)
        counts = np.bincount(samples, minlength=n)
        assert chi2_pvalue_ok(counts, np.exp(logp), 1e-6)


def test_summary_and_results_line(gl):
    r = gl.summarize(np.array([np.log(0.5), -np.inf, np.log(0.25), np.nan]))
    assert r["n"] == 3 and r["reach"] == 2 / 3
    assert abs(r["nll"] - (np.log(2) + np.log(4)) / 2) < 1e-15
    assert gl.format_line(dict(nll=1.5, reach=0.75, n=8)) == "gen_nll:NLL=1.5 reach=0.75 n=8\n"
    assert gl.format_line(r) == "gen_nll:NLL=%s reach=%s n=3\n" % (str(r["nll"]), str(r["reach"]))


def test_edge_pairs_both_directions(gl, tmp_path):
    p = tmp_path / "test.txt"
    p.write_text("1\t2\n3\t4\n")
    assert gl.edge_pairs(str(p)).tolist() == [[1, 2], [2, 1], [3, 4], [4, 3]]


def _reroot(tree, r):
    """BFS tree of node r over the undirected edges of ``tree`` (children in id order)"""
    adj = {}
    for v, lst in tree.items():
        for c in lst[1:]:
            adj.setdefault(v, []).append(c)
            adj.setdefault(c, []).append(v)
    out, queue, seen = {r: [r]}, [r], {r}
    while queue:
        v = queue.pop(0)
        for w in sorted(adj.get(v, [])):
            if w not in seen:
                seen.add(w)
                out[v].append(w)
                out[w] = [v]
                queue.append(w)
    return out


def test_host_evaluator_on_lists(gl, tmp_path):
    rng = np.random.RandomState(4)
    n = 12
    emb, bias = rng.normal(0, 0.8, (n, 5)), rng.normal(0, 0.5, n)
    lists = [_lists(TREE, n), _lists(_reroot(TREE, 7), n), _lists({10: [10]}, n)]
    off = np.stack([o for o, _ in lists])
    nbr = np.concatenate([x for _, x in lists])
    base = np.cumsum([0] + [len(x) for _, x in lists])
    p = tmp_path / "test.txt"
    p.write_text("0\t7\n0\t10\n")
    trees = ({0: 0, 7: 1, 10: 2}, off, nbr, base)
    res = gl.GenLikelihoodEval(str(p), n, emb=emb, bias=bias, trees=trees).eval_gen_likelihood()
    lp0, _ = gl.host_graph_softmax(emb, bias, 0, *lists[0])
    lp7, _ = gl.host_graph_softmax(emb, bias, 7, *lists[1])
    assert res["n"] == 4 and res["reach"] == 0.5  # (0 -> 10): 10 is not in 0's tree; (10 -> 0): 10 is isolated
    assert abs(res["nll"] - (-lp0[7] - lp7[0]) / 2) < 1e-14
    with pytest.raises(ValueError):
        gl.GenLikelihoodEval(str(p), n)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _bare_engine(monkeypatch):
    from graphgan_amd import engine as eng_mod
    monkeypatch.setattr(eng_mod, "lib", _NoLib())
    e = eng_mod.Engine.__new__(eng_mod.Engine)
    e.n_node, e.n_emb = 10, 4
    e.tree_roots = np.arange(3, dtype=np.int32)
    e._ctx = ctypes.c_void_p()
    return e


def test_engine_graph_softmax_validates_before_the_device(monkeypatch):
    e = _bare_engine(monkeypatch)
    bad = [
        dict(slots=[3]), dict(slots=[-1]), dict(slots=[[0, 1]]), dict(slots=[0.5]),
        dict(slots=[0, 1], nodes=[np.array([1])]),                     # one list for two slots
        dict(slots=[0], nodes=[np.array([10])]),                        # node out of range
        dict(slots=[0], nodes=[np.array([-1])]),
        dict(slots=[0, 1], nodes=(np.array([1, 2]), np.array([0, 1]))),  # offsets too short
        dict(slots=[0, 1], nodes=(np.array([1, 2]), np.array([0, 2, 1]))),  # not monotone / wrong end
        dict(slots=[0], nodes=np.array([1, 2])),                         # neither a list nor (flat, offsets)
    ]
    for kw in bad:
        slots = kw.pop("slots")
        with pytest.raises(ValueError):
            e.graph_softmax(slots, **kw)


def test_engine_gen_nll_knob_defaults_off():
    from graphgan_amd import config
    assert config.engine_gen_nll is False


def test_abi_declares_graph_softmax():
    from graphgan_amd import _lib
    assert "gg_graph_softmax" in _lib.SIGNATURES
    assert (_lib.GG_GS_FOR_D, _lib.GG_GS_Q3_STORE) == (1, 2)
    assert _lib.lib.gg_abi_version() == _lib.ABI_VERSION == 9
