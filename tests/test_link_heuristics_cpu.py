"""The host side of the neighbourhood link-prediction baselines (graphgan_amd/evaluation/link_heuristics.py, graph_gan.py's
engine_lp_heuristics, the ``python -m graphgan_amd.heuristics`` command line) -- the definitions against Python sets and
networkx, the fixed-point node weights and their bound, the results line, its place and its cache, the refusals -- and the C
ABI's declaration of gg_pair_neighbors / gg_distinct_degrees."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lh():
    from graphgan_amd.evaluation import link_heuristics
    return link_heuristics


def test_header_declares_and_library_exports_the_two_symbols():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {"gg_distinct_degrees": ["gg_ctx*", "int32_t*"],
            "gg_pair_neighbors": ["gg_ctx*", "constint32_t*", "constint32_t*", "int64_t", "constuint64_t*", "int32_t", "int32_t*", "int32_t*",
                                  "int32_t*", "uint64_t*", "double*"]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name) and hasattr(_lib.lib, name)
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays


def test_chunk_length_and_audit_are_in_step_with_the_source():
    from graphgan_amd import _lib
    from graphgan_amd.engine import Engine
    src = open(os.path.join(ROOT, "graphgan_amd", "csrc", "pair_neighbors.hip")).read()
    m = re.search(r"constexpr int PN_CHUNK = (\d+);", src)
    assert m and int(m.group(1)) == _lib.PAIR_NEIGHBORS_CHUNK == Engine.PAIR_NEIGHBORS_CHUNK
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    assert re.search(r"^pair_neighbors\.o: AUDIT = 'pn_\[a-z_\]\*kernel' 3 ", mk, flags=re.M)  # the three group widths
    assert re.search(r"^AUDITED = .*\bpair_neighbors\.o\b", mk, flags=re.M)
    assert len(re.findall(r"pn_sweep_kernel<(\d+)>", src)) == 3


def _multigraph(seed, n=60, e=260):
    """random edges with duplicates (both orientations) and self-loops; nodes n - 3 .. n - 1 stay isolated"""
    rs = np.random.RandomState(seed)
    edges = rs.randint(0, n - 3, size=(e, 2))
    edges = np.concatenate([edges, edges[:40], edges[40:80, ::-1], np.repeat(np.arange(0, 20, 2), 2).reshape(-1, 2)])
    return n, edges[rs.permutation(len(edges))]


def _sets(n, edges):
    N = [set() for _ in range(n)]
    for a, b in np.asarray(edges).tolist():
        if a != b:
            N[a].add(b)
            N[b].add(a)
    return N


def brute_force(n, edges, u, v, weights):
    """the definitions of the header, restated with Python sets and Python integers"""
    N = _sets(n, edges)
    cn, du, dv, ws = [], [], [], [[] for _ in weights]
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        C = (N[a] & N[b]) - {a, b}
        cn.append(len(C))
        du.append(len(N[a]))
        dv.append(len(N[b]))
        for j, w in enumerate(weights):
            ws[j].append(sum(int(w[x]) for x in C))
    return cn, du, dv, ws


def test_host_sweep_equals_the_set_definition(lh):
    n, edges = _multigraph(1)
    rs = np.random.RandomState(2)
    u = np.concatenate([rs.randint(0, n, 400), np.arange(n), edges[:50, 0]])
    v = np.concatenate([rs.randint(0, n, 400), np.arange(n), edges[:50, 1]])  # random pairs, u == v, pairs that are edges
    ptr, adj = lh.set_adjacency(edges, n)
    N = _sets(n, edges)
    assert np.diff(ptr).tolist() == [len(s) for s in N]
    assert all(adj[ptr[x]:ptr[x + 1]].tolist() == sorted(N[x]) for x in range(n))
    assert (np.diff(ptr)[-3:] == 0).all() and any(x in N[x] for x in range(n)) is False
    w = rs.randint(0, 1 << 41, size=(3, n)).astype(np.uint64)
    res = lh.host_pair_neighbors(ptr, adj, u, v, w)
    cn, du, dv, ws = brute_force(n, edges, u, v, w)
    assert res["cn"].tolist() == cn and res["deg_u"].tolist() == du and res["deg_v"].tolist() == dv
    assert res["wsum"].dtype == np.uint64 and res["wsum"].tolist() == ws
    none = lh.host_pair_neighbors(ptr, adj, u, v)
    assert none["wsum"].shape == (0, len(u)) and none["cn"].tolist() == cn
    # the adjacency of a CSR (every edge in both directions, a self-loop twice) is the same sets
    from graphgan_amd.engine import edges_to_csr
    ptr2, adj2 = lh.csr_set_adjacency(*edges_to_csr(n, edges))
    assert np.array_equal(ptr, ptr2) and np.array_equal(adj, adj2)
    # the indices from those integers
    idx = lh.host_link_heuristics(ptr, adj, u, v)
    deg = np.diff(ptr)
    for i in range(len(u)):
        C = (N[u[i]] & N[v[i]]) - {u[i], v[i]}
        union = len(N[u[i]]) + len(N[v[i]]) - len(C)
        assert idx["cn"][i] == len(C) and idx["pa"][i] == len(N[u[i]]) * len(N[v[i]])
        assert idx["jaccard"][i] == (len(C) / union if union else 0.0)
        aa = math.fsum(1.0 / math.log(deg[x]) for x in C)
        ra = math.fsum(1.0 / deg[x] for x in C)
        # quantisation: every weight is within 2^-41 of its value (rint of the value times 2^40); the float64 of the integer
        # sum and the reference's own roundings: (cn + 1) ulps of the value
        for got, ref in ((idx["aa"][i], aa), (idx["ra"][i], ra)):
            assert abs(got - ref) <= len(C) * 2.0 ** -41 + (len(C) + 1) * 2.0 ** -52 * ref
    assert idx["cn"].dtype == np.int64 and idx["pa"].dtype == np.int64 and idx["jaccard"].dtype == np.float64


def test_host_indices_equal_networkx(lh):
    nx = pytest.importorskip("networkx")
    n, edges = _multigraph(3)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((a, b) for a, b in edges.tolist() if a != b)
    rs = np.random.RandomState(4)
    u, v = rs.randint(0, n, 300), rs.randint(0, n, 300)
    keep = u != v
    u, v = u[keep], v[keep]
    pairs = list(zip(u.tolist(), v.tolist()))
    ptr, adj = lh.set_adjacency(edges, n)
    idx = lh.host_link_heuristics(ptr, adj, u, v)
    assert idx["cn"].tolist() == [len(list(nx.common_neighbors(G, a, b))) for a, b in pairs]
    assert idx["pa"].tolist() == [p for _, _, p in nx.preferential_attachment(G, pairs)]
    assert idx["jaccard"].tolist() == [p for _, _, p in nx.jaccard_coefficient(G, pairs)]
    for key, fn in (("aa", nx.adamic_adar_index), ("ra", nx.resource_allocation_index)):
        ref = np.array([p for _, _, p in fn(G, pairs)])
        assert np.all(np.abs(idx[key] - ref) <= idx["cn"] * 2.0 ** -41 + (idx["cn"] + 1) * 2.0 ** -52 * ref)


def test_node_weights_at_the_small_degrees(lh):
    w = lh.node_weights(np.array([0, 1, 2, 3, 1000]))
    assert w.dtype == np.uint64 and w.shape == (2, 5)
    assert w[0].tolist() == [0, 0, int(np.rint(2.0 ** 40 / np.log(2.0))), int(np.rint(2.0 ** 40 / np.log(3.0))), int(np.rint(2.0 ** 40 / np.log(1000.0)))]
    assert w[1].tolist() == [0, 1 << 40, 1 << 39, int(np.rint(2.0 ** 40 / 3.0)), int(np.rint(2.0 ** 40 / 1000.0))]
    # each weight within half a unit of 2^-40 of its value: the bound of the sums
    d = np.arange(2, 5000)
    w = lh.node_weights(d)
    assert np.max(np.abs(w[0] / 2.0 ** 40 - 1.0 / np.log(d))) <= 2.0 ** -41 * (1 + 2.0 ** -8)
    assert np.max(np.abs(w[1] / 2.0 ** 40 - 1.0 / d)) <= 2.0 ** -41 * (1 + 2.0 ** -8)
    assert int(w.max()) * 4999 < 1 << 63


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def test_config_knob_defaults_off():
    from graphgan_amd import config
    assert config.engine_lp_heuristics is False


def test_evaluation_lines_with_and_without_the_knob(lh, tmp_path, monkeypatch):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    assert cfg.engine_lp_heuristics is False
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    want = GraphGAN.evaluation(g)  # the knob's default: off
    del cfg.engine_lp_heuristics
    assert GraphGAN.evaluation(g) == want and len(want) == 3  # a user's config without the knob
    assert open(cfg.result_filename).read() == "".join(want + want) and "graph_lp" not in "".join(want)
    cfg.engine_lp_heuristics = True
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_lp", "gen_nll"]
    assert lines[:2] == want[:2] and lines[3] == want[2]
    direct = lh.LinkHeuristicsEval(cfg.train_filename, cfg.test_filename, cfg.test_neg_filename, n).eval_link_heuristics()
    assert lines[2] == lh.format_results(direct)
    assert re.fullmatch(r"graph_lp:cn=\S+ jaccard=\S+ aa=\S+ ra=\S+ pa=\S+ n_test=2898\n", lines[2])
    assert all(0.5 < direct[k] <= 1.0 for k in lh.INDICES) and direct["n_test"] == 2 * 1449  # (the fixture's edge counts)
    assert lines[2] == "graph_lp:" + " ".join("%s=%s" % (k, str(direct[k])) for k in ("cn", "jaccard", "aa", "ra", "pa", "n_test")) + "\n"
    # the second evaluation repeats the cached string: nothing is computed again
    monkeypatch.setattr(lh.LinkHeuristicsEval, "eval_link_heuristics", lambda self: pytest.fail("the line was computed twice"))
    assert GraphGAN.evaluation(g) == lines and g._graph_lp_line == lines[2]
    assert open(cfg.result_filename).read() == "".join(want + want + lines + lines)


def test_the_aucs_are_the_mann_whitney_statistic_of_the_integers(lh, tmp_path):
    """a small case by hand: the path 0 - 1 - 2 - 3 and the star 4 - {5, 6, 7}"""
    from graphgan_amd.evaluation.link_prediction_lr import auc
    train, test, neg = (str(tmp_path / x) for x in ("train.txt", "test.txt", "neg.txt"))
    open(train, "w").write("0 1\n1 2\n2 3\n4 5\n4 6\n4 7\n1 0\n3 3\n")
    open(test, "w").write("0 2\n5 6\n")     # one common neighbour each (1; 4)
    open(neg, "w").write("0 3\n0 4\n1 1\n")  # none; none; u == v: C = N(1) = {0, 2}
    res = lh.LinkHeuristicsEval(train, test, neg, 8).eval_link_heuristics()
    truth = np.array([1, 1, 0, 0, 0])
    w = lh.node_weights([1, 2, 2, 1, 3, 1, 1, 1])
    assert res["cn"] == auc([1, 1, 0, 0, 2], truth) == 4 / 6
    assert res["pa"] == auc([2, 1, 1, 3, 4], truth)
    assert res["jaccard"] == auc([1 / 2, 1 / 1, 0.0, 0.0, 2 / 2], truth)
    assert w[0, 0] == 0 and w[1, 0] == 1 << 40  # (node 0 has degree 1: no Adamic-Adar weight)
    assert res["aa"] == auc([int(w[0, 1]), int(w[0, 4]), 0, 0, int(w[0, 0]) + int(w[0, 2])], truth) == 4.5 / 6  # (a tie with the first positive)
    assert res["ra"] == auc([int(w[1, 1]), int(w[1, 4]), 0, 0, int(w[1, 0]) + int(w[1, 2])], truth) == 4 / 6
    assert res["n_test"] == 5


def test_refusals_come_before_anything_is_computed(lh, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_lp_heuristics
    cfg, g, n = _layout(tmp_path)
    cfg.engine_lp_heuristics = True
    good = cfg.test_neg_filename
    cfg.test_neg_filename = str(tmp_path / "no_such_negatives.txt")
    with pytest.raises(ValueError, match="engine_lp_heuristics needs test edges and test negatives: config.test_neg_filename does not exist"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    cfg.test_neg_filename, cfg.test_filename = good, str(tmp_path / "no_such_test.txt")
    with pytest.raises(ValueError, match="config.test_filename does not exist"):
        _check_lp_heuristics(cfg)
    with pytest.raises(ValueError, match="test_filename"):
        _check_lp_heuristics(types.SimpleNamespace(engine_lp_heuristics=True))
    _check_lp_heuristics(types.SimpleNamespace())  # the knob absent: nothing to check
    _check_lp_heuristics(types.SimpleNamespace(engine_lp_heuristics=False))
    # the module's own refusals
    with pytest.raises(ValueError, match="node id outside"):
        lh.set_adjacency([[0, 5]], 5)
    ptr, adj = lh.set_adjacency([[0, 1]], 3)
    with pytest.raises(ValueError, match="node id outside"):
        lh.host_pair_neighbors(ptr, adj, [0], [3])
    with pytest.raises(ValueError, match="same length"):
        lh.host_pair_neighbors(ptr, adj, [0, 1], [1])
    empty = str(tmp_path / "empty.txt")
    open(empty, "w").close()
    with pytest.raises(ValueError, match="both classes"):
        lh.LinkHeuristicsEval(cfg.train_filename, good, empty, n).eval_link_heuristics()


def test_command_line_on_the_host(lh, tmp_path):
    from graphgan_amd import heuristics
    n, edges = _multigraph(5, n=30, e=90)
    rs = np.random.RandomState(6)
    pairs = rs.randint(0, n + 2, size=(40, 2))  # (ids behind the training file's: isolated nodes)
    train, pfile, out = (str(tmp_path / x) for x in ("train.txt", "pairs.txt", "scores.tsv"))
    np.savetxt(train, edges, fmt="%d")
    np.savetxt(pfile, pairs, fmt="%d", delimiter="\t")
    assert heuristics.main(["--train", train, "--pairs", pfile, "--out", out, "--host"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert len(rows) == 40 and all(len(r) == 7 for r in rows)
    ptr, adj = lh.set_adjacency(edges, n + 2)
    idx = lh.host_link_heuristics(ptr, adj, pairs[:, 0], pairs[:, 1])
    cn, du, dv, _ = brute_force(n + 2, edges, pairs[:, 0], pairs[:, 1], [])
    assert [[int(r[0]), int(r[1])] for r in rows] == pairs.tolist()
    assert [int(r[2]) for r in rows] == cn and [int(r[6]) for r in rows] == [a * b for a, b in zip(du, dv)]
    for k, name in ((3, "jaccard"), (4, "aa"), (5, "ra")):
        assert [float(r[k]) for r in rows] == idx[name].tolist()
    with open(pfile, "w") as f:
        f.write("1 2 3\n")
    with pytest.raises(SystemExit):
        heuristics.main(["--train", train, "--pairs", pfile, "--out", out, "--host"])
    with pytest.raises(SystemExit):
        heuristics.main(["--train", train, "--out", out, "--host"])
