"""The host side of the edge-list split (graphgan_amd/split.py, the ``python -m graphgan_amd.split`` command line): the numpy
Boruvka rounds against the Kruskal restatement (tests/support/spanning_forest_ref.py) and against scipy, the split's
properties on CA-GrQc, the refusals, the files -- and the C ABI's declaration of gg_undirected_edges / gg_spanning_forest."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests.support import spanning_forest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp():
    from graphgan_amd import split
    return split


@pytest.fixture(scope="module")
def graphs():
    """(n, raw edges) of the two graphs the forest tests share, with the restatement's edge list: never changed"""
    out = {}
    for name, (n, edges) in (("ca_grqc", ref.ca_grqc_union()), ("random", ref.random_graph())):
        out[name] = dict(n=n, edges=edges, E=ref.edge_list(ref.neighbor_sets(n, edges)))
    assert len(out["random"]["E"]) > 100000
    return out


def check_against_kruskal(sp, g, seed=0, prio=None):
    n, E = g["n"], g["E"]
    got_E = sp.undirected_edge_list(g["edges"], n)
    assert got_E.dtype == np.int32 and got_E.tolist() == [list(e) for e in E]
    sf = sp.host_spanning_forest(got_E, n, seed=seed, priority=prio)
    forest, component, k = ref.kruskal(n, E, ref.default_priorities(len(E), seed) if prio is None else prio)
    assert sf["forest"].dtype == np.uint8 and sf["component"].dtype == np.int32
    assert sf["forest"].tolist() == forest and sf["component"].tolist() == component
    assert (sf["m"], sf["n_forest"], sf["n_components"]) == (len(E), sum(forest), k) and k == n - sum(forest)
    assert sf["rounds"] <= math.ceil(math.log2(max(n, 2))) + 1
    assert sf["sweep_hooks"].tolist()[-1] == 0 and int(sf["sweep_hooks"].sum()) == sum(forest) and len(sf["sweep_hooks"]) == sf["rounds"] + 1
    return sf


@pytest.mark.parametrize("seed", (0, 1))
def test_host_forest_equals_kruskal_on_ca_grqc(sp, graphs, seed):
    check_against_kruskal(sp, graphs["ca_grqc"], seed)


def test_host_forest_on_the_ca_grqc_training_graph_known_counts(sp):
    from tests.helpers import load_ca_grqc
    d, n, _ = load_ca_grqc()
    E = sp.undirected_edge_list(d["train"], n)
    sf = sp.host_spanning_forest(E, n, seed=0)
    used = len(np.unique(E))
    assert (n, len(E), sf["n_forest"], sf["n_components"], n - used, sf["rounds"]) == (5242, 13036, 4761, 481, 124, 4)


def test_host_forest_equals_kruskal_on_the_random_graph(sp, graphs):
    sf = check_against_kruskal(sp, graphs["random"])
    assert sf["n_components"] > 2000 and sf["rounds"] >= 5


def test_programmed_priorities_and_ties(sp):
    n, edges = ref.path_graph(1025)
    g = dict(n=n, edges=edges, E=ref.edge_list(ref.neighbor_sets(n, edges)))
    m = len(g["E"])
    for prio in (np.arange(m), np.arange(m)[::-1].copy(), np.zeros(m, np.int64), np.full(m, 2 ** 32 - 1), np.where(np.arange(m) % 2, 0, 2 ** 32 - 1)):
        sf = check_against_kruskal(sp, g, prio=prio)
        assert sf["n_forest"] == m and sf["n_components"] == 1
    assert check_against_kruskal(sp, g, prio=np.arange(m))["rounds"] == 1  # ascending along the path: every node's best edge points back
    n, edges = ref.complete_graph(65)
    g = dict(n=n, edges=edges, E=ref.edge_list(ref.neighbor_sets(n, edges)))
    for seed in (0, 1, 0xFFFFFFFF):
        check_against_kruskal(sp, g, seed)
    for bad in (np.arange(5), np.zeros(len(g["E"])), np.full(len(g["E"]), -1), np.full(len(g["E"]), 2 ** 32)):
        with pytest.raises(ValueError, match=r"host_spanning_forest: priority must be a uint32 array \[2080\]"):
            sp.host_spanning_forest(g["E"], n, priority=bad)


def test_default_priorities_are_the_headers_hash(sp):
    for seed in (0, 1, 0xFFFFFFFF):
        assert sp.default_priorities(300, seed).tolist() == ref.default_priorities(300, seed)
    assert sp.default_priorities(300, 0).dtype == np.uint32 and sp.default_priorities(0, 0).shape == (0,)


def test_host_forest_against_scipy(sp, graphs):
    pytest.importorskip("scipy")
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
    for name, seed in (("ca_grqc", 0), ("ca_grqc", 1), ("random", 0)):
        g = graphs[name]
        n, E = g["n"], np.array(g["E"])
        m = len(E)
        sf = sp.host_spanning_forest(E, n, seed=seed)
        key = (sp.default_priorities(m, seed).astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)
        rank = np.empty(m, dtype=np.int64)
        rank[np.argsort(key)] = np.arange(1, m + 1)  # distinct positive weights in key order (exact in float64)
        T = minimum_spanning_tree(coo_matrix((rank.astype(np.float64), (E[:, 0], E[:, 1])), shape=(n, n)).tocsr()).tocoo()
        took = set(zip(T.row.tolist(), T.col.tolist()))
        assert [int((a, b) in took) for a, b in E.tolist()] == sf["forest"].tolist()
        k, lab = connected_components(coo_matrix((np.ones(m), (E[:, 0], E[:, 1])), shape=(n, n)), directed=False)
        assert k == sf["n_components"]
        first = np.full(k, n)
        np.minimum.at(first, lab, np.arange(n))
        assert first[lab].tolist() == sf["component"].tolist()


@pytest.fixture(scope="module")
def grqc_split(sp, graphs):
    g = graphs["ca_grqc"]
    return sp.split_edges(g["edges"], g["n"], ratio=0.1, seed=0)


def components_of(n, edge_rows):
    return ref.kruskal(n, [tuple(e) for e in edge_rows], [0] * len(edge_rows))[1]


def test_split_properties_on_ca_grqc(sp, graphs, grqc_split):
    g = graphs["ca_grqc"]
    n, E = g["n"], g["E"]
    m = len(E)
    train, test, neg, stats = grqc_split
    assert train.dtype == test.dtype == neg.dtype == np.int32
    n_test = int(math.floor(0.1 * m + 0.5))
    assert len(test) == len(neg) == n_test == stats["test"] == stats["test_neg"] and len(train) == m - n_test == stats["train"]
    tr, te = [tuple(e) for e in train.tolist()], [tuple(e) for e in test.tolist()]
    assert sorted(tr + te) == E and not set(tr) & set(te)  # train and test partition E
    assert tr == sorted(tr) and te == sorted(te)  # each in j order
    full = components_of(n, E)
    assert components_of(n, tr) == full  # the training graph is not cut apart
    deg_full, deg_train = np.bincount(np.array(E).reshape(-1), minlength=n), np.bincount(train.reshape(-1), minlength=n)
    assert not np.any((deg_full > 0) & (deg_train == 0))  # no node loses its last edge
    ng = [tuple(e) for e in neg.tolist()]
    assert len(set(ng)) == len(ng) and not set(ng) & set(E) and all(a < b for a, b in ng)
    assert np.all(deg_full[neg.reshape(-1)] > 0)  # both ends on nodes with an edge
    forest = ref.kruskal(n, E, ref.default_priorities(m, 0))[0]
    at = {e: j for j, e in enumerate(E)}
    assert not any(forest[at[e]] for e in te)  # no held-out edge is a forest edge
    assert stats == dict(nodes=n, edges=m, components=len(set(full)), largest=int(np.bincount(full).max()), isolated=int((deg_full == 0).sum()),
                         forest=sum(forest), candidates=m - sum(forest), train=m - n_test, test=n_test, test_neg=n_test, rounds=stats["rounds"])
    assert sp.format_summary(stats).startswith("nodes=%d edges=%d components=" % (n, m)) and " rounds=%d" % stats["rounds"] in sp.format_summary(stats)


def test_split_seeds_and_protect_none(sp, graphs, grqc_split):
    g = graphs["ca_grqc"]
    again = sp.split_edges(g["edges"], g["n"], ratio=0.1, seed=0)
    other = sp.split_edges(g["edges"], g["n"], ratio=0.1, seed=1)
    for x, y in zip(grqc_split[:3], again[:3]):
        assert np.array_equal(x, y)
    assert not np.array_equal(grqc_split[1], other[1]) and not np.array_equal(grqc_split[2], other[2])
    # a shuffled list with both directions, duplicates and self-loops is the same graph: the same split
    rs = np.random.RandomState(0)
    e = np.concatenate([g["edges"], g["edges"][:50, ::-1], [[3, 3], [7, 7]]])
    for x, y in zip(grqc_split[:3], sp.split_edges(e[rs.permutation(len(e))], g["n"], ratio=0.1, seed=0)[:3]):
        assert np.array_equal(x, y)
    # protect = "none" draws from all edges: at this ratio some forest edge is held out
    train, test, neg, stats = sp.split_edges(g["edges"], g["n"], ratio=0.1, seed=0, protect="none")
    m = len(g["E"])
    assert stats["candidates"] == m and len(test) == grqc_split[3]["test"] and len(train) == m - len(test)
    forest = ref.kruskal(g["n"], g["E"], ref.default_priorities(m, 0))[0]
    at = {e: j for j, e in enumerate(g["E"])}
    assert any(forest[at[tuple(e)]] for e in test.tolist())
    with pytest.raises(ValueError, match="protect must be 'forest' or 'none'"):
        sp.split_edges(g["edges"], g["n"], protect="tree")


def test_split_refusals(sp, graphs):
    g = graphs["ca_grqc"]
    m = len(g["E"])
    n_forest = sum(ref.kruskal(g["n"], g["E"], ref.default_priorities(m, 0))[0])
    want = int(math.floor(0.9 * m + 0.5))
    with pytest.raises(ValueError, match=r"asks for %d test edges, %d edges can be held out" % (want, m - n_forest)):
        sp.split_edges(g["edges"], g["n"], ratio=0.9)
    with pytest.raises(ValueError, match=r"asks for 0 test edges, %d edges can be held out" % (m - n_forest)):
        sp.split_edges(g["edges"], g["n"], ratio=1e-6)
    n, edges = ref.complete_graph(12)  # 66 edges, 11 of them the forest; no non-edge
    with pytest.raises(ValueError, match=r"7 negatives asked for, only 0 non-edges exist among the 12 nodes with an edge"):
        sp.split_edges(edges, n, ratio=0.1)
    n, edges = ref.path_graph(30)  # a tree: nothing can be held out
    with pytest.raises(ValueError, match=r"asks for 3 test edges, 0 edges can be held out"):
        sp.split_edges(edges, n, ratio=0.1)
    assert len(sp.split_edges(edges, n, ratio=0.1, protect="none")[1]) == 3


def test_command_line_host_round_trip(sp, graphs, tmp_path, capsys):
    from graphgan_amd import utils
    g = graphs["ca_grqc"]
    src, prefix = str(tmp_path / "edges.txt"), str(tmp_path / "out")
    np.savetxt(src, g["edges"], fmt="%d")
    assert sp.main(["--edges", src, "--out-prefix", prefix, "--ratio", "0.1", "--seed", "0", "--host"]) == 0
    train, test, neg, stats = sp.split_edges(g["edges"], g["n"], ratio=0.1, seed=0)
    assert capsys.readouterr().out == sp.format_summary(stats) + "\n"
    for suffix, part in (("_train.txt", train), ("_test.txt", test), ("_test_neg.txt", neg)):
        raw = open(prefix + suffix, "rb").read()
        assert raw == "".join("%d\t%d\n" % (a, b) for a, b in part.tolist()).encode()  # tab and \n: the shipped files' format
        assert utils.read_edges_from_file(prefix + suffix) == part.tolist()
    n_read, graph = utils.read_edges(prefix + "_train.txt", prefix + "_test.txt")
    assert n_read == len(np.unique(np.array(g["E"]))) and sum(len(v) for v in graph.values()) == 2 * len(train)
    from graphgan_amd.evaluation.link_prediction import LinkPredictEval
    emd = np.random.RandomState(0).rand(g["n"], 4)
    acc = LinkPredictEval("", prefix + "_test.txt", prefix + "_test_neg.txt", g["n"], 4, emd=emd).eval_link_prediction()
    assert 0.0 <= acc <= 1.0  # the evaluator reads the two files
    with pytest.raises(SystemExit):
        sp.main(["--edges", src, "--out-prefix", prefix, "--ratio", "0.95", "--host"])


def test_header_declares_and_library_exports_the_two_symbols():
    from graphgan_amd import _lib
    from graphgan_amd.engine import Engine
    text = open(_lib.HEADER_PATH).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = {"gg_undirected_edges": ["gg_ctx*", "int64_t*", "int32_t*"],
            "gg_spanning_forest": ["gg_ctx*", "uint32_t", "constuint32_t*", "int64_t", "uint8_t*", "int32_t*", "int64_t*", "int64_t*", "double*", "double*"]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name) and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["gg_spanning_forest"][1][1] is ctypes.c_uint32 and _lib.SIGNATURES["gg_spanning_forest"][1][3] is ctypes.c_int64
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "spanning-forest sweep" in text and "0x53504C54" in text
    assert int(re.search(r"^#define\s+GG_SF_MAX_SWEEPS\s+(\d+)", text, flags=re.M).group(1)) == _lib.SF_MAX_SWEEPS
    for method in ("undirected_edges", "spanning_forest", "connected_components"):
        assert callable(getattr(Engine, method))


def test_source_and_audit_are_in_step(sp):
    src = open(os.path.join(ROOT, "graphgan_amd", "csrc", "spanning_forest.hip")).read()
    assert int(re.search(r"SF_SEED_SALT = (0x[0-9A-Fa-f]+)u;", src).group(1), 16) == sp.SEED_SALT == ref.SALT
    kernels = re.findall(r"^__global__ .*void (sf_\w+_kernel)\(", src, flags=re.M)
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    assert re.search(r"^spanning_forest\.o: AUDIT = 'sf_\[a-z0-9_\]\*kernel' %d " % len(kernels), mk, flags=re.M)
    assert re.search(r"^AUDITED = .*\bspanning_forest\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\bspanning_forest\.o\b", mk, flags=re.M)
    device = src[:src.index("int ceil_log2(")]  # the kernels: integer only, no inline assembly
    assert not re.search(r"\b(float|double|fmaf?|__f\w+_rn|asm)\b", device)
    # one definition of the hash, shared with the neighbour-mode sweep
    csrc = os.path.join(ROOT, "graphgan_amd", "csrc")
    assert sum(open(os.path.join(csrc, f)).read().count("uint32_t fmix32(") for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp"))) == 1
