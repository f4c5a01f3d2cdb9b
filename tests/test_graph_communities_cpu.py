"""The host side of the label-propagation community baseline and the modularity lines (graphgan_amd/evaluation/graph_communities.py,
graph_gan.py's engine_cluster_graph_baseline / engine_cluster_modularity, the ``python -m graphgan_amd.communities`` command line) --
the hash, the numpy rules against the restatement in dicts and sets (tests/support/communities_ref.py), modularity against
networkx, the renumbering, both results lines, their places and caches, the refusals -- and the C ABI's declaration of
gg_neighbor_mode / gg_label_propagation / gg_partition_edges."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

from tests.support import communities_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gc():
    from graphgan_amd.evaluation import graph_communities
    return graph_communities


@pytest.fixture(scope="module")
def lh():
    from graphgan_amd.evaluation import link_heuristics
    return link_heuristics


def test_header_declares_and_library_exports_the_three_symbols():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {"gg_neighbor_mode": ["gg_ctx*", "constint32_t*", "uint32_t", "int32_t", "constint32_t*", "int64_t", "int32_t*", "double*"],
            "gg_label_propagation": ["gg_ctx*", "uint32_t", "int32_t", "int32_t*", "int32_t*", "int32_t*", "int32_t*", "double*"],
            "gg_partition_edges": ["gg_ctx*", "constint32_t*", "int32_t", "int64_t*", "int64_t*", "double*"]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name) and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["gg_neighbor_mode"][1][2] is ctypes.c_uint32 and _lib.SIGNATURES["gg_label_propagation"][1][1] is ctypes.c_uint32
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "neighbour-mode sweep" in open(_lib.HEADER_PATH).read()


def test_constants_and_audit_are_in_step_with_the_source():
    from graphgan_amd import _lib
    from graphgan_amd.engine import Engine
    src = open(os.path.join(ROOT, "graphgan_amd", "csrc", "communities.hip")).read()
    m = re.search(r"constexpr int CM_LDS_CAP = (\d+);", src)
    assert m and int(m.group(1)) == _lib.NEIGHBOR_MODE_LDS_CAP == Engine.NEIGHBOR_MODE_LDS_CAP
    assert 2 * 2 * 4 * 2 * int(m.group(1)) <= 160 * 1024  # two workgroups' (label, count) tables of 2 x CAP slots share a CU's LDS
    m = re.search(r"constexpr int CM_CHUNK = (\d+);", src)
    assert m and int(m.group(1)) == _lib.PARTITION_EDGES_CHUNK == Engine.PARTITION_EDGES_CHUNK == 512
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    assert re.search(r"^communities\.o: AUDIT = 'cm_\[a-z0-9_\]\*kernel' 9 ", mk, flags=re.M)  # 3 + 2 mode kernels, 3 edge kernels, the initialiser
    assert re.search(r"^AUDITED = .*\bcommunities\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\bcommunities\.o\b", mk, flags=re.M)
    # ONE set of mode kernels: the side of a half-step is an argument, not a second kernel
    assert len(re.findall(r"^__global__ .*void cm_mode_\w+_kernel\(", src, flags=re.M)) == 2 and "side_h" in src
    device = src[:src.index("int mode_class(")]  # the kernels, and the whole header of their shared parts: no floating point
    device += open(os.path.join(ROOT, "graphgan_amd", "csrc", "set_sweep.h")).read()
    assert not re.search(r"\b(float|double|fmaf?|__f\w+_rn)\b", device)


def test_fmix32_known_answers(gc):
    known = {0: 0, 1: 0x514E28B7, 2: 0x30F4C306, 0xFFFFFFFF: 0x81F16F39, 0x9E3779B9: None, 12345: None}
    for x, want in known.items():
        assert gc.fmix32(x) == ref.fmix32(x)
        if want is not None:
            assert gc.fmix32(x) == want, hex(x)
    xs = np.concatenate([np.arange(1000), np.random.RandomState(0).randint(0, 2 ** 32, 1000, dtype=np.uint64)]).astype(np.uint32)
    got = gc.fmix32(xs)
    assert got.dtype == np.uint32 and got.tolist() == [ref.fmix32(int(x)) for x in xs]
    assert len(set(got.tolist())) == len(set(xs.tolist()))  # a bijection on uint32
    assert gc.iteration_state(3, 2) == ref.side_state(3, 2) and gc.half_step_salt(3, 2, 1) == ref.salt_of(3, 2, 1)
    assert gc.iteration_state(2 ** 32 + 3, 2) == ref.side_state(3, 2)  # seeds are taken mod 2^32


def _multigraph(seed, n=70, e=200):
    """random edges with duplicates (both orientations) and self-loops; nodes n - 3 .. n - 1 stay isolated"""
    rs = np.random.RandomState(seed)
    edges = rs.randint(0, n - 3, size=(e, 2))
    edges = np.concatenate([edges, edges[:40], edges[40:80, ::-1], np.repeat(np.arange(0, 20, 2), 2).reshape(-1, 2)])
    return n, edges[rs.permutation(len(edges))]


def test_host_rules_equal_the_restatement(gc, lh):
    n, edges = _multigraph(1)
    N = ref.neighbor_sets(n, edges)
    ptr, adj = lh.set_adjacency(edges, n)
    assert np.diff(ptr).tolist() == [len(s) for s in N] and not np.diff(ptr)[-3:].any()
    rs = np.random.RandomState(2)
    fields = [np.arange(n), np.zeros(n, np.int64), rs.randint(0, 3, n), rs.randint(0, 2 ** 31 - 1, n), np.full(n, 2 ** 31 - 1)]
    for labels in fields:
        for salt in (0, 1, 0xDEADBEEF):
            for keep in (True, False):
                got = gc.host_neighbor_mode(ptr, adj, labels, salt=salt, keep=keep)
                assert got.dtype == np.int32 and got.tolist() == ref.neighbor_mode(N, labels, salt, keep), (salt, keep)
    sub = np.array([5, 69, 5, 0, 68])
    assert gc.host_neighbor_mode(ptr, adj, fields[2], salt=7, nodes=sub).tolist() == ref.neighbor_mode(N, fields[2], 7, True, sub)
    assert gc.host_neighbor_mode(ptr, adj, fields[2], nodes=np.zeros(0, np.int64)).shape == (0,)
    for seed in (0, 1, 2 ** 32 - 1):
        for max_iters in (1, 3, 100):
            got = gc.host_label_propagation(ptr, adj, seed=seed, max_iters=max_iters)
            L, t, conv, changed = ref.label_propagation(N, seed, max_iters)
            assert got["labels"].tolist() == L and got["iters"] == t and got["converged"] == conv and got["changed"].tolist() == changed
            assert got["labels"].dtype == np.int32 and got["changed"].dtype == np.int64
    assert got["converged"] and got["changed"][-1] == 0 and got["labels"][-3:].tolist() == [n - 3, n - 2, n - 1]
    for assign, k in ((rs.randint(-1, 4, n), 4), (rs.randint(-1, 4, n), 7), (np.zeros(n, np.int64), 1), (np.full(n, -1), 2), (np.arange(n), n)):
        got = gc.host_partition_edges(ptr, adj, assign, k)
        intra, tot = ref.partition_edges(N, assign, k)
        assert got["intra"].tolist() == intra and got["tot"].tolist() == tot and got["intra"].dtype == got["tot"].dtype == np.int64
        q, want = gc.modularity_from_counts(got["intra"], got["tot"]), ref.modularity(intra, tot)
        assert (math.isnan(q) and math.isnan(want)) or q == want


def test_modularity_against_networkx(gc, lh):
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.community import modularity
    n, edges = _multigraph(3)
    ptr, adj = lh.set_adjacency(edges, n)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(u), int(v)) for u, v in edges if u != v)  # (a simple graph: the neighbour sets)
    rs = np.random.RandomState(4)
    for k in (1, 2, 5, 20):
        assign = rs.randint(0, k, n)
        cnt = gc.host_partition_edges(ptr, adj, assign, k)
        want = modularity(G, [set(np.flatnonzero(assign == c).tolist()) for c in range(k)])
        assert abs(gc.modularity_from_counts(cnt["intra"], cnt["tot"]) - want) <= 1e-12, k
    # a partition of a subset is the partition of the induced subgraph
    inside = np.flatnonzero(rs.random_sample(n) < 0.6)
    assign = np.full(n, -1)
    assign[inside] = rs.randint(0, 3, len(inside))
    cnt = gc.host_partition_edges(ptr, adj, assign, 3)
    H = G.subgraph(inside.tolist())
    want = modularity(H, [set(np.flatnonzero(assign == c).tolist()) for c in range(3)])
    assert abs(gc.modularity_from_counts(cnt["intra"], cnt["tot"]) - want) <= 1e-12
    assert int(cnt["tot"].sum()) == 2 * H.number_of_edges()
    assert math.isnan(gc.modularity_from_counts([0, 0], [0, 0]))  # no edge inside
    assert gc.modularity_from_counts([4], [4]) == 0.0 and gc.modularity_from_counts([2, 2], [2, 2]) == 0.5


def test_relabel(gc):
    comm, k = gc.relabel([7, 3, 7, 9, 3, 0])
    assert comm.tolist() == [0, 1, 0, 2, 1, 3] and k == 4 and comm.dtype == np.int32  # numbered by the smallest member
    assert gc.relabel(np.arange(5)[::-1])[0].tolist() == [0, 1, 2, 3, 4]
    assert gc.relabel(np.zeros(0, np.int32)) [1] == 0
    rs = np.random.RandomState(0)
    labels = rs.randint(0, 2 ** 31 - 1, 40)[rs.randint(0, 40, 300)]
    comm, k = gc.relabel(labels)
    want, wk = ref.relabel(labels.tolist())
    assert comm.tolist() == want and k == wk


def test_disjoint_cliques_become_the_components(gc, lh):
    """cliques of 3, 5 and 8 nodes and two isolated nodes: label propagation ends with one label per component"""
    sizes, edges, comp, v0 = (3, 5, 8), [], [], 0
    for c, s in enumerate(sizes):
        edges += [(v0 + i, v0 + j) for i in range(s) for j in range(i + 1, s)]
        comp += [c] * s
        v0 += s
    n = v0 + 2
    comp += [3, 4]
    perm = np.random.RandomState(1).permutation(n)  # (node ids that do not follow the cliques)
    edges = perm[np.array(edges)]
    want = np.empty(n, np.int64)
    want[perm] = comp
    N = ref.neighbor_sets(n, edges)
    for seed in (0, 1, 2):
        L, t, conv, changed = ref.label_propagation(N, seed, 100)
        assert conv and t < 100, "the restatement does not converge on disjoint cliques"
        ptr, adj = lh.set_adjacency(edges, n)
        got = gc.host_label_propagation(ptr, adj, seed=seed, max_iters=100)
        assert got["labels"].tolist() == L and got["converged"] and got["iters"] == t
        assert gc.relabel(got["labels"])[0].tolist() == ref.relabel(want.tolist())[0]  # the communities are the components
        fit = gc.fit_communities(*gc.host_sweeps(edges, n), seed=seed, n_init=2, max_iters=100)
        assert fit["k"] == 5 and int((fit["tot"] > 0).sum()) == 3 and fit["converged"]
        m2 = float(sum(s * (s - 1) for s in sizes))
        assert fit["q"] == pytest.approx(1.0 - sum((s * (s - 1) / m2) ** 2 for s in sizes), abs=1e-15)


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def _labels_for(cfg, n, tmp_path):
    rs = np.random.RandomState(5)
    nodes = np.sort(rs.permutation(n)[:n // 4])
    cfg.labels_filename = str(tmp_path / "labels.txt")
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d\t%d\n" % (v, 10 * int(c)) for v, c in zip(nodes, rs.randint(0, 4, size=len(nodes))))
    return nodes


def test_config_knob_defaults():
    from graphgan_amd import config
    assert config.engine_cluster_graph_baseline is False and config.engine_cluster_modularity is False
    assert (config.engine_lpa_n_init, config.engine_lpa_max_iters) == (4, 100)


def test_graph_cluster_line_with_and_without_the_knob(gc, tmp_path, monkeypatch):
    from graphgan_amd import utils
    from graphgan_amd.evaluation import node_clustering as ncl
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    nodes = _labels_for(cfg, n, tmp_path)
    assert cfg.engine_cluster_graph_baseline is False and cfg.engine_cluster_modularity is False
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    cfg.engine_nc_graph_baseline, cfg.engine_lsp_iters = True, 5
    want = GraphGAN.evaluation(g)  # the knobs' default: off
    del cfg.engine_cluster_graph_baseline, cfg.engine_cluster_modularity, cfg.engine_lpa_n_init, cfg.engine_lpa_max_iters
    g._graph_nc_line = None
    assert GraphGAN.evaluation(g) == want and [ln.split(":")[0] for ln in want] == ["gen", "dis", "graph_nc", "gen_nll"]  # a config without them
    assert open(cfg.result_filename).read() == "".join(want + want) and "graph_cluster" not in "".join(want)  # byte-identical files
    cfg.engine_cluster_graph_baseline, cfg.engine_lpa_n_init, cfg.engine_lpa_max_iters = True, 2, 60
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_nc", "graph_cluster", "gen_nll"]  # after graph_nc, before gen_nll
    assert lines[:3] == want[:3] and lines[4] == want[3]
    ev = gc.GraphCommunityEval(cfg.train_filename, cfg.labels_filename, n, n_init=2, max_iters=60, seed=0)
    direct = ev.eval_graph_communities()
    assert lines[3] == gc.format_results(direct)
    assert lines[3] == "graph_cluster:" + " ".join("%s=%s" % (k, str(direct[k])) for k in
                                                   ("NMI", "ARI", "purity", "Q", "communities", "n", "iters", "converged", "seed")) + "\n"
    assert re.fullmatch(r"graph_cluster:NMI=\S+ ARI=\S+ purity=\S+ Q=0\.\d+ communities=\d+ n=%d iters=\d+ converged=(True|False) seed=[01]\n" % len(nodes),
                        lines[3])
    # the line is the restatement's: the restart with the highest Q of the whole training graph, scored on the labelled nodes
    edges = np.array(utils.read_edges_from_file(cfg.train_filename))
    N = ref.neighbor_sets(n, edges)
    runs = []
    for seed in (0, 1):
        L, t, conv, _ = ref.label_propagation(N, seed, 60)
        comm, k = ref.relabel(L)
        intra, tot = ref.partition_edges(N, comm, k)
        runs.append((ref.modularity(intra, tot), seed, comm, t, conv, sum(1 for x in tot if x > 0)))
    q, seed, comm, t, conv, communities = max(runs, key=lambda r: (r[0], -r[1]))
    assert (direct["Q"], direct["seed"], direct["iters"], direct["converged"], direct["communities"]) == (q, seed, t, conv, communities)
    assert ev.last_fit["communities"].tolist() == comm and 0.5 < q < 1.0
    _, classes, _ = utils.read_labels(cfg.labels_filename, n)
    scores = ncl.cluster_metrics(classes, np.array(comm)[nodes])
    assert (direct["NMI"], direct["ARI"], direct["purity"]) == (scores["nmi"], scores["ari"], scores["purity"])
    # the second evaluation repeats the cached string: nothing is computed again
    monkeypatch.setattr(gc.GraphCommunityEval, "eval_graph_communities", lambda self: pytest.fail("the line was computed twice"))
    assert GraphGAN.evaluation(g) == lines and g._graph_cluster_line == lines[3]
    assert open(cfg.result_filename).read() == "".join(want + want + lines + lines)


def test_modularity_lines_and_their_place(gc, lh, tmp_path):
    from graphgan_amd import utils
    from graphgan_amd.evaluation import node_clustering as ncl
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    nodes = _labels_for(cfg, n, tmp_path)
    cfg.engine_node_clustering, cfg.engine_cluster_n_init, cfg.engine_cluster_max_iters = True, 2, 30
    cfg.engine_emb_spectrum = True
    want = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in want] == ["gen", "dis", "gen_cluster", "dis_cluster", "gen_spec", "dis_spec"]
    cfg.engine_cluster_modularity = True
    lines = GraphGAN.evaluation(g)  # no *_sil lines: behind the *_cluster lines
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "gen_cluster", "dis_cluster", "gen_mod", "dis_mod", "gen_spec", "dis_spec"]
    assert lines[:4] == want[:4] and lines[6:] == want[4:]  # the other lines keep every byte
    cfg.engine_cluster_silhouette = True
    both = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in both] == ["gen", "dis", "gen_cluster", "dis_cluster", "gen_sil", "dis_sil", "gen_mod", "dis_mod", "gen_spec", "dis_spec"]
    assert both[6:8] == lines[4:6] and both[:4] == want[:4]
    edges = np.array(utils.read_edges_from_file(cfg.train_filename))
    N = ref.neighbor_sets(n, edges)
    _, classes, values = utils.read_labels(cfg.labels_filename, n)
    m2 = sum(1 for v in nodes.tolist() for w in N[v] if w in set(nodes.tolist()))
    label_q = None
    for i, (mode, line) in enumerate(zip(cfg.modes, lines[4:6])):
        nce = ncl.NodeClusterEval(cfg.emb_filenames[i], cfg.labels_filename, n, cfg.n_emb, n_init=2, max_iters=30, seed=g.seed)
        nce.eval_node_clustering()
        fit = nce.last_partition
        qs = []
        for part, k in ((fit["assign"], fit["k"]), (classes, len(values))):
            full = [-1] * n
            for v, c in zip(nodes.tolist(), np.asarray(part).tolist()):
                full[v] = c
            qs.append(ref.modularity(*ref.partition_edges(N, full, k)))
        assert line == "%s_mod:Q=%s label_Q=%s k=4 n=%d edges=%d\n" % (mode, str(qs[0]), str(qs[1]), len(nodes), m2 // 2), line
        assert label_q in (None, qs[1]) and m2 > 0
        label_q = qs[1]
        assert line == gc.format_modularity(mode, gc.eval_cluster_modularity(gc.host_sweeps(edges, n)[1], n, fit))


def test_refusals(gc, lh, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_cluster_graph_baseline, _check_node_clustering
    cfg, g, n = _layout(tmp_path)
    cfg.engine_cluster_modularity = True
    with pytest.raises(ValueError, match="engine_cluster_modularity needs engine_node_clustering"):
        GraphGAN.evaluation(g)
    with pytest.raises(ValueError, match="engine_cluster_modularity needs engine_node_clustering"):
        _check_node_clustering(types.SimpleNamespace(engine_cluster_modularity=True))
    cfg.engine_cluster_modularity = False
    cfg.engine_cluster_graph_baseline = True
    cfg.labels_filename = str(tmp_path / "no_such_labels.txt")
    with pytest.raises(ValueError, match="engine_cluster_graph_baseline needs labels: config.labels_filename does not exist"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
    with pytest.raises(ValueError, match="labels_filename"):
        _check_cluster_graph_baseline(types.SimpleNamespace(engine_cluster_graph_baseline=True))
    _labels_for(cfg, n, tmp_path)
    for name in ("engine_lpa_n_init", "engine_lpa_max_iters"):
        for bad in (0, -3, 2.5, True, "4"):
            setattr(cfg, name, bad)
            with pytest.raises(ValueError, match="%s must be an integer >= 1" % name):
                _check_cluster_graph_baseline(cfg)
        setattr(cfg, name, 3)
    _check_cluster_graph_baseline(cfg)
    _check_cluster_graph_baseline(types.SimpleNamespace())  # the knob absent: nothing to check
    _check_cluster_graph_baseline(types.SimpleNamespace(engine_cluster_graph_baseline=False, engine_lpa_n_init=0))
    # the module's own refusals, with the texts of the ABI
    ptr, adj = lh.set_adjacency([[0, 1], [1, 2]], 4)
    for call, text in ((lambda: gc.host_neighbor_mode(ptr, adj, [0, 1, -5, 2]), r"host_neighbor_mode: labels\[2\] = -5 is negative"),
                       (lambda: gc.host_neighbor_mode(ptr, adj, [0, 1, 2 ** 31, -1]), r"labels\[2\] = 2147483648 does not fit in 31 bits"),
                       (lambda: gc.host_neighbor_mode(ptr, adj, [0, 1, 2]), r"labels must be an int array \[4\]"),
                       (lambda: gc.host_neighbor_mode(ptr, adj, [0.0, 1, 2, 3]), r"labels must be an int array \[4\]"),
                       (lambda: gc.host_neighbor_mode(ptr, adj, [0, 1, 2, 3], nodes=[0, 4]), r"nodes\[1\] = 4 out of range \[0, 4\)"),
                       (lambda: gc.host_neighbor_mode(ptr, adj, [0, 1, 2, 3], nodes=[-1]), r"nodes\[0\] = -1 out of range \[0, 4\)"),
                       (lambda: gc.host_label_propagation(ptr, adj, max_iters=0), r"host_label_propagation: max_iters = 0 is below 1"),
                       (lambda: gc.host_label_propagation(ptr, adj, max_iters=True), r"max_iters = True is below 1"),
                       (lambda: gc.host_partition_edges(ptr, adj, [0, 1, 2, 0], 2), r"host_partition_edges: assign\[2\] = 2 outside \[-1, 2\)"),
                       (lambda: gc.host_partition_edges(ptr, adj, [0, -2, 2, 0], 2), r"assign\[1\] = -2 outside \[-1, 2\)"),
                       (lambda: gc.host_partition_edges(ptr, adj, [0, 1, 0], 2), r"assign must be an int array \[4\]"),
                       (lambda: gc.host_partition_edges(ptr, adj, [0, 0, 0, 0], 0), r"n_label = 0 is below 1"),
                       (lambda: gc.fit_communities(None, None, n_init=0), r"n_init must be an integer >= 1"),
                       (lambda: gc.GraphCommunityEval("t", "l", 4, n_init=0), r"n_init must be an integer >= 1"),
                       (lambda: gc.GraphCommunityEval("t", "l", 4, max_iters=0), r"max_iters = 0 is below 1")):
        with pytest.raises(ValueError, match=text):
            call()


def test_command_line_on_the_host(gc, tmp_path, capsys):
    from graphgan_amd import communities
    from tests.support import label_spread_ref as ls
    edges, lab, _, _ = ls.planted_partition(0)
    edges = np.concatenate([edges, [[300, 301]]])  # ids 256 .. 299 have no edge: communities of their own
    tfile, out = str(tmp_path / "train.txt"), str(tmp_path / "comm.tsv")
    np.savetxt(tfile, edges, fmt="%d")
    assert communities.main(["--train", tfile, "--out", out, "--host", "--seed", "3", "--n-init", "3", "--max-iters", "50"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert [int(r[0]) for r in rows] == list(range(302)) and all(len(r) == 2 for r in rows)
    N = ref.neighbor_sets(302, edges)
    runs = []
    for seed in (3, 4, 5):
        comm, k = ref.relabel(ref.label_propagation(N, seed, 50)[0])
        runs.append((ref.modularity(*ref.partition_edges(N, comm, k)), -seed, comm, k))
    q, neg_seed, comm, k = max(runs, key=lambda r: r[:2])
    assert [int(r[1]) for r in rows] == comm
    assert capsys.readouterr().out.strip() == "communities=%d Q=%s iters=%d converged=True seed=%d" % (
        k, str(q), ref.label_propagation(N, -neg_seed, 50)[1], -neg_seed)
    assert rows[300][1] == rows[301][1] and len({r[1] for r in rows[256:300]}) == 44
    for bad in (["--n-init", "0"], ["--max-iters", "0"]):
        with pytest.raises(SystemExit):
            communities.main(["--train", tfile, "--out", out, "--host"] + bad)
    with pytest.raises(SystemExit):
        communities.main(["--out", out, "--host"])
