"""The host side of the graph-only ranking baselines (graphgan_amd/evaluation/graph_ranking.py, graph_gan.py's
engine_link_rank_graph_baseline / engine_rec_graph_baseline, the ``python -m graphgan_amd.recommend`` command line): the numpy rules
against the restatement in sets and ints (tests/support/two_hop_ref.py), Adamic-Adar against networkx inside the quantisation bound,
the one rank derivation against the brute-force order, the results lines, their place and their caches -- and the ABI declarations
of gg_two_hop_topk / gg_two_hop_rank."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests.support import two_hop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gr():
    from graphgan_amd.evaluation import graph_ranking
    return graph_ranking


@pytest.fixture(scope="module")
def lh():
    from graphgan_amd.evaluation import link_heuristics
    return link_heuristics


def test_header_declares_and_library_exports_the_two_symbols():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {"gg_two_hop_topk": ["gg_ctx*", "constint32_t*", "int64_t", "int32_t", "constuint64_t*", "int32_t", "int64_t", "int32_t*", "uint64_t*", "int32_t*",
                                "double*"],
            "gg_two_hop_rank": ["gg_ctx*", "constint32_t*", "constint32_t*", "int64_t", "constuint64_t*", "int32_t", "int64_t", "uint64_t*", "int32_t*",
                                "int32_t*", "int32_t*", "double*"]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name) and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["gg_two_hop_topk"][1][2] is ctypes.c_int64 and _lib.SIGNATURES["gg_two_hop_rank"][1][6] is ctypes.c_int64
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "two-hop sweep" in open(_lib.HEADER_PATH).read()


def test_constants_and_audit_are_in_step_with_the_source(gr):
    from graphgan_amd import _lib
    from graphgan_amd.engine import Engine
    src = open(os.path.join(ROOT, "graphgan_amd", "csrc", "two_hop.hip")).read()
    m = re.search(r"constexpr int TH_LDS_CAP = (\d+);", src)
    assert m and int(m.group(1)) == _lib.TWO_HOP_LDS_CAP == Engine.TWO_HOP_LDS_CAP
    assert 2 * int(m.group(1)) * (4 + 8) <= 64 * 1024  # the (column, uint64 sum) table of 2 x CAP slots stays within 64 KiB per workgroup
    m = re.search(r"constexpr int TH_MAX_K = (\d+);", src)
    assert m and int(m.group(1)) == gr.MAX_K == 256
    mk = open(os.path.join(ROOT, "graphgan_amd", "csrc", "Makefile")).read()
    assert re.search(r"^two_hop\.o: AUDIT = 'th_\[a-z0-9_\]\*kernel' 4 ", mk, flags=re.M)  # rank and top-K, each with the table in LDS and global
    assert re.search(r"^AUDITED = .*\btwo_hop\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\btwo_hop\.o\b", mk, flags=re.M)
    assert sorted(re.findall(r"^__global__ .*void (th_\w+_kernel)\(", src, flags=re.M)) == ["th_rank_kernel", "th_topk_kernel"]
    device = src[:src.index("int th_run(")]  # the kernels, and the whole header of their shared parts: no floating point, no inline assembly
    device += open(os.path.join(ROOT, "graphgan_amd", "csrc", "set_sweep.h")).read()
    assert not re.search(r"\b(float|double|fmaf?|__f\w+_rn|asm)\b", device)


def small_graph():
    """60 nodes, the last three isolated, duplicates and self-loops; weights below 2^41 with a zero"""
    rs = np.random.RandomState(0)
    n = 60
    e = rs.randint(0, n - 3, size=(150, 2))
    e = np.concatenate([e, e[:10], e[10:20, ::-1], [[5, 5], [7, 7]]])
    w = rs.randint(0, 2 ** 41, n).astype(np.uint64)
    w[3] = 0
    return n, e, w


def test_host_functions_against_the_restatement(gr, lh):
    n, e, w = small_graph()
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    assert [len(s) for s in N] == np.diff(ptr).tolist() and not N[n - 1]
    rs = np.random.RandomState(1)
    for weights in (None, w):
        for exclude in (True, "self"):
            for k in (1, 7, 256):
                t = gr.host_two_hop_topk(ptr, adj, np.arange(n), k, weights, exclude)
                assert t["col"].dtype == np.int32 and t["score"].dtype == np.uint64 and t["n_pos"].dtype == np.int32
                for u in range(n):
                    col, score, n_pos = ref.topk(N, u, k, weights, exclude)
                    assert (t["col"][u].tolist(), t["score"][u].tolist(), int(t["n_pos"][u])) == (col, score, n_pos)
            u, v = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)  # every target of every query
            r = gr.host_two_hop_rank(ptr, adj, u, v, weights, exclude)
            assert r["rank"].dtype == r["n_cand"].dtype == np.int64 and r["score"].dtype == np.uint64
            for i in rs.permutation(n * n)[:600].tolist() + [0, n - 1, n * n - 1]:
                want = ref.rank(N, int(u[i]), int(v[i]), weights, exclude)
                assert {key: int(r[key][i]) for key in want} == want
            # the scores are the pair-neighbour sweep's
            pn = lh.host_pair_neighbors(ptr, adj, u, v, None if weights is None else weights[None, :])
            assert r["score"].tolist() == (pn["cn"].tolist() if weights is None else pn["wsum"][0].tolist())
    assert gr.host_two_hop_topk(ptr, adj, [], 3)["col"].shape == (0, 3) and gr.host_two_hop_rank(ptr, adj, [], [])["rank"].shape == (0,)


def test_full_rank_places_zero_score_targets_without_visiting_them(gr, lh):
    """the derivation alone, from the restatement's counts: targets 0, n - 1, mid-range, u itself, neighbours, in both modes"""
    n, e, w = small_graph()
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    u, v = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    for exclude, code in ((True, 2), ("self", 1)):
        want = [ref.rank(N, a, b, None, exclude) for a, b in zip(u.tolist(), v.tolist())]
        cols = {key: np.array([x[key] for x in want]) for key in want[0]}
        assert (cols["score"] == 0).sum() > n * n // 2 and (cols["score"][v == 0] == 0).any() and (cols["score"][v == n - 1] == 0).all()
        rank, n_cand = gr.full_rank(ptr, adj, u, v, code, cols["score"], cols["ahead"], cols["n_pos"], cols["pos_below"])
        assert rank.tolist() == cols["rank"].tolist() and n_cand.tolist() == cols["n_cand"].tolist()
    assert gr.full_rank(ptr, adj, [], [], 2, [], [], [], [])[0].shape == (0,)


def test_adamic_adar_against_networkx_inside_the_quantisation_bound(gr, lh):
    nx = pytest.importorskip("networkx")
    n, e, _ = small_graph()
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((a, b) for a, b in e.tolist() if a != b)
    ptr, adj = lh.set_adjacency(e, n)
    deg = np.diff(ptr)
    u, v = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    keep = u != v
    u, v = u[keep], v[keep]
    aa = gr.host_two_hop_rank(ptr, adj, u, v, gr.index_weights("aa", deg), "self")["score"].astype(np.float64) / lh.SCALE
    cn = gr.host_two_hop_rank(ptr, adj, u, v, None, "self")["score"]
    want = np.array([p for _, _, p in nx.adamic_adar_index(G, list(zip(u.tolist(), v.tolist())))])
    # link_heuristics' bound: every weight is rounded by at most 2^-41, so a sum of cn of them by at most cn * 2^-41 (+ the float64
    # rounding of networkx's own sum, below 1e-12 here)
    assert np.all(np.abs(aa - want) <= cn * 2.0 ** -41 + 1e-12) and want.max() > 1.0
    assert [c for _, c, _ in sorted(((-p, c, 0) for c, p in zip(v[u == 4].tolist(), want[u == 4].tolist()) if p > 0))[:3]] == [
        c for c in gr.host_two_hop_topk(ptr, adj, [4], 3, gr.index_weights("aa", deg), "self")["col"][0].tolist() if c >= 0][:3]


def test_index_weights_and_the_refusals(gr, lh):
    deg = np.array([0, 1, 2, 5])
    assert gr.index_weights("cn", deg) is None
    assert gr.index_weights("aa", deg).tolist() == lh.node_weights(deg)[0].tolist() and gr.index_weights("ra", deg).tolist() == lh.node_weights(deg)[1].tolist()
    assert gr.index_weights("aa", deg).dtype == np.uint64 and gr.index_weights("aa", deg).flags["C_CONTIGUOUS"]
    ptr, adj = lh.set_adjacency([[0, 1], [1, 2]], 4)
    for call, text in ((lambda: gr.index_weights("jaccard", deg), r"index must be one of 'cn', 'aa', 'ra', got 'jaccard'"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0], exclude=False), r"host_two_hop_topk: exclude must be True or 'self', got False: .*rank first for itself"),
                       (lambda: gr.host_two_hop_rank(ptr, adj, [0], [1], exclude=False), r"host_two_hop_rank: exclude must be True or 'self', got False"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0], exclude="graph"), r"exclude must be True or 'self', got 'graph'"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0], k=0), r"k must be an integer in \[1, 256\], got 0"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0], k=257), r"k must be an integer in \[1, 256\], got 257"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0, 4]), r"host_two_hop_topk: rows\[1\] = 4 out of range \[0, 4\)"),
                       (lambda: gr.host_two_hop_rank(ptr, adj, [0, -1], [0, 0]), r"host_two_hop_rank: u\[1\] = -1 out of range \[0, 4\)"),
                       (lambda: gr.host_two_hop_rank(ptr, adj, [0, 1], [9, 0]), r"host_two_hop_rank: v\[0\] = 9 out of range \[0, 4\)"),
                       (lambda: gr.host_two_hop_rank(ptr, adj, [0, 1], [0]), r"u and v must have the same length, got 2 and 1"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0], weights=[1, 2, 3]), r"weights must be None or 4 non-negative integers"),
                       (lambda: gr.host_two_hop_topk(ptr, adj, [0], weights=[1, 2, 3, -1]), r"weights must be None or 4 non-negative integers"),
                       (lambda: gr.check_scratch("f", 0), r"f: scratch_bytes must be None or a positive integer, got 0"),
                       (lambda: gr.GraphRankEval("t", "e", 4, indices=("cn", "katz")), r"index must be one of 'cn', 'aa', 'ra', got 'katz'"),
                       (lambda: gr.GraphRankEval("t", "e", 4, indices=()), r"at least one index"),
                       (lambda: gr.GraphRankEval("t", "e", 4, ks=(1, 0)), r"GraphRankEval: every K must be a positive integer"),
                       (lambda: gr.GraphRecEval("t", "e", 4, ks=(2, 257)), r"GraphRecEval: every K must lie in \[1, 256\]"),
                       (lambda: gr.GraphRecEval("t", "e", 4, ks=()), r"GraphRecEval: every K must lie in \[1, 256\]"),
                       (lambda: gr.format_results("lp", "cn", {}, ()), r"kind must be 'rank' or 'rec'")):
        with pytest.raises(ValueError, match=text):
            call()
    assert gr.check_scratch("f", None) == 0 and gr.check_scratch("f", 4096) == 4096 and gr.check_exclude("f", True) == 2 and gr.check_exclude("f", "self") == 1


def test_filtered_ranks_are_link_rankings_and_the_lines_are_what_they_say(gr, lh, tmp_path):
    from graphgan_amd.evaluation import link_ranking as lrank
    from graphgan_amd.evaluation import recommendation as rec
    n, e, _ = small_graph()
    train, test = e[:120], np.array([[a, b] for a, b in e[120:150].tolist() if a != b] + [[0, n - 1]])
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    np.savetxt(tr, train, fmt="%d")
    np.savetxt(te, test, fmt="%d")
    N = ref.neighbor_sets(n, train)
    ks = (1, 3, 50)
    ev = gr.GraphRankEval(tr, te, n, indices=("cn", "ra"), ks=ks)
    res = ev.eval_graph_ranking()
    pairs = np.concatenate([np.stack([test[:, 0], test[:, 1]], axis=1), np.stack([test[:, 1], test[:, 0]], axis=1)]).reshape(2, -1, 2).transpose(1, 0, 2).reshape(-1, 2)
    deg = [len(s) for s in N]
    for index in ("cn", "ra"):
        w = None if index == "cn" else lh.node_weights(deg)[1].tolist()
        got = [ref.rank(N, a, b, w, True) for a, b in pairs.tolist()]
        ranks = lrank.filtered_ranks(pairs[:, 0], pairs[:, 1], [x["rank"] for x in got])  # link_ranking's own filter and summary
        want = lrank.summarize(ranks, ks)
        want["reach"] = sum(1 for x in got if x["score"] > 0) / len(pairs)
        assert res[index] == want and 0.0 < want["reach"] < 1.0
        line = gr.format_results("rank", index, res[index], ks)
        assert line == "graph_rank:index=%s MRR=%s MR=%s H@1=%s H@3=%s H@50=%s n=%d reach=%s\n" % (
            index, str(want["mrr"]), str(want["mr"]), str(want["hits"][1]), str(want["hits"][3]), str(want["hits"][50]), len(pairs), str(want["reach"]))
    assert ev.lines() == [gr.format_results("rank", i, res[i], ks) for i in ("cn", "ra")]
    # the recommendation line: RecommendEval's queries and scoring; a -1 column is a miss
    rk = (2, 5)
    rev = gr.GraphRecEval(tr, te, n, indices=("aa",), ks=rk)
    test_nbrs = rec._neighbour_sets(test.tolist(), n)
    queries = [u for u in range(n) if test_nbrs[u]]
    w = lh.node_weights(deg)[0].tolist()
    ranked = np.array([ref.topk(N, u, 5, w, True)[0] for u in queries])
    assert (ranked == -1).any()
    want = rec.precision_recall(ranked, queries, test_nbrs, rk)
    assert rev.eval_graph_recommendation() == {"aa": want}
    assert rev.lines() == ["graph_rec:index=aa P@2=%s R@2=%s P@5=%s R@5=%s\n" % (str(want[2][0]), str(want[2][1]), str(want[5][0]), str(want[5][1]))]


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def test_config_knob_defaults():
    from graphgan_amd import config
    assert config.engine_link_rank_graph_baseline is False and config.engine_rec_graph_baseline is False
    assert config.engine_graph_rank_indices == ("cn", "aa", "ra")


@pytest.mark.parametrize("app", ["link_prediction", "recommendation"])
def test_lines_their_place_their_caches_and_a_config_without_the_knobs(gr, tmp_path, monkeypatch, app):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path, app)
    assert cfg.engine_link_rank_graph_baseline is False and cfg.engine_rec_graph_baseline is False
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    cfg.engine_lp_heuristics = True
    cfg.engine_link_rank_ks, cfg.engine_rec_ks = (1, 20), (3, 10)
    want = GraphGAN.evaluation(g)  # the knobs' default: off
    first = open(cfg.result_filename, "rb").read()
    del cfg.engine_link_rank_graph_baseline, cfg.engine_rec_graph_baseline, cfg.engine_graph_rank_indices
    assert GraphGAN.evaluation(g) == want and [ln.split(":")[0] for ln in want] == ["gen", "dis", "graph_lp", "gen_nll"]  # a config without them
    assert open(cfg.result_filename, "rb").read() == first + first  # byte-identical
    cfg.engine_link_rank_graph_baseline, cfg.engine_rec_graph_baseline = True, True
    cfg.engine_graph_rank_indices = ("aa",)  # (several indices, in the knob's order: the evaluators' own test above)
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_lp", "graph_rank", "graph_rec", "gen_nll"]
    assert lines[:3] == want[:3] and lines[5] == want[3]  # the other lines keep every byte
    direct = gr.GraphRankEval(cfg.train_filename, cfg.test_filename, n, indices=("aa",), ks=(1, 20)).lines()
    direct += gr.GraphRecEval(cfg.train_filename, cfg.test_filename, n, indices=("aa",), ks=(3, 10)).lines()
    assert lines[3:5] == direct
    assert re.fullmatch(r"graph_rank:index=aa MRR=0\.\d+ MR=\d+\.\d+ H@1=0\.\d+ H@20=0\.\d+ n=\d+ reach=0\.\d+\n", lines[3]), lines[3]
    assert re.fullmatch(r"graph_rec:index=aa P@3=0\.\d+ R@3=0\.\d+ P@10=0\.\d+ R@10=0\.\d+\n", lines[4]), lines[4]
    print("CA-GrQc, host: " + " | ".join(ln.strip() for ln in lines[3:5]))
    # the second evaluation repeats the cached strings: nothing is computed again
    monkeypatch.setattr(gr.GraphRankEval, "lines", lambda self: pytest.fail("the graph_rank lines were computed twice"))
    monkeypatch.setattr(gr.GraphRecEval, "lines", lambda self: pytest.fail("the graph_rec lines were computed twice"))
    assert GraphGAN.evaluation(g) == lines and g._graph_rank_lines == lines[3:4] and g._graph_rec_lines == lines[4:5]
    assert open(cfg.result_filename, "rb").read() == first + first + "".join(lines + lines).encode()


def test_the_knobs_are_checked_where_the_others_are(gr, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_graph_ranking
    cfg, g, n = _layout(tmp_path)
    test_file = cfg.test_filename
    for knob in ("engine_link_rank_graph_baseline", "engine_rec_graph_baseline"):
        setattr(cfg, knob, True)
        cfg.test_filename = str(tmp_path / "no_such_test.txt")
        with pytest.raises(ValueError, match="%s needs test edges: config.test_filename does not exist" % knob):
            GraphGAN.evaluation(g)
        assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
        with pytest.raises(ValueError, match="test_filename"):
            _check_graph_ranking(types.SimpleNamespace(**{knob: True}))
        cfg.test_filename = test_file
        cfg.engine_graph_rank_indices = ("cn", "pa")
        with pytest.raises(ValueError, match="index must be one of 'cn', 'aa', 'ra', got 'pa'"):
            GraphGAN.evaluation(g)
        cfg.engine_graph_rank_indices = ("cn",)
        _check_graph_ranking(cfg)
        setattr(cfg, knob, False)
    cfg.engine_link_rank_graph_baseline, cfg.engine_link_rank_ks = True, (1, 0)
    with pytest.raises(ValueError, match="GraphRankEval: every K must be a positive integer"):
        GraphGAN.evaluation(g)
    cfg.engine_link_rank_graph_baseline, cfg.engine_rec_graph_baseline, cfg.engine_rec_ks = False, True, (2, 300)
    with pytest.raises(ValueError, match=r"GraphRecEval: every K must lie in \[1, 256\]"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    _check_graph_ranking(types.SimpleNamespace())  # the knobs absent: nothing to check
    _check_graph_ranking(types.SimpleNamespace(engine_rec_graph_baseline=False, engine_rec_ks=(0,)))


def test_command_line_on_the_host(gr, lh, tmp_path, capsys):
    from graphgan_amd import recommend
    n, e, _ = small_graph()
    tfile, out, nodes_file = str(tmp_path / "train.txt"), str(tmp_path / "rec.tsv"), str(tmp_path / "ids.txt")
    np.savetxt(tfile, e, fmt="%d")
    n_file = int(e.max()) + 1
    N = ref.neighbor_sets(n_file, e)
    deg = [len(s) for s in N]
    assert recommend.main(["--train", tfile, "--out", out, "--host", "--k", "4", "--index", "cn"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    want = []
    for u in range(n_file):
        if N[u]:
            col, score, _ = ref.topk(N, u, 4, None, True)
            want += [[str(u), str(c), str(s)] for c, s in zip(col, score) if c >= 0]
    assert rows == want and len(rows) > n_file
    assert capsys.readouterr().out.strip() == "nodes=%d lines=%d index=cn k=4" % (sum(1 for s in N if s), len(want))
    with open(nodes_file, "w") as f:
        f.write("7\n3\n7\n")
    assert recommend.main(["--train", tfile, "--out", out, "--host", "--nodes", nodes_file]) == 0  # the defaults: aa, k = 10
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    w = lh.node_weights(deg)[0].tolist()
    want = []
    for u in (7, 3, 7):
        col, score, _ = ref.topk(N, u, 10, w, True)
        want += [[str(u), str(c), repr(s / 2.0 ** 40)] for c, s in zip(col, score) if c >= 0]
    assert rows == want and rows
    for bad in (["--k", "0"], ["--k", "257"], ["--index", "pa"]):
        with pytest.raises(SystemExit):
            recommend.main(["--train", tfile, "--out", out, "--host"] + bad)
    with open(nodes_file, "w") as f:
        f.write("%d\n" % n_file)
    with pytest.raises(SystemExit):
        recommend.main(["--train", tfile, "--out", out, "--host", "--nodes", nodes_file])
    with pytest.raises(SystemExit):
        recommend.main(["--out", out, "--host"])
