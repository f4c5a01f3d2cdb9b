"""The host side of the graph-only pair baseline (graphgan_amd/evaluation/graph_pairs.py, graph_gan.py's engine_pair_graph_baseline /
engine_recon_graph_baseline, the ``python -m graphgan_amd.predict_graph`` command line): the numpy rules against the restatement in
sets and ints (tests/support/two_hop_pairs_ref.py), Adamic-Adar inside the quantisation bound of float64, the positives rule the two
pair evaluators share, the results lines, their place and their caches -- and the ABI declaration of gg_two_hop_top_pairs."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

from tests.support import two_hop_pairs_ref as pref
from tests.support import two_hop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gp():
    from graphgan_amd.evaluation import graph_pairs
    return graph_pairs


@pytest.fixture(scope="module")
def lh():
    from graphgan_amd.evaluation import link_heuristics
    return link_heuristics


def test_header_declares_and_library_exports_the_symbol():
    from graphgan_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = ["gg_ctx*", "constint32_t*", "int64_t", "int64_t", "constuint64_t*", "int32_t", "int64_t", "int64_t", "int32_t*", "int32_t*", "uint64_t*", "int64_t*",
            "int64_t*", "double*"]
    m = re.search(r"int\s+gg_two_hop_top_pairs\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/graphgan_hip.h does not declare gg_two_hop_top_pairs"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == want
    assert [re.sub(r"^.*\W(\w+)$", r"\1", a) for a in args] == ["ctx", "nodes", "m", "k", "weights", "exclude", "scratch_bytes", "buffer_entries", "out_u", "out_v",
                                                              "out_score", "n_found", "stats", "kernel_ms"]
    sig = _lib.SIGNATURES["gg_two_hop_top_pairs"][1]
    assert len(sig) == len(args) and [i for i, t in enumerate(sig) if t is ctypes.c_int64] == [2, 3, 6, 7] and sig[5] is ctypes.c_int32
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "gg_two_hop_top_pairs") and hasattr(_lib.lib, "gg_two_hop_top_pairs")
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "two-hop pair sweep" in text


def test_constants_and_audit_are_in_step_with_the_source(gp):
    from graphgan_amd.engine import Engine
    csrc = os.path.join(ROOT, "graphgan_amd", "csrc")
    src, sweep = open(os.path.join(csrc, "two_hop_pairs.hip")).read(), open(os.path.join(csrc, "two_hop.hip")).read()
    for mine, theirs, kind in (("THP_LDS_CAP", "TH_LDS_CAP", "int"), ("THP_NARROW", "TH_NARROW", "int"), ("THP_BLOCKS", "TH_BLOCKS", "int"),
                               ("THP_SCRATCH", "TH_SCRATCH", "int64_t")):  # the shape of the two-hop sweep, restated
        a = re.search(r"constexpr %s %s = ([^;]+);" % (kind, mine), src)
        b = re.search(r"constexpr %s %s = ([^;]+);" % (kind, theirs), sweep)
        assert a and b and a.group(1) == b.group(1), mine
    assert int(re.search(r"constexpr int THP_LDS_CAP = (\d+);", src).group(1)) == Engine.TWO_HOP_LDS_CAP
    assert re.search(r"constexpr int64_t THP_MAX_K = 1 << 20;", src) and gp.MAX_K == Engine.TWO_HOP_TOP_PAIRS_MAX_K == 1 << 20
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^two_hop_pairs\.o: AUDIT = 'thp_\[a-z0-9_\]\*kernel' 4 ", mk, flags=re.M)  # LDS / global table, with / without the bitmap
    assert re.search(r"^AUDITED = .*\btwo_hop_pairs\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\btwo_hop_pairs\.o\b", mk, flags=re.M)
    assert re.findall(r"^__global__ .*void (thp_\w*kernel)\(", src, flags=re.M) == ["thp_kernel"]
    device = src[:src.index("struct Entry {")]  # the kernel and the consumers' header: no floating point, no inline assembly
    device += open(os.path.join(csrc, "set_consume.h")).read()
    device = re.sub(r"//[^\n]*", "", device)  # (the code; a comment may say that batches double)
    assert not re.search(r"\b(float|double|fmaf?|__f\w+_rn|asm)\b", device)
    assert "set_floor_consume" in device and "atomicAdd(f.fill, total)" in device


def small_graph():
    """60 nodes, the last three isolated, duplicates and self-loops; weights below 2^41 with a zero"""
    rs = np.random.RandomState(0)
    n = 60
    e = rs.randint(0, n - 3, size=(150, 2))
    e = np.concatenate([e, e[:10], e[10:20, ::-1], [[5, 5], [7, 7]]])
    w = rs.randint(0, 2 ** 41, n).astype(np.uint64)
    w[int(e[0, 0])] = 0
    return n, e, w


def test_host_rules_against_the_restatement(gp, lh):
    n, e, w = small_graph()
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    assert np.diff(ptr).tolist() == [len(s) for s in N] and np.diff(ptr)[-3:].tolist() == [0, 0, 0]
    rs = np.random.RandomState(1)
    sets = [None, np.arange(n), np.array([0, 31, 32, n - 1]), np.unique(rs.randint(0, n, 25)), np.array([], dtype=np.int64), np.array([4]), np.array([4, 9])]
    for weights in (None, w):
        for exclude in (True, False):
            for nodes in sets:
                cand = pref.candidates(N, nodes, None if weights is None else weights.tolist(), exclude)
                for k in (1, 7, len(cand), len(cand) + 3) if nodes is None or len(nodes) > 4 else (3,):
                    if k < 1:
                        continue
                    res = gp.host_two_hop_top_pairs(ptr, adj, k, nodes=nodes, weights=weights, exclude=exclude)
                    u, v, s, f = pref.head(cand, k)
                    assert res["u"].dtype == np.int32 and res["v"].dtype == np.int32 and res["score"].dtype == np.uint64
                    assert (res["u"].tolist(), res["v"].tolist(), res["score"].tolist(), res["n_found"]) == (u, v, s, f), (k, exclude)
    full = pref.candidates(N, None, None, False)
    assert len(full) > len(pref.candidates(N, None, None, True)) > 100 and any(c[2] > 1 for c in full)
    # keeping only the k best between sources loses nothing: many merges, one result
    big = gp.host_two_hop_top_pairs(ptr, adj, 50, weights=w)
    assert (big["u"].tolist(), big["v"].tolist(), big["score"].tolist()) == pref.head(pref.candidates(N, None, w.tolist(), True), 50)[:3]
    for bad, text in ((dict(k=0), r"k must be an integer in \[1, 2\^20\]"), (dict(k=2 ** 20 + 1), r"k must be an integer"), (dict(k=3, exclude="self"), "exclude must be True or False"),
                      (dict(k=3, nodes=[3, 3]), r"nodes\[1\] = 3 is not above nodes\[0\] = 3"), (dict(k=3, nodes=[0, n]), r"nodes\[1\] = %d out of range" % n),
                      (dict(k=3, weights=np.ones(n - 1, np.uint64)), "weights must be None or %d non-negative integers" % n)):
        with pytest.raises(ValueError, match="host_two_hop_top_pairs: " + text):
            gp.host_two_hop_top_pairs(ptr, adj, **bad)


def test_adamic_adar_lies_within_the_quantisation_bound_of_float64(gp, lh):
    from graphgan_amd.evaluation import graph_ranking as gr
    n, e, _ = small_graph()
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    deg = np.diff(ptr)
    res = gp.host_two_hop_top_pairs(ptr, adj, 400, weights=gr.index_weights("aa", deg))
    assert res["n_found"] == 400
    for u, v, s in zip(res["u"].tolist(), res["v"].tolist(), res["score"].tolist()):
        common = N[u] & N[v]
        exact = sum(1.0 / math.log(len(N[w])) for w in common)
        # every weight is rint(2^40 / ln deg): half a unit of 2^-40 per common neighbour
        assert abs(s / 2.0 ** 40 - exact) <= len(common) * 2.0 ** -41 + 1e-15 * exact, (u, v)


def test_the_positives_rule_is_one_function_with_the_outputs_it_had(gp, tmp_path):
    from graphgan_amd.evaluation import pair_prediction as pp
    train = [[0, 1], [1, 2], [2, 3], [3, 0], [5, 6], [6, 6]]
    test = [[0, 2], [2, 0], [1, 3], [1, 1], [0, 1], [1, 0], [0, 4], [7, 5], [5, 3], [3, 5], [6, 2]]
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    np.savetxt(tr, train, fmt="%d")
    np.savetxt(te, test, fmt="%d")
    nodes = [0, 1, 2, 3, 5, 6]
    positives, dropped = pp.held_out_positives(test, nodes, pp.undirected(train))
    # kept: (0, 2), (1, 3), (3, 5), (2, 6); dropped: the repeat (2, 0), the loop, the training edge twice, node 4, node 7, the repeat (3, 5)
    assert positives == {(0, 2), (1, 3), (3, 5), (2, 6)} and dropped == 7
    emd = np.random.RandomState(2).randn(8, 4)
    old = pp.PairPredictionEval(tr, te, 8, 4, emd=emd, ks=(2, 5)).eval_pair_prediction()
    assert (old["n_test"], old["dropped"], old["n"]) == (4, 7, 6)
    new = gp.GraphPairsEval(tr, te, 8, ks=(2, 5))
    res = new.eval_graph_pairs()
    assert new.nodes.tolist() == nodes and set(res) == {"cn", "aa", "ra"}
    assert all((r["n_test"], r["dropped"], r["n"]) == (4, 7, 6) for r in res.values())
    # common neighbours on the 4-cycle: (0, 2) and (1, 3) share two nodes each and lead; both are positives
    assert res["cn"]["pr"] == {2: (1.0, 0.5), 5: (0.4, 0.5)} and res["cn"]["found"] == 2
    rec = new.eval_graph_reconstruction()["cn"]
    assert rec["edges"] == 5 and rec["found"] == 2 and rec["pr"][2] == (0.0, 0.0)  # no edge of a 4-cycle has a common neighbour
    assert new.lines("pairs")[0] == "graph_pairs:index=cn P@2=1.0 R@2=0.5 P@5=0.4 R@5=0.5 n_test=4 dropped=7 n=6 found=2\n"
    assert new.lines("recon")[0] == "graph_recon:index=cn P@2=0.0 R@2=0.0 P@5=0.0 R@5=0.0 edges=5 n=6 found=2\n"
    with pytest.raises(ValueError, match="kind must be 'pairs' or 'recon'"):
        new.lines("rank")
    with pytest.raises(ValueError, match="pair prediction needs test edges"):
        gp.GraphPairsEval(tr, None, 8).eval_graph_pairs()


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def test_config_knob_defaults():
    from graphgan_amd import config
    assert config.engine_pair_graph_baseline is False and config.engine_recon_graph_baseline is False
    assert config.engine_graph_rank_indices == ("cn", "aa", "ra") and config.engine_pair_ks == (100, 1000, 10000)


@pytest.mark.parametrize("app", ["link_prediction", "recommendation"])
def test_lines_their_place_their_caches_and_a_config_without_the_knobs(gp, tmp_path, monkeypatch, app):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path, app)
    assert cfg.engine_pair_graph_baseline is False and cfg.engine_recon_graph_baseline is False
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    cfg.engine_lp_heuristics = True
    cfg.engine_pair_ks = (10, 200)
    want = GraphGAN.evaluation(g)  # the knobs' default: off
    first = open(cfg.result_filename, "rb").read()
    del cfg.engine_pair_graph_baseline, cfg.engine_recon_graph_baseline
    assert GraphGAN.evaluation(g) == want and [ln.split(":")[0] for ln in want] == ["gen", "dis", "graph_lp", "gen_nll"]  # a config without them
    assert open(cfg.result_filename, "rb").read() == first + first  # byte-identical
    cfg.engine_pair_graph_baseline, cfg.engine_recon_graph_baseline = True, True
    cfg.engine_graph_rank_indices = ("cn", "ra")
    g._graph_rec_lines = ["graph_rec:index=cn stub\n"]  # (a cached line: the two-hop evaluators have their own test)
    cfg.engine_rec_graph_baseline = True
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_lp", "graph_rec", "graph_pairs", "graph_pairs", "graph_recon", "graph_recon", "gen_nll"]
    assert lines[:3] == want[:3] and lines[8] == want[3]  # the other lines keep every byte
    ev = gp.GraphPairsEval(cfg.train_filename, cfg.test_filename, n, indices=("cn", "ra"), ks=(10, 200))
    assert lines[4:8] == ev.lines("pairs") + ev.lines("recon")
    assert re.fullmatch(r"graph_pairs:index=cn P@10=\d\.\d+ R@10=[\d.e-]+ P@200=\d\.\d+ R@200=[\d.e-]+ n_test=\d+ dropped=\d+ n=\d+ found=200\n", lines[4]), lines[4]
    assert re.fullmatch(r"graph_recon:index=ra P@10=\d\.\d+ R@10=[\d.e-]+ P@200=\d\.\d+ R@200=[\d.e-]+ edges=\d+ n=\d+ found=200\n", lines[7]), lines[7]
    print("CA-GrQc, host: " + " | ".join(ln.strip() for ln in lines[4:8]))
    # the second evaluation repeats the cached strings: nothing is computed again
    monkeypatch.setattr(gp.GraphPairsEval, "lines", lambda self, kind="pairs": pytest.fail("the graph_%s lines were computed twice" % kind))
    assert GraphGAN.evaluation(g) == lines and g._graph_pairs_lines == lines[4:6] and g._graph_recon_lines == lines[6:8]
    cfg.engine_rec_graph_baseline = False  # where the graph_rec line would stand
    assert GraphGAN.evaluation(g) == lines[:3] + lines[4:]
    cfg.engine_pair_graph_baseline = False
    assert GraphGAN.evaluation(g) == lines[:3] + lines[6:]


def test_the_knobs_are_checked_where_the_others_are(gp, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_graph_pairs
    cfg, g, n = _layout(tmp_path)
    test_file, train_file = cfg.test_filename, cfg.train_filename
    cfg.engine_pair_graph_baseline = True
    cfg.test_filename = str(tmp_path / "no_such_test.txt")
    with pytest.raises(ValueError, match="engine_pair_graph_baseline needs test edges: config.test_filename does not exist"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
    with pytest.raises(ValueError, match="engine_pair_graph_baseline needs the training edges"):
        _check_graph_pairs(types.SimpleNamespace(engine_pair_graph_baseline=True))
    cfg.engine_pair_graph_baseline, cfg.engine_recon_graph_baseline = False, True
    _check_graph_pairs(cfg)  # the reconstruction lines need no test edges
    cfg.train_filename = str(tmp_path / "no_such_train.txt")
    with pytest.raises(ValueError, match="engine_recon_graph_baseline needs the training edges: config.train_filename does not exist"):
        _check_graph_pairs(cfg)
    cfg.train_filename, cfg.test_filename = train_file, test_file
    for knob in ("engine_pair_graph_baseline", "engine_recon_graph_baseline"):
        cfg.engine_pair_graph_baseline = cfg.engine_recon_graph_baseline = False
        setattr(cfg, knob, True)
        cfg.engine_graph_rank_indices = ("cn", "ppr")
        with pytest.raises(ValueError, match="index must be one of 'cn', 'aa', 'ra', got 'ppr'"):
            GraphGAN.evaluation(g)
        cfg.engine_graph_rank_indices = ("cn",)
        cfg.engine_pair_ks = (10, 0)
        with pytest.raises(ValueError, match="engine_pair_ks must be a sequence of positive integers"):
            GraphGAN.evaluation(g)
        cfg.engine_pair_ks = (10,)
        _check_graph_pairs(cfg)
    assert not os.path.exists(cfg.result_filename)
    _check_graph_pairs(types.SimpleNamespace())  # the knobs absent: nothing to check
    _check_graph_pairs(types.SimpleNamespace(engine_recon_graph_baseline=False, engine_pair_ks=(0,)))


def test_command_line_on_the_host(gp, lh, tmp_path, capsys):
    from graphgan_amd import predict_graph
    n, e, _ = small_graph()
    tfile, out = str(tmp_path / "train.txt"), str(tmp_path / "pred.tsv")
    np.savetxt(tfile, e, fmt="%d")
    n_file = int(e.max()) + 1
    N = ref.neighbor_sets(n_file, e)
    nodes = sorted(set(e.reshape(-1).tolist()))  # the nodes with an edge: a node with a self-loop alone is one of them
    assert predict_graph.main(["--train", tfile, "--out", out, "--host", "--k", "40"]) == 0  # the default index: cn
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    want = pref.candidates(N, nodes, None, True)[:40]
    assert rows == [[str(u), str(v), str(s)] for u, v, s in want] and len(rows) == 40
    assert capsys.readouterr().out.strip() == "pairs=40 index=cn k=40"
    w = lh.node_weights([len(s) for s in N])[0].tolist()
    assert predict_graph.main(["--train", tfile, "--out", out, "--host", "--k", "100000", "--index", "aa", "--include-known"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    want = pref.candidates(N, nodes, w, False)
    assert rows == [[str(u), str(v), repr(s / 2.0 ** 40)] for u, v, s in want] and 100 < len(rows) < 100000
    assert any((int(r[0]), int(r[1])) in {(min(a, b), max(a, b)) for a, b in e.tolist()} for r in rows)  # known edges are kept
    for bad in (["--k", "0"], ["--k", str(2 ** 20 + 1)], ["--index", "ppr"], []):
        with pytest.raises(SystemExit):
            predict_graph.main(["--train", tfile, "--out", out, "--host"] + bad)
    with pytest.raises(SystemExit):
        predict_graph.main(["--out", out, "--host", "--k", "3"])
