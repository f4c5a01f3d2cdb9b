"""The host side of global top-K pair prediction (graphgan_amd/evaluation/pair_prediction.py, graph_gan.py's
engine_pair_prediction / engine_graph_reconstruction, the ``python -m graphgan_amd.predict`` command line) -- the float64 query
against brute force, P@K / R@K by hand, both results lines, their place and `dropped`, every refusal -- the C ABI's declaration
of gg_top_pairs, the build's audit of its kernels, and the restatement of the device schedule the GPU tests rely on."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests.support import top_pairs_ref as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphgan_amd", "csrc")


@pytest.fixture(scope="module")
def pp():
    from graphgan_amd.evaluation import pair_prediction
    return pair_prediction


def test_header_declares_and_library_exports_gg_top_pairs():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = ["gg_ctx*", "int32_t", "int32_t", "constint32_t*", "int64_t", "int64_t", "int32_t", "int64_t", "int32_t*", "int32_t*", "float*", "int64_t*",
            "int64_t*", "double*"]
    m = re.search(r"int\s+gg_top_pairs\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/graphgan_hip.h does not declare gg_top_pairs"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == want
    sig = _lib.SIGNATURES["gg_top_pairs"][1]
    assert len(sig) == len(args) and sig[4] is ctypes.c_int64 and sig[5] is ctypes.c_int64 and sig[7] is ctypes.c_int64
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "gg_top_pairs") and hasattr(_lib.lib, "gg_top_pairs")
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "pair consumer" in open(_lib.HEADER_PATH).read()


def test_every_pair_instance_is_audited_and_passes():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^top_pairs\.o: AUDIT = 'tp_\(f32\|bf16\)_kernel' (\d+) ", mk, flags=re.M)
    assert m and int(m.group(1)) == 5 * 2  # (fp32 + 4 bf16 widths) x (with, without the set's bitmap)
    assert re.search(r"^OBJ = .*\btop_pairs\.o\b", mk, flags=re.M) and re.search(r"^AUDITED = .*\btop_pairs\.o\b", mk, flags=re.M)
    remarks = os.path.join(CSRC, "top_pairs.remarks")
    assert os.path.isfile(remarks), "the build leaves top_pairs.remarks"
    r = subprocess.run(["bash", os.path.join(CSRC, "check_no_scratch.sh"), remarks, "tp_(f32|bf16)_kernel", "10", "pair tile-stream kernels"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "10 pair tile-stream kernels, no scratch, no spill" in r.stdout, r.stdout + r.stderr
    names = set(re.findall(r"Function Name: (\S*tp_(?:f32|bf16)_kernel\S*)", open(remarks).read()))
    assert len(names) == 10 and sum("Lb1E" in x for x in names) == 5


def _brute(X, nodes, k, graph):
    """the definition pair by pair"""
    ids = list(range(len(X))) if nodes is None else list(nodes)
    items = []
    for i, u in enumerate(ids):
        for v in ids[i + 1:]:
            if graph is not None and v in graph[u]:
                continue
            items.append((-(float(np.dot(X[u], X[v])) + 0.0), u, v))
    items.sort()
    return items[:k]


def test_host_top_pairs_against_brute_force(pp):
    rs = np.random.RandomState(3)
    X = rs.randint(-1, 2, size=(70, 5)).astype(np.float64)   # small integers: ties everywhere
    X[9] = 0.0
    edges = rs.randint(0, 70, size=(150, 2)).tolist() + [[4, 4], [1, 2], [2, 1], [1, 2]]
    graph = pp.neighbour_sets(edges, 70)
    some = np.array(sorted(set(rs.randint(0, 70, size=30).tolist()) | {0, 69}))
    for nodes in (None, some, np.array([5]), np.array([], dtype=np.int64), np.array([3, 60])):
        for g in (None, graph):
            for k in (1, 7, 200, 5000):
                for block in (4, 512):
                    res = pp.host_top_pairs(X, nodes, k, graph=g, block=block)
                    want = _brute(X, nodes, k, g)
                    f = res["n_found"]
                    assert f == len(want) and res["u"].shape == (k,) and res["u"].dtype == np.int32
                    assert list(zip((-res["score"][:f]).tolist(), res["u"][:f].tolist(), res["v"][:f].tolist())) == [(s + 0.0, u, v) for s, u, v in want]
                    assert (res["u"][f:] == -1).all() and (res["v"][f:] == -1).all() and np.isneginf(res["score"][f:]).all()
    with pytest.raises(ValueError, match="strictly ascending"):
        pp.host_top_pairs(X, [3, 3], 2)
    # the test reference agrees with it
    S = tp.gram(X)
    for g in (None, graph):
        a, b = tp.ref_top_pairs(S, 300, some, g), pp.host_top_pairs(X, some, 300, graph=g)
        assert np.array_equal(a[0], b["u"]) and np.array_equal(a[1], b["v"]) and np.array_equal(a[2], b["score"]) and a[3] == b["n_found"]


def test_precision_recall_by_hand(pp):
    pairs = [(0, 1), (2, 3), (0, 5), (1, 4), (6, 7)]
    positives = {(2, 3), (1, 4), (8, 9), (6, 7)}
    pr = pp.precision_recall(pairs, positives, (1, 2, 4, 5, 10))
    assert pr == {1: (0.0, 0.0), 2: (0.5, 0.25), 4: (0.5, 0.5), 5: (0.6, 0.75), 10: (0.3, 0.75)}  # K beyond the list: hits / K
    nan = pp.precision_recall(pairs, set(), (2,))[2]
    assert nan[0] == 0.0 and np.isnan(nan[1])
    assert pp.precision_recall([], positives, (3,)) == {3: (0.0, 0.0)}
    res = dict(pr=pr, n_test=4, dropped=2, n=10, found=5, precision="fp32", edges=4)
    assert pp.format_pairs("gen", res, (2, 5)) == "gen_pairs:P@2=0.5 R@2=0.25 P@5=0.6 R@5=0.75 n_test=4 dropped=2 n=10 found=5 precision=fp32\n"
    assert pp.format_recon("dis", res, (1,)) == "dis_recon:P@1=0.0 R@1=0.0 edges=4 n=10 found=5 precision=fp32\n"


def test_evaluator_positives_and_dropped(pp, tmp_path):
    train = [(0, 1), (1, 2), (2, 3), (3, 4), (1, 0), (5, 5), (4, 6)]
    test = [(0, 2), (2, 0), (0, 1), (3, 3), (1, 9), (4, 1), (0, 2), (6, 0)]   # duplicate, training edge, self-loop, node 9 untrained
    for name, ee in (("train.txt", train), ("test.txt", test)):
        with open(tmp_path / name, "w") as f:
            f.writelines("%d\t%d\n" % e for e in ee)
    X = np.zeros((10, 3))
    X[[0, 2], 0] = 3.0      # (0, 2) is the best pair; then those of node 4 with 1 and 6 ... (4, 6) is a training edge
    X[[1, 4, 6], 1] = 2.0
    ev = pp.PairPredictionEval(str(tmp_path / "train.txt"), str(tmp_path / "test.txt"), 10, 3, emd=X, ks=(1, 2, 3))
    assert ev.nodes.tolist() == [0, 1, 2, 3, 4, 5, 6] and ev.train_edges == {(0, 1), (1, 2), (2, 3), (3, 4), (4, 6)}
    res = ev.eval_pair_prediction()
    assert (res["n_test"], res["dropped"], res["n"], res["found"]) == (3, 5, 7, 3)      # positives (0, 2), (1, 4), (0, 6)
    assert res["pr"] == {1: (1.0, 1 / 3), 2: (1.0, 2 / 3), 3: (2 / 3, 2 / 3)}            # ranking: (0, 2), (1, 4), (1, 6), ...
    rec = ev.eval_graph_reconstruction()
    assert (rec["edges"], rec["found"]) == (5, 3) and rec["pr"] == {1: (0.0, 0.0), 2: (0.0, 0.0), 3: (0.0, 0.0)}   # (0, 2), (1, 4), (1, 6)
    ev4 = pp.PairPredictionEval(str(tmp_path / "train.txt"), None, 10, 3, emd=X, ks=(4,))
    assert ev4.eval_graph_reconstruction()["pr"][4] == (0.25, 0.2)                       # the fourth pair is the training edge (4, 6)
    with pytest.raises(ValueError, match="needs test edges"):
        ev4.eval_pair_prediction()
    for bad, text in ((dict(ks=()), "engine_pair_ks"), (dict(ks=(0,)), "engine_pair_ks"), (dict(ks=(1 << 21,)), "engine_pair_ks"),
                      (dict(ks=(True,)), "engine_pair_ks"), (dict(ks=3), "engine_pair_ks"), (dict(precision="fp16"), "engine_pair_precision"),
                      (dict(emd=None), "needs an engine or an embedding matrix")):
        with pytest.raises(ValueError, match=text):
            pp.PairPredictionEval(str(tmp_path / "train.txt"), None, 10, 3, **dict(dict(emd=X), **bad))


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def test_config_knobs_default_off():
    from graphgan_amd import config
    assert config.engine_pair_prediction is False and config.engine_graph_reconstruction is False
    assert config.engine_pair_ks == (100, 1000, 10000) and config.engine_pair_precision == "fp32"


def test_evaluation_lines_their_place_and_knobs_off(pp, tmp_path):
    from graphgan_amd import utils
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path)
    cfg.engine_lp_heuristics = cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    want = GraphGAN.evaluation(g)  # the knobs' default: off
    del cfg.engine_pair_prediction, cfg.engine_graph_reconstruction, cfg.engine_pair_ks, cfg.engine_pair_precision
    assert GraphGAN.evaluation(g) == want and [ln.split(":")[0] for ln in want] == ["gen", "dis", "graph_lp", "gen_nll"]
    assert open(cfg.result_filename).read() == "".join(want + want) and "_pairs" not in "".join(want) and "_recon" not in "".join(want)
    cfg.engine_pair_prediction = cfg.engine_graph_reconstruction = True
    cfg.engine_pair_ks = (10, 300)
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "gen_pairs", "dis_pairs", "gen_recon", "dis_recon", "graph_lp", "gen_nll"]
    assert lines[:2] == want[:2] and lines[6:] == want[2:]
    for i, mode in enumerate(cfg.modes):
        emd = utils.read_embeddings(cfg.emb_filenames[i], n_node=n, n_embed=cfg.n_emb)
        ev = pp.PairPredictionEval(cfg.train_filename, cfg.test_filename, n, cfg.n_emb, emd=emd, ks=(10, 300))
        assert lines[2 + i] == pp.format_pairs(mode, ev.eval_pair_prediction(), (10, 300))
        assert lines[4 + i] == pp.format_recon(mode, ev.eval_graph_reconstruction(), (10, 300))
        assert re.fullmatch(r"%s_pairs:P@10=\S+ R@10=\S+ P@300=\S+ R@300=\S+ n_test=\d+ dropped=\d+ n=\d+ found=300 precision=fp32\n" % mode, lines[2 + i])
        assert re.fullmatch(r"%s_recon:P@10=\S+ R@10=\S+ P@300=\S+ R@300=\S+ edges=\d+ n=\d+ found=300 precision=fp32\n" % mode, lines[4 + i])
    assert open(cfg.result_filename).read() == "".join(want + want + lines)
    cfg.engine_pair_prediction = False
    cfg.engine_pair_ks = (5,)
    assert [ln.split(":")[0] for ln in GraphGAN.evaluation(g)] == ["gen", "dis", "gen_recon", "dis_recon", "graph_lp", "gen_nll"]


def test_refusals_come_before_anything_is_computed(tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_pair_prediction
    cfg, g, n = _layout(tmp_path)
    test_filename = cfg.test_filename
    cfg.engine_pair_prediction = True
    cfg.test_filename = str(tmp_path / "no_such_test.txt")
    with pytest.raises(ValueError, match="engine_pair_prediction needs test edges: config.test_filename does not exist"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    with pytest.raises(ValueError, match="engine_graph_reconstruction needs the training edges"):
        _check_pair_prediction(types.SimpleNamespace(engine_graph_reconstruction=True))
    with pytest.raises(ValueError, match="engine_pair_prediction needs the training edges"):
        _check_pair_prediction(types.SimpleNamespace(engine_pair_prediction=True, train_filename=str(tmp_path / "nope")))
    cfg.test_filename = test_filename
    for ks in ((), (0, 10), (10, (1 << 20) + 1), (2.5,), 7):
        cfg.engine_pair_ks = ks
        with pytest.raises(ValueError, match="engine_pair_ks must be a sequence of positive integers"):
            GraphGAN.evaluation(g)
    cfg.engine_pair_ks = (10,)
    cfg.engine_pair_precision = "fp16"
    with pytest.raises(ValueError, match="engine_pair_precision must be 'fp32' or 'bf16'"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    _check_pair_prediction(types.SimpleNamespace())  # knobs absent: nothing to check


def test_command_line_on_the_host(pp, tmp_path):
    from graphgan_amd import predict
    rs = np.random.RandomState(6)
    ids = np.array([3, 4, 9, 10, 11, 20, 21, 22, 40])
    X = rs.randint(-2, 3, size=(len(ids), 4)).astype(np.float64)
    emb, out, train = str(tmp_path / "x.emb"), str(tmp_path / "pred.tsv"), str(tmp_path / "train.txt")
    with open(emb, "w") as f:
        f.write("%d\t4\n" % len(ids))
        for i in rs.permutation(len(ids)):  # rows in any order
            f.write("%d\t%s\n" % (ids[i], "\t".join(repr(float(v)) for v in X[i])))
    edges = [(3, 9), (9, 20), (20, 3), (40, 21), (21, 22), (9, 3)]   # nodes 4, 10, 11 have no training edge
    with open(train, "w") as f:
        f.writelines("%d\t%d\n" % e for e in edges)
    pos = {int(v): i for i, v in enumerate(ids)}
    graph = pp.neighbour_sets([(pos[a], pos[b]) for a, b in edges], len(ids))
    trained = sorted({pos[a] for e in edges for a in e})

    def rows_of():
        return [ln.rstrip("\n").split("\t") for ln in open(out)]

    for flags, nodes, g in (([], trained, graph), (["--include-known"], trained, None), (["--all-nodes"], None, graph),
                            (["--all-nodes", "--include-known"], None, None)):
        assert predict.main(["--emb", emb, "--train", train, "--k", "12", "--host", "--out", out] + flags) == 0
        want = _brute(X, nodes, 12, g)
        assert [(int(r[0]), int(r[1]), float(r[2])) for r in rows_of()] == [(int(ids[u]), int(ids[v]), -s + 0.0) for s, u, v in want]
    assert predict.main(["--emb", emb, "--train", train, "--k", "1000", "--host", "--out", out]) == 0
    assert len(rows_of()) == len(trained) * (len(trained) - 1) // 2 - 5     # every pair but the 5 distinct training edges
    for bad in (["--k", "0"], ["--k", str((1 << 20) + 1)], ["--k", "3", "--precision", "fp16"]):
        with pytest.raises(SystemExit):
            predict.main(["--emb", emb, "--train", train, "--host", "--out", out] + bad)
    with open(train, "a") as f:
        f.write("3\t5\n")
    with pytest.raises(SystemExit):
        predict.main(["--emb", emb, "--train", train, "--k", "3", "--host", "--out", out])


def test_schedule_restatement_counts():
    """the arithmetic of the device schedule, as tests/test_gpu_top_pairs.py asserts it against the device's stats"""
    S = tp.gram(tp.ascending_table(257, 8))
    sim = tp.simulate_schedule(S, 1, 1 + 4096)
    assert sim["retries"] > 0 and sim["launches"] > sim["retries"] and sim["compactions"] >= 1
    big = tp.simulate_schedule(S, 1, 1 << 22)                  # the whole triangle fits: one rectangle, the final compaction
    assert big == dict(launches=1, retries=0, compactions=1, appended=257 * 256 // 2)
    # the all-zero table: everything ties; only pairs lexicographically below the floor pass once k are known
    Z = np.zeros((257, 257), dtype=np.float32)
    sim = tp.simulate_schedule(Z, 10, 10 + 4096)
    assert sim["retries"] == 0 and sim["appended"] < 257 * 256 // 2
    assert tp.simulate_schedule(Z, 5, 5 + 4096, nodes=[7]) == dict(launches=0, retries=0, compactions=0, appended=0)
