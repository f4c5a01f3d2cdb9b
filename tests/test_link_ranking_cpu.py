"""The host side of full-ranking link evaluation (graphgan_amd/evaluation/link_ranking.py, graph_gan.py's engine_link_rank):
the float64 ranking against a brute-force double loop, the filtered-rank identity against brute-force refiltering, the tie
rule's closed form, the results lines -- and the C ABI's declaration of gg_rank_scores."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lr():
    from graphgan_amd.evaluation import link_ranking
    return link_ranking


def _toy(seed=0, n=40, d=6, n_train=70, n_test=25):
    """40 nodes: random training edges (some twice, some reversed, a self-loop), test pairs that include training neighbours,
    a u == v pair and repeated pairs"""
    rs = np.random.RandomState(seed)
    train = rs.randint(0, n, size=(n_train, 2))
    train = np.concatenate([train, train[:5], train[5:9, ::-1], [[3, 3]]])
    test = rs.randint(0, n, size=(n_test, 2))
    test = np.concatenate([test, train[:3], [[7, 7]], test[:2], test[2:4, ::-1]])
    E = rs.randn(n, d)
    return n, train, test, E


def _nbrs(train, n):
    nb = [set() for _ in range(n)]
    for a, b in np.asarray(train).tolist():
        nb[a].add(b)
        nb[b].add(a)
    return nb


def brute_rank(S, u, v, nbrs=None):
    """the definition, one column at a time: (rank, n_cand) of target v in row S[u]"""
    n = len(S)
    rank = n_cand = 1
    for c in range(n):
        if c == v:
            continue
        if nbrs is not None and (c == u or c in nbrs[u]):
            continue
        n_cand += 1
        if S[u][c] > S[u][v] or (S[u][c] == S[u][v] and c < v):
            rank += 1
    return rank, n_cand


def brute_filtered(u, v, rank):
    test_nbrs = {}
    for a, b, r in zip(u, v, rank):
        test_nbrs.setdefault(a, {})[b] = r
    return [r - sum(1 for b2, r2 in test_nbrs[a].items() if b2 != b and r2 < r) for a, b, r in zip(u, v, rank)]


def _pairs(test):
    p = np.empty((2 * len(test), 2), dtype=np.int64)
    p[0::2], p[1::2] = test, test[:, ::-1]
    return p


@pytest.mark.parametrize("exclude", [False, True])
def test_host_rank_equals_the_brute_force_double_loop(lr, exclude):
    n, train, test, E = _toy()
    p = _pairs(test)
    S = E @ E.T
    nbrs = _nbrs(train, n) if exclude else None
    graph = lr.train_csr(train, n) if exclude else None
    rank, n_cand, score = lr.host_rank(lambda nodes: E[nodes] @ E.T, p[:, 0], p[:, 1], n, graph, chunk=7)
    want = [brute_rank(S, a, b, nbrs) for a, b in p.tolist()]
    assert rank.tolist() == [w[0] for w in want]
    assert n_cand.tolist() == [w[1] for w in want]
    assert np.array_equal(score, S[p[:, 0], p[:, 1]])
    assert (rank >= 1).all() and (rank <= n_cand).all()
    if exclude:  # targets that are training neighbours, and u == v, are ranked among the candidates plus themselves
        assert any(b in nbrs[a] for a, b in p.tolist()) and any(a == b for a, b in p.tolist())


def test_train_csr_lists_are_sorted_and_undirected(lr):
    n, train, _, _ = _toy()
    rowptr, col = lr.train_csr(train, n)
    nbrs = _nbrs(train, n)
    for a in range(n):
        lst = col[rowptr[a]:rowptr[a + 1]]
        assert (np.diff(lst) >= 0).all() and set(lst.tolist()) == nbrs[a]


def test_filtered_rank_identity_against_brute_force_refiltering(lr):
    """rank minus the other test neighbours ranked in front == the rank recomputed with those neighbours removed from the
    candidates (scores without ties: the ranks of one source are positions in one total order)"""
    n, train, test, E = _toy(seed=3)
    p = _pairs(test)
    S = E @ E.T
    nbrs = _nbrs(train, n)
    rank, _, _ = lr.host_rank(lambda nodes: E[nodes] @ E.T, p[:, 0], p[:, 1], n, lr.train_csr(train, n))
    got = lr.filtered_ranks(p[:, 0], p[:, 1], rank)
    assert got.tolist() == brute_filtered(p[:, 0].tolist(), p[:, 1].tolist(), rank.tolist())
    test_nbrs = _nbrs(test, n)
    for (a, b), f in zip(p.tolist(), got.tolist()):
        drop = [set(x) for x in nbrs]
        drop[a] = (nbrs[a] | test_nbrs[a]) - {b}
        if not (test_nbrs[a] - {b}) & (nbrs[a] | {a}):  # (an excluded test neighbour was never counted)
            assert f == brute_rank(S, a, b, drop)[0]
    assert (got >= 1).all() and (got <= rank).all() and (got < rank).any()


def test_filtered_rank_counts_a_repeated_pair_once(lr):
    u = np.array([5, 5, 5, 5, 2])
    v = np.array([1, 9, 1, 4, 1])
    rank = np.array([10, 3, 10, 7, 4])
    assert lr.filtered_ranks(u, v, rank).tolist() == [8, 3, 8, 6, 4]
    assert lr.filtered_ranks([], [], []).tolist() == []


def test_all_equal_scores_rank_by_column(lr):
    """every score ties (an all-zero table, and -0.0 beside +0.0): rank = 1 + the eligible columns below v"""
    n, train, test, _ = _toy(seed=5)
    p = _pairs(test)
    nbrs = _nbrs(train, n)
    Z = np.zeros((n, 4))
    Z[::2] = -0.0
    rank, n_cand, _ = lr.host_rank(lambda nodes: Z[nodes] @ Z.T, p[:, 0], p[:, 1], n, lr.train_csr(train, n))
    for (a, b), r, c in zip(p.tolist(), rank.tolist(), n_cand.tolist()):
        elig = [x for x in range(n) if x != a and x not in nbrs[a] and x != b]
        assert r == 1 + sum(1 for x in elig if x < b) and c == len(elig) + 1
    rank, n_cand, _ = lr.host_rank(lambda nodes: Z[nodes] @ Z.T, p[:, 0], p[:, 1], n)
    assert rank.tolist() == (p[:, 1] + 1).tolist() and (n_cand == n).all()


def test_summarize_and_the_results_line(lr):
    res = lr.summarize([1, 2, 4, 300, 100000], ks=(1, 10, 100, 1000))
    assert res == dict(mrr=(1 + 0.5 + 0.25 + 1 / 300 + 1e-5) / 5, mr=100307 / 5, hits={1: 0.2, 10: 0.6, 100: 0.6, 1000: 0.8}, n=5)
    line = lr.format_results("gen", res, (1, 10, 100, 1000))
    assert line == "gen_rank:MRR=%s MR=20061.4 H@1=0.2 H@10=0.6 H@100=0.6 H@1000=0.8 n=5\n" % str(res["mrr"])
    assert lr.format_results("dis", lr.summarize([1, 1]), (1, 10, 100)) == "dis_rank:MRR=1.0 MR=1.0 H@1=1.0 H@10=1.0 H@100=1.0 n=2\n"
    assert lr.summarize([], ks=(3,)) == dict(mrr=0.0, mr=0.0, hits={3: 0.0}, n=0)
    for bad in ((), (0,), (1.5,), (True,)):
        with pytest.raises(ValueError, match="positive integer"):
            lr.LinkRankEval("e", "tr", "te", 4, 2, emd=np.zeros((4, 2)), ks=bad)
    with pytest.raises(ValueError, match="precision"):
        lr.LinkRankEval("e", "tr", "te", 4, 2, emd=np.zeros((4, 2)), precision="fp16")


# ---- graph_gan.evaluation()
def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


@pytest.mark.parametrize("app", ["link_prediction", "recommendation"])
def test_evaluation_lines_with_and_without_the_knob(lr, tmp_path, app):
    from graphgan_amd import utils
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path, app)
    assert cfg.engine_link_rank is False
    want = GraphGAN.evaluation(g)  # the knob's default: off
    del cfg.engine_link_rank
    assert GraphGAN.evaluation(g) == want and len(want) == 2  # a user's config without the knob
    assert open(cfg.result_filename).read() == "".join(want + want) and "_rank" not in "".join(want)
    cfg.engine_link_rank, cfg.engine_link_rank_ks = True, (1, 10, 100, 1000)
    cfg.engine_lp_classifier, cfg.engine_lp_iters = True, 5
    lines = GraphGAN.evaluation(g)
    assert lines[:2] == want and len(lines) == 6
    assert [ln.split(":")[0] for ln in lines[2:]] == ["gen_lp", "dis_lp", "gen_rank", "dis_rank"]  # behind the *_lp lines
    n_test = len(utils.read_edges_from_file(cfg.test_filename))
    for i, (mode, line) in enumerate(zip(cfg.modes, lines[4:])):
        emd = utils.read_embeddings(cfg.emb_filenames[i], n_node=n, n_embed=cfg.n_emb)
        ev = lr.LinkRankEval("unused", cfg.train_filename, cfg.test_filename, n, cfg.n_emb, emd=emd, ks=(1, 10, 100, 1000))
        res = ev.eval_link_ranking()
        assert line == lr.format_results(mode, res, (1, 10, 100, 1000))
        assert re.fullmatch(r"%s_rank:MRR=\S+ MR=\S+ H@1=\S+ H@10=\S+ H@100=\S+ H@1000=\S+ n=%d\n" % (mode, 2 * n_test), line)
        assert 0.0 < res["mrr"] <= 1.0 and 1.0 <= res["mr"] <= n
        assert res["hits"][1] <= res["hits"][10] <= res["hits"][100] <= res["hits"][1000] <= 1.0
    assert open(cfg.result_filename).read() == "".join(want + want + lines)
    del cfg.engine_link_rank_ks  # the default K
    assert GraphGAN.evaluation(g)[4].count("H@") == 3


def test_evaluation_with_the_knob_needs_the_test_file(tmp_path):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, _ = _layout(tmp_path)
    cfg.engine_link_rank = True
    os.remove(cfg.test_filename)
    with pytest.raises(ValueError, match="engine_link_rank needs test edges.*test_filename"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)  # refused before anything is computed


def test_config_knobs_default_off():
    from graphgan_amd import config
    assert config.engine_link_rank is False
    assert config.engine_link_rank_ks == (1, 10, 100) and config.engine_link_rank_precision == "fp32"


def test_header_declares_and_library_exports_gg_rank_scores():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"int\s+gg_rank_scores\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/graphgan_hip.h does not declare gg_rank_scores"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == [
        "gg_ctx*", "int32_t", "constint32_t*", "constint32_t*", "int64_t", "int32_t", "int32_t", "int32_t*", "int32_t*", "float*", "double*"]
    assert len(_lib.SIGNATURES["gg_rank_scores"][1]) == len(args)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gg_rank_scores")
    assert _lib.header_abi_version() == 9  # additive: the ABI number stays


def test_rank_kernels_are_audited_by_the_build():
    """the count consumer must stay in registers, fully inlined into both producers: the Makefile audits rank_score.o like the
    other tile-stream objects, and the remarks of the current build show one kernel per instantiation and no callee"""
    csrc = os.path.join(ROOT, "graphgan_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^AUDITED = .*\brank_score\.o\b", mk, flags=re.M) and "rank_(f32|bf16)_kernel" in mk
    remarks = os.path.join(csrc, "rank_score.remarks")
    assert os.path.exists(remarks), "rank_score.remarks is written by the build (make -C graphgan_amd/csrc)"
    text = open(remarks).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 10 and all("rank_" in x and "kernel" in x for x in names), names  # kernels only: nothing behind a call
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 10
