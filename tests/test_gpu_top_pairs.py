"""Global top-K pair prediction on the device (graphgan_amd/csrc/top_pairs.hip: gg_top_pairs, Engine.top_pairs) and the
PairPredictionEval lines with an engine.

Everything is checked EXACTLY -- u, v, the bits of score and n_found -- against tests/support/top_pairs_ref.py: plain numpy over a
full score matrix.  Integer tables of {-1, 0, 1} are exact in fp32 and bf16 in any summation order; fp32 Gaussian tables take
their score matrix from the oracle's fp32 rows (the k-ordered fmaf chain), bf16 Gaussian tables from Engine.topk over all rows
with k = N (the top-K consumer: existing code on the same stream).  The counts of retries and compactions are predicted by the
restatement of the host schedule before they are asserted."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc
from tests.support import top_pairs_ref as tp

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def buffers(k):
    return (k + 4096, 2 * (k + 4096), None)


def assert_equal(res, want, k, ctx=""):
    u, v, s, f = want
    assert res["n_found"] == f, (ctx, res["n_found"], f)
    assert res["u"].dtype == np.int32 and res["u"].shape == (k,) and res["score"].dtype == np.float32
    bad = np.flatnonzero((res["u"] != u[:k]) | (res["v"] != v[:k]))
    assert len(bad) == 0, (ctx, bad[:5], res["u"][bad[:5]], res["v"][bad[:5]], u[bad[:5]], v[bad[:5]])
    assert np.array_equal(tp.bits(res["score"]), tp.bits(s[:k])), ctx
    assert (res["u"][f:] == -1).all() and (res["v"][f:] == -1).all() and np.isneginf(res["score"][f:]).all()


def check(eng, S, ks, nodes=None, nbrs=None, precisions=PRECISIONS, which=0, bufs=buffers, sims=True):
    """every k of ks (prefixes of ONE reference at max(ks)), every precision, every buffer size; the stats against the schedule"""
    kmax = max(ks)
    want = tp.ref_top_pairs(S, kmax, nodes, nbrs)
    out, sim_of = {}, {}
    for k in ks:
        f = min(k, want[3])
        w = (np.concatenate([want[0][:f], np.full(k - f, -1, np.int32)]), np.concatenate([want[1][:f], np.full(k - f, -1, np.int32)]),
             np.concatenate([want[2][:f], np.full(k - f, -np.inf, np.float32)]), f)
        for precision in precisions:
            for buf in bufs(k):
                res = eng.top_pairs(k, nodes=nodes, which=which, precision=precision, exclude=nbrs is not None, buffer_entries=buf)
                assert_equal(res, w, k, (k, precision, buf))
                st = res["stats"]
                assert st["buffer_entries"] == (buf or tp.default_buffer(k))
                if sims and buf is not None and S.shape[0] <= 300:
                    if (k, buf) not in sim_of:
                        sim_of[(k, buf)] = tp.simulate_schedule(S, k, buf, nodes, nbrs)
                    sim = sim_of[(k, buf)]
                    assert {x: st[x] for x in sim} == sim, (k, precision, buf, st, sim)
                out[(k, precision, buf)] = res
    return out


def n_pairs(n):
    return n * (n - 1) // 2


@pytest.mark.parametrize("d", [8, 50, 128, 256, 512])
def test_integer_tables_both_precisions(ga, d):
    """every KS instance of the bf16 stream (d = 8 .. 512 -> KS = 4, 4, 8, 16, 32) and the fp32 instance; N from one pair to several
    row tiles and column tiles; k from 1 past the number of candidates; ties everywhere (scores are integers in [-d, d])"""
    for n in (2, 3, 31, 33, 129, 257, 4100):
        E = tp.int_table(n, d, 100 * d + n)
        S = tp.gram(E)
        eng = ga.Engine(E, E[::-1].copy())
        ks = sorted({1, 2, 255, 1000, min(n_pairs(n) + 7, tp.MAX_K)})   # (N = 4 100 has more candidates than the largest k)
        check(eng, S, ks if n < 4100 else ks[:-1])
        if n == 4100:
            check(eng, tp.gram(E[::-1]), [1000], which=1, bufs=lambda k: (None,))
        eng.close()


def test_all_zero_table_gives_the_first_pairs_lexicographically(ga):
    n, d = 257, 8
    E = np.zeros((n, d), dtype=np.float32)
    eng = ga.Engine(E, E)
    for k in (1, 300, 1000):
        res = eng.top_pairs(k, exclude=False, buffer_entries=k + 4096)
        uu, vv = np.triu_indices(n, 1)
        assert np.array_equal(res["u"], uu[:k]) and np.array_equal(res["v"], vv[:k]) and (tp.bits(res["score"]) == 0).all()
    check(eng, tp.gram(E), [1, 300, 1000])
    eng.close()


def test_signed_zero_scores_tie(ga):
    """every product underflows to +0 or -0 (rows of +-1e-30): all scores tie, the order is lexicographic, and the score bits are
    those Engine.rank reports for the pair"""
    n, d = 129, 8
    sign = np.where(np.arange(n) % 3 == 0, -1.0, 1.0).astype(np.float32)
    E = (sign[:, None] * np.full((n, d), 1e-30, dtype=np.float32)).astype(np.float32)
    eng = ga.Engine(E, E)
    uu, vv = np.triu_indices(n, 1)
    for precision in PRECISIONS:
        k = 500
        want = eng.rank(uu[:k].astype(np.int32), vv[:k].astype(np.int32), precision=precision, exclude=False)["score"]
        assert (want == 0).all()
        for buf in buffers(k):
            res = eng.top_pairs(k, precision=precision, exclude=False, buffer_entries=buf)
            assert res["n_found"] == k and np.array_equal(res["u"], uu[:k]) and np.array_equal(res["v"], vv[:k])
            assert np.array_equal(tp.bits(res["score"]), tp.bits(want))
    eng.close()


@pytest.mark.parametrize("n", [129, 257, 4100])
def test_programmed_peaks_on_tile_borders(ga, n):
    peaks = [(0, 1), (31, 32), (127, 128)] + ([(n - 2, n - 1)] if n > 129 else [])   # (at N = 129 the last two are one pair)
    E = tp.peaks_table(n, 50, peaks)
    eng = ga.Engine(E, E)
    out = check(eng, tp.gram(E), [4, 300])
    for key, res in out.items():
        assert list(zip(res["u"].tolist(), res["v"].tolist()))[:len(peaks)] == peaks, key
        assert res["score"][:len(peaks)].tolist() == [256.0, 225.0, 196.0, 169.0][:len(peaks)]
    eng.close()


def test_the_diagonal_and_the_lower_triangle_are_never_returned(ga):
    """u . u is the largest score of every row, and every (v, u) with v < u ties the (u, v) that is returned"""
    n, d = 257, 128
    E = np.zeros((n, d), dtype=np.float32)
    E[:, 0] = 1.0
    E[np.arange(n), 1 + np.arange(n) % (d - 1)] = 3.0     # u . u = 10; u . v = 10 where the coordinates agree, else 1
    eng = ga.Engine(E, E)
    out = check(eng, tp.gram(E), [1, 255, n_pairs(n) + 7])
    for res in out.values():
        f = res["n_found"]
        assert (res["u"][:f] < res["v"][:f]).all()
    res = out[(n_pairs(n) + 7, "fp32", None)]
    assert res["n_found"] == n_pairs(n) and len(set(zip(res["u"][:-7].tolist(), res["v"][:-7].tolist()))) == n_pairs(n)
    eng.close()


def test_exclude_drops_training_edges_and_the_next_pairs_appear(ga):
    n, d, k = 257, 50, 300
    E = tp.int_table(n, d, 11)
    S = tp.gram(E)
    eng = ga.Engine(E, E)
    best = tp.ref_top_pairs(S, 40)
    edges = np.stack([best[0][:40:2], best[1][:40:2]], axis=1)                       # every other one of the 40 best pairs
    edges = np.concatenate([edges, edges[:5], [[7, 7], [7, 7], [256, 256]], edges[:3, ::-1]])  # duplicates, self-loops, both directions
    with pytest.raises(ga._lib.GraphGANHipError, match="gg_top_pairs: exclude = 1 needs the training graph"):
        eng.top_pairs(k)
    eng.set_graph_csr(*ga.edges_to_csr(n, edges))
    nbrs = tp.nbr_sets(n, edges)
    out = check(eng, S, [1, k], nbrs=nbrs)
    res = out[(k, "fp32", None)]
    got = set(zip(res["u"].tolist(), res["v"].tolist()))
    assert not got & {(min(a, b), max(a, b)) for a, b in edges.tolist()}
    assert {(int(a), int(b)) for a, b in zip(best[0][1:40:2], best[1][1:40:2])} <= got
    check(eng, S, [k], nbrs=None, bufs=lambda k: (None,))                             # exclude = False ignores the graph
    # a second graph replaces the first
    edges2 = np.stack([best[0][1:40:2], best[1][1:40:2]], axis=1)
    eng.set_graph_csr(*ga.edges_to_csr(n, edges2))
    out2 = check(eng, S, [k], nbrs=tp.nbr_sets(n, edges2), bufs=lambda k: (None,))
    got2 = set(zip(out2[(k, "fp32", None)]["u"].tolist(), out2[(k, "fp32", None)]["v"].tolist()))
    assert {(int(a), int(b)) for a, b in edges[:20].tolist()} <= got2
    eng.close()


def test_node_sets(ga):
    n, d = 300, 50
    E = tp.int_table(n, d, 21)
    S = tp.gram(E)
    eng = ga.Engine(E, E)
    edges = ga.synth_powerlaw(n, 3, 5, 6)
    eng.set_graph_csr(*ga.edges_to_csr(n, edges))
    nbrs = tp.nbr_sets(n, edges)
    rs = np.random.RandomState(3)
    border = np.array([0, 31, 32, n - 1], dtype=np.int32)
    some = np.unique(np.concatenate([border, rs.choice(n, 90, replace=False)])).astype(np.int32)
    # the best column of the whole table is not a member
    bu, bv, _, _ = tp.ref_top_pairs(S, 1)
    without = np.array([x for x in range(n) if x != int(bv[0])], dtype=np.int32)
    for nodes in (border, some, without):
        for nb in (None, nbrs):
            out = check(eng, S, [1, 255, 1000], nodes=nodes, nbrs=nb)
            for res in out.values():
                f = res["n_found"]
                assert np.isin(res["u"][:f], nodes).all() and np.isin(res["v"][:f], nodes).all()
    # m = 0, 1: nothing found, nothing launched; m = 2: the one pair
    for nodes in (np.zeros(0, np.int32), np.array([5], np.int32)):
        res = eng.top_pairs(3, nodes=nodes, exclude=False)
        assert res["n_found"] == 0 and (res["u"] == -1).all() and np.isneginf(res["score"]).all() and res["stats"]["launches"] == 0
    res = eng.top_pairs(3, nodes=[5, 290], exclude=False)
    assert res["n_found"] == 1 and (res["u"][0], res["v"][0], res["score"][0]) == (5, 290, S[5, 290])
    # every node given explicitly equals NULL
    for precision in PRECISIONS:
        a = eng.top_pairs(1000, precision=precision)
        b = eng.top_pairs(1000, nodes=np.arange(n, dtype=np.int32), precision=precision)
        assert a["n_found"] == b["n_found"] and np.array_equal(a["u"], b["u"]) and np.array_equal(a["v"], b["v"])
        assert np.array_equal(tp.bits(a["score"]), tp.bits(b["score"]))
    eng.close()


@pytest.mark.parametrize("n,d", [(129, 50), (129, 128), (4100, 50), (4100, 128)])
def test_fp32_gaussian_tables_against_the_oracle(ga, n, d):
    rs = np.random.RandomState(n + d)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    S = orc.c_all_score_rows(orc.pad_rows(E), np.zeros(n, np.float32), np.arange(n, dtype=np.int32))
    eng = ga.Engine(E, E)
    edges = ga.synth_powerlaw(n, 3, 1, 2)
    eng.set_graph_csr(*ga.edges_to_csr(n, edges))
    ks = [1, 255, 1000]
    out = check(eng, S, ks, precisions=("fp32",))
    check(eng, S, [1000], nbrs=tp.nbr_sets(n, edges), precisions=("fp32",))
    if n == 4100:   # the schedule's counts at the minimum buffer, predicted before they are asserted
        sim = tp.simulate_schedule(S, 1000, 1000 + 4096)
        assert sim["compactions"] > 1
        st = out[(1000, "fp32", 1000 + 4096)]["stats"]
        assert {x: st[x] for x in sim} == sim and st["compactions"] > 0
        again = eng.top_pairs(1000, exclude=False, buffer_entries=1000 + 4096)   # a rerun is bit-equal
        first = out[(1000, "fp32", 1000 + 4096)]
        assert all(np.array_equal(first[x].view(np.int32), again[x].view(np.int32)) for x in ("u", "v", "score"))
    eng.close()


@pytest.mark.parametrize("n,d", [(129, 50), (256, 128), (200, 300)])
def test_bf16_gaussian_tables_against_the_topk_and_rank_consumers(ga, n, d):
    rs = np.random.RandomState(7 * n + d)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    eng = ga.Engine(E, E)
    full = eng.topk(rows=None, k=n, precision="bf16", exclude=False)
    S = np.zeros((n, n), dtype=np.float32)
    S[np.arange(n)[:, None], full["col"]] = full["score"]
    out = check(eng, S, [1, 255, 1000], precisions=("bf16",))
    res = out[(1000, "bf16", None)]
    f = res["n_found"]
    rk = eng.rank(res["u"][:f], res["v"][:f], precision="bf16", exclude=False)
    assert np.array_equal(tp.bits(rk["score"]), tp.bits(res["score"][:f]))
    eng.close()


def test_ascending_table_retries_and_the_result_stays_exact(ga):
    """N = 257, k = 1: 32 896 pairs against a buffer of k + 4 096 entries; every pair of the second row tile beats the floor
    the first one left, so its rectangle overflows and is split"""
    n, k = 257, 1
    E = tp.ascending_table(n, 8)
    S = tp.gram(E)
    assert n_pairs(n) == 32896 and n_pairs(n) > k + 4096
    sim = tp.simulate_schedule(S, k, k + 4096)
    assert sim["retries"] > 0
    eng = ga.Engine(E, E)
    out = check(eng, S, [1, 255])
    for precision in PRECISIONS:
        st = out[(1, precision, k + 4096)]["stats"]
        assert st["retries"] == sim["retries"] > 0 and st["launches"] == sim["launches"]
    eng.close()


def test_larger_case_several_row_passes(ga):
    """N = 24 576 at d = 8, k = 10 000: 192 row tiles of 128-tile rectangles and the growing first ones at the minimum buffer"""
    n, d, k = 24576, 8, 10000
    E = tp.int_table(n, d, 99)
    want = tp.ref_top_pairs_small_ints(E, k)
    eng = ga.Engine(E, E)
    for precision, buf in (("fp32", k + 4096), ("bf16", None)):
        res = eng.top_pairs(k, precision=precision, exclude=False, buffer_entries=buf)
        assert_equal(res, want, k, (precision, buf))
        assert res["stats"]["launches"] > (6 if buf else 1) and res["ms"] > 0
    eng.close()


def test_every_refusal_through_engine_and_the_c_abi(ga):
    n, d = 64, 8
    E = tp.int_table(n, d, 1)
    eng = ga.Engine(E, E)
    L = ga._lib.lib
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def raw(which=0, precision=0, nodes=None, m=0, k=4, exclude=0, buf=0, null_out=False):
        u, v, s = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float32)
        nf = ctypes.c_int64()
        rc = L.gg_top_pairs(eng._ctx, which, precision, P(nodes), m, k, exclude, buf, None if null_out else P(u), P(v), P(s), ctypes.byref(nf), None, None)
        return rc, None

    def refused(text, **kw):
        rc, _ = raw(**kw)
        assert rc == ga.GG_EINVAL, (text, rc)
        with pytest.raises(ga._lib.GraphGANHipError) as ei:
            ga._lib.check(rc, eng._ctx)
        msg = str(ei.value)
        assert "gg_top_pairs: " in msg and text in msg, (text, msg)

    refused("which must be 0 (generator) or 1 (discriminator)", which=2)
    refused("precision must be 0 (fp32) or 1 (bf16)", precision=2)
    refused("exclude must be 0 or 1", exclude=2)
    refused("k = 0 outside [1, 2^20]", k=0)
    refused("k = 1048577 outside [1, 2^20]", k=(1 << 20) + 1)
    refused("buffer_entries = 4099 outside [k + 4096, 2^26] (0: the default)", buf=4099)
    refused("buffer_entries = 67108865 outside [k + 4096, 2^26] (0: the default)", buf=(1 << 26) + 1)
    refused("exclude = 1 needs the training graph (gg_set_graph_csr)", exclude=1)
    refused("nodes[1] = 64 out of range [0, 64)", nodes=np.array([1, 64, 3], np.int32), m=3)
    refused("nodes[0] = -1 out of range [0, 64)", nodes=np.array([-1], np.int32), m=1)
    refused("nodes[2] = 5 is not above nodes[1] = 5 (strictly ascending ids)", nodes=np.array([1, 5, 5], np.int32), m=3)
    refused("nodes[1] = 2 is not above nodes[0] = 9 (strictly ascending ids)", nodes=np.array([9, 2], np.int32), m=2)
    refused("bad argument", null_out=True)
    assert L.gg_top_pairs(None, 0, 0, None, 0, 1, 0, 0, None, None, None, None, None, None) == ga.GG_EINVAL
    for kw, text in ((dict(k=0), "k must be an integer in"), (dict(k=2.5), "k must be an integer in"), (dict(k=4, precision="fp16"), "precision must be"),
                     (dict(k=4, which=2), "which must be"), (dict(k=4, buffer_entries=4099), "buffer_entries must be")):
        with pytest.raises(ValueError, match=text):
            eng.top_pairs(**kw)
    with pytest.raises(ga._lib.GraphGANHipError, match=re.escape("gg_top_pairs: nodes[1] = 3 is not above nodes[0] = 3")):
        eng.top_pairs(4, nodes=[3, 3], exclude=False)
    eng.close()


def _write_edges(path, edges):
    with open(path, "w") as f:
        for a, b in edges:
            f.write("%d\t%d\n" % (a, b))


def test_results_lines_with_an_engine_equal_the_host_evaluator(ga, tmp_path):
    from graphgan_amd.evaluation import pair_prediction as pp
    n, d = 300, 50
    E = tp.int_table(n, d, 31)
    edges = ga.synth_powerlaw(n, 3, 8, 9)
    rs = np.random.RandomState(0)
    hold = rs.rand(len(edges)) < 0.2
    train, test = edges[~hold], np.concatenate([edges[hold], [[4, 4]], edges[~hold][:3], edges[hold][:2]])
    _write_edges(tmp_path / "train.txt", train.tolist())
    _write_edges(tmp_path / "test.txt", test.tolist())
    eng = ga.Engine(E, E[::-1].copy())
    eng.set_graph_csr(*ga.edges_to_csr(n, train))
    ks = (10, 100, 1000)
    # the positives by hand: distinct undirected test edges between nodes with a training edge, no training edge, no self-loop
    und = lambda ee: {(min(a, b), max(a, b)) for a, b in np.asarray(ee).tolist() if a != b}
    members = set(train.ravel().tolist())
    positives = {e for e in und(test) - und(train) if e[0] in members and e[1] in members}
    counts = " n_test=%d dropped=%d n=%d " % (len(positives), len(test) - len(positives), len(members))
    assert len(test) - len(positives) >= 6
    for which, tab in ((0, E), (1, E[::-1].copy())):
        for precision in PRECISIONS:
            kw = dict(which=which, ks=ks, precision=precision)
            dev = pp.PairPredictionEval(str(tmp_path / "train.txt"), str(tmp_path / "test.txt"), n, d, engine=eng, **kw)
            host = pp.PairPredictionEval(str(tmp_path / "train.txt"), str(tmp_path / "test.txt"), n, d, emd=tab, **kw)
            a, b = pp.format_pairs("gen", dev.eval_pair_prediction(), ks), pp.format_pairs("gen", host.eval_pair_prediction(), ks)
            assert a == b and a.startswith("gen_pairs:P@10=") and counts in a, (a, b, counts)
            a, b = pp.format_recon("dis", dev.eval_graph_reconstruction(), ks), pp.format_recon("dis", host.eval_graph_reconstruction(), ks)
            assert a == b and a.startswith("dis_recon:P@10="), (a, b)
    eng.close()


def test_ca_grqc_lines_are_printed(ga, tmp_path, capsys):
    """the shipped CA-GrQc fixture with its initial embeddings: printed, not gated"""
    from graphgan_amd.evaluation import pair_prediction as pp
    data, n, _ = load_ca_grqc()
    emb = ca_grqc_init_embeddings(data, n).astype(np.float32)
    d = emb.shape[1]
    eng = ga.Engine(emb, emb)
    train_path, test_path = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    _write_edges(train_path, data["train"].tolist())
    _write_edges(test_path, data["test"].tolist())
    eng.set_graph_csr(*ga.edges_to_csr(n, data["train"]))
    lines = []
    for which, mode in ((0, "gen"), (1, "dis")):
        ev = pp.PairPredictionEval(train_path, test_path, n, d, engine=eng, which=which)
        lines.append(pp.format_pairs(mode, ev.eval_pair_prediction()))
        lines.append(pp.format_recon(mode, ev.eval_graph_reconstruction()))
    with capsys.disabled():
        print("\nCA-GrQc, initial embeddings:\n" + "".join(lines))
    assert all(re.match(r"(gen|dis)_(pairs|recon):P@100=", x) for x in lines)
    eng.close()
