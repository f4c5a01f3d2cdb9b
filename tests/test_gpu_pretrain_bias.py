"""node2vec (p, q) biased walks of the skip-gram pre-training rows on the device (gg_pretrain_set_walk_bias, contract P2b).

The rule is exact integer arithmetic: paths, path lengths and all three row arrays are compared BIT FOR BIT with the numpy
oracle of tests/support/pretrain_bias_ref.py (independent code, checked on the host in test_pretrain_bias_cpu.py), the
second step's distribution against the node2vec law by chi-square, and a whole biased pre-training epoch against the numpy
discriminator on the oracle's rows."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.helpers import GOLD, load_ca_grqc, load_small, star_graph_edges
from tests.support import pretrain_bias_ref as bref
from tests.support import pretrain_ref as ref
from tests.support.graph_softmax_ref import chi2_pvalue_ok

pytestmark = pytest.mark.gpu

BIASES = [(4096, 1024, 256), (256, 1024, 4096), (1, 64, 4096), (1, 1, 4096)]


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def _engine(ga, n, rowptr, col, d=8, seed=0, **kw):
    emb = (np.random.RandomState(seed).rand(n, d).astype(np.float32) - 0.5) / d
    eng = ga.Engine(emb, emb, **kw)
    eng.set_graph_csr(rowptr, col)
    return eng, emb


def _weights(rowptr):
    from graphgan_amd import pretrain
    return pretrain.noise_weights(rowptr)


def _run(eng, starts, *args):
    rows, paths, plen = eng.prepare_pretrain(starts, *args, fetch=True)
    return (paths, plen) + tuple(eng.get_d_data())


def _compare(eng, rowptr, col, n, starts, wps, walk_len, window, n_neg, seed, stream, bias, weights, stats=None, walked=None):
    eng.pretrain_set_walk_bias(*bias)
    rows, paths, plen = eng.prepare_pretrain(starts, wps, walk_len, window, n_neg, seed, stream, fetch=True)
    want = bref.rows(rowptr, col, n, starts, wps, walk_len, window, n_neg, seed, stream, bias, weights=weights, stats=stats, walked=walked)
    assert np.array_equal(plen, want["path_len"])
    assert np.array_equal(paths, want["paths"])
    assert rows == want["row_off"][-1] == len(want["center"])
    c, x, lab = eng.get_d_data()
    assert np.array_equal(c, want["center"])
    assert np.array_equal(x, want["neighbor"])
    assert np.array_equal(lab, want["label"])
    return want


SHAPES = [(2, 1, 0), (7, 2, 1), (40, 5, 5)]  # (walk_len, window, n_neg)


@pytest.mark.parametrize("gi", [0, 1, 2, 3])
def test_bit_exact_on_the_small_graphs(ga, gi):
    _, n, graph = load_small(gi)
    rowptr, col = orc.graph_to_csr(n, graph)
    eng, _ = _engine(ga, n, rowptr, col)
    w = _weights(rowptr)
    starts = np.arange(n, dtype=np.int32)
    try:
        for k, (walk_len, window, n_neg) in enumerate(SHAPES):
            for b, bias in enumerate(BIASES):
                walked = None  # (the oracle walks once per bias and shape: the noise weights do not enter the walks)
                for weights in (None, w):
                    eng.pretrain_set_noise(weights)
                    want = _compare(eng, rowptr, col, n, starts, 3, walk_len, window, n_neg, 11 + gi, 8 * k + b, bias, weights, walked=walked)
                    walked = (want["paths"], want["path_len"])
    finally:
        eng.close()


def test_duplicate_neighbour_and_self_loop_in_a_raw_list(ga):
    """A CSR handed raw to set_graph_csr: node 0 lists 1 twice and itself, node 2 lists 2 -- and the lists are not symmetric
    (3 lists 0, 0 does not list 3).  x == prev is tested before membership (the self-loop 0 -> 0 -> 0 is a return), and
    membership is in the list of prev as stored (from 3 -> 0, the candidates of 0 are judged by the list of 3)."""
    lists = [[1, 0, 2, 1, 4], [0, 2, 5], [2, 0, 1, 3], [0, 4, 2], [3, 0, 5, 1], [1, 4, 0]]
    n = len(lists)
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.array([v for x in lists for v in x], dtype=np.int32)
    eng, _ = _engine(ga, n, rowptr, col)
    starts = np.arange(n, dtype=np.int32)
    try:
        for b, bias in enumerate(BIASES + [(4096, 1, 1)]):
            want = _compare(eng, rowptr, col, n, starts, 40, 12, 2, 2, 5, b, bias, None)
            scalar = bref.scalar_walks(rowptr, col, starts, 40, 12, 5, b, bias)
            assert np.array_equal(want["paths"], scalar[0])
    finally:
        eng.close()


def test_bit_exact_on_a_hub_where_the_exact_draw_decides(ga):
    """(4096, 1, 1) on a 3000-leaf star: from the centre a candidate other than the previous leaf is accepted with
    probability 1 / 4096, so almost every centre hop exhausts its 32 trials and the wave-cooperative draw runs on the
    3000-entry list thousands of times.  (1, 1, 4096): the same list, every candidate but the return accepted at once."""
    edges, n = star_graph_edges(3000)
    rowptr, col = ga.edges_to_csr(n + 3, edges)  # three isolated nodes behind the star
    n += 3
    eng, _ = _engine(ga, n, rowptr, col)
    w = _weights(rowptr)
    starts = np.concatenate([[0, n - 1, 0, n - 2], np.arange(1, n, 13)]).astype(np.int32)
    try:
        eng.pretrain_set_noise(w)
        st = {}
        want = _compare(eng, rowptr, col, n, starts, 5, 40, 5, 5, 3, 1, (4096, 1, 1), w, stats=st)
        assert want["path_len"][5:10].tolist() == [1] * 5
        p = want["paths"]
        centre_hops = int((p[:, 1:-1] == 0).sum())  # hops h >= 2 made from the centre (cur = path[h - 1] = 0, h - 1 >= 1)
        from_centre = int((st["fallback_from"] == 0).sum())
        print("hub: %d centre hops, %d by the exact draw; %d exact draws in all" % (centre_hops, from_centre, st["fallback_hops"]))
        assert centre_hops > 5000 and from_centre > centre_hops // 2
        st = {}
        _compare(eng, rowptr, col, n, starts, 5, 40, 5, 5, 3, 1, (1, 1, 4096), w, stats=st)
    finally:
        eng.close()


@pytest.mark.parametrize("bias", [(256, 1024, 4096), (4096, 1024, 256)])
def test_bit_exact_on_ca_grqc_all_nodes(ga, bias):
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng, _ = _engine(ga, n, rowptr, col)
    w = _weights(rowptr)
    starts = np.arange(n, dtype=np.int32)
    try:
        eng.pretrain_set_noise(w)
        _compare(eng, rowptr, col, n, starts, 2, 40, 5, 5, 2, 7, bias, w)
    finally:
        eng.close()


def test_equal_weights_and_a_graph_reload(ga):
    _, n, graph = load_small(2)
    rowptr, col = orc.graph_to_csr(n, graph)
    starts = np.arange(n, dtype=np.int32)
    args = (3, 20, 3, 4, 21, 5)
    fresh, _ = _engine(ga, n, rowptr, col)
    eng, _ = _engine(ga, n, rowptr, col)
    try:
        want = _run(fresh, starts, *args)  # an engine that never set a bias
        for bias in ((7, 7, 7), (1, 1, 1)):
            eng.pretrain_set_walk_bias(256, 1024, 4096)
            assert not np.array_equal(_run(eng, starts, *args)[0], want[0])
            eng.pretrain_set_walk_bias(*bias)
            got = _run(eng, starts, *args)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), bias
        # the bias survives set_graph_csr (the noise table does not)
        eng.pretrain_set_walk_bias(4096, 1024, 256)
        before = _run(eng, starts, *args)
        eng.set_graph_csr(rowptr, col)
        after = _run(eng, starts, *args)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        oracle = bref.rows(rowptr, col, n, starts, *args, (4096, 1024, 256))
        assert np.array_equal(after[0], oracle["paths"]) and np.array_equal(after[3], oracle["neighbor"])
        # ... and a reload with another graph of as many nodes uses the new lists (the sorted copy is rebuilt)
        shifted = {(v + 1) % n: [(x + 1) % n for x in reversed(graph[v])] for v in graph}
        rowptr2, col2 = orc.graph_to_csr(n, shifted)
        eng.set_graph_csr(rowptr2, col2)
        _compare(eng, rowptr2, col2, n, starts, *args, (4096, 1024, 256), None)
    finally:
        eng.close()
        fresh.close()


def test_decomposition_independence(ga):
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng, _ = _engine(ga, n, rowptr, col)
    try:
        eng.pretrain_set_noise(_weights(rowptr))
        eng.pretrain_set_walk_bias(4096, 1024, 256)
        args = (3, 20, 3, 4, 21, 5)
        starts = np.arange(0, n, 3, dtype=np.int32)
        whole = _run(eng, starts, *args)
        again = _run(eng, starts, *args)
        assert all(np.array_equal(a, b) for a, b in zip(whole, again))  # a repeated call: identical bits
        cut = len(starts) // 3
        first, second = _run(eng, starts[:cut], *args), _run(eng, starts[cut:], *args)
        for a, b, c in zip(whole, first, second):
            assert np.array_equal(a, np.concatenate([b, c]))
        perm = np.random.RandomState(0).permutation(len(starts))
        shuffled = _run(eng, starts[perm], *args)
        wps = args[0]
        per_walk = np.array([ref.rows_of_length(l, args[2], args[3]) for l in range(args[1] + 1)])
        off = np.concatenate([[0], np.cumsum(per_walk[whole[1]])])
        off_s = np.concatenate([[0], np.cumsum(per_walk[shuffled[1]])])
        for k in range(0, len(perm), 37):  # start k of the shuffled call = start perm[k] of the ordered one
            a, b = perm[k] * wps, k * wps
            assert np.array_equal(shuffled[0][b:b + wps], whole[0][a:a + wps])
            for arr_s, arr_w in zip(shuffled[2:], whole[2:]):
                assert np.array_equal(arr_s[off_s[b]:off_s[b + wps]], arr_w[off[a]:off[a + wps]])
    finally:
        eng.close()


@pytest.mark.parametrize("bias", [(4096, 1024, 256), (256, 1024, 4096)])
def test_second_step_follows_the_node2vec_law_on_the_device(ga, bias):
    n, rowptr, col = bref.law_graph()
    a = bref.LAW_ARGS
    eng, _ = _engine(ga, n, rowptr, col)
    try:
        eng.pretrain_set_walk_bias(*bias)
        rows, paths, plen = eng.prepare_pretrain(np.array([a["start"]], dtype=np.int32), a["n_walks"], a["walk_len"], 1, 0, a["seed"],
                                                 a["stream"], fetch=True)
    finally:
        eng.close()
    counts, other = bref.law_counts(paths)
    print("law on the device %s: conditioned walks %d, shares %s" % (bias, counts.sum(), np.round(counts / counts.sum(), 4).tolist()))
    assert other == 0 and counts.sum() > 10_000
    assert chi2_pvalue_ok(counts, bref.law_expected(bias), 1e-6)


def test_error_codes_of_the_c_abi(ga):
    from graphgan_amd import _lib
    lib = _lib.lib
    _, n, graph = load_small(0)
    rowptr, col = orc.graph_to_csr(n, graph)
    emb = np.zeros((n, 4), np.float32)
    starts = np.arange(n, dtype=np.int32)
    rows = ctypes.c_int64(-1)
    eng = ga.Engine(emb, emb)
    try:
        # the weights alone are checked: no graph needed
        assert lib.gg_pretrain_set_walk_bias(eng._ctx, 0, 1, 1) == _lib.GG_EINVAL
        assert lib.gg_pretrain_set_walk_bias(eng._ctx, 1, 1, 65537) == _lib.GG_EINVAL
        assert lib.gg_pretrain_set_walk_bias(None, 1, 1, 1) == _lib.GG_EINVAL
        assert lib.gg_pretrain_set_walk_bias(eng._ctx, 65536, 1, 2) == _lib.GG_OK
        prepare = lambda: lib.gg_prepare_pretrain(eng._ctx, starts.ctypes.data_as(ctypes.c_void_p), n, 1, 10, 2, 3, 1, 0,  # noqa: E731
                                                  ctypes.byref(rows), None, None)
        assert prepare() == _lib.GG_EINVAL  # biased, no graph
        eng.set_graph_csr(rowptr, col)
        assert prepare() == _lib.GG_OK and rows.value > 0
        eng.d_rows = rows.value  # (the raw call went past Engine.prepare_pretrain, which records the count for get_d_data)
        # a rejected setting leaves the bias as it was
        before = eng.get_d_data()[1]
        assert lib.gg_pretrain_set_walk_bias(eng._ctx, 1, 0, 1) == _lib.GG_EINVAL
        assert prepare() == _lib.GG_OK and np.array_equal(eng.get_d_data()[1], before)
        want = bref.rows(rowptr, col, n, starts, 1, 10, 2, 3, 1, 0, (65536, 1, 2))
        assert np.array_equal(before, want["neighbor"])
    finally:
        eng.close()


def test_walks_and_graph_softmax_are_untouched(ga):
    _, n, graph = load_small(1)
    rowptr, col = orc.graph_to_csr(n, graph)
    eng, emb = _engine(ga, n, rowptr, col)
    try:
        roots = np.arange(n, dtype=np.int32)
        eng.set_tree_mode(0)
        eng.build_trees(roots, device=True)
        slots = np.arange(n, dtype=np.int32)
        nw = np.full(n, 6, np.int32)
        eng.pretrain_set_walk_bias(4096, 1, 16)
        pre = lambda: eng.prepare_pretrain(roots, 3, 12, 2, 3, 5, 77)  # noqa: E731
        w1 = eng.walk_sample(slots, nw, False, 13, 2)
        rows0 = pre()
        w2 = eng.walk_sample(slots, nw, False, 13, 2)
        for k in w1:
            assert np.array_equal(w1[k], w2[k]), k
        s1 = eng.graph_softmax(slots)
        assert pre() == rows0
        s2 = eng.graph_softmax(slots)
        assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])
        # the sorted copy of the lists is shared with the top-K exclusion: both users see the same lists, whoever built it
        t1 = eng.topk(slots, k=3, which=1, exclude=True)
        pre()
        t2 = eng.topk(slots, k=3, which=1, exclude=True)
        assert np.array_equal(t1["col"], t2["col"]) and np.array_equal(t1["score"], t2["score"])
    finally:
        eng.close()


def test_end_to_end_on_ca_grqc(ga):
    """One biased pre-training epoch (p = 0.25, q = 4) through pretrain.pretrain against the numpy discriminator on the
    ORACLE's biased rows and the same batch starts.  Gate: |acc_engine - acc_oracle| <= 0.005, the gate of the uniform
    end-to-end test; the oracle leg's row count is the one recorded in tests/golden/pretrain_bias_ca_grqc.json (computed on
    the host), its accuracies are printed beside the recorded ones.  Whether biased beats uniform is not gated."""
    import types
    from graphgan_amd import pretrain
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    cfg = types.SimpleNamespace(**vars(ref.e2e_config()), engine_pretrain_p=0.25, engine_pretrain_q=4)
    gold = json.load(open(os.path.join(GOLD, "pretrain_bias_ca_grqc.json")))
    assert list(pretrain.walk_bias(0.25, 4)) == gold["bias"]
    table = pretrain.pretrain(cfg, n, rowptr, col)
    leg = bref.oracle_leg(d, n, rowptr, col, tuple(gold["bias"]))
    acc_engine = orc.eval_link_prediction(table.astype(np.float64), d["test"].tolist(), d["test_neg"].tolist())
    dist = float(np.max(np.abs(table - leg["table"])))
    print("biased pretrain e2e: rows=%d steps=%d acc_init=%.6f acc_oracle=%.6f acc_engine=%.6f max_abs_table_distance=%.3e (golden: %s)"
          % (leg["rows"], leg["steps"], leg["acc_init"], leg["acc_oracle"], acc_engine, dist, json.dumps(gold)))
    assert leg["rows"] == gold["rows"]
    assert abs(acc_engine - leg["acc_oracle"]) <= 0.005


def test_trainer_writes_the_missing_pretrain_file_with_biased_walks(ga, tmp_path):
    from graphgan_amd import pretrain, utils
    from graphgan_amd.graph_gan import GraphGAN
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    d, n, graph = write_reference_layout(base)
    # (steps of at most 256 rows take the engine's atomic-free gradient kernel: two runs then give identical bits)
    over = dict(engine_seed=3, engine_pretrain_walks=2, engine_pretrain_len=10, engine_pretrain_window=2, engine_pretrain_neg=3,
                engine_pretrain_batch=256)
    cfg = make_cfg(base, engine_pretrain=True, engine_pretrain_p=0.25, engine_pretrain_q=4, **over)
    os.remove(cfg.pretrain_emb_filename_d)
    g = GraphGAN(cfg)
    try:
        rowptr, col = ga.edges_to_csr(n, d["train"])
        want = pretrain.pretrain(cfg, n, rowptr, col)
        got = utils.read_embeddings(cfg.pretrain_emb_filename_d, n, cfg.n_emb)
        assert np.array_equal(got.astype(np.float32), want) and np.array_equal(got, want.astype(np.float64))
        assert np.array_equal(g.node_embed_init_d, got)
        uniform = pretrain.pretrain(make_cfg(base, engine_pretrain=True, **over), n, rowptr, col)
        assert not np.array_equal(uniform, want)  # the knobs reached the walks
    finally:
        if getattr(g, "engine", None) is not None:
            g.engine.close()
