"""Skip-gram pre-training rows on the device (gg_pretrain_set_noise / gg_prepare_pretrain, graphgan_amd/pretrain.py).

The sampling contract P1-P5 is exact integer arithmetic: paths, path lengths and all three row arrays are compared BIT FOR
BIT with the numpy oracle of tests/support/pretrain_ref.py (independent code, checked on the host in test_pretrain_cpu.py).
Float results (one optimizer step, a whole pre-training epoch) are compared with the numpy discriminator of the oracle."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.helpers import GOLD, load_ca_grqc, load_small, star_graph_edges
from tests.support import pretrain_ref as ref
from tests.support.graph_softmax_ref import chi2_pvalue_ok

pytestmark = pytest.mark.gpu


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


def _compare(eng, rowptr, col, n, starts, wps, walk_len, window, n_neg, seed, stream, weights):
    rows, paths, plen = eng.prepare_pretrain(starts, wps, walk_len, window, n_neg, seed, stream, fetch=True)
    want = ref.rows(rowptr, col, n, starts, wps, walk_len, window, n_neg, seed, stream, weights=weights)
    assert np.array_equal(plen, want["path_len"])
    assert np.array_equal(paths, want["paths"])
    assert rows == want["row_off"][-1] == len(want["center"])
    c, x, lab = eng.get_d_data()
    assert np.array_equal(c, want["center"])
    assert np.array_equal(x, want["neighbor"])
    assert np.array_equal(lab, want["label"])
    return want


SHAPES = [(1, 1, 5), (2, 1, 0), (2, 5, 1), (40, 1, 1), (40, 2, 5), (40, 5, 5), (40, 5, 0), (7, 2, 1)]  # (walk_len, window, n_neg)


@pytest.mark.parametrize("gi", [0, 1, 2, 3])
def test_bit_exact_on_the_small_graphs(ga, gi):
    _, n, graph = load_small(gi)
    rowptr, col = orc.graph_to_csr(n, graph)
    eng, _ = _engine(ga, n, rowptr, col)
    w = _weights(rowptr)
    starts = np.arange(n, dtype=np.int32)
    try:
        for k, (walk_len, window, n_neg) in enumerate(SHAPES):
            for weights in (None, w):
                eng.pretrain_set_noise(weights)
                _compare(eng, rowptr, col, n, starts, 3, walk_len, window, n_neg, 11 + gi, k, weights)
    finally:
        eng.close()


def test_bit_exact_on_ca_grqc_all_nodes(ga):
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng, _ = _engine(ga, n, rowptr, col)
    w = _weights(rowptr)
    starts = np.arange(n, dtype=np.int32)
    try:
        eng.pretrain_set_noise(w)
        _compare(eng, rowptr, col, n, starts, 4, 10, 2, 3, 1, 0x50000000, w)
        _compare(eng, rowptr, col, n, starts, 2, 40, 5, 5, 2, 7, w)
        eng.pretrain_set_noise(None)
        _compare(eng, rowptr, col, n, starts, 2, 40, 5, 1, 0xFEDCBA9876543210, 0xFFFFFFFF, None)
    finally:
        eng.close()


def test_bit_exact_on_a_hub_isolated_starts_and_four_nodes(ga):
    edges, n = star_graph_edges(3000)
    rowptr, col = ga.edges_to_csr(n + 3, edges)  # three isolated nodes behind the star
    n += 3
    eng, _ = _engine(ga, n, rowptr, col)
    w = _weights(rowptr)
    w[5::2] = 0  # zero-weight nodes are drawn through the collision rule only
    try:
        for weights in (None, w):
            eng.pretrain_set_noise(weights)
            starts = np.concatenate([[0, n - 1, 0, n - 2], np.arange(1, n, 13)]).astype(np.int32)
            want = _compare(eng, rowptr, col, n, starts, 5, 40, 5, 5, 3, 1, weights)
            assert want["path_len"][5:10].tolist() == [1] * 5 and want["row_off"][10] == want["row_off"][5]
            only_isolated = np.array([n - 1, n - 2, n - 3], dtype=np.int32)
            rows, paths, plen = eng.prepare_pretrain(only_isolated, 2, 40, 5, 5, 3, 1, fetch=True)
            assert rows == 0 and plen.tolist() == [1] * 6 and np.all(paths[:, 1:] == -1) and eng.get_d_data()[0].size == 0
            rows = eng.prepare_pretrain(np.zeros(0, np.int32), 2, 40, 5, 5, 3, 1)
            assert rows == 0
    finally:
        eng.close()
    # four nodes: almost every negative collides with the centre or the context
    rowptr4, col4 = ga.edges_to_csr(4, np.array([[0, 1], [1, 2], [2, 3], [3, 0], [0, 2]], dtype=np.int32))
    eng, _ = _engine(ga, 4, rowptr4, col4)
    try:
        for weights in (None, np.array([1, 0, 7, 2], dtype=np.uint32), np.array([0, 0, 0, 9], dtype=np.uint32)):
            eng.pretrain_set_noise(weights)
            for walk_len, window, n_neg in ((40, 5, 5), (2, 1, 1), (40, 2, 64), (256, 16, 1)):
                _compare(eng, rowptr4, col4, 4, np.array([3, 0, 1, 2, 3], dtype=np.int32), 7, walk_len, window, n_neg, 9, 4, weights)
    finally:
        eng.close()


def test_decomposition_independence(ga):
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng, _ = _engine(ga, n, rowptr, col)
    try:
        eng.pretrain_set_noise(_weights(rowptr))
        args = (3, 20, 3, 4, 21, 5)
        starts = np.arange(0, n, 3, dtype=np.int32)

        def run(s):
            rows, paths, plen = eng.prepare_pretrain(s, *args, fetch=True)
            return (paths, plen) + eng.get_d_data()

        whole = run(starts)
        again = run(starts)
        assert all(np.array_equal(a, b) for a, b in zip(whole, again))  # a repeated call: identical bits
        cut = len(starts) // 3
        first, second = run(starts[:cut]), run(starts[cut:])
        for a, b, c in zip(whole, first, second):
            assert np.array_equal(a, np.concatenate([b, c]))
        perm = np.random.RandomState(0).permutation(len(starts))
        shuffled = run(starts[perm])
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


def test_walks_graph_softmax_and_a_begun_launch_are_untouched(ga):
    _, n, graph = load_small(1)
    rowptr, col = orc.graph_to_csr(n, graph)
    eng, emb = _engine(ga, n, rowptr, col)
    try:
        roots = np.arange(n, dtype=np.int32)
        eng.set_tree_mode(0)
        eng.build_trees(roots, device=True)
        slots = np.arange(n, dtype=np.int32)
        nw = np.full(n, 6, np.int32)
        pre = lambda: eng.prepare_pretrain(roots, 3, 12, 2, 3, 5, 77)  # noqa: E731
        rows0 = pre()
        rows_ref = eng.get_d_data()
        w1 = eng.walk_sample(slots, nw, False, 13, 2)
        pre()
        w2 = eng.walk_sample(slots, nw, False, 13, 2)
        for k in w1:
            assert np.array_equal(w1[k], w2[k]), k
        s1 = eng.graph_softmax(slots)
        pre()
        s2 = eng.graph_softmax(slots)
        assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])
        g1 = eng.prepare_g(slots, 5, 13, 3)
        eng.prepare_g_begin(slots, 5, 13, 3)
        assert pre() == rows0
        got = eng.get_d_data()
        g2 = eng.prepare_g(slots, 5, 13, 3)
        for a, b in zip(g1, g2):
            assert np.array_equal(a, b)
        for a, b in zip(rows_ref, got):
            assert np.array_equal(a, b)
    finally:
        eng.close()


def test_error_codes(ga, monkeypatch):
    from graphgan_amd import _lib
    lib = _lib.lib
    _, n, graph = load_small(0)
    rowptr, col = orc.graph_to_csr(n, graph)
    emb = np.zeros((n, 4), np.float32)
    starts = np.arange(n, dtype=np.int32)
    sp = starts.ctypes.data_as(ctypes.c_void_p)

    def raw(eng, s=sp, ns=n, wps=1, walk_len=10, window=2, n_neg=3):
        rows = ctypes.c_int64(-1)
        return lib.gg_prepare_pretrain(eng._ctx, s, ns, wps, walk_len, window, n_neg, 1, 0, ctypes.byref(rows), None, None)

    eng = ga.Engine(emb, emb)
    try:
        assert raw(eng) == _lib.GG_EINVAL  # no graph
        eng.set_graph_csr(rowptr, col)
        assert raw(eng) == _lib.GG_OK
        for kw in (dict(wps=0), dict(walk_len=0), dict(walk_len=257), dict(window=0), dict(window=17), dict(n_neg=-1), dict(n_neg=65),
                   dict(ns=-1)):
            assert raw(eng, **kw) == _lib.GG_EINVAL, kw
        for bad in (-1, n):
            s = starts.copy()
            s[n // 2] = bad
            assert raw(eng, s=s.ctypes.data_as(ctypes.c_void_p)) == _lib.GG_EINVAL
        zero = np.zeros(n, np.uint32)
        assert lib.gg_pretrain_set_noise(eng._ctx, zero.ctypes.data_as(ctypes.c_void_p)) == _lib.GG_EINVAL
        with pytest.raises(ValueError):
            eng.pretrain_set_noise(zero)
        # gg_set_graph_csr drops the noise table: the rows are the uniform ones again
        eng.pretrain_set_noise(_weights(rowptr))
        eng.set_graph_csr(rowptr, col)
        eng.prepare_pretrain(starts, 2, 10, 2, 3, 4, 4)
        uniform = ref.rows(rowptr, col, n, starts, 2, 10, 2, 3, 4, 4, weights=None)
        assert np.array_equal(eng.get_d_data()[1], uniform["neighbor"])
        # between gg_epoch_begin and the matching commit
        eng.epoch_begin()
        assert raw(eng) == _lib.GG_EINVAL
        eng.epoch_add(starts[:4], do_d=True, do_g=False, seed=1)
        assert raw(eng) == _lib.GG_EINVAL
        eng.epoch_commit(1)
        assert raw(eng) == _lib.GG_OK
    finally:
        eng.close()
    # more than 2^31 - 1 rows: a ring (no dead ends), 5 000 walks of 256 nodes, window 16, 64 negatives = 5000 * 65 * 7920 rows
    m = 64
    ring = np.array([[i, (i + 1) % m] for i in range(m)], dtype=np.int32)
    rp, cl = ga.edges_to_csr(m, ring)
    eng = ga.Engine(np.zeros((m, 4), np.float32), np.zeros((m, 4), np.float32))
    try:
        eng.set_graph_csr(rp, cl)
        many = (np.arange(5000) % m).astype(np.int32)
        assert 5000 * ref.rows_of_length(256, 16, 64) > 2 ** 31 - 1
        assert raw(eng, s=many.ctypes.data_as(ctypes.c_void_p), ns=5000, walk_len=256, window=16, n_neg=64) == _lib.GG_ECAPACITY
        assert eng.prepare_pretrain(many[:100], 1, 256, 16, 64, 1, 0) == 100 * ref.rows_of_length(256, 16, 64)  # (the limits themselves are fine)
        # an attached communicator (single rank only).  One GPU here: gg_comm_init attaches a 1-rank communicator only with
        # GG_COMM_FORCE=1 (world 1 otherwise needs none and attaches nothing)
        monkeypatch.setenv("GG_COMM_FORCE", "1")
        eng.comm_init(ga.Engine.comm_unique_id(), 0, 1)
        assert raw(eng, s=many.ctypes.data_as(ctypes.c_void_p), ns=10) == _lib.GG_EINVAL
    finally:
        eng.close()


def test_one_optimizer_step_on_pretraining_rows(ga):
    """One gg_d_pass step on pre-training rows against the oracle's lazy-Adam discriminator, smoke()'s tolerances (rtol 1e-5,
    atol 1e-6).  The gated step has 256 rows.  Why not the pre-training batch of 4 096: the first Adam step moves an element by
    lr * g / (|g| + 3.2e-7), and in a 4 096-row step of these rows a few of the 10^5 touched elements have summed gradients
    that cancel to |g| ~ 1e-7, where one ulp of a sigmoid moves the update by micro-units.  The ORACLE ITSELF leaves the
    tolerance there: its fp32-sigmoid and fp64-sigmoid variants (GG_ORACLE_SIGMOID64, at most 1 ulp apart per value) differ by
    3.4e-6 max abs with 2 elements outside the tolerance at 4 096 rows and lr 5e-3, against 1.9e-9 and none at 256 rows
    (measured on the host, same rows and init).  The 4 096-row figures of the engine are printed, not gated."""
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    for batch, gated in ((256, True), (4096, False)):
        eng, emb = _engine(ga, n, rowptr, col, d=50, seed=1, lr_dis=5e-3, optimizer=ga.GG_OPT_ADAM_LAZY)
        try:
            eng.pretrain_set_noise(_weights(rowptr))
            rows = eng.prepare_pretrain(np.arange(n, dtype=np.int32), 4, 10, 2, 3, 1, 0)
            c, x, lab = eng.get_d_data()
            s = (rows // 2 // 4096) * 4096
            eng.d_pass(np.array([s], dtype=np.int64), batch)
            dis = orc.Discriminator(emb, 5e-3, lazy=True)
            dis.d_step(c[s:s + batch].astype(np.int64), x[s:s + batch].astype(np.int64), lab[s:s + batch], 1e-5)
            E, b = eng.get_embeddings(1), eng.get_bias(1)
            diff = np.abs(E - dis.E)
            print("pretrain step: batch=%d max_abs_table=%.3e outside_tolerance=%d of %d touched, max_abs_bias=%.3e"
                  % (batch, diff.max(), int((diff > 1e-6 + 1e-5 * np.abs(dis.E)).sum()), int((dis.E != emb).sum()), np.abs(b - dis.b).max()))
            if gated:
                assert np.allclose(E, dis.E, rtol=1e-5, atol=1e-6)  # smoke()'s tolerances
                assert np.allclose(b, dis.b, rtol=1e-5, atol=1e-6)
        finally:
            eng.close()


def test_end_to_end_on_ca_grqc(ga):
    """One pre-training epoch through pretrain.pretrain against the numpy discriminator on the same rows and batch starts.
    Gates: |acc_engine - acc_oracle| <= 0.005 (the project's +-0.5 % north star) and acc_oracle >= acc_init + 0.25 (a broken
    fixture).  The max-abs table distance is reported, not gated (tests/golden/pretrain_ca_grqc.json keeps the measured one)."""
    from graphgan_amd import pretrain
    d, n, graph = load_ca_grqc()
    rowptr, col = ga.edges_to_csr(n, d["train"])
    cfg = ref.e2e_config()
    table = pretrain.pretrain(cfg, n, rowptr, col)
    leg = ref.oracle_leg(d, n, rowptr, col)
    acc_engine = orc.eval_link_prediction(table.astype(np.float64), d["test"].tolist(), d["test_neg"].tolist())
    dist = float(np.max(np.abs(table - leg["table"])))
    gold = json.load(open(os.path.join(GOLD, "pretrain_ca_grqc.json")))
    print("pretrain e2e: rows=%d steps=%d acc_init=%.6f acc_oracle=%.6f acc_engine=%.6f max_abs_table_distance=%.3e (golden: %s)"
          % (leg["rows"], leg["steps"], leg["acc_init"], leg["acc_oracle"], acc_engine, dist, json.dumps(gold)))
    assert leg["rows"] == gold["rows"]
    assert leg["acc_oracle"] >= leg["acc_init"] + 0.25
    assert abs(acc_engine - leg["acc_oracle"]) <= 0.005


def test_trainer_writes_the_missing_pretrain_file(ga, tmp_path):
    from graphgan_amd import pretrain, utils
    from graphgan_amd.graph_gan import GraphGAN
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    d, n, graph = write_reference_layout(base)
    # (steps of at most 256 rows take the engine's atomic-free gradient kernel: two runs then give identical bits)
    over = dict(engine_seed=3, engine_pretrain_walks=2, engine_pretrain_len=10, engine_pretrain_window=2, engine_pretrain_neg=3,
                engine_pretrain_batch=256)
    cfg = make_cfg(base, **over)
    os.remove(cfg.pretrain_emb_filename_d)
    os.rmdir(os.path.dirname(cfg.pretrain_emb_filename_d))  # the directory is created too
    with pytest.raises(FileNotFoundError):
        GraphGAN(cfg)  # engine_pretrain defaults to False: a missing file raises as before
    assert not os.path.exists(cfg.pretrain_emb_filename_d)
    cfg = make_cfg(base, engine_pretrain=True, **over)
    g = GraphGAN(cfg)
    try:
        rowptr, col = ga.edges_to_csr(n, d["train"])
        want = pretrain.pretrain(cfg, n, rowptr, col)
        got = utils.read_embeddings(cfg.pretrain_emb_filename_d, n, cfg.n_emb)
        assert np.array_equal(got.astype(np.float32), want) and np.array_equal(got, want.astype(np.float64))
        assert np.array_equal(g.node_embed_init_d, got) and np.array_equal(g.node_embed_init_g, got)
    finally:
        if getattr(g, "engine", None) is not None:
            g.engine.close()


def test_scale_one_call_on_the_million_node_graph(ga):
    """10^6 nodes / 10^7 edges, 65 536 starts x 10 walks x 40 nodes, window 5, 5 negatives: the row count is the formula's, the
    label pattern is exact, 256 random walks and their rows equal the oracle's, and the negatives' node histogram passes a
    chi-square test against the weights at p > 1e-6 over 1 024 buckets of consecutive node ids (a collision moves a draw to
    node + 1, which leaves its bucket only at a bucket's last node: ~1e-3 of the ~1e-4 of draws that collide at all, far
    below the sampling noise of 1.2e9 draws)."""
    from graphgan_amd import _lib
    n, B = 1_000_000, 1024
    edges = ga.synth_powerlaw(n, 10, 1, 2)
    rowptr, col = ga.edges_to_csr(n, edges)
    w = _weights(rowptr)
    eng, _ = _engine(ga, n, rowptr, col, d=4)
    try:
        eng.pretrain_set_noise(w)
        starts = np.random.RandomState(5).choice(n, 65536, replace=False).astype(np.int32)
        wps, walk_len, window, n_neg, seed, stream = 10, 40, 5, 5, 8, 0x50000000
        rows, paths, plen = eng.prepare_pretrain(starts, wps, walk_len, window, n_neg, seed, stream, fetch=True)
        per_len = np.array([ref.rows_of_length(l, window, n_neg) for l in range(walk_len + 1)], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(per_len[plen])])
        assert rows == off[-1]
        buf = np.empty(rows, dtype=np.float32)
        eng._ck(_lib.lib.gg_get_d_data(eng._ctx, None, None, buf.ctypes.data_as(ctypes.c_void_p)))
        lab = buf.reshape(-1, 1 + n_neg)
        assert np.all(lab[:, 0] == 1.0) and np.all(lab[:, 1:] == 0.0)
        del lab
        nb = buf.view(np.int32)
        eng._ck(_lib.lib.gg_get_d_data(eng._ctx, None, nb.ctypes.data_as(ctypes.c_void_p), None))
        sel = np.sort(np.random.RandomState(6).choice(len(plen), 256, replace=False))
        want = ref.rows(rowptr, col, n, starts, wps, walk_len, window, n_neg, seed, stream, weights=w, select=sel)
        assert np.array_equal(plen, want["path_len"]) and np.array_equal(paths[sel], want["paths"][sel])
        assert np.array_equal(want["row_off"], off)
        for k, g in enumerate(sel):
            assert np.array_equal(nb[off[g]:off[g + 1]], want["neighbor"][want["sel_off"][k]:want["sel_off"][k + 1]]), g
        counts = np.zeros(n, dtype=np.int64)
        negs = nb.reshape(-1, 1 + n_neg)
        for a in range(0, len(negs), 1 << 24):
            counts += np.bincount(negs[a:a + (1 << 24), 1:].reshape(-1), minlength=n)
        assert counts.sum() == rows // (1 + n_neg) * n_neg
        edges_b = np.linspace(0, n, B + 1).astype(np.int64)
        got_b = np.add.reduceat(counts, edges_b[:-1])
        exp_b = np.add.reduceat(w.astype(np.float64), edges_b[:-1])
        assert chi2_pvalue_ok(got_b, exp_b, 1e-6)
        c = np.empty(rows, dtype=np.int32)  # the centres of the selected walks
        eng._ck(_lib.lib.gg_get_d_data(eng._ctx, c.ctypes.data_as(ctypes.c_void_p), None, None))
        for k, g in enumerate(sel):
            assert np.array_equal(c[off[g]:off[g + 1]], want["center"][want["sel_off"][k]:want["sel_off"][k + 1]]), g
    finally:
        eng.close()
