"""The generator's exact graph softmax on the device (gg_graph_softmax / Engine.graph_softmax) and the held-out likelihood.

Reference: the float64 DP of ``host_graph_softmax`` (checked against a brute-force enumeration of every walk and against the
sampler mirror in tests/test_graph_softmax_cpu.py) on the reference-shaped lists ``gg_get_trees`` downloads -- Q3 removals
included."""
import ctypes

import numpy as np
import pytest

from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc, load_small
from tests.support import row_dot_shapes as rd
from tests.support.graph_softmax_ref import chi2_pvalue_ok

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_ABORT, TOL_SUM, P_MIN = 1e-4, 1e-6, 1e-5, 1e-30


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def _ca_engine(ga, seed=3):
    d, n, graph = load_ca_grqc()
    emb = ca_grqc_init_embeddings(d, n).astype(np.float32)
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng = ga.Engine(emb, emb)
    eng.set_graph_csr(rowptr, col)
    bias = np.random.RandomState(seed).normal(0.0, 0.5, n).astype(np.float32)
    eng.set_bias(0, bias)
    eng.set_tree_mode(0)
    eng.build_trees(np.arange(n, dtype=np.int32), device=True)
    return eng, emb, bias, n


@pytest.fixture(scope="module")
def ca(ga):
    eng, emb, bias, n = _ca_engine(ga)
    yield eng, emb, bias, n
    eng.close()


def _check_against_dp(eng, emb, bias, slots, logp, abort, for_d):
    """-> the largest deviations (log-probability, abort mass, total mass) over the slots, for a test that reports them"""
    from graphgan_amd.evaluation.generator_likelihood import host_graph_softmax
    off, nbr, base = eng.get_trees()
    worst = np.zeros(3)
    for k, r in enumerate(slots):
        root = int(eng.tree_roots[r])
        want, a = host_graph_softmax(emb, bias, root, off[r], nbr[base[r]:base[r + 1]], for_d)
        got = logp[k].astype(np.float64)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (r, np.flatnonzero(np.isfinite(got) != np.isfinite(want))[:5])
        sel = np.isfinite(want) & (want >= np.log(P_MIN))
        dev = (np.max(np.abs(got[sel] - want[sel]), initial=0.0), abs(float(abort[k]) - a),
               abs(np.exp(got[np.isfinite(got)]).sum() + float(abort[k]) - 1.0))
        assert dev[0] <= TOL_LOGP, (r, for_d, dev[0])
        assert dev[1] <= TOL_ABORT, (r, for_d, abort[k], a)
        assert dev[2] <= TOL_SUM, (r, for_d, dev[2])
        worst = np.maximum(worst, dev)
    return worst


@pytest.mark.parametrize("for_d", [False, True])
def test_parity_on_ca_grqc_all_roots(ca, for_d):
    eng, emb, bias, n = ca
    slots = np.arange(n, dtype=np.int32)
    logp, abort = eng.graph_softmax(slots, for_d=for_d)
    assert logp.shape == (n, n) and abort.shape == (n,)
    _check_against_dp(eng, emb, bias, slots, logp, abort, for_d)
    off, _, _ = eng.get_trees()
    kids = off[slots, eng.tree_roots[slots] + 1] - off[slots, eng.tree_roots[slots]] - 1
    assert np.all(abort[kids == 0] == 1.0)  # a root without children: every walk aborts
    if not for_d:
        assert np.all(abort[kids > 0] == 0.0)  # no Q3 bits yet: every G-mode walk of a root with children ends somewhere
    else:
        assert np.any(abort[kids > 0] > 0.0)


def test_query_path_and_determinism(ca):
    eng, emb, bias, n = ca
    rng = np.random.RandomState(7)
    slots = np.arange(n, dtype=np.int32)  # 5 242 slots: two internal passes (4 096 + 1 146)
    dense, ab = eng.graph_softmax(slots)
    dense2, ab2 = eng.graph_softmax(slots)
    assert np.array_equal(dense.view(np.uint32), dense2.view(np.uint32)) and np.array_equal(ab, ab2)
    nodes = [rng.randint(0, n, size=rng.randint(0, 40)) for _ in range(n)]
    q, qa = eng.graph_softmax(slots, nodes=nodes)
    for k in range(n):
        assert np.array_equal(q[k].view(np.uint32), dense[k, nodes[k]].view(np.uint32))
    assert np.array_equal(qa, ab)
    flat = np.concatenate(nodes)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in nodes], out=off[1:])
    qf, _ = eng.graph_softmax(slots, nodes=(flat, off))
    assert np.array_equal(qf.view(np.uint32), np.concatenate(q).view(np.uint32))
    # a slot alone, in a shuffled subset, behind the pass boundary: the same bits
    for r in (0, 4095, 4096, n - 1):
        alone, a1 = eng.graph_softmax([r])
        assert np.array_equal(alone[0].view(np.uint32), dense[r].view(np.uint32)) and a1[0] == ab[r]
    sub = rng.permutation(n)[:700].astype(np.int32)
    part, pa = eng.graph_softmax(sub)
    assert np.array_equal(part.view(np.uint32), dense[sub].view(np.uint32)) and np.array_equal(pa, ab[sub])
    both = np.concatenate([np.arange(4090, 4100), [3, 3]]).astype(np.int32)
    part, _ = eng.graph_softmax(both)
    assert np.array_equal(part.view(np.uint32), dense[both].view(np.uint32))


def test_walks_around_a_call_are_unchanged(ca):
    eng, emb, bias, n = ca
    slots = np.arange(0, n, 37, dtype=np.int32)
    nw = np.full(len(slots), 20, np.int32)
    eng.set_bias(0, bias)  # (a fresh generator state: the walks' edge-score cache starts empty)
    w1 = eng.walk_sample(slots, nw, False, 99, 5)
    eng.graph_softmax(slots)
    w2 = eng.walk_sample(slots, nw, False, 99, 5)
    for key in ("samples", "paths", "path_len", "root_status"):
        assert np.array_equal(w1[key], w2[key]), key


def test_between_prepare_g_begin_and_prepare_g(ga):
    eng, emb, bias, n = _ca_engine(ga, seed=4)
    slots = np.arange(0, n, 3, dtype=np.int32)
    want = eng.prepare_g(slots, 20, 11, 3)
    eng.prepare_g_begin(slots, 20, 11, 3)
    eng.graph_softmax(slots[:50])
    got = eng.prepare_g(slots, 20, 11, 3)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    eng.close()


def _walk_hist(ga, eng, slot, for_d, n_walks, seed):
    res = eng.walk_sample([slot], [n_walks], for_d, seed, 1)
    return res["samples"], int(res["root_status"][0])


def test_sampler_law(ga, ca):
    """the end-node histogram of 2^18 walks of gg_walk_sample against exp(logp): chi^2 below its 1e-6 quantile"""
    eng, emb, bias, n = ca
    W = 1 << 18
    slots = np.arange(n, dtype=np.int32)
    logp_g, ab_g = eng.graph_softmax(slots)
    logp_d, ab_d = eng.graph_softmax(slots, for_d=True)
    rng = np.random.RandomState(5)
    deg = np.asarray(eng._rowptr[1:] - eng._rowptr[:-1])
    g_roots = [int(np.argmax(deg))] + rng.choice(np.flatnonzero((deg >= 2) & (ab_g == 0)), 3, replace=False).tolist()
    for r in g_roots:
        samples, status = _walk_hist(ga, eng, r, False, W, 1234)
        assert status == ga.GG_ROOT_OK
        assert chi2_pvalue_ok(np.bincount(samples, minlength=n), np.exp(logp_g[r].astype(np.float64)), 1e-6), r
    d_ok = np.flatnonzero((ab_d == 0) & (deg >= 2))
    d_roots = rng.choice(d_ok, 4, replace=False).tolist()
    for r in d_roots:
        samples, status = _walk_hist(ga, eng, r, True, W, 4321)
        assert status == ga.GG_ROOT_OK
        assert chi2_pvalue_ok(np.bincount(samples, minlength=n), np.exp(logp_d[r].astype(np.float64)), 1e-6), r
    # the reference aborts a whole D-mode root at its first dead end: a root with A >= 1e-4 cannot survive 2^18 walks
    aborting = rng.choice(np.flatnonzero(ab_d >= 1e-4), 8, replace=False).tolist()
    st = eng.walk_sample(aborting, [W] * len(aborting), True, 777, 2, fetch=True)["root_status"]
    assert np.all(st == ga.GG_ROOT_ABORTED), st


def test_after_prepare_d_the_removed_fathers_count(ga):
    eng, emb, bias, n = _ca_engine(ga, seed=6)
    slots = np.arange(n, dtype=np.int32)
    before, _ = eng.graph_softmax(slots)
    eng.prepare_d(slots, 21, 0, fetch=False)  # D-mode walks remove father entries of depth-1 children for good (Q3)
    off, nbr, base = eng.get_trees()
    assert (nbr == -1).sum() > 0
    logp, abort = eng.graph_softmax(slots)
    assert not np.array_equal(before, logp)
    assert np.any(abort > 0)  # a depth-1 leaf without its father entry is a dead end now
    pick = np.unique(np.concatenate([np.flatnonzero(abort > 0)[:200], np.arange(0, n, 13)])).astype(np.int32)
    _check_against_dp(eng, emb, bias, pick, logp[pick], abort[pick], False)
    eng.close()


@pytest.mark.parametrize("d", rd.GS_WIDTHS)
def test_every_row_width_instance_against_the_dp(ga, d):
    """gs_fill_kernel<1>, <2>, <4>, <8> (float4 chunks per lane of the 16-lane row dot): one chunk into the <4> and the <8> instance
    (129, 257), their last widths (256, 512), and the two narrow instances, on the 90-node golden graph with every slot; G mode on
    fresh trees, D mode after a prepare_d, so that Q3 bits exist.

    The file's own tolerances hold at every width: on the MI355X the largest deviation of a log-probability was 9.5e-7 (d = 129,
    D mode; 4.8e-7 at d = 512), of an abort mass 3.0e-8, of a total mass 4.9e-8.  So the bound derived from the tables' fp32
    score error (row_dot_shapes.logp_tolerance: 2 (max_depth + 2) e(d) = 1.9e-4 at d = 512, max_depth = 8) is not needed here:
    the kernel's score runs in float64 on the fp32 rows."""
    g, n, graph = load_small(3)
    emb, bias = rd.table(n, d)
    rowptr, col = ga.graph_to_csr(n, graph)
    eng = ga.Engine(emb, emb)
    eng.set_bias(0, bias)
    eng.set_graph_csr(rowptr, col)
    eng.set_tree_mode(0)
    slots = np.arange(n, dtype=np.int32)
    eng.build_trees(slots, device=True)
    for for_d in (False, True):
        if for_d:
            eng.prepare_d(slots, 21, 0, fetch=False)
            assert (eng.get_trees()[1] == -1).sum() > 0
        logp, abort = eng.graph_softmax(slots, for_d=for_d)
        assert logp.shape == (n, n) and np.isfinite(logp).sum() > n
        worst = _check_against_dp(eng, emb, bias, slots, logp, abort, for_d)
        print("d = %3d for_d = %d max_depth = %d: |dlogp| %.3g  |dabort| %.3g  |sum - 1| %.3g" %
              (d, for_d, eng.max_depth, worst[0], worst[1], worst[2]))
    eng.close()


def test_scale_powerlaw_with_hubs(ga):
    n, m, d = 200_000, 10, 128
    edges = ga.synth_powerlaw(n, m, 1, 2)
    rowptr, col = ga.edges_to_csr(n, edges)
    rng = np.random.RandomState(8)
    emb = (rng.normal(0, 0.12, (n, d))).astype(np.float32)
    eng = ga.Engine(emb, emb)
    eng.set_graph_csr(rowptr, col)
    bias = rng.normal(0, 0.3, n).astype(np.float32)
    eng.set_bias(0, bias)
    deg = rowptr[1:] - rowptr[:-1]
    hubs = np.argsort(-deg, kind="stable")[:8]
    roots = np.unique(np.concatenate([hubs, rng.choice(n, 56, replace=False)]))[:64].astype(np.int32)
    eng.set_tree_mode(0)
    eng.build_trees(roots, device=True)
    slots = np.arange(len(roots), dtype=np.int32)
    logp, abort = eng.graph_softmax(slots)
    assert eng.last_graph_softmax_ms > 0.0
    _check_against_dp(eng, emb, bias, slots, logp, abort, False)
    logp_d, abort_d = eng.graph_softmax(slots[:8], for_d=True)
    _check_against_dp(eng, emb, bias, slots[:8], logp_d, abort_d, True)
    eng.close()


def _raw(ga, eng, slots, q_off=None, q_node=None, flags=0):
    from graphgan_amd._lib import lib
    slots = np.ascontiguousarray(slots, np.int32)
    ns = len(slots)
    logp = np.empty((max(ns, 1), eng.n_node), np.float32)
    ab = np.empty(max(ns, 1), np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    q = None if q_off is None else np.empty(max(int(q_off[-1]), 1), np.float32)
    rc = lib.gg_graph_softmax(eng._ctx, p(slots), ns, flags, None if q_off is not None else p(logp), p(q_off), p(q_node), p(q), p(ab), None)
    msg = lib.gg_last_error(eng._ctx)
    return rc, (msg or b"").decode()


def test_errors(ga):
    from tests.helpers import star_graph_edges
    eng, emb, bias, n = _ca_engine(ga, seed=9)
    rc, msg = _raw(ga, eng, [n])
    assert rc == ga.GG_EINVAL and "slot" in msg
    rc, msg = _raw(ga, eng, [0, 1], np.array([0, 1, 2], np.int64), np.array([3, n], np.int32))
    assert rc == ga.GG_EINVAL and "q_node" in msg
    rc, _ = _raw(ga, eng, [0, 1], np.array([0, 1, 2], np.int64), np.array([3, 4], np.int32))
    assert rc == 0
    with pytest.raises(ValueError):
        eng.graph_softmax([n])
    with pytest.raises(ValueError):
        eng.graph_softmax([0], nodes=[np.array([n])])
    # lazy resident trees
    eng.set_tree_mode(1, 64)
    eng.build_trees(np.arange(0, 64, dtype=np.int32), device=True)
    assert eng.lazy_stats()["lazy"]
    rc, msg = _raw(ga, eng, [0])
    assert rc == ga.GG_EINVAL and "gg_set_tree_mode(ctx, 0)" in msg
    eng.set_tree_mode(0)
    eng.build_trees(np.arange(0, 64, dtype=np.int32), device=True)
    assert _raw(ga, eng, [0])[0] == 0
    # a non-finite generator
    bad = emb.copy()
    bad[5, 3] = np.nan
    eng.set_embeddings(0, bad)
    rc, msg = _raw(ga, eng, [0])
    assert rc == ga.GG_EINVAL and "non-finite" in msg
    eng.close()
    # trees without edge indices: lists of one graph uploaded beside another
    e1, nn = star_graph_edges(40)
    r1, c1 = ga.edges_to_csr(nn, e1)
    off, nbr, base, md = ga.host_build_trees(nn, r1, c1, np.arange(nn, dtype=np.int32))
    e2 = e1.copy()
    e2[:, 1] = (e2[:, 1] + 1) % nn
    e2 = e2[e2[:, 0] != e2[:, 1]]
    r2, c2 = ga.edges_to_csr(nn, e2)
    z = np.random.RandomState(0).rand(nn, 8).astype(np.float32)
    eng2 = ga.Engine(z, z)
    eng2.set_graph_csr(r2, c2)
    eng2.set_trees(np.arange(nn, dtype=np.int32), off, nbr, base, md)
    assert not eng2.get_tree_order()[4]
    rc, msg = _raw(ga, eng2, [0])
    assert rc == ga.GG_EINVAL and "edges_valid" in msg
    eng2.close()


def test_gen_nll_end_to_end(tmp_path):
    """graph_gan.py on the short schedule: the gen_nll line is appended, the other lines and the embeddings do not move, the value
    matches the float64 fallback on the engine's tables and trees, and root batches give the same line bit for bit"""
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    from graphgan_amd.evaluation import generator_likelihood as gl
    from graphgan_amd.graph_gan import GraphGAN
    runs = {}
    for name, over in (("off", {}), ("on", dict(engine_gen_nll=True)), ("batches", dict(engine_gen_nll=True, engine_tree_budget_gb=1e-5, engine_batch_roots=1000))):
        base = str(tmp_path / name)
        write_reference_layout(base)
        cfg = make_cfg(base, n_epochs=1, n_epochs_dis=1, n_epochs_gen=1, engine_seed=3, **over)
        g = GraphGAN(cfg)
        assert g._all_resident == (name != "batches")
        g.train()
        lines = open(cfg.result_filename).read().splitlines()
        emb = open(cfg.emb_filenames[0]).read()
        if name == "on":
            E, b = g.engine.get_embeddings(0), g.engine.get_bias(0)
            off, nbr, base_ = g.engine.get_trees()
            host = gl.GenLikelihoodEval(cfg.test_filename, g.n_node, emb=E, bias=b, trees=(g._slot_of_root, off, nbr, base_)).eval_gen_likelihood()
            dev = g.gen_likelihood()
            assert dev["n"] == host["n"] and dev["reach"] == host["reach"]
            assert abs(dev["nll"] - host["nll"]) <= 1e-5 * abs(host["nll"])
        g.engine.close()
        runs[name] = (lines, emb)
    off_lines, on_lines, b_lines = runs["off"][0], runs["on"][0], runs["batches"][0]
    assert [x for x in on_lines if not x.startswith("gen_nll:")] == off_lines
    nll_lines = [x for x in on_lines if x.startswith("gen_nll:")]
    assert len(nll_lines) == 2  # before training and after the epoch
    assert all(x.startswith("gen_nll:NLL=") and " reach=" in x and " n=" in x for x in nll_lines)
    assert runs["on"][1] == runs["off"][1]
    assert [x for x in b_lines if x.startswith("gen_nll:")] == nll_lines
