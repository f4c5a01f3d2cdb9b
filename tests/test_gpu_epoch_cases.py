"""The root-batched epoch (csrc/epoch.hip: gg_epoch_begin / gg_epoch_add / gg_epoch_commit / gg_q3_*) against the sequential C
oracle on the ladder of tests/support/epoch_cases.py: every batch plan, whole and lazy trees, the trainer's call shapes, the
rewards of the commit, a new graph between epochs, the passes over what was committed, the refusals, determinism.  Rows, pairs,
store words and tree lists are compared for EXACT equality; only the passes have a band -- step_grad_cases' own.  The premises
(the ladder's degrees, the bits in every word, the split-independence of the reference, the fill of the band) are checked without
a GPU in tests/test_epoch_cases_cpu.py."""
import ctypes

import numpy as np
import pytest

from tests.support import epoch_cases as ec
from tests.support import step_grad_cases as sg

pytestmark = pytest.mark.gpu

ALL = 1 << 30
# Lazy trees (bfs_gpu.hip, build_trees_lazy): a level is expanded while (nodes so far + its adjacency entries) fit the cap, and a
# root whose own degree + 1 exceeds it is built whole at once.  At 70 that is the hubs of raw degree 96 and 97.  A hub ROOT's walks
# end two levels below it (hub -> leaf -> pendant), which a lazy tree resolves: no hub falls back, at any cap.  A leaf or pendant
# root's exact part holds its hub's children only when the hub's adjacency fits (raw degree <= 65: 3 nodes + 65 entries).  Around
# the two large hubs the exact part ends AT the hub, a walk through it needs three more lists, and some of those slots fall back
# to whole trees: in epoch 0 of the one-hub-per-batch plan 21 slots, all of them leaves and pendants of the two large hubs, none
# around the others (at a cap of 40: 225 slots, and two batches rebuilt whole).  Later epochs and other cuts move a few.
LAZY_CAP = 70


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def c():
    return ec.case()


def make_engine(ga, c, tree_mode=None, graph=True, **kw):
    eng = ga.Engine(c.E, c.Ed, optimizer=ga.GG_OPT_SGD, **kw)
    eng.set_bias(0, c.b)
    eng.set_bias(1, c.bd)
    if tree_mode is not None:
        eng.set_tree_mode(*tree_mode)
    if graph:
        eng.set_graph_csr(c.rowptr, c.col)
    return eng


def same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (name, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got.ravel() != want.ravel())[0])
        raise AssertionError("%s: first difference at %d of %d: %r against %r" % (name, k, got.size, got.ravel()[k], want.ravel()[k]))


def run_epoch(eng, c, plan, ep, ref, trees_at=None, on_add=None):
    """One outer epoch of the plan on the engine, every return and array against ref = oracle_epochs(...)[ep]."""
    eng.epoch_begin()
    prev = (0, 0)
    for i, (batch, shift) in enumerate(zip(plan.batches, plan.shifts)):
        sd, sgen = ec.streams(ep, shift)
        got = eng.epoch_add(batch, True, True, c.n_sample, c.seed, sd, sgen)
        assert got == ref["cum"][i], "%s, epoch %d, batch %d: (rows, pairs) %r against %r" % (plan.name, ep, i, got, ref["cum"][i])
        if len(batch) == 0:
            assert got == prev
        prev = got
        if on_add:
            on_add(i, batch)
        if trees_at == i:
            off, nbr, base = eng.get_trees()
            want_off, want_nbr, want_base = ref["segments"]
            same("tree offsets after batch %d" % i, off, want_off)
            same("tree bases after batch %d" % i, base, want_base)
            same("tree lists after batch %d (mutations included)" % i, nbr, want_nbr)
            assert (want_nbr < 0).any()
    rows, pairs = ref["cum"][-1]
    assert eng.epoch_commit(1) == rows and eng.epoch_commit(0) == pairs
    cen, nb, lab = eng.get_d_data()
    n1, n2, rew = eng.get_g_data()
    tag = "%s, epoch %d: " % (plan.name, ep)
    for name, got in (("center", cen), ("neighbor", nb), ("label", lab), ("node_1", n1), ("node_2", n2)):
        same(tag + name, got, ref[name])
    word_off, words = eng.q3_get()
    same(tag + "word_off", word_off, c.word_off)
    same(tag + "Q3 words", words, ref["words"])
    return dict(center=cen, neighbor=nb, label=lab, node_1=n1, node_2=n2, reward=rew, words=words)


def trees_batch(c, plan):
    """The last batch that holds the hub of raw degree 97: its trees are compared after the add of epoch 1."""
    top = int(c.hubs[np.argmax(c.deg[c.hubs])])
    return max(i for i, b in enumerate(plan.batches) if top in b)


# ------------------------------------------------------------------------------------------------ 1. every plan, whole trees
@pytest.mark.parametrize("name", ec.PLANS)
def test_every_plan_equals_the_oracle_over_two_epochs(ga, c, name):
    plan = ec.plan(c, name)
    at = trees_batch(c, plan)
    ref = ec.oracle_epochs(c, plan, 2, segments_of=(1, at))
    eng = make_engine(ga, c)
    try:
        assert ref[0]["words"].any() and len(ref[0]["center"]) > 0 and len(ref[0]["node_1"]) > 0
        run_epoch(eng, c, plan, 0, ref[0])
        run_epoch(eng, c, plan, 1, ref[1], trees_at=at)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. lazy trees
@pytest.mark.parametrize("name", ("hubs-alone", "permuted-37-empty-batch", "three-hubs-come-back"))
def test_lazy_trees_equal_the_oracle(ga, c, name):
    plan = ec.plan(c, name)
    ref = ec.oracle_epochs(c, plan, 2)
    eng = make_engine(ga, c, tree_mode=(1, LAZY_CAP))
    whole = np.zeros(c.n, bool)     # root -> its slot held a whole tree after an add (built whole at once, fallen back, batch rebuilt)
    lazy_left = [0]                 # slots that were still lazy after their add: lazy trees carried those walks to the end

    def on_add(i, batch):
        if len(batch) == 0:
            return
        if not eng.lazy_stats()["lazy"]:                      # (a batch whose fallbacks overflowed the arena is rebuilt whole)
            whole[batch] = True
            return
        info = eng.get_lazy_trees()["info"]
        done = info[:, 0] >= info[:, 1]                       # exact nodes = nodes of the component
        whole[batch] |= done
        lazy_left[0] += int((~done).sum())

    try:
        run_epoch(eng, c, plan, 0, ref[0], on_add=on_add)
        first = whole.copy()
        run_epoch(eng, c, plan, 1, ref[1], on_add=on_add)
        st = eng.lazy_stats()
        print("lazy trees, cap %d, plan %s: %s, %d slots lazy to the end" % (LAZY_CAP, name, {k: st[k] for k in ("fallback_roots", "fallback_rounds", "resolved")}, lazy_left[0]))
        print("whole trees by hub (hub, raw degree, roots around it that had a whole tree): %s"
              % [(int(h), int(c.deg[h]), int(whole[c.info["hub_of"] == h].sum())) for h in c.hubs])
        assert st["fallback_roots"] > 0 and lazy_left[0] > c.n // 2
        assert len(np.unique(np.concatenate(plan.batches))) == c.n
        if name == "hubs-alone":    # every hub is a batch of its own: whole at once where its degree + 1 exceeds the cap, lazy otherwise
            large = [int(h) for h in c.hubs if c.deg[h] + 1 > LAZY_CAP]
            assert len(large) == 2 and [int(h) for h in c.hubs if first[h]] == large
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. the trainer's call shapes
def test_the_trainers_call_shapes(ga, c):
    plan = ec.plan(c, "descending-100")
    run = ec.OracleRun(c)
    eng = make_engine(ga, c)
    cat = lambda parts, k: np.concatenate([p[k] for p in parts])
    try:
        # (d) a commit with no add at all; passes over nothing leave the tables alone, bit for bit
        eng.epoch_begin(True, True)
        assert eng.epoch_commit(1) == 0 and eng.epoch_commit(0) == 0
        assert all(len(a) == 0 for a in eng.get_d_data() + eng.get_g_data())
        eng.d_pass([], ALL)
        eng.g_pass([], ALL)
        for which, E, b in ((0, c.E, c.b), (1, c.Ed, c.bd)):
            same("table %d after the empty passes" % which, eng.get_embeddings(which), E)
            same("bias %d after the empty passes" % which, eng.get_bias(which), b)
        # (a) D only
        eng.epoch_begin(True, False)
        rows = []
        for batch in plan.batches:
            rows.append(run.add(batch, True, False, 0, 0)["rows"])
            got = eng.epoch_add(batch, True, False, c.n_sample, c.seed, 0, 0)
            assert got == (sum(len(r[0]) for r in rows), 0)
        assert eng.epoch_commit(1) == got[0]
        for k, name in enumerate(("center", "neighbor", "label")):
            same("(a) " + name, eng.get_d_data()[k], cat(rows, k))
        same("(a) Q3 words", eng.q3_get()[1], run.words())
        # (b) both in one add; the D pass between the two commits
        eng.epoch_begin(True, True)
        rows, pairs = [], []
        for batch in plan.batches:
            a = run.add(batch, True, True, 2, 3)
            rows.append(a["rows"])
            pairs.append(a["pairs"])
            got = eng.epoch_add(batch, True, True, c.n_sample, c.seed, 2, 3)
        assert got == (sum(len(r[0]) for r in rows), sum(len(p[0]) for p in pairs))
        assert eng.epoch_commit(1) == got[0]
        for k, name in enumerate(("center", "neighbor", "label")):
            same("(b) " + name, eng.get_d_data()[k], cat(rows, k))
        eng.d_pass([0], ALL)
        assert eng.epoch_commit(0) == got[1]
        n1, n2, rew = eng.get_g_data()
        same("(b) node_1", n1, cat(pairs, 0))
        same("(b) node_2", n2, cat(pairs, 1))
        assert rew.tobytes() == eng.pair_reward(n1, n2).tobytes()             # ... under the discriminator the pass left
        assert not np.array_equal(eng.get_embeddings(1), c.Ed)
        words_b = run.words()
        same("(b) Q3 words", eng.q3_get()[1], words_b)
        # (c) G only, on another stream: the G-mode walks of the lists as the D-mode walks left them
        eng.epoch_begin(False, True)
        pairs = []
        for batch in plan.batches:
            pairs.append(run.add(batch, False, True, 0, 9)["pairs"])
            got = eng.epoch_add(batch, False, True, c.n_sample, c.seed, 0, 9)
            assert got[1] == sum(len(p[0]) for p in pairs)
        assert eng.epoch_commit(0) == got[1]
        n1, n2, _ = eng.get_g_data()
        same("(c) node_1", n1, cat(pairs, 0))
        same("(c) node_2", n2, cat(pairs, 1))
        same("(c) Q3 words: G-mode walks set none", eng.q3_get()[1], words_b)
        fresh = ec.OracleRun(c)                                               # ... and they DID read the bits
        unread = np.concatenate([fresh.add(b, False, True, 0, 9)["pairs"][0] for b in plan.batches])
        assert len(unread) != len(n1) or not np.array_equal(unread, n1)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. rewards belong to the commit
def test_rewards_are_evaluated_at_the_commit(ga, c):
    plan = ec.plan(c, "descending-100")
    ref = ec.oracle_epochs(c, plan, 1)[0]
    rs = np.random.RandomState(44)
    D2, b2 = (0.5 * rs.randn(c.n, c.d)).astype(np.float32), (0.1 * rs.randn(c.n)).astype(np.float32)
    eng = make_engine(ga, c)
    try:
        eng.epoch_begin()
        for batch in plan.batches:
            eng.epoch_add(batch, True, True, c.n_sample, c.seed, 0, 1)
        old = eng.pair_reward(ref["node_1"], ref["node_2"])
        eng.set_embeddings(1, D2)
        eng.set_bias(1, b2)
        assert eng.epoch_commit(0) == len(ref["node_1"])
        n1, n2, rew = eng.get_g_data()
        same("node_1", n1, ref["node_1"])
        same("node_2", n2, ref["node_2"])
        assert rew.tobytes() == eng.pair_reward(n1, n2).tobytes()
        assert (rew != old).mean() > 0.9
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. a new graph re-lays the store
def test_a_new_graph_relays_and_zeroes_the_store(ga, c):
    c2 = ec.case(ec.PERMUTED_LEAVES)
    assert c2.n == c.n and not np.array_equal(c2.word_off, c.word_off) and np.array_equal(c2.E, c.E)
    assert [int(c2.deg[h]) for h in c.hubs] != [int(c.deg[h]) for h in c.hubs]
    plan = ec.plan(c, "permuted-37")
    plan2 = ec.plan(c2, "permuted-37")
    eng = make_engine(ga, c)
    try:
        run_epoch(eng, c, plan, 0, ec.oracle_epochs(c, plan, 1)[0])
        eng.set_graph_csr(c2.rowptr, c2.col)
        word_off, words = eng.q3_get()
        same("word_off of the new graph", word_off, c2.word_off)
        assert len(words) == c2.word_off[-1] and not words.any()
        run = ec.OracleRun(c2)
        ref = ec.oracle_epochs(c2, plan2, 2, run=run)
        run_epoch(eng, c2, plan2, 0, ref[0])
        run_epoch(eng, c2, plan2, 1, ref[1])
        eng.q3_clear()
        word_off, words = eng.q3_get()
        same("word_off after q3_clear", word_off, c2.word_off)
        assert len(words) == c2.word_off[-1] and not words.any()
        run_epoch(eng, c2, plan2, 0, ref[0])                    # epoch 0 again: a fresh process of the reference
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. the passes consume what was committed
def test_the_passes_consume_what_was_committed(ga, c):
    """One whole-list D pass and G pass over a committed epoch against step_grad_cases' float64 SGD step, in its band.  Measured
    fill of the band (err / band, printed): 0.381 for the D pass over 2 582 rows, 0.489 for the G pass over 32 868 pairs; the
    oracle's fp32 step fills it by 0.381 / 0.490 (ec.PASS_CPU_FILL).  What would leave it by a factor of 10 or more -- a mean
    over 1 % more pairs, a pass over all batches but the last -- is shown in tests/test_epoch_cases_cpu.py."""
    plan = ec.plan(c, "permuted-37")
    ref = ec.oracle_epochs(c, plan, 1)[0]
    eng = make_engine(ga, c, lr_gen=sg.LR_SGD, lr_dis=sg.LR_SGD, lambda_gen=sg.LAMBDA, lambda_dis=sg.LAMBDA)
    try:
        eng.epoch_begin()
        for batch in plan.batches:
            eng.epoch_add(batch, True, True, c.n_sample, c.seed, 0, 1)
        assert eng.epoch_commit(1) == len(ref["center"])
        u, v, lab = eng.get_d_data()
        same("center", u, ref["center"])
        r, want_E, want_b, band_E, band_b = ec.pass_reference("d", c.Ed, c.bd, u, v, lab)
        sg.check_scores("d", r)
        eng.d_pass([0], ALL)
        Ed1, bd1 = eng.get_embeddings(1), eng.get_bias(1)
        fill_d = max(sg.ratio(Ed1, want_E, band_E), sg.ratio(bd1, want_b, band_b))
        print("D pass over %d rows: err / band %.3f" % (len(u), fill_d))
        assert fill_d <= 1.0, fill_d
        same("generator table after the D pass", eng.get_embeddings(0), c.E)
        n = eng.epoch_commit(0)
        n1, n2, rew = eng.get_g_data()
        assert n == len(n1) == len(ref["node_1"])
        same("node_1", n1, ref["node_1"])
        r, want_E, want_b, band_E, band_b = ec.pass_reference("g", c.E, c.b, n1, n2, rew)
        sg.check_scores("g", r)
        eng.g_pass([0], ALL)
        E1, b1 = eng.get_embeddings(0), eng.get_bias(0)
        fill_g = max(sg.ratio(E1, want_E, band_E), sg.ratio(b1, want_b, band_b))
        print("G pass over %d pairs: err / band %.3f" % (n, fill_g))
        assert fill_g <= 1.0, fill_g
        same("discriminator table after the G pass", eng.get_embeddings(1), Ed1)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def refused(ga, fn, text, ctx=None, rc=None):
    """fn raises (Engine) or returns GG_EINVAL (C ABI, rc given): the code and the text."""
    from graphgan_amd import _lib
    if rc is None:
        with pytest.raises(ga.GraphGANHipError) as ei:
            fn()
        assert ei.value.code == ga.GG_EINVAL and text in str(ei.value), str(ei.value)
    else:
        assert rc == ga.GG_EINVAL
        msg = _lib.lib.gg_last_error(ctx).decode()
        assert text in msg, msg


def test_refusals_leave_the_engine_and_the_accumulated_rows_usable(ga, c):
    from graphgan_amd import _lib
    lib = _lib.lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    no_graph = "epoch: call gg_set_graph_csr first"
    eng = make_engine(ga, c, graph=False)
    some = np.array([1, 2, 3], np.int32)
    n64 = ctypes.c_int64(-7)
    try:
        for fn in (eng.epoch_begin, lambda: eng.epoch_add(some), lambda: eng.epoch_commit(1), lambda: eng.epoch_commit(0), eng.q3_clear, eng.q3_get):
            refused(ga, fn, no_graph)
        ctx = eng._ctx
        refused(ga, None, no_graph, ctx, lib.gg_epoch_begin(ctx, 1, 1))
        refused(ga, None, no_graph, ctx, lib.gg_epoch_add(ctx, P(some), 3, 1, 1, 4, 0, 0, 1, None, None))
        refused(ga, None, no_graph, ctx, lib.gg_epoch_commit(ctx, 1, ctypes.byref(n64)))
        refused(ga, None, no_graph, ctx, lib.gg_q3_clear(ctx))
        refused(ga, None, no_graph, ctx, lib.gg_q3_get(ctx, None, None))
        assert n64.value == -7
        eng.set_graph_csr(c.rowptr, c.col)
        plan = ec.Plan("two-batches", [c.roots[:300], c.roots[300:520]], [0, 0])
        ref = ec.oracle_epochs(c, plan, 1)[0]
        eng.epoch_begin()
        assert eng.epoch_add(plan.batches[0], True, True, c.n_sample, c.seed, 0, 1) == ref["cum"][0]
        # ---- refused, through the C ABI and through Engine
        for roots, k in ((None, 3), (P(some), -1), (None, -1)):
            refused(ga, None, "gg_epoch_add: bad roots", ctx, lib.gg_epoch_add(ctx, roots, k, 1, 1, 4, c.seed, 0, 1, None, None))
        for bad in (c.n, -1, 1 << 30):
            roots = np.array([5, bad, 7], np.int32)
            text = "gg_build_trees_device: root %d out of range" % bad
            refused(ga, lambda: eng.epoch_add(roots, True, True, c.n_sample, c.seed, 0, 1), text)
            refused(ga, None, text, ctx, lib.gg_epoch_add(ctx, P(roots), 3, 1, 0, 4, c.seed, 0, 1, None, None))
        twice = np.array([600, 8, 9, 600], np.int32)
        text = "gg_epoch_add: root 600 appears twice in one batch"
        refused(ga, lambda: eng.epoch_add(twice, True, True, c.n_sample, c.seed, 0, 1), text)
        refused(ga, None, text, ctx, lib.gg_epoch_add(ctx, P(twice), 4, 0, 1, 4, c.seed, 0, 1, None, None))
        refused(ga, lambda: eng.epoch_commit(2), "gg_epoch_commit: which must be")
        refused(ga, None, "gg_epoch_commit: which must be", ctx, lib.gg_epoch_commit(ctx, -1, ctypes.byref(n64)))
        assert n64.value == -7
        # ---- accepted: no roots (with or without a pointer) reports the totals; the outputs may be NULL
        rows, pairs = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.gg_epoch_add(ctx, None, 0, 1, 1, 4, c.seed, 0, 1, ctypes.byref(rows), ctypes.byref(pairs)) == 0
        assert (rows.value, pairs.value) == ref["cum"][0]
        assert eng.epoch_add(some[:0], True, True, c.n_sample, c.seed, 0, 1) == ref["cum"][0]
        b1 = plan.batches[1]
        assert lib.gg_epoch_add(ctx, P(b1), len(b1), 1, 1, c.n_sample, c.seed, 0, 1, None, None) == 0
        assert lib.gg_epoch_add(ctx, None, 0, 1, 1, 4, c.seed, 0, 1, ctypes.byref(rows), None) == 0 and rows.value == ref["cum"][1][0]
        assert lib.gg_epoch_commit(ctx, 1, None) == 0
        # ---- the rows of the batch before the refusals are still there, and the engine goes on
        assert eng.epoch_commit(0) == ref["cum"][1][1]
        eng.d_rows = ref["cum"][1][0]   # (committed through the C ABI: Engine.get_d_data sizes its arrays by the count it saw)
        for k, name in enumerate(("center", "neighbor", "label")):
            same(name, eng.get_d_data()[k], ref[name])
        for k, name in enumerate(("node_1", "node_2")):
            same(name, eng.get_g_data()[k], ref[name])
        same("Q3 words", eng.q3_get()[1], ref["words"])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 8. determinism
def test_two_fresh_engines_give_the_same_bits(ga, c):
    plan = ec.plan(c, "permuted-37")
    ref = ec.oracle_epochs(c, plan, 2)
    outs = []
    for _ in range(2):
        eng = make_engine(ga, c)
        try:
            outs.append([run_epoch(eng, c, plan, ep, ref[ep]) for ep in range(2)])
        finally:
            eng.close()
    for ep in range(2):
        for key in ("center", "neighbor", "label", "node_1", "node_2", "reward", "words"):
            assert outs[0][ep][key].tobytes() == outs[1][ep][key].tobytes(), (ep, key)
        assert np.isfinite(outs[0][ep]["reward"]).all() and outs[0][ep]["reward"].min() > 0
