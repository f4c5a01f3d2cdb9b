"""The premises of tests/test_gpu_epoch_cases.py, checked without a GPU on the oracle alone (tests/support/epoch_cases.py): the
ladder's hubs sit on both sides of every word edge of the Q3 store; the walks set bits in every word, and more in the second
epoch; the duplicate / self-loop hub has bits whose index is not the CSR position; roots abort and hubs do not; the stored bits
decide the next epoch's walks; the reference does not depend on the batch split; a root that comes back is walked anew; and the
band of the pass test holds the oracle's own fp32 step over a committed epoch with room to spare.  A ladder without the
duplicate hub, or with every hub below 32 children, fails here."""
import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.support import epoch_cases as ec
from tests.support import step_grad_cases as sg


@pytest.fixture(scope="module")
def c():
    return ec.case()


@pytest.fixture(scope="module")
def one(c):
    """Two epochs of the one-batch plan."""
    return ec.oracle_epochs(c, ec.plan(c, "one-batch"), 2)


def popcount(words):
    return sum(bin(int(w)).count("1") for w in words)


def children_of(c, r):
    return c.nbr0[c.base[r] + c.off[r, r] + 1: c.base[r] + c.off[r, r + 1]]


def check_ladder(c):
    """The shape of the graph (the degenerate ladders of the last test fail here)."""
    n, info = c.n, c.info
    assert c.deg[0] == 0 and c.deg[n - 1] == 0 and (c.deg[1:n - 1] > 0).all()
    assert 650 <= n <= 1100 and c.d == 8
    # raw, symmetric, duplicates kept: every entry has its mirror, as often as itself
    src = np.repeat(np.arange(n), c.deg)
    fwd = np.sort(src * n + c.col)
    assert np.array_equal(fwd, np.sort(c.col.astype(np.int64) * n + src))
    # one component plus the two isolated nodes: the tree of hub 1 holds every other node
    assert c.off[1, n] == 2 * (n - 2) - 1
    dup = info["dup_hub"]
    assert dup is not None, "no duplicate / self-loop hub"
    regular = [h for h in info["hubs"] if h != dup]
    assert sorted(c.deg[regular]) == sorted(ec.HUB_RAW_DEGREES) == [2, 31, 32, 33, 63, 64, 65, 96, 97]
    assert max(len(children_of(c, h)) for h in regular) > 32
    # the store's layout: word_off advances by ceil(raw degree / 32) at every hub
    assert np.array_equal(np.diff(c.word_off), (c.deg + 31) // 32)
    assert [int(c.word_off[h + 1] - c.word_off[h]) for h in regular] == list(ec.HUB_WORDS) == [1, 1, 1, 2, 2, 2, 3, 3, 4]
    # the duplicate hub: 32 distinct neighbours, raw degree >= 34, duplicate and self-loop FIRST in file order
    adj = c.col[c.rowptr[dup]:c.rowptr[dup + 1]]
    assert c.deg[dup] == ec.DUP_RAW_DEGREE >= 34 and len(set(adj) - {dup}) == 32
    assert adj[0] == adj[1] and adj[2] == adj[3] == dup
    kids = children_of(c, dup)
    assert len(kids) == 32 and c.word_off[dup + 1] - c.word_off[dup] == 2           # two words where the children need one
    pos = [int(np.flatnonzero(adj == k)[0]) for k in kids]
    assert sum(p != j for j, p in enumerate(pos)) >= 31                              # rank among tree children != CSR position
    # every leaf carries a private pendant node
    for h in info["hubs"]:
        for x in info["leaves_of"][h]:
            assert set(c.col[c.rowptr[x]:c.rowptr[x + 1]]) - {h} and c.deg[x] in (2, 3)


def test_ladder_has_the_degrees_and_the_store_layout(c):
    check_ladder(c)
    assert tuple(p.name for p in ec.plans(c)) == ec.PLANS


def test_bits_reach_every_word_and_grow(c, one):
    w0, w1 = one[0]["words"], one[1]["words"]
    big = [h for h in c.hubs if len(children_of(c, h)) > 32]
    assert len(big) >= 6
    for h in big:
        a, b = c.word_off[h], c.word_off[h] + (len(children_of(c, h)) + 31) // 32
        assert (w0[a:b] != 0).all(), "hub %d: a word without a bit after epoch 0: %s" % (h, w0[a:b])
        assert popcount(w1[a:b]) > popcount(w0[a:b]), "hub %d: epoch 1 set no further bit" % h
        assert (w1[a:b] & w0[a:b] == w0[a:b]).all()                                  # bits are never taken back
    top = c.hubs[np.argmax(c.deg[c.hubs])]
    bits = [j for j in range(len(children_of(c, top))) if w1[c.word_off[top] + j // 32] >> (j % 32) & 1]
    print("highest set bit on the largest hub: %d of %d children" % (max(bits), len(children_of(c, top))))
    assert max(bits) >= 96                                                           # the fourth word


def test_duplicate_hub_has_a_bit_off_its_csr_position(c, one):
    dup = c.info["dup_hub"]
    adj = c.col[c.rowptr[dup]:c.rowptr[dup + 1]]
    kids = children_of(c, dup)
    w = one[0]["words"][c.word_off[dup]:c.word_off[dup + 1]]
    assert w[1] == 0                                                                 # 32 children: the second word stays empty
    moved = [j for j in range(32) if w[0] >> j & 1 and int(np.flatnonzero(adj == kids[j])[0]) != j]
    assert len(moved) >= 8, moved
    # ... and read by CSR position the same walks would have set other bits
    by_pos = 0
    for j in range(32):
        if w[0] >> j & 1:
            by_pos |= 1 << int(np.flatnonzero(adj == kids[j])[0])
    assert by_pos != int(w[0])


def test_roots_abort_and_hubs_yield_rows(c, one):
    for ep in one:
        st = ep["batch"][0]["d"]["root_status"]
        frac = (st != 0).mean()
        print("%d of %d roots abort, %d D rows, %d G pairs" % ((st == 1).sum(), c.n, len(ep["center"]), len(ep["node_1"])))
        assert 0.1 <= frac <= 0.9
        assert (st[c.hubs] == 0).all() and set(c.hubs) <= set(ep["center"])
        assert (st[c.info["isolated"]] == 2).all()
        assert len(ep["center"]) == 2 * c.deg[st == 0].sum()


def test_stored_bits_decide_the_next_epoch(c, one):
    """Epoch 1 on trees with the bits cleared: other G-mode walks (as the CA-GrQc test shows at its end).  The D-mode samples are
    the SAME: a D-mode walk removes the root from a depth-1 child's list before scoring it, whether or not it is still there
    (module docstring of epoch_cases) -- asserted, so that nobody expects the D rows to catch a lost bit."""
    run = ec.OracleRun(c)
    p = ec.plan(c, "one-batch")
    sd, sg = ec.streams(1)
    cleared = run.add(p.batches[0], True, True, sd, sg)
    kept = one[1]["batch"][0]
    assert np.array_equal(cleared["d"]["samples"], kept["d"]["samples"]) and np.array_equal(cleared["rows"][1], kept["rows"][1])
    assert not np.array_equal(cleared["g"]["paths"], kept["g"]["paths"])
    assert len(cleared["pairs"][0]) != len(kept["pairs"][0]) or not np.array_equal(cleared["pairs"][0], kept["pairs"][0])
    # per hub: the G-mode walks of a hub root never read a bit (the root's own list is never mutated); those of its leaves do
    differs = [r for r in range(c.n) if not np.array_equal(cleared["g"]["paths"][r * c.n_sample:(r + 1) * c.n_sample],
                                                            kept["g"]["paths"][r * c.n_sample:(r + 1) * c.n_sample])]
    assert len(differs) >= 20


def test_reference_does_not_depend_on_the_split(c, one):
    base_plan = ec.plan(c, "one-batch")
    want = [ec.per_root(c, base_plan, ep) for ep in one]
    end = ec.OracleRun(c)
    ec.oracle_epochs(c, base_plan, 2, run=end)
    for p in ec.plans(c):
        visited = np.concatenate(p.batches)
        if len(np.unique(visited)) != len(visited):
            continue
        run = ec.OracleRun(c)
        ref = ec.oracle_epochs(c, p, 2, run=run)
        for ep in range(2):
            got = ec.per_root(c, p, ref[ep])
            assert sorted(got) == sorted(int(r) for r in visited)
            if len(visited) == c.n:
                assert got == want[ep], p.name
                assert np.array_equal(ref[ep]["words"], one[ep]["words"])
                assert ref[ep]["cum"][-1] == one[ep]["cum"][-1]
            elif ep == 0:
                assert all(got[r] == want[0][r] for r in got), p.name
        if len(visited) == c.n:
            assert np.array_equal(run.nbr, end.nbr), p.name
        else:   # a subset: the trees of the roots it leaves out stay pristine
            out = np.setdiff1d(c.roots, visited)
            assert all(np.array_equal(run.nbr[c.base[r]:c.base[r + 1]], c.nbr0[c.base[r]:c.base[r + 1]]) for r in out)
            assert all(np.array_equal(run.nbr[c.base[r]:c.base[r + 1]], end.nbr[c.base[r]:c.base[r + 1]]) for r in c.hubs)
    assert sum(len(np.unique(np.concatenate(p.batches))) == len(np.concatenate(p.batches)) for p in ec.plans(c)) == len(ec.PLANS) - 1


def test_plans_have_the_shapes_they_are_for(c):
    ps = {p.name: p for p in ec.plans(c)}
    size = lambda name: [len(b) for b in ps[name].batches]
    assert size("one-batch") == [c.n]
    assert size("ones-then-rest") == [1] * 40 + [c.n - 40]
    assert size("sizes-1-2-63-64-65-rest")[:5] == [1, 2, 63, 64, 65]
    assert (np.diff(np.concatenate(ps["descending-100"].batches)) == -1).all()
    assert len(ps["permuted-37"].batches) >= 20 and (np.diff(np.concatenate(ps["permuted-37"].batches)) < 0).sum() > c.n // 4
    mid = size("permuted-37-empty-batch")
    assert 0 in mid[1:-1] and sum(mid) == c.n
    alone = ps["hubs-alone"].batches
    assert [int(b[0]) for b in alone if len(b) == 1] == list(c.hubs) and all(len(b) > 1 for b in alone[0::2])
    third = np.concatenate(ps["every-third-root"].batches)
    assert set(c.hubs) <= set(third) and len(third) < c.n // 2 and len(np.unique(third)) == len(third)
    back = ps["three-hubs-come-back"]
    flat = np.concatenate(back.batches)
    rep = [r for r in np.unique(flat) if (flat == r).sum() == 2]
    assert len(rep) == 3 and set(rep) <= set(c.hubs) and c.info["dup_hub"] in rep and len(flat) == c.n + 3
    assert all(len(np.unique(b)) == len(b) for p in ps.values() for b in p.batches)   # never twice in ONE batch


def test_a_root_that_comes_back_is_walked_anew(c):
    p = ec.plan(c, "three-hubs-come-back")
    run = ec.OracleRun(c)
    ref = ec.oracle_epochs(c, p, 1, run=run)[0]
    visits = ec.per_root(c, p, ref)
    i_back = [i for i, s in enumerate(p.shifts) if s][0]
    for r in p.batches[i_back]:
        first, second = visits[int(r)]
        assert first[0] == second[0] == 0
        assert first[1] != second[1] and first[3] != second[3]                       # other D samples, other G paths
    # the second visit adds bits to those of the first, and its G-mode walks read the union: without the first visit's bits
    # (a store that lost them) the same G-mode draws give other paths
    lone = ec.OracleRun(c)
    sd, sg = ec.streams(0, ec.REPEAT_SHIFT)
    alone = lone.add(p.batches[i_back], True, True, sd, sg)
    assert np.array_equal(alone["d"]["samples"], ref["batch"][i_back]["d"]["samples"])
    once = ec.oracle_epochs(c, ec.plan(c, "one-batch"), 1)[0]["words"]
    for r in p.batches[i_back]:
        a, b = c.word_off[r], c.word_off[r + 1]
        if c.deg[r] > 40:
            assert popcount(ref["words"][a:b]) > max(popcount(once[a:b]), popcount(lone.words()[a:b]))


# ------------------------------------------------------------------------------------------------ the passes over a committed epoch
def _fp32_step(model, E, b, u, v, x, seed):
    """One SGD step in the oracle's fp32: loss_and_grads rows, summed per table row in fp32 in a shuffled order."""
    from tests.test_step_grad_cases_cpu import _shuffled_sum32
    m = (orc.Discriminator if model == "d" else orc.Generator)(E, sg.LR_SGD)
    m.b[:] = b
    u64, v64 = u.astype(np.int64), v.astype(np.int64)
    _, gu, gv, gb = m.loss_and_grads(u64, v64, x, sg.LAMBDA)
    G = _shuffled_sum32(len(E), np.concatenate([u64, v64]), np.concatenate([gu, gv]), seed)
    Gb = _shuffled_sum32(len(E), v64, gb, seed + 1)
    return E - np.float32(sg.LR_SGD) * G, b - np.float32(sg.LR_SGD) * Gb


pass_reference = ec.pass_reference


def test_pass_band_holds_the_oracles_fp32_step_over_a_committed_epoch(c):
    ep = ec.oracle_epochs(c, ec.plan(c, "permuted-37"), 1)[0]
    u, v, lab = ep["center"], ep["neighbor"], ep["label"]
    ref, want_E, want_b, band_E, band_b = pass_reference("d", c.Ed, c.bd, u, v, lab)
    sg.check_scores("d", ref)
    Ed1, bd1 = _fp32_step("d", c.Ed, c.bd, u, v, lab, 5)
    fill_d = max(sg.ratio(Ed1, want_E, band_E), sg.ratio(bd1, want_b, band_b))
    assert np.abs(want_E - c.Ed).max() > 1e-3
    dis = orc.Discriminator(Ed1, sg.LR_SGD)
    dis.b[:] = bd1
    n1, n2 = ep["node_1"], ep["node_2"]
    rew = dis.reward(n1.astype(np.int64), n2.astype(np.int64))
    ref, want_E, want_b, band_E, band_b = pass_reference("g", c.E, c.b, n1, n2, rew)
    sg.check_scores("g", ref)
    E1, b1 = _fp32_step("g", c.E, c.b, n1, n2, rew, 7)
    fill_g = max(sg.ratio(E1, want_E, band_E), sg.ratio(b1, want_b, band_b))
    assert np.abs(want_E - c.E).max() > 1e-3
    print("D pass over %d rows: fp32 reference err/band %.3f; G pass over %d pairs: %.3f; recorded %.3f" % (len(u), fill_d, len(n1), fill_g, ec.PASS_CPU_FILL))
    assert max(fill_d, fill_g) <= ec.PASS_CPU_FILL <= 0.5
    # the band would notice a wrong pair count in the generator's mean: one pair more in the denominator of a short list is out
    # of reach of ANY fp32 band over 3e4 pairs, so the test asserts what the existing 2e-5 bound could not see: a 1 % error
    bad = sg.grad_reference("g", c.E, c.b, n1, n2, rew, sg.LAMBDA, mut=dict(n_mean=len(n1) * 1.01), sums_only=True)
    bad_E, bad_b, _, _ = sg.opt_step("sgd", c.E, c.b, bad["G"], bad["Gb"], band_E * 0, band_b * 0, None, sg.OptState(c.E.shape), sg.LR_SGD)
    f = max(sg.ratio(bad_E, want_E, band_E), sg.ratio(bad_b, want_b, band_b))
    print("the mean's denominator 1 %% too large leaves the band by %.3g" % f)
    assert f >= 10.0
    # ... and a pass over the pairs of all batches but the last (an accumulator that lost a batch)
    k = ep["cum"][-2][1]
    short = sg.grad_reference("g", c.E, c.b, n1[:k], n2[:k], rew[:k], sg.LAMBDA, sums_only=True)
    bad_E, bad_b, _, _ = sg.opt_step("sgd", c.E, c.b, short["G"], short["Gb"], band_E * 0, band_b * 0, None, sg.OptState(c.E.shape), sg.LR_SGD)
    assert max(sg.ratio(bad_E, want_E, band_E), sg.ratio(bad_b, want_b, band_b)) >= 10.0


# ------------------------------------------------------------------------------------------------ degenerate ladders fail
def test_degenerate_ladders_fail_the_checks():
    with pytest.raises(AssertionError):
        check_ladder(ec.Case(ec.LEAVES, dup_hub=False))
    with pytest.raises(AssertionError):
        check_ladder(ec.Case(tuple(min(k, 28) for k in ec.LEAVES), dup_hub=True))
