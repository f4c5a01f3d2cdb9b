"""The distribution cache of the training step's two walk launches (walk_sample.hip / prepare.hip: dc_request, dc_valid,
dc_key), as a matrix: every case runs the same call sequence on
  (a) an engine with the cache on (the default),
  (b) an engine created with GG_NO_DIST_CACHE=1,
  (c) the C oracle on its own whole trees,
and asserts that (a) = (c) bit for bit (D rows, G pairs, root_status, the G-mode walks), that every array of (a) = the same
array of (b) (rewards as uint32 views: same kernel, tables and pairs), and that the cache was USED: over the G call the engine
with the cache scores strictly fewer rows for the same number of hops.  Each case also asserts the counters that prove the path
it names was reached (walk_reruns, fallback_roots, lazy).  No tolerance anywhere: integer or uint32-view equality only.

The cases, their graphs and the oracle side live in tests/support/dist_cache_cases.py; what the lazy cases presuppose about
the walks is asserted on the CPU in tests/test_dist_cache_cases_cpu.py.

The case the file exists for is "lazy_fallback_in_g": a G launch on lazy trees whose walks ask for a slot's whole tree after
the D launch of the step registered distributions under that slot's POOL ranks.  The rebuilt tree gives the same rank values
to other nodes; a rerun that still looked distributions up sampled from another node's prefix sums wherever k agreed
(profiles/r23_dist_cache_rebuild_parent.txt: the case on the library before the fix).  walk_finalize now drops the look-up
request once a rebuild has succeeded."""
import numpy as np
import pytest

from tests.support import dist_cache_cases as dc

pytestmark = pytest.mark.gpu

COUNTERS = ("rows_scored", "hops", "walk_reruns", "score_launches")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


_oracle_cache = {}


def oracle_rounds(case):
    """(c), computed once per (graph, roots, seed, n_sample, rounds): the engines never see these arrays."""
    key = (case["graph"], case["roots"].tobytes(), case["seed"], case["n_sample"], case["rounds"])
    if key not in _oracle_cache:
        _oracle_cache[key] = dc.oracle_rounds(case)
    return _oracle_cache[key]


def snapshot(eng):
    c = eng.counters()
    s = {k: int(c[k]) for k in COUNTERS}
    st = eng.lazy_stats()
    s["fallback_roots"], s["lazy"] = st["fallback_roots"], st["lazy"]
    return s


def moved(before, after):
    return {k: after[k] - before[k] for k in COUNTERS + ("fallback_roots",)}


def make_engine(ga, case, cache_on, monkeypatch):
    """Environment first (gg_create reads it), then the engine, the graph and -- for the prepare cases -- the trees."""
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    if cache_on:
        monkeypatch.delenv("GG_NO_DIST_CACHE", raising=False)
    else:
        monkeypatch.setenv("GG_NO_DIST_CACHE", "1")
    g = dc.graph_of(case)
    eng = ga.Engine(g["E"], g["E"])
    eng.set_bias(0, g["b"])
    if case["tree_mode"] is None:
        eng.set_tree_mode(0)
    else:
        eng.set_tree_mode(*case["tree_mode"])
    eng.set_graph_csr(g["rowptr"], g["col"])
    return eng


def check_lazy_build(eng, case):
    """The engine's own exact level and rank split are what the CPU side assumed -- or the case tests nothing, loudly."""
    st = eng.lazy_stats()
    assert st["lazy"] and st["fallback_roots"] == 0
    info = eng.get_lazy_trees()["info"]
    tree_roots = {t["root"] for t in dc.lazy_graph()["trees"]}
    n_lazy = 0
    for s, root in enumerate(case["roots"]):
        lzs, P, L, _seg = (int(x) for x in info[s])
        if int(root) in tree_roots:
            assert (lzs, P, L) == (dc.LZS, dc.P_EXACT, dc.L_EXACT), "slot %d: lzs %d P %d L %d" % (s, lzs, P, L)
            assert lzs < P
            n_lazy += 1
        else:
            assert lzs == P  # a component within the node limit: whole
    assert st["lazy_slots"] == n_lazy > 0


def run_prepare_case(ga, case, cache_on, monkeypatch):
    """The case's rounds of prepare_d / prepare_g over every slot: [(D arrays, G arrays, movement over D, movement over G)]."""
    eng = make_engine(ga, case, cache_on, monkeypatch)
    eng.build_trees(case["roots"], device=True)
    if case["graph"] == "lazy":
        check_lazy_build(eng, case)
    slots = np.arange(len(case["roots"]), dtype=np.int32)
    out = []
    for r in range(case["rounds"]):
        s0 = snapshot(eng)
        c, nb, lab, dst = eng.prepare_d(slots, case["seed"], 2 * r)
        s1 = snapshot(eng)
        if case.get("entry") == "begin":
            eng.prepare_g_begin(slots, case["n_sample"], case["seed"], 2 * r + 1)
        n1, n2, rew, gst = eng.prepare_g(slots, case["n_sample"], case["seed"], 2 * r + 1)
        s2 = snapshot(eng)
        w = eng.get_walks()
        out.append((dict(center=c, neighbor=nb, label=lab, root_status=dst),
                    dict(node_1=n1, node_2=n2, reward=rew, root_status=gst, samples=w["samples"], paths=w["paths"], path_len=w["path_len"]),
                    moved(s0, s1), moved(s1, s2), s2))
    eng.close()
    return out


def same_paths(got, want, what):
    """paths[:path_len] walk by walk (the engines' rows may be wider than the oracle's: a rerun lengthens the stride)."""
    assert np.array_equal(got["path_len"], want["path_len"]), what + ": path_len"
    width = int(want["path_len"].max()) if len(want["path_len"]) else 0
    m = np.arange(width)[None, :] < want["path_len"][:, None]
    a, b = got["paths"][:, :width][m], want["paths"][:, :width][m]
    if not np.array_equal(a, b):
        rows = np.flatnonzero((np.where(m, got["paths"][:, :width], -1) != np.where(m, want["paths"][:, :width], -1)).any(axis=1))
        w = int(rows[0])
        raise AssertionError("%s: paths differ in %d walks, first at walk %d: got %s, want %s" % (
            what, len(rows), w, got["paths"][w, : want["path_len"][w]].tolist(), want["paths"][w, : want["path_len"][w]].tolist()))


def same_array(got, want, what):
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    if got.shape != want.shape or not np.array_equal(got, want):
        n = min(len(got), len(want))
        bad = np.flatnonzero(got[:n] != want[:n])
        raise AssertionError("%s: lengths %d / %d, %d entries differ, first at %s" % (what, len(got), len(want), len(bad), bad[:1].tolist()))


def compare_round(tag, a, b, want):
    (ad, ag, _, _, _), (bd, bg, _, _, _), (wd, wg) = a, b, want
    # (a) against the oracle; walks first: they say WHICH walk went wrong
    same_paths(ag, wg, tag + " G walks (a) vs oracle")
    same_array(ag["samples"], wg["samples"], tag + " G samples (a) vs oracle")
    for k in ("center", "neighbor", "label", "root_status"):
        same_array(ad[k], wd[k], tag + " D %s (a) vs oracle" % k)
    for k in ("node_1", "node_2", "root_status"):
        same_array(ag[k], wg[k], tag + " G %s (a) vs oracle" % k)
    # (a) against the engine without the cache, rewards included
    for k in ("center", "neighbor", "label", "root_status"):
        same_array(ad[k], bd[k], tag + " D %s (a) vs (b)" % k)
    for k in ("node_1", "node_2", "reward", "root_status", "samples", "path_len"):
        same_array(ag[k], bg[k], tag + " G %s (a) vs (b)" % k)
    same_paths(ag, bg, tag + " G walks (a) vs (b)")


def check_cache_used(tag, a_g, b_g, strict):
    print("%s: G call rows_scored %d with the cache, %d without; hops %d / %d" % (tag, a_g["rows_scored"], b_g["rows_scored"], a_g["hops"], b_g["hops"]))
    assert a_g["hops"] == b_g["hops"] > 0, tag
    if strict:
        assert a_g["rows_scored"] < b_g["rows_scored"], tag + ": no look-up of the G launch hit"


# ------------------------------------------------------------------------------------------------ 1: whole trees
@pytest.mark.parametrize("case", dc.WHOLE_CASES, ids=[c["name"] for c in dc.WHOLE_CASES])
def test_whole_trees(ga, case, monkeypatch):
    """Level pipeline, two levels + finisher, the two-half launch; edge-score sharing off and forced; two D/G rounds: the second
    D launch refills a table the first G launch has read."""
    a = run_prepare_case(ga, case, True, monkeypatch)
    b = run_prepare_case(ga, case, False, monkeypatch)
    want = oracle_rounds(case)
    for r in range(case["rounds"]):
        tag = "%s round %d" % (case["name"], r)
        compare_round(tag, a[r], b[r], want[r])
        assert want[r][1]["hops"] > 10000
        check_cache_used(tag, a[r][3], b[r][3], case["strict"][r])
        assert a[r][2]["fallback_roots"] == 0 and a[r][3]["fallback_roots"] == 0 and not a[r][4]["lazy"]
    if case["env"].get("GG_WALK_SPLIT") == "1":
        # the G launches DID run as two halves: one score kernel per half and level, twice the unsplit engine's count
        unsplit = run_prepare_case(ga, dict(case, env=dict(case["env"], GG_WALK_SPLIT="0")), True, monkeypatch)
        for r in range(case["rounds"]):
            assert a[r][3]["score_launches"] == 2 * unsplit[r][3]["score_launches"] > 0, (case["name"], r)


# ------------------------------------------------------------------------------------------------ 2-6: lazy trees
@pytest.mark.parametrize("case", dc.LAZY_CASES, ids=[c["name"] for c in dc.LAZY_CASES])
def test_lazy_trees(ga, case, monkeypatch):
    """No rebuild at all (pool ranks agree between the launches: hits are legitimate and must occur); a rebuild in the D launch
    (its rerun registers from the rebuilt trees); a rebuild in the G launch -- the rerun must not look up what the D launch
    registered under pool ranks --, also with an arena of one tree (the whole batch is rebuilt) and through prepare_g_begin."""
    a = run_prepare_case(ga, case, True, monkeypatch)
    b = run_prepare_case(ga, case, False, monkeypatch)
    want = oracle_rounds(case)
    for r in range(case["rounds"]):
        tag = "%s round %d" % (case["name"], r)
        # the path the case names was reached, in both engines, before anything is compared
        for x in (a[r], b[r]):
            for moved_by, expect in ((x[2], case["fallback"][r][0]), (x[3], case["fallback"][r][1])):
                if expect == 0:
                    assert moved_by["fallback_roots"] == 0, tag
                else:
                    assert moved_by["fallback_roots"] > 0 and moved_by["walk_reruns"] > 0, tag
                    if case["lazy_after"]:
                        assert moved_by["fallback_roots"] == expect, tag
            assert x[4]["lazy"] == case["lazy_after"], tag
        compare_round(tag, a[r], b[r], want[r])
        check_cache_used(tag, a[r][3], b[r][3], case["strict"][r])
        assert a[r][3]["rows_scored"] <= b[r][3]["rows_scored"], tag


def run_epoch_case(ga, case, cache_on, monkeypatch):
    eng = make_engine(ga, case, cache_on, monkeypatch)
    s0 = snapshot(eng)
    eng.epoch_begin()
    eng.epoch_add(case["batches"][0], n_sample=case["n_sample"], seed=case["seed"])
    s1 = snapshot(eng)
    eng.epoch_add(case["batches"][1], n_sample=case["n_sample"], seed=case["seed"])
    s2 = snapshot(eng)
    w = eng.get_walks()  # (the last batch's G-mode walks)
    eng.epoch_commit(1)
    eng.epoch_commit(0)
    d, g = eng.get_d_data(), eng.get_g_data()
    eng.close()
    return dict(center=d[0], neighbor=d[1], label=d[2], node_1=g[0], node_2=g[1], reward=g[2], walks=w, first=moved(s0, s1), both=moved(s0, s2))


def test_lazy_fallback_in_g_epoch(ga, monkeypatch):
    """The same rebuild inside gg_epoch_add (the third place that requests a look-up launch): rows and pairs of the epoch."""
    case = dc.EPOCH_CASE
    a = run_epoch_case(ga, case, True, monkeypatch)
    b = run_epoch_case(ga, case, False, monkeypatch)
    want = [dc.oracle_rounds(dict(case, roots=roots, rounds=1), roots)[0] for roots in case["batches"]]
    for x in (a, b):
        assert x["first"]["fallback_roots"] == 2 and x["first"]["walk_reruns"] > 0
        assert x["both"]["fallback_roots"] == 2  # (the quiet tree's batch asks for nothing)
    last = dict(want[1][1])
    same_paths(a["walks"], last, "epoch: last batch's G walks (a) vs oracle")
    for k in ("center", "neighbor", "label"):
        same_array(a[k], np.concatenate([w[0][k] for w in want]), "epoch D %s (a) vs oracle" % k)
    for k in ("node_1", "node_2"):
        same_array(a[k], np.concatenate([w[1][k] for w in want]), "epoch G %s (a) vs oracle" % k)
    for k in ("center", "neighbor", "label", "node_1", "node_2", "reward"):
        same_array(a[k], b[k], "epoch %s (a) vs (b)" % k)
    check_cache_used("epoch (D and G launches of both batches)", a["both"], b["both"], True)


# ------------------------------------------------------------------------------------------------ 7: a capacity rerun that keeps its cache mode
def run_capacity_case(ga, case, cache_on, monkeypatch):
    eng = make_engine(ga, case, cache_on, monkeypatch)
    roots = dc.capacity_roots()
    eng.build_trees(roots, device=True)
    slots = np.arange(len(roots), dtype=np.int32)
    s0 = snapshot(eng)
    c, nb, lab, dst = eng.prepare_d(slots[: case["d_slots"]], case["seed"], 0)
    s1 = snapshot(eng)
    n1, n2, rew, gst = eng.prepare_g(slots, case["n_sample"], case["seed"], 1)
    s2 = snapshot(eng)
    w = eng.get_walks()
    eng.close()
    return (dict(center=c, neighbor=nb, label=lab, root_status=dst),
            dict(node_1=n1, node_2=n2, reward=rew, root_status=gst, samples=w["samples"], paths=w["paths"], path_len=w["path_len"]),
            moved(s0, s1), moved(s1, s2), s2)


def test_whole_capacity_rerun_keeps_the_cache(ga, monkeypatch):
    """A fresh engine's first D launch (8 slots) teaches the sync-free launches a small capacity; the G launch over every root
    exceeds it and is rerun in sized mode -- trees unchanged, so the rerun still looks distributions up, and is right."""
    case = dc.CAPACITY_CASE
    a = run_capacity_case(ga, case, True, monkeypatch)
    b = run_capacity_case(ga, case, False, monkeypatch)
    o = dc.Oracle(dc.whole_graph(), dc.capacity_roots())
    slots = np.arange(len(dc.capacity_roots()), dtype=np.int32)
    want = (o.prepare_d(slots[: case["d_slots"]], case["seed"], 0), o.prepare_g(slots, case["n_sample"], case["seed"], 1))
    for x in (a, b):
        assert x[3]["walk_reruns"] > 0 and x[3]["fallback_roots"] == 0 and x[2]["fallback_roots"] == 0
    compare_round("capacity rerun", a, b, want)
    check_cache_used("capacity rerun", a[3], b[3], True)
