"""The two-hop pair sweep on the device (gg_two_hop_top_pairs, Engine.two_hop_top_pairs) and the graph_pairs / graph_recon results
lines.

Everything is an integer, so every comparison is EXACT equality of u, v, score and n_found: with the restatement in sets, lists and
ints (tests/support/two_hop_pairs_ref.py), with Engine.pair_neighbors and Engine.two_hop_topk, and with the host functions of
evaluation/graph_pairs.py.  The graphs take every path of the sweep: LDS and global tables, narrow and wide lists, several scratch
passes, batches larger than a launch, overflowing buffers, compactions and skipped sources.

The degree ladder has more than 2 100 000 candidate pairs, more than the largest k (2^20): the requests relative to the number of candidates
run on the ladder restricted by ``nodes`` to its special nodes and every second pool node (the sums still range over the whole
graph), and the whole ladder is asked for 2^20 pairs once."""
import ctypes
import re

import numpy as np
import pytest

from tests.support import label_spread_ref as ls
from tests.support import two_hop_pairs_ref as pref
from tests.support import two_hop_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def engine_for(ga, n, edges=None):
    table = np.zeros((n, 4), np.float32)  # (the sweep reads no embedding)
    eng = ga.Engine(table, table)
    if edges is not None:
        eng.set_graph_csr(*ga.edges_to_csr(n, np.asarray(edges, dtype=np.int32).reshape(-1, 2)))
    return eng


def check(res, want, what=None):
    u, v, s, f = want
    assert res["u"].dtype == np.int32 and res["v"].dtype == np.int32 and res["score"].dtype == np.uint64 and res["ms"] >= 0.0
    assert res["n_found"] == f, what
    assert res["u"].tolist() == u and res["v"].tolist() == v and res["score"].tolist() == s, what


def same_bits(a, b):
    return a["n_found"] == b["n_found"] and all(np.array_equal(a[key], b[key]) for key in ("u", "v", "score"))


def against_ref(eng, N, k, nodes=None, weights=None, exclude=True, **kw):
    res = eng.two_hop_top_pairs(k, nodes=nodes, weights=weights, exclude=exclude, **kw)
    check(res, pref.top_pairs(N, k, nodes, None if weights is None else weights.tolist(), exclude), (k, exclude))
    return res


@pytest.fixture(scope="module")
def ladder(ga):
    """the degree ladder of the label-spreading tests, resident, with its neighbour sets, one weight array below 2^41 with twenty
    zeros (sums pass 2^32), the dense rows of the restatement and -- on demand, kept -- its sorted candidates: shared, never changed"""
    n, edges, info = ls.hub_graph(0)
    N = ref.neighbor_sets(n, edges)
    rs = np.random.RandomState(5)
    w = rs.randint(0, 2 ** 41, n).astype(np.uint64)
    w[rs.permutation(n)[:20]] = 0
    w[info["hub_b"]] = 2 ** 41 - 1
    eng = engine_for(ga, n, edges)
    T = np.array([pref.upper_expansion(N, u) for u in range(n)])
    cap = ga.Engine.TWO_HOP_LDS_CAP
    assert ((T > 0) & (T <= cap)).sum() >= 10 and (T > cap).sum() >= 500  # both table classes
    dense = {False: [ref.dense_row(N, u) for u in range(n)], True: [ref.dense_row(N, u, w.tolist()) for u in range(n)]}
    assert max(max(r) for r in dense[True]) > 2 ** 32
    special = sorted([int(info[k]) for k in ("hub_a", "hub_b", "isolated")] + info["probes"].tolist())
    sub = np.array(sorted(set(range(0, info["pool"], 2)) | set(special)))
    cache = {}

    def cand(weighted, exclude, nodes=None):
        key = (weighted, exclude, nodes is not None)
        if key not in cache:
            cache[key] = pref.candidates(N, nodes, w.tolist() if weighted else None, exclude, rows=dense[weighted])
        return cache[key]

    yield dict(n=n, N=N, eng=eng, w=w, T=T, cand=cand, sub=sub, edges=np.asarray(edges), **info)
    eng.close()


@pytest.mark.parametrize("exclude", (True, False))
@pytest.mark.parametrize("weighted", (False, True))
def test_the_degree_ladder_against_the_restatement(ladder, weighted, exclude):
    g = ladder
    eng, w = g["eng"], g["w"] if weighted else None
    cand = g["cand"](weighted, exclude)
    assert len(cand) > 2 ** 20
    for k in (1, 2, 255, 256, 257, 1000):
        res = eng.two_hop_top_pairs(k, weights=w, exclude=exclude)
        check(res, pref.head(cand, k), k)
        if k == 1:
            assert res["stats"]["skipped"] > 0 and res["stats"]["swept"] > 0  # the bound drops sources, and the result above is unchanged
    if weighted:
        assert cand[0][2] > 2 ** 32 and len({c[2] >> 32 for c in cand[:1000]}) > 1  # the sums pass 2^32: the high word of the floor decides
    sub = g["sub"]
    cs = g["cand"](weighted, exclude, sub)
    c = len(cs)
    assert 1000 < c < 2 ** 20 - 7
    for k in (c - 1, c, c + 7):
        check(eng.two_hop_top_pairs(k, nodes=sub, weights=w, exclude=exclude), pref.head(cs, k), k)


def test_the_whole_ladder_at_the_largest_k(ladder):
    g = ladder
    check(g["eng"].two_hop_top_pairs(2 ** 20, weights=g["w"], exclude=True), pref.head(g["cand"](True, True), 2 ** 20))


def test_ties_are_cut_by_the_pair_rule(ga):
    n = 257
    edges = ls.circulant(n, (1, 5))
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    for exclude in (True, False):
        cand = pref.candidates(N, exclude=exclude)
        assert len({c[2] for c in cand}) == 2 and cand[0][2] == 2  # two scores only: almost every cut falls inside a tie
        for k in (1, 2, 63, 64, 65, 256, 257, 1000, len(cand) - 1, len(cand), len(cand) + 1):
            check(eng.two_hop_top_pairs(k, exclude=exclude), pref.head(cand, k), k)
    eng.close()
    L = 40
    star = [(0, 1 + j) for j in range(L)]
    N = ref.neighbor_sets(L + 1, star)
    eng = engine_for(ga, L + 1, star)
    count = L * (L - 1) // 2
    cand = pref.candidates(N)
    assert len(cand) == count and {c[2] for c in cand} == {1}
    for k in (count - 1, count, count + 1):
        for exclude in (True, False):
            check(eng.two_hop_top_pairs(k, exclude=exclude), pref.head(cand, k), k)  # (centre and leaf share nobody: the edges score 0)
    eng.close()


def test_both_words_of_the_floor_decide(ga):
    """weights 7 * 2^32 + a random low word: the pairs with one common neighbour share the high word 7 and differ in the low word, the
    pairs with two have a high word of 14 or 15 -- on the ladder's weights no cut falls between two scores of one high word"""
    n, rs = 200, np.random.RandomState(9)
    edges = rs.randint(0, n, (500, 2))
    w = ((7 << 32) + rs.randint(0, 2 ** 32, n)).astype(np.uint64)
    w[rs.permutation(n)[:20]] = 0
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    for exclude in (True, False):
        cand = pref.candidates(N, None, w.tolist(), exclude)
        scores = {c[2] for c in cand}
        for k in (1, 2, 255, 256, 257, 1000, len(cand) - 1, len(cand), len(cand) + 7):
            if k <= len(cand) and k > 100:
                fs = cand[k - 1][2]
                assert any(s != fs and s >> 32 == fs >> 32 for s in scores) and any(s >> 32 != fs >> 32 for s in scores)
            check(eng.two_hop_top_pairs(k, weights=w, exclude=exclude, buffer_entries=minimum_buffer(ga, eng, k, weights=w, exclude=exclude)),
                  pref.head(cand, k), (k, exclude))  # (the smallest buffer: the floor is stored and compared again and again)
            check(eng.two_hop_top_pairs(k, weights=w, exclude=exclude), pref.head(cand, k), (k, exclude))
    eng.close()


def stars(sizes):
    """one star per size: centre, then `size` leaves; -> (n, edges, centres, first leaves): the first leaf's T' is size - 1"""
    edges, centres, firsts, nxt = [], [], [], 0
    for d in sizes:
        centres.append(nxt)
        firsts.append(nxt + 1)
        edges += [(nxt, nxt + 1 + j) for j in range(d)]
        nxt += d + 1
    return nxt, edges, centres, firsts


def test_sources_on_both_sides_of_the_lds_cap_and_across_it_after_a_new_graph(ga):
    cap = ga.Engine.TWO_HOP_LDS_CAP
    n_all = stars([cap + 1, cap + 2, cap + 3])[0] + 1
    eng = engine_for(ga, n_all)
    k = 3000  # (past the first leaf's pairs: the second leaf, one entry smaller, is in the head too)
    for shift in (0, 1, -2):  # the second and the third set_graph_csr move the sources: cap -> cap + 1 (global) -> cap - 2 (LDS), ...
        sizes = [cap + shift, cap + 1 + shift, cap + 2 + shift]
        _, edges, centres, firsts = stars(sizes)
        N = ref.neighbor_sets(n_all, edges)
        eng.set_graph_csr(*ga.edges_to_csr(n_all, np.array(edges, dtype=np.int32)))
        assert [pref.upper_expansion(N, f) for f in firsts] == [cap - 1 + shift, cap + shift, cap + 1 + shift]
        for best in range(3):  # the star whose centre weighs most leads: each first leaf heads the list once
            w = np.ones(n_all, np.uint64)
            w[centres] = [5 + (j == best) for j in range(3)]
            end = firsts[best] + sizes[best]  # (the head lies inside the heaviest star: its first two leaves with the leaves above them)
            want = [(a, b, 6) for a in range(firsts[best], firsts[best] + 2) for b in range(a + 1, end)][:k]
            check(eng.two_hop_top_pairs(k, weights=w), pref.head(want, k), (shift, best))
        want = [(a, b, 1) for a in range(firsts[0], firsts[0] + 2) for b in range(a + 1, firsts[0] + sizes[0])][:k]
        check(eng.two_hop_top_pairs(k), pref.head(want, k), shift)
    eng.close()


def planted(n, seed, pair, n_common=25, n_random=300):
    """a random graph in which `pair` shares n_common neighbours, more than any other pair"""
    rs = np.random.RandomState(seed)
    a, b = pair
    others = np.array([x for x in range(n) if x not in pair])
    W = rs.permutation(others)[:n_common]
    edges = [(a, int(x)) for x in W] + [(int(x), b) for x in W] + rs.randint(0, n, (n_random, 2)).tolist()
    return edges, W


def test_the_upper_triangle_holds_every_pair_once(ga):
    n = 130
    for pair in ((0, 1), (31, 32), (n - 2, n - 1)):
        edges, _ = planted(n, 3, pair)
        N = ref.neighbor_sets(n, edges)
        eng = engine_for(ga, n, edges)
        res = against_ref(eng, N, 50)
        assert (int(res["u"][0]), int(res["v"][0])) == pair and int(res["score"][0]) >= 25
        k_all = len(pref.candidates(N, exclude=False)) + 3
        res = against_ref(eng, N, k_all, exclude=False)
        got = list(zip(res["u"][:res["n_found"]].tolist(), res["v"][:res["n_found"]].tolist()))
        assert all(a < b for a, b in got) and len(set(got)) == len(got)
        eng.close()
    # a source whose only partners have smaller ids: node 9 fills nothing itself, its pairs arrive from 2 and 3
    edges = [(5, 9), (5, 2), (5, 3)]
    N = ref.neighbor_sets(10, edges)
    assert pref.upper_expansion(N, 9) == 0
    eng = engine_for(ga, 10, edges)
    res = against_ref(eng, N, 8)
    assert list(zip(res["u"][:3].tolist(), res["v"][:3].tolist())) == [(2, 3), (2, 9), (3, 9)] and res["n_found"] == 3
    eng.close()


def test_nodes_restrict_the_endpoints_only(ga):
    n, rs = 130, np.random.RandomState(8)
    edges, W = planted(n, 4, (40, 77))
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    k_all = n * n
    every = against_ref(eng, N, k_all)
    assert same_bits(every, eng.two_hop_top_pairs(k_all, nodes=np.arange(n)))  # every node given explicitly equals None
    edge_ids = np.array([0, 31, 32, n - 1])
    for trial in range(4):
        nodes = np.unique(np.concatenate([edge_ids, rs.permutation(n)[:30 + 20 * trial]]))
        for exclude in (True, False):
            against_ref(eng, N, 500, nodes=nodes, exclude=exclude)
            against_ref(eng, N, k_all, nodes=nodes, exclude=exclude)
    # the best pair's v is no member: the pair is gone; its common neighbours are no members and still count for (40, x)
    nodes = np.array([x for x in range(n) if x != 77 and x not in set(W.tolist()[:20])])
    res = against_ref(eng, N, 300, nodes=nodes)
    got = set(zip(res["u"].tolist(), res["v"].tolist()))
    assert (40, 77) not in got and not any(77 in p for p in got)
    only = np.array([40, 77])
    res = against_ref(eng, N, 5, nodes=only)  # no common neighbour is a member: the score is that of the whole graph
    assert res["n_found"] == 1 and int(res["score"][0]) == len(N[40] & N[77]) >= 25
    for nodes in ([], [40], [40, 77], [3, 4]):
        res = against_ref(eng, N, 4, nodes=np.array(nodes, dtype=np.int64))
        assert res["n_found"] == (1 if nodes == [40, 77] else len(N[3] & N[4]) > 0 if nodes == [3, 4] else 0)
    eng.close()


def test_exclude_drops_the_training_edges_and_nothing_else(ga):
    tri = [(0, 1), (1, 2), (0, 2)]
    N = ref.neighbor_sets(4, tri)
    eng = engine_for(ga, 4, tri)
    res = against_ref(eng, N, 5, exclude=False)
    assert res["n_found"] == 3 and res["u"][:3].tolist() == [0, 0, 1] and res["v"][:3].tolist() == [1, 2, 2] and res["score"][:3].tolist() == [1, 1, 1]
    assert against_ref(eng, N, 5, exclude=True)["n_found"] == 0
    eng.close()
    n = 130
    edges, _ = planted(n, 6, (10, 90))
    edges += [(90, 10), (10, 90)]  # the best pair is a training edge (twice, both orientations)
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    res = against_ref(eng, N, 40, exclude=False)
    assert (int(res["u"][0]), int(res["v"][0])) == (10, 90)
    res = against_ref(eng, N, 40, exclude=True)
    assert (10, 90) not in set(zip(res["u"].tolist(), res["v"].tolist()))
    eng.close()
    eng = engine_for(ga, 20, np.zeros((0, 2), np.int32))  # a graph without edges
    for exclude in (True, False):
        res = eng.two_hop_top_pairs(7, exclude=exclude)
        assert res["n_found"] == 0 and res["u"].tolist() == [-1] * 7 and res["v"].tolist() == [-1] * 7 and res["score"].tolist() == [0] * 7
    eng.close()


def minimum_buffer(ga, eng, k, **kw):
    with pytest.raises(ga.GraphGANHipError) as ei:
        eng.two_hop_top_pairs(k, buffer_entries=1, **kw)
    m = re.search(r"buffer_entries = 1 outside \[(\d+), (\d+)\] \(0: the default; the minimum is k \+ (\d+), the most entries one source can append\)", str(ei.value))
    assert m and int(m.group(1)) == k + int(m.group(3)), str(ei.value)
    return int(m.group(1))


def test_the_buffer_and_the_scratch_cap_change_no_output(ga, ladder):
    g = ladder
    eng, k = g["eng"], 1000
    for weighted in (False, True):
        w = g["w"] if weighted else None
        want = pref.head(g["cand"](weighted, True), k)
        lo = minimum_buffer(ga, eng, k, weights=w)
        assert lo == k + int(np.minimum(g["T"], g["n"] - 1 - np.arange(g["n"])).max())
        for buf in (lo, 2 * lo, None):
            res = eng.two_hop_top_pairs(k, weights=w, buffer_entries=buf)
            check(res, want, buf)
            if buf == lo:
                assert res["stats"]["compactions"] > 1 and res["stats"]["appended"] > lo  # (the last one always counts)
        # A global table of the ladder has 4096 or 8192 slots of 12 bytes, and a batch has up to 256, then 512, ... of them: under these
        # caps a batch's tables go in several passes -- a half and a third of 256 tables of 4096 slots -- and in one pass per table.
        # The pass count is no output; what is asked is that the cap changes no bit.
        slots = 2 ** np.ceil(np.log2(2 * np.minimum(g["T"], g["n"] - 1 - np.arange(g["n"]))[g["T"] > ga.Engine.TWO_HOP_LDS_CAP]))
        assert set(slots.tolist()) <= {4096.0, 8192.0} and len(slots) > 256
        for scratch in (128 * 49152, 86 * 49152, 1):
            check(eng.two_hop_top_pairs(k, weights=w, scratch_bytes=scratch), want, scratch)
    with pytest.raises(ga.GraphGANHipError) as ei:
        eng.two_hop_top_pairs(k, buffer_entries=lo - 1)
    assert "gg_two_hop_top_pairs: buffer_entries = %d outside [%d, " % (lo - 1, lo) in str(ei.value)


def test_an_overflowing_first_batch_is_rerun_in_halves(ga):
    n = 300
    edges = [(a, b) for a in range(n) for b in range(a + 1, n)]
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    lo = minimum_buffer(ga, eng, 1, exclude=False)
    assert lo == 1 + n - 1
    res = against_ref(eng, N, 1, exclude=False, buffer_entries=lo)  # 256 sources append 43 000 pairs to 300 entries
    assert res["stats"]["retries"] > 0 and res["stats"]["compactions"] > 0
    cand = pref.candidates(N, exclude=False)
    for k in (5, 300, len(cand)):
        lo = minimum_buffer(ga, eng, k, exclude=False)
        res = eng.two_hop_top_pairs(k, exclude=False, buffer_entries=lo)
        check(res, pref.head(cand, k), k)
        assert same_bits(res, eng.two_hop_top_pairs(k, exclude=False))
    assert against_ref(eng, N, 10)["n_found"] == 0  # every pair is an edge
    eng.close()


def test_more_sources_than_a_launch_has_workgroups(ga):
    n = 6001  # batches of 256, 512, 1024, 2048 and then more than the 2048 workgroups of a launch
    edges = ls.circulant(n, (1, 5))
    N = ref.neighbor_sets(n, edges)
    eng = engine_for(ga, n, edges)
    cand = pref.candidates(N)
    n_src = sum(1 for u in range(n - 1) if pref.upper_expansion(N, u) > 0)
    assert n_src > 256 + 512 + 1024 + 2048 + 2048
    for k in (500, len(cand)):
        res = eng.two_hop_top_pairs(k)
        check(res, pref.head(cand, k), k)
        assert res["stats"]["swept"] == n_src and res["stats"]["launches"] == 5 and res["stats"]["skipped"] == 0
    eng.close()


def test_the_source_order_and_the_skip_bound_change_no_output(ga, ladder):
    g, rs = ladder, np.random.RandomState(21)
    n, k = g["n"], 1000
    perm = rs.permutation(n)  # old id -> new id
    back = np.argsort(perm)
    edges_p = perm[g["edges"]]
    Np = ref.neighbor_sets(n, edges_p)
    eng_p = engine_for(ga, n, edges_p)
    for weighted in (False, True):
        w = g["w"] if weighted else None
        wp = None if w is None else w[back]  # the weight of new node x is that of old node back[x]
        res_p = eng_p.two_hop_top_pairs(k, weights=wp)
        check(res_p, pref.top_pairs(Np, k, None, None if wp is None else wp.tolist(), True), weighted)
        assert res_p["stats"]["skipped"] > 0
        orig = g["eng"].two_hop_top_pairs(k, weights=w)
        assert res_p["score"].tolist() == orig["score"].tolist()
        cut = int(orig["score"][-1])
        mapped = {}
        for a, b, s in zip(back[res_p["u"]].tolist(), back[res_p["v"]].tolist(), res_p["score"].tolist()):
            mapped.setdefault(s, set()).add((min(a, b), max(a, b)))
        mine = {}
        for a, b, s in zip(orig["u"].tolist(), orig["v"].tolist(), orig["score"].tolist()):
            mine.setdefault(s, set()).add((a, b))
        assert all(mapped[s] == mine[s] for s in mine if s > cut) and len([s for s in mine if s > cut]) >= 1
        if weighted:  # distinct scores: the same pairs in the same order
            head = [i for i, s in enumerate(orig["score"].tolist()) if s > cut and orig["score"].tolist().count(s) == 1][:200]
            assert len(head) >= 10
            assert [(min(a, b), max(a, b)) for a, b in zip(back[res_p["u"][head]].tolist(), back[res_p["v"][head]].tolist())] == \
                list(zip(orig["u"][head].tolist(), orig["v"][head].tolist()))
    eng_p.close()


def test_cross_checks_with_the_pair_neighbour_and_the_two_hop_sweeps(ga, ladder):
    g = ladder
    eng = g["eng"]
    for exclude in (True, False):
        res = eng.two_hop_top_pairs(5000, weights=g["w"], exclude=exclude)
        pn = eng.pair_neighbors(res["u"], res["v"], g["w"][None, :])
        assert res["score"].tolist() == pn["wsum"][0].tolist()
        res = eng.two_hop_top_pairs(5000, exclude=exclude)
        assert res["score"].tolist() == eng.pair_neighbors(res["u"], res["v"])["cn"].tolist()
        assert same_bits(res, eng.two_hop_top_pairs(5000, exclude=exclude))  # two runs, equal bits
    n, rs = 300, np.random.RandomState(17)
    edges = rs.randint(0, n, (600, 2))
    w = rs.randint(0, 2 ** 41, n).astype(np.uint64)
    small = engine_for(ga, n, edges)
    for weights in (None, w):
        rows = small.two_hop_topk(np.arange(n), k=256, weights=weights, exclude=True)
        assert rows["n_pos"].max() <= 256
        merged = sorted((-int(s), u, int(c)) for u in range(n) for c, s in zip(rows["col"][u].tolist(), rows["score"][u].tolist()) if c > u)
        res = small.two_hop_top_pairs(len(merged) + 5, weights=weights, exclude=True)
        assert res["n_found"] == len(merged) > 100
        assert [(-s, u, c) for u, c, s in zip(res["u"].tolist(), res["v"].tolist(), res["score"].tolist())][:len(merged)] == merged
    small.close()


def test_refusals_name_the_function_and_the_value(ga):
    from graphgan_amd import _lib
    n = 50
    eng = engine_for(ga, n)
    with pytest.raises(ga.GraphGANHipError) as ei:
        eng.two_hop_top_pairs(3)
    assert ei.value.code == ga.GG_EINVAL and "gg_two_hop_top_pairs: needs the training graph (gg_set_graph_csr)" in str(ei.value)
    ring = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int32)
    eng.set_graph_csr(*ga.edges_to_csr(n, ring))

    def refused(call, text, exc=None):
        with pytest.raises(exc or ga.GraphGANHipError) as ei:
            call()
        assert text in str(ei.value), str(ei.value)
        if exc is None:
            assert ei.value.code == ga.GG_EINVAL

    # through Engine: the Python layer refuses the same things, before the ABI
    V = ValueError
    for k in (0, 2 ** 20 + 1, -1, 2.0, True):
        refused(lambda: eng.two_hop_top_pairs(k), "two_hop_top_pairs: k must be an integer in [1, 2^20], got %r" % (k,), V)
    refused(lambda: eng.two_hop_top_pairs(3, nodes=[0, 3, 50]), "two_hop_top_pairs: nodes[2] = 50 out of range [0, 50)", V)
    refused(lambda: eng.two_hop_top_pairs(3, nodes=[-1, 3]), "two_hop_top_pairs: nodes[0] = -1 out of range [0, 50)", V)
    refused(lambda: eng.two_hop_top_pairs(3, nodes=[0, 5, 5]), "two_hop_top_pairs: nodes[2] = 5 is not above nodes[1] = 5 (strictly ascending ids)", V)
    refused(lambda: eng.two_hop_top_pairs(3, nodes=[4, 9, 7, 1]), "two_hop_top_pairs: nodes[2] = 7 is not above nodes[1] = 9 (strictly ascending ids)", V)
    for e in (1, 0, "self", None):
        refused(lambda: eng.two_hop_top_pairs(3, exclude=e), "two_hop_top_pairs: exclude must be True or False, got %r" % (e,), V)
    refused(lambda: eng.two_hop_top_pairs(3, weights=np.ones(49, np.uint64)), "two_hop_top_pairs: weights must be None or 50 non-negative integers", V)
    refused(lambda: eng.two_hop_top_pairs(3, weights=-np.ones(50, np.int64)), "two_hop_top_pairs: weights must be None or 50 non-negative integers", V)
    for s in (0, -4, 1.5):
        refused(lambda: eng.two_hop_top_pairs(3, scratch_bytes=s), "two_hop_top_pairs: scratch_bytes must be None or a positive integer, got %r" % (s,), V)
    for b in (0, -4, 1.5, True):
        refused(lambda: eng.two_hop_top_pairs(3, buffer_entries=b), "two_hop_top_pairs: buffer_entries must be None or a positive integer, got %r" % (b,), V)
    refused(lambda: eng.two_hop_top_pairs(3, weights=np.full(50, 2 ** 62, np.uint64)),
            "gg_two_hop_top_pairs: the largest weight 4611686018427387904 times the largest degree 2 does not fit in 63 bits")
    # a ring: T'(u) = 2 for most u, so one source appends at most 2 entries
    refused(lambda: eng.two_hop_top_pairs(3, buffer_entries=4),
            "gg_two_hop_top_pairs: buffer_entries = 4 outside [5, 67108864] (0: the default; the minimum is k + 2, the most entries one source can append)")
    refused(lambda: eng.two_hop_top_pairs(3, buffer_entries=2 ** 26 + 1), "gg_two_hop_top_pairs: buffer_entries = 67108865 outside [5, 67108864]")

    # through the C ABI
    L, p = _lib.lib, lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ou, ov, sc = np.full(4, -7, np.int32), np.full(4, -7, np.int32), np.full(4, 7, np.uint64)
    found, stats = np.full(1, -7, np.int64), np.full(6, -7, np.int64)
    big = np.full(n, 2 ** 62, np.uint64)

    def raw(nodes=None, m=0, k=3, w=None, excl=1, scratch=0, buf=0, ou=ou, ov=ov, sc=sc, found=found, stats=stats):
        return lambda: _lib.check(L.gg_two_hop_top_pairs(eng._ctx, p(nodes), m, k, p(w), excl, scratch, buf, p(ou), p(ov), p(sc), p(found), p(stats), None), eng._ctx)

    raw()()  # (kernel_ms may be NULL)
    assert ou.tolist() == [0, 0, 1, -7] and ov.tolist() == [2, 48, 3, -7] and sc.tolist() == [1, 1, 1, 7] and found.tolist() == [3]  # only k entries are written
    assert stats[0] >= 1 and stats[4] == n - 2 and stats[5] == 0  # (the two last nodes of the ring have nobody above them)
    raw(stats=None)()
    for k in (0, 2 ** 20 + 1, -1):
        refused(raw(k=k), "gg_two_hop_top_pairs: k = %d outside [1, 2^20]" % k)
    for e in (2, 3, -1):
        refused(raw(excl=e), "gg_two_hop_top_pairs: exclude = %d is neither 0 nor 1" % e)
    refused(raw(scratch=-1), "gg_two_hop_top_pairs: scratch_bytes = -1 is negative")
    refused(raw(buf=-2), "gg_two_hop_top_pairs: buffer_entries = -2 is negative")
    for kw in (dict(ou=None), dict(ov=None), dict(sc=None), dict(found=None)):
        refused(raw(**kw), "gg_two_hop_top_pairs: out_u, out_v, out_score and n_found must not be NULL")
    refused(raw(nodes=np.array([0, 1], np.int32), m=-1), "gg_two_hop_top_pairs: m = -1 is negative")
    refused(raw(nodes=np.array([0, 50], np.int32), m=2), "gg_two_hop_top_pairs: nodes[1] = 50 out of range [0, 50)")
    refused(raw(nodes=np.array([-3, 5], np.int32), m=2), "gg_two_hop_top_pairs: nodes[0] = -3 out of range [0, 50)")
    refused(raw(nodes=np.array([0, 7, 7], np.int32), m=3), "gg_two_hop_top_pairs: nodes[2] = 7 is not above nodes[1] = 7 (strictly ascending ids)")
    refused(raw(w=big), "gg_two_hop_top_pairs: the largest weight 4611686018427387904 times the largest degree 2 does not fit in 63 bits")
    refused(raw(buf=4), "gg_two_hop_top_pairs: buffer_entries = 4 outside [5, 67108864] (0: the default; the minimum is k + 2, the most entries one source can append)")
    raw(excl=0, buf=5)()  # the engine stays usable (a ring has no triangle: its edges score 0 and stay out either way)
    assert ou.tolist() == [0, 0, 1, -7] and ov.tolist() == [2, 48, 3, -7] and found.tolist() == [3]
    raw(nodes=np.zeros(1, np.int32), m=0)()  # an empty set: nothing found, the outputs padded
    assert ou.tolist() == [-1, -1, -1, -7] and sc.tolist() == [0, 0, 0, 7] and found.tolist() == [0]
    eng.close()


def _files(tmp_path, train, test):
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    np.savetxt(tr, train, fmt="%d")
    np.savetxt(te, test, fmt="%d")
    return tr, te


def test_results_lines_with_an_engine_are_string_equal_to_the_host_evaluator_on_a_random_graph(ga, tmp_path):
    from graphgan_amd.evaluation import graph_pairs as gp
    n, rs = 400, np.random.RandomState(31)
    edges = rs.randint(0, n - 5, (1500, 2))
    train, test = edges[:1300], edges[1300:]
    tr, te = _files(tmp_path, train, test)
    eng = engine_for(ga, n, train)
    ks = (10, 100, 3000)
    dev, host = gp.GraphPairsEval(tr, te, n, engine=eng, ks=ks), gp.GraphPairsEval(tr, te, n, ks=ks)
    for kind, prefix in (("pairs", "graph_pairs:index="), ("recon", "graph_recon:index=")):
        a, b = dev.lines(kind), host.lines(kind)
        assert a == b and len(a) == 3 and [ln.split(" ")[0].split("=")[1] for ln in a] == ["cn", "aa", "ra"]
        assert all(ln.startswith(prefix) and ln.endswith("\n") for ln in a)
    eng.close()


def test_results_lines_on_ca_grqc_beside_the_embedding_lines(ga, tmp_path):
    from graphgan_amd.evaluation import graph_pairs as gp
    from graphgan_amd.evaluation import pair_prediction as pp
    from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc
    d, n, _ = load_ca_grqc()
    train, test = np.asarray(d["train"]), np.asarray(d["test"])
    tr, te = _files(tmp_path, train, test)
    emb = ca_grqc_init_embeddings(d, n).astype(np.float32)
    eng = ga.Engine(emb, emb)
    eng.set_graph_csr(*ga.edges_to_csr(n, train.astype(np.int32)))
    ks = (100, 1000)
    dev, host = gp.GraphPairsEval(tr, te, n, engine=eng, ks=ks), gp.GraphPairsEval(tr, te, n, ks=ks)
    lines = dev.lines("pairs") + dev.lines("recon")
    assert lines == host.lines("pairs") + host.lines("recon") and len(lines) == 6  # all three indices, both kinds
    pe = pp.PairPredictionEval(tr, te, n, emb.shape[1], engine=eng, ks=ks)
    emb_pairs, emb_recon = pe.eval_pair_prediction(), pe.eval_graph_reconstruction()
    graph = dev.eval_graph_pairs()["cn"]
    assert (graph["n_test"], graph["dropped"], graph["n"]) == (emb_pairs["n_test"], emb_pairs["dropped"], emb_pairs["n"])  # one rule for the positives
    print("CA-GrQc, shipped rows: " + pp.format_pairs("gen", emb_pairs, ks).strip())  # reported, not gated
    print("CA-GrQc, shipped rows: " + pp.format_recon("gen", emb_recon, ks).strip())
    for ln in lines:
        print("CA-GrQc, graph only:  " + ln.strip())
    eng.close()
