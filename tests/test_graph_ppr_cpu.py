"""The host side of the rooted-PageRank ranking baseline (graphgan_amd/evaluation/graph_ppr.py, graph_gan.py's
engine_link_rank_ppr_baseline / engine_rec_ppr_baseline, ``python -m graphgan_amd.recommend --index ppr``): the numpy rounds against
the restatement in dicts and ints (tests/support/ppr_ref.py), the invariants of the rule, the scores against a float64 dense solve
inside a derived bound, the edge cases, the results lines, their place and their caches -- and the ABI declarations, the constants
and the build audit of gg_ppr_topk / gg_ppr_rank."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests.support import ppr_ref as ref
from tests.support import two_hop_ref as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 40
# (alpha_q, eps_q): the defaults, a coarse pair (few pushes), a fine pair (many rounds), the largest alpha, the smallest product
QUANTA = ((9830, 109951163), (32768, 1 << 32), (9830, 1 << 20), (65535, 2), (1, 65536))


@pytest.fixture(scope="module")
def gp():
    from graphgan_amd.evaluation import graph_ppr
    return graph_ppr


@pytest.fixture(scope="module")
def lh():
    from graphgan_amd.evaluation import link_heuristics
    return link_heuristics


def test_header_declares_and_library_exports_the_two_symbols():
    from graphgan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {"gg_ppr_topk": ["gg_ctx*", "constint32_t*", "int64_t", "int32_t", "uint32_t", "uint64_t", "int32_t", "int32_t", "int64_t", "int32_t*", "uint64_t*",
                            "int32_t*", "int32_t*", "int32_t*", "uint64_t*", "double*"],
            "gg_ppr_rank": ["gg_ctx*", "constint32_t*", "constint32_t*", "int64_t", "uint32_t", "uint64_t", "int32_t", "int32_t", "int64_t", "uint64_t*",
                            "int32_t*", "int32_t*", "int32_t*", "int32_t*", "int32_t*", "uint64_t*", "double*"]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, types_ in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/graphgan_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == types_
        assert len(_lib.SIGNATURES[name][1]) == len(args)
        assert hasattr(so, name) and hasattr(_lib.lib, name)
    for name, at in (("gg_ppr_topk", 4), ("gg_ppr_rank", 4)):
        sig = _lib.SIGNATURES[name][1]
        assert sig[at] is ctypes.c_uint32 and sig[at + 1] is ctypes.c_uint64 and sig[at + 2] is ctypes.c_int32 and sig[at + 4] is ctypes.c_int64
    assert _lib.header_abi_version() == 9 and so.gg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays
    assert "push sweep" in open(_lib.HEADER_PATH).read()


def test_constants_footprint_and_audit_are_in_step_with_the_source():
    from graphgan_amd import _lib
    from graphgan_amd.engine import Engine
    csrc = os.path.join(ROOT, "graphgan_amd", "csrc")
    src = open(os.path.join(csrc, "ppr_push.hip")).read()
    consume = open(os.path.join(csrc, "set_consume.h")).read()
    m = re.search(r"constexpr int PPR_LDS_CAP = (\d+);", src)
    assert m and int(m.group(1)) == _lib.PPR_LDS_CAP == Engine.PPR_LDS_CAP
    cap = int(m.group(1))
    assert re.search(r"constexpr int PPR_LDS_SLOTS = 2 \* PPR_LDS_CAP;", src)
    k = int(re.search(r"constexpr int SET_MAX_K = (\d+);", consume).group(1))
    assert k == 256 == int(re.search(r"constexpr int TH_MAX_K = (\d+);", open(os.path.join(csrc, "two_hop.hip")).read()).group(1))
    # one workgroup: keys, r and p over 2 x CAP slots; per frontier entry the share, two list entries and a 16-bit long-list index;
    # the top-K consumer's survivors, histogram and fold words (the larger of the two consumers); the counters and fold words
    table, frontier, consumer = 2 * cap * (4 + 8 + 8), cap * (8 + 2 * 4 + 2), k * (8 + 4) + 256 * 4 + 4 * 8 + 8 + 4 * 4 + 4 * 4
    assert table + frontier + consumer + 4 * 4 + 4 * 8 <= 64 * 1024
    assert 2 * cap == 2048  # set_table_slots(CAP): an LDS task never needs more slots than the arrays hold
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^ppr_push\.o: AUDIT = 'pp_\[a-z0-9_\]\*kernel' 4 ", mk, flags=re.M)  # rank and top-K, each with the tables in LDS and global
    assert re.search(r"^AUDITED = .*\bppr_push\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\bppr_push\.o\b", mk, flags=re.M)
    assert re.search(r"^[a-z_. ]*\bppr_push\.o\b[a-z_. ]*: set_sweep\.h$", mk, flags=re.M)
    assert re.search(r"^[a-z_. ]*\bppr_push\.o\b[a-z_. ]*: set_consume\.h$", mk, flags=re.M) and re.search(r"^[a-z_. ]*\btwo_hop\.o\b[a-z_. ]*: set_consume\.h$", mk, flags=re.M)
    assert sorted(re.findall(r"^__global__ .*void (pp_\w+_kernel)\(", src, flags=re.M)) == ["pp_rank_kernel", "pp_topk_kernel"]
    device = src[:src.index("int pp_run(")] + consume  # the kernels and the whole header of the shared consumers
    assert not re.search(r"\b(float|double|fmaf?|__f\w+_rn|asm)\b", device)
    assert '#include "set_consume.h"' in open(os.path.join(csrc, "two_hop.hip")).read()  # the two-hop sweep uses the same consumers


def small_graph():
    """60 nodes, the last three isolated, duplicates and self-loops"""
    rs = np.random.RandomState(0)
    n = 60
    e = rs.randint(0, n - 3, size=(150, 2))
    e = np.concatenate([e, e[:10], e[10:20, ::-1], [[5, 5], [7, 7]]])
    return n, e


def test_host_rounds_and_the_invariants_against_the_restatement(gp, lh):
    n, e = small_graph()
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    assert [len(s) for s in N] == np.diff(ptr).tolist() and not N[n - 1]
    rows = np.arange(n)
    u, v = np.repeat(rows, n), np.tile(rows, n)  # every target of every root
    rs = np.random.RandomState(1)
    for alpha_q, eps_q in QUANTA:
        alpha, eps = alpha_q / 65536.0, eps_q / float(ONE)
        assert gp.quantise(alpha, eps) == (alpha_q, eps_q)
        kmin, B, E = ref.bounds(n, alpha_q, eps_q)
        assert gp.touched_bound(n, alpha_q, eps_q) == E
        for max_rounds in (200, 3):
            dense = [ref.dense_row(N, a, alpha_q, eps_q, max_rounds) for a in range(n)]
            for a, (row, info) in enumerate(dense):  # the rule's consequences (sum p + sum r == 2^40 is asserted per round inside)
                assert sum(row) + info["residual"] == ONE and info["sum_deg"] <= B and len(info["touched"]) <= E
                assert info["rounds"] <= max_rounds and info["converged"] == int(not [x for x, rx in info["r"].items() if rx > 0 and rx >= eps_q * max(len(N[x]), 1)])
            for exclude in (True, "self"):
                for k in (1, 7, 256):
                    t = gp.host_ppr_topk(ptr, adj, rows, k, alpha, eps, max_rounds, exclude)
                    assert t["col"].dtype == np.int32 and t["score"].dtype == t["residual"].dtype == np.uint64 and t["rounds"].dtype == np.int32
                    for a in range(n):
                        col, score, n_pos = th.topk(N, a, k, None, exclude, row=dense[a][0])
                        assert (t["col"][a].tolist(), t["score"][a].tolist(), int(t["n_pos"][a])) == (col, score, n_pos)
                    info = [d[1] for d in dense]
                    assert t["rounds"].tolist() == [i["rounds"] for i in info] and t["converged"].tolist() == [i["converged"] for i in info]
                    assert t["residual"].tolist() == [i["residual"] for i in info] and t["pushed"].tolist() == [i["sum_deg"] for i in info]
                r = gp.host_ppr_rank(ptr, adj, u, v, alpha, eps, max_rounds, exclude)
                assert r["rank"].dtype == r["n_cand"].dtype == np.int64 and r["score"].dtype == np.uint64
                for i in rs.permutation(n * n)[:300].tolist() + [0, n - 1, n * n - 1]:
                    want = th.rank(N, int(u[i]), int(v[i]), None, exclude, row=dense[int(u[i])][0])
                    assert {key: int(r[key][i]) for key in want} == want
                    assert (int(r["rounds"][i]), int(r["residual"][i])) == (dense[int(u[i])][1]["rounds"], dense[int(u[i])][1]["residual"])
                mix = rs.permutation(n * n)[:500]  # unsorted queries: the same bits per query
                r2 = gp.host_ppr_rank(ptr, adj, u[mix], v[mix], alpha, eps, max_rounds, exclude)
                assert all(np.array_equal(r2[key], r[key][mix]) for key in r)
    assert gp.host_ppr_topk(ptr, adj, [], 3)["col"].shape == (0, 3) and gp.host_ppr_rank(ptr, adj, [], [])["rank"].shape == (0,)


def test_scores_against_the_float64_dense_solve_inside_the_derived_bound(gp, lh):
    """ppr_x = alpha (I - (1 - alpha) A D^-1)^-1 e_x obeys ppr_x = alpha e_x + (1 - alpha) / deg(x) * sum over w in N(x) of ppr_w, so
    a REAL partial push of t units at x (p[x] += alpha t, r[x] -= t, r[w] += (1 - alpha) t / deg for w in N(x)) keeps
    p + sum_x r[x] ppr_x = ONE * ppr_u exactly.  An integer push from r0 hands share * deg = (1 - alpha) r0 + d - rem units to the
    neighbours, with d = the fraction the shift drops from alpha r0 (0 <= d < 1) and rem < deg: that is the real push of
    t = r0 - (rem - d) / (1 - alpha), which would book alpha t to p[x] and leave r0 - t in r[x].  The integer push books
    alpha r0 - d and leaves rem: it differs by moving m = (alpha rem - d) / (1 - alpha) units from r[x] to p[x], which changes
    p + sum r ppr by m (e_x - ppr_x), of L1 norm at most 2 |m| <= 2 max(1, alpha (deg - 1)) / (1 - alpha) (rem <= deg - 1, d < 1; ppr_x
    is a distribution: no reachable node is isolated).  At the end |p - ONE ppr_u|_1 <= |sum r ppr|_1 + sum of the moves
    = residual + sum over pushes of 2 max(1, alpha (deg - 1)) / (1 - alpha); 1e-12 covers the float64 solve."""
    n, e = small_graph()
    rs = np.random.RandomState(3)
    big_n = 300
    big = rs.randint(0, big_n, size=(900, 2))
    for nn, edges in ((n, e), (big_n, big)):
        N = ref.neighbor_sets(nn, edges)
        ptr, adj = lh.set_adjacency(edges, nn)
        deg = np.diff(ptr).astype(np.float64)
        A = np.zeros((nn, nn))
        for x in range(nn):
            A[list(N[x]), x] = 1.0 / deg[x] if deg[x] else 0.0  # column x of A D^-1
        for alpha_q, eps_q in ((9830, 109951163), (9830, 1 << 20), (32768, 1 << 26), (58982, 1 << 22)):
            alpha = alpha_q / 65536.0
            ppr = alpha * np.linalg.inv(np.eye(nn) - (1.0 - alpha) * A)
            roots = [x for x in range(nn) if N[x]][::1 if nn == n else 7]
            res = gp.host_ppr_topk(ptr, adj, roots, 1, alpha, eps_q / float(ONE), 500, "self")
            assert res["converged"].all()
            worst = 0.0
            for a in roots:
                row, info = ref.dense_row(N, a, alpha_q, eps_q, 500)
                err = np.abs(np.array(row, dtype=np.float64) / ONE - ppr[:, a]).sum()
                bound = (info["residual"] + sum(2.0 * max(1.0, alpha * (d - 1)) / (1.0 - alpha) for d, _, _ in info["err_terms"])) / ONE + 1e-12
                assert err <= bound, (a, alpha_q, eps_q, err, bound)
                # the moves themselves, as derived: |alpha rem - d| / (1 - alpha) each -- the tighter form of the same bound
                exact = (info["residual"] + sum(2.0 * abs(alpha * rem - dq / 65536.0) / (1.0 - alpha) for _, rem, dq in info["err_terms"])) / ONE + 1e-12
                assert err <= exact <= bound
                worst = max(worst, err / (info["residual"] / ONE + 1e-12))
            print("n=%d alpha_q=%d eps_q=%d: largest error / residual = %.6f" % (nn, alpha_q, eps_q, worst))


def test_edge_cases_of_the_rule(gp, lh):
    # 0: a centre with 300 leaves (1 .. 300); 301-302 an edge; 303 isolated
    n = 304
    e = [[0, j] for j in range(1, 301)] + [[301, 302]]
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    # a degree-0 root: everything is kept in one round
    t = gp.host_ppr_topk(ptr, adj, [303], 5, exclude="self")
    assert (int(t["rounds"][0]), int(t["converged"][0]), int(t["residual"][0]), int(t["n_pos"][0])) == (1, 1, 0, 0) and (t["col"] == -1).all()
    r = gp.host_ppr_rank(ptr, adj, [303], [303], exclude="self")
    assert int(r["score"][0]) == ONE and int(r["rank"][0]) == 1
    info = ref.push(N, 303, 9830, 109951163, 200)
    assert info["p"] == {303: ONE} and info["rounds"] == 1 and info["pushes"] == 1 and info["sum_deg"] == 0
    # a root with eps_q deg > 2^40: nothing moves
    eps = (1 << 32) / float(ONE)
    assert (1 << 32) * 300 > ONE
    t = gp.host_ppr_topk(ptr, adj, [0, 1], 5, 0.5, eps, exclude="self")
    assert t["rounds"].tolist() == [0, 1] and t["converged"].tolist() == [1, 1] and int(t["residual"][0]) == ONE
    assert int(t["n_pos"][0]) == 0 and (t["col"][0] == -1).all() and (t["score"][0] == 0).all()
    r = gp.host_ppr_rank(ptr, adj, [0, 0], [5, 0], 0.5, eps, exclude="self")
    assert r["score"].tolist() == [0, 0] and r["rank"].tolist() == [5, 1] and r["rounds"].tolist() == [0, 0] and r["residual"].tolist() == [ONE, ONE]
    assert ref.push(N, 0, 32768, 1 << 32, 200)["rounds"] == 0
    # max_rounds = 1, unconverged
    t = gp.host_ppr_topk(ptr, adj, [0, 301], 256, max_rounds=1, exclude="self")
    assert t["rounds"].tolist() == [1, 1] and t["converged"].tolist() == [0, 0]
    keep = (ONE * 9830) >> 16
    assert int(t["residual"][0]) == ONE - keep and t["score"][0].tolist() == [0] * 256  # only the root holds p; it is excluded
    assert t["n_pos"].tolist() == [0, 0] and int(gp.host_ppr_rank(ptr, adj, [0], [0], max_rounds=1, exclude="self")["score"][0]) == keep


def test_quantise_and_every_value_error(gp, lh):
    assert gp.quantise(0.15, 1e-4) == (9830, 109951163) and gp.quantise(0.5, 2.0 ** -8) == (32768, 1 << 32)
    assert gp.quantise(0.99999, 2.0 ** -39) == (65535, 2) and gp.quantise(2.0 ** -16, 2.0 ** -24) == (1, 65536)
    assert gp.quantise(np.float32(0.25), np.float64(1e-6)) == (16384, 1099512)
    ptr, adj = lh.set_adjacency([[0, 1], [1, 2]], 4)
    V = ValueError
    for call, text in ((lambda: gp.quantise(0.0, 1e-4), r"alpha = 0.0 gives alpha_q = 0 outside \[1, 65535\]"),
                       (lambda: gp.quantise(1.0, 1e-4), r"alpha = 1.0 gives alpha_q = 65536 outside \[1, 65535\]"),
                       (lambda: gp.quantise(-0.2, 1e-4), r"alpha = -0.2 gives alpha_q = -13107 outside \[1, 65535\]"),
                       (lambda: gp.quantise(0.15, 0.004), r"eps = 0.004 gives eps_q = 4398046511 outside \[1, 4294967296\]"),
                       (lambda: gp.quantise(0.15, -1e-4), r"eps = -0.0001 gives eps_q outside \[1, 4294967296\]"),
                       (lambda: gp.quantise(0.15, 1e30), r"eps = 1e\+30 gives eps_q outside \[1, 4294967296\]"),
                       (lambda: gp.quantise(0.15, 0.0), r"alpha_q \* eps_q = 9830 is below 65536 \(alpha = 0.15, eps = 0.0\)"),
                       (lambda: gp.quantise(0.15, 1e-13), r"alpha_q \* eps_q = 9830 is below 65536"),
                       (lambda: gp.quantise(2.0 ** -16, 2.0 ** -25), r"alpha_q \* eps_q = 32768 is below 65536"),
                       (lambda: gp.quantise(float("nan"), 1e-4), r"alpha and eps must be finite"),
                       (lambda: gp.quantise(0.15, float("inf")), r"alpha and eps must be finite"),
                       (lambda: gp.quantise("a", 1e-4), r"alpha and eps must be numbers"),
                       (lambda: gp.quantise(None, 1e-4), r"alpha and eps must be numbers"),
                       (lambda: gp.check_max_rounds("f", 0), r"f: max_rounds must be a positive integer, got 0"),
                       (lambda: gp.check_max_rounds("f", 2.0), r"f: max_rounds must be a positive integer, got 2.0"),
                       (lambda: gp.check_max_rounds("f", True), r"f: max_rounds must be a positive integer, got True"),
                       (lambda: gp.host_ppr_topk(ptr, adj, [0], exclude=False), r"host_ppr_topk: exclude must be True or 'self', got False"),
                       (lambda: gp.host_ppr_rank(ptr, adj, [0], [1], exclude="graph"), r"host_ppr_rank: exclude must be True or 'self', got 'graph'"),
                       (lambda: gp.host_ppr_topk(ptr, adj, [0], k=0), r"host_ppr_topk: k must be an integer in \[1, 256\], got 0"),
                       (lambda: gp.host_ppr_topk(ptr, adj, [0], k=257), r"host_ppr_topk: k must be an integer in \[1, 256\], got 257"),
                       (lambda: gp.host_ppr_topk(ptr, adj, [0, 4]), r"host_ppr_topk: rows\[1\] = 4 out of range \[0, 4\)"),
                       (lambda: gp.host_ppr_rank(ptr, adj, [0, -1], [0, 0]), r"host_ppr_rank: u\[1\] = -1 out of range \[0, 4\)"),
                       (lambda: gp.host_ppr_rank(ptr, adj, [0, 1], [9, 0]), r"host_ppr_rank: v\[0\] = 9 out of range \[0, 4\)"),
                       (lambda: gp.host_ppr_rank(ptr, adj, [0, 1], [0]), r"u and v must have the same length, got 2 and 1"),
                       (lambda: gp.host_ppr_topk(ptr, adj, [0], max_rounds=0), r"host_ppr_topk: max_rounds must be a positive integer, got 0"),
                       (lambda: gp.host_ppr_rank(ptr, adj, [0], [1], alpha=1.5), r"alpha = 1.5 gives alpha_q = 98304 outside"),
                       (lambda: gp.GraphPprRankEval("t", "e", 4, ks=(1, 0)), r"GraphPprRankEval: every K must be a positive integer"),
                       (lambda: gp.GraphPprRankEval("t", "e", 4, eps=1.0), r"eps = 1.0 gives eps_q = 1099511627776 outside"),
                       (lambda: gp.GraphPprRankEval("t", "e", 4, max_rounds=-1), r"GraphPprRankEval: max_rounds must be a positive integer, got -1"),
                       (lambda: gp.GraphPprRecEval("t", "e", 4, ks=(2, 257)), r"GraphPprRecEval: every K must lie in \[1, 256\]"),
                       (lambda: gp.GraphPprRecEval("t", "e", 4, ks=()), r"GraphPprRecEval: every K must lie in \[1, 256\]"),
                       (lambda: gp.GraphPprRecEval("t", "e", 4, alpha=0), r"alpha = 0 gives alpha_q = 0 outside"),
                       (lambda: gp.format_results("lp", {}, (), 0.15, 1e-4), r"kind must be 'rank' or 'rec'")):
        with pytest.raises(V, match=text):
            call()


def test_full_rank_places_zero_score_targets_from_the_push_sweeps_counts(gp, lh):
    """graph_ranking.full_rank, unchanged, on the restatement's counts under a coarse pair that leaves most scores zero: targets 0,
    n - 1, mid-range, u itself, neighbours, in both modes"""
    from graphgan_amd.evaluation import graph_ranking as gr
    n, e = small_graph()
    N = ref.neighbor_sets(n, e)
    ptr, adj = lh.set_adjacency(e, n)
    u, v = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    alpha_q, eps_q = 32768, 1 << 32
    dense = [ref.dense_row(N, a, alpha_q, eps_q, 200)[0] for a in range(n)]
    for exclude, code in ((True, 2), ("self", 1)):
        want = [th.rank(N, a, b, None, exclude, row=dense[a]) for a, b in zip(u.tolist(), v.tolist())]
        cols = {key: np.array([x[key] for x in want]) for key in want[0]}
        assert (cols["score"] == 0).sum() > n * n // 2 and (cols["score"][v == 0] == 0).any() and (cols["score"][(v == n - 1) & (u != n - 1)] == 0).all()
        rank, n_cand = gr.full_rank(ptr, adj, u, v, code, cols["score"], cols["ahead"], cols["n_pos"], cols["pos_below"])
        assert rank.tolist() == cols["rank"].tolist() and n_cand.tolist() == cols["n_cand"].tolist()


def test_evaluators_are_link_rankings_and_the_lines_are_what_they_say(gp, lh, tmp_path):
    from graphgan_amd.evaluation import link_ranking as lrank
    from graphgan_amd.evaluation import recommendation as rec
    n, e = small_graph()
    train, test = e[:120], np.array([[a, b] for a, b in e[120:150].tolist() if a != b] + [[0, n - 1]])
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    np.savetxt(tr, train, fmt="%d")
    np.savetxt(te, test, fmt="%d")
    N = ref.neighbor_sets(n, train)
    ks = (1, 3, 50)
    alpha, eps = 0.25, 2.0 ** -12
    alpha_q, eps_q = gp.quantise(alpha, eps)
    ev = gp.GraphPprRankEval(tr, te, n, ks=ks, alpha=alpha, eps=eps, max_rounds=6)
    res = ev.eval_graph_ranking()
    from graphgan_amd.evaluation.generator_likelihood import edge_pairs
    pairs = edge_pairs(te)  # LinkRankEval's queries: every test edge in both directions ...
    assert sorted(pairs.tolist()) == sorted(test.tolist() + test[:, ::-1].tolist())
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]  # ... sorted by their root (the summary's float sums take this order)
    dense = {a: ref.dense_row(N, a, alpha_q, eps_q, 6) for a in set(pairs[:, 0].tolist())}
    got = [th.rank(N, a, b, None, True, row=dense[a][0]) for a, b in pairs.tolist()]
    want = lrank.summarize(lrank.filtered_ranks(pairs[:, 0], pairs[:, 1], [x["rank"] for x in got]), ks)  # link_ranking's own filter and summary
    want["reach"] = sum(1 for x in got if x["score"] > 0) / len(pairs)
    want["rounds"] = max(dense[a][1]["rounds"] for a in pairs[:, 0].tolist())
    want["converged"] = sum(dense[a][1]["converged"] for a in pairs[:, 0].tolist()) / len(pairs)
    want["residual"] = float(sum(dense[a][1]["residual"] for a in pairs[:, 0].tolist())) / len(pairs) / float(ONE)
    assert res == want and 0.0 < want["reach"] < 1.0 and want["rounds"] == 6 and 0.0 < want["converged"] < 1.0
    line = gp.format_results("rank", res, ks, alpha, eps)
    assert line == "graph_rank:index=ppr MRR=%s MR=%s H@1=%s H@3=%s H@50=%s n=%d reach=%s alpha=0.25 eps=0.000244140625 rounds=6 converged=%s residual=%s\n" % (
        str(want["mrr"]), str(want["mr"]), str(want["hits"][1]), str(want["hits"][3]), str(want["hits"][50]), len(pairs), str(want["reach"]),
        str(want["converged"]), str(want["residual"]))
    assert ev.lines() == [line]
    # the recommendation line: RecommendEval's queries and scoring; a -1 column is a miss
    rk = (2, 5)
    rev = gp.GraphPprRecEval(tr, te, n, ks=rk, alpha=0.5, eps=2.0 ** -8)
    test_nbrs = rec._neighbour_sets(test.tolist(), n)
    queries = [u for u in range(n) if test_nbrs[u]]
    ranked = np.array([ref.topk(N, u, 5, 32768, 1 << 32, 200, True)[0] for u in queries])
    assert (ranked == -1).any()
    want = rec.precision_recall(ranked, queries, test_nbrs, rk)
    assert rev.eval_graph_recommendation() == want
    assert rev.lines() == ["graph_rec:index=ppr P@2=%s R@2=%s P@5=%s R@5=%s alpha=0.5 eps=0.00390625\n" % (str(want[2][0]), str(want[2][1]), str(want[5][0]), str(want[5][1]))]


def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def test_config_knob_defaults():
    from graphgan_amd import config
    assert config.engine_link_rank_ppr_baseline is False and config.engine_rec_ppr_baseline is False
    assert (config.engine_ppr_alpha, config.engine_ppr_eps, config.engine_ppr_max_rounds) == (0.15, 1e-4, 200)


@pytest.mark.parametrize("app", ["link_prediction", "recommendation"])
def test_lines_their_place_their_caches_and_a_config_without_the_knobs(gp, tmp_path, monkeypatch, app):
    from graphgan_amd.evaluation import graph_ranking as gr
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, n = _layout(tmp_path, app)
    assert cfg.engine_link_rank_ppr_baseline is False and cfg.engine_rec_ppr_baseline is False
    cfg.engine_gen_nll = True
    g.gen_likelihood = lambda: dict(nll=1.5, reach=1.0, n=7)  # (the NLL line needs an engine; its POSITION does not)
    cfg.engine_lp_heuristics = True
    cfg.engine_link_rank_ks, cfg.engine_rec_ks = (1, 20), (3, 10)
    want = GraphGAN.evaluation(g)  # the knobs' default: off
    first = open(cfg.result_filename, "rb").read()
    for knob in ("engine_link_rank_ppr_baseline", "engine_rec_ppr_baseline", "engine_ppr_alpha", "engine_ppr_eps", "engine_ppr_max_rounds"):
        delattr(cfg, knob)
    assert GraphGAN.evaluation(g) == want and [ln.split(":")[0] for ln in want] == ["gen", "dis", "graph_lp", "gen_nll"]  # a config without them
    assert open(cfg.result_filename, "rb").read() == first + first  # byte-identical
    # alone: where the two-hop lines would stand
    from graphgan_amd.graph_gan import _ppr_kw
    assert _ppr_kw(cfg) == dict(alpha=0.15, eps=1e-4, max_rounds=200)  # the parameters absent: the defaults
    cfg.engine_link_rank_ppr_baseline, cfg.engine_rec_ppr_baseline = True, True
    cfg.engine_ppr_eps, cfg.engine_ppr_max_rounds = 2.0 ** -10, 50  # (a coarse threshold: the host rounds of 4 000 roots stay quick)
    pkw = dict(eps=2.0 ** -10, max_rounds=50)
    lines = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in lines] == ["gen", "dis", "graph_lp", "graph_rank", "graph_rec", "gen_nll"]
    assert lines[:3] == want[:3] and lines[5] == want[3]  # the other lines keep every byte
    direct = gp.GraphPprRankEval(cfg.train_filename, cfg.test_filename, n, ks=(1, 20), **pkw).lines()
    direct += gp.GraphPprRecEval(cfg.train_filename, cfg.test_filename, n, ks=(3, 10), **pkw).lines()
    assert lines[3:5] == direct
    assert re.fullmatch(r"graph_rank:index=ppr MRR=0\.\d+ MR=\d+\.\d+ H@1=0\.\d+ H@20=0\.\d+ n=\d+ reach=0\.\d+ alpha=0\.15 eps=0\.0009765625 rounds=\d+ converged=1\.0 "
                        r"residual=0\.\d+\n", lines[3]), lines[3]
    assert re.fullmatch(r"graph_rec:index=ppr P@3=0\.\d+ R@3=0\.\d+ P@10=0\.\d+ R@10=0\.\d+ alpha=0\.15 eps=0\.0009765625\n", lines[4]), lines[4]
    print("CA-GrQc, host: " + " | ".join(ln.strip() for ln in lines[3:5]))
    # the second evaluation repeats the cached strings: nothing is computed again
    monkeypatch.setattr(gp.GraphPprRankEval, "lines", lambda self: pytest.fail("the graph_rank ppr line was computed twice"))
    monkeypatch.setattr(gp.GraphPprRecEval, "lines", lambda self: pytest.fail("the graph_rec ppr line was computed twice"))
    assert GraphGAN.evaluation(g) == lines and g._graph_ppr_rank_lines == lines[3:4] and g._graph_ppr_rec_lines == lines[4:5]
    assert open(cfg.result_filename, "rb").read() == first + first + "".join(lines + lines).encode()
    # beside the two-hop lines: behind the last graph_rank line and behind the last graph_rec line
    cfg.engine_link_rank_graph_baseline, cfg.engine_rec_graph_baseline, cfg.engine_graph_rank_indices = True, True, ("cn", "aa")
    g._graph_rank_lines = ["graph_rank:index=cn stub\n", "graph_rank:index=aa stub\n"]  # (cached lines: the two-hop evaluators have their own test)
    g._graph_rec_lines = ["graph_rec:index=cn stub\n", "graph_rec:index=aa stub\n"]
    both = GraphGAN.evaluation(g)
    assert both == lines[:3] + g._graph_rank_lines + lines[3:4] + g._graph_rec_lines + lines[4:5] + lines[5:]
    cfg.engine_link_rank_ppr_baseline = False
    assert GraphGAN.evaluation(g) == lines[:3] + g._graph_rank_lines + g._graph_rec_lines + lines[4:5] + lines[5:]
    assert gr.INDICES == ("cn", "aa", "ra")


def test_the_knobs_are_checked_where_the_others_are(gp, tmp_path):
    from graphgan_amd.graph_gan import GraphGAN, _check_graph_ppr
    cfg, g, n = _layout(tmp_path)
    test_file = cfg.test_filename
    for knob in ("engine_link_rank_ppr_baseline", "engine_rec_ppr_baseline"):
        setattr(cfg, knob, True)
        cfg.test_filename = str(tmp_path / "no_such_test.txt")
        with pytest.raises(ValueError, match="%s needs test edges: config.test_filename does not exist" % knob):
            GraphGAN.evaluation(g)
        assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
        with pytest.raises(ValueError, match="test_filename"):
            _check_graph_ppr(types.SimpleNamespace(**{knob: True}))
        cfg.test_filename = test_file
        for name, bad, text in (("engine_ppr_alpha", 1.0, r"alpha = 1.0 gives alpha_q = 65536 outside \[1, 65535\]"),
                                ("engine_ppr_eps", 0.5, r"eps = 0.5 gives eps_q = 549755813888 outside \[1, 4294967296\]"),
                                ("engine_ppr_eps", 1e-13, r"alpha_q \* eps_q = 9830 is below 65536"),
                                ("engine_ppr_max_rounds", 0, r"max_rounds must be a positive integer, got 0")):
            good = getattr(cfg, name)
            setattr(cfg, name, bad)
            with pytest.raises(ValueError, match=text):
                GraphGAN.evaluation(g)
            setattr(cfg, name, good)
        _check_graph_ppr(cfg)
        setattr(cfg, knob, False)
    cfg.engine_link_rank_ppr_baseline, cfg.engine_link_rank_ks = True, (1, 0)
    with pytest.raises(ValueError, match="GraphPprRankEval: every K must be a positive integer"):
        GraphGAN.evaluation(g)
    cfg.engine_link_rank_ppr_baseline, cfg.engine_rec_ppr_baseline, cfg.engine_rec_ks = False, True, (2, 300)
    with pytest.raises(ValueError, match=r"GraphPprRecEval: every K must lie in \[1, 256\]"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)
    _check_graph_ppr(types.SimpleNamespace())  # the knobs absent: nothing to check
    _check_graph_ppr(types.SimpleNamespace(engine_rec_ppr_baseline=False, engine_ppr_alpha=7.0))


def test_command_line_on_the_host(gp, lh, tmp_path, capsys):
    from graphgan_amd import recommend
    n, e = small_graph()
    tfile, out, nodes_file = str(tmp_path / "train.txt"), str(tmp_path / "rec.tsv"), str(tmp_path / "ids.txt")
    np.savetxt(tfile, e, fmt="%d")
    n_file = int(e.max()) + 1
    N = ref.neighbor_sets(n_file, e)
    assert recommend.main(["--train", tfile, "--out", out, "--host", "--k", "4", "--index", "ppr"]) == 0  # the defaults: 0.15, 1e-4, 200
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    want = []
    for u in range(n_file):
        if N[u]:
            col, score, _ = ref.topk(N, u, 4, 9830, 109951163, 200, True)
            want += [[str(u), str(c), repr(s / 2.0 ** 40)] for c, s in zip(col, score) if c >= 0]
    assert rows == want and len(rows) > n_file
    assert capsys.readouterr().out.strip() == "nodes=%d lines=%d index=ppr k=4" % (sum(1 for s in N if s), len(want))
    with open(nodes_file, "w") as f:
        f.write("7\n3\n7\n")
    assert recommend.main(["--train", tfile, "--out", out, "--host", "--nodes", nodes_file, "--index", "ppr", "--alpha", "0.5", "--eps", "6.103515625e-05",
                           "--max-rounds", "3"]) == 0
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    want = []
    for u in (7, 3, 7):
        col, score, _ = ref.topk(N, u, 10, 32768, 1 << 26, 3, True)
        want += [[str(u), str(c), repr(s / 2.0 ** 40)] for c, s in zip(col, score) if c >= 0]
    assert rows == want and rows
    for bad in (["--index", "ppr", "--alpha", "1.0"], ["--index", "ppr", "--eps", "0.5"], ["--index", "ppr", "--eps", "1e-13"], ["--index", "ppr", "--max-rounds", "0"],
                ["--index", "pa"], ["--index", "katz"]):
        with pytest.raises(SystemExit):
            recommend.main(["--train", tfile, "--out", out, "--host"] + bad)
    assert recommend.main(["--train", tfile, "--out", out, "--host", "--alpha", "7"]) == 0  # (the parameters belong to ppr alone)
