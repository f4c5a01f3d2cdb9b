"""Full-ranking link evaluation (gg_rank_scores / Engine.rank) and the LinkRankEval evaluator on the device.

fp32 is checked EXACTLY: the reference of a query (u, v) is the oracle's fp32 score row of u (orc.c_all_score_rows with zero
bias: the k-ordered fmaf chain of the matrix-core kernel) and the definition -- rank = 1 + the candidates c != v with
s(u, c) > s(u, v), or s(u, c) == s(u, v) and c < v; candidates: every node, or every node but u and its training neighbours,
and always v -- so rank, n_cand and the bits of score must all be equal.  bf16 is checked against fp64 numpy on the
bf16-rounded table (a band per query) and, bit for bit, against the top-K stream of the same precision."""
import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def _bf16_round(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, like v_cvt_pk_bf16_f32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _nbr_sets(rowptr, col):
    return [set(col[rowptr[v]:rowptr[v + 1]].tolist()) for v in range(len(rowptr) - 1)]


def _graph(ga, n, seed):
    """power-law graph with duplicated adjacency entries (a few edges listed twice); below 64 nodes a ring with chords"""
    if n >= 64:
        edges = ga.synth_powerlaw(n, 3, seed, seed + 1)
    else:
        rs = np.random.RandomState(seed)
        ring = [(i, (i + 1) % n) for i in range(n)]
        chords = [(a, b) for a, b in rs.randint(0, n, size=(n, 2)).tolist() if a != b]
        edges = np.array(ring + chords, dtype=np.int32)
    edges = np.concatenate([edges, edges[:: max(1, len(edges) // 40)]])
    return ga.edges_to_csr(n, edges)


def oracle_rows(E, rows):
    return orc.c_all_score_rows(orc.pad_rows(E), np.zeros(E.shape[0], np.float32), np.ascontiguousarray(rows, dtype=np.int32))


def ref_rank(S, u, v, nbrs=None):
    """The definition on score rows S [len(u), n] (row i belongs to u[i]; any float dtype) -> rank, n_cand, score."""
    n = S.shape[1]
    cols = np.arange(n)
    rank, n_cand = np.zeros(len(u), np.int64), np.zeros(len(u), np.int64)
    score = np.zeros(len(u), S.dtype)
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        s = S[i]
        cand = np.ones(n, dtype=bool)
        if nbrs is not None:
            cand[a] = False
            if nbrs[a]:
                cand[list(nbrs[a])] = False
        cand[b] = True
        ahead = (s > s[b]) | ((s == s[b]) & (cols < b))
        rank[i], n_cand[i], score[i] = 1 + int((ahead & cand).sum()), int(cand.sum()), s[b]
    return rank, n_cand, score


def assert_exact(res, want):
    assert np.array_equal(res["rank"], want[0]), np.flatnonzero(res["rank"] != want[0])[:5]
    assert np.array_equal(res["n_cand"], want[1]), np.flatnonzero(res["n_cand"] != want[1])[:5]
    assert np.array_equal(res["score"].view(np.uint32), want[2].astype(np.float32).view(np.uint32))


def _queries(rs, n, m, nbrs):
    """random pairs, and among them: u == v, targets that are training neighbours, a repeated query"""
    u = rs.randint(0, n, m).astype(np.int32)
    v = rs.randint(0, n, m).astype(np.int32)
    v[0] = u[0]
    for i in range(1, m, 7):
        if nbrs[u[i]]:
            v[i] = sorted(nbrs[u[i]])[i % len(nbrs[u[i]])]
    if m > 60:
        u[5], v[5] = u[60], v[60]
    return u, v


@pytest.mark.parametrize("d", [1, 36, 50, 64, 72, 128])
@pytest.mark.parametrize("n", [3, 31, 32, 33, 127, 128, 129, 257, 1000])
def test_rank_fp32_exact_against_the_oracle(ga, n, d):
    """every boundary of the plan: partial 32-row and 128-column tiles, one and several column splits, a partial k-chunk
    (d = 36, 72), both models, both exclude values; m = 1, 31, 32, 33, 100 are prefixes of one query list"""
    rs = np.random.RandomState(1000 * d + n)
    Eg = (rs.randn(n, d) * 0.5).astype(np.float32)
    Ed = (rs.randn(n, d) * 0.3).astype(np.float32)
    rowptr, col = _graph(ga, n, 7)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(Eg, Ed)
    eng.set_graph_csr(rowptr, col)
    u, v = _queries(rs, n, 100, nbrs)
    assert any(b in nbrs[a] for a, b in zip(u.tolist(), v.tolist()))
    for which, E in ((0, Eg), (1, Ed)):
        S = oracle_rows(E, u)
        for exclude in (False, True):
            want = ref_rank(S, u, v, nbrs if exclude else None)
            for m in (1, 31, 32, 33, 100) if which == 0 else (100,):
                res = eng.rank(u[:m], v[:m], which=which, exclude=exclude)
                assert res["rank"].dtype == np.int32 and res["rank"].shape == (m,) and res["kernel_ms"] > 0
                assert_exact(res, tuple(w[:m] for w in want))
            assert res["rank"][5] == res["rank"][60] and (res["rank"] >= 1).all() and (res["rank"] <= res["n_cand"]).all()
    eng.close()


def test_rank_more_queries_than_one_pass(ga):
    """the queries are processed in internal passes of 4 096: with 4 097 the second pass holds one query, and it -- like every
    other -- equals the same query issued alone"""
    n, d, m = 300, 20, 4097
    rs = np.random.RandomState(4)
    E = (rs.randn(n, d) * 0.4).astype(np.float32)
    rowptr, col = _graph(ga, n, 3)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    u, v = _queries(rs, n, m, nbrs)
    S = oracle_rows(E, u)
    for exclude in (False, True):
        res = eng.rank(u, v, exclude=exclude)
        assert_exact(res, ref_rank(S, u, v, nbrs if exclude else None))
        for lo, hi in ((4096, 4097), (4000, 4097), (0, 40)):
            alone = eng.rank(u[lo:hi], v[lo:hi], exclude=exclude)
            for k in ("rank", "n_cand"):
                assert np.array_equal(alone[k], res[k][lo:hi])
            assert np.array_equal(alone["score"].view(np.uint32), res["score"][lo:hi].view(np.uint32))
    eng.close()


def test_rank_partial_counts_of_the_column_splits_add_up(ga):
    """8 queries on 5 000 nodes: one row tile, so the columns are split over 40 workgroups whose counts must add up"""
    n, d = 5000, 16
    rs = np.random.RandomState(6)
    E = (rs.randn(n, d) * 0.4).astype(np.float32)
    rowptr, col = _graph(ga, n, 5)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    u, v = _queries(rs, n, 8, nbrs)
    u[2] = int(np.argmax(np.diff(rowptr)))  # the largest hub: its list spans several iterations of the gathered-column kernel
    S = oracle_rows(E, u)
    for exclude in (False, True):
        res = eng.rank(u, v, exclude=exclude)
        assert_exact(res, ref_rank(S, u, v, nbrs if exclude else None))
        assert res["rank"].max() > 1000  # (poorly ranked targets: every split contributes)
    eng.close()


def test_rank_ties_are_decided_by_the_column(ga):
    """small-integer table (entries in {-1, 0, 1}, 8 columns): most scores tie and every sum is exact"""
    n, d = 700, 8
    rs = np.random.RandomState(11)
    E = rs.randint(-1, 2, size=(n, d)).astype(np.float32)
    rowptr, col = _graph(ga, n, 9)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    u, v = _queries(rs, n, 100, nbrs)
    S = oracle_rows(E, u)
    assert np.array_equal(S, (E[u].astype(np.int64) @ E.T.astype(np.int64)).astype(np.float32))
    tied = (S == S[np.arange(100), v][:, None]).sum(axis=1)
    assert np.median(tied) > 50  # the condition on the input: a target ties with dozens of columns
    for exclude in (False, True):
        assert_exact(eng.rank(u, v, exclude=exclude), ref_rank(S, u, v, nbrs if exclude else None))
    eng.close()


def test_rank_all_zero_table_gives_the_closed_form(ga):
    n, d = 333, 12
    E = np.zeros((n, d), np.float32)
    rowptr, col = _graph(ga, n, 2)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    rs = np.random.RandomState(3)
    u, v = _queries(rs, n, 100, nbrs)
    res = eng.rank(u, v)
    assert np.array_equal(res["rank"], v + 1) and (res["n_cand"] == n).all() and (res["score"] == 0).all()
    res = eng.rank(u, v, exclude=True)
    for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        elig = [c for c in range(n) if c != a and c not in nbrs[a] and c != b]
        assert res["rank"][i] == 1 + sum(1 for c in elig if c < b) and res["n_cand"][i] == len(elig) + 1
    eng.close()


def test_rank_negative_and_positive_zero_tie(ga):
    """rows of +t, their negated copies and zero rows with t^2 below the fp32 range: every product underflows to a signed zero,
    so the chain from +0.0 ends at -0.0 for (+t, -t) -- all 8 products are -0 -- and at +0.0 elsewhere.  The two zeros must
    tie: every rank is decided by the column.  (The oracle's rows add a zero bias, which turns -0.0 into +0.0, so the expected
    bits are written down here; the oracle confirms that every score is a zero.)"""
    n, d = 300, 8
    t = np.float32(1e-30)
    E = np.zeros((n, d), np.float32)
    E[0::3] = t
    E[1::3] = -t
    sign = np.sign(E[:, 0])
    eng = ga.Engine(E, E)
    rs = np.random.RandomState(8)
    u, v = rs.randint(0, n, 64).astype(np.int32), rs.randint(0, n, 64).astype(np.int32)
    assert not oracle_rows(E, u).any()
    S = np.where(sign[u][:, None] * sign[None, :] < 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    want = ref_rank(S, u, v)
    assert set(want[2].view(np.uint32).tolist()) == {0x00000000, 0x80000000}  # the condition on the input: both zeros are targets
    res = eng.rank(u, v)
    assert_exact(res, want)
    assert np.array_equal(res["rank"], v + 1)
    eng.close()


@pytest.mark.parametrize("prec,d", [("fp32", 50), ("fp32", 128), ("bf16", 50), ("bf16", 128), ("bf16", 260)])
def test_rank_is_the_position_in_the_topk_list(ga, prec, d):
    """for every query with an eligible target: rank <= 256 if and only if topk(k = 256) holds v at position rank - 1 of row u,
    with the same score bits -- both precisions, exactly (the threshold is the stream's own number)"""
    n = 1000
    rs = np.random.RandomState(d)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    rowptr, col = _graph(ga, n, 13)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    rows = rs.randint(0, n, 48).astype(np.int32)
    for exclude in (False, True):
        top = eng.topk(rows, k=256, precision=prec, exclude=exclude)
        # targets: entries of the row's own list (head, middle, tail) and random columns (mostly outside the list)
        ri = np.repeat(np.arange(len(rows)), 8)
        v = np.concatenate([np.r_[top["col"][i, [0, 1, 100, 254, 255]], rs.randint(0, n, 3)] for i in range(len(rows))]).astype(np.int32)
        u = rows[ri]
        elig = np.array([not exclude or (b != a and b not in nbrs[a]) for a, b in zip(u.tolist(), v.tolist())])
        assert elig.sum() > 300 and (v >= 0).all()
        res = eng.rank(u, v, precision=prec, exclude=exclude)
        n_in = 0
        for i in np.flatnonzero(elig):
            r, lst = int(res["rank"][i]), top["col"][ri[i]]
            pos = np.flatnonzero(lst == v[i])
            if r <= 256:
                assert lst[r - 1] == v[i], (i, r, pos)
                assert res["score"][i:i + 1].view(np.uint32)[0] == top["score"][ri[i], r - 1:r].view(np.uint32)[0]
                n_in += 1
            else:
                assert len(pos) == 0, (i, r, pos)
        assert n_in >= 5 * len(rows) and n_in < elig.sum()  # both sides of the boundary occur
    eng.close()


@pytest.mark.parametrize("d", [50, 128, 260])
def test_rank_bf16_inside_the_band_of_fp64_on_the_rounded_table(ga, d):
    """every query: the rank lies between the count of columns surely ahead and the count of columns possibly ahead, with the
    project's bf16 score tolerance 2e-3 max(1, max |S|); n_cand is exact"""
    n, m = 1000, 100
    rs = np.random.RandomState(3 * d)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    rowptr, col = _graph(ga, n, 9)
    nbrs = _nbr_sets(rowptr, col)
    eng = ga.Engine(E, E * np.float32(0.5))
    eng.set_graph_csr(rowptr, col)
    u, v = _queries(rs, n, m, nbrs)
    for which, T in ((0, E), (1, E * np.float32(0.5))):
        Eb = _bf16_round(T).astype(np.float64)
        S = Eb[u] @ Eb.T
        tol = 2e-3 * max(1.0, np.abs(S).max())
        for exclude in (False, True):
            res = eng.rank(u, v, which=which, precision="bf16", exclude=exclude)
            _, want_cand, want_score = ref_rank(S, u, v, nbrs if exclude else None)
            assert np.array_equal(res["n_cand"], want_cand)
            assert np.max(np.abs(res["score"] - want_score)) <= tol
            for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
                cand = np.ones(n, dtype=bool)
                if exclude:
                    cand[[a] + list(nbrs[a])] = False
                lo = 1 + int((cand & (S[i] > S[i, b] + tol)).sum())
                cand[b] = False
                hi = 1 + int((cand & (S[i] >= S[i, b] - tol)).sum())
                assert lo <= res["rank"][i] <= hi, (i, lo, int(res["rank"][i]), hi)
    eng.close()


def test_rank_argument_errors(ga):
    E = np.ones((50, 8), np.float32)
    eng = ga.Engine(E, E)
    with pytest.raises(ga.GraphGANHipError) as ei:
        eng.rank([0], [1], exclude=True)  # no graph
    assert ei.value.code == ga.GG_EINVAL and "gg_rank_scores" in str(ei.value) and "gg_set_graph_csr" in str(ei.value)
    for u, v, text in (([0, 3, 50], [1, 2, 3], "u[2] = 50"), ([0, 3], [1, -1], "v[1] = -1")):
        with pytest.raises(ga.GraphGANHipError) as ei:
            eng.rank(u, v)
        assert ei.value.code == ga.GG_EINVAL and "gg_rank_scores" in str(ei.value) and text in str(ei.value)
    for bad in (dict(which=2), dict(precision="fp16")):
        with pytest.raises(ValueError):
            eng.rank([0], [1], **bad)
    with pytest.raises(ValueError):
        eng.rank([0, 1], [1])
    assert eng.rank([], [])["rank"].shape == (0,)
    res = eng.rank([0, 7], [7, 0])  # the engine stays usable: all scores tie at 8
    assert res["rank"].tolist() == [8, 1] and res["n_cand"].tolist() == [50, 50] and res["score"].tolist() == [8.0, 8.0]
    eng.close()
    # precision = 1 with n_emb > 512: gg_rank_scores refuses it like gg_topk_scores, but no engine gets that far -- gg_create
    # itself refuses a table wider than 512 with GG_EINVAL, so the refusal a caller meets is that one
    wide = np.ones((40, 520), np.float32)
    with pytest.raises(ga.GraphGANHipError) as ei:
        ga.Engine(wide, wide)
    assert ei.value.code == ga.GG_EINVAL and "n_emb=520" in str(ei.value)
    widest = np.ones((40, 512), np.float32)
    eng = ga.Engine(widest, widest)
    for prec in ("fp32", "bf16"):  # the widest table there is: all scores tie at 512
        res = eng.rank([0, 5], [1, 0], precision=prec)
        assert res["rank"].tolist() == [2, 1] and res["score"].tolist() == [512.0, 512.0]
    eng.close()


def test_link_rank_evaluator_on_ca_grqc(ga, tmp_path):
    """engine path == the host pipeline on ranks from the oracle's fp32 rows: the same results line, the same integer
    statistics, float means equal under == (float64 arithmetic on equal integers)"""
    from graphgan_amd.evaluation import link_ranking as lr
    d, n, graph = load_ca_grqc()
    tr, te = str(tmp_path / "train.txt"), str(tmp_path / "test.txt")
    for path, key in ((tr, "train"), (te, "test")):
        with open(path, "w") as f:
            f.writelines("%d\t%d\n" % (a, b) for a, b in d[key].tolist())
    emb = ca_grqc_init_embeddings(d, n).astype(np.float32)
    rowptr, col = ga.edges_to_csr(n, d["train"])
    eng = ga.Engine(emb, emb * np.float32(0.5))
    eng.set_graph_csr(rowptr, col)
    ks = (1, 10, 100, 1000)
    ev = lr.LinkRankEval("unused", tr, te, n, 50, engine=eng, which=0, ks=ks)
    pairs = lr.edge_pairs(te)
    assert len(pairs) == 2 * len(d["test"])
    dev_ranks = ev.pair_ranks(pairs)
    want_ranks, _, _ = ref_rank(oracle_rows(emb, pairs[:, 0]), pairs[:, 0], pairs[:, 1], _nbr_sets(rowptr, col))
    assert np.array_equal(dev_ranks, want_ranks)
    dev = ev.eval_link_ranking()
    # the host fallback's own code on the oracle's fp32 rows (float64 scoring may break a tie differently)
    host_ranks = lr.host_rank(lambda nodes: oracle_rows(emb, nodes), pairs[:, 0], pairs[:, 1], n, lr.train_csr(d["train"], n))[0]
    fd, fh = lr.filtered_ranks(pairs[:, 0], pairs[:, 1], dev_ranks), lr.filtered_ranks(pairs[:, 0], pairs[:, 1], host_ranks)
    assert int(fd.sum()) == int(fh.sum()) and all(int((fd <= K).sum()) == int((fh <= K).sum()) for K in ks)
    host = lr.summarize(fh, ks)
    assert dev == host and dev["n"] == len(pairs)
    assert lr.format_results("gen", dev, ks) == lr.format_results("gen", host, ks)
    assert 0.0 < dev["mrr"] <= 1.0 and dev["hits"][1] <= dev["hits"][1000] <= 1.0
    f64 = lr.LinkRankEval("unused", tr, te, n, 50, emd=emb.astype(np.float64), ks=ks).eval_link_ranking()
    print("engine fp32: %r\nhost float64: %r" % (dev, f64))
    assert f64["n"] == dev["n"]
    eng.close()
