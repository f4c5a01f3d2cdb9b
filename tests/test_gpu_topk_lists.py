"""The top-K consumer (gg_topk_scores / Engine.topk) on FULL per-wavefront lists, at every k edge of wave_insert's four
registers per lane, in every tile instance, and on tables smaller than k -- exactly, in fp32 and in bf16.

The tables are programmed (tests/support/topk_shapes.py): every score is an integer that both precisions compute exactly, so the
float64 product ranked by lexsort((column, -score)) is the reference for both, bf16 must equal fp32 bit for bit, and there is no
tolerance anywhere: columns and score bits are compared with array_equal.  4 096 requested rows -- the query nodes and a few
ordinary nodes, with repeats -- give long column splits; tests/test_topk_shapes_cpu.py shows, in a model of the lists, that the
row programs then insert into full lists at the head, at k - 1, across the 64-entry register boundaries, and pass tau without
entering, and that the k best columns of the homed programs all come out of ONE wavefront's list, so that every position of
that list is in the answer."""
import numpy as np
import pytest

from tests.support import topk_shapes as ts

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def long_case(ga):
    """the long table written for k = 256; the reference ranked once at k = 256"""
    c = ts.case(ts.N_LONG, ts.D_LONG, ts.K_LONG)
    eng = ga.Engine(c["E"], c["E"])
    yield dict(c, eng=eng, ref={u: ts.ref_topk(c["S"][u], ts.MAX_K) for u in c["ids"].tolist()})
    eng.close()


def assert_rows(res, rows, k, want):
    """want: {id: (col [>= k], score [>= k])}; every repeat of an id gives the same row, and that row is the reference's"""
    assert res["col"].shape == res["score"].shape == (len(rows), k)
    bits = res["score"].view(np.uint32)
    for u in np.unique(rows).tolist():
        at = np.flatnonzero(rows == u)
        assert (res["col"][at] == res["col"][at[0]]).all() and (bits[at] == bits[at[0]]).all(), u
        wc, wsc = want[u][0][:k], want[u][1][:k]
        assert np.array_equal(res["col"][at[0]], wc), (u, np.flatnonzero(res["col"][at[0]] != wc)[:5], res["col"][at[0]][:8], wc[:8])
        assert ts.bits_equal(res["score"][at[0]], wsc), u


def assert_same(a, b):
    assert np.array_equal(a["col"], b["col"]) and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32))


def _run_case(ga, c, k):
    eng = ga.Engine(c["E"], c["E"])
    want = {u: ts.ref_topk(c["S"][u], k) for u in c["ids"].tolist()}
    res = {p: eng.topk(c["rows"], k=k, precision=p) for p in PRECISIONS}
    eng.close()
    for p in PRECISIONS:
        assert_rows(res[p], c["rows"], k, want)
    assert_same(res["fp32"], res["bf16"])


@pytest.mark.parametrize("k", ts.KS_LONG)
def test_topk_long_lists_at_every_k_edge(ga, long_case, k):
    """24 576 columns in 8 to 16 splits: every wavefront fills its list and goes on inserting for at least 2 k more columns.
    The table written for k = 256 at every k (the reference is ranked once at 256, its prefixes are the answers), and the
    table written for this k: there the k best columns of `tail`, `head`, `asc` and `perm` all come out of ONE wavefront's
    list, so every position of that list -- k - 1 and the ones behind a 64-entry boundary included -- is in the answer"""
    c = long_case
    res = {p: c["eng"].topk(c["rows"], k=k, precision=p) for p in PRECISIONS}
    for p in PRECISIONS:
        assert_rows(res[p], c["rows"], k, c["ref"])
    assert_same(res["fp32"], res["bf16"])
    _run_case(ga, ts.case(ts.N_LONG, ts.D_LONG, k), k)


@pytest.mark.parametrize("n,d,k", ts.INSTANCE_CASES)
def test_topk_full_lists_in_every_tile_instance(ga, n, d, k):
    """KS = 4, 8, 16, 32 of the bf16 stream; the fp32 stream with its dynamic LDS just under 48 KB (d = 380) and above it
    (d = 384, 512: the raised limit); a partial last split"""
    _run_case(ga, ts.case(n, d, k), k)


@pytest.mark.parametrize("k", ts.EXCLUDE_KS)
def test_topk_exclusion_on_a_full_list(ga, k):
    """q_asc is linked to every other one of the last 600 columns of its home wavefront -- the best ones of its row --,
    q_plateau to every other member of its plateaus: a half-wave's candidates mix eligible and excluded columns while the list
    is full"""
    c = ts.case(ts.N_LONG, ts.D_LONG, k)
    rowptr, col = ga.edges_to_csr(c["n"], ts.exclusion_edges(c))
    nbrs = {u: set(col[rowptr[u]:rowptr[u + 1]].tolist()) for u in c["ids"].tolist()}
    want = {u: ts.ref_topk(c["S"][u], k, ts.eligibility(c["n"], u, nbrs[u])) for u in c["ids"].tolist()}
    eng = ga.Engine(c["E"], c["E"])
    eng.set_graph_csr(rowptr, col)
    res = {p: eng.topk(c["rows"], k=k, precision=p, exclude=True) for p in PRECISIONS}
    eng.close()
    for p in PRECISIONS:
        assert_rows(res[p], c["rows"], k, want)
        for name in ("asc", "plateau"):
            u = c["q"][name]
            row = res[p]["col"][np.flatnonzero(c["rows"] == u)[0]]
            assert not (set(row.tolist()) & (nbrs[u] | {u})) and -1 not in row
    assert_same(res["fp32"], res["bf16"])


def _ring(ga, n):
    return ga.edges_to_csr(n, np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int32))


@pytest.mark.parametrize("n", [3, 33, 129])
def test_topk_small_tables_and_k_beyond_the_table(ga, n):
    """entries in {-1, 0, 1}: every score is a small integer and most tie.  k = 1, n - 1, n, n + 1 and 256: a row has n columns
    (n - 3 eligible ones on a ring; none at n = 3), the rest of the list is -1 / -inf"""
    d = 12
    rs = np.random.RandomState(n)
    E = rs.randint(-1, 2, size=(n, d)).astype(np.float32)
    S = ts.gram_rows(E, np.arange(n))
    rowptr, col = _ring(ga, n)
    elig = {u: ts.eligibility(n, u, set(col[rowptr[u]:rowptr[u + 1]].tolist())) for u in range(n)}
    assert all(int(e.sum()) == max(0, n - 3) for e in elig.values())
    eng = ga.Engine(E, E)
    eng.set_graph_csr(rowptr, col)
    some = rs.randint(0, n, 50).astype(np.int32)
    for k in sorted({1, n - 1, n, n + 1, 256}):
        for exclude in (False, True):
            want = {u: ts.ref_topk(S[u], k, elig[u] if exclude else None) for u in range(n)}
            n_real = min(k, max(0, n - 3) if exclude else n)
            assert all(int((w[0] >= 0).sum()) == n_real and np.isneginf(w[1][n_real:]).all() for w in want.values())
            res = {}
            for p in PRECISIONS:
                res[p] = eng.topk(None, k=k, precision=p, exclude=exclude)
                assert_rows(res[p], np.arange(n), k, want)
                assert_rows(eng.topk(some, k=k, precision=p, exclude=exclude), some, k, want)
            assert_same(res["fp32"], res["bf16"])
    eng.close()


def test_topk_signed_zeros_tie(ga):
    """the table of test_rank_negative_and_positive_zero_tie: every product underflows to a signed zero, -0 counts as +0, so
    all scores tie and every row is the columns 0 .. k - 1 with score +0"""
    n, d = 300, 8
    t = np.float32(1e-30)
    E = np.zeros((n, d), np.float32)
    E[0::3] = t
    E[1::3] = -t
    eng = ga.Engine(E, E)
    rows = np.array([0, 1, 2, 150, 298, 299, 1], dtype=np.int32)
    for p in PRECISIONS:
        for k in (1, 100, 256):
            for r in (rows, None):
                res = eng.topk(r, k=k, precision=p)
                assert np.array_equal(res["col"], np.tile(np.arange(k, dtype=np.int32), (len(res["col"]), 1))), (p, k)
                assert not res["score"].view(np.uint32).any(), (p, k)
    eng.close()


def test_topk_runs_at_the_widest_table(ga):
    """d = 512 is the widest table gg_create accepts, so the checks `bf16 supports n_emb <= 512` and `fp32 supports
    n_emb <= 1116` of gg_topk_scores can never refuse a call; both precisions run there"""
    E = np.ones((40, 512), np.float32)
    eng = ga.Engine(E, E)
    for p in PRECISIONS:
        res = eng.topk([0, 39], k=3, precision=p)
        assert res["col"].tolist() == [[0, 1, 2]] * 2 and res["score"].tolist() == [[512.0] * 3] * 2
    eng.close()
    wide = np.ones((40, 513), np.float32)
    with pytest.raises(ga.GraphGANHipError) as ei:
        ga.Engine(wide, wide)
    assert ei.value.code == ga.GG_EINVAL and "n_emb=513" in str(ei.value)
