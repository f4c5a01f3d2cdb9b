"""Top-K under a metric and over a candidate set on the device (graphgan_amd/csrc/topk_score.hip: gg_topk_metric, Engine.topk with
``metric`` / ``candidates`` / ``exclude="self"``) and the k-NN results lines.

Exact answers.  The contract (include/graphgan_hip.h) fixes every operation, so wherever each of them is exact the device must
return the float64 definition bit for bit, in both precisions:
  l2      entries in {-1, 0, 1}: s and h are small integers, t = s - h / 2 a half-integer, the squared distance an integer; the
          table is exact in bf16.  Reference: int64 h_u + h_c - 2 s with lexsort((col, dist2)).  Ties are frequent.
  cosine  rows with exactly 0, 1, 4, 16 or 64 entries of +-1: w is 0, 1, 1/2, 1/4 or 1/8 and s w_c, t w_u are exact.
On a Gaussian table fp32 is bit-exact against a numpy float32 restatement on the oracle's score rows (h = their diagonal; 0.5 h
and 2 t are exact, so each fmaf is ONE rounding of an exact float64 difference; float32 sqrt and division are correctly rounded
in numpy), and bf16 lies inside a band derived from the inputs (``bf16_band``).

Shapes.  N in {1, 31, 129, 4 100, 9 000} x d in {8, 50, 128, 512}: one block, a ragged last tile, several 128-column splits
(1, 31, 33 requested rows: lists that never fill), every width instance of both streams; 4 096 rows with repeats on N = 24 576:
few long splits and full lists, as tests/support/topk_shapes.LONG_CASES."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.support import topk_shapes as ts
from tests.support.allpairs_shapes import bf16_round

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def raw_metric(ga, eng, rows, k, which=0, precision=0, metric=0, exclude=0, cand=None, n_cand=None):
    """gg_topk_metric itself (Engine.topk sends the dot metric without a set to gg_topk_scores) -> (rc, col, score)"""
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    n_rows = eng.n_node if rows is None else len(rows)
    cand = None if cand is None else np.ascontiguousarray(cand, dtype=np.int32)
    col = np.full((n_rows, k if 1 <= k <= 256 else 1), -7, dtype=np.int32)
    score = np.zeros(col.shape, dtype=np.float32)
    rc = ga._lib.lib.gg_topk_metric(eng._ctx, which, P(rows), n_rows, k, precision, metric, exclude, P(cand),
                                    (0 if cand is None else len(cand)) if n_cand is None else n_cand, P(col), P(score), None)
    return rc, col, score


# ---- references ----------------------------------------------------------------------------------------------------------------
def ref_lists(T, V, k, elig=None, pad=-np.inf):
    """per row: the first k eligible columns by (T descending, column ascending), reported with V -> (col int32, value float32);
    with a tuple of k: {k: (col, value)} from ONE sort per row"""
    ks = (k,) if np.isscalar(k) else tuple(k)
    R, n = T.shape
    out = {kk: (np.full((R, kk), -1, dtype=np.int32), np.full((R, kk), pad, dtype=np.float32)) for kk in ks}
    for i in range(R):
        cols = np.arange(n) if elig is None else np.flatnonzero(elig[i])
        o = cols[np.lexsort((cols, -(T[i, cols] + 0.0)))[:max(ks)]]
        for kk, (col, val) in out.items():
            m = min(kk, len(o))
            col[i, :m], val[i, :m] = o[:m], V[i, o[:m]]
    return out[k] if np.isscalar(k) else out


_f64 = {}


def ref_exact(E, rows, k, metric, elig=None):
    """the float64 definition on a table where every operation is exact (k: one k or a tuple, as ref_lists)"""
    if id(E) not in _f64:
        _f64.clear()  # (one table at a time)
        E64 = np.asarray(E, dtype=np.float64)
        _f64[id(E)] = (E, E64, (E64 * E64).sum(axis=1))
    _, E64, h = _f64[id(E)]
    S = E64[rows] @ E64.T + 0.0
    if metric == "l2":
        d2 = (h[rows][:, None] + h[None, :] - 2.0 * S).astype(np.int64)  # the int64 reference: ascending distance, then column
        assert np.array_equal(d2, h[rows][:, None] + h[None, :] - 2.0 * S) and d2.min() >= 0
        return ref_lists(-d2.astype(np.float64), d2.astype(np.float64), k, elig, pad=np.inf)
    if metric == "cosine":
        w = np.where(h > 0, 1.0 / np.sqrt(np.where(h > 0, h, 1.0)), 0.0)
        assert set(np.unique(w).tolist()) <= {0.0, 1.0, 0.5, 0.25, 0.125}
        T = S * w[None, :]
        return ref_lists(T, T * w[rows][:, None], k, elig)
    return ref_lists(S, S, k, elig)


def assert_bits(got_col, got_score, want, what):
    assert np.array_equal(got_col, want[0]), (what, np.argwhere(got_col != want[0])[:5])
    assert ts.bits_equal(got_score, want[1]), (what, np.argwhere(got_score != want[1])[:5])


def sparse_sign_table(n, d, seed):
    """rows with exactly 0, 1, 4, 16 or 64 entries of +-1 (as many of these counts as fit d); nodes 0 and n - 1 and a few more are
    zero rows"""
    rs = np.random.RandomState(seed)
    counts = [c for c in (0, 1, 4, 16, 64) if c <= d]
    E = np.zeros((n, d), dtype=np.float32)
    nz = rs.randint(0, len(counts), size=n)
    nz[[0, n - 1]] = 0
    for i in range(n):
        at = rs.permutation(d)[:counts[nz[i]]]
        E[i, at] = rs.choice([-1.0, 1.0], size=len(at))
    return E


def dense_sign_table(n, d, seed):
    return np.random.RandomState(seed).randint(-1, 2, size=(n, d)).astype(np.float32)


def requested(n, count, seed):
    """`count` rows with repeats, unsorted; the zero rows 0 and n - 1 among them"""
    rows = np.random.RandomState(seed).randint(0, n, size=count).astype(np.int32)
    rows[0] = n - 1
    rows[-1] = 0
    return rows


# ---- exact l2 and cosine on every shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 50, 128, 512])
@pytest.mark.parametrize("n", [1, 31, 129, 4100, 9000])
def test_exact_l2_and_cosine_on_integer_tables(ga, n, d):
    Es, Ed = sparse_sign_table(n, d, 7 * n + d), dense_sign_table(n, d, 3 * n + d)
    assert np.array_equal(bf16_round(Es), Es) and np.array_equal(bf16_round(Ed), Ed)
    eng = ga.Engine(Es, Ed)  # which = 0: the sparse table (power-of-4 norms), which = 1: the dense one (l2 only)
    for n_rows in (1, 31, 33):
        rows = requested(n, n_rows, n + n_rows)
        want = {(w, m, k): ref for w, E, ms in ((0, Es, ("cosine", "l2")), (1, Ed, ("l2",))) for m in ms
                for k, ref in ref_exact(E, rows, (1, 64, 65, 256), m).items()}
        for (which, metric, k), ref in want.items():
            for precision in ("fp32", "bf16"):
                res = eng.topk(rows, k, which=which, precision=precision, metric=metric)
                assert_bits(res["col"], res["score"], ref, (n, d, n_rows, which, metric, k, precision))
                if n > 1 and k == 65:
                    res = eng.topk(rows, k, which=which, precision=precision, metric=metric, exclude="self")
                    elig = np.arange(n)[None, :] != rows[:, None]
                    assert_bits(res["col"], res["score"], ref_exact((Es, Ed)[which], rows, k, metric, elig), ("self", n, d, which, metric, precision))
    eng.close()


@pytest.mark.parametrize("k", [64, 256])
def test_exact_l2_and_cosine_on_long_splits_and_full_lists(ga, k):
    n, d = ts.N_LONG, ts.D_LONG
    splits, cps = ts.topk_plan(n, ts.N_ROWS, k)
    assert ts.max_cols_per_wave(n, cps) >= 3 * k  # long splits: every wavefront's list fills and keeps changing
    Es, Ed = sparse_sign_table(n, d, 5), dense_sign_table(n, d, 6)
    ids = np.array([0, 1, 31, 32, n // 2 + 1, n - 2, n - 1], dtype=np.int32)
    rs = np.random.RandomState(k)
    rows = ids[rs.randint(0, len(ids), size=ts.N_ROWS)]
    rows[:len(ids)] = ids[::-1]
    at = {int(v): i for i, v in enumerate(ids)}
    pick = np.array([at[int(v)] for v in rows])
    eng = ga.Engine(Es, Ed)
    for which, E, metrics in ((0, Es, ("cosine", "l2")), (1, Ed, ("l2",))):
        for metric in metrics:
            wc, wv = ref_exact(E, ids, k, metric)
            for precision in ("fp32", "bf16"):
                res = eng.topk(rows, k, which=which, precision=precision, metric=metric)
                assert_bits(res["col"], res["score"], (wc[pick], wv[pick]), (which, metric, k, precision))
    eng.close()


# ---- the dot metric is gg_topk_scores -------------------------------------------------------------------------------------------
def test_dot_metric_equals_gg_topk_scores_bit_for_bit(ga):
    c = ts.case(ts.N_INST, 128, 65)
    rowptr, col = ga.edges_to_csr(c["n"], ts.exclusion_edges(c))
    rs = np.random.RandomState(1)
    for E in (c["E"], (rs.randn(c["n"], 128) * 0.5).astype(np.float32)):  # the programmed table and a Gaussian one
        eng = ga.Engine(E, E)
        eng.set_graph_csr(rowptr, col)
        rows = c["rows"][:257]
        for precision in (0, 1):
            for exclude in (0, 1):
                old = eng.topk(rows, 65, precision=("fp32", "bf16")[precision], exclude=bool(exclude))
                rc, got_col, got_score = raw_metric(ga, eng, rows, 65, precision=precision, metric=0, exclude=exclude)
                assert rc == 0
                assert np.array_equal(got_col, old["col"]) and ts.bits_equal(got_score, old["score"]), (precision, exclude)
        eng.close()


# ---- fp32 on a Gaussian table: the float32 restatement --------------------------------------------------------------------------
def f32_restatement(S_rows, h, rows, k, metric, elig=None):
    """S_rows float32 [R, n] (the oracle's chain), h float32 [n] (its diagonal): the contract's operations in numpy float32"""
    S_rows, h = np.asarray(S_rows, dtype=np.float32), np.asarray(h, dtype=np.float32)
    if metric == "cosine":
        w = np.where(h == 0, np.float32(0), np.float32(1) / np.sqrt(np.where(h == 0, np.float32(1), h))).astype(np.float32)
        T = S_rows * w[None, :]
        assert T.dtype == np.float32
        return ref_lists(T, T * w[rows][:, None], k, elig)
    # s - 0.5 h and h - 2 t: differences of float32 values of like magnitude are exact in float64, so astype is the fmaf's rounding
    T = (S_rows.astype(np.float64) - 0.5 * h.astype(np.float64)[None, :]).astype(np.float32)
    V = np.maximum(np.float32(0), (h.astype(np.float64)[rows][:, None] - 2.0 * T.astype(np.float64)).astype(np.float32))
    return ref_lists(T, V, k, elig, pad=np.inf)


@pytest.mark.parametrize("n,d", [(1029, 50), (700, 256)])
def test_fp32_gaussian_against_the_float32_restatement(ga, n, d):
    rs = np.random.RandomState(n + d)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    E[5] = 0.0  # a zero row
    S = orc.c_all_score_rows(orc.pad_rows(E), np.zeros(n, np.float32), np.arange(n, dtype=np.int32))
    h = np.diagonal(S).copy()
    rows = requested(n, 97, 4)
    rows[3] = 5
    cand = np.unique(np.concatenate([[0, 31, 32, n - 1, 5], rs.permutation(n)[:n // 3]])).astype(np.int32)
    member = np.zeros(n, dtype=bool)
    member[cand] = True
    eng = ga.Engine(E, E)
    for metric in ("cosine", "l2"):
        for k in (1, 10, 65, 256):
            res = eng.topk(rows, k, metric=metric)
            assert_bits(res["col"], res["score"], f32_restatement(S[rows], h, rows, k, metric), (metric, k))
            mono = np.diff(res["score"].astype(np.float64), axis=1)
            assert np.all(mono >= 0) if metric == "l2" else np.all(mono <= 0)
        elig = member[None, :] & (np.arange(n)[None, :] != rows[:, None])
        res = eng.topk(rows, 65, metric=metric, exclude="self", candidates=cand)
        assert_bits(res["col"], res["score"], f32_restatement(S[rows], h, rows, 65, metric, elig), (metric, "set"))
    res = eng.topk(None, 10, metric="cosine", exclude="self")  # rows == NULL: every node, and each node's nearest other nodes
    assert_bits(res["col"], res["score"], f32_restatement(S, h, np.arange(n), 10, "cosine", ~np.eye(n, dtype=bool)), "all rows")
    eng.close()


# ---- bf16 on a Gaussian table: a band derived from the inputs ---------------------------------------------------------------------
def bf16_band(Eb, rows, metric):
    """Worst-case |device value - float64 value| per (row, column) on the bf16-rounded table Eb (float64), eps = 2^-23 per
    operation (twice the unit roundoff: no assumption on how the matrix instruction rounds its partial sums), g = d eps / (1 - d eps):
      s      d products, exact in fp32 (8 x 8 significant bits), summed in fp32 in any order:  |ds| <= g A,  A = sum |x_ui x_ci|
      h      the fmaf chain of d terms:                                                       |dh| <= g h
      cosine w = 1 / sqrt(h): relative error g / 2 (h) + eps (sqrt) + eps (division) =: ew;  t = fl(s w_c), value = fl(t w_u):
             |dv| <= w_u w_c (g A + |s| (2 ew + 2 eps))
      l2     t = fl(s - h_c / 2):  |dt| <= g A + g h_c / 2 + eps |t|;   value = max(0, fl(h_u - 2 t)):
             |dv| <= g h_u + 2 |dt| + eps |v|
    times 1.001 for the products of these terms (each below 1e-4).  -> (float64 value, float64 ordering value t, band), each [R, n]"""
    d = Eb.shape[1]
    eps = 2.0 ** -23
    g = d * eps / (1 - d * eps)
    S = Eb[rows] @ Eb.T
    A = np.abs(Eb[rows]) @ np.abs(Eb).T
    h = (Eb * Eb).sum(axis=1)
    if metric == "cosine":
        w = np.where(h > 0, 1.0 / np.sqrt(np.where(h > 0, h, 1.0)), 0.0)
        ew = g / 2 + 2 * eps
        T = S * w[None, :]
        return T * w[rows][:, None], T, 1.001 * w[rows][:, None] * w[None, :] * (g * A + np.abs(S) * (2 * ew + 2 * eps))
    T = S - 0.5 * h[None, :]
    V = np.maximum(0.0, h[rows][:, None] - 2.0 * T)
    dt = g * A + 0.5 * g * h[None, :] + eps * np.abs(T)
    return V, T, 1.001 * (g * h[rows][:, None] + 2 * dt + eps * V)


ERRTOL = []  # "case err/tol" lines of this run; written to $GG_TOPK_METRIC_ERRTOL when that names a file


@pytest.mark.parametrize("n,d", [(1029, 50), (3000, 128), (700, 256), (600, 300), (129, 512), (300, 8)])
def test_bf16_gaussian_inside_the_derived_band(ga, n, d):
    rs = np.random.RandomState(2 * n + d)
    E = (rs.randn(n, d) * 0.5).astype(np.float32)
    E[5] = 0.0
    Eb = bf16_round(E).astype(np.float64)
    rows = requested(n, 97, 9)
    rows[3] = 5
    cand = np.unique(np.concatenate([[0, 31, 32, n - 1, 5], rs.permutation(n)[:n // 2]])).astype(np.int32)
    member = np.zeros(n, dtype=bool)
    member[cand] = True
    eng = ga.Engine(E, E)
    for metric in ("cosine", "l2"):
        V, T, band = bf16_band(Eb, rows, metric)
        sign = -1.0 if metric == "l2" else 1.0  # in "larger is better" terms: sign * value
        for k, elig in ((1, None), (65, None), (256, None), (65, member[None, :] & (np.arange(n)[None, :] != rows[:, None]))):
            res = eng.topk(rows, k, precision="bf16", metric=metric, **({} if elig is None else dict(exclude="self", candidates=cand)))
            col, score = res["col"], res["score"].astype(np.float64)
            e = np.ones((len(rows), n), dtype=bool) if elig is None else np.broadcast_to(elig, (len(rows), n))
            worst = 0.0
            for i in range(len(rows)):
                m = min(k, int(e[i].sum()))
                c = col[i, :m]
                assert np.all(col[i, m:] == -1) and np.all(score[i, m:] == -sign * np.inf)
                assert len(set(c.tolist())) == m and c.min(initial=0) >= 0 and np.all(e[i, c])       # distinct and eligible
                err = np.abs(score[i, :m] - V[i, c])
                worst = max(worst, float(np.max(np.divide(err, band[i, c], out=np.zeros(m), where=band[i, c] > 0), initial=0.0)))
                assert np.all(err <= band[i, c]), (metric, k, i, float(err.max()))                   # each score belongs to its column
                assert np.all(np.diff(sign * score[i, :m]) <= 0)                                     # ordered
                if m:
                    best = np.sort(sign * V[i, e[i]])[::-1]
                    b = float(band[i, e[i]].max())
                    assert sign * V[i, c[-1]] >= best[m - 1] - 2 * b, (metric, k, i)                  # the k-th is (nearly) the true k-th
            line = "bf16 %s n=%d d=%d k=%d %s err/tol=%.4f" % (metric, n, d, k, "all" if elig is None else "set+self", worst)
            print(line)
            ERRTOL.append(line)
    eng.close()
    out = os.environ.get("GG_TOPK_METRIC_ERRTOL")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(ERRTOL) + "\n")


# ---- candidate sets and the three exclusions ---------------------------------------------------------------------------------------
def test_candidate_sets_on_exact_tables(ga):
    n, d = 4100, 50
    Es, Ed = sparse_sign_table(n, d, 21), dense_sign_table(n, d, 22)
    rows = requested(n, 33, 2)
    rows[1:5] = [31, 32, 0, n - 1]
    rs = np.random.RandomState(3)
    some = rs.permutation(n)[:900].astype(np.int32)
    sets = dict(edges=np.array([0, 31, 32, n - 1], dtype=np.int32),                      # members at tile edges; fewer than k
                repeated=np.concatenate([some, some[::3], [0, 31, 32, n - 1, 0, 0]]).astype(np.int32),
                single=np.array([32], dtype=np.int32),
                empty=np.zeros(0, dtype=np.int32))
    eng = ga.Engine(Es, Ed)
    for name, cand in sets.items():
        member = np.zeros(n, dtype=bool)
        member[cand] = True
        for which, E, metric in ((0, Es, "cosine"), (0, Es, "dot"), (1, Ed, "l2")):
            for exclude, elig in ((False, np.broadcast_to(member, (len(rows), n))), ("self", member[None, :] & (np.arange(n)[None, :] != rows[:, None]))):
                for k in (1, 65):
                    want = ref_exact(E, rows, k, metric, elig)
                    for precision in ("fp32", "bf16"):
                        res = eng.topk(rows, k, which=which, precision=precision, metric=metric, exclude=exclude, candidates=cand)
                        assert_bits(res["col"], res["score"], want, (name, metric, exclude, k, precision))
                        if name == "empty":
                            assert np.all(res["col"] == -1) and np.all(res["score"] == (np.inf if metric == "l2" else -np.inf))
                        if name == "edges" and k == 65:
                            assert np.all(res["col"][:, 4:] == -1) and set(res["col"][:, :3].ravel().tolist()) <= {0, 31, 32, n - 1}
    eng.close()


def test_an_ineligible_column_never_raises_tau(ga):
    """The best columns of the programmed rows `asc` (every tile beats the whole list) and `plateau` (more than k columns share
    the k-th score) are taken out of the candidate set -- or are training neighbours, or both.  Had one of them entered a list it
    would have raised the list's threshold and an eligible column would be missing from the answer."""
    c = ts.case(ts.N_INST, 128, 65)
    n, k = c["n"], 65
    edges = ts.exclusion_edges(c)
    nb = ts.neighbour_sets(n, edges)
    rowptr, col = ga.edges_to_csr(n, edges)
    q_asc, q_pl = c["q"]["asc"], c["q"]["plateau"]
    out = np.zeros(n, dtype=bool)     # not candidates: the other half of what exclusion_edges links, and a stride of everything else
    home = ts.wave_columns(n, c["cps"])[c["home"][c["prog"]["asc"]]][-600:]
    out[home[0::2]] = True
    out[np.flatnonzero((c["F"][c["prog"]["plateau"]] >= ts.PLATEAU_KTH) & c["ordinary"])[1::2]] = True
    out[5::7] = True
    cand = np.flatnonzero(~out).astype(np.int32)
    rows = np.array([q_asc, q_pl, 1, q_asc, n - 1, q_pl] + c["ids"].tolist(), dtype=np.int32)
    eng = ga.Engine(c["E"], c["E"])
    eng.set_graph_csr(rowptr, col)
    for exclude in (False, True, "self"):
        elig = np.stack([(~out) & (ts.eligibility(n, int(u), nb[int(u)]) if exclude is True else
                                   (np.arange(n) != u) if exclude == "self" else np.ones(n, dtype=bool)) for u in rows])
        want_cols, want_scores = zip(*[ts.ref_topk(c["S"][int(u)], k, elig[i]) for i, u in enumerate(rows)])
        want = (np.stack(want_cols), np.stack(want_scores))
        for precision in ("fp32", "bf16"):
            res = eng.topk(rows, k, precision=precision, exclude=exclude, candidates=cand)
            assert_bits(res["col"], res["score"], want, (exclude, precision))
            assert not out[res["col"][res["col"] >= 0]].any()
    # and without a set: exclude="self" alone drops the query node's own 65 537
    res = eng.topk(rows, k, exclude="self")
    want_cols, want_scores = zip(*[ts.ref_topk(c["S"][int(u)], k, np.arange(n) != u) for u in rows])
    assert_bits(res["col"], res["score"], (np.stack(want_cols), np.stack(want_scores)), "self alone")
    assert not np.any(res["col"] == rows[:, None]) and res["score"][:2].max() < ts.SELF
    eng.close()


# ---- determinism, refusals, the results lines -----------------------------------------------------------------------------------------
def test_runs_are_equal_bit_for_bit(ga):
    rs = np.random.RandomState(12)
    n = 4100
    E = (rs.randn(n, 50) * 0.5).astype(np.float32)
    rows = requested(n, 300, 1)
    cand = rs.permutation(n)[:2000].astype(np.int32)
    eng = ga.Engine(E, E)
    for metric in ("dot", "cosine", "l2"):
        for precision in ("fp32", "bf16"):
            a = eng.topk(rows, 100, precision=precision, metric=metric, exclude="self", candidates=cand)
            b = eng.topk(rows, 100, precision=precision, metric=metric, exclude="self", candidates=cand[::-1].copy())
            assert np.array_equal(a["col"], b["col"]) and ts.bits_equal(a["score"], b["score"])
            part = eng.topk(rows[40:50], 100, precision=precision, metric=metric, exclude="self", candidates=cand)  # another launch plan
            assert np.array_equal(a["col"][40:50], part["col"]) and ts.bits_equal(a["score"][40:50], part["score"])
    eng.close()


def test_every_refusal_names_gg_topk_metric(ga):
    n = 700
    E = np.random.RandomState(0).randn(n, 50).astype(np.float32)
    eng = ga.Engine(E, E)  # no graph
    rows = np.array([3, 4, 5], dtype=np.int32)
    lib, ctx = ga._lib.lib, eng._ctx
    assert raw_metric(ga, eng, rows, 5, metric=1, exclude=2, cand=np.array([1, 2], dtype=np.int32))[0] == 0
    for kwargs, text in ((dict(k=0), r"k = 0 outside \[1, 256\]"), (dict(k=257), r"k = 257 outside \[1, 256\]"),
                         (dict(metric=3), r"metric must be 0 \(dot\), 1 \(cosine\) or 2 \(l2\)"), (dict(metric=-1), r"metric must be 0"),
                         (dict(exclude=3), r"exclude must be 0, 1 \(self and training neighbours\) or 2 \(self\)"), (dict(exclude=-1), r"exclude must be"),
                         (dict(exclude=1), r"exclude = 1 needs the training graph"),
                         (dict(precision=2), r"precision must be 0 \(fp32\) or 1 \(bf16\)"), (dict(which=2), r"which must be 0 \(generator\) or 1"),
                         (dict(rows=np.array([3, n, -1], dtype=np.int32)), r"rows\[1\] = 700 out of range \[0, 700\)"),
                         (dict(rows=np.array([-2, n], dtype=np.int32)), r"rows\[0\] = -2 out of range \[0, 700\)"),
                         (dict(cand=np.array([0, 5, n, -1], dtype=np.int32)), r"cand_nodes\[2\] = 700 out of range \[0, 700\)"),
                         (dict(cand=np.array([-1], dtype=np.int32)), r"cand_nodes\[0\] = -1 out of range \[0, 700\)"),
                         (dict(cand=np.array([1], dtype=np.int32), n_cand=-1), r"n_cand = -1 is negative")):
        rc, col, _ = raw_metric(ga, eng, **dict(dict(rows=rows, k=5), **kwargs))
        assert rc == ga.GG_EINVAL, text
        msg = lib.gg_last_error(ctx).decode()
        assert msg.startswith("gg_topk_metric: ") and re.search(text, msg), (text, msg)
        assert np.all(col == -7)  # nothing was launched, nothing written
    # (bf16 with n_emb > 512 is refused with "bf16 supports n_emb <= 512", but no engine gets that far: gg_create refuses the width)
    for kwargs, text in ((dict(metric="manhattan"), "metric must be"), (dict(exclude="neighbours"), "exclude must be"), (dict(k=0), "k must be"),
                         (dict(precision="fp16"), "precision must be"), (dict(which=2), "which must be")):
        with pytest.raises(ValueError, match="topk: " + text):
            eng.topk(rows, **dict(dict(k=5), **kwargs))
    with pytest.raises(ga._lib.GraphGANHipError, match=r"gg_topk_metric: cand_nodes\[1\] = 700"):
        eng.topk(rows, 5, metric="cosine", candidates=[0, n])
    with pytest.raises(ga._lib.GraphGANHipError, match="gg_topk_metric: exclude = 1 needs the training graph"):
        eng.topk(rows, 5, metric="l2", exclude=True)
    eng.close()


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_knn_lines_with_an_engine_equal_the_float64_host_lines(ga, tmp_path, metric):
    """an integer table with power-of-4 norms: the device's neighbours ARE the float64 evaluator's, so the lines are equal strings"""
    from graphgan_amd.evaluation import node_knn
    from graphgan_amd.graph_gan import GraphGAN
    from tests.test_link_prediction_lr_cpu import _layout
    cfg, g, n = _layout(tmp_path, "link_prediction")
    d = cfg.n_emb
    rs = np.random.RandomState(8)
    labelled = np.sort(rs.permutation(n)[:1500])
    y = rs.randint(0, 5, size=n)
    tables = []
    for seed in (31, 32):  # class-dependent supports, so that the vote means something; norms stay powers of 4
        E = sparse_sign_table(n, d, seed)
        for v in labelled[::2]:
            E[v] = 0.0
            E[v, 4 * y[v]:4 * y[v] + 4] = 1.0
        tables.append(E)
    cfg.labels_filename = str(tmp_path / "labels.txt")
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d\t%d\n" % (v, y[v]) for v in labelled)
    eng = ga.Engine(tables[0], tables[1])
    for i in range(2):
        eng.write_embeddings(i, cfg.emb_filenames[i])
    cfg.engine_nc_knn, cfg.engine_knn_k, cfg.engine_knn_metric = True, 7, metric
    host = GraphGAN.evaluation(g)
    assert [ln.split(":")[0] for ln in host] == ["gen", "dis", "gen_knn", "dis_knn"]
    for precision in ("fp32", "bf16"):
        cfg.engine_knn_precision = precision
        dev = GraphGAN.evaluation(types.SimpleNamespace(config=cfg, engine=eng, n_node=n, seed=0))
        assert dev[2:] == host[2:], (precision, dev[2:], host[2:])
    for i, line in enumerate(host[2:]):
        res = node_knn.NodeKnnEval(cfg.labels_filename, n, d, emd=tables[i].astype(np.float64), k=7, metric=metric, seed=0).eval_node_knn()
        assert line == node_knn.format_results(cfg.modes[i], res) and res["n_train"] == 1350 and res["n_test"] == 150
        assert 0.3 < res["acc"] <= 1.0  # half of the labelled nodes carry their class
    eng.close()
