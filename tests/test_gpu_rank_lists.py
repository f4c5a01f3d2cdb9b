"""The rank consumer (gg_rank_scores / Engine.rank) on the programmed tables of tests/support/topk_shapes.py: exact in fp32
AND in bf16.  Every score is an integer both precisions compute exactly, so rank, n_cand and the bits of score equal the
float64 definition, bf16 equals fp32, and `rank <= k` holds if and only if the top-K list of the same call holds the target at
position rank - 1.  4 096 queries sweep long column splits (16 x 1 536 columns), 40 queries 128-column splits; the targets sit at
the best column, around the k-th place, inside plateaus of equal scores, at the first and last column of every split, at the
query node itself and at an excluded neighbour.  d = 256 runs rank_bf16_kernel<16> and rank_gather_kernel<16>, d = 512 the
widest table and the fp32 kernels' raised LDS limit."""
import numpy as np
import pytest

from tests.support import topk_shapes as ts

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def targets(c, name, k, nbrs):
    """the target columns of the query node of a program, the ones every call must hold first"""
    n, j = c["n"], c["q"][name]
    s = c["S"][j]
    top = ts.ref_topk(s, k + 2)[0]
    top_ex = ts.ref_topk(s, k + 2, ts.eligibility(n, j, nbrs[j]))[0]
    # the best column is j itself; places k, k + 1, k + 2 (without j, under the exclusion: k - 1, k, k + 1); the last column
    v = [top[0], top[k - 1], top[k], top[k + 1], n - 1, top[1], top[k - 2], top_ex[0], top_ex[k - 2], top_ex[k - 1], top_ex[k], int(c["qid"][(c["prog"][name] + 1) % c["P"]])]
    if name == "plateau":                                                       # members of both plateaus
        for val in (ts.PLATEAU_KTH, ts.PLATEAU_TOP):
            members = np.flatnonzero(s == val)
            v += members[[0, 1, len(members) // 2, -2, -1]].tolist() + members[::9].tolist()
    v += sorted(nbrs[j])[:3] + sorted(nbrs[j])[-3:]                                      # excluded neighbours
    for cps in (ts.rank_plan(n, ts.CHUNK)[1], ts.rank_plan(n, 40)[1] * 16, c["cps"]):   # first and last column of the splits
        v += list(range(0, n, cps)) + list(range(cps - 1, n, cps))
    return list(dict.fromkeys(int(x) for x in v))


def queries(c, k, nbrs, m):
    """m queries, unsorted: the targets of the query nodes interleaved -- the first m of them, or all of them, a few of the
    ordinary nodes' and repeats drawn at random"""
    per = [[(c["q"][name], v) for v in targets(c, name, k, nbrs)] for name in c["names"]]
    q = [per[j][i] for i in range(max(len(p) for p in per)) for j in range(c["P"]) if i < len(per[j])]
    q += [(int(u), int(c["S"][int(u)].argmax())) for u in c["ids"][c["P"]:]] + [(int(u), 7) for u in c["ids"][c["P"]:]]  # ordinary nodes
    rs = np.random.RandomState(m)
    pick = np.arange(m) if m < len(q) else np.r_[np.arange(len(q)), rs.randint(0, len(q), m - len(q))]
    q = np.array(q, dtype=np.int32)[rs.permutation(pick)]
    return q[:, 0].copy(), q[:, 1].copy()


@pytest.mark.parametrize("n,d,k", ts.RANK_CASES)
def test_rank_is_exact_in_both_precisions_and_is_the_topk_position(ga, n, d, k):
    c = ts.case(n, d, k)
    rowptr, col = ga.edges_to_csr(n, ts.exclusion_edges(c))
    nbrs = {u: set(col[rowptr[u]:rowptr[u + 1]].tolist()) for u in c["ids"].tolist()}
    assert len(nbrs[c["q"]["asc"]]) >= 144 and len(nbrs[c["q"]["plateau"]]) == 200
    eng = ga.Engine(c["E"], c["E"])
    eng.set_graph_csr(rowptr, col)
    ids = c["ids"]
    for exclude in (False, True):
        elig = {u: ts.eligibility(n, u, nbrs[u]) if exclude else None for u in ids.tolist()}
        top = {p: eng.topk(ids, k=ts.MAX_K, precision=p, exclude=exclude) for p in PRECISIONS}
        row_of = {u: i for i, u in enumerate(ids.tolist())}
        for m in (ts.CHUNK, 40):
            u, v = queries(c, k, nbrs, m)
            assert len(u) == m and set(c["qid"].tolist()) <= set(u.tolist())
            memo = {}
            want = [memo.setdefault((a, b), ts.ref_rank(c["S"][a], b, elig[a])) for a, b in zip(u.tolist(), v.tolist())]
            w_rank, w_cand = np.array([w[0] for w in want]), np.array([w[1] for w in want])
            w_score = np.array([w[2] for w in want], dtype=np.float32)
            # the condition on the input: targets inside and outside the list, at rank 1, k and k + 1, and tied ones
            assert {1, k, k + 1} <= set(w_rank.tolist()) and w_rank.max() > n // 2
            res = {}
            for p in PRECISIONS:
                r = res[p] = eng.rank(u, v, precision=p, exclude=exclude)
                bad = np.flatnonzero(r["rank"] != w_rank)
                assert len(bad) == 0, (p, m, exclude, [(int(u[i]), int(v[i]), int(r["rank"][i]), int(w_rank[i])) for i in bad[:5]])
                assert np.array_equal(r["n_cand"], w_cand) and ts.bits_equal(r["score"], w_score)
                n_in = n_out = 0
                for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
                    if exclude and not elig[a][b]:
                        continue  # (an excluded target is ranked among the candidates, and no list holds it)
                    lst, rk = top[p]["col"][row_of[a]], int(r["rank"][i])
                    if rk <= ts.MAX_K:
                        assert lst[rk - 1] == b and top[p]["score"][row_of[a], rk - 1] == r["score"][i], (p, a, b, rk)
                        n_in += 1
                    else:
                        assert b not in lst, (p, a, b, rk)
                        n_out += 1
                assert n_in > 0 and n_out > 0  # both sides of the boundary occur
            for key in ("rank", "n_cand"):
                assert np.array_equal(res["fp32"][key], res["bf16"][key])
            assert ts.bits_equal(res["fp32"]["score"], res["bf16"]["score"])
    eng.close()
