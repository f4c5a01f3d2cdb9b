"""The normative restatement of the push sweep (include/graphgan_hip.h, "push sweep") in Python dicts, sets and ints, for
tests/test_gpu_ppr.py and tests/test_graph_ppr_cpu.py.  Written from the header's text; it uses none of the package's code and no
numpy arithmetic.  ``push`` is instrumented: the pushes, the sum of deg over the pushes, the touched nodes and the per-push error
terms the float64 comparison needs.  The order, the eligibility and the two result shapes are two_hop_ref's, on the dense row p."""
from tests.support import two_hop_ref as th

ONE = 1 << 40
neighbor_sets = th.neighbor_sets


def bounds(n, alpha_q, eps_q):
    """-> (kmin, B, E) of the header"""
    kmin = (eps_q * alpha_q) >> 16
    assert kmin >= 1
    B = ONE // kmin
    return kmin, B, min(n, 1 + B)


def push(N, u, alpha_q, eps_q, max_rounds):
    """-> dict(p, r: {node: int}, rounds, converged, residual, pushes, sum_deg, touched (set), err_terms: per push (deg, rem, delta)
    with delta = (r0 * alpha_q) mod 2^16, the bits the shift drops)"""
    assert 1 <= alpha_q <= 65535 and 1 <= eps_q <= 1 << 32 and alpha_q * eps_q >= 65536 and max_rounds >= 1
    p, r = {}, {u: ONE}
    touched = {u}
    rounds = pushes = sum_deg = 0
    err_terms = []

    def active():
        return sorted(x for x, rx in r.items() if rx > 0 and rx >= eps_q * max(len(N[x]), 1))

    A = active()
    while A and rounds < max_rounds:
        start = {x: r[x] for x in A}  # the values at the START of the round
        for x in A:
            r[x] = 0
        for x in A:
            r0, deg = start[x], len(N[x])
            keep = (r0 * alpha_q) >> 16 if deg else r0
            rest = r0 - keep
            share = rest // deg if deg else 0
            rem = rest - share * deg
            p[x] = p.get(x, 0) + keep
            r[x] += rem
            for w in N[x]:
                r[w] = r.get(w, 0) + share
                touched.add(w)
            pushes += 1
            sum_deg += deg
            err_terms.append((deg, rem, (r0 * alpha_q) & 0xFFFF if deg else 0))
        rounds += 1
        assert sum(p.values()) + sum(r.values()) == ONE
        A = active()
    return dict(p=p, r=r, rounds=rounds, converged=int(not A), residual=sum(r.values()), pushes=pushes, sum_deg=sum_deg, touched=touched, err_terms=err_terms)


def dense_row(N, u, alpha_q, eps_q, max_rounds):
    """-> (p as a list over all nodes, the push's dict)"""
    res = push(N, u, alpha_q, eps_q, max_rounds)
    row = [0] * len(N)
    for x, px in res["p"].items():
        row[x] = px
    return row, res


def topk(N, u, k, alpha_q, eps_q, max_rounds, exclude=True, row=None):
    """-> (cols [k] padded with -1, scores [k] padded with 0, n_pos)"""
    row = dense_row(N, u, alpha_q, eps_q, max_rounds)[0] if row is None else row
    return th.topk(N, u, k, None, exclude, row=row)


def rank(N, u, v, alpha_q, eps_q, max_rounds, exclude=True, row=None):
    """-> dict(rank, n_cand, score, ahead, n_pos, pos_below)"""
    row = dense_row(N, u, alpha_q, eps_q, max_rounds)[0] if row is None else row
    return th.rank(N, u, v, None, exclude, row=row)
