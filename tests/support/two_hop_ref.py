"""The normative restatement of the two-hop sweep (include/graphgan_hip.h, "two-hop sweep") in Python sets, lists and ints, for
tests/test_gpu_two_hop.py and tests/test_graph_ranking_cpu.py.  Written from the header's text; it uses none of the package's code
and no numpy arithmetic: the dense row S(u, .), the total order over ALL nodes, and everything else read off that order."""
import numpy as np


def neighbor_sets(n, edges):
    """N(v): the distinct neighbours of v other than v, from an edge list with duplicates and self-loops"""
    N = [set() for _ in range(n)]
    for u, v in np.asarray(edges).reshape(-1, 2).tolist():
        if u != v:
            N[u].add(v)
            N[v].add(u)
    return N


def dense_row(N, u, weights=None):
    """S(u, c) for every c, as Python ints"""
    row = [0] * len(N)
    for w in N[u]:
        ww = 1 if weights is None else int(weights[w])
        for c in N[w]:
            row[c] += ww
    return row


def excluded(N, u, exclude):
    """exclude: "self" -> {u}; True -> N(u) + {u}"""
    assert exclude is True or exclude == "self"
    return {u} if exclude == "self" else N[u] | {u}


def order_of(row, cand):
    """the candidates in the total order: score descending, column ascending"""
    return sorted(cand, key=lambda c: (-row[c], c))


def topk(N, u, k, weights=None, exclude=True, row=None):
    """-> (cols [k] padded with -1, scores [k] padded with 0, n_pos)"""
    row = dense_row(N, u, weights) if row is None else row
    ex = excluded(N, u, exclude)
    pos = [c for c in order_of(row, [c for c in range(len(N)) if c not in ex]) if row[c] > 0]
    top = pos[:k]
    return top + [-1] * (k - len(top)), [row[c] for c in top] + [0] * (k - len(top)), len(pos)


def rank(N, u, v, weights=None, exclude=True, row=None):
    """-> dict(rank, n_cand, score, ahead, n_pos, pos_below): the target is always a candidate"""
    row = dense_row(N, u, weights) if row is None else row
    ex = excluded(N, u, exclude) - {v}
    cand = [c for c in range(len(N)) if c not in ex]
    others = [c for c in cand if c != v and row[c] > 0]
    return dict(rank=1 + order_of(row, cand).index(v), n_cand=len(cand), score=row[v], n_pos=len(others),
                ahead=sum(1 for c in others if row[c] > row[v] or (row[c] == row[v] and c < v)), pos_below=sum(1 for c in others if c < v))


def expansion(N, u):
    """T(u): the entries the sweep visits"""
    return sum(len(N[w]) for w in N[u])
