"""The normative restatement of the two-hop pair sweep (include/graphgan_hip.h, "two-hop pair sweep") in Python sets, lists and ints,
for tests/test_gpu_two_hop_pairs.py and tests/test_graph_pairs_cpu.py.  Written from the header's text on two_hop_ref.dense_row; it
uses none of the package's code and no numpy arithmetic: EVERY candidate pair, sorted in the total order, and the head read off."""
from tests.support import two_hop_ref as ref


def candidates(N, nodes=None, weights=None, exclude=True, rows=None):
    """every candidate (u, v, S(u, v)) in the order score descending, (u, v) ascending.  rows: dense_row of every node, if the
    caller has them"""
    n = len(N)
    members = list(range(n)) if nodes is None else [int(x) for x in nodes]
    assert all(a < b for a, b in zip(members, members[1:])) and all(0 <= x < n for x in members)
    inside = set(members)
    out = []
    for u in members:
        row = ref.dense_row(N, u, weights) if rows is None else rows[u]
        reached = set().union(*(N[w] for w in N[u])) if N[u] else set()  # (S(u, c) > 0 only there)
        for c in reached:
            if c > u and row[c] > 0 and c in inside and not (exclude and c in N[u]):
                out.append((-row[c], u, c))
    out.sort()
    return [(u, c, -s) for s, u, c in out]


def head(cand, k):
    """the output of a request for k pairs from the sorted candidates -> (u [k], v [k], score [k], n_found), padded with -1, -1, 0"""
    top = cand[:k]
    pad = k - len(top)
    return [t[0] for t in top] + [-1] * pad, [t[1] for t in top] + [-1] * pad, [t[2] for t in top] + [0] * pad, len(top)


def top_pairs(N, k, nodes=None, weights=None, exclude=True, rows=None):
    return head(candidates(N, nodes, weights, exclude, rows), k)


def upper_expansion(N, u):
    """T'(u): the entries the restricted fill visits"""
    return sum(1 for w in N[u] for c in N[w] if c > u)
