"""The normative restatement of the neighbour-mode sweep, label propagation and the partition edge counts
(include/graphgan_hip.h, "neighbour-mode sweep") in Python dicts, sets and ints, for tests/test_gpu_communities.py and
tests/test_graph_communities_cpu.py.  Written from the header's text; it uses none of the package's code and no numpy arithmetic."""
import numpy as np

M32 = 0xFFFFFFFF


def fmix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def neighbor_sets(n, edges):
    """N(v): the distinct neighbours of v other than v, from an edge list with duplicates and self-loops"""
    N = [set() for _ in range(n)]
    for u, v in np.asarray(edges).reshape(-1, 2).tolist():
        if u != v:
            N[u].add(v)
            N[v].add(u)
    return N


def mode_of(N, labels, v, salt=0, keep=True):
    own = labels[v]
    if not N[v]:
        return own
    cnt = {}
    for w in N[v]:
        cnt[labels[w]] = cnt.get(labels[w], 0) + 1
    cmax = max(cnt.values())
    if keep and cnt.get(own, 0) == cmax:
        return own
    return min((fmix32(l ^ salt), l) for l, c in cnt.items() if c == cmax)[1]


def neighbor_mode(N, labels, salt=0, keep=True, nodes=None):
    labels = [int(x) for x in labels]
    rows = range(len(N)) if nodes is None else [int(x) for x in nodes]
    return [mode_of(N, labels, v, salt, keep) for v in rows]


def side_state(seed, t):
    return fmix32(((seed & M32) ^ 0x85EBCA6B) + 0x9E3779B9 * t)


def salt_of(seed, t, h):
    return fmix32((seed & M32) + 0x9E3779B9 * (2 * (t - 1) + h + 1))


def label_propagation(N, seed=0, max_iters=100):
    """-> (labels, iters, converged, changed list)"""
    n = len(N)
    L = list(range(n))
    changed, t, converged = [], 0, False
    while t < max_iters and not converged:
        t += 1
        st = side_state(seed, t)
        moved = 0
        for h in (0, 1):
            salt = salt_of(seed, t, h)
            new = [mode_of(N, L, v, salt, True) if (fmix32(v ^ st) & 1) == h else L[v] for v in range(n)]
            moved += sum(1 for a, b in zip(new, L) if a != b)
            L = new
        changed.append(moved)
        converged = moved == 0
    return L, t, converged, changed


def partition_edges(N, assign, n_label):
    assign = [int(x) for x in assign]
    intra, tot = [0] * n_label, [0] * n_label
    for v, c in enumerate(assign):
        if c < 0:
            continue
        for w in N[v]:
            if assign[w] >= 0:
                tot[c] += 1
                if assign[w] == c:
                    intra[c] += 1
    return intra, tot


def modularity(intra, tot):
    m2 = sum(tot)
    if m2 == 0:
        return float("nan")
    q = 0.0
    for i, t in zip(intra, tot):
        q += i / m2 - (t / m2) ** 2
    return q


def relabel(labels):
    ids = {}
    for v, l in enumerate(labels):  # (ascending v: a community is numbered when its smallest member is met)
        ids.setdefault(int(l), len(ids))
    return [ids[int(l)] for l in labels], len(ids)


def ladder_graph(cap, seed=0):
    """The degree-ladder graph of tests/support/label_spread_ref.hub_graph -- probes with 0, 1, 2, 3, 4, 5, 63, 64, 65 and 129 distinct
    neighbours, hubs of 3 x 512 + 17 and 4 x 512 + 5, duplicates, self-loops, an isolated node -- with further probes of 15, 16 and
    17 neighbours and one hub of ``cap`` + 37 neighbours (above the workgroup table's capacity), all into a pool of ``cap`` + 100 extra
    nodes appended behind it.  -> (n, edges int32, info)"""
    from tests.support import label_spread_ref as ls
    n0, e0, info = ls.hub_graph(seed)
    rs = np.random.RandomState(seed + 77)
    pool2 = n0 + np.arange(cap + 100)
    extra = {}
    nxt = n0 + len(pool2)
    edges = []
    for name, k in (("p15", 15), ("p16", 16), ("p17", 17), ("giant", cap + 37)):
        extra[name] = nxt
        edges += [(nxt, int(x)) for x in rs.permutation(pool2)[:k]]
        nxt += 1
    edges += [(extra["giant"], extra["giant"])] * 2 + edges[:20]  # (a self-loop and duplicates on the new lists too)
    e = np.concatenate([e0, np.array(edges, dtype=np.int32)]).astype(np.int32)
    return nxt, e[rs.permutation(len(e))], dict(info, **extra)
