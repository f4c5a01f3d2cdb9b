"""The normative restatement of the spanning-forest sweep (include/graphgan_hip.h, "spanning-forest sweep") in Python lists, sets
and ints, for tests/test_gpu_spanning_forest.py and tests/test_split_cpu.py: Kruskal with a union-find over the ascending keys --
NOT the Boruvka rounds of the device and of split.host_spanning_forest.  Written from the header's text; it uses none of the
package's code and no numpy arithmetic.  Also the graphs the two test files share."""
import numpy as np

from tests.support.communities_ref import fmix32, neighbor_sets  # noqa: F401  (the hash and the sets are those of the header)

SALT = 0x53504C54


def edge_list(N):
    """E = {(a, b) : a < b, b in N(a)} ordered by (a, b)"""
    return [(a, b) for a in range(len(N)) for b in sorted(N[a]) if a < b]


def default_priorities(m, seed):
    s = fmix32((seed & 0xFFFFFFFF) ^ SALT)
    return [fmix32(j ^ s) for j in range(m)]


def kruskal(n, E, prio):
    """-> (forest list [m] of 0 / 1, component list [n] = the smallest id of the node's component, n_components)"""
    root = list(range(n))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    forest = [0] * len(E)
    for _, j in sorted(((int(prio[j]) << 32) | j, j) for j in range(len(E))):
        ra, rb = find(E[j][0]), find(E[j][1])
        if ra != rb:
            root[max(ra, rb)] = min(ra, rb)  # (the smaller id stays the root: a root is its component's smallest id)
            forest[j] = 1
    component = [find(v) for v in range(n)]
    return forest, component, len(set(component))


def forest_of(n, edges, seed=0, prio=None):
    """the restatement on a raw edge list (duplicates, both directions, self-loops) -> (E, forest, component, n_components)"""
    E = edge_list(neighbor_sets(n, edges))
    forest, component, k = kruskal(n, E, default_priorities(len(E), seed) if prio is None else prio)
    return E, forest, component, k


# ---- graphs: (n, int32 edge array)
def path_graph(k):
    """nodes 0 .. k - 1 in a row: edge j is (j, j + 1)"""
    return k, np.stack([np.arange(k - 1), np.arange(1, k)], axis=1).astype(np.int32)


def cycle_graph(k):
    return k, np.array([(i, (i + 1) % k) for i in range(k)], dtype=np.int32)


def complete_graph(k):
    return k, np.array([(a, b) for a in range(k) for b in range(a + 1, k)], dtype=np.int32)


def star_graph(leaves, hub=0):
    n = leaves + 1
    others = [v for v in range(n) if v != hub]
    return n, np.array([(hub, v) for v in others], dtype=np.int32)


def two_hubs(leaves):
    """two stars of ``leaves`` leaves each, their hubs joined"""
    n1, e1 = star_graph(leaves)
    e2 = e1 + n1
    return 2 * n1, np.concatenate([e1, e2, [[0, n1]]]).astype(np.int32)


def triangles(k, isolated):
    """k disjoint triangles, then ``isolated`` nodes without an edge"""
    e = [(3 * t + i, 3 * t + (i + 1) % 3) for t in range(k) for i in range(3)]
    return 3 * k + isolated, np.array(e, dtype=np.int32)


def random_graph(n=70000, pairs=105000, seed=5):
    """``pairs`` drawn pairs on n nodes: duplicates and self-loops among them, thousands of components, isolated nodes"""
    rs = np.random.RandomState(seed)
    return n, rs.randint(0, n, size=(pairs, 2)).astype(np.int32)


def permuted(n, edges, seed=9):
    """the same graph under a random renumbering of its nodes"""
    perm = np.random.RandomState(seed).permutation(n).astype(np.int32)
    return n, perm[np.asarray(edges)]


def ca_grqc_union():
    from tests.helpers import load_ca_grqc
    d, n, _ = load_ca_grqc()
    return n, np.concatenate([np.asarray(d["train"]), np.asarray(d["test"])]).astype(np.int32)
