"""Graphs and references of the neighbour-sum sweep and label-spreading tests (tests/test_gpu_label_spread.py,
tests/test_label_propagation_cpu.py).  Everything here restates the definitions of include/graphgan_hip.h ("neighbour-sum sweep")
in numpy on the DIRECTED PAIR SET of the graph -- (v, w) for every w in N(v) -- and uses none of the package's code."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32
CHUNK = 512     # == Engine.NEIGHBOR_SUM_CHUNK (asserted by the tests)
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 129)  # distinct degrees of the probes: every lane-group count (1 .. 64) and one past it
HUB_A, HUB_B = 3 * CHUNK + 17, 4 * CHUNK + 5    # both sides of every chunk edge


def pair_set(n, edges):
    """edge list -> (src, dst) int64 of the pairs (v, w), w in N(v): distinct, without v itself, sorted by (v, w)"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    return key // n, key % n


def neighbor_sum(n, src, dst, X, in_scale=None, out_scale=None):
    """out[v] = out_scale[v] * sum over w in N(v) of in_scale[w] * X[w], in X's dtype (int64: exact; float64: the reference)"""
    X = np.asarray(X)
    G = X if in_scale is None else X * np.asarray(in_scale, dtype=X.dtype)[:, None]
    H = np.zeros((n, X.shape[1]), dtype=X.dtype)
    np.add.at(H, src, G[dst])
    return H if out_scale is None else H * np.asarray(out_scale, dtype=X.dtype)[:, None]


def degrees(n, src):
    return np.bincount(src, minlength=n)


def hub_graph(seed=0):
    """One graph for the sweep's shapes: a pool of HUB_B nodes (0 .. HUB_B - 1); probe j = pool + j has LENGTHS[j] distinct pool
    neighbours; hub A (HUB_A pool neighbours, a random subset) and hub B (the whole pool: its sorted list is 0, 1, 2, ..., so list
    position = node id); a few pool-pool edges; duplicated edges in both orientations, self-loops (also on a hub and a probe) and
    one isolated last node.  -> (n, edges int32 [E, 2], dict(pool, probes, hub_a, hub_b, isolated, a_list))"""
    rs = np.random.RandomState(seed)
    pool = HUB_B
    probes = pool + np.arange(len(LENGTHS))
    hub_a, hub_b, isolated = pool + len(LENGTHS), pool + len(LENGTHS) + 1, pool + len(LENGTHS) + 2
    n = isolated + 1
    edges = [(int(p), int(x)) for p, k in zip(probes, LENGTHS) for x in rs.permutation(pool)[:k]]
    a_list = np.sort(rs.permutation(pool)[:HUB_A])
    edges += [(hub_a, int(x)) for x in a_list]
    edges += [(int(x), hub_b) for x in range(pool)]
    edges += [(int(a), int(b)) for a, b in rs.randint(0, pool, size=(300, 2))]
    e = np.array(edges, dtype=np.int32)
    dup = e[rs.permutation(len(e))[:400]]
    loops = np.repeat(np.concatenate([rs.randint(0, pool, 20), [hub_a, probes[3]]]), 2).reshape(-1, 2)
    e = np.concatenate([e, dup[:200], dup[200:, ::-1], loops]).astype(np.int32)
    return n, e[rs.permutation(len(e))], dict(pool=pool, probes=probes, hub_a=hub_a, hub_b=hub_b, isolated=isolated, a_list=a_list)


def circulant(n=257, steps=(1, 5)):
    """i ~ i +- 1, i +- 5 (mod 257): 4-regular, so s = 1 / sqrt(4) = 0.5 exactly"""
    i = np.arange(n)
    return np.concatenate([np.stack([i, (i + d) % n], axis=1) for d in steps]).astype(np.int32)


def planted_partition(seed, n=256, blocks=4, p_in=0.2, p_out=0.01, n_train=26):
    """256 nodes, block of node i = i mod 4, an edge with probability p_in inside a block and p_out between blocks, RandomState(seed);
    then 26 training nodes from the same stream.  -> (edges int32, labels int64 [n], train int64 [n_train], test int64)"""
    rs = np.random.RandomState(seed)
    lab = np.arange(n) % blocks
    iu, ju = np.triu_indices(n, 1)
    keep = rs.random_sample(len(iu)) < np.where(lab[iu] == lab[ju], p_in, p_out)
    edges = np.stack([iu[keep], ju[keep]], axis=1).astype(np.int32)
    perm = rs.permutation(n)
    return edges, lab.astype(np.int64), np.sort(perm[:n_train]), np.sort(perm[n_train:])


def coefficients(deg, alpha):
    """s, a, b as the header states them: float64, rounded once to fp32"""
    d = np.asarray(deg, dtype=np.float64)
    with np.errstate(divide="ignore"):
        s = np.where(d >= 1, 1.0 / np.sqrt(d), 0.0).astype(np.float32)
        a = np.where(d >= 1, alpha / np.sqrt(d), 0.0).astype(np.float32)
    return s, a, np.float32(1.0 - alpha)


def one_hot(n, train, Y):
    """Y0 float64 [n, C] from the training nodes and their label matrix bool [m, C]"""
    Y0 = np.zeros((n, Y.shape[1]), dtype=np.float64)
    Y0[train] = Y
    return Y0


def label_spread(n, src, dst, Y0, alpha, iters, band=False):
    """The float64 recursion on the fp32-rounded coefficients: F_T, and with ``band`` the bound E_T on |fp32 device F_T - F_T|
        E' = a (A (s E)) (1 + (deg + 2) u) + u ((deg + 2) a (A |s F|) + |F'|),  E_0 = 0
    (the error carried through the sweep, plus (deg + 2) roundings of the sum of deg products scaled by a, plus the final add)."""
    deg = degrees(n, src)
    s, a, b = (np.asarray(x, dtype=np.float64) for x in coefficients(deg, alpha))
    F, E = Y0.copy(), np.zeros_like(Y0)
    base = b * Y0
    g = (deg + 2.0)[:, None]
    for _ in range(iters):
        Fn = a[:, None] * neighbor_sum(n, src, dst, F, in_scale=s) + base
        if band:
            E = a[:, None] * neighbor_sum(n, src, dst, E, in_scale=s) * (1 + g * U) \
                + U * (g * a[:, None] * neighbor_sum(n, src, dst, np.abs(F), in_scale=s) + np.abs(Fn))
        F = Fn
    return (F, E) if band else F


def dense_S(n, src, dst, alpha):
    """(S with the fp32-rounded coefficients: alpha S = diag(a) A diag(s), as float64 matrices) -> (A, aAs, b)"""
    A = np.zeros((n, n))
    A[src, dst] = 1.0
    s, a, b = (np.asarray(x, dtype=np.float64) for x in coefficients(degrees(n, src), alpha))
    return A, a[:, None] * A * s[None, :], float(b)
