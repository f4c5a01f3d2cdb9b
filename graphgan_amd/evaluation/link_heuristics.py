"""Neighbourhood link-prediction baselines: the customary yardsticks of the link-prediction literature, computed on the TRAINING
graph alone -- no embedding takes part.  An embedding whose AUC sits below Adamic-Adar has learnt less than the adjacency lists
already say.

For the training graph, N(x) is the neighbour SET of x (distinct neighbours other than x itself: duplicate edges and self-loops
of the file do not count), deg(x) = |N(x)| and C(u, v) = (N(u) & N(v)) \\ {u, v}; u == v follows the formulas with C = N(u).

    cn        |C(u, v)|
    jaccard   cn / (deg(u) + deg(v) - cn) in float64, 0 where the denominator is 0
    pa        deg(u) deg(v) in int64
    aa        sum over w in C of 1 / ln(deg(w))      (Adamic-Adar)
    ra        sum over w in C of 1 / deg(w)          (resource allocation)

``aa`` and ``ra`` are sums of FIXED-POINT node weights (``node_weights``: rint(2^40 / ln(deg)) for deg >= 2, rint(2^40 / deg) for
deg >= 1, else 0; float64 numpy, one function for the device and the host path), added as unsigned 64-bit integers and divided
by 2^40 at the end.  Integer sums are exact and independent of order, so the device (``Engine.pair_neighbors``, gg_pair_neighbors)
and the host (``host_pair_neighbors``) give the same bits; the quantisation moves a sum by at most cn * 2^-41.

``LinkHeuristicsEval`` scores the two test files exactly as ``LinkPredictEval`` reads them (the first file's edges positive) and
reports, per index, ``link_prediction_lr.auc`` -- the exact Mann-Whitney statistic with average ranks -- of the integer ``cn`` /
weight sums / ``pa`` and the float64 ``jaccard``.  With an ``engine`` the sweep runs on the device on the resident training
graph; without one the same definitions run in numpy on the training file.  The results line is the same string either way.
"""
import numpy as np

from .. import utils
from .link_prediction_lr import auc

SCALE_BITS = 40
SCALE = float(1 << SCALE_BITS)
INDICES = ("cn", "jaccard", "aa", "ra", "pa")


def node_weights(deg):
    """The fixed-point node weights of ``aa`` (row 0) and ``ra`` (row 1) from the distinct degrees: uint64 [2, n_node]."""
    d = np.asarray(deg, dtype=np.float64)
    w = np.zeros((2, len(d)), dtype=np.uint64)
    big, any_ = d >= 2, d >= 1
    w[0, big] = np.rint(SCALE / np.log(d[big])).astype(np.uint64)
    w[1, any_] = np.rint(SCALE / d[any_]).astype(np.uint64)
    return w


def set_adjacency(edges, n_node):
    """Edge list [[a, b], ...] -> (ptr int64 [n_node + 1], adj int64): per node its sorted distinct neighbours without itself."""
    n_node = int(n_node)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if e.size and (e.min() < 0 or e.max() >= n_node):
        raise ValueError("link heuristics: node id outside [0, %d)" % n_node)
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.concatenate([e[:, 0] * n_node + e[:, 1], e[:, 1] * n_node + e[:, 0]]))
    ptr = np.zeros(n_node + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_node, minlength=n_node), out=ptr[1:])
    return ptr, key % n_node


def csr_set_adjacency(rowptr, col):
    """The same from an adjacency CSR that lists every edge in both directions (``Engine.set_graph_csr``'s arrays)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    src = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    return set_adjacency(np.stack([src, np.asarray(col, dtype=np.int64)], axis=1), len(rowptr) - 1)


def host_pair_neighbors(ptr, adj, u, v, weights=None):
    """``Engine.pair_neighbors`` on the host: numpy intersections of the sorted distinct lists, uint64 weight sums.
    -> dict(cn int32 [m], deg_u int32 [m], deg_v int32 [m], wsum uint64 [n_w, m])."""
    u, v = np.asarray(u, dtype=np.int64).reshape(-1), np.asarray(v, dtype=np.int64).reshape(-1)
    if len(u) != len(v):
        raise ValueError("link heuristics: u and v must have the same length, got %d and %d" % (len(u), len(v)))
    n_node = len(ptr) - 1
    if len(u) and (min(u.min(), v.min()) < 0 or max(u.max(), v.max()) >= n_node):
        raise ValueError("link heuristics: node id outside [0, %d)" % n_node)
    w = np.zeros((0, n_node), dtype=np.uint64) if weights is None else np.asarray(weights, dtype=np.uint64).reshape(-1, n_node)
    cn = np.zeros(len(u), dtype=np.int32)
    wsum = np.zeros((len(w), len(u)), dtype=np.uint64)
    for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        c = np.intersect1d(adj[ptr[a]:ptr[a + 1]], adj[ptr[b]:ptr[b + 1]], assume_unique=True)
        c = c[(c != a) & (c != b)]
        cn[i] = len(c)
        if len(w) and len(c):
            wsum[:, i] = w[:, c].sum(axis=1, dtype=np.uint64)
    deg = np.diff(ptr).astype(np.int32)
    return dict(cn=cn, deg_u=deg[u], deg_v=deg[v], wsum=wsum)


def indices(cn, deg_u, deg_v, wsum):
    """The five indices from the sweep's outputs (``wsum`` rows: aa, ra of ``node_weights``) -> dict(cn int64, jaccard float64,
    aa float64, ra float64, pa int64)."""
    cn, du, dv = (np.asarray(x).astype(np.int64) for x in (cn, deg_u, deg_v))
    den = du + dv - cn
    jac = np.zeros(len(cn), dtype=np.float64)
    np.divide(cn, den, out=jac, where=den != 0)
    ws = np.asarray(wsum, dtype=np.uint64).reshape(2, len(cn))
    return dict(cn=cn, jaccard=jac, aa=ws[0].astype(np.float64) / SCALE, ra=ws[1].astype(np.float64) / SCALE, pa=du * dv)


def host_link_heuristics(ptr, adj, u, v):
    """``Engine.link_heuristics`` on the host"""
    res = host_pair_neighbors(ptr, adj, u, v, node_weights(np.diff(ptr)))
    return indices(res["cn"], res["deg_u"], res["deg_v"], res["wsum"])


def format_results(result):
    """The results line ``graph_lp:cn=<auc> jaccard=<auc> aa=<auc> ra=<auc> pa=<auc> n_test=<n>`` (values with ``str``): one line,
    not one per mode -- the graph is the same for both tables."""
    return "graph_lp:" + " ".join("%s=%s" % (k, str(result[k])) for k in INDICES + ("n_test",)) + "\n"


class LinkHeuristicsEval(object):
    def __init__(self, train_filename, test_filename, test_neg_filename, n_node, engine=None):
        self.train_filename, self.test_filename, self.test_neg_filename = train_filename, test_filename, test_neg_filename
        self.n_node = int(n_node)
        # ``engine``: the sweep runs on the device on its resident training graph; otherwise in numpy on the training file
        self.engine = engine

    def read_test(self):
        """(u, v, truth) of the two test files, positives first"""
        pos = utils.read_edges_from_file(self.test_filename)
        neg = utils.read_edges_from_file(self.test_neg_filename)
        if len(pos) == 0 or len(neg) == 0:
            raise ValueError("link heuristics: the test files must hold edges of both classes")
        test = np.array(pos + neg, dtype=np.int64).reshape(-1, 2)
        return test[:, 0], test[:, 1], np.arange(len(test)) < len(pos)

    def sweep(self, u, v):
        """dict(cn, deg_u, deg_v, wsum [2, m]) of the pairs: the integers the AUCs are taken of"""
        if self.engine is not None:
            return self.engine.pair_neighbors(u, v, node_weights(self.engine.distinct_degrees()))
        ptr, adj = set_adjacency(utils.read_edges_from_file(self.train_filename), self.n_node)
        return host_pair_neighbors(ptr, adj, u, v, node_weights(np.diff(ptr)))

    def eval_link_heuristics(self):
        u, v, truth = self.read_test()
        res = self.sweep(u, v)
        idx = indices(res["cn"], res["deg_u"], res["deg_v"], res["wsum"])
        scores = dict(cn=idx["cn"], jaccard=idx["jaccard"], aa=res["wsum"][0], ra=res["wsum"][1], pa=idx["pa"])
        out = dict((k, auc(scores[k], truth)) for k in INDICES)
        out["n_test"] = int(len(truth))
        return out
