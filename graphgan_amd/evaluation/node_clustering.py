"""Node-clustering evaluator: k-means on the frozen embedding rows, scored against the labels by NMI, ARI and purity.

The unsupervised twin of ``node_classification.py``.  ALL labelled nodes (``utils.read_labels``: one integer label per node,
sorted by node id) are clustered -- there is no split -- into ``k`` clusters (``k = 0``: the number of distinct labels) by
Lloyd's algorithm:

    a_i = argmin_c |x_i - c_c|^2 (ties to the lowest c),   c_c <- the mean of its rows (an empty cluster keeps its centroid)

stopped at the first sweep, from the second on, that changes no assignment, or after ``max_iters`` sweeps.  ``n_init`` restarts
with seeds ``seed, seed + 1, ...`` are seeded by k-means++ (``Engine.kmeans_seed``: the stated rule) and the run with the lowest
final inertia is kept, the first on ties.

With an ``engine`` the rows are gathered from the resident table and both the seeding distances and the fit run on the device
(``Engine.kmeans_seed`` / ``kmeans_fit``); nothing of size n x d crosses to the host.  With ``emd`` (and no engine) the same
algorithm -- the seeding rule, the Lloyd loop with the same stop rule, the same tie rule, empty clusters that keep their
centroid -- runs on the host in float64: the CPU fallback, like ``NodeClassifyEval``'s.

The scores are float64 functions of the contingency table n_ij (label i, cluster j), n = the number of nodes:

    NMI    = 2 I(U;V) / (H(U) + H(V)), natural logarithms; 1.0 where both entropies are 0
    ARI    = (sum_ij C(n_ij, 2) - e) / ((a + b) / 2 - e),  a = sum_i C(n_i., 2), b = sum_j C(n_.j, 2), e = a b / C(n, 2);
             1.0 where the denominator is 0
    purity = sum_j max_i n_ij / n
"""
import numpy as np

from .. import utils
from ..engine import kmeans_pp_positions


def format_results(mode, result):
    """One results line: ``<mode>_cluster:NMI=<n> ARI=<a> purity=<p> inertia=<i> k=<k> n=<n> iters=<t> empty=<e>`` (values with
    ``str``)."""
    return "%s_cluster:NMI=%s ARI=%s purity=%s inertia=%s k=%s n=%s iters=%s empty=%s\n" % (
        mode, str(result["nmi"]), str(result["ari"]), str(result["purity"]), str(result["inertia"]), str(result["k"]), str(result["n"]),
        str(result["iters"]), str(result["empty"]))


def contingency(u, v):
    """int64 [number of distinct u, number of distinct v]: how many positions carry the pair"""
    _, ui = np.unique(np.asarray(u), return_inverse=True)
    _, vi = np.unique(np.asarray(v), return_inverse=True)
    ui, vi = ui.reshape(-1), vi.reshape(-1)
    table = np.zeros((int(ui.max()) + 1, int(vi.max()) + 1), dtype=np.int64)
    np.add.at(table, (ui, vi), 1)
    return table


def _entropy(counts, n):
    p = counts[counts > 0].astype(np.float64) / n
    return float(-(p * np.log(p)).sum())


def cluster_metrics(labels, assign):
    """dict(nmi, ari, purity) of a partition ``assign`` against ``labels`` (the definitions in the module text)."""
    t = contingency(labels, assign)
    n = int(t.sum())
    ni, nj = t.sum(axis=1), t.sum(axis=0)
    hu, hv = _entropy(ni, n), _entropy(nj, n)
    if hu == 0.0 and hv == 0.0:
        nmi = 1.0
    else:
        i, j = np.nonzero(t)
        nij = t[i, j].astype(np.float64)
        mi = float((nij / n * (np.log(nij * n) - np.log(ni[i].astype(np.float64) * nj[j].astype(np.float64)))).sum())
        nmi = 2.0 * mi / (hu + hv)
    pairs = lambda x: float((x.astype(np.float64) * (x.astype(np.float64) - 1.0) / 2.0).sum())  # noqa: E731
    s, a, b = pairs(t), pairs(ni), pairs(nj)
    total = n * (n - 1.0) / 2.0
    e = a * b / total if total > 0 else 0.0
    den = (a + b) / 2.0 - e
    ari = 1.0 if den == 0.0 else (s - e) / den
    return dict(nmi=float(nmi), ari=float(ari), purity=float(int(t.max(axis=0).sum())) / n)


def host_assign(X, C):
    """(assign int64 [m], dist2 float64 [m]) of rows X against centroids C in the device's form: g = |c|^2 / 2 - x . c, the
    argmin with ties to the lowest cluster (numpy's argmin), dist2 = max(0, |x|^2 + 2 g)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    g = 0.5 * (C * C).sum(axis=1)[None, :] - X @ C.T
    a = np.argmin(g, axis=1)
    return a, np.maximum(0.0, (X * X).sum(axis=1) + 2.0 * g[np.arange(len(X)), a])


def host_kmeans_fit(X, init, max_iters):
    """The device's fit (``Engine.kmeans_fit``) on the host in float64 from the centroids ``init`` [k, d], with its stop rule:
    after sweep t, stop converged when t >= 2 and no assignment changed; else stop when t == max_iters, WITHOUT an update; else
    update (an empty cluster keeps its centroid).  Returns dict(centroids, assign, dist2, counts, inertia [iters], iters,
    converged)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(init, dtype=np.float64)
    k = len(C)
    if int(max_iters) < 1:
        raise ValueError("k-means: max_iters must be >= 1, got %r" % (max_iters,))
    prev, inertia = None, []
    for t in range(1, int(max_iters) + 1):
        a, dist2 = host_assign(X, C)
        counts = np.bincount(a, minlength=k)
        inertia.append(float(dist2.sum()))
        converged = t >= 2 and np.array_equal(a, prev)
        if converged or t == int(max_iters):
            break
        sums = np.zeros_like(C)
        np.add.at(sums, a, X)
        full = counts > 0
        C[full] = sums[full] / counts[full, None]
        prev = a
    return dict(centroids=C, assign=a, dist2=dist2, counts=counts, inertia=np.array(inertia), iters=t, converged=bool(converged))


def host_kmeans_seed(X, k, seed):
    """``Engine.kmeans_seed`` on the host in float64: positions int64 [k] into the rows of X."""
    X = np.asarray(X, dtype=np.float64)
    return kmeans_pp_positions(len(X), int(k), seed, lambda chosen: host_assign(X, X[chosen])[1])


class NodeClusterEval(object):
    def __init__(self, emb_filename, labels_filename, n_node, n_emb, engine=None, emd=None, which=0, k=0, n_init=4, max_iters=100, seed=0):
        self.emb_filename = emb_filename
        self.labels_filename = labels_filename
        self.n_node, self.n_emb = n_node, n_emb
        if isinstance(k, bool) or int(k) != k or not 0 <= int(k) <= 128:
            raise ValueError("node clustering: k must be an integer in [0, 128] (0 = the number of distinct labels), got %r" % (k,))
        if isinstance(n_init, bool) or int(n_init) != n_init or int(n_init) < 1:
            raise ValueError("node clustering: n_init must be an integer >= 1, got %r" % (n_init,))
        if isinstance(max_iters, bool) or int(max_iters) != max_iters or int(max_iters) < 1:
            raise ValueError("node clustering: max_iters must be an integer >= 1, got %r" % (max_iters,))
        self.k, self.n_init, self.max_iters, self.seed = int(k), int(n_init), int(max_iters), int(seed)
        # ``engine`` (+ ``which``): seeding distances and the fit run on the device on the resident table; otherwise on ``emd``
        # (float64 [n_node, n_emb]) or the re-read ``.emb`` text
        self.engine, self.which = engine, which
        if engine is not None:
            self.emd = None
        else:
            self.emd = emd if emd is not None else utils.read_embeddings(emb_filename, n_node=n_node, n_embed=n_emb)

    def fit(self, nodes, k):
        """the best of ``n_init`` restarts: the lowest final inertia, the first on ties"""
        best = None
        X = None if self.engine is not None else np.asarray(self.emd, dtype=np.float64)[nodes]
        for r in range(self.n_init):
            if self.engine is not None:
                pos = self.engine.kmeans_seed(nodes, k, self.seed + r, which=self.which)
                res = self.engine.kmeans_fit(nodes, k, init=np.asarray(nodes)[pos], max_iters=self.max_iters, which=self.which)
            else:
                res = host_kmeans_fit(X, X[host_kmeans_seed(X, k, self.seed + r)], self.max_iters)
            if best is None or res["inertia"][-1] < best["inertia"][-1]:
                best = res
        return best

    def eval_node_clustering(self):
        nodes, classes, values = utils.read_labels(self.labels_filename, self.n_node)
        k = self.k if self.k else len(values)
        if k > 128:
            raise ValueError("node clustering: %s holds %d distinct labels, the limit of k is 128" % (self.labels_filename, k))
        if len(nodes) < k:
            raise ValueError("node clustering: %d labelled nodes are fewer than k = %d clusters" % (len(nodes), k))
        res = self.fit(nodes, k)
        # the kept fit, for evaluators that judge the same partition (node_silhouette.py): not part of the returned scores
        self.last_partition = dict(nodes=nodes, classes=classes, assign=np.asarray(res["assign"]), k=int(k), n_labels=len(values))
        scores = cluster_metrics(classes, res["assign"])
        return dict(scores, inertia=float(res["inertia"][-1]), k=int(k), n=int(len(nodes)), iters=int(res["iters"]),
                    empty=int((np.asarray(res["counts"]) == 0).sum()))
