"""Node-silhouette evaluator: the label-free score of a partition of the frozen embedding rows.

For rows x_i with clusters c_i (Euclidean distance, NOT squared, so nothing factors through centroids: every pair counts):

    a_i   = the mean distance from i to the OTHER rows of its own cluster
    b_i   = the smallest mean distance from i to the rows of another non-empty cluster (ties to the lowest cluster)
    sil_i = (b_i - a_i) / max(a_i, b_i);   0 for a row alone in its cluster (the scikit-learn convention) and where the
            maximum is 0;   the score is the mean of sil_i

``graph_gan.evaluation()`` reports it, per mode, for two partitions of the labelled nodes: ``sil`` -- the k-means partition that
the ``*_cluster`` line of ``node_clustering.py`` reports (that fit, reused, not refitted) -- and ``label_sil`` -- the labels taken
as the partition: are the classes separated in this embedding?

With an ``engine`` all pairs are streamed on the device (``Engine.silhouette``, gg_silhouette); nothing of size n x n or n x d
crosses to the host.  With ``emd`` (and no engine) the same definition runs on the host in float64 numpy, in row blocks: the CPU
fallback, like ``NodeClusterEval``'s.  ``max_rows`` > 0 evaluates a sample of that many positions, drawn without replacement
by ``RandomState([seed, 0x5349])`` and sorted, each against ALL columns: the usual unbiased estimate of the mean.  A partition
with fewer than two non-empty clusters has no silhouette: its score is ``nan``.
"""
import numpy as np

SAMPLE_STREAM = 0x5349
MAX_K = 128  # the limit of gg_silhouette


def format_results(mode, result):
    """One results line: ``<mode>_sil:sil=<s> label_sil=<l> k=<k> n=<n> rows=<r> precision=<p>`` (values with ``str``)."""
    return "%s_sil:sil=%s label_sil=%s k=%s n=%s rows=%s precision=%s\n" % (
        mode, str(result["sil"]), str(result["label_sil"]), str(result["k"]), str(result["n"]), str(result["rows"]), str(result["precision"]))


def sample_positions(n, max_rows, seed):
    """None (every position) when ``max_rows`` is 0 or >= n, else ``max_rows`` distinct positions, ascending"""
    if isinstance(max_rows, bool) or int(max_rows) != max_rows or int(max_rows) < 0:
        raise ValueError("node silhouette: max_rows must be an integer >= 0 (0 = every row), got %r" % (max_rows,))
    if int(max_rows) == 0 or int(max_rows) >= n:
        return None
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, SAMPLE_STREAM])
    return np.sort(rs.choice(n, size=int(max_rows), replace=False)).astype(np.int64)


def host_silhouette(X, assign, k=None, rows=None, block=512):
    """The definition in float64 on the rows X [m, d] under ``assign`` [m] in [0, k): dict(sil, a, b -- float64 --, nearest int64,
    each [len(rows) or m], mean).  Row blocks of ``block`` rows: nothing of size m x m is held."""
    X, assign = np.asarray(X, dtype=np.float64), np.asarray(assign).astype(np.int64).reshape(-1)
    m = len(X)
    if m < 2 or len(assign) != m:
        raise ValueError("silhouette: needs m >= 2 rows and one cluster per row, got %d rows and %d clusters" % (m, len(assign)))
    k = int(assign.max()) + 1 if k is None else int(k)
    if int(assign.min()) < 0 or int(assign.max()) >= k:
        raise ValueError("silhouette: assign outside [0, k = %d)" % k)
    counts = np.bincount(assign, minlength=k)
    if int((counts > 0).sum()) < 2:
        raise ValueError("silhouette: %d non-empty cluster(s), at least 2 are needed" % int((counts > 0).sum()))
    pos = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64).reshape(-1)
    if len(pos) and (int(pos.min()) < 0 or int(pos.max()) >= m):
        raise ValueError("silhouette: rows outside [0, m = %d)" % m)
    onehot = np.zeros((m, k), dtype=np.float64)
    onehot[np.arange(m), assign] = 1.0
    h = (X * X).sum(axis=1)
    n_out = len(pos)
    sil, a, b = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out)
    nearest = np.zeros(n_out, dtype=np.int64)
    for s in range(0, n_out, int(block)):
        p = pos[s:s + int(block)]
        d = np.sqrt(np.maximum(0.0, h[p][:, None] + h[None, :] - 2.0 * (X[p] @ X.T)))
        d[np.arange(len(p)), p] = 0.0  # the own term, dropped by position
        S = d @ onehot
        own = assign[p]
        r = np.arange(len(p))
        n_own = counts[own]
        a_blk = np.where(n_own > 1, S[r, own] / np.maximum(n_own - 1, 1), 0.0)
        means = np.where(counts[None, :] > 0, S / np.maximum(counts, 1)[None, :], np.inf)
        means[r, own] = np.inf
        near = np.argmin(means, axis=1)  # (ties to the lowest cluster)
        b_blk = means[r, near]
        den = np.maximum(a_blk, b_blk)
        sil[s:s + len(p)] = np.where((n_own > 1) & (den > 0), (b_blk - a_blk) / np.where(den > 0, den, 1.0), 0.0)
        a[s:s + len(p)], b[s:s + len(p)], nearest[s:s + len(p)] = a_blk, b_blk, near
    return dict(sil=sil, a=a, b=b, nearest=nearest, mean=float(sil.sum() / n_out) if n_out else float("nan"))


class NodeSilhouetteEval(object):
    def __init__(self, n_node, n_emb, engine=None, emd=None, which=0, precision="fp32", max_rows=0, seed=0):
        """``engine`` (+ ``which``): all pairs on the device on the resident table, in ``precision`` "fp32" or "bf16"; otherwise
        on ``emd`` (float64 [n_node, n_emb]) on the host, where the reported precision is "float64"."""
        if engine is not None and precision not in ("fp32", "bf16"):
            raise ValueError("node silhouette: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        if engine is None and emd is None:
            raise ValueError("node silhouette: needs an engine or the embedding matrix")
        self.n_node, self.n_emb = n_node, n_emb
        self.engine, self.which, self.emd = engine, which, None if engine is not None else emd
        self.precision = precision if engine is not None else "float64"
        sample_positions(2, max_rows, seed)  # (refuses a bad max_rows here)
        self.max_rows, self.seed = int(max_rows), int(seed)

    def mean_silhouette(self, nodes, assign, k, rows):
        """the mean silhouette of one partition, ``nan`` where fewer than two clusters are non-empty"""
        assign = np.asarray(assign).astype(np.int64).reshape(-1)
        if k > MAX_K:
            raise ValueError("node silhouette: %d clusters, the limit of k is %d" % (k, MAX_K))
        if len(nodes) < 2 or int((np.bincount(assign, minlength=k) > 0).sum()) < 2:
            return float("nan")
        if self.engine is not None:
            return float(self.engine.silhouette(nodes, assign, k=max(int(k), 2), rows=rows, which=self.which, precision=self.precision)["mean"])
        return host_silhouette(np.asarray(self.emd, dtype=np.float64)[nodes], assign, k=k, rows=rows)["mean"]

    def eval_node_silhouette(self, nodes, classes, assign, k):
        """``nodes`` with their label ranks ``classes`` and the clusters ``assign`` in [0, k) of the kept k-means fit
        (``NodeClusterEval.last_partition``) -> dict(sil, label_sil, k, n, rows, precision)"""
        nodes = np.asarray(nodes).astype(np.int64).reshape(-1)
        rows = sample_positions(len(nodes), self.max_rows, self.seed)
        n_labels = int(np.max(classes)) + 1 if len(nodes) else 0
        return dict(sil=self.mean_silhouette(nodes, assign, int(k), rows), label_sil=self.mean_silhouette(nodes, classes, n_labels, rows),
                    k=int(k), n=int(len(nodes)), rows=int(len(nodes) if rows is None else len(rows)), precision=self.precision)
