"""Embedding-spectrum evaluator: what the table itself looks like, with no labels, test edges or negatives.

The PCA of the embedding rows of the nodes that have at least one training edge (degree-0 rows are the untrained U[0, 1) fill and
would be measured as signal), reported through the eigenvalues lambda_1 >= ... >= lambda_d >= 0 of the rows' covariance (divided
by n, not n - 1) and the rows' mean.  With p_j = lambda_j / sum lambda:

    erank     = exp(-sum_j p_j ln p_j) over p_j > 0      the effective rank (Roy & Vetterli): d for an isotropic cloud, 1 for a line
    pr        = (sum lambda)^2 / sum lambda^2             the participation ratio
    top1      = p_1,   top10 = sum_{j <= min(10, d)} p_j  the share of the variance on the first component(s)
    var       = sum lambda                                the total variance: do the rows shrink or blow up?
    mean_norm = |mean|                                    do the rows drift as a block?

A collapse onto few directions shows as erank, pr falling and top1 rising; a common drift as mean_norm growing beside sqrt(var).
``sum lambda == 0`` (all rows equal) prints ``nan`` for the first four.

The algorithm is two passes, the same with and without an engine.  Pass A: the column sums give mean64 = sums / m and the centre
float32(mean64).  Pass B: G = sum_i c_i c_i^T and r = sum_i c_i with c_i = x_i - centre; cov = (G - outer(r, r) / m) / m in
float64 (the fp32 centre is not the float64 mean: r carries the difference).  With an ``engine`` both passes are sweeps on the
device (``Engine.pca``, gg_gram: fp32 chains on the matrix cores, added in float64; nothing of size m x d crosses to the host);
without one ``host_pca`` runs them in float64 numpy on the ``.emb`` text.
"""
import numpy as np

from .. import utils


def pca_cov(G, r, m):
    """cov = (G - outer(r, r) / m) / m in float64 from the centred Gram matrix, the residual sums and the row count"""
    G, r = np.asarray(G, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return (G - np.outer(r, r) / float(m)) / float(m)


def pca_eig(cov):
    """``numpy.linalg.eigh`` of ``cov`` -> (eigenvalues descending, clipped at 0; eigenvectors as ROWS in that order, each signed
    so that its largest-magnitude entry -- the lowest index on ties -- is positive)"""
    lam, vec = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.argsort(-lam, kind="stable")
    lam, vec = np.maximum(lam[order], 0.0), np.ascontiguousarray(vec[:, order].T)
    lead = np.argmax(np.abs(vec), axis=1)  # (argmax: the first of equal maxima)
    sign = np.where(vec[np.arange(len(vec)), lead] < 0, -1.0, 1.0)
    return lam, vec * sign[:, None]


def host_pca(X, nodes, n_components=None):
    """The two-pass PCA of ``Engine.pca`` in float64 numpy on the rows ``nodes`` (m >= 2) of X [n, d]: the centre is
    float32(mean64), as on the device.  Returns dict(mean fp32 [d], eigenvalues float64 [d], components fp32 [n_components, d],
    cov float64 [d, d], m, mean64 -- pass A's float64 mean)."""
    X = np.asarray(X, dtype=np.float64)
    nodes = np.asarray(nodes).astype(np.int64).reshape(-1)
    m, d = len(nodes), X.shape[1]
    if m < 2:
        raise ValueError("host_pca: needs m >= 2 rows, got %d" % m)
    R = X[nodes]
    mean64 = R.sum(axis=0) / m
    center = mean64.astype(np.float32)
    C = R - center.astype(np.float64)
    cov = pca_cov(C.T @ C, C.sum(axis=0), m)
    lam, vec = pca_eig(cov)
    k = d if n_components is None else int(n_components)
    return dict(mean=center, eigenvalues=lam, components=np.ascontiguousarray(vec[:k], dtype=np.float32), cov=cov, m=m, mean64=mean64)


def spectrum_metrics(eigenvalues, mean):
    """dict(erank, pr, top1, top10, var, mean_norm) of a spectrum (any order, negatives clipped at 0) and a mean, in float64"""
    lam = np.sort(np.maximum(np.asarray(eigenvalues, dtype=np.float64).reshape(-1), 0.0))[::-1]
    mean_norm = float(np.sqrt(np.sum(np.asarray(mean, dtype=np.float64) ** 2)))
    total = float(lam.sum())
    if not total > 0.0:
        nan = float("nan")
        return dict(erank=nan, pr=nan, top1=nan, top10=nan, var=total, mean_norm=mean_norm)
    p = lam / total
    pos = p[p > 0]
    return dict(erank=float(np.exp(-np.sum(pos * np.log(pos)))), pr=float(total * total / np.sum(lam * lam)), top1=float(p[0]),
                top10=float(p[:min(10, len(p))].sum()), var=total, mean_norm=mean_norm)


def format_results(mode, result):
    """One results line: ``<mode>_spec:erank=<e> pr=<p> top1=<t> top10=<t> var=<v> mean_norm=<n> n=<n> d=<d>`` (values with ``str``)."""
    return "%s_spec:erank=%s pr=%s top1=%s top10=%s var=%s mean_norm=%s n=%s d=%s\n" % (
        mode, str(result["erank"]), str(result["pr"]), str(result["top1"]), str(result["top10"]), str(result["var"]), str(result["mean_norm"]),
        str(result["n"]), str(result["d"]))


def trained_nodes(train_filename, n_node=None):
    """the nodes with at least one training edge, ascending (int64)"""
    ids = set()
    for edge in utils.read_edges_from_file(train_filename):
        ids.update(edge[:2])
    nodes = np.array(sorted(ids), dtype=np.int64)
    if n_node is not None and len(nodes) and (int(nodes[0]) < 0 or int(nodes[-1]) >= n_node):
        raise ValueError("embedding spectrum: %s names a node outside [0, %d)" % (train_filename, n_node))
    return nodes


class EmbeddingSpectrumEval(object):
    def __init__(self, embed_filename, train_filename, n_node, n_emb, engine=None, which=0):
        """``engine`` (+ ``which``): both passes on the device on the resident table; otherwise float64 on the ``.emb`` text."""
        self.embed_filename, self.train_filename = embed_filename, train_filename
        self.n_node, self.n_emb = n_node, n_emb
        self.engine, self.which = engine, which

    def eval_embedding_spectrum(self):
        """-> dict(erank, pr, top1, top10, var, mean_norm, n, d)"""
        nodes = trained_nodes(self.train_filename, self.n_node)
        if len(nodes) < 2:
            raise ValueError("embedding spectrum: needs at least two nodes with a training edge, %s has %d" % (self.train_filename, len(nodes)))
        if self.engine is not None:
            fit = self.engine.pca(nodes, which=self.which)
        else:
            fit = host_pca(utils.read_embeddings(self.embed_filename, n_node=self.n_node, n_embed=self.n_emb), nodes)
        out = spectrum_metrics(fit["eigenvalues"], fit["mean64"])
        out.update(n=int(len(nodes)), d=int(self.n_emb))
        return out
