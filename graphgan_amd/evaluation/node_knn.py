"""k-nearest-neighbour node classification on the frozen embedding rows: the standard protocol without optimiser knobs.

The labelled nodes (``utils.read_labels``: one integer label per node) are split by ``node_classification.split_nodes`` -- the
classifier's split, so the ``*_knn`` lines are comparable with the lines of ``app = "node_classification"`` --, every test node
takes its ``k`` nearest TRAINING nodes under ``metric`` and the majority label among them:

    "cosine"  t(u, c) = s(u, c) w_c,  w = 1 / |x| (0 for a zero row),  s = x_u . x_c;   nearest = largest t
    "l2"      t(u, c) = s(u, c) - |x_c|^2 / 2  (|x_u - x_c|^2 = |x_u|^2 - 2 t);          nearest = largest t
    "dot"     t(u, c) = s(u, c);                                                          nearest = largest t

Neighbours are ordered by (t descending, node id ascending).  The vote is a plain majority over the k neighbours; classes with
equally many votes are separated by their FIRST neighbour: the class whose first neighbour stands earliest in the list wins.
The results are accuracy and Macro-F1 (``node_classification.metrics``).

With an ``engine`` the neighbour query is ONE ``Engine.topk(test_nodes, k, metric=..., candidates=train_nodes)`` on the device
(gg_topk_metric); only the [n_test, k] neighbour ids cross to the host.  With ``emd`` (and no engine) the same definition runs
on the host in float64 numpy, in row blocks: the CPU fallback, like ``NodeClassifyEval``'s.
"""
import numpy as np

from .. import utils
from . import node_classification as nc

METRICS = ("dot", "cosine", "l2")
MAX_K = 256  # the limit of gg_topk_metric


def format_results(mode, result):
    """One results line: ``<mode>_knn:acc=<a> macro_f1=<f> k=<k> metric=<m> n_train=<n> n_test=<n>`` (values with ``str``)."""
    return "%s_knn:acc=%s macro_f1=%s k=%s metric=%s n_train=%s n_test=%s\n" % (
        mode, str(result["acc"]), str(result["macro_f1"]), str(result["k"]), str(result["metric"]), str(result["n_train"]), str(result["n_test"]))


def check_k(k, n_train):
    """``k`` as an int in [1, min(MAX_K, n_train)], or ValueError"""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError("node knn: k must be an integer in [1, %d], got %r" % (MAX_K, k))
    if n_train is not None and int(k) > n_train:
        raise ValueError("node knn: k = %d exceeds the %d training nodes" % (int(k), n_train))
    return int(k)


def vote(neighbour_classes, n_class):
    """``neighbour_classes`` int [n, k], nearest first -> the predicted class [n]: the class with the most votes, among classes
    with equally many the one whose first neighbour stands earliest."""
    nbr = np.asarray(neighbour_classes).astype(np.int64)
    n, k = nbr.shape
    r = np.repeat(np.arange(n), k)
    count = np.zeros((n, n_class), dtype=np.int64)
    np.add.at(count, (r, nbr.ravel()), 1)
    first = np.full((n, n_class), k, dtype=np.int64)
    np.minimum.at(first, (r, nbr.ravel()), np.tile(np.arange(k), n))
    return np.argmax(count * (k + 1) + (k - first), axis=1)  # (distinct classes have distinct first positions: no tie is left)


def host_neighbours(X, queries, candidates, k, metric="cosine", exclude_self=False, block=512):
    """The device's definition in float64 on the rows X [n_node, d]: for each node of ``queries`` its ``k`` nearest nodes among
    ``candidates`` (ids, free to repeat) by (t descending, node id ascending) -> (col int64 [len(queries), k], score float64):
    score is t w_u (cosine), max(0, |x_u|^2 - 2 t) (l2: the squared distance) or t (dot); -1 / -inf (l2: +inf) padded."""
    if metric not in METRICS:
        raise ValueError("node knn: metric must be 'dot', 'cosine' or 'l2', got %r" % (metric,))
    X = np.asarray(X, dtype=np.float64)
    queries = np.asarray(queries).astype(np.int64).reshape(-1)
    cand = np.unique(np.asarray(candidates).astype(np.int64).reshape(-1))  # ascending ids: a stable sort then breaks ties by id
    h = (X * X).sum(axis=1)
    w = np.where(h > 0, 1.0 / np.sqrt(np.where(h > 0, h, 1.0)), 0.0)
    col = np.full((len(queries), k), -1, dtype=np.int64)
    score = np.full((len(queries), k), np.inf if metric == "l2" else -np.inf)
    for s0 in range(0, len(queries), int(block)):
        q = queries[s0:s0 + int(block)]
        t = X[q] @ X[cand].T + 0.0
        if metric == "cosine":
            t = t * w[cand][None, :]
        elif metric == "l2":
            t = t - 0.5 * h[cand][None, :]
        if exclude_self:
            t = np.where(q[:, None] == cand[None, :], -np.inf, t)
        order = np.argsort(-t, axis=1, kind="stable")[:, :k]
        tk = np.take_along_axis(t, order, axis=1)
        live = np.isfinite(tk)
        tk = np.where(live, tk, 0.0)
        if metric == "cosine":
            val = tk * w[q][:, None]
        elif metric == "l2":
            val = np.maximum(0.0, h[q][:, None] - 2.0 * tk)
        else:
            val = tk
        m = order.shape[1]
        col[s0:s0 + len(q), :m] = np.where(live, cand[order], -1)
        score[s0:s0 + len(q), :m] = np.where(live, val, np.inf if metric == "l2" else -np.inf)
    return col, score


class NodeKnnEval(object):
    def __init__(self, labels_filename, n_node, n_emb, engine=None, emd=None, which=0, k=10, metric="cosine", precision="fp32",
                 train_ratio=0.9, seed=0):
        """``engine`` (+ ``which``): the neighbour query runs on the device on the resident table, in ``precision`` "fp32" or
        "bf16"; otherwise on ``emd`` (float64 [n_node, n_emb]) on the host."""
        if metric not in METRICS:
            raise ValueError("node knn: metric must be 'dot', 'cosine' or 'l2', got %r" % (metric,))
        if engine is not None and precision not in ("fp32", "bf16"):
            raise ValueError("node knn: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        if engine is None and emd is None:
            raise ValueError("node knn: needs an engine or the embedding matrix")
        self.labels_filename, self.n_node, self.n_emb = labels_filename, n_node, n_emb
        self.engine, self.which, self.emd = engine, which, None if engine is not None else emd
        self.k, self.metric, self.precision = check_k(k, None), metric, precision
        self.train_ratio, self.seed = train_ratio, seed

    def split(self):
        """(train nodes, train classes, test nodes, test classes, n_class): ``NodeClassifyEval.split`` of the same file"""
        nodes, classes, values = utils.read_labels(self.labels_filename, self.n_node)
        tr, te = nc.split_nodes(len(nodes), self.train_ratio, self.seed)
        return nodes[tr], classes[tr], nodes[te], classes[te], len(values)

    def neighbours(self, test_nodes, train_nodes):
        """int64 [n_test, k]: the k nearest training nodes of every test node, nearest first"""
        if self.engine is not None:
            res = self.engine.topk(test_nodes, self.k, which=self.which, precision=self.precision, exclude=False, metric=self.metric,
                                   candidates=train_nodes)
            return res["col"].astype(np.int64)
        return host_neighbours(self.emd, test_nodes, train_nodes, self.k, metric=self.metric)[0]

    def eval_node_knn(self):
        tr_n, tr_y, te_n, te_y, n_class = self.split()
        k = check_k(self.k, len(tr_n))
        class_of = np.full(self.n_node, -1, dtype=np.int64)
        class_of[tr_n] = tr_y
        nbr = self.neighbours(te_n, tr_n)
        if nbr.shape != (len(te_n), k) or int(nbr.min()) < 0 or int(class_of[nbr].min()) < 0:
            raise RuntimeError("node knn: the neighbour query returned a node outside the training set")
        acc, macro_f1 = nc.metrics(te_y, vote(class_of[nbr], n_class), n_class)
        return dict(acc=acc, macro_f1=macro_f1, k=k, metric=self.metric, n_train=int(len(tr_n)), n_test=int(len(te_n)))
