"""Label spreading: the customary graph-only baseline of node classification (Zhou et al. 2004, "Learning with local and global
consistency"; scikit-learn's ``LabelSpreading``), computed from the TRAINING graph and the training labels alone -- no embedding
takes part.  An ``acc=`` of an embedding line that sits below this one has learnt less than the adjacency lists and the labels
already say.

On the neighbour SETS of the training graph (``link_heuristics.set_adjacency``: distinct neighbours other than the node itself;
duplicate edges and self-loops of the file do not count), with deg(v) = |N(v)| and S = D^-1/2 A D^-1/2:

    F_0 = Y0,    F_{t+1} = alpha S F_t + (1 - alpha) Y0,    Y0[v, c] = 1 where v is a training node with label c, else 0

in the factored form the device runs (gg_label_spread): H = sum over w in N(v) of s[w] F_t[w], F_{t+1}[v] = a[v] H + b Y0[v] with
``spread_coefficients``: s = fp32(1 / sqrt(deg)), a = fp32(alpha / sqrt(deg)) (0 for an isolated node), b = fp32(1 - alpha) --
float64 numpy rounded once to fp32, ONE function for the device and the host path.  ``host_label_spread`` runs the same recursion
in float64 on those fp32 coefficients widened; the device runs it in fp32 with two separately rounded operations per entry.

Prediction (``predict``).  Single label: argmax_c F[v, c], ties to the LOWEST class; a test node whose row is all zero -- no
training label within ``iters`` hops -- gets the most frequent training label (ties to the lowest class) and is counted as
``unreached``.  Multi-label: the "topk" protocol only -- the k_i largest entries of the row, k_i = the number of labels the node
truly has, ties to the lower class; an all-zero row takes the k_i most frequent training labels.

``LabelSpreadEval`` uses ``node_classification.split_nodes`` on the sorted labelled nodes -- the split of the classifier and the
k-NN lines, so the three are comparable -- and reports ``node_classification.metrics`` / ``ml_metrics``.  With an ``engine`` the fit
runs on the device on the resident training graph (``Engine.label_spread``); without one ``host_label_spread`` runs on the training
file.  Clamped label propagation (Zhu & Ghahramani), class-mass normalisation and edge weights are not built.
"""
import numpy as np

from .. import utils
from . import link_heuristics as lheur
from . import node_classification as nc

MAX_CLASSES = 128  # == GP_MAX_COL of csrc/graph_prop.hip


def check_alpha_iters(fn, alpha, iters):
    """the refusals of gg_label_spread for its two scalars, with its texts"""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0.0 < float(alpha) < 1.0:
        raise ValueError("%s: alpha = %r outside (0, 1)" % (fn, alpha))
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or int(iters) < 1:
        raise ValueError("%s: iters = %r is below 1" % (fn, iters))


def spread_coefficients(deg, alpha):
    """(s fp32 [n], a fp32 [n], b fp32 scalar) from the distinct degrees: s = 1 / sqrt(deg), a = alpha / sqrt(deg) for deg >= 1,
    else 0; b = 1 - alpha.  float64 numpy, rounded once to fp32."""
    d = np.asarray(deg, dtype=np.float64)
    s, a = np.zeros(len(d), dtype=np.float32), np.zeros(len(d), dtype=np.float32)
    pos = d >= 1
    s[pos] = (1.0 / np.sqrt(d[pos])).astype(np.float32)
    a[pos] = (float(alpha) / np.sqrt(d[pos])).astype(np.float32)
    return s, a, np.float32(1.0 - float(alpha))


def label_matrix(fn, labels, m_train, n_class):
    """The training labels as a bool matrix [m_train, n_class]: from an int array [m_train] (single label), a bool / 0-1 matrix
    [m_train, n_class] or a list of label lists (multi-label).  A label outside [0, n_class) is refused with the ABI's text."""
    C = int(n_class)
    if isinstance(labels, (list, tuple)) and any(isinstance(x, (list, tuple, set, frozenset, np.ndarray)) for x in labels):
        if len(labels) != m_train:  # (a Python list of sequences is a list of label lists; a matrix comes as an array)
            raise ValueError("%s: %d label lists for %d training nodes" % (fn, len(labels), m_train))
        Y = np.zeros((m_train, C), dtype=bool)
        for i, row in enumerate(labels):
            for c in row:
                if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < C:
                    raise ValueError("%s: label_bits row %d has a bit set at a position >= n_class = %d" % (fn, i, C))
                Y[i, int(c)] = True
        return Y
    a = np.asarray(labels)
    if a.ndim == 1 and a.shape == (m_train,) and np.issubdtype(a.dtype, np.integer):
        if a.size and (int(a.min()) < 0 or int(a.max()) >= C):
            row = int(np.flatnonzero((a < 0) | (a >= C))[0])
            raise ValueError("%s: label_bits row %d has a bit set at a position >= n_class = %d" % (fn, row, C))
        Y = np.zeros((m_train, C), dtype=bool)
        Y[np.arange(m_train), a] = True
        return Y
    if a.ndim == 2 and a.shape == (m_train, C) and (a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer)):
        if a.dtype != np.bool_ and a.size and (int(a.min()) < 0 or int(a.max()) > 1):
            raise ValueError("%s: the label matrix must hold 0 and 1 only" % fn)
        return a.astype(bool)
    raise ValueError("%s: labels must be an int array [%d], a bool / 0-1 matrix [%d, %d] or a list of label lists, got %s %r"
                     % (fn, m_train, m_train, C, a.dtype, a.shape))


def check_nodes(fn, name, nodes, n_node, distinct=False):
    """-> int64 1-d ids in [0, n_node), refused with the ABI's texts (the FIRST bad index; the first repeat)"""
    a = np.asarray(nodes)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("%s: %s must be a 1-d array of integers" % (fn, name))
    a = a.astype(np.int64)
    bad = np.flatnonzero((a < 0) | (a >= n_node))
    if len(bad):
        raise ValueError("%s: %s[%d] = %d out of range [0, %d)" % (fn, name, bad[0], a[bad[0]], n_node))
    if distinct and len(a):
        _, first, counts = np.unique(a, return_index=True, return_counts=True)
        if counts.max() > 1:
            seen = {}
            for j, v in enumerate(a.tolist()):
                if v in seen:
                    raise ValueError("%s: %s[%d] = %d repeats %s[%d]" % (fn, name, j, v, name, seen[v]))
                seen[v] = j
    return a


def host_neighbor_sum(ptr, adj, X):
    """sum over w in N(v) of X[w] for every node, in X's dtype (float64 for the host evaluator): ``np.add.reduceat`` over the
    gathered rows; a node without neighbours gives 0."""
    X = np.asarray(X)
    H = np.zeros_like(X)
    has = np.diff(ptr) > 0
    if len(adj):
        H[has] = np.add.reduceat(X[adj], ptr[:-1][has], axis=0)
    return H


def host_label_spread(ptr, adj, train_nodes, labels, n_class, alpha=0.9, iters=30, out_nodes=None):
    """``Engine.label_spread`` on the host in float64, on the fp32-rounded ``spread_coefficients`` widened to float64.
    -> dict(F float64 [m_out, n_class], delta float = max |F_T - F_{T-1}| over all nodes)."""
    fn = "host_label_spread"
    n_node = len(ptr) - 1
    if isinstance(n_class, bool) or int(n_class) != n_class or not 1 <= int(n_class) <= MAX_CLASSES:
        raise ValueError("%s: n_class = %r outside [1, %d]" % (fn, n_class, MAX_CLASSES))
    check_alpha_iters(fn, alpha, iters)
    tr = check_nodes(fn, "train_nodes", train_nodes, n_node, distinct=True)
    Y = label_matrix(fn, labels, len(tr), n_class)
    out = None if out_nodes is None else check_nodes(fn, "out_nodes", out_nodes, n_node)
    s, a, b = (np.asarray(x, dtype=np.float64) for x in spread_coefficients(np.diff(ptr), alpha))
    base = np.zeros((n_node, int(n_class)), dtype=np.float64)
    base[tr] = Y * b
    F = np.zeros_like(base)
    F[tr] = Y
    prev = F
    for _ in range(int(iters)):
        prev, F = F, a[:, None] * host_neighbor_sum(ptr, adj, s[:, None] * F) + base
    return dict(F=F if out is None else F[out], delta=float(np.max(np.abs(F - prev))) if F.size else 0.0)


def _ranked(score):
    """positions of every entry of a row in the order (score descending, class ascending)"""
    order = np.argsort(-score, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(score.shape[1]), score.shape), axis=1)
    return rank


def predict(F, train_labels, k=None):
    """The prediction rule stated at the top.  ``train_labels``: the training label matrix bool [m_train, C] (its column sums are
    the label frequencies of the fallback).  Without ``k``: (classes int64 [m], unreached); with ``k`` (one count per row):
    (bool [m, C], unreached)."""
    F = np.asarray(F)
    freq = np.asarray(train_labels).astype(bool).sum(axis=0).astype(np.float64)
    dead = ~np.any(F != 0, axis=1)
    score = np.where(dead[:, None], freq[None, :], F.astype(np.float64))
    if k is None:
        return np.argmax(score, axis=1).astype(np.int64), int(dead.sum())  # (numpy's argmax: the first, so the lowest, class)
    return _ranked(score) < np.asarray(k).reshape(-1, 1), int(dead.sum())


KEYS = ("acc", "macro_f1", "alpha", "iters", "delta", "unreached", "n_train", "n_test")
ML_KEYS = ("acc", "micro_f1") + KEYS[1:]


def format_results(result, multilabel=False):
    """The results line ``graph_nc:acc=<a> macro_f1=<f> alpha=<a> iters=<t> delta=<d> unreached=<u> n_train=<n> n_test=<n>`` (multi-label:
    ``micro_f1=<f>`` behind ``acc``), values with ``str``: one line, not one per mode -- the graph is the same for both tables."""
    return "graph_nc:" + " ".join("%s=%s" % (k, str(result[k])) for k in (ML_KEYS if multilabel else KEYS)) + "\n"


class LabelSpreadEval(object):
    def __init__(self, train_filename, labels_filename, n_node, engine=None, train_ratio=0.9, seed=0, alpha=0.9, iters=30, multilabel=False):
        check_alpha_iters("label spreading", alpha, iters)
        self.train_filename, self.labels_filename, self.n_node = train_filename, labels_filename, int(n_node)
        # ``engine``: the fit runs on the device on its resident training graph; otherwise in float64 numpy on the training file
        self.engine = engine
        self.train_ratio, self.seed = train_ratio, seed
        self.alpha, self.iters, self.multilabel = float(alpha), int(iters), bool(multilabel)

    def split(self):
        """(train nodes, train label matrix bool, test nodes, test classes or label matrix, n_class): ``NodeClassifyEval.split``'s"""
        read = utils.read_multilabels if self.multilabel else utils.read_labels
        nodes, classes, values = read(self.labels_filename, self.n_node)
        n_class = len(values)
        if not 1 <= n_class <= MAX_CLASSES:
            raise ValueError("label spreading: %s holds %d distinct labels, the sweep takes 1 to %d" % (self.labels_filename, n_class, MAX_CLASSES))
        tr, te = nc.split_nodes(len(nodes), self.train_ratio, self.seed)
        tr_y = classes[tr] if self.multilabel else label_matrix("label spreading", classes[tr], len(tr), n_class)
        return nodes[tr], tr_y, nodes[te], classes[te], n_class

    def spread(self, tr_n, tr_y, n_class, te_n):
        """dict(F [n_test, n_class], delta) of the test nodes"""
        if self.engine is not None:
            return self.engine.label_spread(tr_n, tr_y, n_class, alpha=self.alpha, iters=self.iters, out_nodes=te_n)
        ptr, adj = lheur.set_adjacency(utils.read_edges_from_file(self.train_filename), self.n_node)
        return host_label_spread(ptr, adj, tr_n, tr_y, n_class, alpha=self.alpha, iters=self.iters, out_nodes=te_n)

    def eval_label_spread(self):
        tr_n, tr_y, te_n, te_y, n_class = self.split()
        res = self.spread(tr_n, tr_y, n_class, te_n)
        if self.multilabel:
            pred, unreached = predict(res["F"], tr_y, k=te_y.sum(axis=1))
            scores = nc.ml_metrics(te_y, pred)
        else:
            pred, unreached = predict(res["F"], tr_y)
            scores = dict(zip(("acc", "macro_f1"), nc.metrics(te_y, pred, n_class)))
        return dict(scores, alpha=self.alpha, iters=self.iters, delta=float(res["delta"]), unreached=unreached, n_train=int(len(tr_n)),
                    n_test=int(len(te_n)))
