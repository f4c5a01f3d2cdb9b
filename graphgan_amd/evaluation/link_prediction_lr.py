"""Learned link-prediction evaluator: the protocol of the GraphGAN paper (a logistic regression on node-pair features, scored by
accuracy and Macro-F1) and of node2vec (a binary operator on the two endpoint rows, a logistic regression, AUC).
``LinkPredictEval`` keeps the reference's median-threshold line; this one stands beside it.

    x = op(E[u], E[v]) elementwise:  "hadamard" a b, "average" (a + b) / 2, "l1" |a - b|, "l2" (a - b)^2
    z = w . x + b,   loss = (1/M) sum [softplus(z) - y z] + (l2 / 2) |w|^2,   ``iters`` steps of full-batch Adam from 0

on the FROZEN embedding rows.  With an ``engine`` both the fit and the logits run on the device on the resident table
(``Engine.edge_classifier_fit`` / ``edge_classifier_predict``); with ``emd`` (and no engine) the same algorithm runs on the host in
float64, like ``NodeClassifyEval``'s fallback.

Training set (``sample_training_pairs``; a contract: the arrays depend on the files, n_node, the seed and max_train alone).
An edge is the pair (min, max) of its ends, keyed min * n_node + max.
  1. positives: the distinct training edges in ascending key order; if there are more than ``max_train``, those at the first
     ``max_train`` positions of ``rs.permutation(n_positives)``, rs = RandomState([seed, 0x4C50]) (no permutation is drawn otherwise);
  2. negatives: as many as positives, from the same ``rs``, by rejection in rounds.  A round that still needs ``k`` pairs draws
     ``a = rs.randint(0, n_node, 2 k + 16)`` and then ``b = rs.randint(0, n_node, 2 k + 16)``; candidate i is (a[i], b[i]).
     Candidates with a == b are dropped, the others are keyed, and in candidate order a key is dropped when it is a training
     edge, a test edge, a pair of the test-negatives file, or was accepted or seen earlier; the first k survivors are accepted.
So nothing the test set holds takes part in the fit.  If fewer free pairs exist than are needed a ValueError says so.
The training rows are the positives, then the negatives; labels 1, then 0.

Test set: the two files exactly as ``LinkPredictEval`` reads them, the first file's edges positive.
Results: ``acc`` (threshold at logit 0, an exact 0 predicts "no edge"), ``macro_f1`` (``node_classification.metrics`` over the two
classes), ``auc`` (exact Mann-Whitney with average ranks for ties, float64 on the host from the logits), ``n_train``, ``n_test``.
"""
import numpy as np

from .. import utils
from .node_classification import _adam, metrics

OPERATORS = ("hadamard", "average", "l1", "l2")  # numbered 0 .. 3 as gg_edge_classifier_*'s `op`


def format_results(mode, result):
    """One results line: ``<mode>_lp:acc=<a> macro_f1=<f> auc=<u> n_train=<n> n_test=<n>`` (values with ``str``)."""
    return "%s_lp:acc=%s macro_f1=%s auc=%s n_train=%s n_test=%s\n" % (mode, str(result["acc"]), str(result["macro_f1"]), str(result["auc"]),
                                                                      str(result["n_train"]), str(result["n_test"]))


def operator_name(op):
    """the operator's name from its name or its number 0 .. 3"""
    if isinstance(op, str) and op in OPERATORS:
        return op
    if not isinstance(op, (str, bool)) and isinstance(op, (int, np.integer)) and 0 <= int(op) <= 3:
        return OPERATORS[int(op)]
    raise ValueError("link prediction: operator must be one of %s or a number in [0, 3], got %r" % (", ".join(OPERATORS), op))


def features(A, B, op):
    """op(A, B) elementwise in the dtype of the rows"""
    op = operator_name(op)
    if op == "hadamard":
        return A * B
    if op == "average":
        return (A + B) * A.dtype.type(0.5)
    if op == "l1":
        return np.abs(A - B)
    return (A - B) * (A - B)


def host_lossgrad(X, y, w, b, l2):
    """float64 loss and gradients of the objective above on features X [M, d], labels y in {0, 1}, in the stable forms
    softplus(z) = max(z, 0) + log1p(exp(-|z|)), sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e)."""
    y = np.asarray(y, dtype=np.float64)
    z = X @ w + b
    e = np.exp(-np.abs(z))
    loss = float((np.maximum(z, 0.0) + np.log1p(e) - y * z).sum() / len(y) + 0.5 * l2 * (w * w).sum())
    p = np.where(z >= 0, 1.0, e) / (1.0 + e) - y
    return loss, p @ X / len(y) + l2 * w, p.sum() / len(y)


def host_fit(X, y, iters, lr, l2):
    """The device's fit on the host in float64: full-batch Adam (0.9, 0.999, 1e-8, bias-corrected) from zeros -> (w [d], b, loss)."""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]

    def lossgrad(W, b):
        loss, gw, gb = host_lossgrad(X, y, W[0], b[0], l2)
        return loss, gw[None, :], np.array([gb])

    W, b, losses = _adam(lossgrad, np.zeros(d + 1), (1, d), iters, lr)
    return W[0], float(b[0]), losses


def auc(scores, truth):
    """The area under the ROC curve as the Mann-Whitney statistic: the share of (positive, negative) pairs the scores order
    rightly, a tie counting 1/2 -- from average ranks, in float64 with integer rank sums (exact)."""
    s = np.asarray(scores, dtype=np.float64)
    t = np.asarray(truth).astype(bool)
    n_pos, n_neg = int(t.sum()), int((~t).sum())
    if s.shape != t.shape or s.ndim != 1 or n_pos == 0 or n_neg == 0:
        raise ValueError("auc: needs one score per label and both classes (%d positives, %d negatives)" % (n_pos, n_neg))
    order = np.argsort(s, kind="stable")
    ss = s[order]
    first = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))  # the start of every run of equal scores
    run = np.diff(np.concatenate([first, [len(ss)]]))
    # twice the average 1-based rank of a run starting at f with r members: 2 f + r + 1 (an integer)
    twice_rank = np.repeat(2 * first + run + 1, run)
    twice_sum = int(twice_rank[t[order]].sum())
    return float((twice_sum - n_pos * (n_pos + 1)) / (2.0 * n_pos * n_neg))


def edge_keys(edges, n_node):
    """int64 keys min * n_node + max of an edge list [[a, b], ...] (ids inside [0, n_node))"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if e.size and (e.min() < 0 or e.max() >= n_node):
        raise ValueError("link prediction: node id outside [0, %d)" % n_node)
    return np.minimum(e[:, 0], e[:, 1]) * np.int64(n_node) + np.maximum(e[:, 0], e[:, 1])


def _in_sorted(sorted_keys, keys):
    if len(sorted_keys) == 0:
        return np.zeros(len(keys), dtype=bool)
    pos = np.minimum(np.searchsorted(sorted_keys, keys), len(sorted_keys) - 1)
    return sorted_keys[pos] == keys


def sample_training_pairs(train_edges, held_out_edges, n_node, seed, max_train):
    """The training set of the module's docstring -> (u int64 [2 P], v int64 [2 P], y int64 [2 P]), u < v on every negative
    row and u <= v on every positive one; ``held_out_edges``: the test edges and the test negatives together."""
    n_node, max_train = int(n_node), int(max_train)
    if max_train < 1:
        raise ValueError("link prediction: max_train must be >= 1, got %d" % max_train)
    rs = np.random.RandomState([int(seed), 0x4C50])
    train = np.unique(edge_keys(train_edges, n_node))
    if len(train) == 0:
        raise ValueError("link prediction: the training file holds no edge")
    pos = train
    if len(pos) > max_train:
        pos = train[rs.permutation(len(train))[:max_train]]
    need = len(pos)
    forbidden = np.unique(np.concatenate([train, edge_keys(held_out_edges, n_node)]))
    n_self = int(np.sum(forbidden // n_node == forbidden % n_node))
    free = n_node * (n_node - 1) // 2 - (len(forbidden) - n_self)
    if free < need:
        raise ValueError("link prediction: %d negative pairs are needed and %d of the %d pairs of %d nodes are neither training nor test pairs"
                         % (need, free, n_node * (n_node - 1) // 2, n_node))
    neg = np.zeros(0, dtype=np.int64)
    while len(neg) < need:
        k = need - len(neg)
        a = rs.randint(0, n_node, 2 * k + 16).astype(np.int64)
        b = rs.randint(0, n_node, 2 * k + 16).astype(np.int64)
        keep = a != b
        key = np.minimum(a, b)[keep] * np.int64(n_node) + np.maximum(a, b)[keep]
        key = key[~_in_sorted(forbidden, key) & ~_in_sorted(np.sort(neg), key)]
        _, first = np.unique(key, return_index=True)
        neg = np.concatenate([neg, key[np.sort(first)][:k]])
    u = np.concatenate([pos // n_node, neg // n_node])
    v = np.concatenate([pos % n_node, neg % n_node])
    y = np.concatenate([np.ones(need, dtype=np.int64), np.zeros(need, dtype=np.int64)])
    return u, v, y


class LinkPredictLREval(object):
    def __init__(self, train_filename, test_filename, test_neg_filename, n_node, n_embed, emd=None, engine=None, which=0, operator="hadamard",
                 iters=200, lr=0.05, l2=1e-4, seed=0, max_train=1 << 20):
        self.train_filename, self.test_filename, self.test_neg_filename = train_filename, test_filename, test_neg_filename
        self.n_node, self.n_embed = int(n_node), int(n_embed)
        self.operator = operator_name(operator)
        self.iters, self.lr, self.l2 = int(iters), float(lr), float(l2)
        self.seed, self.max_train = int(seed), int(max_train)
        # ``engine`` (+ ``which``): fit and logits run on the device on the resident table; otherwise on ``emd`` (float64
        # [n_node, n_embed]) in float64 on the host
        self.engine, self.which = engine, which
        if engine is None and emd is None:
            raise ValueError("link prediction: give an engine or the embedding matrix emd")
        self.emd = None if engine is not None else np.asarray(emd, dtype=np.float64)

    def read_sets(self):
        """(train u, v, y; test u, v, y): the training set of the module's docstring and the two test files, positives first"""
        test_pos = utils.read_edges_from_file(self.test_filename)
        test_neg = utils.read_edges_from_file(self.test_neg_filename)
        test = np.array(test_pos + test_neg, dtype=np.int64).reshape(-1, 2)
        if len(test_pos) == 0 or len(test_neg) == 0:
            raise ValueError("link prediction: the test files must hold edges of both classes")
        tr = sample_training_pairs(utils.read_edges_from_file(self.train_filename), test, self.n_node, self.seed, self.max_train)
        ty = (np.arange(len(test)) < len(test_pos)).astype(np.int64)
        return tr + (test[:, 0], test[:, 1], ty)

    def logits(self, sets=None):
        """fit on the training set -> (the test logits, test labels, n_train)"""
        u, v, y, tu, tv, ty = sets if sets is not None else self.read_sets()
        if self.engine is not None:
            res = self.engine.edge_classifier_fit(u, v, y, op=self.operator, which=self.which, iters=self.iters, lr=self.lr, l2=self.l2)
            z = self.engine.edge_classifier_predict(tu, tv, res["w"], res["b"], op=self.operator, which=self.which)
        else:
            w, b, _ = host_fit(features(self.emd[u], self.emd[v], self.operator), y, self.iters, self.lr, self.l2)
            z = features(self.emd[tu], self.emd[tv], self.operator) @ w + b
        return z, ty, int(len(u))

    def eval_link_prediction(self):
        z, ty, n_train = self.logits()
        acc, macro_f1 = metrics(ty, (z > 0).astype(np.int64), 2)
        return dict(acc=acc, macro_f1=macro_f1, auc=auc(z, ty), n_train=n_train, n_test=int(len(ty)))
