"""Node-classification evaluator (the GraphGAN paper's third application, scored by accuracy and Macro-F1).

The labelled nodes (``utils.read_labels``: one integer label per node) are split ``train_ratio : 1 - train_ratio`` (the paper:
9:1), multinomial logistic regression is fitted on the FROZEN embedding rows of the training nodes and applied to the test
nodes:

    z = W . E[node] + b,   loss = -(1/M) sum log softmax(z)[label] + (l2 / 2) |W|^2,   ``iters`` steps of full-batch Adam from 0

With an ``engine`` the rows are gathered from the resident table and both the fit and the prediction run on the device
(``Engine.classifier_fit`` / ``classifier_predict``); nothing of size M x d crosses to the host.  With ``emd`` (and no
engine) the same algorithm runs on the host in float64: the CPU fallback, like ``LinkPredictEval``'s.  The split depends
on the seed and the labelled nodes alone, so the lines of a run are comparable.

Multi-label (``multilabel=True``; the paper's BlogCatalog and Wikipedia give a node several labels).  The file holds lines of
``node label [label ...]`` (``utils.read_multilabels``: a node's labels are the union over its lines), the split is the SAME
``split_nodes``, and the classifier is one-vs-rest logistic regression, one binary problem per class:

    loss = (1/M) sum_i sum_c [softplus(z_ic) - y_ic z_ic] + (l2 / 2) |W|^2

(``Engine.classifier_ml_fit`` / ``classifier_ml_predict``, or the float64 host fallback).  ``ml_protocol="topk"`` is the customary
protocol of DeepWalk / node2vec / GraphGAN: a test node is given as many labels as it truly has -- its k_i highest logits, ties to
the lower class -- so the prediction READS THE TEST NODES' LABEL COUNTS (not which labels).  ``"threshold"`` uses no test
information: the classes with a positive logit.  The results are the exact-match ratio, Micro-F1 and Macro-F1 (``ml_metrics``).
"""
import math

import numpy as np

from .. import utils


def format_results(mode, result):
    """One results line: ``<mode>:acc=<a> macro_f1=<f> n_train=<n> n_test=<n>`` (values with ``str``)."""
    return "%s:acc=%s macro_f1=%s n_train=%s n_test=%s\n" % (mode, str(result["acc"]), str(result["macro_f1"]), str(result["n_train"]),
                                                             str(result["n_test"]))


def format_ml_results(mode, result):
    """One multi-label results line: ``<mode>:acc=<a> micro_f1=<f> macro_f1=<f> n_train=<n> n_test=<n>`` (values with ``str``)."""
    return "%s:acc=%s micro_f1=%s macro_f1=%s n_train=%s n_test=%s\n" % (mode, str(result["acc"]), str(result["micro_f1"]),
                                                                         str(result["macro_f1"]), str(result["n_train"]), str(result["n_test"]))


def split_nodes(n_labelled, train_ratio, seed):
    """(train, test) index arrays into the sorted labelled nodes: a permutation by RandomState([seed, 0x4E43]), the first
    ceil(train_ratio * L) train."""
    perm = np.random.RandomState([int(seed), 0x4E43]).permutation(n_labelled)
    n_train = int(math.ceil(train_ratio * n_labelled))
    if n_train <= 0 or n_train >= n_labelled:
        raise ValueError("node classification: train_ratio = %r of %d labelled nodes leaves the %s side empty"
                         % (train_ratio, n_labelled, "training" if n_train <= 0 else "test"))
    return perm[:n_train], perm[n_train:]


def metrics(truth, pred, n_class):
    """(acc, macro_f1) from one confusion matrix: macro_f1 = the unweighted mean of 2TP / (2TP + FP + FN) over the classes that
    occur in ``truth`` or ``pred`` (0 where the denominator is 0)."""
    truth, pred = np.asarray(truth, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    cm = np.zeros((n_class, n_class), dtype=np.int64)
    np.add.at(cm, (truth, pred), 1)
    tp = np.diag(cm).astype(np.float64)
    den = cm.sum(axis=0) + cm.sum(axis=1)  # 2TP + FP + FN
    present = den > 0
    f1 = np.where(present, 2.0 * tp / np.maximum(den, 1), 0.0)
    acc = float(tp.sum() / len(truth))
    return acc, float(f1[present].mean()) if present.any() else 0.0


def host_lossgrad(X, y, W, b, l2):
    """float64 loss and gradients of the objective above on rows X [M, d]."""
    z = X @ W.T + b
    z -= z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1))
    p = np.exp(z - lse[:, None])
    idx = np.arange(len(y))
    loss = float(-(z[idx, y] - lse).mean() + 0.5 * l2 * (W * W).sum())
    p[idx, y] -= 1.0
    return loss, p.T @ X / len(y) + l2 * W, p.sum(axis=0) / len(y)


def _adam(lossgrad, theta0, shape, iters, lr):
    """``iters`` steps of full-batch Adam (0.9, 0.999, 1e-8, bias-corrected, step count from 1) on theta = (W.ravel(), b) of
    ``shape`` = (n_class, d) from ``theta0``; ``lossgrad(W, b)`` -> (loss, gW, gb) -> (W, b, loss [iters], before each update)."""
    n_class, d = shape
    cd = n_class * d
    theta = theta0
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    losses = np.zeros(iters)
    for t in range(1, iters + 1):
        loss, gW, gb = lossgrad(theta[:cd].reshape(n_class, -1), theta[cd:])
        losses[t - 1] = loss
        g = np.concatenate([gW.ravel(), gb])
        m = 0.9 * m + (1 - 0.9) * g
        v = 0.999 * v + (1 - 0.999) * g * g
        theta = theta - lr * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + 1e-8)
    return theta[:cd].reshape(n_class, -1).copy(), theta[cd:].copy(), losses


def _host_fit(lossgrad, X, labels, n_class, iters, lr, l2):
    """``_adam`` from zeros on ``lossgrad`` (host_lossgrad or host_ml_lossgrad) of the float64 rows X and their labels"""
    X = np.asarray(X, dtype=np.float64)
    return _adam(lambda W, b: lossgrad(X, labels, W, b, l2), np.zeros(n_class * X.shape[1] + n_class), (n_class, X.shape[1]), iters, lr)


def host_fit(X, y, n_class, iters, lr, l2):
    """The device's fit on the host in float64: full-batch Adam (0.9, 0.999, 1e-8, bias-corrected) from zeros -> (W, b, loss)."""
    return _host_fit(host_lossgrad, X, y, n_class, iters, lr, l2)


def host_predict(X, W, b):
    """argmax of the float64 logits, ties to the lowest class (numpy's argmax)."""
    return np.argmax(np.asarray(X, dtype=np.float64) @ W.T + b, axis=1)


def ml_metrics(truth, pred):
    """dict(acc, micro_f1, macro_f1) of indicator matrices bool [n, C]: acc = the exact-match ratio (the whole label set of a
    row correct), micro_f1 = 2 sum TP / (2 sum TP + sum FP + sum FN), macro_f1 = the unweighted mean of the per-class
    2TP / (2TP + FP + FN) over the classes that occur in ``truth`` or ``pred`` (the rule of ``metrics``)."""
    truth, pred = np.asarray(truth).astype(bool), np.asarray(pred).astype(bool)
    tp = (truth & pred).sum(axis=0).astype(np.float64)
    den = truth.sum(axis=0) + pred.sum(axis=0)  # 2TP + FP + FN per class
    present = den > 0
    f1 = np.where(present, 2.0 * tp / np.maximum(den, 1), 0.0)
    return dict(acc=float(np.mean(np.all(truth == pred, axis=1))),
                micro_f1=float(2.0 * tp.sum() / den.sum()) if den.sum() else 0.0,
                macro_f1=float(f1[present].mean()) if present.any() else 0.0)


def host_ml_lossgrad(X, Y, W, b, l2):
    """float64 loss and gradients of the one-vs-rest objective on rows X [M, d] and labels Y bool [M, C], in the stable forms
    softplus(z) = max(z, 0) + log1p(exp(-|z|)), sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e)."""
    Y = np.asarray(Y, dtype=np.float64)
    z = X @ W.T + b
    e = np.exp(-np.abs(z))
    loss = float((np.maximum(z, 0.0) + np.log1p(e) - Y * z).sum() / len(Y) + 0.5 * l2 * (W * W).sum())
    p = np.where(z >= 0, 1.0, e) / (1.0 + e) - Y
    return loss, p.T @ X / len(Y) + l2 * W, p.sum(axis=0) / len(Y)


def host_ml_fit(X, Y, iters, lr, l2):
    """The device's multi-label fit on the host in float64: the Adam of ``host_fit`` from zeros -> (W, b, loss)."""
    return _host_fit(host_ml_lossgrad, X, Y, np.asarray(Y).shape[1], iters, lr, l2)


def host_ml_predict(X, W, b, k=None):
    """bool [M, C] from the float64 logits: with ``k`` the first k[i] classes of row i by (logit descending, class ascending),
    without the classes with z > 0."""
    z = np.asarray(X, dtype=np.float64) @ W.T + b
    if k is None:
        return z > 0
    order = np.argsort(-z, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(z.shape[1]), z.shape), axis=1)
    return rank < np.asarray(k)[:, None]


class NodeClassifyEval(object):
    def __init__(self, embed_filename, labels_filename, n_node, n_embed, emd=None, engine=None, which=0, train_ratio=0.9, seed=0,
                 iters=200, lr=0.05, l2=1e-4, multilabel=False, ml_protocol="topk"):
        """``multilabel``: read ``labels_filename`` with ``utils.read_multilabels`` and fit one-vs-rest logistic regression.
        ``ml_protocol`` "topk" predicts for test node i its k_i best classes, k_i = the number of labels the node truly has --
        the customary protocol, which reads the test nodes' label COUNTS --; "threshold" predicts the classes with a positive
        logit."""
        if ml_protocol not in ("topk", "threshold"):
            raise ValueError("node classification: ml_protocol must be 'topk' or 'threshold', got %r" % (ml_protocol,))
        self.multilabel, self.ml_protocol = bool(multilabel), ml_protocol
        self.embed_filename = embed_filename
        self.labels_filename = labels_filename
        self.n_node = n_node
        self.n_embed = n_embed
        self.train_ratio, self.seed = train_ratio, seed
        self.iters, self.lr, self.l2 = int(iters), float(lr), float(l2)
        # ``engine`` (+ ``which``): fit and prediction run on the device on the resident table; otherwise on ``emd`` (float64
        # [n_node, n_embed]) or the re-read ``.emb`` text
        self.engine, self.which = engine, which
        if engine is not None:
            self.emd = None
        else:
            self.emd = emd if emd is not None else utils.read_embeddings(embed_filename, n_node=n_node, n_embed=n_embed)

    def split(self):
        """(train nodes, train classes, test nodes, test classes, n_class) of the labels file; with ``multilabel`` the classes
        are rows of the bool matrix [L, n_class]."""
        read = utils.read_multilabels if self.multilabel else utils.read_labels
        nodes, classes, values = read(self.labels_filename, self.n_node)
        tr, te = split_nodes(len(nodes), self.train_ratio, self.seed)
        return nodes[tr], classes[tr], nodes[te], classes[te], len(values)

    def eval_node_classification(self):
        tr_n, tr_y, te_n, te_y, n_class = self.split()
        if n_class < 2:
            raise ValueError("node classification: %s holds one label value only" % self.labels_filename)
        ml, eng = self.multilabel, self.engine
        # what the multi-label prediction takes beyond (W, b): with "topk" the test nodes' label counts
        extra = dict(k=te_y.sum(axis=1).astype(np.int32) if self.ml_protocol == "topk" else None) if ml else {}
        if eng is not None:
            fit, predict = (eng.classifier_ml_fit, eng.classifier_ml_predict) if ml else (eng.classifier_fit, eng.classifier_predict)
            res = fit(tr_n, tr_y, n_class, which=self.which, iters=self.iters, lr=self.lr, l2=self.l2)
            pred = predict(te_n, res["W"], res["b"], which=self.which, **extra)
        else:
            lossgrad, predict = (host_ml_lossgrad, host_ml_predict) if ml else (host_lossgrad, host_predict)
            emd = np.asarray(self.emd, dtype=np.float64)
            W, b, _ = _host_fit(lossgrad, emd[tr_n], tr_y, n_class, self.iters, self.lr, self.l2)
            pred = predict(emd[te_n], W, b, **extra)
        scores = ml_metrics(te_y, pred) if ml else dict(zip(("acc", "macro_f1"), metrics(te_y, pred, n_class)))
        return dict(scores, n_train=int(len(tr_n)), n_test=int(len(te_n)))
