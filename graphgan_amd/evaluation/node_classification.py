"""Node-classification evaluator (the GraphGAN paper's third application, scored by accuracy and Macro-F1).

The labelled nodes (``utils.read_labels``: one integer label per node) are split ``train_ratio : 1 - train_ratio`` (the paper:
9:1), multinomial logistic regression is fitted on the FROZEN embedding rows of the training nodes and applied to the test
nodes:

    z = W . E[node] + b,   loss = -(1/M) sum log softmax(z)[label] + (l2 / 2) |W|^2,   ``iters`` steps of full-batch Adam from 0

With an ``engine`` the rows are gathered from the resident table and both the fit and the prediction run on the device
(``Engine.classifier_fit`` / ``classifier_predict``); nothing of size M x d crosses to the host.  With ``emd`` (and no
engine) the same algorithm runs on the host in float64: the CPU fallback, like ``LinkPredictEval``'s.  The split depends
on the seed and the labelled nodes alone, so the lines of a run are comparable.
"""
import math

import numpy as np

from .. import utils


def format_results(mode, result):
    """One results line: ``<mode>:acc=<a> macro_f1=<f> n_train=<n> n_test=<n>`` (values with ``str``)."""
    return "%s:acc=%s macro_f1=%s n_train=%s n_test=%s\n" % (mode, str(result["acc"]), str(result["macro_f1"]), str(result["n_train"]),
                                                             str(result["n_test"]))


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


def host_fit(X, y, n_class, iters, lr, l2):
    """The device's fit on the host in float64: full-batch Adam (0.9, 0.999, 1e-8, bias-corrected) from zeros -> (W, b, loss)."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.zeros(n_class * X.shape[1] + n_class)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    cd = n_class * X.shape[1]
    losses = np.zeros(iters)
    for t in range(1, iters + 1):
        loss, gW, gb = host_lossgrad(X, y, theta[:cd].reshape(n_class, -1), theta[cd:], l2)
        losses[t - 1] = loss
        g = np.concatenate([gW.ravel(), gb])
        m = 0.9 * m + (1 - 0.9) * g
        v = 0.999 * v + (1 - 0.999) * g * g
        theta = theta - lr * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + 1e-8)
    return theta[:cd].reshape(n_class, -1).copy(), theta[cd:].copy(), losses


def host_predict(X, W, b):
    """argmax of the float64 logits, ties to the lowest class (numpy's argmax)."""
    return np.argmax(np.asarray(X, dtype=np.float64) @ W.T + b, axis=1)


class NodeClassifyEval(object):
    def __init__(self, embed_filename, labels_filename, n_node, n_embed, emd=None, engine=None, which=0, train_ratio=0.9, seed=0,
                 iters=200, lr=0.05, l2=1e-4):
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
        """(train nodes, train classes, test nodes, test classes, n_class) of the labels file."""
        nodes, classes, values = utils.read_labels(self.labels_filename, self.n_node)
        tr, te = split_nodes(len(nodes), self.train_ratio, self.seed)
        return nodes[tr], classes[tr], nodes[te], classes[te], len(values)

    def eval_node_classification(self):
        tr_n, tr_y, te_n, te_y, n_class = self.split()
        if n_class < 2:
            raise ValueError("node classification: %s holds one label value only" % self.labels_filename)
        if self.engine is not None:
            fit = self.engine.classifier_fit(tr_n, tr_y, n_class, which=self.which, iters=self.iters, lr=self.lr, l2=self.l2)
            pred = self.engine.classifier_predict(te_n, fit["W"], fit["b"], which=self.which)
        else:
            emd = np.asarray(self.emd, dtype=np.float64)
            W, b, _ = host_fit(emd[tr_n], tr_y, n_class, self.iters, self.lr, self.l2)
            pred = host_predict(emd[te_n], W, b)
        acc, f1 = metrics(te_y, pred, n_class)
        return dict(acc=acc, macro_f1=f1, n_train=int(len(tr_n)), n_test=int(len(te_n)))
