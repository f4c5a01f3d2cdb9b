"""numpy restatement of the node-classification path (include/graphgan_hip.h, gg_classifier_*) in a chosen dtype: loss and
gradient, the full-batch Adam fit, prediction, the train / test split, the metrics, and planted test data.  The float64 run is
the reference of the device tests; the float32 run of the SAME inputs gives the rounding scale a tolerance is derived from
(``tol``)."""
import math

import numpy as np


def lossgrad(X, y, W, b, l2, dtype=np.float64):
    """(loss, gW, gb) of  -(1/M) sum log softmax(W x + b)[y] + (l2 / 2) |W|^2  with every operation in ``dtype``."""
    X, W, b = np.asarray(X, dtype=dtype), np.asarray(W, dtype=dtype), np.asarray(b, dtype=dtype)
    M = dtype(len(y))
    z = X @ W.T + b
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=1, keepdims=True)
    idx = np.arange(len(y))
    loss = ((np.log(s[:, 0]) + mx[:, 0]) - z[idx, y]).sum(dtype=dtype) / M + dtype(0.5) * dtype(l2) * (W * W).sum(dtype=dtype)
    p = e / s
    p[idx, y] -= dtype(1)
    gW = (p.T @ X) / M + dtype(l2) * W
    gb = p.sum(axis=0, dtype=dtype) / M
    return dtype(loss), gW.astype(dtype), gb.astype(dtype)


def adam_fit(lossgrad, X, labels, n_class, iters, lr, l2, dtype, W=None, b=None):
    """Full-batch Adam (0.9, 0.999, 1e-8, bias-corrected, step count from 1) on ``lossgrad(X, labels, W, b, l2, dtype)`` from zeros
    (or W, b), every operation in ``dtype`` -> (W, b, loss [iters]); loss[t] is the loss at the parameters before update t."""
    X = np.asarray(X, dtype=dtype)
    d = X.shape[1]
    W = np.zeros((n_class, d), dtype=dtype) if W is None else np.asarray(W, dtype=dtype).copy()
    b = np.zeros(n_class, dtype=dtype) if b is None else np.asarray(b, dtype=dtype).copy()
    theta = np.concatenate([W.ravel(), b]).astype(dtype)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    b1, b2, eps, lr = dtype(0.9), dtype(0.999), dtype(1e-8), dtype(lr)
    cd = n_class * d
    losses = np.zeros(iters, dtype=dtype)
    for t in range(1, iters + 1):
        loss, gW, gb = lossgrad(X, labels, theta[:cd].reshape(n_class, d), theta[cd:], l2, dtype)
        losses[t - 1] = loss
        g = np.concatenate([gW.ravel(), gb]).astype(dtype)
        m = b1 * m + (dtype(1) - b1) * g
        v = b2 * v + (dtype(1) - b2) * (g * g)
        c1, c2 = dtype(1.0 - 0.9 ** t), dtype(1.0 - 0.999 ** t)
        theta = (theta - lr * (m / c1) / (np.sqrt(v / c2) + eps)).astype(dtype)
    return theta[:cd].reshape(n_class, d).copy(), theta[cd:].copy(), losses


def fit(X, y, n_class, iters, lr, l2, dtype=np.float64, W=None, b=None):
    """``adam_fit`` of the softmax loss"""
    return adam_fit(lossgrad, X, y, n_class, iters, lr, l2, dtype, W, b)


def logits(X, W, b, dtype=np.float64):
    return np.asarray(X, dtype=dtype) @ np.asarray(W, dtype=dtype).T + np.asarray(b, dtype=dtype)


def predict(X, W, b, dtype=np.float64):
    """argmax of the logits, ties to the lowest class"""
    return np.argmax(logits(X, W, b, dtype), axis=1)


def split(n_labelled, train_ratio, seed):
    perm = np.random.RandomState([int(seed), 0x4E43]).permutation(n_labelled)
    n_train = int(math.ceil(train_ratio * n_labelled))
    return perm[:n_train], perm[n_train:]


def metrics(truth, pred):
    """(acc, macro_f1): F1 = 2TP / (2TP + FP + FN) per class that occurs in truth or pred, unweighted mean"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    f1 = []
    for c in sorted(set(truth.tolist()) | set(pred.tolist())):
        tp = int(np.sum((truth == c) & (pred == c)))
        fp = int(np.sum((truth != c) & (pred == c)))
        fn = int(np.sum((truth == c) & (pred != c)))
        f1.append(2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    return float(np.mean(truth == pred)), float(np.mean(f1))


def scatter_into_table(rows, N, rs):
    """``rows`` [M, d] at random node ids of a table of N > M rows, the other rows noise 0.3 randn (drawn from ``rs``)
    -> (table fp32 [N, d], nodes int64 [M])"""
    M, d = rows.shape
    assert N > M
    table = 0.3 * rs.randn(N, d)
    nodes = rs.permutation(N)[:M]
    table[nodes] = rows
    return table.astype(np.float32), nodes.astype(np.int64)


def planted(M, d, C, N, seed):
    """Class centres 0.3 randn(C, d), rows centre[y] + 0.15 randn, scattered into a table of N > M rows at random node ids,
    the other rows noise -> (table fp32 [N, d], nodes int64 [M], y int64 [M])."""
    rs = np.random.RandomState(seed)
    centre = 0.3 * rs.randn(C, d)
    y = rs.randint(0, C, size=M)
    table, nodes = scatter_into_table(centre[y] + 0.15 * rs.randn(M, d), N, rs)
    return table, nodes, y.astype(np.int64)


def tol(ref32, ref64):
    """max(8 dev, 1e-6), dev = max |float32 reference - float64 reference| on the test's own inputs (the factor 8: tiles and
    staged partials against numpy's pairwise sums)"""
    dev = float(np.max(np.abs(np.asarray(ref32, dtype=np.float64) - np.asarray(ref64, dtype=np.float64))))
    return max(8.0 * dev, 1e-6)
