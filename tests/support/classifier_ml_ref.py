"""numpy restatement of the multi-label node-classification path (include/graphgan_hip.h, gg_classifier_ml_*) in a chosen dtype:
one-vs-rest logistic regression -- loss and gradient in the stable forms, the two prediction rules, the metrics -- and planted
multi-label test data; the Adam fit, the logits and the scatter into a table are classifier_ref's.  As there, the float64 run is
the reference of the device tests and the float32 run of the SAME inputs gives the rounding scale a tolerance is derived from
(``classifier_ref.tol``)."""
import numpy as np

from tests.support.classifier_ref import adam_fit, logits, scatter_into_table, tol  # noqa: F401  (logits, tol: for this module's users)


def lossgrad(X, Y, W, b, l2, dtype=np.float64):
    """(loss, gW, gb) of  (1/M) sum_i sum_c [softplus(z_ic) - y_ic z_ic] + (l2 / 2) |W|^2  with every operation in ``dtype``;
    with e = exp(-|z|): softplus(z) = max(z, 0) + log1p(e), sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e)."""
    X, W, b = np.asarray(X, dtype=dtype), np.asarray(W, dtype=dtype), np.asarray(b, dtype=dtype)
    Y = np.asarray(Y).astype(dtype)
    M = dtype(len(Y))
    z = X @ W.T + b
    e = np.exp(-np.abs(z))
    terms = np.maximum(z, dtype(0)) + np.log1p(e) - Y * z
    loss = terms.sum(dtype=dtype) / M + dtype(0.5) * dtype(l2) * (W * W).sum(dtype=dtype)
    p = np.where(z >= 0, dtype(1), e) / (dtype(1) + e) - Y
    gW = (p.T @ X) / M + dtype(l2) * W
    gb = p.sum(axis=0, dtype=dtype) / M
    return dtype(loss), gW.astype(dtype), gb.astype(dtype)


def fit(X, Y, iters, lr, l2, dtype=np.float64, W=None, b=None):
    """``adam_fit`` of the one-vs-rest loss; the class count is Y's"""
    return adam_fit(lossgrad, X, Y, np.asarray(Y).shape[1], iters, lr, l2, dtype, W, b)


def predict_topk(z, k):
    """bool [M, C]: row i gets its first k[i] classes in the order (logit descending, class ascending) -- a stable argsort of -z"""
    z = np.asarray(z)
    order = np.argsort(-z, axis=1, kind="stable")
    pred = np.zeros(z.shape, dtype=bool)
    for i, ki in enumerate(np.asarray(k).tolist()):
        pred[i, order[i, :ki]] = True
    return pred


def predict_threshold(z):
    """bool [M, C]: the classes with z > 0, strictly"""
    return np.asarray(z) > 0


def topk_gap(z, k):
    """per row the gap between the k-th and the (k + 1)-th largest logit (inf where k is 0 or C: nothing can flip)"""
    z = np.asarray(z, dtype=np.float64)
    s = -np.sort(-z, axis=1)
    k = np.asarray(k)
    C = z.shape[1]
    rows = np.arange(len(z))
    inner = (k > 0) & (k < C)
    gap = np.full(len(z), np.inf)
    gap[inner] = s[rows[inner], k[inner] - 1] - s[rows[inner], k[inner]]
    return gap


def ml_metrics(truth, pred):
    """dict(acc, micro_f1, macro_f1): exact-match ratio; 2 sum TP / (2 sum TP + sum FP + sum FN); the unweighted mean of the
    per-class F1 over the classes that occur in truth or pred"""
    truth, pred = np.asarray(truth).astype(bool), np.asarray(pred).astype(bool)
    f1, tps, dens = [], 0, 0
    for c in range(truth.shape[1]):
        tp = int(np.sum(truth[:, c] & pred[:, c]))
        fp = int(np.sum(~truth[:, c] & pred[:, c]))
        fn = int(np.sum(truth[:, c] & ~pred[:, c]))
        tps += tp
        dens += 2 * tp + fp + fn
        if 2 * tp + fp + fn:
            f1.append(2.0 * tp / (2 * tp + fp + fn))
    return dict(acc=float(np.mean([np.array_equal(t, p) for t, p in zip(truth, pred)])),
                micro_f1=2.0 * tps / dens if dens else 0.0, macro_f1=float(np.mean(f1)) if f1 else 0.0)


def planted(M, d, C, N, seed):
    """Class centres 0.3 randn(C, d); each row draws 1-3 distinct labels and is the sum of their centres + 0.15 randn; the rows
    are scattered into a table of N > M rows at random node ids, the other rows noise
    -> (table fp32 [N, d], nodes int64 [M], Y bool [M, C])."""
    rs = np.random.RandomState(seed)
    centre = 0.3 * rs.randn(C, d)
    Y = np.zeros((M, C), dtype=bool)
    n_lab = rs.randint(1, min(3, C) + 1, size=M)
    for i in range(M):
        Y[i, rs.permutation(C)[:n_lab[i]]] = True
    table, nodes = scatter_into_table(Y.astype(np.float64) @ centre + 0.15 * rs.randn(M, d), N, rs)
    return table, nodes, Y
