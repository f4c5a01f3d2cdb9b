"""Test references for the generator's graph softmax: every walk of the reference's sampler enumerated (graph_gan.py:225-270
restated over probabilities instead of draws) and a chi-square check of sampled end nodes against a distribution."""
import numpy as np


def enumerate_walks(emb, bias, root, tree, for_d):
    """Exact law of ONE walk on ``tree`` (dict v -> [father, children...], the root's [root, children...]; a removed father
    is simply absent, as after the reference's ``node_neighbor.remove(root)``), by enumerating every walk prefix in float64.
    Returns (P dict node -> probability, abort probability).  The lists are copied: nothing is mutated."""
    emb = np.asarray(emb, dtype=np.float64)
    bias = np.asarray(bias, dtype=np.float64)
    P, A = {}, [0.0]

    def step(cur, prev, is_root, prob):
        node_neighbor = list(tree[cur][1:]) if is_root else list(tree[cur])
        if len(node_neighbor) == 0:
            A[0] += prob
            return
        if for_d:
            if node_neighbor == [root]:
                A[0] += prob
                return
            if root in node_neighbor:
                node_neighbor.remove(root)
        s = np.array([emb[cur] @ emb[w] + bias[w] for w in node_neighbor])
        q = np.exp(s - s.max())
        q /= q.sum()
        for w, qw in zip(node_neighbor, q):
            if w == prev:
                P[cur] = P.get(cur, 0.0) + prob * qw
            else:
                step(w, cur, False, prob * qw)

    step(root, -1, True, 1.0)
    return P, A[0]


def chi2_pvalue_ok(counts, p, alpha):
    """Pearson chi-square of observed end-node ``counts`` against probabilities ``p`` (renormalised): True when the statistic
    lies below the (1 - alpha) quantile.  Bins expecting fewer than 5 are pooled; a sample where p == 0 fails outright."""
    from scipy import stats
    counts = np.asarray(counts, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    if counts[p == 0].sum() > 0:
        return False
    p = p / p.sum()
    N = counts.sum()
    e = N * p
    big = e >= 5
    obs = list(counts[big])
    exp = list(e[big])
    rest_o, rest_e = counts[~big & (p > 0)].sum(), e[~big & (p > 0)].sum()
    if rest_e > 0:
        obs.append(rest_o)
        exp.append(rest_e)
    obs, exp = np.array(obs), np.array(exp)
    if len(obs) < 2:
        return True
    stat = float(((obs - exp) ** 2 / exp).sum())
    return stat < float(stats.chi2.isf(alpha, len(obs) - 1))
