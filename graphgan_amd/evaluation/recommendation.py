"""Recommendation evaluator (the GraphGAN paper's second application, scored by Precision@K / Recall@K).

For every node u with at least one test edge (test edges are undirected), the nodes are ranked by s(u, v) = E[u] . E[v]
(no bias; the link-prediction score, ``link_prediction.py``), score descending and column ascending, over the ELIGIBLE
nodes: every node except u itself and u's neighbours in the training graph.  With T(u) the test neighbours of u:

    P@K = mean_u |top_K(u) & T(u)| / K,        R@K = mean_u |top_K(u) & T(u)| / |T(u)|

With an ``engine`` the ranking is ONE streamed top-K call on the device (``Engine.topk`` with ``max(ks)`` and
``exclude=True`` against the engine's resident training graph; every K is a prefix of it).  With ``emd`` (and no engine)
it runs on the host in float64 with the same tie rule: the CPU fallback, like ``LinkPredictEval``'s.
"""
import numpy as np

from .. import utils


def format_results(mode, result, ks):
    """One results line: ``<mode>:P@2=<p> R@2=<r> P@10=<p> R@10=<r> ...`` (values with ``str``, K in the order of ``ks``)."""
    return mode + ":" + " ".join("P@%d=%s R@%d=%s" % (K, str(result[K][0]), K, str(result[K][1])) for K in ks) + "\n"


def _neighbour_sets(edges, n_node):
    nb = [set() for _ in range(n_node)]
    for a, b in edges:
        nb[a].add(b)
        nb[b].add(a)
    return nb


def host_topk(emd, queries, train_nbrs, k):
    """float64 ranking on the host: per query the first ``k`` eligible columns (score descending, column ascending), padded
    with -1.  ``train_nbrs[u]``: the set of u's training neighbours."""
    emd = np.asarray(emd, dtype=np.float64)
    out = np.full((len(queries), k), -1, dtype=np.int64)
    for i, u in enumerate(queries):
        s = emd @ emd[u]
        elig = np.ones(len(s), dtype=bool)
        elig[u] = False
        if train_nbrs[u]:
            elig[np.fromiter(train_nbrs[u], dtype=np.int64)] = False
        idx = np.flatnonzero(elig)
        top = idx[np.lexsort((idx, -s[idx]))[:k]]
        out[i, :len(top)] = top
    return out


def precision_recall(ranked, queries, test_nbrs, ks):
    """{K: (P@K, R@K)} of ranked columns ``ranked[i]`` (best first) of ``queries[i]`` against the test neighbour sets."""
    res = {}
    for K in ks:
        p = r = 0.0
        for i, u in enumerate(queries):
            t = test_nbrs[u]
            hit = sum(1 for c in ranked[i, :K].tolist() if c in t)
            p += hit / K
            r += hit / len(t)
        res[K] = (p / len(queries), r / len(queries)) if len(queries) else (0.0, 0.0)
    return res


class RecommendEval(object):
    def __init__(self, embed_filename, train_filename, test_filename, n_node, n_embed, emd=None, engine=None, which=0,
                 ks=(2, 10, 20), precision="fp32"):
        self.embed_filename = embed_filename
        self.train_filename = train_filename
        self.test_filename = test_filename
        self.n_node = n_node
        self.n_embed = n_embed
        self.ks = tuple(int(K) for K in ks)
        if not self.ks or min(self.ks) < 1 or max(self.ks) > 256:
            raise ValueError("RecommendEval: every K must lie in [1, 256], got %r" % (ks,))
        self.precision = precision
        # ``engine`` (+ ``which``): the ranking runs on the device against the engine's resident training graph; otherwise
        # on ``emd`` (float64 [n_node, n_embed]) or the re-read ``.emb`` text, against the training file
        self.engine, self.which = engine, which
        if engine is not None:
            self.emd = None
        else:
            self.emd = emd if emd is not None else utils.read_embeddings(embed_filename, n_node=n_node, n_embed=n_embed)

    def eval_recommendation(self):
        test_nbrs = _neighbour_sets(utils.read_edges_from_file(self.test_filename), self.n_node)
        queries = np.array([u for u in range(self.n_node) if test_nbrs[u]], dtype=np.int64)
        kmax = max(self.ks)
        if len(queries) == 0:
            return {K: (0.0, 0.0) for K in self.ks}
        if self.engine is not None:
            ranked = self.engine.topk(queries, k=kmax, which=self.which, precision=self.precision, exclude=True)["col"]
        else:
            train_nbrs = _neighbour_sets(utils.read_edges_from_file(self.train_filename), self.n_node)
            ranked = host_topk(self.emd, queries, train_nbrs, kmax)
        return precision_recall(ranked, queries, test_nbrs, self.ks)
