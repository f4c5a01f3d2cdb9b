"""Full-ranking link evaluation: the exact position of every held-out edge among ALL candidate nodes (MRR, mean rank, Hits@K).

Every test edge is a query in both directions, (a, b) and (b, a), as in ``generator_likelihood.py``.  For a query (u, v)
the nodes are ranked by s(u, c) = E[u] . E[c] (no bias; the link-prediction score, ``link_prediction.py``), score
descending and column ascending, over the candidates: every node except u itself and u's neighbours in the training graph
-- and always the target v.  No negatives file is read.

    rank(u, v)          = 1 + the number of candidates c != v ahead of v
    filtered_rank(u, v) = rank(u, v) - |{v' in T(u), v' != v : rank(u, v') < rank(u, v)}|      T(u): the test neighbours of u

(the other test neighbours of the same source must not push a target down; the ranks of one source are positions in one
total order, so the correction needs no scores).  Over the filtered ranks r of all queries:

    MRR = mean 1 / r,        MR = mean r,        H@K = mean [r <= K]        (K: any positive integers, not capped)

With an ``engine`` the ranks are ONE call of ``Engine.rank`` (``exclude=True`` against the engine's resident training graph:
a streamed count on the device, nothing of size queries x N exists).  With ``emd`` (and no engine) they are computed on the
host in float64 with the same order and tie rule, chunked over the queries: the CPU fallback, like ``RecommendEval``'s.
"""
import numpy as np

from .. import utils
from .generator_likelihood import edge_pairs

DEFAULT_KS = (1, 10, 100)


def format_results(mode, result, ks):
    """One results line: ``<mode>_rank:MRR=<m> MR=<r> H@1=<h> H@10=<h> ... n=<n>`` (values with ``str``, K in the order of ``ks``)."""
    hits = " ".join("H@%d=%s" % (K, str(result["hits"][K])) for K in ks)
    return "%s_rank:MRR=%s MR=%s %s n=%s\n" % (mode, str(result["mrr"]), str(result["mr"]), hits, str(result["n"]))


def train_csr(train_edges, n_node):
    """(rowptr, col) of the undirected training graph, every list sorted (duplicates stay: they are skipped where it matters)."""
    e = np.asarray(train_edges, dtype=np.int64).reshape(-1, 2)
    src = np.concatenate([e[:, 0], e[:, 1]])
    dst = np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((dst, src))
    rowptr = np.zeros(n_node + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n_node), out=rowptr[1:])
    return rowptr, dst[order]


def host_rank(score_rows, u, v, n_node, graph=None, chunk=256):
    """Ranks of the queries (u[i], v[i]) from score rows on the host.  ``score_rows(nodes)`` returns the rows S[nodes, :]
    ([len(nodes), n_node], any float dtype); ``graph`` = (rowptr, col) of the training graph excludes u and its neighbours
    (None: every node is a candidate).  Same order and tie rule as the device (score descending, column ascending, -0 == +0).
    Returns (rank int64 [m], n_cand int64 [m], score [m] in the dtype of the rows)."""
    u = np.asarray(u, dtype=np.int64).reshape(-1)
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    m = len(u)
    rank = np.zeros(m, dtype=np.int64)
    n_cand = np.zeros(m, dtype=np.int64)
    score = None
    cols = np.arange(n_node, dtype=np.int64)
    for c0 in range(0, m, chunk):
        uu, vv = u[c0:c0 + chunk], v[c0:c0 + chunk]
        S = np.asarray(score_rows(uu))
        if score is None:
            score = np.zeros(m, dtype=S.dtype)
        idx = np.arange(len(uu))
        sv = S[idx, vv]
        ahead = (S > sv[:, None]) | ((S == sv[:, None]) & (cols[None, :] < vv[:, None]))
        excl = np.zeros(S.shape, dtype=bool)
        if graph is not None:
            rowptr, col = graph
            deg = (rowptr[uu + 1] - rowptr[uu]).astype(np.int64)
            if deg.sum():
                pos = np.arange(deg.sum(), dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg)
                excl[np.repeat(idx, deg), col[np.repeat(rowptr[uu], deg) + pos]] = True
            excl[idx, uu] = True
        excl[idx, vv] = False  # the target is always a candidate
        rank[c0:c0 + chunk] = 1 + (ahead & ~excl).sum(axis=1)
        n_cand[c0:c0 + chunk] = n_node - excl.sum(axis=1)
        score[c0:c0 + chunk] = sv
    return rank, n_cand, (score if score is not None else np.zeros(0))


def filtered_ranks(u, v, rank):
    """rank(u, v) minus the number of OTHER test neighbours v' of the same source with rank(u, v') < rank(u, v); a pair that
    occurs several times among the queries is one test neighbour.  Vectorised over a sort by (u, rank)."""
    u = np.asarray(u, dtype=np.int64).reshape(-1)
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    rank = np.asarray(rank, dtype=np.int64).reshape(-1)
    if len(u) == 0:
        return rank.copy()
    pairs, first, inverse = np.unique(np.stack([u, v], axis=1), axis=0, return_index=True, return_inverse=True)
    pu, pr = pairs[:, 0], rank[first]
    order = np.lexsort((pr, pu))
    su, sr = pu[order], pr[order]
    pos = np.arange(len(order), dtype=np.int64)
    new_u = np.r_[True, su[1:] != su[:-1]]
    new_run = new_u | np.r_[True, sr[1:] != sr[:-1]]  # a run: the pairs of one source with one rank
    group_start = np.maximum.accumulate(np.where(new_u, pos, 0))
    run_start = np.maximum.accumulate(np.where(new_run, pos, 0))
    less = np.empty(len(order), dtype=np.int64)
    less[order] = run_start - group_start
    return rank - less[inverse.reshape(-1)]


def summarize(ranks, ks=DEFAULT_KS):
    """dict(mrr, mr, hits={K: H@K}, n) of (filtered) ranks: float64 means of integers."""
    r = np.asarray(ranks, dtype=np.int64).reshape(-1)
    n = int(len(r))
    if n == 0:
        return dict(mrr=0.0, mr=0.0, hits={int(K): 0.0 for K in ks}, n=0)
    return dict(mrr=float(np.mean(1.0 / r.astype(np.float64))), mr=float(r.sum()) / n,
                hits={int(K): float(int((r <= int(K)).sum())) / n for K in ks}, n=n)


class LinkRankEval(object):
    def __init__(self, embed_filename, train_filename, test_filename, n_node, n_embed, emd=None, engine=None, which=0,
                 ks=DEFAULT_KS, precision="fp32"):
        self.embed_filename = embed_filename
        self.train_filename = train_filename
        self.test_filename = test_filename
        self.n_node = n_node
        self.n_embed = n_embed
        ks = tuple(ks)
        if not ks or any(isinstance(K, bool) or int(K) != K or int(K) < 1 for K in ks):
            raise ValueError("LinkRankEval: every K must be a positive integer, got %r" % (ks,))
        self.ks = tuple(int(K) for K in ks)
        if precision not in ("fp32", "bf16"):
            raise ValueError("LinkRankEval: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        self.precision = precision
        # ``engine`` (+ ``which``): the ranks are counted on the device against the engine's resident training graph; otherwise
        # on ``emd`` (float64 [n_node, n_embed]) or the re-read ``.emb`` text, against the training file
        self.engine, self.which = engine, which
        if engine is not None:
            self.emd = None
        else:
            self.emd = emd if emd is not None else utils.read_embeddings(embed_filename, n_node=n_node, n_embed=n_embed)

    def pair_ranks(self, pairs):
        """unfiltered rank of every (u, v) query -> int64 [m]"""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) == 0:
            return np.zeros(0, dtype=np.int64)
        if self.engine is not None:
            res = self.engine.rank(pairs[:, 0], pairs[:, 1], which=self.which, precision=self.precision, exclude=True)
            return res["rank"].astype(np.int64)
        emd = np.asarray(self.emd, dtype=np.float64)
        graph = train_csr(utils.read_edges_from_file(self.train_filename), self.n_node)
        return host_rank(lambda nodes: emd[nodes] @ emd.T, pairs[:, 0], pairs[:, 1], self.n_node, graph)[0]

    def eval_link_ranking(self):
        pairs = edge_pairs(self.test_filename)
        ranks = filtered_ranks(pairs[:, 0], pairs[:, 1], self.pair_ranks(pairs))
        return summarize(ranks, self.ks)
