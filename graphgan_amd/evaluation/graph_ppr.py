"""Rooted (personalised) PageRank as a graph-only ranking baseline: what ranking every node by its rooted PageRank on the TRAINING
graph alone reaches on the two ranking evaluators -- the index of Liben-Nowell & Kleinberg and of the node2vec paper that looks
further than the two hops of ``graph_ranking.py``.  No embedding takes part.

The scores come from the push sweep (include/graphgan_hip.h, "push sweep"): the local push of Andersen, Chung & Lang, done
synchronously in fixed-point integers on the neighbour SETS N(x) of ``link_heuristics.set_adjacency``.  ONE = 2^40.  With
``(alpha_q, eps_q) = quantise(alpha, eps)`` the state of a query with root u is p[x], r[x] (unsigned 64-bit), all zero except
r[u] = ONE, and a round is

    A = {x : r[x] > 0 and r[x] >= eps_q max(deg(x), 1)};  empty: converged, stop;  otherwise every x in A pushes simultaneously
    from r0 = r[x] at the START of the round:
        keep = (r0 alpha_q) >> 16  (keep = r0 where deg(x) = 0);  rest = r0 - keep;  share = rest // deg(x);  rem = rest - share deg(x)
        p[x] += keep;  r[x] = rem + (what arrives this round);  r[w] += share for every w in N(x)

until ``max_rounds`` rounds have pushed.  S(u, c) = p[c]; ``rounds``: the rounds that pushed; ``converged``: the active set after
the last round is empty; ``residual`` = sum r.  sum p + sum r == ONE after every round.  Eligibility, order and the two result
shapes are ``graph_ranking``'s: exclude True / "self", score descending, column ascending, zero-score nodes never listed, and the
rank's integers go through ``graph_ranking.full_rank`` unchanged.

With an ``engine`` the rounds run on the device (``Engine.ppr_topk`` / ``ppr_rank``, gg_ppr_topk / gg_ppr_rank); without one the
same rounds run in numpy on the training file (``host_ppr_topk`` / ``host_ppr_rank``).  Everything is an integer, so both give the
same bits and the results lines are the same strings.
"""
import numpy as np

from .. import utils
from . import graph_ranking as grank
from . import link_ranking as lrank
from . import recommendation as rec
from .generator_likelihood import edge_pairs

ONE = 1 << 40
DEFAULT_ALPHA, DEFAULT_EPS, DEFAULT_MAX_ROUNDS = 0.15, 1e-4, 200


def quantise(alpha, eps):
    """(alpha, eps) -> (alpha_q, eps_q) = (rint(alpha 2^16), max(1, rint(eps 2^40))): the ONE quantisation of the device and the
    host path.  alpha_q must lie in [1, 65535], eps_q in [1, 2^32], and alpha_q eps_q >= 65536 (a push retires at least one unit per
    unit of degree, which bounds the work)."""
    try:
        a, e = float(alpha), float(eps)
    except (TypeError, ValueError):
        raise ValueError("graph ppr: alpha and eps must be numbers, got %r and %r" % (alpha, eps))
    if not np.isfinite(a) or not np.isfinite(e):
        raise ValueError("graph ppr: alpha and eps must be finite, got %r and %r" % (alpha, eps))
    alpha_q = int(np.rint(a * 65536.0))
    if not 1 <= alpha_q <= 65535:
        raise ValueError("graph ppr: alpha = %r gives alpha_q = %d outside [1, 65535]" % (alpha, alpha_q))
    if e < 0 or e * float(ONE) >= 2.0 ** 62:
        raise ValueError("graph ppr: eps = %r gives eps_q outside [1, 4294967296]" % (eps,))
    eps_q = max(1, int(np.rint(e * float(ONE))))
    if eps_q > 1 << 32:
        raise ValueError("graph ppr: eps = %r gives eps_q = %d outside [1, 4294967296]" % (eps, eps_q))
    if alpha_q * eps_q < 65536:
        raise ValueError("graph ppr: alpha_q * eps_q = %d is below 65536 (alpha = %r, eps = %r): the work of a query would be unbounded"
                         % (alpha_q * eps_q, alpha, eps))
    return alpha_q, eps_q


def check_max_rounds(fn, max_rounds):
    if isinstance(max_rounds, (bool, np.bool_)) or not isinstance(max_rounds, (int, np.integer)) or not 1 <= int(max_rounds) <= 2 ** 31 - 1:
        raise ValueError("%s: max_rounds must be a positive integer, got %r" % (fn, max_rounds))
    return int(max_rounds)


def touched_bound(n_node, alpha_q, eps_q):
    """E = min(n_node, 1 + ONE // kmin): the distinct nodes a query can touch (the device sizes its tables from it)"""
    return min(int(n_node), 1 + ONE // ((eps_q * alpha_q) >> 16))


class _Rounds(object):
    """the rounds in numpy over two dense work arrays that are zeroed again behind every query"""

    def __init__(self, ptr, adj, alpha_q, eps_q, max_rounds):
        self.ptr, self.adj = np.asarray(ptr, dtype=np.int64), np.asarray(adj, dtype=np.int64)
        self.deg = np.diff(self.ptr).astype(np.uint64)
        self.alpha_q, self.eps_q, self.max_rounds = np.uint64(alpha_q), np.uint64(eps_q), max_rounds
        self.r = np.zeros(len(self.deg), dtype=np.uint64)
        self.p = np.zeros(len(self.deg), dtype=np.uint64)

    def run(self, u):
        """-> (cols ascending, p[cols], rounds, converged, residual, pushed entries): cols are the touched nodes"""
        r, p, deg, one = self.r, self.p, self.deg, np.uint64(1)
        r[u] = np.uint64(ONE)
        seen = [np.array([u], dtype=np.int64)]
        front = seen[0] if np.uint64(ONE) >= self.eps_q * max(deg[u], one) else seen[0][:0]
        rounds = pushed = 0
        while len(front) and rounds < self.max_rounds:
            r0, d = r[front], deg[front]
            keep = np.where(d > 0, (r0 * self.alpha_q) >> np.uint64(16), r0)
            rest = r0 - keep
            share = np.where(d > 0, rest // np.maximum(d, one), np.uint64(0))
            p[front] += keep
            r[front] = rest - share * d
            di = d.astype(np.int64)
            tot = int(di.sum())
            pos = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(di) - di, di)
            cols = self.adj[np.repeat(self.ptr[front], di) + pos]
            np.add.at(r, cols, np.repeat(share, di))
            cand = np.unique(cols)
            seen.append(cand)
            front = cand[r[cand] >= self.eps_q * deg[cand]]
            rounds += 1
            pushed += tot
        cols = np.unique(np.concatenate(seen))
        score, residual = p[cols].copy(), int(r[cols].sum())
        r[cols] = 0
        p[cols] = 0
        return cols, score, rounds, int(len(front) == 0), residual, pushed


def _args(fn, ptr, alpha, eps, max_rounds, exclude):
    alpha_q, eps_q = quantise(alpha, eps)
    return len(ptr) - 1, grank.check_exclude(fn, exclude), alpha_q, eps_q, check_max_rounds(fn, max_rounds)


def host_ppr_topk(ptr, adj, rows, k=10, alpha=DEFAULT_ALPHA, eps=DEFAULT_EPS, max_rounds=DEFAULT_MAX_ROUNDS, exclude=True):
    """``Engine.ppr_topk`` on the host -> dict(col int32 [m, k], score uint64 [m, k], n_pos int32 [m], rounds int32 [m], converged
    int32 [m], residual uint64 [m], pushed int64 [m] = the adjacency entries the query's pushes walked)."""
    fn = "host_ppr_topk"
    n_node, code, alpha_q, eps_q, max_rounds = _args(fn, ptr, alpha, eps, max_rounds, exclude)
    k = grank.check_k(fn, k)
    rows = grank.check_ids(fn, "rows", rows, n_node)
    m = len(rows)
    col = np.full((m, k), -1, dtype=np.int32)
    score = np.zeros((m, k), dtype=np.uint64)
    n_pos, rounds, converged = (np.zeros(m, dtype=np.int32) for _ in range(3))
    residual, pushed = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.int64)
    big = np.uint64(np.iinfo(np.uint64).max)
    state = _Rounds(ptr, adj, alpha_q, eps_q, max_rounds)
    for i, u in enumerate(rows.tolist()):
        c, s, rounds[i], converged[i], res, pushed[i] = state.run(u)
        residual[i] = res
        keep = grank._eligible(state.ptr, state.adj, u, c, code) & (s > 0)
        c, s = c[keep], s[keep]
        n_pos[i] = len(c)
        top = np.lexsort((c, big - s))[:k]
        col[i, :len(top)] = c[top]
        score[i, :len(top)] = s[top]
    return dict(col=col, score=score, n_pos=n_pos, rounds=rounds, converged=converged, residual=residual, pushed=pushed)


def host_ppr_rank(ptr, adj, u, v, alpha=DEFAULT_ALPHA, eps=DEFAULT_EPS, max_rounds=DEFAULT_MAX_ROUNDS, exclude=True):
    """``Engine.ppr_rank`` on the host -> dict(rank int64 [m], n_cand int64 [m], score uint64 [m], ahead, n_pos, pos_below, rounds,
    converged int32 [m], residual uint64 [m]).  The rounds of a root run once, however many of its queries the request holds."""
    fn = "host_ppr_rank"
    n_node, code, alpha_q, eps_q, max_rounds = _args(fn, ptr, alpha, eps, max_rounds, exclude)
    u, v = grank.check_ids(fn, "u", u, n_node), grank.check_ids(fn, "v", v, n_node)
    if len(u) != len(v):
        raise ValueError("%s: u and v must have the same length, got %d and %d" % (fn, len(u), len(v)))
    m = len(u)
    score, residual = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    ahead, n_pos, pos_below, rounds, converged = (np.zeros(m, dtype=np.int32) for _ in range(5))
    state = _Rounds(ptr, adj, alpha_q, eps_q, max_rounds)
    order = np.argsort(u, kind="stable")
    last, row = -1, None
    for i in order.tolist():
        a, b = int(u[i]), int(v[i])
        if a != last:
            last, row = a, state.run(a)
            ok = grank._eligible(state.ptr, state.adj, a, row[0], code) & (row[1] > 0)
        c, s = row[0], row[1]
        at = np.searchsorted(c, b)
        sv = s[at] if at < len(c) and c[at] == b else np.uint64(0)
        keep = ok & (c != b)
        c, s = c[keep], s[keep]
        score[i], rounds[i], converged[i], residual[i] = sv, row[2], row[3], row[4]
        n_pos[i] = len(c)
        ahead[i] = int(((s > sv) | ((s == sv) & (c < b))).sum())
        pos_below[i] = int((c < b).sum())
    rank, n_cand = grank.full_rank(state.ptr, state.adj, u, v, code, score, ahead, n_pos, pos_below)
    return dict(rank=rank, n_cand=n_cand, score=score, ahead=ahead, n_pos=n_pos, pos_below=pos_below, rounds=rounds, converged=converged, residual=residual)


def format_results(kind, result, ks, alpha, eps):
    """One results line (values with ``str``, K in the order of ``ks``):
    kind "rank"  ``graph_rank:index=ppr MRR=<m> MR=<r> H@1=<h> ... n=<n> reach=<r> alpha=<a> eps=<e> rounds=<largest> converged=<share
                 of queries> residual=<mean residual / 2^40>``
    kind "rec"   ``graph_rec:index=ppr P@2=<p> R@2=<r> ... alpha=<a> eps=<e>``"""
    line = grank.format_results(kind, "ppr", result, ks)[:-1] + " alpha=%s eps=%s" % (str(alpha), str(eps))
    if kind == "rank":
        line += " rounds=%s converged=%s residual=%s" % (str(result["rounds"]), str(result["converged"]), str(result["residual"]))
    return line + "\n"


class _PprEval(grank._GraphEval):
    def __init__(self, train_filename, test_filename, n_node, engine, alpha, eps, max_rounds):
        super(_PprEval, self).__init__(train_filename, test_filename, n_node, engine, grank.INDICES)
        quantise(alpha, eps)
        self.alpha, self.eps = alpha, eps
        self.max_rounds = check_max_rounds(type(self).__name__, max_rounds)


class GraphPprRankEval(_PprEval):
    """The ``graph_rank:index=ppr`` line: the queries of ``LinkRankEval`` (every test edge in both directions, ``exclude=True``),
    sorted by their first node so that a root is pushed once, ranked by the push sweep; filtered ranks and their summary by
    ``link_ranking``; ``reach``: the share of queries with score > 0."""

    def __init__(self, train_filename, test_filename, n_node, engine=None, ks=lrank.DEFAULT_KS, alpha=DEFAULT_ALPHA, eps=DEFAULT_EPS,
                 max_rounds=DEFAULT_MAX_ROUNDS):
        super(GraphPprRankEval, self).__init__(train_filename, test_filename, n_node, engine, alpha, eps, max_rounds)
        ks = tuple(ks)
        if not ks or any(isinstance(K, bool) or int(K) != K or int(K) < 1 for K in ks):
            raise ValueError("GraphPprRankEval: every K must be a positive integer, got %r" % (ks,))
        self.ks = tuple(int(K) for K in ks)

    def sweep(self, u, v):
        if self.engine is not None:
            return self.engine.ppr_rank(u, v, alpha=self.alpha, eps=self.eps, max_rounds=self.max_rounds, exclude=True)
        ptr, adj = self.adjacency()
        return host_ppr_rank(ptr, adj, u, v, self.alpha, self.eps, self.max_rounds, True)

    def eval_graph_ranking(self):
        """dict(mrr, mr, hits, n, reach, rounds, converged, residual)"""
        pairs = edge_pairs(self.test_filename)
        pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
        res = self.sweep(pairs[:, 0], pairs[:, 1])
        r = lrank.summarize(lrank.filtered_ranks(pairs[:, 0], pairs[:, 1], res["rank"]), self.ks)
        n = len(pairs)
        r["reach"] = float(int((res["score"] > 0).sum())) / n if n else 0.0
        r["rounds"] = int(res["rounds"].max()) if n else 0
        r["converged"] = float(int(res["converged"].sum())) / n if n else 0.0
        r["residual"] = float(int(res["residual"].astype(np.uint64).sum())) / n / float(ONE) if n else 0.0
        return r

    def lines(self):
        return [format_results("rank", self.eval_graph_ranking(), self.ks, self.alpha, self.eps)]


class GraphPprRecEval(_PprEval):
    """The ``graph_rec:index=ppr`` line: the queries and the scoring of ``RecommendEval`` (every node with a test edge; P@K / R@K of
    the first K of one list of max(ks)), the lists from the push sweep with ``exclude=True``; a -1 column is a miss."""

    def __init__(self, train_filename, test_filename, n_node, engine=None, ks=(2, 10, 20), alpha=DEFAULT_ALPHA, eps=DEFAULT_EPS, max_rounds=DEFAULT_MAX_ROUNDS):
        super(GraphPprRecEval, self).__init__(train_filename, test_filename, n_node, engine, alpha, eps, max_rounds)
        ks = tuple(ks)
        if not ks or any(isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= grank.MAX_K for K in ks):
            raise ValueError("GraphPprRecEval: every K must lie in [1, %d], got %r" % (grank.MAX_K, ks))
        self.ks = tuple(int(K) for K in ks)

    def sweep(self, queries, k):
        if self.engine is not None:
            return self.engine.ppr_topk(queries, k=k, alpha=self.alpha, eps=self.eps, max_rounds=self.max_rounds, exclude=True)
        ptr, adj = self.adjacency()
        return host_ppr_topk(ptr, adj, queries, k, self.alpha, self.eps, self.max_rounds, True)

    def eval_graph_recommendation(self):
        """{K: (P@K, R@K)}"""
        test_nbrs = rec._neighbour_sets(utils.read_edges_from_file(self.test_filename), self.n_node)
        queries = np.array([u for u in range(self.n_node) if test_nbrs[u]], dtype=np.int64)
        if len(queries) == 0:
            return {K: (0.0, 0.0) for K in self.ks}
        return rec.precision_recall(self.sweep(queries, max(self.ks))["col"], queries, test_nbrs, self.ks)

    def lines(self):
        return [format_results("rec", self.eval_graph_recommendation(), self.ks, self.alpha, self.eps)]
