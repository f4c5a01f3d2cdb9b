"""Graph-only ranking baselines: what ranking every node by a neighbourhood index on the TRAINING graph alone reaches on the two
ranking evaluators (``link_ranking.py``: MRR / MR / Hits@K; ``recommendation.py``: P@K / R@K) -- no embedding takes part.

N(x) is the neighbour SET of x in the training graph (``link_heuristics.set_adjacency``: distinct, without x itself).  For a
query node u the two-hop sweep gives one row of A W A:

    S(u, c) = sum over w in N(u) & N(c) of weights[w]          (unsigned 64-bit integers; no weights: every weight 1)

which is the ``cn`` / ``wsum`` of ``pair_neighbors`` for the pair (u, c), also at c == u.  ``index_weights``: "cn" -> None, "aa" /
"ra" -> the fixed-point weights of ``link_heuristics.node_weights`` (rint(2^40 / ln deg), rint(2^40 / deg)).

Eligible candidates: ``exclude="self"`` every c != u; ``exclude=True`` every c outside N(u) + {u} (those of ``Engine.topk(...,
exclude=True)``).  ``exclude=False`` is refused: S(u, u) >= S(u, c) for every c, so u would rank first for itself.  The order is
score descending, column ascending (``Engine.topk`` / ``Engine.rank``).

    two_hop_topk   per query the first k eligible candidates with S > 0 (padding: col -1, score 0) and n_pos, the number of
                   eligible candidates with S > 0.  Zero-score nodes never enter a list: they would fill it by node id.
    two_hop_rank   per query (u, v), over the eligible c != v (the target itself is always a candidate): score = S(u, v),
                   n_pos = |{c : S > 0}|, ahead = |{c : S > 0, (S, -c) > (S(u, v), -v)}|, pos_below = |{c : S > 0, c < v}|, and
                   from them by ``full_rank`` -- ONE function for the device and the host path -- the position of v in the total
                   order over ALL candidates: 1 + ahead if score > 0, else 1 + n_pos + (the eligible c < v) - pos_below.  The
                   zero-score nodes are counted by a searchsorted in the excluded set, never visited.

With an ``engine`` the sweeps run on the device on its resident training graph (``Engine.two_hop_topk`` / ``two_hop_rank``,
gg_two_hop_topk / gg_two_hop_rank); without one the same integers come from numpy on the training file (``host_two_hop_topk`` /
``host_two_hop_rank``).  Everything is an integer, so both give the same bits and the results lines are the same strings.
"""
import numpy as np

from .. import utils
from . import link_heuristics as lheur
from . import link_ranking as lrank
from . import recommendation as rec
from .generator_likelihood import edge_pairs

INDICES = ("cn", "aa", "ra")
MAX_K = 256  # == TH_MAX_K of csrc/two_hop.hip


def index_weights(index, deg):
    """The node weights of a ranking index from the distinct degrees: None for "cn", uint64 [n_node] for "aa" / "ra"."""
    if index not in INDICES:
        raise ValueError("graph ranking: index must be one of 'cn', 'aa', 'ra', got %r" % (index,))
    if index == "cn":
        return None
    return np.ascontiguousarray(lheur.node_weights(deg)[INDICES.index(index) - 1])


def check_exclude(fn, exclude):
    """-> the ABI's code: 2 for True (u and its training neighbours), 1 for "self" (u alone)"""
    if exclude is True:
        return 2
    if isinstance(exclude, str) and exclude == "self":
        return 1
    if exclude is False:
        raise ValueError("%s: exclude must be True or 'self', got False: S(u, u) >= S(u, c) for every c, so u would rank first for itself" % fn)
    raise ValueError("%s: exclude must be True or 'self', got %r" % (fn, exclude))


def check_k(fn, k):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (fn, MAX_K, k))
    return int(k)


def check_weights(fn, weights, n_node):
    if weights is None:
        return None
    w = np.asarray(weights)
    if w.shape != (n_node,) or not np.issubdtype(w.dtype, np.integer) or (w.size and int(w.min()) < 0):
        raise ValueError("%s: weights must be None or %d non-negative integers" % (fn, n_node))
    return np.ascontiguousarray(w, dtype=np.uint64)


def check_ids(fn, name, ids, n_node):
    a = np.asarray(ids)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: %s must hold integers" % (fn, name))
    a = a.astype(np.int64).reshape(-1)
    bad = np.flatnonzero((a < 0) | (a >= n_node))
    if len(bad):
        raise ValueError("%s: %s[%d] = %d out of range [0, %d)" % (fn, name, bad[0], a[bad[0]], n_node))
    return a


def check_pair_k(fn, k):
    """the k of the two-hop pair sweep (graph_pairs.py, Engine.two_hop_top_pairs): an integer in [1, 2^20]"""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 1 << 20:
        raise ValueError("%s: k must be an integer in [1, 2^20], got %r" % (fn, k))
    return int(k)


def check_ascending_ids(fn, name, ids, n_node):
    """ids in [0, n_node), strictly ascending -> int64 array (the node set of the two-hop pair sweep)"""
    a = check_ids(fn, name, ids, n_node)
    bad = np.flatnonzero(np.diff(a) <= 0)
    if len(bad):
        i = int(bad[0]) + 1
        raise ValueError("%s: %s[%d] = %d is not above %s[%d] = %d (strictly ascending ids)" % (fn, name, i, a[i], name, i - 1, a[i - 1]))
    return a


def check_scratch(fn, scratch_bytes):
    if scratch_bytes is None:
        return 0
    if isinstance(scratch_bytes, (bool, np.bool_)) or not isinstance(scratch_bytes, (int, np.integer)) or int(scratch_bytes) < 1:
        raise ValueError("%s: scratch_bytes must be None or a positive integer, got %r" % (fn, scratch_bytes))
    return int(scratch_bytes)


def _row(ptr, adj, u, w):
    """the reached nodes of query u (ascending, u itself among them) and their sums"""
    nb = adj[ptr[u]:ptr[u + 1]]
    deg = ptr[nb + 1] - ptr[nb]
    tot = int(deg.sum())
    if tot == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64)
    pos = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg)
    cols = adj[np.repeat(ptr[nb], deg) + pos]
    wt = np.repeat(np.ones(len(nb), dtype=np.uint64) if w is None else w[nb], deg)
    uc, inv = np.unique(cols, return_inverse=True)
    s = np.zeros(len(uc), dtype=np.uint64)
    np.add.at(s, inv.reshape(-1), wt)
    return uc.astype(np.int64), s


def _eligible(ptr, adj, u, cols, code):
    ok = cols != u
    if code == 2:
        ok &= ~np.isin(cols, adj[ptr[u]:ptr[u + 1]])
    return ok


def host_two_hop_topk(ptr, adj, rows, k=10, weights=None, exclude=True):
    """``Engine.two_hop_topk`` on the host -> dict(col int32 [m, k], score uint64 [m, k], n_pos int32 [m])."""
    fn = "host_two_hop_topk"
    n_node = len(ptr) - 1
    code, k = check_exclude(fn, exclude), check_k(fn, k)
    rows = check_ids(fn, "rows", rows, n_node)
    w = check_weights(fn, weights, n_node)
    col = np.full((len(rows), k), -1, dtype=np.int32)
    score = np.zeros((len(rows), k), dtype=np.uint64)
    n_pos = np.zeros(len(rows), dtype=np.int32)
    big = np.uint64(np.iinfo(np.uint64).max)
    for i, u in enumerate(rows.tolist()):
        c, s = _row(ptr, adj, u, w)
        keep = _eligible(ptr, adj, u, c, code) & (s > 0)
        c, s = c[keep], s[keep]
        n_pos[i] = len(c)
        top = np.lexsort((c, big - s))[:k]
        col[i, :len(top)] = c[top]
        score[i, :len(top)] = s[top]
    return dict(col=col, score=score, n_pos=n_pos)


def full_rank(ptr, adj, u, v, code, score, ahead, n_pos, pos_below):
    """The position of every target in the total order over ALL its candidates, and their number, from the sweep's outputs
    -> (rank int64 [m], n_cand int64 [m]).  excl(u) = {u} (code 1) or N(u) + {u} (code 2), without the target v; the eligible
    c < v are v minus the excluded ids below v: a searchsorted in the sorted lists (row * n_node + id ascends over ``adj``)."""
    u, v = np.asarray(u, dtype=np.int64).reshape(-1), np.asarray(v, dtype=np.int64).reshape(-1)
    n_node = len(ptr) - 1
    score, ahead, n_pos, pos_below = (np.asarray(x).astype(np.int64 if i else np.uint64) for i, x in enumerate((score, ahead, n_pos, pos_below)))
    excl_below = (u < v).astype(np.int64)
    n_excl = (u != v).astype(np.int64)
    if code == 2 and len(u):
        key = np.repeat(np.arange(n_node, dtype=np.int64), np.diff(ptr)) * n_node + adj
        at = np.searchsorted(key, u * n_node + v)
        member = np.zeros(len(u), dtype=bool)
        inside = at < len(key)
        member[inside] = key[at[inside]] == (u * n_node + v)[inside]
        excl_below += at - ptr[u]
        n_excl += (ptr[u + 1] - ptr[u]) - member
    e_below = v - excl_below
    rank = np.where(score > 0, 1 + ahead, 1 + n_pos + (e_below - pos_below))
    return rank.astype(np.int64), (n_node - n_excl).astype(np.int64)


def host_two_hop_rank(ptr, adj, u, v, weights=None, exclude=True):
    """``Engine.two_hop_rank`` on the host -> dict(rank int64 [m], n_cand int64 [m], score uint64 [m], ahead int32 [m], n_pos int32
    [m], pos_below int32 [m])."""
    fn = "host_two_hop_rank"
    n_node = len(ptr) - 1
    code = check_exclude(fn, exclude)
    u, v = check_ids(fn, "u", u, n_node), check_ids(fn, "v", v, n_node)
    if len(u) != len(v):
        raise ValueError("%s: u and v must have the same length, got %d and %d" % (fn, len(u), len(v)))
    w = check_weights(fn, weights, n_node)
    m = len(u)
    score = np.zeros(m, dtype=np.uint64)
    ahead, n_pos, pos_below = (np.zeros(m, dtype=np.int32) for _ in range(3))
    for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        c, s = _row(ptr, adj, a, w)
        at = np.flatnonzero(c == b)
        sv = s[at[0]] if len(at) else np.uint64(0)
        keep = _eligible(ptr, adj, a, c, code) & (c != b) & (s > 0)
        c, s = c[keep], s[keep]
        score[i] = sv
        n_pos[i] = len(c)
        ahead[i] = int(((s > sv) | ((s == sv) & (c < b))).sum())
        pos_below[i] = int((c < b).sum())
    rank, n_cand = full_rank(ptr, adj, u, v, code, score, ahead, n_pos, pos_below)
    return dict(rank=rank, n_cand=n_cand, score=score, ahead=ahead, n_pos=n_pos, pos_below=pos_below)


def format_results(kind, index, result, ks):
    """One results line (values with ``str``, K in the order of ``ks``):
    kind "rank"  ``graph_rank:index=<i> MRR=<m> MR=<r> H@1=<h> ... n=<n> reach=<r>``
    kind "rec"   ``graph_rec:index=<i> P@2=<p> R@2=<r> ...``"""
    if kind == "rank":
        hits = " ".join("H@%d=%s" % (K, str(result["hits"][K])) for K in ks)
        return "graph_rank:index=%s MRR=%s MR=%s %s n=%s reach=%s\n" % (index, str(result["mrr"]), str(result["mr"]), hits, str(result["n"]), str(result["reach"]))
    if kind == "rec":
        return "graph_rec:index=%s " % index + " ".join("P@%d=%s R@%d=%s" % (K, str(result[K][0]), K, str(result[K][1])) for K in ks) + "\n"
    raise ValueError("graph ranking: kind must be 'rank' or 'rec', got %r" % (kind,))


def check_indices(indices):
    indices = (indices,) if isinstance(indices, str) else tuple(indices)
    if not indices:
        raise ValueError("graph ranking: at least one index of 'cn', 'aa', 'ra' is needed")
    for index in indices:
        index_weights(index, np.zeros(0))
    return indices


class _GraphEval(object):
    def __init__(self, train_filename, test_filename, n_node, engine=None, indices=INDICES):
        self.train_filename, self.test_filename = train_filename, test_filename
        self.n_node = int(n_node)
        # ``engine``: the sweep runs on the device on its resident training graph; otherwise in numpy on the training file
        self.engine = engine
        self.indices = check_indices(indices)
        self._adj = None

    def degrees(self):
        if self.engine is not None:
            return self.engine.distinct_degrees()
        return np.diff(self.adjacency()[0])

    def adjacency(self):
        if self._adj is None:
            self._adj = lheur.set_adjacency(utils.read_edges_from_file(self.train_filename), self.n_node)
        return self._adj


class GraphRankEval(_GraphEval):
    """The ``graph_rank`` lines: the queries of ``LinkRankEval`` (every test edge in both directions, ``exclude=True``), ranked by
    the two-hop sweep; filtered ranks and their summary by ``link_ranking``; ``reach``: the share of queries with score > 0."""

    def __init__(self, train_filename, test_filename, n_node, engine=None, indices=INDICES, ks=lrank.DEFAULT_KS):
        super(GraphRankEval, self).__init__(train_filename, test_filename, n_node, engine, indices)
        ks = tuple(ks)
        if not ks or any(isinstance(K, bool) or int(K) != K or int(K) < 1 for K in ks):
            raise ValueError("GraphRankEval: every K must be a positive integer, got %r" % (ks,))
        self.ks = tuple(int(K) for K in ks)

    def sweep(self, u, v, weights):
        if self.engine is not None:
            return self.engine.two_hop_rank(u, v, weights=weights, exclude=True)
        ptr, adj = self.adjacency()
        return host_two_hop_rank(ptr, adj, u, v, weights, True)

    def eval_graph_ranking(self):
        """{index: dict(mrr, mr, hits, n, reach)}"""
        pairs = edge_pairs(self.test_filename)
        deg = self.degrees()
        out = {}
        for index in self.indices:
            res = self.sweep(pairs[:, 0], pairs[:, 1], index_weights(index, deg))
            r = lrank.summarize(lrank.filtered_ranks(pairs[:, 0], pairs[:, 1], res["rank"]), self.ks)
            r["reach"] = float(int((res["score"] > 0).sum())) / len(pairs) if len(pairs) else 0.0
            out[index] = r
        return out

    def lines(self):
        res = self.eval_graph_ranking()
        return [format_results("rank", index, res[index], self.ks) for index in self.indices]


class GraphRecEval(_GraphEval):
    """The ``graph_rec`` lines: the queries and the scoring of ``RecommendEval`` (every node with a test edge; P@K / R@K of the
    first K of one list of max(ks)), the lists from the two-hop sweep with ``exclude=True``; a -1 column is a miss."""

    def __init__(self, train_filename, test_filename, n_node, engine=None, indices=INDICES, ks=(2, 10, 20)):
        super(GraphRecEval, self).__init__(train_filename, test_filename, n_node, engine, indices)
        ks = tuple(ks)
        if not ks or any(isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= MAX_K for K in ks):
            raise ValueError("GraphRecEval: every K must lie in [1, %d], got %r" % (MAX_K, ks))
        self.ks = tuple(int(K) for K in ks)

    def sweep(self, queries, k, weights):
        if self.engine is not None:
            return self.engine.two_hop_topk(queries, k=k, weights=weights, exclude=True)
        ptr, adj = self.adjacency()
        return host_two_hop_topk(ptr, adj, queries, k, weights, True)

    def eval_graph_recommendation(self):
        """{index: {K: (P@K, R@K)}}"""
        test_nbrs = rec._neighbour_sets(utils.read_edges_from_file(self.test_filename), self.n_node)
        queries = np.array([u for u in range(self.n_node) if test_nbrs[u]], dtype=np.int64)
        deg = self.degrees()
        out = {}
        for index in self.indices:
            if len(queries) == 0:
                out[index] = {K: (0.0, 0.0) for K in self.ks}
                continue
            ranked = self.sweep(queries, max(self.ks), index_weights(index, deg))["col"]
            out[index] = rec.precision_recall(ranked, queries, test_nbrs, self.ks)
        return out

    def lines(self):
        res = self.eval_graph_recommendation()
        return [format_results("rec", index, res[index], self.ks) for index in self.indices]
