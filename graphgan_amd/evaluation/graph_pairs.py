"""Graph-only global top-K pair baseline: what "the K pairs with the largest neighbourhood index" reach on the two protocols of
``pair_prediction.py`` -- the graph-only lines the ``*_pairs`` / ``*_recon`` lines stand on.  No embedding takes part.

N(x) is the neighbour SET of x in the training graph (``link_heuristics.set_adjacency``: distinct, without x itself).  The two-hop
pair sweep ranks ALL unordered pairs at once:

    score        S(u, v) = sum over w in N(u) & N(v) of weights[w]      (unsigned 64-bit integers; no weights: every weight 1) --
                 the ``cn`` / ``wsum`` of ``pair_neighbors``, the score of ``two_hop_rank``.  w ranges over the WHOLE graph; only
                 the endpoints are restricted by ``nodes``.
    candidates   the pairs {u, v}, u < v, both in ``nodes`` (None: every node; else ids, strictly ascending), with S(u, v) > 0 and,
                 with ``exclude``, v not in N(u).  ``exclude=False`` keeps the edges: u < v rules out the self pair.  Zero-score
                 pairs never enter: they would fill the list by id.
    order        score descending, then (u, v) ascending: total and integer.
    output       the first k (1 <= k <= 2^20) triples; n_found = min(k, candidates); padding -1, -1, 0.

``index_weights`` (``graph_ranking``): "cn" -> None, "aa" / "ra" -> the fixed-point weights of ``link_heuristics.node_weights``.
Rooted PageRank is not symmetric in (u, v) and is no index here.

With an ``engine`` the sweep runs on the device on its resident training graph (``Engine.two_hop_top_pairs``,
gg_two_hop_top_pairs: a floor consumer on the filled table of the two-hop sweep); without one ``host_two_hop_top_pairs`` runs the
same integer rules in numpy on the training file.  Everything is an integer, so both give the same bits and the results lines are
the same strings.

    graph_pairs:index=<i> P@<k>=<p> R@<k>=<r> ... n_test=<t> dropped=<d> n=<m> found=<f>     (training edges dropped; held-out edges positive)
    graph_recon:index=<i> P@<k>=<p> R@<k>=<r> ... edges=<e> n=<m> found=<f>                  (nothing dropped; training edges positive)

Positives, ``dropped``, ``nodes`` (the nodes with a training edge) and P@K / R@K are exactly those of ``PairPredictionEval``."""
import numpy as np

from .. import utils
from . import graph_ranking as grank
from . import link_heuristics as lheur
from . import pair_prediction as ppair
from .embedding_spectrum import trained_nodes

INDICES = grank.INDICES
MAX_K = 1 << 20  # the limit of gg_two_hop_top_pairs (graph_ranking.check_pair_k)


def host_two_hop_top_pairs(ptr, adj, k, nodes=None, weights=None, exclude=True):
    """``Engine.two_hop_top_pairs`` on the host, source by source (``graph_ranking``'s row expansion); between sources only the
    k best so far are kept -> dict(u int32 [k], v int32 [k], score uint64 [k] (-1, -1, 0 behind n_found), n_found)."""
    fn = "host_two_hop_top_pairs"
    n_node = len(ptr) - 1
    k = grank.check_pair_k(fn, k)
    if not isinstance(exclude, (bool, np.bool_)):
        raise ValueError("%s: exclude must be True or False, got %r" % (fn, exclude))
    w = grank.check_weights(fn, weights, n_node)
    ids = None if nodes is None else grank.check_ascending_ids(fn, "nodes", nodes, n_node)
    member = np.ones(n_node, dtype=bool)
    if ids is None:
        ids = np.arange(n_node, dtype=np.int64)
    else:
        member[:] = False
        member[ids] = True
    big = np.uint64(np.iinfo(np.uint64).max)
    best = [np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.int64)]
    held = [[], [], []]
    n_held = 0

    def merge():
        s, a, b = (np.concatenate([best[i]] + held[i]) for i in range(3))
        o = np.lexsort((b, a, big - s))[:k]
        best[0], best[1], best[2] = s[o], a[o], b[o]
        for h in held:
            del h[:]

    for u in ids.tolist():
        c, s = grank._row(ptr, adj, u, w)
        keep = (c > u) & (s > 0)
        keep[keep] &= member[c[keep]]
        if exclude:
            keep &= ~np.isin(c, adj[ptr[u]:ptr[u + 1]])
        if len(best[0]) == k:  # nothing at or behind the k-th best known can enter: (s, u, c) with s == the k-th score comes behind it
            keep &= s > best[0][-1]
        if not keep.any():
            continue
        held[0].append(s[keep]), held[1].append(np.full(int(keep.sum()), u, dtype=np.int64)), held[2].append(c[keep])
        n_held += int(keep.sum())
        if n_held >= max(4 * k, 1 << 16):
            merge()
            n_held = 0
    merge()
    n_found = len(best[0])
    out_u, out_v, out_s = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32), np.zeros(k, dtype=np.uint64)
    out_u[:n_found], out_v[:n_found], out_s[:n_found] = best[1], best[2], best[0]
    return dict(u=out_u, v=out_v, score=out_s, n_found=n_found)


def format_pairs(index, res, ks):
    """'graph_pairs:index=<i> P@100=<p> R@100=<r> ... n_test=<t> dropped=<d> n=<m> found=<f>\\n'"""
    return "graph_pairs:index=%s %s n_test=%s dropped=%s n=%s found=%s\n" % (
        index, ppair._pr_text(res, ks), str(res["n_test"]), str(res["dropped"]), str(res["n"]), str(res["found"]))


def format_recon(index, res, ks):
    """'graph_recon:index=<i> P@100=<p> R@100=<r> ... edges=<e> n=<m> found=<f>\\n'"""
    return "graph_recon:index=%s %s edges=%s n=%s found=%s\n" % (index, ppair._pr_text(res, ks), str(res["edges"]), str(res["n"]), str(res["found"]))


class GraphPairsEval(object):
    """The ``graph_pairs`` / ``graph_recon`` lines: the node set, the positives and the scoring of ``PairPredictionEval``, the ranking
    from the two-hop pair sweep, one call at max(ks) per index and line.  ``test_filename`` may be None for the reconstruction lines
    alone."""

    def __init__(self, train_filename, test_filename, n_node, engine=None, indices=INDICES, ks=ppair.DEFAULT_KS):
        self.train_filename, self.test_filename = train_filename, test_filename
        self.n_node = int(n_node)
        self.engine = engine
        self.indices = grank.check_indices(indices)
        self.ks = ppair.check_ks(ks)
        self._adj = self._train = self._nodes = None

    def _read(self):
        if self._train is None:
            self._train = utils.read_edges_from_file(self.train_filename)
            self.train_edges = ppair.undirected(self._train)
            self._nodes = trained_nodes(self.train_filename, self.n_node)
        return self._nodes

    @property
    def nodes(self):
        return self._read()

    def adjacency(self):
        if self._adj is None:
            self._read()
            self._adj = lheur.set_adjacency(self._train, self.n_node)
        return self._adj

    def degrees(self):
        if self.engine is not None:
            return self.engine.distinct_degrees()
        return np.diff(self.adjacency()[0])

    def _top(self, index, exclude):
        k, nodes = max(self.ks), self.nodes
        w = grank.index_weights(index, self.degrees())
        if self.engine is not None:
            res = self.engine.two_hop_top_pairs(k, nodes=nodes, weights=w, exclude=exclude)
        else:
            ptr, adj = self.adjacency()
            res = host_two_hop_top_pairs(ptr, adj, k, nodes=nodes, weights=w, exclude=exclude)
        f = res["n_found"]
        return list(zip(res["u"][:f].tolist(), res["v"][:f].tolist())), f

    def eval_graph_pairs(self):
        """{index: dict(pr {k: (P, R)}, n_test, dropped, n, found)}"""
        if self.test_filename is None:
            raise ValueError("pair prediction needs test edges")
        nodes = self.nodes
        positives, dropped = ppair.held_out_positives(utils.read_edges_from_file(self.test_filename), nodes, self.train_edges)
        out = {}
        for index in self.indices:
            pairs, found = self._top(index, True)
            out[index] = dict(pr=ppair.precision_recall(pairs, positives, self.ks), n_test=len(positives), dropped=dropped, n=len(nodes), found=found)
        return out

    def eval_graph_reconstruction(self):
        """{index: dict(pr {k: (P, R)}, edges, n, found)}"""
        nodes = self.nodes
        out = {}
        for index in self.indices:
            pairs, found = self._top(index, False)
            out[index] = dict(pr=ppair.precision_recall(pairs, self.train_edges, self.ks), edges=len(self.train_edges), n=len(nodes), found=found)
        return out

    def lines(self, kind="pairs"):
        """the results lines of one kind, "pairs" or "recon", one per index"""
        if kind == "pairs":
            res = self.eval_graph_pairs()
            return [format_pairs(index, res[index], self.ks) for index in self.indices]
        if kind == "recon":
            res = self.eval_graph_reconstruction()
            return [format_recon(index, res[index], self.ks) for index in self.indices]
        raise ValueError("graph pairs: kind must be 'pairs' or 'recon', got %r" % (kind,))
