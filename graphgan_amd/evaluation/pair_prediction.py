"""Global top-K pair prediction: which K pairs of the whole graph are the most likely (missing) edges?

ONE ranking over all unordered pairs {u, v}, u < v, of the nodes with a training edge, by s(u, v) = emd[u] . emd[v] (no bias),
score descending, ties by (u, v) ascending.  Its head gives two protocols of the embedding literature:

    pair prediction         global link-prediction precision@K: the pairs that are training edges are dropped; are the best-scored
                            non-edges the held-out edges?            "gen_pairs:P@<k>=<p> R@<k>=<r> ... n_test= dropped= n= found= precision="
    graph reconstruction    precision@K of SDNE / HOPE: nothing is dropped; are the best-scored pairs the training edges?
                                                                     "gen_recon:P@<k>=<p> R@<k>=<r> ... edges= n= found= precision="

    P@K = hits in the first min(K, found) entries / K        R@K = hits / positives  (nan without positives)

No negatives file is read and nothing is normalised per node.  With ``engine`` one ``Engine.top_pairs`` call at max(ks)
(gg_top_pairs: a floor consumer on the matrix-core tile stream) serves a line; only the K triples cross to the host.  With ``emd``
(and no engine) ``host_top_pairs`` runs the same definition in float64 numpy, in row blocks."""
import numpy as np

from .. import utils
from .embedding_spectrum import trained_nodes

DEFAULT_KS = (100, 1000, 10000)
MAX_K = 1 << 20  # the limit of gg_top_pairs
PRECISIONS = ("fp32", "bf16")


def check_ks(ks):
    """engine_pair_ks: a non-empty sequence of positive integers <= 2^20 -> tuple of int"""
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError("engine_pair_ks must be a sequence of positive integers <= 2^20, got %r" % (ks,))
    if not ks or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K for k in ks):
        raise ValueError("engine_pair_ks must be a sequence of positive integers <= 2^20, got %r" % (ks,))
    return tuple(int(k) for k in ks)


def check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError("engine_pair_precision must be 'fp32' or 'bf16', got %r" % (precision,))
    return precision


def neighbour_sets(edges, n_node):
    """undirected neighbour sets of an edge list (self-loops and duplicates are harmless)"""
    nbrs = [set() for _ in range(n_node)]
    for e in edges:
        a, b = int(e[0]), int(e[1])
        nbrs[a].add(b)
        nbrs[b].add(a)
    return nbrs


def host_top_pairs(emd, nodes, k, graph=None, block=512):
    """The k best pairs {u, v}, u < v, of ``nodes`` (None: every row; else ids, strictly ascending) under emd[u] . emd[v] in
    float64, score descending (-0 == +0), ties by (u, v) ascending; ``graph``: None, or neighbour sets -- the pairs with v in
    graph[u] are dropped.  Row blocks of ``block`` rows; between blocks only the k best so far are kept.
    -> dict(u int32 [k], v int32 [k], score float64 [k] (-1, -1, -inf behind n_found), n_found)"""
    E = np.asarray(emd, dtype=np.float64)
    ids = np.arange(E.shape[0], dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
    if len(ids) > 1 and not (np.diff(ids) > 0).all():
        raise ValueError("host_top_pairs: nodes must be strictly ascending")
    k = int(k)
    X = E[ids]
    best_s, best_u, best_v = np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64)
    for b0 in range(0, len(ids), block):
        b1 = min(len(ids), b0 + block)
        S = X[b0:b1] @ X[b0:].T + 0.0           # columns from the block's first row on: v > u lies there
        ok = np.arange(b1 - b0)[:, None] < np.arange(len(ids) - b0)[None, :]
        if graph is not None:
            for i in range(b0, b1):
                nb = graph[int(ids[i])]
                if nb:
                    cols = np.fromiter(nb, dtype=np.int64, count=len(nb))
                    pos = np.minimum(np.searchsorted(ids, cols), len(ids) - 1)
                    pos = pos[(ids[pos] == cols) & (pos >= b0)]   # the neighbours that are members, as columns of this block
                    ok[i - b0, pos - b0] = False
        r, c = np.nonzero(ok)
        s, u, v = S[r, c], ids[b0 + r], ids[b0 + c]
        if len(s) > k:      # the block's own k best before the merge (ties at the cut resolved by the full sort below)
            cut = np.partition(s, len(s) - k)[len(s) - k]
            keep = s >= cut
            s, u, v = s[keep], u[keep], v[keep]
        s, u, v = np.concatenate([best_s, s]), np.concatenate([best_u, u]), np.concatenate([best_v, v])
        o = np.lexsort((v, u, -s))[:k]
        best_s, best_u, best_v = s[o], u[o], v[o]
    n_found = len(best_s)
    out_u, out_v, out_s = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32), np.full(k, -np.inf, dtype=np.float64)
    out_u[:n_found], out_v[:n_found], out_s[:n_found] = best_u, best_v, best_s
    return dict(u=out_u, v=out_v, score=out_s, n_found=n_found)


def precision_recall(pairs, positives, ks):
    """pairs: the ranked (u, v) list, u < v; positives: a set of (u, v), u < v -> {k: (P@k, R@k)} with
    P@k = hits in the first min(k, len(pairs)) entries / k, R@k = hits / len(positives) (nan without positives)"""
    hit = np.array([(int(a), int(b)) in positives for a, b in pairs], dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(hit)])
    out = {}
    for k in ks:
        h = int(cum[min(int(k), len(hit))])
        out[int(k)] = (h / float(k), h / float(len(positives)) if len(positives) else float("nan"))
    return out


def undirected(edges):
    """the distinct undirected edges of a list without self-loops: a set of (min, max)"""
    return {(min(int(e[0]), int(e[1])), max(int(e[0]), int(e[1]))) for e in edges if int(e[0]) != int(e[1])}


def held_out_positives(test_edges, nodes, train_edges):
    """The positives of pair prediction and the number of test edges dropped: a test edge counts once, as (min, max), if it is no
    self-loop, both ends are in ``nodes`` and it is no training edge -> (set of (u, v), u < v; dropped).  The one rule of
    ``PairPredictionEval`` and ``graph_pairs.GraphPairsEval``."""
    member = set(np.asarray(nodes).tolist())
    positives, dropped = set(), 0
    for e in test_edges:
        a, b = min(int(e[0]), int(e[1])), max(int(e[0]), int(e[1]))
        if a == b or a not in member or b not in member or (a, b) in train_edges or (a, b) in positives:
            dropped += 1
        else:
            positives.add((a, b))
    return positives, dropped


class PairPredictionEval(object):
    def __init__(self, train_filename, test_filename, n_node, n_emb, engine=None, emd=None, which=0, ks=DEFAULT_KS, precision="fp32"):
        """``engine`` (+ ``which``): Engine.top_pairs on the resident table and training graph; otherwise float64 numpy on ``emd``
        ([n_node, n_emb]).  ``test_filename`` may be None for the reconstruction line alone."""
        self.ks, self.precision = check_ks(ks), check_precision(precision)
        if engine is None and emd is None:
            raise ValueError("PairPredictionEval needs an engine or an embedding matrix")
        self.n_node, self.n_emb, self.engine, self.emd, self.which = n_node, n_emb, engine, emd, which
        train = utils.read_edges_from_file(train_filename)
        self.train_edges = undirected(train)
        self.nodes = trained_nodes(train_filename, n_node)
        self._train_raw = train
        self.test_filename = test_filename

    def _top(self, exclude):
        k = max(self.ks)
        if self.engine is not None:
            res = self.engine.top_pairs(k, nodes=self.nodes.astype(np.int32), which=self.which, precision=self.precision, exclude=exclude)
        else:
            res = host_top_pairs(self.emd, self.nodes, k, graph=neighbour_sets(self._train_raw, self.n_node) if exclude else None)
        f = res["n_found"]
        return list(zip(res["u"][:f].tolist(), res["v"][:f].tolist())), f

    def eval_pair_prediction(self):
        """-> dict(pr {k: (P, R)}, n_test, dropped, n, found, precision)"""
        if self.test_filename is None:
            raise ValueError("pair prediction needs test edges")
        positives, dropped = held_out_positives(utils.read_edges_from_file(self.test_filename), self.nodes, self.train_edges)
        pairs, found = self._top(True)
        return dict(pr=precision_recall(pairs, positives, self.ks), n_test=len(positives), dropped=dropped, n=len(self.nodes), found=found,
                    precision=self.precision)

    def eval_graph_reconstruction(self):
        """-> dict(pr {k: (P, R)}, edges, n, found, precision)"""
        pairs, found = self._top(False)
        return dict(pr=precision_recall(pairs, self.train_edges, self.ks), edges=len(self.train_edges), n=len(self.nodes), found=found,
                    precision=self.precision)


def _pr_text(res, ks):
    return " ".join("P@%d=%s R@%d=%s" % (k, str(res["pr"][k][0]), k, str(res["pr"][k][1])) for k in ks)


def format_pairs(mode, res, ks=DEFAULT_KS):
    """'gen_pairs:P@100=<p> R@100=<r> ... n_test=<t> dropped=<d> n=<m> found=<f> precision=<p>\\n'"""
    return "%s_pairs:%s n_test=%s dropped=%s n=%s found=%s precision=%s\n" % (
        mode, _pr_text(res, ks), str(res["n_test"]), str(res["dropped"]), str(res["n"]), str(res["found"]), str(res["precision"]))


def format_recon(mode, res, ks=DEFAULT_KS):
    """'gen_recon:P@100=<p> R@100=<r> ... edges=<e> n=<m> found=<f> precision=<p>\\n'"""
    return "%s_recon:%s edges=%s n=%s found=%s precision=%s\n" % (
        mode, _pr_text(res, ks), str(res["edges"]), str(res["n"]), str(res["found"]), str(res["precision"]))
