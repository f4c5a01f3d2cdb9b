"""Label-propagation communities and modularity: the graph-only side of node clustering.  What a community detector reaches on
the TRAINING graph alone against the labels -- no embedding takes part -- and whether a partition of the nodes (the k-means
clusters of an embedding, the labels) is a partition of the graph into communities.  A ``gen_cluster:NMI=`` below the
``graph_cluster:NMI=`` line has learnt less about the classes than the adjacency lists already say.

On the neighbour SETS of the training graph (``link_heuristics.set_adjacency``: distinct neighbours other than the node itself).

Neighbour mode (gg_neighbor_mode).  With cnt(l) = |{w in N(v) : labels[w] == l}| and cmax = max cnt: a node without neighbours
keeps its label; with ``keep`` a node whose own label reaches cmax keeps it; otherwise the node takes the label with cnt == cmax
that has the smallest pair (fmix32(l ^ salt), l) -- ``fmix32`` the MurmurHash3 finaliser on uint32.  All integer, so the device
and the host agree exactly.

Label propagation (gg_label_propagation; Raghavan et al. 2007).  From L[v] = v; iteration t = 1, 2, ... draws a side for every
node, side(v) = fmix32(v ^ st) & 1 with st = fmix32((seed ^ 0x85ebca6b) + 0x9E3779B9 t), and runs two half-steps h = 0, 1: the
nodes of side h take the neighbour mode of L (salt = fmix32(seed + 0x9E3779B9 (2 (t - 1) + h + 1)), keep on) all at once, the
others keep their label.  It stops at the first iteration that moves no label, or after ``max_iters``.  Plain synchronous
updates do not converge (neighbouring nodes swap labels for ever), and neither does a fixed split; a split redrawn every
iteration does.

Modularity (gg_partition_edges).  For a partition ``assign`` (-1: outside) tot[c] counts the ordered pairs (v, w), w in N(v),
with v in class c and w inside the partition, intra[c] those with w in class c too.  With M2 = sum tot,

    Q = sum over c, ascending, of (intra[c] / M2 - (tot[c] / M2)^2)        (float64; nan where M2 == 0)

computed by ``modularity_from_counts`` for the device and the host path alike.

``GraphCommunityEval`` runs ``n_init`` restarts (seeds ``seed, seed + 1, ...``) on the WHOLE training graph, keeps the one with
the highest Q (the first on ties; Q needs no labels) and scores it over the labelled nodes with
``node_clustering.cluster_metrics``.  ``eval_cluster_modularity`` scores a partition of the labelled nodes, and the labels taken
as a partition, on the subgraph the labelled nodes induce.  With an ``engine`` the sweeps run on the device on the resident
training graph; without one the ``host_*`` functions run the same rules in numpy on the training file.  ``n_init = 4`` and
``max_iters = 100`` are provisional defaults: no labelled real dataset was at hand to choose them on.  Weighted edges, overlapping
communities and the Louvain / Leiden moves are not built.
"""
import numpy as np

from .. import utils
from . import link_heuristics as lheur

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9


def fmix32(x):
    """the MurmurHash3 finaliser: a Python int -> int, or an array -> uint32 array (arithmetic mod 2^32)"""
    if isinstance(x, (int, np.integer)):
        x = int(x) & M32
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M32
        return x ^ (x >> 16)
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def iteration_state(seed, t):
    """st of iteration t (the side of node v is fmix32(v ^ st) & 1)"""
    return fmix32(((int(seed) & M32) ^ 0x85EBCA6B) + GOLDEN * int(t))


def half_step_salt(seed, t, h):
    return fmix32((int(seed) & M32) + GOLDEN * (2 * (int(t) - 1) + int(h) + 1))


def check_labels(fn, labels, n_node):
    """-> int32 [n_node], every label in [0, 2^31); refused with the ABI's text (the FIRST offender)"""
    a = np.asarray(labels)
    if a.shape != (n_node,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: labels must be an int array [%d], got %s %r" % (fn, n_node, a.dtype, a.shape))
    bad = np.flatnonzero((a < 0) | (a > 0x7FFFFFFF))
    if len(bad):
        if a[bad[0]] < 0:
            raise ValueError("%s: labels[%d] = %d is negative" % (fn, bad[0], a[bad[0]]))
        raise ValueError("%s: labels[%d] = %d does not fit in 31 bits" % (fn, bad[0], a[bad[0]]))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_assign(fn, assign, n_node, n_label):
    """-> int32 [n_node], every entry in [-1, n_label); refused with the ABI's texts"""
    if isinstance(n_label, bool) or int(n_label) != n_label or int(n_label) < 1:
        raise ValueError("%s: n_label = %r is below 1" % (fn, n_label))
    a = np.asarray(assign)
    if a.shape != (n_node,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: assign must be an int array [%d], got %s %r" % (fn, n_node, a.dtype, a.shape))
    bad = np.flatnonzero((a < -1) | (a >= int(n_label)))
    if len(bad):
        raise ValueError("%s: assign[%d] = %d outside [-1, %d)" % (fn, bad[0], a[bad[0]], int(n_label)))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_max_iters(fn, max_iters):
    if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or int(max_iters) < 1:
        raise ValueError("%s: max_iters = %r is below 1" % (fn, max_iters))


def _check_nodes(fn, nodes, n_node):
    a = np.asarray(nodes)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("%s: nodes must be a 1-d array of integers" % fn)
    a = a.astype(np.int64)
    bad = np.flatnonzero((a < 0) | (a >= n_node))
    if len(bad):
        raise ValueError("%s: nodes[%d] = %d out of range [0, %d)" % (fn, bad[0], a[bad[0]], n_node))
    return a


def host_neighbor_mode(ptr, adj, labels, salt=0, keep=True, nodes=None):
    """``Engine.neighbor_mode`` in numpy on the set adjacency (ptr, adj): int32 [m]."""
    fn = "host_neighbor_mode"
    n = len(ptr) - 1
    lab = check_labels(fn, labels, n).astype(np.int64)
    rows = None if nodes is None else _check_nodes(fn, nodes, n)
    out = lab.copy()
    if len(adj):
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
        nl = lab[np.asarray(adj, dtype=np.int64)]
        order = np.lexsort((nl, src))
        s, l = src[order], nl[order]
        start = np.flatnonzero(np.concatenate([[True], (s[1:] != s[:-1]) | (l[1:] != l[:-1])]))
        rs_, rl = s[start], l[start]  # one run per (node, neighbour label)
        cnt = np.diff(np.concatenate([start, [len(s)]]))
        h = fmix32(rl.astype(np.uint32) ^ np.uint32(int(salt) & M32)).astype(np.int64)
        best = np.lexsort((rl, h, -cnt, rs_))  # per node: count descending, hash ascending, label ascending
        first = best[np.concatenate([[True], rs_[best][1:] != rs_[best][:-1]])]
        out[rs_[first]] = rl[first]
        if keep:
            cmax = np.zeros(n, dtype=np.int64)
            cmax[rs_[first]] = cnt[first]
            own = rl == lab[rs_]
            stay = rs_[own][cnt[own] == cmax[rs_[own]]]
            out[stay] = lab[stay]
    out = out.astype(np.int32)
    return out if rows is None else out[rows]


def host_label_propagation(ptr, adj, seed=0, max_iters=100):
    """``Engine.label_propagation`` on the host: dict(labels int32 [n], iters, converged, changed int64 [iters])."""
    check_max_iters("host_label_propagation", max_iters)
    n = len(ptr) - 1
    L = np.arange(n, dtype=np.int32)
    ids = np.arange(n, dtype=np.uint32)
    changed, converged, t = [], False, 0
    while t < int(max_iters) and not converged:
        t += 1
        side = fmix32(ids ^ np.uint32(iteration_state(seed, t))) & np.uint32(1)
        moved = 0
        for h in (0, 1):
            new = np.where(side == h, host_neighbor_mode(ptr, adj, L, salt=half_step_salt(seed, t, h), keep=True), L)
            moved += int((new != L).sum())
            L = new.astype(np.int32)
        changed.append(moved)
        converged = moved == 0
    return dict(labels=L, iters=t, converged=bool(converged), changed=np.array(changed, dtype=np.int64))


def host_partition_edges(ptr, adj, assign, n_label):
    """``Engine.partition_edges`` on the host: dict(intra int64 [n_label], tot int64 [n_label])."""
    n = len(ptr) - 1
    a = check_assign("host_partition_edges", assign, n, n_label).astype(np.int64)
    src = a[np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))]
    dst = a[np.asarray(adj, dtype=np.int64)] if len(adj) else np.zeros(0, np.int64)
    inside = (src >= 0) & (dst >= 0)
    tot = np.bincount(src[inside], minlength=int(n_label)).astype(np.int64)
    intra = np.bincount(src[inside & (src == dst)], minlength=int(n_label)).astype(np.int64)
    return dict(intra=intra, tot=tot)


def modularity_from_counts(intra, tot):
    """Q = sum over the classes in ascending order of (intra / M2 - (tot / M2)^2), M2 = sum tot, in float64; nan where M2 == 0.
    The ONE function behind every Q of the package (device counts and host counts)."""
    intra, tot = np.asarray(intra, dtype=np.int64), np.asarray(tot, dtype=np.int64)
    m2 = int(tot.sum())
    if m2 == 0:
        return float("nan")
    terms = intra.astype(np.float64) / float(m2) - (tot.astype(np.float64) / float(m2)) ** 2
    return float(np.cumsum(terms)[-1])  # (cumsum adds in ascending order)


def relabel(labels):
    """(communities int32 [n] numbered 0 .. k - 1 in ascending order of their smallest member, k)"""
    a = np.asarray(labels)
    if a.size == 0:
        return np.zeros(0, dtype=np.int32), 0
    _, first, inv = np.unique(a, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32), int(len(first))


def fit_communities(propagate, edges, seed=0, n_init=4, max_iters=100):
    """The best of ``n_init`` label propagations (seeds ``seed, seed + 1, ...`` mod 2^32): the highest modularity, the first on
    ties.  ``propagate(seed, max_iters)`` and ``edges(assign, n_label)`` are the device's or the host's.  -> dict(communities
    int32 [n] (``relabel``), k, q, intra, tot, iters, converged, seed)."""
    if isinstance(n_init, bool) or int(n_init) != n_init or int(n_init) < 1:
        raise ValueError("label propagation: n_init must be an integer >= 1, got %r" % (n_init,))
    check_max_iters("label propagation", max_iters)
    best = None
    for r in range(int(n_init)):
        s = (int(seed) + r) & M32
        res = propagate(s, int(max_iters))
        comm, k = relabel(res["labels"])
        cnt = edges(comm, max(k, 1))
        q = modularity_from_counts(cnt["intra"], cnt["tot"])
        if best is None or q > best["q"]:
            best = dict(communities=comm, k=k, q=q, intra=np.asarray(cnt["intra"]), tot=np.asarray(cnt["tot"]), iters=int(res["iters"]),
                        converged=bool(res["converged"]), seed=s)
    return best


def host_sweeps(train_edges, n_node):
    """(propagate, edges) of ``fit_communities`` in numpy on an edge list"""
    ptr, adj = lheur.set_adjacency(train_edges, n_node)
    return (lambda seed, max_iters: host_label_propagation(ptr, adj, seed=seed, max_iters=max_iters),
            lambda assign, n_label: host_partition_edges(ptr, adj, assign, n_label))


def engine_sweeps(engine):
    return (lambda seed, max_iters: engine.label_propagation(seed=seed, max_iters=max_iters),
            lambda assign, n_label: engine.partition_edges(assign, n_label))


KEYS = ("NMI", "ARI", "purity", "Q", "communities", "n", "iters", "converged", "seed")


def format_results(result):
    """The results line ``graph_cluster:NMI=<n> ARI=<a> purity=<p> Q=<q> communities=<c> n=<n> iters=<t> converged=<b> seed=<s>``
    (values with ``str``): one line, not one per mode -- the graph is the same for both tables."""
    return "graph_cluster:" + " ".join("%s=%s" % (k, str(result[k])) for k in KEYS) + "\n"


def format_modularity(mode, result):
    """One results line: ``<mode>_mod:Q=<q> label_Q=<q> k=<k> n=<n> edges=<M2 / 2>`` (values with ``str``)."""
    return "%s_mod:Q=%s label_Q=%s k=%s n=%s edges=%s\n" % (mode, str(result["Q"]), str(result["label_Q"]), str(result["k"]), str(result["n"]),
                                                          str(result["edges"]))


class GraphCommunityEval(object):
    def __init__(self, train_filename, labels_filename, n_node, engine=None, n_init=4, max_iters=100, seed=0):
        if isinstance(n_init, bool) or int(n_init) != n_init or int(n_init) < 1:
            raise ValueError("label propagation: n_init must be an integer >= 1, got %r" % (n_init,))
        check_max_iters("label propagation", max_iters)
        self.train_filename, self.labels_filename, self.n_node = train_filename, labels_filename, int(n_node)
        # ``engine``: the sweeps run on the device on its resident training graph; otherwise in numpy on the training file
        self.engine = engine
        self.n_init, self.max_iters, self.seed = int(n_init), int(max_iters), int(seed)

    def sweeps(self):
        if self.engine is not None:
            return engine_sweeps(self.engine)
        return host_sweeps(utils.read_edges_from_file(self.train_filename), self.n_node)

    def eval_graph_communities(self):
        from . import node_clustering as ncl  # (imports the engine module, which imports this one)
        nodes, classes, _ = utils.read_labels(self.labels_filename, self.n_node)
        propagate, edges = self.sweeps()
        fit = fit_communities(propagate, edges, seed=self.seed, n_init=self.n_init, max_iters=self.max_iters)
        self.last_fit = fit
        scores = ncl.cluster_metrics(classes, fit["communities"][nodes])
        return dict(NMI=scores["nmi"], ARI=scores["ari"], purity=scores["purity"], Q=fit["q"], communities=int((fit["tot"] > 0).sum()),
                    n=int(len(nodes)), iters=fit["iters"], converged=fit["converged"], seed=fit["seed"])


def eval_cluster_modularity(edges, n_node, partition):
    """Modularity of a partition of the labelled nodes on the subgraph they induce, beside that of the labels taken as the
    partition.  ``edges(assign, n_label)``: the device's or the host's ``partition_edges``; ``partition``: ``NodeClusterEval``'s
    ``last_partition`` (nodes, classes, assign, k, n_labels).  -> dict(Q, label_Q, k, n, edges = M2 / 2)."""
    nodes = np.asarray(partition["nodes"], dtype=np.int64)
    full = np.full(int(n_node), -1, dtype=np.int32)
    full[nodes] = np.asarray(partition["assign"], dtype=np.int32)
    cnt = edges(full, int(partition["k"]))
    full[nodes] = np.asarray(partition["classes"], dtype=np.int32)
    lab = edges(full, max(int(partition["n_labels"]), 1))
    return dict(Q=modularity_from_counts(cnt["intra"], cnt["tot"]), label_Q=modularity_from_counts(lab["intra"], lab["tot"]),
                k=int(partition["k"]), n=int(len(nodes)), edges=int(np.asarray(cnt["tot"]).sum()) // 2)
