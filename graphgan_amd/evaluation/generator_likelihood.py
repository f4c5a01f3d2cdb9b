"""Held-out likelihood of the generator: how probable the test edges are under the generator's graph softmax.

The generator of GraphGAN is a distribution: for a root u, G(v | u) is the law of the end node of one walk on u's BFS tree
(``GraphGAN.sample``, graph_gan.py:225-270; ``Engine.graph_softmax`` computes it exactly on the device).  Every test edge is
scored in both directions, (u -> v) and (v -> u), against the G-mode distribution of its first node as the root, with the Q3
bits the training has left (graph_gan.py:258-259):

    nll   = mean of -log G(v | u) over the pairs with G(v | u) > 0
    reach = fraction of pairs with G(v | u) > 0
    n     = number of pairs

``host_graph_softmax`` is the float64 host fallback on the reference-shaped lists ``Engine.get_trees`` returns (a father
entry of -1 marks a Q3 removal).
"""
import numpy as np

from .. import utils


def format_line(result):
    """The results line: ``gen_nll:NLL=<nll> reach=<reach> n=<n>`` (values with ``str``)."""
    return "gen_nll:NLL=%s reach=%s n=%s\n" % (str(result["nll"]), str(result["reach"]), str(result["n"]))


def host_graph_softmax(emb, bias, root, off, nbr, for_d=False):
    """float64 G(. | root) of one tree given as the reference's lists: node v's list is ``nbr[off[v]:off[v + 1]]`` =
    [father, children...] (the root's: [root, children...]; an empty list: v is not in the tree; a father of -1: removed by
    Q3).  Scores s(v, w) = emb[v] . emb[w] + bias[w].  Returns (logp float64 [n_node] with -inf where P = 0, abort mass)."""
    emb = np.asarray(emb, dtype=np.float64)
    bias = np.asarray(bias, dtype=np.float64)
    off = np.asarray(off, dtype=np.int64)
    nbr = np.asarray(nbr, dtype=np.int64)
    n = len(off) - 1
    root = int(root)
    ln = off[1:] - off[:-1]
    src = np.repeat(np.arange(n, dtype=np.int64), ln)        # the list each entry belongs to
    pos = np.arange(len(src), dtype=np.int64) - off[src]     # its position in that list (0 = the head)
    dst = nbr[: len(src)]
    child = pos >= 1
    head = (pos == 0) & (src != root) & (dst >= 0)
    if for_d:
        head &= dst != root
    cand = child | head
    s = np.full(len(src), -np.inf)
    if cand.any():
        s[cand] = np.einsum("ij,ij->i", emb[src[cand]], emb[dst[cand]]) + bias[dst[cand]]
    # log-sum-exp of every list over its candidates
    m = np.full(n, -np.inf)
    np.maximum.at(m, src[cand], s[cand])
    tot = np.zeros(n)
    np.add.at(tot, src[cand], np.exp(s[cand] - m[src[cand]]))
    with np.errstate(divide="ignore"):
        lse = m + np.log(tot)
    # log reach, top-down level by level
    logR = np.full(n, -np.inf)
    logR[root] = 0.0
    frontier = np.array([root], dtype=np.int64)
    inl = np.zeros(n, dtype=bool)
    while len(frontier):
        inl[:] = False
        inl[frontier] = True
        e = np.flatnonzero(child & inl[src])
        logR[dst[e]] = logR[src[e]] + s[e] - lse[src[e]]
        frontier = dst[e]
    logp = np.full(n, -np.inf)
    eh = np.flatnonzero(head)
    logp[src[eh]] = logR[src[eh]] + s[eh] - lse[src[eh]]
    has_cand = np.zeros(n, dtype=bool)
    has_cand[src[cand]] = True
    dead = (ln > 0) & ~has_cand & np.isfinite(logR)
    abort = float(np.exp(logR[dead]).sum())
    return logp, abort


def edge_pairs(test_filename):
    """(root, node) pairs of the test edges in file order, both directions: (a, b), (b, a), ... -> int64 [2m, 2]."""
    edges = np.asarray(utils.read_edges_from_file(test_filename), dtype=np.int64).reshape(-1, 2)
    pairs = np.empty((2 * len(edges), 2), dtype=np.int64)
    pairs[0::2] = edges
    pairs[1::2] = edges[:, ::-1]
    return pairs


def summarize(logp):
    """dict(nll, reach, n) of the pairs' log-probabilities (float64 reductions in pair order; NaN = a pair not scored)."""
    logp = np.asarray(logp, dtype=np.float64)
    logp = logp[~np.isnan(logp)]
    ok = np.isfinite(logp)
    n = int(len(logp))
    return dict(nll=float(-logp[ok].mean()) if ok.any() else float("nan"), reach=float(ok.mean()) if n else 0.0, n=n)


class GenLikelihoodEval(object):
    """``engine`` + ``slot_of_root`` (root -> resident slot): the resident trees and their Q3 bits; ``engine`` alone: whole trees
    built for batches of ``batch_roots`` test roots with the Q3 bits of the root-batched epochs' store (the engine's tree
    mode is restored afterwards).  Without an engine: ``emb``, ``bias`` and ``trees`` = (root -> slot, off, nbr, base) of
    ``Engine.get_trees`` on the host (float64)."""

    def __init__(self, test_filename, n_node, engine=None, slot_of_root=None, batch_roots=4096, emb=None, bias=None, trees=None):
        self.test_filename = test_filename
        self.n_node = n_node
        self.engine, self.slot_of_root = engine, slot_of_root
        self.batch_roots = max(1, int(batch_roots))
        self.emb, self.bias, self.trees = emb, bias, trees
        if engine is None and (emb is None or bias is None or trees is None):
            raise ValueError("GenLikelihoodEval: an engine, or emb + bias + trees for the host fallback")

    def pair_logp(self, pairs):
        """log G(node | root) of every (root, node) pair (float64; fp32 values from the device); NaN for a pair whose root has
        no resident slot (``slot_of_root`` mode)."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        out = np.full(len(pairs), np.nan)
        if len(pairs) == 0:
            return out
        order = np.argsort(pairs[:, 0], kind="stable")
        roots, starts = np.unique(pairs[order, 0], return_index=True)
        bounds = np.append(starts, len(order))
        groups = [order[bounds[i]:bounds[i + 1]] for i in range(len(roots))]
        if self.engine is None:
            slot_of, off, nbr, base = self.trees
            for u, g in zip(roots.tolist(), groups):
                r = slot_of[u]
                lp, _ = host_graph_softmax(self.emb, self.bias, u, off[r], nbr[base[r]:base[r + 1]], for_d=False)
                out[g] = lp[pairs[g, 1]]
            return out
        if self.slot_of_root is not None:
            keep = [i for i, u in enumerate(roots.tolist()) if u in self.slot_of_root]
            if keep:
                q, _ = self.engine.graph_softmax([self.slot_of_root[int(roots[i])] for i in keep], nodes=[pairs[groups[i], 1] for i in keep])
                for i, qi in zip(keep, q):
                    out[groups[i]] = qi
            return out
        mode = self.engine.tree_mode
        self.engine.set_tree_mode(0)
        try:
            for k0 in range(0, len(roots), self.batch_roots):
                batch = roots[k0:k0 + self.batch_roots]
                self.engine.build_trees(batch, device=True)
                gs = groups[k0:k0 + self.batch_roots]
                q, _ = self.engine.graph_softmax(np.arange(len(batch)), nodes=[pairs[g, 1] for g in gs], q3_store=True)
                for g, qi in zip(gs, q):
                    out[g] = qi
        finally:
            self.engine.set_tree_mode(*mode)
        return out

    def eval_gen_likelihood(self):
        return summarize(self.pair_logp(edge_pairs(self.test_filename)))
