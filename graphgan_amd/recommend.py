"""Friends-of-friends recommendation from a training graph: for every listed node its best candidates by a neighbourhood index.

    python -m graphgan_amd.recommend --train T.txt --out rec.tsv [--k 10] [--index aa] [--nodes ids.txt] [--device 0 | --host]
                                     [--alpha 0.15] [--eps 1e-4] [--max-rounds 200]

Reads the training edges (one ``u v`` per line) and writes, for every node of ``--nodes`` (one id per line; default: every node
with an edge, ascending), up to ``--k`` lines ``node<TAB>candidate<TAB>score``, best first: the nodes two hops away that are
neither the node itself nor one of its training neighbours, ranked by ``--index`` (``cn`` common neighbours, ``aa`` Adamic-Adar,
``ra`` resource allocation; ``evaluation/graph_ranking.py``), score descending, candidate ascending.  A node with fewer than
``--k`` candidates of positive score gets fewer lines.  ``score`` is the integer for ``cn`` and ``wsum / 2^40`` for ``aa`` / ``ra``
(the fixed-point sum of ``link_heuristics.node_weights``).  Nodes are numbered 0 .. the largest id of the file.  On a device the
lists are ``Engine.two_hop_topk`` (gg_two_hop_topk); ``--host`` runs the same integer rules in numpy and writes the same file.

``--index ppr`` ranks by rooted PageRank instead (``evaluation/graph_ppr.py``: the push sweep, ``Engine.ppr_topk`` / gg_ppr_topk, or
its numpy rounds under ``--host``), which reaches past two hops: restart probability ``--alpha``, push threshold ``--eps`` per unit of
degree, at most ``--max-rounds`` rounds per node; ``score`` is ``p / 2^40``, the share of the walk's mass that rests on the candidate.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation import graph_ppr as gppr
from .evaluation import graph_ranking as grank
from .evaluation import link_heuristics as lheur


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.recommend", description=__doc__.split("\n")[0])
    ap.add_argument("--train", required=True, help="training edges: lines of 'u v'")
    ap.add_argument("--out", required=True, help="output: lines of node<TAB>candidate<TAB>score")
    ap.add_argument("--k", type=int, default=10, help="candidates per node at most, in [1, %d] (default 10)" % grank.MAX_K)
    ap.add_argument("--index", default="aa", choices=grank.INDICES + ("ppr",), help="the ranking index (default aa)")
    ap.add_argument("--alpha", type=float, default=gppr.DEFAULT_ALPHA, help="ppr: restart probability (default %s)" % gppr.DEFAULT_ALPHA)
    ap.add_argument("--eps", type=float, default=gppr.DEFAULT_EPS, help="ppr: push threshold per unit of degree (default %s)" % gppr.DEFAULT_EPS)
    ap.add_argument("--max-rounds", type=int, default=gppr.DEFAULT_MAX_ROUNDS, help="ppr: rounds per node at most (default %d)" % gppr.DEFAULT_MAX_ROUNDS)
    ap.add_argument("--nodes", default=None, help="query nodes, one id per line (default: every node with an edge)")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="numpy on the host, no device")
    args = ap.parse_args(argv)
    if not 1 <= args.k <= grank.MAX_K:
        ap.error("--k must lie in [1, %d]" % grank.MAX_K)
    ppr = args.index == "ppr"
    if ppr:
        try:
            gppr.quantise(args.alpha, args.eps)
            gppr.check_max_rounds("--max-rounds", args.max_rounds)
        except ValueError as e:
            ap.error(str(e))
    rows = [r for r in utils.read_edges_from_file(args.train) if r]
    if any(len(r) != 2 for r in rows):
        ap.error("--train: every line must hold two node ids")
    train = np.array(rows, dtype=np.int64).reshape(-1, 2)
    if train.size == 0:
        ap.error("--train: no edge")
    if train.min() < 0:
        ap.error("--train: negative node id")
    n = int(train.max()) + 1
    if n > 2 ** 31 - 1:
        ap.error("node ids must be below 2^31 - 1")
    ptr, adj = lheur.set_adjacency(train, n)
    deg = np.diff(ptr)
    if args.nodes is None:
        nodes = np.flatnonzero(deg > 0)
    else:
        with open(args.nodes) as f:
            nodes = np.array([int(x) for x in f.read().split()], dtype=np.int64)
        if len(nodes) and (nodes.min() < 0 or nodes.max() >= n):
            ap.error("--nodes: node id outside [0, %d)" % n)
    w = None if ppr else grank.index_weights(args.index, deg)
    pkw = dict(alpha=args.alpha, eps=args.eps, max_rounds=args.max_rounds)
    if args.host:
        res = gppr.host_ppr_topk(ptr, adj, nodes, args.k, exclude=True, **pkw) if ppr else grank.host_two_hop_topk(ptr, adj, nodes, args.k, w, True)
    else:
        from .engine import Engine, edges_to_csr
        table = np.zeros((n, 4), dtype=np.float32)  # (the sweep reads no embedding; a context needs tables)
        eng = Engine(table, table, device=args.device)
        try:
            eng.set_graph_csr(*edges_to_csr(n, train))
            res = eng.ppr_topk(nodes, k=args.k, exclude=True, **pkw) if ppr else eng.two_hop_topk(nodes, k=args.k, weights=w, exclude=True)
        finally:
            eng.close()
    with open(args.out, "w") as f:
        for u, cols, scores in zip(nodes.tolist(), res["col"].tolist(), res["score"].tolist()):
            for c, s in zip(cols, scores):
                if c >= 0:
                    f.write("%d\t%d\t%s\n" % (u, c, str(s) if args.index == "cn" else repr(s / lheur.SCALE)))
    print("nodes=%d lines=%d index=%s k=%d" % (len(nodes), int((res["col"] >= 0).sum()), args.index, args.k))
    return 0


if __name__ == "__main__":
    sys.exit(main())
