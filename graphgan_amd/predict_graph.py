"""The most likely missing edges of a graph from its edge list alone: the best pairs by a neighbourhood index.

    python -m graphgan_amd.predict_graph --train T.txt --k 1000 --out pred.tsv [--index cn|aa|ra] [--include-known] [--device 0 | --host]

Reads the training edges (one ``u v`` per line) and writes the ``k`` best pairs of ONE ranking over all unordered pairs {u, v},
u < v, of the nodes with an edge, as lines ``u<TAB>v<TAB>score``, best first: ranked by ``--index`` (``cn`` common neighbours,
``aa`` Adamic-Adar, ``ra`` resource allocation; ``evaluation/graph_pairs.py``), score descending, ties to the lower (u, v).  Only
pairs with a positive score are written, so there may be fewer than ``k`` lines.  The training edges themselves are dropped from
the ranking unless ``--include-known`` is given (then the head of the list is the graph-reconstruction ranking).  ``score`` is
the integer for ``cn`` and ``wsum / 2^40`` for ``aa`` / ``ra`` (the fixed-point sum of ``link_heuristics.node_weights``).  ``k`` is
in [1, 2^20]; nodes are numbered 0 .. the largest id of the file.  On a device the query is ``Engine.two_hop_top_pairs``
(gg_two_hop_top_pairs); ``--host`` runs the same integer rules in numpy and writes the same file.  No ``.emb`` file is read: the
embedding side of the question is ``graphgan_amd.predict``.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation import graph_pairs as gpairs
from .evaluation import graph_ranking as grank
from .evaluation import link_heuristics as lheur


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.predict_graph", description=__doc__.split("\n")[0])
    ap.add_argument("--train", required=True, help="training edges: lines of 'u v'")
    ap.add_argument("--out", required=True, help="output: lines of u<TAB>v<TAB>score")
    ap.add_argument("--k", type=int, required=True, help="pairs to report, 1 .. 2^20")
    ap.add_argument("--index", default="cn", choices=grank.INDICES, help="the ranking index (default cn)")
    ap.add_argument("--include-known", action="store_true", help="keep the training edges in the ranking")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="numpy on the host, no device")
    args = ap.parse_args(argv)
    if not 1 <= args.k <= gpairs.MAX_K:
        ap.error("--k must be in [1, %d], got %d" % (gpairs.MAX_K, args.k))
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
    w = grank.index_weights(args.index, np.diff(ptr))
    nodes = np.unique(train)
    exclude = not args.include_known
    if args.host:
        res = gpairs.host_two_hop_top_pairs(ptr, adj, args.k, nodes=nodes, weights=w, exclude=exclude)
    else:
        from .engine import Engine, edges_to_csr
        table = np.zeros((n, 4), dtype=np.float32)  # (the sweep reads no embedding; a context needs tables)
        eng = Engine(table, table, device=args.device)
        try:
            eng.set_graph_csr(*edges_to_csr(n, train))
            res = eng.two_hop_top_pairs(args.k, nodes=nodes, weights=w, exclude=exclude)
        finally:
            eng.close()
    f_ = res["n_found"]
    with open(args.out, "w") as f:
        for a, b, s in zip(res["u"][:f_].tolist(), res["v"][:f_].tolist(), res["score"][:f_].tolist()):
            f.write("%d\t%d\t%s\n" % (a, b, str(s) if args.index == "cn" else repr(s / lheur.SCALE)))
    print("pairs=%d index=%s k=%d" % (f_, args.index, args.k))
    return 0


if __name__ == "__main__":
    sys.exit(main())
