"""The most likely missing edges of a graph under the rows of an ``.emb`` file.

    python -m graphgan_amd.predict --emb X.emb --train T.txt --k 1000 --out pred.tsv [--precision fp32|bf16] [--include-known]
                                   [--all-nodes] [--device 0 | --host]

Writes the ``k`` best-scored pairs of ONE ranking over all unordered pairs {u, v}, u < v, as lines ``u<TAB>v<TAB>score``, best
first; ``score`` is the dot product of the two rows by ``repr(float(v))``; ties go to the lower (u, v).  The pairs are those of
the nodes with an edge in ``--train`` (``--all-nodes``: of every row of the file); the training edges themselves are dropped
from the ranking unless ``--include-known`` is given (then the head of the list is the graph-reconstruction ranking).  ``k`` is
in [1, 2^20]; fewer lines are written when there are fewer pairs.  On a device the query is ``Engine.top_pairs`` (gg_top_pairs);
``--host`` runs ``pair_prediction.host_top_pairs`` in float64 numpy.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation import pair_prediction
from .project import read_emb


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.predict", description=__doc__.split("\n")[0])
    ap.add_argument("--emb", required=True, help="embedding text file (header 'N d', rows 'id v0 v1 ...')")
    ap.add_argument("--train", required=True, help="training edges, lines of 'u v'")
    ap.add_argument("--out", required=True, help="output: lines of u<TAB>v<TAB>score")
    ap.add_argument("--k", type=int, required=True, help="pairs to report, 1 .. 2^20")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32", help="device scores: exact fp32 or bf16 inputs (default fp32)")
    ap.add_argument("--include-known", action="store_true", help="keep the training edges in the ranking")
    ap.add_argument("--all-nodes", action="store_true", help="pairs of every row of the file, not only of the nodes with a training edge")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="float64 numpy on the host, no device")
    args = ap.parse_args(argv)
    if not 1 <= args.k <= pair_prediction.MAX_K:
        ap.error("--k must be in [1, %d], got %d" % (pair_prediction.MAX_K, args.k))
    ids, X = read_emb(args.emb)
    edges = np.asarray(utils.read_edges_from_file(args.train), dtype=np.int64).reshape(-1, 2)
    missing = edges[~np.isin(edges, ids)]
    if len(missing):
        ap.error("--train: node %d is not a row of %s" % (int(missing[0]), args.emb))
    pos_edges = np.searchsorted(ids, edges)  # the edges between ROWS of X
    nodes = None if args.all_nodes else np.unique(pos_edges)
    exclude = not args.include_known
    if args.host:
        graph = pair_prediction.neighbour_sets(pos_edges, len(ids)) if exclude else None
        res = pair_prediction.host_top_pairs(X, nodes, args.k, graph=graph)
    else:
        from .engine import Engine, edges_to_csr
        X32 = X.astype(np.float32)
        eng = Engine(X32, X32, device=args.device)
        try:
            if exclude:
                eng.set_graph_csr(*edges_to_csr(len(ids), pos_edges.astype(np.int32)))
            res = eng.top_pairs(args.k, nodes=None if nodes is None else nodes.astype(np.int32), precision=args.precision, exclude=exclude)
        finally:
            eng.close()
    f_ = res["n_found"]
    with open(args.out, "w") as f:
        for a, b, v in zip(res["u"][:f_].tolist(), res["v"][:f_].tolist(), res["score"][:f_].tolist()):
            f.write("%d\t%d\t%s\n" % (ids[a], ids[b], repr(float(v))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
