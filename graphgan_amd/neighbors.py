"""The nearest neighbours of the rows of an ``.emb`` file.

    python -m graphgan_amd.neighbors --emb X.emb --k 10 --out nn.tsv [--metric cosine|l2|dot] [--nodes ids.txt]
                                     [--precision fp32|bf16] [--device 0 | --host]

Writes ``k`` lines ``node<TAB>neighbour<TAB>score`` per queried node, nearest first, the node itself excluded; values by
``repr(float(v))``.  ``score`` is the cosine similarity (default), the dot product, or for ``l2`` the SQUARED Euclidean distance
(smallest first).  Ties go to the lower id.  ``--nodes`` names a file of node ids (whitespace separated) to query; without it
every row of the file is queried.  Neighbours are searched among the rows of the file.  ``k`` is in [1, min(256, rows - 1)].  On
a device the query is ``Engine.topk`` (gg_topk_metric, exclude = "self"); ``--host`` runs ``node_knn.host_neighbours`` in
float64 numpy.
"""
import argparse
import sys

import numpy as np

from .evaluation import node_knn
from .project import read_emb


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.neighbors", description=__doc__.split("\n")[0])
    ap.add_argument("--emb", required=True, help="embedding text file (header 'N d', rows 'id v0 v1 ...')")
    ap.add_argument("--out", required=True, help="output: lines of node<TAB>neighbour<TAB>score")
    ap.add_argument("--k", type=int, required=True, help="neighbours per node, 1 .. min(256, rows - 1)")
    ap.add_argument("--metric", choices=("cosine", "l2", "dot"), default="cosine", help="default cosine; l2 reports the squared distance")
    ap.add_argument("--nodes", default=None, help="file of node ids to query (default: every row of the file)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32", help="device scores: exact fp32 or bf16 inputs (default fp32)")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="float64 numpy on the host, no device")
    args = ap.parse_args(argv)
    ids, X = read_emb(args.emb)
    if not 1 <= args.k <= min(node_knn.MAX_K, len(ids) - 1):
        ap.error("--k must be in [1, %d], got %d" % (min(node_knn.MAX_K, len(ids) - 1), args.k))
    pos = np.arange(len(ids), dtype=np.int64)  # rows of X to query
    if args.nodes:
        with open(args.nodes, "r") as f:
            want = np.array([int(t) for t in f.read().split()], dtype=np.int64)
        missing = want[~np.isin(want, ids)]
        if len(missing):
            ap.error("--nodes: id %d is not a row of %s" % (int(missing[0]), args.emb))
        pos = np.searchsorted(ids, want)
    if args.host:
        col, score = node_knn.host_neighbours(X, pos, np.arange(len(ids)), args.k, metric=args.metric, exclude_self=True)
    else:
        from .engine import Engine
        X32 = X.astype(np.float32)
        eng = Engine(X32, X32, device=args.device)
        try:
            res = eng.topk(pos, args.k, precision=args.precision, exclude="self", metric=args.metric)
            col, score = res["col"], res["score"]
        finally:
            eng.close()
    with open(args.out, "w") as f:
        for p, cs, vs in zip(pos.tolist(), col.tolist(), score.tolist()):
            for c, v in zip(cs, vs):
                f.write("%d\t%d\t%s\n" % (ids[p], ids[c], repr(float(v))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
