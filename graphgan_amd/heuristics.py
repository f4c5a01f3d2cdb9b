"""The neighbourhood link-prediction indices of node pairs on a training graph.

    python -m graphgan_amd.heuristics --train T.txt --pairs P.txt --out scores.tsv [--device 0 | --host]

Reads the training edges and the pairs (one ``u v`` per line, whitespace separated) and writes one line
``u<TAB>v<TAB>cn<TAB>jaccard<TAB>aa<TAB>ra<TAB>pa`` per pair, in the order of the pairs file: common neighbours, Jaccard,
Adamic-Adar, resource allocation and preferential attachment as ``evaluation/link_heuristics.py`` defines them (neighbour sets:
duplicate edges and self-loops do not count); integers as they are, the others by ``repr(float(v))``.  Nodes are numbered
0 .. the largest id of either file; a node without a training edge is isolated.  On a device the sweep is
``Engine.link_heuristics`` (gg_pair_neighbors); ``--host`` runs the same definitions in numpy, with the same output.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation import link_heuristics as lheur


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.heuristics", description=__doc__.split("\n")[0])
    ap.add_argument("--train", required=True, help="training edges: lines of 'u v'")
    ap.add_argument("--pairs", required=True, help="the pairs to score: lines of 'u v'")
    ap.add_argument("--out", required=True, help="output: lines of u<TAB>v<TAB>cn<TAB>jaccard<TAB>aa<TAB>ra<TAB>pa")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="numpy on the host, no device")
    args = ap.parse_args(argv)
    files = {}
    for name in ("train", "pairs"):
        rows = [r for r in utils.read_edges_from_file(getattr(args, name)) if r]
        if any(len(r) != 2 for r in rows):
            ap.error("--%s: every line must hold two node ids" % name)
        files[name] = np.array(rows, dtype=np.int64).reshape(-1, 2)
        if files[name].size and files[name].min() < 0:
            ap.error("--%s: negative node id" % name)
    train, pairs = files["train"], files["pairs"]
    n = int(max([-1] + [int(a.max()) for a in (train, pairs) if a.size])) + 1
    if n > 2 ** 31 - 1:
        ap.error("node ids must be below 2^31 - 1")
    if args.host or len(pairs) == 0:
        ptr, adj = lheur.set_adjacency(train, n)
        res = lheur.host_link_heuristics(ptr, adj, pairs[:, 0], pairs[:, 1])
    else:
        from .engine import Engine, edges_to_csr
        table = np.zeros((n, 4), dtype=np.float32)  # (the sweep reads no embedding; a context needs tables)
        eng = Engine(table, table, device=args.device)
        try:
            eng.set_graph_csr(*edges_to_csr(n, train))
            res = eng.link_heuristics(pairs[:, 0], pairs[:, 1])
        finally:
            eng.close()
    with open(args.out, "w") as f:
        for i, (a, b) in enumerate(pairs.tolist()):
            f.write("%d\t%d\t%d\t%s\t%s\t%s\t%d\n" % (a, b, res["cn"][i], repr(float(res["jaccard"][i])), repr(float(res["aa"][i])),
                                                    repr(float(res["ra"][i])), res["pa"][i]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
