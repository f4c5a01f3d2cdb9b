"""Label-propagation communities of a training graph: a community for every node.

    python -m graphgan_amd.communities --train T.txt --out comm.tsv [--seed 0 --n-init 4 --max-iters 100] [--device 0 | --host]

Reads the training edges (one ``u v`` per line), runs ``--n-init`` label propagations (``evaluation/graph_communities.py``: seeds
``--seed``, ``--seed`` + 1, ...; at most ``--max-iters`` iterations each) on the neighbour sets, keeps the one with the highest
modularity (the first on ties) and writes one line ``node<TAB>community`` per node in ascending node order.  Nodes are numbered
0 .. the largest id of the file; communities are numbered 0 .. k - 1 in ascending order of their smallest member, so a node
without a training edge is a community of its own.  On a device the sweeps are ``Engine.label_propagation`` /
``Engine.partition_edges`` (gg_label_propagation, gg_partition_edges); ``--host`` runs the same integer rules in numpy and
writes the same file.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation import graph_communities as gcomm


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.communities", description=__doc__.split("\n")[0])
    ap.add_argument("--train", required=True, help="training edges: lines of 'u v'")
    ap.add_argument("--out", required=True, help="output: lines of node<TAB>community, one per node")
    ap.add_argument("--seed", type=int, default=0, help="seed of the first restart (default 0)")
    ap.add_argument("--n-init", type=int, default=4, help="restarts, >= 1; the highest modularity is kept (default 4)")
    ap.add_argument("--max-iters", type=int, default=100, help="iterations of a restart at most, >= 1 (default 100)")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="numpy on the host, no device")
    args = ap.parse_args(argv)
    if args.n_init < 1:
        ap.error("--n-init must be at least 1")
    if args.max_iters < 1:
        ap.error("--max-iters must be at least 1")
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
    kw = dict(seed=args.seed, n_init=args.n_init, max_iters=args.max_iters)
    if args.host:
        fit = gcomm.fit_communities(*gcomm.host_sweeps(train, n), **kw)
    else:
        from .engine import Engine, edges_to_csr
        table = np.zeros((n, 4), dtype=np.float32)  # (the sweeps read no embedding; a context needs tables)
        eng = Engine(table, table, device=args.device)
        try:
            eng.set_graph_csr(*edges_to_csr(n, train))
            fit = gcomm.fit_communities(*gcomm.engine_sweeps(eng), **kw)
        finally:
            eng.close()
    with open(args.out, "w") as f:
        f.writelines("%d\t%d\n" % (v, c) for v, c in enumerate(fit["communities"].tolist()))
    print("communities=%d Q=%s iters=%d converged=%s seed=%d" % (fit["k"], str(fit["q"]), fit["iters"], fit["converged"], fit["seed"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
