"""Label spreading from a labels file over a training graph: a label for every unlabelled node.

    python -m graphgan_amd.propagate --train T.txt --labels L.txt --out pred.tsv [--alpha 0.9 --iters 30] [--multilabel] [--device 0 | --host]

Reads the training edges (one ``u v`` per line) and the labels (``node label``; with ``--multilabel`` ``node label [label ...]``,
``utils.read_multilabels``), spreads EVERY labelled node's labels (``evaluation/label_propagation.py``: F <- alpha S F + (1 - alpha) Y
on the neighbour sets, ``iters`` iterations) and writes one line ``node<TAB>label[ label ...]<TAB>score`` per node WITHOUT a label,
in ascending node order.  Single label: the label value of argmax F[node] (ties to the lowest class) and that entry as the score.
``--multilabel``: the k highest entries (ties to the lower class) in that order, k = the mean number of labels of a labelled node
rounded half up, and the highest entry as the score.  A node no label reaches in ``iters`` hops gets the most frequent label(s)
and the score 0.0.  Scores are written by ``repr(float(v))``.  Nodes are numbered 0 .. the largest id of either file; a node without
a training edge is isolated.  On a device the fit is ``Engine.label_spread`` (gg_label_spread); ``--host`` runs the same recursion
in float64 numpy.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation import label_propagation as lprop
from .evaluation import link_heuristics as lheur


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.propagate", description=__doc__.split("\n")[0])
    ap.add_argument("--train", required=True, help="training edges: lines of 'u v'")
    ap.add_argument("--labels", required=True, help="labels: lines of 'node label' (--multilabel: 'node label [label ...]')")
    ap.add_argument("--out", required=True, help="output: lines of node<TAB>label[ label ...]<TAB>score, one per unlabelled node")
    ap.add_argument("--alpha", type=float, default=0.9, help="share a node takes from its neighbours, in (0, 1) (default 0.9)")
    ap.add_argument("--iters", type=int, default=30, help="iterations, >= 1 (default 30)")
    ap.add_argument("--multilabel", action="store_true", help="the labels file gives a node several labels")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="float64 numpy on the host, no device")
    args = ap.parse_args(argv)
    if not 0.0 < args.alpha < 1.0:
        ap.error("--alpha must lie in (0, 1)")
    if args.iters < 1:
        ap.error("--iters must be at least 1")
    rows = [r for r in utils.read_edges_from_file(args.train) if r]
    if any(len(r) != 2 for r in rows):
        ap.error("--train: every line must hold two node ids")
    train = np.array(rows, dtype=np.int64).reshape(-1, 2)
    if train.size and train.min() < 0:
        ap.error("--train: negative node id")
    with open(args.labels) as f:
        ids = [int(line.split()[0]) for line in f if line.split()]
    if not ids:
        ap.error("--labels: no labelled node")
    if min(ids) < 0:
        ap.error("--labels: negative node id")
    n = max(int(train.max()) if train.size else -1, max(ids)) + 1
    if n > 2 ** 31 - 1:
        ap.error("node ids must be below 2^31 - 1")
    try:
        nodes, classes, values = (utils.read_multilabels if args.multilabel else utils.read_labels)(args.labels, n)
    except ValueError as e:
        ap.error("--labels: %s" % e)
    C = len(values)
    if C > lprop.MAX_CLASSES:
        ap.error("--labels: %d distinct labels, the sweep takes at most %d" % (C, lprop.MAX_CLASSES))
    Y = classes if args.multilabel else lprop.label_matrix("propagate", classes, len(nodes), C)
    rest = np.setdiff1d(np.arange(n, dtype=np.int64), nodes)
    if len(rest) == 0:
        F = np.zeros((0, C))
    elif args.host:
        ptr, adj = lheur.set_adjacency(train, n)
        F = lprop.host_label_spread(ptr, adj, nodes, Y, C, alpha=args.alpha, iters=args.iters, out_nodes=rest)["F"]
    else:
        from .engine import Engine, edges_to_csr
        table = np.zeros((n, 4), dtype=np.float32)  # (the sweep reads no embedding; a context needs tables)
        eng = Engine(table, table, device=args.device)
        try:
            eng.set_graph_csr(*edges_to_csr(n, train))
            F = eng.label_spread(nodes, Y, C, alpha=args.alpha, iters=args.iters, out_nodes=rest)["F"]
        finally:
            eng.close()
    k = max(1, int(np.floor(Y.sum(axis=1).mean() + 0.5))) if args.multilabel else 1
    pred, _ = lprop.predict(F, Y, k=np.full(len(rest), k))
    score = F.max(axis=1) if len(rest) else np.zeros(0)
    with open(args.out, "w") as f:
        for i, v in enumerate(rest.tolist()):
            row = np.asarray(F[i], dtype=np.float64)
            if not row.any():
                row = Y.sum(axis=0).astype(np.float64)  # (the fallback's order: label frequency)
            mine = sorted(np.flatnonzero(pred[i]).tolist(), key=lambda c: (-row[c], c))
            f.write("%d\t%s\t%s\n" % (v, " ".join(str(int(values[c])) for c in mine), repr(float(score[i]))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
