"""Project the rows of an ``.emb`` file on their first principal components.

    python -m graphgan_amd.project --emb X.emb --out coords.tsv [--dim 2] [--train T.txt] [--device 0 | --host]

Writes one line ``id<TAB>c1<TAB>...<TAB>c_dim`` per row of the file, in id order, values by ``repr(float(v))``.  With ``--train``
the PCA is FITTED on the nodes with at least one training edge only (degree-0 rows are the untrained fill); all rows are
projected.  ``dim`` is in [1, min(d, 128)].  On a device the fit is ``Engine.pca`` (two gg_gram sweeps) and the projection
``Engine.pca_transform``; ``--host`` runs ``host_pca`` and a float64 projection in numpy.
"""
import argparse
import sys

import numpy as np

from .evaluation import embedding_spectrum as espec


def read_emb(path):
    """``.emb`` text (header ``N<TAB>d``, rows ``id<TAB>v0<TAB>...``) -> (ids int64 ascending, X float64 [len(ids), d])"""
    with open(path, "r") as f:
        head = f.readline().split()
        if len(head) != 2:
            raise ValueError("%s: expected a header 'N d', got %r" % (path, " ".join(head)))
        d = int(head[1])
        rows = {}
        for no, line in enumerate(f, 2):
            tok = line.split()
            if not tok:
                continue
            if len(tok) != d + 1:
                raise ValueError("%s:%d: expected an id and %d values, got %d tokens" % (path, no, d, len(tok)))
            rows[int(tok[0])] = [float(x) for x in tok[1:]]
    if not rows:
        raise ValueError("%s holds no rows" % path)
    ids = np.array(sorted(rows), dtype=np.int64)
    return ids, np.array([rows[int(i)] for i in ids], dtype=np.float64).reshape(len(ids), d)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.project", description=__doc__.split("\n")[0])
    ap.add_argument("--emb", required=True, help="embedding text file (header 'N d', rows 'id v0 v1 ...')")
    ap.add_argument("--out", required=True, help="output: lines of id<TAB>c1<TAB>...<TAB>c_dim")
    ap.add_argument("--dim", type=int, default=2, help="components to project on, 1 .. min(d, 128) (default 2)")
    ap.add_argument("--train", default=None, help="training edges: fit on the nodes with at least one training edge only")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="float64 numpy on the host, no device")
    args = ap.parse_args(argv)
    ids, X = read_emb(args.emb)
    d = X.shape[1]
    if not 1 <= args.dim <= min(d, 128):
        ap.error("--dim must be in [1, %d], got %d" % (min(d, 128), args.dim))
    pos = np.arange(len(ids), dtype=np.int64)  # rows of X to fit on
    if args.train:
        trained = espec.trained_nodes(args.train)
        pos = np.flatnonzero(np.isin(ids, trained))
    if len(pos) < 2:
        ap.error("the fit needs at least two rows, got %d" % len(pos))
    if args.host:
        fit = espec.host_pca(X, pos, n_components=args.dim)
        coords = (X - fit["mean"].astype(np.float64)) @ fit["components"].astype(np.float64).T
    else:
        from .engine import Engine
        X32 = X.astype(np.float32)
        eng = Engine(X32, X32, device=args.device)
        try:
            fit = eng.pca(pos, n_components=args.dim)
            coords = eng.pca_transform(np.arange(len(ids)), fit["mean"], fit["components"])
        finally:
            eng.close()
    with open(args.out, "w") as f:
        for i, row in zip(ids.tolist(), coords.tolist()):
            f.write("%d\t%s\n" % (i, "\t".join(repr(float(v)) for v in row)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
