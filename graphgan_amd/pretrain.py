"""Skip-gram pre-training of the initial embeddings from uniform or node2vec (p, q) biased random walks, on the device.

The reference starts from ``pre_train/*.emb`` files of an external DeepWalk / node2vec run (config.py:33-34); this module
produces such a table from the edge list alone.  ``Engine.prepare_pretrain`` writes the (center, neighbor, label) rows of
the walks' window pairs and their negative samples into the resident discriminator rows, and ``Engine.d_pass`` -- sigmoid
cross-entropy on one table -- trains on them: one-table skip-gram with negative sampling.  All sampling and arithmetic run
in ``libgraphgan_hip.so``.

    python -m graphgan_amd.pretrain --train <edge list> [--test <edge list>] --out <file.emb> [--n-emb 50] [--p 1 --q 1] ...
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import _lib, config as _default_config, engine as _engine

STREAM_BASE = 0x50000000  # Philox stream of epoch e is STREAM_BASE + e (the trainer's prepare calls count up from 0)


def _cfg(cfg, name):
    return getattr(cfg, name, getattr(_default_config, name))


def pairs_of_path(length, window):
    """Window pairs of a path of ``length`` nodes: sum_i min(i, window) + min(length - 1 - i, window)."""
    i = np.arange(int(length))
    return int((np.minimum(i, window) + np.minimum(length - 1 - i, window)).sum())


def rows_bound(walks_per_start, walk_len, window, n_neg):
    """Upper bound of the rows one start node gives (every walk reaches its full length)."""
    return int(walks_per_start) * (1 + int(n_neg)) * pairs_of_path(walk_len, window)


def noise_weights(rowptr):
    """uint32 noise weights round(16 * max(deg, 1) ^ 0.75) -- word2vec's unigram^0.75 on the degrees."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    return np.round(16.0 * np.maximum(deg, 1).astype(np.float64) ** 0.75).astype(np.uint32)


BIAS_SCALE = 4096  # weight of the largest of (1/p, 1, 1/q)


def walk_bias(p, q):
    """Integer walk weights (w_ret, w_com, w_out) of node2vec's return parameter ``p`` and in-out parameter ``q``, each in
    [1/16, 16]: max(1, round(4096 * v / max(v))) for v = (1/p, 1, 1/q).  p = q = 1 gives equal weights, the uniform walk."""
    p, q = float(p), float(q)
    if not (1.0 / 16 <= p <= 16.0 and 1.0 / 16 <= q <= 16.0):
        raise ValueError("walk_bias: p and q must lie in [1/16, 16], got p = %r, q = %r" % (p, q))
    v = (1.0 / p, 1.0, 1.0 / q)
    return tuple(max(1, int(round(BIAS_SCALE * x / max(v)))) for x in v)


def init_table(n_node, n_emb, seed):
    """word2vec's initialisation (U(-0.5, 0.5) / d) from RandomState(seed)."""
    return ((np.random.RandomState(seed).rand(n_node, n_emb) - 0.5) / n_emb).astype(np.float32)


def start_batches(n_node, per_start_bound, rows_per_call):
    """Consecutive node-id ranges whose row bound stays under ``rows_per_call`` (at least one node each)."""
    step = max(1, int(rows_per_call) // max(1, int(per_start_bound)))
    return [(a, min(a + step, n_node)) for a in range(0, n_node, step)]


def pretrain(cfg, n_node, rowptr, col):
    """float32 [n_node, cfg.n_emb]: the discriminator's table after ``engine_pretrain_epochs`` skip-gram epochs."""
    d = int(_cfg(cfg, "n_emb"))
    seed = int(_cfg(cfg, "engine_seed"))
    walks, length = int(_cfg(cfg, "engine_pretrain_walks")), int(_cfg(cfg, "engine_pretrain_len"))
    window, n_neg = int(_cfg(cfg, "engine_pretrain_window")), int(_cfg(cfg, "engine_pretrain_neg"))
    batch = int(_cfg(cfg, "engine_pretrain_batch"))
    bias = walk_bias(_cfg(cfg, "engine_pretrain_p"), _cfg(cfg, "engine_pretrain_q"))
    init = init_table(n_node, d, seed)
    eng = _engine.Engine(init, init, lr_dis=float(_cfg(cfg, "engine_pretrain_lr")), lambda_dis=float(_cfg(cfg, "lambda_dis")),
                         optimizer=_lib.GG_OPT_ADAM_LAZY, device=int(_cfg(cfg, "engine_device")))
    try:
        eng.set_graph_csr(rowptr, col)
        eng.pretrain_set_walk_bias(*bias)
        eng.pretrain_set_noise(noise_weights(rowptr))
        rng = np.random.RandomState(seed)
        batches = start_batches(n_node, rows_bound(walks, length, window, n_neg), int(_cfg(cfg, "engine_pretrain_rows_per_call")))
        for epoch in range(int(_cfg(cfg, "engine_pretrain_epochs"))):
            for a, b in batches:
                rows = eng.prepare_pretrain(np.arange(a, b, dtype=np.int32), walks, length, window, n_neg, seed, STREAM_BASE + epoch)
                if rows == 0:
                    continue
                starts = np.arange(0, rows, batch, dtype=np.int64)
                rng.shuffle(starts)
                eng.d_pass(starts, batch)
        return eng.get_embeddings(1)  # the bias is dropped: the .emb format has none and GraphGAN starts biases at zero
    finally:
        eng.close()


def ensure_pretrained(cfg, n_node, rowptr, col):
    """The trainer's hook: with ``engine_pretrain`` on, produce the missing ``pretrain_emb_filename_*`` files (one run, the
    same table for both) in the reference's ``.emb`` text; existing files are left alone."""
    if not bool(_cfg(cfg, "engine_pretrain")):
        return None
    missing = [f for f in dict.fromkeys((cfg.pretrain_emb_filename_d, cfg.pretrain_emb_filename_g)) if not os.path.exists(f)]
    if not missing:
        return None
    emb = pretrain(cfg, n_node, rowptr, col)
    for f in missing:
        os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
        _engine.host_write_embeddings(f, emb)
    return emb


def main(argv=None):
    ap = argparse.ArgumentParser(description="skip-gram pre-training from uniform or node2vec (p, q) random walks -> .emb")
    ap.add_argument("--train", required=True)
    ap.add_argument("--test", default="")
    ap.add_argument("--out", required=True)
    ap.add_argument("--n-emb", type=int, default=_default_config.n_emb)
    ap.add_argument("--seed", type=int, default=_default_config.engine_seed)
    ap.add_argument("--device", type=int, default=_default_config.engine_device)
    for k in ("walks", "len", "window", "neg", "epochs", "batch", "rows_per_call"):
        ap.add_argument("--" + k.replace("_", "-"), type=int, default=getattr(_default_config, "engine_pretrain_" + k))
    ap.add_argument("--lr", type=float, default=_default_config.engine_pretrain_lr)
    ap.add_argument("--p", type=float, default=_default_config.engine_pretrain_p, help="node2vec return parameter, in [1/16, 16]")
    ap.add_argument("--q", type=float, default=_default_config.engine_pretrain_q, help="node2vec in-out parameter, in [1/16, 16]")
    a = ap.parse_args(argv)
    cfg = argparse.Namespace(n_emb=a.n_emb, engine_seed=a.seed, engine_device=a.device, lambda_dis=_default_config.lambda_dis,
                             engine_pretrain_lr=a.lr, engine_pretrain_p=a.p, engine_pretrain_q=a.q, **{"engine_pretrain_" + k: getattr(a, k) for k in
                                                         ("walks", "len", "window", "neg", "epochs", "batch", "rows_per_call")})
    n_node, rowptr, col = _engine.read_edges_csr(a.train, a.test)
    emb = pretrain(cfg, n_node, rowptr, col)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    _engine.host_write_embeddings(a.out, emb)
    print("wrote %s: %d x %d" % (a.out, emb.shape[0], emb.shape[1]))


if __name__ == "__main__":
    main()
