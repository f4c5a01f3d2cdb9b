"""Train / test split of an edge list for the link-prediction evaluators: the three files every evaluator reads.

    python -m graphgan_amd.split --edges E.txt --out-prefix P [--ratio 0.1 --seed 0 --protect forest|none] [--device 0 | --host]

Reads an edge list (one ``u v`` per line), holds out a share of its edges as test edges WITHOUT cutting the training graph apart,
draws as many non-edges as negatives and writes ``P_train.txt``, ``P_test.txt`` and ``P_test_neg.txt`` (``u<TAB>v`` lines, the
format of the CA-GrQc files: ``utils.read_edges`` and ``LinkPredictEval`` read them).  The customary protocol of node2vec and
GraphGAN.  Nodes are numbered 0 .. the largest id of the file.

The rules -- all integer, so the device and the host path write the same bytes:
  E           the undirected edges {(a, b) : a < b} of the list without duplicates and self-loops, ordered by (a, b), j in [0, m).
  forest      the minimum spanning forest of E under the keys (priority[j] << 32) | j, priority[j] = fmix32(j ^ fmix32(seed ^
              0x53504C54)) (``default_priorities``).  Keys are distinct, so the forest is unique.  With an engine:
              ``Engine.spanning_forest(seed)`` (gg_spanning_forest, Boruvka rounds on the device); without:
              ``host_spanning_forest``, the same rounds in numpy.  Removing edges outside a spanning forest keeps every component
              whole, and no node loses its last edge.
  n_test      floor(ratio * m + 0.5).
  candidates  the j with forest[j] == 0, ascending; with protect = "none" every j.
  test        with rs = RandomState([seed, 0x5350]): the edges at the sorted first n_test entries of
              candidates[rs.permutation(len(candidates))].  Train: all other edges, in j order.
  negatives   by rejection from the same rs behind the permutation, in blocks of NEG_BLOCK = 65 536 pairs: first NEG_BLOCK
              positions for the one end, then NEG_BLOCK for the other (``rs.randint(0, k, NEG_BLOCK)`` each), uniform over the
              ascending array of the k nodes with at least one edge.  A self pair, an edge of the input and a repeat of an earlier
              draw are dropped; the first n_test survivors are kept as (min, max) in draw order.
"""
import argparse
import sys

import numpy as np

from . import utils
from .evaluation.graph_communities import fmix32
from .evaluation.link_prediction_lr import _in_sorted, edge_keys

SEED_SALT = 0x53504C54   # == SF_SEED_SALT of csrc/spanning_forest.hip
NEG_BLOCK = 65536        # pairs per block of the negatives' rejection sampling: part of the rule, the draws depend on it
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _ceil_log2(x):
    return max(int(x) - 1, 0).bit_length()


def undirected_edge_list(edges, n_node):
    """E of the module's docstring from an edge list with duplicates, both directions and self-loops: int32 [m, 2], the
    ``Engine.undirected_edges()`` of the same graph."""
    n_node = int(n_node)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    keys = np.unique(edge_keys(e[e[:, 0] != e[:, 1]], n_node))
    if len(keys) > 2 ** 31 - 1:
        raise ValueError("split: the graph has %d undirected edges, more than 2^31 - 1" % len(keys))
    return np.stack([keys // n_node, keys % n_node], axis=1).astype(np.int32)


def default_priorities(m, seed):
    """prio[j] = fmix32(j ^ fmix32(seed ^ 0x53504C54)): uint32 [m] (the priorities of gg_spanning_forest with prio = NULL)"""
    return fmix32(np.arange(int(m), dtype=np.uint32) ^ np.uint32(fmix32((int(seed) & 0xFFFFFFFF) ^ SEED_SALT)))


def host_spanning_forest(E, n_node, seed=0, priority=None):
    """``Engine.spanning_forest`` on the host: the same Boruvka rounds in numpy, the same integers.  ``E``: the undirected edge
    list int [m, 2] (``undirected_edge_list``).  Returns dict(forest uint8 [m], component int32 [n_node], m, n_forest,
    n_components, rounds, sweep_live, sweep_hooks)."""
    n = int(n_node)
    E = np.asarray(E, dtype=np.int64).reshape(-1, 2)
    m = len(E)
    if priority is None:
        prio = default_priorities(m, seed)
    else:
        prio = np.asarray(priority)
        if prio.shape != (m,) or prio.dtype.kind not in "iu" or (m and (int(prio.min()) < 0 or int(prio.max()) > 0xFFFFFFFF)):
            raise ValueError("host_spanning_forest: priority must be a uint32 array [%d]" % m)
    key = (prio.astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)
    a, b = E[:, 0], E[:, 1]
    ids = np.arange(n, dtype=np.int64)
    comp = ids.copy()
    forest = np.zeros(m, dtype=np.uint8)
    rounds, n_forest, live_n, hook_n = 0, 0, [], []
    max_rounds = _ceil_log2(max(n, 2)) + 1
    while m > 0:
        if rounds > max_rounds:
            raise RuntimeError("host_spanning_forest: internal error: more than %d rounds on %d nodes" % (max_rounds, n))
        cu, cv = comp[a], comp[b]
        live = np.flatnonzero(cu != cv)
        live_n.append(len(live))
        if len(live) == 0:
            hook_n.append(0)
            break
        cu, cv, k = cu[live], cv[live], key[live]
        best = np.full(n, _NONE, dtype=np.uint64)
        np.minimum.at(best, cu, k)
        np.minimum.at(best, cv, k)
        wu, wv = best[cu] == k, best[cv] == k
        parent = comp.copy()
        both, only_u, only_v = wu & wv, wu & ~wv, wv & ~wu
        parent[np.maximum(cu[both], cv[both])] = np.minimum(cu[both], cv[both])  # two components that chose each other: joined once
        parent[cu[only_u]] = cv[only_u]
        parent[cv[only_v]] = cu[only_v]
        win = wu | wv
        forest[live[win]] = 1
        hooks = int(win.sum())
        hook_n.append(hooks)
        for _ in range(_ceil_log2(max(n - n_forest, 2)) + 1):  # a round may hook a chain as long as the graph
            parent = parent[parent]
        comp = parent[comp]
        rounds += 1
        n_forest += hooks
    minid = ids.copy()
    np.minimum.at(minid, comp, ids)
    return dict(forest=forest, component=minid[comp].astype(np.int32), m=m, n_forest=n_forest, n_components=n - n_forest, rounds=rounds,
                sweep_live=np.array(live_n, dtype=np.int64), sweep_hooks=np.array(hook_n, dtype=np.int64))


def draw_negatives(rs, E, n_node, n_neg):
    """``n_neg`` distinct non-edges by the rejection rule of the module's docstring, from the state ``rs`` is in: int32 [n_neg, 2],
    (min, max) rows in draw order.  Raises before any draw if fewer non-edges exist among the nodes with an edge."""
    n_node = int(n_node)
    E = np.asarray(E, dtype=np.int64).reshape(-1, 2)
    keys = E[:, 0] * np.int64(n_node) + E[:, 1]  # ascending: E is ordered by (a, b)
    nodes = np.unique(E)
    k = len(nodes)
    free = k * (k - 1) // 2 - len(E)
    if free < n_neg:
        raise ValueError("split: %d negatives asked for, only %d non-edges exist among the %d nodes with an edge" % (n_neg, free, k))
    kept = np.zeros(0, dtype=np.int64)
    while len(kept) < n_neg:
        u, v = nodes[rs.randint(0, k, NEG_BLOCK)], nodes[rs.randint(0, k, NEG_BLOCK)]
        cand = edge_keys(np.stack([u, v], axis=1), n_node)
        ok = (u != v) & ~_in_sorted(keys, cand) & ~np.isin(cand, kept)
        first = np.zeros(NEG_BLOCK, dtype=bool)
        first[np.unique(cand, return_index=True)[1]] = True  # a repeat inside the block: the first draw stays
        kept = np.concatenate([kept, cand[ok & first]])
    kept = kept[:n_neg]
    return np.stack([kept // n_node, kept % n_node], axis=1).astype(np.int32)


def split_edges(edges, n_node, ratio=0.1, seed=0, protect="forest", engine=None):
    """The split of the module's docstring -> (train int32 [m - n_test, 2], test int32 [n_test, 2], test_neg int32 [n_test, 2],
    stats dict).  ``engine``: an ``Engine`` whose resident graph is the graph of ``edges`` (``set_graph_csr(*edges_to_csr(n_node,
    edges))``): the edge list and the forest come from the device; None: from the host.  Both give the same arrays."""
    if protect not in ("forest", "none"):
        raise ValueError("split_edges: protect must be 'forest' or 'none', got %r" % (protect,))
    n_node, seed = int(n_node), int(seed) & 0xFFFFFFFF
    E = undirected_edge_list(edges, n_node)
    if engine is not None:
        if engine.n_node != n_node or not np.array_equal(engine.undirected_edges(), E):
            raise ValueError("split_edges: the engine's resident graph is not the graph of `edges`")
        sf = engine.spanning_forest(seed=seed)
    else:
        sf = host_spanning_forest(E, n_node, seed=seed)
    m = len(E)
    n_test = int(np.floor(float(ratio) * m + 0.5))
    cand = np.flatnonzero(sf["forest"] == 0) if protect == "forest" else np.arange(m)
    if n_test < 1 or n_test > len(cand):
        raise ValueError("split_edges: ratio = %r of %d edges asks for %d test edges, %d edges can be held out (protect = %r)"
                         % (ratio, m, n_test, len(cand), protect))
    rs = np.random.RandomState([seed, 0x5350])
    test_j = np.sort(cand[rs.permutation(len(cand))][:n_test])
    in_test = np.zeros(m, dtype=bool)
    in_test[test_j] = True
    test_neg = draw_negatives(rs, E, n_node, n_test)
    sizes = np.bincount(sf["component"], minlength=n_node)
    deg = np.bincount(E.reshape(-1), minlength=n_node)
    stats = dict(nodes=n_node, edges=m, components=int(sf["n_components"]), largest=int(sizes.max()) if n_node else 0, isolated=int((deg == 0).sum()),
                 forest=int(sf["n_forest"]), candidates=int(len(cand)), train=int(m - n_test), test=n_test, test_neg=int(len(test_neg)),
                 rounds=int(sf["rounds"]))
    return E[~in_test], E[test_j], test_neg, stats


SUMMARY_KEYS = ("nodes", "edges", "components", "largest", "isolated", "forest", "candidates", "train", "test", "test_neg", "rounds")


def format_summary(stats):
    return " ".join("%s=%d" % (k, stats[k]) for k in SUMMARY_KEYS)


def write_edge_file(path, rows):
    with open(path, "w") as f:
        f.writelines("%d\t%d\n" % (a, b) for a, b in np.asarray(rows).tolist())


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m graphgan_amd.split", description=__doc__.split("\n")[0])
    ap.add_argument("--edges", required=True, help="the edge list: lines of 'u v'")
    ap.add_argument("--out-prefix", required=True, help="writes <prefix>_train.txt, <prefix>_test.txt and <prefix>_test_neg.txt")
    ap.add_argument("--ratio", type=float, default=0.1, help="share of the edges held out (default 0.1)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the edge priorities and of the draws (default 0)")
    ap.add_argument("--protect", choices=("forest", "none"), default="forest",
                    help="forest: never hold out an edge of the spanning forest (default); none: any edge")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default 0)")
    ap.add_argument("--host", action="store_true", help="numpy on the host, no device")
    args = ap.parse_args(argv)
    rows = [r for r in utils.read_edges_from_file(args.edges) if r]
    if any(len(r) != 2 for r in rows):
        ap.error("--edges: every line must hold two node ids")
    edges = np.array(rows, dtype=np.int64).reshape(-1, 2)
    if edges.size == 0:
        ap.error("--edges: no edge")
    if edges.min() < 0:
        ap.error("--edges: negative node id")
    n = int(edges.max()) + 1
    if n > 2 ** 31 - 1:
        ap.error("node ids must be below 2^31 - 1")
    kw = dict(ratio=args.ratio, seed=args.seed, protect=args.protect)
    try:
        if args.host:
            train, test, neg, stats = split_edges(edges, n, **kw)
        else:
            from .engine import Engine, edges_to_csr
            table = np.zeros((n, 4), dtype=np.float32)  # (the sweeps read no embedding; a context needs tables)
            eng = Engine(table, table, device=args.device)
            try:
                eng.set_graph_csr(*edges_to_csr(n, edges))
                train, test, neg, stats = split_edges(edges, n, engine=eng, **kw)
            finally:
                eng.close()
    except ValueError as e:
        ap.error(str(e))
    for suffix, part in (("_train.txt", train), ("_test.txt", test), ("_test_neg.txt", neg)):
        write_edge_file(args.out_prefix + suffix, part)
    print(format_summary(stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
