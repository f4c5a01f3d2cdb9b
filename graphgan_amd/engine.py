"""numpy-facing wrapper of the C ABI (``include/graphgan_hip.h``).

``Engine`` is what the ``graph_gan.py`` mirror drives in place of the reference's
``tf.Session``: each method corresponds to one ``sess.run`` call site or host-side
sampler of ``src/GraphGAN/graph_gan.py`` (cited per method).  All numerics run in
``libgraphgan_hip.so``; nothing here computes scores, samples or updates.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import GGConfig, GGCounters, check, lib
from .evaluation.embedding_spectrum import pca_cov, pca_eig
from .evaluation import link_heuristics as _lheur
from .evaluation import label_propagation as _lprop
from .evaluation import graph_communities as _gcomm
from .evaluation import graph_ranking as _grank
from .evaluation import graph_ppr as _gppr


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


EDGE_OPERATORS = ("hadamard", "average", "l1", "l2")  # the `op` numbers 0 .. 3 of gg_edge_classifier_* (the node2vec paper's table)


def kmeans_pp_positions(m, k, seed, dist2_of):
    """The k-means++ draw of ``Engine.kmeans_seed`` (and of the host evaluator): ``dist2_of(positions so far)`` returns the m
    squared distances to the nearest chosen centre -> int64 [k] positions.  The rule is stated at ``Engine.kmeans_seed``."""
    rs = np.random.RandomState([int(seed), 0x4B4D])
    chosen = [int(rs.randint(m))]
    while len(chosen) < k:
        cum = np.cumsum(np.asarray(dist2_of(np.array(chosen, dtype=np.int64)), dtype=np.float64))
        total = float(cum[-1])
        if total == 0:
            chosen.append(int(rs.randint(m)))
        else:
            r = rs.random_sample() * total
            chosen.append(min(int(np.searchsorted(cum, r, side="right")), m - 1))
    return np.array(chosen, dtype=np.int64)


def pack_label_bits(Y, n_class):
    """bool / 0-1 matrix [m, C] -> the multi-hot mask of gg_classifier_ml_*: uint32 [m, ceil(C / 32)], bit c & 31 of word c >> 5
    = Y[i, c]."""
    Y = np.asarray(Y).astype(bool)
    C, CW = int(n_class), (int(n_class) + 31) // 32
    if Y.ndim != 2 or Y.shape[1] != C:
        raise ValueError("pack_label_bits: expected a matrix [m, %d], got %r" % (C, Y.shape))
    m = Y.shape[0]
    padded = np.zeros((m, 32 * CW), dtype=bool)
    padded[:, :C] = Y
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32, copy=False).reshape(m, CW)


def unpack_label_bits(bits, n_class):
    """the inverse of ``pack_label_bits``: uint32 [m, ceil(C / 32)] -> bool [m, C]"""
    bits = np.ascontiguousarray(bits, dtype="<u4")
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :int(n_class)].astype(bool)


def graph_to_csr(n_node, graph):
    """Adjacency dict of ``utils.read_edges`` -> (rowptr int64 [N+1], col int32), list order kept."""
    deg = np.fromiter((len(graph.get(v, ())) for v in range(n_node)), dtype=np.int64, count=n_node)
    rowptr = np.zeros(n_node + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.empty(int(rowptr[-1]), dtype=np.int32)
    for v in range(n_node):
        lst = graph.get(v)
        if lst:
            col[rowptr[v]:rowptr[v + 1]] = lst
    return rowptr, col


def edges_to_csr(n_node, edges):
    """Vectorised ``read_edges`` adjacency for large synthetic graphs: for edge k = (a, b) the
    reference appends b to graph[a] and then a to graph[b] (utils.py:36-37), in file order."""
    edges = np.asarray(edges).reshape(-1, 2)
    if len(edges) and (int(edges.min()) < 0 or int(edges.max()) >= n_node):  # (the C pass below writes unchecked)
        raise ValueError("edges_to_csr: node id outside [0, %d)" % n_node)
    if 2 * len(edges) < 2 ** 31 - 1:
        try:  # one stable counting pass in C (scipy's COO -> CSR kernel, called directly: no duplicate merging, no index sorting)
            from scipy.sparse import _sparsetools
            src = np.empty(2 * len(edges), dtype=np.int32)
            dst = np.empty(2 * len(edges), dtype=np.int32)
            src[0::2], dst[0::2] = edges[:, 0], edges[:, 1]
            src[1::2], dst[1::2] = edges[:, 1], edges[:, 0]
            indptr = np.zeros(n_node + 1, dtype=np.int32)
            col = np.empty(len(src), dtype=np.int32)
            nothing = np.zeros(len(src), dtype=np.int8)
            _sparsetools.coo_tocsr(n_node, n_node, len(src), src, dst, nothing, indptr, col, np.empty_like(nothing))
            return indptr.astype(np.int64), col
        except Exception:  # a private scipy routine: any change of its signature / dtype dispatch falls back to numpy
            pass
    edges = edges.astype(np.int64)
    src = np.empty(2 * len(edges), dtype=np.int64)
    dst = np.empty(2 * len(edges), dtype=np.int32)
    src[0::2], dst[0::2] = edges[:, 0], edges[:, 1]
    src[1::2], dst[1::2] = edges[:, 1], edges[:, 0]
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(n_node + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n_node), out=rowptr[1:])
    return rowptr, np.ascontiguousarray(dst[order])


def host_build_trees(n_node, rowptr, col, roots, n_threads=0):
    """``construct_trees`` (graph_gan.py:84-108) on host threads; no GPU needed.
    Returns (off int32 [R, N+1], nbr int32, nbr_base int64 [R+1], max_depth)."""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = _i32(col)
    roots = _i32(roots)
    R = len(roots)
    base = np.zeros(R + 1, dtype=np.int64)
    total = check(lib.gg_host_build_trees(n_node, _ptr(rowptr), _ptr(col), _ptr(roots), R, None, None, _ptr(base), 0,
                                          n_threads, None))
    off = np.zeros((R, n_node + 1), dtype=np.int32)
    nbr = np.zeros(max(int(total), 1), dtype=np.int32)
    dmax = np.zeros(1, dtype=np.int32)
    check(lib.gg_host_build_trees(n_node, _ptr(rowptr), _ptr(col), _ptr(roots), R, _ptr(off), _ptr(nbr), _ptr(base),
                                  int(total), n_threads, _ptr(dmax)))
    return off, nbr[: int(total)], base, int(dmax[0])


def read_edges_csr(train_filename, test_filename=""):
    """``utils.read_edges`` (utils.py:12-54) natively -> (n_node, rowptr int64 [N+1], col int32), list order kept."""
    g = _lib.GGGraph()
    check(lib.gg_host_read_edges(str(train_filename).encode(), str(test_filename or "").encode(), ctypes.byref(g)))
    try:
        rowptr = np.ctypeslib.as_array(g.rowptr, shape=(g.n_node + 1,)).copy()
        col = np.ctypeslib.as_array(g.col, shape=(max(g.nnz, 1),))[: g.nnz].copy()
        return int(g.n_node), rowptr, col
    finally:
        lib.gg_host_free_graph(ctypes.byref(g))


class CSRGraph:
    """Read-only stand-in for the reference's adjacency dict (``graph[i]`` -> list of neighbours)."""

    def __init__(self, rowptr, col):
        self.rowptr, self.col = rowptr, col

    def __len__(self):
        return len(self.rowptr) - 1

    def __getitem__(self, v):
        return self.col[self.rowptr[v]:self.rowptr[v + 1]].tolist()

    def get(self, v, default=None):
        return self[v] if 0 <= v < len(self) else default

    def keys(self):
        return range(len(self))

    def __iter__(self):
        return iter(range(len(self)))

    def __contains__(self, v):
        return 0 <= v < len(self)


def host_write_embeddings(path, emb, n_threads=0):
    """The reference's ``.emb`` text (graph_gan.py:293-306), byte-identical, from host threads."""
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    check(lib.gg_host_write_embeddings(_ptr(emb), emb.shape[0], emb.shape[1], str(path).encode(), n_threads))


def synth_powerlaw(n_node, m, seed_graph=1, seed_perm=2):
    """Barabasi-Albert edge list [E, 2] int32 (SURVEY.md section 8d recipe)."""
    n = check(lib.gg_synth_powerlaw(n_node, m, seed_graph, seed_perm, None, 0))
    edges = np.empty((int(n), 2), dtype=np.int32)
    check(lib.gg_synth_powerlaw(n_node, m, seed_graph, seed_perm, _ptr(edges), int(n)))
    return edges


class Engine:
    """One HIP context on one MI355X: both embedding models, graph, trees, sample buffers."""

    def __init__(self, emb_gen, emb_dis, lr_gen=1e-3, lr_dis=1e-3, lambda_gen=1e-5, lambda_dis=1e-5, window_size=2,
                 optimizer=_lib.GG_OPT_ADAM_DENSE, device=0, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8):
        eg = np.ascontiguousarray(emb_gen, dtype=np.float32)  # Q6: fp64 init rounded to fp32 once
        ed = np.ascontiguousarray(emb_dis, dtype=np.float32)
        assert eg.shape == ed.shape and eg.ndim == 2
        self.n_node, self.n_emb = int(eg.shape[0]), int(eg.shape[1])
        cfg = GGConfig(lr_gen, lr_dis, lambda_gen, lambda_dis, adam_beta1, adam_beta2, adam_eps, window_size, optimizer, device)
        self._ctx = ctypes.c_void_p()
        check(lib.gg_create(self.n_node, self.n_emb, _ptr(eg), _ptr(ed), ctypes.byref(cfg), ctypes.byref(self._ctx)))
        self.tree_roots = np.zeros(0, dtype=np.int32)
        self.max_depth = 0
        self._rowptr = None
        self._col = None
        self._set_adj = None
        self.tree_mode = (-1, 0)  # (mode, node_cap) of the last set_tree_mode: the library's default until then
        self.last_graph_softmax_ms = 0.0

    # ------------------------------------------------------------------ life cycle
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            lib.gg_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        return check(rc, self._ctx)

    # ------------------------------------------------------------------ graph / trees
    def set_graph_csr(self, rowptr, col):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        col = _i32(col)
        self._ck(lib.gg_set_graph_csr(self._ctx, _ptr(rowptr), _ptr(col)))
        self._rowptr = rowptr
        self._col = col
        self._set_adj = None  # (the neighbour sets on the host, built when two_hop_rank first derives a full rank)

    def build_trees(self, roots, n_threads=0, device=False):
        """graph_gan.py:31-46,84-108: BFS trees of ``roots`` -> device tree CSR (slot i = roots[i]).
        device=False: threaded host BFS + upload; device=True: BFS on the GPU (same trees)."""
        roots = _i32(roots)
        if device:
            self._ck(lib.gg_build_trees_device(self._ctx, _ptr(roots), len(roots)))
        else:
            self._ck(lib.gg_build_trees(self._ctx, _ptr(roots), len(roots), n_threads))
        self._after_trees(roots)

    def tree_bytes_estimate(self, n_roots):
        """Upper bound of the HBM bytes ``n_roots`` resident trees need (every root reaching every node)."""
        return float(n_roots) * 12.0 * (self.n_node + 1)  # pop order + first-child ranks + edge indices

    def set_tree_mode(self, mode, node_cap=0):
        """gg_set_tree_mode: 0 = whole trees, 1 = lazy trees (exact through a level, children lists below it resolved by the
        walks that need them -- same walks, bit for bit), -1 = lazy from 2^18 nodes on (the default)."""
        self._ck(lib.gg_set_tree_mode(self._ctx, int(mode), int(node_cap)))
        self.tree_mode = (int(mode), int(node_cap))

    def lazy_stats(self):
        out = np.zeros(24, dtype=np.int64)
        self._ck(lib.gg_lazy_stats(self._ctx, _ptr(out)))
        return dict(lazy=bool(out[0]), min_level=int(out[1]), fallback_roots=int(out[2]), fallback_rounds=int(out[3]), exact_nodes=int(out[4]),
                    pool_entries=int(out[5]), lazy_slots=int(out[6]), max_level=int(out[7]), resolved=[int(x) for x in out[8:11]],
                    candidates=int(out[11]), scan_rounds=int(out[12]), max_rounds=int(out[13]), max_degree_resolved=int(out[14]), coop_lists=int(out[15]),
                    slots_by_level=[int(x) for x in out[16:24]])

    def get_lazy_trees(self):
        """Raw arrays of the resident LAZY trees (tests): dict(info [R, 4], base [R], order, cstart, edge, pair)."""
        R = len(self.tree_roots)
        n = ctypes.c_int64()
        self._ck(lib.gg_get_lazy_trees(self._ctx, ctypes.byref(n), None, None, None, None, None, None))
        n = n.value
        info, base = np.zeros((R, 4), np.int32), np.zeros(R, np.int64)
        order, cstart, edge, pair = np.zeros(n, np.int32), np.zeros(n + R, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
        self._ck(lib.gg_get_lazy_trees(self._ctx, None, _ptr(info), _ptr(base), _ptr(order), _ptr(cstart), _ptr(edge), _ptr(pair)))
        return dict(info=info, base=base, order=order, cstart=cstart, edge=edge, pair=pair)

    def set_trees(self, roots, off, nbr, nbr_base, max_depth=0):
        roots, off, nbr = _i32(roots), _i32(off), _i32(nbr)
        nbr_base = np.ascontiguousarray(nbr_base, dtype=np.int64)
        self._ck(lib.gg_set_trees(self._ctx, _ptr(roots), len(roots), _ptr(off), _ptr(nbr), _ptr(nbr_base), max_depth))
        self._after_trees(roots)

    def _after_trees(self, roots):
        self.tree_roots = roots.copy()
        nr, ne, md = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
        self._ck(lib.gg_tree_info(self._ctx, ctypes.byref(nr), ctypes.byref(ne), ctypes.byref(md)))
        self.tree_entries, self.max_depth = ne.value, md.value

    def save_trees(self, path):
        """The tree cache (reference: pickle.dump(self.trees), graph_gan.py:43-46)."""
        self._ck(lib.gg_save_trees(self._ctx, str(path).encode()))

    def load_trees(self, path):
        """pickle.load of the cache (graph_gan.py:35-38): the resident trees as saved by ``save_trees``; refuses a
        cache built from another graph."""
        self._ck(lib.gg_load_trees(self._ctx, str(path).encode()))
        nr = ctypes.c_int32()
        self._ck(lib.gg_tree_info(self._ctx, ctypes.byref(nr), None, None))
        roots = np.zeros(nr.value, dtype=np.int32)
        self._ck(lib.gg_tree_roots(self._ctx, _ptr(roots)))
        self._after_trees(roots)

    def get_trees(self):
        R = len(self.tree_roots)
        off = np.zeros((R, self.n_node + 1), dtype=np.int32)
        nbr = np.zeros(max(self.tree_entries, 1), dtype=np.int32)
        base = np.zeros(R + 1, dtype=np.int64)
        self._ck(lib.gg_get_trees(self._ctx, _ptr(off), _ptr(nbr), _ptr(base)))
        return off, nbr[: self.tree_entries], base

    def get_tree_order(self):
        """The resident trees in BFS-order form: (base [R+1], order, cstart, edge, edges_valid) -- see gg_get_tree_order."""
        R = len(self.tree_roots)
        base = np.zeros(R + 1, dtype=np.int64)
        self._ck(lib.gg_get_tree_order(self._ctx, _ptr(base), None, None, None, None))
        nodes = int(base[R])
        order, cstart, edge = np.zeros(nodes, np.int32), np.zeros(nodes + R, np.int32), np.zeros(nodes, np.int32)
        valid = ctypes.c_int32()
        self._ck(lib.gg_get_tree_order(self._ctx, _ptr(base), _ptr(order), _ptr(cstart), _ptr(edge), ctypes.byref(valid)))
        return base, order, cstart, edge, bool(valid.value)

    # ------------------------------------------------------------------ K1
    def walk_sample(self, slots, n_walks, for_d, seed, stream, stride=None, fetch=True):
        """GraphGAN.sample (graph_gan.py:225-270) for many roots at once."""
        slots, n_walks = _i32(slots), _i32(n_walks)
        stride = int(stride or (self.max_depth + 3))
        total = int(n_walks.sum())
        if not fetch:
            self._ck(lib.gg_walk_sample(self._ctx, _ptr(slots), _ptr(n_walks), len(slots), int(bool(for_d)), seed, stream,
                                        None, None, None, stride, None))
            return None
        samples = np.full(total, -1, dtype=np.int32)
        paths = np.full((total, stride), -1, dtype=np.int32)
        plen = np.zeros(total, dtype=np.int32)
        status = np.zeros(len(slots), dtype=np.int32)
        self._ck(lib.gg_walk_sample(self._ctx, _ptr(slots), _ptr(n_walks), len(slots), int(bool(for_d)), seed, stream,
                                    _ptr(samples), _ptr(paths), _ptr(plen), stride, _ptr(status)))
        self._after_trees(self.tree_roots)  # (lazy trees: slots rebuilt whole may have raised the depth)
        return dict(samples=samples, paths=paths, path_len=plen, root_status=status)

    def get_walks(self):
        """Walk outputs left resident by the last walk_sample / prepare_d / prepare_g call (the (samples, paths)
        ``sample`` returned inside ``prepare_data_for_*``, graph_gan.py:191,210)."""
        tot, stride, ns = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self._ck(lib.gg_walk_info(self._ctx, ctypes.byref(tot), ctypes.byref(stride), ctypes.byref(ns)))
        total, stride, ns = tot.value, stride.value, ns.value
        samples = np.full(total, -1, dtype=np.int32)
        paths = np.full((total, max(stride, 1)), -1, dtype=np.int32)
        plen = np.zeros(total, dtype=np.int32)
        status = np.zeros(ns, dtype=np.int32)
        self._ck(lib.gg_get_walks(self._ctx, _ptr(samples), _ptr(paths), _ptr(plen), _ptr(status)))
        return dict(samples=samples, paths=paths, path_len=plen, root_status=status)

    # ------------------------------------------------------------------ prepared data
    def prepare_d(self, slots, seed, stream, fetch=True):
        """prepare_data_for_d (graph_gan.py:182-202) -> (center, neighbor, label, root_status)."""
        slots = _i32(slots)
        n = ctypes.c_int64()
        status = np.zeros(len(slots), dtype=np.int32) if fetch else None  # no status read-back for resident-only use
        self._ck(lib.gg_prepare_d(self._ctx, _ptr(slots), len(slots), seed, stream, ctypes.byref(n), _ptr(status) if fetch else None))
        self.d_rows = n.value
        if not fetch:
            return n.value
        c, nb, lab = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.float32)
        self._ck(lib.gg_get_d_data(self._ctx, _ptr(c), _ptr(nb), _ptr(lab)))
        return c, nb, lab, status

    def prepare_g(self, slots, n_sample, seed, stream, fetch=True):
        """prepare_data_for_g (graph_gan.py:204-223) -> (node_1, node_2, reward, root_status)."""
        slots = _i32(slots)
        n = ctypes.c_int64()
        status = np.zeros(len(slots), dtype=np.int32) if fetch else None
        self._ck(lib.gg_prepare_g(self._ctx, _ptr(slots), len(slots), n_sample, seed, stream, ctypes.byref(n), _ptr(status) if fetch else None))
        self.g_pairs = n.value
        if not fetch:
            return n.value
        a, b, r = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.float32)
        self._ck(lib.gg_get_g_data(self._ctx, _ptr(a), _ptr(b), _ptr(r)))
        return a, b, r, status

    def prepare_g_begin(self, slots, n_sample, seed, stream):
        """Optional head start: enqueue the walks of the NEXT prepare_g (same arguments) on the side stream now -- before
        the d_pass that precedes it -- without waiting for anything (gg_prepare_g_begin)."""
        slots = _i32(slots)
        self._ck(lib.gg_prepare_g_begin(self._ctx, _ptr(slots), len(slots), n_sample, seed, stream))

    # ------------------------------------------------------------------ skip-gram pre-training rows
    def pretrain_set_noise(self, weights=None):
        """Noise distribution of the negatives of ``prepare_pretrain`` (gg_pretrain_set_noise): uint32 weights per node,
        or None = uniform.  ``set_graph_csr`` drops it."""
        if weights is None:
            self._ck(lib.gg_pretrain_set_noise(self._ctx, None))
            return
        w = np.asarray(weights)
        if w.shape != (self.n_node,) or not np.issubdtype(w.dtype, np.integer):
            raise ValueError("pretrain_set_noise: weights must be %d integers" % self.n_node)
        if w.size and (int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF):
            raise ValueError("pretrain_set_noise: weights must fit uint32")
        if not w.any():
            raise ValueError("pretrain_set_noise: every weight is zero")
        w = np.ascontiguousarray(w, dtype=np.uint32)
        self._ck(lib.gg_pretrain_set_noise(self._ctx, _ptr(w)))

    def pretrain_set_walk_bias(self, w_ret, w_com, w_out):
        """node2vec bias of the walks of ``prepare_pretrain`` (gg_pretrain_set_walk_bias; contract P2b): integer weights in
        [1, 65536] of stepping back to the previous node, to a neighbour of it, and to any other neighbour.  Equal weights
        are the uniform walk.  Kept across ``set_graph_csr``; ``pretrain.walk_bias(p, q)`` gives the weights of (p, q)."""
        for name, val in (("w_ret", w_ret), ("w_com", w_com), ("w_out", w_out)):
            if isinstance(val, (bool, np.bool_)) or not isinstance(val, (int, np.integer)) or not 1 <= int(val) <= 65536:
                raise ValueError("pretrain_set_walk_bias: %s must be an integer in [1, 65536], got %r" % (name, val))
        self._ck(lib.gg_pretrain_set_walk_bias(self._ctx, int(w_ret), int(w_com), int(w_out)))

    def prepare_pretrain(self, starts, walks_per_start, walk_len, window, n_neg, seed, stream, fetch=False):
        """Skip-gram rows from random walks -- uniform, or biased after ``pretrain_set_walk_bias`` -- (gg_prepare_pretrain;
        contract P1-P5 in include/graphgan_hip.h):
        ``walks_per_start`` walks of ``walk_len`` nodes from every node of ``starts``, window pairs as positives, ``n_neg``
        negatives per pair.  The rows replace the resident discriminator rows (``get_d_data`` / ``d_pass``).  Returns the row
        count, or with ``fetch`` (rows, paths int32 [walks, walk_len] with -1 behind a walk's end, path_len int32 [walks])."""
        starts_a = np.asarray(starts)
        if starts_a.ndim != 1 or (starts_a.size and not np.issubdtype(starts_a.dtype, np.integer)):
            raise ValueError("prepare_pretrain: starts must be a 1-d array of integers")
        if starts_a.size and (int(starts_a.min()) < 0 or int(starts_a.max()) >= self.n_node):
            raise ValueError("prepare_pretrain: start outside [0, %d)" % self.n_node)
        for name, val, lo, hi in (("walks_per_start", walks_per_start, 1, 2 ** 31 - 1), ("walk_len", walk_len, 1, 256),
                                  ("window", window, 1, 16), ("n_neg", n_neg, 0, 64), ("seed", seed, 0, 2 ** 64 - 1),
                                  ("stream", stream, 0, 2 ** 32 - 1)):
            if isinstance(val, bool) or int(val) != val or not lo <= int(val) <= hi:
                raise ValueError("prepare_pretrain: %s must be an integer in [%d, %d], got %r" % (name, lo, hi, val))
        if self.n_node < 3:
            raise ValueError("prepare_pretrain: needs at least 3 nodes")
        starts_a = _i32(starts_a)
        nw = len(starts_a) * int(walks_per_start)
        if nw > 2 ** 31 - 1:
            raise ValueError("prepare_pretrain: %d walks in one call" % nw)
        paths = np.empty((nw, int(walk_len)), dtype=np.int32) if fetch else None
        plen = np.empty(nw, dtype=np.int32) if fetch else None
        n = ctypes.c_int64()
        self._ck(lib.gg_prepare_pretrain(self._ctx, _ptr(starts_a), len(starts_a), int(walks_per_start), int(walk_len), int(window),
                                         int(n_neg), int(seed), int(stream), ctypes.byref(n), _ptr(paths), _ptr(plen)))
        self.d_rows = n.value
        if not fetch:
            return n.value
        return n.value, paths, plen

    # ------------------------------------------------------------------ an epoch over root batches (trees not all resident)
    def epoch_begin(self, reset_d=True, reset_g=True):
        """Empty the accumulated discriminator rows / generator pairs of gg_epoch_add."""
        self._ck(lib.gg_epoch_begin(self._ctx, int(bool(reset_d)), int(bool(reset_g))))

    def epoch_add(self, roots, do_d=True, do_g=True, n_sample=20, seed=0, stream_d=0, stream_g=1):
        """prepare_data_for_d / prepare_data_for_g (graph_gan.py:182-223) for one BATCH of roots (node ids): trees built on
        the GPU, the roots' Q3 bits restored from / saved to the persistent store, rows and pairs appended to the epoch's
        arrays.  Returns (rows accumulated so far, pairs accumulated so far)."""
        roots = _i32(roots)
        rows, pairs = ctypes.c_int64(), ctypes.c_int64()
        self._ck(lib.gg_epoch_add(self._ctx, _ptr(roots), len(roots), int(bool(do_d)), int(bool(do_g)), int(n_sample), seed, stream_d,
                                  stream_g, ctypes.byref(rows), ctypes.byref(pairs)))
        if len(roots) and (do_d or do_g):
            self._after_trees(roots)
        return rows.value, pairs.value

    def epoch_commit(self, which):
        """The accumulated rows (which = 1) / pairs with their rewards (which = 0) become the data of d_pass / g_pass; returns their number."""
        n = ctypes.c_int64()
        self._ck(lib.gg_epoch_commit(self._ctx, int(which), ctypes.byref(n)))
        if which == 1:
            self.d_rows = n.value
        else:
            self.g_pairs = n.value
        return n.value

    def get_d_data(self):
        """The resident discriminator rows (center, neighbor, label) -- of the last prepare_d or epoch_commit(1)."""
        n = self.d_rows
        c, nb, lab = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        self._ck(lib.gg_get_d_data(self._ctx, _ptr(c), _ptr(nb), _ptr(lab)))
        return c, nb, lab

    def get_g_data(self):
        """The resident generator pairs (node_1, node_2, reward) -- of the last prepare_g or epoch_commit(0)."""
        n = self.g_pairs
        a, b, r = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        self._ck(lib.gg_get_g_data(self._ctx, _ptr(a), _ptr(b), _ptr(r)))
        return a, b, r

    def q3_clear(self):
        """Forget every in-place tree mutation (graph_gan.py:258-259) kept for the root-batched epochs."""
        self._ck(lib.gg_q3_clear(self._ctx))

    def q3_get(self):
        """(word_off int64 [N+1], words uint32): bit j of root v's words = the father entry of its (j+1)-th tree child was removed."""
        off = np.zeros(self.n_node + 1, dtype=np.int64)
        self._ck(lib.gg_q3_get(self._ctx, _ptr(off), None))
        words = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        self._ck(lib.gg_q3_get(self._ctx, None, _ptr(words)))
        return off, words[: int(off[-1])]

    def d_pass(self, starts, batch_size):
        """One inner D epoch over the prepared rows (graph_gan.py:149-157)."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        self._ck(lib.gg_d_pass(self._ctx, _ptr(starts), len(starts), batch_size))

    def g_pass(self, starts, batch_size):
        """One inner G epoch over the prepared pairs (graph_gan.py:168-176)."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        self._ck(lib.gg_g_pass(self._ctx, _ptr(starts), len(starts), batch_size))

    # ------------------------------------------------------------------ sess.run call sites with host buffers
    def pair_reward(self, u, v):
        """sess.run(discriminator.reward) (graph_gan.py:220-222)."""
        u, v = _i32(u), _i32(v)
        out = np.zeros(len(u), dtype=np.float32)
        self._ck(lib.gg_pair_reward(self._ctx, _ptr(u), _ptr(v), len(u), _ptr(out)))
        return out

    def d_step(self, u, v, label):
        """sess.run(discriminator.d_updates) (graph_gan.py:154-157)."""
        u, v, label = _i32(u), _i32(v), np.ascontiguousarray(label, dtype=np.float32)
        self._ck(lib.gg_d_step(self._ctx, _ptr(u), _ptr(v), _ptr(label), len(u)))

    def g_step(self, u, v, reward):
        """sess.run(generator.g_updates) (graph_gan.py:173-176)."""
        u, v, reward = _i32(u), _i32(v), np.ascontiguousarray(reward, dtype=np.float32)
        self._ck(lib.gg_g_step(self._ctx, _ptr(u), _ptr(v), _ptr(reward), len(u)))

    def all_score(self, rows=None):
        """sess.run(generator.all_score) (graph_gan.py:238) for ``rows`` (None: all) -> fp32 [len(rows), n_node]."""
        if rows is None:
            out = np.zeros((self.n_node, self.n_node), dtype=np.float32)
            self._ck(lib.gg_all_score(self._ctx, None, 0, _ptr(out)))
            return out
        rows = _i32(rows)
        out = np.zeros((len(rows), self.n_node), dtype=np.float32)
        self._ck(lib.gg_all_score(self._ctx, _ptr(rows), len(rows), _ptr(out)))
        return out

    def all_score_reduce(self, rows=None, precision="fp32", logsumexp=True):
        """Rows of ``generator.all_score`` (generator.py:21) streamed through a fused consumer: per row the maximum, its
        column and log-sum-exp over ALL nodes; nothing of size rows x N is materialised.  precision "fp32" (exact) or
        "bf16" (bf16 inputs on the matrix cores, fp32 accumulate).  Returns dict(max, argmax, logsumexp, kernel_ms)."""
        n_rows = self.n_node if rows is None else len(rows)
        rows_a = None if rows is None else _i32(rows)
        mx = np.zeros(n_rows, dtype=np.float32)
        am = np.zeros(n_rows, dtype=np.int32)
        lse = np.zeros(n_rows, dtype=np.float32) if logsumexp else None
        ms = ctypes.c_double()
        self._ck(lib.gg_all_score_reduce(self._ctx, _ptr(rows_a), n_rows, {"fp32": 0, "bf16": 1}[precision], int(bool(logsumexp)),
                                         _ptr(mx), _ptr(am), _ptr(lse), ctypes.byref(ms)))
        return dict(max=mx, argmax=am, logsumexp=lse, kernel_ms=ms.value)

    TOPK_METRICS = ("dot", "cosine", "l2")  # the `metric` numbers 0 .. 2 of gg_topk_metric

    def topk(self, rows=None, k=10, which=0, precision="fp32", exclude=False, metric="dot", candidates=None):
        """Streamed top-K retrieval (gg_topk_scores / gg_topk_metric): for each node of ``rows`` (None: every node) the ``k`` best
        columns of model ``which`` (0 = gen, 1 = dis) under ``metric``:

            "dot"     E[u] . E[c] (no bias), best = largest; ``score`` is the dot product
            "cosine"  E[u] . E[c] / (|E[u]| |E[c]|), best = largest; a zero row scores 0 with everything
            "l2"      |E[u] - E[c]|, best = SMALLEST: ``score`` is the SQUARED distance and every list is nearest first,
                      non-decreasing

        Ties go to the lower column.  ``exclude``: False every node, True without u itself and u's neighbours in the resident
        training graph, "self" without u itself (needs no graph).  ``candidates``: node ids (free to repeat; may be empty) --
        only they are eligible.  Rows with fewer than ``k`` eligible columns are padded with col -1 and score -inf (l2: +inf).
        precision "fp32" (exact scores) or "bf16" (bf16 inputs, fp32 accumulate).  Nothing of size rows x N is materialised.
        ``metric="dot"`` without candidates and with a bool ``exclude`` is gg_topk_scores, as before.
        Returns dict(col int32 [n_rows, k], score fp32 [n_rows, k], kernel_ms)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("topk: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        if which not in (0, 1):
            raise ValueError("topk: which must be 0 (generator) or 1 (discriminator), got %r" % (which,))
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= 256:
            raise ValueError("topk: k must be an integer in [1, 256], got %r" % (k,))
        if metric not in self.TOPK_METRICS:
            raise ValueError("topk: metric must be 'dot', 'cosine' or 'l2', got %r" % (metric,))
        if isinstance(exclude, str) and exclude != "self":
            raise ValueError("topk: exclude must be False, True or 'self', got %r" % (exclude,))
        k = int(k)
        rows_a = None if rows is None else _i32(rows).reshape(-1)
        n_rows = self.n_node if rows_a is None else len(rows_a)
        col = np.empty((n_rows, k), dtype=np.int32)
        score = np.empty((n_rows, k), dtype=np.float32)
        ms = ctypes.c_double()
        prec = {"fp32": 0, "bf16": 1}[precision]
        if metric == "dot" and candidates is None and not isinstance(exclude, str):
            self._ck(lib.gg_topk_scores(self._ctx, which, _ptr(rows_a), n_rows, k, prec, int(bool(exclude)), _ptr(col), _ptr(score), ctypes.byref(ms)))
        else:
            n_cand, cand_a = 0, None
            if candidates is not None:
                cand_a = _i32(candidates).reshape(-1)
                n_cand = len(cand_a)
                if n_cand == 0:
                    cand_a = np.zeros(1, dtype=np.int32)  # (an empty set still needs a pointer: NULL means "no set")
            self._ck(lib.gg_topk_metric(self._ctx, which, _ptr(rows_a), n_rows, k, prec, self.TOPK_METRICS.index(metric),
                                        2 if exclude == "self" else int(bool(exclude)), _ptr(cand_a), n_cand, _ptr(col), _ptr(score), ctypes.byref(ms)))
        return dict(col=col, score=score, kernel_ms=ms.value)

    def rank(self, u, v, which=0, precision="fp32", exclude=False):
        """Full-ranking link evaluation (gg_rank_scores): for each query (u[i], v[i]) the exact rank of column v[i] in row u[i]
        of E . E^T (no bias) of model ``which`` (0 = gen, 1 = dis) among all candidates, in ``topk``'s order (score
        descending, column ascending); with ``exclude`` the candidates are every node but u[i] and its neighbours in the
        resident training graph -- and always the target itself.  precision "fp32" (exact) or "bf16" (bf16 inputs, fp32
        accumulate).  Nothing of size queries x N is materialised.  Returns dict(rank int32 [m] (1 = best), n_cand int32 [m],
        score fp32 [m] = s(u, v), kernel_ms)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("rank: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        if which not in (0, 1):
            raise ValueError("rank: which must be 0 (generator) or 1 (discriminator), got %r" % (which,))
        u_a, v_a = _i32(u).reshape(-1), _i32(v).reshape(-1)
        if len(u_a) != len(v_a):
            raise ValueError("rank: u and v must have the same length, got %d and %d" % (len(u_a), len(v_a)))
        m = len(u_a)
        rank = np.empty(m, dtype=np.int32)
        n_cand = np.empty(m, dtype=np.int32)
        score = np.empty(m, dtype=np.float32)
        ms = ctypes.c_double()
        if m:
            self._ck(lib.gg_rank_scores(self._ctx, which, _ptr(u_a), _ptr(v_a), m, {"fp32": 0, "bf16": 1}[precision], int(bool(exclude)),
                                        _ptr(rank), _ptr(n_cand), _ptr(score), ctypes.byref(ms)))
        return dict(rank=rank, n_cand=n_cand, score=score, kernel_ms=ms.value)

    TOP_PAIRS_MAX_K = 1 << 20  # the limit of gg_top_pairs

    def top_pairs(self, k, nodes=None, which=0, precision="fp32", exclude=True, buffer_entries=None):
        """Global top-K pair prediction (gg_top_pairs): the ``k`` best-scored unordered pairs {u, v}, u < v, of ``nodes`` (None:
        every node; else node ids, strictly ascending) under s(u, v) = E[u] . E[v] (no bias) of model ``which`` (0 = gen,
        1 = dis) -- the bits ``rank(u, v, exclude=False)`` reports -- with ``exclude`` without the pairs whose v is a neighbour of
        u in the resident training graph.  Order: score descending (-0 counts as +0), then (u, v) ascending.  precision "fp32"
        (exact scores) or "bf16" (bf16 inputs, fp32 accumulate).  ``buffer_entries``: None the default max(2^22, 4 k), else the
        device buffer's entries in [k + 4096, 2^26]; it changes no output but ``stats``.  One sweep of the tile stream; nothing
        of size nodes x nodes is materialised.  Returns dict(u int32 [k], v int32 [k], score fp32 [k] (-1, -1, -inf behind
        n_found), n_found = min(k, candidates), stats = dict(launches, retries, compactions, appended, compaction_ms,
        buffer_entries), ms)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("top_pairs: precision must be 'fp32' or 'bf16', got %r" % (precision,))
        if which not in (0, 1):
            raise ValueError("top_pairs: which must be 0 (generator) or 1 (discriminator), got %r" % (which,))
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= self.TOP_PAIRS_MAX_K:
            raise ValueError("top_pairs: k must be an integer in [1, 2^20], got %r" % (k,))
        k = int(k)
        if buffer_entries is not None and (isinstance(buffer_entries, bool) or int(buffer_entries) != buffer_entries
                                           or not k + 4096 <= int(buffer_entries) <= 1 << 26):
            raise ValueError("top_pairs: buffer_entries must be None or an integer in [k + 4096, 2^26], got %r" % (buffer_entries,))
        nodes_a = None if nodes is None else _i32(nodes).reshape(-1)
        if nodes_a is not None and len(nodes_a) == 0:
            nodes_a = np.zeros(1, dtype=np.int32)  # (an empty set still needs a pointer: NULL means "every node")
        m = 0 if nodes is None else len(_i32(nodes).reshape(-1))
        u = np.empty(k, dtype=np.int32)
        v = np.empty(k, dtype=np.int32)
        score = np.empty(k, dtype=np.float32)
        n_found = ctypes.c_int64()
        stats = np.zeros(6, dtype=np.int64)
        ms = ctypes.c_double()
        self._ck(lib.gg_top_pairs(self._ctx, which, {"fp32": 0, "bf16": 1}[precision], _ptr(nodes_a), m, k, int(bool(exclude)),
                                  0 if buffer_entries is None else int(buffer_entries), _ptr(u), _ptr(v), _ptr(score), ctypes.byref(n_found),
                                  _ptr(stats), ctypes.byref(ms)))
        return dict(u=u, v=v, score=score, n_found=int(n_found.value),
                    stats=dict(launches=int(stats[0]), retries=int(stats[1]), compactions=int(stats[2]), appended=int(stats[3]),
                               compaction_ms=stats[4] / 1000.0, buffer_entries=int(stats[5])), ms=ms.value)

    PAIR_NEIGHBORS_CHUNK = _lib.PAIR_NEIGHBORS_CHUNK  # entries of a pair's shorter neighbour list per task of the sweep (longer lists are split)

    def distinct_degrees(self):
        """deg(x) = |N(x)| of every node of the resident training graph (gg_distinct_degrees), N(x) the distinct entries of x's
        list other than x itself: int32 [n_node]."""
        deg = np.empty(self.n_node, dtype=np.int32)
        self._ck(lib.gg_distinct_degrees(self._ctx, _ptr(deg)))
        return deg

    def pair_neighbors(self, u, v, weights=None):
        """The pair-neighbour sweep (gg_pair_neighbors): for each pair (u[i], v[i]) the common neighbours C = (N(u) & N(v)) \\ {u, v}
        in the resident training graph -- neighbour SETS: duplicates and self-loops of the lists do not count; u == v gives
        C = N(u).  ``weights``: None or a uint64 array [n_w, n_node], n_w <= 4, of fixed-point node weights; they are summed over
        C as unsigned 64-bit integers, so exchanging the ends, permuting the pairs or running again changes no bit
        (max(weights) * max(deg) must fit in 63 bits).  No embedding table is read.  Returns dict(cn int32 [m] = |C|, deg_u int32
        [m], deg_v int32 [m], wsum uint64 [n_w, m], kernel_ms)."""
        u_a, v_a = _i32(u).reshape(-1), _i32(v).reshape(-1)
        if len(u_a) != len(v_a):
            raise ValueError("pair_neighbors: u and v must have the same length, got %d and %d" % (len(u_a), len(v_a)))
        w_a, n_w = None, 0
        if weights is not None:
            w_a = np.ascontiguousarray(weights, dtype=np.uint64)
            if w_a.ndim != 2 or w_a.shape[1] != self.n_node:
                raise ValueError("pair_neighbors: weights must be a uint64 array [n_w, %d], got shape %r" % (self.n_node, w_a.shape))
            n_w = int(w_a.shape[0])
        m = len(u_a)
        cn, deg_u, deg_v = (np.empty(m, dtype=np.int32) for _ in range(3))
        wsum = np.empty((n_w, m), dtype=np.uint64)
        ms = ctypes.c_double()
        self._ck(lib.gg_pair_neighbors(self._ctx, _ptr(u_a), _ptr(v_a), m, _ptr(w_a) if n_w else None, n_w, _ptr(cn), _ptr(deg_u), _ptr(deg_v),
                                       _ptr(wsum) if n_w else None, ctypes.byref(ms)))
        return dict(cn=cn, deg_u=deg_u, deg_v=deg_v, wsum=wsum, kernel_ms=ms.value)

    def link_heuristics(self, u, v):
        """The neighbourhood link-prediction indices of the pairs (u[i], v[i]) on the resident training graph
        (evaluation/link_heuristics.py): one ``pair_neighbors`` sweep with the fixed-point Adamic-Adar and resource-allocation
        weights of ``link_heuristics.node_weights(distinct_degrees())``.  Returns dict(cn int64 [m], jaccard float64 [m], aa
        float64 [m], ra float64 [m], pa int64 [m]); aa and ra are within cn * 2^-41 of the un-quantised sums."""
        res = self.pair_neighbors(u, v, _lheur.node_weights(self.distinct_degrees()))
        return _lheur.indices(res["cn"], res["deg_u"], res["deg_v"], res["wsum"])

    NEIGHBOR_SUM_CHUNK = _lib.NEIGHBOR_SUM_CHUNK  # neighbours of a node per task of the neighbour-sum sweep (a node with more is split)

    def _gp_scale(self, fn, name, scale):
        if scale is None:
            return None
        a = np.ascontiguousarray(scale, dtype=np.float32)
        if a.shape != (self.n_node,):
            raise ValueError("%s: %s must be a float array [%d] or None, got shape %r" % (fn, name, self.n_node, a.shape))
        return a

    def neighbor_sum(self, X, in_scale=None, out_scale=None, nodes=None):
        """The neighbour-sum sweep (gg_neighbor_sum) on the neighbour SETS N(v) of the resident training graph (those of
        ``pair_neighbors``): out[i, c] = out_scale[v] * sum over w in N(v) of (in_scale[w] * X[w, c]), v = nodes[i] (``nodes`` None: every
        node).  X is a float array [n_node, n_col], n_col <= 128; a scale of None means no multiply.  fp32: one rounded multiply per
        gathered element, adds, one rounded multiply at the end, no fused multiply-add.  The order of a node's adds is not
        specified, but the bits of its row depend on its neighbours, the gathered values and n_col alone: a rerun, a permuted or
        repeated ``nodes`` and a subset return the same bits per node.  No embedding table is read.
        Returns dict(out fp32 [m, n_col], ms)."""
        fn = "neighbor_sum"
        X_a = np.ascontiguousarray(X, dtype=np.float32)
        if X_a.ndim != 2 or X_a.shape[0] != self.n_node:
            raise ValueError("%s: X must be a float matrix [%d, n_col], got shape %r" % (fn, self.n_node, X_a.shape))
        n_col = int(X_a.shape[1])
        if not 1 <= n_col <= _lib.NEIGHBOR_SUM_MAX_COL:
            raise ValueError("%s: n_col = %d outside [1, %d]" % (fn, n_col, _lib.NEIGHBOR_SUM_MAX_COL))
        in_a, os_a = self._gp_scale(fn, "in_scale", in_scale), self._gp_scale(fn, "out_scale", out_scale)
        nodes_a = None if nodes is None else _i32(_lprop.check_nodes(fn, "nodes", nodes, self.n_node))
        m = self.n_node if nodes_a is None else len(nodes_a)
        out = np.empty((m, n_col), dtype=np.float32)
        ms = ctypes.c_double()
        if m:
            self._ck(lib.gg_neighbor_sum(self._ctx, _ptr(X_a), n_col, _ptr(in_a), _ptr(os_a), _ptr(nodes_a), m, _ptr(out), ctypes.byref(ms)))
        return dict(out=out, ms=ms.value)

    def label_spread(self, train_nodes, labels, n_class, alpha=0.9, iters=30, out_nodes=None):
        """Label spreading on the resident training graph (gg_label_spread; evaluation/label_propagation.py): F_0 = Y0,
        F_{t+1} = alpha S F_t + (1 - alpha) Y0 with S = D^-1/2 A D^-1/2 on the neighbour sets, ``iters`` iterations on the device.
        ``labels``: an int array [m_train] (single label), a bool / 0-1 matrix [m_train, n_class] or a list of label lists
        (multi-label); ``train_nodes`` distinct.  The coefficients are ``label_propagation.spread_coefficients`` of
        ``distinct_degrees()``.  ``iters = T`` equals T ``neighbor_sum(F, in_scale=s)`` calls composed with float32 a * H + base, bit
        for bit.  Returns dict(F fp32 [m_out, n_class] -- the rows of ``out_nodes``, None: every node --, delta = max |F_T - F_{T-1}|
        over all nodes, ms)."""
        fn = "label_spread"
        if isinstance(n_class, bool) or int(n_class) != n_class or not 1 <= int(n_class) <= _lib.NEIGHBOR_SUM_MAX_COL:
            raise ValueError("%s: n_class = %r outside [1, %d]" % (fn, n_class, _lib.NEIGHBOR_SUM_MAX_COL))
        C = int(n_class)
        _lprop.check_alpha_iters(fn, alpha, iters)
        tr = _i32(_lprop.check_nodes(fn, "train_nodes", train_nodes, self.n_node, distinct=True))
        bits = pack_label_bits(_lprop.label_matrix(fn, labels, len(tr), C), C)
        out_a = None if out_nodes is None else _i32(_lprop.check_nodes(fn, "out_nodes", out_nodes, self.n_node))
        s, a, _ = _lprop.spread_coefficients(self.distinct_degrees(), alpha)
        m_out = self.n_node if out_a is None else len(out_a)
        F = np.empty((m_out, C), dtype=np.float32)
        delta, ms = ctypes.c_float(), ctypes.c_double()
        self._ck(lib.gg_label_spread(self._ctx, _ptr(tr), _ptr(bits), len(tr), C, float(alpha), int(iters), _ptr(s), _ptr(a), _ptr(out_a), m_out,
                                     _ptr(F), ctypes.byref(delta), ctypes.byref(ms)))
        return dict(F=F, delta=float(delta.value), ms=ms.value)

    NEIGHBOR_MODE_LDS_CAP = _lib.NEIGHBOR_MODE_LDS_CAP  # neighbours of a node the neighbour-mode sweep counts in an LDS table (a longer list: a table in global memory)
    PARTITION_EDGES_CHUNK = _lib.PARTITION_EDGES_CHUNK  # neighbours of a node per task of partition_edges (a node with more is split)

    def neighbor_mode(self, labels, salt=0, keep=True, nodes=None):
        """The neighbour-mode sweep (gg_neighbor_mode) on the neighbour SETS N(v) of the resident training graph (those of
        ``pair_neighbors``): for v = nodes[i] (``nodes`` None: every node) the most frequent label among labels[w], w in N(v).  A
        node without neighbours keeps its label; with ``keep`` so does a node whose own label is among the most frequent;
        otherwise ties go to the label with the smallest pair (fmix32(l ^ salt), l) (evaluation/graph_communities.py).  ``labels``:
        an int array [n_node], every label >= 0.  All integer: a rerun, a permuted or repeated ``nodes`` and a subset return the
        same value per node.  No embedding table is read.  Returns dict(out int32 [m], ms)."""
        fn = "neighbor_mode"
        lab = _gcomm.check_labels(fn, labels, self.n_node)
        nodes_a = None if nodes is None else _i32(_lprop.check_nodes(fn, "nodes", nodes, self.n_node))
        m = self.n_node if nodes_a is None else len(nodes_a)
        out = np.empty(m, dtype=np.int32)
        ms = ctypes.c_double()
        if m:
            self._ck(lib.gg_neighbor_mode(self._ctx, _ptr(lab), int(salt) & 0xFFFFFFFF, int(bool(keep)), _ptr(nodes_a), m, _ptr(out), ctypes.byref(ms)))
        return dict(out=out, ms=ms.value)

    def label_propagation(self, seed=0, max_iters=100):
        """Label-propagation community detection on the resident training graph (gg_label_propagation;
        evaluation/graph_communities.py): from L[v] = v, every iteration redraws a split of the nodes into two sides and lets
        first one side, then the other take ``neighbor_mode(L, keep=True)`` at once; it stops at the first iteration that moves
        no label or after ``max_iters``.  Labels, the side test and the counters stay on the device; ``T`` iterations equal 2 T
        ``neighbor_mode`` calls composed on the host, bit for bit.  Returns dict(labels int32 [n_node], iters, converged, changed
        int64 [iters] -- the labels each iteration moved --, ms)."""
        fn = "label_propagation"
        _gcomm.check_max_iters(fn, max_iters)
        labels = np.empty(self.n_node, dtype=np.int32)
        changed = np.zeros(int(max_iters), dtype=np.int32)
        iters, converged, ms = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        self._ck(lib.gg_label_propagation(self._ctx, int(seed) & 0xFFFFFFFF, int(max_iters), _ptr(labels), ctypes.byref(iters), ctypes.byref(converged),
                                          _ptr(changed), ctypes.byref(ms)))
        return dict(labels=labels, iters=int(iters.value), converged=bool(converged.value), changed=changed[:iters.value].astype(np.int64), ms=ms.value)

    def partition_edges(self, assign, n_label):
        """The edge counts of a partition of the resident training graph (gg_partition_edges): ``assign`` an int array [n_node]
        with a class in [0, n_label) or -1 for "outside the partition"; tot[c] = the ordered pairs (v, w), w in N(v), with v in
        class c and w inside the partition, intra[c] those with w in class c too.  Exact integers.  Returns dict(intra int64
        [n_label], tot int64 [n_label], ms)."""
        a = _gcomm.check_assign("partition_edges", assign, self.n_node, n_label)
        intra, tot = np.zeros(int(n_label), dtype=np.int64), np.zeros(int(n_label), dtype=np.int64)
        ms = ctypes.c_double()
        self._ck(lib.gg_partition_edges(self._ctx, _ptr(a), int(n_label), _ptr(intra), _ptr(tot), ctypes.byref(ms)))
        return dict(intra=intra, tot=tot, ms=ms.value)

    def modularity(self, assign):
        """Newman's modularity Q of the partition ``assign`` (classes >= 0, -1: outside; the subgraph the inside nodes induce) on
        the neighbour sets of the resident training graph: ``graph_communities.modularity_from_counts`` of ``partition_edges``;
        nan where no edge lies inside."""
        a = np.asarray(assign)
        n_label = max(int(a.max()) + 1, 1) if a.size and np.issubdtype(a.dtype, np.integer) else 1
        res = self.partition_edges(_gcomm.check_assign("modularity", a, self.n_node, n_label), n_label)
        return _gcomm.modularity_from_counts(res["intra"], res["tot"])

    def undirected_edges(self):
        """The undirected edge list of the resident training graph (gg_undirected_edges): E = {(a, b) : a < b, b in N(a)} over
        the neighbour SETS (those of ``pair_neighbors``: no duplicate, no self-loop), ordered by (a, b): int32 [m, 2].  Built once
        per graph; ``set_graph_csr`` drops it."""
        m = ctypes.c_int64()
        self._ck(lib.gg_undirected_edges(self._ctx, ctypes.byref(m), None))
        edges = np.empty((int(m.value), 2), dtype=np.int32)
        if m.value:
            self._ck(lib.gg_undirected_edges(self._ctx, ctypes.byref(m), _ptr(edges)))
        return edges

    def spanning_forest(self, seed=0, priority=None, sweeps=False):
        """The minimum spanning forest of the resident training graph and its connected components (gg_spanning_forest): Boruvka
        rounds on the device over ``undirected_edges()``.  Edge j has the key (priority[j] << 32) | j; ``priority``: an integer array
        [m] with values in [0, 2^32), or None for fmix32(j ^ fmix32(seed ^ 0x53504C54)) (split.default_priorities).  Keys are
        distinct, so the forest is unique: forest[j] = 1 exactly when Kruskal in ascending key order takes edge j, whatever the
        grid or the run.  component[v] = the smallest node id of v's component.  Returns dict(forest uint8 [m], component int32
        [n_node], m, n_forest, n_components (isolated nodes count), rounds, ms); with ``sweeps`` also sweep_live / sweep_hooks
        int64 and sweep_ms float64, one entry per edge sweep (the rounds and the last sweep, which hooks nothing)."""
        fn = "spanning_forest"
        m = ctypes.c_int64()
        self._ck(lib.gg_undirected_edges(self._ctx, ctypes.byref(m), None))
        m = int(m.value)
        prio = None
        if priority is not None:
            prio = np.asarray(priority)
            if prio.shape != (m,) or prio.dtype.kind not in "iu":
                raise ValueError("%s: priority must be a uint32 array [%d]" % (fn, m))
            if m and (int(prio.min()) < 0 or int(prio.max()) > 0xFFFFFFFF):
                raise ValueError("%s: priority must be a uint32 array [%d]: a value outside [0, 2^32)" % (fn, m))
            prio = np.ascontiguousarray(prio, dtype=np.uint32)
        forest = np.zeros(m, dtype=np.uint8)
        component = np.empty(self.n_node, dtype=np.int32)
        stats = np.zeros(4, dtype=np.int64)
        cnt = np.full((_lib.SF_MAX_SWEEPS, 2), -1, dtype=np.int64) if sweeps else None
        sms = np.full(_lib.SF_MAX_SWEEPS, -1.0, dtype=np.float64) if sweeps else None
        ms = ctypes.c_double()
        self._ck(lib.gg_spanning_forest(self._ctx, int(seed) & 0xFFFFFFFF, _ptr(prio), m, _ptr(forest), _ptr(component), _ptr(stats), _ptr(cnt), _ptr(sms),
                                        ctypes.byref(ms)))
        res = dict(forest=forest, component=component, m=int(stats[0]), n_forest=int(stats[1]), n_components=int(stats[2]), rounds=int(stats[3]), ms=ms.value)
        if sweeps:
            k = int((cnt[:, 0] >= 0).sum())
            res.update(sweep_live=cnt[:k, 0].copy(), sweep_hooks=cnt[:k, 1].copy(), sweep_ms=sms[:k].copy())
        return res

    def connected_components(self):
        """component[v] = the smallest node id of v's connected component in the resident training graph (an isolated node is its
        own component): the ``component`` output of ``spanning_forest(seed=0)``, int32 [n_node]."""
        return self.spanning_forest(seed=0)["component"]

    TWO_HOP_LDS_CAP = _lib.TWO_HOP_LDS_CAP  # expansion entries of a query the two-hop sweep accumulates in an LDS table (more: a table in global memory)

    def _two_hop_args(self, fn, weights, exclude, scratch_bytes):
        return _grank.check_weights(fn, weights, self.n_node), _grank.check_exclude(fn, exclude), _grank.check_scratch(fn, scratch_bytes)

    def two_hop_topk(self, rows, k=10, weights=None, exclude=True, scratch_bytes=None):
        """The two-hop sweep's lists (gg_two_hop_topk; evaluation/graph_ranking.py): for each query node rows[i] the first ``k``
        (<= 256) eligible candidates c with S(u, c) > 0, S(u, c) = sum over w in N(u) & N(c) of weights[w] on the neighbour SETS
        of the resident training graph (those of ``pair_neighbors``: S is its ``cn`` / ``wsum``), score descending, column
        ascending.  ``weights``: None (every weight 1: common neighbours) or [n_node] non-negative integers, summed as unsigned
        64-bit integers (max(weights) * max(deg) must fit in 63 bits).  ``exclude``: True -- without u and its training
        neighbours, the candidates of ``topk(exclude=True)`` -- or "self" -- without u alone; False is refused.  ``scratch_bytes``:
        the cap on the global-memory tables of one internal pass (None: the default); results do not depend on it.  All integer: a
        rerun and permuted, repeated or subset queries return the same bits per query.  No embedding table is read.
        Returns dict(col int32 [m, k] padded with -1, score uint64 [m, k] padded with 0, n_pos int32 [m] = the eligible candidates
        with S > 0, which may exceed k, ms)."""
        fn = "two_hop_topk"
        w, code, scratch = self._two_hop_args(fn, weights, exclude, scratch_bytes)
        k = _grank.check_k(fn, k)
        rows_a = _i32(_grank.check_ids(fn, "rows", rows, self.n_node))
        m = len(rows_a)
        col = np.full((m, k), -1, dtype=np.int32)
        score = np.zeros((m, k), dtype=np.uint64)
        n_pos = np.zeros(m, dtype=np.int32)
        ms = ctypes.c_double()
        if m:
            self._ck(lib.gg_two_hop_topk(self._ctx, _ptr(rows_a), m, k, _ptr(w), code, scratch, _ptr(col), _ptr(score), _ptr(n_pos), ctypes.byref(ms)))
        return dict(col=col, score=score, n_pos=n_pos, ms=ms.value)

    def two_hop_rank(self, u, v, weights=None, exclude=True, scratch_bytes=None):
        """The two-hop sweep's ranks (gg_two_hop_rank; evaluation/graph_ranking.py): for each query (u[i], v[i]) the position of
        v in ``two_hop_topk``'s order of row u over ALL candidates -- the eligible nodes and always the target itself, the
        contract of ``rank``.  The device counts, over the eligible c != v with S(u, c) > 0, n_pos (all of them), ahead (those
        before v in the order) and pos_below (those with c < v); ``graph_ranking.full_rank`` places a zero-score target among
        the zero-score nodes without visiting them.  With an eligible target and score > 0, rank <= k holds exactly when
        ``two_hop_topk`` lists v at position rank - 1.  Returns dict(rank int64 [m] (1 = best), n_cand int64 [m], score uint64 [m]
        = S(u, v), ahead int32 [m], n_pos int32 [m], pos_below int32 [m], ms)."""
        fn = "two_hop_rank"
        w, code, scratch = self._two_hop_args(fn, weights, exclude, scratch_bytes)
        u_a, v_a = _i32(_grank.check_ids(fn, "u", u, self.n_node)), _i32(_grank.check_ids(fn, "v", v, self.n_node))
        if len(u_a) != len(v_a):
            raise ValueError("%s: u and v must have the same length, got %d and %d" % (fn, len(u_a), len(v_a)))
        m = len(u_a)
        score = np.zeros(m, dtype=np.uint64)
        ahead, n_pos, pos_below = (np.zeros(m, dtype=np.int32) for _ in range(3))
        ms = ctypes.c_double()
        if m:
            self._ck(lib.gg_two_hop_rank(self._ctx, _ptr(u_a), _ptr(v_a), m, _ptr(w), code, scratch, _ptr(score), _ptr(ahead), _ptr(n_pos), _ptr(pos_below),
                                         ctypes.byref(ms)))
        else:
            return dict(rank=np.zeros(0, dtype=np.int64), n_cand=np.zeros(0, dtype=np.int64), score=score, ahead=ahead, n_pos=n_pos, pos_below=pos_below, ms=0.0)
        if self._set_adj is None:
            self._set_adj = _lheur.csr_set_adjacency(self._rowptr, self._col)
        rank, n_cand = _grank.full_rank(self._set_adj[0], self._set_adj[1], u_a, v_a, code, score, ahead, n_pos, pos_below)
        return dict(rank=rank, n_cand=n_cand, score=score, ahead=ahead, n_pos=n_pos, pos_below=pos_below, ms=ms.value)

    TWO_HOP_TOP_PAIRS_MAX_K = 1 << 20  # the limit of gg_two_hop_top_pairs

    def two_hop_top_pairs(self, k, nodes=None, weights=None, exclude=True, scratch_bytes=None, buffer_entries=None):
        """The two-hop pair sweep (gg_two_hop_top_pairs; evaluation/graph_pairs.py): the ``k`` (<= 2^20) best unordered pairs
        {u, v}, u < v, of ``nodes`` (None: every node; else node ids, strictly ascending) under S(u, v) = sum over w in N(u) & N(v)
        of weights[w] on the neighbour SETS of the resident training graph -- the ``cn`` / ``wsum`` of ``pair_neighbors``, the
        score of ``two_hop_rank``; w ranges over the whole graph, only the endpoints are restricted by ``nodes`` -- with S > 0
        and, with ``exclude`` True, without the pairs that are training edges (False keeps them: u < v rules out the self pair).
        Order: score descending, then (u, v) ascending.  ``weights``: None (every weight 1) or [n_node] non-negative integers,
        summed as unsigned 64-bit integers (max(weights) * max(deg) must fit in 63 bits).  ``scratch_bytes``: the cap on the
        global-memory tables of one internal pass; ``buffer_entries``: the device buffer's entries, at least k + the most entries
        one source can append (the refusal names the minimum); None: the defaults.  Neither changes an output but ``stats``.  All
        integer: the graph-only line beside ``top_pairs``; no embedding table is read.  Returns dict(u int32 [k], v int32 [k],
        score uint64 [k] (-1, -1, 0 behind n_found), n_found = min(k, candidates), stats = dict(launches, retries, compactions,
        appended, swept, skipped), ms)."""
        fn = "two_hop_top_pairs"
        w, scratch = _grank.check_weights(fn, weights, self.n_node), _grank.check_scratch(fn, scratch_bytes)
        k = _grank.check_pair_k(fn, k)
        if not isinstance(exclude, (bool, np.bool_)):
            raise ValueError("%s: exclude must be True or False, got %r" % (fn, exclude))
        if buffer_entries is not None and (isinstance(buffer_entries, (bool, np.bool_)) or not isinstance(buffer_entries, (int, np.integer))
                                           or int(buffer_entries) < 1):
            raise ValueError("%s: buffer_entries must be None or a positive integer, got %r" % (fn, buffer_entries))
        nodes_a = None if nodes is None else _i32(_grank.check_ascending_ids(fn, "nodes", nodes, self.n_node))
        m = 0 if nodes_a is None else len(nodes_a)
        if nodes_a is not None and m == 0:
            nodes_a = np.zeros(1, dtype=np.int32)  # (an empty set still needs a pointer: NULL means "every node")
        u = np.empty(k, dtype=np.int32)
        v = np.empty(k, dtype=np.int32)
        score = np.empty(k, dtype=np.uint64)
        n_found = ctypes.c_int64()
        stats = np.zeros(6, dtype=np.int64)
        ms = ctypes.c_double()
        self._ck(lib.gg_two_hop_top_pairs(self._ctx, _ptr(nodes_a), m, k, _ptr(w), int(bool(exclude)), scratch, 0 if buffer_entries is None else int(buffer_entries),
                                          _ptr(u), _ptr(v), _ptr(score), ctypes.byref(n_found), _ptr(stats), ctypes.byref(ms)))
        return dict(u=u, v=v, score=score, n_found=int(n_found.value),
                    stats=dict(launches=int(stats[0]), retries=int(stats[1]), compactions=int(stats[2]), appended=int(stats[3]), swept=int(stats[4]),
                               skipped=int(stats[5])), ms=ms.value)

    PPR_LDS_CAP = _lib.PPR_LDS_CAP  # touched nodes E = min(n_node, 1 + 2^40 / kmin) up to which the push sweep keeps its tables in LDS (more: global memory)

    def _ppr_args(self, fn, alpha, eps, max_rounds, exclude, scratch_bytes):
        alpha_q, eps_q = _gppr.quantise(alpha, eps)
        return alpha_q, eps_q, _gppr.check_max_rounds(fn, max_rounds), _grank.check_exclude(fn, exclude), _grank.check_scratch(fn, scratch_bytes)

    def ppr_topk(self, rows, k=10, alpha=0.15, eps=1e-4, max_rounds=200, exclude=True, scratch_bytes=None):
        """The push sweep's lists (gg_ppr_topk; evaluation/graph_ppr.py): for each query node rows[i] the first ``k`` (<= 256)
        eligible candidates c with p[c] > 0, p the rooted PageRank of rows[i] on the neighbour SETS of the resident training graph
        by the synchronous local push in fixed-point integers (2^40 = all the mass), score descending, column ascending.
        ``alpha``: the restart probability, ``eps``: the push threshold per unit of degree, both quantised by
        ``graph_ppr.quantise``; ``max_rounds``: the rounds of a query at most.  ``exclude`` and ``scratch_bytes`` as
        ``two_hop_topk``'s.  All integer: a rerun and permuted, repeated or subset queries return the same bits per query.
        Returns dict(col int32 [m, k] padded with -1, score uint64 [m, k] padded with 0, n_pos int32 [m], rounds int32 [m] = the
        rounds that pushed, converged int32 [m], residual uint64 [m] = the mass not yet pushed, ms)."""
        fn = "ppr_topk"
        alpha_q, eps_q, max_rounds, code, scratch = self._ppr_args(fn, alpha, eps, max_rounds, exclude, scratch_bytes)
        k = _grank.check_k(fn, k)
        rows_a = _i32(_grank.check_ids(fn, "rows", rows, self.n_node))
        m = len(rows_a)
        col = np.full((m, k), -1, dtype=np.int32)
        score = np.zeros((m, k), dtype=np.uint64)
        n_pos, rounds, converged = (np.zeros(m, dtype=np.int32) for _ in range(3))
        residual = np.zeros(m, dtype=np.uint64)
        ms = ctypes.c_double()
        if m:
            self._ck(lib.gg_ppr_topk(self._ctx, _ptr(rows_a), m, k, alpha_q, eps_q, max_rounds, code, scratch, _ptr(col), _ptr(score), _ptr(n_pos), _ptr(rounds),
                                     _ptr(converged), _ptr(residual), ctypes.byref(ms)))
        return dict(col=col, score=score, n_pos=n_pos, rounds=rounds, converged=converged, residual=residual, ms=ms.value)

    def ppr_rank(self, u, v, alpha=0.15, eps=1e-4, max_rounds=200, exclude=True, scratch_bytes=None):
        """The push sweep's ranks (gg_ppr_rank; evaluation/graph_ppr.py): for each query (u[i], v[i]) the position of v in
        ``ppr_topk``'s order of root u over ALL candidates, the contract of ``two_hop_rank`` with S = p.  Queries with equal u that
        stand next to each other share one push (sort by u to use it); a query's outputs depend on its own (u, v) alone.
        Returns dict(rank int64 [m] (1 = best), n_cand int64 [m], score uint64 [m] = p[v], ahead, n_pos, pos_below int32 [m],
        rounds, converged int32 [m], residual uint64 [m], ms)."""
        fn = "ppr_rank"
        alpha_q, eps_q, max_rounds, code, scratch = self._ppr_args(fn, alpha, eps, max_rounds, exclude, scratch_bytes)
        u_a, v_a = _i32(_grank.check_ids(fn, "u", u, self.n_node)), _i32(_grank.check_ids(fn, "v", v, self.n_node))
        if len(u_a) != len(v_a):
            raise ValueError("%s: u and v must have the same length, got %d and %d" % (fn, len(u_a), len(v_a)))
        m = len(u_a)
        score, residual = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        ahead, n_pos, pos_below, rounds, converged = (np.zeros(m, dtype=np.int32) for _ in range(5))
        out = dict(score=score, ahead=ahead, n_pos=n_pos, pos_below=pos_below, rounds=rounds, converged=converged, residual=residual)
        if not m:
            return dict(rank=np.zeros(0, dtype=np.int64), n_cand=np.zeros(0, dtype=np.int64), ms=0.0, **out)
        ms = ctypes.c_double()
        self._ck(lib.gg_ppr_rank(self._ctx, _ptr(u_a), _ptr(v_a), m, alpha_q, eps_q, max_rounds, code, scratch, _ptr(score), _ptr(ahead), _ptr(n_pos),
                                 _ptr(pos_below), _ptr(rounds), _ptr(converged), _ptr(residual), ctypes.byref(ms)))
        if self._set_adj is None:
            self._set_adj = _lheur.csr_set_adjacency(self._rowptr, self._col)
        rank, n_cand = _grank.full_rank(self._set_adj[0], self._set_adj[1], u_a, v_a, code, score, ahead, n_pos, pos_below)
        return dict(rank=rank, n_cand=n_cand, ms=ms.value, **out)

    def graph_softmax(self, slots, for_d=False, nodes=None, q3_store=False):
        """The generator's distribution G(v | root) of the tree in each slot, exactly (gg_graph_softmax): the law of the end node
        of one walk of ``walk_sample`` on the same slot and mode (graph_gan.py:225-270).  Log-probabilities in fp32, -inf where
        P = 0 (the root, unreached nodes, dropped fathers).  ``q3_store``: the Q3 bits of the root-batched epochs' store
        instead of the slots' own.  Returns (logp fp32 [n_slots, N], abort fp32 [n_slots]) -- abort = the mass of walks that
        end in ``return None, None`` -- or, with ``nodes`` (one array per slot, or a tuple (flat node ids, offsets
        [n_slots + 1])), (q_logp fp32, abort) with q_logp of the queried nodes (flat, in slot order; per-slot lists: a list of
        arrays).  The whole trees must be resident (set_tree_mode(0)); time of the sweeps in ``last_graph_softmax_ms``."""
        slots_a = np.asarray(slots)
        if slots_a.ndim != 1 or (slots_a.size and not np.issubdtype(slots_a.dtype, np.integer)):
            raise ValueError("graph_softmax: slots must be a 1-d array of integers")
        slots_a = _i32(slots_a)
        R = len(self.tree_roots)
        if slots_a.size and (int(slots_a.min()) < 0 or int(slots_a.max()) >= R):
            raise ValueError("graph_softmax: slot outside [0, %d)" % R)
        ns = len(slots_a)
        flags = (_lib.GG_GS_FOR_D if for_d else 0) | (_lib.GG_GS_Q3_STORE if q3_store else 0)
        abort = np.zeros(ns, dtype=np.float32)
        ms = ctypes.c_double()
        if nodes is None:
            logp = np.empty((ns, self.n_node), dtype=np.float32)
            self._ck(lib.gg_graph_softmax(self._ctx, _ptr(slots_a), ns, flags, _ptr(logp), None, None, None, _ptr(abort), ctypes.byref(ms)))
            self.last_graph_softmax_ms = ms.value
            return logp, abort
        per_slot = isinstance(nodes, list)
        if per_slot:
            if len(nodes) != ns:
                raise ValueError("graph_softmax: %d node lists for %d slots" % (len(nodes), ns))
            lists = [np.asarray(x).reshape(-1) for x in nodes]
            off = np.zeros(ns + 1, dtype=np.int64)
            np.cumsum([len(x) for x in lists], out=off[1:])
            flat = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        else:
            if not (isinstance(nodes, tuple) and len(nodes) == 2):
                raise ValueError("graph_softmax: nodes must be a list of per-slot arrays or a tuple (flat node ids, offsets)")
            flat, off = np.asarray(nodes[0]).reshape(-1), np.asarray(nodes[1]).reshape(-1)
            if len(off) != ns + 1 or (len(off) and (off[0] != 0 or off[-1] != len(flat) or np.any(np.diff(off) < 0))):
                raise ValueError("graph_softmax: offsets must be [n_slots + 1], monotone, from 0 to len(nodes)")
            off = np.ascontiguousarray(off, dtype=np.int64)
        if flat.size and (not np.issubdtype(flat.dtype, np.integer) or int(flat.min()) < 0 or int(flat.max()) >= self.n_node):
            raise ValueError("graph_softmax: node id outside [0, %d)" % self.n_node)
        flat = _i32(flat)
        q = np.empty(len(flat), dtype=np.float32)
        self._ck(lib.gg_graph_softmax(self._ctx, _ptr(slots_a), ns, flags, None, _ptr(off), _ptr(flat), _ptr(q), _ptr(abort), ctypes.byref(ms)))
        self.last_graph_softmax_ms = ms.value
        if per_slot:
            return [q[off[k]:off[k + 1]] for k in range(ns)], abort
        return q, abort

    # ------------------------------------------------------------------ node classification (gg_classifier_*)
    def _nc_args(self, fn, nodes, which, n_class, labels=None):
        if which not in (0, 1):
            raise ValueError("%s: which must be 0 (generator) or 1 (discriminator), got %r" % (fn, which))
        if isinstance(n_class, bool) or int(n_class) != n_class or not 2 <= int(n_class) <= 128:
            raise ValueError("%s: n_class must be an integer in [2, 128], got %r" % (fn, n_class))
        nodes_a = np.asarray(nodes)
        if nodes_a.ndim != 1 or nodes_a.size == 0 or not np.issubdtype(nodes_a.dtype, np.integer):
            raise ValueError("%s: nodes must be a non-empty 1-d array of integers" % fn)
        if int(nodes_a.min()) < 0 or int(nodes_a.max()) >= self.n_node:
            raise ValueError("%s: node id outside [0, %d)" % (fn, self.n_node))
        if labels is None:
            return _i32(nodes_a), None
        labels_a = np.asarray(labels)
        if labels_a.shape != nodes_a.shape or not np.issubdtype(labels_a.dtype, np.integer):
            raise ValueError("%s: labels must be integers, one per node" % fn)
        if int(labels_a.min()) < 0 or int(labels_a.max()) >= int(n_class):
            raise ValueError("%s: label outside [0, n_class = %d)" % (fn, int(n_class)))
        return _i32(nodes_a), _i32(labels_a)

    def _nc_params(self, fn, W, b):
        W = np.ascontiguousarray(W, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if W.ndim != 2 or W.shape[1] != self.n_emb or b.shape != (W.shape[0],):
            raise ValueError("%s: W must be [n_class, %d] and b [n_class], got %r and %r" % (fn, self.n_emb, W.shape, b.shape))
        return W, b

    def _nc_lossgrad(self, cfunc, nodes_a, labels_dev, which, l2, W, b):
        """the loss-and-gradient call of either label form: ``labels_dev`` is what ``cfunc`` reads (int32 classes or mask words)"""
        loss = np.zeros(1, dtype=np.float32)
        gW = np.empty_like(W)
        gb = np.empty_like(b)
        self._ck(cfunc(self._ctx, which, _ptr(nodes_a), _ptr(labels_dev), len(nodes_a), int(W.shape[0]), _ptr(W), _ptr(b), float(l2),
                       _ptr(loss), _ptr(gW), _ptr(gb)))
        return dict(loss=float(loss[0]), gW=gW, gb=gb)

    def _nc_fit(self, fn, cfunc, nodes_a, labels_dev, n_class, which, iters, lr, l2, W, b):
        """the fit call of either label form (``fn``: the public method, for the error texts; ``labels_dev`` as in _nc_lossgrad)"""
        C = int(n_class)
        if isinstance(iters, bool) or int(iters) != iters or int(iters) < 1:
            raise ValueError("%s: iters must be an integer >= 1, got %r" % (fn, iters))
        if not (np.isfinite(lr) and lr > 0) or not (np.isfinite(l2) and l2 >= 0):
            raise ValueError("%s: lr must be > 0 and l2 >= 0, got %r and %r" % (fn, lr, l2))
        if (W is None) != (b is None):
            raise ValueError("%s: give both W and b, or neither" % fn)
        if W is None:
            W, b = np.zeros((C, self.n_emb), dtype=np.float32), np.zeros(C, dtype=np.float32)
        else:
            W, b = self._nc_params(fn, W, b)
            if W.shape[0] != C:
                raise ValueError("%s: W has %d rows, n_class is %d" % (fn, W.shape[0], C))
            W, b = W.copy(), b.copy()
        loss = np.empty(int(iters), dtype=np.float32)
        ms = ctypes.c_double()
        self._ck(cfunc(self._ctx, which, _ptr(nodes_a), _ptr(labels_dev), len(nodes_a), C, int(iters), float(lr), float(l2),
                       _ptr(W), _ptr(b), _ptr(loss), ctypes.byref(ms)))
        return dict(W=W, b=b, loss=loss, ms=ms.value)

    def classifier_lossgrad(self, nodes, labels, W, b, which=0, l2=0.0):
        """Loss and gradients of multinomial logistic regression on the rows ``nodes`` of table ``which`` (0 = gen, 1 = dis)
        at (W [C, n_emb], b [C]) (gg_classifier_lossgrad: one fused sweep on the device).  Returns dict(loss, gW, gb)."""
        W, b = self._nc_params("classifier_lossgrad", W, b)
        nodes_a, labels_a = self._nc_args("classifier_lossgrad", nodes, which, int(W.shape[0]), labels)
        return self._nc_lossgrad(lib.gg_classifier_lossgrad, nodes_a, labels_a, which, l2, W, b)

    def classifier_fit(self, nodes, labels, n_class, which=0, iters=200, lr=0.05, l2=1e-4, W=None, b=None):
        """``iters`` steps of full-batch Adam on the logistic-regression loss of the rows ``nodes`` of table ``which``
        (gg_classifier_fit), from zeros unless (W, b) are given; fit on the device, one synchronisation.  Returns
        dict(W fp32 [n_class, n_emb], b fp32 [n_class], loss fp32 [iters] -- the loss before each update --, ms)."""
        nodes_a, labels_a = self._nc_args("classifier_fit", nodes, which, n_class, labels)
        return self._nc_fit("classifier_fit", lib.gg_classifier_fit, nodes_a, labels_a, n_class, which, iters, lr, l2, W, b)

    def classifier_predict(self, nodes, W, b, which=0, logits=False):
        """argmax_c (W . E[node] + b)[c] of the rows ``nodes`` of table ``which``, ties to the lowest class
        (gg_classifier_predict).  Returns pred int32 [len(nodes)], or (pred, logits fp32 [len(nodes), C]) with ``logits``."""
        W, b = self._nc_params("classifier_predict", W, b)
        C = int(W.shape[0])
        nodes_a, _ = self._nc_args("classifier_predict", nodes, which, C)
        pred = np.empty(len(nodes_a), dtype=np.int32)
        z = np.empty((len(nodes_a), C), dtype=np.float32) if logits else None
        self._ck(lib.gg_classifier_predict(self._ctx, which, _ptr(nodes_a), len(nodes_a), C, _ptr(W), _ptr(b), _ptr(pred), _ptr(z)))
        return (pred, z) if logits else pred

    # ------------------------------------------------------------------ multi-label node classification (gg_classifier_ml_*)
    def _nc_label_bits(self, fn, labels, m, n_class):
        """labels as a bool / 0-1 matrix [m, C] or as packed uint32 [m, CW] -> packed uint32 [m, CW], no bit at a position >= C"""
        C, CW = int(n_class), (int(n_class) + 31) // 32
        a = np.asarray(labels)
        if a.ndim == 2 and a.shape == (m, CW) and a.dtype == np.uint32:
            if C % 32 and np.any(a[:, -1] >> np.uint32(C % 32)):
                row = int(np.flatnonzero(a[:, -1] >> np.uint32(C % 32))[0])
                raise ValueError("%s: label_bits row %d has a bit set at a position >= n_class = %d" % (fn, row, C))
            return np.ascontiguousarray(a)
        if a.ndim != 2 or a.shape != (m, C) or not (a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer)):
            raise ValueError("%s: labels must be a bool / 0-1 matrix [%d, %d] or packed uint32 [%d, %d], got %s %r"
                             % (fn, m, C, m, CW, a.dtype, a.shape))
        if a.dtype != np.bool_ and a.size and (int(a.min()) < 0 or int(a.max()) > 1):
            raise ValueError("%s: the label matrix must hold 0 and 1 only" % fn)
        return pack_label_bits(a, C)

    def classifier_ml_lossgrad(self, nodes, labels, W, b, which=0, l2=0.0):
        """Loss and gradients of one-vs-rest logistic regression (per-class sigmoid cross-entropy, every class normalised by the
        row count) on the rows ``nodes`` of table ``which`` at (W [C, n_emb], b [C]); ``labels`` is a bool / 0-1 matrix [m, C] or
        packed uint32 [m, ceil(C / 32)] (gg_classifier_ml_lossgrad: the fused sweep on the device).  Returns dict(loss, gW, gb)."""
        W, b = self._nc_params("classifier_ml_lossgrad", W, b)
        C = int(W.shape[0])
        nodes_a, _ = self._nc_args("classifier_ml_lossgrad", nodes, which, C)
        bits = self._nc_label_bits("classifier_ml_lossgrad", labels, len(nodes_a), C)
        return self._nc_lossgrad(lib.gg_classifier_ml_lossgrad, nodes_a, bits, which, l2, W, b)

    def classifier_ml_fit(self, nodes, labels, n_class, which=0, iters=200, lr=0.05, l2=1e-4, W=None, b=None):
        """``iters`` steps of full-batch Adam on the one-vs-rest loss of the rows ``nodes`` of table ``which``
        (gg_classifier_ml_fit), from zeros unless (W, b) are given; labels as in ``classifier_ml_lossgrad``.  Returns
        dict(W fp32 [n_class, n_emb], b fp32 [n_class], loss fp32 [iters] -- the loss before each update --, ms)."""
        nodes_a, _ = self._nc_args("classifier_ml_fit", nodes, which, n_class)
        bits = self._nc_label_bits("classifier_ml_fit", labels, len(nodes_a), n_class)
        return self._nc_fit("classifier_ml_fit", lib.gg_classifier_ml_fit, nodes_a, bits, n_class, which, iters, lr, l2, W, b)

    def classifier_ml_predict(self, nodes, W, b, which=0, k=None, logits=False):
        """The label sets of the rows ``nodes`` of table ``which`` under (W, b) (gg_classifier_ml_predict).  With ``k`` (one
        integer in [0, C] per row): the first k[i] classes of row i in the order (logit descending, class ascending); without:
        the classes whose logit is > 0.  Returns pred bool [len(nodes), C], or (pred, logits fp32 [len(nodes), C])."""
        W, b = self._nc_params("classifier_ml_predict", W, b)
        C = int(W.shape[0])
        nodes_a, _ = self._nc_args("classifier_ml_predict", nodes, which, C)
        k_a = None
        if k is not None:
            k_a = np.asarray(k)
            if k_a.shape != nodes_a.shape or not np.issubdtype(k_a.dtype, np.integer):
                raise ValueError("classifier_ml_predict: k must be integers, one per node")
            if int(k_a.min()) < 0 or int(k_a.max()) > C:
                raise ValueError("classifier_ml_predict: k outside [0, n_class = %d]" % C)
            k_a = _i32(k_a)
        bits = np.empty((len(nodes_a), (C + 31) // 32), dtype=np.uint32)
        z = np.empty((len(nodes_a), C), dtype=np.float32) if logits else None
        self._ck(lib.gg_classifier_ml_predict(self._ctx, which, _ptr(nodes_a), len(nodes_a), C, _ptr(W), _ptr(b), _ptr(k_a), _ptr(bits), _ptr(z)))
        pred = unpack_label_bits(bits, C)
        return (pred, z) if logits else pred

    # ------------------------------------------------------------------ learned link prediction (gg_edge_classifier_*)
    def _ec_args(self, fn, u, v, which, op, y=None):
        """-> (op number, u int32, v int32, y int32 or None), refused as the ABI refuses them"""
        if which not in (0, 1):
            raise ValueError("%s: which must be 0 (generator) or 1 (discriminator), got %r" % (fn, which))
        if isinstance(op, str):
            if op not in EDGE_OPERATORS:
                raise ValueError("%s: operator must be one of %s or a number in [0, 3], got %r" % (fn, ", ".join(EDGE_OPERATORS), op))
            op = EDGE_OPERATORS.index(op)
        elif isinstance(op, bool) or not isinstance(op, (int, np.integer)) or not 0 <= int(op) <= 3:
            raise ValueError("%s: operator must be one of %s or a number in [0, 3], got %r" % (fn, ", ".join(EDGE_OPERATORS), op))
        u_a, v_a = np.asarray(u), np.asarray(v)
        if u_a.ndim != 1 or u_a.size == 0 or u_a.shape != v_a.shape or not (np.issubdtype(u_a.dtype, np.integer) and np.issubdtype(v_a.dtype, np.integer)):
            raise ValueError("%s: u and v must be non-empty 1-d arrays of integers of one length" % fn)
        if min(int(u_a.min()), int(v_a.min())) < 0 or max(int(u_a.max()), int(v_a.max())) >= self.n_node:
            raise ValueError("%s: node id outside [0, %d)" % (fn, self.n_node))
        if y is None:
            return int(op), _i32(u_a), _i32(v_a), None
        y_a = np.asarray(y)
        if y_a.shape != u_a.shape or not (y_a.dtype == np.bool_ or np.issubdtype(y_a.dtype, np.integer)):
            raise ValueError("%s: y must be 0 / 1, one per edge" % fn)
        if y_a.dtype != np.bool_ and (int(y_a.min()) < 0 or int(y_a.max()) > 1):
            raise ValueError("%s: y must be 0 / 1, one per edge" % fn)
        return int(op), _i32(u_a), _i32(v_a), _i32(y_a.astype(np.int32))

    def _ec_params(self, fn, w, b):
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if w.shape != (self.n_emb,) or b.shape != (1,):
            raise ValueError("%s: w must be [%d] and b a scalar, got %r and %r" % (fn, self.n_emb, w.shape, b.shape))
        return w, b

    def edge_classifier_lossgrad(self, u, v, y, w, b, op="hadamard", which=0, l2=0.0):
        """Loss and gradients of logistic regression on x = op(E[u], E[v]) of the edges (u[i], v[i]) with labels y[i] in {0, 1},
        rows of table ``which`` (0 = gen, 1 = dis), at (w [n_emb], b scalar) (gg_edge_classifier_lossgrad: one sweep on the
        device).  ``op``: "hadamard", "average", "l1", "l2" or its number 0 .. 3.  Returns dict(loss, gw, gb)."""
        w, b = self._ec_params("edge_classifier_lossgrad", w, b)
        op, u_a, v_a, y_a = self._ec_args("edge_classifier_lossgrad", u, v, which, op, y)
        loss, gb = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
        gw = np.empty_like(w)
        self._ck(lib.gg_edge_classifier_lossgrad(self._ctx, which, op, _ptr(u_a), _ptr(v_a), _ptr(y_a), len(u_a), _ptr(w), _ptr(b), float(l2),
                                                 _ptr(loss), _ptr(gw), _ptr(gb)))
        return dict(loss=float(loss[0]), gw=gw, gb=float(gb[0]))

    def edge_classifier_fit(self, u, v, y, op="hadamard", which=0, iters=200, lr=0.05, l2=1e-4, w=None, b=None):
        """``iters`` steps of full-batch Adam on the loss of ``edge_classifier_lossgrad`` (gg_edge_classifier_fit), from zeros
        unless (w, b) are given; fit on the device, one synchronisation.  Returns dict(w fp32 [n_emb], b float, loss fp32 [iters]
        -- the loss before each update --, ms)."""
        fn = "edge_classifier_fit"
        op, u_a, v_a, y_a = self._ec_args(fn, u, v, which, op, y)
        if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= 1000000:
            raise ValueError("%s: iters must be an integer in [1, 10^6], got %r" % (fn, iters))
        if not (np.isfinite(lr) and lr > 0) or not (np.isfinite(l2) and l2 >= 0):
            raise ValueError("%s: lr must be > 0 and l2 >= 0, got %r and %r" % (fn, lr, l2))
        if (w is None) != (b is None):
            raise ValueError("%s: give both w and b, or neither" % fn)
        if w is None:
            w, b = np.zeros(self.n_emb, dtype=np.float32), np.zeros(1, dtype=np.float32)
        else:
            w, b = self._ec_params(fn, w, b)
            w, b = w.copy(), b.copy()
        loss = np.empty(int(iters), dtype=np.float32)
        ms = ctypes.c_double()
        self._ck(lib.gg_edge_classifier_fit(self._ctx, which, op, _ptr(u_a), _ptr(v_a), _ptr(y_a), len(u_a), int(iters), float(lr), float(l2),
                                            _ptr(w), _ptr(b), _ptr(loss), ctypes.byref(ms)))
        return dict(w=w, b=float(b[0]), loss=loss, ms=ms.value)

    def edge_classifier_predict(self, u, v, w, b, op="hadamard", which=0):
        """The logits w . op(E[u], E[v]) + b of the edges (u[i], v[i]) on table ``which`` (gg_edge_classifier_predict): fp32 [len(u)]."""
        w, b = self._ec_params("edge_classifier_predict", w, b)
        op, u_a, v_a, _ = self._ec_args("edge_classifier_predict", u, v, which, op)
        z = np.empty(len(u_a), dtype=np.float32)
        self._ck(lib.gg_edge_classifier_predict(self._ctx, which, op, _ptr(u_a), _ptr(v_a), len(u_a), _ptr(w), _ptr(b), _ptr(z)))
        return z

    # ------------------------------------------------------------------ node clustering (gg_kmeans_*)
    def _km_args(self, fn, nodes, which, k=None):
        """-> nodes int32, refused as the ABI refuses them"""
        if which not in (0, 1):
            raise ValueError("%s: which must be 0 (generator) or 1 (discriminator), got %r" % (fn, which))
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 128):
            raise ValueError("%s: k must be an integer in [1, 128], got %r" % (fn, k))
        nodes_a = np.asarray(nodes)
        if nodes_a.ndim != 1 or nodes_a.size == 0 or not np.issubdtype(nodes_a.dtype, np.integer):
            raise ValueError("%s: nodes must be a non-empty 1-d array of integers" % fn)
        if int(nodes_a.min()) < 0 or int(nodes_a.max()) >= self.n_node:
            raise ValueError("%s: node id outside [0, %d)" % (fn, self.n_node))
        return _i32(nodes_a)

    def _km_centroids(self, fn, name, values):
        """a float array [k, n_emb] -> (fp32 copy, None); an integer array of k node ids -> (None, int32)"""
        a = np.asarray(values)
        if np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_:
            if a.ndim != 1 or not 1 <= a.size <= 128:
                raise ValueError("%s: %s as node ids must be a 1-d array of 1 .. 128 integers, got shape %r" % (fn, name, a.shape))
            if int(a.min()) < 0 or int(a.max()) >= self.n_node:
                raise ValueError("%s: %s holds a node id outside [0, %d)" % (fn, name, self.n_node))
            return None, _i32(a)
        if not np.issubdtype(a.dtype, np.floating) or a.ndim != 2 or a.shape[1] != self.n_emb or not 1 <= a.shape[0] <= 128:
            raise ValueError("%s: %s must be floats [k, %d] with k in [1, 128] or k integer node ids, got %s %r" % (fn, name, self.n_emb, a.dtype, a.shape))
        return np.array(a, dtype=np.float32, order="C"), None

    def kmeans_step(self, nodes, centroids=None, centroid_nodes=None, which=0, sums=True):
        """ONE k-means sweep over the rows ``nodes`` of table ``which`` (gg_kmeans_step) at ``centroids`` (floats [k, n_emb]) or at
        the table rows ``centroid_nodes`` (k node ids; nothing but the ids goes to the device) -- exactly one of the two.
        Returns dict(assign int32 [m] -- ties to the lowest cluster --, dist2 fp32 [m], inertia float, and unless ``sums`` is
        False: sums fp32 [k, n_emb], counts int32 [k])."""
        fn = "kmeans_step"
        if (centroids is None) == (centroid_nodes is None):
            raise ValueError("%s: give exactly one of centroids and centroid_nodes" % fn)
        nodes_a = self._km_args(fn, nodes, which)
        if centroids is not None:
            cen, ids = self._km_centroids(fn, "centroids", np.asarray(centroids, dtype=np.float32))
        else:
            ids_a = np.asarray(centroid_nodes)
            if not np.issubdtype(ids_a.dtype, np.integer):
                raise ValueError("%s: centroid_nodes must be integer node ids" % fn)
            cen, ids = self._km_centroids(fn, "centroid_nodes", ids_a)
        k, m = int(len(cen) if cen is not None else len(ids)), len(nodes_a)
        assign, dist2 = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.float32)
        s = np.empty((k, self.n_emb), dtype=np.float32) if sums else None
        counts = np.empty(k, dtype=np.int32) if sums else None
        inertia = np.zeros(1, dtype=np.float64)
        self._ck(lib.gg_kmeans_step(self._ctx, which, _ptr(nodes_a), m, k, _ptr(cen), _ptr(ids), _ptr(assign), _ptr(dist2), _ptr(s), _ptr(counts),
                                    _ptr(inertia)))
        out = dict(assign=assign, dist2=dist2, inertia=float(inertia[0]))
        if sums:
            out.update(sums=s, counts=counts)
        return out

    def kmeans_fit(self, nodes, k=None, init=None, max_iters=100, which=0):
        """Lloyd's k-means on the rows ``nodes`` of table ``which`` (gg_kmeans_fit), fitted on the device with one
        synchronisation.  ``init``: floats [k, n_emb], or k node ids (the start is those table rows); ``k`` may be left out (it
        is ``len(init)``).  Stops at the first sweep (from the second on) that changes no assignment, or after ``max_iters``
        sweeps without a last update, so the returned state is consistent: ``kmeans_step`` at the returned centroids gives the
        returned assign, dist2, counts and last inertia bit for bit.  An empty cluster keeps its centroid.  Returns
        dict(centroids fp32 [k, n_emb], assign int32 [m], dist2 fp32 [m], counts int32 [k], inertia float64 [iters], iters,
        converged, ms)."""
        fn = "kmeans_fit"
        if init is None:
            raise ValueError("%s: init is required (floats [k, n_emb] or k node ids; Engine.kmeans_seed draws them)" % fn)
        nodes_a = self._km_args(fn, nodes, which, k)
        cen, ids = self._km_centroids(fn, "init", init)
        n_k = int(len(cen) if cen is not None else len(ids))
        if k is not None and int(k) != n_k:
            raise ValueError("%s: init has %d centroids, k is %d" % (fn, n_k, int(k)))
        if isinstance(max_iters, bool) or int(max_iters) != max_iters or not 1 <= int(max_iters) <= 1000000:
            raise ValueError("%s: max_iters must be an integer in [1, 10^6], got %r" % (fn, max_iters))
        T, m = int(max_iters), len(nodes_a)
        if cen is None:
            cen = np.zeros((n_k, self.n_emb), dtype=np.float32)
        assign, dist2 = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.float32)
        counts = np.empty(n_k, dtype=np.int32)
        inertia = np.zeros(T, dtype=np.float64)
        iters, conv, ms = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        self._ck(lib.gg_kmeans_fit(self._ctx, which, _ptr(nodes_a), m, n_k, T, _ptr(cen), _ptr(ids), _ptr(assign), _ptr(dist2), _ptr(counts),
                                   _ptr(inertia), ctypes.byref(iters), ctypes.byref(conv), ctypes.byref(ms)))
        return dict(centroids=cen, assign=assign, dist2=dist2, counts=counts, inertia=inertia[:iters.value].copy(), iters=int(iters.value),
                    converged=bool(conv.value), ms=ms.value)

    def kmeans_seed(self, nodes, k, seed, which=0):
        """k-means++ seeding driven from the host over device distances -> int64 [k] POSITIONS into ``nodes``.  The rule:
        rs = RandomState([seed, 0x4B4D]); the first centre is position rs.randint(m); for every further centre dist2 comes from
        ``kmeans_step(nodes, centroid_nodes=<the centres so far>)`` (m floats to the host, never m x n_emb), cum = its float64
        cumulative sum, r = rs.random_sample() * cum[-1], position = min(searchsorted(cum, r, side="right"), m - 1); where
        cum[-1] == 0 the position is rs.randint(m)."""
        nodes_a = self._km_args("kmeans_seed", nodes, which, k)
        step = lambda chosen: self.kmeans_step(nodes_a, centroid_nodes=nodes_a[chosen], which=which, sums=False)["dist2"]  # noqa: E731
        return kmeans_pp_positions(len(nodes_a), int(k), seed, step)

    # ------------------------------------------------------------------ silhouette of a partition (gg_silhouette)
    def silhouette(self, nodes, assign, k=None, rows=None, which=0, precision="fp32"):
        """The exact silhouette of the partition ``assign`` of the rows ``nodes`` of table ``which`` over ALL pairs (gg_silhouette;
        Euclidean distance, the definition in include/graphgan_hip.h), streamed on the device: nothing of size m x m exists.
        ``nodes``: 1-d integers, m >= 2 DISTINCT node ids; ``assign``: 1-d integers [m] in [0, k) with at least two non-empty
        clusters; ``k``: integer in [2, 128], None = max(assign) + 1; ``rows``: None (every position) or 1-d integers, positions
        into ``nodes`` (free to repeat), each evaluated against all m columns with the full call's bits; precision "fp32" or
        "bf16" (the silhouette of the bf16-rounded table).  Returns dict(sil fp32, a fp32, b fp32, nearest int32 -- each
        [len(rows) or m] --, mean float, ms)."""
        fn = "silhouette"
        if precision not in ("fp32", "bf16"):
            raise ValueError("%s: precision must be 'fp32' or 'bf16', got %r" % (fn, precision))
        if which not in (0, 1):
            raise ValueError("%s: which must be 0 (generator) or 1 (discriminator), got %r" % (fn, which))
        nodes_a, assign_a = np.asarray(nodes), np.asarray(assign)
        for name, arr in (("nodes", nodes_a), ("assign", assign_a)):
            if arr.ndim != 1 or not np.issubdtype(arr.dtype, np.integer) or arr.dtype == np.bool_:
                raise ValueError("%s: %s must be a 1-d array of integers" % (fn, name))
        m = len(nodes_a)
        if m < 2:
            raise ValueError("%s: m = %d outside [2, 2^31 - 1]" % (fn, m))
        if len(assign_a) != m:
            raise ValueError("%s: nodes and assign must have the same length, got %d and %d" % (fn, m, len(assign_a)))
        if k is None:
            k = int(assign_a.max()) + 1
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= 128:
            raise ValueError("%s: k must be an integer in [2, 128], got %r" % (fn, k))
        k = int(k)
        if int(nodes_a.min()) < 0 or int(nodes_a.max()) >= self.n_node:
            raise ValueError("%s: node id outside [0, %d)" % (fn, self.n_node))
        if int(assign_a.min()) < 0 or int(assign_a.max()) >= k:
            raise ValueError("%s: assign outside [0, k = %d)" % (fn, k))
        rows_a = None
        if rows is not None:
            rows_a = np.asarray(rows)
            if rows_a.ndim != 1 or rows_a.size == 0 or not np.issubdtype(rows_a.dtype, np.integer) or rows_a.dtype == np.bool_:
                raise ValueError("%s: rows must be None or a non-empty 1-d array of integers" % fn)
            if int(rows_a.min()) < 0 or int(rows_a.max()) >= m:
                raise ValueError("%s: rows outside [0, m = %d)" % (fn, m))
            rows_a = np.ascontiguousarray(rows_a, dtype=np.int64)
        n_out = m if rows_a is None else len(rows_a)
        nodes_a, assign_a = _i32(nodes_a), _i32(assign_a)
        sil, a, b = (np.empty(n_out, dtype=np.float32) for _ in range(3))
        nearest = np.empty(n_out, dtype=np.int32)
        mean = np.zeros(1, dtype=np.float64)
        ms = ctypes.c_double()
        self._ck(lib.gg_silhouette(self._ctx, which, _ptr(nodes_a), _ptr(assign_a), m, k, _ptr(rows_a), n_out if rows_a is not None else 0,
                                   {"fp32": 0, "bf16": 1}[precision], _ptr(sil), _ptr(a), _ptr(b), _ptr(nearest), _ptr(mean), ctypes.byref(ms)))
        return dict(sil=sil, a=a, b=b, nearest=nearest, mean=float(mean[0]), ms=ms.value)

    # ------------------------------------------------------------------ PCA of the rows (gg_gram)
    def gram(self, nodes, center=None, which=0, gram=True):
        """The centred Gram matrix of the rows ``nodes`` of table ``which`` (gg_gram): with c_i = E[node_i] - center in fp32
        (``center``: floats [n_emb], None = no subtraction) ``sums`` = sum_i c_i and ``gram`` = sum_i c_i c_i^T, fp32 chains per
        workgroup on the matrix cores, added in float64.  ``gram=False`` is the sums-only sweep (the mean pass; the same ``sums``
        bits).  Returns dict(sums float64 [n_emb], gram float64 [n_emb, n_emb] or None, ms)."""
        fn = "gram"
        nodes_a = self._km_args(fn, nodes, which)
        cen = None
        if center is not None:
            cen = np.ascontiguousarray(center, dtype=np.float32)
            if cen.shape != (self.n_emb,) or not np.all(np.isfinite(cen)):
                raise ValueError("%s: center must be %d finite floats, got shape %r" % (fn, self.n_emb, cen.shape))
        d = self.n_emb
        sums = np.zeros(d, dtype=np.float64)
        G = np.zeros((d, d), dtype=np.float64) if gram else None
        ms = ctypes.c_double()
        self._ck(lib.gg_gram(self._ctx, which, _ptr(nodes_a), len(nodes_a), _ptr(cen), _ptr(sums), _ptr(G), ctypes.byref(ms)))
        return dict(sums=sums, gram=G, ms=ms.value)

    def pca(self, nodes, n_components=None, which=0):
        """PCA of the rows ``nodes`` (m >= 2) of table ``which`` in two sweeps on the device.  Pass A, ``gram(center=None,
        gram=False)``: mean64 = sums / m, center = float32(mean64).  Pass B, ``gram(center)``: G and the residual sums r (the fp32
        centre is not the float64 mean).  Host, float64: cov = (G - outer(r, r) / m) / m, numpy.linalg.eigh, eigenvalues
        descending and clipped at 0, every eigenvector signed so that its largest-magnitude entry (the lowest index on ties) is
        positive.  Returns dict(mean fp32 [d], eigenvalues float64 [d], components fp32 [n_components, d] (rows; None = all d),
        cov float64 [d, d], m, mean64 -- pass A's float64 mean --, ms -- the device time of both sweeps)."""
        fn = "pca"
        nodes_a = self._km_args(fn, nodes, which)
        m, d = len(nodes_a), self.n_emb
        if m < 2:
            raise ValueError("%s: needs m >= 2 rows, got %d" % (fn, m))
        if n_components is None:
            n_components = d
        if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= int(n_components) <= d:
            raise ValueError("%s: n_components must be an integer in [1, %d], got %r" % (fn, d, n_components))
        a = self.gram(nodes_a, center=None, which=which, gram=False)
        mean64 = a["sums"] / m
        center = mean64.astype(np.float32)
        b = self.gram(nodes_a, center=center, which=which, gram=True)
        cov = pca_cov(b["gram"], b["sums"], m)
        lam, vec = pca_eig(cov)
        return dict(mean=center, eigenvalues=lam, components=np.ascontiguousarray(vec[:int(n_components)], dtype=np.float32), cov=cov, m=m,
                    mean64=mean64, ms=a["ms"] + b["ms"])

    def pca_transform(self, nodes, mean, components, which=0):
        """The rows ``nodes`` of table ``which`` projected on ``components`` [n_components <= 128, n_emb] about ``mean`` [n_emb]
        -> fp32 [m, n_components].  It is the logits of ``classifier_predict`` with W = components and
        b = float32(-(components64 @ mean64)): the dot products run on the uncentred rows, so the rounding is relative to
        |W| |x|, not to the centred value -- good for plotting and for features, not a bit contract of its own."""
        fn = "pca_transform"
        W = np.ascontiguousarray(components, dtype=np.float32)
        mu = np.ascontiguousarray(mean, dtype=np.float32)
        if W.ndim != 2 or W.shape[1] != self.n_emb or mu.shape != (self.n_emb,):
            raise ValueError("%s: components must be [n_components, %d] and mean [%d], got %r and %r" % (fn, self.n_emb, self.n_emb, W.shape, mu.shape))
        if not 1 <= W.shape[0] <= 128:
            raise ValueError("%s: n_components = %d outside [1, 128]" % (fn, W.shape[0]))
        nodes_a = self._km_args(fn, nodes, which)
        bias = (-(W.astype(np.float64) @ mu.astype(np.float64))).astype(np.float32)
        if W.shape[0] == 1:  # (gg_classifier_predict takes 2 .. 128 classes: a second, zero component rides along)
            z = self.classifier_predict(nodes_a, np.vstack([W, np.zeros_like(W)]), np.append(bias, np.float32(0)), which=which, logits=True)[1]
            return np.ascontiguousarray(z[:, :1])
        return self.classifier_predict(nodes_a, W, bias, which=which, logits=True)[1]

    def get_embeddings(self, which):
        """sess.run(embedding_matrix) (graph_gan.py:298); which: 0 = gen, 1 = dis."""
        out = np.zeros((self.n_node, self.n_emb), dtype=np.float32)
        self._ck(lib.gg_get_embeddings(self._ctx, which, _ptr(out)))
        return out

    def write_embeddings(self, which, path, n_threads=0):
        """write_embeddings_to_file (graph_gan.py:293-306) for one model, natively."""
        self._ck(lib.gg_write_embeddings(self._ctx, which, str(path).encode(), n_threads))

    def write_embeddings_bin(self, which, path):
        """Binary side-car of the ``.emb`` text (same fp32 numbers; header "GGEB", version, n_emb, n_node)."""
        self._ck(lib.gg_write_embeddings_bin(self._ctx, which, str(path).encode()))

    def edge_scores(self, which, u, v):
        """Evaluator scores np.dot(emd[u], emd[v]) (link_prediction.py:26-27) from the resident table, float64."""
        u, v = _i32(u), _i32(v)
        out = np.zeros(len(u), dtype=np.float64)
        self._ck(lib.gg_edge_scores(self._ctx, which, _ptr(u), _ptr(v), len(u), _ptr(out)))
        return out

    def get_bias(self, which):
        out = np.zeros(self.n_node, dtype=np.float32)
        self._ck(lib.gg_get_bias(self._ctx, which, _ptr(out)))
        return out

    def set_embeddings(self, which, emb):
        emb = np.ascontiguousarray(emb, dtype=np.float32)
        assert emb.shape == (self.n_node, self.n_emb)
        self._ck(lib.gg_set_embeddings(self._ctx, which, _ptr(emb)))

    def set_bias(self, which, bias):
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        assert bias.shape == (self.n_node,)
        self._ck(lib.gg_set_bias(self._ctx, which, _ptr(bias)))

    def save_state(self, path):
        self._ck(lib.gg_save_state(self._ctx, path.encode()))

    def load_state(self, path):
        self._ck(lib.gg_load_state(self._ctx, path.encode()))

    def counters(self):
        c = GGCounters()
        self._ck(lib.gg_get_counters(self._ctx, ctypes.byref(c)))
        return {k: getattr(c, k) for k, _ in GGCounters._fields_ if k != "reserved"}

    def set_profiling(self, every_n):
        """HIP events around every ``every_n``-th walk launch (1 = every launch and every pass, the default;
        0 = none).  With ``every_n != 1`` ``d_pass`` / ``g_pass`` return once their kernels are enqueued."""
        self._ck(lib.gg_set_profiling(self._ctx, int(every_n)))

    def set_profiling_solo(self, solo):
        """solo=True (default): profiled side-stream walks are measured alone; False: overlapped with the D update."""
        self._ck(lib.gg_set_profiling_solo(self._ctx, int(bool(solo))))

    def synchronize(self):
        self._ck(lib.gg_synchronize(self._ctx))

    # ------------------------------------------------------------------ multi-GPU
    @staticmethod
    def comm_unique_id():
        buf = (ctypes.c_char * 128)()
        check(lib.gg_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (ctypes.c_char * 128).from_buffer_copy(unique_id)
        self._ck(lib.gg_comm_init(self._ctx, buf, rank, world))

    def comm_stats(self):
        """Gradient-exchange statistics of this rank: dict(sparse_steps, dense_steps, bytes_sent, world) + what kind the sparse
        steps were (pack_steps: all-gather of fixed-capacity row packs; owner_steps: owner-partitioned send / recv + gather) and
        whether the owner-partitioned exchange moves bf16 rows."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(lib.gg_comm_stats_ex(self._ctx, _ptr(out)))
        return dict(sparse_steps=int(out[0] + out[1]), dense_steps=int(out[2]), bytes_sent=int(out[3]), world=int(out[4]),
                    pack_steps=int(out[0]), owner_steps=int(out[1]), bf16_rows=bool(out[5]))

    def comm_barrier(self):
        self._ck(lib.gg_comm_barrier(self._ctx))
