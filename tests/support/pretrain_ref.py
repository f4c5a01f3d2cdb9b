"""numpy oracle of the pre-training sampling contract P1-P5 (include/graphgan_hip.h), written from the rule text alone:
a vectorised Philox4x32-10 over uint64 arrays, the integer threshold, uniform walks, window pairs, negatives, rows.
It never calls into the library."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable uint64 arrays holding 32-bit words; returns the four output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)])
    k0, k1 = _U(int(k0) & 0xFFFFFFFF), _U(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = _U(0xD2511F53) * c0
        p1 = _U(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _U(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> _U(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + _U(0x9E3779B9)) & _M32
        k1 = (k1 + _U(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def uniform53(seed, stream, root, walk, hop):
    """P1: the 53-bit numerator m; counter (hop, walk, root, stream), key = the two halves of seed."""
    seed = int(seed)
    o0, o1, _, _ = philox4x32_10(hop, walk, root, stream, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return ((o0 >> _U(5)) << _U(26)) | (o1 >> _U(6))


def threshold(m, K):
    """floor(m * K / 2^53) for m < 2^53, K < 2^63, exactly: the 128-bit product from 32-bit limbs."""
    m, K = np.broadcast_arrays(np.asarray(m, dtype=np.uint64), np.asarray(K, dtype=np.uint64))
    a0, a1, b0, b1 = m & _M32, m >> _U(32), K & _M32, K >> _U(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _U(32)) + (p01 & _M32) + (p10 & _M32)
    lo = (p00 & _M32) | ((mid & _M32) << _U(32))
    hi = p11 + (p01 >> _U(32)) + (p10 >> _U(32)) + (mid >> _U(32))
    return (hi << _U(11)) | (lo >> _U(53))


def pair_template(length, window):
    """P3: (i, j) index arrays of the pairs of a path of ``length`` nodes, in pair order."""
    I, J = [], []
    for i in range(length):
        for j in range(max(i - window, 0), min(i + window, length - 1) + 1):
            if j != i:
                I.append(i)
                J.append(j)
    return np.array(I, dtype=np.int64), np.array(J, dtype=np.int64)


def rows_of_length(length, window, n_neg):
    """P5: rows of a walk of ``length`` nodes."""
    return (1 + n_neg) * sum(min(i, window) + min(length - 1 - i, window) for i in range(length))


def walks(rowptr, col, starts, walks_per_start, walk_len, seed, stream):
    """P2 for every (start index, w): paths int32 [n_walks, walk_len] (-1 behind the end), path_len int32 [n_walks]."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    root = np.repeat(starts, walks_per_start)
    w = np.tile(np.arange(walks_per_start, dtype=np.int64), len(starts))
    nw = len(root)
    paths = np.full((nw, walk_len), -1, dtype=np.int32)
    plen = np.ones(nw, dtype=np.int32)
    if nw == 0:
        return paths, plen
    paths[:, 0] = root
    alive = np.arange(nw)
    cur = root.copy()
    for h in range(1, walk_len):
        k = rowptr[cur[alive] + 1] - rowptr[cur[alive]]
        alive = alive[k > 0]
        if len(alive) == 0:
            break
        k = k[k > 0]
        t = threshold(uniform53(seed, stream, root[alive], w[alive], h), k).astype(np.int64)
        nxt = col[rowptr[cur[alive]] + t]
        cur[alive] = nxt
        paths[alive, h] = nxt
        plen[alive] = h + 1
    return paths, plen


def rows(rowptr, col, n_node, starts, walks_per_start, walk_len, window, n_neg, seed, stream, weights=None, select=None):
    """P1-P5.  Returns dict(paths, path_len, row_off int64 [n_walks + 1], center, neighbor, label): the rows of the whole call,
    or with ``select`` (walk indices) only those walks' rows, concatenated in the order given (row_off still describes the
    whole call)."""
    starts = np.asarray(starts, dtype=np.int64)
    paths, plen = walks(rowptr, col, starts, walks_per_start, walk_len, seed, stream)
    nw = len(plen)
    per_len = np.array([rows_of_length(l, window, n_neg) for l in range(walk_len + 1)], dtype=np.int64)
    row_off = np.zeros(nw + 1, dtype=np.int64)
    np.cumsum(per_len[plen], out=row_off[1:])
    sel = np.arange(nw) if select is None else np.asarray(select, dtype=np.int64)
    out_off = np.zeros(len(sel) + 1, dtype=np.int64)
    np.cumsum(per_len[plen[sel]], out=out_off[1:])
    total = int(out_off[-1])
    center = np.zeros(total, np.int32)
    neighbor = np.zeros(total, np.int32)
    label = np.zeros(total, np.float32)
    cum = None
    if weights is not None:
        cum = np.cumsum(np.asarray(weights, dtype=np.uint64), dtype=np.uint64)
        assert int(cum[-1]) >= 1
    root = np.repeat(starts, walks_per_start)
    wno = np.tile(np.arange(walks_per_start, dtype=np.int64), len(starts))
    np1 = 1 + n_neg
    for length in np.unique(plen[sel]):
        I, J = pair_template(int(length), window)
        P = len(I)
        if P == 0:
            continue
        pos = np.nonzero(plen[sel] == length)[0]
        for a in range(0, len(pos), 2048):
            ps = pos[a:a + 2048]
            g = sel[ps]
            c = paths[g][:, I].astype(np.int64)   # [n, P]
            x = paths[g][:, J].astype(np.int64)
            blockc = np.repeat(c[:, :, None], np1, axis=2)
            blockn = np.empty_like(blockc)
            blockn[:, :, 0] = x
            if n_neg:
                hop = walk_len + np.arange(P, dtype=np.int64)[:, None] * n_neg + np.arange(n_neg, dtype=np.int64)[None, :]
                m = uniform53(seed, stream, root[g][:, None, None], wno[g][:, None, None], hop[None, :, :])
                if cum is not None:
                    node = np.searchsorted(cum, threshold(m, cum[-1]), side="right").astype(np.int64)  # first j with C_j > t
                else:
                    node = threshold(m, n_node).astype(np.int64)
                for _ in range(2):
                    hit = (node == c[:, :, None]) | (node == x[:, :, None])
                    node = np.where(hit, (node + 1) % n_node, node)
                blockn[:, :, 1:] = node
            lab = np.zeros((len(g), P, np1), np.float32)
            lab[:, :, 0] = 1.0
            dst = (out_off[ps][:, None] + np.arange(P * np1, dtype=np.int64)[None, :]).reshape(-1)
            center[dst] = blockc.reshape(-1)
            neighbor[dst] = blockn.reshape(-1)
            label[dst] = lab.reshape(-1)
    return dict(paths=paths, path_len=plen, row_off=row_off, sel_off=out_off, center=center, neighbor=neighbor, label=label)


# ----------------------------------------------------------------------------- the end-to-end schedule on CA-GrQc

def e2e_config():
    """The schedule of the end-to-end test: d = 50, engine_seed 1, lr 5e-3, lambda 1e-5, 4 walks x 10 nodes, window 2,
    3 negatives, batch 4096, one epoch."""
    import types
    return types.SimpleNamespace(n_emb=50, engine_seed=1, engine_device=0, lambda_dis=1e-5, engine_pretrain_lr=5e-3,
                                 engine_pretrain_walks=4, engine_pretrain_len=10, engine_pretrain_window=2, engine_pretrain_neg=3,
                                 engine_pretrain_epochs=1, engine_pretrain_batch=4096, engine_pretrain_rows_per_call=1 << 26)


def oracle_leg(d, n, rowptr, col):
    """The numpy side of the end-to-end test: the rows of the contract (weights round(16 * max(deg, 1) ^ 0.75), stream
    0x50000000, all nodes in id order, one call) through the oracle's lazy-Adam discriminator in the batch order of
    RandomState(engine_seed).  ``d``: the CA-GrQc fixture (test / test_neg edges).  Returns dict(rows, steps, acc_init,
    acc_oracle, table)."""
    from oracle import graphgan_oracle as orc
    cfg = e2e_config()
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    weights = np.round(16.0 * np.maximum(deg, 1).astype(np.float64) ** 0.75).astype(np.uint32)
    r = rows(rowptr, col, n, np.arange(n), cfg.engine_pretrain_walks, cfg.engine_pretrain_len, cfg.engine_pretrain_window,
             cfg.engine_pretrain_neg, cfg.engine_seed, 0x50000000, weights=weights)
    init = ((np.random.RandomState(cfg.engine_seed).rand(n, cfg.n_emb) - 0.5) / cfg.n_emb).astype(np.float32)
    test, test_neg = d["test"].tolist(), d["test_neg"].tolist()
    acc_init = orc.eval_link_prediction(init.astype(np.float64), test, test_neg)
    dis = orc.Discriminator(init, cfg.engine_pretrain_lr, lazy=True)
    n_rows, batch = len(r["center"]), cfg.engine_pretrain_batch
    starts = np.arange(0, n_rows, batch, dtype=np.int64)
    np.random.RandomState(cfg.engine_seed).shuffle(starts)
    c, x, lab = r["center"].astype(np.int64), r["neighbor"].astype(np.int64), r["label"]
    for s in starts:
        dis.d_step(c[s:s + batch], x[s:s + batch], lab[s:s + batch], cfg.lambda_dis)
    acc = orc.eval_link_prediction(dis.E.astype(np.float64), test, test_neg)
    return dict(rows=n_rows, steps=len(starts), acc_init=acc_init, acc_oracle=acc, table=dis.E)
