"""numpy oracle of the biased-walk rule P2b (include/graphgan_hip.h), written from the rule text alone: the class of a
candidate, the R = 32 rejection trials with their hop words, the exact draw behind them.  ``walks`` is vectorised over the
walks (loops over hops and trials, with masks), ``scalar_walks`` restates the rule one walk, one hop, one list entry at a
time for cross-checking, ``rows`` composes the walks with pretrain_ref's pairs / negatives.  It never calls the library."""
import numpy as np

from tests.support import pretrain_ref as ref

R = 32
HOP_C, HOP_A = 1 << 31, 1 << 30  # hop words of the candidate draws r >= 1 / the accept draws: base + 256 r + h


def _check_bias(bias):
    w = tuple(int(x) for x in bias)
    assert len(w) == 3 and all(1 <= x <= 65536 for x in w), bias
    return w


def _edge_keys(rowptr, col):
    """Sorted keys u * n + v of every list entry: x occurs in adj(prev) <=> prev * n + x is among them."""
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    return np.unique(src * n + col), n


def _classes(x, prev, keys, n, bias):
    """Class weights of candidates x (int64 array) with previous nodes prev (broadcastable)."""
    w_ret, w_com, w_out = bias
    x, prev = np.broadcast_arrays(np.asarray(x, dtype=np.int64), np.asarray(prev, dtype=np.int64))
    k = prev * n + x
    pos = np.searchsorted(keys, k)
    member = keys[np.minimum(pos, len(keys) - 1)] == k if len(keys) else np.zeros(x.shape, bool)
    return np.where(x == prev, w_ret, np.where(member, w_com, w_out)).astype(np.int64)


def walks(rowptr, col, starts, walks_per_start, walk_len, seed, stream, bias, stats=None):
    """P2b for every (start index, w): paths int32 [n_walks, walk_len] (-1 behind the end), path_len int32 [n_walks].
    ``stats`` (a dict) receives ``biased_hops`` and ``fallback_hops`` (hops that ran trials / whose R trials all failed) and
    ``fallback_from`` (int64 array: the node cur of every fallback hop)."""
    bias = _check_bias(bias)
    M = max(bias)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    keys, n = _edge_keys(rowptr, col)
    root = np.repeat(starts, walks_per_start)
    w = np.tile(np.arange(walks_per_start, dtype=np.int64), len(starts))
    nw = len(root)
    paths = np.full((nw, walk_len), -1, dtype=np.int32)
    plen = np.ones(nw, dtype=np.int32)
    n_biased, fb_from, cums = 0, [], {}
    if nw:
        paths[:, 0] = root
    alive = np.arange(nw)
    cur = root.copy()
    prev = np.full(nw, -1, dtype=np.int64)
    equal = bias[0] == bias[1] == bias[2]
    for h in range(1, walk_len):
        if len(alive) == 0:
            break
        k = rowptr[cur[alive] + 1] - rowptr[cur[alive]]
        alive, k = alive[k > 0], k[k > 0]
        if len(alive) == 0:
            break
        e0 = rowptr[cur[alive]]
        nxt = np.full(len(alive), -1, dtype=np.int64)
        plain = np.ones(len(alive), bool) if (h == 1 or equal) else k == 1
        if plain.any():
            a = alive[plain]
            nxt[plain] = col[e0[plain] + ref.threshold(ref.uniform53(seed, stream, root[a], w[a], h), k[plain]).astype(np.int64)]
        pend = np.nonzero(~plain)[0]  # positions in alive still without an accepted candidate
        n_biased += len(pend)
        for r in range(R):
            if len(pend) == 0:
                break
            a = alive[pend]
            hop_c = h if r == 0 else HOP_C + 256 * r + h
            m_c, m_a = ref.uniform53(seed, stream, root[a], w[a], np.array([[hop_c], [HOP_A + 256 * r + h]], dtype=np.int64))
            x = col[e0[pend] + ref.threshold(m_c, k[pend]).astype(np.int64)]
            c = _classes(x, prev[a], keys, n, bias)
            t_a = ref.threshold(m_a, M).astype(np.int64)  # (drawn for every candidate here; the rule needs it only below M)
            ok = (c == M) | (t_a < c)
            nxt[pend[ok]] = x[ok]
            pend = pend[~ok]
        for i in pend:  # the exact draw
            g = alive[i]
            lst = col[e0[i]:e0[i] + k[i]]
            key = (int(cur[g]), int(prev[g]))
            if key not in cums:  # (a hub is left towards the same few neighbours again and again)
                cums[key] = np.cumsum(_classes(lst, prev[g], keys, n, bias))
            cum = cums[key]
            t = int(ref.threshold(ref.uniform53(seed, stream, root[g], w[g], HOP_C + 256 * R + h), int(cum[-1])))
            nxt[i] = lst[np.searchsorted(cum, t, side="right")]  # the first entry whose inclusive prefix sum exceeds t
            fb_from.append(int(cur[g]))
        prev[alive] = cur[alive]
        cur[alive] = nxt
        paths[alive, h] = nxt
        plen[alive] = h + 1
    if stats is not None:
        stats.update(biased_hops=n_biased, fallback_hops=len(fb_from), fallback_from=np.array(fb_from, dtype=np.int64))
    return paths, plen


def scalar_walks(rowptr, col, starts, walks_per_start, walk_len, seed, stream, bias):
    """The same rule, deliberately naive: python loops over walks, hops, trials and list entries, membership by a scan."""
    w_ret, w_com, w_out = _check_bias(bias)
    M = max(w_ret, w_com, w_out)
    rowptr = [int(v) for v in rowptr]
    col = [int(v) for v in col]

    def draw(s, wi, hop, K):
        return int(ref.threshold(ref.uniform53(seed, stream, s, wi, hop), K))

    def cls(x, prev):
        if x == prev:
            return w_ret
        for e in range(rowptr[prev], rowptr[prev + 1]):
            if col[e] == x:
                return w_com
        return w_out

    paths, plen = [], []
    for s in (int(v) for v in starts):
        for wi in range(walks_per_start):
            path = [s]
            for h in range(1, walk_len):
                cur = path[h - 1]
                e0, k = rowptr[cur], rowptr[cur + 1] - rowptr[cur]
                if k == 0:
                    break
                if h == 1 or k == 1 or w_ret == w_com == w_out:
                    path.append(col[e0 + draw(s, wi, h, k)])
                    continue
                prev, got = path[h - 2], None
                for r in range(R):
                    x = col[e0 + draw(s, wi, h if r == 0 else 2 ** 31 + 256 * r + h, k)]
                    c = cls(x, prev)
                    if c == M or draw(s, wi, 2 ** 30 + 256 * r + h, M) < c:
                        got = x
                        break
                if got is None:
                    W = sum(cls(col[e], prev) for e in range(e0, e0 + k))
                    t, acc = draw(s, wi, 2 ** 31 + 256 * R + h, W), 0
                    for e in range(e0, e0 + k):
                        acc += cls(col[e], prev)
                        if acc > t:
                            got = col[e]
                            break
                path.append(got)
            plen.append(len(path))
            paths.append(path + [-1] * (walk_len - len(path)))
    return np.array(paths, dtype=np.int32).reshape(-1, walk_len), np.array(plen, dtype=np.int32)


def rows(rowptr, col, n_node, starts, walks_per_start, walk_len, window, n_neg, seed, stream, bias, weights=None, stats=None,
         walked=None):
    """P1, P2b, P3-P5: dict(paths, path_len, row_off int64 [n_walks + 1], center, neighbor, label) of one call -- the
    biased walks above, then pairs, negatives and rows composed from pretrain_ref's pair_template / uniform53 / threshold.
    ``walked``: the (paths, path_len) of an earlier call with the same walk arguments (the walks do not depend on window,
    negatives or noise weights), to save walking again."""
    starts = np.asarray(starts, dtype=np.int64)
    paths, plen = walked if walked is not None else walks(rowptr, col, starts, walks_per_start, walk_len, seed, stream, bias, stats=stats)
    nw = len(plen)
    per_len = np.array([ref.rows_of_length(l, window, n_neg) for l in range(walk_len + 1)], dtype=np.int64)
    row_off = np.zeros(nw + 1, dtype=np.int64)
    np.cumsum(per_len[plen], out=row_off[1:])
    total = int(row_off[-1])
    center, neighbor, label = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(total, np.float32)
    cum = None
    if weights is not None:
        cum = np.cumsum(np.asarray(weights, dtype=np.uint64), dtype=np.uint64)
        assert int(cum[-1]) >= 1
    root = np.repeat(starts, walks_per_start)
    wno = np.tile(np.arange(walks_per_start, dtype=np.int64), len(starts))
    np1 = 1 + n_neg
    for length in np.unique(plen):
        I, J = ref.pair_template(int(length), window)
        P = len(I)
        if P == 0:
            continue
        pos = np.nonzero(plen == length)[0]
        for a in range(0, len(pos), 2048):
            g = pos[a:a + 2048]
            c = paths[g][:, I].astype(np.int64)  # [n, P]
            x = paths[g][:, J].astype(np.int64)
            nb = np.empty((len(g), P, np1), dtype=np.int64)
            nb[:, :, 0] = x
            if n_neg:
                hop = walk_len + np.arange(P, dtype=np.int64)[:, None] * n_neg + np.arange(n_neg, dtype=np.int64)[None, :]
                m = ref.uniform53(seed, stream, root[g][:, None, None], wno[g][:, None, None], hop[None, :, :])
                if cum is not None:
                    node = np.searchsorted(cum, ref.threshold(m, cum[-1]), side="right").astype(np.int64)
                else:
                    node = ref.threshold(m, n_node).astype(np.int64)
                for _ in range(2):
                    hit = (node == c[:, :, None]) | (node == x[:, :, None])
                    node = np.where(hit, (node + 1) % n_node, node)
                nb[:, :, 1:] = node
            lab = np.zeros((len(g), P, np1), np.float32)
            lab[:, :, 0] = 1.0
            dst = (row_off[g][:, None] + np.arange(P * np1, dtype=np.int64)[None, :]).reshape(-1)
            center[dst] = np.repeat(c[:, :, None], np1, axis=2).reshape(-1)
            neighbor[dst] = nb.reshape(-1)
            label[dst] = lab.reshape(-1)
    return dict(paths=paths, path_len=plen, row_off=row_off, center=center, neighbor=neighbor, label=label)


# ----------------------------------------------------------------------------- the law test's graph

LAW_EDGES = [(1, 4), (0, 1), (1, 2), (1, 5), (0, 2), (1, 3), (0, 3), (1, 6), (4, 7), (5, 7), (6, 7)]  # file order
LAW_ARGS = dict(start=0, n_walks=40_000, walk_len=3, seed=11, stream=2)


def law_graph():
    """(n, rowptr, col) of the 8-node graph of the law test: undirected, every list in the file order of LAW_EDGES.  From
    0 -> 1 the candidates are 0 (return), 2 and 3 (neighbours of 0), 4, 5 and 6 (neither)."""
    n = 8
    lists = [[] for _ in range(n)]
    for a, b in LAW_EDGES:
        lists[a].append(b)
        lists[b].append(a)
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return n, rowptr, np.array([v for x in lists for v in x], dtype=np.int32)


def law_counts(paths):
    """Among the walks with path[1] == 1: the counts of path[2] over the nodes 0 | 2, 3 | 4, 5, 6 (six numbers, in the order
    of law_expected) and the number of walks whose path[2] is any other value."""
    second = paths[paths[:, 1] == 1, 2]
    counts = np.array([(second == v).sum() for v in (0, 2, 3, 4, 5, 6)], dtype=np.int64)
    return counts, int(len(second) - counts.sum())


def law_expected(bias):
    w_ret, w_com, w_out = bias
    return np.array([w_ret, w_com, w_com, w_out, w_out, w_out], dtype=np.float64)  # nodes 0 | 2, 3 | 4, 5, 6


# ----------------------------------------------------------------------------- the end-to-end schedule on CA-GrQc

def oracle_leg(d, n, rowptr, col, bias):
    """pretrain_ref.oracle_leg with biased walks: the rows of the contract through the oracle's lazy-Adam discriminator in
    the batch order of RandomState(engine_seed).  Returns dict(rows, steps, acc_init, acc_oracle, table)."""
    from oracle import graphgan_oracle as orc
    cfg = ref.e2e_config()
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    weights = np.round(16.0 * np.maximum(deg, 1).astype(np.float64) ** 0.75).astype(np.uint32)
    r = rows(rowptr, col, n, np.arange(n), cfg.engine_pretrain_walks, cfg.engine_pretrain_len, cfg.engine_pretrain_window,
             cfg.engine_pretrain_neg, cfg.engine_seed, 0x50000000, bias, weights=weights)
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
