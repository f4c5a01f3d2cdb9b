"""What tests/test_gpu_top_pairs.py and tests/test_pair_prediction_cpu.py share: the plain numpy reference of gg_top_pairs over a
FULL score matrix, a restatement of its host schedule (graphgan_amd/csrc/top_pairs.hip, PairRun) that predicts the launches,
retries, compactions and appended entries of a call, and the tables of the tests.

Order: (s, u, v) is ahead of (s', u', v') when s > s', or s == s' (-0 == +0) and (u, v) < (u', v') lexicographically.
Candidates: u < v, both members of `nodes`; with a graph, v not in nbrs[u]."""
import numpy as np

MAX_K = 1 << 20
MIN_BUF, MAX_BUF = 1 << 22, 1 << 26
TILE = 32 * 128
MAX_ROW_TILES = 128
MAX_AREA = (1 << 32) - (1 << 27)
INT_MAX = 0x7FFFFFFF


def cdiv(a, b):
    return -(-a // b)


def default_buffer(k):
    return max(MIN_BUF, 4 * k)


def eligible(n, nodes=None, nbrs=None):
    """[n, n] bool: (u, v) is a candidate"""
    ok = np.triu(np.ones((n, n), dtype=bool), 1)
    if nodes is not None:
        mem = np.zeros(n, dtype=bool)
        mem[np.asarray(nodes, dtype=np.int64)] = True
        ok &= mem[:, None] & mem[None, :]
    if nbrs is not None:
        for u in range(n):
            if nbrs[u]:
                ok[u, sorted(nbrs[u])] = False
    return ok


def ref_top_pairs(S, k, nodes=None, nbrs=None):
    """S [n, n]: S[u, v] the score of row u, column v (any dtype; its values are returned as they are)
    -> (u int32 [k], v int32 [k], score S.dtype [k], n_found), -1 / -1 / -inf behind n_found"""
    n = S.shape[0]
    uu, vv = np.nonzero(eligible(n, nodes, nbrs))
    s = S[uu, vv]
    key = s.astype(np.float64) + 0.0
    if len(s) > k:  # the candidates at or above the k-th score, then the full order among them
        cut = np.partition(key, len(key) - k)[len(key) - k]
        keep = key >= cut
        uu, vv, s, key = uu[keep], vv[keep], s[keep], key[keep]
    o = np.lexsort((vv, uu, -key))[:k]
    f = len(o)
    u_out, v_out = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32)
    s_out = np.full(k, -np.inf, dtype=np.float32 if S.dtype.kind != "f" else S.dtype)
    u_out[:f], v_out[:f], s_out[:f] = uu[o], vv[o], s[o]
    return u_out, v_out, s_out, f


def ref_top_pairs_small_ints(E, k, block=2048):
    """The reference for a large table of small integers, in row blocks: the scores of rows [b0, b1) x columns [b0, n) (exact in
    float32 BLAS; the collected ones are taken to int64), the pairs at or above a running threshold -- the k-th best score
    collected so far, which never exceeds the k-th best of all -- are kept, then the full order.
    -> (u, v, score float32, n_found)"""
    X = np.asarray(E, dtype=np.float32)
    n = X.shape[0]
    assert float(np.abs(X).max()) ** 2 * X.shape[1] < 1 << 20
    thr = -np.inf
    uu, vv, ss = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        S = X[b0:b1] @ X[b0:].T
        S[:, :b1 - b0][np.tril_indices(b1 - b0)] = -np.inf        # v <= u: no pair
        if thr == -np.inf and np.count_nonzero(S > -np.inf) > k:
            thr = np.partition(S.ravel(), S.size - k)[S.size - k]
        r, c = np.nonzero(S >= thr) if thr > -np.inf else np.nonzero(S > -np.inf)
        uu, vv = np.concatenate([uu, r + b0]), np.concatenate([vv, c + b0])
        ss = np.concatenate([ss, np.rint(S[r, c]).astype(np.int64)])
        if len(ss) > k:
            thr = float(np.partition(ss, len(ss) - k)[len(ss) - k])
            keep = ss >= thr
            uu, vv, ss = uu[keep], vv[keep], ss[keep]
    o = np.lexsort((vv, uu, -ss))[:k]
    f = len(o)
    u_out, v_out, s_out = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32), np.full(k, -np.inf, dtype=np.float32)
    u_out[:f], v_out[:f], s_out[:f] = uu[o], vv[o], ss[o]
    return u_out, v_out, s_out, f


def simulate_schedule(S, k, cap, nodes=None, nbrs=None):
    """PairRun of top_pairs.hip in plain Python on the full score matrix S (float32: the stream's scores)
    -> dict(launches, retries, compactions, appended)"""
    n = S.shape[0]
    ids = np.arange(n, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
    m = len(ids)
    st = dict(launches=0, retries=0, compactions=0, appended=0)
    if m < 2:
        return st
    ok = eligible(n, nodes, nbrs)[ids]
    Sr = np.asarray(S)[ids]
    U = np.broadcast_to(ids[:, None], Sr.shape)
    V = np.broadcast_to(np.arange(n, dtype=np.int64)[None, :], Sr.shape)
    state = dict(s=np.zeros(0, Sr.dtype), u=np.zeros(0, np.int64), v=np.zeros(0, np.int64), floor=(-np.inf, INT_MAX, INT_MAX))
    T, n_up = cdiv(m, 32), cdiv(n, 128) * 128

    def first_col(rt):
        return int(ids[rt * 32]) & ~127

    def compact():
        o = np.lexsort((state["v"], state["u"], -(state["s"].astype(np.float64) + 0.0)))[:k]
        state["s"], state["u"], state["v"] = state["s"][o], state["u"][o], state["v"][o]
        if len(o) == k:
            state["floor"] = (state["s"][-1], int(state["u"][-1]), int(state["v"][-1]))
        st["compactions"] += 1

    def run(rt0, rt1, cbeg, cend):
        nt = rt1 - rt0
        c_lo = max(cbeg, first_col(rt0)) if nt > 0 else cbeg
        if nt <= 0 or c_lo >= cend:
            return
        tiles = cdiv(cend - c_lo, 128)
        st["launches"] += 1
        rows = slice(rt0 * 32, min(m, rt1 * 32))
        s, u, v = Sr[rows, c_lo:cend], U[rows, c_lo:cend], V[rows, c_lo:cend]
        fs, fu, fv = state["floor"]
        hit = ok[rows, c_lo:cend] & ((s > fs) | ((s == fs) & ((u < fu) | ((u == fu) & (v < fv)))))
        cnt = int(hit.sum())
        if len(state["s"]) + cnt <= cap:
            st["appended"] += cnt
            state["s"], state["u"], state["v"] = (np.concatenate([state["s"], s[hit]]), np.concatenate([state["u"], u[hit]]),
                                                  np.concatenate([state["v"], v[hit]]))
            if len(state["s"]) > min(k + (cap - k) // 2, max(3 * k, 1 << 16)):
                compact()
            return
        st["retries"] += 1
        if len(state["s"]) > k:
            compact()
        if nt > 1:
            mid = rt0 + nt // 2
            run(rt0, mid, cbeg, cend)
            run(mid, rt1, cbeg, cend)
        else:
            assert tiles > 1, "one 32 x 128 tile overflowed"
            mid = c_lo + (tiles // 2) * 128
            run(rt0, rt1, c_lo, mid)
            run(rt0, rt1, mid, cend)

    area = max(cap - k, TILE)
    rt, c = 0, -1
    while rt < T:
        cs = first_col(rt) if c < 0 else c
        w = n_up - cs
        if w <= 0:
            rt, c = rt + 1, -1
            continue
        if c < 0 and 32 * w <= area:
            nt = min(T - rt, MAX_ROW_TILES, area // (32 * w))
            run(rt, rt + nt, cs, n)
            rt += nt
        else:
            cw = max(128, area // 32 // 128 * 128)
            ce = min(n_up, cs + cw)
            run(rt, rt + 1, cs, min(ce, n))
            c = ce
            if c >= n:
                rt, c = rt + 1, -1
        area = min(area * 2, MAX_AREA)
    compact()
    return st


# ---- tables --------------------------------------------------------------------------------------------------------------------
def int_table(n, d, seed):
    """entries of {-1, 0, 1}: every score is a small integer, exact in fp32 and bf16 in any summation order"""
    return np.random.RandomState(seed).randint(-1, 2, size=(n, d)).astype(np.float32)


def gram(E):
    """E . E^T in float64 (exact on integer tables) as float32; + 0.0: the zero the chains from +0.0 end at"""
    E64 = np.asarray(E, dtype=np.float64)
    return (E64 @ E64.T + 0.0).astype(np.float32)


def ascending_table(n, d):
    """s(u, v) = (u // 32) (v // 32): every pair of a later row tile beats the floor the earlier tiles left"""
    E = np.zeros((n, d), dtype=np.float32)
    E[:, 0] = np.arange(n) // 32
    return E


def peaks_table(n, d, peaks):
    """a table whose best pairs are exactly `peaks`, in that order: pair j holds 16 - j at coordinate j of both ends (d > len(peaks),
    the ends of different peaks distinct); every other score is 0"""
    E = np.zeros((n, d), dtype=np.float32)
    for j, (a, b) in enumerate(peaks):
        E[a, j] = E[b, j] = 16 - j
    return E


def nbr_sets(n, edges):
    nb = [set() for _ in range(n)]
    for a, b in np.asarray(edges).reshape(-1, 2).tolist():
        nb[a].add(b)
        nb[b].add(a)
    return nb


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
