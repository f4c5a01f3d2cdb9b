"""What tests/test_gpu_gram.py shares: the closed forms and the error bands of gg_gram (graphgan_amd/csrc/gram.hip), and tables on
which its arithmetic is exact.

EXACT.  With table entries and centre in {-1, 0, 1} every c = x - center is an integer of magnitude <= 2, every product is at most
4, and every partial sum stays below 2^24 for m <= 40 000: each float32 chain is exact in any order, so sums and gram equal the
int64 closed form.  A row behind m that entered as 0 - center, a dropped or doubled row, a stale tile or a partial added twice
changes an integer.

DYADIC.  A table whose columns hold fixed proportions of two values with a dyadic mean (m a multiple of 4): {0, 1} with m / 4 ones
(mean 1/4), {-1, 1} with m / 4 minus-ones (mean 1/2), {0, 1} with m / 2 ones (mean 1/2).  The float32 centre IS the mean, c is a
multiple of 1/4, every product a multiple of 1/16, every sum exact: G and r = 0 are exact on the device, and the float64 host
arithmetic behind them is the same code on the same numbers.

BAND.  Against float64 on C = float64(X) - float64(center), entry (j, l) of gram may differ by at most
    (m + 3) 2^-24 sum_i |C_ij| |C_il|
-- the standard bound of an m-term float32 chain at its worst case (one chain over all rows, whatever the launch plan), two
relative roundings for the two subtractions and one for slack -- and entry j of sums by (m + 1) 2^-24 sum_i |C_ij|.
"""
import numpy as np

U = 2.0 ** -24
N_TABLE = 5000


def int_tables(d):
    """two tables [N_TABLE, d] with entries in {-1, 0, 1}"""
    rs = np.random.RandomState(9000 + d)
    return rs.randint(-1, 2, size=(N_TABLE, d)).astype(np.float32), rs.randint(-1, 2, size=(N_TABLE, d)).astype(np.float32)


def draw_nodes(rs, m, n_table=N_TABLE):
    """node ids with replacement, one id three times"""
    nodes = rs.randint(0, n_table, size=m)
    if m > 2:
        nodes[m // 2] = nodes[0]
        nodes[-1] = nodes[0]
    return nodes


def int_gram(X, center=None):
    """(sums int64 [d], gram int64 [d, d]) of integer rows X [m, d] about an integer centre"""
    Xi = np.rint(np.asarray(X)).astype(np.int64)
    assert np.array_equal(Xi, np.asarray(X))
    if center is not None:
        ci = np.rint(np.asarray(center)).astype(np.int64)
        assert np.array_equal(ci, np.asarray(center))
        Xi = Xi - ci[None, :]
    G = Xi.T @ Xi
    assert int(np.abs(G).max(initial=0)) < 2 ** 24 and int(np.abs(Xi).sum(axis=0).max(initial=0)) < 2 ** 24
    return Xi.sum(axis=0), G


def bands(X, center):
    """(C^T C float64, its band [d, d], column sums float64, their band [d]) for float32 rows X [m, d] and a float32 centre (or None)"""
    C = np.asarray(X, dtype=np.float64)
    if center is not None:
        C = C - np.asarray(center, dtype=np.float64)[None, :]
    m = len(C)
    A = np.abs(C)
    return C.T @ C, (m + 3) * U * (A.T @ A), C.sum(axis=0), (m + 1) * U * A.sum(axis=0)


def dyadic_table(m, d, seed):
    """float32 [m, d], m a multiple of 4: column j is of kind j % 3 -- {0, 1} with m / 4 ones, {-1, 1} with m / 4 minus-ones,
    {0, 1} with m / 2 ones --, each column shuffled on its own.  Column means 1/4, 1/2, 1/2."""
    assert m % 4 == 0 and m >= 4
    rs = np.random.RandomState(seed)
    X = np.zeros((m, d), dtype=np.float32)
    for j in range(d):
        kind = j % 3
        if kind == 0:
            col = np.r_[np.ones(m // 4), np.zeros(3 * m // 4)]
        elif kind == 1:
            col = np.r_[-np.ones(m // 4), np.ones(3 * m // 4)]
        else:
            col = np.r_[np.ones(m // 2), np.zeros(m // 2)]
        X[:, j] = rs.permutation(col)
    return X


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
