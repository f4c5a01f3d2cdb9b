"""What tests/test_gpu_classifier_shapes.py and tests/test_classifier_shapes_cpu.py share: a plain-Python restatement of the
sweep's launch plan (graphgan_amd/csrc/row_tiles.h, row_tile_plan), the case lists, integer tables with the closed forms of the
sweep's outputs at W = 0, b = 0, l2 = 0, and label generators.

Exact row accounting.  With table entries in {-1, 0, 1} and zero parameters every logit is 0: softmax gives p = 1 / C per class
(exact in float32 when C is a power of two), the sigmoid 1 / 2.  Every term the sweep sums is then a multiple of 1 / C (1 / 2)
whose numerator stays below 2^24 (``headroom``), so every float32 partial sum is exact IN ANY ORDER, and the outputs are one
correctly rounded division away from integers:
    softmax:  gb[c] = fp32(M / C - n_c) / fp32(M),   gW[c] = fp32(S / C - S_c) / fp32(M)
    sigmoid:  gb[c] = fp32(M / 2 - n_c) / fp32(M),   gW[c] = fp32(S / 2 - S_c) / fp32(M)
(S = sum of the gathered rows, S_c = the sum over the rows that carry class c, n_c their count).  A dropped or doubled row, a
tile read from stale LDS or a partial summed twice changes an integer numerator and with it the bits."""
import numpy as np

NC_RT, NC_MAX_GRID, NC_LDS = 64, 512, 150 * 1024  # rows per tile, workgroups at most, dynamic LDS at most (row_tiles.h)
N_TABLE = 5000


def cdiv(a, b):
    return -(-a // b)


def ld_of(d):
    """the row stride of the resident tables: d rounded up to a multiple of 4"""
    return cdiv(d, 4) * 4


def sweep_plan(C, ld):
    """row_tiles.h's row_tile_plan for C classes at row stride ld -> dict(CT, DT, KW, chunks, lds): the template instance, the
    k-chunk of the W staging (== ld: W is staged once per workgroup), the column counts of the chunks, the dynamic LDS bytes"""
    CT, DT = cdiv(C, 32), cdiv(ld, 32)
    fixed = 4 * NC_RT * ((32 * DT + 1) + (32 * CT + 1))
    KW = (NC_LDS - fixed) // (4 * 32 * CT) - 1
    KW = ld if KW >= ld else KW // 4 * 4
    chunks = [min(KW, ld - k0) for k0 in range(0, ld, KW)]
    return dict(CT=CT, DT=DT, KW=KW, chunks=chunks, lds=fixed + 4 * 32 * CT * (KW + 1))


def grid_of(M):
    return min(NC_MAX_GRID, cdiv(M, NC_RT))


# the (CT, DT) instances whose W does not fit beside the tile at ld = 32 DT: staged per tile in k-chunks
CHUNKED = {(4, 5), (4, 6), (4, 7), (4, 8), (3, 7), (3, 8)}

# every (CT, DT) instance at full tiles, three row tiles (the last with 2 rows)
M_SMALL = 130
INSTANCE_CASES = [(C, d) for C in (32, 64, 96, 128) for d in (32, 64, 96, 128, 160, 192, 224, 256)]
# just over a tile edge in C, in d or in both; d = 1 and d = 3 are padded to ld = 4
RAGGED_CASES = [(33, 33), (65, 97), (97, 129), (96, 225), (127, 161), (128, 193), (3, 1), (2, 3)]
# more tiles than workgroups: 513 tiles (workgroup 0 takes a second tile, with one valid row); 1062 tiles (workgroups 0 .. 37
# take three tiles, the others two; the last tile has 5 rows)
M1, M2 = 32769, 67909
MULTI_TILE_SHAPES = [(8, 2), (50, 40), (224, 96), (160, 128), (256, 128)]  # (d, C); the last three are chunked
MULTI_TILE_CASES = [(M, d, C) for M in (M1, M2) for d, C in MULTI_TILE_SHAPES]
PREDICT_CASES = [(128, 128), (96, 256), (128, 256)]  # (C, d): 66, 99 and 132 KiB of W in LDS
M_PREDICT = 9001  # 1024 workgroups of 4 rows: three trips of the row loop, the last with 809 rows


def is_pow2(C):
    return C & (C - 1) == 0


def int_tables(d):
    """two tables [N_TABLE, d] with entries in {-1, 0, 1}"""
    rs = np.random.RandomState(7000 + d)
    return rs.randint(-1, 2, size=(N_TABLE, d)).astype(np.float32), rs.randint(-1, 2, size=(N_TABLE, d)).astype(np.float32)


def draw_nodes(rs, M):
    """node ids with replacement, one id three times"""
    nodes = rs.randint(0, N_TABLE, size=M)
    if M > 2:
        nodes[M // 2] = nodes[0]
        nodes[-1] = nodes[0]
    return nodes


def draw_labels(rs, M, C):
    """one class per row; class C - 1 has no row"""
    return rs.randint(0, C - 1, size=M) if C > 2 else np.zeros(M, dtype=np.int64)


def draw_label_sets(rs, M, C):
    """bool [M, C]: 0 - 3 labels per row (rows without a label occur), row 1 with every label, row 2 with none; class C - 1 is
    carried by row 1 alone"""
    Y = np.zeros((M, C), dtype=bool)
    n = rs.randint(0, 4, size=M)
    cols = rs.randint(0, max(C - 1, 1), size=(M, 3))
    for j in range(3):
        rows = np.flatnonzero(n > j)
        Y[rows, cols[rows, j]] = True
    if M > 2:
        Y[1] = True
        Y[2] = False
    return Y


def headroom(X, C):
    """the largest numerator (in units of 1 / C) any partial sum of the exact check can reach: max_col sum_i |x_i| (C - 1), and
    M (C - 1) for the bias"""
    X = np.asarray(X)
    return int(max(np.abs(X).sum(axis=0).max(), len(X))) * (C - 1)


def _exact(X, onehot, den):
    """fp32(S / den - S_c) / fp32(M) and fp32(M / den - n_c) / fp32(M) from integer numerators"""
    Xi = np.rint(np.asarray(X)).astype(np.int64)
    assert np.array_equal(Xi, np.asarray(X)) and np.abs(Xi).max() <= 1
    H = np.asarray(onehot).astype(np.float64)
    M = np.float32(len(Xi))
    S_c = np.rint(H.T @ Xi.astype(np.float64)).astype(np.int64)  # (integers below 2^53: the float64 product is exact)
    num_w = Xi.sum(axis=0)[None, :] - den * S_c  # units of 1 / den
    num_b = len(Xi) - den * np.asarray(onehot).astype(np.int64).sum(axis=0)
    assert max(int(np.abs(num_w).max()), int(np.abs(num_b).max())) < 2 ** 24
    gW = (num_w.astype(np.float64) / den).astype(np.float32)
    gb = (num_b.astype(np.float64) / den).astype(np.float32)
    assert np.array_equal(gW.astype(np.float64) * den, num_w) and np.array_equal(gb.astype(np.float64) * den, num_b)
    return gW / M, gb / M


def exact_softmax(X, y, C):
    """(gW, gb) of the softmax sweep at W = 0, b = 0, l2 = 0 on an integer table; C a power of two"""
    assert is_pow2(C)
    onehot = np.zeros((len(y), C), dtype=bool)
    onehot[np.arange(len(y)), y] = True
    return _exact(X, onehot, C)


def exact_sigmoid(X, Y):
    """(gW, gb) of the one-vs-rest sweep at W = 0, b = 0, l2 = 0 on an integer table; any C"""
    return _exact(X, Y, 2)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

