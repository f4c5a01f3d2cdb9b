"""What the tests of the learned link-prediction path share (tests/test_link_prediction_lr_cpu.py and
tests/test_gpu_link_prediction_lr.py): a numpy restatement of gg_edge_classifier_* (include/graphgan_hip.h) in a chosen dtype --
the four operators, loss and gradient, the Adam fit (classifier_ref.adam_fit), the logits --, a brute-force AUC, a plain-Python
restatement of the negative sampler's contract (graphgan_amd/evaluation/link_prediction_lr.py), the launch plan of
edge_sweep_kernel / edge_predict_kernel (graphgan_amd/csrc/classifier.hip) with the trip-structure sizes derived from it, and the
closed forms of the sweep's outputs on integer tables.  As in classifier_ref the float64 run is the reference of the device tests
and the float32 run of the SAME inputs gives the rounding scale a tolerance is derived from (``classifier_ref.tol``).

The model is the one-vs-rest model of classifier_ml_ref at one class on the rows x = op(E[u], E[v]): its ``lossgrad`` is used as
it is.

Exact edge accounting.  With table entries in {-1, 0, 1}, w = 0, b = 0, l2 = 0 every logit is 0 and sigmoid - y = +-1/2.
Every feature is an integer (Hadamard, L1, L2) or a multiple of 1/2 (average), so every term the sweep sums is a multiple of
1/2 (1/4) whose numerator stays below 2^24 (``headroom``): every float32 partial sum is exact IN ANY ORDER and
    gw = fp32(sum_i (1/2 - y_i) x_i) / fp32(M),   gb = fp32(M / 2 - n_1) / fp32(M)
bit for bit.  A dropped, doubled or stale edge changes an integer numerator."""
import numpy as np

from tests.support import classifier_ml_ref as ml_ref
from tests.support.classifier_ref import adam_fit, tol  # noqa: F401  (tol: for this module's users)
from tests.support.classifier_shapes import cdiv

OPERATORS = ("hadamard", "average", "l1", "l2")

# ---- the launch plan (classifier.hip: EC_LANES, EC_EDGES, EC_MAX_GRID, EC_PREDICT_GRID, edge_plan)
EC_LANES, EC_EDGES, EC_MAX_GRID, EC_PREDICT_GRID = 16, 16, 1024, 1024


def nj_of(ld):
    """float4 pieces of a row per lane: the template instance"""
    return cdiv(ld, 4 * EC_LANES)


def sweep_grid(M):
    return min(EC_MAX_GRID, cdiv(M, EC_EDGES))


def predict_grid(M):
    return min(EC_PREDICT_GRID, cdiv(M, EC_EDGES))


def trips(M, grid):
    """per workgroup the valid-edge counts of its trips (trips of 16 edges go to workgroups round robin)"""
    n_trips = cdiv(M, EC_EDGES)
    return [[min(EC_EDGES, M - EC_EDGES * t) for t in range(wg, n_trips, grid)] for wg in range(grid)]


def trip_counts(M, grid):
    """(fewest trips of a workgroup, most trips, workgroups with the most, valid edges of the last trip)"""
    n_trips = cdiv(M, EC_EDGES)
    q, r = divmod(n_trips, grid)
    return (q, q, grid, M - EC_EDGES * (n_trips - 1)) if r == 0 else (q, q + 1, r, M - EC_EDGES * (n_trips - 1))


def second_trip_single_edge(M, grid_of=sweep_grid):
    """workgroup 0 alone takes a second trip, with a single valid edge"""
    return trip_counts(M, grid_of(M)) == (1, 2, 1, 1)


def two_and_three_trips_ragged(M, grid_of=sweep_grid):
    """every workgroup takes at least two trips, some take three, the last trip is ragged"""
    lo, hi, _, last = trip_counts(M, grid_of(M))
    return lo == 2 and hi == 3 and last < EC_EDGES


def smallest(pred, hi=1 << 20):
    """the smallest M in [1, hi) with pred(M)"""
    for M in range(1, hi):
        if pred(M):
            return M
    raise AssertionError("no M below %d" % hi)


# workgroup 0 alone takes a second trip, with a single valid edge: one edge more than the full grid of full trips
M_SECOND_TRIP = EC_MAX_GRID * EC_EDGES + 1
# every workgroup takes two trips, workgroup 0 a third one with one edge -- the smallest M with two- and three-trip workgroups
# and a ragged last trip; M_THREE_TRIPS moves the edge of the third trips inside the grid: workgroups 0 .. 36 take three trips,
# the last of them with 5 edges
M_THREE_TRIPS_MIN = 2 * EC_MAX_GRID * EC_EDGES + 1
M_THREE_TRIPS = (2 * EC_MAX_GRID + 36) * EC_EDGES + 5
# edge_predict_kernel: three trips of the row loop, the last ragged (workgroups 0 .. 17; 7 edges in the last trip)
M_PREDICT = (2 * EC_PREDICT_GRID + 17) * EC_EDGES + 7


# ---- the model
def op_name(op):
    return op if isinstance(op, str) else OPERATORS[op]


def features(A, B, op, dtype=np.float64):
    """op(A, B) elementwise with every operation in ``dtype``"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    op = op_name(op)
    if op == "hadamard":
        return A * B
    if op == "average":
        return (A + B) * dtype(0.5)
    if op == "l1":
        return np.abs(A - B)
    t = A - B
    return t * t


def lossgrad(A, B, y, w, b, l2, op, dtype=np.float64):
    """(loss, gw [d], gb) of (1/M) sum [softplus(z) - y z] + (l2 / 2) |w|^2, z = w . op(A, B) + b, every operation in ``dtype``"""
    X = features(A, B, op, dtype)
    loss, gW, gb = ml_ref.lossgrad(X, np.asarray(y).reshape(-1, 1), np.asarray(w).reshape(1, -1), np.asarray([b]).reshape(1), l2, dtype)
    return loss, gW[0], gb[0]


def fit(A, B, y, iters, lr, l2, op, dtype=np.float64, w=None, b=None):
    """``classifier_ref.adam_fit`` of the loss above from zeros (or w, b) -> (w [d], b, loss [iters])"""
    X = features(A, B, op, dtype)
    W0 = None if w is None else np.asarray(w).reshape(1, -1)
    b0 = None if b is None else np.asarray([b]).reshape(1)
    W, bb, losses = adam_fit(ml_ref.lossgrad, X, np.asarray(y).reshape(-1, 1), 1, iters, lr, l2, dtype, W0, b0)
    return W[0], bb[0], losses


def logits(A, B, w, b, op, dtype=np.float64):
    return features(A, B, op, dtype) @ np.asarray(w, dtype=dtype) + dtype(b)


def auc_brute(scores, truth):
    """the share of (positive, negative) pairs with score(positive) > score(negative), a tie counting 1/2: every pair counted"""
    s, t = np.asarray(scores, dtype=np.float64), np.asarray(truth).astype(bool)
    pos, neg = s[t], s[~t]
    twice = 0
    for p in pos.tolist():
        twice += 2 * int(np.sum(p > neg)) + int(np.sum(p == neg))
    return twice / (2.0 * len(pos) * len(neg))


# ---- the negative sampler's contract, restated with sets and loops
def sample_training_pairs(train_edges, held_out_edges, n_node, seed, max_train):
    """graphgan_amd/evaluation/link_prediction_lr.py, sample_training_pairs: the same draws in the same order"""
    rs = np.random.RandomState([int(seed), 0x4C50])
    key = lambda a, b: min(a, b) * n_node + max(a, b)  # noqa: E731
    train = sorted({key(int(a), int(b)) for a, b in train_edges})
    pos = train
    if len(train) > max_train:
        pos = [train[i] for i in rs.permutation(len(train))[:max_train].tolist()]
    forbidden = set(train) | {key(int(a), int(b)) for a, b in held_out_edges}
    neg, seen = [], set()
    while len(neg) < len(pos):
        k = len(pos) - len(neg)
        a = rs.randint(0, n_node, 2 * k + 16).tolist()
        b = rs.randint(0, n_node, 2 * k + 16).tolist()
        got = 0
        for x, y in zip(a, b):
            if x == y or key(x, y) in forbidden or key(x, y) in seen:
                continue
            if got < k:  # (a round accepts its first k survivors; the later ones are not remembered)
                seen.add(key(x, y))
                neg.append(key(x, y))
                got += 1
    u = np.array([q // n_node for q in pos + neg], dtype=np.int64)
    v = np.array([q % n_node for q in pos + neg], dtype=np.int64)
    y = np.array([1] * len(pos) + [0] * len(neg), dtype=np.int64)
    return u, v, y


# ---- the exact-integer check
def int_features(A, B, op):
    """(numerators int64 [M, d], denominator) of op(A, B) on integer rows: the features are numerators / denominator exactly"""
    Ai, Bi = np.rint(A).astype(np.int64), np.rint(B).astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(Bi, B) and max(np.abs(Ai).max(), np.abs(Bi).max()) <= 1
    op = op_name(op)
    if op == "hadamard":
        return Ai * Bi, 1
    if op == "average":
        return Ai + Bi, 2
    if op == "l1":
        return np.abs(Ai - Bi), 1
    return (Ai - Bi) ** 2, 1


def headroom(num):
    """the largest numerator (in the finest unit: 1 / (2 x denominator)) any partial sum of the exact check can reach:
    max_col sum_i |x_i|, and M for the bias"""
    return int(max(np.abs(num).sum(axis=0).max(), len(num)))


def exact(A, B, y, op):
    """(gw fp32 [d], gb fp32) of the sweep at w = 0, b = 0, l2 = 0 on integer tables, from integer numerators"""
    num, den = int_features(A, B, op)
    assert headroom(num) < 2 ** 24
    sign = 1 - 2 * np.asarray(y, dtype=np.int64)  # 2 (1/2 - y)
    M = np.float32(len(num))
    num_w = (sign[:, None] * num).sum(axis=0)  # units of 1 / (2 den)
    num_b = int(sign.sum())
    gw = (num_w.astype(np.float64) / (2 * den)).astype(np.float32)
    assert np.array_equal(gw.astype(np.float64) * (2 * den), num_w)
    return gw / M, np.float32(num_b / 2.0) / M


# ---- planted link-prediction data
def planted_case(op, base, seed=0, n=40, h=16, d=16, n_test=30):
    """A graph whose edges are ALL pairs of the nodes 0 .. h - 1 (every other pair is a non-edge) and a table under which
    the features of edges and non-edges are separated for operator ``op``; the files of an evaluator under directory ``base``.
      hadamard  group rows 3 e_0 + noise, the others noise: x_0 is 9 on an edge and about 0 elsewhere
      average   x_0 of the rows +3 in the group, -3 elsewhere: the mean is 3 on an edge, 0 or -3 elsewhere
      l1, l2    group rows noise, the others 3 randn: |a - b| is about 0 on an edge and large elsewhere
    (noise: 0.01 randn).  -> dict(table fp32 [n, d], train, test, test_neg: file names, n, d, stat: the separating statistic of a
    pair as a function (A, B) -> float64 [M], larger on edges)"""
    import os
    rs = np.random.RandomState([int(seed), OPERATORS.index(op_name(op))])
    op = op_name(op)
    table = 0.01 * rs.randn(n, d)
    if op == "hadamard":
        table[:h, 0] += 3.0
        stat = lambda A, B: (A * B)[:, 0]  # noqa: E731
    elif op == "average":
        table[:h, 0] += 3.0
        table[h:, 0] -= 3.0
        stat = lambda A, B: ((A + B) * 0.5)[:, 0]  # noqa: E731
    else:
        table[h:] = 3.0 * rs.randn(n - h, d)
        stat = lambda A, B: -np.abs(A - B).sum(axis=1) if op == "l1" else -((A - B) ** 2).sum(axis=1)  # noqa: E731
    table = table.astype(np.float32)
    clique = [(a, b) for a in range(h) for b in range(a + 1, h)]
    others = [(a, b) for a in range(n) for b in range(a + 1, n) if b >= h]
    perm = rs.permutation(len(clique))
    test = [clique[i] for i in perm[:n_test]]
    train = [clique[i] for i in perm[n_test:]]
    test_neg = [others[i] for i in rs.permutation(len(others))[:n_test]]
    names = {}
    for name, edges in (("train", train), ("test", test), ("test_neg", test_neg)):
        names[name] = os.path.join(str(base), "%s_%s.txt" % (op, name))
        with open(names[name], "w") as f:  # (some edges reversed: the evaluator canonicalises)
            f.writelines("%d\t%d\n" % ((b, a) if (a + b) % 3 == 0 else (a, b)) for a, b in edges)
    return dict(names, table=table, n=n, d=d, stat=stat, clique=np.array(clique), others=np.array(others))
