"""What tests/test_node_clustering_cpu.py and tests/test_gpu_kmeans.py share: the blob inputs, the int64 closed form of one
k-means sweep on integer tables, the float64 sweep and the derived error bands.

Blobs.  Centres RandomState(9100 + d).randint(-4, 5, (k, d)) * 4.0, redrawn until distinct: two centres differ by at least 4
in one coordinate; points = centre + uniform(-0.5, 0.5) per coordinate, cast to float32; the labels are shuffled.  A point is
within sqrt(d) / 2 of its own centre and at least 4 - 1/2 from any other along one coordinate.

Bands.  For a k-ordered float32 chain of d products the error of one score g_ic = |c|^2 / 2 - x . c is at most
(d + 2) u (|x| |c| + |c|^2 / 2), u = 2^-24; dist2 = |x|^2 + 2 g adds the chain of |x|^2 and two roundings.  All of it stays below
    band_i = 4 (d + 2) u (|x_i|^2 + max_c |c_c|^2)
which is the bound both the argmin check (the float64 distance to the device's centroid is within one band of the float64
minimum) and the dist2 check use."""
import numpy as np

U = 2.0 ** -24
BLOB_SHAPES = [(2, 3, 40), (5, 16, 60), (33, 33, 10)]          # (k, d, points per blob)
BLOB_SHAPES_GPU = BLOB_SHAPES + [(40, 128, 30), (128, 256, 5)]


def blobs(k, d, per):
    """-> (X float32 [k per, d], labels int64 [k per], first int64 [k]: the position of the first point of every blob)"""
    rs = np.random.RandomState(9100 + d)
    while True:
        centres = rs.randint(-4, 5, size=(k, d)) * 4.0
        if len(np.unique(centres, axis=0)) == k:
            break
    labels = rs.permutation(np.repeat(np.arange(k), per))
    X = (centres[labels] + rs.uniform(-0.5, 0.5, size=(k * per, d))).astype(np.float32)
    first = np.array([int(np.flatnonzero(labels == c)[0]) for c in range(k)], dtype=np.int64)
    return X, labels, first


def bad_start(labels, first):
    """``first`` with cluster k - 1 moved onto a second point of blob 0"""
    pos = first.copy()
    pos[-1] = int(np.flatnonzero(labels == 0)[1])
    return pos


def int_step(X, C):
    """One sweep on integer rows X [M, d] and integer centroids C [k, d] in int64, everything doubled where the device holds
    half-integers: argmin_c (|c|^2 - 2 x . c) with ties to the lowest c -> dict(assign, dist2, sums, counts, inertia), exact."""
    Xi, Ci = np.rint(np.asarray(X)).astype(np.int64), np.rint(np.asarray(C)).astype(np.int64)
    assert np.array_equal(Xi, np.asarray(X)) and np.array_equal(Ci, np.asarray(C))
    Xf, Cf = Xi.astype(np.float64), Ci.astype(np.float64)  # (integers far below 2^53: the float64 products are exact)
    g2 = (Ci * Ci).sum(axis=1)[None, :] - 2 * np.rint(Xf @ Cf.T).astype(np.int64)
    assign = np.argmin(g2, axis=1)  # (the first minimum: the lowest cluster)
    dist2 = np.maximum(0, (Xi * Xi).sum(axis=1) + g2[np.arange(len(Xi)), assign])
    onehot = np.zeros((len(Xi), len(Ci)))
    onehot[np.arange(len(Xi)), assign] = 1.0
    sums = np.rint(onehot.T @ Xf).astype(np.int64)
    assert np.abs(sums).max(initial=0) < 2 ** 24 and dist2.max() < 2 ** 24
    two = np.sort(g2, axis=1)[:, :2]
    ties = float(np.mean(two[:, 0] == two[:, 1])) if len(Ci) > 1 else 0.0  # the share of rows whose minimum is attained twice
    return dict(assign=assign, dist2=dist2, sums=sums, counts=np.bincount(assign, minlength=len(Ci)), inertia=int(dist2.sum()), ties=ties)


def f64_dist(X, C):
    """float64 squared distances [M, k], by differences (no cancellation)"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    out = np.empty((len(X), len(C)))
    for c in range(len(C)):
        out[:, c] = ((X - C[c]) ** 2).sum(axis=1)
    return out


def band(X, C):
    """band_i of the module text -> float64 [M]"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return 4.0 * (X.shape[1] + 2) * U * ((X * X).sum(axis=1) + (C * C).sum(axis=1).max())


def update_from_step(step, centroids):
    """fp32(sums / fp32(counts)) of a ``kmeans_step`` result, an empty cluster keeping its centroid: the update in numpy's
    correctly rounded float32 division"""
    counts = np.asarray(step["counts"])
    new = np.array(centroids, dtype=np.float32)
    full = counts > 0
    new[full] = step["sums"][full] / counts[full].astype(np.float32)[:, None]
    return new
