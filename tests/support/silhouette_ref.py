"""References for the silhouette tests (include/graphgan_hip.h, gg_silhouette): a float64 restatement of the definition with its
tie rule, the fp32 closed form of the stated operation sequence on tables whose distances are integers, those tables, and the
error band of the fp32 / bf16 device result against float64, derived from the inputs."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32


def brute_force(X, assign, k):
    """the definition, one pair at a time (python floats): dict(sil, a, b, nearest, mean)"""
    X = [[float(v) for v in row] for row in np.asarray(X, dtype=np.float64)]
    assign = [int(c) for c in assign]
    m = len(X)
    n = [sum(1 for c in assign if c == cc) for cc in range(k)]
    sil, a, b, near = [], [], [], []
    for i in range(m):
        S = [0.0] * k
        for j in range(m):
            if j != i:
                S[assign[j]] += sum((x - y) ** 2 for x, y in zip(X[i], X[j])) ** 0.5
        ci = assign[i]
        ai = S[ci] / (n[ci] - 1) if n[ci] > 1 else 0.0
        bi, bc = None, -1
        for c in range(k):
            if c != ci and n[c] > 0 and (bi is None or S[c] / n[c] < bi):  # strict: ties to the lowest cluster
                bi, bc = S[c] / n[c], c
        den = max(ai, bi)
        sil.append(0.0 if n[ci] == 1 or den == 0.0 else (bi - ai) / den)
        a.append(ai), b.append(bi), near.append(bc)
    return dict(sil=np.array(sil), a=np.array(a), b=np.array(b), nearest=np.array(near, dtype=np.int64), mean=sum(sil) / m)


def _finish(S, assign, counts, own_rows, dtype):
    """(a, b, nearest, sil) from the sums S [rows, k] of the rows with clusters ``own_rows`` in ``dtype`` arithmetic"""
    r = np.arange(len(S))
    n_own = counts[own_rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(n_own > 1, S[r, own_rows].astype(dtype) / np.maximum(n_own - 1, 1).astype(dtype), dtype(0)).astype(dtype)
        means = np.where(counts[None, :] > 0, S.astype(dtype) / np.maximum(counts, 1).astype(dtype)[None, :], dtype(np.inf)).astype(dtype)
    means[r, own_rows] = np.inf
    nearest = np.argmin(means, axis=1)  # the first minimum: ties to the lowest cluster
    b = means[r, nearest].astype(dtype)
    den = np.maximum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        sil = np.where((n_own > 1) & (den > 0), ((b - a).astype(dtype) / den).astype(dtype), dtype(0)).astype(dtype)
    return a, b, nearest, sil


def float64_ref(X, assign, k, rows=None):
    """the definition in float64 with whole matrices (test sizes): dict(sil, a, b, nearest, mean, dist [rows, m], means [rows, k])"""
    X, assign = np.asarray(X, dtype=np.float64), np.asarray(assign).astype(np.int64)
    m = len(X)
    pos = np.arange(m) if rows is None else np.asarray(rows).astype(np.int64)
    counts = np.bincount(assign, minlength=k)
    diff = X[pos][:, None, :] - X[None, :, :] if m * len(pos) * X.shape[1] <= 1 << 24 else None
    if diff is not None:
        d = np.sqrt((diff * diff).sum(axis=2))
    else:
        h = (X * X).sum(axis=1)
        d = np.sqrt(np.maximum(0.0, h[pos][:, None] + h[None, :] - 2.0 * X[pos] @ X.T))
    d[np.arange(len(pos)), pos] = 0.0
    onehot = np.zeros((m, k))
    onehot[np.arange(m), assign] = 1.0
    S = d @ onehot
    a, b, nearest, sil = _finish(S, assign, counts, assign[pos], np.float64)
    means = np.where(counts[None, :] > 0, S / np.maximum(counts, 1)[None, :], np.inf)
    return dict(sil=sil, a=a, b=b, nearest=nearest, mean=float(sil.sum() / len(pos)), dist=d, means=means, counts=counts)


# ---- tables on which every distance is an integer
def exact_coords(d, q):
    """q^2 coordinates spread over the whole width d (every 32-wide k-chunk of a wide table gets some)"""
    assert q * q <= d
    return (np.arange(q * q) * d) // (q * q)


def exact_table(t, d, q):
    """row i = t_i on the q^2 coordinates of exact_coords, 0 elsewhere: |x_i - x_j| = q |t_i - t_j|; t in [0, 64) is exact in bf16"""
    t = np.asarray(t)
    assert t.min() >= 0 and t.max() < 64
    X = np.zeros((len(t), d), dtype=np.float32)
    X[:, exact_coords(d, q)] = t[:, None].astype(np.float32)
    return X


def fp32_closed_form(t, q, assign, k, rows=None):
    """The stated fp32 operation sequence on an exact table: every distance q |t_i - t_j| and every sum is an integer below 2^24
    (asserted), exact in fp32 in any order; then a = S / (float)(n - 1), b = min S / (float)n, sil = (b - a) / fmaxf(a, b), each ONE
    correctly rounded fp32 operation."""
    t, assign = np.asarray(t).astype(np.int64), np.asarray(assign).astype(np.int64)
    m = len(t)
    pos = np.arange(m) if rows is None else np.asarray(rows).astype(np.int64)
    counts = np.bincount(assign, minlength=k)
    d = q * np.abs(t[pos][:, None] - t[None, :])
    d[np.arange(len(pos)), pos] = 0
    onehot = np.zeros((m, k), dtype=np.int64)
    onehot[np.arange(m), assign] = 1
    S = d @ onehot
    assert S.max() < 1 << 24
    a, b, nearest, sil = _finish(S.astype(np.float32), assign, counts, assign[pos], np.float32)
    return dict(sil=sil, a=a, b=b, nearest=nearest.astype(np.int32), mean=float(sil.astype(np.float64).sum() / len(pos)))


# ---- bf16 rounding and the derived band
def round_bf16(X):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32"""
    bits = np.ascontiguousarray(X, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(np.shape(X))


def band(ref, X, assign, k, ld, rows=None):
    """Tolerances of the device's fp32 results against ``ref = float64_ref(X, ...)`` (X: the table the device multiplies -- the
    bf16-rounded one for bf16), derived from the inputs.  With u = 2^-24 and ld the padded width of the dot products:
      d^2:   h_i, h_j and s_ij are ld-term fp32 sums of products bounded (Cauchy-Schwarz) by h_i, h_j, (h_i + h_j) / 2, and the
             add, the doubling-and-subtract round once each:  |D(d^2)| <= e2 = 2 (ld + 3) u (h_i + h_j)
      d:     |sqrt(x + e) - sqrt(x)| <= min(sqrt(e), e / sqrt(x)), plus the square root's own rounding u d
      S_ic:  the sum of the term errors plus an n_c-term fp32 sum in any order, n_c u S (1 + n_c u)
      mean:  divided by the count, plus the division's rounding u |mean|
      b:     |min f - min g| <= max |f - g| over the clusters
      sil:   (b - a) / M, M = max(a, b):  (Da + Db) (1 + |sil|) / (M - Da - Db) + 3 u  (subtraction, division)
    -> dict(a, b, sil [rows], mean, gap [rows]: how far, in units of the band, the second-nearest cluster is behind the nearest)"""
    X, assign = np.asarray(X, dtype=np.float64), np.asarray(assign).astype(np.int64)
    m = len(X)
    pos = np.arange(m) if rows is None else np.asarray(rows).astype(np.int64)
    counts, d = ref["counts"], ref["dist"]
    h = (X * X).sum(axis=1)
    e2 = 2.0 * (ld + 3) * U * (h[pos][:, None] + h[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        ed = np.minimum(np.sqrt(e2), np.where(d > 0, e2 / d, np.inf)) + U * (d + np.sqrt(e2))
    ed[np.arange(len(pos)), pos] = 0.0
    onehot = np.zeros((m, k))
    onehot[np.arange(m), assign] = 1.0
    S = d @ onehot
    nc = counts[None, :].astype(np.float64)
    eS = ed @ onehot + nc * U * (S + ed @ onehot) * (1.0 + nc * U)
    r, own = np.arange(len(pos)), assign[pos]
    n_own = counts[own]
    ea = np.where(n_own > 1, eS[r, own] / np.maximum(n_own - 1, 1), 0.0) + U * ref["a"]
    emeans = np.where(counts[None, :] > 0, eS / np.maximum(counts, 1)[None, :], 0.0) + U * np.where(np.isfinite(ref["means"]), ref["means"], 0.0)
    emeans[r, own] = 0.0
    eb = emeans.max(axis=1)
    M = np.maximum(ref["a"], ref["b"])
    esil = np.where(n_own > 1, (ea + eb) * (1.0 + np.abs(ref["sil"])) / np.maximum(M - ea - eb, 1e-300) + 3.0 * U, 0.0)
    others = ref["means"].copy()
    others[r, own] = np.inf
    others[r, ref["nearest"]] = np.inf
    second = others.min(axis=1)
    gap = np.where(np.isfinite(second), (second - ref["b"]) / np.maximum(2.0 * eb, 1e-300), np.inf)
    return dict(a=ea, b=eb, sil=esil, mean=float(esil.sum() / len(pos)) + 2.0 * U, gap=gap)
