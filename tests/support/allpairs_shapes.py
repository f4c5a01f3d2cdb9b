"""What tests/test_gpu_allpairs_wide.py and tests/test_allpairs_shapes_cpu.py share: a plain-Python restatement of the launch
plan of the wide all-pairs consumer (graphgan_amd/csrc/all_score.hip: bf16_shape, column_split and the lines of reduce_once
that choose all_score_reduce_bf16_x32_kernel), the case lists, tables with an exact answer, and the float64 reference.

Why these shapes.  A workgroup of the wide kernel sweeps the 32-column tiles of ONE column split; the number of splits is about
256 / row tiles, so a call with few row tiles gets 128-column splits: four tiles, which the prologue alone covers.  A row list
may repeat ids, so MANY row tiles can be asked of a SMALL table: the columns then fall into few, long splits and the sweep
recycles its four tile buffers and its ring of four bias tiles many times.

Exact answers.  Table entries are in {-1, 0, 1} with at most NNZ non-zeros per row, the bias is an integer in [-3, 3]: bf16
holds every value, every product and every fp32 partial sum is an integer far below 2^24, so every score is exact in any
summation order, `max` is exact and `argmax` is the lowest column among the maxima (numpy argmax).  The float64 product
E . E^T is exact as well.  Planted columns are copies of a source row u with a bias above every random bias: in row u they
score nnz(u) + bias, more than any column that is not a copy of u can."""
import numpy as np

NNZ = 24                       # non-zeros per row at most
BIAS_RANDOM = (-3, 1)          # random columns
BIAS_TIE, BIAS_WIN = 2, 3      # members of a tie group / single planted maxima and the raised last member of a group
U = 2.0 ** -24                 # unit roundoff of fp32


def cdiv(a, b):
    return -(-a // b)


def bf16_shape(d):
    """all_score.hip, bf16_shape: the k-steps (of 16) of the bf16 copy of the table"""
    ks_need = cdiv(d, 16)
    return 4 if ks_need <= 4 else 8 if ks_need <= 8 else 16 if ks_need <= 16 else 32


def column_split(n, row_tiles, target, max_splits=0x7FFFFFFF):
    """all_score.hip, column_split -> (splits, cols_per_split)"""
    want = max(1, min(cdiv(n, 128), cdiv(target, row_tiles), max_splits))
    cps = cdiv(cdiv(n, want), 128) * 128
    return cdiv(n, cps), cps


def wide_plan(n, n_rows, d, nw4=False):
    """reduce_once's plan for a bf16 call that takes the wide kernel (n_rows >= 512): the instance <KS, RB, NW>, the rows of a
    workgroup, the grid (splits x row_tiles) and the 32-column tiles each split sweeps.  nw4: the process runs with GG_K7_NW4"""
    assert n_rows >= 512
    KS = bf16_shape(d)
    RB, NW = (1, 8) if KS == 32 else (4, 4) if (nw4 and KS == 16) else (2, 8)
    tile_rows = 512 if KS <= 16 else 256
    assert tile_rows == 32 * RB * NW
    row_tiles = cdiv(n_rows, tile_rows)
    splits, cps = column_split(n, row_tiles, 256)
    tiles = [cdiv(min(n, (s + 1) * cps) - s * cps, 32) for s in range(splits)]
    last_cols = n - (splits - 1) * cps - (tiles[-1] - 1) * 32
    return dict(KS=KS, RB=RB, NW=NW, tile_rows=tile_rows, row_tiles=row_tiles, splits=splits, cols_per_split=cps, tiles=tiles,
                last_cols=last_cols)


def where(plan, col):
    """(split, tile of the split, column of the tile, half-wave group) of a column: lanes 0-31 of a wavefront hold tile columns
    0-3 of every eight, lanes 32-63 columns 4-7"""
    s, c = divmod(col, plan["cols_per_split"])
    return s, c // 32, c % 32, (c % 8) // 4


# ---- cases -------------------------------------------------------------------------------------------------------------------
# name -> (n, row tiles requested, single planted maxima, tie groups).  Columns are written split * cols_per_split + 32 tile + c.
N_LONG4, N_LONG1 = 3973, 1999
D_INSTANCES = (50, 128, 256, 300)       # KS = 4, 8, 16, 32: the four default instances
D_EDGES = (8, 64, 65, 257, 512)         # mostly padding; a full KS = 4; one element in a fifth k-step; ...; a full KS = 32

GEOMETRY = {
    # 4 splits of 1024 columns: 32, 32, 32, 29 tiles, the last with 5 columns
    "LONG4": dict(n=N_LONG4, row_tiles=64,
                  singles=[0 * 1024 + 32 * 4 + 0, 0 * 1024 + 32 * 5 + 5, 1 * 1024 + 32 * 6 + 2, 2 * 1024 + 32 * 7 + 7,  # tiles = 0, 1, 2, 3 mod 4
                           0 * 1024 + 32 * 13 + 30, 2 * 1024 + 32 * 18 + 9, 1 * 1024 + 32 * 31 + 31,                   # ... a second time round the ring
                           1 * 1024, 3 * 1024, N_LONG4 - 1],                       # first column of a split > 0; the last valid column
                  groups=[(0 * 1024 + 32 * 9 + 1, 0 * 1024 + 32 * 9 + 5),          # c, c + 4: the two lanes of a row
                          (1 * 1024 + 32 * 10 + 2, 1 * 1024 + 32 * 10 + 10),       # c, c + 8: two registers of one lane
                          (2 * 1024 + 32 * 5 + 3, 2 * 1024 + 32 * 22 + 0),         # a tile and a later one, the same lane
                          (2 * 1024 + 32 * 6 + 6, 2 * 1024 + 32 * 20 + 1),         # a tile and a later one, the earlier on the other lane
                          (0 * 1024 + 32 * 12 + 17, 3 * 1024 + 32 * 2 + 1),        # a split and a later one
                          (1 * 1024 + 32 * 3 + 4, 1 * 1024 + 32 * 7 + 4, 3 * 1024 + 32 * 28 + 3)]),  # three members, the last in the partial tile
    # 1 split of 63 tiles, the last with 15 columns
    "LONG1": dict(n=N_LONG1, row_tiles=256,
                  singles=[32 * 4 + 1, 32 * 5 + 6, 32 * 6 + 3, 32 * 7 + 4, 32 * 40 + 0, 32 * 57 + 31, 32 * 59 + 13, N_LONG1 - 1],
                  groups=[(32 * 9 + 1, 32 * 9 + 5), (32 * 10 + 2, 32 * 10 + 10), (32 * 5 + 3, 32 * 50 + 0), (32 * 6 + 6, 32 * 44 + 1),
                          (32 * 11 + 20, 32 * 62 + 2)]),
    # the same table, 255 full row tiles and one that holds a single row
    "LONG1_ODD": dict(n=N_LONG1, row_tiles=None, n_rows=255 * 512 + 1, like="LONG1"),
    # 1 split of 2 tiles, the last with 1 column
    "TINY33": dict(n=33, row_tiles=None, n_rows=512, singles=[], groups=[(1, 5), (2, 10), (7, 32)]),
    # 1 split of 1 tile with 5 columns; a second row tile with one row
    "TINY5": dict(n=5, row_tiles=None, n_rows=513, singles=[], groups=[(0, 4)]),
}

EXACT_CASES = ([("LONG4", d) for d in D_INSTANCES + D_EDGES] + [("LONG1", d) for d in D_INSTANCES] + [("LONG1_ODD", 256)]
               + [(name, d) for name in ("TINY33", "TINY5") for d in D_INSTANCES])
DENSE_CASES = [("LONG4", d) for d in D_INSTANCES]
NW4_CASE = ("LONG4", 256)


def n_rows_of(name, d):
    g = GEOMETRY[name]
    return g["n_rows"] if g["row_tiles"] is None else g["row_tiles"] * (512 if bf16_shape(d) <= 16 else 256)


def plan_of(name, d, nw4=False):
    return wide_plan(GEOMETRY[name]["n"], n_rows_of(name, d), d, nw4)


# ---- tables ------------------------------------------------------------------------------------------------------------------
def int_table(n, d, singles, groups, seed):
    """-> dict(E [n, d] float32 of {-1, 0, 1}, bias_a, bias_b [n] float32 integers, source {planted column: source row},
    sources [source rows in planting order]).
    Every row has m = min(d, NNZ) non-zeros at random k, one of them in the last k-step that holds data (k >= 16 ((d - 1) // 16)).
    Every single and every tie group takes a source row u of its own (not a planted column): its columns become copies of row u.  bias_a: singles BIAS_WIN, group members BIAS_TIE (a tie).  bias_b: the LAST
    member of every group raised by one (no tie: the last member wins)."""
    rs = np.random.RandomState(seed)
    m = min(d, NNZ)
    last0 = 16 * ((d - 1) // 16)
    E = np.zeros((n, d), dtype=np.float32)
    # m distinct k per row: one in the last k-step with data (key -1), then the m - 1 smallest of the other random keys
    keys = rs.rand(n, d)
    keys[np.arange(n), rs.randint(last0, d, size=n)] = -1.0
    pos = np.argsort(keys, axis=1)[:, :m]
    E[np.arange(n)[:, None], pos] = rs.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(n, m))
    bias = rs.randint(BIAS_RANDOM[0], BIAS_RANDOM[1] + 1, size=n).astype(np.float32)
    planted = set(singles) | {c for g in groups for c in g}
    assert len(planted) == len(singles) + sum(len(g) for g in groups) and all(0 <= c < n for c in planted)
    free = [int(c) for c in rs.permutation(n) if c not in planted]
    # source rows: all m non-zeros, and at most m - 2 in common with any other source row (at d = 8 many rows are equal) -- a
    # copy of ANOTHER source then scores at most m - 2 + BIAS_WIN in row u, less than u's own copies (m + BIAS_TIE at least)
    sources = []
    for _ in range(len(singles) + len(groups)):
        while np.count_nonzero(E[free[-1]]) < m or any(E[free[-1]] @ E[u] > m - 2 for u in sources):
            free.pop()
        sources.append(free.pop())
    bias_a, bias_b, source = bias.copy(), bias.copy(), {}
    for u, cols in zip(sources, [(c,) for c in singles] + [tuple(g) for g in groups]):
        for c in cols:
            E[c] = E[u]
            source[c] = u
            bias_a[c] = bias_b[c] = BIAS_WIN if len(cols) == 1 else BIAS_TIE
        if len(cols) > 1:
            bias_b[cols[-1]] = BIAS_TIE + 1
    return dict(E=E, bias_a=bias_a, bias_b=bias_b, source=source, sources=sources)


def dense_table(n, d, seed):
    """random float tables scaled so that a row's score with itself, d sigma^2 = 30 on average, stays inside the range of the
    wide kernel's reference-free sum (scores in [-80, 80]) -> (E, bias)"""
    rs = np.random.RandomState(seed)
    return (rs.randn(n, d) * np.sqrt(30.0 / d)).astype(np.float32), (rs.randn(n) * 0.1).astype(np.float32)


def bf16_round(x):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def requested_rows(n, n_rows, must, seed):
    """n_rows ids drawn with replacement from n nodes (every id repeats when n_rows > n), unsorted; the ids of `must` stand at
    the beginning (ascending), at the end (descending: the last row of the last row tile is must[0]) and across the first tile
    edge of 256 and of 512 rows"""
    rs = np.random.RandomState(seed)
    rows = rs.randint(0, n, size=n_rows).astype(np.int32)
    must = np.asarray(sorted(must), dtype=np.int32)
    k = min(len(must), n_rows // 8)
    if k:
        rows[:k] = must[:k]
        rows[n_rows - k:] = must[:k][::-1]
        for edge in (256, 512):
            if edge + k <= n_rows - k:
                rows[edge - k // 2: edge - k // 2 + k] = must[:k]
    return rows


def gram(E):
    """E . E^T in float64 (exact on integer tables: every entry is an integer below 2^53)"""
    E64 = np.asarray(E, dtype=np.float64)
    return E64 @ E64.T


def reduce_ref(G, bias, lse=True):
    """per node the float64 max, numpy argmax (lowest column among the maxima) and log-sum-exp of G + bias, and the range of
    all scores -> dict(max, argmax, lse, lo, hi)"""
    S = G + np.asarray(bias, dtype=np.float64)[None, :]
    mx = S.max(axis=1)
    out = dict(max=mx, argmax=S.argmax(axis=1).astype(np.int32), lse=None, lo=float(S.min()), hi=float(mx.max()))
    if lse:
        S -= mx[:, None]
        np.exp(S, out=S)
        out["lse"] = mx + np.log(S.sum(axis=1))
    return out


_cases = {}


def exact_case(name, d):
    """the integer table of a case with its requested rows, its plans and the float64 references of both bias vectors; made
    once per (name, d) and left unchanged"""
    if (name, d) not in _cases:
        g = GEOMETRY[name]
        geo = GEOMETRY[g.get("like", name)]
        n = g["n"]
        t = int_table(n, d, geo["singles"], geo["groups"], seed=1000 * len(name) + n + d)
        n_rows = n_rows_of(name, d)
        G = gram(t["E"])
        c = dict(t, name=name, n=n, d=d, singles=list(geo["singles"]), groups=[tuple(x) for x in geo["groups"]], n_rows=n_rows,
                 rows=requested_rows(n, n_rows, list(t["sources"]) + sorted(t["source"]), seed=n + d), plan=plan_of(name, d),
                 plan_all=wide_plan(n, n, d) if n >= 512 else None, ref_a=reduce_ref(G, t["bias_a"]), ref_b=reduce_ref(G, t["bias_b"]))
        _cases[(name, d)] = c
    return _cases[(name, d)]


def dense_case(name, d):
    """a dense float table at the geometry of a case; the float64 reference is taken on the bf16-rounded table"""
    key = (name, d, "dense")
    if key not in _cases:
        n = GEOMETRY[name]["n"]
        E, bias = dense_table(n, d, seed=77 + d)
        n_rows = n_rows_of(name, d)
        _cases[key] = dict(E=E, bias=bias, n=n, d=d, n_rows=n_rows, rows=requested_rows(n, n_rows, range(0, n, 97), seed=d),
                           plan=plan_of(name, d), ref=reduce_ref(gram(bf16_round(E)), bias))
    return _cases[key]


# ---- the log-sum-exp of the wide kernel ----------------------------------------------------------------------------------------
SCORE_RANGE, LSE_MAX = 80.0, 85.0  # the wide kernel's sum stays finite and non-zero inside: exp(+-85) is inside fp32, 1e37 / 1e-37


def in_range(ref):
    """the condition under which the wide kernel cannot raise its overflow flag (the call would silently be repeated with the
    narrow kernel): every score in [-80, 80], every row's log-sum-exp <= 85.  Then a lane's sum of at most 16 tiles terms, each
    in [e^-80, e^80], is at least e^-80 > 1.2e-38 (no underflow to 0) and at most e^85 < 3e38 (no overflow)."""
    return -SCORE_RANGE <= ref["lo"] and ref["hi"] <= SCORE_RANGE and (ref["lse"] is None or float(ref["lse"].max()) <= LSE_MAX)


def lse_bound(ref, tiles):
    """|device log-sum-exp - float64| at most, for EXACT scores x (integer tables: the accumulators hold x itself), from the
    arithmetic of all_score_reduce_bf16_x32_kernel.  u = 2^-24, X = max |x|, T = tiles of the longest split.
      term      exp2(fl(x fl(log2 e))): the constant and the product are rounded once each, so the argument is x log2 e (1 + e),
                |e| <= 2 u, and the value moves by the factor 2^(x log2 e e) = exp(x e): relative 2 X u; v_exp_f32 itself is
                accurate to one ulp = 2 u relative                                                        -> (2 X + 2) u
      lane sum  16 T positive terms added one after another in fp32                                       -> (16 T - 1) u
      rebase    s exp2(fl(-max log2 e)): one more exponential and a product                               -> (2 X + 3) u
      lanes     the two lanes of a row merge as a + b exp(m_b - m_a), |m_b - m_a| <= 2 X: an exponential
                (argument error 2 (2 X) u, one ulp), a product and a sum                                  -> (4 X + 4) u
      splits    merged on the host in float64: nothing at this scale
    All of these are relative errors of a positive sum, so together they bound the relative error e_s of sum_j exp(x_j), and the
    logarithm moves by |log(1 + e_s)| <= 1.01 e_s (e_s < 1e-3).  Last, the result is rounded to fp32: half an ulp, <= u |lse|.
    At X = 27, T = 32 this is 4.6e-5 -- the 2e-3 max |S| band of the float test is 5.4e-2."""
    X = max(abs(ref["lo"]), abs(ref["hi"]))
    e_s = U * ((2 * X + 2) + (16 * tiles - 1) + (2 * X + 3) + (4 * X + 4))
    assert e_s < 1e-3
    return 1.01 * e_s + U * float(np.abs(ref["lse"]).max())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
