"""What tests/test_gpu_topk_lists.py, tests/test_gpu_rank_lists.py and tests/test_topk_shapes_cpu.py share: a plain-Python
restatement of the launch plans of the top-K and the rank consumer (graphgan_amd/csrc/topk_score.hip, rank_score.hip), tables
whose score rows are PROGRAMMED column by column and exact in fp32 and in bf16, the float64 reference, and a model of the
per-wavefront k-lists that says which paths of wave_insert a row program drives.

Why these shapes.  A workgroup sweeps one column split; its 4 wavefronts take 32 columns each of every 128-column tile and keep
a sorted k-list per (wavefront, row).  A call with few row tiles gets 128-column splits -- 32 columns per wavefront, so a list
with k >= 32 never fills and every insertion goes into an empty list.  A row list may repeat ids: 4 096 requested rows make 128
row tiles, the columns fall into few, long splits, and a wavefront sees hundreds of columns.

Exact answers.  Every table entry is an integer with |x| <= 256 (bf16 holds it).  Program j is a function f_j(column) with
integer values in [-65280, 65535]; it owns the coordinates (j, d - 1 - j): an ordinary node c holds hi = f // 256 and
lo = f - 256 hi there, the query node q_j holds 256 and 1 there and 0 elsewhere, so row q_j of E . E^T is f_j(c) at every
ordinary column c, 0 at the other query nodes and 65537 at q_j itself.  Every product is an integer below 2^17 and every row
sum stays below 2^24, so all scores are exact in any summation order, and float64 E . E^T followed by
lexsort((col, -score)) is the reference for both precisions.

Homes.  The answer of a row is the merge of 4 x splits lists: when the best columns are spread over all of them, only the head
of each list is in the answer and a wrong entry deeper down is invisible (a shift applied to the first 128 entries only, or a
k-th score taken one place too high, passed every test written that way).  So each program has a HOME wavefront -- its query
node is the first column of it -- and `tail`, `head`, `asc` and `perm` are lowered by LOW in every other wavefront: the final
list of the home, every position of it, IS the row's answer."""
import numpy as np

from tests.support.allpairs_shapes import bf16_round, bf16_shape, cdiv, column_split

CHUNK = 4096                 # TK_CHUNK, RK_CHUNK: requested rows / queries per internal pass
MAX_K = 256                  # TK_MAX_K
PART_CAP = 256 << 20         # TK_PART_CAP
FAR = -60000                 # "far below": under every other value of a program
F_MIN, F_MAX = -65280, 65535
SELF = 256 * 256 + 1         # a query node's score with itself


# ---- plans ---------------------------------------------------------------------------------------------------------------------
def topk_plan(n, n_rows, k):
    """gg_topk_scores -> (splits, cols_per_split)"""
    chunk = min(n_rows, CHUNK)
    cap = PART_CAP // (chunk * 4 * k * 8)
    return column_split(n, cdiv(chunk, 32), 2048, cap)


def rank_plan(n, m):
    """gg_rank_scores -> (splits, cols_per_split): the same plan without the cap"""
    return column_split(n, cdiv(min(m, CHUNK), 32), 2048)


def where(cps, c):
    """(split, wavefront, index in that wavefront's sequence of columns) of column c"""
    return c // cps, (c % cps % 128) // 32, (c % cps // 128) * 32 + c % 32


def wave_columns(n, cps):
    """{(split, wavefront): its columns in the order it meets them (ascending)}; tile t of a wavefront is [32 t, 32 t + 32)"""
    c = np.arange(n)
    split, wave = c // cps, (c % cps % 128) // 32
    return {(int(s), int(w)): c[(split == s) & (wave == w)] for s in range(cdiv(n, cps)) for w in range(4)
            if np.any((split == s) & (wave == w))}


def max_cols_per_wave(n, cps):
    return max(len(v) for v in wave_columns(n, cps).values())


# ---- row programs --------------------------------------------------------------------------------------------------------------
PROGRAMS = ("tail", "head", "asc", "plateau", "const", "desc", "perm")  # a table of 2 P <= d coordinates takes the first P
HOMED = ("tail", "head", "asc", "perm")   # programs whose k best columns all lie in ONE wavefront, the program's home
LOW = 30000                               # ... because every other wavefront's values are lowered by this much
CONST = 1000
PLATEAU_TOP, PLATEAU_KTH = 5, 4   # about 100 columns score 5, about 300 score 4 -- all over the table --, the rest 0 .. 3


def k0_of(k):
    return cdiv(k, 32) * 32


def tail_kth(k):
    """the k-th value of the fill 64 (K0 + 4 - i), i = 0 .. K0 - 1"""
    return 64 * (k0_of(k) + 4 - (k - 1))


def entrant_lane(t):
    """where in tile t the single entrant of `tail` / `head` sits (it moves over the lanes of the half-wave)"""
    return (7 * t + 3) % 32


def homes(n, cps, P):
    """the home wavefront (split, wavefront) of each program: distinct, in a complete split behind the first.  The query node of
    a program is the FIRST column of its home, so the list of that wavefront opens with the node's score with itself."""
    full = n // cps
    assert full >= 2
    h = [(1 + j % (full - 1), (j + 1) % 4) for j in range(P)]
    assert len(set(h)) == P
    return h


def program(name, n, cps, k, seed, home):
    """f(column) of one program, [n] int64, for the plan cols_per_split = cps and the list length k.  Per wavefront: i is the
    index in its sequence, t = i // 32 its tile, K0 = k rounded up to 32.  A homed program is lowered by LOW outside its home:
    what one wavefront's list holds at the end -- every position of it -- is then the answer of the whole row."""
    rs = np.random.RandomState(seed)
    c = np.arange(n, dtype=np.int64)
    waves = wave_columns(n, cps)
    if name == "asc":          # every tile's 32 candidates beat the whole list (all but the node itself at its head)
        f = c.copy()
    elif name == "desc":       # nothing enters after the fill
        f = -c
    elif name == "const":      # every tile passes x >= tau and nothing enters
        f = np.full(n, CONST, dtype=np.int64)
    elif name == "perm":
        f = 1 + rs.permutation(n).astype(np.int64)
    elif name == "plateau":    # more than k columns share the k-th score, across wavefronts and splits
        f = rs.randint(0, PLATEAU_KTH, size=n).astype(np.int64)
        pick = rs.permutation(n)
        f[pick[:300]] = PLATEAU_KTH
        f[pick[300:400]] = PLATEAU_TOP
    else:
        assert name in ("tail", "head")
        K0 = k0_of(k)
        f = np.full(n, FAR + LOW, dtype=np.int64)
        for seq in waves.values():
            i = np.arange(len(seq))
            fill = i < K0
            f[seq[fill]] = 64 * (K0 + 4 - i[fill])
            for t in range(K0 // 32, cdiv(len(seq), 32)):
                tile = seq[32 * t:32 * t + 32]
                step = 1 + (t - K0 // 32)
                # tail: above the k-th, below the (k - 1)-th value (64 apart): it lands at k - 1 and evicts the entrant before it
                # head: above every value of the fill and above the entrant before it: it lands in front of them all
                assert step < 64
                f[tile[entrant_lane(t) % len(tile)]] = (tail_kth(k) if name == "tail" else 64 * (K0 + 4)) + step
    if name in HOMED:
        assert len(waves[home]) >= k and np.sort(f[waves[home]])[-k] > 0   # the k best of the home beat the other query nodes' 0
        out = np.ones(n, dtype=bool)
        out[waves[home]] = False
        f[out] -= LOW
    return f


def programmed_table(n, d, cps, k, seed):
    """-> dict(E [n, d] float32, names, F [P, n] int64 the programs (valid at the ordinary columns), home, qid [P] the query nodes)"""
    names = PROGRAMS[:min(len(PROGRAMS), d // 2)]
    P = len(names)
    assert 2 * P <= d and P <= 32
    home = homes(n, cps, P)
    qid = np.array([s * cps + 32 * w for s, w in home], dtype=np.int32)
    assert all(where(cps, int(q)) == (s, w, 0) for q, (s, w) in zip(qid, home))
    F = np.stack([program(name, n, cps, k, seed + 17 * j, home[j]) for j, name in enumerate(names)])
    assert F.min() >= F_MIN and F.max() <= F_MAX
    hi = F // 256
    lo = F - 256 * hi
    assert np.abs(hi).max() <= 256 and lo.min() >= 0 and lo.max() <= 255
    E = np.zeros((n, d), dtype=np.float32)
    for j in range(P):
        E[:, j], E[:, d - 1 - j] = hi[j], lo[j]
    E[qid] = 0.0
    for j in range(P):
        E[qid[j], j], E[qid[j], d - 1 - j] = 256.0, 1.0
    return dict(E=E, names=names, F=F, home=home, qid=qid)


def gram_rows(E, ids):
    """rows `ids` of E . E^T in float64 (exact: every entry is an integer below 2^53); + 0.0 turns a -0.0 into +0.0, the zero
    the fp32 chain from +0.0 ends at"""
    E64 = np.asarray(E, dtype=np.float64)
    return E64[np.asarray(ids)] @ E64.T + 0.0


# ---- reference -----------------------------------------------------------------------------------------------------------------
def ref_topk(s, k, elig=None):
    """the k best columns of the score row s by (score descending, column ascending), eligible ones only; -1 / -inf padded"""
    cols = np.arange(len(s)) if elig is None else np.flatnonzero(elig)
    o = np.lexsort((cols, -s[cols]))[:k]
    col, score = np.full(k, -1, dtype=np.int32), np.full(k, -np.inf, dtype=np.float32)
    col[:len(o)], score[:len(o)] = cols[o], s[cols[o]]
    return col, score


def ref_rank(s, v, elig=None):
    """the definition: rank = 1 + the candidates c != v ahead of v, candidates = the eligible columns and always v
    -> (rank, n_cand, score)"""
    cand = np.ones(len(s), dtype=bool) if elig is None else np.array(elig, dtype=bool)
    cand[v] = True
    ahead = (s > s[v]) | ((s == s[v]) & (np.arange(len(s)) < v))
    return 1 + int((ahead & cand).sum()), int(cand.sum()), np.float32(s[v])


def eligibility(n, u, nbrs):
    """exclude = True: every column but u and its neighbours"""
    e = np.ones(n, dtype=bool)
    e[u] = False
    if len(nbrs):
        e[np.asarray(sorted(nbrs))] = False
    return e


# ---- model of the consumer -----------------------------------------------------------------------------------------------------
def model_topk(s, cps, k, elig=None):
    """The per-wavefront lists and the merge of topk_score.hip on one score row s, in plain Python.  Per wavefront and 32-column
    tile: the columns with score >= tau pass (tau: the list's k-th score, -inf until it is full), the eligible ones are merged
    into the list, the best k stay.  Then the lists are merged in (split, wavefront) order; a list whose head does not beat the
    running k-th key is skipped.  A key is (-score, column): smaller is better.
    -> (col, score, events): events[(split, wavefront)] is a list with one dict per tile
       full      the list held k entries before the tile
       passed    columns with score >= tau;  cands: the eligible ones among them
       pos       positions at which candidates entered the list
       moved     surviving entries that changed their 64-entry block
       shift     the largest shift of a surviving entry
    and events["merge"] = dict(merged, skipped)."""
    n = len(s)
    events, lists = {}, []
    for key, seq in sorted(wave_columns(n, cps).items()):
        L, ev = [], []
        for t in range(cdiv(len(seq), 32)):
            tile = seq[32 * t:32 * t + 32]
            full = len(L) == k
            tau = -L[k - 1][0] if full else -np.inf
            passed = tile[s[tile] >= tau]
            cands = passed if elig is None else passed[elig[passed]]
            e = dict(k=k, full=full, passed=len(passed), cands=len(cands), pos=[], moved=0, shift=0)
            if len(cands):
                new = sorted(L + [(-s[c], int(c)) for c in cands])[:k]
                newpos = {x: p for p, x in enumerate(new)}
                mine = {int(c) for c in cands}
                e["pos"] = [p for p, x in enumerate(new) if x[1] in mine]
                for p, x in enumerate(L):
                    if x in newpos:
                        e["shift"] = max(e["shift"], newpos[x] - p)
                        e["moved"] += (newpos[x] // 64) != (p // 64)
                L = new
            ev.append(e)
        events[key] = ev
        lists.append(L)
    cur, merged, skipped = [], 0, 0
    for L in lists:
        if not L or (len(cur) == k and L[0] >= cur[k - 1]):
            skipped += 1
            continue
        cur = sorted(cur + L)[:k]
        merged += 1
    events["merge"] = dict(merged=merged, skipped=skipped)
    col, score = np.full(k, -1, dtype=np.int32), np.full(k, -np.inf, dtype=np.float32)
    col[:len(cur)], score[:len(cur)] = [x[1] for x in cur], [-x[0] for x in cur]
    return col, score, events


def totals(events):
    """the event counts of a row over all wavefronts"""
    tiles = [e for key, ev in events.items() if key != "merge" for e in ev]
    return dict(full_insertions=sum(1 for e in tiles if e["full"] and e["pos"]),
                moved_between_blocks=sum(e["moved"] for e in tiles),
                entrants_at_0=sum(1 for e in tiles if e["full"] and 0 in e["pos"]),
                entrants_at_last=sum(1 for e in tiles if e["full"] and e["pos"] and e["pos"][-1] == e["k"] - 1),
                passed_nothing_entered=sum(1 for e in tiles if e["full"] and e["passed"] and not e["pos"]),
                largest_shift=max([e["shift"] for e in tiles] + [0]))


# ---- cases ---------------------------------------------------------------------------------------------------------------------
N_ROWS = 4096
N_LONG, D_LONG, K_LONG = 24576, 50, 256
KS_LONG = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
N_INST, KS_INST, DS_INST = 9000, (65, 255), (8, 128, 256, 300, 380, 384, 512)
EXCLUDE_KS = (65, 256)
INSTANCE_CASES = [(N_INST, d, k) for k in KS_INST for d in DS_INST]
LONG_CASES = [(N_LONG, D_LONG, k) for k in KS_LONG]   # one table per k: its programs are written for the plan of that k
RANK_CASES = [(N_LONG, 50, K_LONG), (N_INST, 256, 255), (N_INST, 300, 255), (N_INST, 512, 255)]

_cases = {}


def case(n, d, k):
    """the programmed table for the plan of (n, 4 096 rows, k) with the requested rows -- the query nodes and a few ordinary
    nodes, drawn with repeats, unsorted -- and the float64 score row of every distinct id; made once, left unchanged.
    q: {program: its query node}, prog: {program: its index}, ordinary: [n] bool"""
    if (n, d, k) not in _cases:
        splits, cps = topk_plan(n, N_ROWS, k)
        t = programmed_table(n, d, cps, k, seed=n + 31 * d + k)
        P = len(t["names"])
        ordinary = np.ones(n, dtype=bool)
        ordinary[t["qid"]] = False
        ids = np.array(t["qid"].tolist() + [1, n // 2 + 1, n - 1], dtype=np.int32)
        assert len(set(ids.tolist())) == P + 3
        rs = np.random.RandomState(n + d + k)
        rows = ids[rs.randint(0, len(ids), size=N_ROWS)]
        rows[:len(ids)] = ids[::-1]
        S = dict(zip(ids.tolist(), gram_rows(t["E"], ids)))
        _cases[(n, d, k)] = dict(t, n=n, d=d, k=k, P=P, splits=splits, cps=cps, ids=ids, rows=rows, S=S, ordinary=ordinary,
                                 q={name: int(t["qid"][j]) for j, name in enumerate(t["names"])},
                                 prog={name: j for j, name in enumerate(t["names"])})
    return _cases[(n, d, k)]


def exclusion_edges(c):
    """a graph on a case's table: q_asc is linked to every other one of the last 600 columns of its home wavefront -- the best
    ones of its row --, q_plateau to every other member of its two plateaus (the columns that share the k-th score, at
    k <= 100 and above) -> [E, 2] int32"""
    q, prog = c["q"], c["prog"]
    best = wave_columns(c["n"], c["cps"])[c["home"][prog["asc"]]][-600:]
    plateau = np.flatnonzero((c["F"][prog["plateau"]] >= PLATEAU_KTH) & c["ordinary"])
    edges = [(q["asc"], int(v)) for v in best[1::2]] + [(q["plateau"], int(v)) for v in plateau[::2]]
    return np.array(edges, dtype=np.int32)


def neighbour_sets(n, edges):
    nb = [set() for _ in range(n)]
    for a, b in np.asarray(edges).tolist():
        nb[a].add(b)
        nb[b].add(a)
    return nb


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
