"""Cases of the distribution-cache matrix (tests/test_gpu_dist_cache.py) and the CPU side of every one of them: graphs,
generator tables, call sequences, the C oracle's expected arrays, and -- for the cases that need a lazy slot to be rebuilt
whole in a chosen launch -- the preconditions on the oracle's own walks (tests/test_dist_cache_cases_cpu.py).

Nothing here touches the engine.  Walks are counter based (spec S4: Philox keyed by seed, stream, root id, walk, hop), so which
walk stands on which node is a fact of (graph, tables, seed, stream) alone and can be chosen, and asserted, without a GPU.

THE LAZY GRAPH.  One graph of BFS-numbered regular trees serves every lazy case; a case picks its roots.  A regular tree has a
root with M children and C children per node on levels 1-3; level 4 holds leaves, except the "hot" nodes, which have two
children of their own.  With the node limit CAP the engine's build rule (a level is expanded while nodes so far + adjacency
entries of the level fit the limit) makes such a tree exact through level L = 2: ranks [0, LZS) have built lists, ranks
[LZS, P) are level 2, and every rank from P on is a pool rank handed out in resolution order.  Levels 3 and 4 are resolved by
the walks; a walk standing on a hot node asks for the slot's whole tree.  Every level-2 and level-3 node has a father and C
children, so k = C + 1 for all of them: in the rebuilt whole tree, where the ranks from P on name the level-3 nodes in BFS
order, any stale (slot, rank, has-father) key of the distribution cache matches on k.

The biases steer the walks (scores are E[cur].E[v] + b[v]; the rows of E are small noise): most walks go root -> A1 (the SECOND
level-1 node) -> B (its second child) -> one of B's children X0, X1 -> a leaf; a few go root -> A0 -> F0 (the FIRST level-2
node) -> one of its children Y0, Y1.  In the lazy tree B's list is the first one resolved, so X_i gets pool rank P + i; in the
whole tree rank P + i is Y_i.  X1 prefers its second child, Y1 its first: a walk on Y1 that samples from X1's prefix sums takes
another child than the oracle's walk.  What differs between the tree kinds is the first child of X1:
  "target": hot, with a small probability -- the few D-mode walks (deg(root) = M) miss it, the G-mode walks (n_sample) find it;
  "loud":   hot, with a large probability -- the D-mode walks find it;
  "quiet":  a leaf -- the slot stays lazy whatever is asked.
"""
import ctypes

import numpy as np

from oracle import graphgan_oracle as orc

M, C = 12, 2          # children of the root / of every node on levels 1-3
CAP = 64              # set_tree_mode(1, CAP): 1 + 12 + 12 * 3 = 49 fits, 37 + 24 * 3 = 109 does not: exact through level 2
L_EXACT = 2
LZS = 1 + M           # ranks with built children lists (levels 0, 1)
P_EXACT = 1 + M + M * C   # first pool rank
D_LAZY = 8
N_SAMPLE_LAZY = 300
SEED_LAZY = 65        # the first seed at which check_target holds for both target trees (scanned on the CPU; asserted by the CPU test)
KINDS = ("target", "target", "quiet", "loud")   # trees of the lazy graph, in node order; then a pair and an isolated node


# ------------------------------------------------------------------------------------------------ graphs
def csr_from_edges(n, edges):
    """Symmetric CSR with sorted adjacency lists from undirected edges (u, v), u != v, no duplicates."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    u = np.concatenate([e[:, 0], e[:, 1]])
    v = np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((v, u))
    u, v = u[order], v[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, u + 1, 1)
    return np.cumsum(rowptr), v.astype(np.int32)


def bfs_levels(n, rowptr, col, root):
    """(level [n] with -1 outside the component, father [n], order) of the FIFO BFS in adjacency order (construct_trees)."""
    level = np.full(n, -1, dtype=np.int64)
    father = np.full(n, -1, dtype=np.int64)
    level[root] = 0
    father[root] = root
    queue = [int(root)]
    for cur in queue:
        for w in col[rowptr[cur]: rowptr[cur + 1]]:
            if level[w] < 0:
                level[w] = level[cur] + 1
                father[w] = cur
                queue.append(int(w))
    return level, father, np.array(queue, dtype=np.int64)


def predicted_exact_level(rowptr, level, order, cap):
    """The engine's build rule for a lazy slot (bfs_gpu.hip): level `depth` >= 1 is expanded only while (nodes through that
    level) + (adjacency entries of its nodes) <= cap.  Returns (L, lzs, P): the level the exact part ends with, the ranks
    with built lists, the first pool rank."""
    deg = rowptr[1:] - rowptr[:-1]
    lv = level[order]
    depth = 1
    while True:
        tail = int((lv <= depth).sum())
        D = int(deg[order[lv == depth]].sum())
        if tail + D > cap or not (lv == depth + 1).any():
            return depth, int((lv < depth).sum()), tail
        depth += 1


def _regular_tree(base, hot):
    """Edges of one tree with BFS-ordered ids from `base`: returns (edges, levels, next id); `hot` = indices into level 4."""
    levels = [np.array([base])]
    nxt = base + 1
    edges = []
    for width in (M, C, C, C):
        parents = levels[-1]
        kids = nxt + np.arange(len(parents) * width)
        edges += list(zip(np.repeat(parents, width), kids))
        levels.append(kids)
        nxt += len(kids)
    hot_nodes = levels[4][list(hot)]
    kids = nxt + np.arange(2 * len(hot_nodes))
    edges += list(zip(np.repeat(hot_nodes, 2), kids))
    levels.append(kids)
    nxt += len(kids)
    return edges, levels, int(nxt)


_LAZY = None


def lazy_graph():
    """The lazy graph: dict(n, rowptr, col, E, b, trees=[dict(kind, root, levels, A0, A1, F0, B, X, Y, Z)], pair_root, iso)."""
    global _LAZY
    if _LAZY is not None:
        return _LAZY
    edges, trees, nxt = [], [], 0
    # indices within a level (C = 2): level 2: A_i's children are 2 i, 2 i + 1 -> F0 = 0, B = 3; level 3: F0's children Y0, Y1 = 0, 1,
    # B's children X0, X1 = 6, 7; level 4: Y1's children are 2, 3, X1's children are 14, 15
    for kind in KINDS:
        hot = () if kind == "quiet" else (14,)
        e, lv, end = _regular_tree(nxt, hot)
        edges += e
        A0, A1 = int(lv[1][0]), int(lv[1][1])
        F0, B = int(lv[2][0]), int(lv[2][3])
        X, Y = lv[3][6:8].copy(), lv[3][0:2].copy()
        trees.append(dict(kind=kind, root=int(lv[0][0]), levels=lv, A0=A0, A1=A1, F0=F0, B=B, X=X, Y=Y, Z=int(lv[4][14])))
        nxt = end
    pair_root = nxt
    edges.append((nxt, nxt + 1))
    iso = nxt + 2
    n = nxt + 3
    rowptr, col = csr_from_edges(n, edges)
    rs = np.random.RandomState(20)
    E = (rs.randn(n, D_LAZY) * 0.3).astype(np.float32)
    b = np.zeros(n, dtype=np.float32)
    for t in trees:
        lv = t["levels"]
        b[lv[2]] = 8.0            # deeper is better: a walk goes down until it stands on a leaf
        b[lv[3]] = 10.0
        b[lv[4]] = 12.0
        b[lv[5]] = 14.0
        b[t["A1"]], b[t["A0"]] = 6.0, 2.8           # root: A1 ~0.94, A0 ~0.04
        b[lv[2][2]] = 4.5                           # A1: B, not its sibling
        b[lv[2][1]] = 4.5                           # A0: F0, not its sibling
        x1a, x1b = lv[4][14], lv[4][15]             # children of X1
        b[x1a], b[x1b] = {"target": (9.1, 12.0), "loud": (12.0, 9.0), "quiet": (9.1, 12.0)}[t["kind"]]
        b[lv[4][3]] = 9.0                           # Y1 (level-3 index 1, children 2 and 3) prefers its FIRST child
    _LAZY = dict(n=n, rowptr=rowptr, col=col, E=E, b=b, trees=trees, pair_root=int(pair_root), iso=int(iso))
    return _LAZY


_WHOLE = None


def whole_graph():
    """A preferential-attachment graph (1 500 nodes, 4 edges per new node: hubs with k > 16 next to short lists), d = 32."""
    global _WHOLE
    if _WHOLE is not None:
        return _WHOLE
    n, m = 1500, 4
    rs = np.random.RandomState(5)
    edges = {(i, j) for i in range(m + 1) for j in range(i + 1, m + 1)}
    ends = [x for e in edges for x in e]
    for v in range(m + 1, n):
        picked = set()
        while len(picked) < m:
            picked.add(ends[rs.randint(len(ends))])
        for w in picked:
            edges.add((w, v))
            ends += [w, v]
    rowptr, col = csr_from_edges(n, sorted(edges))
    E = (rs.randn(n, 32) * 0.5).astype(np.float32)
    b = (rs.randn(n) * 0.1).astype(np.float32)
    _WHOLE = dict(n=n, rowptr=rowptr, col=col, E=E, b=b)
    return _WHOLE


# ------------------------------------------------------------------------------------------------ the cases
def _lazy_roots(kinds):
    g = lazy_graph()
    roots = [t["root"] for t in g["trees"] if t["kind"] in kinds]
    return np.array(roots + [g["pair_root"], g["iso"]], dtype=np.int32)


def _whole_case(name, env, strict=True):
    roots = np.random.RandomState(6).permutation(whole_graph()["n"])[:256].astype(np.int32)
    return dict(name=name, graph="whole", env=env, tree_mode=None, roots=roots, n_sample=64, seed=31, rounds=2, strict=[strict, strict])


# `strict[r]`: the G call of round r must score strictly fewer rows with the cache than without it.
#   GG_ES_MODE=2 scores every adjacency whole and shares it: distributions of <= 16 candidates are evaluated by the walks
#   themselves (self_early) and never reach the cache, and the rows of a shared adjacency are counted once whoever asks -- the
#   row count need not move, so the strict condition is asserted with GG_ES_MODE=0 only (the arrays are compared either way).
WHOLE_CASES = [
    _whole_case("levels_es0", {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0"}),
    _whole_case("levels_es2", {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "2"}, strict=False),
    _whole_case("hybrid2_es0", {"GG_WALK_LEVELS": "2", "GG_ES_MODE": "0"}),
    _whole_case("split_es0", {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0", "GG_WALK_SPLIT": "1", "GG_WALK_SPLIT_MIN": "512"}),
    _whole_case("split_es2", {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "2", "GG_WALK_SPLIT": "1", "GG_WALK_SPLIT_MIN": "512"}, strict=False),
]


def _lazy_case(name, kinds, fallback, env=None, strict=(True, True), **kw):
    """`fallback[r]` = (slots rebuilt whole by the D call of round r, by its G call)."""
    e = {"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0"}
    e.update(env or {})
    c = dict(name=name, graph="lazy", env=e, tree_mode=(1, CAP), roots=_lazy_roots(kinds), n_sample=N_SAMPLE_LAZY, seed=SEED_LAZY,
             rounds=2, strict=list(strict), fallback=fallback, entry="prepare", lazy_after=True)
    c.update(kw)
    return c


# In the cases whose first G launch is voided by a rebuild, the launch that counts is the rerun, and (the fix) the rerun scores
# privately: its row count is the uncached engine's.  The strict condition is asserted on the second round, whose D launch
# registers from the rebuilt trees and whose G launch hits; round 0 asserts "not more".
LAZY_CASES = [
    _lazy_case("lazy_no_fallback", ("quiet",), [(0, 0), (0, 0)]),
    _lazy_case("lazy_fallback_in_d", ("loud", "quiet"), [(1, 0), (0, 0)]),
    _lazy_case("lazy_fallback_in_g", ("target", "quiet"), [(0, 2), (0, 0)], strict=(False, True)),
    _lazy_case("lazy_fallback_in_g_arena1", ("target", "quiet"), [(0, 2), (0, 0)], env={"GG_LZ_ARENA": "1"}, strict=(False, True), lazy_after=False),
    _lazy_case("lazy_fallback_in_g_begin", ("target", "quiet"), [(0, 2), (0, 0)], strict=(False, True), entry="begin"),
]
DEFECT_CASE = "lazy_fallback_in_g"

# The epoch entry point: batch 0 holds the two target trees (their G launch is voided and rerun), batch 1 the quiet tree (its
# G launch hits): the strict condition is asserted over the whole epoch.
EPOCH_CASE = dict(name="lazy_fallback_in_g_epoch", graph="lazy", env={"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0"}, tree_mode=(1, CAP),
                  batches=[_lazy_roots(("target",)), _lazy_roots(("quiet",))[:1]], n_sample=N_SAMPLE_LAZY, seed=SEED_LAZY)

# A capacity rerun of a cached G launch on whole trees: the first D launch of a fresh engine (8 slots, sized) teaches the
# sync-free launches a capacity of a few thousand 16-candidate chunks per level; the G launch over every root brings ~10^5
# walks whose second hop alone needs tens of thousands of chunks.
CAPACITY_CASE = dict(name="whole_capacity_rerun", graph="whole", env={"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0"}, tree_mode=None,
                     d_slots=8, n_sample=64, seed=47)


def capacity_roots():
    return np.arange(whole_graph()["n"], dtype=np.int32)


def graph_of(case):
    return lazy_graph() if case["graph"] == "lazy" else whole_graph()


# ------------------------------------------------------------------------------------------------ the oracle's arrays
class Oracle:
    """Whole trees of `roots` (slot i = roots[i]) and the prepare calls on them: D rows in the reference's layout
    (graph_gan.py:182-202: per root with walks, its neighbours labelled 1 then its samples labelled 0), G pairs from the
    paths (graph_gan.py:272-291).  The trees carry the D-mode walks' in-place removals from call to call, as the engine's."""

    def __init__(self, g, roots):
        self.g, self.roots = g, np.ascontiguousarray(roots, dtype=np.int32)
        self.off, nbr, self.base, self.dmax = orc.c_build_trees(g["n"], g["rowptr"], g["col"], self.roots)
        self.nbr = nbr.copy()
        self.Ep = orc.pad_rows(g["E"])
        self.deg = (g["rowptr"][1:] - g["rowptr"][:-1]).astype(np.int32)

    def walks(self, slots, n_walks, for_d, seed, stream):
        return orc.c_walk_sample(self.Ep, self.g["b"], self.off, self.nbr, self.base, self.roots, slots, n_walks, for_d, seed, stream, self.dmax + 3)

    def prepare_d(self, slots, seed, stream):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        nw = self.deg[self.roots[slots]]
        want = self.walks(slots, nw, True, seed, stream)
        rowptr, col = self.g["rowptr"], self.g["col"]
        c, nb, lab = [], [], []
        w = 0
        for i, s in enumerate(slots):
            r, k = int(self.roots[s]), int(nw[i])
            if want["root_status"][i] == 0 and k > 0:
                c.append(np.full(2 * k, r, np.int32))
                nb.append(col[rowptr[r]: rowptr[r + 1]])
                nb.append(want["samples"][w: w + k])
                lab.append(np.concatenate([np.ones(k, np.float32), np.zeros(k, np.float32)]))
            w += k
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        return dict(center=cat(c, np.int32), neighbor=cat(nb, np.int32), label=cat(lab, np.float32), root_status=want["root_status"], walks=want)

    def prepare_g(self, slots, n_sample, seed, stream, window=2):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        want = self.walks(slots, np.full(len(slots), n_sample, np.int32), False, seed, stream)
        lib = orc.c_oracle()
        stride = want["paths"].shape[1]
        a = np.zeros(2 * window * stride, np.int32)
        b = np.zeros(2 * window * stride, np.int32)
        n1, n2 = [], []
        pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
        for w in np.flatnonzero(want["path_len"] > 0):
            row = want["paths"][w]
            k = lib.orc_pairs_from_path(row.ctypes.data_as(ctypes.c_void_p), int(want["path_len"][w]), window, pa, pb)
            n1.append(a[:k].copy())
            n2.append(b[:k].copy())
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int32)
        return dict(node_1=cat(n1), node_2=cat(n2), root_status=want["root_status"], samples=want["samples"], paths=want["paths"],
                    path_len=want["path_len"], hops=want["hops"])


def oracle_rounds(case, roots=None):
    """[(D result, G result)] of the case's rounds: round r uses streams 2 r and 2 r + 1, every slot."""
    roots = case["roots"] if roots is None else roots
    o = Oracle(graph_of(case), roots)
    slots = np.arange(len(roots), dtype=np.int32)
    return [(o.prepare_d(slots, case["seed"], 2 * r), o.prepare_g(slots, case["n_sample"], case["seed"], 2 * r + 1)) for r in range(case.get("rounds", 1))]


# ------------------------------------------------------------------------------------------------ the lazy preconditions
def _stood_on(res, w0, w1):
    """Per walk of [w0, w1): the nodes it stood on (its path without the closing back-step)."""
    return [res["paths"][w, : max(int(res["path_len"][w]) - 1, 0)] for w in range(w0, w1)]


def _spec_choice(Ep, b, cur, cand, m):
    """Spec S1-S3, S5 for one distribution: the index picked among `cand` by a walk on `cur` whose hop drew m."""
    lib = orc.c_oracle()
    ld = Ep.shape[1]
    rows = [np.ascontiguousarray(Ep[v]) for v in cand]
    cr = np.ascontiguousarray(Ep[cur])
    s = [np.float32(lib.orc_dot16(cr.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p), ld)) + np.float32(b[v]) for r, v in zip(rows, cand)]
    mx = max(s)
    w = [int(lib.orc_weight(ctypes.c_float(lib.orc_expf(ctypes.c_float(np.float32(x - mx)))))) for x in s]
    t = (int(m) * sum(w)) >> 53
    acc = 0
    for j, x in enumerate(w):
        acc += x
        if acc > t:
            return j
    return len(w) - 1


def tree_facts(tree, d_walks, g_walks, seed, g_stream):
    """What the oracle's D-mode walks (`d_walks` = (result, first walk, end)) and G-mode walks of one regular tree did; the
    CPU test asserts on these, the seed scan reads them.  Ranks are BFS ranks = node id - root id (the trees are BFS numbered)."""
    g = lazy_graph()
    level, father, order = bfs_levels(g["n"], g["rowptr"], g["col"], tree["root"])
    has_kids = np.zeros(g["n"], dtype=bool)
    has_kids[father[order[1:]]] = True
    first_L = int(order[level[order] == L_EXACT][0])
    d_nodes = _stood_on(*d_walks)
    g_nodes = _stood_on(*g_walks)
    flat = lambda xs: np.unique(np.concatenate(xs)) if len(xs) else np.zeros(0, np.int64)
    dn, gn = flat(d_nodes), flat(g_nodes)
    deep_nonleaf = lambda v: v[(level[v] >= L_EXACT + 2) & has_kids[v]]
    d_L1 = dn[level[dn] == L_EXACT + 1]
    g_L1 = gn[level[gn] == L_EXACT + 1]
    facts = dict(
        d_deep_nonleaf=deep_nonleaf(dn), g_deep_nonleaf=deep_nonleaf(gn),
        d_L1_foreign=d_L1[(father[d_L1] != first_L) & has_kids[d_L1]], g_L1_first=g_L1[father[g_L1] == first_L],
        d_L_nodes=dn[level[dn] == L_EXACT], first_L=first_L, level=level, father=father)
    # The collision the parent commit's rerun runs into.  The D-mode walks stood on ONE level-2 node, so its list was the first
    # one resolved and its i-th child holds pool rank P + i; the D launch registered the children it stood on.  In the whole
    # tree rank P + i is the i-th child of the first level-2 node.  A G-mode walk standing on that node finds the stale entry
    # (k = C + 1 on both sides) and samples from the other node's prefix sums: `changed` lists the walks whose pick then differs.
    changed = []
    if len(facts["d_L_nodes"]) == 1 and int(facts["d_L_nodes"][0]) != first_L:
        B = int(facts["d_L_nodes"][0])
        kids = lambda v: [int(x) for x in order if father[x] == v and x != v]
        stale = {P_EXACT + i: x for i, x in enumerate(kids(B)) if x in set(d_L1.tolist())}
        res, w0, w1 = g_walks
        for w in range(w0, w1):
            path = res["paths"][w, : int(res["path_len"][w])]
            for hop in range(len(path) - 1):
                y = int(path[hop])
                if level[y] != L_EXACT + 1:
                    continue
                x = stale.get(y - tree["root"])
                if x is not None and x != y:
                    cand_y = [int(father[y])] + kids(y)
                    cand_x = [int(father[x])] + kids(x)
                    assert len(cand_x) == len(cand_y) == C + 1
                    m = orc.uniform53(seed, g_stream, tree["root"], w - w0, hop)
                    right = _spec_choice(res["Ep"], g["b"], y, cand_y, m)
                    assert cand_y[right] == int(path[hop + 1])  # (the restatement agrees with the oracle's walk)
                    wrong = _spec_choice(res["Ep"], g["b"], x, cand_x, m)
                    if wrong != right:
                        changed.append((w, hop, y, x, right, wrong))
                break  # (the first level-3 node of the walk: whatever follows a wrong pick is another walk)
    facts["changed"] = changed
    return facts


def check_target(case, r=0):
    """Facts of every regular tree among the case's roots for round r: {slot: (kind, facts)}."""
    g = lazy_graph()
    o = Oracle(g, case["roots"])
    slots = np.arange(len(case["roots"]), dtype=np.int32)
    for q in range(r + 1):
        d = o.prepare_d(slots, case["seed"], 2 * q)
        gg = o.prepare_g(slots, case["n_sample"], case["seed"], 2 * q + 1)
    dw = d["walks"]
    gg["Ep"] = o.Ep
    nw = o.deg[case["roots"]]
    dptr = np.concatenate([[0], np.cumsum(nw)])
    out = {}
    for s, root in enumerate(case["roots"]):
        tree = [t for t in g["trees"] if t["root"] == root]
        if not tree:
            continue
        ns = case["n_sample"]
        out[s] = (tree[0]["kind"], tree_facts(tree[0], (dw, int(dptr[s]), int(dptr[s + 1])), (gg, s * ns, (s + 1) * ns), case["seed"], 2 * r + 1))
    return out
