"""Cases of the generator-change matrix (tests/test_gpu_generator_changes.py) and the CPU side of every one of them: graphs,
the two generators A and B, the call sequence of every cache row, the C oracle's arrays, and the SENSITIVITY of a checked launch
(tests/test_generator_change_cases_cpu.py asserts it for every pair chosen here; the GPU test asserts it where B comes out of an
optimizer step).

Nothing here touches the engine.  Walks are counter based (spec S4: Philox keyed by seed, stream, root id, walk, hop): with the
same trees, seed and stream, the walks under A's tables and under B's draw the same uniforms and differ only through the scores.

SENSITIVITY.  A checked launch counts only if, under the oracle, at most half of its walks end on the same node with A's tables as
with B's (from the same tree state): a launch that sampled from scores, prefix sums or distributions of A would then be caught on
most walks, and not on a few of them by luck.

THE ROWS.  Every row is a call sequence: `pre` on generator A (it warms the cache the row names), the trigger, `check`.
  ("d", s) = prepare_d over every slot on stream s, ("g", s) = prepare_g with N_SAMPLE walks per root on stream s,
  ("begin", s) = prepare_g_begin with the arguments of the ("g", s) that follows the trigger (nothing for the oracle)."""
import numpy as np

from oracle import graphgan_oracle as orc
from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc, load_small
from tests.support import dist_cache_cases as dc

SEED = 7
N_SAMPLE = 20
MAX_EQUAL = 0.5        # the sensitivity condition: share of walks with equal end nodes under A and under B
GS_SLOTS = 40          # graph_softmax row: 40 slots of CA-GrQc, whole trees
GS_FACTOR = 100.0      # ... whose DP under A and under B differ by at least GS_FACTOR x TOL_LOGP on every slot with children

csr_from_edges = dc.csr_from_edges   # symmetric CSR from undirected edges: numpy only


# ------------------------------------------------------------------------------------------------ graphs
def csr_from_lists(n, graph):
    """The reference's adjacency dict (lists in file order, self loops and repeated edges as read) as CSR, without the library."""
    return orc.graph_to_csr(n, graph)


_GRAPHS = {}


def graph(name):
    """dict(name, n, rowptr, col, E, roots, d_mode): "small1" (64 nodes), "small3" (90 nodes), every node a root; "ca": CA-GrQc with
    every 20th node as a root (263 roots, trees up to 17 levels deep), whose D-mode launches are not checked (most of its roots
    have one or two walks: see the CPU test); "small1_90": small 1 with 26 isolated nodes behind it and the 90 rows of small 3's
    E -- the graph an engine of small 3's size holds BEFORE set_graph_csr replaces it."""
    if name in _GRAPHS:
        return _GRAPHS[name]
    if name in ("small1", "small3"):
        g, n, adj = load_small(int(name[-1]))
        rowptr, col = csr_from_lists(n, adj)
        out = dict(name=name, n=n, rowptr=rowptr, col=col, E=g["E"].astype(np.float32), roots=np.arange(n, dtype=np.int32), d_mode=True)
    elif name == "small1_90":
        s1, s3 = graph("small1"), graph("small3")
        rowptr = np.concatenate([s1["rowptr"], np.full(s3["n"] - s1["n"], s1["rowptr"][-1], np.int64)])
        out = dict(name=name, n=s3["n"], rowptr=rowptr, col=s1["col"], E=s3["E"], roots=s3["roots"], d_mode=True)
    elif name == "ca":
        d, n, adj = load_ca_grqc()
        rowptr, col = csr_from_lists(n, adj)
        out = dict(name=name, n=n, rowptr=rowptr, col=col, E=ca_grqc_init_embeddings(d, n).astype(np.float32),
                   roots=np.arange(0, n, 20, dtype=np.int32), d_mode=False)
    else:
        raise KeyError(name)
    _GRAPHS[name] = out
    return out


# ------------------------------------------------------------------------------------------------ the two generators
def bias_of(g):
    return (2.0 * np.random.RandomState(1).randn(g["n"])).astype(np.float32)


def bias_pair(g):
    """A = (E, b_A), B = (E, -b_A), b_A = 2 RandomState(1).randn(n)."""
    b = bias_of(g)
    return dict(E=g["E"], b=b), dict(E=g["E"], b=-b)


def emb_pair(g):
    """A pair that differs in E only.  NOT E_B = -E_A: the generator's score E[u] . E[v] + b[v] is bilinear in E, so the negated
    table gives the same scores bit for bit and every walk ends where it ended (the CPU test asserts the share 1.0).  The rows of
    the ODD nodes are negated instead: every score between an odd and an even node changes its sign, the others stay."""
    E_B = g["E"].copy()
    E_B[1::2] *= np.float32(-1.0)
    b = bias_of(g)
    return dict(E=g["E"], b=b), dict(E=E_B, b=b)


def negated_emb_pair(g):
    b = bias_of(g)
    return dict(E=g["E"], b=b), dict(E=-g["E"], b=b)


PAIRS = {"bias": bias_pair, "emb": emb_pair}


# ------------------------------------------------------------------------------------------------ the rows
# `env`: set before the engine exists (gg_create reads it); a value of None removes the variable (the library's default).
# The G launch comes first and is repeated at once: the engine's first launch finds the cache cold, its repeat is the warm proof.
# (Behind a D launch over every root of a 64-node graph there is nothing left to score: the proof would read 0 < 0.)  No D launch
# follows before the trigger: every walk launch clears g_paths_valid and only prepare_g sets it, so a g_pass as one batch takes
# the whole-walk route (run_path_step) only if the trigger stands directly behind a prepare_g.  The D launch is the first of the
# checked ones.
ES_PRE = [("g", 1), ("g", 1)]
# Rows in which a whole-pass trigger reaches the whole-walk route.  In "dist" a D launch, in "begun" a prepare_g_begin stands
# between the last prepare_g and the trigger: there a g_pass as one batch is one run_step over the pair arrays, the path g_step
# takes, and the matrix has no such cell.
WHOLE_WALK_ROWS = ("es2", "es1")
ROWS = {
    # the edge-score cache alone (no distribution cache beside it: what the repeat launch saves is the edge scores')
    "es2": dict(env={"GG_WALK_LEVELS": "64", "GG_ES_MODE": "2", "GG_NO_DIST_CACHE": "1"}, pre=ES_PRE, check=[("d", 2), ("g", 3)]),
    "es1": dict(env={"GG_WALK_LEVELS": "64", "GG_ES_MODE": None, "GG_NO_DIST_CACHE": "1"}, pre=ES_PRE, check=[("d", 2), ("g", 3)]),
    # the distribution cache alone: step 0, then the D launch of step 1 | trigger | its G launch
    "dist": dict(env={"GG_WALK_LEVELS": "64", "GG_ES_MODE": "0", "GG_NO_DIST_CACHE": None}, pre=[("d", 0), ("g", 1), ("d", 2)], check=[("g", 3)]),
    # a begun launch, every cache at its default
    "begun": dict(env={"GG_WALK_LEVELS": "64", "GG_ES_MODE": None, "GG_NO_DIST_CACHE": None},
                  pre=[("d", 0), ("g", 1), ("d", 2), ("begin", 3)], check=[("g", 3)]),
}


def check_ops(row, g):
    """The row's checked launches on graph g: D-mode launches on the small graphs only."""
    return [op for op in ROWS[row]["check"] if op[0] != "d" or g["d_mode"]]


# ------------------------------------------------------------------------------------------------ the oracle side of a sequence
class Oracle(dc.Oracle):
    """dist_cache_cases.Oracle (whole trees that carry the D-mode walks' Q3 removals from call to call, D rows, G pairs) with
    tables that can be replaced between two calls, and a tree state that can be copied."""

    def __init__(self, g, roots, tables):
        dc.Oracle.__init__(self, dict(g, E=tables["E"], b=tables["b"]), roots)
        self.slots = np.arange(len(self.roots), dtype=np.int32)

    def set_tables(self, tables):
        self.g = dict(self.g, E=tables["E"], b=np.ascontiguousarray(tables["b"], dtype=np.float32))
        self.Ep = orc.pad_rows(tables["E"])

    def tree_lists(self):
        """(off, nbr, base, max depth) in the reference's shape, Q3 removals (-1) included: what Engine.set_trees takes."""
        return self.off, self.nbr.copy(), self.base, self.dmax

    def run(self, op, n_sample=N_SAMPLE, seed=SEED):
        kind, stream = op
        if kind == "d":
            return self.prepare_d(self.slots, seed, stream)
        if kind == "g":
            return self.prepare_g(self.slots, n_sample, seed, stream)
        assert kind == "begin"
        return None

    def end_nodes_under(self, tables, op, n_sample=N_SAMPLE, seed=SEED):
        """The end nodes the launch `op` WOULD give under `tables` from the present tree state; the state is left as it was."""
        keep = (self.g, self.Ep, self.nbr)
        self.nbr = self.nbr.copy()
        self.set_tables(tables)
        res = self.run(op, n_sample, seed)
        self.g, self.Ep, self.nbr = keep
        return (res["walks"] if op[0] == "d" else res)["samples"]


def equal_share(a, b):
    """Share of walks that end on the same node (an aborted root's -1 on both sides counts as equal: nothing to tell apart)."""
    assert a.shape == b.shape and len(a) > 0
    return float(np.mean(a == b))


def run_sequence(g, roots, A, B, row):
    """The oracle through `pre` on A and `check` on B.  Returns (oracle, [result of every pre op], [(op, result under B, share of
    equal end nodes against the same launch under A)] of the checked launches)."""
    o = Oracle(g, roots, A)
    pre = [o.run(op) for op in ROWS[row]["pre"]]
    o.set_tables(B)
    return o, pre, run_checks(o, A, check_ops(row, g))


def run_checks(o, A, ops):
    """The checked launches on the oracle's present tables, each with its share against A's tables from the same tree state."""
    out = []
    for op in ops:
        stale = o.end_nodes_under(A, op)
        res = o.run(op)
        out.append((op, res, equal_share((res["walks"] if op[0] == "d" else res)["samples"], stale)))
    return out


def issue_table(g, A, B):
    """The figures the issue quotes: fresh trees, D launch on stream 0, then G launch with 20 walks per root on stream 1."""
    o = Oracle(g, g["roots"], B)
    out = []
    for op in (("d", 0), ("g", 1)):
        stale = o.end_nodes_under(A, op)
        res = o.run(op)
        out.append(equal_share((res["walks"] if op[0] == "d" else res)["samples"], stale))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ graph_softmax row
def gs_case():
    """CA-GrQc, the first GS_SLOTS of its roots (every 20th node), bias pair; trees fresh (no Q3 removals), G mode."""
    g = graph("ca")
    A, B = bias_pair(g)
    return g, g["roots"][:GS_SLOTS].copy(), A, B


def gs_difference(dp, off, nbr, base, roots, A, B):
    """Per slot: (has children, max |logp_A - logp_B| over the nodes with P > 0) of the float64 DP `dp` = host_graph_softmax."""
    out = []
    for r, root in enumerate(roots):
        lists = nbr[base[r]:base[r + 1]]
        la, _ = dp(A["E"], A["b"], int(root), off[r], lists, False)
        lb, _ = dp(B["E"], B["b"], int(root), off[r], lists, False)
        fin = np.isfinite(la)
        assert np.array_equal(fin, np.isfinite(lb))
        kids = int(off[r][root + 1] - off[r][root]) - 1
        out.append((kids > 0, float(np.max(np.abs(la[fin] - lb[fin]), initial=0.0))))
    return out
