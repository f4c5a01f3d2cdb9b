"""Cases of the root-batched epoch tests (tests/test_gpu_epoch_cases.py) and their CPU side (tests/test_epoch_cases_cpu.py): a
small graph whose hubs sit on both sides of every word edge of the Q3 store, the batch plans over its roots, and the reference
-- the sequential C oracle driven batch by batch on trees that live for the whole run.  Numpy and the oracle only; nothing
here touches the engine.

THE GRAPH (ladder()).  Node 0 and node n - 1 are isolated.  Nodes 1 .. 10 are hubs chained 1 - 2 - ... - 10; hub h has k_h leaves
and every leaf a private pendant node, so that a depth-1 child has a tree child of its own.  The RAW degrees of hubs 1 .. 9 --
leaves plus chain edges, np.diff(rowptr) -- are 2, 31, 32, 33, 63, 64, 65, 96, 97: one, two, three and four words of the store
(ceil(raw degree / 32)), with a hub on either side of every edge.  Hub 10 has 32 DISTINCT neighbours (31 leaves and hub 9) and
raw degree 35: the file starts with its first leaf edge twice and a self-loop (which read_edges appends twice), so its adjacency
begins [x, x, 10, 10, ...]; the rank of a tree child among the tree children -- the bit index of the store -- differs from the CSR
position for every child but the first, and the store holds two words where the 32 children need one.

WHAT THE WALKS DO ON IT (oracle/walk_oracle.c).  D-mode from a hub: hub -> leaf (the leaf's father entry is removed: a bit of the
hub) -> pendant -> back: never aborts.  D-mode from a leaf: a walk that picks the pendant finds the list [leaf] and aborts the
root: about a third of all roots.  G-mode walks remove nothing but READ the lists: from a leaf whose father entry is still there
a walk may step back to the root and end.  So the stored bits decide G-mode walks.  They do NOT decide D-mode walks: a D-mode
walk removes the root from a depth-1 child's list before it scores the list, whether an earlier walk has done so or not, and the
abort test comes before the removal -- the D samples of an epoch are the same with the bits cleared (the CPU test asserts this
beside the G-mode difference).

REPEATED ROOTS.  A root that comes back in a later batch of the same epoch is walked again on the same lists.  With the streams
of its first visit every draw would repeat -- the Philox counter is (hop, walk, root, stream) -- and the visit would prove
nothing, so a plan gives a later batch a stream shift: the second visit draws anew, sets further bits, and its G-mode walks see
the union.
"""
import collections

import numpy as np

from oracle import graphgan_oracle as orc

D_EMB = 8
N_SAMPLE = 4
SEED = 5            # (seeds 1 .. 4 miss a condition of the CPU test: mostly the lone child in the last word of a hub of 33, 65 or 97
                    # children, which epoch 0 visits with probability 0.63)
WINDOW = 2
HUB_RAW_DEGREES = (2, 31, 32, 33, 63, 64, 65, 96, 97)      # hubs 1 .. 9, chain edges included
HUB_WORDS = (1, 1, 1, 2, 2, 2, 3, 3, 4)                    # ceil(raw degree / 32)
LEAVES = (1, 29, 30, 31, 61, 62, 63, 94, 95)               # raw degree minus the chain edges (hub 1 has one, the others two)
DUP_LEAVES = 31                                            # hub 10: 31 leaves + hub 9 = 32 distinct neighbours
DUP_RAW_DEGREE = DUP_LEAVES + 1 + 1 + 2                    # ... + the duplicate + the self-loop's two entries
PERMUTED_LEAVES = (95, 61, 1, 94, 29, 63, 31, 30, 62)      # case 5: other degrees at the same ids, the same node count

# Largest |fp32 reference - float64 step| / band of the D pass and the G pass over one committed epoch of the ladder, as
# tests/test_epoch_cases_cpu.py measures it in the way of step_grad_cases.CPU_FILL.  That test fails when it measures more, or
# when this exceeds 0.5.  (Measured: 0.381 for the D pass over 2 582 rows, 0.490 for the G pass over 32 868 pairs -- the rounding
# of the new value against the 2 u |var| the band grants it, as in step_grad_cases.)
PASS_CPU_FILL = 0.49


# ------------------------------------------------------------------------------------------------ the graph
def edges_to_raw_csr(n, edges):
    """read_edges' adjacency (utils.py:36-37): edge k = (a, b) appends b to graph[a], then a to graph[b], in file order; duplicates
    kept, a self-loop twice."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    src, dst = np.empty(2 * len(edges), np.int64), np.empty(2 * len(edges), np.int32)
    src[0::2], dst[0::2] = edges[:, 0], edges[:, 1]
    src[1::2], dst[1::2] = edges[:, 1], edges[:, 0]
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
    return rowptr, dst[order]


def ladder(leaves=LEAVES, dup_hub=True):
    """(n, rowptr, col, info).  info: hubs (ids, hub 10 last when present), dup_hub (its id or None), leaves_of {hub: ids},
    isolated (ids), edges.  dup_hub=False builds the degenerate ladder without the duplicate / self-loop hub."""
    n_hubs = len(leaves) + (1 if dup_hub else 0)
    counts = list(leaves) + ([DUP_LEAVES] if dup_hub else [])
    hubs = list(range(1, n_hubs + 1))
    nxt = n_hubs + 1
    leaves_of, pend_of = {}, {}
    for h, k in zip(hubs, counts):
        leaves_of[h] = list(range(nxt, nxt + k))
        nxt += k
    for h in hubs:
        for x in leaves_of[h]:
            pend_of[x] = nxt
            nxt += 1
    n = nxt + 1                                   # ... and the isolated last node
    edges = []
    if dup_hub:
        h = hubs[-1]
        edges += [(h, leaves_of[h][0]), (h, leaves_of[h][0]), (h, h)]     # FIRST in the file: first in its adjacency
    for a, b in zip(hubs[:-1], hubs[1:]):
        edges.append((a, b))
    for h in hubs:
        for x in leaves_of[h]:
            if not (dup_hub and h == hubs[-1] and x == leaves_of[h][0]):
                edges.append((h, x))
            edges.append((x, pend_of[x]))
    rowptr, col = edges_to_raw_csr(n, edges)
    hub_of = np.zeros(n, np.int32)                # the hub a node hangs on (itself for a hub, 0 for the isolated nodes)
    for h in hubs:
        hub_of[h] = h
        for x in leaves_of[h]:
            hub_of[x] = hub_of[pend_of[x]] = h
    info = dict(hubs=hubs, dup_hub=hubs[-1] if dup_hub else None, leaves_of=leaves_of, isolated=[0, n - 1], edges=np.array(edges, np.int32),
                hub_of=hub_of)
    return n, rowptr, col, info


def gauss_tables(n, seed):
    """Generator and discriminator tables: Gaussian rows of deviation 0.5, biases of deviation 0.1."""
    rs = np.random.RandomState(seed)
    E, b = (0.5 * rs.randn(n, D_EMB)).astype(np.float32), (0.1 * rs.randn(n)).astype(np.float32)
    Ed, bd = (0.5 * rs.randn(n, D_EMB)).astype(np.float32), (0.1 * rs.randn(n)).astype(np.float32)
    return E, b, Ed, bd


class Case:
    """A graph, its tables and the pristine trees of ALL roots (slot r = root r)."""

    def __init__(self, leaves=LEAVES, dup_hub=True, seed=SEED):
        self.n, self.rowptr, self.col, self.info = ladder(leaves, dup_hub)
        n = self.n
        self.d, self.n_sample, self.seed = D_EMB, N_SAMPLE, seed      # one seed for the tables and for the walks' Philox key
        self.deg = np.diff(self.rowptr).astype(np.int32)
        self.E, self.b, self.Ed, self.bd = gauss_tables(n, seed)
        self.roots = np.arange(n, dtype=np.int32)
        self.hubs = np.array(self.info["hubs"], np.int32)
        self.word_off = np.concatenate([[0], np.cumsum((self.deg.astype(np.int64) + 31) // 32)])
        self.off, nbr, self.base, dmax = orc.c_build_trees(n, self.rowptr, self.col, self.roots)
        self.nbr0 = nbr.copy()
        self.stride = dmax + 3
        for a in (self.rowptr, self.col, self.deg, self.E, self.b, self.Ed, self.bd, self.roots, self.off, self.nbr0, self.base, self.word_off):
            a.flags.writeable = False


_CASES = {}


def case(leaves=LEAVES, dup_hub=True):
    key = (tuple(leaves), dup_hub)
    if key not in _CASES:
        _CASES[key] = Case(leaves, dup_hub)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ the reference
def d_rows(c, batch, want):
    """prepare_data_for_d's rows of one batch (graph_gan.py:190-200), as _oracle_d_rows of tests/test_gpu_epoch.py builds them."""
    cen, nb, lab, w = [], [], [], 0
    for i, r in enumerate(batch):
        k = int(c.deg[r])
        if want["root_status"][i] == 0 and k > 0:
            cen += [int(r)] * (2 * k)
            nb += list(c.col[c.rowptr[r]:c.rowptr[r + 1]]) + list(want["samples"][w:w + k])
            lab += [1] * k + [0] * k
        w += k
    return np.array(cen, np.int32), np.array(nb, np.int32), np.array(lab, np.float32)


def g_pairs(want, window=WINDOW):
    n1, n2 = [], []
    for wlk in range(len(want["path_len"])):
        L = want["path_len"][wlk]
        if L > 0:
            for a, b in orc.pairs_from_path(list(want["paths"][wlk, :L]), window):
                n1.append(a)
                n2.append(b)
    return np.array(n1, np.int32), np.array(n2, np.int32)


class OracleRun:
    """The reference's self.trees for one run: built once, mutated by every D-mode walk since (graph_gan.py:258-259)."""

    def __init__(self, c):
        self.c = c
        self.nbr = c.nbr0.copy()
        self.Ep = orc.pad_rows(c.E)

    def clear_bits(self):
        self.nbr[:] = self.c.nbr0

    def walks(self, batch, for_d, stream, n_walks=None):
        c = self.c
        batch = np.ascontiguousarray(batch, np.int32)
        nw = c.deg[batch] if for_d else np.full(len(batch), c.n_sample if n_walks is None else n_walks, np.int32)
        return orc.c_walk_sample(self.Ep, c.b, c.off, self.nbr, c.base, c.roots, batch, nw, for_d, c.seed, stream, c.stride)

    def add(self, batch, do_d, do_g, stream_d, stream_g):
        """One gg_epoch_add: dict(d, g: the walks, or None; rows: (center, neighbor, label); pairs: (node_1, node_2))."""
        out = dict(d=None, g=None, rows=(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
                   pairs=(np.zeros(0, np.int32), np.zeros(0, np.int32)))
        if len(batch) and do_d:
            out["d"] = self.walks(batch, True, stream_d)
            out["rows"] = d_rows(self.c, batch, out["d"])
        if len(batch) and do_g:
            out["g"] = self.walks(batch, False, stream_g)
            out["pairs"] = g_pairs(out["g"])
        return out

    def words(self):
        """The mutation state in the store's layout (as _oracle_q3_bits of tests/test_gpu_epoch.py): bit j of root r = the father
        entry of its (j + 1)-th tree child is gone."""
        c, nbr = self.c, self.nbr
        words = np.zeros(int(c.word_off[-1]), np.uint32)
        for r in range(c.n):
            lst = nbr[c.base[r] + c.off[r, r]: c.base[r] + c.off[r, r + 1]]          # [r, child_1, ..., child_k]
            for j, ch in enumerate(lst[1:]):
                if nbr[c.base[r] + c.off[r, ch]] < 0:
                    words[c.word_off[r] + j // 32] |= np.uint32(1 << (j % 32))
        return words

    def segments(self, batch):
        """(off [B, n + 1], nbr, base [B + 1]) of the batch's trees as they are now: what gg_get_trees shows after the add."""
        c = self.c
        segs = [self.nbr[c.base[r]:c.base[r + 1]] for r in batch]
        base = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
        return c.off[np.asarray(batch, np.int64)].copy(), (np.concatenate(segs) if segs else np.zeros(0, np.int32)), base


Plan = collections.namedtuple("Plan", "name batches shifts")   # shifts[i]: added to both streams of batch i (repeated roots)


def streams(epoch, shift=0):
    return 2 * epoch + shift, 2 * epoch + 1 + shift


def oracle_epochs(c, plan, n_epochs, segments_of=None, run=None):
    """The reference over `n_epochs` outer epochs of the plan: per epoch dict(cum [(rows, pairs) after each batch], center,
    neighbor, label, node_1, node_2, words, batch [the add() of every batch]); segments_of = (epoch, batch index) adds
    "segments": the trees of that batch right after its add."""
    run = run or OracleRun(c)
    out = []
    for ep in range(n_epochs):
        rows, pairs, cum, adds, seg = [], [], [], [], None
        n_rows = n_pairs = 0
        for i, (batch, shift) in enumerate(zip(plan.batches, plan.shifts)):
            sd, sg = streams(ep, shift)
            a = run.add(batch, True, True, sd, sg)
            rows.append(a["rows"])
            pairs.append(a["pairs"])
            n_rows += len(a["rows"][0])
            n_pairs += len(a["pairs"][0])
            cum.append((n_rows, n_pairs))
            adds.append(a)
            if segments_of == (ep, i):
                seg = run.segments(batch)
        cat = lambda parts, k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
        out.append(dict(cum=cum, center=cat(rows, 0, np.int32), neighbor=cat(rows, 1, np.int32), label=cat(rows, 2, np.float32),
                        node_1=cat(pairs, 0, np.int32), node_2=cat(pairs, 1, np.int32), words=run.words(), batch=adds, segments=seg))
    return out


def per_root(c, plan, epoch_ref):
    """{root: [(D status, D samples, D paths, G paths) per visit]} of one epoch of oracle_epochs."""
    out = {}
    for batch, a in zip(plan.batches, epoch_ref["batch"]):
        wd = wg = 0
        for i, r in enumerate(batch):
            k = int(c.deg[r])
            d, g = a["d"], a["g"]
            out.setdefault(int(r), []).append((int(d["root_status"][i]), d["samples"][wd:wd + k].tobytes(), d["paths"][wd:wd + k].tobytes(),
                                               g["paths"][wg:wg + c.n_sample].tobytes()))
            wd += k
            wg += c.n_sample
    return out


# ------------------------------------------------------------------------------------------------ the passes over a committed epoch
def pass_reference(model, E, b, u, v, x):
    """(reference, E', b', band of E', band of b') of one whole-list SGD pass of model "d" / "g" with step_grad_cases' constants:
    that module's float64 step and its band (the staged pass's terms from 16 384 pairs on, as its cases take them)."""
    from tests.support import step_grad_cases as sg
    ref = sg.grad_reference(model, E, b, u, v, x, sg.LAMBDA)
    scale = sg.hub_scale(model == "g", len(u)) if sg.staged(len(u), E.shape[1], "sgd", {}) else None
    dG, dGb = sg.grad_bands(ref, scale)
    return (ref,) + sg.opt_step("sgd", E, b, ref["G"], ref["Gb"], dG, dGb, None, sg.OptState(E.shape), sg.LR_SGD)


# ------------------------------------------------------------------------------------------------ the plans
REPEAT_SHIFT = 100


def _chunks(a, size):
    return [a[i:i + size] for i in range(0, len(a), size)]


def plans(c):
    roots, n, hubs = c.roots, c.n, c.hubs
    perm = np.random.RandomState(5).permutation(n).astype(np.int32)
    out = []

    def add(name, batches, shifts=None):
        batches = [np.ascontiguousarray(b, np.int32) for b in batches]
        out.append(Plan(name, batches, list(shifts) if shifts is not None else [0] * len(batches)))

    add("one-batch", [roots])
    add("ones-then-rest", [roots[i:i + 1] for i in range(40)] + [roots[40:]])
    cuts = np.cumsum([0, 1, 2, 63, 64, 65])
    add("sizes-1-2-63-64-65-rest", [roots[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [roots[cuts[-1]:]])
    add("descending-100", _chunks(roots[::-1], 100))
    add("permuted-37", _chunks(perm, 37))
    p37 = _chunks(perm, 37)
    add("permuted-37-empty-batch", p37[:len(p37) // 2] + [perm[:0]] + p37[len(p37) // 2:])
    others = np.setdiff1d(roots, hubs)
    between = np.array_split(others, len(hubs) + 1)
    alone = [between[0]]
    for i, h in enumerate(hubs):
        alone += [np.array([h], np.int32), between[i + 1]]
    add("hubs-alone", alone)
    add("every-third-root", _chunks(np.union1d(roots[::3], hubs), 128))
    back = np.array([hubs[-1], hubs[6], hubs[8]], np.int32)         # the duplicate hub, raw degrees 65 and 97
    asc = _chunks(roots, 200)
    add("three-hubs-come-back", asc[:2] + [back] + asc[2:], [0, 0, REPEAT_SHIFT] + [0] * (len(asc) - 2))
    return out


def plan(c, name):
    return [p for p in plans(c) if p.name == name][0]


PLANS = ("one-batch", "ones-then-rest", "sizes-1-2-63-64-65-rest", "descending-100", "permuted-37", "permuted-37-empty-batch", "hubs-alone",
         "every-third-root", "three-hubs-come-back")   # the names plans() gives, in its order (the CPU test compares)
