"""Cases of the window-size tests of the generator's half of a training step (tests/test_gpu_window.py), and their CPU side
(tests/test_window_cases_cpu.py): graphs, tables, the window list, the C oracle's walks and their pairs, a float64 restatement of
one generator SGD step on a pair list, and the band a table entry must lie in after that step.  Numpy only; nothing here touches
the engine.

GRAPHS.  "small" is load_small(3) as tests/test_gpu_steps.py uses it: 90 nodes, shallow trees (path stride <= 17, the SHORT
instances of path_grad_kernel).  "deep" is a chain 0 - 1 - ... - 39 with a leaf 40 + j on every fifth chain node 5 j (48 nodes).
Its DRIVING generator table has column 0 = sqrt(0.2) v on the chain, so the score of the edge (v, v + 1) is about 0.2 v (v + 1):
a walk climbs the chain to node 39, steps back to 38 and ends.  From the leaf on node 0 that is a path of 41 nodes: the tree depth
is 40, the stride 43, and the kernels run with SHORT = false -- ids and stage slots at positions >= 16 come from memory, a walk's
pairs from 64 on take their reward from memory.

The driving table's scores reach several hundred: 1 - sigmoid(s) is exactly 0 there, and a gradient computed on it would hide any
index error.  So the walks are made with the driving table, and the pass runs on a MODERATE table (Gaussian, scores of order
1.5) that the test swaps in before g_pass; the engine keeps walks, pairs and rewards across set_embeddings / set_bias.

THE BAND.  One SGD step is E' = E - lr G with, for the n pairs (u_i, v_i) with reward r_i,
    s_i = E[u_i] . E[v_i] + b[v_i],  sg_i = sigmoid(s_i),  ds_i = -(r_i / n) (1 - sg_i)  (0 outside 1e-5 <= sg_i <= 1)
    G[u_i] += ds_i E[v_i] + lambda E[u_i],   G[v_i] += ds_i E[u_i] + lambda E[v_i],   Gb[v_i] += ds_i.
sgd_reference() evaluates this in float64 from the fp32 inputs and returns with it A (the same sums over absolute values), m (the
number of pair contributions per row) and S_max (the largest sum_k |x_k| |y_k| + |b| over the pairs).  An fp32 evaluation in any
order differs from it, in entry (r, k) of the new table, by at most about
    lr (m_r + 8 + 2 (d + 2) S_max) u A[r, k]  +  2 u (|E[r, k]| + lr |G[r, k]|),      u = 2^-24:
  * m_r u A: a sum of m_r fp32 terms in any order (each partial sum is below A in magnitude and is rounded once);
  * 8 u A: the roundings inside one term -- r / n, the product with 1 - sg, the sum of the two directions' ds, the fused
    multiply-adds with the row, lambda times the pair count times the row;
  * 2 (d + 2) S_max u A: an fp32 score carries an error of up to (d + 2) u S (d products, the bias); d(1 - sg)/ds = -sg (1 - sg),
    so 1 - sg changes by at most that RELATIVE amount; doubled for the exponential and the division;
  * 2 u (|E| + lr |G|): lr G rounded, the subtraction rounded.
Not covered term by term: sg itself is rounded to fp32, an ABSOLUTE error of up to u in 1 - sg, i.e. a relative one of u / (1 - sg),
up to 3 000 u at s = 8.  Such a term is as small in A as it is in G, so a row whose pairs ALL had scores near 8 could leave the
band; check_moderate() keeps the scores inside [-8, 8], where they spread like the table's Gaussians, and
tests/test_window_cases_cpu.py measures what is left: the oracle's own fp32 rows, summed in fp32 in a shuffled order, stay below
0.2 of the band on every case.  The same test shows the band is not vacuous: one swapped reward, one dropped pair, one wrong bias
index leave it by a factor of 10 or more.  The bias band is the same with Ab, mb, |b| and |Gb|.
"""
import numpy as np

from oracle import graphgan_oracle as orc
from tests.helpers import load_small

WINDOWS = (1, 2, 3, 5, 64)
WIDE_WINDOW = 2 ** 31 - 1      # must behave exactly like 64 (no path of these graphs has 64 nodes)
DIMS = (8, 50)                 # widths of the deep graph's tables
SEED, STREAM = 9, 1
PASS_LR_GEN = 0.05             # as tests/test_gpu_steps.py: the loss is a mean over thousands of pairs
LAMBDA_GEN = 1e-5
U = 2.0 ** -24
SCORE_LIMIT = 8.0
SCAN_TILE = 2048               # prepare.hip: walks per tile of the pair_ptr scan
TILE_CASES = ((89, 23), (64, 32), (3, 683))   # (slots, walks per root) on "small": 2047, 2048, 2049 walks
DEEP_CHAIN, DEEP_EVERY = 40, 5
DEEP_WALKS, SMALL_WALKS = 2, 20


class Case:
    """One graph with its tables.  walk_E / walk_b: the generator the walks are sampled with; pass_E / pass_b: the generator the
    fused pass runs on (the same arrays on "small"); dis_E / dis_b: the discriminator of the rewards."""

    def __init__(self, name, n, rowptr, col, walk, passing, dis, n_sample):
        self.name, self.n, self.rowptr, self.col = name, n, rowptr, col
        (self.walk_E, self.walk_b), (self.pass_E, self.pass_b), (self.dis_E, self.dis_b) = walk, passing, dis
        self.n_sample = n_sample
        self.d = self.walk_E.shape[1]
        self.swap = self.pass_E is not self.walk_E
        self.roots = np.arange(n, dtype=np.int32)
        self.off, self.nbr, self.base, self.dmax = orc.c_build_trees(n, rowptr, col, self.roots)
        self.stride = self.dmax + 3


def _gauss(rs, n, d, row_scale, bias_scale):
    return (rs.randn(n, d) * row_scale).astype(np.float32), (rs.randn(n) * bias_scale).astype(np.float32)


def _dis_table(n, d, seed, widen=1.0):
    """Gaussian discriminator with scores of standard deviation 3 * widen: some rewards sit at the +10 clip."""
    return _gauss(np.random.RandomState(seed), n, d, np.sqrt(3.0 * widen / np.sqrt(d)), 0.1)


# (seed, widen) of the discriminator per width: the first of a short scan at which even the window-1 pairs -- tree edges only, 94
# distinct ones on "deep" -- have rewards at the +10 clip.  At d = 50 a score is a sum of 50 products and its tails are Gaussian:
# sigma 3 clipped none, 4.5 does.  "small" (d = 6) takes the wider one too.
DIS_TABLE = {8: (300, 1.0), 50: (303, 1.5)}
SMALL_DIS_TABLE = (11, 1.5)


def small_case():
    g, n, graph = load_small(3)
    rowptr, col = orc.graph_to_csr(n, graph)
    E, b = np.ascontiguousarray(g["E"], dtype=np.float32), np.ascontiguousarray(g["b"], dtype=np.float32)
    d = E.shape[1]
    return Case("small", n, rowptr, col, (E, b), (E, b), _dis_table(n, d, *SMALL_DIS_TABLE), SMALL_WALKS)


def deep_graph():
    edges = [(v, v + 1) for v in range(DEEP_CHAIN - 1)]
    edges += [(DEEP_EVERY * j, DEEP_CHAIN + j) for j in range(DEEP_CHAIN // DEEP_EVERY)]
    n = DEEP_CHAIN + DEEP_CHAIN // DEEP_EVERY
    graph = {v: [] for v in range(n)}
    for a, c in edges:
        graph[a].append(c)
        graph[c].append(a)
    return n, graph


def deep_case(d):
    n, graph = deep_graph()
    rowptr, col = orc.graph_to_csr(n, graph)
    rs = np.random.RandomState(100 + d)
    E = (rs.randn(n, d) * 0.05).astype(np.float32)
    E[:DEEP_CHAIN, 0] = (np.sqrt(0.2) * np.arange(DEEP_CHAIN)).astype(np.float32)
    b = (0.1 * np.sin(np.arange(n))).astype(np.float32)
    moderate = _gauss(np.random.RandomState(200 + d), n, d, np.sqrt(1.5 / np.sqrt(d)), 0.3)
    return Case("deep", n, rowptr, col, (E, b), moderate, _dis_table(n, d, *DIS_TABLE[d]), DEEP_WALKS)


# ------------------------------------------------------------------------------------------------ the oracle's walks and pairs
def oracle_walks(case, slots=None, n_sample=None, after_d=False):
    """G-mode walks of the C oracle on the case's walking table: dict(paths, path_len, root_status, ...).  after_d: behind the
    D-mode walks of a prepare_d of all roots (seed SEED, stream 0), which remove father entries from the trees (Q3)."""
    slots = case.roots if slots is None else np.asarray(slots, dtype=np.int32)
    nw = np.full(len(slots), case.n_sample if n_sample is None else n_sample, dtype=np.int32)
    Ep, nbr = orc.pad_rows(case.walk_E), case.nbr
    if after_d:
        nbr = nbr.copy()
        deg = (case.rowptr[1:] - case.rowptr[:-1]).astype(np.int32)
        orc.c_walk_sample(Ep, case.walk_b, case.off, nbr, case.base, case.roots, case.roots, deg, True, SEED, 0, case.stride)
    return orc.c_walk_sample(Ep, case.walk_b, case.off, nbr, case.base, case.roots, slots, nw, False, SEED, STREAM, case.stride)


def expand(walks, window):
    """(node_1, node_2, pairs per walk) of the oracle's walks through orc.pairs_from_path."""
    n1, n2, per = [], [], []
    for w in range(len(walks["path_len"])):
        L = int(walks["path_len"][w])
        pr = orc.pairs_from_path(walks["paths"][w, :L].tolist(), window) if L > 0 else []
        per.append(len(pr))
        n1 += [p[0] for p in pr]
        n2 += [p[1] for p in pr]
    return np.array(n1, dtype=np.int32), np.array(n2, dtype=np.int32), np.array(per, dtype=np.int64)


def path_nodes(walks):
    """L of every walk: nodes of the path once the back-step is dropped."""
    return np.maximum(walks["path_len"].astype(np.int64) - 1, 0)


# ------------------------------------------------------------------------------------------------ float64 SGD step and its band
def sgd_reference(E, b, u, v, r, lam=LAMBDA_GEN, n=None, bias_of=None):
    """One generator gradient on the pair list, float64 from the fp32 inputs (module docstring).  dict(G, Gb, A, Ab, m, mb,
    S_max, s): gradient of the table / bias, the same sums over absolute values, contributions per row, the largest
    sum |x||y| + |b|, the scores.  `n` (the mean's denominator, default: the pairs given) and `bias_of` (the node whose bias
    enters each score, default v) exist for the deliberately wrong variants of tests/test_window_cases_cpu.py."""
    E64, b64 = np.asarray(E, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    r64 = np.asarray(r, dtype=np.float32).astype(np.float64)
    n = len(u) if n is None else n
    bs = b64[v if bias_of is None else np.asarray(bias_of, dtype=np.int64)]
    Eu, Ev = E64[u], E64[v]
    s = np.einsum("ij,ij->i", Eu, Ev) + bs
    S = np.einsum("ij,ij->i", np.abs(Eu), np.abs(Ev)) + np.abs(bs)
    sg = 1.0 / (1.0 + np.exp(-s))
    inside = (sg >= 1e-5) & (sg <= 1.0)
    ds = np.where(inside, -(r64 / n) * (1.0 - sg), 0.0)
    lam = float(np.float32(lam))
    G, A = np.zeros_like(E64), np.zeros_like(E64)
    Gb, Ab = np.zeros_like(b64), np.zeros_like(b64)
    m, mb = np.zeros(len(E64)), np.zeros(len(E64))
    np.add.at(G, u, ds[:, None] * Ev + lam * Eu)
    np.add.at(G, v, ds[:, None] * Eu + lam * Ev)
    np.add.at(A, u, np.abs(ds)[:, None] * np.abs(Ev) + lam * np.abs(Eu))
    np.add.at(A, v, np.abs(ds)[:, None] * np.abs(Eu) + lam * np.abs(Ev))
    np.add.at(Gb, v, ds)
    np.add.at(Ab, v, np.abs(ds))
    np.add.at(m, u, 1.0)
    np.add.at(m, v, 1.0)
    np.add.at(mb, v, 1.0)
    return dict(G=G, Gb=Gb, A=A, Ab=Ab, m=m, mb=mb, S_max=float(S.max(initial=0.0)), s=s, n=n)


def sgd_step(E, b, ref, lr=PASS_LR_GEN):
    """(table, bias) after the step, float64."""
    return np.asarray(E, np.float32).astype(np.float64) - lr * ref["G"], np.asarray(b, np.float32).astype(np.float64) - lr * ref["Gb"]


def bands(E, b, ref, lr=PASS_LR_GEN):
    """(band of every table entry, band of every bias entry) after the step: module docstring."""
    E64, b64 = np.abs(np.asarray(E, np.float32).astype(np.float64)), np.abs(np.asarray(b, np.float32).astype(np.float64))
    d = E64.shape[1]
    sens = 2.0 * (d + 2) * ref["S_max"]
    band_E = lr * (ref["m"][:, None] + 8.0 + sens) * U * ref["A"] + 2.0 * U * (E64 + lr * np.abs(ref["G"]))
    band_b = lr * (ref["mb"] + 8.0 + sens) * U * ref["Ab"] + 2.0 * U * (b64 + lr * np.abs(ref["Gb"]))
    return band_E, band_b


def band_ratio(got_E, got_b, E, b, ref, lr=PASS_LR_GEN):
    """Largest |got - float64 step| / band over the table and the bias (both must be <= 1)."""
    want_E, want_b = sgd_step(E, b, ref, lr)
    band_E, band_b = bands(E, b, ref, lr)
    return (float((np.abs(np.asarray(got_E, dtype=np.float64) - want_E) / band_E).max()),
            float((np.abs(np.asarray(got_b, dtype=np.float64) - want_b) / band_b).max()))


def gradient_share(got_E, got_b, E, b, ref, lr=PASS_LR_GEN):
    """band_ratio with the rounding of the result itself (up to u |got| per entry) taken off the error first: what the gradient's
    sum contributes.  A figure to print -- band_ratio of an exact gradient sits near 0.5 wherever the gradient is small, whatever
    the route; this one tells the routes apart.  Nothing is asserted on it."""
    want_E, want_b = sgd_step(E, b, ref, lr)
    band_E, band_b = bands(E, b, ref, lr)
    gE, gb = np.asarray(got_E, dtype=np.float64), np.asarray(got_b, dtype=np.float64)
    return (float((np.maximum(np.abs(gE - want_E) - U * np.abs(gE), 0.0) / band_E).max()),
            float((np.maximum(np.abs(gb - want_b) - U * np.abs(gb), 0.0) / band_b).max()))


def check_moderate(case, u, v):
    """Every score of the pass table on these pairs lies in [-8, 8]: no pair near the sg >= 1e-5 cut (s = -11.5), where fp32 and
    float64 could disagree about `inside`, and 1 - sigmoid(s) >= 3.3e-4 everywhere."""
    E64, b64 = case.pass_E.astype(np.float64), case.pass_b.astype(np.float64)
    s = np.einsum("ij,ij->i", E64[u], E64[v]) + b64[v]
    assert len(s) > 0 and np.abs(s).max() <= SCORE_LIMIT, (case.name, case.d, float(np.abs(s).max()))
    return s
