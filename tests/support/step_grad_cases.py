"""Cases of the gradient tests of the pair-list steps (tests/test_gpu_step_grads.py) and their CPU side
(tests/test_step_grad_cases_cpu.py): a float64 restatement of one d_step / g_step gradient, float64 SGD / dense Adam / lazy Adam,
the band a table entry must lie in after a step, the dispatch of run_step restated, and the case lists.  Numpy only; nothing here
touches the engine, and only window_clip_leg(), which takes its graph and walks from window_cases, the oracle.

WHY THESE CONSTANTS.  The suite's other step tests run with lambda = 1e-5 and lr = 1e-3: the regulariser moves an entry by 5e-9,
far below their tolerances, and Adam's m / sqrt(v) hides any factor on a row's gradient.  Here lr = 2^-3 and lambda = 2^-4 (powers of
two: lr G and lambda x are exact), so the L2 term of a row named m times, lambda m x, is of the size of the data term; and the Adam
legs run with adam_eps = 1 >> sqrt(v), where the update is close to lr_t m / eps: linear in the gradient.  Its gain lr_t (1 - b1) is
lr sqrt(1 - b2) = 1.01 at lr = 32, which the generator's batches of up to 64 pairs use.  Larger batches name a row up to 130 times
(lambda m = 8), and the discriminator's data term is a sum, not a mean: they take lr = 4, gain 1 / 8, so that the first step leaves the
scores of the second moderate (check_scores).

THE GRADIENT (header of steps.hip; discriminator.py:21-32, generator.py:22-31).  For the n pairs (u_i, v_i, x_i):
    s_i = E[u_i] . E[v_i] + b[v_i],  sg_i = sigmoid(s_i)
    D:  ds_i = sg_i - x_i                                   G:  ds_i = -(x_i / n) (1 - sg_i), 0 outside 1e-5 <= sg_i <= 1
    G[u_i] += ds_i E[v_i] + lambda E[u_i],   G[v_i] += ds_i E[u_i] + lambda E[v_i],   Gb[v_i] += ds_i (+ lambda b[v_i]: D only)
With k simulated replicas (GG_COMM_FAKE_WORLD=k) n is the pair count of all ranks, k times the list's, and the applied gradient is k
times the local one.

THE BAND OF THE GRADIENT.  An fp32 evaluation in any order differs from the float64 one, in entry (r, c), by at most
    dG = (m_r + 8) u A[r, c] + u Q[r, c],     u = 2^-24
  * m_r u A: a sum of m_r fp32 terms in any order; A is the same sum over absolute values;
  * 8 u A: the roundings inside one term -- x / n, the product with 1 - sg, the two multiply-adds with the rows, lambda times the
    row, the u side's running sum;
  * u Q, Q[r] = sum_i w_i ((d + 2) S_i / 4 + 4) |partner row of i|, w_i = 1 (D) or x_i / n (G): the ABSOLUTE error of sg_i.  An fp32
    score differs from s_i by at most (d + 2) u S_i, S_i = sum_c |x_c| |y_c| + |b| (d products and the bias, any order), and
    d sg / d s = sg (1 - sg) <= 1 / 4; the exponential (2 ulp), 1 + e, the division and sg - x or 1 - sg round once each: 4 u.  Unlike
    window_cases.bands this needs no 1 - sg bounded away from 0, and it covers the discriminator, whose ds = sg - x has no relative
    accuracy at all where sg is close to the label.  P is Q without the bracket: the sum of the partner rows' absolute values.
  * hub rows of a staged pass (more than 64 staged gradients) are summed in 64-bit fixed point: every contribution is rounded to a
    multiple of 1 / scale -- m_r / (2 scale) in all, scale = 2^32 (D) or 2^(32 + floor(log2 n)) (G, hub_scale) -- and the sum is
    rounded to fp32 once, u |G|.  Every row of a staged case gets both terms: which rows are hubs is the kernel's business.
A clipped pair has ds = 0 exactly on both sides, PROVIDED fp32 and float64 agree about `inside`: check_scores keeps every score
0.5 away from the cut at s = -11.51, the clipped ones below -13, all others inside [-8, 8].

THE BAND OF THE STEP.  SGD: lr dG + 2 u (|E| + lr |G|): lr G rounded, the subtraction rounded (window_cases.bands).  Adam
(adam_elem's sequence: m = m b1; m += (1 - b1) g; v = v b2; v += g g (1 - b2); var -= lr_t m / (sqrt(v) + eps)) carries a band on the
moments from step to step, to first order:
    dm' = b1 dm + (1 - b1) dG + 3 u (|b1 m| + |(1 - b1) g|)
    dv' = b2 dv + (1 - b2) (2 |g| dG + dG^2) + 4 u (b2 v + (1 - b2) g^2)
    d sqrt(v') <= min(sqrt(dv'), dv' / (2 sqrt(v')))
    band = lr_t (dm' / den + |m'| d sqrt(v') / den^2) + 6 u |update| + 2 u (|var| + |update|),     den = sqrt(v') - d sqrt(v') + eps >= eps
(6 u |update|: lr_t m, the root, the sum with eps, the quotient, and the same on perturbed operands.  The last term is the rounding of
the new value, u |var'|, taken TWICE, as the SGD band takes it: where the gradient hardly moves an entry this rounding is the whole
error, and a band that its own fp32 reference fills by more than half is rejected by tests/test_step_grad_cases_cpu.py.)
lr_t and the beta powers are fp32 HOST arithmetic of the library, (lr * sqrtf(1 - b2p)) / (1 - b1p) with b1p *= b1 per step; they
are evaluated here in numpy float32, which rounds every operation the same way, and enter the float64 step as inputs (1 - b2p is a
difference of nearly equal numbers: in float64 it would differ by 1e-5 relative).  So do 1 - b1 and 1 - b2.
Lazy Adam is node-granular: a row named by u or v advances its bias too, with gradient 0 where it was only a centre.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
LR_SGD = 2.0 ** -3
LAMBDA = 2.0 ** -4
ADAM_EPS = 1.0
BETA1, BETA2 = 0.9, 0.999
SCORE_LIMIT = 8.0
CLIP_CUT = math.log(1e-5 / (1.0 - 1e-5))    # sigmoid(s) = 1e-5 at s = -11.5129
CLIP_MARGIN = 0.5
COLD_SCORE = -13.0
COLD_DOT = -20.0                            # what the cold rows are built for

# Largest |fp32 reference - float64 step| / band that tests/test_step_grad_cases_cpu.py measures over all cases and both steps, with the
# oracle's fp32 gradient rows summed in fp32 in a shuffled order and the fp32 optimizer (the hub quantisation where a case has hubs).
# The test fails when it measures more, or when this exceeds 0.5.
CPU_FILL = 0.498

# restated from steps.hip / gg_internal.h (tests/test_step_grad_cases_cpu.py checks that the lines are still there)
DET_MAX_PAIRS = 256
DET_LDS_ROW_BYTES = 144 * 1024
SG_THRESHOLD = 64
PPG_LARGE, PPG_MIDDLE = 16384, 2048


def adam_lr(model, n):
    return 32.0 if model == "g" and n <= 64 else 4.0


def mean_off_by_one_visible(n_mean, d):
    """Whether a worst-case fp32 band can tell a generator mean over n + 1 pairs from the mean over n by a factor of 10.  The wrong
    denominator moves a bias gradient Gb = -sum (x / n) (1 - sg) by Gb / (n + 1), about half of sum (x / n) / n for moderate scores; the
    band of that entry is at least u Qb = u sum (x / n) ((d + 2) S / 4 + 4) with S about 0.64 |row|^2 + 0.24 for Gaussian rows and
    biases of deviation 0.3.  Their quotient, 1 / (2 n u ((d + 2) S / 4 + 4)), bounds the factor from above; the roundings of the sum
    and of the bias itself take about half of it again, so it must reach 20.  True for every case up to 2053 pairs (22 at d = 257)
    and at 16384 pairs for d = 6 (73); 10 at d = 65 and 5 at d = 129 there."""
    S = 0.64 * ROW_NORM2(d) + 0.24
    return 1.0 / (2.0 * n_mean * U * ((d + 2) * S / 4.0 + 4.0)) >= 20.0


def hub_scale(per_pair_mean, n):
    return 2.0 ** (32 + (int(math.floor(math.log2(n))) if per_pair_mean and n > 1 else 0))


# ------------------------------------------------------------------------------------------------ the dispatch of run_step
def ld_of(d):
    return (d + 3) // 4 * 4


def nf_of(d, top=32):
    nf = (ld_of(d) + 15) // 16
    return 4 if nf <= 4 else 8 if nf <= 8 else 16 if nf <= 16 or top == 16 else 32


def ppg_of(n):
    return 16 if n >= PPG_LARGE else 4 if n >= PPG_MIDDLE else 1


def rows_fit_lds(n, d):
    return 2 * n * ld_of(d) * 4 <= DET_LDS_ROW_BYTES


def staged(n, d, optimizer, env):
    return (n >= PPG_LARGE and int(env.get("GG_STAGE_T", SG_THRESHOLD)) > 0 and ld_of(d) <= 256 and optimizer != "dense"
            and "GG_NO_STAGED_GRAD" not in env)


def route(n, d, optimizer, env=None):
    """(gradient kernel instance, optimizer kernel) of one d_step / g_step on n pairs of width d; optimizer: "dense", "lazy", "sgd"."""
    env = env or {}
    replicas = int(env.get("GG_COMM_FAKE_WORLD", 0)) > 1
    tail = {"dense": "adam_dense_kernel", "lazy": "sparse_opt_kernel<0>", "sgd": "sparse_opt_kernel<1>"}[optimizer]
    tf = lambda x: "true" if x else "false"
    if env.get("GG_DETERMINISTIC", "1") != "0" and n <= DET_MAX_PAIRS:
        fits = rows_fit_lds(n, d)
        fused = not replicas and optimizer != "dense" and fits and "GG_NO_FUSED_SMALL_STEP" not in env
        opt = (2 if optimizer == "sgd" else 1) if fused else 0
        return "pair_grad_det_kernel<%d,%s,%d,%s>" % (nf_of(d), tf(fits), opt, tf(n <= 64)), "fused" if fused else tail
    ppg = ppg_of(n)
    if staged(n, d, optimizer, env):
        ld = ld_of(d)
        mode = 2 if replicas else 1 if optimizer == "sgd" else 0
        return "pair_grad16_kernel<%d,true>" % nf_of(d, 16), "staged_opt_kernel<%d,%d>+%s" % (mode, 1 if ld <= 64 else 2 if ld <= 128 else 4, tail)
    if ppg == 16 and nf_of(d) <= 16 and "GG_OLD_PAIR_GRAD" not in env:
        return "pair_grad16_kernel<%d,false>" % nf_of(d, 16), tail
    return "pair_grad_kernel<%d,false>@ppg%d" % (nf_of(d), ppg), tail


def stage_counts(n_rows, u, v, ppg=16):
    """Staged gradients per table row as pair_occ_count_kernel counts them: one per pair for v, one per run of equal u inside a group."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    p = np.arange(len(u))
    run_end = (p == len(u) - 1) | ((p + 1) % ppg == 0)
    run_end[:-1] |= u[1:] != u[:-1]
    return np.bincount(v, minlength=n_rows) + np.bincount(u[run_end], minlength=n_rows)


# ------------------------------------------------------------------------------------------------ float64 gradient
def _scatter(n_rows, rows, vals):
    out = np.zeros((n_rows,) + vals.shape[1:])
    if len(rows) == 0:
        return out
    order = np.argsort(rows, kind="stable")
    r = rows[order]
    starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
    out[r[starts]] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def grad_reference(model, E, b, u, v, x, lam=LAMBDA, world=1, mut=None, sums_only=False):
    """The applied gradient of one step of model "d" / "g" on the pair list, float64 from the fp32 inputs (module docstring).
    dict(G, Gb, A, Ab, m, mb, S_max, s, P, Pb, Q, Qb, inside, n).  `mut` holds the deliberately wrong variants of
    tests/test_step_grad_cases_cpu.py: l2_u / l2_v (weight of the L2 term per pair), l2_b (weight of lambda b_v), keep (pairs that
    exist), x (labels / rewards), n_mean (the mean's denominator), force_inside (pairs whose clip is ignored), row_gain {row: factor}.
    sums_only: G and Gb alone (what a wrong variant is needed for)."""
    mut = mut or {}
    E64, b64 = np.asarray(E, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    x64 = np.asarray(mut.get("x", x), dtype=np.float32).astype(np.float64)
    n, n_rows, d = len(u), len(E64), E64.shape[1]
    n_mean = mut.get("n_mean", n * world)
    lam = float(np.float32(lam))
    Eu, Ev, bv = E64[u], E64[v], b64[v]
    aEu, aEv = np.abs(Eu), np.abs(Ev)
    s = np.einsum("ij,ij->i", Eu, Ev) + bv
    S = np.einsum("ij,ij->i", aEu, aEv) + np.abs(bv)
    sg = 1.0 / (1.0 + np.exp(-s))
    keep = np.asarray(mut.get("keep", np.ones(n, bool)), dtype=np.float64)
    if model == "d":
        inside = np.ones(n, bool)
        ds, w = sg - x64, np.ones(n)
    else:
        inside = ((sg >= 1e-5) & (sg <= 1.0)) | np.asarray(mut.get("force_inside", np.zeros(n, bool)))
        ds, w = np.where(inside, -(x64 / n_mean) * (1.0 - sg), 0.0), np.where(inside, np.abs(x64) / n_mean, 0.0)
    ds, w = ds * keep, w * keep
    l2u = lam * keep * np.asarray(mut.get("l2_u", np.ones(n)), dtype=np.float64)
    l2v = lam * keep * np.asarray(mut.get("l2_v", np.ones(n)), dtype=np.float64)
    l2b = lam * keep * mut.get("l2_b", 1.0 if model == "d" else 0.0)
    sens = w * ((d + 2) * S / 4.0 + 4.0)
    rows = np.concatenate([u, v])
    ads = np.abs(ds)
    G = _scatter(n_rows, rows, np.concatenate([ds[:, None] * Ev + l2u[:, None] * Eu, ds[:, None] * Eu + l2v[:, None] * Ev]))
    Gb = _scatter(n_rows, v, ds + l2b * bv)
    for r, gain in mut.get("row_gain", {}).items():
        G[r] *= gain
        Gb[r] *= gain
    k = float(world)   # every simulated rank brings this rank's gradient: an exact factor on the sum and on its error
    if sums_only:
        return dict(G=k * G, Gb=k * Gb)
    A = _scatter(n_rows, rows, np.concatenate([ads[:, None] * aEv + l2u[:, None] * aEu, ads[:, None] * aEu + l2v[:, None] * aEv]))
    P = _scatter(n_rows, rows, np.concatenate([w[:, None] * aEv, w[:, None] * aEu]))
    Q = _scatter(n_rows, rows, np.concatenate([sens[:, None] * aEv, sens[:, None] * aEu]))
    Ab = _scatter(n_rows, v, ads + l2b * np.abs(bv))
    Pb, Qb = _scatter(n_rows, v, w), _scatter(n_rows, v, sens)
    m = np.bincount(rows, weights=np.concatenate([keep, keep]), minlength=n_rows).astype(np.float64)
    mb = np.bincount(v, weights=keep, minlength=n_rows).astype(np.float64)
    return dict(G=k * G, Gb=k * Gb, A=k * A, Ab=k * Ab, m=m, mb=mb, S_max=float(S.max(initial=0.0)), s=s, P=k * P, Pb=k * Pb, Q=k * Q, Qb=k * Qb,
                inside=inside, n=n, world=world)


def grad_bands(ref, scale=None):
    """(dG, dGb) of the module docstring; scale: the fixed-point scale of a staged pass, or None."""
    dG = (ref["m"][:, None] + 8.0) * U * ref["A"] + U * ref["Q"]
    dGb = (ref["mb"] + 8.0) * U * ref["Ab"] + U * ref["Qb"]
    if scale is not None:
        dG = dG + ref["world"] * ref["m"][:, None] / (2.0 * scale) + U * np.abs(ref["G"])
        dGb = dGb + ref["world"] * ref["mb"] / (2.0 * scale) + U * np.abs(ref["Gb"])
    return dG, dGb


def check_scores(model, ref, cold=None):
    """Every score at most 8 in magnitude, except the pairs named cold, which lie below -13: no score within 0.5 of the clip's cut."""
    s = ref["s"]
    cold = np.zeros(len(s), bool) if cold is None else np.asarray(cold, bool)
    assert model == "g" or not cold.any()
    assert len(s) > 0 and np.abs(s[~cold]).max(initial=0.0) <= SCORE_LIMIT, float(np.abs(s[~cold]).max())
    assert (s[cold] <= COLD_SCORE).all() and COLD_SCORE <= CLIP_CUT - CLIP_MARGIN
    assert np.array_equal(ref["inside"], ~cold)
    return s


# ------------------------------------------------------------------------------------------------ float64 optimizers
def f32(x):
    return np.float32(x)


class OptState:
    """Moments of table and bias (float64), their bands, and the fp32 beta powers of the library's host side."""

    def __init__(self, shape_E):
        z = lambda s: np.zeros(s)
        self.m, self.v, self.dm, self.dv = [z(shape_E), z(shape_E[0])], [z(shape_E), z(shape_E[0])], [z(shape_E), z(shape_E[0])], [z(shape_E), z(shape_E[0])]
        self.b1p, self.b2p, self.t = f32(BETA1), f32(BETA2), 0

    def lr_t(self, lr):
        return float((f32(lr) * np.sqrt(f32(1) - self.b2p)) / (f32(1) - self.b1p))


def opt_step(kind, E, b, G, Gb, dG, dGb, touched, state, lr, eps=ADAM_EPS):
    """One step of "sgd" / "dense" / "lazy" from the fp32 tables: (E', b', band of E', band of b'), float64; `state` advances.
    touched: the rows the pair list names (lazy Adam updates these, table row and bias).  A band of 0 means: the exact bits."""
    E64, b64 = np.asarray(E, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    out = []
    if kind == "sgd":
        for var, g, dg in ((E64, G, dG), (b64, Gb, dGb)):
            out.append((var - lr * g, lr * dg + 2.0 * U * (np.abs(var) + lr * np.abs(g))))
    else:
        b1, b2 = float(f32(BETA1)), float(f32(BETA2))
        c1, c2 = float(f32(1) - f32(BETA1)), float(f32(1) - f32(BETA2))
        lr_t, eps = state.lr_t(lr), float(f32(eps))
        for i, (var, g, dg) in enumerate(((E64, G, dG), (b64, Gb, dGb))):
            rows = np.ones(len(var), bool) if kind == "dense" else np.asarray(touched, bool)
            m0, v0, dm0, dv0 = state.m[i][rows], state.v[i][rows], state.dm[i][rows], state.dv[i][rows]
            g, dg = g[rows], dg[rows]
            m1 = b1 * m0 + c1 * g
            dm1 = b1 * dm0 + c1 * dg + 3.0 * U * (np.abs(b1 * m0) + np.abs(c1 * g))
            v1 = b2 * v0 + c2 * g * g
            dv1 = b2 * dv0 + c2 * (2.0 * np.abs(g) * dg + dg * dg) + 4.0 * U * v1
            sq = np.sqrt(v1)
            with np.errstate(divide="ignore", invalid="ignore"):
                dsq = np.where(sq > 0, np.minimum(np.sqrt(dv1), dv1 / (2.0 * sq)), np.sqrt(dv1))
            upd = lr_t * m1 / (sq + eps)
            den = np.maximum(sq - dsq, 0.0) + eps
            band = lr_t * (dm1 / den + np.abs(m1) * dsq / (den * den)) + 6.0 * U * np.abs(upd) + 2.0 * U * (np.abs(var[rows]) + np.abs(upd))
            band = np.where((m1 == 0) & (dm1 == 0), 0.0, band)   # no moment, no gradient: var - 0 is var
            new, bnd = var.copy(), np.zeros_like(var)
            new[rows], bnd[rows] = var[rows] - upd, band
            state.m[i][rows], state.v[i][rows], state.dm[i][rows], state.dv[i][rows] = m1, v1, dm1, dv1
            out.append((new, bnd))
        state.b1p, state.b2p = f32(state.b1p * f32(BETA1)), f32(state.b2p * f32(BETA2))
    state.t += 1
    return out[0][0], out[1][0], out[0][1], out[1][1]


def ratio(got, want, band):
    """Largest |got - want| / band; inf when an entry with band 0 differs at all."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if (err[band == 0] != 0).any():
        return float("inf")
    pos = band > 0
    return float((err[pos] / band[pos]).max(initial=0.0))


# ------------------------------------------------------------------------------------------------ tables and pair lists
C0, W0, SELF = 0, 1, 2                     # small batches: the centre of half the batch, the neighbour of half, the self-pair row
HUB_V = ((10, 70), (11, 100), (12, 130))   # large batches: (row, pairs that name it as v)
HUB_U, HUB_U_RUNS = 13, 90                 # ... a row that is the centre of 90 scattered single pairs
T64, T65 = 14, 15                          # ... rows with exactly 64 and 65 staged gradients
FIRST_FREE = 20                            # rows below are named only on purpose; 3 .. 9 and 16 .. 19 never: untouched rows
TABLE_ROWS = {"small": 600, "middle": 1000, "large": 4000}
REPEATS = 4


def ROW_NORM2(d):
    """|row|^2 of the Gaussian tables: 0.8 sqrt(d) (scores of standard deviation 0.8) up to d = 25, then 4 (standard deviation 4 / sqrt(d)).  One
    step moves the score of a pair by about lr |ds| |row|^2 per time the pair's rows are named together: wide rows of norm^2 sqrt(d)
    would carry the scores of the second step past 8; and a sum of 6 products has heavy tails."""
    return min(0.8 * math.sqrt(d), 4.0)


RUN = {"small": 1, "middle": 6, "runs8": 8, "runs5": 5, "none": 1}


class Batch:
    """One table of model "d" / "g" and the two pair lists of a case.  cold[k]: the clipped pairs of list k."""

    def __init__(self, model, n, d, layout, clip):
        self.model, self.n, self.d, self.layout, self.clip = model, n, d, layout, clip
        kind = layout if layout in ("small", "middle") else "large"
        n_cold = max(1, n // 10) if clip else 0
        base = TABLE_ROWS[kind]
        self.n_rows = base + 2 * n_cold
        rs = np.random.RandomState(1000 * (n % 997) + 7 * d + (model == "g") + 2 * clip + 4 * len(layout))
        E = rs.randn(self.n_rows, d) * math.sqrt(ROW_NORM2(d) / d)
        b = 0.3 * rs.randn(self.n_rows)
        E[SELF] *= min(1.0, math.sqrt(2.0 / float(E[SELF] @ E[SELF])))   # a self pair scores |x|^2
        if clip:   # cold rows: base + j scores COLD_DOT with base + n_cold + j', whatever j and j'; no other pair names them
            w = rs.randn(d)
            w *= math.sqrt(-COLD_DOT) / np.linalg.norm(w)
            noise = 0.02 * d ** -0.5
            E[base:base + n_cold] = w + noise * rs.randn(n_cold, d)
            E[base + n_cold:] = -w + noise * rs.randn(n_cold, d)
        self.E, self.b = E.astype(np.float32), b.astype(np.float32)
        self.steps, self.cold = [], []
        for k in range(2):
            u, v, cold = self._pairs(rs, kind, base, n_cold, k)
            x = (rs.rand(n) < 0.5).astype(np.float32) if model == "d" else (rs.rand(n) * 2).astype(np.float32)
            for a in (u, v, x, cold):
                a.flags.writeable = False
            self.steps.append((u, v, x))
            self.cold.append(cold)
        self.E.flags.writeable = self.b.flags.writeable = False

    def _pairs(self, rs, kind, base, n_cold, k):
        n, run = self.n, RUN[self.layout]
        lo = 10 if kind != "large" else FIRST_FREE
        u = np.repeat(rs.randint(lo, base, (n + run - 1) // run), run)[:n].astype(np.int32)
        v = rs.randint(lo, base, n).astype(np.int32)
        same = u == v                                      # self pairs are made on purpose only, of a row scaled for it
        v[same] = lo + (v[same] - lo + 1) % (base - lo)
        cold = np.zeros(n, bool)
        if kind == "small":
            u[:n // 2] = C0
            rep = min(REPEATS, n // 2)
            v[n // 2 - rep:n - rep] = W0                   # ... of which `rep` pairs are (C0, W0): the same pair repeated
            if n >= 8:
                u[-1] = v[-1] = u[-2] = v[-2] = SELF
                u[-3], v[-4] = W0, C0                      # rows named on both sides
            free = n - 5 - np.arange(n_cold)
        elif kind == "middle":
            u[-1] = v[-1] = SELF
            v[-2] = u[0]
            free = n - 5 - np.arange(n_cold)
        else:
            pos, at = rs.permutation(n), 0
            for row, cnt in HUB_V + ((T64, 64), (T65, 65)):
                v[pos[at:at + cnt]] = row
                at += cnt
            u[pos[at:at + HUB_U_RUNS]] = HUB_U
            at += HUB_U_RUNS
            u[pos[at]] = v[pos[at]] = SELF
            free = pos[at + 1:at + 1 + n_cold]
        if n_cold:
            j = np.arange(n_cold)
            u[free], v[free], cold[free] = base + j, base + n_cold + (j + k) % n_cold, True
        return u, v, cold


@functools.lru_cache(maxsize=8)
def batch(model, n, d, layout, clip=False):
    return Batch(model, n, d, layout, clip)


class Case:
    def __init__(self, model, n, d, layout, optimizer, env=(), clip=False):
        self.model, self.n, self.d, self.layout, self.optimizer, self.clip = model, n, d, layout, optimizer, clip
        self.env = dict(env)
        self.world = int(self.env.get("GG_COMM_FAKE_WORLD", 1))
        self.lr = LR_SGD if optimizer == "sgd" else adam_lr(model, n)
        self.route = route(n, d, optimizer, self.env)
        self.staged = staged(n, d, optimizer, self.env)
        self.scale = hub_scale(model == "g", n) if self.staged else None
        tag = "-".join("%s=%s" % (k[3:].lower(), val) for k, val in sorted(self.env.items()))
        self.id = "%s-n%d-d%d-%s-%s%s%s" % (model, n, d, layout, optimizer, "-clip" if clip else "", "-" + tag if tag else "")

    def batch(self):
        return batch(self.model, self.n, self.d, self.layout, self.clip)

    def batch_key(self):
        return (self.model, self.n, self.d, self.layout, self.clip, self.world, self.staged)

    def __repr__(self):
        return self.id


SMALL_N, SMALL_D = (1, 37, 64, 65, 256), (6, 50, 65, 129, 257)
LDS_EDGE = ((64, 288), (64, 289), (256, 73))          # n ld <= 18432: (64, 288) and (256, 65) fit, (64, 289) and (256, 73) do not
NO_FUSED, ATOMIC = {"GG_NO_FUSED_SMALL_STEP": "1"}, {"GG_DETERMINISTIC": "0"}
MIDDLE_N, MIDDLE_D = (300, 2047, 2048, 2053), (6, 65, 129, 257)
LARGE_N, LARGE_D = (16384, 16389), (6, 65, 129, 256)
DECLINED_D = 260
LARGE_ROUTES = (("lazy", {}), ("sgd", {}), ("lazy", {"GG_STAGE_T": "0"}), ("dense", {}), ("sgd", {"GG_OLD_PAIR_GRAD": "1", "GG_NO_STAGED_GRAD": "1"}),
                ("lazy", {"GG_NO_STAGED_GRAD": "1"}), ("lazy", {"GG_COMM_FAKE_WORLD": "2"}), ("sgd", {"GG_COMM_FAKE_WORLD": "2"}))


def _small_cases():
    out = []
    shapes = [(n, d) for n in SMALL_N for d in SMALL_D] + list(LDS_EDGE)
    for i, (n, d) in enumerate(shapes):
        kinds = [("dense", {}), ("lazy", {}), ("sgd", {}), ("lazy", NO_FUSED), ("sgd", NO_FUSED), ("lazy", ATOMIC), ("sgd", ATOMIC), ("dense", ATOMIC)]
        for j, (opt, env) in enumerate(kinds):
            out.append(Case("dg"[(i + j) % 2], n, d, "small", opt, env))
    return out


def _middle_cases():
    out = []
    for i, n in enumerate(MIDDLE_N):
        for j, opt in enumerate(("lazy", "sgd", "dense")):
            for k, model in enumerate("dg"):
                out.append(Case(model, n, MIDDLE_D[(i // 2 * 3 + j + 2 * k) % 4], "middle", opt))
    return out


def _large_cases():
    out, layouts = [], ("runs8", "runs5", "none")
    for i, d in enumerate(LARGE_D):
        for j, (opt, env) in enumerate(LARGE_ROUTES):
            model = "dg"[(i + j) % 2]
            out.append(Case(model, LARGE_N[(i + j // 2) % 2], d, "runs8" if model == "d" and j < 2 else layouts[(i + j) % 3], opt, env))
    for j, (opt, env) in enumerate(LARGE_ROUTES[:2] + LARGE_ROUTES[3:4]):   # staging declined above ld = 256
        out.append(Case("dg"[j % 2], LARGE_N[(j + 1) % 2], DECLINED_D, layouts[j], opt, env))
    return out


def _clip_cases():
    return [Case("g", 64, 50, "small", "lazy", clip=True), Case("g", 64, 50, "small", "sgd", clip=True), Case("g", 256, 65, "small", "dense", clip=True),
            Case("g", 300, 65, "middle", "sgd", clip=True), Case("g", 2048, 6, "middle", "lazy", clip=True),
            Case("g", 16384, 65, "runs5", "sgd", clip=True), Case("g", 16389, 129, "none", "lazy", clip=True)]


SMALL_CASES, MIDDLE_CASES, LARGE_CASES, CLIP_CASES = _small_cases(), _middle_cases(), _large_cases(), _clip_cases()
CASES = SMALL_CASES + MIDDLE_CASES + LARGE_CASES + CLIP_CASES
assert len({c.id for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------ one case, step by step
class Walker:
    """The float64 side of a case: reference(k, E, b) is the gradient of pair list k on the fp32 tables (E, b); advance() applies
    it with the case's optimizer and returns (E', b', band of E', band of b')."""

    def __init__(self, case):
        self.case, self.b = case, case.batch()
        self.state = OptState(self.b.E.shape)

    def reference(self, k, E, b, mut=None, sums_only=False):
        u, v, x = self.b.steps[k]
        return grad_reference(self.case.model, E, b, u, v, x, LAMBDA, self.case.world, mut, sums_only)

    def touched(self, k):
        u, v, _ = self.b.steps[k]
        t = np.zeros(self.b.n_rows, bool)
        t[u] = t[v] = True
        return t

    def advance(self, k, E, b, ref, applied=None, state=None):
        """applied: a (wrong) gradient to apply in place of ref's; the band is always ref's."""
        dG, dGb = grad_bands(ref, self.case.scale)
        g = applied or ref
        return opt_step(self.case.optimizer, E, b, g["G"], g["Gb"], dG, dGb, self.touched(k), state or self.state, self.case.lr)


# ------------------------------------------------------------------------------------------------ one whole-walk pass with clipped pairs
WINDOW_LEG_LR = 2.0 ** -8     # the rows of this 90-node graph are named by hundreds of the pass's 6 500 pairs: lr lambda m stays below 1
WINDOW_LEG_COLD_BIAS = -22.0


def window_clip_leg():
    """window_cases' "small" graph at window 2 with a pass table whose scores are moderate, except that a tenth of the pairs end in a
    node with bias -22: s = E[u] . E[v] + b[v] <= -14 there, the data term of those pairs is exactly zero and their L2 term remains.
    (case, u, v, cold): the window_cases.Case (pass table swapped in behind the walks), the oracle's pairs, the clipped ones."""
    from tests.support import window_cases as wc
    base = wc.small_case()
    rs = np.random.RandomState(77)
    E, b = wc._gauss(rs, base.n, base.d, math.sqrt(1.5 / math.sqrt(base.d)), 0.3)
    u, v, _ = wc.expand(wc.oracle_walks(base), 2)
    cnt, total, cold_nodes = np.bincount(v, minlength=base.n), 0, []
    for node in rs.permutation(base.n):
        if cnt[node] > 0 and total + cnt[node] <= len(v) // 10:
            cold_nodes.append(node)
            total += cnt[node]
    b[cold_nodes] = WINDOW_LEG_COLD_BIAS
    case = wc.Case("small", base.n, base.rowptr, base.col, (base.walk_E, base.walk_b), (E, b), (base.dis_E, base.dis_b), wc.SMALL_WALKS)
    return case, u, v, np.isin(v, cold_nodes)


def window_leg_step(case, u, v, rew, staged_route, mut=None):
    """(reference, E', b', band of E', band of b') of the pass: one SGD step of the generator on the walks' pairs."""
    ref = grad_reference("g", case.pass_E, case.pass_b, u, v, rew, LAMBDA, 1, mut)
    dG, dGb = grad_bands(ref, hub_scale(True, len(u)) if staged_route else None)
    return (ref,) + opt_step("sgd", case.pass_E, case.pass_b, ref["G"], ref["Gb"], dG, dGb, None, OptState(case.pass_E.shape), WINDOW_LEG_LR)
