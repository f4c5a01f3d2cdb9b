"""Cases of the staged optimizer's bit-identity check, shared by tools/record_staged_golden.py (writes the yardstick with the
build it is run on) and tests/test_gpu_staged_opt_bits.py (replays them and demands the same bits).

The stage rows of a fused pass come from the gradient kernels and are a function of the inputs alone; staged_opt_kernel
sums a row's segment in ascending key order and applies the optimizer, so the resulting tables do not depend on scheduling
and one build reproduces them bit for bit.  A case yields, per pass, the SHA-256 of the embedding table and of the bias
vector, and after the last pass 64 seeded sample rows of both as uint32."""
import hashlib
import os

import numpy as np

N_NODE = 20000
N_CENTRE_IDS = 4000          # centre ids 0 .. 3999, neighbour ids 4000 .. 19999: disjoint ranges
N_CENTRES = 2100             # one run of 8 pairs each: 16 800 pairs (>= 16 384: the staged path)
LENGTHS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64)   # segment lengths that must all occur
HUB_LENGTHS = (65, 80, 130)  # more than 64 gradients: hub rows
ROWS_PER_LENGTH = 3
WIDTHS = (8, 50, 128, 200, 256)
N_SAMPLE = 64


def d_pairs():
    """(u, v, label) of the fused D pass: every centre has one run of 8 pairs, so a centre row gets one gradient and a
    neighbour row as many as its multiplicity in v."""
    rs = np.random.RandomState(11)
    n_pairs = 8 * N_CENTRES
    u = np.repeat(rs.permutation(N_CENTRE_IDS)[:N_CENTRES], 8).astype(np.int32)
    ids = N_CENTRE_IDS + rs.permutation(N_NODE - N_CENTRE_IDS)
    mult = [m for m in LENGTHS[1:] for _ in range(ROWS_PER_LENGTH)] + list(HUB_LENGTHS)
    mult += [1] * (n_pairs - sum(mult))
    assert len(mult) <= len(ids)
    v = np.repeat(ids[: len(mult)], mult).astype(np.int32)
    rs.shuffle(v)
    lab = (rs.rand(n_pairs) < 0.5).astype(np.float32)
    assert len(u) == len(v) == n_pairs >= 16384
    return u, v, lab


def d_tables(d):
    rs = np.random.RandomState(1000 + d)
    Eg = (rs.randn(N_NODE, d) * 0.3).astype(np.float32)
    Ed = (rs.randn(N_NODE, d) * 0.3).astype(np.float32)
    bd = (rs.randn(N_NODE) * 0.1).astype(np.float32)
    return Eg, Ed, bd


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _result(E_b_per_pass):
    """{name: array} of one case from the (E, b) pairs read back after each pass."""
    out = {}
    for k, (E, b) in enumerate(E_b_per_pass):
        out["sha_E_pass%d" % k] = np.array(_digest(E))
        out["sha_b_pass%d" % k] = np.array(_digest(b))
    E, b = E_b_per_pass[-1]
    rows = np.sort(np.random.RandomState(5).choice(E.shape[0], min(N_SAMPLE, E.shape[0]), replace=False))
    out["rows"] = rows.astype(np.int32)
    out["sample_E"] = np.ascontiguousarray(E[rows]).view(np.uint32)
    out["sample_b"] = np.ascontiguousarray(b[rows]).view(np.uint32)
    return out


class _Env:
    """Environment variables of one case (the library reads them when the engine is created or when the pass runs)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_d_case(ga, d, opt, env=None):
    """Two fused D passes, (u, v) and then (v, u): the second reads non-zero moments and needs the reset counts."""
    u, v, lab = d_pairs()
    Eg, Ed, bd = d_tables(d)
    with _Env(env or {}):
        eng = ga.Engine(Eg, Ed, optimizer=ga.GG_OPT_ADAM_LAZY if opt == "lazy" else ga.GG_OPT_SGD)
        eng.set_bias(1, bd)
        passes = []
        for a, b in ((u, v), (v, u)):
            eng.d_step(a, b, lab)
            passes.append((eng.get_embeddings(1), eng.get_bias(1)))
        eng.close()
    return _result(passes)


def run_g_case(ga, opt, env=None):
    """Two whole-walk G passes on the small fixture graph (prepare_g + g_pass over all pairs)."""
    from tests.helpers import load_small
    g, n, graph = load_small(3)
    rs = np.random.RandomState(0)
    Ed = (rs.randn(n, g["E"].shape[1]) * 0.8).astype(np.float32)
    rowptr, col = ga.graph_to_csr(n, graph)
    slots = np.arange(n, dtype=np.int32)
    with _Env(env or {}):
        eng = ga.Engine(g["E"], Ed, optimizer=ga.GG_OPT_ADAM_LAZY if opt == "lazy" else ga.GG_OPT_SGD)
        eng.set_bias(0, g["b"])
        eng.set_graph_csr(rowptr, col)
        eng.build_trees(np.arange(n))
        passes = []
        for rnd in range(2):
            eng.prepare_g(slots, 20, 4, 2 * rnd + 1, fetch=False)
            eng.g_pass([0], 1 << 30)
            passes.append((eng.get_embeddings(0), eng.get_bias(0)))
        eng.close()
    return _result(passes)


def _cases():
    cases = {}
    for d in WIDTHS:
        for opt in ("lazy", "sgd"):
            cases["d_pass-d%d-%s" % (d, opt)] = (run_d_case, dict(d=d, opt=opt))
    cases["d_pass-d128-lazy-replicas2"] = (run_d_case, dict(d=128, opt="lazy", env={"GG_COMM_FAKE_WORLD": "2"}))
    for opt in ("lazy", "sgd"):
        cases["g_pass-early-%s" % opt] = (run_g_case, dict(opt=opt))
        cases["g_pass-noearly-%s" % opt] = (run_g_case, dict(opt=opt, env={"GG_NO_EARLY_SLOTS": "1"}))
    cases["g_pass-minsel-lazy"] = (run_g_case, dict(opt="lazy", env={"GG_STAGE_T": "100000"}))
    cases["g_pass-replicas2-lazy"] = (run_g_case, dict(opt="lazy", env={"GG_COMM_FAKE_WORLD": "2"}))
    return cases


CASES = _cases()


def run_case(ga, name):
    fn, kw = CASES[name]
    return fn(ga, **kw)
