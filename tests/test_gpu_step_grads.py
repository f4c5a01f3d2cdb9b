"""The gradients of d_step / g_step against a float64 restatement, with a regulariser and a gradient scale that can be seen, on
every route of run_step's dispatch (cases, restatement and bands: tests/support/step_grad_cases.py; their premises, among them that
every wrong L2 term, wrong 1 / n, doubled hub row or ignored clip leaves the band by a factor of 10: tests/test_step_grad_cases_cpu.py).

Each case makes one engine with lr = 2^-3 (SGD) or 4 / 32 with adam_eps = 1 (Adam) and lambda = 2^-4, takes two steps on two pair
lists -- the second reads non-zero moments, advanced beta powers and reset stage counts -- and requires, after each,
|table - float64 step| <= band on the whole table and the whole bias; the float64 step starts from the fp32 tables the engine held
before the step.  Rows that no pair names keep their bits under every optimizer here (dense Adam decays them, but their moments
are zero).  Set GG_STEP_GRAD_ERRTOL to a path to get the err / band of every case appended there.

Measured on an MI355X: err / band at most 0.497 on any case, on most between 0.4 and 0.5 -- as in tests/test_gpu_window.py it is the rounding of the new
value itself, which the band allows twice, on an entry the gradient hardly moves.  With that rounding taken off, the gradient's share of
the band is at most 0.14 (pair_grad_kernel with atomics), 0.12 (pair_grad16_kernel, staged or not) and 0.10 (pair_grad_det_kernel,
fused or not); 0.015 on the whole-walk pass."""
import os

import numpy as np
import pytest

from tests.support import step_grad_cases as sg

pytestmark = pytest.mark.gpu

CASE_ENV = ("GG_DETERMINISTIC", "GG_NO_FUSED_SMALL_STEP", "GG_STAGE_T", "GG_OLD_PAIR_GRAD", "GG_NO_STAGED_GRAD", "GG_COMM_FAKE_WORLD",
            "GG_COMM_DENSE_RATIO", "GG_COMM_OWNER", "GG_COMM_OWNER_MIN", "GG_COMM_BF16", "GG_STAGE_MAX_BYTES", "GG_DET_WORKGROUPS")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in CASE_ENV:
        monkeypatch.delenv(name, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def share(got, want, band):
    """sg.ratio with the rounding of the result itself (up to u |got| per entry) taken off the error: the gradient's part.  Printed only."""
    err = np.maximum(np.abs(got.astype(np.float64) - want) - sg.U * np.abs(got), 0.0)
    return float((err[band > 0] / band[band > 0]).max(initial=0.0))


def report(line):
    print(line)
    path = os.environ.get("GG_STEP_GRAD_ERRTOL")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def run_case(ga, case, monkeypatch, check=True):
    """Both steps of the case on a fresh engine; (table, bias) after the second.  check: every step against its band."""
    for name, value in case.env.items():   # gg_create reads most of them, the step the rest: set through both
        monkeypatch.setenv(name, value)
    bt, which = case.batch(), 1 if case.model == "d" else 0
    opt = {"sgd": ga.GG_OPT_SGD, "lazy": ga.GG_OPT_ADAM_LAZY, "dense": ga.GG_OPT_ADAM_DENSE}[case.optimizer]
    eng = ga.Engine(bt.E, bt.E, lr_gen=case.lr, lr_dis=case.lr, lambda_gen=sg.LAMBDA, lambda_dis=sg.LAMBDA, adam_eps=sg.ADAM_EPS, optimizer=opt)
    eng.set_bias(which, bt.b)
    walker = sg.Walker(case)
    E, b = bt.E, bt.b
    named = np.zeros(bt.n_rows, bool)
    ratios = []
    for k, (u, v, x) in enumerate(bt.steps):
        (eng.d_step if which == 1 else eng.g_step)(u, v, x)
        got_E, got_b = eng.get_embeddings(which), eng.get_bias(which)
        assert got_E.shape == bt.E.shape and got_E.dtype == np.float32
        named |= walker.touched(k)
        if check:
            ref = walker.reference(k, E, b)
            sg.check_scores(case.model, ref, bt.cold[k])
            want_E, want_b, band_E, band_b = walker.advance(k, E, b, ref)
            ratios.append((sg.ratio(got_E, want_E, band_E), sg.ratio(got_b, want_b, band_b), max(share(got_E, want_E, band_E), share(got_b, want_b, band_b))))
            assert np.abs(got_E - E).max() > 1e-3                                       # the step moved the table
            assert (~named).sum() >= 7
            assert np.array_equal(bits(got_E[~named]), bits(bt.E[~named])) and np.array_equal(bits(got_b[~named]), bits(bt.b[~named])), k
        E, b = got_E, got_b
    other = eng.get_embeddings(1 - which)
    assert np.array_equal(bits(other), bits(bt.E))                                        # the other model's table is not written
    eng.close()
    for name in case.env:
        monkeypatch.delenv(name)
    if check:
        report("%s [%s]: err/band step 1 table %.3f bias %.3f, step 2 table %.3f bias %.3f (gradient's share %.3f %.3f)" %
               (case.id, " + ".join(case.route), ratios[0][0], ratios[0][1], ratios[1][0], ratios[1][1], ratios[0][2], ratios[1][2]))
        for k, (rE, rb, _) in enumerate(ratios):
            assert rE <= 1.0 and rb <= 1.0, (case.id, case.route, k, rE, rb)
    return E, b


UNFUSED = [c for c in sg.SMALL_CASES if c.env == sg.NO_FUSED and sg.rows_fit_lds(c.n, c.d)]
STAGED_LAZY = [c for c in sg.LARGE_CASES + sg.CLIP_CASES if c.staged and c.optimizer == "lazy" and c.world == 1]


def fused_twin(case):
    return next(c for c in sg.SMALL_CASES if c.batch_key() == case.batch_key() and c.optimizer == case.optimizer and c.route[1] == "fused")


# The bit comparisons below need the final tables of these cases only.  The band test leaves them here so that the comparisons
# do not run the same engines again; a comparison that finds no entry (a -k selection, another order) runs the case itself, so
# nothing depends on which tests ran before.
COMPARED = {c.id for c in UNFUSED + [fused_twin(c) for c in UNFUSED] + STAGED_LAZY}
FINAL = {}


def final_tables(ga, case, monkeypatch):
    return FINAL[case.id] if case.id in FINAL else run_case(ga, case, monkeypatch, check=False)


@pytest.mark.parametrize("case", sg.CASES, ids=[c.id for c in sg.CASES])
def test_two_steps_stay_inside_the_band(ga, case, monkeypatch):
    tabs = run_case(ga, case, monkeypatch)
    if case.id in COMPARED:
        FINAL[case.id] = tabs


@pytest.mark.parametrize("case", UNFUSED, ids=[c.id for c in UNFUSED])
def test_fused_small_step_has_the_bits_of_the_unfused_one(ga, case, monkeypatch):
    """pair_grad_det_kernel<.., OPT = 1 / 2> applies opt_row's operation sequence to the sum it holds in registers: the bits of the
    gradient kernel + flag compaction + sparse_opt_kernel."""
    assert case.route[1].startswith("sparse_opt_kernel") and case.route[0].split(",")[2] == "0"
    tabs = [final_tables(ga, c, monkeypatch) for c in (case, fused_twin(case))]
    assert np.array_equal(bits(tabs[0][0]), bits(tabs[1][0])) and np.array_equal(bits(tabs[0][1]), bits(tabs[1][1]))


@pytest.mark.parametrize("case", STAGED_LAZY, ids=[c.id for c in STAGED_LAZY])
def test_staged_lazy_steps_are_bit_reproducible(ga, case, monkeypatch):
    """Stage segments are summed in key order and hub rows in fixed point: a repeated run gives the same bits."""
    first = final_tables(ga, case, monkeypatch)
    again = run_case(ga, case, monkeypatch, check=False)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(bits(first[1]), bits(again[1]))


# ------------------------------------------------------------------------------------------------ the whole-walk pass
@pytest.fixture(scope="module")
def leg():
    return sg.window_clip_leg()


@pytest.mark.parametrize("route,env", [("staged", {}), ("atomic", {"GG_STAGE_T": "0"}), ("hubs", {"GG_STAGE_T": "3"})], ids=["staged", "atomic", "hubs"])
def test_whole_walk_pass_with_clipped_pairs_and_a_visible_regulariser(ga, leg, route, env, monkeypatch):
    """path_grad_kernel on window_cases' "small" graph, window 2, lambda = 2^-4, SGD: a tenth of the pairs end in a node with bias -22
    and are clipped -- their data term is exactly zero, their L2 term (lam_n = lambda * npair) remains.  The pass table is swapped in
    behind the walks as tests/test_gpu_window.py does it."""
    from tests.support import window_cases as wc
    case, want_u, want_v, cold = leg
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    eng = ga.Engine(case.walk_E, case.dis_E, window_size=2, optimizer=ga.GG_OPT_SGD, lr_gen=sg.WINDOW_LEG_LR, lambda_gen=sg.LAMBDA)
    eng.set_bias(0, case.walk_b)
    eng.set_bias(1, case.dis_b)
    eng.set_graph_csr(case.rowptr, case.col)
    eng.build_trees(case.roots)
    u, v, rew, _ = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM)
    assert np.array_equal(u, want_u) and np.array_equal(v, want_v)
    eng.set_embeddings(0, case.pass_E)
    eng.set_bias(0, case.pass_b)
    eng.g_pass([0], len(u))
    got_E, got_b = eng.get_embeddings(0), eng.get_bias(0)
    assert eng.counters()["g_steps"] == 1
    eng.close()
    for name in env:
        monkeypatch.delenv(name)
    ref, want_E, want_b, band_E, band_b = sg.window_leg_step(case, u, v, rew, route != "atomic")
    sg.check_scores("g", ref, cold)
    rE, rb = sg.ratio(got_E, want_E, band_E), sg.ratio(got_b, want_b, band_b)
    report("whole-walk pass, %s: %d pairs, %d clipped, err/band table %.3f bias %.3f (gradient's share %.3f)" %
           (route, len(u), int(cold.sum()), rE, rb, max(share(got_E, want_E, band_E), share(got_b, want_b, band_b))))
    assert np.abs(got_E - case.pass_E).max() > 1e-3
    assert rE <= 1.0 and rb <= 1.0, (route, rE, rb)
