"""The generator's half of a training step at window sizes 1, 3 and up, and on deep paths (cases and the band:
tests/support/window_cases.py; their premises: tests/test_window_cases_cpu.py).

window_size selects three routes: path_reward_kernel (window <= 2) or pair_fill + pair_reward_kernel behind the walks; the
whole-walk path_grad_kernel (window <= 2) or the generic pair kernels; the early staging index (window <= 2) or none.  Window 1
runs the whole-walk kernels' index arithmetic on another pair layout than window 2, and has its own stage-size bound.  The "deep"
graph (stride 43) runs the SHORT = false instances: ids and stage slots from memory at positions >= 16, rewards from memory for a
walk's pairs from 64 on.  Walk counts of 2047, 2048 and 2049 put the pair_ptr scan on both sides of one tile."""
import types

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.support import window_cases as wc

pytestmark = pytest.mark.gpu

CASES = [("small", None)] + [("deep", d) for d in wc.DIMS]
CASE_IDS = ["small"] + ["deep%d" % d for d in wc.DIMS]
CLIP = np.log1p(np.exp(10.0))
STAGE_ENV = ("GG_STAGE_T", "GG_NO_PATH_GRAD", "GG_NO_PATH_REWARD", "GG_NO_EARLY_SLOTS", "GG_NO_STAGED_GRAD")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def refs():
    """The cases with the oracle's walks, and their pairs per window: computed once, shared, never written to."""
    out = {}
    for key in CASES:
        case = wc.small_case() if key[0] == "small" else wc.deep_case(key[1])
        walks = wc.oracle_walks(case)
        pairs = {}
        for window in wc.WINDOWS + (wc.WIDE_WINDOW,):
            u, v, _ = wc.expand(walks, min(window, 64))   # (2^31 - 1 == 64: tests/test_window_cases_cpu.py)
            u.flags.writeable = v.flags.writeable = False
            pairs[window] = (u, v)
        out[key] = types.SimpleNamespace(case=case, walks=walks, pairs=pairs)
    return out


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in STAGE_ENV:
        monkeypatch.delenv(name, raising=False)


def make_engine(ga, case, window, **kw):
    eng = ga.Engine(case.walk_E, case.dis_E, window_size=window, **kw)
    eng.set_bias(0, case.walk_b)
    eng.set_bias(1, case.dis_b)
    eng.set_graph_csr(case.rowptr, case.col)
    eng.build_trees(case.roots)
    assert eng.max_depth + 3 == case.stride
    return eng


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def swap_in_pass_table(eng, case, u, v, rew):
    """The moderate generator of the deep cases; walks, pairs and rewards stay resident across the upload."""
    if not case.swap:
        return
    eng.set_embeddings(0, case.pass_E)
    eng.set_bias(0, case.pass_b)
    u2, v2, rew2 = eng.get_g_data()
    assert np.array_equal(u2, u) and np.array_equal(v2, v) and np.array_equal(bits(rew2), bits(rew))


# ------------------------------------------------------------------------------------------------ a, b: pairs and rewards
@pytest.mark.parametrize("window", wc.WINDOWS + (wc.WIDE_WINDOW,))
@pytest.mark.parametrize("key", CASES, ids=CASE_IDS)
def test_pairs_and_rewards(ga, refs, key, window, monkeypatch):
    """prepare_g: pairs, pair count and root_status equal the oracle's walks expanded with pairs_from_path bit for bit; rewards
    within 1e-5 of Discriminator.reward, bit-equal to the per-pair kernel, with the +10 clip exercised."""
    r = refs[key]
    case = r.case
    want_u, want_v = r.pairs[window]
    eng = make_engine(ga, case, window)
    u, v, rew, st = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM)
    assert np.array_equal(st, r.walks["root_status"])
    assert eng.g_pairs == len(want_u) > 1000
    assert np.array_equal(u, want_u) and np.array_equal(v, want_v)
    dis = orc.Discriminator(case.dis_E, 1e-3)
    dis.b[:] = case.dis_b
    want = dis.reward(u.astype(np.int64), v.astype(np.int64))
    err = float(np.max(np.abs(rew - want)))
    clipped = int((np.abs(want - CLIP) < 1e-5).sum())
    print("%s d=%d W=%d: %d pairs, |reward - numpy| %.3g, %d at the clip" % (case.name, case.d, window, len(u), err, clipped))
    assert err <= 1e-5
    assert clipped > 0 and (np.abs(rew - CLIP) < 1e-5).any()
    assert np.array_equal(bits(eng.pair_reward(u, v)), bits(rew))
    if window <= 2:  # the whole-walk reward kernel against pair_fill + pair_reward behind the walks
        monkeypatch.setenv("GG_NO_PATH_REWARD", "1")
        u2, v2, rew2, _ = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM)
        monkeypatch.delenv("GG_NO_PATH_REWARD")
        assert np.array_equal(u2, u) and np.array_equal(v2, v) and np.array_equal(bits(rew2), bits(rew))
    eng.close()


@pytest.mark.parametrize("window", [1, 3])
@pytest.mark.parametrize("slots,per_root", wc.TILE_CASES)
def test_pairs_around_one_scan_tile(ga, refs, slots, per_root, window):
    """2047, 2048 and 2049 launched walks: the pair_ptr scan ends inside its first tile, at its end, one walk into the second."""
    case = refs[("small", None)].case
    sl = np.arange(slots, dtype=np.int32)
    walks = wc.oracle_walks(case, sl, per_root)
    assert len(walks["path_len"]) in (wc.SCAN_TILE - 1, wc.SCAN_TILE, wc.SCAN_TILE + 1)
    want_u, want_v, _ = wc.expand(walks, window)
    eng = make_engine(ga, case, window)
    u, v, rew, st = eng.prepare_g(sl, per_root, wc.SEED, wc.STREAM)
    assert np.array_equal(st, walks["root_status"])
    assert eng.g_pairs == len(want_u) > 1000 and np.array_equal(u, want_u) and np.array_equal(v, want_v)
    assert np.array_equal(bits(eng.pair_reward(u, v)), bits(rew))
    eng.close()


# ------------------------------------------------------------------------------------------------ c: the fused pass, SGD
def routes_of(window):
    """(name, environment) of the engines of one case: staged, all atomic, mostly hubs, generic pair kernel."""
    if window <= 2:
        return (("staged", {}), ("atomic", {"GG_STAGE_T": "0"}), ("hubs", {"GG_STAGE_T": "3"}), ("pair kernel", {"GG_NO_PATH_GRAD": "1"}))
    return (("default", {}), ("atomic", {"GG_STAGE_T": "0"}))


def run_fused_pass(ga, case, window, env, monkeypatch, fetch):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    eng = make_engine(ga, case, window, optimizer=ga.GG_OPT_SGD, lr_gen=wc.PASS_LR_GEN, lambda_gen=wc.LAMBDA_GEN)
    got = None
    if fetch:
        u, v, rew, _ = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM)
        swap_in_pass_table(eng, case, u, v, rew)
        got = (u, v, rew)
        n_pairs = len(u)
    else:  # nothing reads the pair arrays before the pass
        n_pairs = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM, fetch=False)
        if case.swap:
            eng.set_embeddings(0, case.pass_E)
            eng.set_bias(0, case.pass_b)
    eng.g_pass([0], n_pairs)
    tabs = (eng.get_embeddings(0), eng.get_bias(0))
    assert eng.counters()["g_steps"] == 1
    eng.close()
    for name in env:
        monkeypatch.delenv(name)
    return tabs, got, n_pairs


@pytest.mark.parametrize("window", wc.WINDOWS)
@pytest.mark.parametrize("key", CASES, ids=CASE_IDS)
def test_fused_pass_is_inside_the_band(ga, refs, key, window, monkeypatch):
    """g_pass([0], n_pairs), SGD: table and bias inside the band of the float64 restatement on every route the window allows.
    Measured on an MI355X: err / band between 0.41 and 0.48 (table) and 0.26 and 0.48 (bias) on every case, the same figure on
    every route of a case -- it is the rounding of E - lr G itself, on an entry the gradient hardly moves; the gradient's own share
    of the band is at most 0.074 on any route (deep, d = 8, window 1, generic pair kernel; 0.052 with atomics, 0.012 staged)."""
    r = refs[key]
    case = r.case
    ref = None
    for i, (route, env) in enumerate(routes_of(window)):
        (got_E, got_b), fetched, n_pairs = run_fused_pass(ga, case, window, env, monkeypatch, fetch=(i == 0))
        if fetched is not None:
            u, v, rew = fetched
            assert np.array_equal(u, r.pairs[window][0]) and np.array_equal(v, r.pairs[window][1])
            wc.check_moderate(case, u, v)
            ref = wc.sgd_reference(case.pass_E, case.pass_b, u, v, rew)
        assert n_pairs == ref["n"]
        rE, rb = wc.band_ratio(got_E, got_b, case.pass_E, case.pass_b, ref)
        moved = float(np.abs(got_E - case.pass_E).max())
        sE, sb = wc.gradient_share(got_E, got_b, case.pass_E, case.pass_b, ref)
        print("%s d=%d W=%d %-11s: %d pairs, moved %.3g, err/band table %.3f bias %.3f (gradient's share %.3f %.3f)" %
              (case.name, case.d, window, route, n_pairs, moved, rE, rb, sE, sb))
        assert moved > 1e-4
        assert rE <= 1.0 and rb <= 1.0, (route, rE, rb)


# ------------------------------------------------------------------------------------------------ d: lazy Adam
@pytest.mark.parametrize("window", [1, 3])
def test_lazy_adam_rounds_match_the_oracle(ga, refs, window):
    case = refs[("small", None)].case
    eng = make_engine(ga, case, window, optimizer=ga.GG_OPT_ADAM_LAZY)
    gen = orc.Generator(case.walk_E, 1e-3, lazy=True)
    gen.b[:] = case.walk_b
    for rnd in range(2):
        u, v, rew, _ = eng.prepare_g(case.roots, case.n_sample, wc.SEED, 2 * rnd + 1)
        eng.g_pass([0], len(u))
        gen.g_step(u.astype(np.int64), v.astype(np.int64), rew, 1e-5)
        assert len(u) > 1000
        assert np.allclose(eng.get_embeddings(0), gen.E, rtol=2e-5, atol=2e-6), rnd
        assert np.allclose(eng.get_bias(0), gen.b, rtol=2e-5, atol=2e-6), rnd
    assert np.abs(gen.E - case.walk_E).max() > 1e-4
    eng.close()


# ------------------------------------------------------------------------------------------------ e: bit reproducibility
@pytest.mark.parametrize("window", [1, 2])
@pytest.mark.parametrize("d", wc.DIMS)
def test_staged_deep_paths_are_bit_reproducible(ga, refs, d, window, monkeypatch):
    """GG_STAGE_T=100000: every row of the 48-node table is staged and summed in key order by path_grad_kernel<.., STAGED,
    SHORT = false>: three fresh engines give the same bits."""
    case = refs[("deep", d)].case
    assert case.stride > 17
    tabs = [run_fused_pass(ga, case, window, {"GG_STAGE_T": "100000"}, monkeypatch, fetch=False)[0] for _ in range(3)]
    assert np.abs(tabs[0][0] - case.pass_E).max() > 1e-4
    for k in (1, 2):
        assert np.array_equal(bits(tabs[0][0]), bits(tabs[k][0])) and np.array_equal(bits(tabs[0][1]), bits(tabs[k][1]))


# ------------------------------------------------------------------------------------------------ f: early launch, early index
def run_step_sequence(ga, case, window, begin, env, monkeypatch):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    eng = make_engine(ga, case, window, optimizer=ga.GG_OPT_SGD, lr_gen=wc.PASS_LR_GEN, lambda_gen=wc.LAMBDA_GEN)
    rows = eng.prepare_d(case.roots, wc.SEED, 0, fetch=False)
    assert rows > 400
    if begin:
        eng.prepare_g_begin(case.roots, case.n_sample, wc.SEED, wc.STREAM)
    # batches of 256 rows take the atomic-free gradient kernel: the discriminator the rewards are computed with has the same
    # bits in every run (one fused batch of these ~1 000 rows would add them with fp32 atomics)
    eng.d_pass(np.arange(0, rows, 256), 256)
    u, v, rew, st = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM)
    eng.g_pass([0], len(u))
    out = (u, v, rew, st, eng.get_embeddings(0), eng.get_bias(0))
    eng.close()
    for name in env:
        monkeypatch.delenv(name)
    return out


@pytest.mark.parametrize("window", [1, 3])
def test_early_walk_launch_and_early_index(ga, refs, window, monkeypatch):
    """prepare_d, prepare_g_begin, d_pass, prepare_g, g_pass against the same sequence without the begin call, and with the early
    staging index switched off: same pairs and rewards bit for bit; tables inside the band, and at window 1 (the whole-walk pass
    on the early index), with every row staged, bit for bit."""
    case = refs[("small", None)].case
    stage = {"GG_STAGE_T": "100000"} if window == 1 else {}
    runs = [run_step_sequence(ga, case, window, True, stage, monkeypatch),
            run_step_sequence(ga, case, window, False, stage, monkeypatch),
            run_step_sequence(ga, case, window, True, dict(stage, GG_NO_EARLY_SLOTS="1"), monkeypatch)]
    u, v, rew, st = runs[0][:4]
    want_u, want_v, _ = wc.expand(wc.oracle_walks(case, after_d=True), window)   # (the D walks removed father entries: Q3)
    assert len(u) > 1000 and np.array_equal(u, want_u) and np.array_equal(v, want_v)
    ref = wc.sgd_reference(case.walk_E, case.walk_b, u, v, rew)
    for k, run in enumerate(runs):
        assert np.array_equal(run[0], u) and np.array_equal(run[1], v) and np.array_equal(run[3], st), k
        assert np.array_equal(bits(run[2]), bits(rew)), k
        rE, rb = wc.band_ratio(run[4], run[5], case.walk_E, case.walk_b, ref)
        print("W=%d sequence %d: err/band table %.3f bias %.3f" % (window, k, rE, rb))
        assert rE <= 1.0 and rb <= 1.0, k
        if window == 1:
            assert np.array_equal(bits(run[4]), bits(runs[0][4])) and np.array_equal(bits(run[5]), bits(runs[0][5])), k
    assert np.abs(runs[0][4] - case.walk_E).max() > 1e-4


# ------------------------------------------------------------------------------------------------ g: minibatch passes
def test_minibatch_passes_at_window_1(ga, refs):
    """g_pass(starts, 64) == the g_step sequence, as test_passes_equal_sequences_of_steps checks at window 2.  The passing engine
    never fetched its pairs: they are filled on first use, behind a whole-walk reward kernel that did not need them."""
    case = refs[("small", None)].case
    eng, eng2 = make_engine(ga, case, 1), make_engine(ga, case, 1)
    n_pairs = eng.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM, fetch=False)
    u, v, rew, _ = eng2.prepare_g(case.roots, case.n_sample, wc.SEED, wc.STREAM)
    assert n_pairs == len(u) and np.array_equal(u, refs[("small", None)].pairs[1][0])
    starts = np.arange(0, len(u), 64)
    assert len(starts) > 100 and len(u) % 64 != 0   # (a ragged last batch)
    np.random.RandomState(0).shuffle(starts)
    eng.g_pass(starts, 64)
    for s in starts:
        eng2.g_step(u[s:s + 64], v[s:s + 64], rew[s:s + 64])
    assert np.abs(eng.get_embeddings(0) - case.walk_E).max() > 1e-4
    assert np.allclose(eng.get_embeddings(0), eng2.get_embeddings(0), rtol=1e-6, atol=1e-7)
    assert np.allclose(eng.get_bias(0), eng2.get_bias(0), rtol=1e-6, atol=1e-7)
    eng.close()
    eng2.close()


# ------------------------------------------------------------------------------------------------ h: refusals, the wide window
@pytest.mark.parametrize("window", [0, -1])
def test_window_below_1_is_refused(ga, refs, window):
    case = refs[("small", None)].case
    with pytest.raises(ga.GraphGANHipError) as ei:
        ga.Engine(case.walk_E, case.dis_E, window_size=window)
    assert "window_size" in str(ei.value) and str(window) in str(ei.value)
    assert ei.value.code == ga.GG_EINVAL


@pytest.mark.parametrize("d", wc.DIMS)
def test_widest_window_equals_window_64(ga, refs, d, monkeypatch):
    """window_size = 2^31 - 1: no overflow in i + window + 1, no capacity in proportion to the window -- the pairs, rewards and
    pass result of window 64 (no path has 64 nodes)."""
    case = refs[("deep", d)].case
    (E_w, b_w), (u_w, v_w, r_w), _ = run_fused_pass(ga, case, wc.WIDE_WINDOW, {}, monkeypatch, fetch=True)
    (E_64, b_64), (u_64, v_64, r_64), _ = run_fused_pass(ga, case, 64, {}, monkeypatch, fetch=True)
    assert len(u_w) == len(u_64) > 30000
    assert np.array_equal(u_w, u_64) and np.array_equal(v_w, v_64) and np.array_equal(bits(r_w), bits(r_64))
    ref = wc.sgd_reference(case.pass_E, case.pass_b, u_64, v_64, r_64)
    for got_E, got_b in ((E_w, b_w), (E_64, b_64)):
        rE, rb = wc.band_ratio(got_E, got_b, case.pass_E, case.pass_b, ref)
        assert rE <= 1.0 and rb <= 1.0
    # (>= 16 384 pairs: the generic pass stages its rows; staged sums and hub sums do not depend on the arrival order)
    assert np.array_equal(bits(E_w), bits(E_64)) and np.array_equal(bits(b_w), bits(b_64))


# ------------------------------------------------------------------------------------------------ i: the trainer
@pytest.mark.parametrize("window", [1, 3])
def test_fast_mode_trainer_at_other_windows(tmp_path, window):
    """The fast-mode schedule of tests/test_gpu_e2e.py::test_fast_mode_schedule_matches_oracle at window_size 1 and 3, on the
    root subset of test_reduced_schedule_matches_oracle, two inner epochs; the oracle trainer gets the same window."""
    from tests.test_gpu_e2e import make_cfg, write_reference_layout
    base = str(tmp_path)
    d, n, graph = write_reference_layout(base)
    big = 1 << 30
    cfg = make_cfg(base, n_epochs=1, n_epochs_dis=2, n_epochs_gen=2, dis_interval=2, gen_interval=2, engine_seed=23,
                   batch_size_gen=big, batch_size_dis=big, engine_optimizer="adam_lazy", engine_profile_every=3, window_size=window)
    from graphgan_amd.graph_gan import GraphGAN
    g = GraphGAN(cfg)
    subset = list(range(0, n, 7))
    g.root_nodes = subset
    g.trees = g.construct_trees(subset)
    g.train()
    ocfg = orc.Config()
    ocfg.n_epochs_dis = ocfg.n_epochs_gen = ocfg.dis_interval = ocfg.gen_interval = 2
    ocfg.batch_size_gen = ocfg.batch_size_dis = big
    ocfg.window_size = window
    o = orc.GraphGANOracle(n, graph, g.node_embed_init_g, g.node_embed_init_d, cfg=ocfg, rng="counter", arith="spec", seed=23, lazy_adam=True)
    o.root_nodes = subset
    o.train_epoch(0)
    eg, ed = g.generator.embedding_matrix, g.discriminator.embedding_matrix
    for got, want in ((eg, o.generator.E), (ed, o.discriminator.E)):
        diff = np.abs(got - want)
        print("W=%d abs diff: mean %.3g p99 %.3g max %.3g" % (window, diff.mean(), np.quantile(diff, 0.99), diff.max()))
        assert diff.mean() < 2e-5 and np.quantile(diff, 0.99) < 2e-4
    assert np.abs(eg - g.node_embed_init_g.astype(np.float32)).max() > 1e-3  # training moved the tables
    lines = open(cfg.result_filename).read().split()
    acc_g, acc_d = float(lines[2][4:]), float(lines[3][4:])
    oacc_g = orc.eval_link_prediction(o.generator.E.astype(np.float64), d["test"].tolist(), d["test_neg"].tolist())
    oacc_d = orc.eval_link_prediction(o.discriminator.E.astype(np.float64), d["test"].tolist(), d["test_neg"].tolist())
    assert abs(acc_g - oacc_g) <= 0.005 and abs(acc_d - oacc_d) <= 0.005
