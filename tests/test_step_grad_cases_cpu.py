"""The premises of tests/test_gpu_step_grads.py, checked without a GPU against the oracle (cases, restatement and bands:
tests/support/step_grad_cases.py): the float64 restatement agrees with the oracle's loss_and_grads; the band holds the oracle's own
fp32 gradient rows, summed in fp32 in a shuffled order and applied with the oracle's fp32 optimizer, with room to spare; every
deliberately wrong gradient leaves the band by a factor of 10 or more, under SGD and under both Adam variants; the case lists
reach every kernel instance of run_step's dispatch; and the restated dispatch lines are still in the sources."""
import copy
import os

import numpy as np

from oracle import graphgan_oracle as orc
from tests.support import step_grad_cases as sg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc")
BY_BATCH = sorted(sg.CASES, key=lambda c: (str(c.batch_key()), c.id))


# ------------------------------------------------------------------------------------------------ the oracle's fp32 step
def _shuffled_sum32(n_rows, rows, vals, seed):
    """vals (fp32 rows) added per table row in float32, in a shuffled order."""
    order = np.random.RandomState(seed).permutation(len(rows))
    order = order[np.argsort(rows[order], kind="stable")]
    r = rows[order]
    starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
    out = np.zeros((n_rows,) + vals.shape[1:], dtype=np.float32)
    out[r[starts]] = np.add.reduceat(vals[order], starts, axis=0, dtype=np.float32)
    return out


def _fixed_point_sum(n_rows, rows, vals, scale, hubs):
    """The hub rows' sums as hub_add / hub_finalize_kernel form them: every contribution rounded to 1 / scale, the sum rounded once."""
    out = {}
    for h in hubs:
        q = np.rint(vals[rows == h].astype(np.float64) * scale).sum(axis=0)
        out[h] = (q / scale).astype(np.float32)
    return out


class Fp32Side:
    """The oracle's fp32 arithmetic on a case: loss_and_grads rows, an fp32 sum, TF1Adam / SGD in fp32."""

    def __init__(self, case):
        self.case, self.b = case, case.batch()
        lazy = case.optimizer == "lazy"
        self.opt = orc.TF1Adam([self.b.E.shape, self.b.b.shape], case.lr, eps=sg.ADAM_EPS, lazy=lazy)

    def rows(self, k, E, b):
        c = self.case
        u, v, x = self.b.steps[k]
        u, v = u.astype(np.int64), v.astype(np.int64)
        model = (orc.Discriminator if c.model == "d" else orc.Generator)(E, c.lr)
        model.b[:] = b
        if c.model == "g":
            x = x / np.float32(c.world)   # the mean over the pairs of all simulated ranks (a power of two: exact)
        _, gu, gv, gb = model.loss_and_grads(u, v, x, sg.LAMBDA)
        assert gu.dtype == np.float32 and gb.dtype == np.float32
        return np.concatenate([u, v]), np.concatenate([gu, gv]), v, gb

    def step(self, k, E, b, seed=5, rows=None):
        c = self.case
        rows, vals, brows, bvals = rows or self.rows(k, E, b)
        G, Gb = _shuffled_sum32(self.b.n_rows, rows, vals, seed), _shuffled_sum32(self.b.n_rows, brows, bvals, seed + 1)
        if c.staged:
            u, v, _ = self.b.steps[k]
            hubs = np.flatnonzero(sg.stage_counts(self.b.n_rows, u, v) > sg.SG_THRESHOLD)
            for h, row in _fixed_point_sum(self.b.n_rows, rows, vals, c.scale, hubs).items():
                G[h] = row
            for h, val in _fixed_point_sum(self.b.n_rows, brows, bvals, c.scale, hubs).items():
                Gb[h] = val
        G, Gb = G * np.float32(c.world), Gb * np.float32(c.world)
        E, b = E.copy(), b.copy()
        if c.optimizer == "sgd":
            E -= np.float32(c.lr) * G
            b -= np.float32(c.lr) * Gb
        else:
            idx = np.unique(rows)   # node-granular in lazy mode (PairModel._bias_slices); dense Adam decays every row anyway
            self.opt.step([E, b], [(idx, G[idx]), (idx, Gb[idx])])
        assert E.dtype == np.float32 and b.dtype == np.float32
        return E, b


# ------------------------------------------------------------------------------------------------ agreement, not too tight
def test_band_holds_the_oracles_fp32_step_on_every_case():
    worst, worst_id = 0.0, None
    for case in BY_BATCH:
        w, f = sg.Walker(case), Fp32Side(case)
        bt = w.b
        E, b = bt.E, bt.b
        fills = []
        for k in range(2):
            ref = w.reference(k, E, b)
            sg.check_scores(case.model, ref, bt.cold[k])
            # agreement: the oracle's rows, summed in float64, against the restatement, to the accuracy of one fp32 term
            orc_rows = f.rows(k, E, b)
            rows, vals, brows, bvals = orc_rows
            G_orc = case.world * sg._scatter(bt.n_rows, rows, vals.astype(np.float64))
            Gb_orc = case.world * sg._scatter(bt.n_rows, brows, bvals.astype(np.float64))
            assert (np.abs(G_orc - ref["G"]) <= sg.U * (8.0 * ref["A"] + ref["Q"])).all(), (case, k)
            assert (np.abs(Gb_orc - ref["Gb"]) <= sg.U * (8.0 * ref["Ab"] + ref["Qb"])).all(), (case, k)
            want_E, want_b, band_E, band_b = w.advance(k, E, b, ref)
            assert np.abs(want_E - E).max() > 1e-3, (case, k)                    # the step moves the table
            got_E, got_b = f.step(k, E, b, rows=orc_rows)
            fills.append(max(sg.ratio(got_E, want_E, band_E), sg.ratio(got_b, want_b, band_b)))
            un = ~w.touched(0) if k == 0 else ~(w.touched(0) | w.touched(1))
            assert un.sum() >= 7 and np.array_equal(got_E[un], bt.E[un]) and np.array_equal(got_b[un], bt.b[un])
            E, b = got_E, got_b
        print("%-60s %-40s fp32 reference err/band %.3f %.3f" % (case.id, "+".join(case.route), fills[0], fills[1]))
        if max(fills) > worst:
            worst, worst_id = max(fills), case.id
    print("largest fill %.4f (%s); recorded %.4f" % (worst, worst_id, sg.CPU_FILL))
    assert worst <= sg.CPU_FILL <= 0.5, (worst, worst_id)


# ------------------------------------------------------------------------------------------------ not vacuous
def _mutations(case, bt, ref, k=0):
    """{name: mut of grad_reference} of every deliberately wrong gradient that applies to pair list k of the case."""
    u, v, x = bt.steps[k]
    v64, x64 = v.astype(np.int64), x.astype(np.float64)
    n, cold, m = len(u), bt.cold[k], ref["m"]
    one, zero = np.ones(n), np.zeros(n)
    sgm = 1.0 / (1.0 + np.exp(-ref["s"]))
    lone = 1.0 / m[v64]                                                  # prefers pairs whose v row collects few gradients
    live = ~cold
    out = {"u-side L2 dropped": dict(l2_u=zero), "v-side L2 dropped": dict(l2_v=zero)}
    out["bias L2 dropped" if case.model == "d" else "bias L2 added"] = dict(l2_b=0.0 if case.model == "d" else 1.0)
    run_end = np.ones(n, bool)
    run_end[:-1] = u[1:] != u[:-1]
    if not run_end.all():
        out["L2 once per run of equal u"] = dict(l2_u=run_end.astype(np.float64))
    if (u == v).any():
        out["L2 once per distinct row of a self pair"] = dict(l2_v=(u != v).astype(np.float64))
    weight = np.abs(sgm - x64) if case.model == "d" else x64 * (1.0 - sgm)
    k_drop = int(np.argmax(np.where(live, (weight + 1e-3) * lone, -1.0)))
    out["one pair dropped"] = dict(keep=np.arange(n) != k_drop)
    if n >= 2:
        nxt = np.minimum(np.arange(n) + 1, n - 1)
        gain = np.abs(x64 - x64[nxt]) * (1.0 if case.model == "d" else 1.0 - sgm)
        k_swap = int(np.argmax(np.where(live & live[nxt], gain * lone, -1.0)))
        swapped = x.copy()
        swapped[[k_swap, k_swap + 1]] = swapped[[k_swap + 1, k_swap]]
        out["one label swapped with its neighbour's" if case.model == "d" else "one reward swapped with its neighbour's"] = dict(x=swapped)
    if case.staged:
        hubs = np.flatnonzero(sg.stage_counts(bt.n_rows, u, v) > sg.SG_THRESHOLD)
        out["the gradient of one hub row doubled"] = dict(row_gain={int(hubs[0]): 2.0})
    if case.model == "g":
        name = "1 / n taken as 1 / (n + 1)"
        out[name if sg.mean_off_by_one_visible(n * case.world, case.d) else "(printed only) " + name] = dict(n_mean=n * case.world + 1)
        out["the mean's denominator 1 % too large"] = dict(n_mean=n * case.world * 1.01)
        if case.world > 1:
            out["the mean over this rank's pairs, not all ranks'"] = dict(n_mean=n)
    if cold.any():
        k_cold = int(np.argmax(np.where(cold, x64 / np.maximum(m[u.astype(np.int64)], m[v64]), -1.0)))
        out["the clip ignored on one clipped pair"] = dict(force_inside=np.arange(n) == k_cold)
        w = one.copy()
        w[k_cold] = 0.0
        out["a clipped pair's L2 term dropped with its data term"] = dict(l2_u=w, l2_v=w)
    return out


def test_every_mutation_leaves_the_band():
    """Each wrong gradient, applied with the case's optimizer in float64, against the band around the right one: a factor >= 10.
    A mutation that hits ONE pair hits the pair its error weighs most on (as tests/test_window_cases_cpu.py does and explains).
    1 / (n + 1) changes the data term by 1 / n relative, while the fp32 score of a width-d row alone may move sg by (d + 2) S u / 4:
    it is asserted on every generator case where step_grad_cases.mean_off_by_one_visible says a worst-case band can tell the two
    apart -- every case up to 2053 pairs, and the 16384-pair cases at d = 6 -- and printed on the wider 16384-pair cases (1.6 at the
    least).  EVERY generator case, those included, asserts a denominator that is 1 % too large, and the cases with two simulated
    ranks the mean over one rank's pairs: the gradient's scale is checked on every route."""
    seen = {}
    key, base = None, None
    for case in BY_BATCH:
        w, bt = sg.Walker(case), case.batch()
        if case.batch_key() != key:
            ref = w.reference(0, bt.E, bt.b)
            muts = _mutations(case, bt, ref)
            wrong = {}
            for name, mut in muts.items():
                wrong[name] = w.reference(0, bt.E, bt.b, mut, sums_only=True)
            key, base = case.batch_key(), (ref, wrong)
        ref, wrong = base
        want_E, want_b, band_E, band_b = w.advance(0, bt.E, bt.b, ref, state=copy.deepcopy(w.state))
        for name, bad in wrong.items():
            bad_E, bad_b, _, _ = w.advance(0, bt.E, bt.b, ref, applied=bad, state=copy.deepcopy(w.state))
            f = max(sg.ratio(bad_E, want_E, band_E), sg.ratio(bad_b, want_b, band_b))
            seen.setdefault(name, []).append((f, case.id))
            if not name.startswith("(printed only)"):
                assert f >= 10.0, (case, name, f)
    for name, fs in sorted(seen.items()):
        print("%-55s %4d cases, leaves the band by at least %.3g (%s)" % (name, len(fs), min(fs)[0], min(fs)[1]))
    every = {"u-side L2 dropped", "v-side L2 dropped", "bias L2 dropped", "bias L2 added", "L2 once per run of equal u",
             "L2 once per distinct row of a self pair", "one pair dropped", "one label swapped with its neighbour's",
             "one reward swapped with its neighbour's", "the gradient of one hub row doubled", "1 / n taken as 1 / (n + 1)",
             "the clip ignored on one clipped pair", "a clipped pair's L2 term dropped with its data term",
             "the mean's denominator 1 % too large", "the mean over this rank's pairs, not all ranks'"}
    assert every <= set(seen)
    gen = {c.id for c in sg.CASES if c.model == "g"}
    assert {i for _, i in seen["the mean's denominator 1 % too large"]} == gen
    off_by_one = {i for _, i in seen["1 / n taken as 1 / (n + 1)"]}
    assert {c.id for c in sg.CASES if c.model == "g" and (c.n <= 2053 or c.d == 6)} == off_by_one
    assert {i for _, i in seen["the mean over this rank's pairs, not all ranks'"]} == {c.id for c in sg.CASES if c.model == "g" and c.world > 1}
    for name in every:   # under SGD and under both Adam variants
        ids = [i for _, i in seen[name]]
        for opt in ("sgd", "lazy") + (() if "hub" in name or "rank" in name else ("dense",)):   # (dense Adam never stages: no hub rows, no staged replicas)
            assert any("-%s" % opt in i for i in ids), (name, opt)


# ------------------------------------------------------------------------------------------------ the pair lists' structure
def test_pair_lists_have_the_structure_the_cases_are_for():
    for case in sg.CASES:
        bt = case.batch()
        assert bt.E.dtype == np.float32 and bt.E.shape == (bt.n_rows, case.d) and 600 <= bt.n_rows <= 8000
        (u0, v0, x0), (u1, v1, x1) = bt.steps
        assert len(u0) == len(u1) == case.n and not (np.array_equal(u0, u1) and np.array_equal(v0, v1))
        if case.model == "d":
            assert set(np.unique(x0)) <= {0.0, 1.0}
        else:
            assert x0.min() >= 0 and x0.max() < 2
        for k, (u, v, x) in enumerate(bt.steps):
            cold, n = bt.cold[k], case.n
            assert cold.sum() == (max(1, n // 10) if case.clip else 0)
            if case.layout == "small" and n >= 8:
                assert (u == sg.C0).sum() >= n // 2 and (v == sg.W0).sum() >= n // 2 - cold.sum()   # one centre / one neighbour for half
                assert ((u == sg.C0) & (v == sg.W0)).sum() >= sg.REPEATS                       # the same pair repeated
                assert ((u == v) & (u == sg.SELF)).sum() == 2                                   # self pairs
                assert (u == sg.W0).any() and (v == sg.C0).any()                                # rows named on both sides
            if case.layout == "middle":
                runs = np.diff(np.flatnonzero(np.concatenate([[True], u[1:] != u[:-1], [True]])))
                assert (runs == 6).sum() > n // 8 and 6 % 4 != 0                                # runs cross the 4-pair groups
                assert (u == v).any()
            if case.n >= sg.PPG_LARGE:
                cnt = sg.stage_counts(bt.n_rows, u, v)
                for row, c in sg.HUB_V:
                    assert cnt[row] == c and 65 <= c <= 130
                assert 65 <= cnt[sg.HUB_U] <= 130
                assert cnt[sg.T64] == 64 == sg.SG_THRESHOLD and cnt[sg.T65] == 65
                assert sorted(np.flatnonzero(cnt > sg.SG_THRESHOLD)) == [10, 11, 12, 13, 15]
                assert (u == v).any()
                run = sg.RUN[case.layout]
                if run > 1:
                    runs = np.diff(np.flatnonzero(np.concatenate([[True], u[1:] != u[:-1], [True]])))
                    assert (runs == run).sum() > n // (2 * run)
    assert 16389 % 16 == 5 and 2053 % 4 == 1   # ragged last groups


# ------------------------------------------------------------------------------------------------ routes reached
def test_cases_reach_every_instance_of_the_dispatch():
    grad = {c.route[0] for c in sg.CASES}
    opt = {part for c in sg.CASES for part in c.route[1].split("+")}
    print("\n".join(sorted(grad) + sorted(opt)))
    want = {"pair_grad_det_kernel<%d,true,%d,%s>" % (nf, o, s) for nf in (4, 8, 16, 32) for o in (0, 1, 2) for s in ("true", "false")}
    want |= {"pair_grad_det_kernel<8,false,0,false>", "pair_grad_det_kernel<16,false,0,false>", "pair_grad_det_kernel<32,false,0,false>",
             "pair_grad_det_kernel<32,false,0,true>"}
    want |= {"pair_grad_kernel<%d,false>@ppg%d" % (nf, p) for nf in (4, 8, 16, 32) for p in (1, 4)}
    want |= {"pair_grad_kernel<%d,false>@ppg16" % nf for nf in (4, 8, 16, 32)}
    want |= {"pair_grad16_kernel<%d,%s>" % (nf, s) for nf in (4, 8, 16) for s in ("true", "false")}
    assert grad == want, (sorted(want - grad), sorted(grad - want))
    want_opt = {"adam_dense_kernel", "sparse_opt_kernel<0>", "sparse_opt_kernel<1>", "fused"}
    want_opt |= {"staged_opt_kernel<%d,%d>" % (mode, nc) for mode in (0, 1, 2) for nc in (1, 2, 4)}
    assert opt == want_opt, (sorted(want_opt - opt), sorted(opt - want_opt))
    # the fused and the unfused small step of one batch, for the bit comparison; a staged lazy case to repeat
    fused = {(c.batch_key(), c.optimizer) for c in sg.SMALL_CASES if c.route[1] == "fused"}
    unfused = {(c.batch_key(), c.optimizer) for c in sg.SMALL_CASES if c.env == sg.NO_FUSED and sg.rows_fit_lds(c.n, c.d)}
    assert len(unfused) >= 20 and unfused <= fused
    assert any(c.staged and c.optimizer == "lazy" and c.world == 1 for c in sg.LARGE_CASES)
    # each gradient-kernel family has a generator case with clipped pairs
    fam = {c.route[0].split("<")[0] for c in sg.CLIP_CASES}
    assert fam == {"pair_grad_det_kernel", "pair_grad_kernel", "pair_grad16_kernel"}
    assert any(c.staged for c in sg.CLIP_CASES)
    # both sides of the LDS limit, as the issue names them
    assert [sg.rows_fit_lds(n, d) for n, d in ((64, 288), (64, 289), (256, 65), (256, 73))] == [True, False, True, False]
    assert {c.model for c in sg.CASES} == {"d", "g"}


def test_restated_dispatch_is_still_in_the_sources():
    # drift guard: tests/support/step_grad_cases.py restates these lines.  If this fails after an edit of a source file, the dispatch
    # may have changed: update route() / staged() / hub_scale() and the case lists there (or, after a mere reformat, the texts below)
    copied = {
        "steps.hip": ("s.ppg = n >= 16384 ? PAIRS_PER_GROUP : (n >= 2048 ? 4 : 1);",
                      "constexpr int PAIRS_PER_GROUP = 16;",
                      "constexpr int DET_MAX_PAIRS = 256;",
                      "constexpr size_t DET_LDS_ROW_BYTES = 144 * 1024;",
                      "return (size_t)2 * s.n * s.ld * sizeof(float) <= DET_LDS_ROW_BYTES && det_lds_granted(ctx->device);",
                      "if (ctx->deterministic && n <= DET_MAX_PAIRS) {",
                      "const int nfd = (ctx->ld + 15) / 16;",
                      "if (nfd <= 4) e = launch_pair_grad_det<4>(ctx, s, o, fused);",
                      "else if (nfd <= 8) e = launch_pair_grad_det<8>(ctx, s, o, fused);",
                      "else if (nfd <= 16) e = launch_pair_grad_det<16>(ctx, s, o, fused);",
                      "else e = launch_pair_grad_det<32>(ctx, s, o, fused);",
                      "const int fused = (!replicas && opt != GG_OPT_ADAM_DENSE && det_rows_fit_lds(ctx, s) && !getenv(\"GG_NO_FUSED_SMALL_STEP\")) ? (opt == GG_OPT_SGD ? 2 : 1) : 0;",
                      "if (s.n <= 64) hipLaunchKernelGGL((pair_grad_det_kernel<NF, true, OPT, true>), grid, dim3(DET_THREADS), dyn, ctx->stream, s, o);",
                      "const int fit = n >= 16384 && n < (1 << 30) && staged_allowed(ctx) ? staged_reserve(ctx, 2 * (int64_t)n, 2 * (int64_t)n) : 1;",
                      "return ctx->sg_threshold > 0 && ctx->ld <= 256 && ctx->cfg.optimizer != GG_OPT_ADAM_DENSE && !getenv(\"GG_NO_STAGED_GRAD\");",
                      "if (STAGED || (s.ppg == PAIRS_PER_GROUP && nf <= 16 && !getenv(\"GG_OLD_PAIR_GRAD\"))) {",
                      "if (nf <= 4) hipLaunchKernelGGL((pair_grad16_kernel<4, STAGED>), g, b, 0, ctx->stream, s);",
                      "else if (nf <= 8) hipLaunchKernelGGL((pair_grad16_kernel<8, STAGED>), g, b, 0, ctx->stream, s);",
                      "else hipLaunchKernelGGL((pair_grad16_kernel<16, STAGED>), g, b, 0, ctx->stream, s);",
                      "else if (nf <= 16) hipLaunchKernelGGL((pair_grad_kernel<16, false>), g, b, 0, ctx->stream, s);",
                      "else hipLaunchKernelGGL((pair_grad_kernel<32, false>), g, b, 0, ctx->stream, s);",
                      "if (ctx->ld <= 64) hipLaunchKernelGGL((staged_opt_kernel<MODE, 1>), g, b, 0, ctx->stream, o);",
                      "else if (ctx->ld <= 128) hipLaunchKernelGGL((staged_opt_kernel<MODE, 2>), g, b, 0, ctx->stream, o);",
                      "else hipLaunchKernelGGL((staged_opt_kernel<MODE, 4>), g, b, 0, ctx->stream, o);",
                      "return std::ldexp(1.0f, 32 + (per_pair_mean && n > 1 ? (int)std::ilogb((double)n) : 0));",
                      "const float scale = hub_scale(!s.is_d, n);",
                      "const bool run_end = p == n - 1 || (p + 1) % ppg == 0 || u[p + 1] != u[p];",
                      "const int sv = cnt[iv] <= T ? off[iv] + slot_v[p] : -3 - off[iv];"),
        "gg_internal.h": ("int sg_threshold = 64;",),
        "gg_api.hip": ("ctx->ld = (n_emb + 3) / 4 * 4;",),
    }
    for name, texts in copied.items():
        src = open(os.path.join(CSRC, name)).read()
        for text in texts:
            assert text in src, "%s no longer contains %r: restate the dispatch in tests/support/step_grad_cases.py" % (name, text)
    assert (sg.DET_MAX_PAIRS, sg.DET_LDS_ROW_BYTES, sg.SG_THRESHOLD, sg.PPG_LARGE, sg.PPG_MIDDLE) == (256, 144 * 1024, 64, 16384, 2048)
    # the restatement itself, at the edges of every rung
    assert [sg.ld_of(d) for d in (1, 4, 5, 257, 260)] == [4, 4, 8, 260, 260]
    assert [sg.nf_of(d) for d in (6, 64, 65, 128, 129, 256, 257)] == [4, 4, 8, 8, 16, 16, 32]
    assert [sg.ppg_of(n) for n in (256, 2047, 2048, 16383, 16384)] == [1, 1, 4, 4, 16]
    assert sg.hub_scale(False, 16389) == 2.0 ** 32 and sg.hub_scale(True, 16384) == 2.0 ** 46 == sg.hub_scale(True, 16389)
    assert sg.hub_scale(True, 16383) == 2.0 ** 45 and sg.hub_scale(True, 1) == 2.0 ** 32
    assert sg.route(64, 50, "lazy") == ("pair_grad_det_kernel<4,true,1,true>", "fused")
    assert sg.route(65, 50, "sgd", sg.NO_FUSED) == ("pair_grad_det_kernel<4,true,0,false>", "sparse_opt_kernel<1>")
    assert sg.route(257, 50, "lazy") == ("pair_grad_kernel<4,false>@ppg1", "sparse_opt_kernel<0>")
    assert sg.route(16384, 260, "lazy") == ("pair_grad_kernel<32,false>@ppg16", "sparse_opt_kernel<0>")
    assert sg.route(16384, 256, "sgd") == ("pair_grad16_kernel<16,true>", "staged_opt_kernel<1,4>+sparse_opt_kernel<1>")
    assert sg.route(16383, 256, "sgd") == ("pair_grad_kernel<16,false>@ppg4", "sparse_opt_kernel<1>")


# ------------------------------------------------------------------------------------------------ the whole-walk leg
def test_whole_walk_leg_has_clipped_pairs_and_a_band_that_sees_them():
    case, u, v, cold = sg.window_clip_leg()
    assert case.swap and case.stride <= 17 and len(u) > 6000
    assert 0.08 * len(u) <= cold.sum() <= 0.1 * len(u)
    dis = orc.Discriminator(case.dis_E, 1e-3)
    dis.b[:] = case.dis_b
    rew = dis.reward(u.astype(np.int64), v.astype(np.int64))
    ref, want_E, want_b, band_E, band_b = sg.window_leg_step(case, u, v, rew, True)
    sg.check_scores("g", ref, cold)
    # the oracle's fp32 rows, summed in fp32 in a shuffled order, applied in fp32
    gen = orc.Generator(case.pass_E, sg.WINDOW_LEG_LR)
    gen.b[:] = case.pass_b
    _, gu, gv, gb = gen.loss_and_grads(u.astype(np.int64), v.astype(np.int64), rew, sg.LAMBDA)
    rows = np.concatenate([u, v]).astype(np.int64)
    G32 = _shuffled_sum32(case.n, rows, np.concatenate([gu, gv]), 5)
    Gb32 = _shuffled_sum32(case.n, v.astype(np.int64), gb, 6)
    lr = np.float32(sg.WINDOW_LEG_LR)
    fill = max(sg.ratio(case.pass_E - lr * G32, want_E, band_E), sg.ratio(case.pass_b - lr * Gb32, want_b, band_b))
    print("whole-walk leg: %d pairs, %d clipped, fp32 reference err/band %.3f" % (len(u), cold.sum(), fill))
    assert fill <= sg.CPU_FILL
    # the clipped pair an ignored clip weighs most on, to first order: lr (r / n) |partner row| against the band of the row it lands in
    step, E64 = sg.WINDOW_LEG_LR * rew.astype(np.float64) / len(u), np.abs(case.pass_E.astype(np.float64))
    weigh = np.maximum((step[:, None] * E64[v] / band_E[u]).max(axis=1), (step[:, None] * E64[u] / band_E[v]).max(axis=1))
    k_cold = int(np.argmax(np.where(cold, weigh, -1.0)))
    w = np.ones(len(u))
    w[k_cold] = 0.0
    muts = {"the clip ignored on one clipped pair": dict(force_inside=np.arange(len(u)) == k_cold),
            "the clip ignored on the pairs that end in one cold node": dict(force_inside=v == v[k_cold]),
            "a clipped pair's L2 term dropped with its data term": dict(l2_u=w, l2_v=w),
            "u-side L2 dropped": dict(l2_u=np.zeros(len(u))), "v-side L2 dropped": dict(l2_v=np.zeros(len(u))),
            "bias L2 added": dict(l2_b=1.0), "1 / n taken as 1 / (n + 1)": dict(n_mean=len(u) + 1)}
    for name, mut in muts.items():
        _, bad_E, bad_b, _, _ = sg.window_leg_step(case, u, v, rew, True, mut)
        f = max(sg.ratio(bad_E, want_E, band_E), sg.ratio(bad_b, want_b, band_b))
        print("    %-55s leaves the band by %.3g" % (name, f))
        assert f >= 10.0, (name, f)
