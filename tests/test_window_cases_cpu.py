"""The premises of tests/test_gpu_window.py, checked without a GPU against the oracle: the cases of tests/support/window_cases.py
have the properties the GPU test relies on (deep paths, walks with more than 64 pairs, walk counts around one scan tile, rewards
at the clip, moderate scores); a window of 2^31 - 1 expands the pairs of 64; the band of the float64 SGD restatement holds the
oracle's own fp32 gradient rows summed in fp32 in any order, with room to spare; and it is narrow enough to see one swapped reward,
one dropped pair or one wrong bias index."""
import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.support import window_cases as wc

BAND_WINDOWS = (1, 2, 3, 64)
CLIP = np.log1p(np.exp(10.0))


@pytest.fixture(scope="module")
def cases():
    out = {("small", None): wc.small_case()}
    for d in wc.DIMS:
        out[("deep", d)] = wc.deep_case(d)
    return {k: (c, wc.oracle_walks(c)) for k, c in out.items()}


def _pairs_and_rewards(case, walks, window):
    u, v, per = wc.expand(walks, window)
    dis = orc.Discriminator(case.dis_E, 1e-3)
    dis.b[:] = case.dis_b
    return u, v, per, dis.reward(u.astype(np.int64), v.astype(np.int64))


def test_case_properties(cases):
    small, sw = cases[("small", None)]
    assert small.n == 90 and small.stride <= 17 and not small.swap                       # the SHORT instances
    # load_small(3) has four nodes without an edge (they occur in its test edges only): their roots abort, as in every prepare_g
    # test on this graph; no other root fails
    deg = np.diff(small.rowptr)
    assert np.array_equal(sw["root_status"] != 0, deg == 0) and int((deg == 0).sum()) == 4
    assert len(sw["path_len"]) == 90 * wc.SMALL_WALKS < wc.SCAN_TILE                      # (what the tile cases are for)
    for (slots, per_root), want in zip(wc.TILE_CASES, (2047, 2048, 2049)):
        w = wc.oracle_walks(small, np.arange(slots), per_root)
        assert len(w["path_len"]) == slots * per_root == want
        assert np.array_equal(w["root_status"] != 0, deg[:slots] == 0)
        assert wc.expand(w, 1)[2].sum() > 1000
    assert (wc.SCAN_TILE - 1, wc.SCAN_TILE, wc.SCAN_TILE + 1) == (2047, 2048, 2049)
    for d in wc.DIMS:
        deep, dw = cases[("deep", d)]
        assert deep.n == 48 and deep.d == d and deep.swap
        assert deep.stride == 43 > 17                                                    # SHORT = false
        assert len(dw["path_len"]) == 48 * wc.DEEP_WALKS == 96 and not dw["root_status"].any()   # every root is OK
        L = wc.path_nodes(dw)
        assert L.min() == 2 and L.max() == 41 == deep.stride - 2
        assert int((L > 16).sum()) >= 20, int((L > 16).sum())                            # ids / slots at positions >= 16
        assert (L == 2).any() and (L == 3).any()
        per1 = wc.expand(dw, 1)[2]
        assert per1.max() > 64, per1.max()                                               # the k >= 64 reward fallback, at window 1 already
        assert np.array_equal(per1, np.where(L >= 2, 2 * L - 2, 0))
        per2 = wc.expand(dw, 2)[2]
        assert np.array_equal(per2, np.where(L >= 3, 4 * L - 6, np.where(L == 2, 2, 0)))  # (the n_stage bound of run_path_step)
    for (name, d), (case, walks) in cases.items():
        for window in wc.WINDOWS:
            u, v, per, rew = _pairs_and_rewards(case, walks, window)
            wc.check_moderate(case, u, v)
            assert (np.abs(rew - CLIP) < 1e-5).any(), (name, d, window)                  # the +10 clip is exercised
            assert (np.abs(rew - CLIP) > 1.0).any()


def test_wide_window_expands_the_pairs_of_64(cases):
    for d in wc.DIMS:
        case, walks = cases[("deep", d)]
        for w in range(len(walks["path_len"])):
            path = walks["paths"][w, : walks["path_len"][w]].tolist()
            assert orc.pairs_from_path(path, wc.WIDE_WINDOW) == orc.pairs_from_path(path, 64)
            assert len(path) - 1 < 64


def _fp32_step(case, u, v, rew, seed):
    """The oracle's fp32 gradient rows, accumulated in float32 one row at a time in a shuffled order: (G, Gb), fp32."""
    gen = orc.Generator(case.pass_E, wc.PASS_LR_GEN)
    gen.b[:] = case.pass_b
    _, gu, gv, gb = gen.loss_and_grads(u.astype(np.int64), v.astype(np.int64), rew, wc.LAMBDA_GEN)
    rows, vals = np.concatenate([u, v]).astype(np.int64), np.concatenate([gu, gv])
    order = np.random.RandomState(seed).permutation(len(rows))
    G = np.zeros_like(case.pass_E)
    np.add.at(G, rows[order], vals[order])          # (unbuffered: one fp32 addition per row, in this order)
    order = np.random.RandomState(seed + 1).permutation(len(v))
    Gb = np.zeros_like(case.pass_b)
    np.add.at(Gb, v.astype(np.int64)[order], gb[order])
    assert G.dtype == np.float32 and Gb.dtype == np.float32
    return G, Gb


@pytest.mark.parametrize("window", BAND_WINDOWS)
def test_band_holds_the_fp32_reference_and_sees_one_wrong_pair(cases, window):
    for (name, d), (case, walks) in cases.items():
        u, v, per, rew = _pairs_and_rewards(case, walks, window)
        E, b = case.pass_E, case.pass_b
        ref = wc.sgd_reference(E, b, u, v, rew)
        want_E, want_b = wc.sgd_step(E, b, ref)
        assert np.abs(want_E - E).max() > 1e-4                                           # the step moves the table
        G32, Gb32 = _fp32_step(case, u, v, rew, 5)
        # the gradient's share of the band: the step itself in float64 ...
        rE, rb = wc.band_ratio(E.astype(np.float64) - wc.PASS_LR_GEN * G32, b.astype(np.float64) - wc.PASS_LR_GEN * Gb32, E, b, ref)
        # ... and with the step in fp32 as well.  Rounding E - lr G to fp32 alone costs up to u |E'| of the 2 u |E| the band has
        # for it, so this ratio comes close to 0.5 wherever the gradient is small
        lr = np.float32(wc.PASS_LR_GEN)
        sE, sb = wc.band_ratio(E - lr * G32, b - lr * Gb32, E, b, ref)
        print("%s d=%s W=%d: %d pairs, S_max %.3g, fp32 reference err/band: table %.3f bias %.3f; with an fp32 step %.3f %.3f" %
              (name, case.d, window, len(u), ref["S_max"], rE, rb, sE, sb))
        assert rE <= 0.5 and rb <= 0.5
        assert sE <= 1.0 and sb <= 1.0

        # ---- deliberately wrong variants, as float64 restatements, on "deep": each must leave the band by a factor of 10 or more.
        # Each hits ONE pair: the one its error weighs most on, to first order.  A single arbitrary pair need not show -- at window 64
        # a pair is one of 37 420 and the median pair dropped moves the table by 2 to 4 bands -- but an index error of a kernel
        # hits every pair of a kind, these among them.  ("small" is left out: its hub rows collect thousands of gradients, m_r u A
        # is wide there, and no single pair of 6 510 moves such a row by 10 bands.)
        if name != "deep":
            continue
        first = np.concatenate([[0], np.cumsum(per)])[:-1]
        in_walk = np.arange(len(u)) - np.repeat(first, per)
        late = np.arange(len(u)) + 1 < len(u)
        late[:-1] &= in_walk[1:] > in_walk[:-1]                                          # (k + 1 is a pair of the same walk)
        r64, b64 = rew.astype(np.float64), b.astype(np.float64)
        sig = lambda x: 1.0 / (1.0 + np.exp(-x))
        nxt = np.minimum(np.arange(len(u)) + 1, len(u) - 1)
        pick = lambda weight: int(np.argmax(np.where(late, weight, -1.0)))
        k_swap = pick((1.0 - sig(ref["s"])) * np.abs(r64 - r64[nxt]))
        k_drop = pick((1.0 - sig(ref["s"])) * r64)
        k_bias = pick(r64 * np.abs(sig(ref["s"]) - sig(ref["s"] - b64[v] + b64[u])))
        swapped = rew.copy()
        swapped[[k_swap, k_swap + 1]] = swapped[[k_swap + 1, k_swap]]
        keep = np.arange(len(u)) != k_drop
        wrong_bias = v.copy()
        wrong_bias[k_bias] = u[k_bias]
        variants = {
            "swapped reward": wc.sgd_reference(E, b, u, v, swapped),
            "dropped pair": wc.sgd_reference(E, b, u[keep], v[keep], rew[keep], n=len(u)),
            "bias of the first node": wc.sgd_reference(E, b, u, v, rew, bias_of=wrong_bias),
        }
        for what, bad in variants.items():
            bad_E, bad_b = wc.sgd_step(E, b, bad)
            fE, fb = wc.band_ratio(bad_E, bad_b, E, b, ref)
            print("    %-24s leaves the band by %.0f (table) %.0f (bias)" % (what, fE, fb))
            assert max(fE, fb) >= 10.0, (name, case.d, window, what, fE, fb)
