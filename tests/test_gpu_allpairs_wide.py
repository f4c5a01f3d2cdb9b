"""The wide all-pairs consumer (graphgan_amd/csrc/all_score.hip, all_score_reduce_bf16_x32_kernel<KS, RB, NW, LSE>) PAST its
prologue: column splits of 29 - 63 tiles, where the four tile buffers and the ring of four bias tiles are recycled, the bias of
tile t + 4 is a real number, the winning tile has an index above 3 and the tile count is odd; and the tie rule of its argmax.

A row list may repeat ids, so many row tiles are asked of a small table and the columns fall into few, long splits
(tests/support/allpairs_shapes.py; the premises, the plan included, are checked in tests/test_allpairs_shapes_cpu.py).

Three kinds of comparison.  EXACT: on tables of {-1, 0, 1} with an integer bias every score is an integer, `max` must equal the
float64 reference bit for bit and `argmax` must be numpy's (the lowest column among the maxima) -- with planted maxima in every
position of the ring and tie groups across the two lanes of a row, two registers of a lane, two tiles, two splits.  DERIVED: the
log-sum-exp on those exact scores within allpairs_shapes.lse_bound, which follows the kernel's arithmetic.  FLOAT: one dense
random table per KS within the band of test_all_score_streamed_consumer.  Everywhere the wide kernel's max / argmax equal the
narrow kernel's bit for bit.  The inputs keep the wide kernel's reference-free sum in range BY THE REFERENCE (in_range, asserted
in the CPU test): otherwise the call would be repeated with the narrow kernel and these tests would check the wrong one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import allpairs_shapes as ap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def narrow_call(eng, rows, **kw):
    os.environ["GG_ALLPAIRS_NARROW"] = "1"  # (read per call)
    try:
        return eng.all_score_reduce(rows, precision="bf16", **kw)
    finally:
        del os.environ["GG_ALLPAIRS_NARROW"]


def check_exact(tag, res, ref, rows, tiles):
    """max bit for bit, argmax numpy's, the log-sum-exp (if asked for) inside the derived bound; repeated ids identical.
    -> the largest log-sum-exp error (None without)"""
    idx = np.arange(len(ref["max"])) if rows is None else rows
    assert ap.bits_equal(res["max"], ref["max"][idx].astype(np.float32)), tag
    bad = np.flatnonzero(res["argmax"] != ref["argmax"][idx])
    assert len(bad) == 0, (tag, "row position, node, got, want", [(int(i), int(idx[i]), int(res["argmax"][i]), int(ref["argmax"][idx[i]])) for i in bad[:8]])
    if res["logsumexp"] is None:
        return None
    err = float(np.max(np.abs(res["logsumexp"].astype(np.float64) - ref["lse"][idx])))
    bound = ap.lse_bound(ref, tiles)
    print("%s: max |lse - float64| = %.3g, bound %.3g (%d tiles)" % (tag, err, bound, tiles))
    assert err <= bound, (tag, err, bound)
    if rows is not None:  # a node's row is the same sum in the same order wherever it is asked for
        order = np.argsort(rows, kind="stable")
        same = rows[order][1:] == rows[order][:-1]
        got = res["logsumexp"][order].view(np.uint32)
        assert np.array_equal(got[1:][same], got[:-1][same]), tag
    return err


def run_exact(ga, name, d):
    """every call of one exact case -> the largest log-sum-exp error"""
    c = ap.exact_case(name, d)
    rows, p = c["rows"], c["plan"]
    eng = ga.Engine(c["E"], c["E"])
    worst = 0.0
    try:
        for bias, ref, v in ((c["bias_a"], c["ref_a"], "ties"), (c["bias_b"], c["ref_b"], "last member raised")):
            eng.set_bias(0, bias)
            tag = "%s d=%d KS=%d %s" % (name, d, p["KS"], v)
            wide = eng.all_score_reduce(rows, precision="bf16")
            worst = max(worst, check_exact(tag + " rows listed", wide, ref, rows, max(p["tiles"])))
            check_exact(tag + " rows listed, no lse", eng.all_score_reduce(rows, precision="bf16", logsumexp=False), ref, rows, max(p["tiles"]))
            narrow = narrow_call(eng, rows, logsumexp=False)
            assert ap.bits_equal(wide["max"], narrow["max"]) and np.array_equal(wide["argmax"], narrow["argmax"]), tag
            if c["plan_all"] is not None:  # rows = None: n rows, an ordinary plan (splits of four tiles) on the same table
                t_all = max(c["plan_all"]["tiles"])
                worst = max(worst, check_exact(tag + " all rows", eng.all_score_reduce(None, precision="bf16"), ref, None, t_all))
                check_exact(tag + " all rows, no lse", eng.all_score_reduce(None, precision="bf16", logsumexp=False), ref, None, t_all)
    finally:
        eng.close()
    return worst


@pytest.mark.parametrize("name,d", ap.EXACT_CASES)
def test_wide_consumer_exact_past_the_prologue(ga, name, d):
    """LONG4: 4 splits of 32, 32, 32, 29 tiles (5 columns in the last); LONG1: one split of 63 tiles (15 columns in the last), also
    with a last row tile of one row; TINY: 33 and 5 nodes.  Integer tables: max and argmax bit for bit against float64, for a
    listed set of rows with repeats and for rows = None, with and without the log-sum-exp, with tie groups tied (the lowest
    column wins) and with their last member raised by one (it wins); the log-sum-exp inside the bound derived in
    allpairs_shapes.lse_bound; wide = narrow bit for bit.  Largest |log-sum-exp - float64| measured on an MI355X, KS = 4 / 8 /
    16 / 32: 3.3e-6 / 3.4e-6 / 2.0e-6 / 2.2e-6 at LONG4 (bound 4.6e-5), 5.3e-6 / 4.0e-6 / 3.1e-6 / 2.8e-6 at LONG1 (bound 7.6e-5),
    at most 1.0e-6 at TINY (bound 1.7e-5) -- about one spacing of fp32 at a log-sum-exp of 16 - 32 (1.9e-6)."""
    worst = run_exact(ga, name, d)
    print("%s d=%d KS=%d: largest |lse - float64| = %.3g" % (name, d, ap.bf16_shape(d), worst))


@pytest.mark.parametrize("name,d", ap.DENSE_CASES)
def test_wide_consumer_dense_floats_past_the_prologue(ga, name, d):
    """a dense random table (scores up to ~50: nothing that sparse +-1 rows could hide) at LONG4, one per KS: float64 on the
    bf16-rounded table within the band of test_all_score_streamed_consumer, 2e-3 max(1, max |S|); wide = narrow bit for bit"""
    c = ap.dense_case(name, d)
    rows, ref = c["rows"], c["ref"]
    eng = ga.Engine(c["E"], c["E"])
    try:
        eng.set_bias(0, c["bias"])
        wide = eng.all_score_reduce(rows, precision="bf16")
        narrow = narrow_call(eng, rows)
        no_lse = eng.all_score_reduce(rows, precision="bf16", logsumexp=False)
    finally:
        eng.close()
    band = 2e-3 * max(1.0, abs(ref["lo"]), abs(ref["hi"]))
    e_max = float(np.max(np.abs(wide["max"] - ref["max"][rows])))
    e_lse = float(np.max(np.abs(wide["logsumexp"] - ref["lse"][rows])))
    print("dense %s d=%d: |max - float64| %.3g, |lse - float64| %.3g, band %.3g" % (name, d, e_max, e_lse, band))
    assert e_max <= band and e_lse <= band
    # argmax: the reference's column, or one whose float64 score is within the band of the maximum
    Eb = ap.bf16_round(c["E"]).astype(np.float64)
    s_at = np.einsum("ij,ij->i", Eb[rows], Eb[wide["argmax"]]) + c["bias"].astype(np.float64)[wide["argmax"]]
    assert np.all(np.abs(s_at - ref["max"][rows]) <= band) and np.mean(wide["argmax"] == ref["argmax"][rows]) > 0.97
    assert ap.bits_equal(wide["max"], narrow["max"]) and np.array_equal(wide["argmax"], narrow["argmax"])
    assert ap.bits_equal(no_lse["max"], narrow["max"]) and np.array_equal(no_lse["argmax"], narrow["argmax"])
    assert np.max(np.abs(wide["logsumexp"] - narrow["logsumexp"])) <= band


def test_one_wave_instance_in_a_child_process():
    """all_score_reduce_bf16_x32_kernel<16, 4, 4> (GG_K7_NW4, read once per process): LONG4 at d = 256 with and without the
    log-sum-exp against the same exact reference, in ONE fresh child (tests/support/allpairs_nw4_child.py) that exits non-zero
    on a mismatch"""
    env = dict(os.environ, GG_K7_NW4="1")
    env.pop("GG_ALLPAIRS_NARROW", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.support.allpairs_nw4_child"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "one-wave instance ok" in r.stdout
