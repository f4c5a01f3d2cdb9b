"""Child process of tests/test_gpu_allpairs_wide.py::test_one_wave_instance_in_a_child_process.  The library reads GG_K7_NW4
once per process, so the <16, 4, 4> instance of the wide all-pairs kernel needs a process that starts with it: this one runs
LONG4 at d = 256 with and without the log-sum-exp, both bias vectors, against the exact float64 reference and exits non-zero
on a mismatch."""
import os
import sys

import numpy as np

from tests.support import allpairs_shapes as ap


def main():
    if not os.environ.get("GG_K7_NW4"):
        print("GG_K7_NW4 is not set: this process would run the default instance")
        return 2
    import graphgan_amd as ga
    name, d = ap.NW4_CASE
    c = ap.exact_case(name, d)
    p = ap.plan_of(name, d, nw4=True)
    rows, tiles = c["rows"], max(p["tiles"])
    eng = ga.Engine(c["E"], c["E"])
    bad = 0
    try:
        for bias, ref, v in ((c["bias_a"], c["ref_a"], "ties"), (c["bias_b"], c["ref_b"], "last member raised")):
            eng.set_bias(0, bias)
            for lse in (True, False):
                res = eng.all_score_reduce(rows, precision="bf16", logsumexp=lse)
                ok_max = ap.bits_equal(res["max"], ref["max"][rows].astype(np.float32))
                n_arg = int(np.count_nonzero(res["argmax"] != ref["argmax"][rows]))
                line = "<%d, %d, %d> %s lse=%d: max %s, %d wrong argmax" % (p["KS"], p["RB"], p["NW"], v, lse, "equal" if ok_max else "DIFFERS", n_arg)
                ok = ok_max and n_arg == 0
                if lse:
                    err = float(np.max(np.abs(res["logsumexp"].astype(np.float64) - ref["lse"][rows])))
                    bound = ap.lse_bound(ref, tiles)
                    line += ", |lse - float64| %.3g (bound %.3g)" % (err, bound)
                    ok = ok and err <= bound
                print(line)
                bad += not ok
    finally:
        eng.close()
    if bad:
        return 1
    print("one-wave instance ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
