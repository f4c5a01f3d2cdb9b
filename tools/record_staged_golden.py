#!/usr/bin/env python
"""Record tests/golden/staged_opt_parent.npz: what the library AS BUILT writes into the tables in the cases of
tests/staged_opt_cases.py (SHA-256 of every table after every pass, 64 sample rows as uint32).

Run it on the GPU with the build whose results are to be kept -- the commit BEFORE a change of staged_opt_kernel -- and
commit the file; tests/test_gpu_staged_opt_bits.py then holds every later build to those bits.  Every case is run twice
and must reproduce itself, otherwise nothing is written.

    python tools/record_staged_golden.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "staged_opt_parent.npz"))
    args = ap.parse_args()
    import graphgan_amd as ga
    from tests import staged_opt_cases as sc

    out = {}
    for name in sc.CASES:
        first, second = sc.run_case(ga, name), sc.run_case(ga, name)
        for k in first:
            if not np.array_equal(first[k], second[k]):
                sys.exit("case %s does not reproduce itself (%s differs between two runs): not recorded" % (name, k))
            out["%s/%s" % (name, k)] = first[k]
        print("%-32s E %s  b %s" % (name, str(first["sha_E_pass1"])[:16], str(first["sha_b_pass1"])[:16]), flush=True)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print("wrote %s: %d cases, %d bytes" % (args.out, len(sc.CASES), size))
    if size >= 1 << 20:
        sys.exit("the fixture must stay under 1 MiB")


if __name__ == "__main__":
    main()
