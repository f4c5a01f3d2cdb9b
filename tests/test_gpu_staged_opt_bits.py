"""staged_opt_kernel against the bits of the build that tests/golden/staged_opt_parent.npz was recorded from
(tools/record_staged_golden.py, run on the commit before the kernel was pipelined).

The kernel sums the staged gradient rows of a table row in ascending key order and applies lazy Adam / SGD; the order of
its fp32 operations is a contract (row sum ((0 + x_k0) + x_k1) + ..., bias sum per lane over ranks t, t + 16, ... and the
xor butterfly 8, 4, 2, 1, adam_elem without contraction), so a restructured kernel must reproduce the recorded tables
bit for bit.  The float64 oracle cannot show that.

Cases (tests/staged_opt_cases.py): two fused D passes, (u, v) then (v, u), on 20 000 nodes with 16 800 pairs whose
neighbour rows collect exactly 1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 48, 63 and 64 gradients, a few hub rows above 64,
for d = 8 (lanes without a chunk), 50 (partial last chunk), 128 (two chunks), 200 and 256 (four), lazy Adam and SGD; one
with two simulated replicas (the sums go to the accumulators); whole-walk G passes on the small fixture graph with the
early staging index, without it, and with GG_STAGE_T=100000 (segments of hundreds of rows: minimum selection)."""
import os

import numpy as np
import pytest

from tests import staged_opt_cases as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "staged_opt_parent.npz")


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_every_segment_length_occurs():
    """The D cases' pairs: centre and neighbour ids disjoint, one run of 8 pairs per centre, and every listed segment
    length present among the neighbour rows, with hub rows above 64."""
    u, v, _ = sc.d_pairs()
    assert len(v) >= 16384 and u.max() < sc.N_CENTRE_IDS <= v.min() and v.max() < sc.N_NODE
    runs = u.reshape(-1, 8)
    assert (runs == runs[:, :1]).all() and len(np.unique(runs[:, 0])) == len(runs)
    mult = np.bincount(v, minlength=sc.N_NODE)
    present = set(np.unique(mult).tolist())
    for length in sc.LENGTHS:
        assert length in present, length
    assert (mult > 64).sum() >= 3


@pytest.mark.parametrize("name", list(sc.CASES))
def test_tables_equal_the_recorded_bits(ga, golden, name):
    got = sc.run_case(ga, name)
    keys = sorted(k for k in golden if k.startswith(name + "/"))
    assert keys == sorted("%s/%s" % (name, k) for k in got)
    for k in keys:
        want, have = golden[k], got[k.split("/", 1)[1]]
        if want.dtype.kind in "US":
            assert str(want) == str(have), k
        else:
            assert want.dtype == have.dtype and np.array_equal(want, have), k
