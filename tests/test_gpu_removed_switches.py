"""The timing switches that used to make the shipped kernels compute wrong trees, walks or sums (GG_WALK_EXPERIMENT,
GG_BFS_EXPERIMENT, GG_LZ_ABLATE, GG_DET_PROFILE, GG_K7_DBG) are gone from the library: with every one of them set, the
device BFS (whole and lazy), the level kernels, the resolve kernel and the finisher are still bit-exact against the oracle."""
import numpy as np
import pytest

from tests.helpers import load_small
from tests.test_gpu_lazy import run_lazy
from tests.test_gpu_walk import run_both

pytestmark = pytest.mark.gpu

REMOVED = {"GG_WALK_EXPERIMENT": "1", "GG_BFS_EXPERIMENT": "2", "GG_LZ_ABLATE": "1", "GG_DET_PROFILE": "1", "GG_K7_DBG": "1"}


def test_removed_switches_change_nothing(monkeypatch):
    for name, value in REMOVED.items():  # (before any engine exists: gg_create and the first launches read the environment)
        monkeypatch.setenv(name, value)
    import graphgan_amd as ga
    g, n, graph = load_small(1)
    rowptr, col = ga.graph_to_csr(n, graph)
    # whole trees from the device BFS, then a D and a G round of walks
    hops = run_both(ga, n, rowptr, col, np.arange(n), g["E"], g["b"], rounds=2, seed=1919, device_bfs=True)
    assert hops > 0
    # lazy trees (exact through a level of 8 nodes at most), every resolved list against the whole trees
    hops, resolved, st = run_lazy(ga, n, rowptr, col, np.arange(n), g["E"], g["b"], rounds=4, seed=4322, node_cap=8, expect_lazy=False,
                                  monkeypatch=monkeypatch)
    assert hops > 100
