"""GPU parity of the walk sampler at every template instance of its row dot (spec S1): level_score_kernel<NCH> and
walk_sample_kernel<NCH, LAZY> with NCH = 1, 2, 4, 8 float4 chunks per lane of a 16-lane group, in the modes that make each of
them score hops, at the widths where the instance changes (65, 129, 257), where a row is padded inside its last float4 (1, 509)
and at the widest row gg_create accepts (512) -- BIT-EXACT against the C oracle (oracle/walk_oracle.c, orc_dot16), on whole trees
and on lazy trees.  tests/support/row_dot_shapes.py holds the restated dispatch and the case lists;
tests/test_row_dot_shapes_cpu.py checks that the lists reach every instance and that the oracle's walks change when any 64-column
block or the last chunk of the rows is dropped, so a kernel that reads fewer chunks than its row has cannot pass here."""
import numpy as np
import pytest

from tests.helpers import load_small, star_graph_edges
from tests.support import row_dot_shapes as rd
from tests.test_gpu_lazy import run_lazy
from tests.test_gpu_walk import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def set_mode(monkeypatch, mode):
    """gg_create reads the variables: set before the engine exists"""
    for var in ("GG_WALK_LEVELS", "GG_ES_MODE", "GG_FIN_THRESHOLD", "GG_WALK_SPLIT"):
        monkeypatch.delenv(var, raising=False)
    for var, val in rd.walk_env(mode).items():
        monkeypatch.setenv(var, val)


@pytest.mark.parametrize("d,mode", rd.WALK_CASES)
def test_walks_bit_exact_at_every_width_instance(ga, d, mode, monkeypatch):
    """D, G, D, G on load_small(1), every root: the second pair of rounds reads the edge scores the first one cached, and the
    tree mutation state (Q3) is compared after every round."""
    set_mode(monkeypatch, mode)
    g, n, graph = load_small(1)
    E, b = rd.table(n, d)
    rowptr, col = ga.graph_to_csr(n, graph)
    hops = run_both(ga, n, rowptr, col, np.arange(n), E, b, rounds=4, seed=99)
    assert hops > 100


@pytest.mark.parametrize("d,mode", rd.HUB_CASES)
def test_hub_list_at_a_wide_row(ga, d, mode, monkeypatch):
    """The 1 501-candidate hub list of tests/test_gpu_walk.py's test_hub_lists_longer_than_one_pass at a row of 320 floats: in
    "finisher" mode through score_block<8> and its HBM-scratch branch (sbuf_glb), in "levels" mode through the hub path."""
    set_mode(monkeypatch, mode)
    edges, n = star_graph_edges(rd.HUB_LEAVES)
    rowptr, col = ga.edges_to_csr(n, edges)
    E, b = rd.table(n, d)
    roots = np.array([0, 1, 2, n - 1, n - 2], dtype=np.int32)
    run_both(ga, n, rowptr, col, roots, E, b, rounds=4, seed=5, n_sample=200)


@pytest.mark.parametrize("gi,cap,d,mode", rd.LAZY_CASES)
def test_lazy_walks_bit_exact_at_every_width_instance(ga, gi, cap, d, mode, monkeypatch):
    """Lazy trees (exact through a level, deeper lists resolved by the walks): the walks against the oracle's on whole trees,
    every resolved list against the whole trees' BFS order (check_lazy_arrays, inside run_lazy)."""
    set_mode(monkeypatch, mode)
    g, n, graph = load_small(gi)
    E, b = rd.table(n, d)
    rowptr, col = ga.graph_to_csr(n, graph)
    hops, resolved, st = run_lazy(ga, n, rowptr, col, np.arange(n), E, b, rounds=4, seed=4321 + gi, node_cap=cap, expect_lazy=False,
                                  monkeypatch=monkeypatch)
    assert hops > 100
