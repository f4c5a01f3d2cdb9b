"""node2vec (p, q) biased pre-training walks on the host (no GPU): the numpy oracle of the rule P2b against a naive scalar
restatement, against the uniform oracle at equal weights, against the node2vec law by chi-square, its structural properties,
and the host side of the feature -- walk_bias(p, q), config knobs, binding, ABI number, Engine.pretrain_set_walk_bias."""
import ctypes

import numpy as np
import pytest

from tests.helpers import load_small
from tests.support import pretrain_bias_ref as bref
from tests.support import pretrain_ref as ref
from tests.support.graph_softmax_ref import chi2_pvalue_ok

BIASES = [(4096, 1024, 256), (256, 1024, 4096), (1, 64, 4096)]


def _csr(n, graph):
    from oracle import graphgan_oracle as orc
    return orc.graph_to_csr(n, graph)


@pytest.mark.parametrize("gi", [0, 1, 2, 3])
def test_vectorised_oracle_equals_the_scalar_walker(gi):
    _, n, graph = load_small(gi)
    rowptr, col = _csr(n, graph)
    starts = np.arange(n)
    for k, bias in enumerate(BIASES):
        got = bref.walks(rowptr, col, starts, 3, 12, 5 + gi, k, bias)
        want = bref.scalar_walks(rowptr, col, starts, 3, 12, 5 + gi, k, bias)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), bias


@pytest.mark.parametrize("gi", [0, 1, 2, 3])
def test_equal_weights_are_the_uniform_walk_bit_for_bit(gi):
    _, n, graph = load_small(gi)
    rowptr, col = _csr(n, graph)
    starts = np.arange(n)
    got = bref.walks(rowptr, col, starts, 3, 12, 9, 4, (7, 7, 7))
    want = ref.walks(rowptr, col, starts, 3, 12, 9, 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    r = bref.rows(rowptr, col, n, starts, 3, 12, 2, 3, 9, 4, (7, 7, 7))
    u = ref.rows(rowptr, col, n, starts, 3, 12, 2, 3, 9, 4)
    for key in ("paths", "path_len", "row_off", "center", "neighbor", "label"):
        assert np.array_equal(r[key], u[key]), key


@pytest.mark.parametrize("bias", [(4096, 1024, 256), (256, 1024, 4096)])
def test_second_step_follows_the_node2vec_law(bias):
    n, rowptr, col = bref.law_graph()
    a = bref.LAW_ARGS
    paths, plen = bref.walks(rowptr, col, np.array([a["start"]]), a["n_walks"], a["walk_len"], a["seed"], a["stream"], bias)
    counts, other = bref.law_counts(paths)
    print("law %s: conditioned walks %d, shares %s, expected %s"
          % (bias, counts.sum(), np.round(counts / counts.sum(), 4).tolist(), np.round(bref.law_expected(bias) / bref.law_expected(bias).sum(), 4).tolist()))
    assert other == 0 and counts.sum() > 10_000
    assert chi2_pvalue_ok(counts, bref.law_expected(bias), 1e-6)


@pytest.mark.parametrize("gi", [0, 1, 2, 3])
def test_every_step_is_an_edge_and_walks_end_only_at_degree_zero(gi):
    _, n, graph = load_small(gi)
    rowptr, col = _csr(n, graph)
    deg = np.diff(rowptr)
    edges = {(a, int(b)) for a in range(n) for b in col[rowptr[a]:rowptr[a + 1]]}
    for bias in BIASES:
        paths, plen = bref.walks(rowptr, col, np.arange(n), 3, 12, 3, 1, bias)
        for g in range(len(plen)):
            p = paths[g, :plen[g]]
            assert p[0] == g // 3 and np.all(paths[g, plen[g]:] == -1)
            assert all((int(p[h - 1]), int(p[h])) in edges for h in range(1, len(p)))
            assert plen[g] == 12 or deg[p[-1]] == 0


def test_fallback_runs_on_a_star():
    """(4096, 1, 1) on a star: from the centre almost every candidate is rejected 32 times, so the exact draw decides; it
    equals the scalar walker there too."""
    m = 300
    rowptr = np.concatenate([[0, m], m + np.arange(1, m + 1)]).astype(np.int64)
    col = np.concatenate([np.arange(1, m + 1), np.zeros(m)]).astype(np.int32)
    st = {}
    got = bref.walks(rowptr, col, np.arange(1, 31), 2, 20, 1, 0, (4096, 1, 1), stats=st)
    want = bref.scalar_walks(rowptr, col, np.arange(1, 31), 2, 20, 1, 0, (4096, 1, 1))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert st["fallback_hops"] > st["biased_hops"] // 2 and np.all(st["fallback_from"] == 0)


def test_walk_bias_of_p_and_q():
    from graphgan_amd import pretrain
    assert pretrain.walk_bias(0.25, 4) == (4096, 1024, 256)
    assert pretrain.walk_bias(4, 0.25) == (256, 1024, 4096)
    a = pretrain.walk_bias(1, 1)
    assert a[0] == a[1] == a[2]
    assert pretrain.walk_bias(1 / 16, 16) == (4096, 256, 16) and pretrain.walk_bias(16, 1 / 16) == (16, 256, 4096)
    assert all(isinstance(v, int) and 1 <= v <= 65536 for v in pretrain.walk_bias(16, 16))
    for p, q in ((0.06, 1), (1, 16.5), (0, 1), (1, -1), (float("nan"), 1), (1, float("inf"))):
        with pytest.raises(ValueError):
            pretrain.walk_bias(p, q)


def test_config_defaults_are_the_uniform_walk():
    from graphgan_amd import config
    assert config.engine_pretrain_p == 1.0 and config.engine_pretrain_q == 1.0


def test_abi_declares_the_walk_bias_entry_point():
    from graphgan_amd import _lib
    assert "gg_pretrain_set_walk_bias" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gg_pretrain_set_walk_bias")
    assert _lib.lib.gg_abi_version() == _lib.ABI_VERSION == _lib.header_abi_version() == 9  # an additive entry point


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_engine_walk_bias_validates_before_the_device(monkeypatch):
    from graphgan_amd import engine as eng_mod
    monkeypatch.setattr(eng_mod, "lib", _NoLib())
    e = eng_mod.Engine.__new__(eng_mod.Engine)
    e.n_node, e.n_emb = 10, 4
    e._ctx = ctypes.c_void_p()
    for bad in ((0, 1, 1), (1, 65537, 1), (1, 1, 0), (1.0, 1, 1), (1, 2.5, 1), (True, 1, 1), (1, 1, False), (-1, 1, 1), ("1", 1, 1),
                (1, 1, None)):
        with pytest.raises(ValueError):
            e.pretrain_set_walk_bias(*bad)
    with pytest.raises(AssertionError):  # valid weights do reach the library
        e.pretrain_set_walk_bias(1, 65536, np.int32(7))
