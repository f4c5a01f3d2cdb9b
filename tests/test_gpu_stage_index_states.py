"""The early staging index through all of its states on ONE engine, against an engine that never builds it.

The generator pass's staging index is built on the side stream behind the G-mode walks (enqueue_path_slots) and consumed by
the next whole-walk g_pass; a caller that runs minibatch steps instead leaves it unconsumed, and after two such indexes in a
row the library stops building it and frees its buffers, until a whole-walk pass shows up again.  Engine A walks

    1. prepare_g + whole g_pass            the early index is consumed
    2. 4 x (prepare_g + g_pass of one 64-pair minibatch: the atomic-free kernel, reproducible)
                                           two indexes go unconsumed: from the third of these prepare_g calls on none is
                                           built and the buffers are freed
    3. prepare_g + whole g_pass            no early index: the pass builds its own
    4. prepare_g + whole g_pass            the early index again, in new (cleared) buffers

and engine B the same with GG_NO_EARLY_SLOTS=1 for its whole life.  The stage rows and their sum order do not depend on where
the index was built (tests/golden/staged_opt_parent.npz: the g_pass-early-* and g_pass-noearly-* digests are equal), so the
generator's tables of A and B must be equal bit for bit after every pass.

The graph is the small fixture of staged_opt_cases.run_g_case (90 nodes, d = 6, every node a root, 20 samples): at the
threshold of 64 it has both segment rows and hub rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WHOLE = 1 << 30
BATCHES = (WHOLE, 64, 64, 64, 64, WHOLE, WHOLE)


def _run(ga, opt):
    """(E, b) of the generator as uint32 after each pass of the sequence."""
    from tests.helpers import load_small
    g, n, graph = load_small(3)
    rs = np.random.RandomState(0)
    Ed = (rs.randn(n, g["E"].shape[1]) * 0.8).astype(np.float32)
    rowptr, col = ga.graph_to_csr(n, graph)
    slots = np.arange(n, dtype=np.int32)
    eng = ga.Engine(g["E"], Ed, optimizer=ga.GG_OPT_ADAM_LAZY if opt == "lazy" else ga.GG_OPT_SGD)
    eng.set_bias(0, g["b"])
    eng.set_graph_csr(rowptr, col)
    eng.build_trees(np.arange(n))
    passes = []
    for rnd, batch in enumerate(BATCHES):
        n_pairs = eng.prepare_g(slots, 20, 4, 2 * rnd + 1, fetch=False)
        assert n_pairs > 64  # (a 64-pair batch is a minibatch, not the whole pass)
        eng.g_pass([0], batch)
        passes.append(tuple(np.ascontiguousarray(x).view(np.uint32).copy() for x in (eng.get_embeddings(0), eng.get_bias(0))))
    eng.close()
    return passes


@pytest.mark.parametrize("opt", ["lazy", "sgd"])
def test_early_index_states_match_no_early_index(monkeypatch, opt):
    import graphgan_amd as ga
    monkeypatch.delenv("GG_NO_EARLY_SLOTS", raising=False)
    a = _run(ga, opt)
    monkeypatch.setenv("GG_NO_EARLY_SLOTS", "1")
    b = _run(ga, opt)
    assert len(a) == len(b) == len(BATCHES)
    for k in range(1, len(a)):  # every pass moved the tables: the comparison below is not one of untouched arrays
        assert not np.array_equal(a[k][0], a[k - 1][0]), k
    for k, ((Ea, ba), (Eb, bb)) in enumerate(zip(a, b)):
        assert Ea.dtype == Eb.dtype == np.uint32 and np.array_equal(Ea, Eb), "embeddings after pass %d" % k
        assert np.array_equal(ba, bb), "bias after pass %d" % k
