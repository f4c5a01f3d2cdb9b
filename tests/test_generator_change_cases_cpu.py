"""The premises of tests/test_gpu_generator_changes.py, checked without a GPU (with the oracle and the library built, as the
suite's other CPU tests that import the package) on the oracle: every pair of generators that
tests/support/generator_change_cases.py chooses on the host is SENSITIVE on every checked launch of every row -- at most half of
the walks end on the same node under A's tables as under B's -- so a launch that read anything of A after the change to B cannot
pass the bit-exact comparison by luck.  Every measured share is printed (-s shows them)."""
import numpy as np
import pytest

from tests.support import generator_change_cases as gc

# (graph, pair): the host-chosen pairs of the GPU matrix.  The E pair is used on the small graphs.
HOST_PAIRS = [("small1", "bias"), ("small3", "bias"), ("ca", "bias"), ("small1", "emb"), ("small3", "emb")]


@pytest.mark.parametrize("gname,pair", HOST_PAIRS, ids=["%s-%s" % p for p in HOST_PAIRS])
def test_every_checked_launch_is_sensitive(gname, pair):
    g = gc.graph(gname)
    A, B = gc.PAIRS[pair](g)
    for row in gc.ROWS:
        o, pre, checks = gc.run_sequence(g, g["roots"], A, B, row)
        assert len(checks) == len(gc.check_ops(row, g)) > 0
        for op, res, share in checks:
            walks = res["walks"] if op[0] == "d" else res
            print("%s %s pair, row %s, checked launch %s: %d walks, share of equal end nodes %.3f" % (gname, pair, row, op, len(walks["samples"]), share))
            assert share <= gc.MAX_EQUAL, (gname, pair, row, op, share)
            assert 2 * (walks["root_status"] == 0).sum() > len(g["roots"])   # (aborted roots count as EQUAL above; they are the minority)


def test_the_figures_of_fresh_trees():
    """D launch on stream 0 and G launch on stream 1 of fresh trees, bias pair, seed 7.  CA-GrQc in D mode does NOT meet the
    condition (most of its roots have one or two walks, and one candidate apart from the root): its D launches are not checked."""
    got = {}
    for gname in ("small1", "small3", "ca"):
        g = gc.graph(gname)
        got[gname] = gc.issue_table(g, *gc.bias_pair(g))
        print("%s: equal end nodes D-mode %.2f, G-mode %.2f" % ((gname,) + got[gname]))
    for gname in ("small1", "small3"):
        assert max(got[gname]) <= gc.MAX_EQUAL
    assert got["ca"][1] <= gc.MAX_EQUAL < got["ca"][0]
    assert not gc.graph("ca")["d_mode"] and gc.check_ops("es2", gc.graph("ca")) == [("g", 3)]


@pytest.mark.parametrize("gname", ["small1", "small3"])
def test_a_negated_embedding_table_changes_no_walk(gname):
    """Why the E pair negates the odd rows only: E[u] . E[v] is bilinear, -E scores exactly like E."""
    g = gc.graph(gname)
    d, gm = gc.issue_table(g, *gc.negated_emb_pair(g))
    assert d == gm == 1.0


def test_graphs():
    s1, s3, ca, p = gc.graph("small1"), gc.graph("small3"), gc.graph("ca"), gc.graph("small1_90")
    assert (s1["n"], s3["n"], ca["n"]) == (64, 90, 5242) and len(ca["roots"]) == 263
    assert p["n"] == 90 and len(p["rowptr"]) == 91 and np.array_equal(p["rowptr"][:65], s1["rowptr"]) and p["rowptr"][-1] == len(s1["col"])
    o = gc.Oracle(ca, ca["roots"], gc.bias_pair(ca)[0])
    assert o.dmax == 16   # (17 levels)
    # the replaced root list of the distribution-cache row puts another node on every slot
    assert not np.any(s1["roots"] == s1["roots"][::-1])


@pytest.mark.parametrize("pair", ["bias", "emb"])
def test_graph_softmax_pair_differs_on_every_slot_with_children(pair):
    """graph_softmax row: on every checked slot with children the float64 DP under A and under B differ by at least 100 x the
    tolerance of the comparison, so the private score table of A cannot pass for B's: the bias pair (set_bias, load_state) and
    the E pair (set_embeddings).  Needs no GPU, but the library built: host_graph_softmax lives in the package, which loads it."""
    from graphgan_amd.evaluation.generator_likelihood import host_graph_softmax
    from tests.test_gpu_graph_softmax import TOL_LOGP
    g, roots, _, _ = gc.gs_case()
    A, B = gc.PAIRS[pair](g)
    o = gc.Oracle(g, roots, A)
    off, nbr, base, _ = o.tree_lists()
    diffs = gc.gs_difference(host_graph_softmax, off, nbr, base, roots, A, B)
    with_kids = [d for k, d in diffs if k]
    print("graph_softmax: %d slots, %d with children, smallest max |logp_A - logp_B| = %.3g" % (len(diffs), len(with_kids), min(with_kids)))
    assert len(with_kids) >= gc.GS_SLOTS // 2
    assert min(with_kids) >= gc.GS_FACTOR * TOL_LOGP
