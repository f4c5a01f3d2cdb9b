"""The silhouette on the device (graphgan_amd/csrc/silhouette.hip: gg_silhouette, Engine.silhouette) and the NodeSilhouetteEval
evaluator on an engine, at the smallest shapes at which the padding of the cluster-sorted copy, the masking of pad columns, the
flush at a cluster change, the sum over wavefronts and column splits and the own-term skip can each go wrong.

EXACT: on tables whose rows are an integer t_i in [0, 64) on q^2 coordinates (tests/support/silhouette_ref.py, exact_table) every
distance q |t_i - t_j| and every sum is an integer below 2^24, exact in fp32 (and the table is exact in bf16), so sil, a, b and
nearest must equal the fp32 closed form BIT FOR BIT in both precisions.  The column split of the copy is 1 while the padded set
has at most 128 rows and above 1 beyond (silhouette.hip, gg_silhouette: column_split of the set alone), so m <= 33 with k = 2
runs one split, m >= 127 several, and m = 8 200 more than one row pass as well.
DERIVED: Gaussian tables against float64 (for bf16: float64 on the bf16-rounded table) inside the band silhouette_ref.band derives
from the inputs.  PROPERTIES: run-to-run bits, permutation, rows against the full call, the mean, every GG_EINVAL text.

Set GG_SIL_ERRTOL to a path to get the err / tol of every derived case appended there."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests.support import silhouette_ref as sr

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16")
# exact tables: (d, q) -> rows of the table (the cases draw their nodes from it)
EXACT_TABLES = {(8, 2): 8300, (50, 1): 300, (128, 4): 2700, (512, 4): 160}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


_engines, _t = {}, {}


def exact_t(d, q):
    if (d, q) not in _t:
        _t[(d, q)] = np.random.RandomState(1000 + d + q).randint(0, 64, size=EXACT_TABLES[(d, q)])
    return _t[(d, q)]


@pytest.fixture(scope="module")
def engine_of(ga):
    def get(key, make):
        if key not in _engines:
            while len(_engines) >= 4:
                _engines.pop(next(iter(_engines))).close()
            _engines[key] = ga.Engine(*make())
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()
    _t.clear()
    _float.clear()


def exact_engine(engine_of, d, q):
    def make():
        X = sr.exact_table(exact_t(d, q), d, q)
        return X, X[::-1].copy()  # the discriminator's table: the rows reversed
    return engine_of(("exact", d, q), make)


def sized_assign(rs, sizes):
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes))


def random_assign(rs, m, k):
    a = rs.randint(0, k, size=m)
    a[0], a[-1] = 0, k - 1  # at least two non-empty clusters
    return a


K128_SIZES = [(1, 31, 32, 33, 0)[c % 5] for c in range(128)]  # 2 489 rows, every fifth cluster empty

# (id, d, q, m, k, sizes or None)
EXACT_CASES = [("m%d" % m, 8, 2, m, 2 if m < 64 else 3, None) for m in (2, 31, 32, 33, 127, 128, 129, 257)] + [
    ("m8200-two-row-passes", 8, 2, 8200, 3, None),
    ("k3-sizes-1-31-32-33", 50, 1, 97, 5, (1, 31, 0, 32, 33)),
    ("k128-sizes-1-31-32-33-0", 128, 4, int(np.sum(K128_SIZES)), 128, K128_SIZES),
    ("k128-m2", 128, 4, 2, 128, [0] * 60 + [1] + [0] * 66 + [1]),
    ("boundary-inside-a-128-column-step", 128, 4, 200, 3, (1, 166, 33)),
    ("d50", 50, 1, 129, 3, None),
    ("d512-the-widest-table", 512, 4, 129, 3, None),
]


def check_exact(res, want, tag):
    for key in ("sil", "a", "b"):
        bad = np.flatnonzero(bits(res[key]) != bits(want[key]))
        assert len(bad) == 0, (tag, key, bad[:8], res[key][bad[:8]], want[key][bad[:8]])
    assert np.array_equal(res["nearest"], want["nearest"]), (tag, "nearest")
    assert res["mean"] == want["mean"], (tag, "mean", res["mean"], want["mean"])


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_tables_equal_the_fp32_closed_form_bit_for_bit(engine_of, case):
    name, d, q, m, k, sizes = case
    eng = exact_engine(engine_of, d, q)
    t_all = exact_t(d, q)
    rs = np.random.RandomState(len(name) + m)
    nodes = rs.permutation(len(t_all))[:m]
    assign = sized_assign(rs, sizes) if sizes is not None else random_assign(rs, m, k)
    assert len(assign) == m
    want = sr.fp32_closed_form(t_all[nodes], q, assign, k)
    rows = rs.randint(0, m, size=min(m, 40))
    for precision in PRECISIONS:
        res = eng.silhouette(nodes, assign, k=k, precision=precision)
        check_exact(res, want, (name, precision))
        part = eng.silhouette(nodes, assign, k=k, rows=rows, precision=precision)
        check_exact(part, sr.fp32_closed_form(t_all[nodes], q, assign, k, rows=rows), (name, precision, "rows"))
    singles = np.flatnonzero(np.bincount(assign, minlength=k)[assign] == 1)
    assert not res["sil"][singles].any() and not res["a"][singles].any()
    if name.startswith("k128-sizes"):
        assert len(singles) == 26 and m == 26 * 97 - 33 and 128 - len(np.unique(assign)) == 25  # (clusters 125 .. 127: sizes 1, 31, 32)
    # the discriminator's table holds the rows reversed
    rev = (len(t_all) - 1 - nodes).astype(np.int64)
    check_exact(eng.silhouette(rev, assign, k=k, which=1), want, (name, "which=1"))


def test_a_tie_in_b_goes_to_the_lowest_cluster(engine_of):
    eng = exact_engine(engine_of, 8, 2)
    t_all = exact_t(8, 2)
    pick = lambda v, n: np.flatnonzero(t_all == v)[:n]  # noqa: E731
    nodes = np.concatenate([pick(20, 4), pick(30, 3), pick(40, 4)])
    assert len(nodes) == 11
    mid = np.arange(4, 7)
    for assign, near_mid in (([0] * 4 + [1] * 3 + [2] * 4, 0), ([1] * 4 + [0] * 3 + [2] * 4, 1), ([2] * 4 + [0] * 3 + [1] * 4, 1)):
        assign = np.array(assign)
        want = sr.fp32_closed_form(t_all[nodes], 2, assign, 3)
        assert np.all(want["nearest"][mid] == near_mid) and np.all(want["b"][mid] == 20.0)
        for precision in PRECISIONS:
            check_exact(eng.silhouette(nodes, assign, k=3, precision=precision), want, ("tie", precision))


# ---- derived band on Gaussian tables
_float = {}
FLOAT_N = 700


def float_table(d):
    if d not in _float:
        rs = np.random.RandomState(50 + d)
        centre = rs.randint(0, 6, size=FLOAT_N)
        means = 0.5 * rs.randn(6, d)
        _float[d] = ((means[centre] + 0.3 * rs.randn(FLOAT_N, d)).astype(np.float32), (0.3 * rs.randn(FLOAT_N, d) + 0.05).astype(np.float32), centre)
    return _float[d]


def float_engine(engine_of, d):
    return engine_of(("float", d), lambda: float_table(d)[:2])


def report(tag, err, tol):
    ratio = float(np.max(np.asarray(err) / np.maximum(np.asarray(tol), 1e-300))) if np.size(err) else 0.0
    line = "%s: err/tol %.4g" % (tag, ratio)
    print(line)
    path = os.environ.get("GG_SIL_ERRTOL")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    return ratio


FLOAT_CASES = [(50, 300, 5, 0, False), (50, 601, 7, 1, True), (128, 600, 6, 0, False), (128, 257, 3, 1, True)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,m,k,which,sample", FLOAT_CASES)
def test_gaussian_tables_inside_the_derived_band(engine_of, d, m, k, which, sample, precision):
    eng = float_engine(engine_of, d)
    T = float_table(d)[which]
    rs = np.random.RandomState(d + m)
    nodes = rs.permutation(FLOAT_N)[:m]
    # a partition with structure (the table's own centres, folded to k) and one without
    assign = float_table(d)[2][nodes] % k if which == 0 else random_assign(rs, m, k)
    assign[0], assign[-1] = 0, k - 1
    rows = np.sort(rs.permutation(m)[:64]) if sample else None
    if precision == "fp32":
        X, ld = T[nodes].astype(np.float64), (d + 3) // 4 * 4
    else:
        ks_need = (d + 15) // 16
        X, ld = sr.round_bf16(T[nodes]).astype(np.float64), 16 * (4 if ks_need <= 4 else 8 if ks_need <= 8 else 16 if ks_need <= 16 else 32)
    ref = sr.float64_ref(X, assign, k, rows=rows)
    tol = sr.band(ref, X, assign, k, ld, rows=rows)
    res = eng.silhouette(nodes, assign, k=k, rows=rows, which=which, precision=precision)
    tag = "%s d %d m %d k %d%s" % (precision, d, m, k, " rows 64" if sample else "")
    worst = 0.0
    for key in ("a", "b", "sil"):
        worst = max(worst, report("%s %s" % (tag, key), np.abs(res[key].astype(np.float64) - ref[key]), tol[key]))
    worst = max(worst, report("%s mean" % tag, [abs(res["mean"] - ref["mean"])], [tol["mean"]]))
    assert worst < 1.0, (tag, worst)
    clear = tol["gap"] > 1.0  # the nearest cluster is decided outside the band
    assert clear.mean() > 0.9 and np.array_equal(res["nearest"][clear], ref["nearest"][clear]), tag
    assert res["mean"] == float(res["sil"].astype(np.float64).sum() / len(res["sil"]))
    assert res["ms"] > 0.0


# ---- properties
@pytest.mark.parametrize("precision", PRECISIONS)
def test_same_bits_on_every_run_under_permutation_and_with_rows(engine_of, precision):
    eng = float_engine(engine_of, 50)
    rs = np.random.RandomState(77)
    m, k = 601, 7
    nodes = rs.permutation(FLOAT_N)[:m]
    assign = random_assign(rs, m, k)
    one = eng.silhouette(nodes, assign, k=k, precision=precision)
    two = eng.silhouette(nodes, assign, k=k, precision=precision)
    for key in ("sil", "a", "b", "nearest"):
        assert np.array_equal(bits(one[key]), bits(two[key])), key
    assert one["mean"] == two["mean"] == float(one["sil"].astype(np.float64).sum() / m)
    assert len(np.unique(bits(one["sil"]))) > m // 2  # (no degenerate output)
    perm = rs.permutation(m)
    moved = eng.silhouette(nodes[perm], assign[perm], k=k, precision=precision)
    for key in ("sil", "a", "b", "nearest"):
        assert np.array_equal(bits(moved[key]), bits(one[key][perm])), key
    assert eng.silhouette(nodes, assign, precision=precision)["mean"] == one["mean"]  # k = max(assign) + 1
    more = eng.silhouette(nodes, assign, k=k + 9, precision=precision)  # further empty clusters change nothing
    assert np.array_equal(bits(more["sil"]), bits(one["sil"])) and np.array_equal(more["nearest"], one["nearest"])
    # rows: a sample with repeats, in any order -- the full call's entries
    rows = np.concatenate([rs.permutation(m)[:45], [600, 0, 600, 17, 17]])
    part = eng.silhouette(nodes, assign, k=k, rows=rows, precision=precision)
    for key in ("sil", "a", "b", "nearest"):
        assert np.array_equal(bits(part[key]), bits(one[key][rows])), key
    assert part["mean"] == float(part["sil"].astype(np.float64).sum() / len(rows))
    single = eng.silhouette(nodes, assign, k=k, rows=[333], precision=precision)
    assert bits(single["sil"])[0] == bits(one["sil"])[333] and single["mean"] == float(one["sil"][333])


def test_every_refusal_names_its_limit(ga, engine_of):
    eng = float_engine(engine_of, 50)
    lib, ctx = ga._lib.lib, eng._ctx
    m = 40
    nodes = np.arange(m, dtype=np.int32)
    assign = (np.arange(m) % 3).astype(np.int32)
    out = np.zeros(m, dtype=np.float32)
    near = np.zeros(m, dtype=np.int32)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(nodes=nodes, assign=assign, m=m, k=3, rows=None, n_rows=0, precision=0, which=0):
        return lib.gg_silhouette(ctx, which, P(nodes), P(assign), m, k, P(rows), n_rows, precision, P(out), P(out), P(out), P(near), None, None)

    assert call() == 0
    twice = nodes.copy()
    twice[7] = twice[3]
    far = nodes.copy()
    far[5] = FLOAT_N
    wrong = assign.copy()
    wrong[9] = 3
    for kwargs, text in ((dict(k=1), r"k = 1 outside \[2, 128\]"), (dict(k=129), r"k = 129 outside \[2, 128\]"),
                         (dict(m=1), r"m = 1 outside \[2, 2\^31 - 1\]"),
                         (dict(assign=np.zeros(m, dtype=np.int32)), r"1 non-empty cluster\(s\), at least 2 are needed"),
                         (dict(nodes=twice), r"node id 3 is repeated \(nodes\[7\]\)"),
                         (dict(nodes=far), r"nodes\[5\] = 700 out of range \[0, 700\)"),
                         (dict(assign=wrong), r"assign\[9\] = 3 outside \[0, k = 3\)"),
                         (dict(assign=-assign), r"assign\[1\] = -1 outside \[0, k = 3\)"),
                         (dict(rows=np.array([0, 40], dtype=np.int64), n_rows=2), r"rows\[1\] = 40 outside \[0, m = 40\)"),
                         (dict(rows=np.array([-1], dtype=np.int64), n_rows=1), r"rows\[0\] = -1 outside \[0, m = 40\)"),
                         (dict(rows=np.array([0], dtype=np.int64), n_rows=0), r"n_rows = 0 outside \[1, 2\^31 - 1\]"),
                         (dict(precision=2), r"precision must be 0 \(fp32\) or 1 \(bf16\)"), (dict(which=2), r"which must be 0 \(generator\) or 1")):
        assert call(**kwargs) == ga.GG_EINVAL, text
        msg = lib.gg_last_error(ctx).decode()
        assert msg.startswith("gg_silhouette: ") and re.search(text, msg), (text, msg)
    # the wrapper refuses the same arguments
    for kwargs, text in ((dict(k=1), "k must be an integer in"), (dict(k=True), "k must be"), (dict(k=2), "assign outside"), (dict(rows=[40]), "rows outside"),
                         (dict(rows=[]), "rows must be"), (dict(rows=[0.5]), "rows must be"), (dict(precision="fp16"), "precision must be"),
                         (dict(which=2), "which must be")):
        with pytest.raises(ValueError, match="silhouette: " + text):
            eng.silhouette(nodes, assign, **kwargs)
    with pytest.raises(ValueError, match="same length"):
        eng.silhouette(nodes, assign[:-1])
    with pytest.raises(ValueError, match="m = 1 outside"):
        eng.silhouette([3], [0])
    with pytest.raises(ValueError, match="node id outside"):
        eng.silhouette(far, assign)
    with pytest.raises(ValueError, match="nodes must be a 1-d array of integers"):
        eng.silhouette(nodes.astype(np.float32), assign)
    with pytest.raises(ga.GraphGANHipError, match="is repeated"):
        eng.silhouette(twice, assign)
    with pytest.raises(ga.GraphGANHipError, match="non-empty"):
        eng.silhouette(nodes, np.zeros(m, dtype=np.int64), k=2)


# ---- the evaluator on an engine
def _write_emb(path, emb):
    with open(path, "w") as f:
        f.write("%d\t%d\n" % emb.shape)
        for i, row in enumerate(np.asarray(emb, dtype=np.float64).tolist()):
            f.write(str(i) + "\t" + "\t".join(repr(x) for x in row) + "\n")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_evaluation_lines_on_blobs_match_the_host_evaluator(ga, tmp_path, precision):
    from graphgan_amd.graph_gan import GraphGAN
    from tests.support import kmeans_ref as kr
    X, labels, _ = kr.blobs(5, 16, 60)
    X = X.astype(np.float32)
    n = len(X)
    tables = (X, (0.5 * X).astype(np.float32))
    shuffled = np.random.RandomState(4).permutation(labels)
    cfg = types.SimpleNamespace(app="clustering", modes=["gen", "dis"], n_emb=16, test_filename="", result_filename=str(tmp_path / "res.txt"),
                                emb_filenames=[str(tmp_path / "gen.emb"), str(tmp_path / "dis.emb")], labels_filename=str(tmp_path / "labels.txt"),
                                engine_node_clustering=True, engine_cluster_silhouette=True, engine_sil_precision=precision)
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d %d\n" % (i, 7 * int(c)) for i, c in enumerate(shuffled))
    for path, T in zip(cfg.emb_filenames, tables):
        _write_emb(path, T)
    eng = ga.Engine(*tables)
    try:
        dev = GraphGAN.evaluation(types.SimpleNamespace(config=cfg, engine=eng, n_node=n, seed=0))
    finally:
        eng.close()
    host = GraphGAN.evaluation(types.SimpleNamespace(config=cfg, engine=None, n_node=n, seed=0))
    assert [ln.split(":")[0] for ln in dev] == ["gen_cluster", "dis_cluster", "gen_sil", "dis_sil"] == [ln.split(":")[0] for ln in host]
    pat = r"%s_sil:sil=(\S+) label_sil=(\S+) k=5 n=300 rows=300 precision=%s\n"
    for i, mode in enumerate(cfg.modes):
        got, want = re.fullmatch(pat % (mode, precision), dev[2 + i]), re.fullmatch(pat % (mode, "float64"), host[2 + i])
        assert got and want, (dev[2 + i], host[2 + i])
        T = tables[i] if precision == "fp32" else sr.round_bf16(tables[i])
        ld = 16 if precision == "fp32" else 64
        for grp, part in ((1, labels), (2, shuffled)):  # k-means finds the blobs (whatever it numbers them); the labels are shuffled
            ref = sr.float64_ref(T.astype(np.float64), part, 5)
            tol = sr.band(ref, T.astype(np.float64), part, 5, ld)["mean"]
            # (the host evaluator reads the unrounded text: for bf16 the reference moves to the rounded table, inside the band of the rounding)
            assert abs(float(got.group(grp)) - ref["mean"]) <= tol, (mode, grp)
            if precision == "fp32":
                assert abs(float(got.group(grp)) - float(want.group(grp))) <= tol + 1e-12, (mode, grp)
            report("evaluator %s %s %s" % (precision, mode, ("sil", "label_sil")[grp - 1]), [abs(float(got.group(grp)) - ref["mean"])], [tol])
        assert float(got.group(1)) > 0.5 > 0.05 > float(got.group(2))  # separated blobs; shuffled labels separate nothing


def test_ca_grqc_lines_are_reported(ga, tmp_path):
    """the shipped CA-GrQc embeddings under random labels: reported, not gated (there are no labels for this graph)"""
    from graphgan_amd.graph_gan import GraphGAN
    from tests.helpers import ca_grqc_init_embeddings
    from tests.test_gpu_e2e import write_reference_layout
    d, n, _ = write_reference_layout(str(tmp_path))
    emb = ca_grqc_init_embeddings(d, n).astype(np.float32)
    rs = np.random.RandomState(5)
    cfg = types.SimpleNamespace(app="clustering", modes=["gen", "dis"], n_emb=emb.shape[1], test_filename="", result_filename=str(tmp_path / "res.txt"),
                                emb_filenames=["", ""], labels_filename=str(tmp_path / "labels.txt"), engine_node_clustering=True,
                                engine_cluster_silhouette=True, engine_cluster_n_init=1, engine_cluster_max_iters=20)
    with open(cfg.labels_filename, "w") as f:
        f.writelines("%d %d\n" % (v, c) for v, c in zip(range(n), rs.randint(0, 8, size=n)))
    eng = ga.Engine(emb, (2 * emb).astype(np.float32))
    try:
        lines = GraphGAN.evaluation(types.SimpleNamespace(config=cfg, engine=eng, n_node=n, seed=0))
    finally:
        eng.close()
    print("".join(lines[2:]))
    for mode, line in zip(cfg.modes, lines[2:]):
        m = re.fullmatch(r"%s_sil:sil=(\S+) label_sil=(\S+) k=8 n=%d rows=%d precision=fp32\n" % (mode, n, n), line)
        assert m and -1.0 <= float(m.group(2)) <= 1.0 and -1.0 <= float(m.group(1)) <= 1.0, line
