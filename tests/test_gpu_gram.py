"""The centred Gram sweep on the device (graphgan_amd/csrc/gram.hip: gg_gram, Engine.gram / pca / pca_transform) and the
embedding-spectrum lines of ``GraphGAN.evaluation``, at the smallest shapes at which the sweep can go wrong: every width instance
DT = ceil(d / 32), the ragged widths 33 and 50, one row, a row short of / a row past a tile, three tiles, more tiles than workgroups.

Three kinds of comparison (tests/support/gram_ref.py).  EXACT: integer tables and centres against the int64 closed form -- a
padding row that entered as 0 - center, a dropped or doubled row, a stale tile or a partial added twice changes an integer.
BITWISE: NULL centre against a zero centre, the sums-only sweep against the full one, a rerun, the mirror entries, and on dyadic
tables the device PCA against the float64 host PCA.  DERIVED: Gaussian tables against float64 inside the bands
(m + 3) 2^-24 sum_i |C_ij| |C_il| (gram) and (m + 1) 2^-24 sum_i |C_ij| (sums), worst case of an m-term float32 chain.

Set GG_GRAM_ERRTOL to a path to get the largest err / tol of every derived case appended there."""
import ctypes
import os
import types

import numpy as np
import pytest

from tests.support import gram_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


_engines = {}
MAX_ENGINES = 4


@pytest.fixture(scope="module")
def int_engine(ga):
    def get(d):
        if d not in _engines:
            while len(_engines) >= MAX_ENGINES:
                _engines.pop(next(iter(_engines))).close()
            _engines[d] = ga.Engine(*gr.int_tables(d))
        return _engines[d]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def report(tag, err, tol):
    ratio = float(np.max(err / np.maximum(tol, 1e-300))) if np.size(err) else 0.0
    line = "%s: err/tol %.4g" % (tag, ratio)
    print(line)
    path = os.environ.get("GG_GRAM_ERRTOL")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    return ratio


# ---- 1. exact on integer tables
def exact_leg(eng, d, m, which, seed, centred):
    rs = np.random.RandomState(seed)
    nodes = gr.draw_nodes(rs, m)
    center = None
    if centred:
        center = rs.randint(-1, 2, size=d).astype(np.float32)
        center[0] = 1.0  # (never all zero: a padding row that entered as 0 - center shows in column 0)
    T = gr.int_tables(d)[which]
    want_s, want_g = gr.int_gram(T[nodes], center)
    got = eng.gram(nodes, center=center, which=which)
    tag = "exact (m %d, d %d, which %d, centre %s)" % (m, d, which, centred)
    assert got["sums"].dtype == np.float64 and got["gram"].shape == (d, d), tag
    assert np.array_equal(got["sums"], want_s.astype(np.float64)), (tag, "sums", np.flatnonzero(got["sums"] != want_s)[:8])
    bad = np.argwhere(got["gram"] != want_g.astype(np.float64))
    assert len(bad) == 0, (tag, "gram", bad[:8], got["gram"][tuple(bad[:8].T)], want_g[tuple(bad[:8].T)])
    assert gr.bits_equal(got["gram"], got["gram"].T.copy()), (tag, "symmetry")
    alone = eng.gram(nodes, center=center, which=which, gram=False)
    assert alone["gram"] is None and gr.bits_equal(alone["sums"], got["sums"]), (tag, "sums-only")


@pytest.mark.parametrize("d", [8, 32, 33, 50, 64, 96, 128, 160, 192, 224, 256])
def test_exact_on_every_width_at_the_tile_edges(int_engine, d):
    eng = int_engine(d)
    for m in (1, 2, 63, 64, 65, 129):
        for centred in (False, True):
            exact_leg(eng, d, m, (m + d) & 1, 31 * d + m, centred)
    exact_leg(eng, d, 65, 1 - ((65 + d) & 1), d, True)  # the other table


def test_exact_with_more_tiles_than_workgroups(ga, int_engine):
    m = 64 * ga._lib.GRAM_MAX_GRID + 1  # workgroup 0 takes a second tile, with one valid row
    assert m <= 40000
    for centred in (False, True):
        exact_leg(int_engine(8), 8, m, 0, 5, centred)
    exact_leg(int_engine(8), 8, 2 * m + 700, 1, 6, True)  # three tiles for some workgroups, two for the others


# ---- 2. bit contracts
@pytest.mark.parametrize("d", [50, 128])
def test_null_centre_is_a_zero_centre_and_reruns_repeat(ga, d):
    rs = np.random.RandomState(40 + d)
    X = (0.4 * rs.randn(3000, d) + 0.3).astype(np.float32)
    X[5, :4] = [-0.0, 0.0, 1e-40, -1e-40]  # signed zeros and subnormals pass through x - (+0) unchanged
    eng = ga.Engine(X, X)
    try:
        nodes = rs.randint(0, 3000, size=1500)
        nodes[:2] = 5
        a = eng.gram(nodes)
        z = eng.gram(nodes, center=np.zeros(d, dtype=np.float32))
        assert gr.bits_equal(a["sums"], z["sums"]) and gr.bits_equal(a["gram"], z["gram"])
        c = X[nodes].astype(np.float64).mean(axis=0).astype(np.float32)
        full, again, alone = eng.gram(nodes, center=c), eng.gram(nodes, center=c), eng.gram(nodes, center=c, gram=False)
        assert gr.bits_equal(full["sums"], again["sums"]) and gr.bits_equal(full["gram"], again["gram"])
        assert alone["gram"] is None and gr.bits_equal(alone["sums"], full["sums"])
        assert gr.bits_equal(full["gram"], full["gram"].T.copy())
        assert not gr.bits_equal(full["gram"], a["gram"]) and full["ms"] > 0
    finally:
        eng.close()


# ---- 3. Gaussian tables against float64 inside the derived bands
_gauss = {}


def gaussian_case(ga, m, d):
    if (m, d) not in _gauss:
        rs = np.random.RandomState(1000 + d)
        X = (0.5 * rs.randn(m + 100, d) * (1.0 + np.arange(d) % 7)[None, :] + rs.randn(d)[None, :]).astype(np.float32)
        nodes = rs.permutation(m + 100)[:m]
        center = X[nodes].astype(np.float64).mean(axis=0).astype(np.float32)
        _gauss[(m, d)] = (X, nodes, center)
    return _gauss[(m, d)]


@pytest.mark.parametrize("m,d", [(200, 50), (4097, 128), (1000, 256)])
def test_gaussian_against_float64(ga, m, d):
    X, nodes, center = gaussian_case(ga, m, d)
    eng = ga.Engine(X, X[::-1].copy())
    try:
        got = eng.gram(nodes, center=center)
        raw = eng.gram(nodes)
    finally:
        eng.close()
    for tag, res, c in (("centred", got, center), ("raw", raw, None)):
        G64, g_tol, s64, s_tol = gr.bands(X[nodes], c)
        rg = report("gram %s (m %d, d %d)" % (tag, m, d), np.abs(res["gram"] - G64), g_tol)
        rs_ = report("sums %s (m %d, d %d)" % (tag, m, d), np.abs(res["sums"] - s64), s_tol)
        assert rg <= 1.0 and rs_ <= 1.0, (tag, rg, rs_)


# ---- 4. Engine.pca
def check_sign_convention(components):
    lead = np.argmax(np.abs(components), axis=1)
    assert (components[np.arange(len(components)), lead] > 0).all()


@pytest.mark.parametrize("m,d", [(132, 50), (4, 8), (260, 256)])
def test_pca_equals_the_host_pca_on_a_dyadic_table(ga, m, d):
    from graphgan_amd.evaluation import embedding_spectrum as es
    X = gr.dyadic_table(m, d, seed=m + d)
    filler = np.full((3, d), 7.5, dtype=np.float32)  # rows that are not part of the fit
    T = np.vstack([filler[:1], X, filler[1:]])
    nodes = np.arange(1, m + 1)
    eng = ga.Engine(T, T)
    try:
        b = eng.gram(nodes, center=(X.astype(np.float64).sum(axis=0) / m).astype(np.float32))
        assert not b["sums"].any()  # the residual sums about a dyadic mean: exact zeros
        fit = eng.pca(nodes, n_components=min(d, 5))
    finally:
        eng.close()
    host = es.host_pca(T, nodes, n_components=min(d, 5))
    assert fit["m"] == m and gr.bits_equal(fit["mean"], host["mean"]) and gr.bits_equal(fit["mean64"], host["mean64"])
    assert gr.bits_equal(fit["cov"], host["cov"])
    assert np.allclose(fit["cov"], np.cov(X.astype(np.float64), rowvar=False, bias=True), rtol=0, atol=1e-13)
    assert gr.bits_equal(fit["eigenvalues"], host["eigenvalues"]) and gr.bits_equal(fit["components"], host["components"])
    assert fit["components"].shape == (min(d, 5), d) and fit["components"].dtype == np.float32
    assert (np.diff(fit["eigenvalues"]) <= 0).all() and (fit["eigenvalues"] >= 0).all()
    check_sign_convention(fit["components"])


_blobs = {}


def blob_table():
    if "t" not in _blobs:
        rs = np.random.RandomState(77)
        centres = 3.0 * rs.randn(6, 40)
        labels = rs.randint(0, 6, size=1500)
        X = (centres[labels] + 0.5 * rs.randn(1500, 40) * (1.0 + np.arange(40) % 5)[None, :] + 2.0).astype(np.float32)
        _blobs["t"] = X
    return _blobs["t"]


def test_pca_eigenvalues_on_blobs_inside_the_weyl_band(ga):
    from graphgan_amd.evaluation import embedding_spectrum as es
    X = blob_table()
    nodes = np.arange(0, 1500, 1)[::-1].copy()
    m = len(nodes)
    eng = ga.Engine(X, X)
    try:
        fit = eng.pca(nodes)
    finally:
        eng.close()
    G64, g_tol, r64, r_tol = gr.bands(X[nodes], fit["mean"])
    cov64 = es.pca_cov(G64, r64, m)
    lam64 = np.maximum(np.sort(np.linalg.eigvalsh(cov64))[::-1], 0.0)
    a = np.abs(r64)
    tol = g_tol + (np.outer(a, r_tol) + np.outer(r_tol, a) + np.outer(r_tol, r_tol)) / m
    bound = float(np.sqrt((tol * tol).sum())) / m
    err = np.abs(fit["eigenvalues"] - lam64)
    ratio = report("pca eigenvalues on blobs (m %d, d %d)" % (m, X.shape[1]), err, np.full_like(err, bound))
    assert ratio <= 1.0
    assert np.allclose(fit["eigenvalues"], es.host_pca(X, nodes)["eigenvalues"], rtol=1e-5, atol=1e-9)
    check_sign_convention(fit["components"])
    assert abs(float(fit["components"][0].astype(np.float64) @ fit["components"][1].astype(np.float64))) < 1e-5


# ---- 5. pca_transform
def test_pca_transform_is_exact_on_an_integer_table(int_engine):
    d = 50
    eng = int_engine(d)
    T = gr.int_tables(d)[1]
    rs = np.random.RandomState(3)
    nodes = gr.draw_nodes(rs, 700)
    mean = rs.randint(-1, 2, size=d).astype(np.float32)
    for n_comp in (1, 2, 33, 50):
        cols = rs.permutation(d)[:n_comp]
        signs = rs.choice([-1.0, 1.0], size=n_comp)
        W = np.zeros((n_comp, d), dtype=np.float32)
        W[np.arange(n_comp), cols] = signs
        got = eng.pca_transform(nodes, mean, W, which=1)
        want = (signs[None, :] * (T[nodes][:, cols].astype(np.float64) - mean[cols].astype(np.float64)[None, :])).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (700, n_comp)
        assert np.array_equal(got, want), n_comp


def test_pca_transform_on_blobs_against_float64(ga):
    X = blob_table()
    d = X.shape[1]
    nodes = np.arange(1500)
    eng = ga.Engine(X, X)
    try:
        fit = eng.pca(nodes, n_components=3)
        got = eng.pca_transform(np.arange(0, 1500, 3), fit["mean"], fit["components"])
    finally:
        eng.close()
    W, mu, R = fit["components"].astype(np.float64), fit["mean"].astype(np.float64), X[::3].astype(np.float64)
    want = (R - mu) @ W.T
    tol = (d + 2) * gr.U * (np.abs(R) @ np.abs(W).T + (np.abs(W) @ np.abs(mu))[None, :])
    assert report("pca_transform on blobs", np.abs(got - want), tol) <= 1.0
    assert want[:, 0].var() > want[:, 1].var() > want[:, 2].var()


def test_cli_on_the_device_agrees_with_its_host_leg(tmp_path):
    """python -m graphgan_amd.project: ids out of order in the file, the fit on the nodes with a training edge only.  The two legs
    fit the same rows in different precisions: the top two eigenvalues of the blob table are separated by more than 1, the
    covariances agree to about 10^-6 (the Weyl test above), so the coordinates agree far inside 10^-3."""
    from graphgan_amd import project
    X = blob_table()[:300]
    emb, train = tmp_path / "x.emb", tmp_path / "train.txt"
    order = np.random.RandomState(2).permutation(300)
    emb.write_text("300\t40\n" + "".join("%d\t%s\n" % (i, "\t".join(repr(float(v)) for v in X[i])) for i in order))
    train.write_text("".join("%d\t%d\n" % (i, i + 1) for i in range(0, 250)))  # nodes 251 .. 299 are projected, not fitted
    outs = []
    for leg in ([], ["--host"]):
        out = tmp_path / ("coords%d.tsv" % len(outs))
        assert project.main(["--emb", str(emb), "--out", str(out), "--train", str(train), "--dim", "2"] + leg) == 0
        rows = [ln.split("\t") for ln in out.read_text().splitlines()]
        assert [int(r[0]) for r in rows] == list(range(300)) and all(len(r) == 3 for r in rows)
        outs.append(np.array([[float(v) for v in r[1:]] for r in rows]))
    assert np.abs(outs[0] - outs[1]).max() < 1e-3 and outs[1][:251].var(axis=0).min() > 1.0
    assert np.abs(outs[1][:251].mean(axis=0)).max() < 1e-5  # centred on the fitted rows


# ---- 6. refusals
def test_argument_errors_name_the_entry(ga, int_engine):
    eng = int_engine(8)
    lib, ctx = ga._lib.lib, eng._ctx
    n = gr.N_TABLE
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nodes = np.arange(10, dtype=np.int32)
    sums = np.zeros(8)

    def call(ctx=ctx, which=0, nodes=nodes, m=None, center=None):
        return lib.gg_gram(ctx, which, p(nodes), len(nodes) if m is None else m, None if center is None else p(center), p(sums), None, None)

    outside = nodes.copy()
    outside[7] = n
    nan_centre = np.zeros(8, dtype=np.float32)
    nan_centre[3] = np.nan
    wide = ga.Engine(np.zeros((4, 260), np.float32), np.zeros((4, 260), np.float32))
    try:
        cases = [(lambda: call(which=2), ctx, "which must be 0"), (lambda: call(m=0), ctx, "m = 0 outside [1, 2^31 - 1]"),
                 (lambda: call(nodes=outside), ctx, "node id %d (entry 7) outside [0, %d)" % (n, n)),
                 (lambda: call(center=nan_centre), ctx, "center[3] = nan is not finite"),
                 (lambda: call(ctx=wide._ctx, nodes=np.arange(3, dtype=np.int32)), wide._ctx, "supports n_emb <= 256 (got 260)")]
        for fn, c, text in cases:
            assert fn() == ga.GG_EINVAL, text
            msg = lib.gg_last_error(c).decode()
            assert text in msg and "gg_gram" in msg, (text, msg)
    finally:
        wide.close()
    for bad in (dict(which=2), dict(center=np.zeros(7, np.float32)), dict(center=nan_centre)):
        with pytest.raises(ValueError, match="gram"):
            eng.gram(nodes, **bad)
    with pytest.raises(ValueError, match="gram"):
        eng.gram([0, n])
    with pytest.raises(ValueError, match="pca: needs m >= 2 rows, got 1"):
        eng.pca([3])
    with pytest.raises(ValueError, match="pca_transform: n_components = 129 outside"):
        eng.pca_transform(nodes, np.zeros(8, np.float32), np.zeros((129, 8), np.float32))
    assert eng.gram(nodes)["sums"].shape == (8,)  # the engine stays usable


# ---- 7. the results lines
def test_evaluation_appends_the_spectrum_lines(ga, tmp_path):
    from graphgan_amd.evaluation import embedding_spectrum as es
    from graphgan_amd.graph_gan import GraphGAN
    from tests.helpers import load_ca_grqc
    from tests.test_gpu_e2e import make_cfg
    m, d = 132, 16
    n = m + 2  # nodes 40 and n - 1 have no training edge: their rows are not part of the spectrum
    trained = np.array([v for v in range(n) if v not in (40, n - 1)])
    Tg, Td = np.full((n, d), 9.25, dtype=np.float32), np.full((n, d), -3.5, dtype=np.float32)
    Tg[trained], Td[trained] = gr.dyadic_table(m, d, 1), gr.dyadic_table(m, d, 2)[:, ::-1]
    base = str(tmp_path)
    cfg = make_cfg(base, app="none", n_emb=d)
    os.makedirs(os.path.dirname(cfg.train_filename))
    os.makedirs(os.path.dirname(cfg.emb_filenames[0]))
    ring = np.stack([trained, np.roll(trained, -1)], axis=1)
    test_edges = np.array([[40, 0], [n - 1, 5], [2, 9]])
    for path, edges in ((cfg.train_filename, ring), (cfg.test_filename, test_edges)):
        with open(path, "w") as f:
            f.writelines("%d\t%d\n" % (a, b) for a, b in edges.tolist())
    eng = ga.Engine(Tg, Td)
    try:
        eng.set_graph_csr(*ga.edges_to_csr(n, ring))
        g = types.SimpleNamespace(config=cfg, engine=eng, n_node=n, seed=0, gen_likelihood=lambda: dict(nll=1.0, reach=1.0, n=3))
        cfg.engine_link_rank, cfg.engine_gen_nll = True, True
        want = GraphGAN.evaluation(g)  # the knob's default: off
        assert [ln.split(":")[0] for ln in want] == ["gen_rank", "dis_rank", "gen_nll"]
        cfg.engine_emb_spectrum = True
        lines = GraphGAN.evaluation(g)
        assert [ln.split(":")[0] for ln in lines] == ["gen_rank", "dis_rank", "gen_spec", "dis_spec", "gen_nll"]
        assert lines[:2] + lines[4:] == want
        assert open(cfg.result_filename).read() == "".join(want + lines)
        for i, mode in enumerate(("gen", "dis")):  # the engine-less float64 evaluator on the written .emb text: the same string
            eng.write_embeddings(i, cfg.emb_filenames[i])
            host = es.EmbeddingSpectrumEval(cfg.emb_filenames[i], cfg.train_filename, n, d).eval_embedding_spectrum()
            assert lines[2 + i] == es.format_results(mode, host), (lines[2 + i], es.format_results(mode, host))
            fields = dict(f.split("=") for f in lines[2 + i].strip().split(":")[1].split(" "))
            assert list(fields) == ["erank", "pr", "top1", "top10", "var", "mean_norm", "n", "d"]
            assert fields["n"] == str(m) and fields["d"] == str(d)
            assert 1.0 < float(fields["erank"]) <= d and 0.0 < float(fields["top1"]) < float(fields["top10"]) <= 1.0 + 1e-12
        del cfg.engine_emb_spectrum  # a user's config without the knob
        assert GraphGAN.evaluation(g) == want
    finally:
        eng.close()
    # the shipped CA-GrQc rows: printed, not gated
    ca, _, _ = load_ca_grqc()
    ids, rows = ca["emb_ids"].astype(np.int64), ca["emb_rows"].astype(np.float32)
    T = np.zeros((int(ids.max()) + 1, rows.shape[1]), dtype=np.float32)
    T[ids] = rows
    eng = ga.Engine(T, T)
    try:
        fit = eng.pca(ids)
    finally:
        eng.close()
    res = es.spectrum_metrics(fit["eigenvalues"], fit["mean64"])
    res.update(n=len(ids), d=rows.shape[1])
    print("CA-GrQc pre-trained rows: " + es.format_results("gen", res).strip())
