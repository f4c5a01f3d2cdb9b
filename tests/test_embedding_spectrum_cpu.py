"""The host side of the embedding spectrum (graphgan_amd/evaluation/embedding_spectrum.py): the metrics on known spectra, the
two-pass float64 PCA against numpy.cov on the shipped CA-GrQc rows, the results line, the ``engine_emb_spectrum`` knob of
``GraphGAN.evaluation`` without an engine, the presence of gg_gram in header, binding and library, and the command line's host leg."""
import math
import os
import re

import numpy as np
import pytest

from tests.helpers import load_ca_grqc


@pytest.fixture(scope="module")
def es():
    from graphgan_amd.evaluation import embedding_spectrum
    return embedding_spectrum


def test_metrics_on_known_spectra(es):
    for d in (1, 2, 7, 50):
        r = es.spectrum_metrics(np.full(d, 0.3), np.zeros(d))
        assert abs(r["erank"] - d) <= 1e-12 * d and abs(r["pr"] - d) <= 1e-12 * d
        assert r["top1"] == pytest.approx(1.0 / d, rel=1e-15) and r["top10"] == pytest.approx(min(10, d) / d, rel=1e-14)
        assert r["var"] == pytest.approx(0.3 * d, rel=1e-15) and r["mean_norm"] == 0.0
    r = es.spectrum_metrics([0.0, 2.5, 0.0], [3.0, 4.0, 0.0])
    assert (r["erank"], r["pr"], r["top1"], r["top10"], r["var"], r["mean_norm"]) == (1.0, 1.0, 1.0, 1.0, 2.5, 5.0)
    r = es.spectrum_metrics(np.zeros(4), [1.0, 0.0, 0.0, 0.0])
    assert all(math.isnan(r[k]) for k in ("erank", "pr", "top1", "top10")) and r["var"] == 0.0 and r["mean_norm"] == 1.0
    # any order in, negatives (eigh's rounding of a zero eigenvalue) clipped; 12 eigenvalues: top10 leaves the two smallest out
    lam = np.array([1.0, 12.0, 3.0, 2.0, 11.0, 4.0, 10.0, 5.0, 9.0, 6.0, 8.0, 7.0, -1e-17])
    r = es.spectrum_metrics(lam, np.zeros(13))
    p = np.sort(lam[:12])[::-1] / 78.0
    assert r["top1"] == 12.0 / 78.0 and r["top10"] == pytest.approx(75.0 / 78.0, rel=1e-15) and r["var"] == 78.0
    assert r["erank"] == pytest.approx(float(np.exp(-(p * np.log(p)).sum())), rel=1e-14) and r["pr"] == pytest.approx(78.0 ** 2 / 650.0, rel=1e-15)


def test_host_pca_against_numpy_cov_on_ca_grqc(es):
    ca, _, _ = load_ca_grqc()
    ids, rows = ca["emb_ids"].astype(np.int64), ca["emb_rows"].astype(np.float64)
    X = np.zeros((int(ids.max()) + 1, rows.shape[1]))
    X[ids] = rows
    fit = es.host_pca(X, ids)
    want = np.cov(rows, rowvar=False, bias=True)
    assert np.abs(fit["cov"] - want).max() <= 1e-10 * np.abs(want).max()
    lam = np.sort(np.linalg.eigvalsh(want))[::-1]
    assert np.abs(fit["eigenvalues"] - lam).max() <= 1e-10 * lam[0]
    assert fit["m"] == len(ids) and fit["mean"].dtype == np.float32 and np.array_equal(fit["mean"], rows.mean(axis=0).astype(np.float32))
    assert np.allclose(fit["mean64"], rows.mean(axis=0), rtol=1e-13)
    V = fit["components"].astype(np.float64)
    assert V.shape == (50, 50) and np.abs(V @ V.T - np.eye(50)).max() < 1e-5  # orthonormal rows
    assert np.abs(V @ want @ V.T - np.diag(fit["eigenvalues"])).max() <= 1e-5 * lam[0]  # ... that diagonalise the covariance
    lead = np.argmax(np.abs(V), axis=1)
    assert (V[np.arange(50), lead] > 0).all()  # the sign convention
    assert np.array_equal(es.host_pca(X, ids, n_components=3)["components"], fit["components"][:3])
    res = es.spectrum_metrics(fit["eigenvalues"], fit["mean64"])
    print("CA-GrQc pre-trained rows: " + es.format_results("gen", dict(res, n=len(ids), d=50)).strip())
    assert 1.0 < res["pr"] <= res["erank"] <= 50.0  # (the participation ratio never exceeds the effective rank)
    with pytest.raises(ValueError, match="m >= 2"):
        es.host_pca(X, ids[:1])


def test_sign_convention_on_ties(es):
    lam, vec = es.pca_eig(np.diag([1.0, 3.0, 2.0]))
    assert lam.tolist() == [3.0, 2.0, 1.0] and np.array_equal(np.abs(vec), np.eye(3)[[1, 2, 0]]) and (vec.sum(axis=1) == 1.0).all()
    # the eigenvector (1, -1) / sqrt(2) has two entries of the largest magnitude: the lower index is made positive
    lam, vec = es.pca_eig(np.array([[2.0, -1.0], [-1.0, 2.0]]))
    assert lam.tolist() == [3.0, 1.0] and vec[0, 0] > 0 > vec[0, 1] and vec[1, 0] > 0 and vec[1, 1] > 0
    assert es.pca_eig(np.diag([1.0, -1e-18]))[0].tolist() == [1.0, 0.0]  # clipped at 0


def test_format_results(es):
    res = dict(erank=41.5, pr=32.25, top1=0.125, top10=0.5, var=12.9, mean_norm=2.66, n=5119, d=50)
    assert es.format_results("gen", res) == "gen_spec:erank=41.5 pr=32.25 top1=0.125 top10=0.5 var=12.9 mean_norm=2.66 n=5119 d=50\n"
    res.update(erank=float("nan"), pr=float("nan"), top1=float("nan"), top10=float("nan"), var=0.0)
    assert es.format_results("dis", res) == "dis_spec:erank=nan pr=nan top1=nan top10=nan var=0.0 mean_norm=2.66 n=5119 d=50\n"


# ---- graph_gan.evaluation()
def _layout(tmp_path, app="link_prediction"):
    from tests.test_link_prediction_lr_cpu import _layout as layout
    return layout(tmp_path, app)


def test_evaluation_lines_with_and_without_the_knob(es, tmp_path):
    from graphgan_amd import config, utils
    from graphgan_amd.evaluation import link_prediction as lp
    from graphgan_amd.graph_gan import GraphGAN
    assert config.engine_emb_spectrum is False
    cfg, g, n = _layout(tmp_path)
    assert cfg.engine_emb_spectrum is False
    # the list as the code before the knob builds it: the two link-prediction lines and nothing else
    want = ["%s:%s\n" % (m, str(lp.LinkPredictEval(cfg.emb_filenames[i], cfg.test_filename, cfg.test_neg_filename, n, cfg.n_emb).eval_link_prediction()))
            for i, m in enumerate(cfg.modes)]
    assert GraphGAN.evaluation(g) == want  # the knob's default: off
    del cfg.engine_emb_spectrum
    assert GraphGAN.evaluation(g) == want  # a user's config without the knob
    cfg.engine_emb_spectrum = True
    lines = GraphGAN.evaluation(g)
    assert lines[:2] == want and [ln.split(":")[0] for ln in lines[2:]] == ["gen_spec", "dis_spec"]
    assert open(cfg.result_filename).read() == "".join(want + want + lines)
    trained = es.trained_nodes(cfg.train_filename)
    deg = np.bincount(np.array(utils.read_edges_from_file(cfg.train_filename)).reshape(-1), minlength=n)
    assert np.array_equal(trained, np.flatnonzero(deg > 0)) and 2 <= len(trained) < n  # some nodes occur in the test file alone
    for i, (mode, line) in enumerate(zip(cfg.modes, lines[2:])):
        emd = utils.read_embeddings(cfg.emb_filenames[i], n_node=n, n_embed=cfg.n_emb)
        fit = es.host_pca(emd, trained)
        res = dict(es.spectrum_metrics(fit["eigenvalues"], fit["mean64"]), n=len(trained), d=cfg.n_emb)
        assert line == es.format_results(mode, res)
        assert re.fullmatch(r"%s_spec:erank=\S+ pr=\S+ top1=\S+ top10=\S+ var=\S+ mean_norm=\S+ n=%d d=%d\n" % (mode, len(trained), cfg.n_emb), line)
    # the discriminator's file holds the generator's rows doubled: the shape of the spectrum is the same, the scale is not
    f = [dict(kv.split("=") for kv in ln.strip().split(":")[1].split(" ")) for ln in lines[2:]]
    assert float(f[1]["erank"]) == pytest.approx(float(f[0]["erank"]), rel=1e-9) and float(f[1]["var"]) == pytest.approx(4 * float(f[0]["var"]), rel=1e-9)
    assert float(f[1]["mean_norm"]) == pytest.approx(2 * float(f[0]["mean_norm"]), rel=1e-12)


def test_evaluation_with_the_knob_needs_two_trained_nodes(tmp_path):
    from graphgan_amd.graph_gan import GraphGAN
    cfg, g, _ = _layout(tmp_path)
    cfg.engine_emb_spectrum = True
    with open(cfg.train_filename, "w") as f:
        f.write("3\t3\n")  # one node with a training edge
    with pytest.raises(ValueError, match="engine_emb_spectrum needs at least two nodes with a training edge: .* has 1"):
        GraphGAN.evaluation(g)
    assert not os.path.exists(cfg.result_filename)  # refused before anything is computed
    os.remove(cfg.train_filename)
    with pytest.raises(ValueError, match="engine_emb_spectrum needs the training edges.*train_filename"):
        GraphGAN.evaluation(g)


def test_gg_gram_in_header_binding_and_library():
    from graphgan_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^int gg_gram\(gg_ctx \*ctx, int which, const int32_t \*nodes, int64_t m, const float \*center", header, flags=re.M)
    assert "gg_gram" in _lib.SIGNATURES and len(_lib.SIGNATURES["gg_gram"][1]) == 8
    assert _lib.lib.gg_gram.argtypes == _lib.SIGNATURES["gg_gram"][1]  # the built library exports it
    assert _lib.header_abi_version() == 9 == _lib.ABI_VERSION == _lib.lib.gg_abi_version()
    assert _lib.GRAM_MAX_GRID == 512
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "gram.hip")).read()
    assert re.search(r"constexpr int GRAM_MAX_GRID = %d;" % _lib.GRAM_MAX_GRID, src)


# ---- python -m graphgan_amd.project --host
def test_cli_host_projection_of_six_nodes(tmp_path):
    from graphgan_amd import project
    # ids 0 .. 5; nodes 0 .. 3 carry training edges and form the square (+-2, +-1) about (10, 20): mean (10, 20) exactly,
    # cov = diag(4, 1), components e_1, e_2 (signed positive); nodes 4 and 5 are projected, not fitted
    rows = {0: (12.0, 21.0), 1: (8.0, 21.0), 2: (12.0, 19.0), 3: (8.0, 19.0), 4: (10.5, 20.0), 5: (13.0, 27.5)}
    emb, train, out = tmp_path / "x.emb", tmp_path / "train.txt", tmp_path / "coords.tsv"
    emb.write_text("6\t2\n" + "".join("%d\t%r\t%r\n" % (i, rows[i][0], rows[i][1]) for i in (3, 0, 5, 1, 4, 2)))
    train.write_text("0\t1\n1\t2\n2\t3\n")
    assert project.main(["--emb", str(emb), "--out", str(out), "--train", str(train), "--host"]) == 0
    assert out.read_text() == "".join("%d\t%r\t%r\n" % (i, rows[i][0] - 10.0, rows[i][1] - 20.0) for i in range(6))
    assert project.main(["--emb", str(emb), "--out", str(out), "--train", str(train), "--host", "--dim", "1"]) == 0
    assert out.read_text() == "".join("%d\t%r\n" % (i, rows[i][0] - 10.0) for i in range(6))
    # without --train all six rows are fitted: the projection is centred on their mean
    assert project.main(["--emb", str(emb), "--out", str(out), "--host"]) == 0
    got = np.array([[float(v) for v in ln.split("\t")[1:]] for ln in out.read_text().splitlines()])
    assert got.shape == (6, 2) and np.abs(got.mean(axis=0)).max() < 1e-6 and got[:, 0].var() >= got[:, 1].var()
    for bad in (["--dim", "0"], ["--dim", "3"]):
        with pytest.raises(SystemExit):
            project.main(["--emb", str(emb), "--out", str(out), "--host"] + bad)
