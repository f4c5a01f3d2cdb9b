"""The checkpoint file (gg_save_state / gg_load_state, gg_api.hip: state_io) beyond tests/test_gpu_steps.py's
test_state_save_restore: a resumed run equals an uninterrupted one BIT FOR BIT (the step count, both beta powers and all four
moment tables of both models: allclose behind one step does not see them), every refused file leaves all four tables as they
were, a dense-Adam file loads into a lazy-Adam engine as the code says, and a checkpoint whose generator holds a NaN loads, is
reported by the next walk launch as an error, and is forgotten with the next finite checkpoint.

Loading a checkpoint into an engine whose walk caches are warm is a column of tests/test_gpu_generator_changes.py."""
import struct

import numpy as np
import pytest

from oracle import graphgan_oracle as orc
from tests.support import generator_change_cases as gc

pytestmark = pytest.mark.gpu

N = 100
HEADER = struct.Struct("<4s5i")   # magic, version, n_node, n_emb, ld, optimizer (gg_api.hip: StateHeader)


@pytest.fixture(scope="module")
def ga():
    import graphgan_amd
    return graphgan_amd


def opt_of(ga, name):
    return {"dense": ga.GG_OPT_ADAM_DENSE, "lazy": ga.GG_OPT_ADAM_LAZY, "sgd": ga.GG_OPT_SGD}[name]


def models(n, d, seed=1):
    rs = np.random.RandomState(seed)
    return ((rs.randn(n, d) * 0.5).astype(np.float32), (rs.randn(n, d) * 0.5).astype(np.float32),
            (rs.randn(n) * 0.1).astype(np.float32), (rs.randn(n) * 0.1).astype(np.float32))


def engine(ga, tabs, opt, zero=False, **kw):
    Eg, Ed, bg, bd = [t * np.float32(0) for t in tabs] if zero else tabs
    eng = ga.Engine(Eg, Ed, optimizer=opt_of(ga, opt), lr_gen=0.01, lr_dis=0.01, **kw)
    eng.set_bias(0, bg)
    eng.set_bias(1, bd)
    return eng


def batches(n, count, seed):
    """`count` batches of 64 pairs with repeated rows (half of a batch shares its first node), labels and rewards."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        u, v = rs.randint(0, n, 64), rs.randint(0, n, 64)
        u[:32] = u[0]
        out.append((u, v, (rs.rand(64) < 0.5).astype(np.float32), (rs.rand(64) * 2).astype(np.float32)))
    return out


def steps(eng, bs):
    for u, v, lab, rew in bs:
        eng.d_step(u, v, lab)
        eng.g_step(u, v, rew)


def tables(eng):
    return [eng.get_embeddings(0), eng.get_embeddings(1), eng.get_bias(0), eng.get_bias(1)]


def same_bits(got, want, what):
    for name, a, b in zip(("gen E", "dis E", "gen b", "dis b"), got, want):
        bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
        assert len(bad) == 0, "%s: %s differs in %d of %d words, first at %d" % (what, name, len(bad), a.size, bad[0])


@pytest.mark.parametrize("d", [50, 6])
@pytest.mark.parametrize("opt", ["dense", "lazy", "sgd"])
def test_resume_equals_no_interruption(ga, opt, d, monkeypatch, tmp_path):
    """3 D and 3 G steps, save, 3 more of each; a second engine created with ZERO tables loads the file and runs the same 3 + 3:
    all four tables equal as uint32 views.  GG_DETERMINISTIC=1 and batches of 64: the atomic-free kernel, so the uninterrupted
    run is reproducible at all.  d = 50 and d = 6: the rows are padded (ld != d) and the file stores the padded rows."""
    monkeypatch.setenv("GG_DETERMINISTIC", "1")
    tabs = models(N, d)
    first, second = batches(N, 3, 10), batches(N, 3, 11)
    eng = engine(ga, tabs, opt)
    steps(eng, first)
    path = str(tmp_path / "resume.ggst")
    eng.save_state(path)
    at_save = tables(eng)
    steps(eng, second)
    want = tables(eng)
    eng.close()
    assert not np.array_equal(at_save[0], want[0]) and not np.array_equal(at_save[1], want[1])
    res = engine(ga, tabs, opt, zero=True)
    res.load_state(path)
    same_bits(tables(res), at_save, "%s d=%d: the loaded tables" % (opt, d))
    steps(res, second)
    same_bits(tables(res), want, "%s d=%d: 3 + 3 steps behind the load" % (opt, d))
    res.close()


def patched(blob, **fields):
    names = ("magic", "version", "n_node", "n_emb", "ld", "optimizer")
    h = dict(zip(names, HEADER.unpack_from(blob)))
    h.update(fields)
    return HEADER.pack(*[h[k] for k in names]) + blob[HEADER.size:]


def test_refused_files_change_nothing(ga, monkeypatch, tmp_path):
    """An SGD file into an Adam engine and the reverse, a file of another n_node and of another n_emb: GG_EINVAL; a wrong magic,
    one trailing byte: GG_EIO (the latter with "nothing was loaded").  Behind every refusal all four tables hold the bits they
    held before the call, and the engine still steps like one that never saw the file."""
    monkeypatch.setenv("GG_DETERMINISTIC", "1")
    d = 50
    tabs = models(N, d)
    bs = batches(N, 2, 12)
    files = {}
    for name, n, dd, opt in (("adam", N, d, "lazy"), ("sgd", N, d, "sgd"), ("n101", N + 1, d, "lazy"), ("d6", N, 6, "lazy")):
        e = engine(ga, models(n, dd, seed=5), opt)
        steps(e, batches(n, 1, 13))
        files[name] = str(tmp_path / (name + ".ggst"))
        e.save_state(files[name])
        e.close()
    blob = open(files["adam"], "rb").read()
    assert HEADER.unpack_from(blob)[:4] == (b"GGST", 1, N, d)
    files["magic"] = str(tmp_path / "magic.ggst")
    open(files["magic"], "wb").write(patched(blob, magic=b"GGSX"))
    files["trailing"] = str(tmp_path / "trailing.ggst")
    open(files["trailing"], "wb").write(blob + b"\0")
    sgd_blob = open(files["sgd"], "rb").read()
    files["sgd_trailing"] = str(tmp_path / "sgd_trailing.ggst")
    open(files["sgd_trailing"], "wb").write(sgd_blob + b"\0")

    def refused(eng, name, code, text=None):
        before = tables(eng)
        with pytest.raises(ga.GraphGANHipError) as ei:
            eng.load_state(files[name])
        assert ei.value.code == code, (name, ei.value.code, str(ei.value))
        assert text is None or text in str(ei.value), (name, str(ei.value))
        same_bits(tables(eng), before, "refused file %s" % name)

    for opt, other, trailing in (("lazy", "sgd", "trailing"), ("dense", "sgd", "trailing"), ("sgd", "adam", "sgd_trailing")):
        eng = engine(ga, tabs, opt)
        clean = engine(ga, tabs, opt)
        steps(eng, bs[:1])
        steps(clean, bs[:1])
        refused(eng, other, ga.GG_EINVAL)
        refused(eng, "n101", ga.GG_EINVAL)
        refused(eng, "d6", ga.GG_EINVAL)
        refused(eng, "magic", ga.GG_EIO)
        refused(eng, trailing, ga.GG_EIO, "nothing was loaded")
        steps(eng, bs[1:])
        steps(clean, bs[1:])
        same_bits(tables(eng), tables(clean), "%s engine: a step behind the refusals (step count, beta powers, moments untouched)" % opt)
        eng.close()
        clean.close()


def test_dense_adam_file_into_a_lazy_adam_engine(ga, monkeypatch, tmp_path):
    """state_io compares only "SGD or not": a dense-Adam file is accepted by a lazy-Adam engine.  The next steps equal those of a
    lazy engine that holds the same state -- one that loaded the same bytes under a lazy-Adam header."""
    monkeypatch.setenv("GG_DETERMINISTIC", "1")
    d = 50
    tabs = models(N, d)
    dense = engine(ga, tabs, "dense")
    steps(dense, batches(N, 3, 20))
    path = str(tmp_path / "dense.ggst")
    dense.save_state(path)
    saved = tables(dense)
    dense.close()
    blob = open(path, "rb").read()
    assert HEADER.unpack_from(blob)[5] == ga.GG_OPT_ADAM_DENSE
    as_lazy = str(tmp_path / "as_lazy.ggst")
    open(as_lazy, "wb").write(patched(blob, optimizer=ga.GG_OPT_ADAM_LAZY))
    a, b = engine(ga, tabs, "lazy", zero=True), engine(ga, tabs, "lazy", zero=True)
    a.load_state(path)
    b.load_state(as_lazy)
    same_bits(tables(a), saved, "dense file in a lazy engine: the loaded tables")
    more = batches(N, 3, 21)
    steps(a, more)
    steps(b, more)
    same_bits(tables(a), tables(b), "dense file in a lazy engine: 3 + 3 steps behind the load")
    assert not np.array_equal(tables(a)[0], saved[0])
    a.close()
    b.close()


@pytest.mark.parametrize("levels", ["0", "64"])
def test_checkpoint_with_a_nan_in_the_generator(ga, levels, monkeypatch, tmp_path):
    """It loads; the next walk_sample returns GG_EINVAL ("non-finite": an error code, nothing faults), in the per-walk kernel and
    in the level pipeline; a following load of a finite file clears the flag, and the walks equal the oracle's."""
    monkeypatch.setenv("GG_WALK_LEVELS", levels)
    g = gc.graph("small3")
    A = gc.bias_pair(g)[0]
    n, roots = g["n"], g["roots"]
    bad = A["E"].copy()
    bad[7, 2] = np.nan
    paths = {}
    for name, E in (("nan", bad), ("finite", A["E"])):
        e = ga.Engine(E, A["E"])
        e.set_bias(0, A["b"])
        paths[name] = str(tmp_path / (name + ".ggst"))
        e.save_state(paths[name])
        e.close()
    eng = ga.Engine(A["E"] * np.float32(0.5), A["E"])
    eng.set_graph_csr(g["rowptr"], g["col"])
    eng.build_trees(roots, device=True)
    nw = np.full(n, 5, np.int32)
    eng.walk_sample(roots, nw, False, 3, 1)      # (a launch on other, finite tables first: the caches are warm)
    eng.load_state(paths["nan"])
    assert np.isnan(eng.get_embeddings(0)[7, 2])
    with pytest.raises(ga.GraphGANHipError) as ei:
        eng.walk_sample(roots, nw, False, 3, 1)
    assert ei.value.code == ga.GG_EINVAL and "non-finite" in str(ei.value)
    eng.load_state(paths["finite"])
    got = eng.walk_sample(roots, nw, False, 3, 1)
    off, nbr, base, dmax = orc.c_build_trees(n, g["rowptr"], g["col"], roots)
    want = orc.c_walk_sample(orc.pad_rows(A["E"]), A["b"], off, nbr.copy(), base, roots, roots, nw, False, 3, 1, got["paths"].shape[1])
    for k in ("samples", "path_len", "root_status"):
        assert np.array_equal(got[k], want[k]), k
    m = np.arange(got["paths"].shape[1])[None, :] < want["path_len"][:, None]
    assert np.array_equal(got["paths"][m], want["paths"][m])
    eng.close()
