"""Build audits.  The kernels that must keep their operands in registers -- the wide all-pairs kernel
(graphgan_amd/csrc/all_score.hip, all_score_reduce_bf16_x32_kernel), the tile-stream kernels of all_score.hip and topk_score.hip,
the graph-softmax kernels -- fail the build if an instantiation uses scratch (csrc/check_no_scratch.sh) -- checked here on the
auditor itself: the remarks of the current build pass, a copy with one spilled instantiation fails.  And the product path
never touches the oracle."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc")
CHECK = os.path.join(CSRC, "check_no_scratch.sh")
# object -> the audits of its Makefile rule: (kernel-name regex, min count, label)
AUDITS = {
    "all_score": [("all_score_reduce_bf16_x32_kernel", 10, "instantiations of the wide all-pairs kernel"),
                  ("all_score_reduce_(f32|bf16)_kernel", 5, "all-pairs tile-stream kernels")],
    "topk_score": [("topk_(f32|bf16)_kernel", 5, "top-K tile-stream kernels")],
    "graph_softmax": [("gs_[a-z_]*kernel", 10, "graph-softmax kernels")],
}


@pytest.mark.parametrize("obj", sorted(AUDITS))
def test_scratch_check_accepts_the_build_and_rejects_a_spill(tmp_path, obj):
    remarks = os.path.join(CSRC, obj + ".remarks")
    if not os.path.exists(remarks):
        pytest.skip("%s.remarks is written by the build (make -C graphgan_amd/csrc)" % obj)
    args = [str(a) for audit in AUDITS[obj] for a in audit]
    ok = subprocess.run(["bash", CHECK, remarks] + args, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert ok.stdout.count("no scratch, no spill") == len(AUDITS[obj])
    for label in (a[2] for a in AUDITS[obj]):
        assert label in ok.stdout
    text = open(remarks).read()
    for pat, _, _ in AUDITS[obj]:  # one instantiation of every audited kernel family spilled: rejected
        m = re.search(r"(Function Name: \S*(?:%s)\S*.*?ScratchSize \[bytes/lane\]: )0" % pat, text, flags=re.S)
        assert m
        bad = text[:m.end() - 1] + "832" + text[m.end():]
        p = tmp_path / "bad.remarks"
        p.write_text(bad)
        res = subprocess.run(["bash", CHECK, str(p)] + args, capture_output=True, text=True)
        assert res.returncode != 0 and "spills" in res.stderr


ROOT = os.path.dirname(os.path.dirname(CSRC))
# timing switches that made the shipped kernels compute wrong results; removed from the library (profiles/r19_switch_removal_*)
REMOVED_SWITCHES = ("GG_WALK_EXPERIMENT", "GG_BFS_EXPERIMENT", "GG_BFS_PROFILE", "GG_LZ_ABLATE", "GG_K7_DBG", "GG_K7_ABLATIONS", "GG_DET_PROFILE")
SOURCE_SUFFIXES = (".py", ".hip", ".cpp", ".c", ".h", ".sh", ".md", ".txt", ".json")


def source_files(top):
    """Text sources under `top` (a file, or a directory walked recursively); build products and caches are not sources."""
    if os.path.isfile(top):
        yield top
        return
    for dirpath, dirs, files in os.walk(top):
        dirs[:] = [d for d in dirs if d != "__pycache__"]
        for f in files:
            if f.endswith(SOURCE_SUFFIXES) or f == "Makefile":
                yield os.path.join(dirpath, f)


def read(path):
    return open(path, errors="replace").read()


def test_removed_timing_switches_are_gone():
    """None of the removed switches is named in the library, its header, the tools or the README."""
    for top in ("graphgan_amd", "include", "tools", "README.md"):
        for path in source_files(os.path.join(ROOT, top)):
            text = read(path)
            hits = [name for name in REMOVED_SWITCHES if name in text]
            assert not hits, (path, hits)


def readme_env_table():
    """The rows of README's environment table ("| variable | effect |" up to the first line that is no row)."""
    lines = read(os.path.join(ROOT, "README.md")).splitlines()
    start = lines.index("| variable | effect |")
    rows = []
    for ln in lines[start:]:
        if not ln.startswith("|"):
            break
        rows.append(ln)
    return "\n".join(rows)


def test_every_library_knob_is_in_the_readme_table():
    """Every GG_... variable the library reads with getenv has its row (or row part) in README's environment table."""
    names = set()
    for path in source_files(CSRC):
        names.update(re.findall(r'getenv\(\s*"(GG_[A-Z0-9_]+)"', read(path)))
    assert len(names) > 40  # (the scan found the library's getenv calls)
    table = readme_env_table()
    documented = set(re.findall(r"`(GG_[A-Z0-9_]+)", table))
    assert not sorted(names - documented), "read by the library, missing in README's environment table"


def test_every_knob_a_test_sets_is_still_read():
    """A GG_... variable that a test puts into the environment is read somewhere -- by the library, the package, bench.py or
    the tests' own helpers: a kept knob must not leave with the removed ones (whose names only the test that proves them
    inert still sets)."""
    tests_dir = os.path.join(ROOT, "tests")
    set_by_tests = set()
    for f in sorted(os.listdir(tests_dir)):
        if not f.endswith(".py"):
            continue
        text = read(os.path.join(tests_dir, f))
        set_by_tests.update(re.findall(r'setenv\(\s*["\'](GG_[A-Z0-9_]+)["\']', text))
        set_by_tests.update(re.findall(r'\[["\'](GG_[A-Z0-9_]+)["\']\]\s*=(?!=)', text))
        set_by_tests.update(re.findall(r'["\'](GG_[A-Z0-9_]+)["\']\s*:', text))      # entries of an environment dict
        set_by_tests.update(re.findall(r'environ,[^)]*?\b(GG_[A-Z0-9_]+)\s*=', text))  # keyword of a dict(os.environ, ...)
    assert len(set_by_tests) > 20  # (the scan found the tests' settings)
    read_somewhere = set()
    reader = re.compile(r'(?:getenv\(|environ\.get\(|environ\[)\s*["\'](GG_[A-Z0-9_]+)["\']\]?(?!\s*=[^=])')
    for top in ("graphgan_amd", "bench.py", "tests"):
        for path in source_files(os.path.join(ROOT, top)):
            read_somewhere.update(reader.findall(read(path)))
    assert not sorted(set_by_tests - read_somewhere - set(REMOVED_SWITCHES)), "set by a test, read nowhere"


def test_product_path_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under graphgan_amd/ may import, load or execute it (a product path that routed
    through the CPU restatement would void every parity claim), and bench.py may name it only inside its cpu_baseline legs."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pat = re.compile(r"(from\s+oracle\b|import\s+oracle\b|oracle[/\\.]|walk_oracle|libwalk_oracle)")
    for dirpath, _, files in os.walk(os.path.join(root, "graphgan_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".sh")) or f == "Makefile":
                src = open(os.path.join(dirpath, f), errors="replace").read()
                hits = [ln for ln in src.splitlines() if pat.search(ln) and not ln.lstrip().startswith(("#", "//", "*"))]
                # comments may cite the oracle (what a kernel is checked against); code may not use it
                hits = [ln for ln in hits if "import" in ln or "CDLL" in ln or "dlopen" in ln or "open(" in ln]
                assert not hits, (os.path.join(dirpath, f), hits[:3])
    bench = open(os.path.join(root, "bench.py")).read()
    for m in re.finditer(r"^\s*from oracle import|^\s*import oracle", bench, flags=re.M):
        # every import sits inside one of the CPU-baseline functions (all three run behind the timed region)
        head = bench[:m.start()]
        fn = re.findall(r"^def (\w+)\(", head, flags=re.M)[-1]
        assert fn in ("cpu_baseline", "cpu_baseline_faithful", "cpu_baseline_threads"), fn
