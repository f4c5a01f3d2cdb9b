"""Build audit of the Gram kernels (graphgan_amd/csrc/gram.hip), as tests/test_silhouette_audit_cpu.py checks the silhouette
object: the sweep keeps up to 144 accumulators per lane in registers across all tiles of a workgroup, so the build fails if an
instantiation uses scratch or spills (csrc/check_no_scratch.sh) -- checked here on the auditor itself: the remarks of the current
build pass, a copy with one spilled instantiation fails.  The audit is about scratch and spills only."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc")
CHECK = os.path.join(CSRC, "check_no_scratch.sh")
# the audits of gram.o's Makefile rule: (kernel-name regex, min count, label); 8 DT widths x {sums only, with the products} + the reducer
AUDITS = [("gram_[a-z_]*kernel", 17, "Gram kernels"), ("gram_sweep_kernelILi[0-9]ELb1E", 8, "Gram sweep instantiations with the products")]


def test_the_makefile_rule_carries_these_audits():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^AUDITED = .*\bgram\.o\b", mk, flags=re.M) and re.search(r"^OBJ = .*\bgram\.o\b", mk, flags=re.M)
    rule = mk[re.search(r"^gram\.o: AUDIT = ", mk, flags=re.M).end():].split("\npretrain.o")[0]
    for pat, count, label in AUDITS:
        assert "'%s' %d '%s'" % (pat, count, label) in rule


def test_scratch_check_accepts_the_build_and_rejects_a_spill(tmp_path):
    remarks = os.path.join(CSRC, "gram.remarks")
    if not os.path.exists(remarks):
        pytest.skip("gram.remarks is written by the build (make -C graphgan_amd/csrc)")
    args = [str(a) for audit in AUDITS for a in audit]
    ok = subprocess.run(["bash", CHECK, remarks] + args, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert ok.stdout.count("no scratch, no spill") == len(AUDITS)
    for _, _, label in AUDITS:
        assert label in ok.stdout
    text = open(remarks).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 17 and all("gram_" in x and "kernel" in x for x in names), names  # kernels only: nothing behind a call
    assert sum("gram_sweep_kernel" in x for x in names) == 16 and sum("gram_reduce_kernel" in x for x in names) == 1
    short = subprocess.run(["bash", CHECK, remarks, AUDITS[0][0], "18", AUDITS[0][2]], capture_output=True, text=True)
    assert short.returncode != 0 and "expected at least 18" in short.stderr  # a missing instantiation is noticed
    for pat, _, _ in AUDITS:  # one instantiation of every audited kernel family spilled: rejected
        m = re.search(r"(Function Name: \S*(?:%s)\S*.*?ScratchSize \[bytes/lane\]: )0" % pat, text, flags=re.S)
        assert m
        bad = text[:m.end() - 1] + "832" + text[m.end():]
        p = tmp_path / "bad.remarks"
        p.write_text(bad)
        res = subprocess.run(["bash", CHECK, str(p)] + args, capture_output=True, text=True)
        assert res.returncode != 0 and "spills" in res.stderr
