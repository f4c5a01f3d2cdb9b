"""Build audit of the silhouette kernels (graphgan_amd/csrc/silhouette.hip), as tests/test_build_audit_cpu.py checks the other
tile-stream objects: the consumer's running sums and the producers' fragments must stay in registers, so the build fails if an
instantiation uses scratch (csrc/check_no_scratch.sh) -- checked here on the auditor itself: the remarks of the current build
pass, a copy with one spilled instantiation fails."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc")
CHECK = os.path.join(CSRC, "check_no_scratch.sh")
# the audits of silhouette.o's Makefile rule: (kernel-name regex, min count, label)
AUDITS = [("sil_(f32|bf16)_kernel", 5, "silhouette tile-stream kernels"), ("sil_[a-z0-9_]*kernel", 10, "silhouette kernels")]


def test_the_makefile_rule_carries_these_audits():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^AUDITED = .*\bsilhouette\.o\b", mk, flags=re.M)
    rule = mk[re.search(r"^silhouette\.o: AUDIT = ", mk, flags=re.M).end():].split("\ngraph_softmax.o")[0]
    for pat, count, label in AUDITS:
        assert "'%s' %d '%s'" % (pat, count, label) in rule


def test_scratch_check_accepts_the_build_and_rejects_a_spill(tmp_path):
    remarks = os.path.join(CSRC, "silhouette.remarks")
    if not os.path.exists(remarks):
        pytest.skip("silhouette.remarks is written by the build (make -C graphgan_amd/csrc)")
    args = [str(a) for audit in AUDITS for a in audit]
    ok = subprocess.run(["bash", CHECK, remarks] + args, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert ok.stdout.count("no scratch, no spill") == len(AUDITS)
    for _, _, label in AUDITS:
        assert label in ok.stdout
    text = open(remarks).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 10 and all("sil_" in x and "kernel" in x for x in names), names  # kernels only: nothing behind a call
    for pat, _, _ in AUDITS:  # one instantiation of every audited kernel family spilled: rejected
        m = re.search(r"(Function Name: \S*(?:%s)\S*.*?ScratchSize \[bytes/lane\]: )0" % pat, text, flags=re.S)
        assert m
        bad = text[:m.end() - 1] + "832" + text[m.end():]
        p = tmp_path / "bad.remarks"
        p.write_text(bad)
        res = subprocess.run(["bash", CHECK, str(p)] + args, capture_output=True, text=True)
        assert res.returncode != 0 and "spills" in res.stderr
