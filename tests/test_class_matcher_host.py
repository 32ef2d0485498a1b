"""Runs the CPU-only test program of utils::ClassMatcherMixin, feature::Feature and feature::Extractor
(sparsebase_amd/host/tests/test_class_matcher.cc): the matcher's choices on dummy features A ... F with a fused AB and a
fused CDE, params reaching the merged class, the refusal of an unregistered feature, Subtract, the static Extract, the
slice-copy idiom, a copy that holds added features, and 24 registered singles matched promptly.  The program links
nothing of the device library."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


def test_class_matcher_program_cpu(built):
    exe = os.path.join(built, "test_class_matcher")
    out = run(exe, timeout=60)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") == 14, out
    needed = subprocess.check_output(["ldd", exe], text=True)
    assert "libsbx" not in needed and "amdhip" not in needed, needed
