"""CPU unit test of the exact binary -> decimal conversion used by the device text writers
(sparsebase_amd/csrc/sbx_bin2dec.h compiled for the host) against snprintf("%.*g"): float and double, every precision
1..17 for every input, no input skipped; where the 128-bit fast path applies it is also compared with the multi-limb
path."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bin2dec_matches_printf_g(tmp_path):
    exe = str(tmp_path / "bin2dec_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "sparsebase_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "bin2dec_check.cc"), "-o", exe], check=True)
    for seed in (1, 2):
        p = subprocess.run([exe, "400000", str(seed)], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0 and p.stdout.startswith("ok"), p.stdout[-2000:]
        doubles, floats = (int(x) for x in p.stdout.split()[1:3])
        assert doubles >= 400000 and floats >= 400000
