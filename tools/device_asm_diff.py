#!/usr/bin/env python3
"""Per-kernel comparison of device assembly files whose symbol order may differ: tools/device_asm_diff.py A.s B.s [A2.s B2.s ...]

For a host-only change of a .hip file: compile the file before and after with the build's flags (sparsebase_amd/build.py)
plus `--cuda-device-only -S`, and every kernel must come out the same.  Labels numbered by a function's index in the file
(.LBB<i>_<j>, .Lfunc_end<i>, ...) and the per-compile __hip_cuid hash are normalised; everything else — each kernel's
code and descriptor, the file's header and trailer, each kernel's metadata entry — must match byte for byte.
Exit status 1 if anything differs."""
import re
import sys


def norm(t):
    t = re.sub(r'\.L(BB|func_end|func_begin|tmp|JTI|CPI)(\d+)', r'.L\1N', t)
    return re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', t)


def pieces(path):
    head, _, meta = norm(open(path).read()).partition('\t.amdgpu_metadata')
    parts = re.split(r'(?m)^(?=\t\.section\t\.text\.)', head)
    d = {'<header>': parts[0]}
    for p in parts[1:]:
        name = re.match(r'\t\.section\t\.text\.([^,]+),', p).group(1)
        body, sep, tail = p.partition('\t.section\t.AMDGPU.gpr_maximums')
        d[name] = body
        if sep:
            d['<trailer>'] = tail
    # (the metadata's own trailer goes with no kernel: the entries may come in another order)
    meta, sep, tail = meta.partition('amdhsa.target:')
    return d, sorted(re.split(r'(?m)^(?=  - \.(?:agpr_count|args):)', meta)) + [sep + tail]


bad = 0
for a_path, b_path in zip(sys.argv[1::2], sys.argv[2::2]):
    (a, am), (b, bm) = pieces(a_path), pieces(b_path)
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print('%s vs %s: %d / %d kernels, differing: %s; metadata entries %d / %d, same: %s' % (
        a_path, b_path, len(a) - 2, len(b) - 2, ', '.join(diff) or 'none', len(am), len(bm), am == bm))
    bad += len(diff) + (am != bm)
sys.exit(1 if bad else 0)
