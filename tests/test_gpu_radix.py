"""The library's radix sort itself (internal entry points, reached through their mangled names): every record shape,
counts around the tile sizes of the persistent pass kernel, 1 ... 8 digit passes, against torch's stable sort; and the
ping-pong front sbx_sort_pairs, which plans the passes itself and hands the buffers back sorted-first."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class Pass(C.Structure):
    _fields_ = [("shift", C.c_int), ("bits", C.c_int)]


@pytest.fixture(scope="module")
def internal():
    from sparsebase_amd import capi, ops
    hd = ops.handle_for(torch.device("cuda", 0))
    names = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout

    def sym(stem):
        m = re.search(r"\b(_Z\d+%s\w*)" % stem, names)
        assert m, f"{stem} is not exported by {capi.LIB_PATH}"
        f = getattr(hd.lib, m.group(1))
        f.restype = C.c_int
        return f

    return hd, sym


@pytest.fixture(scope="module")
def rs(internal):
    hd, sym = internal
    return hd, sym("sbx_radix_sortP"), sym("sbx_radix_plan"), sym("sbx_arena_begin")


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


@pytest.mark.parametrize("kbytes,pbytes", [(4, 0), (4, 4), (4, 8), (8, 0), (8, 4), (8, 8)])
def test_radix_sort_record_shapes_and_tile_edges(rs, kbytes, pbytes):
    hd, sort, plan, arena_begin = rs
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1000 * kbytes + pbytes)
    tile = 512 * (4 if (kbytes, pbytes) == (8, 8) else 8)
    counts = [2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1, 3 * tile, 100_003, 1_500_000]
    # (low bits, high bits): 1 pass ... 8 passes; narrow ranges give long runs of equal keys (stability)
    ranges = [(3, 0), (8, 0), (9, 0), (20, 0), (31, 0)] if kbytes == 4 else [(1, 1), (7, 9), (20, 20), (31, 31), (32, 32)]
    for count in counts:
        for lo_bits, hi_bits in ranges:
            keys = torch.randint(0, 1 << lo_bits, (count,), device=dev, dtype=torch.int64, generator=g)
            if kbytes == 8:
                keys = keys | (torch.randint(0, 1 << hi_bits, (count,), device=dev, dtype=torch.int64, generator=g) << 32)
            else:
                keys = keys.to(torch.int32)
            pay = None
            if pbytes:
                pay = torch.arange(count, device=dev, dtype=torch.int64 if pbytes == 8 else torch.int32) * 3 + 1
            passes = (Pass * 16)()
            n_passes = plan(0, lo_bits, 32, 32 + hi_bits, passes)
            assert 1 <= n_passes <= 8
            ka, kb = keys.clone(), torch.zeros_like(keys)
            pa = pay.clone() if pbytes else None
            pb = torch.zeros_like(pay) if pbytes else None
            in_b = C.c_int(0)
            hd.bind_stream()
            hd.check(arena_begin(hd.h))
            hd.check(sort(hd.h, kbytes, pbytes, ptr(ka), ptr(kb), ptr(pa), ptr(pb), C.c_int64(count), passes, n_passes,
                          C.byref(in_b)))
            torch.cuda.synchronize()
            # unsigned order == signed order here: the keys are non-negative except (32, 32), compared as unsigned
            ref_keys = keys if not (kbytes == 8 and hi_bits == 32) else keys ^ (1 << 63)
            order = torch.sort(ref_keys, stable=True)[1]
            got_k = kb if in_b.value else ka
            assert torch.equal(got_k, keys[order]), (count, lo_bits, hi_bits)
            if pbytes:
                got_p = pb if in_b.value else pa
                assert torch.equal(got_p, pay[order]), (count, lo_bits, hi_bits)


@pytest.mark.parametrize("kbytes,pbytes", [(4, 4), (8, 0), (8, 4)])
def test_sort_pairs_hands_back_the_sorted_buffers_first(internal, rs, kbytes, pbytes):
    """sbx_sort_pairs over 0 ... 3 passes (the result lands on either side of the ping-pong) and the counts at which a
    wrong swap or a missed early return shows: *a holds the stably sorted records, {*a, *b} are the caller's two
    buffers, and with count < 2 or no bit to sort by neither the pointers nor the contents change."""
    hd, sym = internal
    _, _, plan, arena_begin = rs
    sort_pairs = sym("sbx_sort_pairsP")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(77 * kbytes + pbytes)
    tile = 512 * 8
    kdt = torch.int32 if kbytes == 4 else torch.int64
    # (lo0, hi0, lo1, hi1) -> 0, 1, 2, 3 passes; 8-byte keys also with the second range in the high word
    ranges = [(0, 0, 0, 0), (0, 8, 0, 0), (0, 16, 0, 0), (0, 24, 0, 0)]
    if kbytes == 8:
        ranges += [(0, 0, 32, 32), (0, 0, 32, 40), (0, 8, 32, 40), (0, 16, 32, 40)]
    seen_passes, seen_sides = set(), set()
    for count in [0, 1, 2, 63, 64, 65, tile + 1]:
        # (one element more than `count`: a guard the sort must leave alone, and no empty tensor for count 0)
        keys = torch.randint(0, 1 << 24, (count + 1,), device=dev, dtype=torch.int64, generator=g)
        if kbytes == 8:
            keys = keys | (torch.randint(0, 1 << 8, (count + 1,), device=dev, dtype=torch.int64, generator=g) << 32)
        keys = keys.to(kdt)
        pay = torch.arange(count + 1, device=dev, dtype=torch.int32) * 3 + 1 if pbytes else None
        for lo0, hi0, lo1, hi1 in ranges:
            n_passes = plan(lo0, hi0, lo1, hi1, (Pass * 16)())
            seen_passes.add(n_passes)
            ka, kb = keys.clone(), torch.full_like(keys, -7)
            pa = pay.clone() if pbytes else None
            pb = torch.full_like(pay, -7) if pbytes else None
            a, b = C.c_void_p(ka.data_ptr()), C.c_void_p(kb.data_ptr())
            va, vb = (C.c_void_p(pa.data_ptr()), C.c_void_p(pb.data_ptr())) if pbytes else (None, None)
            hd.bind_stream()
            hd.check(arena_begin(hd.h))
            hd.check(sort_pairs(hd.h, kbytes, pbytes, C.byref(a), C.byref(b), C.byref(va) if pbytes else None,
                                C.byref(vb) if pbytes else None, C.c_int64(count), lo0, hi0, lo1, hi1))
            torch.cuda.synchronize()
            case = (count, lo0, hi0, lo1, hi1)
            assert {a.value, b.value} == {ka.data_ptr(), kb.data_ptr()} and a.value != b.value, case
            if pbytes:
                assert {va.value, vb.value} == {pa.data_ptr(), pb.data_ptr()} and va.value != vb.value, case
                assert (va.value == pa.data_ptr()) == (a.value == ka.data_ptr()), case  # keys and payloads swap together
            if count < 2 or n_passes == 0:
                assert a.value == ka.data_ptr(), case
                assert torch.equal(ka, keys) and bool((kb == -7).all()), case
                if pbytes:
                    assert torch.equal(pa, pay) and bool((pb == -7).all()), case
                continue
            mask = (((1 << hi0) - 1) ^ ((1 << lo0) - 1)) | (((1 << hi1) - 1) ^ ((1 << lo1) - 1))
            order = torch.sort(keys[:count].to(torch.int64) & mask, stable=True)[1]
            got_k = ka if a.value == ka.data_ptr() else kb
            seen_sides.add(a.value == ka.data_ptr())
            assert torch.equal(got_k[:count], keys[:count][order]), case
            assert int(ka[count]) == int(keys[count]) and int(kb[count]) == -7, case
            if pbytes:
                got_p = pa if va.value == pa.data_ptr() else pb
                assert torch.equal(got_p[:count], pay[:count][order]), case
                assert int(pa[count]) == int(pay[count]) and int(pb[count]) == -7, case
    assert seen_passes == {0, 1, 2, 3} and seen_sides == {True, False}
