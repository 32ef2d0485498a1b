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


class Emit(C.Structure):  # struct sbx_radix_emit (sbx_internal.h)
    _fields_ = [("map", C.c_void_p), ("out", C.c_void_p), ("bits_a", C.c_void_p), ("bits_b", C.c_void_p),
                ("pos_of", C.c_void_p), ("low_mask", C.c_uint32)]


@pytest.mark.parametrize("form", ["split", "packed"])
def test_radix_sort_emit_writes_values_bits_and_positions(internal, rs, form):
    """sbx_radix_sort_emit: the sort of 64-bit keys whose last digit pass stores no keys but, per key at sorted position
    p, out[p] = value (the key's low word under low_mask, through `map` when there is one), the value's bit in up to two
    bitmaps and pos_of[value] = p — how the RCM's radix routes write a level (the queue, the visited and frontier
    bitmaps, the level positions).  Both key forms of sbx_rcm.hip: 'split' — a value in the low word and a parent
    position from bit 32 on, of which only the latter is sorted (low_mask = 0); 'packed' — parent << low_bits | value,
    sorted whole (low_mask = 2^low_bits - 1).  1 ... 8 digit passes, counts around the tile (4096 keys), every output
    absent in some cases; values are distinct within a call, as vertex ids are (pos_of[value] is otherwise a race) and
    `map` is a permutation, as the rank order is.  The bitmaps are ORed into (their random prefill must survive),
    pos_of keeps its prefill where no value points, out[count] is not touched.  Against torch's stable sort of the
    sorted bits and plain indexing."""
    hd, sym = internal
    _, _, plan, arena_begin = rs
    sort_emit = sym("sbx_radix_sort_emitP")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed({"split": 4242, "packed": 2424}[form])
    tile = 4096  # 64-bit keys without a payload: 512 threads x 8
    counts = [2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile, 100_003]
    seen_passes, seen_options = set(), set()
    case = 0
    for count in counts:
        vb = max(1, (2 * count - 1).bit_length())  # values below 2^vb: at least twice as many as keys
        V = 1 << vb
        # bits of the parent position: split — sorted alone; packed — on top of the vb value bits
        widths = [1, 8, 9, 16, 20, 31] if form == "split" else [1, 16 - vb, 25 - vb, 33 - vb, 41 - vb, 49 - vb, 57 - vb, 64 - vb]
        for pb in widths:
            if pb < 1:
                continue
            case += 1
            use_map, use_a, use_b, use_pos = (bool((case * 7 + 3) >> i & 1) for i in range(4))
            seen_options |= {("map", use_map), ("bits_a", use_a), ("bits_b", use_b), ("pos_of", use_pos)}
            value = torch.randperm(V, device=dev, generator=g)[:count]
            parent = torch.randint(0, 1 << pb, (count,), device=dev, dtype=torch.int64, generator=g)
            passes = (Pass * 16)()
            if form == "split":
                keys = value | (parent << 32)
                n_passes = plan(0, 0, 32, 32 + pb, passes)
                low_mask = 0
                sorted_bits = parent
            else:
                keys = value | (parent << vb)  # (bit 63 may be set: compared as unsigned below)
                n_passes = plan(0, vb + pb, 0, 0, passes)
                low_mask = V - 1
                sorted_bits = keys ^ (-(1 << 63))
            assert 1 <= n_passes <= 8 and n_passes == ((pb if form == "split" else vb + pb) + 7) // 8
            seen_passes.add(n_passes)
            table = torch.randperm(V, device=dev, generator=g).to(torch.int32) if use_map else None
            words = (V + 31) // 32
            fill_a = torch.randint(-2 ** 31, 2 ** 31, (words,), device=dev, dtype=torch.int64, generator=g).to(torch.int32)
            fill_b = torch.randint(-2 ** 31, 2 ** 31, (words,), device=dev, dtype=torch.int64, generator=g).to(torch.int32)
            bits_a, bits_b = (fill_a.clone() if use_a else None), (fill_b.clone() if use_b else None)
            pos_of = torch.full((V,), -1, device=dev, dtype=torch.int32) if use_pos else None
            out = torch.full((count + 1,), -5, device=dev, dtype=torch.int32)
            ka, kb = keys.clone(), torch.zeros_like(keys)
            em = Emit(table.data_ptr() if use_map else None, out.data_ptr(), bits_a.data_ptr() if use_a else None,
                      bits_b.data_ptr() if use_b else None, pos_of.data_ptr() if use_pos else None, low_mask)
            hd.bind_stream()
            hd.check(arena_begin(hd.h))
            hd.check(sort_emit(hd.h, ptr(ka), ptr(kb), C.c_int64(count), passes, n_passes, C.byref(em)))
            torch.cuda.synchronize()
            what = (form, count, vb, pb, n_passes, use_map, use_a, use_b, use_pos)
            order = torch.sort(sorted_bits, stable=True)[1]
            v = keys[order] & 0xFFFFFFFF
            if low_mask:
                v = v & low_mask
            assert torch.equal(v, value[order]), what  # (the test's own key layout)
            want = (table.to(torch.int64)[v] if use_map else v).cpu().numpy()
            got = out.cpu().numpy()
            assert np.array_equal(got[:count], want.astype(np.int32)), what
            assert got[count] == -5, what
            add = np.zeros(words, np.uint32)
            np.bitwise_or.at(add, want >> 5, np.uint32(1) << (want & 31).astype(np.uint32))
            for used, bits, fill in ((use_a, bits_a, fill_a), (use_b, bits_b, fill_b)):
                if used:
                    assert np.array_equal(bits.cpu().numpy().view(np.uint32), fill.cpu().numpy().view(np.uint32) | add), what
            if use_pos:
                want_pos = np.full(V, -1, np.int32)
                want_pos[want] = np.arange(count, dtype=np.int32)
                assert np.array_equal(pos_of.cpu().numpy(), want_pos), what
    assert seen_passes == ({1, 2, 3, 4} if form == "split" else {1, 2, 3, 4, 5, 6, 7, 8}), seen_passes
    assert len(seen_options) == 8, seen_options
