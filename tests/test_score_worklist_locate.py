"""csrc/score_worklist.h: wl_locate_select - the slot -> (class, position) search of score_group_kernel, written without early exits so
that the four counts are one round trip - against wl_locate, which the host replay and tests/test_score_worklist_index.py hold to the
lists' definition.  Both compiled for the host as libpgx.so compiles them for the device (tests/emu/score_worklist_locate_emu.cpp).

Count vectors as in test_score_worklist_index.py: {0, 1, 2, 5}^4 and the two at the 32-bit end.  Every slot from 0 to total + 2 (the
slots at and past the total: "this workgroup leaves"), and the last 32-bit slot; for the two large vectors, where that is 2^32 slots,
every slot within 3 of a class edge, of zero and of the 32-bit end, and a million consecutive slots from each edge.

Also the item's keep words as the kernel fetches them with bit 32 (wl_words_begin, wl_words_shift): one 4-word load that stays inside
the group's row, moved down where the row's last item is short."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = list(itertools.product((0, 1, 2, 5), repeat=4))
LARGE = [(2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30 - 1), (0, 0, 0, 2 ** 32 - 1)]


@pytest.fixture(scope="module")
def loc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("score_worklist_locate") / "libscore_worklist_locate_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "score_worklist_locate_emu.cpp")])
    lib = C.CDLL(so)
    lib.wl_emu_locate.argtypes = lib.wl_emu_locate_select.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.wl_emu_locate_mismatches.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]
    lib.wl_emu_locate_mismatches.restype = C.c_int64
    return lib


def _both(loc, arr, slot):
    pa, pb = C.c_uint32(), C.c_uint32()
    a, b = loc.wl_emu_locate(arr, slot, C.byref(pa)), loc.wl_emu_locate_select(arr, slot, C.byref(pb))
    return (a, pa.value if a >= 0 else None), (b, pb.value if b >= 0 else None)


def test_select_equals_locate_on_every_slot_up_to_the_total_and_past_it(loc):
    for c in SMALL:
        arr = (C.c_uint32 * 4)(*c)
        total = sum(c)
        want = [(k, p) for k in (3, 2, 1, 0) for p in range(c[k])] + [(-1, None)] * 3        # heaviest class first; total .. total + 2 leave
        for slot in list(range(total + 3)) + [total + 1000, 2 ** 32 - 1]:
            a, b = _both(loc, arr, slot)
            assert a == b, (c, slot, a, b)
            assert b == (want[slot] if slot < len(want) else (-1, None)), (c, slot, b)      # ... and both are the definition
        assert loc.wl_emu_locate_mismatches(arr, 0, total + 3) == 0


def test_select_equals_locate_at_the_32_bit_end(loc):
    for c in LARGE:
        arr = (C.c_uint32 * 4)(*c)
        edges = [int(e) for e in np.cumsum([0, c[3], c[2], c[1], c[0]], dtype=np.int64)]
        assert edges[-1] == 2 ** 32 - 1
        near = {s for e in edges + [0, 2 ** 32 - 1] for s in range(e - 3, e + 4) if 0 <= s < 2 ** 32}
        for slot in sorted(near):
            a, b = _both(loc, arr, slot)
            assert a == b, (c, slot, a, b)
            k = int(np.searchsorted(edges, slot, side="right")) - 1                          # the definition, from the edges
            assert b == ((3 - k, slot - edges[k]) if slot < edges[-1] else (-1, None)), (c, slot, b)
        for e in edges[:-1]:
            assert loc.wl_emu_locate_mismatches(arr, e, min(1 << 20, 2 ** 32 - 1 - e)) == 0
        assert loc.wl_emu_locate_mismatches(arr, 2 ** 32 - (1 << 20), (1 << 20) - 1) == 0
        assert loc.wl_emu_locate_mismatches(arr, 2 ** 32 - 1, 1) == 0


def test_an_items_keep_words_come_from_one_load_inside_the_row(loc):
    """wl_words_begin / wl_words_shift: for every row length W >= 4 and every item of it, words w0 .. w0 + 3 with zeros at and past W"""
    loc.wl_emu_item_words.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    for W in range(4, 14):
        row = np.arange(1, W + 1, dtype=np.uint64) * np.uint64(0x0101010101010101)     # distinct, non-zero, both halves in use
        for w0 in range(0, W, 4):
            out = (C.c_uint64 * 4)()
            b = loc.wl_emu_item_words(row.ctypes.data_as(C.POINTER(C.c_uint64)), W, w0, out)
            assert 0 <= b <= w0 and b + 4 <= W, (W, w0, b)
            want = [int(row[w0 + k]) if w0 + k < W else 0 for k in range(4)]
            assert list(out) == want, (W, w0, list(out), want)
