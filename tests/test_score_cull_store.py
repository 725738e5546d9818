"""csrc/score_worklist.h: wl_tile_store_index - which keep word a thread of score_cull_kernel stores behind the tile's barrier (thread
t: group t / 4 of the tile, word t % 4 of the workgroup's item column) - against the plain `g * W + w` loop over the tile's groups
and the column's words.  Compiled for the host as libpgx.so compiles it for the device (tests/emu/score_cull_store_emu.cpp).

Row lengths W 1 .. 9 (a last column of one to four words), every column, tiles of 1, 7, 8, 63 and 64 groups at the start, in the
middle and at the end of the groups: every word of the tile is stored once, by the thread the layout names, and nothing else is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("score_cull_store") / "libscore_cull_store_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "score_cull_store_emu.cpp")])
    lib = C.CDLL(so)
    lib.wl_emu_tile_store.argtypes = [C.POINTER(C.c_uint64), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.wl_emu_tile_store.restype = C.c_int64
    return lib


def test_every_word_of_the_tile_is_stored_once_by_its_thread(emu):
    assert emu.wl_emu_item_words_per_workgroup() == 4
    groups = 200
    for W in range(1, 10):
        for x in range((W + 3) // 4):
            for t0, cnt in ((0, 64), (64, 64), (136, 64), (0, 1), (192, 8), (128, 7), (128, 63), (199, 1)):
                keep = np.zeros(groups * W, dtype=np.uint64)
                stores = emu.wl_emu_tile_store(keep.ctypes.data_as(C.POINTER(C.c_uint64)), groups, W, t0, cnt, x)
                want = np.zeros((groups, W), dtype=np.uint64)
                for g in range(t0, t0 + cnt):                       # the plain loop
                    for w in range(4 * x, min(4 * x + 4, W)):
                        want[g, w] = ((g - t0) << 32) | (w - 4 * x + 1)
                assert stores == cnt * (min(4 * x + 4, W) - 4 * x), (W, x, t0, cnt, stores)
                assert np.array_equal(keep.reshape(groups, W), want), (W, x, t0, cnt)


def test_four_neighbouring_threads_store_adjacent_words(emu):
    """the point of the layout: threads 4 k .. 4 k + 3 write the 32 contiguous bytes of one item"""
    W, x, t0 = 8, 1, 64
    keep = np.zeros(200 * W, dtype=np.uint64)
    emu.wl_emu_tile_store(keep.ctypes.data_as(C.POINTER(C.c_uint64)), 200, W, t0, 64, x)
    at = np.flatnonzero(keep)
    assert at.size == 256 and np.array_equal(at.reshape(64, 4), (t0 + np.arange(64))[:, None] * W + 4 * x + np.arange(4)[None, :])
    assert np.array_equal(keep[at] & np.uint64(0xffffffff), np.tile(np.arange(1, 5, dtype=np.uint64), 64))
