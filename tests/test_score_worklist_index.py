"""csrc/score_worklist.h, compiled for the host exactly as libpgx.so compiles it for the device (tests/emu/score_worklist_emu.cpp):
the class of a weight, the item record, the (class, position) of a slot given four counts - and both sides of the lists replayed on
the CPU: whatever the order in which the cull kernel's workgroups append, the group kernel's grid runs every non-empty item exactly
once and no empty one, each on the XCD of its group, the heavier classes in front.  Plus the planner's decision to use the lists."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BOX, BOXALL, BALL, VANISHING = 0, 1, 2, 3          # score_plan.h GroupBound


@pytest.fixture(scope="module")
def wl(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("score_worklist") / "libscore_worklist_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "score_worklist_emu.cpp")])
    lib = C.CDLL(so)
    lib.wl_emu_class.argtypes = [C.c_uint] * 4
    lib.wl_emu_fits.argtypes = [C.c_int64, C.c_int]
    for f in (lib.wl_emu_item, lib.wl_emu_item_group, lib.wl_emu_item_column):
        f.restype = C.c_uint32
    lib.wl_emu_item.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    lib.wl_emu_item_group.argtypes = lib.wl_emu_item_column.argtypes = [C.c_uint32, C.c_int]
    lib.wl_emu_locate.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.wl_emu_run.restype = C.c_int64
    return lib


def test_constants_are_the_kernels(wl):
    xcds, classes, item_words, stride, count_words = (wl.wl_consts(k) for k in range(5))
    assert (xcds, classes, item_words) == (8, 4, 4)          # 8 XCDs; four classes; kCullWaves words per item
    assert stride * 4 >= 128 and count_words == xcds * classes * stride      # a cache line per count
    seen = {wl.wl_emu_count_index(x, c) for x in range(xcds) for c in range(classes)}
    assert len(seen) == 32 and max(seen) < count_words and all(i % stride == 0 for i in seen)


def test_class_of_a_weight_at_each_threshold_and_either_side(wl):
    for t in ((24, 64, 160), (1, 2, 3), (8, 8, 8), (32, 1 << 30, 1 << 30), (5, 5, 9)):
        for k, thr in enumerate(t):
            for wgt in (thr - 1, thr, thr + 1):
                if wgt < 1:
                    continue
                want = sum(1 for x in t if wgt >= x)
                assert wl.wl_emu_class(wgt, *t) == want, (t, wgt)
        assert wl.wl_emu_class(1, *t) == sum(1 for x in t if 1 >= x)
        assert wl.wl_emu_class(256, *t) == sum(1 for x in t if 256 >= x)      # the heaviest item there is: 4 words x 64 steps
    # two classes: thresholds no weight reaches leave classes 0 and 1 only
    assert {wl.wl_emu_class(w, 32, 1 << 30, 1 << 30) for w in range(1, 257)} == {0, 1}
    # ascending weights never descend in class
    cls = [wl.wl_emu_class(w, 16, 48, 128) for w in range(1, 257)]
    assert cls == sorted(cls) and set(cls) == {0, 1, 2, 3}


def test_every_slot_below_the_total_is_one_class_and_position_heaviest_first(wl):
    """exhaustive over count vectors from {0, 1, 2, 5}^4 (zeros in any class), plus large ones at the 32-bit end"""
    pos = C.c_uint32()
    vectors = list(itertools.product((0, 1, 2, 5), repeat=4)) + [(2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30 - 1), (0, 0, 0, 2 ** 32 - 1)]
    for c in vectors:
        arr = (C.c_uint32 * 4)(*c)
        total = sum(c)
        if total <= 64:
            got = []
            for slot in range(total):
                cls = wl.wl_emu_locate(arr, slot, C.byref(pos))
                assert cls >= 0, (c, slot)
                got.append((cls, pos.value))
            want = [(k, p) for k in (3, 2, 1, 0) for p in range(c[k])]      # heaviest class first, positions ascending
            assert got == want, c
            for slot in (total, total + 1, total + 1000, 2 ** 32 - 1):
                assert wl.wl_emu_locate(arr, slot, C.byref(pos)) == -1, (c, slot)
        else:
            edges = np.cumsum([0, c[3], c[2], c[1], c[0]])
            for k in range(4):
                if c[3 - k] == 0:
                    continue
                for slot, p in ((int(edges[k]), 0), (int(edges[k + 1]) - 1, c[3 - k] - 1)):
                    assert wl.wl_emu_locate(arr, slot, C.byref(pos)) == 3 - k and pos.value == p, (c, slot)
            if total < 2 ** 32:
                assert wl.wl_emu_locate(arr, total, C.byref(pos)) == -1


def test_item_record_round_trips_and_fits_are_exact(wl):
    for columns in (1, 2, 3, 4, 5, 8, 9, 4096):
        xb = wl.wl_emu_xbits(columns)
        assert (1 << xb) >= columns and (xb == 0 or (1 << (xb - 1)) < columns)
        gmax = (1 << (32 - xb)) - 1
        for g in (0, 1, 7, 8, 15624, gmax):
            for x in (0, columns // 2, columns - 1):
                item = wl.wl_emu_item(g, x, xb)
                assert (wl.wl_emu_item_group(item, xb), wl.wl_emu_item_column(item, xb)) == (g, x)
        assert wl.wl_emu_fits(gmax + 1, columns) == 1 and wl.wl_emu_fits(gmax + 2, columns) == 0
    assert wl.wl_emu_fits(0, 4) == 0 and wl.wl_emu_fits(4, 0) == 0


def _run(wl, weights, t, tiles):
    groups, columns = weights.shape
    cap = (groups + 7) // 8 * columns
    counts = np.zeros(32, np.uint32)
    taken = np.zeros(groups * columns, np.int32)
    order = np.zeros(8 * cap, np.uint32)
    w = np.ascontiguousarray(weights, np.uint32)
    tl = np.ascontiguousarray(tiles, np.int32)
    ran = wl.wl_emu_run(w.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int(groups), C.c_int(columns), (C.c_uint32 * 3)(*t),
                        tl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(len(tl)), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                        taken.ctypes.data_as(C.POINTER(C.c_int32)), order.ctypes.data_as(C.POINTER(C.c_uint32)))
    return ran, counts.reshape(8, 4), taken.reshape(groups, columns), order


def test_the_grid_runs_every_non_empty_item_once_whatever_the_append_order(wl):
    rng = np.random.default_rng(3)
    t = (24, 64, 160)
    for groups, columns in ((2, 1), (9, 1), (65, 2), (193, 1), (1537, 2), (100, 8)):
        for density in (0.0, 0.05, 0.4, 1.0):
            weights = (rng.integers(1, 257, (groups, columns)) * (rng.random((groups, columns)) < density)).astype(np.uint32)
            ntiles = (groups + 63) // 64 * columns
            for tiles in (np.arange(ntiles), np.arange(ntiles)[::-1], rng.permutation(ntiles)):
                ran, counts, taken, order = _run(wl, weights, t, tiles)
                assert ran == np.count_nonzero(weights)
                assert np.array_equal(taken, (weights != 0).astype(np.int32))
                cls = np.array([[wl.wl_emu_class(int(v), *t) if v else -1 for v in row] for row in weights])
                for xcd in range(8):
                    for c in range(4):
                        assert counts[xcd, c] == np.count_nonzero(cls[xcd::8] == c)
                    mine = order[xcd::8]                                   # this XCD's workgroups in dispatch order
                    k = int(counts[xcd].sum())
                    assert np.all(mine[:k] != 0) and np.all(mine[k:] == 0)    # the workgroups that leave come last
                    ran_cls = [wl.wl_emu_class(int(v), *t) for v in mine[:k]]
                    assert ran_cls == sorted(ran_cls, reverse=True)          # heaviest class first


def _plan(wl, bound=BOX, homography=0, n=4097, Mpad=320, ordered=1, masks=0, counters=0, split=0, group_xcd=-1, cull_segs=256,
          worklist=-1, t=(24, 64, 160)):
    out = (C.c_int64 * 12)()
    wl.wl_emu_plan((C.c_int64 * 14)(bound, homography, n, Mpad, ordered, masks, counters, split, group_xcd, cull_segs, worklist, *t), out)
    return dict(zip(("path", "worklist", "columns", "xbits", "cap", "grid", "t1", "t2", "t3", "split", "gblocks", "group_xcd"), out))


def test_the_plan_uses_the_lists_for_ordered_pose_batches_only_and_never_under_a_forced_geometry(wl):
    p = _plan(wl)
    groups = 65
    assert p["path"] == 2 and p["worklist"] == 1 and p["columns"] == 2 and p["xbits"] == 1 and p["cap"] == 9 * 2 and p["grid"] == 8 * 18
    assert (p["t1"], p["t2"], p["t3"]) == (24, 64, 160)
    assert p["split"] == 5 and p["gblocks"] == 72 * 5          # the strided geometry's fields stay what they were
    assert _plan(wl, counters=1)["worklist"] == 1             # pgx_score_stats counts the launch it describes
    off = dict(worklist=0, columns=0, xbits=0, cap=0, grid=0, t1=0, t2=0, t3=0)
    for kw in (dict(worklist=0), dict(ordered=0), dict(group_xcd=0), dict(split=3), dict(split=5), dict(cull_segs=1), dict(cull_segs=255),
               dict(masks=1), dict(homography=1), dict(bound=BALL), dict(bound=BOXALL), dict(bound=VANISHING)):
        q = _plan(wl, **kw)
        assert q["path"] == 2 and {k: q[k] for k in off} == off, kw
        same = _plan(wl, **dict(kw, worklist=0))
        assert (q["split"], q["gblocks"], q["group_xcd"]) == (same["split"], same["gblocks"], same["group_xcd"])
    # the A/B switch turns the lists on for any type on the co-located mapping, and for a pose batch forced onto it
    for kw in (dict(bound=BALL), dict(bound=VANISHING), dict(homography=1), dict(ordered=0, group_xcd=1)):
        assert _plan(wl, worklist=1, **kw)["worklist"] == 1, kw
    assert _plan(wl, worklist=1, ordered=0)["worklist"] == 0 and _plan(wl, worklist=1, split=3)["worklist"] == 0
    assert _plan(wl, group_xcd=1)["worklist"] == 1            # forcing the mapping the batch takes anyway changes nothing
    # geometry: one column up to four words, a partial last item, the record's bits
    for Mpad, columns, xbits in ((64, 1, 0), (256, 1, 0), (320, 2, 1), (512, 2, 1), (576, 3, 2), (2048, 8, 3)):
        q = _plan(wl, Mpad=Mpad, n=10 ** 6)
        assert (q["worklist"], q["columns"], q["xbits"], q["cap"], q["grid"]) == (1, columns, xbits, 1954 * columns, 8 * 1954 * columns)
    # too many items for the lists' memory: the strided parts
    assert _plan(wl, Mpad=1 << 20, n=10 ** 6)["worklist"] == 0
    assert _plan(wl, t=(8, 1 << 30, 1 << 30))["t2"] == 1 << 30
    assert groups == (4097 + 63) // 64
