"""csrc/score_runs.h, compiled for the host exactly as libpgx.so compiles it for the device (tests/emu/score_runs_emu.cpp): the
distance to the end of a run from a head mask, the (count, value) word, and the segmented reduction of score_group_kernel's queued
exact path driven by both - against scalar loops and per-run sums computed directly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = (1 << 64) - 1


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("score_runs") / "libscore_runs_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "score_runs_emu.cpp")])
    lib = C.CDLL(so)
    lib.sr_run_dist.argtypes, lib.sr_run_dist.restype = [C.c_uint64, C.c_int], C.c_int
    lib.sr_pack.argtypes, lib.sr_pack.restype = [C.c_uint, C.c_uint64], C.c_uint64
    lib.sr_count.argtypes, lib.sr_count.restype = [C.c_uint64], C.c_uint
    lib.sr_value.argtypes, lib.sr_value.restype = [C.c_uint64], C.c_uint64
    lib.sr_max_term.restype = C.c_uint64
    lib.sr_segmented_sum.argtypes = [C.c_uint64, C.POINTER(C.c_uint), C.POINTER(C.c_uint64), C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
    lib.sr_segmented_sum.restype = C.c_int
    return lib


def _masks():
    """head masks (bit 0 always set: lane 0 starts a run): one run of 64, 64 runs of one, both alternations, blocks, random"""
    out = [1, ALL, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA | 1, 1 | (1 << 63), 1 | (1 << 1), 1 | (1 << 32), 0x0101010101010101,
           ALL >> 1, (ALL << 32) & ALL | 1]
    rng = np.random.default_rng(7)
    for density in (0.02, 0.1, 0.5, 0.9):
        for _ in range(60):
            bits = rng.random(64) < density
            out.append(1 | sum(1 << int(i) for i in np.flatnonzero(bits)))
    return out


def _run_ends(heads):
    """scalar loop: for every lane, the first lane behind it that starts a run (64 if none)"""
    ends, nxt = [0] * 64, 64
    for i in range(63, -1, -1):
        ends[i] = nxt
        if (heads >> i) & 1:
            nxt = i
    return ends


def test_distance_to_run_end_equals_a_scalar_loop(runs):
    for heads in _masks():
        ends = _run_ends(heads)
        for lane in range(64):
            assert runs.sr_run_dist(heads, lane) == ends[lane] - lane, (hex(heads), lane)


def _segmented(runs, heads, count, value):
    oc, ov = np.zeros(64, np.uint32), np.zeros(64, np.uint64)
    rounds = runs.sr_segmented_sum(heads, count.ctypes.data_as(C.POINTER(C.c_uint)), value.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   oc.ctypes.data_as(C.POINTER(C.c_uint)), ov.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rounds, oc, ov


def test_segmented_sum_equals_per_run_sums(runs):
    top = int(runs.sr_max_term())
    assert top == 1 << 50 and runs.sr_max_terms() == 64
    rng = np.random.default_rng(11)
    for heads in _masks():
        ends = _run_ends(heads)
        for mode in range(3):
            # counts all 0 | mixed | all 1; terms random in [0, 2^50] whatever the count, at the extreme all exactly 2^50
            count = (rng.random(64) < (0.0, 0.5, 1.0)[mode]).astype(np.uint32)
            value = rng.integers(0, top, 64, dtype=np.uint64, endpoint=True)
            if mode == 2:
                value[:] = top
            rounds, oc, ov = _segmented(runs, heads, count, value)
            longest = max(ends[i] - i for i in range(64))
            assert rounds == (longest - 1).bit_length()          # stops with the first round no run reaches
            for lane in range(64):
                assert int(oc[lane]) == int(count[lane:ends[lane]].sum()), (hex(heads), lane)
                assert int(ov[lane]) == sum(int(v) for v in value[lane:ends[lane]]), (hex(heads), lane)


def test_pack_round_trips_at_the_extremes(runs):
    top = 1 << 50
    for count, value in ((0, 0), (1, 0), (0, top), (1, top), (64, 64 * top), (64, 0), (0, 64 * top), (63, 64 * top - 1), (17, 123456789)):
        p = runs.sr_pack(count, value)
        assert (runs.sr_count(p), runs.sr_value(p)) == (count, value)
    # 64 terms of exactly 2^50 with count 1 each, added as packed words: no carry from the value into the count
    p = 0
    for _ in range(64):
        p = (p + runs.sr_pack(1, top)) & ALL
    assert (runs.sr_count(p), runs.sr_value(p)) == (64, 64 * top)
    # one run of 64 through the reduction itself
    rounds, oc, ov = _segmented(runs, 1, np.ones(64, np.uint32), np.full(64, top, np.uint64))
    assert rounds == 6 and int(oc[0]) == 64 and int(ov[0]) == 64 * top
