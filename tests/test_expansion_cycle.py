"""The cycle driver of csrc/expansion_cycle.h (compiled into tests/emu/libmf_emu.so exactly as libpgx.so compiles it) over the CPU
backend of tests/emu/mf_emu.cpp, against the oracle's pgxo_expansion: the plain loop without skip rule, first-cycle memo, batches or
identical-call answer.  All four claim to be invisible, so labels, energy and cycles must be the oracle's under every schedule - the
unbatched loop and the batched one under four scripts of declined moves."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers import random_sym_graph
from test_emu import _p, emu  # noqa: F401  (the fixture that builds and loads libmf_emu.so)

NONE, EVERY_FIRST_ATTEMPT, RANDOM, FIRST_OF_BATCH = 0, 1, 2, 3                 # mf_emu.cpp kDecline*
SCHEDULES = ((0, NONE), (1, NONE), (1, EVERY_FIRST_ATTEMPT), (1, RANDOM), (1, FIRST_OF_BATCH))   # (batched, decline script)
WRITTEN, UPLOADED, INJECTED, POINTS, RESIDENT = range(5)                       # mf_emu.cpp emu_cycle_event
COUNTS = ("solved", "skipped_host", "skipped_device", "restored", "declined", "batches_after_decline", "backend_declines",
          "backend_skips", "answered", "memo_hits")


class Ctx:
    """What a libpgx context is to pgx_expansion: the state of expansion_cycle.h and the memo's snapshots."""

    def __init__(self, lib, memo=1):
        lib.emu_cycle_new.restype = C.c_void_p
        self.lib, self.h = lib, C.c_void_p(lib.emu_cycle_new(C.c_int(memo)))

    def close(self):
        self.lib.emu_cycle_free(self.h)

    def event(self, event, arg=0, ids=None):
        ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
        self.lib.emu_cycle_event(self.h, C.c_int(event), C.c_int(arg), _p(ids, C.c_int64), C.c_int(0 if ids is None else ids.size))

    def run(self, Dq, graph, lq, hq, labels, max_cycles=1000, batched=0, script=NONE, seed=0, graph_version=1, want_rc=0):
        n, L = Dq.shape
        lab = np.ascontiguousarray(labels, np.int32).copy()
        Dq = np.ascontiguousarray(Dq, np.int64)
        off, idx, mult = (np.ascontiguousarray(g, np.int32) for g in graph)
        if idx.size == 0:
            idx, mult = np.zeros(1, np.int32), np.ones(1, np.int32)
        e, cyc, counts = C.c_int64(), C.c_int(), np.zeros(10, np.int64)
        rc = self.lib.emu_cycle_run(self.h, C.c_int64(n), C.c_int(L), _p(Dq, C.c_int64), _p(off, C.c_int32), _p(idx, C.c_int32),
                                    _p(mult, C.c_int32), C.c_int64(lq), C.c_int64(hq), _p(lab, C.c_int32), C.c_int(max_cycles),
                                    C.c_int(batched), C.c_int64(graph_version), C.c_int(script), C.c_uint64(seed), C.byref(e),
                                    C.byref(cyc), _p(counts, C.c_int64))
        assert rc == want_rc, f"the cycle driver returned {rc}"
        if rc != 0:
            return None
        k = dict(zip(COUNTS, (int(v) for v in counts)))
        assert k["solved"] + k["skipped_host"] + k["skipped_device"] + k["restored"] == L * cyc.value, k     # every move is accounted for once
        assert k["declined"] == k["backend_declines"] and k["skipped_device"] == k["backend_skips"], k          # ... as the backend saw it
        return lab, int(e.value), int(cyc.value), k


def expand(lib, Dq, graph, lq, hq, labels, ids=None, **kw):
    """one call on a fresh context, set up as the C ABI's callers do: unary table, labels, expansion"""
    ctx = Ctx(lib)
    try:
        ctx.event(RESIDENT, ids=np.arange(Dq.shape[1]) if ids is None else ids)
        ctx.event(UPLOADED, arg=int(np.max(labels)))
        return ctx.run(Dq, graph, lq, hq, labels, **kw)
    finally:
        ctx.close()


def random_problem(rng, n=None, L=None, lq=None):
    n = int(rng.integers(2, 61)) if n is None else n
    L = int(rng.integers(2, 9)) if L is None else L
    Dq = rng.integers(0, 20, (n, L)).astype(np.int64)                       # costs full of ties
    graph = random_sym_graph(rng, n, float(rng.choice([0.0, 0.1, 0.3])))
    lq = int(rng.choice([0, 2, 4, 8])) if lq is None else lq
    return Dq, graph, lq, int(rng.choice([0, 3, 10, 40]))


def test_emulated_energy_is_the_oracles(emu, oracle):  # noqa: F811
    rng = np.random.default_rng(3)
    emu.emu_cycle_energy.restype = C.c_int64
    for _ in range(200):
        Dq, graph, lq, hq = random_problem(rng)
        n, L = Dq.shape
        lab = rng.integers(0, L, n).astype(np.int32)
        off, idx, mult = (np.ascontiguousarray(g, np.int32) for g in graph)
        if idx.size == 0:
            idx, mult = np.zeros(1, np.int32), np.ones(1, np.int32)
        got = emu.emu_cycle_energy(C.c_int64(n), C.c_int(L), _p(Dq, C.c_int64), _p(off, C.c_int32), _p(idx, C.c_int32), _p(mult, C.c_int32),
                                   C.c_int64(lq), C.c_int64(hq), _p(lab, C.c_int32))
        assert got == oracle.energy(Dq, graph, lq, hq, lab)


def test_every_schedule_computes_the_oracles_expansion(emu, oracle):  # noqa: F811
    """40 random problems (n 2..60, L 2..8, costs full of ties, lambda_q in {0, 2, 4, 8}, h in {0, 3, 10, 40}) x 4 starting labellings
    (zeros, constant, random, argmin) x max_cycles in {1, 2, 1000} x (unbatched, batched under each of the four decline scripts): labels,
    energy_q and cycles equal oracle.expansion's in each of the 2 400 runs, and every branch of the driver ran.  Totals over the fixed
    seeds: 19 410 moves solved, 996 skipped on the host, 474 skipped on the device, 7 554 declined, 6 002 batches opened behind a
    decline (restored moves: test_memo_restores_the_unchanged_prefix)."""
    rng = np.random.default_rng(11)
    total = dict.fromkeys(COUNTS, 0)
    runs = 0
    for trial in range(40):
        Dq, graph, lq, hq = random_problem(rng)
        n, L = Dq.shape
        starts = (np.zeros(n, np.int32), np.full(n, rng.integers(0, L), np.int32), rng.integers(0, L, n).astype(np.int32),
                  np.argmin(Dq, axis=1).astype(np.int32))
        for start, max_cycles in itertools.product(starts, (1, 2, 1000)):
            ref, ref_e, ref_cyc = oracle.expansion(Dq, graph, lq, hq, start, max_cycles=max_cycles)
            for batched, script in SCHEDULES:
                lab, e, cyc, k = expand(emu, Dq, graph, lq, hq, start, max_cycles=max_cycles, batched=batched, script=script, seed=trial + 1)
                where = dict(trial=trial, n=n, L=L, lq=lq, hq=hq, max_cycles=max_cycles, batched=batched, script=script)
                assert np.array_equal(lab, ref), where
                assert e == ref_e and cyc == ref_cyc, where
                assert not k["answered"] and (batched and lq > 0 or k["declined"] + k["skipped_device"] == 0), where
                for name in COUNTS:
                    total[name] += k[name]
                runs += 1
    assert runs == 40 * 4 * 3 * 5
    for name in ("solved", "skipped_host", "skipped_device", "declined", "batches_after_decline"):
        assert total[name] > 0, (name, total)


def column_ids(tables):
    """one number per distinct column content: the identity pgx_pearl_unary gives a column is what it was computed from"""
    seen = {}
    return [np.array([seen.setdefault(T[:, l].tobytes(), len(seen)) for l in range(T.shape[1])], np.int64) for T in tables]


@pytest.mark.parametrize("batched,script", SCHEDULES)
def test_memo_restores_the_unchanged_prefix(emu, oracle, batched, script):  # noqa: F811
    """The sequence of test_first_cycle_memo_is_transparent on 40 sites: expansions from zeros on tables that share a leading block of
    columns, then have one more column appended, then a middle column altered, then are identical.  Every call equals the oracle's and
    restores exactly the unchanged prefix (computed here from the tables): 0, 3, 2 and 5 moves per schedule."""
    rng = np.random.default_rng(21)
    n, lq, hq = 40, 4, 10
    cols = rng.integers(0, 20, (n, 6)).astype(np.int64)
    graph = random_sym_graph(rng, n, 0.1)
    altered = cols[:, 2].copy()
    altered[::3] += 1
    tables = [cols[:, :3], cols[:, :4], np.column_stack([cols[:, :2], altered, cols[:, 3:5]])]
    tables.append(tables[-1].copy())
    ctx = Ctx(emu)
    try:
        prev, restored = None, []
        for T, ids in zip(tables, column_ids(tables)):
            want = 0
            while prev is not None and want < min(T.shape[1], prev.shape[1]) and np.array_equal(T[:, want], prev[:, want]):
                want += 1
            ctx.event(RESIDENT, ids=ids)
            ctx.event(UPLOADED, arg=0)
            lab, e, cyc, k = ctx.run(T, graph, lq, hq, np.zeros(n, np.int32), batched=batched, script=script, seed=5)
            ref, ref_e, ref_cyc = oracle.expansion(T, graph, lq, hq, np.zeros(n, np.int32))
            assert np.array_equal(lab, ref) and e == ref_e and cyc == ref_cyc
            assert k["restored"] == want, (k, want)
            restored.append(k["restored"])
            prev = T
        assert restored == [0, 3, 2, 5] and k["memo_hits"] == 10
        # not from zeros, lambda = 0, another graph, the memo switched off: nothing is restored
        ctx.event(UPLOADED, arg=1)
        assert ctx.run(tables[-1], graph, lq, hq, np.ones(n, np.int32), batched=batched, script=script)[3]["restored"] == 0
        ctx.event(UPLOADED, arg=0)
        assert ctx.run(tables[-1], graph, 0, hq, np.zeros(n, np.int32), batched=batched, script=script)[3]["restored"] == 0
        ctx.event(UPLOADED, arg=0)
        lab, e, cyc, k = ctx.run(tables[-1], graph, lq, hq, np.zeros(n, np.int32), batched=batched, script=script, graph_version=2)
        assert k["restored"] == 0 and np.array_equal(lab, ref) and e == ref_e and cyc == ref_cyc
    finally:
        ctx.close()
    off = Ctx(emu, memo=0)
    try:
        for _ in range(2):
            off.event(RESIDENT, ids=np.arange(5))
            off.event(UPLOADED, arg=0)
            lab, e, cyc, k = off.run(tables[-1], graph, lq, hq, np.zeros(n, np.int32), batched=batched, script=script)
            assert k["restored"] == 0 and k["memo_hits"] == 0 and np.array_equal(lab, ref) and e == ref_e and cyc == ref_cyc
    finally:
        off.close()


@pytest.mark.parametrize("batched,script", SCHEDULES)
def test_identical_call_is_answered_until_an_event_says_otherwise(emu, oracle, batched, script):  # noqa: F811
    """A second identical call after a fixed point is answered with zero moves solved, the same energy and cycles = 1; after each event
    of ExpansionState (labels written, labels uploaded, a table injected, the point set changed, other columns resident), after another
    lambda, h or graph, and after a final cycle that only moved ties, it is not - and equals the oracle's either way."""
    rng = np.random.default_rng(31)
    Dq, graph, lq, hq = random_problem(rng, n=40, L=5, lq=4)
    n, L = Dq.shape
    ids = np.arange(L)
    kw = dict(batched=batched, script=script, seed=9)
    ctx = Ctx(emu)
    try:
        def fixed_point():
            ctx.event(RESIDENT, ids=ids)
            ctx.event(UPLOADED, arg=0)
            lab, e, cyc, k = ctx.run(Dq, graph, lq, hq, np.zeros(n, np.int32), **kw)
            assert not k["answered"]
            return lab, e

        def again(lab, e, answered, **changes):
            args = dict(lq=lq, hq=hq, graph_version=1)
            args.update(changes)
            got, e2, cyc2, k = ctx.run(Dq, graph, args["lq"], args["hq"], lab, graph_version=args["graph_version"], **kw)
            ref, ref_e, ref_cyc = oracle.expansion(Dq, graph, args["lq"], args["hq"], lab)
            assert np.array_equal(got, ref) and e2 == ref_e and cyc2 == ref_cyc
            assert k["answered"] == answered, (k, changes)
            if answered:
                assert k["solved"] == 0 and k["skipped_host"] == L and cyc2 == 1 and e2 == e and np.array_equal(got, lab)
            return got

        lab, e = fixed_point()
        again(lab, e, 1)
        again(lab, e, 1)                                        # ... as often as it is asked
        ctx.event(RESIDENT, ids=ids)                            # the same identities: still the same problem
        again(lab, e, 1)
        ctx.event(WRITTEN)
        again(lab, e, 0)
        again(lab, e, 1)                                        # (that run ended on the fixed point again)
        ctx.event(UPLOADED, arg=int(lab.max()))
        again(lab, e, 0)
        ctx.event(INJECTED)
        again(lab, e, 0)
        again(lab, e, 0)                                        # a table without identity records no fixed point either
        lab, e = fixed_point()
        ctx.event(POINTS)
        ctx.event(RESIDENT, ids=ids)                            # the same models on the new points are other columns
        again(lab, e, 0)
        lab, e = fixed_point()
        ctx.event(RESIDENT, ids=ids[::-1])
        again(lab, e, 0)
        lab, e = fixed_point()
        again(lab, e, 0, hq=hq + 1)
        lab, e = fixed_point()
        again(lab, e, 0, lq=lq + 2)
        lab, e = fixed_point()
        again(lab, e, 0, graph_version=2)
        lab, e = fixed_point()
        got, e2, cyc2, k = ctx.run(Dq, graph, lq, hq, lab, max_cycles=0, **kw)       # no cycle allowed: nothing to answer, nothing runs
        assert (e2, cyc2) == (e, 0) and not k["answered"] and k["solved"] == 0 and np.array_equal(got, lab)
        # lambda = 0: the graph is not looked at (costs without ties, or the closed form keeps moving them at equal energy)
        Dq = np.random.default_rng(2).permutation(n * L).reshape(n, L).astype(np.int64)
        ctx.event(RESIDENT, ids=ids + 10)
        ctx.event(UPLOADED, arg=0)
        lab0, e0, _, _ = ctx.run(Dq, graph, 0, hq, np.zeros(n, np.int32), **kw)
        again(lab0, e0, 1, lq=0, graph_version=7)
        # a final cycle that only moved ties (equal costs: every move takes every site at equal energy) is no fixed point
        flat = np.full((5, 3), 7, np.int64)
        ring = random_sym_graph(np.random.default_rng(1), 5, 1.0)
        ctx.event(RESIDENT, ids=np.arange(3))
        ctx.event(UPLOADED, arg=0)
        tie, te, tcyc, k = ctx.run(flat, ring, 2, 0, np.zeros(5, np.int32), **kw)
        ref, ref_e, ref_cyc = oracle.expansion(flat, ring, 2, 0, np.zeros(5, np.int32))
        assert np.array_equal(tie, ref) and (te, tcyc) == (ref_e, ref_cyc) == (35, 1) and tie.any() and not k["answered"]
        got, e2, cyc2, k = ctx.run(flat, ring, 2, 0, tie, **kw)
        ref, ref_e, ref_cyc = oracle.expansion(flat, ring, 2, 0, tie)
        assert not k["answered"] and k["solved"] > 0 and np.array_equal(got, ref) and (e2, cyc2) == (ref_e, ref_cyc)
    finally:
        ctx.close()


def test_a_broken_batch_protocol_stays_an_error(emu):  # noqa: F811
    """"A batched move was not enqueued" and "move of a batch did not run" (a slot reports status 2 for a move the host's bookkeeping says
    had to run) end the expansion with the backend's error instead of a labelling."""
    rng = np.random.default_rng(41)
    Dq, graph, lq, hq = random_problem(rng, n=20, L=4, lq=4)
    for broken in (4, 5):                                       # mf_emu.cpp kBreakNotEnqueued, kBreakDidNotRun
        assert expand(emu, Dq, graph, lq, hq, np.zeros(20, np.int32), batched=1, script=broken, want_rc=-20) is None
        assert expand(emu, Dq, graph, lq, hq, np.zeros(20, np.int32), batched=0, script=broken) is not None     # (no batch: nothing to break)
