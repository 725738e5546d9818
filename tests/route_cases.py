"""The routing cases of tests/golden/expansion_routes_v1.json: which min-cut solver takes a move, pinned at the smallest shapes on
either side of each routing edge (csrc/move_route.h).  tests/golden/make_golden_routes.py records them, tests/test_gpu_routes.py
replays them; both go through run_case(), so the two cannot drift apart.

Expansion cases, each in a fresh context: (1) expansion from zeros, (2) the same call again, (3) L single expand_alpha calls from
seeded random labels.  After each step: SHA-256 of the labels, energy_q, cycles, the six expansion_paths entries, mincuts /
relabelled_sites / skipped_moves of expansion_stats and both one_workgroup_launches counters.
Cut cases: gc_labeling and gc_inliers of a seeded 2-D line problem with lambda 0.3: flag hash, count, index list hash and what the
two calls added to expansion_paths."""
import contextlib
import functools
import hashlib
import os

import numpy as np

from helpers import csr_from_pairs, realistic_labeling_problem

ROUTE_ENV = ("PGX_MF_TILE", "PGX_MF_TILE_BATCH", "PGX_MF_REGION", "PGX_TILE_EXPANSION_MAX", "PGX_TILE_MINI", "PGX_GC_FLIP")
SWITCHES = ({}, {"PGX_MF_TILE": "0"}, {"PGX_MF_TILE_BATCH": "0"}, {"PGX_MF_REGION": "0"}, {"PGX_TILE_EXPANSION_MAX": "0"},
            {"PGX_TILE_EXPANSION_MAX": "8192"}, {"PGX_TILE_MINI": "0"})
SIZES = (700, 1024, 1025, 3000, 8192, 8193)    # the LDS-resident kernel's limit, tile_expansion_max and the one-workgroup limit, both sides
CUT_SIZES = (187, 8192, 8193)
STAT_KEYS = ("mincuts", "relabelled_sites", "skipped_moves")


def _env_id(env):
    return ",".join(f"{k[4:]}={v}" for k, v in env.items()) or "default"


def cases():
    """{case id: (kind, problem name, environment)} in a fixed order"""
    out = {}
    for n in SIZES:
        for env in SWITCHES:
            out[f"expansion-{n}-{_env_id(env)}"] = ("expansion", f"realistic-{n}", env)
    out["expansion-domino3000-MF_TILE=0"] = ("expansion", "domino-3000", {"PGX_MF_TILE": "0"})
    out["expansion-wide12000-default"] = ("expansion", "wide-12000", {})
    out["expansion-30000-default"] = ("expansion", "realistic-30000", {})
    for n in CUT_SIZES:
        for flip in ("1", "0"):
            for tile in ("1", "0"):
                env = {"PGX_GC_FLIP": flip, "PGX_MF_TILE": tile}
                out[f"cut-{n}-{_env_id(env)}"] = ("cut", f"line-{n}", env)
    return out


@functools.lru_cache(maxsize=None)
def problem(name):
    """(Dq [n, L], graph, lambda, label cost) of an expansion problem / (points, model, T2) of a cut problem; built once per
    process and shared by the cases that use it (nobody writes to the arrays)"""
    kind, n = name.split("-")
    n = int(n)
    if kind == "realistic":
        L, lam, h = (6, 0.15, 4.0) if n == 30000 else (5, 0.2, 3.0)
        Dq, graph = realistic_labeling_problem(n, L=L, lam=lam, seed=n + L)
        return Dq, graph, lam, h
    if kind == "domino":      # test_gpu_parity.py test_region_moves_decline_a_domino_of_weak_sinks
        a = np.arange(n - 1)
        graph = csr_from_pairs(n, a, a + 1, np.full(n - 1, 2))
        Dq = np.zeros((n, 2), np.int64)
        Dq[:, 1] = 1
        Dq[0] = (1 << 40, 0)
        return Dq, graph, 0.5, 0.0
    if kind == "wide":        # test_gpu_parity.py test_region_moves_decline_wide_graphs: a site of more than 32 neighbours
        rng = np.random.default_rng(9)
        L, lam, h = 4, 0.2, 2.0
        Dq, (off, idx, mult) = realistic_labeling_problem(n, L=L, lam=lam, seed=99)
        src = np.repeat(np.arange(n), np.diff(off))
        iu, ju, mu = src[src < idx], idx[src < idx], mult[src < idx]
        for hub in (17, 5000):
            spokes = np.setdiff1d(rng.choice(n, 60, replace=False), np.concatenate([[hub], idx[off[hub]:off[hub + 1]]]))
            iu = np.concatenate([iu, np.minimum(hub, spokes)])
            ju = np.concatenate([ju, np.maximum(hub, spokes)])
            mu = np.concatenate([mu, np.ones(spokes.size, mu.dtype)])
        graph = csr_from_pairs(n, iu, ju, mu)
        assert np.diff(graph[0]).max() > 32
        return Dq, graph, lam, h
    if kind == "line":
        from pyprogressivex import datasets
        per = n // 5
        pts, _, gt = datasets.make_lines(n_per_line=per, n_lines=3, n_outliers=n - 3 * per, seed=n)
        assert pts.shape[0] == n
        return pts, gt[0], 2.25 * 2.0 * 2.0
    raise KeyError(name)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.pop(k, None) for k in ROUTE_ENV}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ROUTE_ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _counters(ctx):
    st = ctx.expansion_stats()
    return {"paths": ctx.expansion_paths(), "stats": {k: st[k] for k in STAT_KEYS}, "launches": ctx.one_workgroup_launches()}


def _run_expansion(ctx, name):
    Dq, graph, lam, h = problem(name)
    n, L = Dq.shape
    ctx.set_unary_q(Dq)
    ctx.set_graph(*graph)
    ctx.set_labels(np.zeros(n, np.int32))
    rec = {}
    for step in ("from_zeros", "again"):
        eq, _, cycles = ctx.expansion(lam, h)
        rec[step] = {"labels": sha(ctx.get_labels()), "energy_q": int(eq), "cycles": int(cycles), **_counters(ctx)}
    ctx.set_labels(np.random.default_rng(n).integers(0, L, n).astype(np.int32))
    changed = [int(ctx.expand_alpha(lam, h, alpha)) for alpha in range(L)]
    rec["single_moves"] = {"labels": sha(ctx.get_labels()), "energy_q": int(ctx.energy(lam, h)[0]), "changed": changed, **_counters(ctx)}
    return rec


def _run_cut(ctx, name):
    from pyprogressivex import _lib
    pts, model, T2 = problem(name)
    ctx.set_points(_lib.LINE2D, pts)
    ctx.graph_build(pts, _lib.GRAPH_KNN, k=3, fetch=False)   # (k = 3: the pairwise term moves some flags but not all - with 6 neighbours lambda 0.3 pulls every point in)
    before = ctx.expansion_paths()
    flags = ctx.gc_labeling(model, T2, 0.3)
    index = ctx.gc_inliers(model, T2, 0.3)
    after = ctx.expansion_paths()
    return {"flags": sha(flags), "count": int(flags.sum()), "index": sha(index), "index_count": int(index.shape[0]),
            "paths": {k: after[k] - before[k] for k in after}, "launches": ctx.one_workgroup_launches()}


def run_case(case_id):
    """the record of one case, from a fresh context created under the case's switches (they are read when a context is created)"""
    from pyprogressivex import _lib
    kind, name, env = cases()[case_id]
    with _environment(env):
        ctx = _lib.Context(0)
    try:
        return _run_expansion(ctx, name) if kind == "expansion" else _run_cut(ctx, name)
    finally:
        ctx.close()


def must_keep(field):
    """fields the generator may not drop, whatever two runs of one commit say: what a case computed and which solver computed it"""
    leaf = field.rsplit(".", 1)[-1]
    return leaf in ("labels", "energy_q", "cycles", "flags", "count", "index") or ".paths." in f".{field}"


def flatten(rec, prefix=""):
    """{"a.b.c": leaf} of a nested record: the unit in which the generator keeps or drops fields and the replay compares them"""
    out = {}
    for k, v in rec.items():
        if isinstance(v, dict):
            out.update(flatten(v, f"{prefix}{k}."))
        else:
            out[f"{prefix}{k}"] = v
    return out
