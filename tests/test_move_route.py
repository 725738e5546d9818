"""The planner of csrc/move_route.h (compiled into tests/emu/libmf_emu.so exactly as libpgx.so compiles it) against a transcription
of the predicates it replaced.  Before it, "which min-cut solver takes this move, which follows, is the cycle batched" was spelled out
in five places of three files that had to agree; the transcription below copies each of them as it stood at commit 3624eec, with
its file:line, redundant terms included.  Every point of the grid is compared - none is skipped."""
import ctypes as C
import itertools

import numpy as np

from test_emu import emu  # noqa: F401  (the fixture that builds and loads libmf_emu.so)

TILE, REGION, LEVEL = 1, 2, 3            # move_route.h Solver
CYCLE, SINGLE, CUT = 0, 1, 2             # move_route.h MoveKind
TILE_SINGLE_MAX = 8192                   # pgx_internal.h:153 `int tile_single_max = 8192;` (no setter, no environment switch)

NS = (1, 1024, 1025, 4096, 8192, 8193, 300000, 2 ** 30 - 1, 2 ** 30)
DEGREES = (0, 1, 32, 33)
EXPANSION_MAX = (0, 1024, 8192)


def region_moves_apply(mf_region, max_degree, L, gn):
    # maxflow.hip:1178  return ctx->mf_region && ctx->max_degree >= 1 && ctx->max_degree <= 32 && ctx->L <= 64 && ctx->gn < ((int64_t)1 << 30);
    return bool(mf_region and max_degree >= 1 and max_degree <= 32 and L <= 64 and gn < (1 << 30))


def parent_order(mf_tile, mf_region, tem, n, L, max_degree, gn, wq, source_reach):
    """the solvers maxflow.hip expand_alpha_on tried, in its order"""
    order = []
    # maxflow_tile.hip:1477  if (n > ctx->tile_single_max || n > 8192 || L > kMaxL) ... return PGX_TILE_FALLBACK;      (kMaxL = 64)
    tile_refuses = n > TILE_SINGLE_MAX or n > 8192 or L > 64
    # maxflow_tile.hip:1574  if (stride < 1 || stride > 32 || mv.L > kMaxL || n >= ((int64_t)1 << 30)) return PGX_TILE_FALLBACK;
    region_refuses = max_degree < 1 or max_degree > 32 or L > 64 or n >= (1 << 30)
    pair = True    # maxflow.hip:1187  const bool pair = true;
    # maxflow.hip:1193  region_first = !source_reach && wq == nullptr && L <= 64 && n > ctx->tile_expansion_max && region_moves_apply(ctx);
    region_first = (not source_reach) and (not wq) and L <= 64 and n > tem and region_moves_apply(mf_region, max_degree, L, gn)
    # maxflow.hip:1194  if (ctx->mf_tile && !source_reach && n <= ctx->tile_single_max && n <= 8192 && L <= 64 && !region_first)
    if mf_tile and not source_reach and n <= TILE_SINGLE_MAX and n <= 8192 and L <= 64 and not region_first:
        assert not tile_refuses        # (the callee's guard was dead code behind the caller's test)
        order.append(TILE)
    # maxflow.hip:1288  if (!source_reach && wq == nullptr && pair && L <= 64 && region_moves_apply(ctx))
    if not source_reach and not wq and pair and L <= 64 and region_moves_apply(mf_region, max_degree, L, gn):
        assert not region_refuses
        order.append(REGION)
        # maxflow.hip:1291  if (region_first && ctx->mf_tile && n <= ctx->tile_single_max && n <= 8192)
        if region_first and mf_tile and n <= TILE_SINGLE_MAX and n <= 8192:
            assert not tile_refuses
            order.append(TILE)
    order.append(LEVEL)    # maxflow.hip:1298  mf_expand_alpha(be, v, tune, changed, ctx->stats)
    return order


def parent_route(mf_tile, mf_tile_batch, mf_region, gc_flip, tem, n, max_degree, gn, kind, declined):
    """(order, flip, batched) as the three files decided them"""
    if declined:
        mf_region = 0      # capi.hip:1111-1114  the move a batch declined is run again with ctx->mf_region = 0 ...
    if kind == CUT:
        L = 2              # pointwise.hip:355  expand_alpha_on(ctx, n, 2, dq, labels, wq, lambda_q, 0, flip ? 1 : 0, &changed, flip)
        # pointwise.hip:345  flip = ctx->gc_flip != 0 && !(ctx->mf_tile && n <= ctx->tile_single_max && n <= 8192);
        flip = bool(gc_flip != 0 and not (mf_tile and n <= TILE_SINGLE_MAX and n <= 8192))
        return parent_order(mf_tile, mf_region, tem, n, L, max_degree, gn, wq=True, source_reach=flip), flip, False
    L = 64                 # maxflow.hip:1168  expand_alpha_launch refuses L > kMfMaxLabels (64) before it routes
    order = parent_order(mf_tile, mf_region, tem, n, L, max_degree, gn, wq=False, source_reach=False)   # maxflow.hip:1171
    batched = False        # capi.hip:961  pgx_expand_alpha: region_defer is 0;  capi.hip:1091  ... and 0 again for the re-run of :1113
    if kind == CYCLE and not declined:
        dq_n = n           # maxflow.hip:1188  expand_alpha_on insists on ctx->gn == n
        # capi.hip:1069  (ctx->mf_tile && ctx->mf_tile_batch && ctx->dq_n <= ctx->tile_single_max && ctx->dq_n <= 8192 && ctx->L <= 64) ||
        # capi.hip:1070  (region_moves_apply(ctx) && !(ctx->mf_tile && ctx->dq_n <= ctx->tile_single_max && ctx->dq_n <= ctx->tile_expansion_max))
        batched = bool((mf_tile and mf_tile_batch and dq_n <= TILE_SINGLE_MAX and dq_n <= 8192 and L <= 64) or
                       (region_moves_apply(mf_region, max_degree, L, gn) and not (mf_tile and dq_n <= TILE_SINGLE_MAX and dq_n <= tem)))
    return order, False, batched


def test_planner_is_the_parents_predicates_on_the_whole_grid(emu):  # noqa: F811
    out = np.zeros(5, np.int32)
    points = 0
    for n, deg, (tile, batch, region, flip), tem, kind, declined in itertools.product(
            NS, DEGREES, itertools.product((0, 1), repeat=4), EXPANSION_MAX, (CYCLE, SINGLE, CUT), (False, True)):
        emu.emu_plan_move(C.c_int(tile), C.c_int(batch), C.c_int(region), C.c_int(flip), C.c_int(tem), C.c_int64(n), C.c_int(deg),
                          C.c_int64(n), C.c_int(kind), C.c_int(int(declined)), out.ctypes.data_as(C.POINTER(C.c_int32)))
        got_order = [int(s) for s in out[:3] if s != 0]
        want_order, want_flip, want_batched = parent_route(tile, batch, region, flip, tem, n, deg, n, kind, declined)
        where = dict(n=n, max_degree=deg, mf_tile=tile, mf_tile_batch=batch, mf_region=region, gc_flip=flip, tile_expansion_max=tem,
                     kind=kind, declined=declined)
        assert got_order[0] == want_order[0], where
        assert got_order == want_order, where
        assert list(out[:3]) == got_order + [0] * (3 - len(got_order)), where      # no hole in the list
        assert bool(out[3]) == want_flip, where
        assert bool(out[4]) == want_batched, where
        # what "pgx_expansion: a batched move was not enqueued" guarded at run time: only the one-workgroup solvers can be enqueued
        assert not out[4] or got_order[0] in (TILE, REGION), where
        assert got_order[-1] == LEVEL and len(set(got_order)) == len(got_order), where
        if kind == CUT:
            assert REGION not in got_order and (not out[3] or got_order == [LEVEL]), where
        points += 1
    assert points == len(NS) * len(DEGREES) * 16 * len(EXPANSION_MAX) * 3 * 2
