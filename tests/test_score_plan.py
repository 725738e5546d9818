"""csrc/score_plan.h (compiled into tests/emu/libmf_emu.so exactly as libpgx.so compiles it) against what it replaced.

plan_score: before it, what a scoring launch looks like - path, filter level, guards, chunking, the group-major geometry, the
fixed-point scale, whether the mirror is written - was decided over 130 lines of score.hip score_dispatch and score_launch, between
the launches.  parent_plan() below copies those decisions as they stood at commit c168894, each line with its file:line, redundant
terms included; every output field is compared on every point of the grids, doubles by their bits.  None is skipped.

ScoreBatch: the batch and the last launch's results were sixteen loose pgx_ctx fields written from four files.  ParentFields below
replays the parent's writes, event by event, refused and failed calls included; seeded random scripts run on both and every
question must get the same answer after every event - except where this file says otherwise, and says what the answer is now."""
import ctypes as C
import itertools
import math
import struct

import numpy as np

from test_emu import emu  # noqa: F401  (the fixture that builds and loads libmf_emu.so)

BOX, BOXALL, BALL, VANISHING = 0, 1, 2, 3          # score_plan.h GroupBound
# name: (Filter<MT>::enabled, Filter32<MT>::enabled, Residual<MT>::bound, Filter32<MT> derives from Filter32<kHomography>)
#   score_filters.hip.h:31,39,64,91 (Filter) and :128,172,250,331,410,469,518 + 566-567,614 + 663 (Filter32); residuals.hip.h:48,63,80,103,121,138,158,174 (bound)
TYPES = {"line": (0, 1, BALL, 0), "homography": (1, 1, BOX, 1), "fundamental": (0, 1, BOXALL, 0), "pnp": (1, 1, BOX, 0),
         "vanishing_point": (0, 1, VANISHING, 0), "homography_sym": (1, 1, BOX, 1), "plane": (0, 1, BALL, 0), "sphere": (0, 1, BALL, 0)}
K_SUPER = 8                 # pgx_internal.h:208
K_SCORE_BLOCK = 256         # score.hip:25
OUT_L = ("path", "filter", "chunk", "chunks", "words", "groups", "cull_segs", "gps", "W", "group_xcd", "nrep", "split", "gblocks",
         "zero_words", "dense_min", "counters", "verify", "mirror")
OUT_D = ("guard", "guard32", "qscale")


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 or x != x else math.nan      # std::sqrt of a negative number is NaN, not an exception


def parent_plan(name, sw, cu_count, n, M, Mpad, ordered, point_sort, T2, umax, fscale, global_n, want_masks, score_stats, blocks_per_cu):
    """score.hip score_launch (:990) and score_dispatch<MT> (:673) of the parent; sw = the pgx_ctx switch fields by their old names"""
    f64_enabled, f32_enabled, bound, homography = TYPES[name]
    out = dict.fromkeys(OUT_L + OUT_D, 0)
    out.update(guard=0.0, guard32=0.0, qscale=0.0)
    # ---- score_launch
    groups = Mpad // K_SCORE_BLOCK                                                  # score.hip:995
    if groups == 0:      # (no Mpad below 256 ever reached this line - capi.hip:442 and solve.hip:570 round up - and it divided by zero there;
        groups = 1       #  the grid goes below for W = 1: the planner counts one block)
    target_blocks = (cu_count if cu_count > 0 else 256) * blocks_per_cu            # score.hip:998
    chunks = (target_blocks + groups - 1) // groups                                # score.hip:999
    chunk = (n + chunks - 1) // chunks                                             # score.hip:1000
    chunk = ((chunk + 63) // 64) * 64                                              # score.hip:1001
    if chunk < 64:                                                                 # score.hip:1002
        chunk = 64
    if chunk > 65472:                                                              # score.hip:1003
        chunk = 65472
    chunks = (n + chunk - 1) // chunk                                              # score.hip:1004
    if chunks > 65535:                                                             # score.hip:1005
        chunks = 65535                                                             # score.hip:1006
        chunk = (((n + chunks - 1) // chunks + 63) // 64) * 64                     # score.hip:1007
        chunks = (n + chunk - 1) // chunk                                          # score.hip:1008
    out["chunk"], out["chunks"], out["words"] = chunk, chunks, (n + 63) // 64     # score.hip:1010-1012
    # ---- score_dispatch<MT>
    T = _sqrt(T2)                                                                  # score.hip:676
    guard = 0.0                                                                    # score.hip:677
    filt = bool(f64_enabled and sw["filter_enabled"] and T > 0.0 and math.isfinite(T) and math.isfinite(umax) and
                umax <= T * 268435456.0)                                           # score.hip:678-679
    if filt:
        guard = 4.5 * 1.1102230246251565e-16 * (1.0 + umax + T) * 16777216.0 / T   # score.hip:681
        filt = math.isfinite(guard)                                                # score.hip:682
    guard32 = 0.0                                                                  # score.hip:685
    filt32 = bool(filt and sw["filter_enabled"] == 1 and umax <= T * 16384.0)      # score.hip:686
    if filt32:
        guard32 = 5.5 * 5.9604644775390625e-8 * (1.0 + umax + T) * 1024.0 / T      # score.hip:688
        filt32 = math.isfinite(guard32) and guard32 < 1e30                         # score.hip:689
    if bound == VANISHING:                                                         # score.hip:691
        filt32 = bool(sw["filter_enabled"] == 1 and T > 0.0 and math.isfinite(T) and T2 < 1e30)   # score.hip:692
    if homography:                                                                 # score.hip:693
        filt32 = bool(sw["filter_enabled"] == 1 and T2 > 1e-24 and T2 < 1e24)      # score.hip:694
    if bound == BALL:                                                              # score.hip:695
        filt32 = bool(sw["filter_enabled"] == 1 and T2 > 1e-24 and T2 < 1e24 and math.isfinite(fscale))   # score.hip:696
        guard32 = fscale                                                           # score.hip:697
    if bound == BOXALL:                                                            # score.hip:699
        filt32 = bool(sw["filter_enabled"] == 1 and T2 > 1e-12 and T2 < 1e12 and math.isfinite(fscale))   # score.hip:700
        guard32 = fscale * fscale                                                  # score.hip:701
    if not (fscale <= 1e30):                                                       # score.hip:705
        filt = filt32 = False
    out["filter"] = 2 if filt32 else (1 if filt else 0)                            # score.hip:706
    out["guard"], out["guard32"] = guard, guard32
    out["path"] = 1                                                                # score.hip:805
    if f32_enabled:                                                                # score.hip:707
        if filt32 and point_sort and sw["score_cull"]:                             # score.hip:708
            groups = (n + 63) // 64                                                # score.hip:710
            segs = sw["score_cull_segs"]                                           # score.hip:711
            gps = ((groups + segs - 1) // segs + K_SUPER - 1) // K_SUPER * K_SUPER # score.hip:712
            W = Mpad // 64                                                         # score.hip:713
            group_xcd = sw["score_group_xcd"] if sw["score_group_xcd"] >= 0 else (1 if ordered else 0)   # score.hip:720 (h_perm.empty() ? 0 : 1)
            nrep = sw["score_nrep"] if sw["score_nrep"] > 0 else (8 if group_xcd else 1)                 # score.hip:721
            xcd_local = 1 if group_xcd else 0                                      # score.hip:722
            lg = 0                                                                 # score.hip:729
            n_scale = global_n if global_n > n else n                              # score.hip:730
            while (1 << lg) < n_scale + 1:                                         # score.hip:731
                lg += 1
            qscale = math.ldexp(1.0, 62 - lg if 62 - lg < 50 else 50)              # score.hip:732
            zero_words = nrep * Mpad * 3                                           # score.hip:734
            split_cfg = sw["score_split"] if sw["score_split"] > 0 else (
                5 if (group_xcd or name == "pnp") else (16 if name in ("vanishing_point", "fundamental") else 8))   # score.hip:749-750
            split = split_cfg if split_cfg < W else W                              # score.hip:751
            gblocks = ((groups + 7) // 8) * 8 * split if (xcd_local & 1) else groups * split   # score.hip:752
            if want_masks:                                                         # score.hip:753
                dense, counters = 65, 0                                            # score.hip:759
            elif score_stats:                                                      # score.hip:760
                dense, counters = sw["score_dense_min"], 1                         # score.hip:767
            else:
                dense, counters = sw["score_dense_min"], 0                         # score.hip:777
            verify = 1 if (counters and sw["verify"]) else 0                       # score.hip:768
            mirror = 1 if (sw["score_mirror"] and not want_masks) else 0           # score.hip:783, :798
            out.update(path=2, groups=groups, cull_segs=segs, gps=gps, W=W, group_xcd=group_xcd, nrep=nrep, split=split,   # score.hip:801
                       gblocks=gblocks % 2 ** 32, zero_words=zero_words, dense_min=dense, counters=counters, verify=verify, mirror=mirror, qscale=qscale)
    return out


def _plan(emu, name, sw, cu_count, n, M, Mpad, ordered, point_sort, T2, umax, fscale, global_n, want_masks, counters, blocks_per_cu, traits=None):  # noqa: F811
    tr = TYPES[name] if traits is None else traits
    in_i = np.array(list(tr) + [sw["filter_enabled"], sw["score_cull"], sw["score_mirror"], sw["verify"], sw["score_split"], sw["score_group_xcd"],
                                sw["score_nrep"], sw["score_dense_min"], sw["score_cull_segs"], cu_count, M, Mpad, int(ordered), int(point_sort),
                                int(want_masks), int(counters), blocks_per_cu], np.int32)
    in_l = np.array([n, global_n], np.int64)
    in_d = np.array([T2, umax, fscale], np.float64)
    out_l, out_d = np.zeros(18, np.int64), np.zeros(3, np.float64)
    emu.emu_plan_score(in_i.ctypes.data_as(C.POINTER(C.c_int32)), in_l.ctypes.data_as(C.POINTER(C.c_int64)), in_d.ctypes.data_as(C.POINTER(C.c_double)),
                       out_l.ctypes.data_as(C.POINTER(C.c_int64)), out_d.ctypes.data_as(C.POINTER(C.c_double)))
    got = dict(zip(OUT_L, (int(v) for v in out_l)))
    got.update(zip(OUT_D, (float(v) for v in out_d)))
    return got


def _bits(x):
    return struct.pack("<d", x)


def _compare(got, want, where):
    for k in OUT_L:
        assert got[k] == want[k], (k, got[k], want[k], where)
    for k in OUT_D:
        assert _bits(got[k]) == _bits(want[k]), (k, got[k], want[k], where)


DEFAULT_SW = dict(filter_enabled=1, score_cull=1, score_mirror=1, verify=0, score_split=0, score_group_xcd=-1, score_nrep=0, score_dense_min=32,
                  score_cull_segs=256)
NS = (1, 63, 64, 65, 511, 512, 513, 4096, 10 ** 6, 2 ** 31 - 1)
MS = (1, 64, 65, 256, 257, 2048)
UP, DOWN = math.inf, -math.inf


def _around(x):
    return (math.nextafter(x, DOWN), x, math.nextafter(x, UP))


def test_filter_level_and_path_are_the_parents_on_the_whole_grid(emu):  # noqa: F811
    """every term of the filter predicates and of the path predicate, both sides: the eight types (and a type without an f32 filter),
    PGX_NO_FILTER 0 / 1 / 2, cull, sorted points, masks, counters, PGX_VERIFY, mirror, and T2 / umax / fscale one step inside and
    outside every window, plus 0, inf and NaN"""
    t2s = (0.0, -1.0, math.inf, math.nan, 1.0) + _around(1e-24) + _around(1e-12) + _around(1e12) + _around(1e24) + _around(1e30)
    T2, T = 4.0, 2.0
    umaxs = (0.0, math.inf, math.nan) + _around(T * 16384.0) + _around(T * 268435456.0)
    fscales = (1.0, math.inf, math.nan) + _around(1e30)
    floats = [(t2, 1.0, fs) for t2 in t2s for fs in (1.0, math.nextafter(1e30, UP))] + [(T2, um, fs) for um in umaxs for fs in fscales]
    # umax against a T2 whose guards overflow or vanish: the isfinite(guard) terms
    floats += [(1e-320, 1e-320, 1.0), (5e-324, 0.0, 1.0), (1e300, 1e300, 1.0), (1e-300, 1e-140, 1.0)]
    points = 0
    for name, fe, cull, srt, (masks, counters, verify, mirror), (t2, um, fs) in itertools.product(
            TYPES, (0, 1, 2), (0, 1), (0, 1), ((0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1), (0, 1, 1, 0), (1, 1, 1, 0)), floats):
        sw = dict(DEFAULT_SW, filter_enabled=fe, score_cull=cull, verify=verify, score_mirror=mirror)
        args = (name, sw, 256, 4097, 257, 512, True, bool(srt), t2, um, fs, 0, bool(masks), bool(counters), 64)
        _compare(_plan(emu, *args), parent_plan(*args), args)
        points += 1
    assert points == len(TYPES) * 3 * 2 * 2 * 5 * len(floats) and len(floats) == 2 * len(t2s) + len(umaxs) * len(fscales) + 4
    # a type without an f32 filter never leaves the chunked path (score.hip:707 `if constexpr (Filter32<MT>::enabled)`): no such type exists
    # today, so the transcription is told through a ninth table entry
    TYPES["no_f32"] = (1, 0, BOX, 0)
    try:
        for fe, srt, (t2, um, fs) in itertools.product((0, 1, 2), (0, 1), floats):
            args = ("no_f32", dict(DEFAULT_SW, filter_enabled=fe), 256, 4097, 257, 512, True, bool(srt), t2, um, fs, 0, False, False, 64)
            got = _plan(emu, *args)
            _compare(got, parent_plan(*args), args)
            assert got["path"] == 1
            points += 1
    finally:
        del TYPES["no_f32"]
    assert points == (len(TYPES) * 3 * 2 * 2 * 5 + 3 * 2) * len(floats)


def test_launch_geometry_is_the_parents_on_the_whole_grid(emu):  # noqa: F811
    """the group-major geometry and the chunking: group_xcd -1 / 0 / 1 x ordered or not, nrep 0 / 8 / 16, split 0 / 3 / 16 against
    W = 1, 4, 5, 32, cull_segs 1 / 256 / 65535, blocks_per_cu 1 / 64, every n (which crosses the 65 472 and 65 535 clamps), every M,
    score_global_n 0 / n / 5e7, on every type (the automatic split is per type), with the cull on and off (both paths' fields)"""
    mpads = {1: (64, 256), 64: (64, 256), 65: (256, 320), 256: (256,), 257: (320, 512), 2048: (2048,)}     # W = Mpad / 64 = 1, 4, 5, 8, 32
    points = 0
    # (a) everything that meets in one expression is crossed: (group_xcd, ordered, nrep, split, type, Mpad, n), and (n, cull_segs)
    for name, gx, ordered, nrep, split, M, n in itertools.product(TYPES, (-1, 0, 1), (False, True), (0, 8, 16), (0, 3, 16), MS, NS):
        for Mpad in mpads[M]:
            sw = dict(DEFAULT_SW, score_group_xcd=gx, score_nrep=nrep, score_split=split)
            args = (name, sw, 256, n, M, Mpad, ordered, True, 1.0, 1.0, 1.0, 0, False, False, 64)
            got = _plan(emu, *args)
            _compare(got, parent_plan(*args), args)
            assert got["path"] == 2
            points += 1
    want = len(TYPES) * 3 * 2 * 3 * 3 * len(NS) * sum(len(v) for v in mpads.values())
    for name, n, segs in itertools.product(TYPES, NS, (1, 256, 65535)):
        args = (name, dict(DEFAULT_SW, score_cull_segs=segs), 256, n, 257, 512, True, True, 1.0, 1.0, 1.0, 0, False, False, 64)
        _compare(_plan(emu, *args), parent_plan(*args), args)
        points += 1
    want += len(TYPES) * len(NS) * 3
    assert points == want
    # (b) the chunking and the fixed-point scale: (n, Mpad, cu_count, blocks_per_cu) and (n, score_global_n), on both paths
    for n, M, cu, bpc, gn, cull, dense in itertools.product(NS, MS, (0, 1, 256, 304), (1, 64), (0, "n", 5 * 10 ** 7), (0, 1), (1, 32, 65)):
        for Mpad in mpads[M]:
            if Mpad % K_SCORE_BLOCK:
                continue        # (the chunked kernel's grid divides by Mpad / 256: Mpad is a multiple of 256 wherever it runs; counted below)
            sw = dict(DEFAULT_SW, score_cull=cull, score_dense_min=dense)
            args = ("pnp", sw, cu, n, M, Mpad, False, True, 1.0, 1.0, 1.0, n if gn == "n" else gn, False, False, bpc)
            _compare(_plan(emu, *args), parent_plan(*args), args)
            points += 1
    pads_256 = sum(1 for v in mpads.values() for p in v if p % K_SCORE_BLOCK == 0)
    assert points == want + len(NS) * 4 * 2 * 3 * 2 * 3 * pads_256


# ---- ScoreBatch against the parent's field writes ----------------------------------------------------------------------------------
class ParentFields:
    """the sixteen pgx_ctx fields at c168894 and every write to them"""

    def __init__(self):
        self.M = self.Mpad = 0                       # pgx_internal.h:80
        self.words = 0                               # pgx_internal.h:81
        self.have_masks = False                      # pgx_internal.h:82
        self.score_has_compound = 0                  # pgx_internal.h:83
        self.last_score_filtered = self.last_score_path = 0   # pgx_internal.h:50-51
        self.last_acc, self.last_nrep, self.last_qscale = 0, 0, 0.0   # pgx_internal.h:86-88
        self.last_acc_M = self.last_acc_Mpad = 0     # pgx_internal.h:89
        self.mirror_valid = 0                        # pgx_internal.h:163
        self.h_perm = []                             # pgx_internal.h:165
        self.counts_p = False                        # ctx->counts.p: allocated by the first accepted launch (score.hip:1019), never released
        self.n = 0                                   # points resident (the refusals read it)

    def set_points(self, ok):
        self.M = 0; self.last_acc = 0                # capi.hip:324  # noqa: E702
        self.n = 1 if ok else 0                      # capi.hip:323, :331
        if not ok:
            self.mirror_valid = 0                    # capi.hip:331

    def upload(self, M, perm, outcome):              # outcome: "ok" | "refused" | "failed"
        if self.n <= 0 or M <= 0 or outcome == "refused":   # capi.hip:428-429
            return
        self.mirror_valid = 0                        # capi.hip:433
        self.h_perm = list(perm) if perm is not None else []   # capi.hip:440-441
        self.Mpad = (M + 255) // 256 * 256           # capi.hip:442
        if outcome == "failed":                      # capi.hip:447-467: hipHostMalloc, ensure, hipMemcpyAsync
            return
        self.M = M; self.last_acc = 0                # capi.hip:469  # noqa: E702

    def generate(self, M, outcome):
        if self.n <= 0 or outcome == "refused":      # solve.hip:552-561
            return
        self.h_perm = []                             # solve.hip:567
        self.mirror_valid = 0                        # solve.hip:568
        self.Mpad = (M + 255) // 256 * 256           # solve.hip:570
        if outcome == "failed":                      # solve.hip:571-591
            return
        self.M = M; self.last_acc = 0                # solve.hip:593  # noqa: E702

    def launch(self, plan, has_compound, masks, acc, outcome):
        self.score_has_compound = int(has_compound)  # capi.hip:502 / :671 - before the request is looked at
        self.mirror_valid = 0                        # score.hip:992
        if self.n <= 0 or self.M <= 0:               # score.hip:993-994
            return False
        self.words = plan["words"]                   # score.hip:1012
        if outcome == "failed":                      # score.hip:1014: the first allocation of the launch
            return True
        self.counts_p = True                         # score.hip:1019
        self.have_masks = bool(masks)                # score.hip:1024
        self.last_score_filtered = plan["filter"]    # score.hip:706
        if plan["path"] == 2:
            self.mirror_valid = plan["mirror"]       # score.hip:798
            self.last_acc, self.last_nrep, self.last_qscale = acc, plan["nrep"], plan["qscale"]   # score.hip:799
            self.last_acc_M, self.last_acc_Mpad = self.M, self.Mpad
            self.last_score_path = 2                 # score.hip:801
        else:
            self.last_score_path = 1                 # score.hip:805
            self.last_acc = 0                        # score.hip:806
        return True

    def reduced(self):
        self.mirror_valid = 0                        # comm.hip:358

    # ---- what the entry points answered
    def fetchable(self):
        return self.M > 0 and self.counts_p          # capi.hip:527, comm.hip:189, :233, :343

    def fetch_source(self):
        return "mirror" if self.mirror_valid else "device"     # capi.hip:539 (the capacity term holds whenever the flag does)

    def fetch_order(self):
        return list(self.h_perm[:self.M]) if len(self.h_perm) >= self.M else None     # capi.hip:552

    def mask_rows(self):
        return self.have_masks and self.M > 0        # pointwise.hip:400

    def acc_exportable(self):
        return bool(self.last_acc != 0 and self.last_score_path == 2 and self.last_acc_M == self.M and self.last_acc_Mpad == self.Mpad)   # comm.hip:320


READY, NONE, CHANGED = 0, 1, 2


def _query(emu, h):  # noqa: F811
    out, perm = np.zeros(15, np.int64), np.zeros(4096, np.int32)
    emu.emu_batch_query.restype = C.c_double
    q = emu.emu_batch_query(C.c_void_p(h), out.ctypes.data_as(C.POINTER(C.c_int64)), perm.ctypes.data_as(C.POINTER(C.c_int32)))
    keys = ("table", "mask_rows", "from_mirror", "ordered", "acc_exportable", "acc_stale", "M", "Mpad", "has_compound", "masks", "words", "path",
            "filter", "nrep", "acc")
    got = dict(zip(keys, (int(v) for v in out)))
    got["qscale"] = q
    got["perm"] = [int(v) for v in perm[:got["M"]]] if got["ordered"] else None
    return got


def _event(emu, h, event, a=0, b=0, perm=None, plan=None, acc=0, q=0.0):  # noqa: F811
    pl = np.array(plan if plan is not None else [0] * 5, np.int64)
    pm = None if perm is None else np.array(perm, np.int32)
    emu.emu_batch_event(C.c_void_p(h), C.c_int(event), C.c_int(a), C.c_int(b), None if pm is None else pm.ctypes.data_as(C.POINTER(C.c_int32)),
                        pl.ctypes.data_as(C.POINTER(C.c_int64)), C.c_uint64(acc), C.c_double(q))


def test_the_batch_owner_answers_as_the_parents_fields_did(emu):  # noqa: F811
    emu.emu_batch_new.restype = C.c_void_p
    steps = deliberate = failed_uploads = flag_cases = 0
    kinds = set()
    for seed in range(300):
        rng = np.random.default_rng(seed)
        h = emu.emu_batch_new()
        par = ParentFields()
        launched_batch = None      # what this file keeps to STATE the new answers: the batch id the last accepted launch scored ...
        batch_id = 0               # ... and the resident one's (every accepted change of the batch or the points is a new one)
        untouched = None           # set by a failed upload / solve: the owner's answers from before it
        words = 0
        flag_diverged = False      # a refused or failed launch wrote the parent's compound flag (capi.hip:502); the owner keeps the launch's
        for _ in range(40):
            kind = rng.choice(["points", "points_failed", "upload", "upload", "upload_refused", "upload_failed", "generate", "generate_refused",
                               "generate_failed", "launch", "launch", "launch", "launch_failed", "reduce"])
            kinds.add(str(kind))
            before = _query(emu, h)
            if kind in ("points", "points_failed"):
                par.set_points(kind == "points")
                words = int(rng.integers(1, 70))       # (n + 63) / 64 of these points: every launch on them writes the same
                _event(emu, h, 0)
                batch_id += 1
                untouched = None
            elif kind.startswith("upload"):
                M = 0 if kind == "upload_refused" else int(rng.choice([1, 64, 65, 256, 257, 700]))
                perm = [int(v) for v in rng.permutation(M)] if M > 64 and rng.random() < 0.6 else None
                outcome = kind.partition("_")[2] or "ok"
                accepted = par.n > 0 and M > 0
                par.upload(M, perm, outcome)
                if accepted and outcome == "ok":
                    _event(emu, h, 1, M, (M + 255) // 256 * 256, perm)
                    batch_id += 1
                    untouched = None
                elif accepted and outcome == "failed":
                    untouched = before
                    failed_uploads += 1
            elif kind.startswith("generate"):
                M = int(rng.choice([1, 3, 64, 192, 300]))
                outcome = kind.partition("_")[2] or "ok"
                accepted = par.n > 0 and outcome != "refused"
                par.generate(M, outcome)
                if accepted and outcome == "ok":
                    _event(emu, h, 2, M, (M + 255) // 256 * 256)
                    batch_id += 1
                    untouched = None
                elif accepted and outcome == "failed":
                    untouched = before
                    failed_uploads += 1
            elif kind.startswith("launch"):
                if untouched is not None:
                    continue       # (after a failed upload the parent's M and Mpad are of two batches: what it launched then is not modelled)
                path = int(rng.choice([1, 2]))
                masks = bool(rng.random() < 0.4)
                plan = dict(path=path, filter=int(rng.choice([0, 1, 2])) if path == 1 else 2, words=words,
                            nrep=int(rng.choice([1, 8, 16])) if path == 2 else 0, mirror=int(path == 2 and not masks and rng.random() < 0.8),
                            qscale=math.ldexp(1.0, int(rng.integers(30, 51))) if path == 2 else 0.0)
                has_compound, acc = bool(rng.random() < 0.5), int(rng.integers(1, 2 ** 40)) * 8
                outcome = "failed" if kind == "launch_failed" else "ok"
                accepted = par.launch(plan, has_compound, masks, acc, outcome)
                if accepted and outcome == "ok":
                    _event(emu, h, 3, int(has_compound), int(masks), None, [plan["path"], plan["filter"], plan["words"], plan["nrep"], plan["mirror"]],
                           acc, plan["qscale"])
                    launched_batch = batch_id
                    flag_diverged = False
                else:
                    if accepted:
                        _event(emu, h, 4)
                    flag_diverged = flag_diverged or int(has_compound) != before["has_compound"]
            else:
                if not (par.acc_exportable() and before["acc_exportable"]):
                    continue       # pgx_score_allreduce replaces the table only when every rank exported its accumulators
                par.reduced()
                _event(emu, h, 5)
            got = _query(emu, h)
            steps += 1
            if untouched is not None:
                # NEW ANSWER (a failed upload / solve): the parent had written Mpad and the order of the batch that never arrived and kept
                # M of the old one.  The owner's records are exactly what they were before the call.
                assert got == untouched
                continue
            current = launched_batch == batch_id
            assert got["M"] == par.M and (par.M == 0 or got["Mpad"] == par.Mpad)
            assert (got["table"] == NONE) == (not par.fetchable())
            if par.fetchable() and not current:
                # NEW ANSWER (the one deliberate change): the parent handed out the old launch's rows, cut or padded to the new M and
                # un-permuted by the new order; the owner says the batch changed - for the table, the mask rows and the accumulators
                assert got["table"] == CHANGED and got["mask_rows"] in (CHANGED, NONE) and not got["acc_exportable"]
                assert (got["mask_rows"] == CHANGED) == par.have_masks
                deliberate += 1
            elif par.fetchable():
                assert got["table"] == READY
                assert ("mirror" if got["from_mirror"] else "device") == par.fetch_source()
                assert got["perm"] == par.fetch_order()
                assert (got["mask_rows"] == READY) == par.mask_rows() and got["mask_rows"] != CHANGED
                assert bool(got["masks"]) == par.have_masks and got["words"] == par.words
                assert bool(got["acc_exportable"]) == par.acc_exportable() and not got["acc_stale"]
                if got["acc_exportable"]:
                    assert (got["acc"], got["nrep"]) == (par.last_acc, par.last_nrep) and _bits(got["qscale"]) == _bits(par.last_qscale)
                if flag_diverged:
                    # NEW ANSWER: a refused or failed launch after this one wrote ITS compound flag into the parent's field, and the
                    # next fetch applied it to this launch's table; the owner keeps the flag of the launch that produced the table
                    flag_cases += 1
                else:
                    assert got["has_compound"] == par.score_has_compound
            else:
                assert got["mask_rows"] == NONE and not got["acc_exportable"] and not par.acc_exportable()
            # pgx_score_stats, pgx_score_kernel_times: path and filter level of the last accepted launch, whatever happened since
            assert (got["path"], got["filter"]) == (par.last_score_path, par.last_score_filtered)
        emu.emu_batch_free(C.c_void_p(h))
    assert steps > 8000 and deliberate > 500 and failed_uploads > 300 and flag_cases > 10
    assert len(kinds) == 11
