"""The cases behind tests/golden/kat_reductions_v1.npz: every Gram and residual-sum reduction pass of csrc/fit.hip and
csrc/pointwise.hip at the sizes where its trees change shape, recorded bit for bit on an MI355X at the commit before the passes were
written once (tests/golden/make_golden_reductions.py) and replayed by tests/test_gpu_reductions.py.

run(ctx) makes every call and returns (floats, ints, calls, digest): per group one concatenated float64 and one int64 array, the
list of (call, number of floats, number of ints) that says which slice belongs to which call, and the SHA-256 of every input array
in the order of use (numpy does not promise a stable Generator stream across versions: a digest mismatch means the inputs moved,
not the kernels).  The file holds the outputs only.

Sizes.  Block passes (pgx_gram, pgx_gram_labels: 256 points per block, 4 waves; final pass 16 lanes per value): n = 1, 64, 65 (a
second wave), 257 (a second block), 4097 (17 blocks: past the final pass's stride).  Residual sums (final pass 256 threads):
n = 65 537 too (257 blocks).  Labels: K = 3 with label 1 empty and label 3 the outlier label, and K = 1.  Index lists: m = 0, 1, 257
(one index repeated), and every point once at n = 4097.  Weights: none / power 1 / power 2, all three at n = 257 and one of them
in turn at the other sizes.  One-wave passes (pgx_gram_batch, pgx_pnp_refine_batch): m = 1, 21, 65 (a second trip of the lane
loop), 130 (a third).  The pose rows carry one point on the camera plane of the pose (|z_c| < 1e-12) so that `bad` counts."""
import hashlib

import numpy as np

from helpers import ALL_MODEL_CASES, make_case
from pyprogressivex import _lib

NORM = np.array([0.01, 300.0, 200.0, 0.012, 310.0, 190.0])      # Hartley normalisation of the DLT / 8-point rows
WEIGHTS = ((False, 2), (True, 1), (True, 2))                    # (use the weights, power)
BLOCK_SIZES = (1, 64, 65, 257, 4097)
SUM_SIZES = BLOCK_SIZES + (65537,)
BATCH_SHAPES = ((1, 1), (3, 21), (2, 65), (2, 130))
# (case of helpers.make_case, row kind, what the parameter block is)
GRAM_COMBOS = (("line", _lib.GRAM_AFFINE, None), ("plane", _lib.GRAM_AFFINE, None), ("homography", _lib.GRAM_AFFINE, None),
               ("pnp", _lib.GRAM_AFFINE, None), ("homography", _lib.GRAM_DLT_H, "norm"), ("fundamental", _lib.GRAM_EPI_F, "norm"),
               ("vanishing_point", _lib.GRAM_VP, None), ("pnp", _lib.GRAM_PNP_GN, "pose"), ("sphere", _lib.GRAM_SPHERE, "round"),
               ("circle", _lib.GRAM_CIRCLE, "round"))


class Recorder:
    def __init__(self):
        self.sha, self.floats, self.ints, self.calls = hashlib.sha256(), {}, {}, {}

    def inputs(self, *arrays):
        for a in arrays:
            if a is not None:
                self.sha.update(np.ascontiguousarray(a).tobytes())

    def out(self, group, call, floats, ints=()):
        f = np.asarray(floats, dtype=np.float64).reshape(-1)
        i = np.asarray(ints, dtype=np.int64).reshape(-1)
        self.floats.setdefault(group, []).append(f)
        self.ints.setdefault(group, []).append(i)
        self.calls.setdefault(group, []).append((call, f.size, i.size))

    def result(self):
        return ({g: np.concatenate(v) for g, v in self.floats.items()}, {g: np.concatenate(v) for g, v in self.ints.items()},
                self.calls, self.sha.hexdigest())


def _labels(rng, n):
    """labels 0 and 2 populated, 1 empty, 3 = the outlier label of the K = 3 calls"""
    if n < 3:
        return np.zeros(n, np.int32)
    lab = rng.choice(np.array([0, 2, 3], dtype=np.int32), n).astype(np.int32)
    lab[:3] = (0, 2, 3)
    return lab


def _on_camera_plane(pose, point):
    """the pose with t_z moved so that the 2D-3D row `point` has z_c = 0"""
    P = np.array(pose, dtype=np.float64).reshape(3, 4)
    P[2, 3] = -float(P[2, :3] @ point[2:5])
    return P.reshape(-1)


def _params(what, pts, models, first):
    """[3, np] parameter blocks, one per label / selection; first[k] = the point that block k puts on the camera plane (or None)"""
    if what is None:
        return None
    if what == "norm":
        return np.array([NORM * (1.0 + 0.001 * k) for k in range(3)])
    if what == "pose":
        return np.array([models[k] if first[k] is None else _on_camera_plane(models[k], pts[first[k]]) for k in range(3)])
    centre, scale = pts.mean(axis=0), float(pts.std()) + 1.0
    return np.array([np.concatenate([centre, [scale]]) * (1.0 + 0.001 * k) for k in range(3)])


def _tri(G):
    q = G.shape[-1]
    iu = np.triu_indices(q)
    return G[..., iu[0], iu[1]]


def _gram_block_passes(ctx, rec, name, kind, what, nan_row=False):
    group = f"gram_{name}_{kind}" + ("_nan" if nan_row else "")
    for j, n in enumerate((257,) if nan_row else BLOCK_SIZES):
        mt, pts, models, _ = make_case(name, n, 3, seed=100 + n)
        rng = np.random.default_rng(200 + n)
        if nan_row:
            pts[7] = np.nan
        labels = _labels(rng, n)
        weights = rng.random(n) + 0.5
        first = [int(np.flatnonzero(labels == k)[0]) if (labels == k).any() else None for k in range(3)]
        prm = _params(what, pts, models, first)
        lists = []
        if n == 257 and not nan_row:
            long = rng.permutation(n).astype(np.int32)
            long[0], long[6] = first[0], long[5]
            lists = [np.zeros(0, np.int32), long[:1].copy(), long]
        elif n == 4097:
            lists = [rng.permutation(n).astype(np.int32)]
        rec.inputs(pts, labels, weights, prm, *lists)
        ctx.set_points(mt, pts)
        ctx.set_labels(labels)
        for use_w, wpow in (WEIGHTS if n == 257 and not nan_row else (WEIGHTS[j % 3],)):
            w, tag = weights if use_w else None, f"n{n}_w{int(use_w)}p{wpow}"
            for K in (3, 1):
                G, cnt, bad = ctx.gram_labels(kind, K, params=None if prm is None else prm[:K], weights=w, wpow=wpow)
                rec.out(group, f"{tag}_labels_K{K}", _tri(G), np.concatenate([cnt, bad]))
            for k in range(4):
                G, cnt, bad = ctx.gram(kind, ("label", k), params=None if prm is None else prm[min(k, 2)], weights=w, wpow=wpow)
                rec.out(group, f"{tag}_label{k}", _tri(G), (cnt, bad))
            for idx in lists:
                G, cnt, bad = ctx.gram(kind, ("index", idx), params=None if prm is None else prm[0], weights=w, wpow=wpow)
                rec.out(group, f"{tag}_index_m{idx.size}", _tri(G), (cnt, bad))


def _gram_batches(ctx, rec, name, kind, what):
    group = f"gram_batch_{name}_{kind}"
    n = 300
    mt, pts, models, _ = make_case(name, n, 3, seed=7)
    rng = np.random.default_rng(8)
    weights = rng.random(n) + 0.5
    ctx.set_points(mt, pts)
    rec.inputs(pts, weights)
    for j, (B, m) in enumerate(BATCH_SHAPES):
        index = rng.integers(0, n, (B, m)).astype(np.int32)
        prm = _params(what, pts, models, [int(index[0, 0]), None, None])
        prm = None if prm is None else prm[:B]
        rec.inputs(index, prm)
        for use_w, wpow in (WEIGHTS if (B, m) == (3, 21) else (WEIGHTS[j % 3],)):
            G, bad = ctx.gram_batch(kind, index, params=prm, weights=weights if use_w else None, wpow=wpow)
            rec.out(group, f"B{B}_m{m}_w{int(use_w)}p{wpow}", _tri(G), bad)


def _pose_refits(ctx, rec):
    n = 600
    mt, pts, models, thr = make_case("pnp", n, 3, seed=21)
    rng = np.random.default_rng(22)
    P = models[0].reshape(3, 4)
    cam = pts[:, 2:5] @ P[:, :3].T + P[:, 3]
    inl = np.flatnonzero(((cam[:, :2] / cam[:, 2:3] - pts[:, :2]) ** 2).sum(axis=1) < 2.25 * thr * thr)
    assert len(inl) >= 65, "the pose case has too few inliers for a 65-point selection"
    weights = rng.random(n) + 0.5
    ctx.set_points(mt, pts)
    rec.inputs(pts, weights)
    for B, m in ((3, 21), (2, 65)):
        picks = np.array([np.sort(rng.choice(inl, m, replace=False)) for _ in range(B)]).astype(np.int32)
        inits = np.tile(models[0], (B, 1)).reshape(B, 3, 4)
        inits[:, :, 3] += rng.normal(0, 0.01, (B, 3))
        inits = inits.reshape(B, 12)
        inits[1] = _on_camera_plane(inits[1], pts[picks[1, 0]])          # this selection fails: status 0
        rec.inputs(picks, inits)
        for use_w, wpow in WEIGHTS:
            poses, ok = ctx.pnp_refine_batch(inits, picks, weights=weights if use_w else None, wpow=wpow)
            assert not ok[1] and ok[0], "the planted failure (and only it) must come back with status 0"
            rec.out("pnp_refine_batch", f"B{B}_m{m}_w{int(use_w)}p{wpow}", poses, ok)


def _residual_sums(ctx, rec, name, nan_row=False):
    group = f"residual_sums_{name}" + ("_nan" if nan_row else "")
    for n in ((257,) if nan_row else SUM_SIZES):
        mt, pts, models, thr = make_case(name, n, 3, seed=300 + n)
        rng = np.random.default_rng(400 + n)
        if nan_row:
            pts[7] = np.nan
        labels = _labels(rng, n)
        rec.inputs(pts, labels, models)
        ctx.set_points(mt, pts)
        ctx.set_labels(labels)
        rec.out(group, f"n{n}_K3", ctx.residual_sums(models))
        rec.out(group, f"n{n}_K1", ctx.residual_sums(models[:1]))
        rec.out(group, f"n{n}_single", [ctx.residual_sum(models[min(k, 2)], k) for k in range(4)])
        if name == "line" and n == 65537:                                 # the three reductions of pgx_preference: 257 blocks
            comp = rng.uniform(0, 1, n) * (rng.uniform(0, 1, n) < 0.5)
            rec.inputs(comp)
            ctx.set_compound(comp)
            p = ctx.preference(models[0], 2.25 * thr * thr, slot=0)
            rec.out("preference_line", f"n{n}", (p["dot"], p["pref_sqnorm"], p["comp_sqnorm"]))
            ctx.set_compound(None)


def run(ctx):
    rec = Recorder()
    for name, kind, what in GRAM_COMBOS:
        _gram_block_passes(ctx, rec, name, kind, what)
        _gram_batches(ctx, rec, name, kind, what)
    _gram_block_passes(ctx, rec, "line", _lib.GRAM_AFFINE, None, nan_row=True)
    _pose_refits(ctx, rec)
    for name in ALL_MODEL_CASES:
        _residual_sums(ctx, rec, name)
    _residual_sums(ctx, rec, "line", nan_row=True)
    return rec.result()
