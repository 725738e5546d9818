"""Regenerates tests/golden/kat_refits_v1.npz: the point sets, weights, labellings and selections of the refit accuracy tests
and, for every (selection, weighting) pair, what tests/refit_exact.py - the refits restated from their definitions in mpmath at 50
digits - answers: the model, its vector in the normalised space, the terms of the tolerance and the tolerance.  Run from the
repository root: `python tests/golden/make_golden_refits.py` (needs mpmath).  Fixture = data only, produced by this project's test
code alone: which points of make_case are inliers of its first ground-truth structure, so that the selections can be drawn by
kind, is decided by a plain numpy distance (distances()), not by the oracle.

plan(name) (no mpmath) lays out one type: 300 points of make_case(name, 1000, 3, SEED) - 230 inliers of the first structure, 70 of the
far points, shuffled - then copies of one selection moved by 1e4 (two-view types, vanishing point: the normalisation's case) or 1e3 (line,
plane: the raw moments' case); the labelling (0: 200 inliers spread over the set, 1: the other inliers, 2: the rest) and the
selections of refit_accuracy_cases.py's docstring.  row(name, plan, selection, weighting) is one fixture row.  Every fixture meets
the conditions check_row() states; a selection that fails one is drawn again (`attempt`), never kept and exempted.
homography_sym has the homography's fixtures (its model is [H | H^-1] of the same fit)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
import refit_exact as X  # noqa: E402
from refit_accuracy_cases import (BASE, FAMILY, FILE, MINIMAL, NMAX, SEED, STORED, WIDTH, ZERO_AT, C_D0, C_FAC, C_FIRST,  # noqa: E402
                                  C_GAP, C_INV0, C_INVS, C_J0, C_JS, C_JTJ0, C_KAPPA, C_LMAX, C_MODEL, C_ND0, C_NORM, C_R0, C_RS,
                                  C_SENS, C_START, C_THETA, C_TOL)

SIZES = (9, 21, 63, 64, 65, 128, 129, 200)
WIDE_ON = ("index128", "index200", "label0")
START_SCALES = (1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5)
START_MOTION = (1e-6, -2e-6, 1.5e-6, 1e-4, -2e-4, 3e-4)     # (omega, dt) from the minimiser to the start of a pose fixture's run
FIT = dict(homography=X.homography, fundamental=X.fundamental, vanishing_point=X.vanishing_point, line=X.flat, plane=X.flat,
           circle=X.round_, sphere=X.round_)


def weights():
    """[2, NMAX]: uniform in [0.5, 1.5]; log-uniform over 1e-3 .. 1e3 with both ends present and an exact zero at ZERO_AT"""
    rng = np.random.default_rng(SEED + 77)
    wide = 10.0 ** rng.uniform(-3.0, 3.0, NMAX)
    wide[ZERO_AT], wide[ZERO_AT + 1], wide[ZERO_AT + 2] = 0.0, 1e-3, 1e3
    return np.stack([rng.uniform(0.5, 1.5, NMAX), wide])


def distances(name, pts, m):
    """a plain geometric distance of every point to the model m, in numpy: only the ORDER it gives is used (plan() below)"""
    with np.errstate(all="ignore"):
        if name in ("line", "plane"):
            d = pts.shape[1]
            return np.abs(pts @ m[:d] + m[d])
        if name in ("circle", "sphere"):
            d = pts.shape[1]
            return np.abs(np.linalg.norm(pts - m[:d], axis=1) - m[d])
        if name == "vanishing_point":                           # the end point against the line through the midpoint and the vanishing point
            mid = np.column_stack([(pts[:, 0] + pts[:, 2]) / 2, (pts[:, 1] + pts[:, 3]) / 2, np.ones(len(pts))])
            ln = np.cross(mid, m[None, :])
            return np.abs(ln[:, 0] * pts[:, 0] + ln[:, 1] * pts[:, 1] + ln[:, 2]) / np.hypot(ln[:, 0], ln[:, 1])
        if name == "pnp":
            Xc = pts[:, 2:] @ m.reshape(3, 4)[:, :3].T + m.reshape(3, 4)[:, 3]
            return np.hypot(Xc[:, 0] / Xc[:, 2] - pts[:, 0], Xc[:, 1] / Xc[:, 2] - pts[:, 1])
        x1 = np.column_stack([pts[:, :2], np.ones(len(pts))])
        x2 = np.column_stack([pts[:, 2:], np.ones(len(pts))])
        M = m[:9].reshape(3, 3)
        if name == "homography":
            y = x1 @ M.T
            return np.hypot(y[:, 0] / y[:, 2] - pts[:, 2], y[:, 1] / y[:, 2] - pts[:, 3])
        l2, l1 = x1 @ M.T, x2 @ M                               # fundamental matrix: Sampson
        return np.abs((x2 * l2).sum(1)) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)


def plan(name, attempt=0):
    from helpers import make_case
    mt, pts, models, thr = make_case(name, 1000, 3, seed=SEED)
    # make_case gives the first structure 200 points of 800 and repeats 200 rows: its inliers are the 240 nearest points, whatever
    # the unit of the distance; the rest is drawn from the points beyond the 300th
    dist = distances(name, pts, models[0])
    order = np.argsort(np.where(np.isfinite(dist), dist, np.inf), kind="stable")
    inl = np.zeros(len(pts), dtype=bool)
    inl[order[:240]] = True
    far = np.zeros(len(pts), dtype=bool)
    far[order[300:]] = True
    rng = np.random.default_rng(1000 * SEED + 10 * STORED.index(name) + 100000 * attempt)
    take = np.concatenate([rng.choice(np.flatnonzero(inl), 230, replace=False), rng.choice(np.flatnonzero(far), BASE - 230, replace=False)])
    take = take[rng.permutation(BASE)]
    if not inl[take[ZERO_AT]]:                                  # the point whose wide weight is zero is an inlier, in label 0
        j = int(np.flatnonzero(inl[take])[0])
        take[[ZERO_AT, j]] = take[[j, ZERO_AT]]
    base, good = pts[take], inl[take]
    ipos, opos = np.flatnonzero(good), np.flatnonzero(~good)
    lab0 = np.sort(np.concatenate([[ZERO_AT], rng.choice(ipos[ipos != ZERO_AT], 199, replace=False)]))
    labels = np.full(BASE, 2, dtype=np.int8)
    labels[ipos], labels[lab0] = 1, 0
    sels = []                                                   # (tag, index list | None, label | -1)
    m0 = MINIMAL[name]
    for m in sorted(set((m0, m0 + 1) + SIZES)):
        idx = rng.choice(ipos, m, replace=False)
        if f"index{m}" in WIDE_ON and ZERO_AT not in idx:
            idx[0] = ZERO_AT
        sels.append((f"index{m}", idx, -1))
    rep = rng.choice(ipos, 21, replace=False)
    rep[5] = rep[2]
    sels.append(("repeated", rep, -1))
    sels.append(("label0", None, 0))
    sels.append(("label1", None, 1))
    sels.append(("inliers", rng.choice(ipos, 100, replace=False), -1))
    sels.append(("mixed", rng.permutation(np.concatenate([rng.choice(ipos, 80, replace=False), rng.choice(opos, 20, replace=False)])), -1))
    extra = np.zeros((0, base.shape[1]))
    if FAMILY[name] in ("two_view", "vp"):
        src = dict((t, i) for t, i, _ in sels)["index21"]
        extra, shift = base[src], np.full(base.shape[1], 1e4)
        sels.append(("shifted", BASE + np.arange(len(src)), -1))
    elif FAMILY[name] == "flat":
        src = dict((t, i) for t, i, _ in sels)["index64"]
        extra, shift = base[src], np.full(base.shape[1], 1e3)
        sels.append(("offset", BASE + np.arange(len(src)), -1))
    if len(extra):
        base = np.vstack([base, extra + shift])
        labels = np.concatenate([labels, np.full(len(extra), 2, dtype=np.int8)])
    start = models[0] if name == "pnp" else None
    return dict(name=name, pts=np.ascontiguousarray(base), labels=labels, sels=sels, start=start)


def fixtures_of(p):
    """[(selection number, weighting 0 off | 1 uniform | 2 wide)]"""
    out = []
    for s, (tag, _, _) in enumerate(p["sels"]):
        out += [(s, 0), (s, 1)] + ([(s, 2)] if tag in WIDE_ON else [])
    return out


def members(p, s):
    tag, idx, label = p["sels"][s]
    return np.flatnonzero(p["labels"] == label) if idx is None else np.asarray(idx)


def row(name, p, s, weighting, W):
    idx = members(p, s)
    w = None if weighting == 0 else W[weighting - 1][idx]
    out = np.zeros(WIDTH)
    if name == "pnp":
        pts = p["pts"][idx]
        end, _ = X.pnp_run(pts, w, p["start"], iterations=400, until=1e-40)     # the minimiser, from the ground-truth pose
        assert X.pnp_jacobian_check(pts, w, p["start"]) <= 1e-15                  # analytic against central differences
        st = X.pnp_state(pts, w, p["start"])                                      # the single step: from the ground-truth pose
        # the run's start: a fixed motion away from the minimiser, at the largest scale from which the reference's own run is below
        # 1e-12 within 6 iterations (Gauss-Newton converges linearly: the larger the residual, the slower, the nearer the start)
        for scale in START_SCALES:
            start = X.pnp_moved(end, [scale * x for x in START_MOTION])
            _, first = X.pnp_run(pts, w, start, iterations=6)
            if first is not None:
                break
        P = np.array([float(x) for x in end])
        at = X.pnp_state(pts, w, P)
        nd = float(np.linalg.norm(st["delta"]))
        out[C_TOL] = X.FACTOR * X.EPS * st["inv"] * (st["J"] * st["r"] + st["JtJ"] * nd)
        out[C_INV0], out[C_J0], out[C_R0], out[C_JTJ0], out[C_ND0], out[C_KAPPA] = st["inv"], st["J"], st["r"], st["JtJ"], nd, st["kappa"]
        out[C_FIRST] = 0 if first is None else first
        out[C_INVS], out[C_JS], out[C_RS] = at["inv"], at["J"], at["r"]
        out[C_D0], out[C_MODEL], out[C_START] = st["delta"], P, start
        return out
    r = FIT[name](p["pts"][idx], w)
    out[C_TOL], out[C_LMAX], out[C_GAP], out[C_FAC] = r["tol"], r["lam_max"], r["gap"], r["factor"]
    if len(r["sens"]):
        out[C_SENS] = r["sens"][0]
    out[C_NORM.start:C_NORM.start + len(r["norm"])] = r["norm"]
    out[C_THETA.start:C_THETA.start + len(r["theta"])] = r["theta"]
    out[C_MODEL.start:C_MODEL.start + len(r["model"])] = r["model"]
    return out


def check_row(name, p, s, out):
    """the conditions every fixture meets: tolerance <= 1e-6; the pose's one-step half kappa(J^T J) <= 1e10; its convergence half
    (every selection) the reference's own run below |delta| = 1e-12 within 6 iterations"""
    if not (0 < out[C_TOL] <= 1e-6):
        return f"tolerance {out[C_TOL]:.3g}"
    if name == "pnp":
        if not out[C_KAPPA] <= 1e10:
            return f"kappa {out[C_KAPPA]:.3g}"
        if not 1 <= out[C_FIRST] <= 6:
            return f"no convergence within 6 iterations ({out[C_FIRST]:.0f})"
    return None


def generate(verbose=True, first_attempt=None):
    """every array of the file; first_attempt = {type: the draw to begin with} (the regeneration check begins with the stored one)"""
    W = weights()
    out = dict(w=W, seed=np.array([SEED]))
    pts = np.zeros((len(STORED), NMAX, 5))
    labels = np.full((len(STORED), NMAX), -1, dtype=np.int8)
    npts, sel_flat, selinfo, meta, rows = [], [], [], [], []
    for t, name in enumerate(STORED):
        for attempt in range(0 if first_attempt is None else int(first_attempt[name]), 20):
            p = plan(name, attempt)
            fx = fixtures_of(p)
            got = [row(name, p, s, wt, W) for s, wt in fx]
            bad = [(p["sels"][s][0], wt, msg) for (s, wt), r in zip(fx, got) for msg in [check_row(name, p, s, r)] if msg]
            if not bad:
                break
            if verbose:
                print(name, "attempt", attempt, "drawn again:", bad)
        else:
            raise SystemExit(f"{name}: no plan met the conditions")
        n = len(p["pts"])
        pts[t, :n, :p["pts"].shape[1]] = p["pts"]
        labels[t, :n] = p["labels"]
        npts.append([n, attempt])
        first = len(selinfo)
        for tag, idx, label in p["sels"]:
            idx = np.zeros(0, dtype=np.int64) if idx is None else idx
            selinfo.append([t, sum(len(x) for x in sel_flat), len(idx), label])
            sel_flat.append(idx)
        meta += [[t, first + s, wt] for s, wt in fx]
        rows += got
        if name == "pnp":
            out["pnp_start"] = np.asarray(p["start"], dtype=np.float64)
        if verbose:
            print(f"{name}: {len(fx)} fixtures, worst tolerance {max(r[C_TOL] for r in got):.3g}")
    out.update(pts=pts, labels=labels, npts=np.array(npts, dtype=np.int32), sel=np.concatenate(sel_flat).astype(np.int16),
               selinfo=np.array(selinfo, dtype=np.int32), meta=np.array(meta, dtype=np.int16), fx=np.array(rows))
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(FILE, **data)
    print("wrote", os.path.basename(FILE), os.path.getsize(FILE), "bytes,", len(data["fx"]), "fixtures")
