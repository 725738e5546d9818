"""Regenerates tests/golden/kat_3d_v1.npz: seeded inputs + the oracle's outputs for the 3-D point-cloud types (planes, type 6;
spheres, type 8): residuals, score table, preference, unary table, minimal solvers (the sphere's also under a radius range) and the
Gram rows of the refits.  Run from the repository root: `python tests/golden/make_golden_3d.py`.  Same status as kat_v1.npz: the
reference has no such model types, so the vectors pin the oracle against itself over time and CPU<->GPU; the checks against exact
arithmetic and the hand-checkable cases live in tests/test_oracle.py.  Fixture = data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
import pgx_oracle as O  # noqa: E402
from helpers import MODEL_CASES_3D, make_case  # noqa: E402

out = {}
rng = np.random.default_rng(13)
for name, mt in MODEL_CASES_3D.items():
    pts, models, thr = make_case(name, 200, 6, seed=41)[1:]
    T2 = 2.25 * thr * thr
    comp = rng.uniform(0, 1, 200) * (rng.uniform(0, 1, 200) < 0.5)
    out[f"{name}_pts"], out[f"{name}_models"], out[f"{name}_thr"], out[f"{name}_comp"] = pts, models, np.array([thr]), comp
    out[f"{name}_sq0"] = O.squared_residuals(mt, pts, models[0])
    out[f"{name}_plain0"] = np.array([O.residual(mt, p, models[0]) for p in pts])
    sc = O.score(mt, pts, models, T2, compound=comp, has_compound=True, exponent=2, want_masks=True)
    for k in ("counts", "values", "shared", "scores", "masks"):
        out[f"{name}_{k}"] = sc[k]
    out[f"{name}_pref0"] = O.preference(mt, pts, models[0], T2)
    out[f"{name}_unary_q"] = O.unary_q(mt, pts, models[:3], thr, 0.1)
    smp = rng.integers(0, 200, (64, O.SAMPLE_SIZE[mt])).astype(np.int32)
    smp[:4, 1] = smp[:4, 0]
    out[f"{name}_samples"], out[f"{name}_solved"] = smp, O.solve_minimal(mt, pts, smp)
    idx = rng.permutation(200)[:120]
    w = rng.random(200) + 0.5
    out[f"{name}_idx"], out[f"{name}_w"] = idx, w
    out[f"{name}_G{O.GRAM_AFFINE}"] = O.gram(O.GRAM_AFFINE, pts, idx, weights=w, wpow=1)[0]
    if name == "sphere":
        prm = np.concatenate([pts[idx].mean(axis=0), [pts[idx].std()]])
        out["sphere_gram_params"] = prm
        out[f"sphere_G{O.GRAM_SPHERE}"] = O.gram(O.GRAM_SPHERE, pts, idx, params=prm, weights=w, wpow=1)[0]
        radii = out["sphere_solved"][:, 3]
        rr = np.array([0.5, float(np.nanmedian(radii))])     # the upper end IS a radius of the batch: inclusive
        out["sphere_radius_range"] = rr
        out["sphere_solved_ranged"] = O.solve_minimal(mt, pts, smp, radius_range=(rr[0], rr[1]))
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_3d_v1.npz"), **out)
print("wrote kat_3d_v1.npz with", len(out), "arrays")
