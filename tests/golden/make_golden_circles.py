"""Regenerates tests/golden/kat_circles_v1.npz: seeded inputs + the oracle's outputs for the 2-D circle (findCircles, type 10):
residuals, score table with masks, preference, unary table, residual sums, the 3-point solver without and under a radius range and
the Gram rows of the refit (GRAM_AFFINE, GRAM_CIRCLE).  Run from the repository root: `python tests/golden/make_golden_circles.py`.
Same status as kat_3d_v1.npz: the reference has no such model type, so the vectors pin the oracle against itself over time and
CPU<->GPU; the checks against exact arithmetic and the hand-checkable cases live in tests/test_oracle.py.  Fixture = data only.
Made from the oracle alone, at the commit that added type 10 to it (the child of dcbe3fa, "Describe lines/planes and
circles/spheres once per family")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
import pgx_oracle as O  # noqa: E402
from helpers import MODEL_CASES_2D, make_case  # noqa: E402

out = {}
rng = np.random.default_rng(14)
name, mt = "circle", MODEL_CASES_2D["circle"]
pts, models, thr = make_case(name, 200, 6, seed=41)[1:]
T2 = 2.25 * thr * thr
comp = rng.uniform(0, 1, 200) * (rng.uniform(0, 1, 200) < 0.5)
out["circle_pts"], out["circle_models"], out["circle_thr"], out["circle_comp"] = pts, models, np.array([thr]), comp
out["circle_sq0"] = O.squared_residuals(mt, pts, models[0])
out["circle_plain0"] = np.array([O.residual(mt, p, models[0]) for p in pts])
sc = O.score(mt, pts, models, T2, compound=comp, has_compound=True, exponent=2, want_masks=True)
for k in ("counts", "values", "shared", "scores", "masks"):
    out[f"circle_{k}"] = sc[k]
out["circle_pref0"] = O.preference(mt, pts, models[0], T2)
out["circle_unary_q"] = O.unary_q(mt, pts, models[:3], thr, 0.1)
labels = rng.integers(0, 4, 200).astype(np.int32)
out["circle_labels"] = labels
out["circle_residual_sums"] = np.array([O.residual_sum(mt, pts, models[k], labels, k) for k in range(3)])
smp = rng.integers(0, 200, (64, O.SAMPLE_SIZE[mt])).astype(np.int32)
smp[:4, 1] = smp[:4, 0]
out["circle_samples"], out["circle_solved"] = smp, O.solve_minimal(mt, pts, smp)
radii = out["circle_solved"][:, 2]
finite = np.sort(radii[np.isfinite(radii)])
rr = np.array([40.0, float(finite[len(finite) // 2])])     # the upper end IS a radius of the batch: inclusive
out["circle_radius_range"] = rr
out["circle_solved_ranged"] = O.solve_minimal(mt, pts, smp, radius_range=(rr[0], rr[1]))
idx = rng.permutation(200)[:120]
w = rng.random(200) + 0.5
out["circle_idx"], out["circle_w"] = idx, w
out[f"circle_G{O.GRAM_AFFINE}"] = O.gram(O.GRAM_AFFINE, pts, idx, weights=w, wpow=1)[0]
prm = np.concatenate([pts[idx].mean(axis=0), [pts[idx].std()]])
out["circle_gram_params"] = prm
out[f"circle_G{O.GRAM_CIRCLE}"] = O.gram(O.GRAM_CIRCLE, pts, idx, params=prm, weights=w, wpow=1)[0]
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_circles_v1.npz"), **out)
print("wrote kat_circles_v1.npz with", len(out), "arrays")
