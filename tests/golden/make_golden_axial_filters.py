#!/usr/bin/env python3
"""Regenerates tests/golden/kat_axial_filters_v1.npz: what the f32 filters of the axial types decide, recorded ONCE on an MI355X with the
library of the commit before the four filters were written as one (csrc/score_filters.hip.h, AxialFilter32) and replayed by
tests/test_gpu_axial_filters.py on the library as built.  The scene, the batches and what is recorded are in
tests/axial_filter_cases.py.  Fixture = data only: the scene and the hypotheses come from this project's generators, the keep words
and the counters from its own library.

Every type runs twice on a context of its own; nothing may differ between the two runs, and every batch must meet the conditions
check() states, or the script stops without writing.  Run from the repository root (needs the GPU):
    python tests/golden/make_golden_axial_filters.py [output.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
import axial_filter_cases as A  # noqa: E402
from pyprogressivex import _lib  # noqa: E402


def check(mt, path, filt, counters, keep):
    """the conditions every recorded batch meets: the cull and the f32 filter ran; the set bits of the keep words are the surviving
    steps; the cull decided both ways, and so did the filter; the special rows are culled everywhere / nowhere"""
    groups = (A.N + 63) // 64
    if (path, filt) != ("cull + group-major", "f32"):
        return f"path {path}, filter {filt}"
    if keep.shape != (groups, A.MPAD // 64) or A.popcount(keep) != counters[0]:
        return f"keep words {keep.shape}, {A.popcount(keep)} bits, {counters[0]} surviving steps"
    if not 0.05 * groups * A.M < counters[0] < 0.95 * groups * A.M:
        return f"{counters[0]} of {groups * A.M} steps survive"
    if not counters[2] < counters[1] < 0.5 * counters[0] * 64:
        return f"{counters[1]} exact evaluations of {counters[0]} surviving steps, {counters[2]} inlier pairs"
    culled, kept = A.SPECIAL[mt]
    for back in culled:
        if A.column(keep, A.M - back).any():
            return f"row M - {back} is not culled everywhere"
    for back in kept:
        if not A.column(keep, A.M - back).all():
            return f"row M - {back} is culled somewhere"
    return None


def main():
    pts, nrm, gt = A.scene()
    out = dict(pts=pts, nrm=nrm, T2=np.array([A.T2]), kappa=np.array([A.KAPPA]), types=np.array(A.TYPES, dtype=np.int32))
    for mt in A.TYPES:
        models = A.hypotheses(mt, gt)
        runs = []
        for _ in range(2):
            ctx = _lib.Context(0)
            try:
                runs.append(A.run_on(ctx, mt, pts, nrm, models))
            finally:
                ctx.close()
        (path, filt, counters, keep), b = runs
        if (path, filt) != b[:2] or not np.array_equal(counters, b[2]) or not np.array_equal(keep, b[3]):
            sys.exit(f"type {mt}: two runs of the same library differ ({counters} then {b[2]}); nothing written")
        msg = check(mt, path, filt, counters, keep)
        if msg:
            sys.exit(f"type {mt}: {msg}; nothing written")
        mixed = int(sum(0 < int(A.column(keep, r).sum()) < keep.shape[0] for r in range(A.M)))
        print(f"type {mt}: {dict(zip(A.COUNTERS, counters.tolist()))}, {mixed} of {A.M} hypotheses culled in some groups and kept in others", flush=True)
        out[f"models_{mt}"], out[f"keep_{mt}"], out[f"counters_{mt}"] = models, keep, counters
    path = sys.argv[1] if len(sys.argv) > 1 else A.FILE
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
