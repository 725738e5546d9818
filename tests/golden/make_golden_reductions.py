#!/usr/bin/env python3
"""The Gram and residual-sum reduction passes, recorded ONCE on an MI355X at the commit before csrc/fit.hip and csrc/pointwise.hip
stated each of them once (the single-label and the all-labels forms were separate kernels until then):
tests/golden/kat_reductions_v1.npz, replayed bit for bit by tests/test_gpu_reductions.py.  The cases are in
tests/reduction_cases.py.  The file holds outputs only - per group one float64 and one int64 array - with the SHA-256 of the
inputs and the commit.  Every case runs twice and both runs must agree (the trees are fixed: nothing may differ).  Run from the
repository root (a few seconds):
    python tests/golden/make_golden_reductions.py [output.npz [commit]]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import reduction_cases  # noqa: E402
from pyprogressivex import _lib  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "kat_reductions_v1.npz")


def main():
    with _lib.Context(0) as ctx:
        a, b = (reduction_cases.run(ctx) for _ in range(2))
    assert a[3] == b[3] and a[2] == b[2], "the inputs of two runs differ"
    for kind in (0, 1):
        for g in a[kind]:
            if a[kind][g].tobytes() != b[kind][g].tobytes():
                sys.exit(f"{g}: two runs of the same commit differ; nothing written")
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"      # (an exported tree: the caller names the commit)
    out = {f"f_{g}": v for g, v in a[0].items()}
    out.update({f"i_{g}": v for g, v in a[1].items()})
    out["inputs_sha256"] = np.array(a[3])
    out["recorded_at_commit"] = np.array(commit)
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(a[0])} groups, {sum(len(c) for c in a[2].values())} calls, "
          f"{sum(v.size for v in a[0].values())} doubles, inputs {a[3][:16]}.., commit {commit}")


if __name__ == "__main__":
    main()
