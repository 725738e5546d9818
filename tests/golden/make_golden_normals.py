"""Regenerates tests/golden/kat_normals_v1.npz: neighbourhoods of a make_cylinders scene and, for each, what the definition of
pgx_estimate_normals (include/pgx.h) gives in mpmath at 50 digits on the same binary64 coordinates: the eigenvector of the smallest
eigenvalue of the neighbourhood's covariance (as a double-double, hi + lo) and all three eigenvalues.  Run from the repository root:
`python tests/golden/make_golden_normals.py` (needs mpmath and the built oracle, whose numpy k-NN lists pick the neighbourhoods).
Fixture = data only, produced by this project's test code alone.

Layout: 60 neighbourhoods for each of k = 2, 5, 16 from the symmetric k-NN graph of the scene (2 000 points: 3 cylinders x 500,
500 outliers, seed 11), centres drawn among the cylinders' points, and 60 more of k = 16 on the scene moved by 1e6 in every
coordinate (the rounded sums are the inputs: their reference is that of the moved, rounded coordinates).  A neighbourhood is its centre
followed by its row in ascending index order.  Every fixture meets the condition of check(): tolerance_factor(m) * EPS * lambda_max /
(lambda_1 - lambda_0) <= 1e-6; a draw that fails it is drawn again, never kept and exempted."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
import normals_model as NM  # noqa: E402

FILE = os.path.join(HERE, "kat_normals_v1.npz")
DIGITS = 50
SEED = 11
PER_GROUP = 60
GROUPS = ((2, 0.0), (5, 0.0), (16, 0.0), (16, 1e6))     # (k, shift)


def exact(nb):
    """nb [m, 3] binary64, the centre first -> (normal hi [3], normal lo [3], eigenvalues [3] ascending) at 50 digits"""
    import mpmath
    from mpmath import mp, mpf
    mp.dps = DIGITS
    m = len(nb)
    e = [[mpf(float(p[a])) - mpf(float(nb[0][a])) for a in range(3)] for p in nb]
    mu = [sum(ej[a] for ej in e) / m for a in range(3)]
    C = mpmath.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            C[a, b] = sum((ej[a] - mu[a]) * (ej[b] - mu[b]) for ej in e)
    E, Q = mp.eigsy(C)
    order = sorted(range(3), key=lambda t: E[t])
    v = [Q[a, order[0]] for a in range(3)]
    nv = mp.sqrt(sum(x * x for x in v))
    v = [x / nv for x in v]
    hi = [float(x) for x in v]
    lo = [float(x - mpf(h)) for x, h in zip(v, hi)]
    return np.array(hi), np.array(lo), np.array([float(E[t]) for t in order])


def check(m, eig):
    gap = eig[1] - eig[0]
    return gap > 0 and NM.tolerance_factor(m) * NM.EPS * eig[2] / gap <= 1e-6


def generate(verbose=True):
    import pgx_oracle as O
    from pyprogressivex import datasets
    pts, _, labels, _ = datasets.make_cylinders(n_per_cylinder=500, n_cylinders=3, n_outliers=500, seed=SEED)
    rng = np.random.default_rng(SEED)
    flat, sizes, his, los, eigs, tags = [], [], [], [], [], []
    for g, (k, shift) in enumerate(GROUPS):
        moved = pts + shift
        off, idx, _ = O.graph_build(moved, 2, k=k)
        cand = rng.permutation(np.flatnonzero(labels > 0))
        kept = 0
        for i in cand:
            row = idx[off[i]:off[i + 1]]
            nb = moved[np.concatenate([[i], row])]
            if len(nb) < 3:
                continue
            hi, lo, eig = exact(nb)
            if not check(len(nb), eig):
                continue
            flat.append(nb)
            sizes.append(len(nb))
            his.append(hi)
            los.append(lo)
            eigs.append(eig)
            tags.append(g)
            kept += 1
            if kept == PER_GROUP:
                break
        else:
            raise SystemExit(f"group {g}: fewer than {PER_GROUP} neighbourhoods met the condition")
        if verbose:
            print(f"k = {k}, shift {shift:g}: {kept} neighbourhoods, m = {min(sizes[-kept:])} .. {max(sizes[-kept:])}")
    return dict(points=np.vstack(flat), sizes=np.array(sizes, dtype=np.int32), normal_hi=np.array(his), normal_lo=np.array(los),
                eig=np.array(eigs), group=np.array(tags, dtype=np.int8), groups=np.array(GROUPS), seed=np.array([SEED]))


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(FILE, **data)
    print("wrote", os.path.basename(FILE), os.path.getsize(FILE), "bytes,", len(data["sizes"]), "neighbourhoods")
