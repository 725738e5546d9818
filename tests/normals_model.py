"""pgx_estimate_normals (include/pgx.h) restated in numpy / plain Python: TEST INFRASTRUCTURE ONLY.

Every sum is a Python loop over Python floats (IEEE binary64, one rounding per operation, no contraction), in the order the header
states: the self term first, the row of the symmetric CSR in its own order.  The eigenpair comes from the oracle's pgxo_eigh_smallest
(cyclic Jacobi in the device kernel's operation order), so the device is expected to return these BITS.

estimate(points, off, idx, viewpoint=None) -> dict(normals [n, 3], curvature [n], undefined, cov [n, 3, 3], defined [n] bool,
sweeps [n]).  `plant` switches on one deliberate error at a time, for the tests that show the accuracy bound refuses them:
"no_self" (the self term dropped from both passes, m = row length), "uncentred" (one pass, c_ab = sum e_a e_b about the point itself),
"f32" (the covariance formed in binary32), "largest" (the eigenvector of the largest eigenvalue).

tolerance_factor(m) is the C(m) of DESIGN.md 4.10: the angle between the computed normal and the exact one of the same binary64
coordinates is at most C(m) * EPS * lambda_max / (lambda_1 - lambda_0)."""
import math

import numpy as np

EPS = 2.0 ** -52
MAX_SWEEPS = 10          # the premise of the Jacobi term of C(m); the tests check it on every matrix they bound


def tolerance_factor(m):
    """C(m), in units of EPS = 2^-52 = twice the unit roundoff u (the factor 2 is Davis-Kahan's: sin(angle) <= 2 |E| / gap).  In units
    of u * lambda_max the perturbation E of the covariance matrix is bounded by (DESIGN.md 4.10 derives each term)
      3 (m + 4 + 2 sqrt(m - 1))     the offsets' rounding, the centred differences', the products' and the sequential sum's
      61 per sweep                  three rotations, each (4 sqrt 2 + 6) u |A|_F with |A|_F <= sqrt 3 lambda_max
      22 per sweep                  the same three rotations on the accumulated eigenvector (not amplified by the gap; counted as if)
      6                             the off-diagonal part the stopping rule leaves, and the second-order terms
    with MAX_SWEEPS sweeps."""
    return 3.0 * (m + 4.0 + 2.0 * math.sqrt(m - 1.0)) + (61.0 + 22.0) * MAX_SWEEPS + 6.0


def _f32(x):
    return float(np.float32(x))


def covariance(P, i, row, plant=None):
    """(c [3][3] as nested lists, m, finite) of point i with neighbours `row` (P: list of [x, y, z] Python floats)"""
    xi = P[i]
    nb = [P[j] for j in row]
    m = len(nb) + (0 if plant == "no_self" else 1)
    finite = all(math.isfinite(v) for v in xi) and all(math.isfinite(v) for p in nb for v in p)
    if plant == "f32":
        rnd = _f32
    else:
        def rnd(x):
            return x
    e = [[rnd(p[a] - xi[a]) for a in range(3)] for p in nb]
    if plant == "uncentred":
        mu = [0.0, 0.0, 0.0]
        terms = e
    else:
        s = [0.0, 0.0, 0.0]
        for ej in e:
            for a in range(3):
                s[a] = rnd(s[a] + ej[a])
        mu = [rnd(s[a] / m) if m else math.nan for a in range(3)]
        terms = ([] if plant == "no_self" else [[0.0, 0.0, 0.0]]) + e
    c = [[0.0] * 3 for _ in range(3)]
    first = True
    for ej in terms:
        d = [rnd(ej[a] - mu[a]) for a in range(3)]
        for a in range(3):
            for b in range(a, 3):
                prod = rnd(d[a] * d[b])
                c[a][b] = prod if first else rnd(c[a][b] + prod)
        first = False
    for a in range(3):
        for b in range(a):
            c[a][b] = c[b][a]
    return c, m, finite


def orient(n, x, viewpoint=None):
    """the sign rule: the entry of largest magnitude (lowest index on ties) positive, then towards the viewpoint"""
    n = [float(v) for v in n]
    big = n[0]
    if abs(n[1]) > abs(big):
        big = n[1]
    if abs(n[2]) > abs(big):
        big = n[2]
    if big < 0.0:
        n = [-v for v in n]
    if viewpoint is not None:
        v = [float(t) for t in viewpoint]
        t = ((v[0] - x[0]) * n[0] + (v[1] - x[1]) * n[1]) + (v[2] - x[2]) * n[2]
        if t < 0.0:
            n = [-v for v in n]
    return n


def estimate(points, off, idx, viewpoint=None, plant=None):
    import pgx_oracle as O
    pts = np.ascontiguousarray(points, dtype=np.float64)
    n = pts.shape[0]
    P = pts.tolist()
    off = np.asarray(off).tolist()
    idx = np.asarray(idx).tolist()
    cov = np.full((n, 3, 3), np.nan)
    defined = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            c, m, finite = covariance(P, i, idx[off[i]:off[i + 1]], plant)
            if m < 3 or not finite or not all(math.isfinite(v) for r in c for v in r):
                continue
            cov[i] = c
            defined[i] = True
    normals = np.full((n, 3), np.nan)
    curvature = np.full(n, np.nan)
    sweeps = np.zeros(n, dtype=np.int32)
    sel = np.flatnonzero(defined)
    if len(sel):
        A = cov[sel]
        if plant == "largest":
            w, V = np.linalg.eigh(A)
            vec, val = V[:, :, 2], w[:, 2]
        else:
            vec, val, sw = O.eigh_smallest(A)
            sweeps[sel] = sw
        with np.errstate(all="ignore"):
            trace = (A[:, 0, 0] + A[:, 1, 1]) + A[:, 2, 2]
            curvature[sel] = val / trace
        for k, i in enumerate(sel):
            normals[i] = orient(vec[k], P[i], viewpoint)
    return dict(normals=normals, curvature=curvature, undefined=int(n - len(sel)), cov=cov, defined=defined, sweeps=sweeps)


def star_graph(sizes):
    """symmetric CSR of disjoint stars: neighbourhood f has sizes[f] sites, its centre first; the centre's row is its leaves in
    ascending order, a leaf's row is the centre.  Returns (off, idx, centres)."""
    off, idx, centres = [0], [], []
    base = 0
    for m in sizes:
        centres.append(base)
        idx += list(range(base + 1, base + m))
        off.append(len(idx))
        for _ in range(m - 1):
            idx.append(base)
            off.append(len(idx))
        base += m
    return np.array(off, dtype=np.int32), np.array(idx, dtype=np.int32), np.array(centres, dtype=np.int64)


def angle_to(n, hi, lo):
    """the angle between the vector n and the unit vector hi + lo (a double-double), up to sign: |n x d| / |n| with d = n - (hi + lo)
    taken after the signs are aligned - d is small and its rounding error second order, where the cross product of two nearly parallel
    vectors would lose the angle in its own rounding"""
    n = np.asarray(n, dtype=np.float64)
    hi, lo = np.asarray(hi, dtype=np.float64), np.asarray(lo, dtype=np.float64)
    if float(np.dot(n, hi)) < 0.0:
        hi, lo = -hi, -lo
    d = (n - hi) - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.linalg.norm(np.cross(n, d)) / (np.linalg.norm(n) * np.linalg.norm(hi)))
