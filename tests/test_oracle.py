"""CPU tests of the oracle itself: hand-checkable known answers, exact-rational cross-checks of every residual formula,
max-flow against scipy, expansion moves against brute force, and the committed golden vectors.

The reference ships no tests or golden vectors for this path => parity is UNPINNED against upstream;
these tests pin the oracle against the mathematics it restates and against regressions.
"""
import decimal
import itertools
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from helpers import ALL_MODEL_CASES, MODEL_CASES, MODEL_CASES_2D, MODEL_CASES_3D, make_case, random_sym_graph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_v1.npz")


# ---- hand-checkable residuals ----------------------------------------------------------------------------------------
def test_residual_known_answers(oracle):
    O = oracle
    # axis-aligned line x = 3:  (1, 0, -3)
    assert O.squared_residuals(O.LINE2D, [[5.0, 9.0], [3.0, -1.0]], [1.0, 0.0, -3.0]).tolist() == [4.0, 0.0]
    # identity homography: residual = squared displacement
    assert O.squared_residuals(O.HOMOGRAPHY, [[1, 2, 4, 6]], np.eye(3).reshape(-1)).tolist() == [25.0]
    # pure translation (2, 0): maps (1,2) -> (3,2)
    H = np.array([1, 0, 2, 0, 1, 0, 0, 0, 1.0])
    assert O.squared_residuals(O.HOMOGRAPHY, [[1, 2, 3, 2]], H).tolist() == [0.0]
    # symmetric transfer error under identity = 2 x one-way
    Hs = np.concatenate([np.eye(3).reshape(-1), np.eye(3).reshape(-1)])
    assert O.squared_residuals(O.HOMOGRAPHY_SYM, [[1, 2, 4, 6]], Hs).tolist() == [50.0]
    # pure x-translation F = [t]_x with t = (1,0,0): epipolar lines are horizontal, Sampson = dy^2 / 2
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0.0])
    assert O.squared_residuals(O.FUNDAMENTAL, [[0, 0, 7, 0], [0, 0, 7, 2]], F).tolist() == [0.0, 2.0]
    # PnP, P = [I | 0]: projection of (2, 4, 2) is (1, 2)
    P = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(-1)
    assert O.squared_residuals(O.PNP, [[1, 2, 2, 4, 2], [0, 0, 2, 4, 2]], P).tolist() == [0.0, 5.0]
    # vanishing point at infinity in direction x (v2 = 0): horizontal segments have zero residual
    vp = np.array([1.0, 0.0, 0.0])
    assert O.squared_residuals(O.VANISHING_POINT, [[0, 5, 10, 5]], vp).tolist() == [0.0]
    # vertical segment of half-length 3: its start point is 3 px away from the horizontal line through its midpoint
    assert O.squared_residuals(O.VANISHING_POINT, [[4, 2, 4, 8]], vp).tolist() == [9.0]
    # unsquared residual used by PEARL's refit test
    assert O.residual(O.LINE2D, [5.0, 9.0], [1.0, 0.0, -3.0]) == 2.0
    assert O.residual(O.HOMOGRAPHY, [1, 2, 4, 6], np.eye(3).reshape(-1)) == 5.0
    # plane z = 3, i.e. (0, 0, 1, -3): a point 2 above it, one 2 below it, one on it
    assert O.squared_residuals(O.PLANE3D, [[7.0, -1.0, 5.0], [0.0, 4.0, 1.0], [9.0, 9.0, 3.0]], [0.0, 0.0, 1.0, -3.0]).tolist() == [4.0, 4.0, 0.0]
    assert O.residual(O.PLANE3D, [7.0, -1.0, 5.0], [0.0, 0.0, 1.0, -3.0]) == 2.0
    # sphere of radius 3 about (1, 2, 3): 2 outside the shell, 2 inside it, on it, and its centre (|0 - 3| = 3)
    sph = [1.0, 2.0, 3.0, 3.0]
    assert O.squared_residuals(O.SPHERE3D, [[6.0, 2.0, 3.0], [1.0, 1.0, 3.0], [1.0, 2.0, 0.0], [1.0, 2.0, 3.0]], sph).tolist() == [4.0, 4.0, 0.0, 9.0]
    assert O.residual(O.SPHERE3D, [6.0, 2.0, 3.0], sph) == 2.0 and O.residual(O.SPHERE3D, [1.0, 1.0, 3.0], sph) == 2.0
    # r = 0 is the distance from the centre; r < 0 is evaluated as the formula stands: | |p - c| - r | = |p - c| + |r|
    assert O.squared_residuals(O.SPHERE3D, [[4.0, 6.0, 3.0]], [1.0, 2.0, 3.0, 0.0]).tolist() == [25.0]
    assert O.squared_residuals(O.SPHERE3D, [[4.0, 6.0, 3.0]], [1.0, 2.0, 3.0, -2.0]).tolist() == [49.0]
    assert O.residual(O.SPHERE3D, [4.0, 6.0, 3.0], [1.0, 2.0, 3.0, -2.0]) == 7.0
    # circle of radius 3 about (1, 2): 2 outside it, 2 inside it, on it, and its centre (|0 - 3| = 3); r = 0 and r < 0 as for the sphere
    cir = [1.0, 2.0, 3.0]
    assert O.squared_residuals(O.CIRCLE2D, [[6.0, 2.0], [1.0, 1.0], [1.0, -1.0], [1.0, 2.0]], cir).tolist() == [4.0, 4.0, 0.0, 9.0]
    assert O.residual(O.CIRCLE2D, [6.0, 2.0], cir) == 2.0 and O.residual(O.CIRCLE2D, [1.0, 1.0], cir) == 2.0
    assert O.squared_residuals(O.CIRCLE2D, [[4.0, 6.0]], [1.0, 2.0, 0.0]).tolist() == [25.0]
    assert O.squared_residuals(O.CIRCLE2D, [[4.0, 6.0]], [1.0, 2.0, -2.0]).tolist() == [49.0]
    assert O.residual(O.CIRCLE2D, [4.0, 6.0], [1.0, 2.0, -2.0]) == 7.0


def _exact_sq(name, p, m):
    p = [Fr(float(x)) for x in p]
    m = [Fr(float(x)) for x in m]
    if name == "line":
        return (m[0] * p[0] + m[1] * p[1] + m[2]) ** 2
    if name in ("homography", "homography_sym"):
        t1 = m[0] * p[0] + m[1] * p[1] + m[2]
        t2 = m[3] * p[0] + m[4] * p[1] + m[5]
        t3 = m[6] * p[0] + m[7] * p[1] + m[8]
        r = (p[2] - t1 / t3) ** 2 + (p[3] - t2 / t3) ** 2
        if name == "homography_sym":
            g = m[9:]
            s1 = g[0] * p[2] + g[1] * p[3] + g[2]
            s2 = g[3] * p[2] + g[4] * p[3] + g[5]
            s3 = g[6] * p[2] + g[7] * p[3] + g[8]
            r += (p[0] - s1 / s3) ** 2 + (p[1] - s2 / s3) ** 2
        return r
    if name == "fundamental":
        x1, y1, x2, y2 = p
        Fx = [m[0] * x1 + m[1] * y1 + m[2], m[3] * x1 + m[4] * y1 + m[5], m[6] * x1 + m[7] * y1 + m[8]]
        Ftx = [m[0] * x2 + m[3] * y2 + m[6], m[1] * x2 + m[4] * y2 + m[7], m[2] * x2 + m[5] * y2 + m[8]]
        num = (x2 * Fx[0] + y2 * Fx[1] + Fx[2]) ** 2
        return num / (Fx[0] ** 2 + Fx[1] ** 2 + Ftx[0] ** 2 + Ftx[1] ** 2)
    if name == "pnp":
        u, v, X, Y, Z = p
        px = m[0] * X + m[1] * Y + m[2] * Z + m[3]
        py = m[4] * X + m[5] * Y + m[6] * Z + m[7]
        pz = m[8] * X + m[9] * Y + m[10] * Z + m[11]
        return (u - px / pz) ** 2 + (v - py / pz) ** 2
    if name == "vanishing_point":
        xs, ys, xe, ye = p
        mx, my = (xs + xe) / 2, (ys + ye) / 2
        lx, ly, lz = my * m[2] - m[1], -(mx * m[2] - m[0]), mx * m[1] - my * m[0]
        return (lx * xs + ly * ys + lz) ** 2 / (lx * lx + ly * ly)
    if name == "plane":
        return (m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3]) ** 2
    if name == "sphere":
        # (|p - c| - r)^2 = q + r^2 - 2 r sqrt(q), q = |p - c|^2 rational; the root to 80 significant digits
        q = (p[0] - m[0]) ** 2 + (p[1] - m[1]) ** 2 + (p[2] - m[2]) ** 2
        with decimal.localcontext() as c:
            c.prec = 80
            root = (decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).sqrt()
            rq = Fr(*root.as_integer_ratio())
        return q + m[3] ** 2 - 2 * m[3] * rq
    if name == "circle":
        # the same on two coordinates: (|p - c| - r)^2 = q + r^2 - 2 r sqrt(q), q = (x - cx)^2 + (y - cy)^2
        q = (p[0] - m[0]) ** 2 + (p[1] - m[1]) ** 2
        with decimal.localcontext() as c:
            c.prec = 80
            root = (decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).sqrt()
            rq = Fr(*root.as_integer_ratio())
        return q + m[2] ** 2 - 2 * m[2] * rq
    raise KeyError(name)


@pytest.mark.parametrize("name", list(ALL_MODEL_CASES))
def test_residuals_against_exact_rational_arithmetic(oracle, name):
    """Independent check of every formula: evaluate the published definition in exact rational arithmetic."""
    mt, pts, models, thr = make_case(name, 40, 4, seed=1)
    for model in models:
        got = oracle.squared_residuals(mt, pts, model)
        for i in range(pts.shape[0]):
            ex = float(_exact_sq(name, pts[i], model))
            assert abs(got[i] - ex) <= 1e-9 * max(abs(ex), 1e-30) + 1e-18 * max(1.0, abs(ex)), (name, i)


# ---- a1 semantics -----------------------------------------------------------------------------------------------------
def test_score_semantics(oracle):
    O = oracle
    pts = np.array([[0.0, 0], [1.0, 0], [2.0, 0], [3.0, 0]])
    model = np.array([[1.0, 0, 0]])  # r^2 = x^2 : 0, 1, 4, 9
    s = O.score(O.LINE2D, pts, model, 4.0, want_masks=True)
    assert s["counts"][0] == 2 and s["masks"][0, 0] == 0b0011          # strict <
    assert s["values"][0] == (1 - 0 / 4) + (1 - 1 / 4) and s["shared"][0] == 0.0
    assert s["scores"][0] == s["values"][0]                            # empty compound: no subtraction (:110)
    comp = np.array([0.5, 1.0, 1.0, 1.0])
    s2 = O.score(O.LINE2D, pts, model, 4.0, compound=comp, exponent=2)
    assert s2["shared"][0] == min(0.5, 1.0) + min(1.0, 0.75)           # :115-117
    assert s2["scores"][0] == s2["values"][0] - 1.25 ** 2              # :120
    s3 = O.score(O.LINE2D, pts, model, 4.0, compound=comp, exponent=0)
    assert s3["scores"][0] == s3["values"][0] - 1.0                    # pow(x, 0) == 1 is still subtracted
    # early exit (:105-106): Score() iff count + 1 < best
    assert O.score(O.LINE2D, pts, model, 4.0, best_inlier_number=[3])["counts"][0] == 2
    assert O.score(O.LINE2D, pts, model, 4.0, best_inlier_number=[4])["counts"][0] == 0


def test_preference_tanimoto_compound_unseen(oracle):
    O = oracle
    pts = np.array([[0.0, 0], [1.0, 0], [3.0, 0]])
    pref = O.preference(O.LINE2D, pts, [1.0, 0, 0], 4.0)
    assert pref.tolist() == [1.0, 0.75, 0.0]                           # max(0, 1 - r^2/T^2), progx_model.h:85
    d, a, b = O.tanimoto_terms(pref, np.array([1.0, 0.0, 1.0]))
    assert (d, a, b) == (1.0, 1.0 + 0.5625, 2.0)
    ok, t = O.is_valid_tanimoto(d, a, b, 0.5)
    assert t == 1.0 / (1.5625 + 2.0 - 1.0) and ok                      # 0.39 < 0.5 -> valid
    assert not O.is_valid_tanimoto(d, a, b, 0.3)[0]
    ok, t = O.is_valid_tanimoto(0.0, 0.0, 0.0, 0.4)                    # 0/0 = NaN -> valid (progressive_x.h:587)
    assert ok and np.isnan(t)
    assert O.compound_max(np.array([[0.1, 0.9, 0.0], [0.5, 0.2, 0.0]])).tolist() == [0.5, 0.9, 0.0]
    # progressive_x.h:495-513
    for args in [(0.5, 4, 1000, 1, 5000), (0.1, 3, 400, 600, 1886), (0.05, 2, 10, 0, 100)]:
        omc, m, it, cov, n = args
        want = int(round((n - cov) * (1 - omc ** (1.0 / it)) ** (1.0 / m)))
        assert O.predicted_unseen_inliers(*args) == want


def test_unary_semantics(oracle):
    O = oracle
    pts = np.array([[0.0, 0], [1.0, 0], [2.0, 0], [2.5, 0]])
    thr, lam = 4.0 / 3.0, 0.25                                         # T2 = 9/4 thr^2 = 4
    D = O.unary(O.LINE2D, pts, [[1.0, 0, 0]], thr, lam)
    T2 = 9.0 / 4.0 * thr * thr
    assert D[:, 1].tolist() == [0.75] * 4                              # outlier label: 1 - lambda (PEARL.h:100-101)
    assert D[0, 0] == 0.0 and D[1, 0] == 0.75 * 1.0 / T2
    assert D[2, 0] == 0.75 * 4.0 / T2                                  # r^2 == T2 is NOT beyond the threshold (:123)
    assert D[3, 0] == 1.5                                              # beyond: 2 (1 - lambda)
    Dq = O.unary_q(O.LINE2D, pts, [[1.0, 0, 0]], thr, lam)
    assert Dq[3, 0] == 3 << 31 and Dq[0, 1] == 3 << 30
    assert O.quantize_lambda(0.25) == 1 << 30 and O.quantize_lambda(0.1) % 2 == 0


# ---- max-flow / expansion ----------------------------------------------------------------------------------------------
def test_maxflow_against_scipy(oracle):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_flow
    rng = np.random.default_rng(0)
    for _ in range(150):
        nn = int(rng.integers(4, 14))
        na = int(rng.integers(5, 50))
        fr, to = rng.integers(0, nn, na), rng.integers(0, nn, na)
        keep = fr != to
        fr, to = fr[keep], to[keep]
        cap = rng.integers(0, 30, len(fr))
        f, side = oracle.maxflow(nn, fr, to, cap, 0, nn - 1)
        A = np.zeros((nn, nn), dtype=np.int32)
        np.add.at(A, (fr, to), cap)
        assert f == maximum_flow(csr_matrix(A), 0, nn - 1).flow_value
        assert side[nn - 1] == 1 and (f == 0 or side[0] == 0)


def _energy_py(Dq, graph, lq, hq, lab):
    off, idx, mult = graph
    e = sum(int(Dq[i, lab[i]]) for i in range(len(lab)))
    for i in range(len(lab)):
        for a in range(off[i], off[i + 1]):
            if idx[a] < i and lab[idx[a]] != lab[i]:
                e += lq * int(mult[a])
    return e + hq * len(set(int(x) for x in lab))


def test_expansion_move_is_optimal_and_maximal(oracle):
    """Every move must (1) reach the minimum over all 2^k binary moves and (2) be the UNION of all optimal moves
    (ties -> alpha; BK's what_segment default SOURCE) — brute force on <= 9 sites."""
    rng = np.random.default_rng(1)
    for trial in range(250):
        n, L = int(rng.integers(2, 10)), int(rng.integers(2, 5))
        Dq = rng.integers(0, 12, (n, L)).astype(np.int64)
        graph = random_sym_graph(rng, n, 0.4)
        lq, hq = int(rng.integers(0, 4)) * 2, int(rng.integers(0, 8))
        lab = rng.integers(0, L, n).astype(np.int32)
        assert oracle.energy(Dq, graph, lq, hq, lab) == _energy_py(Dq, graph, lq, hq, lab)
        alpha = int(rng.integers(0, L))
        new, changed, _ = oracle.expand_alpha(Dq, graph, lq, hq, alpha, lab)
        act = [i for i in range(n) if lab[i] != alpha]
        best, union = None, lab.copy()
        for bits in itertools.product([0, 1], repeat=len(act)):
            l2 = lab.copy()
            for b, i in zip(bits, act):
                if b == 0:
                    l2[i] = alpha
            e = _energy_py(Dq, graph, lq, hq, l2)
            if best is None or e < best:
                best, union = e, l2.copy()
            elif e == best:
                union[l2 == alpha] = alpha
        assert _energy_py(Dq, graph, lq, hq, new) == best
        assert np.array_equal(new, union)
        assert changed == int(np.sum(new != lab))


def test_full_expansion_small_reaches_global_optimum_mostly(oracle):
    """alpha-expansion is a local search; on tiny instances it must at least never be worse than any single-label
    labelling and never increase the energy from its start."""
    rng = np.random.default_rng(4)
    for _ in range(40):
        n, L = int(rng.integers(3, 9)), int(rng.integers(2, 4))
        Dq = rng.integers(0, 20, (n, L)).astype(np.int64)
        graph = random_sym_graph(rng, n, 0.5)
        lq, hq = 2 * int(rng.integers(0, 4)), int(rng.integers(0, 10))
        start = np.zeros(n, np.int32)
        lab, e, cyc = oracle.expansion(Dq, graph, lq, hq, start)
        assert e == oracle.energy(Dq, graph, lq, hq, lab) <= oracle.energy(Dq, graph, lq, hq, start)
        for l in range(L):
            assert e <= oracle.energy(Dq, graph, lq, hq, np.full(n, l, np.int32))
        assert 1 <= cyc <= 1000


def test_bucket_and_residual_sum(oracle):
    labels = np.array([2, 0, 1, 0, 5, 2, 1], dtype=np.int32)
    counts, order = oracle.bucket(labels, 3)                           # L = 3: labels >= 2 are the outlier bucket
    assert counts.tolist() == [2, 2, 3] and order.tolist() == [1, 3, 2, 6, 0, 4, 5]
    pts = np.array([[1.0, 0], [2.0, 0], [3.0, 0]])
    assert oracle.residual_sum(0, pts, [1.0, 0, 0], np.array([1, 0, 1], np.int32), 1) == 4.0


# ---- committed golden vectors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_golden_vectors(oracle, name):
    g = np.load(GOLDEN)
    mt = MODEL_CASES[name]
    pts, models, thr, comp = g[f"{name}_pts"], g[f"{name}_models"], float(g[f"{name}_thr"][0]), g[f"{name}_comp"]
    T2 = 2.25 * thr * thr
    assert np.array_equal(oracle.squared_residuals(mt, pts, models[0]), g[f"{name}_sq0"])
    sc = oracle.score(mt, pts, models, T2, compound=comp, has_compound=True, exponent=2, want_masks=True)
    for k in ("counts", "values", "shared", "scores", "masks"):
        assert np.array_equal(sc[k], g[f"{name}_{k}"]), k
    assert np.array_equal(oracle.preference(mt, pts, models[0], T2), g[f"{name}_pref0"])
    assert np.array_equal(oracle.unary_q(mt, pts, models[:3], thr, 0.1), g[f"{name}_unary_q"])


def test_golden_expansion(oracle):
    g = np.load(GOLDEN)
    graph = (g["exp_off"], g["exp_idx"], g["exp_mult"])
    lab, e, cyc = oracle.expansion(g["exp_Dq"], graph, int(g["exp_lq"][0]), int(g["exp_hq"][0]),
                                   np.zeros(400, np.int32))
    assert np.array_equal(lab, g["exp_labels"]) and e == int(g["exp_energy"][0]) and cyc == int(g["exp_cycles"][0])


def test_minimal_solvers_agree_with_the_host_formulas():
    """oracle C restatement of the 2-point line / 2-segment vanishing point solvers vs the numpy estimators"""
    import pgx_oracle as O
    from pyprogressivex import _estimators, datasets
    rng = np.random.default_rng(0)
    pts, _, _ = datasets.make_lines(seed=2)
    smp = rng.integers(0, len(pts), (500, 2)).astype(np.int32)
    smp[:10, 1] = smp[:10, 0]
    ref, src = _estimators.LineEstimator().minimal(pts, smp)
    got = O.solve_minimal(O.LINE2D, pts, smp)
    assert np.isnan(got[:10]).all() and np.array_equal(np.nonzero(~np.isnan(got[:, 0]))[0], src)
    assert np.abs(got[src] - ref).max() < 1e-12
    segs, _, _ = datasets.make_vanishing_points(n_inliers=600, n_vps=3, n_outliers=200, seed=1)
    smp = rng.integers(0, len(segs), (500, 2)).astype(np.int32)
    ref, src = _estimators.VanishingPointEstimator().minimal(segs, smp)
    got = O.solve_minimal(O.VANISHING_POINT, segs, smp)
    assert np.array_equal(np.nonzero(~np.isnan(got[:, 0]))[0], src)
    assert np.abs(got[src] - ref).max() < 1e-12


# ---- committed vectors + hand-checkable cases ------------------------------------------------------------
GOLDEN_CIRCLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_circles_v1.npz")
GOLDEN_NEXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_next_v1.npz")


def test_golden_next_rows(oracle):
    g = np.load(GOLDEN_NEXT)
    for d in (2, 4, 5):
        for tag, kind, radius, k in (("ball", 0, 6.0, 5), ("knn", 2, 0.0, 8)):
            got = oracle.graph_build(g[f"g{d}_pts"], kind, radius=radius, k=k)
            for name, a in zip(("off", "idx", "mult"), got):
                assert np.array_equal(a, g[f"g{d}_{tag}_{name}"]), (d, tag, name)
    prm = np.array([0.01, 300.0, 200.0, 0.012, 310.0, 190.0])
    for name, kinds in (("line", [(oracle.GRAM_AFFINE, None)]), ("vanishing_point", [(oracle.GRAM_VP, None)]),
                        ("homography", [(oracle.GRAM_AFFINE, None), (oracle.GRAM_DLT_H, prm)]),
                        ("fundamental", [(oracle.GRAM_EPI_F, prm)]), ("pnp", [(oracle.GRAM_PNP_GN, "model")])):
        for kind, p in kinds:
            p = g[f"m_{name}_model"][:12] if isinstance(p, str) else p
            G, cnt, bad = oracle.gram(kind, g[f"m_{name}_pts"], g[f"m_{name}_idx"], params=p, weights=g[f"m_{name}_w"], wpow=2)
            ref = g[f"m_{name}_G{kind}"]
            assert cnt == 120 and bad == 0 and np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
    for name in ("line", "vanishing_point", "homography", "fundamental", "pnp"):
        got = oracle.solve_minimal(MODEL_CASES[name], g[f"s_{name}_pts"], g[f"s_{name}_samples"])
        assert np.array_equal(got, g[f"s_{name}_models"], equal_nan=True)


def test_graph_lists_hand_checked(oracle):
    # five collinear points at 0, 1, 2, 4, 8: the lists can be read off
    pts = np.array([[0.0, 0], [1, 0], [2, 0], [4, 0], [8, 0]])
    lists = oracle.graph_lists(pts, 2)
    assert lists.tolist() == [[1, 2], [0, 2], [1, 0], [2, 1], [3, 2]]     # ties (|2-1| = |2-... ) broken by index
    ball = oracle.graph_lists(pts, 2, radius=2.0)
    assert ball.tolist() == [[1, 2], [0, 2], [1, 0], [2, -1], [-1, -1]]   # squared distance <= 4
    off, idx, mult = oracle.graph_from_lists(ball)
    assert off.tolist() == [0, 2, 4, 7, 8, 8] and idx.tolist() == [1, 2, 0, 2, 0, 1, 3, 2]
    assert mult.tolist() == [2, 2, 2, 2, 2, 2, 1, 1]                      # 3 lists 2, 2 does not list 3


def test_gram_and_solvers_hand_checked(oracle):
    pts = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]])
    G, cnt, bad = oracle.gram(oracle.GRAM_AFFINE, pts, [0, 1, 2])
    assert cnt == 3 and bad == 0 and G.tolist() == [[3.0, 4.0, 2.0], [4.0, 8.0, 4.0], [2.0, 4.0, 4.0]]
    m = oracle.solve_minimal(oracle.LINE2D, pts, np.array([[0, 1], [1, 2], [0, 0]], np.int32))
    assert m[0].tolist() == [-0.0, 1.0, -0.0] or m[0].tolist() == [0.0, 1.0, 0.0]   # the x axis: normal (0, 1), c = 0
    assert m[1].tolist() == [-1.0, 0.0, 2.0] and np.isnan(m[2]).all()              # x = 2
    segs = np.array([[0.0, 0, 1, 1], [0.0, 2, 1, 1], [0.0, 0, 2, 2]])               # two segments meeting at (1, 1)
    v = oracle.solve_minimal(oracle.VANISHING_POINT, segs, np.array([[0, 1], [0, 2]], np.int32))
    assert np.allclose(v[0, :2] / v[0, 2], [1.0, 1.0]) and np.isnan(v[1]).all()     # collinear segments: no model


def test_device_solvers_agree_with_independent_numpy_solvers(oracle):
    """The C restatements the GPU is held to (elimination / bisection, no library calls) against the host numpy solvers
    that use different methods (LAPACK solve, SVD null space + companion eigenvalues, Kabsch alignment): same solution
    sets up to the methods' own accuracy."""
    from pyprogressivex import _estimators, datasets
    rng = np.random.default_rng(0)
    pts, gt, _ = datasets.make_homographies(seed=0)
    smp = rng.integers(0, len(pts), (300, 4)).astype(np.int32)
    m = oracle.solve_minimal(oracle.HOMOGRAPHY, pts, smp)
    ref, src = _estimators.HomographyEstimator().minimal(pts, smp)
    ok = np.nonzero(~np.isnan(m[:, 0]))[0]
    assert abs(len(ok) - len(src)) <= 2
    for i in np.intersect1d(ok, src):
        r = ref[np.nonzero(src == i)[0][0]]
        assert np.abs(m[i] - r).max() <= 1e-9 * max(1.0, np.abs(r).max())
    pts, gt, _ = datasets.make_two_view_motions(seed=0)
    sel = np.nonzero(gt == 1)[0]
    smp = np.stack([rng.choice(sel, 7, replace=False) for _ in range(200)]).astype(np.int32)
    m = oracle.solve_minimal(oracle.FUNDAMENTAL, pts, smp)
    ref, src = _estimators.FundamentalEstimator().minimal(pts, smp)
    for s in range(len(smp)):
        A = [ref[i] for i in np.nonzero(src == s)[0]]
        B = [m[3 * s + q] for q in range(3) if not np.isnan(m[3 * s + q, 0])]
        assert len(A) == len(B)
        for a in A:
            assert min(min(np.abs(a - b).max(), np.abs(a + b).max()) for b in B) < 1e-8
    x1, x2, K, gtp, poses = datasets.make_poses(n_per_object=400, n_objects=3, n_outliers=300, seed=0)
    pp, f = datasets.normalize_pnp(x1, x2, K)
    smp = np.stack([rng.choice(np.nonzero(gtp == 1 + s % 3)[0], 3, replace=False) for s in range(300)]).astype(np.int32)
    m = oracle.solve_minimal(oracle.PNP, pp, smp)
    ref, src = _estimators.PnPEstimator().minimal(pp, smp)
    same = 0
    for s in range(len(smp)):
        A = [ref[i] for i in np.nonzero(src == s)[0]]
        B = [m[4 * s + q] for q in range(4) if not np.isnan(m[4 * s + q, 0])]
        if len(A) != len(B):
            continue                                   # borderline roots: the consistency thresholds decide differently
        same += 1
        for a in A:
            assert min(np.abs(a - b).max() / max(1.0, np.abs(a).max()) for b in B) < 1e-5
        for b in B:                                    # a rotation, and it reprojects its three sample points
            P = b.reshape(3, 4)
            assert abs(np.linalg.det(P[:, :3]) - 1.0) < 1e-9
            Xc = pp[smp[s], 2:] @ P[:, :3].T + P[:, 3]
            assert np.abs(Xc[:, :2] / Xc[:, 2:] - pp[smp[s], :2]).max() < 1e-6
    assert same >= 290


def test_gc_labeling_minimises_the_restated_energy(oracle):
    """GC-RANSAC's inlier/outlier cut [U-12]: the oracle builds the graph the way upstream's Energy::add_term1/add_term2
    would; here the energy is written down directly (integer terms, every undirected pair once) and minimised by brute
    force on <= 10 points of a 2-D line problem.  The cut must reach the minimum and, among the minimisers, return the
    smallest inlier set (sink segment = sites that still reach t; ties -> outlier)."""
    from pyprogressivex import _lib
    rng = np.random.default_rng(5)
    q = lambda x: int(np.rint(x * 4294967296.0))
    hit_tie = 0
    for trial in range(200):
        n = int(rng.integers(2, 11))
        pts = np.column_stack([rng.random(n) * 10, rng.normal(0, 1.0, n)])
        if trial % 3 == 0:
            pts[:, 1] = np.round(pts[:, 1])          # many equal residuals -> ties
        model = np.array([0.0, 1.0, 0.0])            # the line y = 0: r = |y|
        T2, lam = float(rng.choice([0.25, 1.0, 2.25])), float(rng.choice([0.1, 0.3, 0.5, 0.9]))
        graph = random_sym_graph(rng, n, 0.5)
        flags = oracle.gc_labeling(_lib.LINE2D, pts, model, T2, lam, graph)
        sq = pts[:, 1] ** 2
        inl = sq <= T2
        e = np.where(inl, sq / T2, 1.0)
        lq = 2 * int(np.rint(lam * 2147483648.0))
        off, idx = graph[0], graph[1]
        pairs = [(i, int(j)) for i in range(n) for j in idx[off[i]:off[i + 1]] if i < j]

        def energy(x):   # x[i] = 1 inlier
            tot = 0
            for i in range(n):
                if inl[i]:
                    tot += q((1 - lam) * (1 - e[i])) if x[i] == 0 else 0
                else:
                    tot += q((1 - lam) * e[i]) if x[i] == 1 else 0
            for i, j in pairs:
                if x[i] == 0 and x[j] == 0:
                    tot += 2 * q(lam * 0.25 * (e[i] + e[j]))
                elif x[i] != x[j]:
                    tot += lq
            return tot

        best, inter, nbest = None, None, 0
        for x in itertools.product([0, 1], repeat=n):
            en = energy(x)
            if best is None or en < best:
                best, inter, nbest = en, np.array(x), 1
            elif en == best:
                inter, nbest = inter & np.array(x), nbest + 1
        hit_tie += nbest > 1
        assert energy(tuple(int(f) for f in flags)) == best
        assert np.array_equal(flags, inter)
    assert hit_tie > 5


def test_greedy_labeling_u8_against_a_python_transcription_and_brute_force(oracle):
    """U-8: GCO-v3's labelling of an energy without smooth costs.  The C restatement is checked against a direct Python
    transcription of the greedy facility-location rule on random instances, against brute force over all L^n labellings
    (<= 12 sites: greedy is a heuristic - never better than the optimum, optimal on instances with well separated
    clusters), and the h = 0 case (per-site argmin) IS the optimum."""
    import itertools
    rng = np.random.default_rng(5)

    def transcription(D, h):
        n, L = D.shape
        if h <= 0:
            return np.argmin(D, axis=1).astype(np.int32)
        e = np.full(n, 1 << 35, dtype=np.int64)
        lab = np.zeros(n, dtype=np.int32)
        closed = list(range(L))
        while closed:
            deltas = [h + int(np.minimum(D[:, l] - e, 0).sum()) for l in closed]
            k = int(np.argmin(deltas))                         # first minimum = lowest label index
            if deltas[k] >= 0:
                break
            l = closed.pop(k)
            take = D[:, l] < e
            e[take] = D[take, l]
            lab[take] = l
        return lab

    def energy(D, h, lab):
        return int(D[np.arange(len(lab)), lab].sum()) + h * len(set(lab.tolist()))

    optimal = 0
    for trial in range(300):
        n, L = int(rng.integers(1, 13)), int(rng.integers(2, 5))
        D = rng.integers(0, 2 << 32, (n, L)).astype(np.int64)
        if trial % 3 == 0:                                      # ties everywhere
            D = (D >> 31) << 31
        if trial % 5 == 0:                                      # separated clusters: one cheap label per site
            D[np.arange(n), rng.integers(0, L, n)] >>= 8
        h = int(rng.integers(0, 3)) * int(rng.integers(0, 4 << 32))
        lab, e, opened = oracle.greedy_labeling(D, h)
        ref = transcription(D, h)
        assert np.array_equal(lab, ref), (trial, lab, ref)
        assert e == energy(D, h, lab) and opened >= len(set(lab.tolist()))
        if L ** n <= 30000:
            best = min(energy(D, h, np.array(c, dtype=np.int32)) for c in itertools.product(range(L), repeat=n))
            assert e >= best
            optimal += e == best
            if h == 0:
                assert e == best
    assert optimal > 100          # the heuristic finds the optimum on most of these small instances
    # golden case readable by hand: two sites, label 1 is cheaper for both but costs a second opening
    D = np.array([[10, 4], [10, 4]], dtype=np.int64) << 32
    lab, e, opened = oracle.greedy_labeling(D, 3 << 32)
    assert lab.tolist() == [1, 1] and opened == 1 and e == (8 + 3) << 32
    D = np.array([[1, 9], [9, 1]], dtype=np.int64) << 32
    assert oracle.greedy_labeling(D, 20 << 32)[0].tolist() == [0, 0]      # a second label is not worth 20
    assert oracle.greedy_labeling(D, 2 << 32)[0].tolist() == [0, 1]


def test_round2_golden_vectors(oracle):
    """tests/golden/kat_r2.npz (make_golden_r2.py): greedy labelling, PROSAC growth function, sampler draws for fixed seeds.
    Regression fixtures of the build - the reference holds none."""
    import os
    from pyprogressivex import _proposal
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_r2.npz"))
    for k in range(3):
        lab, e, opened = oracle.greedy_labeling(g[f"greedy{k}_D"], oracle.quantize(float(g[f"greedy{k}_h"][0])))
        assert np.array_equal(lab, g[f"greedy{k}_labels"]) and e == int(g[f"greedy{k}_energy"][0]) and opened == int(g[f"greedy{k}_opened"][0])
    gf = _proposal.prosac_growth_function(249, 7, 100000)
    assert np.array_equal(gf, g["prosac_growth_249_7"])
    # properties of T'_n: 1 for n <= m, strictly increasing afterwards, T'_N close to T_N (the last subset is drawn T_N times)
    assert np.all(gf[:7] == 1) and np.all(np.diff(gf[6:]) >= 1) and 0.9e5 < gf[-1] < 1.1e5
    assert np.array_equal(_proposal.prosac_growth_function(2000, 4, 100000)[::50], g["prosac_growth_2000_4"])
    assert np.array_equal(_proposal.ProsacSampler(300, np.random.default_rng(1)).draw(400, 4), g["prosac_draw"])
    pn = _proposal.ProgressiveNapsacSampler(300, np.random.default_rng(2), g["pnapsac_pts"], (640, 480, 640, 480), 4)
    draw = pn.draw(400, 4)
    assert np.array_equal(draw, g["pnapsac_draw"])
    # the first blend * n samples are local: centre k - 1 in the last column, companions from the centre's grid cells
    assert np.array_equal(draw[:150, 3][:100], np.arange(100))
    cid, members = pn.cells[-1]                     # coarsest layer (2 cells per dimension)
    local = sum(set(r[:3]).issubset(set(members[int(cid[r[3]])].tolist())) for r in draw[:150])
    assert local >= 100                             # the rest fell through to the global PROSAC sampler


def test_jacobi_eigen_solver_against_lapack_and_by_hand(oracle):
    """Round 6: the refits' small dense solve restated as cyclic Jacobi (pgxo_eigh_smallest; the device kernel runs the same operation
    order and must return the same bits: tests/test_gpu_parity.py).  Against numpy's LAPACK, tolerance stated: the eigenVALUE to
    64 eps relative to the spectral radius; the sign-normalised eigenVECTOR to 1e-12 when the smallest eigenvalue is separated from the
    next by >= 1e-3 of the spectral radius (the refits' A^T A of noisy data), and always an eigenvector in the residual sense
    |A v - val v| <= 1e-13 |A|.  Known answers: diag(3, 1, 2) -> e_2; [[2, 1], [1, 2]] -> (1, -1) / sqrt 2 with value 1."""
    vec, val, sw = oracle.eigh_smallest(np.array([np.diag([3.0, 1.0, 2.0])]))
    assert np.array_equal(vec[0], [0.0, 1.0, 0.0]) and val[0] == 1.0 and sw[0] == 0
    vec, val, _ = oracle.eigh_smallest(np.array([[[2.0, 1.0], [1.0, 2.0]]]))
    assert abs(val[0] - 1.0) < 1e-15 and np.allclose(np.abs(vec[0]), np.sqrt(0.5), atol=1e-15) and vec[0][0] * vec[0][1] < 0
    rng = np.random.default_rng(12)
    for q in (2, 3, 7, 9):
        X = rng.standard_normal((300, 30, q))
        A = np.einsum("bni,bnj->bij", X, X)
        A[:40] *= 1e-9
        A[40:80] *= 1e9
        A[80:100, :, 0] *= 1e-4              # badly scaled columns (what Hartley normalisation is there to avoid)
        A[80:100, 0, :] *= 1e-4
        vec, val, sw = oracle.eigh_smallest(A)
        w, V = np.linalg.eigh(A)
        rad = np.abs(w).max(axis=1)
        assert (np.abs(val - w[:, 0]) <= 64 * 2.3e-16 * rad).all()
        res = np.abs(np.einsum("bij,bj->bi", A, vec) - val[:, None] * vec).max(axis=1)
        assert (res <= 1e-13 * rad).all() and np.allclose((vec * vec).sum(1), 1.0, atol=1e-14)
        gap = (w[:, 1] - w[:, 0]) >= 1e-3 * rad
        sgn = np.sign((V[:, :, 0] * vec).sum(axis=1))
        assert gap.sum() > 100 and np.abs(vec * sgn[:, None] - V[:, :, 0])[gap].max() <= 1e-12
        assert sw.max() <= 12
    # NaN / Inf / zero matrices come back without hanging (NaN rows stay NaN, the zero matrix gives e_0 with value 0)
    bad = np.zeros((3, 3, 3))
    bad[0, 1, 1] = np.nan
    bad[1, 0, 2] = bad[1, 2, 0] = np.inf
    vec, val, sw = oracle.eigh_smallest(bad)
    assert np.array_equal(vec[2], [1.0, 0.0, 0.0]) and val[2] == 0.0


# ---- the 3-D point-cloud types (planes, type 6; spheres, type 8): the oracle rows against exact arithmetic --------------------------
GOLDEN_3D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_3d_v1.npz")


def test_model_dims_agree_with_the_product_table_for_every_type_number(oracle):
    """pgxo_model_dims against pyprogressivex._lib.MODEL_TABLE (the numbers of csrc/residuals.hip.h) for 0 .. 10: the same types
    exist on both sides (10 known; 7 and 9 do not exist), with the same point and parameter dimensions and, where the oracle has a
    solver, the same sample size"""
    from pyprogressivex import _lib
    assert sum(t in _lib.MODEL_TABLE for t in range(11)) == 9 and 7 not in _lib.MODEL_TABLE and 9 not in _lib.MODEL_TABLE
    for t in range(11):
        dims = oracle.model_dims(t)
        if t in _lib.MODEL_TABLE:
            assert dims == _lib.MODEL_TABLE[t][:2] == (oracle.POINT_DIM[t], oracle.PARAM_DIM[t]), t
            assert oracle.SAMPLE_SIZE.get(t, 0) == _lib.MODEL_TABLE[t][2], t
        else:
            assert dims is None and t not in oracle.POINT_DIM and t not in oracle.PARAM_DIM, t
    assert oracle.model_dims(-1) is None and np.isnan(oracle.squared_residuals(7, np.zeros((0, 3)), np.zeros(4))).all()
    assert (oracle.PLANE3D, oracle.SPHERE3D) == (_lib.PLANE3D, _lib.SPHERE3D) == (6, 8)
    assert oracle.GRAM_SPHERE == _lib.GRAM_SPHERE and oracle.GRAM_AFFINE == _lib.GRAM_AFFINE
    assert oracle.CIRCLE2D == _lib.CIRCLE2D == 10 and oracle.GRAM_CIRCLE == _lib.GRAM_CIRCLE == 6
    assert oracle.model_dims(11) is None and np.isnan(oracle.squared_residuals(9, np.zeros((0, 2)), np.zeros(3))).all()


@pytest.mark.parametrize("name", list(MODEL_CASES_3D) + list(MODEL_CASES_2D))
def test_plain_residual_of_the_3d_types_is_not_the_root_of_the_square(oracle, name):
    """pgxo_residual (PEARL's refit sums) returns r itself for the types whose squared residual is defined as r * r, as the device's
    Residual<>::plain does.  In binary floating point sqrt(fl(r * r)) == r as long as r * r neither overflows nor underflows, so the
    two readings part only at the ends of the range: r = 1e-170 (r * r = 0) and r = 1e200 (r * r = inf).  Both are pinned here; in
    range, r * r is the squared residual bit for bit and agrees with exact arithmetic."""
    mt, pts, models, thr = make_case(name, 200, 3, seed=3)
    for model in models:
        sq = oracle.squared_residuals(mt, pts, model)
        for i in range(pts.shape[0]):
            r = oracle.residual(mt, pts[i], model)
            assert r >= 0.0 and r * r == sq[i] and np.sqrt(sq[i]) == r
            ex = float(_exact_sq(name, pts[i], model))
            assert abs(r * r - ex) <= 1e-9 * max(abs(ex), 1e-30) + 1e-18 * max(1.0, abs(ex))
    if name == "plane":      # the plane z = 0 and points 1e-170 / 1e200 above it
        cases = [([0.0, 0.0, 1e-170], [0.0, 0.0, 1.0, 0.0], 1e-170), ([0.0, 0.0, 1e200], [0.0, 0.0, 1.0, 0.0], 1e200)]
    elif name == "circle":   # the centre of a circle of radius 1e-170 / 1e200
        cases = [([1.0, 2.0], [1.0, 2.0, 1e-170], 1e-170), ([1.0, 2.0], [1.0, 2.0, 1e200], 1e200)]
    else:                    # the centre of a sphere of radius 1e-170 / 1e200
        cases = [([1.0, 2.0, 3.0], [1.0, 2.0, 3.0, 1e-170], 1e-170), ([1.0, 2.0, 3.0], [1.0, 2.0, 3.0, 1e200], 1e200)]
    for p, m, r in cases:
        sq = oracle.squared_residuals(mt, [p], m)[0]
        assert oracle.residual(mt, p, m) == r and np.sqrt(sq) != r and sq in (0.0, np.inf)
        assert oracle.residual_sum(mt, np.array([p, p]), m, np.zeros(2, np.int32), 0) == r + r
    labels = np.arange(pts.shape[0], dtype=np.int32) % 3
    seq = 0.0
    for i in np.nonzero(labels == 1)[0]:
        seq += oracle.residual(mt, pts[i], models[0])
    assert oracle.residual_sum(mt, pts, models[0], labels, 1) == seq


def _exact_circumsphere(P):
    """centre (Fractions), squared radius (Fraction) and squared conditioning det^2 / (|a1|^2 |a2|^2 |a3|^2) of the sphere through
    the four points P [4][3] of doubles, by Cramer's rule in exact rational arithmetic; None for coplanar points"""
    P = [[Fr(float(v)) for v in row] for row in P]
    a = [[P[i][k] - P[0][k] for k in range(3)] for i in (1, 2, 3)]
    h = [sum(v * v for v in ai) / 2 for ai in a]

    def det3(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    det = det3(a)
    if det == 0:
        return None
    e = []
    for k in range(3):
        mk = [[h[i] if j == k else a[i][j] for j in range(3)] for i in range(3)]
        e.append(det3(mk) / det)
    cond2 = det * det / (sum(v * v for v in a[0]) * sum(v * v for v in a[1]) * sum(v * v for v in a[2]))
    return [P[0][k] + e[k] for k in range(3)], sum(v * v for v in e), cond2


def _sqrt_fraction(q, digits=60):
    with decimal.localcontext() as c:
        c.prec = digits
        return Fr(*(decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).sqrt().as_integer_ratio())


def test_sphere_solver_against_exact_rational_arithmetic(oracle):
    """The oracle's 4-point sphere solver against the circumsphere in exact arithmetic (the centre of four points with double
    coordinates is a rational number; the radius is the root of one, taken to 60 digits): centre and radius within 1e-9 relative
    on every sample whose conditioning |det(a1, a2, a3)| / (|a1| |a2| |a3|) is at least 1e-3; at most 5 % of the samples may fall
    under that rule.  400 samples of a four-sphere scene, half from one sphere and half anywhere."""
    from pyprogressivex import datasets
    pts, gt, _ = datasets.make_spheres(500, 4, 500, seed=0)
    rng = np.random.default_rng(0)
    one = np.nonzero(gt == 1)[0]
    smp = np.vstack([np.stack([rng.choice(one, 4, replace=False) for _ in range(200)]),
                     np.stack([rng.choice(len(pts), 4, replace=False) for _ in range(200)])]).astype(np.int32)
    got = oracle.solve_minimal(oracle.SPHERE3D, pts, smp)
    skipped, worst_c, worst_r = 0, 0.0, 0.0
    for s in range(len(smp)):
        ex = _exact_circumsphere(pts[smp[s]])
        if ex is None or ex[2] < Fr(1, 10 ** 6):
            skipped += 1
            continue
        c, r2, _ = ex
        r = _sqrt_fraction(r2)
        assert np.isfinite(got[s]).all(), s
        ec = max(abs(Fr(float(got[s, k])) - c[k]) for k in range(3)) / max(abs(v) for v in c)
        er = abs(Fr(float(got[s, 3])) - r) / r
        worst_c, worst_r = max(worst_c, float(ec)), max(worst_r, float(er))
        assert ec <= Fr(1, 10 ** 9) and er <= Fr(1, 10 ** 9), (s, float(ec), float(er))
    print(f"sphere solver: {skipped} of {len(smp)} samples under the conditioning rule, worst relative error centre {worst_c:.3g} radius {worst_r:.3g}")
    assert skipped <= 0.05 * len(smp)
    # every point of a sample lies on its sphere: the exact residual of the oracle's model is at rounding level
    for s in range(0, 200, 20):
        for i in smp[s]:
            assert float(_exact_sq("sphere", pts[i], got[s])) <= (1e-9 * max(1.0, abs(got[s]).max())) ** 2


def test_plane_solver_against_exact_rational_arithmetic(oracle):
    """The oracle's 3-point plane solver: the exact (rational) residual of the three sample points under the returned model and
    | |n|^2 - 1 | are bounded by 1e-9 x the coordinate scale (10)"""
    from pyprogressivex import datasets
    pts, gt, _ = datasets.make_planes(500, 4, 500, seed=0)
    rng = np.random.default_rng(1)
    one = np.nonzero(gt == 1)[0]
    smp = np.vstack([np.stack([rng.choice(one, 3, replace=False) for _ in range(150)]),
                     np.stack([rng.choice(len(pts), 3, replace=False) for _ in range(150)])]).astype(np.int32)
    got = oracle.solve_minimal(oracle.PLANE3D, pts, smp)
    scale = float(np.abs(pts).max())
    assert 1.0 <= scale <= 10.0 + 1.0
    worst_r, worst_n = 0.0, 0.0
    for s in range(len(smp)):
        assert np.isfinite(got[s]).all()
        m = [Fr(float(v)) for v in got[s]]
        for i in smp[s]:
            p = [Fr(float(v)) for v in pts[i]]
            worst_r = max(worst_r, abs(float(m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3])))
        worst_n = max(worst_n, abs(float(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] - 1)))
    print(f"plane solver: worst exact residual of a sample point {worst_r:.3g}, worst | |n|^2 - 1 | {worst_n:.3g}")
    assert worst_r <= 1e-9 * scale and worst_n <= 1e-9 * scale


def test_3d_solvers_hand_checked_degenerate_and_radius_range(oracle):
    O = oracle
    pts = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, -1.0, 0], [2.0, 0, 0], [3.0, 0, 0], [0, 0, 0],
                    [np.nan, 0, 0], [np.inf, 1, 1], [0, 0, 5.0]])
    # the unit sphere about the origin through four of its points; the plane z = 0 through three of them
    m = O.solve_minimal(O.SPHERE3D, pts, np.array([[0, 1, 2, 3]], np.int32))
    assert m[0].tolist() == [0.0, 0.0, 0.0, 1.0]
    m = O.solve_minimal(O.PLANE3D, pts, np.array([[0, 1, 2], [0, 2, 1]], np.int32))
    assert np.abs(m[0]).tolist() == [0.0, 0.0, 1.0, 0.0] and np.abs(m[1]).tolist() == [0.0, 0.0, 1.0, 0.0] and m[0][2] == -m[1][2]
    # plane: collinear, coincident, out-of-range index, NaN and Inf coordinates -> NaN rows
    bad = O.solve_minimal(O.PLANE3D, pts, np.array([[0, 5, 6], [0, 0, 2], [0, 1, 11], [0, -1, 2], [0, 1, 8], [0, 1, 9]], np.int32))
    assert np.isnan(bad).all()
    # sphere: coplanar (four points of z = 0), coincident, out-of-range, NaN and Inf -> NaN rows
    bad = O.solve_minimal(O.SPHERE3D, pts, np.array([[0, 1, 2, 4], [0, 0, 2, 3], [0, 1, 2, 11], [-1, 1, 2, 3], [0, 1, 2, 8], [0, 1, 2, 9]], np.int32))
    assert np.isnan(bad).all()
    # the radius range is inclusive at both ends: the sphere through (+-1, 0, 0), (0, 1, 0), (0, 0, 5) has r = 2.6 about (0, 0, 2.4)
    smp = np.array([[0, 1, 2, 10], [0, 1, 2, 3]], np.int32)
    free = O.solve_minimal(O.SPHERE3D, pts, smp)
    assert np.allclose(free[0], [0.0, 0.0, 2.4, 2.6], rtol=1e-15, atol=1e-15) and free[1, 3] == 1.0
    r = float(free[0, 3])
    for rng_, keep in (((r, r), [True, False]), ((1.0, r), [True, True]), ((1.0, np.nextafter(r, 0.0)), [False, True]),
                       ((np.nextafter(1.0, 2.0), np.inf), [True, False]), ((0.0, 1.0), [False, True]), ((0.0, np.inf), [True, True])):
        out = O.solve_minimal(O.SPHERE3D, pts, smp, radius_range=rng_)
        assert (~np.isnan(out[:, 0])).tolist() == keep, rng_
        assert np.array_equal(out[keep], free[keep])
    for bad_range in ((-1.0, 2.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError):
            O.solve_minimal(O.SPHERE3D, pts, smp, radius_range=bad_range)
    # the plane solver does not read the range
    assert np.array_equal(O.solve_minimal(O.PLANE3D, pts, smp[:, :3].copy(), radius_range=(5.0, 6.0)), O.solve_minimal(O.PLANE3D, pts, smp[:, :3].copy()))


def test_3d_solvers_are_bitwise_the_host_estimators(oracle):
    """two restatements of the operation order in include/pgx.h (C here, numpy in _estimators.py) return the same bits and the same
    set of samples without a model, with and without a radius range"""
    from pyprogressivex import _estimators, datasets
    rng = np.random.default_rng(5)
    pts, _, _ = datasets.make_planes(300, 3, 300, seed=2)
    smp = rng.integers(0, len(pts), (600, 3)).astype(np.int32)
    smp[:10, 2] = smp[:10, 0]
    ref, src = _estimators.PlaneEstimator().minimal(pts, smp)
    got = oracle.solve_minimal(oracle.PLANE3D, pts, smp)
    assert np.isnan(got[:10]).all() and np.array_equal(np.nonzero(~np.isnan(got[:, 0]))[0], src) and np.array_equal(got[src], ref)
    pts, _, _ = datasets.make_spheres(300, 3, 300, seed=2)
    smp = rng.integers(0, len(pts), (600, 4)).astype(np.int32)
    smp[:10, 3] = smp[:10, 1]
    for rr in ((0.0, np.inf), (0.4, 2.0)):
        est = _estimators.SphereEstimator()
        est.radius_range = rr
        ref, src = est.minimal(pts, smp)
        got = oracle.solve_minimal(oracle.SPHERE3D, pts, smp, radius_range=rr)
        # a repeated point makes det cancel to 0 only up to rounding: where it does not, the numerators cancel exactly (n2 = 0,
        # n3 = -n1, h3 = h1), so the row is the sphere of radius 0 at p0 - which a range with rmin > 0 removes
        assert (np.isnan(got[:10, 3]) | (got[:10, 3] == 0.0)).all() and (rr[0] == 0.0 or np.isnan(got[:10]).all())
        assert np.array_equal(np.nonzero(~np.isnan(got[:, 0]))[0], src) and np.array_equal(got[src], ref)
        assert 10 < len(src) < 590 or rr[1] == np.inf          # the range keeps some samples and removes others


def test_gram_sphere_rows_hand_checked_and_affine_on_3d_points(oracle):
    O = oracle
    pts = np.array([[3.0, 2.0, 1.0], [1.0, 2.0, 5.0]])
    # o = (1, 2, 1), s = 2: rows (1, 1, 0, 0, 1) and (1, 0, 0, 2, 4)
    blocks, bad = O.gram_rows(O.GRAM_SPHERE, pts, [1.0, 2.0, 1.0, 2.0])
    assert len(blocks) == 1 and not bad.any() and blocks[0].tolist() == [[1.0, 1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0, 4.0]]
    G, cnt, nbad = O.gram(O.GRAM_SPHERE, pts, [0, 1], params=[1.0, 2.0, 1.0, 2.0])
    assert cnt == 2 and nbad == 0 and G.tolist() == [[2, 1, 0, 2, 5], [1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [2, 0, 0, 4, 8], [5, 1, 0, 8, 17]]
    G, cnt, nbad = O.gram(O.GRAM_SPHERE, pts, [0, 1], params=[1.0, 2.0, 1.0, 2.0], weights=np.array([2.0, 3.0]), wpow=1)
    assert G[0].tolist() == [5.0, 2.0, 0.0, 6.0, 14.0]
    # GRAM_AFFINE needs nothing for 3-column points: rows (1, x, y, z)
    G, cnt, nbad = O.gram(O.GRAM_AFFINE, pts, [0, 1])
    assert G.shape == (4, 4) and G[0].tolist() == [2.0, 4.0, 4.0, 6.0] and G[3, 3] == 26.0


@pytest.mark.parametrize("offset", [0.0, 1e3, 1e6])
def test_refits_on_the_oracle_rows_recover_noise_free_structures(oracle, offset):
    """PlaneEstimator / SphereEstimator driven by the ORACLE's Gram rows recover a known plane / sphere from noise-free points, also
    1e3 and 1e6 from the origin (the case DESIGN.md 4.6 gives for the normalised sphere rows).

    Bounds, from the arithmetic and not from the results.  The inputs themselves are rounded to ulp(|o|), and both refits solve a
    small eigenproblem whose condition number on these scenes is of the order 10^2, so neither can do better than ~10^2 ulp(|o|): the
    floor is set to 10^3 ulp(max(1, |o|)).  The SPHERE rows are centred and scaled before they are squared, so that floor is its
    whole bound (1.2e-7 at 1e6; measured 3e-12).  The PLANE refit forms its scatter as G - W mean mean^T from the UN-centred sums of
    GRAM_AFFINE: the entries of both terms are ~|o|^2, each carries a few eps of relative rounding, so the scatter is known to
    ~4 eps |o|^2 and the normal to that over the smallest in-plane variance (4^2 / 12 for this patch): 1.5e-3 at 1e6 (measured
    3e-4 .. 5e-4 in the normal, 1.4e-3 in the residual of a patch corner), 1.5e-9 at 1e3, rounding level at the origin.  That
    loss is a property of the plane refit, stated in DESIGN.md 4.5: a cloud in map coordinates should be shifted to its centroid."""
    from oracle_ctx import OracleContext
    from pyprogressivex import _estimators
    rng = np.random.default_rng(2)
    ctx = OracleContext()
    o = np.array([offset, -offset, 0.5 * offset])
    floor = 1e3 * np.spacing(max(1.0, offset))
    # plane: unit normal n through c, a 4 x 4 patch
    nrm = np.array([2.0, -1.0, 2.0]) / 3.0
    e1 = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
    e2 = np.cross(nrm, e1)
    st = rng.uniform(-2.0, 2.0, (300, 2))
    c = o + np.array([1.0, 2.0, 3.0])
    pts = c + st[:, :1] * e1 + st[:, 1:] * e2
    plane_bound = 4.0 * np.finfo(np.float64).eps * float(c @ c) / (16.0 / 12.0) + floor
    ctx.set_points(oracle.PLANE3D, pts)
    for w in (None, rng.random(300) + 0.5):
        fit = _estimators.PlaneEstimator().nonminimal(ctx, ("index", np.arange(300)), w)
        assert len(fit) == 1
        m = fit[0] * np.sign(fit[0][:3] @ nrm)
        err_n = np.abs(m[:3] - nrm).max()
        err_r = np.sqrt(oracle.squared_residuals(oracle.PLANE3D, pts, fit[0])).max()
        print(f"plane refit at offset {offset:g}: normal error {err_n:.3g}, worst residual {err_r:.3g} (bound {plane_bound:.3g})")
        assert abs(m[:3] @ m[:3] - 1.0) <= 1e-12
        assert err_n <= plane_bound and err_r <= 2.0 * np.sqrt(2.0) * plane_bound + floor     # a corner lies 2 sqrt(2) from the centre
    # sphere: radius 1.5 about c, the cap z > 0.3 r and beyond
    d = rng.normal(size=(400, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.3
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = c + 1.5 * d
    ctx.set_points(oracle.SPHERE3D, pts)
    for w in (None, rng.random(400) + 0.5):
        fit = _estimators.SphereEstimator().nonminimal(ctx, ("index", np.arange(400)), w)
        assert len(fit) == 1
        err_c, err_r = np.abs(fit[0][:3] - c).max(), abs(fit[0][3] - 1.5)
        print(f"sphere refit at offset {offset:g}: centre error {err_c:.3g}, radius error {err_r:.3g} (bound {floor:.3g})")
        assert err_c <= floor and err_r <= floor
    sel = np.arange(0, 400, 2)
    ctx.set_labels((np.arange(400) % 2).astype(np.int32))
    a = _estimators.SphereEstimator().nonminimal(ctx, ("label", 0), None)
    b = _estimators.SphereEstimator().nonminimal(ctx, ("index", sel), None)
    assert np.array_equal(a[0], b[0])


def test_golden_3d_rows(oracle):
    """the committed known answers of the plane / sphere rows (tests/golden/make_golden_3d.py): residuals, score table, preference,
    unary table, solver outputs (with a radius range) bit for bit, Gram matrices to 1e-12"""
    g = np.load(GOLDEN_3D)
    for name, mt in MODEL_CASES_3D.items():
        pts, models, thr, comp = g[f"{name}_pts"], g[f"{name}_models"], float(g[f"{name}_thr"][0]), g[f"{name}_comp"]
        T2 = 2.25 * thr * thr
        assert np.array_equal(oracle.squared_residuals(mt, pts, models[0]), g[f"{name}_sq0"])
        assert np.array_equal(np.array([oracle.residual(mt, p, models[0]) for p in pts]), g[f"{name}_plain0"])
        sc = oracle.score(mt, pts, models, T2, compound=comp, has_compound=True, exponent=2, want_masks=True)
        for k in ("counts", "values", "shared", "scores", "masks"):
            assert np.array_equal(sc[k], g[f"{name}_{k}"]), k
        assert sc["counts"].max() > 30
        assert np.array_equal(oracle.preference(mt, pts, models[0], T2), g[f"{name}_pref0"])
        assert np.array_equal(oracle.unary_q(mt, pts, models[:3], thr, 0.1), g[f"{name}_unary_q"])
        assert np.array_equal(oracle.solve_minimal(mt, pts, g[f"{name}_samples"]), g[f"{name}_solved"], equal_nan=True)
        for kind in (oracle.GRAM_AFFINE,) + ((oracle.GRAM_SPHERE,) if name == "sphere" else ()):
            prm = g["sphere_gram_params"] if kind == oracle.GRAM_SPHERE else None
            G, cnt, bad = oracle.gram(kind, pts, g[f"{name}_idx"], params=prm, weights=g[f"{name}_w"], wpow=1)
            ref = g[f"{name}_G{kind}"]
            assert cnt == 120 and bad == 0 and np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
    rr = g["sphere_radius_range"]
    out = oracle.solve_minimal(oracle.SPHERE3D, g["sphere_pts"], g["sphere_samples"], radius_range=(float(rr[0]), float(rr[1])))
    assert np.array_equal(out, g["sphere_solved_ranged"], equal_nan=True)
    assert np.isnan(out[:, 0]).sum() > np.isnan(g["sphere_solved"][:, 0]).sum()


# ---- the 2-D circle (type 10): the same evidence as the sphere's --------------------------------------------------------------------
def _exact_circumcircle(P):
    """centre (Fractions), squared radius (Fraction) and squared conditioning det^2 / (|a1|^2 |a2|^2) of the circle through the three
    points P [3][2] of doubles, by Cramer's rule in exact rational arithmetic; None for collinear points"""
    P = [[Fr(float(v)) for v in row] for row in P]
    a = [[P[i][k] - P[0][k] for k in range(2)] for i in (1, 2)]
    h = [(ai[0] * ai[0] + ai[1] * ai[1]) / 2 for ai in a]
    det = a[0][0] * a[1][1] - a[0][1] * a[1][0]
    if det == 0:
        return None
    e = [(h[0] * a[1][1] - h[1] * a[0][1]) / det, (a[0][0] * h[1] - a[1][0] * h[0]) / det]
    cond2 = det * det / ((a[0][0] ** 2 + a[0][1] ** 2) * (a[1][0] ** 2 + a[1][1] ** 2))
    return [P[0][0] + e[0], P[0][1] + e[1]], e[0] * e[0] + e[1] * e[1], cond2


def test_circle_solver_against_exact_rational_arithmetic(oracle):
    """The oracle's 3-point circle solver against the circumcircle in exact arithmetic (the centre of three points with double
    coordinates is a rational number; the radius is the root of one, taken to 60 digits): centre and radius within 1e-9 relative on
    every sample whose conditioning |det(a1, a2)| / (|a1| |a2|) is at least 1e-3; at most 5 % of the samples may fall under that
    rule.  400 samples of a four-circle scene, half from one circle and half anywhere."""
    from pyprogressivex import datasets
    pts, gt, _ = datasets.make_circles(500, 4, 500, seed=0)
    rng = np.random.default_rng(0)
    one = np.nonzero(gt == 1)[0]
    smp = np.vstack([np.stack([rng.choice(one, 3, replace=False) for _ in range(200)]),
                     np.stack([rng.choice(len(pts), 3, replace=False) for _ in range(200)])]).astype(np.int32)
    got = oracle.solve_minimal(oracle.CIRCLE2D, pts, smp)
    assert got.shape == (400, 3)
    skipped, worst_c, worst_r = 0, 0.0, 0.0
    for s in range(len(smp)):
        ex = _exact_circumcircle(pts[smp[s]])
        if ex is None or ex[2] < Fr(1, 10 ** 6):
            skipped += 1
            continue
        c, r2, _ = ex
        r = _sqrt_fraction(r2)
        assert np.isfinite(got[s]).all(), s
        ec = max(abs(Fr(float(got[s, k])) - c[k]) for k in range(2)) / max(abs(v) for v in c)
        er = abs(Fr(float(got[s, 2])) - r) / r
        worst_c, worst_r = max(worst_c, float(ec)), max(worst_r, float(er))
        assert ec <= Fr(1, 10 ** 9) and er <= Fr(1, 10 ** 9), (s, float(ec), float(er))
    print(f"circle solver: {skipped} of {len(smp)} samples under the conditioning rule, worst relative error centre {worst_c:.3g} radius {worst_r:.3g}")
    assert skipped <= 0.05 * len(smp)
    # every point of every sample lies on its circle: the exact residual of the oracle's model is at rounding level
    for s in range(len(smp)):
        if np.isfinite(got[s]).all():
            for i in smp[s]:
                assert float(_exact_sq("circle", pts[i], got[s])) <= (1e-9 * max(1.0, abs(got[s]).max())) ** 2, s


def test_circle_solver_hand_checked_degenerate_and_radius_range(oracle):
    """the solver's NaN cases with dyadic coordinates (every difference and product exact, so det == 0 exactly), the inclusive
    radius range, rmin == rmax, refused ranges"""
    O = oracle
    pts = np.array([[3.0, 2.0], [1.0, 4.0], [-1.0, 2.0], [1.0, 0.0],              # 0-3: the circle of radius 2 about (1, 2)
                    [0.5, 0.25], [1.5, 0.75], [3.5, 1.75],                       # 4-6: collinear
                    [np.nan, 0.0], [np.inf, 1.0],                                # 7, 8
                    [5.0, 0.0], [-5.0, 0.0], [0.0, 5.0],                         # 9-11: radius 5 about the origin
                    [1e200, 0.0], [0.0, 1e200], [-1e200, 0.0]])                  # 12-14: h overflows: a non-finite centre
    m = O.solve_minimal(O.CIRCLE2D, pts, np.array([[0, 1, 2], [3, 2, 1], [2, 3, 0]], np.int32))
    assert m.tolist() == [[1.0, 2.0, 2.0]] * 3
    # collinear, coincident (twice and three times the same point), out-of-range indices, NaN and Inf coordinates, overflow -> NaN rows
    bad = O.solve_minimal(O.CIRCLE2D, pts, np.array([[4, 5, 6], [6, 4, 5], [0, 0, 1], [1, 0, 0], [2, 2, 2], [0, 1, 15], [0, -1, 2],
                                                     [0, 1, 7], [0, 1, 8], [12, 13, 14]], np.int32))
    assert bad.shape == (10, 3) and np.isnan(bad).all()
    smp = np.array([[9, 10, 11], [0, 1, 2]], np.int32)            # radii 5 and 2
    free = O.solve_minimal(O.CIRCLE2D, pts, smp)
    assert free.tolist() == [[0.0, 0.0, 5.0], [1.0, 2.0, 2.0]]
    for rng_, keep in (((5.0, 5.0), [True, False]), ((2.0, 2.0), [False, True]), ((2.0, 5.0), [True, True]),
                       ((2.0, np.nextafter(5.0, 0.0)), [False, True]), ((np.nextafter(2.0, 3.0), np.inf), [True, False]),
                       ((0.0, 2.0), [False, True]), ((0.0, np.inf), [True, True]), ((3.0, 4.0), [False, False]),
                       ((6.0, 6.0), [False, False])):
        out = O.solve_minimal(O.CIRCLE2D, pts, smp, radius_range=rng_)
        assert (~np.isnan(out[:, 0])).tolist() == keep, rng_
        assert np.array_equal(out[keep], free[keep]) and np.isnan(out[~np.array(keep)]).all()
    for bad_range in ((-1.0, 2.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError):
            O.solve_minimal(O.CIRCLE2D, pts, smp, radius_range=bad_range)


def test_circle_solver_is_bitwise_the_host_estimator(oracle):
    """two restatements of the operation order csrc/solve.hip documents (C here, numpy in _estimators.py) return the same bits and
    the same set of samples without a model, with and without a radius range"""
    from pyprogressivex import _estimators, datasets
    rng = np.random.default_rng(6)
    pts, _, _ = datasets.make_circles(300, 3, 300, seed=2)
    smp = rng.integers(0, len(pts), (600, 3)).astype(np.int32)
    smp[:10, 2] = smp[:10, 0]
    for rr in ((0.0, np.inf), (60.0, 300.0)):
        est = _estimators.CircleEstimator()
        est.radius_range = rr
        ref, src = est.minimal(pts, smp)
        got = oracle.solve_minimal(oracle.CIRCLE2D, pts, smp, radius_range=rr)
        # a repeated point: a_2 = 0 exactly, so det = a_10 0 - a_11 0 = 0 exactly (unlike the sphere's 3 x 3 determinant)
        assert np.isnan(got[:10]).all()
        assert np.array_equal(np.nonzero(~np.isnan(got[:, 0]))[0], src) and np.array_equal(got[src], ref)
        assert 10 < len(src) < 590 or rr[1] == np.inf          # the range keeps some samples and removes others


def test_gram_circle_rows_hand_checked(oracle):
    O = oracle
    pts = np.array([[3.0, 2.0], [1.0, 6.0]])
    # o = (1, 2), s = 2: rows (1, 1, 0, 1) and (1, 0, 2, 4)
    blocks, bad = O.gram_rows(O.GRAM_CIRCLE, pts, [1.0, 2.0, 2.0])
    assert len(blocks) == 1 and not bad.any() and blocks[0].tolist() == [[1.0, 1.0, 0.0, 1.0], [1.0, 0.0, 2.0, 4.0]]
    G, cnt, nbad = O.gram(O.GRAM_CIRCLE, pts, [0, 1], params=[1.0, 2.0, 2.0])
    assert cnt == 2 and nbad == 0 and G.tolist() == [[2, 1, 2, 5], [1, 1, 0, 1], [2, 0, 4, 8], [5, 1, 8, 17]]
    G, cnt, nbad = O.gram(O.GRAM_CIRCLE, pts, [0, 1], params=[1.0, 2.0, 2.0], weights=np.array([2.0, 3.0]), wpow=1)
    assert G[0].tolist() == [5.0, 2.0, 6.0, 14.0]
    G, cnt, nbad = O.gram(O.GRAM_AFFINE, pts, [0, 1])
    assert G.shape == (3, 3) and G[0].tolist() == [2.0, 4.0, 8.0]


@pytest.mark.parametrize("offset", [0.0, 1e3, 1e6])
def test_circle_refit_on_the_oracle_rows_recovers_a_noise_free_circle(oracle, offset):
    """CircleEstimator driven by the ORACLE's Gram rows (GRAM_AFFINE, then GRAM_CIRCLE on centred and scaled coordinates) recovers
    a known circle from noise-free points on three quarters of it, also 1e3 and 1e6 from the origin.  Bound as the sphere's
    (test_refits_on_the_oracle_rows_recover_noise_free_structures): the inputs are rounded to ulp(|o|) and the eigenproblem's
    condition number on such an arc is of the order 10^2, so the floor is 10^3 ulp(max(r, |o|)); the rows are centred before they
    are squared, so that floor is the whole bound."""
    from oracle_ctx import OracleContext
    from pyprogressivex import _estimators
    rng = np.random.default_rng(2)
    ctx = OracleContext()
    c = np.array([offset + 300.0, -offset + 200.0])
    phi = rng.uniform(0.0, 1.5 * np.pi, 400)
    pts = c + 75.0 * np.column_stack([np.cos(phi), np.sin(phi)])
    floor = 1e3 * np.spacing(max(75.0, offset + 300.0))
    ctx.set_points(oracle.CIRCLE2D, pts)
    for w in (None, rng.random(400) + 0.5):
        fit = _estimators.CircleEstimator().nonminimal(ctx, ("index", np.arange(400)), w)
        assert len(fit) == 1
        err_c, err_r = np.abs(fit[0][:2] - c).max(), abs(fit[0][2] - 75.0)
        print(f"circle refit at offset {offset:g}: centre error {err_c:.3g}, radius error {err_r:.3g} (bound {floor:.3g})")
        assert err_c <= floor and err_r <= floor
    ctx.set_labels((np.arange(400) % 2).astype(np.int32))
    a = _estimators.CircleEstimator().nonminimal(ctx, ("label", 0), None)
    b = _estimators.CircleEstimator().nonminimal(ctx, ("index", np.arange(0, 400, 2)), None)
    assert np.array_equal(a[0], b[0])


def test_golden_circle_rows(oracle):
    """the committed known answers of the circle rows (tests/golden/make_golden_circles.py): residuals, score table with masks,
    preference, unary table, residual sums, solver outputs without and with a radius range bit for bit, Gram matrices to 1e-12"""
    g = np.load(GOLDEN_CIRCLES)
    mt = MODEL_CASES_2D["circle"]
    pts, models, thr, comp = g["circle_pts"], g["circle_models"], float(g["circle_thr"][0]), g["circle_comp"]
    T2 = 2.25 * thr * thr
    assert pts.shape == (200, 2) and models.shape == (6, 3) and thr == 2.0
    assert np.array_equal(oracle.squared_residuals(mt, pts, models[0]), g["circle_sq0"])
    assert np.array_equal(np.array([oracle.residual(mt, p, models[0]) for p in pts]), g["circle_plain0"])
    sc = oracle.score(mt, pts, models, T2, compound=comp, has_compound=True, exponent=2, want_masks=True)
    for k in ("counts", "values", "shared", "scores", "masks"):
        assert np.array_equal(sc[k], g[f"circle_{k}"]), k
    assert sc["counts"].max() > 30
    assert np.array_equal(oracle.preference(mt, pts, models[0], T2), g["circle_pref0"])
    assert np.array_equal(oracle.unary_q(mt, pts, models[:3], thr, 0.1), g["circle_unary_q"])
    labels = g["circle_labels"]
    assert np.array_equal(np.array([oracle.residual_sum(mt, pts, models[k], labels, k) for k in range(3)]), g["circle_residual_sums"])
    assert np.array_equal(oracle.solve_minimal(mt, pts, g["circle_samples"]), g["circle_solved"], equal_nan=True)
    rr = g["circle_radius_range"]
    out = oracle.solve_minimal(mt, pts, g["circle_samples"], radius_range=(float(rr[0]), float(rr[1])))
    assert np.array_equal(out, g["circle_solved_ranged"], equal_nan=True)
    assert np.isnan(out[:, 0]).sum() > np.isnan(g["circle_solved"][:, 0]).sum() and (out[:, 2] == rr[1]).any()
    for kind in (oracle.GRAM_AFFINE, oracle.GRAM_CIRCLE):
        prm = g["circle_gram_params"] if kind == oracle.GRAM_CIRCLE else None
        G, cnt, bad = oracle.gram(kind, pts, g["circle_idx"], params=prm, weights=g["circle_w"], wpow=1)
        ref = g[f"circle_G{kind}"]
        assert cnt == 120 and bad == 0 and np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
