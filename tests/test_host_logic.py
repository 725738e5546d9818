"""Host control flow (ProgressiveX.run / Pearl.run / ProposalEngine / the five API functions) on a CPU-only box: the
package's GPU context is replaced by tests/oracle_ctx.OracleContext (test infrastructure).  Checks the reference's
output conventions and that the pipeline recovers the planted structures."""
import numpy as np
import pytest

import pyprogressivex as px
from oracle_ctx import OracleContext
from pyprogressivex import _api, datasets


@pytest.fixture()
def oracle_backend(monkeypatch):
    monkeypatch.setattr(_api, "_ctx", OracleContext())
    yield


def _me(labels, K, gt):
    pred = np.where(labels == K, 0, labels + 1)   # predicted outlier label K -> 0, model k -> k+1
    return datasets.misclassification(pred, gt)


def test_lines_pipeline(oracle_backend):
    pts, gt, _ = datasets.make_lines(n_per_line=150, n_lines=3, n_outliers=150, seed=0)
    L, lab = px.findLines(pts, np.array(0), 1000, 1000, threshold=2.0, conf=0.99, sampler_id=0, seed=1,
                          minimum_point_number=40)
    assert L.shape == (3, 3) and L.dtype == np.float64 and lab.dtype == np.int32 and lab.shape == (600,)
    assert lab.max() == 3 and _me(lab, 3, gt) < 0.05
    assert np.allclose(np.hypot(L[:, 0], L[:, 1]), 1.0)


def test_homography_pipeline_and_single_model_convention(oracle_backend):
    pts, gt, _ = datasets.make_homographies(n_per_plane=150, n_planes=2, n_outliers=150, seed=0)
    H, lab = px.findHomographies(pts, 1000, 1000, 1000, 1000, threshold=3.0, conf=0.99, sampler_id=3, seed=1,
                                 minimum_point_number=20)
    assert H.shape == (6, 3) and _me(lab, 2, gt) < 0.05
    # exactly one model: 0 = inlier, 1 = outlier (progressive_x.h:382-384)
    H1, lab1 = px.findHomographies(pts, 1000, 1000, 1000, 1000, threshold=3.0, conf=0.99, sampler_id=0, seed=1,
                                   minimum_point_number=20, maximum_model_number=1)
    assert H1.shape == (3, 3) and set(np.unique(lab1)) == {0, 1} and 120 < int((lab1 == 0).sum()) < 200
    # symmetric transfer error switch (north-star wording) recovers the same planes
    Hs, labs = px.findHomographies(pts, 1000, 1000, 1000, 1000, threshold=3.0, conf=0.99, sampler_id=0, seed=1,
                                   minimum_point_number=20, residual="symmetric")
    assert Hs.shape == (6, 3) and _me(labs, 2, gt) < 0.05


def test_philox_samplers_through_the_pipeline(oracle_backend):
    """sampler_rng="philox": the uniform (id 0), PROSAC (id 1) and NAPSAC (id 3) samplers on the in-repo counter-based generator, host side
    (the numpy restatement; the GPU context draws the same rows on the device - tests/test_gpu_api.py): same quality, and the
    stream is a function of the seed alone."""
    pts, gt, _ = datasets.make_homographies(n_per_plane=150, n_planes=2, n_outliers=150, seed=0)
    kw = dict(threshold=3.0, conf=0.99, seed=1, minimum_point_number=20, sampler_rng="philox")
    for sid in (0, 1, 3):
        H, lab = px.findHomographies(pts, 1000, 1000, 1000, 1000, sampler_id=sid, **kw)
        if sid == 1:     # PROSAC takes the index order for a quality order: here the first plane's points come first, it is found first
            assert H.shape[0] >= 3 and np.mean(lab[:150] == 0) > 0.9
        else:
            assert H.shape == (6, 3) and _me(lab, 2, gt) < 0.05, sid
        H2, lab2 = px.findHomographies(pts, 1000, 1000, 1000, 1000, sampler_id=sid, **kw)
        assert np.array_equal(H, H2) and np.array_equal(lab, lab2)
    # P-NAPSAC (id 2): sequential per-point state - drawn by libpgx's host code (csrc/sampler_host.hip) from the same generator
    H3, lab3 = px.findHomographies(pts, 1000, 1000, 1000, 1000, sampler_id=2, **kw)
    assert H3.shape[0] >= 3
    H4, lab4 = px.findHomographies(pts, 1000, 1000, 1000, 1000, sampler_id=2, **kw)
    assert np.array_equal(H3, H4) and np.array_equal(lab3, lab4)


def test_two_view_motion_pipeline(oracle_backend):
    # the epipolar constraint is weak (uniform outliers often fit, small spurious instances survive): few outliers and
    # a minimum instance size of 80 make the outcome stable across seeds (ME 0.08-0.15 for seeds 1-5)
    pts, gt, _ = datasets.make_two_view_motions(n_per_motion=150, n_motions=2, n_outliers=20, seed=0)
    F, lab = px.findTwoViewMotions(pts, 1000, 1000, 1000, 1000, threshold=0.5, conf=0.99, sampler_id=0, seed=1,
                                   minimum_point_number=80, max_iters=1500)
    assert F.shape == (6, 3)
    assert _me(lab, 2, gt) < 0.25


def test_pose_pipeline(oracle_backend, capsys):
    x1, x2, K, gt, poses = datasets.make_poses(n_per_object=200, n_objects=2, n_outliers=100, seed=0)
    P, lab = px.find6DPoses(x1, x2, K, seed=1, minimum_point_number=20)
    assert "Neighborhood calculation time" in capsys.readouterr().out       # progressivex_python.cpp:109
    assert P.shape == (6, 4) and _me(lab, 2, gt) < 0.05
    # recovered poses are close to the planted ones (rotation < 1 deg, translation < 5 mm)
    for k in range(2):
        Pk = P[3 * k: 3 * k + 3]
        err = min(np.degrees(np.arccos(np.clip((np.trace(Pk[:, :3].T @ g.reshape(3, 4)[:, :3]) - 1) / 2, -1, 1)))
                  for g in poses)
        assert err < 1.0


def test_vanishing_point_pipeline_with_weights(oracle_backend):
    pts, gt, _ = datasets.make_vanishing_points(n_inliers=450, n_vps=3, n_outliers=150, seed=0)
    w = np.ones(600)
    V, lab = px.findVanishingPoints(pts, w, 1000, 1000, threshold=1.5, conf=0.99, sampler_id=0, seed=1,
                                    minimum_point_number=30)
    assert V.shape == (3, 3) and _me(lab, 3, gt) < 0.1
    assert np.allclose(np.linalg.norm(V, axis=1), 1.0)


def test_spatial_coherence_path_runs(oracle_backend):
    pts, gt, _ = datasets.make_lines(n_per_line=120, n_lines=2, n_outliers=100, seed=3)
    L, lab = px.findLines(pts, np.array(0), 1000, 1000, threshold=2.0, conf=0.99, sampler_id=2, seed=2,
                          minimum_point_number=30, spatial_coherence_weight=0.02, neighborhood_ball_radius=20.0)
    assert L.shape == (2, 3) and _me(lab, 2, gt) < 0.1


def test_reference_quirks(oracle_backend):
    from pyprogressivex import _engine
    # scoring exponent is truncated to int (setExponent(const int), scoring_function_with_compound_model.h:39)
    pxr = _engine.ProgressiveX(OracleContext(), None, np.zeros((4, 2)), None, None, _engine.MultiModelSettings(),
                               scoring_exponent=2.5)
    assert pxr.scoring_exponent == 2
    s = _engine.MultiModelSettings()
    assert (s.minimum_number_of_inliers, s.max_proposal_number_without_change, s.max_iteration_number,
            s.max_local_optimization_number, s.max_outer_iterations) == (20, 10, 5000, 50, 10)


# ----------------------------------------------------------------------------------------------------------------------
# non-minimal refits: the algebra around the device's Gram pass (ctx.gram), here on the oracle-backed context
# ----------------------------------------------------------------------------------------------------------------------
def _octx(model_type, pts):
    from oracle_ctx import OracleContext
    ctx = OracleContext()
    ctx.set_points(model_type, pts)
    return ctx


def test_refits_recover_the_generating_models():
    from pyprogressivex import _estimators, _lib, datasets
    rng = np.random.default_rng(3)
    # line: total least squares
    t = rng.random(300) * 100
    pts = np.column_stack([t, 0.5 * t + 7.0]) + rng.normal(0, 1e-3, (300, 2))
    m = _estimators.LineEstimator().nonminimal(_octx(_lib.LINE2D, pts), ("index", np.arange(300)))[0]
    assert abs(abs(m[0] * 2 + m[1] * (-1)) / np.hypot(2, -1) - 0) < 1e-3 or abs(m[0] / m[1] + 0.5) < 1e-4
    assert np.abs(pts @ m[:2] + m[2]).max() < 1e-2
    # homography: exact correspondences -> H up to scale
    H = np.array([[1.1, 0.05, 20.0], [-0.03, 0.95, -12.0], [1e-5, -2e-5, 1.0]])
    a = rng.random((200, 2)) * 800
    b = np.column_stack([a, np.ones(200)]) @ H.T
    corr = np.column_stack([a, b[:, :2] / b[:, 2:]])
    ctx = _octx(_lib.HOMOGRAPHY, corr)
    ctx.set_labels(np.where(np.arange(200) < 150, 0, 1))
    h = _estimators.HomographyEstimator().nonminimal(ctx, ("label", 0))[0].reshape(3, 3)
    assert np.abs(h - H / H[2, 2]).max() < 1e-6 * np.abs(H).max()
    # fundamental matrix: x2^T F x1 = 0 on noise-free data
    pts2, gt2, _ = datasets.make_two_view_motions(seed=1)
    sel = np.nonzero(gt2 == 1)[0][:500]
    F = _estimators.FundamentalEstimator().nonminimal(_octx(_lib.FUNDAMENTAL, pts2), ("index", sel))[0].reshape(3, 3)
    x1 = np.column_stack([pts2[sel, :2], np.ones(len(sel))])
    x2 = np.column_stack([pts2[sel, 2:], np.ones(len(sel))])
    alg = np.abs(np.einsum("ij,jk,ik->i", x2, F, x1))
    assert np.median(alg) < 5e-3 and abs(np.linalg.det(F)) < 1e-9
    # PnP: Gauss-Newton from a perturbed pose converges back
    x1p, x2p, K, gtp, poses = datasets.make_poses(n_per_object=400, n_objects=2, n_outliers=0, seed=2)
    norm, f = datasets.normalize_pnp(x1p, x2p, K)
    sel = np.nonzero(gtp == 1)[0]
    P0 = poses[0].reshape(3, 4).copy()
    P0[:, 3] += np.array([2.0, -1.5, 4.0])
    est = _estimators.PnPEstimator()
    fit = est.nonminimal(_octx(_lib.PNP, norm), ("index", sel), init=P0.reshape(-1))[0].reshape(3, 4)
    assert np.abs(fit - poses[0].reshape(3, 4)).max() < 0.5      # mm-level on a 50 mm object at 600-900 mm, 1 px noise
    assert est.nonminimal(_octx(_lib.PNP, norm), ("index", sel), init=None) == []
    # vanishing point: segments through a common point
    vp = np.array([1500.0, -700.0])
    mid = rng.random((300, 2)) * 1000
    d = (vp - mid) / np.linalg.norm(vp - mid, axis=1, keepdims=True)
    segs = np.column_stack([mid - 30 * d, mid + 30 * d])
    v = _estimators.VanishingPointEstimator().nonminimal(_octx(_lib.VANISHING_POINT, segs), ("index", np.arange(300)))[0]
    assert abs(v[2]) > 0 and np.abs(v[:2] / v[2] - vp).max() < 1e-3


def test_batched_refits_equal_single_refits_on_the_oracle_context():
    # nonminimal_batch (one gram_batch call per Gram request of the refit) must return exactly what per-selection refits
    # (one gram call per request) return when both are fed by the same Gram provider; PnP's two statements agree to rounding
    from pyprogressivex import _estimators, _lib, datasets
    rng = np.random.default_rng(1)
    pts, gt, _ = datasets.make_homographies(n_per_plane=200, n_planes=2, n_outliers=50, seed=1)
    inl = np.nonzero(gt == 1)[0]
    picks = np.array([np.sort(rng.choice(inl, 28, replace=False)) for _ in range(6)])
    for est, mt in ((_estimators.HomographyEstimator(), _lib.HOMOGRAPHY), (_estimators.FundamentalEstimator(), _lib.FUNDAMENTAL)):
        ctx = _octx(mt, pts)
        w = rng.random(len(pts)) + 0.5
        batch = est.nonminimal_batch(ctx, picks, w)
        for b in range(len(picks)):
            single = est.nonminimal(ctx, ("index", picks[b]), w)
            assert len(single) == len(batch[b]) == 1 and np.array_equal(single[0], batch[b][0])
    # vanishing points (one Gram pass, stacked 3x3 eigh) and the symmetric-homography wrapper: bitwise as well
    segs, _, _ = datasets.make_vanishing_points(n_inliers=600, n_vps=3, n_outliers=200, seed=2)
    ctx = _octx(_lib.VANISHING_POINT, segs)
    est = _estimators.VanishingPointEstimator()
    vpicks = np.array([np.sort(rng.choice(len(segs), 14, replace=False)) for _ in range(7)])
    w = rng.random(len(segs)) + 0.5
    batch = est.nonminimal_batch(ctx, vpicks, w)
    for b in range(7):
        single = est.nonminimal(ctx, ("index", vpicks[b]), w)
        assert len(single) == len(batch[b]) == 1 and np.array_equal(single[0], batch[b][0])
    est = _estimators.SymmetricHomographyEstimator()
    ctx = _octx(_lib.HOMOGRAPHY_SYM, pts)
    batch = est.nonminimal_batch(ctx, picks, None)
    for b in range(len(picks)):
        single = est.nonminimal(ctx, ("index", picks[b]), None)
        assert len(single) == len(batch[b]) == 1 and np.array_equal(single[0], batch[b][0])
    # PnP: selections converge after different numbers of Gauss-Newton steps; an un-initialised fit returns nothing
    x1p, x2p, K, gtp, poses = datasets.make_poses(n_per_object=300, n_objects=1, n_outliers=0, seed=2)
    norm, f = datasets.normalize_pnp(x1p, x2p, K)
    ctx = _octx(_lib.PNP, norm)
    est = _estimators.PnPEstimator()
    picks = np.array([np.sort(rng.choice(300, 21, replace=False)) for _ in range(5)])
    P0 = poses[0].copy()
    P0[[3, 7, 11]] += [1.0, -1.0, 2.0]
    batch = est.nonminimal_batch(ctx, picks, None, init=P0)
    for b in range(5):
        single = est.nonminimal(ctx, ("index", picks[b]), None, init=P0)
        # the batched refit solves with the pseudo-inverse (lstsq's cut-off) instead of lstsq itself: equal up to rounding
        assert np.allclose(single[0], batch[b][0], rtol=1e-9, atol=1e-12)
    assert est.nonminimal_batch(ctx, picks, None, init=None) == [[]] * 5
    # a degenerate selection (one point 21 times: rank-deficient normal equations -> minimum-norm step) and weights
    w = rng.random(300) + 0.5
    picks2 = np.vstack([picks[:2], np.full((1, 21), 7)])
    batch = est.nonminimal_batch(ctx, picks2, w, init=P0)
    for b in range(3):
        single = est.nonminimal(ctx, ("index", picks2[b]), w, init=P0)
        assert len(single) == len(batch[b])
        if single:
            assert np.allclose(single[0], batch[b][0], rtol=1e-6, atol=1e-9)


def test_label_refits_in_one_pass_equal_per_label_refits_on_the_oracle_context():
    # PEARL::parameterEstimation refits every instance per iteration: nonminimal_labels (one Gram launch per step for all
    # labels, stacked small solves) must return what K separate nonminimal(("label", k)) calls return - bitwise for the
    # closed-form solvers, up to rounding for the PnP Gauss-Newton (pseudo-inverse instead of lstsq)
    from pyprogressivex import _estimators, _lib, datasets
    rng = np.random.default_rng(4)
    cases = []
    pts, gt, models = datasets.make_homographies(n_per_plane=150, n_planes=3, n_outliers=60, seed=2)
    cases.append((_estimators.HomographyEstimator(), _lib.HOMOGRAPHY, pts, gt, None, True))
    cases.append((_estimators.FundamentalEstimator(), _lib.FUNDAMENTAL, pts, gt, None, True))
    segs, gts, _ = datasets.make_vanishing_points(n_inliers=450, n_vps=3, n_outliers=100, seed=2)
    cases.append((_estimators.VanishingPointEstimator(), _lib.VANISHING_POINT, segs, gts, None, True))
    x1p, x2p, K, gtp, poses = datasets.make_poses(n_per_object=200, n_objects=3, n_outliers=50, seed=2)
    norm, f = datasets.normalize_pnp(x1p, x2p, K)
    inits = [p + 1e-3 * rng.normal(size=12) for p in poses]
    cases.append((_estimators.PnPEstimator(), _lib.PNP, norm, gtp, inits, False))
    for est, mt, data, labels_gt, inits, bitwise in cases:
        ctx = _octx(mt, data)
        Kl = int(labels_gt.max())
        lab = np.where(labels_gt > 0, labels_gt - 1, Kl).astype(np.int32)    # instance k -> label k, outliers -> label K
        lab[:5] = Kl + 1                                                     # a label with 5 points only (too few for H / F)
        ctx.set_labels(lab)
        w = rng.random(len(data)) + 0.5
        n_lab = Kl + 2
        ini = None if inits is None else list(inits) + [inits[0], inits[0]]
        many = est.nonminimal_labels(ctx, n_lab, w, inits=ini, skip=(1,))
        assert many[1] == []
        for k in range(n_lab):
            if k == 1:
                continue
            single = est.nonminimal(ctx, ("label", k), w, init=None if ini is None else ini[k])
            assert len(single) == len(many[k]), (type(est).__name__, k)
            if single:
                if bitwise:
                    assert np.array_equal(single[0], many[k][0]), (type(est).__name__, k)
                elif k < Kl:   # (on the outlier label / a 5-point label Gauss-Newton diverges: rounding differences are amplified)
                    assert np.allclose(single[0], many[k][0], rtol=1e-9, atol=1e-12)


def test_preference_slots_are_recycled(oracle_backend):
    """Rejected proposals and instances removed by PEARL give their preference slot back (each is N * 8 bytes on the
    device): the slot index never exceeds the number of live models."""
    from pyprogressivex import _engine
    seen = []
    orig = OracleContext.preference

    def spy(self, model, T2, slot, **kw):
        seen.append(int(slot))
        return orig(self, model, T2, slot, **kw)
    OracleContext.preference = spy
    try:
        pts, gt, _ = datasets.make_lines(n_per_line=120, n_lines=3, n_outliers=200, seed=3)
        L, lab = px.findLines(pts, np.array(0), 1000, 1000, threshold=2.0, conf=0.99, sampler_id=0, seed=2,
                              minimum_point_number=40, max_outer_iterations=25, maximum_tanimoto_similarity=1e-9)
    finally:
        OracleContext.preference = orig
    # the first model is accepted (Tanimoto 0/0 -> NaN -> valid), every later proposal overlaps it a little and is rejected
    # (until 10 rejections end the run): all of them reuse slot 1
    assert len(L) == 1 and len(seen) >= 5 and seen[0] == 0 and set(seen[1:]) == {1}


def test_bundled_scenes_reach_the_recorded_numbers_on_the_cpu_port(oracle_backend):
    """One seed of three bundled scenes with the recording notebook's exact arguments (scripts/eval_scenes.py) through the
    CPU-backed context: the host logic alone (samplers, replay with local optimisation, PEARL, Tanimoto gate) reaches
    the reference's recorded misclassification errors; the GPU suite repeats this on libpgx with three seeds."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_scenes", os.path.join(root, "scripts", "eval_scenes.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    assert E.homography_scene("unionhouse", 0)[0] <= 3 * E.RECORDED_H["unionhouse"]
    assert E.homography_scene("oldclassicswing", 0)[0] <= 3 * E.RECORDED_H["oldclassicswing"]
    assert E.two_view_scene("book", 0)[0] <= 3 * E.RECORDED_F["book"]


def test_misclassification_overloads_of_progx_utils():
    """progx_utils.h:98-274: both getMisclassificationError overloads, against brute force over permutations."""
    import itertools
    rng = np.random.default_rng(0)
    for trial in range(20):
        n, K, Ka = 60, int(rng.integers(1, 4)), int(rng.integers(1, 4))
        ann = rng.integers(0, Ka + 1, n)
        lab = rng.integers(-1, K + 1, n)
        # (labeling, annotation): literal greedy pairing, checked against a direct transcription
        got = datasets.misclassification_labeling(lab, ann, K, Ka)
        all1 = np.where(lab + 1 <= K, lab + 1, -1)
        used, pair = set(), {0: 0}
        for i in range(1, Ka + 1):
            best, size = -1, -1
            for j in range(1, K + 1):
                if j in used:
                    continue
                sz = int(((all1 == j) & (ann == i)).sum())
                if best == -1 or size < sz:
                    best, size = j, sz
            if best != -1:
                used.add(best)
                pair[i] = best
        out = all1.copy()
        for j in range(n):
            if lab[j] != -1 and all1[j] == pair.get(int(ann[j]), 0):
                out[j] = ann[j]
        assert got == 100.0 * (out != ann).sum() / n
        # (models, annotation): permutations of the model ids by brute force
        pref = (rng.random((K, n)) < 0.3).astype(float)
        got = datasets.misclassification_models(pref, ann, Ka)
        owner = np.where(pref.any(axis=0), np.argmax(pref > 0, axis=0), -1)
        mk = max(K, Ka)
        best = n
        for perm in itertools.permutations(range(mk)):
            ids = np.where(owner >= 0, np.array(perm)[np.maximum(owner, 0)] + 1, 0)
            err = int(((owner >= 0) & (ids != ann)).sum() + ((owner < 0) & (ann != 0)).sum())
            best = min(best, err)
        assert abs(got - 100.0 * best / n) < 1e-12
    assert datasets.misclassification_models(np.zeros((10, 5)), np.zeros(5, int), 2) == -1.0


# ---- [U-14] validity stages of the fundamental-matrix estimator (host, numpy) --------------------------------------------------
def test_fundamental_validity_stages():
    """Oriented epipolar constraint, symmetric-epipolar support and DEGENSAC of _estimators.FundamentalEstimator: the true
    geometry passes all of them, a hypothesis from a mirrored sample fails the orientation test, and a rank-one pseudo-solution
    (whose Sampson inliers hug one line per image) fails the symmetric test."""
    from pyprogressivex import _estimators, datasets
    pts, gt, models = datasets.make_two_view_motions(n_per_motion=300, n_motions=1, n_outliers=100, sigma=0.3, seed=3)
    est = _estimators.FundamentalEstimator()
    assert est.validity == "off"                                               # opt-in: nothing of it is verifiable
    est.validity = "full"
    rng = np.random.default_rng(0)
    inl = np.nonzero(gt == 1)[0]
    smp = np.array([rng.choice(inl, 7, replace=False) for _ in range(50)])
    hyp, src = est.minimal(pts, smp)
    ok = est.valid_samples(pts, smp, hyp, src)
    # among the up-to-three roots per sample, the one closest to the truth is oriented consistently
    F0 = models[0] / np.linalg.norm(models[0])
    err = np.minimum(np.abs(hyp - F0).sum(1), np.abs(hyp + F0).sum(1))
    best = np.array([np.nonzero(src == k)[0][np.argmin(err[src == k])] for k in range(len(smp)) if (src == k).any()])
    assert ok[best].mean() > 0.7                                               # (noisy minimal solutions)
    assert est.valid_samples(pts, smp, np.tile(F0, (len(smp), 1)), np.arange(len(smp))).all()   # the true geometry: every sample
    # one correspondence of the sample mirrored through the epipole's far side: points "behind" the camera
    x1, x2 = est._hom(pts[smp[0]])
    e2 = np.linalg.svd(F0.reshape(3, 3))[0][:, 2]
    sg = np.sign(((x1 @ F0.reshape(3, 3).T) * np.cross(e2[None, :], x2)).sum(-1))
    assert (sg > 0).all() or (sg < 0).all()
    # the truth keeps its support under the symmetric distance; a rank-one matrix a b^T does not
    never = lambda c: np.full(len(c), -np.inf)                                   # (plane-and-parallax candidates never win here)
    from pyprogressivex import _lib as L
    octx = OracleContext()
    octx.set_points(L.FUNDAMENTAL, pts)
    valid, _ = est.valid_best(octx, pts, F0, smp[0], 0.75, never)
    assert valid
    a, b = np.array([0.0, 1.0, -500.0]), np.array([0.0, 1.0, -480.0])            # "x' on the line y = 500" times "x on y = 480"
    band = pts.copy()
    band[:150, 1] = 480.0 + rng.normal(0, 0.2, 150)                              # plenty of points near ONE of the two lines only
    band[150:300, 3] = 500.0 + rng.normal(0, 0.2, 150)
    R1 = np.outer(a, b).reshape(-1) / np.linalg.norm(np.outer(a, b))
    samp, sym = est._sampson_and_symmetric(R1.reshape(3, 3), band)
    assert (samp < 2.25 * 0.75 ** 2).sum() >= 250 and ((samp < 2.25 * 0.75 ** 2) & (sym < 9 * 0.75 ** 2)).sum() < 100
    octx.set_points(L.FUNDAMENTAL, band)
    inl_n, sup_n = octx.epipolar_support(R1, 2.25 * 0.75 ** 2, 9 * 0.75 ** 2)   # the counts the stage uses = the numpy formula's
    assert inl_n == int((samp < 2.25 * 0.75 ** 2).sum()) and sup_n == int(((samp < 2.25 * 0.75 ** 2) & (sym < 9 * 0.75 ** 2)).sum())
    valid, _ = est.valid_best(octx, band, R1, None, 0.75, never)
    assert not valid
    est_off = _estimators.FundamentalEstimator()
    est_off.validity = "off"
    assert est_off.valid_best(None, band, R1, None, 0.75, never)[0]


def test_sharding_is_opt_in(monkeypatch):
    """a torch.distributed.run job whose ranks call the API independently must not be pulled into a collective.
    default_exchange returns None unless the call (distributed=True) or the environment (PGX_MULTI_GPU=1) opts in, and refuses a
    launch that spans nodes before touching RCCL."""
    from pyprogressivex import parallel
    for key in ("PGX_MULTI_GPU", "PGX_FORCE_COMM", "LOCAL_WORLD_SIZE", "GROUP_WORLD_SIZE", "NNODES"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "4")

    class NoComm:      # a context without RCCL: reaching init_rccl would fail loudly
        nranks = 1

    assert parallel.default_exchange(NoComm()) is None
    assert parallel.default_exchange(NoComm(), distributed=False) is None
    monkeypatch.setenv("PGX_MULTI_GPU", "1")
    assert parallel.default_exchange(NoComm(), distributed=False) is None       # the call wins over the environment
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "2")                                 # 4 ranks, 2 per node
    import pytest
    with pytest.raises(RuntimeError, match="one node"):
        parallel.default_exchange(NoComm())
    with pytest.raises(RuntimeError, match="one node"):
        parallel.default_exchange(NoComm(), distributed=True)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert parallel.default_exchange(NoComm(), distributed=True) is None        # one rank: nothing to shard


def test_vectorised_fisher_yates_keeps_the_generator_stream():
    """_proposal._fisher_yates_rows (all rows at once) against the per-row scalar loop it replaced: same rows, same generator
    state afterwards - every seeded result of the package is unchanged by the vectorisation."""
    from pyprogressivex import _proposal as P
    for seed in range(120):
        r0 = np.random.default_rng(seed)
        m = int(r0.integers(2, 8))
        count = int(r0.integers(1, 300))
        tops = r0.integers(m, m + int(r0.choice([1, 3, 10, 50, 1000])), count).astype(np.int64)
        bad = np.nonzero(r0.random(count) < 0.6)[0]
        a, b = np.zeros((count, m), np.int64), np.zeros((count, m), np.int64)
        ra, rb = np.random.default_rng(seed + 7), np.random.default_rng(seed + 7)
        P._fisher_yates_rows(ra, a, tops, bad, m)
        P._fisher_yates_rows_scalar(rb, b, tops, bad, m)
        assert np.array_equal(a, b) and ra.random() == rb.random()
        for r in bad:
            assert len(set(a[r])) == m and a[r].max() < tops[r]
        # the table walk runs in libpgx's host code for C-contiguous int64 rows (above) and in numpy otherwise: the same rows
        wide = np.zeros((count, 2 * m), np.int64)
        c = wide[:, ::2]
        rc = np.random.default_rng(seed + 7)
        P._fisher_yates_rows(rc, c, tops, bad, m)
        assert np.array_equal(c, b)


def test_host_row_helpers_of_libpgx_match_numpy():
    """pgx_host_rows_with_duplicates against sort + compare, and _distinct_rows end to end: rows of distinct indices below their
    tops, and the same rows and generator state as the all-numpy statement of the function."""
    from pyprogressivex import _lib, _proposal as P
    rng = np.random.default_rng(5)
    for _ in range(200):
        m = int(rng.integers(1, 9))
        count = int(rng.integers(0, 400))
        s = rng.integers(0, int(rng.choice([m, 2 * m, 50, 10 ** 6])) + 1, (count, m)).astype(np.int64)
        srt = np.sort(s, axis=1)
        ref = (srt[:, 1:] == srt[:, :-1]).any(axis=1) if m > 1 else np.zeros(count, bool)
        assert np.array_equal(_lib.host_rows_with_duplicates(s), ref)

    def distinct_rows_numpy(rng, tops, m, retries=4):   # the function as it was before the helpers (numpy only)
        tops = np.asarray(tops, dtype=np.int64)
        s = (rng.random((tops.shape[0], m)) * tops[:, None]).astype(np.int64)
        if m < 2:
            return s
        dense = tops < 4 * m
        for _ in range(retries):
            srt = np.sort(s, axis=1)
            bad = (srt[:, 1:] == srt[:, :-1]).any(axis=1) & ~dense
            if not bad.any():
                break
            s[bad] = (rng.random((int(bad.sum()), m)) * tops[bad][:, None]).astype(np.int64)
        srt = np.sort(s, axis=1)
        bad = np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0]
        P._fisher_yates_rows_scalar(rng, s, tops, bad, m)
        return s

    for seed in range(60):
        r0 = np.random.default_rng(seed)
        m = int(r0.integers(1, 8))
        count = int(r0.integers(1, 1200))
        tops = r0.integers(m, m + int(r0.choice([1, 4, 30, 2000])), count).astype(np.int64)
        ra, rb = np.random.default_rng(seed + 99), np.random.default_rng(seed + 99)
        a = P._distinct_rows(ra, tops, m)
        b = distinct_rows_numpy(rb, tops, m)
        assert np.array_equal(a, b) and ra.random() == rb.random()
        assert (a < tops[:, None]).all() and (a >= 0).all()
        if m > 1:
            assert not _lib.host_rows_with_duplicates(a).any()
