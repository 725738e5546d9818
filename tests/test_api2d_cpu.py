"""findCircles (model type 10) without a GPU, as tests/test_api3d_cpu.py does for planes and spheres: the whole drop-in call on the
oracle-backed context, every decision of the outer loop / PEARL replayed by oracle/progx_replay.c (no tie tolerance: both sides sum
sequentially) and every proposal walk by oracle/progx_proposal.c.  The oracle's circle rows themselves are checked against exact
arithmetic in tests/test_oracle.py; tests/test_gpu_api.py and tests/test_gpu_replay.py run the same scenes on the device and compare
with what these runs return."""
import warnings

import numpy as np
import pytest

import progx_proposal as Q
import progx_replay as R
import pyprogressivex as px
import replay_helpers as H
from helpers import edge_clouds_2d, match_3d, scene_3d
from oracle_ctx import OracleContext
from pyprogressivex import _api
from test_api3d_cpu import run_replay_walks

SIGMA = 0.5                      # make_circles' noise, in pixels; the threshold is the call's default (2.0)


@pytest.fixture()
def cpu_api(monkeypatch):
    monkeypatch.setattr(_api, "_ctx", OracleContext())


def test_oracle_context_radius_range_has_the_device_semantics_for_circles():
    """include/pgx.h pgx_set_radius_range: the circle solver reads the same context state as the sphere solver - [0, +inf] at
    creation, kept across set_points (also from one of the two types to the other), inclusive at both ends, rmin == rmax allowed;
    refused ranges leave the state alone; the line solver on the same 2-D points does not read it"""
    import pgx_oracle as O
    ctx = OracleContext()
    assert ctx.radius_range == (0.0, np.inf)
    pts = np.array([[3.0, 2.0], [1.0, 4.0], [-1.0, 2.0], [5.0, 0.0], [-5.0, 0.0], [0.0, 5.0]])
    smp = np.array([[0, 1, 2], [3, 4, 5]], np.int32)               # radii 2 and 5
    ctx.set_points(O.CIRCLE2D, pts)
    assert ctx.solve_minimal(smp).tolist() == [[1.0, 2.0, 2.0], [0.0, 0.0, 5.0]]
    ctx.set_radius_range(3.0, np.inf)
    assert (~np.isnan(ctx.solve_minimal(smp)[:, 0])).tolist() == [False, True]
    for bad in ((-1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(RuntimeError):
            ctx.set_radius_range(*bad)
    assert ctx.radius_range == (3.0, np.inf)
    ctx.set_points(O.CIRCLE2D, pts)                                # a new point set keeps the range
    assert (~np.isnan(ctx.solve_minimal(smp)[:, 0])).tolist() == [False, True]
    ctx.set_radius_range(2.0, 2.0)
    assert (~np.isnan(ctx.solve_minimal(smp)[:, 0])).tolist() == [True, False]
    ctx.set_radius_range(2.0, 5.0)                                 # inclusive at both ends
    assert (~np.isnan(ctx.solve_minimal(smp)[:, 0])).tolist() == [True, True]
    ctx.set_radius_range(np.nextafter(2.0, 3.0), np.nextafter(5.0, 0.0))
    assert (~np.isnan(ctx.solve_minimal(smp)[:, 0])).tolist() == [False, False]
    ctx.set_points(O.LINE2D, pts)                                  # the line solver does not read it
    assert np.isfinite(ctx.solve_minimal(smp[:, :2].copy())).all()
    ctx.set_radius_range()
    assert ctx.radius_range == (0.0, np.inf)


def test_three_circle_scene_is_recovered_and_equals_both_replays(cpu_api):
    """3 x 800 inliers + 800 outliers with the call's default arguments (Progressive NAPSAC, threshold 2): three models, each
    within 5 sigma = 2.5 px of its ground truth in every parameter, under 3 % of the points labelled differently from the
    generator; decisions and proposal walks equal the replays.  Measured on the oracle-backed context: the worst parameter is
    0.037 px from the truth (0.07 sigma) and 0.5 % of the points are labelled differently, so the planes' and spheres' rule holds
    for circles as it stands."""
    pts, gt, truth = scene_3d("circle")
    out, rec, K, wrec = run_replay_walks(px.findCircles, pts, seed=1, minimum_point_number=100)
    assert K == 3 and len(wrec.walks) >= 3 and out[0].shape == (3, 3)
    worst = match_3d("circle", out[0], truth).max()
    order = [int(np.argmin([match_3d("circle", out[0][k:k + 1], truth[j:j + 1])[0] for k in range(3)])) for j in range(3)]
    relabelled = np.full(len(pts), 0)
    for j, k in enumerate(order):
        relabelled[out[1] == k] = j + 1
    print(f"findCircles on the oracle context: worst parameter error {worst:.3g} px, {np.mean(relabelled != gt):.4f} of the points relabelled")
    assert worst <= 5 * SIGMA
    assert np.mean(relabelled != gt) < 0.03
    verdicts, after, brk = H.summary(rec.events)
    assert sum(verdicts) >= 3 and after[-1] == 3
    assert any(e[0] == R.EV_REFIT for e in rec.events) and any(e[0] == Q.EV_LO_ROUND for w in wrec.walks for e in w["events"])


@pytest.mark.parametrize("kw", [
    dict(sampler_id=0), dict(sampler_id=3), dict(sampler_id=1), dict(sampler_id=2),
    dict(sampler_id=2, scoring_exponent=1), dict(sampler_id=2, scoring_exponent=2),
    dict(sampler_id=3, scoring_exponent=1), dict(sampler_id=3, scoring_exponent=2),
    dict(sampler_id=3, spatial_coherence_weight=0.1), dict(sampler_id=2, spatial_coherence_weight=0.1, neighborhood="knn:6"),
    dict(sampler_id=0, sampler_rng="philox"), dict(sampler_id=3, sampler_rng="philox"), dict(sampler_id=3, radius_range=(20.0, 300.0)),
    dict(sampler_id=3, local_optimization="lsq")],
    ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()))
def test_samplers_exponents_and_coherence_equal_both_replays(cpu_api, kw):
    """the planes' and the spheres' sampler and option matrix together, on circles: every sampler, both exponents, spatial coherence
    on two neighbourhoods, both sample generators, a radius range, the least-squares local optimisation"""
    pts, gt, truth = scene_3d("circle")
    out, rec, K, wrec = run_replay_walks(px.findCircles, pts, seed=2, minimum_point_number=100, **kw)
    assert 1 <= K <= 4
    found = match_3d("circle", out[0], truth) <= 5 * SIGMA
    assert found.sum() >= (3 if K >= 3 else K)
    if kw.get("spatial_coherence_weight", 0.0) > 0:
        assert any(e[0] == R.EV_PEARL_ITER for e in rec.events)


def test_weights_reach_the_refits_and_the_replays_agree(cpu_api):
    pts, gt, truth = scene_3d("circle")
    w = np.random.default_rng(3).random(len(pts)) + 0.25
    kw = dict(seed=1, minimum_point_number=100, sampler_id=3)
    out, rec, K, _ = run_replay_walks(px.findCircles, pts, weights=w, **kw)
    plain = px.findCircles(pts, **kw)
    assert K == 3 and plain[0].shape == out[0].shape and match_3d("circle", out[0], truth).max() <= 5 * SIGMA
    assert not np.array_equal(plain[0], out[0]) and np.abs(plain[0] - out[0]).max() < 5 * SIGMA
    with pytest.raises(ValueError):
        px.findCircles(pts, weights=w[:-1], **kw)


def test_radius_range_that_excludes_a_true_circle(cpu_api):
    """radii 50, 100 and 150 by construction; radius_range = (30, 125) leaves the two small ones: no returned model has a radius
    outside the range, the large circle's points end as outliers, both replays agree.  Without the range all three are found."""
    rng = np.random.default_rng(8)
    centres = np.array([[200.0, 200.0], [600.0, 300.0], [400.0, 750.0]])
    radii = np.array([50.0, 100.0, 150.0])
    parts, gt = [], []
    for k in range(3):
        phi = rng.uniform(0.0, 2.0 * np.pi, 800)
        parts.append(centres[k] + np.column_stack([np.cos(phi), np.sin(phi)]) * (radii[k] + rng.normal(0, SIGMA, 800))[:, None])
        gt.append(np.full(800, k + 1))
    parts.append(rng.uniform(0, 1000, (800, 2)))
    gt.append(np.zeros(800, int))
    order = rng.permutation(3200)
    pts, gt = np.vstack(parts)[order], np.concatenate(gt)[order]
    truth = np.column_stack([centres, radii])
    kw = dict(seed=1, minimum_point_number=100)
    out, rec, K, _ = run_replay_walks(px.findCircles, pts, radius_range=(30.0, 125.0), **kw)
    assert K == 2 and (out[0][:, 2] >= 30.0).all() and (out[0][:, 2] <= 125.0).all()
    d = match_3d("circle", out[0], truth)
    assert d[0] <= 5 * SIGMA and d[1] <= 5 * SIGMA and d[2] > 20.0
    assert np.mean(out[1][gt == 3] == K) > 0.9                    # the excluded circle's points: outliers
    free, _, Kf, _ = run_replay_walks(px.findCircles, pts, **kw)
    assert Kf == 3 and match_3d("circle", free[0], truth).max() <= 5 * SIGMA


EDGE_NAMES = ["n_equals_sample_size", "coincident", "collinear", "outliers_only", "offset_1e6"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_inputs_run_and_equal_the_replay(cpu_api, name):
    """degenerate and hostile 2-D clouds through run + replay for samplers 0, 2, 3 with and without spatial coherence: no exception,
    no numpy warning, decisions equal the replay; exactly degenerate clouds (dyadic coordinates: det == 0 exactly) give no model; an
    offset of 1e6 does not lose the two circles"""
    pts, zero = edge_clouds_2d()[name]
    for sampler_id in (0, 2, 3):
        for sc in (0.0, 0.1):
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                out, rec, rep = H.run_and_replay(px.findCircles, pts, seed=1, sampler_id=sampler_id, spatial_coherence_weight=sc,
                                                 minimum_point_number=20)
            K = H.assert_agree(out, rec, rep, 1)
            what = (name, sampler_id, sc)
            assert out[0].shape == (K, 3) and out[1].shape == (len(pts),) and np.isfinite(out[0]).all(), what
            if zero or name in ("n_equals_sample_size", "outliers_only"):
                assert K == 0, what
            if name == "offset_1e6":
                assert K == 2, what


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "refused_nan", "refused_inf"])
def test_non_finite_rows_are_refused_as_on_the_device(cpu_api, name):
    """pgx_graph_build lays its grid over x and y and refuses a NaN / Inf there; a 2-D point has no other column, so every non-finite
    row of a findCircles input is refused, in either column, by both contexts (a RuntimeError)"""
    pts, _ = edge_clouds_2d()[name]
    for sampler_id in (0, 3):
        with pytest.raises(RuntimeError, match="non-finite"):
            px.findCircles(pts, seed=1, sampler_id=sampler_id, minimum_point_number=20)


def test_replay_soak_slice_cpu_circles(cpu_api):
    """20 random small findCircles calls (tests/soak_replay.py, types=("circle",): random samplers, exponents, weights, radius ranges,
    ball radii, local optimisation, scenes far from the origin) on the oracle-backed context: every decision equals the replay with
    no tie tolerance, every proposal walk equals the proposal replay"""
    import soak_replay
    assert soak_replay.soak(9002, 20, verbose=False, tie=0.0, types=("circle",)) == 0
    assert soak_replay.LAST["per_type"] == {"findCircles": 20} and soak_replay.LAST["proposals"] > 40
