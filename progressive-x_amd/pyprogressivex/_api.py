"""The five entry points of the reference's pybind11 module (and findPlanes / findSpheres / findLines3D / findCylinders / findCones /
findPrimitives / findOrientedPrimitives / findCircles, the same pipeline on 3-D point clouds and 2-D point sets), same names /
argument order / defaults / return layout /
error messages (/root/reference/src/pyprogressivex/src/bindings.cpp:9-392 wrappers, :410-491 defaults) and the
parameter plumbing of the problem drivers (/root/reference/src/pyprogressivex/src/progressivex_python.cpp:41-666),
including their quirks: unknown sampler ids print to stderr and return zero models,
findTwoViewMotions ignores scoring_exponent, findLines ignores weights, only findVanishingPoints forwards do_logging.

Extensions that do not change the reference behaviour when left at their defaults (keyword-only):
  seed=None                     reproducible sampling (the reference seeds from std::random_device)
  sampler_rng="numpy"           "philox": the samplers draw from the in-repo counter-based generator (_rng.py) - uniform, NAPSAC and PROSAC on the device inside the solver's launch, Progressive NAPSAC (sequential) in libpgx's host code
  refit_solver="lapack"         "jacobi": the refits' smallest-eigenvector solves run through pgx_eigh_smallest_batch (batched cyclic Jacobi
                                on the device, bitwise a CPU restatement, ~1e-13 from LAPACK) instead of numpy.linalg.eigh: round 6
  distributed=None              True: shard the proposal batches over the ranks of this launch (every rank must make the same
                                call on the same data; checked).  None: only if PGX_MULTI_GPU=1.  Never implicit.
  max_outer_iterations=10       the reference's hard cap on proposals per call (progressive_x.h:272)
  residual="transfer"           findHomographies: "symmetric" switches to the symmetric transfer error (U-1 switch)
  neighborhood="flann_like"     U-7 switch: "flann_like" (<= 5 nearest neighbours inside the ball, what upstream's
                                checks=6 approximate search can return at most), "radius" (all points in the ball),
                                or "knn:<k>"
  labeling_l0="greedy"          U-8 switch, only matters when spatial_coherence_weight == 0 (the default of four of the
                                five entry points): PEARL then sets no smooth cost, and GCO-v3's expansion() labels such
                                an energy by its special-case solver (greedy facility location over the label costs)
                                instead of alpha-expansion; "expansion" = alpha-expansion moves (round 1's behaviour)
  local_optimization="auto"     U-12 switch: "auto" = GC-RANSAC's graph-cut local optimisation whenever the spatial
                                coherence weight is in (0, 1) (the cut runs on the GPU, pgx_gc_labeling), iterated
                                least-squares refits otherwise; "lsq" = refits only
"""
import sys

import numpy as np

from . import _components, _engine, _estimators, _extents, _lib, _proposal

_ctx = None


def _context():
    """One GPU context per process (device = $PGX_DEVICE or $LOCAL_RANK or 0).  Raises if libpgx.so or the GPU is
    missing — there is no CPU path."""
    global _ctx
    if _ctx is None:
        import os
        dev = int(os.environ.get("PGX_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _ctx = _lib.Context(dev)
    return _ctx


def _as_f64(a):
    # py::array_t<double> with forcecast (bindings.cpp:10): any dtype is converted; the raw buffer is then read as if
    # C-contiguous, which np.ascontiguousarray makes explicit
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64)


def _shape2(a):
    if a.ndim < 2:
        raise ValueError("array must be 2-dimensional")  # pybind11 would fail on buf.shape[1]
    return a.shape[0], a.shape[1]


def _weights(weights_, n=None):
    """bindings.cpp:200-208: a 0-d / empty array means "no weights".  The reference then reads weights[i] for every point
    without a length check (undefined behaviour for a short array); here a length other than n is a ValueError."""
    w = np.asarray(weights_, dtype=np.float64)
    if w.ndim == 0 or w.size == 0:
        return None
    w = np.ascontiguousarray(w).reshape(-1)
    if n is not None and w.shape[0] != n:
        raise ValueError(f"weights should have one entry per row ({n}), got {w.shape[0]}")
    return w


def _unknown_sampler(sampler_id):
    # progressivex_python.cpp:240-245 (message kept literally, including its omission of id 3)
    sys.stderr.write(f"Unknown sampler identifier: {sampler_id}. The accepted samplers are 0 (uniform sampling), "
                     "1 (PROSAC sampling), 2 (P-NAPSAC sampling)\n")


def _run(estimator, pts, graph_points, radius, sampler_factory, *, threshold, conf, spatial_coherence_weight,
         maximum_tanimoto_similarity, max_iters, minimum_point_number, maximum_model_number, scoring_exponent=2,
         do_logging=False, weights=None, seed=None, max_outer_iterations=10, neighborhood="flann_like",
         local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack",
         setup=None):
    """setup(ctx), when given, runs on the context right after the run has made the points resident (per-call context state such as
    findSpheres' radius range and findCylinders' normals, which belong to a point set)."""
    n = pts.shape[0]
    if sampler_rng not in ("numpy", "philox"):
        raise ValueError("sampler_rng should be 'numpy' or 'philox'")
    if refit_solver not in ("lapack", "jacobi"):
        raise ValueError("refit_solver should be 'lapack' or 'jacobi'")
    estimator.refit_solver = str(refit_solver)   # the refits' small eigen-solves: numpy on the host / pgx_eigh_smallest_batch (_estimators.py)
    if getattr(sampler_factory, "unknown", False):
        # progressivex_python.cpp:240-245: message on stderr, zero models, labelling left at its initial zeros
        _unknown_sampler(sampler_factory.sampler_id)
        return [], np.zeros(n, dtype=np.int32), None
    ctx = _context()
    # multi-GPU, OPT-IN (distributed=True or PGX_MULTI_GPU=1, one process per GPU, WORLD_SIZE > 1): the proposal batches are
    # sharded over the ranks and the score triples all-gathered over RCCL (parallel.py); everything else runs replicated, so
    # every rank returns the same result.  Every rank must make this call with the same data (checked) and draw the same
    # samples: an unset seed is replaced by one the launch agrees on.
    from . import parallel
    exchange = parallel.default_exchange(ctx, distributed)
    if exchange is not None:
        parallel.check_same_problem(exchange, pts, params=(
            type(estimator).__name__, float(radius), getattr(sampler_factory, "sampler_id", None), float(threshold), float(conf),
            float(spatial_coherence_weight), float(maximum_tanimoto_similarity), int(max_iters), int(minimum_point_number),
            int(maximum_model_number), int(scoring_exponent), seed, int(max_outer_iterations), str(neighborhood),
            str(local_optimization), str(labeling_l0), str(sampler_rng), getattr(estimator, "validity", None), str(pearl_abs), str(refit_solver))
            + ((tuple(float(v) for v in estimator.radius_range),) if hasattr(estimator, "radius_range") else ()))
        if seed is None:
            seed = parallel.shared_seed()
    rng = np.random.default_rng(seed)
    # FlannNeighborhoodGraph(&points, radius) [U-7]: built on the GPU (pgx_graph_build) and left resident there; the
    # CSR comes back for the neighbourhood samplers.
    resident = True
    # ... and it only comes BACK to the host for the sampler that walks it (NAPSAC): 74 MB of CSR at N = 1e6 otherwise cross PCIe
    # for nothing (find6DPoses always samples uniformly)
    fetch = bool(getattr(sampler_factory, "needs_graph", True))
    if neighborhood == "radius":
        graph = ctx.graph_build(graph_points, _lib.GRAPH_BALL, radius=radius, fetch=fetch)
    elif str(neighborhood).startswith("knn:"):
        graph = ctx.graph_build(graph_points, _lib.GRAPH_KNN, k=int(str(neighborhood)[4:]), fetch=fetch)
    else:
        graph = ctx.graph_build(graph_points, _lib.GRAPH_KNN_IN_BALL, radius=radius, k=5, fetch=fetch)
    if not fetch:
        graph = None
    if sampler_rng == "philox" and getattr(sampler_factory, "kind", None) == "pnapsac":   # (sequential: drawn by libpgx's host code)
        sampler = _proposal.PhiloxProgressiveNapsacSampler(n, rng, *sampler_factory.pnapsac_args)
    else:
        sampler = sampler_factory(n, rng, graph)
    if sampler_rng == "philox" and type(sampler) is _proposal.UniformSampler:   # the in-repo counter-based generator (device-drawable)
        sampler = _proposal.PhiloxUniformSampler(n, rng)
    elif sampler_rng == "philox" and type(sampler) is _proposal.NapsacSampler:
        sampler = _proposal.PhiloxNapsacSampler(n, rng, graph)
    elif sampler_rng == "philox" and type(sampler) is _proposal.ProsacSampler:
        sampler = _proposal.PhiloxProsacSampler(n, rng, sample_size=sampler.prosac_m, convergence_iterations=sampler.t_n)
    s = _engine.MultiModelSettings()
    s.minimum_number_of_inliers = int(minimum_point_number)          # progressivex_python.cpp:261
    s.inlier_outlier_threshold = float(threshold)                    # :263
    s.set_confidence(float(conf))                                    # :265
    s.maximum_tanimoto_similarity = float(maximum_tanimoto_similarity)   # :267
    s.spatial_coherence_weight = float(spatial_coherence_weight)     # :269
    s.max_iteration_number = int(max_iters)                          # :271
    if maximum_model_number > 0:                                     # :273-274
        s.maximum_model_number = int(maximum_model_number)
    s.point_weights = weights
    s.max_outer_iterations = int(max_outer_iterations)
    s.local_optimization = str(local_optimization)   # "auto": GC-RANSAC's graph-cut LO; "lsq": refits only
    if labeling_l0 not in ("greedy", "expansion"):
        raise ValueError("labeling_l0 should be 'greedy' or 'expansion'")
    s.labeling_l0 = str(labeling_l0)
    if pearl_abs not in ("double", "int"):
        raise ValueError("pearl_abs should be 'double' or 'int'")
    s.pearl_abs = str(pearl_abs)        # [U-16] which abs() PEARL.h:465 resolves to
    if trace is not None and hasattr(trace, "begin"):
        # diagnostics hook (_engine.EV_*): what the run is made of, for a replay of its decisions (tests/)
        trace.begin(dict(model_type=estimator.model_type, points=pts, graph_points=graph_points, radius=float(radius),
                         neighborhood=str(neighborhood), sample_size=int(estimator.sample_size),
                         nonminimal_sample_size=int(estimator.nonminimal_sample_size), settings=s))
    px = _engine.ProgressiveX(ctx, estimator, pts, graph, sampler, s, scoring_exponent=scoring_exponent,
                              do_logging=do_logging, graph_resident=resident, exchange=exchange, trace=trace, setup=setup)
    models, stats = px.run()
    labeling = np.asarray(stats.labeling, dtype=np.int64).astype(np.int32)     # bindings.cpp:152-156
    return models, labeling, stats


# the options of _run that every entry point takes under the same name
_RUN_OPTIONS = ("threshold", "conf", "spatial_coherence_weight", "maximum_tanimoto_similarity", "max_iters", "minimum_point_number",
                "maximum_model_number", "scoring_exponent", "seed", "max_outer_iterations", "neighborhood", "local_optimization",
                "labeling_l0", "distributed", "sampler_rng", "trace", "pearl_abs", "refit_solver")


def _run_options(args, **changed):
    """_run's keyword options from an entry point's arguments (args = its locals()); `changed` replaces or adds some"""
    return {**{name: args[name] for name in _RUN_OPTIONS}, **changed}


def _stack(estimator, models, cols):
    rows = estimator.rows_per_model
    out = np.zeros((rows * len(models), cols), dtype=np.float64)
    for k, m in enumerate(models):
        out[rows * k: rows * (k + 1)] = estimator.output(m.descriptor)
    return out


def _sampler_factory(sampler_id, valid, pts=None, sizes=None, sample_size=None, prosac_sample_size=None):
    def make(n, rng, graph):
        kind = valid[sampler_id]
        if kind == "uniform":
            return _proposal.UniformSampler(n, rng)
        if kind == "prosac":
            return _proposal.ProsacSampler(n, rng, sample_size=prosac_sample_size)
        if kind == "pnapsac":                # ProgressiveNapsacSampler<4>(&points, {16,8,4,2}, m, {w1,h1,w2,h2}, 0.5)
            return _proposal.ProgressiveNapsacSampler(n, rng, pts, sizes, sample_size)
        return _proposal.NapsacSampler(n, rng, graph)
    make.unknown = sampler_id not in valid
    make.kind = valid.get(sampler_id)
    make.pnapsac_args = (pts, sizes, sample_size)
    make.needs_graph = valid.get(sampler_id) == "napsac"
    make.sampler_id = sampler_id
    return make


def findHomographies(corrs, w1, h1, w2, h2, threshold=4.0, conf=0.5, spatial_coherence_weight=0.0,
                     neighborhood_ball_radius=200.0, maximum_tanimoto_similarity=0.4, max_iters=1000,
                     minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                     do_logging=False, *, seed=None, max_outer_iterations=10, residual="transfer", neighborhood="flann_like",
                     local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """bindings.cpp:99-166, progressivex_python.cpp:173-304.  Returns (H[(3K),3] float64, labels[n] int32)."""
    corrs = _as_f64(corrs)
    n, dim = _shape2(corrs)
    if dim != 4 or n < 4:
        raise ValueError("corrs should be an array with dims [n,4], n>=4")           # bindings.cpp:119-124
    if do_logging and sampler_id == 1:
        print("Note: PROSAC sampler requires the correspondences to be order by quality, e.g., SNN ratio.")
    if do_logging and sampler_id == 2:
        print("Note: Progressive NAPSAC sampler requires the correspondences to be order by quality, e.g., SNN ratio.")
    est = (_estimators.SymmetricHomographyEstimator() if residual == "symmetric" else _estimators.HomographyEstimator())
    # NB: the driver never calls progressive_x.log(): do_logging only triggers the sampler notes (:219-226)
    models, labels, _ = _run(est, corrs, corrs, neighborhood_ball_radius,
                             _sampler_factory(sampler_id, {0: "uniform", 1: "prosac", 2: "pnapsac", 3: "napsac"}, corrs,
                                              (w1, h1, w2, h2), est.sample_size),
                             **_run_options(locals()))
    return _stack(est, models, 3), labels


def findTwoViewMotions(corrs, w1, h1, w2, h2, threshold=4.0, conf=0.5, spatial_coherence_weight=0.0,
                       neighborhood_ball_radius=200.0, maximum_tanimoto_similarity=0.4, max_iters=1000,
                       minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=3,
                       do_logging=False, *, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                     local_optimization="auto", labeling_l0="greedy", distributed=None, validity="off", sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """bindings.cpp:324-392, progressivex_python.cpp:537-666.  Returns (F[(3K),3], labels[n]).
    validity [U-14, keyword-only, not in the reference's signature]: which of the estimator's model-validity stages run -
    "off" (the default: strict restatement of what is in the snapshot, i.e. none), "oriented", "symmetric" (oriented +
    symmetric-epipolar support) or "full" (+ DEGENSAC: the recollection of gcransac's FundamentalMatrixEstimator::isValidModel;
    its source is absent from the snapshot and no bundled scene measures better with it, so it is opt-in - INTEGRATION.md)."""
    if validity not in ("off", "oriented", "symmetric", "full"):
        raise ValueError("validity should be 'off', 'oriented', 'symmetric' or 'full'")
    corrs = _as_f64(corrs)
    n, dim = _shape2(corrs)
    if dim != 4 or n < 7:
        raise ValueError("corrs should be an array with dims [n,4], n>=7")           # bindings.cpp:344-349
    if do_logging and sampler_id == 1:
        print("Note: PROSAC sampler requires the correspondences to be order by quality, e.g., SNN ratio.")
    if do_logging and sampler_id == 2:
        print("Note: Progressive NAPSAC sampler requires the correspondences to be order by quality, e.g., SNN ratio.")
    est = _estimators.FundamentalEstimator()
    est.validity = validity
    # the driver ignores scoring_exponent (never calls setScoringExponent: :621-638) => ProgressiveX's default 2
    models, labels, _ = _run(est, corrs, corrs, neighborhood_ball_radius,
                             _sampler_factory(sampler_id, {0: "uniform", 1: "prosac", 2: "pnapsac", 3: "napsac"}, corrs,
                                              (w1, h1, w2, h2), est.sample_size),
                             **_run_options(locals(), scoring_exponent=2))
    return _stack(est, models, 3), labels


findFundamentalMatrices = findTwoViewMotions   # name used by BASELINE.json's north star


def findVanishingPoints(lines, weights, w, h, threshold=4.0, conf=0.5, spatial_coherence_weight=0.0,
                        neighborhood_ball_radius=200.0, maximum_tanimoto_similarity=0.4, max_iters=1000,
                        minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                        do_logging=False, *, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                     local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """bindings.cpp:168-245, progressivex_python.cpp:306-423.  Returns (vp[K,3], labels[n]).  Only sampler ids 0/1
    exist for this driver, so the DEFAULT id 3 returns zero models, as in the reference."""
    lines = _as_f64(lines)
    n, dim = _shape2(lines)
    if dim != 4 or n < 2:
        raise ValueError("lines should be an array with dims [n,4], n>=2")           # bindings.cpp:188-193
    if do_logging and sampler_id == 1:
        print("Note: PROSAC sampler requires the correspondences to be order by quality, e.g., SNN ratio.")
    est = _estimators.VanishingPointEstimator()
    models, labels, _ = _run(est, lines, lines, neighborhood_ball_radius,
                             _sampler_factory(sampler_id, {0: "uniform", 1: "prosac"}),
                             **_run_options(locals(), do_logging=bool(do_logging), weights=_weights(weights, n)))     # :401
    return _stack(est, models, 3), labels


def findLines(points, weights, w, h, threshold=2.0, conf=0.5, spatial_coherence_weight=0.0,
              neighborhood_ball_radius=200.0, maximum_tanimoto_similarity=0.4, max_iters=1000,
              minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
              do_logging=False, *, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                     local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """bindings.cpp:247-322, progressivex_python.cpp:425-535.  Returns (lines[K,3], labels[n]).  Sampler ids 0/1/2
    (2 = NAPSAC here); the default 3 returns zero models; `weights` is parsed and ignored, as in the reference."""
    points = _as_f64(points)
    n, dim = _shape2(points)
    if dim != 2 or n < 2:
        raise ValueError("Points should be an array with dims [n,3], n>=2")          # bindings.cpp:267-270 (sic)
    _weights(weights)         # parsed and unused (progressivex_python.cpp:466-482): any length is accepted, as upstream
    if do_logging and sampler_id == 1:
        print("Note: PROSAC sampler requires the points to be order by quality, e.g., SNN ratio.")
    est = _estimators.LineEstimator()
    models, labels, _ = _run(est, points, points, neighborhood_ball_radius,
                             _sampler_factory(sampler_id, {0: "uniform", 1: "prosac", 2: "napsac"},
                                              prosac_sample_size=4),     # the HOMOGRAPHY sample size (quirk, :463)
                             **_run_options(locals()))
    return _stack(est, models, 3), labels


def _point_cloud(points, weights, n_min, dim=3):
    """the input checks of the point-cloud calls (3-D; dim=2: findCircles' point sets): points [n, dim] with n >= n_min, weights [n] or
    None; and Progressive NAPSAC's grid, which starts at the corner of the bounding box of the finite coordinates and spans its
    extents.  Returns (points, weights, grid points, extents)."""
    points = _as_f64(points)
    if points.ndim != 2 or points.shape[1] != dim or points.shape[0] < n_min:
        raise ValueError(f"points should be an array with dims [n,{dim}], n>={n_min}")
    w = None if weights is None else _weights(weights, points.shape[0])
    finite = np.isfinite(points)
    if finite.all():
        lo = points.min(axis=0)
        ext = points.max(axis=0) - lo
    else:   # the box of the finite values: one NaN or Inf row must not flatten the grid for all the others
        lo = np.where(finite, points, np.inf).min(axis=0)
        ext = np.where(finite, points, -np.inf).max(axis=0) - lo
        lo = np.where(np.isfinite(lo), lo, 0.0)
    ext = np.where(np.isfinite(ext) & (ext > 0), ext, 1.0)
    return points, w, np.ascontiguousarray(points - lo), ext


def _radius_range(radius_range):
    """radius_range=None or (rmin, rmax) of findSpheres / findCircles / findCylinders -> (rmin, rmax), checked"""
    if radius_range is None:
        return 0.0, np.inf
    try:
        rmin, rmax = (float(v) for v in radius_range)
    except (TypeError, ValueError):
        raise ValueError("radius_range should be a pair (rmin, rmax)") from None
    if not (rmin >= 0.0 and rmax >= rmin):
        raise ValueError("radius_range should satisfy 0 <= rmin <= rmax (no NaN)")
    return rmin, rmax


def _oriented(est, points, normals):
    """the normals check of the calls on oriented points: normals [n, 3], one row per point, become est.normals; returns the points
    as float64 (their own checks are _point_cloud's)"""
    points, nrm = _as_f64(points), _as_f64(normals)
    if nrm.ndim != 2 or nrm.shape[1] != 3 or (points.ndim == 2 and nrm.shape[0] != points.shape[0]):
        raise ValueError("normals should be an array with dims [n,3], one row per point")
    est.normals = nrm
    return points


def findPlanes(points, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
               neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
               minimum_point_number=10, maximum_model_number=-1, sampler_id=2, scoring_exponent=2,
               do_logging=False, *, seed=None, max_outer_iterations=10, neighborhood="flann_like",
               local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Multi-plane fitting of a 3-D point cloud (no reference counterpart: the findLines pipeline one dimension up).
    points [n, 3]; returns (planes[K, 4] float64 (a, b, c, d) with (a, b, c) a unit normal, labels[n] int32) in findLines'
    labelling convention.  threshold (point-to-plane distance) and neighborhood_ball_radius are in the cloud's own units: the
    defaults (5 cm, 50 cm) suit a metre-scale scene such as a depth-sensor or LiDAR frame.  `weights` [n], when given, weight
    the least-squares refits.  Sampler ids: 0 uniform, 1 PROSAC (points ordered by quality), 2 NAPSAC on the neighbourhood graph
    (the default), 3 Progressive NAPSAC on a grid over the bounding box (1 and 3 take the points as ordered by quality: their
    first samples come from the first points); any other id prints to stderr and returns zero models, as the other entry
    points do.  Large clouds: the compound score value - shared^scoring_exponent squares the support a candidate shares with
    the accepted planes, whose slabs cross every patch, so with the default 2 that penalty grows with n^2 against a value that
    grows with n and later planes lose to tilted partial ones (six-plane scenes at 10^5 points: scoring_exponent=1 recovers all
    six, 2 three to five - DESIGN.md 4.5); minimum_point_number has to exceed the outliers a slab of width 3 x threshold
    holds, or spurious planes through the outliers are accepted."""
    return _find_primitive(_estimators.PlaneEstimator(), points, weights, None, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def _find_primitive(est, points, weights, radius_range, sampler_id, do_logging, radius, **run_kw):
    """findPlanes / findSpheres / findCircles / findLines3D / findCylinders / findCones / findTori / findPrimitives behind their signatures: the estimator says the point dimension (its
    model type's), the sample size (= the fewest points accepted) and the columns of a model.  Only an estimator with a radius takes
    radius_range (its takes_radius_range says so): it goes to the estimator, and the estimator's context_setup puts its per-call state on
    the context."""
    points, w, grid_pts, ext = _point_cloud(points, weights, est.sample_size, dim=_lib.POINT_DIM[est.model_type])
    if est.takes_radius_range:
        est.radius_range = _radius_range(radius_range)
    if do_logging and sampler_id == 1:
        print("Note: PROSAC sampler requires the points to be order by quality, e.g., SNN ratio.")
    models, labels, _ = _run(est, points, points, radius,
                             _sampler_factory(sampler_id, {0: "uniform", 1: "prosac", 2: "napsac", 3: "pnapsac"}, grid_pts, ext,
                                              est.sample_size),
                             do_logging=bool(do_logging), weights=w, setup=est.context_setup, **run_kw)
    return _stack(est, models, est.cols), labels


def findSpheres(points, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
                neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
                minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                do_logging=False, *, radius_range=None, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Multi-sphere fitting of a 3-D point cloud (no reference counterpart: findPlanes' pipeline with a 4-point sphere solver and an
    algebraic refit).  points [n, 3]; returns (spheres[K, 4] float64 (cx, cy, cz, r), labels[n] int32) in findPlanes' labelling
    convention.  threshold bounds the distance from the sphere's surface, abs(|p - c| - r), in the cloud's units.  radius_range=(rmin, rmax)
    (keyword-only; default: any radius) drops hypotheses and refits whose radius lies outside it.  Sampler ids as findPlanes', but
    the default is 3, Progressive NAPSAC on a grid over the bounding box: NAPSAC (2) draws the seed's nearest neighbours, which at
    scan densities lie a few point spacings apart, where the curvature across four points is below the noise and the minimal sphere
    is close to random; the grid's cells span caps with usable curvature.  Samplers 3 and 1 take the points as ordered by quality (every
proposal starts from the first points): shuffle a cloud that comes in scan order.  Like findPlanes, minimum_point_number has to exceed the
    outliers a shell of width 3 x threshold holds."""
    return _find_primitive(_estimators.SphereEstimator(), points, weights, radius_range, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def findCircles(points, weights=None, threshold=2.0, conf=0.5, spatial_coherence_weight=0.0,
                neighborhood_ball_radius=200.0, maximum_tanimoto_similarity=0.4, max_iters=1000,
                minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                do_logging=False, *, radius_range=None, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Multi-circle fitting of a 2-D point set (no reference counterpart: findSpheres one dimension down, with a 3-point circle solver
    and an algebraic refit).  points [n, 2]; returns (circles[K, 3] float64 (cx, cy, r), labels[n] int32) in findPlanes' labelling
    convention.  threshold bounds the distance from the circle, abs(|p - c| - r); it and neighborhood_ball_radius default to findLines'
    pixel-scale values (edge points of round parts, fiducials, arcs).  `weights` [n], when given, weight the least-squares refits.
    radius_range=(rmin, rmax) (keyword-only; default: any radius) drops hypotheses and refits whose radius lies outside it - with straight
    edges in the scene, an rmax of the order of the image size keeps near-lines out.  Sampler ids as findSpheres': 0 uniform, 1 PROSAC,
    2 NAPSAC on the neighbourhood graph, 3 (the default) Progressive NAPSAC on a grid over the bounding box; any other id prints to
    stderr and returns zero models.  Samplers 3 and 1 take the points as ordered by quality (every proposal starts from the first
    points): shuffle a set that comes in contour order.  minimum_point_number has to exceed the outliers an annulus of width
    3 x threshold holds."""
    return _find_primitive(_estimators.CircleEstimator(), points, weights, radius_range, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def findLines3D(points, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
                neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
                minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                do_logging=False, *, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Multi-line fitting of a 3-D point cloud: poles, cables, rails, pipe axes, edges, tracks (no reference counterpart: findPlanes'
    pipeline with a 2-point solver and the scatter's largest eigenvector as the refit).  points [n, 3]; returns (lines[K, 6] float64
    (px, py, pz, dx, dy, dz), a point on the line and a unit direction, labels[n] int32) in findPlanes' labelling convention.  threshold
    bounds the distance from the point to the line's axis, in the cloud's units; the defaults suit a metre-scale scene.  `weights` [n],
    when given, weight the least-squares refits.  Sampler ids as findSpheres': 0 uniform, 1 PROSAC, 2 NAPSAC on the neighbourhood graph,
    3 (the default) Progressive NAPSAC on a grid over the bounding box; any other id prints to stderr and returns zero models.  The
    default follows findSpheres'; measured on make_lines3d scenes (six lines, half outliers, 10^4 to 10^6 points) it is
    not the best choice: with minimum_point_number = n / 150 samplers 2, 1 and 0 found all six lines at every size, 2 and 0 six times
    faster than 3 at 10^6 points, and 3 stopped at three lines at 10^4 - try sampler_id=2 or 0 first on a large cloud.  Samplers 3 and 1
    take the points as ordered by quality (every proposal starts from the first points): shuffle a cloud that comes in scan order.
    minimum_point_number has two lower bounds: the outliers a tube of radius 1.5 x threshold holds along the longest line the scene
    admits, and the points a line crossing two true lines collects from both - about 3 x threshold / sin(angle) of each one's length -
    or spurious lines through the outliers or between two lines are accepted.  It also has an upper side: the run stops when fewer
    inliers than that are predicted as still unseen, and in the same measurement no sampler returned all six lines with n / 40."""
    return _find_primitive(_estimators.Line3DEstimator(), points, weights, None, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def _neighbourhood_graph(k, radius):
    """estimateNormals' and splitComponents' (k, radius), checked -> graph_build's kind, radius and k: k alone the k nearest neighbours,
    both the k nearest inside the ball, the radius alone every point inside the ball"""
    if k is None and radius is None:
        raise ValueError("k or radius should be given")
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
            raise ValueError("k should be an integer >= 2 (or None with a radius)")
    if radius is not None:
        try:
            radius = float(radius)
        except (TypeError, ValueError):
            raise ValueError("radius should be None or a number > 0") from None
        if not (radius > 0.0 and np.isfinite(radius)):
            raise ValueError("radius should be None or a number > 0")
    kind = _lib.GRAPH_BALL if k is None else _lib.GRAPH_KNN if radius is None else _lib.GRAPH_KNN_IN_BALL
    return dict(kind=kind, radius=0.0 if radius is None else radius, k=1 if k is None else int(k))


def estimateNormals(points, k=16, radius=None, viewpoint=None, return_curvature=False):
    """Per-point surface normals of a 3-D point cloud, on the GPU: the eigenvector of the smallest eigenvalue of the covariance of each
    point's neighbourhood in the neighbourhood graph (include/pgx.h pgx_estimate_normals states the arithmetic).  points [n, 3], n >= 3,
    finite; returns normals [n, 3] float64 (unit to rounding) - and, with return_curvature=True, (normals, curvature [n]): the surface
    variation lambda_0 / trace, 0 on a plane, at most 1/3.  The graph: k given and radius None - the k nearest neighbours (the default,
    k = 16; the graph build takes k <= 16); k and radius given - the k nearest inside the ball; k=None and radius given - every point
    inside the ball.  The neighbourhood is the point's row of the SYMMETRIC graph - j is a neighbour of i when either lists the other -
    so a point can have more than k neighbours.  The normals are unsigned (the entry of largest magnitude is made positive) unless a
    viewpoint (3 finite numbers) is given: then each normal points to the half-space of the viewpoint as seen from its point.
    findCylinders accepts either.  Consistent orientation by propagation over the graph is not done.  NaN rows mark undefined normals:
    a point with fewer than two neighbours (a ball that holds none), or a neighbourhood whose covariance is not finite."""
    points = _as_f64(points)
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 3:
        raise ValueError("points should be an array with dims [n,3], n>=3")
    graph = _neighbourhood_graph(k, radius)
    if viewpoint is not None:
        try:
            viewpoint = np.asarray(viewpoint, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("viewpoint should be None or 3 finite numbers") from None
        if viewpoint.shape[0] != 3 or not np.isfinite(viewpoint).all():
            raise ValueError("viewpoint should be None or 3 finite numbers")
    ctx = _context()
    ctx.graph_build(points, fetch=False, **graph)
    normals, curvature, _ = ctx.estimate_normals(points, viewpoint=viewpoint, want_curvature=bool(return_curvature))
    return (normals, curvature) if return_curvature else normals


def splitComponents(points, labels, model_number, k=16, radius=None, minimum_point_number=10, keep="all"):
    """Splits the models of a labelling into instances, on the GPU: a find* call returns models of infinite extent, and a model's label
    collects every point near it - two table tops that happen to be coplanar, the wall behind them, a stripe of the outliers.  An
    instance is a connected piece: a connected component of the model's points in the neighbourhood graph of the cloud (include/pgx.h
    pgx_label_components states the definition).  points [n, d], d = 2 or 3, finite; labels [n] integers in any find* labelling
    convention: 0 .. model_number-1 are the models, anything else - the outlier label, a negative number - is an outlier.  Returns
    (new_labels [n] int32, parent [K'] int32): instance j consists of the points with new_labels == j and is a piece of the model
    parent[j], so the caller writes planes[parent]; K' = len(parent) is the new outlier label.  keep="all": every component of at
    least minimum_point_number points becomes an instance; keep="largest": only the largest component of each model (ties: the one
    with the smallest point index), under the same size test.  Instances are ordered by (model ascending, size descending, smallest
    point index ascending); a model none of whose components passes the size test is absent from parent.
    The graph is estimateNormals': k given and radius None - the k nearest neighbours (the default, k = 16; the graph build takes
    k <= 16); k and radius given - the k nearest inside the ball; k=None and radius given - every point inside the ball.  What the
    neighbourhood means here: two points belong to one surface when a chain of neighbours of the same model joins them, so choose
    radius as the largest gap that still counts as one surface - a few point spacings.  A k-NN graph without a radius joins stragglers
    over any distance: every point has k neighbours however far away, and two pieces a metre apart hang together through them.
    The function is a post-process of a finished labelling: it changes nothing about how the find* calls score, sample or label."""
    points = _as_f64(points)
    if points.ndim != 2 or points.shape[1] not in (2, 3):
        raise ValueError("points should be an array with dims [n,2] or [n,3]")
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != points.shape[0]:
        raise ValueError("labels should be an array with dims [n], one entry per point")
    if labels.dtype == np.bool_ or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("labels should be integers")
    if isinstance(model_number, bool) or not isinstance(model_number, (int, np.integer)) or not 0 <= model_number < 2 ** 31:
        raise ValueError("model_number should be an integer >= 0")
    graph = _neighbourhood_graph(k, radius)
    if isinstance(minimum_point_number, bool) or not isinstance(minimum_point_number, (int, np.integer)) or minimum_point_number < 1:
        raise ValueError("minimum_point_number should be an integer >= 1")
    if keep not in _components.KEEP:
        raise ValueError('keep should be "all" or "largest"')
    model_number = int(model_number)
    if points.shape[0] == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    live = (labels >= 0) & (labels < model_number)              # before the cast to int32: an int64 outlier label may not fit
    device_labels = np.where(live, labels, -1).astype(np.int32)
    ctx = _context()
    ctx.graph_build(points, fetch=False, **graph)
    comp, first, sizes = ctx.label_components(device_labels, model_number)
    return _components.regroup(device_labels, model_number, comp, first, sizes, int(minimum_point_number), keep)


def instanceExtents(points, labels, models, model_type, parent=None):
    """Bounds the instances of a labelling on their surfaces, on the GPU: the find* calls return surfaces of infinite extent and
    splitComponents a label per point; this call says how far along its surface each instance reaches - the length of a pipe, the
    rectangle of a table top, whether a cylinder is a full pipe or a half shell, the covered area of a sphere cap (include/pgx.h
    pgx_instance_extents states the definition).  points [n, 3]; labels [n] integers, 0 .. K'-1 the instances and anything else an
    outlier; models [K, p] rows of model_type - planes 6, spheres 8, 3-D lines 12, cylinders 14, cones 16, tori 22, or the union types
    18 and 20 whose first column is the class; parent [K'] integers as splitComponents returns them: instance j lies on
    models[parent[j]].  parent=None: K' = K and instance j lies on model j.
    Each instance gets a frame - an origin o, an axis g and two directions u, v, orthonormal - and two coordinates (a, b) of e = x - o:
    plane (e.u, e.v); line (e.g, -); cylinder and cone (e.g, the angle about g from u towards v); sphere (the cosine of the angle to
    g = e_z, the azimuth from e_x); torus (the angle about the axis, the angle about the tube's centre circle from the outward
    direction towards g).  Angles are counted in 64 sectors of 2 pi / 64.
    Returns a dict of arrays over the K' instances: kind (0 plane, 1 line, 2 cylinder or cone, 3 sphere, 4 torus, -1 no frame: a row
    with a non-finite parameter, a zero direction or an unknown class), surface (the single model type, -1 without a frame), count,
    origin, axis, u, v [K', 3], radii [K', 2] (cylinder (r, 0), cone (cos, sin) of the half-angle, sphere (r, 0), torus (R, r)), lo
    and hi [K', 2] (the bounds of the linear coordinates; +inf and -inf where there are none), sectors [K', 2] uint64 (the occupied
    sectors of the angular coordinates), occupancy [K'] uint64 (bit 8 bin_a + bin_b of the 8 x 8 grid between the bounds), arc
    [K', 2, 2] (start and length in radians of the shortest run of sectors holding every occupied one; NaN for a linear coordinate),
    area [K'] (the occupied cells in the surface's metric; NaN for a line) - and skipped, the number of points with an instance's label
    that could not be placed (a non-finite coordinate, a point on the axis, an instance without a frame).
    The function is a post-process of a finished labelling: it changes nothing about how the find* calls score, sample or label."""
    points = _as_f64(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points should be an array with dims [n,3]")
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != points.shape[0]:
        raise ValueError("labels should be an array with dims [n], one entry per point")
    if labels.dtype == np.bool_ or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("labels should be integers")
    if isinstance(model_type, bool) or not isinstance(model_type, (int, np.integer)) or int(model_type) not in _extents.MODEL_TYPES:
        raise ValueError("model_type should be one of the 3-D surface types 6, 8, 12, 14, 16, 18, 20, 22")
    model_type = int(model_type)
    models = _as_f64(models)
    if models.ndim != 2 or models.shape[1] != _extents.PARAM_DIM[model_type]:
        raise ValueError(f"models should be an array with dims [K,{_extents.PARAM_DIM[model_type]}] for model_type {model_type}")
    if parent is not None:
        parent = np.asarray(parent)
        if parent.ndim != 1:
            raise ValueError("parent should be None or an array with dims [K']")
        if parent.dtype == np.bool_ or not np.issubdtype(parent.dtype, np.integer):
            raise ValueError("parent should be integers")
        if len(parent) and (parent.min() < 0 or parent.max() >= models.shape[0]):
            raise ValueError("parent should index the rows of models")
    instances = models.shape[0] if parent is None else parent.shape[0]
    if instances > _lib.EXTENTS_MAX_INSTANCES:
        raise ValueError(f"at most {_lib.EXTENTS_MAX_INSTANCES} instances")
    rows, surface = _extents.frames(models, model_type, parent)
    live = (labels >= 0) & (labels < instances)                 # before the cast to int32: an int64 outlier label may not fit
    device_labels = np.where(live, labels, -1).astype(np.int32)
    out = _context().instance_extents(points, device_labels, rows)
    arc, area = _extents.derive(surface, rows, out["lo"], out["hi"], out["sectors"], out["occupancy"])
    return dict(kind=rows[:, 0].astype(np.int32), surface=surface, count=out["count"], skipped=out["skipped"],
                origin=rows[:, 1:4].copy(), axis=rows[:, 4:7].copy(), u=rows[:, 7:10].copy(), v=rows[:, 10:13].copy(),
                radii=rows[:, 13:15].copy(), lo=out["lo"], hi=out["hi"], sectors=out["sectors"], occupancy=out["occupancy"],
                arc=arc, area=area)


def findCylinders(points, normals, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
                  neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
                  minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                  do_logging=False, *, radius_range=None, seed=None, max_outer_iterations=10, neighborhood="flann_like",
                  local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Multi-cylinder fitting of an oriented 3-D point cloud: pipes, columns, trunks, tanks (no reference counterpart: findSpheres'
    pipeline with a 2-point solver on points with normals and a Gauss-Newton refit of the geometric distance).  points [n, 3], normals
    [n, 3] (required): one surface normal per point, as a normal estimator gives them (estimateNormals(points) computes them from the
    cloud itself) - they may be unsigned (either orientation) and
    need not be unit length; only the minimal solver reads them, and a sample whose normals are parallel, zero or not finite gives no
    hypothesis.  Returns (cylinders[K, 7] float64 (px, py, pz, dx, dy, dz, r): a point on the axis - the foot of its points' mean -,
    a unit direction and a radius; labels[n] int32) in findPlanes' labelling convention.  The axis is a line: the model says nothing
    about where the cylinder ends.  threshold bounds the distance from the point to the cylinder's surface, abs(|(x - p) x d| - r), in
    the cloud's units.  radius_range=(rmin, rmax) (keyword-only; default: any radius) drops hypotheses and refits whose radius lies
    outside it.  `weights` [n], when given, weight the least-squares refits.  Sampler ids as findSpheres': 0 uniform, 1 PROSAC, 2 NAPSAC
    on the neighbourhood graph, 3 (the default, following findSpheres) Progressive NAPSAC on a grid over the bounding box; any other id
    prints to stderr and returns zero models.  Samplers 3 and 1 take the points as ordered by quality (every proposal starts from the
    first points): shuffle a cloud that comes in scan order.  Measured on make_cylinders scenes (six cylinders, half outliers, 10^4 to
    10^6 points, radius_range=(0.1, 2)), nothing recovers all six reliably: with minimum_point_number = n / 40 every
    sampler returned three to five cylinders, all but one of them true ones; with n / 150 the default found five, six and five of six
    and uniform sampling six at 10^4 and 10^6, but 8 of those 12 runs also returned up to three cylinders that match no true one.  No
    sampler stood out (NAPSAC, the fastest for 3-D lines, was the slowest at 10^6).  minimum_point_number has to exceed the outliers a
    shell of width 3 x threshold about the largest admitted cylinder holds, and what a cylinder through the crossing of two true ones
    collects, or spurious cylinders are accepted - an rmax keeps that shell small; it also has the upper side findLines3D describes:
    the run stops when fewer inliers than that are predicted as still unseen."""
    est = _estimators.CylinderEstimator()
    points = _oriented(est, points, normals)
    return _find_primitive(est, points, weights, radius_range, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def _angle_range(angle_range):
    """angle_range=(amin, amax) of findCones, half-angles in degrees -> (sin amin, sin amax), checked like radius_range"""
    try:
        amin, amax = (float(v) for v in angle_range)
    except (TypeError, ValueError):
        raise ValueError("angle_range should be a pair (amin, amax) of half-angles in degrees") from None
    if not (amin > 0.0 and amax >= amin and amax < 90.0):
        raise ValueError("angle_range should satisfy 0 < amin <= amax < 90 (degrees, no NaN)")
    return float(np.sin(np.deg2rad(amin))), float(np.sin(np.deg2rad(amax)))


def findCones(points, normals, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
              neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
              minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
              do_logging=False, *, angle_range=(1.0, 89.0), seed=None, max_outer_iterations=10, neighborhood="flann_like",
              local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Multi-cone fitting of an oriented 3-D point cloud: funnels, reducers, hoppers, tapered columns (no reference counterpart:
    findCylinders' pipeline with a 3-point solver on points with normals and a Gauss-Newton refit on six parameters).  points [n, 3],
    normals [n, 3] (required): one surface normal per point, as a normal estimator gives them (estimateNormals(points) computes them
    from the cloud itself) - they may be unsigned and need not be unit length; only the minimal solver reads them, and a sample whose
    three tangent planes have no single common point gives no hypothesis.  Returns (cones[K, 8] float64 (ax, ay, az, dx, dy, dz, c, s):
    the apex, a unit axis direction pointing into the nappe, and the cosine and sine of the half-angle, both positive; labels[n]
    int32) in findPlanes' labelling convention.  The model is one nappe without ends: it says nothing about where the cone is cut.
    threshold bounds abs(c rho - s h) in the cloud's units, with h = (x - a) . d the height over the apex and rho = |(x - a) x d| the
    distance from the axis: the distance to the generatrix line, which is the distance to the surface except behind the apex
    (h c + rho s < 0), where it is smaller than the distance to the apex.  angle_range=(amin, amax) (keyword-only, half-angles in
    degrees, 0 < amin <= amax < 90) drops hypotheses and refits whose half-angle lies outside it.  `weights` [n], when given, weight
    the least-squares refits.  Sampler ids, the remaining arguments and their caveats are findCylinders'; recovery on make_cones
    scenes is reported, not tuned, in DESIGN.md 4.12."""
    est = _estimators.ConeEstimator()
    points = _oriented(est, points, normals)
    return _find_primitive(est, points, weights, _angle_range(angle_range), sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def findTori(points, normals, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
             neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
             minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
             do_logging=False, *, radius_range=(0.0, np.inf), major_radius_range=(0.0, np.inf), seed=None, max_outer_iterations=10,
             neighborhood="flann_like", local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None,
             pearl_abs="double", refit_solver="lapack"):
    """Multi-torus fitting of an oriented 3-D point cloud: pipe elbows, fillets, rings, handles, tyres (no reference counterpart:
    findCones' pipeline with a 4-point solver on points with normals, two hypotheses per sample, and a Gauss-Newton refit on seven
    parameters).  points [n, 3], normals [n, 3] (required): one surface normal per point, as a normal estimator gives them
    (estimateNormals(points) computes them from the cloud itself) - they may be unsigned and need not be unit length; only the minimal
    solver reads them, as LINES: the axis of a surface of revolution meets every one of its normals, and a sample whose four normal
    lines have no common transversal gives no hypothesis.  That makes the solver more sensitive to the normals than the cylinder's and
    the cone's: with normals tilted by 5 degrees few all-inlier samples give a usable torus.  Returns (tori[K, 8]
    float64 (cx, cy, cz, dx, dy, dz, R, r): the centre, a unit axis direction (its sign means nothing), the major radius from the axis
    to the tube's centre circle and the minor (tube) radius; labels[n] int32) in findPlanes' labelling convention.  The model is a
    whole RING torus, R > r > 0: it says nothing about which arc of an elbow exists, and spindle or horn tori are never returned.
    threshold bounds abs(sqrt((rho - R)^2 + h^2) - r) in the cloud's units, with h = (x - c) . d the height over the centre plane and
    rho = |(x - c) x d| the distance from the axis: the distance from the torus' surface.  radius_range=(rmin, rmax) bounds the tube
    radius r and major_radius_range=(Rmin, Rmax) the major radius R (both keyword-only; default: any) of hypotheses and refits.
    `weights` [n], when given, weight the least-squares refits.  Sampler ids, the remaining arguments and their caveats are
    findCylinders'; recovery on make_tori scenes is reported, not tuned, in DESIGN.md 4.15."""
    est = _estimators.TorusEstimator()
    points = _oriented(est, points, normals)
    try:
        est.major_radius_range = _radius_range(major_radius_range)
    except ValueError as e:
        raise ValueError(str(e).replace("radius_range", "major_radius_range")) from None
    return _find_primitive(est, points, weights, radius_range, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


PRIMITIVE_CLASSES = dict(_estimators.PRIMITIVE_CLASSES)   # name -> class number (column 0 of findPrimitives' models)


def findPrimitives(points, normals, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
                   neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
                   minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                   do_logging=False, *, classes=("plane", "sphere", "cylinder", "cone"), radius_range=None, angle_range=(1.0, 89.0), seed=None,
                   max_outer_iterations=10, neighborhood="flann_like", local_optimization="auto", labeling_l0="greedy", distributed=None,
                   sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """Planes, spheres, cylinders and cones of an oriented 3-D point cloud in ONE fit: walls, tanks, pipes and reducers of the same scan
    compete for its points under one compound score, one Tanimoto validation and one labelling (no reference counterpart: findCones'
    pipeline on a model type whose instances carry their class).  points [n, 3], normals [n, 3].  The normals are REQUIRED whatever the
    classes - also for classes=("plane",), whose solver does not read them: a sample is four oriented points, and the call does not
    change its inputs with its options.  They may be unsigned and need not be unit length; only the minimal solvers of cylinders and
    cones read them.  estimateNormals(points, radius=...) computes them from the cloud itself: choose its radius against the noise, a
    few times sigma at least (16 nearest neighbours of a dense scan see only its noise).
    Returns (models[K, 9] float64, labels[n] int32) in findPlanes' labelling convention.  Column 0 of a model is its class number
    (PRIMITIVE_CLASSES: plane 6, sphere 8, cylinder 14, cone 16), columns 1 .. 8 that class's model row as findPlanes (a, b, c, d),
    findSpheres (cx, cy, cz, r), findCylinders (px, py, pz, dx, dy, dz, r) and findCones (ax, ay, az, dx, dy, dz, c, s) return it, padded
    with zeros.  threshold bounds the class's own residual, in the cloud's units.  Every sample of four points gives up to four
    hypotheses: the plane of its first three points, the sphere of all four, the cylinder of the first two and the cone of the first
    three with their normals.  An instance never changes class: refits keep the class of the hypothesis they start from.
    classes (keyword-only) selects the classes that are proposed, by name; radius_range=(rmin, rmax) bounds the radii of spheres and
    cylinders (default: any), angle_range=(amin, amax) the half-angles of cones in degrees, 0 < amin <= amax < 90.  PEARL refits no
    instance with fewer points than the largest refit among the selected classes needs (6 with cones).  `weights`, the sampler ids and
    the remaining arguments are findCones'.  What the call recovers on make_primitives scenes, and what the four single-class calls
    find on the same scenes, is reported, not tuned, in DESIGN.md 4.13."""
    est = _estimators.PrimitiveEstimator(classes)
    points = _oriented(est, points, normals)
    est.sine_range = _angle_range(angle_range)
    return _find_primitive(est, points, weights, radius_range, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def findOrientedPrimitives(points, normals, weights=None, threshold=0.05, conf=0.5, spatial_coherence_weight=0.0,
                           neighborhood_ball_radius=0.5, maximum_tanimoto_similarity=0.4, max_iters=1000,
                           minimum_point_number=10, maximum_model_number=-1, sampler_id=3, scoring_exponent=2,
                           do_logging=False, *, normal_tolerance=20.0, classes=("plane", "sphere", "cylinder", "cone"), radius_range=None,
                           angle_range=(1.0, 89.0), seed=None, max_outer_iterations=10, neighborhood="flann_like", local_optimization="auto",
                           labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """findPrimitives with the compatibility test of Schnabel, Wahl and Klein ("Efficient RANSAC for Point-Cloud Shape Detection", 4.3): a
    point supports a plane, sphere, cylinder or cone only if it lies within `threshold` of it AND its normal deviates from the shape's
    normal at that point by less than `normal_tolerance` degrees.  Under findPrimitives the normals are read by the minimal solvers
    alone, and a flexible shape collects the points of a wall or of the outlier cloud by distance; here scores, preference vectors,
    PEARL's data costs, the inlier / outlier cut and the inlier lists of the refits all apply the test (model type 20: DESIGN.md 4.14).
    A hypothesis that disagrees with the normals of its own sample is never scored.
    points [n, 3], normals [n, 3]: unsigned and unnormalised normals are fine (the test squares the cosine); a zero or non-finite
    normal supports nothing.  normal_tolerance (keyword-only, degrees, 0 < tolerance <= 90; else ValueError) defaults to 20, the order
    of magnitude Schnabel et al. use - a default, NOT a value tuned on this project's scenes; normals estimated from a noisy scan want
    a tolerance above their own error (DESIGN.md 4.14 reports 10, 20 and 40 degrees as found).  90 degrees accepts every defined
    normal.  All other parameters, their order and the return value (models[K, 9], labels[n]) are findPrimitives'; the refits are
    the same least-squares fits on the compatible inliers, and the distance sums PEARL compares before and after a refit ignore the
    normals (they are the quantity the refits minimise)."""
    est = _estimators.OrientedPrimitiveEstimator(classes, normal_tolerance)
    points = _oriented(est, points, normals)
    est.sine_range = _angle_range(angle_range)
    return _find_primitive(est, points, weights, radius_range, sampler_id, do_logging, neighborhood_ball_radius,
                           **_run_options(locals()))


def find6DPoses(x1y1, x2y2z2, K, threshold=4.0, conf=0.90, spatial_coherence_weight=0.1,
                neighborhood_ball_radius=20.0, maximum_tanimoto_similarity=0.9, max_iters=400,
                minimum_point_number=2 * 3, maximum_model_number=-1, *, seed=None, max_outer_iterations=10, scoring_exponent=2,
                neighborhood="flann_like",
                     local_optimization="auto", labeling_l0="greedy", distributed=None, sampler_rng="numpy", trace=None, pearl_abs="double", refit_solver="lapack"):
    """bindings.cpp:9-97, progressivex_python.cpp:41-171.  Returns (P[(3K),4], labels[n]).
    scoring_exponent [keyword-only, not in the reference's signature]: the driver never calls setScoringExponent, so the class default
    2 applies (progressive_x.h:183) - the default here.  The compound-model score is value - shared^exponent
    (scoring_function_with_compound_model.h:110-121): at 10^6 points a new object's incidental overlap with a dozen accepted models
    (~300-500 units of shared support) squared exceeds its whole value (~47 000), its score goes negative and junk hypotheses win the
    proposal - the call stops at 12-14 of BASELINE config C4's 16 objects (scripts/c4_missing.py).  exponent = 1 keeps the penalty
    on the scale of the support."""
    import time
    x1 = _as_f64(x1y1)
    n, dim = _shape2(x1)
    if dim != 2 or n < 3:
        raise ValueError("x1y1 should be an array with dims [n,2], n>=3")            # bindings.cpp:26-31
    x2 = _as_f64(x2y2z2)
    na, dima = _shape2(x2)
    if dima != 3:
        raise ValueError("x2y2z2 should be an array with dims [n,3], n>=3")          # :37-39
    if na != n:
        raise ValueError("x1y1 and x2y2z2 should be the same size")                  # :40-42
    Km = _as_f64(K)
    if Km.ndim != 2 or Km.shape != (3, 3):
        raise ValueError("K should be an array with dims [3,3]")                     # :48-50
    Kinv = np.linalg.inv(Km)                                                          # progressivex_python.cpp:69-70
    un = Kinv[0, 0] * x1[:, 0] + Kinv[0, 1] * x1[:, 1] + Kinv[0, 2]                    # :88
    vn = Kinv[1, 0] * x1[:, 0] + Kinv[1, 1] * x1[:, 1] + Kinv[1, 2]                    # :89
    normalized = np.ascontiguousarray(np.column_stack([un, vn, x2]))                   # :88-92
    raw = np.column_stack([x1, x2])                                                    # :82-86 (graph on RAW points)
    f = 0.5 * (Km[0, 0] + Km[1, 1])                                                    # :96
    t0 = time.perf_counter()
    est = _estimators.PnPEstimator()

    def factory(n_, rng, graph):
        print("Neighborhood calculation time = %f secs." % (time.perf_counter() - t0))   # :109
        return _proposal.UniformSampler(n_, rng)                                          # :112 always uniform
    factory.needs_graph = False

    models, labels, _ = _run(est, normalized, raw, neighborhood_ball_radius, factory,
                             **_run_options(locals(), threshold=threshold / f, scoring_exponent=int(scoring_exponent)))
    return _stack(est, models, 4), labels
