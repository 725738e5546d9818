"""The host-side size switches of the C ABI (progressive-x_amd/csrc/*.hip), both sides of each, and the hand-over of resident state
between unlike problems on one context.

The kernels are compared with the oracle at wave and block edges elsewhere (tests/test_gpu_parity.py).  The switches here are HOST
constants that pick another copy path, buffer layout or launch plan once an argument passes a size; every case below names the
constant, the sizes on each side and - for the read-back ring - the bytes of the copy, read off the code, so that the straddle can
be checked by arithmetic.  Bars are those of tests/test_gpu_parity.py: integers bit for bit, floating sums 1e-9 of the matrix or
value scale; where the design makes a result independent of the batch size (one wave per selection, one lane per matrix, the same
reduction tree) the batched call is also compared bitwise with the same call made one item at a time.

The read-back ring (capi.hip d2h / sync_deliver): a copy of at most kStageMax = 32 768 bytes is staged in the pinned ring and
delivered after the synchronisation, a longer one goes straight into the caller's memory.  The ring's second condition,
h_rb_used + bytes > kStageRing = 262 144, cannot be met by any entry point today: the ring is emptied by every sync_deliver and by
CTX_GUARD, and no entry point enqueues more than three copies between two deliveries.  pgx_graph_fetch comes closest - offsets,
neighbours and multiplicities, three copies of at most 32 768 bytes: 98 304 bytes in flight
(test_graph_fetch_either_side_of_the_ring, first case); pgx_gram_batch, pgx_pnp_refine_batch, pgx_eigh_smallest_batch and
pgx_bucket enqueue two.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import csr_from_pairs, make_case
from pyprogressivex import _lib

pytestmark = pytest.mark.gpu

REL = 1e-9
STAGE_MAX = 32768          # capi.hip kStageMax
NORM = np.array([0.01, 300.0, 200.0, 0.012, 310.0, 190.0])     # Hartley normalisation of the DLT rows, as tests/test_gpu_parity.py


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


def _close(G, Gr):
    """a floating sum against the oracle's: 1e-9 of the matrix scale, which must not be zero"""
    scale = float(np.abs(Gr).max())
    assert scale > 0.0, "degenerate reference: the Gram scale is zero"
    return float(np.abs(np.asarray(G) - Gr).max()) <= REL * scale


def _same(a, b):
    """bitwise equality of nested results (dicts of arrays, tuples, scalars)"""
    if isinstance(a, dict):
        return all(_same(a[k], b[k]) for k in a if not k.startswith("_"))
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_score(got, ref, exponent=2, masks=True, what=""):
    assert np.array_equal(got["counts"], ref["counts"]), f"{what}: inlier counts differ"
    if masks:
        assert np.array_equal(got["masks"], ref["masks"]), f"{what}: inlier masks differ"
    assert _rel(got["values"], ref["values"]) <= REL, what
    assert _rel(got["shared"], ref["shared"]) <= REL, what
    scale = np.maximum(np.abs(ref["values"]), np.abs(ref["shared"]) ** exponent) + 1e-300
    assert np.max(np.abs(got["scores"] - ref["scores"]) / scale) <= REL, what


_CASES = {}


def _case(name, n, M, seed):
    """make_case, computed once per argument set and shared (the arrays are never written)"""
    key = (name, n, M, seed)
    if key not in _CASES:
        _CASES[key] = make_case(name, n, M, seed=seed)
        for a in _CASES[key][1:3]:
            a.setflags(write=False)
    return _CASES[key]


# ----------------------------------------------------------------------------------------------------------------------
# A.1  the read-back ring: one batch just under and one just over 32 768 bytes of read-back
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [91, 92])
def test_gram_batch_either_side_of_the_ring(gpu_ctx, oracle, B):
    """pgx_gram_batch, GRAM_DLT_H: nv = 45 doubles per selection.  B = 91: 91 * 45 * 8 = 32 760 bytes (staged); B = 92: 33 120 bytes
    (direct); the bad counters, 4 B bytes, are staged in both.  One wave per selection reduces its own rows by a fixed shuffle tree,
    so row b is bitwise the B = 1 call on selection b."""
    assert 91 * 45 * 8 <= STAGE_MAX < 92 * 45 * 8
    n, m = 500, 14
    mt, pts, _, _ = _case("homography", n, 1, 3)
    rng = np.random.default_rng(B)
    gpu_ctx.set_points(mt, pts)
    weights = rng.random(n) + 0.5
    index = np.array([rng.choice(n, m, replace=False) for _ in range(B)]).astype(np.int32)
    prm = np.array([NORM * (1.0 + 0.1 * rng.random(6)) for _ in range(B)])
    for w, wpow in ((None, 2), (weights, 1), (weights, 2)):
        G, bad = gpu_ctx.gram_batch(_lib.GRAM_DLT_H, index, params=prm, weights=w, wpow=wpow)
        assert G.shape == (B, 9, 9) and bad.shape == (B,)
        for b in range(B):
            G1, bad1 = gpu_ctx.gram_batch(_lib.GRAM_DLT_H, index[b:b + 1], params=prm[b:b + 1], weights=w, wpow=wpow)
            assert np.array_equal(G[b], G1[0]) and bad[b] == bad1[0], f"row {b} of {B} is not the one-selection call (wpow {wpow})"
            Gr, _, badr = oracle.gram(_lib.GRAM_DLT_H, pts, index[b], params=prm[b], weights=w, wpow=wpow)
            assert int(bad[b]) == badr and _close(G[b], Gr), f"row {b} of {B}, wpow {wpow}"


def _sparse_labels(rng, n, K, populated):
    labels = rng.choice(np.array(list(populated) + [K], dtype=np.int32), n).astype(np.int32)     # label K = outlier
    for k in populated:
        assert (labels == k).sum() > 0
    return labels


def _check_gram_labels(gpu_ctx, oracle, kind, pts, labels, K, populated, prm, w, wpow, singles):
    G, cnt, bad = gpu_ctx.gram_labels(kind, K, params=prm, weights=w, wpow=wpow)
    empty = np.ones(K, bool)
    empty[list(populated)] = False
    assert not cnt[empty].any() and not bad[empty].any() and not G[empty].any(), "an empty label came back with a count or a matrix"
    for k in singles:                                         # the single-label call: the same kernels with one item
        Gk, ck, bk = gpu_ctx.gram(kind, ("label", k), params=None if prm is None else prm[k], weights=w, wpow=wpow)
        assert np.array_equal(G[k], Gk) and (int(cnt[k]), int(bad[k])) == (ck, bk), f"label {k} of {K}, wpow {wpow}"
    for k in populated:
        Gr, cntr, badr = oracle.gram(kind, pts, np.flatnonzero(labels == k), params=None if prm is None else prm[k], weights=w, wpow=wpow)
        assert (int(cnt[k]), int(bad[k])) == (cntr, badr) and cntr > 0 and _close(G[k], Gr), f"label {k} of {K}, wpow {wpow}"


@pytest.mark.parametrize("K", [89, 90, 91, 92])
def test_gram_labels_either_side_of_the_ring(gpu_ctx, oracle, K):
    """pgx_gram_labels reads result and counters back in ONE copy of K * nv * 8 + 2 K * 4 bytes (fit.hip gram_labels_launch).
    GRAM_DLT_H, nv = 45: K = 89: 32 040 + 712 = 32 752 bytes (staged); K = 90: 32 400 + 720 = 33 120 (direct); K = 91: 33 488 and
    K = 92: 33 856 (direct; the sizes at which the result alone crosses).  Most labels are empty, four are populated, label K is the
    outlier label.  pgx_gram is the one-item call of the same gram_kernel / gram_final_kernel (blockIdx.y = label): entry k is
    bitwise the single-label call - one kernel compared with itself here; tests/test_gpu_reductions.py pins the bits."""
    assert 89 * (45 * 8 + 8) <= STAGE_MAX < 90 * (45 * 8 + 8) and 91 * 45 * 8 <= STAGE_MAX < 92 * 45 * 8
    n = 3001
    mt, pts, _, _ = _case("homography", n, 1, 4)
    rng = np.random.default_rng(K)
    populated = (0, 1, K // 2, K - 1)
    labels = _sparse_labels(rng, n, K, populated)
    gpu_ctx.set_points(mt, pts)
    gpu_ctx.set_labels(labels)
    weights = rng.random(n) + 0.5
    prm = np.array([NORM * (1.0 + 0.001 * k) for k in range(K)])
    for w, wpow in ((None, 2), (weights, 1), (weights, 2)):
        _check_gram_labels(gpu_ctx, oracle, _lib.GRAM_DLT_H, pts, labels, K, populated, prm, w, wpow, range(K))


@pytest.mark.parametrize("K", [585, 586, 4096])
def test_gram_labels_up_to_the_label_limit(gpu_ctx, oracle, K):
    """The affine rows of 2-D points, nv = 6: one copy of K * 48 + 2 K * 4 = 56 K bytes.  K = 585: 32 760 (staged); K = 586: 32 816
    (direct); K = 4096, the most pgx_gram_labels accepts: 229 376 (direct), grid (blocks, 4096), scratch partials[4096][12][6] | out |
    counters[8192] | prm[4096][12] behind one fused upload.  K = 4097 is refused."""
    assert 585 * 56 <= STAGE_MAX < 586 * 56
    n = 3001
    mt, pts, _, _ = _case("line", n, 1, 5)
    rng = np.random.default_rng(K)
    populated = (0, 1, K // 2 - 1, K - 1)
    labels = _sparse_labels(rng, n, K, populated)
    gpu_ctx.set_points(mt, pts)
    gpu_ctx.set_labels(labels)
    weights = rng.random(n) + 0.5
    singles = sorted(set(populated) | {2, K // 2, K - 2})
    for w, wpow in ((None, 2), (weights, 2)):
        _check_gram_labels(gpu_ctx, oracle, _lib.GRAM_AFFINE, pts, labels, K, populated, None, w, wpow, singles)
    if K == 4096:
        with pytest.raises(_lib.PgxError, match="pgx_gram_labels"):
            gpu_ctx.gram_labels(_lib.GRAM_AFFINE, 4097)
        _check_gram_labels(gpu_ctx, oracle, _lib.GRAM_AFFINE, pts, labels, K, populated, None, None, 2, populated)   # the refusal left the state alone


@pytest.mark.parametrize("K", [4096, 4097])
def test_residual_sums_either_side_of_the_ring(gpu_ctx, oracle, K):
    """pgx_residual_sums reads K doubles back: K = 4096: 32 768 bytes (staged, the largest staged copy there is); K = 4097: 32 776
    (direct).  pgx_residual_sum is the K = 1 call of the same kernels (blockIdx.y = label - label0): sums[k] is bitwise
    pgx_residual_sum(model k, k) - one kernel compared with itself here; tests/test_gpu_reductions.py pins the bits."""
    assert 4096 * 8 <= STAGE_MAX < 4097 * 8
    n = 3001
    mt, pts, base, _ = _case("line", n, 7, 6)
    rng = np.random.default_rng(K)
    populated = (0, 1, K // 2, K - 1)
    labels = _sparse_labels(rng, n, K, populated)
    gpu_ctx.set_points(mt, pts)
    gpu_ctx.set_labels(labels)
    models = np.ascontiguousarray(base[np.arange(K) % len(base)])
    sums = gpu_ctx.residual_sums(models)
    empty = np.ones(K, bool)
    empty[list(populated)] = False
    assert not sums[empty].any()
    for k in populated:
        ref = oracle.residual_sum(mt, pts, models[k], labels, k)
        assert ref > 0.0 and abs(sums[k] - ref) <= REL * ref
        assert sums[k] == gpu_ctx.residual_sum(models[k], k)


@pytest.fixture(scope="module")
def pose_refits(oracle):
    """342 selections of 21 inliers of one pose, starts slightly off, with known failures spread through the batch (a point on the
    camera plane of the start), and the CPU reference of all of them, computed once: the host iteration of PnPEstimator._fit_many
    (numpy, pseudo-inverse with the kernel's cut-off) on the ORACLE's Gram matrices."""
    from pyprogressivex import _estimators
    n, m, B = 2000, 21, 342
    mt, pts, models, thr = _case("pnp", n, 3, 21)
    rng = np.random.default_rng(12)
    with np.errstate(invalid="ignore"):
        inl = np.flatnonzero(oracle.squared_residuals(mt, pts, models[0]) < 2.25 * thr * thr)
    assert len(inl) > 3 * m
    picks = np.array([np.sort(rng.choice(inl, m, replace=False)) for _ in range(B)]).astype(np.int32)
    inits = np.tile(models[0], (B, 1)).reshape(B, 3, 4)
    inits[:, :, 3] += rng.normal(0, 0.01, (B, 3))
    failing = (0, 7, 170, 340, 341)
    for b in failing:                                        # z_c = 0 for the selection's first point
        inits[b, 2, 3] = -float(inits[b, 2, :3] @ pts[picks[b, 0], 2:5])
    inits = inits.reshape(B, 12)

    def gram(kind, prm, use_w, wpow, rows):
        out = [oracle.gram(kind, pts, picks[r], params=prm[j]) for j, r in enumerate(rows)]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
    ref = _estimators.ESTIMATORS["pnp"]()._fit_many(gram, B, list(inits))
    assert [len(r) for r in ref] == [0 if b in failing else 1 for b in range(B)], "the reference fails exactly at the planted rows"
    return mt, pts, picks, inits, failing, ref


@pytest.mark.parametrize("B", [341, 342])
def test_pnp_refine_batch_either_side_of_the_ring(gpu_ctx, pose_refits, B):
    """pgx_pnp_refine_batch reads B poses of 12 doubles back: B = 341: 32 736 bytes (staged); B = 342: 32 832 (direct); the status
    words, 4 B bytes, are staged in both.  One wave owns one selection for all its Gauss-Newton steps: row b is bitwise the B = 1
    call, failures included.  Against the CPU iteration: 1e-9 of max(1, |pose|), the bar of
    test_device_pose_refits_reproduce_the_host_iteration."""
    assert 341 * 96 <= STAGE_MAX < 342 * 96
    mt, pts, picks, inits, failing, ref = pose_refits
    gpu_ctx.set_points(mt, pts)
    P, ok = gpu_ctx.pnp_refine_batch(inits[:B], picks[:B])
    assert [bool(v) for v in ok] == [b not in failing for b in range(B)]
    for b in range(B):
        P1, ok1 = gpu_ctx.pnp_refine_batch(inits[b:b + 1], picks[b:b + 1])
        assert np.array_equal(P[b], P1[0], equal_nan=True) and ok[b] == ok1[0], f"row {b} of {B} is not the one-selection call"
        if ok[b]:
            assert np.abs(P[b] - ref[b][0]).max() <= REL * max(1.0, np.abs(ref[b][0]).max()), f"row {b} of {B}"
    # fewer than 4 points: every selection of the batch fails (m is a property of the batch), in the batch as one by one
    P, ok = gpu_ctx.pnp_refine_batch(inits[:B], picks[:B, :3])
    assert not ok.any()
    for b in (0, 1, B // 2, B - 1):
        P1, ok1 = gpu_ctx.pnp_refine_batch(inits[b:b + 1], picks[b:b + 1, :3])
        assert np.array_equal(P[b], P1[0], equal_nan=True) and not ok1[0]


def _eigen_mix(rng, B, q):
    """symmetric matrices with the bad ones of test_device_jacobi_eigen_solver_is_bitwise_the_oracles spread through the batch"""
    X = rng.standard_normal((B, 12, q))
    A = np.einsum("bni,bnj->bij", X, X)
    k = np.arange(B)
    A[k % 9 == 1] *= 1e-12
    A[k % 9 == 2] *= 1e12
    A[k % 61 == 3] = 0.0
    A[k % 61 == 4] = np.eye(q)
    A[k % 61 == 5, 0, 0] = np.nan
    rows = k % 9 == 6
    A[rows, :, 0] *= 1e-5
    A[rows, 0, :] *= 1e-5
    return A


@pytest.mark.parametrize("q,B", [(9, 455), (9, 456), (3, 4096), (3, 4097), (9, 20011)])
def test_eigh_smallest_batch_either_side_of_the_ring(gpu_ctx, oracle, q, B):
    """pgx_eigh_smallest_batch reads B * q * 8 bytes of vectors and B * 8 of values back.  q = 9: B = 455: 32 760 bytes of vectors
    (staged); B = 456: 32 832 (direct).  Values: B = 4096: 32 768 (staged); B = 4097: 32 776 (direct).  B = 20 011: both direct, 313
    workgroups.  One lane per matrix in the oracle's operation order: array_equal whatever the batch."""
    assert 455 * 72 <= STAGE_MAX < 456 * 72 and 4096 * 8 <= STAGE_MAX < 4097 * 8
    A = _eigen_mix(np.random.default_rng(B), B, q)
    vec, val = gpu_ctx.eigh_smallest_batch(A)
    rvec, rval, _ = oracle.eigh_smallest(A)
    assert np.array_equal(vec, rvec, equal_nan=True) and np.array_equal(val, rval, equal_nan=True)
    assert np.isfinite(rval).sum() > B // 2 and np.isnan(rval).any()


@pytest.mark.parametrize("S", [1365, 1366])
def test_solve_minimal_models_either_side_of_the_ring(gpu_ctx, oracle, S):
    """pgx_solve_minimal(models_out), 2-point lines: S * 3 * 8 bytes.  S = 1365: 32 760 (staged); S = 1366: 32 784 (direct)."""
    assert 1365 * 24 <= STAGE_MAX < 1366 * 24
    n = 3001
    mt, pts, _, _ = _case("line", n, 1, 5)
    samples = np.random.default_rng(S).integers(0, n, (S, 2)).astype(np.int32)
    samples[:5, 1] = samples[:5, 0]                                                  # degenerate: NaN rows
    gpu_ctx.set_points(mt, pts)
    got = gpu_ctx.solve_minimal(samples)
    ref = oracle.solve_minimal(mt, pts, samples)
    assert np.isnan(ref[:5]).all() and np.isfinite(ref[:, 0]).sum() > S // 2 and np.array_equal(got, ref, equal_nan=True)


@pytest.mark.parametrize("S", [4096, 4097])
def test_sampled_rows_either_side_of_the_ring(gpu_ctx, oracle, S):
    """pgx_solve_minimal_sampled(samples_out), 2-point lines: S * 2 * 4 bytes.  S = 4096: 32 768 (staged); S = 4097: 32 776 (direct)."""
    assert 4096 * 8 <= STAGE_MAX < 4097 * 8
    n = 3001
    mt, pts, _, _ = _case("line", n, 1, 5)
    gpu_ctx.set_points(mt, pts)
    key, batch = 0xFEEDFACE12345678, 11
    models, smp = gpu_ctx.solve_minimal_sampled(key, batch, S, fetch=True, fetch_samples=True)
    want = oracle.sample_uniform(key, batch, 0, S, n, 2)
    assert np.array_equal(smp, want)
    assert np.array_equal(models, oracle.solve_minimal(mt, pts, want), equal_nan=True)


def test_score_inliers_either_side_of_the_ring(gpu_ctx, oracle):
    """pgx_score_inliers beyond kCompactSmall points reads count * 4 bytes back: at most 8 192 inliers staged, more direct."""
    n = 20011
    mt, pts, models, thr = _case("line", n, 3, 8)
    gpu_ctx.set_points(mt, pts)
    seen = set()
    for T2 in (2.25 * thr * thr, 1e12):
        gpu_ctx.score(models, T2, want_masks=True)
        for row in range(len(models)):
            with np.errstate(invalid="ignore"):
                ref = np.flatnonzero(oracle.squared_residuals(mt, pts, models[row]) < T2)
            assert np.array_equal(gpu_ctx.score_inliers(row), ref)
            seen.add(len(ref) * 4 > STAGE_MAX)
            seen.add(0 < len(ref) * 4 <= STAGE_MAX)
    assert seen == {True, False} and len(ref) > 8192


@pytest.mark.parametrize("n,pairs", [(8191, 4096), (8192, 4096), (8192, 4097)])
def test_graph_fetch_either_side_of_the_ring(gpu_ctx, n, pairs):
    """pgx_graph_fetch enqueues THREE copies before one delivery - the most of any entry point: offsets (n + 1) * 4 bytes, neighbours
    and multiplicities E * 4 each.  (8191, 4096 pairs): 32 768 + 32 768 + 32 768, all staged, 98 304 bytes in the ring at once;
    (8192, 4096): offsets 32 772 direct between two staged copies; (8192, 4097): E = 8194, all three direct.  The reference is the CSR
    that was set."""
    assert (8191 + 1) * 4 <= STAGE_MAX < (8192 + 1) * 4 and 2 * 4096 * 4 <= STAGE_MAX < 2 * 4097 * 4
    rng = np.random.default_rng(n + pairs)
    iu = rng.permutation(n - 1)[:pairs]                       # pairs (i, i + 1): distinct, never a self-loop
    graph = csr_from_pairs(n, iu, iu + 1, rng.integers(1, 3, pairs))
    gpu_ctx.set_graph(*graph)
    assert gpu_ctx.graph_size() == (n, 2 * pairs)
    for a, b in zip(gpu_ctx.graph_fetch(), graph):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [4096, 4097])
def test_preference_vectors_either_side_of_the_ring(gpu_ctx, oracle, n):
    """pgx_preference(pref_out), pgx_get_preference and pgx_get_compound read n doubles back: n = 4096: 32 768 bytes (staged);
    n = 4097: 32 776 (direct).  Bit-exact, as everywhere."""
    assert 4096 * 8 <= STAGE_MAX < 4097 * 8
    mt, pts, models, thr = _case("line", n, 3, n)
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(mt, pts)
    prefs = np.stack([oracle.preference(mt, pts, m, T2) for m in models])
    assert (prefs > 0).any()
    for k, m in enumerate(models):
        assert np.array_equal(gpu_ctx.preference(m, T2, slot=k, want_pref=True)["pref"], prefs[k])
    for k in range(len(models)):
        assert np.array_equal(gpu_ctx.get_preference(k), prefs[k])
    assert np.array_equal(gpu_ctx.compound_update(np.arange(len(models)), want_compound=True), oracle.compound_max(prefs))
    assert np.array_equal(gpu_ctx.get_compound(), oracle.compound_max(prefs))


# ----------------------------------------------------------------------------------------------------------------------
# A.2  long index lists in pgx_gram: the fused upload of counters | index stops at kFusedIndexMax = 65 536 entries
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,prm", [("line", _lib.GRAM_AFFINE, None), ("plane", _lib.GRAM_AFFINE, None),
                                           ("homography", _lib.GRAM_DLT_H, NORM), ("sphere", _lib.GRAM_SPHERE, np.array([5.1, 4.9, 5.3, 2.5])),
                                           ("circle", _lib.GRAM_CIRCLE, np.array([510.0, 490.0, 250.0]))])
def test_gram_index_lists_either_side_of_the_fused_upload(gpu_ctx, oracle, name, kind, prm):
    """fit.hip gram_launch: up to 65 536 entries the index list is uploaded in one command with the 64 zero bytes of the counters in
    front of it; a longer one is uploaded from the caller's array behind a memset of the two counters in use.  m = 65 536 (fused),
    65 537 and 70 001 (a permutation of all points; separate), with and without weights, each call twice (fixed reduction tree:
    array_equal), and a short list after every long one and the other way round - counters and index share the scratch buffer.  An
    index list whose entry at position 65 536 is out of range is refused before anything is enqueued."""
    n = 70001
    mt, pts, _, _ = _case(name, n, 1, 13)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.int32)
    weights = rng.random(n) + 0.5
    gpu_ctx.set_points(mt, pts)

    def check(index, w, wpow):
        G, cnt, bad = gpu_ctx.gram(kind, ("index", index), params=prm, weights=w, wpow=wpow)
        Gr, cntr, badr = oracle.gram(kind, pts, index, params=prm, weights=w, wpow=wpow)
        assert (cnt, bad) == (cntr, badr) == (len(index), 0), f"{name} m = {len(index)}"
        assert _close(G, Gr), f"{name} m = {len(index)} wpow {wpow}"
        return G
    short = perm[-100:]
    check(short[:1], None, 2)
    for m in (65536, 65537, 70001):
        for w, wpow in ((None, 2), (weights, 2), (weights, 1)):
            G = check(perm[:m], w, wpow)
            assert np.array_equal(G, gpu_ctx.gram(kind, ("index", perm[:m]), params=prm, weights=w, wpow=wpow)[0]), f"{name} m = {m}: not reproducible"
            check(short, w, wpow)
    bad_list = perm[:65537].copy()
    bad_list[65536] = n
    with pytest.raises(_lib.PgxError, match="out of range"):
        gpu_ctx.gram(kind, ("index", bad_list), params=prm)
    bad_list[65536] = -1
    with pytest.raises(_lib.PgxError, match="out of range"):
        gpu_ctx.gram(kind, ("index", bad_list), params=prm)
    check(short, None, 2)
    check(perm[:65537], weights, 2)


# ----------------------------------------------------------------------------------------------------------------------
# A.3  scoring batch sizes: the locality reorder (M > 64), the padding of the batch to 256, the host mirror
# ----------------------------------------------------------------------------------------------------------------------
def _spread16(x):
    x = x & 0xffff
    x = (x | (x << 8)) & 0x00ff00ff
    x = (x | (x << 4)) & 0x0f0f0f0f
    x = (x | (x << 2)) & 0x33333333
    x = (x | (x << 1)) & 0x55555555
    return x


def _locality_keys(mt, models):
    """capi.hip locality_keys restated: the Morton code of where a hypothesis sends its probe point; None for the model types that
    are not reordered"""
    q = np.asarray(models, dtype=np.float64)
    with np.errstate(all="ignore"):
        if mt == _lib.PNP:
            x, y = q[:, 3] / q[:, 11], q[:, 7] / q[:, 11]
        elif mt in (_lib.HOMOGRAPHY, _lib.HOMOGRAPHY_SYM):
            x, y = q[:, 2] / q[:, 8], q[:, 5] / q[:, 8]
        else:
            return None
    fx, fy = x[np.isfinite(x)], y[np.isfinite(y)]
    keys = np.full(len(q), 1 << 32, dtype=np.int64)
    if not (len(fx) and len(fy) and fx.max() > fx.min() and fy.max() > fy.min()):
        return keys
    for m in range(len(q)):
        if np.isfinite(x[m]) and np.isfinite(y[m]):
            qx = int((x[m] - fx.min()) / (fx.max() - fx.min()) * 65535.0)
            qy = int((y[m] - fy.min()) / (fy.max() - fy.min()) * 65535.0)
            keys[m] = _spread16(qx) | (_spread16(qy) << 1)
    return keys


def _shuffled_family(name, n, M, seed):
    """(model type, points, models [M], threshold): the hypotheses of make_case, pushed along an ordered family (the probe point
    moves monotonically with the row), shuffled, one degenerate row among them"""
    mt, pts, base, thr = _case(name, n, M, seed)
    models = base.copy()
    t = np.linspace(0.0, 1.0, M)
    if mt == _lib.PNP:
        models[:, 3] += 1e-3 * t * np.abs(models[:, 11])
    elif mt == _lib.HOMOGRAPHY:
        models[:, 2] += 1e-3 * t * np.abs(models[:, 8])
    elif mt == _lib.CIRCLE2D:
        models[:, 2] += 1e-3 * t                      # (cx, cy, r): the radius
    else:
        models[:, 3] += 1e-3 * t
    models = models[np.random.default_rng(seed + M).permutation(M)]
    models[M // 3] = np.nan
    return mt, pts, np.ascontiguousarray(models), thr


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("name", ["pnp", "homography", "plane", "circle"])
def test_score_batch_sizes_across_the_reorder_and_the_padding(gpu_ctx, oracle, name, n):
    """capi.hip pgx_score_upload: a batch of more than 64 pose or homography hypotheses is reordered by locality key (the results come
    back in the caller's order through the device permutation, or through its host copy when the launch wrote the host mirror); Mpad
    rounds M up to 256 and the tail of the permutation is zero-filled.  M = 64 | 65 (reorder), 255 | 256 | 257 and 511 | 512 | 513
    (padding), 2049 (nine 256-blocks), with and without masks (without: the mirror), with and without the compound vector.  Planes (3-D)
    and circles (2-D) are never reordered and take the same sizes."""
    comp = np.random.default_rng(11).uniform(0, 1, n) * (np.random.default_rng(12).uniform(0, 1, n) < 0.5)
    resident = None
    for M in (64, 65, 255, 256, 257, 511, 512, 513, 2049):
        mt, pts, models, thr = _shuffled_family(name, n, M, seed=n)
        if resident is None:
            gpu_ctx.set_points(mt, pts)
            resident = pts
        assert np.array_equal(pts, resident)                     # (the points of make_case do not depend on M)
        keys = _locality_keys(mt, models)
        if keys is not None:
            assert (np.diff(keys) < 0).any(), "the batch is already in key order: the reorder would not permute"
        T2 = 2.25 * thr * thr
        for has_compound in (False, True):
            gpu_ctx.set_compound(comp if has_compound else None)
            ref = oracle.score(mt, pts, models, T2, compound=comp, has_compound=has_compound, want_masks=True)
            assert ref["counts"].max() > 0 and ref["counts"][M // 3] == 0
            for want_masks in (True, False):
                got = gpu_ctx.score(models, T2, has_compound=has_compound, want_masks=want_masks)
                _check_score(got, ref, masks=want_masks, what=f"{name} n = {n} M = {M} compound {has_compound} masks {want_masks}")
    gpu_ctx.set_compound(None)


@pytest.mark.parametrize("name,S", [("pnp", 33), ("homography", 100), ("plane", 100), ("circle", 100)])
def test_device_generated_batches_come_back_in_sample_order_after_a_reordered_upload(gpu_ctx, oracle, name, S):
    """pgx_solve_minimal / pgx_solve_minimal_sampled leave their hypotheses in sample order (identity permutation on the device).  After
    a REORDERED upload of another M on the same context, a stale host permutation or mirror would shuffle the rows of the fetch: the
    table must be the oracle's, row for row - with masks (copied from the device) and without (the host mirror)."""
    n = 130
    mt, pts, models, thr = _shuffled_family(name, n, 513, seed=n)
    m = {"pnp": 3}.get(name, 4 if name == "homography" else 3)
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(mt, pts)
    gpu_ctx.set_compound(None)
    samples = np.random.default_rng(S).integers(0, n, (S, m)).astype(np.int32)
    key, batch = 0x0123456789ABCDEF, 3
    drawn = oracle.sample_uniform(key, batch, 0, S, n, m)
    ref_up = oracle.score(mt, pts, models, T2, want_masks=True)
    for who, smp in (("solve_minimal", samples), ("solve_minimal_sampled", drawn)):
        ref_models = oracle.solve_minimal(mt, pts, smp)
        ref = oracle.score(mt, pts, ref_models, T2, want_masks=True)
        assert ref["counts"].max() > 0 and len(np.unique(ref["counts"])) > 2, "a shuffle of the rows would not show"
        for want_masks in (False, True):
            up = gpu_ctx.score(models, T2, want_masks=want_masks)                   # M = 513: reordered for poses and homographies
            assert np.array_equal(up["counts"], ref_up["counts"])
            with pytest.raises(_lib.PgxError, match="empty sample batch"):           # a refused call leaves the uploaded batch, and its order
                gpu_ctx.solve_minimal(np.zeros((0, m), np.int32))
            gpu_ctx.score_launch(T2, want_masks=want_masks)
            _check_score(gpu_ctx.score_fetch(want_masks=want_masks), ref_up, masks=want_masks, what=f"{name}: the uploaded batch after a refused {who}")
            if who == "solve_minimal":
                got_models = gpu_ctx.solve_minimal(smp)
            else:
                got_models, got_smp = gpu_ctx.solve_minimal_sampled(key, batch, S, fetch=True, fetch_samples=True)
                assert np.array_equal(got_smp, smp)
            assert np.array_equal(got_models, ref_models, equal_nan=True)
            gpu_ctx.score_launch(T2, want_masks=want_masks)
            got = gpu_ctx.score_fetch(want_masks=want_masks)
            _check_score(got, ref, masks=want_masks, what=f"{name} {who} masks {want_masks}")
            assert _same(got, gpu_ctx.score_fetch(want_masks=want_masks)), "a second fetch of the same launch differs"


# ----------------------------------------------------------------------------------------------------------------------
# A.4  small fixed limits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8192, 8193])
@pytest.mark.parametrize("L", [63, 64])
def test_bucket_at_the_label_limit(gpu_ctx, oracle, n, L):
    """pointwise.hip kMaxBucketLabels = 64: L = 63 and 64 are served, 65 is refused.  The order is n * 4 bytes of read-back:
    n = 8192: 32 768 (staged); n = 8193: 32 772 (direct)."""
    assert 8192 * 4 <= STAGE_MAX < 8193 * 4
    labels = np.random.default_rng(n + L).integers(0, L, n).astype(np.int32)
    labels[:L] = np.arange(L)                                   # every label present
    gpu_ctx.set_labels(labels)
    counts, order = gpu_ctx.bucket(L)
    rc, ro = oracle.bucket(labels, L)
    assert np.array_equal(counts, rc) and np.array_equal(order, ro) and (rc > 0).all()
    assert np.array_equal(gpu_ctx.bucket(L, want_order=False)[0], rc)
    with pytest.raises(_lib.PgxError, match="pgx_bucket"):
        gpu_ctx.bucket(65)
    assert np.array_equal(gpu_ctx.bucket(L)[1], ro)


def test_preference_slot_limit(gpu_ctx, oracle):
    """capi.hip slot_buffer: slots 0 .. 4096 exist; 4097 is refused, by pgx_preference and by pgx_get_preference."""
    n = 3001
    mt, pts, models, thr = _case("line", n, 3, 5)
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(mt, pts)
    ref = [oracle.preference(mt, pts, m, T2) for m in models]
    assert np.array_equal(gpu_ctx.preference(models[0], T2, slot=0, want_pref=True)["pref"], ref[0])
    assert np.array_equal(gpu_ctx.preference(models[1], T2, slot=4096, want_pref=True)["pref"], ref[1])
    with pytest.raises(_lib.PgxError, match="slot"):
        gpu_ctx.preference(models[2], T2, slot=4097)
    with pytest.raises(_lib.PgxError, match="slot"):
        gpu_ctx.get_preference(4097)
    with pytest.raises(_lib.PgxError, match="slot"):
        gpu_ctx.get_preference(4095)                            # inside the table, never written
    assert np.array_equal(gpu_ctx.get_preference(4096), ref[1]) and np.array_equal(gpu_ctx.get_preference(0), ref[0])
    assert np.array_equal(gpu_ctx.compound_update([4096, 0], want_compound=True), oracle.compound_max(np.stack([ref[1], ref[0]])))


def test_compound_update_at_the_chunk_limits(gpu_ctx, oracle):
    """pointwise.hip compound_launch: the kernel argument holds 32 slot pointers, more slots run as chunks that continue the maximum.
    K = 32 (one full chunk), 33 (a chunk of one behind it), 64 (two full chunks), 65."""
    n = 3001
    mt, pts, models, thr = _case("line", n, 65, 2)
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(mt, pts)
    prefs = np.stack([oracle.preference(mt, pts, m, T2) for m in models])
    for k in range(65):
        gpu_ctx.preference(models[k], T2, slot=k)
    order = np.random.default_rng(3).permutation(65)
    for K in (32, 33, 64, 65):
        slots = order[:K]
        ref = oracle.compound_max(prefs[slots])
        assert np.array_equal(gpu_ctx.compound_update(slots, want_compound=True), ref), K
    tail_only = np.zeros((33, n))
    tail_only[32] = prefs[0]                                     # the only non-zero vector sits in the second chunk
    far_line = np.array([1.0, 0.0, 1e9])                         # nowhere near the points: preference 0 everywhere
    assert not oracle.preference(mt, pts, far_line, T2).any() and prefs[0].any()
    for k in range(32):
        gpu_ctx.preference(far_line, T2, slot=100 + k)
    got = gpu_ctx.compound_update(list(range(100, 132)) + [0], want_compound=True)
    assert np.array_equal(got, oracle.compound_max(tail_only)) and got.any()


# ----------------------------------------------------------------------------------------------------------------------
# A.5  grid coarsening in the neighbourhood graph
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,k", [(_lib.GRAPH_BALL, 1), (_lib.GRAPH_KNN_IN_BALL, 5)])
def test_graph_grid_is_coarsened_beyond_the_cell_limit(gpu_ctx, oracle, kind, k):
    """graph.hip grid_pass: cells of size radius (1 + 1e-9) over the extent of the first two coordinates; while
    (floor(ext0 / cell) + 1) (floor(ext1 / cell) + 1) exceeds kMaxCells = 2^22 the cell grows by 1.5.  300 points in the unit square and
    two at (+-1e7, +-1e7) with radius 0.08: 2.5e8 cells a side uncoarsened, 30 coarsening steps, after which the unit square is one
    cell of two query slices - the lists must not notice."""
    rng = np.random.default_rng(5)
    pts = np.vstack([rng.random((300, 2)), [[1e7, 1e7], [-1e7, -1e7]]])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    radius = 0.08
    cell = radius * (1.0 + 1e-9)
    ext = pts.max(axis=0) - pts.min(axis=0)
    assert (np.floor(ext[0] / cell) + 1.0) * (np.floor(ext[1] / cell) + 1.0) > 2.0 ** 22 and (ext[0] / cell + 1.0) ** 2 > 2.0 ** 22
    ref = oracle.graph_build(pts, kind, radius=radius, k=k)
    assert len(ref[1]) > 300, "the graph has arcs to get wrong"
    got = gpu_ctx.graph_build(pts, kind, radius=radius, k=k)
    for name, a, b in zip(("off", "idx", "mult"), got, ref):
        assert np.array_equal(a, b), f"{name} differs"
    far = [int(i) for i in np.flatnonzero(np.abs(pts[:, 0]) > 2.0)]
    assert len(far) == 2 and all(got[0][i + 1] == got[0][i] for i in far)      # the two far points have no neighbours


# ----------------------------------------------------------------------------------------------------------------------
# B  state hand-overs on one context
# ----------------------------------------------------------------------------------------------------------------------
def _raw_gram_with_resident_weights(ctx, idx):
    """pgx_gram with use_weights = 1 through the C ABI (Context.gram would upload the weights it is handed)"""
    out = np.zeros(64)
    cnt, bad = C.c_int64(), C.c_int64()
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    rc = ctx._lib.pgx_gram(ctx._h, C.c_int(_lib.GRAM_AFFINE), None, C.c_int(0), C.c_int(0), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                           C.c_int64(len(idx)), C.c_int(0), C.c_int(1), C.c_int(2), out.ctypes.data_as(C.POINTER(C.c_double)),
                           C.byref(cnt), C.byref(bad))
    return rc, ctx._lib.pgx_last_error(ctx._h)


def test_state_hand_overs_on_one_context(gpu_ctx, oracle):
    """One script on the session's context: sizes walk up, down and up again over three model types, so that every resident buffer is
    grown, reused while larger than needed, and regrown.  Every step is compared with the oracle and, bitwise, with a FRESH context
    that performs only that step."""
    def both(mt, pts, step):
        """step(ctx) on the long-lived context and on a fresh one that has seen nothing but these points"""
        gpu_ctx.set_points(mt, pts)
        got = step(gpu_ctx)
        with _lib.Context(0) as fresh:
            fresh.set_points(mt, pts)
            alone = step(fresh)
        assert _same(got, alone), "the long-lived context and a fresh one disagree"
        return got

    # ---- 1: large, poses: M = 2049 with masks, gram_batch B = 92, gram_labels K = 92
    n1 = 20011
    mt1, pts1, models1, thr1 = _shuffled_family("pnp", n1, 2049, seed=7)
    rng = np.random.default_rng(1)
    index1 = np.array([rng.choice(n1, 14, replace=False) for _ in range(92)]).astype(np.int32)
    prm1 = np.ascontiguousarray(_case("pnp", n1, 2049, 7)[2][np.arange(92) % 3, :12])
    labels1 = _sparse_labels(rng, n1, 92, (0, 5, 91))

    def step1(ctx):
        ctx.set_labels(labels1)
        return (ctx.score(models1, 2.25 * thr1 * thr1, want_masks=True),
                ctx.gram_batch(_lib.GRAM_PNP_GN, index1, params=prm1),
                ctx.gram_labels(_lib.GRAM_PNP_GN, 92, params=prm1))
    sc, (Gb, badb), (Gl, cntl, badl) = both(mt1, pts1, step1)
    _check_score(sc, oracle.score(mt1, pts1, models1, 2.25 * thr1 * thr1, want_masks=True), what="step 1")
    for b in range(92):
        Gr, _, badr = oracle.gram(_lib.GRAM_PNP_GN, pts1, index1[b], params=prm1[b])
        assert int(badb[b]) == badr and _close(Gb[b], Gr), f"step 1 gram_batch row {b}"
    for k in range(92):
        sel = np.flatnonzero(labels1 == k)
        if len(sel):
            Gr, cntr, badr = oracle.gram(_lib.GRAM_PNP_GN, pts1, sel, params=prm1[k])
            assert (int(cntl[k]), int(badl[k])) == (cntr, badr) and _close(Gl[k], Gr), f"step 1 gram_labels label {k}"
        else:
            assert cntl[k] == 0 and not Gl[k].any()

    # ---- 2: tiny, another type: M = 3 without masks; the inlier rows of step 1 are gone; a 1-entry index list
    n2 = 65
    mt2, pts2, models2, thr2 = _case("line", n2, 3, 2)

    def step2(ctx):
        got = ctx.score(models2, 2.25 * thr2 * thr2)
        # include/pgx.h: "the last launch that produced masks"; a launch without masks (or new points) ends it - refused, never an old row
        with pytest.raises(_lib.PgxError, match="no masks"):
            ctx.score_inliers(0)
        return got, ctx.gram(_lib.GRAM_AFFINE, ("index", np.array([64], np.int32)))
    sc, (G, cnt, bad) = both(mt2, pts2, step2)
    _check_score(sc, oracle.score(mt2, pts2, models2, 2.25 * thr2 * thr2), masks=False, what="step 2")
    Gr, cntr, badr = oracle.gram(_lib.GRAM_AFFINE, pts2, np.array([64]))
    assert (cnt, bad) == (cntr, badr) == (1, 0) and _close(G, Gr)

    # ---- 3: large again, a third type: M = 513 with masks, the long index list
    n3 = 70001
    mt3, pts3, models3, thr3 = _shuffled_family("sphere", n3, 513, seed=13)
    perm3 = np.random.default_rng(3).permutation(n3).astype(np.int32)
    sph = np.array([5.1, 4.9, 5.3, 2.5])

    def step3(ctx):
        return (ctx.score(models3, 2.25 * thr3 * thr3, want_masks=True), ctx.score_inliers(512),
                ctx.gram(_lib.GRAM_SPHERE, ("index", perm3[:65537]), params=sph), ctx.gram(_lib.GRAM_SPHERE, ("index", perm3[:3]), params=sph))
    sc, inl, (G, cnt, bad), (Gs, cnts, bads) = both(mt3, pts3, step3)
    ref3 = oracle.score(mt3, pts3, models3, 2.25 * thr3 * thr3, want_masks=True)
    _check_score(sc, ref3, what="step 3")
    with np.errstate(invalid="ignore"):
        assert np.array_equal(inl, np.flatnonzero(oracle.squared_residuals(mt3, pts3, models3[512]) < 2.25 * thr3 * thr3))
    Gr, cntr, badr = oracle.gram(_lib.GRAM_SPHERE, pts3, perm3[:65537], params=sph)
    assert (cnt, bad) == (cntr, badr) and _close(G, Gr)
    Gr, cntr, badr = oracle.gram(_lib.GRAM_SPHERE, pts3, perm3[:3], params=sph)
    assert (cnts, bads) == (cntr, badr) and _close(Gs, Gr)

    # ---- 4: one launch, two fetches; with masks, then without: a mask fetch of the second launch is refused
    def step4(ctx):
        ctx.score_upload(models3)
        ctx.score_launch(2.25 * thr3 * thr3, want_masks=True)
        a = ctx.score_fetch(want_masks=True)
        b = ctx.score_fetch(want_masks=True)
        ctx.score_launch(2.25 * thr3 * thr3, want_masks=False)
        c = ctx.score_fetch()
        d = ctx.score_fetch()
        with pytest.raises(_lib.PgxError, match="masks were not requested"):
            ctx.score_fetch(want_masks=True)
        return a, b, c, d, ctx.score_fetch()
    a, b, c, d, e = both(mt3, pts3, step4)
    assert _same(a, b) and _same(c, d) and _same(c, e)
    _check_score(a, ref3, what="step 4 with masks")
    _check_score(c, ref3, masks=False, what="step 4 without masks")
    assert np.array_equal(a["values"], c["values"]) and np.array_equal(a["counts"], c["counts"])

    # ---- 5: set_points ends the earlier point set's weights, PROSAC table, labels, graph and global n
    n5, n6 = 3000, 2999
    mt5, pts5, _, _ = _case("plane", n5, 1, 5)
    mt6, pts6, models6, thr6 = _shuffled_family("pnp", n6, 257, seed=6)
    gpu_ctx.set_points(mt5, pts5)
    gpu_ctx.set_weights(np.full(n5, 3.0))
    gpu_ctx.sampler_prosac_set(np.full(400, n5, np.int32))
    gpu_ctx.set_labels(np.ones(n5, np.int32))
    gpu_ctx.graph_build(pts5, _lib.GRAPH_KNN, k=4, fetch=False)
    gpu_ctx.score_set_global_n(50_000_000)                                                # (set_points below is what has to end it)
    assert gpu_ctx.graph_size()[0] == n5
    G5 = gpu_ctx.gram(_lib.GRAM_AFFINE, ("label", 1))                                     # all of it in use before the hand-over
    assert G5[1] == n5 and _close(G5[0], oracle.gram(_lib.GRAM_AFFINE, pts5, np.arange(n5))[0])
    smp5 = gpu_ctx.solve_minimal_sampled(5, 1, 400, fetch=False, fetch_samples=True, sampler="prosac")[1]
    assert np.array_equal(smp5, oracle.sample_prosac(5, 1, 0, 400, n5, np.full(400, n5, np.int32), 3))
    assert gpu_ctx.solve_minimal_sampled(5, 1, 64, fetch=False, fetch_samples=True, sampler="napsac")[1].shape == (64, 3)

    def step5(ctx):
        rc, msg = _raw_gram_with_resident_weights(ctx, np.arange(10))                     # weights
        assert rc != 0 and b"no weights are resident" in msg
        with pytest.raises(_lib.PgxError, match="pgx_sampler_prosac_set"):               # PROSAC table
            ctx.solve_minimal_sampled(5, 1, 400, sampler="prosac")
        with pytest.raises(_lib.PgxError, match="labels not set"):                       # labels
            ctx.gram(_lib.GRAM_AFFINE, ("label", 1))
        with pytest.raises(_lib.PgxError, match="labels not set"):
            ctx.residual_sums(models6[:2])
        with pytest.raises(_lib.PgxError, match="graph"):                                # graph (n5 sites, n6 points)
            ctx.solve_minimal_sampled(5, 1, 64, sampler="napsac")
        with pytest.raises(_lib.PgxError, match="graph"):
            ctx.gc_labeling(models6[0], 2.25 * thr6 * thr6, 0.2)
        ctx.score_upload(models6)                                                        # global n: the fixed-point scale of the sums
        ctx.score_launch(2.25 * thr6 * thr6)
        return ctx.score_fetch(), ctx.score_accumulators()
    sc, acc = both(mt6, pts6, step5)
    _check_score(sc, oracle.score(mt6, pts6, models6, 2.25 * thr6 * thr6), masks=False, what="step 5")
    assert np.array_equal(acc["counts"].astype(np.int64), sc["counts"])
