"""Synthetic workloads of BASELINE.json (sizes/distributions: SURVEY.md §8d) and the reference's data-file format.

Everything is float64 and generated with numpy's PCG64 from an explicit seed, so the GPU box and this container build
identical inputs from the same numpy version.  Nothing here touches /root/reference at run time.
"""
import numpy as np

from . import _lib

TLESS_K = np.array([[1075.65087891, 0.0, 370.068878174],
                    [0.0, 1073.90344238, 278.721588135],
                    [0.0, 0.0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------------------------------------------------
def rodrigues(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def random_rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    return rodrigues(axis, rng.uniform(0, max_angle))


def normalize_pnp(x1y1, x2y2z2, K):
    """find6DPoses_ marshalling (progressivex_python.cpp:64-98): rows (u_n, v_n, X, Y, Z), threshold scale f."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kinv = np.linalg.inv(K)
    x = np.asarray(x1y1, dtype=np.float64)
    un = Kinv[0, 0] * x[:, 0] + Kinv[0, 1] * x[:, 1] + Kinv[0, 2]
    vn = Kinv[1, 0] * x[:, 0] + Kinv[1, 1] * x[:, 1] + Kinv[1, 2]
    pts = np.column_stack([un, vn, np.asarray(x2y2z2, dtype=np.float64)])
    f = 0.5 * (K[0, 0] + K[1, 1])
    return np.ascontiguousarray(pts), f


# ---------------------------------------------------------------------------------------------------------------------
# C1  2D multi-line
# ---------------------------------------------------------------------------------------------------------------------
def make_lines(n_per_line=500, n_lines=3, n_outliers=500, sigma=0.5, size=1000.0, seed=0):
    rng = np.random.default_rng(seed)
    pts, labels, models = [], [], []
    for k in range(n_lines):
        a, b = rng.uniform(0, size, 2), rng.uniform(0, size, 2)
        dirv = (b - a) / np.linalg.norm(b - a)
        nrm = np.array([-dirv[1], dirv[0]])
        t = rng.uniform(0, 1, n_per_line)[:, None]
        p = a + t * (b - a) + rng.normal(0, sigma, n_per_line)[:, None] * nrm
        pts.append(p)
        labels.append(np.full(n_per_line, k + 1))
        models.append(np.array([nrm[0], nrm[1], -nrm @ a]))
    pts.append(rng.uniform(0, size, (n_outliers, 2)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(models)


def make_planes(n_per_plane=8000, n_planes=6, n_outliers=48000, sigma=0.01, size=10.0, patch=4.0, seed=0):
    """findPlanes' workload: K planes with uniformly random unit normals through a patch centre drawn in the middle of the box
    [0, size]^3; the inliers of plane k lie on a square patch (side `patch`, random in-plane orientation) around the centre with
    Gaussian noise of `sigma` along the normal; the outliers are uniform in the box.  Returns (points [n, 3], labels [n]
    (k + 1 = plane k, 0 = outlier), gt_planes [K, 4] = (a, b, c, d) with (a, b, c) a unit normal)."""
    rng = np.random.default_rng(seed)
    pts, labels, models = [], [], []
    for k in range(n_planes):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        centre = rng.uniform(0.3 * size, 0.7 * size, 3)
        e1 = np.cross(nrm, rng.normal(size=3))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nrm, e1)
        st = rng.uniform(-0.5 * patch, 0.5 * patch, (n_per_plane, 2))
        p = centre + st[:, :1] * e1 + st[:, 1:] * e2 + rng.normal(0, sigma, n_per_plane)[:, None] * nrm
        pts.append(p)
        labels.append(np.full(n_per_plane, k + 1))
        models.append(np.array([nrm[0], nrm[1], nrm[2], -nrm @ centre]))
    pts.append(rng.uniform(0, size, (n_outliers, 3)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(models)


def make_lines3d(n_per_line=2000, n_lines=6, n_outliers=12000, sigma=0.01, size=10.0, length=(4.0, 10.0), seed=0):
    """findLines3D's workload: K segments with uniformly random unit directions and lengths uniform in `length`, each lying wholly
    inside the box [0, size]^3 (the midpoint is drawn where both ends fit); the inliers of line k are uniform along its segment with
    isotropic Gaussian noise of `sigma` per coordinate (their distance to the axis is Rayleigh, mean sigma sqrt(pi / 2)); the outliers
    are uniform in the box.  Returns (points [n, 3], labels [n] (k + 1 = line k, 0 = outlier), gt_lines [K, 6] = (midpoint, unit
    direction)).  A pure function of the seed."""
    rng = np.random.default_rng(seed)
    if not 0.0 < length[0] <= length[1] <= size:
        raise ValueError("length should satisfy 0 < min <= max <= size")
    pts, labels, models = [], [], []
    for k in range(n_lines):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        ln = rng.uniform(length[0], length[1])
        half = 0.5 * ln * np.abs(d)
        mid = rng.uniform(half, size - half)
        t = rng.uniform(-0.5 * ln, 0.5 * ln, n_per_line)
        pts.append(mid + t[:, None] * d + rng.normal(0, sigma, (n_per_line, 3)))
        labels.append(np.full(n_per_line, k + 1))
        models.append(np.concatenate([mid, d]))
    pts.append(rng.uniform(0, size, (n_outliers, 3)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(models).reshape(-1, 6)


def make_cylinders(n_per_cylinder=8000, n_cylinders=6, n_outliers=48000, sigma=0.01, size=10.0, radius=(0.3, 1.0), length=(3.0, 6.0),
                   coverage=1.0, normal_noise_deg=5.0, seed=0, normals="synthetic"):
    """findCylinders' workload: K cylinders with uniformly random unit axis directions, radii uniform in `radius` and lengths uniform in
    `length`, each lying wholly inside the box [0, size]^3 (the midpoint is drawn where both end discs fit; cylinders may cross); the
    inliers of cylinder k are uniform on its lateral surface - or, with coverage < 1, on the arc of that fraction of the circumference
    around a random direction (what one scan sees of a pipe) - with Gaussian noise of `sigma` along the radius; their normals are the
    radial unit vectors tilted by an angle uniform in [0, normal_noise_deg] about a random axis orthogonal to them, each with a random
    sign.  The outliers are uniform in the box with uniformly random unit normals.  Returns (points [n, 3], normals [n, 3] (unit),
    labels [n] (k + 1 = cylinder k, 0 = outlier), gt_cylinders [K, 7] = (midpoint of the axis segment, unit direction, radius)).
    A pure function of the seed.  normals="estimated" returns, in place of those synthetic normals, what estimateNormals(points) computes
    from the same points (k = 16 nearest neighbours, unsigned; needs the GPU): the normals a scan of the scene would come with."""
    if normals not in ("synthetic", "estimated"):
        raise ValueError('normals should be "synthetic" or "estimated"')
    rng = np.random.default_rng(seed)
    if not 0.0 < coverage <= 1.0:
        raise ValueError("coverage should lie in (0, 1]")
    if not (0.0 < length[0] <= length[1] and 0.0 < radius[0] <= radius[1] and length[1] + 2.0 * radius[1] <= size):
        raise ValueError("length and radius should satisfy 0 < min <= max and max length + 2 max radius <= size")
    pts, nrm, labels, models = [], [], [], []
    for k in range(n_cylinders):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        r = rng.uniform(radius[0], radius[1])
        ln = rng.uniform(length[0], length[1])
        half = 0.5 * ln * np.abs(d) + r
        mid = rng.uniform(half, size - half)
        e1 = np.cross(d, rng.normal(size=3))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(d, e1)
        t = rng.uniform(-0.5 * ln, 0.5 * ln, n_per_cylinder)
        phi = rng.uniform(-np.pi * coverage, np.pi * coverage, n_per_cylinder)
        rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
        pts.append(mid + t[:, None] * d + rad * (r + rng.normal(0, sigma, n_per_cylinder))[:, None])
        # tilt: rotate rad by `ang` towards a random unit vector orthogonal to it (psi picks it in the tangent plane spanned by d, d x rad)
        ang = np.deg2rad(rng.uniform(0.0, normal_noise_deg, n_per_cylinder))
        psi = rng.uniform(0.0, 2.0 * np.pi, n_per_cylinder)
        tang = np.cos(psi)[:, None] * d + np.sin(psi)[:, None] * np.cross(d, rad)
        nk = np.cos(ang)[:, None] * rad + np.sin(ang)[:, None] * tang
        nrm.append(nk * rng.choice([-1.0, 1.0], n_per_cylinder)[:, None])
        labels.append(np.full(n_per_cylinder, k + 1))
        models.append(np.concatenate([mid, d, [r]]))
    pts.append(rng.uniform(0, size, (n_outliers, 3)))
    no = rng.normal(size=(n_outliers, 3))
    nrm.append(no / np.linalg.norm(no, axis=1)[:, None])
    labels.append(np.zeros(n_outliers, dtype=int))
    pts, nrm = np.ascontiguousarray(np.vstack(pts)), np.ascontiguousarray(np.vstack(nrm))
    if normals == "estimated":
        from ._api import estimateNormals
        nrm = estimateNormals(pts)
    return pts, nrm, np.concatenate(labels).astype(np.int32), np.array(models).reshape(-1, 7)


def make_cones(n_per_cone=8000, n_cones=6, n_outliers=48000, sigma=0.01, size=10.0, half_angle_deg=(15.0, 40.0), extent=(1.0, 4.0),
               normal_noise_deg=5.0, seed=0, normals="synthetic"):
    """findCones' workload: K cones with uniformly random unit axis directions and half-angles uniform in `half_angle_deg` (degrees),
    each cut to the axial extent [hmin, hmax] = `extent` measured from the apex along the axis and lying wholly inside the box
    [0, size]^3 (the apex is drawn where the piece up to hmax fits; cones may cross); the inliers of cone k are uniform on that piece
    of its lateral surface (the height is the root of a uniform draw between hmin^2 and hmax^2: the circumference grows with the
    height) with Gaussian noise of `sigma` along the surface normal cos(theta) rhohat - sin(theta) d; their normals are those unit
    surface normals tilted by an angle uniform in [0, normal_noise_deg] about a random axis orthogonal to them, each with a random
    sign.  The outliers are uniform in the box with uniformly random unit normals.  Returns (points [n, 3], normals [n, 3] (unit),
    labels [n] (k + 1 = cone k, 0 = outlier), gt_cones [K, 8] = (apex, unit direction into the nappe, cos(theta), sin(theta))).
    A pure function of the seed.  normals="estimated" returns, in place of those synthetic normals, what estimateNormals(points) computes
    from the same points (k = 16 nearest neighbours, unsigned; needs the GPU)."""
    if normals not in ("synthetic", "estimated"):
        raise ValueError('normals should be "synthetic" or "estimated"')
    rng = np.random.default_rng(seed)
    amin, amax = (float(v) for v in half_angle_deg)
    hmin, hmax = (float(v) for v in extent)
    if not (0.0 < amin <= amax < 90.0 and 0.0 <= hmin < hmax):
        raise ValueError("half_angle_deg and extent should satisfy 0 < min <= max < 90 and 0 <= hmin < hmax")
    tmax = np.deg2rad(amax)
    if not max(hmax / np.cos(tmax), 2.0 * hmax * np.tan(tmax)) <= size:
        raise ValueError("the largest cone, hmax / cos(max angle) long and 2 hmax tan(max angle) wide, should fit the box")
    pts, nrm, labels, models = [], [], [], []
    for k in range(n_cones):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        theta = np.deg2rad(rng.uniform(amin, amax))
        c, s = np.cos(theta), np.sin(theta)
        side = hmax * np.tan(theta) * np.sqrt(np.maximum(0.0, 1.0 - d * d))
        lo, hi = np.minimum(0.0, hmax * d - side), np.maximum(0.0, hmax * d + side)
        apex = rng.uniform(-lo, size - hi)
        e1 = np.cross(d, rng.normal(size=3))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(d, e1)
        h = np.sqrt(rng.uniform(hmin * hmin, hmax * hmax, n_per_cone))
        phi = rng.uniform(-np.pi, np.pi, n_per_cone)
        rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
        nk0 = c * rad - s * d
        pts.append(apex + h[:, None] * d + (h * (s / c))[:, None] * rad + nk0 * rng.normal(0, sigma, n_per_cone)[:, None])
        # tilt: rotate the normal by `ang` towards a random unit vector of its tangent plane, spanned by the generatrix and d x rad
        ang = np.deg2rad(rng.uniform(0.0, normal_noise_deg, n_per_cone))
        psi = rng.uniform(0.0, 2.0 * np.pi, n_per_cone)
        tang = np.cos(psi)[:, None] * (c * d + s * rad) + np.sin(psi)[:, None] * np.cross(d, rad)
        nk = np.cos(ang)[:, None] * nk0 + np.sin(ang)[:, None] * tang
        nrm.append(nk * rng.choice([-1.0, 1.0], n_per_cone)[:, None])
        labels.append(np.full(n_per_cone, k + 1))
        models.append(np.concatenate([apex, d, [c, s]]))
    pts.append(rng.uniform(0, size, (n_outliers, 3)))
    no = rng.normal(size=(n_outliers, 3))
    nrm.append(no / np.linalg.norm(no, axis=1)[:, None])
    labels.append(np.zeros(n_outliers, dtype=int))
    pts, nrm = np.ascontiguousarray(np.vstack(pts)), np.ascontiguousarray(np.vstack(nrm))
    if normals == "estimated":
        from ._api import estimateNormals
        nrm = estimateNormals(pts)
    return pts, nrm, np.concatenate(labels).astype(np.int32), np.array(models).reshape(-1, 8)


def make_primitives(n_per=8000, n_outliers=32000, seed=0, n_each=1, sigma=0.01, size=10.0, normal_noise_deg=5.0, normals="synthetic"):
    """findPrimitives' workload: `n_each` planes, spheres, cylinders and cones in one box [0, size]^3, `n_per` points on each, and
    `n_outliers` uniform points.  The instances and their inliers are those of make_planes, make_spheres, make_cylinders and make_cones
    with their default shapes, each called for its class alone (no outliers) under its own seed derived from `seed`, so every class keeps
    its generator's conventions and its noise of `sigma` along the surface normal; instances of different classes may cross.  The
    normals: the cylinders' and cones' are their generators' tilted ones; the planes' and spheres' are the true unit normals (the plane's
    normal, the sphere's radial direction) tilted the same way - by an angle uniform in [0, normal_noise_deg] towards a random unit
    vector orthogonal to them, each with a random sign; the outliers' are uniformly random unit vectors.  Returns (points [n, 3],
    normals [n, 3] (unit), gt_class [n] (the class number 6 / 8 / 14 / 16 of the point's instance, 0 = outlier), gt_instance [n]
    (k + 1 = row k of gt_models, 0 = outlier), gt_models [4 n_each, 9] = (class, the generator's model row padded with zeros), planes
    first, then spheres, cylinders, cones).  A pure function of the seed.  normals="estimated" returns, in place of the synthetic
    normals, what estimateNormals(points) computes from the same points (k = 16 nearest neighbours, unsigned; needs the GPU)."""
    if normals not in ("synthetic", "estimated"):
        raise ValueError('normals should be "synthetic" or "estimated"')
    if n_each < 1 or n_per < 1 or n_outliers < 0:
        raise ValueError("n_each and n_per should be at least 1, n_outliers at least 0")
    seeds = [int(v) for v in np.random.SeedSequence(int(seed)).generate_state(5)]
    rng = np.random.default_rng(seeds[4])

    def tilted(nk0):
        t = np.cross(nk0, rng.normal(size=nk0.shape))
        t /= np.linalg.norm(t, axis=1)[:, None]
        ang = np.deg2rad(rng.uniform(0.0, normal_noise_deg, len(nk0)))
        nk = np.cos(ang)[:, None] * nk0 + np.sin(ang)[:, None] * t
        return nk * rng.choice([-1.0, 1.0], len(nk0))[:, None]

    p_pl, l_pl, g_pl = make_planes(n_per_plane=n_per, n_planes=n_each, n_outliers=0, sigma=sigma, size=size, seed=seeds[0])
    p_sp, l_sp, g_sp = make_spheres(n_per_sphere=n_per, n_spheres=n_each, n_outliers=0, sigma=sigma, size=size, seed=seeds[1])
    p_cy, n_cy, l_cy, g_cy = make_cylinders(n_per_cylinder=n_per, n_cylinders=n_each, n_outliers=0, sigma=sigma, size=size,
                                            normal_noise_deg=normal_noise_deg, seed=seeds[2])
    p_co, n_co, l_co, g_co = make_cones(n_per_cone=n_per, n_cones=n_each, n_outliers=0, sigma=sigma, size=size,
                                        normal_noise_deg=normal_noise_deg, seed=seeds[3])
    n_pl = tilted(g_pl[l_pl - 1, :3])
    radial = p_sp - g_sp[l_sp - 1, :3]
    n_sp = tilted(radial / np.linalg.norm(radial, axis=1)[:, None])
    out_p = rng.uniform(0, size, (n_outliers, 3))
    out_n = rng.normal(size=(n_outliers, 3))
    out_n /= np.linalg.norm(out_n, axis=1)[:, None]
    pts = np.ascontiguousarray(np.vstack([p_pl, p_sp, p_cy, p_co, out_p]))
    nrm = np.ascontiguousarray(np.vstack([n_pl, n_sp, n_cy, n_co, out_n]))
    parts = ((_lib.PLANE3D, l_pl, g_pl), (_lib.SPHERE3D, l_sp, g_sp), (_lib.CYLINDER3D, l_cy, g_cy), (_lib.CONE3D, l_co, g_co))
    gt = np.zeros((4 * n_each, 9))
    cls, inst = [], []
    for j, (c, lab, g) in enumerate(parts):
        gt[j * n_each:(j + 1) * n_each, 0] = c
        gt[j * n_each:(j + 1) * n_each, 1:1 + g.shape[1]] = g
        cls.append(np.full(len(lab), c))
        inst.append(lab + j * n_each)
    cls.append(np.zeros(n_outliers, dtype=int))
    inst.append(np.zeros(n_outliers, dtype=int))
    if normals == "estimated":
        from ._api import estimateNormals
        nrm = estimateNormals(pts)
    return pts, nrm, np.concatenate(cls).astype(np.int32), np.concatenate(inst).astype(np.int32), gt


def make_tori(n_per_torus=8000, n_tori=6, n_outliers=48000, sigma=0.01, size=10.0, major_radius=(0.8, 2.0), minor_radius=(0.2, 0.5),
              normal_noise_deg=5.0, seed=0, normals="synthetic"):
    """findTori's workload: K ring tori with uniformly random unit axis directions, major radii R uniform in `major_radius` and minor
    (tube) radii r uniform in `minor_radius` (max r < min R), each lying wholly inside the box [0, size]^3 (tori may cross); the
    inliers of torus k are uniform on its surface - the angle phi about the axis is uniform and the tube angle theta is drawn with
    density proportional to R + r cos(theta), the circumference at that angle, by rejection - with Gaussian noise of `sigma` along the
    surface normal cos(theta) rhohat + sin(theta) d; their normals are those unit surface normals tilted by an angle uniform in
    [0, normal_noise_deg] about a random axis orthogonal to them, each with a random sign.  The outliers are uniform in the box with
    uniformly random unit normals.  Returns (points [n, 3], normals [n, 3] (unit), labels [n] (k + 1 = torus k, 0 = outlier),
    gt_tori [K, 8] = (centre, unit axis direction, R, r)).  A pure function of the seed.  normals="estimated" returns, in place of
    those synthetic normals, what estimateNormals(points) computes from the same points (k = 16 nearest neighbours, unsigned; needs
    the GPU)."""
    if normals not in ("synthetic", "estimated"):
        raise ValueError('normals should be "synthetic" or "estimated"')
    rng = np.random.default_rng(seed)
    Rlo, Rhi = (float(v) for v in major_radius)
    rlo, rhi = (float(v) for v in minor_radius)
    if not (0.0 < rlo <= rhi < Rlo <= Rhi):
        raise ValueError("major_radius and minor_radius should satisfy 0 < rmin <= rmax < Rmin <= Rmax")
    if not 2.0 * (Rhi + rhi) <= size:
        raise ValueError("the largest torus, 2 (Rmax + rmax) wide, should fit the box")
    pts, nrm, labels, models = [], [], [], []
    for k in range(n_tori):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        R, r = rng.uniform(Rlo, Rhi), rng.uniform(rlo, rhi)
        half = R * np.sqrt(np.maximum(0.0, 1.0 - d * d)) + r
        centre = rng.uniform(half, size - half)
        e1 = np.cross(d, rng.normal(size=3))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(d, e1)
        theta = np.empty(0)
        while theta.size < n_per_torus:
            cand = rng.uniform(-np.pi, np.pi, n_per_torus)
            theta = np.concatenate([theta, cand[rng.uniform(0.0, R + r, n_per_torus) < R + r * np.cos(cand)]])
        theta = theta[:n_per_torus]
        phi = rng.uniform(-np.pi, np.pi, n_per_torus)
        rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
        ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
        nk0 = ct * rad + st * d
        pts.append(centre + (R + r * ct) * rad + (r * st) * d + nk0 * rng.normal(0, sigma, n_per_torus)[:, None])
        # tilt: rotate the normal by `ang` towards a random unit vector of its tangent plane, spanned by the tube's tangent and d x rad
        ang = np.deg2rad(rng.uniform(0.0, normal_noise_deg, n_per_torus))
        psi = rng.uniform(0.0, 2.0 * np.pi, n_per_torus)
        tang = np.cos(psi)[:, None] * (ct * d - st * rad) + np.sin(psi)[:, None] * np.cross(d, rad)
        nk = np.cos(ang)[:, None] * nk0 + np.sin(ang)[:, None] * tang
        nrm.append(nk * rng.choice([-1.0, 1.0], n_per_torus)[:, None])
        labels.append(np.full(n_per_torus, k + 1))
        models.append(np.concatenate([centre, d, [R, r]]))
    pts.append(rng.uniform(0, size, (n_outliers, 3)))
    no = rng.normal(size=(n_outliers, 3))
    nrm.append(no / np.linalg.norm(no, axis=1)[:, None])
    labels.append(np.zeros(n_outliers, dtype=int))
    pts, nrm = np.ascontiguousarray(np.vstack(pts)), np.ascontiguousarray(np.vstack(nrm))
    if normals == "estimated":
        from ._api import estimateNormals
        nrm = estimateNormals(pts)
    return pts, nrm, np.concatenate(labels).astype(np.int32), np.array(models).reshape(-1, 8)


def make_spheres(n_per_sphere=8000, n_spheres=6, n_outliers=48000, sigma=0.01, size=10.0, radius=(0.3, 1.5), coverage=1.0, seed=0):
    """findSpheres' workload: K non-overlapping spheres with radii uniform in `radius` and centres inside the box [0, size]^3 (each
    sphere lies wholly inside it); the inliers of sphere k are uniform on its surface - or, with coverage < 1, on the cap of that
    fraction of the surface facing a random direction (what one depth scan sees of a ball) - with Gaussian noise of `sigma` along
    the radius; the outliers are uniform in the box.  Returns (points [n, 3], labels [n] (k + 1 = sphere k, 0 = outlier),
    gt_spheres [K, 4] = (cx, cy, cz, r))."""
    rng = np.random.default_rng(seed)
    if not 0.0 < coverage <= 1.0:
        raise ValueError("coverage should lie in (0, 1]")
    spheres = []
    for _ in range(100000):
        if len(spheres) == n_spheres:
            break
        r = rng.uniform(radius[0], radius[1])
        c = rng.uniform(r, size - r, 3)
        if all(np.linalg.norm(c - g[:3]) > r + g[3] for g in spheres):
            spheres.append(np.array([c[0], c[1], c[2], r]))
    if len(spheres) < n_spheres:
        raise ValueError("cannot place that many non-overlapping spheres in the box")
    pts, labels = [], []
    for k, g in enumerate(spheres):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        # uniform on the cap {d : d . axis >= 1 - 2 coverage} (area fraction = coverage): the height d . axis is uniform
        t = rng.uniform(1.0 - 2.0 * coverage, 1.0, n_per_sphere)
        phi = rng.uniform(0.0, 2.0 * np.pi, n_per_sphere)
        e1 = np.cross(axis, rng.normal(size=3))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(axis, e1)
        rho = np.sqrt(np.maximum(0.0, 1.0 - t * t))
        d = t[:, None] * axis + (rho * np.cos(phi))[:, None] * e1 + (rho * np.sin(phi))[:, None] * e2
        pts.append(g[:3] + d * (g[3] + rng.normal(0, sigma, n_per_sphere))[:, None])
        labels.append(np.full(n_per_sphere, k + 1))
    pts.append(rng.uniform(0, size, (n_outliers, 3)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(spheres).reshape(-1, 4)


def make_circles(n_per_circle=2000, n_circles=4, n_outliers=8000, sigma=0.5, size=1000.0, radius=(40.0, 150.0), coverage=1.0, seed=0):
    """findCircles' workload (make_spheres in 2-D, pixel scale): K non-overlapping circles with radii uniform in `radius` and centres
    inside the box [0, size]^2 (each circle lies wholly inside it); the inliers of circle k are uniform on it - or, with coverage < 1,
    on the arc of that fraction of the circumference around a random direction - with Gaussian noise of `sigma` along the radius;
    the outliers are uniform in the box.  Returns (points [n, 2], labels [n] (k + 1 = circle k, 0 = outlier),
    gt_circles [K, 3] = (cx, cy, r))."""
    rng = np.random.default_rng(seed)
    if not 0.0 < coverage <= 1.0:
        raise ValueError("coverage should lie in (0, 1]")
    circles = []
    for _ in range(100000):
        if len(circles) == n_circles:
            break
        r = rng.uniform(radius[0], radius[1])
        c = rng.uniform(r, size - r, 2)
        if all(np.linalg.norm(c - g[:2]) > r + g[2] for g in circles):
            circles.append(np.array([c[0], c[1], r]))
    if len(circles) < n_circles:
        raise ValueError("cannot place that many non-overlapping circles in the box")
    pts, labels = [], []
    for k, g in enumerate(circles):
        mid = rng.uniform(0.0, 2.0 * np.pi)
        phi = mid + rng.uniform(-np.pi * coverage, np.pi * coverage, n_per_circle)
        d = np.column_stack([np.cos(phi), np.sin(phi)])
        pts.append(g[:2] + d * (g[2] + rng.normal(0, sigma, n_per_circle))[:, None])
        labels.append(np.full(n_per_circle, k + 1))
    pts.append(rng.uniform(0, size, (n_outliers, 2)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(circles).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# C2  multi-homography
# ---------------------------------------------------------------------------------------------------------------------
def make_homographies(n_per_plane=600, n_planes=5, n_outliers=2000, sigma=0.5, size=1000.0, seed=0):
    rng = np.random.default_rng(seed)
    pts, labels, models = [], [], []
    for k in range(n_planes):
        H = np.eye(3)
        H[:2, :2] += rng.uniform(-0.2, 0.2, (2, 2))
        H[:2, 2] = rng.uniform(-50, 50, 2)
        H[2, :2] = rng.uniform(-1e-4, 1e-4, 2)
        c = rng.uniform(0.2 * size, 0.8 * size, 2)
        x = c + rng.uniform(-0.15 * size, 0.15 * size, (n_per_plane, 2))
        xh = np.column_stack([x, np.ones(n_per_plane)]) @ H.T
        y = xh[:, :2] / xh[:, 2:3] + rng.normal(0, sigma, (n_per_plane, 2))
        pts.append(np.column_stack([x, y]))
        labels.append(np.full(n_per_plane, k + 1))
        models.append(H.reshape(-1))
    pts.append(rng.uniform(0, size, (n_outliers, 4)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(models)


# ---------------------------------------------------------------------------------------------------------------------
# C3  multi two-view motion
# ---------------------------------------------------------------------------------------------------------------------
def make_two_view_motions(n_per_motion=10000, n_motions=8, n_outliers=20000, sigma=0.5, f=800.0, size=1000.0, seed=0):
    rng = np.random.default_rng(seed)
    K = np.array([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1.0]])
    Kinv = np.linalg.inv(K)
    pts, labels, models = [], [], []
    for k in range(n_motions):
        R = random_rotation(rng, np.deg2rad(15))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        center = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(4, 8)])
        X = center + rng.uniform(-0.7, 0.7, (n_per_motion, 3))
        x1 = X @ K.T
        x1 = x1[:, :2] / x1[:, 2:3]
        X2 = X @ R.T + t
        x2 = X2 @ K.T
        x2 = x2[:, :2] / x2[:, 2:3] + rng.normal(0, sigma, (n_per_motion, 2))
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        F = Kinv.T @ tx @ R @ Kinv
        F /= np.linalg.norm(F)
        pts.append(np.column_stack([x1, x2]))
        labels.append(np.full(n_per_motion, k + 1))
        models.append(F.reshape(-1))
    pts.append(rng.uniform(0, size, (n_outliers, 4)))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(pts)), np.concatenate(labels).astype(np.int32), np.array(models)


# ---------------------------------------------------------------------------------------------------------------------
# C4  multi 6D pose + the metric batch of 2048 hypotheses
# ---------------------------------------------------------------------------------------------------------------------
def make_poses(n_per_object=50000, n_objects=16, n_outliers=200000, sigma=1.0, seed=0, K=TLESS_K):
    """Returns raw inputs of find6DPoses (pixels, mm) + ground truth poses [n_objects, 12] and labels (0 = outlier)."""
    rng = np.random.default_rng(seed)
    x1, x2, labels, poses = [], [], [], []
    for k in range(n_objects):
        R = random_rotation(rng)
        tz = rng.uniform(600, 900)
        # object centre projects inside the 720 x 540 image
        cu, cv = rng.uniform(100, 620), rng.uniform(80, 460)
        t = np.array([(cu - K[0, 2]) / K[0, 0] * tz, (cv - K[1, 2]) / K[1, 1] * tz, tz])
        X = rng.normal(size=(n_per_object, 3))
        X = X / np.linalg.norm(X, axis=1, keepdims=True) * (50.0 * rng.uniform(0, 1, (n_per_object, 1)) ** (1 / 3))
        Xc = X @ R.T + t
        uv = Xc @ K.T
        uv = uv[:, :2] / uv[:, 2:3] + rng.normal(0, sigma, (n_per_object, 2))
        x1.append(uv)
        x2.append(X)
        labels.append(np.full(n_per_object, k + 1))
        poses.append(np.column_stack([R, t]).reshape(-1))
    x1.append(np.column_stack([rng.uniform(0, 720, n_outliers), rng.uniform(0, 540, n_outliers)]))
    Xo = rng.normal(size=(n_outliers, 3))
    Xo = Xo / np.linalg.norm(Xo, axis=1, keepdims=True) * (50.0 * rng.uniform(0, 1, (n_outliers, 1)) ** (1 / 3))
    x2.append(Xo)
    labels.append(np.zeros(n_outliers, dtype=int))
    return (np.ascontiguousarray(np.vstack(x1)), np.ascontiguousarray(np.vstack(x2)), np.array(K, dtype=np.float64),
            np.concatenate(labels).astype(np.int32), np.array(poses))


def make_pose_hypotheses(gt_poses, M=2048, max_angle_deg=30.0, max_shift_mm=100.0, seed=1):
    """Metric batch: the GT poses followed by poses perturbed by U(0,max_angle) / U(0,max_shift)."""
    rng = np.random.default_rng(seed)
    gt = np.asarray(gt_poses, dtype=np.float64).reshape(-1, 3, 4)
    out = [p.reshape(-1) for p in gt[:M]]
    while len(out) < M:
        P = gt[rng.integers(0, gt.shape[0])]
        dR = rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(0, max_angle_deg)))
        dt = rng.normal(size=3)
        dt = dt / np.linalg.norm(dt) * rng.uniform(0, max_shift_mm)
        out.append(np.column_stack([dR @ P[:, :3], P[:, 3] + dt]).reshape(-1))
    return np.ascontiguousarray(np.array(out[:M]))


# ---------------------------------------------------------------------------------------------------------------------
# C5  multi vanishing point
# ---------------------------------------------------------------------------------------------------------------------
def make_vanishing_points(n_inliers=100000, n_vps=6, n_outliers=100000, sigma_deg=0.5, size=1000.0, seed=0):
    rng = np.random.default_rng(seed)
    vps = []
    for k in range(n_vps):
        if k < n_vps // 2:  # finite, within +-3000 px
            v = np.array([rng.uniform(-3000, 3000), rng.uniform(-3000, 3000), 1.0])
        else:  # near-infinite
            ang = rng.uniform(0, np.pi)
            v = np.array([np.cos(ang), np.sin(ang), rng.uniform(-1e-6, 1e-6)])
        vps.append(v / np.linalg.norm(v))
    segs, labels = [], []
    per = n_inliers // n_vps
    for k, v in enumerate(vps):
        m = rng.uniform(0, size, (per, 2))
        # direction from the midpoint towards the vanishing point (homogeneous: v_xy - v_z * m)
        dirv = v[:2] - v[2] * m
        ang = np.arctan2(dirv[:, 1], dirv[:, 0]) + np.deg2rad(rng.normal(0, sigma_deg, per))
        half = rng.uniform(20, 120, per)[:, None] / 2
        dvec = np.column_stack([np.cos(ang), np.sin(ang)])
        segs.append(np.column_stack([m - half * dvec, m + half * dvec]))
        labels.append(np.full(per, k + 1))
    m = rng.uniform(0, size, (n_outliers, 2))
    ang = rng.uniform(0, np.pi, n_outliers)
    half = rng.uniform(20, 120, n_outliers)[:, None] / 2
    dvec = np.column_stack([np.cos(ang), np.sin(ang)])
    segs.append(np.column_stack([m - half * dvec, m + half * dvec]))
    labels.append(np.zeros(n_outliers, dtype=int))
    return np.ascontiguousarray(np.vstack(segs)), np.concatenate(labels).astype(np.int32), np.array(vps)


# ---------------------------------------------------------------------------------------------------------------------
# reference data-file format (progx_utils.h:32-96 / dataset_comparison/utils.py:15-27)
# ---------------------------------------------------------------------------------------------------------------------
def load_points_with_labels(path):
    """7-column AdelaideRMF text file `x1 y1 1 x2 y2 1 label` -> (corrs[n,4], labels[n]); label 0 = outlier."""
    M = np.loadtxt(path)
    corrs = np.ascontiguousarray(np.concatenate((M[:, :2], M[:, 3:5]), axis=1))
    return corrs, M[:, -1].astype(np.int32)


def misclassification(segmentation, ref_segmentation):
    """dataset_comparison/utils.py:51-66 — min over label permutations of the fraction of disagreeing points.

    Implemented with the Hungarian algorithm on the confusion matrix, which gives the same minimum as enumerating the
    permutations of the reference ids but scales past 8 labels."""
    from scipy.optimize import linear_sum_assignment
    seg = np.asarray(segmentation).astype(np.int64)
    ref = np.asarray(ref_segmentation).astype(np.int64)
    n = int(ref.max()) + 1
    conf = np.zeros((n, n), dtype=np.int64)  # the reference only permutes ids 0..n-1; other predicted ids never match
    ok = seg < n
    np.add.at(conf, (ref[ok], seg[ok]), 1)
    r, c = linear_sum_assignment(-conf)
    return 1.0 - conf[r, c].sum() / len(seg)


def misclassification_labeling(labeling, annotation, K, K_annot):
    """progx_utils.h:201-274, the (labeling, annotation) overload of getMisclassificationError, restated literally:
    predicted label l means cluster l + 1 (labels with l + 1 > K are left unassigned, -1 = outlier stays 0), every
    ground-truth cluster 1..K_annot greedily takes the unused predicted cluster with the largest overlap (first maximum
    wins; the first candidate is always taken because the reference compares an int -1 with a size_t), matched points
    take the annotation's id, the error is the PERCENTAGE of points whose ids still differ."""
    lab = np.asarray(labeling).astype(np.int64)
    ann = np.asarray(annotation).astype(np.int64)
    all1 = np.full(lab.shape[0], -1, dtype=np.int64)
    ok = lab + 1 <= K
    all1[ok] = lab[ok] + 1
    used = np.zeros(K + 1, dtype=bool)
    pair = {0: 0}
    for i in range(1, K_annot + 1):
        best, best_size = -1, -1
        for j in range(1, K + 1):
            if used[j]:
                continue
            size = int(np.count_nonzero((all1 == j) & (ann == i)))
            if best == -1 or best_size < size:
                best, best_size = j, size
        if best == -1:
            continue
        used[best] = True
        pair[i] = best
    gt_pair = np.array([pair.get(int(a), 0) for a in ann], dtype=np.int64)
    hit = (lab != -1) & (all1 == gt_pair)
    all1 = np.where(hit, ann, all1)
    return 100.0 * float(np.count_nonzero(all1 != ann)) / lab.shape[0]


def misclassification_models(preferences, annotation, K_annot):
    """progx_utils.h:98-199, the (models, annotation) overload: a point is claimed by the FIRST model whose preference
    exceeds FLT_EPSILON; over all permutations of the model ids the smallest number of points whose claimed id differs
    from the annotation (unclaimed points are right iff the annotation is 0), as a PERCENTAGE.  The permutation loop is an
    assignment problem and is solved as one; -1 for more than 9 models, as in the reference."""
    from scipy.optimize import linear_sum_assignment
    pref = np.asarray(preferences, dtype=np.float64)
    ann = np.asarray(annotation).astype(np.int64)
    K = pref.shape[0]
    if K > 9:
        return -1.0
    claimed = pref > np.finfo(np.float32).eps
    owner = np.where(claimed.any(axis=0), np.argmax(claimed, axis=0), -1)      # first model with preference 1
    mk = max(K, K_annot)
    gain = np.zeros((mk, mk), dtype=np.int64)                                   # gain[m, id-1] = points of m annotated id
    for m in range(K):
        ids, cnt = np.unique(ann[owner == m], return_counts=True)
        for a, c in zip(ids, cnt):
            if 1 <= a <= mk:
                gain[m, a - 1] += c
    r, c = linear_sum_assignment(-gain)
    right = int(gain[r, c].sum()) + int(np.count_nonzero((owner == -1) & (ann == 0)))
    return 100.0 * float(ann.shape[0] - right) / ann.shape[0]


MODEL_TYPES = dict(line=_lib.LINE2D, homography=_lib.HOMOGRAPHY, fundamental=_lib.FUNDAMENTAL, pnp=_lib.PNP,
                   vanishing_point=_lib.VANISHING_POINT, plane=_lib.PLANE3D, sphere=_lib.SPHERE3D, circle=_lib.CIRCLE2D,
                   line3d=_lib.LINE3D, cylinder=_lib.CYLINDER3D, cone=_lib.CONE3D, primitive=_lib.PRIMITIVE3D,
                   oriented_primitive=_lib.ORIENTED_PRIMITIVE3D, torus=_lib.TORUS3D)
