"""Shared by tests/test_cloud_clean_cpu.py and tests/test_gpu_cloud_clean.py (not a test module): the k nearest points, the two
outlier filters and the normals restated in NumPy, the host build of mvster_amd/csrc/knn_math.h, and
the case clouds.

Neither yardstick comes from the reference tree, which has no such step: the restatement follows the definition in float64 over
all pairs (np.lexsort on (index, d2)), the host build is the kernels' own arithmetic compiled for the CPU, once as a brute force
and once through a hash grid with the stopping rule."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from tests import cloud_nn_cases as N
from tests import fusion_scene_cases as C

MD = N.MD
ROWS = 512                                 # the restatement sorts ROWS x M distances at a time
KNN_KEYS = ("dist2", "index", "count")


# ---- the definition, restated -------------------------------------------------------------------------------------------

def knn_numpy(query, target, k, max_dist, cell, exclude_self=False):
    """Brute force over all pairs in float64, np.lexsort on (index, d2) -> dict like fusion.nearest_neighbors (NumPy arrays)."""
    query = np.asarray(query, np.float32).reshape(-1, 3)
    target = np.asarray(target, np.float32).reshape(-1, 3)
    Q = len(query)
    qv, tv = N.valid_points(query, cell), N.valid_points(target, cell)
    limit = np.float64(np.float32(max_dist)) * np.float64(np.float32(max_dist))
    dist2 = np.full((Q, k), np.inf, np.float64)
    index = np.full((Q, k), -1, np.int64)
    tidx = np.nonzero(tv)[0]
    t64 = target[tidx].astype(np.float64)
    for q0 in range(0, Q, ROWS):
        qs = slice(q0, min(q0 + ROWS, Q))
        a = np.where(qv[qs, None], query[qs], 0).astype(np.float64)
        dx, dy, dz = (a[:, None, j] - t64[None, :, j] for j in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[d2 > limit] = np.inf
        if exclude_self:
            d2[np.arange(q0, qs.stop)[:, None] == tidx[None]] = np.inf
        order = np.lexsort((np.broadcast_to(tidx, d2.shape), d2), axis=1)[:, :k]
        m = order.shape[1]
        dist2[qs, :m] = np.take_along_axis(d2, order, 1)
        index[qs, :m] = tidx[order]
    index[~np.isfinite(dist2)] = -1
    index[~qv] = -1
    count = (index >= 0).sum(1).astype(np.int32)
    dist2[~qv] = np.nan
    return dict(dist2=dist2, index=index, count=count, dropped_query=int((~qv).sum()), dropped_target=int((~tv).sum()))


def radius_numpy(points, radius, nb_points, cell):
    """-> (neighbours [M] int32, keep [M] bool)"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    v = N.valid_points(points, cell)
    limit = np.float64(np.float32(radius)) * np.float64(np.float32(radius))
    p = points[v].astype(np.float64)
    nb = np.zeros(len(points), np.int32)
    cnt = np.zeros(len(p), np.int64)
    for q0 in range(0, len(p), ROWS):
        a = p[q0:q0 + ROWS]
        dx, dy, dz = (a[:, None, j] - p[None, :, j] for j in range(3))
        cnt[q0:q0 + ROWS] = (((dx * dx + dy * dy) + dz * dz) <= limit).sum(1) - 1          # but the point itself
    nb[v] = cnt
    return nb, v & (nb >= nb_points)


def mean_numpy(lists, k):
    """The statistical filter's mean from the lists of knn_numpy(..., exclude_self=True), summed in list order."""
    s = np.zeros(len(lists["count"]), np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(k):
            s = s + np.sqrt(lists["dist2"][:, j])
    mean = s / np.float64(k)
    mean[lists["count"] < k] = np.inf
    mean[np.isnan(lists["dist2"][:, 0])] = np.nan
    return mean


def stats_numpy(mean, std_ratio):
    """-> n, mu, sigma, threshold with NumPy's own (pairwise) sums"""
    part = mean[np.isfinite(mean)]
    n = len(part)
    mu = float(part.mean()) if n else float("nan")
    sigma = float(part.std(ddof=1)) if n >= 2 else 0.0
    return n, mu, sigma, mu + std_ratio * sigma


def normals_numpy(points, lists, toward=None):
    """numpy.linalg.eigh on the covariance of every neighbourhood of knn_numpy(..., exclude_self=True) -> normals [M,3] float64
    (zeros where count < 2), valid [M], gap [M] = (l1 - l0) / l2 (inf where not valid)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    M = len(points)
    normals, valid, gap = np.zeros((M, 3)), lists["count"] >= 2, np.full(M, np.inf)
    for i in np.nonzero(valid)[0]:
        e = points[lists["index"][i, :lists["count"][i]]].astype(np.float64) - points[i].astype(np.float64)
        m = len(e) + 1
        mean = e.sum(0) / m
        w, v = np.linalg.eigh(e.T @ e / m - np.outer(mean, mean))
        normals[i], gap[i] = v[:, 0], (w[1] - w[0]) / w[2]
        if toward is not None and normals[i] @ (toward[i].astype(np.float64) - points[i].astype(np.float64)) < 0:
            normals[i] = -normals[i]
    return normals, valid, gap


def eigh_normals(cov):
    """cov [M,6] (xx, xy, xz, yy, yz, zz) -> the unit eigenvectors of the smallest eigenvalues [M,3] and the gaps [M]."""
    A = np.zeros((len(cov), 3, 3))
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[:, a, b] = A[:, b, a] = cov[:, j]
    w, v = np.linalg.eigh(A)
    return v[:, :, 0], (w[:, 1] - w[:, 0]) / w[:, 2]


def angles(a, b):
    """The angle between two fields of unit vectors up to sign [M], from the cross product (exact near 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


def assert_same_knn(got, want, what=""):
    for key in ("dropped_query", "dropped_target"):
        assert int(got[key]) == int(want[key]), (what, key, int(got[key]), int(want[key]))
    for key in KNN_KEYS:
        assert_bytes(got[key], want[key], (what, key))


def assert_bytes(g, w, what=""):
    g, w = np.asarray(g), np.asarray(w)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = (g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(1)
        raise AssertionError((what, "%d rows differ, the first: %d" % (bad.sum(), np.nonzero(bad)[0][0])))


# ---- the host build of mvster_amd/csrc/knn_math.h -------------------------------------------------------------------------

_HM = {}


def load_knn_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/knn_hostmath.cpp with the flags of ``cloud_nn_cases.load_nn_hostmath`` and load it, once per
    process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of knn_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libknnhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "knn_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, f, i, d = ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int, ctypes.c_double
    for fn, res in ((h.hm_knn_brute, None), (h.hm_knn_grid, l)):
        fn.restype, fn.argtypes = res, [p, l, p, l, f, f, i, i, p, p, p, p]
    h.hm_radius_count.restype, h.hm_radius_count.argtypes = None, [p, l, f, f, i, p]
    h.hm_knn_mean.restype, h.hm_knn_mean.argtypes = None, [p, l, f, f, i, i, p, p]
    h.hm_knn_stats.restype, h.hm_knn_stats.argtypes = None, [p, l, d, p, p]
    h.hm_knn_normals.restype, h.hm_knn_normals.argtypes = None, [p, l, f, f, i, i, p, p, p, p]
    _HM[compilers] = h
    return h


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def knn_host(h, query, target, k, max_dist, cell, exclude_self=False, grid=False):
    query, target = _f32(query), _f32(target)
    Q = len(query)
    dist2, index, count = np.zeros((Q, k), np.float64), np.zeros((Q, k), np.int64), np.zeros(Q, np.int32)
    dropped = np.zeros(2, np.int64)
    probes = (h.hm_knn_grid if grid else h.hm_knn_brute)(query.ctypes.data, Q, target.ctypes.data, len(target), max_dist, cell, k,
                                                         int(exclude_self), dist2.ctypes.data, index.ctypes.data,
                                                         count.ctypes.data, dropped.ctypes.data)
    out = dict(dist2=dist2, index=index, count=count, dropped_query=int(dropped[0]), dropped_target=int(dropped[1]))
    if grid:
        out["probes"] = probes
    return out


def radius_host(h, points, radius, nb_points, cell, grid=False):
    """-> (neighbours, keep)"""
    points = _f32(points)
    nb = np.zeros(len(points), np.int32)
    h.hm_radius_count(points.ctypes.data, len(points), radius, cell, int(grid), nb.ctypes.data)
    return nb, N.valid_points(points, cell) & (nb >= nb_points)


def statistical_host(h, points, k, std_ratio, max_dist, cell, grid=False):
    """-> dict(mean, count, n, mu, sigma, threshold, keep)"""
    points = _f32(points)
    M = len(points)
    count, mean = np.zeros(M, np.int32), np.zeros(M, np.float64)
    h.hm_knn_mean(points.ctypes.data, M, max_dist, cell, k, int(grid), count.ctypes.data, mean.ctypes.data)
    stats, keep = np.zeros(4, np.float64), np.zeros(M, np.uint8)
    h.hm_knn_stats(mean.ctypes.data, M, std_ratio, stats.ctypes.data, keep.ctypes.data)
    return dict(mean=mean, count=count, n=int(stats[0]), mu=float(stats[1]), sigma=float(stats[2]), threshold=float(stats[3]),
                keep=keep.astype(bool))


def normals_host(h, points, k, max_dist, cell, toward=None, grid=False):
    """-> dict(normals [M,3] float32, valid [M] bool, cov [M,6] float64)"""
    points = _f32(points)
    M = len(points)
    tw = None if toward is None else _f32(toward)
    normals, valid, cov = np.zeros((M, 3), np.float32), np.zeros(M, np.uint8), np.zeros((M, 6), np.float64)
    h.hm_knn_normals(points.ctypes.data, M, max_dist, cell, k, int(grid), None if tw is None else tw.ctypes.data,
                     normals.ctypes.data, valid.ctypes.data, cov.ctypes.data)
    return dict(normals=normals, valid=valid.astype(bool), cov=cov)


# ---- the case clouds ---------------------------------------------------------------------------------------------------------

def lattice(n, step=1.0, origin=(0.0, 0.0, 0.0)):
    g = np.arange(n, dtype=np.float64) * step
    return (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)).astype(np.float32)


_KNN = None
LATTICE_K = 10                             # interior lattice points: 6 neighbours at d2 = 1, 12 at d2 = 2 -- the cut falls among those


def knn_cases():
    """name -> (query, target, max_dist, same): ``same``: the query IS the target (exclude_self is allowed).  Built once."""
    global _KNN
    if _KNN is not None:
        return _KNN
    rng = np.random.RandomState(23)
    base = N.cases()
    out = {}
    for name in ("ties", "faces", "invalid", "all_invalid_target", "one_cell", "m1", "q0", "m0", "odd", "at_max_dist",
                 "below_max_dist", "far_outside"):
        q, t, md = base[name]
        out[name] = (q, t, md, False)
    md, g = MD, np.float64(N.default_cell(MD))

    def put(name, q, t=None, max_dist=md):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        out[name] = (q, q if t is None else np.ascontiguousarray(t, np.float32).reshape(-1, 3), N.f32(max_dist), t is None)
    # an integer lattice of 9^3 points: many exact ties, the cut at k = LATTICE_K inside the group d2 = 2
    lat = lattice(9)
    put("lattice", lat[rng.permutation(len(lat))], max_dist=2.5)
    # every point three times (d2 = 0 between distinct indices), shuffled
    pts = (rng.rand(120, 3) * 2 - 1) * md
    put("duplicates", np.repeat(pts, 3, 0)[rng.permutation(360)])
    # targets exactly at max_dist (3-4-5 triangles on every axis pair and sign) and one float32 beyond it
    e = 2.0 ** -6
    at = np.array([[3, 4, 0], [-3, 4, 0], [0, 3, -4], [4, 0, 3], [0, -4, -3], [5, 0, 0], [0, 0, -5]], np.float64) * e
    beyond = at.astype(np.float32).copy()
    for row in beyond:
        j = int(np.argmax(np.abs(row)))
        row[j] = np.nextafter(row[j], np.float32(np.sign(row[j]) * np.inf))
    put("boundary", np.zeros((1, 3)), np.concatenate([beyond, at]), 5 * e)
    # the stopping rule.  Query 0: its list of k = 2 is full after shell 1 with entries at 1.9 g and 1.95 g, and shell 2 holds a
    # nearer one at 1.1 g.  Query 1 (60 max_dist away): two near targets in its own cell, the third at 3.99 g = just inside
    # max_dist in shell 4 = R - 1, the last shell that can hold a candidate but through rounding, and a decoy beyond max_dist.
    q0, t0 = N.ring_stop(g, np.zeros(3))
    extra = q0[0] - 1.95 * g / np.sqrt(3.0)
    o = np.array([0.0, 60 * md, 0.0])
    q1 = np.array([0.95, 0.5, 0.5]) * g + o
    t1 = np.stack([q1 + [0, 0.1 * g, 0], q1 + [0, 0, -0.2 * g], q1 + [3.99 * g, 0, 0], q1 + [-4.02 * g, 0, 0]])
    put("stop_rule", np.concatenate([q0, q1[None]]), np.concatenate([t0, extra[None], t1]))
    # everything in one cell of every grid but the smallest
    put("single_cell", (np.array([3.0, 1.0, -2.0]) + 0.1 + 0.8 * rng.rand(700, 3)) * g)
    # random clouds against themselves and against another
    put("self_random", N.random_cloud(3000, md, seed=11))
    put("pair_random", N.random_cloud(1500, md, seed=12), N.random_cloud(2500, md, seed=13))
    put("all_invalid", np.full((70, 3), np.nan))
    put("empty", np.zeros((0, 3)))
    _KNN = out
    return out


KNN_CASE_NAMES = ("ties", "faces", "invalid", "all_invalid_target", "one_cell", "m1", "q0", "m0", "odd", "at_max_dist",
                  "below_max_dist", "far_outside", "lattice", "duplicates", "boundary", "stop_rule", "single_cell", "self_random",
                  "pair_random", "all_invalid", "empty")
KS = (1, 2, 5, 16, 32)


def case_ks(name):
    """The k a case runs at: all of KS for the small ones, fewer for the crowded ones (one_cell: 5 000 targets in a cell)."""
    if name == "lattice":
        return (LATTICE_K, 32)
    if name in ("one_cell", "self_random", "pair_random", "faces"):
        return (5, 32)
    if name == "stop_rule":
        return (2, 3)
    return KS


def scale_cloud():
    return N.random_cloud(100003, MD, seed=31)


# radius filter: a dense lattice (every point has >= 3 neighbours at distance 1), lone points and an isolated pair
RADIUS = 1.1


def radius_cloud():
    """-> (points, kinds): kinds 0 = lattice, 1 = lone, 2 = pair; shuffled, with two invalid rows (kind 3)."""
    rng = np.random.RandomState(5)
    lat = lattice(6)
    lone = np.array([[20, 0, 0], [0, -20, 3], [-15, 15, 15], [40, 40, -40]], np.float32)
    pair = np.array([[0, 30, 0], [0.5, 30, 0]], np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    pts = np.concatenate([lat, lone, pair, bad])
    kinds = np.concatenate([np.zeros(len(lat)), np.ones(4), np.full(2, 2), np.full(2, 3)]).astype(int)
    order = rng.permutation(len(pts))
    return pts[order], kinds[order]


# statistical filter: a Gaussian blob of 4096 points and 16 planted points far outside it
STAT_K, STAT_RATIO, STAT_MD = 8, 2.0, 4.0


def blob_cloud():
    """-> (points [4112,3], planted [4112] bool), shuffled"""
    rng = np.random.RandomState(9)
    blob = rng.randn(4096, 3)
    d = rng.randn(16, 3)
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * (6.0 + 3.0 * rng.rand(16, 1))
    pts = np.concatenate([blob, far]).astype(np.float32)
    planted = np.arange(len(pts)) >= 4096
    order = rng.permutation(len(pts))
    return pts[order], planted[order]


# normals
GAP = 1e-3                                 # (l1 - l0) / l2 every compared point must have
ANGLE = 1e-6                               # rad


def plane_cloud():
    """A tilted plane of 40 x 40 jittered points with noise of 2 % of the spacing off the plane -> (points, k, max_dist)."""
    rng = np.random.RandomState(3)
    u, v = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij")
    uv = np.stack([u, v], -1).reshape(-1, 2) + 0.3 * (rng.rand(1600, 2) - 0.5)
    a, b = np.array([0.8, 0.36, 0.48]), np.array([-0.6, 0.48, 0.64])
    n = np.cross(a, b)
    pts = uv[:, :1] * a + uv[:, 1:] * b + 0.02 * rng.randn(1600, 1) * n + np.array([3.0, -7.0, 2.0])
    return (0.05 * pts).astype(np.float32), 12, 0.15


def sphere_cloud():
    """3 000 points on the unit sphere around (1, 2, 3) -> (points, centre, k, max_dist)."""
    rng = np.random.RandomState(4)
    d = rng.randn(3000, 3)
    c = np.array([1.0, 2.0, 3.0])
    return (d / np.linalg.norm(d, axis=1, keepdims=True) + c).astype(np.float32), c.astype(np.float32), 10, 0.3


def few_cloud():
    """A lone point (0 neighbours), a pair (1 each) and a triangle (2 each), max_dist 1 -> (points, neighbours)"""
    pts = np.array([[10, 0, 0], [0, 10, 0], [0.5, 10, 0], [0, 0, 10], [0.5, 0, 10], [0, 0.5, 10.25]], np.float32)
    return pts, np.array([0, 1, 1, 2, 2, 2])


def cross_cloud():
    """The origin and (+-1, 0, 0), (0, +-1, 0): the origin's C is diag(2/5, 2/5, 0) exactly, no rotation, the normal (0, 0, 1)
    exactly -- so n . (toward - p) is exactly 0 for toward = (1, 0, 0).  max_dist 1.25: the others see the origin and nothing else
    but each other at sqrt(2) > 1.25."""
    return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)


def line_cloud():
    """30 points on a line (every neighbourhood collinear: two equal smallest eigenvalues up to rounding)"""
    t = np.arange(30, dtype=np.float64)[:, None]
    return (np.array([0.3, -0.2, 0.1]) + t * np.array([0.02, 0.03, -0.015])).astype(np.float32)
