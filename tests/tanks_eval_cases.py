"""Shared by tests/test_tanks_eval_cpu.py and tests/test_gpu_tanks_eval.py (not a test module): the Tanks and Temples evaluation
protocol restated in NumPy, the host build of mvster_amd/csrc/reg_math.h, and the cases.

Neither the benchmark's toolbox nor Open3D can be run here, so the restatement follows the protocol's written definition (DESIGN.md
section 4.19) and is the reference: the crop rule edge by edge in float64, Umeyama's closed form on centred pairs (not on the 18
sums the product uses), ICP over scipy's cKDTree (brute force where scipy is missing), the thinning of tests/voxel_thin_cases.py
and np.histogram itself."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np

from tests import cloud_nn_cases as N
from tests import fusion_scene_cases as C
from tests import voxel_thin_cases as V

AXES = {"X": 0, "Y": 1, "Z": 2}
SUM_NAMES = ("n", "d2", "s0", "s1", "s2", "t0", "t1", "t2", "ss") + tuple("t%ds%d" % (a, b) for a in range(3) for b in range(3))


def f32(x):
    return float(np.float32(x))


def smallest_cell(max_dist):
    return N.cell_values(max_dist)[0]


# ---- the definition, restated -----------------------------------------------------------------------------------------------

def volume(axis, poly2d, axis_min, axis_max, w=0.0):
    """-> dict(orthogonal_axis, axis_min, axis_max, polygon [P,3]) from the polygon's (u, v) rows."""
    a = AXES[axis]
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    poly = np.full((len(poly2d), 3), w, np.float64)
    poly[:, u], poly[:, v] = np.asarray(poly2d, np.float64)[:, 0], np.asarray(poly2d, np.float64)[:, 1]
    return dict(orthogonal_axis=axis, axis_min=float(axis_min), axis_max=float(axis_max), polygon=poly)


def transform_numpy(points, T):
    """q = T p in float64, one operation at a time in the header's order -> [N,3] float64."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    if T is None:
        return p
    T = np.asarray(T, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1)


def moved_numpy(points, T):
    """float32(T p); the input's own bits without a transform."""
    if T is None:
        return np.asarray(points, np.float32).reshape(-1, 3).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        return transform_numpy(points, T).astype(np.float32)


def inside_numpy(q, vol):
    """The crop rule on float64 points, edge by edge."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    a = AXES[vol["orthogonal_axis"]]
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    poly = np.asarray(vol["polygon"], np.float64)
    P = len(poly)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = np.isfinite(q).all(1) & (q[:, a] >= vol["axis_min"]) & (q[:, a] <= vol["axis_max"])
        qu, qv = q[:, u], q[:, v]
        odd = np.zeros(len(q), bool)
        for j in range(P):
            k = (j + 1) % P
            uj, vj, uk, vk = poly[j, u], poly[j, v], poly[k, u], poly[k, v]
            cross = ((vj < qv) & (vk >= qv)) | ((vk < qv) & (vj >= qv))
            node = uj + (qv - vj) / (vk - vj) * (uk - uj)
            odd ^= cross & (node < qu)
    return ok & odd


def crop_numpy(points, vol, T=None):
    """-> dict flags [N] uint8, index [K] int64, points [K,3] float32."""
    flags = inside_numpy(transform_numpy(points, T), vol)
    index = np.nonzero(flags)[0].astype(np.int64)
    return dict(flags=flags.astype(np.uint8), index=index, points=moved_numpy(points, T)[index])


def terms_numpy(source, index, dist2, target):
    """[Q,18] float64: the terms of every pair, zeros where there is none."""
    s = np.asarray(source, np.float32).reshape(-1, 3).astype(np.float64)
    has = np.asarray(index) >= 0
    t = np.asarray(target, np.float32).reshape(-1, 3).astype(np.float64)[np.where(has, index, 0)]
    out = np.zeros((len(s), 18), np.float64)
    out[:, 0] = 1.0
    out[:, 1] = np.where(has, dist2, 0.0)
    out[:, 2:5], out[:, 5:8] = s, t
    out[:, 8] = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    for a in range(3):
        for b in range(3):
            out[:, 9 + 3 * a + b] = t[:, a] * s[:, b]
    out[~has] = 0.0
    return out


def fsum_columns(terms):
    """math.fsum of every column (the exact sum, rounded once) and the sum of the absolute terms."""
    return (np.array([math.fsum(terms[:, j]) for j in range(terms.shape[1])]),
            np.array([math.fsum(np.abs(terms[:, j])) for j in range(terms.shape[1])]))


def umeyama_pairs(s, t, with_scaling=True):
    """Umeyama's closed form on centred pairs (float64 [n,3] each) -> 4 x 4 or None."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    n = len(s)
    if n < 3:
        return None
    ms, mt = s.mean(0), t.mean(0)
    sc, tc = s - ms, t - mt
    var = (sc * sc).sum() / n
    if not var > 0:
        return None
    U, D, Vt = np.linalg.svd(tc.T @ sc / n)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = (U * S) @ Vt
    c = (D * S).sum() / var if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c * R, mt - c * (R @ ms)
    return T


class Searcher:
    """Nearest target up to max_dist (its float32 value) of float32 queries: scipy's cKDTree where it is installed (the d2 and
    the limit are then re-evaluated as csrc/nn_math.h writes them), else the brute force of tests/cloud_nn_cases.py."""

    def __init__(self, target, max_dist):
        self.target = np.asarray(target, np.float32).reshape(-1, 3)
        self.md = f32(max_dist)
        try:
            from scipy.spatial import cKDTree
            ok = np.isfinite(self.target).all(1)
            self.ids = np.nonzero(ok)[0]
            self.tree = cKDTree(self.target[ok].astype(np.float64)) if ok.any() else None
        except ImportError:
            self.tree = self.ids = None

    def __call__(self, query):
        """-> (index [Q] int64, -1 for none; dist2 [Q] float64, inf for none)."""
        q = np.asarray(query, np.float32).reshape(-1, 3)
        if self.ids is None:
            r = N.nearest_numpy(q, self.target, self.md, smallest_cell(self.md))
            return r["index"], np.where(r["index"] >= 0, r["dist2"], np.inf)
        index, d2 = np.full(len(q), -1, np.int64), np.full(len(q), np.inf)
        ok = np.isfinite(q).all(1)
        if self.tree is not None and ok.any():
            _, j = self.tree.query(q[ok].astype(np.float64), distance_upper_bound=self.md * (1 + 1e-9))
            has = j < len(self.ids)
            jj = self.ids[np.where(has, j, 0)]
            d = q[ok].astype(np.float64) - self.target[jj].astype(np.float64)
            dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            has &= dd <= np.float64(self.md) * np.float64(self.md)
            index[ok], d2[ok] = np.where(has, jj, -1), np.where(has, dd, np.inf)
        return index, d2


def icp_numpy(source, target, max_dist, init=None, with_scaling=True, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=20,
              search=None):
    """register_clouds restated -> dict like it; ``history`` also carries the rmse / fitness changes."""
    src = np.asarray(source, np.float32).reshape(-1, 3)
    search = Searcher(target, max_dist) if search is None else search
    tgt = search.target.astype(np.float64)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    Q = len(src)

    def evaluate(M):
        s = moved_numpy(src, M)
        index, d2 = search(s)
        has = index >= 0
        n = int(has.sum())
        return (s[has].astype(np.float64), tgt[index[has]]), (n / Q if Q else 0.0), (math.sqrt(d2[has].sum() / n) if n else 0.0), n

    pairs, fitness, rmse, n = evaluate(T)
    history = [dict(fitness=fitness, inlier_rmse=rmse)]
    iterations, converged = 0, False
    for _ in range(max_iteration):
        U = umeyama_pairs(pairs[0], pairs[1], with_scaling) if n else None
        if U is None:
            break
        T = U @ T
        iterations += 1
        pairs, f2, r2, n = evaluate(T)
        history.append(dict(fitness=f2, inlier_rmse=r2, d_fitness=abs(f2 - fitness), d_rmse=abs(r2 - rmse)))
        done = abs(f2 - fitness) < relative_fitness and abs(r2 - rmse) < relative_rmse
        fitness, rmse = f2, r2
        if done:
            converged = True
            break
    return dict(transformation=T, fitness=fitness, inlier_rmse=rmse, correspondences=n, iterations=iterations, converged=converged,
                history=history)


def stop_margin(history, relative_rmse=1e-6, factor=100.0):
    """True where a converged run's last rmse change is below relative_rmse / factor and the one before it (if any) at least
    relative_rmse * factor, and the fitness did not move in either: only then is the iteration count a property of the data and
    not of the last bits of a sum."""
    steps = history[1:]
    if not steps or steps[-1]["d_rmse"] >= relative_rmse / factor or steps[-1]["d_fitness"] != 0:
        return False
    return len(steps) == 1 or (steps[-2]["d_rmse"] >= relative_rmse * factor or steps[-2]["d_fitness"] >= 1e-4)


def thin_numpy(points, voxel):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    return V.thin_numpy(pts, np.zeros((len(pts), 3), np.uint8), voxel, "mean")["points"]


ICP_ROUNDS = ((1.0, 80.0), (0.5, 20.0), (None, 2.0))


def evaluate_numpy(pred, truth, init_trans=None, refine=True, plot_stretch=5):
    """evaluate_scene restated; ``truth`` = dict(gt_points, volume, tau, gt_trans)."""
    pred = np.asarray(pred, np.float32).reshape(-1, 3)
    vol, tau = truth["volume"], f32(truth["tau"])
    T = init_trans if init_trans is not None else (truth.get("gt_trans") if truth.get("gt_trans") is not None else np.eye(4))
    T = np.array(T, np.float64)
    gt = crop_numpy(truth["gt_points"], vol)["points"]
    rounds = []
    if refine:
        for voxel_over_tau, thr in ICP_ROUNDS:
            s = crop_numpy(pred, vol, T)["points"]
            t = gt
            if voxel_over_tau is not None:
                s, t = thin_numpy(s, voxel_over_tau * tau), thin_numpy(gt, voxel_over_tau * tau)
            assert len(s) <= 4000000 and len(t) <= 4000000               # (the stride of the third round is not restated)
            if len(s) < 1:
                break
            reg = icp_numpy(s, t, thr * tau, max_iteration=20)
            T = reg["transformation"] @ T
            rounds.append(dict(reg, source_points=len(s), target_points=len(t)))
    s, t = thin_numpy(crop_numpy(pred, vol, T)["points"], 0.5 * tau), thin_numpy(gt, 0.5 * tau)
    md = f32(plot_stretch * tau)
    cell = smallest_cell(md)
    way_p, way_g = N.nearest_numpy(s, t, md, cell), N.nearest_numpy(t, s, md, cell)
    out = N.scores_numpy(way_p, way_g, md, tau)
    edges = np.arange(0, tau * plot_stretch, tau / 100.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out.update(edges=edges, cum_source=np.cumsum(np.histogram(way_p["dist"], edges)[0]).astype(np.float64) / np.float64(len(s)),
                   cum_target=np.cumsum(np.histogram(way_g["dist"], edges)[0]).astype(np.float64) / np.float64(len(t)))
    out.update(transformation=T, rounds=rounds, pred_thinned=len(s), gt_thinned=len(t), gt_cropped=len(gt),
               gt_dist=way_g["dist"], pred_dist=way_p["dist"])
    return out


# ---- the host build of mvster_amd/csrc/reg_math.h -----------------------------------------------------------------------------

_HM = {}


def load_reg_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/reg_hostmath.cpp like ``dtu_eval_cases.load_eval_hostmath`` and load it, once per process.  No
    compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of reg_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libreghostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "reg_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, i = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    h.hm_reg_transform.restype, h.hm_reg_transform.argtypes = None, [p, l, p, p]
    h.hm_reg_crop.restype, h.hm_reg_crop.argtypes = l, [p, l, p, p, i, i, p, p, p]
    h.hm_reg_terms.restype, h.hm_reg_terms.argtypes = None, [p, p, p, l, p, l, p]
    h.hm_reg_histogram.restype, h.hm_reg_histogram.argtypes = None, [p, l, p, i, p]
    _HM[compilers] = h
    return h


def volume_words(vol):
    """[2 + 2 P] float64: axis_min, axis_max, (u, v) of every vertex -> (axis, words)."""
    a = AXES[vol["orthogonal_axis"]]
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    poly = np.asarray(vol["polygon"], np.float64)
    return a, np.ascontiguousarray(np.concatenate([[vol["axis_min"], vol["axis_max"]], poly[:, (u, v)].reshape(-1)]), np.float64)


def _rows(T):
    return None if T is None else np.ascontiguousarray(np.asarray(T, np.float64)[:3].reshape(-1))


def crop_host(h, points, vol, T=None):
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    a, words = volume_words(vol)
    rows = _rows(T)
    flags, out, index = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.int64)
    K = h.hm_reg_crop(pts.ctypes.data, n, None if rows is None else rows.ctypes.data, words.ctypes.data, (len(words) - 2) // 2, a,
                      flags.ctypes.data, out.ctypes.data, index.ctypes.data)
    return dict(flags=flags, index=index[:K].copy(), points=out[:K].copy())


def transform_host(h, points, T):
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rows, out = _rows(T), np.zeros((len(pts), 3), np.float32)
    h.hm_reg_transform(pts.ctypes.data, len(pts), rows.ctypes.data, out.ctypes.data)
    return out


def terms_host(h, source, index, dist2, target):
    s, t = np.ascontiguousarray(source, np.float32).reshape(-1, 3), np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    idx, d2 = np.ascontiguousarray(index, np.int64), np.ascontiguousarray(dist2, np.float64)
    out = np.zeros((len(s), 18), np.float64)
    h.hm_reg_terms(s.ctypes.data, idx.ctypes.data, d2.ctypes.data, len(s), t.ctypes.data, len(t), out.ctypes.data)
    return out


def histogram_host(h, dist, edges):
    d, e = np.ascontiguousarray(dist, np.float32), np.ascontiguousarray(edges, np.float64)
    out = np.zeros(len(e) - 1, np.int64)
    h.hm_reg_histogram(d.ctypes.data, len(d), e.ctypes.data, len(e) - 1, out.ctypes.data)
    return out


def assert_crop_same(got, want, what=""):
    for k, dt in (("flags", np.uint8), ("index", np.int64), ("points", np.float32)):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


# ---- crop and transform cases ---------------------------------------------------------------------------------------------------

PENTAGON = ((0, 0), (4, 0), (4, 3), (2, 1), (0, 3))                         # concave at (2, 1)
PENTAGON_TABLE = (((2, 1), True), ((4, 1), True), ((1, 2), True), ((0, 1), False), ((1, 0), False), ((1, 3), False),
                  ((3, 2), False), ((2, 2), False))
CROP_SIZES = (1, 63, 64, 65, 257, 4099)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def similarity(axis, degrees, scale, translation):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * rotation(axis, degrees), translation
    return T


def polygons():
    th = 2 * np.pi * np.arange(1024) / 1024
    r = 2.0 + 0.6 * np.sin(7 * th)
    gon = np.stack([2 + r * np.cos(th), 1.5 + r * np.sin(th)], 1).astype(np.float32).astype(np.float64)
    return dict(triangle=np.array(((0.5, -1), (3.25, 0.5), (-0.75, 2.5)), np.float64), pentagon=np.array(PENTAGON, np.float64),
                pentagon_rev=np.array(PENTAGON[::-1], np.float64), gon1024=gon)


CROP_T = similarity((0.2, -0.4, 0.9), 33.0, 1.3, (0.4, -1.1, 0.7))


def crop_points_for(vol, n, seed, T=None):
    """n float32 points around the volume: uniform over its box grown by a fifth, and from 64 points on also points exactly on
    vertices, on edges, on axis_min / axis_max, and NaN / +-inf coordinates.  With a transform the points are the pre-images."""
    rng = np.random.default_rng(seed)
    a, words = volume_words(vol)
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    uv = words[2:].reshape(-1, 2)
    lo, hi = uv.min(0), uv.max(0)
    q = np.zeros((n, 3), np.float64)
    q[:, u] = rng.uniform(lo[0] - 0.2 * (hi[0] - lo[0]), hi[0] + 0.2 * (hi[0] - lo[0]), n)
    q[:, v] = rng.uniform(lo[1] - 0.2 * (hi[1] - lo[1]), hi[1] + 0.2 * (hi[1] - lo[1]), n)
    span = vol["axis_max"] - vol["axis_min"]
    q[:, a] = rng.uniform(vol["axis_min"] - 0.2 * span, vol["axis_max"] + 0.2 * span, n)
    bad = None
    if n >= 64:
        P = len(uv)
        k = 0
        for j in range(min(P, 8)):                                          # vertices, then edge points at 1/2 and 1/4
            nxt = uv[(j + 1) % P]
            for point in (uv[j], (uv[j] + nxt) / 2, uv[j] + (nxt - uv[j]) / 4):
                q[k, u], q[k, v], q[k, a] = point[0], point[1], vol["axis_min"] + span / 2
                k += 1
        inner = uv.mean(0) if P != 5 else np.array((1.0, 1.0))
        ends = np.float32([vol["axis_min"], vol["axis_max"]])               # (float32 neighbours: the points are float32)
        for w in (ends[0], ends[1], np.nextafter(ends[0], np.float32(-np.inf)), np.nextafter(ends[1], np.float32(np.inf))):
            q[k, u], q[k, v], q[k, a] = inner[0], inner[1], w
            k += 1
        bad = (k, ((0, np.nan), (1, np.inf), (2, -np.inf), (a, np.nan), (u, np.inf), (v, -np.inf)))
    if T is not None:
        Ti = np.linalg.inv(T)
        q = q @ Ti[:3, :3].T + Ti[:3, 3]
    p = q.astype(np.float32)
    if bad is not None:
        k, items = bad
        for j, (col, val) in enumerate(items):
            p[k + j, col] = val
    return p


_CROP = {}


def crop_cases():
    """name -> dict(points, volume, T)."""
    if _CROP:
        return _CROP
    polys = polygons()
    seed = 0
    for pname, poly in polys.items():
        for axis in "XYZ":
            for T in (None, CROP_T):
                seed += 1
                vol = volume(axis, poly, -0.5, 1.25)
                _CROP["%s_%s_%s_n257" % (pname, axis, "t" if T is not None else "p")] = dict(
                    points=crop_points_for(vol, 257, seed, T), volume=vol, T=T)
    for i, n in enumerate(CROP_SIZES):
        for T in (None, CROP_T):
            seed += 1
            vol = volume("XYZ"[i % 3], polys["pentagon"], -0.5, 1.25)
            _CROP["sizes_%s_n%d" % ("t" if T is not None else "p", n)] = dict(points=crop_points_for(vol, n, seed, T), volume=vol, T=T)
    rng = np.random.default_rng(99)
    vol = volume("Z", polys["pentagon"], -1.0, 1.0)
    kept = np.stack([rng.uniform(0.1, 1.9, 300), rng.uniform(0.1, 0.9, 300), rng.uniform(-0.9, 0.9, 300)], 1).astype(np.float32)
    _CROP["all_kept"] = dict(points=kept, volume=vol, T=None)
    _CROP["none_kept"] = dict(points=(kept + np.float32(10)).astype(np.float32), volume=vol, T=None)
    return _CROP


def pentagon_table_points(axis):
    """The table's (u, v) points as 3-D float32 points of the volume with that orthogonal axis -> (points, inside)."""
    vol = volume(axis, PENTAGON, -1.0, 1.0)
    a = AXES[axis]
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    p = np.zeros((len(PENTAGON_TABLE), 3), np.float32)
    for k, ((x, y), _) in enumerate(PENTAGON_TABLE):
        p[k, u], p[k, v] = x, y
    return vol, p, np.array([w for _, w in PENTAGON_TABLE])


# ---- correspondence sums ----------------------------------------------------------------------------------------------------------

SUM_SIZES = (1, 64, 65, 1000, 70000)                                        # 70 000: 18 partial rows of 4096 points
SUM_MAX_DIST = 0.05
SUM_T = similarity((0.3, -0.5, 0.81), 5.0, 1.02, (0.01, 0.02, -0.03))
_SUMS = {}


def sums_case(Q):
    """-> dict(source [Q,3] (before SUM_T), target [M,3], moved = float32(T source), index / dist2 (brute force over all pairs
    with the host build of nn_math.h), terms [Q,18], want [18] = math.fsum, bound [18] = n 2^-52 sum|term|)."""
    if Q in _SUMS:
        return _SUMS[Q]
    rng = np.random.default_rng(1000 + Q)
    M = 1500
    target = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    q = target[rng.integers(0, M, Q)].astype(np.float64) + rng.normal(0, 0.01, (Q, 3))
    far = rng.uniform(0, 1, Q) < 0.15
    if Q > 1:
        q[far] += 5.0                                                       # no candidate
    Ti = np.linalg.inv(SUM_T)
    source = (q @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    if Q >= 64:
        source[7, 1] = np.nan
        source[Q - 2, 0] = np.inf
        source[Q // 2, 2] = np.nan
    moved = moved_numpy(source, SUM_T)
    near = N.nearest_host(N.load_nn_hostmath(), moved, target, SUM_MAX_DIST, smallest_cell(SUM_MAX_DIST))
    terms = terms_numpy(moved, near["index"], near["dist2"], target)
    want, mag = fsum_columns(terms)
    _SUMS[Q] = dict(source=source, target=target, moved=moved, index=near["index"], dist2=near["dist2"], terms=terms, want=want,
                    bound=want[0] * 2.0 ** -52 * mag)
    return _SUMS[Q]


# ---- histogram --------------------------------------------------------------------------------------------------------------------

def histogram_case(bins):
    """10 000 float32 distances with values equal to edges, the last edge, NaN and +inf -> (dist, edges)."""
    rng = np.random.default_rng(bins)
    # 499 bins: the protocol's own edges for tau = 0.02 and plot_stretch = 5
    edges = np.arange(0, 0.02 * 5, 0.02 / 100) if bins == 499 else np.arange(bins + 1) * (0.1 / bins)
    assert len(edges) == bins + 1
    d = rng.uniform(-0.01, 0.12, 10000).astype(np.float32)
    pick = rng.integers(0, len(edges), 600)
    d[:600] = edges[pick].astype(np.float32)                                # equal to an edge where the edge is a float32, beside it else
    d[600:640] = np.float32(edges[-1])
    d[640:660] = np.nan
    d[660:680] = np.inf
    d[680:700] = 0.0
    d[700:720] = np.nextafter(np.float32(edges[-1]), np.float32(1))
    return d, edges


# ---- ICP and the protocol ------------------------------------------------------------------------------------------------------------

G = similarity((0.3, -0.5, 0.81), 2.0, 1.01, (0.02, -0.015, 0.01))
G_RIGID = similarity((0.3, -0.5, 0.81), 2.0, 1.0, (0.02, -0.015, 0.01))
ICP_MAX_DIST = 0.1
ICP_TAU = 0.004
ICP_TOLERANCE_FACTOR = 4.0
_ICP = {}


def surface_cloud():
    """6000 random candidates on z = 0.3 sin 2.1 x + 0.2 cos(1.7 y + 0.4) + 0.15 x y over [-1, 1]^2 (seed 1), thinned greedily,
    in their order, to a minimum separation of 0.012 -> (points float32 [n,3], half = the indices of a random half)."""
    if "surface" not in _ICP:
        rng = np.random.default_rng(1)
        x, y = rng.uniform(-1, 1, 6000), rng.uniform(-1, 1, 6000)
        p = np.stack([x, y, 0.3 * np.sin(2.1 * x) + 0.2 * np.cos(1.7 * y + 0.4) + 0.15 * x * y], 1).astype(np.float32)
        p64 = p.astype(np.float64)
        keep = []
        for i in range(len(p)):
            if not keep or ((p64[keep] - p64[i]) ** 2).sum(1).min() >= 0.012 ** 2:
                keep.append(i)
        pts = p[keep]
        half = np.sort(rng.permutation(len(pts))[:len(pts) // 2])
        _ICP["surface"] = (pts, half)
    return _ICP["surface"]


def icp_case(rigid=False):
    """-> dict(source, target, partner (index of every source point's true partner), G, restated = icp_numpy's result, error =
    the restatement's largest point error, tolerance = 4 x that)."""
    key = "rigid" if rigid else "similarity"
    if key not in _ICP:
        pts, half = surface_cloud()
        g = G_RIGID if rigid else G
        gi = np.linalg.inv(g)
        source = (pts[half].astype(np.float64) @ gi[:3, :3].T + gi[:3, 3]).astype(np.float32)
        restated = icp_numpy(source, pts, ICP_MAX_DIST, with_scaling=not rigid)
        error = point_error(restated["transformation"], source, pts[half])
        _ICP[key] = dict(source=source, target=pts, partner=half, G=g, restated=restated, error=error,
                         tolerance=ICP_TOLERANCE_FACTOR * error)
    return _ICP[key]


def point_error(T, source, partners):
    """The largest distance of float32(T source) from its partner, in float64."""
    d = moved_numpy(source, T).astype(np.float64) - np.asarray(partners, np.float32).astype(np.float64)
    return float(np.sqrt((d * d).sum(1)).max())


def protocol_case():
    """The surface case through the whole protocol with refine: tau = 0.004, crop |x|, |y| <= 0.9 -> dict(pred, truth, G,
    restated = evaluate_numpy's result)."""
    if "protocol" not in _ICP:
        c = icp_case()
        vol = volume("Z", ((-0.9, -0.9), (0.9, -0.9), (0.9, 0.9), (-0.9, 0.9)), -2.0, 2.0)
        truth = dict(gt_points=c["target"], volume=vol, tau=ICP_TAU, gt_trans=None)
        _ICP["protocol"] = dict(pred=c["source"], truth=truth, G=c["G"], restated=evaluate_numpy(c["source"], truth))
    return _ICP["protocol"]


LATTICE = 40


def lattice_case(tau, premoved=False):
    """refine=False with counts known in advance: the ground truth a planar 40 x 40 lattice of spacing 8 tau, the crop's edges at
    half-lattice positions, the prediction by i mod 4: class 0 absent, 1 moved 0.2 tau in z, 2 moved 3 tau in z, 3 moved 0.2 tau
    in x.  -> dict(pred, truth, init_trans, precision = (num, den), recall = (num, den))."""
    s = 8.0 * tau
    i, j = np.meshgrid(np.arange(LATTICE), np.arange(LATTICE), indexing="ij")
    gt = np.stack([i.reshape(-1) * s, j.reshape(-1) * s, np.zeros(LATTICE * LATTICE)], 1)
    lo_i, hi_i, lo_j, hi_j = 3.5, 33.5, 5.5, 36.5
    vol = volume("Z", ((lo_i * s, lo_j * s), (hi_i * s, lo_j * s), (hi_i * s, hi_j * s), (lo_i * s, hi_j * s)), -10 * tau, 10 * tau)
    inside = ((i > lo_i) & (i < hi_i) & (j > lo_j) & (j < hi_j)).reshape(-1)
    cls = np.arange(LATTICE * LATTICE) % 4
    pred = gt.copy()
    pred[cls == 1, 2] += 0.2 * tau
    pred[cls == 2, 2] += 3.0 * tau
    pred[cls == 3, 0] += 0.2 * tau
    pred = pred[cls != 0]
    pin, pcls = inside[cls != 0], cls[cls != 0]
    good = int((pin & (pcls != 2)).sum())
    out = dict(truth=dict(gt_points=gt.astype(np.float32), volume=vol, tau=tau, gt_trans=None), init_trans=None,
               precision=(good, int(pin.sum())), recall=(good, int(inside.sum())))
    if premoved:
        gi = np.linalg.inv(G)
        pred = pred @ gi[:3, :3].T + gi[:3, 3]
        out["init_trans"] = G
    out["pred"] = pred.astype(np.float32)
    return out


# ---- files ------------------------------------------------------------------------------------------------------------------------------

def write_ply_xyz(filename, points, dtype="float"):
    """A binary little-endian PLY with x, y, z as ``float`` or ``double`` (and a uchar property between them)."""
    pts = np.asarray(points)
    np_t = "<f4" if dtype == "float" else "<f8"
    v = np.zeros(len(pts), np.dtype([("x", np_t), ("y", np_t), ("flag", "u1"), ("z", np_t)]))
    v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    with open(filename, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty %s x\nproperty %s y\nproperty uchar flag\n"
                 "property %s z\nend_header\n" % (len(pts), dtype, dtype, dtype)).encode("ascii"))
        f.write(v.tobytes())


def write_volume_json(filename, vol):
    import json
    with open(filename, "w") as f:
        json.dump(dict(axis_max=vol["axis_max"], axis_min=vol["axis_min"], bounding_polygon=np.asarray(vol["polygon"]).tolist(),
                       class_name="SelectionPolygonVolume", orthogonal_axis=vol["orthogonal_axis"], version_major=1,
                       version_minor=0), f, indent=1)


def write_scene_files(folder, scene, truth, gt_trans):
    os.makedirs(folder, exist_ok=True)
    write_ply_xyz(os.path.join(folder, scene + ".ply"), truth["gt_points"])
    write_volume_json(os.path.join(folder, scene + ".json"), truth["volume"])
    np.savetxt(os.path.join(folder, scene + "_trans.txt"), gt_trans)


def write_trajectory_log(filename, poses):
    with open(filename, "w") as f:
        for k, P in enumerate(poses):
            f.write("%d %d %d\n" % (k, k, 0))
            for row in np.asarray(P):
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
