"""Shared by tests/test_cloud_nn_cpu.py and tests/test_gpu_cloud_nn.py (not a test module): cloud-to-cloud nearest distances
 restated in NumPy, the host build of mvster_amd/csrc/nn_math.h, and the case clouds.

Neither yardstick comes from the reference tree, which scores nothing: the restatement follows the definition operation by
operation in float64 over all pairs, the host build is the kernels' own arithmetic compiled for the CPU, once as a brute force
and once through a hash grid.  All are exact, so every comparison is equality of bytes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from tests import fusion_scene_cases as C

HALF = 1 << 20
KEYS = ("dist", "dist2", "index")
MD = 0.5                                   # max_dist of most cases: cell max_dist / 4 = 0.125 is exact in float32
CHUNK = 8192                               # the restatement never holds more than CHUNK x CHUNK distances


def f32(x):
    return float(np.float32(x))


def cell_values(max_dist):
    """The four cells every case runs at: max_dist / 15 (the smallest allowed: the next float32 up where the rounded quotient
    falls below it), max_dist / 4 (the default), max_dist and 4 * max_dist."""
    md = np.float64(np.float32(max_dist))
    c15 = np.float32(md / 15)
    if np.float64(c15) < md / 15:
        c15 = np.nextafter(c15, np.float32(np.inf))
    return (float(c15), f32(md / 4), f32(md), f32(md * 4))


def default_cell(max_dist):
    return f32(np.float64(np.float32(max_dist)) / 4)


# ---- the definition, restated -------------------------------------------------------------------------------------------

def valid_points(points, cell):
    """[M] bool: finite and within 2^20 cells of the origin (vox::point_key)."""
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor(np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64) / np.float64(np.float32(cell)))
        return ((fi >= -HALF) & (fi < HALF)).all(1)


def nearest_numpy(query, target, max_dist, cell):
    """Brute force over all pairs in float64, CHUNK x CHUNK at a time -> dict like fusion.nearest_distances (NumPy arrays)."""
    query = np.asarray(query, np.float32).reshape(-1, 3)
    target = np.asarray(target, np.float32).reshape(-1, 3)
    Q = len(query)
    qv, tv = valid_points(query, cell), valid_points(target, cell)
    limit = np.float64(np.float32(max_dist)) * np.float64(np.float32(max_dist))
    best = np.full(Q, np.inf, np.float64)
    index = np.full(Q, -1, np.int64)
    tidx = np.nonzero(tv)[0]
    t64 = target[tidx].astype(np.float64)
    for q0 in range(0, Q, CHUNK):
        qs = slice(q0, min(q0 + CHUNK, Q))
        a = np.where(qv[qs, None], query[qs], 0).astype(np.float64)
        for t0 in range(0, len(tidx), CHUNK):
            b = t64[t0:t0 + CHUNK]
            dx, dy, dz = (a[:, None, j] - b[None, :, j] for j in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[d2 > limit] = np.inf
            j = np.argmin(d2, axis=1)                    # the first of equal minima: the smallest index of the chunk
            m = d2[np.arange(len(j)), j]
            take = m < best[qs]                          # an earlier chunk keeps a tie: its indices are smaller
            best[qs] = np.where(take, m, best[qs])
            index[qs] = np.where(take, tidx[t0:t0 + CHUNK][j], index[qs])
    best[~qv] = np.nan
    index[~np.isfinite(best)] = -1
    return dict(dist=np.sqrt(best).astype(np.float32), dist2=best, index=index, dropped_query=int((~qv).sum()),
                dropped_target=int((~tv).sum()))


def assert_same(got, want, what=""):
    """Every output of two searches (NumPy arrays) byte for byte (so NaN equals NaN and +inf equals +inf)."""
    for k in ("dropped_query", "dropped_target"):
        assert int(got[k]) == int(want[k]), (what, k, int(got[k]), int(want[k]))
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, int((g.view(np.uint8) != w.view(np.uint8)).reshape(len(g), -1).any(1).sum()))


def scores_from_counts(out, tau=None):
    """The derived scores from the counts and sums of ``out`` (the same fp64 formulas as score_clouds) -> a new dict."""
    out = dict(out)
    nan = float("nan")
    out["accuracy"] = out["pred_sum"] / out["pred_within"] if out["pred_within"] else nan
    out["completeness"] = out["gt_sum"] / out["gt_within"] if out["gt_within"] else nan
    out["overall"] = (out["accuracy"] + out["completeness"]) / 2
    if tau is not None:
        P = out["precision"] = out["pred_below_tau"] / out["pred_valid"] if out["pred_valid"] else nan
        R = out["recall"] = out["gt_below_tau"] / out["gt_valid"] if out["gt_valid"] else nan
        out["fscore"] = 0.0 if P + R == 0 else 2 * P * R / (P + R)
    return out


def scores_numpy(way_pred, way_gt, max_dist, tau=None):
    """score_clouds from two search results, in NumPy float64 (np.sum: pairwise, another order than the kernels')."""
    out = {}
    md = np.float32(max_dist)
    for name, way in (("pred", way_pred), ("gt", way_gt)):
        d = way["dist"]
        within = d <= md
        out[name + "_valid"], out[name + "_within"] = int((~np.isnan(d)).sum()), int(within.sum())
        out[name + "_sum"] = float(d[within].astype(np.float64).sum())
        if tau is not None:
            out[name + "_below_tau"] = int((d < np.float32(tau)).sum())
    return scores_from_counts(out, tau)


# ---- the host build of mvster_amd/csrc/nn_math.h --------------------------------------------------------------------------

_HM = {}


def load_nn_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/nn_hostmath.cpp like ``voxel_thin_cases.load_voxel_hostmath`` (-ffp-contract=off) with the first
    compiler of `compilers` that exists and load it, once per process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of nn_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libnnhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "nn_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, f = ctypes.c_void_p, ctypes.c_long, ctypes.c_float
    for fn, res in ((h.hm_nn_brute, None), (h.hm_nn_grid, l)):
        fn.restype, fn.argtypes = res, [p, l, p, l, f, f, p, p, p, p]
    h.hm_nn_rings.restype, h.hm_nn_rings.argtypes = ctypes.c_int, [f, f]
    h.hm_nn_cell_ok.restype, h.hm_nn_cell_ok.argtypes = ctypes.c_int, [f, f]
    _HM[compilers] = h
    return h


def nearest_host(h, query, target, max_dist, cell, grid=False):
    """hm_nn_brute / hm_nn_grid -> dict like fusion.nearest_distances (NumPy arrays); with the grid also ``probes``."""
    query = np.ascontiguousarray(query, np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    Q = len(query)
    dist, dist2, index, dropped = np.zeros(Q, np.float32), np.zeros(Q, np.float64), np.zeros(Q, np.int64), np.zeros(2, np.int64)
    fn = h.hm_nn_grid if grid else h.hm_nn_brute
    probes = fn(query.ctypes.data, Q, target.ctypes.data, len(target), max_dist, cell, dist.ctypes.data, dist2.ctypes.data,
                index.ctypes.data, dropped.ctypes.data)
    out = dict(dist=dist, dist2=dist2, index=index, dropped_query=int(dropped[0]), dropped_target=int(dropped[1]))
    if grid:
        out["probes"] = probes
    return out


# ---- the case clouds ---------------------------------------------------------------------------------------------------------

def ring_stop(g, origin):
    """(a) for grid edge g: the query at x = 0.95 g of cell (0, 0, 0); target 0 at distance 1.9 g along (-1, -1, -1), in the
    shell-1 cell (-1, -1, -1); target 1 at x = 2.05 g, in the shell-2 cell (2, 0, 0), at distance 1.1 g: it must win."""
    q = np.array([0.95, 0.5, 0.5]) * g
    far = q - 1.9 * g / np.sqrt(3.0)
    near = np.array([2.05, 0.5, 0.5]) * g
    return q[None] + origin, np.stack([far, near]) + origin


def face_values(cell):
    """Scalars on and next to cell faces on both sides of zero, the zeros, and the tiny negatives whose quotient's fraction rounds
    to 1 (the -1e-30 case of voxel_math.h)."""
    c = np.float32(cell)
    on = np.array([k * np.float64(c) for k in range(-3, 4)]).astype(np.float32)
    return np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf)),
                           np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 0.5 * c, -0.5 * c], np.float32)]).astype(np.float32)


def face_points(cell):
    f = face_values(cell)
    per_axis = [np.where(np.arange(3) == ax, val, np.float32(0.5) * np.float32(cell)) for ax in range(3) for val in f]
    return np.concatenate([np.stack(per_axis), np.repeat(f[:, None], 3, 1)]).astype(np.float32)


def invalid_points(max_dist):
    """Rows that are invalid at every cell of cell_values (NaN, +-inf, 3e38, beyond 2^20 cells of the largest cell) and rows
    that are invalid at the two small cells only (1.5 * 2^20 cells of max_dist / 4: inside 2^20 cells of max_dist)."""
    md = np.float32(max_dist)
    always = [np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 21 * 4 * md, -(2.0 ** 21) * 4 * md]
    sometimes = [1.5 * HALF * md / 4, -1.5 * HALF * md / 4]
    rows = []
    for ax in range(3):
        for b in always + sometimes:
            p = np.array([0.3, -0.7, 1.1], np.float32) * md
            p[ax] = b
            rows.append(p)
    rows.append(np.full(3, np.nan, np.float32))
    return np.stack(rows).astype(np.float32)


def random_cloud(M, v, seed):
    """``random_cloud`` of tests/test_gpu_voxel_thin.py: half of the points crowd into about 150 cells of edge v, the other half
    are mostly alone in theirs; 1 % are NaN."""
    rng = np.random.RandomState(seed)
    scale = np.where(rng.rand(M, 1) < 0.5, 0.1, 1.0) * np.array([30.0, 40.0, 15.0])
    pts = ((rng.rand(M, 3) * 2 - 1) * v * scale).astype(np.float32)
    pts[rng.rand(M) < 0.01] = np.nan
    return pts


_CASES = None


def cases():
    """name -> (query [Q,3] float32, target [M,3] float32, max_dist); built once per process, never modified."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.RandomState(17)
    md, g = MD, np.float64(default_cell(MD))
    out = {}

    def put(name, q, t, max_dist=md):
        out[name] = (np.ascontiguousarray(q, np.float32).reshape(-1, 3), np.ascontiguousarray(t, np.float32).reshape(-1, 3),
                     f32(max_dist))
    # (a) ring stop, at the default cell and at the smallest one (60 max_dist apart: each in its own neighbourhood)
    qa, ta = ring_stop(g, np.zeros(3))
    qb, tb = ring_stop(np.float64(cell_values(md)[0]), np.array([0.0, 60 * md, 0.0]))
    put("ring_stop", np.concatenate([qa, qb]), np.concatenate([ta, tb]))
    # (b) a target exactly at max_dist, and max_dist one float32 below
    t345 = np.array([[3.0, 4.0, 0.0]]) * 2.0 ** -6
    put("at_max_dist", np.zeros((1, 3)), t345, 5 * 2.0 ** -6)
    put("below_max_dist", np.zeros((1, 3)), t345, np.nextafter(np.float32(5 * 2.0 ** -6), np.float32(0)))
    # (c) exact ties.  Query 0 sits on a cell corner with equal targets in different cells, query 1 in the middle of a cell with
    # equal targets inside that cell, query 2 on duplicated targets; a decoy further away comes first in every group
    d = 0.25 * g
    c1, c2 = np.array([8.5, 0.5, 0.5]) * g, np.array([-7.5, 3.5, 0.5]) * g
    ties_t = [[3 * d, 0, 0], [0, 0, -d], [-d, 0, 0], [0, d, 0], [d, 0, 0],                      # query 0: indices 1..4 tie
              c1 + [0, 0, 1.5 * d], c1 + [0, -d, 0], c1 + [d, 0, 0], c1 + [0, 0, d],            # query 1: 6, 7, 8 tie
              c2 + [d, d, 0], c2 + [0.5 * d, 0, 0], c2 + [0.5 * d, 0, 0], c2 + [0.5 * d, 0, 0]]   # query 2: 10, 11, 12 are one point
    put("ties", np.stack([np.zeros(3), c1, c2]), np.array([np.asarray(r, np.float64) for r in ties_t]))
    # (d) points on cell faces of the default and of the smallest cell, tiny negatives
    faces = np.concatenate([face_points(g), face_points(cell_values(md)[0])])
    put("faces", np.concatenate([faces, (rng.rand(100, 3) * 8 - 4) * g]), faces[rng.permutation(len(faces))])
    # (e) invalid points among queries and among targets
    bad = invalid_points(md)
    put("invalid", np.concatenate([bad, (rng.rand(60, 3) * 4 - 2) * md])[rng.permutation(len(bad) + 60)],
        np.concatenate([bad, (rng.rand(80, 3) * 4 - 2) * md])[rng.permutation(len(bad) + 80)])
    put("all_invalid_target", (rng.rand(70, 3) * 4 - 2) * md, np.full((33, 3), np.nan))
    # (f) one cell with 5 000 targets, queries inside and beside it
    base = np.array([2.0, -3.0, 5.0])
    inside = (base + 0.05 + 0.9 * rng.rand(5000, 3)) * g
    q_in, q_by = (base + rng.rand(150, 3)) * g, (base + rng.rand(151, 3) * 3 - 1) * g
    put("one_cell", np.concatenate([q_in, q_by]), np.concatenate([inside, (rng.rand(40, 3) * 6 - 3) * md]))
    # (g) queries far outside the target's bounding box: every shell empty
    put("far_outside", (rng.rand(37, 3) + 50) * md, rng.rand(300, 3) * 2 * md)
    # (h) the smallest sizes, and sizes that are no multiple of 64 or 256
    put("m1", (rng.rand(65, 3) * 2 - 1) * md, np.array([[0.1, 0.2, -0.1]]) * md)
    put("q1", np.array([[0.1, 0.2, -0.1]]) * md, (rng.rand(257, 3) * 2 - 1) * md)
    put("q0", np.zeros((0, 3)), (rng.rand(10, 3) * 2 - 1) * md)
    put("m0", (rng.rand(70, 3) * 2 - 1) * md, np.zeros((0, 3)))
    put("odd", (rng.rand(321, 3) * 4 - 2) * md, (rng.rand(259, 3) * 4 - 2) * md)
    # (i) 20 000 random points, half of them crowded, against a shifted and shuffled copy of which 2 % moved far away
    pts = random_cloud(20000, md, seed=5)
    copy = (pts.astype(np.float64) + np.array([0.1, -0.1, 0.1]) * md).astype(np.float32)
    away = rng.rand(len(copy)) < 0.02
    copy[away] += np.float32(300 * md)
    put("random", pts, copy[rng.permutation(len(copy))])
    _CASES = out
    return out


CASE_NAMES = ("ring_stop", "at_max_dist", "below_max_dist", "ties", "faces", "invalid", "all_invalid_target", "one_cell",
              "far_outside", "m1", "q1", "q0", "m0", "odd", "random")

_HOST = {}


def host_case(name, cell, compilers=("g++",)):
    """The host brute force of a case at one cell, computed once per process and never modified."""
    k = (name, cell)
    if k not in _HOST:
        q, t, md = cases()[name]
        _HOST[k] = nearest_host(load_nn_hostmath(compilers), q, t, md, cell)
    return _HOST[k]


def host_pair(query, target, max_dist, cell, compilers=("g++",)):
    """The host brute force of any pair of clouds."""
    return nearest_host(load_nn_hostmath(compilers), query, target, max_dist, cell)
