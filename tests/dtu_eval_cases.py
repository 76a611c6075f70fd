"""Shared by tests/test_dtu_eval_cpu.py and tests/test_gpu_dtu_eval.py (not a test module): the DTU evaluation protocol
 restated in NumPy from the .m files of the reference's evaluations/dtu/, the host build of
mvster_amd/csrc/eval_math.h, and the cases.

The restatement is the reference here (MATLAB cannot be run): reducePts_haa.m as its serial loop in priority order over a brute
force range search in float64, PointCompareMain.m's mask lookup with MATLAB's round, the plane, MaxDistCP.m's block cover and
ComputeStat_func.m's statistics over np.sort.  The nearest distances inside a whole-scan case come from the host brute force of
nn_math.h (tests/cloud_nn_cases.py), which the tests of section 4.17 hold to their own NumPy restatement."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from tests import cloud_nn_cases as N
from tests import fusion_scene_cases as C

DST = 0.2
MAX_DIST = 20.0
MAX_BLOCK = 60.0
IN_MASK, ABOVE_PLANE, COVERED = 1, 2, 4


def f32(x):
    return float(np.float32(x))


# ---- the .m files, restated -----------------------------------------------------------------------------------------------

def splitmix64_numpy(i, seed):
    """key_i of the hashed priority, in uint64 arrays (which wrap modulo 2^64)."""
    c = lambda v: np.array([v & (2 ** 64 - 1)], np.uint64)
    z = np.atleast_1d(np.asarray(i)).astype(np.uint64) + c((seed + 1) * 0x9E3779B97F4A7C15)
    z = (z ^ (z >> c(30))) * c(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> c(27))) * c(0x94D049BB133111EB)
    return z ^ (z >> c(31))


def reduce_numpy(points, dst, priority=None, seed=0):
    """reducePts_haa.m: in priority order, a point that is still set clears every point within dst (inclusive) and stays set.
    -> (keep [M] bool, the invalid points)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    M = len(pts)
    valid = N.valid_points(pts, dst)
    key = splitmix64_numpy(np.arange(M), seed) if priority is None else np.asarray(priority, np.int64)
    order = np.lexsort((np.arange(M), key)) if M else np.zeros(0, np.int64)
    keep = valid.copy()
    vidx = np.nonzero(valid)[0]
    pv = pts[vidx].astype(np.float64)
    d = np.float64(np.float32(dst))
    reach = d * d
    for i in order:
        if not keep[i]:
            continue
        dx, dy, dz = (pts[i, j].astype(np.float64) - pv[:, j] for j in range(3))
        keep[vidx[(dx * dx + dy * dy) + dz * dz <= reach]] = False
        keep[i] = True
    return keep, int((~valid).sum())


def mround_numpy(x):
    """MATLAB's round, halves away from zero, without adding 0.5: the fraction x - trunc(x) is exact."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        return np.where(np.abs(x - t) >= 0.5, t + np.sign(x), t)


def in_obs_mask_numpy(points, mask, bb, res):
    p = np.asarray(points, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = mround_numpy((p - np.asarray(bb, np.float64)[0]) / np.float64(res) + 1.0)
        S = np.array(mask.shape, np.float64)
        inside = ((v >= 1) & (v <= S)).all(1)
    out = np.zeros(len(p), bool)
    vi = v[inside].astype(np.int64) - 1
    out[inside] = np.asarray(mask)[vi[:, 0], vi[:, 1], vi[:, 2]] != 0
    return out


def above_plane_numpy(points, plane):
    p = np.asarray(points, np.float32).astype(np.float64)
    P = np.asarray(plane, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0


def covered_numpy(points, bb, max_block=MAX_BLOCK):
    p = np.asarray(points, np.float32).astype(np.float64)
    bb = np.asarray(bb, np.float64)
    hi = bb[0] + (np.floor((bb[1] - bb[0]) / max_block) + 1.0) * max_block
    with np.errstate(invalid="ignore"):
        return ((p >= bb[0]) & (p < hi)).all(1)


def stats_numpy(dist2, select, max_dist):
    """ComputeStat_func.m for one direction -> dict n, mean, var, median (np.sum / np.sort: another order than the kernels')."""
    dist2 = np.asarray(dist2, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(dist2)
        sel = (np.asarray(select) != 0) & np.isfinite(dist2) & (d < np.float64(np.float32(max_dist)))
    s = np.sort(d[sel])
    n = len(s)
    nan = float("nan")
    if n == 0:
        return dict(n=0, mean=nan, var=nan, median=nan)
    mean = float(s.sum() / n)
    var = float(((s - mean) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    return dict(n=n, mean=mean, var=var, median=float((s[(n - 1) // 2] + s[n // 2]) / 2))


def evaluate_numpy(pred, scan, dst=DST, seed=0, priority=None, reduce=True):
    """PointCompareMain.m + one column of ComputeStat_func.m -> the dict of dtu_eval.evaluate_dtu_scan(return_points=True),
    NumPy arrays for the per-point entries."""
    pred = np.asarray(pred, np.float32).reshape(-1, 3)
    md, cell = f32(scan["max_dist"]), N.default_cell(scan["max_dist"])
    if reduce:
        keep, dropped = reduce_numpy(pred, dst, priority, seed)
    else:
        keep, dropped = np.ones(len(pred), bool), 0
    index = np.nonzero(keep)[0]
    q, stl = pred[index], scan["stl_points"]
    data, back = N.host_pair(q, stl, md, cell), N.host_pair(stl, q, md, cell)
    in_mask = in_obs_mask_numpy(q, scan["obs_mask"], scan["bb"], scan["res"])
    above = above_plane_numpy(stl, scan["plane"])
    sd = stats_numpy(data["dist2"], in_mask & covered_numpy(q, scan["bb"]), md)
    ss = stats_numpy(back["dist2"], above & covered_numpy(stl, scan["bb"]), md)
    out = dict(n_data=sd["n"], mean_data=sd["mean"], var_data=sd["var"], med_data=sd["median"], n_stl=ss["n"], mean_stl=ss["mean"],
               var_stl=ss["var"], med_stl=ss["median"], overall=(sd["mean"] + ss["mean"]) / 2, points_in=len(pred),
               points_reduced=len(q), downsample_factor=len(pred) / len(q) if len(q) else float("nan"),
               data_in_mask=int(in_mask.sum()), stl_above_plane=int(above.sum()), dropped_invalid=dropped,
               dropped_reduced=data["dropped_query"], dropped_stl=data["dropped_target"])
    with np.errstate(invalid="ignore"):
        out.update(Qdata_index=index.astype(np.int64), Qdata=q, Ddata=np.sqrt(data["dist2"]), DataInMask=in_mask,
                   Dstl=np.sqrt(back["dist2"]), StlAbovePlane=above)
    return out


COUNT_KEYS = ("n_data", "n_stl", "points_in", "points_reduced", "data_in_mask", "stl_above_plane", "dropped_invalid",
              "dropped_reduced", "dropped_stl")
EXACT_KEYS = ("med_data", "med_stl", "downsample_factor")
CLOSE_KEYS = ("mean_data", "var_data", "mean_stl", "var_stl", "overall")
POINT_KEYS = ("Qdata_index", "Qdata", "Ddata", "DataInMask", "Dstl", "StlAbovePlane")
REL = 1e-12                                # the project's bound for an fp64 sum against NumPy's


def same_float(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b))


def close_float(a, b, rel=REL):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rel * abs(b)


def assert_stats(got, want, what=""):
    assert got["n"] == want["n"], (what, got, want)
    assert same_float(got["median"], want["median"]), (what, got, want)
    assert close_float(got["mean"], want["mean"]) and close_float(got["var"], want["var"]), (what, got, want)


def assert_scan(got, want, what="", points=True):
    for k in COUNT_KEYS:
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in EXACT_KEYS:
        assert same_float(got[k], want[k]), (what, k, got[k], want[k])
    for k in CLOSE_KEYS:
        assert close_float(got[k], want[k]), (what, k, got[k], want[k])
    if points:
        for k in POINT_KEYS:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (what, k)


# ---- the host build of mvster_amd/csrc/eval_math.h -----------------------------------------------------------------------------

_HM = {}


def load_eval_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/eval_hostmath.cpp like ``cloud_nn_cases.load_nn_hostmath`` and load it, once per process.  No
    compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of eval_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libevalhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "eval_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, f, i = ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int
    h.hm_eval_reduce_serial.restype, h.hm_eval_reduce_serial.argtypes = l, [p, l, f, p, l, p]
    h.hm_eval_reduce_rounds.restype, h.hm_eval_reduce_rounds.argtypes = l, [p, l, f, p, l, i, p]
    h.hm_eval_flags.restype, h.hm_eval_flags.argtypes = None, [p, l, p, p, p, i, p]
    h.hm_eval_stats.restype, h.hm_eval_stats.argtypes = None, [p, p, l, i, f, p]
    h.hm_eval_splitmix64.restype, h.hm_eval_splitmix64.argtypes = ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]
    h.hm_eval_mround.restype, h.hm_eval_mround.argtypes = ctypes.c_double, [ctypes.c_double]
    _HM[compilers] = h
    return h


def reduce_host(h, points, dst, priority=None, seed=0, rounds=0):
    """hm_eval_reduce_serial, or with rounds = 1 / 2 hm_eval_reduce_rounds at that cell factor -> (keep [M] bool, invalid points
    / rounds)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    keep = np.zeros(len(pts), np.uint8)
    prio = None if priority is None else np.ascontiguousarray(priority, np.int64)
    args = (pts.ctypes.data, len(pts), dst, None if prio is None else prio.ctypes.data, seed)
    r = h.hm_eval_reduce_rounds(*args, rounds, keep.ctypes.data) if rounds else h.hm_eval_reduce_serial(*args, keep.ctypes.data)
    return keep.astype(bool), r


def scan_params(scan):
    return np.concatenate([np.asarray(scan["bb"], np.float64).reshape(-1), [scan["res"], MAX_BLOCK],
                           np.asarray(scan["plane"], np.float64).reshape(-1)]).astype(np.float64)


def flags_host(h, points, scan, which=7):
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    mask = np.ascontiguousarray(scan["obs_mask"], np.uint8)
    S, params = np.array(mask.shape, np.int64), scan_params(scan)
    flags = np.zeros(len(pts), np.uint8)
    h.hm_eval_flags(pts.ctypes.data, len(pts), mask.ctypes.data, S.ctypes.data, params.ctypes.data, which, flags.ctypes.data)
    return flags


def flags_numpy(points, scan):
    return (in_obs_mask_numpy(points, scan["obs_mask"], scan["bb"], scan["res"]) * IN_MASK +
            above_plane_numpy(points, scan["plane"]) * ABOVE_PLANE + covered_numpy(points, scan["bb"]) * COVERED).astype(np.uint8)


def stats_host(h, dist2, select, max_dist):
    dist2 = np.ascontiguousarray(dist2, np.float64)
    sel = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
    out = np.zeros(4, np.float64)
    h.hm_eval_stats(dist2.ctypes.data, sel.ctypes.data, len(dist2), 1, max_dist, out.ctypes.data)
    return dict(n=int(out[0]), mean=float(out[1]), var=float(out[2]), median=float(out[3]))


# ---- the reduction cases: name -> dict(points, dst, priority, seed) ---------------------------------------------------------------

def surface(n, seed, x=20.0, y=10.0, noise=0.02):
    """n noisy points on a wavy surface over [0, x] x [0, y] (mm): 100 / mm^2 at the default sizes and n = 20 000."""
    rng = np.random.RandomState(seed)
    u, v = rng.rand(n) * x, rng.rand(n) * y
    z = 0.5 * np.sin(u) * np.cos(0.7 * v) + noise * rng.randn(n)
    return np.stack([u, v, z], 1).astype(np.float32)


NEIGHBOUR_DIRECTIONS = ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [1, -1, 1])
SHELL2_ROWS = 64                                        # where the three shell-2 pairs of neighbour_points begin


def neighbour_pairs(dst, factor):
    """The threshold pairs of (e) for the grid of cell factor * dst: -> (rows [64,3] float64, meta).  Pair k is rows 2k and
    2k + 1, placed symmetrically about a corner of that grid (a multiple of factor * dst on all three axes, on either side of
    the origin) along a direction with 1, 2 or 3 non-zero components, so that it straddles a face, an edge or a corner of
    the cells, at 0.99 or 1.01 dst; every pair is alone in its neighbourhood.  meta[k] = (direction, scale)."""
    d = np.float64(np.float32(dst))
    rows, meta = [], []
    for direction in NEIGHBOUR_DIRECTIONS:
        u = np.asarray(direction, np.float64) / np.linalg.norm(direction)
        for scale in (0.99, 1.01):
            for sign in (1, -1):
                n = len(meta)
                corner = sign * (np.array([40.0 + 10 * n, 7.0, 3.0]) if factor == 1 else np.array([60.0 + 12 * n, 32.0, 4.0])) * d
                rows += [corner - 0.5 * scale * d * u, corner + 0.5 * scale * d * u]
                meta.append((direction, scale))
    return np.asarray(rows), meta


def axes_crossed(points, dst, factor):
    """For consecutive pairs of rows: on how many axes their cells of edge factor * dst differ (vox::point_key's floor)."""
    cell = np.float64(np.float32(factor) * np.float32(dst))
    c = np.floor(np.asarray(points, np.float32).astype(np.float64) / cell)
    return (c[0::2] != c[1::2]).sum(1)


def neighbour_points(dst):
    """(e): the threshold pairs of neighbour_pairs for the cells of edge dst (rows 0 .. 63) and, behind the shell-2 pairs, for
    the cells of edge 2 dst, the default grid (rows 70 .. 133: their corners are corners of both grids); rows 64 .. 69 the
    pair (-1e-30, dst) on each axis, whose cells of edge dst differ by 2 while within dst; the zeros and +-1e-30; and the
    points on and next to cell faces of cloud_nn_cases.face_points at both cell sizes."""
    d = np.float64(np.float32(dst))
    shell2 = []
    for ax in range(3):                                 # cells -1 and 1 on one axis, exactly dst apart after rounding
        a, b = np.array([0.25, 0.25, 0.25]) * d + 20 * d * (ax + 1), np.array([0.25, 0.25, 0.25]) * d + 20 * d * (ax + 1)
        a[ax], b[ax] = -1e-30, d
        shell2 += [a, b]
    tiny = [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1e-30, 1e-30, 1e-30], [-1e-30, -1e-30, -1e-30], [-1e-30, 0.0, 1e-30]]
    return np.concatenate([neighbour_pairs(dst, 1)[0], np.asarray(shell2), neighbour_pairs(dst, 2)[0], np.asarray(tiny),
                           N.face_points(f32(dst)).astype(np.float64) + [0, 0, 100 * d],
                           N.face_points(f32(2 * f32(dst))).astype(np.float64) + [0, 0, 200 * d]]).astype(np.float32)


_REDUCE = None


def reduce_cases():
    global _REDUCE
    if _REDUCE is not None:
        return _REDUCE
    rng = np.random.RandomState(23)
    out = {}

    def put(name, points, dst=DST, priority=None, seed=0):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out[name] = dict(points=pts, dst=f32(dst), priority=None if priority is None else np.ascontiguousarray(priority, np.int64),
                         seed=seed)
    # (a) 300 points on a line, 0.6 dst apart
    line = np.stack([np.arange(300) * 0.6 * 0.25, np.full(300, 0.1), np.full(300, -0.3)], 1)
    put("line_arange", line, 0.25, np.arange(300))
    put("line_hash", line, 0.25)
    # (b) a pair exactly dst apart, and dst one float32 below
    pair = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]]) * 2.0 ** -6
    put("pair_at", pair, 5 * 2.0 ** -6, [0, 1])
    put("pair_below", pair, np.nextafter(np.float32(5 * 2.0 ** -6), np.float32(0)), [0, 1])
    # (c) A - B and B - C within dst, A - C not
    put("chain", np.array([[0.0, 0, 0], [0.8, 0, 0], [1.6, 0, 0]]) * DST, DST, [0, 1, 2])
    # (d) ten duplicates and priority ties: index 1 is the smallest (key, index)
    put("duplicates", np.tile([[0.3, -0.2, 0.7]], (10, 1)), DST, [5, 3, 3, 7, 3, 9, 4, 3, 8, 6])
    # (e) neighbours across faces, edges and corners; zeros and tiny values; the shell-2 pair
    nb = neighbour_points(DST)
    put("neighbours", nb)
    put("neighbours_perm", nb, DST, rng.permutation(len(nb)))
    # (f) invalid points (each twice, so an invalid point has a neighbour at distance 0) among valid ones
    bad = N.invalid_points(DST)
    good = (rng.rand(200, 3) * 4 - 2) * DST
    mixed = np.concatenate([bad, bad, good, np.array([[0.3, -0.7, 1.1]]) * DST])
    put("invalid", mixed[rng.permutation(len(mixed))])
    put("all_invalid", np.full((70, 3), np.nan))
    # (g) 5 000 points inside a ball of diameter dst, 5 000 more within 3 dst
    u = rng.randn(5000, 3)
    ball = u / np.linalg.norm(u, axis=1, keepdims=True) * (0.4995 * DST * rng.rand(5000, 1) ** (1 / 3)) + [1.0, 2.0, 3.0]
    put("ball", ball)
    put("ball_and_more", np.concatenate([ball, [50.0, 2.0, 3.0] + rng.rand(5000, 3) * 3 * DST]))
    # (h) the smallest sizes and one that is no multiple of 64
    put("m0", np.zeros((0, 3)))
    put("m1", [[0.1, 0.2, 0.3]])
    put("m2", [[0.1, 0.2, 0.3], [0.15, 0.2, 0.3]])
    put("m321", rng.rand(321, 3) * 6 * DST)
    # (i) 20 000 noisy points on a wavy surface at 100 / mm^2
    surf = surface(20000, seed=3)
    put("surface_seed0", surf)
    put("surface_seed7", surf, seed=7)
    put("surface_perm", surf, DST, rng.permutation(20000))
    put("surface_16keys", surf, DST, rng.randint(-8, 8, 20000))
    _REDUCE = out
    return out


REDUCE_NAMES = ("line_arange", "line_hash", "pair_at", "pair_below", "chain", "duplicates", "neighbours", "neighbours_perm",
                "invalid", "all_invalid", "ball", "ball_and_more", "m0", "m1", "m2", "m321", "surface_seed0", "surface_seed7",
                "surface_perm", "surface_16keys")

_SERIAL = {}


def reduce_expected(name, compilers=("g++",)):
    """The host's serial loop on a case -> (keep, invalid points); computed once per process and never modified."""
    if name not in _SERIAL:
        c = reduce_cases()[name]
        _SERIAL[name] = reduce_host(load_eval_hostmath(compilers), c["points"], c["dst"], c["priority"], c["seed"])
    return _SERIAL[name]


# ---- mask, plane and cover cases -------------------------------------------------------------------------------------------------

def mask_scan():
    """(j), (k), (l): a 5 x 4 x 3 mask with a known pattern, Res and BB powers of two (every quotient exact) -> (scan, points,
    names of the points)."""
    mask = np.zeros((5, 4, 3), np.uint8)
    mask[0, 0, 0] = mask[2, 1, 1] = mask[4, 3, 2] = mask[1, :, 0] = 1
    bb = np.array([[-2.0, 1.0, 4.0], [126.0, 65.0, 36.0]])          # BB2 - BB1 = 128, 64, 32: 3, 2, 1 blocks of 60
    res, plane = 0.5, np.array([0.5, -0.25, 1.0, -2.0])
    scan = dict(obs_mask=mask, bb=bb, res=res, plane=plane, max_dist=MAX_DIST)
    at = lambda v: bb[0] + (np.asarray(v, np.float64) - 1) * res      # voxel coordinates (1-based, fractional) -> a point
    dn = lambda p: np.nextafter(np.asarray(p, np.float32), np.float32(-np.inf))
    up = lambda p: np.nextafter(np.asarray(p, np.float32), np.float32(np.inf))
    pts, names = [], []

    def put(name, p):
        names.append(name)
        pts.append(np.asarray(p, np.float32))
    put("voxel_1_1_1", at([1, 1, 1]))                                  # set
    put("voxel_0.5_rounds_to_1", at([0.5, 1, 1]))                      # half a voxel below BB1: in the mask, not covered
    put("below_0.5_rounds_to_0", dn(at([0.5, 1, 1])) * [1, 0, 0] + at([0.5, 1, 1]) * [0, 1, 1])
    put("voxel_2.5_rounds_to_3", at([2.5, 2, 2]))                      # (3, 2, 2): set
    put("voxel_2.49_rounds_to_2", at([2.49, 2, 2]))                    # (2, 2, 2): clear ... (2, :, 1) is set only at z index 0
    put("voxel_2_3_1", at([2, 3, 1]))                                  # set by mask[1, :, 0]
    put("voxel_S+0.5_outside", at([5.5, 4, 3]))
    put("voxel_S_set", at([5, 4, 3]))
    put("voxel_S+0.49_inside", at([5.49, 4, 3]))
    put("voxel_-0.5_outside", at([-0.5, 1, 1]))
    put("voxel_1_0.5_0.5", at([1, 0.5, 0.5]))                          # in the mask through two roundings, not covered
    put("nan", [np.nan, 1.0, 4.0])
    put("inf", [np.inf, 1.0, 4.0])
    # (k) the plane: 0.5 x - 0.25 y + z - 2 = 0
    on = np.array([3.0, 2.0, 1.0])
    put("on_plane", on)
    put("above_plane", up(on) * [0, 0, 1] + on * [1, 1, 0])
    put("below_plane", dn(on) * [0, 0, 1] + on * [1, 1, 0])
    # (l) the cover: [BB1, BB1 + (180, 120, 60))
    hi = bb[0] + [180.0, 120.0, 60.0]
    put("at_bb1", bb[0])
    put("below_bb1", dn(bb[0]) * [0, 1, 0] + bb[0] * [1, 0, 1])
    put("at_bb2", bb[1])
    put("at_cover_end", hi)
    for ax in range(3):
        p = bb[0] + [1.0, 1.0, 1.0]
        p[ax] = hi[ax]
        put("cover_end_axis%d" % ax, p)
        put("below_cover_end_axis%d" % ax, dn(p) * np.eye(3)[ax] + p * (1 - np.eye(3)[ax]))
    return scan, np.stack(pts).astype(np.float32), names


# expected (in_obs_mask, above_plane is left to the restatement, covered) of the named points of mask_scan, by hand
MASK_BY_HAND = {"voxel_1_1_1": (True, True), "voxel_0.5_rounds_to_1": (True, False), "below_0.5_rounds_to_0": (False, False),
                "voxel_2.5_rounds_to_3": (True, True), "voxel_2.49_rounds_to_2": (False, True), "voxel_2_3_1": (True, True),
                "voxel_S+0.5_outside": (False, True), "voxel_S_set": (True, True), "voxel_S+0.49_inside": (True, True),
                "voxel_-0.5_outside": (False, False), "voxel_1_0.5_0.5": (True, False), "nan": (False, False), "inf": (False, False),
                "at_bb1": (True, True), "below_bb1": (True, False), "at_bb2": (False, True), "at_cover_end": (False, False)}


# ---- statistics cases: name -> (dist2, select, max_dist) ---------------------------------------------------------------------------

def stats_cases():
    rng = np.random.RandomState(31)
    out = {}
    for n in (0, 1, 2, 3, 1000, 1001):
        d = rng.rand(n) * 25.0                                          # some beyond max_dist
        out["n%d" % n] = (d * d, np.ones(n, bool), MAX_DIST)
    out["nothing_selected"] = (rng.rand(300), np.zeros(300, bool), MAX_DIST)
    out["ties"] = (np.full(1000, 2.25), np.ones(1000, bool), MAX_DIST)
    mixed = np.concatenate([np.full(300, 0.01), np.full(401, 4.0), rng.rand(77)])
    out["ties_in_the_middle"] = (mixed[rng.permutation(len(mixed))], np.ones(len(mixed), bool), MAX_DIST)
    d2 = np.concatenate([[12.0 ** 2 + 16.0 ** 2], rng.rand(50) * 399.0, [np.inf, np.nan, np.inf], [0.0, 0.0]])
    out["at_max_dist_inf_nan"] = (d2, np.ones(len(d2), bool), MAX_DIST)
    d = rng.rand(9000) * 22.0
    out["half_selected"] = (d * d, rng.rand(9000) < 0.5, MAX_DIST)
    return out


STATS_NAMES = ("n0", "n1", "n2", "n3", "n1000", "n1001", "nothing_selected", "ties", "ties_in_the_middle", "at_max_dist_inf_nan",
               "half_selected")


# ---- whole scans -----------------------------------------------------------------------------------------------------------------

def synthetic_scan(seed, nx=150, ny=100, npred=20000):
    """(n): the ground truth is nx x ny surface points 0.2 apart over [0, 0.2 nx] x [0, 0.2 ny]; the prediction npred denser
    noisy points on the same surface plus 2 % outliers 30 .. 100 away; the mask volume starts 2 mm inside the surface in x and 1 mm in y (so the
    block cover cuts ground truth off, too), has a cylindrical hole and ends in a margin; the plane x > 0.02 nx cuts off a tenth of the
    ground truth.  -> (scan dict, pred [npred,3] float32)."""
    rng = np.random.RandomState(seed)
    X, Y = 0.2 * nx, 0.2 * ny
    gx, gy = np.meshgrid(np.arange(nx) * 0.2, np.arange(ny) * 0.2, indexing="ij")
    wave = lambda u, v: 0.5 * np.sin(u) * np.cos(0.7 * v)
    stl = np.stack([gx.ravel(), gy.ravel(), wave(gx, gy).ravel()], 1).astype(np.float32)
    u, v = rng.rand(npred) * X, rng.rand(npred) * Y
    pred = np.stack([u, v, wave(u, v) + 0.05 * rng.randn(npred)], 1)
    far = rng.rand(npred) < 0.02
    w = rng.randn(npred, 3)
    pred[far] += (w / np.linalg.norm(w, axis=1, keepdims=True) * (30 + 70 * rng.rand(npred, 1)))[far]
    res = 0.25
    bb1 = np.array([2.0, 1.0, -4.0])
    S = (int((X - 4.0) / res) + 1, int(Y / res) + 1, 33)
    bb = np.stack([bb1, bb1 + (np.array(S) - 1) * res])
    ii, jj = np.meshgrid(np.arange(S[0]), np.arange(S[1]), indexing="ij")
    hole = (bb1[0] + ii * res - 0.5 * X) ** 2 + (bb1[1] + jj * res - 0.5 * Y) ** 2 < 9.0
    mask = np.repeat((~hole)[:, :, None], S[2], 2).astype(np.uint8)
    mask[:, :, :4] = 0                                                   # nothing observable at the bottom of the volume
    scan = dict(stl_points=stl, obs_mask=mask, bb=bb, res=res, plane=np.array([1.0, 0.0, 0.0, -0.02 * nx]), max_dist=MAX_DIST)
    return scan, pred.astype(np.float32)


_SCANS = {}


def scan_case(name):
    """"scan" (n), and "file1" / "file4" (o, smaller) -> (scan, pred, evaluate_numpy's dict); once per process, never modified."""
    if name not in _SCANS:
        scan, pred = dict(scan=lambda: synthetic_scan(41), file1=lambda: synthetic_scan(42, 90, 60, 8000),
                          file4=lambda: synthetic_scan(43, 80, 70, 7000))[name]()
        _SCANS[name] = (scan, pred, evaluate_numpy(pred, scan))
    return _SCANS[name]


def write_scan_files(data_path, ply_dir, number, scan, pred, drop=()):
    """The files of one scan as DTU lays them out: the stl PLY with normals and colours, the two .mat files (scipy.io.savemat),
    and the prediction as {ply_dir}/mvsnet%03d_l3.ply in the project's own layout."""
    from scipy.io import savemat
    from mvster_amd import fusion
    os.makedirs(os.path.join(data_path, "Points", "stl"), exist_ok=True)
    os.makedirs(os.path.join(data_path, "ObsMask"), exist_ok=True)
    os.makedirs(ply_dir, exist_ok=True)
    stl = scan["stl_points"]
    write_rich_ply(os.path.join(data_path, "Points", "stl", "stl%03d_total.ply" % number), stl)
    m = dict(ObsMask=scan["obs_mask"].astype(bool), BB=scan["bb"], Res=np.float64(scan["res"]))
    savemat(os.path.join(data_path, "ObsMask", "ObsMask%d_10.mat" % number), {k: v for k, v in m.items() if k not in drop})
    savemat(os.path.join(data_path, "ObsMask", "Plane%d.mat" % number), dict(P=scan["plane"].reshape(4, 1)))
    v = np.zeros(len(pred), fusion.PLY_VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = pred[:, 0], pred[:, 1], pred[:, 2]
    fusion.write_ply(os.path.join(ply_dir, "mvsnet%03d_l3.ply" % number), v)


def write_rich_ply(filename, points, double_xyz=False, faces=False, crlf=False):
    """A binary little-endian PLY whose vertex element carries normals, colours and a double besides x, y, z (which sit in the
    middle of the record), optionally x, y, z as doubles, a face element behind, and header lines that end in CR LF."""
    t = "<f8" if double_xyz else "<f4"
    dt = np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("x", t), ("red", "u1"), ("y", t), ("green", "u1"), ("z", t),
                   ("blue", "u1"), ("quality", "<f8"), ("label", "<i2")])
    names = {"<f4": "float", "<f8": "double", "u1": "uchar", "|u1": "uchar", "<i2": "short"}
    v = np.zeros(len(points), dt)
    v["x"], v["y"], v["z"] = points[:, 0], points[:, 1], points[:, 2]
    v["nz"], v["red"], v["quality"], v["label"] = 1.0, 200, 0.5, -3
    head = "ply\nformat binary_little_endian 1.0\ncomment made by the tests\nelement vertex %d\n" % len(v)
    head += "".join("property %s %s\n" % (names[dt[k].str], k) for k in dt.names)
    tail = b""
    if faces:
        head += "element face 1\nproperty list uchar int vertex_indices\n"
        tail = bytes([3]) + np.array([0, 1, 2], "<i4").tobytes()
    with open(filename, "wb") as f:
        f.write((head + "end_header\n").replace("\n", "\r\n" if crlf else "\n").encode("ascii"))
        f.write(v.tobytes() + tail)
