"""Shared by tests/test_dynamic_fusion_cpu.py and tests/test_gpu_dynamic_fusion.py (not a test module): dynamic consistency
checking restated in NumPy on the oracle's round trip, the host build of the geo_math.h functions
the dynamic kernel inlines, the scans of tests/fusion_scene_cases.py with the fraction the restatement keeps on each, a scan
whose levels are known in advance, and the comparison with its bounds.

The reference tree has no dynamic filter, so neither yardstick is pinned against it: the restatement follows the
definition operation by operation, the host build is the kernel's own arithmetic compiled for the CPU."""
import ctypes
import os
import subprocess
import shutil
import warnings

import numpy as np

from mvster_amd.synthetic_scene import plane_depth_maps
from oracle import geo_filter_oracle as GO
from tests import fusion_scene_cases as C

CONF_THRES, THRES_VIEW = 0.3, 2
PIX_BASE, REL_BASE = 0.25, 1 / 1300          # the defaults of fusion.fuse_scene(method="dynamic")


# ---- the rule, restated ---------------------------------------------------------------------------------------------------

def dynamic_reference_view(ref_depth, ref_K, ref_E, confidence, src_depths, src_Ks, src_Es, conf_thres, thres_view,
                           pix_base=PIX_BASE, rel_base=REL_BASE, ref_img=None):
    """Dynamic consistency checking for one reference view, on ``reproject_with_depth`` of the oracle and with its dtype
    flow: the reprojection error in float64, the relative depth error and the reprojected depth in float32, the level
    thresholds float32 products n * base.  Source s passes level n iff both errors are below the level's thresholds;
    count_n = sources passing level n; geo_level = the smallest n in thres_view .. L with count_n >= n (0: none); the
    depth is averaged over the sources passing the loosest level max(L, thres_view).  -> the dict of the oracle's
    ``filter_reference_view`` (``geo_mask_sum`` = the count at the loosest level) plus ``geo_level`` and
    ``level_counts`` {n: count_n}."""
    height, width = ref_depth.shape
    L, n0 = len(src_depths), int(thres_view)
    La = max(L, n0)
    pix_base, rel_base = np.float32(pix_base), np.float32(rel_base)
    cols, rows = np.meshgrid(np.arange(0, width), np.arange(0, height))
    photo_mask = confidence > conf_thres
    counts = {n: np.zeros(ref_depth.shape, dtype=np.int32) for n in list(range(n0, L + 1)) + [La]}
    depth_sum = 0
    for d, K, E in zip(src_depths, src_Ks, src_Es):
        depth_back, x_back, y_back, _, _ = GO.reproject_with_depth(ref_depth, ref_K, ref_E, d, K, E)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            pixel_error = np.sqrt((x_back - cols) ** 2 + (y_back - rows) ** 2)          # float32 - int64: float64
            relative_error = np.abs(depth_back - ref_depth) / ref_depth                 # float32
            assert pixel_error.dtype == np.float64 and relative_error.dtype == np.float32

            def passes(n):
                pix, rel = np.float32(n) * pix_base, np.float32(n) * rel_base           # float32 products
                return np.logical_and(pixel_error < np.float64(pix), relative_error < rel)
            for n in counts:
                counts[n] = counts[n] + passes(n).astype(np.int32)
            depth_sum = depth_sum + np.where(passes(La), depth_back, np.float32(0))     # python sum(): 0 + d1 + d2 + ...
    votes = counts[La]
    with np.errstate(invalid="ignore", over="ignore"):
        depth_est_averaged = (depth_sum + ref_depth) / (votes + 1)                      # float32 / int32: float64
    geo_level = np.zeros(ref_depth.shape, dtype=np.uint8)
    for n in range(L, n0 - 1, -1):                                                      # the smallest n wins
        geo_level[counts[n] >= n] = n
    geo_mask = geo_level != 0
    final_mask = np.logical_and(photo_mask, geo_mask)
    sel_x, sel_y, sel_d = cols[final_mask], rows[final_mask], depth_est_averaged[final_mask]
    cam = np.matmul(np.linalg.inv(ref_K), np.vstack((sel_x, sel_y, np.ones_like(sel_x))) * sel_d)
    world = np.matmul(np.linalg.inv(ref_E), np.vstack((cam, np.ones_like(sel_x))))[:3]
    out = dict(photo_mask=photo_mask, geo_mask=geo_mask, final_mask=final_mask, geo_mask_sum=votes, geo_level=geo_level,
               depth_est_averaged=depth_est_averaged, level_counts=counts, points=world.transpose((1, 0)))
    if ref_img is not None:
        out["colors"] = (ref_img[final_mask] * 255).astype(np.uint8)
    return out


def restated_scene(sc, conf_thres=CONF_THRES, thres_view=THRES_VIEW, pix_base=PIX_BASE, rel_base=REL_BASE):
    """The restatement over the scan (float images) -> (per-view results, vertex array)."""
    images = sc["images"]
    if images.dtype == np.uint8:
        images = images.astype(np.float32) / np.float32(255.0)
    views = []
    with warnings.catch_warnings():                  # NaN / inf coordinates cast to integers, as in the oracle
        warnings.simplefilter("ignore", RuntimeWarning)
        for r, srcs in sc["pairs"]:
            views.append(dynamic_reference_view(sc["depths"][r], sc["Ks"][r], sc["Es"][r], sc["conf"][r], sc["depths"][srcs],
                                                sc["Ks"][srcs], sc["Es"][srcs], conf_thres, thres_view, pix_base, rel_base,
                                                ref_img=images[r]))
    return views, GO.vertex_array(views)


# ---- the scans -------------------------------------------------------------------------------------------------------------

# Fraction of the R*H*W pixels THE RESTATEMENT ALONE keeps at conf_thres 0.3, thres_view 2 and the default bases, measured on
# the CPU with restated_scene() and re-checked by tests/test_dynamic_fusion_cpu.py.  Half of it is the non-triviality floor of
# every comparison on that scan.  None = small_scene(), otherwise the HARD_CASES entry of that shape and kind.
KEPT = {
    "small": 0.3226,
    "61x83x5-plain": 0.4012,
    "61x83x5-degenerate": 0.2663,
    "61x83x5-occluder": 0.3406,
    "96x128x7-both": 0.2452,
    "96x128x7-degenerate": 0.2953,
    "5x7x3-plain": 0.2286,
    "37x53x6-perK": 0.4490,
    "9x13x4-degenerate": 0.2393,
    "25x41x5-both": 0.2178,
    "11x93x4-occluder": 0.3216,
    "38x53x5-degenerate": 0.2747,
    "300x3x3-plain": 0.1759,
}
EMPTY_ID = "1x300x3-plain"                           # one row of pixels: keeps nothing at thres_view 2
DYN_CASES = [("small", None, KEPT["small"])] + [(C.hard_id(c), c, KEPT[C.hard_id(c)]) for c in C.HARD_CASES
                                                if C.hard_id(c) != EMPTY_ID]
EMPTY_CASE = [c for c in C.HARD_CASES if C.hard_id(c) == EMPTY_ID][0]
assert len(DYN_CASES) == len(KEPT) == len(C.HARD_CASES)


def dyn_scene(case):
    return C.small_scene() if case is None else C.hard_scene(*case[:4])


_RESTATED = {}


def restated_case(name, case):
    """restated_scene of a DYN_CASES scan at the default parameters, computed once per process and never modified."""
    if name not in _RESTATED:
        _RESTATED[name] = restated_scene(dyn_scene(case))
    return _RESTATED[name]


def staircase_scene(H, W, nsrc, seed=0):
    """One reference view (0) and `nsrc` sources that share its camera.  Pixel p has a target k(p) in 0 .. nsrc: sources
    1 .. k carry the reference depth times 1 + (k - 0.5) * REL_BASE -- the same ray, so the reprojection error is 0 and
    the relative depth error (k - 0.5) * REL_BASE passes level k and no level below --, the other sources carry three times
    the depth and pass no level.  So count_n = k for n >= k and 0 below: at thres_view n0, geo_level = k where k >= n0 and 0
    elsewhere, and geo_mask_sum = k.  Every bin of the level counts up to nsrc is used.  -> (scene, k [H,W])."""
    d, K, E = plane_depth_maps(1, H, W, seed=5)
    rng = np.random.RandomState(900 + seed)
    k = rng.randint(0, nsrc + 1, (H, W))
    k.reshape(-1)[:nsrc + 1] = np.arange(nsrc + 1)                                   # every target at least once
    depths = np.empty((nsrc + 1, H, W), np.float32)
    depths[0] = d[0]
    near = d[0].astype(np.float64) * (1 + (k - 0.5) * REL_BASE)
    for s in range(1, nsrc + 1):
        depths[s] = np.where(s <= k, near, 3.0 * d[0]).astype(np.float32)
    V = nsrc + 1
    return dict(depths=depths, Ks=np.repeat(K, V, 0), Es=np.repeat(E, V, 0), conf=np.ones((V, H, W), np.float32),
                images=rng.randint(0, 256, (V, H, W, 3)).astype(np.uint8), pairs=[(0, list(range(1, V)))]), k


# ---- the host build of the dynamic functions of mvster_amd/csrc/geo_math.h ----------------------------------------------

def load_geo_dyn_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/geo_dyn_hostmath.cpp like ``fusion_scene_cases.load_geo_hostmath`` (-ffp-contract=off) with
    the first compiler of `compilers` that exists and load it.  No compiler is an error, never a skip."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of geo_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libgeodynhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "geo_dyn_hostmath.cpp")])
    h = ctypes.CDLL(so)
    h.hm_geo_scene_dynamic.restype = ctypes.c_long
    h.hm_geo_scene_dynamic.argtypes = ([ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 +
                                       [ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 9)
    return h


HOST_KEYS = ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask", "geo_level", "points", "colors",
             "counts")


def run_host_dynamic(dhm, sc, conf_thres=CONF_THRES, thres_view=THRES_VIEW, pix_base=PIX_BASE, rel_base=REL_BASE, images=None):
    """hm_geo_scene_dynamic over the scan -> dict of NumPy arrays with the keys of fuse_scene(method="dynamic")."""
    from mvster_amd import fusion
    t = fusion.scene_tables(sc["pairs"], sc["Ks"], sc["Es"])
    R, smax = t.pair_table.shape
    V, H, W = sc["depths"].shape
    images = sc["images"] if images is None else images
    if images.dtype == np.uint8:
        images = images.astype(np.float32) / np.float32(255.0)
    out = dict(geo_mask_sum=np.zeros((R, H, W), np.int32), depth_est_averaged=np.zeros((R, H, W), np.float64),
               photo_mask=np.zeros((R, H, W), np.uint8), geo_mask=np.zeros((R, H, W), np.uint8),
               final_mask=np.zeros((R, H, W), np.uint8), geo_level=np.zeros((R, H, W), np.uint8),
               points=np.zeros((R * H * W, 3), np.float32), colors=np.zeros((R * H * W, 3), np.uint8),
               counts=np.zeros(R, np.int64))
    ins = [np.ascontiguousarray(a) for a in (sc["depths"], sc["conf"], images, t.pair_table, t.ref_view, t.ref_mats,
                                             t.view_mats)]
    assert ins[0].dtype == ins[1].dtype == ins[2].dtype == np.float32
    m = dhm.hm_geo_scene_dynamic(*[a.ctypes.data for a in ins], R, smax, V, H, W, conf_thres, thres_view, pix_base, rel_base,
                                 *[out[k].ctypes.data for k in HOST_KEYS])
    assert m >= 0, m
    for k in ("photo_mask", "geo_mask", "final_mask"):
        out[k] = out[k].astype(bool)
    out["points"], out["colors"] = out["points"][:m], out["colors"][:m]
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------

def compare_with_restatement(got, want_views, want_vertices, floor):
    """got: dict of NumPy arrays with the keys of fuse_scene(method="dynamic").  The bounds are the fixed filter's
    (``fusion_scene_cases.compare_with_oracle``): geo_level and geo_mask_sum differ on at most FLIP_FRAC of the pixels (a
    source sitting on a level's threshold), depth_est_averaged within AVG_REL where the counts agree, photo_mask equal,
    world points within one float32 ulp of the cloud's largest coordinate and colours equal where both keep the pixel.
    `floor`: the fraction of the R*H*W pixels both sides must keep.  -> the measured figures."""
    votes = np.stack([w["geo_mask_sum"] for w in want_views])
    level = np.stack([w["geo_level"] for w in want_views])
    R, H, W = votes.shape
    fig = {}
    same_votes = got["geo_mask_sum"] == votes
    fig["vote_sum_mismatch_pixels"] = int((~same_votes).sum())
    fig["level_mismatch_pixels"] = int((got["geo_level"] != level).sum())
    assert got["geo_level"].dtype == np.uint8
    assert fig["vote_sum_mismatch_pixels"] <= C.FLIP_FRAC * R * H * W, fig
    assert fig["level_mismatch_pixels"] <= C.FLIP_FRAC * R * H * W, fig
    avg = np.stack([w["depth_est_averaged"] for w in want_views])
    fig["avg_nonfinite_pixels"] = int((~np.isfinite(avg)).sum())
    fig["avg_rel_max"] = C.assert_same_values(got["depth_est_averaged"][same_votes], avg[same_votes], C.AVG_REL)
    assert np.array_equal(got["photo_mask"], np.stack([w["photo_mask"] for w in want_views]))
    final = np.stack([w["final_mask"] for w in want_views])
    agree = got["final_mask"] & final
    fig["final_mask_mismatch_pixels"] = int((got["final_mask"] != final).sum())
    assert fig["final_mask_mismatch_pixels"] <= fig["level_mismatch_pixels"]
    assert np.array_equal(got["geo_mask"], got["geo_level"] != 0)
    assert np.array_equal(got["final_mask"], got["photo_mask"] & got["geo_mask"])
    assert (got["geo_level"] <= got["geo_mask_sum"])[got["geo_mask"]].all()      # level n needs n sources, all counted
    assert np.array_equal(got["counts"], got["final_mask"].reshape(R, -1).sum(1)) and got["counts"].sum() == len(got["points"])
    same_mask_views = (got["final_mask"] == final).reshape(R, -1).all(1)
    assert np.array_equal(got["counts"][same_mask_views], final.reshape(R, -1).sum(1)[same_mask_views])
    fig["points"], fig["restated_points"] = int(len(got["points"])), int(len(want_vertices))
    fig["levels"] = {int(n): int((level == n).sum()) for n in np.unique(level)}
    fig["kept_frac"], fig["kept_floor"] = float(final.mean()), float(floor)
    assert agree.sum() > floor * R * H * W, fig                              # neither empty nor trivial
    want_xyz = np.stack([want_vertices[c] for c in "xyz"], 1)
    want_rgb = np.stack([want_vertices[c] for c in ("red", "green", "blue")], 1)
    assert got["points"].dtype == np.float32 and got["colors"].dtype == np.uint8
    g = C.scatter(got["final_mask"], got["points"]).astype(np.float64)[agree]
    w = C.scatter(final, want_xyz)[agree].astype(np.float64)
    ok = np.isfinite(w)
    assert np.array_equal(np.isfinite(g), ok) and np.array_equal(g[~ok], w[~ok], equal_nan=True)
    ulp = float(np.spacing(np.float32(np.abs(w[ok]).max())))
    fig["xyz_abs_max"], fig["xyz_bound_one_ulp"] = float(np.abs(g[ok] - w[ok]).max()), ulp
    assert fig["xyz_abs_max"] <= ulp, fig
    assert np.array_equal(C.scatter(got["final_mask"], got["colors"])[agree], C.scatter(final, want_rgb)[agree])
    return fig
