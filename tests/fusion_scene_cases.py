"""Shared by tests/test_fusion_scene_cpu.py and tests/test_gpu_fusion_scene.py: the small scan both check against the
oracle, the hard scans (odd sizes, degenerate depths, an occluder, per-view intrinsics), the scans whose survivors are
known in advance, the oracle run over a scan, the host build of geo_math.h, and the comparison with its bounds (not a
test module)."""
import ctypes
import os
import shutil
import subprocess
import warnings

import numpy as np

from mvster_amd.synthetic_scene import plane_depth_maps
from oracle import geo_filter_oracle as GO

CONF_THRES, THRES_VIEW = 0.3, 2
FLIP_FRAC = 2e-4        # tests/test_gpu_fusion.py: only pixel-views sitting on a threshold may vote differently
AVG_REL = 1e-6          # tests/test_gpu_fusion.py: reprojected / averaged depth where the votes agree


def make_pairs(nviews, lo, hi, seed, refs=None):
    """Every view of `refs` (default: all) as a reference view with lo..hi source views in a shuffled order."""
    rng = np.random.RandomState(seed)
    pairs = []
    for r in (range(nviews) if refs is None else refs):
        others = [v for v in range(nviews) if v != r]
        rng.shuffle(others)
        pairs.append((r, others[:rng.randint(lo, hi + 1)]))
    return pairs


def small_scene():
    """7 views of 96 x 128 with noise and outliers, 3 to 5 source views each, random confidence and float images."""
    depths, Ks, Es = plane_depth_maps(7, 96, 128, seed=5, noise=2e-3, outlier_frac=0.05)
    rng = np.random.RandomState(11)
    conf = rng.rand(*depths.shape).astype(np.float32)
    images = rng.rand(*depths.shape, 3).astype(np.float32)
    return dict(depths=depths, Ks=Ks, Es=Es, conf=conf, images=images, pairs=make_pairs(7, 3, 5, seed=2))


HARD_KINDS = ("plain", "degenerate", "occluder", "both", "perK")

# (H, W, V, kind, {thres_view: fraction of the R*H*W pixels the ORACLE ALONE keeps at conf_thres 0.3}).  The fractions
# were measured once on the CPU with oracle_scene() and are re-checked by tests/test_fusion_scene_cpu.py; half of one
# is the non-triviality floor of every comparison of that case, so no case can pass by keeping nothing.  A thres_view
# that is missing keeps (almost) nothing on that shape and is not run.  What each size is there for:
HARD_CASES = [
    (61, 83, 5, "plain", {1: 0.6149, 2: 0.5227}),          # 5063 = 19 * 256 + 199: odd width and height, a tail workgroup
    (61, 83, 5, "degenerate", {1: 0.5395, 2: 0.3686}),
    (61, 83, 5, "occluder", {1: 0.5579, 2: 0.4475}),
    (96, 128, 7, "both", {1: 0.4866, 2: 0.3190}),          # the size of small_scene(), no tail
    (96, 128, 7, "degenerate", {1: 0.5463, 2: 0.3792}),
    (5, 7, 3, "plain", {1: 0.4952, 2: 0.3238}),            # 35 pixels: less than one wave
    (37, 53, 6, "perK", {1: 0.6305, 2: 0.5844}),
    (1, 300, 3, "plain", {1: 0.0078}),          # one row: 7 of 900 pixels kept, none at thres_view 2
    (9, 13, 4, "degenerate", {1: 0.4829, 2: 0.3184}),      # 117 pixels: more than a wave, less than a workgroup
    (25, 41, 5, "both", {1: 0.4820, 2: 0.3019}),           # 1025 = 4 * 256 + 1: one pixel in the tail workgroup
    (11, 93, 4, "occluder", {1: 0.5413, 2: 0.4098}),       # 1023 = 4 * 256 - 1: one idle lane in the last workgroup
    (38, 53, 5, "degenerate", {1: 0.5379, 2: 0.3690}),     # odd width, even height
    (300, 3, 3, "plain", {1: 0.4815, 2: 0.3030}),          # tall and thin: another H / W ratio
]


def hard_id(case):
    return "%dx%dx%d-%s" % case[:4]


def hard_scene(H, W, V, kind, seed=0):
    """A scan that is hard on the kernels' edges.  Always: noise, 5 % outliers, ragged pairs (2..5 source views in a
    shuffled order), random confidence and float images.  `kind`:
      degenerate  3 % zeros (masked pixels), 1 % NaN, 0.5 % +inf, 1 % sign-flipped, 0.5 % 1e-30, 0.5 % 1e30
      occluder    the block [H/4:H/2, W/3:2W/3] of every map x 0.6: a depth discontinuity
      both        the two above
      perK        every view's fx, fy changed by up to 3 %, cx, cy by up to 2 pixels
    Deterministic, NumPy only."""
    assert kind in HARD_KINDS, kind
    depths, Ks, Es = plane_depth_maps(V, H, W, seed=5, noise=1e-3, outlier_frac=0.05)
    rng = np.random.RandomState(1000 + seed)
    conf = rng.rand(*depths.shape).astype(np.float32)
    images = rng.rand(*depths.shape, 3).astype(np.float32)
    if kind in ("occluder", "both"):
        depths[:, H // 4:H // 2, W // 3:2 * W // 3] *= np.float32(0.6)
    if kind in ("degenerate", "both"):
        u = rng.rand(*depths.shape)
        edges = np.cumsum([0.03, 0.01, 0.005, 0.01, 0.005, 0.005])
        depths[u < edges[0]] = 0.0
        depths[(u >= edges[0]) & (u < edges[1])] = np.nan
        depths[(u >= edges[1]) & (u < edges[2])] = np.inf
        flip = (u >= edges[2]) & (u < edges[3])
        depths[flip] = -depths[flip]
        depths[(u >= edges[3]) & (u < edges[4])] = 1e-30
        depths[(u >= edges[4]) & (u < edges[5])] = 1e30
    if kind == "perK":
        Ks = Ks.copy()
        Ks[:, 0, 0] *= (1 + 0.03 * (2 * rng.rand(V) - 1)).astype(np.float32)
        Ks[:, 1, 1] *= (1 + 0.03 * (2 * rng.rand(V) - 1)).astype(np.float32)
        Ks[:, 0, 2] += (2 * (2 * rng.rand(V) - 1)).astype(np.float32)
        Ks[:, 1, 2] += (2 * (2 * rng.rand(V) - 1)).astype(np.float32)
    return dict(depths=depths, Ks=Ks, Es=Es, conf=conf, images=images, pairs=make_pairs(V, 2, min(5, V - 1), seed=2))


def oracle_scene(sc, conf_thres=CONF_THRES, thres_view=THRES_VIEW):
    """filter_depth of the oracle over the scan -> (per-view results, vertex array)."""
    views = []
    with warnings.catch_warnings():                  # NaN / inf coordinates cast to integers, as the reference does
        warnings.simplefilter("ignore", RuntimeWarning)
        for r, srcs in sc["pairs"]:
            views.append(GO.filter_reference_view(sc["depths"][r], sc["Ks"][r], sc["Es"][r], sc["conf"][r],
                                                  sc["depths"][srcs], sc["Ks"][srcs], sc["Es"][srcs], conf_thres,
                                                  thres_view, ref_img=sc["images"][r]))
    return views, GO.vertex_array(views)


def scatter(final_mask, values):
    """[M, k] values in emission order (views in order, pixels row-major) -> [R,H,W,k] map, NaN-free zeros elsewhere."""
    out = np.zeros(final_mask.shape + (values.shape[1],), dtype=values.dtype)
    out[final_mask] = values
    return out


def assert_same_values(got, want, rel):
    """Two float maps with non-finite values: NaN in the same places, +inf / -inf in the same places with the same sign,
    zero where `want` is zero, and the finite non-zero values of `want` within `rel` relative.  -> the worst relative
    error of the finite non-zero values (0.0 if there is none)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), \
        "inf positions or signs differ"
    assert (got[want == 0] == 0).all(), "a zero became non-zero"
    sel = np.isfinite(want) & (want != 0)
    if not sel.any():
        return 0.0
    worst = float((np.abs(got[sel] - want[sel]) / np.abs(want[sel])).max())
    assert worst <= rel, worst
    return worst


def compare_with_oracle(got, want_views, want_vertices, view_masks=None, floor=0.3, thres_view=THRES_VIEW):
    """got: dict of NumPy arrays (geo_mask_sum, depth_est_averaged, photo_mask, geo_mask, final_mask [R,H,W], points
    [M,3] float32, colors [M,3] uint8, counts [R]).  `floor`: the fraction of the R*H*W pixels that both sides must keep
    (0.3 for small_scene; half of the oracle's own kept fraction for a hard scene, HARD_CASES).  Asserts the bounds and
    returns the measured figures."""
    votes = np.stack([w["geo_mask_sum"] for w in want_views])
    R, H, W = votes.shape
    pixel_views = sum(len(w["view_masks"]) for w in want_views) * H * W
    fig = {}
    if view_masks is not None:                                               # [R,Smax,H,W] votes per pixel-view
        flips = sum(int((view_masks[r, s].astype(bool) != m).sum()) for r, w in enumerate(want_views)
                    for s, m in enumerate(w["view_masks"]))
        fig["vote_flips"] = flips
        assert flips <= FLIP_FRAC * pixel_views, fig
    same_votes = got["geo_mask_sum"] == votes
    fig["vote_sum_mismatch_pixels"] = int((~same_votes).sum())
    assert fig["vote_sum_mismatch_pixels"] <= FLIP_FRAC * R * H * W, fig
    avg = np.stack([w["depth_est_averaged"] for w in want_views])
    fig["avg_nonfinite_pixels"] = int((~np.isfinite(avg)).sum())
    fig["avg_rel_max"] = assert_same_values(got["depth_est_averaged"][same_votes], avg[same_votes], AVG_REL)
    assert np.array_equal(got["photo_mask"], np.stack([w["photo_mask"] for w in want_views]))
    final = np.stack([w["final_mask"] for w in want_views])
    agree = got["final_mask"] & final
    fig["final_mask_mismatch_pixels"] = int((got["final_mask"] != final).sum())
    assert fig["final_mask_mismatch_pixels"] <= fig["vote_sum_mismatch_pixels"]
    assert np.array_equal(got["geo_mask"], got["geo_mask_sum"] >= thres_view)
    assert np.array_equal(got["final_mask"], got["photo_mask"] & got["geo_mask"])
    assert np.array_equal(got["counts"], got["final_mask"].reshape(R, -1).sum(1)) and got["counts"].sum() == len(got["points"])
    same_mask_views = (got["final_mask"] == final).reshape(R, -1).all(1)
    assert np.array_equal(got["counts"][same_mask_views], final.reshape(R, -1).sum(1)[same_mask_views])
    fig["points"], fig["oracle_points"] = int(len(got["points"])), int(len(want_vertices))
    fig["kept_frac_per_view"] = [round(float(f), 4) for f in final.reshape(R, -1).mean(1)]
    fig["kept_frac"], fig["kept_floor"] = float(final.mean()), float(floor)
    assert agree.sum() > floor * R * H * W, fig                              # neither empty nor trivial
    want_xyz = np.stack([want_vertices[c] for c in "xyz"], 1)
    want_rgb = np.stack([want_vertices[c] for c in ("red", "green", "blue")], 1)
    assert got["points"].dtype == np.float32 and got["colors"].dtype == np.uint8
    fig["nonfinite_points"] = int((~np.isfinite(got["points"])).any(1).sum())  # recorded: a survivor's depth is finite
    # world points: exact fp64 arithmetic up to rounding order, rounded once to float32 -> one float32 ulp of the cloud's
    # largest coordinate, absolute (the translation can cancel); a non-finite coordinate must be the same on both sides
    g, w = scatter(got["final_mask"], got["points"]).astype(np.float64)[agree], scatter(final, want_xyz)[agree].astype(np.float64)
    ok = np.isfinite(w)
    assert np.array_equal(np.isfinite(g), ok) and np.array_equal(g[~ok], w[~ok], equal_nan=True)
    ulp = float(np.spacing(np.float32(np.abs(w[ok]).max())))
    fig["xyz_abs_max"], fig["xyz_bound_one_ulp"] = float(np.abs(g[ok] - w[ok]).max()), ulp
    assert fig["xyz_abs_max"] <= ulp, fig
    assert np.array_equal(scatter(got["final_mask"], got["colors"])[agree], scatter(final, want_rgb)[agree])
    return fig


# ---- the host build of mvster_amd/csrc/geo_math.h -------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTMATH = os.path.join(ROOT, "tests", "hostmath")
HOST_FLAGS = ["-O2", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas"]


def load_geo_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/geo_hostmath.cpp with the first compiler of `compilers` that exists and load it.  No
    compiler is an error, never a skip: the comparisons that need the host build must not pass by not running."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of geo_math.h cannot be made" % (compilers,))
    so = os.path.join(HOSTMATH, "libgeohostmath.so")
    subprocess.check_call([found[0]] + HOST_FLAGS + ["-o", so, os.path.join(HOSTMATH, "geo_hostmath.cpp")])
    h = ctypes.CDLL(so)
    h.hm_geo_scene.restype = ctypes.c_long
    h.hm_geo_scene.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_float,
                                                                          ctypes.c_float] + [ctypes.c_void_p] * 9
    return h


def run_host_scene(ghm, sc, conf_thres=CONF_THRES, thres_view=THRES_VIEW, images=None):
    """hm_geo_scene over the scan -> dict of NumPy arrays with fuse_scene's keys plus view_mask [R,Smax,H,W]; float images
    (a uint8 image is handed over as v / 255, what read_img returns)."""
    from mvster_amd import fusion
    t = fusion.scene_tables(sc["pairs"], sc["Ks"], sc["Es"])
    R, smax = t.pair_table.shape
    V, H, W = sc["depths"].shape
    images = sc["images"] if images is None else images
    if images.dtype == np.uint8:
        images = images.astype(np.float32) / np.float32(255.0)
    out = dict(geo_mask_sum=np.zeros((R, H, W), np.int32), depth_est_averaged=np.zeros((R, H, W), np.float64),
               photo_mask=np.zeros((R, H, W), np.uint8), geo_mask=np.zeros((R, H, W), np.uint8),
               final_mask=np.zeros((R, H, W), np.uint8), view_mask=np.zeros((R, smax, H, W), np.uint8),
               points=np.zeros((R * H * W, 3), np.float32), colors=np.zeros((R * H * W, 3), np.uint8),
               counts=np.zeros(R, np.int64))
    ins = [np.ascontiguousarray(a) for a in (sc["depths"], sc["conf"], images, t.pair_table, t.ref_view, t.ref_mats,
                                             t.view_mats)]
    assert ins[0].dtype == ins[1].dtype == ins[2].dtype == np.float32
    m = ghm.hm_geo_scene(*[a.ctypes.data for a in ins], R, smax, V, H, W, conf_thres, thres_view, 1.0, 0.01,
                         *[out[k].ctypes.data for k in ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask",
                                                        "final_mask", "view_mask", "points", "colors", "counts")])
    assert m >= 0
    for k in ("photo_mask", "geo_mask", "final_mask"):
        out[k] = out[k].astype(bool)
    out["points"], out["colors"] = out["points"][:m], out["colors"][:m]
    return out


# ---- scans whose survivors are known in advance ----------------------------------------------------------------------

PATTERN_CONF_THRES = 0.5
PATTERNS = ("ones", "zeros", "first", "last", "lane63", "every65", "random", "per_view")


def pattern_mask(name, R, H, W, seed=0):
    """[R,H,W] bool: which pixels of each reference view are to survive."""
    hw = H * W
    p = np.arange(hw)
    rng = np.random.RandomState(77 + seed)
    if name == "ones":
        m = np.ones((R, hw), bool)
    elif name == "zeros":
        m = np.zeros((R, hw), bool)
    elif name == "first":
        m = np.tile(p == 0, (R, 1))
    elif name == "last":
        m = np.tile(p == hw - 1, (R, 1))
    elif name == "lane63":
        m = np.tile(p % 64 == 63, (R, 1))
    elif name == "every65":
        m = np.tile(p % 65 == 0, (R, 1))
    elif name == "random":
        m = rng.rand(R, hw) < 0.5
    elif name == "per_view":                         # densities 0 .. 1 across the views, independent pixels
        m = rng.rand(R, hw) < (np.arange(R) / max(R - 1, 1))[:, None]
    else:
        raise ValueError(name)
    return m.reshape(R, H, W)


def pattern_scene(H, W, V, pattern, rows=None, seed=0):
    """All V views share one camera and one noise-free depth map, so every pixel reprojects onto itself and gets a vote
    from every source view (checked against the oracle in tests/test_fusion_scene_cpu.py); the confidence map is the
    pattern (1 = survive, 0 = not), so at thres_view 1 and conf_thres 0.5 final_mask IS the pattern and the cloud can be
    predicted with NumPy.  `pattern` [V,H,W] bool.  `rows`: the reference view of every row of the pair table, repeats
    allowed (default 0..V-1); each row's sources are all other views.  uint8 images."""
    d, K, E = plane_depth_maps(1, H, W, seed=5)
    rng = np.random.RandomState(500 + seed)
    rows = list(range(V)) if rows is None else list(rows)
    return dict(depths=np.repeat(d, V, 0), Ks=np.repeat(K, V, 0), Es=np.repeat(E, V, 0),
                conf=pattern.astype(np.float32), images=rng.randint(0, 256, (V, H, W, 3)).astype(np.uint8),
                pairs=[(r, [v for v in range(V) if v != r]) for r in rows])


def expected_pattern_cloud(sc, pattern):
    """-> (final_mask [R,H,W], counts [R], colors [M,3]) that fuse_scene must give for pattern_scene at thres_view 1."""
    refs = [r for r, _ in sc["pairs"]]
    final = pattern[refs]
    colors = np.concatenate([sc["images"][r][pattern[r]] for r in refs]) if refs else np.zeros((0, 3), np.uint8)
    return final, final.reshape(len(refs), -1).sum(1), colors
