"""Shared by tests/test_fusion_scene_cpu.py and tests/test_gpu_fusion_scene.py: the small scan both check against the
oracle, the oracle run over a scan, and the comparison with its bounds (not a test module)."""
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


def oracle_scene(sc, conf_thres=CONF_THRES, thres_view=THRES_VIEW):
    """filter_depth of the oracle over the scan -> (per-view results, vertex array)."""
    views = []
    for r, srcs in sc["pairs"]:
        views.append(GO.filter_reference_view(sc["depths"][r], sc["Ks"][r], sc["Es"][r], sc["conf"][r], sc["depths"][srcs],
                                              sc["Ks"][srcs], sc["Es"][srcs], conf_thres, thres_view,
                                              ref_img=sc["images"][r]))
    return views, GO.vertex_array(views)


def scatter(final_mask, values):
    """[M, k] values in emission order (views in order, pixels row-major) -> [R,H,W,k] map, NaN-free zeros elsewhere."""
    out = np.zeros(final_mask.shape + (values.shape[1],), dtype=values.dtype)
    out[final_mask] = values
    return out


def compare_with_oracle(got, want_views, want_vertices, view_masks=None):
    """got: dict of NumPy arrays (geo_mask_sum, depth_est_averaged, photo_mask, geo_mask, final_mask [R,H,W], points
    [M,3] float32, colors [M,3] uint8, counts [R]).  Asserts the bounds and returns the measured figures."""
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
    fig["avg_rel_max"] = float((np.abs(got["depth_est_averaged"] - avg)[same_votes] / np.abs(avg[same_votes])).max())
    assert fig["avg_rel_max"] <= AVG_REL, fig
    assert np.array_equal(got["photo_mask"], np.stack([w["photo_mask"] for w in want_views]))
    final = np.stack([w["final_mask"] for w in want_views])
    agree = got["final_mask"] & final
    fig["final_mask_mismatch_pixels"] = int((got["final_mask"] != final).sum())
    assert fig["final_mask_mismatch_pixels"] <= fig["vote_sum_mismatch_pixels"]
    assert np.array_equal(got["geo_mask"], got["geo_mask_sum"] >= THRES_VIEW)
    assert np.array_equal(got["final_mask"], got["photo_mask"] & got["geo_mask"])
    assert np.array_equal(got["counts"], got["final_mask"].reshape(R, -1).sum(1)) and got["counts"].sum() == len(got["points"])
    same_mask_views = (got["final_mask"] == final).reshape(R, -1).all(1)
    assert np.array_equal(got["counts"][same_mask_views], final.reshape(R, -1).sum(1)[same_mask_views])
    fig["points"], fig["oracle_points"] = int(len(got["points"])), int(len(want_vertices))
    fig["kept_frac_per_view"] = [round(float(f), 4) for f in final.reshape(R, -1).mean(1)]
    assert agree.sum() > 0.3 * R * H * W                                     # neither empty nor trivial
    want_xyz = np.stack([want_vertices[c] for c in "xyz"], 1)
    want_rgb = np.stack([want_vertices[c] for c in ("red", "green", "blue")], 1)
    assert got["points"].dtype == np.float32 and got["colors"].dtype == np.uint8
    # world points: exact fp64 arithmetic up to rounding order, rounded once to float32 -> one float32 ulp of the cloud's
    # largest coordinate, absolute (the translation can cancel)
    ulp = float(np.spacing(np.float32(np.abs(want_xyz).max())))
    d = np.abs(scatter(got["final_mask"], got["points"]).astype(np.float64) - scatter(final, want_xyz))[agree]
    fig["xyz_abs_max"], fig["xyz_bound_one_ulp"] = float(d.max()), ulp
    assert fig["xyz_abs_max"] <= ulp, fig
    assert np.array_equal(scatter(got["final_mask"], got["colors"])[agree], scatter(final, want_rgb)[agree])
    return fig
