"""Whole-scan fusion on the GPU (``fuse_scene`` / ``filter_depth``: mvster_geo_scene_filter + mvster_geo_scene_emit)
against the oracle on the small scan of tests/fusion_scene_cases.py, and against the per-reference-view path
(``filter_reference_view`` over the pairs + ``fuse_views``), which it must reproduce bit for bit except for the world
points: those are fp64 on both sides (library matmul there, fma chains here) and rounded once to float32, so they may
differ by one float32 ulp of the cloud's largest coordinate.

Then the edges (tests/fusion_scene_cases.py): the hard scenes (odd sizes, tail workgroups, maps below one wave, NaN / inf /
zero / negative / tiny / huge depths, an occluder, per-view intrinsics) against the oracle, the per-view path and the
chunked run; every scene bit for bit against the host build of geo_math.h, which is what that header promises; scans
whose survivors are a known pattern, so that the compaction's output can be predicted exactly, up to the pass boundaries
of the scan kernel; and the two contracts of the C ABI that lie below ``fuse_scene``."""
import json
import os
import statistics
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import fusion
from mvster_amd import _lib, formats
from mvster_amd.synthetic_scene import plane_depth_maps
from tests import fusion_scene_cases as C

REPORT = {}
REPORT_DIR = os.environ.get("MVSTER_REPORT_DIR") or os.path.join("build", "reports")   # measured figures of a run


def note(name, **kv):
    REPORT[name] = kv
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "parity_fusion_scene.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def scene(sc, pairs=None, images=None, conf_thres=C.CONF_THRES, thres_view=C.THRES_VIEW, **kw):
    return fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"] if images is None else images, sc["Ks"], sc["Es"],
                             sc["pairs"] if pairs is None else pairs, conf_thres, thres_view, device="cuda:0", **kw)


def per_view(sc, pairs=None, images=None, conf_thres=C.CONF_THRES, thres_view=C.THRES_VIEW):
    """The scan loop over the per-reference-view API -> (results, vertex array)."""
    images = sc["images"] if images is None else images
    views = [fusion.filter_reference_view(sc["depths"][r], sc["Ks"][r], sc["Es"][r], sc["conf"][r], sc["depths"][srcs],
                                          sc["Ks"][srcs], sc["Es"][srcs], conf_thres, thres_view, ref_img=images[r])
             for r, srcs in (sc["pairs"] if pairs is None else pairs)]
    return views, fusion.fuse_views(views)


def as_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def same_bits(a, b):
    """torch.equal that takes NaN for what it is: float maps are compared through their bit patterns."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        as_int = {4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))
    return torch.equal(a, b)


def assert_drop_in(res, views, vertices, tag):
    """Bit-equal to the per-view path in everything but xyz (one-ulp bound)."""
    for k in ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask"):
        want = torch.stack([v[k] for v in views])
        assert res[k].dtype == want.dtype and res[k].shape == want.shape, k
        assert same_bits(res[k], want), (tag, k)
    got = res.vertices()
    assert got.dtype == vertices.dtype and len(got) == len(vertices), tag
    assert res["counts"].tolist() == [len(v["points"]) for v in views]
    for c in ("red", "green", "blue"):
        assert np.array_equal(got[c], vertices[c]), (tag, c)
    if len(got) == 0:
        return 0.0, 0.0
    ulp = float(np.spacing(np.float32(max(np.abs(vertices[c]).max() for c in "xyz"))))
    worst = max(float(np.abs(got[c].astype(np.float64) - vertices[c]).max()) for c in "xyz")
    assert worst <= ulp, (tag, worst, ulp)
    return worst, ulp


def test_small_scene_vs_oracle():
    sc = C.small_scene()
    want_views, want_vertices = C.oracle_scene(sc)
    res = scene(sc)
    for k in ("photo_mask", "geo_mask", "final_mask"):
        assert res[k].dtype == torch.bool and res[k].is_cuda
    assert res["geo_mask_sum"].dtype == torch.int32 and res["depth_est_averaged"].dtype == torch.float64
    assert res["points"].dtype == torch.float32 and res["colors"].dtype == torch.uint8 and res["counts"].shape == (7,)
    fig = C.compare_with_oracle(as_numpy(res), want_views, want_vertices)
    print("scene vs oracle:", fig)
    note("small_scene_vs_oracle", **fig)


def test_small_scene_is_a_drop_in_for_the_per_view_path():
    sc = C.small_scene()
    views, vertices = per_view(sc)
    worst, ulp = assert_drop_in(scene(sc), views, vertices, "small")
    note("small_scene_vs_per_view", xyz_abs_max=worst, xyz_bound_one_ulp=ulp, points=len(vertices))
    assert len(vertices) > 30000


def test_two_calls_give_identical_bytes():
    sc = C.small_scene()
    a, b = scene(sc), scene(sc)
    assert a.vertices().tobytes() == b.vertices().tobytes() and len(a["points"]) > 30000
    for k in ("geo_mask_sum", "depth_est_averaged", "final_mask", "counts"):
        assert torch.equal(a[k], b[k])


def test_ragged_pairs_single_source_and_subset_of_views():
    sc = C.small_scene()
    ragged = [(2, [5]), (0, [6, 2, 4, 5, 1, 3]), (4, [1, 0]), (6, [3, 2, 0])]      # refs 2, 0, 4, 6 of 7 views, 1..6 sources
    for thres_view in (1, 2):
        views, vertices = per_view(sc, pairs=ragged, thres_view=thres_view)
        res = scene(sc, pairs=ragged, thres_view=thres_view)
        assert res["final_mask"].shape[0] == 4
        assert_drop_in(res, views, vertices, "ragged")
    assert int(res["geo_mask_sum"][0].max()) <= 1 and int(res["geo_mask_sum"][1].max()) > 2
    assert int(res["counts"][0]) == 0 and int(res["counts"][1]) > 1000             # one source view cannot give two votes


def test_inputs_as_device_tensors_and_lists():
    sc = C.small_scene()
    want = scene(sc).vertices()
    dev = torch.device("cuda:0")
    res = fusion.fuse_scene(torch.from_numpy(sc["depths"]).to(dev), [torch.from_numpy(c).to(dev) for c in sc["conf"]],
                            list(sc["images"]), sc["Ks"], sc["Es"], sc["pairs"], C.CONF_THRES, C.THRES_VIEW)
    assert res.vertices().tobytes() == want.tobytes()


def test_u8_and_f32_images_give_the_same_colours():
    sc = C.small_scene()
    u8 = np.random.RandomState(3).randint(0, 256, sc["images"].shape).astype(np.uint8)
    u8[sc["pairs"][0][0]].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)           # every value at least once
    f32 = u8.astype(np.float32) / 255.0                                              # what read_img returns
    a, b = scene(sc, images=u8), scene(sc, images=f32)
    assert a.vertices().tobytes() == b.vertices().tobytes()
    want = torch.from_numpy(u8).cuda()[torch.from_numpy(np.array([r for r, _ in sc["pairs"]])).cuda()][a["final_mask"]]
    assert torch.equal(a["colors"], want)


def test_thres_view_above_every_source_count_gives_an_empty_valid_ply(tmp_path):
    sc = C.small_scene()
    res = scene(sc, thres_view=6)
    assert res["points"].shape == (0, 3) and res["colors"].shape == (0, 3) and int(res["counts"].sum()) == 0
    assert not res["geo_mask"].any() and res["photo_mask"].any()
    v = res.vertices()
    assert len(v) == 0 and v.dtype == fusion.PLY_VERTEX_DTYPE
    path = str(tmp_path / "empty.ply")
    fusion.write_ply(path, v)
    assert b"element vertex 0\n" in open(path, "rb").read() and len(fusion.read_ply(path)) == 0


def test_chunked_and_unchunked_runs_are_equal():
    sc = C.small_scene()
    whole = scene(sc)
    for budget in (1, 6000):                                       # one, then two reference views per chunk
        part = scene(sc, scratch_budget=budget)
        assert part.vertices().tobytes() == whole.vertices().tobytes()
        for k in ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask", "counts"):
            assert same_bits(part[k], whole[k]), k


def test_bad_inputs_raise():
    sc = C.small_scene()
    with pytest.raises(RuntimeError):
        scene(sc, pairs=[(0, [1, 7])])
    with pytest.raises(RuntimeError):
        scene(sc, pairs=[(0, [])])
    with pytest.raises(RuntimeError):
        fusion.fuse_scene(list(sc["depths"][:6]) + [sc["depths"][6][:, :100]], sc["conf"], sc["images"], sc["Ks"], sc["Es"],
                          sc["pairs"], 0.3, 2, device="cuda:0")
    with pytest.raises(RuntimeError):
        fusion.fuse_scene(sc["depths"], sc["conf"][:, :50], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], 0.3, 2,
                          device="cuda:0")


@pytest.fixture(scope="module")
def dtu_scene():
    """49 views of 512 x 640, 10 source views each: 62 720 workgroup counts, far beyond one pass of the scan."""
    depths, Ks, Es = plane_depth_maps(49, 512, 640, seed=9, noise=1e-3, outlier_frac=0.1)
    rng = np.random.RandomState(4)
    conf = rng.rand(*depths.shape).astype(np.float32)
    images = rng.randint(0, 256, depths.shape + (3,)).astype(np.uint8)
    return dict(depths=depths, Ks=Ks, Es=Es, conf=conf, images=images, pairs=C.make_pairs(49, 10, 10, seed=6))


def test_dtu_sized_scan_vs_per_view_path(dtu_scene):
    sc = dtu_scene
    f32 = {r: sc["images"][r].astype(np.float32) / 255.0 for r, _ in sc["pairs"]}     # the per-view API takes float images
    views, vertices = per_view(sc, images=f32, conf_thres=0.3, thres_view=3)
    res = scene(sc, conf_thres=0.3, thres_view=3)
    worst, ulp = assert_drop_in(res, views, vertices, "dtu")
    note("dtu_scan_vs_per_view", points=len(vertices), xyz_abs_max=worst, xyz_bound_one_ulp=ulp,
         kept_frac=float(res["final_mask"].float().mean()))
    assert len(vertices) > 100_000                                 # wide baselines: a few per cent of the pixels survive


def test_dtu_sized_scan_timing(dtu_scene):
    """Scene path against the scan loop over the per-view API, both from host NumPy arrays to the vertex array on the
    host; median of three warm runs.  Recorded; the assertion is only that the scene path is not slower (it does a
    strict subset of the loop's transfers, launches and syncs)."""
    sc = dtu_scene
    f32 = sc["images"].astype(np.float32) / 255.0

    def run_scene(events=None):
        t0 = time.perf_counter()
        v = scene(sc, conf_thres=0.3, thres_view=3, events=events).vertices()
        return time.perf_counter() - t0, v

    def run_loop():
        t0 = time.perf_counter()
        _, v = per_view(sc, images=f32, conf_thres=0.3, thres_view=3)
        return time.perf_counter() - t0, v
    run_scene(), run_loop()                                                       # warm-up
    events = []
    t_scene = [run_scene(events)[0] for _ in range(3)]
    t_loop = [run_loop()[0] for _ in range(3)]
    torch.cuda.synchronize()
    kern = {}
    for name, e0, e1 in events:
        kern.setdefault(name, []).append(e0.elapsed_time(e1))
    s, l = statistics.median(t_scene), statistics.median(t_loop)
    note("dtu_scan_timing_49x512x640x10", scene_s=s, per_view_loop_s=l, ratio_loop_over_scene=l / s, scene_runs_s=t_scene,
         per_view_loop_runs_s=t_loop, kernel_ms_median={k: statistics.median(v) for k, v in kern.items()})
    print("scene %.4f s, per-view loop %.4f s, ratio %.2f, kernels %s" % (s, l, l / s, REPORT["dtu_scan_timing_49x512x640x10"]["kernel_ms_median"]))
    assert s <= l


def test_filter_depth_on_a_scan_folder(tmp_path):
    from PIL import Image
    sc = C.small_scene()
    views = [0, 1, 2, 3, 4, 5, 6]
    ids = [v * 3 + 1 for v in views]                                              # file numbers are not stack indices
    scan, out = tmp_path / "scan", tmp_path / "out"
    for d in (scan / "cams", scan / "images", out / "depth_est", out / "confidence"):
        os.makedirs(d)
    rng = np.random.RandomState(8)
    for v, i in zip(views, ids):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3] = sc["Es"][v], sc["Ks"][v], [425.0, 2.5, 192, 905.0]
        formats.write_cam(str(scan / "cams" / ("%08d_cam.txt" % i)), cam)
        Image.fromarray(rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)).save(str(scan / "images" / ("%08d.jpg" % i)))
        formats.save_pfm(str(out / "depth_est" / ("%08d.pfm" % i)), sc["depths"][v])
        formats.save_pfm(str(out / "confidence" / ("%08d.pfm" % i)), sc["conf"][v])
    pairs = [(0, [1, 2, 3]), (4, [5, 6, 0, 2]), (6, [5, 4, 3])]                   # reference views: a subset of the views
    with open(scan / "pair.txt", "w") as f:
        f.write("%d\n" % (len(pairs) + 1))
        for r, srcs in pairs:
            f.write("%d\n%d %s\n" % (ids[r], len(srcs), " ".join("%d 1.0" % ids[s] for s in srcs)))
        f.write("%d\n0\n" % ids[1])                                               # a view without sources is dropped
    ply = str(tmp_path / "fused.ply")
    vertices = fusion.filter_depth(str(scan), str(scan), str(out), ply, conf=0.3, thres_view=2)
    back = fusion.read_ply(ply)
    assert back.tobytes() == vertices.tobytes() and len(back) > 5000
    # the same scan through fuse_scene, from the files as the readers hand them over (cameras as written, decoded JPEGs)
    cams = [formats.read_camera_parameters(str(scan / "cams" / ("%08d_cam.txt" % i))) for i in ids]
    decoded = np.stack([formats.read_img(str(scan / "images" / ("%08d.jpg" % i))) for i in ids])
    res = fusion.fuse_scene(sc["depths"], sc["conf"], decoded, [c[0] for c in cams], [c[1] for c in cams], pairs, 0.3, 2,
                            device="cuda:0")
    assert res.vertices().tobytes() == back.tobytes()
    for k, (r, _) in enumerate(pairs):
        for name in ("photo", "geo", "final"):
            png = np.array(Image.open(str(out / "mask" / ("%08d_%s.png" % (ids[r], name)))))
            assert png.dtype == np.uint8 and set(np.unique(png)) <= {0, 255}
            assert np.array_equal(png > 0, res[name + "_mask"][k].cpu().numpy()), (r, name)
    assert len(os.listdir(out / "mask")) == 9


# ---- edges: hard scenes, the host build bit for bit, predictable survivors, scan boundaries, ABI contracts ----------

HARD = [pytest.param(case, tv, kept / 2, id="%s-tv%d" % (C.hard_id(case), tv)) for case in C.HARD_CASES
        for tv, kept in sorted(case[4].items())]
HARD_SCENES = [pytest.param(case, id=C.hard_id(case)) for case in C.HARD_CASES]
RESULT_KEYS = ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask", "counts")


@pytest.fixture(scope="module")
def ghm():
    """The host build of geo_math.h by the recipe of the CPU suite; ROCm's clang++ as a host-only compiler where there is
    no g++.  Without either the tests that need it fail."""
    return C.load_geo_hostmath(("g++", "clang++"))


@pytest.mark.parametrize("case,thres_view,floor", HARD)
def test_hard_scene_vs_oracle(case, thres_view, floor):
    sc = C.hard_scene(*case[:4])
    want_views, want_vertices = C.oracle_scene(sc, thres_view=thres_view)
    res = scene(sc, thres_view=thres_view)
    fig = C.compare_with_oracle(as_numpy(res), want_views, want_vertices, floor=floor, thres_view=thres_view)
    print("hard scene vs oracle:", C.hard_id(case), thres_view, fig)
    note("hard_vs_oracle_%s_tv%d" % (C.hard_id(case), thres_view), **fig)


@pytest.mark.parametrize("case,thres_view,floor", HARD)
def test_hard_scene_is_a_drop_in_for_the_per_view_path_and_for_its_chunks(case, thres_view, floor):
    sc = C.hard_scene(*case[:4])
    views, vertices = per_view(sc, thres_view=thres_view)
    whole = scene(sc, thres_view=thres_view)
    worst, ulp = assert_drop_in(whole, views, vertices, C.hard_id(case))
    note("hard_vs_per_view_%s_tv%d" % (C.hard_id(case), thres_view), xyz_abs_max=worst, xyz_bound_one_ulp=ulp,
         points=len(vertices))
    assert len(vertices) > floor * whole["final_mask"].numel()
    part = scene(sc, thres_view=thres_view, scratch_budget=1)                 # one reference view per chunk
    assert part.vertices().tobytes() == whole.vertices().tobytes()
    for k in RESULT_KEYS:
        assert same_bits(part[k], whole[k]), k


@pytest.mark.parametrize("case", [c for c in C.HARD_CASES if (c[0], c[1]) in ((61, 83), (25, 41), (5, 7))][:5],
                         ids=C.hard_id)
def test_u8_and_f32_images_give_the_same_bytes_on_odd_sizes(case):
    sc = C.hard_scene(*case[:4])
    u8 = np.random.RandomState(3).randint(0, 256, sc["images"].shape).astype(np.uint8)
    a, b = scene(sc, images=u8), scene(sc, images=u8.astype(np.float32) / 255.0)
    assert a.vertices().tobytes() == b.vertices().tobytes() and len(a["points"]) > 0
    refs = torch.from_numpy(np.array([r for r, _ in sc["pairs"]])).cuda()
    assert torch.equal(a["colors"], torch.from_numpy(u8).cuda()[refs][a["final_mask"]])


def host_vs_gpu(ghm, sc, tag, conf_thres=C.CONF_THRES, thres_view=C.THRES_VIEW):
    """fuse_scene against hm_geo_scene: the figures first (printed and recorded), then every byte.  geo_math.h promises
    that the kernels and the host build execute the same expression tree, so the bound is equality of bit patterns."""
    got = as_numpy(scene(sc, conf_thres=conf_thres, thres_view=thres_view))
    want = C.run_host_scene(ghm, sc, conf_thres=conf_thres, thres_view=thres_view)
    ga, wa = got["depth_est_averaged"].view(np.int64), want["depth_est_averaged"].view(np.int64)
    both_nan = np.isnan(got["depth_est_averaged"]) & np.isnan(want["depth_est_averaged"])
    fig = dict(vote_sum_mismatch_pixels=int((got["geo_mask_sum"] != want["geo_mask_sum"]).sum()),
               avg_bit_mismatch_pixels=int((ga != wa).sum()), avg_nan_payload_mismatch_pixels=int((ga != wa)[both_nan].sum()),
               avg_nonfinite_pixels=int((~np.isfinite(want["depth_est_averaged"])).sum()),
               mask_mismatch_pixels=int(sum((got[k] != want[k]).sum() for k in ("photo_mask", "geo_mask", "final_mask"))),
               points=int(len(got["points"])), host_points=int(len(want["points"])),
               nonfinite_points=int((~np.isfinite(got["points"])).any(1).sum()),
               kept_frac=float(want["final_mask"].mean()))
    if len(got["points"]) == len(want["points"]):
        fig["xyz_bit_mismatch_values"] = int((got["points"].view(np.int32) != want["points"].view(np.int32)).sum())
        fig["xyz_abs_max"] = float(np.nanmax(np.abs(got["points"].astype(np.float64) - want["points"]), initial=0.0))
        fig["color_mismatch_values"] = int((got["colors"] != want["colors"]).sum())
    print("gpu vs host build:", tag, fig)
    note("gpu_vs_host_build_" + tag, **fig)
    assert got["geo_mask_sum"].tobytes() == want["geo_mask_sum"].tobytes(), fig
    assert got["depth_est_averaged"].tobytes() == want["depth_est_averaged"].tobytes(), fig
    for k in ("photo_mask", "geo_mask", "final_mask"):
        assert got[k].dtype == want[k].dtype == np.bool_ and got[k].tobytes() == want[k].tobytes(), (k, fig)
    assert got["counts"].tolist() == want["counts"].tolist(), fig
    assert got["points"].dtype == np.float32 and got["points"].tobytes() == want["points"].tobytes(), fig
    assert got["colors"].dtype == np.uint8 and got["colors"].tobytes() == want["colors"].tobytes(), fig
    return got, fig


def test_small_scene_equals_the_host_build_bit_for_bit(ghm):
    got, _ = host_vs_gpu(ghm, C.small_scene(), "small_scene")
    assert len(got["points"]) > 30000


@pytest.mark.parametrize("case,thres_view,floor", HARD)
def test_hard_scene_equals_the_host_build_bit_for_bit(ghm, case, thres_view, floor):
    got, _ = host_vs_gpu(ghm, C.hard_scene(*case[:4]), "%s_tv%d" % (C.hard_id(case), thres_view), thres_view=thres_view)
    assert len(got["points"]) > floor * got["final_mask"].size


def test_negative_reference_depth_is_treated_as_in_the_reference(ghm):
    """|d_reprojected - d_ref| / d_ref is negative for a negative reference depth and so passes `< 0.01`, as in the
    reference (test_mvs4.py:322-323); whether such a pixel gets a vote is then up to the pixel test alone (none does on
    this scene: the point lies behind the camera).  Pinned against the host build so nobody "fixes" it on one side only."""
    sc = C.hard_scene(61, 83, 5, "degenerate")
    res = as_numpy(scene(sc, thres_view=1))
    neg = np.stack([sc["depths"][r] < 0 for r, _ in sc["pairs"]])
    want = C.run_host_scene(ghm, sc, thres_view=1)
    assert neg.sum() > 100 and np.array_equal(res["geo_mask_sum"][neg], want["geo_mask_sum"][neg])
    assert np.array_equal(res["depth_est_averaged"][neg], want["depth_est_averaged"][neg]) and (res["depth_est_averaged"][neg] < 0).all()
    note("negative_reference_depth", pixels=int(neg.sum()), pixels_with_votes=int((res["geo_mask_sum"][neg] > 0).sum()))


@pytest.mark.parametrize("pattern", C.PATTERNS)
@pytest.mark.parametrize("H,W", [(61, 83), (96, 128)])
def test_compaction_with_predictable_survivors(ghm, H, W, pattern):
    """One camera and one depth map for all views: every pixel gets every vote, final_mask is the confidence pattern,
    and counts, colours and their order follow from the pattern alone."""
    V = 4
    mask = C.pattern_mask(pattern, V, H, W)
    sc = C.pattern_scene(H, W, V, mask)
    final, counts, colors = C.expected_pattern_cloud(sc, mask)
    res = as_numpy(scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=1))
    assert (res["geo_mask_sum"] == V - 1).all() and res["geo_mask"].all()
    assert np.array_equal(res["final_mask"], final) and np.array_equal(res["photo_mask"], final)
    assert res["counts"].tolist() == counts.tolist() and len(res["points"]) == counts.sum() == len(res["colors"])
    assert np.array_equal(res["colors"], colors)
    want = C.run_host_scene(ghm, sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=1)
    assert res["points"].tobytes() == want["points"].tobytes() and np.isfinite(res["points"]).all()
    note("pattern_%s_%dx%d" % (pattern, H, W), points=int(counts.sum()), kept_frac=float(final.mean()))


# n = R * ceil(H*W / 256) workgroup counts go through geo_scene_scan_kernel, 1024 * 16 = 16 384 per pass
@pytest.mark.parametrize("R,H,W,n", [(1, 9, 13, 1), (43, 311, 313, 16383), (64, 256, 256, 16384), (5, 3277, 256, 16385),
                                     (9, 3641, 256, 32769)])
def test_scan_pass_boundaries(R, H, W, n):
    """Two views with one camera and one depth map, each the other's only source, repeated as reference views R times;
    a random half of the pixels survive.  counts, the number of points and every colour against NumPy."""
    lib = _lib.load()
    assert lib.mvster_geo_scene_blocks(R, H, W) == n
    mask = C.pattern_mask("random", 2, H, W, seed=n)
    sc = C.pattern_scene(H, W, 2, mask, rows=[i % 2 for i in range(R)], seed=n)
    final, counts, colors = C.expected_pattern_cloud(sc, mask)
    res = scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=1)
    assert res["counts"].tolist() == counts.tolist() and len(res["points"]) == int(counts.sum()) == len(res["colors"])
    assert torch.equal(res["final_mask"].cpu(), torch.from_numpy(final))
    assert torch.equal(res["colors"].cpu(), torch.from_numpy(colors))
    pts = res["points"].cpu().numpy()
    assert np.isfinite(pts).all()
    bounds = np.concatenate([[0], np.cumsum(counts)])
    for i in range(2, R):                               # a repeated reference view emits the same points again
        assert np.array_equal(pts[bounds[i]:bounds[i + 1]], pts[bounds[i - 2]:bounds[i - 1]]), i
    note("scan_boundary_n%d" % n, R=R, H=H, W=W, points=int(counts.sum()))


class RawScene:
    """mvster_geo_scene_filter / _emit through the C ABI on device tensors, below fuse_scene's argument checks."""

    def __init__(self, sc, images_u8, thres_view=C.THRES_VIEW):
        self.lib, dev = _lib.load(), torch.device("cuda:0")
        self.t = fusion.scene_tables(sc["pairs"], sc["Ks"], sc["Es"])
        self.V, self.H, self.W = sc["depths"].shape
        self.R, self.smax = self.t.pair_table.shape
        self.nblk = self.lib.mvster_geo_scene_blocks(1, self.H, self.W)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                      # noqa: E731
        self.depth, self.conf, self.img = up(sc["depths"]), up(sc["conf"]), up(images_u8)
        self.pairs, self.ref_mats, self.view_mats = up(self.t.pair_table), up(self.t.ref_mats), up(self.t.view_mats)
        self.thres_view, self.dev = thres_view, dev

    def filter(self, ref_view):
        """-> dict of outputs, every buffer pre-filled with a value the kernel never writes."""
        R, H, W, dev = self.R, self.H, self.W, self.dev
        o = dict(ref_view=torch.tensor(ref_view, dtype=torch.int32, device=dev),
                 geo_mask_sum=torch.full((R, H, W), -77, dtype=torch.int32, device=dev),
                 depth_est_averaged=torch.full((R, H, W), -7.5, dtype=torch.float64, device=dev),
                 wg_counts=torch.full((R * self.nblk,), -1, dtype=torch.int32, device=dev),
                 wg_offsets=torch.full((R * self.nblk + 1,), -1, dtype=torch.int64, device=dev))
        for k in ("photo_mask", "geo_mask", "final_mask"):
            o[k] = torch.full((R, H, W), 0xEE, dtype=torch.uint8, device=dev)
        rc = self.lib.mvster_geo_scene_filter(self.depth.data_ptr(), self.conf.data_ptr(), self.pairs.data_ptr(),
                                              o["ref_view"].data_ptr(), self.ref_mats.data_ptr(), self.view_mats.data_ptr(),
                                              o["geo_mask_sum"].data_ptr(), o["depth_est_averaged"].data_ptr(),
                                              o["photo_mask"].data_ptr(), o["geo_mask"].data_ptr(), o["final_mask"].data_ptr(),
                                              o["wg_counts"].data_ptr(), o["wg_offsets"].data_ptr(), R, self.smax, self.V, H, W,
                                              C.CONF_THRES, self.thres_view, 1.0, 0.01,
                                              torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "geo_scene_filter")
        torch.cuda.synchronize()
        return o

    def emit(self, o, M, rows):
        """Emit with capacity M into buffers of `rows` rows filled with a canary -> (points, colors) on the host."""
        points = torch.full((rows, 3), -12345.0, dtype=torch.float32, device=self.dev)
        colors = torch.full((rows, 3), 0xA5, dtype=torch.uint8, device=self.dev)
        rc = self.lib.mvster_geo_scene_emit(o["depth_est_averaged"].data_ptr(), o["final_mask"].data_ptr(),
                                            o["ref_view"].data_ptr(), self.ref_mats.data_ptr(), self.img.data_ptr(), 0,
                                            o["wg_offsets"].data_ptr(), points.data_ptr(), colors.data_ptr(), M, self.R,
                                            self.V, self.H, self.W, torch.cuda.current_stream(self.dev).cuda_stream)
        _lib.check(rc, "geo_scene_emit")
        torch.cuda.synchronize()
        return points.cpu().numpy(), colors.cpu().numpy()


def raw_hard_scene():
    sc = C.hard_scene(61, 83, 5, "plain")                                 # 20 workgroups per view, the last one a tail
    u8 = np.random.RandomState(6).randint(0, 256, sc["images"].shape).astype(np.uint8)
    return sc, u8, RawScene(sc, u8)


def test_abi_reference_view_outside_the_stack_gives_a_zero_row_and_no_survivors():
    """include/mvster_hip.h: a ref_view entry outside [0, V) gives an all-zero row and no survivors.  Rows 1 and 3 hold
    V and -1; the other rows must not notice."""
    sc, u8, raw = raw_hard_scene()
    good = raw.filter(raw.t.ref_view.tolist())
    bad_rows = {1: raw.V, 3: -1}
    bad = raw.filter([bad_rows.get(i, r) for i, r in enumerate(raw.t.ref_view.tolist())])
    nblk = raw.nblk
    counts_good = good["wg_counts"].view(raw.R, nblk).sum(1).tolist()
    assert min(counts_good) > 1000 and int(good["wg_offsets"][-1]) == sum(counts_good)
    for i in range(raw.R):
        for k in ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask"):
            if i in bad_rows:
                assert int(torch.count_nonzero(bad[k][i])) == 0, (i, k)
            else:
                assert same_bits(bad[k][i], good[k][i]), (i, k)
        want = torch.zeros_like(good["wg_counts"][:nblk]) if i in bad_rows else good["wg_counts"][i * nblk:(i + 1) * nblk]
        assert torch.equal(bad["wg_counts"][i * nblk:(i + 1) * nblk], want), i
    M_good, M_bad = int(good["wg_offsets"][-1]), int(bad["wg_offsets"][-1])
    assert M_bad == sum(c for i, c in enumerate(counts_good) if i not in bad_rows)
    pg, cg = raw.emit(good, M_good, M_good + 16)
    pb, cb = raw.emit(bad, M_bad, M_good + 16)
    bounds = np.concatenate([[0], np.cumsum(counts_good)])
    keep = np.concatenate([np.arange(bounds[i], bounds[i + 1]) for i in range(raw.R) if i not in bad_rows])
    assert pb[:M_bad].tobytes() == pg[keep].tobytes() and cb[:M_bad].tobytes() == cg[keep].tobytes()
    assert (pb[M_bad:] == -12345.0).all() and (cb[M_bad:] == 0xA5).all()         # nothing was written for the bad rows
    assert (pg[M_good:] == -12345.0).all() and (cg[M_good:] == 0xA5).all()
    whole = scene(sc, images=u8)                                                # and the good run is fuse_scene's
    assert whole["points"].cpu().numpy().tobytes() == pg[:M_good].tobytes()
    assert whole["colors"].cpu().numpy().tobytes() == cg[:M_good].tobytes()
    note("abi_bad_ref_view", points_good=M_good, points_with_two_bad_rows=M_bad)


def test_abi_emit_truncates_at_the_capacity_of_the_buffers():
    """include/mvster_hip.h: M below the number of survivors truncates the emission; nothing is written behind row M."""
    sc, u8, raw = raw_hard_scene()
    o = raw.filter(raw.t.ref_view.tolist())
    survivors = int(o["wg_offsets"][-1])
    full_p, full_c = raw.emit(o, survivors, survivors)
    M = survivors - 7
    p, c = raw.emit(o, M, M + 16)
    assert p[:M].tobytes() == full_p[:M].tobytes() and c[:M].tobytes() == full_c[:M].tobytes()
    assert (p[M:] == -12345.0).all() and (c[M:] == 0xA5).all()
    assert not (full_p == -12345.0).any()
    note("abi_emit_capacity", survivors=survivors, M=M)
