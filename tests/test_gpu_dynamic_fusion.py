"""Dynamic consistency fusion on the GPU (``fuse_scene(method="dynamic")``: mvster_geo_scene_filter_dynamic +
mvster_geo_scene_emit): bit for bit against the host build of the geo_math.h functions the kernel inlines, within the fixed
filter's bounds against the NumPy restatement (tests/dynamic_fusion_cases.py), scans whose survivors and levels are known in
advance, the limits of the per-pixel level counts, and the entry points above ``fuse_scene``."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import fusion
from mvster_amd import MVS4net, formats, scan
from tests import dynamic_fusion_cases as D
from tests import fusion_scene_cases as C
from tests import scan_dataset_cases as DC
from tests import scan_short_cases as SS

DEV = "cuda:0"
REPORT = {}
REPORT_DIR = os.environ.get("MVSTER_REPORT_DIR") or os.path.join("build", "reports")   # measured figures of a run
CASES = [pytest.param(name, case, kept, id=name) for name, case, kept in D.DYN_CASES]
MAP_KEYS = ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask", "geo_level", "counts")


def note(name, **kv):
    REPORT[name] = kv
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "parity_dynamic_fusion.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def scene(sc, images=None, conf_thres=D.CONF_THRES, thres_view=D.THRES_VIEW, method="dynamic", **kw):
    return fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"] if images is None else images, sc["Ks"], sc["Es"],
                             sc["pairs"], conf_thres, thres_view, device=DEV, method=method, **kw)


def as_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def same_bytes(a, b):
    """Two results of fuse_scene: every map (float maps through their bit patterns, NaN included) and the cloud."""
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def dhm():
    return D.load_geo_dyn_hostmath(("g++", "clang++"))


@pytest.fixture(scope="module")
def results():
    """fuse_scene(method="dynamic") on a DYN_CASES scan at the default parameters, once per module, as NumPy arrays."""
    cache = {}

    def get(name, case):
        if name not in cache:
            cache[name] = as_numpy(scene(D.dyn_scene(case)))
        return cache[name]
    return get


@pytest.mark.parametrize("name,case,kept", CASES)
def test_equals_the_host_build_bit_for_bit(dhm, results, name, case, kept):
    """geo_math.h promises that the kernel and the host build execute the same expression tree: every mask, geo_level,
    geo_mask_sum, depth_est_averaged, counts, points and colours are the same bytes."""
    got = results(name, case)
    want = D.run_host_dynamic(dhm, D.dyn_scene(case))
    ga, wa = got["depth_est_averaged"].view(np.int64), want["depth_est_averaged"].view(np.int64)
    fig = dict(vote_sum_mismatch_pixels=int((got["geo_mask_sum"] != want["geo_mask_sum"]).sum()),
               level_mismatch_pixels=int((got["geo_level"] != want["geo_level"]).sum()),
               avg_bit_mismatch_pixels=int((ga != wa).sum()),
               mask_mismatch_pixels=int(sum((got[k] != want[k]).sum() for k in ("photo_mask", "geo_mask", "final_mask"))),
               points=int(len(got["points"])), host_points=int(len(want["points"])), kept_frac=float(want["final_mask"].mean()))
    print("dynamic gpu vs host build:", name, fig)
    note("gpu_vs_host_build_" + name, **fig)
    assert got["geo_level"].dtype == np.uint8 and got["geo_mask_sum"].dtype == np.int32
    for k in D.HOST_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, fig)
    assert len(got["points"]) > kept / 2 * got["final_mask"].size


@pytest.mark.parametrize("name,case,kept", CASES)
def test_vs_the_restatement(results, name, case, kept):
    views, vertices = D.restated_case(name, case)
    fig = D.compare_with_restatement(results(name, case), views, vertices, floor=kept / 2)
    print("dynamic gpu vs restatement:", name, fig)
    note("gpu_vs_restatement_" + name, **fig)


def test_result_layout_and_two_calls_give_identical_bytes():
    sc = C.small_scene()
    a, b = scene(sc), scene(sc)
    assert a["geo_level"].dtype == torch.uint8 and a["geo_level"].is_cuda and a["geo_level"].shape == a["final_mask"].shape
    assert torch.equal(a["geo_mask"], a["geo_level"] != 0) and torch.equal(a["final_mask"], a["photo_mask"] & a["geo_mask"])
    assert set(range(2, 6)) <= set(torch.unique(a["geo_level"]).tolist())
    same_bytes(a, b)
    assert a.vertices().tobytes() == b.vertices().tobytes() and len(a["points"]) > 20000


@pytest.mark.parametrize("name", ["small", "61x83x5-degenerate", "25x41x5-both"])
def test_chunked_and_unchunked_runs_are_equal(results, name):
    case = dict((n, c) for n, c, _ in D.DYN_CASES)[name]
    sc = D.dyn_scene(case)
    whole = results(name, case)
    for budget in (1, 6000):                                       # one reference view per chunk, then a few
        part = as_numpy(scene(sc, scratch_budget=budget))
        for k in whole:
            assert part[k].tobytes() == whole[k].tobytes(), (budget, k)


@pytest.mark.parametrize("name", ["small", "61x83x5-plain", "5x7x3-plain"])
def test_u8_and_f32_images_give_the_same_bytes(name):
    sc = D.dyn_scene(dict((n, c) for n, c, _ in D.DYN_CASES)[name])
    u8 = np.random.RandomState(3).randint(0, 256, sc["images"].shape).astype(np.uint8)
    a, b = scene(sc, images=u8), scene(sc, images=u8.astype(np.float32) / 255.0)
    same_bytes(a, b)
    assert len(a["points"]) > 0
    refs = torch.from_numpy(np.array([r for r, _ in sc["pairs"]])).cuda()
    assert torch.equal(a["colors"], torch.from_numpy(u8).cuda()[refs][a["final_mask"]])


@pytest.mark.parametrize("pattern", ["ones", "zeros", "lane63", "every65", "per_view"])
@pytest.mark.parametrize("H,W", [(61, 83), (96, 128)])
def test_pattern_scenes_have_predictable_survivors(dhm, H, W, pattern):
    """One camera and one depth map for all views: every source passes the first level, so geo_level is thres_view
    everywhere, final_mask IS the confidence pattern, and counts, colours and their order follow from the pattern."""
    V, thres_view = 4, 2
    mask = C.pattern_mask(pattern, V, H, W)
    sc = C.pattern_scene(H, W, V, mask)
    final, counts, colors = C.expected_pattern_cloud(sc, mask)
    res = as_numpy(scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=thres_view))
    assert (res["geo_level"] == thres_view).all() and (res["geo_mask_sum"] == V - 1).all() and res["geo_mask"].all()
    assert np.array_equal(res["final_mask"], final) and np.array_equal(res["photo_mask"], final)
    assert res["counts"].tolist() == counts.tolist() and len(res["points"]) == counts.sum() == len(res["colors"])
    assert np.array_equal(res["colors"], colors)
    want = D.run_host_dynamic(dhm, sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=thres_view)
    assert res["points"].tobytes() == want["points"].tobytes() and np.isfinite(res["points"]).all()
    above = as_numpy(scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=V))       # L = V - 1 < thres_view: no level
    assert not above["geo_level"].any() and not above["final_mask"].any() and len(above["points"]) == 0
    assert (above["geo_mask_sum"] == V - 1).all()                                    # the loosest level still counts them


def test_thres_view_above_one_rows_source_count_empties_that_row_only():
    V, H, W = 4, 9, 13
    sc = C.pattern_scene(H, W, V, C.pattern_mask("ones", V, H, W))
    sc["pairs"][2] = (2, [0, 3])
    res = scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=3)
    assert res["counts"].tolist() == [H * W, H * W, 0, H * W]
    assert not res["geo_level"][2].any() and (res["geo_level"][[0, 1, 3]] == 3).all()


def test_a_row_of_32_sources_runs_and_33_raise(dhm):
    H, W = 9, 13
    sc = C.pattern_scene(H, W, 33, C.pattern_mask("ones", 33, H, W), rows=[0, 7])
    res = as_numpy(scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=D.THRES_VIEW))
    assert (res["geo_level"] == D.THRES_VIEW).all() and (res["geo_mask_sum"] == 32).all()
    assert res["counts"].tolist() == [H * W, H * W]
    too_many = C.pattern_scene(H, W, 34, C.pattern_mask("ones", 34, H, W), rows=[0])
    with pytest.raises(RuntimeError, match="at most 32 source views"):
        scene(too_many, conf_thres=C.PATTERN_CONF_THRES)
    normal = scene(too_many, conf_thres=C.PATTERN_CONF_THRES, method="normal")       # the fixed filter has no such limit
    assert int(normal["counts"][0]) == H * W
    # every bin of the level counts: a scan built so that pixel p reaches level k(p) and none below
    stairs, k = D.staircase_scene(H, W, 32)
    got = as_numpy(scene(stairs, thres_view=1))
    want = D.run_host_dynamic(dhm, stairs, thres_view=1)
    assert np.array_equal(got["geo_level"][0], k) and np.array_equal(got["geo_mask_sum"][0], k)
    for key in D.HOST_KEYS:
        assert got[key].tobytes() == want[key].tobytes(), key


def test_the_empty_case_writes_a_valid_ply_with_no_vertices(tmp_path):
    sc = C.hard_scene(*D.EMPTY_CASE[:4])
    res = scene(sc)
    assert res["points"].shape == (0, 3) and res["colors"].shape == (0, 3) and int(res["counts"].sum()) == 0
    assert not res["final_mask"].any() and res["photo_mask"].any()
    v = res.vertices()
    assert len(v) == 0 and v.dtype == fusion.PLY_VERTEX_DTYPE
    path = str(tmp_path / "empty.ply")
    fusion.write_ply(path, v)
    assert b"element vertex 0\n" in open(path, "rb").read() and len(fusion.read_ply(path)) == 0


def test_method_normal_is_the_call_without_the_keyword():
    sc = C.small_scene()
    args = (sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], C.CONF_THRES, C.THRES_VIEW)
    plain = fusion.fuse_scene(*args, device=DEV)
    named = fusion.fuse_scene(*args, device=DEV, method="normal")
    explicit = fusion.fuse_scene(*args, 1.0, 0.01, device=DEV, method="normal")
    assert "geo_level" not in plain and sorted(plain) == sorted(named)
    same_bytes(plain, named)
    same_bytes(plain, explicit)
    assert len(plain["points"]) > 30000 and len(plain["points"]) != len(scene(sc)["points"])
    with pytest.raises(RuntimeError, match="bad shape"):
        scene(sc, thres_view=0)
    with pytest.raises(RuntimeError, match="bad shape"):
        scene(sc, pix_base=0.0)


def test_filter_depth_dynamic_on_a_scan_folder(tmp_path):
    from PIL import Image
    sc = C.small_scene()
    ids = [v * 3 + 1 for v in range(7)]                                           # file numbers are not stack indices
    folder, out = tmp_path / "scan", tmp_path / "out"
    for d in (folder / "cams", folder / "images", out / "depth_est", out / "confidence"):
        os.makedirs(d)
    rng = np.random.RandomState(8)
    for v, i in enumerate(ids):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3] = sc["Es"][v], sc["Ks"][v], [425.0, 2.5, 192, 905.0]
        formats.write_cam(str(folder / "cams" / ("%08d_cam.txt" % i)), cam)
        Image.fromarray(rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)).save(str(folder / "images" / ("%08d.jpg" % i)))
        formats.save_pfm(str(out / "depth_est" / ("%08d.pfm" % i)), sc["depths"][v])
        formats.save_pfm(str(out / "confidence" / ("%08d.pfm" % i)), sc["conf"][v])
    pairs = [(0, [1, 2, 3]), (4, [5, 6, 0, 2]), (6, [5, 4, 3])]
    with open(folder / "pair.txt", "w") as f:
        f.write("%d\n" % len(pairs))
        for r, srcs in pairs:
            f.write("%d\n%d %s\n" % (ids[r], len(srcs), " ".join("%d 1.0" % ids[s] for s in srcs)))
    ply = str(tmp_path / "fused.ply")
    vertices = fusion.filter_depth(str(folder), str(folder), str(out), ply, conf=0.3, thres_view=2, filter_method="dynamic")
    back = fusion.read_ply(ply)
    assert back.tobytes() == vertices.tobytes() and len(back) > 3000
    cams = [formats.read_camera_parameters(str(folder / "cams" / ("%08d_cam.txt" % i))) for i in ids]
    decoded = np.stack([formats.read_img(str(folder / "images" / ("%08d.jpg" % i))) for i in ids])
    res = fusion.fuse_scene(sc["depths"], sc["conf"], decoded, [c[0] for c in cams], [c[1] for c in cams], pairs, 0.3, 2,
                            device=DEV, method="dynamic")
    assert res.vertices().tobytes() == back.tobytes()
    for k, (r, _) in enumerate(pairs):
        for name in ("photo", "geo", "final"):
            png = np.array(Image.open(str(out / "mask" / ("%08d_%s.png" % (ids[r], name)))))
            assert png.dtype == np.uint8 and np.array_equal(png > 0, res[name + "_mask"][k].cpu().numpy()), (r, name)
    fixed = fusion.filter_depth(str(folder), str(folder), str(out), str(tmp_path / "fixed.ply"), conf=0.3, thres_view=2)
    assert len(fixed) != len(back)                                                # the keyword chose another rule


def test_reconstruct_scan_dynamic_equals_infer_scan_then_fuse_scene(shipped_cfg, checkpoint, tmp_path):
    """A Tanks-like scan with short source lists, from decoded files to a cloud in one call.  (Random weights: thres_view 1
    and wide bases keep the masks non-trivial; level 1 is then the fixed rule's single vote.)"""
    model = MVS4net(**shipped_cfg)
    model.load_state_dict(checkpoint, strict=True)
    model = model.to(DEV).eval()
    root = str(tmp_path)
    DC.write_dataset_folder(root, "Family", DC.dataset_scan([(184, 128)] * 6, seed=31), SS.PAIRS)
    d = SS.decode_all(root, "Family", "cams", None, 6)
    kw = dict(nviews=SS.NVIEWS, depth_range_kind="min_max", crop_rows=(28, 28), short_sources="fewer_views")
    conf, thres_view, bases = 0.05, 1, dict(pix_base=1.0, rel_base=0.01)
    got = scan.reconstruct_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS, conf=conf,
                                thres_view=thres_view, fusion="dynamic", **bases, **kw)
    inferred = scan.infer_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS, **kw)
    refs = np.asarray(inferred["ref_views"])
    assert refs.tolist() == [0, 1, 2, 3, 4] and got.scan["stats"]["short_views"] == 2
    want = fusion.fuse_scene(inferred["depth"], inferred["photometric_confidence"], inferred["images"][torch.from_numpy(refs).to(DEV)],
                             inferred["Ks"][refs], inferred["Es"][refs], SS.WITH_SOURCES, conf, thres_view, device=DEV,
                             method="dynamic", **bases)
    n = len(got["points"])
    print("reconstruct_scan, dynamic, Tanks-like: %d points of %d pixels" % (n, 5 * 128 * 128))
    assert 0 < n < 5 * 128 * 128 and "geo_level" in got
    same_bytes(got, want)
    with pytest.raises(RuntimeError, match="unknown fusion method"):
        scan.reconstruct_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS, fusion="gipuma", **kw)
