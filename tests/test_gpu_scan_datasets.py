"""Tanks and Temples / ETH3D scans on the GPU: ``ops.load_pack_images_u8`` (per-view crop + resize + pack in one launch) bit
for bit against ``formats.resize_linear`` on the sliced windows, ``infer_scan`` with ``crop_rows`` / ``img_wh`` /
``depth_range_kind="min_max"`` bit for bit against the per-sample forward on ``load_tanks_sample`` / ``load_eth3d_sample``,
``reconstruct_scan`` against ``fusion.fuse_scene`` on the per-sample maps, and the folder entry points."""
import os

import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, formats, fusion, ops, scan
from tests import scan_cases as SC
from tests import scan_dataset_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model(shipped_cfg, checkpoint):
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    return m.to(DEV).eval()


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def _images(sizes, seed):
    rng = np.random.RandomState(seed)
    views = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    views[0][0, :min(sizes[0][1], 256), 0] = np.arange(min(sizes[0][1], 256))     # every level at least once where Ws allows
    return views


def _host(views, Hd, Wd, crop):
    """formats.resize_linear(u8 / 255) on the sliced window, per view -> (RGB0 [V,1,Hd,Wd,4], uint8 [V,Hd,Wd,3])."""
    top, bottom, left, right = crop
    out = np.zeros((len(views), 1, Hd, Wd, 4), dtype=np.float32)
    for v, im in enumerate(views):
        win = im[top:im.shape[0] - bottom, left:im.shape[1] - right]
        out[v, 0, :, :, :3] = formats.resize_linear(win.astype(np.float32) / 255.0, Hd, Wd)
    return out, np.clip(out[:, 0, :, :, :3] * np.float32(255.0), 0, 255).astype(np.uint8)


KERNEL_CASES = {
    # name -> (native sizes, crop, (Hd, Wd))
    "a_tanks_like": ([(120, 128)] * 4, (28, 28, 0, 0), (64, 128)),
    "b_unaligned_window_and_pitch": ([(120, 131)] * 4, (28, 28, 1, 2), (64, 128)),
    "c_eth3d_like_mixed_sizes": ([(150, 200), (141, 211), (128, 256), (64, 128), (64, 300)], (0, 0, 0, 0), (64, 128)),
    "d_uniform": ([(150, 200)] * 3, (0, 0, 0, 0), (64, 128)),
    "e_one_view": ([(141, 211)], (0, 0, 0, 0), (64, 128)),
    "e_one_view_cropped": ([(120, 131)], (28, 28, 1, 2), (64, 128)),
    "crop_then_resize_with_area": ([(160, 280), (150, 230)], (10, 22, 12, 12), (64, 128)),   # 128x256 (2:1) and 118x206 windows
}


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_load_pack_equals_resize_linear_on_the_windows(name):
    sizes, crop, (Hd, Wd) = KERNEL_CASES[name]
    views = _images(sizes, seed=len(name))
    want, want_u8 = _host(views, Hd, Wd, crop)
    got, got_u8 = ops.load_pack_images_u8(views, Hd, Wd, crop=crop, want_u8=True)          # host views: one ragged upload
    alone = ops.load_pack_images_u8(views, Hd, Wd, crop=crop)                               # the instantiation without the 8-bit output
    on_gpu = ops.load_pack_images_u8([torch.from_numpy(v).to(DEV) for v in views], Hd, Wd, crop=crop, want_u8=True)
    torch.cuda.synchronize()
    V = len(views)
    assert got.shape == (V, 1, Hd, Wd, 4) and got.dtype == torch.float32 and got.is_cuda
    assert got_u8.shape == (V, Hd, Wd, 3) and got_u8.dtype == torch.uint8
    bad = int((got.cpu().numpy().view(np.int32) != want.view(np.int32)).sum())
    bad_u8 = int((got_u8.cpu().numpy() != want_u8).sum())
    print("load_pack %s: differing float words %d of %d, bytes %d" % (name, bad, want.size, bad_u8))
    assert bad == 0 and bad_u8 == 0
    assert torch.equal(alone, got) and torch.equal(on_gpu[0], got) and torch.equal(on_gpu[1], got_u8)
    top, bottom, left, right = crop
    if all((h - top - bottom, w - left - right) == (Hd, Wd) for h, w in sizes):
        # a pure crop: the bits of pack_images_u8 on the slices, and the 8-bit output is the slices themselves
        slices = np.stack([v[top:v.shape[0] - bottom, left:v.shape[1] - right] for v in views])
        dev = torch.from_numpy(np.ascontiguousarray(slices)).to(DEV)
        assert torch.equal(got, ops.pack_images_u8(dev)) and torch.equal(got_u8, dev)
    if len(set(sizes)) == 1:
        stack = torch.from_numpy(np.stack(views)).to(DEV)                                   # a GPU stack (read in place where aligned)
        again = ops.load_pack_images_u8(stack, Hd, Wd, crop=crop, want_u8=True)
        assert torch.equal(again[0], got) and torch.equal(again[1], got_u8)
        if not any(crop):
            # the wrapper for one common size: its descriptors are the uniform ones with full-image windows
            wrapped, wrapped_u8 = ops.resize_pack_images_u8(stack, Hd, Wd, want_u8=True)
            assert torch.equal(got, wrapped) and torch.equal(got_u8, wrapped_u8)


def test_load_pack_refuses_what_no_loader_does():
    views = [np.zeros((128, 128, 3), np.uint8)]
    for Hd, Wd in ((256, 128), (128, 192), (100, 128), (0, 64)):
        with pytest.raises(RuntimeError, match="load_pack_images_u8"):
            ops.load_pack_images_u8(views, Hd, Wd)
    with pytest.raises(RuntimeError, match="smaller than the target"):
        ops.load_pack_images_u8(views, 128, 128, crop=(1, 0, 0, 0))
    with pytest.raises(RuntimeError, match=r"uint8 \[H,W,3\]"):
        ops.load_pack_images_u8([views[0].astype(np.float32)], 64, 64)


# ---- scans -----------------------------------------------------------------------------------------------------------------
def _forward(model, sample):
    out = model([torch.from_numpy(np.ascontiguousarray(i[None])).to(DEV) for i in sample["imgs"]],
                {k: torch.from_numpy(np.ascontiguousarray(v[None])).to(DEV) for k, v in sample["proj_matrices"].items()},
                torch.from_numpy(sample["depth_values"][None]).to(DEV))
    return out["depth"][0].clone(), out["photometric_confidence"][0].clone()


def _prepared_u8(sample_imgs):
    """The pixels the reference writes to images/ (test_mvs4.py:262-264) for one prepared float image [3,H,W]."""
    return np.clip(np.transpose(sample_imgs, (1, 2, 0)) * np.float32(255), 0, 255).astype(np.uint8)


NVIEWS = 3
PAIRS_5 = SC.ring_pairs(5, 3)                                                  # three sources each: cut to nviews - 1 = 2


@pytest.fixture(scope="module")
def tanks(model, tmp_path_factory):
    """5 views of 184x128 -> 128x128 on disk, decoded once, with the per-sample maps of every reference view."""
    root = str(tmp_path_factory.mktemp("tanks"))
    sc = DC.dataset_scan([(184, 128)] * 5, seed=21)
    DC.write_dataset_folder(root, "Family", sc, PAIRS_5)
    decoded = scan.read_scan_folder(root, "Family", dataset="tanks")
    samples = [formats.load_tanks_sample(root, "Family", r, srcs, nviews=NVIEWS) for r, srcs in PAIRS_5]
    return dict(root=root, name="Family", decoded=decoded, samples=samples, maps=[_forward(model, s) for s in samples],
                kw=dict(crop_rows=(28, 28)), size=(128, 128), dataset="tanks")


@pytest.fixture(scope="module")
def eth3d(model, tmp_path_factory):
    """5 views of three native sizes -> img_wh = (128, 128); view 3's cam file has a negative depth_min."""
    root = str(tmp_path_factory.mktemp("eth3d"))
    sc = DC.dataset_scan([(150, 200), (141, 211), (256, 256), (150, 200), (141, 211)], seed=22, negative_min_view=3)
    DC.write_dataset_folder(root, "door", sc, PAIRS_5, cams="cams_1")
    decoded = scan.read_scan_folder(root, "door", dataset="eth3d")
    samples = [formats.load_eth3d_sample(root, "door", r, srcs, nviews=NVIEWS, img_wh=(128, 128)) for r, srcs in PAIRS_5]
    return dict(root=root, name="door", decoded=decoded, samples=samples, maps=[_forward(model, s) for s in samples],
                kw=dict(img_wh=(128, 128)), size=(128, 128), dataset="eth3d")


@pytest.mark.parametrize("which", ["tanks", "eth3d"])
def test_infer_scan_is_bit_equal_to_the_per_sample_forward_on_the_loaders_samples(model, request, which):
    case = request.getfixturevalue(which)
    d, (Hd, Wd) = case["decoded"], case["size"]
    report = {}
    for call in ("first", "second"):
        res = scan.infer_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], d["pairs"], nviews=NVIEWS,
                              depth_range_kind="min_max", **case["kw"])
        torch.cuda.synchronize()
        R = len(res["ref_views"])
        assert R == 5 and res["depth"].shape == res["photometric_confidence"].shape == (R, Hd, Wd)
        bad_d = sum(int((res["depth"][r] != case["maps"][r][0]).sum()) for r in range(R))
        bad_c = sum(int((res["photometric_confidence"][r] != case["maps"][r][1]).sum()) for r in range(R))
        report[call] = (bad_d, bad_c)
        print("infer_scan %s %s call: differing depth %d, confidence %d of %d" % (which, call, bad_d, bad_c, R * Hd * Wd))
    assert all(v == (0, 0) for v in report.values()), report
    # the result carries the adjusted cameras (the loader's stage-4 matrices) and the prepared 8-bit images
    for r, sample in enumerate(case["samples"]):
        assert res["Ks"][r].tobytes() == sample["proj_matrices"]["stage4"][0, 1, :3, :3].tobytes()
        assert res["Es"][r].tobytes() == sample["proj_matrices"]["stage4"][0, 0].tobytes()
    assert torch.is_tensor(res["images"]) and res["images"].is_cuda and res["images"].shape == (5, Hd, Wd, 3)
    got_u8 = res["images"].cpu().numpy()
    for r, sample in enumerate(case["samples"]):
        assert np.array_equal(got_u8[r], _prepared_u8(sample["imgs"][0])), r
    assert res["stats"]["source_bytes"] == sum(im.shape[0] * im.shape[1] * 3 for im in d["images"])
    assert res["stats"]["store_bytes"] == scan.store_bytes(5, Hd, Wd)


def test_reconstruct_scan_equals_fuse_scene_on_the_per_sample_maps(model, tanks):
    d = tanks["decoded"]
    conf, thres_view = 0.05, 1                                               # (random weights: keep the masks non-trivial)
    depth = torch.stack([m[0] for m in tanks["maps"]])
    confidence = torch.stack([m[1] for m in tanks["maps"]])
    images = np.stack([_prepared_u8(s["imgs"][0]) for s in tanks["samples"]])
    Ks = np.stack([s["proj_matrices"]["stage4"][0, 1, :3, :3] for s in tanks["samples"]])
    Es = np.stack([s["proj_matrices"]["stage4"][0, 0] for s in tanks["samples"]])
    want = fusion.fuse_scene(depth, confidence, images, Ks, Es, PAIRS_5, conf, thres_view, device=DEV)
    got = scan.reconstruct_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], d["pairs"], conf=conf,
                                thres_view=thres_view, nviews=NVIEWS, depth_range_kind="min_max", crop_rows=(28, 28))
    n = len(got["points"])
    print("reconstruct_scan, Tanks-like: %d points of %d pixels" % (n, 5 * 128 * 128))
    assert 0 < n < 5 * 128 * 128 and n == len(want["points"])
    assert torch.equal(got["points"], want["points"]) and torch.equal(got["colors"], want["colors"])
    for k in ("photo_mask", "geo_mask", "final_mask"):
        assert torch.equal(got[k], want[k])
    assert torch.equal(got["colors"], torch.from_numpy(images).to(DEV)[got["final_mask"].bool()])


@pytest.mark.parametrize("which", ["tanks", "eth3d"])
def test_folder_round_trip(model, request, tmp_path, which):
    """infer_scan_folder(dataset=...) equals infer_scan on the decoded arrays; write_scan_outputs gives the reference's layout
    with the adjusted cameras and the prepared images."""
    from PIL import Image
    case = request.getfixturevalue(which)
    d, (Hd, Wd) = case["decoded"], case["size"]
    kw = {} if which == "tanks" else case["kw"]                             # (Tanks: crop_rows = (28, 28) is the default)
    res = scan.infer_scan_folder(model, case["root"], case["name"], nviews=NVIEWS, dataset=case["dataset"], **kw)
    direct = scan.infer_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], d["pairs"], nviews=NVIEWS,
                             depth_range_kind="min_max", view_ids=d["view_ids"], **case["kw"])
    for k in ("depth", "photometric_confidence", "images"):
        assert torch.equal(res[k], direct[k]), k
    assert np.array_equal(res["Ks"], direct["Ks"]) and res["view_ids"] == direct["view_ids"] == [0, 1, 2, 3, 4]
    assert torch.equal(res["depth"][2], case["maps"][2][0])
    out = os.path.join(str(tmp_path), "out")
    scan.write_scan_outputs(res, res["images"], out)
    for v in range(5):
        name = "{:0>8}".format(v)
        K, E = formats.read_camera_parameters(os.path.join(out, "cams", name + "_cam.txt"))
        stage4 = case["samples"][v]["proj_matrices"]["stage4"][0]
        assert K.tobytes() == stage4[1, :3, :3].tobytes() and E.tobytes() == stage4[0].tobytes()
        assert Image.open(os.path.join(out, "images", name + ".jpg")).size == (Wd, Hd)
        depth, _ = formats.read_pfm(os.path.join(out, "depth_est", name + ".pfm"))
        assert np.array_equal(depth, res["depth"][v].cpu().numpy())
        assert formats.read_pfm(os.path.join(out, "confidence", name + ".pfm"))[0].shape == (Hd, Wd)
