"""Undistortion of a scan on the GPU: csrc/geo_undistort.hip byte for byte against the host build of
csrc/undistort_math.h -- cameras, points, images and their masks -- at the shapes where the kernels can go wrong, a second run
byte for byte against the first, and one scan from a distorted COLMAP text model through ``reconstruct_scan``."""
import os

import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, _lib, scan, sfm
from tests import sfm_cases as S
from tests import undistort_cases as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hm():
    return U.load_undistort_hostmath()


# ---- cameras --------------------------------------------------------------------------------------------------------------------------

def _device_cameras(table, **kw):
    table = np.atleast_2d(table)
    dev = torch.from_numpy(np.ascontiguousarray(table)).to(DEV)
    out = torch.empty(len(table), 8, device=DEV, dtype=torch.float64)
    scale = kw.get("scale")
    sx, sy = scale if scale is not None else (1.0, 1.0)
    _lib.check(_lib.load().mvster_undistort_cameras(dev.data_ptr(), len(table), kw.get("blank", 0.0), kw.get("min_scale", 0.2),
                                                    kw.get("max_scale", 2.0), int(scale is not None), sx, sy, out.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "undistort_cameras")
    return out.cpu().numpy()


def test_cameras_equal_the_host_build(hm):
    table = np.stack([U.CAM_A, U.CAM_A_PLUS, U.CAM_B, U.CAM_C, U.CAM_Z])
    for kw in (dict(), dict(blank=1.0), dict(blank=0.3, min_scale=1.0, max_scale=1.0), dict(scale=(0.77, 1.31))):
        got, again = _device_cameras(table, **kw), _device_cameras(table, **kw)
        U.assert_bytes(got, U.cameras_host(hm, table, kw.get("blank", 0.0), kw.get("min_scale", 0.2), kw.get("max_scale", 2.0),
                                           kw.get("scale")), kw)
        U.assert_bytes(again, got, (kw, "second run"))
    assert _lib.last_kernel() == "undistort_camera_kernel"
    cams = sfm.undistorted_cameras(table, device=DEV)
    want = U.cameras_host(hm, table)
    U.assert_bytes(cams["table"], want)
    assert np.array_equal(cams["sizes"], want[:, [1, 0]].astype(np.int64)) and np.array_equal(cams["K"][:, 0, 2], want[:, 4])
    assert np.array_equal(cams["K"][:, 1, 1], table[:, 4]) and (cams["residual"] <= 1e-14).all()
    assert tuple(cams["sizes"][0]) == (122, 166) and tuple(cams["sizes"][1]) == (113, 151)


def test_cameras_with_fewer_border_points_than_lanes(hm):
    table = np.stack([U.small(U.CAM_C, 1, 1), U.small(U.CAM_A, 2, 3), U.small(U.CAM_B, 3, 2), U.CAM_FOLD])
    for blank in (0.0, 1.0):
        got, again = _device_cameras(table, blank=blank), _device_cameras(table, blank=blank)
        U.assert_bytes(got, U.cameras_host(hm, table, blank), blank)
        U.assert_bytes(again, got, "second run")
    assert got[3, 6] == np.inf and got[3, 7] > 0 and (got[:3, 0] >= 1).all()
    with pytest.raises(RuntimeError, match="camera row 3.*cannot be inverted over the image"):
        sfm.undistorted_cameras(table, device=DEV)


# ---- points --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_points_equal_the_host_build(hm, N):
    rng = np.random.RandomState(N)
    table = np.stack([U.CAM_A, U.CAM_C])
    rows = rng.randint(0, 2, N).astype(np.int32)
    xy = np.stack([rng.rand(N) * U.W, rng.rand(N) * U.H], 1)
    got, res = sfm.undistort_points(table, rows, xy, device=DEV)
    again, res2 = sfm.undistort_points(table, rows, torch.from_numpy(xy).to(DEV), device=DEV)
    want, wres = U.points_host(hm, table, rows, 1, xy)
    U.assert_bytes(got.cpu().numpy(), want)
    U.assert_bytes(res.cpu().numpy(), wres)
    assert torch.equal(again, got) and torch.equal(res2, res) and wres.max() <= 1e-14
    assert _lib.last_kernel() == "undistort_points_kernel"
    back, back2 = sfm.distort_points(table, rows, got, device=DEV), sfm.distort_points(table, rows, got, device=DEV)
    U.assert_bytes(back.cpu().numpy(), U.points_host(hm, table, rows, 0, want)[0])
    assert torch.equal(back, back2) and np.abs(back.cpu().numpy() - xy).max() <= 1e-13 * 141.4      # (1e-13 normalised, in pixels)


# ---- images --------------------------------------------------------------------------------------------------------------------------

def _image_case(hm):
    """Views of A (160 x 120), A+, and C on a 7 x 5 and a 13 x 9 source -> (images, table, rows, cameras, wanted images and masks)"""
    table = np.stack([U.CAM_A, U.CAM_A_PLUS, U.small(U.CAM_C, 7, 5), U.small(U.CAM_C, 13, 9)])
    rows = np.array([0, 1, 2, 3, 0, 3], np.int32)
    images = [U.image(int(table[r, 2]), int(table[r, 1]), seed=10 + k) for k, r in enumerate(rows)]
    ucam = U.cameras_host(hm, table, 1.0)                                       # blank 1: invalid pixels in every view
    cameras = sfm._cameras_of("test", ucam)
    want = [U.image_host(hm, im, table[r], ucam[r]) for im, r in zip(images, rows)]
    return images, table, rows, cameras, want


def _assert_views(got, valid, want, what):
    assert len(got) == len(valid) == len(want)
    for k, (g, m, (w, wm)) in enumerate(zip(got, valid, want)):
        g, m = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (g, m))
        U.assert_bytes(g, w, (what, "image", k))
        U.assert_bytes(m, wm, (what, "valid", k))


def test_images_equal_the_host_build(hm):
    images, table, rows, cameras, want = _image_case(hm)
    pixels = [w.shape[0] * w.shape[1] for w, _ in want]
    assert any(p % 4 for p in pixels) and any(w.shape[1] % 4 for w, _ in want)  # partial last groups, groups across row ends
    assert all(not m.all() and m.any() for _, m in want[:2]) and images[2].shape == (5, 7, 3) and images[3].shape == (9, 13, 3)
    got, valid, cams = sfm.undistort_images(images, table, rows, cameras=cameras, device=DEV)
    assert _lib.last_kernel() == "undistort_images_kernel" and cams["table"] is cameras["table"]
    _assert_views(got, valid, want, "one chunk")
    assert all(isinstance(g, np.ndarray) and g.dtype == np.uint8 for g in got)
    again, valid2, _ = sfm.undistort_images(images, table, rows, cameras=cameras, device=DEV)
    _assert_views(again, valid2, want, "second run")
    # three chunks: 160 x 120 x 3 = 57 600 bytes a large view; the small ones ride along
    chunked, valid3, _ = sfm.undistort_images(images, table, rows, cameras=cameras, chunk_bytes=60000, device=DEV)
    _assert_views(chunked, valid3, want, "three chunks")
    tiny, valid4, _ = sfm.undistort_images(images, table, rows, cameras=cameras, chunk_bytes=1, device=DEV)      # a chunk per image
    _assert_views(tiny, valid4, want, "a chunk per image")
    kept, valid5, _ = sfm.undistort_images(images, table, rows, cameras=cameras, keep_on_device=True, device=DEV)
    assert all(torch.is_tensor(t) and t.device.type == "cuda" and t.dtype == torch.uint8 for t in kept + valid5)
    _assert_views(kept, valid5, want, "keep_on_device")
    on_gpu = [torch.from_numpy(im).to(DEV) for im in images]
    from_gpu, valid6, _ = sfm.undistort_images(on_gpu, table, rows, cameras=cameras, device=DEV)
    _assert_views(from_gpu, valid6, want, "GPU tensors in")
    mixed = [t if k % 2 else im for k, (t, im) in enumerate(zip(on_gpu, images))]
    from_mixed, valid7, _ = sfm.undistort_images(mixed, table, rows, cameras=cameras, chunk_bytes=60000, keep_on_device=True, device=DEV)
    _assert_views(from_mixed, valid7, want, "host arrays and GPU tensors mixed")


def test_images_with_the_default_cameras_and_the_identity(hm):
    table = np.stack([U.CAM_B, U.CAM_Z])
    images = [U.image(U.H, U.W, seed=1), U.image(U.H, U.W, seed=2)]
    got, valid, cams = sfm.undistort_images(images, table, [0, 1], device=DEV)
    ucam = U.cameras_host(hm, table)
    U.assert_bytes(cams["table"], ucam)
    _assert_views(got, valid, [U.image_host(hm, im, table[r], ucam[r]) for r, im in enumerate(images)], "defaults")
    one = sfm.undistorted_cameras(table, scale=(1.0, 1.0), device=DEV)
    same, ok, _ = sfm.undistort_images(images[1:], table, [1], cameras=one, device=DEV)
    ok = ok[0].astype(bool)
    assert np.array_equal(same[0][ok], images[1][ok]) and ok[1:-1, 1:-1].all()


# ---- one scan, end to end ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(shipped_cfg, checkpoint):
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    return m.to(DEV).eval()


def test_distorted_text_model_through_reconstruct_scan(hm, model, tmp_path):
    """Lens A (SIMPLE_RADIAL k = -0.12, the same field of view) on 192 x 144 photographs: the undistorted images are 200 x 147,
    which the scan entry brings to 128 x 192, the smallest size the cascade is run at elsewhere in the suite."""
    pytest.importorskip("PIL.Image")
    V, Ws, Hs, s = 7, 192, 144, 1.2
    raw = S.synthetic_model(V=V, P=400, seed=6, rings=2, dropout=0.2, width=Ws, height=Hs, focal=U.F * s, model=2)
    raw["cameras"] = {3: (2, Ws, Hs, [U.F * s, U.CX * s, U.CY * s, -0.12])}
    mdir, idir = str(tmp_path / "sparse"), str(tmp_path / "images")
    S.write_text(raw, mdir)
    photos = S.write_images(raw, idir, seed=9)
    with pytest.raises(RuntimeError, match="image_undistorter"):
        sfm.scan_from_sfm(mdir, idir, num_src=4, device=DEV)
    got = sfm.scan_from_sfm(mdir, idir, num_src=4, device=DEV, undistort=True, keep_on_device=True)
    kept = sfm.read_sfm_model(mdir, distortion="keep")
    table = kept["camera_table"]
    ucam = U.cameras_host(hm, table)
    Hd, Wd = int(ucam[0, 1]), int(ucam[0, 0])
    assert (Hd, Wd) == (147, 200) and len(got["images"]) == len(got["valid"]) == V and got["dropped_views"] == []
    for k, name in enumerate(got["names"]):
        w, wm = U.image_host(hm, photos[name], table[0], ucam[0])
        assert got["images"][k].device.type == "cuda"
        U.assert_bytes(got["images"][k].cpu().numpy(), w, name)
        U.assert_bytes(got["valid"][k].cpu().numpy(), wm, name)
    K = np.array([[ucam[0, 2], 0, ucam[0, 4]], [0, ucam[0, 3], ucam[0, 5]], [0, 0, 1]], np.float32)
    K[:2] /= 4.0
    assert np.array_equal(got["Ks"], np.tile(K, (V, 1, 1))) and got["pairs"] == sfm.view_graph(kept, num_src=4, device=DEV)["pairs"]
    res = scan.reconstruct_scan(model, got["images"], got["Ks"], got["Es"], got["depth_ranges"], got["pairs"], conf=0.05,
                                thres_view=1, nviews=5, depth_range_kind="min_max", short_sources="fewer_views", max_h=192, max_w=256)
    depth = res.scan["depth"]
    assert tuple(depth.shape) == (V, 128, 192) and bool(torch.isfinite(depth).all()) and bool((depth > 0).all())
    # the folder round trip, from host copies of the images
    host = dict(got, images=[im.cpu().numpy() for im in got["images"]])
    root = str(tmp_path / "scan")
    sfm.write_scan_folder(host, root, ndepths=48)
    back = scan.read_scan_folder(root, "", dataset="tanks")
    assert back["view_ids"] == got["view_ids"] and np.array_equal(back["Ks"], got["Ks"]) and np.array_equal(back["Es"], got["Es"])
    assert back["depth_ranges"] == got["depth_ranges"] and back["pairs"] == got["pairs"]
    assert all(im.shape == (Hd, Wd, 3) for im in back["images"])
    sfm.write_scan_folder(got, str(tmp_path / "scan2"), ndepths=48)            # GPU tensors are brought to the host
    assert os.path.exists(os.path.join(str(tmp_path / "scan2"), "images", "{:0>8}.jpg".format(got["view_ids"][0])))
