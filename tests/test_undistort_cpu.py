"""Undistortion of a scan without a GPU: the host build of csrc/undistort_math.h against an independent
NumPy restatement (another evaluation order) and scipy's map_coordinates, the readers with ``distortion="keep"`` and the argument
checks."""
import numpy as np
import pytest
import torch

from mvster_amd import sfm
from tests import sfm_cases as S
from tests import undistort_cases as U

NAMES = ("A", "A_plus", "B", "C", "Z")


@pytest.fixture(scope="module")
def hm():
    return U.load_undistort_hostmath()


def _ulps(got, want):
    return (np.abs(got - want) / np.spacing(np.abs(want))).max()


# ---- distortion and its inverse ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_distort_is_within_4_ulp_of_numpy(hm, name):
    c = U.CAMERAS[name]
    u, v = U.grid(c)
    assert len(u) == 31 * 31 and np.abs(u).max() > 0.5
    gu, gv = U.distort_host(hm, c, u, v)
    wu, wv = U.distort_numpy(c, u, v)
    worst = max(_ulps(gu, wu), _ulps(gv, wv))
    print("%s: distort differs from NumPy by at most %.1f ulp" % (name, worst))
    assert worst <= 4.0
    if name != "Z":
        assert np.abs(gu - u).max() > 1e-3                                      # (there is distortion)


@pytest.mark.parametrize("name", NAMES)
def test_undistort_residual_and_round_trip(hm, name):
    c = U.CAMERAS[name]
    assert hm.hm_und_newton_steps() == 10
    ud, vd = U.grid(c)                                                          # the grid as distorted positions
    u, v, res = U.undistort_host(hm, c, ud, vd)
    wu, wv, wres = U.undistort_numpy(c, ud, vd)
    print("%s: residual %.2e (NumPy's %.2e), against NumPy's solution %.2e" % (name, res.max(), wres.max(),
                                                                               max(np.abs(u - wu).max(), np.abs(v - wv).max())))
    assert res.max() <= 1e-14 and max(np.abs(u - wu).max(), np.abs(v - wv).max()) <= 1e-13
    fu, fv = U.distort_numpy(c, u, v)
    assert max(np.abs(fu - ud).max(), np.abs(fv - vd).max()) <= 1e-14           # the residual, by the restatement
    gu, gv = U.distort_host(hm, c, ud, vd)                                      # the grid as undistorted positions, and back
    bu, bv, bres = U.undistort_host(hm, c, gu, gv)
    assert bres.max() <= 1e-14 and max(np.abs(bu - ud).max(), np.abs(bv - vd).max()) <= 1e-13


def test_a_fold_over_camera_reports_its_residual(hm):
    ud, vd = U.grid(U.CAM_FOLD)
    _, _, res = U.undistort_host(hm, U.CAM_FOLD, ud, vd)
    assert (res > sfm.RESIDUAL_BOUND).any() and np.isinf(res).any() and not np.isnan(res).any()
    near = (ud * ud + vd * vd) < 0.03                                           # close to the axis the lens still inverts
    assert near.sum() > 20 and res[near].max() <= 1e-14
    out = U.cameras_host(hm, U.CAM_FOLD)[0]
    assert out[6] > sfm.RESIDUAL_BOUND and out[7] > 0
    with pytest.raises(RuntimeError, match="camera row 0.*cannot be inverted over the image"):
        sfm._cameras_of("undistorted_cameras", U.cameras_host(hm, U.CAM_FOLD))
    # a non-finite point, and a record that is no camera
    _, _, bad = U.undistort_host(hm, U.CAM_A, np.array([np.nan, np.inf, 0.1]), np.array([0.0, 0.0, np.nan]))
    assert np.isinf(bad).all()
    none = U.CAM_A.copy()
    none[0] = 7.0
    assert np.isinf(U.cameras_host(hm, none)[0, 6]) and (U.cameras_host(hm, none)[0, :6] == 0).all()


# ---- the undistorted camera --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("blank", [0.0, 1.0])
def test_undistorted_camera_equals_numpy(hm, name, blank):
    c = U.CAMERAS[name]
    got = U.cameras_host(hm, c, blank)[0]
    wn, hn, cx, cy, sw, sh = U.camera_numpy(c, blank)
    print("%s blank %g: scale W = %.4f, scale H = %.4f -> %d x %d" % (name, blank, sw, sh, wn, hn))
    assert (int(got[0]), int(got[1])) == (wn, hn) and got[0] == int(got[0]) and got[1] == int(got[1])
    assert got[2] == c[3] and got[3] == c[4] and abs(got[4] - cx) <= 1e-12 and abs(got[5] - cy) <= 1e-12
    assert got[6] <= 1e-14 and got[7] == 0
    if name == "A_plus":
        assert wn < U.W and hn < U.H                                            # (the output is smaller than the source)


def test_the_sizes_of_the_prototype():
    for name, want in (("A", 166.99), ("A_plus", 151.76), ("B", 171.44), ("C", 175.88)):
        assert abs(U.camera_numpy(U.CAMERAS[name])[4] - want) < 0.006


@pytest.mark.parametrize("name", NAMES)
def test_scale_clamps_and_a_given_scale(hm, name):
    c = U.CAMERAS[name]
    one = U.cameras_host(hm, c, 0.0, 1.0, 1.0)[0]
    assert tuple(one[:6]) == (U.W, U.H, c[3], c[4], c[5], c[6])                 # both clamps reached: scale 1
    lo, hi = U.cameras_host(hm, c, 0.0, 1.5, 2.0)[0], U.cameras_host(hm, c, 0.0, 0.2, 0.5)[0]
    assert tuple(lo[:2]) == (240, 180) and tuple(hi[:2]) == (80, 60)
    given = U.cameras_host(hm, c, scale=(0.77, 1.31))[0]
    wn, hn, cx, cy, _, _ = U.camera_numpy(c, scale=(0.77, 1.31))
    assert (given[0], given[1]) == (wn, hn) and abs(given[4] - cx) <= 1e-12 and abs(given[5] - cy) <= 1e-12 and given[6] == 0


# ---- images --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,blank", [("A", 0.0), ("A", 1.0), ("A_plus", 0.0), ("B", 0.5), ("C", 0.0), ("C", 1.0)])
def test_images_against_map_coordinates(hm, name, blank):
    from scipy import ndimage
    c = U.CAMERAS[name]
    o = U.cameras_host(hm, c, blank)[0]
    src = U.image(U.H, U.W, seed=3)
    dst, valid = U.image_host(hm, src, c, o)
    sx, sy = U.sources_numpy(c, o)
    gx, gy = U.sources_host(hm, c, o)
    assert max(np.abs(gx - sx).max(), np.abs(gy - sy).max()) <= 1e-10           # pixels; the restatement sums in another order
    inside = (sx >= 0) & (sx <= U.W - 1) & (sy >= 0) & (sy <= U.H - 1)
    edge = (np.minimum(np.abs(sx), np.abs(sx - (U.W - 1))) < 1e-9) | (np.minimum(np.abs(sy), np.abs(sy - (U.H - 1))) < 1e-9)
    assert not edge.any() and np.array_equal(valid.astype(bool), inside)       # (no pixel sits on the edge of validity)
    if blank == 0.0:                                                            # (the rule is per axis: a corner pixel may still look outside)
        assert valid.mean() > 0.995 and valid[2:-2, 2:-2].all()
    else:
        assert not valid.all() and valid.mean() > 0.5
    worst = 0.0
    for k in range(3):
        want = ndimage.map_coordinates(src[..., k].astype(np.float64), [sy[inside], sx[inside]], order=1, mode="nearest")
        worst = max(worst, np.abs(dst[..., k][inside].astype(np.float64) - want).max())
    print("%s blank %g: %d x %d, %.1f%% valid, max |byte - float| = %.6f" % (name, blank, o[0], o[1], 100 * valid.mean(), worst))
    assert worst <= 0.5 + 1e-9
    assert (dst[~inside] == 0).all()
    assert len(np.unique(dst)) > 200                                            # (a real picture came out)


def test_identity_gives_the_source_back(hm):
    o = U.cameras_host(hm, U.CAM_Z, scale=(1.0, 1.0))[0]
    assert tuple(o[:6]) == (U.W, U.H, U.F, U.F, U.CX, U.CY)
    src = U.image(U.H, U.W, seed=5)
    dst, valid = U.image_host(hm, src, U.CAM_Z, o)
    ok = valid.astype(bool)
    assert np.array_equal(dst[ok], src[ok])
    assert ok[1:-1, 1:-1].all() and (dst[~ok] == 0).all()                       # only the outermost ring may be invalid


def test_small_and_odd_images(hm):
    """7 x 5 and 13 x 9 sources (row bytes no multiple of 4), 1 x 1 and 2 x 3: the host build against the restatement"""
    for w, h in ((7, 5), (13, 9), (2, 3), (1, 1)):
        c = U.small(U.CAM_C, w, h)
        o = U.cameras_host(hm, c, 1.0)[0]
        assert o[6] <= 1e-14 and o[0] >= 1 and o[1] >= 1
        src = U.image(h, w, seed=w)
        dst, valid = U.image_host(hm, src, c, o)
        sx, sy = U.sources_numpy(c, o)
        inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        assert np.array_equal(valid.astype(bool), inside) and (dst[~inside] == 0).all()


# ---- the readers ----------------------------------------------------------------------------------------------------------------------

def _raw_with(cameras, seed=31):
    """``sfm_cases.synthetic_model`` with the given {camera id: (model, params)}, its views dealt out among them"""
    raw = S.synthetic_model(V=9, P=120, seed=seed, model=2)
    ids = sorted(cameras)
    raw["cameras"] = {cid: (cameras[cid][0], U.W, U.H, list(cameras[cid][1])) for cid in ids}
    raw["images"] = [im[:3] + (ids[im[0] % len(ids)],) + im[4:] for im in raw["images"]]
    return raw


def test_keep_reads_text_and_binary_to_the_same_table(tmp_path):
    raw = _raw_with({3: U.COLMAP["A"], 8: U.COLMAP["B"], 5: U.COLMAP["C"]})
    S.write_text(raw, str(tmp_path / "t"))
    S.write_binary(raw, str(tmp_path / "b"))
    text, binary = (sfm.read_sfm_model(str(tmp_path / sub), distortion="keep") for sub in ("t", "b"))
    U.assert_bytes(text["camera_table"], binary["camera_table"])
    U.assert_bytes(text["camera_row"], binary["camera_row"])
    U.assert_bytes(text["camera_table"], np.stack([U.CAM_A, U.CAM_C, U.CAM_B]))        # by ascending camera id: 3, 5, 8
    assert text["camera_row"].dtype == np.int32
    assert np.array_equal(text["camera_row"], np.searchsorted([3, 5, 8], text["camera_ids"]))
    assert set(text["camera_row"]) == {0, 1, 2}
    v = int(np.nonzero(text["camera_ids"] == 5)[0][0])
    assert text["K"][v, 0, 0] == U.F and text["K"][v, 1, 1] == 141.4 and text["K"][v, 0, 2] == U.CX and tuple(text["sizes"][v]) == (U.H, U.W)
    for sub in ("t", "b"):                                                     # the default still raises
        with pytest.raises(RuntimeError, match="image_undistorter"):
            sfm.read_sfm_model(str(tmp_path / sub))
    with pytest.raises(RuntimeError, match="distortion"):
        sfm.read_sfm_model(str(tmp_path / "t"), distortion="drop")


def test_keep_still_refuses_an_unknown_model_and_takes_pinholes(tmp_path):
    raw = _raw_with({3: U.COLMAP["A"], 4: (6, [140.0] * 12)})
    S.write_text(raw, str(tmp_path / "t"))
    S.write_binary(raw, str(tmp_path / "b"))
    for sub in ("t", "b"):
        for mode in ("raise", "keep"):
            with pytest.raises(RuntimeError, match="image_undistorter"):
                sfm.read_sfm_model(str(tmp_path / sub), distortion=mode)
    bad = _raw_with({3: (2, [U.F, U.CX, U.CY, float("nan")])})
    S.write_binary(bad, str(tmp_path / "n"))
    with pytest.raises(RuntimeError, match="not finite"):
        sfm.read_sfm_model(str(tmp_path / "n"), distortion="keep")
    pin = _raw_with({3: (1, [U.F, 141.4, U.CX, U.CY]), 4: (0, [U.F, U.CX, U.CY])})
    S.write_text(pin, str(tmp_path / "p"))
    table = sfm.read_sfm_model(str(tmp_path / "p"), distortion="keep")["camera_table"]
    assert tuple(table[0]) == (4, U.W, U.H, U.F, 141.4, U.CX, U.CY, 0, 0, 0, 0, 0) and tuple(table[1]) == tuple(U.CAM_Z)


# ---- the argument checks ------------------------------------------------------------------------------------------------------------

def test_argument_checks_come_before_the_device():
    table = np.stack([U.CAM_A, U.CAM_C])
    img = np.zeros((U.H, U.W, 3), np.uint8)
    for kw in (dict(blank_pixels=-0.1), dict(blank_pixels=1.5), dict(blank_pixels=float("nan")), dict(min_scale=0.0),
               dict(min_scale=3.0), dict(max_scale=float("inf"))):
        with pytest.raises(RuntimeError, match="blank_pixels|min_scale"):
            sfm.undistorted_cameras(table, **kw)
    for scale in ((1.0,), (0.0, 1.0), (1.0, float("nan")), 2.0, (1.0, 2000.0)):
        with pytest.raises(RuntimeError, match="scale"):
            sfm.undistorted_cameras(table, scale=scale)
    for bad in (table[:, :11], np.zeros((0, 12)), np.where(np.arange(12) == 0, 1.0, table), np.where(np.arange(12) == 1, 0.0, table),
                np.where(np.arange(12) == 7, np.nan, table), np.where(np.arange(12) == 2, 12.5, table)):
        with pytest.raises(RuntimeError, match="camera"):
            sfm.undistorted_cameras(bad)
    for chunk in (0, -1, 2.5):
        with pytest.raises(RuntimeError, match="chunk_bytes"):
            sfm.undistort_images([img], table, [0], chunk_bytes=chunk)
    with pytest.raises(RuntimeError, match="its camera .row 1. says 120x160"):
        sfm.undistort_images([img, img[:100]], table, [0, 1])
    with pytest.raises(RuntimeError, match=r"uint8 \[H,W,3\]"):
        sfm.undistort_images([img.astype(np.float32)], table, [0])
    with pytest.raises(RuntimeError, match=r"uint8 \[H,W,3\]"):
        sfm.undistort_images([torch.zeros(U.H, U.W, dtype=torch.uint8)], table, [0])
    for rows in ([2], [-1], [0, 0]):
        with pytest.raises(RuntimeError, match="camera_row"):
            sfm.undistort_images([img], table, rows)
    with pytest.raises(RuntimeError, match="camera_row"):
        sfm.undistort_points(table, [0, 2], np.zeros((2, 2)))
    with pytest.raises(RuntimeError, match="camera_row"):
        sfm.distort_points(table, [0], np.zeros((2, 2)))
    with pytest.raises(RuntimeError, match=r"\[N,2\] float64"):
        sfm.undistort_points(table, [0], np.zeros((1, 3)))
    with pytest.raises(RuntimeError, match=r"cameras\[\"table\"\]"):
        sfm.undistort_images([img], table, [0], cameras=dict(table=np.zeros((1, 8))))
    with pytest.raises(RuntimeError, match="blank_pixels"):
        sfm.scan_from_sfm("nowhere", "nowhere", undistort=True, blank_pixels=2.0)
    if not torch.cuda.is_available():
        for call in (lambda: sfm.undistorted_cameras(table), lambda: sfm.undistort_points(table, [0], np.zeros((1, 2))),
                     lambda: sfm.distort_points(table, [1], np.zeros((1, 2))), lambda: sfm.undistort_images([img], table, [0])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_assemble_scan_keeps_its_defaults_and_takes_the_new_arguments(tmp_path):
    raw = S.synthetic_model(V=6, P=80, seed=2, model=1)
    S.write_text(raw, str(tmp_path))
    model = sfm.read_sfm_model(str(tmp_path))
    graph = S.graph_host(S.load_sfm_hostmath(), S.arrays_of(model), num_src=3)
    load = lambda v: np.full((120, 160, 3), v, np.uint8)
    plain = sfm.assemble_scan(model, graph, load)
    assert "valid" not in plain and plain["Ks"][0, 0, 0] == np.float32(140.0 / 4)
    K = model["K"].copy()
    K[:, 0, 2] += 4.0
    seen = {}

    def transform(images, keep):
        seen["keep"] = list(keep)
        return [im[:100] for im in images], dict(valid=[np.ones((100, 160), np.uint8)] * len(images))
    other = sfm.assemble_scan(model, graph, load, K=K, transform=transform)
    assert len(seen["keep"]) == len(other["images"]) == len(other["valid"]) and other["images"][0].shape == (100, 160, 3)
    assert np.array_equal(other["Ks"][:, 0, 2], plain["Ks"][:, 0, 2] + 1.0) and other["pairs"] == plain["pairs"]
