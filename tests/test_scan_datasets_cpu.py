"""Host side of the Tanks and Temples / ETH3D scan path (no GPU): the min/max cam reader and the stage matrices against a
literal restatement of the two loaders (tests/scan_dataset_cases.py), byte for byte; the descriptor and table builder of
``ops.load_pack_images_u8``; the per-sample comparators ``load_tanks_sample`` / ``load_eth3d_sample``; what ``infer_scan``
refuses before any device work; and that nothing changes without the new keywords."""
import os

import numpy as np
import pytest
import torch

from mvster_amd import formats, ops, scan
from tests import scan_cases as SC
from tests import scan_dataset_cases as DC


def _model():
    from mvster_amd import MVS4net
    from tests.conftest import SHIPPED
    return MVS4net(**SHIPPED).eval()                                         # on the CPU: device work would raise differently


# ---- cam reader ------------------------------------------------------------------------------------------------------------
LINE11 = {"two": "425.0 935.5", "three": "425.0 2.5 935.5", "four": "425.0 2.5 192 905.0", "negative": "-0.75 0.01 256 37.25"}


@pytest.mark.parametrize("name", sorted(LINE11))
def test_minmax_reader_equals_the_loaders_readers(tmp_path, name):
    sc = DC.dataset_scan([(96, 128)], seed=3)
    path = os.path.join(str(tmp_path), "cam.txt")
    K = sc["Kfull"][0] + np.float32(1.0 / 3.0)                               # digits that do not round-trip through float32 trivially
    DC.write_cam_file(path, K.astype(np.float64) + 1e-9, sc["Es"][0].astype(np.float64) - 1e-9, LINE11[name])
    for eth3d in (False, True):
        want = DC.ref_read_cam_file(path, eth3d=eth3d)
        got = formats.read_cam_file_minmax(path, negative_min_to=1 if eth3d else None)
        assert got[0].dtype == got[1].dtype == np.float32 and got[0].shape == (3, 3) and got[1].shape == (4, 4)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert got[2] == want[2] and got[3] == want[3] and type(got[2]) is type(want[2])
        # what the loaders hand to the forward
        assert np.array([got[2], got[3]], dtype=np.float32).tobytes() == np.array([want[2], want[3]], dtype=np.float32).tobytes()
    first, last = float(LINE11[name].split()[0]), float(LINE11[name].split()[-1])
    assert formats.read_cam_file_minmax(path)[2:] == (first, last)
    assert formats.read_cam_file_minmax(path, negative_min_to=1)[2] == (1 if first < 0 else first)
    # the DTU reader on the same file: full-resolution K here, K / 4 there; an interval there
    Kq = formats.read_cam_file(path)[0]
    assert np.array_equal(formats.read_cam_file_minmax(path)[0][:2], Kq[:2] * 4.0)


# ---- stage matrices --------------------------------------------------------------------------------------------------------
def _odd_cameras(V, seed):
    """Intrinsics and extrinsics with full 24-bit mantissas."""
    rng = np.random.RandomState(seed)
    Ks = np.zeros((V, 3, 3), np.float32)
    Ks[:, 0, 0] = 1400 + 300 * rng.rand(V)
    Ks[:, 1, 1] = 1400 + 300 * rng.rand(V)
    Ks[:, 0, 2] = 900 + 100 * rng.rand(V)
    Ks[:, 1, 2] = 500 + 100 * rng.rand(V)
    Ks[:, 0, 1] = rng.rand(V) * 1e-3
    Ks[:, 2, 2] = 1
    Es = rng.randn(V, 4, 4).astype(np.float32)
    Es[:, 3] = (0, 0, 0, 1)
    return Ks, Es


def test_tanks_stage_matrices_carry_the_loaders_bits():
    """stage_proj_matrices(K / 4) == the x 0.125, x 2, x 2, x 2 chain after ``cy - 28``: every factor is a power of two."""
    Ks, Es = _odd_cameras(4, 11)
    want = DC.ref_stage_chain([DC.ref_tanks_intrinsics(K.copy(), 28) for K in Ks], list(Es))
    got = formats.stage_proj_matrices(formats._quarter(formats.crop_intrinsics(Ks, 28, 0)), Es)
    for k in ("stage1", "stage2", "stage3", "stage4"):
        assert got[k].dtype == np.float32 and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(formats.crop_intrinsics(Ks, 28, 0)[:, 1, 2], Ks[:, 1, 2] - np.float32(28))
    assert np.array_equal(formats.crop_intrinsics(Ks, 0, 3)[:, 0, 2], Ks[:, 0, 2] - np.float32(3))
    # ... and through the scan path, whose Ks come and go in the quarter-resolution convention
    Hd, Wd, crop, Kq = scan._dataset_inputs("u8", [(184, 128)] * 4, DC.quarter(Ks), (28, 28), None)
    assert (Hd, Wd, crop) == (128, 128, (28, 28, 0, 0))
    plan = scan.plan_scan(Kq, Es, [(1.0, 2.0)] * 4, SC.ring_pairs(4, 2), nviews=3, depth_range_kind="min_max")
    for k in want:
        assert plan.proj[k].tobytes() == want[k].tobytes(), k


def test_eth3d_stage_matrices_carry_the_loaders_bits_with_per_view_factors():
    Ks, Es = _odd_cameras(3, 12)
    sizes = [(141, 211), (150, 200), (141, 211)]                             # two native sizes: a factor pair per view
    img_wh = (128, 64)
    want = DC.ref_stage_chain([DC.ref_eth3d_intrinsics(K.copy(), img_wh, h, w) for K, (h, w) in zip(Ks, sizes)], list(Es))
    scaled = [formats.scale_intrinsics(K, img_wh[1] / h, img_wh[0] / w) for K, (h, w) in zip(Ks, sizes)]
    got = formats.stage_proj_matrices(formats._quarter(np.stack(scaled)), Es)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert not np.array_equal(got["stage4"][0, 1], got["stage4"][1, 1])
    Hd, Wd, crop, Kq = scan._dataset_inputs("u8", sizes, DC.quarter(Ks), None, img_wh)
    assert (Hd, Wd, crop) == (64, 128, (0, 0, 0, 0))
    plan = scan.plan_scan(Kq, Es, [(1.0, 2.0)] * 3, SC.ring_pairs(3, 2), nviews=3, depth_range_kind="min_max")
    for k in want:
        assert plan.proj[k].tobytes() == want[k].tobytes(), k


# ---- descriptors and tables ------------------------------------------------------------------------------------------------
def test_descriptor_and_table_builder():
    sizes = [(150, 200), (141, 211), (128, 256), (64, 128), (64, 300), (141, 211), (150, 200)]
    Hd, Wd = 64, 128
    desc, tables, total = ops.load_pack_descriptors(sizes, Hd, Wd)
    assert desc.dtype == np.int32 and desc.shape == (7, ops.LOAD_PACK_DESC_WORDS) and tables.dtype == np.int32
    offs = (desc[:, 0].astype(np.int64) & 0xffffffff) | (desc[:, 1].astype(np.int64) << 32)
    end = 0
    for v, (h, w) in enumerate(sizes):
        assert offs[v] % 16 == 0 and offs[v] >= end                          # aligned, not overlapping
        end = offs[v] + h * w * 3
        Hs, Ws, y0, x0, hw, ww, tab, area = desc[v, 2:10]
        assert (Hs, Ws) == (h, w) and (y0, x0, hw, ww) == (0, 0, h, w)
        assert 0 <= y0 and 0 <= x0 and y0 + hw <= Hs and x0 + ww <= Ws        # the window lies inside its image
        assert area == int((h, w) == (128, 256))
        assert not desc[v, 10:].any()
    assert end <= total and total % 16 == 0
    # tables: one per distinct window size that needs one (the 64x128 view needs none), shared between equal sizes
    per = 2 * Wd + 2 * Hd
    assert tables.size == 4 * per
    assert desc[0, 8] == desc[6, 8] and desc[1, 8] == desc[5, 8] and len({int(desc[v, 8]) for v in (0, 1, 2, 4)}) == 4
    for v in (0, 1, 2, 4):
        t = int(desc[v, 8])
        assert t % 4 == 0 and t + per <= tables.size
        sx, fx, sy, fy = formats.resize_tables(sizes[v][0], sizes[v][1], Hd, Wd)
        want = np.concatenate([sx.view(np.int32), fx.view(np.int32), sy.view(np.int32), fy.view(np.int32)])
        assert np.array_equal(tables[t:t + per], want)
        assert sx.max() < sizes[v][1] and sy.max() < sizes[v][0]               # tap indices relative to the window, inside it
    # the builder is memoised; what a caller does to its arrays does not reach the next one
    desc[:], tables[:] = -1, -1
    again = ops.load_pack_descriptors(sizes, Hd, Wd)
    assert again[0][0, 2] == 150 and again[1].min() >= 0 and again[2] == total
    # a crop: the window moves, the taps are those of the window's size; a pure crop has no table at all
    desc, tables, total = ops.load_pack_descriptors([(120, 131)] * 4, 64, 128, crop=(28, 28, 1, 2))
    assert tables.size == 0 and total == 4 * ((120 * 131 * 3 + 15) // 16 * 16)
    assert all(tuple(d[2:10]) == (120, 131, 28, 1, 64, 128, 0, 0) for d in desc)
    desc, tables, _ = ops.load_pack_descriptors([(160, 280)], 64, 128, crop=(10, 22, 12, 12))
    assert tuple(desc[0, 2:10]) == (160, 280, 10, 12, 128, 256, 0, 1) and tables.size == per
    sx = formats.resize_tables(128, 256, 64, 128)[0]
    assert np.array_equal(tables[:Wd], sx.view(np.int32))
    # an offset past 2^31: low and high word
    big, _, total = ops.load_pack_descriptors([(16384, 16384)] * 4, 64, 64)
    offs = (big[:, 0].astype(np.int64) & 0xffffffff) | (big[:, 1].astype(np.int64) << 32)
    assert list(offs) == [k * 16384 * 16384 * 3 for k in range(4)] and total == 4 * 16384 * 16384 * 3 and big[3, 0] < 0
    for bad in (dict(sizes=[(64, 128)], Hd=64, Wd=96), dict(sizes=[(64, 128)], Hd=0, Wd=128),
                dict(sizes=[(150, 200), (63, 200)], Hd=64, Wd=128), dict(sizes=[(150, 200)], Hd=64, Wd=128, crop=(50, 50, 0, 0)),
                dict(sizes=[(150, 200)], Hd=64, Wd=128, crop=(-1, 0, 0, 0))):
        with pytest.raises(RuntimeError, match="load_pack_images_u8"):
            ops.load_pack_descriptors(**bad)


def test_load_pack_entry_is_declared_bound_exported_and_validates_on_the_host():
    """Bad descriptors through the C ABI: the error code comes back before anything is launched (the device pointers here
    are stand-in addresses that nothing dereferences)."""
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvster_hip.h")).read()
    name = "mvster_load_pack_images_u8"
    assert name in _lib.SIGNATURES and hasattr(lib, name) and ("int %s(" % name) in header
    fn = lib.mvster_load_pack_images_u8
    a, b, c, d, e = 1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 36
    Hd, Wd = 64, 128
    desc, tables, total = ops.load_pack_descriptors([(150, 200), (64, 128)], Hd, Wd)

    def call(dh, buf=a, nbytes=total, dev=b, tab=c, words=tables.size, out=d, V=2, Hd=Hd, Wd=Wd):
        dh = np.ascontiguousarray(dh, dtype=np.int32)
        return fn(buf, nbytes, dh.ctypes.data, dev, tab, words, out, e, V, Hd, Wd, None)

    assert call(desc, buf=None) == _lib.ERR_NULL and call(desc, dev=None) == _lib.ERR_NULL
    assert call(desc, out=None) == _lib.ERR_NULL and call(desc, tab=None) == _lib.ERR_NULL
    assert fn(a, total, None, b, c, tables.size, d, e, 2, Hd, Wd, None) == _lib.ERR_NULL
    for kw in (dict(V=0), dict(V=65536), dict(Hd=0), dict(Wd=96), dict(Hd=100), dict(buf=a + 4), dict(tab=c + 8), dict(nbytes=0)):
        assert call(desc, **kw) == _lib.ERR_SHAPE, kw

    def with_(v, word, value):
        bad = desc.copy()
        bad[v, word] = value
        return bad
    for what, bad in (("image past the buffer", with_(1, 0, (total // 16) * 16)), ("misaligned offset", with_(1, 0, desc[1, 0] + 4)),
                      ("negative offset", with_(0, 1, -1)), ("Hs 0", with_(0, 2, 0)), ("Ws -1", with_(0, 3, -1)),
                      ("image larger than the buffer", with_(0, 2, 1 << 20)),
                      ("window below the image", with_(0, 4, 1)), ("window right of the image", with_(0, 5, 1)),
                      ("negative y0", with_(0, 4, -1)), ("window taller than the image", with_(0, 6, 151)),
                      ("enlarging in y", with_(0, 6, 63)), ("enlarging in x", with_(0, 7, 127)),
                      ("table past the blob", with_(0, 8, 4)), ("misaligned table", with_(0, 8, 2)), ("negative table", with_(0, 8, -4)),
                      ("area flag on a window that is not 2x", with_(0, 9, 1))):
        assert call(bad) == _lib.ERR_SHAPE, what
    assert call(desc, words=tables.size - 1) == _lib.ERR_SHAPE
    two, t2, n2 = ops.load_pack_descriptors([(128, 256)], Hd, Wd)
    two[0, 9] = 0
    assert call(two, nbytes=n2, words=t2.size, V=1) == _lib.ERR_SHAPE          # ... and off on one that is
    # the Python entry: shapes first, then the device
    with pytest.raises(RuntimeError, match=r"view 1: expects uint8 \[H,W,3\]"):
        ops.load_pack_images_u8([np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 3), np.float32)], 64, 64)
    with pytest.raises(RuntimeError, match="smaller than the target"):
        ops.load_pack_images_u8([np.zeros((64, 64, 3), np.uint8)], 128, 64)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.load_pack_images_u8([np.zeros((64, 64, 3), np.uint8)], 64, 64)


# ---- sample builders -------------------------------------------------------------------------------------------------------
def test_load_tanks_sample_is_slicing_and_the_loaders_cameras(tmp_path):
    import PIL  # noqa: F401  (the folder helpers need it: missing is a failure, not a skip)
    sc = DC.dataset_scan([(120, 128)] * 4, seed=5)
    pairs = [(0, [1, 2, 3]), (1, [0, 2, 3]), (2, [3, 1, 0]), (3, [2, 1, 0])]
    DC.write_dataset_folder(str(tmp_path), "Family", sc, pairs)
    got = formats.load_tanks_sample(str(tmp_path), "Family", 2, pairs[2][1], nviews=3)     # cut to two sources, not padded
    views = [2, 3, 1]
    assert len(got["imgs"]) == 3 and got["filename"] == "Family/{}/00000002{}"
    intr, extr = [], []
    for i, v in enumerate(views):
        img = formats.read_img(os.path.join(str(tmp_path), "Family", "images", "{:0>8}.jpg".format(v)))
        want = img[28:120 - 28, :, :].transpose(2, 0, 1)
        assert got["imgs"][i].shape == (3, 64, 128) and got["imgs"][i].dtype == np.float32
        assert np.ascontiguousarray(got["imgs"][i]).tobytes() == np.ascontiguousarray(want).tobytes()
        K, E, dmin, dmax = DC.ref_read_cam_file(os.path.join(str(tmp_path), "Family", "cams", "{:0>8}_cam.txt".format(v)))
        intr.append(DC.ref_tanks_intrinsics(K))
        extr.append(E)
        if i == 0:
            assert got["depth_values"].tobytes() == np.array([dmin, dmax], dtype=np.float32).tobytes()
    want_proj = DC.ref_stage_chain(intr, extr)
    for k in want_proj:
        assert got["proj_matrices"][k].tobytes() == want_proj[k].tobytes(), k
    short = formats.load_tanks_sample(str(tmp_path), "Family", 0, [1], nviews=3)           # the loader runs it with two views
    assert len(short["imgs"]) == 2 and short["proj_matrices"]["stage1"].shape == (2, 2, 4, 4)


def test_load_eth3d_sample_is_resize_linear_and_per_view_factors(tmp_path):
    import PIL  # noqa: F401
    sizes = [(150, 200), (141, 211), (128, 256), (150, 200)]
    sc = DC.dataset_scan(sizes, seed=6, negative_min_view=1)
    pairs = [(0, [1, 2, 3]), (1, [0, 2, 3]), (2, [3, 1, 0]), (3, [2, 1, 0])]
    DC.write_dataset_folder(str(tmp_path), "door", sc, pairs, cams="cams_1")
    img_wh = (128, 64)
    got = formats.load_eth3d_sample(str(tmp_path), "door", 1, pairs[1][1], nviews=4, img_wh=img_wh)
    views = [1, 0, 2, 3]
    intr, extr = [], []
    for i, v in enumerate(views):
        img = formats.read_img(os.path.join(str(tmp_path), "door", "images", "{:0>8}.jpg".format(v)))
        assert img.shape[:2] == sizes[v]
        want = formats.resize_linear(img, 64, 128).transpose(2, 0, 1)
        assert got["imgs"][i].shape == (3, 64, 128)
        assert np.ascontiguousarray(got["imgs"][i]).tobytes() == np.ascontiguousarray(want).tobytes()
        K, E, dmin, dmax = DC.ref_read_cam_file(os.path.join(str(tmp_path), "door", "cams_1", "{:0>8}_cam.txt".format(v)), eth3d=True)
        intr.append(DC.ref_eth3d_intrinsics(K, img_wh, *sizes[v]))
        extr.append(E)
        if i == 0:
            assert dmin == 1                                                   # the file says -3.5
            assert got["depth_values"].tobytes() == np.array([dmin, dmax], dtype=np.float32).tobytes()
    want_proj = DC.ref_stage_chain(intr, extr)
    for k in want_proj:
        assert got["proj_matrices"][k].tobytes() == want_proj[k].tobytes(), k
    with pytest.raises(RuntimeError, match="never enlarges"):
        formats.load_eth3d_sample(str(tmp_path), "door", 1, pairs[1][1], nviews=4, img_wh=(256, 128))


def test_folder_readers_and_plans_follow_the_sample_builders(tmp_path):
    """read_scan_folder / plan_scan_folder with ``dataset``: the plan's stacks and depth_values are the sample builders'."""
    import PIL  # noqa: F401
    pairs = [(0, [1, 2, 3]), (1, [0, 2, 3]), (2, [3, 1, 0]), (3, [2, 1, 0])]
    tanks = DC.dataset_scan([(120, 128)] * 4, seed=7)
    DC.write_dataset_folder(str(tmp_path), "Horse", tanks, pairs)
    eth = DC.dataset_scan([(150, 200), (141, 211), (128, 256), (150, 200)], seed=8, negative_min_view=2)
    DC.write_dataset_folder(str(tmp_path), "door", eth, pairs, cams="cams_1")
    sc, plan = scan.plan_scan_folder(str(tmp_path), "Horse", nviews=3, dataset="tanks")
    assert plan.depth_values.shape == (4, 2) and [im.shape for im in sc["images"]] == [(120, 128, 3)] * 4
    for r in range(4):
        want = formats.load_tanks_sample(str(tmp_path), "Horse", r, pairs[r][1], nviews=3)
        assert plan.depth_values[r].tobytes() == want["depth_values"].tobytes()
        for k in plan.proj:
            assert plan.proj[k][plan.view_table[r]].tobytes() == want["proj_matrices"][k].tobytes(), (r, k)
    sc, plan = scan.plan_scan_folder(str(tmp_path), "door", nviews=4, dataset="eth3d", img_wh=(128, 64))
    assert sc["depth_ranges"][2][0] == 1
    for r in range(4):
        want = formats.load_eth3d_sample(str(tmp_path), "door", r, pairs[r][1], nviews=4, img_wh=(128, 64))
        assert plan.depth_values[r].tobytes() == want["depth_values"].tobytes()
        for k in plan.proj:
            assert plan.proj[k][plan.view_table[r]].tobytes() == want["proj_matrices"][k].tobytes(), (r, k)
    with pytest.raises(RuntimeError, match="smaller than img_wh"):
        scan.plan_scan_folder(str(tmp_path), "door", nviews=4, dataset="eth3d")                # the default 1920 x 1280
    with pytest.raises(RuntimeError, match="dataset = 'dtu'"):
        scan.read_scan_folder(str(tmp_path), "door", dataset="dtu")
    with pytest.raises(RuntimeError, match=r"cams.00000000_cam.txt does not exist"):
        scan.read_scan_folder(str(tmp_path), "door", dataset="tanks")                          # ETH3D keeps them in cams_1/


# ---- infer_scan: validation before any device work ---------------------------------------------------------------------
def test_infer_scan_dataset_modes_validate_on_the_host():
    m = _model()
    sc = SC.synthetic_scan(4, 120, 128, seed=1)
    pairs = SC.ring_pairs(4, 2)
    mm = [(400.0, 900.0)] * 4
    args = (sc["Ks"], sc["Es"], mm, pairs)
    kw = dict(nviews=3, depth_range_kind="min_max")
    # what passes the host checks stops at the missing device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(28, 28), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, list(sc["images"]), *args, img_wh=(128, 64), **kw)
    mixed = [sc["images"][0], sc["images"][1][:100, :], sc["images"][2][:, :100], sc["images"][3]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, mixed, *args, img_wh=(64, 64), **kw)                # views of different native sizes are fine here
    # a short source list: refused, naming the view (by its file number where there is one)
    short = [(0, [1, 2]), (1, [0, 2]), (2, [3]), (3, [2, 1])]
    with pytest.raises(RuntimeError, match=r"reference view 2 has 1 source views, fewer than nviews - 1 = 2.*padding"):
        scan.infer_scan(m, sc["images"], sc["Ks"], sc["Es"], mm, short, crop_rows=(28, 28), **kw)
    with pytest.raises(RuntimeError, match=r"reference view 12 has 1 source views"):
        scan.infer_scan(m, sc["images"], sc["Ks"], sc["Es"], mm, short, img_wh=(128, 64), view_ids=[10, 11, 12, 13], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # ... while the DTU path pads it, as before
        scan.infer_scan(m, sc["images"][:, :64], sc["Ks"], sc["Es"], sc["depth_ranges"], short, nviews=3)
    # a crop that leaves a size that is not a multiple of 64
    with pytest.raises(RuntimeError, match=r"crop_rows = \(20, 20\) leaves 80x128.*multiples of 64"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(20, 20), **kw)
    with pytest.raises(RuntimeError, match=r"leaves 0x128"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(60, 60), **kw)
    # img_wh larger than a view, or not admissible
    low = [sc["images"][0], sc["images"][1][:60, :], sc["images"][2], sc["images"][3]]
    with pytest.raises(RuntimeError, match=r"image 1 is 60x128, smaller than img_wh = \(128, 64\).*enlarges"):
        scan.infer_scan(m, low, *args, img_wh=(128, 64), **kw)
    with pytest.raises(RuntimeError, match=r"img_wh = \(100, 64\).*multiples of 64"):
        scan.infer_scan(m, sc["images"], *args, img_wh=(100, 64), **kw)
    # one image preparation at a time
    with pytest.raises(RuntimeError, match="give one of them"):
        scan.infer_scan(m, sc["images"], *args, img_wh=(128, 64), max_h=64, **kw)
    with pytest.raises(RuntimeError, match="give one of them"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(28, 28), max_w=128, **kw)
    with pytest.raises(RuntimeError, match="give one of them"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(28, 28), img_wh=(128, 64), **kw)
    # float32 images that would need resampling (or cropping): uint8 is the way in
    floats = np.ascontiguousarray((sc["images"].astype(np.float32) / 255.0).transpose(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match="float32 images of 120x128 would be cropped or resampled to 64x128.*uint8"):
        scan.infer_scan(m, floats, *args, img_wh=(128, 64), **kw)
    with pytest.raises(RuntimeError, match="float32 images of 120x128 would be cropped or resampled to 64x128.*uint8"):
        scan.infer_scan(m, floats, *args, crop_rows=(28, 28), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # ... already at the target size: nothing to do
        scan.infer_scan(m, floats[:, :, :64], *args, img_wh=(128, 64), **kw)
    # mixed sizes with crop_rows
    with pytest.raises(RuntimeError, match=r"image 1 is 100x128 but image 0 is 120x128: with crop_rows all views"):
        scan.infer_scan(m, mixed, *args, crop_rows=(28, 28), **kw)
    # the source bytes count towards max_store_bytes
    need, source = scan.store_bytes(4, 64, 128), 4 * 120 * 128 * 3
    with pytest.raises(RuntimeError, match=r"need %d \+ %d bytes" % (need, source)):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(28, 28), max_store_bytes=need + source - 1, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(28, 28), max_store_bytes=need + source, **kw)
    with pytest.raises(RuntimeError, match="depth_range_kind = 'max_min'"):
        scan.infer_scan(m, sc["images"], *args, crop_rows=(28, 28), nviews=3, depth_range_kind="max_min")
    with pytest.raises(RuntimeError, match=r"\(depth_min, depth_max\)"):
        scan.infer_scan(m, sc["images"], sc["Ks"], sc["Es"], np.zeros((4, 3), np.float32), pairs, crop_rows=(28, 28), **kw)


# ---- nothing changes without the keywords ------------------------------------------------------------------------------
def test_plan_scan_reads_two_columns_as_before_by_default():
    sc = SC.synthetic_scan(7, 64, 64, seed=2)
    old = scan.plan_scan(sc["Ks"], sc["Es"], sc["depth_ranges"], SC.PAIRS_7, 5, 192)
    named = scan.plan_scan(sc["Ks"], sc["Es"], sc["depth_ranges"], SC.PAIRS_7, nviews=5, ndepths=192, depth_range_kind="min_interval")
    assert old.depth_values.shape == (6, 192)
    for r, view in enumerate(old.ref_views):
        dmin, dint = sc["depth_ranges"][view]
        assert old.depth_values[r].tobytes() == formats.depth_value_range(dmin, dint, 192).tobytes()
    assert old.depth_values.tobytes() == named.depth_values.tobytes() and np.array_equal(old.view_table, named.view_table)
    assert list(old.view_table[2]) == [2, 0, 1, 0, 0]                          # the DTU loader's padding is untouched
    mm = scan.plan_scan(sc["Ks"], sc["Es"], sc["depth_ranges"], SC.PAIRS_7, 5, 192, depth_range_kind="min_max")
    assert mm.depth_values.shape == (6, 2)
    assert mm.depth_values.tobytes() == np.asarray(sc["depth_ranges"], np.float32)[old.ref_views].tobytes()
    for k in old.proj:
        assert old.proj[k].tobytes() == mm.proj[k].tobytes()
