"""The loader's input scaling without a GPU: target sizes and intrinsics, the per-axis tap tables, the host build of
csrc/resize_math.h against an independent NumPy restatement and ``formats.resize_linear`` (bit for bit, all three),
``load_eval_sample(resample=True)``, the validation in ``infer_scan`` before any device work, ``scan.plan_inputs`` in the
``max_h`` / ``max_w`` mode, and that the op's own C entry is gone."""
import os

import numpy as np
import pytest
import torch

from mvster_amd import formats, ops, scan
from tests import resize_cases as RC
from tests import scan_cases as SC


# ---- sizes and intrinsics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given,want", RC.LOADER_SIZES)
def test_target_size_and_intrinsics_follow_the_loader(given, want):
    h, w, max_h, max_w = given
    Hd, Wd, scale_h, scale_w = formats.scale_input_size(h, w, max_h, max_w)
    assert (Hd, Wd) == want and isinstance(Hd, int) and isinstance(Wd, int)
    assert Hd % 64 == 0 and Wd % 64 == 0 and Hd <= min(h, max_h) and Wd <= min(w, max_w)
    assert scale_h == 1.0 * float(Hd) / h and scale_w == 1.0 * float(Wd) / w
    if want == (h, w):
        assert scale_h == 1.0 and scale_w == 1.0                             # exactly: the intrinsics keep their bits
    K = np.array([[2892.33, 0.0, 823.205], [0.0, 2883.175, 619.071], [0.0, 0.0, 1.0]], dtype=np.float32)
    K[:2] /= 4.0                                                             # (read_cam_file's quarter-resolution convention)
    mine = formats.scale_intrinsics(K, scale_h, scale_w)
    ref = K.copy()                                                           # general_eval4.py:102-105, on a float32 matrix
    ref[0, :] *= 1.0 * float(Wd) / w
    ref[1, :] *= 1.0 * float(Hd) / h
    assert mine.dtype == np.float32 and mine.tobytes() == ref.tobytes() and mine is not K
    stack = formats.scale_intrinsics(np.stack([K, K * np.float32(1.5)]), scale_h, scale_w)
    assert stack[0].tobytes() == ref.tobytes() and stack.shape == (2, 3, 3)


def test_dtu_default_runs_at_832_not_864():
    """1200 x 1600 within the reference's default max_h = 864, max_w = 1152: the factor is 0.72 and 0.72 * 1200 = 864, which
    is not a multiple of 64 (13.5 * 64), so the floor division lands on 832 -- the size the reference runs DTU at."""
    assert 864 % 64 == 32 and 1.0 * 1152 / 1600 * 1200 // 64 * 64 == 832.0
    assert formats.scale_input_size(1200, 1600, 864, 1152)[:2] == (832, 1152)


# ---- tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_tables_are_in_range_and_equal_the_scalar_restatement(name):
    Hs, Ws, Hd, Wd, _ = RC.CASES[name]
    sx, fx, sy, fy = formats.resize_tables(Hs, Ws, Hd, Wd)
    for s, f, ns, nd in ((sx, fx, Ws, Wd), (sy, fy, Hs, Hd)):
        assert s.dtype == np.int32 and f.dtype == np.float32 and s.shape == f.shape == (nd,)
        assert s.min() >= 0 and s.max() <= ns - 1
        assert f.min() >= 0.0 and f.max() < 1.0
        assert np.all(f[s == ns - 1] == 0.0)
        rs, rf, high = RC.ref_axis_table(ns, nd)
        assert s.tolist() == rs and f.tobytes() == np.array(rf, dtype=np.float32).tobytes()
        # the loader never enlarges: the upper clamp is reached only at scale 1, in the last sample
        assert [i for i, h in enumerate(high) if h] == ([nd - 1] if ns == nd else [])


def test_identity_tables_and_the_clamp_at_scale_one():
    sx, fx, sy, fy = formats.resize_tables(64, 200, 64, 200)
    assert np.array_equal(sx, np.arange(200)) and np.array_equal(sy, np.arange(64))
    assert not fx.any() and not fy.any()
    assert sx[-1] == 199 and fx[-1] == 0.0 and sy[-1] == 63 and fy[-1] == 0.0   # clamped: the second tap is not read
    # ... and the value there is the source pixel itself
    img = np.random.RandomState(0).rand(64, 200, 3).astype(np.float32)
    assert formats.resize_linear(img, 64, 200).tobytes() == img.tobytes()


def test_table_1600_to_1152_written_out():
    sx, fx, _, _ = formats.resize_tables(1200, 1600, 832, 1152)
    assert sx[:3].tolist() == [0, 1, 2] and sx[-3:].tolist() == [1596, 1597, 1598]
    assert fx[:3].tolist() == [np.float32(0.19444445), np.float32(0.58333337), np.float32(0.97222233)]
    # 2:1 -- every fraction is one half, every first tap even (the kernel takes the area path there)
    sx, fx, sy, fy = formats.resize_tables(2048, 2560, 1024, 1280)
    assert np.array_equal(sx, 2 * np.arange(1280)) and np.all(fx == 0.5) and np.array_equal(sy, 2 * np.arange(1024))


# ---- arithmetic: host build == restatement == formats.resize_linear ------------------------------------------------------
@pytest.fixture(scope="module")
def hostmath():
    return RC.load_resize_hostmath()


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_host_build_equals_restatement_equals_resize_linear(hostmath, name):
    Hs, Ws, Hd, Wd, kind = RC.CASES[name]
    u8 = RC.case_images(name, 1)
    assert u8.shape == (1, Hs, Ws, 3)
    want, want_u8 = RC.ref_outputs(u8, Hd, Wd)
    got, got_u8 = RC.run_host(hostmath, u8, Hd, Wd, formats.resize_tables(Hs, Ws, Hd, Wd))
    assert got.tobytes() == want.tobytes(), "host build of resize_math.h != restatement: %d elements" % (got != want).sum()
    assert got_u8.tobytes() == want_u8.tobytes()
    floats = u8[0].astype(np.float32) / 255.0                                # read_img
    mine = formats.resize_linear(floats, Hd, Wd)
    assert mine.dtype == np.float32 and mine.shape == (Hd, Wd, 3)
    assert np.ascontiguousarray(mine).tobytes() == np.ascontiguousarray(want[0, 0, :, :, :3]).tobytes()
    assert not got[..., 3].any()
    if kind == "constant":
        assert np.all(got[0, 0, :, :, :3] == np.float32(1.0)) and np.all(got_u8 == 255)
    if (Hs, Ws) == (Hd, Wd):
        assert np.array_equal(got_u8, u8) and got[0, 0, :, :, :3].tobytes() == floats.tobytes()


def test_area_path_is_the_two_by_two_mean(hostmath):
    u8 = RC.case_images("checkerboard_area", 1)
    got, _ = RC.run_host(hostmath, u8, 64, 128, formats.resize_tables(128, 256, 64, 128))
    S = u8[0].astype(np.float32) / np.float32(255)
    mean = ((S[0::2, 0::2] + S[0::2, 1::2]) + (S[1::2, 0::2] + S[1::2, 1::2])) * np.float32(0.25)
    assert got[0, 0, :, :, :3].tobytes() == np.ascontiguousarray(mean).tobytes()


def test_resize_linear_refuses_what_the_loader_never_does():
    img = np.zeros((64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match="never enlarges"):
        formats.resize_linear(img, 128, 64)
    with pytest.raises(RuntimeError, match="float32"):
        formats.resize_linear(img.astype(np.float64), 64, 64)


# ---- the loader ------------------------------------------------------------------------------------------------------------
def test_load_eval_sample_resamples_on_request(tmp_path):
    import PIL  # noqa: F401  (the folder helpers need it: missing is a failure, not a skip)
    sc = SC.synthetic_scan(4, 96, 160, seed=5)
    pairs = SC.ring_pairs(4, 3)
    SC.write_scan_folder(str(tmp_path), "s", sc, pairs)
    assert formats.scale_input_size(96, 160, 64, 128)[:2] == (64, 64)
    for max_h, max_w, size in ((64, 128, (64, 64)), (96, 128, (64, 128))):
        got = formats.load_eval_sample(str(tmp_path), "s", 1, pairs[1][1], 4, max_h=max_h, max_w=max_w, resample=True)
        Hd, Wd, scale_h, scale_w = formats.scale_input_size(96, 160, max_h, max_w)
        assert (Hd, Wd) == size
        Ks, Es = [], []
        for i, v in enumerate([1] + pairs[1][1][:3]):
            img = formats.read_img(os.path.join(str(tmp_path), "s", "images", "{:0>8}.jpg".format(v)))
            assert img.shape == (96, 160, 3)
            want = formats.resize_linear(img, Hd, Wd).transpose(2, 0, 1)
            assert got["imgs"][i].shape == (3, Hd, Wd) and got["imgs"][i].dtype == np.float32
            assert np.ascontiguousarray(got["imgs"][i]).tobytes() == np.ascontiguousarray(want).tobytes()
            K, E, _, _ = formats.read_cam_file(os.path.join(str(tmp_path), "s", "cams", "{:0>8}_cam.txt".format(v)), 1.06, 192)
            Ks.append(formats.scale_intrinsics(K, scale_h, scale_w))
            Es.append(E)
        want_proj = formats.stage_proj_matrices(Ks, Es)
        for k in ("stage1", "stage2", "stage3", "stage4"):
            assert got["proj_matrices"][k].tobytes() == want_proj[k].tobytes()
    # the default still refuses, with the message it always had
    with pytest.raises(NotImplementedError, match="resize the images first"):
        formats.load_eval_sample(str(tmp_path), "s", 1, pairs[1][1], 4, max_h=64, max_w=128)
    with pytest.raises(NotImplementedError, match="resize the images first"):
        formats.load_eval_sample(str(tmp_path), "s", 1, pairs[1][1], 4)


# ---- infer_scan: validation before any device work ---------------------------------------------------------------------
def _model():
    from mvster_amd import MVS4net
    from tests.conftest import SHIPPED
    return MVS4net(**SHIPPED).eval()


def test_infer_scan_with_scaling_validates_on_the_host():
    m = _model()                                                             # on the CPU: device work would raise differently
    sc = SC.synthetic_scan(4, 96, 160, seed=1)
    pairs = SC.ring_pairs(4, 2)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"], pairs)
    # without the new arguments: refused as before
    with pytest.raises(RuntimeError, match="96x160.*multiples of 64"):
        scan.infer_scan(m, sc["images"], *args)
    # with them the size passes, and only the device is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, sc["images"], *args, max_h=64, max_w=128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, list(sc["images"]), *args, max_h=96)              # one side alone; a sequence of views
    # the source stack counts towards max_store_bytes (64x64 after scaling)
    need, source = scan.store_bytes(4, 64, 64), 4 * 96 * 160 * 3
    with pytest.raises(RuntimeError, match=r"need %d \+ %d bytes" % (need, source)):
        scan.infer_scan(m, sc["images"], *args, max_h=64, max_w=128, max_store_bytes=need + source - 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, sc["images"], *args, max_h=64, max_w=128, max_store_bytes=need + source)
    # views of different native sizes
    mixed = [sc["images"][0], sc["images"][1][:, :128], sc["images"][2], sc["images"][3]]
    with pytest.raises(RuntimeError, match=r"image 1 is \(96, 128, 3\).*different native sizes"):
        scan.infer_scan(m, mixed, *args, max_h=64, max_w=128)
    # float32 images that would need resampling: uint8 is the way in
    floats = np.ascontiguousarray((sc["images"].astype(np.float32) / 255.0).transpose(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match="float32 images of 96x160 would be resampled to 64x64.*uint8"):
        scan.infer_scan(m, floats, *args, max_h=64, max_w=128)
    # ... while float32 images that already have the loader's size pass
    ok = np.zeros((4, 3, 64, 128), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, ok, *args, max_h=64, max_w=128)
    with pytest.raises(RuntimeError, match="nothing is left"):
        scan.infer_scan(m, np.zeros((4, 60, 200, 3), np.uint8), *args, max_h=64, max_w=128)


def test_plan_scan_folder_plans_from_the_scaled_intrinsics(tmp_path):
    import PIL  # noqa: F401  (the folder helpers need it: missing is a failure, not a skip)
    sc = SC.synthetic_scan(4, 96, 160, seed=2)
    pairs = SC.ring_pairs(4, 2)
    SC.write_scan_folder(str(tmp_path), "s", sc, pairs)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        scan.plan_scan_folder(str(tmp_path), "s", nviews=3)
    got, plan = scan.plan_scan_folder(str(tmp_path), "s", nviews=3, max_h=96, max_w=128)
    Hd, Wd, scale_h, scale_w = formats.scale_input_size(96, 160, 96, 128)
    assert (Hd, Wd) == (64, 128)
    want = formats.stage_proj_matrices(formats.scale_intrinsics(got["Ks"], scale_h, scale_w), got["Es"])
    for k in want:
        assert plan.proj[k].tobytes() == want[k].tobytes()
    meta = formats.load_eval_sample(str(tmp_path), "s", 0, pairs[0][1], 3, max_h=96, max_w=128, resample=True)
    assert plan.proj["stage4"][plan.view_table[0]].tobytes() == meta["proj_matrices"]["stage4"].tobytes()


# ---- the planning function in the max_h / max_w mode ---------------------------------------------------------------------
@pytest.mark.parametrize("given,want", [((192, 320, 128, 256), (128, 192))] + RC.LOADER_SIZES)
def test_plan_inputs_with_scaling_gives_the_loaders_size_intrinsics_and_uniform_descriptors(given, want):
    Hs, Ws, max_h, max_w = given
    V = 3
    images = np.zeros((V, Hs, Ws, 3), np.uint8)
    Ks = SC.synthetic_scan(V, 64, 64, seed=3)["Ks"]
    inp = scan.plan_inputs(images, Ks, max_h=max_h, max_w=max_w)
    Hd, Wd, scale_h, scale_w = formats.scale_input_size(Hs, Ws, max_h, max_w)
    assert (inp.H, inp.W) == (Hd, Wd) == want and inp.crop == (0, 0, 0, 0)
    assert inp.Ks.tobytes() == formats.scale_intrinsics(Ks, scale_h, scale_w).tobytes() and inp.Ks is not Ks
    assert (inp.kind, inp.V, inp.sizes, inp.prepare) == ("u8", V, [(Hs, Ws)] * V, True) and inp.images is images
    assert inp.source_bytes == V * Hs * Ws * 3
    # the same record from a sequence of views, and from one side alone where that side decides
    again = scan.plan_inputs(list(images), Ks, max_h=max_h, max_w=max_w)
    assert (again.H, again.W, again.sizes, again.source_bytes) == (Hd, Wd, inp.sizes, inp.source_bytes)
    assert again.Ks.tobytes() == inp.Ks.tobytes()
    # what the launch gets for it: the views where a packed stack has them, one table for all, the area flag only at 2:1
    desc, tables, total = ops.load_pack_descriptors(inp.sizes, inp.H, inp.W, inp.crop)
    offs = (desc[:, 0].astype(np.int64) & 0xffffffff) | (desc[:, 1].astype(np.int64) << 32)
    assert list(offs) == [v * Hs * Ws * 3 for v in range(V)] and total == V * Hs * Ws * 3
    area = int(Hs == 2 * Hd and Ws == 2 * Wd)
    assert area == int(given == (2048, 2560, 1024, 1280))
    assert all(tuple(d[2:10]) == (Hs, Ws, 0, 0, Hs, Ws, 0, area) for d in desc)
    sx, fx, sy, fy = formats.resize_tables(Hs, Ws, Hd, Wd)
    one = np.concatenate([sx.view(np.int32), fx.view(np.int32), sy.view(np.int32), fy.view(np.int32)])
    assert np.array_equal(tables, one if (Hs, Ws) != (Hd, Wd) else one[:0])  # (the identity size reads no table)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_resize_entry_is_declared_bound_and_exported():
    """The op kept its name; its C entry went when the launch became mvster_load_pack_images_u8's (whose error returns
    tests/test_scan_datasets_cpu.py pins)."""
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(RC.ROOT, "include", "mvster_hip.h")).read()
    name = "mvster_resize_pack_images_u8"
    assert name not in _lib.SIGNATURES and not hasattr(lib, name) and name not in header
    assert callable(ops.resize_pack_images_u8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resize_pack_images_u8(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), 64, 64)
