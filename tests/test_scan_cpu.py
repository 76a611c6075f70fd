"""Host side of the scan-level inference path (mvster_amd.scan): planning tables against the per-sample loader, the 8-bit
image contract, input validation before any device work, the two new ABI entries.  No GPU."""
import os

import numpy as np
import pytest
import torch

from mvster_amd import formats, scan
from tests import scan_cases as SC


def test_planning_tables_equal_the_per_sample_loader(tmp_path):
    """For every reference view: projection stacks, depth_values and view order of the scan planning, gathered by its
    view table, equal formats.load_eval_sample bit for bit (padding, cutting and dropping included)."""
    pytest.importorskip("PIL")
    nviews = 5
    sc = SC.synthetic_scan(7, 128, 192, seed=3)
    SC.write_scan_folder(str(tmp_path), "scan1", sc, SC.PAIRS_7)
    got, plan = scan.plan_scan_folder(str(tmp_path), "scan1", nviews=nviews)
    metas = formats.eval_view_list(str(tmp_path), ["scan1"], nviews)
    assert [m[1] for m in metas] == [got["view_ids"][r] for r in plan.ref_views] == [0, 1, 2, 3, 4, 6]
    # view 5 has no sources and nobody lists it: it is not part of the scan, and file number 6 sits in slot 5
    assert got["view_ids"] == [0, 1, 2, 3, 4, 6] and plan.ref_views.tolist() == [0, 1, 2, 3, 4, 5]
    assert plan.view_table.dtype == np.int32 and plan.view_table.shape == (6, nviews)
    assert plan.view_table[2].tolist() == [2, 0, 1, 0, 0]                    # padded by repeating the first source
    assert plan.view_table[0].tolist() == [0, 1, 2, 3, 4]                    # cut to nviews - 1
    for row, (_, ref_view, src_views) in enumerate(metas):
        want = formats.load_eval_sample(str(tmp_path), "scan1", ref_view, src_views, nviews)
        views = plan.view_table[row]
        assert [got["view_ids"][v] for v in views] == [ref_view] + list(src_views[:nviews - 1])
        for k in ("stage1", "stage2", "stage3", "stage4"):
            stack = plan.proj[k][views]
            assert stack.dtype == np.float32 and stack.tobytes() == want["proj_matrices"][k].tobytes(), (row, k)
        assert plan.depth_values[row].tobytes() == want["depth_values"].tobytes()
        for v, img in zip(views, want["imgs"]):                              # same decoded files, read_img's arithmetic
            mine = (np.float32(1) * got["images"][v].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
            assert mine.tobytes() == np.ascontiguousarray(img).tobytes()
    slot = {v: i for i, v in enumerate(got["view_ids"])}
    assert plan.fusion_pairs == [(slot[r], [slot[v] for v in s]) for r, s in SC.PAIRS_7 if s]


def test_u8_contract_equals_read_img(tmp_path):
    """float32(u8) / float32(255) -- what mvster_pack_images_u8 computes -- is read_img's value for all 256 levels."""
    Image = pytest.importorskip("PIL.Image")
    levels = np.arange(256, dtype=np.uint8)
    img = np.stack([levels.reshape(16, 16)] * 3, -1)
    path = os.path.join(str(tmp_path), "levels.png")
    Image.fromarray(img).save(path)                                          # lossless: every level reaches read_img
    want = formats.read_img(path)
    assert want.dtype == np.float32 and np.array_equal((want[..., 0] * 255).round().astype(np.uint8).reshape(-1), levels)
    mine = levels.astype(np.float32) / np.float32(255)
    assert mine.dtype == np.float32 and mine.tobytes() == np.ascontiguousarray(want[..., 0]).tobytes()
    # a true division: multiplying by the rounded reciprocal differs for some levels, so the kernel must not do that
    assert np.any(levels.astype(np.float32) * np.float32(1.0 / 255.0) != mine)


def _model():
    from mvster_amd import MVS4net
    from tests.conftest import SHIPPED
    return MVS4net(**SHIPPED).eval()


def test_validation_names_the_offender_before_any_device_work():
    m = _model()                                                             # on the CPU: device work would raise differently
    sc = SC.synthetic_scan(4, 64, 128, seed=1)
    pairs = SC.ring_pairs(4, 2)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"])
    mixed = [sc["images"][0], sc["images"][1][:, :64], sc["images"][2], sc["images"][3]]
    with pytest.raises(RuntimeError, match=r"image 1 is \(64, 64, 3\)"):
        scan.infer_scan(m, mixed, *args, pairs)
    with pytest.raises(RuntimeError, match="96x128.*multiples of 64"):
        scan.infer_scan(m, np.zeros((4, 96, 128, 3), np.uint8), *args, pairs)
    with pytest.raises(RuntimeError, match="name view 7"):
        scan.infer_scan(m, sc["images"], *args, pairs + [(1, [0, 7])])
    need = scan.store_bytes(4, 64, 128)
    assert need == 4 * 64 * 128 * 15 * 4
    with pytest.raises(RuntimeError, match="need %d bytes" % need):
        scan.infer_scan(m, sc["images"], *args, pairs, max_store_bytes=need - 1)
    with pytest.raises(RuntimeError, match="3 images for 4"):
        scan.infer_scan(m, sc["images"][:3], *args, pairs)
    with pytest.raises(RuntimeError, match="uint8 .* or float32"):
        scan.infer_scan(m, sc["images"].astype(np.float64), *args, pairs)
    # everything valid: only now the device is looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.infer_scan(m, sc["images"], *args, pairs, max_store_bytes=need)


def test_folder_validation_names_the_missing_view(tmp_path):
    pytest.importorskip("PIL")
    sc = SC.synthetic_scan(3, 64, 64, seed=2)
    SC.write_scan_folder(str(tmp_path), "s", sc, [(0, [1, 2]), (1, [0, 9])])
    with pytest.raises(RuntimeError, match="names view 9"):
        scan.infer_scan_folder(_model(), str(tmp_path), "s")


def test_view_table_is_checked_on_the_host():
    from mvster_amd import ops
    assert ops.check_view_table([[0, 1, 1], [2, 0, 0]], 3).dtype == np.int32
    with pytest.raises(RuntimeError, match=r"view index 3 \(row 1, column 2\)"):
        ops.check_view_table([[0, 1, 1], [2, 0, 3]], 3)
    with pytest.raises(RuntimeError, match="view index -1"):
        ops.check_view_table([[0, -1]], 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_images_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


def test_new_entries_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvster_hip.h")).read()
    for name in ("mvster_pack_images_u8", "mvster_warp_agg_fwd_indexed", "mvster_gather_views"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and ("int %s(" % name) in header
    # argument validation happens before any HIP call
    assert lib.mvster_pack_images_u8(None, None, 1, 4, 4, None) == _lib.ERR_NULL
    assert lib.mvster_pack_images_u8(1 << 32, 1 << 33, 0, 4, 4, None) == _lib.ERR_SHAPE
    assert lib.mvster_warp_agg_fwd_indexed(None, None, None, None, None, None, 1, 1, 1, 8, 4, 4, 4, 4, 1, 1, 2.0, 0, None) \
        == _lib.ERR_NULL
    assert lib.mvster_warp_agg_fwd_indexed(1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 36, None, 0, 1, 1, 8, 4, 4, 4, 4, 1, 1,
                                           2.0, 0, None) == _lib.ERR_SHAPE
    assert lib.mvster_gather_views(1 << 32, 1 << 33, 1 << 34, 2, 1, 2, 6, None) == _lib.ERR_SHAPE


def test_package_exports():
    import mvster_amd
    for n in ("infer_scan", "infer_scan_folder", "reconstruct_scan", "write_scan_outputs"):
        assert callable(getattr(mvster_amd, n)) and n in mvster_amd.__all__
