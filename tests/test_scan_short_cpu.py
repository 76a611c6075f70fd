"""Host side of ``short_sources="fewer_views"`` (mvster_amd.scan): a reference view with fewer than ``nviews - 1`` sources
runs with the sources it has.  Planning tables, the count check, the two counted ABI entries, and the mirror of the refusal
test of tests/test_scan_datasets_cpu.py.  No GPU."""
import os

import numpy as np
import pytest

from mvster_amd import formats, ops, scan
from tests import scan_cases as SC
from tests import scan_short_cases as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from mvster_amd import MVS4net
    from tests.conftest import SHIPPED
    return MVS4net(**SHIPPED).eval()


def test_plan_scan_keeps_short_lists_and_pads_the_table_with_the_reference_view():
    sc = SC.synthetic_scan(6, 64, 64, seed=4)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"])
    plan = scan.plan_scan(*args, SS.PAIRS_CUT, nviews=SS.NVIEWS, short_sources="fewer_views")
    assert scan.ScanPlan._fields[-1] == "source_counts"
    assert plan.ref_views.tolist() == [0, 1, 2, 4, 5]                          # view 3 has no sources: dropped
    assert plan.source_counts.dtype == np.int32 and plan.source_counts.tolist() == [3, 2, 1, 3, 3]
    assert plan.view_table.dtype == np.int32 and plan.view_table.tolist() == [
        [0, 1, 2, 3],                                                          # five sources cut to nviews - 1 = 3
        [1, 0, 2, 1],                                                          # unused slot: the reference's own number
        [2, 1, 2, 2],
        [4, 3, 2, 0],
        [5, 4, 0, 1]]
    for k in ("stage1", "stage2", "stage3", "stage4"):
        assert np.isfinite(plan.proj[k][plan.view_table]).all()
    assert plan.fusion_pairs == [(r, s) for r, s in SS.PAIRS_CUT if s]         # full lists: what fusion reads
    # the used part of every row is the per-sample loader's view order, and the table passes the checks the kernels rely on
    for row, n, (r, srcs) in zip(plan.view_table, plan.source_counts, plan.fusion_pairs):
        assert row[:1 + n].tolist() == [r] + srcs[:SS.NVIEWS - 1]
    assert ops.check_view_table(plan.view_table, 6).tolist() == plan.view_table.tolist()
    assert ops.check_source_counts(plan.source_counts, SS.NVIEWS - 1, 5).tolist() == [3, 2, 1, 3, 3]
    # the default is untouched: padded by repeating the first source, every count nviews - 1
    old = scan.plan_scan(*args, SS.PAIRS_CUT, nviews=SS.NVIEWS)
    assert old.view_table.tolist() == [[0, 1, 2, 3], [1, 0, 2, 0], [2, 1, 1, 1], [4, 3, 2, 0], [5, 4, 0, 1]]
    assert old.source_counts.tolist() == [3] * 5
    assert old.depth_values.tobytes() == plan.depth_values.tobytes()
    none = scan.plan_scan(*args, SS.PAIRS_CUT, nviews=SS.NVIEWS, short_sources=None)
    assert none.view_table.tolist() == old.view_table.tolist()
    with pytest.raises(RuntimeError, match=r"short_sources = 'pad'"):
        scan.plan_scan(*args, SS.PAIRS_CUT, nviews=SS.NVIEWS, short_sources="pad")
    with pytest.raises(RuntimeError, match="short_sources"):
        scan.infer_scan(_model(), sc["images"], *args, SS.PAIRS_CUT, nviews=SS.NVIEWS, short_sources=True)


def test_short_samples_get_store_entries_of_their_own_batch_size():
    """The per-sample forward runs the FPN on a sample's own 1 + n images and picks kernels by batch, so the views of a short
    sample get store entries computed in batches of 1 + n: one page per distinct short count, behind the scan's V views."""
    sc = SC.synthetic_scan(6, 64, 64, seed=4)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"])
    plan = scan.plan_scan(*args, SS.PAIRS, nviews=SS.NVIEWS, short_sources="fewer_views")
    entries, pages, store_views = scan._short_entries(plan, 6, SS.NVIEWS)
    assert pages == [(2, [3, 4], 6), (3, [0, 1, 2], 8)] and store_views == 11        # (batch, views, first entry)
    assert entries.dtype == np.int32 and entries.tolist() == [
        [0, 1, 2, 3],                                                          # full samples read the scan's own entries
        [9, 8, 10, 9],                                                         # view 1 with sources 0, 2: the batch-of-3 page
        [2, 1, 3, 4],
        [6, 7, 6, 6],                                                          # view 3 with source 4: the batch-of-2 page
        [4, 3, 2, 0]]
    assert ops.check_view_table(entries, store_views).tolist() == entries.tolist()
    # a scan without short lists has no pages: the stores and the FPN runs are those of the default
    full = scan.plan_scan(*args, SC.ring_pairs(6, 3), nviews=SS.NVIEWS, short_sources="fewer_views")
    entries, pages, store_views = scan._short_entries(full, 6, SS.NVIEWS)
    assert pages == [] and store_views == 6 and entries.tolist() == full.view_table.tolist()
    need = scan.store_bytes(11, 64, 64)
    with pytest.raises(RuntimeError, match="level stores of 11 views of 64x64 need %d bytes" % need):
        scan.infer_scan(_model(), sc["images"], *args, SS.PAIRS, nviews=SS.NVIEWS, short_sources="fewer_views",
                        max_store_bytes=need - 1)


def test_plan_scan_folder_takes_the_keyword(tmp_path):
    pytest.importorskip("PIL")
    from tests import scan_dataset_cases as DC
    sc = DC.dataset_scan([(120, 128)] * 6, seed=5)
    DC.write_dataset_folder(str(tmp_path), "Family", sc, SS.PAIRS)
    with pytest.raises(RuntimeError, match=r"reference view 1 has 2 source views.*short_sources='fewer_views'"):
        scan.plan_scan_folder(str(tmp_path), "Family", nviews=SS.NVIEWS, dataset="tanks")
    got, plan = scan.plan_scan_folder(str(tmp_path), "Family", nviews=SS.NVIEWS, dataset="tanks", short_sources="fewer_views")
    assert got["view_ids"] == [0, 1, 2, 3, 4] and plan.source_counts.tolist() == SS.COUNTS
    # every row, cut to its count, is the sample the Tanks loader builds
    for row, n, (r, srcs) in zip(plan.view_table, plan.source_counts, SS.WITH_SOURCES):
        want = formats.load_tanks_sample(str(tmp_path), "Family", r, srcs, nviews=SS.NVIEWS)
        assert len(want["imgs"]) == 1 + n
        for k in ("stage1", "stage2", "stage3", "stage4"):
            assert plan.proj[k][row[:1 + n]].tobytes() == want["proj_matrices"][k].tobytes(), (r, k)
    with pytest.raises(RuntimeError, match="short_sources"):
        scan.plan_scan_folder(str(tmp_path), "Family", nviews=SS.NVIEWS, dataset="tanks", short_sources="fewer")


def test_source_counts_are_checked_on_the_host():
    got = ops.check_source_counts([1, 4, 2], 4, 3)
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == [1, 4, 2]
    assert ops.check_source_counts(np.array([3], dtype=np.int64), 3, 1).tolist() == [3]
    with pytest.raises(RuntimeError, match=r"source count 0 \(row 1\)"):
        ops.check_source_counts([1, 0, 2], 4, 3)
    with pytest.raises(RuntimeError, match=r"source count 5 \(row 2\).*1\.\.NV = 4"):
        ops.check_source_counts([1, 4, 5], 4, 3)
    with pytest.raises(RuntimeError, match=r"source count -1 \(row 0\)"):
        ops.check_source_counts([-1], 4, 1)
    with pytest.raises(RuntimeError, match=r"must be \[B\] = \[3\]"):
        ops.check_source_counts([1, 2], 4, 3)                                   # wrong length
    with pytest.raises(RuntimeError, match=r"must be \[B\]"):
        ops.check_source_counts([[1, 2, 3]], 4, 3)                              # wrong dimension
    with pytest.raises(RuntimeError, match=r"must be \[B\]"):
        ops.check_source_counts(2, 4, 1)


def test_counted_entries_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mvster_hip.h")).read()
    for name in ("mvster_warp_agg_fwd_counted", "mvster_warp_agg_fwd_indexed_counted"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and ("int %s(" % name) in header
    # the uncounted argument lists plus the counts before the stream
    assert _lib.SIGNATURES["mvster_warp_agg_fwd_counted"] == \
        _lib.SIGNATURES["mvster_warp_agg_fwd"][:-1] + [_lib._f] + _lib.SIGNATURES["mvster_warp_agg_fwd"][-1:]
    assert _lib.SIGNATURES["mvster_warp_agg_fwd_indexed_counted"] == \
        _lib.SIGNATURES["mvster_warp_agg_fwd_indexed"][:-1] + [_lib._f] + _lib.SIGNATURES["mvster_warp_agg_fwd_indexed"][-1:]
    # argument validation happens before any HIP call (stand-in addresses that nothing dereferences)
    p = [1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 36]
    plain = (1, 2, 8, 4, 4, 4, 4, 4, 4, 128, 128, 128, 1, 1, 2.0, 0)          # B NV C G D h w Hs Ws strides gc fuse temp variant
    assert lib.mvster_warp_agg_fwd_counted(None, None, None, None, None, None, *plain, 1 << 37, None) == _lib.ERR_NULL
    assert lib.mvster_warp_agg_fwd_counted(*p, None, *plain, None, None) == _lib.ERR_NULL            # no counts
    assert lib.mvster_warp_agg_fwd_counted(*p, None, 1, 0, *plain[2:], 1 << 37, None) == _lib.ERR_SHAPE  # NV = 0
    assert lib.mvster_warp_agg_fwd_counted(*p, None, 1, 2, 8, 4, 65, *plain[5:], 1 << 37, None) == _lib.ERR_SHAPE  # D > 64
    idx = (3, 1, 2, 8, 4, 4, 4, 4, 1, 1, 2.0, 0)                               # V B NV C G D h w gc fuse temp variant
    assert lib.mvster_warp_agg_fwd_indexed_counted(None, None, None, None, None, None, *idx, 1 << 37, None) == _lib.ERR_NULL
    assert lib.mvster_warp_agg_fwd_indexed_counted(*p, None, *idx, None, None) == _lib.ERR_NULL      # no counts
    assert lib.mvster_warp_agg_fwd_indexed_counted(p[0], None, *p[2:], None, *idx, 1 << 37, None) == _lib.ERR_NULL   # no table
    assert lib.mvster_warp_agg_fwd_indexed_counted(*p, None, 0, *idx[1:], 1 << 37, None) == _lib.ERR_SHAPE   # V = 0
    # the forms kept for the record have no counted launch
    assert lib.mvster_warp_agg_fwd_counted(*p, None, *plain[:-1], 4, 1 << 37, None) == _lib.ERR_UNSUPPORTED
    assert lib.mvster_warp_agg_fwd_indexed_counted(*p, None, *idx[:-1], 5, 1 << 37, None) == _lib.ERR_UNSUPPORTED


def test_short_lists_pass_the_host_checks_with_the_keyword():
    """The mirror of the refusal in tests/test_scan_datasets_cpu.py: with ``short_sources="fewer_views"`` the same calls get
    as far as the missing device."""
    m = _model()                                                             # on the CPU: device work would raise differently
    sc = SC.synthetic_scan(4, 120, 128, seed=9)
    mm = [(400.0, 900.0)] * 4
    short = [(0, [1, 2]), (1, [0, 2]), (2, [3]), (3, [2, 1])]
    kw = dict(nviews=3, depth_range_kind="min_max")
    with pytest.raises(RuntimeError, match=r"reference view 2 has 1 source views, fewer than nviews - 1 = 2"):
        scan.infer_scan(m, sc["images"], sc["Ks"], sc["Es"], mm, short, crop_rows=(28, 28), **kw)
    for how in (dict(crop_rows=(28, 28)), dict(img_wh=(128, 64), view_ids=[10, 11, 12, 13])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            scan.infer_scan(m, sc["images"], sc["Ks"], sc["Es"], mm, short, short_sources="fewer_views", **how, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # the DTU loader's inputs take it too
        scan.infer_scan(m, sc["images"][:, :64], sc["Ks"], sc["Es"], sc["depth_ranges"], short, nviews=3,
                        short_sources="fewer_views")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan.reconstruct_scan(m, sc["images"], sc["Ks"], sc["Es"], mm, short, crop_rows=(28, 28), short_sources="fewer_views",
                              **kw)
