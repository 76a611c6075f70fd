"""Dynamic consistency fusion without a GPU: the restatement's kept fractions, the host build of the geo_math.h functions
the dynamic kernel inlines against the restatement, scans whose levels are known in advance, and the argument checks of the
C ABI and of ``fuse_scene`` that come before any device is touched."""
import os
import re

import numpy as np
import pytest

from tests import dynamic_fusion_cases as D
from tests import fusion_scene_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [pytest.param(name, case, kept, id=name) for name, case, kept in D.DYN_CASES]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def dhm():
    return D.load_geo_dyn_hostmath()


def test_entry_point_is_declared_exported_and_bound(lib):
    from mvster_amd import _lib
    text = open(os.path.join(ROOT, "include", "mvster_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(mvster_\w+)\s*\(", text))
    n = "mvster_geo_scene_filter_dynamic"
    assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES


@pytest.mark.parametrize("name,case,kept", CASES)
def test_committed_kept_fractions_hold(name, case, kept):
    views, vertices = D.restated_case(name, case)
    got = float(np.stack([w["final_mask"] for w in views]).mean())
    assert abs(got - kept) <= 1e-4 and got > 0, (got, kept)
    assert len(vertices) == sum(int(w["final_mask"].sum()) for w in views)


@pytest.mark.parametrize("name,case,kept", CASES)
def test_host_build_vs_restatement(dhm, name, case, kept):
    """geo::dynamic_votes serially over the scan against the NumPy restatement, within the fixed filter's bounds."""
    views, vertices = D.restated_case(name, case)
    got = D.run_host_dynamic(dhm, D.dyn_scene(case))
    fig = D.compare_with_restatement(got, views, vertices, floor=kept / 2)
    print("dynamic host build vs restatement:", name, fig)
    if fig["final_mask_mismatch_pixels"] == 0:
        assert len(got["points"]) == len(vertices) and np.array_equal(got["colors"][:, 0], vertices["red"])


def test_the_empty_case_keeps_nothing(dhm):
    sc = C.hard_scene(*D.EMPTY_CASE[:4])
    views, vertices = D.restated_scene(sc)
    got = D.run_host_dynamic(dhm, sc)
    assert len(vertices) == 0 and len(got["points"]) == 0 and not got["final_mask"].any() and (got["counts"] == 0).all()
    assert np.array_equal(got["geo_level"], np.stack([w["geo_level"] for w in views]))
    assert got["photo_mask"].any()


@pytest.mark.parametrize("name", ["small", "96x128x7-both", "96x128x7-degenerate"])
def test_every_level_from_thres_view_to_five_occurs(dhm, name):
    case = dict((n, c) for n, c, _ in D.DYN_CASES)[name]
    views, _ = D.restated_case(name, case)
    got = D.run_host_dynamic(dhm, D.dyn_scene(case))
    for level in (np.stack([w["geo_level"] for w in views]), got["geo_level"]):
        assert set(range(D.THRES_VIEW, 6)) <= set(np.unique(level).tolist())
    for w in views:                                     # count_n grows with n: a source that passes level n passes n + 1
        ns = sorted(w["level_counts"])
        assert all((w["level_counts"][a] <= w["level_counts"][b]).all() for a, b in zip(ns, ns[1:]))


@pytest.mark.parametrize("H,W", [(61, 83), (9, 13)])
@pytest.mark.parametrize("thres_view", [1, 2, 3])
def test_pattern_scene_passes_at_thres_view_or_not_at_all(dhm, H, W, thres_view):
    """One camera and one noise-free depth map for all views: every source passes every level, so geo_level is
    thres_view where the row has that many sources and 0 where it has fewer (rows of 3 and of 2 sources)."""
    V = 4
    pattern = C.pattern_mask("random", V, H, W)
    sc = C.pattern_scene(H, W, V, pattern)
    sc["pairs"][1] = (1, [0, 3])                                             # L = 2 in this row, 3 in the others
    L = np.array([len(s) for _, s in sc["pairs"]])
    want_level = np.where(L >= thres_view, thres_view, 0).astype(np.uint8)
    views, _ = D.restated_scene(sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=thres_view)
    got = D.run_host_dynamic(dhm, sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=thres_view)
    for r in range(V):
        assert (views[r]["geo_level"] == want_level[r]).all() and (got["geo_level"][r] == want_level[r]).all(), r
        assert (got["geo_mask_sum"][r] == L[r]).all() and (views[r]["geo_mask_sum"] == L[r]).all()
    final = pattern & (want_level != 0)[:, None, None]
    assert np.array_equal(got["final_mask"], final) and np.array_equal(np.stack([w["final_mask"] for w in views]), final)
    assert np.array_equal(got["counts"], final.reshape(V, -1).sum(1))
    assert np.array_equal(got["colors"], np.concatenate([sc["images"][r][final[r]] for r in range(V)]))
    if thres_view == 3:
        assert not final[1].any() and final[0].any() and final[2].any() and final[3].any()


@pytest.mark.parametrize("nsrc,thres_view", [(32, 1), (32, 5), (7, 2), (3, 5)])
def test_staircase_scene_gives_the_levels_it_was_built_for(dhm, nsrc, thres_view):
    """Every bin of the per-pixel level counts, up to 32 sources: pixel p is built to reach k(p) agreeing sources at level
    k(p) and none below, so geo_level = k where k >= thres_view, 0 elsewhere, and geo_mask_sum = k at the loosest level."""
    sc, k = D.staircase_scene(9, 13, nsrc)
    want_level = np.where((k >= thres_view) & (k > 0), k, 0)
    want_sum = k if nsrc >= thres_view else np.where(k <= thres_view, k, 0)          # La = thres_view: sources of k <= La pass
    views, _ = D.restated_scene(sc, thres_view=thres_view)
    got = D.run_host_dynamic(dhm, sc, thres_view=thres_view)
    for level, votes in ((views[0]["geo_level"], views[0]["geo_mask_sum"]), (got["geo_level"][0], got["geo_mask_sum"][0])):
        assert np.array_equal(level, want_level) and np.array_equal(votes, want_sum)
    C.assert_same_values(got["depth_est_averaged"][0], views[0]["depth_est_averaged"], C.AVG_REL)
    if nsrc >= thres_view:
        assert set(np.unique(got["geo_level"]).tolist()) == {0} | set(range(thres_view, nsrc + 1))
    else:
        assert not got["geo_mask"].any()


def test_abi_returns_its_error_codes_without_a_gpu(lib):
    """A NULL pointer, non-positive sizes, Smax = 33, thres_view = 0 and bases that are zero, negative, NaN or infinite
    come back as error codes before any GPU call; the device pointers are stand-in addresses nothing may dereference."""
    from mvster_amd import _lib
    p = 1 << 32
    ptrs = [p] * 14
    sizes = dict(R=2, Smax=3, V=4, H=8, W=8)

    def filt(ptrs=ptrs, thres_view=2, pix_base=0.25, rel_base=1 / 1300, **kw):
        s = dict(sizes, **kw)
        return lib.mvster_geo_scene_filter_dynamic(*ptrs, s["R"], s["Smax"], s["V"], s["H"], s["W"], 0.3, thres_view,
                                                   pix_base, rel_base, None)
    for k in range(14):
        assert filt(ptrs[:k] + [None] + ptrs[k + 1:]) == _lib.ERR_NULL, k
    for name in sizes:
        assert filt(**{name: 0}) == _lib.ERR_SHAPE and filt(**{name: -1}) == _lib.ERR_SHAPE, name
    assert filt(R=1 << 30, H=1 << 15, W=1 << 15) == _lib.ERR_SHAPE
    assert filt(Smax=33) == _lib.ERR_UNSUPPORTED and filt(Smax=1 << 20) == _lib.ERR_UNSUPPORTED
    assert filt(thres_view=0) == _lib.ERR_SHAPE and filt(thres_view=-3) == _lib.ERR_SHAPE
    for bad in (0.0, -0.25, float("nan"), float("inf")):
        assert filt(pix_base=bad) == _lib.ERR_SHAPE, bad
        assert filt(rel_base=bad) == _lib.ERR_SHAPE, bad
    assert filt(ptrs[:3] + [None] + ptrs[4:], Smax=33, thres_view=0) == _lib.ERR_NULL       # pointers are checked first


def test_fuse_scene_checks_the_method_before_touching_a_device():
    """No device is named and every input is a NumPy array: anything but the method check would raise 'runs on MI355X
    only' instead."""
    from mvster_amd import fusion
    sc = C.small_scene()
    args = (sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], 0.3, 2)
    with pytest.raises(RuntimeError, match="unknown fusion method 'bogus'"):
        fusion.fuse_scene(*args, method="bogus")
    with pytest.raises(RuntimeError, match="pix_thres / rel_thres are the fixed thresholds"):
        fusion.fuse_scene(*args, method="dynamic", pix_thres=1.0)
    with pytest.raises(RuntimeError, match="pix_thres / rel_thres are the fixed thresholds"):
        fusion.fuse_scene(*args, method="dynamic", rel_thres=0.01)
    with pytest.raises(RuntimeError, match="runs on MI355X only"):                    # the method itself is accepted
        fusion.fuse_scene(*args, method="dynamic")
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        fusion.fuse_scene(*args, method="normal", pix_thres=1.0, rel_thres=0.01)
    with pytest.raises(RuntimeError, match="unknown fusion method"):
        fusion.filter_depth("nowhere", "nowhere", "nowhere", "nowhere.ply", filter_method="gipuma")
