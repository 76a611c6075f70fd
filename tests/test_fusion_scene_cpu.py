"""Whole-scan fusion without a GPU: the C ABI of the scene kernels (declared, exported, bound, arguments validated before
any GPU call), ``scene_tables`` against ``view_matrices``, and the per-pixel arithmetic of mvster_amd/csrc/geo_math.h --
the functions geo_filter.hip and geo_scene.hip inline -- compiled for the host and run serially over a scan against
oracle/geo_filter_oracle.py."""
import os
import re

import numpy as np
import pytest

from tests import fusion_scene_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvster_geo_scene_blocks", "mvster_geo_scene_filter", "mvster_geo_scene_emit")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ghm():
    return C.load_geo_hostmath()


def test_scene_entry_points_are_declared_exported_and_bound(lib):
    from mvster_amd import _lib
    text = open(os.path.join(ROOT, "include", "mvster_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(mvster_\w+)\s*\(", text))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n
    import mvster_amd
    assert callable(mvster_amd.fuse_scene) and callable(mvster_amd.filter_depth) and callable(mvster_amd.scene_tables)


def test_scene_arguments_are_validated_without_a_gpu(lib):
    """Null pointers, non-positive sizes, Smax <= 0 and an unknown image kind come back as error codes before any GPU
    call; the device pointers are stand-in addresses that nothing may dereference."""
    from mvster_amd import _lib
    p = 1 << 32
    ptrs = [p] * 13
    sizes = dict(R=2, Smax=3, V=4, H=8, W=8)

    def filt(ptrs=ptrs, **kw):
        s = dict(sizes, **kw)
        return lib.mvster_geo_scene_filter(*ptrs, s["R"], s["Smax"], s["V"], s["H"], s["W"], 0.3, 2, 1.0, 0.01, None)
    for k in range(13):
        assert filt(ptrs[:k] + [None] + ptrs[k + 1:]) == _lib.ERR_NULL, k
    for name in sizes:
        assert filt(**{name: 0}) == _lib.ERR_SHAPE and filt(**{name: -1}) == _lib.ERR_SHAPE, name
    assert filt(R=1 << 30, H=1 << 15, W=1 << 15) == _lib.ERR_SHAPE          # more workgroups than a grid holds

    def emit(ptrs=None, kind=0, M=5, R=2, V=4, H=8, W=8):
        a = ptrs or [p] * 8
        return lib.mvster_geo_scene_emit(a[0], a[1], a[2], a[3], a[4], kind, a[5], a[6], a[7], M, R, V, H, W, None)
    for k in range(8):
        assert emit([p] * k + [None] + [p] * (7 - k)) == _lib.ERR_NULL, k
    assert emit(M=-1) == _lib.ERR_SHAPE and emit(R=0) == _lib.ERR_SHAPE and emit(V=0) == _lib.ERR_SHAPE
    assert emit(H=0) == _lib.ERR_SHAPE and emit(W=-3) == _lib.ERR_SHAPE
    assert emit(kind=2) == _lib.ERR_UNSUPPORTED
    assert emit([p] * 6 + [None, None], M=0) == 0                          # an empty cloud needs no buffers and no launch
    assert lib.mvster_geo_scene_blocks(49, 512, 640) == 49 * 1280
    assert lib.mvster_geo_scene_blocks(1, 5, 7) == 1 and lib.mvster_geo_scene_blocks(3, 16, 17) == 6
    assert lib.mvster_geo_scene_blocks(0, 4, 4) == _lib.ERR_SHAPE and lib.mvster_geo_scene_blocks(1, 4, -4) == _lib.ERR_SHAPE


def test_scene_tables_match_view_matrices_bit_for_bit():
    from mvster_amd import fusion
    sc = C.small_scene()
    pairs = [(3, [1]), (0, [6, 2, 4, 5, 1]), (5, [0, 3])] + sc["pairs"]     # ragged, one single-source view, a repeat
    t = fusion.scene_tables(pairs, sc["Ks"], sc["Es"])
    R, smax = len(pairs), 5
    assert t.pair_table.shape == (R, smax) and t.pair_table.dtype == np.int32 and t.ref_view.dtype == np.int32
    assert t.ref_mats.shape == (R, 30) and t.view_mats.shape == (R, smax, 42)
    assert t.ref_mats.dtype == t.view_mats.dtype == np.float64
    for i, (r, srcs) in enumerate(pairs):
        ns = len(srcs)
        assert t.ref_view[i] == r and list(t.pair_table[i, :ns]) == srcs and (t.pair_table[i, ns:] == -1).all()
        rm, vm = fusion.view_matrices(sc["Ks"][r], sc["Es"][r], sc["Ks"][srcs], sc["Es"][srcs])
        assert t.ref_mats[i, :18].tobytes() == rm.tobytes()
        assert t.view_mats[i, :ns].tobytes() == vm.tobytes() and (t.view_mats[i, ns:] == 0).all()
        einv = np.linalg.inv(sc["Es"][r])                                   # float32, as filter_depth inverts it
        assert t.ref_mats[i, 18:].tobytes() == einv[:3].astype(np.float64).tobytes()


@pytest.mark.parametrize("pairs", [[(0, [1, 7])], [(7, [1])], [(0, [-1, 2])], [(0, [])], []])
def test_scene_tables_fail_loudly(pairs):
    from mvster_amd import fusion
    sc = C.small_scene()
    with pytest.raises(RuntimeError):
        fusion.scene_tables(pairs, sc["Ks"], sc["Es"])


def test_fuse_scene_refuses_cpu_only_inputs():
    from mvster_amd import fusion
    sc = C.small_scene()
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], 0.3, 2)
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], 0.3, 2, device="cpu")


run_host_scene = C.run_host_scene

# small_scene with its floor of 0.3, then every hard scene at the thres_view values HARD_CASES lists, with half of the
# oracle-only kept fraction written there as the floor
SCENE_CASES = [pytest.param(None, C.THRES_VIEW, 0.3, id="small_scene")] + [
    pytest.param(case, tv, kept / 2, id="%s-tv%d" % (C.hard_id(case), tv)) for case in C.HARD_CASES
    for tv, kept in sorted(case[4].items())]


@pytest.mark.parametrize("case,thres_view,floor", SCENE_CASES)
def test_geo_math_host_scene_vs_oracle(ghm, case, thres_view, floor):
    """The shared header, serially over the scan: votes, average, back-projection and emission order against the oracle.
    Bounds: vote flips on at most 2e-4 of the pixel-views, depth_est_averaged within 1e-6 relative where the votes
    agree (NaN, +-inf and zero exactly where the oracle has them), world points within one float32 ulp of the cloud's
    largest coordinate where the final masks agree, colours equal."""
    sc = C.small_scene() if case is None else C.hard_scene(*case[:4])
    want_views, want_vertices = C.oracle_scene(sc, thres_view=thres_view)
    if case is not None:                             # the floor in HARD_CASES is what the oracle alone keeps here
        kept = float(np.stack([w["final_mask"] for w in want_views]).mean())
        assert abs(kept - case[4][thres_view]) < 5e-5 and kept > 0, (kept, case[4])
    got = run_host_scene(ghm, sc, thres_view=thres_view)
    fig = C.compare_with_oracle(got, want_views, want_vertices, view_masks=got["view_mask"], floor=floor,
                                thres_view=thres_view)
    print("geo_math host scene vs oracle:", fig)
    if fig["final_mask_mismatch_pixels"] == 0:                               # then the clouds line up vertex by vertex
        assert len(got["points"]) == len(want_vertices)
        assert np.array_equal(got["colors"][:, 0], want_vertices["red"])


def test_hard_cases_cover_the_sizes_the_kernels_go_wrong_at():
    """The list itself: every kind, a map below one wave, between a wave and a workgroup, 256k + 1, 256k - 1, an odd
    width with an even height, a wide and a tall thin shape -- and the degenerate kinds really hold every bad value."""
    hw = [c[0] * c[1] for c in C.HARD_CASES]
    assert {c[3] for c in C.HARD_CASES} == set(C.HARD_KINDS)
    assert any(n < 64 for n in hw) and any(64 < n < 256 for n in hw)
    assert any(n > 256 and n % 256 == 1 for n in hw) and any(n > 256 and n % 256 == 255 for n in hw)
    assert any(c[1] % 2 == 1 and c[0] % 2 == 0 for c in C.HARD_CASES)
    assert any(c[0] >= 100 * c[1] for c in C.HARD_CASES) and any(c[1] >= 100 * c[0] for c in C.HARD_CASES)
    d = C.hard_scene(61, 83, 5, "degenerate")["depths"]
    assert np.isnan(d).any() and np.isposinf(d).any() and (d == 0).any() and (d < 0).any()
    assert (d == np.float32(1e-30)).any() and (d == np.float32(1e30)).any()
    a, b = C.hard_scene(37, 53, 6, "perK"), C.hard_scene(37, 53, 6, "perK")
    assert a["depths"].tobytes() == b["depths"].tobytes() and a["Ks"].tobytes() == b["Ks"].tobytes()    # deterministic
    assert len({k.tobytes() for k in a["Ks"]}) == 6 and max(len(s) for _, s in a["pairs"]) > min(len(s) for _, s in a["pairs"])


def test_compare_with_oracle_understands_non_finite_values():
    """assert_same_values: NaN matches NaN only, inf matches inf of the same sign only, zero stays zero."""
    want = np.array([1.0, np.nan, np.inf, -np.inf, 0.0, 2.0])
    assert C.assert_same_values(want.copy(), want, C.AVG_REL) == 0.0
    assert C.assert_same_values(want * np.where(np.isfinite(want), 1 + 5e-7, 1), want, C.AVG_REL) > 0
    for k, bad in [(0, np.nan), (1, 1.0), (2, -np.inf), (3, np.inf), (2, 1e308), (4, 1e-300), (5, 2.0 + 1e-5), (0, 0.0)]:
        got = want.copy()
        got[k] = bad
        with pytest.raises(AssertionError):
            C.assert_same_values(got, want, C.AVG_REL)


@pytest.mark.parametrize("H,W", [(61, 83), (96, 128), (9, 13), (35, 256)])
def test_pattern_scene_every_pixel_gets_every_vote(ghm, H, W):
    """The premise of the compaction tests on the GPU: with one camera and one noise-free depth map for all views the
    oracle casts every vote, so final_mask is the confidence pattern; the host build agrees and emits the predicted
    colours in the predicted order."""
    V = 3
    pattern = C.pattern_mask("random", V, H, W)
    sc = C.pattern_scene(H, W, V, pattern)
    f32 = dict(sc, images=sc["images"].astype(np.float32) / np.float32(255.0))
    want_views, _ = C.oracle_scene(f32, conf_thres=C.PATTERN_CONF_THRES, thres_view=1)
    for w in want_views:
        assert (w["geo_mask_sum"] == V - 1).all()
    final, counts, colors = C.expected_pattern_cloud(sc, pattern)
    assert np.array_equal(np.stack([w["final_mask"] for w in want_views]), final)
    got = run_host_scene(ghm, sc, conf_thres=C.PATTERN_CONF_THRES, thres_view=1)
    assert (got["geo_mask_sum"] == V - 1).all() and np.array_equal(got["final_mask"], final)
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["colors"], colors)


def test_pattern_masks_are_what_their_names_say():
    R, H, W = 3, 61, 83
    hw = H * W
    m = {n: C.pattern_mask(n, R, H, W).reshape(R, hw) for n in C.PATTERNS}
    assert m["ones"].all() and not m["zeros"].any()
    assert m["first"].sum() == R and m["first"][:, 0].all() and m["last"].sum() == R and m["last"][:, hw - 1].all()
    assert m["lane63"].sum() == R * (hw // 64) and m["lane63"][:, 63::64].all()
    assert m["every65"][:, ::65].all() and m["every65"].sum() == R * len(range(0, hw, 65))
    assert 0.45 < m["random"].mean() < 0.55
    assert not m["per_view"][0].any() and m["per_view"][R - 1].all() and 0.4 < m["per_view"][1].mean() < 0.6


def test_geo_math_host_scene_thres_view_above_every_source_count(ghm):
    sc = C.small_scene()
    got = run_host_scene(ghm, sc, thres_view=6)
    assert len(got["points"]) == 0 and not got["geo_mask"].any() and (got["counts"] == 0).all()
