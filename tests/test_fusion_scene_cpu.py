"""Whole-scan fusion without a GPU: the C ABI of the scene kernels (declared, exported, bound, arguments validated before
any GPU call), ``scene_tables`` against ``view_matrices``, and the per-pixel arithmetic of mvster_amd/csrc/geo_math.h --
the functions geo_filter.hip and geo_scene.hip inline -- compiled for the host and run serially over a scan against
oracle/geo_filter_oracle.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fusion_scene_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTMATH = os.path.join(ROOT, "tests", "hostmath")
NEW = ("mvster_geo_scene_blocks", "mvster_geo_scene_filter", "mvster_geo_scene_emit")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ghm():
    so = os.path.join(HOSTMATH, "libgeohostmath.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HOSTMATH, "geo_hostmath.cpp")])
    h = ctypes.CDLL(so)
    h.hm_geo_scene.restype = ctypes.c_long
    h.hm_geo_scene.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_float,
                                                                          ctypes.c_float] + [ctypes.c_void_p] * 9
    return h


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


def run_host_scene(ghm, sc, conf_thres=C.CONF_THRES, thres_view=C.THRES_VIEW):
    from mvster_amd import fusion
    t = fusion.scene_tables(sc["pairs"], sc["Ks"], sc["Es"])
    R, smax = t.pair_table.shape
    V, H, W = sc["depths"].shape
    out = dict(geo_mask_sum=np.zeros((R, H, W), np.int32), depth_est_averaged=np.zeros((R, H, W), np.float64),
               photo_mask=np.zeros((R, H, W), np.uint8), geo_mask=np.zeros((R, H, W), np.uint8),
               final_mask=np.zeros((R, H, W), np.uint8), view_mask=np.zeros((R, smax, H, W), np.uint8),
               points=np.zeros((R * H * W, 3), np.float32), colors=np.zeros((R * H * W, 3), np.uint8),
               counts=np.zeros(R, np.int64))
    ins = [np.ascontiguousarray(a) for a in (sc["depths"], sc["conf"], sc["images"], t.pair_table, t.ref_view, t.ref_mats,
                                             t.view_mats)]
    assert ins[0].dtype == ins[1].dtype == ins[2].dtype == np.float32
    m = ghm.hm_geo_scene(*[a.ctypes.data for a in ins], R, smax, V, H, W, conf_thres, thres_view, 1.0, 0.01,
                         *[out[k].ctypes.data for k in ("geo_mask_sum", "depth_est_averaged", "photo_mask", "geo_mask",
                                                        "final_mask", "view_mask", "points", "colors", "counts")])
    assert m >= 0
    for k in ("photo_mask", "geo_mask", "final_mask"):
        out[k] = out[k].astype(bool)
    out["points"], out["colors"] = out["points"][:m], out["colors"][:m]
    return out


def test_geo_math_host_scene_vs_oracle(ghm):
    """The shared header, serially over the scan: votes, average, back-projection and emission order against the oracle.
    Bounds: vote flips on at most 2e-4 of the pixel-views, depth_est_averaged within 1e-6 relative where the votes
    agree, world points within one float32 ulp of the cloud's largest coordinate where the final masks agree, colours
    equal."""
    sc = C.small_scene()
    want_views, want_vertices = C.oracle_scene(sc)
    got = run_host_scene(ghm, sc)
    fig = C.compare_with_oracle(got, want_views, want_vertices, view_masks=got["view_mask"])
    print("geo_math host scene vs oracle:", fig)
    if fig["final_mask_mismatch_pixels"] == 0:                               # then the clouds line up vertex by vertex
        assert len(got["points"]) == len(want_vertices)
        assert np.array_equal(got["colors"][:, 0], want_vertices["red"])


def test_geo_math_host_scene_thres_view_above_every_source_count(ghm):
    sc = C.small_scene()
    got = run_host_scene(ghm, sc, thres_view=6)
    assert len(got["points"]) == 0 and not got["geo_mask"].any() and (got["counts"] == 0).all()
