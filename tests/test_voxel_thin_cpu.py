"""Voxel-grid thinning without a GPU: the host build of mvster_amd/csrc/voxel_math.h against the NumPy
restatement bit for bit, the properties the definition promises, and the argument checks of the Python entry points."""
import inspect

import numpy as np
import pytest
import torch

from mvster_amd import fusion, scan
from tests import voxel_thin_cases as T


@pytest.fixture(scope="module")
def vhm():
    return T.load_voxel_hostmath()


@pytest.mark.parametrize("v", T.VOXEL_SIZES)
def test_case_clouds_are_what_they_claim(vhm, v):
    clouds = T.case_clouds(v)
    assert tuple(clouds) == T.CASE_NAMES
    assert [len(clouds["m%d" % m][0]) for m in (0, 1, 63, 64, 65, 257)] == [0, 1, 63, 64, 65, 257]
    one, distinct = T.thin_numpy(*clouds["one_voxel"], v, "mean"), T.thin_numpy(*clouds["distinct"], v, "mean")
    assert one["counts"].tolist() == [4096] and one["dropped"] == 0
    assert distinct["counts"].tolist() == [1] * 4096 and distinct["first"].tolist() == list(range(4096))
    half = T.thin_numpy(*clouds["half"], v, "mean")
    assert half["counts"].tolist() == [2] and half["colors"].tolist() == [[11, 1, 255]]          # x.5 rounds up
    # the clamp is hit: some face value has (q - i) * 65536 == 65536
    f = T.face_values(v).astype(np.float64) / np.float64(np.float32(v))
    assert ((f - np.floor(f)) * 65536.0 >= 65536.0).any()
    valid, _, t, _ = T.point_terms(clouds["faces"][0], v)
    assert valid.all() and t.max() == 65535 and t.min() == 0
    bad = T.thin_numpy(*clouds["invalid"], v, "mean")
    assert bad["dropped"] == 28 and bad["counts"].sum() == len(clouds["invalid"][0]) - 28
    empty = T.thin_numpy(*clouds["all_invalid"], v, "mean")
    assert empty["dropped"] == 70 and len(empty["points"]) == 0
    col = T.thin_numpy(*clouds["colliding"], v, "mean")
    assert len(col["counts"]) == T.COLLIDING_VOXELS and sorted(col["counts"].tolist()) == [1] * 160 + [2] * 40
    assert T.default_slots(len(clouds["colliding"][0])) == 512 == fusion.thin_slots(len(clouds["colliding"][0]))


@pytest.mark.parametrize("reduce", T.REDUCES)
@pytest.mark.parametrize("v", T.VOXEL_SIZES)
def test_host_build_equals_the_restatement_on_every_case_cloud(vhm, v, reduce):
    for name, (pts, cols) in T.case_clouds(v).items():
        valid, _, t, key = T.point_terms(pts, v)
        hv, hkey, ht = T.host_point_terms(vhm, pts, v)
        assert np.array_equal(valid, hv) and np.array_equal(key, hkey) and np.array_equal(t, ht), name
        T.assert_same(T.host_case(name, v, reduce), T.thin_numpy(pts, cols, v, reduce), name)


def random_cloud(M, v, seed):
    """Points around the origin at mixed scales with the special values of the case clouds mixed in."""
    rng = np.random.RandomState(seed)
    v64 = np.float64(np.float32(v))
    pts = ((rng.rand(M, 3) * 2 - 1) * v64 * np.array([3.0, 40.0, 0.9])).astype(np.float32)
    special = np.concatenate([T.face_values(v), np.array([np.nan, np.inf, -np.inf, 3e38, 2.0 ** 21 * v], np.float32)])
    where = rng.rand(M, 3) < 0.02
    pts[where] = special[rng.randint(0, len(special), int(where.sum()))]
    return pts, rng.randint(0, 256, (M, 3)).astype(np.uint8)


@pytest.mark.parametrize("v", T.VOXEL_SIZES)
def test_host_build_equals_the_restatement_on_200000_random_points(vhm, v):
    pts, cols = random_cloud(200000, v, seed=3)
    valid, _, t, key = T.point_terms(pts, v)
    hv, hkey, ht = T.host_point_terms(vhm, pts, v)
    assert np.array_equal(valid, hv) and np.array_equal(key, hkey) and np.array_equal(t, ht)
    assert 1000 < (~valid).sum() < 30000 and (t == 65535).sum() > 0
    for reduce in T.REDUCES:
        want = T.thin_numpy(pts, cols, v, reduce)
        T.assert_same(T.thin_host(vhm, pts, cols, v, reduce), want, reduce)
        assert want["counts"].max() > 4 and (want["counts"] == 1).sum() > 100


@pytest.mark.parametrize("v", T.VOXEL_SIZES)
def test_mean_lies_inside_its_voxel_and_first_is_a_subset_in_input_order(vhm, v):
    pts, cols = random_cloud(50000, v, seed=4)
    clouds = [(pts, cols)] + [T.case_clouds(v)[n] for n in ("faces", "one_voxel", "colliding", "m257")]
    v64 = np.float64(np.float32(v))
    for p, c in clouds:
        mean, first = T.thin_host(vhm, p, c, v, "mean"), T.thin_host(vhm, p, c, v, "first")
        _, i, _, _ = T.point_terms(p, v)
        cell = i[mean["first"]].astype(np.float64)
        lo, hi = (cell * v64).astype(np.float32), ((cell + 1) * v64).astype(np.float32)      # the faces, rounded like the mean
        assert ((mean["points"] >= lo) & (mean["points"] <= hi)).all()
        f = first["first"]
        assert (np.diff(f) > 0).all() and np.array_equal(f, mean["first"]) and np.array_equal(first["counts"], mean["counts"])
        assert first["points"].tobytes() == p[f].tobytes() and first["colors"].tobytes() == c[f].tobytes()
        assert first["counts"].sum() + first["dropped"] == len(p)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------

P, CL = torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8)


@pytest.mark.parametrize("bad", [0, -0.2, float("nan"), float("inf"), 1e-60, 1e60, None, "abc"])
def test_thin_points_rejects_a_bad_voxel_size(bad):
    with pytest.raises(RuntimeError, match="voxel_size"):
        fusion.thin_points(P, CL, bad)


def test_thin_points_checks_its_arguments_before_the_gpu():
    with pytest.raises(RuntimeError, match="unknown voxel reduction"):
        fusion.thin_points(P, CL, 0.2, reduce="median")
    with pytest.raises(RuntimeError, match=r"points must be \[M,3\] float32"):
        fusion.thin_points(P.double(), CL, 0.2)
    with pytest.raises(RuntimeError, match=r"points must be \[M,3\] float32"):
        fusion.thin_points(torch.zeros(5, 4), CL, 0.2)
    with pytest.raises(RuntimeError, match=r"colors must be \[M,3\] uint8"):
        fusion.thin_points(P, CL[:4], 0.2)
    with pytest.raises(RuntimeError, match=r"colors must be \[M,3\] uint8"):
        fusion.thin_points(P, CL.float(), 0.2)
    with pytest.raises(RuntimeError, match="torch tensors"):
        fusion.thin_points(P.numpy(), CL.numpy(), 0.2)
    for slots in (48, 63, 100, 32, 0, -64, 64.0, 1 << 31):                   # not a power of two, too small, not an int, too large
        with pytest.raises(RuntimeError, match="table_slots"):
            fusion.thin_points(torch.zeros(33, 3), torch.zeros(33, 3, dtype=torch.uint8), 0.2, table_slots=slots)
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # everything else is fine: only the device is not
        fusion.thin_points(P, CL, 0.2, table_slots=64)
    assert [fusion.thin_slots(m) for m in (0, 1, 32, 33, 64, 65, 240, 257)] == [64, 64, 64, 128, 128, 256, 512, 1024]


def test_entry_points_check_the_voxel_keywords_before_anything_else():
    z = np.zeros((2, 4, 4), np.float32)
    for kw, match in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=-1), "voxel_size"),
                      (dict(voxel_size=float("nan")), "voxel_size"), (dict(voxel_size=0.2, voxel_reduce="median"),
                                                                      "unknown voxel reduction")):
        with pytest.raises(RuntimeError, match="fuse_scene: .*" + match):
            fusion.fuse_scene(z, z, np.zeros((2, 4, 4, 3), np.uint8), [np.eye(3)] * 2, [np.eye(4)] * 2, [(0, [1])], 0.3, 1, **kw)
        with pytest.raises(RuntimeError, match="filter_depth: .*" + match):
            fusion.filter_depth("nowhere", "nowhere", "nowhere", "nowhere.ply", **kw)
        with pytest.raises(RuntimeError, match="reconstruct_scan: .*" + match):
            scan.reconstruct_scan(None, None, None, None, None, None, **kw)
    for fn, names in ((fusion.fuse_scene, ("voxel_size", "voxel_reduce")), (fusion.filter_depth, ("voxel_size", "voxel_reduce")),
                      (scan.reconstruct_scan, ("voxel_size", "voxel_reduce"))):
        sig = inspect.signature(fn).parameters
        assert [sig[n].default for n in names] == [None, "mean"], fn


def test_vertices_thinned_without_a_thinned_cloud_raises():
    res = fusion.SceneResult(points=torch.zeros(2, 3), colors=torch.zeros(2, 3, dtype=torch.uint8))
    assert len(res.vertices()) == 2 and len(res.vertices(thinned=False)) == 2
    with pytest.raises(RuntimeError, match="no thinned cloud"):
        res.vertices(thinned=True)
    res.update(thin_points=torch.ones(1, 3), thin_colors=torch.full((1, 3), 7, dtype=torch.uint8))
    v = res.vertices(thinned=True)
    assert len(v) == 1 and v["x"][0] == 1.0 and v["blue"][0] == 7
