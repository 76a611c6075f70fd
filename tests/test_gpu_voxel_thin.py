"""Voxel-grid thinning on the GPU (``fusion.thin_points``: mvster_voxel_thin_insert + mvster_voxel_thin_emit, DESIGN.md section
4.16): bit for bit against the host build of mvster_amd/csrc/voxel_math.h on every case cloud of tests/voxel_thin_cases.py,
independent of the table size and of the run, and through ``fuse_scene`` / ``filter_depth`` / ``reconstruct_scan``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mvster_amd import MVS4net, _lib, formats, fusion, scan
from tests import fusion_scene_cases as C
from tests import scan_dataset_cases as DC
from tests import scan_short_cases as SS
from tests import voxel_thin_cases as T

DEV = "cuda:0"
COMPILERS = ("g++", "clang++")              # ROCm's clang++ as a host-only compiler where there is no g++


def thin_gpu(points, colors, v, reduce, **kw):
    """fusion.thin_points on NumPy arrays -> dict of NumPy arrays."""
    out = fusion.thin_points(torch.from_numpy(points).to(DEV), torch.from_numpy(colors).to(DEV), v, reduce, **kw)
    assert isinstance(out["dropped"], int) and set(out) == set(T.KEYS) | {"dropped"}
    return {k: (t.cpu().numpy() if torch.is_tensor(t) else t) for k, t in out.items()}


def thinned_part(res):
    """The thin_* entries of a SceneResult as a thinning result (NumPy arrays)."""
    return dict({k: res["thin_" + k].cpu().numpy() for k in T.KEYS}, dropped=res["thin_dropped"])


def same_bytes(a, b, keys):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("reduce", T.REDUCES)
@pytest.mark.parametrize("v", T.VOXEL_SIZES)
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_case_cloud_equals_the_host_build_bit_for_bit(name, v, reduce):
    pts, cols = T.case_clouds(v, COMPILERS)[name]
    want = T.host_case(name, v, reduce, COMPILERS)
    got = thin_gpu(pts, cols, v, reduce)
    print("thin %s v=%g %s: %d points -> %d voxels, %d dropped" % (name, v, reduce, len(pts), len(got["first"]), got["dropped"]))
    T.assert_same(got, want, name)


def random_cloud(M, v, seed):
    """Half of the points crowd into about 150 voxels, the other half are mostly alone in theirs; 1 % are NaN."""
    rng = np.random.RandomState(seed)
    scale = np.where(rng.rand(M, 1) < 0.5, 0.1, 1.0) * np.array([30.0, 40.0, 15.0])
    pts = ((rng.rand(M, 3) * 2 - 1) * v * scale).astype(np.float32)
    pts[rng.rand(M) < 0.01] = np.nan
    return pts, rng.randint(0, 256, (M, 3)).astype(np.uint8)


@pytest.mark.parametrize("reduce", T.REDUCES)
def test_result_does_not_depend_on_the_table_size_or_on_the_run(reduce):
    v = 0.3
    clouds = dict(T.case_clouds(v, COMPILERS), random=random_cloud(100003, v, seed=5))
    for name in ("colliding", "m257", "one_voxel", "faces", "invalid", "random"):
        pts, cols = clouds[name]
        base = thin_gpu(pts, cols, v, reduce)
        if name == "random":                                                 # 391 workgroups, shared and single voxels
            T.assert_same(base, T.thin_numpy(pts, cols, v, reduce), name)
            assert base["counts"].max() > 8 and (base["counts"] == 1).sum() > 100 and base["dropped"] > 500
        slots = fusion.thin_slots(len(pts))
        for other in (2 * slots, 16 * slots):
            T.assert_same(thin_gpu(pts, cols, v, reduce, table_slots=other), base, (name, other))
        T.assert_same(thin_gpu(pts, cols, v, reduce, table_slots=slots), base, (name, "explicit default"))
        T.assert_same(thin_gpu(pts, cols, v, reduce), base, (name, "second run"))


def test_table_slots_is_checked_on_the_host_before_any_launch():
    pts, cols = random_cloud(1000, 0.3, seed=6)
    p, c = torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV)
    for slots in (1024, 1000, 3000, 2047, 0):                                # below 2 * M, or not a power of two
        with pytest.raises(RuntimeError, match="table_slots"):
            fusion.thin_points(p, c, 0.3, table_slots=slots)
    # and below the Python checks, at the C ABI: MVSTER_ERR_SHAPE, the scratch untouched
    lib = _lib.load()
    nblk = lib.mvster_voxel_thin_blocks(1000)
    assert nblk == 4 and lib.mvster_voxel_thin_blocks(0) == _lib.ERR_SHAPE
    scratch = torch.full((3 * 4096 + 1000 + nblk + 2 * (nblk + 3),), -7, dtype=torch.int32, device=DEV)
    keys, first, slot = scratch[:2 * 4096], scratch[2 * 4096:3 * 4096], scratch[3 * 4096:3 * 4096 + 1000]
    wgc, wgo = scratch[3 * 4096 + 1000:3 * 4096 + 1000 + nblk], scratch[3 * 4096 + 1000 + nblk:]
    stream = torch.cuda.current_stream().cuda_stream
    for slots, voxel in ((1024, 0.3), (3000, 0.3), (32, 0.3), (4096, 0.0), (4096, float("inf"))):
        rc = lib.mvster_voxel_thin_insert(p.data_ptr(), 1000, voxel, keys.data_ptr(), first.data_ptr(), slots, slot.data_ptr(),
                                          wgc.data_ptr(), wgo.data_ptr(), stream)
        assert rc == _lib.ERR_SHAPE, (slots, voxel)
    torch.cuda.synchronize()
    assert bool((scratch == -7).all())
    assert thin_gpu(pts, cols, 0.3, "mean", table_slots=2048)["dropped"] == int(np.isnan(pts).any(1).sum())


def odd_scene_result(**kw):
    sc = C.hard_scene(61, 83, 5, "plain")                                    # 5063 pixels per view: a tail workgroup
    return fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], C.CONF_THRES, C.THRES_VIEW,
                             device=DEV, **kw)


def scene_voxel(points):
    """An edge that puts several points of a scan's cloud into most voxels: 1/24 of the cloud's largest extent."""
    p = points[torch.isfinite(points).all(1)]
    return float((p.max(0)[0] - p.min(0)[0]).max()) / 24


@pytest.mark.parametrize("reduce", T.REDUCES)
def test_fuse_scene_thins_its_whole_cloud_and_leaves_the_rest_alone(reduce):
    plain = odd_scene_result()
    v = scene_voxel(plain["points"])
    res = odd_scene_result(voxel_size=v, voxel_reduce=reduce)
    assert set(res) == set(plain) | {"thin_points", "thin_colors", "thin_counts", "thin_first", "thin_dropped"}
    same_bytes(res, plain, list(plain))
    want = T.thin_numpy(plain["points"].cpu().numpy(), plain["colors"].cpu().numpy(), v, reduce)
    T.assert_same(thinned_part(res), want, reduce)
    M, U = len(plain["points"]), len(want["first"])
    print("fuse_scene 61x83x5, voxel %.4g, %s: %d points -> %d" % (v, reduce, M, U))
    assert M > 10000 and 100 < U < M / 2 and want["dropped"] == 0
    assert res.vertices().tobytes() == plain.vertices().tobytes() and len(res.vertices(thinned=True)) == U
    chunks = odd_scene_result(voxel_size=v, voxel_reduce=reduce, scratch_budget=1)      # one reference view per chunk
    same_bytes(chunks, res, [k for k in res if k != "thin_dropped"])
    assert chunks["thin_dropped"] == res["thin_dropped"] == 0
    with pytest.raises(RuntimeError, match="no thinned cloud"):
        plain.vertices(thinned=True)


def test_a_scan_without_survivors_gives_an_empty_thinned_cloud():
    sc = C.hard_scene(1, 300, 3, "plain")                                    # one row of pixels: nothing survives thres_view 2
    res = fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], C.CONF_THRES, 2, device=DEV,
                            voxel_size=0.2)
    assert len(res["points"]) == 0 and res["thin_dropped"] == 0
    for k, shape, dtype in (("points", (0, 3), torch.float32), ("colors", (0, 3), torch.uint8), ("counts", (0,), torch.int32),
                            ("first", (0,), torch.int64)):
        t = res["thin_" + k]
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda, k
    assert len(res.vertices(thinned=True)) == 0


def test_filter_depth_writes_the_thinned_cloud(tmp_path):
    from PIL import Image
    sc = C.small_scene()
    ids = [v * 3 + 1 for v in range(7)]                                           # file numbers are not stack indices
    folder, out = tmp_path / "scan", tmp_path / "out"
    for d in (folder / "cams", folder / "images", out / "depth_est", out / "confidence"):
        os.makedirs(d)
    rng = np.random.RandomState(8)
    for v, i in enumerate(ids):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3] = sc["Es"][v], sc["Ks"][v], [425.0, 2.5, 192, 905.0]
        formats.write_cam(str(folder / "cams" / ("%08d_cam.txt" % i)), cam)
        Image.fromarray(rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)).save(str(folder / "images" / ("%08d.jpg" % i)))
        formats.save_pfm(str(out / "depth_est" / ("%08d.pfm" % i)), sc["depths"][v])
        formats.save_pfm(str(out / "confidence" / ("%08d.pfm" % i)), sc["conf"][v])
    pairs = [(0, [1, 2, 3]), (4, [5, 6, 0, 2]), (6, [5, 4, 3])]
    with open(folder / "pair.txt", "w") as f:
        f.write("%d\n" % len(pairs))
        for r, srcs in pairs:
            f.write("%d\n%d %s\n" % (ids[r], len(srcs), " ".join("%d 1.0" % ids[s] for s in srcs)))
    full = fusion.filter_depth(str(folder), str(folder), str(out), str(tmp_path / "full.ply"), conf=0.3, thres_view=2)
    v = scene_voxel(torch.from_numpy(np.stack([full[c] for c in "xyz"], 1)))
    for reduce in T.REDUCES:
        ply = str(tmp_path / (reduce + ".ply"))
        vertices = fusion.filter_depth(str(folder), str(folder), str(out), ply, conf=0.3, thres_view=2, voxel_size=v,
                                       voxel_reduce=reduce)
        back = fusion.read_ply(ply)
        want = T.thin_numpy(np.stack([full[c] for c in "xyz"], 1), np.stack([full[c] for c in ("red", "green", "blue")], 1), v, reduce)
        assert back.tobytes() == vertices.tobytes() and 100 < len(back) == len(want["first"]) < len(full) / 2
        assert np.stack([back[c] for c in "xyz"], 1).tobytes() == want["points"].tobytes()
        assert np.stack([back[c] for c in ("red", "green", "blue")], 1).tobytes() == want["colors"].tobytes()
    assert fusion.read_ply(str(tmp_path / "full.ply")).tobytes() == full.tobytes()


def test_reconstruct_scan_writes_the_thinned_cloud(shipped_cfg, checkpoint, tmp_path):
    model = MVS4net(**shipped_cfg)
    model.load_state_dict(checkpoint, strict=True)
    model = model.to(DEV).eval()
    root = str(tmp_path)
    DC.write_dataset_folder(root, "Family", DC.dataset_scan([(184, 128)] * 6, seed=31), SS.PAIRS)
    d = SS.decode_all(root, "Family", "cams", None, 6)
    kw = dict(nviews=SS.NVIEWS, depth_range_kind="min_max", crop_rows=(28, 28), short_sources="fewer_views", conf=0.05,
              thres_view=1)
    args = (model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS)
    plain = scan.reconstruct_scan(*args, plyfilename=str(tmp_path / "full.ply"), **kw)
    v = scene_voxel(plain["points"])
    got = scan.reconstruct_scan(*args, plyfilename=str(tmp_path / "thin.ply"), voxel_size=v, voxel_reduce="mean", **kw)
    same_bytes(got, plain, list(plain))
    want = T.thin_numpy(plain["points"].cpu().numpy(), plain["colors"].cpu().numpy(), v, "mean")
    T.assert_same(thinned_part(got), want)
    back = fusion.read_ply(str(tmp_path / "thin.ply"))
    print("reconstruct_scan, Tanks-like, voxel %.4g: %d points -> %d" % (v, len(plain["points"]), len(back)))
    assert back.tobytes() == got.vertices(thinned=True).tobytes() and 0 < len(back) == len(want["first"]) < len(plain["points"])
    assert fusion.read_ply(str(tmp_path / "full.ply")).tobytes() == plain.vertices().tobytes()
    with pytest.raises(RuntimeError, match="voxel_size"):
        scan.reconstruct_scan(*args, voxel_size=0.0, **kw)
