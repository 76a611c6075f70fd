"""Cleaning a fused cloud on the GPU (``fusion.nearest_neighbors`` / ``radius_outliers`` / ``statistical_outliers`` /
``estimate_normals``: csrc/geo_knn.hip): every output byte for byte against the host build of
mvster_amd/csrc/knn_math.h on the cases of tests/cloud_clean_cases.py, independent of the cell, the table and the run; the
filters on clouds with a known answer; the normals against numpy.linalg.eigh; and the keywords of ``fuse_scene`` /
``filter_depth`` / ``reconstruct_scan``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mvster_amd import MVS4net, dtu_eval, formats, fusion, scan
from tests import cloud_clean_cases as K
from tests import cloud_nn_cases as N
from tests import fusion_scene_cases as C
from tests import scan_dataset_cases as DC
from tests import scan_short_cases as SS

DEV = "cuda:0"
COMPILERS = ("g++", "clang++")              # ROCm's clang++ as a host-only compiler where there is no g++


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host():
    return K.load_knn_hostmath(COMPILERS)


def to_numpy(out):
    return {k: (t.cpu().numpy() if torch.is_tensor(t) else t) for k, t in out.items()}


def knn_gpu(q, t, k, md, cell=None, same=False, **kw):
    """fusion.nearest_neighbors on NumPy arrays -> dict of NumPy arrays; ``same``: one tensor as query and target."""
    td = dev(t)
    out = to_numpy(fusion.nearest_neighbors(td if same else dev(q), td, k, md, cell, **kw))
    assert set(out) == set(K.KNN_KEYS) | {"dropped_query", "dropped_target"}
    return out


_HOST = {}


def host_knn(name, k, ex, cell):
    """The host brute force of a case, computed once per process and never modified."""
    key = (name, k, ex, cell)
    if key not in _HOST:
        q, t, md, _ = K.knn_cases()[name]
        _HOST[key] = K.knn_host(host(), q, t, k, md, cell, ex)
    return _HOST[key]


# ---- k nearest ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.KNN_CASE_NAMES)
def test_case_equals_the_host_brute_force_bit_for_bit(name):
    """Every k of the case (k > M among them: m1, boundary, the empty and invalid clouds), exclude_self on and off where the query
    is the target, at the default cell."""
    q, t, md, same = K.knn_cases()[name]
    cell = N.default_cell(md)
    for k in K.case_ks(name):
        for ex in ((False, True) if same else (False,)):
            got = knn_gpu(q, t, k, md, same=same, exclude_self=ex)
            print("knn %s k=%d exclude_self=%s: %d -> %d, counts %s" % (name, k, ex, len(q), len(t), np.bincount(got["count"], minlength=1)[:8]))
            K.assert_same_knn(got, host_knn(name, k, ex, cell), (name, k, ex))


@pytest.mark.parametrize("name", ("random", "ties", "invalid", "one_cell", "m0", "q0"))
def test_k_1_is_nearest_distances(name):
    q, t, md = N.cases()[name]
    nn = to_numpy(fusion.nearest_distances(dev(q), dev(t), md))
    got = knn_gpu(q, t, 1, md)
    K.assert_bytes(got["dist2"][:, 0], nn["dist2"], name)
    K.assert_bytes(got["index"][:, 0], nn["index"], name)
    assert (got["count"] == (nn["index"] >= 0)).all() and got["dropped_target"] == nn["dropped_target"]


@pytest.mark.parametrize("name", ("lattice", "duplicates", "stop_rule", "faces", "invalid", "single_cell", "boundary", "pair_random"))
def test_cell_table_and_run_do_not_change_a_byte(name):
    """Three cell sizes (max_dist / 15, the default, 4 max_dist), 1 x and 16 x the table, a second run, reused grids."""
    q, t, md, same = K.knn_cases()[name]
    k = K.case_ks(name)[0]
    c = N.cell_values(md)
    for cell in (c[0], c[1], c[3]):
        want = host_knn(name, k, same, cell)                                 # (validity, and only it, depends on the cell)
        for slots in (None, 16 * fusion.thin_slots(len(t))):
            for run in range(2):
                K.assert_same_knn(knn_gpu(q, t, k, md, cell, same=same, exclude_self=same, table_slots=slots), want, (name, cell, slots, run))
        tg = fusion.CloudGrid(dev(t), cell)
        qg = tg if same else fusion.CloudGrid(dev(q), cell)
        K.assert_same_knn(to_numpy(fusion.nearest_neighbors(qg, tg, k, md, exclude_self=same)), want, (name, cell, "grids"))
    if name == "lattice":
        assert all(K.knn_host(host(), q, t, k, md, cell, True)["dist2"].tobytes() == want["dist2"].tobytes() for cell in c[:2])
        with pytest.raises(RuntimeError, match="has cell"):
            fusion.nearest_neighbors(tg, tg, k, md, cell=c[1])


def test_a_cloud_of_100003_points_at_k_20():
    pts = K.scale_cloud()
    cell = N.default_cell(K.MD)
    want = K.knn_host(host(), pts, pts, 20, K.MD, cell, True, grid=True)     # (the CPU tests prove grid = brute force)
    got = knn_gpu(pts, pts, 20, K.MD, same=True, exclude_self=True)
    print("knn 100 003 points, k = 20: %d full lists, %d empty, %d dropped" % ((got["count"] == 20).sum(), (got["count"] == 0).sum(),
                                                                               got["dropped_query"]))
    K.assert_same_knn(got, want, "scale")
    assert (got["count"] == 20).sum() > 40000 and 0 < (got["count"] < 20).sum()


# ---- the filters and the normals against the host build ------------------------------------------------------------------

SELF_CLOUDS = ("lattice", "duplicates", "single_cell", "self_random", "invalid", "all_invalid", "empty", "faces")


def check_filter(out, pts, keep, extra=()):
    assert set(out) == {"keep", "index", "points", "dropped"} | set(extra)
    K.assert_bytes(out["keep"], keep, "keep")
    K.assert_bytes(out["index"], np.nonzero(keep)[0].astype(np.int64), "index")
    K.assert_bytes(out["points"], pts[keep], "points")


@pytest.mark.parametrize("name", SELF_CLOUDS)
def test_radius_outliers_equal_the_host_build(name):
    pts = K.knn_cases()[name][0]
    md = K.knn_cases()[name][2]
    cell = N.default_cell(md)
    for nb_points in (1, 4):
        nb, keep = K.radius_host(host(), pts, md, nb_points, cell)
        for run in range(2):
            got = to_numpy(fusion.radius_outliers(dev(pts), md, nb_points))
            K.assert_bytes(got["neighbours"], nb, (name, "neighbours"))
            check_filter(got, pts, keep, ("neighbours",))
            assert got["dropped"] == (~N.valid_points(pts, cell)).sum()
    other = to_numpy(fusion.radius_outliers(fusion.CloudGrid(dev(pts), N.cell_values(md)[3]), md, 4))
    if name not in ("invalid", "faces"):
        K.assert_bytes(other["neighbours"], nb, (name, "another cell"))


def same_float(a, b):
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("name", SELF_CLOUDS)
def test_statistical_outliers_equal_the_host_build(name):
    pts = K.knn_cases()[name][0]
    md = K.knn_cases()[name][2]
    cell = N.default_cell(md)
    for k, ratio in ((1, 0.0), (6, 1.5), (32, -0.5)):
        want = K.statistical_host(host(), pts, k, ratio, md, cell)
        for run in range(2):
            got = to_numpy(fusion.statistical_outliers(dev(pts), k, ratio, md))
            K.assert_bytes(got["mean"], want["mean"], (name, k, "mean"))
            print("statistical %s k=%d: n %d mu %.17g sigma %.17g threshold %.17g, %d kept" % (name, k, got["n"], got["mu"], got["sigma"],
                                                                                              got["threshold"], got["keep"].sum()))
            assert got["n"] == want["n"] and all(same_float(got[key], want[key]) for key in ("mu", "sigma", "threshold")), (got, want)
            check_filter(got, pts, want["keep"], ("mean", "n", "mu", "sigma", "threshold"))


@pytest.mark.parametrize("name", SELF_CLOUDS)
def test_normals_equal_the_host_build(name):
    pts = K.knn_cases()[name][0]
    md = K.knn_cases()[name][2]
    cell = N.default_cell(md)
    rng = np.random.RandomState(1)
    toward = (rng.rand(len(pts), 3) * 4 - 2).astype(np.float32) * np.float32(md)
    for k in (2, 7, 32):
        for tw in (None, toward):
            want = K.normals_host(host(), pts, k, md, cell, toward=tw)
            for run in range(2):
                got = to_numpy(fusion.estimate_normals(dev(pts), k, md, toward=None if tw is None else dev(tw)))
                assert set(got) == {"normals", "valid"}
                K.assert_bytes(got["valid"], want["valid"], (name, k, "valid"))
                K.assert_bytes(got["normals"], want["normals"], (name, k, "normals"))


# ---- filters on clouds with a known answer -----------------------------------------------------------------------------------

def test_radius_filter_on_a_lattice_lone_points_and_a_pair():
    pts, kinds = K.radius_cloud()
    cols = np.random.RandomState(2).randint(0, 256, (len(pts), 3)).astype(np.uint8)
    for nb_points in (1, 2):
        got = to_numpy(fusion.radius_outliers(dev(pts), K.RADIUS, nb_points, colors=dev(cols)))
        want = (kinds == 0) | ((kinds == 2) & (nb_points == 1))
        assert got["keep"].tolist() == want.tolist() and got["dropped"] == 2
        check_filter(got, pts, want, ("neighbours", "colors"))
        K.assert_bytes(got["colors"], cols[want], "colors")
        nb, keep = K.radius_host(host(), pts, K.RADIUS, nb_points, N.default_cell(K.RADIUS))
        K.assert_bytes(got["neighbours"], nb)
        assert keep.tolist() == want.tolist()


def test_statistical_filter_on_a_blob_with_planted_points():
    """Every planted point is removed; keep is exact for the returned threshold; the threshold is within 1e-12 relative of the
    restatement (NumPy's pairwise sums over n <= 4112 terms of one sign: n 2^-53 = 4.6e-13)."""
    pts, planted = K.blob_cloud()
    cell = N.default_cell(K.STAT_MD)
    got = to_numpy(fusion.statistical_outliers(dev(pts), K.STAT_K, K.STAT_RATIO, K.STAT_MD))
    want_mean = K.mean_numpy(K.knn_numpy(pts, pts, K.STAT_K, K.STAT_MD, cell, True), K.STAT_K)
    n, mu, sigma, threshold = K.stats_numpy(want_mean, K.STAT_RATIO)
    print("blob: n %d, mu %.17g (NumPy %.17g), sigma %.17g (%.17g), threshold %.17g (%.17g), %d kept" %
          (got["n"], got["mu"], mu, got["sigma"], sigma, got["threshold"], threshold, got["keep"].sum()))
    K.assert_bytes(got["mean"], want_mean, "mean")
    assert got["n"] == n
    assert abs(got["threshold"] - threshold) <= 1e-12 * threshold and abs(got["mu"] - mu) <= 1e-12 * mu
    with np.errstate(invalid="ignore"):
        assert got["keep"].tolist() == (np.isfinite(got["mean"]) & (got["mean"] <= got["threshold"])).tolist()
    assert not got["keep"][planted].any() and got["keep"][~planted].mean() > 0.9
    check_filter(got, pts, got["keep"], ("mean", "n", "mu", "sigma", "threshold"))
    want = K.statistical_host(host(), pts, K.STAT_K, K.STAT_RATIO, K.STAT_MD, cell)
    assert (got["n"], got["mu"], got["sigma"], got["threshold"]) == (want["n"], want["mu"], want["sigma"], want["threshold"])
    K.assert_bytes(got["keep"], want["keep"])


# ---- normals -------------------------------------------------------------------------------------------------------------------

def test_normals_of_a_noisy_plane_against_eigh():
    """Within 1e-6 rad of numpy.linalg.eigh on the restatement's covariance (float32 output: about 1e-7 rad; fp64 eigenvector
    error <= eps ||C|| / gap with gap >= 1e-3), for every point: all are valid and all satisfy the gap condition."""
    pts, k, md = K.plane_cloud()
    want, valid, gap = K.normals_numpy(pts, K.knn_numpy(pts, pts, k, md, N.default_cell(md), True))
    got = to_numpy(fusion.estimate_normals(dev(pts), k, md))
    ang = K.angles(got["normals"], want)
    print("plane: smallest gap %.3g, largest angle %.3g rad" % (gap.min(), ang.max()))
    assert valid.all() and got["valid"].all() and gap.min() >= K.GAP
    assert ang.max() <= K.ANGLE
    K.assert_bytes(got["normals"], K.normals_host(host(), pts, k, md, N.default_cell(md))["normals"])


def test_normals_of_a_sphere_face_where_they_are_told():
    pts, centre, k, md = K.sphere_cloud()
    radial = (pts - centre).astype(np.float64)
    inward = to_numpy(fusion.estimate_normals(dev(pts), k, md, toward=dev(np.broadcast_to(centre, pts.shape))))
    outward_to = (centre + 100 * (pts - centre)).astype(np.float32)
    outward = to_numpy(fusion.estimate_normals(dev(pts), k, md, toward=dev(outward_to)))
    assert inward["valid"].all() and outward["valid"].all()
    assert ((inward["normals"] * radial).sum(1) < -0.9).all() and ((outward["normals"] * radial).sum(1) > 0.9).all()
    K.assert_bytes(inward["normals"], -outward["normals"])
    K.assert_bytes(outward["normals"], K.normals_host(host(), pts, k, md, N.default_cell(md), toward=outward_to)["normals"])


def test_normals_with_too_few_neighbours_an_exact_zero_and_a_line():
    pts, nbs = K.few_cloud()
    few = to_numpy(fusion.estimate_normals(dev(pts), 5, 1.0))
    assert few["valid"].tolist() == (nbs >= 2).tolist() and (few["normals"][:3] == 0).all()
    K.assert_bytes(few["normals"], K.normals_host(host(), pts, 5, 1.0, 0.25)["normals"])
    pts = K.cross_cloud()
    for tw, want in (((1, 0, 0), (0, 0, 1)), ((1, 0, -1), (0, 0, -1)), ((0, -3, 2), (0, 0, 1))):
        got = to_numpy(fusion.estimate_normals(dev(pts), 4, 1.25, toward=dev(np.tile(np.array(tw, np.float32), (5, 1)))))
        assert got["valid"].tolist() == [True] + [False] * 4 and got["normals"][0].tolist() == list(want), (tw, got["normals"][0])
    pts = K.line_cloud()                                                     # collinear: bit-equal to the host, nothing else is claimed
    for k in (2, 6):
        got = to_numpy(fusion.estimate_normals(dev(pts), k, 0.5))
        want = K.normals_host(host(), pts, k, 0.5, N.default_cell(0.5))
        assert got["valid"].all()
        K.assert_bytes(got["normals"], want["normals"], "line")


# ---- wiring ----------------------------------------------------------------------------------------------------------------------

def scene_result(sc, **kw):
    return fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], C.CONF_THRES, C.THRES_VIEW,
                             device=DEV, **kw)


def same_bytes(a, b, keys):
    for k in keys:
        if torch.is_tensor(a[k]):
            x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
        else:
            assert a[k] == b[k], k


def scene_scale(points):
    ok = points[torch.isfinite(points).all(1)]
    return float((ok.max(0)[0] - ok.min(0)[0]).max()) / 24


def camera_centres(sc):
    return np.stack([np.linalg.inv(np.asarray(sc["Es"][r], np.float64))[:3, 3] for r, _ in sc["pairs"]]).astype(np.float32)


@pytest.mark.parametrize("thin", (False, True))
def test_fuse_scene_keywords(thin):
    sc = C.hard_scene(61, 83, 5, "plain")
    base = scene_result(sc)
    md = scene_scale(base["points"])
    kw = dict(voxel_size=md / 3) if thin else {}
    plain = scene_result(sc, **kw)
    none = scene_result(sc, outliers=None, normals=None, **kw)
    assert list(none) == list(plain)
    same_bytes(none, plain, list(plain))
    pre = "thin_" if thin else ""
    pts, cols = plain[pre + "points"], plain[pre + "colors"]
    view = torch.repeat_interleave(torch.arange(len(sc["pairs"]), device=DEV), plain["counts"])
    if thin:
        view = view[plain["thin_first"]]
    centres = dev(camera_centres(sc))
    for outliers in (fusion.RadiusOutliers(md, 6), fusion.StatisticalOutliers(8, 1.0, 2 * md), None):
        got = scene_result(sc, outliers=outliers, normals=fusion.Normals(10, 2 * md), **kw)
        same_bytes(got, plain, list(plain))
        if isinstance(outliers, fusion.RadiusOutliers):
            f = fusion.radius_outliers(pts, md, 6, colors=cols)
            assert (got["final_radius"], got["final_nb_points"]) == (N.f32(md), 6)
        elif outliers is not None:
            f = fusion.statistical_outliers(pts, 8, 1.0, 2 * md, colors=cols)
            assert all(got["final_" + key] == f[key] for key in ("n", "mu", "sigma", "threshold")) and got["final_n"] > 100
        else:
            f = dict(points=pts, colors=cols, index=torch.arange(len(pts), device=DEV))
        same_bytes(dict(final_points=f["points"], final_colors=f["colors"], final_index=f["index"]), got,
                   ["final_points", "final_colors", "final_index"])
        nrm = fusion.estimate_normals(f["points"], 10, 2 * md, toward=centres[view[f["index"]]])
        same_bytes(dict(final_normals=nrm["normals"], final_normal_valid=nrm["valid"]), got, ["final_normals", "final_normal_valid"])
        n, ok = got["final_normals"][got["final_normal_valid"]], got["final_normal_valid"]
        to_cam = centres[view[f["index"]]][ok] - got["final_points"][ok]
        print("scene (thin %s, %s): %d -> %d points, %d normals" % (thin, type(outliers).__name__, len(pts), len(f["points"]), len(n)))
        assert 100 < len(f["points"]) <= len(pts) and len(n) > 100 and bool(((n.double() * to_cam.double()).sum(1) >= 0).all())
        if isinstance(outliers, fusion.StatisticalOutliers):                 # a ratio of 1: the upper tail goes
            assert len(f["points"]) < len(pts)
        # the filter alone: no normals in the result
        if outliers is not None:
            alone = scene_result(sc, outliers=outliers, **kw)
            assert "final_normals" not in alone
            same_bytes(alone, got, ["final_points", "final_colors", "final_index"])
        v = got.vertices(final=True)
        assert np.stack([v[c] for c in "xyz"], 1).tobytes() == got["final_points"].cpu().numpy().tobytes()
    with pytest.raises(RuntimeError, match="no cleaned cloud"):
        plain.vertices(final=True)


def test_filter_depth_writes_the_final_cloud(tmp_path):
    from PIL import Image
    sc = C.hard_scene(61, 83, 5, "plain")
    folder, out = tmp_path / "scan", tmp_path / "out"
    for d in (folder / "cams", folder / "images", out / "depth_est", out / "confidence"):
        os.makedirs(d)
    rng = np.random.RandomState(8)
    for v in range(5):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3] = sc["Es"][v], sc["Ks"][v], [425.0, 2.5, 192, 905.0]
        formats.write_cam(str(folder / "cams" / ("%08d_cam.txt" % v)), cam)
        Image.fromarray(rng.randint(0, 256, (61, 83, 3)).astype(np.uint8)).save(str(folder / "images" / ("%08d.jpg" % v)))
        formats.save_pfm(str(out / "depth_est" / ("%08d.pfm" % v)), sc["depths"][v])
        formats.save_pfm(str(out / "confidence" / ("%08d.pfm" % v)), sc["conf"][v])
    with open(folder / "pair.txt", "w") as f:
        f.write("%d\n" % len(sc["pairs"]))
        for r, srcs in sc["pairs"]:
            f.write("%d\n%d %s\n" % (r, len(srcs), " ".join("%d 1.0" % s for s in srcs)))
    args = (str(folder), str(folder), str(out))
    kw = dict(conf=C.CONF_THRES, thres_view=C.THRES_VIEW)
    full = fusion.filter_depth(*args, str(tmp_path / "full.ply"), **kw)
    xyz = np.stack([full[c] for c in "xyz"], 1)
    md = scene_scale(torch.from_numpy(xyz))
    assert fusion.read_ply(str(tmp_path / "full.ply")).tobytes() == full.tobytes()       # without the keywords: today's file
    # the filter alone: the old layout, fewer points (nb_points above the median count within md / 4: about half of them go)
    nb_points = int(np.median(to_numpy(fusion.radius_outliers(dev(xyz), md / 4, 1))["neighbours"])) + 1
    ply = str(tmp_path / "radius.ply")
    vertices = fusion.filter_depth(*args, ply, outliers=fusion.RadiusOutliers(md / 4, nb_points), **kw)
    want = to_numpy(fusion.radius_outliers(dev(xyz), md / 4, nb_points))
    print("filter_depth: %d points, %d with >= %d neighbours within %.4g" % (len(full), len(vertices), nb_points, md / 4))
    assert fusion.read_ply(ply).tobytes() == vertices.tobytes() and 100 < len(vertices) == len(want["index"]) < len(full)
    assert np.stack([vertices[c] for c in "xyz"], 1).tobytes() == want["points"].tobytes()
    assert vertices["red"].tobytes() == full["red"][want["index"]].tobytes()
    # with normals: x y z nx ny nz red green blue
    ply = str(tmp_path / "normals.ply")
    vertices = fusion.filter_depth(*args, ply, outliers=fusion.StatisticalOutliers(8, 1.0, 2 * md), normals=fusion.Normals(10, 2 * md),
                                   voxel_size=md / 3, **kw)
    data = open(ply, "rb").read()
    body = np.frombuffer(data[data.index(b"end_header\n") + 11:], dtype=fusion.PLY_NORMAL_VERTEX_DTYPE)
    assert b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in data and len(body) == len(vertices) > 100
    assert dtu_eval.read_ply_points(ply).tobytes() == np.stack([vertices[c] for c in "xyz"], 1).tobytes()
    lengths = np.linalg.norm(np.stack([body["nx"], body["ny"], body["nz"]], 1).astype(np.float64), axis=1)
    assert body["blue"].tobytes() == vertices["blue"].tobytes() and (np.abs(lengths[lengths > 0] - 1) < 1e-6).all() and (lengths > 0).sum() > 100


def test_reconstruct_scan_writes_the_final_cloud(shipped_cfg, checkpoint, tmp_path):
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
    md = scene_scale(plain["points"])
    spec = dict(outliers=fusion.StatisticalOutliers(6, 1.0, md), normals=fusion.Normals(8, md))
    got = scan.reconstruct_scan(*args, plyfilename=str(tmp_path / "final.ply"), **spec, **kw)
    same_bytes(got, plain, list(plain))
    f = fusion.statistical_outliers(plain["points"], 6, 1.0, md, colors=plain["colors"])
    same_bytes(dict(final_points=f["points"], final_colors=f["colors"], final_index=f["index"]), got,
               ["final_points", "final_colors", "final_index"])
    data = open(str(tmp_path / "final.ply"), "rb").read()
    body = np.frombuffer(data[data.index(b"end_header\n") + 11:], dtype=fusion.PLY_NORMAL_VERTEX_DTYPE)
    print("reconstruct_scan, Tanks-like: %d points -> %d, %d with a normal" % (len(plain["points"]), len(body),
                                                                              int(got["final_normal_valid"].sum())))
    assert 0 < len(body) == len(f["index"]) <= len(plain["points"])
    assert np.stack([body[c] for c in "xyz"], 1).tobytes() == got["final_points"].cpu().numpy().tobytes()
    assert np.stack([body[c] for c in ("nx", "ny", "nz")], 1).tobytes() == got["final_normals"].cpu().numpy().tobytes()
    assert fusion.read_ply(str(tmp_path / "full.ply")).tobytes() == plain.vertices().tobytes()
