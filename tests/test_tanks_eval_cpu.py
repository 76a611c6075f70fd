"""The Tanks and Temples evaluation protocol without a GPU: the host build of mvster_amd/csrc/reg_math.h
against the NumPy restatement (tests/tanks_eval_cases.py) byte for byte, the host pieces of mvster_amd.tanks_eval (umeyama, the
file readers, the argument checks), and the cases themselves."""
import json

import numpy as np
import pytest
import torch

from tests import tanks_eval_cases as T


@pytest.fixture(scope="module")
def hm():
    return T.load_reg_hostmath()


@pytest.mark.parametrize("name", sorted(T.crop_cases()))
def test_crop_of_the_host_build_is_the_restatement(hm, name):
    c = T.crop_cases()[name]
    T.assert_crop_same(T.crop_host(hm, c["points"], c["volume"], c["T"]), T.crop_numpy(c["points"], c["volume"], c["T"]), name)
    if c["T"] is not None:
        assert T.transform_host(hm, c["points"], c["T"]).tobytes() == T.moved_numpy(c["points"], c["T"]).tobytes(), name


def test_host_build_with_the_other_compiler_gives_the_same_bytes(hm):
    other = T.load_reg_hostmath(("clang++",))
    for name in ("gon1024_Y_t_n257", "sizes_t_n4099", "pentagon_rev_X_p_n257"):
        c = T.crop_cases()[name]
        T.assert_crop_same(T.crop_host(other, c["points"], c["volume"], c["T"]), T.crop_host(hm, c["points"], c["volume"], c["T"]), name)


def test_crop_rule_on_vertices_and_edges(hm):
    """The table of DESIGN.md section 4.19: the rule's values on the concave pentagon's vertices and edges, on every axis, from the
    restatement and from the host build."""
    for axis in "XYZ":
        vol, pts, want = T.pentagon_table_points(axis)
        assert T.inside_numpy(pts.astype(np.float64), vol).tolist() == want.tolist(), axis
        assert T.crop_host(hm, pts, vol)["flags"].astype(bool).tolist() == want.tolist(), axis
    # both ends of the extrusion are inside, the next double beyond either is not
    vol, pts, _ = T.pentagon_table_points("Z")
    q = np.array([[1, 1, -1.0], [1, 1, 1.0], [1, 1, np.nextafter(-1.0, -2)], [1, 1, np.nextafter(1.0, 2)], [1, 1, np.nan],
                  [np.inf, 1, 0], [1, -np.inf, 0]])
    assert T.inside_numpy(q, vol).tolist() == [True, True, False, False, False, False, False]


def test_crop_cases_are_what_they_claim():
    cases = T.crop_cases()
    for n in T.CROP_SIZES:
        assert len(cases["sizes_p_n%d" % n]["points"]) == n and len(cases["sizes_t_n%d" % n]["points"]) == n
    for axis in "XYZ":
        for poly, P in (("triangle", 3), ("pentagon", 5), ("pentagon_rev", 5), ("gon1024", 1024)):
            for t in "pt":
                c = cases["%s_%s_%s_n257" % (poly, axis, t)]
                assert c["volume"]["orthogonal_axis"] == axis and len(c["volume"]["polygon"]) == P
                flags = T.crop_numpy(c["points"], c["volume"], c["T"])["flags"]
                assert 20 < flags.sum() < 237, (poly, axis, t, int(flags.sum()))
                assert np.isnan(c["points"]).any() and np.isinf(c["points"]).any()
                assert not flags[~np.isfinite(c["points"]).all(1)].any()
    # the two orientations of the pentagon keep the same points
    for axis in "XYZ":
        a, b = cases["pentagon_%s_p_n257" % axis], cases["pentagon_rev_%s_p_n257" % axis]
        assert T.inside_numpy(a["points"].astype(np.float64), a["volume"]).tolist() == \
            T.inside_numpy(a["points"].astype(np.float64), b["volume"]).tolist()
    # without a transform the special points sit exactly on vertices, on edges and on the two ends
    c = cases["pentagon_Z_p_n257"]
    assert c["points"][0].tolist() == [0, 0, 0.375] and c["points"][1].tolist() == [2, 0, 0.375] and c["points"][3].tolist() == [4, 0, 0.375]
    assert c["points"][15:17, 2].tolist() == [-0.5, 1.25]                   # (3 points for each of the 5 vertices come first)
    flags = T.crop_numpy(c["points"], c["volume"])["flags"]
    assert flags[15] and flags[16] and not flags[17] and not flags[18]
    assert T.crop_numpy(cases["all_kept"]["points"], cases["all_kept"]["volume"])["flags"].all()
    assert not T.crop_numpy(cases["none_kept"]["points"], cases["none_kept"]["volume"])["flags"].any()


def test_crop_rule_agrees_with_the_winding_number_off_the_boundary():
    """An independent check of the even-odd rule: for points away from the boundary of the concave pentagon it is the winding
    number (the sum of the signed angles the edges subtend), in both orientations."""
    rng = np.random.default_rng(3)
    p = np.stack([rng.uniform(-1, 5, 20000), rng.uniform(-1, 4, 20000), np.zeros(20000)], 1)
    for poly in (T.PENTAGON, T.PENTAGON[::-1]):
        vol = T.volume("Z", poly, -1, 1)
        v = np.asarray(poly, np.float64)
        a, b = v[None] - p[:, None, :2], np.roll(v, -1, 0)[None] - p[:, None, :2]
        ang = np.arctan2(a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0], (a * b).sum(-1)).sum(1)
        wound = np.abs(ang) > np.pi
        near = np.abs(np.abs(ang) - np.pi) < 1.0                           # (close to the boundary the angle sum is not decisive)
        got = T.inside_numpy(p, vol)
        assert (~near).sum() > 15000 and (got == wound)[~near].all()


@pytest.mark.parametrize("Q", T.SUM_SIZES)
def test_terms_of_the_host_build_are_the_restatement(hm, Q):
    c = T.sums_case(Q)
    got = T.terms_host(hm, c["moved"], c["index"], c["dist2"], c["target"])
    assert got.tobytes() == c["terms"].tobytes(), Q


def test_sums_cases_are_what_they_claim():
    from mvster_amd import _lib
    lib = _lib.load()
    for Q in T.SUM_SIZES:
        c = T.sums_case(Q)
        n = int((c["index"] >= 0).sum())
        assert len(c["source"]) == Q and c["want"][0] == n and n >= 1, Q
        if Q >= 64:
            assert n < Q - 3 and np.isnan(c["dist2"]).sum() == 3 and np.isinf(c["dist2"]).sum() >= 1, Q
            assert (c["bound"] > 0).all(), Q
    assert lib.mvster_reg_sum_rows(T.SUM_SIZES[-1]) >= 4                     # several partial rows
    assert lib.mvster_reg_sum_rows(1000) == 1


@pytest.mark.parametrize("bins", (1, 499, 4096))
def test_histogram_of_the_host_build_is_numpy(hm, bins):
    d, edges = T.histogram_case(bins)
    want = np.histogram(d, edges)[0]
    assert T.histogram_host(hm, d, edges).tolist() == want.tolist()
    assert 0 < want.sum() < len(d) - 40 and np.isnan(d).sum() == 20 and (d == np.float32(edges[-1])).sum() >= 40
    assert (d.astype(np.float64)[:600, None] == edges[None]).any(1).sum() >= 1   # values equal to an edge


def test_umeyama_recovers_a_known_similarity():
    from mvster_amd import tanks_eval
    rng = np.random.default_rng(4)
    s = rng.normal(0, 1, (50, 3))
    for with_scaling, G in ((True, T.G), (False, T.G_RIGID), (True, T.CROP_T)):
        t = s @ G[:3, :3].T + G[:3, 3]
        U = tanks_eval.umeyama(tanks_eval.pair_sums(s, t), with_scaling)
        assert np.abs(U - G).max() < 1e-12
        assert np.abs(U - T.umeyama_pairs(s, t, with_scaling)).max() < 1e-12
    assert tanks_eval.umeyama(tanks_eval.pair_sums(s[:2], s[:2])) is None     # n < 3
    assert tanks_eval.umeyama(tanks_eval.pair_sums(np.ones((5, 3)), s[:5])) is None   # zero variance
    assert tanks_eval.umeyama(np.zeros(18)) is None
    with pytest.raises(RuntimeError, match="umeyama: sums"):
        tanks_eval.umeyama(np.zeros(17))


def test_umeyama_on_a_plane_takes_the_reflection_branch():
    """All z = 0: the covariance has rank two, the SVD's third vectors are free in sign, and only S = diag(1, 1, -1) turns the
    reflection it may return into the rotation."""
    from mvster_amd import tanks_eval
    rng = np.random.default_rng(5)
    s = np.concatenate([rng.normal(0, 1, (40, 2)), np.zeros((40, 1))], 1)
    seen = set()
    for deg in (10.0, 100.0, 170.0, 200.0, 275.0, 350.0):
        for axis in ((0, 0, 1), (1, 0, 0), (0.3, -0.5, 0.81)):
            G = T.similarity(axis, deg, 0.7, (1.0, -2.0, 0.5))
            t = s @ G[:3, :3].T + G[:3, 3]
            sums = tanks_eval.pair_sums(s, t)
            U = tanks_eval.umeyama(sums)
            assert np.linalg.det(U[:3, :3]) > 0 and np.abs(U - G).max() < 1e-12, (deg, axis)
            Us, _, Vt = np.linalg.svd(sums[9:18].reshape(3, 3) / 40 - np.outer(sums[5:8] / 40, sums[2:5] / 40))
            seen.add(bool(np.linalg.det(Us) * np.linalg.det(Vt) < 0))
    assert seen == {True, False}                                            # both branches were taken


def test_icp_case_stops_with_a_margin():
    """The restatement on the fixed case: converged with fitness 1, at an iteration where the rmse change clears relative_rmse by
    100 x on both sides -- only then may the GPU's iteration count be held to it."""
    pts, half = T.surface_cloud()
    d = pts[:, None, :].astype(np.float64) - pts[None].astype(np.float64)
    d2 = (d * d).sum(-1)
    d2[np.arange(len(pts)), np.arange(len(pts))] = np.inf
    assert 3000 < len(pts) < 6000 and d2.min() >= 0.012 ** 2 and len(half) == len(pts) // 2
    for rigid in (False, True):
        c = T.icp_case(rigid)
        r = c["restated"]
        assert r["converged"] and r["fitness"] == 1.0 and 5 <= r["iterations"] <= 15
        assert T.stop_margin(r["history"]), [h.get("d_rmse") for h in r["history"]]
        steps = r["history"][1:]
        assert steps[-1]["d_rmse"] < 1e-8 and steps[-2]["d_rmse"] > 1e-4
        assert 2e-8 < c["error"] < 2e-7 and c["tolerance"] == 4 * c["error"]   # float32 rounding of coordinates near 1
        assert np.abs(r["transformation"] - c["G"]).max() < 1e-8
    far = T.icp_numpy(T.icp_case()["source"] + np.float32(10), pts, T.ICP_MAX_DIST)
    assert far["iterations"] == 0 and not far["converged"] and far["fitness"] == 0 and (far["transformation"] == np.eye(4)).all()


def test_protocol_case_has_no_count_near_tau():
    p = T.protocol_case()
    r = p["restated"]
    assert r["precision"] == 1.0 and r["pred_valid"] == r["pred_below_tau"] > 1500
    assert 0.45 < r["recall"] < 0.55 and r["gt_valid"] == r["gt_thinned"] == r["gt_cropped"]
    gd, pd = r["gt_dist"].astype(np.float64), r["pred_dist"].astype(np.float64)
    assert not ((gd > T.ICP_TAU / 8) & (gd < 2 * T.ICP_TAU)).any() and (pd < T.ICP_TAU / 8).all()
    assert np.abs(r["transformation"] - p["G"]).max() < 1e-8
    assert len(r["rounds"]) == 3 and all(rd["converged"] and rd["fitness"] == 1.0 for rd in r["rounds"])
    assert len(r["edges"]) == 500 and r["cum_source"][-1] == 1.0 and r["recall"] <= r["cum_target"][-1] <= 1.0


@pytest.mark.parametrize("premoved", (False, True))
def test_lattice_case_counts(premoved):
    c = T.lattice_case(0.01, premoved)
    r = T.evaluate_numpy(c["pred"], c["truth"], c["init_trans"], refine=False)
    assert (r["pred_below_tau"], r["pred_valid"]) == c["precision"] and (r["gt_below_tau"], r["gt_valid"]) == c["recall"]
    assert c["recall"][1] == 30 * 31 and c["precision"][0] < c["precision"][1] < c["recall"][1]


def test_file_readers(tmp_path):
    from mvster_amd import dtu_eval, tanks_eval
    c = T.lattice_case(0.005)
    folder = str(tmp_path / "Truck")
    T.write_scene_files(folder, "Truck", c["truth"], T.G)
    vol = tanks_eval.read_crop_volume(folder + "/Truck.json")
    assert vol.orthogonal_axis == "Z" and (vol.axis_min, vol.axis_max) == (c["truth"]["volume"]["axis_min"], c["truth"]["volume"]["axis_max"])
    assert vol.polygon.dtype == np.float64 and vol.polygon.tobytes() == c["truth"]["volume"]["polygon"].tobytes()
    assert tanks_eval.read_transform(folder + "/Truck_trans.txt").tobytes() == T.G.tobytes()
    assert dtu_eval.read_ply_points(folder + "/Truck.ply").tobytes() == c["truth"]["gt_points"].tobytes()
    T.write_ply_xyz(str(tmp_path / "d.ply"), c["truth"]["gt_points"].astype(np.float64), "double")
    assert dtu_eval.read_ply_points(str(tmp_path / "d.ply")).tobytes() == c["truth"]["gt_points"].tobytes()
    with open(folder + "/bad.json", "w") as f:
        json.dump(dict(axis_min=0, axis_max=1, orthogonal_axis="Z"), f)
    with pytest.raises(RuntimeError, match="read_crop_volume: .* has no 'bounding_polygon'"):
        tanks_eval.read_crop_volume(folder + "/bad.json")
    with pytest.raises(RuntimeError, match="TanksSceneTruth.from_files: .*Barn.ply does not exist"):
        tanks_eval.TanksSceneTruth.from_files(str(tmp_path), "Barn")
    with pytest.raises(RuntimeError, match="no tau is known for scene 'Shed'"):
        tanks_eval.TanksSceneTruth.from_files(str(tmp_path), "Shed")
    assert tanks_eval.SCENE_TAU == dict(Barn=0.01, Caterpillar=0.005, Church=0.025, Courthouse=0.025, Ignatius=0.003,
                                        Meetingroom=0.01, Truck=0.005)


def test_trajectory_log_and_transform(tmp_path):
    from mvster_amd import tanks_eval
    rng = np.random.default_rng(6)
    poses = np.stack([T.similarity(rng.normal(0, 1, 3), rng.uniform(0, 360), 1.0, rng.normal(0, 2, 3)) for _ in range(12)])
    S = T.similarity((0.1, 0.9, -0.3), 40.0, 2.5, (3.0, -1.0, 0.5))
    moved = np.stack([S @ P for P in poses])
    moved[:, :3, :3] /= 2.5
    a, b = str(tmp_path / "est.log"), str(tmp_path / "colmap.log")
    T.write_trajectory_log(a, poses)
    T.write_trajectory_log(b, moved)
    meta, got = tanks_eval.read_trajectory_log(a)
    assert meta.tolist() == [[k, k, 0] for k in range(12)] and got.tobytes() == poses.tobytes()
    assert np.abs(tanks_eval.trajectory_transform(a, b) - S).max() < 1e-12
    assert np.abs(tanks_eval.trajectory_transform(poses, moved, T.G) - T.G @ S).max() < 1e-12
    with open(a, "a") as f:
        f.write("1 2 3\n")
    with pytest.raises(RuntimeError, match="read_trajectory_log: .* 5 lines per camera"):
        tanks_eval.read_trajectory_log(a)
    with pytest.raises(RuntimeError, match="trajectory_transform: the two trajectories"):
        tanks_eval.trajectory_transform(poses, moved[:5])
    with pytest.raises(RuntimeError, match="do not determine a similarity"):
        tanks_eval.trajectory_transform(poses[:2], moved[:2])


def _vol(P=5, axis="Z", **kw):
    from mvster_amd import tanks_eval
    th = 2 * np.pi * np.arange(P) / max(P, 1)
    d = dict(orthogonal_axis=axis, axis_min=-1.0, axis_max=1.0, polygon=np.stack([np.cos(th), np.sin(th), 0 * th], 1))
    d.update(kw)
    return tanks_eval.CropVolume(**d)


def test_bad_arguments_are_rejected_by_name():
    from mvster_amd import tanks_eval as E
    pts = torch.zeros(5, 3)
    for P in (2, 1025, 0):
        with pytest.raises(RuntimeError, match="crop_points: volume.polygon must have 3 .. 1024 vertices, not %d" % P):
            E.crop_points(pts, _vol(P))
    with pytest.raises(RuntimeError, match="volume.orthogonal_axis must be 'X', 'Y' or 'Z'"):
        E.crop_points(pts, _vol(axis="W"))
    with pytest.raises(RuntimeError, match="crop_points: volume.polygon, axis_min and axis_max must be finite"):
        E.crop_points(pts, _vol(axis_min=float("nan")))
    with pytest.raises(RuntimeError, match="volume.polygon must be \\[P,3\\]"):
        E.crop_points(pts, _vol(polygon=np.zeros((5, 2))))
    with pytest.raises(RuntimeError, match="volume must be a CropVolume"):
        E.crop_points(pts, dict())
    for bad in (np.eye(3), np.full((4, 4), np.nan), np.ones((4, 4)), "x"):
        with pytest.raises(RuntimeError, match="crop_points: transform must be"):
            E.crop_points(pts, _vol(), transform=bad)
    with pytest.raises(RuntimeError, match="transform_points: transform must be a 4 x 4 matrix, not None"):
        E.transform_points(pts, None)
    with pytest.raises(RuntimeError, match="crop_points: points must be \\[M,3\\] float32"):
        E.crop_points(pts.double(), _vol())
    with pytest.raises(RuntimeError, match="crop_points: points must be a torch tensor"):
        E.crop_points(np.zeros((5, 3), np.float32), _vol())
    for tau in (float("nan"), float("inf"), 0, -1, "x"):
        with pytest.raises(RuntimeError, match="TanksSceneTruth: tau"):
            E.TanksSceneTruth(pts, _vol(), tau)
    with pytest.raises(RuntimeError, match="TanksSceneTruth: gt_trans must be"):
        E.TanksSceneTruth(pts, _vol(), 0.01, gt_trans=np.eye(3))
    for md in (0, float("nan"), -1):
        with pytest.raises(RuntimeError, match="register_clouds: max_dist"):
            E.register_clouds(pts, pts, md)
        with pytest.raises(RuntimeError, match="registration_sums: max_dist"):
            E.registration_sums(pts, pts, md)
    with pytest.raises(RuntimeError, match="register_clouds: relative_rmse"):
        E.register_clouds(pts, pts, 0.1, relative_rmse=-1)
    with pytest.raises(RuntimeError, match="register_clouds: max_iteration"):
        E.register_clouds(pts, pts, 0.1, max_iteration=1.5)
    with pytest.raises(RuntimeError, match="register_clouds: init must be"):
        E.register_clouds(pts, pts, 0.1, init=np.zeros((4, 4)))
    with pytest.raises(RuntimeError, match="register_clouds: cell must be >= max_dist / 15"):
        E.register_clouds(pts, pts, 0.1, cell=0.001)
    for edges in ([0.0], np.arange(4098.0), [0, 2, 1], [0, np.nan], "x"):
        with pytest.raises(RuntimeError, match="distance_histogram: edges"):
            E.distance_histogram(torch.zeros(5), edges)
    with pytest.raises(RuntimeError, match="distance_histogram: dist must be a \\[N\\] float32"):
        E.distance_histogram(torch.zeros(5, 1), [0, 1])
    with pytest.raises(RuntimeError, match="evaluate_scene: truth must be a TanksSceneTruth"):
        E.evaluate_scene(pts, None)
    with pytest.raises(RuntimeError, match="evaluate_tanks: .*Barn.ply does not exist"):
        E.evaluate_tanks("/nonexistent", "/nonexistent", scenes=("Barn",))


def test_cpu_tensors_are_refused():
    from mvster_amd import tanks_eval as E
    pts = torch.zeros(5, 3)
    for what, call in (("crop_points", lambda: E.crop_points(pts, _vol())),
                       ("transform_points", lambda: E.transform_points(pts, np.eye(4))),
                       ("registration_sums", lambda: E.registration_sums(pts, pts, 0.1)),
                       ("register_clouds", lambda: E.register_clouds(pts, pts, 0.1)),
                       ("distance_histogram", lambda: E.distance_histogram(torch.zeros(5), [0, 1])),
                       ("TanksSceneTruth", lambda: E.TanksSceneTruth(pts, _vol(), 0.01))):
        with pytest.raises(RuntimeError, match=r"tanks_eval\.%s runs on MI355X only.*no CPU fallback" % what):
            call()


def test_library_rejects_bad_sizes_before_any_launch():
    """The entry points of geo_reg.hip validate before the first HIP call (stand-in addresses: nothing is dereferenced)."""
    from mvster_amd import _lib
    lib = _lib.load()
    a = 1 << 32
    S, Nl = _lib.ERR_SHAPE, _lib.ERR_NULL
    big = (1 << 29) + 1
    assert lib.mvster_reg_blocks(0) == S and lib.mvster_reg_blocks(big) == S and lib.mvster_reg_blocks(257) == 2
    assert lib.mvster_reg_transform(a, 5, None, a, None) == Nl and lib.mvster_reg_transform(a, 0, a, a, None) == S
    for P in (2, 1025, -1):
        assert lib.mvster_reg_crop_flags(a, 5, None, a, P, 2, 0, a, a, a, None) == S
    for axis in (-1, 3):
        assert lib.mvster_reg_crop_flags(a, 5, None, a, 5, axis, 0, a, a, a, None) == S
    assert lib.mvster_reg_crop_flags(a, 0, None, a, 5, 2, 0, a, a, a, None) == S
    assert lib.mvster_reg_crop_flags(a, big, None, a, 5, 2, 0, a, a, a, None) == S
    assert lib.mvster_reg_crop_flags(a, 5, None, a, 5, 2, 4096, a, a, a, None) == S
    assert lib.mvster_reg_crop_flags(a, 5, None, None, 5, 2, 0, a, a, a, None) == Nl
    assert lib.mvster_reg_crop_emit(a, None, 5, None, a, a, 6, 0, a, None, a, None) == S
    assert lib.mvster_reg_crop_emit(a, None, 5, None, a, a, -1, 0, a, None, a, None) == S
    assert lib.mvster_reg_crop_emit(a, None, 5, None, a, a, 0, 0, None, None, None, None) == 0    # nothing kept: no launch
    assert lib.mvster_reg_crop_emit(a, a, 5, None, a, a, 2, 0, a, None, a, None) == Nl
    assert lib.mvster_reg_sum_rows(0) == S and lib.mvster_reg_sum_rows(big) == S
    assert lib.mvster_reg_sums(a, a, a, 0, a, 5, a, a, None) == S and lib.mvster_reg_sums(a, a, a, 5, None, 5, a, a, None) == S
    assert lib.mvster_reg_sums(a, a, a, 5, a, 5, None, a, None) == Nl
    for bins in (0, 4097):
        assert lib.mvster_reg_histogram(a, 5, a, bins, a, None) == S
    assert lib.mvster_reg_histogram(a, 0, a, 5, a, None) == S and lib.mvster_reg_histogram(a, 5, None, 5, a, None) == Nl
