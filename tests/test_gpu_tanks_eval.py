"""The Tanks and Temples evaluation protocol on the GPU: mvster_amd.tanks_eval against the host build of
mvster_amd/csrc/reg_math.h (byte for byte) and the NumPy restatement of the protocol (tests/tanks_eval_cases.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cloud_nn_cases as N
from tests import tanks_eval_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gpu(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def crop_volume(vol):
    from mvster_amd import tanks_eval
    return tanks_eval.CropVolume(vol["orthogonal_axis"], vol["axis_min"], vol["axis_max"], vol["polygon"])


def truth_of(t):
    from mvster_amd import tanks_eval
    return tanks_eval.TanksSceneTruth(gpu(t["gt_points"]), crop_volume(t["volume"]), t["tau"], t["gt_trans"])


def run_crop(c, **kw):
    from mvster_amd import tanks_eval
    got = tanks_eval.crop_points(gpu(c["points"]), crop_volume(c["volume"]), transform=c["T"], **kw)
    assert got["kept"] == got["points"].shape[0] == got["index"].shape[0]
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}


# ---- crop and transform -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(T.crop_cases()))
def test_crop_points_is_the_host_build(name):
    c = T.crop_cases()[name]
    want = T.crop_host(T.load_reg_hostmath(), c["points"], c["volume"], c["T"])
    got = run_crop(c)
    T.assert_crop_same(got, want, name)
    T.assert_crop_same(run_crop(c), got, name + " (second run)")
    T.assert_crop_same(run_crop(c, _max_grid=3), want, name + " (three workgroups: every one strides over the tiles)")
    if name == "none_kept":
        assert got["kept"] == 0 and got["points"].shape == (0, 3) and got["index"].shape == (0,)
    if name == "all_kept":
        assert got["kept"] == len(c["points"]) and got["points"].tobytes() == c["points"].tobytes()


def test_crop_points_carries_colors_and_transform_points_is_the_host_build():
    from mvster_amd import tanks_eval
    c = T.crop_cases()["sizes_t_n4099"]
    colors = np.random.default_rng(8).integers(0, 256, (4099, 3)).astype(np.uint8)
    got = tanks_eval.crop_points(gpu(c["points"]), crop_volume(c["volume"]), transform=c["T"], colors=gpu(colors))
    index = got["index"].cpu().numpy()
    assert 0 < len(index) < 4099 and got["colors"].cpu().numpy().tobytes() == colors[index].tobytes()
    moved = tanks_eval.transform_points(gpu(c["points"]), c["T"]).cpu().numpy()
    assert moved.tobytes() == T.transform_host(T.load_reg_hostmath(), c["points"], c["T"]).tobytes()
    assert got["points"].cpu().numpy().tobytes() == moved[index].tobytes()
    assert tanks_eval.transform_points(gpu(np.zeros((0, 3), np.float32)), c["T"]).shape == (0, 3)
    empty = tanks_eval.crop_points(gpu(np.zeros((0, 3), np.float32)), crop_volume(c["volume"]))
    assert empty["kept"] == 0 and empty["points"].shape == (0, 3) and empty["flags"].shape == (0,)


def test_crop_rule_on_vertices_and_edges():
    for axis in "XYZ":
        vol, pts, want = T.pentagon_table_points(axis)
        got = run_crop(dict(points=pts, volume=vol, T=None))
        assert got["flags"].astype(bool).tolist() == want.tolist(), axis


# ---- correspondence sums ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Q", T.SUM_SIZES)
def test_registration_sums_against_fsum(Q):
    from mvster_amd import fusion, tanks_eval
    c = T.sums_case(Q)
    grid = fusion.CloudGrid(gpu(c["target"]), T.smallest_cell(T.SUM_MAX_DIST))
    src = gpu(c["source"])
    got = tanks_eval.registration_sums(src, grid, T.SUM_MAX_DIST, transform=T.SUM_T)
    assert got.dtype == np.float64 and got.shape == (18,)
    # the correspondences are brute force's: the moved cloud, every index and every d2
    moved = tanks_eval.transform_points(src, T.SUM_T)
    assert moved.cpu().numpy().tobytes() == c["moved"].tobytes()
    near = fusion.nearest_distances(moved, grid, T.SUM_MAX_DIST)
    assert near["index"].cpu().numpy().tobytes() == c["index"].tobytes() and near["dist2"].cpu().numpy().tobytes() == c["dist2"].tobytes()
    assert got[0] == c["want"][0]                                            # n, exactly
    err = np.abs(got - c["want"])
    print("Q = %d: n = %d, |sum - fsum| / bound = %s" % (Q, int(got[0]), np.array2string(err / c["bound"], precision=3)))
    assert (err <= c["bound"]).all(), [(T.SUM_NAMES[j], err[j], c["bound"][j]) for j in np.nonzero(err > c["bound"])[0]]
    again = tanks_eval.registration_sums(src, grid, T.SUM_MAX_DIST, transform=T.SUM_T)
    assert again.tobytes() == got.tobytes()
    # the target as a tensor, binned inside the call: the same bytes
    assert tanks_eval.registration_sums(src, gpu(c["target"]), T.SUM_MAX_DIST, transform=T.SUM_T).tobytes() == got.tobytes()


def test_registration_sums_without_a_candidate_are_zero():
    from mvster_amd import tanks_eval
    c = T.sums_case(1000)
    far = gpu(c["moved"] + np.float32(10))
    for target in (gpu(c["target"]), gpu(np.zeros((0, 3), np.float32))):
        got = tanks_eval.registration_sums(far, target, T.SUM_MAX_DIST)
        assert got.tobytes() == np.zeros(18).tobytes()
    assert tanks_eval.registration_sums(gpu(np.zeros((0, 3), np.float32)), gpu(c["target"]), T.SUM_MAX_DIST).tobytes() == np.zeros(18).tobytes()


def test_grid_of_the_wrong_cell_is_refused():
    from mvster_amd import fusion, tanks_eval
    c = T.sums_case(64)
    src = gpu(c["source"])
    small = fusion.CloudGrid(gpu(c["target"]), 0.001)
    with pytest.raises(RuntimeError, match="registration_sums: cell must be >= max_dist / 15"):
        tanks_eval.registration_sums(src, small, T.SUM_MAX_DIST)
    with pytest.raises(RuntimeError, match="register_clouds: cell must be >= max_dist / 15"):
        tanks_eval.register_clouds(src, small, T.SUM_MAX_DIST)
    grid = fusion.CloudGrid(gpu(c["target"]), 0.02)
    with pytest.raises(RuntimeError, match="register_clouds: the CloudGrid given as target has cell"):
        tanks_eval.register_clouds(src, grid, T.SUM_MAX_DIST, cell=0.01)


# ---- histogram --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", (1, 499, 4096))
def test_distance_histogram_is_numpy(bins):
    from mvster_amd import tanks_eval
    d, edges = T.histogram_case(bins)
    got = tanks_eval.distance_histogram(gpu(d), edges)
    assert got.dtype == np.int64 and got.tolist() == np.histogram(d, edges)[0].tolist()
    assert tanks_eval.distance_histogram(gpu(np.zeros(0, np.float32)), edges).tolist() == [0] * bins


# ---- ICP -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rigid", (False, True))
def test_register_clouds_on_the_surface_case(rigid):
    """Tolerance: 4 x the restatement's own largest point error on this case (float32 rounding of the coordinates; about 8e-8
    here), computed in tests/tanks_eval_cases.py from the restatement alone."""
    from mvster_amd import fusion, tanks_eval
    c = T.icp_case(rigid)
    r = c["restated"]
    got = tanks_eval.register_clouds(gpu(c["source"]), gpu(c["target"]), T.ICP_MAX_DIST, with_scaling=not rigid)
    err = T.point_error(got["transformation"], c["source"], c["target"][c["partner"]])
    print("rigid = %s: iterations %d (restated %d), largest point error %.3e (restated %.3e, tolerance %.3e)" %
          (rigid, got["iterations"], r["iterations"], err, c["error"], c["tolerance"]))
    assert got["converged"] and got["fitness"] == 1.0 and got["correspondences"] == len(c["source"])
    assert err <= c["tolerance"]
    assert T.stop_margin(r["history"]) and got["iterations"] == r["iterations"]    # (the CPU test holds the margin)
    assert len(got["history"]) == got["iterations"] + 1
    for h, w in zip(got["history"], r["history"]):
        assert h["fitness"] == w["fitness"] and abs(h["inlier_rmse"] - w["inlier_rmse"]) <= c["tolerance"]
    if rigid:
        R = got["transformation"][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    # the target as a grid built once gives the same transformation, bit for bit
    grid = fusion.CloudGrid(gpu(c["target"]), T.smallest_cell(T.ICP_MAX_DIST))
    again = tanks_eval.register_clouds(gpu(c["source"]), grid, T.ICP_MAX_DIST, with_scaling=not rigid)
    assert again["transformation"].tobytes() == got["transformation"].tobytes() and again["iterations"] == got["iterations"]


def test_register_clouds_far_away_returns_init():
    from mvster_amd import tanks_eval
    c = T.icp_case()
    init = T.similarity((0, 0, 1), 3.0, 1.0, (0.0, 0.0, 10.0))
    got = tanks_eval.register_clouds(gpu(c["source"]), gpu(c["target"]), T.ICP_MAX_DIST, init=init)
    assert got["transformation"].tobytes() == init.tobytes()
    assert got["fitness"] == 0 and got["inlier_rmse"] == 0 and got["iterations"] == 0 and got["converged"] is False
    assert got["history"] == [dict(fitness=0.0, inlier_rmse=0.0)]
    none = tanks_eval.register_clouds(gpu(c["source"]), gpu(c["target"]), T.ICP_MAX_DIST, max_iteration=0)
    assert none["iterations"] == 0 and none["converged"] is False and (none["transformation"] == np.eye(4)).all()


# ---- the protocol ----------------------------------------------------------------------------------------------------------------------------

def test_evaluate_scene_with_refinement():
    """The surface case through the three ICP rounds: the restatement's integers (precision exactly 1, recall with no count
    near tau) and its transformation."""
    from mvster_amd import tanks_eval
    p = T.protocol_case()
    want = p["restated"]
    truth = truth_of(p["truth"])
    got = tanks_eval.evaluate_scene(gpu(p["pred"]), truth)
    err, werr = np.abs(got["transformation"] - p["G"]).max(), np.abs(want["transformation"] - p["G"]).max()
    print("transformation error %.3e (restated %.3e); rounds %s (restated %s)" %
          (err, werr, [r["iterations"] for r in got["rounds"]], [r["iterations"] for r in want["rounds"]]))
    for k in ("pred_valid", "pred_within", "pred_below_tau", "gt_valid", "gt_within", "gt_below_tau", "pred_thinned", "gt_thinned", "gt_cropped"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["precision"] == 1.0 and got["recall"] == want["recall"] and got["fscore"] == want["fscore"]
    assert err <= T.ICP_TOLERANCE_FACTOR * werr
    assert len(got["rounds"]) == 3
    for g, w in zip(got["rounds"], want["rounds"]):
        assert g["converged"] and g["fitness"] == 1.0 and g["source_points"] == w["source_points"] and g["target_points"] == w["target_points"]
        if T.stop_margin(w["history"]):                                      # (round 1 stops marginally: its outcome, not its count)
            assert g["iterations"] == w["iterations"]
    assert got["edges"].tobytes() == want["edges"].tobytes()
    assert np.abs(got["cum_source"] - want["cum_source"]).max() <= 2.0 / want["pred_thinned"]    # (distances of 1e-8 beside the first edges)
    assert got["recall"] <= got["cum_target"][-1] <= 1.0 and got["cum_source"][-1] == 1.0
    # the truth's grids were made once: a second evaluation gives the same result
    again = tanks_eval.evaluate_scene(gpu(p["pred"]), truth)
    assert again["transformation"].tobytes() == got["transformation"].tobytes() and again["recall"] == got["recall"]


@pytest.mark.parametrize("premoved", (False, True))
def test_evaluate_scene_counts_known_in_advance(premoved):
    from mvster_amd import tanks_eval
    c = T.lattice_case(0.01, premoved)
    got = tanks_eval.evaluate_scene(gpu(c["pred"]), truth_of(c["truth"]), init_trans=c["init_trans"], refine=False)
    assert (got["pred_below_tau"], got["pred_valid"]) == c["precision"] and (got["gt_below_tau"], got["gt_valid"]) == c["recall"]
    P, R = c["precision"][0] / c["precision"][1], c["recall"][0] / c["recall"][1]
    assert got["precision"] == P and got["recall"] == R and got["fscore"] == 2 * P * R / (P + R)
    assert got["rounds"] == [] and got["cum_source"][-1] == 1.0 and R < got["cum_target"][-1] < 1.0   # (3 tau is on the curve)
    want = T.evaluate_numpy(c["pred"], c["truth"], c["init_trans"], refine=False)
    if not premoved:                                                         # (distances of exactly 0.2 tau and 3 tau: the same bins)
        assert got["cum_source"].tobytes() == want["cum_source"].tobytes() and got["cum_target"].tobytes() == want["cum_target"].tobytes()


def test_evaluate_tanks_on_a_folder_of_two_scenes(tmp_path):
    from mvster_amd import tanks_eval
    data, plys, out = str(tmp_path / "data"), str(tmp_path / "plys"), str(tmp_path / "out")
    os.makedirs(plys)
    cases = {}
    for scene in ("Barn", "Truck"):
        c = cases[scene] = T.lattice_case(tanks_eval.SCENE_TAU[scene], premoved=True)
        T.write_scene_files(os.path.join(data, scene), scene, c["truth"], c["init_trans"])
        T.write_ply_xyz(os.path.join(plys, scene + ".ply"), c["pred"])
    got = tanks_eval.evaluate_tanks(plys, data, scenes=("Barn", "Truck"), out_dir=out, device=DEV, refine=False)
    f = []
    for row, scene in zip(got["rows"], ("Barn", "Truck")):
        c = cases[scene]
        assert row["scene"] == scene and row["tau"] == N.f32(tanks_eval.SCENE_TAU[scene])
        assert (row["pred_below_tau"], row["pred_valid"]) == c["precision"] and (row["gt_below_tau"], row["gt_valid"]) == c["recall"]
        f.append(row["fscore"])
    assert got["mean_fscore"] == float(np.mean(f))
    with open(os.path.join(out, "tanks_eval.json")) as fh:
        back = json.load(fh)
    assert back["mean_fscore"] == got["mean_fscore"] and [r["scene"] for r in back["rows"]] == ["Barn", "Truck"]
    assert back["rows"][0]["transformation"] == got["rows"][0]["transformation"].tolist()
