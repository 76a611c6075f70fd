"""The DTU evaluation protocol without a GPU: the host build of mvster_amd/csrc/eval_math.h against
the NumPy restatement of the .m files on every case, the cases themselves, the file readers, and the argument checks of
mvster_amd.dtu_eval."""
import os

import numpy as np
import pytest
import torch

from tests import dtu_eval_cases as E


@pytest.fixture(scope="module")
def hm():
    return E.load_eval_hostmath()


# ---- the point reduction ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.REDUCE_NAMES)
def test_serial_loop_of_the_host_build_is_the_restatement(hm, name):
    c = E.reduce_cases()[name]
    keep, dropped = E.reduce_expected(name)
    want, want_dropped = E.reduce_numpy(c["points"], c["dst"], c["priority"], c["seed"])
    assert dropped == want_dropped
    assert keep.tobytes() == want.tobytes(), (name, int(keep.sum()), int(want.sum()))


@pytest.mark.parametrize("factor", (2, 1))
@pytest.mark.parametrize("name", E.REDUCE_NAMES)
def test_round_iteration_reaches_the_serial_loop(hm, name, factor):
    """The rounds of geo_eval.hip in their host form (3 x 3 x 3 cells of edge 2 dst, or 5 x 5 x 5 of edge dst; double-buffered
    states) leave the serial loop's set, so both search bounds and the rounds hold on every case."""
    c = E.reduce_cases()[name]
    keep, rounds = E.reduce_host(hm, c["points"], c["dst"], c["priority"], c["seed"], rounds=factor)
    assert rounds >= 0, "a round decided nothing"
    assert keep.tobytes() == E.reduce_expected(name)[0].tobytes(), name
    if name == "line_arange":
        assert rounds == 300                               # every point waits for the one before it
    if name.startswith("surface") and name != "surface_16keys":
        assert rounds <= 20, rounds                        # hashed or permuted priorities: a shallow dependency chain


def test_splitmix64_and_mround(hm):
    idx = np.array([0, 1, 2, 12345, 2 ** 31, 2 ** 40 + 17], np.uint64)
    for seed in (0, 1, 7, 2 ** 62 + 5):
        want = E.splitmix64_numpy(idx, seed)
        assert [hm.hm_eval_splitmix64(int(i), seed) for i in idx] == [int(w) for w in want]
    # splitmix64's published first outputs for the state 0: the hash of i = 0 under seed 0 is the generator's first value
    assert hm.hm_eval_splitmix64(0, 0) == 0xE220A8397B1DCDAF
    below_half = np.nextafter(0.5, 0.0)
    for x, want in ((0.5, 1.0), (-0.5, -1.0), (below_half, 0.0), (-below_half, -0.0), (1.5, 2.0), (2.5, 3.0), (-2.5, -3.0), (2.4999, 2.0),
                    (0.0, 0.0), (2.0 ** 52 + 1, 2.0 ** 52 + 1), (2.0 ** 51 + 0.5, 2.0 ** 51 + 1), (1e300, 1e300), (-7.0, -7.0)):
        assert hm.hm_eval_mround(x) == want and E.mround_numpy(x) == want, x
    assert np.isnan(hm.hm_eval_mround(float("nan")))


def test_reduction_cases_are_what_they_claim():
    kept = lambda name: E.reduce_expected(name)[0]
    assert np.array_equal(np.nonzero(kept("line_arange"))[0], np.arange(0, 300, 2))
    n = int(kept("line_hash").sum())
    assert 100 <= n < 150, n                                 # between every third and every second point
    assert kept("pair_at").tolist() == [True, False] and kept("pair_below").tolist() == [True, True]
    assert kept("chain").tolist() == [True, False, True]     # the dropped B suppresses nobody
    assert np.nonzero(kept("duplicates"))[0].tolist() == [1]
    first = int(np.lexsort((np.arange(5000), E.splitmix64_numpy(np.arange(5000), 0)))[0])
    assert np.nonzero(kept("ball"))[0].tolist() == [first]
    assert kept("ball_and_more")[:5000].sum() == 1 and kept("ball_and_more")[5000:].sum() > 10
    keep, dropped = E.reduce_expected("invalid")
    bad = ~E.N.valid_points(E.reduce_cases()["invalid"]["points"], E.DST)
    assert dropped == bad.sum() > 40 and not keep[bad].any()
    assert E.reduce_expected("all_invalid")[1] == 70 and not kept("all_invalid").any()
    assert kept("m0").shape == (0,) and kept("m1").tolist() == [True] and kept("m2").tolist() in ([True, False], [False, True])
    for name in ("surface_seed0", "surface_seed7", "surface_perm", "surface_16keys"):
        factor = 20000 / kept(name).sum()
        assert 5 < factor < 9, (name, factor)
    assert kept("surface_seed0").tobytes() != kept("surface_seed7").tobytes()
    # (e): the pairs at 0.99 dst lose one point, the pairs at 1.01 dst none -- on the cells of edge dst and of edge 2 dst
    nb = E.reduce_cases()["neighbours"]["points"]
    k = kept("neighbours")
    for factor, first in ((1, 0), (2, E.SHELL2_ROWS + 6)):
        rows, meta = E.neighbour_pairs(E.DST, factor)
        assert nb[first:first + 64].tobytes() == rows.astype(np.float32).tobytes()
        crossed = E.axes_crossed(nb[first:first + 64], E.DST, factor)
        # every pair straddles as many cell axes of ITS grid as its direction has components: 12 faces, 12 edges, 8 corners
        assert crossed.tolist() == [int(np.count_nonzero(direction)) for direction, _ in meta], (factor, crossed)
        assert np.bincount(crossed).tolist() == [0, 12, 12, 8]
        for pair, (_, scale) in enumerate(meta):
            a, b = first + 2 * pair, first + 2 * pair + 1
            assert (k[a] and k[b]) == (scale > 1), (factor, pair, k[a], k[b])
            assert k[a] or k[b]
    # the pairs about corners of the 2 dst grid straddle the same axes of the dst grid (a multiple of 2 dst is one of dst)
    first = E.SHELL2_ROWS + 6
    assert E.axes_crossed(nb[first:first + 64], E.DST, 1).tolist() == E.axes_crossed(nb[first:first + 64], E.DST, 2).tolist()
    for ax in range(3):                                      # the shell-2 pairs: the cells of edge dst only
        a, b = E.SHELL2_ROWS + 2 * ax, E.SHELL2_ROWS + 2 * ax + 1
        cells = np.floor(nb[[a, b]].astype(np.float64) / np.float64(np.float32(E.DST)))
        assert cells[1, ax] - cells[0, ax] == 2 and k[a] != k[b]
        assert E.axes_crossed(nb[[a, b]], E.DST, 2).tolist() == [1]


# ---- masks, plane, cover ------------------------------------------------------------------------------------------------------

def test_predicates_of_the_host_build_are_the_restatement(hm):
    scan, pts, names = E.mask_scan()
    rng = np.random.RandomState(5)
    more = (scan["bb"][0] - 2 + rng.rand(4000, 3) * [8, 6, 5]).astype(np.float32)      # around the mask volume
    wide = (scan["bb"][0] - 30 + rng.rand(2000, 3) * [260, 200, 130]).astype(np.float32)  # around the cover's ends
    allp = np.concatenate([pts, more, wide])
    got, want = E.flags_host(hm, allp, scan), E.flags_numpy(allp, scan)
    assert got.tobytes() == want.tobytes()
    for bit in (1, 2, 4):
        assert 20 < ((want & bit) != 0).sum() < len(allp) - 20, bit
    for which in (1, 2, 4, 5, 6):
        assert E.flags_host(hm, allp, scan, which).tobytes() == (want & which).tobytes()
    by_name = dict(zip(names, want[:len(names)]))
    for name, (in_mask, covered) in E.MASK_BY_HAND.items():
        assert (bool(by_name[name] & 1), bool(by_name[name] & 4)) == (in_mask, covered), name
    assert [bool(by_name[n] & 2) for n in ("on_plane", "above_plane", "below_plane")] == [False, True, False]
    for ax in range(3):
        assert not by_name["cover_end_axis%d" % ax] & 4 and by_name["below_cover_end_axis%d" % ax] & 4
    assert scan["obs_mask"].sum() == 7                       # the known pattern: 3 single voxels and a row of 4


# ---- statistics ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.STATS_NAMES)
def test_statistics_of_the_host_build_are_the_restatement(hm, name):
    dist2, select, md = E.stats_cases()[name]
    E.assert_stats(E.stats_host(hm, dist2, select, md), E.stats_numpy(dist2, select, md), name)


def test_statistics_cases_are_what_they_claim():
    cases = E.stats_cases()
    s = E.stats_numpy(*cases["at_max_dist_inf_nan"])
    assert s["n"] == 52                                      # 50 random and two zeros: not the 20.0, not inf, not NaN
    assert np.sqrt(cases["at_max_dist_inf_nan"][0][0]) == 20.0
    assert E.stats_numpy(*cases["ties"]) == dict(n=1000, mean=1.5, var=0.0, median=1.5)
    assert E.stats_numpy(*cases["n0"])["n"] == 0 and np.isnan(E.stats_numpy(*cases["nothing_selected"])["median"])
    one = E.stats_numpy(np.array([4.0]), np.array([True]), 20.0)
    assert one == dict(n=1, mean=2.0, var=0.0, median=2.0)
    assert E.stats_numpy(*cases["ties_in_the_middle"])["median"] == 2.0


# ---- whole scans --------------------------------------------------------------------------------------------------------------

def test_synthetic_scan_leaves_enough_points():
    scan, pred, want = E.scan_case("scan")
    assert len(scan["stl_points"]) == 15000 and len(pred) == 20000
    assert want["n_data"] > 1000 and want["n_stl"] > 1000, (want["n_data"], want["n_stl"])
    assert want["n_data"] < want["data_in_mask"] <= want["points_reduced"] < 20000   # the cover and the 20 mm filter both bite
    assert 0.85 * 15000 < want["stl_above_plane"] < 0.95 * 15000
    assert want["n_stl"] < want["stl_above_plane"]
    assert 0 < want["mean_data"] < 1 and 0 < want["mean_stl"] < 1
    for name in ("file1", "file4"):
        w = E.scan_case(name)[2]
        assert w["n_data"] > 300 and w["n_stl"] > 300


# ---- files --------------------------------------------------------------------------------------------------------------------

def test_read_ply_points_with_extra_properties(tmp_path):
    from mvster_amd import dtu_eval, fusion
    pts = (np.random.RandomState(2).rand(257, 3) * 100 - 50).astype(np.float32)
    for kw in (dict(), dict(double_xyz=True), dict(faces=True), dict(crlf=True), dict(crlf=True, faces=True)):
        fn = str(tmp_path / "rich.ply")
        E.write_rich_ply(fn, pts, **kw)
        got = dtu_eval.read_ply_points(fn)
        assert got.dtype == np.float32 and got.tobytes() == pts.tobytes(), kw
    v = np.zeros(5, fusion.PLY_VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = pts[:5, 0], pts[:5, 1], pts[:5, 2]
    fusion.write_ply(str(tmp_path / "own.ply"), v)
    assert dtu_eval.read_ply_points(str(tmp_path / "own.ply")).tobytes() == pts[:5].tobytes()
    (tmp_path / "ascii.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(RuntimeError, match="ascii.ply"):
        dtu_eval.read_ply_points(str(tmp_path / "ascii.ply"))
    (tmp_path / "twice.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\n"
                                         b"property float z\nproperty float x\nend_header\n" + b"\0" * 16)
    with pytest.raises(RuntimeError, match="read_ply_points: vertex property 'float x' of .*twice.ply"):
        dtu_eval.read_ply_points(str(tmp_path / "twice.ply"))
    (tmp_path / "short.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\n"
                                         b"property float y\nproperty float z\nend_header\n" + b"\0" * 20)
    with pytest.raises(RuntimeError, match="short.ply"):
        dtu_eval.read_ply_points(str(tmp_path / "short.ply"))


def test_scan_truth_from_files(tmp_path):
    from mvster_amd import dtu_eval
    scan, pred, _ = E.scan_case("file1")
    data, plys = str(tmp_path / "data"), str(tmp_path / "plys")
    E.write_scan_files(data, plys, 1, scan, pred)
    t = dtu_eval.read_scan_truth(data, 1)
    assert t["stl_points"].tobytes() == scan["stl_points"].tobytes()
    assert t["obs_mask"].dtype == np.uint8 and np.array_equal(t["obs_mask"], scan["obs_mask"])
    assert np.array_equal(t["bb"], scan["bb"]) and t["res"] == scan["res"] and np.array_equal(t["plane"], scan["plane"])
    assert dtu_eval.read_ply_points(os.path.join(plys, "mvsnet001_l3.ply")).tobytes() == pred.tobytes()
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # read, then refused: the truth lives on the GPU
        dtu_eval.DTUScanTruth.from_files(data, 1, device="cpu")
    with pytest.raises(RuntimeError, match="stl004_total.ply does not exist"):
        dtu_eval.DTUScanTruth.from_files(data, 4)
    E.write_scan_files(data, plys, 4, scan, pred, drop=("ObsMask",))
    with pytest.raises(RuntimeError, match=r"ObsMask4_10\.mat has no variable 'ObsMask'"):
        dtu_eval.DTUScanTruth.from_files(data, 4)
    E.write_scan_files(data, plys, 9, scan, pred)
    with open(os.path.join(data, "ObsMask", "Plane9.mat"), "wb") as f:                  # what `save -v7.3` starts with
        f.write(b"MATLAB 7.3 MAT-file, Platform: GLNXA64".ljust(116) + b"\0" * 8 + b"\x00\x02IM" + b"\0" * 384)
    with pytest.raises(RuntimeError, match=r"Plane9\.mat is a MATLAB v7\.3"):
        dtu_eval.DTUScanTruth.from_files(data, 9)
    with pytest.raises(RuntimeError, match="mvsnet010_l3.ply"):
        dtu_eval.evaluate_dtu(plys, data, scans=(10,))
    assert dtu_eval.DTU_EVAL_SCANS == (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)


# ---- arguments ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_rejected_by_name():
    from mvster_amd import dtu_eval
    pts = torch.zeros(5, 3)
    for dst in (0, -0.2, float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(RuntimeError, match="reduce_points: dst"):
            dtu_eval.reduce_points(pts, dst)
    for seed in (-1, 1.5, 2 ** 63):
        with pytest.raises(RuntimeError, match="reduce_points: seed"):
            dtu_eval.reduce_points(pts, seed=seed)
    with pytest.raises(RuntimeError, match="reduce_points: priority must have the length"):
        dtu_eval.reduce_points(pts, priority=torch.arange(4))
    with pytest.raises(RuntimeError, match="reduce_points: priority must be an int64"):
        dtu_eval.reduce_points(pts, priority=torch.arange(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="reduce_points: priority must be an int64"):
        dtu_eval.reduce_points(pts, priority=list(range(5)))
    with pytest.raises(RuntimeError, match="reduce_points: priority must be on the device"):
        dtu_eval.reduce_points(pts, priority=torch.empty(5, dtype=torch.int64, device="meta"))
    with pytest.raises(RuntimeError, match=r"reduce_points: points must be \[M,3\] float32"):
        dtu_eval.reduce_points(torch.zeros(5, 2))
    with pytest.raises(RuntimeError, match=r"reduce_points: points must be \[M,3\] float32"):
        dtu_eval.reduce_points(torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="reduce_points: table_slots"):
        dtu_eval.reduce_points(pts, table_slots=100)
    for dst, factor in ((0.2, 0), (0.2, 3), (0.2, 2.0), (3e38, 2)):
        with pytest.raises(RuntimeError, match="reduce_points: _cell_factor"):
            dtu_eval.reduce_points(pts, dst, _cell_factor=factor)
    mask, bb, plane = np.ones((3, 3, 3), np.uint8), np.array([[0.0, 0, 0], [1, 1, 1]]), np.array([0.0, 0, 1, 0])
    truth = lambda **kw: dtu_eval.DTUScanTruth(**dict(dict(stl_points=pts, obs_mask=mask, bb=bb, res=0.5, plane=plane), **kw))
    with pytest.raises(RuntimeError, match="DTUScanTruth: obs_mask must be 3-D"):
        truth(obs_mask=np.ones((3, 3), np.uint8))
    for bad in (np.zeros((3, 2)), np.zeros(6), np.full((2, 3), np.nan)):
        with pytest.raises(RuntimeError, match="DTUScanTruth: bb must be 2 x 3"):
            truth(bb=bad)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="DTUScanTruth: res must be finite and > 0"):
            truth(res=bad)
    for bad in (np.zeros(3), np.zeros((4, 2))):
        with pytest.raises(RuntimeError, match="DTUScanTruth: plane must have length 4"):
            truth(plane=bad)
    with pytest.raises(RuntimeError, match="DTUScanTruth: max_dist"):
        truth(max_dist=0)
    with pytest.raises(RuntimeError, match=r"DTUScanTruth: stl_points must be \[M,3\] float32"):
        truth(stl_points=torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="evaluate_dtu_scan: truth must be a DTUScanTruth"):
        dtu_eval.evaluate_dtu_scan(pts, None)
    with pytest.raises(RuntimeError, match="distance_stats: select"):
        dtu_eval.distance_stats(torch.zeros(4, dtype=torch.float64), torch.zeros(3, dtype=torch.bool), 20.0)
    with pytest.raises(RuntimeError, match="distance_stats: dist2"):
        dtu_eval.distance_stats(torch.zeros(4), torch.zeros(4, dtype=torch.bool), 20.0)


def test_cpu_tensors_are_refused():
    from mvster_amd import dtu_eval
    pts = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match=r"dtu_eval\.reduce_points runs on MI355X only.*no CPU fallback"):
        dtu_eval.reduce_points(pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dtu_eval.reduce_points(pts, priority=torch.arange(5))
    with pytest.raises(RuntimeError, match=r"dtu_eval\.DTUScanTruth runs on MI355X only.*no CPU fallback"):
        dtu_eval.DTUScanTruth(pts, np.ones((3, 3, 3)), np.array([[0.0, 0, 0], [1, 1, 1]]), 0.5, np.array([0.0, 0, 1, 0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dtu_eval.distance_stats(torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.bool), 20.0)


def test_library_rejects_bad_sizes_before_any_launch():
    """The entry points of geo_eval.hip validate before the first HIP call (stand-in addresses: nothing is dereferenced)."""
    from mvster_amd import _lib
    lib = _lib.load()
    a = 1 << 32
    assert lib.mvster_eval_reduce_init(None, 5, 0.2, a, a, None) == _lib.ERR_NULL
    assert lib.mvster_eval_reduce_init(a, 5, 0.2, a, None, None) == _lib.ERR_NULL
    assert lib.mvster_eval_reduce_init(a, 0, 0.2, a, a, None) == _lib.ERR_SHAPE
    assert lib.mvster_eval_reduce_init(a, 5, 0.0, a, a, None) == _lib.ERR_SHAPE
    ok = [a, 5, a, a, 64, a, 3, 0.2, 2, None, 0, 5, a, a, 8, None]
    for pos, bad, code in ((0, None, _lib.ERR_NULL), (12, None, _lib.ERR_NULL), (1, 6, _lib.ERR_SHAPE), (4, 100, _lib.ERR_SHAPE),
                           (6, 6, _lib.ERR_SHAPE), (7, float("inf"), _lib.ERR_SHAPE), (7, 3e38, _lib.ERR_SHAPE), (8, 0, _lib.ERR_SHAPE),
                           (8, 3, _lib.ERR_SHAPE), (10, -1, _lib.ERR_SHAPE), (14, 0, _lib.ERR_SHAPE), (14, 65, _lib.ERR_SHAPE)):
        args = list(ok)
        args[pos] = bad
        assert lib.mvster_eval_reduce_rounds(*args) == code, (pos, bad)
    assert lib.mvster_eval_flags(a, 5, None, 3, 3, 3, a, 1, a, a, None) == _lib.ERR_NULL
    assert lib.mvster_eval_flags(a, 5, a, 3, 0, 3, a, 1, a, a, None) == _lib.ERR_SHAPE
    assert lib.mvster_eval_flags(a, 5, None, 0, 0, 0, a, 8, a, a, None) == _lib.ERR_SHAPE
    assert lib.mvster_eval_stats_slots(0) == _lib.ERR_SHAPE and lib.mvster_eval_stats_slots(1) == 1
    assert lib.mvster_eval_stats_slots(4097) == 2 and lib.mvster_eval_stats_slots(1 << 29) == 256
    assert lib.mvster_eval_stats(a, a, 5, 1, 20.0, a, a, None, a, None) == _lib.ERR_NULL
    assert lib.mvster_eval_stats(a, a, 5, 0, 20.0, a, a, a, a, None) == _lib.ERR_SHAPE
    assert lib.mvster_eval_stats(a, a, 5, 1, -1.0, a, a, a, a, None) == _lib.ERR_SHAPE
