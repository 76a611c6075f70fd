"""Cleaning a fused cloud without a GPU: the host brute force of mvster_amd/csrc/knn_math.h against the
NumPy restatement bit for bit (lists, counts, the radius filter), the host grid search against the host brute force at three
cell sizes (which proves the stopping rule for a full list), the statistical filter and the normals against NumPy within bounds
derived here, what the case clouds claim, the argument checks of the Python entry points and the PLY with normals."""
import numpy as np
import pytest
import torch

from mvster_amd import dtu_eval, fusion
from tests import cloud_clean_cases as K
from tests import cloud_nn_cases as N


@pytest.fixture(scope="module")
def khm():
    return K.load_knn_hostmath()


def grid_cells(md):
    """max_dist / 15, the default and 4 max_dist"""
    c = N.cell_values(md)
    return (c[0], c[1], c[3])


def test_case_clouds_are_what_they_claim(khm):
    cases = K.knn_cases()
    assert tuple(cases) == K.KNN_CASE_NAMES
    # lattice: an interior point has 6 neighbours at d2 = 1 and 12 at d2 = 2, so k = 10 cuts the second group: by index
    q, t, md, same = cases["lattice"]
    got = K.knn_host(khm, q, t, K.LATTICE_K, md, N.default_cell(md), True)
    inner = np.nonzero(((q >= 2) & (q <= 6)).all(1))[0]
    assert same and len(inner) == 125
    for i in inner[:20]:
        assert got["dist2"][i].tolist() == [1.0] * 6 + [2.0] * 4
        d2 = ((t.astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(1)
        assert got["index"][i, 6:].tolist() == np.nonzero(d2 == 2.0)[0][:4].tolist()      # the four smallest indices of twelve
    # duplicates: with exclude_self a point's two copies are its nearest neighbours at d2 = 0, without it the point itself too
    q, t, md, _ = cases["duplicates"]
    cell = N.default_cell(md)
    on, off = K.knn_host(khm, q, t, 5, md, cell, True), K.knn_host(khm, q, t, 5, md, cell, False)
    assert (on["dist2"][:, :2] == 0).all() and (on["dist2"][:, 2] > 0).all() and (on["index"][:, :2] != np.arange(360)[:, None]).all()
    assert (off["dist2"][:, :3] == 0).all() and (np.sort(off["index"][:, :3], 1) == off["index"][:, :3]).all()
    assert ((off["index"][:, :3] == np.arange(360)[:, None]).sum(1) == 1).all()
    # boundary: the seven targets exactly at max_dist are found, the seven one float32 beyond are not
    q, t, md, _ = cases["boundary"]
    got = K.knn_host(khm, q, t, 32, md, N.default_cell(md))
    assert got["count"].tolist() == [7] and got["index"][0, :7].tolist() == list(range(7, 14))
    assert (got["dist2"][0, :7] == np.float64(md) ** 2).all() and np.isposinf(got["dist2"][0, 7:]).all()
    # stop_rule: query 0's list is full after shell 1 and the nearer target of shell 2 still enters it; query 1's third neighbour
    # lies in shell 4 of 5
    q, t, md, _ = cases["stop_rule"]
    g = N.default_cell(md)
    shell = lambda a, b: int(np.abs(np.floor(b.astype(np.float64) / g) - np.floor(a.astype(np.float64) / g)).max())
    assert [shell(q[0], t[j]) for j in (0, 1, 2)] == [1, 2, 1] and khm.hm_knn_brute is not None
    got = K.knn_host(khm, q, t, 2, md, g)
    assert got["index"][0].tolist() == [1, 0] and abs(np.sqrt(got["dist2"][0, 0]) / g - 1.1) < 1e-5
    got = K.knn_host(khm, q, t, 3, md, g)
    assert got["index"][1].tolist() == [3, 4, 5] and shell(q[1], t[5]) == 4 and N.load_nn_hostmath().hm_nn_rings(md, g) == 5
    assert got["count"].tolist() == [3, 3] and shell(q[1], t[6]) == 4
    # single_cell: one cell at the default grid
    q = cases["single_cell"][0]
    assert len({tuple(c) for c in np.floor(q.astype(np.float64) / g)}) == 1
    # radius cloud, blob, few
    pts, kinds = K.radius_cloud()
    nb, _ = K.radius_host(khm, pts, K.RADIUS, 1, N.default_cell(K.RADIUS))
    assert nb[kinds == 0].min() == 3 and nb[kinds == 0].max() == 6 and (nb[kinds == 1] == 0).all() and (nb[kinds == 2] == 1).all()
    pts, nbs = K.few_cloud()
    assert K.knn_host(khm, pts, pts, 5, 1.0, 0.25, True)["count"].tolist() == nbs.tolist()


@pytest.mark.parametrize("name", K.KNN_CASE_NAMES)
def test_host_brute_force_equals_the_restatement(khm, name):
    q, t, md, same = K.knn_cases()[name]
    cells = N.cell_values(md) if name in ("invalid", "faces", "ties") else (N.default_cell(md),)
    for cell in cells:
        for k in K.case_ks(name):
            for ex in ((False, True) if same else (False,)):
                K.assert_same_knn(K.knn_host(khm, q, t, k, md, cell, ex), K.knn_numpy(q, t, k, md, cell, ex), (name, cell, k, ex))
    with pytest.raises(AssertionError):                                      # (the comparison can fail)
        K.assert_bytes(np.zeros(3), np.array([0.0, -0.0, 0.0]))


@pytest.mark.parametrize("which", range(3))
def test_host_grid_search_equals_the_host_brute_force(khm, which):
    """R shells are enough, and stopping after shell r once the list is full and its k-th d2 <= (r cell)^2 (1 - 2^-20) loses
    nothing: neither a nearer point nor an index tie at the list's end."""
    for name, (q, t, md, same) in K.knn_cases().items():
        cell = grid_cells(md)[which]
        if which == 0 and name == "self_random":                             # 35^3 cells per query on the host: fewer queries
            continue
        if which == 0 and name in ("pair_random", "one_cell"):
            q = q[:150]
        for k in K.case_ks(name):
            for ex in ((False, True) if same else (False,)):
                K.assert_same_knn(K.knn_host(khm, q, t, k, md, cell, ex, grid=True), K.knn_host(khm, q, t, k, md, cell, ex),
                                  (name, cell, k, ex))


def test_radius_filter_equals_the_restatement(khm):
    pts, kinds = K.radius_cloud()
    for cell in grid_cells(K.RADIUS):
        for nb_points in (1, 2):
            want = K.radius_numpy(pts, K.RADIUS, nb_points, cell)
            for grid in (False, True):
                got = K.radius_host(khm, pts, K.RADIUS, nb_points, cell, grid)
                K.assert_bytes(got[0], want[0], ("neighbours", cell, grid))
                K.assert_bytes(got[1], want[1], ("keep", cell, grid))
            assert want[1].tolist() == ((kinds == 0) | ((kinds == 2) & (nb_points == 1))).tolist()
    for name in ("duplicates", "lattice", "invalid", "self_random"):
        q, _, md, _ = K.knn_cases()[name]
        cell = N.default_cell(md)
        want = K.radius_numpy(q, md, 3, cell)
        for grid in (False, True):
            got = K.radius_host(khm, q, md, 3, cell, grid)
            K.assert_bytes(got[0], want[0], (name, grid))
            K.assert_bytes(got[1], want[1], (name, grid))


def test_statistical_filter_against_numpy(khm):
    """mean bit-equal to the restatement summed in list order; threshold within 1e-12 relative of NumPy's (n <= 4112 terms of one
    sign in mu, error <= n 2^-53 = 4.6e-13 relative, the same for the sum of squares; sqrt halves it); keep exactly
    mean <= threshold for the threshold returned."""
    pts, planted = K.blob_cloud()
    cell = N.default_cell(K.STAT_MD)
    lists = K.knn_numpy(pts, pts, K.STAT_K, K.STAT_MD, cell, True)
    want_mean = K.mean_numpy(lists, K.STAT_K)
    for grid in (False, True):
        got = K.statistical_host(khm, pts, K.STAT_K, K.STAT_RATIO, K.STAT_MD, cell, grid)
        K.assert_bytes(got["mean"], want_mean, ("mean", grid))
        K.assert_bytes(got["count"], lists["count"], ("count", grid))
        n, mu, sigma, threshold = K.stats_numpy(want_mean, K.STAT_RATIO)
        print("statistical: n %d, mu %.17g (NumPy %.17g), sigma %.17g (%.17g), threshold %.17g (%.17g)" %
              (got["n"], got["mu"], mu, got["sigma"], sigma, got["threshold"], threshold))
        assert got["n"] == n and n > 4096
        assert abs(got["mu"] - mu) <= 1e-12 * mu and abs(got["sigma"] - sigma) <= 1e-12 * sigma
        assert abs(got["threshold"] - threshold) <= 1e-12 * threshold
        with np.errstate(invalid="ignore"):
            assert got["keep"].tolist() == (np.isfinite(want_mean) & (want_mean <= got["threshold"])).tolist()
        assert not got["keep"][planted].any() and got["keep"][~planted].mean() > 0.9
    # fewer than two participants: sigma 0; none: NaN and nothing kept; invalid points NaN, isolated ones +inf
    pts, _ = K.few_cloud()
    got = K.statistical_host(khm, pts, 2, 1.0, 1.0, 0.25)
    assert got["n"] == 3 and got["keep"].tolist() == [False] * 3 + [m <= got["threshold"] for m in got["mean"][3:]]
    assert np.isposinf(got["mean"][:3]).all()
    one = K.statistical_host(khm, np.array([[0, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [9, 9, 9]], np.float32), 1, 1.0, 1.0, 0.25)
    assert one["n"] == 2 and one["sigma"] == 0.0 and one["mu"] == 0.5 and one["keep"].tolist() == [True, True, False, False]
    assert np.isnan(one["mean"][2]) and np.isposinf(one["mean"][3])
    none = K.statistical_host(khm, pts[:1], 1, 1.0, 1.0, 0.25)
    assert none["n"] == 0 and np.isnan(none["mu"]) and np.isnan(none["threshold"]) and not none["keep"].any()


def test_normals_against_eigh(khm):
    """Host normals against numpy.linalg.eigh of the same C: angle <= 1e-6 rad (the float32 output rounds each component by
    <= 2^-24, about 1e-7 rad; the fp64 eigenvector error is <= eps ||C|| / gap <= 2.2e-16 / 1e-3), on clouds where
    (l1 - l0) / l2 >= 1e-3 for every point -- checked here, no point is left out."""
    sphere = K.sphere_cloud()
    for pts, k, md in (K.plane_cloud(), (sphere[0], sphere[2], sphere[3])):
        for grid in (False, True):
            got = K.normals_host(khm, pts, k, md, N.default_cell(md), grid=grid)
            assert got["valid"].all()
            want, gap = K.eigh_normals(got["cov"])
            ang = K.angles(got["normals"], want)
            print("normals: %d points, smallest gap %.3g, largest angle %.3g rad" % (len(pts), gap.min(), ang.max()))
            assert gap.min() >= K.GAP
            assert ang.max() <= K.ANGLE
            lead = got["normals"][np.arange(len(pts)), np.abs(got["normals"]).argmax(1)]
            assert (lead > 0).all()                                          # the raw sign
            assert np.abs(np.linalg.norm(got["normals"].astype(np.float64), axis=1) - 1).max() < 2e-7
    # the restatement from the lists (another C, summed by NumPy) agrees as well
    pts, k, md = K.plane_cloud()
    cell = N.default_cell(md)
    want, valid, gap = K.normals_numpy(pts, K.knn_numpy(pts, pts, k, md, cell, True))
    got = K.normals_host(khm, pts, k, md, cell)
    assert valid.all() and gap.min() >= K.GAP and K.angles(got["normals"], want).max() <= K.ANGLE
    # signs: toward the centre, away from it
    pts, centre, k, md = K.sphere_cloud()
    cell = N.default_cell(md)
    inward = K.normals_host(khm, pts, k, md, cell, toward=np.broadcast_to(centre, pts.shape))
    outward = K.normals_host(khm, pts, k, md, cell, toward=(centre + 100 * (pts - centre)).astype(np.float32))
    radial = (pts - centre).astype(np.float64)
    assert ((inward["normals"] * radial).sum(1) < -0.9).all() and ((outward["normals"] * radial).sum(1) > 0.9).all()
    K.assert_bytes(inward["normals"], -outward["normals"])
    # 0 and 1 neighbours: zeros, not valid
    pts, nbs = K.few_cloud()
    few = K.normals_host(khm, pts, 5, 1.0, 0.25)
    assert few["valid"].tolist() == (nbs >= 2).tolist() and (few["normals"][:3] == 0).all()
    flat = np.cross(pts[4].astype(np.float64) - pts[3], pts[5].astype(np.float64) - pts[3])
    assert K.angles(few["normals"][3:], np.tile(flat / np.linalg.norm(flat), (3, 1))).max() <= K.ANGLE    # the triangle's plane
    # n . (toward - p) exactly 0 keeps the raw sign; a negative product flips
    pts = K.cross_cloud()
    for tw, want in (((1, 0, 0), (0, 0, 1)), ((1, 0, -1), (0, 0, -1)), ((0, -3, 2), (0, 0, 1))):
        got = K.normals_host(khm, pts, 4, 1.25, 0.3125, toward=np.tile(np.array(tw, np.float32), (5, 1)))
        assert got["valid"].tolist() == [True] + [False] * 4 and got["normals"][0].tolist() == list(want), (tw, got["normals"][0])
        assert got["cov"][0].tolist() == [0.4, 0.0, 0.0, 0.4, 0.0, 0.0]


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------

A, B = torch.zeros(5, 3), torch.zeros(7, 3)


def test_entry_points_check_their_arguments_before_the_gpu():
    calls = {
        "nearest_neighbors": lambda k=3, md=0.5, **kw: fusion.nearest_neighbors(A, B, k, md, **kw),
        "statistical_outliers": lambda k=3, md=0.5, **kw: fusion.statistical_outliers(A, k, 2.0, md, **kw),
        "estimate_normals": lambda k=3, md=0.5, **kw: fusion.estimate_normals(A, k, md, **kw),
    }
    for name, call in calls.items():
        for bad in (0, 33, -1, 2.5, None, True):
            with pytest.raises(RuntimeError, match=name + ": k must be an integer in 1 .. 32"):
                call(k=bad)
        for bad in (0, -0.2, float("nan"), float("inf"), 1e-60, 1e60, None, "abc"):
            with pytest.raises(RuntimeError, match=name + ": max_dist"):
                call(md=bad)
        for bad in (0, -1, float("nan"), float("inf"), 0.5 / 15.1):
            with pytest.raises(RuntimeError, match=name + ": cell"):
                call(cell=bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # everything else is fine: only the device is not
            call()
    for bad in (0, -0.2, float("nan"), float("inf"), None):
        with pytest.raises(RuntimeError, match="radius_outliers: radius"):
            fusion.radius_outliers(A, bad, 2)
    for bad in (0, -1, 1.5, None):
        with pytest.raises(RuntimeError, match="radius_outliers: nb_points"):
            fusion.radius_outliers(A, 0.5, bad)
    with pytest.raises(RuntimeError, match="radius_outliers: cell must be >= radius / 15"):
        fusion.radius_outliers(A, 0.5, 2, cell=0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fusion.radius_outliers(A, 0.5, 2)
    for bad in (float("nan"), float("inf"), None, "x"):
        with pytest.raises(RuntimeError, match="statistical_outliers: std_ratio"):
            fusion.statistical_outliers(A, 3, bad, 0.5)
    with pytest.raises(RuntimeError, match="exclude_self needs as many queries as targets"):
        fusion.nearest_neighbors(A, B, 3, 0.5, exclude_self=True)
    with pytest.raises(RuntimeError, match=r"query must be \[M,3\] float32"):
        fusion.nearest_neighbors(A.double(), B, 3, 0.5)
    with pytest.raises(RuntimeError, match="target must be a torch tensor"):
        fusion.nearest_neighbors(A, B.numpy(), 3, 0.5)
    with pytest.raises(RuntimeError, match=r"points must be \[M,3\] float32"):
        fusion.estimate_normals(torch.zeros(5, 4), 3, 0.5)
    with pytest.raises(RuntimeError, match="toward must be a"):
        fusion.estimate_normals(A, 3, 0.5, toward=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="colors must be a"):
        fusion.radius_outliers(A, 0.5, 2, colors=torch.zeros(5, 3))
    for slots in (48, 100, 32, 64.0):
        with pytest.raises(RuntimeError, match="table_slots"):
            fusion.nearest_neighbors(A, torch.zeros(33, 3), 3, 0.5, table_slots=slots)

    class FakeGrid(fusion.CloudGrid):                                        # a CloudGrid of another cell, without a GPU
        def __init__(self, cell, M):
            self.cell, self.M = cell, M
    for call in (lambda g: fusion.nearest_neighbors(A, g, 3, 0.5, cell=0.25), lambda g: fusion.nearest_neighbors(g, B, 3, 0.5, cell=0.25),
                 lambda g: fusion.statistical_outliers(g, 3, 2.0, 0.5, cell=0.25), lambda g: fusion.estimate_normals(g, 3, 0.5, cell=0.25),
                 lambda g: fusion.radius_outliers(g, 0.5, 2, cell=0.25)):
        with pytest.raises(RuntimeError, match="has cell 0.125, not the cell 0.25"):
            call(FakeGrid(0.125, 7))


def test_scan_level_keywords_are_checked_before_anything_runs():
    bad = [dict(outliers=(0.5, 2)), dict(outliers=fusion.RadiusOutliers(0.0, 2)), dict(outliers=fusion.RadiusOutliers(0.5, 0)),
           dict(outliers=fusion.StatisticalOutliers(0, 2.0, 0.5)), dict(outliers=fusion.StatisticalOutliers(33, 2.0, 0.5)),
           dict(outliers=fusion.StatisticalOutliers(8, float("nan"), 0.5)), dict(outliers=fusion.StatisticalOutliers(8, 2.0, -1)),
           dict(normals=(8, 0.5)), dict(normals=fusion.Normals(0, 0.5)), dict(normals=fusion.Normals(8, float("inf")))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="fuse_scene: (outliers|normals)"):
            fusion.fuse_scene(None, None, None, None, None, None, 0.5, 2, **kw)
        with pytest.raises(RuntimeError, match="filter_depth: (outliers|normals)"):
            fusion.filter_depth("nowhere", "nowhere", "nowhere", "nowhere.ply", **kw)
        from mvster_amd import scan
        with pytest.raises(RuntimeError, match="reconstruct_scan: (outliers|normals)"):
            scan.reconstruct_scan(None, None, None, None, None, None, **kw)
    assert fusion.RadiusOutliers(0.5, 2) == (0.5, 2) and fusion.StatisticalOutliers(8, 2.0, 0.5).std_ratio == 2.0
    assert fusion.Normals(12, 0.1)._fields == ("k", "max_dist") and fusion.MAX_K == 32


def test_c_abi_checks_come_before_any_hip_call():
    """Stand-in addresses that nothing may dereference: every bad argument is refused with MVSTER_ERR_SHAPE / _NULL."""
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    p = 1 << 32
    grid = (p, p, 100, p, p, 256, p, 10, 100)                                # records, cell_of_point, M, keys, first, slots, starts, ncells, nrecords
    query = (p, p, p, 100, p, p, 256, p, p, 10, 100)

    def knn(md=0.5, cell=0.125, k=3, ex=0, M=100, out=p):
        return lib.mvster_cloud_knn_query(*query, md, cell, k, ex, M, out, p, p, None)
    assert [knn(k=0), knn(k=33), knn(md=0.0), knn(md=float("inf")), knn(cell=0.5 / 16), knn(cell=float("nan")), knn(ex=1, M=99),
            knn(ex=2)] == [_lib.ERR_SHAPE] * 8
    assert knn(out=None) == _lib.ERR_NULL
    assert lib.mvster_cloud_knn_query(p, p, p, 100, p, p, 100, p, p, 10, 100, 0.5, 0.125, 3, 0, 100, p, p, p, None) == _lib.ERR_SHAPE
    for k in (0, 33):
        assert lib.mvster_cloud_knn_mean(*grid, 0.5, 0.125, k, p, p, None) == _lib.ERR_SHAPE
        assert lib.mvster_cloud_knn_normals(*grid, 0.5, 0.125, k, p, None, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_knn_mean(*grid, 0.5, 0.125, 3, None, p, None) == _lib.ERR_NULL
    assert lib.mvster_cloud_knn_mean(*grid, -1.0, 0.125, 3, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_knn_normals(*grid, 0.5, 0.125, 3, None, None, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_cloud_radius_count(*grid, 0.5, 0.01, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_radius_count(*grid, 0.5, 0.125, None, None) == _lib.ERR_NULL
    assert lib.mvster_cloud_radius_count(p, p, 0, p, p, 256, p, 10, 100, 0.5, 0.125, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_knn_stats_rows(0) == _lib.ERR_SHAPE and lib.mvster_cloud_knn_stats_rows(5000) == 2
    assert lib.mvster_cloud_knn_stats_rows(1 << 29) == 256 and lib.mvster_cloud_knn_stats_rows((1 << 29) + 1) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_knn_stats(p, 100, float("nan"), p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_knn_stats(p, 0, 2.0, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_knn_stats(None, 100, 2.0, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_cloud_keep_flags(p, p, 0, None, None, 100, p, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_cloud_keep_flags(None, p, 1, None, None, 100, p, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_cloud_keep_flags(None, None, 0, p, None, 100, p, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_cloud_keep_flags(None, None, 0, p, p, 0, p, p, p, None) == _lib.ERR_SHAPE


# ---- the PLY with normals ---------------------------------------------------------------------------------------------------

def test_write_ply_with_normals_round_trips_and_without_them_writes_the_old_bytes(tmp_path):
    rng = np.random.RandomState(0)
    v = np.empty(37, dtype=fusion.PLY_VERTEX_DTYPE)
    for name in "xyz":
        v[name] = rng.randn(37).astype(np.float32)
    for name in ("red", "green", "blue"):
        v[name] = rng.randint(0, 256, 37)
    normals = rng.randn(37, 3).astype(np.float32)
    plain, with_n = str(tmp_path / "plain.ply"), str(tmp_path / "normals.ply")
    fusion.write_ply(plain, v)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert open(plain, "rb").read() == header.encode("ascii") + v.tobytes()
    assert fusion.read_ply(plain).tobytes() == v.tobytes()
    fusion.write_ply(with_n, v, normals=torch.from_numpy(normals))
    data = open(with_n, "rb").read()
    head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
    assert [l.split()[-1] for l in head if l.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert len(data) == data.index(b"end_header\n") + 11 + 37 * 27
    xyz = dtu_eval.read_ply_points(with_n)
    assert xyz.tobytes() == np.stack([v["x"], v["y"], v["z"]], 1).tobytes()
    body = np.frombuffer(data[-37 * 27:], dtype=fusion.PLY_NORMAL_VERTEX_DTYPE)
    assert np.stack([body["nx"], body["ny"], body["nz"]], 1).tobytes() == normals.tobytes() and body["green"].tobytes() == v["green"].tobytes()
    with pytest.raises(RuntimeError, match="normals must be"):
        fusion.write_ply(with_n, v, normals=normals[:5])
