"""A scan from a structure-from-motion model without a GPU: the host build of csrc/sfm_math.h against
the NumPy restatement, the error bound of the header's term against long double libm, the readers of COLMAP's text and binary
layouts, the scan folder round trip and the argument checks."""
import os

import numpy as np
import pytest

from mvster_amd import formats, scan, sfm
from tests import sfm_cases as S

NUM_SRC = 10


@pytest.fixture(scope="module")
def hm():
    return S.load_sfm_hostmath()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """seed -> (raw, model read from the text form)"""
    out = {}
    for seed in (11, 12):
        raw = S.synthetic_model(V=40, P=900, seed=seed, rings=2, dropout=0.35, id_step=3, repeat=0.1, orphans=0.05)
        path = str(tmp_path_factory.mktemp("sfm%d" % seed))
        S.write_text(raw, path)
        out[seed] = (raw, sfm.read_sfm_model(path))
    return out


# ---- the host build against NumPy -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [11, 12])
def test_host_scores_are_within_one_unit_per_term_of_numpy(hm, models, seed):
    a = S.arrays_of(models[seed][1])
    got, want, nc = S.pair_scores_host(hm, a), S.pair_scores_numpy(a), S.common_counts(a)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    off = ~np.eye(len(nc), dtype=bool)
    print("pairs with common points: %d, max |q_host - q_numpy| = %d, max n_common = %d" % ((nc[off] > 0).sum(), diff.max(), nc[off].max()))
    assert (nc[off] > 0).sum() > 200 and (got == got.T).all() and (np.diag(got) == 0).all()
    assert (diff[off] <= nc[off]).all()


@pytest.mark.parametrize("seed", [11, 12])
def test_host_depth_ranges_equal_numpy_bytes(hm, models, seed):
    a = S.arrays_of(models[seed][1])
    got, want = S.depth_ranges_host(hm, a), S.depth_ranges_numpy(a)
    assert want[0].min() >= 0 and want[0].max() > 100
    for g, w, name in zip(got, want, ("n", "depth_min", "depth_max")):
        S.assert_bytes(g, w, name)


def test_host_depth_ranges_on_the_edge_counts(hm):
    a, n = S.depth_case()
    got, want = S.depth_ranges_host(hm, a), S.depth_ranges_numpy(a)
    assert np.array_equal(got[0], n)
    for g, w, name in zip(got, want, ("n", "depth_min", "depth_max")):
        S.assert_bytes(g, w, name)
    assert got[1][6] == got[2][6] == 3.25 and np.isnan(got[1][9]) and np.isnan(got[2][9])


def _qualifying_rows(q, nc, num_src):
    """Rows whose list cannot change under a change of every score by up to n_common: among the partners with common points in
    list order, all neighbours up to the first unlisted one differ by more than 2 max(n_common); a list shorter than num_src
    must hold every such partner."""
    V, ok = len(q), []
    for i in range(V):
        cand = [j for j in range(V) if j != i and nc[i, j] > 0]
        cand.sort(key=lambda j: (-int(q[i, j]), j))
        listed = min(num_src, sum(1 for j in cand if q[i, j] > 0))
        good = listed == num_src or listed == len(cand)
        for a, b in zip(cand[:listed], cand[1:listed + 1]):
            good = good and int(q[i, a]) - int(q[i, b]) > 2 * max(nc[i, a], nc[i, b])
        ok.append(good)
    return np.array(ok)


@pytest.mark.parametrize("seed", [11, 12])
def test_host_source_lists_equal_numpy_where_the_gaps_allow(hm, models, seed):
    a = S.arrays_of(models[seed][1])
    qn, nc = S.pair_scores_numpy(a), S.common_counts(a)
    rows = _qualifying_rows(qn, nc, NUM_SRC)
    print("rows whose list is decided by the gaps: %d of %d" % (rows.sum(), len(rows)))
    assert rows.mean() >= 0.9
    want = S.select_numpy(qn, NUM_SRC)
    got = S.select_host(hm, S.pair_scores_host(hm, a), NUM_SRC)
    assert np.array_equal(got[0][rows], want[0][rows]) and np.array_equal(got[2][rows], want[2][rows])
    # and on one and the same matrix the two selections agree everywhere
    same = S.select_host(hm, qn, NUM_SRC)
    for g, w in zip(same, want):
        S.assert_bytes(g, w)


@pytest.mark.parametrize("V,levels", [(65, None), (130, 3)])
def test_host_selection_equals_numpy_on_ties(hm, V, levels):
    q = S.select_matrix(V, seed=V, levels=levels)
    for num_src in (1, 10, 64):
        for g, w in zip(S.select_host(hm, q, num_src), S.select_numpy(q, num_src)):
            S.assert_bytes(g, w, (V, num_src))


def test_pair_decode_enumerates_every_pair_rows_first(hm):
    for L in (2, 3, 64, 65, 300):
        n = L * (L - 1) // 2
        ab = np.zeros((n, 2), np.int64)
        hm.hm_sfm_pairs(L, ab.ctypes.data)
        i, j = np.triu_indices(L, 1)
        assert np.array_equal(ab[:, 0], i) and np.array_equal(ab[:, 1], j), L
    for L in (1 << 20, 3037000):                                            # the ends of long tracks, where the square root only proposes
        n, ab = L * (L - 1) // 2, np.zeros(2, np.int64)
        for e, want in ((0, (0, 1)), (L - 2, (0, L - 1)), (L - 1, (1, 2)), (n - 1, (L - 2, L - 1)), (n - 2, (L - 3, L - 1)),
                        (n - 3, (L - 3, L - 2))):
            hm.hm_sfm_pair_at(e, L, ab.ctypes.data)
            assert tuple(ab) == want, (L, e)


# ---- the error bound of the header's term -------------------------------------------------------------------------------------------

BOUND = 2.0 ** -33


def _sweep():
    """Triples (C_i, C_j, X) whose angle runs through 0, theta0 = 5 and 180 degrees and their float64 neighbourhoods, at several
    scales and orientations -> (ci, cj, x)"""
    rng = np.random.RandomState(7)
    fine = np.concatenate([[0.0], 2.0 ** np.arange(-60, 0, 2.0)])
    degs = np.concatenate([fine, 5.0 - fine[1:], 5.0 + fine, 180.0 - fine, np.linspace(0.0, 180.0, 721), np.linspace(3.0, 7.0, 401),
                           np.linspace(4.999, 5.001, 201), rng.rand(500) * 180.0])
    ci, cj, x = [], [], []
    for scale_a, scale_b, shift in ((1.0, 1.0, 0.0), (3.7, 0.21, 10.0), (1e-3, 2e3, -1e3), (640.0, 655.0, 1e5)):
        Q = S.look_at(rng.randn(3), rng.randn(3))                              # some rotation
        for d in degs:
            t = np.radians(d)
            a, b = np.array([1.0, 0.0, 0.0]) * scale_a, np.array([np.cos(t), np.sin(t), 0.0]) * scale_b
            o = rng.randn(3) * shift
            ci.append(Q @ a + o)
            cj.append(Q @ b + o)
            x.append(o)
    ci, cj, x = np.array(ci), np.array(cj), np.array(x)
    # exact 0 and 180 and their neighbours in float64: b = a, b = -a, and both one step off in one coordinate
    a = np.array([3.0, -2.0, 1.5])
    for s in (1.0, -1.0):
        for step in (0, 1, 2, 3):
            b = s * a.copy()
            for _ in range(step):
                b[1] = np.nextafter(b[1], np.inf)
            ci, cj, x = np.vstack([ci, a]), np.vstack([cj, b]), np.vstack([x, np.zeros(3)])
    return ci, cj, x


def test_term_is_within_two_to_the_minus_33_of_long_double(hm):
    ci, cj, x = _sweep()
    worst = 0.0
    for params in ((5.0, 1.0, 10.0), (5.0, sfm.SIGMA_MIN, sfm.SIGMA_MIN), (0.0, 1.0, 3.0), (180.0, 2.0, 1.0)):
        r = S.terms_host(hm, ci, cj, x, *params)
        e = np.abs(r["err"]).max()
        print("theta0 = %g, sigma = %g / %g: max |term - long double| = %.3e over %d triples (bound %.3e)"
              % (params + (e, len(ci), BOUND)))
        assert e <= BOUND and (r["term"] >= 0).all() and (r["term"] <= 1.0).all()
        worst = max(worst, e)
    assert worst > 0.0                                                      # (the comparison did run)
    r = S.terms_host(hm, ci, cj, x)
    assert r["theta"][-8] == 0.0 and r["term"][-8] == S.terms_host(hm, ci[:1], ci[:1], x[:1])["term"][0]      # b = a: theta = 0
    assert abs(r["theta"][-4] - 180.0) < 1e-12
    # theta exactly theta0: the term is exactly 1, q_term exactly 2^32
    th = float(r["theta"][100])
    one = S.terms_host(hm, ci[100:101], cj[100:101], x[100:101], th, 1.0, 10.0)
    assert one["term"][0] == 1.0 and int(one["qterm"][0]) == 1 << 32
    # a point at a centre: 0
    assert S.terms_host(hm, x[:1], cj[:1], x[:1])["term"][0] == 0.0


def test_exp_neg_against_numpy(hm):
    xs = -np.concatenate([[0.0, 5e-324, 1e-300], 10.0 ** np.linspace(-17, 2, 4000), [99.999, 100.0]])
    got = np.array([hm.hm_sfm_exp_neg(float(v)) for v in xs])
    want = np.exp(xs)
    assert (np.abs(got - want) <= 4 * np.spacing(want)).all()
    assert hm.hm_sfm_exp_neg(-100.0000001) == 0.0 and hm.hm_sfm_exp_neg(float("-inf")) == 0.0 and hm.hm_sfm_exp_neg(float("nan")) == 0.0


# ---- the readers ------------------------------------------------------------------------------------------------------------------------

ARRAYS = ("image_ids", "camera_ids", "qvecs", "tvecs", "R", "centres", "K", "sizes", "point_ids", "points", "view_ptr", "view_pts",
          "pt_ptr", "pt_views")


def test_text_and_binary_forms_read_to_identical_arrays(models, tmp_path):
    raw, text = models[11]
    S.write_binary(raw, str(tmp_path / "bin"))
    S.write_text(raw, str(tmp_path / "plain"), comments=False)
    binary, plain = sfm.read_sfm_model(str(tmp_path / "bin")), sfm.read_sfm_model(str(tmp_path / "plain"))
    for other in (binary, plain):
        for k in ARRAYS:
            S.assert_bytes(other[k], text[k], k)
        assert other["names"] == text["names"]
    # ordered by image id, ids not contiguous, names with spaces and folders kept whole
    assert np.array_equal(text["image_ids"], 1 + 3 * np.arange(40)) and text["names"][0] == "view 000.png"
    assert text["names"][1] == "ring1/view_001.png"
    # the tables: sorted distinct points per view, transposed per point; -1, repeats and ids without a point are gone
    by_id = {im[0]: im for im in raw["images"]}
    known = set(int(p[0]) for p in raw["points"])
    for v, iid in enumerate(text["image_ids"]):
        ids = sorted(set(int(p) for p in by_id[int(iid)][5][:, 2]) & known)
        assert len(ids) < len(by_id[int(iid)][5])                               # (something was dropped in every view)
        got = text["point_ids"][text["view_pts"][text["view_ptr"][v]:text["view_ptr"][v + 1]]]
        assert np.array_equal(got, ids), v
    for p in (0, 17, len(text["point_ids"]) - 1):
        views = text["pt_views"][text["pt_ptr"][p]:text["pt_ptr"][p + 1]]
        want = [v for v in range(40) if p in text["view_pts"][text["view_ptr"][v]:text["view_ptr"][v + 1]]]
        assert list(views) == want
    # x_cam = R X + t and C = -R^T t
    assert np.allclose(np.einsum("vij,vj->vi", text["R"], text["centres"]) + text["tvecs"], 0, atol=1e-12)
    assert np.allclose(text["R"] @ text["R"].transpose(0, 2, 1), np.eye(3), atol=1e-12)


def test_binary_is_preferred_and_a_bare_folder_raises(models, tmp_path):
    raw, _ = models[11]
    other = S.synthetic_model(V=5, P=50, seed=3)
    S.write_text(other, str(tmp_path))
    S.write_binary(raw, str(tmp_path))
    assert len(sfm.read_sfm_model(str(tmp_path))["image_ids"]) == 40
    with pytest.raises(RuntimeError, match="neither"):
        sfm.read_sfm_model(str(tmp_path / "nothing"))


def test_empty_observation_line_and_missing_last_line(tmp_path):
    raw = S.synthetic_model(V=4, P=60, seed=5, dropout=0.0)
    raw["images"][1] = raw["images"][1][:5] + (np.zeros((0, 3)),)
    S.write_text(raw, str(tmp_path / "a"))
    S.write_binary(raw, str(tmp_path / "b"))
    a, b = sfm.read_sfm_model(str(tmp_path / "a")), sfm.read_sfm_model(str(tmp_path / "b"))
    v = int(np.nonzero(a["image_ids"] == raw["images"][1][0])[0][0])
    assert a["view_ptr"][v] == a["view_ptr"][v + 1] and np.array_equal(a["view_ptr"], b["view_ptr"])
    assert (np.diff(a["view_ptr"]) > 0).sum() == 3
    # a file that ends right after the last image's first line
    lines = open(str(tmp_path / "a" / "images.txt")).read().rstrip("\n").split("\n")
    last = raw["images"][-1][0]
    open(str(tmp_path / "a" / "images.txt"), "w").write("\n".join(lines[:-1]) + "\n")
    c = sfm.read_sfm_model(str(tmp_path / "a"))
    w = int(np.nonzero(c["image_ids"] == last)[0][0])
    assert c["view_ptr"][w] == c["view_ptr"][w + 1] and len(c["image_ids"]) == 4


@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
def test_models_without_distortion_are_taken(tmp_path, model):
    raw = S.synthetic_model(V=3, P=30, seed=model, model=model)
    S.write_text(raw, str(tmp_path / "t"))
    S.write_binary(raw, str(tmp_path / "b"))
    for sub in ("t", "b"):
        m = sfm.read_sfm_model(str(tmp_path / sub))
        assert m["K"][0, 0, 0] == 140.0 and m["K"][0, 0, 2] == 80.0 and m["K"][0, 1, 2] == 60.0 and tuple(m["sizes"][0]) == (120, 160)
        assert m["K"][0, 1, 1] == (140.0 * 1.01 if model == 1 else 140.0)


@pytest.mark.parametrize("model,at", [(2, 3), (3, 4), (4, 6)])
def test_a_distorted_model_raises_and_names_the_undistorter(tmp_path, model, at):
    raw = S.synthetic_model(V=3, P=30, seed=1, model=model)
    m, w, h, params = raw["cameras"][3]
    raw["cameras"][3] = (m, w, h, params[:at] + [0.01] + params[at + 1:])
    S.write_text(raw, str(tmp_path / "t"))
    S.write_binary(raw, str(tmp_path / "b"))
    for sub in ("t", "b"):
        with pytest.raises(RuntimeError, match="image_undistorter"):
            sfm.read_sfm_model(str(tmp_path / sub))


def test_an_unknown_camera_model_raises(tmp_path):
    raw = S.synthetic_model(V=3, P=30, seed=1)
    raw["cameras"][3] = (6, 160, 120, [140.0] * 12)
    S.write_text(raw, str(tmp_path / "t"))
    S.write_binary(raw, str(tmp_path / "b"))
    for sub in ("t", "b"):
        with pytest.raises(RuntimeError, match="image_undistorter"):
            sfm.read_sfm_model(str(tmp_path / sub))


# ---- to a scan and back ---------------------------------------------------------------------------------------------------------------

def test_write_scan_folder_then_read_scan_folder(hm, models, tmp_path):
    pytest.importorskip("PIL.Image")
    raw, model = models[12]
    rng = np.random.RandomState(0)
    graph = S.graph_host(hm, S.arrays_of(model), num_src=4)
    graph["n_obs"] = graph["n_obs"].copy()
    graph["n_obs"][7] = 0                                                    # (stands for a view with nothing in front of it)
    sc = sfm.assemble_scan(model, graph, lambda v: rng.randint(0, 256, size=(120, 160, 3)).astype(np.uint8))
    V = len(sc["view_ids"])
    assert V == 39 and sc["dropped_views"] == [int(model["image_ids"][7])] and int(model["image_ids"][7]) not in sc["view_ids"]
    assert all(len(s) <= 4 for _, s in sc["pairs"]) and sc["Ks"].dtype == np.float32 and sc["Es"].dtype == np.float32
    assert np.array_equal(sc["Ks"][:, 0, 0], np.full(V, np.float32(140.0 / 4)))
    root = str(tmp_path / "scan")
    sfm.write_scan_folder(sc, root, ndepths=48)
    back = scan.read_scan_folder(root, "", dataset="tanks")
    assert back["view_ids"] == sc["view_ids"]                                # (every kept view has sources here)
    assert np.array_equal(back["Ks"], sc["Ks"]) and np.array_equal(back["Es"], sc["Es"])
    assert back["depth_ranges"] == sc["depth_ranges"] and back["pairs"] == sc["pairs"]
    assert all(im.shape == (120, 160, 3) for im in back["images"])
    name = os.path.join(root, "cams", "{:0>8}_cam.txt".format(sc["view_ids"][3]))
    lo, hi = sc["depth_ranges"][3]
    K, E, dmin, dmax = formats.read_cam_file_minmax(name)
    assert (dmin, dmax) == (lo, hi) and np.array_equal(K[:2], sc["Ks"][3][:2] * 4)
    _, _, dmin, interval = formats.read_cam_file(name, 1.0, 48)
    assert dmin == lo and abs(interval - (hi - lo) / 48) <= 1e-15 * hi
    # the scores of pair.txt are the graph's
    lines = open(os.path.join(root, "pair.txt")).read().split("\n")
    assert int(lines[0]) == V
    r, srcs = sc["pairs"][0]
    fields = lines[2 + 2 * r].split()
    assert [float(s) for s in fields[2::2]] == sc["pair_scores"][0] and int(fields[0]) == len(srcs)
    # the plan the scan entry makes of it
    plan = scan.plan_scan(sc["Ks"], sc["Es"], sc["depth_ranges"], sc["pairs"], nviews=5, depth_range_kind="min_max",
                          short_sources="fewer_views")
    assert len(plan.ref_views) == len(sc["pairs"])


def test_assemble_scan_refuses_an_image_of_another_size(hm, models):
    _, model = models[12]
    graph = S.graph_host(hm, S.arrays_of(model))
    with pytest.raises(RuntimeError, match="camera says"):
        sfm.assemble_scan(model, graph, lambda v: np.zeros((100, 160, 3), np.uint8))


# ---- the argument checks ------------------------------------------------------------------------------------------------------------

def test_argument_checks_come_before_the_device(models):
    _, model = models[11]
    a = S.arrays_of(model)
    for kw in (dict(theta0=-1.0), dict(theta0=181.0), dict(sigma1=0.0), dict(sigma2=0.01), dict(sigma1=float("inf")),
               dict(theta0=float("nan"))):
        with pytest.raises(RuntimeError, match="theta0|sigma"):
            sfm.pair_scores(a["centres"], a["points"], a["pt_ptr"], a["pt_views"], **kw)
        with pytest.raises(RuntimeError, match="theta0|sigma"):
            sfm.view_graph(model, **kw)
    for num_src in (0, 65, 2.5):
        with pytest.raises(RuntimeError, match="num_src"):
            sfm.view_graph(model, num_src=num_src)
    import torch
    with pytest.raises(RuntimeError, match="num_src"):
        sfm.select_sources(torch.zeros(4, 4, dtype=torch.int64), 0)
    with pytest.raises(RuntimeError, match=r"int64 \[V,V\]"):
        sfm.select_sources(torch.zeros(4, 5, dtype=torch.int64), 3)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sfm.select_sources(torch.zeros(4, 4, dtype=torch.int64), 3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sfm.view_graph(model)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sfm.depth_ranges(a["rt"], a["points"], a["view_ptr"], a["view_pts"])


def test_tables_are_checked_on_the_host():
    ptr, idx = np.array([0, 2, 3], np.int64), np.array([0, 1, 1], np.int32)
    sfm._check_table("t", "pt", ptr, idx, 2, 2)
    for bad_ptr, bad_idx in ((np.array([0, 2, 4], np.int64), idx), (np.array([1, 2, 3], np.int64), idx),
                             (np.array([0, 3, 2, 3], np.int64)[:3], idx), (ptr, np.array([0, 1, 2], np.int32)),
                             (ptr, np.array([0, -1, 1], np.int32)), (ptr[:2], idx)):
        with pytest.raises(RuntimeError):
            sfm._check_table("t", "pt", bad_ptr, bad_idx, 2, 2)
    s = sfm.structure([1, 0, 1, 1, 0], [2, 0, 2, 1, 0], 3, 3)
    assert list(s["view_ptr"]) == [0, 1, 3, 3] and list(s["view_pts"]) == [0, 1, 2]
    assert list(s["pt_ptr"]) == [0, 1, 2, 3] and list(s["pt_views"]) == [0, 1, 1]


def test_write_scan_folder_checks_its_dict(tmp_path):
    sc = dict(view_ids=[1, 2], Ks=np.zeros((2, 3, 3)), Es=np.zeros((2, 4, 4)), images=[np.zeros((8, 8, 3), np.uint8)],
              depth_ranges=[(1.0, 2.0)] * 2, pairs=[])
    with pytest.raises(RuntimeError, match="view_ids"):
        sfm.write_scan_folder(sc, str(tmp_path))
    with pytest.raises(RuntimeError, match="ndepths"):
        sfm.write_scan_folder(sc, str(tmp_path), ndepths=0)
