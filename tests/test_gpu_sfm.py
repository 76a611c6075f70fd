"""A scan from a structure-from-motion model on the GPU: csrc/geo_sfm.hip byte for byte against the host
build of csrc/sfm_math.h -- pair scores, source lists, depth ranges -- at the shapes where the kernels can go wrong, and one scan
from a COLMAP text model through ``reconstruct_scan``."""
import os

import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, scan, sfm
from tests import scan_cases as SC
from tests import sfm_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hm():
    return S.load_sfm_hostmath()


def _device_graph(a, num_src=10, params=(5.0, 1.0, 10.0)):
    """The three launches on the arrays -> (q, index, value, count, n, depth_min, depth_max) as host arrays"""
    q = sfm.pair_scores(a["centres"], a["points"], a["pt_ptr"], a["pt_views"], *params, device=DEV)
    index, value, count = sfm.select_sources(q, num_src)
    n, lo, hi = sfm.depth_ranges(a["rt"], a["points"], a["view_ptr"], a["view_pts"], device=DEV)
    return tuple(t.cpu().numpy() for t in (q, index, value, count, n, lo, hi))


def _host_graph(hm, a, num_src=10, params=(5.0, 1.0, 10.0)):
    q = S.pair_scores_host(hm, a, *params)
    return (q,) + S.select_host(hm, q, num_src) + S.depth_ranges_host(hm, a)


NAMES = ("q", "src_index", "src_q", "src_count", "n", "depth_min", "depth_max")


def _compare(hm, a, num_src=10, params=(5.0, 1.0, 10.0), what=""):
    got, again, want = _device_graph(a, num_src, params), _device_graph(a, num_src, params), _host_graph(hm, a, num_src, params)
    for g, g2, w, name in zip(got, again, want, NAMES):
        S.assert_bytes(g, w, (what, name))
        S.assert_bytes(g2, g, (what, name, "second run"))
    return got


# ---- views and tracks ---------------------------------------------------------------------------------------------------------------

def test_two_views(hm):
    got = _compare(hm, S.two_view_case(), what="V=2")
    assert got[0][0, 1] == got[0][1, 0] > 0 and got[0][0, 0] == got[0][1, 1] == 0
    assert list(got[1][:, 0]) == [1, 0] and list(got[3]) == [1, 1] and (got[1][:, 1:] == -1).all()


def test_a_model_without_points_and_one_without_pairs(hm):
    centres = S.ring_centres(3)
    none = S.arrays_from(centres, np.zeros((0, 3)), S.rows_at(centres), [], [])
    got = _compare(hm, none, what="P=0")
    assert (got[0] == 0).all() and (got[3] == 0).all() and (got[4] == 0).all() and np.isnan(got[5]).all()
    lone = S.arrays_from(centres, [[0.0, 0.1, 0.2], [0.3, 0.0, 0.1]], S.rows_at(centres), [0, 2], [0, 1])      # tracks of 1 only
    got = _compare(hm, lone, what="no pairs")
    assert (got[0] == 0).all() and list(got[4]) == [1, 0, 1] and got[5][0] == got[6][0] > 0


def test_tracks_of_1_2_64_65_300_and_a_view_without_observations(hm):
    a, lengths = S.track_case()
    assert sorted(set(lengths)) == list(S.TRACK_LENGTHS) and a["view_ptr"][-1] == a["view_ptr"][-2]
    got = _compare(hm, a, what="tracks")
    q = got[0]
    assert (q == q.T).all() and (np.diag(q) == 0).all() and (q[-1] == 0).all() and got[3][-1] == 0 and got[4][-1] == 0
    assert np.isnan(got[5][-1]) and np.isnan(got[6][-1]) and (got[1][-1] == -1).all()
    # every pair of every track got its term: the pairs with a positive score are pairs of views that share a point
    nc = S.common_counts(a)
    assert ((q > 0) <= (nc > 0)).all() and (q > 0).sum() > 20000              # (a term is 0 beyond some 73 degrees)


def test_random_model_through_view_graph(hm, tmp_path):
    raw = S.synthetic_model(V=70, P=3000, seed=21, rings=3, dropout=0.4, repeat=0.1, orphans=0.05, id_step=2)
    S.write_binary(raw, str(tmp_path))
    model = sfm.read_sfm_model(str(tmp_path))
    a = S.arrays_of(model)
    want = S.graph_host(hm, a, num_src=10)
    got, again = sfm.view_graph(model, device=DEV), sfm.view_graph(model, device=DEV)
    for k in ("q", "src_index", "src_q", "src_count", "n_obs", "depth_min", "depth_max", "score"):
        S.assert_bytes(got[k], want[k], k)
        S.assert_bytes(again[k], got[k], (k, "second run"))
    assert got["pairs"] == want["pairs"] and got["pair_scores"] == want["pair_scores"] and len(got["pairs"]) == 70
    assert (got["score"] * S.TWO32 == got["q"]).all() and got["n_obs"].min() > 50
    _compare(hm, a, what="random")


# ---- the term ---------------------------------------------------------------------------------------------------------------------------

def test_term_edges(hm):
    a = S.term_case()
    q = _compare(hm, a, what="term")[0]
    nc = S.common_counts(a)
    assert nc[0, 4] == 3                                                     # point 2, seen twice by both, counts once
    one = S.terms_host(hm, a["centres"][[0]], a["centres"][[1]], a["points"][[0]])
    assert one["theta"][0] == 0.0 and q[0, 1] == 2 * int(one["qterm"][0])    # points 0 and 2: the same centre, theta = 0 on both
    far = S.terms_host(hm, a["centres"][[0]], a["centres"][[2]], a["points"][[0]])
    assert abs(far["theta"][0] - 180.0) < 1e-12 and q[0, 2] == int(far["qterm"][0]) == 0
    assert q[0, 3] == int(S.terms_host(hm, a["centres"][[0]], a["centres"][[3]], a["points"][[0]])["qterm"][0])   # point 1 adds 0
    # theta exactly theta0 on the pair 4 / 5 over point 3: the term is 1, and q[4][5] holds 2^32 for it
    th = float(S.terms_host(hm, a["centres"][[4]], a["centres"][[5]], a["points"][[3]])["theta"][0])
    q2 = _compare(hm, a, params=(th, 1.0, 10.0), what="theta0")[0]
    rest = int(S.terms_host(hm, a["centres"][[4]], a["centres"][[5]], a["points"][[0]], th, 1.0, 10.0)["qterm"][0])
    assert q2[4, 5] == (1 << 32) + rest


# ---- the depth range ------------------------------------------------------------------------------------------------------------------

def test_depth_range_edges(hm):
    a, n = S.depth_case()
    got = _compare(hm, a, what="depth")
    assert np.array_equal(got[4], n)
    want = S.depth_ranges_numpy(a)
    for g, w in zip(got[4:], want):
        S.assert_bytes(g, w)
    assert got[5][6] == got[6][6] == 3.25 and got[5][0] == got[6][0] and np.isnan(got[5][9])
    assert got[5][8] != got[6][8] and (np.float64(got[5][8]).view(np.uint64) >> 8) == (np.float64(got[6][8]).view(np.uint64) >> 8)


# ---- source selection -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,levels,density", [(65, None, 0.5), (130, 3, 0.5), (130, None, 0.04), (3, 2, 1.0)])
def test_selection(hm, V, levels, density):
    q = S.select_matrix(V, seed=V, density=density, levels=levels)
    dq = torch.from_numpy(q).to(DEV)
    for num_src in (1, 10, 64):
        got, again = sfm.select_sources(dq, num_src), sfm.select_sources(dq, num_src)
        want = S.select_host(hm, q, num_src)
        for g, g2, w, name in zip(got, again, want, ("index", "value", "count")):
            S.assert_bytes(g.cpu().numpy(), w, (V, num_src, name))
            assert torch.equal(g, g2)
        count = want[2]
        positives = (q > 0).sum(1)
        assert np.array_equal(count, np.minimum(positives, num_src))
    if levels is not None and V > 3:
        index, value, _ = S.select_host(hm, q, 10)
        ties = (value[:, :-1] == value[:, 1:]) & (value[:, 1:] > 0)
        assert ties.sum() > V and (index[:, :-1][ties] < index[:, 1:][ties]).all()      # equal scores: by index
    if density < 0.1:
        assert (want[2] < 64).all() and (want[2] < 10).any()                            # num_src beyond the positive partners


# ---- one scan, end to end ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(shipped_cfg, checkpoint):
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    return m.to(DEV).eval()


def _colmap_text_model(sc, path, seed=0):
    """The scan's cameras and a sparse cloud on the plane they look at, written as a COLMAP text model -> the raw model"""
    rng = np.random.RandomState(seed)
    V, H, W = sc["images"].shape[:3]
    K = sc["Ks"].astype(np.float64).copy()
    K[:, :2] *= 4.0
    E = sc["Es"].astype(np.float64)
    n, c = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0]), 650.0       # the plane of synthetic_scene
    pts = []
    for v in range(V):                                                         # points: pixels of every view, on the plane
        R, t = E[v, :3, :3], E[v, :3, 3]
        uv = np.stack([rng.rand(60) * W, rng.rand(60) * H, np.ones(60)])
        rays = np.linalg.inv(K[v]) @ uv
        nr = n @ R.T
        d = (c + nr @ t) / (nr @ rays)
        pts.append((R.T @ (rays * d - t[:, None])).T)
    pts = np.concatenate(pts)
    images = []
    for v in range(V):
        R, t = E[v, :3, :3], E[v, :3, 3]
        cam = pts @ R.T + t
        u, w = K[v, 0, 0] * cam[:, 0] / cam[:, 2] + K[v, 0, 2], K[v, 1, 1] * cam[:, 1] / cam[:, 2] + K[v, 1, 2]
        seen = np.nonzero((cam[:, 2] > 0) & (u >= 0) & (u < W) & (w >= 0) & (w < H))[0]
        rows = np.stack([u[seen], w[seen], seen + 1.0], 1)
        images.append((v + 1, S.quaternion_of(R), t, v + 1, "%08d.png" % v, rows))
    raw = dict(cameras={v + 1: (1, W, H, [K[v, 0, 0], K[v, 1, 1], K[v, 0, 2], K[v, 1, 2]]) for v in range(V)}, images=images,
               points=[(p + 1, pts[p], (128, 128, 128), 0.5, []) for p in range(len(pts))])
    S.write_text(raw, path)
    return raw


def test_scan_from_a_text_model_through_reconstruct_scan(model, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    V, H, W = 7, 128, 192
    sc = SC.synthetic_scan(V, H, W, seed=4)
    mdir, idir = str(tmp_path / "sparse"), str(tmp_path / "images")
    _colmap_text_model(sc, mdir)
    os.makedirs(idir)
    for v in range(V):
        Image.fromarray(sc["images"][v]).save(os.path.join(idir, "%08d.png" % v))
    got = sfm.scan_from_sfm(mdir, idir, num_src=4, device=DEV)
    graph = sfm.view_graph(sfm.read_sfm_model(mdir), num_src=4, device=DEV)
    assert got["pairs"] == graph["pairs"] and len(got["pairs"]) == V and got["dropped_views"] == []
    assert got["view_ids"] == list(range(1, V + 1)) and np.array_equal(np.stack(got["images"]), sc["images"])
    assert np.abs(got["Ks"] - sc["Ks"]).max() < 1e-4 and np.abs(got["Es"] - sc["Es"]).max() < 1e-3
    lo, hi = np.array(got["depth_ranges"]).T
    assert (lo > 0).all() and (lo < hi).all()
    res = scan.reconstruct_scan(model, got["images"], got["Ks"], got["Es"], got["depth_ranges"], got["pairs"], conf=0.05,
                                thres_view=1, nviews=5, depth_range_kind="min_max", short_sources="fewer_views", max_h=H, max_w=W)
    n = len(res["points"])
    print("reconstruct_scan from a COLMAP text model: %d points of %d pixels, sources per view %s"
          % (n, V * H * W, [len(s) for _, s in got["pairs"]]))
    assert 0 < n < V * H * W and [(int(r), list(s)) for r, s in res.scan["pairs"]] == graph["pairs"]
