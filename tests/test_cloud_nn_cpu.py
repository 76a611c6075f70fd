"""Cloud-to-cloud nearest distances without a GPU: the host brute force of mvster_amd/csrc/nn_math.h
against the NumPy restatement bit for bit, the host grid search against the host brute force at four cell sizes (which proves
the ring bounds), what the case clouds claim, and the argument checks of the Python entry points."""
import numpy as np
import pytest
import torch

from mvster_amd import fusion
from tests import cloud_nn_cases as N


@pytest.fixture(scope="module")
def nhm():
    return N.load_nn_hostmath()


def test_cell_values_and_rings(nhm):
    for md in (N.MD, 5 * 2.0 ** -6, 0.3, 1.0, 7e-3):
        cells = N.cell_values(md)
        assert [bool(nhm.hm_nn_cell_ok(md, c)) for c in cells] == [True] * 4
        assert not nhm.hm_nn_cell_ok(md, float(np.nextafter(np.float32(cells[0]), np.float32(0))))
        rings = [nhm.hm_nn_rings(md, c) for c in cells]
        assert rings[0] in (16, 17) and rings[1:] == [5, 2, 2], rings
        assert fusion._check_max_dist_cell("x", md, None) == (N.f32(md), cells[1])
        for c in cells:
            assert fusion._check_max_dist_cell("x", md, c) == (N.f32(md), c)


def test_case_clouds_are_what_they_claim(nhm):
    cases = N.cases()
    assert tuple(cases) == N.CASE_NAMES
    assert all(len(q) <= 20000 and len(t) <= 20000 for q, t, _ in cases.values())
    g = N.default_cell(N.MD)
    # (a): the nearer target lies two cells away, the farther one in a neighbouring cell -- at the default and the smallest cell
    q, t, md = cases["ring_stop"]
    for pair, cell in ((0, g), (1, N.cell_values(md)[0])):
        want = N.host_case("ring_stop", cell)
        ci = np.floor(q[pair].astype(np.float64) / cell)
        shell = [int(np.abs(np.floor(t[2 * pair + j].astype(np.float64) / cell) - ci).max()) for j in (0, 1)]
        assert shell == [1, 2] and want["index"][pair] == 2 * pair + 1
        assert abs(want["dist"][pair] / cell - 1.1) < 1e-5
    # (b)
    assert N.host_case("at_max_dist", g)["index"].tolist() == [0] and N.host_case("at_max_dist", g)["dist"][0] == 5 * 2.0 ** -6
    below = N.host_case("below_max_dist", g)
    assert below["index"].tolist() == [-1] and np.isposinf(below["dist"]).all() and np.isposinf(below["dist2"]).all()
    # (c): the smallest index among equal d2, in different cells, inside one cell, and on duplicates
    q, t, md = cases["ties"]
    d2 = ((q[:, None].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(-1)
    assert [np.nonzero(row == row.min())[0].tolist() for row in d2] == [[1, 2, 3, 4], [6, 7, 8], [10, 11, 12]]
    for cell in N.cell_values(md):
        assert N.host_case("ties", cell)["index"].tolist() == [1, 6, 10]
    cells = np.floor(t.astype(np.float64) / g)
    assert len({tuple(c) for c in cells[1:5]}) == 3 and len({tuple(c) for c in cells[6:9]}) == 1
    # (e): queries and targets that are invalid at every cell, and some only at the small ones
    q, t, md = cases["invalid"]
    dropped = [N.host_case("invalid", c)["dropped_query"] for c in N.cell_values(md)]
    assert dropped == [28, 28, 22, 22] and np.isnan(N.host_case("invalid", g)["dist"]).sum() == 28
    allbad = N.host_case("all_invalid_target", g)
    assert allbad["dropped_target"] == 33 and (allbad["index"] == -1).all() and np.isposinf(allbad["dist"]).all()
    # (f): 5 000 targets in one cell of the default grid
    _, t, _ = cases["one_cell"]
    assert len({tuple(c) for c in np.floor(t[:5000].astype(np.float64) / g)}) == 1
    # (g): nothing within max_dist, every shell searched
    far = N.nearest_host(nhm, *cases["far_outside"][:2], N.MD, g, grid=True)
    assert (far["index"] == -1).all() and far["probes"] == 37 * 11 ** 3
    # (i): crowded and lonely queries, found and not found
    rnd = N.host_case("random", g)
    assert 150 < rnd["dropped_query"] < 260 and 50 < np.isposinf(rnd["dist"]).sum() < 1000
    assert (rnd["index"] >= 0).sum() > 18000 and len(np.unique(rnd["index"])) > 15000


@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_host_brute_force_equals_the_restatement(nhm, name):
    q, t, md = N.cases()[name]
    cells = N.cell_values(md) if name in ("invalid", "faces", "ties") else (N.default_cell(md),)
    for cell in cells:
        N.assert_same(N.host_case(name, cell), N.nearest_numpy(q, t, md, cell), (name, cell))


@pytest.mark.parametrize("which", range(4))
def test_host_grid_search_equals_the_host_brute_force(nhm, which):
    """The ring bounds: R shells are enough, and stopping after shell r once best_d2 <= (r cell)^2 (1 - 2^-20) loses nothing."""
    for name, (q, t, md) in N.cases().items():
        cell = N.cell_values(md)[which]
        got = N.nearest_host(nhm, q, t, md, cell, grid=True)
        N.assert_same(got, N.host_case(name, cell), (name, cell))


def test_scores_of_the_restatement_on_a_known_pair():
    a = np.array([[0, 0, 0], [1, 0, 0], [5, 0, 0], [np.nan, 0, 0]], np.float32)
    b = np.array([[0, 0, 0.25], [1, 0.5, 0]], np.float32)
    ab, ba = N.nearest_numpy(a, b, 1.0, 0.25), N.nearest_numpy(b, a, 1.0, 0.25)
    s = N.scores_numpy(ab, ba, 1.0, tau=0.3)
    assert (s["pred_valid"], s["pred_within"], s["pred_below_tau"], s["gt_valid"], s["gt_within"], s["gt_below_tau"]) == (3, 2, 1, 2, 2, 1)
    assert s["accuracy"] == 0.375 and s["completeness"] == 0.375 and s["overall"] == 0.375
    assert s["precision"] == 1 / 3 and s["recall"] == 0.5 and s["fscore"] == 2 * (1 / 3) * 0.5 / (1 / 3 + 0.5)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------

A, B = torch.zeros(5, 3), torch.zeros(7, 3)


@pytest.mark.parametrize("bad", [0, -0.2, float("nan"), float("inf"), 1e-60, 1e60, None, "abc"])
def test_a_bad_max_dist_is_rejected(bad):
    with pytest.raises(RuntimeError, match="nearest_distances: max_dist"):
        fusion.nearest_distances(A, B, bad)
    with pytest.raises(RuntimeError, match="score_clouds: max_dist"):
        fusion.score_clouds(A, B, bad)


def test_entry_points_check_their_arguments_before_the_gpu():
    for bad in (0, -1, float("nan"), float("inf"), "abc", 0.5 / 15.1, 1e-60):
        with pytest.raises(RuntimeError, match="nearest_distances: cell"):
            fusion.nearest_distances(A, B, 0.5, cell=bad)
        with pytest.raises(RuntimeError, match="score_clouds: cell"):
            fusion.score_clouds(A, B, 0.5, cell=bad)
    with pytest.raises(RuntimeError, match=r"cell must be >= max_dist / 15 = "):
        fusion.nearest_distances(A, B, 0.5, cell=0.033)
    for bad in (0, -0.1, float("nan"), 0.6, "abc"):
        with pytest.raises(RuntimeError, match="score_clouds: tau"):
            fusion.score_clouds(A, B, 0.5, tau=bad)
    with pytest.raises(RuntimeError, match=r"query must be \[M,3\] float32"):
        fusion.nearest_distances(A.double(), B, 0.5)
    with pytest.raises(RuntimeError, match=r"target must be \[M,3\] float32"):
        fusion.nearest_distances(A, torch.zeros(7, 4), 0.5)
    with pytest.raises(RuntimeError, match="query must be a torch tensor"):
        fusion.nearest_distances(A.numpy(), B, 0.5)
    with pytest.raises(RuntimeError, match=r"gt must be \[M,3\] float32"):
        fusion.score_clouds(A, B.half(), 0.5)
    with pytest.raises(RuntimeError, match=r"points must be \[M,3\] float32"):
        fusion.CloudGrid(torch.zeros(3), 0.1)
    with pytest.raises(RuntimeError, match="CloudGrid: cell"):
        fusion.CloudGrid(A, 0.0)
    for slots in (48, 63, 100, 32, 0, -64, 64.0, 1 << 31):                   # not a power of two, too small, not an int, too large
        with pytest.raises(RuntimeError, match="table_slots"):
            fusion.nearest_distances(A, torch.zeros(33, 3), 0.5, table_slots=slots)
        with pytest.raises(RuntimeError, match="table_slots"):
            fusion.CloudGrid(torch.zeros(33, 3), 0.1, table_slots=slots)
    for call in (lambda: fusion.nearest_distances(A, B, 0.5, cell=N.cell_values(0.5)[0], table_slots=64), lambda: fusion.score_clouds(A, B, 0.5, tau=0.5),
                 lambda: fusion.CloudGrid(A, 0.125)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # everything else is fine: only the device is not
            call()
    assert fusion.MAX_CLOUD_POINTS == 1 << 29
    assert "observability masks and ground plane are NOT applied" in fusion.score_clouds.__doc__
