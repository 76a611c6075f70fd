"""Cloud-to-cloud nearest distances and scan scores on the GPU (``fusion.nearest_distances`` / ``CloudGrid`` / ``score_clouds``:
mvster_cloud_grid_build, mvster_cloud_nn_query, mvster_cloud_score): every output byte for byte against
the host brute force of mvster_amd/csrc/nn_math.h on every case of tests/cloud_nn_cases.py, at four cell sizes and two table
sizes, independent of the run; the scores' counts exact and their sums against NumPy's."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mvster_amd import _lib, fusion
from tests import cloud_nn_cases as N
from tests import fusion_scene_cases as C

DEV = "cuda:0"
COMPILERS = ("g++", "clang++")              # ROCm's clang++ as a host-only compiler where there is no g++


def dev(a):
    return torch.from_numpy(a).to(DEV)


def to_numpy(out):
    assert set(out) == set(N.KEYS) | {"dropped_query", "dropped_target"}
    return {k: (t.cpu().numpy() if torch.is_tensor(t) else t) for k, t in out.items()}


def nn_gpu(query, target, max_dist, cell=None, **kw):
    """fusion.nearest_distances on NumPy arrays -> dict of NumPy arrays."""
    return to_numpy(fusion.nearest_distances(dev(query), dev(target), max_dist, cell, **kw))


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_case_equals_the_host_brute_force_bit_for_bit(name, which):
    q, t, md = N.cases()[name]
    cell = N.cell_values(md)[which]
    want = N.host_case(name, cell, COMPILERS)
    got = nn_gpu(q, t, md, cell)
    found = got["index"] >= 0
    print("nn %s cell=%.5g: %d -> %d, %d found, %d dropped + %d, max dist %.6g" % (
        name, cell, len(q), len(t), found.sum(), got["dropped_query"], got["dropped_target"],
        got["dist"][found].max() if found.any() else float("nan")))
    N.assert_same(got, want, (name, cell))
    N.assert_same(nn_gpu(q, t, md, cell, table_slots=8 * fusion.thin_slots(len(t))), want, (name, cell, "8 x the slots"))
    if which == 1:                                                           # the default cell is that one
        N.assert_same(nn_gpu(q, t, md), want, (name, "default cell"))


@pytest.mark.parametrize("name", ("random", "one_cell", "ties", "invalid"))
def test_two_runs_and_a_reused_grid_give_the_same_bytes(name):
    q, t, md = N.cases()[name]
    cell = N.default_cell(md)
    want = N.host_case(name, cell, COMPILERS)
    qd, td = dev(q), dev(t)
    tg, qg = fusion.CloudGrid(td, cell), fusion.CloudGrid(qd, cell)
    assert (tg.dropped, qg.dropped, len(tg), len(qg)) == (want["dropped_target"], want["dropped_query"], len(t), len(q))
    for query, target in ((qd, td), (qd, tg), (qg, tg), (qg, td), (qd, tg)):
        N.assert_same(to_numpy(fusion.nearest_distances(query, target, md)), want, name)
    with pytest.raises(RuntimeError, match="has cell"):
        fusion.nearest_distances(qd, tg, md, cell=N.cell_values(md)[2])


def test_bad_arguments_are_refused_on_the_host_before_any_launch():
    q, t, md = N.cases()["odd"]
    qd, td = dev(q), dev(t)
    with pytest.raises(RuntimeError, match="table_slots"):
        fusion.nearest_distances(qd, td, md, table_slots=512)               # below 2 * 259
    with pytest.raises(RuntimeError, match="cell must be >= max_dist / 15"):
        fusion.nearest_distances(qd, fusion.CloudGrid(td, md / 16), md)
    # and below the Python checks, at the C ABI: MVSTER_ERR_SHAPE, the outputs untouched
    lib = _lib.load()
    g = fusion.CloudGrid(td, N.default_cell(md))
    out = torch.full((len(q) * 4,), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for max_dist, cell, slots in ((md, md / 16, g.slots), (0.0, g.cell, g.slots), (md, float("inf"), g.slots), (md, g.cell, g.slots - 1),
                                  (md, g.cell, 32)):
        rc = lib.mvster_cloud_nn_query(g.records.data_ptr(), g.cell_of_point.data_ptr(), g.starts.data_ptr(), len(q), g.keys.data_ptr(),
                                       g.cell_of_slot.data_ptr(), slots, g.starts.data_ptr(), g.records.data_ptr(), g.ncells,
                                       g.records.shape[0], max_dist, cell, out.data_ptr(), out.data_ptr(), out.data_ptr(), stream)
        assert rc == _lib.ERR_SHAPE, (max_dist, cell, slots)
    assert lib.mvster_cloud_score_slots(0) == _lib.ERR_SHAPE and lib.mvster_cloud_score_slots(5000) == 2
    assert lib.mvster_cloud_score(out.data_ptr(), len(q), md, 2 * md, out.data_ptr(), out.data_ptr(), stream) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def check_scores(got, q, t, md, tau, cell):
    """Counts exact, sums to 1e-12 relative (float32 inputs, n <= 20 000, another order of summation), the rest the same fp64
    formulas on the exact counts and the returned sums."""
    ways = (N.host_pair(q, t, md, cell, COMPILERS), N.host_pair(t, q, md, cell, COMPILERS))
    want = N.scores_numpy(*ways, md, tau)
    assert set(got) == set(want) | {"dropped_pred", "dropped_gt"}
    assert (got["dropped_pred"], got["dropped_gt"]) == (ways[0]["dropped_query"], ways[0]["dropped_target"])
    for k in want:
        if k.endswith(("_valid", "_within", "_below_tau")):
            assert isinstance(got[k], int) and got[k] == want[k], (k, got[k], want[k])
    for k in ("pred_sum", "gt_sum"):
        print("score %s: %.17g against NumPy's %.17g" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    same = N.scores_from_counts(got, tau)
    for k in ("accuracy", "completeness", "overall") + (("precision", "recall", "fscore") if tau is not None else ()):
        assert got[k] == same[k] or (math.isnan(got[k]) and math.isnan(same[k])), (k, got[k], same[k])


@pytest.mark.parametrize("name,tau", [("random", 0.1), ("random", None), ("invalid", 0.5), ("one_cell", 0.02), ("m0", 0.1),
                                      ("q0", 0.1), ("all_invalid_target", 0.25), ("far_outside", 0.3)])
def test_score_clouds_counts_are_exact_and_sums_agree_with_numpy(name, tau):
    q, t, md = N.cases()[name]
    got = fusion.score_clouds(dev(q), dev(t), md, tau)
    check_scores(got, q, t, md, tau, N.default_cell(md))
    again = fusion.score_clouds(fusion.CloudGrid(dev(q), N.default_cell(md)), dev(t), md, tau)
    assert repr(again) == repr(got)                                          # two runs, a reused grid: the same bytes
    if name in ("m0", "all_invalid_target"):                                 # no valid gt point: recall is 0 / 0
        assert math.isnan(got["accuracy"]) and got["precision"] == 0.0 and math.isnan(got["recall"]) and math.isnan(got["fscore"])
    if name == "far_outside":                                                # valid points both ways, none within max_dist
        assert math.isnan(got["accuracy"]) and math.isnan(got["overall"]) and got["fscore"] == 0.0
    if name == "q0":
        assert math.isnan(got["accuracy"]) and math.isnan(got["precision"]) and math.isnan(got["fscore"])


def test_a_fused_scene_scored_against_itself():
    sc = C.hard_scene(61, 83, 5, "plain")
    res = fusion.fuse_scene(sc["depths"], sc["conf"], sc["images"], sc["Ks"], sc["Es"], sc["pairs"], C.CONF_THRES, C.THRES_VIEW,
                            device=DEV)
    p = res["points"]
    ok = p[torch.isfinite(p).all(1)]
    md = float((ok.max(0)[0] - ok.min(0)[0]).max()) / 24
    got = fusion.score_clouds(p, p, md, tau=md / 2)
    print("scene of %d points against itself: %r" % (len(p), got))
    assert len(p) > 10000 and got["pred_valid"] == got["gt_valid"] == len(p) - got["dropped_pred"] == got["pred_below_tau"]
    assert got["accuracy"] == 0.0 and got["completeness"] == 0.0 and got["overall"] == 0.0
    assert got["precision"] == 1.0 and got["recall"] == 1.0 and got["fscore"] == 1.0
    near = fusion.nearest_distances(p, p, md)
    first = N.nearest_numpy(p[:300].cpu().numpy(), p.cpu().numpy(), md, N.default_cell(md))     # duplicates: the smallest index
    assert np.array_equal(near["index"][:300].cpu().numpy(), first["index"]) and bool((near["dist2"][near["index"] >= 0] == 0).all())
