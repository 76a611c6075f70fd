"""The scenes of tests/warp_exact_cases.py are what they claim to be -- exact in fp32, and holding the edge each is named
after, counted from the taps -- and the fp64 reference agrees with the oracle's aggregate_views.  CPU only: a later edit
of a scene cannot hollow out the GPU tests that stand on it."""
import pytest
import torch

from oracle import mvs4_oracle as O
from tests import warp_exact_cases as WX

D_ALL = (3, 4, 8, 12)


def taps_of(name, D=4):
    sc = WX.scene(name, D)
    return sc, WX.scene_taps(sc)


@pytest.mark.parametrize("name", sorted(WX.SCENES))
@pytest.mark.parametrize("D", D_ALL)
def test_positions_are_exact_in_fp32(name, D):
    """op by op in torch fp32 == fp64, bit for bit after conversion (after make_taps' clamp: see the module docstring for the
    pz == 0 samples of bad_depth); so are the corners and the weights"""
    sc = WX.scene(name, D)
    s32 = WX.positions(sc.rt, sc.hypo, sc.Hs, sc.Ws, torch.float32)
    s64 = WX.positions(sc.rt, sc.hypo, sc.Hs, sc.Ws, torch.float64)
    for a, b, size in zip(s32, s64, (sc.Ws, sc.Hs)):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(WX.clamp_position(a, size).double(), WX.clamp_position(b, size))
        if name != "bad_depth":
            assert torch.equal(a.double(), b) and b.abs().max() < 2 ** 8
    t32, t64 = WX.make_taps(*s32, sc.Hs, sc.Ws), WX.make_taps(*s64, sc.Hs, sc.Ws)
    assert torch.equal(t32.x0, t64.x0) and torch.equal(t32.y0, t64.y0) and torch.equal(t32.mask, t64.mask)
    for a, b in zip(t32.wgt, t64.wgt):
        assert torch.equal(a.double(), b)


def test_scene_shapes_and_cameras():
    for name in WX.SCENES:
        sc = WX.scene(name, 4)
        assert (sc.Hs - 1) & (sc.Hs - 2) == 0 and (sc.Ws - 1) & (sc.Ws - 2) == 0
        assert sc.NV in (2, 3) and (sc.h, sc.w) in ((9, 23), (12, 70), (16, 16))
        assert tuple(sc.rt.shape) == (sc.B, sc.NV, 12) and tuple(sc.hypo.shape) == (sc.B, 4, sc.h, sc.w)
        assert (sc.rt[:, :, 6:8] == 0).all() and (sc.rt[:, :, 8] == 1).all()
        assert torch.equal(sc.rt[:, :, :6] * 2, (sc.rt[:, :, :6] * 2).round()) and torch.equal(sc.rt[:, :, 9:11] * 4, (sc.rt[:, :, 9:11] * 4).round())
        if name != "bad_depth":
            assert (sc.rt[:, :, 11] == 0).all()
            assert all(v in (1.0, 2.0, 4.0, 8.0) for v in sc.hypo.unique().tolist())
    for name in ("shift", "border", "tile_corner"):
        sc = WX.scene(name, 4)
        assert sc.B == 2 and not torch.equal(sc.rt[0], sc.rt[1])
    # every configuration the kernels distinguish is there, and the three heavy scenes run on all of them
    cfgs = {(c.C, c.G, c.D, c.group, c.fuse) for c in WX.CONFIGS}
    assert {(8, 4, 4, True, True), (8, 8, 8, True, True), (8, 4, 4, True, False), (8, 4, 12, True, True), (16, 4, 4, True, True),
            (32, 8, 8, True, True), (64, 8, 8, True, True), (64, 4, 4, True, True), (16, 16, 4, False, True)} <= cfgs
    assert any(c.D == 3 for c in WX.CONFIGS) and any(c.C == 64 and not c.group for c in WX.CONFIGS)
    for name in WX.SCENES:
        assert sum(1 for s, _ in WX.CASES if s == name) >= (len(WX.CONFIGS) if name in WX.ON_ALL else 2)


def test_shift_is_interior_and_fractional():
    sc, tp = taps_of("shift")
    assert (tp.mask == 15).all()
    assert not WX.windows(sc, "row").outside and not WX.windows(sc, "tile").outside      # (the scaling test relies on it)


def test_integer_masks():
    sc, tp = taps_of("integer")
    assert (tp.mask == 1).all()
    assert (tp.x0 == sc.Ws - 1).any() and (tp.y0 == sc.Hs - 1).any()


def test_border_edges():
    sc, tp = taps_of("border")
    sx, sy = WX.positions(sc.rt, sc.hypo, sc.Hs, sc.Ws, torch.float64)
    assert sx.min() <= -1.5 and sx.max() >= sc.Ws + 0.5 and sy.min() <= -1.5 and sy.max() >= sc.Hs + 0.5
    for x0 in (-2, -1, sc.Ws - 1, sc.Ws):
        assert (tp.x0 == x0).any(), x0
    for y0 in (-2, -1, sc.Hs - 1, sc.Hs):
        assert (tp.y0 == y0).any(), y0
    # the single-tap masks a padded edge can produce: (edge, mask) with nw = 1, ne = 2, sw = 4, se = 8
    wx1 = sx - sx.floor()
    wy1 = sy - sy.floor()
    left, right = tp.x0 == -1, (tp.x0 == sc.Ws - 1) & (wx1 > 0)
    top, bottom = tp.y0 == -1, (tp.y0 == sc.Hs - 1) & (wy1 > 0)
    for edge, masks in ((left, (2, 8)), (right, (1, 4)), (top, (4, 8)), (bottom, (1, 2))):
        for m in masks:
            assert (edge & (tp.mask == m)).any(), m
    # all four map corners carry weight
    n = WX.contributions(sc)
    for yy in (0, sc.Hs - 1):
        for xx in (0, sc.Ws - 1):
            assert n[:, :, yy, xx].sum() > 0, (yy, xx)


def test_tile_corner_records():
    sc, tp = taps_of("tile_corner")
    k = WX.touched_tiles(sc)
    for want in (4, 2, 1):
        assert (k == want).any(), want
    tx0, tx1 = tp.xs[0] // 32, tp.xs[1] // 32
    ty0, ty1 = tp.ys[0] // 16, tp.ys[2] // 16
    full = tp.mask == 15
    assert (full & (tx0 != tx1) & (ty0 == ty1)).any() and (full & (tx0 == tx1) & (ty0 != ty1)).any()
    assert (full & (tx0 != tx1) & (ty0 != ty1)).any()
    assert -(-sc.Ws // 32) == 3 and -(-sc.Hs // 16) == 3          # with a ragged column and row of tiles, one texel wide
    n = WX.contributions(sc)
    assert n[:, :, :, 64].sum() > 0 and n[:, :, 32, :].sum() > 0


def test_minify_shares_footprints():
    sc, tp = taps_of("minify")
    key = (tp.y0 * 1000 + tp.x0)[0, 0, 0]
    assert key.unique().numel() < key.numel()


@pytest.mark.parametrize("D", D_ALL)
def test_collapse_is_one_footprint(D):
    sc, tp = taps_of("collapse", D)
    for b in range(sc.B):
        for v in range(sc.NV):
            assert tp.x0[b, v].unique().numel() == 1 and tp.y0[b, v].unique().numel() == 1
    n = WX.contributions(sc)
    assert set(n.unique().tolist()) == {0, sc.h * sc.w * D}
    assert (WX.touched_tiles(sc)[0, 1] == 4).all()
    # the fixed-point counters hold it: h * w * D contributions of less than 2^37 units stay far below 2^63, and a single one
    # below the 2^51 of fix_cvt
    assert sc.h * sc.w * D * 2 ** 37 < 2 ** 62


def lanes_outside(sc, kind):
    return [rec[5] for rec in WX.windows(sc, kind).outside]


def test_transpose_leaves_the_window():
    sc = WX.scene("transpose", 4)
    assert max(lanes_outside(sc, "row")) > WX.QUEUE_DIRECT
    assert max(lanes_outside(sc, "tile")) > WX.QUEUE_DIRECT


@pytest.mark.parametrize("D", (4, 12))
def test_stragglers_stay_direct(D):
    sc = WX.scene("stragglers", D)
    for kind in ("row", "tile"):
        lanes = lanes_outside(sc, kind)
        assert lanes and 1 <= min(lanes) and max(lanes) <= WX.QUEUE_DIRECT, (kind, sorted(set(lanes)))


def test_window_edge_taps():
    sc = WX.scene("window_edge", 4)
    for kind, (wx, wy) in (("row", WX.ROW_WIN), ("tile", WX.TILE_WIN)):
        edge = WX.windows(sc, kind).edge
        assert any(ax == wx - 1 and 0 <= ay < wy for ax, ay in edge), kind
        assert any(ax == wx and 0 <= ay < wy for ax, ay in edge), kind
        assert any(ay == wy - 1 and 0 <= ax < wx for ax, ay in edge), kind
        assert any(ay == wy and 0 <= ax < wx for ax, ay in edge), kind


def test_empty_view_has_no_weighted_tap():
    sc, tp = taps_of("empty_view")
    v = sc.facts["empty"]
    assert (tp.mask[:, v] == 0).all() and (tp.mask[:, 1 - v] != 0).any()
    assert WX.contributions(sc)[v].sum() == 0
    for kind in ("row", "tile"):
        org = WX.windows(sc, kind).origin
        assert (org[:, :, v] == WX.EMPTY).all() and (org[:, :, 1 - v] != WX.EMPTY).all()


@pytest.mark.parametrize("D", D_ALL)
def test_bad_depth_counts(D):
    sc, tp = taps_of("bad_depth", D)
    assert int(sc.hypo.isnan().sum()) * sc.NV == sc.facts["nan"]
    pz = sc.hypo.unsqueeze(1) + sc.rt[:, :, 11].view(sc.B, sc.NV, 1, 1, 1)
    assert int((pz == 0).sum()) == sc.facts["pz_zero"]
    assert set(pz[~pz.isnan()].unique().tolist()) == {-1.0, 0.0, 1.0, 2.0, 4.0, 8.0}
    # pz == 0 with px == 0: the x position is 0 (three such samples leave the map in y, the fourth sits on texel (0, 0));
    # NaN depths sample zeros
    sx, sy = WX.positions(sc.rt, sc.hypo, sc.Hs, sc.Ws, torch.float64)
    assert (sx[0, 0, 0, 0:4, 4] == 0).all() and sy[0, 0, 0, 3, 4] == 0 and tp.mask[0, 0, 0, 3, 4] == 1
    assert (tp.mask[0, 0, 0, 0:3, 4] == 0).all()
    assert (tp.mask[sc.hypo.isnan().unsqueeze(1).expand_as(tp.mask)] == 0).all()


@pytest.mark.parametrize("name", ("shift", "border"))
@pytest.mark.parametrize("cfg", ("c8g4d4", "c8g4d4nf", "sq16d4", "c16g4d3nf"))
def test_reference_agrees_with_oracle(name, cfg):
    """aggregate (explicit taps, rt itself) against oracle.aggregate_views (grid_sample, projection matrices composing to the
    same rt with an identity reference camera) in float64: value and all feature gradients to 1e-12 of the maximum"""
    sc, c, ref, src, gout, (out, wsum, g_ref, g_src) = WX.reference(name, cfg)
    pm = torch.zeros(sc.B, sc.NV + 1, 2, 4, 4, dtype=torch.float64)
    pm[:, :, :] = torch.eye(4, dtype=torch.float64)
    pm[:, 1:, 0, :3, :3] = sc.rt[:, :, :9].double().view(sc.B, sc.NV, 3, 3)
    pm[:, 1:, 0, :3, 3] = sc.rt[:, :, 9:].double()
    feats = [ref.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)]
    feats += [src[v].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for v in range(sc.NV)]
    cor = O.aggregate_views(feats, pm, sc.hypo.double(), c.group, c.G, attn_temp=WX.ATTN_TEMP, attn_fuse_d=c.fuse)
    cor.backward(gout.double().permute(0, 4, 1, 2, 3))
    want = cor.detach().permute(0, 2, 3, 4, 1)
    assert (out - want).abs().max() <= 1e-12 * want.abs().max()
    grads = [feats[0].grad.permute(0, 2, 3, 1)] + [f.grad.permute(0, 2, 3, 1) for f in feats[1:]]
    scale = max(g.abs().max() for g in grads)
    assert (g_ref - grads[0]).abs().max() <= 1e-12 * scale
    for v in range(sc.NV):
        assert (g_src[v] - grads[v + 1]).abs().max() <= 1e-12 * scale


def test_bound_and_kernel_names():
    c = WX.CONFIG["c8g4d4"]
    # make_fix_scale's comment, by hand: cormax = 9, dcor = 2 (1 + 2*4*5*9/2) = 362, bound = 362 * 3 / 2
    assert WX.fix_bound(2.0, 3.0, 1.0, c) == 543.0
    assert WX.fix_bound(2.0, 1.0, 3.0, WX.CONFIG["sq16d4"]) == 4 * 3 * 2.0 * (1 + 2 * 16 * 5 * 36 / 2)
    assert WX.first_pass_kernel(c, "atomic") == "warp_agg_bwd_tile_kernel<4, true, 4, 4>"
    assert WX.first_pass_kernel(c, "sorted") == "warp_agg_bwd_kernel<8, 4, true, 8, true>"
    assert WX.first_pass_kernel(WX.CONFIG["c8g4d12"], "gather") == "warp_agg_bwd_kernel<8, 4, true, 16>"
    assert WX.first_pass_kernel(WX.CONFIG["sq64d3"], "atomic") == "warp_agg_bwd_kernel<64, 64, false, 8>"
