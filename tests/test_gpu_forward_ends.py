"""The two ends of the eval forward without their glue launches: FPN conv0 reading the image planes itself, with the
projections and the first stage's hypotheses in the same launch (mvster_conv_narrow_pair_planes), and the last stage's
selection interpolating the coarse stages' confidence maps (mvster_deconv_select_riders).  Every comparison is the new
launch against the launches it replaces on the same inputs, bit for bit.  Needs an MI355X."""
import ctypes

import pytest
import torch

from mvster_amd import MVS4net, _lib, ops
from mvster_amd import conv_plan as cp
from mvster_amd import modules as M
from mvster_amd.graph import GraphedForward
from mvster_amd.synthetic import make_inputs, randomize_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), ctypes.c_void_p)


@pytest.fixture(scope="module")
def conv0_weights():
    """conv0[0] / conv0[1] in the kernels' layout: w1 [3,3,4,8] (the fourth input channel meets the pack's zero), w2 [3,3,8,8],
    scale / shift [8] each."""
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)                                  # noqa: E731
    return tuple(t.to(DEV).contiguous() for t in (0.3 * r(3, 3, 4, 8), 1 + 0.2 * r(8), 0.3 * r(8), 0.2 * r(3, 3, 8, 8), 1 + 0.2 * r(8),
                                                   0.3 * r(8)))


def _pair_packed(imgs, wts, wpc):
    w1, sc1, sh1, w2, sc2, sh2 = wts
    B, _, H, W = imgs[0].shape
    x = ops.pack_images(imgs)
    out = torch.empty(len(imgs) * B, 1, H, W, 8, device=DEV)
    _lib.check(_lib.load().mvster_conv_narrow_pair(x.data_ptr(), w1.data_ptr(), sc1.data_ptr(), sh1.data_ptr(), w2.data_ptr(),
                                                   sc2.data_ptr(), sh2.data_ptr(), out.data_ptr(), len(imgs) * B, H, W, 1, 1, wpc,
                                                   ops._stream()), "pair")
    return out


def _pair_planes(imgs, wts, wpc, side=None):
    """-> (out, rt, hypo); side = (pms, dv, D, h, w, inverse) or None."""
    w1, sc1, sh1, w2, sc2, sh2 = wts
    B, _, H, W = imgs[0].shape
    N = len(imgs)
    out = torch.full((N * B, 1, H, W, 8), float("nan"), device=DEV)
    rt = hypo = None
    tail = (None, 0, None, None, 0, None, 0, 0, 0, 0)
    if side is not None:
        pms, dv, D, h, w, inverse = side
        rt = torch.full((len(pms), B, N - 1, 12), float("nan"), device=DEV)
        hypo = torch.full((B, D, h, w), float("nan"), device=DEV)
        tail = (_ptrs(pms), len(pms), rt.data_ptr(), dv.data_ptr(), dv.shape[1], hypo.data_ptr(), D, h, w, int(inverse))
    _lib.check(_lib.load().mvster_conv_narrow_pair_planes(_ptrs(imgs), N, B, H, W, w1.data_ptr(), sc1.data_ptr(), sh1.data_ptr(),
                                                          w2.data_ptr(), sc2.data_ptr(), sh2.data_ptr(), out.data_ptr(), 1, 1, wpc,
                                                          *tail, ops._stream()), "pair_planes")
    assert _lib.last_kernel() == "conv_narrow_pair_kernel<0, true>"
    return out, rt, hypo


# one 14 x 64 tile exactly; ragged last tile row and column; batch stride inside a view + three column tiles with a 1-pixel
# last one; smaller than one tile in both axes
PAIR_SHAPES = [(1, 1, 14, 64), (2, 1, 30, 70), (3, 2, 15, 129), (1, 1, 3, 5)]


@pytest.mark.parametrize("N,B,H,W", PAIR_SHAPES)
def test_planar_pair_equals_pack_then_pair(conv0_weights, N, B, H, W):
    """conv_narrow_pair_kernel's planar form on the views' [B,3,H,W] planes against pack_images + the RGB0 form (the C
    entries directly: no size rule reroutes the small maps), one and two workgroups per CU."""
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    imgs = [torch.randn(B, 3, H, W, generator=g).to(DEV) for _ in range(N)]         # (negative values included)
    for wpc in (1, 2):
        want = _pair_packed(imgs, conv0_weights, wpc)
        got, _, _ = _pair_planes(imgs, conv0_weights, wpc)
        assert want.abs().max() > 0 and torch.equal(got, want), (wpc, (got - want).abs().max().item())


def test_planar_pair_on_unaligned_views_of_one_buffer(conv0_weights):
    """The images as views into one flat buffer at element offsets that are no multiple of four (16 bytes): what
    ``GraphedForward(packed=True)`` hands the forward."""
    N, B, H, W = 3, 2, 15, 129
    n = B * 3 * H * W
    g = torch.Generator().manual_seed(5)
    flat = torch.randn(1 + N * (n + 3), generator=g).to(DEV)
    imgs = [flat[1 + k * (n + 3):1 + k * (n + 3) + n].view(B, 3, H, W) for k in range(N)]
    assert [im.data_ptr() % 16 for im in imgs] == [4, 8, 12] and all(im.is_contiguous() for im in imgs)
    want = _pair_packed(imgs, conv0_weights, 1)
    got, _, _ = _pair_planes(imgs, conv0_weights, 1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("inverse", [True, False])
def test_side_jobs_equal_the_prologue(conv0_weights, B, inverse):
    """rt and the first stage's hypotheses from the conv0 launch against ``ops.forward_prologue`` (and conv0 itself against the
    pack + pair launches beside them); 128 x 320: the hypotheses take two side workgroups."""
    N, H, W, D = 3, 128, 320, 8
    imgs, proj, dv = make_inputs(nviews=N, H=H, W=W, batch=B, seed=3 + B, device=DEV)
    pms = [proj["stage%d" % (s + 1)].to(DEV, torch.float32).contiguous() for s in range(4)]
    dv = dv.to(DEV)
    packed, rt_want, hypo_want = ops.forward_prologue(imgs, pms, dv, D, H // 8, W // 8, inverse)
    got, rt, hypo = _pair_planes(imgs, conv0_weights, 1, side=(pms, dv, D, H // 8, W // 8, inverse))
    assert torch.equal(rt, rt_want) and torch.equal(hypo, hypo_want)
    assert torch.isfinite(rt).all() and torch.isfinite(hypo).all()
    assert torch.equal(got, _pair_packed(imgs, conv0_weights, 1))


@pytest.mark.parametrize("B,size", [(1, (32, 48)), (2, (32, 48)), (1, (48, 80))])
@pytest.mark.parametrize("want_logits", [False, True])
def test_selection_with_riders(B, size, want_logits):
    """``fused_conv11_select`` with the three coarse maps as riders against the same call without them followed by
    ``ops.upsample_bilinear_multi``: the three up-sampled maps and every output of the selection.  D = 4, stage maps
    H/8, H/4, H/2 of the output size."""
    D, (H, W) = 4, size
    torch.manual_seed(H + B)
    m = M.reg2d(input_channel=4, base_channel=8)
    m.load_state_dict(randomize_state(m.state_dict(), seed=3, prob_gain=8.0))
    L = cp.Reg2dPlan(m.to(DEV).eval()).conv11
    t = torch.randn(B, D, H // 2, W // 2, 16, device=DEV)
    c0 = torch.randn(B, D, H, W, 8, device=DEV)
    hypo = (1.0 / (1.0 / 900 + 2e-5 * (torch.arange(D).view(1, D, 1, 1) + 0.1 * torch.rand(B, D, H, W)))).float().to(DEV)
    maps = [torch.rand(B, H // f, W // f, device=DEV) for f in (8, 4, 2)]
    want = cp.fused_conv11_select(L, t, c0, hypo, 1.0, True, want_logits)
    want_ups = ops.upsample_bilinear_multi(maps, H, W)
    got = cp.fused_conv11_select(L, t, c0, hypo, 1.0, True, want_logits, upsample=maps, up_size=(H, W))
    assert _lib.last_kernel().startswith("deconv_select_mfma_kernel<4, ")
    assert set(got) == set(want) | {"upsampled"} and ("logits" in got) == want_logits
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert len(got["upsampled"]) == 3
    for u, w_ in zip(got["upsampled"], want_ups):
        assert u.shape == (B, H, W) and torch.equal(u, w_)


def _leaves(out):
    for k, v in out.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                yield (k, kk), vv
        else:
            yield (k,), v


def _clone(out):
    return {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v.clone()) for k, v in out.items()}


def _assert_same(got, want):
    n = 0
    for path, t in _leaves(got):
        w_ = want[path[0]] if len(path) == 1 else want[path[0]][path[1]]
        assert t.shape == w_.shape and torch.equal(t, w_), path
        n += 1
    assert n == sum(1 for _ in _leaves(want))


class _EntryLog:
    """Names of the library's launching entries in call order (every forward-path entry is one launch)."""

    def __init__(self):
        self.lib = _lib.load()
        self.names = []

    def __enter__(self):
        self.orig = {}
        for name in _lib.SIGNATURES:
            if name in ("mvster_last_kernel", "mvster_build_flags"):
                continue
            fn = self.orig[name] = getattr(self.lib, name)

            def wrapped(*a, _fn=fn, _name=name):
                self.names.append(_name)
                return _fn(*a)
            setattr(self.lib, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():                                       # (the very objects that carry the argtypes)
            setattr(self.lib, name, fn)


# 3 x 64 x 128 (image sizes are multiples of 64): conv0 below the pair kernel's size rule -- the prologue stays, the up-sampling
# rides; 3 x 384 x 448: the pair kernel, so both glue launches go
@pytest.mark.parametrize("nviews,H,W,pair", [(3, 64, 128, False), (3, 384, 448, True)])
def test_whole_forward_equals_separate_launches(shipped_cfg, checkpoint, monkeypatch, nviews, H, W, pair):
    """Shipped configuration, golden checkpoint: every tensor of the output dict with the new launches equals the forward with
    ``merge_launches`` off -- eager, through ``GraphedForward`` replay (plain and with the inputs as views of one flat buffer)
    and through the model's own graph cache; the entry log shows that the new path ran, with two launches fewer than the
    merged launches it replaces (the same forward with the two new forms switched off)."""
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    m.to(DEV).eval()
    assert (nviews * H * W >= cp.NARROW_PAIR_MIN_PIXELS) == pair
    imgs, proj, dv = make_inputs(nviews=nviews, H=H, W=W, seed=41, device=DEV)
    a = (imgs, proj, dv)
    m.merge_launches = False
    want = _clone(m.forward_eager(*a))                                           # (the plans are built here: weight packing)
    m.merge_launches = True
    with monkeypatch.context() as mp:                                            # the merged launches these two replace
        mp.setattr(cp.FpnPlan, "conv0_planes", lambda self, imgs, side=None: None)
        mp.setattr(cp, "RIDER_DEPTHS", ())
        with _EntryLog() as before:
            _assert_same(m.forward_eager(*a), want)
    assert before.names[0] == "mvster_forward_prologue" and before.names[-1] == "mvster_upsample_bilinear_multi"
    assert ("mvster_conv_narrow_pair" in before.names) == pair
    with _EntryLog() as new:
        got = m.forward_eager(*a)
    _assert_same(got, want)
    names = set(new.names)
    assert new.names[-1] == "mvster_deconv_select_riders" and "mvster_upsample_bilinear_multi" not in names
    assert new.names.count("mvster_deconv_select_riders") == 1 and new.names.count("mvster_deconv_select") == 3
    if pair:
        assert new.names[0] == "mvster_conv_narrow_pair_planes" and "mvster_forward_prologue" not in names
        assert "mvster_pack_images" not in names and "mvster_conv_narrow_pair" not in names
    else:
        assert new.names[0] == "mvster_forward_prologue" and "mvster_conv_narrow_pair_planes" not in names
    # two launches fewer where conv0 takes the planes, one fewer (the up-sampling) where the prologue stays
    assert len(new.names) == len(before.names) - (2 if pair else 1), (len(new.names), len(before.names))
    for packed in (False, True):
        gf = GraphedForward(m, *a, packed=packed)
        _assert_same(gf(), want)
        _assert_same(gf(), want)
    for got in (m(*a), m(*a), m(*a)):                                             # eager, captured, replayed
        _assert_same(got, want)
