"""The weight-gradient case table (tests/wgrad_cases.py) checked without a GPU: its fp64 reference against the
definition and against autograd of the layers themselves, the conditions the exact comparison rests on, the kernel
instantiations it must name, and that every convolution of the network has a case."""
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import wgrad_cases as WC


def naive_dw(x, gy, kernel, stride, padding):
    """dW[co][ci][tap] = sum over output voxels o of gy[o][co] * x[o * s - p + tap][ci], voxel by voxel."""
    B, Di, Hi, Wi, CI = x.shape
    _, Do, Ho, Wo, CO = gy.shape
    dw = torch.zeros((CO, CI) + tuple(kernel), dtype=torch.float64)
    xd, gd = x.double(), gy.double()
    for b in range(B):
        for zo in range(Do):
            for yo in range(Ho):
                for xo in range(Wo):
                    for kz in range(kernel[0]):
                        for ky in range(kernel[1]):
                            for kx in range(kernel[2]):
                                iz = zo * stride[0] - padding[0] + kz
                                iy = yo * stride[1] - padding[1] + ky
                                ix = xo * stride[2] - padding[2] + kx
                                if 0 <= iz < Di and 0 <= iy < Hi and 0 <= ix < Wi:
                                    dw[:, :, kz, ky, kx] += torch.outer(gd[b, zo, yo, xo], xd[b, iz, iy, ix])
    return dw


def test_reference_equals_the_definition():
    g = torch.Generator().manual_seed(1)
    # strided, with keeps
    x, gy = torch.randn(2, 3, 5, 6, 5, generator=g), torch.randn(2, 2, 3, 3, 7, generator=g)
    want = naive_dw(x, gy, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    got = WC.reference_dw(x, gy, (3, 3, 3), (2, 2, 2), (1, 1, 1), co_keep=6, ci_keep=3)
    assert got.shape == (6, 3, 3, 3, 3)
    assert (got - want[:6, :3]).abs().max() <= 1e-12 * want.abs().max()
    # mirrored, with keeps
    x, gy = torch.randn(1, 2, 4, 5, 4, generator=g), torch.randn(1, 2, 4, 5, 6, generator=g)
    want = naive_dw(x, gy, (1, 3, 3), (1, 1, 1), (0, 1, 1)).flip(2, 3, 4).transpose(0, 1)
    got = WC.reference_dw(x, gy, (1, 3, 3), (1, 1, 1), (0, 1, 1), co_keep=5, ci_keep=1, mirrored=True)
    assert got.shape == (1, 5, 1, 3, 3)
    assert (got - want[:1, :5]).abs().max() <= 1e-12 * want.abs().max()


def cl(t):      # NCDHW -> NDHWC
    return t.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("kernel,stride", [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2))])
def test_transposed_form_is_conv_transpose_autograd(kernel, stride):
    """The form of layer_form("convT", ...) -- the operands' roles swapped -- is the weight gradient of F.conv_transpose3d."""
    g = torch.Generator().manual_seed(2)
    cin, cout = 16, 8
    form, CI, CO, k, s, p, co_keep, ci_keep = WC.layer_form("convT", cin, cout, kernel, stride)
    assert (form, CI, CO, co_keep, ci_keep) == ("transposed", 8, 16, 16, 8)
    x = torch.randn(2, cin, 2, 3, 4, generator=g, dtype=torch.float64)
    w = torch.randn((cin, cout) + kernel, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose3d(x, w, None, stride=s, padding=p, output_padding=tuple(si - 1 for si in s))
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    got = WC.reference_dw(cl(gy), cl(x), k, s, p, co_keep, ci_keep)
    assert got.shape == w.grad.shape
    assert (got - w.grad).abs().max() <= 1e-12 * w.grad.abs().max()


@pytest.mark.parametrize("cin,cout", [(16, 1), (64, 8)])
def test_mirrored_form_is_the_layers_own_gradient(cin, cout):
    """layer_form's mirrored call (narrow output side: the output gradient, padded to 4 / 8 channels, takes the x role)
    gives the layer's dW [cout, cin, k]."""
    g = torch.Generator().manual_seed(3)
    form, CI, CO, k, s, p, co_keep, ci_keep = WC.layer_form("conv", cin, cout, (1, 3, 3), (1, 1, 1))
    assert (form, CO, co_keep, ci_keep) == ("mirrored", cin, cin, cout) and CI == (4 if cout <= 4 else 8)
    x = torch.randn(1, cin, 2, 4, 5, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 1, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, w, None, padding=(0, 1, 1))
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    gyp = F.pad(cl(gy), (0, CI - cout))
    got = WC.reference_dw(gyp, cl(x), k, s, p, co_keep, ci_keep, mirrored=True)
    assert got.shape == w.grad.shape
    assert (got - w.grad).abs().max() <= 1e-12 * w.grad.abs().max()


def test_finish_reference_on_a_hand_made_slot():
    """finish_reference against the sentence it mirrors, on a packed slot small enough to write down: 3 taps, two per
    tile (cip 8), so the second group's upper half is a dead tap."""
    partial = torch.arange(2 * 2 * 16 * 16, dtype=torch.float32).reshape(2, 2, 16, 16)
    dw = WC.finish_reference(partial, 3, 8, 5, 7, False, True)
    assert dw.shape == (5, 7, 3) and not dw.isnan().any()
    for co, ci, tap in ((0, 0, 0), (4, 6, 1), (2, 3, 2)):
        g, col = tap // 2, (tap % 2) * 8 + ci
        assert dw[co, ci, 2 - tap] == partial[0, g, co, col].double() + partial[1, g, co, col].double()
    sw = WC.finish_reference(partial, 3, 8, 5, 7, True, False)
    assert torch.equal(sw, dw.flip(2).transpose(0, 1))


@pytest.mark.parametrize("c", WC.CASES, ids=WC.IDS)
def test_case_is_well_formed(c):
    Do, Ho, Wo = WC.out_size(c)
    assert min(Do, Ho, Wo) >= 1
    assert c.B * Do * Ho * Wo <= WC.P_MAX                      # what the exact comparison rests on
    assert max(c.B * c.D * c.H * c.W * c.CI, c.B * Do * Ho * Wo * c.CO) <= 1_500_000      # the suite stays quick
    assert 1 <= c.co_keep <= c.CO <= 80 and 1 <= c.ci_keep <= c.CI <= 64
    assert c.padding == tuple(k // 2 for k in c.kernel)
    assert c.form in ("plain", "transposed", "mirrored", "direct")
    if c.form == "transposed":
        # a ConvTranspose layer's output (the x role here) is `stride` times its input
        assert (c.D, c.H, c.W) == tuple(o * s for o, s in zip((Do, Ho, Wo), c.stride))
    if c.form == "mirrored":
        assert c.stride == (1, 1, 1) and c.CI <= 8 < c.CO and c.kernel != (1, 1, 1)
    x, gy = WC.make_inputs(c, exact=True)
    assert tuple(x.shape) == (c.B, c.D, c.H, c.W, c.CI) and tuple(gy.shape) == (c.B, Do, Ho, Wo, c.CO)
    assert x.abs().max() <= 2 and gy.abs().max() <= 2 and torch.equal(x, x.round()) and torch.equal(gy, gy.round())


def test_names_are_unique_and_inputs_differ():
    assert len(set(WC.IDS)) == len(WC.IDS)
    a, b = WC.BY_NAME["p1_16_16_w100_h7_s1"], WC.BY_NAME["p1_16_16_w100_h7_s3"]
    assert not torch.equal(WC.make_inputs(a, True)[0], WC.make_inputs(b, True)[0])


def test_required_kernel_coverage():
    names = {c.kernel_name for c in WC.CASES}
    pers = {"conv_wgrad_pers_kernel<%s>" % a for a in
            ("1, 1, 1, 4, 64", "1, 1, 1, 4, 80", "2, 1, 1, 4, 64", "2, 1, 1, 4, 80", "1, 2, 1, 4, 64", "1, 2, 1, 2, 80",
             "2, 2, 1, 2, 64", "2, 2, 1, 2, 80", "1, 1, 3, 2, 64", "1, 1, 3, 2, 48")}
    assert pers <= names, pers - names
    assert {n for n in names if n.startswith("conv_wgrad_pers_kernel")} == pers      # the ten reachable forms, no other
    lds = set()
    for n in names:
        m = re.fullmatch(r"conv_wgrad_lds_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>", n)
        if m:
            mt, nt, ty, kw, pcb, sw = map(int, m.groups())
            lds.add((ty, kw, pcb, sw))
    want = {(1, 1, 0, 1),                                              # 1x1
            (3, 3, 0, 1), (3, 3, 4, 1), (3, 3, 8, 1), (3, 3, 0, 2), (3, 3, 8, 2),
            (9, 3, 0, 1), (9, 3, 4, 1), (9, 3, 8, 1),                  # (no stride-2 form of 27 taps)
            (5, 5, 0, 1), (5, 5, 0, 2), (5, 5, 8, 2)}
    assert want <= lds, want - lds
    for n in ("conv_wgrad_kernel<5, 4>", "conv_wgrad_kernel<1, 1>", "conv_wgrad_kernel<4, 2>", "conv_wgrad_packed_kernel<1, 4>",
              "conv_wgrad_packed_kernel<1, 8>"):
        assert n in names, n
    # every kd = 1 persistent form: a single-chunk case whose height is no multiple of R, and a multi-chunk case
    for n in pers:
        mt, nt, kd, R, xc = map(int, re.findall(r"\d+", n))
        mine = [c for c in WC.CASES if c.kernel_name == n]
        assert any(c.W <= xc and c.H % R for c in mine), n
        assert any(c.W > xc for c in mine), n
        assert any(c.B == 2 and c.D == 2 for c in mine) or kd == 3, n
    # slot caps: one workgroup walks five units or more, an odd and an even count
    for fam in ("pers_kernel<1, 1, 1,", "pers_kernel<2, 1, 1,", "pers_kernel<1, 2, 1,", "pers_kernel<2, 2, 1,", "pers_kernel<1, 1, 3,"):
        assert {c.slots for c in WC.CASES if fam in c.kernel_name} >= {None, 1, 3}, fam


def _convs(model):
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose3d)):
            k, s, p = tuple(m.kernel_size), tuple(m.stride), tuple(m.padding)
            if len(k) == 2:
                k, s, p = (1,) + k, (1,) + s, (0,) + p
            yield ("convT" if isinstance(m, nn.ConvTranspose3d) else "conv", m.in_channels, m.out_channels, k, s, p)


def test_every_layer_of_the_network_has_a_case():
    from mvster_amd import MVS4net
    from mvster_amd.train_ops import _FpnGather
    from tests.conftest import SHIPPED
    table = {(c.form, c.CI, c.CO, c.kernel, c.stride, c.padding) for c in WC.CASES}
    keeps = {(c.form, c.CI, c.CO, c.kernel, c.stride, c.co_keep, c.ci_keep) for c in WC.CASES}
    layers = set()
    for cfg in (SHIPPED, dict(SHIPPED, reg_net="reg3d", mono=False), dict(SHIPPED, group_cor_dim=[4, 4, 4, 4])):
        layers |= set(_convs(MVS4net(**cfg)))
    assert len(layers) >= 40
    for kind, cin, cout, k, s, p in sorted(layers):
        form, CI, CO, k2, s2, p2, co_keep, ci_keep = WC.layer_form(kind, cin, cout, k, s, p)
        assert (form, CI, CO, k2, s2, p2) in table, (kind, cin, cout, k, s)
        if co_keep < CO or ci_keep < CI:           # the padded heads and the RGB layer: their keeps too
            assert (form, CI, CO, k2, s2, co_keep, ci_keep) in keeps, (kind, cin, cout, k, s)
    # the FPN gather's 64 -> 72 1x1 (train_ops._FpnGather.backward): gG carries a pitch of 80 channels
    assert _FpnGather.PITCH == {8: 80}
    assert ("plain", 64, 80, (1, 1, 1), (1, 1, 1), 72, 64) in keeps
