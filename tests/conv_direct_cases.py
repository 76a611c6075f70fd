"""Layers, inputs and tile shapes of the direct / split-K convolution edge cases -- TEST INFRASTRUCTURE.

Shared by tests/test_gpu_conv_direct_edges.py (which compares) and scripts/record_conv_direct.py (which records the
digests of tests/golden/conv_direct_parent.json), so that both build the same tensors from the same seeds.
"""
import hashlib

import torch

# name -> (cin, cout, kernel, stride, padding, transposed, skip)
LAYERS = {
    "c16_333": (16, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, False),
    "c32_333": (32, 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, False),
    "c64_333": (64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, False),
    "c16_32_133_s2": (16, 32, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, False),
    "c32_64_133_s2": (32, 64, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, False),
    "t64_32": (64, 32, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, False),
    "t64_32_skip": (64, 32, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, True),
    "t32_16": (32, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, False),
    "t32_16_skip": (32, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, True),
    "c64_72_111": (64, 72, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, False),      # 5 N tiles: the nt = 5 instances
    "c64_144_111": (64, 144, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, False),    # 9 N tiles: the nt = 3 and 9 instances
    "c16_32_155_s2": (16, 32, (1, 5, 5), (1, 2, 2), (0, 2, 2), False, False),
    "c8_16_133": (8, 16, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),
    "c4_8_133": (4, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),
}

# [B, D, H, W]: one voxel; odd sizes below one M tile; an M tile that straddles two batch items; the coarse stage's
# 8 x 8 x 10; several workgroups
SHAPES = [(1, 1, 1, 1), (1, 2, 5, 7), (2, 3, 9, 21), (1, 8, 8, 10), (1, 4, 16, 20)]


def direct_tiles(cin, ntile_total):
    """Every (mt, nt) instance of variant 0 that divides the layer's N tiles."""
    out = [(mt, nt) for nt in (1, 2, 4) for mt in (1, 2, 4) if ntile_total % nt == 0]
    if cin == 64:
        out += [(mt, nt) for nt in (5, 3) for mt in (1, 2, 4) if ntile_total % nt == 0]
        out += [(mt, 9) for mt in (1, 2) if ntile_total % 9 == 0]
    return out


def splitk_tiles(cin, ntile_total):
    if cin < 16:
        return []
    return [(mt, nt) for mt, nt in ((1, 1), (1, 2), (1, 4), (2, 1), (2, 2)) if ntile_total % nt == 0]


def make_case(name, shape, dev):
    """-> (layer, x, skip, skip_mode, reference [fp64, channels-last])."""
    import mvster_amd.conv_plan as cp
    cin, cout, k, s, p, transposed, with_skip = LAYERS[name]
    B, D, H, W = shape
    g = torch.Generator().manual_seed(1000 * sorted(LAYERS).index(name) + SHAPES.index(tuple(shape)))
    fan = cin * k[0] * k[1] * k[2]
    wshape = (cin, cout) + k if transposed else (cout, cin) + k
    w = (torch.randn(*wshape, generator=g) * (2.0 / fan) ** 0.5).to(dev)
    bias = (torch.randn(cout, generator=g) * 0.1).to(dev)
    x = torch.randn(B, D, H, W, cin, generator=g).to(dev)
    layer = cp.ConvLayer(w, transposed, s, p, bias=bias, relu=True)
    oshape = layer.out_shape(B, D, H, W)
    skip = torch.randn(*oshape, cout, generator=g).to(dev) if with_skip else None
    xd = x.permute(0, 4, 1, 2, 3).double()
    if transposed:
        ref = torch.nn.functional.conv_transpose3d(xd, w.double(), stride=s, padding=p,
                                                   output_padding=tuple(si - 1 for si in s))
    else:
        ref = torch.nn.functional.conv3d(xd, w.double(), stride=s, padding=p)
    ref = ref * layer.scale[:cout].double().view(1, -1, 1, 1, 1) + layer.shift[:cout].double().view(1, -1, 1, 1, 1)
    ref = ref.clamp_min(0).permute(0, 2, 3, 4, 1)
    if skip is not None:
        ref = ref + skip.double()
    return layer, x, skip, (cp.SKIP_ADD if with_skip else cp.SKIP_NONE), ref


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def key(name, shape, variant):
    return "%s|%s|v%d" % (name, "x".join(map(str, shape)), variant)
