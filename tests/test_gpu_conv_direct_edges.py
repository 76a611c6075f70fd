"""Direct (variant 0) and split-K (variant 2) convolution kernel at its edge shapes.

conv_mfma_kernel walks the kernel taps in scalar registers and decides padding from a per-voxel bit mask
(mvster_amd/csrc/conv_taps.h).  Every other convolution kernel is tested for equality with this one, so its output is
pinned three ways for each layer x input of tests/conv_direct_cases.py:
  * every tile shape of variant 0 equals tiles (1, 1, 0) bit for bit, every tile shape of variant 2 equals (1, 1, 2);
  * variant 0 is within 2e-5 x max|y| of an fp64 convolution (the bound of test_conv_bn_relu);
  * the SHA-256 of both outputs equals the digest recorded from the kernel as it was before the scalar tap walk
    (tests/golden/conv_direct_parent.json, written by scripts/record_conv_direct.py): same K order, same split-K
    wave -> step assignment, same reduction order, same epilogue.
"""
import json
import os

import pytest
import torch

from tests.conv_direct_cases import LAYERS, SHAPES, digest, direct_tiles, key, make_case, splitk_tiles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_direct_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_direct_and_splitk_edges(name, golden):
    from mvster_amd import _lib
    cin = LAYERS[name][0]
    for shape in SHAPES:
        layer, x, skip, skip_mode, ref = make_case(name, shape, DEV)
        base = layer(x, skip=skip, skip_mode=skip_mode, tiles=(1, 1, 0))
        assert _lib.last_kernel() == "conv_mfma_kernel<%d, 1, 1, false>" % cin, _lib.last_kernel()
        err = (base.double() - ref).abs().max().item()
        bound = 2e-5 * ref.abs().max().item()
        print("%s %s: variant 0 max|err| %.3e (bound %.3e)" % (name, shape, err, bound))
        assert err <= bound, (name, shape, err, bound)
        assert digest(base) == golden[key(name, shape, 0)], (name, shape, "variant 0 differs from the recorded kernel")
        for mt, nt in direct_tiles(cin, layer.ntile_total):
            got = layer(x, skip=skip, skip_mode=skip_mode, tiles=(mt, nt, 0))
            assert _lib.last_kernel() == "conv_mfma_kernel<%d, %d, %d, false>" % (cin, mt, nt), _lib.last_kernel()
            assert torch.equal(got, base), (name, shape, mt, nt)
        tiles2 = splitk_tiles(cin, layer.ntile_total)
        if tiles2:
            base2 = layer(x, skip=skip, skip_mode=skip_mode, tiles=(1, 1, 2))
            assert _lib.last_kernel() == "conv_mfma_kernel<%d, 1, 1, true>" % cin, _lib.last_kernel()
            assert digest(base2) == golden[key(name, shape, 2)], (name, shape, "variant 2 differs from the recorded kernel")
            for mt, nt in tiles2:
                got = layer(x, skip=skip, skip_mode=skip_mode, tiles=(mt, nt, 2))
                assert _lib.last_kernel() == "conv_mfma_kernel<%d, %d, %d, true>" % (cin, mt, nt), _lib.last_kernel()
                assert torch.equal(got, base2), (name, shape, "splitk", mt, nt)
