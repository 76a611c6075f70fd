#!/usr/bin/env python
"""Record the SHA-256 digests of the direct (variant 0) and split-K (variant 2) convolution kernel's outputs for the
layers and inputs of tests/conv_direct_cases.py -> tests/golden/conv_direct_parent.json.

Run it with the library whose output is to be pinned (MVSTER_LIB=/path/to/libmvster_hip.so for one built from another
commit): tests/test_gpu_conv_direct_edges.py then asserts that the current kernel reproduces those bits.  The file
holds digests only.

    python scripts/record_conv_direct.py [--out tests/golden/conv_direct_parent.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.conv_direct_cases import LAYERS, SHAPES, digest, key, make_case, splitk_tiles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_direct_parent.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    out = {}
    for name in sorted(LAYERS):
        for shape in SHAPES:
            layer, x, skip, skip_mode, _ = make_case(name, shape, dev)
            out[key(name, shape, 0)] = digest(layer(x, skip=skip, skip_mode=skip_mode, tiles=(1, 1, 0)))
            if splitk_tiles(LAYERS[name][0], layer.ntile_total):
                out[key(name, shape, 2)] = digest(layer(x, skip=skip, skip_mode=skip_mode, tiles=(1, 1, 2)))
    torch.cuda.synchronize()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(out), args.out))


if __name__ == "__main__":
    main()
