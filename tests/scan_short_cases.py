"""Shared by tests/test_scan_short_cpu.py and tests/test_gpu_scan_short.py (not a test module): a scan whose pair lists are
shorter than ``nviews - 1``."""
import os

import numpy as np

from mvster_amd import formats

NVIEWS = 4
# 6 views, nviews - 1 = 3 sources at most.  Lengths 3, 2, 3, 1, 3, 0: the one-source view (3) directly follows and directly
# precedes a three-source view, so nothing of one replay can leak into the next unnoticed; view 5 has no sources and nobody
# lists it (fusion wants a depth map for every listed source)
PAIRS = [(0, [1, 2, 3]), (1, [0, 2]), (2, [1, 3, 4]), (3, [4]), (4, [3, 2, 0]), (5, [])]
WITH_SOURCES = [(r, s) for r, s in PAIRS if s]
COUNTS = [3, 2, 3, 1, 3]
# one list longer than nviews - 1 (cut) next to the short ones
PAIRS_CUT = [(0, [1, 2, 3, 4, 5]), (1, [0, 2]), (2, [1]), (3, []), (4, [3, 2, 0]), (5, [4, 0, 1, 2])]


def decode_all(root, name, cams, negative_min_to, V):
    """Every view of a dataset folder as ``infer_scan`` takes it -- also those ``pair.txt`` gives no sources, which
    ``scan.read_scan_folder`` leaves out: decoded images, quarter-resolution intrinsics, extrinsics, (depth_min, depth_max)."""
    from PIL import Image
    images, Ks, Es, ranges = [], [], [], []
    for v in range(V):
        images.append(np.array(Image.open(os.path.join(root, name, "images", "{:0>8}.jpg".format(v))), dtype=np.uint8))
        K, E, dmin, dmax = formats.read_cam_file_minmax(os.path.join(root, name, cams, "{:0>8}_cam.txt".format(v)), negative_min_to)
        K[:2, :] /= 4.0
        Ks.append(K)
        Es.append(E)
        ranges.append((dmin, dmax))
    return dict(images=images, Ks=np.stack(Ks), Es=np.stack(Es), depth_ranges=ranges)
