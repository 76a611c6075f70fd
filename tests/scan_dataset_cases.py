"""Shared by tests/test_scan_datasets_cpu.py and tests/test_gpu_scan_datasets.py (not a test module): cam files and scan
folders in the layouts of the reference's Tanks and Temples and ETH3D loaders, and a LITERAL restatement of what those
loaders compute on the host -- their ``read_cam_file`` and the projection-matrix chain of their ``__getitem__``
(datasets/tanks.py:33-46, :91-127; datasets/eth3d.py:40-55, :89-128) -- importing nothing from mvster_amd."""
import os

import numpy as np

from tests import scan_cases as SC


# ---- the loaders, restated -------------------------------------------------------------------------------------------------
def _fromstring(text):
    """``np.fromstring(text, dtype=np.float32, sep=' ')`` as the loaders call it (text mode; where a NumPy no longer has it,
    the same parse through ``str.split``)."""
    if hasattr(np, "fromstring"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            return np.fromstring(text, dtype=np.float32, sep=" ")
    return np.array(text.split(), dtype=np.float32)


def ref_read_cam_file(filename, eth3d=False):
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = _fromstring(" ".join(lines[1:5])).reshape((4, 4))
    intrinsics = _fromstring(" ".join(lines[7:10])).reshape((3, 3))
    depth_min = float(lines[11].split()[0])
    if eth3d and depth_min < 0:
        depth_min = 1
    depth_max = float(lines[11].split()[-1])
    return intrinsics, extrinsics, depth_min, depth_max


def ref_stage_chain(intrinsics_list, extrinsics_list):
    """The x 0.125, x 2, x 2, x 2 chain over a sample's views -> dict stage1..4 of [N,2,4,4] (intrinsics are modified in
    place, as the loaders do)."""
    stacks = [[], [], [], []]
    for intrinsics, extrinsics in zip(intrinsics_list, extrinsics_list):
        mats = [np.zeros(shape=(2, 4, 4), dtype=np.float32) for _ in range(4)]
        intrinsics[:2, :] *= 0.125
        mats[0][0, :4, :4] = extrinsics.copy()
        mats[0][1, :3, :3] = intrinsics.copy()
        for k in (1, 2, 3):
            intrinsics[:2, :] *= 2
            mats[k][0, :4, :4] = extrinsics.copy()
            mats[k][1, :3, :3] = intrinsics.copy()
        for k in range(4):
            stacks[k].append(mats[k])
    return {"stage%d" % (k + 1): np.stack(stacks[k]) for k in range(4)}


def ref_tanks_intrinsics(intrinsics, top=28):
    intrinsics[1, 2] = intrinsics[1, 2] - top
    return intrinsics


def ref_eth3d_intrinsics(intrinsics, img_wh, original_h, original_w):
    intrinsics[0] *= img_wh[0] / original_w
    intrinsics[1] *= img_wh[1] / original_h
    return intrinsics


# ---- files -----------------------------------------------------------------------------------------------------------------
def write_cam_file(path, K, E, line11):
    """MVSNet-style cam file with FULL-resolution intrinsics; ``line11``: the depth numbers as text."""
    with open(path, "w") as f:
        f.write("extrinsic\n")
        for i in range(4):
            f.write(" ".join(repr(float(x)) for x in E[i]) + "\n")
        f.write("\nintrinsic\n")
        for i in range(3):
            f.write(" ".join(repr(float(x)) for x in K[i]) + "\n")
        f.write("\n" + line11 + "\n")


def dataset_scan(sizes, seed=0, negative_min_view=None):
    """A synthetic scan whose views have the native ``sizes`` [(Hs, Ws)]: images list of uint8 [Hs,Ws,3], full-resolution
    intrinsics ``Kfull`` (principal point and focal length proportional to each view's size), ``Es``, (depth_min,
    depth_max) per view.  The cameras are those of ``scan_cases.synthetic_scan`` at the largest size."""
    V = len(sizes)
    H0, W0 = max(h for h, _ in sizes), max(w for _, w in sizes)
    base = SC.synthetic_scan(V, H0, W0, seed=seed)
    images, Kfull = [], []
    for v, (h, w) in enumerate(sizes):
        big = SC.synthetic_scan(V, h, w, seed=seed + 1 + v)["images"][v]
        images.append(np.ascontiguousarray(big))
        K = base["Ks"][v].copy()
        K[:2] *= 4.0
        K[0] *= np.float32(w / W0)
        K[1] *= np.float32(h / H0)
        Kfull.append(K)
    ranges = [(float(np.float32(base["depth_ranges"][v][0])), float(np.float32(base["depth_ranges"][v][0] + 2.5 * 1.06 * 192)))
              for v in range(V)]
    if negative_min_view is not None:
        ranges[negative_min_view] = (-3.5, ranges[negative_min_view][1])
    return dict(images=images, Kfull=np.stack(Kfull), Es=base["Es"], ranges=ranges)


def write_dataset_folder(root, scan, sc, pairs, cams="cams"):
    """``images/%08d.jpg``, ``<cams>/%08d_cam.txt`` (line 11: depth_min, an interval, a plane count, depth_max) and
    ``pair.txt``; file numbers = view numbers."""
    from PIL import Image
    base = os.path.join(root, scan)
    os.makedirs(os.path.join(base, "images"), exist_ok=True)
    os.makedirs(os.path.join(base, cams), exist_ok=True)
    for v, img in enumerate(sc["images"]):
        Image.fromarray(img).save(os.path.join(base, "images", "{:0>8}.jpg".format(v)), quality=95)
        dmin, dmax = sc["ranges"][v]
        write_cam_file(os.path.join(base, cams, "{:0>8}_cam.txt".format(v)), sc["Kfull"][v], sc["Es"][v],
                       "%r 2.65 192 %r" % (dmin, dmax))
    with open(os.path.join(base, "pair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for r, srcs in pairs:
            f.write("%d\n%d %s\n" % (r, len(srcs), " ".join("%d 1.0" % v for v in srcs)))
    return base


def quarter(K):
    """Full-resolution intrinsics -> the convention ``infer_scan`` takes (rows 0-1 divided by 4)."""
    K = np.array(K, dtype=np.float32)
    K[..., :2, :] /= 4.0
    return K
