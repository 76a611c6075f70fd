"""Shared by tests/test_scan_cpu.py and tests/test_gpu_scan.py: synthetic scans in memory and on disk (not a test module)."""
import os

import numpy as np

from mvster_amd import formats
from mvster_amd.synthetic import DTU_DEPTH_MIN
from mvster_amd.synthetic_scene import plane_depth_maps

# 7 views: view 2 has fewer than nviews - 1 = 4 sources (padding), view 5 has none (dropped), view 0 more than 4 (cut)
PAIRS_7 = [(0, [1, 2, 3, 4, 6]), (1, [0, 2, 3, 4]), (2, [0, 1]), (3, [4, 2, 1, 0]), (4, [3, 6, 0, 1]), (5, []),
           (6, [4, 3, 2, 0])]


def ring_pairs(V, nsrc):
    """Every view a reference view with its ``nsrc`` nearest neighbours by number (cyclic)."""
    offs = [o for k in range(1, nsrc + 1) for o in (k, -k)][:nsrc]
    return [(r, [(r + o) % V for o in offs]) for r in range(V)]


def synthetic_scan(V, H, W, seed=0):
    """Seeded 8-bit images [V,H,W,3] with low-frequency structure, quarter-resolution intrinsics (the convention of
    ``formats.read_cam_file``), extrinsics and a DTU-like (depth_min, depth_interval) per view."""
    _, Ks, Es = plane_depth_maps(V, H, W, seed=seed)                 # full-resolution intrinsics
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    images = []
    for v in range(V):
        base = 0.25 * (np.sin(xs * (9.0 - v % 5) / W + v) * np.cos(ys * (6.0 + v % 3) / H) + 1.0)
        img = 0.5 * rng.rand(H, W, 3).astype(np.float32) + base[..., None]
        images.append(np.clip(img * 255, 0, 255).astype(np.uint8))
    Kq = Ks.copy()
    Kq[:, :2, :] /= 4.0
    ranges = [(DTU_DEPTH_MIN + 1.5 * v, 2.5 * 1.06) for v in range(V)]
    return dict(images=np.stack(images), Ks=Kq, Es=Es, depth_ranges=ranges)


def write_scan_folder(root, scan, sc, pairs, images_dir="images"):
    """The reference's evaluation layout: ``images/%08d.jpg``, ``cams/%08d_cam.txt``, ``pair.txt`` (file numbers = view
    numbers).  The cam files carry FULL-resolution intrinsics (``read_cam_file`` divides by 4)."""
    from PIL import Image
    base = os.path.join(root, scan)
    os.makedirs(os.path.join(base, images_dir), exist_ok=True)
    os.makedirs(os.path.join(base, "cams"), exist_ok=True)
    for v in range(len(sc["images"])):
        Image.fromarray(sc["images"][v]).save(os.path.join(base, images_dir, "{:0>8}.jpg".format(v)), quality=95)
        cam = np.zeros((2, 4, 4), dtype=np.float32)
        cam[0] = sc["Es"][v]
        cam[1, :3, :3] = sc["Ks"][v]
        cam[1, :2, :3] *= 4.0
        cam[1, 3, :2] = sc["depth_ranges"][v]                        # depth_min, depth_interval (two fields: no plane count)
        with open(os.path.join(base, "cams", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write("extrinsic\n")
            for i in range(4):
                f.write(" ".join(repr(float(x)) for x in cam[0, i]) + "\n")
            f.write("\nintrinsic\n")
            for i in range(3):
                f.write(" ".join(repr(float(x)) for x in cam[1, i, :3]) + "\n")
            f.write("\n%r %r\n" % (float(cam[1, 3, 0]), float(cam[1, 3, 1])))
    with open(os.path.join(base, "pair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for r, srcs in pairs:
            f.write("%d\n%d %s\n" % (r, len(srcs), " ".join("%d 1.0" % v for v in srcs)))
    return base


def sample_of(sc, plan, r):
    """Per-sample inputs of reference view row ``r`` as the per-sample loop builds them: ([1,3,H,W] float images in
    ``read_img``'s arithmetic, proj dict of [1,N,2,4,4], depth_values [1,ndv]); NumPy."""
    row = plan.view_table[r]
    imgs = [(np.asarray(sc["images"][v], dtype=np.float32) / 255.0).transpose(2, 0, 1)[None] for v in row]
    proj = {k: m[row][None] for k, m in plan.proj.items()}
    return imgs, proj, plan.depth_values[r][None]
