"""On-disk formats either side of the path: PFM depth / confidence maps, MVSNet-style
``*_cam.txt`` and ``pair.txt``, the evaluation sample (view list, images, multi-scale ``proj_matrices`` dict,
``depth_values``) the forward pass takes.

Behaviour follows the reference's readers and writers -- ``datasets/data_io.py:6-71`` (``read_pfm`` / ``save_pfm``),
``datasets/general_eval4.py:24-57`` (view list), ``:59-79`` (``read_cam_file``), ``:81-86`` (``read_img``), ``:92-108``
(admissible image size), ``:111-188`` (sample), ``datasets/tanks.py`` / ``datasets/eth3d.py`` (``read_cam_file_minmax``,
``load_tanks_sample``, ``load_eth3d_sample``: restated and compared in ``tests/test_scan_datasets_cpu.py``), ``test_mvs4.py:94-103`` (``read_camera_parameters``), ``:126-136``
(``read_pair_file``), ``:138-155`` (``write_cam``).  **Pinned** by ``tests/golden/g10_formats.npz``: the bytes / text /
arrays the reference's own functions write and read for the same inputs (``oracle/make_golden.py g10``), compared
byte for byte and element for element in ``tests/test_formats_cpu.py``.
"""
import os
import re
import sys

import numpy as np

_PFM_DIMS = re.compile(r"^(\d+)\s(\d+)\s$")       # "<width> <height>\n": exactly what the reference accepts


def _pfm_header(f):
    """-> (channels, width, height, scale, numpy byte-order character) of an open PFM file."""
    magic = f.readline().decode("utf-8").rstrip()
    if magic not in ("PF", "Pf"):
        raise Exception("Not a PFM file.")
    dims = _PFM_DIMS.match(f.readline().decode("utf-8"))
    if dims is None:
        raise Exception("Malformed PFM header.")
    scale = float(f.readline().rstrip())
    # the sign of the scale line is the byte-order flag: negative = little-endian samples
    return (3 if magic == "PF" else 1), int(dims.group(1)), int(dims.group(2)), abs(scale), ("<" if scale < 0 else ">")


def read_pfm(filename):
    """-> (data [H,W] or [H,W,3] in top-to-bottom row order, dtype as stored, scale)."""
    with open(filename, "rb") as f:
        channels, width, height, scale, order = _pfm_header(f)
        samples = np.fromfile(f, order + "f")
    shape = (height, width, 3) if channels == 3 else (height, width)
    return samples.reshape(shape)[::-1], scale       # rows are stored bottom-to-top


def save_pfm(filename, image, scale=1):
    """float32 [H,W], [H,W,1] (both 'Pf') or [H,W,3] ('PF'); samples go out in the array's own byte order."""
    if image.dtype.name != "float32":
        raise Exception("Image dtype must be float32.")
    grey = image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1)
    if not grey and not (image.ndim == 3 and image.shape[2] == 3):
        raise Exception("Image must have H x W x 3, H x W x 1 or H x W dimensions.")
    order = image.dtype.byteorder
    little = order == "<" or (order == "=" and sys.byteorder == "little")
    header = "%s\n%d %d\n%f\n" % ("Pf" if grey else "PF", image.shape[1], image.shape[0], -scale if little else scale)
    with open(filename, "wb") as f:
        f.write(header.encode("utf-8"))
        image[::-1].tofile(f)


def _cam_lines(filename):
    with open(filename) as f:
        return [line.rstrip() for line in f.readlines()]


def read_camera_parameters(filename):
    """``extrinsic`` 4x4 on lines 1-4, ``intrinsic`` 3x3 on lines 7-9 -> (intrinsics, extrinsics), float32."""
    lines = _cam_lines(filename)
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
    return intrinsics, extrinsics


def read_cam_file(filename, interval_scale=1.0, ndepths=192):
    """Evaluation-time reader: intrinsics of the quarter-resolution stage (rows 0-1 divided by 4), depth_min and the
    depth interval (rescaled to ``ndepths`` planes when the file carries a plane count, then times interval_scale)."""
    lines = _cam_lines(filename)
    intrinsics, extrinsics = read_camera_parameters(filename)
    intrinsics[:2, :] /= 4.0
    fields = lines[11].split()
    depth_min, depth_interval = float(fields[0]), float(fields[1])
    if len(fields) >= 3:
        depth_max = depth_min + int(float(fields[2])) * depth_interval
        depth_interval = (depth_max - depth_min) / ndepths
    return intrinsics, extrinsics, depth_min, depth_interval * interval_scale


def read_cam_file_minmax(filename, negative_min_to=None):
    """The reader of the Tanks and Temples and ETH3D loaders (datasets/tanks.py:33-46, datasets/eth3d.py:40-55) ->
    (intrinsics at FULL resolution, extrinsics, depth_min, depth_max): the first and the LAST number of line 11, whatever
    lies between them (an interval, a plane count).  ``negative_min_to=1``: ETH3D's clamp, a negative depth_min becomes 1."""
    intrinsics, extrinsics = read_camera_parameters(filename)
    fields = _cam_lines(filename)[11].split()
    depth_min, depth_max = float(fields[0]), float(fields[-1])
    if negative_min_to is not None and depth_min < 0:
        depth_min = negative_min_to
    return intrinsics, extrinsics, depth_min, depth_max


def write_cam(filename, cam):
    """cam [2,4,4]: [0] extrinsic, [1][:3,:3] intrinsic, [1][3] = depth_min, interval, planes, depth_max."""
    with open(filename, "w") as f:
        f.write("extrinsic\n")
        for i in range(4):
            f.write("".join(str(cam[0][i][j]) + " " for j in range(4)) + "\n")
        f.write("\nintrinsic\n")
        for i in range(3):
            f.write("".join(str(cam[1][i][j]) + " " for j in range(3)) + "\n")
        f.write("\n" + " ".join(str(cam[1][3][j]) for j in range(4)) + "\n")


def read_pair_file(filename):
    """-> [(ref_view, [src_view, ...]), ...]; views without sources are dropped."""
    data = []
    with open(filename) as f:
        for _ in range(int(f.readline())):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if src_views:
                data.append((ref_view, src_views))
    return data


def stage_proj_matrices(intrinsics, extrinsics):
    """Per-view (quarter-resolution) intrinsics [N,3,3] + extrinsics [N,4,4] -> the forward pass's dict
    ``stage1..stage4`` of [N,2,4,4] float32 ([.,0] = extrinsic, [.,1,:3,:3] = intrinsic scaled 1/2, 1, 2, 4)."""
    n = len(intrinsics)
    base = np.zeros((n, 2, 4, 4), dtype=np.float32)
    base[:, 0] = np.asarray(extrinsics, dtype=np.float32)
    base[:, 1, :3, :3] = np.asarray(intrinsics, dtype=np.float32)
    out = {}
    for name, s in (("stage1", 0.5), ("stage2", 1.0), ("stage3", 2.0), ("stage4", 4.0)):
        m = base.copy()
        m[:, 1, :2, :] = base[:, 1, :2, :] * s
        out[name] = m
    return out


def depth_value_range(depth_min, depth_interval, ndepths=192):
    """The ``depth_values`` vector of a sample (general_eval4.py:168-170)."""
    return np.arange(depth_min, depth_interval * (ndepths - 0.5) + depth_min, depth_interval, dtype=np.float32)


def read_img(filename):
    """8-bit image file -> float32 [H,W,3] in 0..1 (general_eval4.py:81-86)."""
    from PIL import Image
    return np.array(Image.open(filename), dtype=np.float32) / 255.0


def eval_view_list(datapath, scans, nviews):
    """[(scan, ref_view, src_views), ...] over the scans' ``pair.txt`` (general_eval4.py:24-57): reference views
    without sources are dropped, a source list shorter than ``nviews`` is filled up with its first entry."""
    metas = []
    for scan in scans:
        for ref_view, src_views in read_pair_file(os.path.join(datapath, scan, "pair.txt")):
            if len(src_views) < nviews:
                src_views = src_views + [src_views[0]] * (nviews - len(src_views))
            metas.append((scan, ref_view, src_views))
    return metas


def _admissible_size(h, w, max_h, max_w, base=64):
    """The size the reference's loader brings an image to (general_eval4.py:92-100): shrunk to fit max_h x max_w,
    then rounded down to multiples of ``base`` (float arithmetic as there)."""
    if h > max_h or w > max_w:
        scale = 1.0 * max_h / h
        if scale * w > max_w:
            scale = 1.0 * max_w / w
        return scale * w // base * base, scale * h // base * base
    return 1.0 * w // base * base, 1.0 * h // base * base


def scale_input_size(h, w, max_h, max_w):
    """The loader's target size for an ``h`` x ``w`` image within ``max_h`` x ``max_w`` (general_eval4.py:92-103) ->
    ``(Hd, Wd, scale_h, scale_w)``: ints and the two Python floats the intrinsics are multiplied by.  Float arithmetic as
    there: 1200 x 1600 within 864 x 1152 gives 832 x 1152 (0.72 * 1200 = 864 = 13.5 * 64, rounded down), the size the
    reference runs DTU at."""
    new_w, new_h = _admissible_size(h, w, max_h, max_w)
    return int(new_h), int(new_w), 1.0 * new_h / h, 1.0 * new_w / w


def scale_intrinsics(K, scale_h, scale_w):
    """A copy of the float32 intrinsics ``K`` [3,3] or [V,3,3] with row 0 times ``scale_w`` and row 1 times ``scale_h``
    (general_eval4.py:104-105: two in-place multiplications of a float32 matrix by a Python float)."""
    K = np.array(K, dtype=np.float32)
    K[..., 0, :] *= scale_w
    K[..., 1, :] *= scale_h
    return K


def crop_intrinsics(K, top, left):
    """A copy of the float32 intrinsics ``K`` [3,3] or [V,3,3] for an image that lost ``top`` rows and ``left`` columns:
    ``cy - top``, ``cx - left`` (datasets/tanks.py:58: ``intrinsics[1,2] = intrinsics[1,2] - 28``, one float32 subtraction)."""
    K = np.array(K, dtype=np.float32)
    K[..., 1, 2] = K[..., 1, 2] - top
    K[..., 0, 2] = K[..., 0, 2] - left
    return K


def _axis_table(ns, nd):
    """xofs / alpha of OpenCV's resize.cpp (INTER_LINEAR, float path) for one axis: ns source -> nd output samples."""
    inv = np.float64(nd) / np.float64(ns)
    scale = np.float64(1.0) / inv                                            # two roundings, not ns / nd
    f = ((np.arange(nd, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= ns - 1
    s[low], f[low] = 0, 0.0
    s[high], f[high] = ns - 1, 0.0                                           # (the second tap is not read there)
    return s, f.astype(np.float32)


def resize_tables(Hs, Ws, Hd, Wd):
    """Per-axis tap tables of ``cv2.resize(img [Hs,Ws], (Wd, Hd))``, INTER_LINEAR -> ``(sx, fx, sy, fy)``: first tap (int32)
    and fraction (float32) per output column / row; the weights are ``1.f - f`` and ``f``.  Built once per size pair on
    the host, in double precision, as OpenCV builds them before it touches a pixel; the GPU kernel gets them uploaded."""
    sx, fx = _axis_table(int(Ws), int(Wd))
    sy, fy = _axis_table(int(Hs), int(Hd))
    return sx, fx, sy, fy


def resize_linear(img, Hd, Wd):
    """``cv2.resize(img, (Wd, Hd))`` with default arguments for a float32 [Hs,Ws,C] image (OpenCV's resize.cpp, float path,
    restated; csrc/resize_math.h is the same arithmetic on the GPU): horizontal pass, then vertical, every product and
    sum rounded to float32 on its own; the 2 x 2 mean of the area path at exactly 2:1 on both axes.  There is no
    ``cv2`` to pin this against: agreement with a particular OpenCV binary is to within the last place of single results
    (its SIMD builds may fuse the vertical pass) and has not been measured."""
    img = np.asarray(img)
    if img.dtype != np.float32 or img.ndim != 3:
        raise RuntimeError("resize_linear: expects a float32 [H,W,C] image, got %s %s" % (img.dtype, img.shape))
    Hs, Ws = img.shape[:2]
    Hd, Wd = int(Hd), int(Wd)
    if not (0 < Hd <= Hs and 0 < Wd <= Ws):
        raise RuntimeError("resize_linear: %dx%d -> %dx%d: the loader never enlarges" % (Hs, Ws, Hd, Wd))
    if Ws == 2 * Wd and Hs == 2 * Hd:
        return ((img[0::2, 0::2] + img[0::2, 1::2]) + (img[1::2, 0::2] + img[1::2, 1::2])) * np.float32(0.25)
    sx, fx, sy, fy = resize_tables(Hs, Ws, Hd, Wd)
    sx1, sy1 = np.minimum(sx + 1, Ws - 1), np.minimum(sy + 1, Hs - 1)        # (weight 0 where the clamp acts)
    one = np.float32(1.0)
    a0, a1 = (one - fx)[None, :, None], fx[None, :, None]
    b0, b1 = (one - fy)[:, None, None], fy[:, None, None]
    t0 = img[sy][:, sx] * a0 + img[sy][:, sx1] * a1
    t1 = img[sy1][:, sx] * a0 + img[sy1][:, sx1] * a1
    return t0 * b0 + t1 * b1


def load_eval_sample(datapath, scan, ref_view, src_views, nviews, interval_scale=1.06, ndepths=192,
                     max_h=None, max_w=None, resample=False):
    """One evaluation sample as ``general_eval4.MVSDataset.__getitem__`` (:111-188) hands it to the forward pass:
    ``imgs`` list of [3,H,W] float32, ``proj_matrices`` dict stage1..4 of [N,2,4,4], ``depth_values`` [ndepths],
    ``filename`` pattern.  With the default ``resample=False`` images must already have an admissible size (H, W
    multiples of 64 within max_h x max_w) and anything else raises.  ``resample=True``: images are brought to the
    loader's size with ``resize_linear`` and the intrinsics scaled, as ``scale_mvs_input`` does, for samples whose views
    share one native size (the reference's second resampling of a source to its reference view's size is not done:
    DESIGN.md section 7)."""
    imgs, intr, extr, depth_values = [], [], [], None
    first_hw = None
    for i, vid in enumerate([ref_view] + list(src_views[:nviews - 1])):
        img_file = os.path.join(datapath, "{}/images_post/{:0>8}.jpg".format(scan, vid))
        if not os.path.exists(img_file):
            img_file = os.path.join(datapath, "{}/images/{:0>8}.jpg".format(scan, vid))
        img = read_img(img_file)
        K, E, depth_min, depth_interval = read_cam_file(
            os.path.join(datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid)), interval_scale, ndepths)
        h, w = img.shape[:2]
        new_w, new_h = _admissible_size(h, w, h if max_h is None else max_h, w if max_w is None else max_w)
        if resample:
            if first_hw is not None and (h, w) != first_hw:
                raise NotImplementedError("image %s is %dx%d but the sample's reference view is %dx%d: views of different "
                                          "native sizes within a scan are not supported" % (img_file, h, w, *first_hw))
            if (new_h, new_w) != (h, w):
                img = resize_linear(img, int(new_h), int(new_w))
        elif (new_h, new_w) != (h, w) or (first_hw is not None and (h, w) != first_hw):
            raise NotImplementedError("image %s is %dx%d and would be resampled to %dx%d: resize the images first"
                                      % (img_file, h, w, *(first_hw or (new_h, new_w))))
        K[0, :] *= 1.0 * new_w / w
        K[1, :] *= 1.0 * new_h / h
        first_hw = first_hw or (h, w)
        imgs.append(img.transpose(2, 0, 1))
        intr.append(K)
        extr.append(E)
        if i == 0:
            depth_values = depth_value_range(depth_min, depth_interval, ndepths)
    return {"imgs": imgs, "proj_matrices": stage_proj_matrices(intr, extr), "depth_values": depth_values,
            "filename": scan + "/{}/" + "{:0>8}".format(ref_view) + "{}"}


def _quarter(K):
    """Full-resolution intrinsics -> the quarter-resolution convention of ``read_cam_file`` / ``stage_proj_matrices`` (rows
    0-1 divided by 4, exact).  ``stage_proj_matrices`` of it carries the bits of the Tanks / ETH3D loaders' chain
    ``x 0.125, x 2, x 2, x 2`` (datasets/tanks.py:96-110): every factor is a power of two (tests/test_scan_datasets_cpu.py)."""
    K = np.array(K, dtype=np.float32)
    K[..., :2, :] /= 4.0
    return K


def _dataset_sample(datapath, scan, ref_view, src_views, nviews, cams, prepare, negative_min_to):
    imgs, intr, extr, depth_values = [], [], [], None
    for i, vid in enumerate([ref_view] + list(src_views[:nviews - 1])):     # cut, never padded (tanks.py:68)
        img = read_img(os.path.join(datapath, scan, "images", "{:0>8}.jpg".format(vid)))
        K, E, depth_min, depth_max = read_cam_file_minmax(os.path.join(datapath, scan, cams, "{:0>8}_cam.txt".format(vid)),
                                                          negative_min_to)
        K, img = prepare(K, img)
        imgs.append(img.transpose(2, 0, 1))
        intr.append(_quarter(K))
        extr.append(E)
        if i == 0:
            depth_values = np.array([depth_min, depth_max], dtype=np.float32)
    return {"imgs": imgs, "proj_matrices": stage_proj_matrices(intr, extr), "depth_values": depth_values,
            "filename": scan + "/{}/" + "{:0>8}".format(ref_view) + "{}"}


def load_tanks_sample(datapath, scan, ref_view, src_views, nviews=7, crop_rows=(28, 28)):
    """One sample as ``datasets/tanks.py`` ``MVSDataset.__getitem__`` (:65-133) builds it from ``datapath/scan`` (the caller
    joins the split): ``crop_rows = (top, bottom)`` rows cut off every image without resampling and ``cy - top`` (:53-60;
    the loader's 1080 -> 1024), cameras from ``cams/``, ``depth_values`` = [depth_min, depth_max] of the reference view's
    cam file, the source list cut to ``nviews - 1`` and never padded.  ``imgs`` list of [3,H,W] float32."""
    top, bottom = int(crop_rows[0]), int(crop_rows[1])

    def prepare(K, img):
        return crop_intrinsics(K, top, 0), img[top:img.shape[0] - bottom, :, :]
    return _dataset_sample(datapath, scan, ref_view, src_views, nviews, "cams", prepare, None)


def load_eth3d_sample(datapath, scan, ref_view, src_views, nviews=7, img_wh=(1920, 1280)):
    """One sample as ``datasets/eth3d.py`` ``MVSDataset.__getitem__`` (:67-135): every image resized to ``img_wh = (W, H)``
    from its own native size (``resize_linear`` where the loader calls ``cv2.resize``) and its intrinsics scaled by its own
    ``W / original_w``, ``H / original_h`` (:89-90), cameras from ``cams_1/``, a negative depth_min replaced by 1 (:51-52),
    ``depth_values`` = [depth_min, depth_max].  Views of different native sizes are fine: the target does not depend on a
    view's partners.  Enlarging raises, as ``resize_linear`` does."""
    Wd, Hd = int(img_wh[0]), int(img_wh[1])

    def prepare(K, img):
        h, w = img.shape[:2]
        return scale_intrinsics(K, Hd / h, Wd / w), resize_linear(img, Hd, Wd)
    return _dataset_sample(datapath, scan, ref_view, src_views, nviews, "cams_1", prepare, 1)
