"""A scan from a structure-from-motion model: read a COLMAP sparse model (text or binary), score every
pair of views over the sparse points both see, list each view's best sources and take each view's depth range from the
percentiles of its sparse depths -- on the GPU (csrc/geo_sfm.hip; the definition is csrc/sfm_math.h) -- and hand ``infer_scan`` /
``reconstruct_scan`` the dict ``scan.read_scan_folder`` returns, or write the scan folder it reads.

The definition is this project's own, written out in sfm_math.h; where it departs from the customary conversion scripts of the
MVSNet family (a point seen twice in an image counts once; a partner with score zero is never listed; only finite depths
z > 0 enter the range) DESIGN.md says so.  There is no CPU fallback for the three launches.

Undistortion (csrc/geo_undistort.hip, the definition is csrc/undistort_math.h).  By default a model with
distortion still raises and names COLMAP's ``image_undistorter``; ``read_sfm_model(path, distortion="keep")`` takes SIMPLE_RADIAL,
RADIAL and OPENCV cameras as they are, ``undistorted_cameras`` gives the pinhole camera of every undistorted image,
``undistort_points`` / ``distort_points`` take points through the inverse and the distortion, ``undistort_images`` resamples
all images of a chunk in one launch, and ``scan_from_sfm(..., undistort=True)`` does all of it on the way to a scan.  The
definition is this project's own, modelled on COLMAP's undistortion; COLMAP itself was not at hand to compare against, and
DESIGN.md lists the deviations.  Fisheye, FOV, FULL_OPENCV and THIN_PRISM cameras are out of scope.  No CPU fallback either."""
import os
import struct

import numpy as np
import torch

from . import _lib, formats

MAX_VIEWS = 16384                         # sfm::kMaxViews
MAX_SOURCES = 64                          # sfm::kMaxSources
SIGMA_MIN = 0.05                          # sfm::kSigmaMin
TWO32 = 4294967296.0

# model id -> (name, number of parameters, position of the first distortion parameter)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3, 3), 1: ("PINHOLE", 4, 4), 2: ("SIMPLE_RADIAL", 4, 3), 3: ("RADIAL", 5, 3),
                 4: ("OPENCV", 8, 4)}
_MODEL_IDS = {name: mid for mid, (name, _, _) in CAMERA_MODELS.items()}
CAMERA_RECORD = 12                        # und::kCam: model id, W, H, fx, fy, cx, cy, k1, k2, p1, p2, pad
RESIDUAL_BOUND = 1e-9                     # und::kResidualBound, normalised units
MAX_SIDE = 1 << 20                        # und::kMaxSide
MAX_SCALE = 1024.0


# ---- reading a model -------------------------------------------------------------------------------------------------------------

def _intrinsics(what, model, params, keep=False):
    """-> K [3,3] float64 of a camera without distortion; anything else raises.  ``keep``: distortion parameters are taken as
    they are (finite), and K describes the distorted camera."""
    if model not in CAMERA_MODELS:
        raise RuntimeError("read_sfm_model: %s has camera model %r; only SIMPLE_PINHOLE, PINHOLE and the SIMPLE_RADIAL / RADIAL / "
                           "OPENCV models with every distortion parameter 0 are taken: run COLMAP's image_undistorter first "
                           "(undistortion is out of scope here)" % (what, model))
    name, count, first = CAMERA_MODELS[model]
    if len(params) != count:
        raise RuntimeError("read_sfm_model: %s (%s) has %d parameters, not %d" % (what, name, len(params), count))
    if keep and not all(np.isfinite(float(p)) for p in params):
        raise RuntimeError("read_sfm_model: %s (%s) has a parameter that is not finite: %s" % (what, name, [float(p) for p in params]))
    if not keep and any(float(p) != 0.0 for p in params[first:]):
        raise RuntimeError("read_sfm_model: %s (%s) has distortion parameters %s: run COLMAP's image_undistorter first and "
                           "read the undistorted model (undistortion is out of scope here)"
                           % (what, name, [float(p) for p in params[first:]]))
    if name in ("PINHOLE", "OPENCV"):
        fx, fy, cx, cy = (float(p) for p in params[:4])
    else:
        fx, cx, cy = (float(p) for p in params[:3])
        fy = fx
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)


def _data_lines(path):
    with open(path) as f:
        return [line.rstrip("\r\n") for line in f]


def _read_cameras_text(path):
    cams = {}
    for line in _data_lines(path):
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        f = line.split()
        if f[1] not in _MODEL_IDS:
            _intrinsics("camera %s" % f[0], f[1], [])
        cams[int(f[0])] = (_MODEL_IDS[f[1]], int(f[2]), int(f[3]), [float(x) for x in f[4:]])
    return cams


def _read_images_text(path):
    """-> [(id, qvec, tvec, camera_id, name, point ids)].  Two lines per image; the second may be empty.  A name may hold
    spaces: it is everything after the ninth field."""
    out, header = [], None
    for line in _data_lines(path):
        if line.lstrip().startswith("#"):
            continue
        if header is None:
            if not line.strip():
                continue
            f = line.split(None, 9)
            if len(f) < 10:
                raise RuntimeError("read_sfm_model: %s: an image line needs ID QW QX QY QZ TX TY TZ CAMERA_ID NAME, got %r"
                                   % (path, line))
            header = (int(f[0]), [float(x) for x in f[1:5]], [float(x) for x in f[5:8]], int(f[8]), f[9].strip())
        else:
            f = line.split()
            if len(f) % 3:
                raise RuntimeError("read_sfm_model: %s: the observations of image %d are not X Y POINT3D_ID triples"
                                   % (path, header[0]))
            out.append(header + (np.array([int(x) for x in f[2::3]], dtype=np.int64),))
            header = None
    if header is not None:
        out.append(header + (np.zeros(0, np.int64),))                          # (the file ended before an empty second line)
    return out


def _read_points_text(path):
    ids, xyz = [], []
    for line in _data_lines(path):
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        f = line.split()
        ids.append(int(f[0]))
        xyz.append([float(f[1]), float(f[2]), float(f[3])])
    return np.array(ids, dtype=np.int64), np.array(xyz, dtype=np.float64).reshape(-1, 3)


def _read_cameras_binary(path):
    buf, cams = open(path, "rb").read(), {}
    (count,), at = struct.unpack_from("<Q", buf, 0), 8
    for _ in range(count):
        cid, model, w, h = struct.unpack_from("<iiQQ", buf, at)
        at += 24
        if model not in CAMERA_MODELS:
            _intrinsics("camera %d" % cid, model, [])
        n = CAMERA_MODELS[model][1]
        cams[cid] = (model, int(w), int(h), list(struct.unpack_from("<%dd" % n, buf, at)))
        at += 8 * n
    return cams


_POINT2D = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])


def _read_images_binary(path):
    buf, out = open(path, "rb").read(), []
    (count,), at = struct.unpack_from("<Q", buf, 0), 8
    for _ in range(count):
        f = struct.unpack_from("<i7di", buf, at)
        at += 64
        end = buf.index(b"\0", at)
        name = buf[at:end].decode("utf-8")
        at = end + 1
        (n,) = struct.unpack_from("<Q", buf, at)
        at += 8
        ids = np.frombuffer(buf, _POINT2D, n, at)["id"].astype(np.int64)
        at += 24 * n
        out.append((f[0], list(f[1:5]), list(f[5:8]), f[8], name, ids))
    return out


def _read_points_binary(path):
    buf = open(path, "rb").read()
    (count,), at = struct.unpack_from("<Q", buf, 0), 8
    ids, xyz = np.zeros(count, np.int64), np.zeros((count, 3), np.float64)
    for k in range(count):
        pid, x, y, z = struct.unpack_from("<Q3d", buf, at)
        (track,) = struct.unpack_from("<Q", buf, at + 43)
        ids[k], xyz[k] = pid, (x, y, z)
        at += 51 + 8 * track
    return ids, xyz


def rotation_of(qvec):
    """Unit quaternions (w, x, y, z) [V,4] -> rotations [V,3,3] float64 (COLMAP's convention: x_cam = R X + t).  The
    quaternion is normalised first."""
    q = np.asarray(qvec, dtype=np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3), dtype=np.float64)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y
    return R


def structure(view_of_obs, point_of_obs, V, P):
    """Observations (view index, point index), in any order and with repeats -> ``view_ptr`` [V+1] int64, ``view_pts`` int32 (per
    view its sorted distinct points) and the transpose ``pt_ptr`` [P+1] int64, ``pt_views`` int32."""
    view_of_obs = np.asarray(view_of_obs, dtype=np.int64)
    point_of_obs = np.asarray(point_of_obs, dtype=np.int64)
    key = np.unique(view_of_obs * max(P, 1) + point_of_obs)                     # a point seen twice in a view counts once
    vi, pi = key // max(P, 1), key % max(P, 1)
    view_ptr = np.zeros(V + 1, np.int64)
    view_ptr[1:] = np.cumsum(np.bincount(vi, minlength=V))
    order = np.argsort(pi * max(V, 1) + vi, kind="stable")
    pt_ptr = np.zeros(P + 1, np.int64)
    pt_ptr[1:] = np.cumsum(np.bincount(pi, minlength=P))
    return dict(view_ptr=view_ptr, view_pts=pi.astype(np.int32), pt_ptr=pt_ptr, pt_views=vi[order].astype(np.int32))


def camera_record(model, w, h, params):
    """A camera of ``CAMERA_MODELS`` -> its record of ``CAMERA_RECORD`` doubles (csrc/undistort_math.h): model id, W, H, fx, fy,
    cx, cy, k1, k2, p1, p2, 0.  SIMPLE_PINHOLE and PINHOLE enter as SIMPLE_RADIAL and OPENCV with every distortion parameter 0."""
    p = [float(x) for x in params]
    if model in (1, 4):
        fx, fy, cx, cy = p[:4]
        dist = (p[4:8] if model == 4 else [0.0] * 4)
        mid = 4
    else:
        fx, cx, cy = p[:3]
        fy = fx
        dist = [p[3], p[4] if model == 3 else 0.0, 0.0, 0.0] if model in (2, 3) else [0.0] * 4
        mid = 3 if model == 3 else 2
    return np.array([mid, w, h, fx, fy, cx, cy] + dist + [0.0], dtype=np.float64)


def read_sfm_model(path, distortion="raise"):
    """``path/{cameras,images,points3D}.bin`` (preferred when both forms exist) or ``.txt`` -> dict.  Views are ordered by image
    id: ``image_ids`` [V] int64, ``names`` (list), ``camera_ids`` [V], ``qvecs`` [V,4] (w, x, y, z), ``tvecs`` [V,3], ``R``
    [V,3,3], ``centres`` [V,3] = -R^T t, ``K`` [V,3,3] at full resolution, ``sizes`` [V,2] int64 = (height, width), all float64
    unless said; ``point_ids`` [P] int64 ascending, ``points`` [P,3] float64; and the observation tables of ``structure``: per
    view the sorted distinct points it observes and the transpose.  Observations are the POINT3D_ID column of the images
    file (the track lists of the points file are not read); an id of -1, or one the points file does not hold, is dropped.
    PINHOLE and SIMPLE_PINHOLE cameras are taken, SIMPLE_RADIAL / RADIAL / OPENCV only when every distortion parameter is 0;
    anything else raises.  ``distortion="keep"``: SIMPLE_RADIAL, RADIAL and OPENCV cameras are taken with any finite
    parameters; ``K`` and ``sizes`` then describe the distorted cameras, and the dict also holds ``camera_table`` [C,12] float64
    (``camera_record`` of every camera a view names, by ascending camera id) and ``camera_row`` [V] int32, each view's row in
    it: what ``undistorted_cameras`` and ``undistort_images`` take.  Any other camera model raises in both modes."""
    if distortion not in ("raise", "keep"):
        raise RuntimeError("read_sfm_model: distortion = %r (\"raise\" or \"keep\")" % (distortion,))
    keep = distortion == "keep"
    def have(ext):
        return all(os.path.exists(os.path.join(path, n + ext)) for n in ("cameras", "images", "points3D"))
    if have(".bin"):
        cams = _read_cameras_binary(os.path.join(path, "cameras.bin"))
        images = _read_images_binary(os.path.join(path, "images.bin"))
        point_ids, points = _read_points_binary(os.path.join(path, "points3D.bin"))
    elif have(".txt"):
        cams = _read_cameras_text(os.path.join(path, "cameras.txt"))
        images = _read_images_text(os.path.join(path, "images.txt"))
        point_ids, points = _read_points_text(os.path.join(path, "points3D.txt"))
    else:
        raise RuntimeError("read_sfm_model: %s holds neither cameras.bin, images.bin and points3D.bin nor the three .txt files" % path)
    if not images:
        raise RuntimeError("read_sfm_model: %s lists no image" % path)
    images.sort(key=lambda im: im[0])
    ids = np.array([im[0] for im in images], dtype=np.int64)
    if len(np.unique(ids)) != len(ids) or len(np.unique(point_ids)) != len(point_ids):
        raise RuntimeError("read_sfm_model: %s repeats an image id or a point id" % path)
    order = np.argsort(point_ids, kind="stable")
    point_ids, points = point_ids[order], points[order]
    V, P = len(images), len(point_ids)
    K, sizes = np.zeros((V, 3, 3)), np.zeros((V, 2), np.int64)
    for v, im in enumerate(images):
        if im[3] not in cams:
            raise RuntimeError("read_sfm_model: image %d names camera %d, which cameras does not hold" % (im[0], im[3]))
        model, w, h, params = cams[im[3]]
        K[v] = _intrinsics("camera %d" % im[3], model, params, keep)
        sizes[v] = (h, w)
    qvecs = np.array([im[1] for im in images], dtype=np.float64).reshape(V, 4)
    tvecs = np.array([im[2] for im in images], dtype=np.float64).reshape(V, 3)
    R = rotation_of(qvecs)
    centres = -np.einsum("vji,vj->vi", R, tvecs)
    view_of = np.repeat(np.arange(V, dtype=np.int64), [len(im[5]) for im in images])
    pid = np.concatenate([im[5] for im in images]) if V else np.zeros(0, np.int64)
    at = np.searchsorted(point_ids, pid)
    known = (pid >= 0) & (at < P)
    known[known] = point_ids[at[known]] == pid[known]
    out = dict(image_ids=ids, names=[im[4] for im in images], camera_ids=np.array([im[3] for im in images], dtype=np.int64),
               qvecs=qvecs, tvecs=tvecs, R=R, centres=centres, K=K, sizes=sizes, point_ids=point_ids, points=points)
    out.update(structure(view_of[known], at[known], V, P))
    if keep:
        used = sorted(set(int(c) for c in out["camera_ids"]))
        out["camera_table"] = np.stack([camera_record(*cams[c]) for c in used])
        out["camera_row"] = np.searchsorted(np.array(used, dtype=np.int64), out["camera_ids"]).astype(np.int32)
    return out


# ---- the three launches -----------------------------------------------------------------------------------------------------------

def _device(what, device):
    if not torch.cuda.is_available():
        raise RuntimeError("mvster_amd.sfm.%s runs on MI355X only (there is no CPU fallback)" % what)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("mvster_amd.sfm.%s runs on MI355X only: device = %s (there is no CPU fallback)" % (what, dev))
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _check_params(what, theta0, sigma1, sigma2):
    theta0, sigma1, sigma2 = float(theta0), float(sigma1), float(sigma2)
    if not 0.0 <= theta0 <= 180.0:
        raise RuntimeError("%s: theta0 = %r (degrees, 0 .. 180)" % (what, theta0))
    for name, s in (("sigma1", sigma1), ("sigma2", sigma2)):
        if not (SIGMA_MIN <= s < float("inf")):
            raise RuntimeError("%s: %s = %r (degrees, at least %g: the error bound of the term holds from there)"
                               % (what, name, s, SIGMA_MIN))
    return theta0, sigma1, sigma2


def _check_num_src(what, num_src):
    if int(num_src) != num_src or not 1 <= int(num_src) <= MAX_SOURCES:
        raise RuntimeError("%s: num_src = %r (1 .. %d)" % (what, num_src, MAX_SOURCES))
    return int(num_src)


def _check_table(what, name, ptr, idx, rows, limit):
    """A CSR table on the host: ptr [rows+1] from 0, non-decreasing, ending at len(idx); idx within 0 .. limit-1."""
    if ptr.shape != (rows + 1,) or idx.ndim != 1:
        raise RuntimeError("%s: %s_ptr must be [%d] and the indices one-dimensional, got %s and %s"
                           % (what, name, rows + 1, ptr.shape, idx.shape))
    if ptr[0] != 0 or ptr[-1] != len(idx) or (np.diff(ptr) < 0).any():
        raise RuntimeError("%s: %s_ptr must rise from 0 to the number of indices (%d)" % (what, name, len(idx)))
    if len(idx) and (idx.min() < 0 or idx.max() >= limit):
        raise RuntimeError("%s: the %s table holds an index outside 0 .. %d" % (what, name, limit - 1))


def _check_views(what, V):
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError("%s: %d views (1 .. %d)" % (what, V, MAX_VIEWS))


def _f64(what, name, a, cols, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if t.dtype != torch.float64 or t.ndim != 2 or t.shape[1] != cols:
        raise RuntimeError("%s: %s must be [N,%d] float64, got %s %s" % (what, name, cols, tuple(t.shape), t.dtype))
    return t.to(dev).contiguous()


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _launch_pairs(lib, centres, points, pt_ptr_d, pt_views_d, item_ptr_d, total, params, q, stream):
    V, P = centres.shape[0], points.shape[0]
    _lib.check(lib.mvster_sfm_pair_scores(centres.data_ptr(), V, _ptr(points), P, pt_ptr_d.data_ptr(), _ptr(pt_views_d),
                                          pt_views_d.numel(), item_ptr_d.data_ptr(), total, params[0], params[1], params[2],
                                          q.data_ptr(), stream), "sfm_pair_scores")


def _items(pt_ptr):
    """-> (item_ptr [P+1] int64: the prefix sum of L (L - 1) / 2, total)"""
    L = np.diff(pt_ptr)
    item_ptr = np.zeros(len(pt_ptr), np.int64)
    item_ptr[1:] = np.cumsum(L * (L - 1) // 2)
    return item_ptr, int(item_ptr[-1])


def pair_scores(centres, points, pt_ptr, pt_views, theta0=5.0, sigma1=1.0, sigma2=10.0, device=None, out=None):
    """``q`` [V,V] int64 on the GPU: the quantised scores (units of 2^-32) of all pairs of views.  ``centres`` [V,3] and ``points``
    [P,3] float64 (arrays, or tensors on the GPU); ``pt_ptr`` [P+1] / ``pt_views``: per point its sorted distinct views, on
    the host (``structure``) -- they are checked there, and the prefix sum over the pairs of every track is formed there.
    Integer atomics only: two runs give the same bytes.  ``out``: an int64 [V,V] tensor on the GPU to fill.  No read-back."""
    what = "pair_scores"
    params = _check_params(what, theta0, sigma1, sigma2)
    dev = _device(what, device)
    centres, points = _f64(what, "centres", centres, 3, dev), _f64(what, "points", points, 3, dev)
    V, P = centres.shape[0], points.shape[0]
    _check_views(what, V)
    pt_ptr, pt_views = _host(pt_ptr, np.int64), _host(pt_views, np.int32)
    _check_table(what, "pt", pt_ptr, pt_views, P, V)
    if (np.diff(pt_ptr) > V).any():
        raise RuntimeError("%s: a track is longer than the %d views: its views are not distinct" % (what, V))
    item_ptr, total = _items(pt_ptr)
    q = torch.empty(V, V, device=dev, dtype=torch.int64) if out is None else out
    if q.shape != (V, V) or q.dtype != torch.int64 or q.device != dev or not q.is_contiguous():
        raise RuntimeError("%s: out must be a contiguous int64 [%d,%d] tensor on %s" % (what, V, V, dev))
    with torch.cuda.device(dev):
        _launch_pairs(_lib.load(), centres, points, torch.from_numpy(pt_ptr).to(dev), torch.from_numpy(pt_views).to(dev),
                      torch.from_numpy(item_ptr).to(dev), total, params, q, torch.cuda.current_stream(dev).cuda_stream)
    return q


def depth_ranges(rt, points, view_ptr, view_pts, device=None):
    """Per view, on the GPU: ``n`` [V] int32 = its distinct points with a finite depth > 0, ``depth_min`` / ``depth_max`` [V]
    float64 = the depths of rank n // 100 and 99 n // 100 in ascending order (NaN for n = 0), by an exact radix selection.
    ``rt`` [V,4] float64 = the third row of R and t_z; ``points`` [P,3] float64; ``view_ptr`` [V+1] / ``view_pts``: per view its
    sorted distinct points, on the host.  -> (n, depth_min, depth_max).  No read-back."""
    what = "depth_ranges"
    dev = _device(what, device)
    rt, points = _f64(what, "rt", rt, 4, dev), _f64(what, "points", points, 3, dev)
    V, P = rt.shape[0], points.shape[0]
    _check_views(what, V)
    view_ptr, view_pts = _host(view_ptr, np.int64), _host(view_pts, np.int32)
    _check_table(what, "view", view_ptr, view_pts, V, P)
    n = torch.empty(V, device=dev, dtype=torch.int32)
    lo, hi = torch.empty(V, device=dev, dtype=torch.float64), torch.empty(V, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        vp, vi = torch.from_numpy(view_ptr).to(dev), torch.from_numpy(view_pts).to(dev)
        _lib.check(_lib.load().mvster_sfm_depth_ranges(rt.data_ptr(), V, _ptr(points), P, vp.data_ptr(), _ptr(vi), vi.numel(),
                                                       n.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream), "sfm_depth_ranges")
    return n, lo, hi


def select_sources(q, num_src=10):
    """Per row of ``q`` (int64 [V,V] on the GPU): the first ``num_src`` (1 .. 64) views j != i with q[i][j] > 0 in (q
    descending, j ascending) order -> ``index`` [V,num_src] int32 (-1 where the list ends), ``value`` [V,num_src] int64 (0
    there), ``count`` [V] int32, on the GPU.  No read-back."""
    what = "select_sources"
    num_src = _check_num_src(what, num_src)
    if not torch.is_tensor(q) or q.ndim != 2 or q.shape[0] != q.shape[1] or q.dtype != torch.int64:
        raise RuntimeError("%s: q must be an int64 [V,V] tensor" % what)
    if q.device.type != "cuda":
        raise RuntimeError("mvster_amd.sfm.%s runs on MI355X only: q is on %s (there is no CPU fallback)" % (what, q.device))
    V, dev = q.shape[0], q.device
    _check_views(what, V)
    q = q.contiguous()
    index = torch.empty(V, num_src, device=dev, dtype=torch.int32)
    value = torch.empty(V, num_src, device=dev, dtype=torch.int64)
    count = torch.empty(V, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvster_sfm_select_sources(q.data_ptr(), V, num_src, index.data_ptr(), value.data_ptr(),
                                                         count.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "sfm_select_sources")
    return index, value, count


def depth_rows(model):
    """``rt`` [V,4] float64 of ``depth_ranges``: the third row of every rotation and t_z."""
    return np.ascontiguousarray(np.concatenate([model["R"][:, 2, :], model["tvecs"][:, 2:3]], axis=1), dtype=np.float64)


def view_graph(model, theta0=5.0, sigma1=1.0, sigma2=10.0, num_src=10, device=None):
    """The view graph of a model (``read_sfm_model``) -> dict of host arrays: ``q`` int64 [V,V], ``score`` float64 [V,V] =
    q / 2^32 (exact), ``src_index`` [V,num_src] int32, ``src_q`` [V,num_src] int64, ``src_count`` [V] int32, ``pairs`` =
    [(view, [sources])] as ``formats.read_pair_file`` (views without sources left out) with ``pair_scores`` the lists of their
    scores, ``n_obs`` [V] int32, ``depth_min`` / ``depth_max`` [V] float64 (NaN where n_obs = 0).  Five launches on one stream;
    every result lands in one device buffer and comes back in ONE read-back."""
    what = "view_graph"
    params = _check_params(what, theta0, sigma1, sigma2)
    ns = _check_num_src(what, num_src)
    dev = _device(what, device)
    V, P = len(model["image_ids"]), len(model["point_ids"])
    _check_views(what, V)
    for name, rows, limit in (("view", V, P), ("pt", P, V)):
        _check_table(what, name, model[name + "_ptr"], model[name + ("_pts" if name == "view" else "_views")], rows, limit)
    item_ptr, total = _items(model["pt_ptr"])
    lib = _lib.load()
    sizes = (V * V * 8, V * ns * 8, V * ns * 4, V * 4, V * 4, V * 8, V * 8)    # q, src_q, src_index, src_count, n, min, max
    starts = np.concatenate([[0], np.cumsum([(s + 7) // 8 * 8 for s in sizes])])
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        centres, points, rt = up(model["centres"], np.float64), up(model["points"], np.float64), up(depth_rows(model), np.float64)
        pt_ptr, pt_views = up(model["pt_ptr"], np.int64), up(model["pt_views"], np.int32)
        view_ptr, view_pts = up(model["view_ptr"], np.int64), up(model["view_pts"], np.int32)
        buf = torch.empty(int(starts[-1]), device=dev, dtype=torch.uint8)
        part = [buf[int(starts[k]):int(starts[k]) + sizes[k]] for k in range(len(sizes))]
        q = part[0].view(torch.int64).view(V, V)
        _launch_pairs(lib, centres, points, pt_ptr, pt_views, up(item_ptr, np.int64), total, params, q, stream)
        _lib.check(lib.mvster_sfm_select_sources(q.data_ptr(), V, ns, part[2].data_ptr(), part[1].data_ptr(), part[3].data_ptr(),
                                                 stream), "sfm_select_sources")
        _lib.check(lib.mvster_sfm_depth_ranges(rt.data_ptr(), V, _ptr(points), P, view_ptr.data_ptr(), _ptr(view_pts),
                                               view_pts.numel(), part[4].data_ptr(), part[5].data_ptr(), part[6].data_ptr(),
                                               stream), "sfm_depth_ranges")
        host = buf.cpu().numpy()                                                # the one read-back
    got = [host[int(starts[k]):int(starts[k]) + sizes[k]] for k in range(len(sizes))]
    out = dict(q=got[0].view(np.int64).reshape(V, V).copy(), src_q=got[1].view(np.int64).reshape(V, ns).copy(),
               src_index=got[2].view(np.int32).reshape(V, ns).copy(), src_count=got[3].view(np.int32).copy(),
               n_obs=got[4].view(np.int32).copy(), depth_min=got[5].view(np.float64).copy(),
               depth_max=got[6].view(np.float64).copy())
    out["score"] = out["q"].astype(np.float64) / TWO32
    out["pairs"], out["pair_scores"] = source_lists(out["src_index"], out["src_q"], out["src_count"])
    return out


def source_lists(src_index, src_q, src_count):
    """The selection's arrays -> (pairs [(view, [sources])], scores [[float]]); a view without sources is left out."""
    pairs, scores = [], []
    for v in range(len(src_count)):
        c = int(src_count[v])
        if c:
            pairs.append((v, [int(j) for j in src_index[v, :c]]))
            scores.append([float(s) / TWO32 for s in src_q[v, :c]])
    return pairs, scores


# ---- undistortion -------------------------------------------------------------------------------------------------------------------

def _check_camera_table(what, camera_table):
    """-> the table as a contiguous [C,12] float64 host array; every record must be one the kernels take"""
    t = _host(camera_table, np.float64)
    if t.ndim != 2 or t.shape[1] != CAMERA_RECORD or not len(t):
        raise RuntimeError("%s: camera_table must be [C,%d] float64 with C >= 1, got %s" % (what, CAMERA_RECORD, t.shape))
    if not np.isfinite(t).all():
        raise RuntimeError("%s: camera_table holds a value that is not finite" % what)
    for r, c in enumerate(t):
        if c[0] not in (2.0, 3.0, 4.0):
            raise RuntimeError("%s: camera row %d has model id %r; SIMPLE_RADIAL (2), RADIAL (3) and OPENCV (4) are taken" % (what, r, c[0]))
        if c[1] != int(c[1]) or c[2] != int(c[2]) or not (1 <= c[1] <= MAX_SIDE and 1 <= c[2] <= MAX_SIDE):
            raise RuntimeError("%s: camera row %d is %r x %r pixels (whole numbers, 1 .. %d)" % (what, r, c[1], c[2], MAX_SIDE))
        if not (c[3] > 0 and c[4] > 0):
            raise RuntimeError("%s: camera row %d has focal lengths %r, %r" % (what, r, c[3], c[4]))
    return t


def _check_rows(what, camera_row, count, C):
    rows = _host(camera_row, np.int32)
    if rows.shape != (count,):
        raise RuntimeError("%s: camera_row must be [%d], got %s" % (what, count, rows.shape))
    if count and (rows.min() < 0 or rows.max() >= C):
        raise RuntimeError("%s: camera_row holds a row outside 0 .. %d" % (what, C - 1))
    return rows


def _check_scales(what, blank_pixels, min_scale, max_scale, scale):
    blank, lo, hi = float(blank_pixels), float(min_scale), float(max_scale)
    if not 0.0 <= blank <= 1.0:
        raise RuntimeError("%s: blank_pixels = %r (0 .. 1)" % (what, blank_pixels))
    if not 0.0 < lo <= hi <= MAX_SCALE:
        raise RuntimeError("%s: min_scale = %r, max_scale = %r (0 < min_scale <= max_scale <= %g)" % (what, min_scale, max_scale, MAX_SCALE))
    if scale is not None:
        try:
            sx, sy = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise RuntimeError("%s: scale = %r (None or a pair (scale_x, scale_y))" % (what, scale))
        if not (0.0 < sx <= MAX_SCALE and 0.0 < sy <= MAX_SCALE):
            raise RuntimeError("%s: scale = %r (both within (0, %g])" % (what, scale, MAX_SCALE))
        scale = (sx, sy)
    return blank, lo, hi, scale


def _cameras_of(what, table):
    """The kernel's [C,8] -> the dict of ``undistorted_cameras``; raises on a camera whose distortion cannot be inverted"""
    C = len(table)
    for r in range(C):
        if not table[r, 6] <= RESIDUAL_BOUND:
            raise RuntimeError("%s: camera row %d: the distortion cannot be inverted over the image: %d of its border pixels "
                               "keep a residual above %g after the Newton steps (the worst: %g, normalised units)"
                               % (what, r, int(table[r, 7]), RESIDUAL_BOUND, table[r, 6]))
    K = np.zeros((C, 3, 3), np.float64)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = table[:, 2], table[:, 3], table[:, 4], table[:, 5], 1.0
    return dict(sizes=table[:, [1, 0]].astype(np.int64), K=K, residual=table[:, 6].copy(), table=table)


def undistorted_cameras(camera_table, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, scale=None, device=None):
    """The PINHOLE camera of every camera's undistorted image.  ``camera_table`` [C,12] float64 (``read_sfm_model(...,
    distortion="keep")``).  The border pixel centres are undistorted (ten Newton steps each) and projected; from their extremes
    come the per-axis scales at which no blank pixel shows (``blank_pixels=0``) or every source pixel is kept (1), clamped to
    ``min_scale .. max_scale``; W' = max(1, int(scale_x W)), cx' = cx W' / W, the focal lengths stay.  ``scale=(sx, sy)`` sets the
    scales and skips the border.  -> dict of host arrays after ONE read-back: ``sizes`` [C,2] int64 = (height, width), ``K``
    [C,3,3], ``residual`` [C] (the worst over the border, normalised units) and ``table`` [C,8], what ``undistort_images``
    takes.  Raises when a residual exceeds 1e-9: that camera's distortion cannot be inverted over its image."""
    what = "undistorted_cameras"
    blank, lo, hi, scale = _check_scales(what, blank_pixels, min_scale, max_scale, scale)
    table = _check_camera_table(what, camera_table)
    dev = _device(what, device)
    with torch.cuda.device(dev):
        cams = torch.from_numpy(table).to(dev)
        out = torch.empty(len(table), 8, device=dev, dtype=torch.float64)
        sx, sy = scale if scale is not None else (1.0, 1.0)
        _lib.check(_lib.load().mvster_undistort_cameras(cams.data_ptr(), len(table), blank, lo, hi, int(scale is not None), sx, sy,
                                                        out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "undistort_cameras")
        got = out.cpu().numpy()                                                 # the one read-back
    return _cameras_of(what, got)


def _points(what, direction, camera_table, camera_row, xy, device):
    table = _check_camera_table(what, camera_table)
    if not torch.is_tensor(xy):
        xy = torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float64))
    if xy.dtype != torch.float64 or xy.ndim != 2 or xy.shape[1] != 2:
        raise RuntimeError("%s: xy must be [N,2] float64, got %s %s" % (what, tuple(xy.shape), xy.dtype))
    N = xy.shape[0]
    rows = _check_rows(what, camera_row, N, len(table))
    dev = _device(what, device)
    with torch.cuda.device(dev):
        xy = xy.to(dev).contiguous()
        out = torch.empty(N, 2, device=dev, dtype=torch.float64)
        residual = torch.empty(N, device=dev, dtype=torch.float64)
        if N:
            cams, rows_d = torch.from_numpy(table).to(dev), torch.from_numpy(rows).to(dev)
            _lib.check(_lib.load().mvster_undistort_points(cams.data_ptr(), len(table), rows_d.data_ptr(), N, direction, xy.data_ptr(),
                                                           out.data_ptr(), residual.data_ptr(),
                                                           torch.cuda.current_stream(dev).cuda_stream), "undistort_points")
    return out, residual


def undistort_points(camera_table, camera_row, xy, device=None):
    """``xy`` [N,2] float64 (array or tensor), pixel coordinates in the distorted images of the cameras ``camera_row`` [N] names
    -> (``xy'`` [N,2], ``residual`` [N]) float64 on the GPU: the points without the distortion, in the pixels of the SAME fx,
    fy, cx, cy (apply an undistorted camera's cx' - cx yourself), and what the ten Newton steps left (normalised units; +inf
    where they stopped: a determinant <= 0 or an iterate that is not finite).  No read-back."""
    return _points("undistort_points", 1, camera_table, camera_row, xy, device)


def distort_points(camera_table, camera_row, xy, device=None):
    """The other direction of ``undistort_points`` -> ``xy'`` [N,2] float64 on the GPU.  No read-back."""
    return _points("distort_points", 0, camera_table, camera_row, xy, device)[0]


def _round16(n):
    return (int(n) + 15) // 16 * 16


def undistort_images(images, camera_table, camera_row, cameras=None, chunk_bytes=1 << 30, keep_on_device=False, device=None):
    """``images``: a list of uint8 [H,W,3] arrays or tensors (host or GPU), image k taken by camera ``camera_row[k]`` of
    ``camera_table`` -> (``images'``, ``valid``, ``cameras``): the undistorted images (uint8 [H',W',3]), per image a uint8 [H',W']
    mask (0 where the pixel looks outside the source; such a pixel is black), and the dict of ``undistorted_cameras`` (made
    with its defaults when ``cameras`` is None).  The list is worked through in chunks of at most ``chunk_bytes`` of source
    (an image larger than that is a chunk of its own): one upload, ONE launch and one read-back per chunk.
    ``keep_on_device=True`` returns GPU tensors and reads nothing back.  An image whose size differs from its camera's raises."""
    what = "undistort_images"
    if int(chunk_bytes) != chunk_bytes or int(chunk_bytes) < 1:
        raise RuntimeError("%s: chunk_bytes = %r (a whole number of bytes, at least 1)" % (what, chunk_bytes))
    table = _check_camera_table(what, camera_table)
    images = list(images)
    rows = _check_rows(what, camera_row, len(images), len(table))
    for k, img in enumerate(images):
        if not torch.is_tensor(img):
            images[k] = img = np.asarray(img)
        dtype_ok = img.dtype == (torch.uint8 if torch.is_tensor(img) else np.uint8)
        if not dtype_ok or img.ndim != 3 or img.shape[2] != 3:
            raise RuntimeError("%s: image %d must be uint8 [H,W,3], got %s %s" % (what, k, tuple(img.shape), img.dtype))
        H, W = int(table[rows[k], 2]), int(table[rows[k], 1])
        if tuple(img.shape[:2]) != (H, W):
            raise RuntimeError("%s: image %d is %dx%d but its camera (row %d) says %dx%d"
                               % (what, k, img.shape[0], img.shape[1], rows[k], H, W))
    if cameras is not None:
        ucam = _host(cameras["table"], np.float64)
        if ucam.shape != (len(table), 8):
            raise RuntimeError("%s: cameras[\"table\"] must be [%d,8], got %s" % (what, len(table), ucam.shape))
        cameras = _cameras_of(what, ucam)
    dev = _device(what, device)
    if cameras is None:
        cameras = undistorted_cameras(table, device=dev)
    ucam = np.ascontiguousarray(cameras["table"], dtype=np.float64)
    chunks, start, used = [], 0, 0
    for k, img in enumerate(images):                                             # chunks of at most chunk_bytes of source
        n = 3 * img.shape[0] * img.shape[1]
        if k > start and used + n > int(chunk_bytes):
            chunks.append((start, k))
            start, used = k, 0
        used += n
    if images:
        chunks.append((start, len(images)))
    out_images, out_valid = [], []
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        cams_d, ucam_d = torch.from_numpy(table).to(dev), torch.from_numpy(ucam).to(dev)
        for lo, hi in chunks:
            V = hi - lo
            views, group_ptr = np.zeros((V, 8), np.int64), np.zeros(V + 1, np.int64)
            order = [k for k in range(lo, hi) if not torch.is_tensor(images[k])] + [k for k in range(lo, hi) if torch.is_tensor(images[k])]
            src_at, dst_at, valid_at = 0, 0, 0
            for k in order:                                                    # host images first: they go up in one copy
                Hs, Ws = images[k].shape[:2]
                Hd, Wd = (int(s) for s in cameras["sizes"][rows[k]])
                views[k - lo] = (src_at, dst_at, valid_at, Hs, Ws, Hd, Wd, rows[k])
                src_at, dst_at, valid_at = src_at + 3 * Hs * Ws, dst_at + _round16(3 * Hd * Wd), valid_at + _round16(Hd * Wd)
            group_ptr[1:] = np.cumsum((views[:, 5] * views[:, 6] + 3) // 4)
            src = torch.empty(src_at, device=dev, dtype=torch.uint8)
            host = [images[k].reshape(-1) for k in order if not torch.is_tensor(images[k])]
            if host:
                block = torch.from_numpy(np.concatenate(host) if len(host) > 1 else np.ascontiguousarray(host[0]))
                src[:block.numel()].copy_(block)                                # the one upload
            for k in order:
                if torch.is_tensor(images[k]):
                    at = int(views[k - lo, 0])
                    src[at:at + images[k].numel()].copy_(images[k].reshape(-1))
            out = torch.empty(dst_at + valid_at, device=dev, dtype=torch.uint8)   # images, then masks: one buffer, one read-back
            tables = torch.from_numpy(np.concatenate([views.reshape(-1), group_ptr])).to(dev)
            _lib.check(lib.mvster_undistort_images(src.data_ptr(), src_at, out.data_ptr(), dst_at, out.data_ptr() + dst_at, valid_at,
                                                   tables.data_ptr(), tables.data_ptr() + views.size * 8, V, int(group_ptr[-1]),
                                                   cams_d.data_ptr(), ucam_d.data_ptr(), len(table), stream), "undistort_images")
            got = out if keep_on_device else out.cpu().numpy()                  # (the chunk's one read-back)
            for k in range(lo, hi):
                _, d, m, _, _, Hd, Wd, _ = (int(x) for x in views[k - lo])
                img, mask = got[d:d + 3 * Hd * Wd], got[dst_at + m:dst_at + m + Hd * Wd]
                out_images.append(img.view(Hd, Wd, 3) if keep_on_device else img.reshape(Hd, Wd, 3).copy())
                out_valid.append(mask.view(Hd, Wd) if keep_on_device else mask.reshape(Hd, Wd).copy())
    return out_images, out_valid, cameras


# ---- to a scan ------------------------------------------------------------------------------------------------------------------------

def assemble_scan(model, graph, load_image, K=None, transform=None):
    """A model (``read_sfm_model``), its ``view_graph`` and ``load_image(view) -> uint8 [H,W,3]`` -> the scan dict of
    ``scan_from_sfm``.  Host work only, unless ``transform`` does more.  ``K`` [V,3,3]: the views' full-resolution intrinsics in
    place of the model's; ``transform(images, kept views) -> (images, dict of further entries)`` is applied to the loaded
    (and size-checked) images of the kept views: how ``scan_from_sfm(..., undistort=True)`` puts undistorted images, their
    cameras and their ``valid`` masks into the scan."""
    keep = np.nonzero(graph["n_obs"] > 0)[0]
    if not len(keep):
        raise RuntimeError("scan_from_sfm: no view of the model has a sparse point in front of it")
    slot = {int(v): k for k, v in enumerate(keep)}
    images = []
    for v in keep:
        img = np.asarray(load_image(int(v)), dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3 or tuple(img.shape[:2]) != tuple(int(s) for s in model["sizes"][v]):
            raise RuntimeError("scan_from_sfm: image %s is %s but its camera says %dx%d: the images must be the ones the "
                               "model was made from" % (model["names"][v], tuple(img.shape), *model["sizes"][v]))
        images.append(img)
    Es = np.zeros((len(keep), 4, 4), dtype=np.float32)
    Es[:, :3, :3], Es[:, :3, 3], Es[:, 3, 3] = model["R"][keep], model["tvecs"][keep], 1.0
    pairs, scores = [], []
    for (v, srcs), sc in zip(graph["pairs"], graph["pair_scores"]):
        if v not in slot:
            continue
        kept = [(slot[j], s) for j, s in zip(srcs, sc) if j in slot]
        if kept:
            pairs.append((slot[v], [j for j, _ in kept]))
            scores.append([s for _, s in kept])
    more = {}
    if transform is not None:
        images, more = transform(images, keep)
    Kfull = model["K"] if K is None else np.asarray(K, dtype=np.float64)
    return dict(more, images=images, Ks=formats._quarter(Kfull[keep].astype(np.float32)), Es=Es,
                depth_ranges=[(float(graph["depth_min"][v]), float(graph["depth_max"][v])) for v in keep], pairs=pairs,
                pair_scores=scores, view_ids=[int(model["image_ids"][v]) for v in keep],
                names=[model["names"][v] for v in keep],
                dropped_views=[int(model["image_ids"][v]) for v in np.nonzero(graph["n_obs"] <= 0)[0]])


def scan_from_sfm(model_dir, image_dir, theta0=5.0, sigma1=1.0, sigma2=10.0, num_src=10, device=None, undistort=False,
                  blank_pixels=0.0, keep_on_device=False):
    """A COLMAP sparse model and its (undistorted) images -> the dict ``scan.read_scan_folder`` returns: ``images`` (list of
    uint8 [H,W,3], ``image_dir/<name>``), ``Ks`` [V,3,3] float32 in the quarter-resolution convention (rows 0-1 divided by 4),
    ``Es`` [V,4,4] float32, ``depth_ranges`` = [(depth_min, depth_max)] for ``depth_range_kind="min_max"``, ``pairs`` (indices
    into the views) with ``pair_scores``, ``view_ids`` (the image ids) and ``names``; ``dropped_views``: the image ids of the
    views without a single sparse point in front of them, which have no depth range and are left out (of the lists of the
    others too, which are not filled up again).  A view may have fewer than ``num_src`` sources: run ``infer_scan`` /
    ``reconstruct_scan`` with ``short_sources="fewer_views"``, ``depth_range_kind="min_max"`` and ``max_h=`` / ``max_w=`` or
    ``img_wh=``.

    ``undistort=True``: the model is read with ``distortion="keep"`` and ``image_dir`` holds the photographs the model was made
    from.  The view graph is the same (it depends on the poses and the sparse points only); the images of the kept views are
    undistorted on the GPU (``undistort_images``, ``blank_pixels`` as in ``undistorted_cameras``), ``Ks`` are the undistorted
    cameras' and ``valid`` lists a uint8 [H',W'] mask per view.  ``keep_on_device=True`` leaves images and masks on the GPU, as
    ``infer_scan`` takes them.  A model without distortion goes the same way: its cameras are then rescaled by the border rule
    (ideally scale 1, but a size may lose a pixel to rounding), and the images are resampled once."""
    from PIL import Image
    if not undistort and (blank_pixels != 0.0 or keep_on_device):
        raise RuntimeError("scan_from_sfm: blank_pixels and keep_on_device belong to undistort=True")
    if undistort:
        _check_scales("scan_from_sfm", blank_pixels, 0.2, 2.0, None)
    model = read_sfm_model(model_dir, distortion="keep" if undistort else "raise")
    load = lambda v: np.array(Image.open(os.path.join(image_dir, model["names"][v])).convert("RGB"), dtype=np.uint8)
    graph = view_graph(model, theta0, sigma1, sigma2, num_src, device)
    if not undistort:
        return assemble_scan(model, graph, load)
    cams = undistorted_cameras(model["camera_table"], blank_pixels, device=device)

    def transform(images, keep):
        out, valid, _ = undistort_images(images, model["camera_table"], model["camera_row"][keep], cameras=cams,
                                         keep_on_device=keep_on_device, device=device)
        return out, dict(valid=valid)
    return assemble_scan(model, graph, load, K=cams["K"][model["camera_row"]], transform=transform)


def write_scan_folder(scan, root, ndepths=192):
    """Write ``root/images/%08d.jpg``, ``root/cams/%08d_cam.txt`` and ``root/pair.txt`` (with scores) for a scan dict of
    ``scan_from_sfm``, numbered by ``view_ids``: the folder ``read_scan_folder(root, "", dataset="tanks")`` reads.  The cam
    files hold the full-resolution intrinsics (the float32 values, in their shortest spelling) and on line 11 ``depth_min
    (depth_max - depth_min) / ndepths ndepths depth_max`` with the float64 values spelled exactly, so
    ``formats.read_cam_file_minmax`` gives (min, max) back and ``formats.read_cam_file(..., ndepths)`` min and that interval.
    A view no list names and which has no sources does not come back from ``read_scan_folder``, which takes its views from
    pair.txt."""
    from PIL import Image
    ndepths = int(ndepths)
    if ndepths < 1:
        raise RuntimeError("write_scan_folder: ndepths = %d" % ndepths)
    ids = [int(v) for v in scan["view_ids"]]
    V = len(ids)
    Ks, Es = np.asarray(scan["Ks"], dtype=np.float32), np.asarray(scan["Es"], dtype=np.float32)
    if Ks.shape != (V, 3, 3) or Es.shape != (V, 4, 4) or len(scan["images"]) != V or len(scan["depth_ranges"]) != V:
        raise RuntimeError("write_scan_folder: %d view_ids but Ks %s, Es %s, %d images, %d depth_ranges"
                           % (V, Ks.shape, Es.shape, len(scan["images"]), len(scan["depth_ranges"])))
    for sub in ("images", "cams"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for v in range(V):
        name = "{:0>8}".format(ids[v])
        Image.fromarray(_host(scan["images"][v], np.uint8)).save(os.path.join(root, "images", name + ".jpg"))
        K = Ks[v].copy()
        K[:2, :] *= 4.0                                                         # exact: back to full resolution
        lo, hi = float(scan["depth_ranges"][v][0]), float(scan["depth_ranges"][v][1])
        with open(os.path.join(root, "cams", name + "_cam.txt"), "w") as f:
            f.write("extrinsic\n")
            for r in range(4):
                f.write(" ".join(str(x) for x in Es[v, r]) + "\n")
            f.write("\nintrinsic\n")
            for r in range(3):
                f.write(" ".join(str(x) for x in K[r]) + "\n")
            f.write("\n%r %r %d %r\n" % (lo, (hi - lo) / ndepths, ndepths, hi))
    lists = {int(r): ([int(j) for j in srcs], sc) for (r, srcs), sc in
             zip(scan["pairs"], scan.get("pair_scores") or [[0.0] * len(s) for _, s in scan["pairs"]])}
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write("%d\n" % V)
        for v in range(V):
            srcs, sc = lists.get(v, ([], []))
            f.write("%d\n%d" % (ids[v], len(srcs)))
            for j, s in zip(srcs, sc):
                f.write(" %d %r" % (ids[j], float(s)))
            f.write("\n")
