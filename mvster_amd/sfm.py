"""A scan from a structure-from-motion model: read a COLMAP sparse model (text or binary), score every
pair of views over the sparse points both see, list each view's best sources and take each view's depth range from the
percentiles of its sparse depths -- on the GPU (csrc/geo_sfm.hip; the definition is csrc/sfm_math.h) -- and hand ``infer_scan`` /
``reconstruct_scan`` the dict ``scan.read_scan_folder`` returns, or write the scan folder it reads.

The definition is this project's own, written out in sfm_math.h; where it departs from the customary conversion scripts of the
MVSNet family (a point seen twice in an image counts once; a partner with score zero is never listed; only finite depths
z > 0 enter the range) DESIGN.md says so.  Undistortion is out of scope: a model with distortion raises and names COLMAP's
``image_undistorter``.  There is no CPU fallback for the three launches."""
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


# ---- reading a model -------------------------------------------------------------------------------------------------------------

def _intrinsics(what, model, params):
    """-> K [3,3] float64 of a camera without distortion; anything else raises."""
    if model not in CAMERA_MODELS:
        raise RuntimeError("read_sfm_model: %s has camera model %r; only SIMPLE_PINHOLE, PINHOLE and the SIMPLE_RADIAL / RADIAL / "
                           "OPENCV models with every distortion parameter 0 are taken: run COLMAP's image_undistorter first "
                           "(undistortion is out of scope here)" % (what, model))
    name, count, first = CAMERA_MODELS[model]
    if len(params) != count:
        raise RuntimeError("read_sfm_model: %s (%s) has %d parameters, not %d" % (what, name, len(params), count))
    if any(float(p) != 0.0 for p in params[first:]):
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


def read_sfm_model(path):
    """``path/{cameras,images,points3D}.bin`` (preferred when both forms exist) or ``.txt`` -> dict.  Views are ordered by image
    id: ``image_ids`` [V] int64, ``names`` (list), ``camera_ids`` [V], ``qvecs`` [V,4] (w, x, y, z), ``tvecs`` [V,3], ``R``
    [V,3,3], ``centres`` [V,3] = -R^T t, ``K`` [V,3,3] at full resolution, ``sizes`` [V,2] int64 = (height, width), all float64
    unless said; ``point_ids`` [P] int64 ascending, ``points`` [P,3] float64; and the observation tables of ``structure``: per
    view the sorted distinct points it observes and the transpose.  Observations are the POINT3D_ID column of the images
    file (the track lists of the points file are not read); an id of -1, or one the points file does not hold, is dropped.
    PINHOLE and SIMPLE_PINHOLE cameras are taken, SIMPLE_RADIAL / RADIAL / OPENCV only when every distortion parameter is 0;
    anything else raises."""
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
        K[v] = _intrinsics("camera %d" % im[3], model, params)
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


# ---- to a scan ------------------------------------------------------------------------------------------------------------------------

def assemble_scan(model, graph, load_image):
    """A model (``read_sfm_model``), its ``view_graph`` and ``load_image(view) -> uint8 [H,W,3]`` -> the scan dict of
    ``scan_from_sfm``.  Host work only."""
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
    return dict(images=images, Ks=formats._quarter(model["K"][keep].astype(np.float32)), Es=Es,
                depth_ranges=[(float(graph["depth_min"][v]), float(graph["depth_max"][v])) for v in keep], pairs=pairs,
                pair_scores=scores, view_ids=[int(model["image_ids"][v]) for v in keep],
                names=[model["names"][v] for v in keep],
                dropped_views=[int(model["image_ids"][v]) for v in np.nonzero(graph["n_obs"] <= 0)[0]])


def scan_from_sfm(model_dir, image_dir, theta0=5.0, sigma1=1.0, sigma2=10.0, num_src=10, device=None):
    """A COLMAP sparse model and its (undistorted) images -> the dict ``scan.read_scan_folder`` returns: ``images`` (list of
    uint8 [H,W,3], ``image_dir/<name>``), ``Ks`` [V,3,3] float32 in the quarter-resolution convention (rows 0-1 divided by 4),
    ``Es`` [V,4,4] float32, ``depth_ranges`` = [(depth_min, depth_max)] for ``depth_range_kind="min_max"``, ``pairs`` (indices
    into the views) with ``pair_scores``, ``view_ids`` (the image ids) and ``names``; ``dropped_views``: the image ids of the
    views without a single sparse point in front of them, which have no depth range and are left out (of the lists of the
    others too, which are not filled up again).  A view may have fewer than ``num_src`` sources: run ``infer_scan`` /
    ``reconstruct_scan`` with ``short_sources="fewer_views"``, ``depth_range_kind="min_max"`` and ``max_h=`` / ``max_w=`` or
    ``img_wh=``."""
    from PIL import Image
    model = read_sfm_model(model_dir)
    graph = view_graph(model, theta0, sigma1, sigma2, num_src, device)
    return assemble_scan(model, graph, lambda v: np.array(Image.open(os.path.join(image_dir, model["names"][v])).convert("RGB"),
                                                          dtype=np.uint8))


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
        Image.fromarray(np.asarray(scan["images"][v], dtype=np.uint8)).save(os.path.join(root, "images", name + ".jpg"))
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
