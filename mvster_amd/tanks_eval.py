"""The Tanks and Temples evaluation protocol on the GPU: what the benchmark's evaluation does before
and while it measures distances -- move the reconstruction into the ground truth's frame, crop both clouds to the scene's polygon
volume (``crop_points``), refine the alignment with three rounds of ICP on thinned clouds (``register_clouds``), thin both clouds
at tau / 2 and take precision, recall and F-score at tau with the cumulative distance curves (``evaluate_scene``).  Everything per
point is defined exactly in ``mvster_amd/csrc/reg_math.h`` and runs in ``csrc/geo_reg.hip``; the nearest neighbours are
``fusion.nearest_distances``, the thinning ``fusion.thin_points``.  Neither the benchmark's Python toolbox nor Open3D was
available when this was written: the protocol is implemented from its description, and agreement with Open3D itself has not been
tested.  No CPU fallback.
"""
import collections
import json
import math
import os

import numpy as np
import torch

from . import _lib
from .dtu_eval import read_ply_points, smallest_cell
from .fusion import CloudGrid, _as_grid, _check_cloud, _check_length, _check_max_dist_cell, _check_tau, nearest_distances, thin_points

SCENE_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}
TANKS_TRAINING_SCENES = tuple(SCENE_TAU)
MIN_POLYGON, MAX_POLYGON = 3, 1024      # vertices of a crop volume's polygon (csrc/reg_math.h)
MAX_BINS = 4096                         # bins of distance_histogram (an LDS histogram per workgroup)
ROUND3_MAX_POINTS = 4000000             # the third ICP round takes every k-th point of a cropped cloud larger than this
ICP_ROUNDS = ((1.0, 80.0), (0.5, 20.0), (None, 2.0))   # (voxel / tau or None, ICP threshold / tau) of the three rounds
_AXES = {"X": 0, "Y": 1, "Z": 2}

CropVolume = collections.namedtuple("CropVolume", "orthogonal_axis axis_min axis_max polygon")


def _no_cpu(what, name):
    return RuntimeError("mvster_amd.tanks_eval.%s runs on MI355X only: %s must be a tensor on the GPU (there is no CPU fallback)"
                        % (what, name))


# ---- 1. the crop volume ---------------------------------------------------------------------------------------------------

def read_crop_volume(json_file):
    """The benchmark's ``<scene>.json`` (a selection polygon volume: ``orthogonal_axis``, ``axis_min``, ``axis_max``,
    ``bounding_polygon`` [P][3]) -> ``CropVolume(orthogonal_axis, axis_min, axis_max, polygon [P,3] float64)``."""
    with open(json_file) as f:
        d = json.load(f)
    for k in ("orthogonal_axis", "axis_min", "axis_max", "bounding_polygon"):
        if k not in d:
            raise RuntimeError("read_crop_volume: %s has no %r" % (json_file, k))
    vol = CropVolume(str(d["orthogonal_axis"]).upper(), float(d["axis_min"]), float(d["axis_max"]),
                     np.asarray(d["bounding_polygon"], np.float64))
    _check_volume("read_crop_volume", vol)
    return vol


def _check_volume(what, volume):
    """-> (axis 0 / 1 / 2, [2 + 2 P] float64: axis_min, axis_max, (u, v) of every vertex)."""
    if not isinstance(volume, CropVolume):
        raise RuntimeError("%s: volume must be a CropVolume, not %s" % (what, type(volume).__name__))
    if volume.orthogonal_axis not in _AXES:
        raise RuntimeError("%s: volume.orthogonal_axis must be 'X', 'Y' or 'Z', not %r" % (what, volume.orthogonal_axis))
    axis = _AXES[volume.orthogonal_axis]
    try:
        poly = np.asarray(volume.polygon, np.float64)
        lo, hi = float(volume.axis_min), float(volume.axis_max)
    except (TypeError, ValueError):
        raise RuntimeError("%s: volume.polygon, axis_min and axis_max must be numbers" % what) from None
    if poly.ndim != 2 or poly.shape[1] != 3:
        raise RuntimeError("%s: volume.polygon must be [P,3], not %s" % (what, poly.shape))
    if not MIN_POLYGON <= poly.shape[0] <= MAX_POLYGON:
        raise RuntimeError("%s: volume.polygon must have %d .. %d vertices, not %d" % (what, MIN_POLYGON, MAX_POLYGON, poly.shape[0]))
    if not (np.isfinite(poly).all() and np.isfinite(lo) and np.isfinite(hi)):
        raise RuntimeError("%s: volume.polygon, axis_min and axis_max must be finite" % what)
    u, v = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    return axis, np.concatenate([[lo, hi], poly[:, (u, v)].reshape(-1)]).astype(np.float64)


def _check_transform(what, name, T):
    """None, or a 4 x 4 matrix with finite entries and the last row 0 0 0 1 -> float64 [4,4] (NumPy)."""
    if T is None:
        return None
    try:
        M = np.array(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, np.float64)
    except (TypeError, ValueError):
        raise RuntimeError("%s: %s must be a 4 x 4 matrix of numbers" % (what, name)) from None
    if M.shape != (4, 4) or not np.isfinite(M).all() or not (M[3] == (0, 0, 0, 1)).all():
        raise RuntimeError("%s: %s must be a finite 4 x 4 matrix with the last row 0 0 0 1, not shape %s" % (what, name, M.shape))
    return M


def _rows(T):
    """The 12 doubles the entry points read on the host (kept alive by the caller for the call)."""
    return np.ascontiguousarray(T[:3].reshape(-1), np.float64)


def _check_points(what, name, points):
    if not isinstance(points, torch.Tensor):
        raise RuntimeError("%s: %s must be a torch tensor (on the GPU), not %s" % (what, name, type(points).__name__))
    _check_cloud(what, name, points)
    if not points.is_cuda:
        raise _no_cpu(what, name)


# ---- 2. transform and crop -------------------------------------------------------------------------------------------------

def transform_points(points, transform):
    """``float32(T p)`` for ``points`` [N,3] float32 on the GPU and ``transform`` a 4 x 4 matrix (last row 0 0 0 1), formed in
    fp64 in the order csrc/reg_math.h states -> [N,3] float32 on the GPU.  One launch, nothing read back.  No CPU fallback."""
    what = "transform_points"
    T = _check_transform(what, "transform", transform)
    if T is None:
        raise RuntimeError("%s: transform must be a 4 x 4 matrix, not None" % what)
    _check_points(what, "points", points)
    out = torch.empty_like(points, memory_format=torch.contiguous_format)
    N = points.shape[0]
    if N:
        rows, points = _rows(T), points.contiguous()
        with torch.cuda.device(points.device):
            rc = _lib.load().mvster_reg_transform(points.data_ptr(), N, rows.ctypes.data, out.data_ptr(),
                                                  torch.cuda.current_stream(points.device).cuda_stream)
            _lib.check(rc, "reg_transform")
    return out


def crop_points(points, volume, transform=None, colors=None, _max_grid=0):
    """The points of ``points`` [N,3] float32 (on the GPU) that lie inside the ``CropVolume``, after ``transform`` (a 4 x 4
    matrix or None) has moved them: q = T p in fp64, the inside test on the fp64 q (csrc/reg_math.h: every coordinate finite,
    axis_min <= q_w <= axis_max, the even-odd rule over the polygon's edges), the kept points as float32(q) in the input's
    order.  -> dict on the GPU: ``points`` [K,3] float32, ``index`` [K] int64 (ascending positions in the input), ``flags`` [N]
    uint8 (1 = inside), ``colors`` [K,3] uint8 where ``colors`` [N,3] uint8 was given; ``kept`` = K (int).  Three launches and
    one read-back (K); no atomics: two runs give the same bytes.  ``_max_grid`` (workgroups at most) is for the tests.  No CPU
    fallback."""
    what = "crop_points"
    axis, vol = _check_volume(what, volume)
    T = _check_transform(what, "transform", transform)
    _check_points(what, "points", points)
    N, dev = points.shape[0], points.device
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (N, 3) or colors.dtype != torch.uint8:
            raise RuntimeError("%s: colors must be a [N,3] uint8 tensor with the N of points (%d)" % (what, N))
        if colors.device != dev:
            raise _no_cpu(what, "colors")
    out = dict(points=torch.empty(0, 3, device=dev, dtype=torch.float32), index=torch.empty(0, device=dev, dtype=torch.int64),
               flags=torch.empty(N, device=dev, dtype=torch.uint8), kept=0)
    if colors is not None:
        out["colors"] = torch.empty(0, 3, device=dev, dtype=torch.uint8)
    if N == 0:
        return out
    lib = _lib.load()
    rows = None if T is None else _rows(T)
    tptr = None if rows is None else rows.ctypes.data
    points = points.contiguous()
    cptr = None if colors is None else colors.contiguous()
    with torch.cuda.device(dev):
        nblk = lib.mvster_reg_blocks(N)
        _lib.check(min(nblk, 0), "reg_blocks")
        volume_dev = torch.from_numpy(vol).to(dev)
        wg_counts = torch.empty(nblk, device=dev, dtype=torch.int32)
        wg_offsets = torch.empty(nblk + 1, device=dev, dtype=torch.int64)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.mvster_reg_crop_flags(points.data_ptr(), N, tptr, volume_dev.data_ptr(), (len(vol) - 2) // 2, axis, _max_grid,
                                       out["flags"].data_ptr(), wg_counts.data_ptr(), wg_offsets.data_ptr(), stream)
        _lib.check(rc, "reg_crop_flags")
        K = int(wg_offsets[nblk].item())                                     # the one read-back
        if K == 0:
            return out
        out.update(points=torch.empty(K, 3, device=dev, dtype=torch.float32), index=torch.empty(K, device=dev, dtype=torch.int64), kept=K)
        if colors is not None:
            out["colors"] = torch.empty(K, 3, device=dev, dtype=torch.uint8)
        rc = lib.mvster_reg_crop_emit(points.data_ptr(), None if cptr is None else cptr.data_ptr(), N, tptr, out["flags"].data_ptr(),
                                      wg_offsets.data_ptr(), K, _max_grid, out["points"].data_ptr(),
                                      out["colors"].data_ptr() if colors is not None else None, out["index"].data_ptr(), stream)
        _lib.check(rc, "reg_crop_emit")
    return out


# ---- 3. correspondence sums ---------------------------------------------------------------------------------------------------

def _search_lengths(what, target, max_dist, cell):
    """-> (max_dist, cell) as float32 values: the cell is ``cell``, else the target's where it is a CloudGrid, else the smallest
    the search takes for max_dist; it must be one the search takes (>= max_dist / 15)."""
    md = _check_length(what, "max_dist", max_dist)
    if cell is None:
        cell = target.cell if isinstance(target, CloudGrid) else smallest_cell(md)
    return _check_max_dist_cell(what, md, cell)


def _target_grid(what, target, cell):
    """A tensor is binned at ``cell``; a CloudGrid must have that cell."""
    if not isinstance(target, CloudGrid):
        _check_points(what, "target", target)
    return _as_grid(what, "target", target, cell)


def _sums_on_gpu(lib, source, grid, md, rows12):
    """The 18 sums of ``source`` moved by the 12 doubles ``rows12`` (None: as it is) against ``grid`` -> [18] float64 on the GPU;
    nothing is read back."""
    dev, Q = source.device, source.shape[0]
    out = torch.zeros(18, device=dev, dtype=torch.float64)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        moved = source
        if rows12 is not None:
            moved = torch.empty_like(source)
            _lib.check(lib.mvster_reg_transform(source.data_ptr(), Q, rows12.ctypes.data, moved.data_ptr(), stream), "reg_transform")
        near = nearest_distances(moved, grid, md)                             # the query's grid is built without a read-back
        nrows = lib.mvster_reg_sum_rows(Q)
        _lib.check(min(nrows, 0), "reg_sum_rows")
        partial = torch.empty(nrows, 18, device=dev, dtype=torch.float64)
        rc = lib.mvster_reg_sums(moved.data_ptr(), near["index"].data_ptr(), near["dist2"].data_ptr(), Q,
                                 grid.points.data_ptr() if grid.M else None, grid.M, partial.data_ptr(), out.data_ptr(), stream)
        _lib.check(rc, "reg_sums")
    return out


def registration_sums(source, target_grid, max_dist, transform=None, cell=None):
    """The sums an ICP iteration needs, over the points of ``source`` [Q,3] float32 (on the GPU) that have a point of the
    target within ``max_dist``: ``source`` is first moved by ``transform`` as in ``transform_points``, its nearest target comes
    from ``fusion.nearest_distances`` against ``target_grid`` (a ``CloudGrid``, or a tensor that is binned here).  -> float64
    [18] (NumPy): n, sum d2, sum s (3), sum t (3), sum s.s, sum t_a s_b (9, row a, column b) with s the moved source point as
    float32 widened to fp64, t its nearest target and d2 the search's ``dist2``.  One partial row per workgroup, added in row
    order: no floating-point atomics, two runs give the same bytes.  One read-back (the 18 doubles), besides the target's grid
    where it is built here.  No CPU fallback."""
    what = "registration_sums"
    T = _check_transform(what, "transform", transform)
    md, c = _search_lengths(what, target_grid, max_dist, cell)
    _check_points(what, "source", source)
    grid = _target_grid(what, target_grid, c)
    if grid.device != source.device:
        raise RuntimeError("%s: source and target must be on one GPU, not %s and %s" % (what, source.device, grid.device))
    out = _sums_on_gpu(_lib.load(), source.contiguous(), grid, md, None if T is None else _rows(T))
    return out.cpu().numpy()


# ---- 4. similarity from sums ---------------------------------------------------------------------------------------------------

def pair_sums(source, target):
    """The 18 sums of ``registration_sums`` for given pairs (NumPy [n,3] each, d2 = |t - s|^2): for ``umeyama`` on the host."""
    s, t = np.asarray(source, np.float64).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3)
    if s.shape != t.shape:
        raise RuntimeError("pair_sums: source and target must have one shape, not %s and %s" % (s.shape, t.shape))
    return np.concatenate([[len(s), ((t - s) ** 2).sum()], s.sum(0), t.sum(0), [(s * s).sum()], (t.T @ s).reshape(-1)])


def umeyama(sums, with_scaling=True):
    """The similarity (Umeyama 1991) that moves the source of ``sums`` (the 18 values of ``registration_sums``) onto its
    targets in the least-squares sense, on the host in fp64: mu_s = sum s / n, mu_t = sum t / n, Sigma = sum t s^T / n - mu_t
    mu_s^T = U D V^T, S = diag(1, 1, sign) with sign = -1 iff det(U) det(V) < 0, R = U S V^T, c = tr(D S) / (sum s.s / n -
    |mu_s|^2) (1 without scaling), t = mu_t - c R mu_s.  -> float64 [4,4], or None for n < 3, a variance that is not > 0 or
    sums that are not finite."""
    a = np.asarray(sums, np.float64).reshape(-1)
    if a.shape != (18,):
        raise RuntimeError("umeyama: sums must be the 18 values of registration_sums, not shape %s" % (a.shape,))
    n = a[0]
    if not np.isfinite(a).all() or n < 3:
        return None
    mu_s, mu_t = a[2:5] / n, a[5:8] / n
    var = a[8] / n - mu_s @ mu_s
    if not var > 0:
        return None
    sigma = a[9:18].reshape(3, 3) / n - np.outer(mu_t, mu_s)
    U, D, Vt = np.linalg.svd(sigma)
    S = np.array([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = (U * S) @ Vt
    c = float((D * S).sum() / var) if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mu_t - c * (R @ mu_s)
    return T if np.isfinite(T).all() else None


# ---- 5. ICP ---------------------------------------------------------------------------------------------------------------------

def _fit(sums, Q):
    n = sums[0]
    return (n / Q if Q else 0.0), (math.sqrt(sums[1] / n) if n > 0 else 0.0)


def register_clouds(source, target, max_dist, init=None, with_scaling=True, relative_fitness=1e-6, relative_rmse=1e-6,
                    max_iteration=20, cell=None):
    """Point-to-point ICP of ``source`` [Q,3] float32 (on the GPU) onto ``target`` (a tensor or a ``CloudGrid``, built once)
    with correspondences up to ``max_dist``, estimating a similarity (``with_scaling``) or a rigid motion.  T_0 = ``init`` or I.
    The source at iteration k is always float32(T_k source), formed from the original cloud: no drift.  Per iteration: the sums
    at T_k (``registration_sums``) give fitness = n / Q and rmse = sqrt(sum d2 / n) (0 for n = 0) and the update U
    (``umeyama``); T_{k+1} = U T_k; the sums at T_{k+1}; stop, ``converged``, when |fitness change| < ``relative_fitness`` and
    |rmse change| < ``relative_rmse``.  With no correspondence, or an update that ``umeyama`` cannot form, the current T comes
    back with ``converged=False``; nothing is raised.  One read-back of 18 doubles per evaluation (``iterations`` + 1 of them)
    and nothing else.

    -> dict: ``transformation`` float64 [4,4] (NumPy), ``fitness``, ``inlier_rmse``, ``correspondences`` (int) at that
    transformation, ``iterations`` (updates applied), ``converged``, ``history`` (fitness and inlier_rmse of every evaluation).

    The benchmark's toolbox is remembered to pass its iteration count positionally into the slot of Open3D's ``relative_rmse``;
    that could not be verified when this was written.  Whoever wants that behaviour passes ``relative_rmse=20,
    max_iteration=30``.  No CPU fallback."""
    what = "register_clouds"
    T = _check_transform(what, "init", init)
    T = np.eye(4) if T is None else T
    for name, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        if not (isinstance(v, (int, float)) and not isinstance(v, bool) and v >= 0 and np.isfinite(v)):
            raise RuntimeError("%s: %s must be a finite number >= 0, not %r" % (what, name, v))
    if not isinstance(max_iteration, int) or isinstance(max_iteration, bool) or max_iteration < 0:
        raise RuntimeError("%s: max_iteration must be an int >= 0, not %r" % (what, max_iteration))
    md, c = _search_lengths(what, target, max_dist, cell)
    _check_points(what, "source", source)
    grid = _target_grid(what, target, c)
    if grid.device != source.device:
        raise RuntimeError("%s: source and target must be on one GPU, not %s and %s" % (what, source.device, grid.device))
    lib, source, Q = _lib.load(), source.contiguous(), source.shape[0]

    def evaluate(M):
        sums = _sums_on_gpu(lib, source, grid, md, _rows(M)).cpu().numpy()    # the iteration's one read-back
        return sums, _fit(sums, Q)

    sums, (fitness, rmse) = evaluate(T)
    history = [dict(fitness=fitness, inlier_rmse=rmse)]
    iterations, converged = 0, False
    for _ in range(max_iteration):
        U = umeyama(sums, with_scaling) if sums[0] > 0 else None
        if U is None:
            break
        T = U @ T
        T[3] = (0, 0, 0, 1)
        iterations += 1
        sums, (f2, r2) = evaluate(T)
        history.append(dict(fitness=f2, inlier_rmse=r2))
        done = abs(f2 - fitness) < relative_fitness and abs(r2 - rmse) < relative_rmse
        fitness, rmse = f2, r2
        if done:
            converged = True
            break
    return dict(transformation=T, fitness=fitness, inlier_rmse=rmse, correspondences=int(sums[0]), iterations=iterations,
                converged=converged, history=history)


# ---- 6. distance histogram ------------------------------------------------------------------------------------------------------

def _check_edges(what, edges):
    try:
        e = np.ascontiguousarray(edges, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise RuntimeError("%s: edges must be numbers" % what) from None
    if not 2 <= len(e) <= MAX_BINS + 1:
        raise RuntimeError("%s: edges must hold 1 .. %d bins (2 .. %d values), not %d values" % (what, MAX_BINS, MAX_BINS + 1, len(e)))
    if not np.isfinite(e).all() or (e[:-1] > e[1:]).any():
        raise RuntimeError("%s: edges must be finite and increase monotonically" % what)
    return e


def _hist_on_gpu(lib, dist, edges_dev, bins, out):
    N = dist.shape[0]
    if N == 0:
        out.zero_()
        return
    rc = lib.mvster_reg_histogram(dist.data_ptr(), N, edges_dev.data_ptr(), bins, out.data_ptr(),
                                  torch.cuda.current_stream(dist.device).cuda_stream)
    _lib.check(rc, "reg_histogram")


def distance_histogram(dist, edges):
    """``np.histogram(dist, edges)[0]`` on the GPU for ``dist`` [N] float32 (on the GPU) and ``edges`` (B + 1 float64 values on
    the host, finite and non-decreasing, B <= 4096): edges[k] <= d < edges[k+1] in fp64, the last bin closed on the right; NaN
    and values outside the edges are not counted.  -> int64 [B] (NumPy).  Integer atomics on an LDS histogram per workgroup; one
    read-back.  It is for the benchmark's cumulative curves.  No CPU fallback."""
    what = "distance_histogram"
    e = _check_edges(what, edges)
    if not isinstance(dist, torch.Tensor) or dist.dim() != 1 or dist.dtype != torch.float32:
        raise RuntimeError("%s: dist must be a [N] float32 tensor" % what)
    if dist.shape[0] > 1 << 29:
        raise RuntimeError("%s: at most 2^29 distances, not %d" % (what, dist.shape[0]))
    if not dist.is_cuda:
        raise _no_cpu(what, "dist")
    dev, bins = dist.device, len(e) - 1
    out = torch.empty(bins, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _hist_on_gpu(_lib.load(), dist.contiguous(), torch.from_numpy(e).to(dev), bins, out)
    return out.cpu().numpy()


# ---- 7. the protocol ------------------------------------------------------------------------------------------------------------

def _thin(points, voxel):
    return thin_points(points, torch.zeros(points.shape[0], 3, device=points.device, dtype=torch.uint8), voxel, "mean")["points"]


def _round3_stride(points):
    n = points.shape[0]
    k = int(round(n / ROUND3_MAX_POINTS)) if n > ROUND3_MAX_POINTS else 1
    return points[::k].contiguous() if k > 1 else points


def _downsample(points, tau, voxel_over_tau):
    return _round3_stride(points) if voxel_over_tau is None else _thin(points, voxel_over_tau * tau)


def search_cell(tau, max_dist):
    """The edge of the search grid the protocol uses for a search up to ``max_dist``: the smallest the search takes
    (max_dist / 15), but not below tau / 2 -- no thinned cloud of the protocol has more than one point per voxel of tau / 2, and
    a smaller cell only adds empty cells to walk.  The results do not depend on it."""
    return max(smallest_cell(max_dist), float(np.float32(0.5 * tau)))


class TanksSceneTruth:
    """The ground truth of one Tanks and Temples scene on the GPU: ``gt_points`` [N,3] float32 (a tensor on the GPU), the
    scene's ``CropVolume``, its distance threshold ``tau`` (finite, > 0) and ``gt_trans``, the 4 x 4 matrix that moves a
    reconstruction made with the benchmark's cameras into the ground truth's frame (or None).  The cropped ground truth is made
    here (one read-back); its thinnings at tau and tau / 2, the third round's cloud and their search grids are made when first
    used and reused by every ``evaluate_scene``."""

    def __init__(self, gt_points, volume, tau, gt_trans=None):
        what = "TanksSceneTruth"
        self.tau = _check_length(what, "tau", tau)
        _check_volume(what, volume)
        self.volume = volume
        self.gt_trans = _check_transform(what, "gt_trans", gt_trans)
        _check_points(what, "gt_points", gt_points)
        self.device = gt_points.device
        self.cropped = crop_points(gt_points, volume)["points"]
        self._grids = {}

    @classmethod
    def from_files(cls, data_path, scene, device="cuda:0", tau=None):
        """``<scene>.ply`` (``dtu_eval.read_ply_points``), ``<scene>.json`` (``read_crop_volume``) and ``<scene>_trans.txt`` (a
        4 x 4 matrix as text) from ``data_path/<scene>/`` if that folder exists, else from ``data_path``; ``tau`` defaults to
        ``SCENE_TAU[scene]``."""
        folder = os.path.join(data_path, scene) if os.path.isdir(os.path.join(data_path, scene)) else data_path
        if tau is None:
            if scene not in SCENE_TAU:
                raise RuntimeError("TanksSceneTruth.from_files: no tau is known for scene %r (one of %s); pass tau=" %
                                   (scene, ", ".join(SCENE_TAU)))
            tau = SCENE_TAU[scene]
        files = [os.path.join(folder, scene + ext) for ext in (".ply", ".json", "_trans.txt")]
        for f in files:
            if not os.path.exists(f):
                raise RuntimeError("TanksSceneTruth.from_files: %s does not exist" % f)
        return cls(torch.from_numpy(read_ply_points(files[0])).to(device), read_crop_volume(files[1]), tau,
                   read_transform(files[2]))

    def level(self, voxel_over_tau, max_dist):
        """The cropped ground truth downsampled as an ICP round does (``voxel_over_tau`` None: every k-th point) as the
        CloudGrid a search up to ``max_dist`` uses; cached."""
        key = (voxel_over_tau, max_dist)
        if key not in self._grids:
            self._grids[key] = CloudGrid(_downsample(self.cropped, self.tau, voxel_over_tau), search_cell(self.tau, max_dist),
                                         _what="TanksSceneTruth", _name="gt_points")
        return self._grids[key]


def read_transform(filename):
    """A 4 x 4 matrix written as text (``<scene>_trans.txt``) -> float64 [4,4]."""
    try:
        M = np.loadtxt(filename, dtype=np.float64)
    except ValueError:
        raise RuntimeError("read_transform: %s does not hold numbers" % filename) from None
    if M.shape != (4, 4):
        raise RuntimeError("read_transform: %s must hold a 4 x 4 matrix, not shape %s" % (filename, M.shape))
    return M


def evaluate_scene(pred_points, truth, init_trans=None, refine=True, plot_stretch=5):
    """The benchmark's evaluation of a reconstructed cloud ``pred_points`` [M,3] float32 (on the GPU) against a
    ``TanksSceneTruth``.  T = ``init_trans``, or ``truth.gt_trans``, or I.  With ``refine`` three ICP rounds, each T <- U T with U
    from ``register_clouds(s, t, threshold, max_iteration=20)``, s the prediction moved by T, cropped and downsampled, t the
    ground truth cropped and downsampled: round 1 ``thin_points(mean)`` at tau with the threshold 80 tau, round 2 at tau / 2 with
    20 tau, round 3 no thinning (every k-th point, k = round(n / 4e6), of a cropped cloud of more than 4e6 points) with 2 tau; a
    round that is left without a source point ends the refinement.  Then both clouds, cropped and thinned at tau / 2:
    ``fusion.nearest_distances`` both ways up to ``plot_stretch`` tau, precision / recall / fscore and the raw counts exactly
    as ``fusion.score_clouds(tau=tau)`` forms them, and over edges = np.arange(0, tau plot_stretch, tau / 100) the cumulative
    histograms ``cum_source`` / ``cum_target`` divided by the number of points of each thinned cloud.

    -> dict: ``precision``, ``recall``, ``fscore``, ``pred_valid`` / ``pred_within`` / ``pred_below_tau`` / ``pred_sum`` and the
    same with ``gt_``, ``transformation`` float64 [4,4], ``rounds`` (one dict per ICP round: fitness, inlier_rmse, iterations,
    converged, source_points, target_points), ``edges``, ``cum_source``, ``cum_target`` (NumPy), ``points_in``,
    ``pred_cropped``, ``pred_thinned``, ``gt_cropped``, ``gt_thinned``.  Deviation: ``thin_points`` anchors its voxel grid at the
    origin where Open3D anchors it at the cloud's minimum corner minus half a voxel.  No CPU fallback."""
    what = "evaluate_scene"
    if not isinstance(truth, TanksSceneTruth):
        raise RuntimeError("%s: truth must be a TanksSceneTruth, not %s" % (what, type(truth).__name__))
    T = _check_transform(what, "init_trans", init_trans)
    T = T if T is not None else (truth.gt_trans if truth.gt_trans is not None else np.eye(4))
    stretch = _check_length(what, "plot_stretch", plot_stretch)
    _check_points(what, "pred_points", pred_points)
    if pred_points.device != truth.device:
        raise RuntimeError("%s: pred_points and truth must be on one GPU, not %s and %s" % (what, pred_points.device, truth.device))
    tau, dev = truth.tau, truth.device
    md = _check_length(what, "plot_stretch * tau", stretch * tau)
    t32 = _check_tau(what, tau, md)
    edges = np.arange(0, tau * stretch, tau / 100.0)
    edges = _check_edges(what, edges)
    rounds = []
    if refine:
        for voxel_over_tau, thr in ICP_ROUNDS:
            s = _downsample(crop_points(pred_points, truth.volume, transform=T)["points"], tau, voxel_over_tau)
            if s.shape[0] < 1:
                break
            grid = truth.level(voxel_over_tau, _check_length(what, "threshold", thr * tau))
            reg = register_clouds(s, grid, thr * tau, max_iteration=20)
            T = reg["transformation"] @ T
            T[3] = (0, 0, 0, 1)
            rounds.append(dict(fitness=reg["fitness"], inlier_rmse=reg["inlier_rmse"], iterations=reg["iterations"],
                               converged=reg["converged"], source_points=int(s.shape[0]), target_points=grid.M))
    cropped = crop_points(pred_points, truth.volume, transform=T)
    s = _thin(cropped["points"], 0.5 * tau)
    gt = truth.level(0.5, md)
    cell = gt.cell
    sg = CloudGrid(s, cell, _what=what, _name="pred_points")
    ways = (nearest_distances(sg, gt, md, cell), nearest_distances(gt, sg, md, cell))
    bins = len(edges) - 1
    stats = torch.zeros(2, 4, device=dev, dtype=torch.float64)
    hist = torch.zeros(2, bins, device=dev, dtype=torch.int64)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        edges_dev = torch.from_numpy(edges).to(dev)
        for w, way in enumerate(ways):
            Q = way["dist"].shape[0]
            if Q == 0:
                continue
            slots = lib.mvster_cloud_score_slots(Q)
            _lib.check(min(slots, 0), "cloud_score_slots")
            partial = torch.empty(slots, 4, device=dev, dtype=torch.float64)
            _lib.check(lib.mvster_cloud_score(way["dist"].data_ptr(), Q, md, t32, partial.data_ptr(), stats[w].data_ptr(), stream),
                       "cloud_score")
            _hist_on_gpu(lib, way["dist"], edges_dev, bins, hist[w])
    back = torch.cat([stats.view(torch.int64).reshape(-1), hist.reshape(-1)]).cpu().numpy()    # the one read-back
    rows, counts = back[:8].view(np.float64).reshape(2, 4), back[8:].reshape(2, bins)
    out = {}
    for name, (valid, within, below, total) in zip(("pred", "gt"), rows):
        out[name + "_valid"], out[name + "_within"], out[name + "_below_tau"], out[name + "_sum"] = int(valid), int(within), int(below), float(total)
    nan = float("nan")
    P = out["precision"] = out["pred_below_tau"] / out["pred_valid"] if out["pred_valid"] else nan
    R = out["recall"] = out["gt_below_tau"] / out["gt_valid"] if out["gt_valid"] else nan
    out["fscore"] = 0.0 if P + R == 0 else 2 * P * R / (P + R)
    with np.errstate(invalid="ignore", divide="ignore"):
        out.update(edges=edges, cum_source=np.cumsum(counts[0]).astype(np.float64) / np.float64(s.shape[0]),
                   cum_target=np.cumsum(counts[1]).astype(np.float64) / np.float64(gt.M))
    out.update(transformation=T, rounds=rounds, tau=tau, points_in=int(pred_points.shape[0]), pred_cropped=cropped["kept"],
               pred_thinned=int(s.shape[0]), gt_cropped=int(truth.cropped.shape[0]), gt_thinned=gt.M)
    return out


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, list):
        return [_jsonable(x) for x in v]
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    return v


def evaluate_tanks(ply_dir, data_path, scenes=TANKS_TRAINING_SCENES, out_dir=None, device="cuda:0", refine=True):
    """``evaluate_scene`` for every scene of ``scenes`` (default: the seven training scenes): the cloud ``{ply_dir}/{scene}.ply``
    against ``TanksSceneTruth.from_files(data_path, scene)`` -> dict ``rows`` (one ``evaluate_scene`` dict per scene, with
    ``scene``) and ``mean_fscore``.  With ``out_dir`` everything is written to ``{out_dir}/tanks_eval.json``."""
    rows = []
    for scene in scenes:
        ply = os.path.join(ply_dir, "%s.ply" % scene)
        if not os.path.exists(ply):
            raise RuntimeError("evaluate_tanks: %s does not exist" % ply)
        truth = TanksSceneTruth.from_files(data_path, scene, device=device)
        pred = torch.from_numpy(read_ply_points(ply)).to(device)
        rows.append(dict(evaluate_scene(pred, truth, refine=refine), scene=scene))
    out = dict(rows=rows, mean_fscore=float(np.mean([r["fscore"] for r in rows])) if rows else float("nan"))
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "tanks_eval.json"), "w") as f:
            json.dump(_jsonable(out), f, indent=1)
    return out


# ---- camera trajectories (host helpers) ------------------------------------------------------------------------------------------

def read_trajectory_log(filename):
    """A camera trajectory in the benchmark's ``.log`` format -- per camera one line of three integers, then the four rows of
    its 4 x 4 camera-to-world matrix -> (metadata int64 [n,3], poses float64 [n,4,4])."""
    with open(filename) as f:
        lines = [l.split() for l in f if l.strip()]
    if len(lines) % 5:
        raise RuntimeError("read_trajectory_log: %s must hold 5 lines per camera, not %d lines" % (filename, len(lines)))
    meta, poses = [], []
    try:
        for i in range(0, len(lines), 5):
            meta.append([int(v) for v in lines[i]])
            poses.append([[float(v) for v in l] for l in lines[i + 1:i + 5]])
        meta, poses = np.array(meta, np.int64).reshape(-1, 3), np.array(poses, np.float64).reshape(-1, 4, 4)
    except ValueError:
        raise RuntimeError("read_trajectory_log: %s is not a trajectory log (three integers, then four rows of four numbers)" % filename) from None
    return meta, poses


def trajectory_transform(est_log, colmap_log, gt_trans=None):
    """For a cloud that was not reconstructed with the benchmark's own cameras: the closed-form similarity (``umeyama``) that
    moves the camera centres of ``est_log`` onto those of ``colmap_log`` (files, or [n,4,4] pose arrays; camera i of one is
    camera i of the other), followed by ``gt_trans`` -> float64 [4,4], the ``init_trans`` of ``evaluate_scene``.  The toolbox's
    RANSAC over these correspondences is out of scope: every camera takes part."""
    est, col = (read_trajectory_log(x)[1] if isinstance(x, (str, os.PathLike)) else np.asarray(x, np.float64) for x in (est_log, colmap_log))
    if est.ndim != 3 or est.shape[1:] != (4, 4) or est.shape != col.shape:
        raise RuntimeError("trajectory_transform: the two trajectories must be [n,4,4] with one n, not %s and %s" % (est.shape, col.shape))
    U = umeyama(pair_sums(est[:, :3, 3], col[:, :3, 3]), True)
    if U is None:
        raise RuntimeError("trajectory_transform: %d camera centres do not determine a similarity" % len(est))
    G = _check_transform("trajectory_transform", "gt_trans", gt_trans)
    return U if G is None else G @ U
