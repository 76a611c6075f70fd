"""The DTU evaluation protocol on the GPU: what the MATLAB programs of the reference's
``evaluations/dtu/`` compute -- ``reducePts_haa.m`` (``reduce_points``), the observability mask, ground plane and block cover of
``PointCompareMain.m`` / ``MaxDistCP.m`` (``DTUScanTruth``), the statistics of ``ComputeStat_func.m`` (``distance_stats``) and
the loop over the 22 evaluation scans of ``BaseEvalMain_func.m`` (``evaluate_dtu``).  The nearest distances are
``fusion.nearest_distances``; everything per point is defined exactly in ``mvster_amd/csrc/eval_math.h`` and runs in
``csrc/geo_eval.hip``.  MATLAB's own random stream is not reproduced: ``priority=`` replays a ``RandOrd``.  No CPU fallback.
"""
import json
import os
import re

import numpy as np
import torch

from . import _lib
from .fusion import MIN_CELLS_PER_MAX_DIST, CloudGrid, _check_cloud, _check_length, _check_max_dist_cell, nearest_distances, thin_slots

DTU_EVAL_SCANS = (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)   # UsedSets
ROUNDS_PER_BATCH = 8                    # rounds of the reduction between two read-backs of the undecided count
MAX_BLOCK = 60.0                        # MaxDist of PointCompareMain.m: the edge of MaxDistCP's blocks
IN_MASK, ABOVE_PLANE, COVERED = 1, 2, 4  # the bits of a flag byte (mvster_eval_flags)


def _no_cpu(what, name):
    return RuntimeError("mvster_amd.dtu_eval.%s runs on MI355X only: %s must be a tensor on the GPU (there is no CPU fallback)"
                        % (what, name))


# ---- 1. reducePts_haa -------------------------------------------------------------------------------------------------

def reduce_points(points, dst=0.2, priority=None, seed=0, table_slots=None, _cell_factor=None):
    """``reducePts_haa.m`` on the GPU (defined exactly in mvster_amd/csrc/eval_math.h): the subset of
    ``points`` [M,3] float32 (on the GPU) in which no two kept points are within ``dst`` (its float32 value; finite, > 0) of
    each other, chosen greedily in priority order.  Point i has the priority (key_i, i): key_i = splitmix64(i, ``seed``)
    (``seed`` an int >= 0), or ``priority[i]`` of an int64 [M] tensor on the same GPU (ties allowed: the index decides) -- the
    way to replay a MATLAB run's ``RandOrd``.  A point is kept iff it is valid (finite, within 2^20 cells of edge ``dst`` of
    the origin) and no kept point of smaller priority has d2 <= dst^2 (fp64, inclusive).  That set is unique: it is what the
    serial loop of the .m file leaves set, and it depends neither on ``table_slots`` nor on the run.  (The search grid's cell
    is 2 * dst with 27 cells searched, or dst with 125 where 2 * dst overflows float32; ``_cell_factor`` is for the tests and
    the benchmark, which hold both grids to the same bytes.)

    -> dict: ``keep`` bool [M], ``index`` int64 [K] ascending (the order of ``pts(:,indexSet)``), ``points`` [K,3] on the GPU;
    ``dropped_invalid`` (int); ``rounds`` (int, reported only: it may differ between runs).  A round is one launch in which every
    undecided point decides from the states of its close neighbours of smaller priority; the host launches rounds in batches of
    ROUNDS_PER_BATCH and reads one vector of undecided counts per batch, stops at zero and raises if a batch decided nothing.
    With hashed priorities the depth is small (about 10 rounds); with ``priority = arange`` on a raster-ordered cloud every
    point can wait for the one before it and the depth can reach M rounds: allowed, and merely slow.  No CPU fallback."""
    what = "reduce_points"
    d = _check_length(what, "dst", dst)
    if not isinstance(seed, int) or isinstance(seed, bool) or seed < 0 or seed >= 1 << 63:
        raise RuntimeError("%s: seed must be an int in 0 .. 2^63 - 1, not %r" % (what, seed))
    if not isinstance(points, torch.Tensor):
        raise RuntimeError("%s: points must be a torch tensor (on the GPU), not %s" % (what, type(points).__name__))
    _check_cloud(what, "points", points)
    M = points.shape[0]
    if priority is not None:
        if not isinstance(priority, torch.Tensor) or priority.dtype != torch.int64:
            raise RuntimeError("%s: priority must be an int64 tensor, not %s" %
                               (what, priority.dtype if isinstance(priority, torch.Tensor) else type(priority).__name__))
        if tuple(priority.shape) != (M,):
            raise RuntimeError("%s: priority must have the length of points, [%d], not %s" % (what, M, tuple(priority.shape)))
        if priority.device != points.device:
            raise RuntimeError("%s: priority must be on the device of points (%s), not %s" % (what, points.device, priority.device))
    slots = thin_slots(M) if table_slots is None else table_slots
    if not isinstance(slots, int) or slots < thin_slots(M) or slots & (slots - 1) or slots > 1 << 30:
        raise RuntimeError("%s: table_slots must be a power of two, >= max(64, 2 * M) = %d and <= 2^30, not %r" %
                           (what, max(64, 2 * M), table_slots))
    with np.errstate(over="ignore"):
        twice = bool(np.isfinite(np.float32(2) * np.float32(d)))
    cell_factor = (2 if twice else 1) if _cell_factor is None else _cell_factor
    if not isinstance(cell_factor, int) or cell_factor not in (1, 2) or (cell_factor == 2 and not twice):
        raise RuntimeError("%s: _cell_factor must be 1 or 2 with _cell_factor * dst a finite float32, not %r" % (what, _cell_factor))
    if not points.is_cuda:
        raise _no_cpu(what, "points")
    dev = points.device
    if M == 0:
        return dict(keep=torch.zeros(0, device=dev, dtype=torch.bool), index=torch.zeros(0, device=dev, dtype=torch.int64),
                    points=points.new_zeros(0, 3), dropped_invalid=0, rounds=0)
    grid = CloudGrid(points, float(np.float32(cell_factor) * np.float32(d)), table_slots, _what=what)
    state = torch.empty(M, device=dev, dtype=torch.int32)
    counts = torch.empty(ROUNDS_PER_BATCH + 1, device=dev, dtype=torch.int64)   # behind the counts: the invalid points
    lib = _lib.load()
    rounds, dropped = 0, M                                                      # (no valid point at the grid's cell: none at dst)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.mvster_eval_reduce_init(grid.points.data_ptr(), M, d, state.data_ptr(), counts.data_ptr() + 8 * ROUNDS_PER_BATCH, stream)
        _lib.check(rc, "eval_reduce_init")
        left = grid.records.shape[0]                                         # the grid's points: undecided, but for those invalid at dst
        prio = None if priority is None else priority.contiguous()
        while left and grid.ncells:
            rc = lib.mvster_eval_reduce_rounds(grid.records.data_ptr(), grid.records.shape[0], grid.keys.data_ptr(),
                                               grid.cell_of_slot.data_ptr(), grid.slots, grid.starts.data_ptr(), grid.ncells, d, cell_factor,
                                               None if prio is None else prio.data_ptr(), seed, M, state.data_ptr(),
                                               counts.data_ptr(), ROUNDS_PER_BATCH, stream)
            _lib.check(rc, "eval_reduce_rounds")
            *after, dropped = counts.tolist()                                 # the batch's one read-back
            if 0 in after:
                rounds += after.index(0) + 1
                break
            if after[-1] >= left:
                raise RuntimeError("%s: %d rounds decided nothing (%d points undecided)" % (what, ROUNDS_PER_BATCH, left))
            left = after[-1]
            rounds += ROUNDS_PER_BATCH
    keep = state == 1
    index = torch.nonzero(keep).reshape(-1)
    return dict(keep=keep, index=index, points=grid.points[index], dropped_invalid=dropped, rounds=rounds)


# ---- 3. ComputeStat_func ----------------------------------------------------------------------------------------------------

def _launch_stats(lib, dist2, flags, need, md, out_row, stream):
    """The statistics of one direction into out_row [4] float64 (n, mean, var, median); nothing is read back."""
    N = dist2.shape[0]
    if N == 0:
        return
    slots = lib.mvster_eval_stats_slots(N)
    _lib.check(min(slots, 0), "eval_stats_slots")
    dev = dist2.device
    partial = torch.empty(slots, 2, device=dev, dtype=torch.float64)
    hist = torch.empty(8 * 2 * 256, device=dev, dtype=torch.int32)
    work = torch.empty(6, device=dev, dtype=torch.int64)
    rc = lib.mvster_eval_stats(dist2.data_ptr(), flags.data_ptr(), N, need, md, partial.data_ptr(), hist.data_ptr(), work.data_ptr(),
                               out_row.data_ptr(), stream)
    _lib.check(rc, "eval_stats")


def _empty_stats(dev, rows):
    nan = float("nan")
    return torch.tensor([[0.0, nan, nan, nan]] * rows, device=dev, dtype=torch.float64)


def distance_stats(dist2, select, max_dist):
    """The statistics ``ComputeStat_func.m`` takes of one direction: ``dist2`` [N] float64 on the GPU (squared distances, as
    ``fusion.nearest_distances`` gives them), ``select`` [N] bool or uint8 (non-zero: the point counts).  With d = sqrt(dist2),
    over the selected points with a finite dist2 and d < ``max_dist`` (strict; its float32 value) -> dict ``n``, ``mean``,
    ``var`` (second pass, / (n - 1); 0 for n = 1), ``median`` (exact: a radix selection, no sort); NaN for n = 0.  One
    read-back; two runs give the same bytes.  No CPU fallback."""
    what = "distance_stats"
    md = _check_length(what, "max_dist", max_dist)
    if not isinstance(dist2, torch.Tensor) or dist2.dim() != 1 or dist2.dtype != torch.float64:
        raise RuntimeError("%s: dist2 must be a [N] float64 tensor" % what)
    if not isinstance(select, torch.Tensor) or tuple(select.shape) != tuple(dist2.shape) or select.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("%s: select must be a [N] bool or uint8 tensor with the N of dist2 (%d)" % (what, dist2.shape[0]))
    if not dist2.is_cuda or select.device != dist2.device:
        raise _no_cpu(what, "dist2 and select")
    dev = dist2.device
    out = _empty_stats(dev, 1)
    with torch.cuda.device(dev):
        _launch_stats(_lib.load(), dist2.contiguous(), (select != 0).to(torch.uint8), 1, md, out[0],
                      torch.cuda.current_stream(dev).cuda_stream)
    n, mean, var, med = out[0].tolist()
    return dict(n=int(n), mean=mean, var=var, median=med)


# ---- 2. the ground truth of a scan ---------------------------------------------------------------------------------------------

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
              "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
              "double": "<f8", "float64": "<f8"}


def read_ply_points(filename):
    """x, y, z of a binary little-endian PLY's ``vertex`` element as float32 [N,3] (NumPy).  The element may carry any scalar
    properties besides (normals, colours, doubles); it must be the file's first element.  Header lines may end in LF or CR LF.  ``fusion.read_ply`` reads only the
    layout ``fusion.write_ply`` writes."""
    with open(filename, "rb") as f:
        data = f.read()
    m = re.search(rb"(?:^|\n)end_header[ \t]*\r?\n", data)                     # header lines may end in LF or in CR LF
    if m is None:
        raise RuntimeError("read_ply_points: %s has no PLY header" % filename)
    end = m.end()
    head = [l.split() for l in data[:end].decode("ascii", "replace").splitlines() if l.strip()]
    if head[0] != ["ply"] or ["format", "binary_little_endian", "1.0"] not in head:
        raise RuntimeError("read_ply_points: %s is not a binary little-endian PLY" % filename)
    elements = [i for i, l in enumerate(head) if l[0] == "element"]
    if not elements or head[elements[0]][1] != "vertex":
        raise RuntimeError("read_ply_points: the first element of %s is not 'vertex'" % filename)
    n = int(head[elements[0]][2])
    fields = []
    for l in head[elements[0] + 1:elements[1] if len(elements) > 1 else len(head)]:
        if l[0] != "property":
            continue
        if l[1] == "list" or l[1] not in _PLY_TYPES:
            raise RuntimeError("read_ply_points: vertex property %r of %s is not a scalar" % (" ".join(l[1:]), filename))
        if len(l) != 3 or l[2] in [f[0] for f in fields]:
            raise RuntimeError("read_ply_points: vertex property %r of %s has no name of its own" % (" ".join(l[1:]), filename))
        fields.append((l[2], _PLY_TYPES[l[1]]))
    dt = np.dtype(fields)
    if not all(k in dt.names for k in "xyz"):
        raise RuntimeError("read_ply_points: the vertex element of %s has no x, y, z" % filename)
    if len(data) < end + n * dt.itemsize:
        raise RuntimeError("read_ply_points: %s ends before its %d vertices" % (filename, n))
    v = np.frombuffer(data, dtype=dt, count=n, offset=end)
    return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)


def _loadmat(filename, names):
    try:
        from scipy.io import loadmat
    except ImportError:
        raise RuntimeError("DTUScanTruth.from_files: reading %s needs scipy (scipy.io.loadmat), which is not installed" % filename) from None
    if not os.path.exists(filename):
        raise RuntimeError("DTUScanTruth.from_files: %s does not exist" % filename)
    try:
        mat = loadmat(filename)
    except NotImplementedError:
        raise RuntimeError("DTUScanTruth.from_files: %s is a MATLAB v7.3 (HDF5) container, which scipy.io.loadmat does not read; "
                           "save it again with -v7" % filename) from None
    for k in names:
        if k not in mat:
            raise RuntimeError("DTUScanTruth.from_files: %s has no variable %r" % (filename, k))
    return mat


def read_scan_truth(data_path, scan, margin=10):
    """The three files of one scan as ``PointCompareMain.m`` reads them -> dict of NumPy arrays: ``stl_points`` [N,3] float32
    (Points/stl/stl%03d_total.ply), ``obs_mask`` [S1,S2,S3] uint8, ``bb`` [2,3] and ``res`` (ObsMask/ObsMask%d_%d.mat: ObsMask,
    BB, Res), ``plane`` [4] (ObsMask/Plane%d.mat: P)."""
    ply = os.path.join(data_path, "Points", "stl", "stl%03d_total.ply" % scan)
    if not os.path.exists(ply):
        raise RuntimeError("DTUScanTruth.from_files: %s does not exist" % ply)
    mask = _loadmat(os.path.join(data_path, "ObsMask", "ObsMask%d_%d.mat" % (scan, margin)), ("ObsMask", "BB", "Res"))
    plane = _loadmat(os.path.join(data_path, "ObsMask", "Plane%d.mat" % scan), ("P",))
    return dict(stl_points=read_ply_points(ply), obs_mask=np.ascontiguousarray(mask["ObsMask"] != 0).astype(np.uint8),
                bb=np.asarray(mask["BB"], np.float64), res=float(np.asarray(mask["Res"], np.float64).reshape(-1)[0]),
                plane=np.asarray(plane["P"], np.float64).reshape(-1))


def smallest_cell(max_dist):
    """The smallest search cell ``fusion.nearest_distances`` takes for ``max_dist``: max_dist / 15, rounded up to a float32."""
    md = np.float64(np.float32(max_dist))
    c = np.float32(md / MIN_CELLS_PER_MAX_DIST)
    if np.float64(c) < md / MIN_CELLS_PER_MAX_DIST:
        c = np.nextafter(c, np.float32(np.inf))
    return float(c)


class DTUScanTruth:
    """The ground truth of one DTU scan on the GPU: ``stl_points`` [N,3] float32 (a tensor on the GPU), ``obs_mask`` [S1,S2,S3]
    (array or tensor, non-zero = observable), ``bb`` [2,3], ``res`` > 0 and ``plane`` [4] as the .mat files hold them (float64),
    ``max_dist`` the outlier threshold (20 mm).  The stl cloud's CloudGrid, its ``above_plane`` and ``covered`` flags and the
    uploaded mask are made once and reused by every ``evaluate_dtu_scan``.  ``cell``: the edge of the search grid, by default
    the smallest ``nearest_distances`` takes (``smallest_cell(max_dist)``, max_dist / 15): DTU clouds have a spacing of 0.2 mm
    against max_dist = 20 mm, a query scans 27 cells before it may stop, and a cell of max_dist / 4 would hold some 600 surface
    points where this one holds some 45; the result does not depend on it.  One read-back for the grid and one for
    ``stl_above_plane``."""

    def __init__(self, stl_points, obs_mask, bb, res, plane, max_dist=20.0, cell=None):
        what = "DTUScanTruth"
        self.max_dist = _check_length(what, "max_dist", max_dist)
        self.cell = smallest_cell(self.max_dist) if cell is None else _check_max_dist_cell(what, self.max_dist, cell)[1]
        mask = obs_mask.detach().cpu().numpy() if isinstance(obs_mask, torch.Tensor) else np.asarray(obs_mask)
        if mask.ndim != 3 or min(mask.shape) < 1:
            raise RuntimeError("%s: obs_mask must be 3-D [S1,S2,S3], not %s" % (what, tuple(mask.shape)))
        try:
            bb = np.asarray(bb.detach().cpu().numpy() if isinstance(bb, torch.Tensor) else bb, np.float64)
            plane = np.asarray(plane.detach().cpu().numpy() if isinstance(plane, torch.Tensor) else plane, np.float64).reshape(-1)
            res = float(res)
        except (TypeError, ValueError):
            raise RuntimeError("%s: bb, res and plane must be numbers" % what) from None
        if bb.shape != (2, 3) or not np.isfinite(bb).all():
            raise RuntimeError("%s: bb must be 2 x 3 and finite, not shape %s" % (what, bb.shape))
        if not (np.isfinite(res) and res > 0):
            raise RuntimeError("%s: res must be finite and > 0, not %r" % (what, res))
        if plane.shape != (4,) or not np.isfinite(plane).all():
            raise RuntimeError("%s: plane must have length 4 and be finite, not shape %s" % (what, plane.shape))
        if not isinstance(stl_points, torch.Tensor):
            raise RuntimeError("%s: stl_points must be a torch tensor (on the GPU), not %s" % (what, type(stl_points).__name__))
        _check_cloud(what, "stl_points", stl_points)
        if not stl_points.is_cuda:
            raise _no_cpu(what, "stl_points")
        dev = self.device = stl_points.device
        self.shape = tuple(int(s) for s in mask.shape)
        self.bb, self.res, self.plane = bb, res, plane
        self.mask = torch.from_numpy(np.ascontiguousarray(mask != 0).astype(np.uint8)).to(dev)
        self.params = torch.tensor(list(bb.reshape(-1)) + [res, MAX_BLOCK] + list(plane), dtype=torch.float64).to(dev)
        self.grid = CloudGrid(stl_points, self.cell, _what=what, _name="stl_points")
        self.flags, counts = self.point_flags(self.grid.points, ABOVE_PLANE | COVERED)
        self.stl_above_plane = int(counts[1])

    @classmethod
    def from_files(cls, data_path, scan, margin=10, max_dist=20.0, device="cuda:0", cell=None):
        """The scan's ground truth from ``Points/stl/stl%03d_total.ply``, ``ObsMask/ObsMask%d_%d.mat`` and ``ObsMask/Plane%d.mat``
        under ``data_path`` (``read_scan_truth``; scipy.io.loadmat)."""
        t = read_scan_truth(data_path, scan, margin)
        return cls(torch.from_numpy(t.pop("stl_points")).to(device), max_dist=max_dist, cell=cell, **t)

    def point_flags(self, points, which=IN_MASK | ABOVE_PLANE | COVERED):
        """One byte per point of ``points`` [N,3] float32 on the GPU: IN_MASK | ABOVE_PLANE | COVERED, each only where ``which``
        asks for it -> (flags [N] uint8, counts [3] int64 = the points with each bit), both on the GPU."""
        what = "DTUScanTruth.point_flags"
        _check_cloud(what, "points", points)
        if not points.is_cuda or points.device != self.device:
            raise _no_cpu(what, "points")
        N = points.shape[0]
        flags = torch.empty(N, device=self.device, dtype=torch.uint8)
        counts = torch.zeros(3, device=self.device, dtype=torch.int64)
        if N:
            points = points.contiguous()
            with torch.cuda.device(self.device):
                rc = _lib.load().mvster_eval_flags(points.data_ptr(), N, self.mask.data_ptr(), *self.shape, self.params.data_ptr(),
                                                   which, flags.data_ptr(), counts.data_ptr(),
                                                   torch.cuda.current_stream(self.device).cuda_stream)
                _lib.check(rc, "eval_flags")
        return flags, counts


# ---- 4. a scan, and the 22 of them ------------------------------------------------------------------------------------------

def evaluate_dtu_scan(pred_points, truth, dst=0.2, seed=0, priority=None, reduce=True, return_points=False):
    """``PointCompareMain.m`` and one column of ``ComputeStat_func.m`` for a predicted cloud ``pred_points`` [M,3] float32 on the
    GPU against a ``DTUScanTruth``: (1) ``reduce_points(pred_points, dst, priority, seed)`` unless ``reduce=False``; (2)
    ``fusion.nearest_distances`` both ways at ``truth.max_dist``, the reduced cloud's grid built once and used as query and as
    target; (3) a data point counts iff in_obs_mask and covered, an stl point iff above_plane and covered; (4) the statistics of
    the distances < max_dist, read back in one copy.

    -> dict: ``n_data``, ``mean_data`` (accuracy), ``var_data``, ``med_data``; ``n_stl``, ``mean_stl`` (completeness), ``var_stl``,
    ``med_stl``; ``overall`` = (mean_data + mean_stl) / 2; ``points_in``, ``points_reduced``, ``downsample_factor``,
    ``data_in_mask``, ``stl_above_plane``, ``rounds``, ``dropped_invalid`` (of the prediction), ``dropped_reduced`` (``reduce=False``
    only: invalid points at the search cell), ``dropped_stl``.  With ``return_points=True`` also the per-point GPU tensors
    BaseEval holds: ``Qdata_index`` int64 [K] into pred_points, ``Qdata`` [K,3], ``Ddata`` [K] and ``Dstl`` [N] float64 (+inf
    where MATLAB keeps a distance of 20 .. 60: the < 20 filter discards both; NaN for an invalid point), ``DataInMask`` [K] and
    ``StlAbovePlane`` [N] bool."""
    what = "evaluate_dtu_scan"
    if not isinstance(truth, DTUScanTruth):
        raise RuntimeError("%s: truth must be a DTUScanTruth, not %s" % (what, type(truth).__name__))
    if not isinstance(pred_points, torch.Tensor):
        raise RuntimeError("%s: pred_points must be a torch tensor (on the GPU), not %s" % (what, type(pred_points).__name__))
    _check_cloud(what, "pred_points", pred_points)
    if reduce:
        red = reduce_points(pred_points, dst, priority, seed)
        q, index, rounds, dropped = red["points"], red["index"], red["rounds"], red["dropped_invalid"]
    else:
        if not pred_points.is_cuda:
            raise _no_cpu(what, "pred_points")
        q, rounds, dropped = pred_points.contiguous(), 0, 0
        index = torch.arange(q.shape[0], device=q.device)
    if q.device != truth.device:
        raise RuntimeError("%s: pred_points and truth must be on one GPU, not %s and %s" % (what, q.device, truth.device))
    dev, md = truth.device, truth.max_dist
    qgrid = CloudGrid(q, truth.cell, _what=what, _name="pred_points")
    data = nearest_distances(qgrid, truth.grid, md)
    stl = nearest_distances(truth.grid, qgrid, md)
    dflags, dcounts = truth.point_flags(q, IN_MASK | COVERED)
    stats = _empty_stats(dev, 2)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        lib = _lib.load()
        _launch_stats(lib, data["dist2"], dflags, IN_MASK | COVERED, md, stats[0], stream)
        _launch_stats(lib, stl["dist2"], truth.flags, ABOVE_PLANE | COVERED, md, stats[1], stream)
    back = torch.cat([stats.view(torch.int64).reshape(-1), dcounts]).cpu().numpy()    # the one read-back
    rows = back[:8].view(np.float64).reshape(2, 4)
    out = {}
    for name, row in zip(("data", "stl"), rows):
        out["n_" + name], out["mean_" + name], out["var_" + name], out["med_" + name] = int(row[0]), float(row[1]), float(row[2]), float(row[3])
    out["overall"] = (out["mean_data"] + out["mean_stl"]) / 2
    M, K = pred_points.shape[0], q.shape[0]
    out.update(points_in=M, points_reduced=K, downsample_factor=M / K if K else float("nan"), data_in_mask=int(back[8]),
               stl_above_plane=truth.stl_above_plane, rounds=rounds, dropped_invalid=dropped, dropped_reduced=qgrid.dropped,
               dropped_stl=truth.grid.dropped)
    if return_points:
        out.update(Qdata_index=index, Qdata=q, Ddata=data["dist2"].sqrt(), DataInMask=(dflags & IN_MASK) != 0,
                   Dstl=stl["dist2"].sqrt(), StlAbovePlane=(truth.flags & ABOVE_PLANE) != 0)
    return out


_BASESTAT = (("nStl", "n_stl"), ("nData", "n_data"), ("MeanStl", "mean_stl"), ("MeanData", "mean_data"), ("VarStl", "var_stl"),
             ("VarData", "var_data"), ("MedStl", "med_stl"), ("MedData", "med_data"))


def evaluate_dtu(ply_dir, data_path, scans=DTU_EVAL_SCANS, method="mvsnet", light="l3", out_dir=None, dst=0.2, seed=0,
                 device="cuda:0"):
    """``BaseEvalMain_func.m`` + ``ComputeStat_func.m``: for every scan of ``scans`` (default: the 22 evaluation sets) the cloud
    ``{ply_dir}/{method}{scan:03d}_{light}.ply`` against ``DTUScanTruth.from_files(data_path, scan)`` -> dict: ``rows`` (one
    ``evaluate_dtu_scan`` dict per scan, with ``scan``), ``BaseStat`` (nStl, nData, MeanStl, MeanData, VarStl, VarData, MedStl,
    MedData: lists in scan order), ``mean_acc`` = mean(MeanData), ``mean_comp`` = mean(MeanStl), ``mean_overall`` = their mean.
    With ``out_dir`` the two lines ``"%f\\n" % mean_acc`` and ``"%f\\n" % mean_comp`` are appended to
    ``TotalStat_{method}_Eval_.txt`` as the .m file does, and everything is written to ``TotalStat_{method}_Eval_.json``; no
    .mat output."""
    rows = []
    for scan in scans:
        ply = os.path.join(ply_dir, "%s%03d_%s.ply" % (method.lower(), scan, light))
        if not os.path.exists(ply):
            raise RuntimeError("evaluate_dtu: %s does not exist" % ply)
        truth = DTUScanTruth.from_files(data_path, scan, device=device)
        pred = torch.from_numpy(read_ply_points(ply)).to(device)
        rows.append(dict(evaluate_dtu_scan(pred, truth, dst=dst, seed=seed), scan=int(scan)))
    stat = {m: [r[k] for r in rows] for m, k in _BASESTAT}
    nan = float("nan")
    acc = float(np.mean(stat["MeanData"])) if rows else nan
    comp = float(np.mean(stat["MeanStl"])) if rows else nan
    out = dict(rows=rows, BaseStat=stat, mean_acc=acc, mean_comp=comp, mean_overall=(acc + comp) / 2.0)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        base = os.path.join(out_dir, "TotalStat_%s_Eval_" % method)
        with open(base + ".txt", "a") as f:
            f.write("%f\n" % acc)
            f.write("%f\n" % comp)
        with open(base + ".json", "w") as f:
            json.dump(dict(out, method=method, light=light, max_dist=20.0, dst=dst, seed=seed), f, indent=1)
    return out
