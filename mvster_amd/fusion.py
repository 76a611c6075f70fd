"""Depth-map filtering for fusion: the step after the forward pass.

Mirrors the reference's ``test_mvs4.py`` functions -- ``check_geometric_consistency`` (:313-328, built on
``reproject_with_depth`` :273-310) and the per-reference-view part of ``filter_depth`` (:352-407) -- on one fused
gfx950 kernel (``mvster_geo_filter``) instead of NumPy + ``cv2.remap`` per view pair.  Inputs may be NumPy arrays
(as in the reference) or torch tensors; NumPy in gives NumPy out.  The small camera-matrix algebra stays on the host
in NumPy float32, exactly as the reference computes it; everything per pixel runs on the GPU.

A whole scan -- the reference's unit of work (``filter_depth``, test_mvs4.py:331-421) -- goes through ``fuse_scene`` /
``filter_depth``: every map is uploaded once and three launches (``mvster_geo_scene_filter`` = filter pass + scan of the
workgroup counts, ``mvster_geo_scene_emit``) produce the masks and the point cloud in the reference's order.  With
``method="dynamic"`` the filter pass is ``mvster_geo_scene_filter_dynamic``: dynamic consistency checking, the rule Tanks
and Temples and ETH3D scans are fused with (not in the reference).
"""
import collections
import os

import numpy as np
import torch

from . import _lib, formats
from . import mesh as mesh_mod
from .mesh import MeshClean, TSDFMesh  # noqa: F401  (the ``mesh=`` / ``mesh_clean=`` specs of the scan-level entry points)


def _np32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32)


def view_matrices(ref_K, ref_E, src_Ks, src_Es):
    """-> (ref_mats [18], view_mats [NS,42]) float64 holding the reference's float32 products/inverses."""
    ref_K, ref_E = _np32(ref_K), _np32(ref_E)
    ref_mats = np.concatenate([np.linalg.inv(ref_K).reshape(-1), ref_K.reshape(-1)]).astype(np.float64)
    rows = []
    for K, E in zip(src_Ks, src_Es):
        K, E = _np32(K), _np32(E)
        a = np.matmul(E, np.linalg.inv(ref_E))[:3]          # reference -> source camera
        b = np.matmul(ref_E, np.linalg.inv(E))[:3]          # source -> reference camera
        rows.append(np.concatenate([a.reshape(-1), K.reshape(-1), np.linalg.inv(K).reshape(-1), b.reshape(-1)]))
    return ref_mats, np.stack(rows).astype(np.float64)


def _dev_depth(d, dev):
    if isinstance(d, torch.Tensor):
        return d.to(dev, torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(dev)


def geometric_filter(ref_depth, ref_K, ref_E, src_depths, src_Ks, src_Es, per_view=False, pix_thres=1.0, rel_thres=0.01,
                     device="cuda:0"):
    """One launch for a reference view against all its source views.  -> dict of CUDA tensors:
    ``mask_sum`` [H,W] int32 (consistent views per pixel), ``depth_sum`` [H,W] (sum of their reprojected depths) and,
    with ``per_view``, ``view_mask`` [NS,H,W] bool, ``view_depth``, ``x_src``, ``y_src`` [NS,H,W]."""
    dev = torch.device(device)
    dref = _dev_depth(ref_depth, dev)
    if isinstance(src_depths, torch.Tensor):
        dsrc = src_depths.to(dev, torch.float32).contiguous()
    else:
        dsrc = torch.stack([_dev_depth(d, dev) for d in src_depths]).contiguous()
    H, W = dref.shape
    NS = dsrc.shape[0]
    if tuple(dsrc.shape) != (NS, H, W) or len(src_Ks) != NS or len(src_Es) != NS:
        raise RuntimeError("geometric_filter: inconsistent shapes")
    ref_mats, view_mats = view_matrices(ref_K, ref_E, src_Ks, src_Es)
    ref_mats = torch.from_numpy(ref_mats).to(dev)
    view_mats = torch.from_numpy(view_mats).to(dev)
    mask_sum = torch.empty(H, W, device=dev, dtype=torch.int32)
    depth_sum = torch.empty(H, W, device=dev, dtype=torch.float32)
    vm = torch.empty(NS, H, W, device=dev, dtype=torch.uint8) if per_view else None
    vd, xs, ys = (torch.empty(NS, H, W, device=dev, dtype=torch.float32) for _ in range(3)) if per_view else (None,) * 3

    def ptr(t):
        return None if t is None else t.data_ptr()
    rc = _lib.load().mvster_geo_filter(ptr(dref), ptr(dsrc), ptr(ref_mats), ptr(view_mats), ptr(mask_sum), ptr(depth_sum),
                                       ptr(vm), ptr(vd), ptr(xs), ptr(ys), NS, H, W, float(pix_thres), float(rel_thres),
                                       torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "geo_filter")
    out = {"mask_sum": mask_sum, "depth_sum": depth_sum, "depth_ref": dref}
    if per_view:
        out.update(view_mask=vm.bool(), view_depth=vd, x_src=xs, y_src=ys)
    return out


def check_geometric_consistency(depth_ref, intrinsics_ref, extrinsics_ref, depth_src, intrinsics_src, extrinsics_src):
    """Reference signature (test_mvs4.py:313): -> (mask, depth_reprojected, x2d_src, y2d_src), NumPy in / NumPy out."""
    r = geometric_filter(depth_ref, intrinsics_ref, extrinsics_ref, [depth_src], [intrinsics_src], [extrinsics_src],
                         per_view=True)
    res = (r["view_mask"][0], r["view_depth"][0], r["x_src"][0], r["y_src"][0])
    if isinstance(depth_ref, torch.Tensor):
        return res
    return tuple(t.cpu().numpy() for t in res)


def filter_reference_view(ref_depth, ref_K, ref_E, confidence, src_depths, src_Ks, src_Es, conf_thres, thres_view,
                          ref_img=None):
    """The per-reference-view part of the reference's ``filter_depth`` (test_mvs4.py:352-407): photometric, geometric
    and final masks, the averaged depth (float64, like NumPy's float32 / int32 division) and the fused world points
    [M,3] of the pixels that pass; with ``ref_img`` [H,W,3] (float, 0..1, as ``read_img`` returns it) also their
    colours [M,3] uint8 (:395-396, :407).  Tensors stay on the GPU."""
    r = geometric_filter(ref_depth, ref_K, ref_E, src_depths, src_Ks, src_Es)
    dev = r["mask_sum"].device
    conf = _dev_depth(confidence, dev)
    photo_mask = conf > conf_thres
    geo_mask = r["mask_sum"] >= thres_view
    final_mask = photo_mask & geo_mask
    avg = (r["depth_sum"] + r["depth_ref"]).double() / (r["mask_sum"] + 1).double()
    H, W = avg.shape
    ys, xs = torch.nonzero(final_mask, as_tuple=True)                      # row-major order = NumPy's x[mask]
    depth = avg[ys, xs]
    kinv = torch.from_numpy(np.linalg.inv(_np32(ref_K)).astype(np.float64)).to(dev)
    einv = torch.from_numpy(np.linalg.inv(_np32(ref_E)).astype(np.float64)).to(dev)
    pix = torch.stack([xs.double() * depth, ys.double() * depth, depth])   # (x, y, 1) * depth
    cam = kinv @ pix
    world = (einv @ torch.cat([cam, torch.ones_like(depth)[None]], 0))[:3]
    out = dict(photo_mask=photo_mask, geo_mask=geo_mask, final_mask=final_mask, geo_mask_sum=r["mask_sum"],
               depth_est_averaged=avg, points=world.t().contiguous())
    if ref_img is not None:
        img = ref_img if isinstance(ref_img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref_img))
        img = img.to(dev)
        if tuple(img.shape[:2]) != (H, W) or img.shape[-1] != 3:
            raise RuntimeError("filter_reference_view: ref_img must be [H,W,3] at the depth map's resolution")
        out["colors"] = (img[ys, xs] * 255).to(torch.uint8)              # (color * 255).astype(np.uint8): truncation
    return out


PLY_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def fuse_views(per_view_results):
    """Concatenate the ``points`` / ``colors`` of consecutive ``filter_reference_view`` results in reference-view order
    into the structured vertex array the reference hands to plyfile (test_mvs4.py:409-418): x, y, z float32 (the float64
    world points rounded once) and red, green, blue uint8."""
    pts = torch.cat([r["points"] for r in per_view_results], 0).to(torch.float32).cpu().numpy()
    cols = torch.cat([r["colors"] for r in per_view_results], 0).cpu().numpy()
    v = np.empty(len(pts), dtype=PLY_VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    v["red"], v["green"], v["blue"] = cols[:, 0], cols[:, 1], cols[:, 2]
    return v


PLY_NORMAL_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                    ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(filename, vertices, normals=None):
    """Binary little-endian PLY with one ``vertex`` element, the file ``PlyData([PlyElement.describe(v, 'vertex')])
    .write(f)`` produces for the array above (test_mvs4.py:420-421).  ``normals`` [M,3] (array or tensor; default None: the
    same bytes as ever): the vertex element is x y z nx ny nz red green blue, the order Open3D writes."""
    v = np.ascontiguousarray(vertices, dtype=PLY_VERTEX_DTYPE)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        n = _np32(normals)
        if n.shape != (len(v), 3):
            raise RuntimeError("write_ply: normals must be [M,3] with the M of vertices (%d), not %s" % (len(v), n.shape))
        w = np.empty(len(v), dtype=PLY_NORMAL_VERTEX_DTYPE)
        for name in PLY_VERTEX_DTYPE.names:
            w[name] = v[name]
        w["nx"], w["ny"], w["nz"] = n[:, 0], n[:, 1], n[:, 2]
        v = w
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + props +
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())


def read_ply(filename):
    """Inverse of ``write_ply`` (round-trip tests and downstream checks)."""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    n = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    if "format binary_little_endian 1.0" not in head:
        raise RuntimeError("read_ply: only the binary little-endian layout of write_ply is read")
    return np.frombuffer(data[end:end + n * PLY_VERTEX_DTYPE.itemsize], dtype=PLY_VERTEX_DTYPE).copy()


# ---- a whole scan at once ------------------------------------------------------------------------------------------

SceneTables = collections.namedtuple("SceneTables", "pair_table ref_view ref_mats view_mats")
SCRATCH_BUDGET = 64 << 20      # bytes of per-call scratch (tables, workgroup counts and offsets) before fuse_scene chunks


def scene_tables(pairs, Ks, Es):
    """pairs [(ref_view, [src_view, ...]), ...] (``formats.read_pair_file``), Ks [V,3,3], Es [V,4,4] -> SceneTables:
    ``pair_table`` [R,Smax] int32 padded with -1, ``ref_view`` [R] int32, ``ref_mats`` [R,30] float64 = inv(K_ref),
    K_ref, inv(E_ref)[:3], ``view_mats`` [R,Smax,42] float64 (zeros behind the padding).  Pure NumPy; row r holds the
    very bits ``view_matrices`` gives for reference view r (float32 products and inverses, widened)."""
    pairs = [(int(r), [int(v) for v in srcs]) for r, srcs in pairs]
    V = len(Ks)
    if len(Es) != V or not pairs:
        raise RuntimeError("scene_tables: need one K and one E per view and at least one reference view")
    for r, srcs in pairs:
        if not srcs:
            raise RuntimeError("scene_tables: reference view %d has an empty source list" % r)
        for v in [r] + srcs:
            if not 0 <= v < V:
                raise RuntimeError("scene_tables: view index %d lies outside the stack of %d views" % (v, V))
    R, smax = len(pairs), max(len(srcs) for _, srcs in pairs)
    pair_table = np.full((R, smax), -1, dtype=np.int32)
    ref_mats = np.zeros((R, 30), dtype=np.float64)
    view_mats = np.zeros((R, smax, 42), dtype=np.float64)
    for i, (r, srcs) in enumerate(pairs):
        pair_table[i, :len(srcs)] = srcs
        rm, vm = view_matrices(Ks[r], Es[r], [Ks[v] for v in srcs], [Es[v] for v in srcs])
        ref_mats[i, :18] = rm
        ref_mats[i, 18:] = np.linalg.inv(_np32(Es[r]))[:3].reshape(-1)
        view_mats[i, :len(srcs)] = vm
    return SceneTables(pair_table, np.array([r for r, _ in pairs], dtype=np.int32), ref_mats, view_mats)


class SceneResult(dict):
    """What ``fuse_scene`` returns: a dict of tensors on the GPU (``points``, ``colors``, ``counts``, ``photo_mask``,
    ``geo_mask``, ``final_mask``, ``geo_mask_sum``, ``depth_est_averaged``; with ``method="dynamic"`` also ``geo_level``)
    plus ``vertices()``."""

    def vertices(self, thinned=False, final=False):
        """The structured vertex array of filter_depth (test_mvs4.py:409-418) on the host, ready for ``write_ply``;
        ``thinned``: of the voxel-thinned cloud (``fuse_scene(voxel_size=...)``), an error if there is none; ``final``: of the
        cleaned cloud (``fuse_scene(outliers=..., normals=...)``), an error if there is none."""
        if thinned and "thin_points" not in self:
            raise RuntimeError("SceneResult.vertices(thinned=True): this result holds no thinned cloud (fuse_scene was "
                               "called without voxel_size)")
        if final and "final_points" not in self:
            raise RuntimeError("SceneResult.vertices(final=True): this result holds no cleaned cloud (fuse_scene was called "
                               "without outliers and normals)")
        pts, cols = (self[("final_" if final else "thin_" if thinned else "") + k].cpu().numpy() for k in ("points", "colors"))
        v = np.empty(len(pts), dtype=PLY_VERTEX_DTYPE)
        v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
        v["red"], v["green"], v["blue"] = cols[:, 0], cols[:, 1], cols[:, 2]
        return v


def _scene_stack(x, dev, dtype, what):
    """Maps of a scan (array, tensor, or a sequence of either) -> one contiguous tensor [V, ...] on ``dev``."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        x = list(x)
        if len({tuple(m.shape) for m in x}) > 1:
            raise RuntimeError("fuse_scene: %s maps of different sizes inside one scan" % what)
        if all(isinstance(m, torch.Tensor) for m in x):
            x = torch.stack([m.to(dev) for m in x])
        else:
            x = np.stack([m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in x])
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=dtype))
    return x.to(dev, getattr(torch, np.dtype(dtype).name)).contiguous()


FUSION_METHODS = ("normal", "dynamic")
PIX_THRES, REL_THRES = 1.0, 0.01        # the reference's fixed thresholds (test_mvs4.py:319, :323): method "normal"
PIX_BASE, REL_BASE = 0.25, 1 / 1300     # the base errors of the public dynamic-fusion scripts: method "dynamic"
MAX_DYNAMIC_SOURCES = 32                # sources per reference view the dynamic filter's per-pixel level counts hold


def _check_method(what, method, pix_thres=None, rel_thres=None):
    if method not in FUSION_METHODS:
        raise RuntimeError("%s: unknown fusion method %r (one of %s)" % (what, method, ", ".join(FUSION_METHODS)))
    if method == "dynamic" and (pix_thres is not None or rel_thres is not None):
        raise RuntimeError("%s: pix_thres / rel_thres are the fixed thresholds of method 'normal'; method 'dynamic' takes "
                           "pix_base / rel_base" % what)


VOXEL_REDUCE = ("mean", "first")
MAX_THIN_POINTS = 1 << 29               # a slot index and its leader mark share 32 bits (mvster_voxel_thin_blocks)


def _check_voxel(what, voxel_size, voxel_reduce):
    """voxel_size None (no thinning) or a number whose float32 value is finite and > 0; voxel_reduce one of VOXEL_REDUCE."""
    if voxel_reduce not in VOXEL_REDUCE:
        raise RuntimeError("%s: unknown voxel reduction %r (one of %s)" % (what, voxel_reduce, ", ".join(VOXEL_REDUCE)))
    if voxel_size is None:
        return None
    try:
        with np.errstate(over="ignore"):
            v = float(np.float32(voxel_size))
    except (TypeError, ValueError):
        raise RuntimeError("%s: voxel_size must be a number, not %r" % (what, voxel_size)) from None
    if not (np.isfinite(v) and v > 0):
        raise RuntimeError("%s: voxel_size must be finite and > 0 as a float32, not %r" % (what, voxel_size))
    return v


def thin_slots(M):
    """The table size ``thin_points`` uses for M points: the smallest power of two >= 2 * M, at least 64."""
    return max(64, 1 << max(0, 2 * int(M) - 1).bit_length())


def thin_points(points, colors, voxel_size, reduce="mean", table_slots=None):
    """Voxel-grid thinning of a cloud on the GPU (what Open3D and PCL call voxel_down_sample, defined
    exactly in mvster_amd/csrc/voxel_math.h): ``points`` [M,3] float32 and ``colors`` [M,3] uint8 tensors on the GPU, one
    output point per occupied voxel of edge ``voxel_size`` (its float32 value; finite, > 0).  ``reduce="first"`` keeps each
    voxel's first input point and colour as they are, ``"mean"`` gives the mean of the voxel's points (16-bit fixed-point
    offsets inside the voxel, integer sums) and the mean colour rounded half up.  Voxels come in the order of their first
    point, so the thinned cloud keeps the input's order.  Points with a NaN or infinite coordinate, or beyond 2^20 voxels from
    the origin on an axis, take no part.  -> dict: ``points`` [U,3] float32, ``colors`` [U,3] uint8, ``counts`` [U] int32
    (points per voxel), ``first`` [U] int64 (index of each voxel's first point: gathers any other per-point attribute) on the
    GPU, ``dropped`` (int) = the points that took no part.  Integer atomics only: two runs give the same bytes.  One host
    synchronisation (U and ``dropped`` in one copy).  ``table_slots``: size of the hash table, a power of two >= max(64,
    2 * M) (default: the smallest); the result does not depend on it.  No CPU fallback."""
    v = _check_voxel("thin_points", voxel_size, reduce)
    if v is None:
        raise RuntimeError("thin_points: voxel_size must be finite and > 0 as a float32, not None")
    if not isinstance(points, torch.Tensor) or not isinstance(colors, torch.Tensor):
        raise RuntimeError("thin_points: points and colors must be torch tensors (on the GPU)")
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise RuntimeError("thin_points: points must be [M,3] float32, not %s %s" % (tuple(points.shape), points.dtype))
    if tuple(colors.shape) != tuple(points.shape) or colors.dtype != torch.uint8:
        raise RuntimeError("thin_points: colors must be [M,3] uint8 with the M of points (%d), not %s %s" %
                           (points.shape[0], tuple(colors.shape), colors.dtype))
    M = points.shape[0]
    if M > MAX_THIN_POINTS:
        raise RuntimeError("thin_points: at most 2^29 points, not %d" % M)
    slots = thin_slots(M) if table_slots is None else table_slots
    if not isinstance(slots, int) or slots < thin_slots(M) or slots & (slots - 1) or slots > 1 << 30:
        raise RuntimeError("thin_points: table_slots must be a power of two, >= max(64, 2 * M) = %d and <= 2^30, not %r" %
                           (max(64, 2 * M), table_slots))
    if not points.is_cuda or colors.device != points.device:
        raise RuntimeError("mvster_amd.fusion.thin_points runs on MI355X only: points and colors must be tensors on one GPU "
                           "(there is no CPU fallback)")
    dev = points.device
    empty = dict(points=torch.empty(0, 3, device=dev, dtype=torch.float32), colors=torch.empty(0, 3, device=dev, dtype=torch.uint8),
                 counts=torch.empty(0, device=dev, dtype=torch.int32), first=torch.empty(0, device=dev, dtype=torch.int64))
    if M == 0:
        return dict(empty, dropped=0)
    points, colors = points.contiguous(), colors.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        nblk = lib.mvster_voxel_thin_blocks(M)
        _lib.check(min(nblk, 0), "voxel_thin_blocks")
        keys = torch.empty(slots, device=dev, dtype=torch.int64)
        first = torch.empty(slots, device=dev, dtype=torch.int32)
        slot = torch.empty(M, device=dev, dtype=torch.int32)
        wg_counts = torch.empty(nblk, device=dev, dtype=torch.int32)
        wg_offsets = torch.empty(nblk + 3, device=dev, dtype=torch.int64)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.mvster_voxel_thin_insert(points.data_ptr(), M, v, keys.data_ptr(), first.data_ptr(), slots, slot.data_ptr(),
                                          wg_counts.data_ptr(), wg_offsets.data_ptr(), stream)
        _lib.check(rc, "voxel_thin_insert")
        U, dropped, status = wg_offsets[nblk:].tolist()                      # the one host sync
        if status:
            raise RuntimeError("thin_points: a point found no slot in a table of %d slots for %d points" % (slots, M))
        if U == 0:
            return dict(empty, dropped=dropped)
        del keys
        mean = reduce == "mean"
        out = dict(points=torch.empty(U, 3, device=dev, dtype=torch.float32), colors=torch.empty(U, 3, device=dev, dtype=torch.uint8),
                   counts=torch.empty(U, device=dev, dtype=torch.int32), first=torch.empty(U, device=dev, dtype=torch.int64))
        sums = torch.empty(U, 6, device=dev, dtype=torch.int64) if mean else None
        rc = lib.mvster_voxel_thin_emit(points.data_ptr(), colors.data_ptr(), M, v, 0 if mean else 1, first.data_ptr(),
                                        slot.data_ptr(), wg_offsets.data_ptr(), sums.data_ptr() if mean else None,
                                        out["points"].data_ptr(), out["colors"].data_ptr(), out["counts"].data_ptr(),
                                        out["first"].data_ptr(), U, stream)
        _lib.check(rc, "voxel_thin_emit")
    return dict(out, dropped=dropped)


MAX_CLOUD_POINTS = 1 << 29              # as in thin_points: the grid of a cloud is built on the thinning's table
MIN_CELLS_PER_MAX_DIST = 15             # cell >= max_dist / 15: at most 17 shells per query (csrc/nn_math.h)


def _check_length(what, name, value):
    """A length whose float32 value is finite and > 0 -> that value as a Python float."""
    try:
        with np.errstate(over="ignore"):
            v = float(np.float32(value))
    except (TypeError, ValueError):
        raise RuntimeError("%s: %s must be a number, not %r" % (what, name, value)) from None
    if not (np.isfinite(v) and v > 0):
        raise RuntimeError("%s: %s must be finite and > 0 as a float32, not %r" % (what, name, value))
    return v


def _check_max_dist_cell(what, max_dist, cell):
    """-> (max_dist, cell) as float32 values; cell defaults to float32(max_dist / 4) and must be >= max_dist / 15."""
    md = _check_length(what, "max_dist", max_dist)
    c = _check_length(what, "cell", md / 4 if cell is None else cell)
    if not c >= md / MIN_CELLS_PER_MAX_DIST:
        raise RuntimeError("%s: cell must be >= max_dist / %d = %r, not %r" % (what, MIN_CELLS_PER_MAX_DIST,
                                                                                md / MIN_CELLS_PER_MAX_DIST, cell))
    return md, c


def _check_cloud(what, name, points):
    if not isinstance(points, torch.Tensor):
        raise RuntimeError("%s: %s must be a torch tensor (on the GPU) or a CloudGrid, not %s" % (what, name, type(points).__name__))
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise RuntimeError("%s: %s must be [M,3] float32, not %s %s" % (what, name, tuple(points.shape), points.dtype))
    if points.shape[0] > MAX_CLOUD_POINTS:
        raise RuntimeError("%s: at most 2^29 points, not %d in %s" % (what, points.shape[0], name))


class CloudGrid:
    """The uniform hash grid of a cloud: ``points`` [M,3] float32 on the GPU, binned into cells of edge
    ``cell`` (its float32 value; finite, > 0).  Built once and reused: a ground-truth cloud is scored against many clouds, and
    ``nearest_distances`` / ``score_clouds`` take a CloudGrid wherever they take a cloud, as the query (its cell order is the
    order the queries are handled in) and as the target.  Points with a NaN or infinite coordinate, or beyond 2^20 cells from the
    origin on an axis, take no part: ``dropped`` counts them.  The cells are the voxels of ``thin_points``: the same table
    (``mvster_voxel_thin_insert``), then ``mvster_cloud_grid_build``.  One host synchronisation (the occupied cells, ``dropped``
    and the table's status in one copy).  ``table_slots`` as in ``thin_points``; nothing computed from the grid depends on it.
    No CPU fallback."""

    def __init__(self, points, cell, table_slots=None, _what="CloudGrid", _name="points", _read_back=True):
        self.cell = _check_length(_what, "cell", cell)
        _check_cloud(_what, _name, points)
        M = self.M = points.shape[0]
        slots = thin_slots(M) if table_slots is None else table_slots
        if not isinstance(slots, int) or slots < thin_slots(M) or slots & (slots - 1) or slots > 1 << 30:
            raise RuntimeError("%s: table_slots must be a power of two, >= max(64, 2 * M) = %d and <= 2^30, not %r" %
                               (_what, max(64, 2 * M), table_slots))
        if not points.is_cuda:
            raise RuntimeError("mvster_amd.fusion.%s runs on MI355X only: %s must be a tensor on the GPU (there is no CPU "
                               "fallback)" % (_what, _name))
        dev = self.device = points.device
        self.points, self.slots = points.contiguous(), slots
        # (an empty cloud's table holds vox::kEmpty everywhere; any other is filled by mvster_voxel_thin_insert)
        self.keys = torch.full((slots,), -1, device=dev, dtype=torch.int64) if M == 0 else torch.empty(slots, device=dev, dtype=torch.int64)
        self.cell_of_slot = torch.empty(slots, device=dev, dtype=torch.int32)
        self.cell_of_point = torch.empty(M, device=dev, dtype=torch.int32)
        self.starts = torch.zeros(1, device=dev, dtype=torch.int64)
        self.records = torch.empty(0, 4, device=dev, dtype=torch.int32)
        self.ncells, self.dropped = 0, 0
        if M == 0:
            return
        lib = _lib.load()
        with torch.cuda.device(dev):
            nblk = lib.mvster_voxel_thin_blocks(M)
            _lib.check(min(nblk, 0), "voxel_thin_blocks")
            wg_counts = torch.empty(nblk, device=dev, dtype=torch.int32)
            wg_offsets = torch.empty(nblk + 3, device=dev, dtype=torch.int64)
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = lib.mvster_voxel_thin_insert(self.points.data_ptr(), M, self.cell, self.keys.data_ptr(), self.cell_of_slot.data_ptr(),
                                              slots, self.cell_of_point.data_ptr(), wg_counts.data_ptr(), wg_offsets.data_ptr(),
                                              stream)
            _lib.check(rc, "voxel_thin_insert")
            if _read_back:
                U, self.dropped, status = wg_offsets[nblk:].tolist()             # the one host sync
                if status:
                    raise RuntimeError("%s: a point found no slot in a table of %d slots for %d points" % (_what, slots, M))
                if U == 0:                                                       # every point invalid: cell_of_point is all -1
                    return
            else:                                                                # queries: M bounds the cells, nothing is read
                U, self.dropped = M, wg_offsets[nblk + 1]
            counts = torch.empty(U, device=dev, dtype=torch.int32)
            local = torch.empty(M, device=dev, dtype=torch.int32)
            self.starts = torch.empty(U + 1, device=dev, dtype=torch.int64)
            self.records = torch.empty(M - (self.dropped if _read_back else 0), 4, device=dev, dtype=torch.int32)
            rc = lib.mvster_cloud_grid_build(self.points.data_ptr(), M, self.cell_of_slot.data_ptr(), self.cell_of_point.data_ptr(),
                                             wg_offsets.data_ptr(), counts.data_ptr(), local.data_ptr(), self.starts.data_ptr(), U,
                                             self.records.data_ptr(), stream)
            _lib.check(rc, "cloud_grid_build")
            self.ncells = U

    def __len__(self):
        return self.M


def _as_grid(what, name, cloud, cell, table_slots=None, read_back=True):
    """A cloud given as a tensor or as a CloudGrid -> a CloudGrid of edge ``cell``."""
    if isinstance(cloud, CloudGrid):
        if cloud.cell != cell:
            raise RuntimeError("%s: the CloudGrid given as %s has cell %r, not the cell %r of this call" % (what, name, cloud.cell, cell))
        return cloud
    return CloudGrid(cloud, cell, table_slots, _what=what, _name=name, _read_back=read_back)


def _nearest(what, query, target, max_dist, cell, table_slots, read_back_query):
    md = _check_length(what, "max_dist", max_dist)
    if cell is None and isinstance(target, CloudGrid):
        cell = target.cell
    elif cell is None and isinstance(query, CloudGrid):
        cell = query.cell
    md, c = _check_max_dist_cell(what, md, cell)
    for name, cloud in (("query", query), ("target", target)):                  # both before either grid is built
        if not isinstance(cloud, CloudGrid):
            _check_cloud(what, name, cloud)
    tg = _as_grid(what, "target", target, c, table_slots)
    qg = _as_grid(what, "query", query, c, None, read_back_query)
    if qg.device != tg.device:
        raise RuntimeError("%s: query and target must be on one GPU, not %s and %s" % (what, qg.device, tg.device))
    dev, Q = qg.device, qg.M
    out = dict(dist=torch.empty(Q, device=dev, dtype=torch.float32), dist2=torch.empty(Q, device=dev, dtype=torch.float64),
               index=torch.empty(Q, device=dev, dtype=torch.int64), dropped_query=qg.dropped, dropped_target=tg.dropped)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().mvster_cloud_nn_query(
            qg.records.data_ptr(), qg.cell_of_point.data_ptr(), qg.starts.data_ptr() + 8 * (qg.starts.numel() - 1), Q,
            tg.keys.data_ptr(), tg.cell_of_slot.data_ptr(), tg.slots, tg.starts.data_ptr(), tg.records.data_ptr(), tg.ncells,
            tg.records.shape[0], md, c, out["dist"].data_ptr(), out["dist2"].data_ptr(), out["index"].data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "cloud_nn_query")
    return out


def nearest_distances(query, target, max_dist, cell=None, table_slots=None):
    """For every point of ``query`` its nearest point of ``target`` up to ``max_dist``, on the GPU (defined
    exactly in mvster_amd/csrc/nn_math.h): ``query`` [Q,3] and ``target`` [M,3] float32 tensors on the GPU, or either as a
    ``CloudGrid`` (built once, reused).  In fp64, d2 = (dx*dx + dy*dy) + dz*dz; a query's candidates are the valid targets with
    d2 <= max_dist^2 (``max_dist`` at its float32 value; finite, > 0) and its result the candidate with the smallest
    (d2, index).  -> dict of GPU tensors at the query's positions: ``dist2`` [Q] float64 = d2, ``dist`` [Q] float32 =
    (float)sqrt(d2), ``index`` [Q] int64 into the target as given; +inf / +inf / -1 without a candidate, NaN / NaN / -1 for an
    invalid query (a NaN or infinite coordinate, or beyond 2^20 cells from the origin); invalid targets take no part.
    ``dropped_target`` (int) and ``dropped_query`` count the invalid points; ``dropped_query`` is an int for a CloudGrid and a
    0-dim int64 tensor on the GPU for a tensor, whose binning synchronises nothing.  ``cell``: the edge of the search grid,
    default float32(max_dist / 4) or the CloudGrid's; >= max_dist / 15.  The result depends neither on ``cell`` (but through
    which points are valid), nor on ``table_slots`` (the target's table, as in ``thin_points``), nor on the run.  An empty or
    entirely invalid target gives every valid query +inf / -1.  One host synchronisation where the target is a tensor (its
    grid), none where it is a CloudGrid.  No CPU fallback."""
    return _nearest("nearest_distances", query, target, max_dist, cell, table_slots, False)


def _check_tau(what, tau, md):
    if tau is None:
        return None
    t = _check_length(what, "tau", tau)
    if not t <= md:
        raise RuntimeError("%s: tau must be <= max_dist = %r, not %r" % (what, md, tau))
    return t


def score_clouds(pred, gt, max_dist, tau=None, cell=None):
    """The scores of a predicted cloud against a ground-truth cloud from ``nearest_distances`` both ways.
    ``pred`` / ``gt``: [N,3] float32 tensors on the GPU or CloudGrids.  -> dict of Python numbers:
    ``accuracy`` = the mean of pred -> gt ``dist`` over those <= ``max_dist``, ``completeness`` = the same for gt -> pred,
    ``overall`` = their mean (DTU's three numbers, distances capped by leaving out what is beyond ``max_dist``); with ``tau``
    (0 < tau <= max_dist) also ``precision`` = the pred points with dist < tau over the valid pred points, ``recall`` = the same
    for gt -> pred and ``fscore`` = 2PR / (P + R), 0 when P + R = 0 (Tanks and Temples, ETH3D).  An empty mean is NaN.  The raw
    numbers come along: ``pred_valid`` / ``pred_within`` / ``pred_below_tau`` (counts), ``pred_sum`` (fp64 sum of the dist <=
    max_dist), the same with ``gt_``, ``dropped_pred``, ``dropped_gt``.  The sums are formed per workgroup and added in a fixed
    order: two runs give the same bytes.  One read-back of its own, besides the one of each grid it has to build.

    DTU's observability masks and ground plane are NOT applied: those files are not ours to read.  The numbers are the DTU
    protocol's only for clouds the caller has masked already.  The whole protocol -- point reduction, masks, plane, median and
    variance -- is ``mvster_amd.dtu_eval.evaluate_dtu_scan``."""
    what = "score_clouds"
    md = _check_length(what, "max_dist", max_dist)
    t = _check_tau(what, tau, md)
    if cell is None:
        cell = next((g.cell for g in (pred, gt) if isinstance(g, CloudGrid)), None)
    md, c = _check_max_dist_cell(what, md, cell)
    for name, cloud in (("pred", pred), ("gt", gt)):
        if not isinstance(cloud, CloudGrid):
            _check_cloud(what, name, cloud)
    gp, gg = _as_grid(what, "pred", pred, c), _as_grid(what, "gt", gt, c)
    ways = (_nearest(what, gp, gg, md, c, None, True), _nearest(what, gg, gp, md, c, None, True))
    dev = gp.device
    stats = torch.zeros(2, 4, device=dev, dtype=torch.float64)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for w, way in enumerate(ways):
            Q = way["dist"].shape[0]
            if Q == 0:
                continue
            slots = lib.mvster_cloud_score_slots(Q)
            _lib.check(min(slots, 0), "cloud_score_slots")
            partial = torch.empty(slots, 4, device=dev, dtype=torch.float64)
            rc = lib.mvster_cloud_score(way["dist"].data_ptr(), Q, md, 0.0 if t is None else t, partial.data_ptr(),
                                        stats[w].data_ptr(), stream)
            _lib.check(rc, "cloud_score")
    rows = stats.tolist()                                                        # the one read-back
    out = dict(dropped_pred=gp.dropped, dropped_gt=gg.dropped)
    for name, (valid, within, below, total) in zip(("pred", "gt"), rows):
        out[name + "_valid"], out[name + "_within"], out[name + "_sum"] = int(valid), int(within), total
        if t is not None:
            out[name + "_below_tau"] = int(below)
    nan = float("nan")
    out["accuracy"] = out["pred_sum"] / out["pred_within"] if out["pred_within"] else nan
    out["completeness"] = out["gt_sum"] / out["gt_within"] if out["gt_within"] else nan
    out["overall"] = (out["accuracy"] + out["completeness"]) / 2
    if t is not None:
        P = out["precision"] = out["pred_below_tau"] / out["pred_valid"] if out["pred_valid"] else nan
        R = out["recall"] = out["gt_below_tau"] / out["gt_valid"] if out["gt_valid"] else nan
        out["fscore"] = 0.0 if P + R == 0 else 2 * P * R / (P + R)
    return out


# ---- cleaning a fused cloud: k nearest, outlier filters, normals --------------------------------------

MAX_K = 32                              # knn::kMaxK of csrc/knn_math.h

RadiusOutliers = collections.namedtuple("RadiusOutliers", "radius nb_points")
StatisticalOutliers = collections.namedtuple("StatisticalOutliers", "k std_ratio max_dist")
Normals = collections.namedtuple("Normals", "k max_dist")


def _check_k(what, k, name="k", hi=MAX_K):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= hi:
        raise RuntimeError("%s: %s must be an integer in 1 .. %d, not %r" % (what, name, hi, k))
    return int(k)


def _check_ratio(what, std_ratio, name="std_ratio"):
    try:
        r = float(std_ratio)
    except (TypeError, ValueError):
        raise RuntimeError("%s: %s must be a number, not %r" % (what, name, std_ratio)) from None
    if not np.isfinite(r):
        raise RuntimeError("%s: %s must be finite, not %r" % (what, name, std_ratio))
    return r


def _self_grid(what, points, max_dist, cell, name="max_dist"):
    """The checks every operation on one cloud shares, then its grid -> (grid, max_dist, cell)."""
    md = _check_length(what, name, max_dist)
    if cell is None and isinstance(points, CloudGrid):
        cell = points.cell
    try:
        md, c = _check_max_dist_cell(what, md, cell)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace("max_dist", name)) from None
    if not isinstance(points, CloudGrid):
        _check_cloud(what, "points", points)
    return _as_grid(what, "points", points, c), md, c


def _grid_args(g):
    """A cloud's grid as the kernels of geo_knn.hip take it, searched against itself."""
    return (g.records.data_ptr(), g.cell_of_point.data_ptr(), g.M, g.keys.data_ptr(), g.cell_of_slot.data_ptr(), g.slots,
            g.starts.data_ptr(), g.ncells, g.records.shape[0])


def nearest_neighbors(query, target, k, max_dist, cell=None, table_slots=None, exclude_self=False):
    """For every point of ``query`` its ``k`` (1 .. 32) nearest points of ``target`` up to ``max_dist``, on the GPU (DESIGN.md
    section 4.20; defined exactly in mvster_amd/csrc/knn_math.h).  Clouds, ``max_dist``, ``cell``, ``table_slots`` and point
    validity as in ``nearest_distances``.  A query's candidates are the valid targets with d2 <= max_dist^2; with
    ``exclude_self`` (needs as many queries as targets) the target whose index is the query's own position is left out -- only
    that one, a duplicate with another index stays.  -> dict of GPU tensors: ``dist2`` [Q,k] float64 and ``index`` [Q,k] int64,
    the first min(k, candidates) candidates in ascending (d2, index) order, unfilled places +inf / -1, an invalid query NaN / -1;
    ``count`` [Q] int32 (0 for an invalid query); ``dropped_query`` / ``dropped_target`` as in ``nearest_distances``.  k = 1
    gives ``nearest_distances``.  The result depends neither on ``cell``, nor on ``table_slots``, nor on the run.  No CPU
    fallback."""
    what = "nearest_neighbors"
    k = _check_k(what, k)
    md = _check_length(what, "max_dist", max_dist)
    if cell is None and isinstance(target, CloudGrid):
        cell = target.cell
    elif cell is None and isinstance(query, CloudGrid):
        cell = query.cell
    md, c = _check_max_dist_cell(what, md, cell)
    for name, cloud in (("query", query), ("target", target)):                  # both before either grid is built
        if isinstance(cloud, CloudGrid):
            _as_grid(what, name, cloud, c)
        else:
            _check_cloud(what, name, cloud)
    if exclude_self and len(query) != len(target):
        raise RuntimeError("%s: exclude_self needs as many queries as targets (the same cloud), not %d and %d" %
                           (what, len(query), len(target)))
    tg = _as_grid(what, "target", target, c, table_slots)
    qg = tg if query is target else _as_grid(what, "query", query, c, None, False)
    if qg.device != tg.device:
        raise RuntimeError("%s: query and target must be on one GPU, not %s and %s" % (what, qg.device, tg.device))
    dev, Q = qg.device, qg.M
    out = dict(dist2=torch.empty(Q, k, device=dev, dtype=torch.float64), index=torch.empty(Q, k, device=dev, dtype=torch.int64),
               count=torch.empty(Q, device=dev, dtype=torch.int32), dropped_query=qg.dropped, dropped_target=tg.dropped)
    if Q == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().mvster_cloud_knn_query(
            qg.records.data_ptr(), qg.cell_of_point.data_ptr(), qg.starts.data_ptr() + 8 * (qg.starts.numel() - 1), Q,
            tg.keys.data_ptr(), tg.cell_of_slot.data_ptr(), tg.slots, tg.starts.data_ptr(), tg.records.data_ptr(), tg.ncells,
            tg.records.shape[0], md, c, k, 1 if exclude_self else 0, tg.M, out["dist2"].data_ptr(), out["index"].data_ptr(),
            out["count"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "cloud_knn_query")
    return out


def _compact(g, flags, wg_offsets, kept, colors=None):
    """The kept points of a grid's cloud in cloud order (mvster_reg_crop_emit) -> (index int64, points, colors or None)."""
    dev = g.device
    index = torch.empty(kept, device=dev, dtype=torch.int64)
    points = torch.empty(kept, 3, device=dev, dtype=torch.float32)
    cols = torch.empty(kept, 3, device=dev, dtype=torch.uint8) if colors is not None else None
    if kept:
        rc = _lib.load().mvster_reg_crop_emit(g.points.data_ptr(), None if colors is None else colors.data_ptr(), g.M, None,
                                              flags.data_ptr(), wg_offsets.data_ptr(), kept, 0, points.data_ptr(),
                                              None if cols is None else cols.data_ptr(), index.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "reg_crop_emit")
    return index, points, cols


def _check_colors(what, points, colors):
    if colors is None:
        return None
    M = len(points)
    if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (M, 3) or colors.dtype != torch.uint8:
        raise RuntimeError("%s: colors must be a [M,3] uint8 tensor with the M of points (%d)" % (what, M))
    if not colors.is_cuda:
        raise RuntimeError("%s: colors must be on the GPU of points (there is no CPU fallback)" % what)
    return colors.contiguous()


def radius_outliers(points, radius, nb_points, cell=None, colors=None):
    """The radius outlier filter on the GPU (PCL's RadiusOutlierRemoval, Open3D's remove_radius_outlier):
    ``neighbours`` = the valid points within ``radius`` (d2 <= radius^2 in fp64) of a point, the point itself -- its own index,
    not its duplicates -- left out; a point is kept iff it is valid and has at least ``nb_points`` (an integer >= 1) of them.
    ``points`` [M,3] float32 on the GPU or a ``CloudGrid``; ``cell`` as in ``nearest_distances`` (default radius / 4).  ->
    dict: ``keep`` [M] bool, ``neighbours`` [M] int32 (0 for an invalid point), ``index`` [K] int64 (the kept positions, cloud
    order), ``points`` [K,3] (and ``colors`` [K,3] where ``colors`` [M,3] uint8 is given) on the GPU, ``dropped`` (invalid
    points).  One read-back of its own (K), besides the grid's.  No atomics: two runs give the same bytes.  No CPU fallback."""
    what = "radius_outliers"
    nb = _check_k(what, nb_points, "nb_points", (1 << 31) - 1)
    colors = _check_colors(what, points, colors)
    g, r, c = _self_grid(what, points, radius, cell, "radius")
    dev, M = g.device, g.M
    keep = torch.zeros(M, device=dev, dtype=torch.uint8)
    neighbours = torch.zeros(M, device=dev, dtype=torch.int32)
    kept = 0
    wg_offsets = None
    if M:
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.mvster_cloud_radius_count(*_grid_args(g), r, c, neighbours.data_ptr(), stream), "cloud_radius_count")
            tiles = lib.mvster_reg_blocks(M)
            _lib.check(min(tiles, 0), "reg_blocks")
            wg_counts = torch.empty(tiles, device=dev, dtype=torch.int32)
            wg_offsets = torch.empty(tiles + 1, device=dev, dtype=torch.int64)
            _lib.check(lib.mvster_cloud_keep_flags(g.cell_of_point.data_ptr(), neighbours.data_ptr(), nb, None, None, M,
                                                   keep.data_ptr(), wg_counts.data_ptr(), wg_offsets.data_ptr(), stream),
                       "cloud_keep_flags")
            kept = int(wg_offsets[tiles])                                        # the one read-back
    with torch.cuda.device(dev):
        index, pts, cols = _compact(g, keep, wg_offsets, kept, colors)
    out = dict(keep=keep.bool(), neighbours=neighbours, index=index, points=pts, dropped=g.dropped)
    if cols is not None:
        out["colors"] = cols
    return out


def statistical_outliers(points, k, std_ratio, max_dist, cell=None, colors=None):
    """The statistical outlier filter on the GPU (PCL's StatisticalOutlierRemoval, Open3D's remove_statistical_outlier, with a
    search cap).  A valid point takes part iff it has ``k`` (1 .. 32) other points within ``max_dist``;
    ``mean`` = the mean distance to its k nearest.  Over the n participants mu and sigma (n - 1 in the denominator; 0 for
    n < 2) of ``mean``; kept iff it takes part and mean <= ``threshold`` = mu + ``std_ratio`` * sigma.  A point with fewer than k
    neighbours within ``max_dist`` is isolated: removed, and no part of the statistics.  -> dict: ``keep`` [M] bool, ``mean``
    [M] float64 (+inf for an isolated point, NaN for an invalid one), ``n`` (int), ``mu``, ``sigma``, ``threshold`` (Python
    floats), ``index`` / ``points`` (/ ``colors``) of the kept points in cloud order, ``dropped``.  The sums are formed per
    workgroup and added in a fixed order, no floating-point atomics: two runs give the same bytes.  One read-back of its own
    (the kept count and the four scalars in one copy), besides the grid's.  No CPU fallback."""
    what = "statistical_outliers"
    k = _check_k(what, k)
    ratio = _check_ratio(what, std_ratio)
    colors = _check_colors(what, points, colors)
    g, md, c = _self_grid(what, points, max_dist, cell)
    dev, M = g.device, g.M
    keep = torch.zeros(M, device=dev, dtype=torch.uint8)
    mean = torch.empty(M, device=dev, dtype=torch.float64)
    nan = float("nan")
    vals, wg_offsets = [0.0, nan, 0.0, nan, 0.0], None
    if M:
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            count = torch.empty(M, device=dev, dtype=torch.int32)
            _lib.check(lib.mvster_cloud_knn_mean(*_grid_args(g), md, c, k, count.data_ptr(), mean.data_ptr(), stream),
                       "cloud_knn_mean")
            rows = lib.mvster_cloud_knn_stats_rows(M)
            _lib.check(min(rows, 0), "cloud_knn_stats_rows")
            partial = torch.empty(rows, 2, device=dev, dtype=torch.float64)
            stats = torch.empty(5, device=dev, dtype=torch.float64)
            _lib.check(lib.mvster_cloud_knn_stats(mean.data_ptr(), M, ratio, partial.data_ptr(), stats.data_ptr(), stream),
                       "cloud_knn_stats")
            tiles = lib.mvster_reg_blocks(M)
            _lib.check(min(tiles, 0), "reg_blocks")
            wg_counts = torch.empty(tiles, device=dev, dtype=torch.int32)
            wg_offsets = torch.empty(tiles + 1, device=dev, dtype=torch.int64)
            _lib.check(lib.mvster_cloud_keep_flags(None, None, 0, mean.data_ptr(), stats.data_ptr(), M, keep.data_ptr(),
                                                   wg_counts.data_ptr(), wg_offsets.data_ptr(), stream), "cloud_keep_flags")
            vals = stats.tolist()                                                # the one read-back
    with torch.cuda.device(dev):
        index, pts, cols = _compact(g, keep, wg_offsets, int(vals[4]), colors)
    out = dict(keep=keep.bool(), mean=mean, n=int(vals[0]), mu=vals[1], sigma=vals[2], threshold=vals[3], index=index,
               points=pts, dropped=g.dropped)
    if cols is not None:
        out["colors"] = cols
    return out


def estimate_normals(points, k, max_dist, toward=None, cell=None):
    """A normal per point on the GPU (defined exactly in mvster_amd/csrc/knn_math.h): the unit
    eigenvector of the smallest eigenvalue of the covariance of the point and its ``k`` (1 .. 32) nearest other points within
    ``max_dist``, by a fixed number of cyclic Jacobi sweeps in fp64.  ``toward`` [M,3] float32 (one position per point, e.g.
    the camera centre it was seen from): the normal is turned so that n . (toward - p) >= 0; without it, or where that product
    is exactly 0, the component of largest magnitude is positive.  -> dict: ``normals`` [M,3] float32 and ``valid`` [M] bool;
    a point with fewer than two neighbours, or an invalid one, gets zeros and False.  Nothing is read back besides the grid's
    read-back.  No CPU fallback."""
    what = "estimate_normals"
    k = _check_k(what, k)
    if toward is not None and (not isinstance(toward, torch.Tensor) or tuple(toward.shape) != (len(points), 3) or
                               toward.dtype != torch.float32):
        raise RuntimeError("%s: toward must be a [M,3] float32 tensor with the M of points (%d)" % (what, len(points)))
    g, md, c = _self_grid(what, points, max_dist, cell)
    dev, M = g.device, g.M
    if toward is not None:
        if toward.device != dev:
            raise RuntimeError("%s: toward must be on the GPU of points (there is no CPU fallback)" % what)
        toward = toward.contiguous()
    normals = torch.zeros(M, 3, device=dev, dtype=torch.float32)
    valid = torch.zeros(M, device=dev, dtype=torch.uint8)
    if M:
        with torch.cuda.device(dev):
            rc = _lib.load().mvster_cloud_knn_normals(*_grid_args(g), md, c, k, g.points.data_ptr(),
                                                      None if toward is None else toward.data_ptr(), normals.data_ptr(),
                                                      valid.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(rc, "cloud_knn_normals")
    return dict(normals=normals, valid=valid.bool())


def _check_clean(what, outliers, normals):
    """The ``outliers`` / ``normals`` keywords of the scan-level entry points, checked before anything runs."""
    if outliers is not None:
        if isinstance(outliers, RadiusOutliers):
            _check_length(what, "outliers.radius", outliers.radius)
            _check_k(what, outliers.nb_points, "outliers.nb_points", (1 << 31) - 1)
        elif isinstance(outliers, StatisticalOutliers):
            _check_k(what, outliers.k, "outliers.k")
            _check_ratio(what, outliers.std_ratio, "outliers.std_ratio")
            _check_length(what, "outliers.max_dist", outliers.max_dist)
        else:
            raise RuntimeError("%s: outliers must be None, a RadiusOutliers or a StatisticalOutliers, not %r" % (what, outliers))
    if normals is not None:
        if not isinstance(normals, Normals):
            raise RuntimeError("%s: normals must be None or a Normals, not %r" % (what, normals))
        _check_k(what, normals.k, "normals.k")
        _check_length(what, "normals.max_dist", normals.max_dist)


def _clean_scene(res, Es, pairs, thinned, outliers, normals):
    """fuse_scene's last step: the cloud that would be written through the filter, then the normals -> the ``final_*`` keys."""
    pre = "thin_" if thinned else ""
    pts, cols = res[pre + "points"], res[pre + "colors"]
    dev = pts.device
    out = {}
    if isinstance(outliers, RadiusOutliers):
        f = radius_outliers(pts, outliers.radius, outliers.nb_points, colors=cols)
        out.update(final_radius=float(np.float32(outliers.radius)), final_nb_points=int(outliers.nb_points))
    elif isinstance(outliers, StatisticalOutliers):
        f = statistical_outliers(pts, outliers.k, outliers.std_ratio, outliers.max_dist, colors=cols)
        out.update(("final_" + key, f[key]) for key in ("n", "mu", "sigma", "threshold"))
    else:
        f = dict(points=pts, colors=cols, index=torch.arange(len(pts), device=dev, dtype=torch.int64))
    out.update(final_points=f["points"], final_colors=f["colors"], final_index=f["index"])
    if normals is not None:
        # the camera centre -R^T T = inv(E)[:3, 3] of the reference view a point came from (a voxel: of its first point)
        centres = np.stack([np.linalg.inv(np.asarray(Es[r], np.float64))[:3, 3] for r, _ in pairs]).astype(np.float32)
        view = torch.repeat_interleave(torch.arange(len(pairs), device=dev), res["counts"].to(dev), output_size=len(res["points"]))
        if thinned:
            view = view[res["thin_first"]]
        toward = torch.from_numpy(centres).to(dev)[view[f["index"]]]
        nrm = estimate_normals(f["points"], normals.k, normals.max_dist, toward=toward)
        out.update(final_normals=nrm["normals"], final_normal_valid=nrm["valid"])
    return out


def fuse_scene(depths, confidences, images, Ks, Es, pairs, conf_thres, thres_view, pix_thres=None, rel_thres=None,
               device=None, scratch_budget=SCRATCH_BUDGET, events=None, method="normal", pix_base=PIX_BASE,
               rel_base=REL_BASE, voxel_size=None, voxel_reduce="mean", outliers=None, normals=None, mesh=None, mesh_clean=None):
    """filter_depth (test_mvs4.py:331-421) for a scan whose maps are in memory.  depths / confidences [V,H,W], images
    [V,H,W,3] (uint8, or float 0..1 as ``read_img`` returns it), Ks [V,3,3], Es [V,4,4]: NumPy arrays, tensors or
    sequences of them, indexed by the view numbers in ``pairs`` [(ref_view, [src_view, ...]), ...].  Tensors already on
    the GPU are used as they are.  -> SceneResult (tensors on the GPU): ``points`` [M,3] float32 and ``colors`` [M,3]
    uint8 in the reference's order (reference views in pair order, pixels row-major), ``counts`` [R] int64 survivors
    per reference view, ``photo_mask`` / ``geo_mask`` / ``final_mask`` [R,H,W] bool, ``geo_mask_sum`` [R,H,W] int32,
    ``depth_est_averaged`` [R,H,W] float64.  The only host synchronisation is the read-back of the workgroup offsets
    at the view boundaries (M and ``counts``), once per call -- once per chunk of reference views when the tables and
    scan scratch of the whole scan would exceed ``scratch_budget`` bytes; the result does not depend on the chunking.
    ``events``: a list that receives (name, start, end) torch.cuda.Event triples around the two library calls (timing).

    ``method``: ``"normal"`` is the reference's rule, a vote per source view within ``pix_thres`` pixels (default 1) and
    ``rel_thres`` relative depth (default 0.01), ``thres_view`` votes to survive.  ``"dynamic"`` is dynamic consistency
    checking: a pixel survives if for some n in ``thres_view`` .. its number of sources at least n
    sources agree within n * ``pix_base`` pixels and n * ``rel_base`` relative depth; the result then also holds
    ``geo_level`` [R,H,W] uint8, that n (0 = none), ``geo_mask_sum`` counts the sources agreeing at the loosest level and
    ``depth_est_averaged`` averages over them.  At most 32 sources per reference view; ``pix_thres`` / ``rel_thres``
    belong to ``"normal"`` and may not be given.

    ``voxel_size`` (default None: nothing changes): the whole cloud, after its chunks are joined, also goes through
    ``thin_points(points, colors, voxel_size, voxel_reduce)`` and the result holds ``thin_points``, ``thin_colors``,
    ``thin_counts``, ``thin_first`` and ``thin_dropped`` beside the unchanged ``points``, ``colors`` and ``counts``.

    ``outliers`` (a ``RadiusOutliers`` or a ``StatisticalOutliers``) / ``normals`` (a ``Normals``); default None, None: nothing
    changes.  Otherwise the cloud that would be written -- ``thin_*`` with a ``voxel_size``, else ``points`` / ``colors`` -- goes
    through ``radius_outliers`` / ``statistical_outliers``, then ``estimate_normals``, and the result additionally holds
    ``final_points``, ``final_colors``, ``final_index`` (int64, into the cloud it was taken from), the filter's scalars
    (``final_n``, ``final_mu``, ``final_sigma``, ``final_threshold``, or ``final_radius``, ``final_nb_points``) and, with
    ``normals``, ``final_normals`` / ``final_normal_valid``: oriented toward the camera centre -R^T T of the reference view a
    point came from (a voxel: of its first point).  Every other key stays byte-equal.

    ``mesh`` (a ``TSDFMesh(voxel_size, trunc=None, min_weight=2, sparse=False)``; default None: nothing changes and no launch is
    added; ``sparse=True``: the same mesh from a brick-sparse volume, DESIGN.md section 4.25, in another vertex order): the
    reference views' ``depth_est_averaged`` (as float32) under ``final_mask``, their images and cameras are fused into a TSDF
    over the box of the cloud that would be written (``final_*``, else ``thin_*``, else ``points``) and meshed by marching
    tetrahedra (``mesh.mesh_scene``); the result additionally holds ``mesh_vertices`` [Nv,3] float32,
    ``mesh_colors`` [Nv,3] uint8, ``mesh_triangles`` [Nt,3] int32 and ``mesh_volume`` (the grid: origin, voxel_size, dims,
    trunc, min_weight, bounds; None for an empty cloud).  Every other key stays byte-equal.

    ``mesh_clean`` (a ``MeshClean(weld=True, min_triangles=0, largest_only=False, normals=False)``, only with ``mesh``; default
    None: nothing changes and no launch is added): the extracted mesh goes through ``mesh.clean_mesh`` and
    the ``mesh_*`` keys hold the cleaned mesh, with ``mesh_clean_stats`` and, where normals were asked for, ``mesh_normals``
    [Nv,3] float32 and ``mesh_normals_valid`` [Nv] uint8."""
    _check_method("fuse_scene", method, pix_thres, rel_thres)
    _check_voxel("fuse_scene", voxel_size, voxel_reduce)
    _check_clean("fuse_scene", outliers, normals)
    mesh_spec = mesh_mod.check_mesh_spec("fuse_scene", mesh)
    clean_spec = mesh_mod.check_clean_spec("fuse_scene", mesh_clean, mesh)
    dynamic = method == "dynamic"
    pix_thres = PIX_THRES if pix_thres is None else pix_thres
    rel_thres = REL_THRES if rel_thres is None else rel_thres
    if device is None:
        devs = [m.device for x in (depths, confidences, images) for m in ([x] if isinstance(x, torch.Tensor) else
                                                                          x if not isinstance(x, np.ndarray) else [])
                if isinstance(m, torch.Tensor) and m.is_cuda]
        if not devs:
            raise RuntimeError("mvster_amd.fusion.fuse_scene runs on MI355X only: pass device= or tensors on the GPU "
                               "(there is no CPU fallback)")
        device = devs[0]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("mvster_amd.fusion.fuse_scene runs on MI355X only (there is no CPU fallback)")
    Ks = [_np32(k) for k in Ks]
    Es = [_np32(e) for e in Es]
    tables = scene_tables(pairs, Ks, Es)
    depth = _scene_stack(depths, dev, np.float32, "depth")
    conf = _scene_stack(confidences, dev, np.float32, "confidence")
    first = images if isinstance(images, (torch.Tensor, np.ndarray)) else images[0]
    is_u8 = first.dtype in (torch.uint8, np.dtype(np.uint8))
    img = _scene_stack(images, dev, np.uint8 if is_u8 else np.float32, "image")
    if depth.dim() != 3 or conf.shape != depth.shape or tuple(img.shape) != tuple(depth.shape) + (3,):
        raise RuntimeError("fuse_scene: map sizes differ inside the scan (depth %s, confidence %s, images %s)" %
                           (tuple(depth.shape), tuple(conf.shape), tuple(img.shape)))
    V, H, W = depth.shape
    if V != len(Ks):
        raise RuntimeError("fuse_scene: %d depth maps for %d cameras" % (V, len(Ks)))
    R, smax = tables.pair_table.shape
    if dynamic and smax > MAX_DYNAMIC_SOURCES:
        raise RuntimeError("fuse_scene: method 'dynamic' takes at most %d source views per reference view, a row of "
                           "pairs has %d" % (MAX_DYNAMIC_SOURCES, smax))
    lib = _lib.load()
    nblk = lib.mvster_geo_scene_blocks(1, H, W)
    _lib.check(min(nblk, 0), "geo_scene_blocks")
    per_view = nblk * 12 + 8 + smax * (4 + 42 * 8) + 4 + 30 * 8          # counts + offsets + table rows of one view
    chunk = max(1, min(R, int(scratch_budget) // per_view))
    mask_sum = torch.empty(R, H, W, device=dev, dtype=torch.int32)
    avg = torch.empty(R, H, W, device=dev, dtype=torch.float64)
    photo, geo, final = (torch.empty(R, H, W, device=dev, dtype=torch.bool) for _ in range(3))
    level = torch.empty(R, H, W, device=dev, dtype=torch.uint8) if dynamic else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    pts, cols, counts = [], [], []
    for r0 in range(0, R, chunk):
        r1 = min(R, r0 + chunk)
        n = r1 - r0
        # one upload for the chunk's tables: int32 pair table and view list, then the float64 blocks
        ints = np.concatenate([tables.pair_table[r0:r1].reshape(-1), tables.ref_view[r0:r1]])
        if ints.size % 2:
            ints = np.concatenate([ints, np.zeros(1, np.int32)])
        host = np.concatenate([ints.view(np.float64), tables.ref_mats[r0:r1].reshape(-1),
                               tables.view_mats[r0:r1].reshape(-1)])
        blob = torch.from_numpy(host).to(dev)
        base = blob.data_ptr()
        p_pairs, p_ref = base, base + 4 * n * smax
        p_rm = base + 4 * ints.size
        p_vm = p_rm + 8 * n * 30
        wg_counts = torch.empty(n * nblk, device=dev, dtype=torch.int32)
        wg_offsets = torch.empty(n * nblk + 1, device=dev, dtype=torch.int64)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if events is not None else None
        if marks:
            marks[0].record()
        if dynamic:
            rc = lib.mvster_geo_scene_filter_dynamic(depth.data_ptr(), conf.data_ptr(), p_pairs, p_ref, p_rm, p_vm,
                                                     mask_sum[r0:r1].data_ptr(), avg[r0:r1].data_ptr(),
                                                     photo[r0:r1].data_ptr(), geo[r0:r1].data_ptr(), final[r0:r1].data_ptr(),
                                                     level[r0:r1].data_ptr(), wg_counts.data_ptr(), wg_offsets.data_ptr(), n,
                                                     smax, V, H, W, float(conf_thres), int(thres_view), float(pix_base),
                                                     float(rel_base), stream)
        else:
            rc = lib.mvster_geo_scene_filter(depth.data_ptr(), conf.data_ptr(), p_pairs, p_ref, p_rm, p_vm,
                                             mask_sum[r0:r1].data_ptr(), avg[r0:r1].data_ptr(), photo[r0:r1].data_ptr(),
                                             geo[r0:r1].data_ptr(), final[r0:r1].data_ptr(), wg_counts.data_ptr(),
                                             wg_offsets.data_ptr(), n, smax, V, H, W, float(conf_thres), int(thres_view),
                                             float(pix_thres), float(rel_thres), stream)
        _lib.check(rc, "geo_scene_filter_dynamic" if dynamic else "geo_scene_filter")
        if marks:
            marks[1].record()
        bounds = wg_offsets[::nblk].cpu()                                   # the one host sync: M and the per-view counts
        M = int(bounds[-1])
        counts.append(bounds[1:] - bounds[:-1])
        points = torch.empty(M, 3, device=dev, dtype=torch.float32)
        colors = torch.empty(M, 3, device=dev, dtype=torch.uint8)
        if marks:
            marks[2].record()
        rc = lib.mvster_geo_scene_emit(avg[r0:r1].data_ptr(), final[r0:r1].data_ptr(), p_ref, p_rm, img.data_ptr(),
                                       0 if is_u8 else 1, wg_offsets.data_ptr(), points.data_ptr() if M else None,
                                       colors.data_ptr() if M else None, M, n, V, H, W, stream)
        _lib.check(rc, "geo_scene_emit")
        if marks:
            marks[3].record()
            events += [("filter+scan", marks[0], marks[1]), ("emit", marks[2], marks[3])]
        pts.append(points)
        cols.append(colors)
    res = SceneResult(points=pts[0] if len(pts) == 1 else torch.cat(pts), colors=cols[0] if len(cols) == 1 else torch.cat(cols),
                      counts=torch.cat(counts).to(dev), photo_mask=photo, geo_mask=geo, final_mask=final,
                      geo_mask_sum=mask_sum, depth_est_averaged=avg)
    if dynamic:
        res["geo_level"] = level
    if voxel_size is not None:
        res.update(("thin_" + k, t) for k, t in thin_points(res["points"], res["colors"], voxel_size, voxel_reduce).items())
    if outliers is not None or normals is not None:
        res.update(_clean_scene(res, Es, pairs, voxel_size is not None, outliers, normals))
    if mesh_spec is not None:
        res.update(mesh_mod.mesh_fused(res, img, Ks, Es, [r for r, _ in pairs], mesh_spec, clean=clean_spec, sparse=mesh.sparse))
    return res


def write_scene_ply(filename, res, thinned=False):
    """The cloud of a SceneResult as the scan-level entry points write it: the cleaned one (with its normals) where there is
    one, else the thinned one where ``thinned``, else ``points`` / ``colors``.  -> the vertex array written."""
    final = "final_points" in res
    vertices = res.vertices(thinned=thinned, final=final)
    write_ply(filename, vertices, res["final_normals"].cpu().numpy() if "final_normals" in res else None)
    return vertices


def filter_depth(pair_folder, scan_folder, out_folder, plyfilename, conf=0.9, thres_view=5, device="cuda:0",
                 filter_method="normal", pix_base=PIX_BASE, rel_base=REL_BASE, voxel_size=None, voxel_reduce="mean",
                 outliers=None, normals=None, mesh=None, meshfilename=None, mesh_clean=None):
    """The reference's ``filter_depth`` (test_mvs4.py:331-421; its ``args.conf`` / ``args.thres_view`` are keywords
    here): reads ``pair_folder/pair.txt``, ``scan_folder/cams/{:0>8}_cam.txt`` and ``images/{:0>8}.jpg``,
    ``out_folder/depth_est/{:0>8}.pfm`` and ``confidence/{:0>8}.pfm`` -- every file once --, fuses the scan on the GPU and
    writes ``out_folder/mask/{:0>8}_{photo,geo,final}.png`` (:390-393) and the point cloud ``plyfilename``.
    ``filter_method="dynamic"`` (with ``pix_base`` / ``rel_base``) writes the same files with the masks of dynamic
    consistency checking, see ``fuse_scene``.  With ``voxel_size`` the cloud written and returned is the voxel-thinned one
    (``thin_points`` with ``voxel_reduce``).  ``outliers`` / ``normals``: as ``fuse_scene``; the cloud written and returned is
    then the cleaned one, with nx ny nz in the file where normals were asked for.  ``mesh`` (a ``TSDFMesh``): as ``fuse_scene``;
    the triangle mesh is written to ``meshfilename`` (``mesh.write_mesh_ply``), which is required then and refused without
    ``mesh``.  ``mesh_clean`` (a ``MeshClean``, only with ``mesh``): as ``fuse_scene``; the mesh written is the cleaned one, with
    nx ny nz in the file where normals were asked for.  -> the vertex array."""
    _check_method("filter_depth", filter_method)
    _check_voxel("filter_depth", voxel_size, voxel_reduce)
    _check_clean("filter_depth", outliers, normals)
    mesh_mod.check_mesh_spec("filter_depth", mesh)
    mesh_mod.check_clean_spec("filter_depth", mesh_clean, mesh)
    if (mesh is None) != (meshfilename is None):
        raise RuntimeError("filter_depth: mesh and meshfilename go together (a TSDFMesh and the file its mesh is written to)")
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("filter_depth reads the scan's JPEGs and writes its mask PNGs with Pillow (PIL), which is "
                           "not installed; fuse_scene() on arrays needs no image library") from e
    pairs = formats.read_pair_file(os.path.join(pair_folder, "pair.txt"))
    views = sorted({v for r, srcs in pairs for v in [r] + srcs})
    slot = {v: i for i, v in enumerate(views)}
    name = "{:0>8}".format
    cams = [formats.read_camera_parameters(os.path.join(scan_folder, "cams", name(v) + "_cam.txt")) for v in views]
    depths = [np.asarray(formats.read_pfm(os.path.join(out_folder, "depth_est", name(v) + ".pfm"))[0], np.float32)
              for v in views]
    confs = [np.asarray(formats.read_pfm(os.path.join(out_folder, "confidence", name(v) + ".pfm"))[0], np.float32)
             for v in views]
    # 8-bit pixels as stored: (read_img's v / 255 * 255) truncated is v again, so the float image is never needed
    images = [np.array(Image.open(os.path.join(scan_folder, "images", name(v) + ".jpg")), dtype=np.uint8) for v in views]
    res = fuse_scene(depths, confs, images, [c[0] for c in cams], [c[1] for c in cams],
                     [(slot[r], [slot[v] for v in srcs]) for r, srcs in pairs], conf, thres_view, device=device,
                     method=filter_method, pix_base=pix_base, rel_base=rel_base, voxel_size=voxel_size,
                     voxel_reduce=voxel_reduce, outliers=outliers, normals=normals, mesh=mesh, mesh_clean=mesh_clean)
    if mesh is not None:
        mesh_mod.write_result_mesh(meshfilename, res)
    os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
    masks = {k: res[k + "_mask"].cpu().numpy() for k in ("photo", "geo", "final")}
    for i, (ref_view, _) in enumerate(pairs):
        for k, m in masks.items():                                          # save_mask: bool -> uint8 * 255
            Image.fromarray(m[i].astype(np.uint8) * 255).save(os.path.join(out_folder, "mask", name(ref_view) + "_%s.png" % k))
    return write_scene_ply(plyfilename, res, thinned=voxel_size is not None)
