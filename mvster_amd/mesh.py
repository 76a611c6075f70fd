"""Meshing a scan on the GPU: the filtered depth maps of a scan fused into a truncated signed distance
field (TSDF) on a dense grid, and the welded, indexed, coloured triangle mesh of its zero level by marching tetrahedra.

The definition is ``mvster_amd/csrc/tsdf_math.h``; the kernels are ``mvster_amd/csrc/geo_mesh.hip``.  ``integrate_tsdf`` is one
launch for all views of a scan, ``extract_mesh`` is count -> scan -> emit with one read-back (the two counts), no atomics: two
runs give the same bytes, and the bytes are those of the host build of the header (tests/test_gpu_mesh.py).  It is this
project's own definition, modelled on KinectFusion / Open3D-style integration: nearest-pixel sampling, the projective distance
along z, unit weights, a dense grid.  Open3D is not at hand, so agreement with it is untested.  There is no CPU fallback.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_NODES = (1 << 31) - 1               # tsdf::kMaxNodes: node and vertex numbers are int32
MAX_SIDE = 1 << 20                      # H, W at most
NODE_BYTES = 12 + 3                     # tsdf, weight, rgb, has_color of the volume + edge mask and rank of an extraction
MEMORY_BUDGET = 8 << 30                 # bytes a mesh_scene volume and its extraction may take
MIN_TRUNC_VOXELS = 2.0                  # trunc >= 2 voxels: the ends of a crossing edge (length <= sqrt(3) voxels) are not both clamped
DEFAULT_TRUNC_VOXELS = 4.0

MAX_AXIS = 1 << 20                      # tsdfs::kMaxAxis: nodes per axis of a sparse volume's virtual grid
MAX_BRICKS = 1 << 27                    # tsdfs::kMaxBricks: the brick directory is dense over the virtual grid
BRICK = 8
BRICK_NODES = BRICK ** 3
BRICK_BYTES = BRICK_NODES * NODE_BYTES + 12      # a brick's nodes with their extraction + its counts and offsets
DIRECTORY_BYTES = 5                     # per brick of the virtual grid: the directory word and the allocation's flag


class TSDFMesh(collections.namedtuple("TSDFMesh", "voxel_size trunc min_weight", defaults=(None, 2))):
    """The ``mesh=`` spec of the scan-level entry points.  ``sparse`` (default False) is a fourth field kept beside the tuple, so
    that ``TSDFMesh(0.01) == (0.01, None, 2)`` stays true: with ``sparse=True`` the scan is meshed in a ``SparseTSDFVolume``."""
    def __new__(cls, voxel_size, trunc=None, min_weight=2, sparse=False):
        self = super().__new__(cls, voxel_size, trunc, min_weight)
        self.sparse = sparse
        return self

    def __repr__(self):
        return "TSDFMesh(voxel_size=%r, trunc=%r, min_weight=%r, sparse=%r)" % (tuple(self) + (self.sparse,))

    def _replace(self, **kw):
        d = dict(zip(self._fields, self), sparse=self.sparse)
        d.update(kw)
        return TSDFMesh(**d)

    def __reduce__(self):
        return TSDFMesh, tuple(self) + (self.sparse,)


Mesh = collections.namedtuple("Mesh", "vertices colors triangles")
SparseMesh = collections.namedtuple("SparseMesh", "vertices colors triangles vertex_key")
# the ``mesh_clean=`` spec of the scan-level entry points (a keyword of its own: TSDFMesh(0.01) == (0.01, None, 2) is pinned)
MeshClean = collections.namedtuple("MeshClean", "weld min_triangles largest_only normals", defaults=(True, 0, False, False))

MAX_CLEAN_VERTICES = 1 << 29            # mesh::kMaxVertices: the weld table holds at most 2^30 slots, two per vertex
MAX_CLEAN_TRIANGLES = 1 << 29           # mesh::kMaxTriangles: 3 Nt corners are counted in 32 bits


class TSDFVolume:
    """What ``integrate_tsdf`` returns: ``tsdf`` [nz,ny,nx] float32, ``weight`` [nz,ny,nx] int32 (the views counted), ``rgb``
    [nz,ny,nx,3] uint8 and ``has_color`` [nz,ny,nx] uint8 on the GPU, and the grid: ``origin`` (3 floats), ``voxel_size``,
    ``dims`` = (nx, ny, nz), ``trunc``.  Node (i, j, k) is at origin + voxel_size * (i, j, k) and at [k, j, i] in the tensors."""

    def __init__(self, tsdf, weight, rgb, has_color, origin, voxel_size, dims, trunc):
        self.tsdf, self.weight, self.rgb, self.has_color = tsdf, weight, rgb, has_color
        self.origin, self.voxel_size, self.dims, self.trunc = tuple(float(o) for o in origin), float(voxel_size), tuple(dims), trunc

    def params(self):
        return dict(origin=self.origin, voxel_size=self.voxel_size, dims=self.dims, trunc=self.trunc)


# ---- argument checks (all on the host, before any device call) ----------------------------------------------------------------------

def _number(what, name, value, positive=True):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise RuntimeError("%s: %s must be a number, not %r" % (what, name, value)) from None
    if not math.isfinite(v) or (positive and not v > 0):
        raise RuntimeError("%s: %s must be finite%s, not %r" % (what, name, " and > 0" if positive else "", value))
    return v


def _check_trunc(what, voxel, trunc):
    """-> trunc, ``DEFAULT_TRUNC_VOXELS`` voxels where it is None; refused below ``MIN_TRUNC_VOXELS`` voxels."""
    if trunc is None:
        return DEFAULT_TRUNC_VOXELS * voxel
    t = _number(what, "trunc", trunc)
    if t < MIN_TRUNC_VOXELS * voxel:
        raise RuntimeError("%s: trunc must be >= %g * voxel_size = %r, not %r (both ends of a crossing edge could be clamped)" %
                           (what, MIN_TRUNC_VOXELS, MIN_TRUNC_VOXELS * voxel, trunc))
    return t


def _check_min_weight(what, min_weight):
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, np.integer)) or not 1 <= int(min_weight) < (1 << 31):
        raise RuntimeError("%s: min_weight must be an integer >= 1, not %r" % (what, min_weight))
    return int(min_weight)


def _check_dims(what, dims):
    try:
        d = tuple(int(x) for x in dims)
        exact = all(int(x) == x for x in dims)
    except (TypeError, ValueError):
        raise RuntimeError("%s: dims must be three integers (nx, ny, nz), not %r" % (what, dims)) from None
    if len(d) != 3 or not exact:
        raise RuntimeError("%s: dims must be three integers (nx, ny, nz), not %r" % (what, dims))
    if min(d) < 2:
        raise RuntimeError("%s: a grid needs at least 2 nodes per axis, not %r" % (what, d))
    if d[0] * d[1] * d[2] > MAX_NODES:
        raise RuntimeError("%s: a grid holds at most 2^31 - 1 nodes, not %d (%r)" % (what, d[0] * d[1] * d[2], d))
    return d


def _check_origin(what, origin):
    try:
        o = tuple(float(x) for x in origin)
    except (TypeError, ValueError):
        raise RuntimeError("%s: origin must be three numbers, not %r" % (what, origin)) from None
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise RuntimeError("%s: origin must be three finite numbers, not %r" % (what, origin))
    return o


def check_mesh_spec(what, mesh):
    """The ``mesh`` keyword of the scan-level entry points, checked before anything runs -> (voxel, trunc, min_weight) or None."""
    if mesh is None:
        return None
    if not isinstance(mesh, TSDFMesh):
        raise RuntimeError("%s: mesh must be None or a TSDFMesh, not %r" % (what, mesh))
    voxel = _number(what, "mesh.voxel_size", mesh.voxel_size)
    _flag(what, "mesh.sparse", mesh.sparse)
    return voxel, _check_trunc(what, voxel, mesh.trunc), _check_min_weight(what, mesh.min_weight)


def _shape(x):
    if isinstance(x, (torch.Tensor, np.ndarray)):
        return tuple(x.shape)
    x = list(x)
    shapes = {tuple(m.shape) for m in x}
    if len(shapes) != 1:
        raise RuntimeError("maps of different sizes inside one scan: %s" % sorted(shapes))
    return (len(x),) + shapes.pop()


def _stack(x, dev, dtype):
    """Maps of a scan (array, tensor, or a sequence of either) -> one contiguous tensor [V, ...] of ``dtype`` on ``dev``."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        x = list(x)
        if all(isinstance(m, torch.Tensor) for m in x):
            x = torch.stack([m.to(dev) for m in x])
        else:
            x = np.stack([m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in x])
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(dev, dtype).contiguous()


def _cameras(what, Ks, Es, V):
    """-> views [V,21] float64: K (row major), R, t.  K's third row must be 0 0 1 (the kernels do not read it)."""
    def host(a):
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    Ks, Es = [host(k) for k in Ks], [host(e) for e in Es]
    if len(Ks) != V or len(Es) != V:
        raise RuntimeError("%s: %d depth maps for %d intrinsics and %d extrinsics" % (what, V, len(Ks), len(Es)))
    rows = np.empty((V, 21), np.float64)
    for v, (K, E) in enumerate(zip(Ks, Es)):
        if K.shape != (3, 3) or E.shape != (4, 4):
            raise RuntimeError("%s: Ks[%d] must be [3,3] and Es[%d] [4,4], not %s and %s" % (what, v, v, K.shape, E.shape))
        if not (np.isfinite(K).all() and np.isfinite(E).all()):
            raise RuntimeError("%s: the camera of view %d holds a value that is not finite" % (what, v))
        if tuple(K[2]) != (0.0, 0.0, 1.0):
            raise RuntimeError("%s: the third row of Ks[%d] must be 0 0 1, not %r" % (what, v, tuple(K[2])))
        rows[v, :9], rows[v, 9:18], rows[v, 18:] = K.reshape(-1), E[:3, :3].reshape(-1), E[:3, 3]
    return rows


def _device(what, device, tensors):
    if device is None:
        devs = [m.device for x in tensors for m in ([x] if isinstance(x, torch.Tensor) else
                                                    x if not isinstance(x, np.ndarray) and x is not None else [])
                if isinstance(m, torch.Tensor) and m.is_cuda]
        if not devs:
            raise RuntimeError("mvster_amd.mesh.%s runs on MI355X only: pass device= or tensors on the GPU (there is no CPU "
                               "fallback)" % what)
        device = devs[0]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("mvster_amd.mesh.%s runs on MI355X only (there is no CPU fallback)" % what)
    return dev


def _check_maps(what, depths, masks, images):
    ds = _shape(depths)
    if len(ds) != 3 or ds[0] < 1 or ds[1] < 1 or ds[2] < 1 or max(ds[1:]) > MAX_SIDE:
        raise RuntimeError("%s: depths must be [V,H,W] with V, H, W >= 1 and H, W <= 2^20, not %s" % (what, ds))
    if masks is not None and _shape(masks) != ds:
        raise RuntimeError("%s: masks must have the shape of depths %s, not %s" % (what, ds, _shape(masks)))
    if _shape(images) != ds + (3,):
        raise RuntimeError("%s: images must be [V,H,W,3] with the V, H, W of depths %s, not %s" % (what, ds, _shape(images)))
    first = images if isinstance(images, (torch.Tensor, np.ndarray)) else list(images)[0]
    if first.dtype not in (torch.uint8, np.dtype(np.uint8)):
        raise RuntimeError("%s: images must be uint8, not %s" % (what, first.dtype))
    return ds


# ---- integration ------------------------------------------------------------------------------------------------------------------------

def integrate_tsdf(depths, masks, images, Ks, Es, origin, voxel_size, dims, trunc, device=None, fill=None):
    """All views of a scan fused into a TSDF on the GPU in one launch (``mvster_tsdf_integrate``).  ``depths`` [V,H,W]
    (converted to float32), ``masks`` [V,H,W] (a pixel is used where its mask is not 0; None: every pixel), ``images``
    [V,H,W,3] uint8, ``Ks`` [V,3,3] (third row 0 0 1) and ``Es`` [V,4,4] world -> camera, widened to float64: arrays,
    tensors or sequences of them.  The grid has ``dims`` = (nx, ny, nz) nodes (each >= 2, at most 2^31 - 1 in all), node
    (i, j, k) at ``origin`` + ``voxel_size`` (i, j, k) in float64.  Per node and view: the nearest pixel of the node's
    projection; depth d there (skipped where masked, not finite or <= 0); sdf = d - z of the node in the camera; skipped
    where sdf < -``trunc``; f = min(1, sdf / trunc).  -> ``TSDFVolume``: tsdf = the mean of f over the views counted (1 where
    none), weight = their number, rgb = the rounded mean of the pixels with sdf <= trunc.  Every view has weight 1
    (per-pixel confidence weights are out of scope).  Nothing is read back.  ``fill`` (tests): a byte the outputs are filled with
    before the kernel writes them.  No CPU fallback."""
    what = "integrate_tsdf"
    V, H, W = _check_maps(what, depths, masks, images)
    views = _cameras(what, Ks, Es, V)
    o = _check_origin(what, origin)
    voxel = _number(what, "voxel_size", voxel_size)
    nx, ny, nz = _check_dims(what, dims)
    t = _number(what, "trunc", trunc)
    dev = _device(what, device, (depths, masks, images))
    depth = _stack(depths, dev, torch.float32)
    mask = torch.ones(V, H, W, device=dev, dtype=torch.uint8) if masks is None else (_stack(masks, dev, torch.bool)).to(torch.uint8)
    img = _stack(images, dev, torch.uint8)
    vol = TSDFVolume(torch.empty(nz, ny, nx, device=dev, dtype=torch.float32), torch.empty(nz, ny, nx, device=dev, dtype=torch.int32),
                     torch.empty(nz, ny, nx, 3, device=dev, dtype=torch.uint8), torch.empty(nz, ny, nx, device=dev, dtype=torch.uint8),
                     o, voxel, (nx, ny, nz), t)
    if fill is not None:
        for out in (vol.tsdf, vol.weight, vol.rgb, vol.has_color):
            out.view(torch.uint8).fill_(int(fill))
    with torch.cuda.device(dev):
        table = torch.from_numpy(views).to(dev)
        rc = _lib.load().mvster_tsdf_integrate(depth.data_ptr(), mask.data_ptr(), img.data_ptr(), table.data_ptr(), V, H, W, o[0], o[1],
                                               o[2], voxel, nx, ny, nz, t, vol.tsdf.data_ptr(), vol.weight.data_ptr(),
                                               vol.rgb.data_ptr(), vol.has_color.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "tsdf_integrate")
    return vol


# ---- extraction --------------------------------------------------------------------------------------------------------------------------

def _check_volume(what, volume):
    if not isinstance(volume, TSDFVolume):
        raise RuntimeError("%s: volume must be a TSDFVolume, not %s" % (what, type(volume).__name__))
    nx, ny, nz = _check_dims(what, volume.dims)
    _check_origin(what, volume.origin)
    _number(what, "volume.voxel_size", volume.voxel_size)
    for name, shape, dtype in (("tsdf", (nz, ny, nx), torch.float32), ("weight", (nz, ny, nx), torch.int32),
                               ("rgb", (nz, ny, nx, 3), torch.uint8), ("has_color", (nz, ny, nx), torch.uint8)):
        t = getattr(volume, name)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype:
            raise RuntimeError("%s: volume.%s must be a %s tensor of shape %s" % (what, name, dtype, shape))
    for name in ("tsdf", "weight", "rgb", "has_color"):
        t = getattr(volume, name)
        if not t.is_cuda or t.device != volume.tsdf.device:
            raise RuntimeError("%s: volume.%s must be on the GPU of volume.tsdf (there is no CPU fallback)" % (what, name))
    return nx, ny, nz


def extract_mesh(volume, min_weight=1, fill=None):
    """The zero level of a ``TSDFVolume`` as a welded, indexed, coloured triangle mesh by marching tetrahedra on the GPU
    (``mvster_mesh_count`` / ``mvster_mesh_emit_vertices`` / ``mvster_mesh_emit_triangles``; defined exactly in
    mvster_amd/csrc/tsdf_math.h).  A node is known where weight >= ``min_weight`` and inside where tsdf < 0; a cell takes part
    where its 8 corners are known.  -> ``Mesh``: ``vertices`` [Nv,3] float32, ``colors`` [Nv,3] uint8, ``triangles`` [Nt,3]
    int32, on the GPU; vertices in the order of their owner node and edge, triangles in the order cell, tetrahedron, triangle,
    counter-clockwise seen from the free-space (tsdf > 0) side; every vertex is used, none appears twice.  A node with
    tsdf == 0 is outside, so a vertex may coincide with a node and triangles without area are kept.  Nv = Nt = 0 is a valid
    result.  One read-back (the two counts).  ``fill`` (tests): a byte the outputs are filled with before the kernels write
    them.  No CPU fallback."""
    what = "extract_mesh"
    mw = _check_min_weight(what, min_weight)
    nx, ny, nz = _check_volume(what, volume)
    dev = volume.tsdf.device
    tsdf, weight, rgb, has = (getattr(volume, k).contiguous() for k in ("tsdf", "weight", "rgb", "has_color"))
    lib = _lib.load()
    nodes = nx * ny * nz
    tiles = lib.mvster_mesh_blocks(nodes)
    _lib.check(min(tiles, 0), "mesh_blocks")
    o, voxel = volume.origin, volume.voxel_size
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        edge_mask = torch.empty(nodes, device=dev, dtype=torch.uint8)
        rank = torch.empty(nodes, device=dev, dtype=torch.int16)
        counts = torch.empty(2, tiles, device=dev, dtype=torch.int32)
        offsets = torch.empty(2, tiles + 1, device=dev, dtype=torch.int64)
        _lib.check(lib.mvster_mesh_count(tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, mw, edge_mask.data_ptr(), rank.data_ptr(),
                                         counts[0].data_ptr(), counts[1].data_ptr(), offsets[0].data_ptr(), offsets[1].data_ptr(),
                                         stream), "mesh_count")
        nv, nt = (int(c) for c in offsets[:, tiles].cpu())                        # the one read-back
        if nv > MAX_NODES:
            raise RuntimeError("extract_mesh: the mesh would have %d vertices; triangles hold int32 vertex numbers (at most "
                               "2^31 - 1)" % nv)
        vertices = torch.empty(nv, 3, device=dev, dtype=torch.float32)
        colors = torch.empty(nv, 3, device=dev, dtype=torch.uint8)
        triangles = torch.empty(nt, 3, device=dev, dtype=torch.int32)
        if fill is not None:
            for t in (vertices, colors, triangles):
                t.view(torch.uint8).fill_(int(fill))
        _lib.check(lib.mvster_mesh_emit_vertices(tsdf.data_ptr(), rgb.data_ptr(), has.data_ptr(), o[0], o[1], o[2], voxel, nx, ny, nz,
                                                 edge_mask.data_ptr(), rank.data_ptr(), offsets[0].data_ptr(), nv,
                                                 vertices.data_ptr() if nv else None, colors.data_ptr() if nv else None, stream),
                   "mesh_emit_vertices")
        _lib.check(lib.mvster_mesh_emit_triangles(tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, mw, edge_mask.data_ptr(),
                                                  rank.data_ptr(), offsets[0].data_ptr(), offsets[1].data_ptr(), nv, nt,
                                                  triangles.data_ptr() if nt else None, stream), "mesh_emit_triangles")
    return Mesh(vertices, colors, triangles)


# ---- brick-sparse volumes (defined exactly in mvster_amd/csrc/tsdf_sparse_math.h) -------------------------------

class SparseTSDFVolume:
    """A TSDF stored in 8 x 8 x 8 bricks: the grid (``origin``, ``voxel_size``, ``dims`` = (nx, ny, nz), each axis at most 2^20 and
    no limit on the product, ``trunc``), the directory ``brick_slot`` [nbz,nby,nbx] int32 (a brick's place in ``bricks``, -1 =
    absent), ``bricks`` [Nb] int32 (ascending brick numbers bi + nbx (bj + nby bk)) and brick-major ``tsdf`` / ``weight`` /
    ``has_color`` [Nb,512] and ``rgb`` [Nb,512,3], a node's place in its brick being li + 8 (lj + 8 lk).  It means the dense
    ``TSDFVolume`` of the same grid with every node of an absent brick at weight 0, tsdf 1 (``densify``)."""

    def __init__(self, brick_slot, bricks, tsdf, weight, rgb, has_color, origin, voxel_size, dims, trunc):
        self.brick_slot, self.bricks = brick_slot, bricks
        self.tsdf, self.weight, self.rgb, self.has_color = tsdf, weight, rgb, has_color
        self.origin, self.voxel_size, self.dims, self.trunc = tuple(float(o) for o in origin), float(voxel_size), tuple(dims), trunc

    @property
    def n_bricks(self):
        return int(self.bricks.shape[0])

    def params(self):
        return dict(origin=self.origin, voxel_size=self.voxel_size, dims=self.dims, trunc=self.trunc, sparse=True,
                    bricks=self.n_bricks, grid_bricks=int(self.brick_slot.numel()))


def brick_dims(dims):
    """-> (nbx, nby, nbz), the bricks per axis of a grid of ``dims`` nodes"""
    return tuple((int(n) + BRICK - 1) // BRICK for n in dims)


def _check_sparse_dims(what, dims):
    try:
        d = tuple(int(x) for x in dims)
        exact = all(int(x) == x for x in dims)
    except (TypeError, ValueError):
        raise RuntimeError("%s: dims must be three integers (nx, ny, nz), not %r" % (what, dims)) from None
    if len(d) != 3 or not exact:
        raise RuntimeError("%s: dims must be three integers (nx, ny, nz), not %r" % (what, dims))
    if min(d) < 2 or max(d) > MAX_AXIS:
        raise RuntimeError("%s: a sparse grid needs 2 .. 2^20 nodes per axis, not %r" % (what, d))
    nb = brick_dims(d)
    if nb[0] * nb[1] * nb[2] > MAX_BRICKS:
        raise RuntimeError("%s: a sparse grid holds at most 2^27 bricks of 8 x 8 x 8 nodes (its directory is dense), not %d (%r nodes)" %
                           (what, nb[0] * nb[1] * nb[2], d))
    return d, nb


def _check_allocation_cameras(what, views, origin, voxel, dims):
    """What the covering property of ``allocate`` assumes of the cameras (tsdf_sparse_math.h): K upper triangular with a
    diagonal that is not 0, and R orthonormal closely enough that R^T (R x) stays within a quarter of a voxel of every node x."""
    reach = max(max(abs(o), abs(o + voxel * (n - 1))) for o, n in zip(origin, dims))
    for v, row in enumerate(views):
        K, R = row[:9].reshape(3, 3), row[9:18].reshape(3, 3)
        if K[1, 0] != 0.0 or K[0, 0] == 0.0 or K[1, 1] == 0.0:
            raise RuntimeError("%s: Ks[%d] must be upper triangular with K_00 and K_11 not 0 (the allocation inverts it in closed "
                               "form), not %r" % (what, v, K.tolist()))
        err = float(np.abs(R.T @ R - np.eye(3)).max())
        if 3.0 * err * reach > 0.25 * voxel:
            raise RuntimeError("%s: the rotation of view %d is orthonormal only to %.3g; at a distance of %g from the world's origin "
                               "that moves a node by more than a quarter of the voxel %g, and the allocation could miss a brick" %
                               (what, v, err, reach, voxel))


def _mask_bytes(masks, V, H, W, dev):
    return torch.ones(V, H, W, device=dev, dtype=torch.uint8) if masks is None else _stack(masks, dev, torch.bool).to(torch.uint8)


def _allocate(what, depth, mask, views, o, voxel, dims, nb, t, dev):
    """-> brick_slot [nbz,nby,nbx] int32 and bricks [Nb] int32 on ``dev`` (one read-back: Nb)"""
    lib = _lib.load()
    V, H, W = depth.shape
    nbricks = nb[0] * nb[1] * nb[2]
    tiles = (nbricks + BRICK_NODES - 1) // BRICK_NODES
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        table = torch.from_numpy(views).to(dev)
        flags = torch.empty(nbricks, device=dev, dtype=torch.uint8)
        counts = torch.empty(tiles, device=dev, dtype=torch.int32)
        offsets = torch.empty(tiles + 1, device=dev, dtype=torch.int64)
        _lib.check(lib.mvster_tsdf_sparse_mark(depth.data_ptr(), mask.data_ptr(), table.data_ptr(), V, H, W, o[0], o[1], o[2], voxel,
                                               dims[0], dims[1], dims[2], t, flags.data_ptr(), stream), "tsdf_sparse_mark")
        _lib.check(lib.mvster_tsdf_sparse_compact_count(flags.data_ptr(), nbricks, counts.data_ptr(), offsets.data_ptr(), stream),
                   "tsdf_sparse_compact_count")
        n = int(offsets[tiles].cpu())                                             # the one read-back
        slot = torch.empty(nb[2], nb[1], nb[0], device=dev, dtype=torch.int32)
        bricks = torch.empty(n, device=dev, dtype=torch.int32)
        _lib.check(lib.mvster_tsdf_sparse_compact_emit(flags.data_ptr(), nbricks, offsets.data_ptr(), n, slot.data_ptr(),
                                                       bricks.data_ptr() if n else None, stream), "tsdf_sparse_compact_emit")
    return slot, bricks


def allocate_bricks(depths, masks, Ks, Es, origin, voxel_size, dims, trunc, device=None):
    """The bricks of a sparse volume that the maps of a scan need, on the GPU (``mvster_tsdf_sparse_mark`` and the two compaction
    calls): every pixel with mask != 0 and a finite depth d > 0 allocates the bricks its slab touches -- its frustum between camera
    z = max(d - trunc, 0) and d + trunc, back-projected, as a box in node coordinates widened by 2 nodes.  Every node some view
    counts within +-trunc then lies with its 26 neighbours in allocated bricks (proved in tsdf_sparse_math.h), so the sparse mesh
    is the dense one.  K must be upper triangular.  -> (``brick_slot`` [nbz,nby,nbx] int32, ``bricks`` [Nb] int32 ascending).  One
    read-back (Nb).  No CPU fallback."""
    what = "allocate_bricks"
    ds = _shape(depths)
    if len(ds) != 3 or min(ds) < 1 or max(ds[1:]) > MAX_SIDE:
        raise RuntimeError("%s: depths must be [V,H,W] with V, H, W >= 1 and H, W <= 2^20, not %s" % (what, ds))
    if masks is not None and _shape(masks) != ds:
        raise RuntimeError("%s: masks must have the shape of depths %s, not %s" % (what, ds, _shape(masks)))
    V, H, W = ds
    views = _cameras(what, Ks, Es, V)
    o = _check_origin(what, origin)
    voxel = _number(what, "voxel_size", voxel_size)
    d, nb = _check_sparse_dims(what, dims)
    t = _number(what, "trunc", trunc)
    _check_allocation_cameras(what, views, o, voxel, d)
    dev = _device(what, device, (depths, masks))
    return _allocate(what, _stack(depths, dev, torch.float32), _mask_bytes(masks, V, H, W, dev), views, o, voxel, d, nb, t, dev)


def _check_bricks(what, bricks, nbricks, dev):
    """A caller's own brick list: integers, ascending without duplicates, in 0 .. nbricks - 1 -> int32 tensor on ``dev``"""
    b = bricks.detach().cpu().numpy() if isinstance(bricks, torch.Tensor) else np.asarray(bricks)
    if b.ndim != 1 or (b.size and b.dtype.kind not in "iu"):
        raise RuntimeError("%s: bricks must be a 1-d array of integer brick numbers, not %s %s" % (what, b.shape, b.dtype))
    b = b.astype(np.int64)
    if b.size and (b.min() < 0 or b.max() >= nbricks):
        raise RuntimeError("%s: bricks must lie in 0 .. %d, not %d" % (what, nbricks - 1, b.min() if b.min() < 0 else b.max()))
    if b.size > 1 and not (np.diff(b) > 0).all():
        raise RuntimeError("%s: bricks must be ascending and without duplicates" % what)
    return torch.from_numpy(b.astype(np.int32)).to(dev)


def sparse_bytes(n_bricks, grid_bricks):
    """The bytes a sparse volume of ``n_bricks`` bricks and its extraction take in a virtual grid of ``grid_bricks`` bricks"""
    return int(n_bricks) * BRICK_BYTES + int(grid_bricks) * DIRECTORY_BYTES


def integrate_tsdf_sparse(depths, masks, images, Ks, Es, origin, voxel_size, dims, trunc, bricks=None, device=None, fill=None,
                          memory_budget=None):
    """``integrate_tsdf`` into a ``SparseTSDFVolume`` (``mvster_tsdf_sparse_integrate``: one launch for all views, one workgroup
    per brick, the same ``tsdf::add_view``): the nodes of allocated bricks carry exactly what ``integrate_tsdf`` gives them.
    ``dims``: each axis 2 .. 2^20, at most 2^27 bricks in all, no limit on the nodes.  ``bricks`` (None: ``allocate_bricks`` of the
    same maps): the caller's own set of brick numbers, ascending, without duplicates, in range.  ``memory_budget`` (None: not
    checked): refused where the allocated bricks with their extraction take more bytes, after the allocation's read-back.
    ``fill`` (tests): a byte the outputs are filled with before the kernel writes them.  No CPU fallback."""
    what = "integrate_tsdf_sparse"
    V, H, W = _check_maps(what, depths, masks, images)
    views = _cameras(what, Ks, Es, V)
    o = _check_origin(what, origin)
    voxel = _number(what, "voxel_size", voxel_size)
    d, nb = _check_sparse_dims(what, dims)
    t = _number(what, "trunc", trunc)
    budget = None if memory_budget is None else _number(what, "memory_budget", memory_budget)
    nbricks = nb[0] * nb[1] * nb[2]
    if bricks is None:
        _check_allocation_cameras(what, views, o, voxel, d)
    dev = _device(what, device, (depths, masks, images))
    if bricks is not None:
        bricks = _check_bricks(what, bricks, nbricks, dev)
    depth = _stack(depths, dev, torch.float32)
    mask = _mask_bytes(masks, V, H, W, dev)
    img = _stack(images, dev, torch.uint8)
    if bricks is None:
        slot, bricks = _allocate(what, depth, mask, views, o, voxel, d, nb, t, dev)
    else:
        slot = torch.full((nbricks,), -1, device=dev, dtype=torch.int32)
        slot[bricks.long()] = torch.arange(len(bricks), device=dev, dtype=torch.int32)
        slot = slot.view(nb[2], nb[1], nb[0])
    n = int(bricks.shape[0])
    if budget is not None and sparse_bytes(n, nbricks) > budget:
        # the bricks follow a surface: their number falls with the square of the voxel size (the directory's with the cube)
        fit = voxel * 1.05 * math.sqrt(sparse_bytes(n, nbricks) / budget)
        raise RuntimeError("%s: the volume would hold %d bricks of 8 x 8 x 8 nodes (of %d in the grid) = %d bytes with its extraction, "
                           "above the memory_budget of %d bytes; a voxel_size of about %g would fit" %
                           (what, n, nbricks, sparse_bytes(n, nbricks), int(budget), fit))
    vol = SparseTSDFVolume(slot, bricks, torch.empty(n, BRICK_NODES, device=dev, dtype=torch.float32),
                           torch.empty(n, BRICK_NODES, device=dev, dtype=torch.int32),
                           torch.empty(n, BRICK_NODES, 3, device=dev, dtype=torch.uint8),
                           torch.empty(n, BRICK_NODES, device=dev, dtype=torch.uint8), o, voxel, d, t)
    if fill is not None:
        for out in (vol.tsdf, vol.weight, vol.rgb, vol.has_color):
            out.view(torch.uint8).fill_(int(fill))
    if n:
        with torch.cuda.device(dev):
            table = torch.from_numpy(views).to(dev)
            rc = _lib.load().mvster_tsdf_sparse_integrate(depth.data_ptr(), mask.data_ptr(), img.data_ptr(), table.data_ptr(), V, H, W,
                                                          o[0], o[1], o[2], voxel, d[0], d[1], d[2], t, bricks.data_ptr(), n,
                                                          vol.tsdf.data_ptr(), vol.weight.data_ptr(), vol.rgb.data_ptr(),
                                                          vol.has_color.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(rc, "tsdf_sparse_integrate")
    return vol


def _check_sparse_volume(what, volume):
    if not isinstance(volume, SparseTSDFVolume):
        raise RuntimeError("%s: volume must be a SparseTSDFVolume, not %s" % (what, type(volume).__name__))
    d, nb = _check_sparse_dims(what, volume.dims)
    _check_origin(what, volume.origin)
    _number(what, "volume.voxel_size", volume.voxel_size)
    if not isinstance(volume.bricks, torch.Tensor) or volume.bricks.dim() != 1 or volume.bricks.dtype != torch.int32:
        raise RuntimeError("%s: volume.bricks must be an int32 tensor [Nb]" % what)
    n = volume.bricks.shape[0]
    if n > nb[0] * nb[1] * nb[2]:
        raise RuntimeError("%s: volume.bricks holds %d bricks, the grid %d" % (what, n, nb[0] * nb[1] * nb[2]))
    for name, shape, dtype in (("brick_slot", (nb[2], nb[1], nb[0]), torch.int32), ("tsdf", (n, BRICK_NODES), torch.float32),
                               ("weight", (n, BRICK_NODES), torch.int32), ("rgb", (n, BRICK_NODES, 3), torch.uint8),
                               ("has_color", (n, BRICK_NODES), torch.uint8)):
        t = getattr(volume, name)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype:
            raise RuntimeError("%s: volume.%s must be a %s tensor of shape %s" % (what, name, dtype, shape))
    for name in ("brick_slot", "bricks", "tsdf", "weight", "rgb", "has_color"):
        t = getattr(volume, name)
        if not t.is_cuda or t.device != volume.tsdf.device:
            raise RuntimeError("%s: volume.%s must be on the GPU of volume.tsdf (there is no CPU fallback)" % (what, name))
    return d, nb, n


def extract_mesh_sparse(volume, min_weight=1, keys=False, fill=None):
    """``extract_mesh`` of a ``SparseTSDFVolume`` on the GPU (``mvster_mesh_sparse_count`` / ``_emit_vertices`` /
    ``_emit_triangles``): the dense extraction of the volume it means, a brick at a time on a 10 x 10 x 10 window staged in LDS.
    -> ``Mesh``, or with ``keys`` a ``SparseMesh`` whose ``vertex_key`` [Nv] int64 = global owner node * 8 + d names every vertex
    whatever the order.  Vertices are in the order (brick, node in the brick, d), triangles in (brick, cell, tetrahedron,
    triangle): the same vertices and triangles as ``extract_mesh`` on ``densify(volume)``, in another order.  One read-back (the
    two counts).  ``fill`` (tests): a byte the outputs are filled with before the kernels write them.  No CPU fallback."""
    what = "extract_mesh_sparse"
    mw = _check_min_weight(what, min_weight)
    keys = _flag(what, "keys", keys)
    (nx, ny, nz), nb, n = _check_sparse_volume(what, volume)
    dev = volume.tsdf.device
    tsdf, weight, rgb, has, slot, bricks = (getattr(volume, k).contiguous() for k in ("tsdf", "weight", "rgb", "has_color", "brick_slot",
                                                                                     "bricks"))
    nv = nt = 0
    o, voxel = volume.origin, volume.voxel_size
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if n:
            edge_mask = torch.empty(n * BRICK_NODES, device=dev, dtype=torch.uint8)
            rank = torch.empty(n * BRICK_NODES, device=dev, dtype=torch.int16)
            counts = torch.empty(2, n, device=dev, dtype=torch.int32)
            offsets = torch.empty(2, n + 1, device=dev, dtype=torch.int64)
            _lib.check(lib.mvster_mesh_sparse_count(tsdf.data_ptr(), weight.data_ptr(), slot.data_ptr(), bricks.data_ptr(), n, nx, ny, nz,
                                                    mw, edge_mask.data_ptr(), rank.data_ptr(), counts[0].data_ptr(),
                                                    counts[1].data_ptr(), offsets[0].data_ptr(), offsets[1].data_ptr(), stream),
                       "mesh_sparse_count")
            nv, nt = (int(c) for c in offsets[:, n].cpu())                        # the one read-back
            if nv > MAX_NODES:
                raise RuntimeError("extract_mesh_sparse: the mesh would have %d vertices; triangles hold int32 vertex numbers (at most "
                                   "2^31 - 1)" % nv)
        vertices = torch.empty(nv, 3, device=dev, dtype=torch.float32)
        colors = torch.empty(nv, 3, device=dev, dtype=torch.uint8)
        triangles = torch.empty(nt, 3, device=dev, dtype=torch.int32)
        vkeys = torch.empty(nv, device=dev, dtype=torch.int64) if keys else None
        if fill is not None:
            for t in (vertices, colors, triangles) + ((vkeys,) if keys else ()):
                t.view(torch.uint8).fill_(int(fill))
        if nv:
            _lib.check(lib.mvster_mesh_sparse_emit_vertices(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), has.data_ptr(),
                                                            slot.data_ptr(), bricks.data_ptr(), n, o[0], o[1], o[2], voxel, nx, ny, nz,
                                                            edge_mask.data_ptr(), rank.data_ptr(), offsets[0].data_ptr(), nv,
                                                            vertices.data_ptr(), colors.data_ptr(), vkeys.data_ptr() if keys else None,
                                                            stream), "mesh_sparse_emit_vertices")
        if nt:
            _lib.check(lib.mvster_mesh_sparse_emit_triangles(tsdf.data_ptr(), weight.data_ptr(), slot.data_ptr(), bricks.data_ptr(), n,
                                                             nx, ny, nz, mw, edge_mask.data_ptr(), rank.data_ptr(),
                                                             offsets[0].data_ptr(), offsets[1].data_ptr(), nv, nt, triangles.data_ptr(),
                                                             stream), "mesh_sparse_emit_triangles")
    return SparseMesh(vertices, colors, triangles, vkeys) if keys else Mesh(vertices, colors, triangles)


def densify(volume):
    """The dense ``TSDFVolume`` a ``SparseTSDFVolume`` means (plain torch scatter; for tests and small grids): nodes of absent
    bricks get weight 0, tsdf 1, rgb 0, has_color 0.  Refused above the dense limits."""
    what = "densify"
    (nx, ny, nz), nb, n = _check_sparse_volume(what, volume)
    _check_dims(what, (nx, ny, nz))
    dev = volume.tsdf.device
    px, py, pz = (b * BRICK for b in nb)                                          # the grid padded to whole bricks
    full = dict(tsdf=torch.ones(pz, py, px, device=dev, dtype=torch.float32), weight=torch.zeros(pz, py, px, device=dev, dtype=torch.int32),
                rgb=torch.zeros(pz, py, px, 3, device=dev, dtype=torch.uint8), has_color=torch.zeros(pz, py, px, device=dev, dtype=torch.uint8))
    b = volume.bricks.long()
    bi, bj, bk = b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])
    l = torch.arange(BRICK, device=dev)
    k = (bk[:, None] * BRICK + l)[:, :, None, None]
    j = (bj[:, None] * BRICK + l)[:, None, :, None]
    i = (bi[:, None] * BRICK + l)[:, None, None, :]
    for name, t in full.items():
        src = getattr(volume, name)
        t[k, j, i] = src.view((n, BRICK, BRICK, BRICK) + tuple(src.shape[2:]))
    return TSDFVolume(*(full[name][:nz, :ny, :nx].contiguous() for name in ("tsdf", "weight", "rgb", "has_color")), volume.origin,
                      volume.voxel_size, (nx, ny, nz), volume.trunc)


# ---- a scan's maps to a mesh ------------------------------------------------------------------------------------------------------------

def grid_for_bounds(what, lo, hi, voxel, trunc, memory_budget=MEMORY_BUDGET, sparse=False):
    """The grid of ``mesh_scene``: the box (lo, hi) padded by ``trunc`` on every side, origin at its low corner, as many nodes
    per axis as cover it (at least 2) -> (origin, dims).  Refused where the volume and its extraction (``NODE_BYTES`` a node)
    would take more than ``memory_budget`` bytes or more than 2^31 - 1 nodes; the message names the voxel size that fits.
    ``sparse``: the virtual grid of a ``SparseTSDFVolume``: the node cap does not apply; refused above 2^20 nodes per axis, 2^27
    bricks, or where the brick directory alone is above the budget (the bricks are checked once they are allocated)."""
    lo, hi = _check_origin(what, lo), _check_origin(what, hi)
    if any(h < l for l, h in zip(lo, hi)):
        raise RuntimeError("%s: bounds must be (lo, hi) with lo <= hi on every axis, not %r, %r" % (what, lo, hi))
    budget = _number(what, "memory_budget", memory_budget)
    origin = tuple(l - trunc for l in lo)
    ext = [(h + trunc) - o for h, o in zip(hi, origin)]
    dims = tuple(max(2, int(math.ceil(e / voxel)) + 1) for e in ext)
    if sparse:
        nb = brick_dims(dims)
        grid_bricks = nb[0] * nb[1] * nb[2]
        if max(dims) > MAX_AXIS or grid_bricks > MAX_BRICKS or grid_bricks * DIRECTORY_BYTES > budget:
            raise RuntimeError("%s: the sparse grid would hold %d x %d x %d nodes in %d bricks (a directory of %d bytes), above 2^20 "
                               "nodes per axis, 2^27 bricks or the memory_budget of %d bytes" %
                               (what, dims[0], dims[1], dims[2], grid_bricks, grid_bricks * DIRECTORY_BYTES, int(budget)))
        return origin, dims
    nodes = dims[0] * dims[1] * dims[2]
    cap = min(MAX_NODES, int(budget // NODE_BYTES))
    if nodes > cap:
        fit = voxel
        while True:                                                             # (a few steps of 5%: the count falls with the cube)
            fit *= 1.05
            if math.prod(max(2, int(math.ceil(e / fit)) + 1) for e in ext) <= cap:
                break
        raise RuntimeError("%s: the volume would hold %d nodes (%d x %d x %d) = %d bytes with its extraction, above the "
                           "memory_budget of %d bytes (and the limit of 2^31 - 1 nodes); a voxel_size of %g would fit" %
                           (what, nodes, dims[0], dims[1], dims[2], nodes * NODE_BYTES, int(budget), fit))
    return origin, dims


def _frustum_bounds(depth, mask, views, H, W):
    """The box of the views' frusta between the least and the greatest used depth of each: a cover of every back-projected
    pixel.  One read-back (two numbers per view)."""
    used = (mask != 0) & torch.isfinite(depth) & (depth > 0)
    big = torch.finfo(torch.float32).max
    near = torch.where(used, depth, depth.new_full((), big)).flatten(1).amin(1)
    far = torch.where(used, depth, depth.new_full((), 0.0)).flatten(1).amax(1)
    ends = torch.stack([near, far], 1).double().cpu().numpy()
    pts = []
    for v, (dn, df) in enumerate(ends):
        if not df > 0:
            continue
        K, R, t = views[v, :9].reshape(3, 3), views[v, 9:18].reshape(3, 3), views[v, 18:]
        corners = np.array([[x, y, 1.0] for x in (-0.5, W - 0.5) for y in (-0.5, H - 0.5)])
        rays = np.linalg.solve(K, corners.T).T
        for d in (dn, df):
            pts.append((rays * d - t) @ R)                                      # R^T (c - t), row-wise
    if not pts:
        raise RuntimeError("mesh_scene: no pixel with a usable depth, so there are no bounds; pass bounds=")
    pts = np.concatenate(pts)
    return pts.min(0), pts.max(0)


def mesh_scene(depths, masks, images, Ks, Es, voxel_size, trunc=None, bounds=None, min_weight=2, memory_budget=MEMORY_BUDGET,
               device=None, fill=None, mesh_clean=None, sparse=False):
    """``integrate_tsdf`` then ``extract_mesh`` for the maps of a scan.  ``trunc`` defaults to 4 ``voxel_size`` and is refused
    below 2 ``voxel_size`` (the ends of a crossing edge could both be clamped).  ``bounds`` = (lo, hi), three numbers each: the
    grid covers the box padded by ``trunc``, its origin is lo - trunc (``grid_for_bounds``); None: the box of the views' frusta
    between each view's least and greatest used depth (one more read-back).  A volume above ``memory_budget`` bytes is refused
    with the voxel size that would fit.  ``min_weight`` (default 2): a node seen by fewer views is unknown.  -> dict:
    ``vertices``, ``colors``, ``triangles`` (as ``extract_mesh``) and ``volume`` (the ``TSDFVolume``).  ``mesh_clean`` (a
    ``MeshClean``; default None: nothing changes and no launch is added): the extracted mesh goes through ``clean_mesh`` and
    the three keys hold the cleaned mesh, with ``clean_stats`` and, where asked for, ``normals`` / ``normals_valid``.
    ``sparse`` (default False: nothing changes, the same launches and bytes): ``allocate_bricks``, ``integrate_tsdf_sparse`` and
    ``extract_mesh_sparse``: the node cap of the dense grid does not apply, ``memory_budget`` is checked
    against the allocated bricks, ``volume`` is a ``SparseTSDFVolume`` and the result also holds ``vertex_key``.  The mesh is
    the dense one in another vertex and triangle order."""
    what = "mesh_scene"
    sparse = _flag(what, "sparse", sparse)
    clean = check_clean_spec(what, mesh_clean)
    V, H, W = _check_maps(what, depths, masks, images)
    views = _cameras(what, Ks, Es, V)
    voxel = _number(what, "voxel_size", voxel_size)
    t = _check_trunc(what, voxel, trunc)
    mw = _check_min_weight(what, min_weight)
    if bounds is not None:
        try:
            lo, hi = bounds
        except (TypeError, ValueError):
            raise RuntimeError("%s: bounds must be (lo, hi), not %r" % (what, bounds)) from None
        origin, dims = grid_for_bounds(what, lo, hi, voxel, t, memory_budget, sparse)
    else:
        _number(what, "memory_budget", memory_budget)
    dev = _device(what, device, (depths, masks, images))
    depth = _stack(depths, dev, torch.float32)
    mask = torch.ones(V, H, W, device=dev, dtype=torch.uint8) if masks is None else _stack(masks, dev, torch.bool).to(torch.uint8)
    if bounds is None:
        lo, hi = _frustum_bounds(depth, mask, views, H, W)
        origin, dims = grid_for_bounds(what, lo, hi, voxel, t, memory_budget, sparse)
    if sparse:
        vol = integrate_tsdf_sparse(depth, mask, images, Ks, Es, origin, voxel, dims, t, device=dev, memory_budget=memory_budget)
        m = extract_mesh_sparse(vol, mw, keys=True, fill=fill)
        out = dict(vertices=m.vertices, colors=m.colors, triangles=m.triangles, volume=vol, vertex_key=m.vertex_key)
    else:
        vol = integrate_tsdf(depth, mask, images, Ks, Es, origin, voxel, dims, t, device=dev)
        m = extract_mesh(vol, mw, fill=fill)
        out = dict(vertices=m.vertices, colors=m.colors, triangles=m.triangles, volume=vol)
    if clean is not None:
        c = clean_mesh(m.vertices, m.triangles, m.colors, *clean, fill=fill, _checked=True)
        out.update(_cleaned_keys(c, clean, ""))
        if sparse:
            out["vertex_key"] = m.vertex_key[c["vertex_index"]]
    return out


def _cleaned_keys(c, clean, prefix):
    """What a ``MeshClean`` adds to a result: the cleaned mesh over the three mesh keys, its statistics, its normals if asked."""
    out = {prefix + "vertices": c["vertices"], prefix + "colors": c["colors"], prefix + "triangles": c["triangles"],
           prefix + "clean_stats": c["stats"]}
    if clean.normals:
        out[prefix + "normals"], out[prefix + "normals_valid"] = c["normals"], c["normals_valid"]
    return out


def mesh_fused(res, images, Ks, Es, ref_views, spec, what="fuse_scene", clean=None, sparse=False):
    """fuse_scene's last step with a ``TSDFMesh``: the reference views' ``depth_est_averaged`` (as float32) under
    ``final_mask``, their images and cameras through ``mesh_scene``, within the box of the cloud that would be written
    (``final_*``, else ``thin_*``, else ``points``) -> the ``mesh_*`` keys.  An empty cloud gives an empty mesh.  ``clean`` (a
    checked ``MeshClean``): the mesh goes through ``clean_mesh``; the ``mesh_*`` keys hold the cleaned mesh, with
    ``mesh_clean_stats`` and, where asked for, ``mesh_normals`` / ``mesh_normals_valid``.  ``sparse``: the spec's fourth field
    (``mesh_scene(..., sparse=True)``; one more key, ``mesh_vertex_key``)."""
    voxel, trunc, mw = spec
    pts = res["final_points"] if "final_points" in res else res["thin_points"] if "thin_points" in res else res["points"]
    dev = pts.device
    if images.dtype != torch.uint8:                                             # float 0 .. 1: the bytes fuse_scene's colours have
        images = (images.to(torch.float32) * 255.0).to(torch.int32).to(torch.uint8)
    idx = torch.as_tensor(np.asarray(ref_views, np.int64), device=dev)
    if len(pts) == 0:
        out = dict(mesh_vertices=torch.empty(0, 3, device=dev, dtype=torch.float32),
                   mesh_colors=torch.empty(0, 3, device=dev, dtype=torch.uint8),
                   mesh_triangles=torch.empty(0, 3, device=dev, dtype=torch.int32), mesh_volume=None)
        if sparse:
            out["mesh_vertex_key"] = torch.empty(0, device=dev, dtype=torch.int64)
        if clean is not None:
            out.update(_cleaned_keys(clean_mesh(out["mesh_vertices"], out["mesh_triangles"], out["mesh_colors"], *clean, _checked=True),
                                     clean, "mesh_"))
        return out
    box = torch.stack([pts.amin(0), pts.amax(0)]).double().cpu().numpy()       # one read-back: the cloud's box
    if not np.isfinite(box).all():
        raise RuntimeError("%s: the cloud holds a point that is not finite, so the mesh has no bounds" % what)
    m = mesh_scene(res["depth_est_averaged"].to(torch.float32), res["final_mask"], images[idx], [Ks[int(r)] for r in ref_views],
                   [Es[int(r)] for r in ref_views], voxel, trunc, (box[0], box[1]), mw, device=dev, **(dict(sparse=True) if sparse else {}))
    vol = m["volume"]
    out = dict(mesh_vertices=m["vertices"], mesh_colors=m["colors"], mesh_triangles=m["triangles"],
               mesh_volume=dict(vol.params(), min_weight=mw, bounds=(tuple(box[0]), tuple(box[1]))))
    if sparse:
        out["mesh_vertex_key"] = m["vertex_key"]
    if clean is not None:
        c = clean_mesh(m["vertices"], m["triangles"], m["colors"], *clean, _checked=True)
        out.update(_cleaned_keys(c, clean, "mesh_"))
        if sparse:
            out["mesh_vertex_key"] = m["vertex_key"][c["vertex_index"]]
    return out


# ---- cleaning a mesh ------------------------------------------------------------------------------------------------------------------

def _flag(what, name, value):
    if not isinstance(value, (bool, np.bool_)):
        raise RuntimeError("%s: %s must be True or False, not %r" % (what, name, value))
    return bool(value)


def _check_min_triangles(what, min_triangles):
    if isinstance(min_triangles, (bool, np.bool_)) or not isinstance(min_triangles, (int, np.integer)) or \
            not 0 <= int(min_triangles) < (1 << 31):
        raise RuntimeError("%s: min_triangles must be an integer >= 0 (and below 2^31), not %r" % (what, min_triangles))
    return int(min_triangles)


def check_clean_spec(what, mesh_clean, mesh=True):
    """The ``mesh_clean`` keyword of the scan-level entry points, checked before anything runs -> a ``MeshClean`` of plain Python
    values, or None.  ``mesh``: the call's ``mesh=`` keyword (a ``MeshClean`` without a mesh to clean is refused)."""
    if mesh_clean is None:
        return None
    if not isinstance(mesh_clean, MeshClean):
        raise RuntimeError("%s: mesh_clean must be None or a MeshClean, not %r" % (what, mesh_clean))
    if mesh is None:
        raise RuntimeError("%s: mesh_clean needs mesh= (a TSDFMesh): there is no mesh to clean" % what)
    return MeshClean(_flag(what, "mesh_clean.weld", mesh_clean.weld), _check_min_triangles(what, mesh_clean.min_triangles),
                     _flag(what, "mesh_clean.largest_only", mesh_clean.largest_only), _flag(what, "mesh_clean.normals", mesh_clean.normals))


def clean_slots(n_vertices):
    """The smallest weld table ``clean_mesh`` takes: a power of two, at least max(64, 2 * Nv) slots."""
    return max(64, 1 << max(0, 2 * int(n_vertices) - 1).bit_length())


def _check_triangles(what, triangles, n_vertices, checked=False):
    """triangles [Nt,3] int32 with every index in 0 .. n_vertices - 1 (one read-back of the least and the greatest index, before
    any launch of the library; ``checked``: the mesh is ``extract_mesh``'s own and the look is left out) -> Nt"""
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int32:
        raise RuntimeError("%s: triangles must be an int32 tensor [Nt,3], not %s" %
                           (what, (tuple(triangles.shape), triangles.dtype) if isinstance(triangles, torch.Tensor) else type(triangles).__name__))
    nt = triangles.shape[0]
    if nt > MAX_CLEAN_TRIANGLES:
        raise RuntimeError("%s: at most 2^29 triangles, not %d" % (what, nt))
    if nt and not checked:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(triangles)).cpu())
        if lo < 0 or hi >= n_vertices:
            raise RuntimeError("%s: a triangle names vertex %d, outside 0 .. %d" % (what, lo if lo < 0 else hi, n_vertices - 1))
    return nt


def _check_vertices(what, vertices, colors=None):
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise RuntimeError("%s: vertices must be a float32 tensor [Nv,3], not %s" %
                           (what, (tuple(vertices.shape), vertices.dtype) if isinstance(vertices, torch.Tensor) else type(vertices).__name__))
    if vertices.shape[0] > MAX_CLEAN_VERTICES:
        raise RuntimeError("%s: at most 2^29 vertices, not %d" % (what, vertices.shape[0]))
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.shape != vertices.shape or colors.dtype != torch.uint8):
        raise RuntimeError("%s: colors must be a uint8 tensor [Nv,3] with the Nv of vertices" % what)
    return vertices.shape[0]


def _on_gpu(what, *tensors):
    ts = [t for t in tensors if t is not None]
    if not all(t.is_cuda and t.device == ts[0].device for t in ts):
        raise RuntimeError("mvster_amd.mesh.%s runs on MI355X only: its tensors must be on one GPU (there is no CPU fallback)" % what)
    return ts[0].device


class _CleanPlan:
    """``mvster_mesh_clean_plan`` run on a mesh and its ONE read-back: ``canon``, ``labels`` [Nv], ``tri_labels``,
    ``tri_component`` [Nt], ``roots``, ``comp_vertices``, ``comp_triangles`` [components] on the GPU, and as Python ints
    ``nv_out``, ``nt_out``, ``components``, ``canonical``, ``dropped``, ``kept``.  ``emit`` writes the compacted mesh."""

    def __init__(self, what, vertices, triangles, n_vertices, weld, min_triangles, largest_only, slots):
        lib = _lib.load()
        dev = triangles.device
        self.vertices, self.triangles = vertices, triangles.contiguous()
        nv, nt = self.nv, self.nt = n_vertices, triangles.shape[0]
        rows = min(nv, nt)
        i32 = dict(device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev).cuda_stream
            self.canon, self.labels = torch.empty(nv, **i32), torch.empty(nv, **i32)
            self.tri_labels, self.tri_component = torch.empty(nt, **i32), torch.empty(nt, **i32)
            table = torch.empty(2 * slots, **i32) if weld else None
            comp = torch.empty(3, rows, **i32)
            n_ints, n_longs = ctypes.c_long(), ctypes.c_long()
            _lib.check(lib.mvster_mesh_clean_work(nv, nt, ctypes.byref(n_ints), ctypes.byref(n_longs)), "mesh_clean_work")
            self.work_ints = torch.empty(n_ints.value, **i32)
            self.work_longs = torch.empty(n_longs.value, device=dev, dtype=torch.int64)
            _lib.check(lib.mvster_mesh_clean_plan(None if vertices is None else self.vertices.data_ptr(), self.triangles.data_ptr(), nv,
                                                  nt, int(weld), min_triangles, int(largest_only),
                                                  table.data_ptr() if weld else None, slots if weld else 0, self.canon.data_ptr(),
                                                  self.labels.data_ptr(), self.tri_labels.data_ptr(), self.tri_component.data_ptr(),
                                                  comp[0].data_ptr(), comp[1].data_ptr(), comp[2].data_ptr(), rows,
                                                  self.work_ints.data_ptr(), self.work_longs.data_ptr(), self.stream), "mesh_clean_plan")
            stats = [int(x) for x in self.work_longs[-8:].cpu()]                   # the one read-back: counts and status
        self.nv_out, self.nt_out, self.components, self.canonical, self.dropped, self.kept, status = stats[:7]
        if status:
            raise RuntimeError("%s: the weld table of %d slots is full (this cannot happen at the enforced size)" % (what, slots))
        self.roots, self.comp_vertices, self.comp_triangles = (comp[k, :self.components] for k in range(3))

    def emit(self, colors, vertices, out_colors, triangles, vertex_index, triangle_index, nv_out=None, nt_out=None):
        """The kept vertices and triangles into the caller's buffers (``nv_out`` / ``nt_out``: their capacity in entries)."""
        nv_out = self.nv_out if nv_out is None else nv_out
        nt_out = self.nt_out if nt_out is None else nt_out
        with torch.cuda.device(self.triangles.device):
            _lib.check(_lib.load().mvster_mesh_clean_emit(
                self.vertices.data_ptr(), None if colors is None else colors.data_ptr(), self.triangles.data_ptr(), self.nv, self.nt,
                self.canon.data_ptr(), self.work_ints.data_ptr(), nv_out, nt_out,
                vertices.data_ptr() if nv_out else None, out_colors.data_ptr() if nv_out and colors is not None else None,
                triangles.data_ptr() if nt_out else None, vertex_index.data_ptr() if nv_out else None,
                triangle_index.data_ptr() if nt_out else None, self.stream), "mesh_clean_emit")


def mesh_components(triangles, n_vertices):
    """The connected components of a triangle list on the GPU (defined exactly in
    mvster_amd/csrc/mesh_math.h): ``triangles`` [Nt,3] int32 on the GPU with every index in 0 .. ``n_vertices`` - 1.  A triangle
    that names a vertex twice is dropped; two others are connected if they share a vertex (vertex connectivity: Open3D's
    ``cluster_connected_triangles`` connects across shared edges only).  -> dict of GPU tensors: ``labels`` [n_vertices] int32 =
    the smallest vertex of a vertex's component (-1 for a vertex no kept triangle names), ``tri_labels`` [Nt] int32 (-1 for a
    dropped triangle), ``tri_component`` [Nt] int32 = the row of the triangle's component in the table, and the table in
    ascending order of ``roots`` [C] int32 with ``n_vertices`` / ``n_triangles`` [C] int32.  Lock-free union-find with integer
    atomics: the result does not depend on the run.  One read-back (C) besides the look at the index range.  No CPU fallback."""
    what = "mesh_components"
    if isinstance(n_vertices, (bool, np.bool_)) or not isinstance(n_vertices, (int, np.integer)) or \
            not 0 <= int(n_vertices) <= MAX_CLEAN_VERTICES:
        raise RuntimeError("%s: n_vertices must be an integer in 0 .. 2^29, not %r" % (what, n_vertices))
    nv = int(n_vertices)
    nt = _check_triangles(what, triangles, nv)
    dev = _on_gpu(what, triangles)
    if nv == 0 or nt == 0:
        e = torch.empty(0, device=dev, dtype=torch.int32)
        return dict(labels=torch.full((nv,), -1, device=dev, dtype=torch.int32), tri_labels=e, tri_component=e.clone(), roots=e.clone(),
                    n_vertices=e.clone(), n_triangles=e.clone())
    p = _CleanPlan(what, None, triangles, nv, False, 0, False, 0)
    return dict(labels=p.labels, tri_labels=p.tri_labels, tri_component=p.tri_component, roots=p.roots, n_vertices=p.comp_vertices,
                n_triangles=p.comp_triangles)


def vertex_normals(vertices, triangles, fill=None, _checked=False):
    """Area-weighted vertex normals on the GPU (defined exactly in mvster_amd/csrc/mesh_math.h):
    ``vertices`` [Nv,3] float32 and ``triangles`` [Nt,3] int32 on the GPU.  With the positions widened to fp64, a triangle
    (a, b, c) gives n_t = (b - a) x (c - a); a vertex's N is the sum of n_t over the triangles that name it in ascending triangle
    index (once per occurrence), its normal (float)(N / |N|).  -> dict: ``normals`` [Nv,3] float32 and ``valid`` [Nv] uint8:
    zeros and 0 where |N| is 0 or not finite or no triangle names the vertex.  The normal follows the winding; for
    ``extract_mesh`` output it points to the free-space side.  This is the project's own definition (Open3D sums unit triangle
    normals).  The order of every sum is fixed (vertex -> triangle rows put into ascending order): no floating-point atomics,
    two runs give the same bytes.  No read-back besides the look at the index range.  ``fill`` (tests): a byte the outputs are
    filled with before the kernels write them.  No CPU fallback."""
    what = "vertex_normals"
    nv = _check_vertices(what, vertices)
    nt = _check_triangles(what, triangles, nv, _checked)
    dev = _on_gpu(what, vertices, triangles)
    if nv == 0 or nt == 0:
        return dict(normals=torch.zeros(nv, 3, device=dev, dtype=torch.float32), valid=torch.zeros(nv, device=dev, dtype=torch.uint8))
    vertices, triangles = vertices.contiguous(), triangles.contiguous()
    normals = torch.empty(nv, 3, device=dev, dtype=torch.float32)
    valid = torch.empty(nv, device=dev, dtype=torch.uint8)
    if fill is not None:
        normals.view(torch.uint8).fill_(int(fill))
        valid.fill_(int(fill))
    with torch.cuda.device(dev):
        lib = _lib.load()
        blocks = lib.mvster_mesh_normals_blocks(nv)
        work_ints = torch.empty(2 * nv + blocks, device=dev, dtype=torch.int32)
        work_longs = torch.empty(blocks + 1, device=dev, dtype=torch.int64)
        rows = torch.empty(3 * nt, device=dev, dtype=torch.int32)
        _lib.check(lib.mvster_mesh_vertex_normals(vertices.data_ptr(), triangles.data_ptr(), nv, nt, work_ints.data_ptr(),
                                                  work_longs.data_ptr(), rows.data_ptr(), normals.data_ptr(), valid.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "mesh_vertex_normals")
    return dict(normals=normals, valid=valid)


def clean_mesh(vertices, triangles, colors=None, weld=True, min_triangles=0, largest_only=False, normals=False, table_slots=None,
               fill=None, _checked=False):
    """A mesh cleaned on the GPU (defined exactly in mvster_amd/csrc/mesh_math.h): ``vertices`` [Nv,3]
    float32, ``triangles`` [Nt,3] int32 (every index in 0 .. Nv-1) and optionally ``colors`` [Nv,3] uint8, tensors on the GPU.  In
    this order: ``weld``: vertices whose three coordinates compare equal (-0.0 equals 0.0; one that is not finite equals
    nothing) become the one with the smallest index, which keeps its own position and colour; a triangle with two equal corners
    after that, or with a corner that is not finite, is dropped (collinear ones with three distinct corners are kept, duplicate
    triangles are not looked for); the rest fall into components by shared vertices (``mesh_components``); a component is kept
    iff it has at least ``min_triangles`` triangles and, with ``largest_only``, is the one with the most (ties: the one with the
    smallest vertex); the kept triangles stay in input order, the vertices they use (canonical ones) stay in input order, and the
    indices are renumbered.  -> dict: ``vertices`` [Nv',3], ``colors`` [Nv',3] (None without ``colors``), ``triangles``
    [Nt',3], ``vertex_index`` [Nv'] and ``triangle_index`` [Nt'] int64 into the input; with ``normals``: ``normals`` [Nv',3]
    float32 and ``normals_valid`` [Nv'] uint8, ``vertex_normals`` of the cleaned mesh; ``stats``: ``welded`` (vertices that
    coincide with an earlier one), ``degenerate`` (triangles dropped), ``components``, ``components_kept``,
    ``triangles_removed``, ``vertices_removed`` (Python ints).  Integer atomics only and fixed sum orders: two runs give the same
    bytes, whatever ``table_slots`` (the weld's hash table: a power of two >= max(64, 2 * Nv), default the smallest).  One
    read-back holds the counts and the table's status; the public call looks at the index range before (one more).  An empty
    input (Nv = 0 or Nt = 0) launches nothing and gives an empty mesh.  ``fill`` (tests): a byte the outputs are filled with
    before the kernels write them.  No CPU fallback."""
    what = "clean_mesh"
    weld, largest_only, normals = _flag(what, "weld", weld), _flag(what, "largest_only", largest_only), _flag(what, "normals", normals)
    min_triangles = _check_min_triangles(what, min_triangles)
    nv = _check_vertices(what, vertices, colors)
    slots = clean_slots(nv) if table_slots is None else table_slots
    if isinstance(slots, bool) or not isinstance(slots, int) or slots < clean_slots(nv) or slots & (slots - 1) or slots > 1 << 30:
        raise RuntimeError("%s: table_slots must be a power of two, >= max(64, 2 * Nv) = %d and <= 2^30, not %r" %
                           (what, max(64, 2 * nv), table_slots))
    nt = _check_triangles(what, triangles, nv, _checked)
    dev = _on_gpu(what, vertices, triangles, colors)
    if nv == 0 or nt == 0:
        nvo, nto, plan = 0, 0, None
        stats = dict(welded=0, degenerate=0, components=0, components_kept=0)
    else:
        vertices = vertices.contiguous()
        colors = None if colors is None else colors.contiguous()
        plan = _CleanPlan(what, vertices, triangles, nv, weld, min_triangles, largest_only, slots)
        nvo, nto = plan.nv_out, plan.nt_out
        stats = dict(welded=nv - plan.canonical, degenerate=plan.dropped, components=plan.components, components_kept=plan.kept)
    stats.update(triangles_removed=nt - nto, vertices_removed=nv - nvo)
    out = dict(vertices=torch.empty(nvo, 3, device=dev, dtype=torch.float32),
               colors=None if colors is None else torch.empty(nvo, 3, device=dev, dtype=torch.uint8),
               triangles=torch.empty(nto, 3, device=dev, dtype=torch.int32), vertex_index=torch.empty(nvo, device=dev, dtype=torch.int64),
               triangle_index=torch.empty(nto, device=dev, dtype=torch.int64), stats=stats)
    if fill is not None:
        for k in ("vertices", "colors", "triangles", "vertex_index", "triangle_index"):
            if out[k] is not None:
                out[k].view(torch.uint8).fill_(int(fill))
    if plan is not None:
        plan.emit(colors, out["vertices"], out["colors"], out["triangles"], out["vertex_index"], out["triangle_index"])
    if normals:
        n = vertex_normals(out["vertices"], out["triangles"], fill=fill, _checked=True)
        out["normals"], out["normals_valid"] = n["normals"], n["valid"]
    return out


# ---- files -------------------------------------------------------------------------------------------------------------------------------

PLY_XYZ_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
PLY_XYZRGB_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
PLY_NORMAL_FIELDS = [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _ply_vertex_dtype(with_normals, with_colors):
    if not with_normals:
        return PLY_XYZRGB_DTYPE if with_colors else PLY_XYZ_DTYPE
    return np.dtype(PLY_XYZ_DTYPE.descr + PLY_NORMAL_FIELDS + (PLY_XYZRGB_DTYPE.descr[3:] if with_colors else []))


def write_mesh_ply(filename, vertices, triangles, colors=None, normals=None):
    """A triangle mesh as a binary little-endian PLY: ``vertex`` (x y z float, with ``normals`` nx ny nz float behind them, with
    ``colors`` red green blue uchar last) and ``face`` (``property list uchar int vertex_indices``, three indices each).  Arrays
    or tensors; an empty mesh is a valid file."""
    v, t = _host(vertices), _host(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise RuntimeError("write_mesh_ply: vertices must be [Nv,3] and triangles [Nt,3], not %s and %s" % (v.shape, t.shape))
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise RuntimeError("write_mesh_ply: a triangle names a vertex outside 0 .. %d" % (len(v) - 1))
    rec = np.empty(len(v), dtype=_ply_vertex_dtype(normals is not None, colors is not None))
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        n = _host(normals)
        if n.shape != v.shape or n.dtype != np.float32:
            raise RuntimeError("write_mesh_ply: normals must be [Nv,3] float32 with the Nv of vertices, not %s %s" % (n.shape, n.dtype))
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        c = _host(colors)
        if c.shape != v.shape or c.dtype != np.uint8:
            raise RuntimeError("write_mesh_ply: colors must be [Nv,3] uint8 with the Nv of vertices, not %s %s" % (c.shape, c.dtype))
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    faces = np.empty(len(t), dtype=PLY_FACE_DTYPE)
    faces["n"], faces["v"] = 3, t
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + props +
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(t))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_mesh_ply(filename, with_normals=False):
    """Inverse of ``write_mesh_ply`` -> (vertices [Nv,3] float32, triangles [Nt,3] int32, colors [Nv,3] uint8 or None); with
    ``with_normals`` a fourth entry, normals [Nv,3] float32 or None.  A file with normals is read either way."""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in head or "property list uchar int vertex_indices" not in head:
        raise RuntimeError("read_mesh_ply: only the binary little-endian layout of write_mesh_ply is read")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nt = int([l for l in head if l.startswith("element face")][0].split()[-1])
    has_normals, has_colors = "property float nx" in head, "property uchar red" in head
    dt = _ply_vertex_dtype(has_normals, has_colors)
    rec = np.frombuffer(data[end:end + nv * dt.itemsize], dtype=dt)
    faces = np.frombuffer(data[end + nv * dt.itemsize:end + nv * dt.itemsize + nt * PLY_FACE_DTYPE.itemsize], dtype=PLY_FACE_DTYPE)
    if len(rec) != nv or len(faces) != nt or (nt and not (faces["n"] == 3).all()):
        raise RuntimeError("read_mesh_ply: %s is cut short or holds a face that is not a triangle" % filename)
    v = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
    c = np.stack([rec["red"], rec["green"], rec["blue"]], 1).astype(np.uint8) if has_colors else None
    out = (v, faces["v"].astype(np.int32).reshape(-1, 3), c)
    if with_normals:
        out += (np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float32) if has_normals else None,)
    return out


def write_result_mesh(filename, res):
    """The ``mesh_*`` keys of a SceneResult as a PLY, with ``mesh_normals`` where the result has them."""
    write_mesh_ply(filename, res["mesh_vertices"], res["mesh_triangles"], res["mesh_colors"],
                   res["mesh_normals"] if "mesh_normals" in res else None)
