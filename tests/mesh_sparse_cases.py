"""Shared by tests/test_mesh_sparse_cpu.py and tests/test_gpu_mesh_sparse.py (not a test module): the host build of
mvster_amd/csrc/tsdf_sparse_math.h, the cases of tests/mesh_cases.py refined and cut into bricks, the needed bricks of a scan
restated in NumPy from the definition, and the canonical form in which a sparse and a dense mesh are compared.

The yardstick is the dense path: ``mesh_cases.integrate_host`` / ``extract_host``, the host build of tsdf_math.h, which the
existing tests pin against NumPy."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

from tests import fusion_scene_cases as C
from tests import mesh_cases as M

BRICK, BRICK_NODES = 8, 512
MAP_KEYS = ("depths", "masks", "images", "Ks", "Es", "origin", "voxel", "dims", "trunc")

_HM = {}


def load_sparse_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/tsdf_sparse_hostmath.cpp as ``mesh_cases.load_tsdf_hostmath`` does and load it, once per process.
    No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of tsdf_sparse_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libtsdfsparsehostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "tsdf_sparse_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, i, d = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double
    h.hm_sparse_grid_bricks.restype, h.hm_sparse_grid_bricks.argtypes = l, [l, l, l]
    h.hm_sparse_mark.restype, h.hm_sparse_mark.argtypes = None, [p, p, p, i, i, i, d, d, d, d, i, i, i, d, p]
    h.hm_sparse_integrate.restype, h.hm_sparse_integrate.argtypes = None, [p, p, p, p, i, i, i, d, d, d, d, i, i, i, d, p, l, p, p, p, p]
    h.hm_sparse_count.restype, h.hm_sparse_count.argtypes = None, [p, p, p, p, l, i, i, i, i, p, p, p]
    h.hm_sparse_emit.restype, h.hm_sparse_emit.argtypes = None, [p, p, p, p, p, p, l, d, d, d, d, i, i, i, i, p, p, p, p, p, p]
    _HM[compilers] = h
    return h


# ---- bricks -----------------------------------------------------------------------------------------------------------------------------

def brick_dims(dims):
    return tuple((int(n) + BRICK - 1) // BRICK for n in dims)


def directory(bricks, dims):
    """-> brick_slot [nbricks] int32 of an ascending brick list"""
    nb = brick_dims(dims)
    slot = np.full(nb[0] * nb[1] * nb[2], -1, np.int32)
    slot[np.asarray(bricks, np.int64)] = np.arange(len(bricks), dtype=np.int32)
    return slot


def brick_sets(dims, seed):
    """name -> ascending int32 brick list: the full set, the empty set, a single brick, a seeded random half"""
    nb = brick_dims(dims)
    n = nb[0] * nb[1] * nb[2]
    rng = np.random.RandomState(seed)
    half = np.sort(rng.permutation(n)[:max(1, n // 2)])
    return {"full": np.arange(n, dtype=np.int32), "empty": np.zeros(0, np.int32), "single": np.array([rng.randint(n)], np.int32),
            "half": half.astype(np.int32)}


def node_bricks(dims):
    """-> the brick number of every node, [nz,ny,nx] int64"""
    nx, ny, nz = dims
    nb = brick_dims(dims)
    k, j, i = np.meshgrid(np.arange(nz) // BRICK, np.arange(ny) // BRICK, np.arange(nx) // BRICK, indexing="ij")
    return i + nb[0] * (j + nb[1] * k)


def cut_into_bricks(v, bricks):
    """A dense volume (a case of ``mesh_cases``) cut into the bricks of the list -> dict of brick-major arrays; words beyond the
    grid hold the empty values"""
    nx, ny, nz = v["dims"]
    nb = brick_dims(v["dims"])
    pad = lambda a, fill: np.pad(np.asarray(a).reshape((nz, ny, nx) + np.asarray(a).shape[3:]),
                                 [(0, nb[2] * BRICK - nz), (0, nb[1] * BRICK - ny), (0, nb[0] * BRICK - nx)] + [(0, 0)] * (np.asarray(a).ndim - 3),
                                 constant_values=fill)
    b = np.asarray(bricks, np.int64)
    bi, bj, bk = b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])
    l = np.arange(BRICK)
    k = (bk[:, None] * BRICK + l)[:, :, None, None]
    j = (bj[:, None] * BRICK + l)[:, None, :, None]
    i = (bi[:, None] * BRICK + l)[:, None, None, :]
    out = {}
    for name, fill, dtype in (("tsdf", 1.0, np.float32), ("weight", 0, np.int32), ("rgb", 0, np.uint8), ("has_color", 0, np.uint8)):
        a = pad(np.asarray(v[name], dtype), fill)[k, j, i]
        out[name] = np.ascontiguousarray(a.reshape((len(b), BRICK_NODES) + a.shape[4:]))
    return out


def masked_outside(v, bricks):
    """The dense volume with the weights of the nodes outside the bricks set to 0 (what the sparse volume means, as far as the
    extraction can tell)"""
    inside = np.isin(node_bricks(v["dims"]), np.asarray(bricks, np.int64))
    return dict(v, weight=np.where(inside, np.asarray(v["weight"]).reshape(inside.shape), 0).astype(np.int32))


# ---- the host build ------------------------------------------------------------------------------------------------------------------------

def _maps(depths, masks, Ks, Es):
    return (np.ascontiguousarray(depths, np.float32), np.ascontiguousarray(np.asarray(masks) != 0, np.uint8),
            np.ascontiguousarray(M.views_table(Ks, Es)))


def allocate_host(h, depths, masks, Ks, Es, origin, voxel, dims, trunc):
    """-> bricks [Nb] int32 ascending"""
    depth, mask, views = _maps(depths, masks, Ks, Es)
    V, H, W = depth.shape
    nb = brick_dims(dims)
    flags = np.zeros(nb[0] * nb[1] * nb[2], np.uint8)
    h.hm_sparse_mark(depth.ctypes.data, mask.ctypes.data, views.ctypes.data, V, H, W, *[float(o) for o in origin], float(voxel),
                     *[int(n) for n in dims], float(trunc), flags.ctypes.data)
    assert set(np.unique(flags)) <= {0, 1}
    return np.nonzero(flags)[0].astype(np.int32)


def integrate_sparse_host(h, depths, masks, images, Ks, Es, origin, voxel, dims, trunc, bricks):
    """-> dict of brick-major arrays (pre-filled with a sentinel the build must overwrite)"""
    depth, mask, views = _maps(depths, masks, Ks, Es)
    img = np.ascontiguousarray(images, np.uint8)
    V, H, W = depth.shape
    b = np.ascontiguousarray(bricks, np.int32)
    n = len(b)
    out = dict(tsdf=np.full((n, BRICK_NODES), np.nan, np.float32), weight=np.full((n, BRICK_NODES), -9, np.int32),
               rgb=np.full((n, BRICK_NODES, 3), 0xCD, np.uint8), has_color=np.full((n, BRICK_NODES), 0xCD, np.uint8))
    h.hm_sparse_integrate(depth.ctypes.data, mask.ctypes.data, img.ctypes.data, views.ctypes.data, V, H, W, *[float(o) for o in origin],
                          float(voxel), *[int(x) for x in dims], float(trunc), b.ctypes.data, n, out["tsdf"].ctypes.data,
                          out["weight"].ctypes.data, out["rgb"].ctypes.data, out["has_color"].ctypes.data)
    return out


def extract_sparse_host(h, vol, bricks, origin, voxel, dims, min_weight):
    """vol: brick-major arrays -> vertices, colors, triangles, keys"""
    b = np.ascontiguousarray(bricks, np.int32)
    n = len(b)
    slot = directory(b, dims)
    f, w = np.ascontiguousarray(vol["tsdf"], np.float32), np.ascontiguousarray(vol["weight"], np.int32)
    c, hc = np.ascontiguousarray(vol["rgb"], np.uint8), np.ascontiguousarray(vol["has_color"], np.uint8)
    edge_mask, vbase, counts = np.zeros(max(1, n * BRICK_NODES), np.uint8), np.zeros(max(1, n * BRICK_NODES), np.int64), np.zeros(2, np.int64)
    h.hm_sparse_count(f.ctypes.data, w.ctypes.data, slot.ctypes.data, b.ctypes.data, n, *[int(x) for x in dims], int(min_weight),
                      edge_mask.ctypes.data, vbase.ctypes.data, counts.ctypes.data)
    nv, nt = int(counts[0]), int(counts[1])
    vertices, colors = np.full((nv, 3), np.nan, np.float32), np.full((nv, 3), 0xCD, np.uint8)
    keys, triangles = np.full(nv, -1, np.int64), np.full((nt, 3), -1, np.int32)
    h.hm_sparse_emit(f.ctypes.data, w.ctypes.data, c.ctypes.data, hc.ctypes.data, slot.ctypes.data, b.ctypes.data, n,
                     *[float(o) for o in origin], float(voxel), *[int(x) for x in dims], int(min_weight), edge_mask.ctypes.data,
                     vbase.ctypes.data, vertices.ctypes.data, colors.ctypes.data, keys.ctypes.data, triangles.ctypes.data)
    return vertices, colors, triangles, keys


# ---- the canonical form ----------------------------------------------------------------------------------------------------------------------

def dense_keys(owners):
    owners = np.asarray(owners, np.int64).reshape(-1, 2)
    return owners[:, 0] * 8 + owners[:, 1]


def canonical(vertices, colors, triangles, keys):
    """-> (keys ascending, positions and colours in that order, the triangles as key triples in emission rotation, sorted)"""
    keys = np.asarray(keys, np.int64)
    assert len(np.unique(keys)) == len(keys), "a vertex key appears twice"
    order = np.argsort(keys, kind="stable")
    tri = keys[np.asarray(triangles, np.int64).reshape(-1, 3)]
    tri = tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))] if len(tri) else tri
    return keys[order], np.asarray(vertices)[order], np.asarray(colors)[order], tri


def assert_canonically_equal(got, want, what=""):
    """got, want: (vertices, colors, triangles, keys)"""
    g, w = canonical(*got), canonical(*want)
    for a, b, part in zip(g, w, ("keys", "positions", "colours", "triangles")):
        M.assert_bytes(a, b, (what, part))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------

REFINED = (("sphere_views", 4), ("plane", 4), ("plane_65", 2), ("bad_depths", 1), ("bad_depths", 3))
TIGHT = (("sphere_views", 4), ("plane", 4), ("plane_65", 2))                     # allocated <= 2 x needed is asked of these


@functools.lru_cache(None)
def refined(name, s):
    """A map case with its grid refined by s: voxel / s, dims (n - 1) s + 1, trunc 4 voxels"""
    c = dict(M.map_cases()[name])
    c["voxel"] = c["voxel"] / s
    c["dims"] = tuple((n - 1) * s + 1 for n in c["dims"])
    c["trunc"] = 4 * c["voxel"]
    return c


@functools.lru_cache(None)
def plane_129():
    """The plane in a 129^3 grid around it (same voxel): the plane sits mid-grid"""
    c = dict(M.map_cases()["plane"])
    c["origin"] = (-64 * c["voxel"], -64 * c["voxel"], M.PLANE_DEPTH - 64.6 * c["voxel"])
    c["dims"] = (129, 129, 129)
    return c


@functools.lru_cache(None)
def plane_huge():
    """The plane maps in a virtual grid of 2048 x 2048 x 1024 nodes = 2^32, the origin shifted so that the plane sits mid-grid"""
    c = dict(M.map_cases()["plane"])
    o = c["origin"]
    c["origin"] = (o[0] - 1024 * c["voxel"], o[1] - 1024 * c["voxel"], o[2] - 512 * c["voxel"])
    c["dims"] = (2048, 2048, 1024)
    return c


def needed_bricks(c):
    """The bricks the covering property speaks of, from the definition in NumPy: the nodes some view counts with
    -trunc <= sdf <= trunc, and their 26 neighbours -> ascending brick numbers"""
    nx, ny, nz = c["dims"]
    xs, ys, zs = M.node_coords(c["origin"], c["voxel"], c["dims"])
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    near = np.zeros((nz, ny, nx), bool)
    trunc = np.float64(c["trunc"])
    with np.errstate(all="ignore"):
        for v in range(len(c["depths"])):
            K, E = np.asarray(c["Ks"][v], np.float64), np.asarray(c["Es"][v], np.float64)
            H, W = c["depths"][v].shape
            cam = [((E[a, 0] * x + E[a, 1] * y) + E[a, 2] * z) + E[a, 3] for a in range(3)]
            u = ((K[0, 0] * cam[0] + K[0, 1] * cam[1]) + K[0, 2] * cam[2]) / cam[2] + 0.5
            t = ((K[1, 0] * cam[0] + K[1, 1] * cam[1]) + K[1, 2] * cam[2]) / cam[2] + 0.5
            ok = (cam[2] > 0) & (u >= 0) & (u < W) & (t >= 0) & (t < H)
            px, py = np.where(ok, u, 0).astype(np.int64), np.where(ok, t, 0).astype(np.int64)
            d = np.asarray(c["depths"][v], np.float32)[py, px]
            ok &= (np.asarray(c["masks"][v])[py, px] != 0) & np.isfinite(d) & (d > 0)
            sdf = d.astype(np.float64) - cam[2]
            near |= ok & (sdf >= -trunc) & (sdf <= trunc)
    ring = np.zeros_like(near)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ring |= M._shifted(near, (dx, dy, dz), False)
    return np.unique(node_bricks(c["dims"])[ring])


@functools.lru_cache(None)
def host_sparse(name, s, min_weight=1):
    """allocate + integrate + extract of a refined map case in the host build, computed once -> dict"""
    h = load_sparse_hostmath()
    c = refined(name, s)
    bricks = allocate_host(h, *(c[k] for k in ("depths", "masks", "Ks", "Es", "origin", "voxel", "dims", "trunc")))
    vol = integrate_sparse_host(h, *(c[k] for k in MAP_KEYS), bricks)
    return dict(bricks=bricks, volume=vol, mesh=extract_sparse_host(h, vol, bricks, c["origin"], c["voxel"], c["dims"], min_weight))


@functools.lru_cache(None)
def host_dense(name, s):
    """integrate_host of a refined map case, computed once -> tsdf, weight, rgb, has_color"""
    c = refined(name, s)
    return M.integrate_host(M.load_tsdf_hostmath(), *(c[k] for k in MAP_KEYS))


@functools.lru_cache(None)
def host_huge():
    """The 2^32-node plane in the host build, computed once -> dict"""
    h = load_sparse_hostmath()
    c = plane_huge()
    bricks = allocate_host(h, *(c[k] for k in ("depths", "masks", "Ks", "Es", "origin", "voxel", "dims", "trunc")))
    vol = integrate_sparse_host(h, *(c[k] for k in MAP_KEYS), bricks)
    return dict(bricks=bricks, volume=vol, mesh=extract_sparse_host(h, vol, bricks, c["origin"], c["voxel"], c["dims"], 1))


ANY_S_VOLUMES = ("grid_13x7x5", "grid_65x3x3", "grid_257x2x3", "grid_2x2x2", "holes", "exact_zero_random", "sphere_cut")


def rounding_term(v):
    """As tests/test_mesh_cpu.py: float32 rounding of a coordinate of magnitude <= m and of a sample |tsdf| <= 1, doubled"""
    m = max(abs(o) + v["voxel"] * n for o, n in zip(v["origin"], v["dims"]))
    return 2 * (np.sqrt(3) * m + v["trunc"]) * 2.0 ** -24
