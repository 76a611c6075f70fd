"""Shared by tests/test_mesh_cpu.py and tests/test_gpu_mesh.py (not a test module): the cases, TSDF integration and marching
tetrahedra restated in NumPy, and the host build of mvster_amd/csrc/tsdf_math.h.

Neither yardstick comes from the reference tree, which has no such step, nor from Open3D, which is not at hand.  The
restatement follows the definition vectorised over the nodes, with NumPy's own float64 operations in the order the definition
gives (so it can be compared byte for byte), and derives the triangles of a tetrahedron from the parity rule and the
determinant of the tetrahedron's edge vectors, not from the packed case table of the header; the host build is the kernels'
own arithmetic compiled for the CPU."""
import ctypes
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np

from tests import fusion_scene_cases as C

# ---- the definition, restated in NumPy ----------------------------------------------------------------------------------------------


def node_coords(origin, voxel, dims):
    """-> x [nx], y [ny], z [nz] float64"""
    return tuple(np.float64(o) + np.float64(voxel) * np.arange(n, dtype=np.float64) for o, n in zip(origin, dims))


def integrate_numpy(depths, masks, images, Ks, Es, origin, voxel, dims, trunc):
    """-> tsdf [nz,ny,nx] float32, weight int32, rgb [nz,ny,nx,3] uint8, has_color uint8"""
    nx, ny, nz = dims
    xs, ys, zs = node_coords(origin, voxel, dims)
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    sum_f = np.zeros((nz, ny, nx))
    w = np.zeros((nz, ny, nx), np.int64)
    c = np.zeros((nz, ny, nx), np.int64)
    col = np.zeros((nz, ny, nx, 3), np.int64)
    trunc = np.float64(trunc)
    with np.errstate(all="ignore"):
        for v in range(len(depths)):
            K, E = np.asarray(Ks[v], np.float64), np.asarray(Es[v], np.float64)
            H, W = depths[v].shape
            cam = [((E[a, 0] * x + E[a, 1] * y) + E[a, 2] * z) + E[a, 3] for a in range(3)]
            front = cam[2] > 0
            u = ((K[0, 0] * cam[0] + K[0, 1] * cam[1]) + K[0, 2] * cam[2]) / cam[2] + 0.5
            t = ((K[1, 0] * cam[0] + K[1, 1] * cam[1]) + K[1, 2] * cam[2]) / cam[2] + 0.5
            ok = front & (u >= 0) & (u < W) & (t >= 0) & (t < H)
            px, py = np.where(ok, u, 0).astype(np.int64), np.where(ok, t, 0).astype(np.int64)
            d = np.asarray(depths[v], np.float32)[py, px]
            ok &= (np.asarray(masks[v])[py, px] != 0) & np.isfinite(d) & (d > 0)
            sdf = d.astype(np.float64) - cam[2]
            ok &= ~(sdf < -trunc)
            f = np.minimum(1.0, sdf / trunc)
            sum_f = np.where(ok, sum_f + f, sum_f)
            w += ok
            near = ok & (sdf <= trunc)
            col += np.where(near[..., None], np.asarray(images[v])[py, px].astype(np.int64), 0)
            c += near
        tsdf = np.where(w > 0, sum_f / np.maximum(w, 1), 1.0).astype(np.float32)
    rgb = np.where(c[..., None] > 0, (2 * col + c[..., None]) // np.maximum(2 * c[..., None], 1), 0).astype(np.uint8)
    return tsdf, w.astype(np.int32), rgb, (c > 0).astype(np.uint8)


def _bits(d):
    return d & 1, (d >> 1) & 1, (d >> 2) & 1


def _shifted(a, d, fill):
    """b[k,j,i] = a[k+dz, j+dy, i+dx], ``fill`` outside"""
    dx, dy, dz = d
    out = np.full(a.shape, fill, a.dtype)
    nz, ny, nx = a.shape
    src = a[max(dz, 0):nz + min(dz, 0), max(dy, 0):ny + min(dy, 0), max(dx, 0):nx + min(dx, 0)]
    out[max(-dz, 0):nz + min(-dz, 0), max(-dy, 0):ny + min(-dy, 0), max(-dx, 0):nx + min(-dx, 0)] = src
    return out


def _sign(p):
    """The sign of a permutation of 0 .. n-1"""
    return (-1) ** sum(1 for a in range(len(p)) for b in range(a + 1, len(p)) if p[a] > p[b])


# the six tetrahedra in the definition's order: corner offsets (v0, v1, v2, v3) and the sign of det[e_a e_b e_c]
TETS = []
for perm in itertools.permutations(range(3)):                                   # lexicographic: xyz xzy yxz yzx zxy zyx
    a, b, _ = perm
    axes = np.eye(3)[list(perm)]
    TETS.append(((0, 1 << a, (1 << a) | (1 << b), 7), int(round(np.linalg.det(axes)))))


def tet_triangles(inside, det):
    """inside: 4 booleans of (v0 .. v3) -> the triangles as tuples of three (p, q) corner pairs, p < q, counter-clockwise seen
    from the outside corners, by the parity rule: with v_i alone inside, j the least other corner and (i, j, k, l) an even
    permutation, (ij, ik, il); alone outside: k and l exchanged; i < j inside and (i, j, k, l) even: the quadrilateral
    (ik, il, jl, jk), cut along its first and third corner.  A mirrored tetrahedron (det < 0) turns every triangle round."""
    ins = [p for p in range(4) if inside[p]]
    outs = [p for p in range(4) if not inside[p]]
    e = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        i, j = ins
        k, l = outs if _sign((i, j) + tuple(outs)) > 0 else outs[::-1]
        quad = [e(i, k), e(i, l), e(j, l), e(j, k)]
        tris = [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    else:
        lone, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
        j, k, l = rest
        if (_sign((lone, j, k, l)) > 0) != (len(ins) == 1):
            k, l = l, k
        tris = [(e(lone, j), e(lone, k), e(lone, l))]
    return [(t[0], t[2], t[1]) for t in tris] if det < 0 else tris


def extract_numpy(tsdf, weight, rgb, has_color, origin, voxel, dims, min_weight):
    """-> vertices [Nv,3] float32, colors [Nv,3] uint8, triangles [Nt,3] int32, owners [Nv,2] int64 (owner node, d)"""
    nx, ny, nz = dims
    f = np.asarray(tsdf, np.float32).reshape(nz, ny, nx)
    known = np.asarray(weight).reshape(nz, ny, nx) >= min_weight
    inside = f < 0
    valid = np.ones((nz, ny, nx), bool)                                         # indexed by the cell's lowest node
    for c in range(8):
        valid &= _shifted(known, _bits(c), False)
    has = np.zeros((nz, ny, nx, 8), bool)
    for d in range(1, 8):
        any_cell = np.zeros((nz, ny, nx), bool)
        for s in range(8):
            if s & d == 0:
                any_cell |= _shifted(valid, tuple(-b for b in _bits(s)), False)
        has[..., d] = any_cell & (_shifted(inside, _bits(d), False) != inside) & _shifted(np.ones_like(inside), _bits(d), False)
    kk, jj, ii, dd = np.nonzero(has)                                            # row major: node index, then d
    owner = ii + nx * (jj + ny * kk)
    number = {(int(n), int(d)): r for r, (n, d) in enumerate(zip(owner, dd))}
    di, dj, dk = _bits(dd)
    fa, fb = f[kk, jj, ii].astype(np.float64), f[kk + dk, jj + dj, ii + di].astype(np.float64)
    with np.errstate(all="ignore"):
        t = fa / (fa - fb)
        xs, ys, zs = node_coords(origin, voxel, dims)
        pos = np.stack([xs[ii] + t * (xs[ii + di] - xs[ii]), ys[jj] + t * (ys[jj + dj] - ys[jj]),
                        zs[kk] + t * (zs[kk + dk] - zs[kk])], 1).astype(np.float32)
        col = np.asarray(rgb, np.uint8).reshape(nz, ny, nx, 3).astype(np.float64)
        hc = np.asarray(has_color).reshape(nz, ny, nx) != 0
        ha, hb = hc[kk, jj, ii], hc[kk + dk, jj + dj, ii + di]
        ca, cb = col[kk, jj, ii], col[kk + dk, jj + dj, ii + di]
        ca, cb = np.where(ha[:, None], ca, cb), np.where(hb[:, None], cb, ca)
        none = ~(ha | hb)
        ca[none], cb[none] = 0, 0
        colors = np.clip(np.floor(ca + t[:, None] * (cb - ca) + 0.5), 0, 255).astype(np.uint8)
    tris = []
    mixed = valid.copy()
    all_in, all_out = np.ones_like(valid), np.ones_like(valid)
    for c in range(8):
        s = _shifted(inside, _bits(c), False)
        all_in &= s
        all_out &= ~s
    mixed &= ~(all_in | all_out)
    for k, j, i in zip(*np.nonzero(mixed)):                                     # row major: cell index order
        for corners, det in TETS:
            nodes = [(i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)) for c in corners]
            ins = [bool(inside[n[2], n[1], n[0]]) for n in nodes]
            for tri in tet_triangles(ins, det):
                row = []
                for p, q in tri:
                    a = nodes[p]
                    row.append(number[(int(a[0] + nx * (a[1] + ny * a[2])), corners[q] ^ corners[p])])
                tris.append(row)
    return pos, colors, np.asarray(tris, np.int32).reshape(-1, 3), np.stack([owner, dd], 1).astype(np.int64).reshape(-1, 2)


# ---- the host build of mvster_amd/csrc/tsdf_math.h ----------------------------------------------------------------------------------

_HM = {}


def load_tsdf_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/tsdf_hostmath.cpp with the flags of ``fusion_scene_cases.load_geo_hostmath`` and load it, once per
    process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of tsdf_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libtsdfhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "tsdf_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, i, d = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double
    h.hm_tsdf_grid_ok.restype, h.hm_tsdf_grid_ok.argtypes = i, [l, l, l]
    h.hm_tsdf_integrate.restype, h.hm_tsdf_integrate.argtypes = None, [p, p, p, p, i, i, i, d, d, d, d, i, i, i, d, p, p, p, p]
    h.hm_tsdf_count.restype, h.hm_tsdf_count.argtypes = None, [p, p, i, i, i, i, p, p, p]
    h.hm_tsdf_emit.restype, h.hm_tsdf_emit.argtypes = None, [p, p, p, p, d, d, d, d, i, i, i, i, p, p, p, p, p, p]
    _HM[compilers] = h
    return h


def views_table(Ks, Es):
    """-> [V,21] float64: K, R, t (what mesh._cameras builds)"""
    return np.stack([np.concatenate([np.asarray(K, np.float64).reshape(-1), np.asarray(E, np.float64)[:3, :3].reshape(-1),
                                     np.asarray(E, np.float64)[:3, 3]]) for K, E in zip(Ks, Es)])


def integrate_host(h, depths, masks, images, Ks, Es, origin, voxel, dims, trunc):
    depth = np.ascontiguousarray(depths, np.float32)
    mask = np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)
    img = np.ascontiguousarray(images, np.uint8)
    views = np.ascontiguousarray(views_table(Ks, Es))
    V, H, W = depth.shape
    nx, ny, nz = dims
    tsdf, weight = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.int32)
    rgb, has = np.zeros((nz, ny, nx, 3), np.uint8), np.zeros((nz, ny, nx), np.uint8)
    h.hm_tsdf_integrate(depth.ctypes.data, mask.ctypes.data, img.ctypes.data, views.ctypes.data, V, H, W, *[float(o) for o in origin],
                        float(voxel), nx, ny, nz, float(trunc), tsdf.ctypes.data, weight.ctypes.data, rgb.ctypes.data, has.ctypes.data)
    return tsdf, weight, rgb, has


def extract_host(h, tsdf, weight, rgb, has_color, origin, voxel, dims, min_weight):
    """-> vertices, colors, triangles, owners as ``extract_numpy``"""
    nx, ny, nz = dims
    f, w = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.int32)
    c, hc = np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(has_color, np.uint8)
    n = nx * ny * nz
    edge_mask, vbase, counts = np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(2, np.int64)
    h.hm_tsdf_count(f.ctypes.data, w.ctypes.data, nx, ny, nz, int(min_weight), edge_mask.ctypes.data, vbase.ctypes.data, counts.ctypes.data)
    nv, nt = int(counts[0]), int(counts[1])
    vertices, colors = np.full((nv, 3), np.nan, np.float32), np.full((nv, 3), 0xCD, np.uint8)
    owners, triangles = np.full((nv, 2), -1, np.int64), np.full((nt, 3), -1, np.int32)
    h.hm_tsdf_emit(f.ctypes.data, w.ctypes.data, c.ctypes.data, hc.ctypes.data, *[float(o) for o in origin], float(voxel), nx, ny, nz,
                   int(min_weight), edge_mask.ctypes.data, vbase.ctypes.data, vertices.ctypes.data, colors.ctypes.data,
                   owners.ctypes.data, triangles.ctypes.data)
    return vertices, colors, triangles, owners


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """-> E [4,4] world -> camera, z forward, x right, y down"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    if abs(fwd @ up) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    E = np.eye(4)
    E[:3, :3] = np.stack([right, down, fwd])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def pinhole(f, H, W, skew=0.0):
    return np.array([[f, skew, W / 2 - 0.3], [0.0, f * 1.02, H / 2 + 0.2], [0.0, 0.0, 1.0]])


def sphere_depth(K, E, H, W, centre, radius):
    """Analytic z-depth of the sphere along every pixel's ray, 0 where the ray misses"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rays = np.linalg.solve(K, np.stack([x.ravel(), y.ravel(), np.ones(H * W)]))     # z component 1
    cc = E[:3, :3] @ np.asarray(centre, np.float64) + E[:3, 3]
    a, b = (rays * rays).sum(0), rays.T @ cc
    disc = b * b - a * (cc @ cc - radius * radius)
    with np.errstate(invalid="ignore"):
        s = (b - np.sqrt(disc)) / a
    return np.where((disc >= 0) & (s > 0), s, 0.0).reshape(H, W).astype(np.float32)


def image(h, w, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127.5 + 90.0 * np.sin(x[..., None] * (0.21 + 0.05 * np.arange(3)) + seed) * np.cos(y[..., None] * (0.17 + 0.04 * np.arange(3)))
    return np.clip(base + rng.randint(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)


def sphere_volume(dims, origin, voxel, centre_nodes, radius_nodes, trunc_nodes=4.0, seed=0):
    """An exact signed-distance sphere sampled on the grid (clamped at the truncation), weight 1, seeded colours"""
    xs, ys, zs = node_coords(origin, voxel, dims)
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    centre = np.asarray(origin, np.float64) + voxel * np.asarray(centre_nodes, np.float64)
    dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius_nodes * voxel
    rng = np.random.RandomState(seed)
    nx, ny, nz = dims
    return dict(tsdf=np.clip(dist / (trunc_nodes * voxel), -1.0, 1.0).astype(np.float32), weight=np.ones((nz, ny, nx), np.int32),
                rgb=rng.randint(0, 256, size=(nz, ny, nx, 3)).astype(np.uint8), has_color=(rng.rand(nz, ny, nx) > 0.2).astype(np.uint8),
                origin=tuple(origin), voxel=voxel, dims=tuple(dims), min_weight=1, centre=centre, radius=radius_nodes * voxel,
                trunc=trunc_nodes * voxel)


def random_volume(dims, seed, min_weight=1, zero_share=0.0):
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    f = rng.uniform(-1, 1, size=(nz, ny, nx)).astype(np.float32)
    if zero_share:
        f[rng.rand(nz, ny, nx) < zero_share] = 0.0
    return dict(tsdf=f, weight=rng.randint(0, 4, size=(nz, ny, nx)).astype(np.int32),
                rgb=rng.randint(0, 256, size=(nz, ny, nx, 3)).astype(np.uint8), has_color=(rng.rand(nz, ny, nx) > 0.3).astype(np.uint8),
                origin=(0.3 * seed, -1.7, 2.9), voxel=0.013 * (seed + 1), dims=tuple(dims), min_weight=min_weight)


SPHERE_DIMS, SPHERE_VOXEL, SPHERE_ORIGIN = (16, 15, 14), 0.37, (-1.3, 0.7, 2.1)
SPHERE_CENTRE_NODES, SPHERE_RADIUS_NODES = (7.3, 6.9, 6.6), 5.0


def _zero_plane():
    """tsdf = (k - 3) / 4 exactly: the nodes of layer 3 are exactly 0 (outside), every crossing vertex coincides with one"""
    v = random_volume((6, 5, 7), 5)
    v["tsdf"] = np.broadcast_to(((np.arange(7, dtype=np.float32) - 3) / 4)[:, None, None], (7, 5, 6)).copy()
    v["weight"][:] = 1
    return v


def _all_outside():
    v = random_volume((9, 4, 3), 6)
    v["tsdf"] = np.abs(v["tsdf"]) + np.float32(0.01)
    v["weight"][:] = 2
    return v


@functools.lru_cache(None)
def volume_cases():
    """name -> a volume written directly (tsdf, weight, rgb, has_color, origin, voxel, dims, min_weight)"""
    return {
        "sphere_inside": sphere_volume(SPHERE_DIMS, SPHERE_ORIGIN, SPHERE_VOXEL, SPHERE_CENTRE_NODES, SPHERE_RADIUS_NODES),
        "sphere_cut": sphere_volume(SPHERE_DIMS, SPHERE_ORIGIN, SPHERE_VOXEL, (3.2, 6.9, 11.4), SPHERE_RADIUS_NODES, seed=1),
        "holes": dict(sphere_volume(SPHERE_DIMS, SPHERE_ORIGIN, SPHERE_VOXEL, SPHERE_CENTRE_NODES, SPHERE_RADIUS_NODES, seed=2),
                      weight=np.random.RandomState(3).randint(0, 4, size=SPHERE_DIMS[::-1]).astype(np.int32), min_weight=2),
        "grid_2x2x2": dict(random_volume((2, 2, 2), 1), weight=np.ones((2, 2, 2), np.int32)),
        "grid_13x7x5": random_volume((13, 7, 5), 2, min_weight=1),
        "grid_65x3x3": random_volume((65, 3, 3), 3, min_weight=1),
        "grid_257x2x3": random_volume((257, 2, 3), 4, min_weight=1),
        "no_sign_change": _all_outside(),
        "exact_zero_plane": _zero_plane(),
        "exact_zero_random": random_volume((11, 6, 5), 7, min_weight=1, zero_share=0.15),
    }


def _bad_depth_maps():
    """Depth maps with NaN, +-inf, 0 and negative values and masked pixels; one camera behind which part of the grid lies and one
    that looks away from it"""
    H, W, dims, voxel, origin = 40, 56, (13, 7, 5), 0.21, (-1.2, -0.7, 1.6)
    centre = np.asarray(origin) + voxel * (np.asarray(dims) - 1) / 2
    K = pinhole(48.0, H, W, skew=0.4)
    Es = [look_at(centre + (0.0, 0.0, -2.5), centre, up=(0, 1, 0)), look_at(centre + (2.0, 0.3, -1.0), centre, up=(0, 1, 0)),
          look_at(centre + (0.3, 0.0, 0.0), centre + (3.0, 0.0, 0.0), up=(0, 1, 0)),       # inside the grid: nodes behind it
          look_at(centre + (0.0, 0.0, -2.5), centre + (0.0, 0.0, -9.0), up=(0, 1, 0))]     # looks away: no node in its image
    rng = np.random.RandomState(11)
    depths = rng.uniform(1.8, 3.2, size=(4, H, W)).astype(np.float32)
    depths[2] = rng.uniform(0.2, 1.5, size=(H, W))
    bad = rng.rand(4, H, W)
    for lo, value in ((0.00, np.nan), (0.05, np.inf), (0.10, -np.inf), (0.15, 0.0), (0.20, -1.5)):
        depths[(bad >= lo) & (bad < lo + 0.05)] = value
    masks = rng.rand(4, H, W) > 0.15
    images = np.stack([image(H, W, s) for s in range(4)])
    return dict(depths=depths, masks=masks, images=images, Ks=[K] * 4, Es=Es, origin=origin, voxel=voxel, dims=dims,
                trunc=4 * voxel, min_weight=1)


def _sphere_maps():
    """Six views of 48 x 64 around the sphere of ``sphere_inside`` with analytic ray-sphere z-depths"""
    H, W = 48, 64
    v = volume_cases()["sphere_inside"]
    K = pinhole(52.0, H, W)
    Es = [look_at(v["centre"] + 6.0 * np.asarray(d, np.float64), v["centre"]) for d in
          ((1, 0.05, 0.1), (-1, 0.1, -0.05), (0.05, 1, 0.1), (0.1, -1, 0.05), (0.05, 0.1, 1), (0.1, -0.05, -1))]
    depths = np.stack([sphere_depth(K, E, H, W, v["centre"], v["radius"]) for E in Es])
    return dict(depths=depths, masks=depths > 0, images=np.stack([image(H, W, 20 + s) for s in range(6)]), Ks=[K] * 6, Es=Es,
                origin=v["origin"], voxel=v["voxel"], dims=v["dims"], trunc=4 * v["voxel"], min_weight=1, centre=v["centre"],
                radius=v["radius"])


PLANE_DEPTH, PLANE_COLOUR = 2.5, (200, 40, 97)


def _plane_maps(dims=(12, 9, 10)):
    """One view looking along +z at the plane z = PLANE_DEPTH with a constant image"""
    H, W, voxel = 48, 64, 0.05
    origin = (-0.27, -0.21, PLANE_DEPTH - 4.6 * voxel)
    K = pinhole(60.0, H, W)
    img = np.empty((1, H, W, 3), np.uint8)
    img[...] = PLANE_COLOUR
    return dict(depths=np.full((1, H, W), PLANE_DEPTH, np.float32), masks=np.ones((1, H, W), bool), images=img, Ks=[K], Es=[np.eye(4)],
                origin=origin, voxel=voxel, dims=dims, trunc=4 * voxel, min_weight=1)


@functools.lru_cache(None)
def map_cases():
    """name -> the maps of a scan and a grid (depths, masks, images, Ks, Es, origin, voxel, dims, trunc, min_weight)"""
    wide = _plane_maps((65, 3, 10))
    wide["origin"] = (-0.8, -0.05, wide["origin"][2])
    return {"sphere_views": _sphere_maps(), "plane": _plane_maps(), "plane_65": wide, "bad_depths": _bad_depth_maps()}


GRID_KEYS = ("origin", "voxel", "dims")


@functools.lru_cache(None)
def host_volume(name):
    """The host build's volume of a map case -> dict like a volume case"""
    c = map_cases()[name]
    tsdf, weight, rgb, has = integrate_host(load_tsdf_hostmath(), *(c[k] for k in ("depths", "masks", "images", "Ks", "Es", "origin",
                                                                                    "voxel", "dims", "trunc")))
    return dict(c, tsdf=tsdf, weight=weight, rgb=rgb, has_color=has)


def all_volumes():
    """name -> volume: the direct ones and the host build's volumes of the map cases"""
    out = dict(volume_cases())
    out.update((name, host_volume(name)) for name in map_cases())
    return out


@functools.lru_cache(None)
def host_mesh(name):
    """The host build's mesh of a volume (computed once, shared by the tests) -> vertices, colors, triangles, owners"""
    v = all_volumes()[name]
    return extract_host(load_tsdf_hostmath(), v["tsdf"], v["weight"], v["rgb"], v["has_color"], v["origin"], v["voxel"], v["dims"],
                        v["min_weight"])


def assert_bytes(g, w, what=""):
    g, w = np.asarray(g), np.asarray(w)
    assert g.dtype.itemsize == w.dtype.itemsize and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.nonzero(np.frombuffer(g.tobytes(), np.uint8) != np.frombuffer(w.tobytes(), np.uint8))[0]
        k = int(bad[0]) // g.dtype.itemsize
        raise AssertionError((what, "%d bytes differ, the first in element %d: %r against %r" % (len(bad), k, g.ravel()[k], w.ravel()[k])))
