"""Shared by tests/test_mesh_clean_cpu.py and tests/test_gpu_mesh_clean.py (not a test module): the cases, mesh cleaning (DESIGN.md
section 4.24) restated in NumPy, and the host build of mvster_amd/csrc/mesh_math.h.

Neither yardstick comes from the reference tree, which has no such step, nor from Open3D or SciPy.  The restatement is plain NumPy
and goes another way than the header: coinciding vertices are found by sorting the rows (np.unique), not by hashing; components
by label propagation to a fixed point, not by union-find; a vertex's normal sum by rounds over the sorted (vertex, triangle)
pairs, not by walking the triangles.  Its float64 operations are NumPy's own in the order the definition gives, so it can be
compared byte for byte.  The host build is the kernels' own arithmetic and the header's serial host forms compiled for the CPU."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

from tests import fusion_scene_cases as C
from tests import mesh_cases as M

# ---- the definition, restated in NumPy ----------------------------------------------------------------------------------------------


def weld_numpy(vertices, weld=True):
    """-> canon [Nv] int32"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    canon = np.arange(len(v), dtype=np.int64)
    if not weld or not len(v):
        return canon.astype(np.int32)
    finite = np.isfinite(v).all(1)
    idx = np.nonzero(finite)[0]
    rows = v[idx] + np.float32(0.0)                                             # -0.0 + 0.0 = +0.0: equal floats, equal bits
    _, inverse = np.unique(rows.view(np.uint32), axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    first = np.full(inverse.max() + 1 if len(idx) else 0, len(v), np.int64)
    np.minimum.at(first, inverse, idx)
    canon[idx] = first[inverse]
    return canon.astype(np.int32)


def dropped_numpy(vertices, corners):
    """corners [Nt,3]: canonical -> bool [Nt]"""
    a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    bad = (a == b) | (a == c) | (b == c)
    if vertices is not None:
        finite = np.isfinite(np.asarray(vertices, np.float32).reshape(-1, 3)).all(1)
        bad |= ~finite[corners].all(1)
    return bad


def components_numpy(vertices, triangles, n_vertices, canon=None):
    """-> labels [Nv], tri_labels [Nt], tri_component [Nt], roots, n_vertices, n_triangles [C] (int32)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    canon = np.arange(n_vertices) if canon is None else np.asarray(canon, np.int64)
    corners = canon[t] if len(t) else t
    kept = ~dropped_numpy(vertices, corners)
    k = corners[kept]
    low = np.arange(n_vertices, dtype=np.int64)                                # the least vertex known to be connected to v
    while True:
        m = low[k].min(1) if len(k) else np.zeros(0, np.int64)
        nxt = low.copy()
        np.minimum.at(nxt, k.reshape(-1), np.repeat(m, 3))
        nxt = nxt[nxt]                                                          # (a shortcut: low[low[v]] is connected to v too)
        if (nxt == low).all():
            break
        low = nxt
    used = np.zeros(n_vertices, bool)
    used[k.reshape(-1)] = True
    labels = np.where(used, low, -1)
    tri_labels = np.full(len(t), -1, np.int64)
    tri_labels[kept] = labels[k[:, 0]] if len(k) else 0
    roots = np.nonzero(labels == np.arange(n_vertices))[0]
    rank = np.full(n_vertices, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    tri_component = np.where(tri_labels >= 0, rank[np.maximum(tri_labels, 0)], -1) if n_vertices else tri_labels.copy()
    nv = np.bincount(rank[labels[used]], minlength=len(roots))
    nt = np.bincount(tri_component[kept], minlength=len(roots))
    i32 = lambda a: np.asarray(a, np.int32)
    return dict(labels=i32(labels), tri_labels=i32(tri_labels), tri_component=i32(tri_component), roots=i32(roots), n_vertices=i32(nv),
                n_triangles=i32(nt))


def normals_numpy(vertices, triangles):
    """-> normals [Nv,3] float32, valid [Nv] uint8"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    N = np.zeros((len(v), 3))
    with np.errstate(all="ignore"):
        e1, e2 = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        vert, tri = t.reshape(-1), np.repeat(np.arange(len(t)), 3)
        order = np.lexsort((tri, vert))                                         # by vertex, then ascending triangle
        vert, tri = vert[order], tri[order]
        start = np.r_[0, np.nonzero(np.diff(vert))[0] + 1] if len(vert) else np.zeros(0, np.int64)
        place = np.arange(len(vert)) - np.repeat(start, np.diff(np.r_[start, len(vert)]))
        for r in range(int(place.max()) + 1 if len(place) else 0):              # round r: every vertex adds its r-th triangle
            sel = place == r
            N[vert[sel]] = N[vert[sel]] + n[tri[sel]]
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        valid = (length > 0) & np.isfinite(length)
        normals = np.where(valid[:, None], N / np.where(valid, length, 1.0)[:, None], 0.0).astype(np.float32)
    return normals, valid.astype(np.uint8)


def clean_numpy(vertices, colors, triangles, weld=True, min_triangles=0, largest_only=False, normals=False):
    """-> dict like mesh.clean_mesh (arrays; stats as there)"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int32).reshape(-1, 3)
    canon = weld_numpy(v, weld).astype(np.int64)
    comp = components_numpy(v, t, len(v), canon)
    nt = comp["n_triangles"].astype(np.int64)
    keep = nt >= min_triangles
    if largest_only and len(nt):
        best = np.lexsort((comp["roots"], -nt))[0]                              # the most triangles, then the smallest root
        keep &= np.arange(len(nt)) == best
    tkeep = (comp["tri_component"] >= 0) & keep[np.maximum(comp["tri_component"], 0)] if len(nt) else np.zeros(len(t), bool)
    rank = np.full(len(v), -1, np.int64)
    rank[comp["roots"]] = np.arange(len(nt))
    vkeep = (comp["labels"] >= 0) & keep[rank[np.maximum(comp["labels"], 0)]] if len(nt) else np.zeros(len(v), bool)
    number = np.cumsum(vkeep) - 1
    out = dict(vertices=v[vkeep], colors=None if colors is None else np.asarray(colors, np.uint8)[vkeep],
               triangles=number[canon[t[tkeep]]].astype(np.int32).reshape(-1, 3), vertex_index=np.nonzero(vkeep)[0].astype(np.int64),
               triangle_index=np.nonzero(tkeep)[0].astype(np.int64),
               stats=dict(welded=int((canon != np.arange(len(v))).sum()), degenerate=int((comp["tri_labels"] < 0).sum()),
                          components=len(nt), components_kept=int(keep.sum()), triangles_removed=int(len(t) - tkeep.sum()),
                          vertices_removed=int(len(v) - vkeep.sum())))
    if normals:
        out["normals"], out["normals_valid"] = normals_numpy(out["vertices"], out["triangles"])
    return out


# ---- the host build of mvster_amd/csrc/mesh_math.h ----------------------------------------------------------------------------------

_HM = {}


def load_mesh_clean_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/mesh_clean_hostmath.cpp with the flags of ``fusion_scene_cases.load_geo_hostmath`` and load it, once
    per process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of mesh_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libmeshcleanhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "mesh_clean_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, i = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    h.hm_mesh_weld.restype, h.hm_mesh_weld.argtypes = None, [p, l, i, p]
    h.hm_mesh_components.restype, h.hm_mesh_components.argtypes = l, [p, p, l, l, p, p, p, p, p, p, p]
    h.hm_mesh_clean.restype, h.hm_mesh_clean.argtypes = None, [p, p, p, l, l, i, l, i, p, p, p, p, p, p]
    h.hm_mesh_normals.restype, h.hm_mesh_normals.argtypes = None, [p, p, l, l, p, p]
    h.hm_mesh_sort_row.restype, h.hm_mesh_sort_row.argtypes = None, [p, l]
    _HM[compilers] = h
    return h


def _ptr(a):
    return None if a is None else a.ctypes.data


def components_host(h, vertices, triangles, n_vertices, canon=None):
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    v = None if vertices is None else np.ascontiguousarray(vertices, np.float32)
    cn = None if canon is None else np.ascontiguousarray(canon, np.int32)
    rows = min(n_vertices, len(t))
    labels, tl, tc = np.full(n_vertices, -7, np.int32), np.full(len(t), -7, np.int32), np.full(len(t), -7, np.int32)
    table = np.full((3, rows), -7, np.int32)
    n = h.hm_mesh_components(_ptr(v), t.ctypes.data, n_vertices, len(t), _ptr(cn), labels.ctypes.data, tl.ctypes.data, tc.ctypes.data,
                             table[0].ctypes.data, table[1].ctypes.data, table[2].ctypes.data)
    return dict(labels=labels, tri_labels=tl, tri_component=tc, roots=table[0, :n].copy(), n_vertices=table[1, :n].copy(),
                n_triangles=table[2, :n].copy())


def normals_host(h, vertices, triangles):
    v, t = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    normals, valid = np.full((len(v), 3), np.nan, np.float32), np.full(len(v), 0xCD, np.uint8)
    h.hm_mesh_normals(v.ctypes.data, t.ctypes.data, len(v), len(t), normals.ctypes.data, valid.ctypes.data)
    return normals, valid


def clean_host(h, vertices, colors, triangles, weld=True, min_triangles=0, largest_only=False, normals=False):
    """-> dict like mesh.clean_mesh (arrays)"""
    v, t = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, np.uint8)
    ov, oc, ot = np.zeros((len(v), 3), np.float32), None if c is None else np.zeros((len(v), 3), np.uint8), np.zeros((len(t), 3), np.int32)
    vi, ti, stats = np.zeros(len(v), np.int64), np.zeros(len(t), np.int64), np.zeros(6, np.int64)
    h.hm_mesh_clean(v.ctypes.data, _ptr(c), t.ctypes.data, len(v), len(t), int(weld), int(min_triangles), int(largest_only),
                    ov.ctypes.data, _ptr(oc), ot.ctypes.data, vi.ctypes.data, ti.ctypes.data, stats.ctypes.data)
    nv, nt = int(stats[0]), int(stats[1])
    out = dict(vertices=ov[:nv].copy(), colors=None if c is None else oc[:nv].copy(), triangles=ot[:nt].copy(), vertex_index=vi[:nv].copy(),
               triangle_index=ti[:nt].copy(),
               stats=dict(welded=len(v) - int(stats[3]), degenerate=int(stats[4]), components=int(stats[2]), components_kept=int(stats[5]),
                          triangles_removed=len(t) - nt, vertices_removed=len(v) - nv))
    if normals:
        out["normals"], out["normals_valid"] = normals_host(h, out["vertices"], out["triangles"])
    return out


CLEAN_KEYS = ("vertices", "colors", "triangles", "vertex_index", "triangle_index")
COMPONENT_KEYS = ("labels", "tri_labels", "tri_component", "roots", "n_vertices", "n_triangles")


def assert_clean_equal(got, want, what=""):
    """Two results of a clean-up (dicts of arrays), byte for byte"""
    for k in CLEAN_KEYS + (("normals", "normals_valid") if "normals" in want else ()):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            M.assert_bytes(got[k], want[k], (what, k))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


# ---- facts about a mesh ---------------------------------------------------------------------------------------------------------------

def closed_and_oriented(triangles):
    """Every directed edge once, and its reverse once"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = e[:, 0] * (t.max() + 1 if len(t) else 1) + e[:, 1]
    rev = e[:, 1] * (t.max() + 1 if len(t) else 1) + e[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


def euler(n_vertices, triangles):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return n_vertices - len(np.unique(e, axis=0)) + len(t)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def node_sphere_volume():
    """A closed sphere whose surface passes through grid nodes (30 nodes with tsdf exactly 0)"""
    return M.sphere_volume((16, 16, 16), (0, 0, 0), 1.0, (8, 8, 8), 5.0)


def two_spheres_volume():
    """Two disjoint spheres: the minimum of two sphere tsdfs"""
    a = M.sphere_volume((24, 12, 12), (0, 0, 0), 1.0, (6, 6, 6), 4.0)
    b = M.sphere_volume((24, 12, 12), (0, 0, 0), 1.0, (17, 6, 6), 2.5)
    return dict(a, tsdf=np.minimum(a["tsdf"], b["tsdf"]))


def extra_volumes():
    return {"node_sphere": node_sphere_volume(), "two_spheres": two_spheres_volume()}


@functools.lru_cache(None)
def extracted(name):
    """The host build's mesh of a volume of mesh_cases or of ``extra_volumes`` -> vertices, colors, triangles"""
    if name in extra_volumes():
        v = extra_volumes()[name]
        return M.extract_host(M.load_tsdf_hostmath(), v["tsdf"], v["weight"], v["rgb"], v["has_color"], v["origin"], v["voxel"], v["dims"],
                              v["min_weight"])[:3]
    return M.host_mesh(name)[:3]


def extracted_names():
    return sorted(M.volume_cases()) + sorted(M.map_cases()) + sorted(extra_volumes())


def _colors(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3)).astype(np.uint8)


def random_mesh(nv, nt, seed):
    """nv vertices on a small integer lattice (so about half of them coincide with another) and nt triangles of random indices
    (some name a vertex twice)"""
    rng = np.random.RandomState(seed)
    side = max(2, int(round((nv / 2.0) ** (1.0 / 3.0))))
    v = rng.randint(0, side, size=(nv, 3)).astype(np.float32) * np.float32(0.37)
    t = rng.randint(0, max(nv, 1), size=(nt, 3)).astype(np.int32)
    return v, _colors(nv, seed + 1), t


SCAN_TILE = 1024 * 16                                                           # the single-workgroup scan takes this many counts a pass


@functools.lru_cache(None)
def hand_meshes():
    """name -> (vertices [Nv,3] float32, colors [Nv,3] uint8, triangles [Nt,3] int32): the sizes and shapes at which the kernels
    could go wrong"""
    out = {}
    rng = np.random.RandomState(42)
    # a strip under a permutation of the vertex numbers: long chains, hooks in both directions across workgroups
    n = 5000
    perm = rng.permutation(n + 2).astype(np.int32)
    pos = np.stack([np.arange(n + 2) * 0.5, (np.arange(n + 2) % 2) * 1.0, np.sin(np.arange(n + 2) * 0.01)], 1).astype(np.float32)
    v = np.empty_like(pos)
    v[perm] = pos
    out["strip_5000"] = (v, _colors(n + 2, 1), perm[np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)].astype(np.int32))
    # a fan around one vertex: one hot counter and a long row to put in order
    n = 3000
    ang = np.arange(n + 1) * (2 * np.pi / (n + 1))
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.3]], rim]).astype(np.float32)
    out["fan_3000"] = (v, _colors(n + 2, 2), np.stack([np.zeros(n, np.int64), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32))
    # separate triangles: a component table of many rows
    for n in (2000, 6000):
        v = rng.uniform(-5, 5, size=(3 * n, 3)).astype(np.float32)
        out["separate_%d" % n] = (v, _colors(3 * n, 3), rng.permutation(3 * n).astype(np.int32).reshape(n, 3))
    # 300 vertices at one position and 300 at its negative-zero twin, welded into one
    v = np.concatenate([np.tile(np.float32([0.0, 1.5, 0.0]), (300, 1)), np.tile(np.float32([-0.0, 1.5, -0.0]), (300, 1)),
                        rng.uniform(-1, 1, size=(6, 3)).astype(np.float32)])
    k = np.arange(600)
    out["coincident_600"] = (v, _colors(606, 4), np.stack([k[::-1], 600 + k % 5, 601 + k % 5], 1).astype(np.int32))
    # vertices no triangle names, before, between and behind the used ones
    v = rng.uniform(-1, 1, size=(12, 3)).astype(np.float32)
    out["unused_vertices"] = (v, _colors(12, 5), np.int32([[2, 3, 5], [3, 2, 7], [9, 7, 5], [2, 5, 7]]))
    # triangles that name a vertex twice or three times in the input
    v = rng.uniform(-1, 1, size=(9, 3)).astype(np.float32)
    out["repeated_indices"] = (v, _colors(9, 6), np.int32([[0, 0, 1], [1, 2, 3], [4, 5, 4], [6, 7, 7], [8, 8, 8], [3, 2, 4], [5, 6, 7]]))
    # NaN and +-inf coordinates: such a vertex welds with nothing, its triangles are dropped
    v = rng.randint(0, 3, size=(40, 3)).astype(np.float32)
    v[3], v[4], v[11], v[12], v[20], v[21] = [np.nan, 0, 0], [np.nan, 0, 0], [1, np.inf, 2], [1, np.inf, 2], [0, 1, -np.inf], [np.nan] * 3
    out["not_finite"] = (v, _colors(40, 7), rng.randint(0, 40, size=(120, 3)).astype(np.int32))
    # two tetrahedra of the same size: the tie of largest_only goes to the smaller root
    v = rng.uniform(-1, 1, size=(8, 3)).astype(np.float32)
    tet = np.int32([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    out["two_tetrahedra"] = (v, _colors(8, 8), np.concatenate([tet + 4, tet]).astype(np.int32))
    # sizes around the workgroup, and 16 385 (65 workgroups: the scan itself stays inside its first pass, see tile_crossing_mesh)
    for nv, nt in ((1, 1), (1, 257), (255, 257), (256, 256), (257, 255), (257, 1), (SCAN_TILE + 1, SCAN_TILE + 1)):
        out["random_%dx%d" % (nv, nt)] = random_mesh(nv, nt, 100 + nv + nt)
    return out


TILE_CROSSING_TRIANGLES = 1600000


@functools.lru_cache(None)
def tile_crossing_mesh():
    """The one mesh that takes the scans past their first pass.  The kernels scan one count per workgroup of 256 vertices or
    triangles and the single-workgroup scan takes SCAN_TILE counts a pass, so that needs more than SCAN_TILE * 256 = 4 194 304
    vertices, in the input (the roots, the kept vertices and triangles) and in the cleaned mesh (the normals' rows): 1.6 M
    triangles over 4.8 M vertices under a seeded permutation of the vertex numbers, every fourth triangle sharing a vertex with
    the one before it (so components have 1 or 2 triangles and 400 000 vertices are unused).  Not in ``all_meshes``: the GPU test
    runs it under two settings, the CPU tests leave it alone.  -> (vertices, colors, triangles)"""
    n = TILE_CROSSING_TRIANGLES
    rng = np.random.RandomState(77)
    t = rng.permutation(3 * n).astype(np.int32).reshape(n, 3)
    t[1::4, 0] = t[0::4, 0]
    v = rng.uniform(-50, 50, size=(3 * n, 3)).astype(np.float32)
    return v, rng.randint(0, 256, size=(3 * n, 3)).astype(np.uint8), t


def all_meshes():
    """name -> (vertices, colors, triangles): every extracted mesh and every hand-built one"""
    out = {name: extracted(name) for name in extracted_names()}
    out.update(hand_meshes())
    return out


SETTINGS = (dict(), dict(weld=False), dict(min_triangles=15), dict(largest_only=True), dict(weld=True, min_triangles=2, largest_only=True))


@functools.lru_cache(None)
def host_clean(name, setting, normals=True):
    """The host build's clean-up of a mesh under SETTINGS[setting] (computed once, shared by the tests)"""
    v, c, t = all_meshes()[name]
    return clean_host(load_mesh_clean_hostmath(), v, c, t, normals=normals, **SETTINGS[setting])
