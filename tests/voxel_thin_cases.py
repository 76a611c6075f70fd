"""Shared by tests/test_voxel_thin_cpu.py and tests/test_gpu_voxel_thin.py (not a test module): voxel-grid thinning
 restated in NumPy, the host build of mvster_amd/csrc/voxel_math.h, and the case clouds.

Neither yardstick comes from the reference tree, which has no thinning: the restatement follows the definition operation by
operation in float64 / int64, the host build is the kernels' own arithmetic compiled for the CPU.  Both are exact, so every
comparison is equality of bytes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from tests import fusion_scene_cases as C

VOXEL_SIZES = (0.2, 0.3, 1.0)
REDUCES = ("mean", "first")
HALF = 1 << 20
KEYS = ("points", "colors", "counts", "first")


# ---- the definition, restated -------------------------------------------------------------------------------------------

def point_terms(points, v):
    """-> (valid [M] bool, i [M,3] int64, t [M,3] int64, key [M] uint64); i, t and key are 0 where invalid."""
    v = np.float64(np.float32(v))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64) / v          # a division, not a reciprocal
        fi = np.floor(q)
        valid = ((fi >= -HALF) & (fi < HALF)).all(1)                                       # NaN and inf fail both
        frac = (q - fi) * 65536.0
    i = np.where(valid[:, None], fi, 0).astype(np.int64)
    t = np.minimum(np.floor(np.where(valid[:, None], frac, 0)).astype(np.int64), 65535)    # the clamp: q - i may round to 1
    key = (((i[:, 0] + HALF) << 42) | ((i[:, 1] + HALF) << 21) | (i[:, 2] + HALF)).astype(np.uint64)
    key[~valid] = 0
    return valid, i, t, key


def thin_numpy(points, colors, v, reduce):
    """The thinning on the CPU: np.unique on the keys, np.add.at in int64 -> dict like fusion.thin_points (NumPy arrays)."""
    assert reduce in REDUCES
    points = np.asarray(points, np.float32).reshape(-1, 3)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    valid, i, t, key = point_terms(points, v)
    idx = np.nonzero(valid)[0]
    uniq, first, inv, n = np.unique(key[idx], return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    f = idx[first]                                       # lowest input index of each voxel
    order = np.argsort(f, kind="stable")                 # output order: increasing f
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    U = len(uniq)
    out = dict(counts=n[order].astype(np.int32), first=f[order].astype(np.int64), dropped=int((~valid).sum()))
    if reduce == "first":
        out["points"], out["colors"] = points[out["first"]].copy(), colors[out["first"]].copy()
        return out
    S, Csum = np.zeros((U, 3), np.int64), np.zeros((U, 3), np.int64)
    np.add.at(S, rank[inv], t[idx])
    np.add.at(Csum, rank[inv], colors[idx].astype(np.int64))
    nn = out["counts"].astype(np.int64)[:, None]
    iv = i[out["first"]].astype(np.float64)
    v64 = np.float64(np.float32(v))
    out["points"] = ((iv + (S.astype(np.float64) + 0.5 * nn.astype(np.float64)) / (nn.astype(np.float64) * 65536.0)) * v64
                     ).astype(np.float32).reshape(-1, 3)
    out["colors"] = ((2 * Csum + nn) // (2 * nn)).astype(np.uint8).reshape(-1, 3)
    return out


def assert_same(got, want, what=""):
    """Every output of two thinnings (NumPy arrays) byte for byte."""
    assert got["dropped"] == want["dropped"], (what, got["dropped"], want["dropped"])
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, int((g != w).sum()))


# ---- the host build of mvster_amd/csrc/voxel_math.h --------------------------------------------------------------------

_HM = {}


def load_voxel_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/voxel_hostmath.cpp like ``fusion_scene_cases.load_geo_hostmath`` (-ffp-contract=off) with the
    first compiler of `compilers` that exists and load it, once per process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of voxel_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libvoxelhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "voxel_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, f, i = ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int
    h.hm_voxel_points.restype, h.hm_voxel_points.argtypes = None, [p, l, f, p, p, p]
    h.hm_voxel_hash.restype, h.hm_voxel_hash.argtypes = None, [p, l, p]
    h.hm_voxel_thin.restype, h.hm_voxel_thin.argtypes = l, [p, p, l, f, i, p, p, p, p, p]
    _HM[compilers] = h
    return h


def host_point_terms(h, points, v):
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    M = len(points)
    valid, key, t = np.zeros(M, np.uint8), np.zeros(M, np.uint64), np.zeros((M, 3), np.int32)
    h.hm_voxel_points(points.ctypes.data, M, v, valid.ctypes.data, key.ctypes.data, t.ctypes.data)
    return valid.astype(bool), key, t


def host_hash(h, key):
    key = np.ascontiguousarray(key, np.uint64)
    out = np.zeros(len(key), np.uint64)
    h.hm_voxel_hash(key.ctypes.data, len(key), out.ctypes.data)
    return out


def thin_host(h, points, colors, v, reduce):
    """hm_voxel_thin -> dict like fusion.thin_points (NumPy arrays)."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    M = len(points)
    op, oc = np.zeros((M, 3), np.float32), np.zeros((M, 3), np.uint8)
    on, of, dropped = np.zeros(M, np.int32), np.zeros(M, np.int64), np.zeros(1, np.int64)
    U = h.hm_voxel_thin(points.ctypes.data, colors.ctypes.data, M, v, REDUCES.index(reduce), op.ctypes.data, oc.ctypes.data,
                        on.ctypes.data, of.ctypes.data, dropped.ctypes.data)
    return dict(points=op[:U].copy(), colors=oc[:U].copy(), counts=on[:U].copy(), first=of[:U].copy(), dropped=int(dropped[0]))


# ---- the case clouds -------------------------------------------------------------------------------------------------------

def default_slots(M):
    """fusion.thin_slots: the smallest power of two >= 2 * M, at least 64."""
    return max(64, 1 << max(0, 2 * M - 1).bit_length())


COLLIDING_VOXELS, COLLIDING_DOUBLES = 200, 40            # M = 240 -> 512 slots, load factor 0.47


def colliding_cloud(h, v, rng):
    """COLLIDING_VOXELS distinct voxels whose keys all have home slot slots - 3 at the default table size of the cloud (found
    by brute force with the header's hash): a probe run COLLIDING_VOXELS long that wraps past the table's end.  The first
    COLLIDING_DOUBLES voxels hold two points."""
    M = COLLIDING_VOXELS + COLLIDING_DOUBLES
    slots = default_slots(M)
    g = np.arange(-40, 40, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    key = (((cells[:, 0] + HALF) << 42) | ((cells[:, 1] + HALF) << 21) | (cells[:, 2] + HALF)).astype(np.uint64)
    home = host_hash(h, key) & np.uint64(slots - 1)
    hit = cells[home == np.uint64(slots - 3)][:COLLIDING_VOXELS]
    assert len(hit) == COLLIDING_VOXELS
    cells = np.concatenate([hit, hit[:COLLIDING_DOUBLES]])
    u = np.concatenate([np.full((COLLIDING_VOXELS, 3), 0.5), np.full((COLLIDING_DOUBLES, 3), 0.25)])
    pts = ((cells + u) * np.float64(np.float32(v))).astype(np.float32)[rng.permutation(M)]
    valid, got_key, _ = host_point_terms(h, pts, v)
    homes = host_hash(h, got_key) & np.uint64(slots - 1)
    assert valid.all() and len(np.unique(got_key)) == COLLIDING_VOXELS and (homes == np.uint64(slots - 3)).all()
    return pts


def face_values(v):
    """Scalars on and next to voxel faces on both sides of zero, the zeros, and values whose q - i rounds to 1 (the clamp)."""
    v32 = np.float32(v)
    on = np.array([k * np.float64(v32) for k in range(-3, 4)]).astype(np.float32)
    vals = np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf)),
                           np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 0.5 * v32, -0.5 * v32], np.float32)])
    return vals.astype(np.float32)


def invalid_points(v):
    """[N,3]: NaN, +-inf and |p| beyond 2^20 voxels in each axis (other axes valid), plus the points on the range's two ends:
    -2^20 * v is the lowest valid coordinate, +2^20 * v the first invalid one.  -> (points, how many are invalid)."""
    v32 = np.float32(v)
    edge = np.float32(HALF) * v32                            # exact: a power of two times v
    bad = np.array([np.nan, np.inf, -np.inf, 1.5 * edge, -1.5 * edge, edge, np.nextafter(-edge, np.float32(-np.inf)), 3e38,
                    -3e38], np.float32)
    good = np.array([-edge, np.nextafter(edge, np.float32(0))], np.float32)
    rows = []
    for ax in range(3):
        for b in np.concatenate([bad, good]):
            p = np.array([0.3, -0.7, 1.1], np.float32) * v32
            p[ax] = b
            rows.append(p)
    rows.append(np.full(3, np.nan, np.float32))
    return np.stack(rows).astype(np.float32), 3 * len(bad) + 1


_CLOUDS = {}


def case_clouds(v, compilers=("g++",)):
    """name -> (points [M,3] float32, colors [M,3] uint8) for voxel edge `v`; built once per process, never modified."""
    if v in _CLOUDS:
        return _CLOUDS[v]
    h = load_voxel_hostmath(compilers)
    rng = np.random.RandomState(int(v * 1000) + 7)
    v64 = np.float64(np.float32(v))
    out = {}

    def with_colors(p):
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        return p, rng.randint(0, 256, p.shape).astype(np.uint8)
    for M in (0, 1, 63, 64, 65, 257):                          # about 216 voxels: shared and single voxels mixed
        out["m%d" % M] = with_colors((rng.rand(M, 3) * 6 - 3) * v64)
    out["one_voxel"] = with_colors((np.array([2, -3, 5]) + 0.05 + 0.9 * rng.rand(4096, 3)) * v64)
    g = np.arange(-8, 8)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out["distinct"] = with_colors((cells[rng.permutation(4096)] + 0.5) * v64)
    f = face_values(v)
    per_axis = [np.where(np.arange(3) == ax, val, np.float32(0.5) * np.float32(v)) for ax in range(3) for val in f]
    out["faces"] = with_colors(np.concatenate([np.stack(per_axis), np.repeat(f[:, None], 3, 1)]))
    bad, nbad = invalid_points(v)
    mixed = np.concatenate([bad, (rng.rand(40, 3) * 4 - 2) * v64])[rng.permutation(len(bad) + 40)]
    out["invalid"] = with_colors(mixed)
    assert thin_numpy(*out["invalid"], v, "first")["dropped"] == nbad
    out["all_invalid"] = with_colors(np.full((70, 3), np.nan))
    p = np.array([[0.25, 0.5, 0.75]] * 2) * v64
    out["half"] = (p.astype(np.float32), np.array([[10, 0, 254], [11, 1, 255]], np.uint8))   # means 10.5, 0.5, 254.5
    out["colliding"] = with_colors(colliding_cloud(h, v, rng))
    _CLOUDS[v] = out
    return out


CASE_NAMES = ("m0", "m1", "m63", "m64", "m65", "m257", "one_voxel", "distinct", "faces", "invalid", "all_invalid", "half",
              "colliding")

_HOST = {}


def host_case(name, v, reduce, compilers=("g++",)):
    """thin_host of a case cloud, computed once per process and never modified."""
    k = (name, v, reduce)
    if k not in _HOST:
        _HOST[k] = thin_host(load_voxel_hostmath(compilers), *case_clouds(v, compilers)[name], v, reduce)
    return _HOST[k]
