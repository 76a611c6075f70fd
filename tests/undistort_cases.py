"""Shared by tests/test_undistort_cpu.py and tests/test_gpu_undistort.py (not a test module): the cameras of the cases, the
undistortion restated in NumPy in another evaluation order, the host build of
mvster_amd/csrc/undistort_math.h, and seeded images.

Neither yardstick comes from the reference tree, which has no such step, nor from COLMAP, which is not at hand: the restatement
follows the definition in float64 with NumPy's own operations, the host build is the kernels' own arithmetic compiled for the
CPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from tests import fusion_scene_cases as C

W, H, F, CX, CY = 160, 120, 140.0, 80.3, 59.6


def record(model, params, w=W, h=H):
    """A 12-double camera record from COLMAP's parameter list of the model"""
    from mvster_amd import sfm
    return sfm.camera_record(model, w, h, params)


CAM_A = record(2, [F, CX, CY, -0.12])
CAM_A_PLUS = record(2, [F, CX, CY, 0.12])
CAM_B = record(3, [F, CX, CY, -0.2, 0.05])
CAM_C = record(4, [F, 141.4, CX, CY, -0.25, 0.08, 0.002, -0.003])
CAM_Z = record(2, [F, CX, CY, 0.0])
CAM_FOLD = record(2, [F, CX, CY, -3.0])                                         # folds over inside the image
CAMERAS = dict(A=CAM_A, A_plus=CAM_A_PLUS, B=CAM_B, C=CAM_C, Z=CAM_Z)
# COLMAP's parameter lists of the same cameras, for the readers
COLMAP = dict(A=(2, [F, CX, CY, -0.12]), B=(3, [F, CX, CY, -0.2, 0.05]), C=(4, [F, 141.4, CX, CY, -0.25, 0.08, 0.002, -0.003]))


def small(cam, w, h):
    """The same lens with the same field of view on a w x h image (focal lengths and principal point in proportion)"""
    c = cam.copy()
    c[1], c[2], c[3], c[4], c[5], c[6] = w, h, cam[3] * w / W, cam[4] * h / H, cam[5] * w / W, cam[6] * h / H
    return c


# ---- the definition, restated in NumPy (another evaluation order) -------------------------------------------------------------------

def distort_numpy(c, u, v):
    k1, k2, p1, p2 = c[7:11]
    r2 = u * u + v * v
    radial = 1.0 + r2 * (k1 + k2 * r2)
    return (u * radial + p2 * (r2 + 2 * u * u) + 2 * p1 * u * v, v * radial + p1 * (r2 + 2 * v * v) + 2 * p2 * u * v)


def jacobian_numpy(c, u, v):
    k1, k2, p1, p2 = c[7:11]
    r2 = u * u + v * v
    radial, slope = 1.0 + r2 * (k1 + k2 * r2), 2 * k1 + 4 * k2 * r2
    a = radial + slope * u * u + 6 * p2 * u + 2 * p1 * v
    d = radial + slope * v * v + 6 * p1 * v + 2 * p2 * u
    b = slope * u * v + 2 * p1 * u + 2 * p2 * v
    return a, b, b, d


def undistort_numpy(c, ud, vd, steps=10):
    """Newton from (ud, vd), ``steps`` steps, every point to the end -> (u, v, residual)"""
    u, v = np.array(ud, dtype=np.float64), np.array(vd, dtype=np.float64)
    for _ in range(steps):
        fu, fv = distort_numpy(c, u, v)
        a, b, cc, d = jacobian_numpy(c, u, v)
        det = a * d - b * cc
        u, v = u - (d * (fu - ud) - b * (fv - vd)) / det, v - (a * (fv - vd) - cc * (fu - ud)) / det
    fu, fv = distort_numpy(c, u, v)
    return u, v, np.maximum(np.abs(fu - ud), np.abs(fv - vd))


def camera_numpy(c, blank=0.0, min_scale=0.2, max_scale=2.0, scale=None, margin=1e-6):
    """-> (W', H', cx', cy', scale_x W, scale_y H).  Asserts that scale W and scale H stay further than ``margin`` from a whole
    number, so that another summation order cannot give another size."""
    w, h, fx, fy, cx, cy = int(c[1]), int(c[2]), c[3], c[4], c[5], c[6]
    if scale is None:
        ys, xs = np.arange(h) + 0.5, np.arange(w) + 0.5
        col = lambda px: undistort_numpy(c, (np.full(h, px) - cx) / fx, (ys - cy) / fy)
        row = lambda py: undistort_numpy(c, (xs - cx) / fx, (np.full(w, py) - cy) / fy)
        left, right = col(0.5)[0] * fx + cx, col(w - 0.5)[0] * fx + cx
        top, bottom = row(0.5)[1] * fy + cy, row(h - 0.5)[1] * fy + cy
        with np.errstate(divide="ignore", invalid="ignore"):
            min_x = min(cx / (cx - left.max()), (w - 0.5 - cx) / (right.max() - cx))
            max_x = max(cx / (cx - left.min()), (w - 0.5 - cx) / (right.min() - cx))
            min_y = min(cy / (cy - top.max()), (h - 0.5 - cy) / (bottom.max() - cy))
            max_y = max(cy / (cy - top.min()), (h - 0.5 - cy) / (bottom.min() - cy))
            sx = float(np.clip(1.0 / (min_x * blank + max_x * (1.0 - blank)), min_scale, max_scale))
            sy = float(np.clip(1.0 / (min_y * blank + max_y * (1.0 - blank)), min_scale, max_scale))
    else:
        sx, sy = scale
    for s in (sx * w, sy * h):
        assert abs(s - round(s)) > margin or s == round(s), ("a size at the edge of a whole number", s)
    wn, hn = max(1, int(sx * w)), max(1, int(sy * h))
    return wn, hn, cx * wn / w, cy * hn / h, sx * w, sy * h


def sources_numpy(c, o):
    """The source location of every pixel of the undistorted camera o = (W', H', fx, fy, cx', cy', ...) -> sx, sy [H',W']"""
    wn, hn = int(o[0]), int(o[1])
    x, y = np.meshgrid(np.arange(wn, dtype=np.float64), np.arange(hn, dtype=np.float64))
    ud, vd = distort_numpy(c, (x + 0.5 - o[4]) / o[2], (y + 0.5 - o[5]) / o[3])
    return c[3] * ud + c[5] - 0.5, c[4] * vd + c[6] - 0.5


def grid(c, n=31):
    """n x n pixel positions over the image of c -> normalised (u, v), flat"""
    x, y = np.meshgrid(np.linspace(0.0, c[1], n), np.linspace(0.0, c[2], n))
    return ((x - c[5]) / c[3]).ravel(), ((y - c[6]) / c[4]).ravel()


def image(h, w, seed):
    """A seeded uint8 [h,w,3] image: smooth waves plus noise, so that neighbouring taps differ and every byte value occurs"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127.5 + 90.0 * np.sin(x[..., None] * (0.11 + 0.03 * np.arange(3)) + seed) * np.cos(y[..., None] * (0.07 + 0.02 * np.arange(3)))
    return np.clip(base + rng.randint(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)


# ---- the host build of mvster_amd/csrc/undistort_math.h ----------------------------------------------------------------------------

_HM = {}


def load_undistort_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/undistort_hostmath.cpp with the flags of ``fusion_scene_cases.load_geo_hostmath`` and load it, once
    per process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of undistort_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libundistorthostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "undistort_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, i, d = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double
    h.hm_und_distort.restype, h.hm_und_distort.argtypes = None, [p, l, p, p]
    h.hm_und_undistort.restype, h.hm_und_undistort.argtypes = None, [p, l, p, p, p]
    h.hm_und_cameras.restype, h.hm_und_cameras.argtypes = None, [p, i, d, d, d, i, d, d, p]
    h.hm_und_points.restype, h.hm_und_points.argtypes = None, [p, i, p, l, i, p, p, p]
    h.hm_und_image.restype, h.hm_und_image.argtypes = None, [p, l, l, p, p, l, l, p, p]
    h.hm_und_sources.restype, h.hm_und_sources.argtypes = None, [p, p, l, l, p]
    h.hm_und_newton_steps.restype, h.hm_und_newton_steps.argtypes = i, []
    _HM[compilers] = h
    return h


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def distort_host(h, c, u, v):
    uv, out = _f64(np.stack([u, v], 1)), np.zeros((len(u), 2))
    h.hm_und_distort(_f64(c).ctypes.data, len(u), uv.ctypes.data, out.ctypes.data)
    return out[:, 0], out[:, 1]


def undistort_host(h, c, ud, vd):
    uv, out, res = _f64(np.stack([ud, vd], 1)), np.zeros((len(ud), 2)), np.zeros(len(ud))
    h.hm_und_undistort(_f64(c).ctypes.data, len(ud), uv.ctypes.data, out.ctypes.data, res.ctypes.data)
    return out[:, 0], out[:, 1], res


def cameras_host(h, table, blank=0.0, min_scale=0.2, max_scale=2.0, scale=None):
    """-> [C,8]: what mvster_undistort_cameras writes"""
    table = _f64(np.atleast_2d(table))
    out = np.zeros((len(table), 8))
    sx, sy = scale if scale is not None else (1.0, 1.0)
    h.hm_und_cameras(table.ctypes.data, len(table), blank, min_scale, max_scale, int(scale is not None), sx, sy, out.ctypes.data)
    return out


def points_host(h, table, rows, direction, xy):
    table, rows, xy = _f64(np.atleast_2d(table)), np.ascontiguousarray(rows, np.int32), _f64(xy).reshape(-1, 2)
    out, res = np.zeros((len(xy), 2)), np.zeros(len(xy))
    h.hm_und_points(table.ctypes.data, len(table), rows.ctypes.data, len(xy), direction, xy.ctypes.data, out.ctypes.data, res.ctypes.data)
    return out, res


def image_host(h, src, c, o):
    """-> (dst uint8 [H',W',3], valid uint8 [H',W'])"""
    src, c, o = np.ascontiguousarray(src, np.uint8), _f64(c), _f64(o)
    hd, wd = int(o[1]), int(o[0])
    dst, valid = np.zeros((hd, wd, 3), np.uint8), np.zeros((hd, wd), np.uint8)
    h.hm_und_image(src.ctypes.data, src.shape[0], src.shape[1], c.ctypes.data, o.ctypes.data, hd, wd, dst.ctypes.data, valid.ctypes.data)
    return dst, valid


def sources_host(h, c, o):
    c, o = _f64(c), _f64(o)
    hd, wd = int(o[1]), int(o[0])
    s = np.zeros((hd, wd, 2))
    h.hm_und_sources(c.ctypes.data, o.ctypes.data, hd, wd, s.ctypes.data)
    return s[..., 0], s[..., 1]


def assert_bytes(g, w, what=""):
    g, w = np.asarray(g), np.asarray(w)
    assert g.dtype.itemsize == w.dtype.itemsize and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.nonzero(np.frombuffer(g.tobytes(), np.uint8) != np.frombuffer(w.tobytes(), np.uint8))[0]
        k = int(bad[0]) // g.dtype.itemsize
        raise AssertionError((what, "%d bytes differ, the first in element %d: %r against %r" % (len(bad), k, g.ravel()[k], w.ravel()[k])))
