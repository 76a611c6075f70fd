"""Shared by tests/test_resize_cpu.py and tests/test_gpu_resize.py (not a test module): the size cases of the loader's input
scaling, seeded 8-bit images, the host build of mvster_amd/csrc/resize_math.h, and an INDEPENDENT restatement of
``cv2.resize(img, (Wd, Hd))`` (INTER_LINEAR, float32 image) in plain scalar-style NumPy -- written from OpenCV's resize.cpp
(float path, scalar form), importing nothing from mvster_amd:

* ``inv = (double)Wd / Ws; scale_x = 1.0 / inv``; per output column ``fx = (float)((dx + 0.5) * scale_x - 0.5)``,
  ``sx = floor(fx)``, ``fx -= sx``; ``sx < 0 -> sx = 0, fx = 0``; ``sx >= Ws - 1 -> sx = Ws - 1, fx = 0`` and only the
  first tap is read there; rows likewise.
* horizontal pass per source row ``t = S[sx] * (1.f - fx) + S[sx + 1] * fx``, then ``D = t0 * (1.f - fy) + t1 * fy``; every
  product and sum a float32 operation of its own (NumPy never fuses).
* ``Ws == 2 Wd and Hs == 2 Hd``: the area path, ``((s00 + s01) + (s10 + s11)) * 0.25f``.
* the image is ``float32(u8) / 255.0f``.

There is no cv2 to pin the restatement itself; the tests pin GPU = host build = this, bit for bit.
"""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np

# (Hs, Ws, max_h, max_w) -> (Hd, Wd): what general_eval4.MVSDataset.scale_mvs_input arrives at
LOADER_SIZES = [((1200, 1600, 864, 1152), (832, 1152)), ((1200, 1600, 1200, 1600), (1152, 1600)),
                ((1080, 1920, 1024, 1920), (1024, 1792)), ((2048, 2560, 1024, 1280), (1024, 1280)),
                ((576, 768, 864, 1152), (576, 768))]

# name -> (Hs, Ws, Hd, Wd, image kind)
CASES = {
    "dtu_default": (1200, 1600, 832, 1152, "random"),
    "dtu_raw": (1200, 1600, 1152, 1600, "random"),
    "hd_1080": (1080, 1920, 1024, 1792, "random"),
    "area_2to1": (2048, 2560, 1024, 1280, "random"),
    "identity_64": (64, 64, 64, 64, "random"),
    "odd_source": (130, 197, 64, 128, "random"),               # odd source size, a different factor per axis
    "identity_in_y": (64, 200, 64, 192, "random"),
    "constant_255": (130, 197, 64, 128, "constant"),
    "checkerboard": (96, 160, 64, 128, "checker"),
    "checkerboard_area": (128, 256, 64, 128, "checker"),
}


def case_images(name, V=1):
    """uint8 [V,Hs,Ws,3], seeded by the case; a different image per view (view 0 of "constant" is 255 everywhere)."""
    Hs, Ws, _, _, kind = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) * 16 + V)
    if kind == "random":
        img = rng.randint(0, 256, size=(V, Hs, Ws, 3)).astype(np.uint8)
        img[0, 0, :min(Ws, 256), 0] = np.arange(min(Ws, 256))               # every level at least once where Ws allows
        return img
    if kind == "constant":
        return np.stack([np.full((Hs, Ws, 3), 255 - 37 * v, dtype=np.uint8) for v in range(V)])
    ys, xs = np.mgrid[0:Hs, 0:Ws]
    out = []
    for v in range(V):                                                      # one-pixel checkerboard, phase and levels per view
        lo, hi = 40 * v, 255 - 25 * v
        board = np.where((ys + xs + v) % 2 == 0, lo, hi).astype(np.uint8)
        out.append(np.stack([board, 255 - board, board], -1))
    return np.stack(out)


# ---- the independent restatement -------------------------------------------------------------------------------------------

def ref_axis_table(ns, nd):
    """One axis, one output sample at a time: -> (s int list, f float32 list, clamped-high bool list)."""
    inv = float(nd) / float(ns)
    scale = 1.0 / inv
    s_out, f_out, high = [], [], []
    for d in range(nd):
        f = np.float32((d + 0.5) * scale - 0.5)                             # Python doubles: two roundings, no fma
        s = int(math.floor(float(f)))
        f = np.float32(f - np.float32(s))
        hi = False
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= ns - 1:
            s, f, hi = ns - 1, np.float32(0), True
        s_out.append(s)
        f_out.append(f)
        high.append(hi)
    return s_out, f_out, high


def ref_resize(u8, Hd, Wd):
    """uint8 [Hs,Ws,3] -> float32 [Hd,Wd,3], one output row at a time."""
    Hs, Ws = u8.shape[:2]
    S = u8.astype(np.float32) / np.float32(255.0)
    D = np.empty((Hd, Wd, 3), dtype=np.float32)
    if Ws == 2 * Wd and Hs == 2 * Hd:
        for y in range(Hd):
            top, bottom = S[2 * y], S[2 * y + 1]
            D[y] = ((top[0::2] + top[1::2]) + (bottom[0::2] + bottom[1::2])) * np.float32(0.25)
        return D
    sx, fx, xhigh = ref_axis_table(Ws, Wd)
    sy, fy, yhigh = ref_axis_table(Hs, Hd)
    sx, xhigh = np.array(sx), np.array(xhigh)
    a1 = np.array(fx, dtype=np.float32)[:, None]
    a0 = np.float32(1.0) - a1
    inner = ~xhigh

    def hpass(row):
        t = np.empty((Wd, 3), dtype=np.float32)
        t[inner] = row[sx[inner]] * a0[inner] + row[sx[inner] + 1] * a1[inner]
        t[xhigh] = row[sx[xhigh]] * np.float32(1.0)                         # only the first tap is read there
        return t

    for y in range(Hd):
        b1 = np.float32(fy[y])
        b0 = np.float32(1.0) - b1
        t0 = hpass(S[sy[y]])
        if yhigh[y]:
            D[y] = t0 * np.float32(1.0)
        else:
            D[y] = t0 * b0 + hpass(S[sy[y] + 1]) * b1
    return D


def ref_outputs(u8_stack, Hd, Wd):
    """What ops.resize_pack_images_u8 must write for uint8 [V,Hs,Ws,3]: (RGB0 float32 [V,1,Hd,Wd,4], uint8 [V,Hd,Wd,3])."""
    V = len(u8_stack)
    out = np.zeros((V, 1, Hd, Wd, 4), dtype=np.float32)
    for v in range(V):
        out[v, 0, :, :, :3] = ref_resize(u8_stack[v], Hd, Wd)
    small = np.clip(out[:, 0, :, :, :3] * np.float32(255.0), 0, 255).astype(np.uint8)     # test_mvs4.py:262-264
    return out, small


# ---- the host build of mvster_amd/csrc/resize_math.h -----------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTMATH = os.path.join(ROOT, "tests", "hostmath")
HOST_FLAGS = ["-O2", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas"]


def load_resize_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/resize_hostmath.cpp with the first compiler of `compilers` that exists and load it.  No
    compiler is an error, never a skip: the comparisons that need the host build must not pass by not running."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of resize_math.h cannot be made" % (compilers,))
    so = os.path.join(HOSTMATH, "libresizehostmath.so")
    subprocess.check_call([found[0]] + HOST_FLAGS + ["-o", so, os.path.join(HOSTMATH, "resize_hostmath.cpp")])
    h = ctypes.CDLL(so)
    h.hm_resize_pack.restype = ctypes.c_int
    h.hm_resize_pack.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5
    return h


def run_host(h, u8_stack, Hd, Wd, tables):
    """hm_resize_pack with `tables` = (sx, fx, sy, fy) as the kernel gets them -> (RGB0 [V,1,Hd,Wd,4], uint8 [V,Hd,Wd,3])."""
    src = np.ascontiguousarray(u8_stack, dtype=np.uint8)
    V, Hs, Ws, _ = src.shape
    sx, fx, sy, fy = [np.ascontiguousarray(t) for t in tables]
    assert sx.dtype == sy.dtype == np.int32 and fx.dtype == fy.dtype == np.float32
    assert sx.shape == fx.shape == (Wd,) and sy.shape == fy.shape == (Hd,)
    out = np.full((V, 1, Hd, Wd, 4), np.nan, dtype=np.float32)
    small = np.zeros((V, Hd, Wd, 3), dtype=np.uint8)
    rc = h.hm_resize_pack(src.ctypes.data, sx.ctypes.data, fx.ctypes.data, sy.ctypes.data, fy.ctypes.data, out.ctypes.data,
                          small.ctypes.data, V, Hs, Ws, Hd, Wd)
    assert rc == 0, "hm_resize_pack: a table entry lies outside the image"
    return out, small
