"""Host build of mvster_amd/csrc/conv_taps.h against the emulator's decode of the K walk.

conv_mfma_kernel finds the tap of a K step by a scalar multiply-shift walk and decides padding from a per-voxel bit mask.
For every layer geometry below, every class, every voxel of the output lattice (all corners, edges and interior voxels of
a small input), and for the plain walk and each of the four split-K waves, the (tap, channel, offset, inside) sequence of
the host build must equal the decode tests/conv_emulator.py:run_layer uses: kk // CIN, kk % CIN, and the bounds test.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mvster_amd import conv_plan as cp
from mvster_amd.conv_plan import GEOM, GEOM_CLASS

HERE = os.path.dirname(os.path.abspath(__file__))

# kernel, stride, padding, transposed
GEOMETRIES = {
    "333_s1": ((3, 3, 3), (1, 1, 1), (1, 1, 1), False),
    "133_s2": ((1, 3, 3), (1, 2, 2), (0, 1, 1), False),
    "t133_s2": ((1, 3, 3), (1, 2, 2), (0, 1, 1), True),      # parity classes of 1 / 2 / 2 / 4 taps
    "155_s2": ((1, 5, 5), (1, 2, 2), (0, 2, 2), False),
    "111": ((1, 1, 1), (1, 1, 1), (0, 0, 0), False),
}
CINS = (4, 8, 16, 32, 64, 80)
INPUT = (2, 3, 4, 5)       # B, Di, Hi, Wi


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler: the host build of conv_taps.h cannot be made")
    so = str(tmp_path_factory.mktemp("conv_taps") / "libconvtaps.so")
    subprocess.check_call([cxx, "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "hostmath", "conv_taps_hostmath.cpp")])
    h = ctypes.CDLL(so)
    h.hm_conv_tap_walk.restype = ctypes.c_int
    h.hm_conv_tap_walk.argtypes = [ctypes.c_int] * 14 + [ctypes.c_void_p]
    h.hm_conv_masks_fit.restype = ctypes.c_int
    h.hm_conv_masks_fit.argtypes = [ctypes.c_int] * 3
    return h


def emulator_walk(cin, steps, kd, kh, kw, Di, Hi, Wi, iz0, iy0, ix0):
    """The decode of tests/conv_emulator.py:run_layer for the K steps `steps` of one voxel."""
    ntaps = kd * kh * kw
    rows = []
    for s in steps:
        for q in range(4):
            kk = s * 16 + q * 4
            tap, ch = kk // cin, kk % cin
            if tap >= ntaps:
                rows.append((s, tap, ch, None, 0))
                continue
            kx, ky, kz = tap % kw, (tap // kw) % kh, tap // (kw * kh)
            iz, iy, ix = iz0 + kz, iy0 + ky, ix0 + kx
            ok = (iz >= 0) and (iz < Di) and (iy >= 0) and (iy < Hi) and (ix >= 0) and (ix < Wi)
            rows.append((s, tap, ch, (kz * Hi + ky) * Wi + kx, int(ok)))
    return rows


def check_voxel(host, cin, nsteps_all, k, dims, i0):
    kd, kh, kw = k
    Di, Hi, Wi = dims
    buf = np.zeros((nsteps_all, 4, 5), dtype=np.int32)
    walks = [(0, 0)] + [(1, w) for w in range(4)]
    covered = []
    for force_cmp in (0, 1):
        for splitk, wave in walks:
            steps = list(range(wave, nsteps_all, 4)) if splitk else list(range(nsteps_all))
            n = host.hm_conv_tap_walk(cin, splitk, wave, nsteps_all, kd, kh, kw, Di, Hi, Wi, i0[0], i0[1], i0[2], force_cmp,
                                      buf.ctypes.data_as(ctypes.c_void_p))
            assert n == len(steps), (cin, k, splitk, wave, n, len(steps))
            want = emulator_walk(cin, steps, kd, kh, kw, Di, Hi, Wi, *i0)
            got = buf[:n].reshape(-1, 5).tolist()
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g[:3] == list(w[:3]) and g[4] == w[4], (cin, k, dims, i0, splitk, wave, force_cmp, g, w)
                if w[3] is not None:
                    assert g[3] == w[3], (cin, k, dims, i0, splitk, wave, force_cmp, g, w)
            if splitk and not force_cmp:
                covered += steps
    assert sorted(covered) == list(range(nsteps_all))      # the four waves take every K step exactly once
    return walks


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("gname", sorted(GEOMETRIES))
def test_tap_walk_matches_emulator_decode(host, gname, cin):
    k, s, p, transposed = GEOMETRIES[gname]
    B, Di, Hi, Wi = INPUT
    cout = 16
    w = torch.zeros(*(((cin, cout) if transposed else (cout, cin)) + k))
    layer = cp.ConvLayer(w, transposed, s, p)
    geom = layer._geom(B, Di, Hi, Wi, cp.SKIP_NONE)[0]
    g = dict(zip(GEOM, geom[:len(GEOM)].tolist()))
    ntap_classes, short, past_end = set(), False, False
    for ci in range(g["nclass"]):
        c = dict(zip(GEOM_CLASS, geom[len(GEOM) + ci * len(GEOM_CLASS):len(GEOM) + (ci + 1) * len(GEOM_CLASS)].tolist()))
        ntaps = c["kd"] * c["kh"] * c["kw"]
        ntap_classes.add(ntaps)
        assert host.hm_conv_masks_fit(c["kd"], c["kh"], c["kw"]) == 1
        short |= c["nsteps"] < 4
        past_end |= (c["nsteps"] * 16 - 1) // cin >= ntaps
        for zo in range(g["Do"]):
            for yo in range(g["Ho"]):
                for xo in range(g["Wo"]):
                    i0 = (zo * g["sd"] - c["pd"], yo * g["sh"] - c["ph"], xo * g["sw"] - c["pw"])
                    check_voxel(host, cin, c["nsteps"], (c["kd"], c["kh"], c["kw"]), (Di, Hi, Wi), i0)
        # a lane past the last voxel: no tap is inside
        check_voxel(host, cin, c["nsteps"], (c["kd"], c["kh"], c["kw"]), (Di, Hi, Wi), (-(1 << 20), -c["ph"], -c["pw"]))
    if gname == "t133_s2":
        assert sorted(ntap_classes) == [1, 2, 4]
    if gname == "111" and cin <= 32:
        assert short                       # nsteps < 4: some split-K waves get no step
    if cin in (4, 8) and gname in ("333_s1", "133_s2", "155_s2"):
        assert past_end                    # the last K step runs past the last tap


def test_wide_kernel_takes_the_comparing_form(host):
    """kd + kh + kw > 32 does not fit the mask word: the walk compares each axis and still equals the decode."""
    k, dims = (1, 2, 40), (1, 3, 45)
    assert host.hm_conv_masks_fit(*k) == 0
    for cin in (4, 16, 32):
        nsteps = (k[0] * k[1] * k[2] * cin + 15) // 16
        for y0 in (-1, 0, 2):
            for x0 in (-39, -3, 0, 7, 44):
                check_voxel(host, cin, nsteps, k, dims, (0, y0, x0))
