"""Argument checks of the eval forward's first and last launch (mvster_conv_narrow_pair_planes, mvster_deconv_select_riders):
every refusal comes before the first HIP call, so it is reported without a GPU.  Device pointers are stand-in addresses that
nothing dereferences; the pointer tables themselves are host memory."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


DEV = 1 << 32           # a stand-in device address, 16-byte aligned


def _table(vals):
    return ctypes.cast((ctypes.c_void_p * len(vals))(*vals), ctypes.c_void_p)


def _planes(lib, imgs, N=2, B=1, H=64, W=64, w1=DEV, out=DEV, side=None):
    tail = side if side is not None else (None, 0, None, None, 0, None, 0, 0, 0, 0)
    return lib.mvster_conv_narrow_pair_planes(imgs, N, B, H, W, w1, DEV, DEV, DEV, DEV, DEV, out, 1, 1, 1, *tail, None)


def test_planar_pair_refuses_bad_arguments(lib):
    from mvster_amd import _lib
    two = _table([DEV, DEV + 4096])
    assert _planes(lib, None) == _lib.ERR_NULL
    assert _planes(lib, two, w1=None) == _lib.ERR_NULL and _planes(lib, two, out=None) == _lib.ERR_NULL
    assert _planes(lib, _table([DEV, None])) == _lib.ERR_NULL                  # a missing view
    assert _planes(lib, _table([DEV, DEV + 2])) == _lib.ERR_SHAPE              # planes are read by 4-byte loads
    assert _planes(lib, _table([DEV] * 9), N=9) == _lib.ERR_SHAPE              # at most 8 views
    assert _planes(lib, two, N=0) == _lib.ERR_SHAPE and _planes(lib, two, H=0) == _lib.ERR_SHAPE
    assert _planes(lib, two, B=1, H=16384, W=16384) == _lib.ERR_SHAPE          # a view's planes: 32-bit buffer offsets
    assert _planes(lib, two, N=8, B=2, H=2048, W=4096) == _lib.ERR_SHAPE       # ... and the output's
    # side jobs: every table and output they need, sane sizes, at least one source view
    pms = _table([DEV] * 4)
    ok_side = (pms, 4, DEV, DEV, 2, DEV, 8, 8, 8, 1)
    for k in (2, 3, 5):
        assert _planes(lib, two, side=ok_side[:k] + (None,) + ok_side[k + 1:]) == _lib.ERR_NULL
    assert _planes(lib, two, side=(_table([DEV, None, DEV, DEV]),) + ok_side[1:]) == _lib.ERR_NULL
    for k, bad in ((1, 0), (1, 9), (4, 0), (6, 1), (7, 0), (8, 0)):            # nstage, ndv, D, h, w
        assert _planes(lib, two, side=ok_side[:k] + (bad,) + ok_side[k + 1:]) == _lib.ERR_SHAPE
    assert _planes(lib, _table([DEV]), N=1, side=ok_side) == _lib.ERR_SHAPE


def _riders(lib, D=4, n=3, ins=None, outs=None, his=None, wis=None, ho=64, wo=64, null=()):
    ins = _table([DEV] * 3) if ins is None else ins
    outs = _table([DEV] * 3) if outs is None else outs
    his = (ctypes.c_int * 3)(8, 16, 32) if his is None else his
    wis = (ctypes.c_int * 3)(8, 16, 32) if wis is None else wis
    tabs = [ins, outs, ctypes.cast(his, ctypes.c_void_p), ctypes.cast(wis, ctypes.c_void_p)]
    for k in null:
        tabs[k] = None
    return lib.mvster_deconv_select_riders(*([DEV] * 14), 1, D, 32, 32, 16, 1, 1.0, *tabs, n, ho, wo, None)


def test_selection_riders_refuse_bad_arguments(lib):
    from mvster_amd import _lib
    for k in range(4):
        assert _riders(lib, null=(k,)) == _lib.ERR_NULL
    assert _riders(lib, ins=_table([DEV, None, DEV])) == _lib.ERR_NULL and _riders(lib, outs=_table([None, DEV, DEV])) == _lib.ERR_NULL
    assert _riders(lib, n=0) == _lib.ERR_SHAPE and _riders(lib, n=4) == _lib.ERR_SHAPE
    assert _riders(lib, ho=0) == _lib.ERR_SHAPE and _riders(lib, wo=-1) == _lib.ERR_SHAPE
    assert _riders(lib, his=(ctypes.c_int * 3)(8, 0, 32)) == _lib.ERR_SHAPE
    # the riders exist on the MFMA kernel (D in {4, 8}) only: any other depth count is refused, nothing launched
    assert _riders(lib, D=5) == _lib.ERR_UNSUPPORTED and _riders(lib, D=16) == _lib.ERR_UNSUPPORTED
