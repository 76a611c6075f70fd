"""Every weight-gradient kernel path (conv_wgrad.hip, conv_wgrad_pers.hip) against the fp64 reference of
tests/wgrad_cases.py, on the product library.

Exact: with integer inputs in {-2, ..., 2} every partial sum is an integer below 2^24, so the slot kernels, their
cross-wave sums and the finish must give the fp64 result bit for bit in whatever order they add.  Guarded: the operands
are views inside NaN-filled buffers and ``partial`` / ``dW`` come back NaN-filled from the allocator, so a read outside a
tensor, a kept element of a slot that no workgroup wrote and an unwritten gradient element all show as NaN.  Pinned:
``_lib.last_kernel()`` must name the instantiation the table expects -- a dispatch edit that moves a layer onto another
kernel fails here instead of quietly dropping that kernel's coverage."""
import ctypes
import json
import os

import pytest
import torch

from tests import wgrad_cases as WC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import _lib, ops
    from mvster_amd import train_ops as T
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN = float("nan")
REPORT = {}


def report_dir():
    """Where the suite's parity reports go: the directory of parity_train.json in tests/test_gpu_train.py's note(), taken
    from there so that the reports stay together if it moves."""
    from tests import test_gpu_train
    return os.path.dirname(next(c for c in test_gpu_train.note.__code__.co_consts
                                if isinstance(c, str) and c.endswith("/parity_train.json")))


def note(name, **kv):
    REPORT[name] = kv
    os.makedirs(report_dir(), exist_ok=True)
    with open(os.path.join(report_dir(), "parity_wgrad.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def guarded(t):
    """A contiguous device copy of ``t`` inside a NaN-filled buffer: more than one full W * C row of NaN on either side."""
    guard = -(-t.shape[-2] * t.shape[-1] // 64) * 64 + 64          # (a multiple of 256 bytes: the view stays 16-byte aligned)
    buf = torch.full((t.numel() + 2 * guard,), NAN, device=DEV, dtype=torch.float32)
    view = buf[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


def run_case(c, x, gy, monkeypatch, poison):
    """ops.conv_wgrad for a table case -> (dW, kernel name); ``poison``: float32 allocations come back NaN-filled."""
    if c.slots is not None:
        monkeypatch.setattr(ops, "WGRAD_MAX_SLOTS", c.slots)
    made = []
    if poison:
        real = torch.empty

        def poisoned(*a, **k):
            t = real(*a, **k)
            if t.is_cuda and t.dtype == torch.float32:
                t.fill_(NAN)
                made.append(tuple(t.shape))
            return t
        monkeypatch.setattr(torch, "empty", poisoned)
    got = ops.conv_wgrad(x, gy, c.kernel, c.stride, c.padding, co_keep=c.co_keep, ci_keep=c.ci_keep, mirrored=c.form == "mirrored")
    name = _lib.last_kernel()
    if poison:
        monkeypatch.setattr(torch, "empty", real)
        assert len(made) == 2 and made[1] == tuple(got.shape), made          # `partial` and dW, both poisoned
        if c.slots is not None:
            assert made[0][0] <= c.slots
    return got, name


@pytest.mark.parametrize("c", WC.CASES, ids=WC.IDS)
def test_exact_guarded_pinned(c, monkeypatch):
    x, gy, want = WC.case_data(c, exact=True)
    xbuf, xg = guarded(x)
    gbuf, gg = guarded(gy)
    got, name = run_case(c, xg, gg, monkeypatch, poison=True)
    again, name2 = run_case(c, xg, gg, monkeypatch, poison=True)
    torch.cuda.synchronize()
    g = got.cpu().double()
    assert tuple(g.shape) == tuple(want.shape)
    assert not g.isnan().any(), "%d NaN of %d: a read outside the tensors or an unwritten element" % (g.isnan().sum().item(), g.numel())
    assert torch.equal(g, want), "max |got - ref| = %g on %s" % ((g - want).abs().max().item(), name)
    assert torch.equal(got, again)
    assert name == c.kernel_name and name2 == c.kernel_name, (name, name2, c.kernel_name)
    # the operands are read-only: the guards and the data are as they were
    assert torch.equal(xg.cpu(), x) and torch.equal(gg.cpu(), gy)
    n = x.numel()
    assert xbuf[:(xbuf.numel() - n) // 2].isnan().all() and xbuf[(xbuf.numel() + n) // 2:].isnan().all()


@pytest.mark.parametrize("c", WC.CASES, ids=WC.IDS)
def test_normal_inputs(c, monkeypatch):
    """randn operands: max |got - ref| <= 2e-5 * max |ref|, the bound of this operation in test_gpu_train.py."""
    x, gy, want = WC.case_data(c, exact=False)
    got, name = run_case(c, x.to(DEV), gy.to(DEV), monkeypatch, poison=False)
    err = ((got.cpu().double() - want).abs().max() / want.abs().max()).item()
    note(c.name, dw=err, kernel=name)
    assert name == c.kernel_name
    assert err <= 2e-5, err


# ---- the finish kernel alone -----------------------------------------------------------------------------------------
# cip -> (ngrp, cop, width, ntaps, co_lim, ci_lim): keeps below the padded sizes; 9 taps four per tile and 27 taps two per
# tile leave dead tap columns
FINISH = {0: (9, 32, 32, 9, 20, 19), 4: (3, 64, 16, 9, 33, 3), 8: (14, 16, 16, 27, 7, 5)}


def finish_partial(nblk, cip, seed):
    """Integer slots (|v| <= 8: any order of at most 300 of them is exact) with NaN in every dropped position."""
    ngrp, cop, width, ntaps, co_lim, ci_lim = FINISH[cip]
    g = torch.Generator().manual_seed(seed)
    partial = torch.randint(-8, 9, (nblk, ngrp, cop, width), generator=g).float()
    grp, co, col = torch.meshgrid(torch.arange(ngrp), torch.arange(cop), torch.arange(width), indexing="ij")
    tap, ci = (grp * (16 // cip) + col // cip, col % cip) if cip else (grp, col)
    partial[:, (tap >= ntaps) | (co >= co_lim) | (ci >= ci_lim)] = NAN
    return partial


def finish_alone(partial, cip, swap, flip):
    ngrp, cop, width, ntaps, co_lim, ci_lim = FINISH[cip]
    dw = torch.full((ci_lim, co_lim, ntaps) if swap else (co_lim, ci_lim, ntaps), NAN, device=DEV, dtype=torch.float32)
    rc = _lib.load().mvster_conv_wgrad_finish(partial.data_ptr(), dw.data_ptr(), partial.shape[0], ngrp, cop, width, ntaps, cip,
                                              co_lim, ci_lim, int(swap), int(flip), ops._stream())
    assert rc == 0
    return dw


@pytest.mark.parametrize("cip", [0, 4, 8])
@pytest.mark.parametrize("nblk", [1, 15, 16, 17, 129, 137, 300])
def test_finish_alone(nblk, cip):
    """1 .. 300 slots -- fewer than the 16 wavefronts, no multiple of 16, more than the 128 of one trip -- against the
    layout formula, exactly."""
    ntaps = FINISH[cip][3]
    partial = finish_partial(nblk, cip, 1000 * cip + nblk)
    pg = partial.to(DEV)
    for swap in (False, True):
        for flip in (False, True):
            want = WC.finish_reference(partial, ntaps, cip, FINISH[cip][4], FINISH[cip][5], swap, flip)
            assert not want.isnan().any()
            got = finish_alone(pg, cip, swap, flip).cpu().double()
            assert torch.equal(got, want), (nblk, cip, swap, flip, (got - want).abs().max().item())


class _Rec(ctypes.Structure):          # FinishArgs of conv_wgrad.hip (as ops.conv_wgrad_flush builds it)
    _fields_ = [("partial", ctypes.c_void_p), ("dw", ctypes.c_void_p)] + [(n, ctypes.c_int) for n in
               ("nblk", "ngrp", "cop", "width", "ntaps", "cip", "co_lim", "ci_lim", "swap", "flip")]


@pytest.mark.parametrize("count", [57, 113])
def test_finish_batch_equals_the_single_finishes(count):
    """More records than one launch holds (56): mixed layouts and slot counts, the same bits as one finish each."""
    pool = []
    for i, (nblk, cip) in enumerate([(1, 0), (17, 4), (129, 8), (16, 0), (137, 4), (15, 8), (40, 0)]):
        pg = finish_partial(nblk, cip, 77 + i).to(DEV)
        for swap, flip in ((0, 0), (1, 1)) if i % 2 else ((0, 1), (1, 0)):
            pool.append((pg, cip, swap, flip, finish_alone(pg, cip, swap, flip)))
    arr = (_Rec * count)()
    outs = []
    for i, r in enumerate(arr):
        pg, cip, swap, flip, single = pool[(5 * i) % len(pool)]
        ngrp, cop, width, ntaps, co_lim, ci_lim = FINISH[cip]
        dw = torch.full_like(single, NAN)
        r.partial, r.dw = pg.data_ptr(), dw.data_ptr()
        (r.nblk, r.ngrp, r.cop, r.width, r.ntaps, r.cip, r.co_lim, r.ci_lim, r.swap, r.flip) = (
            pg.shape[0], ngrp, cop, width, ntaps, cip, co_lim, ci_lim, swap, flip)
        outs.append((dw, single))
    rc = _lib.load().mvster_conv_wgrad_finish_batch(ctypes.cast(arr, ctypes.c_void_p), count, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for i, (dw, single) in enumerate(outs):
        assert not dw.isnan().any() and torch.equal(dw, single), i


# ---- layer_form is what _ConvCL.backward really passes ------------------------------------------------------------------
LAYERS = [
    # kind, cin, cout, kernel, stride, input channels handed in, (B, D, H, W) of the layer's input
    ("conv", 16, 32, (1, 3, 3), (1, 2, 2), 16, (1, 2, 6, 10)),          # plain
    ("convT", 16, 8, (1, 3, 3), (1, 2, 2), 16, (1, 2, 3, 5)),           # transposed
    ("conv", 64, 8, (1, 3, 3), (1, 1, 1), 64, (1, 1, 4, 6)),            # mirrored
    ("conv", 16, 1, (1, 3, 3), (1, 1, 1), 16, (1, 1, 4, 6)),            # mirrored, the head padded to 4 channels
    ("conv", 8, 1, (1, 1, 1), (1, 1, 1), 8, (1, 2, 4, 6)),              # plain, the `prob` head padded to 4 channels
    ("conv", 3, 8, (1, 3, 3), (1, 1, 1), 3, (1, 1, 4, 6)),              # plain, RGB padded to 4 channels
]


@pytest.mark.parametrize("layer", LAYERS, ids=["%s_%d_%d_k%d%d_s%d" % (l[0], l[1], l[2], l[3][0], l[3][2], l[4][2]) for l in LAYERS])
def test_layer_form_matches_conv_cl_backward(layer, monkeypatch):
    kind, cin, cout, k, s, cx, shape = layer
    g = torch.Generator().manual_seed(11)
    p = tuple(ki // 2 for ki in k)
    w = torch.randn(((cin, cout) if kind == "convT" else (cout, cin)) + k, generator=g).to(DEV).requires_grad_(True)
    x = torch.randn(shape + (cx,), generator=g).to(DEV)
    seen = []
    real = ops.conv_wgrad

    def spy(x_cl, gy_cl, kernel, stride, padding, co_keep=None, ci_keep=None, mirrored=False, **kw):
        seen.append((x_cl.shape[-1], gy_cl.shape[-1], tuple(kernel), tuple(stride), tuple(padding), co_keep, ci_keep, bool(mirrored),
                     tuple(x_cl.shape[:4]), tuple(gy_cl.shape[:4])))
        return real(x_cl, gy_cl, kernel, stride, padding, co_keep=co_keep, ci_keep=ci_keep, mirrored=mirrored, **kw)
    monkeypatch.setattr(ops, "conv_wgrad", spy)
    y = T.conv_cl(x, w, None, s, p, kind == "convT")
    y.backward(torch.randn(y.shape, generator=g).to(DEV))
    torch.cuda.synchronize()
    assert len(seen) == 1
    form, CI, CO, k2, s2, p2, co_keep, ci_keep = WC.layer_form(kind, cin, cout, k, s, p)
    assert seen[0][:8] == (CI, CO, k2, s2, p2, co_keep, ci_keep, form == "mirrored")
    # the x role: the layer's input for the plain form, its output gradient for the other two
    assert seen[0][8 if form == "plain" else 9] == tuple(x.shape[:4]) and seen[0][9 if form == "plain" else 8] == tuple(y.shape[:4])
    assert tuple(w.grad.shape) == tuple(w.shape)
    assert any(c.form == form and (c.CI, c.CO, c.kernel, c.stride, c.co_keep, c.ci_keep) == (CI, CO, k2, s2, co_keep, ci_keep)
               for c in WC.CASES)


# ---- status codes: all of these return before any launch ------------------------------------------------------------------
def test_status_codes():
    lib = _lib.load()
    buf = torch.zeros(64, device=DEV)
    p, st = buf.data_ptr(), ops._stream()

    def wgrad(x=p, gy=p, partial=p, nblk=1, B=1, Di=1, Hi=4, Wi=6, CI=16, Do=1, Ho=4, Wo=6, CO=16, k=(1, 3, 3), s=(1, 1, 1),
              pad=(0, 1, 1), packed=0):
        return lib.mvster_conv_wgrad(x, gy, partial, nblk, B, Di, Hi, Wi, CI, Do, Ho, Wo, CO, *k, *s, *pad, packed, st)
    assert wgrad(Wo=5) == _lib.ERR_SHAPE and wgrad(Ho=5) == _lib.ERR_SHAPE and wgrad(Do=2) == _lib.ERR_SHAPE
    assert wgrad(s=(1, 2, 2)) == _lib.ERR_SHAPE                      # (4 x 6 at stride 2 is 2 x 3)
    assert wgrad(nblk=0) == _lib.ERR_SHAPE and wgrad(B=0) == _lib.ERR_SHAPE
    assert wgrad(CI=65) == _lib.ERR_UNSUPPORTED and wgrad(CO=81) == _lib.ERR_UNSUPPORTED
    assert wgrad(packed=1) == _lib.ERR_UNSUPPORTED                   # packed is for CI <= 8
    assert wgrad(x=None) == _lib.ERR_NULL and wgrad(gy=None) == _lib.ERR_NULL and wgrad(partial=None) == _lib.ERR_NULL

    def finish(partial=p, dw=p, nblk=1, ngrp=9, cop=16, width=16, ntaps=9, cip=0, co_lim=16, ci_lim=16):
        return lib.mvster_conv_wgrad_finish(partial, dw, nblk, ngrp, cop, width, ntaps, cip, co_lim, ci_lim, 0, 0, st)
    assert finish(co_lim=17) == _lib.ERR_SHAPE and finish(ci_lim=17) == _lib.ERR_SHAPE and finish(ngrp=8) == _lib.ERR_SHAPE
    assert finish(cip=3) == _lib.ERR_UNSUPPORTED and finish(cip=16) == _lib.ERR_UNSUPPORTED
    assert finish(cip=8, ngrp=5, ci_lim=9) == _lib.ERR_SHAPE and finish(cip=8, ngrp=4, ci_lim=8) == _lib.ERR_SHAPE
    assert finish(cip=4, ngrp=3, ci_lim=4, width=32) == _lib.ERR_SHAPE
    assert finish(partial=None) == _lib.ERR_NULL and finish(dw=None) == _lib.ERR_NULL
    assert lib.mvster_conv_wgrad_finish_batch(None, 1, st) == _lib.ERR_NULL
    rec = (_Rec * 1)()
    assert lib.mvster_conv_wgrad_finish_batch(ctypes.cast(rec, ctypes.c_void_p), 0, st) == _lib.ERR_SHAPE
    assert lib.mvster_conv_wgrad_finish_batch(ctypes.cast(rec, ctypes.c_void_p), 1, st) == _lib.ERR_NULL     # (a record of nulls)
    torch.cuda.synchronize()
    assert not buf.any()                                             # nothing ran
