"""The training step's summary without a GPU: the host restatement of Blend_loss's pooled error figures against loss.py's
tensor expression on CPU tensors, ``reduce_scalar_sums`` with other names, and the new symbols' declarations and argument
checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import train_summary_cases as TC
from tests import validate_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


def _blend_figures_on_cpu(monkeypatch, est, gt, mask, scale):
    """epe, err3, err1 as mvster_amd.loss.Blend_loss forms them on CPU tensors (the per-stage kernels stubbed out)."""
    from mvster_amd import loss as L
    z = torch.zeros(())
    monkeypatch.setattr(L, "stage_losses_total", lambda *a: (z, z, z, z))
    t = torch.from_numpy
    dummy = torch.zeros(1, 4, 1, 1)
    # scale = 128 / (depth_max - depth_min): depth_min = 0 and depth_max = 128 / scale give back the scale only approximately, so
    # the expression is fed through its own arithmetic: the scale the loss forms is the one the restatement gets
    depth_max = 128.0 / t(scale.astype(np.float32))
    depth_min = torch.zeros_like(depth_max)
    used = (128 / (depth_max - depth_min)).numpy()
    r = L.Blend_loss({"stage1": {"depth": t(est), "hypo_depth": dummy, "attn_weight": dummy}}, {"stage1": t(gt)},
                     {"stage1": t(mask)}, depth_max=depth_max, depth_min=depth_min)
    assert len(r) == 7
    return [float(v) for v in r[4:]], used


@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("mask_kind,special,scale_kind", [("80", "invalid_only", "random"), ("all", "invalid_only", "pow2"),
                                                          ("one_empty", "valid_too", "random"), ("80", "valid_too", "pow2"),
                                                          ("all_empty", "invalid_only", "random")])
def test_restatement_against_the_tensor_expression(monkeypatch, shape, mask_kind, special, scale_kind):
    """err3 / err1 bit-equal (counts below 2^24: the fp32 quotient of the expression is the double quotient rounded once);
    epe within rtol 1e-5 (fp32 mean against the fp64 sum), the project's tolerance for these figures."""
    est, gt, mask, scale = TC.make_case(shape, mask_kind, special, scale_kind)
    (epe, err3, err1), used = _blend_figures_on_cpu(monkeypatch, est, gt, mask, scale)
    out, raw = TC.pooled_ref(est, gt, mask, TC.THRESHOLDS, used)
    assert out.dtype == np.float32 and out.shape == (3,)
    print("expression", (epe, err3, err1), "restatement", out.tolist(), "valid", raw[:, 0].sum())
    assert TC.same_f32(np.float32(err3), out[1]) and TC.same_f32(np.float32(err1), out[2]), ((err3, err1), out)
    if math.isnan(epe) or math.isinf(epe):
        assert VC.same_float(epe, float(out[0]))
    else:
        assert abs(epe - float(out[0])) <= 1e-5 * abs(epe), (epe, out[0])
    if mask_kind == "all_empty":
        assert np.isnan(out).all() and raw[:, 0].sum() == 0


def test_restatement_on_a_hand_computed_example():
    """Two images, scales 1 and 0.5; errors 0, 1, 3, 3.5 | 1 (= 2 * 0.5), 3, NaN, and dropped pixels."""
    gt = np.full((2, 2, 3), 10.0, np.float32)
    est = np.array([[[10.0, 11.0, 13.0], [13.5, 99.0, 99.0]], [[12.0, 4.0, np.nan], [np.inf, 99.0, 99.0]]], np.float32)
    mask = np.array([[[1, 1, 1], [1, 0, 0]], [[1, 1, 1], [0, 0, 0]]], np.float32)
    out, raw = TC.pooled_ref(est, gt, mask, (3, 1), np.array([1.0, 0.5], np.float32))
    assert raw[0].tolist() == [4.0, 7.5, 3.0, 2.0]
    assert raw[1, 0] == 3.0 and np.isnan(raw[1, 1]) and raw[1, 2:].tolist() == [2.0, 1.0]      # the NaN: denominator only
    assert np.isnan(out[0])
    assert out[1] == np.float32(np.float32(5.0 / 7.0) * np.float32(100)) and out[2] == np.float32(np.float32(3.0 / 7.0) * np.float32(100))
    out1, _ = TC.pooled_ref(est[:1], gt[:1], mask[:1], (3, 1), None)
    assert out1.tolist() == [1.875, 75.0, 50.0]
    # not "valid minus above": above-3 counts 1 of image 1's three valid pixels (none: 1 and 3 are at-or-below, NaN neither)
    above = VC.raw_ref(est, gt, mask, (3, 1), np.array([1.0, 0.5], np.float32))
    assert above[1, 2] == 0.0 and raw[1, 0] - above[1, 2] != raw[1, 2]


def test_cases_hold_what_the_gpu_test_needs():
    names = [c[0] for c in TC.cases()]
    assert len(names) == len(set(names)) == 40
    est, gt, mask, scale = TC.make_case((2, 129, 161), "80", "invalid_only", "pow2")
    assert scale.tolist() == [1.0, 0.5]
    for n in range(2):
        e = VC.errors(est[n], gt[n], mask[n] > 0.5, scale[n])
        assert (e == 3.0).sum() >= 2 and (e == 1.0).sum() >= 2               # planted exactly on the thresholds, both signs
    _, raw = TC.pooled_ref(est, gt, mask, TC.THRESHOLDS, scale)
    assert (raw[:, 2] > raw[:, 3]).all() and (raw[:, 3] >= 2).all() and (raw[:, 2] < raw[:, 0]).all()
    assert TC.make_case((3, 7, 13), "all_empty", "valid_too", "pow2")[2].sum() == 0
    assert TC.make_case((3, 7, 13), "one_empty", "valid_too", "pow2")[2][2].sum() == 0
    assert TC.make_case((1, 1, 1), "all", "invalid_only", "none")[3] is None


def test_reduce_scalar_sums_with_twenty_names():
    from mvster_amd.graph import GraphedTrainStep
    from mvster_amd.validate import SCALAR_NAMES, reduce_scalar_sums
    names = tuple(SCALAR_NAMES) + GraphedTrainStep.BLEND_NAMES
    assert len(names) == 20 and names[-3:] == ("epe", "err3", "err1")
    g = torch.Generator().manual_seed(3)
    rows = [torch.randn(20, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(4)]
    rows[1][18] = float("nan")
    sums = torch.zeros(20, dtype=torch.float64)
    for r in rows:
        sums += r.to(torch.float64)
    got = reduce_scalar_sums(sums, torch.tensor([4], dtype=torch.int64), names=names)
    want = VC.meter_mean([r.tolist() for r in rows])
    assert list(got.keys()) == list(names)
    assert all(isinstance(got[k], float) and VC.same_float(got[k], w) for k, w in zip(names, want))
    assert math.isnan(got["err3"]) and sum(math.isnan(v) for v in got.values()) == 1
    empty = reduce_scalar_sums(torch.zeros(20, dtype=torch.float64), torch.zeros(1, dtype=torch.int64), names=names)
    assert all(math.isnan(v) for v in empty.values())
    # the default is the 17 names, and a length mismatch raises either way
    with pytest.raises(RuntimeError, match="names"):
        reduce_scalar_sums(sums, torch.tensor([4], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="names"):
        reduce_scalar_sums(torch.zeros(17, dtype=torch.float64), torch.ones(1, dtype=torch.int64), names=names)
    assert list(reduce_scalar_sums(torch.zeros(17, dtype=torch.float64), torch.ones(1, dtype=torch.int64)).keys()) == list(SCALAR_NAMES)


def _c_args(decl):
    """Argument kinds of a C declaration: 'p' pointer, 'i' int, 'l' long."""
    kinds = []
    for a in decl.split(","):
        a = a.strip()
        kinds.append("p" if "*" in a else "l" if re.match(r"(const\s+)?long\b", a) else "i" if re.match(r"(const\s+)?int\b", a) else "?")
    return kinds


def test_declarations_agree_between_header_and_binding(lib):
    from mvster_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvster_hip.h")).read()
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name in ("mvster_pooled_metrics", "mvster_scalar_gather_accumulate"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert _c_args(m.group(1)) == [kind[a] for a in _lib.SIGNATURES[name]], name
        assert hasattr(lib, name)
    # the pooled entry point takes what mvster_depth_metrics takes
    assert _lib.SIGNATURES["mvster_pooled_metrics"] == _lib.SIGNATURES["mvster_depth_metrics"]


def test_new_symbols_check_their_arguments_without_a_gpu(lib):
    """ERR_NULL / ERR_SHAPE come back before any launch; the device pointers are stand-in addresses nothing dereferences."""
    from mvster_amd import _lib
    p = 1 << 32
    thres = (ctypes.c_float * 9)(3, 1, 8, 16, 32, 64, 128, 256, 512)
    th = ctypes.cast(thres, ctypes.c_void_p)

    def pm(est=p, gt=p, mask=p, scale=None, thres=th, K=2, N=2, HW=64, partial=p, raw=p, out=p):
        return lib.mvster_pooled_metrics(est, gt, mask, scale, thres, K, N, HW, partial, raw, out, None)
    for name in ("est", "gt", "mask", "thres", "partial", "raw", "out"):
        assert pm(**{name: None}) == _lib.ERR_NULL, name
    for bad in (dict(K=0), dict(K=9), dict(K=-1), dict(N=0), dict(N=-3), dict(HW=0), dict(HW=-1), dict(N=1 << 30, HW=1 << 20)):
        assert pm(**bad) == _lib.ERR_SHAPE, bad
    table = (ctypes.c_void_p * 33)(*([p] * 33))
    tb = ctypes.cast(table, ctypes.c_void_p)
    f = lib.mvster_scalar_gather_accumulate
    assert f(None, 17, p, p, p, None) == _lib.ERR_NULL
    assert f(tb, 17, None, p, p, None) == _lib.ERR_NULL
    assert f(tb, 17, p, None, p, None) == _lib.ERR_NULL
    assert f(tb, 17, p, p, None, None) == _lib.ERR_NULL
    assert f(tb, 0, p, p, p, None) == _lib.ERR_SHAPE
    assert f(tb, 33, p, p, p, None) == _lib.ERR_SHAPE
    table[5] = None
    assert f(tb, 17, p, p, p, None) == _lib.ERR_NULL                       # a null scalar among the 17


def test_wrappers_refuse_cpu_tensors():
    from mvster_amd import ops
    x = torch.zeros(2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pooled_metrics(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scalar_gather_accumulate([torch.zeros(())] * 17, torch.zeros(17), torch.zeros(17, dtype=torch.float64),
                                     torch.zeros(1, dtype=torch.int64))


def test_summary_needs_a_keyword_the_step_has():
    import inspect
    from mvster_amd.graph import GraphedTrainStep
    sig = inspect.signature(GraphedTrainStep.__init__)
    assert sig.parameters["summary"].default is False
