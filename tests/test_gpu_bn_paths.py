"""Every path of csrc/bn_ops.hip against the float64 reference of tests/bn_cases.py: ``ops.bn_train_fwd`` / ``bn_train_bwd`` /
``bn_relu_fwd`` / ``bn_relu_bwd`` / ``col_sum`` called directly, and ``train_ops.batch_norm_cl`` on the same operands for the
cases a module can express.  tests/test_bn_cases_cpu.py shows which case reaches which path.

Guarded: the operands are views inside NaN-filled buffers and ``torch.empty`` hands out NaN-filled tensors during the calls (y,
pack, the slot buffers, dx, the sums), so an unwritten output element, an unwritten slot that is read, or a read outside a tensor
shows as NaN.  (The BatchNorm and column-sum entries do not note a kernel name: ``_lib.last_kernel()`` has nothing to assert.)

Bound, per output tensor and per element:  |got - ref64| <= 4 * e32 * max |ref64| + 2^-22 * max |ref64|
  e32  the error of PyTorch's own fp32 on the device against the same reference, relative to max |ref64| of the tensor:
       ``F.batch_norm`` under autograd, one call per group (where it refuses one row per group: the reference's own code run in
       fp32 on the device, the measure tests/test_gpu_warp_bwd_exact.py uses),
       ``torch.var_mean`` and the pack's formulas for the pack, ``x.sum(0)`` for the column sums.  Measured against PyTorch,
       never against the kernel; 4 covers another summation order; the second term is a 2-ulp floor.
Two documented limits of the training path widen that bound (DESIGN.md section 8.2 has the measurements behind both):
  pivot   The statistics are single-pass fp32 sums of (x - pivot) and (x - pivot)^2 with the group's first row as the pivot, so
          their rounding grows with r = |pivot - mean| / sqrt(var + eps), about (1 + r) in the mean and (1 + r^2) in the
          variance.  Asserted: every output of the training path keeps the bound times (1 + r)^2, r per group and channel from
          the reference (the largest r of a channel over the groups for the tensors summed over groups).
  shift   y = x * scale + shift with both operands rounded to fp32: y gets 2^-24 * (|x * scale| + |shift|) per element on top,
          half an ulp of each.  It matters where the variance is small against the mean (a constant channel: rstd = 1 /
          sqrt(eps), |shift| about 1100) and is a few percent of the bound elsewhere.
An element whose float64 activation lies within 8 * 2^-24 * (|x * scale| + |shift|) of the ReLU may fall on either side in fp32:
it is left out of the dx comparison and adds |gy| * (1 + |xhat|) to the tolerance of its group's sums.  The band is (1 + r)^2
wider too, as the activation's accuracy is; at most 8 elements per case lie in it, held by the CPU test (the pivot cases lift
their pivot channels' activations above the ReLU for that).  In the non-finite cases the bound holds on the clean channels,
which also must stay finite.
Exact: the counter, the skip gradient (gy itself), the dead channel's zeros, the same bits on a second call, the ticket pool back
at zero where a ticket is taken (the frozen backward, the column sums), and nothing written by a refused call.
parity_bn.json (beside the other parity reports) has e32 and the kernel's error
per case and tensor."""
import contextlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import bn_cases as B

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import ops
    from mvster_amd import train_ops as T
    from tests.test_gpu_conv_choice import poisoned_empty as poisoned_torch_empty
    from tests.test_gpu_warp_bwd_exact import guarded, guards_intact
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN = float("nan")
FLOOR = 2.0 ** -22
REPORT = {}
TRAIN = [c for c in B.CASES if c.kind == "train"]
FROZEN = [c for c in B.CASES if c.kind == "frozen"]
COLSUM = [c for c in B.CASES if c.kind == "colsum"]
MODULE_LEVEL_MAX = 1 << 20        # elements: batch_norm_cl runs too on every case up to this size


def note(name, **kv):
    from tests.test_gpu_wgrad import report_dir
    REPORT[name] = kv
    os.makedirs(report_dir(), exist_ok=True)
    with open(os.path.join(report_dir(), "parity_bn.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def poisoned_empty():
    """``torch.empty`` (tests/test_gpu_conv_choice.py) and ``torch.empty_like`` hand out NaN-filled float32 device tensors"""
    real = torch.empty_like

    def poisoned(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            t.fill_(NAN)
        return t
    torch.empty_like = poisoned
    try:
        with poisoned_torch_empty():
            yield
    finally:
        torch.empty_like = real


class Operands:
    """The operands of a case on the device, each a view inside its own NaN-filled buffer"""

    def __init__(self, inp):
        self.bufs = []
        for k, v in inp.items():
            if k == "frozen":
                v = tuple(self.put(t) for t in v)
            elif v is not None:
                v = self.put(v)
            setattr(self, k, v)

    def put(self, t):
        buf, view = guarded(t)
        self.bufs.append((buf, t.numel()))
        return view

    def intact(self):
        return all(guards_intact(b, n) for b, n in self.bufs)


def judge(fails, rep, key, got, want, base, sel=None, extra=None, widen=None):
    """The bound of the module docstring on one tensor; ``sel``: the elements compared; ``extra``: added to the tolerance;
    ``widen``: the factor of the pivot's distance on the bound, per element"""
    got, base = got.detach().double().cpu(), base.detach().double().cpu()
    sel = torch.ones_like(want, dtype=torch.bool) if sel is None else sel.expand_as(want)
    if not sel.any():
        return
    scale = want[sel].abs().max().item()
    e32 = (base - want)[sel].abs().max().item()
    tol = (4 * e32 + FLOOR * scale) * (1.0 if widen is None else widen) + (0.0 if extra is None else extra)
    tol = tol.expand_as(want)[sel] if torch.is_tensor(tol) else tol
    diff = (got - want)[sel].abs()
    ok = diff <= tol                        # (a NaN in ``got`` compares false)
    err = diff.max().item()
    worst = (diff / tol).max().item() if bool((torch.as_tensor(tol) > 0).all()) else (0.0 if bool(ok.all()) else float("inf"))
    rep[key] = dict(e32=e32 / scale if scale else e32, kernel=err / scale if scale else err, of_bound=worst)
    if not bool(ok.all()):
        fails.append("%s: kernel %.3g, e32 %.3g (of max |ref| %.3g), %.3g of the bound" % (key, rep[key]["kernel"], rep[key]["e32"],
                                                                                         scale, worst))


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def tickets_are_zero(taken=False):
    """The ticket pool is back at zero after a synchronize; ``taken``: a ticket was handed out, so the pool must exist"""
    torch.cuda.synchronize()
    hit = ops._TICKETS.get(DEV)
    if taken:
        assert hit is not None, "no ticket was taken from the pool of %s" % DEV
    return hit is None or int(hit[0].abs().sum()) == 0


def clean_channels(c):
    chan = torch.ones(c.C, dtype=torch.bool)
    if c.flavor == "nonfinite":
        chan[B.POISONED_CHANNEL] = False
    return chan


def dx_extra(c, ref, scale):
    """What the boundary elements of a group add to the tolerance of its dx (they move both sums by at most ``extra``)"""
    if not c.relu or not bool(ref.boundary.any()):
        return None
    e = (scale.abs() * ref.extra / c.rows).nan_to_num(0.0)                                        # [groups, C]
    return (e[:, None] * (1 + ref.xh.reshape(c.groups, c.rows, c.C).abs().nan_to_num(0.0))).reshape(ref.xh.shape)


# ---- training mode --------------------------------------------------------------------------------------------------------
def torch_fp32_train(c, d):
    """PyTorch's own fp32 on the device: F.batch_norm per group under autograd (+ ReLU, + skip), the pack from var_mean"""
    if c.rows == 1:             # (refused by F.batch_norm: the reference's own code in fp32 on the device, as the warp tests do)
        r = B.ref_train(d.x, d.gy, d.weight, d.bias, d.running_mean, d.running_var, c.eps, c.momentum, c.relu, c.groups, d.skip,
                        D=torch.float32)
        return {k: getattr(r, k) for k in ("y", "pack", "running_mean", "running_var", "dx", "dgamma", "dbeta")}
    x = d.x.detach().clone().reshape(c.groups, c.rows, c.C).requires_grad_(True)
    w, b = d.weight.clone().requires_grad_(True), d.bias.clone().requires_grad_(True)
    rm, rv = d.running_mean.clone(), d.running_var.clone()
    ys = [F.batch_norm(x[g], rm, rv, w, b, True, c.momentum, c.eps) for g in range(c.groups)]
    y = torch.stack(ys)
    y = torch.relu(y) if c.relu else y
    y.backward(d.gy.reshape(y.shape))
    if c.skip:
        y = y + d.skip.reshape(y.shape)
    var, mean = torch.var_mean(x.detach(), 1, unbiased=False)
    rstd = torch.rsqrt(var + c.eps)
    scale = d.weight * rstd
    pack = torch.stack([mean, var, rstd, scale, d.bias - mean * scale])
    return dict(y=y.detach().reshape(d.x.shape), pack=pack, running_mean=rm, running_var=rv, dx=x.grad.reshape(d.x.shape),
                dgamma=w.grad, dbeta=b.grad)


def judge_train(c, ref, base, got, tag, fails, rep):
    chan = clean_channels(c)
    extra = ref.extra.nan_to_num(0.0).sum(0) if c.relu else None
    # the documented limit of the single-pass statistics (module docstring): (1 + r)^2 per group and channel
    wg = (1 + ref.pivot.nan_to_num(0.0)) ** 2                                                    # [groups, C]
    wx = wg[:, None, :].expand(c.groups, c.rows, c.C).reshape(ref.y.shape)
    wc = wg.max(0)[0]
    rep[tag + "pivot_distance"] = dict(max=ref.pivot.nan_to_num(0.0).max().item())
    shift = ref.pack[4][:, None, :]
    y_extra = 2.0 ** -24 * ((ref.act.reshape(c.groups, c.rows, c.C) - shift).abs() + shift.abs()).nan_to_num(0.0)
    judge(fails, rep, tag + "y", got["y"], ref.y, base["y"], chan, y_extra.reshape(ref.y.shape), wx)
    judge(fails, rep, tag + "running_mean", got["running_mean"], ref.running_mean, base["running_mean"], chan, None, wc)
    judge(fails, rep, tag + "running_var", got["running_var"], ref.running_var, base["running_var"], chan, None, wc)
    judge(fails, rep, tag + "dx", got["dx"], ref.dx, base["dx"], chan & ~ref.boundary, dx_extra(c, ref, ref.pack[3]), wx)
    judge(fails, rep, tag + "dgamma", got["dgamma"], ref.dgamma, base["dgamma"], chan, extra, wc)
    judge(fails, rep, tag + "dbeta", got["dbeta"], ref.dbeta, base["dbeta"], chan, extra, wc)
    if "pack" in got:
        for i, name in enumerate(("mean", "var", "rstd", "scale", "shift")):
            judge(fails, rep, tag + name, got["pack"][i], ref.pack[i], base["pack"][i], chan, None, wg)
    if c.flavor == "dead" and c.relu:
        for k in ("dx", "dgamma", "dbeta"):
            if not bool((got[k][..., B.DEAD_CHANNEL] == 0).all()):
                fails.append(tag + k + ": the dead channel is not exactly zero")


@pytest.mark.parametrize("c", TRAIN, ids=lambda c: c.name)
def test_training_paths_vs_fp64(c):
    inp, ref = B.reference(c)
    d = Operands(inp)
    fails, rep = [], {}

    def run():
        state = Operands(dict(rm=inp["running_mean"], rv=inp["running_var"]))
        nbt = torch.full((), 7, device=DEV, dtype=torch.int64)
        with poisoned_empty():
            y, pack = ops.bn_train_fwd(d.x, d.weight, d.bias, state.rm, state.rv, c.eps, c.momentum, c.relu, c.groups, nbt, d.skip)
            dx, dbeta, dgamma = ops.bn_train_bwd(d.x, d.gy, pack, c.relu, c.groups)
        torch.cuda.synchronize()
        assert state.intact() and d.intact()
        assert int(nbt) == 7 + c.groups
        return dict(y=y, pack=pack, running_mean=state.rm, running_var=state.rv, dx=dx, dgamma=dgamma, dbeta=dbeta)

    got = run()
    again = run()
    for k in got:
        assert same_bits(got[k], again[k]), "%s differs on a second call" % k
    del again
    base = torch_fp32_train(c, d)
    judge_train(c, ref, base, got, "", fails, rep)
    if inp["x"].numel() <= MODULE_LEVEL_MAX:
        bn = torch.nn.BatchNorm3d(c.C, eps=c.eps, momentum=c.momentum).to(DEV).train()
        with torch.no_grad():
            for name in ("weight", "bias", "running_mean", "running_var"):
                getattr(bn, name).copy_(inp[name])
        x = d.x.reshape(c.groups, c.rows, c.C).requires_grad_(True)
        sk = d.skip.reshape(x.shape).requires_grad_(True) if c.skip else None
        with poisoned_empty():
            y = T.batch_norm_cl(x, bn, relu=c.relu, groups=c.groups, skip=sk)
            y.backward(d.gy.reshape(x.shape))
        assert int(bn.num_batches_tracked) == c.groups
        if c.skip:
            assert same_bits(sk.grad, d.gy.reshape(x.shape)), "the skip gradient is not gy itself"
        mod = dict(y=y.detach().reshape(d.x.shape), running_mean=bn.running_mean, running_var=bn.running_var,
                   dx=x.grad.reshape(d.x.shape), dgamma=bn.weight.grad, dbeta=bn.bias.grad)
        for k, v in mod.items():
            assert same_bits(v.contiguous(), got[k]), "batch_norm_cl and the direct calls differ in %s" % k
        assert d.intact()
    note(c.name, **rep)
    assert not fails, "\n".join(fails)


def test_pairs_refused_writes_nothing():
    """groups * 2C = 2176 > 2048: RuntimeError from both passes, and y, pack, the slot buffer, dx, the sums (every tensor the
    call allocated, NaN-filled), the running statistics and the counter are untouched after a synchronize."""
    c = B.BY_NAME["pairs_refused"]
    d = Operands(B.make_inputs(c))
    before = d.running_mean.clone(), d.running_var.clone()
    nbt = torch.full((), 7, device=DEV, dtype=torch.int64)
    made = []
    real = torch.empty, torch.empty_like

    def recording(alloc):
        def wrapped(*a, **k):
            t = alloc(*a, **k)
            t.fill_(NAN)
            made.append(t)
            return t
        return wrapped
    torch.empty, torch.empty_like = recording(real[0]), recording(real[1])
    try:
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.bn_train_fwd(d.x, d.weight, d.bias, d.running_mean, d.running_var, c.eps, c.momentum, True, c.groups, nbt)
        pack = torch.ones(5, c.groups, c.C, device=DEV)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.bn_train_bwd(d.x, d.gy, pack, True, c.groups)
        scale = torch.ones(c.groups, c.C, device=DEV)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.bn_relu_bwd(d.x, d.gy, scale, scale, scale, scale, True, c.groups)
    finally:
        torch.empty, torch.empty_like = real
    torch.cuda.synchronize()
    assert len(made) >= 9 and all(bool(t.isnan().all()) for t in made)
    assert same_bits(d.running_mean, before[0]) and same_bits(d.running_var, before[1]) and int(nbt) == 7
    assert d.intact() and tickets_are_zero()
    bn = torch.nn.BatchNorm3d(c.C).to(DEV).train()
    with pytest.raises(RuntimeError, match="unsupported"):
        T.batch_norm_cl(d.x.reshape(c.groups, c.rows, c.C), bn, relu=True, groups=c.groups)
    assert int(bn.num_batches_tracked) == 0


def test_groups_must_divide_the_leading_dimension():
    """7 slices cannot form 2 or 3 equal groups: RuntimeError from every entry (the trailing rows used to stay unwritten and
    outside the statistics), nothing written."""
    x = torch.randn(7, 5, 8, device=DEV)
    gy = torch.randn(7, 5, 8, device=DEV)
    w, b = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    rm, rv = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    for groups in (2, 3, 0):
        per = torch.ones(max(groups, 1), 8, device=DEV)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_train_fwd(x, w, b, rm, rv, 1e-5, 0.1, True, groups)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_train_bwd(x, gy, torch.ones(5, max(groups, 1), 8, device=DEV), True, groups)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_relu_fwd(x, per, per, True, groups)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_relu_bwd(x, gy, per, per, per, per, True, groups)
        for train in (True, False):
            bn = torch.nn.BatchNorm3d(8).to(DEV).train(train)
            with pytest.raises(RuntimeError, match="does not divide"):
                T.batch_norm_cl(x, bn, relu=True, groups=groups)
            assert int(bn.num_batches_tracked) == 0
    torch.cuda.synchronize()
    assert bool((rm == 0).all()) and bool((rv == 1).all())
    y, _ = ops.bn_train_fwd(x, w, b, rm, rv, 1e-5, 0.1, True, 7)             # (7 groups of 5 rows do divide)
    assert bool(torch.isfinite(y).all())


# ---- constant statistics (a BatchNorm in eval mode inside a training graph) ---------------------------------------------------
def torch_fp32_frozen(c, d, mean, rstd, scale, shift):
    """PyTorch's own fp32 on the device: the activation under autograd for dx, the two sums in plain ops"""
    x = d.x.detach().clone().reshape(c.groups, c.rows, c.C).requires_grad_(True)
    gy = d.gy.reshape(x.shape)
    act = x * scale[:, None] + shift[:, None]
    y = torch.relu(act) if c.relu else act
    dx, = torch.autograd.grad(y, x, gy)
    g = gy * (act.detach() > 0) if c.relu else gy
    xh = (x.detach() - mean[:, None]) * rstd[:, None]
    y = y.detach() + d.skip.reshape(y.shape) if c.skip else y.detach()
    return dict(y=y.reshape(d.x.shape), dx=dx.reshape(d.x.shape), dgamma=(g * xh).sum((0, 1)), dbeta=g.sum((0, 1)))


def judge_frozen(c, ref, base, got, tag, fails, rep):
    judge(fails, rep, tag + "y", got["y"], ref.y, base["y"])
    judge(fails, rep, tag + "dx", got["dx"], ref.dx, base["dx"], ~ref.boundary)
    extra = ref.extra.sum(0) if c.relu else None
    judge(fails, rep, tag + "dgamma", got["dgamma"], ref.dgamma, base["dgamma"], None, extra)
    judge(fails, rep, tag + "dbeta", got["dbeta"], ref.dbeta, base["dbeta"], None, extra)


@pytest.mark.parametrize("c", FROZEN, ids=lambda c: c.name)
def test_frozen_paths_vs_fp64(c):
    inp, ref = B.reference(c)
    d = Operands(inp)
    mean, rstd, scale, shift = d.frozen
    fails, rep = [], {}

    def run():
        with poisoned_empty():
            y = ops.bn_relu_fwd(d.x, scale, shift, c.relu, c.groups, d.skip)
            dx, dbeta, dgamma = ops.bn_relu_bwd(d.x, d.gy, scale, shift, mean, rstd, c.relu, c.groups)
        assert tickets_are_zero(taken=True) and d.intact()
        return dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta)

    got = run()
    again = run()
    for k in got:
        assert same_bits(got[k], again[k]), "%s differs on a second call" % k
    del again
    judge_frozen(c, ref, torch_fp32_frozen(c, d, mean, rstd, scale, shift), got, "", fails, rep)
    # the module: eval mode, group 0's constants as its running statistics, the same for every group
    bn = torch.nn.BatchNorm3d(c.C, eps=c.eps).to(DEV).eval()
    with torch.no_grad():
        bn.weight.copy_(inp["weight"])
        bn.bias.copy_(inp["bias"])
        bn.running_mean.copy_(inp["frozen"][0][0])
        bn.running_var.copy_(1 / inp["frozen"][1][0].double() ** 2 - c.eps)
    m64, v64 = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    r64 = 1 / (v64 + c.eps).sqrt()
    s64 = inp["weight"].double() * r64
    per = [t.expand(c.groups, c.C) for t in (m64, r64, s64, inp["bias"].double() - m64 * s64)]
    mref = B.ref_frozen(inp["x"], inp["gy"], *per, c.relu, c.groups, inp["skip"])
    x = d.x.reshape(c.groups, c.rows, c.C).requires_grad_(True)
    sk = d.skip.reshape(x.shape).requires_grad_(True) if c.skip else None
    with poisoned_empty():
        y = T.batch_norm_cl(x, bn, relu=c.relu, groups=c.groups, skip=sk)
        y.backward(d.gy.reshape(x.shape))
    if c.skip:
        assert same_bits(sk.grad, d.gy.reshape(x.shape)), "the skip gradient is not gy itself"
    assert int(bn.num_batches_tracked) == 0 and same_bits(bn.running_mean.cpu(), inp["frozen"][0][0])
    mod = dict(y=y.detach().reshape(d.x.shape), dx=x.grad.reshape(d.x.shape), dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    perdev = [t.float().to(DEV) for t in per]
    judge_frozen(c, mref, torch_fp32_frozen(c, d, *perdev), mod, "module.", fails, rep)
    assert tickets_are_zero(taken=True) and d.intact()
    note(c.name, **rep)
    assert not fails, "\n".join(fails)


# ---- column sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", COLSUM, ids=lambda c: c.name)
def test_col_sum_paths_vs_fp64(c):
    inp = B.make_inputs(c)
    want = B.ref_col_sum(inp["x"])
    d = Operands(dict(x=inp["x"]))
    fails, rep = [], {}
    with poisoned_empty():
        got = ops.col_sum(d.x)
        again = ops.col_sum(d.x)
    assert tickets_are_zero(taken=True) and d.intact()
    assert got.shape == (c.C,) and same_bits(got, again)
    judge(fails, rep, "sum", got, want, d.x.sum(0))
    # a 5-D view of the same memory (what a convolution's output gradient looks like) gives the same bits
    if c.rows % 3 == 0:
        assert same_bits(ops.col_sum(d.x.reshape(1, 3, c.rows // 3, 1, c.C)), got)
    note(c.name, **rep)
    assert not fails, "\n".join(fails)
