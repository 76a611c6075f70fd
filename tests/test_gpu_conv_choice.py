"""The kernel the convolution plan ITSELF picks (``ConvLayer.__call__`` without ``tiles``), at sizes nobody tuned, against the
float64 tap loop of tests/conv_choice_cases.py -- for every layer form of the shipped networks, in its eval role and, through
``train_ops.conv_cl``, in its training role (forward, input gradient, in-place weight update).

Exact: integer operands (x, w, skip in {-2..2}, scale in {0.5, 1, 2}, integer shift / head / gradients) keep every partial
sum of every kernel exactly representable (tests/test_conv_choice_cpu.py has the budget, and the float32 restatement of
Winograd F(2x2, 3x3) that extends the claim to variants 8 / 9), so the result must be the float64 one bit for bit.  Guarded:
x and skip are views inside NaN-filled buffers and ``torch.empty`` hands out NaN-filled tensors during the call, so a read
outside a tensor or an unwritten output element shows as NaN.  Named: ``_lib.last_kernel()`` must belong to the family of the
variant word ``_geom`` chose; the direct kernel in its place is the library's "unsupported" answer, tolerated (and reported)
only for a choice the measured table's FAMILY lookup carried over from another shape, never for a heuristic one.  Both plan
modes of the case table run: "shipped" (table + families + heuristics) and "heuristic" (table and families emptied)."""
import contextlib
import json
import os

import pytest
import torch

from tests import conv_choice_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import _lib
    from mvster_amd import conv_plan as cp
    from mvster_amd import train_ops as T
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN = float("nan")
REPORT = {}
EVAL_FORMS = C.unique_forms()
TRAIN_FORMS = [f for f in C.FORMS if f.role == "train" and f.name != "t_fpn_fine_g"]       # (72 outputs: not a conv_cl layer)


def write_report():
    from tests.test_gpu_wgrad import report_dir
    os.makedirs(report_dir(), exist_ok=True)
    with open(os.path.join(report_dir(), "parity_conv_choice.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def guarded(t):
    """A contiguous device copy of ``t`` inside a NaN-filled buffer: more than one full W * C row of NaN on either side."""
    guard = -(-t.shape[-2] * t.shape[-1] // 64) * 64 + 64
    buf = torch.full((t.numel() + 2 * guard,), NAN, device=DEV, dtype=torch.float32)
    view = buf[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


@contextlib.contextmanager
def plan_mode(mode):
    saved = cp._TUNING, cp._FAMILIES
    cp._TUNING, cp._FAMILIES = ({}, {}) if mode == "heuristic" else (None, None)
    try:
        yield
    finally:
        cp._TUNING, cp._FAMILIES = saved


@contextlib.contextmanager
def poisoned_empty():
    """float32 device allocations of ``torch.empty`` come back NaN-filled."""
    real = torch.empty

    def poisoned(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            t.fill_(NAN)
        return t
    torch.empty = poisoned
    try:
        yield
    finally:
        torch.empty = real


def judge_name(name, layer, shape, sm, mode, where, fails):
    """Check (b): -> (variant word, how, fallback)."""
    v, mt, nt, how = C.effective_choice(layer, shape, sm)
    fallback = False
    if not C.names_family(name, v):
        if C.is_direct_fallback(name, v) and mode == "shipped" and how == "family":
            fallback = True
        else:
            fails.append("%s: variant 0x%x (%s) ran %s" % (where, v, how, name))
    return v, how, fallback


def bound_for(v, fallback):
    """Check (c): 2e-5 of max |y| (test_conv_bn_relu, the direct-edges test); the Winograd kernels' own bound is 2e-6
    (test_winograd_conv_against_fp64_and_direct)."""
    return 2e-6 if (v & 0xff) in (8, 9) and not fallback else 2e-5


@pytest.mark.parametrize("f", EVAL_FORMS, ids=[f.name for f in EVAL_FORMS])
def test_eval_role_choice_is_exact_guarded_and_named(f):
    fails, rep = [], {}
    for shape in f.ladder:
        for exact in (True, False):
            d = C.case_data(f, shape, DEV, exact)
            base = C.conv_ref64(d["x"][..., :f.cin], d["w"], f.stride, f.padding, f.transposed)
            xbuf, x = guarded(d["x"]) if exact else (None, d["x"])
            for mode in C.MODES:
                with plan_mode(mode):
                    layer = C.make_layer(f, d["w"], d["prob"])
                    layer.scale[:f.cout] = d["scale"]
                    layer.shift[:f.cout] = d["shift"]
                    for sm in f.skips:
                        where = "%s %s sk%d %s" % ("x".join(map(str, shape)), mode, sm, "exact" if exact else "randn")
                        skip = d["skip"].get(sm)
                        ref = C.epilogue64(base, d["scale"], d["shift"], f.relu, skip, sm, d["prob"])
                        scale = ref.abs().max().item()
                        if sm == C.SKIP_UPSAMPLE_ADD:
                            # bilinear weights are not dyadic: the bound only, for the plan's choice and for the direct kernel
                            if exact:
                                continue
                            got = layer(x, skip=skip, skip_mode=sm)
                            name = _lib.last_kernel()
                            v, how, fb = judge_name(name, layer, shape, sm, mode, where, fails)
                            err = (got.double() - ref).abs().max().item() / scale
                            lat = shape if f.transposed else C.out_shape(f, shape)
                            mt, nt = cp._tiles(lat[0] * lat[1] * lat[2] * lat[3], layer.ntile_total, 1)
                            direct = layer(x, skip=skip, skip_mode=sm, tiles=(mt, nt, 0))
                            e_dir = (direct.double() - ref).abs().max().item() / scale
                            if not _lib.last_kernel().startswith("conv_mfma_kernel<"):
                                fails.append("%s: tiles=(.., 0) ran %s" % (where, _lib.last_kernel()))
                            rep[where] = dict(kernel=name, variant="0x%x" % v, how=how, fallback=fb, err=err, direct_err=e_dir)
                            if not (err <= 2e-5 and e_dir <= 2e-5):
                                fails.append("%s: err %g, direct %g" % (where, err, e_dir))
                            continue
                        sk = guarded(skip)[1] if (exact and skip is not None) else skip
                        with poisoned_empty() if exact else contextlib.nullcontext():
                            got = layer(x, skip=sk, skip_mode=sm)
                        name = _lib.last_kernel()
                        v, how, fb = judge_name(name, layer, shape, sm, mode, where, fails)
                        want_shape = tuple(C.out_shape(f, shape)) + (() if f.prob else (f.cout,))
                        if tuple(got.shape) != want_shape:
                            fails.append("%s: shape %s" % (where, tuple(got.shape)))
                            continue
                        g64 = got.double()
                        err = (g64 - ref).abs().max().item() / max(scale, 1e-30)
                        rep[where] = dict(kernel=name, variant="0x%x" % v, how=how, fallback=fb, err=err)
                        if exact:
                            nan = int(g64.isnan().sum().item())
                            if nan:
                                fails.append("%s: %d NaN of %d on %s (a read outside a tensor or an unwritten element)"
                                             % (where, nan, g64.numel(), name))
                            elif not torch.equal(got, ref.float()):
                                fails.append("%s: max |got - ref| = %g on %s" % (where, (g64 - ref).abs().max().item(), name))
                        elif not err <= bound_for(v, fb):
                            fails.append("%s: err %g > %g on %s" % (where, err, bound_for(v, fb), name))
            if exact:
                # the operand is read-only: the data and its guards are as they were
                n = d["x"].numel()
                if not (torch.equal(x, d["x"]) and xbuf[:(xbuf.numel() - n) // 2].isnan().all() and xbuf[(xbuf.numel() + n) // 2:].isnan().all()):
                    fails.append("%s: the input or its guards were written" % "x".join(map(str, shape)))
    torch.cuda.synchronize()
    REPORT["eval " + f.name] = rep
    write_report()
    assert not fails, "%d failures, first: %s" % (len(fails), fails[:8])


@pytest.mark.parametrize("f", TRAIN_FORMS, ids=[f.name for f in TRAIN_FORMS])
def test_training_role_forward_input_gradient_and_repack(f, monkeypatch):
    """``T.conv_cl(..., tap=True)`` on the integer data: y and x.grad equal float64 autograd through the tap loop exactly, with
    and without a gradient flowing into the tap (the input-gradient layer's SKIP_ADD and SKIP_NONE calls), before and after
    ``w.mul_(2)`` -- the second round runs on what ``repack_on_device`` made of every packed form the two layers hold (wpk,
    wpk_wino, w_small, w_small4, w_deconv / parity classes), so a stale one shows.  The kernels are named as in the eval role;
    the launches are recorded on the thread that makes them (the backward pass runs on autograd's)."""
    calls = []
    orig = cp.ConvLayer.__call__

    def spy(self, x, skip=None, skip_mode=cp.SKIP_NONE, tiles=None):
        out = orig(self, x, skip=skip, skip_mode=skip_mode, tiles=tiles)
        calls.append((self, tuple(x.shape[:4]), skip_mode if skip is not None else cp.SKIP_NONE, _lib.last_kernel()))
        return out
    monkeypatch.setattr(cp.ConvLayer, "__call__", spy)
    wants_dx = f.name not in C.NO_DGRAD
    fails, rep = [], {}
    for shape in f.ladder:
        g = torch.Generator(device=DEV).manual_seed(sum(map(ord, f.name)) + 11 * sum(shape))
        ints = lambda s, m: torch.randint(-m, m + 1, s, generator=g, device=DEV).float()
        x0 = ints(tuple(shape) + (f.cin,), 2)
        w0 = ints(C.weight_shape(f), 2)
        bias = ints((f.cout,), 3) if f.bias else None
        gy = guarded(ints(tuple(C.out_shape(f, shape)) + (f.cout,), 2))[1]
        gtap = guarded(ints(tuple(shape) + (f.cin,), 2))[1]
        xr = x0.double().requires_grad_(wants_dx)
        yc = C.conv_ref64(xr, w0, f.stride, f.padding, f.transposed)
        dxc = torch.autograd.grad(yc, xr, gy.double())[0] if wants_dx else None
        yc = yc.detach()
        for mode in C.MODES:
            with plan_mode(mode):
                T.CACHE.clear()
                w = w0.clone()
                for factor in (1, 2):
                    if factor == 2:
                        w.mul_(2)
                    for tap in (False, True):
                        where = "%s %s x%d %s" % ("x".join(map(str, shape)), mode, factor, "tap" if tap else "notap")
                        x = guarded(x0)[1].requires_grad_(wants_dx)
                        del calls[:]
                        with poisoned_empty():
                            y, xt = T.conv_cl(x, w, bias, f.stride, f.padding, f.transposed, tap=True)
                            if wants_dx:
                                torch.autograd.backward([y, xt] if tap else [y], [gy, gtap] if tap else [gy])
                        torch.cuda.synchronize()
                        want_y = factor * yc + (0 if bias is None else bias.double())
                        if y.isnan().any() or not torch.equal(y.detach(), want_y.float()):
                            fails.append("%s: forward max |got - ref| = %g on %s" % (where, (y.detach().double() - want_y).abs().max().item(), calls[0][3]))
                        if wants_dx:
                            want_dx = factor * dxc + (gtap.double() if tap else 0)
                            if x.grad is None or x.grad.isnan().any() or not torch.equal(x.grad, want_dx.float()):
                                fails.append("%s: x.grad max |got - ref| = %s on %s"
                                             % (where, None if x.grad is None else (x.grad.double() - want_dx).abs().max().item(), calls[-1][3]))
                        if len(calls) != (2 if wants_dx else 1):
                            fails.append("%s: %d layer calls" % (where, len(calls)))
                            continue
                        rec = {}
                        for role, (layer, lshape, sm, name) in zip(("fwd", "dgrad"), calls):
                            if role == "dgrad" and sm != (cp.SKIP_ADD if tap else cp.SKIP_NONE):
                                fails.append("%s: the tap's gradient was not fused (skip mode %d)" % (where, sm))
                            v, how, fb = judge_name(name, layer, lshape, sm, mode, where + " " + role, fails)
                            rec[role] = dict(kernel=name, variant="0x%x" % v, how=how, fallback=fb)
                        rep[where] = rec
    T.CACHE.clear()
    REPORT["train " + f.name] = rep
    write_report()
    assert not fails, "%d failures, first: %s" % (len(fails), fails[:8])


def _layers_of(obj):
    """Every ConvLayer an eval plan holds (attributes and lists of attributes)."""
    out = []
    for v in vars(obj).values():
        for item in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(item, cp.ConvLayer):
                out.append(item)
    return out


def test_every_layer_the_networks_build_has_its_form_in_the_table():
    """Drift guard: each ``ConvLayer`` of the three eval plans, and of ``train_ops.CACHE`` after one small training step of the
    shipped configuration, is a form of the case table -- a new layer (or a changed channel padding, kernel, stride, fused
    head) must be added there, with a ladder, before the suite is green again."""
    from mvster_amd import MVS4net, MVS4net_loss
    from mvster_amd import modules as M
    from mvster_amd.synthetic import make_inputs, randomize_state
    keys = {C.form_key(f): f.name for f in C.FORMS}
    cfg = dict(arch_mode="fpn", reg_net="reg2d", num_stage=4, fpn_base_channel=8, reg_channel=8, stage_splits=[8, 8, 4, 4],
               depth_interals_ratio=[0.5, 0.5, 0.5, 1], group_cor=True, group_cor_dim=[8, 8, 4, 4], inverse_depth=True,
               mono=True, attn_temp=2, attn_fuse_d=True)
    torch.manual_seed(3)
    model = MVS4net(**cfg)
    model.load_state_dict(randomize_state(model.state_dict(), seed=5, prob_gain=4.0))
    model.to(DEV).train()
    H, W, N, B = 64, 128, 3, 2
    imgs, proj, dv = make_inputs(nviews=N, H=H, W=W, seed=4, batch=B)
    imgs = [i.to(DEV) for i in imgs]
    proj = {k: v.to(DEV) for k, v in proj.items()}
    g = torch.Generator().manual_seed(0)
    gt = {"stage%d" % s: (500 + 300 * torch.rand(B, H // 2 ** (4 - s), W // 2 ** (4 - s), generator=g)).to(DEV) for s in range(1, 5)}
    mask = {k: torch.ones_like(v) for k, v in gt.items()}
    T.CACHE.clear()
    out = model(imgs, proj, dv.to(DEV))
    MVS4net_loss(out, gt, mask, stage_lw=[1, 1, 1, 1], l1ot_lw=[0, 1], inverse_depth=True, ot_iter=10, ot_eps=1,
                 ot_continous=False, mono=True)[0].backward()
    torch.cuda.synchronize()
    trained = [hit[2] for hit in T.CACHE._d.values()]
    assert len(trained) >= 60, len(trained)
    T.CACHE.clear()
    model.eval()
    fpn, regs = model._get_plans()
    plans = [fpn] + list(regs)
    for down in (3, 2):
        plans.append(cp.Reg3dPlan(M.reg3d(in_channels=8, base_channels=8, down_size=down).to(DEV).eval()))
    planned = [layer for p in plans for layer in _layers_of(p)]
    assert len(planned) >= 17 + 4 * 10 + 2 * 9, len(planned)
    unknown = sorted({str(C.layer_key(layer)) for layer in trained + planned if C.layer_key(layer) not in keys})
    assert not unknown, unknown
    # and the table lists nothing the networks do not build (a form that left the product leaves the table)
    built = {C.layer_key(layer) for layer in trained + planned} | {C.layer_key(layer) for layer in _layers_of(cp.Reg2dPlan(model.reg[0], fuse_prob_into_conv11=False))}
    stale = sorted(name for k, name in keys.items() if k not in built)
    assert not stale, stale
