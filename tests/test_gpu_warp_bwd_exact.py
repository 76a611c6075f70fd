"""The warp backward (csrc/warp_bwd.hip) against the fp64 reference of tests/warp_exact_cases.py, on scenes whose sampling
positions are exact in fp32: the error measured here is the backward's arithmetic, not coordinate noise, and every edge of
the kernel file is in a scene on purpose (tests/test_warp_exact_cpu.py counts them).

Bound, per gradient tensor and per element:  |got - ref64| <= 4 * e32 * max |ref64| + n * bound * 2^-37
  e32    the error of the SAME reference code run in fp32 on the device by PyTorch, relative to max |ref64| of the tensor
         (measured against PyTorch, never against the kernel; 4 covers another summation order and expf),
  bound  make_fix_scale's largest single contribution, restated on the host from the operand maxima,
  n      the additions the element's fixed-point counter receives: D * NV for a reference pixel, the weighted taps on a source
         texel (+ 1 per scatter window covering it in the gather and atomic forms); half a unit of the documented
         resolution each.
Texels no weighted tap touches must be exactly 0.0.  Operands are views inside NaN-filled guard buffers; the gradient
buffers go in NaN-filled (g_src of the window forms zeroed, as documented); ``_lib.last_kernel()`` is pinned per form.

Worst figures on an MI355X, relative to max |ref64| of the tensor, over all cases and forms (parity_warp_bwd.json has them per
case and form):
  unit variance   g_ref  e32 1.8e-6  kernel 5.3e-6 (tile_corner-sq64d3)     g_src  e32 2.1e-6  kernel 6.1e-6 (border-sq64d3)
                  out    e32 8.2e-7  kernel 2.2e-6                          wsum   e32 1.3e-6  kernel 3.2e-6
                  group correlation stays at 1e-7 .. 4e-7 (shift-c8g4d4: g_ref 1.1e-7, g_src 1.1e-7); the squared differences
                  over 64 channels are the worst of both PyTorch and the kernel, and the closest to the bound: border-sq64d3
                  g_ref uses 0.996 of it (4.14e-6 of 2.31e-6 + 1.85e-6), the next case 0.63.
  heavy tail      g_ref  e32 3.3e-7  kernel 1.6e-4 (minify-c32g8d8)         g_src  e32 7.9e-7  kernel 2.9e-4 (minify-c32g8d8)
                  i.e. one feature of 64 among unit-variance ones costs 100 .. 1000 x in the gradients (shift-c8g4d4: g_ref
                  1.1e-7 -> 1.6e-5, g_src 1.1e-7 -> 2.1e-5; minify-c32g8d8: 1.4e-7 -> 1.6e-4, 4.1e-7 -> 2.9e-4): the bound
                  grows 3000 x (max |feature|^3) and the resolution is absolute.  At most 0.48 of the derived bound.
What the file found when it was written: fmaxf in make_fix_scale dropped a NaN feature maximum (a non-finite ref or src gave
finite gradients in all forms); the window forms left zeros in g_src where no tap or window reached; one unit of the
counters was up to twice the documented bound * 2^-36 (the heavy-tail cases and border-sq64d3 exceeded the bound by it)."""
import ctypes
import json
import os

import pytest
import torch

from tests import warp_exact_cases as WX

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import _lib, ops
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN = float("nan")
FORMS = ("sorted", "gather", "atomic")
REPORT = {}


def report_dir():
    """beside the other parity reports (tests/test_gpu_wgrad.py)"""
    from tests import test_gpu_wgrad
    return test_gpu_wgrad.report_dir()


def note(name, **kv):
    REPORT[name] = kv
    os.makedirs(report_dir(), exist_ok=True)
    with open(os.path.join(report_dir(), "parity_warp_bwd.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def guarded(t, fill=None):
    """A contiguous device copy of ``t`` (or ``fill`` in its shape) inside a NaN-filled buffer, 16-byte aligned"""
    guard = 256
    buf = torch.full((t.numel() + 2 * guard,), NAN, device=DEV, dtype=torch.float32)
    view = buf[guard:guard + t.numel()].view(t.shape)
    if fill is None:
        view.copy_(t)
    else:
        view.fill_(fill)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, n):
    g = (buf.numel() - n) // 2
    return bool(buf[:g].isnan().all() and buf[g + n:].isnan().all())


class Run:
    """The operands of a case on the device, its forward, and the backward in any form"""

    def __init__(self, sc, cfg, ref, src, gout):
        self.sc, self.cfg = sc, cfg
        self.G = cfg.G if cfg.group else cfg.C
        self.bufs = []
        self.ref, self.src, self.rt, self.hypo = (self.put(t) for t in (ref, src, sc.rt, sc.hypo))
        self.gout = self.put(gout)
        self.out, self.wsum = ops.warp_agg_fwd_cl(self.ref, self.src, self.rt, self.hypo, self.G, cfg.group, cfg.fuse, WX.ATTN_TEMP,
                                                  want_wsum=True)

    def put(self, t):
        buf, view = guarded(t)
        self.bufs.append((buf, t.numel()))
        return view

    def backward(self, form, gout=None):
        gb, g_ref = guarded(self.ref, fill=NAN)
        sb, g_src = guarded(self.src, fill=NAN if form == "sorted" else 0.0)
        got = ops.warp_agg_bwd_cl(self.ref, self.src, self.rt, self.hypo, self.out, self.wsum, self.gout if gout is None else gout,
                                  self.G, self.cfg.group, self.cfg.fuse, WX.ATTN_TEMP, deterministic=form == "gather",
                                  sorted_scatter=form == "sorted", into=(g_ref, g_src))
        name = _lib.last_kernel()
        assert got[0] is g_ref and got[1] is g_src
        assert name == WX.first_pass_kernel(self.cfg, form), (form, name)
        assert guards_intact(gb, g_ref.numel()) and guards_intact(sb, g_src.numel()), "a store outside the gradients (%s)" % form
        return g_ref, g_src

    def operands_intact(self):
        return all(guards_intact(b, n) for b, n in self.bufs)


def tolerances(sc, cfg, ref, src, gout, want, base):
    """-> e32 and the two bound terms per gradient tensor: {"ref"/"src": (e32, first term, second term per element and form)}"""
    bound = WX.fix_bound(gout.abs().max().item(), ref.abs().max().item(), src.abs().max().item(), cfg)
    unit = bound * 2.0 ** -37
    n_src = WX.contributions(sc).double()
    cover = WX.windows(sc, "tile" if WX.uses_tiles(cfg) else "row").cover.double()
    tol = {}
    for key, w, b, n in (("ref", want[2], base[2], torch.full(want[2].shape[:3], float(sc.D * sc.NV), dtype=torch.float64)),
                         ("src", want[3], base[3], n_src)):
        scale = w.abs().max().item()
        e32 = (b - w).abs().max().item() / scale
        second = {f: ((n + (cover if key == "src" and f != "sorted" else 0)) * unit).unsqueeze(-1) for f in FORMS}
        tol[key] = (e32, 4 * e32 * scale, second, scale)
    return tol, n_src, bound


def check_case(tag, sc, cfg, ref, src, gout, want):
    """forward, the three backward forms against fp64 with the two-term bound, exact zeros -> the figures of the case"""
    base = WX.gradients(ref, src, sc.rt, sc.hypo, gout, cfg, torch.float32, device=DEV)
    run = Run(sc, cfg, ref, src, gout)
    fig = {}
    # 1. forward: as below without the fixed-point term
    for key, got, w, b in (("out", run.out, want[0], base[0]), ("wsum", run.wsum, want[1], base[1])):
        scale = w.abs().max().item()
        e32 = (b - w).abs().max().item() / scale
        err = (got.cpu().double() - w).abs().max().item() / scale
        fig[key] = {"e32": e32, "kernel": err}
        print(tag, key, "e32 %.3g kernel %.3g" % (e32, err))
    tol, n_src, bound = tolerances(sc, cfg, ref, src, gout, want, base)
    fig["bound"] = bound
    bad = []
    for form in FORMS:
        g_ref, g_src = run.backward(form)
        for key, got, w in (("ref", g_ref, want[2]), ("src", g_src, want[3])):
            e32, first, second, scale = tol[key]
            g = got.cpu().double()
            diff = (g - w).abs()
            allowed = first + second[form]
            fig["%s_%s" % (form, key)] = {"e32": e32, "kernel": diff.max().item() / scale, "term_fp32": first / scale,
                                           "term_fixed_max": second[form].max().item() / scale}
            print(tag, form, key, "e32 %.3g kernel %.3g terms %.3g + %.3g" % (e32, diff.max().item() / scale, first / scale,
                                                                             second[form].max().item() / scale))
            if not bool((diff <= allowed).all()):      # (a NaN fails)
                bad.append("%s %s: %d elements beyond the bound, worst excess %.3g of max|ref64|" % (
                    form, key, int((~(diff <= allowed)).sum()), ((diff - allowed).max().item() / scale)))
        # 3. exact zeros: texels no weighted tap touches
        untouched = (n_src == 0).unsqueeze(-1).expand_as(want[3])
        if not bool((g_src.cpu()[untouched] == 0).all()):
            bad.append("%s src: an untouched texel is not exactly 0" % form)
    assert run.operands_intact()
    note(tag, **fig)
    for key in ("out", "wsum"):
        assert fig[key]["kernel"] <= 4 * fig[key]["e32"], (key, fig[key])
    assert not bad, bad
    return fig


@pytest.mark.parametrize("scene_name,cfg_name", WX.CASES, ids=WX.IDS)
def test_forms_against_fp64(scene_name, cfg_name):
    sc, cfg, ref, src, gout, want = WX.reference(scene_name, cfg_name)
    check_case("%s-%s" % (scene_name, cfg_name), sc, cfg, ref, src, gout, want)


@pytest.mark.parametrize("scene_name,cfg_name", [("shift", "c8g4d4"), ("shift", "c64g8d8"), ("minify", "c8g4d4"), ("minify", "c32g8d8")])
def test_heavy_tail(scene_name, cfg_name):
    """one reference and one source value of 64 among unit-variance features: max |feature|^3 inflates make_fix_scale's bound, and
    with it the absolute resolution of every counter.  The derived bound must still hold; the achieved error is noted beside
    the unit-variance one."""
    sc, cfg, ref, src, gout, want = WX.reference(scene_name, cfg_name, True)
    assert ref.abs().max() == 64.0 and src.abs().max() == 64.0
    check_case("tail-%s-%s" % (scene_name, cfg_name), sc, cfg, ref, src, gout, want)


@pytest.mark.parametrize("cfg_name", ["c8g4d4", "c64g8d8", "c16g4d3nf"])
def test_gradients_follow_grad_out(cfg_name):
    """grad_out * 2^k moves the frexp-based scale by exactly k: the gradients are 2^k times the unscaled ones bit for bit
    (g_src of the atomic form aside: fp32 atomics in arrival order).  All-zero grad_out gives all-zero gradients.  On ``shift``,
    whose taps all fall inside their windows."""
    sc, cfg, ref, src, gout, want = WX.reference("shift", cfg_name)
    run = Run(sc, cfg, ref, src, gout)
    for form in FORMS:
        g_ref, g_src = run.backward(form)
        assert g_ref.isfinite().all() and g_src.isfinite().all()
        for k in (-40, 40):
            s_ref, s_src = run.backward(form, gout=run.gout * 2.0 ** k)
            assert torch.equal(s_ref, g_ref * 2.0 ** k), (form, k)
            if form != "atomic":
                assert torch.equal(s_src, g_src * 2.0 ** k), (form, k)
            else:
                assert ((s_src * 2.0 ** -k - g_src).abs().max() <= 1e-5 * g_src.abs().max()), k
        z_ref, z_src = run.backward(form, gout=torch.zeros_like(run.gout))
        assert (z_ref == 0).all() and (z_src == 0).all(), form


@pytest.mark.parametrize("cfg_name", ["c8g4d4", "c16g4d3nf", "c64g8d8"])
@pytest.mark.parametrize("what", ["grad_out", "ref", "src"])
def test_non_finite_operands_give_nan_everywhere(what, cfg_name):
    """make_fix_scale's promise: with a non-finite operand the gradients are NaN, never silently finite -- one NaN in grad_out,
    one in ref, or one +Inf in a source texel no sample touches: every element of g_ref and of g_src is NaN, in every form (the
    window forms: also the texels no window reaches)."""
    sc, cfg, ref, src, gout, want = WX.reference("shift", cfg_name)
    ref, src, gout = ref.clone(), src.clone(), gout.clone()
    if what == "grad_out":
        gout[1, 0, 4, 11, 0] = NAN
    elif what == "ref":
        ref[0, 3, 7, cfg.C - 1] = NAN
    else:
        free = (WX.contributions(sc)[1, 0] == 0).nonzero()
        assert len(free)
        src[1, 0, int(free[0][0]), int(free[0][1]), 2] = float("inf")
    run = Run(sc, cfg, ref, src, gout)
    for form in FORMS:
        g_ref, g_src = run.backward(form)
        assert g_ref.isnan().all(), (form, int((~g_ref.isnan()).sum()))
        assert g_src.isnan().all(), (form, int((~g_src.isnan()).sum()), int((g_src == 0).sum()))


@pytest.mark.parametrize("cfg_name", ["c16g4d4", "c8g4d4"])
def test_strided_operands(cfg_name):
    """The C entries with padded batches and views (batch stride > h * w * C, view stride > B * Hs * Ws * C, NaN in the padding):
    the operand maxima are then reduced piece by piece and the counting pass runs on its own.  Sorted and gather: the
    contiguous call's bits; atomic: the bound of test_forms_against_fp64; the padding stays NaN."""
    sc, cfg, ref, src, gout, want = WX.reference("tile_corner", cfg_name)
    run = Run(sc, cfg, ref, src, gout)
    B, NV, h, w, Hs, Ws, C, D = sc.B, sc.NV, sc.h, sc.w, sc.Hs, sc.Ws, cfg.C, cfg.D
    n_ref, n_src = h * w * C, Hs * Ws * C
    ref_bs, src_bs = n_ref + 64, n_src + 192
    src_vs = B * src_bs + 128

    def padded(fill):
        pr = torch.full((B, ref_bs), NAN, device=DEV)
        ps = torch.full((NV, src_vs), NAN, device=DEV)
        vr = pr[:, :n_ref]
        vs = ps[:, :B * src_bs].view(NV, B, src_bs)[:, :, :n_src]
        if fill is not None:
            vr.fill_(fill[0])
            vs.fill_(fill[1])
        return pr, ps, vr, vs

    def padding_is_nan(pr, ps):
        return bool(pr[:, n_ref:].isnan().all() and ps[:, B * src_bs:].isnan().all()
                    and ps[:, :B * src_bs].view(NV, B, src_bs)[:, :, n_src:].isnan().all())

    pr, ps, vr, vs = padded(None)
    vr.copy_(run.ref.view(B, n_ref))
    vs.copy_(run.src.view(NV, B, n_src))
    lib = _lib.load()
    base = WX.gradients(ref, src, sc.rt, sc.hypo, gout, cfg, torch.float32, device=DEV)
    tol, n_src_count, bound = tolerances(sc, cfg, ref, src, gout, want, base)
    for form in FORMS:
        c_ref, c_src = run.backward(form)
        gr, gs, g_ref, g_src = padded((NAN, NAN if form == "sorted" else 0.0))
        tail = (B, NV, C, run.G, D, h, w, Hs, Ws, ref_bs, src_vs, src_bs, int(cfg.group), int(cfg.fuse), WX.ATTN_TEMP, ops._stream())
        head = (pr.data_ptr(), ps.data_ptr(), run.rt.data_ptr(), run.hypo.data_ptr(), run.out.data_ptr(), run.wsum.data_ptr(),
                run.gout.data_ptr(), gr.data_ptr(), gs.data_ptr())
        if form == "sorted":
            nf, ni = ops.warp_agg_bwd_sorted_scratch(B, NV, C, D, h, w, Hs, Ws)
            rec = torch.empty(nf, device=DEV)
            ints = torch.empty(ni, device=DEV, dtype=torch.int32)
            _lib.check(lib.mvster_warp_agg_bwd_sorted(*head, rec.data_ptr(), ints.data_ptr(), *tail), "warp_agg_bwd_sorted")
        else:
            nf, ni = ctypes.c_long(0), ctypes.c_long(0)
            _lib.check(lib.mvster_warp_agg_bwd_scratch(B, NV, C, run.G, D, h, w, int(cfg.fuse), ctypes.addressof(nf),
                                                       ctypes.addressof(ni)), "warp_agg_bwd_scratch")
            win = torch.empty(nf.value, device=DEV) if form == "gather" else None
            org = torch.empty(ni.value, device=DEV, dtype=torch.int32)
            _lib.check(lib.mvster_warp_agg_bwd(*head, None if win is None else win.data_ptr(), org.data_ptr(), *tail), "warp_agg_bwd")
        assert _lib.last_kernel() == WX.first_pass_kernel(cfg, form)
        torch.cuda.synchronize()
        assert padding_is_nan(gr, gs) and padding_is_nan(pr, ps), form
        s_ref, s_src = g_ref.reshape(c_ref.shape), g_src.reshape(c_src.shape)
        assert torch.equal(s_ref, c_ref), form
        if form != "atomic":
            assert torch.equal(s_src, c_src), form
        else:
            e32, first, second, scale = tol["src"]
            assert bool(((s_src.cpu().double() - want[3]).abs() <= first + second[form]).all())
