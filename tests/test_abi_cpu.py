"""The C-ABI library builds, loads and exports every symbol include/mvster_hip.h declares
(no compute calls: there is no GPU in this container), and the product refuses CPU tensors."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mvster_hip.h")).read()
    return sorted(set(re.findall(r"\b(?:int|const char\*)\s+(mvster_\w+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    from mvster_amd import _lib
    names = declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), n
    # and the Python binding table covers exactly the header
    assert sorted(_lib.SIGNATURES.keys()) == names


def test_retired_batch_norm_forms_are_gone(lib):
    """Training-mode BatchNorm has one path (mvster_bn_train_fwd / _bwd).  The last-arriver statistics kernel and the
    grid-barrier small-tensor form are neither bound, exported nor declared, and ops has
    no switch or wrapper for them."""
    from mvster_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "mvster_hip.h")).read()
    for name in ("mvster_bn_stats", "mvster_bn_fused_ok", "mvster_bn_fwd_fused", "mvster_bn_bwd_fused"):
        assert name not in _lib.SIGNATURES and not hasattr(lib, name) and name not in header, name
    for name in ("BN_FUSED", "BN_TAILLESS", "bn_fused_ok", "bn_fwd_fused", "bn_bwd_fused", "bn_batch_stats"):
        assert not hasattr(ops, name), name


def test_last_kernel_accessor(lib):
    from mvster_amd import _lib
    assert _lib.last_kernel() == ""            # nothing launched in this process (no GPU here)


def test_null_and_shape_errors_are_reported_without_a_gpu(lib):
    # argument validation happens before any HIP call
    assert lib.mvster_relative_projection(None, None, 1, 2, None) == -1
    assert lib.mvster_init_range(None, 2, None, 1, 8, 4, 4, 1, None) == -1
    assert lib.mvster_upsample_bilinear(None, None, 1, 4, 4, 8, 8, None) == -1
    assert lib.mvster_select_depth(None, None, None, None, 0, None, None, None, None, None, None, None, 1, 4, 4, 4, 0.5,
                                   None) == -1


def test_fused_adam_checks_every_tensor_before_the_first_launch(lib):
    """mvster_fused_adam over 200 tensors (two launches of <= 128) with a null grads[150] returns MVSTER_ERR_NULL; the
    pointers are checked before anything is launched, so nothing of the first 128 tensors is updated (the GPU side of
    this: tests/test_gpu_train.py::test_fused_adam_null_gradient_changes_nothing).  Negative sizes or offsets are
    MVSTER_ERR_SHAPE.  Without a GPU the device pointers are stand-in addresses that nothing may dereference."""
    import ctypes
    from mvster_amd import _lib
    n = 200
    if torch.cuda.is_available():
        keep = torch.zeros(3 * n * 64 + 3, device="cuda")
        base, stride = keep.data_ptr(), 64 * 4
    else:
        base, stride = 1 << 32, 64 * 4
    dev = [base + stride * i for i in range(3 * n)]
    pp = (ctypes.c_void_p * n)(*dev[:n])
    gp = (ctypes.c_void_p * n)(*dev[n:2 * n])
    sizes = (ctypes.c_int * n)(*[64] * n)
    offs = (ctypes.c_int * n)(*[64 * i for i in range(n)])
    cells = base + stride * 3 * n

    def call(count=n):
        return lib.mvster_fused_adam(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(gp, ctypes.c_void_p),
                                     ctypes.cast(sizes, ctypes.c_void_p), ctypes.cast(offs, ctypes.c_void_p), count,
                                     dev[2 * n], dev[2 * n], cells, cells + 8, 0.9, 0.999, 1e-8, 0.0, None)
    gp[150] = None
    assert call() == _lib.ERR_NULL
    gp[150] = dev[n + 150]
    pp[199] = None
    assert call() == _lib.ERR_NULL
    pp[199] = dev[199]
    sizes[170] = -1
    assert call() == _lib.ERR_SHAPE
    sizes[170] = 64
    offs[130] = -64
    assert call() == _lib.ERR_SHAPE
    assert call(0) == _lib.ERR_SHAPE


def test_product_has_no_cpu_fallback(shipped_cfg):
    from mvster_amd import MVS4net, ops
    from mvster_amd.synthetic import make_inputs
    m = MVS4net(**shipped_cfg).eval()
    imgs, proj, dv = make_inputs(nviews=3, H=64, W=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(imgs, proj, dv)
    with pytest.raises(RuntimeError):
        ops.init_range(dv, 8, 8, 8, inverse=True)


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "mvster_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "oracle" not in re.sub(r'""".*?"""', "", open(os.path.join(pkg, fn)).read(), flags=re.S) \
                .replace("CPU oracle lives in oracle/", ""), fn


def test_models_shim_exports_reference_surface():
    import models
    for n in ("MVS4net", "MVS4net_loss", "Blend_loss"):
        assert hasattr(models, n)


def test_state_dict_layout(shipped_cfg, checkpoint):
    from mvster_amd import MVS4net
    m = MVS4net(**shipped_cfg)
    assert sorted(m.state_dict().keys()) == sorted(checkpoint.keys())
    m.load_state_dict(checkpoint, strict=True)
    counts = {}
    for k in checkpoint:
        counts[k.split(".")[0]] = counts.get(k.split(".")[0], 0) + 1
    assert counts == {"feature": 76, "reg": 248, "mono_depth_decoder": 24}


def test_unsupported_switches_fail_loudly():
    from mvster_amd import MVS4net
    with pytest.raises(NotImplementedError):
        MVS4net(dcn=True)
    with pytest.raises(NotImplementedError):
        MVS4net(asff=True)


def test_hypothesis_counts_accepted_and_rejected():
    """stage_splits: the reference takes any --ndepths (mvs4net_utils.py:61-99); here evaluation takes 2..64 per stage (3..64
    with inverse depth: the bounds read hypotheses 1 and 2, :1083), a squared-difference volume at most 8 on the stages with
    32 or more channels, and training at most 16 -- everything else is refused at construction / at the training forward."""
    from mvster_amd import MVS4net
    from mvster_amd.synthetic import make_inputs
    MVS4net(stage_splits=[48, 32, 8, 4], group_cor=True, inverse_depth=True)
    MVS4net(stage_splits=[64, 17, 2, 3], group_cor=True)
    MVS4net(stage_splits=[8, 8, 64, 4])
    for kw in (dict(stage_splits=[65, 8, 4, 4], group_cor=True), dict(stage_splits=[8, 8, 2, 4], group_cor=True, inverse_depth=True),
               dict(stage_splits=[8, 1, 4, 4], group_cor=True), dict(stage_splits=[16, 8, 4, 4]), dict(stage_splits=[8, 9, 4, 4])):
        with pytest.raises(NotImplementedError, match="stage_splits"):
            MVS4net(**kw)
    m = MVS4net(stage_splits=[32, 8, 4, 4], group_cor=True).train()
    imgs, proj, dv = make_inputs(nviews=3, H=64, W=64)
    with pytest.raises(NotImplementedError, match="training"):
        m(imgs, proj, dv)


def test_boundary_rejects_malformed_inputs(shipped_cfg):
    """MVS4net.forward validates what it hands to the kernels as raw pointers: view count, per-stage projection stacks,
    the depth range (shape errors come before the device check, so this runs without a GPU)."""
    from mvster_amd import MVS4net
    from mvster_amd.synthetic import make_inputs
    m = MVS4net(**shipped_cfg).eval()
    imgs, proj, dv = make_inputs(nviews=3, H=64, W=64)
    with pytest.raises(RuntimeError, match="stage3"):
        m(imgs, {k: v for k, v in proj.items() if k != "stage3"}, dv)
    with pytest.raises(RuntimeError, match=r"proj_matrices\['stage2'\]"):
        m(imgs, dict(proj, stage2=proj["stage2"][:, :2]), dv)                 # one view short
    with pytest.raises(RuntimeError, match="views = len"):
        m(imgs[:2], proj, dv)                                                  # list and stacks disagree
    with pytest.raises(RuntimeError, match="depth_values"):
        m(imgs, proj, dv[:, :1])
    with pytest.raises(RuntimeError, match="depth_values"):
        m(imgs, proj, dv.reshape(-1))
    with pytest.raises(RuntimeError, match=r"imgs\[1\]"):
        m([imgs[0], imgs[1][:, :, :32], imgs[2]], proj, dv)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        m([i[:, :, :48] for i in imgs], proj, dv)


def test_model_copies_and_pickles_without_its_caches(shipped_cfg):
    """``copy.deepcopy(model)`` (EMA helpers) and whole-module pickling leave the per-process caches behind (packed-weight plans,
    side streams, captured hipGraphs of the forward cache): the copy has the same parameters and empty caches of its own."""
    import copy
    import io

    import torch
    from mvster_amd import MVS4net
    m = MVS4net(**shipped_cfg).eval()
    m._fwd_cache.entries["some key"] = [1, object()]          # (stands for a captured graph: must not travel)
    m._plans["cuda:0"] = ("plans",)
    c = copy.deepcopy(m)
    assert len(c._fwd_cache.entries) == 0 and c._plans == {} and c._fwd_cache is not m._fwd_cache
    assert len(m._fwd_cache.entries) == 1                       # the original keeps its own
    for (ka, va), (kb, vb) in zip(m.state_dict().items(), c.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    m._fwd_cache.entries.clear()
    m._plans.clear()
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    r = torch.load(buf, weights_only=False)
    assert isinstance(r, MVS4net) and len(r._fwd_cache.entries) == 0 and r.graph_cache is True
