"""The validation pass on the GPU: the masked depth-error reduction against its numpy restatement (tests/validate_cases.py),
the device form of DictAverageMeter, and ``validation_scalars`` / ``Validator`` against the separate calls they stand for
-- bit for bit, with no host synchronisation per batch, and across weights that move between two validation epochs."""
import math

import numpy as np
import pytest
import torch

from tests import validate_cases as VC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import (SCALAR_NAMES, AbsDepthError_metrics, MVS4net, MVS4net_loss, Thres_metrics, Validator, depth_metrics,
                            ops, validation_scalars)
    from mvster_amd.synthetic import make_inputs, randomize_state
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_against_restatement(est, gt, mask, scale):
    out, raw = ops.depth_metrics(_dev(est), _dev(gt), _dev(mask), VC.THRESHOLDS, None if scale is None else _dev(scale))
    out2, raw2 = ops.depth_metrics(_dev(est), _dev(gt), _dev(mask), VC.THRESHOLDS, None if scale is None else _dev(scale))
    out, raw, out2, raw2 = out.cpu().numpy(), raw.cpu().numpy(), out2.cpu().numpy(), raw2.cpu().numpy()
    assert out.dtype == np.float32 and raw.dtype == np.float64
    assert out.tobytes() == out2.tobytes() and raw.tobytes() == raw2.tobytes()          # two runs: identical bits
    want = VC.raw_ref(est, gt, mask, VC.THRESHOLDS, scale)
    N = est.shape[0]
    for n in range(N):
        assert raw[n, 0] == want[n, 0] and raw[n, 2:].tolist() == want[n, 2:].tolist(), (n, raw[n], want[n])     # counts: exactly
        a, b = float(raw[n, 1]), float(want[n, 1])
        print("image %d: valid %d, sum %r (numpy %r)" % (n, want[n, 0], a, b))
        if math.isnan(b) or math.isinf(b):
            assert VC.same_float(a, b), (n, a, b)
        else:
            # any summation order of n non-negative doubles is within n * 2^-53 (relative) of any other
            assert abs(a - b) <= want[n, 0] * 2.0 ** -53 * b, (n, a, b)
    # the derived values from the kernel's own sums: per image float32(float64(x) / float64(n)), then the fp32 in-order mean
    # (N = 1: the per-image value itself)
    derived = VC.out_from_raw(raw)
    assert all(VC.same_float(float(x), float(y)) for x, y in zip(out, derived)), (out, derived)
    # the per-image values on their own: the same image as a batch of one (same sums: a workgroup never mixes two images)
    for n in range(N if N > 1 else 0):
        o1, r1 = ops.depth_metrics(_dev(est[n:n + 1]), _dev(gt[n:n + 1]), _dev(mask[n:n + 1]), VC.THRESHOLDS,
                                   None if scale is None else _dev(scale[n:n + 1]))
        o1, r1 = o1.cpu().numpy(), r1.cpu().numpy()
        assert all(VC.same_float(float(x), float(y)) for x, y in zip(r1[0], raw[n])), (n, r1, raw[n])
        with np.errstate(invalid="ignore", divide="ignore"):
            per_image = [np.float32(np.float64(raw[n, 1 + j]) / np.float64(raw[n, 0])) for j in range(raw.shape[1] - 1)]
        assert all(VC.same_float(float(x), float(y)) for x, y in zip(o1, per_image)), (n, o1, per_image)
    # the threshold ratios rest on counts alone: equal to the restatement's without a detour over the kernel's sums
    ref_out = VC.out_from_raw(want)
    assert all(VC.same_float(float(x), float(y)) for x, y in zip(out[1:], ref_out[1:])), (out, ref_out)
    return out, raw


@pytest.mark.parametrize("name,shape,mask_kind,special", list(VC.cases()), ids=[c[0] for c in VC.cases()])
def test_depth_metrics_against_the_numpy_restatement(name, shape, mask_kind, special):
    est, gt, mask, scale = VC.make_case(shape, mask_kind, special)
    out, raw = _check_against_restatement(est, gt, mask, None)
    if mask_kind == "one_empty":
        assert raw[-1, 0] == 0 and np.isnan(out).all()          # an image without a valid pixel: NaN, not special-cased
    _check_against_restatement(est, gt, mask, scale)


def test_depth_metrics_do_not_depend_on_the_alignment_of_the_planes():
    """Planes that start 4 bytes off a 16-byte boundary take the scalar loads; the pixels a lane sums are the same, so the
    bits are."""
    est, gt, mask, _ = VC.make_case((2, 64, 80), "80", "invalid_only")
    a = ops.depth_metrics(_dev(est), _dev(gt), _dev(mask))

    def off(x):
        buf = torch.empty(x.size + 1, device=DEV)
        buf[1:].copy_(_dev(x).reshape(-1))
        v = buf[1:].view(x.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    b = ops.depth_metrics(off(est), off(gt), off(mask))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_depth_metrics_wrapper_checks():
    x = torch.zeros(2, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.depth_metrics(x, x, x, thresholds=())
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.depth_metrics(x, x, x, thresholds=tuple(range(9)))
    with pytest.raises(RuntimeError, match="one shape"):
        ops.depth_metrics(x, x[:1], x)
    with pytest.raises(RuntimeError, match="fp32-only"):
        ops.depth_metrics(x, x, x > 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.depth_metrics(x.transpose(1, 2), x, x)
    with pytest.raises(RuntimeError, match="one value per image"):
        ops.depth_metrics(x, x, x, scale=torch.ones(3, device=DEV))
    with pytest.raises(RuntimeError, match="float64"):
        ops.scalar_accumulate(torch.zeros(17, device=DEV), torch.zeros(17, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="row must be"):
        ops.scalar_accumulate(torch.zeros(16, device=DEV), torch.zeros(17, dtype=torch.float64, device=DEV),
                              torch.zeros(1, dtype=torch.int64, device=DEV))


def test_scalar_accumulate_is_the_python_float_running_sum():
    g = torch.Generator().manual_seed(5)
    rows = [torch.randn(17, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(7)]
    rows[3][11] = float("nan")
    sums = torch.full((17,), 3.0, dtype=torch.float64, device=DEV)
    count = torch.full((1,), 9, dtype=torch.int64, device=DEV)
    ops.scalar_reset(sums, count)
    assert sums.tolist() == [0.0] * 17 and count.item() == 0
    running = [0.0] * 17
    for i, r in enumerate(rows):
        ops.scalar_accumulate(r.to(DEV), sums, count)
        running = [a + float(b) for a, b in zip(running, r.tolist())]
        got = sums.tolist()
        assert all(VC.same_float(x, y) for x, y in zip(got, running)), (i, got, running)
        assert count.item() == i + 1
    assert math.isnan(running[11]) and sum(math.isnan(v) for v in running) == 1
    ops.scalar_reset(sums, count)
    assert sums.tolist() == [0.0] * 17 and count.item() == 0


# ---- the model-level pieces at 64 x 64, 3 views, batch 2 ------------------------------------------------------------------
CFG = dict(arch_mode="fpn", reg_net="reg2d", num_stage=4, fpn_base_channel=8, reg_channel=8, stage_splits=[8, 8, 4, 4],
           depth_interals_ratio=[0.5, 0.5, 0.5, 1], group_cor=True, group_cor_dim=[8, 8, 4, 4], inverse_depth=True, mono=True,
           attn_temp=2, attn_fuse_d=True)
LOSS_KW = dict(stage_lw=[1, 1, 1, 1], l1ot_lw=[0, 1], inverse_depth=True, ot_iter=10, ot_eps=1, ot_continous=False)
H = W = 64
VIEWS, B = 3, 2


def _batch(seed):
    imgs, proj, dv = make_inputs(nviews=VIEWS, H=H, W=W, seed=seed, batch=B)
    g = torch.Generator().manual_seed(seed)
    gt, mask = {}, {}
    for s in range(1, 5):
        hs, ws = H // 2 ** (4 - s), W // 2 ** (4 - s)
        gt["stage%d" % s] = (500 + 300 * torch.rand(B, hs, ws, generator=g)).to(DEV)
        mask["stage%d" % s] = (torch.rand(B, hs, ws, generator=g) > 0.2).float().to(DEV)
    return [i.to(DEV) for i in imgs], {k: v.to(DEV) for k, v in proj.items()}, dv.to(DEV), gt, mask


def _build(state=None, seed_sd=6):
    torch.manual_seed(4)
    m = MVS4net(**CFG)
    m.load_state_dict(randomize_state(m.state_dict(), seed=seed_sd, prob_gain=4.0) if state is None else state)
    return m.to(DEV).eval()


def _eager_row(model, batch):
    imgs, proj, dv, gt, mask = batch
    with torch.no_grad():
        return validation_scalars(model.forward_eager(imgs, proj, dv), gt, mask, **LOSS_KW).clone()


@pytest.fixture(scope="module")
def setup():
    """One model, three batches and their eager rows (computed once, left unchanged)."""
    model = _build()
    batches = [_batch(seed) for seed in (3, 4, 5)]
    rows = [_eager_row(model, b) for b in batches]
    return model, batches, rows


def _same_bits(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_validation_scalars_are_the_separate_calls(setup):
    model, batches, rows = setup
    imgs, proj, dv, gt, mask = batches[0]
    row = rows[0]
    assert tuple(row.shape) == (17,) and row.dtype == torch.float32 and row.is_cuda
    with torch.no_grad():
        outputs = model(imgs, proj, dv)
        loss, d_loss, c_loss, range_err = MVS4net_loss(outputs, gt, mask, mono=False, **LOSS_KW)
        want = torch.stack([loss] + list(d_loss) + list(c_loss) + list(range_err))
        metrics, _ = ops.depth_metrics(outputs["depth"], gt["stage4"], mask["stage4"])
    print("row", row.tolist())
    assert _same_bits(row[:13], want)
    assert _same_bits(row[13:], metrics)
    assert bool(torch.isfinite(row).all()) and float(row[13]) > 0 and 0 < float(row[14]) <= 1
    # the reference's names on the same numbers
    named = depth_metrics(outputs["depth"], gt["stage4"], mask["stage4"] > 0.5)
    assert list(named.keys()) == list(SCALAR_NAMES[13:])
    for i, k in enumerate(SCALAR_NAMES[13:]):
        assert named[k].dim() == 0 and named[k].is_cuda and _same_bits(named[k], row[13 + i])
    assert _same_bits(AbsDepthError_metrics(outputs["depth"], gt["stage4"], mask["stage4"] > 0.5), row[13])
    for i, t in enumerate((2, 4, 8)):
        assert _same_bits(Thres_metrics(outputs["depth"], gt["stage4"], mask["stage4"] > 0.5, t), row[14 + i])
    assert _same_bits(Thres_metrics(outputs["depth"], gt["stage4"], mask["stage4"], 4.0), row[15])          # a float mask


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
def test_validator_rows_and_mean(setup, capture):
    model, batches, rows = setup
    v = Validator(model, *batches[0], capture=capture, **LOSS_KW)
    assert (v.graph is not None) == capture
    got = [v().clone()] + [v(*b).clone() for b in batches[1:]]
    for i, (g, w) in enumerate(zip(got, rows)):
        assert _same_bits(g, w), (i, g.tolist(), w.tolist())
    mean = v.mean()
    want = VC.meter_mean([r.tolist() for r in rows])
    assert list(mean.keys()) == list(SCALAR_NAMES)
    for k, w in zip(SCALAR_NAMES, want):
        assert isinstance(mean[k], float) and VC.same_float(mean[k], w), (k, mean[k], w)
    assert v.count.item() == 3
    # image_outputs of the last batch, as the reference forms them
    imgs = v.last_images()
    depth, gt4, m4 = v.outputs["depth"], batches[2][3]["stage4"], batches[2][4]["stage4"]
    assert torch.equal(imgs["depth_est"], depth * m4) and torch.equal(imgs["depth_est_nomask"], depth)
    assert torch.equal(imgs["errormap"], (depth - gt4).abs() * m4) and imgs["depth_est_nomask"].data_ptr() != depth.data_ptr()
    # a new epoch
    v.reset()
    v(*batches[1])
    again = v.mean()
    assert all(VC.same_float(again[k], float(x)) for k, x in zip(SCALAR_NAMES, rows[1].tolist()))
    with pytest.raises(RuntimeError, match="static buffer"):
        v(depth_values=batches[0][2][:1])


def test_validate_loop(setup):
    from mvster_amd.validate import validate
    model, batches, rows = setup
    mean = validate(model, iter(batches), **LOSS_KW)
    want = VC.meter_mean([r.tolist() for r in rows])
    assert all(VC.same_float(mean[k], w) for k, w in zip(SCALAR_NAMES, want))
    with pytest.raises(ValueError):
        validate(model, [], **LOSS_KW)


def test_a_warmed_validator_does_not_synchronise(setup):
    model, batches, rows = setup
    v = Validator(model, *batches[0], **LOSS_KW)
    v()
    torch.cuda.synchronize()
    v.reset()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            v(*b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    mean = v.mean()
    want = VC.meter_mean([r.tolist() for r in rows])
    assert all(VC.same_float(mean[k], w) for k, w in zip(SCALAR_NAMES, want))


def _train_loss(out, gt, mask):
    return MVS4net_loss(out, gt, mask, mono=True, **LOSS_KW)


@pytest.mark.parametrize("how", ["eager_adam", "graphed_fused_adam"])
def test_validator_follows_weights_that_moved(how):
    """Between two validation epochs the weights move: by an eager optimizer step, or by replays of a captured training step
    (which touch no version counter).  The next call re-captures and equals a freshly built model that loads the current
    state; the running sums survive the re-capture."""
    model = _build(seed_sd=8)
    batch = _batch(7)
    imgs, proj, dv, gt, mask = batch
    v = Validator(model, *batch, **LOSS_KW)
    first = v().clone()
    stamp = v.stamp
    model.train()
    if how == "eager_adam":
        opt = torch.optim.Adam(model.parameters(), lr=5e-3)
        opt.zero_grad()
        _train_loss(model(imgs, proj, dv), gt, mask)[0].backward()
        opt.step()
    else:
        from mvster_amd.graph import GraphedTrainStep
        from mvster_amd.optim import FusedAdam
        opt = FusedAdam(model.parameters(), lr=5e-3)
        step = GraphedTrainStep(model, opt, _train_loss, imgs, proj, dv, gt, mask, warmup=1)
        stamp = model._state_stamp()                   # (the warm-up steps already moved the weights: the replays must too)
        step()
        step()
    torch.cuda.synchronize()
    model.eval()
    assert model._state_stamp() != stamp
    second = v().clone()
    fresh = _build(state=model.state_dict())
    want = _eager_row(fresh, batch)
    assert _same_bits(second, want), (second.tolist(), want.tolist())
    assert not _same_bits(second, first)
    assert v.stamp == model._state_stamp() and v.count.item() == 2
    mean = v.mean()
    both = VC.meter_mean([first.tolist(), second.tolist()])
    assert all(VC.same_float(mean[k], w) for k, w in zip(SCALAR_NAMES, both))
    third = v().clone()                                # no further change: a plain replay of the new graph
    assert _same_bits(third, want)


def test_validator_refuses_a_model_in_training_mode(setup):
    model, batches, rows = setup
    v = Validator(model, *batches[0], capture=False, **LOSS_KW)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            Validator(model, *batches[0], **LOSS_KW)
        with pytest.raises(RuntimeError, match="eval"):
            v()
    finally:
        model.eval()
