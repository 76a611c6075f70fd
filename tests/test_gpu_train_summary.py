"""The training half of an epoch on the GPU: Blend_loss's pooled error figures against their numpy restatement
(tests/train_summary_cases.py), and ``GraphedTrainStep(summary=True)`` -- the step's 17 (20) scalars, their running sums
and the retained depth map -- against the separate calls they stand for, bit for bit and without a host synchronisation."""
import numpy as np
import pytest
import torch

from tests import train_summary_cases as TC
from tests import validate_cases as VC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mvster_amd import SCALAR_NAMES, Blend_loss, MVS4net, MVS4net_loss, ops
    from mvster_amd.graph import GraphedTrainStep, graph_kernel_nodes
    from mvster_amd.optim import FusedAdam
    from mvster_amd.synthetic import make_inputs, randomize_state
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def _check_against_restatement(est, gt, mask, scale):
    """raw and out bit-equal to the restatement, NaN matching NaN.  The error SUM too: in these cases every fp32 error is a
    multiple of 2^-18 below 2^10 (integer ground truth of 400..900, scales of 0.14..1, products of at least 32) and an image
    has fewer than 2^15 pixels, so every partial sum has at most 43 significant bits: exact in fp64 in any order; a NaN or
    +inf error gives NaN or +inf in any order."""
    out, raw = ops.pooled_metrics(_dev(est), _dev(gt), _dev(mask), TC.THRESHOLDS, _dev(scale))
    out, raw = out.cpu().numpy(), raw.cpu().numpy()
    want_out, want_raw = TC.pooled_ref(est, gt, mask, TC.THRESHOLDS, scale)
    print("out", out.tolist(), "restatement", want_out.tolist())
    print("raw", raw.tolist(), "restatement", want_raw.tolist())
    assert out.dtype == np.float32 and raw.dtype == np.float64 and out.shape == (3,) and raw.shape == (est.shape[0], 4)
    assert TC.same_f64(raw, want_raw)
    assert TC.same_f32(out, want_out)
    return out, raw


@pytest.mark.parametrize("name,shape,mask_kind,special", list(TC.cases()), ids=[c[0] for c in TC.cases()])
def test_pooled_metrics_against_the_numpy_restatement(name, shape, mask_kind, special):
    for scale_kind in ("none", "random", "pow2"):
        est, gt, mask, scale = TC.make_case(shape, mask_kind, special, scale_kind)
        out, raw = _check_against_restatement(est, gt, mask, scale)
        if mask_kind == "all_empty":
            assert raw[:, 0].sum() == 0 and np.isnan(out).all()          # 0 / 0, not special-cased
        elif mask_kind == "one_empty":
            assert raw[-1, 0] == 0 and (shape[0] == 1 or not np.isnan(out[1:]).any())      # pooled: an empty image adds nothing
        if scale_kind == "pow2" and mask_kind != "all_empty" and shape[1] * shape[2] >= 4 and raw[0, 0] > 0:
            # the errors planted exactly on 3 and 1 count as at-or-below
            n = 0
            e = VC.errors(est[n], gt[n], mask[n] > 0.5, scale[n])
            assert (e == 3.0).sum() >= 2 and (e == 1.0).sum() >= 2
            assert raw[n, 2] == np.count_nonzero(e <= 3.0) and raw[n, 3] == np.count_nonzero(e <= 1.0)
            assert raw[n, 2] > np.count_nonzero(e < 3.0) and raw[n, 3] > np.count_nonzero(e < 1.0)


def test_pooled_metrics_do_not_depend_on_the_alignment_of_the_planes():
    est, gt, mask, scale = TC.make_case((2, 64, 80), "80", "invalid_only", "random")
    a = ops.pooled_metrics(_dev(est), _dev(gt), _dev(mask), TC.THRESHOLDS, _dev(scale))

    def off(x):
        buf = torch.empty(x.size + 1, device=DEV)
        buf[1:].copy_(_dev(x).reshape(-1))
        v = buf[1:].view(x.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    b = ops.pooled_metrics(off(est), off(gt), off(mask), TC.THRESHOLDS, _dev(scale))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_wrapper_checks():
    x = torch.zeros(2, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.pooled_metrics(x, x, x, thresholds=())
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.pooled_metrics(x, x, x, thresholds=tuple(range(9)))
    with pytest.raises(RuntimeError, match="one shape"):
        ops.pooled_metrics(x, x[:1], x)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.pooled_metrics(x[0], x[0], x[0])
    with pytest.raises(RuntimeError, match="fp32-only"):
        ops.pooled_metrics(x, x, x > 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.pooled_metrics(x.transpose(1, 2), x, x)
    with pytest.raises(RuntimeError, match="one value per image"):
        ops.pooled_metrics(x, x, x, scale=torch.ones(3, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pooled_metrics(x, x.cpu(), x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pooled_metrics(x, x, x, scale=torch.ones(2))
    sums, count = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    one = torch.ones((), device=DEV)
    with pytest.raises(RuntimeError, match="row and sums"):
        ops.scalar_gather_accumulate([one, one], torch.zeros(3, device=DEV), sums, count)
    with pytest.raises(RuntimeError, match="scalar 1"):
        ops.scalar_gather_accumulate([one, torch.ones(2, device=DEV), one], torch.zeros(3, device=DEV), sums, count)
    with pytest.raises(RuntimeError, match="scalar 2"):
        ops.scalar_gather_accumulate([one, one, torch.ones(())], torch.zeros(3, device=DEV), sums, count)
    with pytest.raises(RuntimeError, match="1 to 32"):
        ops.scalar_gather_accumulate([one] * 33, torch.zeros(33, device=DEV), torch.zeros(33, dtype=torch.float64, device=DEV), count)
    assert sums.tolist() == [0.0] * 3 and count.item() == 0


def test_gather_accumulate_is_stack_and_accumulate():
    g = torch.Generator().manual_seed(11)
    rows = [torch.randn(20, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(5)]
    rows[2][7] = float("nan")
    sums, count = torch.empty(20, dtype=torch.float64, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    ops.scalar_reset(sums, count)
    row = torch.zeros(20, device=DEV)
    for i, r in enumerate(rows):
        d = r.to(DEV)
        # scalars of their own, elements of a larger tensor, and 0-dim views
        scalars = [d[j].clone() if j % 3 == 0 else d[j:j + 1] if j % 3 == 1 else d[j] for j in range(20)]
        ops.scalar_gather_accumulate(scalars, row, sums, count)
        assert TC.same_f32(row.cpu().numpy(), r.numpy())
        assert count.item() == i + 1
    want = VC.meter_mean([r.tolist() for r in rows])
    got = [v / 5 for v in sums.tolist()]
    assert all(VC.same_float(a, b) for a, b in zip(got, want))


# ---- the model-level pieces at 64 x 64, 3 views, batch 2 (the setup of tests/test_gpu_validate.py) -----------------------
CFG = dict(arch_mode="fpn", reg_net="reg2d", num_stage=4, fpn_base_channel=8, reg_channel=8, stage_splits=[8, 8, 4, 4],
           depth_interals_ratio=[0.5, 0.5, 0.5, 1], group_cor=True, group_cor_dim=[8, 8, 4, 4], inverse_depth=True, mono=True,
           attn_temp=2, attn_fuse_d=True)
LOSS_KW = dict(stage_lw=[1, 1, 1, 1], l1ot_lw=[0, 1], inverse_depth=True, ot_iter=10, ot_eps=1, ot_continous=False, mono=True)
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


def _build():
    torch.manual_seed(4)
    m = MVS4net(**CFG)
    m.load_state_dict(randomize_state(m.state_dict(), seed=6, prob_gain=4.0))
    return m.to(DEV).train()


def _loss_fn(out, gt, mask):
    return MVS4net_loss(out, gt, mask, **LOSS_KW)


_RANGE = []


def _depth_range():
    """depth_max, depth_min [B] on the device (made once: the loss function runs inside the capture)."""
    if not _RANGE:
        _RANGE.extend([torch.tensor([935.0, 1100.0], device=DEV), torch.tensor([425.0, 300.0], device=DEV)])
    return _RANGE


def _blend_fn(out, gt, mask):
    depth_max, depth_min = _depth_range()
    return Blend_loss(out, gt, mask, depth_max=depth_max, depth_min=depth_min, **LOSS_KW)


def _twin_row(batch, loss_fn=None):
    """The row's entries from separate eager calls on a freshly built model in training mode: the loss function's returns,
    the depth metrics of the training forward's own depth map; also that depth map."""
    imgs, proj, dv, gt, mask = batch
    model = _build()
    out = model(imgs, proj, dv)
    res = (loss_fn or _loss_fn)(out, gt, mask)
    with torch.no_grad():
        metrics, _ = ops.depth_metrics(out["depth"].detach().contiguous(), gt["stage4"], mask["stage4"])
        row = torch.stack([res[0].detach()] + [t.detach() for r in res[1:4] for t in r] + list(metrics.unbind(0))
                          + [t.detach() for t in res[4:]])
    return row.clone(), out["depth"].detach().clone()


@pytest.fixture(scope="module")
def setup():
    """Three batches and their rows from separate eager calls (computed once, left unchanged)."""
    batches = [_batch(seed) for seed in (3, 4, 5)]
    twins = [_twin_row(b) for b in batches]
    return batches, [t[0] for t in twins], [t[1] for t in twins]


def _same_bits(a, b):
    return a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _step(batch, loss_fn=None, **kw):
    model = _build()
    opt = FusedAdam(model.parameters(), lr=0.0)                  # a zero learning rate: the forward is the same at every step
    return GraphedTrainStep(model, opt, loss_fn or _loss_fn, *batch, warmup=2, **kw)


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
def test_summary_rows_and_mean(setup, capture):
    batches, rows, depths = setup
    step = _step(batches[0], summary=True, capture=capture)
    assert (step.graph is not None) == capture
    assert step.names == tuple(SCALAR_NAMES) and len(step.names) == 17
    assert step.row.dtype == torch.float32 and tuple(step.row.shape) == (17,) and step.sums.dtype == torch.float64
    assert step.count.item() == 0 and step.sums.tolist() == [0.0] * 17          # warm-up and capture left them at zero
    got = []
    for i, b in enumerate(batches):
        loss = step(*b) if i else step()
        assert _same_bits(step.row[0], loss)
        got.append(step.row.clone())
        assert step.count.item() == i + 1
        assert _same_bits(step.depth_est, depths[i])
    for i, (g, w) in enumerate(zip(got, rows)):
        print("step %d row" % i, g.tolist(), "separate calls", w.tolist())
        assert _same_bits(g[:13], w[:13]), (i, g.tolist(), w.tolist())         # the loss function's returns
        assert _same_bits(g[13:], w[13:]), (i, g.tolist(), w.tolist())         # ops.depth_metrics of outputs["depth"]
    assert bool(torch.isfinite(got[0]).all()) and float(got[0][13]) > 0
    mean = step.summary_mean()
    want = VC.meter_mean([r.tolist() for r in got])
    assert list(mean.keys()) == list(SCALAR_NAMES)
    for k, w in zip(SCALAR_NAMES, want):
        assert isinstance(mean[k], float) and VC.same_float(mean[k], w), (k, mean[k], w)
    # image_outputs of the last step
    images = step.last_images()
    depth, gt4, m4 = step.depth_est, batches[2][3]["stage4"], batches[2][4]["stage4"]
    assert sorted(images) == ["depth_est", "depth_est_nomask", "errormap"]
    assert torch.equal(images["depth_est"], depth * m4) and torch.equal(images["depth_est_nomask"], depth)
    assert torch.equal(images["errormap"], (depth - gt4).abs() * m4) and images["depth_est_nomask"].data_ptr() != depth.data_ptr()
    if capture:
        ptr = step.depth_est.data_ptr()
        step()
        assert step.depth_est.data_ptr() == ptr                                 # static: the next replay writes it in place
    # a new epoch
    step.summary_reset()
    assert step.count.item() == 0 and step.sums.tolist() == [0.0] * 17
    step(*batches[1])
    again = step.summary_mean()
    assert all(VC.same_float(again[k], float(x)) for k, x in zip(SCALAR_NAMES, rows[1].tolist()))


def test_a_warmed_summary_step_does_not_synchronise(setup):
    batches, rows, _ = setup
    step = _step(batches[0], summary=True)
    step()
    torch.cuda.synchronize()
    step.summary_reset()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            step.optimizer.param_groups[0]["lr"] = 0.0
            step.optimizer.sync_hyperparameters()
            step(*b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    mean = step.summary_mean()
    want = VC.meter_mean([r.tolist() for r in rows])
    assert all(VC.same_float(mean[k], w) for k, w in zip(SCALAR_NAMES, want))


def test_the_default_step_is_the_step_without_the_keyword(setup, monkeypatch):
    """``summary=False`` captures what the step captured before the keyword existed -- ``_step`` as it was, written out here
    -- kernel node for kernel node, and ``summary=True`` three more: the depth metrics' two, and the gather into the row
    and the sums."""
    from mvster_amd.train_ops import deferred_wgrad_finish
    batches, _, _ = setup
    kept = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: kept(keep_graph=True))

    class StepBefore(GraphedTrainStep):
        def _step(self):
            self.optimizer.zero_grad(set_to_none=True)
            batched = getattr(self, "_batch", None) is not None
            if batched:
                self._cache.run_batch(self._batch)
            try:
                out = self.model(self.imgs, self.proj, self.depth_values)
                res = self.loss_fn(out, self.gt, self.mask)
                loss = res[0] if isinstance(res, (tuple, list)) else res
                with deferred_wgrad_finish(streams=self.wgrad_streams, overlap=self.wgrad_overlap, policy=self.wgrad_policy,
                                           early=self.wgrad_early):
                    loss.backward()
            finally:
                if batched:
                    self._cache.end_batch()
            if self.grad_sync is not None:
                self.grad_sync.sync()
            self.optimizer.step()
            return loss.detach()

    def nodes(cls, **kw):
        model = _build()
        step = cls(model, FusedAdam(model.parameters(), lr=0.0), _loss_fn, *batches[0], warmup=2, **kw)
        counts = graph_kernel_nodes(step.graph)
        return step, counts
    plain, n_plain = nodes(GraphedTrainStep)
    assert plain.summary is False and not hasattr(plain, "row") and not hasattr(plain, "sums")
    with pytest.raises(RuntimeError, match="summary=True"):
        plain.last_images()
    before, n_before = nodes(StepBefore)
    with_summary, n_summary = nodes(GraphedTrainStep, summary=True)
    print("(kernel nodes, nodes) of the captured step: before %r, summary=False %r, summary=True %r" % (n_before, n_plain, n_summary))
    assert n_plain == n_before and n_plain[0] > 100
    assert n_summary == (n_plain[0] + 3, n_plain[1] + 3)
    assert _same_bits(plain(), before())                  # and the kept graphs replay


def test_blend_loss_captures(setup):
    """Blend_loss with [B] device depth_max / depth_min inside the captured step: 20 scalars, the last three
    ``ops.pooled_metrics`` of the step's own depth map; under the sync-debug mode."""
    batches, rows, depths = setup
    _depth_range()
    step = _step(batches[0], loss_fn=_blend_fn, summary=True)
    assert step.names == tuple(SCALAR_NAMES) + ("epe", "err3", "err1") and tuple(step.row.shape) == (20,)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = []
        for i, b in enumerate(batches):
            loss = step(*b) if i else step()
            got.append(step.row.clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert step.count.item() == 3 and _same_bits(got[2][0], loss)
    depth_max, depth_min = _depth_range()
    scale = 128 / (depth_max - depth_min)
    out, _ = ops.pooled_metrics(step.depth_est.contiguous(), batches[2][3]["stage4"], batches[2][4]["stage4"], (3, 1), scale)
    print("row", got[2].tolist(), "pooled", out.tolist())
    assert _same_bits(got[2][17:], out)
    assert bool(torch.isfinite(got[2]).all()) and 0 <= float(out[2]) <= float(out[1]) <= 100
    for g, w in zip(got, rows):
        assert _same_bits(g[:17], w)                              # the first 17: those of MVS4net_loss on the same forward
    # the figures themselves: the boolean-gather expression on the same depth map (fp32 means: rtol 1e-5)
    m = batches[2][4]["stage4"] > 0.5
    s = scale[:, None, None]
    err = torch.abs(step.depth_est * s - batches[2][3]["stage4"] * s)[m]
    want = torch.stack([err.mean(), (err <= 3).float().mean() * 100, (err <= 1).float().mean() * 100])
    assert torch.allclose(out, want, rtol=1e-5, atol=0)
    mean = step.summary_mean()
    assert list(mean.keys()) == list(step.names) and len(mean) == 20
    # and without the summary: the captured step over Blend_loss replays
    plain = _step(batches[0], loss_fn=_blend_fn)
    loss = plain()
    assert _same_bits(loss, rows[0][0]) and not hasattr(plain, "row")


def test_a_loss_function_of_another_form_is_refused(setup):
    batches, rows, _ = setup

    def bare(out, gt, mask):
        return _loss_fn(out, gt, mask)[0]
    with pytest.raises(TypeError, match=r"returned a tensor of shape \(\)"):
        _step(batches[0], loss_fn=bare, summary=True)
    with pytest.raises(TypeError, match=r"a tuple of 2"):
        _step(batches[0], loss_fn=lambda o, g, m: _loss_fn(o, g, m)[:2], summary=True, capture=False)
    step = _step(batches[0], loss_fn=bare)
    assert _same_bits(step(), rows[0][0])
