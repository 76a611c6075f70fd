"""The validation half of the reference's epoch (train_mvs4.py:140-192, ``test_sample_depth`` :252-307) without a host
synchronisation per batch.

The reference runs, per validation sample, the eval forward, the loss, four depth metrics formed with boolean-mask
gathers (``depth_est[mask]``: a device synchronisation each, utils.py:125-159), 17 ``.item()`` calls and six full-size
copies to the host.  Here the metrics are one fused reduction (``mvster_depth_metrics``), the 17 scalars of a batch are
one device row, the epoch's running sums (``DictAverageMeter``, utils.py:103-122) are kept on the device by
``mvster_scalar_accumulate``, and ``Validator`` captures forward + loss + metrics + accumulation in one hipGraph: a
batch is one replay, the epoch ends with one small read-back (``Validator.mean``).
"""
import torch

from . import ops
from .loss import MVS4net_loss

# the keys of test_sample_depth's scalar_outputs, in its order (train_mvs4.py:278-295)
SCALAR_NAMES = (("loss",) + tuple("s%d_d_loss" % s for s in range(4)) + tuple("s%d_c_loss" % s for s in range(4))
                + tuple("s%d_range_err_ratio" % s for s in range(4))
                + ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error"))
THRESHOLDS = (2, 4, 8)


def _planes(depth_est, depth_gt, mask):
    # (a bool mask becomes 0 / 1, which the kernel's `> 0.5` reads like the reference's `mask > 0.5` reads a float one)
    return (depth_est.to(torch.float32).contiguous(), depth_gt.to(torch.float32).contiguous(),
            mask.to(torch.float32).contiguous())


def depth_metrics(depth_est, depth_gt, mask, thresholds=THRESHOLDS):
    """``abs_depth_error`` and ``thres<t>mm_error`` for every ``t`` of ``thresholds`` (utils.py:139-159 under
    ``compute_metrics_for_each_image``: per image over its valid pixels, then the mean over the batch) as 0-dim device
    tensors.  depth_est, depth_gt, mask [B,H,W] on the GPU; ``mask`` bool or float (> 0.5 = valid).  Two launches, no
    synchronisation; an image without a valid pixel makes the batch's values NaN, like the reference."""
    out, _ = ops.depth_metrics(*_planes(depth_est, depth_gt, mask), thresholds=thresholds)
    res = {"abs_depth_error": out[0]}
    for i, t in enumerate(thresholds):
        res["thres%gmm_error" % t] = out[1 + i]
    return res


def Thres_metrics(depth_est, depth_gt, mask, thres):
    """utils.py:139-146 with its signature: the ratio of valid pixels whose error exceeds ``thres``."""
    assert isinstance(thres, (int, float))
    return ops.depth_metrics(*_planes(depth_est, depth_gt, mask), thresholds=(thres,))[0][1]


def AbsDepthError_metrics(depth_est, depth_gt, mask, thres=None):
    """utils.py:150-159 with its signature: the mean absolute error over the valid pixels.  The ``thres=(lo, hi)`` band
    is used by no shipped driver and is not implemented."""
    if thres is not None:
        raise NotImplementedError("AbsDepthError_metrics: the thres=(lo, hi) error band is not implemented")
    return ops.depth_metrics(*_planes(depth_est, depth_gt, mask), thresholds=THRESHOLDS[:1])[0][0]


def validation_scalars(outputs, depth_gt_ms, mask_ms, **loss_kwargs):
    """The 17 scalars of ``test_sample_depth`` (train_mvs4.py:271-295) for one batch as one [17] fp32 device row in the
    order of ``SCALAR_NAMES``: ``MVS4net_loss(outputs, ..., mono=False)`` -- as the reference's driver names its returns:
    ``s*_d_loss`` the second, ``s*_c_loss`` the third -- and the depth metrics of ``outputs["depth"]`` against the last
    stage's ground truth and mask.  No host synchronisation; capturable."""
    stages = [k for k in outputs.keys() if "stage" in k]
    if len(stages) != 4:
        raise NotImplementedError("validation_scalars: the reference's 17 scalars are those of a 4-stage model, got %d stages"
                                  % len(stages))
    with torch.no_grad():
        loss, d_loss, c_loss, range_err = MVS4net_loss(outputs, depth_gt_ms, mask_ms, **dict(loss_kwargs, mono=False))
        last = "stage%d" % len(stages)
        metrics, _ = ops.depth_metrics(*_planes(outputs["depth"], depth_gt_ms[last], mask_ms[last]), thresholds=THRESHOLDS)
        return torch.stack([loss] + list(d_loss) + list(c_loss) + list(range_err) + list(metrics.unbind(0)))


def reduce_scalar_sums(sums, count, group=None, names=SCALAR_NAMES):
    """The arithmetic of ``Validator.mean``: sums [n] fp64 and count [1] int64 (any device) -> {name: sums[i] / count} as
    Python floats -- ``DictAverageMeter.mean`` (utils.py:121-122); ``names``: the n keys (a captured training step over
    ``Blend_loss`` has 20).  With torch.distributed initialised and more than one
    rank in ``group`` (None: the default group), ONE all-reduce of the fp64 vector ``sums || count`` comes first: every
    rank gets (sum over ranks of sums) / (sum over ranks of count).  The reference averages every sample's scalars over
    the ranks instead (``reduce_scalar_outputs``): with DistributedSampler's equal counts the same mean, summed in
    another order."""
    import torch.distributed as dist
    vec = torch.cat([sums.to(torch.float64).reshape(-1), count.to(torch.float64).reshape(-1)])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(vec, group=group)
    host = vec.tolist()                      # (the one read-back)
    if len(host) != len(names) + 1:
        raise RuntimeError("reduce_scalar_sums: %d sums for the %d names of %s" % (len(host) - 1, len(names),
                           "SCALAR_NAMES" if names is SCALAR_NAMES else "names %r" % (tuple(names),)))
    n = host[-1]
    return {k: (v / n if n else float("nan")) for k, v in zip(names, host[:-1])}


class Validator:
    """One validation batch -- eval forward, ``validation_scalars``, accumulation into the epoch's running sums -- as one
    hipGraph on static input buffers (``capture=False``: the identical sequence, eagerly).

    ``__call__`` copies a new batch of the same shapes into the static buffers, replays and returns the static [17] row
    (``SCALAR_NAMES`` order; overwritten by the next call, never read back here): no host synchronisation.  ``mean()``
    is the one synchronising call: the epoch's averages as Python floats.  ``reset()`` starts a new epoch.

    The graph replays the weights as they were folded at capture.  Weights move between validation epochs, so every
    call compares ``model._state_stamp()`` (eager optimizer steps, ``load_state_dict``, a captured training step's
    replay all change it) with the stamp recorded at capture and re-captures when they differ -- plans rebuilt, the
    running sums kept.  The model must be in eval mode (``model.eval()`` / ``model.train()`` around the epoch, as in
    the reference)."""

    def __init__(self, model, imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms, capture=True, **loss_kwargs):
        if model.training:
            raise RuntimeError("Validator runs the eval forward: call model.eval() first")
        self.model, self.loss_kwargs, self.capture = model, loss_kwargs, capture
        self.imgs = [i.clone() for i in imgs]
        self.proj = {k: v.clone() for k, v in proj_matrices.items()}
        self.depth_values = depth_values.clone()
        self.gt = {k: v.clone() for k, v in depth_gt_ms.items()}
        self.mask = {k: v.clone() for k, v in mask_ms.items()}
        dev = self.depth_values.device
        self.sums = torch.empty(len(SCALAR_NAMES), dtype=torch.float64, device=dev)
        self.count = torch.empty(1, dtype=torch.int64, device=dev)
        self.reset()
        self.graph = self.row = self.outputs = self.plans = self.stamp = None
        if capture:
            self._capture()

    def _batch(self, sums, count):
        with torch.no_grad():
            outputs = self.model.forward_eager(self.imgs, self.proj, self.depth_values)
            row = validation_scalars(outputs, self.gt, self.mask, **self.loss_kwargs)
            ops.scalar_accumulate(row, sums, count)
        return outputs, row

    def _capture(self):
        self.graph = self.row = self.outputs = None            # (a re-capture: the old graph's pool goes first)
        scratch = torch.zeros_like(self.sums), torch.zeros_like(self.count)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                                 # builds the plans, warms the allocator; the epoch's sums stay
                self._batch(*scratch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.plans = self.model._get_plans()                   # (kept alive: the graph holds raw pointers into them)
        self.stamp = self.model._state_stamp()
        graph = torch.cuda.CUDAGraph()
        # thread-local capture: a validation epoch runs inside a training driver, where other threads touch the device too
        # (the DataLoader's pin-memory thread, RCCL's watchdog); see graph._CachedForward
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            self.outputs, self.row = self._batch(self.sums, self.count)
        self.graph = graph

    def _load(self, static, new, what):
        if tuple(new.shape) != tuple(static.shape):
            raise RuntimeError("Validator: %s is %s, the static buffer %s (one Validator per batch shape)"
                               % (what, tuple(new.shape), tuple(static.shape)))
        static.copy_(new, non_blocking=True)

    def __call__(self, imgs=None, proj_matrices=None, depth_values=None, depth_gt_ms=None, mask_ms=None):
        if self.model.training:
            raise RuntimeError("Validator runs the eval forward: call model.eval() first")
        if imgs is not None:
            if len(imgs) != len(self.imgs):
                raise RuntimeError("Validator: %d views, captured with %d" % (len(imgs), len(self.imgs)))
            for i, (dst, src) in enumerate(zip(self.imgs, imgs)):
                self._load(dst, src, "imgs[%d]" % i)
        for static, new, what in ((self.proj, proj_matrices, "proj_matrices"), (self.gt, depth_gt_ms, "depth_gt_ms"),
                                  (self.mask, mask_ms, "mask_ms")):
            if new is not None:
                for k in static:
                    self._load(static[k], new[k], "%s[%r]" % (what, k))
        if depth_values is not None:
            self._load(self.depth_values, depth_values, "depth_values")
        if not self.capture:
            self.outputs, self.row = self._batch(self.sums, self.count)
            return self.row
        if self.model._state_stamp() != self.stamp:
            self._capture()                                    # the weights moved: never replay stale folded weights
        self.graph.replay()
        return self.row

    def reset(self):
        """Zero the running sums and the count (one launch)."""
        ops.scalar_reset(self.sums, self.count)

    def mean(self, group=None):
        """The averages over the calls since ``reset()`` as ``{name: float}`` (``SCALAR_NAMES``): the one synchronising
        call -- one read-back of ``sums || count``, after one all-reduce of it when ``group`` (None: the default group of an
        initialised torch.distributed) has more than one rank."""
        return reduce_scalar_sums(self.sums, self.count, group)

    def last_images(self):
        """The reference's ``image_outputs`` of the last batch that it computes (train_mvs4.py:297-302): ``depth_est``
        (masked), ``depth_est_nomask``, ``errormap`` as fresh device tensors -- tensor expressions outside the graph, made
        only when asked."""
        if self.outputs is None:
            raise RuntimeError("Validator.last_images: no batch has run yet")
        last = "stage%d" % len(self.gt)
        depth, gt, mask = self.outputs["depth"], self.gt[last], self.mask[last]
        return {"depth_est": depth * mask, "depth_est_nomask": depth.clone(), "errormap": (depth - gt).abs() * mask}


def validate(model, batches, **loss_kwargs):
    """A validation epoch over an iterable of ``(imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms)`` batches of one
    shape (GPU tensors): -> ``Validator.mean()``.  The model must be in eval mode."""
    v = None
    for batch in batches:
        if v is None:
            v = Validator(model, *batch, **loss_kwargs)
            v()
        else:
            v(*batch)
    if v is None:
        raise ValueError("validate: no batches")
    return v.mean()
