"""Scan-level inference: images and cameras of a whole scan in, the depth and confidence maps of all its reference
views out, on the GPU -- the reference's per-sample loop ``save_scene_depth`` (test_mvs4.py:170-268) as one call.

What the loop recomputes and this path does not:

* **FPN once per image.**  A scan of V images with R reference views of ``nviews`` views each runs FPN4 on ``R * nviews``
  images in the loop; only V are distinct, and FPN4 in eval mode is a per-image function.  Here the FPN plan runs over the
  distinct images in chunks of ``nviews`` (the per-sample batch, so ``conv_plan`` picks the same kernels) and writes the
  four pyramid levels into per-scan *level stores* ``[V,h,w,C]``.
* **One upload per image**, as 8-bit pixels (``ops.pack_images_u8``: 3 instead of 12 bytes per pixel).
* **Cascade per reference view from the stores.**  ``MVS4net._cascade_eval`` -- the very body of the per-sample forward
  after the FPN -- reads the stores through ``ops.warp_agg_fwd_indexed_cl`` and a device view table.  It is captured once
  per scan shape as a hipGraph whose only per-sample inputs are ONE small device buffer (view table, projection stacks,
  ``depth_values``: ~3.5 kB); ``in_flight`` instances replay on streams of their own.  The graph is a single chain of
  launches; nothing here sets anything about hardware queues.
* The maps stay on the device: ``reconstruct_scan`` hands them to ``fusion.fuse_scene`` where they are.

Same kernels on the same operands as ``model(imgs, proj_matrices, depth_values)`` per sample: ``depth`` and
``photometric_confidence`` are bit-equal to it (tests/test_gpu_scan.py).

Scans at their native image size (``max_h`` / ``max_w``): the loader's input scaling
(``general_eval4.MVSDataset.scale_mvs_input``) runs in the launch that packs the 8-bit images
(``ops.load_pack_images_u8``), the intrinsics are scaled on the host.  Without these arguments all images of a scan
must have one admissible size.

The reference's two other evaluation loaders (``crop_rows`` = ``datasets/tanks.py``, ``img_wh`` = ``datasets/eth3d.py``,
``depth_range_kind="min_max"`` for both): a crop, or a resize of every view from its own native
size to one target, in the same launch.  ``plan_inputs`` is the host side of all three.  Those loaders run a reference view
whose pair list is shorter than ``nviews - 1`` with the views it has; ``short_sources="fewer_views"`` does the same on the one
captured cascade: the warp launches read a per-sample source count from the sample's row (``ops.warp_agg_fwd_indexed_cl(...,
nsrc=...)``).
"""
import collections
import os
import weakref

import numpy as np
import torch

from . import formats, ops

ScanPlan = collections.namedtuple("ScanPlan", "ref_views view_table proj depth_values fusion_pairs source_counts")
ScanPlan.__doc__ = """Host planning of a scan (pure NumPy).  ``ref_views`` [R] view numbers that get a depth map, ``view_table``
int32 [R,nviews] (column 0 = the reference view, then its sources cut / padded as ``formats.eval_view_list`` does),
``proj`` dict stage1..4 -> [V,2,4,4] (``formats.stage_proj_matrices`` over ALL views: a sample's stack is
``proj[stage][view_table[r]]``), ``depth_values`` [R,ndv], ``fusion_pairs`` the pairs with sources, full source lists,
``source_counts`` int32 [R]: the sources row r runs with -- ``nviews - 1`` everywhere unless ``short_sources="fewer_views"``,
where a shorter list keeps its length and the unused slots of its row hold the reference view's own number (a valid
index with a finite projection stack, which the counted kernels never read)."""

SHORT_SOURCES = (None, "fewer_views")


def _check_short_sources(short_sources):
    if short_sources not in SHORT_SOURCES:
        raise RuntimeError("infer_scan: short_sources = %r (None or 'fewer_views')" % (short_sources,))


def _as_pairs(pairs, V):
    out = []
    for entry in pairs:
        r, srcs = int(entry[0]), [int(v) for v in entry[1]]
        for v in [r] + srcs:
            if not 0 <= v < V:
                raise RuntimeError("infer_scan: pairs name view %d, which lies outside the scan's %d views" % (v, V))
        out.append((r, srcs))
    return out


DEPTH_RANGE_KINDS = ("min_interval", "min_max")


def plan_scan(Ks, Es, depth_ranges, pairs, nviews=5, ndepths=192, depth_range_kind="min_interval", short_sources=None):
    """Per-view quarter-resolution intrinsics ``Ks`` [V,3,3] and extrinsics ``Es`` [V,4,4] (``formats.read_cam_file``),
    ``depth_ranges`` [V] of (depth_min, depth_interval) or ready ``depth_values`` [V,ndv], ``pairs`` as
    ``formats.read_pair_file`` -> ScanPlan.  View list per reference view as ``formats.eval_view_list`` +
    ``formats.load_eval_sample``: sources cut to ``nviews - 1``, short lists padded by repeating the first source,
    reference views without sources dropped.  ``depth_range_kind="min_max"``: ``depth_ranges`` [V,2] holds (depth_min,
    depth_max), the two values ``datasets/tanks.py:131`` and ``datasets/eth3d.py:133`` hand to the forward, and goes through
    as a sample's ``depth_values`` (ndv = 2) -- the forward reads the first and the last entry and the count, so this is a
    different input from the 192 values the default builds, not a shorthand for them.

    ``short_sources="fewer_views"``: a reference view with fewer than ``nviews - 1`` sources runs with the sources it has, as
    ``datasets/tanks.py:68`` and ``datasets/eth3d.py`` do (they cut a list and never pad it) -- ``source_counts`` says how
    many, nothing is padded by repetition.  With the DTU loader's inputs this DIFFERS from ``general_eval4``'s padding: the
    result is the forward on the unpadded sample."""
    _check_short_sources(short_sources)
    if depth_range_kind not in DEPTH_RANGE_KINDS:
        raise RuntimeError("infer_scan: depth_range_kind = %r (one of %s)" % (depth_range_kind, ", ".join(DEPTH_RANGE_KINDS)))
    Ks = np.asarray(Ks, dtype=np.float32)
    Es = np.asarray(Es, dtype=np.float32)
    V = len(Ks)
    if Ks.shape != (V, 3, 3) or Es.shape != (V, 4, 4):
        raise RuntimeError("infer_scan: Ks must be [V,3,3] and Es [V,4,4], got %s and %s" % (Ks.shape, Es.shape))
    if nviews < 2:
        raise RuntimeError("infer_scan: nviews = %d (at least one source view is needed)" % nviews)
    pairs = _as_pairs(pairs, V)
    dr = np.asarray(depth_ranges, dtype=np.float32)
    if depth_range_kind == "min_max" and (dr.ndim != 2 or dr.shape != (V, 2)):
        raise RuntimeError("infer_scan: depth_ranges must be [V,2] (depth_min, depth_max) with depth_range_kind = 'min_max', "
                           "got %s for %d views" % (dr.shape, V))
    if dr.ndim != 2 or dr.shape[0] != V or dr.shape[1] < 2:
        raise RuntimeError("infer_scan: depth_ranges must be [V,2] (depth_min, depth_interval) or depth_values [V,ndv], "
                           "got %s for %d views" % (dr.shape, V))
    ref_views, table, dvs, fusion_pairs, counts = [], [], [], [], []
    for r, srcs in pairs:
        if not srcs:
            continue                                                        # (read_pair_file drops these too)
        fusion_pairs.append((r, list(srcs)))
        counts.append(min(len(srcs), nviews - 1) if short_sources == "fewer_views" else nviews - 1)
        if short_sources == "fewer_views":
            srcs = srcs + [r] * (nviews - len(srcs))                        # (unused slots: the reference's own number)
        elif len(srcs) < nviews:
            srcs = srcs + [srcs[0]] * (nviews - len(srcs))                  # general_eval4.py:47-49
        ref_views.append(r)
        table.append([r] + srcs[:nviews - 1])
        if depth_range_kind == "min_max":
            dvs.append(dr[r])                                               # np.array([depth_min, depth_max], float32)
        elif dr.shape[1] == 2:
            # (the Python floats read_cam_file returns; a float32 array holds them exactly when they came from one)
            dvs.append(formats.depth_value_range(float(depth_ranges[r][0]), float(depth_ranges[r][1]), ndepths))
        else:
            dvs.append(dr[r])
    if not ref_views:
        raise RuntimeError("infer_scan: no reference view with a source view in pairs")
    return ScanPlan(np.array(ref_views, dtype=np.int64), np.array(table, dtype=np.int32),
                    formats.stage_proj_matrices(Ks, Es), np.stack(dvs).astype(np.float32), fusion_pairs,
                    np.array(counts, dtype=np.int32))


def store_bytes(V, H, W, base_channels=8):
    """Bytes of the four level stores: ``V * H * W * 15 * 4`` for the shipped FPN (8 + 16/4 + 32/16 + 64/64 channels per
    full-resolution pixel)."""
    c = base_channels
    return V * (H * W * c + (H // 2) * (W // 2) * 2 * c + (H // 4) * (W // 4) * 4 * c + (H // 8) * (W // 8) * 8 * c) * 4


def _check_images(images, scaling=False):
    """-> ("u8", [V,H,W,3], [(H, W)] * V) or ("f32", [V,3,H,W], ...): the stack as given (array or tensor, not copied; a
    sequence of views is stacked), after the shape checks.  ``scaling``: the caller brings the images to an admissible size
    (``_scaled_inputs``), so any one common size passes."""
    if not torch.is_tensor(images) and not isinstance(images, np.ndarray):
        images = list(images)
        if not images:
            raise RuntimeError("infer_scan: no images")
        first = tuple(images[0].shape)
        for i, im in enumerate(images):
            if tuple(im.shape) != first and scaling:
                raise RuntimeError("infer_scan: image %d is %s but image 0 is %s: views of different native sizes within a "
                                   "scan are not supported (the reference resamples each source view to its reference "
                                   "view's size, so one image would need a level-store entry per partner size)"
                                   % (i, tuple(im.shape), first))
            if tuple(im.shape) != first:
                raise RuntimeError("infer_scan: image %d is %s but image 0 is %s: all views of a scan must have one size "
                                   "(resize the images first)" % (i, tuple(im.shape), first))
        images = torch.stack(images) if torch.is_tensor(images[0]) else np.stack(images)
    dt = images.dtype
    if dt in (torch.uint8, np.dtype(np.uint8)):
        kind = "u8"
        if images.ndim != 4 or images.shape[3] != 3:
            raise RuntimeError("infer_scan: uint8 images must be [V,H,W,3], got %s" % (tuple(images.shape),))
        H, W = images.shape[1], images.shape[2]
    elif dt in (torch.float32, np.dtype(np.float32)):
        kind = "f32"
        if images.ndim != 4 or images.shape[1] != 3:
            raise RuntimeError("infer_scan: float32 images must be [V,3,H,W], got %s" % (tuple(images.shape),))
        H, W = images.shape[2], images.shape[3]
    else:
        raise RuntimeError("infer_scan: images must be uint8 [V,H,W,3] or float32 [V,3,H,W], got %s" % (dt,))
    if (H % 64 or W % 64 or H == 0 or W == 0) and not (scaling and H > 0 and W > 0):
        raise RuntimeError("infer_scan: image size %dx%d: H and W must be multiples of 64 (resampling stays outside the "
                           "path: resize the images first)" % (H, W))
    return kind, images, [(int(H), int(W))] * int(images.shape[0])


def _scaled_inputs(kind, H, W, Ks, max_h, max_w):
    """The loader's target size and intrinsics for ``H`` x ``W`` images within ``max_h`` x ``max_w`` (``None``: that side
    is not limited) -> (Hd, Wd, scaled copy of ``Ks``)."""
    Hd, Wd, scale_h, scale_w = formats.scale_input_size(H, W, H if max_h is None else max_h, W if max_w is None else max_w)
    if Hd < 64 or Wd < 64:
        raise RuntimeError("infer_scan: image size %dx%d within max_h = %s, max_w = %s gives %dx%d: nothing is left after "
                           "rounding down to multiples of 64" % (H, W, max_h, max_w, Hd, Wd))
    if kind == "f32" and (Hd, Wd) != (H, W):
        raise RuntimeError("infer_scan: float32 images of %dx%d would be resampled to %dx%d, which is done for uint8 images "
                           "only: pass the decoded 8-bit images as uint8 [V,H,W,3]" % (H, W, Hd, Wd))
    return Hd, Wd, formats.scale_intrinsics(Ks, scale_h, scale_w)


def _check_views(images):
    """The images of a scan in the ``crop_rows`` / ``img_wh`` modes -> (kind, list of per-view arrays or tensors as given,
    [(Hs, Ws)] per view): uint8 [H,W,3] views, whose sizes may differ, or float32 [3,H,W] ones."""
    views = list(images)
    if not views:
        raise RuntimeError("infer_scan: no images")
    for i, im in enumerate(views):
        if not torch.is_tensor(im) and not isinstance(im, np.ndarray):
            raise RuntimeError("infer_scan: image %d is a %s, not an array or a tensor" % (i, type(im).__name__))
    dt = views[0].dtype
    if any(im.dtype != dt for im in views):
        raise RuntimeError("infer_scan: the images of a scan must have one dtype")
    if dt in (torch.uint8, np.dtype(np.uint8)):
        kind, sizes = "u8", [tuple(im.shape[:2]) for im in views]
        bad = [i for i, im in enumerate(views) if im.ndim != 3 or im.shape[2] != 3]
    elif dt in (torch.float32, np.dtype(np.float32)):
        kind, sizes = "f32", [tuple(im.shape[1:]) for im in views]
        bad = [i for i, im in enumerate(views) if im.ndim != 3 or im.shape[0] != 3]
    else:
        raise RuntimeError("infer_scan: images must be uint8 [V,H,W,3] or float32 [V,3,H,W], got %s" % (dt,))
    if bad:
        raise RuntimeError("infer_scan: image %d is %s: views must be uint8 [H,W,3] or float32 [3,H,W]"
                           % (bad[0], tuple(views[bad[0]].shape)))
    return kind, views, [(int(h), int(w)) for h, w in sizes]


def _dataset_inputs(kind, sizes, Ks, crop_rows, img_wh):
    """Target size, crop and intrinsics of the two dataset modes -> (Hd, Wd, (top, bottom, left, right), adjusted copy of
    ``Ks``).  ``Ks`` comes and goes in the quarter-resolution convention; the loaders' own operations (``cy - top``,
    datasets/tanks.py:58; a Python-float factor per view and axis, datasets/eth3d.py:89-90) act on the full-resolution
    matrix in between -- the factors 4 and 1/4 are exact, so these are the loaders' bits."""
    Ks = np.array(Ks, dtype=np.float32)
    Ks[:, :2, :] *= 4.0
    if crop_rows is not None:
        top, bottom = int(crop_rows[0]), int(crop_rows[1])
        if top < 0 or bottom < 0:
            raise RuntimeError("infer_scan: crop_rows = %s" % ((top, bottom),))
        for i, hw in enumerate(sizes):
            if hw != sizes[0]:
                raise RuntimeError("infer_scan: image %d is %dx%d but image 0 is %dx%d: with crop_rows all views of a scan must "
                                   "have one size (nothing is resampled)" % ((i,) + hw + sizes[0]))
        Hd, Wd = sizes[0][0] - top - bottom, sizes[0][1]
        if Hd < 64 or Wd < 64 or Hd % 64 or Wd % 64:
            raise RuntimeError("infer_scan: image size %dx%d with crop_rows = %s leaves %dx%d: H and W must be positive "
                               "multiples of 64" % (sizes[0] + ((top, bottom), Hd, Wd)))
        crop = (top, bottom, 0, 0)
        Ks = formats.crop_intrinsics(Ks, top, 0)
    else:
        Wd, Hd = int(img_wh[0]), int(img_wh[1])
        if Hd < 64 or Wd < 64 or Hd % 64 or Wd % 64:
            raise RuntimeError("infer_scan: img_wh = (%d, %d): W and H must be positive multiples of 64" % (Wd, Hd))
        for i, (h, w) in enumerate(sizes):
            if h < Hd or w < Wd:
                raise RuntimeError("infer_scan: image %d is %dx%d, smaller than img_wh = (%d, %d) (%dx%d): nothing here "
                                   "enlarges an image" % (i, h, w, Wd, Hd, Hd, Wd))
            Ks[i] = formats.scale_intrinsics(Ks[i], Hd / h, Wd / w)
        crop = (0, 0, 0, 0)
    if kind == "f32" and (any(hw != (Hd, Wd) for hw in sizes) or any(crop)):
        raise RuntimeError("infer_scan: float32 images of %dx%d would be cropped or resampled to %dx%d, which is done for "
                           "uint8 images only: pass the decoded 8-bit images as uint8 [H,W,3]" % (sizes[0] + (Hd, Wd)))
    Ks[:, :2, :] /= 4.0
    return Hd, Wd, crop, Ks


ScanInputs = collections.namedtuple("ScanInputs", "kind images V sizes H W crop Ks source_bytes prepare exact_sources")
ScanInputs.__doc__ = """What ``plan_inputs`` makes of a scan's images and intrinsics.  ``kind`` "u8" / "f32"; ``images`` as given
(a stack, or the list of views; float32 views and, in the ``max_h`` / ``max_w`` mode, any sequence stacked); ``V``; ``sizes``
[(Hs, Ws)] per view; the target ``H``, ``W``; ``crop`` (top, bottom, left, right); ``Ks`` adjusted to the prepared images;
``prepare``: the images go through ``ops.load_pack_images_u8`` (uint8 images with one of the three preparations, even
where it leaves the size alone), and ``source_bytes`` is what that reads; ``exact_sources``: the loader cuts source lists
and never pads them (``_check_source_counts``, unless ``short_sources="fewer_views"`` runs them as they are)."""


def plan_inputs(images, Ks, max_h=None, max_w=None, crop_rows=None, img_wh=None, Es=None):
    """Host side of the three loaders' image preparations (pure NumPy, no device) -> ScanInputs.  ``max_h`` / ``max_w``:
    every view resized to one target computed from the common native size, nothing cropped; ``crop_rows``, ``img_wh``:
    ``_dataset_inputs``; none of them: the images must have one admissible size already.  ``Es``: where given, its length
    and that of ``Ks`` are checked against the number of views."""
    scaling = max_h is not None or max_w is not None
    datasets = crop_rows is not None or img_wh is not None
    if scaling + (crop_rows is not None) + (img_wh is not None) > 1:
        raise RuntimeError("infer_scan: crop_rows, img_wh and max_h / max_w are three loaders' image preparations: give one "
                           "of them")
    if datasets:
        kind, views, sizes = _check_views(images)
        if not torch.is_tensor(images) and not isinstance(images, np.ndarray):
            images = views                                                  # (a stack stays whole: it can be read where it lies)
    else:
        kind, images, sizes = _check_images(images, scaling)
    V = len(sizes)
    if Es is not None and (len(Ks) != V or len(Es) != V):
        raise RuntimeError("infer_scan: %d images for %d intrinsics and %d extrinsics" % (V, len(Ks), len(Es)))
    (H, W), crop = sizes[0], (0, 0, 0, 0)
    if datasets:
        H, W, crop, Ks = _dataset_inputs(kind, sizes, Ks, crop_rows, img_wh)
        if kind == "f32" and images is views:                               # (already at the target size: nothing to prepare)
            images = torch.stack(views) if torch.is_tensor(views[0]) else np.stack(views)
    elif scaling:
        H, W, Ks = _scaled_inputs(kind, H, W, Ks, max_h, max_w)
    prepare = (scaling or datasets) and kind == "u8"
    source_bytes = sum(h * w * 3 for h, w in sizes) if prepare else 0
    return ScanInputs(kind, images, V, sizes, H, W, crop, Ks, source_bytes, prepare, datasets)


def _check_source_counts(pairs, nviews, view_ids=None):
    """The dataset modes cut a source list to ``nviews - 1`` and never pad it (datasets/tanks.py:68).  Without
    ``short_sources="fewer_views"`` -- which runs such a view with the sources it has, the loaders' behaviour -- a shorter
    list is refused here, naming the view and the keyword."""
    for r, srcs in pairs:
        if 0 < len(srcs) < nviews - 1:
            name = int(r) if view_ids is None else int(view_ids[int(r)])
            raise RuntimeError("infer_scan: reference view %d has %d source views, fewer than nviews - 1 = %d: the Tanks and "
                               "Temples / ETH3D loaders would run it with %d views, but a captured graph has one view count, "
                               "and padding the list (as the DTU loader does) would change the result; pass "
                               "short_sources='fewer_views' to run it as the loaders do, lower nviews or drop "
                               "the view from pairs" % (name, len(srcs), nviews - 1, len(srcs) + 1))


class ScanResult(dict):
    """What ``infer_scan`` returns: ``ref_views`` [R] (view numbers, host), ``depth`` and ``photometric_confidence`` [R,H,W]
    on the GPU, ``Ks`` [V,3,3] / ``Es`` [V,4,4] at output resolution (the stage-4 camera ``write_cam`` gets in the
    reference), ``pairs`` (reference views with sources, full source lists: what fusion reads), ``view_ids`` (file
    numbers of the views), ``stats`` (``fpn_runs``, ``replays``, ``captured``) and whatever else ``keep`` named.  With ``max_h`` / ``max_w``,
    ``crop_rows`` or ``img_wh``: ``images``, the prepared uint8 images [V,H,W,3] on the GPU, and ``Ks`` from the adjusted
    intrinsics."""

    def timings(self):
        """Milliseconds per phase (HIP events recorded by ``infer_scan``; synchronises).  ``upload``: the images and the
        per-sample rows, and with ``max_h`` / ``max_w``, ``crop_rows`` or ``img_wh`` the launch that prepares and packs the
        images (``ops.load_pack_images_u8``: the copy is the bulk of it) -- for all three, not under ``fpn``."""
        torch.cuda.synchronize()
        ev = self.get("events", {})
        return {k: a.elapsed_time(b) for k, (a, b) in ev.items()}


class _Instance:
    """One captured cascade: a static per-sample input buffer, the graph, its static outputs, a stream.  Holds no reference
    back to its runner: a dropped runner must free its graphs by reference count, at once -- a hipGraph destroyed later by
    the cycle collector, while this thread captures another one, aborts the process."""

    def __init__(self, runner, regs):
        dev = runner.dev
        self.stream = torch.cuda.Stream(device=dev)
        self.buf = torch.zeros(runner.row, dtype=torch.float32, device=dev)
        n = runner.nviews
        self.views = self.buf[:n].view(torch.int32).view(1, n)
        self.nsrc = self.buf[n:n + 1].view(torch.int32) if runner.counted else None   # [1]: this sample's source count
        self.pms = [self.buf[o:o + n * 32].view(1, n, 2, 4, 4) for o in runner.proj_off]
        self.dv = self.buf[runner.dv_off:runner.dv_off + runner.ndv].view(1, runner.ndv)
        self.graph = None
        self.outputs = None
        self.regs, self.stores, self.shape = regs, runner.stores, (n, runner.H, runner.W)

    def run(self, model):
        n, H, W = self.shape
        rts = ops.relative_projection_multi(self.pms)
        depth_interval = None
        if not model.inverse_depth:
            depth_interval = (self.dv[:, -1] - self.dv[:, 0]) / self.dv.size(1)
        return model._cascade_eval(self.stores, self.regs, n, 1, H, W, rts, self.dv, depth_interval, views=self.views,
                                   nsrc=self.nsrc)

    def capture(self, model):
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.outputs = self.run(model)


class _ScanRunner:
    """Level stores + captured cascades of one (model state, V, H, W, nviews, ndv, counted) combination; the captured
    instances grow with the largest ``in_flight`` asked for.  ``counted``: the cascade's warp launches are the counted
    entries and read the sample's source count from its row -- one graph for every count from 1 to ``nviews - 1``."""

    def __init__(self, model, V, H, W, nviews, ndv, stamp, counted=False):
        self.dev = next(model.parameters()).device
        self.V, self.H, self.W, self.nviews, self.ndv, self.stamp, self.counted = V, H, W, nviews, ndv, stamp, counted
        c = model.feature.out_channels                                       # [8c, 4c, 2c, c] for stages 1..4
        self.stores = [torch.empty(V, H >> (3 - s), W >> (3 - s), c[s], device=self.dev, dtype=torch.float32)
                       if s < model.num_stage else None for s in range(4)]
        # per-sample row: view table and source count (int32 bits), one projection stack per stage, depth_values; 64-float
        # segments
        seg = lambda k: (k + 63) // 64 * 64
        off = seg(nviews + 1)
        self.proj_off = []
        for _ in range(model.num_stage):
            self.proj_off.append(off)
            off += seg(nviews * 32)
        self.dv_off = off
        self.row = off + seg(ndv)
        self.plans = model._get_plans()                                      # (kept alive: the graphs hold pointers into them)
        self.instances = []

    def rows(self, plan, num_stage, entries=None):
        """All per-sample rows of a scan on the host: [R, row] float32 (the store entries and the count as raw int32 bits).
        ``entries``: the store entries [R,nviews] the warp kernel reads where they are not the view numbers (``_short_entries``)."""
        R = len(plan.ref_views)
        host = np.zeros((R, self.row), dtype=np.float32)
        host[:, :self.nviews] = np.ascontiguousarray(plan.view_table if entries is None else entries, dtype=np.int32).view(np.float32)
        host[:, self.nviews] = plan.source_counts.view(np.float32)
        for s in range(num_stage):
            pm = plan.proj["stage%d" % (s + 1)][plan.view_table]            # [R,nviews,2,4,4]
            host[:, self.proj_off[s]:self.proj_off[s] + self.nviews * 32] = pm.reshape(R, -1)
        host[:, self.dv_off:self.dv_off + self.ndv] = plan.depth_values
        return host


_RUNNERS = weakref.WeakKeyDictionary()          # model -> _ScanRunner (one scan shape resident per model: the stores are large)


def _runner(model, V, H, W, nviews, ndv, counted=False):
    stamp = model._state_stamp()
    from .graph import ForwardCache
    # (the switches that pick kernels or launches: flipped between two calls they are a different graph)
    cfg = ForwardCache.key(model, [torch.empty(1, 3, 1, 1)], {}, torch.empty(1, ndv))[-1]
    key = (V, H, W, nviews, ndv, stamp, cfg, counted)
    hit = _RUNNERS.get(model)
    if hit is None or hit[0] != key:
        if hit is not None:
            hit[1].instances.clear()             # the old graphs and stores go now, before anything new is allocated or captured
            hit = None
            del _RUNNERS[model]
        hit = _RUNNERS[model] = (key, _ScanRunner(model, V, H, W, nviews, ndv, stamp, counted))
    return hit[1]


def _short_entries(plan, V, nviews):
    """Store entries for the reference views that run with fewer sources -> (entries [R,nviews], pages, number of store
    entries).  The per-sample forward runs the FPN on a sample's OWN ``1 + n`` images, and ``conv_plan`` picks kernels by
    batch: in a batch of ``1 + n < nviews`` images a view's features need not carry the bits they have in a batch of
    ``nviews`` (at 128 x 128 a batch of 2 takes other kernels than one of 4 in 12 of the FPN's 18 layers).  So the views of
    the samples with n sources get further entries behind the scan's V, computed in batches of ``1 + n``; ``pages`` lists
    them as (batch, views, first entry) per distinct short count, and the rows of those samples name these entries."""
    entries = np.array(plan.view_table, dtype=np.int32)
    pages, first = [], V
    for n in sorted(set(int(c) for c in plan.source_counts if c < nviews - 1)):
        rows = np.flatnonzero(plan.source_counts == n)
        views = sorted({int(v) for r in rows for v in plan.view_table[r, :1 + n]})
        at = {v: first + i for i, v in enumerate(views)}
        for r in rows:
            entries[r] = at[int(plan.view_table[r, 0])]                      # (unused slots: the reference's own entry)
            entries[r, :1 + n] = [at[int(v)] for v in plan.view_table[r, :1 + n]]
        pages.append((1 + n, views, first))
        first += len(views)
    return entries, pages, first


def _run_fpn(model, runner, kind, dev_images, chunk, packed=None, V=None, pages=()):
    """The FPN plan over the distinct images, ``chunk`` at a time (last chunk padded by repeating its last image), each
    level into its store; then the ``pages`` of ``_short_entries``, each in batches of its own size.  ``packed``: the RGB0
    stack where the caller has made it already; ``V``: the number of images (default: of store entries).  -> number of plan
    runs."""
    fpn = runner.plans[0]
    V = runner.V if V is None else V
    if packed is None and kind == "u8":
        packed = ops.pack_images_u8(dev_images)                              # [V,1,H,W,4], one launch for the scan
    runs = 0
    for batch, views, first in [(chunk, list(range(V)), 0)] + list(pages):
        for a in range(0, len(views), batch):
            b = min(len(views), a + batch)
            idx = views[a:b] + [views[b - 1]] * (batch - (b - a))
            if kind == "u8":
                x = packed[idx[0]:idx[0] + batch] if idx == list(range(idx[0], idx[0] + batch)) else packed[idx]
            else:
                x = ops.pack_images([dev_images[i:i + 1] for i in idx])
            c0, c1, c3, f1 = fpn.trunk(x)
            levels = list(fpn.coarse(c3, f1)) + (list(fpn.tail(c0, c1, f1)) if model.num_stage > 2 else [None, None])
            for s in range(model.num_stage):
                runner.stores[s][first + a:first + b].copy_(levels[s][:b - a, 0])
            runs += 1
    return runs


@torch.no_grad()
def infer_scan(model, images, Ks, Es, depth_ranges, pairs, nviews=5, in_flight=2,
               keep=("depth", "photometric_confidence"), ndepths=192, fpn_chunk=None, max_store_bytes=None, view_ids=None,
               max_h=None, max_w=None, crop_rows=None, img_wh=None, depth_range_kind="min_interval", short_sources=None):
    """Depth and confidence maps of all reference views of a scan.

    ``images``: uint8 [V,H,W,3] (NumPy, or a tensor on the GPU) or float32 [V,3,H,W] in 0..1, or a sequence of per-view
    arrays; ``Ks`` [V,3,3] / ``Es`` [V,4,4]: per-view intrinsics in the quarter-resolution convention of
    ``formats.read_cam_file`` / ``formats.stage_proj_matrices`` and extrinsics; ``depth_ranges`` [V,2] = (depth_min,
    depth_interval) per view as ``read_cam_file`` returns them, or ready ``depth_values`` [V,ndv]; ``pairs`` as
    ``formats.read_pair_file``, indexing the V views.  All views must have one admissible size (H, W multiples of 64);
    anything else raises, as ``formats.load_eval_sample`` does.

    ``in_flight`` captured cascades replay on streams of their own.  ``keep``: the entries of the forward's output dict
    to return as [R,...] stacks -- last-stage names (``"depth"``) or ``"stage2.depth"``; after each replay only these
    are copied out of the graph's static outputs.  ``fpn_chunk``: images per FPN run (default ``nviews``: the
    per-sample batch, the only value that carries the bit-equality with the per-sample forward).  ``max_store_bytes``:
    raise if the level stores (``store_bytes``) would exceed it.

    ``max_h`` / ``max_w`` (both ``None``: nothing below applies): the reference loader's input scaling
    (``general_eval4.MVSDataset.scale_mvs_input``, e.g. 864 / 1152 for DTU).  uint8 images of any one common size are
    shrunk to fit, rounded down to multiples of 64 and resampled on the GPU in the launch that packs them
    (``ops.load_pack_images_u8``); ``Ks`` is scaled to match, and it is the scaled intrinsics the result carries.  The
    result's ``images`` are the resized uint8 images on the GPU (``write_scan_outputs`` and ``reconstruct_scan`` take
    them).  The source stack is extra device memory while it is packed -- ``V * Hs * Ws * 3`` bytes, 282 MB for 49
    views of 1200 x 1600 -- and counts towards ``max_store_bytes``.  float32 images that would need resampling and views
    of different native sizes raise.

    The reference's two other evaluation loaders (each alone, and not together with ``max_h`` / ``max_w``), both usually
    with ``depth_range_kind="min_max"`` (``plan_scan``: ``depth_ranges`` [V,2] = (depth_min, depth_max) per view, passed to
    the forward as they are):

    * ``crop_rows=(top, bottom)``, ``(28, 28)`` for Tanks and Temples (``datasets/tanks.py:53-60``): these rows are cut off
      every view without resampling and ``cy`` is shifted by ``top``.  All views must have one size and what is left must
      be admissible.
    * ``img_wh=(W, H)``, ``(1920, 1280)`` for ETH3D (``datasets/eth3d.py:57-62, :89-90``): every view is resized to this
      size, its intrinsics scaled by its own ``W / Ws``, ``H / Hs``.  ``images`` may be a sequence of views of different
      native sizes; none may be smaller than the target.

    Both run in the same launch; the result carries ``images`` (the prepared uint8 images on the GPU) and the adjusted
    ``Ks``, and the source bytes count towards ``max_store_bytes``, as above.  These loaders cut a source list to
    ``nviews - 1`` and never pad it; see ``short_sources``.

    ``short_sources``: what becomes of a reference view with fewer than ``nviews - 1`` sources (one without any is dropped
    either way).  ``None``: without ``crop_rows`` / ``img_wh`` its list is padded by repeating the first source, as the DTU
    loader does; with them it raises, naming the view.  ``"fewer_views"``: it runs with the sources it has, which is what the
    Tanks and Temples and ETH3D loaders do -- bit-equal to the per-sample forward on the shorter sample
    (``formats.load_tanks_sample`` / ``load_eth3d_sample``).  The scan still replays ONE captured cascade: the warp launches
    are the counted entries (``ops.warp_agg_fwd_indexed_cl(..., nsrc=...)``) and read each sample's count from its row, on
    every view of the scan, also where no list is short.  Allowed without ``crop_rows`` / ``img_wh`` too, where it differs
    from ``general_eval4``'s padding: the result is then the forward on the unpadded sample.  The views of a sample with n
    sources also get level-store entries of their own, computed in FPN batches of ``1 + n`` images as the per-sample forward
    does (``_short_entries``: the FPN's kernels are picked by batch) -- further FPN runs and store bytes, counted in ``stats``
    and against ``max_store_bytes``, only on scans that have such views.
    ``stats["short_views"]`` counts the reference views that ran with fewer sources.  -> ScanResult."""
    _check_short_sources(short_sources)
    counted = short_sources == "fewer_views"
    inp = plan_inputs(images, Ks, max_h, max_w, crop_rows, img_wh, Es)
    kind, V, H, W, Ks = inp.kind, inp.V, inp.H, inp.W, inp.Ks
    if inp.exact_sources and not counted:
        _check_source_counts(_as_pairs(pairs, V), nviews, view_ids)
    plan = plan_scan(Ks, Es, depth_ranges, pairs, nviews, ndepths, depth_range_kind, short_sources)
    if in_flight < 1:
        raise RuntimeError("infer_scan: in_flight = %d" % in_flight)
    chunk = int(fpn_chunk or nviews)
    if not 1 <= chunk <= 16:
        raise RuntimeError("infer_scan: fpn_chunk = %d (1..16 images per FPN run)" % chunk)
    entries, pages, store_views = _short_entries(plan, V, nviews) if counted else (None, (), V)
    need = store_bytes(store_views, H, W, model.feature.out_channels[-1])
    if max_store_bytes is not None and inp.prepare and need + inp.source_bytes > max_store_bytes:
        raise RuntimeError("infer_scan: the level stores of %d views of %dx%d and the %dx%d source images need %d + %d bytes "
                           "(%.2f GB), more than max_store_bytes = %d"
                           % (store_views, H, W, max(h for h, _ in inp.sizes), max(w for _, w in inp.sizes), need, inp.source_bytes,
                              (need + inp.source_bytes) / 1e9, max_store_bytes))
    if max_store_bytes is not None and need > max_store_bytes:
        raise RuntimeError("infer_scan: the level stores of %d views of %dx%d need %d bytes (%.2f GB), more than "
                           "max_store_bytes = %d" % (store_views, H, W, need, need / 1e9, max_store_bytes))
    if model.training:
        raise RuntimeError("infer_scan runs the eval forward: call model.eval() first")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("mvster_amd.scan.infer_scan runs on MI355X only: move the model to the GPU (there is no CPU "
                           "fallback)")
    keep = tuple(keep)
    R = len(plan.ref_views)
    ops.check_view_table(plan.view_table, V, "infer_scan")                  # (the kernels trust the device table)
    if entries is not None:
        ops.check_view_table(entries, store_views, "infer_scan")
    ops.check_source_counts(plan.source_counts, nviews - 1, R, "infer_scan")    # (... and the counts)
    main = torch.cuda.current_stream(dev)
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in ("upload", "fpn", "cascade")}

    with torch.cuda.device(dev):
        ev["upload"][0].record(main)
        runner = _runner(model, store_views, H, W, nviews, plan.depth_values.shape[1], counted)
        packed = small = dev_images = None
        if inp.prepare:                                                      # the upload and the launch that prepares and packs
            packed, small = ops.load_pack_images_u8(inp.images, H, W, crop=inp.crop, want_u8=True, device=dev)
        elif torch.is_tensor(inp.images):
            dev_images = inp.images.to(dev).contiguous()
        else:
            dev_images = torch.from_numpy(np.ascontiguousarray(inp.images)).to(dev)
        samples = torch.from_numpy(runner.rows(plan, model.num_stage, entries)).to(dev)   # all per-sample inputs: ONE upload
        ev["upload"][1].record(main)

        ev["fpn"][0].record(main)
        fpn_runs = _run_fpn(model, runner, kind, dev_images, chunk, packed, V, pages)
        del dev_images, packed                                               # (the full-size stack goes back to the allocator)
        ev["fpn"][1].record(main)

        # [K,R,...] stacks of the kept maps; same-shaped ones share one allocation (one staging copy moves them all)
        captured_now = len(runner.instances) < in_flight
        while len(runner.instances) < in_flight:
            inst = _Instance(runner, runner.plans[1])
            inst.buf.copy_(samples[0])
            if not runner.instances:                                         # eager once (plans, allocator), then capture
                first = inst.run(model)
                for name in keep:
                    _pick(first, name)                                       # (a wrong name raises before the capture)
                del first
            torch.cuda.synchronize(dev)
            inst.capture(model)
            runner.instances.append(inst)
        insts = runner.instances[:in_flight]
        srcs = [[_pick(inst.outputs, name) for name in keep] for inst in insts]
        shapes = [tuple(t.shape[1:]) for t in srcs[0]]
        same = len(set(shapes)) == 1
        if same:
            maps = torch.empty((len(keep), R) + shapes[0], device=dev, dtype=torch.float32)
            stacks = [maps[k] for k in range(len(keep))]
        else:
            maps = None
            stacks = [torch.empty((R,) + sh, device=dev, dtype=torch.float32) for sh in shapes]

        ev["cascade"][0].record(main)
        for inst in insts:
            inst.stream.wait_stream(main)
        for r in range(R):
            i = r % in_flight
            inst = insts[i]
            with torch.cuda.stream(inst.stream):
                inst.buf.copy_(samples[r], non_blocking=True)                # view table + projections + depth range
                inst.graph.replay()
                torch._foreach_copy_([st[r:r + 1] for st in stacks], srcs[i])   # only the kept maps leave the graph's buffers
        for inst in insts:
            main.wait_stream(inst.stream)
        ev["cascade"][1].record(main)

    k4 = plan.proj["stage4"] if "stage4" in plan.proj else None
    res = ScanResult(ref_views=plan.ref_views, pairs=plan.fusion_pairs,
                     Ks=k4[:, 1, :3, :3].copy(), Es=k4[:, 0].copy(),
                     view_ids=list(range(V)) if view_ids is None else [int(v) for v in view_ids],
                     stats={"fpn_runs": fpn_runs, "replays": R, "captured": captured_now, "store_bytes": need,
                            "short_views": int((plan.source_counts < nviews - 1).sum())}, events=ev)
    if inp.prepare:
        res["images"] = small
        res["stats"]["source_bytes"] = inp.source_bytes
    for name, st in zip(keep, stacks):
        res[name] = st
    res.maps, res.map_names = maps, keep
    return res


def _pick(outputs, name):
    cur = outputs
    for part in name.split("."):
        if not isinstance(cur, dict) or part not in cur:
            raise RuntimeError("infer_scan: keep names %r, which is not an entry of the forward's outputs" % name)
        cur = cur[part]
    if not torch.is_tensor(cur):
        raise RuntimeError("infer_scan: keep names %r, which is not a tensor" % name)
    return cur


DATASETS = {"general": ("cams", None), "tanks": ("cams", None), "eth3d": ("cams_1", 1)}   # cam folder, negative depth_min -> ...


def read_scan_folder(datapath, scan, interval_scale=1.06, ndepths=192, dataset="general"):
    """``datapath/scan/{images_post|images}/%08d.jpg``, ``cams/%08d_cam.txt``, ``pair.txt`` -> dict with ``images`` (list of
    uint8 [H,W,3]), ``Ks``, ``Es``, ``depth_ranges``, ``pairs`` (indices into the views) and ``view_ids`` (their file
    numbers, sorted): everything ``infer_scan`` takes.  Every file is read once.

    ``dataset="tanks"`` / ``"eth3d"``: the layouts ``datasets/tanks.py`` (``images/``, ``cams/``) and ``datasets/eth3d.py``
    (``images/``, ``cams_1/``) read, through ``formats.read_cam_file_minmax`` (ETH3D: a negative depth_min becomes 1):
    ``depth_ranges`` holds (depth_min, depth_max) -- ``depth_range_kind="min_max"`` -- and ``Ks`` the files' intrinsics
    brought to the quarter-resolution convention ``infer_scan`` takes (rows 0-1 divided by 4, exact)."""
    from PIL import Image
    if dataset not in DATASETS:
        raise RuntimeError("infer_scan_folder: dataset = %r (one of %s)" % (dataset, ", ".join(sorted(DATASETS))))
    cams, negative_min_to = DATASETS[dataset]
    root = os.path.join(datapath, scan)
    file_pairs = formats.read_pair_file(os.path.join(root, "pair.txt"))
    view_ids = sorted({v for r, srcs in file_pairs for v in [r] + srcs})
    paths = {}
    for v in view_ids:
        img = os.path.join(root, "images_post", "{:0>8}.jpg".format(v))
        if dataset != "general" or not os.path.exists(img):
            img = os.path.join(root, "images", "{:0>8}.jpg".format(v))
        cam = os.path.join(root, cams, "{:0>8}_cam.txt".format(v))
        for f in (img, cam):
            if not os.path.exists(f):
                raise RuntimeError("infer_scan_folder: pair.txt names view %d, but %s does not exist" % (v, f))
        paths[v] = (img, cam)
    slot = {v: i for i, v in enumerate(view_ids)}
    images, Ks, Es, ranges = [], [], [], []
    for v in view_ids:
        images.append(np.array(Image.open(paths[v][0]), dtype=np.uint8))
        if dataset == "general":
            K, E, dmin, dint = formats.read_cam_file(paths[v][1], interval_scale, ndepths)
        else:
            K, E, dmin, dint = formats.read_cam_file_minmax(paths[v][1], negative_min_to)   # (dint: depth_max here)
            K[:2, :] /= 4.0
        Ks.append(K)
        Es.append(E)
        ranges.append((dmin, dint))
    return dict(images=images, Ks=np.stack(Ks), Es=np.stack(Es), depth_ranges=ranges, view_ids=view_ids,
                pairs=[(slot[r], [slot[v] for v in srcs]) for r, srcs in file_pairs])


def _dataset_keywords(dataset, kw):
    """The keywords ``dataset`` stands for, unless the caller gave them: Tanks ``crop_rows=(28, 28)``, ETH3D
    ``img_wh=(1920, 1280)`` (the loaders' own constants), both ``depth_range_kind="min_max"``."""
    kw = dict(kw)
    if dataset == "tanks" and kw.get("crop_rows") is None and kw.get("img_wh") is None:
        kw["crop_rows"] = (28, 28)
    if dataset == "eth3d" and kw.get("crop_rows") is None and kw.get("img_wh") is None:
        kw["img_wh"] = (1920, 1280)
    if dataset != "general":
        kw.setdefault("depth_range_kind", "min_max")
    return kw


def plan_scan_folder(datapath, scan, nviews=5, interval_scale=1.06, ndepths=192, max_h=None, max_w=None, dataset="general",
                     crop_rows=None, img_wh=None, depth_range_kind=None, short_sources=None):
    """Host planning of ``infer_scan_folder`` -> (the ``read_scan_folder`` dict, ScanPlan); no device work.  With ``max_h`` /
    ``max_w``, ``crop_rows`` or ``img_wh`` the plan is made from the adjusted intrinsics (the dict keeps the files' own).
    ``short_sources``: as ``infer_scan``."""
    _check_short_sources(short_sources)
    sc = read_scan_folder(datapath, scan, interval_scale, ndepths, dataset)
    kw = _dataset_keywords(dataset, dict(crop_rows=crop_rows, img_wh=img_wh, **({} if depth_range_kind is None else
                                                                                {"depth_range_kind": depth_range_kind})))
    crop_rows, img_wh, kind_dr = kw["crop_rows"], kw["img_wh"], kw.get("depth_range_kind", "min_interval")
    inp = plan_inputs(sc["images"], sc["Ks"], max_h, max_w, crop_rows, img_wh)
    if inp.exact_sources and short_sources != "fewer_views":
        _check_source_counts(_as_pairs(sc["pairs"], inp.V), nviews, sc["view_ids"])
    return sc, plan_scan(inp.Ks, sc["Es"], sc["depth_ranges"], sc["pairs"], nviews, ndepths, kind_dr, short_sources)


def infer_scan_folder(model, datapath, scan, nviews=5, interval_scale=1.06, ndepths=192, dataset="general", short_sources=None,
                      **kw):
    """``infer_scan`` on a scan folder in the reference's layout (``general_eval4.MVSDataset``).  The result's
    ``ref_views`` / ``pairs`` index ``view_ids`` (the file numbers).  ``max_h`` / ``max_w`` (the loader's arguments) go
    through to ``infer_scan``: a scan is taken at its native image size, as the dataset ships it.

    ``dataset="tanks"``: a Tanks and Temples scan folder (``datapath`` includes the split) as ``datasets/tanks.py`` takes it --
    ``crop_rows=(28, 28)`` and ``depth_range_kind="min_max"`` unless given; the loader's default of 7 views is the caller's
    ``nviews=7``.  ``dataset="eth3d"``: ``datasets/eth3d.py`` -- ``cams_1/``, ``img_wh=(1920, 1280)`` unless given,
    ``depth_range_kind="min_max"``.  ``short_sources="fewer_views"`` (through to ``infer_scan``) runs a reference view whose
    pair list is shorter than ``nviews - 1`` with the sources it has, as both loaders do."""
    sc = read_scan_folder(datapath, scan, interval_scale, ndepths, dataset)
    kw = _dataset_keywords(dataset, kw)
    res = infer_scan(model, sc["images"], sc["Ks"], sc["Es"], sc["depth_ranges"], sc["pairs"], nviews=nviews,
                     ndepths=ndepths, view_ids=sc["view_ids"], short_sources=short_sources, **kw)
    res.setdefault("images", sc["images"])                                  # (the resized ones where infer_scan scaled)
    return res


def _images_u8_hwc(images):
    """The scan's images as uint8 [V,H,W,3] on the host (float 0..1 inputs: clip(x * 255) truncated, test_mvs4.py:262-264)."""
    kind, images, _ = _check_images(images)
    if torch.is_tensor(images):
        images = images.detach().cpu().numpy()
    if kind == "u8":
        return images
    return np.clip(np.transpose(images, (0, 2, 3, 1)) * 255, 0, 255).astype(np.uint8)


def write_scan_outputs(result, images, out_folder):
    """The reference's per-scan output layout (test_mvs4.py:213-264): ``depth_est/%08d.pfm``, ``confidence/%08d.pfm``,
    ``cams/%08d_cam.txt`` (stage-4 camera), ``images/%08d.jpg`` for every reference view, numbered by
    ``result['view_ids']`` -- what ``fusion.filter_depth(pair_folder, out_folder, out_folder, ply)`` reads.  The two map
    stacks leave the device through ONE pinned staging copy."""
    from PIL import Image
    depth, conf = result["depth"], result["photometric_confidence"]
    maps, names = getattr(result, "maps", None), getattr(result, "map_names", ())
    if maps is not None and "depth" in names and "photometric_confidence" in names:
        # (infer_scan keeps same-shaped stacks in one allocation: the whole of it in one copy)
        stage = torch.empty(maps.shape, dtype=torch.float32).pin_memory()
        stage.copy_(maps, non_blocking=True)
        torch.cuda.current_stream(maps.device).synchronize()
        depth_h, conf_h = stage[names.index("depth")].numpy(), stage[names.index("photometric_confidence")].numpy()
    else:
        stage = torch.empty((2,) + tuple(depth.shape), dtype=torch.float32).pin_memory()
        torch._foreach_copy_([stage[0], stage[1]], [depth, conf])
        torch.cuda.current_stream(depth.device).synchronize()
        depth_h, conf_h = stage[0].numpy(), stage[1].numpy()
    imgs = _images_u8_hwc(images)
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(out_folder, sub), exist_ok=True)
    ids = result["view_ids"]
    for i, r in enumerate(result["ref_views"]):
        name = "{:0>8}".format(ids[int(r)])
        formats.save_pfm(os.path.join(out_folder, "depth_est", name + ".pfm"), np.ascontiguousarray(depth_h[i]))
        formats.save_pfm(os.path.join(out_folder, "confidence", name + ".pfm"), np.ascontiguousarray(conf_h[i]))
        cam = np.zeros((2, 4, 4), dtype=np.float32)
        cam[0] = result["Es"][int(r)]
        cam[1, :3, :3] = result["Ks"][int(r)]
        formats.write_cam(os.path.join(out_folder, "cams", name + "_cam.txt"), cam)
        Image.fromarray(imgs[int(r)]).save(os.path.join(out_folder, "images", name + ".jpg"))


def reconstruct_scan(model, images, Ks, Es, depth_ranges, pairs, conf=0.9, thres_view=5, plyfilename=None, short_sources=None,
                     fusion="normal", pix_base=None, rel_base=None, voxel_size=None, voxel_reduce="mean", outliers=None, normals=None,
                     mesh=None, meshfilename=None, mesh_clean=None, **kw):
    """``infer_scan`` followed by ``fusion.fuse_scene`` on the device tensors: the reference's ``save_scene_depth`` +
    ``filter_depth`` (test_mvs4.py:170-268, :331-421) without leaving the GPU.  -> the ``fusion.SceneResult`` (with the
    ``ScanResult`` as its ``scan`` attribute); writes the point cloud to ``plyfilename`` if given.

    Every source view a reference view's pair lists must have a depth map of its own, i.e. be a reference view with
    sources itself (the reference's ``filter_depth`` reads its ``depth_est`` file).  Colours come from the INPUT images
    (with ``max_h`` / ``max_w``, ``crop_rows`` or ``img_wh``: from the prepared ones, the pixels the reference writes to
    ``images/``), not from the
    re-encoded JPEGs the reference reads back from its output folder: positions and masks are the same, colours differ
    by the JPEG re-encoding the reference adds.  ``short_sources``: as ``infer_scan`` (fusion takes the pair lists as they
    are, whatever their lengths).  ``fusion``: ``"normal"`` (the reference's fixed thresholds) or ``"dynamic"`` (dynamic
    consistency checking with ``pix_base`` / ``rel_base``, ``fuse_scene``'s ``method``); none of the three reaches
    ``infer_scan``.  ``voxel_size`` / ``voxel_reduce``: as ``fuse_scene`` (named keywords, they do not reach ``infer_scan``
    either); with a ``voxel_size`` the result also holds the ``thin_*`` cloud and that is the one written to ``plyfilename``.
    ``outliers`` / ``normals``: as ``fuse_scene`` (outlier removal and normals on the cloud that would be written); the
    result then holds the ``final_*`` cloud, and that is the one written, with its normals.  ``mesh`` (a
    ``fusion.TSDFMesh``): as ``fuse_scene`` (TSDF integration of the filtered maps and marching tetrahedra; the result then
    holds the ``mesh_*`` keys); ``meshfilename``: the triangle mesh is written there (only with ``mesh``); ``mesh_clean`` (a
    ``fusion.MeshClean``, only with ``mesh``): as ``fuse_scene`` (the ``mesh_*`` keys and the file hold the cleaned mesh, with its
    normals where asked for).  None of them reaches ``infer_scan``; with the default None nothing changes."""
    from . import fusion as fusion_mod
    from . import mesh as mesh_mod
    fusion_mod._check_method("reconstruct_scan", fusion)
    fusion_mod._check_voxel("reconstruct_scan", voxel_size, voxel_reduce)
    fusion_mod._check_clean("reconstruct_scan", outliers, normals)
    mesh_mod.check_mesh_spec("reconstruct_scan", mesh)
    mesh_mod.check_clean_spec("reconstruct_scan", mesh_clean, mesh)
    if meshfilename is not None and mesh is None:
        raise RuntimeError("reconstruct_scan: meshfilename needs mesh= (a TSDFMesh)")
    bases = {k: v for k, v in (("pix_base", pix_base), ("rel_base", rel_base)) if v is not None}
    inp = plan_inputs(images, Ks, kw.get("max_h"), kw.get("max_w"), kw.get("crop_rows"), kw.get("img_wh"), Es)
    scan = infer_scan(model, inp.images, Ks, Es, depth_ranges, pairs, short_sources=short_sources, **kw)
    # (prepared: uint8 [V,Hd,Wd,3], already on the device; otherwise the input stack, which has the target size)
    kind, images = ("u8", scan["images"]) if inp.prepare else (inp.kind, inp.images)
    slot = {int(r): i for i, r in enumerate(scan["ref_views"])}
    fpairs = []
    for r, srcs in scan["pairs"]:
        for v in srcs:
            if v not in slot:
                raise RuntimeError("reconstruct_scan: reference view %d lists source view %d, which has no depth map (it "
                                   "is not a reference view with sources in pairs)" % (r, v))
        fpairs.append((slot[r], [slot[v] for v in srcs]))
    dev = scan["depth"].device
    idx = torch.from_numpy(np.asarray(scan["ref_views"])).to(dev)
    img = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
    img = img.to(dev)[idx]
    if kind == "f32":
        img = img.permute(0, 2, 3, 1).contiguous()
    refs = np.asarray(scan["ref_views"])
    res = fusion_mod.fuse_scene(scan["depth"], scan["photometric_confidence"], img, scan["Ks"][refs], scan["Es"][refs], fpairs,
                                conf, thres_view, device=dev, method=fusion, voxel_size=voxel_size,
                                voxel_reduce=voxel_reduce, outliers=outliers, normals=normals, mesh=mesh, mesh_clean=mesh_clean, **bases)
    res.scan = scan
    if plyfilename is not None:
        fusion_mod.write_scene_ply(plyfilename, res, thinned=voxel_size is not None)
    if meshfilename is not None:
        mesh_mod.write_result_mesh(meshfilename, res)
    return res
