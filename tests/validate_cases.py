"""Shared by tests/test_validate_cpu.py and tests/test_gpu_validate.py: the host restatement of the depth metrics
(utils.py:125-159 under compute_metrics_for_each_image) in plain numpy, the inputs the GPU kernel is checked on, and the
Python-float form of DictAverageMeter (utils.py:103-122)."""
import math
import struct

import numpy as np

THRESHOLDS = (2, 4, 8)
SHAPES = [(1, 1, 1), (3, 7, 13), (2, 64, 80), (2, 129, 161), (5, 8, 8)]        # N, H, W
MASKS = ["80", "all", "one_empty"]
SPECIALS = ["invalid_only", "valid_too"]


def errors(est, gt, valid, scale=None):
    """fp32 |est - gt| (or |est*s - gt*s|, every operation rounded to fp32 on its own) at the valid pixels of one image."""
    a, b = est[valid].astype(np.float32), gt[valid].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if scale is not None:
            s = np.float32(scale)
            a, b = (a * s).astype(np.float32), (b * s).astype(np.float32)
        return np.abs((a - b).astype(np.float32))


def raw_ref(est, gt, mask, thresholds=THRESHOLDS, scale=None):
    """-> raw [N, 2+K] float64 per image: valid pixels, fp64 sum of the fp32 errors, errors strictly above every threshold."""
    N = est.shape[0]
    raw = np.zeros((N, 2 + len(thresholds)), np.float64)
    for n in range(N):
        e = errors(est[n], gt[n], mask[n] > 0.5, None if scale is None else scale[n])
        raw[n, 0] = e.size
        with np.errstate(invalid="ignore"):
            raw[n, 1] = np.sum(e.astype(np.float64))
            for k, t in enumerate(thresholds):
                raw[n, 2 + k] = np.count_nonzero(e > np.float32(t))
    return raw


def out_from_raw(raw):
    """raw [N, 2+K] -> out [1+K] float32: per image float32(float64(x) / float64(count)) -- 0 / 0 = NaN for an image
    without a valid pixel, like torch.mean of an empty tensor -- then the fp32 mean over the images in image order."""
    N, cols = raw.shape
    out = np.zeros(cols - 1, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(cols - 1):
            acc = np.float32(0)
            for n in range(N):
                acc = np.float32(acc + np.float32(np.float64(raw[n, 1 + j]) / np.float64(raw[n, 0])))
            out[j] = np.float32(acc / np.float32(N))
    return out


def metrics_ref(est, gt, mask, thresholds=THRESHOLDS, scale=None):
    raw = raw_ref(est, gt, mask, thresholds, scale)
    return out_from_raw(raw), raw


def make_case(shape, mask_kind, special, seed=0):
    """est, gt, mask [N,H,W] float32, scale [N] float32.  gt: integers below 2^20, so that the planted errors of exactly 2, 4
    and 8 are exact; est: gt + noise of a few units, negatives, the planted errors, and NaN / +inf at pixels the mask drops
    (``invalid_only``) or also at pixels it keeps (``valid_too``: NaN in image 0, +inf in the last image)."""
    N, H, W = shape
    rng = np.random.default_rng(seed + 1000 * N + 10 * H + W)
    gt = rng.integers(400, 900, size=shape).astype(np.float32)
    est = (gt + rng.normal(0.0, 4.0, size=shape)).astype(np.float32)
    if mask_kind == "all":
        mask = np.ones(shape, np.float32)
    else:
        mask = (rng.random(shape) > 0.2).astype(np.float32)
        if mask_kind == "one_empty":
            mask[N - 1] = 0.0
    flat_e, flat_g, flat_m = est.reshape(N, -1), gt.reshape(N, -1), mask.reshape(N, -1)
    HW = H * W
    for n in range(N):
        idx = rng.permutation(HW)
        for i, d in zip(idx[:6], (2.0, 4.0, 8.0, -2.0, -4.0, -8.0)):           # errors exactly on the thresholds
            flat_e[n, i] = flat_g[n, i] + np.float32(d)
        for i in idx[6:9]:
            flat_e[n, i] = -flat_e[n, i]                                        # negative estimates
        bad = np.flatnonzero(flat_m[n] <= 0.5)
        for i, v in zip(bad[:3], (np.nan, np.inf, -np.inf)):
            flat_e[n, i] = v
    if special == "valid_too":
        good0, goodl = np.flatnonzero(flat_m[0] > 0.5), np.flatnonzero(flat_m[N - 1] > 0.5)
        if good0.size:
            flat_e[0, good0[good0.size // 2]] = np.nan
        if goodl.size > 1:
            flat_e[N - 1, goodl[0]] = np.inf
    scale = (128.0 / rng.uniform(300.0, 900.0, size=N)).astype(np.float32)
    return est, gt, mask, scale


def cases():
    for shape in SHAPES:
        for mask_kind in MASKS:
            for special in SPECIALS:
                yield "%dx%dx%d-%s-%s" % (shape + (mask_kind, special)), shape, mask_kind, special


def bits(x):
    return struct.pack("<d", float(x))


def same_float(a, b):
    """Bit-equal doubles; any NaN equals any NaN."""
    return (math.isnan(a) and math.isnan(b)) or bits(a) == bits(b)


def meter_mean(rows):
    """DictAverageMeter over rows of fp32 values written out: Python-float (double) sums in row order, divided by the count."""
    data = None
    for r in rows:
        vals = [float(v) for v in r]
        data = vals if data is None else [a + b for a, b in zip(data, vals)]
    return [v / len(rows) for v in data]
