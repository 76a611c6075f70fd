"""Shared by tests/test_train_summary_cpu.py and tests/test_gpu_train_summary.py: the host restatement of Blend_loss's pooled
error figures (MVS4Net.py:202-205) in plain numpy and the inputs the GPU kernel is checked on."""
import numpy as np

from tests import validate_cases as VC

THRESHOLDS = (3, 1)
MASKS = VC.MASKS + ["all_empty"]
POW2_SCALES = (1.0, 0.5, 0.25)


def pooled_raw_ref(est, gt, mask, thresholds=THRESHOLDS, scale=None):
    """-> raw [N, 2+K] float64 per image: valid pixels, fp64 sum of the fp32 errors (``validate_cases.errors``), errors at or
    below every threshold -- counted as such: a NaN error is neither above nor at-or-below."""
    N = est.shape[0]
    raw = np.zeros((N, 2 + len(thresholds)), np.float64)
    for n in range(N):
        e = VC.errors(est[n], gt[n], mask[n] > 0.5, None if scale is None else scale[n])
        raw[n, 0] = e.size
        with np.errstate(invalid="ignore"):
            raw[n, 1] = np.sum(e.astype(np.float64))
            for k, t in enumerate(thresholds):
                raw[n, 2 + k] = np.count_nonzero(e <= np.float32(t))
    return raw


def pooled_out_from_raw(raw):
    """raw [N, 2+K] -> out [1+K] float32: the columns summed over the images in image order in fp64; epe =
    float32(sum_e / count), err_k = float32(float32(le_k / count) * float32(100)); 0 / 0 = NaN for a batch without a valid
    pixel."""
    N, cols = raw.shape
    out = np.zeros(cols - 1, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(cols - 1):
            count, x = np.float64(0), np.float64(0)
            for n in range(N):
                count = count + np.float64(raw[n, 0])
                x = x + np.float64(raw[n, 1 + j])
            q = np.float32(x / count)
            out[j] = q if j == 0 else np.float32(q * np.float32(100))
    return out


def pooled_ref(est, gt, mask, thresholds=THRESHOLDS, scale=None):
    raw = pooled_raw_ref(est, gt, mask, thresholds, scale)
    return pooled_out_from_raw(raw), raw


def make_case(shape, mask_kind, special, scale_kind="random", seed=0):
    """``validate_cases.make_case`` (errors planted on 2 / 4 / 8, negatives, NaN / inf at dropped or also at kept pixels)
    with ``all_empty`` masks in addition and, for ``scale_kind="pow2"``, the scales 1, 0.5, 0.25 (image n: the n-th, in
    turn) and estimates planted at gt +- 3 / s and gt +- 1 / s (exact: gt is an integer below 2^20), so that the scaled
    errors lie exactly on the thresholds 3 and 1.  The planted pixels are made valid unless the image is to be empty."""
    est, gt, mask, scale = VC.make_case(shape, "80" if mask_kind == "all_empty" else mask_kind, special, seed)
    N, H, W = shape
    if mask_kind == "all_empty":
        mask[:] = 0.0
    if scale_kind == "none":
        scale = None
    elif scale_kind == "pow2":
        scale = np.array([POW2_SCALES[n % 3] for n in range(N)], np.float32)
        rng = np.random.default_rng(seed + 7 + 1000 * N + 10 * H + W)
        fe, fg, fm = est.reshape(N, -1), gt.reshape(N, -1), mask.reshape(N, -1)
        for n in range(N):
            idx = rng.permutation(H * W)[:4]
            empty = not (fm[n] > 0.5).any()
            for i, d in zip(idx, (3.0, 1.0, -3.0, -1.0)):
                fe[n, i] = fg[n, i] + np.float32(d) / scale[n]
                if not empty:
                    fm[n, i] = 1.0
    return est, gt, mask, scale


def cases():
    for shape in VC.SHAPES:
        for mask_kind in MASKS:
            for special in VC.SPECIALS:
                yield "%dx%dx%d-%s-%s" % (shape + (mask_kind, special)), shape, mask_kind, special


def same_f32(a, b):
    """Bit-equal float32 arrays; NaN matches NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))))


def same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))
