"""The validation pass without a GPU: the new symbols' argument checks, the names and the text of mvster_amd/validate.py,
the arithmetic of Validator.mean against DictAverageMeter (utils.py:103-122) on one process and over two gloo ranks, and
the host restatement of the depth metrics that tests/test_gpu_validate.py holds the kernel to."""
import ctypes
import io
import math
import os
import re
import socket
import tokenize

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import validate_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


def test_new_symbols_check_their_arguments_without_a_gpu(lib):
    """ERR_NULL / ERR_SHAPE come back before any launch; the device pointers are stand-in addresses nothing dereferences."""
    from mvster_amd import _lib
    p = 1 << 32
    thres = (ctypes.c_float * 9)(2, 4, 8, 16, 32, 64, 128, 256, 512)
    th = ctypes.cast(thres, ctypes.c_void_p)

    def dm(est=p, gt=p, mask=p, scale=None, thres=th, K=3, N=2, HW=64, partial=p, raw=p, out=p):
        return lib.mvster_depth_metrics(est, gt, mask, scale, thres, K, N, HW, partial, raw, out, None)
    for name in ("est", "gt", "mask", "thres", "partial", "raw", "out"):
        assert dm(**{name: None}) == _lib.ERR_NULL, name
    assert dm(K=0) == _lib.ERR_SHAPE
    assert dm(K=9) == _lib.ERR_SHAPE
    assert dm(K=-1) == _lib.ERR_SHAPE
    assert dm(N=0) == _lib.ERR_SHAPE
    assert dm(N=-3) == _lib.ERR_SHAPE
    assert dm(HW=0) == _lib.ERR_SHAPE
    assert dm(HW=-1) == _lib.ERR_SHAPE
    assert lib.mvster_scalar_accumulate(None, 17, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_scalar_accumulate(p, 17, None, p, None) == _lib.ERR_NULL
    assert lib.mvster_scalar_accumulate(p, 17, p, None, None) == _lib.ERR_NULL
    assert lib.mvster_scalar_accumulate(p, 0, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_scalar_accumulate(p, -1, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_scalar_reset(None, 17, p, None) == _lib.ERR_NULL
    assert lib.mvster_scalar_reset(p, 17, None, None) == _lib.ERR_NULL
    assert lib.mvster_scalar_reset(p, 0, p, None) == _lib.ERR_SHAPE


def test_slot_counts(lib):
    """Workgroups per image: one per 2048 pixels, between 1 and 256 (the scratch the Python wrapper allocates)."""
    f = lib.mvster_depth_metrics_slots
    assert [f(n) for n in (0, 1, 2048, 2049, 64 * 80, 129 * 161, 512 * 640, 1 << 30)] == [1, 1, 1, 2, 3, 11, 160, 256]


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from mvster_amd import ops
    x = torch.zeros(2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_metrics(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scalar_accumulate(torch.zeros(17), torch.zeros(17, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scalar_reset(torch.zeros(17, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))


def test_scalar_names():
    from mvster_amd import SCALAR_NAMES, validate
    want = ["loss", "s0_d_loss", "s1_d_loss", "s2_d_loss", "s3_d_loss", "s0_c_loss", "s1_c_loss", "s2_c_loss", "s3_c_loss",
            "s0_range_err_ratio", "s1_range_err_ratio", "s2_range_err_ratio", "s3_range_err_ratio", "abs_depth_error",
            "thres2mm_error", "thres4mm_error", "thres8mm_error"]
    assert list(SCALAR_NAMES) == want and len(want) == 17
    assert validate.SCALAR_NAMES is SCALAR_NAMES


def test_band_of_abs_depth_error_is_refused():
    from mvster_amd import AbsDepthError_metrics
    x = torch.zeros(1, 2, 2)
    with pytest.raises(NotImplementedError, match="band"):
        AbsDepthError_metrics(x, x, x > 0, thres=(0.0, 1.0))


def _code_of(path):
    """The file's tokens without comments and strings (docstrings included)."""
    out = []
    for tok in tokenize.generate_tokens(io.StringIO(open(path).read()).readline):
        if tok.type not in (tokenize.COMMENT, tokenize.STRING, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT):
            out.append(tok.string)
    return " ".join(out)


def test_module_has_no_checker_import_and_no_boolean_mask_gather():
    """mvster_amd/validate.py imports nothing of the CPU checkers and indexes no tensor with a mask (``x[mask]``, ``x[e > t]``:
    a device synchronisation each), nor uses the other gathers of data-dependent size or a scalar read-back per batch."""
    code = _code_of(os.path.join(ROOT, "mvster_amd", "validate.py"))
    assert "oracle" not in code
    # an index that is a mask-named value or a comparison
    assert not re.search(r"\[\s*[\w .]*mask\w*\s*(?:[<>=!]=?[^\]]*)?\]", code), "boolean-mask indexing"
    assert not re.search(r"\[[^\]\[]*(?:<|>|==|!=)[^\]\[]*\]", code), "indexing with a comparison"
    for word in ("masked_select", "nonzero", "item", "cpu", "numpy"):
        assert not re.search(r"\. %s \(" % re.escape(word), code), word
    # the regular expressions do see what they are for
    assert re.search(r"\[\s*[\w .]*mask\w*\s*(?:[<>=!]=?[^\]]*)?\]", "depth_est [ mask ]")
    assert re.search(r"\[\s*[\w .]*mask\w*\s*(?:[<>=!]=?[^\]]*)?\]", "d [ mask > 0.5 ]")
    assert re.search(r"\[[^\]\[]*(?:<|>|==|!=)[^\]\[]*\]", "e [ e > 2 ]")


def _rows(seed=0, n=5):
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(17, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(n)]
    rows[2][5] = float("nan")
    return rows


def _sums_of(rows):
    """What mvster_scalar_accumulate leaves: fp64 sums of the fp32 rows in row order, and their number."""
    sums = torch.zeros(17, dtype=torch.float64)
    for r in rows:
        sums += r.to(torch.float64)
    return sums, torch.tensor([len(rows)], dtype=torch.int64)


def test_mean_equals_dict_average_meter_on_one_process():
    from mvster_amd.validate import SCALAR_NAMES, reduce_scalar_sums
    rows = _rows()
    got = reduce_scalar_sums(*_sums_of(rows))
    want = VC.meter_mean([r.tolist() for r in rows])
    assert list(got.keys()) == list(SCALAR_NAMES)
    for k, w in zip(SCALAR_NAMES, want):
        assert isinstance(got[k], float) and VC.same_float(got[k], w), (k, got[k], w)
    assert math.isnan(got[SCALAR_NAMES[5]]) and sum(math.isnan(v) for v in got.values()) == 1
    with pytest.raises(RuntimeError, match="names"):
        reduce_scalar_sums(torch.zeros(3, dtype=torch.float64), torch.ones(1, dtype=torch.int64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mean_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from mvster_amd import shard
    from mvster_amd.validate import reduce_scalar_sums
    shard.init_distributed(backend="gloo")
    sums, count = _sums_of(_rows(seed=10 + rank, n=3 + rank))            # (unequal counts: the quotient of the two sums)
    before = sums.clone()
    got = reduce_scalar_sums(sums, count)
    q.put((rank, got, bool(torch.equal(before.nan_to_num(7.0), sums.nan_to_num(7.0)))))
    dist.destroy_process_group()


def test_mean_over_two_gloo_ranks_is_the_quotient_of_the_summed_vectors():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mean_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    from mvster_amd.validate import SCALAR_NAMES
    parts = [_sums_of(_rows(seed=10 + r, n=3 + r)) for r in range(2)]
    total = parts[0][0] + parts[1][0]                                      # (two addends: no order to choose)
    n = float(parts[0][1].item() + parts[1][1].item())
    for rank, got, untouched in res:
        assert untouched                                                   # the running sums themselves are not reduced in place
        for i, k in enumerate(SCALAR_NAMES):
            assert VC.same_float(got[k], total[i].item() / n), (rank, k)


def test_restatement_gives_nan_for_an_empty_mask():
    est = np.array([[[1.0, 2.0]], [[3.0, 5.0]]], np.float32)
    gt = np.array([[[1.5, 2.0]], [[3.0, 9.0]]], np.float32)
    mask = np.array([[[1.0, 1.0]], [[0.0, 0.0]]], np.float32)
    out, raw = VC.metrics_ref(est, gt, mask)
    assert raw.tolist() == [[2.0, 0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]]
    assert np.isnan(out).all()                        # one image without a valid pixel: the batch's mean is NaN
    out1, _ = VC.metrics_ref(est[:1], gt[:1], mask[:1])
    assert out1.tolist() == [0.25, 0.0, 0.0, 0.0]


def test_restatement_on_a_hand_computed_example():
    """2 x 3, five valid pixels with errors 0, 2, 3, 4.5, 9 (one exactly on a threshold: strict >) and one dropped pixel."""
    gt = np.full((1, 2, 3), 10.0, np.float32)
    est = np.array([[[10.0, 12.0, 13.0], [14.5, 19.0, 100.0]]], np.float32)
    mask = np.array([[[1.0, 1.0, 1.0], [1.0, 1.0, 0.0]]], np.float32)
    out, raw = VC.metrics_ref(est, gt, mask)
    assert raw.tolist() == [[5.0, 18.5, 3.0, 2.0, 1.0]]
    assert out.dtype == np.float32
    assert out.tolist() == [float(np.float32(3.7)), float(np.float32(0.6)), float(np.float32(0.4)), float(np.float32(0.2))]
    # a scale: every product rounded to fp32 before the difference
    s = np.array([0.3], np.float32)
    _, raw_s = VC.metrics_ref(est, gt, mask, scale=s)
    e = [abs(np.float32(np.float32(a) * s[0]) - np.float32(np.float32(10.0) * s[0])) for a in (10.0, 12.0, 13.0, 14.5, 19.0)]
    assert raw_s[0, 0] == 5.0 and raw_s[0, 1] == float(sum(np.float64(v) for v in e))
    # two images: the fp32 mean in image order
    est2, gt2, mask2 = np.concatenate([est, gt]), np.concatenate([gt, gt]), np.concatenate([mask, mask])
    out2, _ = VC.metrics_ref(est2, gt2, mask2)
    assert out2.tolist() == [float(np.float32(np.float32(3.7) / np.float32(2))), float(np.float32(0.3)), float(np.float32(0.2)),
                             float(np.float32(0.1))]


def test_cases_hold_what_the_gpu_test_needs():
    names = [c[0] for c in VC.cases()]
    assert len(names) == len(set(names)) == 30
    est, gt, mask, scale = VC.make_case((2, 129, 161), "80", "valid_too")
    assert 0.75 < mask.mean() < 0.85 and np.isnan(est[0][mask[0] > 0.5]).any() and np.isinf(est[1][mask[1] > 0.5]).any()
    e = VC.errors(est[1], gt[1], mask[1] > 0.5)
    assert all((e == t).any() for t in (2.0, 4.0, 8.0)) and (est < 0).any() and np.isnan(est[mask <= 0.5]).any()
    _, raw = VC.metrics_ref(est, gt, mask)
    assert np.isnan(raw[0, 1]) and np.isinf(raw[1, 1]) and raw[1, 2] >= raw[1, 3] >= raw[1, 4] >= 1
    assert VC.make_case((3, 7, 13), "one_empty", "invalid_only")[2][2].sum() == 0
