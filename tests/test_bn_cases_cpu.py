"""tests/bn_cases.py checked without a GPU: its float64 reference against torch's own BatchNorm in float64, its restatement of
the launch arithmetic against the library's host functions, and every case against the path its row of the table claims."""
import pytest
import torch

from tests import bn_cases as B

TRAIN = [c for c in B.CASES if c.kind == "train"]
FROZEN = [c for c in B.CASES if c.kind == "frozen"]


def _close(got, want, what):
    scale = max(want.abs().max().item(), 1e-300)
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * scale, (what, err / scale)


@pytest.mark.parametrize("c", [c for c in TRAIN if c.flavor != "nonfinite"], ids=lambda c: c.name)
def test_training_reference_agrees_with_torch_float64(c):
    """``groups`` sequential calls of ``torch.nn.BatchNorm3d(...).double()`` in training mode, ReLU and the skip addition
    outside, under autograd: y, the running statistics, the counter and the three gradients to 1e-12 of the tensor's maximum.
    (One row per group is refused by the module -- those cases are held to the formulas alone; a non-finite input has no
    maximum to be relative to.)  The pack is checked against its definition from torch's var_mean."""
    inp, ref = B.reference(c)
    if c.rows == 1:
        assert ref.pack[1].abs().max() == 0 and torch.equal(ref.pack[0], inp["x"].double().reshape(c.groups, c.C))
        want_rv = inp["running_var"].double() * (1 - c.momentum) ** c.groups           # unbias guard: var * 1 = 0
        _close(ref.running_var, want_rv, "running_var")
        assert ref.dx.abs().max() <= 1e-12
        return
    m = torch.nn.BatchNorm3d(c.C, eps=c.eps, momentum=c.momentum).double().train()
    with torch.no_grad():
        m.weight.copy_(inp["weight"])
        m.bias.copy_(inp["bias"])
        m.running_mean.copy_(inp["running_mean"])
        m.running_var.copy_(inp["running_var"])
    x = inp["x"].double().reshape(c.groups, c.rows, c.C).requires_grad_(True)
    y = torch.stack([m(x[g].reshape(c.rows, c.C, 1, 1, 1)).reshape(c.rows, c.C) for g in range(c.groups)])
    y = torch.relu(y) if c.relu else y
    y.backward(inp["gy"].double().reshape(y.shape))
    if c.skip:
        y = y + inp["skip"].double().reshape(y.shape)
    _close(ref.y, y.detach().reshape(ref.y.shape), "y")
    _close(ref.running_mean, m.running_mean, "running_mean")
    _close(ref.running_var, m.running_var, "running_var")
    assert int(m.num_batches_tracked) == c.groups
    _close(ref.dx, x.grad.reshape(ref.dx.shape), "dx")
    _close(ref.dgamma, m.weight.grad, "dgamma")
    _close(ref.dbeta, m.bias.grad, "dbeta")
    var, mean = torch.var_mean(x.detach(), 1, unbiased=False)
    _close(ref.pack[0], mean, "mean")
    if c.flavor != "const":                 # (a constant channel: exactly 0 here, 1e-32 from var_mean)
        _close(ref.pack[1], var, "var")
    _close(ref.pack[2], (var + c.eps).rsqrt(), "rstd")
    _close(ref.pack[3], m.weight.detach() * (var + c.eps).rsqrt(), "scale")
    assert int(ref.boundary.sum()) <= B.MAX_BOUNDARY


@pytest.mark.parametrize("c", [c for c in TRAIN if c.flavor == "nonfinite"], ids=lambda c: c.name)
def test_non_finite_reference_is_clean_outside_its_channel(c):
    """The reference of the non-finite cases is finite in every channel but the poisoned one, and equals there what the same
    input with the channel replaced gives: the channels are independent in the reference, as they must be in the kernels."""
    inp, ref = B.reference(c)
    clean = [ch for ch in range(c.C) if ch != B.POISONED_CHANNEL]
    x2 = inp["x"].clone()
    x2[:, B.POISONED_CHANNEL] = 0.25
    ref2 = B.ref_train(x2, inp["gy"], inp["weight"], inp["bias"], inp["running_mean"], inp["running_var"], c.eps, c.momentum,
                       c.relu, c.groups, inp["skip"])
    for name in ("y", "pack", "running_mean", "running_var", "dx", "dgamma", "dbeta"):
        a, b = getattr(ref, name)[..., clean], getattr(ref2, name)[..., clean]
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    assert not torch.isfinite(ref.pack[..., B.POISONED_CHANNEL]).any()
    assert int(ref.boundary[..., clean].sum()) <= B.MAX_BOUNDARY


@pytest.mark.parametrize("c", FROZEN, ids=lambda c: c.name)
def test_frozen_reference_agrees_with_torch_float64(c):
    """torch's eval-mode batch norm in float64 with the group's constants as running statistics (weight = scale / rstd, bias =
    shift + mean * scale, variance 1 / rstd^2 at eps 1e-300), one call per group, under autograd: y, dx, and the gradients of weight
    and bias summed over the groups, which are sum g * xh and sum g."""
    inp, ref = B.reference(c)
    mean, rstd, scale, shift = (t.double() for t in inp["frozen"])
    x = inp["x"].double().reshape(c.groups, c.rows, c.C).requires_grad_(True)
    w = (scale / rstd).requires_grad_(True)
    b = (shift + mean * scale).requires_grad_(True)
    y = torch.stack([torch.nn.functional.batch_norm(x[g].reshape(c.rows, c.C, 1, 1, 1), mean[g].clone(), 1 / rstd[g] ** 2, w[g], b[g],
                                                    False, 0.0, 1e-300).reshape(c.rows, c.C) for g in range(c.groups)])
    y = torch.relu(y) if c.relu else y
    y.backward(inp["gy"].double().reshape(y.shape))
    if c.skip:
        y = y + inp["skip"].double().reshape(y.shape)
    _close(ref.y, y.detach().reshape(ref.y.shape), "y")
    _close(ref.dx, x.grad.reshape(ref.dx.shape), "dx")
    _close(ref.dgamma, w.grad.sum(0), "dgamma")
    _close(ref.dbeta, b.grad.sum(0), "dbeta")
    assert int(ref.boundary.sum()) <= B.MAX_BOUNDARY


def test_column_sum_reference():
    x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    assert torch.equal(B.ref_col_sum(x), torch.tensor([60.0, 66.0, 72.0, 78.0], dtype=B.D))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    return _lib.load()


def test_slot_functions_equal_the_library(lib):
    """``slots_for`` / ``train_slots_for`` against mvster_bn_slots / mvster_bn_train_slots (host functions) at every case of
    the table and on a sweep across each cap."""
    shapes = {(c.rows, c.C, c.groups) for c in B.CASES if c.kind != "refused"}
    for C in (4, 8, 16, 32, 64):
        q = C // 4
        for groups in (1, 2, 3, 5, 9, 16, 17, 100, 171, 255, 256, 257, 511, 512, 600):
            for n4 in (1, 1023, 1024, 4096, 4097, 8192, 8193, 51 * 4096, 51 * 4096 + 1, 64 * 4096, 64 * 4096 + 1, 128 * 4096 + 1,
                       256 * 4096, 256 * 4096 + 1, 1 << 24):
                shapes.add((max(1, n4 // q), C, groups))
    for rows, C, groups in sorted(shapes):
        assert lib.mvster_bn_slots(rows, C, groups) == B.slots_for(rows, C, groups), (rows, C, groups)
        assert lib.mvster_bn_train_slots(rows, C, groups) == B.train_slots_for(rows, C, groups), (rows, C, groups)
        assert B.train_slots_for(rows, C, groups) <= B.train_apply_blocks(rows, C, groups)
    assert lib.mvster_bn_slots(8, 12, 1) == 0 and lib.mvster_bn_train_slots(8, 128, 1) == 0 and lib.mvster_bn_slots(0, 8, 1) == 0


def test_sum_slots_lane_arithmetic():
    """The examples the comments of bn_ops.hip give: 8 lanes x 16 loads per column at 64 channels, so 128 slots in one round
    and 129 in two; 2048 pairs take two full ``base`` rounds, 1152 a ragged second one."""
    assert B.sum_slots_rounds(128, 1, 64) == [(128, 8, 1)]
    assert B.sum_slots_rounds(129, 1, 64) == [(128, 8, 2)]
    assert B.sum_slots_rounds(256, 1, 32) == [(64, 16, 1)]
    assert B.sum_slots_rounds(1, 16, 64) == [(1024, 1, 1), (1024, 1, 1)]
    assert B.sum_slots_rounds(1, 9, 64) == [(1024, 1, 1), (128, 8, 1)]
    assert B.sum_slots_rounds(1, 17, 32) == [(1024, 1, 1), (64, 16, 1)]
    assert B.col_sum_loop(4096, 1) == (True, False, False) and B.col_sum_loop(3, 1) == (False, True, False)
    assert B.col_sum_loop(6146, 2) == (True, True, True) and B.col_sum_loop(8192, 2) == (True, False, False)


def test_every_case_reaches_the_path_it_claims():
    """The facts a case carries (slots, apply blocks, rounds of the ``base`` loop, rounds of the inner ``n`` loop, whether the
    two-row loop of col_sum and its tail run) equal the restatement, its paths are exactly the ones the restatement derives,
    and every path the table was built for is claimed by at least one case."""
    reached = {}
    for c in B.CASES:
        assert c.rows * c.groups * c.C * 4 <= 23 << 20, c.name               # about 20 MB at the most
        assert B.paths_of(c.kind, c.rows, c.C, c.groups) == set(c.paths), c.name
        if c.kind != "refused":
            assert B.facts(c.kind, c.rows, c.C, c.groups) == c.claims, c.name
            assert c.groups * 2 * c.C <= B.MAX_PAIRS
        for p in c.paths:
            reached.setdefault(p, []).append(c.name)
    for p in B.ALL_PATHS:
        assert reached.get(p), p
        print("%-22s %s" % (p, ", ".join(reached[p][:4]) + (" ..." if len(reached[p]) > 4 else "")))
    assert set(reached) == set(B.ALL_PATHS)
    # the rows of the table that are no path of the launch arithmetic: every numerical flavour on both sizes, ReLU on and off
    for flavor in ("big_mean", "pivot30", "pivot300", "const", "gy_const", "dead", "nonfinite", "eps_mom", "mom0"):
        for size in ("mid", "small"):
            for relu in ("relu", "lin"):
                assert "num-%s-%s-%s" % (flavor, size, relu) in B.BY_NAME
    assert {c.C for c in B.CASES if c.kind == "colsum"} == {4, 8, 16, 32, 64}
    assert {c.claims["slots"] for c in B.CASES if c.kind == "colsum"} >= {1, 2, 130}


def test_flavours_are_what_they_say():
    """From the reference alone: the dead channel is dead, the constant channel has variance 0, the pivot rows lie 30 and 300
    population sigmas out, the big mean is 1000 sigma."""
    for size in ("mid", "small"):
        inp, ref = B.reference(B.BY_NAME["num-dead-%s-relu" % size])
        assert (ref.act[:, B.DEAD_CHANNEL] < 0).all() and ref.dx[:, B.DEAD_CHANNEL].abs().max() == 0
        assert ref.dgamma[B.DEAD_CHANNEL] == 0 and ref.dbeta[B.DEAD_CHANNEL] == 0
        inp, ref = B.reference(B.BY_NAME["num-const-%s-lin" % size])
        assert ref.pack[1][:, B.CONST_CHANNEL].abs().max() == 0
        for k, flavor in ((30, "pivot30"), (300, "pivot300")):
            c = B.BY_NAME["num-%s-%s-lin" % (flavor, size)]
            inp, ref = B.reference(c)
            for g in range(c.groups):
                for ch in B.PIVOT_CHANNELS:
                    rest = inp["x"][g * c.rows + 1:(g + 1) * c.rows, ch].double()
                    dist = (inp["x"][g * c.rows, ch].double() - rest.mean()) / rest.std()
                    assert abs(dist / k - 1) < 0.1, (flavor, size, dist)
        inp, ref = B.reference(B.BY_NAME["num-big_mean-%s-lin" % size])
        assert ((ref.pack[0] / ref.pack[1].sqrt()) > 900).all()
        inp, ref = B.reference(B.BY_NAME["num-gy_const-%s-lin" % size])
        assert ref.dx[:, 1:].abs().max() < 1e-12 and ref.dx[:, 0].abs().max() > 0.1


def test_groups_must_divide_the_leading_dimension():
    """7 slices cannot form 2 or 3 equal groups: every BatchNorm entry raises before it looks at anything else (rows =
    numel // C // groups used to leave the trailing rows unwritten and outside the statistics).  The shape check comes before
    the device check, so this runs without a GPU; tests/test_gpu_bn_paths.py repeats it on device tensors."""
    from mvster_amd import ops
    from mvster_amd import train_ops as T
    x, gy = torch.randn(7, 5, 8), torch.randn(7, 5, 8)
    w, b = torch.ones(8), torch.zeros(8)
    for groups in (2, 3, 0):
        per = torch.ones(max(groups, 1), 8)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_train_fwd(x, w, b, None, None, 1e-5, 0.1, True, groups)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_train_bwd(x, gy, torch.ones(5, max(groups, 1), 8), True, groups)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_relu_fwd(x, per, per, True, groups)
        with pytest.raises(RuntimeError, match="does not divide"):
            ops.bn_relu_bwd(x, gy, per, per, per, per, True, groups)
        for train in (True, False):
            with pytest.raises(RuntimeError, match="does not divide"):
                T.batch_norm_cl(x, torch.nn.BatchNorm3d(8).train(train), relu=True, groups=groups)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # (7 groups of 5 rows do divide: the next check speaks)
        ops.bn_train_fwd(x, w, b, None, None, 1e-5, 0.1, True, 7)
