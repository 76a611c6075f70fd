"""Case table and float64 reference for the BatchNorm / column-sum kernels of csrc/bn_ops.hip (plain torch, CPU).

The five entry points restated operation by operation from the comments of bn_ops.hip:
  training forward    y = relu(x * scale + shift) (+ skip), scale = gamma * rstd, shift = beta - mean * scale, per statistics
                      group; pack = (mean, biased var, rstd, scale, shift); the running statistics after ``groups`` sequential
                      exponential updates with the unbiased variance (factor rows / max(rows - 1, 1)); counter += groups
  training backward   g = gy * (act > 0), xh = (x - mean) * rstd, dx = scale * (g - sum g / n - xh * sum g xh / n);
                      dbeta = sum g, dgamma = sum g xh, summed over the groups
  frozen fwd / bwd    the same with given (mean, rstd, scale, shift); dx = g * scale, the sums are not applied
  column sums         sum of [rows, C] over the rows
and the launch arithmetic (``slots_for``, ``train_slots_for``, ``train_apply_blocks``, the lane and round counts of
``sum_slots``, the two-rows-in-flight loop of ``col_sum_kernel``) as Python functions, so that every case can state which path
of the kernels it reaches; tests/test_bn_cases_cpu.py holds the claims against this restatement and the restatement against
the library's own host functions.

Tensors are [groups * rows, C] (channels last; group g owns rows [g * rows, (g + 1) * rows))."""
import collections

import torch

D = torch.float64
RED_THREADS = 1024            # kRedThreads
MAX_PAIRS = 2048              # kMaxPairs
BOUNDARY = 8 * 2.0 ** -24     # ReLU boundary: |act| <= BOUNDARY * (|x * scale| + |shift|) may fall on either side in fp32
MAX_BOUNDARY = 8              # such elements per case, at most


# ---- launch arithmetic ---------------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


def slots_for(rows, C, groups):
    n4 = rows * (C // 4)
    n = _ceil_div(n4, 4 * RED_THREADS)
    cap = 1 if groups >= 256 else 256 // groups
    return max(1, min(n, cap))


def train_slots_for(rows, C, groups):
    return min(slots_for(rows, C, groups), 4096 // C)


def train_apply_blocks(rows, C, groups):
    n4 = rows * (C // 4)
    n = _ceil_div(n4, 4 * RED_THREADS)
    cap = 1 if groups >= 512 else 512 // groups
    return max(1, min(n, cap))


def sum_slots_rounds(nblk, groups, C):
    """-> [(np, lanes, inner rounds)] per round of the ``base`` loop of sum_slots"""
    pairs = groups * 2 * C
    out = []
    for base in range(0, pairs, RED_THREADS):
        np_ = min(pairs - base, RED_THREADS)
        lanes = 1
        while lanes * 2 * np_ <= RED_THREADS:
            lanes *= 2
        out.append((np_, lanes, _ceil_div(nblk, lanes * 16)))
    return out


def col_sum_loop(n4, nblk):
    """-> (the two-row loop runs in some thread, the tail runs in some thread, the tail runs after the loop in some thread)"""
    stride = nblk * RED_THREADS
    full, rem = divmod(n4, stride)          # threads < rem read full + 1 float4s, the others full
    counts = {full + 1, full} if rem else {full}
    counts.discard(0)
    return (any(k >= 2 for k in counts), any(k % 2 for k in counts), any(k % 2 and k >= 3 for k in counts))


def facts(kind, rows, C, groups):
    """What a launch of ``kind`` ("train", "frozen", "colsum") does, from the restatement"""
    n4 = rows * (C // 4)
    if kind == "train":
        slots, blocks = train_slots_for(rows, C, groups), train_apply_blocks(rows, C, groups)
        rounds = sum_slots_rounds(slots, groups, C) + sum_slots_rounds(slots, 1, C)       # extra workgroup, apply prologue
    elif kind == "frozen":
        slots, blocks = slots_for(rows, C, groups), min(_ceil_div(n4, 256), 2048)
        rounds = sum_slots_rounds(slots, groups, C)
    else:
        slots, blocks = slots_for(rows, C, 1), 0
        rounds = sum_slots_rounds(slots, 1, C)
    f = dict(slots=slots, apply_blocks=blocks, base_rounds=len(sum_slots_rounds(slots, groups if kind != "colsum" else 1, C)),
             inner_rounds=max(r[2] for r in rounds))
    if kind == "colsum":
        f["pair_loop"], f["tail"], _ = col_sum_loop(n4, slots)
    return f


ALL_PATHS = (
    "base_round2_ragged",      # sum_slots: groups * 2C > 1024 with a ragged second round (training extra workgroup)
    "base_round2_full",        # ... with a full second round (2048 pairs)
    "frozen_base_round2",      # the same in the finisher of bn_relu_bwd_reduce_kernel
    "pairs_refused",           # groups * 2C > 2048: MVSTER_ERR_UNSUPPORTED
    "frozen_inner_round2",     # last arriver of bn_relu_bwd_reduce_kernel: more slots than lanes * 16
    "colsum_inner_round2",     # last arriver of col_sum_kernel: the same
    "colsum_pairs_tail",       # col_sum_kernel: two-row loop, then the odd remainder, several slots
    "colsum_pairs_no_tail",    # col_sum_kernel: two-row loop ends even in every thread, several slots
    "cap_C",                   # 4096 / C binds in train_slots_for
    "cap_groups",              # 256 / groups binds in slots_for
    "cap_apply",               # 512 / groups binds in train_apply_blocks
    "ifirst_beyond",           # more apply threads than float4s: the prefetch of the apply kernels has nothing to load
    "rows1",                   # one row per group: the unbias guard
    "small_n4_C4", "small_n4_C8", "small_n4_C16", "small_n4_C32", "small_n4_C64",       # n4 < 1024 at every width
    "stride_tail",             # n4 no multiple of the grid stride: a ragged last grid-stride round
)


def paths_of(kind, rows, C, groups):
    """The paths of ALL_PATHS a launch reaches, from the restatement"""
    n4 = rows * (C // 4)
    pairs = groups * 2 * C
    p = set()
    if kind == "refused":
        return {"pairs_refused"} if pairs > MAX_PAIRS else set()
    f = facts(kind, rows, C, groups)
    if kind == "train":
        if pairs > RED_THREADS:
            p.add("base_round2_full" if pairs % RED_THREADS == 0 else "base_round2_ragged")
        if slots_for(rows, C, groups) > 4096 // C:
            p.add("cap_C")
        if _ceil_div(n4, 4096) > (1 if groups >= 256 else 256 // groups):
            p.add("cap_groups")
        if _ceil_div(n4, 4096) > (1 if groups >= 512 else 512 // groups):
            p.add("cap_apply")
        if n4 < f["apply_blocks"] * RED_THREADS:
            p.add("ifirst_beyond")
        if rows == 1:
            p.add("rows1")
        if n4 < 1024:
            p.add("small_n4_C%d" % C)
        if n4 % (f["apply_blocks"] * RED_THREADS) or n4 % (f["slots"] * RED_THREADS):
            p.add("stride_tail")
    elif kind == "frozen":
        if pairs > RED_THREADS:
            p.add("frozen_base_round2")
        if f["inner_rounds"] > 1:
            p.add("frozen_inner_round2")
    else:
        if f["inner_rounds"] > 1:
            p.add("colsum_inner_round2")
        loop, _, tail_after = col_sum_loop(n4, f["slots"])
        if f["slots"] > 1 and tail_after:
            p.add("colsum_pairs_tail")
        if f["slots"] > 1 and loop and not f["tail"]:
            p.add("colsum_pairs_no_tail")
    return p


# ---- the table ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name kind rows C groups relu skip flavor eps momentum seed claims paths")


def _case(name, kind, rows, C, groups=1, relu=True, skip=False, flavor="typical", eps=1e-5, momentum=0.1, seed=0, claims=None,
          paths=()):
    return Case(name, kind, rows, C, groups, relu, skip, flavor, eps, momentum, seed, claims or {}, frozenset(paths))


def _claims(slots, apply_blocks, base_rounds, inner_rounds, pair_loop=None, tail=None):
    c = dict(slots=slots, apply_blocks=apply_blocks, base_rounds=base_rounds, inner_rounds=inner_rounds)
    if pair_loop is not None:
        c.update(pair_loop=pair_loop, tail=tail)
    return c


def _table():
    t = []
    # tiny: rows 3 and 1 at every width (n4 < 1024, one slot, one apply block, most threads without a float4)
    for C in (4, 8, 16, 32, 64):
        for rows in (3, 1):
            p = ["small_n4_C%d" % C, "ifirst_beyond", "stride_tail"] + (["rows1"] if rows == 1 else [])
            t.append(_case("tiny-r%dc%d" % (rows, C), "train", rows, C, relu=C != 16, skip=C == 8, seed=C + rows,
                           claims=_claims(1, 1, 1, 1), paths=p))
    # ragged: n4 just below, at and just above 1024 k (the nearest multiples of C / 4: a row is C / 4 float4s)
    for C in (8, 64):
        q = C // 4
        for k in (1, 4):
            for d in (-1, 0, 1):
                n4 = 1024 * k + d * q
                slots = 2 if (k == 4 and d == 1) else 1
                p = (["ifirst_beyond", "small_n4_C%d" % C] if n4 < 1024 else []) + (["stride_tail"] if d or slots == 2 else [])
                t.append(_case("ragged-c%dk%d%s" % (C, k, "m0p"[d + 1]), "train", n4 // q, C, relu=d != 0, skip=d == 1,
                               seed=10 * C + 3 * k + d, claims=_claims(slots, slots, 1, 1), paths=p))
    t.append(_case("cap_C", "train", 16385, 64, seed=2, claims=_claims(64, 65, 1, 1), paths=["cap_C", "stride_tail"]))
    t.append(_case("cap_groups", "train", 104449, 8, groups=5, seed=2, claims=_claims(51, 52, 1, 1),
                   paths=["cap_groups", "stride_tail"]))
    # (512 / groups cannot bind below 33 MB unless groups does not divide 512: 171 groups of 8193 four-channel rows, 22 MB)
    t.append(_case("cap_apply", "train", 8193, 4, groups=171, seed=4, claims=_claims(1, 2, 2, 1),
                   paths=["cap_apply", "cap_groups", "base_round2_ragged", "stride_tail"]))
    for C, groups, full in ((64, 9, False), (64, 16, True), (32, 17, False)):
        t.append(_case("pairs_2round-c%dg%d" % (C, groups), "train", 15, C, groups=groups, skip=groups == 9, seed=groups,
                       claims=_claims(1, 1, 2, 1),
                       paths=["base_round2_full" if full else "base_round2_ragged", "small_n4_C%d" % C, "ifirst_beyond",
                              "stride_tail"]))
        t.append(_case("frozen_pairs_2round-c%dg%d" % (C, groups), "frozen", 15, C, groups=groups, skip=groups == 16,
                       seed=groups, claims=_claims(1, _ceil_div(15 * C // 4, 256), 2, 1), paths=["frozen_base_round2"]))
    t.append(_case("pairs_refused", "refused", 15, 64, groups=17, paths=["pairs_refused"]))
    t.append(_case("frozen_2round", "frozen", 33025, 64, seed=5, claims=_claims(130, 2048, 1, 2), paths=["frozen_inner_round2"]))
    t.append(_case("frozen-r3c8", "frozen", 3, 8, relu=False, skip=True, seed=6, claims=_claims(1, 1, 1, 1)))
    t.append(_case("frozen-c16g3", "frozen", 4099, 16, groups=3, seed=7, claims=_claims(5, 65, 1, 1)))
    # column sums: slots 1, 2 and 129+, the two-row loop with and without its tail
    for C in (4, 8, 16, 32, 64):
        q = C // 4
        t.append(_case("colsum-tiny-c%d" % C, "colsum", 3, C, seed=C, claims=_claims(1, 0, 1, 1, False, True)))
        t.append(_case("colsum-1slot-even-c%d" % C, "colsum", 4096 // q, C, seed=C + 1, claims=_claims(1, 0, 1, 1, True, False)))
        t.append(_case("colsum-1slot-odd-c%d" % C, "colsum", 3072 // q - 1, C, seed=C + 2, claims=_claims(1, 0, 1, 1, True, True)))
    for C in (8, 64):
        q = C // 4
        t.append(_case("colsum-2slot-even-c%d" % C, "colsum", 8192 // q, C, seed=C + 3, claims=_claims(2, 0, 1, 1, True, False),
                       paths=["colsum_pairs_no_tail"]))
        t.append(_case("colsum-2slot-odd-c%d" % C, "colsum", 6144 // q + 1, C, seed=C + 4, claims=_claims(2, 0, 1, 1, True, True),
                       paths=["colsum_pairs_tail"]))
    t.append(_case("colsum-130slot-odd-c64", "colsum", 33025, 64, seed=8, claims=_claims(130, 0, 1, 2, True, True),
                   paths=["colsum_inner_round2", "colsum_pairs_tail"]))
    t.append(_case("colsum-130slot-even-c64", "colsum", 33280, 64, seed=9, claims=_claims(130, 0, 1, 2, True, False),
                   paths=["colsum_inner_round2", "colsum_pairs_no_tail"]))
    t.append(_case("colsum-130slot-c16", "colsum", 132100, 16, seed=10, claims=_claims(130, 0, 1, 1, True, True),
                   paths=["colsum_pairs_tail"]))
    t.append(_case("colsum-256slot-c4", "colsum", 1048579, 4, seed=11, claims=_claims(256, 0, 1, 1, True, True),
                   paths=["colsum_pairs_tail"]))
    # numerical cases: the mid-size tensor of the training step (2 x 8 x 64 x 80 x 8: 81920 rows) and two groups of 1280 rows
    for size, rows, groups in (("mid", 81920, 1), ("small", 1280, 2)):
        for flavor, kw in (("big_mean", {}), ("pivot30", {}), ("pivot300", {}), ("const", {}), ("gy_const", {}), ("dead", {}),
                           ("nonfinite", {}), ("eps_mom", dict(eps=1e-3, momentum=0.3)), ("mom0", dict(momentum=0.0))):
            for relu in (True, False):
                slots = 40 if size == "mid" else 1
                t.append(_case("num-%s-%s-%s" % (flavor, size, "relu" if relu else "lin"), "train", rows, 8, groups=groups,
                               relu=relu, flavor=flavor, seed=len(t), claims=_claims(slots, slots, 1, 1),
                               paths=["stride_tail"] if size == "small" else [], **kw))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
POISONED_CHANNEL = 3           # of the "nonfinite" flavor
DEAD_CHANNEL = 2               # of the "dead" flavor
CONST_CHANNEL = 5              # of the "const" flavor
PIVOT_CHANNELS = (1, 6)        # of the "pivot*" flavors


def make_inputs(case):
    """float32 CPU operands of a case: x, gy, skip (or None), weight, bias, running_mean, running_var"""
    g = torch.Generator().manual_seed(1000 + case.seed)
    n, C, rows = case.groups * case.rows, case.C, case.rows
    x = torch.randn(n, C, generator=g) * 2 + 0.5
    gy = torch.randn(n, C, generator=g)
    skip = torch.randn(n, C, generator=g) if case.skip else None
    weight, bias = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    fl = case.flavor
    if fl == "big_mean":
        # (mean 1000, sigma 1; the bias lifts the activations four sigma above the ReLU, whose boundary band is 1e-3 wide
        #  at |x * scale| = 1000 and would otherwise hold hundreds of elements)
        x = (x - 0.5) / 2 + 1000
        bias = 4 * weight
    elif fl in ("pivot30", "pivot300"):
        for gi in range(case.groups):
            for c in PIVOT_CHANNELS:
                x[gi * rows, c] = 0.5 + 2 * (30 if fl == "pivot30" else 300)
        # (the pivot channels' activations are lifted four sigma above the ReLU, as in big_mean: their boundary band widens
        #  with the pivot's distance and would hold up to 1757 elements at 300 sigma; the other channels keep the ReLU busy)
        bias = bias.clone()
        bias[list(PIVOT_CHANNELS)] = 4 * weight[list(PIVOT_CHANNELS)]
    elif fl == "const":
        x[:, CONST_CHANNEL] = 3.0
    elif fl == "gy_const":
        # (channel 0 keeps a random gradient, so that max |dx| gives the bound of the tensor a scale)
        gy[:, 1:] = torch.linspace(-1.0, 1.0, C)[1:]
    elif fl == "dead":
        bias = bias.clone()
        bias[DEAD_CHANNEL] = -50.0
    elif fl == "nonfinite":
        x[7, POISONED_CHANNEL] = float("nan")
        x[(case.groups - 1) * rows + 11, POISONED_CHANNEL] = float("inf")
    return dict(x=x, gy=gy, skip=skip, weight=weight, bias=bias, running_mean=rm, running_var=rv)


def frozen_pack(case, inp):
    """float32 (mean, rstd, scale, shift), each [groups, C], for a frozen case: per-group constants rounded from float64"""
    g = torch.Generator().manual_seed(2000 + case.seed)
    mean = torch.randn(case.groups, case.C, generator=g, dtype=D) * 0.3 + 0.5
    var = torch.rand(case.groups, case.C, generator=g, dtype=D) * 3 + 1
    rstd = (var + case.eps).rsqrt()
    scale = inp["weight"].to(D) * rstd
    shift = inp["bias"].to(D) - mean * scale
    return tuple(t.float() for t in (mean, rstd, scale, shift))


# ---- float64 reference ----------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "y pack running_mean running_var dx dgamma dbeta act xh boundary extra pivot")


def _backward(xg, gy, act, xh, scale, relu, rows, frozen):
    """-> dx, dgamma, dbeta"""
    g = gy * (act > 0) if relu else gy
    sg, sgx = g.sum(1), (g * xh).sum(1)
    if frozen:
        dx = g * scale[:, None]
    else:
        dx = scale[:, None] * (g - sg[:, None] / rows - xh * sgx[:, None] / rows)
    return dx, sgx.sum(0), sg.sum(0)


def _boundary(xg, act, gy, xh, scale, shift, relu, widen=None):
    """-> the mask of the ReLU-boundary elements and what they add to the tolerance of their group's sums [groups, C];
    ``widen`` [groups, C]: a factor on the width of the band"""
    if not relu:
        return torch.zeros_like(act, dtype=torch.bool), torch.zeros_like(scale)
    width = BOUNDARY * ((xg * scale[:, None]).abs() + shift[:, None].abs())
    band = act.abs() <= (width if widen is None else width * widen[:, None])
    extra = (band * gy.abs() * (1 + xh.abs())).sum(1)
    return band, extra


def ref_train(x, gy, weight, bias, running_mean, running_var, eps, momentum, relu, groups, skip=None, D=D):
    """Training-mode forward and backward in float64 -> Ref (tensors in x's shape or [groups, C] / [C]).  ``D``: the type to
    compute in (float32 on the device: the same code as a measure of what fp32 costs, where torch's BatchNorm has no answer)"""
    C = x.shape[-1]
    xg = x.to(D).reshape(groups, -1, C)
    rows = xg.shape[1]
    w, b = weight.to(D), bias.to(D)
    mean = xg.mean(1)
    var = ((xg - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / (var + eps).sqrt()
    scale = w * rstd
    shift = b - mean * scale
    act = xg * scale[:, None] + shift[:, None]
    y = act.clamp_min(0.0) if relu else act
    if skip is not None:
        y = y + skip.to(D).reshape(groups, -1, C)
    rm, rv = running_mean.to(D).clone(), running_var.to(D).clone()
    unbias = rows / max(rows - 1, 1)
    for gi in range(groups):
        rm = (1 - momentum) * rm + momentum * mean[gi]
        rv = (1 - momentum) * rv + momentum * (var[gi] * unbias)
    xh = (xg - mean[:, None]) * rstd[:, None]
    gyd = gy.to(D).reshape(groups, -1, C)
    dx, dgamma, dbeta = _backward(xg, gyd, act, xh, scale, relu, rows, False)
    # the distance of the statistics' pivot, the group's first row, from the mean in standard deviations (eps inside: a constant
    # channel is at distance 0)
    pivot = (xg[:, 0] - mean).abs() * rstd
    # (the activation keeps its accuracy times (1 + r)^2, tests/test_gpu_bn_paths.py, so the band within which the ReLU may
    #  fall on either side is that much wider; still at most MAX_BOUNDARY elements per case)
    band, extra = _boundary(xg, act, gyd, xh, scale, shift, relu, (1 + pivot.nan_to_num(0.0)) ** 2)
    return Ref(y.reshape(x.shape), torch.stack([mean, var, rstd, scale, shift]), rm, rv, dx.reshape(x.shape), dgamma, dbeta,
               act.reshape(x.shape), xh.reshape(x.shape), band.reshape(x.shape), extra, pivot)


def ref_frozen(x, gy, mean, rstd, scale, shift, relu, groups, skip=None):
    """Forward and backward with constant statistics ([groups, C] each) in float64 -> Ref"""
    C = x.shape[-1]
    xg = x.to(D).reshape(groups, -1, C)
    mean, rstd, scale, shift = (t.to(D) for t in (mean, rstd, scale, shift))
    act = xg * scale[:, None] + shift[:, None]
    y = act.clamp_min(0.0) if relu else act
    if skip is not None:
        y = y + skip.to(D).reshape(groups, -1, C)
    xh = (xg - mean[:, None]) * rstd[:, None]
    gyd = gy.to(D).reshape(groups, -1, C)
    dx, dgamma, dbeta = _backward(xg, gyd, act, xh, scale, relu, xg.shape[1], True)
    band, extra = _boundary(xg, act, gyd, xh, scale, shift, relu)
    return Ref(y.reshape(x.shape), None, None, None, dx.reshape(x.shape), dgamma, dbeta, act.reshape(x.shape),
               xh.reshape(x.shape), band.reshape(x.shape), extra, None)


def ref_col_sum(x):
    return x.to(D).reshape(-1, x.shape[-1]).sum(0)


def reference(case):
    """(inputs, Ref) of a training or frozen case"""
    inp = make_inputs(case)
    if case.kind == "train":
        ref = ref_train(inp["x"], inp["gy"], inp["weight"], inp["bias"], inp["running_mean"], inp["running_var"], case.eps,
                        case.momentum, case.relu, case.groups, inp["skip"])
    else:
        inp["frozen"] = frozen_pack(case, inp)
        ref = ref_frozen(inp["x"], inp["gy"], *inp["frozen"], case.relu, case.groups, inp["skip"])
    return inp, ref
