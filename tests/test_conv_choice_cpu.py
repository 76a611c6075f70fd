"""The case table of tests/conv_choice_cases.py checked without a GPU: its reference against PyTorch, the census of what
``ConvLayer._geom`` picks over the table (a stub library stands in for the HIP one: every symbol present), the exactness
budget of the integer data and the float32 restatement of Winograd F(2x2, 3x3) that entitles the GPU test to demand bit-exact
results of variants 8 and 9."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mvster_amd import _lib
from mvster_amd import conv_plan as cp
from tests import conv_choice_cases as C


class _StubLibrary:
    """Every entry point "exists" (``_geom`` only asks ``hasattr``); none is ever called on the CPU."""

    def __getattr__(self, name):
        if name.startswith("mvster_"):
            return lambda *a: _lib.ERR_UNSUPPORTED
        raise AttributeError(name)


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _StubLibrary())
    monkeypatch.setattr(cp, "FORCE_VARIANT", None)


def set_mode(monkeypatch, mode):
    """"shipped": the measured table, its families and the heuristics; "heuristic": table and families empty."""
    if mode == "heuristic":
        monkeypatch.setattr(cp, "_TUNING", {})
        monkeypatch.setattr(cp, "_FAMILIES", {})
    else:
        monkeypatch.setattr(cp, "_TUNING", None)
        monkeypatch.setattr(cp, "_FAMILIES", None)


def stub_layer(f):
    """The form's layer over zero weights; a Winograd-eligible one gets a placeholder for the transformed weights that only
    exist on the device."""
    layer = C.make_layer(f, torch.zeros(C.weight_shape(f)), prob=(torch.zeros(8), torch.zeros(1)) if f.prob else None)
    assert C.layer_key(layer) == C.form_key(f)
    assert layer.wino_eligible() == C.wino_eligible(f)
    if layer.wino_eligible():
        layer.wpk_wino = torch.zeros(1)
    return layer


GEOMETRIES = sorted({(f.kernel, f.stride, f.padding, f.transposed) for f in C.FORMS})


@pytest.mark.parametrize("kernel,stride,padding,transposed", GEOMETRIES)
def test_conv_ref64_is_the_torch_convolution(kernel, stride, padding, transposed):
    g = torch.Generator().manual_seed(sum(kernel) + 3 * sum(stride) + 5 * sum(padding) + transposed)
    cin, cout = 3, 5
    x = torch.randn(2, 4, 6, 8, cin, generator=g, dtype=torch.float64)
    w = torch.randn(*((cin, cout) if transposed else (cout, cin)), *kernel, generator=g, dtype=torch.float64)
    x.requires_grad_(True)
    xn = x.permute(0, 4, 1, 2, 3)
    if transposed:
        want = F.conv_transpose3d(xn, w, stride=stride, padding=padding, output_padding=tuple(s - 1 for s in stride))
    else:
        want = F.conv3d(xn, w, stride=stride, padding=padding)
    got = C.conv_ref64(x, w, stride, padding, transposed)
    want = want.permute(0, 2, 3, 4, 1)
    assert got.shape == want.shape and got.dtype == torch.float64
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    # ... and autograd through it is the reference of the training role's input gradient
    gy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    dx_want, dx_got = torch.autograd.grad(want, x, gy)[0], torch.autograd.grad(got, x, gy)[0]
    assert (dx_got - dx_want).abs().max() <= 1e-12 * dx_want.abs().max()


def test_forms_and_ladders_are_well_formed():
    names = collections.Counter(f.name for f in C.FORMS)
    assert max(names.values()) == 1
    roles = collections.Counter(f.role for f in C.FORMS)
    assert roles["eval"] >= 30 and roles["train"] >= 30 and roles["dgrad"] >= 29
    for f in C.FORMS:
        assert f.ladder and len(set(f.ladder)) == len(f.ladder), f.name
        for B, D, H, W in f.ladder:
            # nothing beyond [10, 1, 128, 160] x 64 channels on either side of the layer
            assert B * D * H * W * (f.cin_pad or f.cin) <= 10 * 128 * 160 * 64, (f.name, (B, D, H, W))
            oB, oD, oH, oW = C.out_shape(f, (B, D, H, W))
            assert oB * oD * oH * oW * f.cout <= 10 * 128 * 160 * 64 * 2.25, (f.name, (B, D, H, W))
            if not f.transposed and f.stride != C.S1:
                assert all(n % s == 0 for n, s in zip((D, H, W), f.stride)), (f.name, (B, D, H, W))   # (its adjoint doubles)
            if C.SKIP_UPSAMPLE_ADD in f.skips:
                assert D == 1 and oH % 2 == 0 and oW % 2 == 0, (f.name, (B, D, H, W))
    # the input-gradient rule, on the examples the training step is known for
    d = {f.name: f for f in C.FORMS if f.role == "dgrad"}
    assert C.form_key(d["d_fpn_conv1_0"])[:7] == (16, 16, 8, C.K155, C.S122, (0, 2, 2), True)      # 8 -> 16 1x5x5 stride 2
    assert C.form_key(d["d_reg2d_conv9"])[:7] == (16, 16, 32, C.K133, C.S122, (0, 1, 1), False)    # transposed 32 -> 16
    assert C.form_key(d["d_mono_head0"])[:7] == (1, 4, 64, C.K133, C.S1, (0, 1, 1), False)         # head 64 -> 1
    assert C.form_key(d["d_reg2d_conv0_g4"])[:7] == (8, 8, 4, C.K133, C.S1, (0, 1, 1), False)      # reg2d conv0, G = 4
    assert C.form_key(d["d_fpn_fine_g"])[:3] == (72, 80, 64)


# variant words (family, workgroups-per-CU bits where the family reads them) the shapes of the table must reach
REQUIRED = ([(v, None) for v in (0, 1, 2, 3, 4, 8, 9, 10)] + [(5, w) for w in (0, 1, 2, 3)] + [(6, 2), (6, 3)] + [("narrow4", None)])


def test_census_of_the_plans_choices(stub, monkeypatch, capsys):
    """``_geom`` over all forms x ladder x plan modes x {SKIP_NONE, SKIP_ADD}: every product variant is named at least once and
    every override branch behind the table lookup is taken and skipped -- a dispatch edit that orphans a kernel fails here.
    The branches are restated from their conditions; where one applies the choice must be its kernel."""
    words = collections.Counter()
    reached = collections.Counter()
    branch = collections.Counter()
    wino = collections.defaultdict(set)
    for mode in C.MODES:
        set_mode(monkeypatch, mode)
        for f in C.unique_forms():
            layer = stub_layer(f)
            for shape in f.ladder:
                lattice = shape if f.transposed else C.out_shape(f, shape)
                voxels = lattice[0] * lattice[1] * lattice[2] * lattice[3]
                for sm in (C.SKIP_NONE, C.SKIP_ADD):
                    _, mt, nt, _, v = layer._geom(*shape, sm)
                    tuned = cp.tuned_choice(layer, *shape, sm)[0]
                    fam = v & 0xff
                    four = fam == 10 and layer.w_small is None
                    words[("0x%x" % v) + (" (four-channel form)" if four else "")] += 1
                    reached["narrow4" if four else fam, None] += 1
                    reached[fam, (v >> 8) & 15] += 1
                    # narrow layers: the table's entry, else the MFMA kernel from NARROW_MIN_VOXELS, else the VALU kernel
                    if layer.w_small is not None:
                        assert fam in (3, 10), (f.name, shape, sm, mode, v)
                        if not (tuned and tuned[0] in (3, 10)):
                            branch["narrow rule", voxels >= 16384] += 1
                            assert (v, mt, nt) == ((10, 0, 0) if voxels >= 16384 else (3, 0, 0)), (f.name, shape, sm, mode, v)
                        else:
                            branch["narrow table", True] += 1
                    else:
                        branch["narrow", False] += 1
                    # 8 -> 4: the four-channel form without a skip, from the same size
                    if layer.w_small4 is not None:
                        take = sm == C.SKIP_NONE and voxels >= 16384
                        branch["narrow4", take] += 1
                        assert four == take, (f.name, shape, sm, mode, v)
                    # 16 -> 8 transposed 3x3: the VALU kernel, or the persistent MFMA kernel from TPERS16_MIN_VOXELS (no head)
                    if layer.w_deconv is not None:
                        take = layer.prob is None and voxels >= 40960
                        branch["deconv", True] += 1
                        branch["tpers16", take] += 1
                        assert (v, mt, nt) == (5, 2, 1) if take else v == 4, (f.name, shape, sm, mode, v)
                    else:
                        branch["deconv", False] += 1
                    # transposed 1x5x5 stride 2, 16 / 32 channels: the persistent kernel from the same size
                    if f.transposed and f.kernel == C.K155:
                        take = layer.cin in (16, 32) and voxels >= 40960
                        branch["tpers5", take] += 1
                        assert ((v, mt, nt) == (5, 2, 1)) == take, (f.name, shape, sm, mode, v)
                    if mode == "heuristic" and layer.wino_eligible() and layer.prob is None:
                        wino[f.name].add(fam in (8, 9))
                        wino[f.name, "nt"].add((fam, nt))
    with capsys.disabled():
        print("\ncensus (variant word -> cases): " + ", ".join("%s: %d" % kv for kv in sorted(words.items())))
    missing = [r for r in REQUIRED if not reached[r]]
    assert not missing, (missing, sorted(words.items()))
    assert not any((v & 0xff) in (7, 11) for v in (int(k.split()[0], 16) for k in words))      # probe variants: never chosen
    for name in ("narrow rule", "narrow4", "tpers16", "tpers5", "deconv"):
        assert branch[name, True] and branch[name, False], (name, branch)
    assert branch["narrow table", True] and branch["narrow", False]
    # every Winograd-eligible form's ladder stands on both sides of _wino_plan's work-unit count, and the ring kernel's
    # ladders on both sides of its two-N-tile count where it has one
    for f in C.unique_forms():
        if C.wino_eligible(f) and not f.prob:
            assert wino[f.name] == {False, True}, (f.name, wino[f.name])
            if len(C.wino_thresholds(f.cin_pad or f.cin, f.cout, f.kernel[0])) == 2:
                assert {(9, 1), (9, 2)} <= wino[f.name, "nt"], (f.name, wino[f.name, "nt"])


def test_heuristic_mode_sees_the_lds_plan_thresholds(stub, monkeypatch):
    """Wo < 24 keeps a layer off the LDS-staged kernel, Ho < 6 takes its four-row tile: both sides are in every ladder of a
    16-channel-multiple conv with a 3- or 5-wide kernel, and the kernel is chosen somewhere on it where its patch fits."""
    set_mode(monkeypatch, "heuristic")
    for f in C.unique_forms():
        if f.transposed or (f.cin_pad or f.cin) % 16 or f.kernel[2] not in (3, 5):
            continue
        layer = stub_layer(f)
        seen, fits = set(), False
        for shape in f.ladder:
            _, _, Ho, Wo = C.out_shape(f, shape)
            _, mt, nt, _, v = layer._geom(*shape, C.SKIP_NONE)
            plan = cp._lds_plan(shape[0], C.out_shape(f, shape)[1], Ho, Wo, f.kernel, f.stride, layer.ntile_total)
            if Wo < 24:
                assert plan is None and (v & 0xff) != 1, (f.name, shape)
            fits = fits or plan is not None
            if (v & 0xff) == 1:
                assert Wo >= 24 and (mt == 2 or Ho >= 6), (f.name, shape, mt)
                seen.add(("lds", mt))
            seen.add(("narrow", Wo < 24))
            seen.add(("low", Ho < 6))
        assert {("narrow", True), ("narrow", False), ("low", True), ("low", False)} <= seen, (f.name, seen)
        assert any(s[0] == "lds" for s in seen) == fits, (f.name, seen)      # (3x3x3 stride 2: the patch never fits the LDS budget)


def test_integer_data_stays_exact_in_float32():
    """K * max |x| * max |w| through the epilogue (scale <= 2, shift, skip, the 8 -> 1 head), counted in halves, and the
    training role's doubled weights: below 2^24, so every partial sum of every kernel is an exactly representable number and
    the order of the additions cannot matter."""
    worst = 0
    for f in C.FORMS:
        b = C.exact_budget(f)
        worst = max(worst, b)
        assert b < 2 ** 24, (f.name, b)
        if f.role == "train":
            assert 2 * C.reduction_length(f) * 2 * 2 * 2 + 3 < 2 ** 24            # forward after w.mul_(2), plus the bias
        if f.role == "dgrad":
            assert 2 * C.reduction_length(f) * 2 * 2 * 2 + 2 < 2 ** 24            # input gradient after w.mul_(2), plus the tap's
    assert worst >= 27 * 64 * 4 * 2                                                # (the 64 -> 64 3x3x3 layer is in the table)
    d = C.case_data(C.BY_NAME["e_reg2d_conv11_prob"], (1, 4, 6, 10), "cpu", exact=True)
    for t in (d["x"], d["w"], d["shift"], d["skip"][C.SKIP_ADD], d["prob"][0], d["prob"][1]):
        assert torch.equal(t, t.round()) and t.abs().max() <= 3
    assert set(d["scale"].tolist()) <= set(C.SCALES)
    assert d["x"].abs().max() == 2 and d["w"].abs().max() == 2


# ---- Winograd F(2x2, 3x3) in float32 ---------------------------------------------------------------------------------------
# the constants of conv_wino.hip: G (weights, packed once: mvster_pack_wino_weights), B^T (input tiles), A^T (output)
G_ = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float32)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float32)


def winograd_f32(x, w):
    """x [B, D, H, W, cin], w [cout, cin, kd, 3, 3] (float32 arrays), padding (kd // 2, 1, 1) -> [B, D, H, W, cout], every
    operation in float32: U = G g G^T, V = B^T d B per 4 x 4 input tile, M = sum over channels and depth taps of U * V,
    Y = A^T M A."""
    B, D, H, W, cin = x.shape
    cout, _, kd = w.shape[:3]
    ty, tx = -(-H // 2), -(-W // 2)
    xp = np.zeros((B, D + kd - 1, 2 * ty + 2, 2 * tx + 2, cin), dtype=np.float32)
    xp[:, kd // 2:kd // 2 + D, 1:H + 1, 1:W + 1] = x
    U = np.einsum("ij,ockjl,ml->kocim", G_, w, G_)
    tiles = np.lib.stride_tricks.sliding_window_view(xp, (4, 4), axis=(2, 3))[:, :, ::2, ::2]     # [B, Dp, ty, tx, cin, 4, 4]
    V = np.einsum("ij,bdyxcjl,ml->bdyxcim", BT, tiles, BT)
    M = np.zeros((B, D, ty, tx, cout, 4, 4), dtype=np.float32)
    for k in range(kd):
        M += np.einsum("ocim,bdyxcim->bdyxoim", U[k], V[:, k:k + D])
    Y = np.einsum("ij,bdyxojl,ml->bdyxoim", AT, M, AT)                                          # [B, D, ty, tx, cout, 2, 2]
    for a in (U, V, M, Y):
        assert a.dtype == np.float32
    y = Y.transpose(0, 1, 2, 5, 3, 6, 4).reshape(B, D, 2 * ty, 2 * tx, cout)
    return y[:, :, :H, :W], float(np.abs(U).max()), float(np.abs(V).max()), float(np.abs(M).max())


@pytest.mark.parametrize("name,shape", [("e_fpn_conv1_x", (2, 1, 7, 9)), ("e_fpn_conv3_x", (1, 1, 6, 11)), ("e_reg_conv6", (1, 3, 6, 10)),
                                        ("e_reg_conv4", (1, 2, 5, 8)), ("d_fpn_out2", (1, 1, 9, 6))])
def test_winograd_restated_in_float32_is_exact_on_the_integer_data(name, shape):
    """What entitles the GPU test to ask variants 8 / 9 for ``torch.equal``: with x, w in {-2..2} the transformed weights are
    multiples of 1/4 with |U| <= 4.5, the transformed tiles integers with |V| <= 8, and K <= 192 products of them stay below
    192 * 4.5 * 8 = 6912 (27648 quarters); the output transform adds nine of those: 2.5e5 quarters, far inside 24 bits.  So
    F(2x2, 3x3) in float32, in any order of its additions, IS the float64 convolution on this data."""
    f = C.BY_NAME[name]
    assert C.wino_eligible(f) and f.cin * f.kernel[0] <= 192
    d = C.case_data(f, shape, "cpu", exact=True)
    want = C.conv_ref64(d["x"], d["w"], f.stride, f.padding, False)
    got, u, v, m = winograd_f32(d["x"].numpy(), d["w"].numpy())
    assert u <= 4.5 and v <= 8 and m <= 6912
    assert np.array_equal(got.astype(np.float64), want.numpy())
    assert max(g.cin * g.kernel[0] for g in C.FORMS if C.wino_eligible(g)) <= 192
    # (and the restatement is not vacuous: on normal data it differs from float64 in the last bits)
    d = C.case_data(f, shape, "cpu", exact=False)
    want = C.conv_ref64(d["x"], d["w"], f.stride, f.padding, False).numpy()
    got = winograd_f32(d["x"].numpy(), d["w"].numpy())[0].astype(np.float64)
    err = np.abs(got - want).max() / np.abs(want).max()
    assert 0 < err <= 2e-6


@pytest.mark.parametrize("name,shape,sm,mode,want", [
    ("e_fpn_conv1_x", (6, 1, 64, 128), 0, "shipped", 0x105), ("e_fpn_conv1_x", (6, 1, 64, 128), 0, "heuristic", 0x108),
    ("e_reg_conv2", (1, 8, 32, 64), 0, "shipped", 0x305), ("e_reg_conv2", (1, 8, 32, 64), 0, "heuristic", 0x1),
    ("e_reg2d_conv1", (1, 4, 12, 20), 0, "shipped", 0x205), ("d_fpn_inner1", (10, 1, 64, 80), 0, "shipped", 0x306),
    ("t_reg2d_conv11", (2, 4, 64, 80), 0, "shipped", 0x5), ("t_reg2d_conv11", (2, 4, 64, 79), 0, "shipped", 0x4),
    ("d_reg2d_conv0_g4", (2, 4, 46, 45), 0, "shipped", 0xa), ("d_reg2d_conv0_g4", (2, 4, 46, 45), 1, "shipped", 0x0)])
def test_choices_the_ladders_were_built_around(stub, monkeypatch, name, shape, sm, mode, want):
    """Ten of the (form, shape) pairs behind the ladders, with the variant word each takes today: family entries measured on
    another shape, the heuristics with the table emptied, both sides of the transposed 16 -> 8 threshold and the two skip
    modes of the 8 -> 4 layer.  (A re-measured table may move the "shipped" ones: then these rows follow it.)"""
    set_mode(monkeypatch, mode)
    f = C.BY_NAME[name]
    assert shape in C.unique_forms()[[C.form_key(g) for g in C.unique_forms()].index(C.form_key(f))].ladder
    assert C.effective_choice(stub_layer(f), shape, sm)[0] == want
