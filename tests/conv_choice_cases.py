"""Case table for the tests of the convolution plan's OWN choice (tests/test_conv_choice_cpu.py, tests/test_gpu_conv_choice.py).

``ConvLayer.__call__`` without ``tiles`` runs the kernel and tile word that ``ConvLayer._geom`` picks for the shape: an exact
entry of the measured table, the nearest entry of the layer's family, the heuristics (``_lds_plan``, split-K, ``_wino_plan``)
and the overrides for narrow and transposed layers.  This module lists

* FORMS: every layer form the shipped networks build -- the eval plans (``Reg2dPlan`` G = 8 / 4, ``Reg3dPlan`` down_size 3 / 2,
  ``FpnPlan``), the training forward (``train_ops.conv_cl``) and the input-gradient layers ``_ConvCL.backward`` constructs
  from it (``dgrad_of`` restates that rule), each with a ladder of input sizes [B, D, H, W] that crosses the thresholds its
  ``_geom`` branch can see;
* ``conv_ref64``: the reference, a plain tap loop in float64 on whatever device its inputs live on;
* the integer / normal test data, the epilogue in float64, and the kernel family a variant word must dispatch.

The thresholds below are written out as numbers (not read from conv_plan): the census test fails when the plan's thresholds
move away from them, which is the point."""
import collections

import torch
import torch.nn.functional as F

from mvster_amd import conv_plan as cp

SKIP_NONE, SKIP_ADD, SKIP_UPSAMPLE_ADD = cp.SKIP_NONE, cp.SKIP_ADD, cp.SKIP_UPSAMPLE_ADD
MODES = ("shipped", "heuristic")

# cin = the weight tensor's input channels, cin_pad = what the kernel reads (None: cin); prob = fused 8 -> 1 head;
# skips = the skip modes the product calls the form with; role = "eval" | "train" | "dgrad"; depth = 1 for the 2-D networks,
# 4 for the cascade volumes; ladder = input shapes [B, D, H, W]
Form = collections.namedtuple("Form", "name cin cout kernel stride padding transposed cin_pad relu prob bias skips role depth "
                                      "ladder")

K133, K333, K155, K111 = (1, 3, 3), (3, 3, 3), (1, 5, 5), (1, 1, 1)
S1, S122, S222 = (1, 1, 1), (1, 2, 2), (2, 2, 2)


def pad_channels(c):
    """train_ops._cin_for: the channel counts the kernels take."""
    return next(a for a in (4, 8, 16, 32, 64) if c <= a)


def same_padding(kernel):
    return tuple(k // 2 for k in kernel)


# ---- size ladders ------------------------------------------------------------------------------------------------------
# All on the lattice the kernel tiles: the output of an ordinary conv, the INPUT of a transposed one.
def tiles_shape(t, depth):
    """[B, D, H, W] with exactly ``t`` 8 x 32 tiles (B * D * ceil(H / 8) * ceil(W / 32)), ragged in H and W; the largest such
    count <= t that factorises."""
    while t > 0:
        for d in ((depth,) if depth == 1 else (4, 2, 3)):
            for tx, w in ((3, 95), (4, 97), (2, 33), (1, 31)):
                for b in (1, 2, 3, 5, 4, 6, 7, 8, 9, 10):
                    r, rem = divmod(t, d * tx * b)
                    if rem == 0 and 1 <= r <= 16:
                        return (b, d, 8 * r - 3, w)
        t -= 1
    raise ValueError("no shape")


def wino_thresholds(cin, cout, kd):
    """Tile counts at which ``_wino_plan`` changes its answer for a Winograd-eligible layer: 192 work units for the 1x3x3
    kernel (16 / 32 input channels), 160 (one N tile) and 224 (two N tiles) for the ring kernel."""
    ntt = cout // 16
    if kd == 1 and cin in (16, 32):
        return [-(-192 // (ntt // (2 if ntt % 2 == 0 else 1)))]
    out = [-(-160 // ntt)]
    if ntt % 2 == 0 and cin != 16:
        out.append(-(-224 // (ntt // 2)))
    return out


def wino_eligible(f):
    return (not f.transposed and f.kernel in (K133, K333) and f.stride == S1 and f.padding == same_padding(f.kernel)
            and (f.cin_pad or f.cin) in (16, 32, 64) and f.cout % 16 == 0)


def lattice_ladder(f, also=()):
    """The tiled-lattice shapes for form ``f`` (and for the forms in ``also``: its input-gradient layer sees the same lattice)."""
    d = f.depth
    shapes = [(1, d, 7, 31),                 # one voxel row below a tile, ragged both ways
              (2, d, 5, 40),                 # Ho < 6: _lds_plan drops to four-row tiles
              (1, d, 16, 23),                # Wo < 24: no LDS plan
              (1, d, 6, 24),                 # ... and at both of its thresholds
              (2, d, 63, 79),                # within FAMILY_REACH of the table's 64 x 80 / 128 x 160 entries, equal to none
              # the family lookup knows voxels, depth and batch, not the aspect: a tall map narrower than a tile and a flat
              # one of eleven ragged tiles, at voxel counts where table entries are in reach
              (4, d, 125, 20), (3, d, 3, 333)]
    for g in (f,) + tuple(also):
        if (g.cin_pad or g.cin) in (4, 8) and g.kernel == K133 and g.stride == S1 and not g.transposed and g.cout in (4, 8):
            shapes += [(1, 1, 127, 129), (1, 1, 128, 128), (2, 4, 46, 45)]       # NARROW_MIN_VOXELS = 16384: 16383, 16384, 16560
        if g.transposed and g.stride == S122 and (g.cin_pad or g.cin) in (16, 32):
            shapes += [(2, 4, 64, 79), (2, 4, 64, 80)] if d > 1 else [(8, 1, 64, 79), (8, 1, 64, 80)]   # TPERS16_MIN_VOXELS = 40960
        if wino_eligible(g):
            for t in wino_thresholds(g.cin_pad or g.cin, g.cout, g.kernel[0]):
                shapes += [tiles_shape(t - 1, d), tiles_shape(t, d)]
    if d == 1:
        shapes.append((10, 1, 64, 80))
        if (f.cin_pad or f.cin) <= 32 and f.cout <= 64 and f.stride == S1:
            shapes.append((10, 1, 128, 160))
    if SKIP_UPSAMPLE_ADD in f.skips:         # the half-resolution skip needs even sizes
        shapes = [(b, dd, h + h % 2, w + w % 2) for b, dd, h, w in shapes]
    out = []
    for s in shapes:
        if s not in out:
            out.append(s)
    return out


def to_input(f, lattice):
    """Input shape whose tiled lattice is ``lattice``."""
    B, D, H, W = lattice
    if f.transposed:
        return lattice
    return (B, D * f.stride[0], H * f.stride[1], W * f.stride[2])


def out_shape(f, shape):
    B, D, H, W = shape
    if f.transposed:
        return (B, D * f.stride[0], H * f.stride[1], W * f.stride[2])
    return (B,) + tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip((D, H, W), f.padding, f.kernel, f.stride))


def dgrad_of(f):
    """The layer ``_ConvCL.backward`` builds for the input gradient of training form ``f``: a transposed layer's adjoint is the
    strided conv over the same weight tensor read as [out = cin, in = cout]; a stride-1 conv's is the conv with flipped taps and
    swapped channels, padding k - 1 - p; a strided conv's is the transposed (parity-class) form.  The output gradient is padded
    to a channel count the kernels take (1 -> 4 for the heads)."""
    co_p = pad_channels(f.cout)
    kw = dict(name="d_" + f.name[2:], cin=f.cout, cout=f.cin, kernel=f.kernel, stride=f.stride, cin_pad=co_p, relu=False, prob=False,
              bias=False, skips=(SKIP_NONE, SKIP_ADD), role="dgrad", depth=f.depth, ladder=None)
    if f.transposed:
        g = Form(padding=f.padding, transposed=False, **kw)
    elif f.stride == S1:
        g = Form(padding=tuple(k - 1 - p for k, p in zip(f.kernel, f.padding)), transposed=False, **kw)
    else:
        g = Form(padding=f.padding, transposed=True, **kw)
    return g


def _form(name, cin, cout, kernel, stride=S1, padding=None, transposed=False, cin_pad=None, relu=False, prob=False, bias=False,
          skips=(SKIP_NONE,), role="eval", depth=1, extra=()):
    """``extra``: input shapes beyond the rule-made ladder (kept in the ``ladder`` field until ``_build`` fills it)."""
    if padding is None:
        padding = same_padding(kernel)
    if cin_pad == cin:
        cin_pad = None
    return Form(name, cin, cout, kernel, stride, padding, transposed, cin_pad, relu, prob, bias, tuple(skips), role, depth, tuple(extra))


def _eval_forms():
    fs = []
    add = lambda *a, **k: fs.append(_form(*a, **k))
    # Reg2dPlan, G = 8 and 4 (conv_plan.py: _cbr3d / _up3d fold BatchNorm and ReLU; conv7 / 9 / 11 add the U-Net skip)
    for G in (8, 4):
        add("e_reg2d_conv0_g%d" % G, G, 8, K133, relu=True, depth=4)
    add("e_reg2d_conv1", 8, 16, K133, S122, relu=True, depth=4, extra=[(1, 4, 12, 20)])      # (a map smaller than a tile)
    add("e_reg_conv2", 16, 16, K333, relu=True, depth=4, extra=[(1, 8, 32, 64)])
    add("e_reg2d_conv3", 16, 32, K133, S122, relu=True, depth=4)
    add("e_reg_conv4", 32, 32, K333, relu=True, depth=4)
    add("e_reg2d_conv5", 32, 64, K133, S122, relu=True, depth=4)
    add("e_reg_conv6", 64, 64, K333, relu=True, depth=4)
    add("e_reg2d_conv7", 64, 32, K133, S122, transposed=True, relu=True, skips=(SKIP_ADD,), depth=4)
    add("e_reg2d_conv9", 32, 16, K133, S122, transposed=True, relu=True, skips=(SKIP_ADD,), depth=4)
    add("e_reg2d_conv11_prob", 16, 8, K133, S122, transposed=True, relu=True, prob=True, skips=(SKIP_ADD,), depth=4)
    add("e_reg2d_conv11", 16, 8, K133, S122, transposed=True, relu=True, skips=(SKIP_ADD,), depth=4)
    # Reg3dPlan, down_size 3 and 2 (conv2 / conv4 / conv6 are reg2d's forms)
    add("e_reg3d_conv0", 8, 8, K333, relu=True, depth=4)
    add("e_reg3d_conv1", 8, 16, K333, S222, relu=True, depth=4)
    add("e_reg3d_conv3", 16, 32, K333, S222, relu=True, depth=4)
    add("e_reg3d_conv5", 32, 64, K333, S222, relu=True, depth=4)
    add("e_reg3d_conv7", 64, 32, K333, S222, transposed=True, relu=True, skips=(SKIP_ADD,), depth=4)
    add("e_reg3d_conv9", 32, 16, K333, S222, transposed=True, relu=True, skips=(SKIP_ADD,), depth=4)
    add("e_reg3d_conv11", 16, 8, K333, S222, transposed=True, relu=True, skips=(SKIP_ADD,), depth=4)
    add("e_reg3d_prob", 8, 1, K333, depth=4)
    # FpnPlan (base 8)
    add("e_fpn_conv0_0", 3, 8, K133, cin_pad=4, relu=True)
    add("e_fpn_conv0_1", 8, 8, K133, relu=True)
    add("e_fpn_conv1_0", 8, 16, K155, S122, relu=True)
    add("e_fpn_conv1_x", 16, 16, K133, relu=True, extra=[(6, 1, 64, 128)])
    add("e_fpn_conv2_0", 16, 32, K155, S122, relu=True)
    add("e_fpn_conv2_x", 32, 32, K133, relu=True)
    add("e_fpn_conv3_0", 32, 64, K155, S122, relu=True)
    add("e_fpn_conv3_x", 64, 64, K133, relu=True)
    add("e_fpn_inner1", 32, 64, K111, bias=True, skips=(SKIP_UPSAMPLE_ADD,))
    add("e_fpn_out1", 64, 64, K111)
    add("e_fpn_out2", 64, 32, K133)
    add("e_fpn_mid_g", 64, 144, K111)
    add("e_fpn_mid_c", 16, 16, K133, bias=True, skips=(SKIP_ADD,))
    add("e_fpn_tail_g", 64, 72, K111)
    add("e_fpn_tail_c", 8, 8, K133, bias=True, skips=(SKIP_ADD,))
    return fs


def _train_forms():
    """Forward layers of the training step (modules.py forward_cl): no BatchNorm folding, no ReLU, shift = bias."""
    fs = []
    add = lambda *a, **k: fs.append(_form(*a, role="train", **k))
    # FPN4, base 8
    add("t_fpn_conv0_0", 3, 8, K133, cin_pad=4)
    add("t_fpn_conv0_1", 8, 8, K133)
    add("t_fpn_conv1_0", 8, 16, K155, S122)
    add("t_fpn_conv1_x", 16, 16, K133, extra=[(6, 1, 64, 128)])
    add("t_fpn_conv2_0", 16, 32, K155, S122)
    add("t_fpn_conv2_x", 32, 32, K133)
    add("t_fpn_conv3_0", 32, 64, K155, S122)
    add("t_fpn_conv3_x", 64, 64, K133)
    add("t_fpn_out1", 64, 64, K111)
    add("t_fpn_inner1", 32, 64, K111, bias=True, skips=(SKIP_UPSAMPLE_ADD,))
    add("t_fpn_out2", 64, 32, K133)
    add("t_fpn_inner2", 16, 64, K111, bias=True, skips=(SKIP_UPSAMPLE_ADD,))
    add("t_fpn_out3", 64, 16, K133)
    add("t_fpn_fine_g", 64, 72, K111)
    add("t_fpn_fine_c", 8, 8, K133, bias=True, skips=(SKIP_ADD,))
    # reg2d, base 8, G = 8 and 4
    for G in (8, 4):
        add("t_reg2d_conv0_g%d" % G, G, 8, K133, depth=4)
    add("t_reg2d_conv1", 8, 16, K133, S122, depth=4, extra=[(1, 4, 12, 20)])
    add("t_reg2d_conv2", 16, 16, K333, depth=4, extra=[(1, 8, 32, 64)])
    add("t_reg2d_conv3", 16, 32, K133, S122, depth=4)
    add("t_reg2d_conv4", 32, 32, K333, depth=4)
    add("t_reg2d_conv5", 32, 64, K133, S122, depth=4)
    add("t_reg2d_conv6", 64, 64, K333, depth=4)
    add("t_reg2d_conv7", 64, 32, K133, S122, transposed=True, depth=4)
    add("t_reg2d_conv9", 32, 16, K133, S122, transposed=True, depth=4)
    add("t_reg2d_conv11", 16, 8, K133, S122, transposed=True, depth=4)
    # mono depth decoder: conv blocks and the one-channel heads (with bias)
    add("t_mono_block0", 64, 32, K133)
    add("t_mono_block1", 32, 16, K133)
    add("t_mono_block2", 16, 8, K133)
    add("t_mono_head0", 64, 1, K133, bias=True)
    add("t_mono_head1", 32, 1, K133, bias=True)
    add("t_mono_head2", 16, 1, K133, bias=True)
    return fs


# no layer from _ConvCL.backward: the images need no gradient; the gather's 1x1 conv runs inside _FpnGather, whose backward
# builds "d_fpn_fine_g" itself
NO_DGRAD = ("t_fpn_conv0_0", "t_fpn_fine_g")


def _build():
    evals, trains = _eval_forms(), _train_forms()
    dgrads = [dgrad_of(f) for f in trains if f.name not in NO_DGRAD]
    # the input gradient of the finest FPN level's gather: [64, 72] read as 72 -> 64, the gradient's 80-channel pitch
    dgrads.append(_form("d_fpn_fine_g", 72, 64, K111, cin_pad=80, role="dgrad"))
    by_train = {"d_" + f.name[2:]: f for f in trains}
    out = []
    for f in evals:
        out.append(f._replace(ladder=tuple(to_input(f, s) for s in lattice_ladder(f)) + f.ladder))
    for f in trains:
        also = () if f.name in NO_DGRAD else (dgrad_of(f),)
        out.append(f._replace(ladder=tuple(to_input(f, s) for s in lattice_ladder(f, also)) + f.ladder))
    for g in dgrads:
        t = by_train.get(g.name)
        if t is None:
            lad = tuple(lattice_ladder(g))
        else:                               # what the training form's ladder hands its backward pass
            lad = tuple(out_shape(t, s) for s in next(o for o in out if o.name == t.name).ladder)
        out.append(g._replace(ladder=lad))
    return out


FORMS = _build()
BY_NAME = {f.name: f for f in FORMS}
assert len(BY_NAME) == len(FORMS)


def form_key(f):
    """What identifies a form on a built layer (``layer_key``)."""
    return (f.cin, f.cin_pad or f.cin, f.cout, f.kernel, f.stride, f.padding, f.transposed, f.relu, f.prob)


def layer_key(layer):
    return (layer._cin_raw, layer.cin, layer.cout, tuple(layer.kernel), tuple(layer.stride), tuple(layer.padding),
            bool(layer.transposed), bool(layer.relu), layer.prob is not None)


def unique_forms(roles=("eval", "train", "dgrad")):
    """One form per key (the first of its name), with the union of the skip modes and ladders of all forms that share the key."""
    out = collections.OrderedDict()
    for f in FORMS:
        if f.role not in roles:
            continue
        k = form_key(f)
        if k in out:
            g = out[k]
            out[k] = g._replace(skips=tuple(sorted(set(g.skips) | set(f.skips))),
                                ladder=g.ladder + tuple(s for s in f.ladder if s not in g.ladder))
        else:
            out[k] = f
    return list(out.values())


def weight_shape(f):
    return ((f.cin, f.cout) if f.transposed else (f.cout, f.cin)) + f.kernel


def make_layer(f, w, prob=None):
    """A fresh ConvLayer of form ``f`` over weight ``w`` (scale 1, shift 0: the tests set the epilogue themselves)."""
    return cp.ConvLayer(w, f.transposed, f.stride, f.padding, relu=f.relu, cin_pad=f.cin_pad, prob=prob)


# ---- the reference --------------------------------------------------------------------------------------------------------
def conv_ref64(x, w, stride, padding, transposed):
    """x [B, D, H, W, cin] channels-last, w in the nn.Conv3d ([cout, cin, kd, kh, kw]) or nn.ConvTranspose3d ([cin, cout, ...])
    layout -> [B, Do, Ho, Wo, cout] in float64: pad, slice, accumulate x_slice @ w[tap], one tap at a time.  The transposed
    form doubles a stride-2 axis (output_padding = stride - 1), as every transposed layer of the networks does."""
    x, w = x.double(), w.double()
    B, D, H, W, _ = x.shape
    kd, kh, kw = w.shape[2:]
    sd, sh, sw = stride
    pd, ph, pw = padding
    if not transposed:
        xp = F.pad(x, (0, 0, pw, pw, ph, ph, pd, pd))
        Do, Ho, Wo = (D + 2 * pd - kd) // sd + 1, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        y = x.new_zeros(B, Do, Ho, Wo, w.shape[0])
        for z in range(kd):
            for r in range(kh):
                for c in range(kw):
                    xs = xp[:, z:z + (Do - 1) * sd + 1:sd, r:r + (Ho - 1) * sh + 1:sh, c:c + (Wo - 1) * sw + 1:sw]
                    y = y + xs @ w[:, :, z, r, c].t()
        return y
    full = [max((n - 1) * s + k, p + n * s) for n, s, k, p in zip((D, H, W), stride, (kd, kh, kw), padding)]
    y = x.new_zeros(B, full[0], full[1], full[2], w.shape[1])
    for z in range(kd):
        for r in range(kh):
            for c in range(kw):
                y[:, z:z + (D - 1) * sd + 1:sd, r:r + (H - 1) * sh + 1:sh, c:c + (W - 1) * sw + 1:sw] += x @ w[:, :, z, r, c]
    return y[:, pd:pd + D * sd, ph:ph + H * sh, pw:pw + W * sw].contiguous()


def epilogue64(y, scale, shift, relu, skip=None, skip_mode=SKIP_NONE, prob=None):
    """The kernels' fused epilogue in float64: y * scale + shift, ReLU, + skip (same shape, or the bilinear x2 align_corners
    up-sampling of a half-resolution map), then the 8 -> 1 head."""
    y = y * scale.double() + shift.double()
    if relu:
        y = y.clamp_min(0)
    if skip_mode == SKIP_ADD:
        y = y + skip.double()
    elif skip_mode == SKIP_UPSAMPLE_ADD:
        s = skip.double()[:, 0].permute(0, 3, 1, 2)
        up = F.interpolate(s, size=(y.shape[2], y.shape[3]), mode="bilinear", align_corners=True)
        y = y + up.permute(0, 2, 3, 1).unsqueeze(1)
    if prob is not None:
        y = y @ prob[0].double() + prob[1].double()
    return y


# ---- test data -------------------------------------------------------------------------------------------------------------
SCALES = (0.5, 1.0, 2.0)


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _ints(shape, lo, hi, g, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()


def case_data(f, shape, device, exact, seed=0):
    """Operands of one eval-role call: x (all ``cin_pad`` channels filled: the padded ones meet zero weights), w, scale, shift,
    the skips for every mode the form allows and the prob head.  ``exact``: integers (x, w, skip in {-2..2}, scale in
    {0.5, 1, 2}, integer shift and head), so that every partial sum of any kernel is exact in float32; otherwise normal
    operands as in test_conv_bn_relu / test_winograd_conv_against_fp64_and_direct."""
    device = torch.device(device)
    g = _gen(device, 1000 * seed + sum(map(ord, f.name)) + 7 * sum(shape) + (1 if exact else 0))
    cin_k = f.cin_pad or f.cin
    oshape = out_shape(f, shape)
    d = {}
    if exact:
        d["x"] = _ints(tuple(shape) + (cin_k,), -2, 2, g, device)
        d["w"] = _ints(weight_shape(f), -2, 2, g, device)
        d["scale"] = torch.tensor(SCALES, device=device)[torch.randint(0, 3, (f.cout,), generator=g, device=device)]
        d["shift"] = _ints((f.cout,), -3, 3, g, device)
        d["prob"] = (_ints((8,), -2, 2, g, device), _ints((1,), -3, 3, g, device)) if f.prob else None
        mk = lambda s: _ints(s, -2, 2, g, device)
    else:
        rn = lambda s: torch.randn(s, generator=g, device=device)
        d["x"] = rn(tuple(shape) + (cin_k,))
        d["w"] = rn(weight_shape(f)) * 0.1
        d["scale"] = torch.rand(f.cout, generator=g, device=device) + 0.5
        d["shift"] = rn((f.cout,)) * 0.1
        d["prob"] = (rn((8,)), rn((1,))) if f.prob else None
        mk = rn
    d["skip"] = {}
    for sm in f.skips:
        if sm == SKIP_ADD:
            d["skip"][sm] = mk(oshape + (f.cout,))
        elif sm == SKIP_UPSAMPLE_ADD:
            d["skip"][sm] = mk((oshape[0], 1, oshape[2] // 2, oshape[3] // 2, f.cout))
    return d


def reduction_length(f):
    """K of one output element: taps x input channels (a transposed layer's largest parity class has ceil(k / s) taps an axis)."""
    if f.transposed:
        taps = 1
        for k, s in zip(f.kernel, f.stride):
            taps *= -(-k // s)
    else:
        taps = f.kernel[0] * f.kernel[1] * f.kernel[2]
    return taps * f.cin


def exact_budget(f):
    """Largest magnitude any float32 intermediate of an exact case can reach, in units of its smallest step (0.5)."""
    acc = reduction_length(f) * 2 * 2                   # |x| <= 2, |w| <= 2
    y = acc * max(SCALES) + 3 + 2                       # scale, shift, skip
    if f.prob:
        y = 8 * 2 * y + 3
    return 2 * y                                        # half-integers: count in halves


# ---- what a choice must dispatch ---------------------------------------------------------------------------------------------
FAMILY_PREFIX = {0: ("conv_mfma_kernel<",), 1: ("conv_lds_kernel<",), 2: ("conv_mfma_kernel<",), 3: ("conv_small_kernel<",),
                 4: ("deconv_small_kernel<",), 5: ("conv_pers_kernel<", "conv_tpers_kernel<", "conv_pers8_kernel<"),
                 6: ("conv1x1_pers_kernel<",), 8: ("conv_wino_kernel<",), 9: ("conv_wino_ring_kernel<",),
                 10: ("conv_narrow_kernel<",)}


def effective_choice(layer, shape, skip_mode):
    """(variant word, mt, nt, how) of ``layer(x)`` without ``tiles``: ``_geom``'s choice after ``__call__``'s own adjustment (the
    LDS / narrow kernels have no fused head: such a layer runs the direct kernel).  how = "exact" | "family" | ... when the
    final choice is the measured table's, else "rule"."""
    _, mt, nt, _, variant = layer._geom(*shape, skip_mode)
    tuned, how = cp.tuned_choice(layer, *shape, skip_mode) if cp.FORCE_VARIANT is None else (None, None)
    if not tuned or [variant, mt, nt] != list(tuned):
        how = "rule"
    if variant != 4 and layer.prob is not None and variant in (1, 3, 10):
        variant, how = 0, "rule"
    return variant, mt, nt, how


def names_family(name, variant):
    """Does kernel ``name`` (``_lib.last_kernel()``) belong to the family of variant word ``variant``?"""
    fam = variant & 0xff
    if not name.startswith(FAMILY_PREFIX[fam]):
        return False
    if fam in (0, 2):
        return name.endswith(", true>" if fam == 2 else ", false>")
    return True


def is_direct_fallback(name, variant):
    """The library answered "unsupported" and ``__call__`` ran the direct kernel instead."""
    return (variant & 0xff) != 0 and name.startswith("conv_mfma_kernel<") and name.endswith(", false>")
