"""Scenes for the warp backward (csrc/warp_bwd.hip) whose sampling positions are EXACT in fp32, and the fp64 reference.

``mv::project`` and ``grid_roundtrip`` (csrc/mvster_math.h) give the same number in fp32 and in fp64 when
  * the source map has Hs - 1 and Ws - 1 powers of two (17 x 33, 33 x 65 here; 33 x 129 for ``window_edge``, whose 96-texel
    window does not fit into 65 columns),
  * ``rt`` has r[6] = r[7] = 0, r[8] = 1, r[0..5] small integers or halves, t_x / t_y multiples of 1/4, t_z = 0,
  * every hypothesis is one of 1, 2, 4, 8, chosen per (pixel, d):
then pz is a power of two, px / pz is dyadic with few fractional bits, and every operation of the chain is exact
(tests/test_warp_exact_cpu.py checks this bit for bit per scene).  The bilinear weights are then exact too, so an fp64
restatement of the stage is an oracle of the kernel's ARITHMETIC, not of its coordinate noise, and every edge of the kernel
file (tile corners of the sorted scatter, the last column of a scatter window, taps at x0 = -1 ...) can be placed on purpose.

``bad_depth`` leaves the construction on purpose (t_z = -2, depths from {1, 2, 3, 4, 6, 10}, NaN depths): pz is still a power
of two, -1 or 0; where pz == 0 the position is px / 1e-9, which is not exact but lands on 0 or beyond the clamp of
``make_taps`` -- positions are therefore compared after that clamp.

The module is plain torch: ``aggregate`` runs in fp64 on the CPU (the reference) and, the same code, in fp32 on the device
(the baseline whose error calibrates the tests' bound)."""
import collections
import functools
import math
import zlib

import numpy as np
import torch

ATTN_TEMP = 2.0
REC_TILE_X, REC_TILE_Y = 32, 16              # source tiles of the sorted scatter (kRecTileX, kRecTileY)
ROW_WIN = (96, 6)                            # kWinX, kWinY: the row kernel's scatter window, one per 64 consecutive pixels
TILE_WIN = (80, 10)                          # kTileWinX, kTileR + 6: the tile kernel's, one per 64 columns x 4 rows
TILE_R = 4
QUEUE_DIRECT = 4                             # kQueueDirect
EMPTY = 0x7fffffff                           # window origin of a workgroup and view without a weighted tap
PZ_ZERO = float(np.float32(1e-9))            # what project() puts in place of pz == 0

Scene = collections.namedtuple("Scene", "name B NV h w Hs Ws D rt hypo facts")
Config = collections.namedtuple("Config", "name C G D group fuse")


# ---- positions, taps ---------------------------------------------------------------------------------------------------
def positions(rt, hypo, Hs, Ws, dtype):
    """Sampling positions [B, NV, D, h, w] of ``mv::project``, operation by operation in ``dtype`` (rt [B, NV, 12] = r[9], t[3];
    hypo [B, D, h, w]), BEFORE the clamp of make_taps."""
    B, D, h, w = hypo.shape
    NV = rt.shape[1]
    dev = rt.device
    r = rt.to(dtype)
    dep = hypo.to(dtype).view(B, 1, D, h, w)
    y = torch.arange(h, dtype=dtype, device=dev).view(1, 1, 1, h, 1)
    x = torch.arange(w, dtype=dtype, device=dev).view(1, 1, 1, 1, w)

    def k(i):
        return r[:, :, i].reshape(B, NV, 1, 1, 1)
    rx = (k(1) * y + k(0) * x) + k(2)
    ry = (k(4) * y + k(3) * x) + k(5)
    rz = (k(7) * y + k(6) * x) + k(8)
    px = rx * dep + k(9)
    py = ry * dep + k(10)
    pz = rz * dep + k(11)
    pz = torch.where(pz == 0, torch.full_like(pz, PZ_ZERO), pz)

    def roundtrip(pix, size):
        g = pix / ((size - 1) / 2.0) - 1.0
        return ((g + 1.0) / 2.0) * float(size - 1)
    return roundtrip(px / pz, Ws), roundtrip(py / pz, Hs)


def clamp_position(s, size):
    """make_taps' clamp: fminf / fmaxf drop a NaN operand, so NaN -> size + 4; beyond one texel outside only zeros are sampled"""
    return torch.where(s.isnan(), torch.full_like(s, float(size + 4)), s.clamp(-4.0, float(size + 4)))


Taps = collections.namedtuple("Taps", "x0 y0 wgt xs ys mask")


def make_taps(sx, sy, Hs, Ws):
    """make_taps + clamp_taps: corner by floor, four weights (nw, ne, sw, se) with the zeros padding applied per tap, the
    clamped tap coordinates and the mask of taps that carry weight.  A non-finite position samples zeros."""
    cx, cy = clamp_position(sx, Ws), clamp_position(sy, Hs)
    fx, fy = cx.floor(), cy.floor()
    wx1, wy1 = cx - fx, cy - fy
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    x0, y0 = fx.long(), fy.long()
    wgt, xs, ys = [], [], []
    mask = torch.zeros_like(x0)
    for t, (dy, dx, wt) in enumerate(((0, 0, wy0 * wx0), (0, 1, wy0 * wx1), (1, 0, wy1 * wx0), (1, 1, wy1 * wx1))):
        tx, ty = x0 + dx, y0 + dy
        ok = (tx >= 0) & (tx < Ws) & (ty >= 0) & (ty < Hs)
        wt = torch.where(ok, wt, torch.zeros_like(wt))
        wgt.append(wt)
        xs.append(tx.clamp(0, Ws - 1))
        ys.append(ty.clamp(0, Hs - 1))
        mask = mask | ((wt != 0).long() << t)
    return Taps(x0, y0, wgt, xs, ys, mask)


def scene_taps(sc, dtype=torch.float64):
    sx, sy = positions(sc.rt, sc.hypo, sc.Hs, sc.Ws, dtype)
    return make_taps(sx, sy, sc.Hs, sc.Ws)


# ---- the stage, with explicit taps ----------------------------------------------------------------------------------------
def aggregate(ref, src, rt, hypo, G, group, fuse, temp=ATTN_TEMP, dtype=torch.float64):
    """ref [B,h,w,C], src [NV,B,Hs,Ws,C], rt [B,NV,12], hypo [B,D,h,w] -> (out [B,D,h,w,G], wsum [B,D,h,w]) in ``dtype`` on the
    operands' device: bilinear taps with zeros padding, group correlation or squared differences, a softmax weight per view
    over the depth axis (``fuse``: per (pixel, d), divided by sqrt(C); otherwise the largest softmax value of the pixel), the
    weighted mean over the views with 1e-8 in the weight sum.  Differentiable in ``ref`` and ``src``."""
    B, h, w, C = ref.shape
    NV, _, Hs, Ws, _ = src.shape
    D = hypo.shape[1]
    sx, sy = positions(rt, hypo, Hs, Ws, dtype)
    tp = make_taps(sx, sy, Hs, Ws)
    refv = ref.to(dtype).view(B, 1, h, w, C)
    boff = (torch.arange(B, device=ref.device) * (Hs * Ws)).view(B, 1, 1, 1)
    wsum = 1e-8
    acc = 0
    for v in range(NV):
        flat = src[v].to(dtype).reshape(B * Hs * Ws, C)
        warped = 0
        for t in range(4):
            idx = boff + tp.ys[t][:, v] * Ws + tp.xs[t][:, v]
            warped = warped + flat[idx] * tp.wgt[t][:, v].unsqueeze(-1)
        if group:
            cor = (warped.view(B, D, h, w, G, C // G) * refv.view(B, 1, h, w, G, C // G)).mean(-1)
        else:
            cor = (refv - warped) ** 2
        if fuse:
            wgt = torch.softmax(cor.sum(-1) / temp, 1) / math.sqrt(C)
        else:
            sm = torch.softmax(cor.sum(-1), 1)
            # the FIRST maximum along depth, spelled out: the kernel's choice on ties (a scene with equal hypotheses)
            top = sm == sm.max(1, keepdim=True)[0]
            first = top & (top.cumsum(1) == 1)
            wgt = (sm * first.to(dtype)).sum(1, keepdim=True).expand(B, D, h, w)
        wsum = wsum + wgt
        acc = acc + wgt.unsqueeze(-1) * cor
    return acc / wsum.unsqueeze(-1), wsum


def gradients(ref, src, rt, hypo, gout, cfg, dtype, device=None):
    """(out, wsum, g_ref, g_src) of ``aggregate`` through autograd, in ``dtype`` on ``device``, returned as fp64 CPU tensors"""
    dev = device or torch.device("cpu")
    r = ref.to(dev, dtype).requires_grad_(True)
    s = src.to(dev, dtype).requires_grad_(True)
    out, wsum = aggregate(r, s, rt.to(dev), hypo.to(dev), cfg.G if cfg.group else cfg.C, cfg.group, cfg.fuse, dtype=dtype)
    out.backward(gout.to(dev, dtype))
    return tuple(t.detach().cpu().double() for t in (out, wsum, r.grad, s.grad))


# ---- what the kernels' accumulators see ---------------------------------------------------------------------------------
def contributions(sc):
    """n_src [NV, B, Hs, Ws]: the number of (pixel, d) samples with a WEIGHTED tap on the texel -- the additions its fixed-point
    counter receives per channel.  (The reference gradient of a pixel receives D * NV.)"""
    tp = scene_taps(sc)
    n = torch.zeros(sc.NV, sc.B, sc.Hs * sc.Ws, dtype=torch.long)
    for t in range(4):
        idx = (tp.ys[t] * sc.Ws + tp.xs[t]).permute(1, 0, 2, 3, 4).reshape(sc.NV, sc.B, -1)
        n.scatter_add_(2, idx, (tp.wgt[t] != 0).long().permute(1, 0, 2, 3, 4).reshape(sc.NV, sc.B, -1))
    return n.view(sc.NV, sc.B, sc.Hs, sc.Ws)


def touched_tiles(sc):
    """[B, NV, D, h, w]: how many 32 x 16 source tiles hold a weighted tap of the sample (= records the sorted scatter writes)"""
    tp = scene_taps(sc)
    tiles_x = -(-sc.Ws // REC_TILE_X)
    ids = [torch.where(tp.wgt[t] != 0, (tp.ys[t] // REC_TILE_Y) * tiles_x + tp.xs[t] // REC_TILE_X, torch.full_like(tp.x0, -1 - t))
           for t in range(4)]
    ids = torch.stack(ids, -1)
    count = torch.zeros_like(tp.x0)
    for t in range(4):
        fresh = ids[..., t] >= 0
        for u in range(t):
            fresh = fresh & (ids[..., t] != ids[..., u])
        count = count + fresh.long()
    return count


Windows = collections.namedtuple("Windows", "origin cover outside edge")


def windows(sc, kind):
    """The scatter windows of the first-pass kernels, restated: ``kind`` = "row" (workgroup = 64 consecutive pixels x all d, 96 x
    6 texels) or "tile" (64 columns x 4 rows x all d, 80 x 10).  A window is anchored at the smallest clamped corner (xa, ya)
    over the workgroup's samples that carry weight, per view.
      origin  [B, nblk, NV, 2]   (EMPTY where the workgroup has no weighted tap in the view)
      cover   [NV, B, Hs, Ws]    windows that cover the texel (inside the map)
      outside list of (b, v, workgroup, wavefront, tap, lanes): wavefronts with >= 1 lane whose weighted tap falls outside
      edge    set of (ax, ay) window coordinates of weighted taps, clipped to [-1, WX] x [-1, WY]"""
    WX, WY = ROW_WIN if kind == "row" else TILE_WIN
    tp = scene_taps(sc)
    B, NV, D, h, w = sc.B, sc.NV, sc.D, sc.h, sc.w
    xs = [t.numpy() for t in tp.xs]
    ys = [t.numpy() for t in tp.ys]
    wt = [(t != 0).numpy() for t in tp.wgt]
    anyw = wt[0] | wt[1] | wt[2] | wt[3]
    if kind == "row":
        # one wavefront per d: its lanes are the workgroup's pixels
        blocks = [[(np.arange(p0, min(p0 + 64, h * w)) // w, np.arange(p0, min(p0 + 64, h * w)) % w)] for p0 in range(0, h * w, 64)]
    else:
        # one wavefront per (row, d); workgroups numbered row-major over (tile row, tile column)
        blocks = []
        for y0 in range(0, h, TILE_R):
            for x0 in range(0, w, 64):
                cols = np.arange(x0, min(x0 + 64, w))
                blocks.append([(np.full(len(cols), y), cols) for y in range(y0, min(y0 + TILE_R, h))])
    origin = np.full((B, len(blocks), NV, 2), EMPTY, dtype=np.int64)
    cover = np.zeros((NV, B, sc.Hs, sc.Ws), dtype=np.int64)
    outside, edge = [], set()
    for b in range(B):
        for v in range(NV):
            for k, waves in enumerate(blocks):
                yy = np.concatenate([wv[0] for wv in waves])
                xx = np.concatenate([wv[1] for wv in waves])
                sel = anyw[b, v][:, yy, xx]
                if not sel.any():
                    continue
                ox = xs[0][b, v][:, yy, xx][sel].min()
                oy = ys[0][b, v][:, yy, xx][sel].min()
                origin[b, k, v] = (ox, oy)
                cover[v, b, oy:oy + WY, ox:ox + WX] += 1
                for r, (wy_, wx_) in enumerate(waves):
                    for d in range(D):
                        for t in range(4):
                            ax = xs[t][b, v, d, wy_, wx_] - ox
                            ay = ys[t][b, v, d, wy_, wx_] - oy
                            on = wt[t][b, v, d, wy_, wx_]
                            out = on & ~((ax >= 0) & (ax < WX) & (ay >= 0) & (ay < WY))
                            if out.any():
                                outside.append((b, v, k, r * D + d, t, int(out.sum())))
                            if on.any():
                                pts = np.stack((np.clip(ax[on], -1, WX), np.clip(ay[on], -1, WY)), 1)
                                edge.update(map(tuple, np.unique(pts, axis=0).tolist()))
    return Windows(origin, torch.from_numpy(cover), outside, edge)


def fix_bound(gomax, refmax, srcmax, cfg):
    """``bound`` of make_fix_scale (csrc/warp_bwd.hip), restated from its comment: the largest single contribution to a
    fixed-point counter, from the operand maxima.  One unit of the counters is the largest power of two <= bound * 2^-36."""
    fmax = max(refmax, srcmax)
    G = cfg.G if cfg.group else cfg.C
    cormax = fmax * fmax if cfg.group else 4.0 * fmax * fmax
    dcor = gomax * (1.0 + 2.0 * G * (1 + cfg.D) * cormax / (ATTN_TEMP if cfg.fuse else 1.0))
    return dcor * fmax / (cfg.C // G) if cfg.group else 4.0 * fmax * dcor


def first_pass_kernel(cfg, form):
    """The name ``_lib.last_kernel()`` reports after ops.warp_agg_bwd_cl (the first pass; the later passes note nothing)"""
    G = cfg.G if cfg.group else cfg.C
    gr = "true" if cfg.group else "false"
    dmax = 8 if cfg.D <= 8 else 16
    if form == "sorted":
        return "warp_agg_bwd_kernel<%d, %d, %s, %d, true>" % (cfg.C, G, gr, dmax)
    if uses_tiles(cfg):
        return "warp_agg_bwd_tile_kernel<%d, %s, %d, %d>" % (G, gr, TILE_R, 4 if cfg.D <= 4 else 8)
    return "warp_agg_bwd_kernel<%d, %d, %s, %d>" % (cfg.C, G, gr, dmax)


def uses_tiles(cfg):
    return cfg.C == 8 and cfg.fuse and cfg.D <= 8


# ---- the scenes -------------------------------------------------------------------------------------------------------------
def _rt(rows):
    """rows[b][v] = (r0, r1, r2, r3, r4, r5, tx, ty[, tz]) -> rt [B, NV, 12]"""
    out = torch.zeros(len(rows), len(rows[0]), 12, dtype=torch.float32)
    for b, views in enumerate(rows):
        for v, m in enumerate(views):
            out[b, v, :6] = torch.tensor(m[:6])
            out[b, v, 8] = 1.0
            out[b, v, 9], out[b, v, 10] = m[6], m[7]
            out[b, v, 11] = m[8] if len(m) > 8 else 0.0
    return out


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _random_hypo(name, B, D, h, w, values=(1.0, 2.0, 4.0, 8.0)):
    vals = torch.tensor(values)
    return vals[torch.randint(0, len(values), (B, D, h, w), generator=_gen(name))]


def shift(D):
    """dyadic translations: interior, fractional footprints; the two batch items see different cameras"""
    rt = _rt([[(1, 0, 3, 0, 1, 2, 2.5, 0.25), (1, 0, 5.5, 0, 1, 4.5, -1.75, 0.25)],
              [(1, 0, 1.5, 0, 1, 5, 4.25, -0.25), (1, 0, 7, 0, 1, 3.5, 0.75, 0.25)]])
    return Scene("shift", 2, 2, 9, 23, 17, 33, D, rt, _random_hypo("shift", 2, D, 9, 23), {})


def integer(D):
    """every position on integer coordinates, x0 = Ws - 1 and y0 = Hs - 1 included: three zero-weight taps, tap mask 1"""
    rt = _rt([[(1, 0, 10, 0, 1, 8, 0, 0), (1, 0, 0, 0, 1, 0, 8, 8)]])
    return Scene("integer", 1, 2, 9, 23, 17, 33, D, rt, _random_hypo("integer", 1, D, 9, 23), {})


def border(D):
    """positions from -1.5 to Ws + 0.5 and likewise in y: all four map corners, x0 in {-2, -1, Ws - 1, Ws}"""
    rt = _rt([[(0.5, 0, -1.5, 0, 2, -0.5, 0.5, 0.25), (0.5, 0, -1, 0, 2, -2, 0, 0)],
              [(0.5, 0, -2, 0, 1.5, -1.5, 1.0, 0), (0.5, 0, -1.5, 0, 2, -1.5, 0.25, 0.5)]])
    return Scene("border", 2, 2, 12, 70, 17, 33, D, rt, _random_hypo("border", 2, D, 12, 70), {})


def tile_corner(D):
    """footprints straddling the corners of the sorted scatter's 32 x 16 source tiles: in x only, in y only, in both; the
    33 x 65 map has a ragged third tile column and row, one texel wide"""
    rt = _rt([[(1, 0, -3, 0, 1, 10, 2.0, 1.0), (1, 0, -4.5, 0, 2, 5.5, 0, 0)],
              [(1, 0, -2, 0, 1, 21, 0.5, 0.5), (0.5, 0, 14.5, 0, 0.5, 12.5, 1.0, 2.0)]])
    return Scene("tile_corner", 2, 2, 12, 70, 33, 65, D, rt, _random_hypo("tile_corner", 2, D, 12, 70), {})


def minify(D):
    """r = diag(1/2, 1/2, 1): neighbouring reference pixels share a footprint"""
    rt = _rt([[(0.5, 0, 0, 0, 0.5, 0, 1.0, 0.5), (0.5, 0, 3, 0, 0.5, 8, 0, 0), (0.5, 0, 20.5, 0, 0.5, 20.5, 0.25, 0.25)]])
    return Scene("minify", 1, 3, 12, 70, 33, 65, D, rt, _random_hypo("minify", 1, D, 12, 70), {})


def collapse(D):
    """r[0..5] = 0 and one hypothesis throughout: every sample of a view lands on ONE footprint -- view 0 inside a tile, view 1 on
    a tile corner (four records per sample: the record lists' worst case); a texel receives h * w * D contributions"""
    rt = _rt([[(0, 0, 0, 0, 0, 0, 10.5, 6.5), (0, 0, 0, 0, 0, 0, 63.0, 31.0)],
              [(0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 5.0, 31.5)]])
    hypo = torch.full((2, D, 16, 16), 2.0)
    return Scene("collapse", 2, 2, 16, 16, 17, 33, D, rt, hypo, {})


def transpose(D):
    """x and y swapped: a reference row walks down a source column, most taps leave the scatter window"""
    rt = _rt([[(0, 1, 2.5, 1, 0, 1.5, 1.0, 0.5), (0, 1, 40, 1, 0, 4, 0, 0)]])
    return Scene("transpose", 1, 2, 9, 23, 33, 65, D, rt, _random_hypo("transpose", 1, D, 9, 23), {})


def stragglers(D):
    """smooth (hypotheses 8 and 4 by d), except for columns 3 and 17, whose hypothesis 1 throws them 12 or more rows down: 1 or
    2 lanes of a wavefront outside the window, never more than 4"""
    rt = _rt([[(1, 0, 2, 0, 1, 0.5, 8.0, 16.0), (1, 0, 0.5, 0, 1, 1, 4.0, 16.0)]])
    hypo = torch.empty(1, D, 12, 70)
    for d in range(D):
        hypo[:, d] = 8.0 if d % 2 == 0 else 4.0
    hypo[:, :, :, 3] = 1.0
    hypo[:, :, :, 17] = 1.0
    return Scene("stragglers", 1, 2, 12, 70, 33, 65, D, rt, hypo, {})


def window_edge(D):
    """weighted taps exactly in the last column / row of a scatter window and exactly one past it, for the 96 x 6 and the 80 x 10
    window: hypothesis 8 except in column 5 (2: four source rows down) and columns 23 and 39 (1: 56 columns to the right)"""
    rt = _rt([[(1, 0, 0.5, 0, 2, 0.5, 64.0, 0), (1, 0, 0.5, 0, 2, 0.5, 0, 8.0)]])
    hypo = torch.full((1, D, 12, 70), 8.0)
    hypo[:, 0::2, :, 5] = 2.0
    hypo[:, 0::2, :, 23] = 1.0
    hypo[:, 0::2, :, 39] = 1.0
    hypo[:, 1::2, 1::2, 9] = 1.0
    return Scene("window_edge", 1, 2, 12, 70, 33, 129, D, rt, hypo, {})


def empty_view(D):
    """view 1 lies wholly outside the map: its workgroups keep the window origin 0x7fffffff, its gradient is exactly zero"""
    rt = _rt([[(1, 0, 3, 0, 1, 2, 2.5, 1.25), (1, 0, 100, 0, 1, 2, 0, 0)],
              [(1, 0, 1.5, 0, 1, 5, 4.0, -2.25), (1, 0, 0, 0, 1, -40, 0.5, 0.5)]])
    return Scene("empty_view", 2, 2, 9, 23, 17, 33, D, rt, _random_hypo("empty_view", 2, D, 9, 23), {"empty": 1})


def bad_depth(D):
    """t_z = -2 with depths from {1, 2, 3, 4, 6, 10}: pz in {-1, 0, 1, 2, 4, 8}.  pz == 0 samples: column 4 of rows 0..3 at d = 0
    (px == 0 in view 0; at row 3 py == 0 too: the sample sits on texel (0, 0)), 6 NaN depths"""
    rt = _rt([[(1, 0, -4, 0, 1, -3, 0, 0, -2.0), (1, 0, 2, 0, 1, 1, 0.5, 0.25, -2.0)]])
    hypo = _random_hypo("bad_depth", 1, D, 9, 23, (1.0, 3.0, 4.0, 6.0, 10.0))
    hypo[0, 0, 0:4, 4] = 2.0
    hypo[0, D - 1, 5, 7:10] = 2.0
    nan = float("nan")
    hypo[0, 0, 8, 20:23] = nan
    hypo[0, D - 1, 2, 0:3] = nan
    return Scene("bad_depth", 1, 2, 9, 23, 17, 33, D, rt, hypo, {"pz_zero": 7 * 2, "nan": 6 * 2})


SCENES = {f.__name__: f for f in (shift, integer, border, tile_corner, minify, collapse, transpose, stragglers, window_edge,
                                  empty_view, bad_depth)}

CONFIGS = [
    Config("c8g4d4", 8, 4, 4, True, True),            # tile kernel, NW = 4
    Config("c8g8d8", 8, 8, 8, True, True),            # tile kernel, NW = 8
    Config("c8g4d4nf", 8, 4, 4, True, False),         # row kernel at C = 8
    Config("c8g4d12", 8, 4, 12, True, True),          # row kernel, kMaxD instance
    Config("c16g4d4", 16, 4, 4, True, True),          # GREF_REG
    Config("c32g8d8", 32, 8, 8, True, True),          # KEEP_WV upper end
    Config("c64g8d8", 64, 8, 8, True, True),          # re-gather, LDS gref
    Config("c64g4d4", 64, 4, 4, True, True),
    Config("sq16d4", 16, 16, 4, False, True),         # squared differences: GO_REG off
    Config("sq64d3", 64, 64, 3, False, True),         # ... and D = 3
    Config("c16g4d3nf", 16, 4, 3, True, False),
]
CONFIG = {c.name: c for c in CONFIGS}
ON_ALL = ("tile_corner", "border", "collapse")
ON_SOME = {
    "shift": ("c8g4d4", "c64g8d8", "c16g4d3nf"),
    "integer": ("c8g8d8", "c16g4d4"),
    "minify": ("c8g4d4", "c32g8d8"),
    "transpose": ("c8g4d4", "c8g4d4nf", "sq16d4"),
    "stragglers": ("c8g4d4", "c8g4d12", "c16g4d4"),
    "window_edge": ("c8g4d4", "c8g4d4nf", "c32g8d8"),
    "empty_view": ("c8g8d8", "c64g4d4"),
    "bad_depth": ("c8g4d4", "sq64d3", "c16g4d4"),
}
CASES = [(s, c.name) for s in ON_ALL for c in CONFIGS] + [(s, c) for s, cs in ON_SOME.items() for c in cs]
IDS = ["%s-%s" % sc for sc in CASES]


@functools.lru_cache(maxsize=None)
def scene(name, D):
    return SCENES[name](D)


def operands(sc, cfg, tail=False):
    """unit-variance ref [B,h,w,C], src [NV,B,Hs,Ws,C] and grad_out [B,D,h,w,G]; ``tail``: one reference and one source texel
    (channel 0 of the middle pixel / of a texel the first sample of view 0 touches) set to 64"""
    g = _gen(sc.name + cfg.name)
    ref = torch.randn(sc.B, sc.h, sc.w, cfg.C, generator=g)
    src = torch.randn(sc.NV, sc.B, sc.Hs, sc.Ws, cfg.C, generator=g)
    gout = torch.randn(sc.B, sc.D, sc.h, sc.w, cfg.G if cfg.group else cfg.C, generator=g)
    if tail:
        ref[0, sc.h // 2, sc.w // 2, 0] = 64.0
        tp = scene_taps(sc)
        k = int((tp.mask[0, 0] != 0).flatten().nonzero()[0])
        t = int(tp.mask[0, 0].flatten()[k]).bit_length() - 1
        src[0, 0, int(tp.ys[t][0, 0].flatten()[k]), int(tp.xs[t][0, 0].flatten()[k]), 0] = 64.0
    return ref, src, gout


@functools.lru_cache(maxsize=None)
def reference(scene_name, cfg_name, tail=False):
    """(scene, config, ref, src, gout, (out, wsum, g_ref, g_src) in fp64) of a case; computed once, shared, not to be modified"""
    cfg = CONFIG[cfg_name]
    sc = scene(scene_name, cfg.D)
    ref, src, gout = operands(sc, cfg, tail)
    return sc, cfg, ref, src, gout, gradients(ref, src, sc.rt, sc.hypo, gout, cfg, torch.float64)
