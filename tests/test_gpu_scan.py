"""Scan-level inference on the GPU (mvster_amd.scan): the two new kernels bit for bit against the forms they restate, the
whole path bit for bit against the per-sample forward, FPN run count, folder round trip into fusion, timing report."""
import json
import math
import os
import statistics

import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, _lib, filter_depth, ops, scan
from mvster_amd.synthetic import make_inputs
from tests import scan_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(shipped_cfg, checkpoint):
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    return m.to(DEV).eval()


# ---- 5: 8-bit images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H,W", [(7, 128, 192), (1, 512, 640), (3, 5, 7)])
def test_pack_images_u8_equals_pack_images_of_read_img_floats(V, H, W):
    rng = np.random.RandomState(V * H)
    u8 = rng.randint(0, 256, size=(V, H, W, 3)).astype(np.uint8)
    u8[0, 0, :min(W, 256), 0] = np.arange(min(W, 256))                       # every level at least once where W allows
    floats = u8.astype(np.float32) / 255.0                                   # read_img (general_eval4.py:81-86)
    want = ops.pack_images([torch.from_numpy(np.ascontiguousarray(f.transpose(2, 0, 1)))[None].to(DEV) for f in floats])
    got = ops.pack_images_u8(torch.from_numpy(u8).to(DEV))
    assert got.shape == want.shape == (V, 1, H, W, 4) and got.dtype == torch.float32
    assert torch.equal(got, want)


# ---- 6: indexed warp ---------------------------------------------------------------------------------------------------
SHIPPED_STAGES = [(64, 8, 8, True, True, 0), (32, 8, 8, True, True, 0), (16, 4, 4, True, True, 0), (8, 4, 4, True, True, 0)]
# one non-shipped shape per remaining launch form the product library accepts: wave-local at another (C, G, D); lane split
# (variant 2), indexed and gathered; one thread per (pixel, d) (variant 1) grouped / squared difference, indexed (C != 16)
# and gathered (C = 16); D > 8 and > 16 (1024-thread forms); attention without the depth fusion
OTHER_FORMS = [(16, 8, 4, True, True, 3), (32, 4, 8, True, False, 0), (32, 8, 8, True, True, 2), (64, 8, 4, True, True, 2),
               (16, 4, 8, True, True, 2), (8, 4, 8, True, True, 1), (16, 4, 4, True, True, 1), (8, 8, 6, False, True, 0),
               (16, 16, 5, False, False, 0), (32, 32, 8, False, True, 0), (64, 4, 12, True, True, 0), (8, 4, 40, True, True, 0),
               (32, 8, 17, True, False, 0)]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C,G,D,gc,fuse,variant", SHIPPED_STAGES + OTHER_FORMS)
def test_indexed_warp_equals_plain_warp_on_gathered_copy(C, G, D, gc, fuse, variant, B):
    h, w, V, NV = 24, 40, 6, 4
    g = torch.Generator().manual_seed(C * 100 + D + B)
    store = torch.randn(V, h, w, C, generator=g).to(DEV)
    _, proj, dv = make_inputs(nviews=NV + 1, H=h * 8, W=w * 8, batch=B, seed=D, rotate=True)
    rt = ops.relative_projection(proj["stage1"].to(DEV))
    hypo = (dv[:, :1, None, None] + (dv[:, -1:, None, None] - dv[:, :1, None, None]) * torch.rand(B, D, h, w, generator=g)).to(DEV)
    table = [[3, 1, 1, 5, 0], [2, 4, 0, 3, 2]][:B]                           # a repeated index in each row
    idx = torch.tensor(table)
    ref = store[idx[:, 0]].contiguous()
    src = store[idx[:, 1:].t().reshape(-1)].view(NV, B, h, w, C).contiguous()
    want, want_ws = ops.warp_agg_fwd_cl(ref, src, rt, hypo, G, gc, fuse, 2.0, want_wsum=True, variant=variant)
    plain_kernel = _lib.last_kernel()
    got, got_ws = ops.warp_agg_fwd_indexed_cl(store, table, rt, hypo, G, gc, fuse, 2.0, want_wsum=True, variant=variant)
    # the same kernel (its indexed instantiation, or the plain one after the gather), not merely the same numbers
    assert _lib.last_kernel().replace(", 0, true>", ">").replace(", true>", ">") == plain_kernel
    if (C, G, D, variant) in [(s[0], s[1], s[2], s[5]) for s in SHIPPED_STAGES]:
        assert _lib.last_kernel() == "warp_agg_fwd_wave_kernel<%d, %d, %d, 0, true>" % (C, G, D)     # truly indexed
    assert torch.equal(got, want) and torch.equal(got_ws, want_ws)
    # a device table is taken as it is
    dev_table = torch.tensor(table, dtype=torch.int32, device=DEV)
    assert torch.equal(ops.warp_agg_fwd_indexed_cl(store, dev_table, rt, hypo, G, gc, fuse, 2.0, variant=variant), want)


def test_indexed_warp_rejects_bad_tables():
    store = torch.zeros(3, 8, 8, 8, device=DEV)
    rt, hypo = torch.zeros(1, 2, 12, device=DEV), torch.ones(1, 4, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="view index 3"):
        ops.warp_agg_fwd_indexed_cl(store, [[0, 1, 3]], rt, hypo, 4)
    with pytest.raises(RuntimeError, match="int32"):
        ops.warp_agg_fwd_indexed_cl(store, torch.zeros(1, 3, dtype=torch.int64, device=DEV), rt, hypo, 4)
    with pytest.raises(RuntimeError, match="inconsistent"):
        ops.warp_agg_fwd_indexed_cl(store, [[0, 1]], rt, hypo, 4)


# ---- 7 + 8: the claim of the feature ------------------------------------------------------------------------------------
def _per_sample(model, sc, plan, r):
    imgs, proj, dv = SC.sample_of(sc, plan, r)
    out = model([torch.from_numpy(np.ascontiguousarray(i)).to(DEV) for i in imgs],
                {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in proj.items()}, torch.from_numpy(dv).to(DEV))
    return out["depth"][0].clone(), out["photometric_confidence"][0].clone()


@pytest.mark.parametrize("V,H,W,pairs", [(7, 128, 192, SC.PAIRS_7), (9, 512, 640, SC.ring_pairs(9, 4))])
def test_infer_scan_is_bit_equal_to_the_per_sample_forward(model, V, H, W, pairs):
    """depth and photometric_confidence of every reference view: zero differing elements against model(imgs, proj, dv) on
    the per-sample inputs, with in_flight 1 and 2, on the capturing call and on a replaying one.  Also the FPN run count:
    ceil(V / nviews) plan runs per scan, not one per reference view."""
    nviews = 5
    sc = SC.synthetic_scan(V, H, W, seed=V)
    plan = scan.plan_scan(sc["Ks"], sc["Es"], sc["depth_ranges"], pairs, nviews)
    R = len(plan.ref_views)
    assert R == sum(1 for _, s in pairs if s)
    want = [_per_sample(model, sc, plan, r) for r in range(R)]               # (eager on the first call, replayed after)
    want2 = _per_sample(model, sc, plan, R - 1)
    assert torch.equal(want2[0], want[R - 1][0]) and torch.equal(want2[1], want[R - 1][1])
    report = {}
    for in_flight in (1, 2):
        for call in ("capture", "replay"):
            res = scan.infer_scan(model, sc["images"], sc["Ks"], sc["Es"], sc["depth_ranges"], pairs, nviews=nviews,
                                  in_flight=in_flight)
            torch.cuda.synchronize()
            assert res["stats"]["captured"] == (call == "capture")
            assert res["stats"]["fpn_runs"] == math.ceil(V / nviews) and res["stats"]["replays"] == R
            assert res["depth"].shape == res["photometric_confidence"].shape == (R, H, W)
            assert np.array_equal(res["ref_views"], plan.ref_views)
            bad_d = sum(int((res["depth"][r] != want[r][0]).sum()) for r in range(R))
            bad_c = sum(int((res["photometric_confidence"][r] != want[r][1]).sum()) for r in range(R))
            report["in_flight%d_%s" % (in_flight, call)] = (bad_d, bad_c)
            print("infer_scan V=%d %dx%d in_flight=%d %s: differing depth %d, confidence %d of %d"
                  % (V, H, W, in_flight, call, bad_d, bad_c, R * H * W))
    assert all(v == (0, 0) for v in report.values()), report
    # output-resolution cameras: the stage-4 camera of the per-sample inputs
    assert np.array_equal(res["Ks"], plan.proj["stage4"][:, 1, :3, :3]) and np.array_equal(res["Es"], sc["Es"])
    assert np.array_equal(res["Ks"][:, :2], sc["Ks"][:, :2] * 4.0)


def test_infer_scan_float_images_and_other_outputs(model):
    """float32 [V,3,H,W] input (read_img's floats) gives the bits of the uint8 input; keep= names other outputs."""
    sc = SC.synthetic_scan(7, 128, 192, seed=7)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"], SC.PAIRS_7)
    a = scan.infer_scan(model, sc["images"], *args, keep=("depth", "photometric_confidence", "stage2.depth"))
    floats = np.ascontiguousarray((sc["images"].astype(np.float32) / 255.0).transpose(0, 3, 1, 2))
    b = scan.infer_scan(model, torch.from_numpy(floats).to(DEV), *args)
    assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["photometric_confidence"], b["photometric_confidence"])
    assert a["stage2.depth"].shape == (6, 128 // 4, 192 // 4)
    with pytest.raises(RuntimeError, match="not an entry"):
        scan.infer_scan(model, sc["images"], *args, keep=("depth", "no_such_map"))


# ---- 9: folder round trip into fusion -----------------------------------------------------------------------------------
def test_write_scan_outputs_then_filter_depth_equals_reconstruct_scan(model, tmp_path):
    """write_scan_outputs -> filter_depth on the folder against reconstruct_scan in memory: same masks and point positions
    bit for bit; colours too when fuse_scene is fed the JPEGs the folder path decodes."""
    Image = pytest.importorskip("PIL.Image")
    from mvster_amd import fusion
    V, H, W = 7, 128, 192
    sc = SC.synthetic_scan(V, H, W, seed=4)
    pairs = SC.ring_pairs(V, 4)
    src = SC.write_scan_folder(str(tmp_path), "scan9", sc, pairs)
    out = os.path.join(str(tmp_path), "out")
    conf, thres_view = 0.05, 1                                               # (random weights: keep the masks non-trivial)
    res = scan.infer_scan_folder(model, str(tmp_path), "scan9")
    scan.write_scan_outputs(res, res["images"], out)
    for sub, n in (("depth_est", "00000003.pfm"), ("confidence", "00000003.pfm"), ("cams", "00000003_cam.txt"), ("images", "00000003.jpg")):
        assert os.path.exists(os.path.join(out, sub, n))
    vertices = filter_depth(src, out, out, os.path.join(out, "fused.ply"), conf=conf, thres_view=thres_view)
    sf = scan.read_scan_folder(str(tmp_path), "scan9")
    mem = scan.reconstruct_scan(model, sf["images"], sf["Ks"], sf["Es"], sf["depth_ranges"], sf["pairs"], conf=conf,
                                thres_view=thres_view, plyfilename=os.path.join(out, "mem.ply"))
    assert torch.equal(mem.scan["depth"], res["depth"])
    mv = mem.vertices()
    print("points: folder %d, memory %d of %d pixels" % (len(vertices), len(mv), V * H * W))
    assert 0 < len(mv) < V * H * W
    for c in "xyz":
        assert np.array_equal(vertices[c], mv[c])
    for k in ("photo", "geo", "final"):
        m = mem[k + "_mask"].cpu().numpy()
        for i, r in enumerate(mem.scan["ref_views"]):
            png = np.array(Image.open(os.path.join(out, "mask", "{:0>8}_{}.png".format(r, k))))
            assert np.array_equal(png > 0, m[i])
    # colours: the same when fusion reads the re-encoded JPEGs, as the folder path does
    jpgs = [np.array(Image.open(os.path.join(out, "images", "{:0>8}.jpg".format(v))), dtype=np.uint8) for v in range(V)]
    again = fusion.fuse_scene(mem.scan["depth"], mem.scan["photometric_confidence"], jpgs, mem.scan["Ks"], mem.scan["Es"],
                              mem.scan["pairs"], conf, thres_view, device=DEV).vertices()
    assert np.array_equal(again, vertices)
    assert np.array_equal(fusion.read_ply(os.path.join(out, "mem.ply")), mv)


# ---- 10: timing ---------------------------------------------------------------------------------------------------------
def test_scan_inference_timing_report(model):
    """A 49-view 512x640 scan, 49 reference views, nviews = 5: infer_scan against the loop this path replaces --
    ``model(imgs, proj, dv)`` per sample through the forward's graph cache, inputs already on the device.  The loop has ONE
    captured forward per shape, so it cannot have two samples in flight: the assertion compares in_flight = 1 on both sides;
    the default in_flight = 2 is measured and reported.  Alternating A/B rounds in one process, HIP-event times, medians.
    Asserts only that the scan path is not slower (ratio >= 1.0): it removes 39 of 49 FPN runs and adds one ~3.5 kB copy
    per sample.  Figures go to $MVSTER_REPORT_DIR/scan_inference.json."""
    V, H, W, nviews, rounds = 49, 512, 640, 5, 4
    sc = SC.synthetic_scan(V, H, W, seed=49)
    pairs = SC.ring_pairs(V, 10)                                             # DTU: ten listed sources, four used
    plan = scan.plan_scan(sc["Ks"], sc["Es"], sc["depth_ranges"], pairs, nviews)
    R = len(plan.ref_views)
    u8 = torch.from_numpy(sc["images"]).to(DEV)
    # the loop's inputs, on the device: read_img's floats (NumPy's true division on the host; a device-side division by a
    # scalar may multiply by the reciprocal, which is not the same number for every level)
    floats = torch.from_numpy(np.ascontiguousarray((sc["images"].astype(np.float32) / 255.0).transpose(0, 3, 1, 2))).to(DEV)
    proj = {k: torch.from_numpy(v).to(DEV) for k, v in plan.proj.items()}
    dvs = torch.from_numpy(plan.depth_values).to(DEV)
    table = torch.from_numpy(plan.view_table.astype(np.int64)).to(DEV)
    samples = [([floats[v:v + 1] for v in plan.view_table[r]], {k: m[table[r]][None].contiguous() for k, m in proj.items()},
                dvs[r:r + 1]) for r in range(R)]
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        keep = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), keep

    def loop():
        return [model(*s)["depth"] for s in samples]

    def scan_path(in_flight, images=u8):
        return scan.infer_scan(model, images, sc["Ks"], sc["Es"], sc["depth_ranges"], pairs, nviews=nviews, in_flight=in_flight)

    loop(), loop()                                                           # eager, then captured
    t = {"loop": [], "scan_if1": [], "scan_if2": [], "scan_if2_host_u8": []}
    phases = []
    for k in (1, 2):
        scan_path(k)                                                         # capture
    for _ in range(rounds):
        t["loop"].append(timed(loop)[0])
        ms, res = timed(lambda: scan_path(1))
        t["scan_if1"].append(ms)
        t["loop"].append(timed(loop)[0])
        ms, res = timed(lambda: scan_path(2))
        t["scan_if2"].append(ms)
        phases.append(res.timings())
        t["scan_if2_host_u8"].append(timed(lambda: scan_path(2, sc["images"]))[0])   # + the 8-bit upload from pageable memory
    want = model(*samples[R - 1])
    assert torch.equal(res["depth"][R - 1], want["depth"][0])
    rec_ms, rec = timed(lambda: scan.reconstruct_scan(model, u8, sc["Ks"], sc["Es"], sc["depth_ranges"], pairs, conf=0.05,
                                                      thres_view=1, nviews=nviews))
    med = {k: statistics.median(v) for k, v in t.items()}
    report = {"scan": "%d views %dx%d, %d reference views, nviews %d" % (V, H, W, R, nviews), "rounds": rounds,
              "median_ms": med, "all_ms": t, "ratio_loop_over_scan_in_flight_1": med["loop"] / med["scan_if1"],
              "ratio_loop_over_scan_in_flight_2": med["loop"] / med["scan_if2"],
              "depth_maps_per_s": {k: 1000.0 * R / v for k, v in med.items()},
              "phase_ms_in_flight_2": {k: statistics.median(p[k] for p in phases) for k in phases[0]},
              "reconstruct_scan_ms": rec_ms, "reconstruct_scan_points": int(len(rec["points"])),
              "fpn_runs": res["stats"]["fpn_runs"], "store_bytes": res["stats"]["store_bytes"],
              "loop": "model(imgs, proj, dv) per sample through ForwardCache, inputs on the device, one sample in flight"}
    out = os.environ.get("MVSTER_REPORT_DIR") or os.path.join(ROOT, "build", "reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "scan_inference.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, sort_keys=True))
    assert report["ratio_loop_over_scan_in_flight_1"] >= 1.0, report
