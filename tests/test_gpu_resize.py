"""The loader's input scaling on the GPU: ``ops.resize_pack_images_u8`` byte for byte against the host build of
csrc/resize_math.h, ``infer_scan`` / ``reconstruct_scan`` / ``write_scan_outputs`` with ``max_h`` / ``max_w`` against the
same path fed host-resized images and scaled intrinsics, and the timing report of the launch."""
import json
import os
import statistics

import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, filter_depth, formats, fusion, ops, scan
from tests import resize_cases as RC
from tests import scan_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(shipped_cfg, checkpoint):
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def hostmath():
    return RC.load_resize_hostmath(("g++", "clang++"))


# ---- the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_resize_pack_equals_the_host_build(hostmath, name, V):
    Hs, Ws, Hd, Wd, kind = RC.CASES[name]
    u8 = RC.case_images(name, V)
    want, want_u8 = RC.run_host(hostmath, u8, Hd, Wd, formats.resize_tables(Hs, Ws, Hd, Wd))
    dev = torch.from_numpy(u8).to(DEV)
    got, got_u8 = ops.resize_pack_images_u8(dev, Hd, Wd, want_u8=True)
    alone = ops.resize_pack_images_u8(dev, Hd, Wd)                           # the instantiation without the 8-bit output
    torch.cuda.synchronize()
    assert got.shape == (V, 1, Hd, Wd, 4) and got.dtype == torch.float32
    assert got_u8.shape == (V, Hd, Wd, 3) and got_u8.dtype == torch.uint8
    bad = int((got.cpu().numpy().view(np.int32) != want.view(np.int32)).sum())
    bad_u8 = int((got_u8.cpu().numpy() != want_u8).sum())
    print("resize_pack %s V=%d %dx%d -> %dx%d: differing float words %d, bytes %d" % (name, V, Hs, Ws, Hd, Wd, bad, bad_u8))
    assert bad == 0 and bad_u8 == 0
    assert torch.equal(alone, got)
    if kind == "constant":
        assert bool((got[0, 0, :, :, :3] == 1.0).all()) and bool((got_u8[0] == 255).all())
    if (Hs, Ws) == (Hd, Wd):
        assert torch.equal(got, ops.pack_images_u8(dev)) and torch.equal(got_u8, dev)


@pytest.mark.parametrize("V,H,W", [(1, 64, 64), (3, 128, 192), (2, 832, 1152)])
def test_identity_size_gives_the_bits_of_pack_images_u8(V, H, W):
    u8 = np.random.RandomState(H + V).randint(0, 256, size=(V, H, W, 3)).astype(np.uint8)
    u8[0, 0, :, 0] = np.arange(W) % 256                                      # every level
    dev = torch.from_numpy(u8).to(DEV)
    got, small = ops.resize_pack_images_u8(dev, H, W, want_u8=True)
    assert torch.equal(got, ops.pack_images_u8(dev)) and torch.equal(small, dev)


@pytest.mark.parametrize("Hs,Ws", [(128, 192), (130, 197)])
def test_every_source_route_gives_the_bits_of_the_host_build(hostmath, Hs, Ws):
    """A list of host views, a host ndarray stack, a CPU tensor stack, a GPU stack and the wrapper on the GPU stack.  Views of
    128 x 192 x 3 bytes are a multiple of 16 long: the stacks are taken as they lie (one flat upload, or read in place);
    those of 130 x 197 x 3 are not, and every route gathers them into the ragged buffer."""
    V, Hd, Wd = 3, 64, 128
    assert (Hs * Ws * 3 % 16 == 0) == ((Hs, Ws) == (128, 192))
    u8 = np.random.RandomState(Hs).randint(0, 256, size=(V, Hs, Ws, 3)).astype(np.uint8)
    want, want_u8 = RC.run_host(hostmath, u8, Hd, Wd, formats.resize_tables(Hs, Ws, Hd, Wd))
    dev = torch.from_numpy(u8).to(DEV)
    routes = {"list of host views": (ops.load_pack_images_u8, list(u8)), "host ndarray stack": (ops.load_pack_images_u8, u8),
              "CPU tensor stack": (ops.load_pack_images_u8, torch.from_numpy(u8)), "GPU stack": (ops.load_pack_images_u8, dev),
              "wrapper on the GPU stack": (ops.resize_pack_images_u8, dev)}
    first = None
    for name, (fn, images) in routes.items():
        got, got_u8 = fn(images, Hd, Wd, want_u8=True)
        alone = fn(images, Hd, Wd)
        torch.cuda.synchronize()
        bad = int((got.cpu().numpy().view(np.int32) != want.view(np.int32)).sum())
        bad_u8 = int((got_u8.cpu().numpy() != want_u8).sum())
        print("%s, %dx%d: differing float words %d, bytes %d" % (name, Hs, Ws, bad, bad_u8))
        assert bad == 0 and bad_u8 == 0, name
        first = first or (got, got_u8)
        assert torch.equal(got, first[0]) and torch.equal(alone, first[0]) and torch.equal(got_u8, first[1]), name


def test_resize_pack_rejects_what_the_loader_never_does():
    dev = torch.zeros(1, 128, 128, 3, dtype=torch.uint8, device=DEV)
    for Hd, Wd in ((256, 128), (128, 192), (100, 128), (0, 64)):
        with pytest.raises(RuntimeError, match="multiples of 64 and not larger"):
            ops.resize_pack_images_u8(dev, Hd, Wd)
    with pytest.raises(RuntimeError, match=r"uint8 \[V,H,W,3\]"):
        ops.resize_pack_images_u8(dev.float(), 64, 64)


# ---- through infer_scan ------------------------------------------------------------------------------------------------------
def _host_resized(sc, Hs, Ws, max_h, max_w):
    """What a caller without the feature would have to prepare: float32 [V,3,Hd,Wd] images and the scaled intrinsics."""
    Hd, Wd, scale_h, scale_w = formats.scale_input_size(Hs, Ws, max_h, max_w)
    floats = np.stack([formats.resize_linear(im.astype(np.float32) / 255.0, Hd, Wd).transpose(2, 0, 1) for im in sc["images"]])
    return Hd, Wd, np.ascontiguousarray(floats), formats.scale_intrinsics(sc["Ks"], scale_h, scale_w)


@pytest.mark.parametrize("V,Hs,Ws,max_h,max_w,size,pairs", [(7, 192, 320, 128, 256, (128, 192), SC.PAIRS_7),
                                                            (5, 1200, 1600, 864, 1152, (832, 1152), SC.ring_pairs(5, 4))])
def test_infer_scan_with_scaling_equals_infer_scan_on_host_resized_images(model, V, Hs, Ws, max_h, max_w, size, pairs):
    """depth and photometric_confidence: zero differing elements between infer_scan(uint8 images at their native size,
    max_h, max_w) and infer_scan(formats.resize_linear's float32 images, scaled intrinsics), on the capturing and on a
    replaying call."""
    sc = SC.synthetic_scan(V, Hs, Ws, seed=V)
    Hd, Wd, floats, Ks = _host_resized(sc, Hs, Ws, max_h, max_w)
    assert (Hd, Wd) == size
    args = (sc["Es"], sc["depth_ranges"], pairs)
    report = {}
    for call in ("capture", "replay"):
        got = scan.infer_scan(model, sc["images"], sc["Ks"], *args, max_h=max_h, max_w=max_w)
        assert got["stats"]["captured"] == (call == "capture")
        want = scan.infer_scan(model, torch.from_numpy(floats).to(DEV), Ks, *args)
        torch.cuda.synchronize()
        R = len(got["ref_views"])
        assert got["depth"].shape == want["depth"].shape == (R, Hd, Wd)
        bad_d = int((got["depth"] != want["depth"]).sum())
        bad_c = int((got["photometric_confidence"] != want["photometric_confidence"]).sum())
        report[call] = (bad_d, bad_c)
        print("infer_scan V=%d %dx%d -> %dx%d %s: differing depth %d, confidence %d of %d"
              % (V, Hs, Ws, Hd, Wd, call, bad_d, bad_c, R * Hd * Wd))
    assert all(v == (0, 0) for v in report.values()), report
    # the result carries the scaled cameras and the resized 8-bit images, the latter still on the device
    assert np.array_equal(got["Ks"], want["Ks"]) and np.array_equal(got["Ks"][:, :2], Ks[:, :2] * 4.0)
    assert torch.is_tensor(got["images"]) and got["images"].is_cuda and got["images"].shape == (V, Hd, Wd, 3)
    want_u8 = np.clip(floats.transpose(0, 2, 3, 1) * np.float32(255), 0, 255).astype(np.uint8)
    assert np.array_equal(got["images"].cpu().numpy(), want_u8)
    assert got["stats"]["source_bytes"] == V * Hs * Ws * 3 and got["stats"]["store_bytes"] == scan.store_bytes(V, Hd, Wd)
    # the other forms the images may come in: the same maps, prepared images, byte count and cameras
    for form, images in (("a list of views", list(sc["images"])), ("a GPU stack", torch.from_numpy(sc["images"]).to(DEV))):
        other = scan.infer_scan(model, images, sc["Ks"], *args, max_h=max_h, max_w=max_w)
        for k in ("depth", "photometric_confidence", "images"):
            assert torch.equal(other[k], got[k]), (form, k)
        assert other["stats"]["source_bytes"] == got["stats"]["source_bytes"] and np.array_equal(other["Ks"], got["Ks"]), form


def test_reconstruct_scan_and_folder_outputs_with_scaling(model, tmp_path):
    """reconstruct_scan with scaling: points and masks of fuse_scene on infer_scan's maps, colours = the kernel's 8-bit output
    at the surviving pixels.  infer_scan_folder -> write_scan_outputs -> filter_depth on the folder runs, and the written
    cameras hold the scaled intrinsics."""
    from PIL import Image
    V, Hs, Ws, max_h, max_w = 7, 192, 320, 128, 256
    conf, thres_view = 0.05, 1                                               # (random weights: keep the masks non-trivial)
    sc = SC.synthetic_scan(V, Hs, Ws, seed=V)
    pairs = SC.ring_pairs(V, 4)
    Hd, Wd, _, Ks = _host_resized(sc, Hs, Ws, max_h, max_w)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"], pairs)
    maps = scan.infer_scan(model, sc["images"], *args, max_h=max_h, max_w=max_w)
    packed, small = ops.resize_pack_images_u8(torch.from_numpy(sc["images"]).to(DEV), Hd, Wd, want_u8=True)
    assert torch.equal(maps["images"], small)
    want = fusion.fuse_scene(maps["depth"], maps["photometric_confidence"], small, maps["Ks"], maps["Es"], maps["pairs"], conf,
                             thres_view, device=DEV)
    got = scan.reconstruct_scan(model, sc["images"], *args, conf=conf, thres_view=thres_view, max_h=max_h, max_w=max_w)
    assert torch.equal(got.scan["depth"], maps["depth"])
    n = len(got["points"])
    print("reconstruct_scan with scaling: %d points of %d pixels" % (n, V * Hd * Wd))
    assert 0 < n < V * Hd * Wd
    assert torch.equal(got["points"], want["points"]) and torch.equal(got["colors"], want["colors"])
    for k in ("photo_mask", "geo_mask", "final_mask"):
        assert torch.equal(got[k], want[k])
    final = got["final_mask"].bool()
    assert final.shape == (V, Hd, Wd)
    assert torch.equal(got["colors"], small[final])                          # reference views in order, pixels row-major
    # the folder round trip
    src = SC.write_scan_folder(str(tmp_path), "scan", sc, pairs)
    out = os.path.join(str(tmp_path), "out")
    res = scan.infer_scan_folder(model, str(tmp_path), "scan", max_h=max_h, max_w=max_w)
    assert torch.is_tensor(res["images"]) and res["images"].shape == (V, Hd, Wd, 3)
    scan.write_scan_outputs(res, res["images"], out)
    decoded = scan.read_scan_folder(str(tmp_path), "scan")                   # (the JPEGs, not the arrays they were made from)
    want_small = ops.resize_pack_images_u8(torch.from_numpy(np.stack(decoded["images"])).to(DEV), Hd, Wd, want_u8=True)[1]
    assert torch.equal(res["images"], want_small)
    for v in range(V):
        name = "{:0>8}".format(v)
        K, E = formats.read_camera_parameters(os.path.join(out, "cams", name + "_cam.txt"))
        want_K = formats.scale_intrinsics(decoded["Ks"], *formats.scale_input_size(Hs, Ws, max_h, max_w)[2:])[v]
        want_K[:2] *= 4.0                                                    # the stage-4 camera
        assert np.array_equal(K, want_K) and np.array_equal(E, decoded["Es"][v])
        assert Image.open(os.path.join(out, "images", name + ".jpg")).size == (Wd, Hd)
        assert formats.read_pfm(os.path.join(out, "depth_est", name + ".pfm"))[0].shape == (Hd, Wd)
    vertices = filter_depth(src, out, out, os.path.join(out, "fused.ply"), conf=conf, thres_view=thres_view)
    print("filter_depth on the written folder: %d points" % len(vertices))
    assert 0 < len(vertices) < V * Hd * Wd


# ---- measurement (a report, not a gate) --------------------------------------------------------------------------------------
def _event_median_us(fn, reps=20):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return statistics.median(times), times


def test_scan_resize_timing_report(model):
    """49 views 1200x1600 -> 832x1152 (the DTU evaluation set within the reference's defaults): HIP-event medians of the
    resize_pack_images_u8 launch with and without the 8-bit output, beside pack_images_u8 on 49 views of 832x1152 (the
    like-for-like floor: the same bytes written); infer_scan end to end with scaling against infer_scan fed 832x1152 uint8
    images directly.  Figures go to $MVSTER_REPORT_DIR/scan_resize.json; nothing is asserted about them."""
    V, Hs, Ws, max_h, max_w, nviews, rounds = 49, 1200, 1600, 864, 1152, 5, 3
    Hd, Wd = formats.scale_input_size(Hs, Ws, max_h, max_w)[:2]
    rng = np.random.RandomState(49)
    big = torch.from_numpy(rng.randint(0, 256, size=(V, Hs, Ws, 3)).astype(np.uint8)).to(DEV)
    small = ops.resize_pack_images_u8(big, Hd, Wd, want_u8=True)[1]
    torch.cuda.synchronize()
    med = {}
    med["resize_pack_images_u8"], all_a = _event_median_us(lambda: ops.resize_pack_images_u8(big, Hd, Wd))
    med["resize_pack_images_u8_with_u8_output"], all_b = _event_median_us(lambda: ops.resize_pack_images_u8(big, Hd, Wd, want_u8=True))
    med["pack_images_u8_at_target_size"], all_c = _event_median_us(lambda: ops.pack_images_u8(small))
    n_out = V * Hd * Wd
    # bytes the algorithm needs: every source byte once (the taps of neighbouring pixels share cache lines), every output once
    moved = {"resize_pack_images_u8": V * Hs * Ws * 3 + n_out * 16,
             "resize_pack_images_u8_with_u8_output": V * Hs * Ws * 3 + n_out * 19,
             "pack_images_u8_at_target_size": n_out * 3 + n_out * 16}
    frac = {k: moved[k] / (med[k] * 1e-6) / 8e12 for k in med}

    # end to end: a synthetic scan at the native size, the same scan already at the target size
    sc = SC.synthetic_scan(V, Hd, Wd, seed=49)
    pairs = SC.ring_pairs(V, 10)
    args = (sc["Es"], sc["depth_ranges"], pairs)
    big_host = big.cpu().numpy()
    Ks_small = formats.scale_intrinsics(sc["Ks"], *formats.scale_input_size(Hs, Ws, max_h, max_w)[2:])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        keep = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), keep

    def scaled(images):
        return scan.infer_scan(model, images, sc["Ks"], *args, nviews=nviews, max_h=max_h, max_w=max_w)

    def direct(images):
        return scan.infer_scan(model, images, Ks_small, *args, nviews=nviews)

    small_host = small.cpu().numpy()
    scaled(big)                                                              # capture
    t = {"scaled_device_u8": [], "direct_device_u8": [], "scaled_host_u8": [], "direct_host_u8": []}
    phases = {"scaled_host_u8": [], "direct_host_u8": []}
    for _ in range(rounds):
        t["scaled_device_u8"].append(timed(lambda: scaled(big))[0])
        t["direct_device_u8"].append(timed(lambda: direct(small))[0])
        ms, res = timed(lambda: scaled(big_host))
        t["scaled_host_u8"].append(ms)
        phases["scaled_host_u8"].append(res.timings())
        ms, res2 = timed(lambda: direct(small_host))
        t["direct_host_u8"].append(ms)
        phases["direct_host_u8"].append(res2.timings())
    # (no comparison of the two results: the direct path starts from the resized images quantised to 8 bits, the scaled
    # one from their float values -- the like-for-like comparison is test_infer_scan_with_scaling_equals_...)
    assert res["depth"].shape == res2["depth"].shape == (len(res["ref_views"]), Hd, Wd)
    e2e = {k: statistics.median(v) for k, v in t.items()}
    report = {"case": "%d views %dx%d -> %dx%d" % (V, Hs, Ws, Hd, Wd), "launch_median_us": med,
              "launch_all_us": {"resize_pack_images_u8": all_a, "resize_pack_images_u8_with_u8_output": all_b,
                                "pack_images_u8_at_target_size": all_c},
              "bytes_moved": moved, "fraction_of_8TBps": frac,
              "ratio_resize_over_pack": med["resize_pack_images_u8"] / med["pack_images_u8_at_target_size"],
              "infer_scan": "%d reference views, nviews %d, in_flight 2" % (len(res["ref_views"]), nviews),
              "infer_scan_median_ms": e2e, "infer_scan_all_ms": t, "rounds": rounds,
              "infer_scan_phase_ms": {k: {p: statistics.median(x[p] for x in v) for p in v[0]} for k, v in phases.items()},
              "source_bytes": res["stats"]["source_bytes"], "store_bytes": res["stats"]["store_bytes"]}
    out = os.environ.get("MVSTER_REPORT_DIR") or os.path.join(ROOT, "build", "reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "scan_resize.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, sort_keys=True))
