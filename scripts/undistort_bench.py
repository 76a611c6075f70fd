#!/usr/bin/env python3
"""Undistortion of a scan's images (``mvster_amd.sfm.undistort_images``) on two synthetic sets, generated
from a seed:

  dtu     49 views of 1200 x 1600;
  photo   64 views of 3000 x 4000, worked through in chunks of --chunk-bytes of source.

All views share one OPENCV camera (k1, k2, p1, p2 = -0.25, 0.08, 0.002, -0.003 at a focal length of 0.875 widths).

Timed per set:
  kernel        ``mvster_undistort_images`` alone on the first chunk, its buffers already on the GPU: windows of as many
                back-to-back launches as fill --window seconds between two HIP events, warm, the median of --runs windows.  From
                it the achieved bytes per second, counting source + destination + mask bytes once each, as a share of the HBM
                peak; and beside it the rate of a plain device-to-device copy that moves the same number of bytes (half of them
                read, half written), timed the same way: the ceiling a memory-bound kernel can hope for.
  end to end    ``sfm.undistort_images`` by the wall clock, host arrays in and host arrays out (uploads, launches, read-backs),
                and with ``keep_on_device=True``.
  grid_sample   ``torch.nn.functional.grid_sample`` (bilinear, fp32) on the same GPU with the sample grid already there,
                including the conversion from and to bytes.  NOT exact: fp32 locations and blends; the bytes that differ from the
                kernel's are counted.
  scipy         ``scipy.ndimage.map_coordinates(order=1)`` on the CPU: 16 worker processes, one view each (locations in NumPy,
                three channels), before the GPU is touched -> views per second.

Writes one JSON file (--out).  Nothing is asserted about speed."""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12                         # bytes per second, MI355X (HBM3E, as specified)
SETS = {"dtu": (49, 1200, 1600), "photo": (64, 3000, 4000)}


def camera(H, W):
    f = 0.875 * W
    return np.array([4, W, H, f, f * 1.01, 0.502 * W, 0.497 * H, -0.25, 0.08, 0.002, -0.003, 0.0], dtype=np.float64)


def images_of(V, H, W, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(V)]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def locations(cam, ucam):
    """The definition in NumPy -> sx, sy [H',W']"""
    wn, hn = int(ucam[0]), int(ucam[1])
    x, y = np.meshgrid(np.arange(wn, dtype=np.float64), np.arange(hn, dtype=np.float64))
    u, v = (x + 0.5 - ucam[4]) / ucam[2], (y + 0.5 - ucam[5]) / ucam[3]
    k1, k2, p1, p2 = cam[7:11]
    r2 = u * u + v * v
    rad = 1.0 + r2 * (k1 + k2 * r2)
    ud, vd = u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u), v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
    return cam[3] * ud + cam[5] - 0.5, cam[4] * vd + cam[6] - 0.5


def _scipy_view(job):
    from scipy import ndimage
    img, cam, ucam = job
    sx, sy = locations(cam, ucam)
    inside = (sx >= 0) & (sx <= img.shape[1] - 1) & (sy >= 0) & (sy <= img.shape[0] - 1)
    out = np.zeros((sx.shape[0], sx.shape[1], 3), np.uint8)
    for k in range(3):
        val = ndimage.map_coordinates(img[..., k].astype(np.float64), [sy, sx], order=1, mode="nearest")
        out[..., k] = np.where(inside, np.floor(val + 0.5), 0)
    return int(out.sum() & 0xffff)


def _scipy_warm(k):
    from scipy import ndimage
    return float(ndimage.map_coordinates(np.eye(4), [[1.5], [1.5]], order=1)[0]) + k


def scipy_views_per_second(images, cam, ucam, workers=16):
    jobs = [(images[k % len(images)], cam, ucam) for k in range(workers)]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        pool.map(_scipy_warm, range(workers), chunksize=1)                      # (the workers are up and have imported scipy)
        t0 = time.perf_counter()
        pool.map(_scipy_view, jobs, chunksize=1)
        secs = time.perf_counter() - t0
    return workers / secs, secs


def window_ms(torch, fn, seconds, runs, warmup):
    """Milliseconds per call of ``fn``: windows of back-to-back calls between two events, each about ``seconds`` long"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(1, int(seconds * 1e3 / max(a.elapsed_time(b), 1e-3)))
    out = []
    for _ in range(runs):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out, reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort.json"))
    ap.add_argument("--sets", default="dtu,photo")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--no-cpu", action="store_true", help="skip the scipy side")
    ap.add_argument("--no-grid-sample", action="store_true")
    args = ap.parse_args()
    names = args.sets.split(",")
    sets = {n: images_of(*SETS[n], seed=len(n)) for n in names}
    cams = {n: camera(SETS[n][1], SETS[n][2]) for n in names}

    import torch
    from mvster_amd import _lib, sfm
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench.py measures on the GPU: there is none")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    report = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "chunk_bytes": args.chunk_bytes, "sets": {}}
    ucams = {}
    for n in names:
        ucams[n] = sfm.undistorted_cameras(cams[n][None], device=dev)
    for n in names:
        V, H, W = SETS[n]
        images, table, rows, ucam = sets[n], cams[n][None], np.zeros(V, np.int32), ucams[n]
        Hd, Wd = (int(s) for s in ucam["sizes"][0])
        entry = {"views": V, "source": [H, W], "undistorted": [Hd, Wd]}
        print("%s: %d views of %d x %d -> %d x %d" % (n, V, H, W, Hd, Wd), flush=True)
        # ---- the kernel alone, on the first chunk
        per = 3 * H * W
        first = max(1, min(V, args.chunk_bytes // per))
        kept, valid, _ = sfm.undistort_images(images[:first], table, rows[:first], cameras=ucam, chunk_bytes=args.chunk_bytes,
                                              keep_on_device=True, device=dev)
        views = np.zeros((first, 8), np.int64)
        r16 = lambda x: (x + 15) // 16 * 16
        for k in range(first):
            views[k] = (k * per, k * r16(3 * Hd * Wd), k * r16(Hd * Wd), H, W, Hd, Wd, 0)
        group_ptr = np.zeros(first + 1, np.int64)
        group_ptr[1:] = np.cumsum((views[:, 5] * views[:, 6] + 3) // 4)
        src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images[:first]])).to(dev)
        dst_bytes, valid_bytes = first * r16(3 * Hd * Wd), first * r16(Hd * Wd)
        out = torch.empty(dst_bytes + valid_bytes, device=dev, dtype=torch.uint8)
        tables = torch.from_numpy(np.concatenate([views.reshape(-1), group_ptr])).to(dev)
        cams_d, ucam_d = torch.from_numpy(table).to(dev), torch.from_numpy(ucam["table"]).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def launch():
            _lib.check(lib.mvster_undistort_images(src.data_ptr(), src.numel(), out.data_ptr(), dst_bytes, out.data_ptr() + dst_bytes,
                                                   valid_bytes, tables.data_ptr(), tables.data_ptr() + views.size * 8, first,
                                                   int(group_ptr[-1]), cams_d.data_ptr(), ucam_d.data_ptr(), 1, stream), "undistort_images")
        ms, reps = window_ms(torch, launch, args.window, args.runs, args.warmup)
        same = all(torch.equal(out[int(views[k, 1]):int(views[k, 1]) + 3 * Hd * Wd].view(Hd, Wd, 3), kept[k]) for k in (0, first - 1))
        moved = first * (per + 4 * Hd * Wd)                                     # source + destination + mask, once each
        half = torch.empty(moved // 2, device=dev, dtype=torch.uint8)
        other = torch.empty_like(half)
        copy_ms, copy_reps = window_ms(torch, lambda: other.copy_(half), args.window, args.runs, args.warmup)
        k_med, c_med = statistics.median(ms), statistics.median(copy_ms)
        entry["kernel"] = {"views": first, "ms": spread(ms), "launches_per_window": reps, "bytes": moved,
                           "bytes_per_s": round(moved / (k_med * 1e-3)), "share_of_hbm_peak": round(moved / (k_med * 1e-3) / HBM_PEAK, 4),
                           "megapixels_per_s": round(first * Hd * Wd / (k_med * 1e-3) / 1e6, 1), "equals_undistort_images": bool(same),
                           "copy_of_the_same_bytes": {"ms": spread(copy_ms), "launches_per_window": copy_reps,
                                                      "bytes_per_s": round(2 * half.numel() / (c_med * 1e-3)),
                                                      "share_of_hbm_peak": round(2 * half.numel() / (c_med * 1e-3) / HBM_PEAK, 4)},
                           "kernel_rate_over_copy_rate": round(c_med / k_med, 4), "valid_share": round(float(valid[0].float().mean()), 4)}
        print("  kernel: %s" % json.dumps(entry["kernel"]), flush=True)
        del half, other, src, out
        # ---- grid_sample, fp32, the grid already on the GPU
        if not args.no_grid_sample:
            F = torch.nn.functional
            sx, sy = (torch.from_numpy(a).to(dev) for a in locations(table[0], ucam["table"][0]))
            grid = torch.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], -1).float()[None]       # align_corners=False
            inside = ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1))[None, None]
            del sx, sy
            some = torch.from_numpy(np.stack(images[:min(first, 8)])).to(dev)

            def sample():
                x = some.permute(0, 3, 1, 2).float()
                y = F.grid_sample(x, grid.expand(len(some), -1, -1, -1), mode="bilinear", padding_mode="border", align_corners=False)
                return torch.where(inside, (y + 0.5).clamp_(0, 255), torch.zeros((), device=dev)).to(torch.uint8).permute(0, 2, 3, 1)
            gs_ms, gs_reps = window_ms(torch, sample, args.window, args.runs, args.warmup)
            got = sample()
            ref = torch.stack([kept[k] for k in range(len(some))])
            diff = (got.int() - ref.int()).abs()
            g_med = statistics.median(gs_ms)
            entry["grid_sample_fp32"] = {"views": len(some), "ms": spread(gs_ms), "launches_per_window": gs_reps,
                                         "megapixels_per_s": round(len(some) * Hd * Wd / (g_med * 1e-3) / 1e6, 1),
                                         "bytes_that_differ_from_the_kernel": int((diff > 0).sum()), "of_bytes": int(diff.numel()),
                                         "max_difference": int(diff.max()),
                                         "kernel_speedup_per_view": round((g_med / len(some)) / (k_med / first), 2)}
            print("  grid_sample: %s" % json.dumps(entry["grid_sample_fp32"]), flush=True)
            del some, grid, inside, got, ref, diff
        del kept, valid
        torch.cuda.empty_cache()
        # ---- end to end
        walls, walls_dev = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sfm.undistort_images(images, table, rows, cameras=ucam, chunk_bytes=args.chunk_bytes, device=dev)
            walls.append((time.perf_counter() - t0) * 1e3)
            del res
            t0 = time.perf_counter()
            res = sfm.undistort_images(images, table, rows, cameras=ucam, chunk_bytes=args.chunk_bytes, keep_on_device=True, device=dev)
            torch.cuda.synchronize()
            walls_dev.append((time.perf_counter() - t0) * 1e3)
            del res
        chunks = -(-V // first)
        entry["end_to_end"] = {"chunks": chunks, "host_in_host_out_wall_ms": spread(walls), "host_in_keep_on_device_wall_ms": spread(walls_dev),
                               "views_per_s_host_out": round(V / (statistics.median(walls) * 1e-3), 1),
                               "views_per_s_keep_on_device": round(V / (statistics.median(walls_dev) * 1e-3), 1)}
        print("  end to end: %s" % json.dumps(entry["end_to_end"]), flush=True)
        report["sets"][n] = entry
    # ---- scipy on the CPU: forked workers must not inherit an open GPU, so this side runs in a fresh interpreter
    if not args.no_cpu:
        import subprocess
        for n in names:
            code = ("import sys, json; sys.path.insert(0, %r); import numpy as np\n"
                    "from scripts import undistort_bench as B\n"
                    "V, H, W = B.SETS[%r]; ucam = np.array(%r)\n"
                    "r, s = B.scipy_views_per_second(B.images_of(2, H, W, 1), B.camera(H, W), ucam)\n"
                    "print(json.dumps([r, s]))\n" % (ROOT, n, [float(x) for x in ucams[n]["table"][0]]))
            rate, secs = json.loads(subprocess.check_output([sys.executable, "-c", code]).decode().strip().split("\n")[-1])
            e = report["sets"][n]
            e["scipy_cpu_16_processes"] = {"views_per_s": round(rate, 3), "seconds_for_16_views": round(secs, 3),
                                           "kernel_speedup": round((e["kernel"]["views"] / (e["kernel"]["ms"]["median"] * 1e-3)) / rate, 1),
                                           "end_to_end_speedup_host_out": round(e["end_to_end"]["views_per_s_host_out"] / rate, 1)}
            print("  %s scipy: %s" % (n, json.dumps(e["scipy_cpu_16_processes"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
