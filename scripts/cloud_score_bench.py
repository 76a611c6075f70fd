#!/usr/bin/env python3
"""Cloud-to-cloud nearest distances and scan scores (``fusion.nearest_distances`` / ``CloudGrid`` / ``score_clouds``, DESIGN.md
section 4.17) at three sizes:

  surface_1m    1 M points against 1 M, both sampled from one synthetic surface (a wavy height field with unit mean spacing,
                noise of half a spacing across it), max_dist = 8 spacings;
  surface_6m    the same with 6.1 M against 6.1 M;
  scan          the cloud ``scan.reconstruct_scan`` makes of a 49-view 512 x 640 synthetic scan (the golden checkpoint) against
                its own thinned cloud (``thin_points``, "mean", about 4 points per voxel), max_dist = 2 voxel edges.

Timed per size, the clouds already on the GPU, between two HIP events around one call, warm, the median of --runs calls (at
least 5) with the lowest and the highest beside it:
  grid_build              ``CloudGrid(target, cell)``
  query_reused_grid       ``nearest_distances(query, grid, max_dist)``: binning the queries + the search
  nearest_distances       ``nearest_distances(query, target, max_dist)``: the two above in one call
  score_clouds            both ways + the reduction + the read-back
at the default cell (max_dist / 4) and, for nearest_distances, at the smallest (max_dist / 15) too.  Baselines:
  torch_cdist_min_fp32    chunked ``torch.cdist`` + ``min`` on the same GPU, what a user writes today: inexact (float32, the
                          matmul form), surface_1m only; its disagreement with the exact result is reported;
  scipy_ckdtree_cpu_s     ``scipy.spatial.cKDTree`` build + query with distance_upper_bound on the CPU, once, if scipy is there.
The launch counts are those of the code path (mvster_voxel_thin_insert 4, mvster_cloud_grid_build 5, mvster_cloud_nn_query 1,
mvster_cloud_score 2); VGPRs and scratch come from the compiler's report on geo_nn.hip when hipcc is on the machine.  Writes
one JSON file (--out)."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def event_ms(fn, runs, warmup):
    """-> (times in ms between two HIP events around one call each, the last result)."""
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times, out


def surface(n, seed, dev):
    """n points of a wavy height field with unit mean spacing and noise of half a spacing across it."""
    g = torch.Generator(device=dev).manual_seed(seed)
    side = float(n) ** 0.5
    xy = torch.rand(n, 2, device=dev, generator=g) * side
    z = 6.0 * torch.sin(xy[:, 0] / 40.0) * torch.cos(xy[:, 1] / 55.0) + 0.5 * torch.randn(n, device=dev, generator=g)
    return torch.cat([xy, z[:, None]], 1).contiguous()


def cdist_min(query, target, qchunk=4096, tchunk=262144):
    """What a user writes today: chunked torch.cdist + min in float32 -> (dist [Q], index [Q])."""
    best = torch.full((len(query),), float("inf"), device=query.device)
    index = torch.full((len(query),), -1, dtype=torch.int64, device=query.device)
    for q0 in range(0, len(query), qchunk):
        q = query[q0:q0 + qchunk]
        for t0 in range(0, len(target), tchunk):
            d, j = torch.cdist(q, target[t0:t0 + tchunk]).min(1)
            take = d < best[q0:q0 + qchunk]
            best[q0:q0 + qchunk] = torch.where(take, d, best[q0:q0 + qchunk])
            index[q0:q0 + qchunk] = torch.where(take, j + t0, index[q0:q0 + qchunk])
    return best, index


def kernel_resources():
    """VGPRs / scratch of the kernels of geo_nn.hip from the compiler's report, or None without hipcc."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "mvster_amd", "csrc", "geo_nn.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"(nn_\w+_kernel)", m.group(1))
            name = name.group(1) if name else None
            if name:
                out[name] = {}
        for key, label in (("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--large", type=int, default=6100000)
    ap.add_argument("--scan-views", type=int, default=49)
    ap.add_argument("--cdist-runs", type=int, default=5)
    ap.add_argument("--no-cdist", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU time of scipy's cKDTree")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "cloud_score.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("cloud_score_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import MVS4net, fusion, scan

    dev = torch.device("cuda:0")
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
              "unit": "ms between two HIP events around one call, warm; median over the runs, lowest and highest beside it; the "
                      "clouds are on the GPU",
              "launches": {"grid_build": 9, "query_reused_grid": 10, "nearest_distances": 19, "score_clouds": 24,
                           "note": "mvster_voxel_thin_insert 4 + mvster_cloud_grid_build 5 per cloud, mvster_cloud_nn_query 1 per "
                                   "way, mvster_cloud_score 2 per way; score_clouds builds each grid once and uses it both ways"},
              "kernel_resources": kernel_resources(), "sizes": []}

    def measure(name, query, target, md, tau, cdist, cpu):
        c4, c15 = float(np.float32(md / 4)), float(np.nextafter(np.float32(md / 15), np.float32(np.inf)))
        entry = {"name": name, "query_points": len(query), "target_points": len(target), "max_dist": md, "tau": tau, "ms": {}}
        t, grid = event_ms(lambda: fusion.CloudGrid(target, c4), args.runs, args.warmup)
        entry["ms"]["grid_build"] = spread(t)
        entry["target_cells"], entry["target_points_per_cell"] = grid.ncells, round((len(target) - grid.dropped) / max(1, grid.ncells), 2)
        t, reused = event_ms(lambda: fusion.nearest_distances(query, grid, md), args.runs, args.warmup)
        entry["ms"]["query_reused_grid"] = spread(t)
        t, out = event_ms(lambda: fusion.nearest_distances(query, target, md), args.runs, args.warmup)
        entry["ms"]["nearest_distances"] = spread(t)
        t, fine = event_ms(lambda: fusion.nearest_distances(query, target, md, cell=c15), args.runs, args.warmup)
        entry["ms"]["nearest_distances_cell_max_dist_15"] = spread(t)
        entry["same_bytes_reused_grid_and_fine_cell"] = bool(all(torch.equal(out[k].view(torch.uint8), o[k].view(torch.uint8))
                                                                 for o in (reused, fine) for k in ("dist", "dist2", "index")))
        t, score = event_ms(lambda: fusion.score_clouds(query, target, md, tau), args.runs, args.warmup)
        entry["ms"]["score_clouds"] = spread(t)
        entry["score"] = score
        entry["found"] = int((out["index"] >= 0).sum())
        entry["grid_build_share_of_nearest_distances"] = round(entry["ms"]["grid_build"]["median"] /
                                                               entry["ms"]["nearest_distances"]["median"], 3)
        del grid, reused, fine
        if cdist:
            t0 = time.perf_counter()
            base = cdist_min(query, target)
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            runs = args.cdist_runs if first < 6 else 2                      # a slow baseline is not run five times over
            t, base = event_ms(lambda: cdist_min(query, target), runs, 0)
            entry["ms"]["torch_cdist_min_fp32"] = spread(t)
            entry["cdist_over_nearest_distances"] = round(entry["ms"]["torch_cdist_min_fp32"]["median"] /
                                                          entry["ms"]["nearest_distances"]["median"], 1)
            ok = out["index"] >= 0
            entry["cdist_max_abs_diff_of_dist"] = float((base[0][ok] - out["dist"][ok]).abs().max())
            entry["cdist_other_index"] = int((base[1][ok] != out["index"][ok]).sum())
            del base
        if cpu:
            try:
                from scipy.spatial import cKDTree
            except ImportError:
                cKDTree = None
            if cKDTree is not None:
                qn, tn = query.cpu().numpy().astype(np.float64), target.cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                d, j = cKDTree(tn).query(qn, k=1, distance_upper_bound=md)
                entry["scipy_ckdtree_cpu_s"] = round(time.perf_counter() - t0, 3)
                ok = (out["index"] >= 0).cpu().numpy()
                entry["scipy_max_abs_diff_of_dist2_sqrt"] = float(np.abs(d[ok] - np.sqrt(out["dist2"].cpu().numpy()[ok])).max())
                entry["scipy_found"] = int(np.isfinite(d).sum())
        print(json.dumps(entry, sort_keys=True), flush=True)
        report["sizes"].append(entry)

    for name, n, cdist in (("surface_1m", args.small, not args.no_cdist), ("surface_6m", args.large, False)):
        measure(name, surface(n, 1, dev), surface(n, 2, dev), 8.0, 1.0, cdist, not args.no_cpu)
        torch.cuda.empty_cache()

    if not args.no_scan:
        from tests import scan_cases as SC
        cfg = dict(arch_mode="fpn", reg_net="reg2d", num_stage=4, fpn_base_channel=8, reg_channel=8, stage_splits=[8, 8, 4, 4],
                   depth_interals_ratio=[0.5, 0.5, 0.5, 1], group_cor=True, group_cor_dim=[8, 8, 4, 4], inverse_depth=True,
                   mono=True, attn_temp=2, attn_fuse_d=True)
        z = np.load(os.path.join(ROOT, "tests", "golden", "g7_checkpoint.npz"))
        model = MVS4net(**cfg)
        model.load_state_dict({k: torch.from_numpy(z[k]) for k in z.keys()}, strict=True)
        model = model.to(dev).eval()
        SV = args.scan_views
        sc = SC.synthetic_scan(SV, 512, 640, seed=49)
        full = scan.reconstruct_scan(model, torch.from_numpy(sc["images"]).to(dev), sc["Ks"], sc["Es"], sc["depth_ranges"],
                                     SC.ring_pairs(SV, 10), conf=0.05, thres_view=1, nviews=5)     # random weights: keep a cloud
        points, colors = full["points"], full["colors"]
        p = points[torch.isfinite(points).all(1)]
        lo = hi = float((p.max(0)[0] - p.min(0)[0]).max())
        lo *= 2.0 ** -19
        for _ in range(40):                                                  # the edge with about 4 points per voxel
            v = float(np.float32((lo * hi) ** 0.5))
            thin = fusion.thin_points(points, colors, v, "mean")
            occ = (len(points) - thin["dropped"]) / max(1, len(thin["first"]))
            if abs(occ / 4 - 1) < 0.03:
                break
            lo, hi = (v, hi) if occ < 4 else (lo, v)
        del model, full
        measure("scan", points, thin["points"], float(np.float32(2 * v)), float(np.float32(v / 2)), False, not args.no_cpu)
        report["sizes"][-1].update(scan="%d views 512x640, nviews 5, 10 listed sources" % SV, voxel_size=v, occupancy=round(occ, 3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
