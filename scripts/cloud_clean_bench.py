#!/usr/bin/env python3
"""Cleaning a fused cloud (``fusion.nearest_neighbors`` / ``radius_outliers`` / ``statistical_outliers`` / ``estimate_normals``,
DESIGN.md section 4.20) at two sizes and three k:

  surface_1m    1 M points sampled from a synthetic surface (a wavy height field with unit mean spacing, noise of half a spacing
                across it), max_dist = 4 spacings (about 50 points), radius filter: 2 spacings, 8 neighbours;
  surface_6m    the same with 6.1 M points;
  scan          ``scan.reconstruct_scan`` of a 49-view 512 x 640 synthetic scan (the golden checkpoint) to a .ply, without the
                keywords, with ``outliers=StatisticalOutliers(20, 2, 6 s)`` and ``normals=Normals(20, 6 s)`` (s = the median
                distance to the nearest other point), and with both and a ``voxel_size``.

Timed per size and k in (8, 20, 32), the cloud already on the GPU, between two HIP events around one call, warm, the median of
--runs calls (at least 5) with the lowest and the highest beside it:
  grid_build              ``CloudGrid(points, cell)``, the part every operation below shares when it is given a tensor
  nearest_neighbors       the [M,k] lists, exclude_self, on the reused grid
  statistical_outliers    on the reused grid: search, statistics, flags, compaction, one read-back
  estimate_normals        on the reused grid, toward one position
  radius_outliers         on the reused grid (no k)
Baselines on the CPU, once each, if scipy is there: ``scipy.spatial.cKDTree`` (build, ``query`` with k + 1 and
distance_upper_bound, ``query_ball_point(return_length=True)``, with --workers threads) and, for the normals, NumPy's batched
``eigh`` on top of the tree's lists; their disagreement with the exact results is reported.  Writes one JSON file (--out)."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
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


def kernel_resources():
    """VGPRs / LDS / scratch of the kernels of geo_knn.hip from the compiler's report, or None without hipcc."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "mvster_amd", "csrc", "geo_knn.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            sym = m.group(1)
            k = re.search(r"knn_kernelILi(\d+)ELi(\d+)ELi(\d)E", sym)
            o = re.search(r"\d+(radius_count|stat_partial|stat_finish|keep_flags|keep_tail)_kernel", sym)
            name = ("knn_kernel<%s, %s, %s>" % (k.group(1), k.group(2), ("lists", "mean", "normals")[int(k.group(3))]) if k else
                    o.group(1) + "_kernel" if o else None)
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--large", type=int, default=6100000)
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 20, 32])
    ap.add_argument("--scan-views", type=int, default=49)
    ap.add_argument("--workers", type=int, default=16, help="threads of the cKDTree queries")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU times of scipy's cKDTree")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "cloud_clean.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("cloud_clean_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import MVS4net, fusion, scan

    dev = torch.device("cuda:0")
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cpu_workers": args.workers},
              "unit": "ms between two HIP events around one call, warm; median over the runs, lowest and highest beside it; the "
                      "cloud is on the GPU; CPU baselines in seconds of wall clock, once",
              "launches": {"grid_build": 9, "nearest_neighbors": 1, "estimate_normals": 1, "radius_outliers": 5,
                           "statistical_outliers": 10,
                           "note": "on a reused grid: the search 1; mvster_cloud_knn_stats 4; mvster_cloud_keep_flags 2 (radius) or 3; "
                                   "mvster_reg_crop_emit 1; a grid is mvster_voxel_thin_insert 4 + mvster_cloud_grid_build 5"},
              "kernel_resources": kernel_resources(), "sizes": []}
    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")

    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if args.no_cpu:
        cKDTree = None

    def measure(name, points, md, radius, nb_points):
        M = len(points)
        c4 = float(np.float32(md / 4))
        entry = {"name": name, "points": M, "max_dist": md, "radius": radius, "nb_points": nb_points, "ms": {}, "cpu_s": {}}
        t, grid = event_ms(lambda: fusion.CloudGrid(points, c4), args.runs, args.warmup)
        entry["ms"]["grid_build"] = spread(t)
        entry["cells"], entry["points_per_cell"] = grid.ncells, round((M - grid.dropped) / max(1, grid.ncells), 2)
        toward = torch.zeros_like(points)
        toward[:, 2] = 1000.0
        rgrid = fusion.CloudGrid(points, float(np.float32(radius / 4)))
        t, rad = event_ms(lambda: fusion.radius_outliers(rgrid, radius, nb_points), args.runs, args.warmup)
        entry["ms"]["radius_outliers"] = spread(t)
        entry["radius_kept"] = len(rad["index"])
        tree = pn = None
        if cKDTree is not None:
            pn = points.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(pn)
            entry["cpu_s"]["ckdtree_build"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            cnt = tree.query_ball_point(pn, radius, workers=args.workers, return_length=True) - 1
            entry["cpu_s"]["radius_outliers"] = round(time.perf_counter() - t0 + entry["cpu_s"]["ckdtree_build"], 3)
            entry["radius_counts_that_differ_from_scipy"] = int((cnt != rad["neighbours"].cpu().numpy()).sum())
            del cnt
        del rgrid, rad
        for k in args.ks:
            row = {}
            t, lists = event_ms(lambda: fusion.nearest_neighbors(grid, grid, k, md, exclude_self=True), args.runs, args.warmup)
            row["nearest_neighbors"] = spread(t)
            row["full_lists"] = int((lists["count"] == k).sum())
            t, stat = event_ms(lambda: fusion.statistical_outliers(grid, k, 2.0, md), args.runs, args.warmup)
            row["statistical_outliers"] = spread(t)
            row["statistical_kept"], row["statistical_n"] = len(stat["index"]), stat["n"]
            t, nrm = event_ms(lambda: fusion.estimate_normals(grid, k, md, toward=toward), args.runs, args.warmup)
            row["estimate_normals"] = spread(t)
            row["normals_valid"] = int(nrm["valid"].sum())
            if tree is not None:
                t0 = time.perf_counter()
                d, j = tree.query(pn, k=k + 1, distance_upper_bound=md, workers=args.workers)
                query_s = time.perf_counter() - t0
                cpu = {"nearest_neighbors": round(query_s + entry["cpu_s"]["ckdtree_build"], 3)}
                full = np.isfinite(d[:, k])
                kth = np.sqrt(lists["dist2"][:, k - 1].cpu().numpy())
                row["scipy_max_abs_diff_of_kth_dist"] = float(np.abs(d[full, k] - kth[full]).max()) if full.any() else None
                row["scipy_full_lists"] = int(full.sum())
                t0 = time.perf_counter()
                mean = d[:, 1:].sum(1) / k
                part = mean[full]
                thr = part.mean() + 2.0 * part.std(ddof=1)
                kept = full & (mean <= thr)
                cpu["statistical_outliers"] = round(time.perf_counter() - t0 + cpu["nearest_neighbors"], 3)
                row["scipy_statistical_kept"] = int(kept.sum())
                t0 = time.perf_counter()
                idx = np.where(np.isfinite(d[:, 1:]), j[:, 1:], np.arange(M)[:, None])       # a missing neighbour: the point itself
                e = pn[idx] - pn[:, None]
                m = np.isfinite(d[:, 1:]).sum(1, keepdims=True) + 1.0
                mu = e.sum(1) / m
                cov = np.einsum("mki,mkj->mij", e, e) / m[:, :, None] - mu[:, :, None] * mu[:, None, :]
                w, v = np.linalg.eigh(cov)
                n_cpu = v[:, :, 0]
                cpu["estimate_normals"] = round(time.perf_counter() - t0 + cpu["nearest_neighbors"], 3)
                ok = nrm["valid"].cpu().numpy() & ((w[:, 1] - w[:, 0]) > 1e-3 * w[:, 2])
                g = nrm["normals"].cpu().numpy().astype(np.float64)
                ang = np.arctan2(np.linalg.norm(np.cross(g[ok], n_cpu[ok]), axis=1), np.abs((g[ok] * n_cpu[ok]).sum(1)))
                row["scipy_eigh_max_angle_rad_where_gap_1e-3"] = float(ang.max()) if ok.any() else None
                row["cpu_s"] = cpu
                del d, j, idx, e, cov, w, v
            entry["ms"]["k%d" % k] = row
            del lists, stat, nrm
            print(json.dumps({name: {"k": k, **row}}, sort_keys=True), flush=True)
        print(json.dumps(entry, sort_keys=True), flush=True)
        report["sizes"].append(entry)
        save()                                                               # (a run cut short keeps what it measured)

    for name, n in (("surface_1m", args.small), ("surface_6m", args.large)):
        measure(name, surface(n, 1, dev), 4.0, 2.0, 8)
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
        images = torch.from_numpy(sc["images"]).to(dev)
        call = (model, images, sc["Ks"], sc["Es"], sc["depth_ranges"], SC.ring_pairs(SV, 10))
        kw = dict(conf=0.05, thres_view=1, nviews=5)                         # random weights: keep a cloud
        full = scan.reconstruct_scan(*call, **kw)
        points = full["points"]
        p = points[torch.isfinite(points).all(1)]
        extent = float((p.max(0)[0] - p.min(0)[0]).max())
        near = fusion.nearest_neighbors(points, points, 1, extent / 64, exclude_self=True)["dist2"][:, 0]
        s = float(near[torch.isfinite(near)].sqrt().median())
        md = float(np.float32(6 * s))
        entry = {"name": "scan", "scan": "%d views 512x640, nviews 5, 10 listed sources" % SV, "points": len(points),
                 "median_nearest_distance": s, "max_dist": md, "ms": {}}
        specs = {"plain": {},
                 "statistical_20_and_normals_20": dict(outliers=fusion.StatisticalOutliers(20, 2.0, md), normals=fusion.Normals(20, md)),
                 "voxel_and_statistical_20_and_normals_20": dict(voxel_size=float(np.float32(2 * s)),
                                                                  outliers=fusion.StatisticalOutliers(20, 2.0, md),
                                                                  normals=fusion.Normals(20, md))}
        with tempfile.TemporaryDirectory() as tmp:
            for label, spec in specs.items():
                ply = os.path.join(tmp, label + ".ply")

                def run():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = scan.reconstruct_scan(*call, plyfilename=ply, **spec, **kw)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3, res
                run()
                times = []
                for _ in range(args.runs):
                    ms, res = run()
                    times.append(ms)
                entry["ms"]["reconstruct_scan_to_ply_wall_" + label] = spread(times)
                entry["written_points_" + label] = len(res["final_points"]) if "final_points" in res else len(points)
                entry["ply_bytes_" + label] = os.path.getsize(ply)
        print(json.dumps(entry, sort_keys=True), flush=True)
        report["sizes"].append(entry)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
