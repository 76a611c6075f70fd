#!/usr/bin/env python3
"""Voxel-grid thinning of a fused cloud (``fusion.thin_points``) on the cloud that
scripts/fusion_dynamic_bench.py fuses (same synthetic scan, ``method="normal"``), at three voxel edges found by bisection so
that the mean occupancy (valid points per occupied voxel) is about 1, 4 and 16.

Timed per edge, the cloud already on the GPU:
  hip_mean / hip_first      ``thin_points`` in its two modes;
  torch_mean / torch_first  the tensor-level form a user would write on the same GPU: keys in torch,
                            ``torch.unique(return_inverse=True, return_counts=True)``, ``scatter_reduce`` / ``index_add_``, and an
                            argsort of the first indices to keep the cloud's order (float64 sums for the mean: not the same
                            bits as ``thin_points``, and not reproducible from run to run);
  numpy_mean                the NumPy restatement (tests/voxel_thin_cases.py) on the CPU, once.
Protocol: every form warmed up, then --runs windows; inside a window the four GPU forms alternate and each is called --reps
times between two device synchronises; a window's figure is its time per call, the report gives the median over the windows
with the lowest and highest window beside it.

End to end: ``scan.reconstruct_scan(..., plyfilename=...)`` on a DTU-sized synthetic scan (--scan-views views of 512 x 640, the
golden checkpoint) with and without ``voxel_size`` (the edge with occupancy about 4 on that scan's cloud), alternating,
host clock from the call to the closed file.  Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HALF = 1 << 20


def torch_keys(points, v):
    q = points.double() / float(np.float32(v))
    fi = torch.floor(q)
    valid = ((fi >= -HALF) & (fi < HALF)).all(1)
    i = fi[valid].long() + HALF
    return valid, (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2]


def thin_torch(points, colors, v, reduce):
    """The tensor-level form -> (points [U,3], colors [U,3], counts [U], first [U]) in the order of the first indices."""
    valid, key = torch_keys(points, v)
    idx = torch.nonzero(valid)[:, 0]
    uniq, inv, counts = torch.unique(key, return_inverse=True, return_counts=True)
    U = len(uniq)
    first = torch.full((U,), len(points), dtype=torch.int64, device=points.device).scatter_reduce(0, inv, idx, "amin")
    order = torch.argsort(first)
    first = first[order]
    if reduce == "first":
        return points[first], colors[first], counts[order], first
    sums = torch.zeros(U, 3, dtype=torch.float64, device=points.device).index_add_(0, inv, points[idx].double())
    csum = torch.zeros(U, 3, dtype=torch.int64, device=points.device).index_add_(0, inv, colors[idx].long())
    n = counts[:, None]
    return (sums / n)[order].float(), ((2 * csum + n) // (2 * n))[order].to(torch.uint8), counts[order], first


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "windows": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--sources", type=int, default=10)
    ap.add_argument("--conf", type=float, default=0.3)
    ap.add_argument("--thres-view", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7, help="timed windows per form")
    ap.add_argument("--reps", type=int, default=10, help="calls per window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scan-views", type=int, default=49)
    ap.add_argument("--scan-runs", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU time of the NumPy restatement")
    ap.add_argument("--no-scan", action="store_true", help="skip the end-to-end reconstruct_scan part")
    ap.add_argument("--out", default=os.path.join("profiles", "voxel_thin.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 windows")
    if not torch.cuda.is_available():
        sys.exit("voxel_thin_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import MVS4net, fusion, scan
    from mvster_amd.synthetic_scene import plane_depth_maps
    from tests import fusion_scene_cases as C
    from tests import scan_cases as SC
    from tests import voxel_thin_cases as T

    dev = torch.device("cuda:0")

    def occupancy(points, colors, v):
        r = fusion.thin_points(points, colors, v, "first")
        return (len(points) - r["dropped"]) / max(1, len(r["first"]))

    def edge_for(points, colors, target):
        """Bisection on log v for a mean occupancy within 3 % of `target` (of 1.03 for target 1: every edge below some size
        has occupancy 1, the one wanted is where sharing starts) -> (float32 edge, occupancy)."""
        goal = max(target, 1.03)
        p = points[torch.isfinite(points).all(1)]
        hi = float((p.max(0)[0] - p.min(0)[0]).max())
        lo = hi * 2.0 ** -19
        for _ in range(40):
            v = float(np.float32((lo * hi) ** 0.5))
            occ = occupancy(points, colors, v)
            if abs(occ / goal - 1) < 0.03:
                break
            lo, hi = (v, hi) if occ < goal else (lo, v)
        return v, occ

    V, H, W = args.views, args.height, args.width
    depths, Ks, Es = plane_depth_maps(V, H, W, seed=9, noise=1e-3, outlier_frac=0.1)
    rng = np.random.RandomState(4)
    conf = rng.rand(V, H, W).astype(np.float32)
    images = rng.randint(0, 256, (V, H, W, 3)).astype(np.uint8)
    pairs = C.make_pairs(V, args.sources, args.sources, seed=6)
    res = fusion.fuse_scene(*[torch.from_numpy(a).to(dev) for a in (depths, conf, images)], Ks, Es, pairs, args.conf,
                            args.thres_view)
    points, colors = res["points"], res["colors"]
    del res, depths, conf, images
    M = len(points)
    report = {"config": {"views": V, "height": H, "width": W, "sources": args.sources, "conf_thres": args.conf,
                         "thres_view": args.thres_view, "runs": args.runs, "reps": args.reps, "warmup": args.warmup,
                         "device": torch.cuda.get_device_name(0)},
              "points": M, "table_slots": fusion.thin_slots(M),
              "unit": "ms per call: host clock around --reps calls between two device synchronises, divided by --reps; "
                      "median over the windows, lowest and highest window beside it; the cloud is on the GPU",
              "edges": []}
    forms = {"hip_mean": lambda v: fusion.thin_points(points, colors, v, "mean"),
             "hip_first": lambda v: fusion.thin_points(points, colors, v, "first"),
             "torch_mean": lambda v: thin_torch(points, colors, v, "mean"),
             "torch_first": lambda v: thin_torch(points, colors, v, "first")}
    for target in (1.0, 4.0, 16.0):
        v, occ = edge_for(points, colors, target)
        for fn in forms.values():
            for _ in range(args.warmup):
                fn(v)
        times = {k: [] for k in forms}
        for _ in range(args.runs):
            for name, fn in forms.items():                          # alternating inside every window
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    out = fn(v)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / args.reps)
                del out
        hip, tor = forms["hip_first"](v), forms["torch_first"](v)
        same_first = bool(torch.equal(hip["first"], tor[3]) and torch.equal(hip["points"], tor[0]) and
                          torch.equal(hip["counts"].long(), tor[2]))
        U, dropped = len(hip["first"]), hip["dropped"]
        hipm, torm = forms["hip_mean"](v), forms["torch_mean"](v)
        entry = {"target_occupancy": target, "voxel_size": v, "occupancy": round(occ, 3), "voxels": U, "dropped": dropped,
                 "ms": {k: spread(x) for k, x in times.items()},
                 "torch_first_equals_hip_first": same_first,
                 "mean_position_max_abs_diff_hip_vs_torch_float64_mean": float((hipm["points"] - torm[0]).abs().max()),
                 "mean_position_bound_half_cell": v / 131072 + float(np.spacing(np.float32(points.abs().max().item()))),
                 "mean_colors_equal_torch": bool(torch.equal(hipm["colors"], torm[1])),
                 "output_bytes": U * 15, "input_bytes": M * 15}
        for mode in ("mean", "first"):
            entry["torch_over_hip_" + mode] = round(entry["ms"]["torch_" + mode]["median"] / entry["ms"]["hip_" + mode]["median"], 2)
        del hip, tor, hipm, torm
        if not args.no_cpu:
            pn, cn = points.cpu().numpy(), colors.cpu().numpy()
            t0 = time.perf_counter()
            want = T.thin_numpy(pn, cn, v, "mean")
            entry["numpy_mean_cpu_s"] = round(time.perf_counter() - t0, 3)
            got = forms["hip_mean"](v)
            entry["hip_mean_equals_numpy_bytes"] = bool(all(got[k].cpu().numpy().tobytes() == want[k].tobytes() for k in T.KEYS)
                                                        and got["dropped"] == want["dropped"])
            del pn, cn, want, got
        print(json.dumps(entry, sort_keys=True), flush=True)
        report["edges"].append(entry)
    del points, colors, forms
    torch.cuda.empty_cache()

    if not args.no_scan:
        cfg = dict(arch_mode="fpn", reg_net="reg2d", num_stage=4, fpn_base_channel=8, reg_channel=8, stage_splits=[8, 8, 4, 4],
                   depth_interals_ratio=[0.5, 0.5, 0.5, 1], group_cor=True, group_cor_dim=[8, 8, 4, 4], inverse_depth=True,
                   mono=True, attn_temp=2, attn_fuse_d=True)
        z = np.load(os.path.join(ROOT, "tests", "golden", "g7_checkpoint.npz"))
        model = MVS4net(**cfg)
        model.load_state_dict({k: torch.from_numpy(z[k]) for k in z.keys()}, strict=True)
        model = model.to(dev).eval()
        SV = args.scan_views
        sc = SC.synthetic_scan(SV, 512, 640, seed=49)
        spairs = SC.ring_pairs(SV, 10)
        u8 = torch.from_numpy(sc["images"]).to(dev)
        kw = dict(conf=0.05, thres_view=1, nviews=5)                # random weights: thresholds that keep a cloud
        sargs = (model, u8, sc["Ks"], sc["Es"], sc["depth_ranges"], spairs)
        full = scan.reconstruct_scan(*sargs, **kw)
        sv, socc = edge_for(full["points"], full["colors"], 4.0)
        n_full = len(full["points"])
        del full
        tmp = tempfile.mkdtemp()
        variants = {"full": {}, "thinned_mean": dict(voxel_size=sv, voxel_reduce="mean")}
        wall, sizes = {k: [] for k in variants}, {}
        for rnd in range(args.warmup + args.scan_runs):
            for name, extra in variants.items():                    # alternating
                ply = os.path.join(tmp, name + ".ply")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                scan.reconstruct_scan(*sargs, plyfilename=ply, **extra, **kw)
                dt = time.perf_counter() - t0
                if rnd >= args.warmup:
                    wall[name].append(dt * 1e3)
                sizes[name] = os.path.getsize(ply)
                os.remove(ply)
        os.rmdir(tmp)
        report["reconstruct_scan"] = {"scan": "%d views 512x640, %d reference views, nviews 5, 10 listed sources" % (SV, SV),
                                      "points": n_full, "voxel_size": sv, "occupancy": round(socc, 3),
                                      "ply_bytes": sizes, "wall_ms": {k: spread(x) for k, x in wall.items()},
                                      "unit": "ms, host clock from the call to the closed .ply (one call per window), file "
                                              "written to the machine's temporary directory"}
        print(json.dumps(report["reconstruct_scan"], sort_keys=True), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
