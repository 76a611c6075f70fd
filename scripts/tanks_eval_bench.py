#!/usr/bin/env python3
"""The Tanks and Temples evaluation protocol on the GPU (``mvster_amd.tanks_eval``) at two sizes:

  surface_1m    the ground truth is 1 M points of the ``surface`` generator of scripts/cloud_score_bench.py (unit mean spacing,
                noise of half a spacing across the surface), the prediction another 1 M sample of it moved by the inverse of a
                small similarity (0.4 degrees, scale 1.002, a shift of 3 spacings), which the three ICP rounds have to find;
                tau = 2 spacings; the crop volume is an octagon over the middle of the surface;
  surface_6m    the same with 6.1 M points each.

Timed per size, the clouds already on the GPU, between two HIP events around one call, warm, the median of --runs calls (at
least 5) with the lowest and the highest beside it:
  TanksSceneTruth          the ground truth's crop (its thinnings and grids are made by the first evaluate_scene and reused)
  crop_points              the prediction moved and cropped
  thin_points_tau, _half   the cropped prediction thinned at tau and at tau / 2
  registration_sums_r1/r3  one evaluation of an ICP iteration (move, bin, search, sums, the read-back of 18 doubles) on the
                           clouds of round 1 (thinned at tau, threshold 80 tau) and of round 3 (unthinned, 2 tau)
  register_clouds_r1       the whole first round
  distance_histogram       the 499 bins of one direction
  evaluate_scene           with a reused truth: refine=True, and refine=False from the known similarity
Baseline: the NumPy + scipy.spatial.cKDTree restatement of tests/tanks_eval_cases.py on the CPU (one thread), at surface_1m
only unless --cpu-large, --cpu-rounds times, alternating with the GPU's timed calls; Open3D itself cannot be run.  Writes one
JSON file (--out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scripts.cloud_score_bench import event_ms, spread, surface  # noqa: E402

TAU = 2.0
PLOT_STRETCH = 5


def cpu_restatement(pred, gt, vol, G_none=None):
    """tests/tanks_eval_cases.evaluate_numpy with cKDTree for the last two searches too (its brute force is for test sizes)
    -> (seconds per stage, result)."""
    from scipy.spatial import cKDTree
    from tests import tanks_eval_cases as T
    t, rounds = {}, []
    t0 = time.perf_counter()
    gtc = T.crop_numpy(gt, vol)["points"]
    t["crop_truth_s"] = time.perf_counter() - t0
    M = np.eye(4)
    t["crop_s"] = t["thin_s"] = t["icp_s"] = 0.0
    for voxel_over_tau, thr in T.ICP_ROUNDS:
        t0 = time.perf_counter()
        s = T.crop_numpy(pred, vol, M)["points"]
        t["crop_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        g = gtc
        if voxel_over_tau is not None:
            s, g = T.thin_numpy(s, voxel_over_tau * TAU), T.thin_numpy(gtc, voxel_over_tau * TAU)
        else:
            k = int(round(len(s) / 4e6)) if len(s) > 4e6 else 1
            s = s[::k]
            k = int(round(len(g) / 4e6)) if len(g) > 4e6 else 1
            g = g[::k]
        t["thin_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        reg = T.icp_numpy(s, g, thr * TAU, max_iteration=20)
        t["icp_s"] += time.perf_counter() - t0
        M = reg["transformation"] @ M
        rounds.append(dict(iterations=reg["iterations"], converged=reg["converged"], fitness=reg["fitness"],
                           inlier_rmse=reg["inlier_rmse"], source_points=len(s), target_points=len(g)))
    t0 = time.perf_counter()
    s, g = T.thin_numpy(T.crop_numpy(pred, vol, M)["points"], 0.5 * TAU), T.thin_numpy(gtc, 0.5 * TAU)
    t["final_crop_thin_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    md = T.f32(PLOT_STRETCH * TAU)
    dp = cKDTree(g.astype(np.float64)).query(s.astype(np.float64), distance_upper_bound=md)[0].astype(np.float32)
    dg = cKDTree(s.astype(np.float64)).query(g.astype(np.float64), distance_upper_bound=md)[0].astype(np.float32)
    edges = np.arange(0, TAU * PLOT_STRETCH, TAU / 100.0)
    hp, hg = np.histogram(dp, edges)[0], np.histogram(dg, edges)[0]
    t["final_searches_s"] = time.perf_counter() - t0
    t["total_s"] = sum(t.values())
    P, R = float((dp < np.float32(TAU)).sum()) / len(s), float((dg < np.float32(TAU)).sum()) / len(g)
    return ({k: round(v, 3) for k, v in t.items()},
            dict(precision=P, recall=R, fscore=2 * P * R / (P + R), transformation=M, rounds=rounds, pred_thinned=len(s),
                 gt_thinned=len(g), hist_sum=[int(hp.sum()), int(hg.sum())]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--large", type=int, default=6100000)
    ap.add_argument("--cpu-rounds", type=int, default=2, help="times the CPU restatement runs, alternating with the GPU (0: never)")
    ap.add_argument("--cpu-large", action="store_true", help="run the CPU restatement at the large size too")
    ap.add_argument("--out", default=os.path.join("profiles", "tanks_eval.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("tanks_eval_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import tanks_eval as E
    from tests import tanks_eval_cases as T

    dev = torch.device("cuda:0")
    G = T.similarity((0.2, -0.3, 0.93), 0.4, 1.002, (3.0, -2.0, 1.0))
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "tau": TAU,
                         "plot_stretch": PLOT_STRETCH, "similarity": G.tolist(), "cpu_rounds": args.cpu_rounds},
              "unit": "ms between two HIP events around one call, warm; median over the runs, lowest and highest beside it; the "
                      "clouds are on the GPU; the CPU restatement in seconds of one thread, each of its runs between two groups "
                      "of the GPU's",
              "not_measured": ["Open3D and the benchmark's own toolbox (not installed)", "a real scene of 10 .. 60 M points",
                               "the fused cloud of reconstruct_scan on a Tanks and Temples scan"], "sizes": []}
    if not args.cpu_large:
        report["not_measured"].append("the CPU restatement at surface_6m")
    for name, n, cpu in (("surface_1m", args.small, args.cpu_rounds > 0), ("surface_6m", args.large, args.cpu_rounds > 0 and args.cpu_large)):
        side = float(n) ** 0.5
        gt = surface(n, 2, dev)
        Gi = torch.from_numpy(np.linalg.inv(G)).to(dev)
        pred = (surface(n, 1, dev).double() @ Gi[:3, :3].T + Gi[:3, 3]).float().contiguous()
        c, r = side / 2, 0.46 * side
        th = 2 * np.pi * (np.arange(8) + 0.5) / 8
        vol = T.volume("Z", np.stack([c + r * np.cos(th), c + r * np.sin(th)], 1), -40.0, 40.0)
        volume = E.CropVolume(vol["orthogonal_axis"], vol["axis_min"], vol["axis_max"], vol["polygon"])
        entry = {"name": name, "points": n, "ms": {}}
        ms = entry["ms"]

        def gpu_group():
            t, truth = event_ms(lambda: E.TanksSceneTruth(gt, volume, TAU), args.runs, args.warmup)
            ms.setdefault("TanksSceneTruth", []).extend(t)
            t, crop = event_ms(lambda: E.crop_points(pred, volume, transform=G), args.runs, args.warmup)
            ms.setdefault("crop_points", []).extend(t)
            cropped = crop["points"]
            zeros = torch.zeros(cropped.shape[0], 3, device=dev, dtype=torch.uint8)
            from mvster_amd import fusion
            t, thin1 = event_ms(lambda: fusion.thin_points(cropped, zeros, TAU, "mean"), args.runs, args.warmup)
            ms.setdefault("thin_points_tau", []).extend(t)
            t, thin2 = event_ms(lambda: fusion.thin_points(cropped, zeros, 0.5 * TAU, "mean"), args.runs, args.warmup)
            ms.setdefault("thin_points_half", []).extend(t)
            entry.update(pred_cropped=crop["kept"], pred_thinned_tau=thin1["points"].shape[0], pred_thinned_half=thin2["points"].shape[0])
            # round 1 and round 3 from the uncorrected prediction: what the first iteration of each sees
            raw = E.crop_points(pred, volume)["points"]
            s1 = E._thin(raw, TAU)
            g1, g3 = truth.level(1.0, 80 * TAU), truth.level(None, 2 * TAU)
            t, _ = event_ms(lambda: E.registration_sums(s1, g1, 80 * TAU), args.runs, args.warmup)
            ms.setdefault("registration_sums_r1", []).extend(t)
            s3 = E._round3_stride(cropped)
            t, _ = event_ms(lambda: E.registration_sums(s3, g3, 2 * TAU), args.runs, args.warmup)
            ms.setdefault("registration_sums_r3", []).extend(t)
            t, reg = event_ms(lambda: E.register_clouds(s1, g1, 80 * TAU, max_iteration=20), args.runs, args.warmup)
            ms.setdefault("register_clouds_r1", []).extend(t)
            entry["register_clouds_r1_iterations"] = reg["iterations"]
            t, out = event_ms(lambda: E.evaluate_scene(pred, truth), args.runs, args.warmup)
            ms.setdefault("evaluate_scene", []).extend(t)
            t, fixed = event_ms(lambda: E.evaluate_scene(pred, truth, init_trans=G, refine=False), args.runs, args.warmup)
            ms.setdefault("evaluate_scene_no_refine", []).extend(t)
            from mvster_amd.fusion import CloudGrid, nearest_distances
            gtf = truth.level(0.5, PLOT_STRETCH * TAU)
            d = nearest_distances(CloudGrid(thin2["points"], gtf.cell), gtf, PLOT_STRETCH * TAU)["dist"]
            t, _ = event_ms(lambda: E.distance_histogram(d, out["edges"]), args.runs, args.warmup)
            ms.setdefault("distance_histogram", []).extend(t)
            return out, fixed

        cpu_runs = []
        out, fixed = gpu_group()
        if cpu:
            try:
                import scipy  # noqa: F401
            except ImportError:
                cpu = False
        if cpu:
            pred_h, gt_h = pred.cpu().numpy(), gt.cpu().numpy()
            for _ in range(args.cpu_rounds):
                secs, res = cpu_restatement(pred_h, gt_h, vol)
                cpu_runs.append(secs)
                out, fixed = gpu_group()                                     # alternate: a GPU group after every CPU run
        entry["ms"] = {k: spread(v) for k, v in ms.items()}
        entry["result"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in out.items()
                           if k not in ("edges", "cum_source", "cum_target")}
        entry["result_no_refine"] = {k: fixed[k] for k in ("precision", "recall", "fscore")}
        entry["transformation_error"] = float(np.abs(out["transformation"] - G).max())
        if cpu_runs:
            total = sorted(c["total_s"] for c in cpu_runs)[len(cpu_runs) // 2]
            entry["cpu_restatement"] = dict(runs=cpu_runs, precision=res["precision"], recall=res["recall"], fscore=res["fscore"],
                                            rounds=res["rounds"], pred_thinned=res["pred_thinned"], gt_thinned=res["gt_thinned"],
                                            transformation_error=float(np.abs(res["transformation"] - G).max()),
                                            same_counts=[res["pred_thinned"] == out["pred_thinned"], res["gt_thinned"] == out["gt_thinned"]],
                                            fscore_difference=abs(res["fscore"] - out["fscore"]))
            entry["cpu_over_gpu"] = round(total * 1000 / entry["ms"]["evaluate_scene"]["median"], 1)
        print(json.dumps(entry, sort_keys=True), flush=True)
        report["sizes"].append(entry)
        del gt, pred
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
