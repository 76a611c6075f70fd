#!/usr/bin/env python3
"""The DTU evaluation protocol on the GPU (``mvster_amd.dtu_eval``) at two sizes:

  surface_1m    1 M predicted points of the ``surface`` generator of scripts/cloud_score_bench.py (unit mean spacing, noise of
                half a spacing across the surface), dst = 2 spacings (a downsample factor of 4 .. 8), max_dist = 100 dst as on
                DTU (20 mm against 0.2 mm); the ground truth is another sample of the surface, reduced at dst like DTU's stl
                clouds; the mask covers the bounding box with a slab of voxels cleared, the plane cuts the lowest points off;
  surface_6m    the same with 6.1 M predicted points.

Timed per size, the clouds already on the GPU, between two HIP events around one call, warm, the median of --runs calls (at
least 5) with the lowest and the highest beside it:
  reduce_points            with its rounds, the points kept and the bytes it allocates at its peak; also on the other grid
                           (_cell_factor=1: cells of edge dst, 125 of them searched instead of 27 of edge 2 dst)
  thin_points_first        ``fusion.thin_points(..., reduce="first")`` at voxel_size = dst: for scale only, it computes something
                           else (one point per cell, survivors arbitrarily close across a cell face)
  evaluate_dtu_scan        with a reused ``DTUScanTruth``
  searches                 the reduced cloud's CloudGrid + ``nearest_distances`` both ways
  flags_and_stats          ``point_flags`` of the reduced cloud + ``distance_stats`` of both directions
Baseline: the NumPy / scipy.spatial.cKDTree restatement of the .m files on the CPU (the greedy loop over query_ball_point in
the same priority order, two cKDTree queries, the NumPy statistics), once, at surface_1m only, if scipy is there; the MATLAB
programs themselves cannot be run.  Writes one JSON file (--out)."""
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

DST = 2.0
MAX_DIST = 200.0


def cpu_restatement(pred, stl, mask, bb, res, plane, seed):
    """The .m files with cKDTree on the CPU -> (seconds per stage, kept points, mean_data, mean_stl)."""
    from scipy.spatial import cKDTree
    from tests import dtu_eval_cases as E
    t = {}
    t0 = time.perf_counter()
    p64 = pred.astype(np.float64)
    tree = cKDTree(p64)
    order = np.lexsort((np.arange(len(pred)), E.splitmix64_numpy(np.arange(len(pred)), seed)))
    keep = np.ones(len(pred), bool)
    for i in order:
        if keep[i]:
            keep[tree.query_ball_point(p64[i], DST)] = False
            keep[i] = True
    t["reduce_s"] = time.perf_counter() - t0
    q = pred[keep]
    t0 = time.perf_counter()
    dd = cKDTree(stl.astype(np.float64)).query(q.astype(np.float64), distance_upper_bound=MAX_DIST)[0]
    ds = cKDTree(q.astype(np.float64)).query(stl.astype(np.float64), distance_upper_bound=MAX_DIST)[0]
    t["searches_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    sd = E.stats_numpy(dd * dd, E.in_obs_mask_numpy(q, mask, bb, res) & E.covered_numpy(q, bb, 60.0), MAX_DIST)
    ss = E.stats_numpy(ds * ds, E.above_plane_numpy(stl, plane) & E.covered_numpy(stl, bb, 60.0), MAX_DIST)
    t["flags_and_stats_s"] = time.perf_counter() - t0
    t["total_s"] = sum(t.values())
    return {k: round(v, 3) for k, v in t.items()}, int(keep.sum()), sd, ss


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--large", type=int, default=6100000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join("profiles", "dtu_eval.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("dtu_eval_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import dtu_eval, fusion

    dev = torch.device("cuda:0")
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "dst": DST,
                         "max_dist": MAX_DIST, "rounds_per_batch": dtu_eval.ROUNDS_PER_BATCH},
              "unit": "ms between two HIP events around one call, warm; median over the runs, lowest and highest beside it; the "
                      "clouds are on the GPU",
              "not_measured": ["the cloud of reconstruct_scan on 49 views of 512 x 640", "the CPU restatement at surface_6m",
                               "a real DTU prediction of 10 .. 30 M points", "the MATLAB programs"],
              "sizes": []}
    for name, n, cpu in (("surface_1m", args.small, not args.no_cpu), ("surface_6m", args.large, False)):
        pred = surface(n, 1, dev)
        stl = dtu_eval.reduce_points(surface(n, 2, dev), DST)["points"].contiguous()
        lo, hi = pred.min(0)[0].cpu().numpy().astype(np.float64), pred.max(0)[0].cpu().numpy().astype(np.float64)
        res = 4.0
        bb1 = np.floor(lo) - 2 * res
        S = tuple(int(s) for s in np.ceil((hi - bb1) / res) + 3)
        mask = np.ones(S, np.uint8)
        mask[S[0] // 3:S[0] // 3 + 5] = 0
        bb = np.stack([bb1, bb1 + (np.array(S) - 1) * res])
        # (the block cover of MaxDistCP is in the protocol's millimetres: 60 is well inside this cloud, as on DTU)
        plane = np.array([0.0, 0.0, 1.0, 5.0])
        entry = {"name": name, "pred_points": n, "stl_points": len(stl), "mask_shape": S, "ms": {}}
        t, truth = event_ms(lambda: dtu_eval.DTUScanTruth(stl, mask, bb, res, plane, max_dist=MAX_DIST), 5, 1)
        entry["ms"]["DTUScanTruth"] = spread(t)
        entry["search_cell"] = truth.cell
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t, red = event_ms(lambda: dtu_eval.reduce_points(pred, DST), args.runs, args.warmup)
        entry["ms"]["reduce_points"] = spread(t)
        entry["reduce_peak_bytes"] = int(torch.cuda.max_memory_allocated() - before)
        entry["reduce_peak_bytes_per_point"] = round(entry["reduce_peak_bytes"] / n, 1)
        entry["rounds"], entry["kept"] = red["rounds"], len(red["index"])
        entry["downsample_factor"] = round(n / len(red["index"]), 3)
        t, other = event_ms(lambda: dtu_eval.reduce_points(pred, DST, _cell_factor=1), args.runs, args.warmup)
        entry["ms"]["reduce_points_cell_factor_1"] = spread(t)
        entry["same_keep_at_cell_factor_1"] = bool(torch.equal(other["keep"], red["keep"]))
        del other
        colors = torch.zeros(n, 3, device=dev, dtype=torch.uint8)
        t, thin = event_ms(lambda: fusion.thin_points(pred, colors, DST, "first"), args.runs, args.warmup)
        entry["ms"]["thin_points_first"] = spread(t)
        entry["thin_points_kept"] = len(thin["first"])
        del thin, colors
        t, out = event_ms(lambda: dtu_eval.evaluate_dtu_scan(pred, truth, DST), args.runs, args.warmup)
        entry["ms"]["evaluate_dtu_scan"] = spread(t)
        entry["result"] = out
        q = red["points"].contiguous()

        def searches():
            g = fusion.CloudGrid(q, truth.cell)
            return fusion.nearest_distances(g, truth.grid, MAX_DIST), fusion.nearest_distances(truth.grid, g, MAX_DIST)
        t, (data, back) = event_ms(searches, args.runs, args.warmup)
        entry["ms"]["searches"] = spread(t)

        def flags_and_stats():
            f, _ = truth.point_flags(q, dtu_eval.IN_MASK | dtu_eval.COVERED)
            return (dtu_eval.distance_stats(data["dist2"], (f & 5) == 5, MAX_DIST),
                    dtu_eval.distance_stats(back["dist2"], (truth.flags & 6) == 6, MAX_DIST))
        t, _ = event_ms(flags_and_stats, args.runs, args.warmup)
        entry["ms"]["flags_and_stats"] = spread(t)
        total = entry["ms"]["evaluate_dtu_scan"]["median"]
        entry["share_of_evaluate_dtu_scan"] = {k: round(entry["ms"][k]["median"] / total, 3)
                                               for k in ("reduce_points", "searches", "flags_and_stats")}
        entry["reduce_over_thin_points_first"] = round(entry["ms"]["reduce_points"]["median"] / entry["ms"]["thin_points_first"]["median"], 2)
        if cpu:
            try:
                import scipy  # noqa: F401
                have = True
            except ImportError:
                have = False
            if have:
                secs, kept, sd, ss = cpu_restatement(pred.cpu().numpy(), stl.cpu().numpy(), mask, bb, res, plane, 0)
                entry["cpu_restatement"] = dict(secs, kept=kept, n_data=sd["n"], mean_data=sd["mean"], n_stl=ss["n"], mean_stl=ss["mean"],
                                                same_kept=kept == entry["kept"], same_n=[sd["n"] == out["n_data"], ss["n"] == out["n_stl"]])
                entry["cpu_over_gpu"] = round(secs["total_s"] * 1000 / total, 1)
        print(json.dumps(entry, sort_keys=True), flush=True)
        report["sizes"].append(entry)
        del truth, red, data, back, pred, stl, q
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
